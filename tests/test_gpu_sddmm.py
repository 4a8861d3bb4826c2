"""GPU: the sampled dense-dense product (voltrix.sddmm, sddmm_kernels.hpp) and the gradients it gives -- autograd.SDDMM in both
operands and autograd.SpMM(..., values=) in its edge values -- against float64 torch.

Oracle: ``(x.double()[rows] * y.double()[cols]).sum(1)``.  Integer operands are exact (bit for bit); random ones stay within
``F 2^-23 (|x| |y|)[e]`` (fp32 products and sum, one fused multiply-add per element)."""
import numpy as np
import pytest
import torch

import voltrix
from conftest import CSR_FIXTURES, load_csr_fixture
from test_hybrid_plan import _random_csr

pytestmark = pytest.mark.gpu

PAIRS = [(torch.float32, torch.float16), (torch.float32, torch.bfloat16), (torch.float16, torch.float16),
         (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32)]
WIDTHS = [8, 20, 40, 128, 512, 1000, 1001]


def _rows(indptr):
    return torch.repeat_interleave(torch.arange(indptr.numel() - 1, device=indptr.device), (indptr[1:] - indptr[:-1]).long())


def _oracle(indptr, indices, x, y):
    rows, cols = _rows(indptr), indices.long()
    ref = (x.double()[rows] * y.double()[cols]).sum(1)
    scale = (x.double().abs()[rows] * y.double().abs()[cols]).sum(1)
    return ref, scale


def _special_graph():
    """Rectangular (3000 x 2500): empty rows, one hub row of 20,500 edges, rows of length 1, short random rows, duplicate entries."""
    rng = np.random.default_rng(5)
    rows = []
    for r in range(3000):
        if r % 11 == 0:
            rows.append(np.zeros(0, np.int64))
        elif r == 1234:
            rows.append(np.sort(rng.integers(0, 2500, 20500)))
        elif r % 3 == 0:
            rows.append(rng.integers(0, 2500, 1))
        else:
            c = np.sort(rng.integers(0, 2500, rng.integers(1, 9)))
            rows.append(np.concatenate([c[:1], c]) if r % 7 == 1 else c)        # duplicates
    indptr = np.zeros(3001, np.int32)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return torch.from_numpy(indptr).cuda(), torch.from_numpy(np.concatenate(rows).astype(np.int32)).cuda(), 3000, 2500


def _operands(n, m, width, pair, integer, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if integer:
        x = torch.randint(-3, 4, (n, width), device="cuda", generator=g).to(pair[0])
        y = torch.randint(-3, 4, (m, width), device="cuda", generator=g).to(pair[1])
    else:
        x = torch.randn(n, width, device="cuda", generator=g).to(pair[0])
        y = torch.randn(m, width, device="cuda", generator=g).to(pair[1])
    return x, y


def _check(indptr, indices, x, y, out, integer):
    ref, scale = _oracle(indptr, indices, x, y)
    assert out.dtype == torch.float32 and out.shape == (indices.numel(),)
    if integer:
        assert torch.equal(out.double(), ref)
    else:
        assert ((out.double() - ref).abs() <= x.shape[1] * 2.0 ** -23 * scale).all()


@pytest.mark.parametrize("name", CSR_FIXTURES)
def test_golden_csr_fixtures(cuda_device, name):
    g = load_csr_fixture(name)
    indptr, indices = torch.from_numpy(g["indptr"]).cuda(), torch.from_numpy(g["indices"]).cuda()
    n = int(g["num_nodes"])
    for pair in PAIRS:
        for integer in (True, False):
            x, y = _operands(n, n, 128, pair, integer, seed=1)
            _check(indptr, indices, x, y, voltrix.sddmm(indptr, indices, x, y), integer)


def test_widths_and_pairs_on_hub_empty_short_duplicate_rows(cuda_device):
    indptr, indices, n, m = _special_graph()
    for width in WIDTHS:
        for pair in PAIRS:
            for integer in (True, False):
                x, y = _operands(n, m, width, pair, integer, seed=width)
                _check(indptr, indices, x, y, voltrix.sddmm(indptr, indices, x, y), integer)


def test_other_pairs_are_cast_and_nothing_to_do(cuda_device):
    indptr, indices, n, m = _special_graph()
    x, y = _operands(n, m, 40, (torch.float16, torch.float32), False, seed=3)
    _check(indptr, indices, x.float(), y, voltrix.sddmm(indptr, indices, x, y), False)
    x, y = _operands(n, m, 40, (torch.float16, torch.bfloat16), True, seed=3)
    _check(indptr, indices, x, y, voltrix.sddmm(indptr, indices, x, y), True)
    empty_ptr = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    out = voltrix.sddmm(empty_ptr, torch.zeros(0, dtype=torch.int32, device="cuda"), x, y)
    assert out.shape == (0,) and out.dtype == torch.float32


def test_determinism_duplicates_and_row_subsets(cuda_device):
    indptr, indices, n, m = _special_graph()
    ip_np = indptr.cpu().numpy()
    keep_np = np.unique(np.concatenate([np.arange(1, n, 3), [1234]]))     # every third row, the hub included
    edge = torch.from_numpy(np.concatenate([np.arange(ip_np[r], ip_np[r + 1]) for r in keep_np])).cuda()
    keep = torch.from_numpy(keep_np).cuda()
    sub_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(np.diff(ip_np)[keep_np])]).astype(np.int32)).cuda()
    for pair in PAIRS:
        for width in (40, 1000):
            x, y = _operands(n, m, width, pair, False, seed=7)
            a = voltrix.sddmm(indptr, indices, x, y)
            b = voltrix.sddmm(indptr, indices, x, y)
            assert torch.equal(a, b)
            # duplicates: the same (row, col) gives the same bits
            key = _rows(indptr) * m + indices.long()
            order = torch.argsort(key)
            same = key[order][1:] == key[order][:-1]
            assert int(same.sum()) > 50
            assert torch.equal(a[order][1:][same], a[order][:-1][same])
            # a subgraph of every third row (the hub included): entries equal the full graph's bit for bit -- position and chunk
            # do not matter
            sub = voltrix.sddmm(sub_ptr, indices[edge].contiguous(), x[keep].contiguous(), y)
            assert torch.equal(sub, a[edge])


def _csr_grad_bound(indptr, indices, g, feat, num_rows):
    """csr(g) @ feat in float64 and its scale csr(|g|) @ |feat|, with the row degrees."""
    a = torch.sparse_csr_tensor(indptr.long(), indices.long(), g.double(), size=(num_rows, feat.shape[0]))
    aa = torch.sparse_csr_tensor(indptr.long(), indices.long(), g.double().abs(), size=(num_rows, feat.shape[0]))
    deg = (indptr[1:] - indptr[:-1]).double()[:, None]
    return a @ feat.double(), aa @ feat.double().abs(), deg


@pytest.mark.parametrize("pair", [(torch.float32, torch.float16), (torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16)])
def test_autograd_sddmm_gradients(cuda_device, pair):
    from voltrix.autograd import SDDMM

    indptr, indices, n, m = _special_graph()
    op = SDDMM(indptr, indices, n, m)
    x, y = _operands(n, m, 40, pair, False, seed=11)
    x.requires_grad_(True)
    y.requires_grad_(True)
    w = torch.randn(indices.numel(), device="cuda")
    s = op(x, y)
    _check(indptr, indices, x.detach(), y.detach(), s.detach(), False)
    (s * w).sum().backward()
    assert x.grad.dtype == x.dtype and y.grad.dtype == y.dtype
    # dense float64 autograd on the masked product
    x64, y64 = x.detach().double().requires_grad_(True), y.detach().double().requires_grad_(True)
    rows, cols = _rows(indptr), indices.long()
    ((x64[rows] * y64[cols]).sum(1) * w.double()).sum().backward()
    t_indptr, t_indices = voltrix.autograd.csr_transpose_device(indptr, indices, n, m)
    for grad, ref, (_, scale, deg), dt in ((x.grad, x64.grad, _csr_grad_bound(indptr, indices, w, y.detach(), n), x.dtype),
                                           (y.grad, y64.grad, _csr_grad_bound(t_indptr, t_indices, w[op.t_order], x.detach(), m),
                                            y.dtype)):
        rnd = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}[dt]     # the cast to the operand's dtype
        assert ((grad.double() - ref).abs() <= (deg + 1) * 2.0 ** -23 * scale + rnd * ref.abs() + 1e-30).all()


def _values_case(op, ip, ix, n, feat, v, w):
    """One forward + backward of op(feat, values=v); checks out, v.grad and feat.grad against float64."""
    b = feat.clone().requires_grad_(True)
    vv = v.clone().requires_grad_(True)
    out = op(b, values=vv)
    (out * w).sum().backward()
    return out, b, vv


def _check_values_grads(ip, ix, n, feat, v, w, out, b, vv):
    a = torch.sparse_csr_tensor(ip.long().cpu(), ix.long().cpu(), v.double().cpu(), size=(n, n)).to_dense().cuda()
    ref = a @ feat.double()
    scale = a.abs() @ feat.double().abs()
    assert ((out.detach().double() - ref).abs() <= 2.0 ** -8 * scale + 1e-5).all()
    g_ref, g_scale = _oracle(ip, ix, w, feat)
    assert vv.grad.dtype == vv.dtype
    assert ((vv.grad.double() - g_ref).abs() <= feat.shape[1] * 2.0 ** -23 * g_scale).all()
    ref_grad = a.T @ w.double()
    scale_g = a.abs().T @ w.double().abs()
    rnd = 2.0 ** -8 if feat.dtype == torch.bfloat16 else 2.0 ** -10
    assert b.grad.dtype == feat.dtype
    assert ((b.grad.double() - ref_grad).abs() <= 2.0 ** -8 * scale_g + rnd * ref_grad.abs() + 1e-4).all()


@pytest.mark.parametrize("csr_path", ["1", "0"])
def test_spmm_values_gradient(cuda_device, csr_path, monkeypatch):
    from voltrix import weighted
    from voltrix.autograd import SpMM

    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "none")
    monkeypatch.setenv("VOLTRIX_CSR_PATH", csr_path)
    ip_np, ix_np = _random_csr(700, 20, seed=41)
    rows = [ix_np[ip_np[r]:ip_np[r + 1]] for r in range(700)]
    dup_rows = [np.concatenate([r[:1], r]) if i % 5 == 0 else r for i, r in enumerate(rows)]
    n = 700
    torch.manual_seed(21)
    w = torch.randn(n, 48, device="cuda")
    for duplicates in (False, True):
        rr = dup_rows if duplicates else rows
        ip = torch.from_numpy(np.concatenate([[0], np.cumsum([len(r) for r in rr])]).astype(np.int32)).cuda()
        ix = torch.from_numpy(np.concatenate(rr).astype(np.int32)).cuda()
        nnz = ix.numel()
        deg = (ip[1:] - ip[:-1]).long()
        sym = (deg.double().clamp(min=1).rsqrt()[_rows(ip)]).float()          # separable: r_i
        for built in ("general", "separable"):
            first = torch.rand(nnz, device="cuda") + 0.2 if built == "general" else sym
            op = SpMM(ip, ix, n, values=first, hash_tag=f"sddmm_values_{duplicates}_{built}")
            assert duplicates or op.weighted.separable == (built == "separable")

            def no_check(*args, **kwargs):
                raise AssertionError("separable_scales ran in a forward with values")

            with monkeypatch.context() as m:         # a forward with values never runs the separable check
                m.setattr(weighted, "separable_scales", no_check)
                for dtype in (torch.float16, torch.bfloat16, torch.float32):
                    feat = torch.randn(n, 48, device="cuda").to(dtype)
                    v = torch.randn(nnz, device="cuda")
                    out, b, vv = _values_case(op, ip, ix, n, feat, v, w)
                    assert not op.weighted.separable and not op.weighted_t.separable
                    _check_values_grads(ip, ix, n, feat, v, w, out, b, vv)


def test_two_forwards_then_the_first_backward(cuda_device, monkeypatch):
    from voltrix.autograd import SpMM

    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "none")
    ip_np, ix_np = _random_csr(500, 16, seed=43)
    ip, ix = torch.from_numpy(ip_np).cuda(), torch.from_numpy(ix_np).cuda()
    n, nnz = 500, len(ix_np)
    torch.manual_seed(22)
    op = SpMM(ip, ix, n, values=torch.rand(nnz, device="cuda") + 0.1, hash_tag="sddmm_two_forwards")
    feat = torch.randn(n, 32, device="cuda").half()
    w1, w2 = torch.randn(n, 32, device="cuda"), torch.randn(n, 32, device="cuda")
    v1, v2 = torch.randn(nnz, device="cuda"), torch.rand(nnz, device="cuda") * 4.0
    b1, b2 = feat.clone().requires_grad_(True), (feat * 0.5).requires_grad_(True)
    vv1, vv2 = v1.clone().requires_grad_(True), v2.clone().requires_grad_(True)
    out1 = op(b1, values=vv1)
    out2 = op(b2, values=vv2)
    (out1 * w1).sum().backward()
    _check_values_grads(ip, ix, n, b1.detach(), v1, w1, out1, b1, vv1)
    (out2 * w2).sum().backward()
    _check_values_grads(ip, ix, n, b2.detach(), v2, w2, out2, b2, vv2)


def test_attention_layer_end_to_end(cuda_device, monkeypatch):
    """One dot-product attention layer on a ~2,000-node graph: scores from autograd.SDDMM, an edge softmax per row in plain torch,
    aggregation with autograd.SpMM(..., values=alpha) on fp16 v; loss and the four weight gradients against a dense float64
    masked-softmax model."""
    from voltrix.autograd import SDDMM, SpMM

    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "none")
    ip_np, ix_np = _random_csr(2000, 12, seed=47)
    deg = np.diff(ip_np)
    rows_np = [np.unique(np.concatenate([ix_np[ip_np[r]:ip_np[r + 1]], [r]])) for r in range(2000)]    # self loops: no empty row
    ip_np = np.concatenate([[0], np.cumsum([len(r) for r in rows_np])]).astype(np.int32)
    ix_np = np.concatenate(rows_np).astype(np.int32)
    assert deg.size == 2000
    n, d_in, d, classes = 2000, 32, 16, 6
    ip, ix = torch.from_numpy(ip_np).cuda(), torch.from_numpy(ix_np).cuda()
    rows = _rows(ip)
    nnz = ix.numel()
    torch.manual_seed(5)
    h = torch.randn(n, d_in, device="cuda")
    labels = torch.randint(0, classes, (n,), device="cuda")
    params = {k: (torch.randn(*s, device="cuda") / s[0] ** 0.5) for k, s in
              (("wq", (d_in, d)), ("wk", (d_in, d)), ("wv", (d_in, d)), ("wo", (d, classes)))}

    scores_op = SDDMM(ip, ix, n)
    agg = SpMM(ip, ix, n, values=torch.ones(nnz, device="cuda"), hash_tag="sddmm_attention")

    def edge_softmax(s):
        m = torch.full((n,), -float("inf"), device="cuda", dtype=s.dtype).scatter_reduce(0, rows, s, "amax")
        e = torch.exp(s - m[rows])
        return e / torch.zeros(n, device="cuda", dtype=s.dtype).index_add(0, rows, e)[rows]

    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    q, k, v = h @ p["wq"], h @ p["wk"], (h @ p["wv"]).half()
    alpha = edge_softmax(scores_op(q, k) / d ** 0.5)
    out = agg(v, values=alpha)
    loss = torch.nn.functional.cross_entropy(out @ p["wo"], labels)
    loss.backward()

    r = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    h64 = h.double()
    s = (h64 @ r["wq"]) @ (h64 @ r["wk"]).T / d ** 0.5
    mask = torch.zeros(n, n, dtype=torch.bool, device="cuda")
    mask[rows, ix.long()] = True
    attn = torch.softmax(s.masked_fill(~mask, -float("inf")), dim=1)
    ref_loss = torch.nn.functional.cross_entropy((attn @ (h64 @ r["wv"])) @ r["wo"], labels)
    ref_loss.backward()
    assert abs(float(loss) - float(ref_loss)) <= 2e-3 * abs(float(ref_loss))
    for name in params:
        err = float((p[name].grad.double() - r[name].grad).norm() / r[name].grad.norm())
        assert err <= 1e-2, (name, err)
