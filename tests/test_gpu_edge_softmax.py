"""GPU: the edge softmax (voltrix.edge_softmax, edge_softmax_kernels.hpp), its backward and autograd.EdgeSoftmax against float64 torch.

Oracle: the segment softmax of ``scale * scores`` in float64.  Bounds (include/voltrix_capi.h): forward
``|alpha - ref| <= ref * 2 (deg_r + |z_e - m_r| + 2) 2^-23 + 2^-126``; backward, with ``D_r = rowsum(alpha g)`` and
``A_r = rowsum(alpha |g|)`` from the kernel's alpha, ``|grad - ref| <= |scale| alpha (2 |g - D_r| + (deg_r + 2) A_r) 2^-23 + 2^-126``."""
import os
import sys

import numpy as np
import pytest
import torch

import voltrix
from conftest import REPO
from voltrix.edge_softmax import edge_softmax_backward

pytestmark = pytest.mark.gpu

CHUNK = 2048          # kChunkEdges: edges per K1 workgroup
INF = float("inf")


def _rows(indptr):
    return torch.repeat_interleave(torch.arange(indptr.numel() - 1, device=indptr.device), (indptr[1:] - indptr[:-1]).long())


def _indptr(lengths):
    ip = np.zeros(len(lengths) + 1, np.int64)
    ip[1:] = np.cumsum(lengths)
    return torch.from_numpy(ip.astype(np.int32)).cuda()


def _special_lengths():
    """Empty rows, rows of length 1, CHUNK - 1, CHUNK and CHUNK + 1 at several offsets, a hub of 300 chunks, short random rows.  It
    opens with a row that fills chunk 0 exactly and one that starts on a chunk boundary and runs past the next."""
    rng = np.random.default_rng(7)
    lengths = [CHUNK, CHUNK + 1]
    for r in range(4000):
        if r % 13 == 0:
            lengths.append(0)
        elif r in (100, 900, 2500):
            lengths += [CHUNK - 1, CHUNK, CHUNK + 1, 0, 1]
        elif r == 1500:
            lengths.append(300 * CHUNK + 17)
        elif r % 3 == 0:
            lengths.append(1)
        else:
            lengths.append(int(rng.integers(1, 40)))
    return lengths


def _segments(indptr):
    """Host int64 row pointers, the first edge of every non-empty row, and the degree of every edge's row."""
    ip = indptr.cpu().numpy().astype(np.int64)
    deg = np.diff(ip)
    return ip, ip[:-1][deg > 0], np.repeat(deg, deg).astype(np.float64)


def _segment_sum(x, ip, starts):
    """Sum of x over every row, per edge (numpy reduceat in float64: no atomics, no contention on hub rows)."""
    deg = np.diff(ip)
    return np.repeat(np.add.reduceat(x, starts), deg[deg > 0]) if starts.size else x


def _ref(indptr, scores, scale):
    """float64 segment softmax on the host (zeros for rows of -inf), z, the row max of z per edge, the degree per edge."""
    ip, starts, deg = _segments(indptr)
    z = scores.double().cpu().numpy() * scale
    d = np.diff(ip)
    mr = np.repeat(np.maximum.reduceat(z, starts), d[d > 0])
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.where(z == -np.inf, 0.0, np.exp(z - np.where(mr == -np.inf, 0.0, mr)))
        s = _segment_sum(e, ip, starts)
        ref = np.where(s > 0, e / np.where(s > 0, s, 1.0), 0.0)
    return ref, z, mr, deg, (ip, starts)


def _check_forward(indptr, scores, scale, alpha):
    ref, z, mr, deg, (ip, starts) = _ref(indptr, scores, scale)
    assert alpha.dtype == torch.float32 and alpha.shape == scores.shape
    a = alpha.double().cpu().numpy()
    with np.errstate(invalid="ignore"):
        gap = np.nan_to_num(np.abs(z - mr), nan=0.0, posinf=0.0)
    bound = ref * 2 * (deg + gap + 2) * 2.0 ** -23 + 2.0 ** -126
    err = np.abs(a - ref)
    assert bool((err <= bound).all()), float((err / bound).max())
    # rows sum to 1 within the sum of the bounds (rows with a finite entry)
    sums, tol, live = _segment_sum(a, ip, starts), _segment_sum(bound, ip, starts), _segment_sum(ref, ip, starts) > 0
    assert bool((np.abs(sums - 1)[live] <= tol[live] + 2.0 ** -40).all())


def _check_backward(indptr, alpha, g, scale, grad):
    ip, starts, deg = _segments(indptr)
    a, gd = alpha.double().cpu().numpy(), g.double().cpu().numpy()
    d = _segment_sum(a * gd, ip, starts)
    aa = _segment_sum(a * np.abs(gd), ip, starts)
    ref = scale * a * (gd - d)
    bound = abs(scale) * a * (2 * np.abs(gd - d) + (deg + 2) * aa) * 2.0 ** -23 + 2.0 ** -126
    err = np.abs(grad.double().cpu().numpy() - ref)
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("scale", [1.0, 0.125, 16 ** -0.5 / 1.4142135623730951, 3.0, -0.5])
def test_special_pattern_forward_and_backward(cuda_device, scale):
    indptr = _indptr(_special_lengths())
    nnz = int(indptr[-1])
    assert nnz > 300 * CHUNK
    g = torch.Generator(device="cuda").manual_seed(3)
    for spread in (4.0, 80.0):              # +-80: the |z - m| term matters
        scores = (torch.rand(nnz, device="cuda", generator=g) * 2 - 1) * spread
        alpha = voltrix.edge_softmax(indptr, scores, scale)
        _check_forward(indptr, scores, scale, alpha)
        grad_alpha = torch.randn(nnz, device="cuda", generator=g)
        _check_backward(indptr, alpha, grad_alpha, scale, edge_softmax_backward(indptr, alpha, grad_alpha, scale))


@pytest.mark.parametrize("scale", [0.0, -0.0])
def test_scale_zero_gives_the_row_mean(cuda_device, scale):
    """scale = 0: every entry 1 / deg_r (crossing rows included, whatever the chunk boundaries), and a zero gradient."""
    indptr = _indptr(_special_lengths())
    nnz = int(indptr[-1])
    scores = torch.randn(nnz, device="cuda") * 30
    alpha = voltrix.edge_softmax(indptr, scores, scale)
    _, _, deg = _segments(indptr)
    a = alpha.double().cpu().numpy()
    assert bool(np.isfinite(a).all())
    assert bool((np.abs(a - 1 / deg) <= 2.0 ** -22 / deg).all()), float(np.abs(a * deg - 1).max())
    _check_forward(indptr, scores, scale, alpha)
    grad = edge_softmax_backward(indptr, alpha, torch.randn(nnz, device="cuda"), scale)
    assert bool((grad == 0).all())


def test_runs_of_empty_rows(cuda_device):
    """Rows of one to three edges between runs of up to 20,000 empty rows: a thread's edges can lie rows apart."""
    rng = np.random.default_rng(13)
    lengths = []
    for _ in range(3000):
        lengths += [int(rng.integers(1, 4))] + [0] * int(rng.integers(0, 20000) if rng.random() < 0.3 else rng.integers(0, 3))
    indptr = _indptr(lengths)
    nnz = int(indptr[-1])
    scores = torch.randn(nnz, device="cuda") * 3
    alpha = voltrix.edge_softmax(indptr, scores, 0.5)
    _check_forward(indptr, scores, 0.5, alpha)
    g = torch.randn(nnz, device="cuda")
    _check_backward(indptr, alpha, g, 0.5, edge_softmax_backward(indptr, alpha, g, 0.5))


def test_web_berkstan_like_reduced_scale(cuda_device):
    import synth_graphs

    indptr, _, _ = synth_graphs.generate("web_berkstan_like", device="cuda", scale=0.25)
    nnz = int(indptr[-1])
    deg = indptr[1:] - indptr[:-1]
    assert int(deg.max()) > 4 * CHUNK
    scores = torch.randn(nnz, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)) * 6
    for scale in (1.0, 0.25):
        alpha = voltrix.edge_softmax(indptr, scores, scale)
        _check_forward(indptr, scores, scale, alpha)
        g = torch.randn(nnz, device="cuda")
        _check_backward(indptr, alpha, g, scale, edge_softmax_backward(indptr, alpha, g, scale))


def test_special_values(cuda_device):
    # short rows, then long rows crossing chunks: all -inf, one NaN, some -inf; the rows around them must stay finite
    short = [[-INF, 1.0, 2.0], [-INF, -INF], [float("nan"), 1.0], [3.0, 4.0], [-INF]]
    rng = np.random.default_rng(11)
    long_inf = np.full(5000, -np.inf)
    long_nan = rng.standard_normal(5000)
    long_nan[4321] = np.nan
    long_some = rng.standard_normal(5000)
    long_some[::7] = -np.inf
    rows = short + [long_inf.tolist(), rng.standard_normal(3000).tolist(), long_nan.tolist(), long_some.tolist(), [0.5, 0.25]]
    indptr = _indptr([len(r) for r in rows])
    scores = torch.tensor(np.concatenate([np.asarray(r, np.float64) for r in rows]), dtype=torch.float32, device="cuda")
    ip = indptr.cpu().numpy()
    alpha = voltrix.edge_softmax(indptr, scores, 0.7)
    seg = lambda t, r: t[ip[r]:ip[r + 1]]                       # noqa: E731
    nan_rows = {2, 7}
    for r in range(len(rows)):
        a = seg(alpha, r)
        if r in nan_rows:
            assert bool(torch.isnan(a).all()), r
        else:
            assert bool(torch.isfinite(a).all()), r
            assert bool((a[seg(scores, r) == -INF] == 0).all()), r
    assert bool((seg(alpha, 1) == 0).all()) and bool((seg(alpha, 4) == 0).all()) and bool((seg(alpha, 5) == 0).all())
    finite = torch.ones(scores.numel(), dtype=torch.bool, device="cuda")
    for r in nan_rows:
        finite[ip[r]:ip[r + 1]] = False
    ref = torch.from_numpy(_ref(indptr, scores.masked_fill(~finite, 0.0), 0.7)[0]).cuda()
    assert bool(((alpha.double() - ref).abs()[finite] <= 1e-5 * ref[finite] + 2.0 ** -126).all())
    g = torch.randn(scores.numel(), device="cuda")
    grad = edge_softmax_backward(indptr, alpha, g, 0.7)
    for r in (1, 4, 5):                                          # rows of -inf: zero gradient
        assert bool((seg(grad, r) == 0).all()), r
    for r in nan_rows:
        assert bool(torch.isnan(seg(grad, r)).all()), r
    assert bool(torch.isfinite(grad[finite]).all())


def test_determinism_and_a_second_stream(cuda_device):
    indptr = _indptr(_special_lengths())
    nnz = int(indptr[-1])
    scores = torch.randn(nnz, device="cuda") * 10
    g = torch.randn(nnz, device="cuda")
    a = voltrix.edge_softmax(indptr, scores, 0.3)
    b = voltrix.edge_softmax(indptr, scores, 0.3)
    assert torch.equal(a, b)
    ga = edge_softmax_backward(indptr, a, g, 0.3)
    assert torch.equal(ga, edge_softmax_backward(indptr, a, g, 0.3))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = voltrix.edge_softmax(indptr, scores, 0.3)
        gc = edge_softmax_backward(indptr, c, g, 0.3)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(a, c) and torch.equal(ga, gc)
    # fp16 scores are cast to fp32 first
    h = scores.half()
    assert torch.equal(voltrix.edge_softmax(indptr, h, 0.3), voltrix.edge_softmax(indptr, h.float(), 0.3))
    assert voltrix.edge_softmax(torch.zeros(5, dtype=torch.int32, device="cuda"), torch.zeros(0, device="cuda")).shape == (0,)


def test_no_host_sync(cuda_device):
    indptr = _indptr(_special_lengths())
    nnz = int(indptr[-1])
    scores = torch.randn(nnz, device="cuda")
    g = torch.randn(nnz, device="cuda")
    voltrix.edge_softmax(indptr, scores)          # library loaded, allocator warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        alpha = voltrix.edge_softmax(indptr, scores, 0.5)
        grad = edge_softmax_backward(indptr, alpha, g, 0.5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    _check_backward(indptr, alpha, g, 0.5, grad)


def test_graph_capture_replays_bit_for_bit(cuda_device):
    indptr = _indptr(_special_lengths())
    nnz = int(indptr[-1])
    scores = torch.randn(nnz, device="cuda") * 5
    eager = voltrix.edge_softmax(indptr, scores, 0.25)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        voltrix.edge_softmax(indptr, scores, 0.25)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = voltrix.edge_softmax(indptr, scores, 0.25)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def _segment_softmax64(indptr, s, scale):
    """The torch composite in float64 on the host (index_add on the device contends on hub rows)."""
    indptr = indptr.cpu()
    rows = _rows(indptr)
    n = indptr.numel() - 1
    z = s * scale
    m = torch.full((n,), -INF, dtype=z.dtype).scatter_reduce(0, rows, z.detach(), "amax")
    e = torch.exp(z - m[rows])
    return e / torch.zeros(n, dtype=z.dtype).index_add(0, rows, e)[rows]


def test_autograd_edge_softmax(cuda_device):
    from voltrix.autograd import EdgeSoftmax

    indptr = _indptr(_special_lengths())
    n, nnz = indptr.numel() - 1, int(indptr[-1])
    op = EdgeSoftmax(indptr, n)
    scores = (torch.randn(nnz, device="cuda") * 3).requires_grad_(True)
    w = torch.randn(nnz, device="cuda")
    alpha = op(scores, 0.4)
    (alpha * w).sum().backward()
    assert torch.equal(alpha.detach(), voltrix.edge_softmax(indptr, scores.detach(), 0.4))
    assert torch.equal(scores.grad, edge_softmax_backward(indptr, alpha.detach(), w, 0.4))
    _check_backward(indptr, alpha.detach(), w, 0.4, scores.grad)
    s64 = scores.detach().double().cpu().requires_grad_(True)
    (_segment_softmax64(indptr, s64, 0.4) * w.double().cpu()).sum().backward()
    assert float((scores.grad.double().cpu() - s64.grad).norm() / s64.grad.norm()) <= 1e-5
    # fp16 scores: the gradient comes back in fp16
    h = scores.detach().half().requires_grad_(True)
    (op(h, 0.4) * w).sum().backward()
    assert h.grad.dtype == torch.float16


def test_attention_layer_end_to_end(cuda_device, monkeypatch):
    """Dot-product attention on a ~2,000-node graph: SDDMM -> EdgeSoftmax(scale = d^-0.5) -> SpMM(values=) on fp16 v; the loss and the
    four weight gradients against a dense float64 masked-softmax model."""
    from test_hybrid_plan import _random_csr
    from voltrix.autograd import SDDMM, EdgeSoftmax, SpMM

    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "none")
    ip_np, ix_np = _random_csr(2000, 12, seed=47)
    rows_np = [np.unique(np.concatenate([ix_np[ip_np[r]:ip_np[r + 1]], [r]])) for r in range(2000)]    # self loops: no empty row
    ip_np = np.concatenate([[0], np.cumsum([len(r) for r in rows_np])]).astype(np.int32)
    ix_np = np.concatenate(rows_np).astype(np.int32)
    n, d_in, d, classes = 2000, 32, 16, 6
    ip, ix = torch.from_numpy(ip_np).cuda(), torch.from_numpy(ix_np).cuda()
    rows = _rows(ip)
    nnz = ix.numel()
    torch.manual_seed(5)
    h = torch.randn(n, d_in, device="cuda")
    labels = torch.randint(0, classes, (n,), device="cuda")
    params = {k: (torch.randn(*s, device="cuda") / s[0] ** 0.5) for k, s in
              (("wq", (d_in, d)), ("wk", (d_in, d)), ("wv", (d_in, d)), ("wo", (d, classes)))}

    scores_op, softmax = SDDMM(ip, ix, n), EdgeSoftmax(ip, n)
    agg = SpMM(ip, ix, n, values=torch.ones(nnz, device="cuda"), hash_tag="edge_softmax_attention")
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    q, k, v = h @ p["wq"], h @ p["wk"], (h @ p["wv"]).half()
    alpha = softmax(scores_op(q, k), d ** -0.5)
    out = agg(v, values=alpha)
    loss = torch.nn.functional.cross_entropy(out @ p["wo"], labels)
    loss.backward()

    r = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    h64 = h.double()
    s = (h64 @ r["wq"]) @ (h64 @ r["wk"]).T * d ** -0.5
    mask = torch.zeros(n, n, dtype=torch.bool, device="cuda")
    mask[rows, ix.long()] = True
    attn = torch.softmax(s.masked_fill(~mask, -INF), dim=1)
    ref_loss = torch.nn.functional.cross_entropy((attn @ (h64 @ r["wv"])) @ r["wo"], labels)
    ref_loss.backward()
    assert abs(float(loss) - float(ref_loss)) <= 2e-3 * abs(float(ref_loss))
    for name in params:
        err = float((p[name].grad.double() - r[name].grad).norm() / r[name].grad.norm())
        assert err <= 1e-2, (name, err)


def test_gat_example_end_to_end(cuda_device, monkeypatch):
    """examples/gat_train.py's two-layer GAT on a ~1,500-node graph: the loss and every parameter gradient against a dense float64 GAT
    with the same parameters."""
    from test_hybrid_plan import _random_csr

    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "none")
    sys.path.insert(0, os.path.join(REPO, "examples"))
    try:
        import gat_train
    finally:
        sys.path.remove(os.path.join(REPO, "examples"))
    n, in_feats, hidden, classes = 1500, 24, 16, 8
    ip_np, ix_np = _random_csr(n, 10, seed=53)
    ip, ix = gat_train.with_self_loops(torch.from_numpy(ip_np).cuda(), torch.from_numpy(ix_np).cuda(), n)
    torch.manual_seed(9)
    graph = gat_train.Graph(ip, ix, n, hash_tag="edge_softmax_gat_test")
    model = gat_train.GAT(graph, in_feats, hidden, classes).cuda()
    x = torch.randn(n, in_feats, device="cuda")
    y = torch.randint(0, classes, (n,), device="cuda")
    loss = torch.nn.functional.cross_entropy(model(x), y)
    loss.backward()

    mask = torch.zeros(n, n, dtype=torch.bool, device="cuda")
    mask[graph.rows, graph.cols] = True
    ref = {name: t.detach().double().clone().requires_grad_(True) for name, t in model.named_parameters()}

    def layer(pre, x64):
        wh = x64 @ ref[pre + ".w.weight"].T
        s = torch.nn.functional.leaky_relu((wh @ ref[pre + ".a_l"])[:, None] + (wh @ ref[pre + ".a_r"])[None, :], 0.2)
        return torch.softmax(s.masked_fill(~mask, -INF), dim=1) @ wh

    out64 = layer("l2", torch.nn.functional.elu(layer("l1", x.double())))
    ref_loss = torch.nn.functional.cross_entropy(out64, y)
    ref_loss.backward()
    assert abs(float(loss) - float(ref_loss)) <= 2e-3 * abs(float(ref_loss))
    for name, t in model.named_parameters():
        err = float((t.grad.double() - ref[name].grad).norm() / ref[name].grad.norm())
        assert err <= 2e-2, (name, err)
