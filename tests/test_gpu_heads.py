"""GPU: the multi-head attention operators -- voltrix.sddmm on [n, H, D], voltrix.edge_softmax on [nnz, H], voltrix.spmm_heads and
their autograd forms -- against float64 oracles per head, and bit for bit against the single-head kernels on contiguous slices.

Bounds (the single-head ones, per head; include/voltrix_capi.h):
  SDDMM         |out - ref| <= D 2^-23 (|x| |y|)[e, h]; integers exact
  edge softmax  |alpha - ref| <= ref 2 (deg_r + |z_e - m_r| + 2) 2^-23 + 2^-126
                |grad - ref| <= |scale| alpha (2 |g - D_r| + (deg_r + 2) A_r) 2^-23 + 2^-126
  aggregation   |out - ref| <= deg_r 2^-23 sum_e |v[e, h]| |feat[col_e, h, d]|"""
import os
import sys

import numpy as np
import pytest
import torch

import voltrix
from conftest import CSR_FIXTURES, REPO, load_csr_fixture
from voltrix.edge_softmax import edge_softmax_backward
from voltrix.sddmm import csr_values_product

pytestmark = pytest.mark.gpu

CHUNK = 2048          # kChunkEdges: edges per K1 workgroup of the edge softmax
INF = float("inf")
PAIRS = [(torch.float32, torch.float16), (torch.float32, torch.bfloat16), (torch.float16, torch.float16),
         (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32)]
TYPES = [torch.float32, torch.float16, torch.bfloat16]
# (H, D); (2, 520): a head of 65 16-byte pieces of fp16 (130 of fp32) -- wider than the 64 lanes of a group
SHAPES = [(1, 64), (2, 8), (4, 16), (8, 8), (8, 16), (8, 64), (3, 20), (16, 32), (2, 520)]
RND = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}     # a cast to the dtype


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


_GRAPHS = {}


def _graph(name):
    """(indptr, indices, num_rows, num_cols) on the device.  'special': the row lengths above over 3,000 columns (rectangular; the long
    rows repeat columns, so duplicates are many); 'amazon0601_like': the synthetic stand-in, 3.4 M edges."""
    if name not in _GRAPHS:
        if name == "special":
            indptr = _indptr(_special_lengths())
            g = torch.Generator(device="cuda").manual_seed(17)
            cols = torch.randint(0, 3000, (int(indptr[-1]),), device="cuda", generator=g)
            indices = (torch.sort(_rows(indptr) * 3000 + cols).values % 3000).to(torch.int32)      # columns sorted inside every row
            _GRAPHS[name] = (indptr, indices, indptr.numel() - 1, 3000)
        elif name == "amazon0601_like":
            import synth_graphs

            indptr, indices, _ = synth_graphs.generate(name, device="cuda")
            _GRAPHS[name] = (indptr.int(), indices.int(), indptr.numel() - 1, indptr.numel() - 1)
        else:
            g = load_csr_fixture(name)
            n = int(g["num_nodes"])
            _GRAPHS[name] = (torch.from_numpy(g["indptr"]).cuda(), torch.from_numpy(g["indices"]).cuda(), n, n)
    return _GRAPHS[name]


def _randn(shape, dtype, seed, integer=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if integer:
        return torch.randint(-3, 4, shape, device="cuda", generator=g).to(dtype)
    return torch.randn(shape, device="cuda", generator=g).to(dtype)


# ---- SDDMM ----------------------------------------------------------------------------------------------------------------------------
def _check_sddmm(indptr, indices, x, y, out, integer, single_head_bits=True):
    rows, cols = _rows(indptr), indices.long()
    heads, dim = x.shape[1], x.shape[2]
    assert out.dtype == torch.float32 and out.shape == (indices.numel(), heads)
    for h in range(heads):
        xs, ys = x[:, h].contiguous(), y[:, h].contiguous()
        ref = (xs.double()[rows] * ys.double()[cols]).sum(1)
        if integer:
            assert torch.equal(out[:, h].double(), ref), h
        else:
            scale = (xs.double().abs()[rows] * ys.double().abs()[cols]).sum(1)
            err = (out[:, h].double() - ref).abs()
            assert bool((err <= dim * 2.0 ** -23 * scale).all()), (h, float((err / (dim * 2.0 ** -23 * scale + 1e-300)).max()))
        if single_head_bits:      # the same lanes per head, the same butterfly: the bits of the 2-D call on the contiguous slices
            assert torch.equal(out[:, h], voltrix.sddmm(indptr, indices, xs, ys)), h


@pytest.mark.parametrize("name", CSR_FIXTURES + ("special",))
def test_sddmm_heads_shapes_and_pairs(cuda_device, name):
    indptr, indices, n, m = _graph(name)
    for heads, dim in SHAPES:
        pairs = PAIRS if name != "special" or (heads, dim) in ((8, 8), (3, 20), (2, 520)) else PAIRS[2:3] + PAIRS[4:]
        for pair in pairs:
            for integer in (True, False):
                x = _randn((n, heads, dim), pair[0], 100 * heads + dim, integer)
                y = _randn((m, heads, dim), pair[1], 100 * heads + dim + 1, integer)
                _check_sddmm(indptr, indices, x, y, voltrix.sddmm(indptr, indices, x, y), integer)


def test_sddmm_heads_large_graph_determinism_duplicates_and_2d_unchanged(cuda_device):
    indptr, indices, n, m = _graph("amazon0601_like")
    assert indices.numel() > 3_000_000
    for heads, dim in ((8, 8), (4, 16), (8, 16)):
        x = _randn((n, heads, dim), torch.float16, 1)
        y = _randn((m, heads, dim), torch.float16, 2)
        out = voltrix.sddmm(indptr, indices, x, y)
        _check_sddmm(indptr, indices, x, y, out, False)
        assert torch.equal(out, voltrix.sddmm(indptr, indices, x, y))
    # duplicates: the same (row, col) gives the same bits in every head
    indptr, indices, n, m = _graph("special")
    x, y = _randn((n, 8, 16), torch.float32, 3), _randn((m, 8, 16), torch.float16, 4)
    out = voltrix.sddmm(indptr, indices, x, y)
    key = _rows(indptr) * m + indices.long()
    order = torch.argsort(key)
    same = key[order][1:] == key[order][:-1]
    assert int(same.sum()) > 1000
    assert torch.equal(out[order][1:][same], out[order][:-1][same])
    # other pairs are cast; nothing to do
    xh, yf = _randn((n, 2, 8), torch.float16, 5), _randn((m, 2, 8), torch.float32, 6)
    _check_sddmm(indptr, indices, xh.float(), yf, voltrix.sddmm(indptr, indices, xh, yf), False)
    empty = voltrix.sddmm(torch.zeros(n + 1, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"), x, y)
    assert empty.shape == (0, 8) and empty.dtype == torch.float32


# ---- edge softmax ---------------------------------------------------------------------------------------------------------------------
def _segments(indptr):
    ip = indptr.cpu().numpy().astype(np.int64)
    deg = np.diff(ip)
    return ip, ip[:-1][deg > 0], np.repeat(deg, deg).astype(np.float64)


def _segment_sum(x, ip, starts):
    deg = np.diff(ip)
    return np.repeat(np.add.reduceat(x, starts), deg[deg > 0]) if starts.size else x


def _ref_softmax(indptr, scores, scale):
    """float64 segment softmax of one column on the host (zeros for rows of -inf), z, the row max of z per edge, the degree per edge."""
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
    assert alpha.dtype == torch.float32 and alpha.shape == scores.shape
    for h in range(scores.shape[1]):
        ref, z, mr, deg, (ip, starts) = _ref_softmax(indptr, scores[:, h], scale)
        a = alpha[:, h].double().cpu().numpy()
        with np.errstate(invalid="ignore"):
            gap = np.nan_to_num(np.abs(z - mr), nan=0.0, posinf=0.0)
        bound = ref * 2 * (deg + gap + 2) * 2.0 ** -23 + 2.0 ** -126
        err = np.abs(a - ref)
        assert bool((err <= bound).all()), (h, float((err / bound).max()))
        # every live row of every head sums to 1 within the summed bound
        sums, tol, live = _segment_sum(a, ip, starts), _segment_sum(bound, ip, starts), _segment_sum(ref, ip, starts) > 0
        assert bool((np.abs(sums - 1)[live] <= tol[live] + 2.0 ** -40).all()), h


def _check_backward(indptr, alpha, g, scale, grad):
    ip, starts, deg = _segments(indptr)
    assert grad.dtype == torch.float32 and grad.shape == alpha.shape
    for h in range(alpha.shape[1]):
        a, gd = alpha[:, h].double().cpu().numpy(), g[:, h].double().cpu().numpy()
        d = _segment_sum(a * gd, ip, starts)
        aa = _segment_sum(a * np.abs(gd), ip, starts)
        ref = scale * a * (gd - d)
        bound = abs(scale) * a * (2 * np.abs(gd - d) + (deg + 2) * aa) * 2.0 ** -23 + 2.0 ** -126
        err = np.abs(grad[:, h].double().cpu().numpy() - ref)
        assert bool((err <= bound).all()), (h, float((err / bound).max()))


@pytest.mark.parametrize("heads", [2, 3, 8, 16])
def test_edge_softmax_heads_special_pattern(cuda_device, heads):
    indptr = _graph("special")[0]
    nnz = int(indptr[-1])
    assert nnz > 300 * CHUNK
    g = torch.Generator(device="cuda").manual_seed(3)
    for scale, spread in ((1.0, 4.0), (0.125, 80.0), (-0.5, 4.0), (3.0, 80.0)):      # +-80: the |z - m| term matters
        scores = (torch.rand(nnz, heads, device="cuda", generator=g) * 2 - 1) * spread
        alpha = voltrix.edge_softmax(indptr, scores, scale)
        _check_forward(indptr, scores, scale, alpha)
        grad_alpha = torch.randn(nnz, heads, device="cuda", generator=g)
        grad = edge_softmax_backward(indptr, alpha, grad_alpha, scale)
        _check_backward(indptr, alpha, grad_alpha, scale, grad)
        for h in range(0, heads, 3):       # the single-head reduction per head: the bits of the 1-D call on the contiguous column
            assert torch.equal(alpha[:, h], voltrix.edge_softmax(indptr, scores[:, h].contiguous(), scale))
            assert torch.equal(grad[:, h], edge_softmax_backward(indptr, alpha[:, h].contiguous(), grad_alpha[:, h].contiguous(), scale))


@pytest.mark.parametrize("name", CSR_FIXTURES + ("amazon0601_like",))
def test_edge_softmax_heads_graphs(cuda_device, name):
    indptr = _graph(name)[0]
    nnz = int(indptr[-1])
    for heads in (4, 8):
        scores = _randn((nnz, heads), torch.float32, heads) * 6
        alpha = voltrix.edge_softmax(indptr, scores, 0.25)
        _check_forward(indptr, scores, 0.25, alpha)
        g = _randn((nnz, heads), torch.float32, heads + 1)
        _check_backward(indptr, alpha, g, 0.25, edge_softmax_backward(indptr, alpha, g, 0.25))


@pytest.mark.parametrize("scale", [0.0, -0.0])
def test_edge_softmax_heads_scale_zero_gives_the_row_mean(cuda_device, scale):
    indptr = _graph("special")[0]
    nnz = int(indptr[-1])
    scores = torch.randn(nnz, 4, device="cuda") * 30
    alpha = voltrix.edge_softmax(indptr, scores, scale)
    _, _, deg = _segments(indptr)
    a = alpha.double().cpu().numpy()
    assert bool(np.isfinite(a).all())
    assert bool((np.abs(a - 1 / deg[:, None]) <= 2.0 ** -22 / deg[:, None]).all())
    _check_forward(indptr, scores, scale, alpha)
    grad = edge_softmax_backward(indptr, alpha, torch.randn(nnz, 4, device="cuda"), scale)
    assert bool((grad == 0).all())


def test_edge_softmax_heads_runs_of_empty_rows(cuda_device):
    rng = np.random.default_rng(13)
    lengths = []
    for _ in range(3000):
        lengths += [int(rng.integers(1, 4))] + [0] * int(rng.integers(0, 20000) if rng.random() < 0.3 else rng.integers(0, 3))
    indptr = _indptr(lengths)
    nnz = int(indptr[-1])
    scores = torch.randn(nnz, 8, device="cuda") * 3
    alpha = voltrix.edge_softmax(indptr, scores, 0.5)
    _check_forward(indptr, scores, 0.5, alpha)
    g = torch.randn(nnz, 8, device="cuda")
    _check_backward(indptr, alpha, g, 0.5, edge_softmax_backward(indptr, alpha, g, 0.5))


def test_edge_softmax_heads_special_values_stay_in_their_row_and_head(cuda_device):
    """Head 1 gets the special rows (all -inf, one NaN, some -inf; short rows and rows crossing chunks); heads 0 and 2 of the same rows
    hold ordinary numbers and must come out finite and correct."""
    short = [[-INF, 1.0, 2.0], [-INF, -INF], [float("nan"), 1.0], [3.0, 4.0], [-INF]]
    rng = np.random.default_rng(11)
    long_inf = np.full(5000, -np.inf)
    long_nan = rng.standard_normal(5000)
    long_nan[4321] = np.nan
    long_some = rng.standard_normal(5000)
    long_some[::7] = -np.inf
    rows = short + [long_inf.tolist(), rng.standard_normal(3000).tolist(), long_nan.tolist(), long_some.tolist(), [0.5, 0.25]]
    indptr = _indptr([len(r) for r in rows])
    special = torch.tensor(np.concatenate([np.asarray(r, np.float64) for r in rows]), dtype=torch.float32, device="cuda")
    nnz = special.numel()
    scores = torch.randn(nnz, 3, device="cuda")
    scores[:, 1] = special
    ip = indptr.cpu().numpy()
    alpha = voltrix.edge_softmax(indptr, scores, 0.7)
    g = torch.randn(nnz, 3, device="cuda")
    grad = edge_softmax_backward(indptr, alpha, g, 0.7)
    seg = lambda t, r: t[ip[r]:ip[r + 1]]                       # noqa: E731
    nan_rows = {2, 7}
    for r in range(len(rows)):
        a = seg(alpha[:, 1], r)
        if r in nan_rows:
            assert bool(torch.isnan(a).all()), r
            assert bool(torch.isnan(seg(grad[:, 1], r)).all()), r
        else:
            assert bool(torch.isfinite(a).all()), r
            assert bool((a[seg(special, r) == -INF] == 0).all()), r
            assert bool(torch.isfinite(seg(grad[:, 1], r)).all()), r
    for r in (1, 4, 5):                                          # rows of -inf: zeros and a zero gradient
        assert bool((seg(alpha[:, 1], r) == 0).all()) and bool((seg(grad[:, 1], r) == 0).all()), r
    # the other heads of the same rows: finite, within the bounds, and the bits of the 1-D call
    others = [0, 2]
    assert bool(torch.isfinite(alpha[:, others]).all()) and bool(torch.isfinite(grad[:, others]).all())
    _check_forward(indptr, scores[:, others].contiguous(), 0.7, alpha[:, others].contiguous())
    _check_backward(indptr, alpha[:, others].contiguous(), g[:, others].contiguous(), 0.7, grad[:, others].contiguous())
    for h in range(3):
        one = voltrix.edge_softmax(indptr, scores[:, h].contiguous(), 0.7)
        assert torch.equal(torch.nan_to_num(alpha[:, h], nan=-1.0), torch.nan_to_num(one, nan=-1.0)), h
    # head 1 outside its NaN rows against the float64 softmax
    finite = torch.ones(nnz, dtype=torch.bool, device="cuda")
    for r in nan_rows:
        finite[ip[r]:ip[r + 1]] = False
    ref = torch.from_numpy(_ref_softmax(indptr, special.masked_fill(~finite, 0.0), 0.7)[0]).cuda()
    assert bool(((alpha[:, 1].double() - ref).abs()[finite] <= 1e-5 * ref[finite] + 2.0 ** -126).all())


def test_edge_softmax_heads_one_head_determinism_streams_capture_no_sync(cuda_device):
    indptr = _graph("special")[0]
    nnz = int(indptr[-1])
    scores = torch.randn(nnz, 8, device="cuda") * 10
    g = torch.randn(nnz, 8, device="cuda")
    # H = 1 given as [nnz, 1]: the bits of the 1-D call
    one = scores[:, :1].contiguous()
    a1 = voltrix.edge_softmax(indptr, one, 0.3)
    assert a1.shape == (nnz, 1) and torch.equal(a1.view(-1), voltrix.edge_softmax(indptr, one.view(-1), 0.3))
    g1 = edge_softmax_backward(indptr, a1, g[:, :1].contiguous(), 0.3)
    assert g1.shape == (nnz, 1) and torch.equal(g1.view(-1), edge_softmax_backward(indptr, a1.view(-1), g[:, 0].contiguous(), 0.3))
    # two calls: the same bits; a second stream: the same bits
    a = voltrix.edge_softmax(indptr, scores, 0.3)
    assert torch.equal(a, voltrix.edge_softmax(indptr, scores, 0.3))
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
    # fp16 scores are cast to fp32 first; nothing to do
    h = scores.half()
    assert torch.equal(voltrix.edge_softmax(indptr, h, 0.3), voltrix.edge_softmax(indptr, h.float(), 0.3))
    assert voltrix.edge_softmax(torch.zeros(5, dtype=torch.int32, device="cuda"), torch.zeros(0, 4, device="cuda")).shape == (0, 4)
    # no host synchronisation
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        alpha = voltrix.edge_softmax(indptr, scores, 0.5)
        grad = edge_softmax_backward(indptr, alpha, g, 0.5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    _check_backward(indptr, alpha, g, 0.5, grad)
    # capture and replay
    eager = voltrix.edge_softmax(indptr, scores, 0.25)
    eager_grad = edge_softmax_backward(indptr, eager, g, 0.25)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        voltrix.edge_softmax(indptr, scores, 0.25)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = voltrix.edge_softmax(indptr, scores, 0.25)
        out_grad = edge_softmax_backward(indptr, out, g, 0.25)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(out_grad, eager_grad)


# ---- aggregation ----------------------------------------------------------------------------------------------------------------------
def _aggregate_ref(indptr, indices, v, feat, num_rows):
    """Per head: csr(v[:, h]) @ feat[:, h] in float64, its scale csr(|v|) @ |feat|, and the row degrees."""
    deg = (indptr[1:] - indptr[:-1]).double()[:, None]
    for h in range(feat.shape[1]):
        a = torch.sparse_csr_tensor(indptr.long(), indices.long(), v[:, h].double(), size=(num_rows, feat.shape[0]))
        aa = torch.sparse_csr_tensor(indptr.long(), indices.long(), v[:, h].double().abs(), size=(num_rows, feat.shape[0]))
        yield h, a @ feat[:, h].double(), aa @ feat[:, h].double().abs(), deg


def _check_aggregate(indptr, indices, v, feat, num_rows, out, single_head_bits=True):
    assert out.dtype == torch.float32 and out.shape == (num_rows,) + tuple(feat.shape[1:])
    empty = indptr[1:] == indptr[:-1]
    assert bool((out[empty] == 0).all())                      # every row written, empty rows zero
    for h, ref, scale, deg in _aggregate_ref(indptr, indices, v, feat, num_rows):
        err = (out[:, h].double() - ref).abs()
        assert bool((err <= deg * 2.0 ** -23 * scale).all()), h
        if single_head_bits:      # both sum one fused multiply-add per element in CSR order
            assert torch.equal(out[:, h], csr_values_product(indptr, indices, v[:, h].contiguous(), num_rows, feat[:, h].contiguous())), h


@pytest.mark.parametrize("name", CSR_FIXTURES + ("special",))
def test_aggregation_heads_shapes_and_types(cuda_device, name):
    indptr, indices, n, m = _graph(name)
    nnz = indices.numel()
    for heads, dim in SHAPES + [(1, 8)]:      # (1, 8): a row of one 16-byte piece for the 16-bit types
        for dtype in TYPES:
            feat = _randn((m, heads, dim), dtype, 7 * heads + dim)
            v = _randn((nnz, heads), torch.float32, 7 * heads + dim + 1)
            out = voltrix.spmm_heads(indptr, indices, v, feat, n)
            _check_aggregate(indptr, indices, v, feat, n, out)
            assert torch.equal(out, voltrix.spmm_heads(indptr, indices, v, feat, n))
    # integers: exact
    feat, v = _randn((m, 4, 16), torch.float16, 1, integer=True), _randn((nnz, 4), torch.float32, 2, integer=True)
    out = voltrix.spmm_heads(indptr, indices, v, feat, n)
    for h, ref, _, _ in _aggregate_ref(indptr, indices, v, feat, n):
        assert torch.equal(out[:, h].double(), ref)


def test_aggregation_heads_large_graph(cuda_device):
    indptr, indices, n, m = _graph("amazon0601_like")
    for heads, dim in ((8, 8), (4, 64)):
        feat = _randn((m, heads, dim), torch.float16, 11)
        v = _randn((indices.numel(), heads), torch.float32, 12)
        _check_aggregate(indptr, indices, v, feat, n, voltrix.spmm_heads(indptr, indices, v, feat, n))
    z = voltrix.spmm_heads(torch.zeros(n + 1, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"),
                           torch.zeros(0, 8, device="cuda"), _randn((m, 8, 8), torch.float16, 1), n)
    assert z.shape == (n, 8, 8) and bool((z == 0).all())


# ---- autograd -------------------------------------------------------------------------------------------------------------------------
def _grad_bound_ok(grad, ref, scale, deg, dtype):
    """The aggregation's bound (one more rounding for the sum's last step, as tests/test_gpu_sddmm.py) plus the cast to ``dtype``."""
    return bool(((grad.double() - ref).abs() <= (deg + 1) * 2.0 ** -23 * scale + RND[dtype] * ref.abs() + 1e-30).all())


@pytest.mark.parametrize("pair", [(torch.float32, torch.float16), (torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16)])
@pytest.mark.parametrize("shape", [(4, 16), (3, 20), (8, 8)])
def test_autograd_sddmm_heads_gradients(cuda_device, pair, shape):
    from voltrix.autograd import SDDMM

    indptr, indices, n, m = _graph("special")
    heads, dim = shape
    op = SDDMM(indptr, indices, n, m)
    x = _randn((n, heads, dim), pair[0], 21).requires_grad_(True)
    y = _randn((m, heads, dim), pair[1], 22).requires_grad_(True)
    w = _randn((indices.numel(), heads), torch.float32, 23)
    s = op(x, y)
    _check_sddmm(indptr, indices, x.detach(), y.detach(), s.detach(), False, single_head_bits=False)
    (s * w).sum().backward()
    assert x.grad.dtype == x.dtype and y.grad.dtype == y.dtype and x.grad.shape == x.shape and y.grad.shape == y.shape
    # float64 torch autograd on the per-head gathered model
    rows, cols = _rows(indptr), indices.long()
    x64, y64 = x.detach().double().requires_grad_(True), y.detach().double().requires_grad_(True)
    ((x64[rows] * y64[cols]).sum(2) * w.double()).sum().backward()
    t_indptr, t_indices = voltrix.autograd.csr_transpose_device(indptr, indices, n, m)
    for h, _, scale, deg in _aggregate_ref(indptr, indices, w, y.detach(), n):
        assert _grad_bound_ok(x.grad[:, h], x64.grad[:, h], scale, deg, x.dtype), h
    for h, _, scale, deg in _aggregate_ref(t_indptr, t_indices, w[op.t_order], x.detach(), m):
        assert _grad_bound_ok(y.grad[:, h], y64.grad[:, h], scale, deg, y.dtype), h


def _segment_softmax64(indptr, s, scale):
    """The torch composite in float64 on the host, [nnz, H] (index_add on the device contends on hub rows)."""
    indptr = indptr.cpu()
    rows = _rows(indptr)
    n = indptr.numel() - 1
    z = s * scale
    idx = rows[:, None].expand_as(z)
    m = torch.full((n, z.shape[1]), -INF, dtype=z.dtype).scatter_reduce(0, idx, z.detach(), "amax")
    e = torch.exp(z - m[rows])
    return e / torch.zeros(n, z.shape[1], dtype=z.dtype).index_add(0, rows, e)[rows]


def test_autograd_edge_softmax_heads(cuda_device):
    from voltrix.autograd import EdgeSoftmax

    indptr = _graph("special")[0]
    n, nnz = indptr.numel() - 1, int(indptr[-1])
    op = EdgeSoftmax(indptr, n)
    scores = (torch.randn(nnz, 4, device="cuda") * 3).requires_grad_(True)
    w = torch.randn(nnz, 4, device="cuda")
    alpha = op(scores, 0.4)
    (alpha * w).sum().backward()
    assert torch.equal(alpha.detach(), voltrix.edge_softmax(indptr, scores.detach(), 0.4))
    assert torch.equal(scores.grad, edge_softmax_backward(indptr, alpha.detach(), w, 0.4))
    _check_forward(indptr, scores.detach(), 0.4, alpha.detach())
    _check_backward(indptr, alpha.detach(), w, 0.4, scores.grad)
    s64 = scores.detach().double().cpu().requires_grad_(True)
    (_segment_softmax64(indptr, s64, 0.4) * w.double().cpu()).sum().backward()
    for h in range(4):
        assert float((scores.grad[:, h].double().cpu() - s64.grad[:, h]).norm() / s64.grad[:, h].norm()) <= 1e-5, h
    half = scores.detach().half().requires_grad_(True)      # fp16 scores: the gradient comes back in fp16
    (op(half, 0.4) * w).sum().backward()
    assert half.grad.dtype == torch.float16 and half.grad.shape == (nnz, 4)


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("shape", [(4, 16), (3, 20), (8, 8)])
def test_autograd_spmm_heads_gradients(cuda_device, dtype, shape):
    from voltrix.autograd import SpMMHeads

    indptr, indices, n, m = _graph("special")
    heads, dim = shape
    nnz = indices.numel()
    op = SpMMHeads(indptr, indices, n, m)
    assert not hasattr(op, "handle") and not hasattr(op, "weighted")          # no reference-format handle
    feat = _randn((m, heads, dim), dtype, 31).requires_grad_(True)
    v = _randn((nnz, heads), torch.float32, 32).requires_grad_(True)
    w = _randn((n, heads, dim), torch.float32, 33)
    out = op(feat, v)
    _check_aggregate(indptr, indices, v.detach(), feat.detach(), n, out.detach(), single_head_bits=False)
    (out * w).sum().backward()
    assert feat.grad.dtype == dtype and feat.grad.shape == feat.shape and v.grad.dtype == torch.float32 and v.grad.shape == v.shape
    # float64 torch autograd on the per-head gathered model
    rows, cols = _rows(indptr), indices.long()
    f64, v64 = feat.detach().double().requires_grad_(True), v.detach().double().requires_grad_(True)
    out64 = torch.zeros(n, heads, dim, dtype=torch.float64, device="cuda").index_add(0, rows, v64[:, :, None] * f64[cols])
    (out64 * w.double()).sum().backward()
    # feat.grad = csr(v)^T @ w per head: the aggregation's bound on the transposed CSR, plus the cast to feat's dtype
    t_indptr, t_indices = voltrix.autograd.csr_transpose_device(indptr, indices, n, m)
    for h, _, scale, deg in _aggregate_ref(t_indptr, t_indices, v.detach()[op.t_order], w, m):
        assert _grad_bound_ok(feat.grad[:, h], f64.grad[:, h], scale, deg, dtype), h
    # v.grad[e, h] = <w[row_e, h], feat[col_e, h]>: the SDDMM's bound
    scale = (w.double().abs()[rows] * feat.detach().double().abs()[cols]).sum(2)
    assert bool(((v.grad.double() - v64.grad).abs() <= dim * 2.0 ** -23 * scale).all())
    # fp16 values: the gradient comes back in fp16
    vh = v.detach().half().requires_grad_(True)
    op(feat.detach(), vh).sum().backward()
    assert vh.grad.dtype == torch.float16


def _self_loop_graph(n, deg, seed):
    from test_hybrid_plan import _random_csr

    ip_np, ix_np = _random_csr(n, deg, seed=seed)
    rows_np = [np.unique(np.concatenate([ix_np[ip_np[r]:ip_np[r + 1]], [r]])) for r in range(n)]    # self loops: no empty row
    ip_np = np.concatenate([[0], np.cumsum([len(r) for r in rows_np])]).astype(np.int32)
    return torch.from_numpy(ip_np).cuda(), torch.from_numpy(np.concatenate(rows_np).astype(np.int32)).cuda()


def test_attention_layer_heads_against_single_head_layers(cuda_device, monkeypatch):
    """SpMMHeads(EdgeSoftmax(SDDMM(q, k), D^-0.5), v) with H = 4 against the four single-head layers SpMM(values=)(EdgeSoftmax(SDDMM))
    on contiguous slices.

    Scores and weights: the multi-head kernels reduce per head exactly as the single-head ones, so alpha[:, h] has the single-head
    bits.  Outputs: both aggregate the SAME alpha with fp16 v.  The multi-head kernel is within deg 2^-23 S of the exact product
    (S = sum_e |alpha| |v|).  The single-head SpMM(values=) installs alpha into an fp16 value plane (a rounding of 2^-11 |alpha|, or
    2^-25 absolute below fp16's normal range) and sums fp32 products in the block format's order over windows padded to 16 columns:
    within sum_e (2^-11 |alpha| + 2^-25) |v| + (deg + 16) 2^-23 S.  The difference is within the sum of the two.  Gradients: every
    weight gradient of both forms against a dense float64 masked-softmax model, 1e-2 in norm as in test_gpu_edge_softmax.py."""
    from voltrix.autograd import SDDMM, EdgeSoftmax, SpMM, SpMMHeads

    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "none")
    n, d_in, heads, dim = 2000, 32, 4, 16
    ip, ix = _self_loop_graph(n, 12, seed=47)
    rows, nnz = _rows(ip), ix.numel()
    torch.manual_seed(5)
    x = torch.randn(n, d_in, device="cuda")
    params = {k: torch.randn(d_in, heads * dim, device="cuda") / d_in ** 0.5 for k in ("wq", "wk", "wv")}
    w_out = torch.randn(n, heads, dim, device="cuda")

    scores_op, softmax, agg = SDDMM(ip, ix, n), EdgeSoftmax(ip, n), SpMMHeads(ip, ix, n)
    p = {k: t.clone().requires_grad_(True) for k, t in params.items()}
    q, k, v = ((x @ p[name]).view(n, heads, dim) for name in ("wq", "wk", "wv"))
    alpha = softmax(scores_op(q, k), dim ** -0.5)
    out = agg(v.half(), alpha)
    (out * w_out).sum().backward()

    single = SpMM(ip, ix, n, values=torch.ones(nnz, device="cuda"), hash_tag="heads_attention_single")
    ps = {k: t.clone().requires_grad_(True) for k, t in params.items()}
    qs, ks, vs = ((x @ ps[name]).view(n, heads, dim) for name in ("wq", "wk", "wv"))
    outs, alphas = [], []
    for h in range(heads):
        a_h = softmax(scores_op(qs[:, h].contiguous(), ks[:, h].contiguous()), dim ** -0.5)
        alphas.append(a_h)
        outs.append(single(vs[:, h].contiguous().half(), values=a_h))
    out_single = torch.stack(outs, 1)
    (out_single * w_out).sum().backward()

    deg = (ip[1:] - ip[:-1]).double()[:, None]
    for h in range(heads):
        assert torch.equal(alpha[:, h].detach(), alphas[h].detach()), h
        a64, v64 = alpha[:, h].detach().double(), v[:, h].detach().half().double().abs()
        s_abs = torch.zeros(n, dim, dtype=torch.float64, device="cuda").index_add(0, rows, a64[:, None] * v64[ix.long()])
        plane = torch.zeros(n, dim, dtype=torch.float64, device="cuda").index_add(
            0, rows, (2.0 ** -11 * a64 + 2.0 ** -25)[:, None] * v64[ix.long()])
        bound = deg * 2.0 ** -23 * s_abs + plane + (deg + 16) * 2.0 ** -23 * s_abs
        assert bool(((out[:, h].double() - out_single[:, h].double()).abs() <= bound).all()), h

    r = {k: t.double().clone().requires_grad_(True) for k, t in params.items()}
    x64 = x.double()
    q64, k64, v64 = ((x64 @ r[name]).view(n, heads, dim) for name in ("wq", "wk", "wv"))
    mask = torch.zeros(n, n, dtype=torch.bool, device="cuda")
    mask[rows, ix.long()] = True
    s = torch.einsum("nhd,mhd->hnm", q64, k64) * dim ** -0.5
    attn = torch.softmax(s.masked_fill(~mask, -INF), dim=2)
    ref = torch.einsum("hnm,mhd->nhd", attn, v64)
    (ref * w_out.double()).sum().backward()
    assert float((out.detach().double() - ref.detach()).norm() / ref.detach().norm()) <= 2e-3
    for name in params:
        for got in (p[name].grad, ps[name].grad):
            err = float((got.double() - r[name].grad).norm() / r[name].grad.norm())
            assert err <= 1e-2, (name, err)


def test_gat_example_with_heads(cuda_device, monkeypatch):
    """examples/gat_train.py: heads = 4 trains three epochs with a finite, decreasing loss through SpMMHeads; heads = 1 builds what it
    builds today (GATLayer on autograd.SpMM with values)."""
    from voltrix.autograd import SpMM, SpMMHeads

    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "none")
    sys.path.insert(0, os.path.join(REPO, "examples"))
    try:
        import gat_train
    finally:
        sys.path.remove(os.path.join(REPO, "examples"))
    n, in_feats, hidden, classes = 1500, 24, 32, 8
    ip, ix = _self_loop_graph(n, 10, seed=53)
    torch.manual_seed(9)
    graph = gat_train.Graph(ip, ix, n, hash_tag="heads_gat_test", heads=4)
    assert isinstance(graph.aggregate, SpMMHeads)
    model = gat_train.GAT(graph, in_feats, hidden, classes).cuda()
    assert isinstance(model.l1, gat_train.GATHeadsLayer) and model.l1.a_l.shape == (4, hidden // 4) and model.l2.a_l.shape == (4, classes)
    x = torch.randn(n, in_feats, device="cuda")
    y = torch.randint(0, classes, (n,), device="cuda")
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    losses = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        logits = model(x)
        assert logits.shape == (n, classes)
        loss = torch.nn.functional.cross_entropy(logits, y)
        loss.backward()
        assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in model.parameters())
        opt.step()
        losses.append(float(loss))
    assert all(np.isfinite(losses)) and losses[2] < losses[1] < losses[0], losses

    one = gat_train.Graph(ip, ix, n, hash_tag="heads_gat_test_one")          # the default: heads = 1
    assert one.heads == 1 and isinstance(one.aggregate, SpMM) and one.aggregate.weighted is not None
    model1 = gat_train.GAT(one, in_feats, hidden, classes)
    assert type(model1.l1) is gat_train.GATLayer and type(model1.l2) is gat_train.GATLayer and model1.l1.a_l.shape == (hidden,)
