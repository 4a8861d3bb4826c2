"""GPU: GAT edge scores (voltrix.gat_score, gat_score_kernels.hpp), the two segment sums of their backward and autograd.GATScore
against float64 on the host.

Oracle: ``z = el[row] + er[col]`` and ``s = z > 0 ? z : float32(slope) z`` in float64 from the float32 inputs; the segment sums by
``np.add.reduceat`` on the CSR and on a host-side stable sort by column.  Bounds (include/voltrix_capi.h; derived, not measured):
forward ``|s - ref| <= 1.5 * 2^-23 |ref| + 2^-149`` (``2^-24 |ref| + 2^-149`` for slope 1 or a power of two); sums
``|d - ref| <= deg * 2^-23 * sum |gz| + 2^-149`` per row (column) and head."""
import functools

import numpy as np
import pytest
import torch

import voltrix
from voltrix.gat_score import gat_score_backward

pytestmark = pytest.mark.gpu

CHUNK = 2048          # kChunkEdges: edges per workgroup of the forward and of the chunk sums
HUB_COL = 5


class _Graph:
    """A CSR pattern [num_rows, num_cols] on the host and on the device, with its transpose by a stable sort by column."""

    def __init__(self, lengths, cols, num_cols):
        lengths = np.asarray(lengths, np.int64)
        self.num_rows, self.num_cols, self.nnz = len(lengths), num_cols, int(lengths.sum())
        self.ip = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        self.cols = np.asarray(cols, np.int64)
        assert self.cols.size == self.nnz
        self.rows = np.repeat(np.arange(self.num_rows), lengths)
        self.order = np.argsort(self.cols, kind="stable")
        self.col_deg = np.bincount(self.cols, minlength=num_cols)
        self.t_ip = np.concatenate([[0], np.cumsum(self.col_deg)]).astype(np.int64)
        self.row_deg = lengths
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).astype(np.int32)).cuda()     # noqa: E731
        self.indptr, self.indices = dev(self.ip), dev(self.cols)
        self.t_indptr, self.t_indices, self.t_order = dev(self.t_ip), dev(self.rows[self.order]), dev(self.order)


def _special_lengths():
    """Empty rows, rows of length 1, CHUNK - 1, CHUNK and CHUNK + 1 at several offsets, a hub of 300 chunks + 17, a run of 20,000 empty
    rows, short random rows.  It opens with a row that fills chunk 0 exactly and one that starts on a chunk boundary."""
    rng = np.random.default_rng(7)
    lengths = [CHUNK, CHUNK + 1]
    for r in range(4000):
        if r % 13 == 0:
            lengths.append(0)
        elif r in (100, 900, 2500):
            lengths += [CHUNK - 1, CHUNK, CHUNK + 1, 0, 1]
        elif r == 1500:
            lengths.append(300 * CHUNK + 17)
        elif r == 3000:
            lengths += [0] * 20000
        elif r % 3 == 0:
            lengths.append(1)
        else:
            lengths.append(int(rng.integers(1, 40)))
    return lengths


@functools.lru_cache(maxsize=None)
def _special():
    lengths = _special_lengths()
    nnz, n = int(np.sum(lengths)), len(lengths)
    rng = np.random.default_rng(17)
    cols = rng.integers(0, n, nnz)
    cols[rng.random(nnz) < 0.25] = HUB_COL             # a hub column: the transposed pass crosses more than 64 chunks too
    g = _Graph(lengths, cols, n + 100)                  # the last 100 columns are never used
    assert g.col_deg[HUB_COL] >= 70 * CHUNK and g.nnz % CHUNK != 0 and g.nnz > 300 * CHUNK
    assert (g.col_deg == 0).sum() >= 100 and (g.row_deg == 0).sum() >= 20000
    return g


@functools.lru_cache(maxsize=None)
def _rect():
    rng = np.random.default_rng(3)
    lengths = rng.integers(0, 12, 37)
    lengths[[4, 20]] = 0
    cols = rng.integers(0, 4, int(lengths.sum()))       # column 4 of the 5 is never used; duplicates are certain
    return _Graph(lengths, cols, 5)


@functools.lru_cache(maxsize=None)
def _empty():
    return _Graph([0] * 9, [], 4)


def _inputs(graph, heads, seed, integer=False):
    """(el, er, g) float32 on the device: [n, H], or 1-D for heads = None."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    shape = lambda n: (n,) if heads is None else (n, heads)        # noqa: E731
    if integer:
        draw = lambda n: torch.randint(-8, 9, shape(n), device="cuda", generator=gen).float()     # noqa: E731
    else:
        draw = lambda n: torch.randn(shape(n), device="cuda", generator=gen)                       # noqa: E731
    return draw(graph.num_rows), draw(graph.num_cols), draw(graph.nnz)


def _np2(t):
    a = t.detach().double().cpu().numpy()
    return a.reshape(a.shape[0], -1)


def _segsum(x, ip):
    """Sum of x [nnz, H] over every segment of ip -> [segments, H], float64, zeros for empty segments."""
    deg = np.diff(ip)
    out = np.zeros((deg.size, x.shape[1]))
    if x.shape[0]:
        out[deg > 0] = np.add.reduceat(x, ip[:-1][deg > 0], axis=0)
    return out


@functools.lru_cache(maxsize=None)
def _pow2(slope):
    m = abs(float(np.float32(slope)))
    return m == 0 or np.log2(m) == np.floor(np.log2(m))


def _oracle(graph, el, er, slope, g=None):
    """float64: the scores and their bound; with g the two sums, their bounds and gz."""
    sl = float(np.float32(slope))
    z = _np2(el)[graph.rows] + _np2(er)[graph.cols]
    with np.errstate(invalid="ignore"):
        ref = np.where(z > 0, z, sl * z)
    bound = (2.0 ** -24 if _pow2(slope) else 1.5 * 2.0 ** -23) * np.abs(ref) + 2.0 ** -149
    if g is None:
        return ref, bound
    gd = _np2(g)
    gz = np.where(z > 0, gd, sl * gd)
    d_el, a_el = _segsum(gz, graph.ip), _segsum(np.abs(gz), graph.ip)
    d_er, a_er = _segsum(gz[graph.order], graph.t_ip), _segsum(np.abs(gz)[graph.order], graph.t_ip)
    b_el = graph.row_deg[:, None] * 2.0 ** -23 * a_el + 2.0 ** -149
    b_er = graph.col_deg[:, None] * 2.0 ** -23 * a_er + 2.0 ** -149
    return ref, bound, (d_el, b_el), (d_er, b_er), gz


def _within(out, ref, bound, what):
    err = np.abs(_np2(out) - ref)
    ratio = float((err / bound).max()) if err.size else 0.0
    print(f"{what}: max err / bound = {ratio:.3f}")
    assert bool((err <= bound).all()), (what, ratio)


def _sums(graph, el, er, g, slope):
    d_el = gat_score_backward(graph.indptr, graph.indices, el, er, g, slope)
    d_er = gat_score_backward(graph.t_indptr, graph.t_indices, er, el, g, slope, order=graph.t_order)
    return d_el, d_er


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _nan_filled_calls(graph, el, er, g, slope):
    """The three results through the C-ABI binding with every output buffer pre-filled with NaN, so an element that no kernel writes
    shows; each has the bits of the public call."""
    from voltrix import capi
    from voltrix.gat_score import workspace_bytes

    two = lambda t: t.view(-1, 1) if t.dim() == 1 else t                    # noqa: E731
    heads = two(g).shape[1]
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")     # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    s, d_el, d_er = nan(graph.nnz, heads), nan(graph.num_rows, heads), nan(graph.num_cols, heads)
    ws = torch.empty(workspace_bytes(graph.num_rows, graph.nnz, heads), dtype=torch.uint8, device="cuda")
    capi.launch_gat_score_csr(graph.indptr, graph.indices, graph.num_rows, two(el), two(er), slope, s, stream)
    capi.launch_gat_score_rowsum_csr(graph.indptr, graph.indices, None, graph.num_rows, two(el), two(er), two(g), slope, d_el, ws, stream)
    capi.launch_gat_score_rowsum_csr(graph.t_indptr, graph.t_indices, graph.t_order, graph.num_cols, two(er), two(el), two(g), slope,
                                     d_er, ws, stream)
    s, d_el, d_er = s.view(g.shape), d_el.view(el.shape), d_er.view(er.shape)
    assert _same_bits(s, voltrix.gat_score(graph.indptr, graph.indices, el, er, slope))
    assert all(_same_bits(a, b) for a, b in zip((d_el, d_er), _sums(graph, el, er, g, slope)))
    return s, d_el, d_er


@pytest.mark.parametrize("slope", [0.2, 0.0, 1.0, -0.5])
def test_forward_within_the_bound(cuda_device, slope):
    for graph in (_special(), _rect()):
        for heads in (None, 1, 2, 3, 8):
            el, er, g = _inputs(graph, heads, seed=11 + (heads or 0))
            s, _, _ = _nan_filled_calls(graph, el, er, g, slope)
            assert s.dtype == torch.float32 and s.shape == g.shape
            ref, bound = _oracle(graph, el, er, slope)
            _within(s, ref, bound, f"forward slope={slope} H={heads}")          # a NaN left in the buffer fails this
            if slope == 1.0:
                assert _same_bits(s, el[torch.from_numpy(graph.rows).cuda()] + er[graph.indices.long()])


@pytest.mark.parametrize("heads", [1, 3, 8])
def test_segment_sums_within_the_bound(cuda_device, heads):
    for graph in (_special(), _rect()):
        for slope in (0.2, -0.5):
            el, er, g = _inputs(graph, heads, seed=23 + heads)
            _, d_el, d_er = _nan_filled_calls(graph, el, er, g, slope)
            assert d_el.shape == (graph.num_rows, heads) and d_er.shape == (graph.num_cols, heads)
            _, _, (r_el, b_el), (r_er, b_er), _ = _oracle(graph, el, er, slope, g)
            _within(d_el, r_el, b_el, f"d_el slope={slope} H={heads}")
            _within(d_er, r_er, b_er, f"d_er slope={slope} H={heads}")
            assert bool((_bits(d_el)[torch.from_numpy(graph.row_deg == 0).cuda()] == 0).all())     # exactly +0
            assert bool((_bits(d_er)[torch.from_numpy(graph.col_deg == 0).cuda()] == 0).all())


def test_one_dimensional_sums_and_no_edges(cuda_device):
    graph = _rect()
    el, er, g = _inputs(graph, None, seed=5)
    s, d_el, d_er = _nan_filled_calls(graph, el, er, g, 0.2)
    assert s.shape == (graph.nnz,) and d_el.shape == (graph.num_rows,) and d_er.shape == (graph.num_cols,)
    s2, d_el2, d_er2 = _nan_filled_calls(graph, el[:, None], er[:, None], g[:, None], 0.2)
    assert _same_bits(s, s2[:, 0]) and _same_bits(d_el, d_el2[:, 0]) and _same_bits(d_er, d_er2[:, 0])
    # nnz == 0 with rows: no score, zero sums
    graph = _empty()
    for heads in (None, 3):
        el, er, g = _inputs(graph, heads, seed=6)
        s, d_el, d_er = _nan_filled_calls(graph, el, er, g, 0.2)
        assert s.numel() == 0 and s.shape == g.shape
        assert d_el.shape == el.shape and d_er.shape == er.shape
        assert bool((_bits(d_el) == 0).all()) and bool((_bits(d_er) == 0).all())


def test_integer_inputs_are_exact(cuda_device):
    """Values in [-8, 8] and slope = 0.25: every product is exact and every partial sum is a multiple of 1/4 below 2^22, so the result is
    float64's in any order -- the hub row and the hub column included."""
    graph = _special()
    for heads in (1, 3):
        el, er, g = _inputs(graph, heads, seed=31, integer=True)
        ref, _, (r_el, _), (r_er, _), gz = _oracle(graph, el, er, 0.25, g)
        assert _segsum(np.abs(gz), graph.ip).max() < 2 ** 22 and _segsum(np.abs(gz)[graph.order], graph.t_ip).max() < 2 ** 22
        s = voltrix.gat_score(graph.indptr, graph.indices, el, er, 0.25)
        d_el, d_er = _sums(graph, el, er, g, 0.25)
        assert np.array_equal(_np2(s), ref)
        assert np.array_equal(_np2(d_el), r_el) and np.array_equal(_np2(d_er), r_er)
        assert r_el[graph.row_deg.argmax()].any() and r_er[HUB_COL].any()


def test_z_equal_zero_takes_the_slope_branch(cuda_device):
    """el, er in {-2 .. 2}: a fifth of the edges have z == +0.  Forward: slope * (+0) with a negative slope is -0 (the z branch would give
    +0).  Backward: those edges contribute slope * g, exactly (integers, slope = -0.5)."""
    graph = _special()
    gen = torch.Generator(device="cuda").manual_seed(41)
    el = torch.randint(-2, 3, (graph.num_rows, 2), device="cuda", generator=gen).float()
    er = torch.randint(-2, 3, (graph.num_cols, 2), device="cuda", generator=gen).float()
    g = torch.randint(-8, 9, (graph.nnz, 2), device="cuda", generator=gen).float()
    s = voltrix.gat_score(graph.indptr, graph.indices, el, er, -0.5)
    z = _np2(el)[graph.rows] + _np2(er)[graph.cols]
    zero = torch.from_numpy(z == 0).cuda()
    assert int(zero.sum()) > graph.nnz // 10
    assert bool((_bits(s)[zero] == -2 ** 31).all())                  # -0.0
    ref, _, (r_el, _), (r_er, _), gz = _oracle(graph, el, er, -0.5, g)
    assert np.array_equal(gz[z == 0], -0.5 * _np2(g)[z == 0])
    d_el, d_er = _sums(graph, el, er, g, -0.5)
    assert np.array_equal(_np2(s), ref) and np.array_equal(_np2(d_el), r_el) and np.array_equal(_np2(d_er), r_er)
    # the rectangular pattern with el = -er on every edge: ReLU's gradient is zero everywhere
    rect = _rect()
    el, er = torch.full((rect.num_rows,), 1.5, device="cuda"), torch.full((rect.num_cols,), -1.5, device="cuda")
    g1 = torch.ones(rect.nnz, device="cuda")
    d_el, d_er = _sums(rect, el, er, g1, 0.0)
    assert bool((d_el == 0).all()) and bool((d_er == 0).all())
    d_el, d_er = _sums(rect, el, er, g1, 3.0)
    assert np.array_equal(_np2(d_el)[:, 0], 3.0 * rect.row_deg) and np.array_equal(_np2(d_er)[:, 0], 3.0 * rect.col_deg)


@pytest.mark.parametrize("heads", [8, 3])
def test_every_head_has_the_bits_of_the_single_head_call(cuda_device, heads):
    graph = _special()
    el, er, g = _inputs(graph, heads, seed=53)
    s = voltrix.gat_score(graph.indptr, graph.indices, el, er, 0.2)
    d_el, d_er = _sums(graph, el, er, g, 0.2)
    for h in range(heads):
        el1, er1, g1 = el[:, h].contiguous(), er[:, h].contiguous(), g[:, h].contiguous()
        assert _same_bits(s[:, h], voltrix.gat_score(graph.indptr, graph.indices, el1, er1, 0.2)), h
        d_el1, d_er1 = _sums(graph, el1, er1, g1, 0.2)
        assert _same_bits(d_el[:, h], d_el1) and _same_bits(d_er[:, h], d_er1), h


def test_special_values_stay_local(cuda_device):
    graph = _special()
    heads = 3
    el, er, g = _inputs(graph, heads, seed=61)
    clean_s = voltrix.gat_score(graph.indptr, graph.indices, el, er, 0.2)
    clean_el, clean_er = _sums(graph, el, er, g, 0.2)
    hub = int(graph.row_deg.argmax())
    r0, c0, e0 = hub, 77, int(graph.ip[hub]) + 5 * CHUNK + 3        # a NaN in the hub row's scalar, +inf in a column's, a NaN in one gradient
    assert graph.col_deg[c0] > 0
    el2, er2, g2 = el.clone(), er.clone(), g.clone()
    el2[r0, 0] = float("nan")
    er2[c0, 1] = float("inf")
    g2[e0, 2] = float("nan")
    s = voltrix.gat_score(graph.indptr, graph.indices, el2, er2, 0.2)
    in_row = torch.zeros(graph.nnz, heads, dtype=torch.bool, device="cuda")
    in_row[graph.ip[r0]:graph.ip[r0 + 1], 0] = True
    in_col = torch.zeros_like(in_row)
    in_col[:, 1] = graph.indices == c0
    assert bool(torch.isnan(s[in_row]).all()) and bool((s[in_col] == float("inf")).all())
    keep = ~(in_row | in_col)
    assert torch.equal(_bits(s)[keep], _bits(clean_s)[keep])
    # a NaN gradient reaches the one row sum and the one column sum that hold it
    d_el, d_er = _sums(graph, el, er, g2, 0.2)
    row_e, col_e = int(graph.rows[e0]), int(graph.cols[e0])
    assert bool(torch.isnan(d_el[row_e, 2])) and bool(torch.isnan(d_er[col_e, 2]))
    m_el = torch.ones_like(d_el, dtype=torch.bool)
    m_el[row_e, 2] = False
    m_er = torch.ones_like(d_er, dtype=torch.bool)
    m_er[col_e, 2] = False
    assert torch.equal(_bits(d_el)[m_el], _bits(clean_el)[m_el]) and torch.equal(_bits(d_er)[m_er], _bits(clean_er)[m_er])
    # the gate only tests z: a NaN or inf scalar puts no NaN into a sum, and changes only the sums that hold its edges
    d_el, d_er = _sums(graph, el2, er2, g, 0.2)
    assert bool(torch.isfinite(d_el).all()) and bool(torch.isfinite(d_er).all())
    touched_el = torch.zeros_like(m_el)
    touched_el[r0, 0] = True
    touched_el[torch.from_numpy(np.unique(graph.rows[graph.cols == c0])).cuda(), 1] = True
    touched_er = torch.zeros_like(m_er)
    touched_er[c0, 1] = True
    touched_er[torch.from_numpy(np.unique(graph.cols[graph.ip[r0]:graph.ip[r0 + 1]])).cuda(), 0] = True
    assert torch.equal(_bits(d_el)[~touched_el], _bits(clean_el)[~touched_el])
    assert torch.equal(_bits(d_er)[~touched_er], _bits(clean_er)[~touched_er])


def _all_three(graph, el, er, g, slope):
    s = voltrix.gat_score(graph.indptr, graph.indices, el, er, slope)
    return (s,) + _sums(graph, el, er, g, slope)


def test_determinism_streams_graph_capture_and_no_host_sync(cuda_device):
    graph = _special()
    el, er, g = _inputs(graph, 3, seed=71)
    first = _all_three(graph, el, er, g, 0.2)                        # library loaded, allocator warm
    second = _all_three(graph, el, er, g, 0.2)
    assert all(_same_bits(a, b) for a, b in zip(first, second))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = _all_three(graph, el, er, g, 0.2)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(_same_bits(a, b) for a, b in zip(first, third))
    torch.cuda.set_sync_debug_mode("error")
    try:
        fourth = _all_three(graph, el, er, g, 0.2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(_same_bits(a, b) for a, b in zip(first, fourth))
    cuda_graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cuda_graph):
        captured = _all_three(graph, el, er, g, 0.2)
    cuda_graph.replay()
    torch.cuda.synchronize()
    assert all(_same_bits(a, b) for a, b in zip(first, captured))
    # fp16 scalars are cast to fp32 first
    h = el.half()
    assert _same_bits(voltrix.gat_score(graph.indptr, graph.indices, h, er, 0.2),
                      voltrix.gat_score(graph.indptr, graph.indices, h.float(), er, 0.2))


def test_autograd_gat_score(cuda_device):
    from voltrix.autograd import GATScore

    graph = _special()
    slope = 0.2
    op = GATScore(graph.indptr, graph.indices, graph.num_rows, graph.num_cols)
    assert op.t_order.dtype == torch.int32
    assert torch.equal(op.t_indptr, graph.t_indptr) and torch.equal(op.t_indices, graph.t_indices)
    for heads in (None, 3):
        el0, er0, w = _inputs(graph, heads, seed=83)
        el, er = el0.clone().requires_grad_(True), er0.clone().requires_grad_(True)
        s = op(el, er, slope)
        assert _same_bits(s.detach(), voltrix.gat_score(graph.indptr, graph.indices, el0, er0, slope))
        (s * w).sum().backward()
        d_el = gat_score_backward(op.indptr, op.indices, el0, er0, w, slope)
        d_er = gat_score_backward(op.t_indptr, op.t_indices, er0, el0, w, slope, order=op.t_order)
        assert _same_bits(el.grad, d_el) and _same_bits(er.grad, d_er)
        # the float64 torch composite on the host
        el64, er64 = el0.double().cpu().requires_grad_(True), er0.double().cpu().requires_grad_(True)
        rows, cols = torch.from_numpy(graph.rows), torch.from_numpy(graph.cols)
        s64 = torch.nn.functional.leaky_relu(el64[rows] + er64[cols], float(np.float32(slope)))
        (s64 * w.double().cpu()).sum().backward()
        _, _, (_, b_el), (_, b_er), _ = _oracle(graph, el0, er0, slope, w)
        _within(el.grad, _np2(el64.grad), b_el, f"autograd d_el H={heads}")
        _within(er.grad, _np2(er64.grad), b_er, f"autograd d_er H={heads}")
        # a second backward: the same bits
        el2, er2 = el0.clone().requires_grad_(True), er0.clone().requires_grad_(True)
        (op(el2, er2, slope) * w).sum().backward()
        assert _same_bits(el2.grad, el.grad) and _same_bits(er2.grad, er.grad)
        # one side without a gradient: None, and the other side unchanged
        el3, er3 = el0.clone().requires_grad_(True), er0.clone()
        (op(el3, er3, slope) * w).sum().backward()
        assert er3.grad is None and _same_bits(el3.grad, el.grad)
        el4, er4 = el0.clone(), er0.clone().requires_grad_(True)
        (op(el4, er4, slope) * w).sum().backward()
        assert el4.grad is None and _same_bits(er4.grad, er.grad)
    # fp16 scalars: the gradients come back in fp16; a transpose built elsewhere is accepted
    shared = GATScore(graph.indptr, graph.indices, graph.num_rows, graph.num_cols,
                      transposed=(op.t_indptr, op.t_indices, op.t_order.long()))
    el, er, w = _inputs(graph, 2, seed=89)
    el, er = el.half().requires_grad_(True), er.half().requires_grad_(True)
    (shared(el, er) * w).sum().backward()
    assert el.grad.dtype == torch.float16 and er.grad.dtype == torch.float16


def test_multi_head_gat_layer_end_to_end(cuda_device):
    """One multi-head GAT layer, SpMMHeads(wh, EdgeSoftmax(GATScore(el, er))), on a 300-node graph with H = 4, D = 8: the loss and the
    gradients of W, a_l, a_r against a dense float64 layer."""
    from voltrix.autograd import EdgeSoftmax, GATScore, SpMMHeads

    n, in_feats, heads, d = 300, 12, 4, 8
    rng = np.random.default_rng(97)
    rows_np = [np.unique(np.concatenate([rng.integers(0, n, int(rng.integers(0, 9))), [r]])) for r in range(n)]   # self loops
    ip = torch.from_numpy(np.concatenate([[0], np.cumsum([len(r) for r in rows_np])]).astype(np.int32)).cuda()
    ix = torch.from_numpy(np.concatenate(rows_np).astype(np.int32)).cuda()
    aggregate = SpMMHeads(ip, ix, n)
    score = GATScore(ip, ix, n, transposed=(aggregate.t_indptr, aggregate.t_indices, aggregate.t_order))
    softmax = EdgeSoftmax(ip, n)
    torch.manual_seed(13)
    x = torch.randn(n, in_feats, device="cuda")
    y = torch.randint(0, d, (n,), device="cuda")
    params = {"w": torch.randn(in_feats, heads * d, device="cuda") / in_feats ** 0.5,
              "a_l": torch.randn(heads, d, device="cuda") / d ** 0.5, "a_r": torch.randn(heads, d, device="cuda") / d ** 0.5}

    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    wh = (x @ p["w"]).view(n, heads, d)
    s = score((wh * p["a_l"]).sum(-1), (wh * p["a_r"]).sum(-1), 0.2)
    out = aggregate(wh.half(), softmax(s))
    loss = torch.nn.functional.cross_entropy(out.mean(1), y)
    loss.backward()

    r = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    mask = torch.zeros(n, n, dtype=torch.bool, device="cuda")
    mask[torch.repeat_interleave(torch.arange(n, device="cuda"), (ip[1:] - ip[:-1]).long()), ix.long()] = True
    wh64 = (x.double() @ r["w"]).view(n, heads, d)
    el64, er64 = (wh64 * r["a_l"]).sum(-1), (wh64 * r["a_r"]).sum(-1)
    s64 = torch.nn.functional.leaky_relu(el64[:, None, :] + er64[None, :, :], 0.2)                 # [n, n, H]
    attn = torch.softmax(s64.masked_fill(~mask[:, :, None], -float("inf")), dim=1)
    out64 = torch.einsum("ijh,jhd->ihd", attn, wh64)
    ref_loss = torch.nn.functional.cross_entropy(out64.mean(1), y)
    ref_loss.backward()
    assert abs(float(loss) - float(ref_loss)) <= 2e-3 * abs(float(ref_loss))
    for name in params:
        err = float((p[name].grad.double() - r[name].grad).norm() / r[name].grad.norm())
        assert err <= 2e-2, (name, err)
