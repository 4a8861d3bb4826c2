"""GPU: the attention operators where an element offset passes 2^31 or an edge id comes near INT_MAX -- the offsets
``e * H + h``, ``col * H * D``, ``row * H * D`` and ``chunk * 2048 * H`` that the kernels form in 64 bits and that no other test reaches.

Four families, each at the smallest size that crosses the boundary (tests/large_offset_cases.py builds them; its CPU test checks the
helpers against small problems worked out directly):

  edge axis    [nnz, H] tensors with nnz * H just above 2^31: H = 64, nnz = 2^25 + 1,234, D one 16-byte piece; gat_score once more at
               H = 8 (nnz = 2^28 + 1,234) and H = 4 (2^29 + 1,234), its 16-byte branches.  The big inputs are one period repeated, the
               float64 reference is the period's, and every period of every big output is compared with it, element by element.
  column axis  a gathered operand [num_cols, H, D] with num_cols * H * D just above 2^31 (num_cols = 2^22 + 5, H D = 512), fp16 and
               fp32, through the autograd operators: the forward gathers from it, the backward writes its gradient on the transposed
               CSR.  The columns in use lie at the start, on either side of the rows where the offset passes 2^30 and 2^31, and at the end.
  row axis     the transposed pattern: out, x / xl and the incoming gradient [num_rows, H, D] are the big tensors, almost all rows empty.
  edge ids     single-head edge softmax, the keep mask's generator and every kernel that takes four edges at a time (single-head sddmm,
               gatv2_score, gatv2_rowsum, the CSR row-gather kernel, spmm_heads, attn_aggregate and d_s) at nnz = 2^31 - 1, the
               documented maximum.

Bounds: the operators' own, per element, computed for the period's rows; where a gradient comes back in fp16 the
cast's rounding is added (``large_offset_cases.cast_bound``, which says how it differs from ``_grad_bound_ok`` of tests/test_gpu_heads.py);
the restated oracles are compared with the originals in the first test.  Outputs that go through the C-ABI binding are pre-filled with NaN (the
mask with a pattern whose bits past H are set), so an element no kernel wrote fails its comparison; the public entry point must give
the same bits.  Every test states its peak memory beforehand (at most 64 GiB), asserts that so much is free -- it fails, it does not
skip -- and frees what it held; it prints its wall time and ``torch.cuda.max_memory_allocated()`` (``-s``; profiles/large_offsets/).
"""
import functools
import gc
import time

import numpy as np
import pytest
import torch

import large_offset_cases as loc
import voltrix
from test_attn_dropout_host import keep_bits, pack, threshold_of
from voltrix import capi
from voltrix.attn_aggregate import attn_aggregate, attn_aggregate_grad_feat, attn_aggregate_grad_scores
from voltrix.autograd import SDDMM, AttnAggregate, CsrPattern, GATv2Score, SpMMHeads
from voltrix.edge_softmax import edge_softmax_backward, workspace_bytes as softmax_workspace_bytes
from voltrix.gat_score import gat_score_backward, workspace_bytes as gat_workspace_bytes
from voltrix.gatv2_score import gatv2_rowsum

pytestmark = pytest.mark.gpu

GIB = 1 << 30
H = 64                               # heads of the edge-axis family
NNZ = 2 ** 25 + 1234                 # NNZ * H = 2^31 + 78,976
NUM_COLS = 2042                      # the period on 1,021 columns, the tail on the other 1,021
BIG = 8.1                            # GiB of one [NNZ, H] float32 tensor (and of every other 2^31-element float32 tensor here), rounded up
SLABS = 4                            # GiB of float64 temporaries of one comparison slab, rounded up
SEED, OFFSET = 2 ** 63 + 12345, 2 ** 33 + 7
P_DROP = 0.6
KS = float(np.float32(1.0) / np.float32(1.0 - P_DROP))
DT = {"fp16": torch.float16, "fp32": torch.float32}
COUNT, HD, AXIS_H, AXIS_D = 2 ** 22 + 5, 512, 8, 64      # the big node axis: COUNT * HD = 2^31 + 2,560 elements
SMALL = 300


@pytest.fixture(autouse=True)
def _measured(request, cuda_device):
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    start = time.perf_counter()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as error:      # a device fault: nothing more is started on the GPU
        pytest.exit(f"device error in {request.node.name}, no further test is started: {error}", returncode=3)
    print(f"\n[measured] {request.node.name}: {time.perf_counter() - start:.2f} s wall, max_memory_allocated "
          f"{torch.cuda.max_memory_allocated() / GIB:.2f} GiB")
    gc.collect()
    torch.cuda.empty_cache()


def teardown_module(module):
    _edge.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


def _need(gib):
    """The test's peak need, stated before anything is allocated, in units of BIG: what the test holds at its peak, torch's temporaries
    included, rounded up (the log under profiles/large_offsets/ has the measured peaks).  It must fit 64 GiB and be free now."""
    assert gib <= 64, gib
    free, total = torch.cuda.mem_get_info()
    assert free >= gib * GIB, f"this test needs {gib:.1f} GiB of device memory, {free / GIB:.1f} GiB of {total / GIB:.1f} GiB are free"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _randn(shape, seed, dtype=torch.float32):
    return torch.randn(shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed)).to(dtype)


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@functools.lru_cache(maxsize=None)
def _edge():
    """The edge-axis pattern and its device transpose, shared by the tests of the family (0.7 GiB) and never written."""
    pc = loc.make_periodic(NNZ, NUM_COLS, "cuda")
    assert pc.nnz * H > 2 ** 31 and (pc.nnz - 1) * H < 2 ** 31 + 2 ** 17 and 2000 < pc.num_rows < 100_000
    return pc, CsrPattern(pc.indptr(), pc.indices(), pc.num_rows, pc.num_cols)


def _scores(pc, heads, seed):
    """Period scores [P_e, heads]: normal with deviation 2, the row of chunk + 1 edges spread over 60, a few -inf entries and one row of
    three edges that is all -inf in the last head."""
    s = 2.0 * _randn((pc.P_e, heads), seed)
    ip, lengths = pc.period.ip, pc.period.lengths
    wide = int(np.flatnonzero(lengths == loc.CHUNK + 1)[0])
    b, e = int(ip[wide]), int(ip[wide + 1])
    s[b:e] = torch.linspace(-30.0, 30.0, e - b, device="cuda")[:, None] + 0.25 * s[b:e]
    gen = torch.Generator(device="cuda").manual_seed(seed + 1)
    pick = torch.randint(0, pc.P_e, (12,), device="cuda", generator=gen)
    s[pick, torch.randint(0, heads, (12,), device="cuda", generator=gen)] = float("-inf")
    masked = int(np.flatnonzero(lengths == 3)[0])
    s[int(ip[masked]):int(ip[masked + 1]), heads - 1] = float("-inf")
    return s


def _tiled(pc, out, period, tail, what, tally):
    ok, worst = loc.check_tiled(out, pc.reps, period, tail, what, tally)
    assert ok, (what, worst)


def _whole(out, ref, bound, what, tally):
    ok, worst = loc.check_whole(out, ref, bound, what, tally)
    assert ok, (what, worst)


# ============================================================================================= the oracles are the operators' own
def test_the_restated_oracles_give_the_values_and_bounds_of_the_operators_own_tests(cuda_device):
    """tests/large_offset_cases.py restates the oracles of the operators' GPU tests so that they run on any device and on a graph given
    by ids.  This keeps the two in step: on the other tests' own patterns and inputs, every value and every bound agrees to float64
    rounding (the sums are taken in another order)."""
    import test_gpu_attn_aggregate as t_attn
    import test_gpu_attn_dropout as t_drop
    import test_gpu_gat_score as t_gat
    import test_gpu_gatv2 as t_v2
    import test_gpu_heads as t_heads

    _need(2)

    def close(got, want):
        want = torch.from_numpy(np.ascontiguousarray(want)).cuda() if isinstance(want, np.ndarray) else want
        torch.testing.assert_close(got.reshape(want.shape), want, rtol=1e-9, atol=1e-300)

    def col_deg(g):
        return torch.from_numpy(g.col_deg_np).double().cuda()

    # attn_aggregate, without and with a keep mask
    graph = t_attn._special()
    g = loc.Graph(graph.lengths, graph.cols_np, graph.num_cols, "cuda")
    s, feat, grad = t_attn._inputs("special", 8, 8, "fp16")
    _, keep, ks = t_drop._mask("special", 8, 8, "fp16", "p0.6")
    for want, got in ((t_attn._oracle(graph, s, feat, grad, 0.5), loc.attn_oracle(g, s, feat, grad, 0.5)),
                      (t_drop._oracle(graph, s, feat, grad, 0.5, keep, ks), loc.attn_oracle(g, s, feat, grad, 0.5, keep, ks))):
        for name in ("out", "l", "d_s"):
            close(got[name][0], want[name][0])
            close(got[name][1], want[name][1])
        assert torch.equal(got["m"], want["m"])
        d_feat = loc.d_feat_of(col_deg(g), {k: g.col_sum(v) for k, v in got["cols"].items()})
        close(d_feat[0], want["d_feat"][0])
        close(d_feat[1], want["d_feat"][1])
    # the edge softmax's reference (tests/test_gpu_heads.py states its bounds inside its checks) and its bound from that file's pieces
    indptr = torch.from_numpy(g.ip.astype(np.int32)).cuda()
    ref, z, mr, deg, _ = t_heads._ref_softmax(indptr, s[:, 0], 0.5)
    with np.errstate(invalid="ignore"):
        gap = np.nan_to_num(np.abs(z - mr), nan=0.0, posinf=0.0)
    alpha, bound = loc.softmax_oracle(g, s, 0.5)
    close(alpha[:, 0], ref)
    close(bound[:, 0], ref * 2 * (deg + gap + 2) * 2.0 ** -23 + 2.0 ** -126)
    # GATv2
    graph = t_v2._special()
    g = loc.Graph(np.diff(graph.ip), graph.cols_np, graph.num_cols, "cuda")
    xl, xr, a, w = t_v2._inputs("special", 3, 20, "fp32")
    want = t_v2._oracle(graph, xl, xr, a, 0.2, w)
    forward, left, term = loc.gatv2_oracle(g, xl, xr, a, 0.2, w)
    right = (g.col_sum(term), loc.column_bound(col_deg(g), g.col_sum(term.abs())))
    for got_pair, want_pair in zip((forward, left, right), want):
        close(got_pair[0], want_pair[0])
        close(got_pair[1], want_pair[1])
    # GAT
    graph = t_gat._rect()
    g = loc.Graph(graph.row_deg, graph.cols, graph.num_cols, "cuda")
    for slope in (0.2, 0.25):
        el, er, w = t_gat._inputs(graph, 3, seed=5)
        ref, bound, d_el, d_er, gz = t_gat._oracle(graph, el, er, slope, w)
        forward, left, terms = loc.gat_oracle(g, el, er, slope, w)
        right = (g.col_sum(terms), loc.column_bound(col_deg(g), g.col_sum(terms.abs())))
        for got_pair, want_pair in zip((forward, left, right), ((ref, bound), d_el, d_er)):
            close(got_pair[0], want_pair[0])
            close(got_pair[1], want_pair[1])


# ================================================================================================================ the edge axis
def test_edge_axis_device_transpose_of_the_periodic_pattern(cuda_device):
    _need(6)
    pc, pattern = _edge()
    t_indptr, t_indices, t_order = pc.transposed()
    assert pattern.t_order.dtype == torch.int32 and pattern.t_indptr.dtype == torch.int32
    assert torch.equal(pattern.t_indptr, t_indptr), "t_indptr"
    assert torch.equal(pattern.t_indices, t_indices), "t_indices"
    assert torch.equal(pattern.t_order, t_order), "t_order"
    assert torch.equal(pattern.indices[pattern.t_order.long()], torch.repeat_interleave(
        torch.arange(pc.num_cols, device="cuda", dtype=torch.int32), (t_indptr[1:] - t_indptr[:-1]).long()))


def test_edge_axis_sddmm_heads(cuda_device):
    _need(2 * BIG + SLABS + 1)
    pc, pattern = _edge()
    x_p, y = _randn((pc.P, H, 8), 1, torch.float16), _randn((NUM_COLS, H, 8), 2, torch.float16)
    x = pc.tile_rows(x_p)
    out = _nan(pc.nnz, H)
    capi.launch_sddmm_heads_csr(pattern.indptr, pattern.indices, pc.num_rows, x, y, out, _stream())
    tally = loc.Tally()
    _tiled(pc, out, loc.sddmm_oracle(pc.period, x_p, y), loc.sddmm_oracle(pc.tail, x_p[:pc.tail_rows], y), "sddmm out", tally)
    tally.assert_complete("sddmm out")
    assert _same_bits(out, voltrix.sddmm(pattern.indptr, pattern.indices, x, y))


def test_edge_axis_edge_softmax_forward_and_backward(cuda_device):
    _need(4 * BIG + SLABS + 1)
    pc, pattern = _edge()
    p, t, scale = pc.period, pc.tail, 0.75
    s_p = _scores(pc, H, 3)
    ref_p, ref_t = loc.softmax_oracle(p, s_p, scale), loc.softmax_oracle(t, s_p[:pc.tail_e], scale)
    ws = torch.empty(softmax_workspace_bytes(pc.num_rows, pc.nnz, H), dtype=torch.uint8, device="cuda")
    tally = loc.Tally()
    s = pc.tile_edges(s_p)
    alpha = _nan(pc.nnz, H)
    capi.launch_edge_softmax_heads_csr(pattern.indptr, pc.num_rows, s, scale, alpha, ws, _stream())
    _tiled(pc, alpha, ref_p, ref_t, "edge_softmax alpha", tally)
    assert _same_bits(alpha, voltrix.edge_softmax(pattern.indptr, s, scale))
    del s, alpha
    # the backward takes the float32 of the exact alpha, which is periodic (the kernel's own is, but not bit for bit), and a periodic g
    a_p, a_t, g_p = ref_p[0].float(), ref_t[0].float(), _randn((pc.P_e, H), 4)
    a, g = pc.tile_edges(a_p, a_t), pc.tile_edges(g_p)
    grad = _nan(pc.nnz, H)
    capi.launch_edge_softmax_heads_backward_csr(pattern.indptr, pc.num_rows, a, g, scale, grad, ws, _stream())
    _tiled(pc, grad, loc.softmax_backward_oracle(p, a_p, g_p, scale), loc.softmax_backward_oracle(t, a_t, g_p[:pc.tail_e], scale),
           "edge_softmax grad", tally)
    tally.assert_complete("edge_softmax alpha", "edge_softmax grad")
    assert _same_bits(grad, edge_softmax_backward(pattern.indptr, a, g, scale))


def test_edge_axis_spmm_heads(cuda_device):
    _need(BIG + SLABS + 1)
    pc, pattern = _edge()
    v_p, feat = _randn((pc.P_e, H), 5), _randn((NUM_COLS, H, 8), 6, torch.float16)
    v = pc.tile_edges(v_p)
    out = _nan(pc.num_rows, H, 8)
    capi.launch_spmm_csr_heads(pattern.indptr, pattern.indices, v, pc.num_rows, feat, out, _stream())
    tally = loc.Tally()
    _tiled(pc, out, loc.aggregate_oracle(pc.period, v_p, feat), loc.aggregate_oracle(pc.tail, v_p[:pc.tail_e], feat), "spmm_heads out", tally)
    tally.assert_complete("spmm_heads out")
    assert _same_bits(out, voltrix.spmm_heads(pattern.indptr, pattern.indices, v, feat, pc.num_rows))
    empty = torch.from_numpy(np.concatenate([np.tile(pc.period.lengths, pc.reps), pc.tail.lengths]) == 0).cuda()
    assert int(empty.sum()) >= 3 * pc.reps and bool((out[empty].view(torch.int32) == 0).all())          # empty rows: +0


def test_edge_axis_gat_score_and_both_sums_of_its_backward(cuda_device):
    _need(3 * BIG + SLABS + 1)
    pc, pattern = _edge()
    p, t, slope = pc.period, pc.tail, 0.2
    el_p, er, g_p = _randn((pc.P, H), 7), _randn((NUM_COLS, H), 8), _randn((pc.P_e, H), 9)
    el = pc.tile_rows(el_p)
    (f_p, r_p, gz_p), (f_t, r_t, gz_t) = loc.gat_oracle(p, el_p, er, slope, g_p), loc.gat_oracle(t, el_p[:pc.tail_rows], er, slope, g_p[:pc.tail_e])
    tally = loc.Tally()
    s = _nan(pc.nnz, H)
    capi.launch_gat_score_csr(pattern.indptr, pattern.indices, pc.num_rows, el, er, slope, s, _stream())
    _tiled(pc, s, f_p, f_t, "gat_score out", tally)
    assert _same_bits(s, voltrix.gat_score(pattern.indptr, pattern.indices, el, er, slope))
    del s
    g = pc.tile_edges(g_p)
    ws = torch.empty(gat_workspace_bytes(max(pc.num_rows, NUM_COLS), pc.nnz, H), dtype=torch.uint8, device="cuda")
    d_el, d_er = _nan(pc.num_rows, H), _nan(NUM_COLS, H)
    capi.launch_gat_score_rowsum_csr(pattern.indptr, pattern.indices, None, pc.num_rows, el, er, g, slope, d_el, ws, _stream())
    capi.launch_gat_score_rowsum_csr(pattern.t_indptr, pattern.t_indices, pattern.t_order, NUM_COLS, er, el, g, slope, d_er, ws, _stream())
    _tiled(pc, d_el, r_p, r_t, "gat_score d_el", tally)
    _whole(d_er, pc.col_sum(gz_p, gz_t), loc.column_bound(pc.col_deg(), pc.col_sum(gz_p.abs(), gz_t.abs())), "gat_score d_er (order)", tally)
    tally.assert_complete("gat_score out", "gat_score d_el", "gat_score d_er (order)")
    assert _same_bits(d_el, gat_score_backward(pattern.indptr, pattern.indices, el, er, g, slope))
    assert _same_bits(d_er, gat_score_backward(pattern.t_indptr, pattern.t_indices, er, el, g, slope, order=pattern.t_order))


@pytest.mark.parametrize("heads,nnz", [(8, 2 ** 28 + 1234), (4, 2 ** 29 + 1234)], ids=["H8", "H4"])
def test_edge_axis_gat_score_forward_of_the_16_byte_branches(cuda_device, heads, nnz):
    _need(2 * BIG + SLABS + 5)
    pc = loc.make_periodic(nnz, NUM_COLS, "cuda")
    assert pc.nnz * heads > 2 ** 31
    indptr, indices = pc.indptr(), pc.indices()
    el_p, er = _randn((pc.P, heads), 10), _randn((NUM_COLS, heads), 11)
    el = pc.tile_rows(el_p)
    s = _nan(pc.nnz, heads)
    capi.launch_gat_score_csr(indptr, indices, pc.num_rows, el, er, 0.2, s, _stream())
    tally = loc.Tally()
    _tiled(pc, s, loc.gat_oracle(pc.period, el_p, er, 0.2), loc.gat_oracle(pc.tail, el_p[:pc.tail_rows], er, 0.2), f"gat_score out H={heads}", tally)
    tally.assert_complete(f"gat_score out H={heads}")
    assert _same_bits(s, voltrix.gat_score(indptr, indices, el, er, 0.2))


def test_edge_axis_gatv2_score_and_both_row_sums(cuda_device):
    _need(3 * BIG + SLABS + 2)
    pc, pattern = _edge()
    p, t, slope = pc.period, pc.tail, 0.2
    xl_p, xr, a = _randn((pc.P, H, 8), 12, torch.float16), _randn((NUM_COLS, H, 8), 13, torch.float16), _randn((H, 8), 14)
    g_p = _randn((pc.P_e, H), 15)
    xl = pc.tile_rows(xl_p)
    (f_p, r_p, term_p), (f_t, r_t, term_t) = (loc.gatv2_oracle(p, xl_p, xr, a, slope, g_p),
                                              loc.gatv2_oracle(t, xl_p[:pc.tail_rows], xr, a, slope, g_p[:pc.tail_e]))
    tally = loc.Tally()
    s = _nan(pc.nnz, H)
    capi.launch_gatv2_score_csr(pattern.indptr, pattern.indices, pc.num_rows, xl, xr, a, slope, s, _stream())
    _tiled(pc, s, f_p, f_t, "gatv2_score out", tally)
    assert _same_bits(s, voltrix.gatv2_score(pattern.indptr, pattern.indices, xl, xr, a, slope))
    del s
    g = pc.tile_edges(g_p)
    big_l, big_r = _nan(pc.num_rows, H, 8), _nan(NUM_COLS, H, 8)
    capi.launch_gatv2_rowsum_csr(pattern.indptr, pattern.indices, None, pc.num_rows, xl, xr, g, slope, big_l, _stream())
    capi.launch_gatv2_rowsum_csr(pattern.t_indptr, pattern.t_indices, pattern.t_order, NUM_COLS, xr, xl, g, slope, big_r, _stream())
    _tiled(pc, big_l, r_p, r_t, "gatv2_rowsum G_l", tally)
    _whole(big_r, pc.col_sum(term_p, term_t), loc.column_bound(pc.col_deg(), pc.col_sum(term_p.abs(), term_t.abs())),
           "gatv2_rowsum G_r (order)", tally)
    tally.assert_complete("gatv2_score out", "gatv2_rowsum G_l", "gatv2_rowsum G_r (order)")
    assert _same_bits(big_l, gatv2_rowsum(pattern.indptr, pattern.indices, xl, xr, g, slope))
    assert _same_bits(big_r, gatv2_rowsum(pattern.t_indptr, pattern.t_indices, xr, xl, g, slope, order=pattern.t_order))


def test_edge_axis_attn_aggregate_and_both_gradients(cuda_device):
    _need(3 * BIG + SLABS + 3)
    pc, pattern = _edge()
    p, t, scale = pc.period, pc.tail, 8 ** -0.5
    s_p, feat, dc_p = _scores(pc, H, 16), _randn((NUM_COLS, H, 8), 17, torch.float16), _randn((pc.P, H, 8), 18)
    ref_p = loc.attn_oracle(p, s_p, feat, dc_p, scale)
    ref_t = loc.attn_oracle(t, s_p[:pc.tail_e], feat, dc_p[:pc.tail_rows], scale)
    s, dc = pc.tile_edges(s_p), pc.tile_rows(dc_p)
    out, m, l = _nan(pc.num_rows, H, 8), _nan(pc.num_rows, H), _nan(pc.num_rows, H)
    capi.launch_attn_aggregate_csr(pattern.indptr, pattern.indices, s, pc.num_rows, feat, scale, out, m, l, _stream())
    tally = loc.Tally()
    _tiled(pc, out, ref_p["out"], ref_t["out"], "attn_aggregate out", tally)
    _tiled(pc, m, (ref_p["m"], None), (ref_t["m"], None), "attn_aggregate m", tally)
    _tiled(pc, l, ref_p["l"], ref_t["l"], "attn_aggregate l", tally)
    assert all(_same_bits(x, y) for x, y in zip((out, m, l), attn_aggregate(pattern.indptr, pattern.indices, s, feat, pc.num_rows, scale,
                                                                           return_stats=True)))
    delta = (dc * out).sum(-1)
    d_s, d_feat = _nan(pc.nnz, H), _nan(NUM_COLS, H, 8)
    capi.launch_attn_aggregate_grad_scores_csr(pattern.indptr, pattern.indices, pc.num_rows, dc, feat, s, m, l, delta, scale, d_s, _stream())
    capi.launch_attn_aggregate_grad_feat_csr(pattern.t_indptr, pattern.t_indices, pattern.t_order, NUM_COLS, dc, s, m, l, scale, d_feat,
                                             _stream())
    _tiled(pc, d_s, ref_p["d_s"], ref_t["d_s"], "attn_aggregate d_s", tally)
    sums = {k: pc.col_sum(ref_p["cols"][k], ref_t["cols"][k]) for k in ref_p["cols"]}
    _whole(d_feat, *loc.d_feat_of(pc.col_deg(), sums), "attn_aggregate d_feat (t_order)", tally)
    tally.assert_complete("attn_aggregate out", "attn_aggregate m", "attn_aggregate l", "attn_aggregate d_s", "attn_aggregate d_feat (t_order)")
    assert _same_bits(d_s, attn_aggregate_grad_scores(pattern.indptr, pattern.indices, dc, feat, s, m, l, delta, scale))
    assert _same_bits(d_feat, attn_aggregate_grad_feat(pattern.t_indptr, pattern.t_indices, pattern.t_order, dc, s, m, l, NUM_COLS, scale))


def test_edge_axis_attn_aggregate_with_a_keep_mask(cuda_device):
    """The keep mask is ``dropout_mask``'s for one period, repeated like every other per-edge input (the generator itself runs at the big
    edge ids in the last family, and the whole mask of ``dropout_mask(nnz, ...)`` in ``test_edge_axis_apply_dropout_mask``)."""
    _need(3 * BIG + SLABS + 3)
    pc, pattern = _edge()
    p, t, scale, dim = pc.period, pc.tail, 0.5, 4             # fp32 rows of one 16-byte piece
    s_p, feat, dc_p = _scores(pc, H, 19), _randn((NUM_COLS, H, dim), 20), _randn((pc.P, H, dim), 21)
    mask_p = voltrix.dropout_mask(pc.P_e, H, P_DROP, SEED, OFFSET)
    keep_p = loc.unpack_keep(mask_p, H)
    assert mask_p.shape == (pc.P_e, 2) and 0.39 < float(keep_p.double().mean()) < 0.41
    ref_p = loc.attn_oracle(p, s_p, feat, dc_p, scale, keep_p, KS)
    ref_t = loc.attn_oracle(t, s_p[:pc.tail_e], feat, dc_p[:pc.tail_rows], scale, keep_p[:pc.tail_e], KS)
    s, dc, mask = pc.tile_edges(s_p), pc.tile_rows(dc_p), pc.tile_edges(mask_p)
    out, m, l = _nan(pc.num_rows, H, dim), _nan(pc.num_rows, H), _nan(pc.num_rows, H)
    capi.launch_attn_aggregate_csr(pattern.indptr, pattern.indices, s, pc.num_rows, feat, scale, out, m, l, _stream(), mask, KS)
    tally = loc.Tally()
    _tiled(pc, out, ref_p["out"], ref_t["out"], "dropout out", tally)
    _tiled(pc, m, (ref_p["m"], None), (ref_t["m"], None), "dropout m", tally)
    _tiled(pc, l, ref_p["l"], ref_t["l"], "dropout l", tally)
    delta = (dc * out).sum(-1)
    d_s, d_feat = _nan(pc.nnz, H), _nan(NUM_COLS, H, dim)
    capi.launch_attn_aggregate_grad_scores_csr(pattern.indptr, pattern.indices, pc.num_rows, dc, feat, s, m, l, delta, scale, d_s, _stream(),
                                               mask, KS)
    capi.launch_attn_aggregate_grad_feat_csr(pattern.t_indptr, pattern.t_indices, pattern.t_order, NUM_COLS, dc, s, m, l, scale, d_feat,
                                             _stream(), mask, KS)
    _tiled(pc, d_s, ref_p["d_s"], ref_t["d_s"], "dropout d_s", tally)
    sums = {k: pc.col_sum(ref_p["cols"][k], ref_t["cols"][k]) for k in ref_p["cols"]}
    _whole(d_feat, *loc.d_feat_of(pc.col_deg(), sums), "dropout d_feat (t_order)", tally)
    tally.assert_complete("dropout out", "dropout m", "dropout l", "dropout d_s", "dropout d_feat (t_order)")
    got = attn_aggregate(pattern.indptr, pattern.indices, s, feat, pc.num_rows, scale, return_stats=True, mask=mask, keep_scale=KS)
    assert all(_same_bits(x, y) for x, y in zip((out, m, l), got))
    assert _same_bits(d_s, attn_aggregate_grad_scores(pattern.indptr, pattern.indices, dc, feat, s, m, l, delta, scale, mask=mask, keep_scale=KS))
    assert _same_bits(d_feat, attn_aggregate_grad_feat(pattern.t_indptr, pattern.t_indices, pattern.t_order, dc, s, m, l, NUM_COLS, scale,
                                                       mask=mask, keep_scale=KS))


def test_edge_axis_apply_dropout_mask(cuda_device):
    _need(6 * BIG + 1)                                        # alpha, the result and the plain-torch temporaries of the call
    pc, _ = _edge()
    alpha_p = torch.rand((pc.P_e, H), device="cuda", generator=torch.Generator(device="cuda").manual_seed(22))
    alpha = pc.tile_edges(alpha_p)
    mask = voltrix.dropout_mask(pc.nnz, H, P_DROP, SEED, OFFSET)
    got = voltrix.apply_dropout_mask(alpha, mask, KS)
    assert got.dtype == torch.float32 and got.shape == alpha.shape
    scaled = alpha_p * KS                                      # one float32 product; a dropped entry is +0 by selection
    visited, ok = 0, torch.ones((), dtype=torch.bool, device="cuda")
    k = max(1, (1 << 26) // alpha_p.numel())
    for lo in list(range(0, pc.reps, k)) + [None]:
        if lo is None:
            e0, e1, want = pc.reps * pc.P_e, pc.nnz, scaled[:pc.tail_e]
        else:
            n = min(k, pc.reps - lo)
            e0, e1, want = lo * pc.P_e, (lo + n) * pc.P_e, scaled.repeat(n, 1)
        want = torch.where(loc.unpack_keep(mask[e0:e1], H), want, torch.zeros_like(want))
        ok = ok & (got[e0:e1].view(torch.int32) == want.view(torch.int32)).all()
        visited += want.numel()
    assert visited == got.numel() and bool(ok)


# ===================================================================================================== edge ids near INT_MAX
def test_edge_ids_single_head_edge_softmax_at_int_max(cuda_device):
    _need(4 * BIG + SLABS + 1)
    nnz = 2 ** 31 - 1
    pc = loc.make_periodic(nnz, 2, "cuda", last_row_crosses=True)          # the column ids play no part
    assert pc.nnz == nnz and nnz % loc.CHUNK != 0 and pc.cut > 0 and nnz - pc.cut < (nnz - 1) // loc.CHUNK * loc.CHUNK
    p, t, scale = pc.period, pc.tail, 1.25
    indptr = pc.indptr()
    assert int(indptr[-1]) == nnz and indptr.numel() == pc.num_rows + 1
    s_p = _scores(pc, 1, 23)
    ref_p, ref_t = loc.softmax_oracle(p, s_p, scale), loc.softmax_oracle(t, s_p[:pc.tail_e], scale)
    ws = torch.empty(softmax_workspace_bytes(pc.num_rows, nnz), dtype=torch.uint8, device="cuda")
    tally = loc.Tally()
    s = pc.tile_edges(s_p)
    alpha = _nan(nnz, 1)
    capi.launch_edge_softmax_csr(indptr, pc.num_rows, s.view(-1), scale, alpha.view(-1), ws, _stream())
    _tiled(pc, alpha, ref_p, ref_t, "edge_softmax alpha at 2^31 - 1", tally)
    assert _same_bits(alpha, voltrix.edge_softmax(indptr, s, scale))                 # [nnz, 1]: the heads = 1 dispatch
    del s, alpha
    a_p, a_t, g_p = ref_p[0].float(), ref_t[0].float(), _randn((pc.P_e, 1), 24)
    a, g = pc.tile_edges(a_p, a_t), pc.tile_edges(g_p)
    grad = _nan(nnz, 1)
    capi.launch_edge_softmax_backward_csr(indptr, pc.num_rows, a.view(-1), g.view(-1), scale, grad.view(-1), ws, _stream())
    _tiled(pc, grad, loc.softmax_backward_oracle(p, a_p, g_p, scale), loc.softmax_backward_oracle(t, a_t, g_p[:pc.tail_e], scale),
           "edge_softmax grad at 2^31 - 1", tally)
    tally.assert_complete("edge_softmax alpha at 2^31 - 1", "edge_softmax grad at 2^31 - 1")
    assert _same_bits(grad, edge_softmax_backward(indptr, a, g, scale))


def test_edge_ids_kernels_that_step_an_edge_id_by_four_at_int_max(cuda_device):
    """nnz = 2^31 - 1 through every kernel whose loop takes four edges at a time -- single-head sddmm, gatv2_score and d_s by 128-edge
    chunks, the CSR row-gather kernel with values, spmm_heads, gatv2_rowsum and attn_aggregate by rows: the last chunk and the last
    row end at INT_MAX, where ``e + 4`` does not fit an int (the loops count their trips).  One head, rows of one
    16-byte piece of fp32; spmm_heads with two heads, its own kernel."""
    _need(5 * BIG + SLABS + 1)
    nnz = 2 ** 31 - 1
    pc = loc.make_periodic(nnz, NUM_COLS, "cuda", last_row_crosses=True)
    assert pc.nnz == nnz and nnz % 128 != 0 and pc.cut >= 2048
    p, t, tr, te, slope, scale = pc.period, pc.tail, pc.tail_rows, pc.tail_e, 0.2, 0.5
    indptr, indices = pc.indptr(), pc.indices()
    x_p, y, a = _randn((pc.P, 1, 4), 71), _randn((NUM_COLS, 1, 4), 72), _randn((1, 4), 73)
    x = pc.tile_rows(x_p)
    x2, y2 = x.view(-1, 4), y.view(-1, 4)
    tally = loc.Tally()
    # the kernels split by edges: sddmm, gatv2_score
    out = _nan(nnz, 1)
    capi.launch_sddmm_csr(indptr, indices, pc.num_rows, x2, y2, out.view(-1), _stream())
    _tiled(pc, out, loc.sddmm_oracle(p, x_p, y), loc.sddmm_oracle(t, x_p[:tr], y), "sddmm out at 2^31 - 1", tally)
    assert _same_bits(out.view(-1), voltrix.sddmm(indptr, indices, x2, y2))
    out.fill_(float("nan"))
    capi.launch_gatv2_score_csr(indptr, indices, pc.num_rows, x, y, a, slope, out, _stream())
    g_p = _randn((pc.P_e, 1), 74)
    (f_p, r_p, _), (f_t, r_t, _) = loc.gatv2_oracle(p, x_p, y, a, slope, g_p), loc.gatv2_oracle(t, x_p[:tr], y, a, slope, g_p[:te])
    _tiled(pc, out, f_p, f_t, "gatv2_score out at 2^31 - 1", tally)
    assert _same_bits(out.view(-1), voltrix.gatv2_score(indptr, indices, x2, y2, a.view(-1), slope))
    del out
    # the kernels that walk a row: gatv2_rowsum, the CSR row-gather kernel with values (spmm_heads with one head), spmm_heads
    g = pc.tile_edges(g_p)
    big_l = _nan(pc.num_rows, 1, 4)
    capi.launch_gatv2_rowsum_csr(indptr, indices, None, pc.num_rows, x, y, g, slope, big_l, _stream())
    _tiled(pc, big_l, r_p, r_t, "gatv2_rowsum G_l at 2^31 - 1", tally)
    assert _same_bits(big_l.view(-1, 4), gatv2_rowsum(indptr, indices, x2, y2, g.view(-1), slope))
    rows = _nan(pc.num_rows, 4)
    capi.launch_spmm_csr_rows(indptr, indices, pc.num_rows, y2, rows, _stream(), 1, values=g.view(-1))
    _tiled(pc, rows.view(-1, 1, 4), loc.aggregate_oracle(p, g_p, y), loc.aggregate_oracle(t, g_p[:te], y), "csr rows with values at 2^31 - 1",
           tally)
    assert _same_bits(rows.view(-1, 1, 4), voltrix.spmm_heads(indptr, indices, g, y, pc.num_rows))
    del g
    v_p, feat2 = _randn((pc.P_e, 2), 75), _randn((NUM_COLS, 2, 4), 76)
    v = pc.tile_edges(v_p)
    rows2 = _nan(pc.num_rows, 2, 4)
    capi.launch_spmm_csr_heads(indptr, indices, v, pc.num_rows, feat2, rows2, _stream())
    _tiled(pc, rows2, loc.aggregate_oracle(p, v_p, feat2), loc.aggregate_oracle(t, v_p[:te], feat2), "spmm_heads out at 2^31 - 1", tally)
    assert _same_bits(rows2, voltrix.spmm_heads(indptr, indices, v, feat2, pc.num_rows))
    del v
    # attn_aggregate: the forward by rows, d_s by chunks (x is the incoming gradient)
    s_p = _scores(pc, 1, 77)
    ref_p, ref_t = loc.attn_oracle(p, s_p, y, x_p, scale), loc.attn_oracle(t, s_p[:te], y, x_p[:tr], scale)
    s = pc.tile_edges(s_p)
    o, m, l = _nan(pc.num_rows, 1, 4), _nan(pc.num_rows, 1), _nan(pc.num_rows, 1)
    capi.launch_attn_aggregate_csr(indptr, indices, s, pc.num_rows, y, scale, o, m, l, _stream())
    _tiled(pc, o, ref_p["out"], ref_t["out"], "attn_aggregate out at 2^31 - 1", tally)
    _tiled(pc, m, (ref_p["m"], None), (ref_t["m"], None), "attn_aggregate m at 2^31 - 1", tally)
    _tiled(pc, l, ref_p["l"], ref_t["l"], "attn_aggregate l at 2^31 - 1", tally)
    delta = (x * o).sum(-1)
    d_s = _nan(nnz, 1)
    capi.launch_attn_aggregate_grad_scores_csr(indptr, indices, pc.num_rows, x, y, s, m, l, delta, scale, d_s, _stream())
    _tiled(pc, d_s, ref_p["d_s"], ref_t["d_s"], "attn_aggregate d_s at 2^31 - 1", tally)
    tally.assert_complete("sddmm out at 2^31 - 1", "gatv2_score out at 2^31 - 1", "gatv2_rowsum G_l at 2^31 - 1",
                          "csr rows with values at 2^31 - 1", "spmm_heads out at 2^31 - 1", "attn_aggregate out at 2^31 - 1",
                          "attn_aggregate d_s at 2^31 - 1")
    got = attn_aggregate(indptr, indices, s.view(-1), y2, pc.num_rows, scale, return_stats=True)
    assert all(_same_bits(u.reshape(-1), w.reshape(-1)) for u, w in zip((o, m, l), got))
    assert _same_bits(d_s.view(-1), attn_aggregate_grad_scores(indptr, indices, x2, y2, s.view(-1), m.view(-1), l.view(-1), delta.view(-1), scale))


@pytest.mark.parametrize("heads", [1, 33])
def test_edge_ids_dropout_mask_at_int_max(cuda_device, heads):
    nnz, words = 2 ** 31 - 1, (heads + 31) // 32
    _need(2 * words * BIG + 10)                               # the mask, the public call's, and the int64 slabs of the bit counts
    mask = torch.full((nnz, words), 0x5A5A5A5A, dtype=torch.int32, device="cuda")    # bits past H set: a word nobody wrote shows
    capi.launch_dropout_mask(nnz, heads, threshold_of(P_DROP), SEED, OFFSET, mask, _stream())
    for first in (0, 2 ** 30 - 2048, nnz - 4096):
        want = pack(keep_bits(4096, heads, threshold_of(P_DROP), SEED, OFFSET, first_edge=first))
        assert np.array_equal(mask[first:first + 4096].cpu().numpy().view(np.uint32), want), first
    valid = [(1 << min(32, heads - 32 * w)) - 1 for w in range(words)]
    kept, visited = 0, 0
    flat, step = mask.view(-1), (1 << 27) * words
    for lo in range(0, flat.numel(), step):
        block = flat[lo:lo + step].view(-1, words)
        for w in range(words):
            assert not bool(((block[:, w].to(torch.int64) & 0xFFFFFFFF) & ~valid[w]).any()), (lo, w)      # bits past H are zero
        kept += int(loc.popcount32(block).sum())
        visited += block.numel()
    assert visited == mask.numel()
    count = nnz * heads
    assert abs(kept / count - (1 - P_DROP)) <= 5 * (P_DROP * (1 - P_DROP) / count) ** 0.5, (kept, count)
    assert torch.equal(mask, voltrix.dropout_mask(nnz, heads, P_DROP, SEED, OFFSET))


# ============================================================================================== a big node axis: columns, rows
def _axis(big):
    case = loc.AxisCase(COUNT, HD, SMALL, big, "cuda")
    assert case.crosses() and case.count * HD > 2 ** 31
    return case, CsrPattern(case.indptr, case.indices, case.num_rows, case.num_cols)


def _big(dtype, seed):
    return _randn((COUNT, AXIS_H, AXIS_D), seed, dtype)


def _rows(out, case, ref, bound, what, tally):
    ok, worst = loc.check_rows(out, case.used_t, ref, bound, what, tally)
    assert ok, (what, worst)


def _axis_need(dtype):
    """GiB at the peak of an axis test: the big operand, its float32 gradient and the cast of it, the float32 temporaries of the
    generator and of the checks (measured: 26.4 GiB with fp16, 34.4 GiB with fp32)."""
    return (4 if dtype == "fp16" else 5) * BIG + 1


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_column_axis_sddmm_three_and_two_dimensional(cuda_device, dtype):
    _need(_axis_need(dtype))
    case, pattern = _axis("cols")
    g, used, dt = case.compact, case.used_t, DT[dtype]
    op = SDDMM(pattern)
    x, y = _randn((SMALL, AXIS_H, AXIS_D), 31, dt).requires_grad_(True), _big(dt, 32).requires_grad_(True)
    w = _randn((case.nnz, AXIS_H), 33)
    tally = loc.Tally()
    s = op(x, y)
    _whole(s.detach(), *loc.sddmm_oracle(g, x.detach(), y.detach()[used]), "SDDMM s", tally)
    (s * w).sum().backward()
    ref, bound = loc.aggregate_oracle(g, w, y.detach()[used], roundings=1)
    _whole(x.grad, ref, loc.cast_bound(ref, bound, dt), "SDDMM x.grad", tally)
    ref, bound = loc.aggregate_columns_oracle(g, w, x.detach(), roundings=1)
    assert y.grad.dtype == dt and y.grad.shape == y.shape
    _rows(y.grad, case, ref, loc.cast_bound(ref, bound, dt), "SDDMM y.grad [num_cols, H, D]", tally)
    y.grad = None
    # the 2-D form on the same memory: one head of H D columns
    x2 = x.detach().view(SMALL, HD).requires_grad_(True)
    y2 = y.detach().view(COUNT, HD).requires_grad_(True)
    s2 = op(x2, y2)
    g2 = (x2.detach().view(SMALL, 1, HD), y2.detach()[used].view(-1, 1, HD))
    ref, bound = loc.sddmm_oracle(g, *g2)
    _whole(s2.detach(), ref[:, 0], bound[:, 0], "SDDMM 2-D s", tally)
    w2 = w[:, 0].contiguous()
    (s2 * w2).sum().backward()
    ref, bound = loc.aggregate_columns_oracle(g, w2[:, None], g2[0], roundings=1)
    _rows(y2.grad, case, ref[:, 0], loc.cast_bound(ref, bound, dt)[:, 0], "SDDMM 2-D y.grad [num_cols, F]", tally)
    tally.assert_complete("SDDMM y.grad [num_cols, H, D]", "SDDMM 2-D y.grad [num_cols, F]")


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_column_axis_spmm_heads(cuda_device, dtype):
    _need(_axis_need(dtype))
    case, pattern = _axis("cols")
    g, used, dt = case.compact, case.used_t, DT[dtype]
    feat, v = _big(dt, 34).requires_grad_(True), _randn((case.nnz, AXIS_H), 35).requires_grad_(True)
    dc = _randn((SMALL, AXIS_H, AXIS_D), 36)
    tally = loc.Tally()
    out = SpMMHeads(pattern)(feat, v)
    _whole(out.detach(), *loc.aggregate_oracle(g, v.detach(), feat.detach()[used]), "SpMMHeads out", tally)
    (out * dc).sum().backward()
    _whole(v.grad, *loc.sddmm_oracle(g, dc, feat.detach()[used]), "SpMMHeads values.grad", tally)
    ref, bound = loc.aggregate_columns_oracle(g, v.detach(), dc, roundings=1)
    _rows(feat.grad, case, ref, loc.cast_bound(ref, bound, dt), "SpMMHeads feat.grad [num_cols, H, D]", tally)
    tally.assert_complete("SpMMHeads feat.grad [num_cols, H, D]")


def _gatv2_autograd(case, pattern, xl, xr, a, w, slope, tally, big):
    """forward, backward and every check of GATv2Score on an axis case; ``big``: which of xl / xr is the big tensor."""
    g, used = case.compact, case.used_t
    s = GATv2Score(pattern)(xl, xr, a, slope)
    xl_c, xr_c = (xl.detach()[used], xr.detach()) if big == "rows" else (xl.detach(), xr.detach()[used])
    (f_ref, f_bound), (l_ref, l_bound), term = loc.gatv2_oracle(g, xl_c, xr_c, a.detach(), slope, w)
    _whole(s.detach(), f_ref, f_bound, "GATv2Score s", tally)
    (s * w).sum().backward()
    r_ref = g.col_sum(term)
    r_bound = loc.column_bound(torch.from_numpy(g.col_deg_np).double().cuda(), g.col_sum(term.abs()))
    a64, a_abs = a.detach().double(), a.detach().double().abs()
    bounds = {"xl": (a64 * l_ref, loc.cast_bound(a64 * l_ref, a_abs * l_bound, xl.dtype)),
              "xr": (a64 * r_ref, loc.cast_bound(a64 * r_ref, a_abs * r_bound, xr.dtype))}
    for name, leaf, is_big in (("xl", xl, big == "rows"), ("xr", xr, big == "cols")):
        if is_big:
            _rows(leaf.grad, case, *bounds[name], f"GATv2Score {name}.grad [{'num_rows' if name == 'xl' else 'num_cols'}, H, D]", tally)
        else:
            _whole(leaf.grad, *bounds[name], f"GATv2Score {name}.grad", tally)
    # a.grad is a dense torch sum over the nodes; on the big axis all but the rows in use add an exact zero, so the formula of
    # tests/test_gpu_gatv2.py counts the compact graph's rows and columns (with the 4.2 M of the big axis it would bound nothing)
    a_ref = (xl_c.double() * l_ref).sum(0) + (xr_c.double() * r_ref).sum(0)
    a_bound = ((xl_c.double().abs() * l_bound).sum(0) + (xr_c.double().abs() * r_bound).sum(0)
               + g.num_rows * loc.U * (xl_c.double() * l_ref).abs().sum(0) + g.num_cols * loc.U * (xr_c.double() * r_ref).abs().sum(0))
    _whole(a.grad, a_ref, a_bound, "GATv2Score a.grad", tally)


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_column_axis_gatv2_score(cuda_device, dtype):
    _need(5 * BIG + 1)                                        # xr and its gradient, G_r, a G_r, xr G_r
    case, pattern = _axis("cols")
    dt = DT[dtype]
    xl, xr = _randn((SMALL, AXIS_H, AXIS_D), 37, dt).requires_grad_(True), _big(dt, 38).requires_grad_(True)
    a, w = _randn((AXIS_H, AXIS_D), 39).requires_grad_(True), _randn((case.nnz, AXIS_H), 40)
    tally = loc.Tally()
    _gatv2_autograd(case, pattern, xl, xr, a, w, 0.2, tally, "cols")
    tally.assert_complete("GATv2Score xr.grad [num_cols, H, D]")


def _attn_autograd(case, pattern, feat, s, dc, scale, tally, big):
    g, used = case.compact, case.used_t
    out = AttnAggregate(pattern)(feat, s, scale)
    feat_c, dc_c = (feat.detach()[used], dc) if big == "cols" else (feat.detach(), dc[used])
    ref = loc.attn_oracle(g, s.detach(), feat_c, dc_c, scale)
    if big == "rows":
        _rows(out.detach(), case, *ref["out"], "AttnAggregate out [num_rows, H, D]", tally)
    else:
        _whole(out.detach(), *ref["out"], "AttnAggregate out", tally)
    out.backward(dc)
    _whole(s.grad, *ref["d_s"], "AttnAggregate scores.grad", tally)
    col_deg = torch.from_numpy(g.col_deg_np).double().cuda()
    d_ref, d_bound = loc.d_feat_of(col_deg, {k: g.col_sum(v) for k, v in ref["cols"].items()})
    d_bound = loc.cast_bound(d_ref, d_bound, feat.dtype)
    if big == "cols":
        _rows(feat.grad, case, d_ref, d_bound, "AttnAggregate feat.grad [num_cols, H, D]", tally)
    else:
        _whole(feat.grad, d_ref, d_bound, "AttnAggregate feat.grad", tally)
    return ref


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_column_axis_attn_aggregate(cuda_device, dtype):
    _need(_axis_need(dtype))
    case, pattern = _axis("cols")
    feat = _big(DT[dtype], 41).requires_grad_(True)
    s, dc = (2.0 * _randn((case.nnz, AXIS_H), 42)).requires_grad_(True), _randn((SMALL, AXIS_H, AXIS_D), 43)
    tally = loc.Tally()
    _attn_autograd(case, pattern, feat, s, dc, AXIS_D ** -0.5, tally, "cols")
    tally.assert_complete("AttnAggregate feat.grad [num_cols, H, D]")


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_row_axis_sddmm(cuda_device, dtype):
    _need(_axis_need(dtype))
    case, pattern = _axis("rows")
    g, used, dt = case.compact, case.used_t, DT[dtype]
    x, y = _big(dt, 51).requires_grad_(True), _randn((SMALL, AXIS_H, AXIS_D), 52, dt).requires_grad_(True)
    w = _randn((case.nnz, AXIS_H), 53)
    tally = loc.Tally()
    s = SDDMM(pattern)(x, y)
    _whole(s.detach(), *loc.sddmm_oracle(g, x.detach()[used], y.detach()), "SDDMM s", tally)
    (s * w).sum().backward()
    ref, bound = loc.aggregate_oracle(g, w, y.detach(), roundings=1)
    _rows(x.grad, case, ref, loc.cast_bound(ref, bound, dt), "SDDMM x.grad [num_rows, H, D]", tally)
    ref, bound = loc.aggregate_columns_oracle(g, w, x.detach()[used], roundings=1)
    _whole(y.grad, ref, loc.cast_bound(ref, bound, dt), "SDDMM y.grad", tally)
    tally.assert_complete("SDDMM x.grad [num_rows, H, D]")


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_row_axis_spmm_heads(cuda_device, dtype):
    _need(5 * BIG + 1)                                        # the incoming gradient, autograd's copy of it, out, and temporaries
    case, pattern = _axis("rows")
    g, used, dt = case.compact, case.used_t, DT[dtype]
    feat = _randn((SMALL, AXIS_H, AXIS_D), 54, dt).requires_grad_(True)
    v, dc = _randn((case.nnz, AXIS_H), 55).requires_grad_(True), _big(torch.float32, 56)
    tally = loc.Tally()
    out = SpMMHeads(pattern)(feat, v)
    assert out.dtype == torch.float32 and out.shape == (COUNT, AXIS_H, AXIS_D)
    _rows(out.detach(), case, *loc.aggregate_oracle(g, v.detach(), feat.detach()), "SpMMHeads out [num_rows, H, D]", tally)
    out.backward(dc)                                           # the incoming gradient is the big tensor
    _whole(v.grad, *loc.sddmm_oracle(g, dc[used], feat.detach()), "SpMMHeads values.grad", tally)
    ref, bound = loc.aggregate_columns_oracle(g, v.detach(), dc[used], roundings=1)
    _whole(feat.grad, ref, loc.cast_bound(ref, bound, dt), "SpMMHeads feat.grad", tally)
    tally.assert_complete("SpMMHeads out [num_rows, H, D]")


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_row_axis_gatv2_score(cuda_device, dtype):
    _need(5 * BIG + 1)
    case, pattern = _axis("rows")
    dt = DT[dtype]
    xl, xr = _big(dt, 57).requires_grad_(True), _randn((SMALL, AXIS_H, AXIS_D), 58, dt).requires_grad_(True)
    a, w = _randn((AXIS_H, AXIS_D), 59).requires_grad_(True), _randn((case.nnz, AXIS_H), 60)
    tally = loc.Tally()
    _gatv2_autograd(case, pattern, xl, xr, a, w, 0.2, tally, "rows")
    tally.assert_complete("GATv2Score xl.grad [num_rows, H, D]")


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_row_axis_attn_aggregate(cuda_device, dtype):
    _need(5 * BIG + 1)
    case, pattern = _axis("rows")
    feat = _randn((SMALL, AXIS_H, AXIS_D), 61, DT[dtype]).requires_grad_(True)
    s, dc = (2.0 * _randn((case.nnz, AXIS_H), 62)).requires_grad_(True), _big(torch.float32, 63)
    tally = loc.Tally()
    scale = AXIS_D ** -0.5
    ref = _attn_autograd(case, pattern, feat, s, dc, scale, tally, "rows")
    tally.assert_complete("AttnAggregate out [num_rows, H, D]")
    # the row statistics of the functional form: m = -inf and l = 0 in every row without entries, as the launcher documents
    out, m, l = attn_aggregate(pattern.indptr, pattern.indices, s.detach(), feat.detach(), COUNT, scale, return_stats=True)
    empty = torch.ones(COUNT, dtype=torch.bool, device="cuda")
    empty[case.used_t] = False
    assert int(empty.sum()) == COUNT - case.used.size
    assert bool((m[empty] == float("-inf")).all()) and bool((l[empty].view(torch.int32) == 0).all())
    assert torch.equal(m[case.used_t].double(), ref["m"])
    _whole(l[case.used_t], *ref["l"], "attn_aggregate l of the rows in use", tally)
    assert int(torch.count_nonzero(out)) == int(torch.count_nonzero(out[case.used_t]))
