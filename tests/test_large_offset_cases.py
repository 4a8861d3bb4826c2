"""CPU: the helpers of tests/test_gpu_large_offsets.py (tests/large_offset_cases.py) with the boundary moved down -- a chunk of 8 edges
and 2^12 in the place of 2^31 -- against the whole small problem worked out directly, so that the GPU run tests the kernels and not
the test: the periodic pattern is a CSR and its transpose by periods is the stable sort of the whole pattern; the period's and the
tail's float64 references, tiled, are the references of the whole problem; the slab-wise comparison visits every element and sees a
single wrong one; the generators put entries on both sides of every boundary.  (That every launcher which takes ``nnz`` refuses 2^31 on the
host is tests/test_core_abi_host.py's.)"""
import numpy as np
import pytest
import torch

import large_offset_cases as loc

CHUNK, BOUNDARY = 8, 2 ** 12
HEADS = 4
NUM_COLS = 14                        # the period on columns 0 .. 6, the tail on 7 .. 13
CPU = torch.device("cpu")
TIGHT = dict(rtol=1e-12, atol=1e-300)


def _small(nnz=BOUNDARY // HEADS + 37, last_row_crosses=False):
    return loc.make_periodic(nnz, NUM_COLS, CPU, chunk=CHUNK, last_row_crosses=last_row_crosses)


def _whole(pc):
    """The whole pattern as one Graph, built from the device arrays the GPU test would launch with."""
    indptr, indices = pc.indptr().numpy().astype(np.int64), pc.indices().numpy().astype(np.int64)
    return loc.Graph(np.diff(indptr), indices, pc.num_cols, CPU), indptr, indices


def _randn(*shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _tiled(pc, ref_p, ref_t, per="edges"):
    n = pc.P_e if per == "edges" else pc.P
    assert ref_p.shape[0] == n
    return torch.cat([ref_p.repeat((pc.reps,) + (1,) * (ref_p.dim() - 1)), ref_t])


@pytest.mark.parametrize("nnz", [BOUNDARY // HEADS + 37, BOUNDARY // HEADS + 1, 3 * 217 + 5, BOUNDARY - 1])
def test_the_periodic_pattern_is_a_csr_and_its_transpose_is_the_stable_sort(nnz):
    pc = _small(nnz, last_row_crosses=nnz == BOUNDARY - 1)
    whole, indptr, indices = _whole(pc)
    assert indptr[0] == 0 and indptr[-1] == pc.nnz == indices.size and (np.diff(indptr) >= 0).all()
    assert indptr.size == pc.num_rows + 1 and 0 <= indices.min() and indices.max() < pc.num_cols
    lengths = np.concatenate([np.tile(pc.period.lengths, pc.reps), pc.tail.lengths])
    assert np.array_equal(np.diff(indptr), lengths)
    assert np.array_equal(indices, np.concatenate([np.tile(pc.period.cols_np, pc.reps), pc.period.cols_np[:pc.tail_e] + NUM_COLS // 2]))
    assert pc.period.cols_np.max() < NUM_COLS // 2 <= pc.tail.cols_np.min()              # the tail's columns hold the tail's entries alone
    assert np.array_equal(pc.col_deg().numpy()[NUM_COLS // 2:], pc.tail.col_deg_np[NUM_COLS // 2:].astype(np.float64))
    assert pc.nnz * HEADS > BOUNDARY or nnz < BOUNDARY // HEADS                           # edges on both sides of the boundary
    t_indptr, t_indices, t_order = (t.numpy().astype(np.int64) for t in pc.transposed())
    assert np.array_equal(t_order, whole.order_np)                                       # brute force: one stable sort of everything
    assert np.array_equal(t_indices, whole.rows_np[whole.order_np]) and np.array_equal(t_indptr, whole.t_ip)
    assert np.array_equal(pc.col_deg().numpy(), whole.col_deg_np.astype(np.float64))
    if nnz == BOUNDARY - 1:      # the last chunk is partial and the last row starts before it
        assert pc.nnz % CHUNK != 0 and pc.cut > 0 and pc.nnz - pc.cut < (pc.nnz - 1) // CHUNK * CHUNK


def test_the_real_period_has_the_rows_the_kernels_branch_on():
    lengths = loc.period_lengths()
    ip = np.concatenate([[0], np.cumsum(lengths)])
    assert ip[-1] % loc.CHUNK != 0 and ip[-1] % 2 == 1 and 40_000 < ip[-1] < 80_000
    assert (lengths == 0).any() and (lengths == 1).any() and (lengths > 2 * loc.CHUNK).any()
    assert any(ip[r] // loc.CHUNK != (ip[r + 1] - 1) // loc.CHUNK and 0 < lengths[r] <= loc.CHUNK for r in range(len(lengths)))
    # the sizes the GPU test uses: reps, tail and the offsets they reach
    for nnz, heads in ((2 ** 25 + 1234, 64), (2 ** 28 + 1234, 8), (2 ** 31 - 1, 1)):
        p_e = int(ip[-1])
        assert (nnz - 1) * heads + heads - 1 >= 2 ** 31 - 2 and nnz // p_e >= 400 and nnz % p_e > 0


def test_tiled_references_equal_the_whole_problem():
    pc = _small()
    whole, _, _ = _whole(pc)
    p, t, h, d = pc.period, pc.tail, HEADS, 4
    # operands: per edge [P_e, H], per row [P, ...], per column [num_cols, ...]
    s_p = 2.0 * _randn(pc.P_e, h, seed=1)
    s_p[5, 1] = float("-inf")
    g_p = _randn(pc.P_e, h, seed=2)
    x_p, y = _randn(pc.P, h, d, seed=3), _randn(NUM_COLS, h, d, seed=4)
    el_p, er = _randn(pc.P, h, seed=5), _randn(NUM_COLS, h, seed=6)
    a, dc_p = _randn(h, d, seed=7), _randn(pc.P, h, d, seed=8)
    s, g, x, el, dc = pc.tile_edges(s_p), pc.tile_edges(g_p), pc.tile_rows(x_p), pc.tile_rows(el_p), pc.tile_rows(dc_p)
    assert s.shape == (pc.nnz, h) and x.shape == (pc.num_rows, h, d)
    assert torch.equal(s[pc.P_e:2 * pc.P_e], s_p) and torch.equal(s[pc.reps * pc.P_e:], s_p[:pc.tail_e])
    te, tr = pc.tail_e, pc.tail_rows

    def same(got_p, got_t, want, per):
        for (gp, gt, w) in zip(got_p, got_t, want):
            torch.testing.assert_close(_tiled(pc, gp, gt, per), w, **TIGHT)

    same(loc.sddmm_oracle(p, x_p, y), loc.sddmm_oracle(t, x_p[:tr], y), loc.sddmm_oracle(whole, x, y), "edges")
    for scale in (1.0, -1.5):      # with a scale below 0 it is +inf that masks an entry
        flip = (lambda v: torch.where(torch.isinf(v), -v, v)) if scale < 0 else (lambda v: v)
        same(loc.softmax_oracle(p, flip(s_p), scale), loc.softmax_oracle(t, flip(s_p[:te]), scale),
             loc.softmax_oracle(whole, flip(s), scale), "edges")
    alpha_p = loc.softmax_oracle(p, s_p, 1.0)[0].float()
    alpha_t = loc.softmax_oracle(t, s_p[:te], 1.0)[0].float()
    alpha = torch.cat([alpha_p.repeat(pc.reps, 1), alpha_t])
    same(loc.softmax_backward_oracle(p, alpha_p, g_p, 0.5), loc.softmax_backward_oracle(t, alpha_t, g_p[:te], 0.5),
         loc.softmax_backward_oracle(whole, alpha, g, 0.5), "edges")
    same(loc.aggregate_oracle(p, g_p, y), loc.aggregate_oracle(t, g_p[:te], y), loc.aggregate_oracle(whole, g, y), "rows")
    # GAT: scores per edge, d_el per row, d_er per column
    for slope in (0.2, 0.25):
        fp, rp, gz_p = loc.gat_oracle(p, el_p, er, slope, g_p)
        ft, rt, gz_t = loc.gat_oracle(t, el_p[:tr], er, slope, g_p[:te])
        fw, rw, gz_w = loc.gat_oracle(whole, el, er, slope, g)
        same(fp, ft, fw, "edges")
        same(rp, rt, rw, "rows")
        torch.testing.assert_close(pc.col_sum(gz_p, gz_t), whole.col_sum(gz_w), **TIGHT)
        torch.testing.assert_close(pc.col_sum(gz_p.abs(), gz_t.abs()), whole.col_sum(gz_w.abs()), **TIGHT)
    # GATv2
    fp, rp, term_p = loc.gatv2_oracle(p, x_p, y, a, 0.2, g_p)
    ft, rt, term_t = loc.gatv2_oracle(t, x_p[:tr], y, a, 0.2, g_p[:te])
    fw, rw, term_w = loc.gatv2_oracle(whole, x, y, a, 0.2, g)
    same(fp, ft, fw, "edges")
    same(rp, rt, rw, "rows")
    torch.testing.assert_close(pc.col_sum(term_p, term_t), whole.col_sum(term_w), **TIGHT)
    # attn_aggregate
    op, ot, ow = (loc.attn_oracle(*args, 0.7) for args in ((p, s_p, y, dc_p), (t, s_p[:te], y, dc_p[:tr]), (whole, s, y, dc)))
    for name, per in (("out", "rows"), ("l", "rows"), ("d_s", "edges")):
        same(op[name], ot[name], ow[name], per)
    assert torch.equal(_tiled(pc, op["m"], ot["m"], "rows"), ow["m"])
    col_deg = pc.col_deg()
    sums_tiled = {k: pc.col_sum(op["cols"][k], ot["cols"][k]) for k in op["cols"]}
    sums_whole = {k: whole.col_sum(ow["cols"][k]) for k in ow["cols"]}
    for got, want in zip(loc.d_feat_of(col_deg, sums_tiled), loc.d_feat_of(col_deg, sums_whole)):
        torch.testing.assert_close(got, want, **TIGHT)
    # with a keep mask that repeats with the period (the tail takes the period's first bits)
    keep_p = torch.rand(pc.P_e, h, generator=torch.Generator().manual_seed(9)) < 0.4
    keep = pc.tile_edges(keep_p)
    mp, mt, mw = (loc.attn_oracle(*args, 0.7, k, 2.5) for args, k in (((p, s_p, y, dc_p), keep_p), ((t, s_p[:te], y, dc_p[:tr]), keep_p[:te]),
                                                                         ((whole, s, y, dc), keep)))
    for name, per in (("out", "rows"), ("l", "rows"), ("d_s", "edges")):
        same(mp[name], mt[name], mw[name], per)
    assert not torch.equal(mp["out"][0], op["out"][0])
    sums_tiled = {k: pc.col_sum(mp["cols"][k], mt["cols"][k]) for k in mp["cols"]}
    sums_whole = {k: whole.col_sum(mw["cols"][k]) for k in mw["cols"]}
    for got, want in zip(loc.d_feat_of(col_deg, sums_tiled), loc.d_feat_of(col_deg, sums_whole)):
        torch.testing.assert_close(got, want, **TIGHT)


def test_the_comparison_visits_every_element_and_sees_a_single_wrong_one():
    pc = _small()
    ref_p, ref_t = _randn(pc.P_e, HEADS, seed=11).double(), _randn(pc.tail_e, HEADS, seed=12).double()
    bound_p, bound_t = 1e-6 * ref_p.abs() + 1e-30, 1e-6 * ref_t.abs() + 1e-30
    good = torch.cat([ref_p.repeat(pc.reps, 1), ref_t])
    for slab_elems in (1, ref_p.numel() * 3 + 1, 1 << 26):
        tally = loc.Tally()
        ok, worst = loc.check_tiled(good, pc.reps, (ref_p, bound_p), (ref_t, bound_t), "good", tally, slab_elems)
        assert ok and worst == 0.0
        tally.assert_complete("good")
        assert tally.visited["good"] == good.numel()
        last_period = (pc.reps - 1) * pc.P_e
        for e, hh in ((0, 0), (pc.P_e - 1, HEADS - 1), (pc.P_e, 0), (last_period, 1), (pc.reps * pc.P_e - 1, 2), (pc.reps * pc.P_e, 0),
                      (pc.nnz - 1, HEADS - 1)):
            for wrong in (1.0 + 3e-6, float("nan")):
                bad = good.clone()
                bad[e, hh] = bad[e, hh] * wrong if wrong == wrong else wrong
                ok, _ = loc.check_tiled(bad, pc.reps, (ref_p, bound_p), (ref_t, bound_t), "bad", loc.Tally(), slab_elems)
                assert not ok, (e, hh, wrong, slab_elems)
    # equality form (the row maximum), and a result that is not periodic
    ok, _ = loc.check_tiled(good, pc.reps, (ref_p, None), (ref_t, None), "equal", loc.Tally())
    assert ok
    bad = good.clone()
    bad[pc.P_e + 3, 0] += 1e-12
    assert not loc.check_tiled(bad, pc.reps, (ref_p, None), (ref_t, None), "equal", loc.Tally())[0]
    assert loc.check_whole(ref_p, ref_p, bound_p, "whole", loc.Tally())[0]
    # a tally that misses elements, or a whole output, fails
    tally = loc.Tally()
    tally.add("part", 10, 11)
    with pytest.raises(AssertionError):
        tally.assert_complete("part")
    with pytest.raises(AssertionError):
        loc.Tally().assert_complete("never checked")


@pytest.mark.parametrize("big", ["cols", "rows"])
def test_the_axis_cases_put_entries_on_both_sides_of_both_limits(big):
    stride = 8
    count = BOUNDARY // stride + 5
    case = loc.AxisCase(count, stride, 30, big, CPU, boundary=BOUNDARY)
    ids = loc.axis_ids(count, stride, BOUNDARY)
    assert case.crosses() and set(ids) <= set(case.used) and case.used[-1] == count - 1 and case.used[0] == 0
    for limit in (BOUNDARY // 2, BOUNDARY):
        first = limit // stride
        assert {first - 1, first, first + 1} <= set(ids) and (first - 1) * stride < limit <= first * stride
    assert count * stride > BOUNDARY
    ip = case.indptr.numpy().astype(np.int64)
    assert ip[0] == 0 and ip[-1] == case.nnz and ip.size == case.num_rows + 1 and (np.diff(ip) >= 0).all()
    # the compact reference, scattered to the used ids, is the reference of the pattern with the real ids
    real = loc.Graph(np.diff(ip), case.indices.numpy(), case.num_cols, CPU)
    h, d = 2, 4
    x, y = _randn(case.num_rows, h, d, seed=1), _randn(case.num_cols, h, d, seed=2)
    v = _randn(case.nnz, h, seed=3)
    used = case.used_t
    xc, yc = (x[used], y) if big == "rows" else (x, y[used])
    torch.testing.assert_close(loc.sddmm_oracle(case.compact, xc, yc)[0], loc.sddmm_oracle(real, x, y)[0], **TIGHT)
    for got, want in zip(loc.aggregate_columns_oracle(case.compact, v, xc), loc.aggregate_columns_oracle(real, v, x)):
        torch.testing.assert_close(got, want[used] if big == "cols" else want, **TIGHT)
    want, want_bound = loc.aggregate_oracle(real, v, y)
    got, got_bound = loc.aggregate_oracle(case.compact, v, yc)
    if big == "rows":
        full = torch.zeros_like(want)
        full[used] = got
        torch.testing.assert_close(full, want, **TIGHT)
        tally = loc.Tally()
        assert loc.check_rows(want, used, got, got_bound + 1e-300, "rows", tally)[0]
        tally.assert_complete("rows")
        bad = want.clone()
        bad[int(used[3]) + 1 if int(used[3]) + 1 not in set(case.used.tolist()) else 7, 0, 0] = 1e-30      # an unused row that is not zero
        assert not loc.check_rows(bad, used, got, got_bound + 1e-300, "rows", loc.Tally())[0]
    else:
        torch.testing.assert_close(got, want, **TIGHT)
    assert np.array_equal(np.unique(case.rows_np if big == "rows" else case.cols_np), case.used)


def test_cast_bound_and_unpack_keep():
    ref, bound = torch.tensor([1.0, -3.0], dtype=torch.float64), torch.tensor([1e-6, 1e-6], dtype=torch.float64)
    assert loc.cast_bound(ref, bound, torch.float32) is bound
    wide = loc.cast_bound(ref, bound, torch.float16)
    assert bool((wide > bound + 2.0 ** -11 * ref.abs()).all()) and bool((wide < bound + 2.0 ** -10 * ref.abs()).all())
    mask = torch.tensor([[5, 1], [-1, 0]], dtype=torch.int32)
    keep = loc.unpack_keep(mask, 33)
    assert keep.shape == (2, 33) and keep[0, :4].tolist() == [True, False, True, False] and bool(keep[0, 32])
    assert bool(keep[1, :32].all()) and not bool(keep[1, 32])
    from voltrix.dropout import unpack_mask
    assert torch.equal(keep, unpack_mask(mask, 33))
    words = torch.tensor([0, 1, -1, 5, -2 ** 31, 0x5A5A5A5A], dtype=torch.int32)
    assert loc.popcount32(words).tolist() == [0, 1, 32, 2, 1, 16]
