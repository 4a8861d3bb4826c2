"""GPU: voltrix.subgraph_csr / induced_subgraph / random_walk / sample_subgraph_rw against the numpy restatement of their contracts
(tests/subgraph_oracle.py) -- exactly, element by element -- and the induced pattern through SpMMReduce, SpMMHeads and AttnAggregate.

One hand-built rectangular CSR, 600 rows x 4,096 columns: the degrees cycle through 0, 1 and g - 1, g, g + 1, 2 g + 1 for every
lane-group width g in {4, 8, 16, 32, 64}; one row has 5,000 entries; rows of length >= 4 hold a duplicate column; one row in three is
unsorted; the last entry of every row has a column of its own at or above 3,496 (so one column set selects only the last entry of every
row: the last lane of the last round).  These are the smallest shapes at which the group tail, the ballot slice, the running offset
and the workgroup tail (R = 257, 600) can go wrong.  The square variant folds the columns into [0, 600); it keeps the rows of degree 0,
so walks on it meet dead ends."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

import subgraph_oracle as oracle
from poisoned_alloc import poisoned

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NUM_ROWS, NUM_COLS, HUB_ROW, HUB_DEGREE, LAST_BASE = 600, 4096, 77, 5000, 3496
GROUPS = (4, 8, 16, 32, 64)
DEGREES = sorted({0, 1} | {d for g in GROUPS for d in (g - 1, g, g + 1, 2 * g + 1)})
ROW_COUNTS = (0, 1, 63, 64, 65, 257, 600)
SEED, OFFSET = 20261019, 2 ** 32 + 7
WALKERS = (0, 1, 63, 64, 65, 257, 600, 1000)
LENGTHS = (0, 1, 3, 4, 5, 8, 33)


class Graph:
    def __init__(self):
        rng = np.random.default_rng(1)
        degrees = np.array([DEGREES[r % len(DEGREES)] for r in range(NUM_ROWS)])
        degrees[HUB_ROW] = HUB_DEGREE
        self.indptr = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int32)
        rows = []
        for r, d in enumerate(degrees):
            cols = rng.integers(0, LAST_BASE, d)
            if d >= 4:
                cols[d // 2] = cols[0]                       # a duplicate column in every row of some length
            if r % 3:
                cols = np.sort(cols)                         # one row in three is unsorted
            if d:
                cols[-1] = LAST_BASE + r                     # the last entry's own column: above every other, a sorted row stays sorted
            rows.append(cols)
        self.indices = np.concatenate(rows).astype(np.int32)
        self.degrees = degrees
        self.square_indices = (self.indices % NUM_ROWS).astype(np.int32)
        self.shuffled = rng.permutation(NUM_ROWS).astype(np.int32)
        self.d_indptr, self.d_indices = torch.from_numpy(self.indptr).to(DEV), torch.from_numpy(self.indices).to(DEV)
        self.d_square = torch.from_numpy(self.square_indices).to(DEV)
        every = np.arange(NUM_COLS)
        self.column_sets = {"none": every[:0], "all": every, "shuffled": rng.permutation(NUM_COLS), "every_other": every[::2],
                            "tenth": np.sort(rng.choice(NUM_COLS, NUM_COLS // 10, replace=False)), "single": self.indices[:1].copy(),
                            "last_entries": LAST_BASE + np.arange(NUM_ROWS)}

    def rows(self, count):
        """``count`` distinct rows in a shuffled order; the hub row is among them from 63 on."""
        s = self.shuffled[:count].copy()
        if count >= 63 and HUB_ROW not in s:
            s[5] = HUB_ROW
        return s

    def row_sets(self):
        sets = {f"R{count}": self.rows(count) for count in ROW_COUNTS}
        sets["duplicates"] = np.concatenate([self.rows(65), self.rows(65)[::-3], [HUB_ROW]]).astype(np.int32)
        return sets


@functools.lru_cache(maxsize=None)
def _graph():
    return Graph()


@functools.lru_cache(maxsize=None)
def _want(row_set, column_set):
    """The oracle's three arrays for one (rows, cols) of the rectangular graph: computed once, shared, never written."""
    g = _graph()
    return oracle.subgraph_csr(g.indptr, g.indices, g.row_sets()[row_set], g.column_sets[column_set], NUM_COLS)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _assert_equals_oracle(got, want, what, names=("s_indptr", "s_local", "s_entries")):
    assert len(got) == len(want) == len(names)
    for name, g, w in zip(names, got, want):
        assert g.dtype == torch.int32 and g.is_cuda and g.is_contiguous(), (what, name)
        assert g.shape == w.shape and np.array_equal(g.cpu().numpy(), w), (what, name)


def test_the_graph_has_the_rows_the_kernels_branch_on():
    g = _graph()
    assert g.indptr[-1] == g.indices.size and set(DEGREES) <= set(g.degrees.tolist()) and g.degrees[HUB_ROW] == HUB_DEGREE
    assert {g - 1 for g in GROUPS} | set(GROUPS) | {g + 1 for g in GROUPS} | {2 * g + 1 for g in GROUPS} <= set(DEGREES)
    unsorted = [r for r in range(NUM_ROWS) if (np.diff(g.indices[g.indptr[r]:g.indptr[r + 1]]) < 0).any()]
    dup = [r for r in range(NUM_ROWS) if np.unique(g.indices[g.indptr[r]:g.indptr[r + 1]]).size < g.degrees[r]]
    assert len(unsorted) > 50 and len(dup) > 100 and g.indices.max() >= NUM_ROWS
    assert all(np.unique(v).size == v.size for v in g.column_sets.values())
    last = _want("R600", "last_entries")                      # one entry of every row that has one, and it is the row's last
    rows = g.rows(600)
    assert np.array_equal(np.diff(last[0]), (g.degrees[rows] > 0).astype(np.int32))
    assert np.array_equal(last[2], (g.indptr[rows + 1] - 1)[g.degrees[rows] > 0])
    assert HUB_ROW in g.rows(63) and np.unique(g.row_sets()["duplicates"]).size < g.row_sets()["duplicates"].size
    assert (g.degrees == 0).sum() > 20 and (np.bincount(g.square_indices, minlength=NUM_ROWS)[g.degrees == 0] > 0).any()


@pytest.mark.parametrize("group", GROUPS)
def test_subgraph_csr_is_exactly_the_oracle(cuda_device, group):
    import voltrix

    g = _graph()
    for row_set, rows in g.row_sets().items():
        d_rows = _dev(rows)
        for column_set, cols in g.column_sets.items():
            got = voltrix.subgraph_csr(g.d_indptr, g.d_indices, d_rows, _dev(cols), NUM_COLS, group=group)
            _assert_equals_oracle(got, _want(row_set, column_set), (group, row_set, column_set))
    full = voltrix.subgraph_csr(g.d_indptr, g.d_indices, _dev(np.arange(NUM_ROWS)), _dev(np.arange(NUM_COLS)), NUM_COLS, group=group)
    _assert_equals_oracle(full, (g.indptr, g.indices, np.arange(g.indices.size, dtype=np.int32)), (group, "identity"))


def test_every_group_width_and_the_default_give_the_same_bits(cuda_device):
    import voltrix
    from voltrix import capi

    g = _graph()
    rows, cols = _dev(g.row_sets()["duplicates"]), _dev(g.column_sets["tenth"])
    results = [voltrix.subgraph_csr(g.d_indptr, g.d_indices, rows, cols, NUM_COLS, group=group) for group in GROUPS + (None,)]
    for other in results[1:]:
        assert all(torch.equal(a, b) for a, b in zip(results[0], other))
    assert results[0][1].numel() > 0
    # the entry points with an explicit width: what subgraph_csr launches, on the same table
    stream = torch.cuda.current_stream().cuda_stream
    table = torch.zeros(NUM_COLS, dtype=torch.int32, device=DEV)
    capi.launch_block_mark_seeds(cols, NUM_COLS, table, stream)
    for group in GROUPS:
        counts = torch.full((rows.numel(),), -7, dtype=torch.int32, device=DEV)
        capi.launch_subgraph_count(g.d_indptr, g.d_indices, NUM_ROWS, rows, table, group, counts, stream)
        assert torch.equal(counts, results[0][0][1:] - results[0][0][:-1])
        s_local, s_entries = torch.full_like(results[0][1], -7), torch.full_like(results[0][2], -7)
        capi.launch_subgraph_fill(g.d_indptr, g.d_indices, NUM_ROWS, rows, table, group, results[0][0], s_local, s_entries, stream)
        assert torch.equal(s_local, results[0][1]) and torch.equal(s_entries, results[0][2])
    with pytest.raises(ValueError):
        voltrix.subgraph_csr(g.d_indptr, g.d_indices, rows, cols, NUM_COLS, group=12)


def test_induced_subgraph(cuda_device):
    import voltrix

    g = _graph()
    for nodes in (g.rows(257), g.rows(65), np.arange(NUM_ROWS, dtype=np.int32)):
        sub = voltrix.induced_subgraph(g.d_indptr, g.d_square, _dev(nodes), validate=True)
        want = oracle.induced_subgraph(g.indptr, g.square_indices, nodes)
        p = sub.pattern
        assert sub.num_nodes == nodes.size == p.num_rows == p.num_cols and p.num_edges == want["indices"].size
        _assert_equals_oracle((p.indptr, p.indices, sub.entries, sub.node_ids),
                              (want["indptr"], want["indices"], want["entries"], want["node_ids"]), nodes.size,
                              ("indptr", "indices", "entries", "node_ids"))
        local, entries = p.indices.cpu().numpy(), sub.entries.cpu().numpy()
        assert np.array_equal(nodes[local], g.square_indices[entries])                     # entries point at the CSR's own entries
        # the transpose the pattern operators use: entry e of it is entry t_order[e] of the pattern, its row the column of that entry
        order = p.t_order.cpu().numpy()
        row_of = np.repeat(np.arange(p.num_rows), np.diff(want["indptr"]))
        assert np.array_equal(np.sort(order), np.arange(p.num_edges)) and p.t_indptr.numel() == p.num_cols + 1
        assert np.array_equal(p.t_indices.cpu().numpy(), row_of[order])
        assert np.array_equal(np.repeat(np.arange(p.num_cols), np.diff(p.t_indptr.cpu().numpy())), local[order])
        assert np.array_equal(g.square_indices[entries[order]], nodes[local[order]])
    # the identity: every node in order gives the graph itself
    assert np.array_equal(p.indptr.cpu().numpy(), g.indptr) and np.array_equal(p.indices.cpu().numpy(), g.square_indices)
    assert np.array_equal(entries, np.arange(g.indices.size))


def _starts(count):
    g = _graph()
    if count == 1000:                                          # duplicate starts: different walks
        return np.concatenate([g.shuffled, g.shuffled[:400]]).astype(np.int32)
    return g.shuffled[:count].copy()


@pytest.mark.parametrize("length", LENGTHS)
def test_random_walk_is_exactly_the_oracle(cuda_device, length):
    import voltrix

    g = _graph()
    for count in WALKERS:
        starts = _starts(count)
        want = oracle.random_walk(g.indptr, g.square_indices, starts, length, SEED, OFFSET)
        if count == 600 and length >= 3:                       # dead ends occur, and not every walk meets one
            ended = (want[0] == -1).any(1)
            assert ended.any() and not ended.all() and (want[1] == -1).any()
        got = voltrix.random_walk(g.d_indptr, g.d_square, _dev(starts), length, SEED, OFFSET)
        assert got[0].shape == (count, length + 1) and got[1].shape == (count, length)
        _assert_equals_oracle(got, want, (count, length), ("nodes", "entries"))
    if length == 5:
        starts = _starts(1000)
        for seed, offset in ((2 ** 40 + 9, 0), (2 ** 64 - 1, 2 ** 64 - 1)):
            got = voltrix.random_walk(g.d_indptr, g.d_square, _dev(starts), length, seed, offset)
            want = oracle.random_walk(g.indptr, g.square_indices, starts, length, seed, offset)
            _assert_equals_oracle(got, want, seed, ("nodes", "entries"))
        first = oracle.random_walk(g.indptr, g.square_indices, starts, length, SEED, OFFSET)[0]
        assert not np.array_equal(first[:400], first[600:])                                # the same starts, other walkers: other walks
        # the rectangular graph: a column at or above 600 is recorded and ends the walk
        got = voltrix.random_walk(g.d_indptr, g.d_indices, _dev(starts), length, SEED, OFFSET)
        want = oracle.random_walk(g.indptr, g.indices, starts, length, SEED, OFFSET)
        assert (want[0] >= NUM_ROWS).any()
        _assert_equals_oracle(got, want, "rectangular", ("nodes", "entries"))


def test_step_major_stores_are_the_transposed_walk(cuda_device):
    from voltrix import capi

    g = _graph()
    starts, length = _dev(_starts(257)), 9
    want = oracle.random_walk(g.indptr, g.square_indices, _starts(257), length, SEED, OFFSET)
    nodes = torch.full((length + 1, 257), -7, dtype=torch.int32, device=DEV)
    entries = torch.full((length, 257), -7, dtype=torch.int32, device=DEV)
    capi.launch_random_walk(g.d_indptr, g.d_square, NUM_ROWS, starts, length, SEED, OFFSET, nodes, entries,
                            torch.cuda.current_stream().cuda_stream, step_major=True)
    assert np.array_equal(nodes.cpu().numpy().T, want[0]) and np.array_equal(entries.cpu().numpy().T, want[1])


def _assert_subgraph(sub, want, what):
    p = sub.pattern
    assert sub.num_nodes == want["num_nodes"] == p.num_rows == p.num_cols
    _assert_equals_oracle((p.indptr, p.indices, sub.entries, sub.node_ids),
                          (want["indptr"], want["indices"], want["entries"], want["node_ids"]), what,
                          ("indptr", "indices", "entries", "node_ids"))


@pytest.mark.parametrize("count,length", [(3, 4), (65, 3), (600, 8)])
def test_sample_subgraph_rw(cuda_device, count, length):
    import voltrix

    g = _graph()
    roots = _starts(count)
    sub = voltrix.sample_subgraph_rw(g.d_indptr, g.d_square, _dev(roots), length, SEED, OFFSET)
    want = oracle.sample_subgraph_rw(g.indptr, g.square_indices, roots, length, SEED, OFFSET)
    _assert_subgraph(sub, want, (count, length))
    ids = sub.node_ids.cpu().numpy()
    assert (np.diff(ids) > 0).all() and set(roots.tolist()) <= set(ids.tolist())
    walked = oracle.random_walk(g.indptr, g.square_indices, roots, length, SEED, OFFSET)[0]
    assert set(ids.tolist()) == set(walked[walked >= 0].tolist())


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_outputs_do_not_depend_on_what_their_memory_held(cuda_device, byte):
    import voltrix

    g = _graph()
    rows, cols, starts = _dev(g.row_sets()["duplicates"]), _dev(g.column_sets["tenth"]), _dev(_starts(257))
    want = voltrix.subgraph_csr(g.d_indptr, g.d_indices, rows, cols, NUM_COLS)
    want_walk = voltrix.random_walk(g.d_indptr, g.d_square, starts, 5, SEED, OFFSET)
    want_sub = voltrix.sample_subgraph_rw(g.d_indptr, g.d_square, starts, 5, SEED, OFFSET)
    with poisoned(byte) as state:
        got = voltrix.subgraph_csr(g.d_indptr, g.d_indices, rows, cols, NUM_COLS)
        after_subgraph = state.filled
        got_walk = voltrix.random_walk(g.d_indptr, g.d_square, starts, 5, SEED, OFFSET)
        after_walk = state.filled
        got_sub = voltrix.sample_subgraph_rw(g.d_indptr, g.d_square, starts, 5, SEED, OFFSET)
    assert after_subgraph >= 3                               # counts, s_local, s_entries
    assert after_walk >= after_subgraph + 2                  # nodes, entries
    assert state.filled >= after_walk + 2 + 2 + 3            # the walk, compact_block's two, subgraph_csr's three
    for a, b in zip(got + got_walk, want + want_walk):
        assert torch.equal(a, b)
    for name in ("indptr", "indices", "t_indptr", "t_indices", "t_order"):
        assert torch.equal(getattr(got_sub.pattern, name), getattr(want_sub.pattern, name)), name
    assert torch.equal(got_sub.node_ids, want_sub.node_ids) and torch.equal(got_sub.entries, want_sub.entries)
    _assert_equals_oracle(got, _want("duplicates", "tenth"), "poisoned")


def test_views_give_the_bits_of_the_contiguous_call(cuda_device):
    import voltrix

    g = _graph()
    rows, cols, starts = g.rows(257), g.column_sets["tenth"], _starts(257)
    want = voltrix.subgraph_csr(g.d_indptr, g.d_indices, _dev(rows), _dev(cols), NUM_COLS)
    want_walk = voltrix.random_walk(g.d_indptr, g.d_square, _dev(starts), 5, SEED, OFFSET)

    def strided(a):
        wide = torch.full((2 * a.size,), -7, dtype=torch.int32, device=DEV)
        wide[::2] = _dev(a)
        return wide[::2]

    def shifted(t, by=3):
        pad = torch.full((by,), -7, dtype=torch.int32, device=DEV)
        return torch.cat([pad, t, pad])[by:-by]

    ip, ix, sq = shifted(g.d_indptr, 1), shifted(g.d_indices), shifted(g.d_square)
    assert not strided(rows).is_contiguous() and ip.storage_offset() == 1 and ix.storage_offset() == 3 and ip.data_ptr() % 16 == 4
    for view_ip, view_ix, view_rows, view_cols in ((g.d_indptr, g.d_indices, strided(rows), strided(cols)),
                                                   (ip, ix, shifted(_dev(rows)), _dev(cols)), (ip, ix, strided(rows), shifted(_dev(cols)))):
        got = voltrix.subgraph_csr(view_ip, view_ix, view_rows, view_cols, NUM_COLS)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    for view_ip, view_ix, view_starts in ((g.d_indptr, g.d_square, strided(starts)), (ip, sq, shifted(_dev(starts))),
                                          (ip, sq, strided(starts))):
        got = voltrix.random_walk(view_ip, view_ix, view_starts, 5, SEED, OFFSET)
        assert all(torch.equal(a, b) for a, b in zip(got, want_walk))
    sub, sub_view = (voltrix.induced_subgraph(a, b, c) for a, b, c in ((g.d_indptr, g.d_square, _dev(rows)), (ip, sq, strided(rows))))
    assert torch.equal(sub.pattern.indices, sub_view.pattern.indices) and torch.equal(sub.entries, sub_view.entries)


@pytest.mark.parametrize("bad", [-1, NUM_ROWS, 2 ** 31 - 1, -2 ** 31])
def test_ids_out_of_range_are_a_value_error(cuda_device, bad):
    import voltrix

    g = _graph()
    rows, cols = g.rows(65), g.column_sets["tenth"]
    bad_rows, bad_cols = rows.copy(), cols.copy()
    bad_rows[40] = bad
    bad_cols[40] = bad if bad != NUM_ROWS else NUM_COLS
    with pytest.raises(ValueError, match="row"):
        voltrix.subgraph_csr(g.d_indptr, g.d_indices, _dev(bad_rows), _dev(cols), NUM_COLS)
    with pytest.raises(ValueError, match="column"):
        voltrix.subgraph_csr(g.d_indptr, g.d_indices, _dev(rows), _dev(bad_cols), NUM_COLS)
    with pytest.raises(ValueError):
        voltrix.induced_subgraph(g.d_indptr, g.d_square, _dev(bad_rows))
    with pytest.raises(ValueError, match="start"):
        voltrix.random_walk(g.d_indptr, g.d_square, _dev(bad_rows), 5, SEED, OFFSET)
    with pytest.raises(ValueError):
        voltrix.sample_subgraph_rw(g.d_indptr, g.d_square, _dev(bad_rows), 5, SEED, OFFSET)
    torch.cuda.synchronize()                                              # and no fault: the device still answers
    good = voltrix.subgraph_csr(g.d_indptr, g.d_indices, _dev(rows), _dev(cols), NUM_COLS)
    _assert_equals_oracle(good, _want("R65", "tenth"), "after the refusals")
    walk = voltrix.random_walk(g.d_indptr, g.d_square, _dev(rows), 5, SEED, OFFSET)
    want = oracle.random_walk(g.indptr, g.square_indices, rows, 5, SEED, OFFSET)
    _assert_equals_oracle(walk, want, "after the refusals", ("nodes", "entries"))


def test_a_duplicate_column_id_is_a_value_error_on_request(cuda_device):
    import voltrix

    g = _graph()
    rows, cols = g.rows(65), g.column_sets["tenth"]
    twice = np.concatenate([cols, cols[7:8]])
    with pytest.raises(ValueError, match="distinct"):
        voltrix.subgraph_csr(g.d_indptr, g.d_indices, _dev(rows), _dev(twice), NUM_COLS, validate=True)
    with pytest.raises(ValueError, match="distinct"):
        voltrix.induced_subgraph(g.d_indptr, g.d_square, _dev(np.concatenate([rows, rows[:1]])), validate=True)
    good = voltrix.subgraph_csr(g.d_indptr, g.d_indices, _dev(rows), _dev(cols), NUM_COLS, validate=True)
    _assert_equals_oracle(good, _want("R65", "tenth"), "after the refusals")


def test_the_pattern_operators_take_the_induced_pattern_as_it_is(cuda_device):
    """Against a dense float64 model of A[nodes][:, nodes] (A counts a repeated entry as often as it appears).  max: every column of
    the features is a permutation of small integers, so a row's maximum has one winner node and both the output and its gradient are
    exact; sum (SpMMHeads with unit values): sums of small integers are exact in fp32, forward and backward.  AttnAggregate: the
    float64 model and the bounds of tests/test_gpu_attn_aggregate.py, on the oracle's arrays of the induced pattern."""
    import voltrix
    from test_gpu_attn_aggregate import _Graph, _oracle, _within
    from voltrix.autograd import AttnAggregate, SpMMHeads, SpMMReduce

    g = _graph()
    nodes = g.rows(257)
    sub = voltrix.induced_subgraph(g.d_indptr, g.d_square, _dev(nodes))
    want = oracle.induced_subgraph(g.indptr, g.square_indices, nodes)
    count, pattern = nodes.size, sub.pattern
    dense = np.zeros((NUM_ROWS, NUM_ROWS))
    np.add.at(dense, (np.repeat(np.arange(NUM_ROWS), g.degrees), g.square_indices), 1.0)
    a = dense[nodes][:, nodes]
    assert a.sum() == pattern.num_edges > count and (a.sum(1) == 0).any() and (a > 1).any()
    gen = torch.Generator().manual_seed(3)
    dim, heads = 12, 2
    # max
    feat = torch.stack([torch.randperm(count, generator=gen) for _ in range(dim)], 1).float() - count // 2
    grad = torch.randint(-4, 5, (count, dim), generator=gen).float()
    f64, g64 = feat.double().numpy(), grad.double().numpy()
    masked = np.where(a[:, :, None] > 0, f64[None, :, :], -np.inf)                          # [row, column, dim]
    ref_max = np.where(a.sum(1)[:, None] > 0, masked.max(1), 0.0)
    ref_grad = np.zeros((count, dim))
    has = a.sum(1) > 0
    np.add.at(ref_grad, (masked.argmax(1)[has], np.broadcast_to(np.arange(dim), (int(has.sum()), dim))), g64[has])
    leaf = feat.to(DEV).requires_grad_(True)
    out = SpMMReduce(pattern, reduce="max")(leaf)
    out.backward(grad.to(DEV))
    assert np.array_equal(out.detach().cpu().double().numpy(), ref_max) and np.array_equal(leaf.grad.cpu().double().numpy(), ref_grad)
    # sum
    feat = torch.randint(-4, 5, (count, heads, dim), generator=gen).float()
    grad = torch.randint(-4, 5, (count, heads, dim), generator=gen).float()
    leaf = feat.to(DEV).requires_grad_(True)
    out = SpMMHeads(pattern)(leaf, torch.ones(pattern.num_edges, heads, device=DEV))
    out.backward(grad.to(DEV))
    assert np.array_equal(out.detach().cpu().double().numpy(), np.einsum("rc,chd->rhd", a, feat.double().numpy()))
    assert np.array_equal(leaf.grad.cpu().double().numpy(), np.einsum("rc,rhd->chd", a, grad.double().numpy()))
    # attention
    model = _Graph(np.diff(want["indptr"]), want["indices"], count)
    dev_gen = torch.Generator(device="cuda").manual_seed(5)
    scores = 2.0 * torch.randn((pattern.num_edges, heads), device="cuda", generator=dev_gen)
    feat = torch.randn((count, heads, dim), device="cuda", generator=dev_gen)
    grad = torch.randn((count, heads, dim), device="cuda", generator=dev_gen)
    ref = _oracle(model, scores, feat, grad, 0.5)
    feat_leaf, score_leaf = feat.clone().requires_grad_(True), scores.clone().requires_grad_(True)
    out = AttnAggregate(pattern)(feat_leaf, score_leaf, 0.5)
    out.backward(grad)
    _within(out.detach(), *ref["out"], "out on the induced pattern")
    _within(score_leaf.grad, *ref["d_s"], "d_s on the induced pattern")
    _within(feat_leaf.grad, *ref["d_feat"], "d_feat on the induced pattern")


@pytest.mark.parametrize("mode", ["cluster", "rw"])
def test_subgraph_example_trains(cuda_device, mode):
    """examples/subgraph_train.py's model on one subgraph batch of the folded test graph -- a chunk of nodes, or the nodes that walks
    visit: six steps with a finite, decreasing loss, every parameter with a finite gradient."""
    import voltrix

    sys.path.insert(0, os.path.join(REPO, "examples"))
    try:
        import subgraph_train as example
    finally:
        sys.path.remove(os.path.join(REPO, "examples"))
    g = _graph()
    in_feats, hidden, classes = 24, 32, 7
    torch.manual_seed(9)
    model = example.SubgraphSAGE(in_feats, hidden, classes).to(DEV)
    x = torch.randn(NUM_ROWS, in_feats, device=DEV)
    y = torch.randint(0, classes, (NUM_ROWS,), device=DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    if mode == "cluster":
        sub = voltrix.induced_subgraph(g.d_indptr, g.d_square, _dev(g.rows(257)))
    else:
        sub = voltrix.sample_subgraph_rw(g.d_indptr, g.d_square, _dev(_starts(65)), example.WALK_LENGTH, seed=5)
    assert sub.num_nodes >= 65 and sub.pattern.num_edges > sub.num_nodes
    losses = [float(example.train_step(model, opt, sub, x, y)) for _ in range(6)]
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in model.parameters())
    assert all(np.isfinite(losses)) and all(b < a for a, b in zip(losses, losses[1:])), losses
