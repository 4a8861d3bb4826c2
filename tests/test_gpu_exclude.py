"""GPU: neighbour sampling with an exclusion list, the (row, column) -> entry lookup and the edge batches that keep their own edges out
of their blocks, bit for bit against the numpy restatement (tests/exclude_oracle.py).  One hand-built CSR of 700 rows
holds every row the kernel branches on -- d' = 0, 1, k, k + 1 and above for every fan-out, exclusions at the first and at the last
position, a row without exclusions between a row whose last and a row whose first entry is excluded, a hub row of degree 5,000 with 300
excluded entries -- and 600 shuffled seeds with duplicates put more than two workgroups on it.  The blocks and the edge batches run on a
small symmetric graph with full fan-outs, so that what must be present without the exclusion is present for certain."""
import functools

import numpy as np
import pytest
import torch

import exclude_oracle as oracle
import sample_oracle
from poisoned_alloc import poisoned

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NUM_ROWS, NUM_COLS, HUB_ROW, HUB_DEGREE, HUB_EXCLUDED, DUP_ROW = 700, 8192, 350, 5000, 300, 351
FANOUTS = (1, 3, 64, None)
SEED, OFFSET = 20261020, 2 ** 32 + 7
NUM_SEEDS, NUM_QUERIES = 600, 5000


def _specs():
    """(degree, excluded positions) of the hand-built rows."""
    rows = [(0, []), (1, []), (1, [0]), (2, [0]), (2, [1]), (5, [0, 1, 2, 3, 4]), (70, list(range(70))), (4, [0, 1, 3]),
            (5, [4]), (5, []), (5, [0]),                    # nothing excluded between "the last" and "the first": the slices' boundaries
            (5, [4]), (0, []), (5, [0]), (3, [2]), (66, []), (3, [0])]
    for k in (1, 3, 64):
        rows += [(k, []), (k + 1, []), (k + 1, [0]), (k + 1, [k]), (k + 2, [0]), (k + 2, [k + 1]), (k + 4, [1, 2, k + 3]),
                 (k + 5, [0, 1, 2, 3, 4]), (k + 5, [k, k + 1, k + 2, k + 3, k + 4]), (2 * k + 7, [0, k, 2 * k + 6]),
                 (k + 1, list(range(k))), (k + 1, list(range(1, k + 1)))]                                      # d' = 1
    return rows


class Graph:
    def __init__(self):
        rng = np.random.default_rng(20261020)
        specs = _specs()
        self.num_specs = len(specs)
        rows = list(specs)
        while len(rows) < NUM_ROWS:                          # random rows: every position excluded with probability 0.2
            d = int(rng.integers(0, 81))
            rows.append((d, np.flatnonzero(rng.random(d) < 0.2).tolist()))
        scattered = rng.choice(np.setdiff1d(np.arange(HUB_DEGREE), np.r_[0:50, 2000:2100, 4950:5000]), 100, replace=False)
        rows[HUB_ROW] = (HUB_DEGREE, np.sort(np.r_[0:50, 2000:2100, 4950:5000, scattered]).tolist())
        rows[DUP_ROW] = (6, [1])                             # its columns are set below
        degrees = np.array([d for d, _ in rows])
        self.indptr = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int64)
        self.indices = np.concatenate([np.sort(rng.choice(NUM_COLS, d, replace=False)) for d in degrees]).astype(np.int64)
        self.indices[self.indptr[DUP_ROW]:self.indptr[DUP_ROW + 1]] = [3, 9, 9, 9, 20, 20]
        self.excluded_of = [np.asarray(q, np.int64) for _, q in rows]
        self.exclude = np.concatenate([self.indptr[r] + q for r, q in enumerate(self.excluded_of)]).astype(np.int64)
        self.degrees, self.held = degrees, np.array([len(q) for q in self.excluded_of])
        assert (np.diff(self.exclude) > 0).all() and self.held[HUB_ROW] == HUB_EXCLUDED
        others = rng.choice(NUM_ROWS, NUM_SEEDS - self.num_specs - 2, replace=True)
        self.seeds = rng.permutation(np.concatenate([np.arange(self.num_specs), [HUB_ROW, DUP_ROW], others]))
        self.shuffled = np.concatenate([rng.permutation(self.indices[a:b]) for a, b in zip(self.indptr[:-1], self.indptr[1:])])
        self.d_indptr, self.d_indices, self.d_seeds = _dev(self.indptr), _dev(self.indices), _dev(self.seeds)
        self.d_exclude, self.d_shuffled = _dev(self.exclude), _dev(self.shuffled)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


@functools.lru_cache(maxsize=None)
def _graph():
    return Graph()


@functools.lru_cache(maxsize=None)
def _want(fanout, replace):
    """The oracle's arrays for one fan-out: computed once, shared, never written."""
    g = _graph()
    return oracle.sample_neighbors(g.indptr, g.indices, g.seeds, fanout, SEED, OFFSET, replace, g.exclude)


def _sample(fanout, replace, exclude="the graph's"):
    import voltrix

    g = _graph()
    return voltrix.sample_neighbors(g.d_indptr, g.d_indices, g.d_seeds, fanout, SEED, OFFSET, replace,
                                    exclude=g.d_exclude if isinstance(exclude, str) else exclude)


def _assert_same(got, want, what):
    assert len(got) == len(want) == 3
    for name, a, b in zip(("s_indptr", "s_indices", "s_entries"), got, want):
        a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
        b = b.cpu().numpy() if isinstance(b, torch.Tensor) else b
        assert a.dtype == b.dtype == np.int32 and np.array_equal(a, b), (what, name)


def test_the_graph_has_the_rows_the_kernel_branches_on():
    g = _graph()
    left = g.degrees - g.held
    on = np.zeros(NUM_ROWS, bool)
    on[g.seeds] = True
    assert g.seeds.size == NUM_SEEDS > 2 * 256 and np.unique(g.seeds).size < NUM_SEEDS and (np.diff(g.seeds) < 0).any()
    for k in (1, 3, 64):
        for dc in (k, k + 1):
            assert (on & (left == dc) & (g.held > 0)).any() and (on & (left == dc) & (g.held == 0)).any(), (k, dc)
        assert (on & (left > k + 1) & (g.held > 1)).any()
    assert (on & (g.degrees == 0)).any() and (on & (left == 0) & (g.degrees > 0)).any() and (on & (left == 0) & (g.degrees > 64)).any()
    assert (on & (left == 1) & (g.held > 0)).any() and (on & (g.degrees == 1) & (g.held == 0)).any()
    first = np.array([q.size > 0 and q[0] == 0 for q in g.excluded_of])
    last = np.array([q.size > 0 and q[-1] == d - 1 for q, d in zip(g.excluded_of, g.degrees)])
    between = last[:-2] & (g.held[1:-1] == 0) & (g.degrees[1:-1] > 0) & first[2:]
    assert between.any() and on[np.flatnonzero(between)[0] + np.arange(3)].all()
    assert on[HUB_ROW] and first[HUB_ROW] and last[HUB_ROW] and left[HUB_ROW] == HUB_DEGREE - HUB_EXCLUDED
    assert all((np.diff(g.indices[a:b]) >= 0).all() for a, b in zip(g.indptr[:-1], g.indptr[1:]))


@pytest.mark.parametrize("replace", [False, True])
@pytest.mark.parametrize("fanout", FANOUTS)
def test_sample_neighbors_with_exclude_is_exactly_the_oracle(cuda_device, fanout, replace):
    g = _graph()
    want = _want(fanout, replace)
    got = _sample(fanout, replace)
    torch.cuda.synchronize()
    _assert_same(got, want, (fanout, replace))
    entries = got[2].cpu().numpy()
    assert entries.size > 0 and not np.isin(entries, g.exclude).any()
    assert np.array_equal(got[1].cpu().numpy(), g.indices[entries])                         # ids into the original indices
    _assert_same(_sample(fanout, replace), got, "a second run")
    # rows without exclusions: the plain call's bits
    plain = [t.cpu().numpy() for t in _sample(fanout, replace, None)]
    mine = [t.cpu().numpy() for t in got]
    free = np.flatnonzero(g.held[g.seeds] == 0)
    assert free.size > 50
    for i in free:
        a, b = mine[0][i], plain[0][i]
        count = mine[0][i + 1] - a
        assert count == plain[0][i + 1] - b and np.array_equal(mine[2][a:a + count], plain[2][b:b + count]), i
    if fanout is not None and not replace:                  # a sampled row keeps CSR order
        assert all((np.diff(mine[2][a:b]) > 0).all() for a, b in zip(mine[0][:-1], mine[0][1:]))


@pytest.mark.parametrize("replace", [False, True])
def test_an_empty_exclude_is_none_and_a_strided_view_is_its_contiguous_copy(cuda_device, replace):
    g = _graph()
    empty = torch.empty(0, dtype=torch.int32, device=DEV)
    for fanout in (3, None):
        _assert_same(_sample(fanout, replace, empty), _sample(fanout, replace, None), "empty")
        _assert_same(_sample(fanout, replace, None),
                     sample_oracle.sample_neighbors(g.indptr, g.indices, g.seeds, fanout, SEED, OFFSET, replace), "plain")
        pairs = torch.stack([g.d_exclude, torch.full_like(g.d_exclude, -7)], 1)
        view = pairs[:, 0]
        assert not view.is_contiguous()
        _assert_same(_sample(fanout, replace, view), _want(fanout, replace), "strided")
        tail = torch.cat([torch.full((3,), 5, dtype=torch.int32, device=DEV), g.d_exclude])[3:]           # an offset view
        _assert_same(_sample(fanout, replace, tail), _want(fanout, replace), "offset")


@pytest.mark.parametrize("replace", [0, 1])
@pytest.mark.parametrize("fanout", [2, None])
def test_the_two_c_symbols_write_the_same_bits_without_a_list(cuda_device, fanout, replace):
    """``voltrix_launch_sample_neighbors`` and ``voltrix_launch_sample_neighbors_excluding`` with ``(NULL, 0)`` on the same seeds and
    the same ``s_indptr`` (the plain rule's), into buffers poisoned with different bytes: every element equal, and the plain oracle's.
    (An empty list takes the launch without a list; a list that holds none of a row's entries is
    test_sample_neighbors_with_exclude_is_exactly_the_oracle's ``free`` rows.)"""
    from voltrix import capi

    g = _graph()
    want = sample_oracle.sample_neighbors(g.indptr, g.indices, g.seeds, fanout, SEED, OFFSET, bool(replace))
    s_indptr, total = _dev(want[0]), int(want[0][-1])
    head = (g.d_indptr.data_ptr(), g.d_indices.data_ptr(), NUM_ROWS, g.d_seeds.data_ptr(), NUM_SEEDS, s_indptr.data_ptr(), total,
            capi.SAMPLE_ALL if fanout is None else fanout, replace, SEED, OFFSET)
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    for name, byte, middle in (("voltrix_launch_sample_neighbors", 0x00, ()), ("voltrix_launch_sample_neighbors_excluding", 0xFF, (0, 0))):
        with poisoned(byte) as state:
            out[name] = torch.empty(total, dtype=torch.int32, device=DEV), torch.empty(total, dtype=torch.int32, device=DEV)
        assert state.filled == 2 and total > NUM_SEEDS
        assert capi._call(name, *head, *middle, out[name][0].data_ptr(), out[name][1].data_ptr(), stream) == 0, name
    torch.cuda.synchronize()
    (plain_indices, plain_entries), (list_indices, list_entries) = out.values()
    assert torch.equal(plain_indices, list_indices) and torch.equal(plain_entries, list_entries)
    _assert_same((s_indptr, plain_indices, plain_entries), want, "the plain rule")


def test_an_invalid_exclude_is_a_value_error(cuda_device):
    g = _graph()
    nnz = g.indices.size
    good = g.exclude[:50]
    for bad in (good[::-1], np.r_[good[:10], good[9], good[10:]], np.r_[good, nnz], np.r_[-1, good], np.r_[good[:5], good[3], good[5:]],
                [7, 7], [nnz], [-1]):
        with pytest.raises(ValueError, match="exclude"):
            _sample(3, False, _dev(np.asarray(bad)))
    for bad in (g.d_exclude.long(), g.d_exclude.cpu(), g.d_exclude[:, None], g.exclude):
        with pytest.raises(ValueError, match="exclude"):
            _sample(3, False, bad)
    _assert_same(_sample(3, False, _dev([nnz - 1])), oracle.sample_neighbors(g.indptr, g.indices, g.seeds, 3, SEED, OFFSET, False, [nnz - 1]),
                 "the last entry alone")


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_outputs_do_not_depend_on_what_their_memory_held(cuda_device, byte):
    import voltrix

    g = _graph()
    rows, cols, want_ids = _queries()
    for fanout, replace in ((3, False), (64, True), (None, False)):
        with poisoned(byte) as state:
            got = _sample(fanout, replace)
        assert state.filled >= 2                               # s_indices, s_entries
        _assert_same(got, _want(fanout, replace), (byte, fanout))
    with poisoned(byte) as state:
        ids = voltrix.find_edges(g.d_indptr, g.d_indices, _dev(rows), _dev(cols))
    assert state.filled >= 1 and np.array_equal(ids.cpu().numpy(), want_ids)


@functools.lru_cache(maxsize=None)
def _queries():
    """5,000 (row, column) pairs and the oracle's ids: present and absent pairs, the hub row, the first and the last column of every
    row, rows of degree 0, rows -1 and num_rows, the row with duplicate columns."""
    g = _graph()
    rng = np.random.default_rng(4)
    owner = np.repeat(np.arange(NUM_ROWS), g.degrees)
    rows, cols = [], []
    some = rng.choice(g.indices.size, 1200, replace=False)                               # present
    rows += owner[some].tolist()
    cols += g.indices[some].tolist()
    rows += rng.integers(0, NUM_ROWS, 1200).tolist()                                       # mostly absent
    cols += rng.integers(0, NUM_COLS, 1200).tolist()
    hub = g.indices[g.indptr[HUB_ROW]:g.indptr[HUB_ROW + 1]]
    rows += [HUB_ROW] * 600
    cols += np.r_[hub[[0, 1, -2, -1]], rng.choice(hub, 296), rng.integers(0, NUM_COLS, 296), [-1, NUM_COLS, 2 ** 31 - 1, -2 ** 31]].tolist()
    full = np.flatnonzero(g.degrees > 0)
    rows += full.tolist() + full.tolist()                                                 # the first and the last column of every row
    cols += g.indices[g.indptr[full]].tolist() + g.indices[g.indptr[full + 1] - 1].tolist()
    for r in np.flatnonzero(g.degrees == 0).tolist() + [-1, NUM_ROWS, -2 ** 31, 2 ** 31 - 1]:
        rows += [r, r]
        cols += [0, int(rng.integers(0, NUM_COLS))]
    for c in (3, 9, 20, 2, 10, 21):
        rows.append(DUP_ROW)
        cols.append(c)
    fill = NUM_QUERIES - len(rows)
    assert fill > 0
    more = rng.choice(g.indices.size, fill)
    rows, cols = np.array(rows + owner[more].tolist()), np.array(cols + g.indices[more].tolist())
    order = rng.permutation(NUM_QUERIES)
    rows, cols = rows[order], cols[order]
    want = oracle.find_edges(g.indptr, g.indices, rows, cols)
    return rows, cols, want


def test_find_edges_is_exactly_the_oracle(cuda_device):
    import voltrix

    g = _graph()
    rows, cols, want = _queries()
    assert rows.size == NUM_QUERIES and (want >= 0).sum() > 2000 and (want < 0).sum() > 1000
    base = g.indptr[DUP_ROW]
    dup = {int(c): int(w) for r, c, w in zip(rows, cols, want) if r == DUP_ROW and c in (3, 9, 20, 2, 10, 21)}
    assert dup == {3: base, 9: base + 1, 20: base + 4, 2: -1, 10: -1, 21: -1}               # the first entry wins
    d_rows, d_cols = _dev(rows), _dev(cols)
    found = voltrix.find_edges(g.d_indptr, g.d_indices, d_rows, d_cols)
    scanned = voltrix.find_edges(g.d_indptr, g.d_indices, d_rows, d_cols, assume_sorted=False)
    torch.cuda.synchronize()
    assert found.dtype == torch.int32 and np.array_equal(found.cpu().numpy(), want)
    assert np.array_equal(scanned.cpu().numpy(), want)
    # shuffled rows: the scan still finds every pair (the id differs, the entry's column does not)
    loose = voltrix.find_edges(g.d_indptr, g.d_shuffled, d_rows, d_cols, assume_sorted=False).cpu().numpy()
    assert np.array_equal(loose, oracle.find_edges(g.indptr, g.shuffled, rows, cols)) and np.array_equal(loose >= 0, want >= 0)
    # views, and nothing to do
    both = torch.stack([d_rows, d_cols], 1)
    assert np.array_equal(voltrix.find_edges(g.d_indptr, g.d_indices, both[:, 0], both[:, 1]).cpu().numpy(), want)
    none = torch.empty(0, dtype=torch.int32, device=DEV)
    assert voltrix.find_edges(g.d_indptr, g.d_indices, none, none).shape == (0,)
    with pytest.raises(ValueError):
        voltrix.find_edges(g.d_indptr, g.d_indices, d_rows, d_cols[:-1])
    # an entry's own endpoints lead back to it wherever its row holds the column once
    entries = _dev(np.arange(0, g.indptr[HUB_ROW], 7))
    r, c = voltrix.edge_endpoints(g.d_indptr, g.d_indices, entries)
    back = voltrix.find_edges(g.d_indptr, g.d_indices, r, c)
    keep = (r != DUP_ROW)
    assert torch.equal(back[keep], entries[keep])


# ---- blocks and edge batches on a symmetric graph
SYM_NODES = 300


class Symmetric:
    def __init__(self):
        rng = np.random.default_rng(8)
        pairs = {(v, (v + s) % SYM_NODES) for v in range(SYM_NODES) for s in (1, 7, 31)}
        pairs |= {(int(a), int(b)) for a, b in rng.integers(0, SYM_NODES, (400, 2)) if a != b}
        pairs |= {(b, a) for a, b in pairs}
        ordered = np.array(sorted(pairs))
        self.rows, self.indices = ordered[:, 0], ordered[:, 1]
        self.indptr = np.concatenate([[0], np.cumsum(np.bincount(self.rows, minlength=SYM_NODES))])
        self.entries = rng.choice(self.indices.size, 40, replace=False)
        e = self.entries[0]                                  # one edge and its reverse both in the batch: the list is deduplicated
        self.entries[1] = oracle.find_edges(self.indptr, self.indices, [self.indices[e]], [self.rows[e]])[0]
        self.reverse = oracle.find_edges(self.indptr, self.indices, self.indices[self.entries], self.rows[self.entries])
        assert (self.reverse >= 0).all()
        self.d_indptr, self.d_indices, self.d_entries = _dev(self.indptr), _dev(self.indices), _dev(self.entries)


@functools.lru_cache(maxsize=None)
def _symmetric():
    return Symmetric()


@pytest.mark.parametrize("replace", [False, True])
def test_sample_blocks_passes_exclude_to_every_layer(cuda_device, replace):
    import voltrix

    s = _symmetric()
    exclude = np.unique(np.r_[s.entries, s.reverse])
    seeds = np.random.default_rng(2).choice(SYM_NODES, 50, replace=False)
    fanouts = (2, None, 3)
    blocks = voltrix.sample_blocks(s.d_indptr, s.d_indices, _dev(seeds), fanouts, SEED, OFFSET, replace, exclude=_dev(exclude))
    want = oracle.sample_blocks(s.indptr, s.indices, seeds, fanouts, SEED, OFFSET, replace, exclude)
    dst = _dev(seeds)
    for layer, (block, ref) in enumerate(zip(blocks[::-1], want[::-1])):
        s_indptr, s_indices, entries = voltrix.sample_neighbors(s.d_indptr, s.d_indices, dst, fanouts[::-1][layer], SEED, OFFSET + layer,
                                                                replace, exclude=_dev(exclude))
        src_ids, local = voltrix.compact_block(dst, s_indices, SYM_NODES)
        assert torch.equal(block.pattern.indptr, s_indptr) and torch.equal(block.pattern.indices, local)
        assert torch.equal(block.entries, entries) and torch.equal(block.src_ids, src_ids) and torch.equal(block.dst_ids, dst)
        assert np.array_equal(entries.cpu().numpy(), ref["entries"]) and np.array_equal(src_ids.cpu().numpy(), ref["src_ids"])
        assert np.array_equal(local.cpu().numpy(), ref["indices"]) and not np.isin(entries.cpu().numpy(), exclude).any()
        dst = src_ids
    plain = voltrix.sample_blocks(s.d_indptr, s.d_indices, _dev(seeds), fanouts, SEED, OFFSET, replace)
    assert any(np.isin(b.entries.cpu().numpy(), exclude).any() for b in plain)               # the exclusion had something to do


def _block_pairs(block):
    """The (destination, source) GLOBAL ids of every entry of a block."""
    indptr = block.pattern.indptr.cpu().numpy().astype(np.int64)
    rows = np.repeat(np.arange(block.num_dst), np.diff(indptr))
    return set(zip(block.dst_ids.cpu().numpy()[rows].tolist(), block.src_ids.cpu().numpy()[block.pattern.indices.cpu().numpy()].tolist()))


def test_sample_edge_batch_keeps_its_edges_and_their_reverses_out_of_its_blocks(cuda_device):
    import voltrix

    s = _symmetric()
    forward = set(zip(s.rows[s.entries].tolist(), s.indices[s.entries].tolist()))
    backward = {(v, u) for u, v in forward}
    batches = {mode: voltrix.sample_edge_batch(s.d_indptr, s.d_indices, s.d_entries, 3, (None, None), SEED, OFFSET, exclude_edges=mode)
               for mode in (None, "self", "reverse")}
    held = {mode: [_block_pairs(block) for block in batch.blocks] for mode, batch in batches.items()}
    # the full neighbourhoods of the batch's own nodes: without the exclusion every batch edge and every reverse is in the output layer
    assert forward <= held[None][-1] and backward <= held[None][-1] and any(forward & pairs for pairs in held[None])
    for block in batches["self"].blocks:
        assert not np.isin(block.entries.cpu().numpy(), s.entries).any()
    assert all(not forward & pairs for pairs in held["self"]) and (backward - forward) <= held["self"][-1]
    for pairs, block in zip(held["reverse"], batches["reverse"].blocks):
        assert not (forward | backward) & pairs
        assert not np.isin(block.entries.cpu().numpy(), np.r_[s.entries, s.reverse]).any()
    # nothing else is removed: the output layer holds every other entry of its rows
    assert held[None][-1] - forward - backward == held["reverse"][-1] and held[None][-1] - forward == held["self"][-1]
    first = batches[None]
    for mode in ("self", "reverse"):
        other = batches[mode]
        for name in ("indptr", "indices", "t_indptr", "t_indices", "t_order"):
            assert torch.equal(getattr(other.pairs, name), getattr(first.pairs, name)), (mode, name)
        assert torch.equal(other.labels, first.labels) and torch.equal(other.node_ids, first.node_ids)
        assert torch.equal(other.src_local, first.src_local) and other.num_exhausted == first.num_exhausted
        assert torch.equal(other.blocks[-1].dst_ids, first.blocks[-1].dst_ids)
    # sampled layers: the oracle's blocks for the list the batch must have built
    fanouts = (3, 2)
    batch = voltrix.sample_edge_batch(s.d_indptr, s.d_indices, s.d_entries, 3, fanouts, SEED, OFFSET, exclude_edges="reverse")
    want = oracle.sample_blocks(s.indptr, s.indices, batch.node_ids.cpu().numpy(), fanouts, SEED, OFFSET, False,
                                np.unique(np.r_[s.entries, s.reverse]))
    for block, ref in zip(batch.blocks, want):
        assert np.array_equal(block.entries.cpu().numpy(), ref["entries"]) and np.array_equal(block.src_ids.cpu().numpy(), ref["src_ids"])
        assert not (forward | backward) & _block_pairs(block)


def test_a_reverse_that_does_not_exist_is_skipped(cuda_device):
    """A directed graph: 0 -> 1 -> 2 -> 0 and 1 -> 0.  The batch is the edges 0 -> 1 (its reverse exists) and 1 -> 2 (it does not)."""
    import voltrix

    indptr, indices = _dev([0, 1, 3, 4]), _dev([1, 0, 2, 0])
    batch = voltrix.sample_edge_batch(indptr, indices, _dev([0, 2]), 1, (None,), SEED, 0, exclude_edges="reverse", exclude_self=False)
    assert _block_pairs(batch.blocks[0]) == {(2, 0)}
    batch = voltrix.sample_edge_batch(indptr, indices, _dev([0, 2]), 1, (None,), SEED, 0, exclude_edges="self", exclude_self=False)
    assert _block_pairs(batch.blocks[0]) == {(2, 0), (1, 0)}


def test_linkpred_example_trains_without_its_own_edges(cuda_device):
    """examples/linkpred_train.py's ``train_step(..., exclude_edges="reverse")`` on one edge batch of the symmetric graph, six steps:
    every loss finite, every parameter with a finite gradient."""
    import os
    import sys

    from conftest import REPO

    sys.path.insert(0, os.path.join(REPO, "examples"))
    try:
        import linkpred_train as example
    finally:
        sys.path.remove(os.path.join(REPO, "examples"))
    s = _symmetric()
    in_feats, hidden = 24, 32
    torch.manual_seed(9)
    model = example.LinkPredictor(in_feats, hidden).to(DEV)
    x = torch.randn(SYM_NODES, in_feats, device=DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = [float(example.train_step(model, opt, s.d_indptr, s.d_indices, x, s.d_entries, seed=5, step=step, fanouts=(3, 4), negatives=3,
                                       exclude_edges="reverse")) for step in range(6)]
    assert len(losses) == 6 and all(np.isfinite(losses)), losses
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in model.parameters())
