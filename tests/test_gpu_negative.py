"""GPU: voltrix.negative_sample / edge_endpoints / sample_edge_batch against the numpy restatement of their contracts
(tests/negative_oracle.py) -- exactly, element by element -- and a batch's pair pattern through autograd.SDDMM.

One hand-built rectangular CSR, 300 rows x 257 columns, every row ascending: runs of empty rows in front, inside and at the end; rows of
degree 1; a full row (every slot is -1); a row that misses exactly one column; a row that holds column 0 and column 256, the two ends of
the search; rows with a duplicate column; a row with a column id of 300, outside the columns.  Every other row has a degree of at most
64: a density of at most 0.25, so with 16 tries a slot is exhausted with a probability below 0.25^16 -- the oracle is asserted to
yield no -1 there, and equality on -1 is never the only thing that was compared.  The square variant keeps the first 257 rows."""
import functools

import numpy as np
import pytest
import torch

import negative_oracle as oracle
import sample_oracle
from poisoned_alloc import poisoned

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NUM_ROWS, NUM_COLS = 300, 257
FULL, MISSING_ONE, ENDS, OUTSIDE, THE_MISSING = 5, 6, 7, 8, 100
EMPTY_RUNS = ((0, 2), (150, 154), (297, 300))
SEED, OFFSET = 20261019, 2 ** 32 + 7
#        S k in {1, 255, 256, 257, 1000}, k in {1, 3, 5, 64}
SIZES = [(1, 1), (85, 3), (51, 5), (256, 1), (4, 64), (257, 1), (200, 5), (1000, 1)]
TRIES = (1, 3, 16, 17)


class Graph:
    def __init__(self):
        rng = np.random.default_rng(1)
        rows = []
        for r in range(NUM_ROWS):
            if any(a <= r < b for a, b in EMPTY_RUNS) or r % 10 == 0:
                cols = np.zeros(0, np.int64)
            elif r == FULL:
                cols = np.arange(NUM_COLS)
            elif r == MISSING_ONE:
                cols = np.delete(np.arange(NUM_COLS), THE_MISSING)
            elif r == ENDS:
                cols = np.array([0, NUM_COLS - 1])
            elif r == OUTSIDE:
                cols = np.concatenate([np.sort(rng.choice(NUM_COLS, 9, replace=False)), [300]])
            elif r % 10 == 1:
                cols = rng.integers(0, NUM_COLS, 1)
            else:
                cols = np.sort(rng.choice(NUM_COLS, rng.integers(2, 64), replace=False))
                if r % 10 == 2:
                    cols = np.sort(np.concatenate([cols, cols[:1]]))            # a duplicate column
            rows.append(cols)
        self.degrees = np.array([len(c) for c in rows])
        self.indptr = np.concatenate([[0], np.cumsum(self.degrees)]).astype(np.int32)
        self.indices = np.concatenate(rows).astype(np.int32)
        self.shuffled = np.concatenate([rng.permutation(c) for c in rows]).astype(np.int32)
        self.ordinary = np.array([r for r in range(NUM_ROWS) if r not in (FULL, MISSING_ONE)])
        self.order = rng.permutation(NUM_ROWS)
        # the square variant: the first 257 rows (the column 300 of row 8 stays outside)
        self.sq_indptr = self.indptr[:NUM_COLS + 1].copy()
        self.sq_indices = self.indices[:self.sq_indptr[-1]].copy()
        self.d_indptr, self.d_indices, self.d_shuffled = _dev(self.indptr), _dev(self.indices), _dev(self.shuffled)
        self.d_sq_indptr, self.d_sq_indices = _dev(self.sq_indptr), _dev(self.sq_indices)

    def sources(self, count, ordinary=False):
        """``count`` row ids in a shuffled order, the special rows among the first eight unless ``ordinary``."""
        pool = self.order[np.isin(self.order, self.ordinary)] if ordinary else self.order
        s = np.resize(pool, count).copy()
        if not ordinary and count >= 8:
            s[:8] = [FULL, MISSING_ONE, ENDS, OUTSIDE, 0, 1, 2, FULL]
        return s.astype(np.int32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


@functools.lru_cache(maxsize=None)
def _graph():
    return Graph()


@functools.lru_cache(maxsize=None)
def _want(count, k, tries, ordinary=False):
    """The oracle's ``(neg, num_exhausted)`` for one size on the rectangular graph: computed once, shared, never written."""
    g = _graph()
    return oracle.negative_sample(g.indptr, g.indices, g.sources(count, ordinary), k, SEED, OFFSET, NUM_COLS, tries)


def _assert_negatives(got, want, what):
    neg, exhausted = got
    assert neg.dtype == torch.int32 and neg.is_cuda and neg.is_contiguous() and neg.shape == want[0].shape, what
    assert np.array_equal(neg.cpu().numpy(), want[0]) and exhausted == want[1] and isinstance(exhausted, int), what


def test_the_graph_has_the_rows_the_kernel_branches_on():
    g = _graph()
    row = lambda r: g.indices[g.indptr[r]:g.indptr[r + 1]]  # noqa: E731
    assert g.indptr[-1] == g.indices.size and all((g.degrees[a:b] == 0).all() for a, b in EMPTY_RUNS)
    assert g.degrees[FULL] == NUM_COLS and np.array_equal(np.setdiff1d(np.arange(NUM_COLS), row(MISSING_ONE)), [THE_MISSING])
    assert row(ENDS).tolist() == [0, NUM_COLS - 1] and row(OUTSIDE)[-1] == 300 and (g.degrees == 1).sum() > 20
    assert all((np.diff(row(r)) >= 0).all() for r in range(NUM_ROWS))
    assert sum((np.diff(row(r)) == 0).any() for r in range(NUM_ROWS)) > 15
    assert g.degrees[g.ordinary].max() <= 64 <= 0.25 * NUM_COLS and not np.array_equal(g.shuffled, g.indices)
    # no vacuous equality: the ordinary rows never run out of 16 tries, the designated rows do
    for count, k in SIZES:
        for tries in (16, 17):
            neg, exhausted = _want(count, k, tries, True)
            assert exhausted == 0 and (neg >= 0).all() and (neg < NUM_COLS).all()
    neg, exhausted = _want(200, 5, 16)
    sources = g.sources(200)
    assert (neg[sources == FULL] == -1).all() and (neg[sources == MISSING_ONE] == -1).any() and exhausted >= 10
    assert (neg[~np.isin(sources, (FULL, MISSING_ONE))] >= 0).all()
    accepted = neg[sources == MISSING_ONE]
    assert set(accepted[accepted >= 0].tolist()) <= {THE_MISSING}


@pytest.mark.parametrize("tries", TRIES)
def test_negative_sample_is_exactly_the_oracle(cuda_device, tries):
    import voltrix

    g = _graph()
    for count, k in SIZES:                                        # slots start at q = j T: every q & 3 for T = 1, 3, 17
        for ordinary in (False, True):
            src = _dev(g.sources(count, ordinary))
            got = voltrix.negative_sample(g.d_indptr, g.d_indices, src, k, SEED, OFFSET, NUM_COLS, tries)
            _assert_negatives(got, _want(count, k, tries, ordinary), (count, k, tries, ordinary))
    if tries == 16:                                               # the high words of the seed, the largest offset
        src = g.sources(200)
        for seed, offset in ((2 ** 40 + 9, 0), (2 ** 64 - 1, 2 ** 64 - 1)):
            got = voltrix.negative_sample(g.d_indptr, g.d_indices, _dev(src), 5, seed, offset, NUM_COLS, tries)
            _assert_negatives(got, oracle.negative_sample(g.indptr, g.indices, src, 5, seed, offset, NUM_COLS, tries), seed)


@pytest.mark.parametrize("tries", [3, 16])
def test_unsorted_rows_give_the_bits_of_the_sorted_graph(cuda_device, tries):
    import voltrix

    g = _graph()
    for count, k in ((257, 1), (200, 5), (4, 64)):
        src = _dev(g.sources(count))
        scan_sorted = voltrix.negative_sample(g.d_indptr, g.d_indices, src, k, SEED, OFFSET, NUM_COLS, tries, assume_sorted=False)
        scan_shuffled = voltrix.negative_sample(g.d_indptr, g.d_shuffled, src, k, SEED, OFFSET, NUM_COLS, tries, assume_sorted=False)
        _assert_negatives(scan_sorted, _want(count, k, tries), (count, k, "scan"))
        _assert_negatives(scan_shuffled, _want(count, k, tries), (count, k, "shuffled"))


def test_a_hub_row(cuda_device):
    """One row of 5,000 columns among 20,000: the binary search and the scan against the oracle."""
    import voltrix

    rng = np.random.default_rng(2)
    hub = np.sort(rng.choice(20000, 5000, replace=False))
    small = [np.sort(rng.choice(20000, 3, replace=False)) for _ in range(9)]
    rows = small[:4] + [hub] + small[4:]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    indices = np.concatenate(rows)
    src = np.concatenate([np.full(300, 4), np.arange(10)])
    want = oracle.negative_sample(indptr, indices, src, 5, SEED, OFFSET, 20000, 16)
    assert want[1] == 0 and not np.isin(want[0][:300], hub).any()
    first = ((oracle.draws(np.arange(300), 0, 1, SEED, OFFSET)[:, 0] * np.uint64(20000)) >> np.uint64(32)).astype(np.int64)
    assert 40 < np.isin(first, hub).sum() < 120                                  # about a quarter of the first tries was rejected
    for assume_sorted in (True, False):
        got = voltrix.negative_sample(_dev(indptr), _dev(indices), _dev(src), 5, SEED, OFFSET, 20000, 16, assume_sorted=assume_sorted)
        _assert_negatives(got, want, ("hub", assume_sorted))


def test_a_graph_of_one_column(cuda_device):
    import voltrix

    indptr, indices = np.array([0, 0, 1, 1, 3]), np.array([0, 0, 0])             # rows: empty, [0], empty, [0, 0]
    src = np.array([0, 1, 2, 3, 0])
    for assume_sorted in (True, False):
        neg, exhausted = voltrix.negative_sample(_dev(indptr), _dev(indices), _dev(src), 3, SEED, OFFSET, 1, 4, assume_sorted=assume_sorted)
        assert neg.cpu().tolist() == [[0, 0, 0], [-1, -1, -1], [0, 0, 0], [-1, -1, -1], [0, 0, 0]] and exhausted == 6
    # no entries at all (``indices`` is empty) and no columns at all
    none = torch.empty(0, dtype=torch.int32, device=DEV)
    neg, exhausted = voltrix.negative_sample(_dev(np.zeros(5)), none, _dev(src), 3, SEED, OFFSET, 7, 4)
    want = oracle.negative_sample(np.zeros(5), np.zeros(0), src, 3, SEED, OFFSET, 7, 4)
    _assert_negatives((neg, exhausted), want, "no entries")
    neg, exhausted = voltrix.negative_sample(_dev(indptr), _dev(indices), _dev(src), 3, SEED, OFFSET, 0, 4)
    assert (neg == -1).all() and exhausted == 15
    neg, exhausted = voltrix.negative_sample(_dev(indptr), _dev(indices), none, 3, SEED, OFFSET, 1, 4)
    assert neg.shape == (0, 3) and exhausted == 0


def test_a_square_graph_with_exclude_self(cuda_device):
    import voltrix

    g = _graph()
    src = np.resize(np.arange(NUM_COLS), 1000)
    plain = oracle.negative_sample(g.sq_indptr, g.sq_indices, src, 3, SEED, OFFSET, None, 16)
    strict = oracle.negative_sample(g.sq_indptr, g.sq_indices, src, 3, SEED, OFFSET, None, 16, True)
    assert (plain[0] == src[:, None]).any() and not (strict[0] == src[:, None]).any()
    for exclude_self, want in ((False, plain), (True, strict)):
        for assume_sorted in (True, False):
            got = voltrix.negative_sample(g.d_sq_indptr, g.d_sq_indices, _dev(src), 3, SEED, OFFSET, None, 16, exclude_self, assume_sorted)
            _assert_negatives(got, want, (exclude_self, assume_sorted))


def test_duplicate_sources_get_different_negatives(cuda_device):
    import voltrix

    g = _graph()
    src = np.full(257, ENDS)
    neg, _ = voltrix.negative_sample(g.d_indptr, g.d_indices, _dev(src), 5, SEED, OFFSET, NUM_COLS)
    got = neg.cpu().numpy()
    assert np.array_equal(got, oracle.negative_sample(g.indptr, g.indices, src, 5, SEED, OFFSET, NUM_COLS)[0])
    assert np.unique(got, axis=0).shape[0] == 257 and not np.isin(got, [0, NUM_COLS - 1]).any()
    assert np.unique(got).size > 200                                             # the 255 other columns, most of them


def _strided(a):
    wide = torch.full((2 * a.size,), -7, dtype=torch.int32, device=DEV)
    wide[::2] = _dev(a)
    return wide[::2]


def _shifted(t, by=3):
    pad = torch.full((by,), -7, dtype=torch.int32, device=DEV)
    return torch.cat([pad, t, pad])[by:-by]


def test_views_give_the_bits_of_the_contiguous_call(cuda_device):
    import voltrix

    g = _graph()
    src = g.sources(257)
    entries = np.random.default_rng(4).integers(0, g.indices.size, 257)
    want_rows, want_cols = oracle.edge_endpoints(g.indptr, g.indices, entries)
    ip, ix = _shifted(g.d_indptr, 1), _shifted(g.d_indices)
    assert not _strided(src).is_contiguous() and ip.storage_offset() == 1 and ix.storage_offset() == 3 and ip.data_ptr() % 16 == 4
    for view_ip, view_ix, view_src in ((g.d_indptr, g.d_indices, _strided(src)), (ip, ix, _shifted(_dev(src))), (ip, ix, _strided(src))):
        got = voltrix.negative_sample(view_ip, view_ix, view_src, 3, SEED, OFFSET, NUM_COLS, 16)
        _assert_negatives(got, _want(257, 3, 16), "views")
    for view_ip, view_ix, view_entries in ((g.d_indptr, g.d_indices, _strided(entries)), (ip, ix, _shifted(_dev(entries)))):
        rows, cols = voltrix.edge_endpoints(view_ip, view_ix, view_entries)
        assert np.array_equal(rows.cpu().numpy(), want_rows) and np.array_equal(cols.cpu().numpy(), want_cols)


def test_edge_endpoints(cuda_device):
    import voltrix

    g = _graph()
    nnz = g.indices.size
    around = [e for a, b in EMPTY_RUNS for e in (g.indptr[a] - 1, g.indptr[b]) if 0 <= e < nnz]      # both sides of every empty run
    assert len(around) == 4 and g.indptr[EMPTY_RUNS[0][1]] == 0 and g.indptr[EMPTY_RUNS[2][0]] == nnz
    for entries in ([0], [nnz - 1], [0, nnz - 1, nnz - 1, 0], around, np.arange(nnz), np.random.default_rng(5).integers(0, nnz, 257)):
        entries = np.asarray(entries)
        rows, cols = voltrix.edge_endpoints(g.d_indptr, g.d_indices, _dev(entries))
        assert rows.dtype == cols.dtype == torch.int32 and rows.shape == cols.shape == entries.shape
        want = np.searchsorted(g.indptr, entries, side="right") - 1
        assert np.array_equal(rows.cpu().numpy(), want) and np.array_equal(cols.cpu().numpy(), g.indices[entries])
        assert (g.degrees[want] > 0).all() and (g.indptr[want] <= entries).all() and (entries < g.indptr[want + 1]).all()
    assert np.array_equal(oracle.edge_endpoints(g.indptr, g.indices, np.arange(nnz))[0], np.repeat(np.arange(NUM_ROWS), g.degrees))
    rows, cols = voltrix.edge_endpoints(g.d_indptr, g.d_indices, torch.empty(0, dtype=torch.int32, device=DEV))
    assert rows.shape == cols.shape == (0,)


@pytest.mark.parametrize("bad", [-1, None, 2 ** 31 - 1, -2 ** 31])
def test_ids_out_of_range_are_a_value_error(cuda_device, bad):
    import voltrix

    g = _graph()
    src, entries = g.sources(65), np.arange(65) * 7
    bad_src, bad_entries = src.copy(), entries.copy()
    bad_src[40] = NUM_ROWS if bad is None else bad
    bad_entries[40] = g.indices.size if bad is None else bad
    with pytest.raises(ValueError, match="source"):
        voltrix.negative_sample(g.d_indptr, g.d_indices, _dev(bad_src), 3, SEED, OFFSET, NUM_COLS)
    with pytest.raises(ValueError, match="entry"):
        voltrix.edge_endpoints(g.d_indptr, g.d_indices, _dev(bad_entries))
    with pytest.raises(ValueError, match="entry"):
        voltrix.sample_edge_batch(g.d_sq_indptr, g.d_sq_indices, _dev(bad_entries), 3, (3, 3), SEED)
    torch.cuda.synchronize()                                              # and no fault: the device still answers
    got = voltrix.negative_sample(g.d_indptr, g.d_indices, _dev(src), 3, SEED, OFFSET, NUM_COLS, 16)
    _assert_negatives(got, oracle.negative_sample(g.indptr, g.indices, src, 3, SEED, OFFSET, NUM_COLS, 16), "after the refusals")
    rows, _ = voltrix.edge_endpoints(g.d_indptr, g.d_indices, _dev(entries))
    assert np.array_equal(rows.cpu().numpy(), oracle.edge_endpoints(g.indptr, g.indices, entries)[0])


def _batch_entries(exhausting):
    """65 entries of the square graph, one source several times; with ``exhausting`` three of them lie in the full row."""
    g = _graph()
    pool = np.concatenate([np.arange(g.sq_indptr[FULL]), np.arange(g.sq_indptr[MISSING_ONE + 1], g.sq_indices.size)])
    entries = np.random.default_rng(6).choice(pool, 65, replace=False)
    if exhausting:
        entries[:3] = g.sq_indptr[FULL] + np.array([0, 100, 256])
    entries[3:5] = g.sq_indptr[ENDS] + np.arange(2)                            # two edges of one source
    return entries.astype(np.int32)


def _assert_batch(batch, want, indptr, indices, fanouts, seed, offset, what):
    p = batch.pairs
    count = want["src"].size
    assert p.num_rows == count and p.num_cols == want["node_ids"].size == batch.node_ids.numel() and batch.num_exhausted == want["num_exhausted"]
    for name, got, ref in (("node_ids", batch.node_ids, want["node_ids"]), ("indptr", p.indptr, want["indptr"]),
                           ("indices", p.indices, want["indices"]), ("src_local", batch.src_local, want["src_local"])):
        assert got.dtype == torch.int32 and got.is_cuda and np.array_equal(got.cpu().numpy(), ref), (what, name)
    assert batch.labels.dtype == torch.float32 and np.array_equal(batch.labels.cpu().numpy(), want["labels"])
    ids, ptr, local = want["node_ids"], want["indptr"], p.indices.cpu().numpy()
    assert (np.diff(ids) > 0).all() and np.array_equal(ids[batch.src_local.cpu().numpy()], want["src"])
    for i in range(count):                                                       # destinations and negatives row by row
        row = ids[local[ptr[i]:ptr[i + 1]]]
        kept = want["neg"][i][want["neg"][i] >= 0]
        assert row[0] == want["dst"][i] and np.array_equal(row[1:], kept), (what, i)
        assert batch.labels[ptr[i]] == 1 and not batch.labels[ptr[i] + 1:ptr[i + 1]].any()
    assert float(batch.labels.sum()) == count
    blocks = sample_oracle.sample_blocks(indptr, indices, ids, fanouts, seed, offset)
    assert len(batch.blocks) == len(blocks) and torch.equal(batch.blocks[-1].dst_ids, batch.node_ids)
    for got, ref in zip(batch.blocks, blocks):
        assert np.array_equal(got.pattern.indptr.cpu().numpy(), ref["indptr"]) and np.array_equal(got.pattern.indices.cpu().numpy(), ref["indices"])
        assert np.array_equal(got.src_ids.cpu().numpy(), ref["src_ids"]) and np.array_equal(got.entries.cpu().numpy(), ref["entries"])
    # the transpose the pattern operators use
    order = p.t_order.cpu().numpy()
    row_of = np.repeat(np.arange(count), np.diff(ptr))
    assert np.array_equal(np.sort(order), np.arange(p.num_edges)) and np.array_equal(p.t_indices.cpu().numpy(), row_of[order])
    assert np.array_equal(np.repeat(np.arange(p.num_cols), np.diff(p.t_indptr.cpu().numpy())), local[order])


@pytest.mark.parametrize("exhausting", [False, True])
def test_sample_edge_batch(cuda_device, exhausting):
    import voltrix

    g = _graph()
    entries, fanouts = _batch_entries(exhausting), (3, 4)
    want = oracle.edge_batch(g.sq_indptr, g.sq_indices, entries, 3, SEED, OFFSET)
    assert (want["num_exhausted"] >= 9) == exhausting and (exhausting or want["num_exhausted"] == 0)
    assert np.unique(want["src"]).size < 65
    batch = voltrix.sample_edge_batch(g.d_sq_indptr, g.d_sq_indices, _dev(entries), 3, fanouts, SEED, OFFSET)
    _assert_batch(batch, want, g.sq_indptr, g.sq_indices, fanouts, SEED, OFFSET, exhausting)
    loose = voltrix.sample_edge_batch(g.d_sq_indptr, g.d_sq_indices, _dev(entries), 3, fanouts, SEED, OFFSET, exclude_self=False, max_tries=2)
    want = oracle.edge_batch(g.sq_indptr, g.sq_indices, entries, 3, SEED, OFFSET, 2, False)
    assert want["num_exhausted"] > 0
    _assert_batch(loose, want, g.sq_indptr, g.sq_indices, fanouts, SEED, OFFSET, (exhausting, "two tries"))


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_outputs_do_not_depend_on_what_their_memory_held(cuda_device, byte):
    import voltrix

    g = _graph()
    src, entries = _dev(g.sources(257)), _dev(_batch_entries(True))
    want_neg = voltrix.negative_sample(g.d_indptr, g.d_indices, src, 5, SEED, OFFSET, NUM_COLS, 3)
    want_scan = voltrix.negative_sample(g.d_indptr, g.d_shuffled, src, 5, SEED, OFFSET, NUM_COLS, 3, assume_sorted=False)
    want_ends = voltrix.edge_endpoints(g.d_sq_indptr, g.d_sq_indices, entries)
    want_batch = voltrix.sample_edge_batch(g.d_sq_indptr, g.d_sq_indices, entries, 3, (3, 4), SEED, OFFSET)
    with poisoned(byte) as state:
        got_neg = voltrix.negative_sample(g.d_indptr, g.d_indices, src, 5, SEED, OFFSET, NUM_COLS, 3)
        got_scan = voltrix.negative_sample(g.d_indptr, g.d_shuffled, src, 5, SEED, OFFSET, NUM_COLS, 3, assume_sorted=False)
        after_negatives = state.filled
        got_ends = voltrix.edge_endpoints(g.d_sq_indptr, g.d_sq_indices, entries)
        after_endpoints = state.filled
        got_batch = voltrix.sample_edge_batch(g.d_sq_indptr, g.d_sq_indices, entries, 3, (3, 4), SEED, OFFSET)
    assert after_negatives >= 2 and after_endpoints >= after_negatives + 2           # neg twice; rows, cols
    assert state.filled >= after_endpoints + 2 + 1 + 2 + 1                            # rows, cols; neg; compact_block's two; the pairs
    assert want_neg[1] > 0 and torch.equal(got_neg[0], want_neg[0]) and got_neg[1] == want_neg[1]
    assert torch.equal(got_scan[0], want_scan[0]) and torch.equal(got_scan[0], got_neg[0])
    assert torch.equal(got_ends[0], want_ends[0]) and torch.equal(got_ends[1], want_ends[1])
    _assert_negatives(got_neg, _want(257, 5, 3), "poisoned")
    for name in ("indptr", "indices", "t_indptr", "t_indices", "t_order"):
        assert torch.equal(getattr(got_batch.pairs, name), getattr(want_batch.pairs, name)), name
        assert torch.equal(getattr(got_batch.blocks[0].pattern, name), getattr(want_batch.blocks[0].pattern, name)), name
    assert torch.equal(got_batch.node_ids, want_batch.node_ids) and torch.equal(got_batch.labels, want_batch.labels)
    assert torch.equal(got_batch.src_local, want_batch.src_local) and got_batch.num_exhausted == want_batch.num_exhausted > 0


def test_sddmm_takes_the_pairs_as_they_are(cuda_device):
    """``SDDMM(batch.pairs)(h[src_local], h)``: the forward and the gradients of both operands against the float64 composite on the
    oracle's arrays, within the bounds tests/test_gpu_sddmm.py holds the operator to."""
    import voltrix
    from test_gpu_sddmm import _check, _rows
    from voltrix.autograd import SDDMM

    def scale_and_degree(owner, other, feat, size):
        """csr(|w|) @ |feat| and the row degrees of the pattern whose entry e lies in row owner[e] and column other[e] (the scale
        test_gpu_sddmm.py's _csr_grad_bound takes from a sparse product; a row of the pairs does not ascend, so it is summed here)."""
        scale = torch.zeros(size, feat.shape[1], dtype=torch.float64, device="cuda")
        scale.index_add_(0, owner, w.double().abs()[:, None] * feat.double().abs()[other])
        return scale, torch.bincount(owner, minlength=size).double()[:, None]


    g = _graph()
    batch = voltrix.sample_edge_batch(g.d_sq_indptr, g.d_sq_indices, _dev(_batch_entries(True)), 3, (3, 4), SEED, OFFSET)
    p = batch.pairs
    count, nodes, width = p.num_rows, p.num_cols, 40
    gen = torch.Generator(device="cuda").manual_seed(11)
    h = torch.randn(nodes, width, device="cuda", generator=gen)
    w = torch.randn(p.num_edges, device="cuda", generator=gen)
    x, y = h[batch.src_local.long()].clone().requires_grad_(True), h.clone().requires_grad_(True)
    s = SDDMM(p)(x, y)
    _check(p.indptr, p.indices, x.detach(), y.detach(), s.detach(), False)
    (s * w).sum().backward()
    x64, y64 = x.detach().double().requires_grad_(True), y.detach().double().requires_grad_(True)
    rows, cols = _rows(p.indptr), p.indices.long()
    ((x64[rows] * y64[cols]).sum(1) * w.double()).sum().backward()
    for grad, ref, (scale, deg) in ((x.grad, x64.grad, scale_and_degree(rows, cols, y.detach(), count)),
                                    (y.grad, y64.grad, scale_and_degree(cols, rows, x.detach(), nodes))):
        assert grad.dtype == torch.float32 and ref.abs().max() > 0
        assert ((grad.double() - ref).abs() <= (deg + 1) * 2.0 ** -23 * scale + 1e-30).all()


def test_linkpred_example_trains(cuda_device):
    """examples/linkpred_train.py's model, at the learning rate its main() uses, on one edge batch of the square test graph, the same
    batch six times: every loss finite, every parameter with a finite gradient, and every later loss below the first one -- the model
    fits the batch it is shown.  (Not "each below the one before": the dot-product decoder is quadratic in the encoder's output, and
    Adam's steps on it are not monotone.)"""
    import os
    import sys

    from conftest import REPO

    sys.path.insert(0, os.path.join(REPO, "examples"))
    try:
        import linkpred_train as example
    finally:
        sys.path.remove(os.path.join(REPO, "examples"))
    g = _graph()
    in_feats, hidden = 24, 32
    torch.manual_seed(9)
    model = example.LinkPredictor(in_feats, hidden).to(DEV)
    x = torch.randn(NUM_COLS, in_feats, device=DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    entries = _dev(_batch_entries(True))
    losses = [float(example.train_step(model, opt, g.d_sq_indptr, g.d_sq_indices, x, entries, seed=5, step=0, fanouts=(3, 4), negatives=3))
              for _ in range(6)]
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in model.parameters())
    assert all(np.isfinite(losses)) and all(later < losses[0] for later in losses[1:]), losses
