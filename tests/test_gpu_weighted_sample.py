"""GPU: voltrix.sampling_weights and sample_neighbors / sample_blocks with ``prob=`` against the numpy restatement of the weighted rule
(tests/weighted_sample_oracle.py) -- exactly, element by element.

One hand-built square CSR of 300 rows (weighted_sample_oracle.build_graph): an empty row, a row of zero weights only, for every fan-out
k rows with k - 1, k and k + 1 positive entries among zero ones (the first and the last entry of each are zero), row 0 (begin == 0:
cum[-1] must not be read) and the last row, a row of 8 entries at the row maximum (T = 2^33: 64 bits) and a hub row of 5,000 entries
with one weight 1.0 and the rest 1e-9, the dominated row on which a rejection loop would spin.  Seed counts 1, 255, 256, 257 and 1,000
(a partial, a full, a second and a fourth workgroup), shuffled, with duplicates."""
import ctypes

import numpy as np
import pytest
import torch

import weighted_sample_oracle as oracle
from poisoned_alloc import poisoned

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED, OFFSET = 20261020, 2 ** 32 + 7


class Graph:
    def __init__(self):
        self.indptr, self.indices, self.prob, self.notes = oracle.build_graph()
        self.q, self.cum, self.positive = oracle.weight_table(self.indptr, self.prob)
        self.d_indptr, self.d_indices = torch.from_numpy(self.indptr).to(DEV), torch.from_numpy(self.indices).to(DEV)
        self._weights, self._wanted = None, {}

    @property
    def weights(self):
        import voltrix

        if self._weights is None:
            self._weights = voltrix.sampling_weights(self.d_indptr, torch.from_numpy(self.prob).to(DEV))
        return self._weights

    def wanted(self, count, fanout, replace):
        """The oracle's answer for the seed set of ``count`` rows: computed once, shared by the tests that need it."""
        key = (count, fanout, replace)
        if key not in self._wanted:
            self._wanted[key] = oracle.sample_neighbors(self.indptr, self.indices, self.q, oracle.seed_sets(count), fanout, SEED, OFFSET,
                                                        replace)
        return self._wanted[key]


_GRAPH = None


def _graph():
    global _GRAPH
    if _GRAPH is None:
        _GRAPH = Graph()
    return _GRAPH


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _assert_equals_oracle(got, want, what):
    assert len(got) == len(want) == 3
    for name, g, w in zip(("s_indptr", "s_indices", "s_entries"), got, want):
        assert g.dtype == torch.int32 and g.is_cuda and g.is_contiguous(), (what, name)
        assert np.array_equal(g.cpu().numpy(), w), (what, name)


def test_the_graph_has_the_rows_the_rule_branches_on():
    g = _graph()
    degree = np.diff(g.indptr)
    assert g.indptr.size == oracle.NUM_ROWS + 1 and degree[1] == 0 and degree[2] > 0 and g.positive[2] == 0 and g.positive[1] == 0
    assert g.indptr[0] == 0 and g.positive[0] == degree[0] > 10 and g.positive[-1] == degree[-1] > 10
    for k in (1, 2, 10, 64):
        for p in (k - 1, k, k + 1):
            rows = [r for (pp, d), r in g.notes.items() if pp == p]
            assert rows, (k, p)
            for r in rows:
                assert g.positive[r] == p and g.q[g.indptr[r]] == 0 and g.q[g.indptr[r + 1] - 1] == 0
    flat = g.q[g.indptr[oracle.FLAT_ROW]:g.indptr[oracle.FLAT_ROW + 1]]
    assert flat.tolist() == [1 << 30] * 8 and int(flat.sum()) == 2 ** 33
    hub = g.q[g.indptr[oracle.HUB_ROW]:g.indptr[oracle.HUB_ROW + 1]]
    assert hub.size == 5000 and hub.max() == 1 << 30 and (hub == 1).sum() == 4999
    for count in oracle.SEED_COUNTS:
        s = oracle.seed_sets(count)
        assert s.size == count and s.min() >= 0 and s.max() < oracle.NUM_ROWS
        if count > 1:
            assert np.unique(s).size < count and not (np.diff(s) >= 0).all() and {0, 1, 2, 299, oracle.FLAT_ROW, oracle.HUB_ROW} <= set(s)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_the_table_equals_the_numpy_table_bit_for_bit(cuda_device, dtype):
    import voltrix

    g = _graph()
    prob = torch.from_numpy(g.prob).to(dtype)
    q, cum, positive = oracle.weight_table(g.indptr, prob.numpy())
    table = voltrix.sampling_weights(g.d_indptr, prob.to(DEV))
    assert isinstance(table, voltrix.SamplingWeights) and (table.nnz, table.num_rows) == (g.indices.size, oracle.NUM_ROWS)
    assert table.cum.dtype == torch.int64 and table.positive.dtype == torch.int32 and table.cum.is_cuda and table.positive.is_cuda
    assert np.array_equal(table.cum.cpu().numpy(), cum) and np.array_equal(table.positive.cpu().numpy(), positive)
    if dtype == torch.float64:
        assert np.array_equal(cum, g.cum)
    # the weights are relative within a row: a power of two changes nothing; the 16-bit types go through float64 exactly
    again = voltrix.sampling_weights(g.d_indptr, (prob * 8).to(DEV))
    assert torch.equal(again.cum, table.cum) and torch.equal(again.positive, table.positive)
    half = torch.from_numpy(g.prob).to(torch.bfloat16)
    want = oracle.weight_table(g.indptr, half.double().numpy())
    got = voltrix.sampling_weights(g.d_indptr, half.to(DEV))
    assert np.array_equal(got.cum.cpu().numpy(), want[1]) and np.array_equal(got.positive.cpu().numpy(), want[2])


def test_sampling_weights_refuses_what_is_no_weight(cuda_device):
    import voltrix

    g = _graph()
    for bad in (-1e-30, float("inf"), float("nan")):
        prob = torch.from_numpy(g.prob).to(DEV)
        prob[12345] = bad
        with pytest.raises(ValueError):
            voltrix.sampling_weights(g.d_indptr, prob)
    with pytest.raises(ValueError):                                       # one weight short of the CSR's entries
        voltrix.sampling_weights(g.d_indptr, torch.from_numpy(g.prob[:-1]).to(DEV))
    with pytest.raises(ValueError):
        voltrix.sampling_weights(g.d_indptr, torch.from_numpy(g.prob).to(DEV).long())
    torch.cuda.synchronize()


@pytest.mark.parametrize("replace", [False, True])
@pytest.mark.parametrize("fanout", oracle.FANOUTS)
def test_exactly_the_oracle(cuda_device, fanout, replace):
    import voltrix

    g = _graph()
    for count in oracle.SEED_COUNTS:
        seeds = oracle.seed_sets(count)
        got = voltrix.sample_neighbors(g.d_indptr, g.d_indices, _dev(seeds), fanout, SEED, OFFSET, replace, prob=g.weights)
        _assert_equals_oracle(got, g.wanted(count, fanout, replace), (fanout, replace, count))
        s_indptr, s_indices, s_entries = (t.cpu().numpy() for t in got)
        p = g.positive[seeds]
        want_sizes = p if fanout is None else np.where(p > 0, fanout, 0) if replace else np.minimum(p, fanout)
        assert np.array_equal(np.diff(s_indptr), want_sizes)
        assert (g.q[s_entries] > 0).all()                                 # no zero-weight entry, ever
        owner = np.repeat(seeds, want_sizes)
        assert ((g.indptr[owner] <= s_entries) & (s_entries < g.indptr[owner + 1])).all() and np.array_equal(g.indices[s_entries], s_indices)
        if not replace:                                                   # CSR order within a row: sorted rows stay sorted
            same_row = np.repeat(np.arange(count), want_sizes)
            inner = same_row[1:] == same_row[:-1]
            assert (np.diff(s_entries)[inner] > 0).all()
            assert (np.diff(s_indices)[inner & (owner[1:] % 3 != 0)] >= 0).all()


def test_outputs_do_not_depend_on_what_their_memory_held(cuda_device):
    import voltrix

    g = _graph()
    seeds = _dev(oracle.seed_sets(257))
    for fanout, replace in ((10, False), (10, True), (None, False), (64, False)):
        results = []
        for byte in (0x00, 0xFF):
            with poisoned(byte) as state:
                results.append(voltrix.sample_neighbors(g.d_indptr, g.d_indices, seeds, fanout, SEED, OFFSET, replace, prob=g.weights))
            assert state.filled >= 2                                      # s_indices, s_entries
        assert all(torch.equal(a, b) for a, b in zip(*results))
        _assert_equals_oracle(results[0], g.wanted(257, fanout, replace), (fanout, replace))


def test_a_rows_sample_does_not_depend_on_its_batch(cuda_device):
    import voltrix

    g = _graph()
    a_seeds, b_seeds = oracle.seed_sets(257), oracle.seed_sets(1000)[::-1].copy()
    for fanout, replace in ((10, False), (2, True)):
        a = [t.cpu().numpy() for t in voltrix.sample_neighbors(g.d_indptr, g.d_indices, _dev(a_seeds), fanout, SEED, OFFSET, replace,
                                                                prob=g.weights)]
        b = [t.cpu().numpy() for t in voltrix.sample_neighbors(g.d_indptr, g.d_indices, _dev(b_seeds), fanout, SEED, OFFSET, replace,
                                                                prob=g.weights)]
        where = {int(r): i for i, r in enumerate(b_seeds)}
        shared = [(i, where[int(r)]) for i, r in enumerate(a_seeds) if int(r) in where]
        assert len(shared) > 100
        for i, j in shared:
            assert np.array_equal(a[2][a[0][i]:a[0][i + 1]], b[2][b[0][j]:b[0][j + 1]]), a_seeds[i]
        alone = voltrix.sample_neighbors(g.d_indptr, g.d_indices, _dev([oracle.HUB_ROW]), fanout, SEED, OFFSET, replace, prob=g.weights)
        i = int(np.flatnonzero(a_seeds == oracle.HUB_ROW)[0])
        assert np.array_equal(alone[2].cpu().numpy(), a[2][a[0][i]:a[0][i + 1]])
        other = voltrix.sample_neighbors(g.d_indptr, g.d_indices, _dev(a_seeds), fanout, SEED, OFFSET + 1, replace, prob=g.weights)
        assert np.array_equal(a[0], other[0].cpu().numpy()) and not np.array_equal(a[2], other[2].cpu().numpy())


@pytest.mark.parametrize("replace", [False, True])
def test_sample_blocks_with_weights(cuda_device, replace):
    import voltrix

    g = _graph()
    seeds = np.unique(oracle.seed_sets(255))[::-1].copy()                 # sample_blocks wants distinct seeds
    got = voltrix.sample_blocks(g.d_indptr, g.d_indices, _dev(seeds), (3, 2), SEED, OFFSET, replace, prob=g.weights)
    want = oracle.sample_blocks(g.indptr, g.indices, g.q, seeds, (3, 2), SEED, OFFSET, replace)
    assert len(got) == len(want) == 2
    for block, ref in zip(got, want):
        p = block.pattern
        assert (block.num_dst, block.num_src) == (ref["num_dst"], ref["num_src"]) == (p.num_rows, p.num_cols)
        for name, tensor in (("indptr", p.indptr), ("indices", p.indices), ("entries", block.entries), ("src_ids", block.src_ids),
                             ("dst_ids", block.dst_ids)):
            assert tensor.dtype == torch.int32 and np.array_equal(tensor.cpu().numpy(), ref[name]), name
        assert torch.equal(block.src_ids[:block.num_dst], block.dst_ids)
        entries = block.entries.cpu().numpy()
        assert (g.q[entries] > 0).all() and (g.prob[entries] > 0).all()   # entries index the original CSR: so do the weights
    assert np.array_equal(got[1].dst_ids.cpu().numpy(), seeds) and torch.equal(got[0].dst_ids, got[1].src_ids)


def test_prob_none_is_the_call_without_the_keyword(cuda_device):
    import voltrix

    g = _graph()
    seeds = _dev(oracle.seed_sets(257))
    for fanout, replace in ((10, False), (10, True), (None, False)):
        a = voltrix.sample_neighbors(g.d_indptr, g.d_indices, seeds, fanout, SEED, OFFSET, replace)
        b = voltrix.sample_neighbors(g.d_indptr, g.d_indices, seeds, fanout, SEED, OFFSET, replace, prob=None)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    distinct = _dev(np.unique(oracle.seed_sets(255)))
    a = voltrix.sample_blocks(g.d_indptr, g.d_indices, distinct, (3, 2), SEED, OFFSET)
    b = voltrix.sample_blocks(g.d_indptr, g.d_indices, distinct, (3, 2), SEED, OFFSET, prob=None)
    for x, y in zip(a, b):
        assert torch.equal(x.entries, y.entries) and torch.equal(x.src_ids, y.src_ids) and torch.equal(x.pattern.indices, y.pattern.indices)


@pytest.mark.parametrize("bad", [-1, oracle.NUM_ROWS, 2 ** 31 - 1, -2 ** 31])
def test_out_of_range_seeds_are_still_a_value_error(cuda_device, bad):
    import voltrix

    g = _graph()
    seeds = oracle.seed_sets(255).copy()
    seeds[40] = bad
    for fanout, replace in ((10, False), (10, True), (None, False)):
        with pytest.raises(ValueError):
            voltrix.sample_neighbors(g.d_indptr, g.d_indices, _dev(seeds), fanout, SEED, OFFSET, replace, prob=g.weights)
    torch.cuda.synchronize()                                              # and no fault: the device still answers
    good = voltrix.sample_neighbors(g.d_indptr, g.d_indices, _dev(oracle.seed_sets(255)), 10, SEED, OFFSET, prob=g.weights)
    _assert_equals_oracle(good, g.wanted(255, 10, False), "after the refusals")


def test_a_table_of_another_graph_is_a_value_error(cuda_device):
    import voltrix

    g = _graph()
    seeds = _dev(oracle.seed_sets(255))
    w = g.weights
    for other in (voltrix.SamplingWeights(w.cum[:-1], w.positive, w.nnz - 1, w.num_rows),
                  voltrix.SamplingWeights(w.cum, w.positive[:-1], w.nnz, w.num_rows - 1)):
        with pytest.raises(ValueError):
            voltrix.sample_neighbors(g.d_indptr, g.d_indices, seeds, 10, SEED, OFFSET, prob=other)


def test_minibatch_example_trains_on_inverse_degree_draws(cuda_device):
    """examples/sage_minibatch_train.py's weighted mode on the test graph: the table of 1 / in_degree counts every entry as positive,
    and six steps on one batch have a finite, decreasing loss, every parameter with a finite gradient."""
    import os
    import sys

    from conftest import REPO

    sys.path.insert(0, os.path.join(REPO, "examples"))
    try:
        import sage_minibatch_train as example
    finally:
        sys.path.remove(os.path.join(REPO, "examples"))
    g = _graph()
    table = example.inverse_degree_weights(g.d_indptr, g.d_indices)
    assert (table.nnz, table.num_rows) == (g.indices.size, oracle.NUM_ROWS)
    assert np.array_equal(table.positive.cpu().numpy(), np.diff(g.indptr))            # every weight is positive
    in_feats, hidden, classes = 24, 32, 7
    torch.manual_seed(9)
    model = example.BlockSAGE(in_feats, hidden, classes).to(DEV)
    x = torch.randn(oracle.NUM_ROWS, in_feats, device=DEV)
    y = torch.randint(0, classes, (oracle.NUM_ROWS,), device=DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    nodes = _dev(np.unique(oracle.seed_sets(255)))
    losses = [float(example.train_step(model, opt, g.d_indptr, g.d_indices, x, y, nodes, seed=5, step=0, fanouts=(3, 5), prob=table))
              for _ in range(6)]
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in model.parameters())
    assert all(np.isfinite(losses)) and all(b < a for a, b in zip(losses, losses[1:])), losses


def test_the_c_symbol_called_directly_equals_the_python_path(cuda_device):
    import voltrix
    from voltrix import capi

    g = _graph()
    seeds = _dev(oracle.seed_sets(257))
    fn = capi.lib().voltrix_sample_neighbors_weighted
    for fanout, replace in ((10, False), (64, False), (10, True), (None, False)):
        s_indptr, s_indices, s_entries = voltrix.sample_neighbors(g.d_indptr, g.d_indices, seeds, fanout, SEED, OFFSET, replace,
                                                                  prob=g.weights)
        total = s_indices.numel()
        cols = torch.full((total,), -7, dtype=torch.int32, device=DEV)
        entries = torch.full((total,), -7, dtype=torch.int32, device=DEV)
        rc = ctypes.c_int(-1)
        fn(g.d_indptr.data_ptr(), g.d_indices.data_ptr(), g.weights.cum.data_ptr(), oracle.NUM_ROWS, seeds.data_ptr(), seeds.numel(),
           s_indptr.data_ptr(), total, -1 if fanout is None else fanout, int(replace), SEED, OFFSET, cols.data_ptr(), entries.data_ptr(),
           torch.cuda.current_stream().cuda_stream, ctypes.byref(rc))
        torch.cuda.synchronize()
        assert rc.value == 0 and torch.equal(cols, s_indices) and torch.equal(entries, s_entries), (fanout, replace)
