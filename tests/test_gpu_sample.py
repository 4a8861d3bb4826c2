"""GPU: voltrix.sample_neighbors / compact_block / sample_blocks against the numpy restatement of the sampling rule
(tests/sample_oracle.py) -- exactly, element by element -- and the sampled blocks through SpMMReduce.

One hand-built rectangular CSR, 600 rows x 4,096 columns: the degrees cycle through 0, 1 and k - 1, k, k + 1, 2 k for every fan-out
under test, 37 and 300; one row has 5,000 entries; rows hold duplicate columns; two rows in three are sorted, the third is not.  These
are the smallest shapes at which the selection, the slot insertion, the copy path and the workgroup tail (S = 257, 600: a second and
third workgroup, the last one partial) can go wrong.  ``sample_blocks`` needs a square graph: the same rows with the columns folded
into [0, 600)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

import sample_oracle as oracle
from poisoned_alloc import poisoned

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NUM_ROWS, NUM_COLS, HUB_ROW, HUB_DEGREE = 600, 4096, 77, 5000
FANOUTS = (1, 2, 10, 25, 64, None)
DEGREES = sorted({0, 1, 37, 300} | {d for k in FANOUTS if k for d in (k - 1, k, k + 1, 2 * k)})
SEED_COUNTS = (0, 1, 63, 64, 65, 257, 600)
SEED, OFFSET = 20261019, 2 ** 32 + 7


class Graph:
    def __init__(self):
        rng = np.random.default_rng(1)
        degrees = np.array([DEGREES[r % len(DEGREES)] for r in range(NUM_ROWS)])
        degrees[HUB_ROW] = HUB_DEGREE
        self.indptr = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int32)
        rows = []
        for r, d in enumerate(degrees):
            cols = rng.integers(0, NUM_COLS, d)
            if d >= 4:
                cols[d // 2] = cols[0]                       # a duplicate column in every row of some length
            rows.append(np.sort(cols) if r % 3 else cols)    # two rows in three sorted
        self.indices = np.concatenate(rows).astype(np.int32)
        self.degrees = degrees
        self.square_indices = (self.indices % NUM_ROWS).astype(np.int32)
        self.shuffled = rng.permutation(NUM_ROWS).astype(np.int32)
        self.d_indptr, self.d_indices = torch.from_numpy(self.indptr).to(DEV), torch.from_numpy(self.indices).to(DEV)
        self.d_square = torch.from_numpy(self.square_indices).to(DEV)

    def seeds(self, count):
        """``count`` distinct rows in a shuffled order; the hub row is among them from 63 on."""
        s = self.shuffled[:count].copy()
        if count >= 63 and HUB_ROW not in s:
            s[5] = HUB_ROW
        return s


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


def test_the_graph_has_the_rows_the_kernel_branches_on():
    g = _graph()
    assert g.indptr[-1] == g.indices.size and set(DEGREES) <= set(g.degrees.tolist()) and g.degrees[HUB_ROW] == HUB_DEGREE
    unsorted = [r for r in range(NUM_ROWS) if (np.diff(g.indices[g.indptr[r]:g.indptr[r + 1]]) < 0).any()]
    dup = [r for r in range(NUM_ROWS) if np.unique(g.indices[g.indptr[r]:g.indptr[r + 1]]).size < g.degrees[r]]
    assert len(unsorted) > 50 and len(dup) > 100 and g.indices.max() >= NUM_ROWS
    for count in SEED_COUNTS:
        assert np.unique(g.seeds(count)).size == count
    assert HUB_ROW in g.seeds(63) and not (np.diff(g.seeds(600)) > 0).all()


@pytest.mark.parametrize("replace", [False, True])
@pytest.mark.parametrize("fanout", FANOUTS)
def test_exactly_the_oracle(cuda_device, fanout, replace):
    import voltrix

    g = _graph()
    for count in SEED_COUNTS:
        seeds = g.seeds(count)
        got = voltrix.sample_neighbors(g.d_indptr, g.d_indices, _dev(seeds), fanout, SEED, OFFSET, replace)
        _assert_equals_oracle(got, oracle.sample_neighbors(g.indptr, g.indices, seeds, fanout, SEED, OFFSET, replace),
                              (fanout, replace, count))
        if count == 600 and fanout is not None:
            sizes = np.diff(got[0].cpu().numpy())
            want = np.where(g.degrees[seeds] > 0, fanout, 0) if replace else np.minimum(g.degrees[seeds], fanout)
            assert np.array_equal(sizes, want)


def test_outputs_do_not_depend_on_what_their_memory_held(cuda_device):
    import voltrix

    g = _graph()
    seeds = _dev(g.seeds(257))
    for fanout, replace in ((10, False), (10, True), (None, False)):
        want = voltrix.sample_neighbors(g.d_indptr, g.d_indices, seeds, fanout, SEED, OFFSET, replace)
        want_block = voltrix.compact_block(seeds, want[1], NUM_COLS)
        with poisoned(0xFF) as state:
            got = voltrix.sample_neighbors(g.d_indptr, g.d_indices, seeds, fanout, SEED, OFFSET, replace)
            filled = state.filled
            got_block = voltrix.compact_block(seeds, got[1], NUM_COLS)
        assert filled >= 2 and state.filled >= filled + 2                 # s_indices, s_entries; src_ids, local_indices
        for a, b in zip(got + got_block, want + want_block):
            assert torch.equal(a, b)


def test_independence_and_repetition(cuda_device):
    import voltrix

    g = _graph()
    a_seeds, b_seeds = g.seeds(257), g.seeds(600)[::-1].copy()
    for fanout, replace in ((10, False), (25, True)):
        a = [t.cpu().numpy() for t in voltrix.sample_neighbors(g.d_indptr, g.d_indices, _dev(a_seeds), fanout, SEED, OFFSET, replace)]
        b = [t.cpu().numpy() for t in voltrix.sample_neighbors(g.d_indptr, g.d_indices, _dev(b_seeds), fanout, SEED, OFFSET, replace)]
        where = {int(r): i for i, r in enumerate(b_seeds)}
        for i, r in enumerate(a_seeds):                                   # a row sampled in two batches gives the same entries
            j = where[int(r)]
            assert np.array_equal(a[2][a[0][i]:a[0][i + 1]], b[2][b[0][j]:b[0][j + 1]]), r
        again = voltrix.sample_neighbors(g.d_indptr, g.d_indices, _dev(a_seeds), fanout, SEED, OFFSET, replace)
        assert all(np.array_equal(x, y.cpu().numpy()) for x, y in zip(a, again))                          # two calls, the same bits
        other = voltrix.sample_neighbors(g.d_indptr, g.d_indices, _dev(a_seeds), fanout, SEED, OFFSET + 1, replace)
        assert np.array_equal(a[0], other[0].cpu().numpy()) and not np.array_equal(a[2], other[2].cpu().numpy())
        other = voltrix.sample_neighbors(g.d_indptr, g.d_indices, _dev(a_seeds), fanout, SEED + 1, OFFSET, replace)
        assert not np.array_equal(a[2], other[2].cpu().numpy())


def test_views_give_the_bits_of_the_contiguous_call(cuda_device):
    import voltrix

    g = _graph()
    seeds = g.seeds(257)
    want = voltrix.sample_neighbors(g.d_indptr, g.d_indices, _dev(seeds), 10, SEED, OFFSET)
    strided = torch.full((2 * seeds.size,), -7, dtype=torch.int32, device=DEV)
    strided[::2] = _dev(seeds)
    shifted = torch.cat([torch.full((3,), -7, dtype=torch.int32, device=DEV), _dev(seeds)])[3:]
    ip = torch.cat([torch.zeros(1, dtype=torch.int32, device=DEV), g.d_indptr])[1:]
    assert not strided[::2].is_contiguous() and shifted.storage_offset() == 3 and ip.data_ptr() % 16 == 4
    for view_ip, view_seeds in ((g.d_indptr, strided[::2]), (g.d_indptr, shifted), (ip, shifted)):
        got = voltrix.sample_neighbors(view_ip, g.d_indices, view_seeds, 10, SEED, OFFSET)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    block = voltrix.compact_block(_dev(seeds), want[1], NUM_COLS)
    for view in (strided[::2], shifted):
        assert all(torch.equal(a, b) for a, b in zip(voltrix.compact_block(view, want[1], NUM_COLS), block))


@pytest.mark.parametrize("count", [1, 65, 600])
def test_compact_block(cuda_device, count):
    import voltrix

    g = _graph()
    seeds = g.seeds(count)
    for fanout in (3, None):
        _, s_indices, _ = voltrix.sample_neighbors(g.d_indptr, g.d_indices, _dev(seeds), fanout, SEED, OFFSET)
        src_ids, local = voltrix.compact_block(_dev(seeds), s_indices, NUM_COLS, validate=True)
        want_src, want_local = oracle.compact_block(seeds, s_indices.cpu().numpy())
        assert src_ids.dtype == torch.int32 and local.dtype == torch.int32
        src, loc = src_ids.cpu().numpy(), local.cpu().numpy()
        assert np.array_equal(src, want_src) and np.array_equal(loc, want_local)
        assert np.array_equal(src[:count], seeds) and (np.diff(src[count:]) > 0).all() and not set(src[count:]) & set(seeds.tolist())
        assert np.array_equal(src[loc], s_indices.cpu().numpy())
    # no sampled entry at all: the seeds alone
    empty = torch.empty(0, dtype=torch.int32, device=DEV)
    src_ids, local = voltrix.compact_block(_dev(seeds), empty, NUM_COLS)
    assert np.array_equal(src_ids.cpu().numpy(), seeds) and local.numel() == 0
    with pytest.raises(ValueError):                                       # duplicate seeds: a precondition, checked on request
        voltrix.compact_block(_dev(np.concatenate([seeds, seeds[:1]])), empty, NUM_COLS, validate=True)


def _blocks(replace=False):
    import voltrix

    g = _graph()
    seeds = g.seeds(65)
    got = voltrix.sample_blocks(g.d_indptr, g.d_square, _dev(seeds), (3, 2), SEED, OFFSET, replace)
    want = oracle.sample_blocks(g.indptr, g.square_indices, seeds, (3, 2), SEED, OFFSET, replace)
    return g, seeds, got, want


@pytest.mark.parametrize("replace", [False, True])
def test_sample_blocks(cuda_device, replace):
    g, seeds, got, want = _blocks(replace)
    assert len(got) == len(want) == 2
    for layer_from_output, (block, ref) in enumerate(zip(got[::-1], want[::-1])):
        p = block.pattern
        assert (block.num_dst, block.num_src) == (ref["num_dst"], ref["num_src"]) == (p.num_rows, p.num_cols)
        for name, tensor in (("indptr", p.indptr), ("indices", p.indices), ("entries", block.entries), ("src_ids", block.src_ids),
                             ("dst_ids", block.dst_ids)):
            assert tensor.dtype == torch.int32 and np.array_equal(tensor.cpu().numpy(), ref[name]), (layer_from_output, name)
        src, dst, entries = block.src_ids.cpu().numpy(), block.dst_ids.cpu().numpy(), block.entries.cpu().numpy()
        assert np.array_equal(src[:block.num_dst], dst)                                    # h_dst = h_src[:num_dst]
        assert (np.diff(src[block.num_dst:]) > 0).all() and not set(src[block.num_dst:]) & set(dst.tolist())
        local = p.indices.cpu().numpy()
        assert np.array_equal(src[local], g.square_indices[entries])                       # entries point at the CSR's own entries
        rows = np.repeat(dst, np.diff(p.indptr.cpu().numpy()))
        assert ((g.indptr[rows] <= entries) & (entries < g.indptr[rows + 1])).all()        # ... of the row they were sampled for
        # layer l from the output used offset + l and fan-out fanouts[-1 - l]
        alone = oracle.sample_neighbors(g.indptr, g.square_indices, dst, (3, 2)[-1 - layer_from_output], SEED,
                                        OFFSET + layer_from_output, replace)
        assert np.array_equal(alone[2], entries)
        # the transpose the pattern operators use
        order = p.t_order.cpu().numpy()
        assert np.array_equal(np.sort(order), np.arange(p.num_edges)) and p.t_indptr.numel() == p.num_cols + 1
        assert np.array_equal(p.t_indices.cpu().numpy(), np.repeat(np.arange(p.num_rows), np.diff(p.indptr.cpu().numpy()))[order])
    assert np.array_equal(got[1].dst_ids.cpu().numpy(), seeds) and torch.equal(got[0].dst_ids, got[1].src_ids)


@pytest.mark.parametrize("bad", [-1, NUM_ROWS, 2 ** 31 - 1, -2 ** 31])
def test_out_of_range_seeds_are_a_value_error(cuda_device, bad):
    import voltrix

    g = _graph()
    seeds = g.seeds(65).copy()
    seeds[40] = bad
    for fanout, replace in ((10, False), (10, True), (None, False)):
        with pytest.raises(ValueError):
            voltrix.sample_neighbors(g.d_indptr, g.d_indices, _dev(seeds), fanout, SEED, OFFSET, replace)
    with pytest.raises(ValueError):
        voltrix.sample_blocks(g.d_indptr, g.d_square, _dev(seeds), (3, 2), SEED)
    torch.cuda.synchronize()                                              # and no fault: the device still answers
    good = voltrix.sample_neighbors(g.d_indptr, g.d_indices, _dev(g.seeds(65)), 10, SEED, OFFSET)
    _assert_equals_oracle(good, oracle.sample_neighbors(g.indptr, g.indices, g.seeds(65), 10, SEED, OFFSET), "after the refusals")


def test_a_block_pattern_through_spmm_reduce(cuda_device):
    """max: equal to a float64 CPU composite on the sampled sub-CSR, bit for bit (a selection does not round), and so is d_feat for
    integer gradients (sums of small integers are exact in fp32); mean: within spmm_reduce's stated bound
    |out - ref| <= (deg + 1) 2^-23 sum_e |feat_e| / deg."""
    from voltrix.autograd import SpMMReduce

    g, seeds, got, want = _blocks()
    gen = torch.Generator().manual_seed(3)
    for block, ref in zip(got, want):
        dim = 20
        ip, cols = ref["indptr"].astype(np.int64), ref["indices"].astype(np.int64)
        deg = np.diff(ip)
        assert (deg == 0).any() and (deg > 1).any()
        feat = torch.randn(block.num_src, dim, generator=gen)
        grad = torch.randint(-4, 5, (block.num_dst, dim), generator=gen).float()
        f64 = feat.double().numpy()
        ref_max, ref_mean, bound = np.zeros((block.num_dst, dim)), np.zeros((block.num_dst, dim)), np.zeros((block.num_dst, dim))
        ref_grad = np.zeros((block.num_src, dim))
        for r in range(block.num_dst):
            if deg[r] == 0:
                continue
            mine = f64[cols[ip[r]:ip[r + 1]]]
            ref_max[r], ref_mean[r] = mine.max(0), mine.mean(0)
            bound[r] = (deg[r] + 1) * 2.0 ** -23 * np.abs(mine).sum(0) / deg[r]
            winner = cols[ip[r] + mine.argmax(0)]                         # the first entry in CSR order on a tie (duplicate columns)
            np.add.at(ref_grad, (winner, np.arange(dim)), grad[r].double().numpy())
        leaf = feat.to(DEV).requires_grad_(True)
        out = SpMMReduce(block.pattern, reduce="max")(leaf)
        out.backward(grad.to(DEV))
        assert out.dtype == torch.float32 and np.array_equal(out.detach().cpu().double().numpy(), ref_max)
        assert np.array_equal(leaf.grad.cpu().double().numpy(), ref_grad)
        mean = SpMMReduce(block.pattern, reduce="mean")(feat.to(DEV))
        assert (np.abs(mean.cpu().double().numpy() - ref_mean) <= bound).all()


def test_minibatch_example_trains(cuda_device):
    """examples/sage_minibatch_train.py's model on sampled batches of the folded test graph: four steps on one batch with a finite,
    decreasing loss, every parameter with a finite gradient."""
    sys.path.insert(0, os.path.join(REPO, "examples"))
    try:
        import sage_minibatch_train as example
    finally:
        sys.path.remove(os.path.join(REPO, "examples"))
    g = _graph()
    in_feats, hidden, classes = 24, 32, 7
    torch.manual_seed(9)
    model = example.BlockSAGE(in_feats, hidden, classes).to(DEV)
    x = torch.randn(NUM_ROWS, in_feats, device=DEV)
    y = torch.randint(0, classes, (NUM_ROWS,), device=DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    nodes = _dev(g.seeds(257))
    losses = [float(example.train_step(model, opt, g.d_indptr, g.d_square, x, y, nodes, seed=5, step=0, fanouts=(3, 5))) for _ in range(6)]
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in model.parameters())
    assert all(np.isfinite(losses)) and all(b < a for a, b in zip(losses, losses[1:])), losses
