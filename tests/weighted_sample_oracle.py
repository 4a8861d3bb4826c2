"""A numpy restatement of the weighted neighbour sampling rule (voltrix/weighted_sample_kernels.hpp, voltrix/sampling.py),
for the tests that hold the table builder, the kernels and the header's host code to it.  Integers only: the draws are Python integers,
the weights int64; the one floating-point step is the table's correctly rounded float64 division.

    q_e = 0 where w_e == 0 or m_r == 0, else max(1, floor((w_e / m_r) * 2^30)), m_r = the row's largest weight, in float64
    cum = the inclusive prefix sum of q over all entries (int64); positive[r] = the entries of row r with q > 0
    draw(r, n) = word n & 3 of Philox((r, (n >> 2) | 0xA0000000, offset lo, offset hi), (seed lo, seed hi))
    x_i = (draw(r, 2 i) << 32) | draw(r, 2 i + 1);  a uniform integer below R: (x_i R) >> 64
    no replacement, p <= k:   the positions with q > 0, in CSR order
    no replacement, p > k:    for i < k: R = the mass not chosen yet, t = (x_i R) >> 64, the smallest j with g(j) > t, g = the running sum
                              of q with the chosen positions set to 0; the k positions ascending
    replacement, T > 0:       position i = the smallest j with c(j) > (x_i T) >> 64, in draw order; exactly k
"""
import numpy as np

from test_attn_dropout_host import philox4x32_10

COUNTER_BITS = 0xA0000000
ONE = 1 << 30


def quantise(indptr, prob):
    """int64 [nnz]: q of every entry, row by row."""
    indptr = np.asarray(indptr, dtype=np.int64)
    w = np.asarray(prob).astype(np.float64)
    assert np.isfinite(w).all() and (w >= 0).all() and w.size == indptr[-1]
    q = np.zeros(w.size, np.int64)
    for r in range(indptr.size - 1):
        mine = w[indptr[r]:indptr[r + 1]]
        if mine.size and mine.max() > 0:
            scaled = np.floor((mine / mine.max()) * float(ONE)).astype(np.int64)
            q[indptr[r]:indptr[r + 1]] = np.where(mine > 0, np.maximum(scaled, 1), 0)
    return q


def weight_table(indptr, prob):
    """``(q, cum, positive)``: int64 [nnz], int64 [nnz], int32 [num_rows]."""
    indptr = np.asarray(indptr, dtype=np.int64)
    q = quantise(indptr, prob)
    positive = np.array([(q[indptr[r]:indptr[r + 1]] > 0).sum() for r in range(indptr.size - 1)], np.int32)
    return q, np.cumsum(q), positive


def draws64(rows, count, seed, offset):
    """A list per row of ``count`` Python integers: x_0 .. x_{count - 1}."""
    rows = np.asarray(rows, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    n = np.arange(2 * count, dtype=np.uint64)
    words = np.stack(philox4x32_10(rows[:, None], (n >> np.uint64(2)) | np.uint64(COUNTER_BITS), offset & 0xFFFFFFFF, offset >> 32,
                                   seed & 0xFFFFFFFF, seed >> 32), -1)                   # [rows, 2 count, 4]
    pick = np.broadcast_to((n & np.uint64(3)).astype(np.int64)[None, :, None], words.shape[:2] + (1,))
    halves = np.take_along_axis(words, pick, -1)[..., 0].astype(np.uint64).tolist()
    return [[(row[2 * i] << 32) | row[2 * i + 1] for i in range(count)] for row in halves]


def successive_positions(q_row, x):
    """The ascending positions successive sampling takes from a row with the int64 weights ``q_row`` and the draws ``x``
    (len(x) = k, below the row's count of positive weights)."""
    left = np.array(q_row, dtype=np.int64)
    assert (left > 0).sum() > len(x)
    chosen = []
    for x_i in x:
        g = np.cumsum(left)
        t = (x_i * int(g[-1])) >> 64
        j = int(np.searchsorted(g, t, side="right"))                       # the smallest j with g(j) > t
        assert left[j] > 0
        chosen.append(j)
        left[j] = 0
    return sorted(chosen)


def replace_positions(q_row, x):
    """The positions the replacement rule takes from a row of positive total weight, in draw order."""
    c = np.cumsum(np.asarray(q_row, dtype=np.int64))
    total = int(c[-1])
    assert total > 0
    return [int(np.searchsorted(c, (x_i * total) >> 64, side="right")) for x_i in x]


def row_positions(q_row, r, k, seed, offset, replace):
    """The positions of one row by the rule (``k=None``: every positive entry)."""
    q_row = np.asarray(q_row, dtype=np.int64)
    positive = np.flatnonzero(q_row > 0)
    if k is None or (not replace and positive.size <= k):
        return positive.tolist()
    if positive.size == 0:
        return []
    x = draws64([r], k, seed, offset)[0]
    return replace_positions(q_row, x) if replace else successive_positions(q_row, x)


def sample_neighbors(indptr, indices, q, seeds, fanout, seed, offset=0, replace=False):
    """``(s_indptr, s_indices, s_entries)`` as int32 arrays: what voltrix.sample_neighbors(prob=) returns for in-range seeds."""
    indptr, indices, seeds = (np.asarray(v, dtype=np.int64) for v in (indptr, indices, seeds))
    entries, counts = [], []
    memo = {}
    for r in seeds.tolist():
        if r not in memo:
            begin, end = int(indptr[r]), int(indptr[r + 1])
            memo[r] = [begin + j for j in row_positions(q[begin:end], r, fanout, seed, offset, replace)]
        entries.extend(memo[r])
        counts.append(len(memo[r]))
    entries = np.array(entries, np.int64)
    s_indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return s_indptr, indices[entries].astype(np.int32), entries.astype(np.int32)


def sample_blocks(indptr, indices, q, seeds, fanouts, seed, offset=0, replace=False):
    """The blocks of voltrix.sample_blocks(prob=) as dicts of int32 arrays, input layer first: layer l from the output samples with
    offset + l, every layer with the one table."""
    from sample_oracle import compact_block

    blocks, dst_ids = [], np.asarray(seeds, dtype=np.int64)
    for layer, fanout in enumerate(reversed(list(fanouts))):
        s_indptr, s_indices, entries = sample_neighbors(indptr, indices, q, dst_ids, fanout, seed, (offset + layer) % 2 ** 64, replace)
        src_ids, local = compact_block(dst_ids, s_indices)
        blocks.append({"indptr": s_indptr, "indices": local, "s_indices": s_indices, "entries": entries, "src_ids": src_ids,
                       "dst_ids": dst_ids.astype(np.int32), "num_dst": dst_ids.size, "num_src": src_ids.size})
        dst_ids = src_ids.astype(np.int64)
    return blocks[::-1]


# ---- the graph of the GPU tests and of the host program: 300 rows, square, with the rows the rule branches on
NUM_ROWS, HUB_ROW, HUB_DEGREE, FLAT_ROW = 300, 77, 5000, 41
FANOUTS = (1, 2, 10, 64, None)


def build_graph():
    """``(indptr int32, indices int32, prob float64, notes)``.  Row 0 (begin == 0) and the last row are drawn rows; row 1 is empty;
    row 2 has only zero weights; for every fan-out k there are rows with p = k - 1, k and k + 1 positive entries among zero ones, the
    first and the last entry of each with weight zero; FLAT_ROW has 8 entries at the row maximum (T = 2^33); HUB_ROW has 5,000 entries,
    one of weight 1.0 and the rest 1e-9 (they quantise to 1: the dominated row on which a rejection loop would spin).  Two rows in
    three are sorted."""
    rng = np.random.default_rng(7)
    rows_w, notes = [], {}
    shapes = [(p, p + z) for k in (1, 2, 10, 64) for p in (k - 1, k, k + 1) for z in (2, 5) if p >= 0]     # (positive, degree)
    for r in range(NUM_ROWS):
        if r == 1:
            w = np.zeros(0)
        elif r == 2:
            w = np.zeros(6)
        elif r == FLAT_ROW:
            w = np.full(8, 3.5)
        elif r == HUB_ROW:
            w = np.full(HUB_DEGREE, 1e-9)
            w[1234] = 1.0
        elif r in (0, NUM_ROWS - 1):
            w = rng.random(40) + 0.01                                      # every entry positive, p > k for k <= 10
        elif r % 2:
            p, d = shapes[(r // 2) % len(shapes)]
            w = np.zeros(d)
            inner = 1 + rng.permutation(d - 2)[:p]                         # the first and the last entry stay zero
            w[inner] = rng.random(p) * 10.0 ** int(rng.integers(-3, 3)) + 1e-4
            notes.setdefault((p, d), r)
        else:
            d = int(rng.integers(1, 200))
            w = rng.random(d) ** 4                                         # skewed
            w[rng.random(d) < 0.2] = 0.0
        rows_w.append(w)
    degrees = np.array([w.size for w in rows_w])
    indptr = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int32)
    cols = []
    for r, d in enumerate(degrees):
        c = rng.integers(0, NUM_ROWS, d)
        cols.append(np.sort(c) if r % 3 else c)
    return indptr, np.concatenate(cols).astype(np.int32), np.concatenate(rows_w), notes


def seed_sets(count):
    """``count`` seed rows, shuffled, with duplicates from 255 on; the special rows are among them from 255 on."""
    rng = np.random.default_rng(100 + count)
    if count == 1:
        return np.array([HUB_ROW], np.int32)
    s = rng.integers(0, NUM_ROWS, count)
    s[:8] = [0, NUM_ROWS - 1, 1, 2, FLAT_ROW, HUB_ROW, HUB_ROW, 0]
    return rng.permutation(s).astype(np.int32)


SEED_COUNTS = (1, 255, 256, 257, 1000)
