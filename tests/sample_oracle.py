"""A numpy restatement of the neighbour sampling rule (voltrix/neighbor_sample_kernels.hpp, voltrix/sampling.py), for the
tests that hold the kernels to it.  Philox4x32-10 is the restatement of tests/test_attn_dropout_host.py; everything here is vectorised
over rows and works on host arrays only.

    draw(r, i) = word i & 3 of Philox((r, (i >> 2) | 0x80000000, offset lo, offset hi), (seed lo, seed hi))
    d <= k, no replacement:   positions 0 .. d - 1
    d > k, no replacement:    Floyd: for i < k, j = d - k + i, t = (draw(r, i) * (j + 1)) >> 32, take t unless taken, then j; ascending
    replacement, d > 0:       position i = (draw(r, i) * d) >> 32, in draw order; exactly k
"""
import numpy as np

from test_attn_dropout_host import philox4x32_10

COUNTER_BIT = 0x80000000


def draws(rows, count, seed, offset):
    """uint64 [len(rows), count]: draw(r, i) for every row id in ``rows`` and i < count."""
    rows = np.asarray(rows, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    i = np.arange(count, dtype=np.uint64)
    words = np.stack(philox4x32_10(rows[:, None], (i >> np.uint64(2)) | np.uint64(COUNTER_BIT), offset & 0xFFFFFFFF, offset >> 32,
                                   seed & 0xFFFFFFFF, seed >> 32), -1)                       # [rows, count, 4]
    pick = np.broadcast_to((i & np.uint64(3)).astype(np.int64)[None, :, None], words.shape[:2] + (1,))
    return np.take_along_axis(words, pick, -1)[..., 0].astype(np.uint64)


def floyd_positions(rows, degrees, k, seed, offset):
    """int64 [len(rows), k], ascending: the positions the rule takes from rows of degree ``degrees`` (every one above k)."""
    rows, degrees = np.asarray(rows, dtype=np.int64), np.broadcast_to(np.asarray(degrees, dtype=np.int64), np.shape(rows))
    assert (degrees > k).all() and k >= 1
    x = draws(rows, k, seed, offset)
    taken = np.full((rows.size, k), -1, np.int64)
    for i in range(k):
        j = degrees - k + i
        t = ((x[:, i] * (j + 1).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
        assert (t >= 0).all() and (t <= j).all()
        seen = (taken[:, :i] == t[:, None]).any(1)
        taken[:, i] = np.where(seen, j, t)
    return np.sort(taken, 1)


def replace_positions(rows, degrees, k, seed, offset):
    """int64 [len(rows), k], in draw order: the positions the replacement rule takes from rows of degree ``degrees`` > 0."""
    degrees = np.broadcast_to(np.asarray(degrees, dtype=np.int64), np.shape(rows))
    assert (degrees > 0).all()
    return ((draws(rows, k, seed, offset) * degrees.astype(np.uint64)[:, None]) >> np.uint64(32)).astype(np.int64)


def sample_neighbors(indptr, indices, seeds, fanout, seed, offset=0, replace=False):
    """``(s_indptr, s_indices, s_entries)`` as int32 arrays: what voltrix.sample_neighbors returns for in-range seeds."""
    indptr, indices, seeds = (np.asarray(v, dtype=np.int64) for v in (indptr, indices, seeds))
    begin, degree = indptr[seeds], indptr[seeds + 1] - indptr[seeds]
    if fanout is None:
        count = degree
        drawn = np.zeros(seeds.size, bool)
    elif replace:
        count = np.where(degree > 0, fanout, 0)
        drawn = degree > 0
    else:
        count = np.minimum(degree, fanout)
        drawn = degree > fanout
    s_indptr = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    total = int(s_indptr[-1])
    owner = np.repeat(np.arange(seeds.size), count)
    entries = begin[owner] + (np.arange(total) - s_indptr[owner])          # the copied rows; the drawn ones are overwritten
    if drawn.any():
        picker = replace_positions if replace else floyd_positions
        positions = picker(seeds[drawn], degree[drawn], fanout, seed, offset)
        entries[s_indptr[:-1][drawn][:, None] + np.arange(fanout)[None, :]] = begin[drawn][:, None] + positions
    return s_indptr.astype(np.int32), indices[entries].astype(np.int32), entries.astype(np.int32)


def compact_block(seeds, s_indices):
    """``(src_ids, local_indices)`` as int32 arrays: the seeds in the given order, then the other sampled columns ascending."""
    seeds, s_indices = np.asarray(seeds, dtype=np.int64), np.asarray(s_indices, dtype=np.int64)
    assert np.unique(seeds).size == seeds.size
    src_ids = np.concatenate([seeds, np.setdiff1d(np.unique(s_indices), seeds)])
    where = {int(c): i for i, c in enumerate(src_ids)}
    local = np.array([where[int(c)] for c in s_indices], np.int64)
    return src_ids.astype(np.int32), local.astype(np.int32)


def sample_blocks(indptr, indices, seeds, fanouts, seed, offset=0, replace=False):
    """The blocks of voltrix.sample_blocks as dicts of int32 arrays, input layer first: layer l from the output samples with offset + l."""
    blocks, dst_ids = [], np.asarray(seeds, dtype=np.int64)
    for layer, fanout in enumerate(reversed(list(fanouts))):
        s_indptr, s_indices, entries = sample_neighbors(indptr, indices, dst_ids, fanout, seed, (offset + layer) % 2 ** 64, replace)
        src_ids, local = compact_block(dst_ids, s_indices)
        blocks.append({"indptr": s_indptr, "indices": local, "s_indices": s_indices, "entries": entries, "src_ids": src_ids,
                       "dst_ids": dst_ids.astype(np.int32), "num_dst": dst_ids.size, "num_src": src_ids.size})
        dst_ids = src_ids.astype(np.int64)
    return blocks[::-1]
