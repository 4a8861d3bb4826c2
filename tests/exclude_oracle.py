"""A numpy restatement of the exclusion rule (voltrix/neighbor_sample_kernels.hpp, voltrix/sampling.py) and of
the (row, column) -> entry lookup, for the tests that hold the kernels to them.  The draws, Floyd's algorithm and the replacement rule
are tests/sample_oracle.py's, unchanged: only the degree they see (d' = d - x) and the mapping of their positions (cand) are new.

    exclude    CSR entry ids, strictly ascending
    row r      lo = lower_bound(exclude, begin), hi = lower_bound(exclude, end), x = hi - lo, q_i = exclude[lo + i] - begin
    cand(t)    t + #{ i : q_i - i <= t }: the position of candidate number t among the d' = d - x positions that are not excluded
    the rule   sample_oracle's with d' in place of d, every position mapped through cand
"""
import numpy as np

import sample_oracle


def cand(excluded, t):
    """The position of candidate number ``t`` in a row whose excluded positions are ``excluded`` (ascending, distinct): written from the
    formula, ``t + #{i : q_i - i <= t}``."""
    q = np.asarray(excluded, dtype=np.int64)
    return int(t) + int((q - np.arange(q.size) <= t).sum())


def candidates(degree, excluded):
    """The positions of a row of ``degree`` entries that are not excluded, in CSR order: written from the DEFINITION (a set difference),
    not from the formula -- ``cand(excluded, t) == candidates(degree, excluded)[t]`` is what the exhaustive test asserts."""
    return np.setdiff1d(np.arange(degree, dtype=np.int64), np.asarray(excluded, dtype=np.int64))


def row_slices(indptr, exclude, rows):
    """``(lo, x)`` for every row id in ``rows``: the row's slice ``exclude[lo : lo + x]``."""
    indptr, exclude, rows = (np.asarray(v, dtype=np.int64) for v in (indptr, exclude, rows))
    lo = np.searchsorted(exclude, indptr[rows], side="left")
    return lo, np.searchsorted(exclude, indptr[rows + 1], side="left") - lo


def sample_neighbors(indptr, indices, seeds, fanout, seed, offset=0, replace=False, exclude=()):
    """``(s_indptr, s_indices, s_entries)`` as int32 arrays: what voltrix.sample_neighbors(..., exclude=) returns for in-range seeds."""
    indptr, indices, seeds = (np.asarray(v, dtype=np.int64) for v in (indptr, indices, seeds))
    exclude = np.asarray(exclude, dtype=np.int64)
    assert (np.diff(exclude) > 0).all() and (exclude.size == 0 or (exclude[0] >= 0 and exclude[-1] < indices.size))
    lo, held = row_slices(indptr, exclude, seeds)
    begin, degree = indptr[seeds], indptr[seeds + 1] - indptr[seeds] - held                  # d'
    assert (degree >= 0).all()
    rows, counts = [], []
    for i, r in enumerate(seeds):
        open_positions = candidates(indptr[r + 1] - indptr[r], exclude[lo[i]:lo[i] + held[i]] - begin[i])
        assert open_positions.size == degree[i]
        if fanout is None or (not replace and degree[i] <= fanout):
            picked = np.arange(degree[i])
        elif degree[i] == 0:
            picked = np.zeros(0, np.int64)
        elif replace:
            picked = sample_oracle.replace_positions([r], [degree[i]], fanout, seed, offset)[0]
        else:
            picked = sample_oracle.floyd_positions([r], [degree[i]], fanout, seed, offset)[0]
        rows.append(begin[i] + open_positions[picked])
        counts.append(len(picked))
    s_indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    entries = np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int64)
    return s_indptr, indices[entries].astype(np.int32), entries.astype(np.int32)


def find_edges(indptr, indices, rows, cols):
    """int32 [Q]: the id of the first entry of row ``rows[i]`` whose column is ``cols[i]``; -1 if there is none or the row is outside
    ``[0, num_rows)``.  A scan, whatever the order of the row."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    out = np.full(len(rows), -1, np.int32)
    for i, (r, c) in enumerate(zip(rows, cols)):
        if 0 <= r < indptr.size - 1:
            hits = np.flatnonzero(indices[indptr[r]:indptr[r + 1]] == c)
            if hits.size:
                out[i] = indptr[r] + hits[0]
    return out


def sample_blocks(indptr, indices, seeds, fanouts, seed, offset=0, replace=False, exclude=()):
    """tests/sample_oracle.py's ``sample_blocks`` with ``exclude`` left out of every layer."""
    blocks, dst_ids = [], np.asarray(seeds, dtype=np.int64)
    for layer, fanout in enumerate(reversed(list(fanouts))):
        s_indptr, s_indices, entries = sample_neighbors(indptr, indices, dst_ids, fanout, seed, (offset + layer) % 2 ** 64, replace, exclude)
        src_ids, local = sample_oracle.compact_block(dst_ids, s_indices)
        blocks.append({"indptr": s_indptr, "indices": local, "s_indices": s_indices, "entries": entries, "src_ids": src_ids,
                       "dst_ids": dst_ids.astype(np.int32), "num_dst": dst_ids.size, "num_src": src_ids.size})
        dst_ids = src_ids.astype(np.int64)
    return blocks[::-1]
