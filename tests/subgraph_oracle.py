"""A numpy restatement of the induced-subgraph contract and of the walk rule (voltrix/induced_subgraph_kernels.hpp, voltrix/subgraph.py,
DESIGN.md 3.24), for the tests that hold the kernels to them.  Philox4x32-10 is the restatement of tests/test_attn_dropout_host.py;
everything here is vectorised and works on host arrays only.

    subgraph_csr:  row i = the entries of row rows[i] whose column is in cols, in CSR order; s_local = the column's position in cols,
                   s_entries = the entry's index in indices; columns outside [0, num_cols) are never selected
    draw(w, t)   = word t & 3 of Philox((w, (t >> 2) | 0xC0000000, offset lo, offset hi), (seed lo, seed hi))
    step t:        d = degree of the node v the walker stands on; d == 0 (or v outside [0, num_rows)): -1 from here on; else the
                   entry at position (draw(w, t) * d) >> 32 of row v, and on to its column
"""
import numpy as np

from test_attn_dropout_host import philox4x32_10

COUNTER_BITS = 0xC0000000


def subgraph_csr(indptr, indices, rows, cols=None, num_cols=None):
    """``(s_indptr, s_local, s_entries)`` as int32 arrays: what voltrix.subgraph_csr returns for in-range rows and distinct cols."""
    indptr, indices, rows = (np.asarray(v, dtype=np.int64) for v in (indptr, indices, rows))
    cols = rows if cols is None else np.asarray(cols, dtype=np.int64)
    num_cols = indptr.size - 1 if num_cols is None else num_cols
    assert np.unique(cols).size == cols.size and (cols.size == 0 or (cols.min() >= 0 and cols.max() < num_cols))
    local_of = np.full(num_cols + 1, -1, np.int64)                     # the last slot: every column outside [0, num_cols)
    local_of[cols] = np.arange(cols.size)
    begin, degree = indptr[rows], indptr[rows + 1] - indptr[rows]
    starts = np.concatenate([[0], np.cumsum(degree)])
    owner = np.repeat(np.arange(rows.size), degree)
    entries = begin[owner] + (np.arange(starts[-1]) - starts[owner])   # every entry of every selected row, in order
    column = indices[entries]
    local = local_of[np.where((column >= 0) & (column < num_cols), column, num_cols)]
    keep = local >= 0
    s_indptr = np.concatenate([[0], np.cumsum(np.bincount(owner[keep], minlength=rows.size))])
    return s_indptr.astype(np.int32), local[keep].astype(np.int32), entries[keep].astype(np.int32)


def walk_draws(walkers, steps, seed, offset):
    """uint64 [len(walkers), steps]: draw(w, t) for every walker index in ``walkers`` and t < steps."""
    walkers = np.asarray(walkers, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    t = np.arange(steps, dtype=np.uint64)
    words = np.stack(philox4x32_10(walkers[:, None], (t >> np.uint64(2)) | np.uint64(COUNTER_BITS), offset & 0xFFFFFFFF, offset >> 32,
                                   seed & 0xFFFFFFFF, seed >> 32), -1)                       # [walkers, steps, 4]
    pick = np.broadcast_to((t & np.uint64(3)).astype(np.int64)[None, :, None], words.shape[:2] + (1,))
    return np.take_along_axis(words, pick, -1)[..., 0].astype(np.uint64)


def random_walk(indptr, indices, starts, length, seed, offset=0):
    """``(nodes [W, length + 1], entries [W, length])`` as int32 arrays: what voltrix.random_walk returns."""
    indptr, indices, starts = (np.asarray(v, dtype=np.int64) for v in (indptr, indices, starts))
    num_rows, count = indptr.size - 1, starts.size
    nodes = np.full((count, length + 1), -1, np.int64)
    entries = np.full((count, length), -1, np.int64)
    nodes[:, 0] = starts
    x = walk_draws(np.arange(count), length, seed, offset)
    for t in range(length):
        v = nodes[:, t]
        inside = (v >= 0) & (v < num_rows)
        at = np.where(inside, v, 0)
        degree = np.where(inside, indptr[at + 1] - indptr[at], 0)
        alive = degree > 0
        position = ((x[:, t] * degree.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
        entry = np.where(alive, indptr[at] + position, 0)
        entries[:, t] = np.where(alive, entry, -1)
        nodes[:, t + 1] = np.where(alive, indices[entry] if indices.size else -1, -1)
    return nodes.astype(np.int32), entries.astype(np.int32)


def induced_subgraph(indptr, indices, nodes):
    """voltrix.induced_subgraph as a dict of int32 arrays."""
    s_indptr, s_local, entries = subgraph_csr(indptr, indices, nodes)
    return {"indptr": s_indptr, "indices": s_local, "entries": entries, "node_ids": np.asarray(nodes, dtype=np.int32),
            "num_nodes": len(nodes)}


def sample_subgraph_rw(indptr, indices, roots, length, seed, offset=0):
    """voltrix.sample_subgraph_rw composed from its parts: the distinct visited nodes in ascending id, then the induced subgraph."""
    nodes, _ = random_walk(indptr, indices, roots, length, seed, offset)
    visited = np.unique(nodes[(nodes >= 0) & (nodes < len(indptr) - 1)])
    return induced_subgraph(indptr, indices, visited)
