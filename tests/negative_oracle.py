"""A numpy restatement of the negative-sampling rule and of the entry -> endpoints search (voltrix/negative_sample_kernels.hpp,
voltrix/negative.py), for the tests that hold the kernels to them.  Philox4x32-10 is the restatement of
tests/test_attn_dropout_host.py; everything here is vectorised over slots and works on host arrays only.

    draw(p, q)   = word q & 3 of Philox((p, (q >> 2) | 0x40000000, offset lo, offset hi), (seed lo, seed hi)); p the POSITION in src
    slot (p, j)  : for t = 0 .. T - 1, c = (draw(p, j T + t) * num_cols) >> 32; rejected if c occurs in row src[p] (or, with
                   exclude_self, c == src[p]); the first accepted c, or -1 after T rejections
    entry e      : the row r with indptr[r] <= e < indptr[r + 1] and the column indices[e]; (-1, -1) outside [0, nnz)

Membership is decided on a sorted key set of the graph's entries, not by a search in the row: it does not care whether rows are sorted.
"""
import numpy as np

from test_attn_dropout_host import philox4x32_10

COUNTER_BITS = 0x40000000


def draws(positions, first, count, seed, offset):
    """uint64 [len(positions), count]: draw(p, q) for every p in ``positions`` and q = first .. first + count - 1."""
    positions = np.asarray(positions, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    q = np.arange(first, first + count, dtype=np.uint64)
    words = np.stack(philox4x32_10(positions[:, None], (q >> np.uint64(2)) | np.uint64(COUNTER_BITS), offset & 0xFFFFFFFF, offset >> 32,
                                   seed & 0xFFFFFFFF, seed >> 32), -1)                       # [positions, count, 4]
    pick = np.broadcast_to((q & np.uint64(3)).astype(np.int64)[None, :, None], words.shape[:2] + (1,))
    return np.take_along_axis(words, pick, -1)[..., 0].astype(np.uint64)


def _keys(indptr, indices, num_cols):
    """The sorted distinct keys row * num_cols + col of every entry whose column is in [0, num_cols)."""
    rows = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))
    inside = (indices >= 0) & (indices < num_cols)
    return np.unique(rows[inside] * num_cols + indices[inside])


def negative_sample(indptr, indices, src, k, seed, offset=0, num_cols=None, max_tries=16, exclude_self=False):
    """``(neg int32 [S, k], num_exhausted)``: what voltrix.negative_sample returns for in-range sources (a source outside
    [0, num_rows) has no neighbours here, as inside the kernel)."""
    indptr, indices, src = (np.asarray(v, dtype=np.int64) for v in (indptr, indices, src))
    num_rows = indptr.size - 1
    num_cols = num_rows if num_cols is None else int(num_cols)
    count, tries = src.size, int(max_tries)
    neg = np.full((count, k), -1, np.int64)
    if count == 0 or num_cols == 0:
        return neg.astype(np.int32), int(neg.size)
    keys = _keys(indptr, indices, num_cols)
    known = (src >= 0) & (src < num_rows)
    x = draws(np.arange(count), 0, k * tries, seed, offset).reshape(count, k, tries)
    cand = ((x * np.uint64(num_cols)) >> np.uint64(32)).astype(np.int64)                     # [S, k, T]
    key = src[:, None, None] * num_cols + cand
    at = np.minimum(np.searchsorted(keys, key), max(keys.size - 1, 0))
    rejected = (keys[at] == key) & known[:, None, None] if keys.size else np.zeros(cand.shape, bool)
    if exclude_self:
        rejected |= cand == src[:, None, None]
    accepted = ~rejected
    first = accepted.argmax(2)                                                               # the first accepted try, 0 where none
    chosen = np.take_along_axis(cand, first[..., None], 2)[..., 0]
    neg = np.where(accepted.any(2), chosen, -1)
    return neg.astype(np.int32), int((neg < 0).sum())


def edge_endpoints(indptr, indices, entries):
    """``(rows, cols)`` as int32 arrays: what voltrix.edge_endpoints computes; (-1, -1) for an id outside [0, nnz)."""
    indptr, indices, entries = (np.asarray(v, dtype=np.int64) for v in (indptr, indices, entries))
    inside = (entries >= 0) & (entries < indices.size)
    rows = np.searchsorted(indptr, entries, side="right") - 1
    cols = indices[np.where(inside, entries, 0)] if indices.size else np.full(entries.shape, -1, np.int64)
    return np.where(inside, rows, -1).astype(np.int32), np.where(inside, cols, -1).astype(np.int32)


def edge_batch(indptr, indices, entries, num_negatives, seed, offset=0, max_tries=16, exclude_self=True):
    """The parts of voltrix.sample_edge_batch that do not come from sample_blocks, as a dict of arrays: node_ids (ascending), the
    pairs CSR on local ids (the positive destination first, then the non-exhausted negatives in slot order), labels, src_local."""
    rows, cols = edge_endpoints(indptr, indices, entries)
    neg, exhausted = negative_sample(indptr, indices, rows, num_negatives, seed, offset, None, max_tries, exclude_self)
    everything = np.concatenate([rows, cols, neg.ravel()])
    node_ids = np.unique(everything[everything >= 0])
    cand = np.concatenate([cols[:, None], neg], 1)
    keep = cand >= 0
    p_indptr = np.concatenate([[0], np.cumsum(keep.sum(1))])
    labels = np.zeros(p_indptr[-1], np.float32)
    labels[p_indptr[:-1]] = 1.0
    return {"node_ids": node_ids.astype(np.int32), "indptr": p_indptr.astype(np.int32),
            "indices": np.searchsorted(node_ids, cand[keep]).astype(np.int32), "globals": cand[keep].astype(np.int32), "labels": labels,
            "src_local": np.searchsorted(node_ids, rows).astype(np.int32), "src": rows, "dst": cols, "neg": neg,
            "num_exhausted": exhausted}
