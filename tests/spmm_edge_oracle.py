"""numpy float64 oracle of ``voltrix.spmm_edge`` and of both its gradients, from the inputs as they are given (the callers convert the
stored fp32 / fp16 / bf16 values to float64 exactly).  None of this is the code under test: the per-entry terms, then float64 sums
over the segments of the entry array (``np.add.reduceat``; for the columns after a stable sort by column).

    forward(indptr, indices, feat, efeat, op, order=None, self_rows=None) -> (out [num_rows, F], mass [num_rows, F], count [num_rows])
    grad_efeat(indptr, indices, grad_out, feat, efeat, op)                -> [nnz, F]
    grad_feat(indptr, indices, grad_out, feat, efeat, op, num_cols)       -> (d_feat [num_cols, F], mass, count [num_cols])

``mass`` is the sum of the absolute terms of an element and ``count`` the number of its terms: the error bound of the fp32 sums is
``(count + 1) 2^-23 mass``.  ``order``: entry ``e`` reads ``efeat[order[e]]`` (the backward on the transposed CSR); ``self_rows``: the
gate's per-row operand.  A closed gate passes nothing (``np.where``, not a product with 0).
"""
import numpy as np

OPS = ("mul", "add", "add_relu", "copy", "gate")


def entry_rows(indptr):
    indptr = np.asarray(indptr, np.int64)
    return np.repeat(np.arange(len(indptr) - 1), indptr[1:] - indptr[:-1])


def segment_sum(values, ptr):
    """[len(ptr) - 1, F]: the sums of ``values[ptr[i]:ptr[i + 1]]``, 0 for an empty segment."""
    ptr = np.asarray(ptr, np.int64)
    out = np.zeros((len(ptr) - 1, values.shape[1]))
    nonempty = ptr[1:] > ptr[:-1]
    if nonempty.any():
        with np.errstate(invalid="ignore"):
            out[nonempty] = np.add.reduceat(values, ptr[:-1][nonempty], axis=0)
    return out


def messages(x, w, op, own=None):
    """The per-entry terms [nnz, F] in float64.  add_relu is ``torch.relu``'s: a NaN stays a NaN."""
    if op == "mul":
        return x * w
    if op == "add":
        return x + w
    if op == "add_relu":
        s = x + w
        return np.where(s < 0, 0.0, s)
    if op == "copy":
        return w + 0.0
    assert op == "gate"
    return np.where(own + w > 0, x, 0.0)


def forward(indptr, indices, feat, efeat, op, order=None, self_rows=None):
    assert op in OPS
    rows = entry_rows(indptr)
    num_rows = len(indptr) - 1
    efeat = np.asarray(efeat, np.float64)
    w = efeat if order is None else efeat[np.asarray(order, np.int64)]
    w = w.reshape(len(rows), -1)
    x = None if op == "copy" else np.asarray(feat, np.float64).reshape(len(feat), -1)[np.asarray(indices, np.int64)]
    own = None if op != "gate" else np.asarray(self_rows, np.float64).reshape(num_rows, -1)[rows]
    with np.errstate(invalid="ignore", over="ignore"):
        terms = messages(x, w, op, own)
    return segment_sum(terms, indptr), segment_sum(np.abs(terms), indptr), np.bincount(rows, minlength=num_rows).astype(np.float64)


def grad_efeat(indptr, indices, grad_out, feat, efeat, op):
    assert op in ("mul", "add", "add_relu", "copy")
    rows = entry_rows(indptr)
    g = np.asarray(grad_out, np.float64).reshape(len(indptr) - 1, -1)[rows]
    if op in ("add", "copy"):
        return g
    x = np.asarray(feat, np.float64).reshape(len(feat), -1)[np.asarray(indices, np.int64)]
    if op == "mul":
        return g * x
    w = np.asarray(efeat, np.float64).reshape(len(rows), -1)
    return np.where(x + w > 0, g, 0.0)


def grad_feat(indptr, indices, grad_out, feat, efeat, op, num_cols):
    """By the definition, a scatter over the entries of the CSR itself (no transpose is built here)."""
    assert op in ("mul", "add", "add_relu")
    rows = entry_rows(indptr)
    cols = np.asarray(indices, np.int64)
    g = np.asarray(grad_out, np.float64).reshape(len(indptr) - 1, -1)[rows]
    if op == "add":
        terms = g
    else:
        w = np.asarray(efeat, np.float64).reshape(len(rows), -1)
        if op == "mul":
            terms = g * w
        else:
            x = np.asarray(feat, np.float64).reshape(num_cols, -1)[cols]
            terms = np.where(x + w > 0, g, 0.0)
    by_col = np.argsort(cols, kind="stable")
    count = np.bincount(cols, minlength=num_cols)
    ptr = np.concatenate([[0], np.cumsum(count)])
    return segment_sum(terms[by_col], ptr), segment_sum(np.abs(terms)[by_col], ptr), count.astype(np.float64)


def transpose(indptr, indices, num_cols):
    """(t_indptr, t_indices, t_order) by a stable sort by column: entry ``e`` of the transpose is entry ``t_order[e]`` of the CSR."""
    rows = entry_rows(indptr)
    cols = np.asarray(indices, np.int64)
    order = np.argsort(cols, kind="stable")
    t_indptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=num_cols))])
    return t_indptr.astype(np.int32), rows[order].astype(np.int32), order.astype(np.int32)
