"""numpy float64 oracle of ``voltrix.spmm_rel`` and of both its gradients, from the inputs as they are given (the callers convert the
stored fp32 / fp16 / bf16 values to float64 exactly).  None of this is the code under test: the per-entry terms, then float64 sums
over the segments of the entry array (``np.add.reduceat``; for columns and types after a stable sort).

    forward(indptr, indices, etype, feat, coef, weight=None)                 -> (out [n, B, F], mass [n, B, F], count [n])
    grad_feat(indptr, indices, etype, grad_out, coef, num_cols, weight=None) -> (dF [num_cols, F], mass, count [num_cols])
    contract(t_indptr, t_indices, t_order, etype, grad_out, coef, weight)    -> the same, on a transposed CSR through ``t_order``
    grad_coef(indptr, indices, etype, grad_out, feat, num_types, weight=None)-> (dC [R, B], mass [R, B], count [R])
    type_norm(indptr, etype)                                                 -> [nnz]
    transpose(indptr, indices, num_cols)                                     -> (t_indptr, t_indices, t_order)

``mass`` is the sum of the absolute terms of an element (for ``grad_coef``: ``sum_e |w_e| sum_f |g x|``) and ``count`` the number of
entries behind it: the bounds of the fp32 sums are ``(count + 2) 2^-23 mass`` (forward), ``(count B + 2)`` (grad_feat) and
``(count + F + 2)`` (grad_coef).
"""
import numpy as np


def entry_rows(indptr):
    indptr = np.asarray(indptr, np.int64)
    return np.repeat(np.arange(len(indptr) - 1), indptr[1:] - indptr[:-1])


def segment_sum(values, ptr):
    """[len(ptr) - 1, ...]: the sums of ``values[ptr[i]:ptr[i + 1]]``, 0 for an empty segment."""
    ptr = np.asarray(ptr, np.int64)
    out = np.zeros((len(ptr) - 1,) + values.shape[1:])
    nonempty = ptr[1:] > ptr[:-1]
    if nonempty.any():
        with np.errstate(invalid="ignore"):
            out[nonempty] = np.add.reduceat(values, ptr[:-1][nonempty], axis=0)
    return out


def _coefficients(etype, coef, weight):
    """c[e, b] = w_e * coef[etype_e, b] in float64."""
    c = np.asarray(coef, np.float64)[np.asarray(etype, np.int64)]
    return c if weight is None else c * np.asarray(weight, np.float64)[:, None]


def forward(indptr, indices, etype, feat, coef, weight=None):
    rows = entry_rows(indptr)
    x = np.asarray(feat, np.float64)[np.asarray(indices, np.int64)]                  # [nnz, F]
    with np.errstate(invalid="ignore", over="ignore"):
        terms = _coefficients(etype, coef, weight)[:, :, None] * x[:, None, :]       # [nnz, B, F]
    return segment_sum(terms, indptr), segment_sum(np.abs(terms), indptr), np.bincount(rows, minlength=len(indptr) - 1).astype(np.float64)


def _by_key(values, absolute, keys, num_keys):
    order = np.argsort(keys, kind="stable")
    count = np.bincount(keys, minlength=num_keys)
    ptr = np.concatenate([[0], np.cumsum(count)])
    return segment_sum(values[order], ptr), segment_sum(absolute[order], ptr), count.astype(np.float64)


def grad_feat(indptr, indices, etype, grad_out, coef, num_cols, weight=None):
    """By the definition, a scatter over the entries of the CSR itself (no transpose is built here)."""
    rows = entry_rows(indptr)
    c = _coefficients(etype, coef, weight)
    g = np.asarray(grad_out, np.float64)[rows]                                       # [nnz, B, F]
    with np.errstate(invalid="ignore", over="ignore"):
        terms = c[:, :, None] * g
    return _by_key(terms.sum(1), np.abs(terms).sum(1), np.asarray(indices, np.int64), num_cols)


def contract(t_indptr, t_indices, t_order, etype, grad_out, coef, weight=None):
    """What the kernel runs: on the transposed CSR, ``etype`` and ``weight`` (CSR entry order) read through ``t_order``."""
    order = np.asarray(t_order, np.int64)
    c = _coefficients(np.asarray(etype)[order], coef, None if weight is None else np.asarray(weight)[order])
    g = np.asarray(grad_out, np.float64)[np.asarray(t_indices, np.int64)]
    terms = c[:, :, None] * g
    rows = entry_rows(t_indptr)
    return segment_sum(terms.sum(1), t_indptr), segment_sum(np.abs(terms).sum(1), t_indptr), \
        np.bincount(rows, minlength=len(t_indptr) - 1).astype(np.float64)


def grad_coef(indptr, indices, etype, grad_out, feat, num_types, weight=None):
    rows = entry_rows(indptr)
    x = np.asarray(feat, np.float64)[np.asarray(indices, np.int64)]
    g = np.asarray(grad_out, np.float64)[rows]
    w = np.ones(len(rows)) if weight is None else np.asarray(weight, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        products = g * x[:, None, :]                                                 # [nnz, B, F]
        dots, masses = w[:, None] * products.sum(2), np.abs(w)[:, None] * np.abs(products).sum(2)
    return _by_key(dots, masses, np.asarray(etype, np.int64), num_types)


def type_norm(indptr, etype):
    rows, etype = entry_rows(indptr), np.asarray(etype, np.int64)
    return np.array([1.0 / np.sum((rows == r) & (etype == t)) for r, t in zip(rows, etype)])


def transpose(indptr, indices, num_cols):
    """(t_indptr, t_indices, t_order) by a stable sort by column: entry ``e`` of the transpose is entry ``t_order[e]`` of the CSR."""
    rows = entry_rows(indptr)
    cols = np.asarray(indices, np.int64)
    order = np.argsort(cols, kind="stable")
    t_indptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=num_cols))])
    return t_indptr.astype(np.int32), rows[order].astype(np.int32), order.astype(np.int32)
