"""Several neighbour aggregates from ONE gather of a CSR pattern: ``out[r, a] = aggrs[a] over the entries e of row r of
feat[indices[e]]`` per element, for any subset of ``sum``, ``mean``, ``max``, ``min``, ``var``, ``std`` -- what a PNA layer (PyG's
``MultiAggregation``, DGL's ``PNAConv``) asks of its ``(mean, max, min, std)`` towers, which ``voltrix.spmm_reduce`` serves with one
gather per aggregator and without a second moment.

No reference counterpart.  One HIP launch straight from the CSR (voltrix/spmm_multi_kernels.hpp); every accumulator stays in registers:

    out = voltrix.spmm_multi(indptr, indices, feat, num_rows, aggrs=("mean", "max", "min", "std"))      # float32 [n, 4, F]
    out, state = voltrix.spmm_multi(..., return_state=True)                                             # what the backward needs
    d_feat = spmm_multi.backward(t_indptr, t_indices, t_order, num_cols, feat=feat, u=..., w=..., mean=state.mean,
                                 g_max=..., argmax=state.argmax, g_min=..., argmin=state.argmin)

``out.view(n, A * F) @ W`` is the layer (the convention of ``spmm_rel``'s ``[n, B, F]``).  ``sum`` has the bits of the CSR row-gather
sum, ``mean`` / ``max`` / ``min`` and the args those of ``voltrix.spmm_reduce`` (the first entry in CSR order wins ties, a NaN wins and
stays, the args are CSR ENTRY ids).  ``var = max(S2 / d - (S1 / d)^2, 0)`` comes from moments SHIFTED by the row's first entry
(``y_e = x_e - x_first``, ``S1 = sum y_e``, ``S2 = sum y_e^2``), never from ``sum x^2``, which cancels on features with a mean:
``|var - ref| <= (d + 4) 2^-23 (2 / d) sum_e (x_e - x_first)^2``; a row of one entry gives ``0`` exactly, a row that holds a NaN or
an infinity gives NaN.  ``std = sqrt(var + eps)``.  A row WITHOUT entries gives ``0`` in every aggregate -- ``std`` included, where
PyG gives ``sqrt(eps)`` -- and ``-1`` in the args: the zeros every other operator here writes.  An aggregate's bits do not depend on
which others are asked for.  No float atomics, the same bits on every call.  Known limit: a hub row (forward) or hub column
(backward) serialises its wave, like ``voltrix.spmm_reduce``.  DESIGN.md 3.31.
"""
from __future__ import annotations

import collections
import math

import torch

from .utils import FEATURE_TYPES, padded_last_dim, piece_width

AGGREGATES = ("sum", "mean", "max", "min", "var", "std")
PNA_AGGREGATES = ("mean", "max", "min", "std")

# what ``return_state`` hands out: int32 ``argmax`` / ``argmin`` and float32 ``mean`` / ``std``, each ``[num_rows, *tail]`` or None where
# the backward of the requested aggregates does not need it.  ``mean`` / ``std`` are views of ``out`` where they are among ``aggrs``.
MultiState = collections.namedtuple("MultiState", ("argmax", "argmin", "mean", "std"))


def check_aggrs(who: str, aggrs, eps) -> tuple:
    """``aggrs`` as a tuple: a non-empty sequence without repeats from ``AGGREGATES``; ``eps`` finite and > 0.  Else ``ValueError``."""
    if isinstance(aggrs, str) or not isinstance(aggrs, (tuple, list)):
        raise ValueError(f"{who}: aggrs must be a sequence of names from {AGGREGATES}, got {aggrs!r}")
    aggrs = tuple(aggrs)
    if not aggrs or any(not isinstance(a, str) or a not in AGGREGATES for a in aggrs) or len(set(aggrs)) != len(aggrs):
        raise ValueError(f"{who}: aggrs must be a non-empty sequence without repeats from {AGGREGATES}, got {aggrs!r}")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not math.isfinite(eps) or not eps > 0:
        raise ValueError(f"{who}: eps must be a finite number > 0, got {eps!r}")
    return aggrs


def spmm_multi(indptr: torch.Tensor, indices: torch.Tensor, feat: torch.Tensor, num_rows: int, aggrs=PNA_AGGREGATES,
               eps: float = 1e-5, return_state: bool = False):
    """Every aggregate of ``aggrs`` over every row's entries of ``feat[indices[e]]`` -> float32 ``[num_rows, len(aggrs),
    *feat.shape[1:]]`` in the order of ``aggrs``, every element written, one launch on the current stream.  With ``return_state`` also
    a ``MultiState``: ``argmax`` / ``argmin`` (int32 ``[num_rows, *tail]``, the CSR entry id of the winner, ``-1`` for a row without
    entries; where max / min is asked for) and ``mean`` / ``std`` (where var / std is asked for: what their gradient needs).

    ``indptr`` / ``indices``: device int32 CSR with ``num_rows`` rows (rectangular patterns and duplicates allowed); ``feat``
    [num_cols, ...] fp32 / fp16 / bf16 as it is (other types as fp32), trailing dimensions flattened.  A row width that is not a
    multiple of 16 bytes is padded with zeros (the padded columns are sliced away); an operand that is contiguous and 16-byte aligned is
    never copied.  A row without entries gives 0 everywhere (PyG's std would be ``sqrt(eps)``).  ``aggrs`` must be a non-empty sequence
    without repeats from ``("sum", "mean", "max", "min", "var", "std")`` and ``eps`` finite and > 0, else ``ValueError``."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    aggrs = check_aggrs("spmm_multi", aggrs, eps)
    assert indptr.is_cuda and indices.is_cuda and indptr.dtype == torch.int32 and indices.dtype == torch.int32
    assert indptr.numel() == num_rows + 1 and feat.is_cuda and feat.dim() >= 2, tuple(feat.shape)
    if feat.dtype not in FEATURE_TYPES:
        feat = feat.float()
    tail = tuple(feat.shape[1:])
    feat = feat.flatten(1)
    dim = feat.shape[1]
    width = piece_width(max(dim, 1), feat.dtype)
    slots = {name: i for i, name in enumerate(aggrs)}
    visible = len(aggrs)
    moments = "var" in slots or "std" in slots
    if return_state and moments:                 # the gradient of var / std needs the mean, that of std the std: hidden slots
        slots.setdefault("mean", len(slots))
        if "std" in aggrs:
            slots.setdefault("std", len(slots))
    out = torch.empty((num_rows, len(slots), width), dtype=torch.float32, device=feat.device)
    argmax = argmin = None
    if return_state and "max" in slots:
        argmax = torch.empty((num_rows, width), dtype=torch.int32, device=feat.device)
    if return_state and "min" in slots:
        argmin = torch.empty((num_rows, width), dtype=torch.int32, device=feat.device)
    if num_rows > 0 and dim > 0:
        feat = padded_last_dim(feat, width)
        num_entries = indices.numel()
        if num_entries == 0:          # nothing is gathered; the entry point still wants pointers it could read
            indices = indptr
            if feat.shape[0] == 0:
                feat = torch.zeros((1, width), dtype=feat.dtype, device=feat.device)
        capi.launch_spmm_multi(indptr.contiguous(), indices.contiguous(), num_rows, feat, slots, eps, out, argmax, argmin,
                               _raw_stream(feat.device), num_entries)

    def shaped(t):                    # [num_rows, width] (maybe a slot of `out`) -> [num_rows, *tail]
        if t is None:
            return None
        if width != dim:
            t = t[:, :dim].contiguous()
        return t.view((num_rows,) + tail) if t.is_contiguous() else t.unflatten(1, tail)

    state = None
    if return_state:
        state = MultiState(shaped(argmax), shaped(argmin), shaped(out[:, slots["mean"]]) if moments else None,
                           shaped(out[:, slots["std"]]) if "std" in aggrs else None)
    if visible != len(slots) or width != dim:
        out = out[:, :visible, :dim].contiguous()
    out = out.view((num_rows, visible) + tail)
    return (out, state) if return_state else out


def spmm_multi_backward(t_indptr: torch.Tensor, t_indices: torch.Tensor, t_order: torch.Tensor, num_cols: int, feat=None, u=None,
                        w=None, mean=None, g_max=None, argmax=None, g_min=None, argmin=None) -> torch.Tensor:
    """The gradient of ``spmm_multi`` for ``feat`` in one launch: ``d_feat[c] = sum over the entries e of column c of u[r] + w[r]
    (feat[c] - mean[r]) + [argmax[r] == e] g_max[r] + [argmin[r] == e] g_min[r]`` (``r`` the entry's row) -> float32 ``[num_cols,
    *tail]``, every row written, columns without entries zero.  The caller forms ``u = g_sum + g_mean / d`` and ``w = 2 g_var / d +
    g_std / (d std)`` with ``d`` the row's entry count (``spmm_reduce.row_degrees``).  Each group -- ``u``; ``w`` with ``feat`` and
    ``mean``; ``g_max`` with ``argmax``; ``g_min`` with ``argmin`` -- is given or None, at least one is; all ``[num_rows, *tail]``
    (``feat`` ``[num_cols, *tail]``, read as fp32: a 16-bit ``feat`` is cast once).  ``t_indptr`` / ``t_indices``: the transposed
    device CSR; ``t_order``: the entry of the CSR that entry ``e`` of the transpose is.  The centred form ``w (x - mean)`` per entry
    does not cancel on features with a mean.  A gather in the transposed CSR's order: no float atomics, the same bits on every call."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    given = [t for t in (u, w, g_max, g_min) if t is not None]
    if not given or (w is None) != (feat is None) or (w is None) != (mean is None) or (g_max is None) != (argmax is None) or \
            (g_min is None) != (argmin is None):
        raise ValueError("spmm_multi.backward: give u, (w, feat, mean), (g_max, argmax), (g_min, argmin) as whole groups, one at least")
    assert t_indptr.is_cuda and t_indices.is_cuda and t_indptr.dtype == torch.int32 and t_indices.dtype == torch.int32
    assert t_indptr.numel() == num_cols + 1 and t_order.is_cuda and t_order.numel() == t_indices.numel()
    t_order = t_order.to(torch.int32).contiguous()
    tail = tuple(given[0].shape[1:])
    dim = given[0].flatten(1).shape[1]
    width = (max(dim, 1) + 3) // 4 * 4

    def dense(t, dtype):              # [rows, width] of `dtype`, contiguous and aligned; padding columns only feed sliced-away output
        if t is None:
            return None
        t = t.flatten(1) if t.dim() != 2 else t
        assert t.is_cuda and t.shape[1] == dim, (tuple(t.shape), dim)
        return padded_last_dim(t.to(dtype), width)

    if mean is not None:              # a slot of the forward's output is read in place: rows of stride(0) floats
        mean = mean.flatten(1) if mean.dim() != 2 else mean
        if not (mean.dtype == torch.float32 and width == dim and mean.stride(1) == 1 and mean.stride(0) % 4 == 0 and
                mean.stride(0) >= dim and mean.data_ptr() % 16 == 0):
            mean = dense(mean, torch.float32)
    out = torch.empty((num_cols, width), dtype=torch.float32, device=given[0].device)
    if t_indices.numel() == 0:        # nothing is gathered: the row-indexed operands may be empty
        out.zero_()
    elif num_cols > 0 and dim > 0:
        capi.launch_spmm_multi_backward(t_indptr.contiguous(), t_indices.contiguous(), t_order, num_cols, dense(feat, torch.float32),
                                        dense(u, torch.float32), dense(w, torch.float32), mean, dense(g_max, torch.float32),
                                        dense(argmax, torch.int32), dense(g_min, torch.float32), dense(argmin, torch.int32), out,
                                        _raw_stream(out.device))
    if width != dim:
        out = out[:, :dim].contiguous()
    return out.view((num_cols,) + tail)


# ``voltrix.spmm_multi`` is the function (voltrix/__init__.py); the backward stays reachable through it
spmm_multi.backward = spmm_multi_backward
spmm_multi.AGGREGATES = AGGREGATES
spmm_multi.MultiState = MultiState
