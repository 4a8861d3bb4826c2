"""Max / min / mean neighbour aggregation on a CSR pattern: ``out[r] = reduce_{e in row r} feat[indices[e]]`` per element -- the
aggregators of max-pool GraphSAGE, PNA's towers, GIN-max and point-cloud edge convolutions, next to the sums every other operator here
computes (``voltrix.spmm``, ``spmm_weighted``, ``spmm_heads``, ``attn_aggregate``).

No reference counterpart.  One HIP launch straight from the CSR (voltrix/spmm_csr_reduce_kernels.hpp): ``feat[indices]`` ([nnz, F]) is
never materialised, nothing is scattered, and the backward is a gather on the transposed CSR:

    out, arg = voltrix.spmm_reduce(indptr, indices, feat, num_rows, reduce="max", return_arg=True)
    d_feat = spmm_reduce_backward(t_indptr, t_indices, t_order, dC, arg, num_cols)            # max / min
    d_feat = spmm_csr_rows(transposed CSR, dC / deg[:, None])                                 # mean (autograd.SpMMReduce)

``arg[r, f]`` is the CSR ENTRY id of the winner, not its column: on a pattern with duplicate ``(row, col)`` entries a column id would
match both and count the gradient twice.  The first entry in CSR order wins ties (``+0`` and ``-0`` tie); a NaN among a row's entries
gives NaN with ``arg`` at the first NaN (``torch.amax``); a row without entries gives ``0`` and ``arg = -1``.  A selection does not
round: ``out`` holds the winning element as float32 for every dtype.  mean is fp32 additions in CSR order and one fp32 division
(``|out - ref| <= (deg + 1) 2^-23 sum_e |feat_e| / deg``; duplicates count twice).  No float atomics, the same bits on every call.
Known limit: a hub row (forward) or hub column (backward) serialises its wave, like ``voltrix.spmm_heads``.  DESIGN.md 3.22.
"""
from __future__ import annotations

import torch

from .utils import FEATURE_TYPES, aligned16, padded_last_dim, piece_width

REDUCTIONS = ("max", "min", "mean")


def spmm_reduce(indptr: torch.Tensor, indices: torch.Tensor, feat: torch.Tensor, num_rows: int, reduce: str = "max",
                return_arg: bool = False):
    """``max`` / ``min`` / ``mean`` over every row's entries of ``feat[indices[e]]`` -> float32 ``[num_rows, *feat.shape[1:]]``, every
    element written, on the current stream; with ``return_arg`` (max / min) also ``arg``, int32 of the same shape: the CSR entry id of
    the winner, ``-1`` for a row without entries.

    ``indptr`` / ``indices``: device int32 CSR with ``num_rows`` rows (rectangular patterns and duplicates allowed); ``feat``
    [num_cols, ...] fp32 / fp16 / bf16 as it is (other types as fp32), trailing dimensions flattened.  A row width that is not a
    multiple of 16 bytes is padded with zeros (the padded columns are sliced away); an operand that is contiguous and 16-byte aligned is
    never copied.  ``reduce`` outside ``("max", "min", "mean")``, or ``return_arg`` with ``"mean"``, is a ``ValueError``."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    if reduce not in REDUCTIONS:
        raise ValueError(f"spmm_reduce: reduce must be one of {REDUCTIONS}, got {reduce!r}")
    if return_arg and reduce == "mean":
        raise ValueError("spmm_reduce: the mean has no winner; return_arg needs reduce='max' or 'min'")
    assert indptr.is_cuda and indices.is_cuda and indptr.dtype == torch.int32 and indices.dtype == torch.int32
    assert indptr.numel() == num_rows + 1 and feat.is_cuda and feat.dim() >= 2, tuple(feat.shape)
    if feat.dtype not in FEATURE_TYPES:
        feat = feat.float()
    tail = tuple(feat.shape[1:])
    feat = feat.flatten(1)
    dim = feat.shape[1]
    width = piece_width(max(dim, 1), feat.dtype)
    out = torch.empty((num_rows, width), dtype=torch.float32, device=feat.device)
    arg = torch.empty((num_rows, width), dtype=torch.int32, device=feat.device) if return_arg else None
    if num_rows > 0 and dim > 0:
        feat = padded_last_dim(feat, width)
        if indices.numel() == 0:      # nothing is gathered; the entry point still wants pointers it could read
            indices = indptr
            if feat.shape[0] == 0:
                feat = torch.zeros((1, width), dtype=feat.dtype, device=feat.device)
        capi.launch_spmm_csr_reduce(indptr.contiguous(), indices.contiguous(), num_rows, feat, reduce, out, arg, _raw_stream(feat.device))
    if width != dim:
        out = out[:, :dim].contiguous()
        arg = arg[:, :dim].contiguous() if return_arg else None
    out = out.view((num_rows,) + tail)
    return (out, arg.view((num_rows,) + tail)) if return_arg else out


def spmm_reduce_backward(t_indptr: torch.Tensor, t_indices: torch.Tensor, t_order: torch.Tensor, grad_out: torch.Tensor,
                         arg: torch.Tensor, num_cols: int) -> torch.Tensor:
    """The gradient of ``spmm_reduce(..., "max" | "min")`` for ``feat``: ``d_feat[c, f] = sum of grad_out[r, f] over the entries e of
    column c with arg[r, f] == e`` -> float32 ``[num_cols, *grad_out.shape[1:]]``, every row written, columns without entries zero.
    ``t_indptr`` / ``t_indices``: the transposed device CSR (``voltrix.autograd.csr_transpose_device``); ``t_order``: device [nnz], the
    entry of the CSR that entry ``e`` of the transpose is (``weighted.transpose_order``; kept as int32); ``grad_out`` (cast to float32)
    and the forward's int32 ``arg``, both ``[num_rows, ...]``.  A gather in the transposed CSR's order: no float atomics, the same bits on
    every call.  A column per lane group: a hub column serialises its wave."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    assert t_indptr.is_cuda and t_indices.is_cuda and t_indptr.dtype == torch.int32 and t_indices.dtype == torch.int32
    assert t_indptr.numel() == num_cols + 1 and grad_out.is_cuda and arg.is_cuda and grad_out.dim() >= 2
    assert arg.shape == grad_out.shape and arg.dtype == torch.int32, (tuple(arg.shape), tuple(grad_out.shape), arg.dtype)
    assert t_order.is_cuda and t_order.numel() == t_indices.numel()
    t_order = t_order.to(torch.int32).contiguous()
    tail = tuple(grad_out.shape[1:])
    grad_out = grad_out.float().flatten(1)
    arg = arg.flatten(1)
    dim = grad_out.shape[1]
    width = (max(dim, 1) + 3) // 4 * 4
    out = torch.empty((num_cols, width), dtype=torch.float32, device=grad_out.device)
    if num_cols > 0 and dim > 0:
        # a lane owns 4 features: both operands are padded with zeros to a multiple of 4 columns.  The padding only feeds output columns
        # that are sliced away below -- a zero-padded arg reads as "entry 0 won" there, which would be wrong anywhere else
        capi.launch_spmm_csr_reduce_backward(t_indptr.contiguous(), t_indices.contiguous(), t_order, num_cols,
                                             padded_last_dim(grad_out, width), padded_last_dim(arg, width), out,
                                             _raw_stream(grad_out.device))
    if width != dim:
        out = out[:, :dim].contiguous()
    return out.view((num_cols,) + tail)


def row_degrees(indptr: torch.Tensor) -> torch.Tensor:
    """float32 [num_rows]: the entries of every row, duplicates counted, 1 for a row without entries (its mean is 0 either way)."""
    return (indptr[1:] - indptr[:-1]).clamp(min=1).float()


def spmm_mean_backward(t_indptr: torch.Tensor, t_indices: torch.Tensor, grad_out: torch.Tensor, degrees: torch.Tensor,
                       num_cols: int) -> torch.Tensor:
    """The gradient of ``spmm_reduce(..., "mean")`` for ``feat``: ``A^T (grad_out / deg)`` -> float32 ``[num_cols, *grad_out.shape[1:]]``
    -- a dense division and the CSR row-gather sum kernel on the transposed CSR (``degrees``: ``row_degrees(indptr)``)."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    tail = tuple(grad_out.shape[1:])
    grad_out = grad_out.float().flatten(1)
    dim = grad_out.shape[1]
    width = (max(dim, 1) + 3) // 4 * 4
    out = torch.empty((num_cols, width), dtype=torch.float32, device=grad_out.device)
    if num_cols > 0 and dim > 0:
        if t_indices.numel() == 0:
            out.zero_()
        else:
            scaled = aligned16(padded_last_dim(grad_out / degrees[:, None], width))
            capi.launch_spmm_csr_rows(t_indptr.contiguous(), t_indices.contiguous(), num_cols, scaled, out, _raw_stream(out.device), 1)
    if width != dim:
        out = out[:, :dim].contiguous()
    return out.view((num_cols,) + tail)


# ``voltrix.spmm_reduce`` is the function (voltrix/__init__.py); the backward pieces stay reachable through it
spmm_reduce.spmm_reduce_backward = spmm_reduce_backward
spmm_reduce.spmm_mean_backward = spmm_mean_backward
spmm_reduce.row_degrees = row_degrees
