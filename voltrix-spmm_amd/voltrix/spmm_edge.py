"""Aggregation with a feature VECTOR per edge on a CSR pattern: ``out[r] = sum_{e in row r} m(feat[indices[e]], efeat[e])`` per element,
with ``m(x, w) = x * w`` (``"mul"``, DGL's ``u_mul_e_sum``), ``x + w`` (``"add"``, ``u_add_e_sum``), ``max(x + w, 0)`` (``"add_relu"``,
GINE's message) or ``w`` (``"copy"``, ``copy_e_sum``) -- what GINE, NNConv / MPNN and CGConv layers aggregate, next to the operators
that take one scalar per edge (``spmm_weighted``, ``spmm_heads``, ``attn_aggregate``) or none (``spmm_reduce``).  ``efeat`` is indexed
by CSR entry id: ``edge_feat[block.entries]`` for a sampled block or subgraph.

No reference counterpart.  One HIP launch straight from the CSR (voltrix/spmm_edge_kernels.hpp): ``feat[indices]`` ([nnz, F]) is never
materialised, nothing is scattered, and both gradients are gathers:

    out     = voltrix.spmm_edge(indptr, indices, feat, efeat, num_rows, op="mul")       # fp32 [num_rows, *tail]; feat=None for "copy"
    d_efeat = voltrix.spmm_edge.grad_efeat(indptr, indices, grad_out, feat, efeat, op)  # fp32 [nnz, *tail]
    d_feat  = voltrix.spmm_edge.grad_feat(t_indptr, t_indices, t_order, grad_out, feat, efeat, op, num_cols)

fp32 additions in CSR order (``|out - ref| <= (k + 1) 2^-23 sum |terms|`` for the ``k`` terms of an element); NaN and inf propagate as
the arithmetic does (``max(NaN + w, 0)`` is NaN); the gate of ``add_relu``'s gradients, ``(x + w) > 0``, has the sign of the exact sum
and is closed at 0, like ``torch.relu``'s.  No float atomics, no workspace, the same bits on every call.  Known limit: a hub row (in
``grad_feat``: a hub column) serialises its wave, like ``voltrix.spmm_heads``.  DESIGN.md 3.28.
"""
from __future__ import annotations

import torch

from .utils import FEATURE_TYPES, padded_last_dim, piece_width

OPS = ("mul", "add", "add_relu", "copy")


def check_operands(who: str, op, feat, efeat, num_entries=None) -> None:
    """The ``ValueError`` cases, before any tensor's device is looked at: an unknown ``op``, ``feat`` given with ``"copy"`` or missing
    otherwise, trailing shapes that differ, ``efeat`` not of ``num_entries`` rows."""
    if op not in OPS:
        raise ValueError(f"{who}: op must be one of {OPS}, got {op!r}")
    if op == "copy" and feat is not None:
        raise ValueError(f"{who}: op 'copy' sums efeat alone; feat must be None")
    if op != "copy" and feat is None:
        raise ValueError(f"{who}: op {op!r} needs feat")
    if efeat is None or efeat.dim() < 2:
        raise ValueError(f"{who}: efeat must be [nnz, ...]")
    if feat is not None and (feat.dim() < 2 or tuple(feat.shape[1:]) != tuple(efeat.shape[1:])):
        raise ValueError(f"{who}: feat {tuple(feat.shape)} and efeat {tuple(efeat.shape)} differ behind the first dimension "
                         f"(one value per head broadcast over the head's width is voltrix.spmm_heads)")
    if num_entries is not None and efeat.shape[0] != num_entries:
        raise ValueError(f"{who}: efeat has {efeat.shape[0]} rows, the pattern {num_entries} entries")


def _as_feature(t):
    return t if t is None or t.dtype in FEATURE_TYPES else t.float()


def _placeholder(width: int, like: torch.Tensor) -> torch.Tensor:
    """One row of zeros: a pointer the entry point may read where an operand has no rows (it is not read on a pattern without entries)."""
    return torch.zeros((1, width), dtype=like.dtype, device=like.device)


def spmm_edge(indptr: torch.Tensor, indices: torch.Tensor, feat, efeat: torch.Tensor, num_rows: int, op: str = "mul") -> torch.Tensor:
    """``sum_{e in row r} m(feat[indices[e]], efeat[e])`` -> float32 ``[num_rows, *efeat.shape[1:]]``, every element written (a row
    without entries: 0), on the current stream.

    ``indptr`` / ``indices``: device int32 CSR with ``num_rows`` rows (rectangular patterns and duplicate entries allowed: everything is
    addressed by entry id); ``efeat`` [nnz, ...] and ``feat`` [num_cols, ...] (``None`` for ``"copy"``) with equal trailing dimensions,
    which are flattened; fp32 / fp16 / bf16 as they are, other types as fp32.  Where the two differ in dtype ``feat`` -- [n, F], the
    cheap one -- is read as fp32; ``efeat`` keeps its stored type.  A row width that is not a whole number of 16-byte pieces of
    ``efeat``'s type is padded with zeros and sliced away: that pads ``efeat`` too, an ``[nnz, F]`` copy -- keep F a multiple of 8 (4
    for fp32) where it matters.  An operand that is contiguous and 16-byte aligned is never copied.  ``ValueError``: an unknown ``op``,
    ``feat`` given with ``"copy"`` or missing otherwise, a shape mismatch (``efeat.shape[0] != indices.numel()`` included)."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    check_operands("spmm_edge", op, feat, efeat, None if indices is None else indices.numel())
    assert indptr.is_cuda and indices.is_cuda and indptr.dtype == torch.int32 and indices.dtype == torch.int32
    assert indptr.numel() == num_rows + 1 and efeat.is_cuda and (feat is None or feat.is_cuda)
    feat, efeat = _as_feature(feat), _as_feature(efeat)
    if feat is not None and feat.dtype != efeat.dtype:
        feat = feat.float()
    return _launch(capi, _raw_stream, indptr, indices, None, feat, efeat, None, num_rows, op)


def _launch(capi, raw_stream, indptr, indices, order, feat, efeat, self_rows, num_rows, op):
    """The forward kernel on operands whose dtypes are a pair it takes: flatten, pad to whole pieces of ``efeat``'s type, launch, slice."""
    tail = tuple(efeat.shape[1:])
    efeat = efeat.flatten(1)
    dim = efeat.shape[1]
    width = piece_width(max(dim, 1), efeat.dtype)
    out = torch.empty((num_rows, width), dtype=torch.float32, device=efeat.device)
    if num_rows > 0 and dim > 0:
        efeat = padded_last_dim(efeat, width)
        feat = None if feat is None else padded_last_dim(feat.flatten(1), width)
        self_rows = None if self_rows is None else padded_last_dim(self_rows.flatten(1), width)
        num_entries = indices.numel()
        if num_entries == 0:          # nothing is gathered; the entry point still wants pointers it could read
            indices, order, efeat = indptr, None, _placeholder(width, efeat)
        if feat is not None and feat.shape[0] == 0:
            feat = _placeholder(width, feat)
        capi.launch_spmm_edge(indptr.contiguous(), indices.contiguous(), order, num_rows, feat, efeat, self_rows, op, out,
                              raw_stream(out.device), num_entries)
    if width != dim:
        out = out[:, :dim].contiguous()
    return out.view((num_rows,) + tail)


def _check_gradient(who: str, op, feat, efeat, grad_out, num_entries) -> None:
    """``check_operands`` for a gradient: add and copy read neither operand, so both may be None there; operands that are given must
    have ``grad_out``'s trailing dimensions."""
    if op in ("add", "copy") and feat is None and efeat is None:
        return
    check_operands(who, op, feat, efeat, num_entries)
    if tuple(grad_out.shape[1:]) != tuple(efeat.shape[1:]):
        raise ValueError(f"{who}: grad_out {tuple(grad_out.shape)} and efeat {tuple(efeat.shape)} differ behind the first dimension")


def grad_efeat(indptr: torch.Tensor, indices: torch.Tensor, grad_out: torch.Tensor, feat, efeat: torch.Tensor, op: str) -> torch.Tensor:
    """The gradient of ``spmm_edge`` for ``efeat`` -> float32 ``[nnz, *efeat.shape[1:]]``, every element written:
    ``g * feat[col_e]`` (mul), ``g`` (add, copy), ``(feat[col_e] + efeat[e]) > 0 ? g : 0`` (add_relu) with ``g = grad_out[row_e]``
    (cast to float32).  One row-parallel launch on the same CSR, no atomics.  mul reads ``feat`` alone, add / copy neither operand (both
    may be None there).
    add_relu reads both in ONE dtype: where they differ both are read as fp32, which copies ``efeat`` ([nnz, F]) -- the one place a mixed
    pair costs that; the gate is the same either way (the conversion is exact)."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    _check_gradient("spmm_edge.grad_efeat", op, feat, efeat, grad_out, None if indices is None else indices.numel())
    assert indptr.is_cuda and indices.is_cuda and indptr.dtype == torch.int32 and indices.dtype == torch.int32
    assert grad_out.is_cuda and grad_out.shape[0] == indptr.numel() - 1
    num_rows, nnz = grad_out.shape[0], indices.numel()
    tail = tuple(grad_out.shape[1:])
    feat, efeat = _as_feature(feat), _as_feature(efeat)
    if op in ("add", "copy"):
        feat = efeat = None
        dtype = torch.float32
    elif op == "mul":
        efeat, dtype = None, feat.dtype
    else:
        if feat.dtype != efeat.dtype:
            feat, efeat = feat.float(), efeat.float()
        dtype = feat.dtype
    grad_out = grad_out.float().flatten(1)
    dim = grad_out.shape[1]
    width = piece_width(max(dim, 1), dtype)
    out = torch.empty((nnz, width), dtype=torch.float32, device=grad_out.device)
    if nnz > 0 and dim > 0:
        feat = None if feat is None else padded_last_dim(feat.flatten(1), width)
        efeat = None if efeat is None else padded_last_dim(efeat.flatten(1), width)
        capi.launch_spmm_edge_grad_efeat(indptr.contiguous(), indices.contiguous(), num_rows, padded_last_dim(grad_out, width), feat,
                                         efeat, dtype, op, out, _raw_stream(out.device))
    if width != dim:
        out = out[:, :dim].contiguous()
    return out.view((nnz,) + tail)


def grad_feat(t_indptr: torch.Tensor, t_indices: torch.Tensor, t_order: torch.Tensor, grad_out: torch.Tensor, feat, efeat: torch.Tensor,
              op: str, num_cols: int) -> torch.Tensor:
    """The gradient of ``spmm_edge`` for ``feat`` -> float32 ``[num_cols, *efeat.shape[1:]]``, every row written, columns without
    entries zero: a gather on the TRANSPOSED CSR (``voltrix.autograd.csr_transpose_device``; ``t_order``: the entry of the CSR that
    entry ``e`` of the transpose is), in its order -- no float atomics, the same bits on every call.

    mul: the forward kernel on the transpose with ``grad_out`` as the gathered operand and ``efeat`` read at ``t_order[e]``; add: the CSR
    row-gather sum of ``grad_out`` (neither operand is read: both may be None); add_relu: the kernel's gate op, ``sum_e (feat[c] + efeat[t_order[e]]) > 0 ? grad_out[row_e] : 0``.
    ``efeat`` keeps its stored 16-bit type beside the fp32 ``grad_out`` (nothing of size [nnz, F] is copied), except that add_relu with a
    ``feat`` of another dtype reads ``efeat`` as fp32 (the gate needs both in one type).  ``"copy"`` has no ``feat``: a ``ValueError``."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    if op == "copy":
        raise ValueError("spmm_edge.grad_feat: op 'copy' has no feat")
    _check_gradient("spmm_edge.grad_feat", op, feat, efeat, grad_out, None if t_indices is None else t_indices.numel())
    assert t_indptr.is_cuda and t_indices.is_cuda and t_indptr.dtype == torch.int32 and t_indices.dtype == torch.int32
    assert t_indptr.numel() == num_cols + 1 and grad_out.is_cuda and t_order.is_cuda and t_order.numel() == t_indices.numel()
    t_order = t_order.to(torch.int32).contiguous()
    grad_out = grad_out.float()
    if op == "add":
        tail = tuple(grad_out.shape[1:])
        grad_out = grad_out.flatten(1)
        dim = grad_out.shape[1]
        width = piece_width(max(dim, 1), torch.float32)
        out = torch.empty((num_cols, width), dtype=torch.float32, device=grad_out.device)
        if num_cols > 0 and dim > 0:
            if t_indices.numel() == 0:
                out.zero_()
            else:
                capi.launch_spmm_csr_rows(t_indptr.contiguous(), t_indices.contiguous(), num_cols, padded_last_dim(grad_out, width), out,
                                          _raw_stream(out.device), 1)
        if width != dim:
            out = out[:, :dim].contiguous()
        return out.view((num_cols,) + tail)
    efeat = _as_feature(efeat)
    if op == "mul":
        return _launch(capi, _raw_stream, t_indptr, t_indices, t_order, grad_out, efeat, None, num_cols, "mul")
    feat = _as_feature(feat)
    if feat.dtype != efeat.dtype:
        feat, efeat = feat.float(), efeat.float()
    assert feat.shape[0] == num_cols, (tuple(feat.shape), num_cols)
    return _launch(capi, _raw_stream, t_indptr, t_indices, t_order, grad_out, efeat, feat, num_cols, "gate")


# ``voltrix.spmm_edge`` is the function (voltrix/__init__.py); the gradients stay reachable through it
spmm_edge.grad_efeat = grad_efeat
spmm_edge.grad_feat = grad_feat
spmm_edge.OPS = OPS
