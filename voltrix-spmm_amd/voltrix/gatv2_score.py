"""GATv2 edge scores: ``s[e, h] = sum_d a[h, d] * leaky_relu(xl[row_e, h, d] + xr[col_e, h, d], slope)`` for every entry of a CSR pattern
(Brody et al.; ``GATv2Conv``) -- the first step of a GATv2 layer, before ``voltrix.edge_softmax`` -- and the gated row sum of its backward.

No reference counterpart -- the reference is forward-only and has no edge values.  The non-linearity sits inside the sum over ``d``, so
``s`` is neither ``voltrix.gat_score`` (per-node scalars) nor ``voltrix.sddmm`` (a bilinear form); a torch composite materialises
``[nnz, H, D]``.  The HIP kernels (voltrix/gatv2_score_kernels.hpp) never do: the forward is split by edges, gathers one row of ``xr`` per
edge and writes ``H`` floats; the backward is a row sum per side,

    s = voltrix.gatv2_score(indptr, indices, xl, xr, a, slope=0.2)              # float32 [nnz, H] (or [nnz]), CSR order
    G_l = gatv2_rowsum(indptr, indices, xl, xr, g, slope)                       # [num_rows, H, D]: sum over every row of gate * g
    G_r = gatv2_rowsum(t_indptr, t_indices, xr, xl, g, slope, order=t_order)    # the same on the transposed CSR
    d_xl, d_xr, d_a = a * G_l, a * G_r, (xl * G_l).sum(0) + (xr * G_r).sum(0)   # dense: leaky_relu(z) = gate(z) * z

with ``gate(z) = 1 if z > 0 else slope`` (``z == 0`` and NaN take the slope branch, as ``torch.nn.functional.leaky_relu``).  No float
atomics and no index op in either direction: the same inputs give the same bits on every call.  Numerics, against float64 from the inputs
as stored: ``|s - ref| <= (D + 2) * 2^-23 * sum_d |a_d| |leaky_relu(z_d)| + 2^-149``; a row sum over ``deg`` entries is within
``deg * 2^-23 * sum_e |gate_e * g_e| + 2^-149``.  ``out[:, h]`` of an ``H``-head call has the bits of the 2-D call on the contiguous slices.
"""
from __future__ import annotations

import torch

from .utils import FEATURE_TYPES, padded_last_dim, piece_width


def _pair(x: torch.Tensor, y: torch.Tensor):
    """``x`` and ``y`` [n, H, D] in one type the kernels take: as they are when they share fp32 / fp16 / bf16, else both as float32."""
    assert x.is_cuda and y.is_cuda and x.dim() == y.dim() and x.dim() in (2, 3) and x.shape[1:] == y.shape[1:], (tuple(x.shape), tuple(y.shape))
    if x.dtype != y.dtype or x.dtype not in FEATURE_TYPES:
        x, y = x.float(), y.float()
    if x.dim() == 2:                      # the 2-D form is the H = 1 layout: the same kernel, the same bits
        x, y = x.unsqueeze(1), y.unsqueeze(1)
    assert x.shape[1] >= 1
    return x, y


def gatv2_score(indptr: torch.Tensor, indices: torch.Tensor, xl: torch.Tensor, xr: torch.Tensor, a: torch.Tensor,
                slope: float = 0.2) -> torch.Tensor:
    """``sum_d a[h, d] * leaky_relu(xl[row_e, h, d] + xr[indices[e], h, d], slope)`` for every entry -> float32 [nnz, H] in CSR order, on
    the current stream.

    ``indptr`` / ``indices``: device int32 CSR ([num_rows + 1], [nnz]; duplicates are edges of their own); ``xl`` CUDA [num_rows, H, D],
    ``xr`` CUDA [num_cols, H, D], ``a`` [H, D] (cast to float32); ``slope``: a finite float.  ``xl`` and ``xr`` run as they are when they
    share fp32 / fp16 / bf16; a mixed or other-typed pair is cast to float32.  The 2-D form ``xl`` [num_rows, D], ``xr`` [num_cols, D],
    ``a`` [D] -> [nnz] is the ``H = 1`` layout.  A head width that is not a multiple of 16 bytes is padded with zeros per head, ``a``
    included.  Passing one tensor as ``xl`` and ``xr`` is GATv2's ``share_weights``."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    assert indptr.is_cuda and indptr.dtype == torch.int32 and indices.is_cuda and indices.dtype == torch.int32
    one_d = xl.dim() == 2
    xl, xr = _pair(xl, xr)
    num_rows, nnz = indptr.numel() - 1, indices.numel()
    heads, head_dim = xl.shape[1], xl.shape[2]
    assert xl.shape[0] == num_rows and a.is_cuda and tuple(a.shape) == ((head_dim,) if one_d else (heads, head_dim)), tuple(a.shape)
    out = torch.empty((nnz, heads), dtype=torch.float32, device=xl.device)
    if nnz > 0 and head_dim == 0:
        out.zero_()
    elif nnz > 0:
        width = piece_width(head_dim, xl.dtype)
        a = padded_last_dim(a.float().reshape(1, heads, head_dim), width).view(heads, width)
        capi.launch_gatv2_score_csr(indptr.contiguous(), indices.contiguous(), num_rows, padded_last_dim(xl, width), padded_last_dim(xr, width),
                                    a, float(slope), out, _raw_stream(xl.device))
    return out.view(-1) if one_d else out


def gatv2_rowsum(indptr: torch.Tensor, indices: torch.Tensor, p: torch.Tensor, q: torch.Tensor, grad: torch.Tensor, slope: float,
                 order: torch.Tensor = None) -> torch.Tensor:
    """One side of the backward: ``G[r, h, d] = sum_{e in row r} gate(p[r, h, d] + q[indices[e], h, d]) * grad[order[e] if order else e,
    h]`` with ``gate(z) = 1 if z > 0 else slope`` -> float32 [num_rows, H, D] (2-D ``p``, ``q`` and 1-D ``grad``: [num_rows, D]); every
    row is written, empty rows are 0.

    ``G_l``: the CSR, ``(p, q) = (xl, xr)``.  ``G_r``: the transposed CSR (``voltrix.autograd.csr_transpose_device``), ``(p, q) = (xr,
    xl)`` and ``order`` = device int32 [nnz], the entry of the CSR that entry ``e`` of the transpose is (``weighted.transpose_order``) --
    ``grad`` stays in CSR order and is never permuted.  A row per lane group: a hub row serialises its wave, as in ``voltrix.spmm_heads``."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    assert indptr.is_cuda and indptr.dtype == torch.int32 and indices.is_cuda and indices.dtype == torch.int32
    one_d = p.dim() == 2
    p, q = _pair(p, q)
    num_rows, nnz = indptr.numel() - 1, indices.numel()
    heads, head_dim = p.shape[1], p.shape[2]
    assert grad.is_cuda and grad.dim() == (1 if one_d else 2)
    grad = grad.float().contiguous().view(-1, 1) if one_d else grad.float().contiguous()
    assert p.shape[0] == num_rows and grad.shape == (nnz, heads), (tuple(p.shape), tuple(grad.shape))
    if order is not None:
        assert order.is_cuda and order.numel() == nnz
        order = order.to(torch.int32).contiguous()
    width = piece_width(head_dim, p.dtype)
    out = torch.empty((num_rows, heads, width), dtype=torch.float32, device=p.device)
    if num_rows > 0 and head_dim > 0:
        capi.launch_gatv2_rowsum_csr(indptr.contiguous(), indices.contiguous(), order, num_rows, padded_last_dim(p, width),
                                     padded_last_dim(q, width), grad, float(slope), out, _raw_stream(p.device))
    if width != head_dim:
        out = out[:, :, :head_dim].contiguous()
    return out.view(num_rows, head_dim) if one_d else out
