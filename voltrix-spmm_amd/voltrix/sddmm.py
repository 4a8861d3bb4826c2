"""Sampled dense-dense product (SDDMM): ``out[e] = <x[row_e], y[indices[e]]>`` for every entry of a CSR pattern.

No reference counterpart -- the reference is forward-only and has no edge values.  It is what a model that learns its edge
values needs: the gradient of ``C = csr(v) @ B`` with respect to the values is ``sddmm(dC, B)``, and dot-product attention scores
are ``sddmm(Q, K)``.  One HIP kernel (voltrix/sddmm_kernels.hpp) splits the work by edges, so hub rows cost what their edges cost.

    scores = voltrix.sddmm(indptr, indices, q, k)          # float32 [nnz], CSR order

Numerics: fp32 products and sum, one fused multiply-add per element, in an order fixed by the width alone:
``|out - ref| <= F 2^-23 (|x| |y|)[e]``; the same inputs give the same bits on every call, and duplicate entries the same value.
"""
from __future__ import annotations

import torch

from .utils import FEATURE_TYPES, padded_last_dim, piece_width

_PAIRS = {(torch.float32, torch.float16), (torch.float32, torch.bfloat16), (torch.float16, torch.float16),
          (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32)}


def sddmm(indptr: torch.Tensor, indices: torch.Tensor, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """``out[e] = sum_k x[row_e, k] * y[indices[e], k]`` -> float32 [nnz] in CSR order, on the current stream.

    ``indptr`` / ``indices``: device int32 CSR of a [num_rows, num_cols] pattern; ``x`` [num_rows, F], ``y`` [num_cols, F], both CUDA.
    Multi-head: ``x`` [num_rows, H, D], ``y`` [num_cols, H, D] -> float32 [nnz, H], ``out[e, h] = <x[row_e, h], y[indices[e], h]>``
    from one launch (voltrix/sddmm_heads_kernels.hpp); ``out[:, h]`` has the bits of the 2-D call on ``x[:, h]``, ``y[:, h]``.
    Pairs (x, y) run as they are: (fp32, fp16), (fp32, bf16), (fp16, fp16), (bf16, bf16), (fp32, fp32); any other pair is cast first
    (x to fp32, and y too unless it is fp16 / bf16).  Widths that are not a multiple of 16 bytes are padded with zeros."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    assert indptr.is_cuda and indices.is_cuda and indptr.dtype == torch.int32 and indices.dtype == torch.int32
    if x.dim() == 3:
        return _sddmm_heads(indptr, indices, x, y)
    assert x.is_cuda and y.is_cuda and x.dim() == 2 and y.dim() == 2 and x.shape[1] == y.shape[1]
    num_rows = indptr.numel() - 1
    assert x.shape[0] == num_rows, (tuple(x.shape), num_rows)
    if (x.dtype, y.dtype) not in _PAIRS:
        y = y if y.dtype in FEATURE_TYPES else y.float()
        x = x.float()
    nnz = indices.numel()
    out = torch.empty(nnz, dtype=torch.float32, device=x.device)
    num_feats = x.shape[1]
    if nnz == 0:
        return out
    if num_feats == 0:
        return out.zero_()
    width = piece_width(num_feats, (x.dtype, y.dtype))
    capi.launch_sddmm_csr(indptr.contiguous(), indices.contiguous(), num_rows, padded_last_dim(x, width), padded_last_dim(y, width), out,
                          _raw_stream(x.device))
    return out


def _sddmm_heads(indptr: torch.Tensor, indices: torch.Tensor, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """The 3-D form of ``sddmm``: one launch for all heads; a head width that is not a multiple of 16 bytes is padded per head."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    assert x.is_cuda and y.is_cuda and y.dim() == 3 and x.shape[1:] == y.shape[1:], (tuple(x.shape), tuple(y.shape))
    num_rows = indptr.numel() - 1
    assert x.shape[0] == num_rows, (tuple(x.shape), num_rows)
    if (x.dtype, y.dtype) not in _PAIRS:
        y = y if y.dtype in FEATURE_TYPES else y.float()
        x = x.float()
    nnz, heads, head_dim = indices.numel(), x.shape[1], x.shape[2]
    assert heads >= 1
    out = torch.empty((nnz, heads), dtype=torch.float32, device=x.device)
    if nnz == 0:
        return out
    if head_dim == 0:
        return out.zero_()
    width = piece_width(head_dim, (x.dtype, y.dtype))
    capi.launch_sddmm_heads_csr(indptr.contiguous(), indices.contiguous(), num_rows, padded_last_dim(x, width), padded_last_dim(y, width),
                                out, _raw_stream(x.device))
    return out


def spmm_heads(indptr: torch.Tensor, indices: torch.Tensor, values: torch.Tensor, feat: torch.Tensor, num_rows: int) -> torch.Tensor:
    """Multi-head aggregation ``out[r, h, :] = sum_{e in row r} values[e, h] * feat[indices[e], h, :]`` -> float32 [num_rows, H, D], on
    the current stream (voltrix/spmm_csr_heads_kernels.hpp).

    ``indptr`` / ``indices``: device int32 CSR with ``num_rows`` rows; ``values`` [nnz, H] in CSR order (cast to float32); ``feat``
    [num_cols, H, D] fp32 / fp16 / bf16 as it is (other types as fp32).  One index read and one gathered row per edge serve all heads;
    nothing is installed into a block-format handle.  fp32 products, one fused multiply-add per element, summed in CSR order:
    ``out[:, h]`` has the bits of ``csr_values_product`` on ``values[:, h]``, ``feat[:, h]``;
    ``|out - ref| <= deg_r 2^-23 sum_e |values[e, h]| |feat[col_e, h, d]|``.  Empty rows are zero."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    assert indptr.is_cuda and indices.is_cuda and indptr.dtype == torch.int32 and indices.dtype == torch.int32
    assert feat.is_cuda and values.is_cuda and feat.dim() == 3 and values.dim() == 2, (tuple(feat.shape), tuple(values.shape))
    assert indptr.numel() == num_rows + 1 and values.shape == (indices.numel(), feat.shape[1]), (tuple(values.shape), tuple(feat.shape))
    if feat.dtype not in FEATURE_TYPES:
        feat = feat.float()
    heads, head_dim = feat.shape[1], feat.shape[2]
    assert heads >= 1
    if indices.numel() == 0 or head_dim == 0 or num_rows == 0:
        return torch.zeros((num_rows, heads, head_dim), dtype=torch.float32, device=feat.device)
    if heads == 1:      # one head is the single-head layout: its kernel, measured faster at H = 1, the same bits
        return csr_values_product(indptr.contiguous(), indices.contiguous(), values.reshape(-1), num_rows,
                                  feat.reshape(feat.shape[0], head_dim)).view(num_rows, 1, head_dim)
    width = piece_width(head_dim, feat.dtype)
    output = torch.empty((num_rows, heads, width), dtype=torch.float32, device=feat.device)
    capi.launch_spmm_csr_heads(indptr.contiguous(), indices.contiguous(), values.float().contiguous(), num_rows,
                               padded_last_dim(feat, width), output, _raw_stream(feat.device))
    return output if width == head_dim else output[:, :, :head_dim].contiguous()


def csr_values_product(indptr: torch.Tensor, indices: torch.Tensor, values: torch.Tensor, num_rows: int,
                       feat: torch.Tensor) -> torch.Tensor:
    """``csr(values) @ feat`` -> float32 [num_rows, F] with the CSR row-gather kernel with values (``spmm_csr_rows_kernel<T, 4,
    true>``): fp32 / fp16 / bf16 rows as they are (other types as fp32), fp32 values, one fused multiply-add per element."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    if feat.dtype not in FEATURE_TYPES:
        feat = feat.float()
    num_feats = feat.shape[1]
    if indices.numel() == 0 or num_feats == 0 or num_rows == 0:
        return torch.zeros(num_rows, num_feats, dtype=torch.float32, device=feat.device)
    width = piece_width(num_feats, feat.dtype)
    output = torch.empty((num_rows, width), dtype=torch.float32, device=feat.device)
    capi.launch_spmm_csr_rows(indptr, indices, num_rows, padded_last_dim(feat, width), output, _raw_stream(feat.device), 1,
                              values=values.float().contiguous())
    return output if width == num_feats else output[:, :num_feats].contiguous()
