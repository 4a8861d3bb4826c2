"""Edge softmax and multi-head aggregation in one launch: ``out[r, h] = sum_{e in row r} alpha[e, h] * feat[indices[e], h]`` with ``alpha``
the softmax of ``scale * scores`` over every row of a CSR pattern -- the last two steps of an attention layer
(``spmm_heads(edge_softmax(scores, scale), feat)``) without ``alpha`` [nnz, H] ever being written, and a backward without ``grad_alpha``.

No reference counterpart -- the reference is forward-only and has no edge values.  The HIP kernels (voltrix/attn_aggregate_kernels.hpp)
keep two numbers per row and head, the maximum ``m`` and the sum ``l`` of the exponentials, from which ``alpha[e, h]`` is recomputed
wherever it is needed:

    out, m, l = voltrix.attn_aggregate(indptr, indices, scores, feat, num_rows, scale, return_stats=True)
    delta = (dC * out).sum(-1)                                                                   # dense [num_rows, H]
    d_s = attn_aggregate_grad_scores(indptr, indices, dC, feat, scores, m, l, delta, scale)      # [nnz, H], split by edges
    d_feat = attn_aggregate_grad_feat(t_indptr, t_indices, t_order, dC, scores, m, l, num_cols, scale)   # the transposed CSR

``sum_e alpha_e <dC_r, feat_e> = <dC_r, out_r>`` turns the softmax backward's row reduction into the dense product ``delta``;
``d_s = scale * alpha * (<dC[row], feat[col]> - delta[row])`` is one SDDMM-shaped launch and ``d_feat`` one ``spmm_heads``-shaped launch
with ``alpha`` recomputed per edge from ``scores[t_order[e]]`` -- ``dC`` is never permuted and no [nnz, H] tensor but ``d_s`` is allocated.
One launch forward instead of four, two and a dense product backward instead of five and two gathers; no float atomics, the same bits on
every call, nothing read back on the host.

Special values are those of the unfused chain: ``-inf`` weighs 0; a row, or a row's head, holding only ``-inf`` gives zeros (``l = 0``)
and zero gradients; an empty row gives zeros; a NaN or ``+inf`` score stays in its own row and head; ``scale = 0`` is the mean over the
entries that are not ``-inf``.  Numerics: DESIGN.md 3.17; ``out[:, h]``, ``d_s[:, h]``, ``d_feat[:, h]`` of an ``H``-head call have the
bits of the 2-D call on the contiguous slices.  Known limit: the forward and ``d_feat`` walk a hub row with one wave, like
``voltrix.spmm_heads``.

Attention dropout: ``mask=`` (int32 [nnz, ceil(H / 32)] keep bits, ``voltrix.dropout_mask``) and ``keep_scale=`` on all
three functions.  ``out = sum_e alpha_e k_e feat_e`` with ``k = keep_scale`` where the bit is set and 0 elsewhere; ``m`` and ``l`` stay
those of the undropped softmax, ``delta = (dC * out).sum(-1)`` holds with the dropped ``out``, ``d_s = scale * alpha * (k * dot - delta)``
and ``d_feat`` weighs by ``alpha * k``.  A dropped entry's row is not read.  ``mask=None`` is the call without dropout, untouched.
"""
from __future__ import annotations

import math

import torch

from .utils import FEATURE_TYPES, padded_last_dim, piece_width


def _scores(scores: torch.Tensor, nnz: int, heads: int) -> torch.Tensor:
    assert scores.is_cuda and scores.numel() == nnz * heads, (tuple(scores.shape), nnz, heads)
    return scores.float().contiguous().view(nnz, heads)


def _finite(scale) -> float:
    scale = float(scale)
    if not math.isfinite(scale):
        raise ValueError(f"attn_aggregate: scale must be finite, got {scale}")
    return scale


def _mask(mask, keep_scale, nnz: int, heads: int, device):
    """``(mask, keep_scale)`` validated and layout-repaired; ``(None, 1.0)`` without a mask."""
    if mask is None:
        return None, 1.0
    from .dropout import check_keep_scale, check_mask

    return check_mask(mask, nnz, heads, device), check_keep_scale(keep_scale)


def attn_aggregate(indptr: torch.Tensor, indices: torch.Tensor, scores: torch.Tensor, feat: torch.Tensor, num_rows: int,
                   scale: float = 1.0, return_stats: bool = False, mask: torch.Tensor = None, keep_scale: float = 1.0):
    """``sum_{e in row r} softmax(scale * scores)[e, h] * feat[indices[e], h, :]`` -> float32 [num_rows, H, D], every element written, on
    the current stream; with ``return_stats`` also ``m`` and ``l``, float32 [num_rows, H]: the row maximum of ``sign(scale) * scores``
    (``-inf`` for an empty row) and the sum of ``exp(|scale| * (sign(scale) * scores - m))``.

    ``indptr`` / ``indices``: device int32 CSR with ``num_rows`` rows (rectangular patterns and duplicates allowed); ``scores`` [nnz, H]
    in CSR order, head index fastest (cast to float32); ``feat`` [num_cols, H, D] fp32 / fp16 / bf16 as it is (other types as fp32);
    ``scale``: a finite float, negative allowed.  The 2-D form ``scores`` [nnz], ``feat`` [num_cols, D] -> [num_rows, D] (``m``, ``l``
    [num_rows]) is the ``H = 1`` layout through the same kernel.  A head width that is not a multiple of 16 bytes is padded with zeros
    per head; an operand that is contiguous and 16-byte aligned is never copied.

    ``mask`` (int32 [nnz, ceil(H / 32)] keep bits) and ``keep_scale`` (finite, >= 0): attention dropout -- a kept entry weighs
    ``alpha * keep_scale``, a dropped one nothing and its row of ``feat`` is not read; ``m`` and ``l`` are those of the call without a
    mask.  A wrong dtype, shape or device of the mask is a ``ValueError``."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    assert indptr.is_cuda and indices.is_cuda and indptr.dtype == torch.int32 and indices.dtype == torch.int32
    assert indptr.numel() == num_rows + 1 and feat.is_cuda and feat.dim() in (2, 3), tuple(feat.shape)
    scale = _finite(scale)
    one_d = feat.dim() == 2
    if one_d:
        assert scores.dim() == 1, tuple(scores.shape)
        feat = feat.unsqueeze(1)
    else:
        assert scores.dim() == 2 and scores.shape[1] == feat.shape[1], (tuple(scores.shape), tuple(feat.shape))
    if feat.dtype not in FEATURE_TYPES:
        feat = feat.float()
    heads, head_dim = feat.shape[1], feat.shape[2]
    assert heads >= 1
    scores = _scores(scores, indices.numel(), heads)
    mask, keep_scale = _mask(mask, keep_scale, indices.numel(), heads, feat.device)
    width = piece_width(max(head_dim, 1), feat.dtype)
    out = torch.empty((num_rows, heads, width), dtype=torch.float32, device=feat.device)
    m = torch.empty((num_rows, heads), dtype=torch.float32, device=feat.device)
    l = torch.empty((num_rows, heads), dtype=torch.float32, device=feat.device)
    if num_rows > 0:
        if mask is None:
            capi.launch_attn_aggregate_csr(indptr.contiguous(), indices.contiguous(), scores, num_rows, padded_last_dim(feat, width), scale,
                                           out, m, l, _raw_stream(feat.device))
        else:
            capi.launch_attn_aggregate_csr(indptr.contiguous(), indices.contiguous(), scores, num_rows, padded_last_dim(feat, width), scale,
                                           out, m, l, _raw_stream(feat.device), mask, keep_scale)
    if width != head_dim:
        out = out[:, :, :head_dim].contiguous()
    if one_d:
        out, m, l = out.view(num_rows, head_dim), m.view(num_rows), l.view(num_rows)
    return (out, m, l) if return_stats else out


def attn_aggregate_grad_scores(indptr: torch.Tensor, indices: torch.Tensor, grad_out: torch.Tensor, feat: torch.Tensor,
                               scores: torch.Tensor, m: torch.Tensor, l: torch.Tensor, delta: torch.Tensor,
                               scale: float = 1.0, mask: torch.Tensor = None, keep_scale: float = 1.0) -> torch.Tensor:
    """The gradient of ``attn_aggregate`` for its scores: ``scale * alpha[e, h] * (<grad_out[row_e, h], feat[indices[e], h]> -
    delta[row_e, h])`` -> float32 [nnz, H] (2-D form: [nnz]), with ``alpha`` recomputed from ``scores`` and the forward's ``m``, ``l``.
    ``delta`` [num_rows, H] is ``(grad_out * out).sum(-1)`` of the forward's ``out``.  ``grad_out`` [num_rows, H, D] (cast to float32),
    ``feat`` as in the forward.  One launch split by edges; a row or head with ``l == 0`` gets zeros.  With ``mask`` / ``keep_scale`` of
    the forward: ``scale * alpha * (k * dot - delta)``, a dropped entry's dot is +0 and its row of ``feat`` is not read."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    assert indptr.is_cuda and indices.is_cuda and indptr.dtype == torch.int32 and indices.dtype == torch.int32
    assert feat.is_cuda and grad_out.is_cuda and feat.dim() in (2, 3) and grad_out.dim() == feat.dim()
    scale = _finite(scale)
    one_d = feat.dim() == 2
    if one_d:
        feat, grad_out = feat.unsqueeze(1), grad_out.unsqueeze(1)
    if feat.dtype not in FEATURE_TYPES:
        feat = feat.float()
    num_rows, nnz = indptr.numel() - 1, indices.numel()
    heads, head_dim = feat.shape[1], feat.shape[2]
    assert grad_out.shape == (num_rows, heads, head_dim), (tuple(grad_out.shape), num_rows, heads, head_dim)
    scores = _scores(scores, nnz, heads)
    m, l, delta = (t.float().contiguous().view(num_rows, heads) for t in (m, l, delta))
    mask, keep_scale = _mask(mask, keep_scale, nnz, heads, feat.device)
    out = torch.empty((nnz, heads), dtype=torch.float32, device=feat.device)
    if nnz > 0 and head_dim == 0:
        out.zero_()
    elif nnz > 0:
        width = piece_width(max(head_dim, 1), feat.dtype)
        extra = () if mask is None else (mask, keep_scale)
        capi.launch_attn_aggregate_grad_scores_csr(indptr.contiguous(), indices.contiguous(), num_rows,
                                                   padded_last_dim(grad_out.float(), width), padded_last_dim(feat, width), scores, m, l, delta,
                                                   scale, out, _raw_stream(feat.device), *extra)
    return out.view(-1) if one_d else out


def attn_aggregate_grad_feat(t_indptr: torch.Tensor, t_indices: torch.Tensor, t_order: torch.Tensor, grad_out: torch.Tensor,
                             scores: torch.Tensor, m: torch.Tensor, l: torch.Tensor, num_cols: int, scale: float = 1.0,
                             mask: torch.Tensor = None, keep_scale: float = 1.0) -> torch.Tensor:
    """The gradient of ``attn_aggregate`` for ``feat``: ``sum_{e in column c} alpha[t_order[e], h] * grad_out[row_e, h, :]`` -> float32
    [num_cols, H, D] (2-D form: [num_cols, D]), every row written.  ``t_indptr`` / ``t_indices``: the transposed device CSR
    (``voltrix.autograd.csr_transpose_device``); ``t_order``: device [nnz], the entry of the CSR that entry ``e`` of the transpose is
    (``weighted.transpose_order``; kept as int32).  ``scores`` stays in CSR order and ``grad_out`` [num_rows, H, D] (fp32 / fp16 / bf16 as
    it is) is never permuted; ``m``, ``l``: the forward's.  A row per lane group: a hub column serialises its wave.  With ``mask`` /
    ``keep_scale`` of the forward (the mask stays in CSR order and is read at ``t_order[e]``) the weight is ``alpha * k`` and a dropped
    entry's row of ``grad_out`` is not read."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    assert t_indptr.is_cuda and t_indices.is_cuda and t_indptr.dtype == torch.int32 and t_indices.dtype == torch.int32
    assert t_indptr.numel() == num_cols + 1 and grad_out.is_cuda and grad_out.dim() in (2, 3)
    scale = _finite(scale)
    one_d = grad_out.dim() == 2
    if one_d:
        grad_out = grad_out.unsqueeze(1)
    if grad_out.dtype not in FEATURE_TYPES:
        grad_out = grad_out.float()
    nnz = t_indices.numel()
    num_rows, heads, head_dim = grad_out.shape
    assert t_order.is_cuda and t_order.numel() == nnz
    t_order = t_order.to(torch.int32).contiguous()
    scores = _scores(scores, nnz, heads)
    m, l = (t.float().contiguous().view(num_rows, heads) for t in (m, l))
    mask, keep_scale = _mask(mask, keep_scale, nnz, heads, grad_out.device)
    width = piece_width(max(head_dim, 1), grad_out.dtype)
    out = torch.empty((num_cols, heads, width), dtype=torch.float32, device=grad_out.device)
    if num_cols > 0:
        extra = () if mask is None else (mask, keep_scale)
        capi.launch_attn_aggregate_grad_feat_csr(t_indptr.contiguous(), t_indices.contiguous(), t_order, num_cols,
                                                 padded_last_dim(grad_out, width), scores, m, l, scale, out, _raw_stream(grad_out.device),
                                                 *extra)
    if width != head_dim:
        out = out[:, :, :head_dim].contiguous()
    return out.view(num_cols, head_dim) if one_d else out


# ``voltrix.attn_aggregate`` is the function (voltrix/__init__.py); the two backward pieces stay reachable through it
attn_aggregate.attn_aggregate_grad_scores = attn_aggregate_grad_scores
attn_aggregate.attn_aggregate_grad_feat = attn_aggregate_grad_feat
