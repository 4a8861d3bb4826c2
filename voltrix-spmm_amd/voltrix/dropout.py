"""Attention dropout: the packed keep mask and what uses it outside the fused operator.

The mask is int32 ``[nnz, W]`` with ``W = ceil(H / 32)`` in CSR edge order: bit ``h & 31`` of word ``h >> 5`` of edge ``e`` set means that
``(e, h)`` is kept.  One bit per edge and head -- 32 times less than the attention weights it acts on, and nothing else is saved for the
backward.  ``dropout_mask`` writes it with a counter-based generator (voltrix/dropout_mask_kernels.hpp): ``(e, h)`` is kept iff word
``h & 3`` of ``Philox4x32-10(counter = (e, h >> 2, offset & 0xffffffff, offset >> 32), key = (seed & 0xffffffff, seed >> 32))`` is
``>= T`` with ``T = min(2**32 - 1, floor(p * 2**32))``: a function of ``(seed, offset, e, h)`` and nothing else, so a mask can be
replayed, inspected, or built by the caller (DropEdge is the same bit on every head).  ``voltrix.attn_aggregate(..., mask=, keep_scale=)``
and ``voltrix.autograd.AttnAggregate`` read it inside the kernels; ``apply_dropout_mask`` is the plain torch form for the unfused chain
``spmm_heads(apply_dropout_mask(edge_softmax(s, scale), mask, keep_scale), feat)``.  No reference counterpart.
"""
from __future__ import annotations

import torch


def mask_words(heads: int) -> int:
    return (int(heads) + 31) // 32


def drop_threshold(p: float) -> int:
    """``T = min(2**32 - 1, floor(p * 2**32))`` in double: an entry is kept iff its 32 random bits are ``>= T``."""
    p = float(p)
    if not 0.0 <= p < 1.0:            # NaN fails both comparisons
        raise ValueError(f"dropout: p must satisfy 0 <= p < 1, got {p}")
    return min(2 ** 32 - 1, int(p * 4294967296.0))


def dropout_mask(nnz: int, heads: int, p: float, seed: int, offset: int = 0, device=None) -> torch.Tensor:
    """The keep mask int32 ``[nnz, ceil(heads / 32)]`` of drop probability ``p`` (module docstring) on ``device`` (default: the current
    CUDA device), on the current stream; bits past ``heads`` are zero, ``p = 0`` sets every bit.  ``0 <= p < 1`` and
    ``0 <= seed, offset < 2**64``, anything else is a ``ValueError`` before any launch.  One launch, nothing read back."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    nnz, heads, seed, offset = int(nnz), int(heads), int(seed), int(offset)
    threshold = drop_threshold(p)
    if nnz < 0 or nnz >= 2 ** 31 or heads < 1:
        raise ValueError(f"dropout_mask: nnz must lie in [0, 2**31) and heads be positive, got {nnz}, {heads}")
    if not (0 <= seed < 2 ** 64 and 0 <= offset < 2 ** 64):
        raise ValueError(f"dropout_mask: seed and offset must lie in [0, 2**64), got {seed}, {offset}")
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    mask = torch.empty((nnz, mask_words(heads)), dtype=torch.int32, device=device)
    if nnz > 0:
        capi.launch_dropout_mask(nnz, heads, threshold, seed, offset, mask, _raw_stream(device))
    return mask


def check_mask(mask: torch.Tensor, nnz: int, heads: int, device) -> torch.Tensor:
    """``mask`` validated (int32 ``[nnz, ceil(heads / 32)]`` on ``device``; ``ValueError`` otherwise) and contiguous."""
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.int32:
        raise ValueError(f"dropout mask: expected an int32 tensor, got {getattr(mask, 'dtype', type(mask))}")
    if tuple(mask.shape) != (nnz, mask_words(heads)):
        raise ValueError(f"dropout mask: expected shape {(nnz, mask_words(heads))} for {nnz} edges and {heads} heads, got "
                         f"{tuple(mask.shape)}")
    if mask.device != device:
        raise ValueError(f"dropout mask: on {mask.device}, the operands on {device}")
    return mask.contiguous()


def check_keep_scale(keep_scale) -> float:
    keep_scale = float(keep_scale)
    if not (0.0 <= keep_scale < float("inf")):
        raise ValueError(f"dropout: keep_scale must be finite and not negative, got {keep_scale}")
    return keep_scale


def unpack_mask(mask: torch.Tensor, heads: int) -> torch.Tensor:
    """bool ``[nnz, heads]`` from the packed mask."""
    h = torch.arange(heads, device=mask.device)
    return ((mask[:, h >> 5] >> (h & 31)) & 1).bool()


def apply_dropout_mask(alpha: torch.Tensor, mask: torch.Tensor, keep_scale: float) -> torch.Tensor:
    """``alpha * keep_scale`` where the mask keeps and 0 elsewhere (a selection, not a product with 0): ``alpha`` ``[nnz, H]`` or
    ``[nnz]`` (one head), ``mask`` int32 ``[nnz, ceil(H / 32)]``.  Plain torch and differentiable in ``alpha``: the dropout step of the
    unfused chain, which has to store ``alpha`` anyway."""
    heads = 1 if alpha.dim() == 1 else alpha.shape[1]
    mask = check_mask(mask, alpha.shape[0], heads, alpha.device)
    keep = unpack_mask(mask, heads).view(alpha.shape)
    return torch.where(keep, alpha * check_keep_scale(keep_scale), torch.zeros((), dtype=alpha.dtype, device=alpha.device))
