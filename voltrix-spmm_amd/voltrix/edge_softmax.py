"""Edge softmax: the softmax of per-edge scores over every row of a CSR pattern -- the step of an attention layer between the scores
(``voltrix.sddmm``) and the aggregation with them (``autograd.SpMM(...)(feat, values=alpha)``).

No reference counterpart -- the reference is forward-only and has no edge values.  Three HIP launches (voltrix/edge_softmax_kernels.hpp)
split the work by edges, so hub rows cost what their edges cost; nothing is read back on the host, so the call can be captured in a graph.

    alpha = voltrix.edge_softmax(indptr, scores, scale=d ** -0.5)      # float32 [nnz], CSR order

    alpha[e] = exp(z_e - m_r) / sum_{e' in row r} exp(z_e' - m_r),   z = scale * scores,  m_r = the row maximum

Special values: ``z = -inf`` gives 0, and a row whose entries are all ``-inf`` gets zeros -- unlike ``torch.softmax``, which gives NaN: a
fully masked row is normal in attention.  A NaN makes its own row NaN and no other.  Numerics: with ``deg_r`` the row's entries and ``ref``
the exact softmax, ``|alpha - ref| <= ref * 2 (deg_r + |z_e - m_r| + 2) 2^-23 + 2^-126``; sums run in an order fixed by the pattern, so the
same inputs give the same bits on every call (no float atomics).  The backward, ``scale * alpha * (g - rowsum(alpha * g))``, is within
``|scale| alpha_e (2 |g_e - D_r| + (deg_r + 2) A_r) 2^-23 + 2^-126`` (``D_r = rowsum(alpha g)``, ``A_r = rowsum(alpha |g|)``).
"""
from __future__ import annotations

import torch


def workspace_bytes(num_rows: int, nnz: int, heads: int = 1) -> int:
    """Bytes of device workspace one call allocates (from torch's allocator, on the current stream); a function of ``nnz`` and
    ``heads`` alone."""
    from . import capi

    if heads == 1:
        return capi.edge_softmax_workspace_bytes(num_rows, nnz)
    return capi.edge_softmax_heads_workspace_bytes(num_rows, nnz, heads)


def _workspace(num_rows: int, nnz: int, device, heads: int = 1) -> torch.Tensor:
    return torch.empty(workspace_bytes(num_rows, nnz, heads), dtype=torch.uint8, device=device)


def edge_softmax(indptr: torch.Tensor, scores: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """Softmax of ``scale * scores`` over every row -> float32 [nnz] in CSR order, on the current stream.

    Multi-head: ``scores`` [nnz, H] (head index fastest) -> [nnz, H], every column its own softmax, special values per head
    (voltrix/edge_softmax_heads_kernels.hpp); ``out[:, h]`` has the bits of the 1-D call on ``scores[:, h]``.
    ``indptr``: device int32 [num_rows + 1] (a valid CSR whose last entry is ``scores.numel()``); ``scores``: CUDA [nnz] in CSR order,
    cast to float32 if it is another type; ``scale``: a finite float (``d ** -0.5`` for dot-product attention costs no extra pass;
    0 gives every entry that is not ``-inf`` 1 / its row's such entries, a mean)."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    assert indptr.is_cuda and indptr.dtype == torch.int32 and scores.is_cuda and scores.dim() in (1, 2)
    num_rows = indptr.numel() - 1
    scores = scores.float().contiguous()
    if scores.dim() == 2:
        nnz, heads = scores.shape
        assert heads >= 1
        if heads == 1:                      # one column is the 1-D layout: the single-head kernels (vector loads), the same bits
            return edge_softmax(indptr, scores.view(-1), scale).view(nnz, 1)
        out = torch.empty_like(scores)
        if nnz == 0:
            return out
        capi.launch_edge_softmax_heads_csr(indptr.contiguous(), num_rows, scores, float(scale), out,
                                           _workspace(num_rows, nnz, scores.device, heads), _raw_stream(scores.device))
        return out
    nnz = scores.numel()
    out = torch.empty(nnz, dtype=torch.float32, device=scores.device)
    if nnz == 0:
        return out
    capi.launch_edge_softmax_csr(indptr.contiguous(), num_rows, scores, float(scale), out, _workspace(num_rows, nnz, scores.device),
                                 _raw_stream(scores.device))
    return out


def edge_softmax_backward(indptr: torch.Tensor, alpha: torch.Tensor, grad_alpha: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """Gradient of ``edge_softmax`` with respect to its scores: ``scale * alpha * (grad_alpha - rowsum(alpha * grad_alpha))`` -> float32
    [nnz]; ``alpha`` is the forward's output.  Rows of zeros (all ``-inf`` scores) get zero gradients.  [nnz, H] tensors: per head."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    assert indptr.is_cuda and indptr.dtype == torch.int32 and alpha.is_cuda and alpha.shape == grad_alpha.shape
    num_rows = indptr.numel() - 1
    alpha = alpha.float().contiguous()
    grad_alpha = grad_alpha.float().contiguous()
    if alpha.dim() == 2:
        nnz, heads = alpha.shape
        assert heads >= 1
        if heads == 1:
            return edge_softmax_backward(indptr, alpha.view(-1), grad_alpha.view(-1), scale).view(nnz, 1)
        out = torch.empty_like(alpha)
        if nnz == 0:
            return out
        capi.launch_edge_softmax_heads_backward_csr(indptr.contiguous(), num_rows, alpha, grad_alpha, float(scale), out,
                                                    _workspace(num_rows, nnz, alpha.device, heads), _raw_stream(alpha.device))
        return out
    nnz = alpha.numel()
    out = torch.empty(nnz, dtype=torch.float32, device=alpha.device)
    if nnz == 0:
        return out
    capi.launch_edge_softmax_backward_csr(indptr.contiguous(), num_rows, alpha, grad_alpha, float(scale), out,
                                          _workspace(num_rows, nnz, alpha.device), _raw_stream(alpha.device))
    return out
