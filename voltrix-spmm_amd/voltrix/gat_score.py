"""GAT edge scores: ``s[e] = leaky_relu(el[row_e] + er[col_e], slope)`` for every entry of a CSR pattern -- the first step of a GAT
layer, before ``voltrix.edge_softmax`` -- and the two segment sums of its backward.

No reference counterpart -- the reference is forward-only and has no edge values.  The HIP kernels (voltrix/gat_score_kernels.hpp) split
the work by edges, read one 4-byte column id per edge (no int64 row / column id tensors) and use no float atomics: the same inputs give
the same bits on every call, forward and backward.  Nothing is read back on the host, so the calls can be captured in a graph.

    s = voltrix.gat_score(indptr, indices, el, er, slope=0.2)         # float32 [nnz] (or [nnz, H]), CSR order
    d_el = gat_score_backward(indptr, indices, el, er, g, slope)      # sum over every row of gate * g
    d_er = gat_score_backward(t_indptr, t_indices, er, el, g, slope, order=t_order)       # the same on the transposed CSR

``z = el[row] + er[col]`` is one fp32 add; ``z > 0`` gives ``z``, anything else ``float32(slope) * z`` (``z == 0`` takes the slope branch,
as ``torch.nn.functional.leaky_relu``).  ``slope`` is any finite float: 1 is the plain sum, 0 is ReLU.  Numerics, against float64 from the
float32 inputs: ``|s - ref| <= 1.5 * 2^-23 |ref| + 2^-149`` (``2^-24 |ref| + 2^-149`` when ``slope`` is 1 or a power of two); a segment
sum over ``deg`` entries is within ``deg * 2^-23 * sum |gate * g| + 2^-149``.  Multi-head: ``el`` [num_rows, H], ``er`` [num_cols, H],
edge tensors [nnz, H] with the head index fastest; ``out[:, h]`` has the bits of the 1-D call on the contiguous slices.
"""
from __future__ import annotations

import torch


def workspace_bytes(num_rows: int, nnz: int, heads: int = 1) -> int:
    """Bytes of device workspace one ``gat_score_backward`` call allocates (from torch's allocator, on the current stream); a function
    of ``nnz`` and ``heads`` alone.  The forward needs none."""
    from . import capi

    return capi.gat_score_workspace_bytes(num_rows, nnz, heads)


def _node_scalars(t: torch.Tensor, name: str) -> torch.Tensor:
    assert t.is_cuda and t.dim() in (1, 2), name
    t = t.float().contiguous()
    return t.view(-1, 1) if t.dim() == 1 else t


def gat_score(indptr: torch.Tensor, indices: torch.Tensor, el: torch.Tensor, er: torch.Tensor, slope: float = 0.2) -> torch.Tensor:
    """``leaky_relu(el[row_e] + er[indices[e]], slope)`` for every entry -> float32 [nnz] in CSR order, on the current stream.

    ``indptr`` / ``indices``: device int32 CSR ([num_rows + 1], [nnz]; duplicates are edges of their own); ``el``: CUDA [num_rows],
    ``er``: CUDA [num_cols], cast to float32 if they are another type; ``slope``: a finite float.  Multi-head: ``el`` [num_rows, H] and
    ``er`` [num_cols, H] -> [nnz, H]."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    assert indptr.is_cuda and indptr.dtype == torch.int32 and indices.is_cuda and indices.dtype == torch.int32
    assert el.dim() == er.dim() and el.shape[1:] == er.shape[1:]
    one_d = el.dim() == 1
    num_rows, nnz = indptr.numel() - 1, indices.numel()
    el, er = _node_scalars(el, "el"), _node_scalars(er, "er")       # 1-D is the [n, 1] layout: the same kernel, the same bits
    assert el.shape[0] == num_rows and el.shape[1] >= 1
    out = torch.empty((nnz, el.shape[1]), dtype=torch.float32, device=el.device)
    if nnz > 0:
        capi.launch_gat_score_csr(indptr.contiguous(), indices.contiguous(), num_rows, el, er, float(slope), out, _raw_stream(el.device))
    return out.view(-1) if one_d else out


def gat_score_backward(indptr: torch.Tensor, indices: torch.Tensor, a: torch.Tensor, b: torch.Tensor, grad: torch.Tensor, slope: float,
                       order: torch.Tensor = None) -> torch.Tensor:
    """One segment sum of the backward: ``out[r] = sum_{e in row r} gate(a[r] + b[indices[e]]) * grad[order[e] if order else e]`` with
    ``gate(z) = 1 if z > 0 else slope`` -> float32 [num_rows] (or [num_rows, H]); every element is written, empty rows are 0.

    ``d_el``: the CSR, ``(a, b) = (el, er)``.  ``d_er``: the transposed CSR (``voltrix.autograd.csr_transpose_device``), ``(a, b) =
    (er, el)`` and ``order`` = device int32 [nnz], the entry of the CSR that entry ``e`` of the transpose is
    (``weighted.transpose_order``) -- ``grad`` stays in CSR order and is never permuted."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    assert indptr.is_cuda and indptr.dtype == torch.int32 and indices.is_cuda and indices.dtype == torch.int32
    assert a.dim() == b.dim() == grad.dim() and a.shape[1:] == b.shape[1:] == grad.shape[1:] and grad.is_cuda
    one_d = a.dim() == 1
    num_rows, nnz = indptr.numel() - 1, indices.numel()
    a, b = _node_scalars(a, "a"), _node_scalars(b, "b")
    grad = grad.float().contiguous()
    grad = grad.view(-1, 1) if one_d else grad
    heads = a.shape[1]
    assert a.shape[0] == num_rows and grad.shape == (nnz, heads) and heads >= 1
    if order is not None:
        assert order.is_cuda and order.numel() == nnz
        order = order.to(torch.int32).contiguous()
    out = torch.empty((num_rows, heads), dtype=torch.float32, device=a.device)
    if num_rows > 0:
        workspace = torch.empty(workspace_bytes(num_rows, nnz, heads), dtype=torch.uint8, device=a.device)
        capi.launch_gat_score_rowsum_csr(indptr.contiguous(), indices.contiguous(), order, num_rows, a, b, grad, float(slope), out,
                                         workspace, _raw_stream(a.device))
    return out.view(-1) if one_d else out
