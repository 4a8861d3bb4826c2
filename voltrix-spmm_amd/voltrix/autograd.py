"""Backward pass of the SpMM: ``dB = A^T @ dC`` through a transposed handle.

No reference counterpart -- the reference is forward-only (voltrix/jit_kernels/spmm.py:53-54 asserts a plain float
input and nothing registers a gradient), which is what keeps it out of GCN *training* loops.  ``A`` is binary, so the
gradient with respect to the dense operand of ``C = A @ B`` is the SpMM of the transposed adjacency with the incoming
gradient; the same kernels run it on a second handle built from the transposed CSR (one device-side sort by column).

    op = voltrix.autograd.SpMM(indptr, indices, num_nodes)        # CPU or CUDA int32 CSR; builds A and A^T handles
    out = op(feat)                                                # float32 [num_nodes, F]; feat.requires_grad honoured
    out.sum().backward()                                          # feat.grad = A^T @ 1

The forward keeps ``voltrix.spmm``'s numerics (fp16 / bf16 operand or scaled-fp16 rounding of an fp32 operand, fp32
accumulate); the backward treats the incoming gradient the same way, i.e. the pair is the exact adjoint up to the
operand rounding the forward applies too.

Edge values that are learnt (attention coefficients, edge gates) get a gradient too.  What flows where:

    op = voltrix.autograd.SpMM(indptr, indices, num_nodes, values=v0)   # built with values
    out = op(feat, values=v)              # csr(v) @ feat; feat.grad = csr(v)^T @ dC, v.grad[e] = <dC[row_e], feat[col_e]>
    s = voltrix.autograd.SDDMM(indptr, indices, num_nodes)(q, k)     # s[e] = <q[row_e], k[col_e]>
                                          # q.grad = csr(ds) @ k, k.grad = csr(ds)^T @ q
    alpha = voltrix.autograd.EdgeSoftmax(indptr, num_nodes)(s, scale)  # softmax of scale * s over every row
                                          # s.grad = scale * alpha * (dalpha - rowsum(alpha * dalpha))

``v.grad`` and both SDDMM forwards are the sampled dense-dense product (``voltrix.sddmm``: fp32 products and sum, within
``F 2^-23 (|x| |y|)[e]``); the SDDMM's backward is the CSR row-gather kernel with values on the CSR and on its transpose.  The edge
softmax's forward and backward are the kernels of ``voltrix.edge_softmax`` (three launches each, deterministic); together the three
operators make an attention layer: ``SpMM(...)(v, values=EdgeSoftmax(...)(SDDMM(...)(q, k), d ** -0.5))``.

GAT's scores are ``voltrix.autograd.GATScore(indptr, indices, n)(el, er, slope)``: ``leaky_relu(el[row] + er[col])`` per edge, with
``el.grad`` / ``er.grad`` as deterministic segment sums over the rows / the columns (``voltrix.gat_score``; [n] or [n, H] scalars).
GATv2's are ``voltrix.autograd.GATv2Score(indptr, indices, n)(xl, xr, a, slope)``: ``sum_d a[h, d] leaky_relu(xl[row, h, d] + xr[col, h, d])``
with ``xl.grad = a G_l``, ``xr.grad = a G_r``, ``a.grad = sum xl G_l + sum xr G_r`` from two gated row sums [n, H, D]
(``voltrix.gatv2_score``); nothing of size [nnz, H, D] exists in either direction.

Multi-head: ``SDDMM`` takes ``q, k`` [n, H, D] and gives scores [nnz, H], ``EdgeSoftmax`` takes [nnz, H], and ``SpMMHeads`` aggregates
``v`` [n, H, D] with weights [nnz, H] -- one launch per operator for all heads, the per-head bits of the single-head kernels:

    alpha = EdgeSoftmax(indptr, n)(SDDMM(indptr, indices, n)(q, k), d ** -0.5)       # [nnz, H]
    out = voltrix.autograd.SpMMHeads(indptr, indices, n)(v, alpha)                   # float32 [n, H, D]

``AttnAggregate`` is the last two steps in one operator, ``AttnAggregate(indptr, indices, n)(v, s, scale)`` ==
``SpMMHeads(...)(v, EdgeSoftmax(...)(s, scale))``: one launch forward, ``alpha`` recomputed in the backward from two numbers per row
and head instead of being stored (``voltrix.attn_aggregate``).
"""
from __future__ import annotations

import torch

from .spmm.spmm import csr_preprocess_device, spmm


def csr_transpose_device(indptr: torch.Tensor, indices: torch.Tensor, num_rows: int, num_cols: int):
    """CSR of ``A^T`` ([num_cols, num_rows]) for a device CSR of ``A`` ([num_rows, num_cols]): int32, rows sorted,
    duplicates kept (they count once in the block format, like everywhere else)."""
    assert indptr.is_cuda and indices.is_cuda and indptr.dtype == torch.int32 and indices.dtype == torch.int32
    from . import capi

    # row ids expanded per entry + one stable radix sort by column + row pointers by binary search (reorder_kernels.hpp;
    # round 2 sorted 64-bit (col, row) keys with torch ops)
    return capi.csr_transpose(indptr.contiguous(), indices.contiguous(), num_rows, num_cols)


class _SpMMFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, op):
        ctx.op = op
        ctx.in_dtype = feat.dtype
        if op.weighted is not None:
            from .weighted import spmm_weighted

            return spmm_weighted(op.weighted, feat)
        return spmm(*op.handle, num_nodes=op.num_rows, num_edges=op.num_edges, feat=feat)

    @staticmethod
    def backward(ctx, grad_out):
        op = ctx.op
        if op.weighted is not None:
            from .weighted import spmm_weighted

            return spmm_weighted(op.weighted_t, grad_out.contiguous()).to(ctx.in_dtype), None
        grad = spmm(*op.handle_t, num_nodes=op.num_cols, num_edges=op.num_edges, feat=grad_out.contiguous())
        return grad.to(ctx.in_dtype), None


class _SpMMValuesFunction(torch.autograd.Function):
    """``csr(values) @ feat`` with gradients for ``feat`` and ``values``; ``op`` holds the pattern and the installed values."""

    @staticmethod
    def forward(ctx, feat, values, op):
        from .weighted import spmm_weighted

        op._install(values.detach())
        ctx.op, ctx.install = op, op._installs
        ctx.save_for_backward(feat, values)
        return spmm_weighted(op.weighted, feat)

    @staticmethod
    def backward(ctx, grad_out):
        from .sddmm import sddmm
        from .weighted import spmm_weighted

        op = ctx.op
        feat, values = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        grad_feat = grad_values = None
        if ctx.needs_input_grad[0]:
            if op._installs != ctx.install:         # a later forward installed other values: put this forward's back
                op._install(values.detach())
            grad_feat = spmm_weighted(op.weighted_t, grad_out).to(feat.dtype)
        if ctx.needs_input_grad[1]:
            grad_values = sddmm(op.weighted.csr[0], op.weighted.csr[1], grad_out, feat).to(values.dtype)
        return grad_feat, grad_values, None


class CsrPattern:
    """A CSR pattern [num_rows, num_cols] (``num_cols`` defaults to ``num_rows``) as the attention operators hold it, built once and
    shared: the device int32 ``indptr`` / ``indices``, ``num_rows`` / ``num_cols`` / ``num_edges``, the transposed CSR ``t_indptr`` /
    ``t_indices`` (``csr_transpose_device``) and ``t_order``, int32 [nnz]: entry ``e`` of the transpose is entry ``t_order[e]`` of the
    CSR (``weighted.transpose_order``).  Everything is built in the constructor.  ``transposed=(t_indptr, t_indices, t_order)`` takes a
    transpose that exists already (any integer type for the order)."""

    def __init__(self, indptr: torch.Tensor, indices: torch.Tensor, num_rows: int, num_cols: int = None, transposed=None):
        assert indptr.dtype == torch.int32 and indices.dtype == torch.int32 and indptr.numel() == num_rows + 1
        self.num_rows = num_rows
        self.num_cols = num_rows if num_cols is None else int(num_cols)
        self.num_edges = int(indices.numel())
        self.indptr, self.indices = indptr.contiguous().cuda(), indices.contiguous().cuda()
        if transposed is None:
            from .weighted import transpose_order

            t_indptr, t_indices = csr_transpose_device(self.indptr, self.indices, num_rows, self.num_cols)
            t_order = transpose_order(self.indptr, self.indices, num_rows)
        else:
            t_indptr, t_indices, t_order = transposed
            assert t_indptr.numel() == self.num_cols + 1 and t_indices.numel() == self.num_edges == t_order.numel()
        self.t_indptr, self.t_indices, self.t_order = t_indptr, t_indices, t_order.to(torch.int32).contiguous()


class _PatternOp:
    """What ``SDDMM``, ``SpMMHeads``, ``GATScore``, ``GATv2Score`` and ``AttnAggregate`` share: ``Op(indptr, indices, num_rows,
    num_cols=None, transposed=None)`` builds a ``CsrPattern`` of its own, ``Op(pattern)`` takes one that exists -- nothing is copied or
    built again, so one graph is transposed once for all its operators.  The pattern's fields read through under their names."""

    def __init__(self, indptr, indices: torch.Tensor = None, num_rows: int = None, num_cols: int = None, transposed=None):
        if isinstance(indptr, CsrPattern):
            assert indices is None and num_rows is None and num_cols is None and transposed is None
            self.pattern = indptr
        else:
            self.pattern = CsrPattern(indptr, indices, num_rows, num_cols, transposed)

    indptr = property(lambda self: self.pattern.indptr)
    indices = property(lambda self: self.pattern.indices)
    t_indptr = property(lambda self: self.pattern.t_indptr)
    t_indices = property(lambda self: self.pattern.t_indices)
    t_order = property(lambda self: self.pattern.t_order)
    num_rows = property(lambda self: self.pattern.num_rows)
    num_cols = property(lambda self: self.pattern.num_cols)
    num_edges = property(lambda self: self.pattern.num_edges)


class _SDDMMFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, op):
        from .sddmm import sddmm

        ctx.op = op
        ctx.save_for_backward(x, y)
        return sddmm(op.indptr, op.indices, x, y)

    @staticmethod
    def backward(ctx, grad_out):
        from .sddmm import csr_values_product

        op = ctx.op
        x, y = ctx.saved_tensors
        g = grad_out.float().contiguous()
        grad_x = grad_y = None
        if x.dim() == 3:                      # multi-head: g [nnz, H]; the aggregation kernel on the CSR and on its transpose
            from .sddmm import spmm_heads

            if ctx.needs_input_grad[0]:
                grad_x = spmm_heads(op.indptr, op.indices, g, y, op.num_rows).to(x.dtype)
            if ctx.needs_input_grad[1]:
                grad_y = spmm_heads(op.t_indptr, op.t_indices, g[op.t_order], x, op.num_cols).to(y.dtype)
            return grad_x, grad_y, None
        if ctx.needs_input_grad[0]:           # csr(g) @ y
            grad_x = csr_values_product(op.indptr, op.indices, g, op.num_rows, y).to(x.dtype)
        if ctx.needs_input_grad[1]:           # csr(g)^T @ x: the transposed CSR, g in its edge order
            grad_y = csr_values_product(op.t_indptr, op.t_indices, g[op.t_order], op.num_cols, x).to(y.dtype)
        return grad_x, grad_y, None


class SDDMM(_PatternOp):
    """``s[e] = <x[row_e], y[col_e]>`` for every entry of a CSR pattern [num_rows, num_cols] (``num_cols`` defaults to ``num_rows``),
    differentiable in both operands: attention scores ``SDDMM(...)(q, k)``.  Built once per pattern: the device CSR, its transpose
    (``csr_transpose_device``) and the transposed edge order (``weighted.transpose_order``, kept as int32) -- or ``SDDMM(pattern)`` on a
    ``CsrPattern`` shared with the other operators of the graph.  Gradients come back in the operands' dtypes.  Multi-head: ``x`` [num_rows, H, D], ``y`` [num_cols, H, D] -> ``s`` [nnz, H]; the backward is ``voltrix.spmm_heads``."""

    def __call__(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        assert x.dim() in (2, 3) and x.dim() == y.dim()
        assert x.shape[0] == self.num_rows and y.shape[0] == self.num_cols and x.shape[1:] == y.shape[1:]
        return _SDDMMFunction.apply(x, y, self)


class _EdgeSoftmaxFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, op, scale):
        from .edge_softmax import edge_softmax

        alpha = edge_softmax(op.indptr, scores, scale)
        ctx.op, ctx.scale, ctx.in_dtype = op, scale, scores.dtype
        ctx.save_for_backward(alpha)
        return alpha

    @staticmethod
    def backward(ctx, grad_alpha):
        from .edge_softmax import edge_softmax_backward

        (alpha,) = ctx.saved_tensors
        grad = edge_softmax_backward(ctx.op.indptr, alpha, grad_alpha, ctx.scale)
        return grad.to(ctx.in_dtype), None, None


class EdgeSoftmax:
    """``alpha = softmax(scale * scores)`` over every row of a CSR pattern with ``num_rows`` rows (``voltrix.edge_softmax``), differentiable
    in the scores: the attention weights between ``SDDMM`` and ``SpMM(..., values=)``.  Holds the device ``indptr``; the column ids do not
    matter.  ``alpha`` is float32; the gradient comes back in the scores' dtype.  ``scores`` [nnz] or, multi-head, [nnz, H]."""

    def __init__(self, indptr, num_rows: int = None):
        if isinstance(indptr, CsrPattern):
            indptr, num_rows = indptr.indptr, indptr.num_rows
        assert indptr.dtype == torch.int32 and indptr.numel() == num_rows + 1
        self.num_rows = num_rows
        self.indptr = indptr.contiguous().cuda()

    def __call__(self, scores: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
        assert scores.dim() in (1, 2)
        return _EdgeSoftmaxFunction.apply(scores, self, float(scale))


class _SpMMHeadsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, values, op):
        from .sddmm import spmm_heads

        ctx.op = op
        ctx.save_for_backward(feat, values)
        return spmm_heads(op.indptr, op.indices, values, feat, op.num_rows)

    @staticmethod
    def backward(ctx, grad_out):
        from .sddmm import sddmm, spmm_heads

        op = ctx.op
        feat, values = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        grad_feat = grad_values = None
        if ctx.needs_input_grad[0]:           # csr(values)^T @ dC per head: the transposed CSR, the values in its edge order
            grad_feat = spmm_heads(op.t_indptr, op.t_indices, values.detach()[op.t_order], grad_out, op.num_cols).to(feat.dtype)
        if ctx.needs_input_grad[1]:           # dv[e, h] = <dC[row_e, h], feat[col_e, h]>
            grad_values = sddmm(op.indptr, op.indices, grad_out, feat).to(values.dtype)
        return grad_feat, grad_values, None


class SpMMHeads(_PatternOp):
    """Multi-head aggregation ``out[r, h] = sum_{e in row r} values[e, h] feat[col_e, h]`` on a CSR pattern [num_rows, num_cols]
    (``num_cols`` defaults to ``num_rows``), differentiable in ``feat`` [num_cols, H, D] and ``values`` [nnz, H]: the last step of a
    multi-head attention layer, ``SpMMHeads(...)(v, EdgeSoftmax(...)(SDDMM(...)(q, k), d ** -0.5))``.  Built once per pattern: the
    device CSR, its transpose and the transposed edge order (kept as int32), or ``SpMMHeads(pattern)`` on a shared ``CsrPattern`` -- no
    block-format handle, and nothing is installed per call (``voltrix.spmm_heads`` reads the values where it uses them).  ``out`` is float32 [num_rows, H, D]; ``feat.grad =
    spmm_heads(csr^T, values[t_order], dC)`` and ``values.grad = sddmm(dC, feat)`` come back in the inputs' dtypes."""

    def __call__(self, feat: torch.Tensor, values: torch.Tensor) -> torch.Tensor:
        assert feat.dim() == 3 and values.dim() == 2 and feat.shape[0] == self.num_cols
        assert values.shape == (self.num_edges, feat.shape[1]), (tuple(values.shape), self.num_edges, feat.shape[1])
        return _SpMMHeadsFunction.apply(feat, values, self)


class _GATScoreFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, el, er, op, slope):
        from .gat_score import gat_score

        ctx.op, ctx.slope = op, slope
        ctx.save_for_backward(el, er)
        return gat_score(op.indptr, op.indices, el, er, slope)

    @staticmethod
    def backward(ctx, grad_out):
        from .gat_score import gat_score_backward

        op = ctx.op
        el, er = ctx.saved_tensors
        g = grad_out.float().contiguous()
        grad_el = grad_er = None
        if ctx.needs_input_grad[0]:           # the sum over every row of the CSR
            grad_el = gat_score_backward(op.indptr, op.indices, el.detach(), er.detach(), g, ctx.slope).to(el.dtype)
        if ctx.needs_input_grad[1]:           # the sum over every column: the transposed CSR, g read through its edge order
            grad_er = gat_score_backward(op.t_indptr, op.t_indices, er.detach(), el.detach(), g, ctx.slope, order=op.t_order).to(er.dtype)
        return grad_el, grad_er, None, None


class GATScore(_PatternOp):
    """GAT's edge scores ``s[e] = leaky_relu(el[row_e] + er[col_e], slope)`` on a CSR pattern [num_rows, num_cols] (``num_cols`` defaults
    to ``num_rows``), differentiable in both node scalars: the first step of ``SpMMHeads(...)(wh, EdgeSoftmax(...)(GATScore(...)(el,
    er)))``.  ``el`` [num_rows] or [num_rows, H], ``er`` [num_cols] or [num_cols, H] -> float32 [nnz] or [nnz, H].  Built once per
    pattern: the device CSR, its transpose and the transposed edge order (kept as int32); ``GATScore(pattern)`` takes a ``CsrPattern``
    shared with the other operators of the graph, ``transposed=(t_indptr, t_indices, t_order)`` a transpose that exists already.  The backward is two segment sums
    (``voltrix.gat_score.gat_score_backward``): no index op, no float atomics, the same bits on every run; gradients come back in the
    inputs' dtypes, and a side that needs none is skipped."""

    def __call__(self, el: torch.Tensor, er: torch.Tensor, slope: float = 0.2) -> torch.Tensor:
        assert el.dim() in (1, 2) and el.dim() == er.dim() and el.shape[1:] == er.shape[1:]
        assert el.shape[0] == self.num_rows and er.shape[0] == self.num_cols
        return _GATScoreFunction.apply(el, er, self, float(slope))


class _GATv2ScoreFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xl, xr, a, op, slope):
        from .gatv2_score import gatv2_score

        ctx.op, ctx.slope = op, slope
        ctx.save_for_backward(xl, xr, a)      # never s, never anything [nnz, H, D]
        return gatv2_score(op.indptr, op.indices, xl, xr, a, slope)

    @staticmethod
    def backward(ctx, grad_out):
        from .gatv2_score import gatv2_rowsum

        op = ctx.op
        xl, xr, a = (t.detach() for t in ctx.saved_tensors)
        g = grad_out.float().contiguous()
        need_l, need_r, need_a = ctx.needs_input_grad[:3]
        grad_xl = grad_xr = grad_a = big_l = big_r = None
        if need_l or need_a:                  # G_l: the gated sum over every row of the CSR
            big_l = gatv2_rowsum(op.indptr, op.indices, xl, xr, g, ctx.slope)
        if need_r or need_a:                  # G_r: over every column: the transposed CSR, g read through its edge order
            big_r = gatv2_rowsum(op.t_indptr, op.t_indices, xr, xl, g, ctx.slope, order=op.t_order)
        if need_l:
            grad_xl = (a.float() * big_l).to(xl.dtype)
        if need_r:
            grad_xr = (a.float() * big_r).to(xr.dtype)
        if need_a:                            # leaky_relu(z) = gate(z) z: two dense reductions over the nodes
            grad_a = ((xl.float() * big_l).sum(0) + (xr.float() * big_r).sum(0)).to(a.dtype)
        return grad_xl, grad_xr, grad_a, None, None


class GATv2Score(_PatternOp):
    """GATv2's edge scores ``s[e, h] = sum_d a[h, d] leaky_relu(xl[row_e, h, d] + xr[col_e, h, d], slope)`` on a CSR pattern [num_rows,
    num_cols] (``num_cols`` defaults to ``num_rows``), differentiable in ``xl``, ``xr`` and ``a``: the first step of
    ``SpMMHeads(...)(xr, EdgeSoftmax(...)(GATv2Score(...)(xl, xr, a)))``.  ``xl`` [num_rows, H, D], ``xr`` [num_cols, H, D], ``a`` [H, D]
    -> float32 [nnz, H]; the 2-D form ([n, D], [D] -> [nnz]) is one head.  Built once per pattern, exactly like ``GATScore``: the device
    CSR, its transpose and the transposed edge order (kept as int32), or ``GATv2Score(pattern)`` on a shared ``CsrPattern``, or
    ``transposed=(t_indptr, t_indices, t_order)``.  Saves ``xl``, ``xr``, ``a`` only.  The backward is two gated row sums
    (``voltrix.gatv2_score.gatv2_rowsum``) and dense torch products: ``xl.grad = a G_l``, ``xr.grad = a G_r``, ``a.grad = sum xl G_l +
    sum xr G_r`` -- no index op, no float atomics, nothing of size [nnz, H, D]; gradients come back in the inputs' dtypes, and a side
    nobody needs is skipped."""

    def __call__(self, xl: torch.Tensor, xr: torch.Tensor, a: torch.Tensor, slope: float = 0.2) -> torch.Tensor:
        assert xl.dim() in (2, 3) and xl.dim() == xr.dim() and xl.shape[1:] == xr.shape[1:] == a.shape
        assert xl.shape[0] == self.num_rows and xr.shape[0] == self.num_cols
        return _GATv2ScoreFunction.apply(xl, xr, a, self, float(slope))


class _AttnAggregateFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, scores, op, scale, mask=None, keep_scale=1.0):
        from .attn_aggregate import attn_aggregate

        ctx.op, ctx.scale, ctx.keep_scale, ctx.dropout = op, scale, keep_scale, mask is not None
        if mask is None:
            out, m, l = attn_aggregate(op.indptr, op.indices, scores, feat, op.num_rows, scale, return_stats=True)
            ctx.save_for_backward(feat, scores, out, m, l)      # never alpha
            return out
        out, m, l = attn_aggregate(op.indptr, op.indices, scores, feat, op.num_rows, scale, return_stats=True, mask=mask,
                                   keep_scale=keep_scale)
        ctx.save_for_backward(feat, scores, out, m, l, mask)    # one bit per edge and head: never alpha, never a float mask
        return out

    @staticmethod
    def backward(ctx, grad_out):
        from .attn_aggregate import attn_aggregate_grad_feat, attn_aggregate_grad_scores

        op = ctx.op
        feat, scores, out, m, l = (t.detach() for t in ctx.saved_tensors[:5])
        drop = {"mask": ctx.saved_tensors[5], "keep_scale": ctx.keep_scale} if ctx.dropout else {}
        grad_out = grad_out.float().contiguous()
        grad_feat = grad_scores = None
        if ctx.needs_input_grad[0]:           # the transposed CSR, alpha recomputed through its edge order; dC is not permuted
            grad_feat = attn_aggregate_grad_feat(op.t_indptr, op.t_indices, op.t_order, grad_out, scores, m, l, op.num_cols,
                                                 ctx.scale, **drop).to(feat.dtype)
        if ctx.needs_input_grad[1]:           # the softmax backward's row sum is the dense product <dC, out> (the dropped out)
            delta = (grad_out * out).sum(-1)
            grad_scores = attn_aggregate_grad_scores(op.indptr, op.indices, grad_out, feat, scores, m, l, delta,
                                                     ctx.scale, **drop).to(scores.dtype)
        return (grad_feat, grad_scores, None, None, None, None) if ctx.dropout else (grad_feat, grad_scores, None, None)


class AttnAggregate(_PatternOp):
    """``out[r, h] = sum_{e in row r} softmax(scale * scores)[e, h] feat[col_e, h]`` on a CSR pattern [num_rows, num_cols] (``num_cols``
    defaults to ``num_rows``) in one launch (``voltrix.attn_aggregate``), differentiable in ``feat`` [num_cols, H, D] and ``scores``
    [nnz, H]: ``SpMMHeads(...)(feat, EdgeSoftmax(...)(scores, scale))`` without the attention weights ever being stored.  The 2-D form
    (``feat`` [num_cols, D], ``scores`` [nnz]) is one head.  Built once per pattern, exactly like ``GATScore``: the device CSR, its
    transpose and the transposed edge order (kept as int32), or ``AttnAggregate(pattern)`` on a shared ``CsrPattern``, or
    ``transposed=(t_indptr, t_indices, t_order)``.  Saves ``feat``, ``scores``, ``out`` and the row statistics ``m``, ``l`` [num_rows, H].
    The backward is ``delta = (dC * out).sum(-1)`` (dense torch), one launch split by edges for ``scores.grad`` and one on the transposed
    CSR for ``feat.grad`` (``voltrix.attn_aggregate.attn_aggregate_grad_scores`` / ``attn_aggregate_grad_feat``): no index op, no float
    atomics, no [nnz, H] tensor but ``scores.grad``; gradients come back in the inputs' dtypes, and a side nobody needs is skipped.

    Attention dropout: ``op(feat, scores, scale, dropout_p=p, training=True, seed=None, offset=0, mask=None)`` drops
    attention weights after the normalisation, ``out = sum_e alpha_e k_e feat_e`` with ``k_e = float32(1) / float32(1 - p)`` for a kept
    entry and 0 for a dropped one.  The keep mask is one bit per edge and head (``voltrix.dropout_mask(nnz, H, p, seed, offset)``, or the
    caller's ``mask=`` int32 [nnz, ceil(H / 32)]); it is all the backward saves besides ``feat, scores, out, m, l``.  ``seed=None`` draws
    a 63-bit seed from torch's default CPU generator on the host (no device synchronisation), so ``torch.manual_seed`` reproduces a run.
    Under graph capture pass ``mask=``: a seed drawn during capture is a host value baked into the graph, and every replay would drop
    the same entries -- generate the mask outside the graph (into the same buffer) and capture only its use.  With ``dropout_p == 0`` or
    ``training=False`` and no ``mask`` the call is the one without dropout: nothing is allocated, the same bits."""

    def __call__(self, feat: torch.Tensor, scores: torch.Tensor, scale: float = 1.0, dropout_p: float = 0.0, training: bool = True,
                 seed: int = None, offset: int = 0, mask: torch.Tensor = None) -> torch.Tensor:
        assert feat.dim() in (2, 3) and scores.dim() == feat.dim() - 1 and feat.shape[0] == self.num_cols
        assert scores.shape[0] == self.num_edges and scores.shape[1:] == feat.shape[1:-1], (tuple(scores.shape), tuple(feat.shape))
        dropout_p = float(dropout_p)
        if not 0.0 <= dropout_p < 1.0:
            raise ValueError(f"AttnAggregate: dropout_p must satisfy 0 <= p < 1, got {dropout_p}")
        if mask is None and (dropout_p == 0.0 or not training):
            return _AttnAggregateFunction.apply(feat, scores, self, float(scale))
        heads = 1 if feat.dim() == 2 else feat.shape[1]
        if mask is None:
            from .dropout import dropout_mask

            if seed is None:
                seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())      # the default CPU generator: no sync
            mask = dropout_mask(self.num_edges, heads, dropout_p, seed, offset, device=feat.device)
        keep_scale = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(1.0 - dropout_p, dtype=torch.float32))
        return _AttnAggregateFunction.apply(feat, scores, self, float(scale), mask, keep_scale)


class _SpMMReduceFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, op):
        from .spmm_reduce import row_degrees, spmm_reduce

        ctx.op, ctx.in_dtype = op, feat.dtype
        if op.reduce == "mean":
            ctx.save_for_backward(row_degrees(op.indptr))       # nothing but the degrees
            return spmm_reduce(op.indptr, op.indices, feat, op.num_rows, "mean")
        out, arg = spmm_reduce(op.indptr, op.indices, feat, op.num_rows, op.reduce, return_arg=True)
        ctx.save_for_backward(arg)                              # the winners' entry ids: never feat
        return out

    @staticmethod
    def backward(ctx, grad_out):
        from .spmm_reduce import spmm_mean_backward, spmm_reduce_backward

        op = ctx.op
        (saved,) = ctx.saved_tensors
        if op.reduce == "mean":
            grad = spmm_mean_backward(op.t_indptr, op.t_indices, grad_out, saved, op.num_cols)
        else:
            grad = spmm_reduce_backward(op.t_indptr, op.t_indices, op.t_order, grad_out, saved, op.num_cols)
        return grad.to(ctx.in_dtype), None


class SpMMReduce(_PatternOp):
    """``out[r] = max | min | mean over the entries e of row r of feat[col_e]`` per element on a CSR pattern [num_rows, num_cols]
    (``num_cols`` defaults to ``num_rows``), differentiable in ``feat`` [num_cols, ...]: ``SpMMReduce(indptr, indices, n, reduce="max")(feat)``
    -- the aggregator of max-pool GraphSAGE, PNA and GIN-max (``voltrix.spmm_reduce``).  Built once per pattern like the attention
    operators: the device CSR, its transpose and the transposed edge order, or ``SpMMReduce(pattern, reduce=...)`` on a ``CsrPattern``
    shared with them.  max / min save the winners' entry ids ``arg`` (int32, the shape of ``out``) and not ``feat``; the gradient of an
    element goes to its one winner (the first in CSR order on a tie) by a gather on the transposed CSR.  mean saves nothing but the
    degrees; its gradient is the CSR row-gather sum on the transposed CSR applied to ``dC / deg``.  No index op, no float atomics, the
    same bits on every call; ``out`` is float32 and the gradient comes back in ``feat``'s dtype."""

    def __init__(self, indptr, indices: torch.Tensor = None, num_rows: int = None, num_cols: int = None, transposed=None,
                 reduce: str = "max"):
        from .spmm_reduce import REDUCTIONS

        if reduce not in REDUCTIONS:
            raise ValueError(f"SpMMReduce: reduce must be one of {REDUCTIONS}, got {reduce!r}")
        super().__init__(indptr, indices, num_rows, num_cols, transposed)
        self.reduce = reduce

    def __call__(self, feat: torch.Tensor) -> torch.Tensor:
        assert feat.dim() >= 2 and feat.shape[0] == self.num_cols, (tuple(feat.shape), self.num_cols)
        return _SpMMReduceFunction.apply(feat, self)


class _SpMMMultiFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, op):
        from .spmm_multi import spmm_multi

        ctx.op, ctx.in_dtype = op, feat.dtype
        out, state = spmm_multi(op.indptr, op.indices, feat, op.num_rows, op.aggrs, op.eps, return_state=True)
        # only what the requested aggregates need: the winners' entry ids for max / min; feat, mean and std for var / std; nothing
        # for sum / mean alone
        ctx.save_for_backward(*[t for t in (state.argmax, state.argmin, state.mean, state.std, feat if op.moments else None)
                                if t is not None])
        return out

    @staticmethod
    def backward(ctx, grad_out):
        from .spmm_multi import spmm_multi_backward
        from .spmm_reduce import row_degrees

        op = ctx.op
        saved = list(ctx.saved_tensors)
        argmax = saved.pop(0) if "max" in op.aggrs else None
        argmin = saved.pop(0) if "min" in op.aggrs else None
        mean = saved.pop(0) if op.moments else None
        std = saved.pop(0) if "std" in op.aggrs else None
        feat = saved.pop(0) if op.moments else None
        g = {name: grad_out[:, i].float() for i, name in enumerate(op.aggrs)}
        shape = (op.num_rows,) + (1,) * (grad_out.dim() - 2)
        deg = row_degrees(op.indptr).view(shape)
        u = w = None                      # u = g_sum + g_mean / d,  w = 2 g_var / d + g_std / (d std)
        if "mean" in g:
            u = g["mean"] / deg
        if "sum" in g:
            u = g["sum"] if u is None else u + g["sum"]
        if "var" in g:
            w = 2.0 * g["var"] / deg
        if "std" in g:
            by_std = g["std"] / (deg * std)
            w = by_std if w is None else w + by_std
        grad = spmm_multi_backward(op.t_indptr, op.t_indices, op.t_order, op.num_cols, feat=feat, u=u, w=w, mean=mean,
                                   g_max=g.get("max"), argmax=argmax, g_min=g.get("min"), argmin=argmin)
        return grad.to(ctx.in_dtype), None


class SpMMMulti(_PatternOp):
    """``out[r, a] = aggrs[a] over the entries e of row r of feat[col_e]`` per element on a CSR pattern [num_rows, num_cols] (``num_cols``
    defaults to ``num_rows``), differentiable in ``feat`` [num_cols, ...]: ``SpMMMulti(indptr, indices, n, aggrs=("mean", "max", "min",
    "std"), eps=1e-5)(feat)`` -> float32 ``[n, len(aggrs), ...]`` -- the aggregators of a PNA layer from one gather
    (``voltrix.spmm_multi``), or ``SpMMMulti(pattern, aggrs=...)`` on a ``CsrPattern`` shared with the other operators.  The backward is
    one gather on the transposed CSR.  Saved is only what the requested aggregates need: the winners' entry ids for max / min (int32,
    never ``feat``); ``feat``, ``mean`` and ``std`` for var / std; nothing for sum / mean alone.  The gradient of max / min goes to the
    one winner of an element (the first in CSR order on a tie).  The gradient of var / std is ``w (x - mean)`` per entry with ``w = 2
    g_var / d + g_std / (d std)``: a non-finite feature in a row makes it NaN for that row's columns (``std`` is NaN there).  A row
    without entries passes nothing back.  No index op, no float atomics, the same bits on every call; ``out`` is float32 and the
    gradient comes back in ``feat``'s dtype."""

    def __init__(self, indptr, indices: torch.Tensor = None, num_rows: int = None, num_cols: int = None, transposed=None,
                 aggrs=("mean", "max", "min", "std"), eps: float = 1e-5):
        from .spmm_multi import check_aggrs

        self.aggrs = check_aggrs("SpMMMulti", aggrs, eps)
        self.eps = float(eps)
        self.moments = "var" in self.aggrs or "std" in self.aggrs
        super().__init__(indptr, indices, num_rows, num_cols, transposed)

    def __call__(self, feat: torch.Tensor) -> torch.Tensor:
        assert feat.dim() >= 2 and feat.shape[0] == self.num_cols, (tuple(feat.shape), self.num_cols)
        return _SpMMMultiFunction.apply(feat, self)


class _SpMMEdgeFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, efeat, op, kind):
        from .spmm_edge import spmm_edge

        ctx.op, ctx.kind = op, kind
        ctx.feat_dtype, ctx.efeat_dtype = None if feat is None else feat.dtype, efeat.dtype
        if kind in ("mul", "add_relu"):         # add and copy: the gradients are functions of grad_out alone
            ctx.save_for_backward(feat, efeat)
        return spmm_edge(op.indptr, op.indices, feat, efeat, op.num_rows, kind)

    @staticmethod
    def backward(ctx, grad_out):
        from .spmm_edge import grad_efeat, grad_feat

        op, kind = ctx.op, ctx.kind
        feat, efeat = ctx.saved_tensors if ctx.saved_tensors else (None, None)
        d_feat = d_efeat = None
        if kind != "copy" and ctx.needs_input_grad[0]:
            d_feat = grad_feat(op.t_indptr, op.t_indices, op.t_order, grad_out, feat, efeat, kind, op.num_cols).to(ctx.feat_dtype)
        if ctx.needs_input_grad[1]:
            d_efeat = grad_efeat(op.indptr, op.indices, grad_out, feat, efeat, kind).to(ctx.efeat_dtype)
        return d_feat, d_efeat, None, None


class SpMMEdge(_PatternOp):
    """``out[r] = sum over the entries e of row r of m(feat[col_e], efeat[e])`` per element on a CSR pattern [num_rows, num_cols]
    (``num_cols`` defaults to ``num_rows``), differentiable in both operands: ``SpMMEdge(indptr, indices, n)(feat, efeat, op="mul")`` with
    ``op`` one of ``"mul"``, ``"add"``, ``"add_relu"`` (GINE's message ``relu(x_j + e_ij)``) and ``"copy"`` (``feat=None``) -- the
    aggregation of GINE, NNConv / MPNN and CGConv layers (``voltrix.spmm_edge``).  ``feat`` [num_cols, ...], ``efeat`` [nnz, ...] in
    CSR entry order with the same trailing dimensions.  Built once per pattern like the attention operators, or ``SpMMEdge(pattern)`` on
    a ``CsrPattern`` shared with them.  Only the gradients ``needs_input_grad`` asks for are computed: ``efeat``'s by one row-parallel
    launch, ``feat``'s by a gather on the transposed CSR.  mul and add_relu save both operands, add and copy nothing.  No index op, no
    float atomics, the same bits on every call; ``out`` is float32 and the gradients come back in the operands' dtypes."""

    def __call__(self, feat, efeat: torch.Tensor, op: str = "mul") -> torch.Tensor:
        from .spmm_edge import check_operands

        check_operands("SpMMEdge", op, feat, efeat, self.num_edges)
        assert feat is None or feat.shape[0] == self.num_cols, (tuple(feat.shape), self.num_cols)
        return _SpMMEdgeFunction.apply(feat, efeat, self, op)


class _SpMMRelFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, coef, weight, op):
        from .spmm_rel import spmm_rel

        ctx.op, ctx.weight = op, weight
        ctx.save_for_backward(feat, coef)           # coef: None for the identity; weight is a constant of the graph, not saved here
        return spmm_rel(op.indptr, op.indices, op.etype, feat, op.num_types if coef is None else coef, op.num_rows, weight)

    @staticmethod
    def backward(ctx, grad_out):
        from .spmm_rel import grad_coef, grad_feat

        op = ctx.op
        feat, coef = ctx.saved_tensors
        d_feat = d_coef = None
        if ctx.needs_input_grad[0]:
            d_feat = grad_feat(op.t_indptr, op.t_indices, op.t_order, op.etype, grad_out, op.num_types if coef is None else coef,
                               op.num_cols, ctx.weight).to(feat.dtype)
        if coef is not None and ctx.needs_input_grad[1]:
            d_coef = grad_coef(op.indptr, op.indices, op.etype, op.type_index, grad_out, feat, ctx.weight).to(coef.dtype)
        return d_feat, d_coef, None, None


class SpMMRel(_PatternOp):
    """``out[i, b] = sum over the entries e of row i of weight[e] * coef[etype[e], b] * feat[col_e]`` on a CSR pattern [num_rows,
    num_cols] whose entries carry a type: R-GCN's aggregation with basis decomposition (``voltrix.spmm_rel``), differentiable in
    ``feat`` [num_cols, F] and ``coef`` [num_types, B]: ``SpMMRel(indptr, indices, n, etype=etype, num_types=R)(feat, coef, weight)`` ->
    float32 [num_rows, B, F]; ``coef=None`` is the identity ([num_rows, R, F], no gradient for it).  ``etype``: int32 [nnz] in CSR
    entry order (``etype[block.entries]`` with ``SpMMRel(block.pattern, ...)``).  ``weight``: fp32 [nnz] or None, the degree normaliser
    (``voltrix.spmm_rel.type_norm``); it gets no gradient: a ``weight`` that requires grad is a ``ValueError``.  Built once per pattern
    like the attention operators, or on a ``CsrPattern`` shared with them; its ``TypeIndex`` (which refuses a type outside
    ``[0, num_types)``) is built once, in the constructor.  Only the gradients ``needs_input_grad`` asks for are computed: ``feat``'s by
    a gather on the transposed CSR, ``coef``'s by one row-parallel launch and two fixed-order row sums.  ``feat`` and ``coef`` alone are
    saved.  No index op, no float atomics, the same bits on every call; the gradients come back in the operands' dtypes."""

    def __init__(self, indptr, indices: torch.Tensor = None, num_rows: int = None, num_cols: int = None, transposed=None, *,
                 etype: torch.Tensor, num_types: int):
        from .spmm_rel import TypeIndex

        super().__init__(indptr, indices, num_rows, num_cols, transposed)
        if etype.dim() != 1 or etype.numel() != self.num_edges:
            raise ValueError(f"SpMMRel: etype must be [nnz] = [{self.num_edges}], got {tuple(etype.shape)}")
        self.num_types = int(num_types)
        self.etype = etype.to(torch.int32).contiguous().cuda()
        self.type_index = TypeIndex(self.etype, self.num_types)

    def __call__(self, feat: torch.Tensor, coef: torch.Tensor = None, weight: torch.Tensor = None) -> torch.Tensor:
        from .spmm_rel import _check

        if weight is not None and weight.requires_grad:
            raise ValueError("SpMMRel: weight is the degree normaliser and gets no gradient; a learnt scalar per edge is "
                             "voltrix.spmm_heads / attn_aggregate")
        _check("SpMMRel", self.pattern.indices, self.etype, coef, weight, feat=feat)
        if coef is not None and coef.shape[0] != self.num_types:
            raise ValueError(f"SpMMRel: coef {tuple(coef.shape)} has not {self.num_types} rows")
        assert feat.shape[0] == self.num_cols, (tuple(feat.shape), self.num_cols)
        return _SpMMRelFunction.apply(feat, coef, weight, self)


class _SpMMFp8Function(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, values, op, scale, out_dtype):
        from .fp8 import quantize_fp8, spmm_fp8

        ctx.op, ctx.values, ctx.in_dtype = op, values, feat.dtype       # values: a constant of the graph; feat is saved nowhere
        return spmm_fp8(op.indptr, op.indices, quantize_fp8(feat, scale), op.num_rows, values, out_dtype)

    @staticmethod
    def backward(ctx, grad_out):
        from . import capi
        from .jit_kernels.spmm import _raw_stream
        from .utils import padded_last_dim, piece_width

        op = ctx.op
        dim = grad_out.shape[1]
        width = piece_width(max(dim, 1), torch.float32)
        out = torch.empty((op.num_cols, width), dtype=torch.float32, device=grad_out.device)
        if op.num_edges == 0 or dim == 0:
            out.zero_()
        elif op.num_cols > 0:
            values = None if ctx.values is None else ctx.values.float()[op.t_order].contiguous()
            capi.launch_spmm_csr_rows(op.t_indptr, op.t_indices, op.num_cols, padded_last_dim(grad_out.float(), width), out,
                                      _raw_stream(out.device), 1, values)
        return out[:, :dim].to(ctx.in_dtype), None, None, None, None


class SpMMFp8(_PatternOp):
    """``out[r] = sum over the entries e of row r of values[e] * q(feat)[col_e]`` on a CSR pattern [num_rows, num_cols], where ``q`` is
    the FP8 (e4m3fn) quantisation of ``voltrix.quantize_fp8``: ``SpMMFp8(indptr, indices, n)(feat, values=None, scale="column")`` ->
    ``out_dtype`` (float32) [num_rows, F] -- aggregation at half the gathered bytes of a 16-bit row (``voltrix.spmm_fp8``; its docstring
    has the error bounds).  Built once per pattern like the attention operators, or ``SpMMFp8(pattern)`` on a ``CsrPattern`` shared
    with them (``block.pattern`` of a sampled block).  The forward quantises ``feat`` and aggregates; ``feat`` is saved nowhere.  The
    backward is STRAIGHT-THROUGH: ``d_feat = csr(values)^T grad_out``, the exact fp32 CSR row-gather sum on the pattern's transpose
    (``values[t_order]`` where values are given), as if the quantiser were the identity; it comes back in ``feat``'s dtype.  ``values``
    (fp32 [nnz], e.g. a degree normaliser) gets no gradient: one that requires grad is a ``ValueError``.  An ``Fp8Rows`` in place of
    ``feat`` is the inference case: nothing is quantised again and no gradient flows."""

    def __call__(self, feat, values: torch.Tensor = None, scale="column", out_dtype=torch.float32) -> torch.Tensor:
        from .fp8 import Fp8Rows, _check_quantize, spmm_fp8

        if values is not None and values.requires_grad:
            raise ValueError("SpMMFp8: values get no gradient; learnt edge values are voltrix.autograd.SpMM(values=) / SpMMHeads")
        if isinstance(feat, Fp8Rows):
            return spmm_fp8(self.indptr, self.indices, feat, self.num_rows, values, out_dtype)
        _check_quantize("SpMMFp8", feat, scale)
        if values is not None and values.numel() != self.num_edges:
            raise ValueError(f"SpMMFp8: values must be [nnz] = [{self.num_edges}], got {tuple(values.shape)}")
        if out_dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError(f"SpMMFp8: out_dtype must be torch.float32, float16 or bfloat16, got {out_dtype}")
        assert feat.shape[0] == self.num_cols, (tuple(feat.shape), self.num_cols)
        return _SpMMFp8Function.apply(feat, values, self, scale, out_dtype)


class SpMM:
    """``C = A @ B`` with a gradient for ``B``.  ``A``: binary CSR [num_rows, num_cols] (``num_cols`` defaults to
    ``num_rows``), or, with ``values`` (round 6), the weighted matrix ``csr(values)``.  Builds two reference-format handles on the current device (A and A^T); both go through
    ``voltrix.spmm`` -- tuner, schedules and the two-level side-car included."""

    def __init__(self, indptr: torch.Tensor, indices: torch.Tensor, num_rows: int, num_cols: int = None, hash_tag: str = None,
                 values: torch.Tensor = None):
        assert indptr.dtype == torch.int32 and indices.dtype == torch.int32 and indptr.numel() == num_rows + 1
        self.num_rows = num_rows
        self.num_cols = num_rows if num_cols is None else int(num_cols)
        self.num_edges = int(indices.numel())
        indptr_d, indices_d = indptr.contiguous().cuda(), indices.contiguous().cuda()
        self.weighted = self.weighted_t = None
        if values is not None:
            # round 6: edge values.  Separable ones (v_ij = r_i c_j: normalised adjacencies) run both directions on the binary
            # operator between two row scalings -- A^T has the factors swapped --; general ones through value planes of A and A^T
            from .weighted import WeightedHandle, csr_preprocess_weighted, transpose_weighted

            values_d = values.contiguous().cuda()
            self.weighted = csr_preprocess_weighted(indptr_d, indices_d, values_d, num_rows, num_cols=self.num_cols)
            if self.weighted.separable:
                t_indptr, t_indices = csr_transpose_device(indptr_d, indices_d, num_rows, self.num_cols)
                t_handle = csr_preprocess_device(t_indptr, t_indices, self.num_cols, num_cols=num_rows)
                self.weighted_t = WeightedHandle(*t_handle, None, self.num_cols, self.num_edges,
                                                 row_scale=self.weighted.col_scale, col_scale=self.weighted.row_scale)
            else:
                t_indptr, t_indices, t_values = transpose_weighted(indptr_d, indices_d, values_d, num_rows, self.num_cols)
                self.weighted_t = csr_preprocess_weighted(t_indptr, t_indices, t_values, self.num_cols, num_cols=num_rows,
                                                          separable=False)
            self.handle = (self.weighted.blk_offsets, self.weighted.hspa_packed, self.weighted.hind)
            self.handle_t = (self.weighted_t.blk_offsets, self.weighted_t.hspa_packed, self.weighted_t.hind)
            if hash_tag is not None:
                self.handle[1].hash_tag = hash_tag
                self.handle_t[1].hash_tag = hash_tag + "/transposed"
            return
        self.handle = csr_preprocess_device(indptr_d, indices_d, num_rows, num_cols=self.num_cols)
        t_indptr, t_indices = csr_transpose_device(indptr_d, indices_d, num_rows, self.num_cols)
        self.handle_t = csr_preprocess_device(t_indptr, t_indices, self.num_cols, num_cols=num_rows)
        if hash_tag is not None:
            self.handle[1].hash_tag = hash_tag
            self.handle_t[1].hash_tag = hash_tag + "/transposed"

    def update_values(self, values: torch.Tensor) -> None:
        """New edge values on the same pattern (CSR order of the constructor's ``indices``): both directions, in place
        (``weighted.update_values``: one scatter per plane, no rebuild).  No gradient flows to values installed here; pass them per
        call instead (``op(feat, values=v)``), which gives ``v`` its gradient through the sampled dense-dense product."""
        from .weighted import transpose_order, update_values

        assert self.weighted is not None, "this operator was built without values"
        values_d = values.contiguous().cuda()
        was_separable = self.weighted.separable
        update_values(self.weighted, values_d)
        indptr_d, indices_d = self.weighted.csr[0], self.weighted.csr[1]
        if self.weighted.separable:                    # A^T has the factors swapped
            self.weighted_t.row_scale, self.weighted_t.col_scale = self.weighted.col_scale, self.weighted.row_scale
        elif was_separable:                            # the new values do not factor: A^T needs a value plane of its own now
            self._general_transposed(values_d)
        else:
            if getattr(self, "_t_order", None) is None:
                self._t_order = transpose_order(indptr_d, indices_d, self.num_rows)
            update_values(self.weighted_t, values_d[self._t_order])

    def _general_transposed(self, values_d: torch.Tensor) -> None:
        """``A^T`` with a value plane of its own, built from ``values`` (CSR order of ``A``)."""
        from .weighted import csr_preprocess_weighted, transpose_weighted

        indptr_d, indices_d = self.weighted.csr[0], self.weighted.csr[1]
        t_indptr, t_indices, t_values = transpose_weighted(indptr_d, indices_d, values_d, self.num_rows, self.num_cols)
        tag = getattr(self.handle_t[1], "hash_tag", None)
        self.weighted_t = csr_preprocess_weighted(t_indptr, t_indices, t_values, self.num_cols, num_cols=self.num_rows,
                                                  separable=False)
        self.handle_t = (self.weighted_t.blk_offsets, self.weighted_t.hspa_packed, self.weighted_t.hind)
        if tag is not None:
            self.handle_t[1].hash_tag = tag

    def _install(self, values: torch.Tensor) -> None:
        """Values of one forward, in both directions.  The first install on a separable operator makes both directions general, once
        (as ``update_values`` does for values that do not factor), so that later installs are scatters without the separable check."""
        from .weighted import make_general

        if self.weighted.separable:
            values_d = values.contiguous().cuda()
            make_general(self.weighted, values_d)
            self._general_transposed(values_d)
        else:
            self.update_values(values)
        self._installs = getattr(self, "_installs", 0) + 1

    def __call__(self, feat: torch.Tensor, values: torch.Tensor = None) -> torch.Tensor:
        """``A @ feat``; with ``values`` ([nnz], CSR order of the constructor's ``indices``; the operator must have been built with
        values) ``csr(values) @ feat``, differentiable in ``feat`` and ``values``.  Each call installs its values in both directions;
        a backward whose forward's values were replaced since installs them again."""
        assert feat.shape[0] == self.num_cols
        if values is None:
            return _SpMMFunction.apply(feat, self)
        assert self.weighted is not None, "this operator was built without values"
        assert values.numel() == self.num_edges, (values.numel(), self.num_edges)
        return _SpMMValuesFunction.apply(feat, values, self)
