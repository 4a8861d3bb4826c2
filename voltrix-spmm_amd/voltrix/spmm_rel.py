"""Relational (R-GCN) aggregation over TYPED edges on a CSR pattern, with basis decomposition:

    out[i, b, :] = sum_{e in row i} w_e * coef[etype_e, b] * feat[col_e, :]        then        h' = out.view(n, B * F) @ V.view(B * F, F_out)

which is Schlichtkrull et al.'s ``sum_r sum_{j in N_r(i)} 1 / c_{i,r} W_r h_j`` with ``W_r = sum_b coef[r, b] V_b``: aggregate first,
transform after.  The output is ``[n, B, F]`` for ``B`` bases whatever the number of relations ``R``; one index read and one gathered
row per edge serve all bases; nothing of size ``[nnz, ., F]`` or ``[R n, .]`` exists; ``V``, ``W_0`` and the activation stay dense
torch.  With ``coef = I_R`` (``coef=None``) the same operator is the plain per-relation sum ``[n, R, F]``.

    out    = voltrix.spmm_rel(indptr, indices, etype, feat, coef, num_rows, weight=None)                      # fp32 [num_rows, B, F]
    d_feat = voltrix.spmm_rel.grad_feat(t_indptr, t_indices, t_order, etype, grad_out, coef, num_cols, weight=None)   # fp32 [num_cols, F]
    d_coef = voltrix.spmm_rel.grad_coef(indptr, indices, etype, type_index, grad_out, feat, weight=None)      # fp32 [R, B]
    norm   = voltrix.spmm_rel.type_norm(indptr, etype, num_types)                                             # fp32 [nnz]

Semantics.  ``indptr`` / ``indices``: device int32 CSR of ``[num_rows, num_cols]``; rectangular patterns and duplicate entries are
allowed.  ``etype``: int32 ``[nnz]`` in CSR entry order with ``0 <= etype < R`` (``etype[block.entries]`` for a sampled block or
subgraph).  ``feat``: ``[num_cols, F]`` fp32 / fp16 / bf16 read as stored, other types as fp32.  ``coef``: ``[R, B]``, read as fp32.
``weight``: optional fp32 ``[nnz]`` (the normaliser ``1 / c_{i,r}``, e.g. ``type_norm``); ``None`` means 1.  Outputs are fp32 with
every element written; a row without entries gives 0 and a type without entries a zero gradient.  ``weight`` gets no gradient (learnt
per-edge scalars are ``voltrix.spmm_heads`` / ``attn_aggregate`` territory).

    forward     out[i, b, f]  = sum_{e in row i}  c_eb * feat[col_e, f]                  c_eb = w_e * coef[etype_e, b]  (fp32; no w: coef)
    grad_feat   dF[c, f]      = sum_{e in col c}  sum_b c_eb * g[row_e, b, f]            g = grad_out, fp32 [num_rows, B, F]
    grad_coef   dC[r, b]      = sum_{e: etype_e = r}  w_e * <g[row_e, b, :], feat[col_e, :]>

fp32 throughout, sums in a fixed order (voltrix/spmm_rel_kernels.hpp; ``grad_coef``: the entries of a type in CSR order in chunks of
``CHUNK``, then the chunks in order), no float atomics, the same bits on every call; NaN and inf propagate as the arithmetic does.
``|out - ref| <= (k + 2) 2^-23 sum |terms|`` for the ``k`` entries of a row, ``(k B + 2)`` for ``grad_feat``, ``(m_r + F + 2)`` for
``grad_coef`` with ``m_r`` entries of type ``r``.  Known limit: a hub row (in ``grad_feat``: a hub column) serialises its wave, like
``voltrix.spmm_heads``.

Which form to use (measured, DESIGN.md 3.29, ``harness/bench_spmm_rel.py``; one layer forward + backward on the MI355X).  Against the
per-edge messages this operator is 3.5-10x faster at every point.  Against transform-first -- ``H_r = h W_r`` for every relation and
``voltrix_launch_spmm_csr_rows`` over ``[R n, F_out]`` with columns ``etype n + col`` -- it wins where the graph is sparse beside the
number of relations and the bases are few (amazon0601-like, 8.4 entries per row, R = 46, B = 8: 1.6-3.2x faster at a sixth to a
quarter of the memory) and LOSES where ``nnz / n`` is large beside ``R`` (reddit-like, 492 entries per row: transform-first is 3-28x
faster), at small ``R`` (4: 0.85x) and at ``B`` = 30 (0.55-0.86x).  Rule of thumb: aggregate first when ``nnz / n < R`` and
``B <= R / 4``.
"""
from __future__ import annotations

import torch

from .utils import FEATURE_TYPES, padded_last_dim, piece_width

BASIS_TILE = 8        # the forward kernel's largest tile of bases (kRelBasisTile): beyond it grid.z walks tiles
CHUNK = 512           # entries of one type per chunk of grad_coef's first-level sum
MAX_TYPES, MAX_BASES = 65536, 1024


def _check(who, indices, etype, coef, weight, feat=None, grad_out=None, num_rows=None):
    """The ``ValueError`` cases, before any tensor's device is looked at."""
    nnz = indices.numel()
    if etype is None or etype.dim() != 1 or etype.numel() != nnz:
        raise ValueError(f"{who}: etype must be [nnz] = [{nnz}], got {None if etype is None else tuple(etype.shape)}")
    if isinstance(coef, torch.Tensor):
        if coef.dim() != 2 or not 1 <= coef.shape[0] <= MAX_TYPES or coef.shape[1] > MAX_BASES:
            raise ValueError(f"{who}: coef must be [R, B] with 1 <= R <= {MAX_TYPES} and B <= {MAX_BASES}, got {tuple(coef.shape)}")
    elif coef is not None and not (isinstance(coef, int) and 1 <= coef <= min(MAX_TYPES, MAX_BASES)):
        raise ValueError(f"{who}: coef must be a tensor [R, B], None or the number of types (the identity, at most {MAX_BASES})")
    if weight is not None and (weight.dim() != 1 or weight.numel() != nnz):
        raise ValueError(f"{who}: weight must be [nnz] = [{nnz}], got {tuple(weight.shape)}")
    if feat is not None and feat.dim() != 2:
        raise ValueError(f"{who}: feat must be [num_cols, F], got {tuple(feat.shape)}")
    if grad_out is not None:
        if grad_out.dim() != 3 or (num_rows is not None and grad_out.shape[0] != num_rows):
            raise ValueError(f"{who}: grad_out must be [num_rows, B, F], got {tuple(grad_out.shape)}")
        if isinstance(coef, torch.Tensor) and grad_out.shape[1] != coef.shape[1]:
            raise ValueError(f"{who}: grad_out {tuple(grad_out.shape)} has not coef's {coef.shape[1]} bases")
        if feat is not None and grad_out.shape[2] != feat.shape[1]:
            raise ValueError(f"{who}: grad_out {tuple(grad_out.shape)} and feat {tuple(feat.shape)} differ in width")


def _coef_table(coef, etype, device):
    """``coef`` as the kernels read it: fp32 ``[R, B_pad]`` with ``B_pad`` = B rounded up to 4, contiguous (a tensor that is that already
    is not copied; the table is small).  ``None``: the identity of ``etype.max() + 1`` types (one read-back); an int: of that many."""
    if coef is None:
        coef = int(etype.max()) + 1 if etype.numel() else 1
    if isinstance(coef, int):
        coef = torch.eye(coef, dtype=torch.float32, device=device)
    bases = coef.shape[1]
    return padded_last_dim(coef.float(), max(4, (bases + 3) // 4 * 4)), bases


def _edge_tables(etype, weight):
    return etype.to(torch.int32).contiguous(), None if weight is None else weight.float().contiguous()


def spmm_rel(indptr: torch.Tensor, indices: torch.Tensor, etype: torch.Tensor, feat: torch.Tensor, coef, num_rows: int,
             weight=None) -> torch.Tensor:
    """``out[i, b] = sum_{e in row i} weight[e] * coef[etype[e], b] * feat[indices[e]]`` -> float32 ``[num_rows, B, F]``, every element
    written (a row without entries: 0), on the current stream.  ``coef=None``: the identity, ``out`` is ``[num_rows, R, F]`` with
    ``R = etype.max() + 1`` (one read-back; pass the number of types as an int to avoid it).  A width that is not a whole number of
    16-byte pieces of ``feat``'s type is padded with zeros and sliced away; a contiguous, 16-byte aligned operand is never copied.
    ``B > BASIS_TILE`` reads the gathered rows once per tile of ``BASIS_TILE`` bases.  ``ValueError``: ``etype`` not ``[nnz]``, ``coef``
    not ``[R, B]``, ``weight`` not ``[nnz]``, ``feat`` not 2-D."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    _check("spmm_rel", indices, etype, coef, weight, feat=feat)
    assert indptr.is_cuda and indices.is_cuda and indptr.dtype == torch.int32 and indices.dtype == torch.int32
    assert indptr.numel() == num_rows + 1 and feat.is_cuda and etype.is_cuda
    if feat.dtype not in FEATURE_TYPES:
        feat = feat.float()
    table, bases = _coef_table(coef, etype, feat.device)
    dim = feat.shape[1]
    width = piece_width(max(dim, 1), feat.dtype)
    out = torch.empty((num_rows, bases, width), dtype=torch.float32, device=feat.device)
    if num_rows > 0 and dim > 0 and bases > 0:
        feat = padded_last_dim(feat, width)
        etype, weight = _edge_tables(etype, weight)
        num_entries = indices.numel()
        if num_entries == 0:          # nothing is gathered; the entry point still wants pointers it could read
            indices = etype = indptr
            weight = None
        if feat.shape[0] == 0:
            feat = torch.zeros((1, width), dtype=feat.dtype, device=feat.device)
        capi.launch_spmm_rel(indptr.contiguous(), indices.contiguous(), etype, weight, num_rows, feat, table, bases, out,
                             _raw_stream(out.device), num_entries)
    if width != dim:
        out = out[:, :, :dim].contiguous()
    return out


def grad_feat(t_indptr: torch.Tensor, t_indices: torch.Tensor, t_order, etype: torch.Tensor, grad_out: torch.Tensor, coef,
              num_cols: int, weight=None) -> torch.Tensor:
    """The gradient of ``spmm_rel`` for ``feat`` -> float32 ``[num_cols, F]``, every element written, columns without entries zero: a
    gather on the TRANSPOSED CSR (``voltrix.autograd.csr_transpose_device``) that contracts ``grad_out`` [num_rows, B, F] over the bases.
    ``etype`` and ``weight`` stay in CSR entry order and are read through ``t_order`` (the entry of the CSR that entry ``e`` of the
    transpose is; ``None``: they are in the transpose's order already).  No float atomics, the same bits on every call."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    _check("spmm_rel.grad_feat", t_indices, etype, coef, weight, grad_out=grad_out)
    assert t_indptr.is_cuda and t_indices.is_cuda and t_indptr.dtype == torch.int32 and t_indices.dtype == torch.int32
    assert t_indptr.numel() == num_cols + 1 and grad_out.is_cuda and etype.is_cuda
    assert t_order is None or (t_order.is_cuda and t_order.numel() == t_indices.numel())
    table, bases = _coef_table(coef, etype, grad_out.device)
    if grad_out.shape[1] != bases:
        raise ValueError(f"spmm_rel.grad_feat: grad_out {tuple(grad_out.shape)} has not coef's {bases} bases")
    dim = grad_out.shape[2]
    width = piece_width(max(dim, 1), torch.float32)
    nnz = t_indices.numel()
    if num_cols == 0 or dim == 0 or bases == 0 or nnz == 0:
        return torch.zeros((num_cols, dim), dtype=torch.float32, device=grad_out.device)
    out = torch.empty((num_cols, width), dtype=torch.float32, device=grad_out.device)
    etype, weight = _edge_tables(etype, weight)
    t_order = None if t_order is None else t_order.to(torch.int32).contiguous()
    capi.launch_spmm_rel_contract(t_indptr.contiguous(), t_indices.contiguous(), t_order, etype, weight, num_cols,
                                  padded_last_dim(grad_out.float(), width), table, out, _raw_stream(out.device))
    return out if width == dim else out[:, :dim].contiguous()


class TypeIndex:
    """The entries of a typed pattern grouped by type, for ``grad_coef``'s fixed-order two-level sum: ``TypeIndex(etype, num_types)``,
    built once per ``etype`` with torch integer ops and ONE read-back (the smallest and largest type and the count per type).
    ``ValueError`` for an ``etype`` outside ``[0, num_types)``: nothing is checked on the device afterwards, so this is where a bad type
    is caught.

    ``order`` int32 [nnz]: the entry ids sorted stably by type.  ``chunk_ptr`` int32 [chunks + 1]: every type's run of ``order`` cut into
    chunks of at most ``CHUNK`` entries (a CSR over ``order`` with a row per chunk).  ``type_ptr`` int32 [num_types + 1]: the chunks of
    every type (a CSR over ``chunk_ids`` = 0 .. chunks - 1 with a row per type; a type without entries has none)."""

    def __init__(self, etype: torch.Tensor, num_types: int, chunk: int = None):
        chunk = CHUNK if chunk is None else int(chunk)
        if etype.dim() != 1 or not 1 <= num_types <= MAX_TYPES or chunk < 1:
            raise ValueError(f"TypeIndex: etype must be [nnz] and 1 <= num_types <= {MAX_TYPES}")
        dev = etype.device
        self.num_types, self.num_entries, self.chunk = int(num_types), int(etype.numel()), chunk
        types = etype.long()
        if self.num_entries:
            counted = torch.bincount(types.clamp(0, num_types - 1), minlength=num_types)
            head = torch.cat([types.min().view(1), types.max().view(1), counted]).tolist()          # the read-back
            if head[0] < 0 or head[1] >= num_types:
                raise ValueError(f"TypeIndex: etype holds {head[0]} .. {head[1]}, outside [0, {num_types})")
            counts = torch.tensor(head[2:], dtype=torch.int64)
            self.order = torch.sort(types, stable=True)[1].to(torch.int32)
        else:
            counts = torch.zeros(num_types, dtype=torch.int64)
            self.order = torch.zeros(0, dtype=torch.int32, device=dev)
        chunks_of = (counts + chunk - 1) // chunk
        type_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(chunks_of, 0)])
        self.num_chunks = int(type_ptr[-1])
        owner = torch.repeat_interleave(torch.arange(num_types), chunks_of)                          # the type of every chunk
        first = (torch.cumsum(counts, 0) - counts)[owner] + (torch.arange(self.num_chunks) - type_ptr[owner]) * chunk
        chunk_ptr = torch.cat([first, torch.tensor([self.num_entries], dtype=torch.int64)])
        self.counts = counts
        self.chunk_ptr, self.type_ptr = chunk_ptr.to(torch.int32).to(dev), type_ptr.to(torch.int32).to(dev)
        self.chunk_ids = torch.arange(self.num_chunks, dtype=torch.int32, device=dev)


def grad_coef(indptr: torch.Tensor, indices: torch.Tensor, etype: torch.Tensor, type_index: TypeIndex, grad_out: torch.Tensor,
              feat: torch.Tensor, weight=None) -> torch.Tensor:
    """The gradient of ``spmm_rel`` for ``coef`` -> float32 ``[R, B]`` (``R = type_index.num_types``), every element written, a type
    without entries zero.  One row-parallel launch writes the dots ``s[e, b] = w_e <grad_out[row_e, b], feat[col_e]>`` (fp32
    ``[nnz, B_pad]``); their sum per type is two plain CSR row-gather sums (``voltrix_launch_spmm_csr_rows``) on ``type_index``'s
    tables: chunks of at most ``CHUNK`` entries of one type, then every type's chunks in order -- no type is summed by one wave, no
    float atomics, the same bits on every call.  ``etype`` itself is read by ``type_index`` alone (it is checked against it)."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    num_rows = indptr.numel() - 1
    _check("spmm_rel.grad_coef", indices, etype, None, weight, feat=feat, grad_out=grad_out, num_rows=num_rows)
    if type_index.num_entries != indices.numel():
        raise ValueError(f"spmm_rel.grad_coef: type_index was built for {type_index.num_entries} entries, the pattern has {indices.numel()}")
    assert indptr.is_cuda and indices.is_cuda and indptr.dtype == torch.int32 and indices.dtype == torch.int32
    assert grad_out.is_cuda and feat.is_cuda
    if feat.dtype not in FEATURE_TYPES:
        feat = feat.float()
    dev = grad_out.device
    types, bases, dim, nnz = type_index.num_types, grad_out.shape[1], grad_out.shape[2], indices.numel()
    if bases == 0 or dim == 0 or nnz == 0 or num_rows == 0:
        return torch.zeros((types, bases), dtype=torch.float32, device=dev)
    width = piece_width(dim, feat.dtype)
    padded = (bases + 3) // 4 * 4
    stream = _raw_stream(dev)
    dots = torch.empty((nnz, padded), dtype=torch.float32, device=dev)
    capi.launch_spmm_rel_dots(indptr.contiguous(), indices.contiguous(), None if weight is None else weight.float().contiguous(), num_rows,
                              padded_last_dim(grad_out.float(), width), padded_last_dim(feat, width), dots, stream)
    partial = torch.empty((type_index.num_chunks, padded), dtype=torch.float32, device=dev)
    capi.launch_spmm_csr_rows(type_index.chunk_ptr, type_index.order, type_index.num_chunks, dots, partial, stream, 1)
    out = torch.empty((types, padded), dtype=torch.float32, device=dev)
    capi.launch_spmm_csr_rows(type_index.type_ptr, type_index.chunk_ids, types, partial, out, stream, 1)
    return out if padded == bases else out[:, :bases].contiguous()


def type_norm(indptr: torch.Tensor, etype: torch.Tensor, num_types: int) -> torch.Tensor:
    """R-GCN's normaliser ``1 / c_{i,r}`` -> float32 ``[nnz]``: one over the number of entries of the same row with the same type.
    Preprocessing in torch ops, on ``etype``'s device."""
    indptr = indptr.long()
    if etype.dim() != 1 or (indptr.numel() and int(indptr[-1]) != etype.numel()):
        raise ValueError("type_norm: etype must be [nnz] in CSR entry order")
    rows = torch.repeat_interleave(torch.arange(indptr.numel() - 1, device=indptr.device), indptr[1:] - indptr[:-1]).to(etype.device)
    _, inverse, counts = torch.unique(rows * int(num_types) + etype.long(), return_inverse=True, return_counts=True)
    return 1.0 / counts[inverse].float()


# ``voltrix.spmm_rel`` is the function (voltrix/__init__.py); the gradients and tables stay reachable through it
spmm_rel.grad_feat = grad_feat
spmm_rel.grad_coef = grad_coef
spmm_rel.type_norm = type_norm
spmm_rel.TypeIndex = TypeIndex
spmm_rel.BASIS_TILE = BASIS_TILE
spmm_rel.CHUNK = CHUNK
