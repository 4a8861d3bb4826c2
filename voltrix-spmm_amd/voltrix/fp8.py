"""FP8 (OCP ``e4m3fn``) feature rows and the aggregation that gathers them straight from the CSR: half the gathered bytes of the
narrowest row the other operators read, for quantised inference and for training with quantised activations and straight-through
gradients (``voltrix.autograd.SpMMFp8``).

    rows = voltrix.quantize_fp8(feat, scale="column")                                                   # Fp8Rows
    out  = voltrix.spmm_fp8(indptr, indices, rows, num_rows, values=None, out_dtype=torch.float32)      # [num_rows, F]
    out  = voltrix.spmm_fp8(pattern, rows)                    # a CsrPattern, or a Block / Subgraph (their ``pattern``), as it is
    x    = voltrix.dequantize_fp8(rows)                                                                 # fp32 [n, F], torch ops

``Fp8Rows``.  ``data``: ``torch.float8_e4m3fn`` ``[n, F16]``, ``F16`` = ``F`` rounded up to 16, the padding bytes 0x00.  ``scale``:
fp32 ``[F16]``, the dequantisation multiplier per feature COLUMN (padding 1); ``inv_scale``: fp32 ``[F16]``; ``dim`` = ``F``.

Why per column and not per row: a per-row scale is a second gathered line per entry, which gives back the bytes fp8 saves; a
per-column scale leaves the sum and is applied once in the epilogue: ``out[i, f] = scale[f] * sum_e v_e * dec(data[col_e, f])``.

``scale=``.  ``"column"``: ``amax_f = max_i |feat[i, f]|`` by torch ops without a host read-back, ``scale = amax / 448``,
``inv_scale = 448 / amax``; ``amax`` is clamped from below to ``AMAX_FLOOR = 2^-100``, so ``inv_scale <= 448 * 2^100`` is finite for
every finite non-zero ``amax`` (fp32 subnormals included) and ``scale >= 2^-100 / 448`` is a normal number; a column of zeros gets
``scale = inv_scale = 1``.  A NaN in column ``f`` makes ``amax_f`` NaN and with it the whole column: accepted.  ``"tensor"``: one
``amax`` over everything.  An fp32 tensor ``[F]`` or a scalar: taken as ``scale`` (static calibration), ``inv_scale = 1 / scale`` in
fp32; non-positive or non-finite entries are the caller's error and are not checked (that would be a host sync).

Quantisation: ``data[i, f] = rne_e4m3(clamp(fp32(feat[i, f]) * inv_scale[f], -448, 448))`` in ONE HIP launch that reads ``feat``
once (fp32 / fp16 / bf16 as stored, other types as fp32): one fp32 multiply, round to nearest even with e4m3 subnormals (spacing
2^-9), +-inf saturates to +-448, NaN gives an e4m3 NaN code, -0 keeps its sign -- torch's
``(x * inv_scale).clamp(-448, 448).to(torch.float8_e4m3fn)`` bit for bit.  A ``feat`` with unit column stride on a 16-byte boundary
(a contiguous one, a column slice of a wider tensor) is never copied.  For finite inputs

    |feat[i, f] - scale[f] * dec(data[i, f])| <= (2^-4 + 2^-20) |feat[i, f]| + 2^-10 scale[f].

Aggregation: fp32 in CSR entry order; decoded values are exact in fp32; with ``values`` one fused multiply-add per element; then one
multiply by ``scale[f]``.  Against float64 on the same bytes, with ``k`` entries in the row,

    |out - ref| <= (k + 2) 2^-23 |scale[f]| sum_e |v_e dec_e|;

integer-valued codes, power-of-two scales and integer values give equality.  ``out_dtype`` fp16 / bf16 is the fp32 result rounded to
nearest even in the epilogue: ``out16 == out32.to(dtype)`` bit for bit.  On low-degree graphs the fp32 output (4 F bytes per row) is
as many bytes as the whole gather (about deg F): the narrow output is what keeps the saving there.  Against the unquantised product
the bound is the quantisation bound above summed over the row with ``|v_e|``, plus the line above.  Every element is written, a row
without entries gives 0; no atomics, no workspace, the same bits on every call.

Where it pays (measured on the MI355X, DESIGN.md 3.30, ``harness/bench_spmm_fp8.py``).  It is an opt-in: ``voltrix.spmm`` never
chooses it.  On low-degree graphs (5-8 entries per row) with ``out_dtype=torch.float16`` the aggregation is 1.3-1.8x faster than the
fp16 row gather and than ``voltrix.spmm``; with the fp32 output it ties them (0.9-1.2x).  On graphs with hub rows or hundreds of
entries per row ``voltrix.spmm``'s block format is 3-30x faster: use that.  ``quantize_fp8`` with ``"column"`` costs 1.2-3x the
aggregation it feeds, so quantise once and aggregate many times, or pass a given ``scale``, which skips the column maxima (not
timed); re-quantising per call loses.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .utils import FEATURE_TYPES, aligned16, padded_last_dim

FP8_MAX = 448.0
AMAX_FLOOR = 2.0 ** -100
OUT_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


@dataclass
class Fp8Rows:
    """Quantised feature rows: ``data`` e4m3fn [n, F16], ``scale`` / ``inv_scale`` fp32 [F16], ``dim`` = F (module docstring)."""
    data: torch.Tensor
    scale: torch.Tensor
    inv_scale: torch.Tensor
    dim: int


def _check_quantize(who: str, feat, scale) -> None:
    """The ``ValueError`` cases of the quantiser, before any tensor's device is looked at."""
    if not isinstance(feat, torch.Tensor) or feat.dim() != 2:
        raise ValueError(f"{who}: feat must be [n, F], got {tuple(feat.shape) if isinstance(feat, torch.Tensor) else type(feat).__name__}")
    if isinstance(scale, str):
        if scale not in ("column", "tensor"):
            raise ValueError(f"{who}: scale must be 'column', 'tensor', a tensor [F] or a scalar, got {scale!r}")
    elif isinstance(scale, torch.Tensor):
        if scale.dim() > 1 or (scale.dim() == 1 and scale.numel() != feat.shape[1]):
            raise ValueError(f"{who}: a scale tensor must be [F] = [{feat.shape[1]}] or a scalar, got {tuple(scale.shape)}")
    elif not isinstance(scale, (int, float)) or isinstance(scale, bool):
        raise ValueError(f"{who}: scale must be 'column', 'tensor', a tensor [F] or a scalar, got {type(scale).__name__}")


def _scales(feat: torch.Tensor, scale, width: int):
    """``(scale, inv_scale)`` fp32 [width] on ``feat``'s device, the padding 1; torch ops, no host read-back."""
    dim = feat.shape[1]
    if isinstance(scale, str):
        if feat.shape[0] == 0 or dim == 0:
            amax = torch.zeros(dim, dtype=torch.float32, device=feat.device)
        elif scale == "column":
            amax = feat.abs().amax(dim=0).float()
        else:
            amax = feat.abs().amax().float().expand(dim)
        floored = amax.clamp_min(AMAX_FLOOR)
        one = torch.ones((), dtype=torch.float32, device=feat.device)
        mult = torch.where(amax == 0, one, floored / FP8_MAX)
        inv = torch.where(amax == 0, one, FP8_MAX / floored)
    else:
        mult = torch.as_tensor(scale, dtype=torch.float32, device=feat.device).expand(dim)
        inv = 1.0 / mult
    pad = (0, width - dim)
    return (torch.nn.functional.pad(mult, pad, value=1.0).contiguous(), torch.nn.functional.pad(inv, pad, value=1.0).contiguous())


def quantize_fp8(feat: torch.Tensor, scale="column") -> Fp8Rows:
    """``feat`` [n, F] -> ``Fp8Rows`` on the current stream: the scales by torch ops (module docstring), the codes by one HIP launch
    that reads ``feat`` once.  ``ValueError``: ``feat`` not 2-D, a ``scale`` tensor that is neither [F] nor a scalar, an unknown
    ``scale`` string."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    _check_quantize("quantize_fp8", feat, scale)
    assert feat.is_cuda
    if feat.dtype not in FEATURE_TYPES:
        feat = feat.float()
    n, dim = feat.shape
    width = (dim + 15) // 16 * 16
    mult, inv = _scales(feat, scale, width)
    data = torch.empty((n, width), dtype=torch.float8_e4m3fn, device=feat.device)
    if n > 0 and dim > 0:
        strided = (dim == 1 or feat.stride(1) == 1) and (n == 1 or feat.stride(0) >= dim)
        if not strided or feat.data_ptr() % 16:
            feat = aligned16(feat.contiguous())
        capi.launch_quantize_fp8_rows(feat, inv, data, _raw_stream(data.device))
    return Fp8Rows(data, mult, inv, dim)


def dequantize_fp8(rows: Fp8Rows) -> torch.Tensor:
    """``scale[f] * dec(data[i, f])`` -> fp32 [n, F], by torch ops (exact but for the one multiply)."""
    if not isinstance(rows, Fp8Rows):
        raise ValueError(f"dequantize_fp8: rows must be an Fp8Rows, got {type(rows).__name__}")
    return rows.data[:, :rows.dim].float() * rows.scale[:rows.dim]


def _pattern_of(graph):
    """The ``CsrPattern`` behind a ``Block`` / ``Subgraph``, a pattern itself, or None."""
    graph = getattr(graph, "pattern", graph)
    return graph if all(hasattr(graph, name) for name in ("indptr", "indices", "num_rows")) and not isinstance(graph, torch.Tensor) else None


def _check_aggregate(who: str, indices, rows, values, out_dtype) -> None:
    """The ``ValueError`` cases of the aggregation, before any tensor's device is looked at."""
    if not isinstance(rows, Fp8Rows):
        raise ValueError(f"{who}: rows must be an Fp8Rows (voltrix.quantize_fp8), got {type(rows).__name__}")
    if values is not None and values.numel() != indices.numel():
        raise ValueError(f"{who}: values must be [nnz] = [{indices.numel()}], got {tuple(values.shape)}")
    if out_dtype not in OUT_DTYPES:
        raise ValueError(f"{who}: out_dtype must be torch.float32, float16 or bfloat16, got {out_dtype}")


def spmm_fp8(indptr, indices=None, rows: Fp8Rows = None, num_rows: int = None, values=None, out_dtype=torch.float32) -> torch.Tensor:
    """``out[i, f] = scale[f] * sum_{e in row i} values[e] * dec(data[indices[e], f])`` -> ``out_dtype`` ``[num_rows, F]``, every element
    written (a row without entries: 0), on the current stream.  ``indptr`` / ``indices``: device int32 CSR of ``[num_rows, num_cols]``,
    rectangular patterns and duplicate entries allowed -- or ``spmm_fp8(pattern, rows, ...)`` with a ``CsrPattern``, ``Block`` or
    ``Subgraph``.  ``values``: optional fp32 ``[nnz]`` in CSR order (``None``: 1).  Error bounds: the module docstring.
    ``ValueError``: ``rows`` not an ``Fp8Rows``, ``values.numel() != indices.numel()``, ``out_dtype`` outside fp32 / fp16 / bf16."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    pattern = _pattern_of(indptr)
    if pattern is not None:
        if isinstance(indices, Fp8Rows) and rows is None:
            rows = indices
        indptr, indices, num_rows = pattern.indptr, pattern.indices, pattern.num_rows
    _check_aggregate("spmm_fp8", indices, rows, values, out_dtype)
    assert indptr.is_cuda and indices.is_cuda and indptr.dtype == torch.int32 and indices.dtype == torch.int32
    assert indptr.numel() == num_rows + 1 and rows.data.is_cuda
    data, dim = rows.data, rows.dim
    width = data.shape[1]
    out = torch.empty((num_rows, width), dtype=out_dtype, device=data.device)
    if num_rows > 0 and width > 0:
        data = padded_last_dim(data, width)
        num_entries = indices.numel()
        values = None if values is None else aligned16(values.float().contiguous())
        if num_entries == 0:          # nothing is gathered; the entry point still wants pointers it could read
            indices, values = indptr, None
        if data.shape[0] == 0:
            data = torch.zeros((1, width), dtype=data.dtype, device=data.device)
        capi.launch_spmm_fp8(indptr.contiguous(), indices.contiguous(), values, num_rows, data, rows.scale.contiguous(), out,
                             _raw_stream(out.device), 1, num_entries)
    return out if width == dim else out[:, :dim].contiguous()


# ``voltrix.spmm_fp8`` is the function; the constants stay reachable through it
spmm_fp8.FP8_MAX = FP8_MAX
spmm_fp8.AMAX_FLOOR = AMAX_FLOOR
