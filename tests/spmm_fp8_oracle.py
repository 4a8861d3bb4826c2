"""The oracle of ``voltrix.quantize_fp8`` / ``voltrix.spmm_fp8``: numpy and torch on the CPU, no device.

``quantize``: the stated rule through torch's own CPU cast, ``(x.float() * inv_scale).clamp(-448, 448).to(float8_e4m3fn)`` -- one
fp32 multiply, round to nearest even, e4m3 subnormals, +-inf saturated, NaN kept.  ``decode_table``: the 256 values of OCP e4m3fn from
the format's definition, in float64.  ``aggregate``: ``scale[f] * sum_e v_e * dec(data[col_e, f])`` in float64, with the mass
``sum_e |v_e dec_e|`` and the entry count per row that the error bound needs.
"""
import numpy as np
import torch

FP8_MAX = 448.0
AMAX_FLOOR = 2.0 ** -100


def decode_table() -> np.ndarray:
    """float64 [256]: ``(-1)^s 2^(e - 7) (1 + m / 8)``; ``e == 0``: ``(-1)^s m 2^-9``; 0x7f and 0xff NaN; 0x80 is -0."""
    table = np.empty(256, np.float64)
    for code in range(256):
        sign = -1.0 if code & 0x80 else 1.0
        e, m = (code >> 3) & 0xF, code & 0x7
        if e == 0xF and m == 0x7:
            table[code] = np.nan
        elif e == 0:
            table[code] = sign * m * 2.0 ** -9
        else:
            table[code] = sign * 2.0 ** (e - 7) * (1.0 + m / 8.0)
    return table


def scales(feat: torch.Tensor, mode):
    """``(scale, inv_scale)`` fp32 [F] by the documented torch formula (CPU)."""
    dim = feat.shape[1]
    if isinstance(mode, str):
        amax = feat.abs().amax(dim=0).float() if mode == "column" else feat.abs().amax().float().expand(dim)
        floored = amax.clamp_min(AMAX_FLOOR)
        one = torch.ones((), dtype=torch.float32)
        return torch.where(amax == 0, one, floored / FP8_MAX), torch.where(amax == 0, one, FP8_MAX / floored)
    scale = torch.as_tensor(mode, dtype=torch.float32).expand(dim)
    return scale, 1.0 / scale


def quantize(feat: torch.Tensor, inv_scale: torch.Tensor) -> torch.Tensor:
    """uint8 [n, F16] codes of ``feat`` [n, F] (CPU, any float type) under fp32 ``inv_scale`` [F]; the padding is 0x00."""
    n, dim = feat.shape
    width = (dim + 15) // 16 * 16
    codes = (feat.float() * inv_scale.float()).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).view(torch.uint8)
    out = torch.zeros((n, width), dtype=torch.uint8)
    out[:, :dim] = codes
    return out


def is_nan_code(codes):
    return (codes & 0x7F) == 0x7F


def aggregate(indptr, indices, codes, scale, values=None):
    """``(ref, mass, count)``: float64 [num_rows, W] ``scale * sum_e v_e dec(codes[col_e])``, float64 [num_rows, W]
    ``sum_e |v_e dec_e|`` and int64 [num_rows] entries per row, for uint8 ``codes`` [*, W] and ``scale`` [W] (numpy)."""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    dec = decode_table()[np.asarray(codes, np.uint8)]
    num_rows = len(indptr) - 1
    count = np.diff(indptr)
    v = np.ones(len(indices), np.float64) if values is None else np.asarray(values, np.float64)
    terms = dec[indices] * v[:, None]                                  # [nnz, W]
    rows = np.repeat(np.arange(num_rows), count)
    ref = np.zeros((num_rows, dec.shape[1]), np.float64)
    mass = np.zeros_like(ref)
    np.add.at(ref, rows, terms)
    np.add.at(mass, rows, np.abs(terms))
    return ref * np.asarray(scale, np.float64), mass, count
