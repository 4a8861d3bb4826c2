"""GPU: ``voltrix.quantize_fp8``, ``voltrix.spmm_fp8`` and ``voltrix.autograd.SpMMFp8`` against the oracle of tests/spmm_fp8_oracle.py
(torch's CPU cast for the quantiser, the format's definition for the decoder, float64 for the sums).  Every comparison is over every
element.

Bounds, with ``u = 2^-23`` and ``k`` entries in the row:

    aggregation on the same bytes     |out - ref| <= (k + 2) u |scale[f]| sum_e |v_e dec_e|       (k - 1 additions or k fused
                                      multiply-adds, one multiply by the scale; twice the first-order sum)
    quantisation, finite inputs       |x - scale dec(q(x))| <= (2^-4 + 2^-20) |x| + 2^-10 scale   (half an ulp of 3 mantissa bits and
                                      the multiply's rounding; half the subnormal spacing 2^-9)
    end to end                        the second summed over the row with |v_e|, plus the first

Integer-valued codes, power-of-two scales and integer values: equality.  A 16-bit output is the fp32 output cast by torch, bit for bit.
"""
import numpy as np
import pytest
import torch

import spmm_fp8_oracle as oracle
from conftest import load_csr_fixture
from poisoned_alloc import poisoned

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
DEV = "cuda"
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
TABLE = oracle.decode_table()


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()]).cpu()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a), _bits(b)))


def _rows_of(codes, scale, dim):
    """``Fp8Rows`` on the device from uint8 codes [n, W] and a scale [W] (CPU tensors)."""
    from voltrix.fp8 import Fp8Rows

    scale = scale.float()
    return Fp8Rows(codes.to(DEV).view(torch.float8_e4m3fn), scale.to(DEV), (1.0 / scale).to(DEV), dim)


# ------------------------------------------------------------------------------------------------------------------- the patterns
class Pattern:
    def __init__(self, lengths, cols, num_cols):
        lengths, cols = np.asarray(lengths, np.int64), np.asarray(cols, np.int64)
        self.num_rows, self.num_cols, self.nnz = len(lengths), int(num_cols), int(lengths.sum())
        assert cols.size == self.nnz
        self.lengths, self.ip, self.cols = lengths, np.concatenate([[0], np.cumsum(lengths)]), cols
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(DEV)     # noqa: E731
        self.indptr, self.indices = dev(self.ip), dev(cols)


_CACHE = {}
HUB = 9


def _pattern(name):
    """"built": 37 rows x 61 columns, degrees 0, 1, 3, 4, 5, 8, 9 (both sides of the 4-entry batch and of a second one), a hub row of
    1,000 entries, duplicates, the last row empty.  "toy40", "skewed_1005": the committed fixtures."""
    if name not in _CACHE:
        if name == "built":
            rng = np.random.default_rng(23)
            lengths = [0, 1, 3, 4, 5, 8, 9, 2, 7, 1000] + [int(v) for v in rng.choice([0, 1, 3, 4, 5, 8, 9], 26)] + [0]
            lengths = np.asarray(lengths, np.int64)
            assert len(lengths) == 37 and lengths[HUB] == 1000 and lengths[-1] == 0
            rows = np.repeat(np.arange(37), lengths)
            cols = np.sort(rows * 61 + rng.integers(0, 61, rows.size)) % 61
            assert len(np.unique(rows * 61 + cols)) < rows.size - 500                  # duplicates are present
            _CACHE[name] = Pattern(lengths, cols, 61)
        else:
            g = load_csr_fixture(name)
            ip = np.asarray(g["indptr"], np.int64)
            _CACHE[name] = Pattern(ip[1:] - ip[:-1], g["indices"], int(g["num_nodes"]))
    return _CACHE[name]


# ------------------------------------------------------------------------------------------------ 1. decode, all 256 codes
def test_decode_of_all_256_codes_is_ocp_e4m3fn(cuda_device):
    """The identity pattern on 16 rows of 16 codes, scale 1: the output IS the decoder.  0x7f / 0xff NaN, 0x80 -> -0 with its sign,
    0x7e -> 448 and 0x01 -> 2^-9: the MI300 FNUZ encoding differs in every one of these."""
    import voltrix

    codes = torch.arange(256, dtype=torch.uint8).view(16, 16)
    rows = _rows_of(codes, torch.ones(16), 16)
    indptr = torch.arange(17, dtype=torch.int32, device=DEV)
    indices = torch.arange(16, dtype=torch.int32, device=DEV)
    table32 = torch.from_numpy(TABLE.astype(np.float32)).view(16, 16)
    nan = torch.isnan(table32)
    assert int(nan.sum()) == 2
    for dtype in DT.values():
        for values in (None, torch.ones(16, device=DEV)):
            out = voltrix.spmm_fp8(indptr, indices, rows, 16, values=values, out_dtype=dtype).cpu()
            want = table32.to(dtype)
            assert out.dtype == dtype and out.shape == (16, 16)
            assert bool(torch.equal(torch.isnan(out), nan))
            differ = (_bits(out) != _bits(want)) & ~nan
            assert not bool(differ.any()), (dtype, values is not None, [hex(c) for c in codes[differ].tolist()])
            assert bool(torch.signbit(out[8, 0])) and float(out[8, 0]) == 0.0 and not bool(torch.signbit(out[0, 0]))
    assert float(out[7, 14]) == 448.0 and float(out[0, 1]) == 2.0 ** -9


# ----------------------------------------------------------------------------------------------------- 2. the quantiser's bits
def _specials():
    """Every midpoint between adjacent codes and its fp32 neighbours, the subnormal range, +-448 and just beyond, +-0, +-inf."""
    finite = np.sort(np.unique(TABLE[~np.isnan(TABLE)]))
    mid = ((finite[:-1] + finite[1:]) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (finite[:-1] + finite[1:]) / 2)         # midpoints are fp32 numbers
    sub = np.linspace(-2.0 ** -6, 2.0 ** -6, 257).astype(np.float32)                    # steps of 2^-13 through the subnormals
    edge = np.array([448, 449, 464, 480, 1e6, 3e38], np.float32)
    edge = np.concatenate([edge, np.nextafter(np.float32(448), np.float32(1e9))[None], np.nextafter(np.float32(448), np.float32(0))[None]])
    pool = np.concatenate([mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf)), sub, edge, -edge,
                           np.array([0.0, -0.0, np.inf, -np.inf], np.float32), finite.astype(np.float32)])
    return torch.from_numpy(pool)


def _feat(n, dim, dtype, kind, seed):
    gen = torch.Generator().manual_seed(seed)
    if kind == "specials":
        pool = _specials()
        take = (torch.arange(n * dim) * 7 + seed) % pool.numel() if n * dim < pool.numel() else torch.arange(n * dim) % pool.numel()
        return pool[take].view(n, dim).to(dtype)
    x = torch.randn(n, dim, generator=gen) * 10.0 ** (torch.rand(n, dim, generator=gen) * 12 - 8)     # twelve decades
    if dim >= 2:
        x[:, dim // 2] = 0.0                                                                # a zero column
    return x.to(dtype)


def _check_rows(rows, feat_cpu, mode, what):
    n, dim = feat_cpu.shape
    width = (dim + 15) // 16 * 16
    # the torch formula where the data lives, bit for bit -- and the same formula on the CPU within one ulp: torch's fp32 division on
    # the device is not correctly rounded (measured: the last bit differs from the CPU's in some columns)
    on_device = oracle.scales(feat_cpu.to(DEV), mode.to(DEV) if isinstance(mode, torch.Tensor) else mode)
    on_host = oracle.scales(feat_cpu, mode)
    assert rows.dim == dim and rows.data.dtype == torch.float8_e4m3fn and rows.data.shape == (n, width) and rows.data.is_contiguous()
    for got, want, near in zip((rows.scale, rows.inv_scale), on_device, on_host):
        assert got.dtype == torch.float32 and got.shape == (width,)
        assert bool(torch.equal(_bits(got)[:dim], _bits(want.contiguous()))) and bool((got[dim:] == 1).all()), what
        assert bool(((got[:dim].cpu().double() - near.double()).abs() <= 2.0 ** -23 * near.double().abs()).all()), what
    got = rows.data.view(torch.uint8).cpu()
    want = oracle.quantize(feat_cpu, rows.inv_scale.cpu()[:dim])
    nan = oracle.is_nan_code(want)
    assert bool(torch.equal(oracle.is_nan_code(got), nan)), what
    differ = (got != want) & ~nan
    assert not bool(differ.any()), (what, int(differ.sum()), [(hex(int(a)), hex(int(b))) for a, b in zip(got[differ][:8], want[differ][:8])])
    assert not bool(got[:, dim:].any()), what                                               # padding bytes are 0x00
    return got


@pytest.mark.parametrize("dtype", list(DT))
def test_quantiser_bits_are_torchs_cast(cuda_device, dtype):
    import voltrix

    nans = 0
    for n in (1, 33):
        for dim in (1, 16, 17, 100, 1040):
            # the specials under power-of-two scales (a given tensor, and a scalar): ties stay ties
            feat = _feat(n, dim, DT[dtype], "specials", seed=n + dim)
            for mode in (torch.ones(dim), 2.0 ** (torch.arange(dim) % 5 - 2).float(), 0.5):
                got = _check_rows(voltrix.quantize_fp8(feat.to(DEV), scale=mode.to(DEV) if isinstance(mode, torch.Tensor) else mode),
                                  feat, mode, (dtype, n, dim, "specials"))
            # random data over twelve decades with a zero column: the three modes
            feat = _feat(n, dim, DT[dtype], "random", seed=100 + n + dim)
            given = (feat.float().abs().amax(dim=0) / 300 + 1e-6)                            # static calibration that saturates a little
            for mode in ("column", "tensor", given):
                _check_rows(voltrix.quantize_fp8(feat.to(DEV), scale=mode.to(DEV) if isinstance(mode, torch.Tensor) else mode),
                            feat, mode, (dtype, n, dim, "random", mode if isinstance(mode, str) else "given"))
            # a NaN under a given scale: that element alone
            feat[n // 2, dim // 3] = float("nan")
            got = _check_rows(voltrix.quantize_fp8(feat.to(DEV), scale=given.to(DEV)), feat, given, (dtype, n, dim, "nan"))
            assert int(oracle.is_nan_code(got[:, :dim]).sum()) == 1 and bool(oracle.is_nan_code(got[n // 2, dim // 3]))
            nans += 1
    assert nans == 10


@pytest.mark.parametrize("dtype", list(DT))
def test_quantiser_reads_strided_and_misaligned_operands(cuda_device, dtype):
    """A column slice of a wider tensor (on a 16-byte boundary: read in place through its row stride; off it: copied) and a contiguous
    view that starts 4 bytes off alignment give the bytes of their contiguous, aligned copies."""
    import voltrix

    per4 = 4 // DT[dtype].itemsize
    for n, dim in ((33, 100), (5, 17), (33, 1040), (1, 16)):
        wide = _feat(n, dim + 40, DT[dtype], "random", seed=dim).to(DEV)
        for first in (16, per4):                                         # byte offsets 16 * itemsize (aligned) and 4
            view = wide[:, first:first + dim]
            assert not view.is_contiguous() or n == 1
            assert (view.data_ptr() % 16 == 0) == (first == 16)
            want = voltrix.quantize_fp8(view.clone(), "column")
            got = voltrix.quantize_fp8(view, "column")
            assert _same_bits(got.data, want.data) and _same_bits(got.scale, want.scale) and _same_bits(got.inv_scale, want.inv_scale)
        flat = torch.zeros(n * dim + 64, dtype=DT[dtype], device=DEV)
        off = flat[per4:per4 + n * dim].view(n, dim)
        off.copy_(wide[:, :dim])
        assert off.is_contiguous() and off.data_ptr() % 16 == 4
        want = voltrix.quantize_fp8(off.clone(), "tensor")
        got = voltrix.quantize_fp8(off, "tensor")
        assert _same_bits(got.data, want.data)
        _check_rows(got, off.cpu(), "tensor", (dtype, n, dim, "offset"))


# ------------------------------------------------------------------------------------------------------------ 3. aggregation
def _operands(p, dim, kind, seed):
    """uint8 codes [num_cols, W], scale [W] and values [nnz] (CPU).  "ints": integer codes in [-3, 3], power-of-two scales, integer
    values; "random": every finite code, positive scales over four decades, normal values."""
    width = (dim + 15) // 16 * 16
    gen = torch.Generator().manual_seed(seed)
    if kind == "ints":
        x = torch.randint(-3, 4, (p.num_cols, dim), generator=gen).float()
        codes = oracle.quantize(x, torch.ones(dim))
        scale = 2.0 ** torch.randint(-3, 4, (width,), generator=gen).float()
        values = torch.randint(-3, 4, (p.nnz,), generator=gen).float()
    else:
        codes = torch.randint(0, 256, (p.num_cols, width), generator=gen, dtype=torch.int32).to(torch.uint8)
        codes[oracle.is_nan_code(codes)] = 0x7E
        codes[:, dim:] = 0
        scale = 10.0 ** (torch.rand(width, generator=gen) * 4 - 3)
        values = torch.randn(p.nnz, generator=gen)
    scale[dim:] = 1.0
    return codes, scale, values


@pytest.mark.parametrize("dim", [16, 48, 128, 1040])
@pytest.mark.parametrize("name", ["built", "toy40", "skewed_1005"])
def test_aggregation_against_float64_on_the_same_bytes(cuda_device, name, dim):
    import voltrix

    p = _pattern(name)
    worst = 0.0
    for kind in ("ints", "random"):
        codes, scale, values = _operands(p, dim, kind, seed=dim + len(name))
        rows = _rows_of(codes, scale, dim)
        for weighted in (False, True):
            v = values if weighted else None
            ref, mass, count = oracle.aggregate(p.ip, p.cols, codes.numpy(), scale.double().numpy(), None if v is None else v.numpy())
            ref, mass = ref[:, :dim], mass[:, :dim]
            out = {key: voltrix.spmm_fp8(p.indptr, p.indices, rows, p.num_rows, values=None if v is None else v.to(DEV), out_dtype=dt)
                   for key, dt in DT.items()}
            got = out["fp32"]
            assert got.dtype == torch.float32 and got.shape == (p.num_rows, dim) and got.is_contiguous()
            if kind == "ints":
                assert bool(np.array_equal(got.double().cpu().numpy(), ref)), (name, dim, weighted)
            else:
                err = np.abs(got.double().cpu().numpy() - ref)
                bound = (count[:, None] + 2) * U * np.abs(scale.double().numpy()[:dim]) * mass
                assert bool((err <= bound).all()), (name, dim, weighted, float((err / np.maximum(bound, 1e-300)).max()))
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert not bool(got[torch.from_numpy(count == 0).to(DEV)].any())               # a row without entries gives 0
            for key in ("fp16", "bf16"):
                assert _same_bits(out[key], got.to(DT[key])), (name, dim, weighted, key)
    print(f"{name} F={dim}: largest error over bound {worst:.3f}")


def test_a_pattern_object_goes_in_as_it_is_and_empty_operands(cuda_device):
    import voltrix
    from voltrix.autograd import CsrPattern

    p = _pattern("built")
    codes, scale, values = _operands(p, 48, "random", seed=3)
    rows = _rows_of(codes, scale, 48)
    want = voltrix.spmm_fp8(p.indptr, p.indices, rows, p.num_rows)
    pattern = CsrPattern(p.indptr, p.indices, p.num_rows, p.num_cols)
    assert _same_bits(voltrix.spmm_fp8(pattern, rows), want)
    holder = type("Holder", (), {"pattern": pattern})()                                   # what a Block / Subgraph is to this operator
    assert _same_bits(voltrix.spmm_fp8(holder, rows, out_dtype=torch.float16), want.half())
    # an empty pattern: every row is written as 0, for every output type and a width with padding
    empty_ptr = torch.zeros(6, dtype=torch.int32, device=DEV)
    none = torch.zeros(0, dtype=torch.int32, device=DEV)
    for dt in DT.values():
        with poisoned(0xFF) as state:
            out = voltrix.spmm_fp8(empty_ptr, none, rows, 5, out_dtype=dt)
        assert state.filled > 0 and out.shape == (5, 48) and out.dtype == dt and not bool(out.any()) and not bool(torch.signbit(out).any())
        out = voltrix.spmm_fp8(empty_ptr, none, rows, 5, values=torch.zeros(0, device=DEV), out_dtype=dt)
        assert out.shape == (5, 48) and not bool(out.any())
    # no rows; no gathered rows at all; no columns
    assert voltrix.spmm_fp8(empty_ptr[:1], none, rows, 0).shape == (0, 48)
    no_rows = voltrix.quantize_fp8(torch.zeros(0, 48, device=DEV))
    assert no_rows.data.shape == (0, 48) and bool((no_rows.scale == 1).all())
    assert not bool(voltrix.spmm_fp8(empty_ptr, none, no_rows, 5).any())
    no_cols = voltrix.quantize_fp8(torch.zeros(7, 0, device=DEV))
    assert no_cols.data.shape == (7, 0) and voltrix.spmm_fp8(empty_ptr, none, no_cols, 5).shape == (5, 0)
    assert voltrix.dequantize_fp8(no_cols).shape == (7, 0)


# ------------------------------------------------------------------------------------------------------------- 4. end to end
@pytest.mark.parametrize("mode", ["column", "tensor"])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_end_to_end_within_the_summed_quantisation_bound(cuda_device, mode, dtype):
    import voltrix

    p = _pattern("built")
    dim = 100
    gen = torch.Generator().manual_seed(41)
    feat = (torch.randn(p.num_cols, dim, generator=gen) * 10.0 ** (torch.rand(1, dim, generator=gen) * 4 - 2)).to(DT[dtype])
    values = torch.randn(p.nnz, generator=gen)
    rows = voltrix.quantize_fp8(feat.to(DEV), mode)
    out = voltrix.spmm_fp8(p.indptr, p.indices, rows, p.num_rows, values=values.to(DEV))
    x, v = feat.double().numpy(), values.double().numpy()
    scale = rows.scale.double().cpu().numpy()[:dim]
    row_of = np.repeat(np.arange(p.num_rows), p.lengths)
    ref, slack = np.zeros((p.num_rows, dim)), np.zeros((p.num_rows, dim))
    np.add.at(ref, row_of, v[:, None] * x[p.cols])
    np.add.at(slack, row_of, np.abs(v)[:, None] * ((2.0 ** -4 + 2.0 ** -20) * np.abs(x[p.cols]) + 2.0 ** -10 * scale))
    _, mass, count = oracle.aggregate(p.ip, p.cols, rows.data.view(torch.uint8).cpu().numpy(), scale_pad(scale), v)
    bound = slack + (count[:, None] + 2) * U * scale * mass[:, :dim]
    err = np.abs(out.double().cpu().numpy() - ref)
    print(f"end to end {mode} {dtype}: largest error over bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    # and the dequantised rows are what the aggregation sums
    back = voltrix.dequantize_fp8(rows)
    assert back.shape == (p.num_cols, dim) and back.dtype == torch.float32
    assert bool((np.abs(back.double().cpu().numpy() - x) <= (2.0 ** -4 + 2.0 ** -20) * np.abs(x) + 2.0 ** -10 * scale).all())


def scale_pad(scale):
    width = (len(scale) + 15) // 16 * 16
    return np.concatenate([scale, np.ones(width - len(scale))])


# ---------------------------------------------------------------------------------------------------------------- 5. same bits
def test_same_bits_on_every_call_and_on_poisoned_memory(cuda_device):
    import voltrix

    p = _pattern("skewed_1005")
    gen = torch.Generator().manual_seed(9)
    feat = torch.randn(p.num_cols, 100, generator=gen).half().to(DEV)
    values = torch.rand(p.nnz, generator=gen).to(DEV)

    def run(out_dtype):
        rows = voltrix.quantize_fp8(feat, "column")
        return rows, voltrix.spmm_fp8(p.indptr, p.indices, rows, p.num_rows, values=values, out_dtype=out_dtype)

    for out_dtype in (torch.float32, torch.bfloat16):
        rows, out = run(out_dtype)
        again_rows, again = run(out_dtype)
        assert _same_bits(rows.data, again_rows.data) and _same_bits(out, again)
        for byte in (0x00, 0xFF):
            with poisoned(byte) as state:
                p_rows, p_out = run(out_dtype)
            assert state.filled > 0
            assert _same_bits(rows.data, p_rows.data) and _same_bits(out, p_out), (out_dtype, byte)


# ------------------------------------------------------------------------------------------------------------------ 6. SpMMFp8
def _straight_through(pattern, grad, values, dtype):
    """``csr(values)^T grad`` by the existing row-gather kernel on the pattern's transpose, in ``dtype``."""
    from voltrix import capi

    out = torch.empty((pattern.num_cols, grad.shape[1]), dtype=torch.float32, device=DEV)
    t_values = None if values is None else values.float()[pattern.t_order].contiguous()
    capi.launch_spmm_csr_rows(pattern.t_indptr, pattern.t_indices, pattern.num_cols, grad.float().contiguous(), out,
                              torch.cuda.current_stream().cuda_stream, 1, t_values)
    return out.to(dtype)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_spmm_fp8_operator_forward_and_straight_through_backward(cuda_device, dtype):
    import voltrix
    from voltrix.autograd import CsrPattern, SpMMFp8

    p = _pattern("built")
    pattern = CsrPattern(p.indptr, p.indices, p.num_rows, p.num_cols)
    op = SpMMFp8(pattern)
    gen = torch.Generator().manual_seed(77)
    for dim in (48, 128):
        base = torch.randn(p.num_cols, dim, generator=gen).to(DT[dtype]).to(DEV)
        grad = torch.randn(p.num_rows, dim, generator=gen).to(DEV)
        for values in (None, torch.randn(p.nnz, generator=gen).to(DEV)):
            for scale in ("column", "tensor"):
                feat = base.clone().requires_grad_(True)
                out = op(feat, values=values, scale=scale)
                want = voltrix.spmm_fp8(p.indptr, p.indices, voltrix.quantize_fp8(base, scale), p.num_rows, values=values)
                assert _same_bits(out.detach(), want)
                out.backward(grad)
                assert feat.grad.dtype == DT[dtype] and _same_bits(feat.grad, _straight_through(pattern, grad, values, DT[dtype]))
    # the constructor's other form builds the same pattern
    assert _same_bits(SpMMFp8(p.indptr, p.indices, p.num_rows, p.num_cols)(base), op(base))
    with pytest.raises(ValueError, match="no gradient"):
        op(base, values=torch.ones(p.nnz, device=DEV, requires_grad=True))
    # an Fp8Rows in place of feat: no gradient, nothing quantised again
    rows = voltrix.quantize_fp8(base, "column")
    out = op(rows, values=values, out_dtype=torch.float16)
    assert not out.requires_grad and out.grad_fn is None
    assert _same_bits(out, voltrix.spmm_fp8(pattern, rows, values=values, out_dtype=torch.float16))


def test_spmm_fp8_operator_on_a_sampled_block(cuda_device):
    import voltrix
    from voltrix.autograd import SpMMFp8

    g = load_csr_fixture("skewed_1005")
    indptr = torch.from_numpy(np.asarray(g["indptr"], np.int32)).to(DEV)
    indices = torch.from_numpy(np.asarray(g["indices"], np.int32)).to(DEV)
    seeds = torch.arange(0, 1005, 5, dtype=torch.int32, device=DEV)
    (block,) = voltrix.sample_blocks(indptr, indices, seeds, [4], seed=5)
    assert block.num_src != block.num_dst and block.pattern.num_edges > 0
    gen = torch.Generator().manual_seed(5)
    feat = torch.randn(block.num_src, 48, generator=gen).half().to(DEV).requires_grad_(True)
    values = torch.rand(block.pattern.num_edges, generator=gen).to(DEV)
    grad = torch.randn(block.num_dst, 48, generator=gen).to(DEV)
    out = SpMMFp8(block.pattern)(feat, values=values)
    assert _same_bits(out.detach(), voltrix.spmm_fp8(block, voltrix.quantize_fp8(feat.detach()), values=values))
    out.backward(grad)
    assert feat.grad.dtype == torch.float16 and _same_bits(feat.grad, _straight_through(block.pattern, grad, values, torch.float16))
