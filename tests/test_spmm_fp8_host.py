"""CPU: the oracle of ``voltrix.spmm_fp8`` against torch's own e4m3fn cast, the quantisation-error bound on wide-range data, the
host-side argument contract of the two C entry points (one child process without a device: tests/spmm_fp8_abi_worker.py), the Python
argument errors that need no device, and the compiler's resource report of every kernel instantiation.  No GPU compute is called here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

import spmm_fp8_abi_worker as worker
import spmm_fp8_oracle as oracle
from kernel_resources import resource_usage
from voltrix import capi

WORKER = os.path.join(REPO, "tests", "spmm_fp8_abi_worker.py")
REPORT = os.path.join(REPO, "profiles", "spmm_fp8", "resource_usage.txt")


# ------------------------------------------------------------------------------------------------------------------------ the oracle
def test_the_decode_table_is_torchs_e4m3fn():
    table = oracle.decode_table()
    torchs = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy()
    nan = np.isnan(table)
    assert np.array_equal(np.nonzero(nan)[0], [0x7F, 0xFF]) and np.array_equal(nan, np.isnan(torchs))
    assert np.array_equal(table[~nan], torchs[~nan].astype(np.float64))
    assert np.array_equal(np.signbit(table[~nan]), np.signbit(torchs[~nan]))
    assert table[0x7E] == 448.0 and table[0xFE] == -448.0 and table[0x01] == 2.0 ** -9 and table[0x08] == 2.0 ** -6
    assert table[0x80] == 0.0 and np.signbit(table[0x80]) and not np.signbit(table[0x00])
    assert table[0x38] == 1.0 and table[0x07] == 7 * 2.0 ** -9


def test_the_oracle_quantiser_rounds_saturates_and_pads():
    x = torch.tensor([[0.0, -0.0, 448.0, 449.0, 1e9, float("inf"), -float("inf"), float("nan"), 2.0 ** -10, 3 * 2.0 ** -10,
                       1.0625, 1.1875, 464.0, -500.0, 2.0 ** -9, 2.0 ** -11, 17.0]])
    codes = oracle.quantize(x, torch.ones(17))
    assert codes.shape == (1, 32) and not codes[0, 17:].any()
    #       0     -0    448   sat   sat   inf   -inf  nan   ties to even: 0, 2^-8, 1.0, 1.25   sat   sat   2^-9  <half  the tie 17 -> 16
    want = [0x00, 0x80, 0x7E, 0x7E, 0x7E, 0x7E, 0xFE, None, 0x00, 0x02, 0x38, 0x3A, 0x7E, 0xFE, 0x01, 0x00, 0x58]
    for i, w in enumerate(want):
        if w is None:
            assert bool(oracle.is_nan_code(codes[0, i]))
        else:
            assert int(codes[0, i]) == w, (i, hex(int(codes[0, i])), hex(w))


def test_the_quantisation_error_bound_on_wide_range_data():
    """``|x - scale dec(q(x))| <= (2^-4 + 2^-20) |x| + 2^-10 scale`` for finite inputs: half an ulp of a 3-bit mantissa plus the fp32
    multiply's rounding, and half the subnormal spacing 2^-9 below the normal range."""
    rng = np.random.default_rng(11)
    table = oracle.decode_table()
    worst = 0.0
    for mode in ("column", "tensor", None):
        x = rng.standard_normal((4096, 24)) * 10.0 ** rng.uniform(-8, 4, (4096, 24))
        x[:, 3] = 0.0
        x[rng.integers(0, 4096, 64), rng.integers(0, 24, 64)] = 0.0
        feat = torch.from_numpy(x.astype(np.float32))
        if mode is None:
            scale = torch.from_numpy(10.0 ** rng.uniform(-3, 2, 24)).float()
            scale, inv = oracle.scales(feat, scale)
        else:
            scale, inv = oracle.scales(feat, mode)
        assert bool(torch.isfinite(inv).all()) and bool(torch.isfinite(scale).all()) and bool((scale > 0).all())
        codes = oracle.quantize(feat, inv)[:, :24].numpy()
        back = table[codes] * scale.double().numpy()
        exact = feat.double().numpy()
        bound = (2.0 ** -4 + 2.0 ** -20) * np.abs(exact) + 2.0 ** -10 * scale.double().numpy()
        if mode is None:                     # a given scale may saturate: the bound is for values inside +-448 scale
            inside = np.abs(exact) <= 448.0 * scale.double().numpy()
            exact, back, bound = exact[inside], back[inside], bound[inside]
        err = np.abs(exact - back)
        assert bool((err <= bound).all()), float((err / bound).max())
        worst = max(worst, float((err / bound).max()))
    print(f"largest quantisation error over bound: {worst:.3f}")
    assert worst > 0.5                       # the data reaches the bound's neighbourhood: it is not vacuous


def test_the_scales_of_tiny_huge_and_zero_columns():
    feat = torch.tensor([[0.0, 1e-45, 3e38, 2.0 ** -100, 1.0], [0.0, -1e-45, -1.0, 0.0, -448.0]])
    scale, inv = oracle.scales(feat, "column")
    assert scale[0] == 1 and inv[0] == 1                                             # a column of zeros
    assert bool(torch.isfinite(inv).all()) and bool(torch.isfinite(scale).all()) and bool((scale > 0).all())
    assert float(inv[1]) == 448.0 * 2.0 ** 100 and float(scale[1]) == np.float32(2.0 ** -100) / np.float32(448.0)
    assert float(scale[4]) == 1.0 and float(inv[4]) == 1.0
    from voltrix import fp8

    assert (fp8.AMAX_FLOOR, fp8.FP8_MAX) == (oracle.AMAX_FLOOR, oracle.FP8_MAX) == (2.0 ** -100, 448.0)


# ------------------------------------------------------------------------------------------------------------------ the C contract
@pytest.fixture(scope="module")
def answers():
    """``{case id: return code}`` of every case, from one child that cannot see a device."""
    run = subprocess.run([sys.executable, WORKER], env={**os.environ, "HIP_VISIBLE_DEVICES": "-1"}, capture_output=True, text=True,
                         timeout=600)
    lines = [json.loads(line) for line in run.stdout.splitlines() if line.startswith("{")]
    assert lines and "devices" in lines[0], f"the child said nothing (exit code {run.returncode}):\n{run.stderr[-3000:]}"
    assert lines[0]["devices"] == 0 and run.returncode != worker.EXIT_DEVICE_VISIBLE, \
        f"the child sees {lines[0]['devices']} device(s) with HIP_VISIBLE_DEVICES=-1: it made no library call"
    got = {line["id"]: line["rc"] for line in lines if "id" in line}
    assert run.returncode == 0 and "done" in lines[-1], f"exit code {run.returncode} after {len(got)} answers:\n{run.stderr[-3000:]}"
    assert lines[-1]["done"] == len(got) == len(worker.cases())
    return got


def test_the_entry_points_are_declared_bound_and_exported():
    import voltrix

    for name in worker.SYMBOLS:
        restype, argtypes = capi.SIGNATURES[name]
        assert restype is capi._I and argtypes[-1] is capi._P and len(argtypes) == len(worker.PARAMS[name]), name
        assert hasattr(capi.lib(), name) and not name.startswith("voltrix_launch_")
    assert "num_entries" in [p for p, _ in worker.PARAMS[worker.SPMM]]
    for wrapper in (capi.launch_quantize_fp8_rows, capi.launch_spmm_fp8):
        assert not hasattr(wrapper, "timer_label")
    assert capi.lib().voltrix_abi_version() == 2
    for name in ("Fp8Rows", "quantize_fp8", "dequantize_fp8", "spmm_fp8"):
        assert callable(getattr(voltrix, name))
    assert callable(voltrix.autograd.SpMMFp8)
    header = open(os.path.join(REPO, "voltrix-spmm_amd", "voltrix", "include", "voltrix", "spmm_fp8_kernels.hpp")).read()
    assert "#define VOLTRIX_SPMM_FP8_UNROLL 4 " in header


def test_every_call_of_the_contract_is_answered_as_the_header_says(answers):
    wrong = {case_id: (answers[case_id], expected) for case_id, _, _, expected in worker.cases() if answers[case_id] != expected}
    assert not wrong, f"(got, expected) by case: {wrong}"
    q, s = worker.QUANTIZE, worker.SPMM
    for symbol in worker.SYMBOLS:
        assert answers[f"{symbol}::baseline"] == worker.LAUNCH
        assert answers[f"{symbol}::rows=0"] == worker.OK and answers[f"{symbol}::rows=-1"] == worker.BAD
        for p in worker.SIXTEEN[symbol]:
            assert answers[f"{symbol}::{p}=NULL"] == answers[f"{symbol}::{p}+4"] == answers[f"{symbol}::{p}+8"] == worker.BAD
    assert answers[f"{s}::values=NULL"] == worker.LAUNCH and answers[f"{s}::values+2"] == worker.BAD
    assert answers[f"{s}::indptr+2"] == answers[f"{s}::indices+2"] == worker.BAD
    assert answers[f"{s}::embedding_dim16=17"] == worker.BAD
    assert answers[f"{s}::num_entries=-1"] == worker.BAD and answers[f"{s}::num_entries=2^31-1"] == worker.LAUNCH
    assert answers[f"{s}::out_dtype=3"] == answers[f"{s}::out_dtype=-1"] == answers[f"{q}::dtype=3"] == answers[f"{q}::dtype=-1"] == worker.BAD


# --------------------------------------------------------------------------------------------------------- Python argument errors
def test_argument_errors_are_value_errors_before_any_device_is_looked_at():
    import voltrix
    from voltrix.fp8 import Fp8Rows

    indptr = torch.tensor([0, 2, 2, 5], dtype=torch.int32)
    indices = torch.tensor([1, 1, 0, 2, 3], dtype=torch.int32)
    feat = torch.zeros(4, 20)                       # CPU tensors: a call past the checks would assert
    rows = Fp8Rows(torch.zeros(4, 32, dtype=torch.uint8).view(torch.float8_e4m3fn), torch.ones(32), torch.ones(32), 20)
    for bad in (torch.zeros(4), torch.zeros(4, 2, 4)):
        with pytest.raises(ValueError):
            voltrix.quantize_fp8(bad)                                   # feat not 2-D
    for bad in (torch.ones(19), torch.ones(1, 20), torch.ones(32), "row", "Column", None, [1.0] * 20):
        with pytest.raises(ValueError):
            voltrix.quantize_fp8(feat, scale=bad)                       # a scale tensor not [F] or scalar / an unknown string
    for good in ("column", "tensor", 0.5, torch.tensor(0.5), torch.ones(20)):
        with pytest.raises(AssertionError):
            voltrix.quantize_fp8(feat, scale=good)                      # past the checks: the CPU tensor is refused by an assertion
    for bad in (feat, rows.data, None, (rows.data, rows.scale)):
        with pytest.raises(ValueError):
            voltrix.spmm_fp8(indptr, indices, bad, 3)                   # rows not an Fp8Rows
    with pytest.raises(ValueError):
        voltrix.dequantize_fp8(feat)
    for bad in (torch.ones(4), torch.ones(6), torch.ones(5, 2)):
        with pytest.raises(ValueError):
            voltrix.spmm_fp8(indptr, indices, rows, 3, values=bad)      # values.numel() != indices.numel()
    for bad in (torch.float64, torch.int32, torch.float8_e4m3fn, None):
        with pytest.raises(ValueError):
            voltrix.spmm_fp8(indptr, indices, rows, 3, out_dtype=bad)   # out_dtype outside the three
    with pytest.raises(AssertionError):
        voltrix.spmm_fp8(indptr, indices, rows, 3, values=torch.ones(5), out_dtype=torch.bfloat16)
    # dequantize is torch ops: it runs on the CPU
    back = voltrix.dequantize_fp8(Fp8Rows(torch.full((2, 16), 0x38, dtype=torch.uint8).view(torch.float8_e4m3fn),
                                          torch.full((16,), 0.5), torch.full((16,), 2.0), 3))
    assert back.shape == (2, 3) and back.dtype == torch.float32 and bool((back == 0.5).all())
    # the autograd operator needs a pattern, which needs a device -- a stand-in with what it reads
    op = voltrix.autograd.SpMMFp8.__new__(voltrix.autograd.SpMMFp8)
    op.pattern = type("Counts", (), {"num_edges": 5, "num_cols": 4, "num_rows": 3, "indices": indices, "indptr": indptr})()
    with pytest.raises(ValueError, match="no gradient"):
        op(feat, values=torch.ones(5, requires_grad=True))
    for bad in (lambda: op(torch.zeros(4)), lambda: op(feat, values=torch.ones(4)), lambda: op(feat, scale="rows"),
                lambda: op(feat, scale=torch.ones(3)), lambda: op(feat, out_dtype=torch.float64),
                lambda: op(rows, values=torch.ones(4)), lambda: op(rows, out_dtype=torch.int8)):
        with pytest.raises(ValueError):
            bad()


# --------------------------------------------------------------------------------------------------------- the compiler's report
SOURCE = r'''
#include "voltrix/spmm_fp8_kernels.hpp"
#define A(TO, W) template __global__ void voltrix::spmm_csr_rows_fp8_kernel<TO, W, 4>(const voltrix::Fp8CsrArgs<TO>);
#define Q(T) template __global__ void voltrix::quantize_fp8_rows_kernel<T>(const voltrix::Fp8QuantArgs<T>);
#define PER_TYPE(T) A(T, false) A(T, true) Q(T)
PER_TYPE(float) PER_TYPE(_Float16) PER_TYPE(uint16_t)
'''


def test_every_instantiation_compiles_without_scratch_spills_or_lds(tmp_path):
    usage, report = resource_usage(SOURCE, tmp_path, "spmm_fp8", ("spmm_csr_rows_fp8_kernel", "quantize_fp8_rows_kernel"))
    aggregate = [n for n in usage if "spmm_csr_rows_fp8_kernel" in n]
    quantize = [n for n in usage if "quantize_fp8_rows_kernel" in n]
    # aggregation: 3 output types x weighted or not; the quantiser: 3 input types
    assert len(aggregate) == 6 and len(quantize) == 3 and len(usage) == 9, sorted(usage)
    assert all(v == (0, 0, 0, 0) for v in usage.values()), {n: v for n, v in usage.items() if v != (0, 0, 0, 0)}
    # the report's remark lines are what profiles/spmm_fp8/resource_usage.txt holds (VOLTRIX_WRITE_PROFILES=1 writes the file anew)
    if os.environ.get("VOLTRIX_WRITE_PROFILES") == "1":
        os.makedirs(os.path.dirname(REPORT), exist_ok=True)
        with open(REPORT, "w") as f:
            f.write(report)
    assert open(REPORT).read() == report, "profiles/spmm_fp8/resource_usage.txt is not this tree's report"
