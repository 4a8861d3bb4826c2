"""CPU: the float64 oracle of ``voltrix.spmm_multi`` against closed forms, the ``var`` bound against a torch-fp32 model of the shifted
rule and of the naive ``E[x^2] - E[x]^2`` (the bound tells them apart), the host-side argument contract of the two C entry points (one
child process without a device: tests/spmm_multi_abi_worker.py), the Python argument errors that need no device, and the compiler's
resource report of every kernel instantiation.  No GPU compute is called here."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

import spmm_multi_abi_worker as worker
import spmm_multi_oracle as oracle
from kernel_resources import resource_usage
from voltrix import capi

WORKER = os.path.join(REPO, "tests", "spmm_multi_abi_worker.py")
REPORT = os.path.join(REPO, "profiles", "spmm_multi", "resource_usage.txt")
INF, NAN = float("inf"), float("nan")


# ------------------------------------------------------------------------------------------------------------------------ the oracle
def _csr(rows_of_cols):
    lengths = [len(r) for r in rows_of_cols]
    indptr = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32)
    return indptr, torch.tensor([c for r in rows_of_cols for c in r], dtype=torch.int32)


def test_the_oracle_against_closed_forms():
    eps = 1e-5
    #                0    1    2    3    4    5    6    7     8     9
    x = torch.tensor([1.0, 2.0, 3.0, 4.0, 7.5, 7.5, 7.5, INF, NAN, -INF])[:, None].repeat(1, 2)
    x[:, 1] = -x[:, 1]
    #       one entry  constant       1 2 3 4       empty  duplicates  inf      nan     -inf first   finite again
    rows = [[4],       [4, 5, 6, 5], [0, 1, 2, 3], [],    [1, 1, 3],  [0, 7],  [8, 2], [9, 0, 1],   [3, 0]]
    indptr, indices = _csr(rows)
    ref = oracle.forward(indptr, indices, x, len(rows), eps)
    col = lambda name: ref[name][:, 0].tolist()       # noqa: E731
    assert ref["deg"].tolist() == [1, 4, 4, 0, 3, 2, 2, 3, 2]
    # a row of one entry, a constant row: var == 0 exactly and std == sqrt(eps); the bound is 0 there
    for r in (0, 1):
        assert col("var")[r] == 0.0 and col("std")[r] == math.sqrt(eps) and col("var_bound")[r] == 0.0
        assert col("mean")[r] == col("max")[r] == col("min")[r] == 7.5 and col("sum")[r] == 7.5 * len(rows[r])
    assert col("argmax")[:2] == [0, 1] and col("argmin")[:2] == [0, 1]              # the first entry wins the ties
    # [1, 2, 3, 4]: mean 2.5, var 1.25; sum (x - x_first)^2 = 0 + 1 + 4 + 9
    assert (col("sum")[2], col("mean")[2], col("max")[2], col("min")[2], col("var")[2]) == (10.0, 2.5, 4.0, 1.0, 1.25)
    assert col("std")[2] == math.sqrt(1.25 + eps) and (col("argmax")[2], col("argmin")[2]) == (8, 5)
    assert col("var_bound")[2] == (4 + 4) * 2.0 ** -23 * (2 / 4) * 14.0
    assert col("std_bound")[2] == col("var_bound")[2] / col("std")[2] + 2.0 ** -22 * col("std")[2]
    # the mirrored column: max and min change places, the moments keep their size
    assert ref["max"][2, 1] == -1.0 and ref["min"][2, 1] == -4.0 and ref["var"][2, 1] == 1.25 and ref["argmax"][2, 1] == 5
    # an empty row: zeros everywhere, std too, args -1
    for name in ("sum", "mean", "max", "min", "var", "std", "var_bound", "std_bound"):
        assert col(name)[3] == 0.0, name
    assert col("argmax")[3] == col("argmin")[3] == -1
    # duplicates count twice: [2, 2, 4]
    assert col("mean")[4] == 8 / 3 and abs(col("var")[4] - 8 / 9) < 1e-15 and col("argmax")[4] == 11 and col("argmin")[4] == 9
    # inf / nan rows: NaN in var and std; max / min as torch.amax / amin; the finite row after them is untouched
    for r in (5, 6, 7):
        assert math.isnan(col("var")[r]) and math.isnan(col("std")[r]) and bool(ref["nonfinite"][r].all())
    assert col("max")[5] == INF and col("min")[5] == 1.0 and col("sum")[5] == INF
    assert math.isnan(col("max")[6]) and math.isnan(col("min")[6]) and col("argmax")[6] == col("argmin")[6] == 14
    assert col("min")[7] == -INF and col("max")[7] == 2.0 and col("argmin")[7] == 16 and col("argmax")[7] == 18
    assert (col("var")[8], col("mean")[8]) == (2.25, 2.5) and not bool(ref["nonfinite"][8].any())


def test_the_backward_oracle_against_closed_forms():
    x = torch.tensor([[1.0], [2.0], [3.0], [4.0], [9.0]])
    indptr, indices = _csr([[0, 1, 2, 3], [], [1, 1], [4]])
    one = lambda *v: torch.tensor([list(v)]).T.double()       # noqa: E731
    want, bound = oracle.backward(indptr, indices, x, 4, {"sum": one(1, 5, 10, 100)})
    assert want[:, 0].tolist() == [1, 21, 1, 1, 100] and bool((bound >= 0).all())
    want, _ = oracle.backward(indptr, indices, x, 4, {"mean": one(4, 5, 10, 100)})
    assert want[:, 0].tolist() == [1, 11, 1, 1, 100]
    want, _ = oracle.backward(indptr, indices, x, 4, {"max": one(1, 5, 10, 100), "min": one(2, 5, 20, 200)})
    assert want[:, 0].tolist() == [2, 30, 0, 1, 300]                     # the tie of row 2 goes to its first entry, once
    # var: 2 (x - mean) / d = (-0.75, -0.25, 0.25, 0.75); a constant row and a single entry pass nothing
    want, bound = oracle.backward(indptr, indices, x, 4, {"var": one(1, 5, 10, 100)})
    assert want[:, 0].tolist() == [-0.75, -0.25, 0.25, 0.75, 0.0] and bool((bound[:4] > 0).all())
    # std: (x - mean) / (d std)
    want, _ = oracle.backward(indptr, indices, x, 4, {"std": one(1, 5, 10, 100)}, eps=1e-5)
    std = math.sqrt(1.25 + 1e-5)
    assert np.allclose(want[:, 0].numpy(), [-1.5 / (4 * std), -0.5 / (4 * std), 0.5 / (4 * std), 1.5 / (4 * std), 0.0], rtol=1e-14, atol=0)


# ---------------------------------------------------------------------------------------------------- the bound tells the rules apart
def _shifted_fp32(rows_x):
    """The kernel's rule with torch fp32 ops, sequential over a row's entries: [d, F] fp32 -> var fp32 [F]."""
    k = rows_x[0]
    s1 = torch.zeros_like(k)
    s2 = torch.zeros_like(k)
    for e in range(rows_x.shape[0]):
        y = rows_x[e] - k
        s1 = s1 + y
        s2 = s2 + y * y
    d = torch.tensor(float(rows_x.shape[0]), dtype=torch.float32)
    m = s1 / d
    var = s2 / d - m * m
    return torch.where(var < 0, torch.zeros_like(var), var)


def _naive_fp32(rows_x):
    """E[x^2] - E[x]^2 from two sequential fp32 sums."""
    s = torch.zeros_like(rows_x[0])
    q = torch.zeros_like(rows_x[0])
    for e in range(rows_x.shape[0]):
        s = s + rows_x[e]
        q = q + rows_x[e] * rows_x[e]
    d = torch.tensor(float(rows_x.shape[0]), dtype=torch.float32)
    return q / d - (s / d) * (s / d)


def test_the_shifted_rule_is_inside_the_var_bound_and_the_naive_rule_outside_it():
    gen = torch.Generator().manual_seed(5)
    lengths = [1, 2, 3, 4, 5, 9, 17, 64, 301, 5003]
    num_cols, f = 400, 8
    worst = {"normal": 0.0, "ints": 0.0, "offset": 0.0}
    for kind in worst:
        if kind == "normal":
            x = torch.randn(num_cols, f, generator=gen)
        elif kind == "ints":
            x = torch.randint(-3, 0, (num_cols, f), generator=gen).float()
        else:
            x = 4096.0 + torch.randn(num_cols, f, generator=gen)
        rows = [torch.randint(0, num_cols, (d,), generator=gen).tolist() for d in lengths]
        indptr, indices = _csr(rows)
        ref = oracle.forward(indptr, indices, x, len(rows))
        for r, cols in enumerate(rows):
            gathered = x[torch.tensor(cols)]
            err = (_shifted_fp32(gathered).double() - ref["var"][r]).abs()
            assert bool((err <= ref["var_bound"][r]).all()), (kind, len(cols))
            if len(cols) > 1:
                worst[kind] = max(worst[kind], float((err / ref["var_bound"][r].clamp_min(1e-300)).max()))
            if kind == "offset" and len(cols) >= 2:
                miss = (_naive_fp32(gathered).double() - ref["var"][r]).abs()
                assert bool((miss > ref["var_bound"][r]).all()), (len(cols), float((miss / ref["var_bound"][r]).min()))
    print(f"shifted rule, worst error / bound: {worst}")
    assert all(v < 0.5 for v in worst.values())


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
        names = [p for p, _ in worker.PARAMS[name]]
        assert "num_entries" in names and "nnz" not in names
    for wrapper in (capi.launch_spmm_multi, capi.launch_spmm_multi_backward):
        assert not hasattr(wrapper, "timer_label")
    assert capi.lib().voltrix_abi_version() == 2
    assert callable(voltrix.spmm_multi) and callable(voltrix.spmm_multi.backward) and callable(voltrix.autograd.SpMMMulti)
    assert voltrix.spmm_multi.AGGREGATES == capi.MULTI_AGGREGATES == oracle.AGGREGATES
    assert tuple(s[len("slot_"):] for s in worker.SLOTS) == capi.MULTI_AGGREGATES


def test_every_call_of_the_contract_is_answered_as_the_header_says(answers):
    wrong = {case_id: (answers[case_id], expected) for case_id, _, _, expected in worker.cases() if answers[case_id] != expected}
    assert not wrong, f"(got, expected) by case: {wrong}"
    f, b = worker.FORWARD, worker.BACKWARD
    for symbol in worker.SYMBOLS:
        assert answers[f"{symbol}::baseline"] == worker.LAUNCH                      # the baseline is not refused
        assert answers[f"{symbol}::rows=0"] == worker.OK and answers[f"{symbol}::rows=-1"] == worker.BAD
        assert answers[f"{symbol}::embedding_dim=-1"] == answers[f"{symbol}::num_entries=-1"] == worker.BAD
        for p in worker.FOUR[symbol]:
            assert answers[f"{symbol}::{p}=NULL"] == answers[f"{symbol}::{p}+2"] == worker.BAD
        for p in worker.SIXTEEN[symbol]:
            assert answers[f"{symbol}::{p}+4"] == answers[f"{symbol}::{p}+8"] == worker.BAD
    for eps in ("0", "-1", "inf", "nan"):
        assert answers[f"{f}::eps={eps}"] == worker.BAD and answers[f"{f}::eps={eps} without std"] == worker.LAUNCH
    for s in worker.SLOTS:
        assert answers[f"{f}::{s} clashes"] == answers[f"{f}::{s}=6"] == worker.BAD
    assert answers[f"{f}::embedding_dim=25"] == answers[f"{b}::embedding_dim=6"] == worker.BAD
    assert answers[f"{f}::argmax without max"] == answers[f"{f}::args without selection"] == worker.BAD
    assert answers[f"{b}::no group"] == worker.BAD and answers[f"{b}::u alone"] == worker.LAUNCH
    assert len(worker.cases()) == 148


# --------------------------------------------------------------------------------------------------------- Python argument errors
def test_argument_errors_are_value_errors_before_any_device_is_looked_at():
    import voltrix

    indptr = torch.tensor([0, 2, 2, 5], dtype=torch.int32)
    indices = torch.tensor([1, 1, 0, 2, 3], dtype=torch.int32)
    feat = torch.zeros(4, 20)                       # CPU tensors: a call past the checks would assert
    for bad in ((), [], "mean", ("mean", "mean"), ("mean", "median"), ("Mean",), ("max", None), None, 3, ("sum", "std", "sum"),
                {"mean": 0}, ("argmax",)):
        with pytest.raises(ValueError):
            voltrix.spmm_multi(indptr, indices, feat, 3, aggrs=bad)
        with pytest.raises(ValueError):
            voltrix.autograd.SpMMMulti(indptr, indices, 3, aggrs=bad)
    for bad in (0, 0.0, -1e-5, INF, NAN, None, "1e-5", True):
        with pytest.raises(ValueError):
            voltrix.spmm_multi(indptr, indices, feat, 3, eps=bad)
        with pytest.raises(ValueError):
            voltrix.autograd.SpMMMulti(indptr, indices, 3, eps=bad)
    for good in (("mean", "max", "min", "std"), ["sum"], oracle.AGGREGATES, tuple(reversed(oracle.AGGREGATES))):
        with pytest.raises(AssertionError):
            voltrix.spmm_multi(indptr, indices, feat, 3, aggrs=good, eps=1)      # past the checks: the CPU tensors are refused
    # the backward: whole groups, one at least
    t = torch.zeros(3, 4)
    for bad in ({}, {"w": t}, {"w": t, "feat": t}, {"w": t, "mean": t}, {"g_max": t}, {"argmin": t.int()}, {"u": t, "feat": t},
                {"u": t, "g_min": t}):
        with pytest.raises(ValueError):
            voltrix.spmm_multi.backward(indptr, indices, indices, 4, **bad)


# --------------------------------------------------------------------------------------------------------- the compiler's report
SOURCE = r'''
#include "voltrix/spmm_multi_kernels.hpp"
#define F(T, M2, SEL) template __global__ void voltrix::spmm_multi_kernel<T, M2, SEL, 4>(const voltrix::SpmmMultiArgs<T>);
#define PER_TYPE(T) F(T, false, 0) F(T, false, 1) F(T, false, 2) F(T, true, 0) F(T, true, 1) F(T, true, 2)
PER_TYPE(float) PER_TYPE(_Float16) PER_TYPE(uint16_t)
#define B(U, W, S) template __global__ void voltrix::spmm_multi_backward_kernel<U, W, S, 4>(const voltrix::SpmmMultiBackwardArgs);
B(false, false, true) B(false, true, false) B(false, true, true) B(true, false, false) B(true, false, true) B(true, true, false)
B(true, true, true)
'''


def test_every_instantiation_compiles_without_scratch_spills_or_lds(tmp_path):
    usage, report = resource_usage(SOURCE, tmp_path, "spmm_multi", ("spmm_multi_kernel", "spmm_multi_backward_kernel"))
    forward = [n for n in usage if "spmm_multi_kernel" in n]
    backward = [n for n in usage if "spmm_multi_backward_kernel" in n]
    # forward: 3 types x second moment or not x {no selection, values, values + args}; backward: the non-empty subsets of {u, w, select}
    assert len(forward) == 18 and len(backward) == 7 and len(usage) == 25, sorted(usage)
    assert all(v == (0, 0, 0, 0) for v in usage.values()), {n: v for n, v in usage.items() if v != (0, 0, 0, 0)}
    # the report's remark lines are what profiles/spmm_multi/resource_usage.txt holds (VOLTRIX_WRITE_PROFILES=1 writes the file anew)
    if os.environ.get("VOLTRIX_WRITE_PROFILES") == "1":
        os.makedirs(os.path.dirname(REPORT), exist_ok=True)
        with open(REPORT, "w") as f:
            f.write(report)
    assert open(REPORT).read() == report, "profiles/spmm_multi/resource_usage.txt is not this tree's report"
