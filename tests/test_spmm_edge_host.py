"""CPU: ``voltrix.spmm_edge``'s float64 oracle on a pattern small enough to work out by hand, the host-side argument contract of its two
C entry points (one child process without a device: tests/spmm_edge_abi_worker.py), the compiler's resource report of every kernel
instantiation, and the Python argument errors that need no device.  No GPU compute is called here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

import spmm_edge_abi_worker as worker
import spmm_edge_oracle as oracle
from kernel_resources import resource_usage
from voltrix import capi

WORKER = os.path.join(REPO, "tests", "spmm_edge_abi_worker.py")
REPORT = os.path.join(REPO, "profiles", "spmm_edge", "resource_usage.txt")

# ------------------------------------------------------------------------------------------------- the oracle, worked out by hand
# 4 rows x 4 columns, F = 2:  row 0 = (c1, c1) -- a duplicate --, row 1 empty, row 2 = (c0, c2, c3), row 3 = (c2)
INDPTR = np.array([0, 2, 2, 5, 6])
INDICES = np.array([1, 1, 0, 2, 3, 2])
FEAT = np.array([[1, -2], [2, 0.5], [-1, 3], [0, -1]], np.float64)
EFEAT = np.array([[3, -0.5], [-1, 2], [2, 1], [0.5, -4], [4, 1], [-2, 2]], np.float64)
#   x + w per entry:  [5, 0]  [1, 2.5]  [3, -1]  [-0.5, -1]  [4, 0]  [-3, 5]      (entry 0 and entry 4 hold an exact zero: gate closed)
GRAD = np.array([[1, 2], [5, 5], [-1, 3], [2, -2]], np.float64)

FORWARD = {
    "mul": [[4, 0.75], [0, 0], [1.5, -15], [2, 6]],
    "add": [[6, 2.5], [0, 0], [6.5, -2], [-3, 5]],
    "add_relu": [[6, 2.5], [0, 0], [7, 0], [0, 5]],
    "copy": [[2, 1.5], [0, 0], [6.5, -2], [-2, 2]],
}
GRAD_EFEAT = {
    "mul": [[2, 1], [2, 1], [-1, -6], [1, 9], [0, -3], [-2, -6]],
    "add": [[1, 2], [1, 2], [-1, 3], [-1, 3], [-1, 3], [2, -2]],
    "copy": [[1, 2], [1, 2], [-1, 3], [-1, 3], [-1, 3], [2, -2]],
    "add_relu": [[1, 0], [1, 2], [-1, 0], [0, 0], [-1, 0], [0, -2]],
}
GRAD_FEAT = {
    "mul": [[-2, 3], [2, 3], [-4.5, -16], [-4, 3]],
    "add": [[-1, 3], [2, 4], [1, 1], [-1, 3]],
    "add_relu": [[-1, 0], [2, 2], [0, -2], [-1, 0]],
}


def test_the_oracle_on_a_pattern_worked_out_by_hand():
    for op, want in FORWARD.items():
        out, mass, count = oracle.forward(INDPTR, INDICES, None if op == "copy" else FEAT, EFEAT, op)
        assert np.array_equal(out, np.array(want, np.float64)), op
        assert np.array_equal(count, [2, 0, 3, 1]) and np.array_equal(mass[1], [0, 0]) and bool((mass >= np.abs(out)).all())
    assert np.array_equal(oracle.forward(INDPTR, INDICES, FEAT, EFEAT, "mul")[1], [[8, 1.25], [0, 0], [2.5, 15], [2, 6]])
    for op, want in GRAD_EFEAT.items():
        assert np.array_equal(oracle.grad_efeat(INDPTR, INDICES, GRAD, FEAT, EFEAT, op), np.array(want, np.float64)), op
    for op, want in GRAD_FEAT.items():
        d, mass, count = oracle.grad_feat(INDPTR, INDICES, GRAD, FEAT, EFEAT, op, 4)
        assert np.array_equal(d, np.array(want, np.float64)), op
        assert np.array_equal(count, [1, 2, 2, 1])
    # the exact zero of x + w in entry 0 (feature 1) and entry 4 (feature 1): the gate is closed there
    assert GRAD_EFEAT["add_relu"][0][1] == 0 and GRAD_EFEAT["add_relu"][4][1] == 0 and FEAT[1, 1] + EFEAT[0, 1] == 0


def test_the_oracle_s_order_indirection_and_gate_are_the_gradient_on_the_transpose():
    """What the kernel runs for ``grad_feat``: the forward on the transposed CSR with ``efeat`` read through ``t_order`` -- op mul on
    ``grad_out`` and op gate with ``self = feat`` -- is the scatter by definition."""
    t_indptr, t_indices, t_order = oracle.transpose(INDPTR, INDICES, 4)
    assert np.array_equal(t_indptr, [0, 1, 3, 5, 6]) and np.array_equal(t_indices, [2, 0, 0, 2, 3, 2])
    assert np.array_equal(t_order, [2, 0, 1, 3, 5, 4])
    mul, _, _ = oracle.forward(t_indptr, t_indices, GRAD, EFEAT, "mul", order=t_order)
    assert np.array_equal(mul, np.array(GRAD_FEAT["mul"], np.float64))
    gate, mass, _ = oracle.forward(t_indptr, t_indices, GRAD, EFEAT, "gate", order=t_order, self_rows=FEAT)
    assert np.array_equal(gate, np.array(GRAD_FEAT["add_relu"], np.float64))
    assert np.array_equal(mass, [[1, 0], [2, 2], [0, 2], [1, 0]])
    # without the indirection the transposed entries would read other rows of efeat
    assert not np.array_equal(oracle.forward(t_indptr, t_indices, GRAD, EFEAT, "mul")[0], mul)
    # a NaN stays a NaN through add_relu, and a closed gate passes nothing, a NaN included
    nan_feat = FEAT.copy()
    nan_feat[0, 0] = np.nan
    assert np.isnan(oracle.forward(INDPTR, INDICES, nan_feat, EFEAT, "add_relu")[0][2, 0])
    nan_grad = GRAD.copy()
    nan_grad[0, 1] = np.nan
    assert oracle.grad_efeat(INDPTR, INDICES, nan_grad, FEAT, EFEAT, "add_relu")[0, 1] == 0


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

    for name in (worker.FORWARD, worker.GRAD):
        restype, argtypes = capi.SIGNATURES[name]
        assert restype is capi._I and argtypes[-1] is capi._P and len(argtypes) == len(worker.PARAMS[name]), name
        assert hasattr(capi.lib(), name)
    assert capi.lib().voltrix_abi_version() == 2
    assert capi.EDGE_OPS == {"mul": worker.MUL, "add": worker.ADD, "add_relu": worker.ADD_RELU, "copy": worker.COPY, "gate": worker.GATE}
    assert not hasattr(capi.launch_spmm_edge, "timer_label") and not hasattr(capi.launch_spmm_edge_grad_efeat, "timer_label")
    assert callable(voltrix.spmm_edge) and callable(voltrix.autograd.SpMMEdge)
    from voltrix.spmm_edge import grad_efeat, grad_feat      # (voltrix.spmm_edge is the function)

    assert voltrix.spmm_edge.grad_efeat is grad_efeat and voltrix.spmm_edge.grad_feat is grad_feat
    with pytest.raises(capi.VoltrixError, match="return code 1"):
        capi.check(1, worker.FORWARD)


def test_every_call_of_the_contract_is_answered_as_the_header_says(answers):
    wrong = {case_id: (answers[case_id], expected) for case_id, _, _, expected in worker.cases() if answers[case_id] != expected}
    assert not wrong, f"(got, expected) by case: {wrong}"
    # the table of the issue, both symbols: a few of its rows by name
    for symbol in (worker.FORWARD, worker.GRAD):
        assert answers[f"{symbol}::baseline"] == worker.LAUNCH
        assert answers[f"{symbol}::num_entries=2^31"] == worker.BAD and answers[f"{symbol}::num_entries=2^31-1"] == worker.LAUNCH
        assert answers[f"{symbol}::num_rows=0"] == worker.OK and answers[f"{symbol}::embedding_dim=0"] == worker.OK
    assert answers[f"{worker.FORWARD}::pair=(1, 0)"] == worker.BAD
    assert answers[f"{worker.FORWARD}::gate self=NULL"] == worker.BAD and answers[f"{worker.FORWARD}::order=NULL"] == worker.LAUNCH
    assert answers[f"{worker.FORWARD}::copy input=NULL"] == worker.LAUNCH


# --------------------------------------------------------------------------------------------------------- the compiler's report
PAIRS = (("float", "float"), ("_Float16", "_Float16"), ("uint16_t", "uint16_t"), ("float", "_Float16"), ("float", "uint16_t"))
SOURCE = r'''
#include "voltrix/spmm_edge_kernels.hpp"
#define K(TI, TE, OP) template __global__ void voltrix::spmm_edge_kernel<TI, TE, OP, 4>(const voltrix::SpmmEdgeArgs<TI, TE>);
#define G(T, OP) template __global__ void voltrix::spmm_edge_grad_efeat_kernel<T, OP, 4>(const voltrix::SpmmEdgeGradArgs<T>);
#define PAIR(TI, TE) K(TI, TE, 0) K(TI, TE, 1) K(TI, TE, 2)
#define PER_TYPE(T) K(T, T, 3) K(float, T, 4) G(T, 0) G(T, 1) G(T, 2)
''' + "\n".join(f"PAIR({ti}, {te})" for ti, te in PAIRS) + "\nPER_TYPE(float) PER_TYPE(_Float16) PER_TYPE(uint16_t)\n"


def test_every_instantiation_compiles_without_scratch_spills_or_lds(tmp_path):
    usage, report = resource_usage(SOURCE, tmp_path, "spmm_edge", ("spmm_edge_kernel", "spmm_edge_grad_efeat_kernel"))
    forward = [n for n in usage if "spmm_edge_kernel" in n]
    grad = [n for n in usage if "spmm_edge_grad_efeat_kernel" in n]
    # {mul, add, add_relu} x 5 pairs + copy x 3 types + gate x 3 types (its gathered operand is fp32), and {mul, add, add_relu} x 3 types
    assert len(forward) == 3 * 5 + 3 + 3 == 21 and len(grad) == 9 and len(usage) == 30, sorted(usage)
    assert all(v == (0, 0, 0, 0) for v in usage.values()), {n: v for n, v in usage.items() if v != (0, 0, 0, 0)}
    # the report's remark lines are what profiles/spmm_edge/resource_usage.txt holds (VOLTRIX_WRITE_PROFILES=1 writes the file anew)
    if os.environ.get("VOLTRIX_WRITE_PROFILES") == "1":
        with open(REPORT, "w") as f:
            f.write(report)
    assert open(REPORT).read() == report, "profiles/spmm_edge/resource_usage.txt is not this tree's report"


# ----------------------------------------------------------------------------------------------------- Python argument errors
def test_argument_errors_are_value_errors_before_any_device_is_looked_at():
    import torch

    import voltrix
    from voltrix.spmm_edge import grad_efeat, grad_feat

    indptr = torch.tensor([0, 2, 2, 5, 6], dtype=torch.int32)
    indices = torch.tensor([1, 1, 0, 2, 3, 2], dtype=torch.int32)
    feat, efeat = torch.zeros(4, 8), torch.zeros(6, 8)            # CPU tensors: a call that got past the checks would assert on them
    for op in ("sum", "relu", "gate", "", None):
        with pytest.raises(ValueError):
            voltrix.spmm_edge(indptr, indices, feat, efeat, 4, op=op)
        with pytest.raises(ValueError):
            grad_efeat(indptr, indices, torch.zeros(4, 8), feat, efeat, op)
        with pytest.raises(ValueError):
            grad_feat(indptr, indices, indices, torch.zeros(4, 8), feat, efeat, op, 4)
    with pytest.raises(ValueError):
        voltrix.spmm_edge(indptr, indices, feat, efeat, 4, op="copy")               # feat given with copy
    with pytest.raises(ValueError):
        grad_feat(indptr, indices, indices, torch.zeros(4, 8), None, efeat, "copy", 4)   # copy has no feat
    for op in ("mul", "add", "add_relu"):
        with pytest.raises(ValueError):
            voltrix.spmm_edge(indptr, indices, None, efeat, 4, op=op)               # feat missing
        with pytest.raises(ValueError):
            voltrix.spmm_edge(indptr, indices, torch.zeros(4, 4), efeat, 4, op=op)  # widths differ
        with pytest.raises(ValueError):
            voltrix.spmm_edge(indptr, indices, torch.zeros(4, 2, 1), torch.zeros(6, 2, 4), 4, op=op)   # one value per head: spmm_heads
        with pytest.raises(ValueError):
            voltrix.spmm_edge(indptr, indices, feat, torch.zeros(5, 8), 4, op=op)   # efeat.shape[0] != indices.numel()
        with pytest.raises(ValueError):
            voltrix.spmm_edge(indptr, indices, feat, torch.zeros(6), 4, op=op)      # no feature dimension
        with pytest.raises(ValueError):
            grad_efeat(indptr, indices, torch.zeros(4, 4), feat, efeat, op)         # grad_out's width
    with pytest.raises(ValueError):
        voltrix.spmm_edge(indptr, indices, None, torch.zeros(5, 8), 4, op="copy")
    # the autograd operator raises the same errors; it needs a pattern, which needs a device -- a stand-in with the two counts it reads
    op = voltrix.autograd.SpMMEdge.__new__(voltrix.autograd.SpMMEdge)
    op.pattern = type("Counts", (), {"num_edges": 6, "num_cols": 4})()
    for bad in (lambda: op(feat, efeat, "sum"), lambda: op(feat, efeat, "copy"), lambda: op(None, efeat, "mul"),
                lambda: op(feat, torch.zeros(5, 8), "mul"), lambda: op(torch.zeros(4, 4), efeat, "add")):
        with pytest.raises(ValueError):
            bad()
