"""CPU: ``voltrix.spmm_rel``'s float64 oracle on a pattern small enough to work out by hand, the host-side argument contract of its
three C entry points (one child process without a device: tests/spmm_rel_abi_worker.py), the compiler's resource report of every kernel
instantiation, ``TypeIndex``'s tables, and the Python argument errors that need no device.  No GPU compute is called here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

import spmm_rel_abi_worker as worker
import spmm_rel_oracle as oracle
from kernel_resources import resource_usage
from voltrix import capi

WORKER = os.path.join(REPO, "tests", "spmm_rel_abi_worker.py")
REPORT = os.path.join(REPO, "profiles", "spmm_rel", "resource_usage.txt")

# ------------------------------------------------------------------------------------------------- the oracle, worked out by hand
# 4 rows x 4 columns, F = 2, R = 3 (type 1 unused), B = 2:  row 0 = (c1, c1) -- a duplicate --, row 1 empty, row 2 = (c0, c2, c3),
# row 3 = (c2)
INDPTR = np.array([0, 2, 2, 5, 6])
INDICES = np.array([1, 1, 0, 2, 3, 2])
ETYPE = np.array([0, 2, 2, 0, 0, 2])
FEAT = np.array([[1, -2], [2, 0.5], [-1, 3], [0, -1]], np.float64)
COEF = np.array([[1, 2], [5, 5], [-1, 0.5]], np.float64)
WEIGHT = np.array([1, 2, 0.5, 1, 2, -1], np.float64)
#   c[e] = w_e coef[etype_e]:   [1, 2]  [-2, 1]  [-0.5, 0.25]  [1, 2]  [2, 4]  [1, -0.5]
#   x[e] = feat[col_e]:         [2, .5] [2, .5]  [1, -2]       [-1, 3] [0, -1] [-1, 3]
GRAD = np.array([[[1, 2], [0, -1]], [[5, 5], [5, 5]], [[-1, 3], [2, 1]], [[2, -2], [1, 0]]], np.float64)      # [4, B, F]

FORWARD = [[[-2, -0.5], [6, 1.5]], [[0, 0], [0, 0]], [[-1.5, 2], [-1.75, 1.5]], [[-1, 3], [0.5, -1.5]]]
FORWARD_UNWEIGHTED_ROW0 = [[0, 0], [5, 1.25]]                 # [1, 2] x + [-1, 0.5] x
#   sum_b c[e, b] g[row_e, b]:  [1, 0]  [-2, -5]  [1, -1.25]  [3, 5]  [6, 10]  [1.5, -2]
GRAD_FEAT = [[1, -1.25], [-1, -5], [4.5, 3], [6, 10]]
#   w_e <g[row_e, b], x[e]>:    [3, -.5]  [6, -1]  [-3.5, 0]  [10, 1]  [-6, -2]  [8, 1]
GRAD_COEF = [[7, -1.5], [0, 0], [10.5, 0]]
TYPE_NORM = [1, 1, 1, 0.5, 0.5, 1]


def test_the_oracle_on_a_pattern_worked_out_by_hand():
    out, mass, count = oracle.forward(INDPTR, INDICES, ETYPE, FEAT, COEF, WEIGHT)
    assert np.array_equal(out, np.array(FORWARD, np.float64))
    assert np.array_equal(count, [2, 0, 3, 1]) and np.array_equal(mass[0], [[6, 1.5], [6, 1.5]]) and not mass[1].any()
    assert bool((mass >= np.abs(out)).all())
    assert np.array_equal(oracle.forward(INDPTR, INDICES, ETYPE, FEAT, COEF)[0][0], np.array(FORWARD_UNWEIGHTED_ROW0, np.float64))
    d, mass, count = oracle.grad_feat(INDPTR, INDICES, ETYPE, GRAD, COEF, 4, WEIGHT)
    assert np.array_equal(d, np.array(GRAD_FEAT, np.float64)) and np.array_equal(count, [1, 2, 2, 1])
    assert np.array_equal(mass[1], [1 + 0 + 2 + 0, 2 + 2 + 4 + 1])
    d, mass, count = oracle.grad_coef(INDPTR, INDICES, ETYPE, GRAD, FEAT, 3, WEIGHT)
    assert np.array_equal(d, np.array(GRAD_COEF, np.float64)) and np.array_equal(count, [3, 0, 3])
    assert not d[1].any() and not mass[1].any()                                   # the unused type: a zero gradient
    assert np.array_equal(mass[0], [2 + 1 + 1 + 9 + 2 * 3, 0.5 + 2 + 3 + 2 * 1])
    # coef = I_R is the plain per-relation sum
    out, _, _ = oracle.forward(INDPTR, INDICES, ETYPE, FEAT, np.eye(3))
    assert np.array_equal(out[2], [[-1, 2], [0, 0], [1, -2]]) and np.array_equal(out[0], [[2, 0.5], [0, 0], [2, 0.5]])


def test_type_norm_and_the_contract_on_the_transpose_through_t_order():
    import torch

    import voltrix

    assert np.array_equal(oracle.type_norm(INDPTR, ETYPE), TYPE_NORM)
    got = voltrix.spmm_rel.type_norm(torch.from_numpy(INDPTR).int(), torch.from_numpy(ETYPE).int(), 3)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), np.array(TYPE_NORM, np.float32))
    # what the kernel runs for grad_feat: on the transposed CSR, etype and weight read through t_order -- the scatter by definition
    t_indptr, t_indices, t_order = oracle.transpose(INDPTR, INDICES, 4)
    assert np.array_equal(t_indptr, [0, 1, 3, 5, 6]) and np.array_equal(t_indices, [2, 0, 0, 2, 3, 2])
    assert np.array_equal(t_order, [2, 0, 1, 3, 5, 4])
    d, mass, count = oracle.contract(t_indptr, t_indices, t_order, ETYPE, GRAD, COEF, WEIGHT)
    want = oracle.grad_feat(INDPTR, INDICES, ETYPE, GRAD, COEF, 4, WEIGHT)
    assert np.array_equal(d, np.array(GRAD_FEAT, np.float64)) and np.array_equal(mass, want[1]) and np.array_equal(count, want[2])
    # without the indirection the transposed entries would read other entries' types and weights
    assert not np.array_equal(oracle.contract(t_indptr, t_indices, np.arange(6), ETYPE, GRAD, COEF, WEIGHT)[0], d)


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
    for wrapper in (capi.launch_spmm_rel, capi.launch_spmm_rel_contract, capi.launch_spmm_rel_dots):
        assert not hasattr(wrapper, "timer_label")
    assert (capi.REL_BASIS_TILE, capi.REL_MAX_TYPES, capi.REL_MAX_BASES) == (voltrix.spmm_rel.BASIS_TILE, worker.MAX_TYPES, worker.MAX_BASES)
    assert callable(voltrix.spmm_rel) and callable(voltrix.autograd.SpMMRel)
    from voltrix.spmm_rel import BASIS_TILE, CHUNK, TypeIndex, grad_coef, grad_feat, type_norm      # (voltrix.spmm_rel is the function)

    assert voltrix.spmm_rel.grad_feat is grad_feat and voltrix.spmm_rel.grad_coef is grad_coef and voltrix.spmm_rel.type_norm is type_norm
    assert voltrix.spmm_rel.TypeIndex is TypeIndex and voltrix.spmm_rel.BASIS_TILE == BASIS_TILE == 8
    assert voltrix.spmm_rel.CHUNK == CHUNK == 512
    header = open(os.path.join(REPO, "voltrix-spmm_amd", "voltrix", "include", "voltrix", "spmm_rel_kernels.hpp")).read()
    assert f"#define VOLTRIX_SPMM_REL_TILE {BASIS_TILE} " in header and "#define VOLTRIX_SPMM_REL_COEF_LDS 0 " in header and "kRelMaxTypes = 65536;" in header and "kRelMaxBases = 1024;" in header


def test_every_call_of_the_contract_is_answered_as_the_header_says(answers):
    wrong = {case_id: (answers[case_id], expected) for case_id, _, _, expected in worker.cases() if answers[case_id] != expected}
    assert not wrong, f"(got, expected) by case: {wrong}"
    # the table of the issue, every symbol: a few of its rows by name
    for symbol in worker.SYMBOLS:
        assert answers[f"{symbol}::baseline"] == worker.LAUNCH
        assert answers[f"{symbol}::num_entries=2^31"] == worker.BAD and answers[f"{symbol}::num_entries=2^31-1"] == worker.LAUNCH
        assert answers[f"{symbol}::rows=0"] == answers[f"{symbol}::embedding_dim=0"] == answers[f"{symbol}::num_bases=0"] == worker.OK
        assert answers[f"{symbol}::num_bases=limit"] == worker.LAUNCH and answers[f"{symbol}::num_bases=limit+1"] == worker.BAD
        assert answers[f"{symbol}::weight=NULL"] == worker.LAUNCH
    assert answers[f"{worker.CONTRACT}::order=NULL"] == worker.LAUNCH
    for symbol in (worker.FORWARD, worker.CONTRACT):
        assert answers[f"{symbol}::num_types=limit"] == worker.LAUNCH and answers[f"{symbol}::num_types=limit+1"] == worker.BAD


# --------------------------------------------------------------------------------------------------------- the compiler's report
SOURCE = r'''
#include "voltrix/spmm_rel_kernels.hpp"
#define K(T, BT) template __global__ void voltrix::spmm_rel_kernel<T, BT, 4>(const voltrix::SpmmRelArgs<T>);
#define D(T) template __global__ void voltrix::spmm_rel_dots_kernel<T, 4>(const voltrix::SpmmRelDotsArgs<T>);
#define PER_TYPE(T) K(T, 4) K(T, 8) D(T)
PER_TYPE(float) PER_TYPE(_Float16) PER_TYPE(uint16_t)
template __global__ void voltrix::spmm_rel_contract_kernel<4, 4>(const voltrix::SpmmRelContractArgs);
'''


def test_every_instantiation_compiles_without_scratch_spills_or_lds(tmp_path):
    usage, report = resource_usage(SOURCE, tmp_path, "spmm_rel", ("spmm_rel_kernel", "spmm_rel_contract_kernel", "spmm_rel_dots_kernel"))
    forward = [n for n in usage if "spmm_rel_kernel" in n]
    dots = [n for n in usage if "spmm_rel_dots_kernel" in n]
    contract = [n for n in usage if "spmm_rel_contract_kernel" in n]
    # forward: tiles {4, 8} x 3 types; dots: 3 types; the contraction reads fp32 alone
    assert len(forward) == 6 and len(dots) == 3 and len(contract) == 1 and len(usage) == 10, sorted(usage)
    # the coefficient table is read by plain loads: no LDS
    assert all(v == (0, 0, 0, 0) for v in usage.values()), {n: v for n, v in usage.items() if v != (0, 0, 0, 0)}
    # the report's remark lines are what profiles/spmm_rel/resource_usage.txt holds (VOLTRIX_WRITE_PROFILES=1 writes the file anew)
    if os.environ.get("VOLTRIX_WRITE_PROFILES") == "1":
        with open(REPORT, "w") as f:
            f.write(report)
    assert open(REPORT).read() == report, "profiles/spmm_rel/resource_usage.txt is not this tree's report"


# --------------------------------------------------------------------------------------------------------------- TypeIndex (CPU)
def test_type_index_tables_and_the_types_it_refuses():
    import torch

    from voltrix.spmm_rel import CHUNK, TypeIndex

    etype = torch.from_numpy(ETYPE).int()
    index = TypeIndex(etype, 3)
    assert index.order.dtype == torch.int32 and index.order.tolist() == [0, 3, 4, 1, 2, 5]           # stable by type
    assert index.chunk_ptr.tolist() == [0, 3, 6] and index.type_ptr.tolist() == [0, 1, 1, 2] and index.chunk_ids.tolist() == [0, 1]
    small = TypeIndex(etype, 4, chunk=2)                                                            # 3 entries: chunks of 2 and 1
    assert small.chunk_ptr.tolist() == [0, 2, 3, 5, 6] and small.type_ptr.tolist() == [0, 2, 2, 4, 4]
    # a long run: every chunk but a type's last holds CHUNK entries, and the chunks tile the sorted entries
    rng = np.random.default_rng(3)
    big = torch.from_numpy(rng.choice(5, size=4 * CHUNK + 77, p=[0.6, 0.0, 0.3, 0.05, 0.05])).int()
    index = TypeIndex(big, 5)
    ptr, tptr = index.chunk_ptr.numpy(), index.type_ptr.numpy()
    assert ptr[0] == 0 and ptr[-1] == big.numel() and (np.diff(ptr) > 0).all() and (np.diff(ptr) <= CHUNK).all()
    assert tptr[-1] == len(ptr) - 1 == index.num_chunks and tptr[2] == tptr[1]                      # type 1 has no chunk
    sorted_types = big.numpy()[index.order.numpy()]
    assert (np.diff(sorted_types) >= 0).all()
    for r in range(5):
        run = sorted_types[ptr[tptr[r]]:ptr[tptr[r + 1]]]
        assert (run == r).all() and len(run) == int((big == r).sum())
        assert (np.diff(ptr[tptr[r]:tptr[r + 1] + 1])[:-1] == CHUNK).all()
    assert int(tptr[1] - tptr[0]) > 2                                                               # more than 2 CHUNK entries of type 0
    empty = TypeIndex(torch.zeros(0, dtype=torch.int32), 3)
    assert empty.num_chunks == 0 and empty.chunk_ptr.tolist() == [0] and empty.type_ptr.tolist() == [0, 0, 0, 0]
    for bad in (3, -1):
        with pytest.raises(ValueError):
            TypeIndex(torch.tensor([0, 2, bad, 1], dtype=torch.int32), 3)
    with pytest.raises(ValueError):
        TypeIndex(etype, 0)


# ----------------------------------------------------------------------------------------------------- Python argument errors
def test_argument_errors_are_value_errors_before_any_device_is_looked_at():
    import torch

    import voltrix
    from voltrix.spmm_rel import TypeIndex, grad_coef, grad_feat

    indptr = torch.from_numpy(INDPTR).int()
    indices = torch.from_numpy(INDICES).int()
    etype = torch.from_numpy(ETYPE).int()
    feat, coef, weight = torch.zeros(4, 8), torch.zeros(3, 2), torch.ones(6)     # CPU tensors: a call past the checks would assert
    grad = torch.zeros(4, 2, 8)
    index = TypeIndex(etype, 3)
    calls = {
        "forward": lambda **k: voltrix.spmm_rel(indptr, indices, k.get("etype", etype), k.get("feat", feat), k.get("coef", coef), 4,
                                                k.get("weight", weight)),
        "grad_feat": lambda **k: grad_feat(indptr, indices, indices, k.get("etype", etype), k.get("grad", grad), k.get("coef", coef), 4,
                                           k.get("weight", weight)),
        "grad_coef": lambda **k: grad_coef(indptr, indices, k.get("etype", etype), index, k.get("grad", grad), k.get("feat", feat),
                                           k.get("weight", weight)),
    }
    for name, fn in calls.items():
        with pytest.raises(ValueError):
            fn(etype=etype[:5])                                   # etype.numel() != indices.numel()
        with pytest.raises(ValueError):
            fn(weight=torch.ones(5))                              # weight not [nnz]
        with pytest.raises(ValueError):
            fn(weight=torch.ones(6, 1))
        with pytest.raises(AssertionError):
            fn()                                                  # past the checks: the CPU tensors are refused by an assertion
    for name in ("forward", "grad_feat"):
        for bad in (torch.zeros(3), torch.zeros(3, 2, 1), torch.zeros(0, 2), torch.zeros(3, 1025)):
            with pytest.raises(ValueError):
                calls[name](coef=bad)                             # coef not [R, B] / outside the limits
    for name in ("forward", "grad_coef"):
        for bad in (torch.zeros(4), torch.zeros(4, 2, 4)):
            with pytest.raises(ValueError):
                calls[name](feat=bad)                             # feat not 2-D
    for name in ("grad_feat", "grad_coef"):
        for bad in (torch.zeros(4, 16), torch.zeros(4, 2, 8, 1)):
            with pytest.raises(ValueError):
                calls[name](grad=bad)                             # grad_out not [num_rows, B, F]
    with pytest.raises(ValueError):
        calls["grad_feat"](grad=torch.zeros(4, 3, 8))             # not coef's bases
    with pytest.raises(ValueError):
        calls["grad_coef"](grad=torch.zeros(5, 2, 8))             # not the pattern's rows
    with pytest.raises(ValueError):
        calls["grad_coef"](grad=torch.zeros(4, 2, 4))             # not feat's width
    with pytest.raises(ValueError):
        grad_coef(indptr, indices, etype, TypeIndex(etype[:5], 3), grad, feat)
    # the autograd operator: a weight that requires grad is refused, not silently given no gradient; the other errors are the same.
    # It needs a pattern, which needs a device -- a stand-in with what it reads
    op = voltrix.autograd.SpMMRel.__new__(voltrix.autograd.SpMMRel)
    op.pattern = type("Counts", (), {"num_edges": 6, "num_cols": 4, "indices": indices})()
    op.etype, op.num_types = etype, 3
    with pytest.raises(ValueError, match="no gradient"):
        op(feat, coef, torch.ones(6, requires_grad=True))
    for bad in (lambda: op(feat, torch.zeros(4, 2)), lambda: op(torch.zeros(4), coef), lambda: op(feat, coef, torch.ones(5)),
                lambda: op(feat, torch.zeros(2))):
        with pytest.raises(ValueError):
            bad()
