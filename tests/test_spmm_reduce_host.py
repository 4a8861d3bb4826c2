"""CPU: the max / min / mean aggregation entry points are declared, bound and exported; their argument checks answer on the host before
any launch; every kernel instantiation compiles for gfx950 without scratch and without spilled registers.  No GPU compute is called
here."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO

from voltrix import capi

HEADER = os.path.join(REPO, "include", "voltrix_capi.h")
VOLTRIX_OK, VOLTRIX_ERR_BAD_SHAPE = 0, 1
NAMES = ("voltrix_launch_spmm_csr_reduce", "voltrix_launch_spmm_csr_reduce_backward")
MAX, MIN, MEAN = 0, 1, 2


def test_header_declares_and_binding_lists_the_entry_points():
    import voltrix

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in capi.SYMBOLS
        assert hasattr(capi.lib(), name)
    assert capi.lib().voltrix_abi_version() == 2
    assert callable(voltrix.spmm_reduce) and callable(voltrix.autograd.SpMMReduce)
    from voltrix.spmm_reduce import spmm_reduce_backward      # (voltrix.spmm_reduce is the function)

    assert callable(spmm_reduce_backward) and voltrix.spmm_reduce.spmm_reduce_backward is spmm_reduce_backward
    assert capi.REDUCE_OPS == {"max": MAX, "min": MIN, "mean": MEAN}


def _ptrs(names, null, offset):
    # host buffers: every call below is refused (or has nothing to do) before a pointer is dereferenced or a kernel launched
    bufs = {k: np.zeros(4096 + 16, np.uint8) for k in names}
    base = {k: b.ctypes.data + (-b.ctypes.data) % 16 for k, b in bufs.items()}
    ptrs = {k: None if k in null else ctypes.c_void_p(base[k] + (offset[1] if offset and offset[0] == k else 0)) for k in names}
    return bufs, ptrs


def _forward(num_rows=4, dim=8, dtype=0, op=MAX, null=("arg",), offset=None):
    bufs, p = _ptrs(("indptr", "indices", "input", "output", "arg"), null, offset)
    rc = ctypes.c_int(-1)
    capi.lib().voltrix_launch_spmm_csr_reduce(p["indptr"], p["indices"], num_rows, dim, p["input"], dtype, op, p["output"], p["arg"],
                                              None, ctypes.byref(rc))
    return rc.value


def _backward(num_cols=4, nnz=6, dim=8, null=(), offset=None):
    bufs, p = _ptrs(("t_indptr", "t_indices", "t_order", "grad_out", "arg", "output"), null, offset)
    rc = ctypes.c_int(-1)
    capi.lib().voltrix_launch_spmm_csr_reduce_backward(p["t_indptr"], p["t_indices"], p["t_order"], num_cols, nnz, dim, p["grad_out"],
                                                       p["arg"], p["output"], None, ctypes.byref(rc))
    return rc.value


def test_forward_argument_validation_on_the_host():
    for name in ("indptr", "indices", "input", "output"):
        assert _forward(null=(name, "arg")) == VOLTRIX_ERR_BAD_SHAPE, name                 # a null pointer
    for name in ("input", "output", "arg"):
        assert _forward(null=(), offset=(name, 4)) == VOLTRIX_ERR_BAD_SHAPE, name           # 16 bytes wanted, off by 4
    for name in ("indptr", "indices"):
        assert _forward(offset=(name, 2)) == VOLTRIX_ERR_BAD_SHAPE, name                    # 4 bytes wanted, off by 2
    assert _forward(op=3) == VOLTRIX_ERR_BAD_SHAPE
    assert _forward(op=-1) == VOLTRIX_ERR_BAD_SHAPE
    assert _forward(dtype=3) == VOLTRIX_ERR_BAD_SHAPE
    assert _forward(dtype=-1) == VOLTRIX_ERR_BAD_SHAPE
    assert _forward(num_rows=-1) == VOLTRIX_ERR_BAD_SHAPE                                   # a negative size
    assert _forward(dim=-4) == VOLTRIX_ERR_BAD_SHAPE
    assert _forward(dim=6) == VOLTRIX_ERR_BAD_SHAPE                                         # fp32 rows: multiples of 4
    assert _forward(dim=12, dtype=1) == VOLTRIX_ERR_BAD_SHAPE                               # 16-bit rows: multiples of 8
    assert _forward(dim=12, dtype=2) == VOLTRIX_ERR_BAD_SHAPE
    assert _forward(op=MEAN, null=()) == VOLTRIX_ERR_BAD_SHAPE                              # the mean has no arg
    assert _forward(op=MEAN, null=(), num_rows=0) == VOLTRIX_ERR_BAD_SHAPE                  # ... checked before "nothing to do"
    assert _forward(dim=6, num_rows=0) == VOLTRIX_ERR_BAD_SHAPE                             # so is the width
    assert _forward(num_rows=0) == VOLTRIX_OK                                               # nothing to do: no launch
    assert _forward(dim=0) == VOLTRIX_OK
    assert _forward(num_rows=0, null=("indptr", "indices", "input", "output", "arg")) == VOLTRIX_OK


def test_backward_argument_validation_on_the_host():
    for name in ("t_indptr", "t_indices", "t_order", "grad_out", "arg", "output"):
        assert _backward(null=(name,)) == VOLTRIX_ERR_BAD_SHAPE, name                       # a null pointer
    for name in ("grad_out", "arg", "output"):
        assert _backward(offset=(name, 4)) == VOLTRIX_ERR_BAD_SHAPE, name                   # 16 bytes wanted, off by 4
    for name in ("t_indptr", "t_indices", "t_order"):
        assert _backward(offset=(name, 2)) == VOLTRIX_ERR_BAD_SHAPE, name                   # 4 bytes wanted, off by 2
    assert _backward(num_cols=-1) == VOLTRIX_ERR_BAD_SHAPE
    assert _backward(nnz=-1) == VOLTRIX_ERR_BAD_SHAPE
    assert _backward(nnz=2 ** 31) == VOLTRIX_ERR_BAD_SHAPE                                  # nnz > INT_MAX
    assert _backward(dim=-4) == VOLTRIX_ERR_BAD_SHAPE
    assert _backward(dim=6) == VOLTRIX_ERR_BAD_SHAPE                                        # a lane owns 4 features
    assert _backward(dim=6, num_cols=0) == VOLTRIX_ERR_BAD_SHAPE
    assert _backward(num_cols=0) == VOLTRIX_OK
    assert _backward(dim=0) == VOLTRIX_OK
    assert _backward(num_cols=0, null=("t_indptr", "t_indices", "t_order", "grad_out", "arg", "output")) == VOLTRIX_OK


def test_a_bad_reduce_is_a_value_error():
    import voltrix

    for reduce in ("sum", "amax", "", None):
        with pytest.raises(ValueError):                      # raised before any tensor is looked at
            voltrix.spmm_reduce(None, None, None, 0, reduce=reduce)
        with pytest.raises(ValueError):
            voltrix.autograd.SpMMReduce(None, reduce=reduce)
    with pytest.raises(ValueError):
        voltrix.spmm_reduce(None, None, None, 0, reduce="mean", return_arg=True)


SOURCE = r'''
#include "voltrix/spmm_csr_reduce_kernels.hpp"
#define K(T, OP, ARG) template __global__ void voltrix::spmm_csr_reduce_kernel<T, OP, ARG, 4>(const voltrix::CsrReduceArgs<T>);
#define ALL(T) K(T, 0, true) K(T, 0, false) K(T, 1, true) K(T, 1, false) K(T, 2, false)
ALL(float) ALL(_Float16) ALL(uint16_t)
template __global__ void voltrix::spmm_csr_reduce_backward_kernel<4>(const voltrix::CsrReduceBackwardArgs);
'''


def test_every_instantiation_compiles_without_scratch_or_spills(tmp_path):
    src = tmp_path / "spmm_reduce.hip"
    src.write_text(SOURCE)
    inc = os.path.join(REPO, "voltrix-spmm_amd", "voltrix", "include")
    run = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", inc,
                          "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", str(tmp_path / "spmm_reduce.o")],
                         capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    usage = {}
    for block in run.stderr.split("remark: Function Name: ")[1:]:
        name = block.split(" ")[0].strip()
        if "spmm_csr_reduce" in name:
            grab = lambda key: int(re.search(key + r": (\d+)", block).group(1))  # noqa: E731
            usage[name] = (grab(r"ScratchSize \[bytes/lane\]"), grab("SGPRs Spill"), grab("VGPRs Spill"))
    # {fp32, fp16, bf16} x ({max, min} x {with, without arg} + mean), and the backward
    forward = [n for n in usage if "spmm_csr_reduce_kernel" in n]
    assert len(forward) == 15 and len([n for n in usage if "spmm_csr_reduce_backward_kernel" in n]) == 1, sorted(usage)
    assert len(usage) == 16 and all(v == (0, 0, 0) for v in usage.values()), usage
