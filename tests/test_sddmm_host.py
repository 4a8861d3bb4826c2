"""CPU: the sampled dense-dense product's C-ABI entry point is declared, bound and exported; its argument checks answer on the host
before any launch; every kernel instantiation compiles for gfx950 without scratch.  No GPU compute is called here."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import REPO

from voltrix import capi

HEADER = os.path.join(REPO, "include", "voltrix_capi.h")
VOLTRIX_OK, VOLTRIX_ERR_BAD_SHAPE = 0, 1
F32, F16, BF16 = 0, 1, 2


def test_header_declares_and_binding_lists_the_entry_point():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bvoltrix_launch_sddmm_csr\s*\(", text)
    assert "voltrix_launch_sddmm_csr" in capi.SYMBOLS
    assert hasattr(capi.lib(), "voltrix_launch_sddmm_csr")


def _call(num_rows=4, nnz=6, width=16, x_dtype=F32, y_dtype=F16, x_offset=0, out_null=False):
    # host buffers: every call below is refused (or has nothing to do) before a pointer is dereferenced or a kernel launched
    indptr = np.zeros(num_rows + 1, np.int32)
    indices = np.zeros(max(nnz, 1), np.int32)
    x = np.zeros(64 * 64 + 16, np.uint8)
    y = np.zeros(64 * 64, np.uint8)
    out = np.zeros(max(nnz, 1), np.float32)
    base = x.ctypes.data + (-x.ctypes.data) % 16                    # 16-byte aligned
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)                 # noqa: E731
    yptr = y.ctypes.data + (-y.ctypes.data) % 16
    rc = ctypes.c_int(-1)
    capi.lib().voltrix_launch_sddmm_csr(ptr(indptr), ptr(indices), ctypes.c_int(num_rows), ctypes.c_int64(nnz), ctypes.c_int(width),
                                        ctypes.c_void_p(base + x_offset), ctypes.c_int(x_dtype), ctypes.c_void_p(yptr),
                                        ctypes.c_int(y_dtype), None if out_null else ptr(out), None, ctypes.byref(rc))
    return rc.value


def test_argument_validation_on_the_host():
    assert _call(width=12, x_dtype=F32, y_dtype=F16) == VOLTRIX_ERR_BAD_SHAPE      # 16-bit operand: width % 8
    assert _call(width=12, x_dtype=F16, y_dtype=F16) == VOLTRIX_ERR_BAD_SHAPE
    assert _call(width=6, x_dtype=F32, y_dtype=F32) == VOLTRIX_ERR_BAD_SHAPE       # fp32 pair: width % 4
    assert _call(x_offset=8) == VOLTRIX_ERR_BAD_SHAPE                              # x not 16-byte aligned
    assert _call(x_dtype=3, y_dtype=F16) == VOLTRIX_ERR_BAD_SHAPE                  # unknown dtype code
    assert _call(x_dtype=F16, y_dtype=F32) == VOLTRIX_ERR_BAD_SHAPE                # pair outside the set
    assert _call(x_dtype=F16, y_dtype=BF16) == VOLTRIX_ERR_BAD_SHAPE
    assert _call(out_null=True) == VOLTRIX_ERR_BAD_SHAPE                           # null out
    assert _call(num_rows=-1) == VOLTRIX_ERR_BAD_SHAPE
    assert _call(nnz=-1) == VOLTRIX_ERR_BAD_SHAPE
    assert _call(width=-8) == VOLTRIX_ERR_BAD_SHAPE
    assert _call(nnz=0) == VOLTRIX_OK                                              # nothing to do: no launch
    assert _call(nnz=0, out_null=True) == VOLTRIX_OK
    assert _call(width=0) == VOLTRIX_OK


SOURCE = r'''
#include "voltrix/sddmm_kernels.hpp"
#define I(X, Y)                                                                                         \
  template __global__ void voltrix::sddmm_csr_kernel<X, Y, 0>(const voltrix::SddmmArgs);                \
  template __global__ void voltrix::sddmm_csr_kernel<X, Y, 1>(const voltrix::SddmmArgs);                \
  template __global__ void voltrix::sddmm_csr_kernel<X, Y, 2>(const voltrix::SddmmArgs);
I(float, _Float16) I(float, voltrix::bfloat16_bits) I(_Float16, _Float16) I(voltrix::bfloat16_bits, voltrix::bfloat16_bits) I(float, float)
'''


def test_every_instantiation_compiles_without_scratch(tmp_path):
    src = tmp_path / "sddmm.hip"
    src.write_text(SOURCE)
    inc = os.path.join(REPO, "voltrix-spmm_amd", "voltrix", "include")
    run = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", inc,
                          "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", str(tmp_path / "sddmm.o")],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    usage = {}
    for block in run.stderr.split("remark: Function Name: ")[1:]:
        name = block.split(" ")[0]
        if "sddmm_csr_kernel" in name:
            usage[name] = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1))
    assert len(usage) == 15, sorted(usage)
    assert all(v == 0 for v in usage.values()), usage
