"""CPU: the GATv2 score entry points are declared, bound and exported; their argument checks answer on the host before any launch;
every kernel instantiation compiles for gfx950 without scratch.  No GPU compute is called here."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import REPO

from voltrix import capi

HEADER = os.path.join(REPO, "include", "voltrix_capi.h")
VOLTRIX_OK, VOLTRIX_ERR_BAD_SHAPE = 0, 1
NAMES = ("voltrix_launch_gatv2_score_csr", "voltrix_launch_gatv2_rowsum_csr")


def test_header_declares_and_binding_lists_the_entry_points():
    import voltrix

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in capi.SYMBOLS
        assert hasattr(capi.lib(), name)
    assert capi.lib().voltrix_abi_version() == 2
    assert callable(voltrix.gatv2_score) and callable(voltrix.autograd.GATv2Score)
    from voltrix.gatv2_score import gatv2_rowsum    # (voltrix.gatv2_score is the function)

    assert callable(gatv2_rowsum) and callable(capi.launch_gatv2_score_csr) and callable(capi.launch_gatv2_rowsum_csr)


def _ptrs(names, null, offset):
    # host buffers: every call below is refused (or has nothing to do) before a pointer is dereferenced or a kernel launched
    bufs = {k: np.zeros(4096 + 32, np.uint8) for k in names}
    base = {k: b.ctypes.data + (-b.ctypes.data) % 16 for k, b in bufs.items()}
    ptrs = {k: None if null == k else ctypes.c_void_p(base[k] + (offset[1] if offset and offset[0] == k else 0)) for k in names}
    return bufs, ptrs


def _forward(num_rows=4, nnz=6, heads=2, head_dim=8, dtype=1, slope=0.2, null=None, offset=None):
    bufs, p = _ptrs(("indptr", "indices", "xl", "xr", "a", "out"), null, offset)
    rc = ctypes.c_int(-1)
    capi.lib().voltrix_launch_gatv2_score_csr(p["indptr"], p["indices"], ctypes.c_int(num_rows), ctypes.c_int64(nnz), ctypes.c_int(heads),
                                              ctypes.c_int(head_dim), p["xl"], p["xr"], ctypes.c_int(dtype), p["a"],
                                              ctypes.c_float(slope), p["out"], None, ctypes.byref(rc))
    return rc.value


def _rowsum(num_rows=4, nnz=6, heads=2, head_dim=8, dtype=1, slope=0.2, null=None, offset=None):
    bufs, p = _ptrs(("indptr", "indices", "order", "p", "q", "grad", "out"), null, offset)
    rc = ctypes.c_int(-1)
    capi.lib().voltrix_launch_gatv2_rowsum_csr(p["indptr"], p["indices"], p["order"], ctypes.c_int(num_rows), ctypes.c_int64(nnz),
                                               ctypes.c_int(heads), ctypes.c_int(head_dim), p["p"], p["q"], ctypes.c_int(dtype),
                                               p["grad"], ctypes.c_float(slope), p["out"], None, ctypes.byref(rc))
    return rc.value


def _common(call):
    assert call(heads=0) == VOLTRIX_ERR_BAD_SHAPE
    assert call(heads=-3) == VOLTRIX_ERR_BAD_SHAPE
    assert call(heads=0, nnz=0, num_rows=0) == VOLTRIX_ERR_BAD_SHAPE      # heads is checked before "nothing to do"
    assert call(num_rows=-1) == VOLTRIX_ERR_BAD_SHAPE
    assert call(nnz=-1) == VOLTRIX_ERR_BAD_SHAPE
    assert call(head_dim=-8) == VOLTRIX_ERR_BAD_SHAPE
    assert call(nnz=2 ** 31) == VOLTRIX_ERR_BAD_SHAPE                     # nnz > INT_MAX
    assert call(num_rows=0) == VOLTRIX_ERR_BAD_SHAPE                      # entries but no row
    assert call(heads=2 ** 16, head_dim=2 ** 15) == VOLTRIX_ERR_BAD_SHAPE  # heads * head_dim > INT_MAX
    for dtype, head_dim in ((1, 4), (1, 12), (2, 20), (0, 2), (0, 6)):    # a head is a whole number of 16-byte pieces
        assert call(dtype=dtype, head_dim=head_dim) == VOLTRIX_ERR_BAD_SHAPE, (dtype, head_dim)
        assert call(dtype=dtype, head_dim=head_dim, nnz=0, num_rows=0) == VOLTRIX_ERR_BAD_SHAPE
    for dtype in (-1, 3, 7):
        assert call(dtype=dtype) == VOLTRIX_ERR_BAD_SHAPE
        assert call(dtype=dtype, nnz=0, num_rows=0) == VOLTRIX_ERR_BAD_SHAPE
    for slope in (float("inf"), float("-inf"), float("nan")):
        assert call(slope=slope) == VOLTRIX_ERR_BAD_SHAPE
        assert call(slope=slope, nnz=0, num_rows=0) == VOLTRIX_ERR_BAD_SHAPE
    assert call(nnz=0, num_rows=0) == VOLTRIX_OK                          # nothing to do: no launch
    assert call(nnz=0, num_rows=0, head_dim=0) == VOLTRIX_OK


def test_forward_argument_validation_on_the_host():
    _common(_forward)
    for name in ("indptr", "indices", "xl", "xr", "a", "out"):
        assert _forward(null=name) == VOLTRIX_ERR_BAD_SHAPE, name
        assert _forward(offset=(name, 2)) == VOLTRIX_ERR_BAD_SHAPE, name   # not 4-byte aligned
    for name in ("xl", "xr", "a"):
        for off in (4, 8):
            assert _forward(offset=(name, off)) == VOLTRIX_ERR_BAD_SHAPE, name    # not 16-byte aligned
    for dtype in (0, 1, 2):
        assert _forward(nnz=0, dtype=dtype) == VOLTRIX_OK                  # no entries: no launch, whatever the pointers
        assert _forward(nnz=0, dtype=dtype, null="out") == VOLTRIX_OK
        assert _forward(head_dim=0, dtype=dtype, null="a") == VOLTRIX_OK   # no columns: no launch


def test_rowsum_argument_validation_on_the_host():
    _common(_rowsum)
    for name in ("indptr", "indices", "p", "q", "grad", "out"):            # `order` may be null
        assert _rowsum(null=name) == VOLTRIX_ERR_BAD_SHAPE, name
    for name in ("indptr", "indices", "order", "p", "q", "grad", "out"):
        assert _rowsum(offset=(name, 2)) == VOLTRIX_ERR_BAD_SHAPE, name    # not 4-byte aligned
    for name in ("p", "q", "out"):
        for off in (4, 8):
            assert _rowsum(offset=(name, off)) == VOLTRIX_ERR_BAD_SHAPE, name     # not 16-byte aligned
    assert _rowsum(nnz=0, null="out") == VOLTRIX_ERR_BAD_SHAPE            # rows to zero-fill but nowhere to write
    assert _rowsum(nnz=0, num_rows=0, null="out") == VOLTRIX_OK
    assert _rowsum(head_dim=0, null="out") == VOLTRIX_OK                  # no columns: no launch


SOURCE = r'''
#include "voltrix/gatv2_score_kernels.hpp"
#define F(T, R) template __global__ void voltrix::gatv2_score_csr_kernel<T, R>(const voltrix::Gatv2ScoreArgs);
#define G(T) template __global__ void voltrix::gatv2_rowsum_csr_kernel<T, 4>(const voltrix::Gatv2RowsumArgs<T>);
F(float, 0) F(float, 1) F(_Float16, 0) F(_Float16, 1) F(voltrix::bfloat16_bits, 0) F(voltrix::bfloat16_bits, 1)
G(float) G(_Float16) G(voltrix::bfloat16_bits)
'''


def test_every_instantiation_compiles_without_scratch(tmp_path):
    src = tmp_path / "gatv2_score.hip"
    src.write_text(SOURCE)
    inc = os.path.join(REPO, "voltrix-spmm_amd", "voltrix", "include")
    run = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", inc,
                          "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", str(tmp_path / "gatv2_score.o")],
                         capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    usage = {}
    for block in run.stderr.split("remark: Function Name: ")[1:]:
        name = block.split(" ")[0].strip()
        if "gatv2" in name:
            usage[name] = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1))
    # the forward for three types x R in {0, 1}, the row sum for three types
    assert len([n for n in usage if "gatv2_score_csr_kernel" in n]) == 6, sorted(usage)
    assert len([n for n in usage if "gatv2_rowsum_csr_kernel" in n]) == 3, sorted(usage)
    assert len(usage) == 9 and all(v == 0 for v in usage.values()), usage
