"""CPU: the GAT score entry points are declared, bound and exported; their argument checks answer on the host before any launch; the
workspace size depends on (nnz, heads) alone and is a multiple of 16; every kernel instantiation compiles for gfx950 without scratch.
No GPU compute is called here."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import REPO

from voltrix import capi

HEADER = os.path.join(REPO, "include", "voltrix_capi.h")
VOLTRIX_OK, VOLTRIX_ERR_BAD_SHAPE = 0, 1
NAMES = ("voltrix_launch_gat_score_csr", "voltrix_launch_gat_score_rowsum_csr", "voltrix_gat_score_workspace_bytes")


def test_header_declares_and_binding_lists_the_entry_points():
    import voltrix

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in capi.SYMBOLS
        assert hasattr(capi.lib(), name)
    assert capi.lib().voltrix_abi_version() == 2
    assert callable(voltrix.gat_score) and callable(voltrix.autograd.GATScore)
    from voltrix.gat_score import gat_score_backward, workspace_bytes    # (voltrix.gat_score is the function)

    assert callable(gat_score_backward) and callable(workspace_bytes)


def _ptrs(names, null, offset):
    # host buffers: every call below is refused (or has nothing to do) before a pointer is dereferenced or a kernel launched
    bufs = {k: np.zeros(4096 + 16, np.uint8) for k in names}
    base = {k: b.ctypes.data + (-b.ctypes.data) % 16 for k, b in bufs.items()}
    ptrs = {k: None if null == k else ctypes.c_void_p(base[k] + (offset[1] if offset and offset[0] == k else 0)) for k in names}
    return bufs, ptrs


def _forward(num_rows=4, nnz=6, heads=2, slope=0.2, null=None, offset=None):
    bufs, p = _ptrs(("indptr", "indices", "el", "er", "out"), null, offset)
    rc = ctypes.c_int(-1)
    capi.lib().voltrix_launch_gat_score_csr(p["indptr"], p["indices"], ctypes.c_int(num_rows), ctypes.c_int64(nnz), ctypes.c_int(heads),
                                            p["el"], p["er"], ctypes.c_float(slope), p["out"], None, ctypes.byref(rc))
    return rc.value


def _rowsum(num_rows=4, nnz=6, heads=2, slope=0.2, null=None, offset=None):
    bufs, p = _ptrs(("indptr", "indices", "order", "a", "b", "grad", "out", "ws"), null, offset)
    rc = ctypes.c_int(-1)
    capi.lib().voltrix_launch_gat_score_rowsum_csr(p["indptr"], p["indices"], p["order"], ctypes.c_int(num_rows), ctypes.c_int64(nnz),
                                                   ctypes.c_int(heads), p["a"], p["b"], p["grad"], ctypes.c_float(slope), p["out"],
                                                   p["ws"], None, ctypes.byref(rc))
    return rc.value


def _common(call):
    assert call(heads=0) == VOLTRIX_ERR_BAD_SHAPE
    assert call(heads=-3) == VOLTRIX_ERR_BAD_SHAPE
    assert call(heads=0, nnz=0) == VOLTRIX_ERR_BAD_SHAPE                  # heads is checked before "nothing to do"
    assert call(num_rows=-1) == VOLTRIX_ERR_BAD_SHAPE
    assert call(nnz=-1) == VOLTRIX_ERR_BAD_SHAPE
    assert call(nnz=2 ** 31) == VOLTRIX_ERR_BAD_SHAPE                     # nnz > INT_MAX
    assert call(num_rows=0) == VOLTRIX_ERR_BAD_SHAPE                      # entries but no row
    assert call(num_rows=2 ** 20, heads=2 ** 12) == VOLTRIX_ERR_BAD_SHAPE  # heads * num_rows > INT_MAX
    for slope in (float("inf"), float("-inf"), float("nan")):
        assert call(slope=slope) == VOLTRIX_ERR_BAD_SHAPE
        assert call(slope=slope, nnz=0, num_rows=0) == VOLTRIX_ERR_BAD_SHAPE
    assert call(nnz=0, num_rows=0) == VOLTRIX_OK                          # nothing to do: no launch


def test_forward_argument_validation_on_the_host():
    _common(_forward)
    for name in ("indptr", "indices", "el", "er", "out"):
        assert _forward(null=name) == VOLTRIX_ERR_BAD_SHAPE, name
        assert _forward(offset=(name, 2)) == VOLTRIX_ERR_BAD_SHAPE, name   # not 4-byte aligned
    assert _forward(nnz=0) == VOLTRIX_OK
    assert _forward(nnz=0, null="out") == VOLTRIX_OK


def test_rowsum_argument_validation_on_the_host():
    _common(_rowsum)
    for name in ("indptr", "indices", "a", "b", "grad", "out", "ws"):
        assert _rowsum(null=name) == VOLTRIX_ERR_BAD_SHAPE, name
    for name in ("indptr", "indices", "order", "a", "b", "grad", "out"):
        assert _rowsum(offset=(name, 2)) == VOLTRIX_ERR_BAD_SHAPE, name    # not 4-byte aligned
    assert _rowsum(offset=("ws", 8)) == VOLTRIX_ERR_BAD_SHAPE             # workspace not 16-byte aligned
    assert _rowsum(nnz=0, null="out") == VOLTRIX_ERR_BAD_SHAPE            # rows to zero-fill but nowhere to write
    assert _rowsum(nnz=0, num_rows=0, null="out") == VOLTRIX_OK


def test_workspace_bytes_depend_on_nnz_and_heads_alone():
    from voltrix.gat_score import workspace_bytes

    f = capi.lib().voltrix_gat_score_workspace_bytes
    assert f(ctypes.c_int(10), ctypes.c_int64(0), ctypes.c_int(4)) == 0
    assert f(ctypes.c_int(-1), ctypes.c_int64(100), ctypes.c_int(4)) == 0
    assert f(ctypes.c_int(10), ctypes.c_int64(100), ctypes.c_int(0)) == 0
    for num_rows, nnz in ((1, 1), (3, 2047), (3, 2048), (3, 2049), (232965, 114615892), (685230, 7600595), (1, 2 ** 31 - 1)):
        chunks = -(-nnz // 2048)
        for heads in (1, 2, 3, 8, 16):
            # rows 8 B per chunk + pad to 16, then per head two partial sums of 4 B per chunk, rounded up to 16
            want = -(-(8 * chunks + 8 * (chunks % 2) + heads * 8 * chunks) // 16) * 16
            got = workspace_bytes(num_rows, nnz, heads)
            assert got == want == f(ctypes.c_int(num_rows), ctypes.c_int64(nnz), ctypes.c_int(heads)) and got % 16 == 0
    assert workspace_bytes(1, 5000, heads=8) == workspace_bytes(4000, 5000, heads=8)
    assert workspace_bytes(7, 5000) == workspace_bytes(7, 5000, heads=1)


SOURCE = r'''
#include "voltrix/gat_score_kernels.hpp"
#define F(H) template __global__ void voltrix::gat_score_kernel<H>(const voltrix::GatScoreArgs);
F(0) F(1) F(4) F(8)
void host_use(const voltrix::GatRowsumArgs& a, float* out, hipStream_t s) {
  hipLaunchKernelGGL(voltrix::gat_score_zero_kernel, dim3(1), dim3(256), 0, s, out, 1ll);
  hipLaunchKernelGGL(voltrix::gat_score_rowsum_chunk_kernel, dim3(1), dim3(256), 0, s, a);
  hipLaunchKernelGGL(voltrix::gat_score_rowsum_merge_kernel, dim3(1), dim3(256), 0, s, a);
}
'''


def test_every_instantiation_compiles_without_scratch(tmp_path):
    src = tmp_path / "gat_score.hip"
    src.write_text(SOURCE)
    inc = os.path.join(REPO, "voltrix-spmm_amd", "voltrix", "include")
    run = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", inc,
                          "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", str(tmp_path / "gat_score.o")],
                         capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    usage = {}
    for block in run.stderr.split("remark: Function Name: ")[1:]:
        name = block.split(" ")[0].strip()
        if "gat_score" in name:
            usage[name] = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1))
    # the forward for any / 1 / 4 / 8 heads, the zero fill, the chunk sums, the merge
    assert len([n for n in usage if "gat_score_kernel" in n]) == 4, sorted(usage)
    for key in ("gat_score_zero_kernel", "gat_score_rowsum_chunk_kernel", "gat_score_rowsum_merge_kernel"):
        assert len([n for n in usage if key in n]) == 1, (key, sorted(usage))
    assert len(usage) == 7 and all(v == 0 for v in usage.values()), usage
