"""CPU: the edge softmax's C-ABI entry points are declared, bound and exported; their argument checks answer on the host before any
launch; the workspace size agrees with what voltrix/edge_softmax.py allocates; every kernel instantiation compiles for gfx950 without
scratch.  No GPU compute is called here."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import REPO

from voltrix import capi

HEADER = os.path.join(REPO, "include", "voltrix_capi.h")
VOLTRIX_OK, VOLTRIX_ERR_BAD_SHAPE = 0, 1
NAMES = ("voltrix_edge_softmax_workspace_bytes", "voltrix_launch_edge_softmax_csr", "voltrix_launch_edge_softmax_backward_csr")


def test_header_declares_and_binding_lists_the_entry_points():
    import voltrix

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in capi.SYMBOLS
        assert hasattr(capi.lib(), name)
    assert callable(voltrix.edge_softmax) and callable(voltrix.autograd.EdgeSoftmax)


def _call(backward=False, num_rows=4, nnz=6, scale=1.0, null=None, offset=None):
    # host buffers: every call below is refused (or has nothing to do) before a pointer is dereferenced or a kernel launched
    bufs = {k: np.zeros(64, np.float32) for k in ("indptr", "in0", "in1", "out", "ws")}
    ptrs = {}
    for k, b in bufs.items():
        base = b.ctypes.data + (-b.ctypes.data) % 16
        ptrs[k] = None if null == k else ctypes.c_void_p(base + (offset[1] if offset and offset[0] == k else 0))
    rc = ctypes.c_int(-1)
    if backward:
        capi.lib().voltrix_launch_edge_softmax_backward_csr(ptrs["indptr"], ctypes.c_int(num_rows), ctypes.c_int64(nnz), ptrs["in0"],
                                                            ptrs["in1"], ctypes.c_float(scale), ptrs["out"], ptrs["ws"], None,
                                                            ctypes.byref(rc))
    else:
        capi.lib().voltrix_launch_edge_softmax_csr(ptrs["indptr"], ctypes.c_int(num_rows), ctypes.c_int64(nnz), ptrs["in0"],
                                                   ctypes.c_float(scale), ptrs["out"], ptrs["ws"], None, ctypes.byref(rc))
    return rc.value


def test_argument_validation_on_the_host():
    for backward in (False, True):
        assert _call(backward, num_rows=-1) == VOLTRIX_ERR_BAD_SHAPE
        assert _call(backward, nnz=-1) == VOLTRIX_ERR_BAD_SHAPE
        assert _call(backward, nnz=2 ** 31) == VOLTRIX_ERR_BAD_SHAPE                   # nnz > INT_MAX
        assert _call(backward, scale=float("inf")) == VOLTRIX_ERR_BAD_SHAPE
        assert _call(backward, scale=float("nan")) == VOLTRIX_ERR_BAD_SHAPE
        assert _call(backward, num_rows=0) == VOLTRIX_ERR_BAD_SHAPE                    # entries but no row
        names = ("indptr", "in0", "out", "ws") + (("in1",) if backward else ())
        for name in names:
            assert _call(backward, null=name) == VOLTRIX_ERR_BAD_SHAPE, name
        for name in ("indptr", "in0", "out"):
            assert _call(backward, offset=(name, 2)) == VOLTRIX_ERR_BAD_SHAPE, name    # not 4-byte aligned
        assert _call(backward, offset=("ws", 8)) == VOLTRIX_ERR_BAD_SHAPE             # workspace not 16-byte aligned
        assert _call(backward, nnz=0) == VOLTRIX_OK                                  # nothing to do: no launch
        assert _call(backward, nnz=0, null="out") == VOLTRIX_OK
        assert _call(backward, nnz=0, num_rows=0) == VOLTRIX_OK


def test_workspace_bytes_agree_with_the_python_layer():
    from voltrix.edge_softmax import workspace_bytes    # (voltrix.edge_softmax is the function)

    f = capi.lib().voltrix_edge_softmax_workspace_bytes
    assert f(ctypes.c_int(10), ctypes.c_int64(0)) == 0
    assert f(ctypes.c_int(-1), ctypes.c_int64(100)) == 0
    for num_rows, nnz in ((1, 1), (3, 2047), (3, 2048), (3, 2049), (232965, 114615892), (685230, 7600595), (1, 2 ** 31 - 1)):
        chunks = -(-nnz // 2048)
        want = 32 * chunks + 8 * (chunks % 2)                     # rows 8 B + pad to 16 + two partials 16 B + merged 8 B per chunk
        assert f(ctypes.c_int(num_rows), ctypes.c_int64(nnz)) == want
        assert workspace_bytes(num_rows, nnz) == want == capi.edge_softmax_workspace_bytes(num_rows, nnz)
    # the size does not depend on the number of rows: a graph can be captured once per nnz
    assert workspace_bytes(1, 5000) == workspace_bytes(4000, 5000)


SOURCE = r'''
#include "voltrix/edge_softmax_kernels.hpp"
#define I(OP)                                                                                         \
  template __global__ void voltrix::edge_softmax_chunk_kernel<voltrix::OP>(const voltrix::EdgeSoftmaxArgs);    \
  template __global__ void voltrix::edge_softmax_merge_kernel<voltrix::OP>(const voltrix::EdgeSoftmaxArgs);    \
  template __global__ void voltrix::edge_softmax_boundary_kernel<voltrix::OP>(const voltrix::EdgeSoftmaxArgs);
I(SoftmaxOp) I(SoftmaxBackwardOp)
'''


def test_every_instantiation_compiles_without_scratch(tmp_path):
    src = tmp_path / "edge_softmax.hip"
    src.write_text(SOURCE)
    inc = os.path.join(REPO, "voltrix-spmm_amd", "voltrix", "include")
    run = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", inc,
                          "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", str(tmp_path / "edge_softmax.o")],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    usage = {}
    for block in run.stderr.split("remark: Function Name: ")[1:]:
        name = block.split(" ")[0]
        if "edge_softmax" in name:
            usage[name] = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1))
    assert len(usage) == 6, sorted(usage)
    assert all(v == 0 for v in usage.values()), usage
