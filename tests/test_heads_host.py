"""CPU: the multi-head attention operators' C-ABI entry points are declared, bound and exported; their argument checks answer on the
host before any launch; the workspace size with one head is the single-head size; every new kernel instantiation compiles for gfx950
without scratch.  No GPU compute is called here."""
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
NAMES = ("voltrix_launch_sddmm_heads_csr", "voltrix_edge_softmax_heads_workspace_bytes", "voltrix_launch_edge_softmax_heads_csr",
         "voltrix_launch_edge_softmax_heads_backward_csr", "voltrix_launch_spmm_csr_heads")


def test_header_declares_and_binding_lists_the_entry_points():
    import voltrix

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in capi.SYMBOLS
        assert hasattr(capi.lib(), name)
    assert capi.lib().voltrix_abi_version() == 2
    assert callable(voltrix.spmm_heads) and callable(voltrix.autograd.SpMMHeads)


def _buffers(names):
    # host buffers: every call below is refused (or has nothing to do) before a pointer is dereferenced or a kernel launched
    bufs = {k: np.zeros(4096 + 16, np.uint8) for k in names}
    return bufs, {k: b.ctypes.data + (-b.ctypes.data) % 16 for k, b in bufs.items()}


def _ptrs(names, null, offset):
    bufs, base = _buffers(names)
    ptrs = {k: None if null == k else ctypes.c_void_p(base[k] + (offset[1] if offset and offset[0] == k else 0)) for k in names}
    return bufs, ptrs


def _sddmm(num_rows=4, nnz=6, heads=2, head_dim=16, x_dtype=F32, y_dtype=F16, null=None, offset=None):
    bufs, p = _ptrs(("indptr", "indices", "x", "y", "out"), null, offset)
    rc = ctypes.c_int(-1)
    capi.lib().voltrix_launch_sddmm_heads_csr(p["indptr"], p["indices"], ctypes.c_int(num_rows), ctypes.c_int64(nnz), ctypes.c_int(heads),
                                              ctypes.c_int(head_dim), p["x"], ctypes.c_int(x_dtype), p["y"], ctypes.c_int(y_dtype),
                                              p["out"], None, ctypes.byref(rc))
    return rc.value


def test_sddmm_heads_argument_validation_on_the_host():
    assert _sddmm(heads=0) == VOLTRIX_ERR_BAD_SHAPE
    assert _sddmm(heads=-2) == VOLTRIX_ERR_BAD_SHAPE
    assert _sddmm(head_dim=12, x_dtype=F32, y_dtype=F16) == VOLTRIX_ERR_BAD_SHAPE      # 16-bit gathered operand: head_dim % 8
    assert _sddmm(head_dim=20, x_dtype=F16, y_dtype=F16) == VOLTRIX_ERR_BAD_SHAPE
    assert _sddmm(head_dim=6, x_dtype=F32, y_dtype=F32) == VOLTRIX_ERR_BAD_SHAPE       # fp32 pair: head_dim % 4
    assert _sddmm(head_dim=-8) == VOLTRIX_ERR_BAD_SHAPE
    assert _sddmm(num_rows=-1) == VOLTRIX_ERR_BAD_SHAPE
    assert _sddmm(nnz=-1) == VOLTRIX_ERR_BAD_SHAPE
    assert _sddmm(nnz=2 ** 31) == VOLTRIX_ERR_BAD_SHAPE
    assert _sddmm(num_rows=0) == VOLTRIX_ERR_BAD_SHAPE                                 # entries but no row
    assert _sddmm(heads=2 ** 20, head_dim=2 ** 12) == VOLTRIX_ERR_BAD_SHAPE            # heads * head_dim > INT_MAX
    assert _sddmm(x_dtype=3, y_dtype=F16) == VOLTRIX_ERR_BAD_SHAPE                     # unknown dtype code
    assert _sddmm(x_dtype=F16, y_dtype=F32) == VOLTRIX_ERR_BAD_SHAPE                   # pairs outside the set
    assert _sddmm(x_dtype=F16, y_dtype=BF16) == VOLTRIX_ERR_BAD_SHAPE
    assert _sddmm(x_dtype=BF16, y_dtype=F16) == VOLTRIX_ERR_BAD_SHAPE
    for name in ("indptr", "indices", "x", "y", "out"):
        assert _sddmm(null=name) == VOLTRIX_ERR_BAD_SHAPE, name
    for name in ("x", "y"):
        assert _sddmm(offset=(name, 8)) == VOLTRIX_ERR_BAD_SHAPE, name                 # not 16-byte aligned
    for name in ("indptr", "indices", "out"):
        assert _sddmm(offset=(name, 2)) == VOLTRIX_ERR_BAD_SHAPE, name                 # not 4-byte aligned
    assert _sddmm(nnz=0) == VOLTRIX_OK                                                 # nothing to do: no launch
    assert _sddmm(nnz=0, null="out") == VOLTRIX_OK
    assert _sddmm(head_dim=0) == VOLTRIX_OK


def _softmax(backward=False, num_rows=4, nnz=6, heads=2, scale=1.0, null=None, offset=None):
    bufs, p = _ptrs(("indptr", "in0", "in1", "out", "ws"), null, offset)
    rc = ctypes.c_int(-1)
    if backward:
        capi.lib().voltrix_launch_edge_softmax_heads_backward_csr(p["indptr"], ctypes.c_int(num_rows), ctypes.c_int64(nnz),
                                                                  ctypes.c_int(heads), p["in0"], p["in1"], ctypes.c_float(scale),
                                                                  p["out"], p["ws"], None, ctypes.byref(rc))
    else:
        capi.lib().voltrix_launch_edge_softmax_heads_csr(p["indptr"], ctypes.c_int(num_rows), ctypes.c_int64(nnz), ctypes.c_int(heads),
                                                         p["in0"], ctypes.c_float(scale), p["out"], p["ws"], None, ctypes.byref(rc))
    return rc.value


def test_edge_softmax_heads_argument_validation_on_the_host():
    for backward in (False, True):
        assert _softmax(backward, heads=0) == VOLTRIX_ERR_BAD_SHAPE
        assert _softmax(backward, heads=-1) == VOLTRIX_ERR_BAD_SHAPE
        assert _softmax(backward, heads=0, nnz=0) == VOLTRIX_ERR_BAD_SHAPE             # heads is checked before "nothing to do"
        assert _softmax(backward, num_rows=-1) == VOLTRIX_ERR_BAD_SHAPE
        assert _softmax(backward, nnz=-1) == VOLTRIX_ERR_BAD_SHAPE
        assert _softmax(backward, nnz=2 ** 31) == VOLTRIX_ERR_BAD_SHAPE                # nnz > INT_MAX
        assert _softmax(backward, scale=float("inf")) == VOLTRIX_ERR_BAD_SHAPE
        assert _softmax(backward, scale=float("nan")) == VOLTRIX_ERR_BAD_SHAPE
        assert _softmax(backward, num_rows=0) == VOLTRIX_ERR_BAD_SHAPE                 # entries but no row
        for name in ("indptr", "in0", "out", "ws") + (("in1",) if backward else ()):
            assert _softmax(backward, null=name) == VOLTRIX_ERR_BAD_SHAPE, name
        for name in ("indptr", "in0", "out"):
            assert _softmax(backward, offset=(name, 2)) == VOLTRIX_ERR_BAD_SHAPE, name  # not 4-byte aligned
        assert _softmax(backward, offset=("ws", 8)) == VOLTRIX_ERR_BAD_SHAPE          # workspace not 16-byte aligned
        assert _softmax(backward, nnz=0) == VOLTRIX_OK                                # nothing to do: no launch
        assert _softmax(backward, nnz=0, null="out") == VOLTRIX_OK
        assert _softmax(backward, nnz=0, num_rows=0) == VOLTRIX_OK


def _aggregate(num_rows=4, heads=2, head_dim=16, dtype=F16, null=None, offset=None):
    bufs, p = _ptrs(("indptr", "indices", "values", "input", "output"), null, offset)
    rc = ctypes.c_int(-1)
    capi.lib().voltrix_launch_spmm_csr_heads(p["indptr"], p["indices"], p["values"], ctypes.c_int(num_rows), ctypes.c_int(heads),
                                             ctypes.c_int(head_dim), p["input"], ctypes.c_int(dtype), p["output"], None,
                                             ctypes.byref(rc))
    return rc.value


def test_aggregation_heads_argument_validation_on_the_host():
    assert _aggregate(heads=0) == VOLTRIX_ERR_BAD_SHAPE
    assert _aggregate(heads=-1) == VOLTRIX_ERR_BAD_SHAPE
    assert _aggregate(head_dim=12, dtype=F16) == VOLTRIX_ERR_BAD_SHAPE                 # 16-bit rows: head_dim % 8
    assert _aggregate(head_dim=20, dtype=BF16) == VOLTRIX_ERR_BAD_SHAPE
    assert _aggregate(head_dim=6, dtype=F32) == VOLTRIX_ERR_BAD_SHAPE                  # fp32 rows: head_dim % 4
    assert _aggregate(head_dim=-8) == VOLTRIX_ERR_BAD_SHAPE
    assert _aggregate(num_rows=-1) == VOLTRIX_ERR_BAD_SHAPE
    assert _aggregate(dtype=3) == VOLTRIX_ERR_BAD_SHAPE
    assert _aggregate(dtype=-1) == VOLTRIX_ERR_BAD_SHAPE
    assert _aggregate(heads=2 ** 20, head_dim=2 ** 12) == VOLTRIX_ERR_BAD_SHAPE        # heads * head_dim > INT_MAX
    for name in ("indptr", "indices", "values", "input", "output"):
        assert _aggregate(null=name) == VOLTRIX_ERR_BAD_SHAPE, name
    for name in ("input", "output"):
        assert _aggregate(offset=(name, 8)) == VOLTRIX_ERR_BAD_SHAPE, name             # not 16-byte aligned
    for name in ("indptr", "indices", "values"):
        assert _aggregate(offset=(name, 2)) == VOLTRIX_ERR_BAD_SHAPE, name             # not 4-byte aligned
    assert _aggregate(num_rows=0) == VOLTRIX_OK                                        # nothing to do: no launch
    assert _aggregate(num_rows=0, null="output") == VOLTRIX_OK
    assert _aggregate(head_dim=0) == VOLTRIX_OK


def test_workspace_bytes_with_one_head_are_the_single_head_bytes():
    from voltrix.edge_softmax import workspace_bytes    # (voltrix.edge_softmax is the function)

    f = capi.lib().voltrix_edge_softmax_heads_workspace_bytes
    assert f(ctypes.c_int(10), ctypes.c_int64(0), ctypes.c_int(4)) == 0
    assert f(ctypes.c_int(-1), ctypes.c_int64(100), ctypes.c_int(4)) == 0
    assert f(ctypes.c_int(10), ctypes.c_int64(100), ctypes.c_int(0)) == 0
    for num_rows, nnz in ((1, 1), (3, 2047), (3, 2048), (3, 2049), (232965, 114615892), (685230, 7600595), (1, 2 ** 31 - 1)):
        assert workspace_bytes(num_rows, nnz, heads=1) == workspace_bytes(num_rows, nnz) == capi.edge_softmax_workspace_bytes(num_rows, nnz)
        assert capi.edge_softmax_heads_workspace_bytes(num_rows, nnz, 1) == workspace_bytes(num_rows, nnz)
        chunks = -(-nnz // 2048)
        for heads in (2, 3, 8, 16):
            # rows 8 B per chunk + pad to 16, then per head two partials 16 B + merged 8 B per chunk
            want = 8 * chunks + 8 * (chunks % 2) + heads * 24 * chunks
            assert workspace_bytes(num_rows, nnz, heads=heads) == want == f(ctypes.c_int(num_rows), ctypes.c_int64(nnz), ctypes.c_int(heads))
    # a function of (nnz, heads) alone: a graph can be captured once per (nnz, heads)
    assert workspace_bytes(1, 5000, heads=8) == workspace_bytes(4000, 5000, heads=8)


SOURCE = r'''
#include "voltrix/edge_softmax_heads_kernels.hpp"
#include "voltrix/sddmm_heads_kernels.hpp"
#include "voltrix/spmm_csr_heads_kernels.hpp"
#define S(X, Y)                                                                                             \
  template __global__ void voltrix::sddmm_heads_csr_kernel<X, Y, 0>(const voltrix::SddmmHeadsArgs);         \
  template __global__ void voltrix::sddmm_heads_csr_kernel<X, Y, 1>(const voltrix::SddmmHeadsArgs);
S(float, _Float16) S(float, voltrix::bfloat16_bits) S(_Float16, _Float16) S(voltrix::bfloat16_bits, voltrix::bfloat16_bits) S(float, float)
#define E(OP)                                                                                                            \
  template __global__ void voltrix::edge_softmax_heads_chunk_kernel<voltrix::OP>(const voltrix::EdgeSoftmaxHeadsArgs);    \
  template __global__ void voltrix::edge_softmax_heads_merge_kernel<voltrix::OP>(const voltrix::EdgeSoftmaxHeadsArgs);    \
  template __global__ void voltrix::edge_softmax_heads_boundary_kernel<voltrix::OP>(const voltrix::EdgeSoftmaxHeadsArgs);
E(SoftmaxHeadsOp) E(SoftmaxBackwardHeadsOp)
#define A(T) template __global__ void voltrix::spmm_csr_heads_kernel<T, 4>(const voltrix::CsrHeadsArgs<T>);
A(float) A(_Float16) A(voltrix::bfloat16_bits)
'''


def test_every_instantiation_compiles_without_scratch(tmp_path):
    src = tmp_path / "heads.hip"
    src.write_text(SOURCE)
    inc = os.path.join(REPO, "voltrix-spmm_amd", "voltrix", "include")
    run = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", inc,
                          "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", str(tmp_path / "heads.o")],
                         capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    usage = {"sddmm_heads_csr_kernel": {}, "edge_softmax_heads_": {}, "spmm_csr_heads_kernel": {}}
    for block in run.stderr.split("remark: Function Name: ")[1:]:
        name = block.split(" ")[0]
        for key in usage:
            if key in name:
                usage[key][name] = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1))
    # 5 operand pairs x (one piece per lane, any number) ; (chunk, merge, boundary) x (forward, backward) ; 3 feature types
    assert len(usage["sddmm_heads_csr_kernel"]) == 10, sorted(usage["sddmm_heads_csr_kernel"])
    assert len(usage["edge_softmax_heads_"]) == 6, sorted(usage["edge_softmax_heads_"])
    assert len(usage["spmm_csr_heads_kernel"]) == 3, sorted(usage["spmm_csr_heads_kernel"])
    for group in usage.values():
        assert all(v == 0 for v in group.values()), group
