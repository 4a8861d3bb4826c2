"""CPU: the multi-head attention operators' C-ABI entry points are declared, bound and exported; their argument checks are rows of
tests/core_abi_cases.py; the workspace size with one head is the single-head size; every new kernel instantiation compiles for gfx950
without scratch.  No GPU compute is called here."""
import ctypes
import os
import re

from conftest import REPO

from kernel_resources import resource_usage
from voltrix import capi

HEADER = os.path.join(REPO, "include", "voltrix_capi.h")
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
    keys = ("sddmm_heads_csr_kernel", "edge_softmax_heads_", "spmm_csr_heads_kernel")
    usage, _ = resource_usage(SOURCE, tmp_path, "heads", keys)
    count = {key: len([n for n in usage if key in n]) for key in keys}
    # 5 operand pairs x (one piece per lane, any number) ; (chunk, merge, boundary) x (forward, backward) ; 3 feature types
    assert count == {"sddmm_heads_csr_kernel": 10, "edge_softmax_heads_": 6, "spmm_csr_heads_kernel": 3}, sorted(usage)
    assert all(v[0] == 0 for v in usage.values()), usage
