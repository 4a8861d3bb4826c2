"""CPU: the edge softmax's C-ABI entry points are declared, bound and exported; their argument checks are rows of
tests/core_abi_cases.py; the workspace size agrees with what voltrix/edge_softmax.py allocates; every kernel instantiation compiles for
gfx950 without scratch.  No GPU compute is called here."""
import ctypes
import os
import re

from conftest import REPO

from kernel_resources import resource_usage
from voltrix import capi

HEADER = os.path.join(REPO, "include", "voltrix_capi.h")
NAMES = ("voltrix_edge_softmax_workspace_bytes", "voltrix_launch_edge_softmax_csr", "voltrix_launch_edge_softmax_backward_csr")


def test_header_declares_and_binding_lists_the_entry_points():
    import voltrix

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in capi.SYMBOLS
        assert hasattr(capi.lib(), name)
    assert callable(voltrix.edge_softmax) and callable(voltrix.autograd.EdgeSoftmax)


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
    usage, _ = resource_usage(SOURCE, tmp_path, "edge_softmax", ("edge_softmax",))
    assert len(usage) == 6, sorted(usage)
    assert all(v[0] == 0 for v in usage.values()), usage
