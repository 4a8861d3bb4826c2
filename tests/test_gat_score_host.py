"""CPU: the GAT score entry points are declared, bound and exported; their argument checks are rows of tests/core_abi_cases.py; the
workspace size depends on (nnz, heads) alone and is a multiple of 16; every kernel instantiation compiles for gfx950 without scratch.
No GPU compute is called here."""
import ctypes
import os
import re

from conftest import REPO

from kernel_resources import resource_usage
from voltrix import capi

HEADER = os.path.join(REPO, "include", "voltrix_capi.h")
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
    usage, _ = resource_usage(SOURCE, tmp_path, "gat_score", ("gat_score",))
    # the forward for any / 1 / 4 / 8 heads, the zero fill, the chunk sums, the merge
    assert len([n for n in usage if "gat_score_kernel" in n]) == 4, sorted(usage)
    for key in ("gat_score_zero_kernel", "gat_score_rowsum_chunk_kernel", "gat_score_rowsum_merge_kernel"):
        assert len([n for n in usage if key in n]) == 1, (key, sorted(usage))
    assert len(usage) == 7 and all(v[0] == 0 for v in usage.values()), usage
