"""CPU: the GATv2 score entry points are declared, bound and exported; their argument checks are rows of tests/core_abi_cases.py;
every kernel instantiation compiles for gfx950 without scratch.  No GPU compute is called here."""
import os
import re

from conftest import REPO

from kernel_resources import resource_usage
from voltrix import capi

HEADER = os.path.join(REPO, "include", "voltrix_capi.h")
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


SOURCE = r'''
#include "voltrix/gatv2_score_kernels.hpp"
#define F(T, R) template __global__ void voltrix::gatv2_score_csr_kernel<T, R>(const voltrix::Gatv2ScoreArgs);
#define G(T) template __global__ void voltrix::gatv2_rowsum_csr_kernel<T, 4>(const voltrix::Gatv2RowsumArgs<T>);
F(float, 0) F(float, 1) F(_Float16, 0) F(_Float16, 1) F(voltrix::bfloat16_bits, 0) F(voltrix::bfloat16_bits, 1)
G(float) G(_Float16) G(voltrix::bfloat16_bits)
'''


def test_every_instantiation_compiles_without_scratch(tmp_path):
    usage, _ = resource_usage(SOURCE, tmp_path, "gatv2_score", ("gatv2",))
    # the forward for three types x R in {0, 1}, the row sum for three types
    assert len([n for n in usage if "gatv2_score_csr_kernel" in n]) == 6, sorted(usage)
    assert len([n for n in usage if "gatv2_rowsum_csr_kernel" in n]) == 3, sorted(usage)
    assert len(usage) == 9 and all(v[0] == 0 for v in usage.values()), usage
