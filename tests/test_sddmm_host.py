"""CPU: the sampled dense-dense product's C-ABI entry point is declared, bound and exported; its argument checks are rows of
tests/core_abi_cases.py; every kernel instantiation compiles for gfx950 without scratch.  No GPU compute is called here."""
import os
import re

from conftest import REPO

from kernel_resources import resource_usage
from voltrix import capi

HEADER = os.path.join(REPO, "include", "voltrix_capi.h")


def test_header_declares_and_binding_lists_the_entry_point():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bvoltrix_launch_sddmm_csr\s*\(", text)
    assert "voltrix_launch_sddmm_csr" in capi.SYMBOLS
    assert hasattr(capi.lib(), "voltrix_launch_sddmm_csr")


SOURCE = r'''
#include "voltrix/sddmm_kernels.hpp"
#define I(X, Y)                                                                                         \
  template __global__ void voltrix::sddmm_csr_kernel<X, Y, 0>(const voltrix::SddmmArgs);                \
  template __global__ void voltrix::sddmm_csr_kernel<X, Y, 1>(const voltrix::SddmmArgs);                \
  template __global__ void voltrix::sddmm_csr_kernel<X, Y, 2>(const voltrix::SddmmArgs);
I(float, _Float16) I(float, voltrix::bfloat16_bits) I(_Float16, _Float16) I(voltrix::bfloat16_bits, voltrix::bfloat16_bits) I(float, float)
'''


def test_every_instantiation_compiles_without_scratch(tmp_path):
    usage, _ = resource_usage(SOURCE, tmp_path, "sddmm", ("sddmm_csr_kernel",))
    assert len(usage) == 15, sorted(usage)
    assert all(v[0] == 0 for v in usage.values()), usage
