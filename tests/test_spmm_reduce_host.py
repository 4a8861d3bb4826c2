"""CPU: the max / min / mean aggregation entry points are declared, bound and exported; their argument checks are rows of
tests/core_abi_cases.py; every kernel instantiation compiles for gfx950 without scratch and without spilled registers.  No GPU compute
is called here."""
import os
import re

import pytest

from conftest import REPO

from kernel_resources import resource_usage
from voltrix import capi

HEADER = os.path.join(REPO, "include", "voltrix_capi.h")
NAMES = ("voltrix_launch_spmm_csr_reduce", "voltrix_launch_spmm_csr_reduce_backward")
MAX, MIN, MEAN = 0, 1, 2


def test_header_declares_and_binding_lists_the_entry_points():
    import voltrix

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in capi.SYMBOLS
        assert hasattr(capi.lib(), name)
    assert capi.lib().voltrix_abi_version() == 2
    assert callable(voltrix.spmm_reduce) and callable(voltrix.autograd.SpMMReduce)
    from voltrix.spmm_reduce import spmm_reduce_backward      # (voltrix.spmm_reduce is the function)

    assert callable(spmm_reduce_backward) and voltrix.spmm_reduce.spmm_reduce_backward is spmm_reduce_backward
    assert capi.REDUCE_OPS == {"max": MAX, "min": MIN, "mean": MEAN}


def test_a_bad_reduce_is_a_value_error():
    import voltrix

    for reduce in ("sum", "amax", "", None):
        with pytest.raises(ValueError):                      # raised before any tensor is looked at
            voltrix.spmm_reduce(None, None, None, 0, reduce=reduce)
        with pytest.raises(ValueError):
            voltrix.autograd.SpMMReduce(None, reduce=reduce)
    with pytest.raises(ValueError):
        voltrix.spmm_reduce(None, None, None, 0, reduce="mean", return_arg=True)


SOURCE = r'''
#include "voltrix/spmm_csr_reduce_kernels.hpp"
#define K(T, OP, ARG) template __global__ void voltrix::spmm_csr_reduce_kernel<T, OP, ARG, 4>(const voltrix::CsrReduceArgs<T>);
#define ALL(T) K(T, 0, true) K(T, 0, false) K(T, 1, true) K(T, 1, false) K(T, 2, false)
ALL(float) ALL(_Float16) ALL(uint16_t)
template __global__ void voltrix::spmm_csr_reduce_backward_kernel<4>(const voltrix::CsrReduceBackwardArgs);
'''


def test_every_instantiation_compiles_without_scratch_or_spills(tmp_path):
    usage, _ = resource_usage(SOURCE, tmp_path, "spmm_reduce", ("spmm_csr_reduce",))
    # {fp32, fp16, bf16} x ({max, min} x {with, without arg} + mean), and the backward
    forward = [n for n in usage if "spmm_csr_reduce_kernel" in n]
    assert len(forward) == 15 and len([n for n in usage if "spmm_csr_reduce_backward_kernel" in n]) == 1, sorted(usage)
    assert len(usage) == 16 and all(v[:3] == (0, 0, 0) for v in usage.values()), usage
