"""CPU: the fused softmax-and-aggregate operator's three C-ABI entry points are declared, bound and exported; their argument checks
are rows of tests/core_abi_cases.py; every kernel instantiation compiles for gfx950 without scratch.  No GPU compute is called here."""
import os
import re

from conftest import REPO

from kernel_resources import resource_usage
from voltrix import capi

HEADER = os.path.join(REPO, "include", "voltrix_capi.h")
NAMES = ("voltrix_launch_attn_aggregate_csr", "voltrix_launch_attn_aggregate_grad_scores_csr",
         "voltrix_launch_attn_aggregate_grad_feat_csr")


def test_header_declares_and_binding_lists_the_entry_points():
    import voltrix

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert name in capi.SYMBOLS, name
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(capi.lib(), name)
    assert capi.lib().voltrix_abi_version() == 2
    assert callable(voltrix.attn_aggregate) and callable(voltrix.autograd.AttnAggregate)
    assert callable(voltrix.attn_aggregate.attn_aggregate_grad_scores) and callable(voltrix.attn_aggregate.attn_aggregate_grad_feat)
    from voltrix.attn_aggregate import attn_aggregate, attn_aggregate_grad_feat, attn_aggregate_grad_scores     # the module too

    assert attn_aggregate is voltrix.attn_aggregate and callable(attn_aggregate_grad_feat) and callable(attn_aggregate_grad_scores)


SOURCE = r'''
#include "voltrix/attn_aggregate_kernels.hpp"
#define F(T) template __global__ void voltrix::attn_aggregate_csr_kernel<T, 4>(const voltrix::AttnAggregateArgs<T>);
F(float) F(_Float16) F(voltrix::bfloat16_bits)
#define S(Y)                                                                                                                 \
  template __global__ void voltrix::attn_aggregate_grad_scores_kernel<Y, 0>(const voltrix::AttnAggregateGradScoresArgs);      \
  template __global__ void voltrix::attn_aggregate_grad_scores_kernel<Y, 1>(const voltrix::AttnAggregateGradScoresArgs);
S(float) S(_Float16) S(voltrix::bfloat16_bits)
#define G(T) template __global__ void voltrix::attn_aggregate_grad_feat_kernel<T, 4>(const voltrix::AttnAggregateGradFeatArgs<T>);
G(float) G(_Float16) G(voltrix::bfloat16_bits)
'''


def test_every_instantiation_compiles_without_scratch(tmp_path):
    keys = ("attn_aggregate_csr_kernel", "attn_aggregate_grad_scores_kernel", "attn_aggregate_grad_feat_kernel")
    usage, _ = resource_usage(SOURCE, tmp_path, "attn_aggregate", keys)
    count = {key: len([n for n in usage if key in n]) for key in keys}
    # 3 feature types ; 3 feature types x (one piece per lane, any number) ; 3 gradient types
    assert count == {"attn_aggregate_csr_kernel": 3, "attn_aggregate_grad_scores_kernel": 6,
                     "attn_aggregate_grad_feat_kernel": 3}, sorted(usage)
    assert all(v[0] == 0 for v in usage.values()), usage
    assert all(v[3] == 0 for v in usage.values()), usage                               # no LDS either
