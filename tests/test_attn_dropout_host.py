"""CPU: attention dropout's packed keep mask and the masked entry points of attn_aggregate.  A numpy restatement of
Philox4x32-10 proves itself on the known-answer vectors and on the kept fraction; the four new C-ABI entry points are declared, bound
and exported; their argument checks are rows of tests/core_abi_cases.py; every new instantiation compiles for gfx950 without scratch
or LDS.  No GPU compute is called here (tests/test_gpu_attn_dropout.py compares the generator kernel with ``keep_bits`` / ``pack``)."""
import os
import re

import numpy as np
import pytest

from conftest import REPO

from kernel_resources import resource_usage
from voltrix import capi

HEADER = os.path.join(REPO, "include", "voltrix_capi.h")
NAMES = ("voltrix_launch_dropout_mask", "voltrix_launch_attn_aggregate_dropout_csr",
         "voltrix_launch_attn_aggregate_dropout_grad_scores_csr", "voltrix_launch_attn_aggregate_dropout_grad_feat_csr")

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
LOW = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on broadcastable integer arrays: the four output words as uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & LOW for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0 = np.uint64(M0) * c0                                    # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & LOW, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & LOW
        k0 = (k0 + np.uint64(W0)) & LOW
        k1 = (k1 + np.uint64(W1)) & LOW
    return [v.astype(np.uint32) for v in np.broadcast_arrays(c0, c1, c2, c3)]


def threshold_of(p):
    return min(2 ** 32 - 1, int(float(p) * 4294967296.0))


def keep_bits(nnz, heads, threshold, seed, offset, first_edge=0):
    """bool [nnz, heads]: (e, h) is kept iff word h & 3 of Philox((e, h >> 2, offset lo, offset hi), (seed lo, seed hi)) >= threshold."""
    e = np.arange(first_edge, first_edge + nnz, dtype=np.uint64)[:, None]
    h = np.arange(heads, dtype=np.uint64)[None, :]
    words = np.stack(philox4x32_10(e, h >> np.uint64(2), offset & 0xFFFFFFFF, offset >> 32, seed & 0xFFFFFFFF, seed >> 32), -1)
    pick = np.broadcast_to((h & np.uint64(3)).astype(np.int64)[..., None], (nnz, heads, 1))
    return np.take_along_axis(words, pick, -1)[..., 0] >= np.uint32(threshold)


def pack(keep):
    """bool [nnz, heads] -> the mask's words as uint32 [nnz, ceil(heads / 32)]; bits past heads are zero."""
    nnz, heads = keep.shape
    out = np.zeros((nnz, (heads + 31) // 32), np.uint32)
    for h in range(heads):
        out[:, h >> 5] |= keep[:, h].astype(np.uint32) << np.uint32(h & 31)
    return out


def test_philox_known_answers():
    cases = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"))
    for counter, key, want in cases:
        assert " ".join("%08x" % int(v) for v in philox4x32_10(*counter, *key)) == want
    # vectorised = elementwise
    got = philox4x32_10(np.array([0, 0x243F6A88]), np.array([0, 0x85A308D3]), np.array([0, 0x13198A2E]), np.array([0, 0x03707344]),
                        np.array([0, 0xA4093822]), np.array([0, 0x299F31D0]))
    assert ["%08x" % int(v[0]) for v in got] == cases[0][2].split() and ["%08x" % int(v[1]) for v in got] == cases[2][2].split()


@pytest.mark.parametrize("p", [0.1, 0.6, 0.9])
def test_kept_fraction_is_one_minus_p(p):
    keep = keep_bits(2 ** 16, 8, threshold_of(p), 1234, 0)
    count = keep.size
    sigma = (p * (1 - p) / count) ** 0.5
    assert abs(keep.mean() - (1 - p)) <= 5 * sigma, (p, keep.mean(), sigma)


def test_threshold_and_packing():
    from voltrix.dropout import drop_threshold, mask_words

    assert drop_threshold(0.0) == 0 and drop_threshold(0.5) == 2 ** 31 and drop_threshold(1 - 2.0 ** -40) == 2 ** 32 - 1
    assert all(drop_threshold(p) == threshold_of(p) for p in (0.1, 0.6, 0.9, 0.999))
    assert [mask_words(h) for h in (1, 32, 33, 64, 65)] == [1, 1, 2, 2, 3]
    assert keep_bits(50, 5, 0, 7, 9).all()                                               # threshold 0 keeps everything
    words = pack(keep_bits(50, 33, threshold_of(0.6), 7, 9))
    assert words.shape == (50, 2) and not (words[:, 1] & ~np.uint32(1)).any()            # bits past H are zero
    # a bit depends on (seed, offset, e, h) only: not on nnz, not on H
    assert np.array_equal(keep_bits(50, 33, 99, 7, 9)[:20, :5], keep_bits(20, 5, 99, 7, 9))
    assert np.array_equal(keep_bits(50, 5, 99, 7, 9)[30:], keep_bits(20, 5, 99, 7, 9, first_edge=30))


def test_header_declares_and_binding_lists_the_entry_points():
    import voltrix

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert name in capi.SYMBOLS, name
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(capi.lib(), name)
        assert name in capi.SIGNATURES, name
    assert capi.lib().voltrix_abi_version() == 2
    assert callable(voltrix.dropout_mask) and callable(voltrix.apply_dropout_mask)


def test_python_layer_rejects_bad_arguments_before_any_launch():
    import torch

    from voltrix.dropout import check_keep_scale, check_mask, dropout_mask

    for p in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            dropout_mask(10, 4, p, 1)
    for seed, offset in ((-1, 0), (2 ** 64, 0), (0, -1), (0, 2 ** 64)):
        with pytest.raises(ValueError):
            dropout_mask(10, 4, 0.5, seed, offset)
    for nnz, heads in ((-1, 4), (2 ** 31, 4), (10, 0)):
        with pytest.raises(ValueError):
            dropout_mask(nnz, heads, 0.5, 1)
    cpu = torch.device("cpu")
    assert check_mask(torch.zeros(10, 2, dtype=torch.int32), 10, 33, cpu).shape == (10, 2)
    strided = torch.zeros(10, 4, dtype=torch.int32)[:, ::2]
    assert check_mask(strided, 10, 33, cpu).is_contiguous()                              # layout-repaired like any operand
    for bad in (torch.zeros(10, 2, dtype=torch.int64), torch.zeros(10, 2), torch.zeros(10, 1, dtype=torch.int32),
                torch.zeros(9, 2, dtype=torch.int32), torch.zeros(20, dtype=torch.int32), None):
        with pytest.raises(ValueError):
            check_mask(bad, 10, 33, cpu)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            check_keep_scale(bad)


def test_apply_dropout_mask_on_the_cpu():
    import torch

    from voltrix.dropout import apply_dropout_mask, unpack_mask

    keep = keep_bits(40, 33, threshold_of(0.6), 3, 4)
    mask = torch.from_numpy(pack(keep).view(np.int32))
    assert torch.equal(unpack_mask(mask, 33), torch.from_numpy(keep))
    alpha = torch.rand(40, 33)
    alpha[0, 0] = float("nan") if not keep[0, 0] else alpha[0, 0]                        # a selection: a dropped NaN does not pass
    got = apply_dropout_mask(alpha, mask, 2.5)
    assert torch.equal(got, torch.where(torch.from_numpy(keep), alpha * 2.5, torch.zeros(())))
    one = apply_dropout_mask(alpha[:, 0].contiguous(), torch.from_numpy(pack(keep[:, :1]).view(np.int32)), 2.5)
    assert one.shape == (40,) and torch.equal(one, got[:, 0])
    with pytest.raises(ValueError):
        apply_dropout_mask(alpha, mask[:, :1], 2.5)


SOURCE = r'''
#include "voltrix/attn_aggregate_kernels.hpp"
#include "voltrix/dropout_mask_kernels.hpp"
#define F(T) template __global__ void voltrix::attn_aggregate_csr_kernel<T, 4, true>(const voltrix::AttnAggregateArgs<T>);
F(float) F(_Float16) F(voltrix::bfloat16_bits)
#define S(Y)                                                                                                                       \
  template __global__ void voltrix::attn_aggregate_grad_scores_kernel<Y, 0, true>(const voltrix::AttnAggregateGradScoresArgs);      \
  template __global__ void voltrix::attn_aggregate_grad_scores_kernel<Y, 1, true>(const voltrix::AttnAggregateGradScoresArgs);
S(float) S(_Float16) S(voltrix::bfloat16_bits)
#define G(T) template __global__ void voltrix::attn_aggregate_grad_feat_kernel<T, 4, true>(const voltrix::AttnAggregateGradFeatArgs<T>);
G(float) G(_Float16) G(voltrix::bfloat16_bits)
void* the_generator() { return reinterpret_cast<void*>(&voltrix::dropout_mask_kernel); }
'''


def test_every_new_instantiation_compiles_without_scratch_or_lds(tmp_path):
    # the masked instantiations carry the template argument `true` (Lb1 in the mangled name); the generator is not a template
    keys = ("attn_aggregate_csr_kernel", "attn_aggregate_grad_scores_kernel", "attn_aggregate_grad_feat_kernel", "dropout_mask_kernel")
    usage, _ = resource_usage(SOURCE, tmp_path, "attn_dropout", keys)
    usage = {n: v for n, v in usage.items() if "dropout_mask_kernel" in n or "Lb1" in n}
    assert [len([n for n in usage if key in n]) for key in keys] == [3, 6, 3, 1], sorted(usage)
    assert all((v[0], v[3]) == (0, 0) for v in usage.values()), usage
