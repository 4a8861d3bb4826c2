"""CPU: attention dropout's packed keep mask and the masked entry points of attn_aggregate.  A numpy restatement of
Philox4x32-10 proves itself on the known-answer vectors and on the kept fraction; the four new C-ABI entry points are declared, bound
and exported; their argument checks answer on the host before any launch; every new instantiation compiles for gfx950 without scratch
or LDS.  No GPU compute is called here (tests/test_gpu_attn_dropout.py compares the generator kernel with ``keep_bits`` / ``pack``)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO

import test_attn_aggregate_host as base
from voltrix import capi

HEADER = os.path.join(REPO, "include", "voltrix_capi.h")
OK, BAD = base.VOLTRIX_OK, base.VOLTRIX_ERR_BAD_SHAPE
F32, F16, BF16 = base.F32, base.F16, base.BF16
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


def _mask_call(nnz=6, heads=2, threshold=5, seed=2 ** 63 + 1, offset=2 ** 40, null=False, offset_bytes=0):
    buf = np.zeros(4096 + 16, np.uint8)
    ptr = None if null else ctypes.c_void_p(buf.ctypes.data + (-buf.ctypes.data) % 16 + offset_bytes)
    rc = ctypes.c_int(-1)
    capi.lib().voltrix_launch_dropout_mask(ctypes.c_int64(nnz), ctypes.c_int(heads), ctypes.c_uint32(threshold), ctypes.c_uint64(seed),
                                           ctypes.c_uint64(offset), ptr, None, ctypes.byref(rc))
    return rc.value


def test_generator_argument_validation_on_the_host():
    assert _mask_call(heads=0) == BAD and _mask_call(heads=-1) == BAD
    assert _mask_call(heads=0, nnz=0) == BAD                                             # heads is checked before "nothing to do"
    assert _mask_call(nnz=-1) == BAD and _mask_call(nnz=2 ** 31) == BAD
    assert _mask_call(null=True) == BAD and _mask_call(offset_bytes=2) == BAD and _mask_call(offset_bytes=1) == BAD
    assert _mask_call(nnz=0) == OK and _mask_call(nnz=0, null=True) == OK                # nothing to do: no launch


FORWARD = base.FORWARD + ("mask",)
GRAD_SCORES = base.GRAD_SCORES + ("mask",)
GRAD_FEAT = base.GRAD_FEAT + ("mask",)


def _forward(num_rows=4, nnz=6, heads=2, head_dim=16, dtype=F16, scale=1.0, null=None, offset=None, keep_scale=2.5):
    bufs, p = base._ptrs(FORWARD, base._nulls(null), offset)
    rc = ctypes.c_int(-1)
    capi.lib().voltrix_launch_attn_aggregate_dropout_csr(p["indptr"], p["indices"], p["scores"], ctypes.c_int(num_rows),
                                                         ctypes.c_int64(nnz), ctypes.c_int(heads), ctypes.c_int(head_dim), p["feat"],
                                                         ctypes.c_int(dtype), ctypes.c_float(scale), p["out"], p["m"], p["l"], p["mask"],
                                                         ctypes.c_float(keep_scale), None, ctypes.byref(rc))
    return rc.value


def _grad_scores(num_rows=4, nnz=6, heads=2, head_dim=16, dtype=F16, scale=1.0, null=None, offset=None, keep_scale=2.5):
    bufs, p = base._ptrs(GRAD_SCORES, base._nulls(null), offset)
    rc = ctypes.c_int(-1)
    capi.lib().voltrix_launch_attn_aggregate_dropout_grad_scores_csr(
        p["indptr"], p["indices"], ctypes.c_int(num_rows), ctypes.c_int64(nnz), ctypes.c_int(heads), ctypes.c_int(head_dim),
        p["grad_out"], p["feat"], ctypes.c_int(dtype), p["scores"], p["m"], p["l"], p["delta"], ctypes.c_float(scale), p["out"],
        p["mask"], ctypes.c_float(keep_scale), None, ctypes.byref(rc))
    return rc.value


def _grad_feat(num_rows=4, nnz=6, heads=2, head_dim=16, dtype=F32, scale=1.0, null=None, offset=None, keep_scale=2.5):
    bufs, p = base._ptrs(GRAD_FEAT, base._nulls(null), offset)
    rc = ctypes.c_int(-1)
    capi.lib().voltrix_launch_attn_aggregate_dropout_grad_feat_csr(
        p["indptr"], p["indices"], p["order"], ctypes.c_int(num_rows), ctypes.c_int64(nnz), ctypes.c_int(heads), ctypes.c_int(head_dim),
        p["grad_out"], ctypes.c_int(dtype), p["scores"], p["m"], p["l"], ctypes.c_float(scale), p["out"], p["mask"],
        ctypes.c_float(keep_scale), None, ctypes.byref(rc))
    return rc.value


def _keep_scale_checks(call):
    for bad in (float("inf"), float("-inf"), float("nan"), -1.0, -2.0 ** -140):
        assert call(keep_scale=bad) == BAD, bad
        assert call(keep_scale=bad, nnz=0, num_rows=0) == BAD, bad                       # before "nothing to do", like scale
    assert call(keep_scale=0.0, nnz=0, num_rows=0) == OK


def test_forward_argument_validation_on_the_host():
    base._shared_checks(_forward, FORWARD, base.ALIGN16["forward"])                      # the mask: null, and 2 bytes off
    _keep_scale_checks(_forward)
    assert _forward(num_rows=0, nnz=0) == OK and _forward(num_rows=0, nnz=0, null=FORWARD) == OK
    assert _forward(head_dim=0) == OK and _forward(head_dim=0, null=FORWARD) == OK
    for name in ("indptr", "out", "m", "l"):
        assert _forward(nnz=0, null=name) == BAD, name
    assert _forward(nnz=0, offset=("out", 8)) == BAD


def test_grad_scores_argument_validation_on_the_host():
    base._shared_checks(_grad_scores, GRAD_SCORES, base.ALIGN16["grad_scores"])
    _keep_scale_checks(_grad_scores)
    assert _grad_scores(nnz=0) == OK and _grad_scores(nnz=0, null=GRAD_SCORES) == OK and _grad_scores(nnz=0, num_rows=0) == OK
    assert _grad_scores(head_dim=0) == OK and _grad_scores(head_dim=0, null=GRAD_SCORES) == OK


def test_grad_feat_argument_validation_on_the_host():
    base._shared_checks(_grad_feat, GRAD_FEAT, base.ALIGN16["grad_feat"])
    _keep_scale_checks(_grad_feat)
    assert _grad_feat(num_rows=0, nnz=0) == OK and _grad_feat(num_rows=0, nnz=0, null=GRAD_FEAT) == OK
    assert _grad_feat(head_dim=0) == OK and _grad_feat(head_dim=0, null=GRAD_FEAT) == OK
    for name in ("indptr", "out"):
        assert _grad_feat(nnz=0, null=name) == BAD, name


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
    src = tmp_path / "attn_dropout.hip"
    src.write_text(SOURCE)
    inc = os.path.join(REPO, "voltrix-spmm_amd", "voltrix", "include")
    run = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", inc,
                          "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", str(tmp_path / "attn_dropout.o")],
                         capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    # the masked instantiations carry the template argument `true` (Lb1 in the mangled name); the generator is not a template
    keys = ("attn_aggregate_csr_kernel", "attn_aggregate_grad_scores_kernel", "attn_aggregate_grad_feat_kernel", "dropout_mask_kernel")
    usage = {key: {} for key in keys}
    for block in run.stderr.split("remark: Function Name: ")[1:]:
        name = block.split(" ")[0].strip()
        for key in keys:
            if key in name and (key == "dropout_mask_kernel" or "Lb1" in name):
                usage[key][name] = (int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1)),
                                    int(re.search(r"LDS Size \[bytes/block\]: (\d+)", block).group(1)))
    assert [len(usage[key]) for key in keys] == [3, 6, 3, 1], {k: sorted(v) for k, v in usage.items()}
    for group in usage.values():
        assert all(v == (0, 0) for v in group.values()), group
