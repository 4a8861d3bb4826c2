"""CPU: the fused softmax-and-aggregate operator's three C-ABI entry points are declared, bound and exported; their argument checks
answer on the host before any launch; every kernel instantiation compiles for gfx950 without scratch.  No GPU compute is called here."""
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


def _ptrs(names, null, offset):
    # host buffers: every call below is refused (or has nothing to do) before a pointer is dereferenced or a kernel launched
    bufs = {k: np.zeros(4096 + 16, np.uint8) for k in names}
    base = {k: b.ctypes.data + (-b.ctypes.data) % 16 for k, b in bufs.items()}
    ptrs = {k: None if k in null else ctypes.c_void_p(base[k] + (offset[1] if offset and offset[0] == k else 0)) for k in names}
    return bufs, ptrs


def _nulls(null):
    return () if null is None else ((null,) if isinstance(null, str) else tuple(null))


FORWARD = ("indptr", "indices", "scores", "feat", "out", "m", "l")
GRAD_SCORES = ("indptr", "indices", "grad_out", "feat", "scores", "m", "l", "delta", "out")
GRAD_FEAT = ("indptr", "indices", "order", "grad_out", "scores", "m", "l", "out")
ALIGN16 = {"forward": ("feat", "out"), "grad_scores": ("grad_out", "feat"), "grad_feat": ("grad_out", "out")}


def _forward(num_rows=4, nnz=6, heads=2, head_dim=16, dtype=F16, scale=1.0, null=None, offset=None):
    bufs, p = _ptrs(FORWARD, _nulls(null), offset)
    rc = ctypes.c_int(-1)
    capi.lib().voltrix_launch_attn_aggregate_csr(p["indptr"], p["indices"], p["scores"], ctypes.c_int(num_rows), ctypes.c_int64(nnz),
                                                 ctypes.c_int(heads), ctypes.c_int(head_dim), p["feat"], ctypes.c_int(dtype),
                                                 ctypes.c_float(scale), p["out"], p["m"], p["l"], None, ctypes.byref(rc))
    return rc.value


def _grad_scores(num_rows=4, nnz=6, heads=2, head_dim=16, dtype=F16, scale=1.0, null=None, offset=None):
    bufs, p = _ptrs(GRAD_SCORES, _nulls(null), offset)
    rc = ctypes.c_int(-1)
    capi.lib().voltrix_launch_attn_aggregate_grad_scores_csr(p["indptr"], p["indices"], ctypes.c_int(num_rows), ctypes.c_int64(nnz),
                                                             ctypes.c_int(heads), ctypes.c_int(head_dim), p["grad_out"], p["feat"],
                                                             ctypes.c_int(dtype), p["scores"], p["m"], p["l"], p["delta"],
                                                             ctypes.c_float(scale), p["out"], None, ctypes.byref(rc))
    return rc.value


def _grad_feat(num_rows=4, nnz=6, heads=2, head_dim=16, dtype=F32, scale=1.0, null=None, offset=None):
    bufs, p = _ptrs(GRAD_FEAT, _nulls(null), offset)
    rc = ctypes.c_int(-1)
    capi.lib().voltrix_launch_attn_aggregate_grad_feat_csr(p["indptr"], p["indices"], p["order"], ctypes.c_int(num_rows),
                                                           ctypes.c_int64(nnz), ctypes.c_int(heads), ctypes.c_int(head_dim),
                                                           p["grad_out"], ctypes.c_int(dtype), p["scores"], p["m"], p["l"],
                                                           ctypes.c_float(scale), p["out"], None, ctypes.byref(rc))
    return rc.value


def _shared_checks(call, names, align16):
    assert call(heads=0) == VOLTRIX_ERR_BAD_SHAPE
    assert call(heads=-2) == VOLTRIX_ERR_BAD_SHAPE
    assert call(heads=0, num_rows=0, nnz=0) == VOLTRIX_ERR_BAD_SHAPE                   # heads is checked before "nothing to do"
    assert call(num_rows=-1) == VOLTRIX_ERR_BAD_SHAPE
    assert call(nnz=-1) == VOLTRIX_ERR_BAD_SHAPE
    assert call(head_dim=-8) == VOLTRIX_ERR_BAD_SHAPE
    assert call(nnz=2 ** 31) == VOLTRIX_ERR_BAD_SHAPE                                  # nnz > INT_MAX
    assert call(heads=2 ** 20, head_dim=2 ** 12) == VOLTRIX_ERR_BAD_SHAPE              # heads * head_dim > INT_MAX
    assert call(num_rows=0) == VOLTRIX_ERR_BAD_SHAPE                                   # entries but no row
    assert call(head_dim=12, dtype=F16) == VOLTRIX_ERR_BAD_SHAPE                       # 16-bit rows: head_dim % 8
    assert call(head_dim=20, dtype=BF16) == VOLTRIX_ERR_BAD_SHAPE
    assert call(head_dim=6, dtype=F32) == VOLTRIX_ERR_BAD_SHAPE                        # fp32 rows: head_dim % 4
    assert call(dtype=3) == VOLTRIX_ERR_BAD_SHAPE
    assert call(dtype=-1) == VOLTRIX_ERR_BAD_SHAPE
    for scale in (float("inf"), float("-inf"), float("nan")):
        assert call(scale=scale) == VOLTRIX_ERR_BAD_SHAPE, scale
        assert call(scale=scale, nnz=0, num_rows=0) == VOLTRIX_ERR_BAD_SHAPE, scale    # also before "nothing to do"
    for name in names:
        assert call(null=name) == VOLTRIX_ERR_BAD_SHAPE, name
        if name in align16:
            assert call(offset=(name, 8)) == VOLTRIX_ERR_BAD_SHAPE, name               # not 16-byte aligned
            assert call(offset=(name, 4)) == VOLTRIX_ERR_BAD_SHAPE, name
        else:
            assert call(offset=(name, 2)) == VOLTRIX_ERR_BAD_SHAPE, name               # not 4-byte aligned


def test_forward_argument_validation_on_the_host():
    _shared_checks(_forward, FORWARD, ALIGN16["forward"])
    assert _forward(num_rows=0, nnz=0) == VOLTRIX_OK                                   # nothing to do: no launch
    assert _forward(num_rows=0, nnz=0, null=FORWARD) == VOLTRIX_OK
    assert _forward(head_dim=0) == VOLTRIX_OK
    assert _forward(head_dim=0, null=FORWARD) == VOLTRIX_OK
    # nnz == 0 with rows still zero-fills out and l: the outputs (and indptr) must be valid, the operands of the edges need not be
    for name in ("indptr", "out", "m", "l"):
        assert _forward(nnz=0, null=name) == VOLTRIX_ERR_BAD_SHAPE, name
    assert _forward(nnz=0, offset=("out", 8)) == VOLTRIX_ERR_BAD_SHAPE


def test_grad_scores_argument_validation_on_the_host():
    _shared_checks(_grad_scores, GRAD_SCORES, ALIGN16["grad_scores"])
    assert _grad_scores(nnz=0) == VOLTRIX_OK                                           # nothing to do: no launch
    assert _grad_scores(nnz=0, null=GRAD_SCORES) == VOLTRIX_OK
    assert _grad_scores(nnz=0, num_rows=0) == VOLTRIX_OK
    assert _grad_scores(head_dim=0) == VOLTRIX_OK
    assert _grad_scores(head_dim=0, null=GRAD_SCORES) == VOLTRIX_OK


def test_grad_feat_argument_validation_on_the_host():
    _shared_checks(_grad_feat, GRAD_FEAT, ALIGN16["grad_feat"])
    assert _grad_feat(num_rows=0, nnz=0) == VOLTRIX_OK                                 # nothing to do: no launch
    assert _grad_feat(num_rows=0, nnz=0, null=GRAD_FEAT) == VOLTRIX_OK
    assert _grad_feat(head_dim=0) == VOLTRIX_OK
    assert _grad_feat(head_dim=0, null=GRAD_FEAT) == VOLTRIX_OK
    for name in ("indptr", "out"):                                                     # nnz == 0 with rows zero-fills grad_feat
        assert _grad_feat(nnz=0, null=name) == VOLTRIX_ERR_BAD_SHAPE, name


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
    src = tmp_path / "attn_aggregate.hip"
    src.write_text(SOURCE)
    inc = os.path.join(REPO, "voltrix-spmm_amd", "voltrix", "include")
    run = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", inc,
                          "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", str(tmp_path / "attn_aggregate.o")],
                         capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    usage = {"attn_aggregate_csr_kernel": {}, "attn_aggregate_grad_scores_kernel": {}, "attn_aggregate_grad_feat_kernel": {}}
    lds = {}
    for block in run.stderr.split("remark: Function Name: ")[1:]:
        name = block.split(" ")[0]
        for key in usage:
            if key in name:
                usage[key][name] = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1))
                lds[name] = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", block).group(1))
    # 3 feature types ; 3 feature types x (one piece per lane, any number) ; 3 gradient types
    assert len(usage["attn_aggregate_csr_kernel"]) == 3, sorted(usage["attn_aggregate_csr_kernel"])
    assert len(usage["attn_aggregate_grad_scores_kernel"]) == 6, sorted(usage["attn_aggregate_grad_scores_kernel"])
    assert len(usage["attn_aggregate_grad_feat_kernel"]) == 3, sorted(usage["attn_aggregate_grad_feat_kernel"])
    for group in usage.values():
        assert all(v == 0 for v in group.values()), group
    assert all(v == 0 for v in lds.values()), lds                                      # no LDS either
