"""ctypes binding of the ahead-of-time C-ABI library ``lib/libvoltrix_hip.so`` (include/voltrix_capi.h).

The library is the drop-in boundary for non-Python hosts and the home of the gfx950 extensions that have no
reference counterpart (fused GPU preprocess, fp16 operand, tile enumeration).  There is NO fallback: if the
library is missing it is built with hipcc (csrc/Makefile); if that fails the import error is raised.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
LIB_PATH = os.path.join(_ROOT, "lib", "libvoltrix_hip.so")
CSRC_DIR = os.path.join(_ROOT, "csrc")

_lib = None

# ---- the binding: one entry per symbol include/voltrix_capi.h declares, ``name: (return type, [parameter types])``.  lib() sets
# ---- restype and argtypes of every symbol from it, so plain ints, floats, data_ptr() values and None convert in C (12 -> 4 us per
# ---- call on the host) and a wrong width or a missing argument is a ctypes.ArgumentError / TypeError before the library is entered.
# ---- tests/test_capi_symbols.py compares every entry with the header's prototype: a new entry point is one line here.  The order is
# ---- the one SYMBOLS has always had (the header's, but for a few entry points it declares further down).
_P, _I, _L, _F, _D, _RC_P = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.POINTER(ctypes.c_int)
_U32, _U64 = ctypes.c_uint32, ctypes.c_uint64
SIGNATURES = {
    "voltrix_abi_version": (_I, []),
    "voltrix_launch_preprocess": (None, [_P, _P, _I, _P, _P, _P, _P, _RC_P]),
    "voltrix_launch_hmat_gen": (None, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _RC_P]),
    "voltrix_launch_hmat_packed_swizzle": (None, [_I, _P, _P, _P, _RC_P]),
    "voltrix_launch_spmm": (None, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _RC_P]),
    "voltrix_launch_spmm_f32_tile": (None, [_P, _P, _P, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P, _P, _RC_P]),
    "voltrix_launch_spmm_f16": (None, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _RC_P]),
    "voltrix_launch_spmm_f16_tile": (None, [_P, _P, _P, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P, _P, _RC_P]),
    "voltrix_spmm_f32_workspace_bytes": (_L, [_L, _I]),
    "voltrix_launch_spmm_f32_as_f16": (None, [_P, _P, _P, _I, _I, _I, _P, _L, _P, _P, _P, _RC_P]),
    "voltrix_launch_spmm_f16_sched": (None, [_P, _P, _P, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P, _I, _P, _P, _I, _P, _P, _I, _P, _RC_P]),
    "voltrix_launch_spmm_bf16_sched": (None, [_P, _P, _P, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P, _I, _P, _P, _I, _P, _P, _I, _P, _RC_P]),
    "voltrix_launch_combine_partials": (None, [_P, _I, _P, _P, _I, _I, _I, _P, _P, _RC_P]),
    "voltrix_stream_table_workspace_bytes": (_L, [_I]),
    "voltrix_stream_table_fill_workspace_bytes": (_L, [_L]),
    "voltrix_launch_stream_table_count": (None, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _RC_P]),
    "voltrix_launch_stream_table_fill": (None, [_P, _I, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _RC_P]),
    "voltrix_launch_spmm_stream_f16": (None, [_P, _P, _I, _I, _P, _L, _P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _P, _RC_P]),
    "voltrix_launch_spmm_stream_bf16": (None, [_P, _P, _I, _I, _P, _L, _P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _P, _RC_P]),
    "voltrix_launch_spmm_panel_f16": (None, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _L, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _RC_P]),
    "voltrix_launch_spmm_panel_bf16": (None, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _L, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _RC_P]),
    "voltrix_launch_spmm_panel_parts_f16": (None, [_P, _P, _P, _P, _I, _P, _I, _P, _I, _I, _P, _L, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _RC_P]),
    "voltrix_launch_spmm_panel_parts_bf16": (None, [_P, _P, _P, _P, _I, _P, _I, _P, _I, _I, _P, _L, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _RC_P]),
    "voltrix_launch_combine_panel_partials": (None, [_P, _I, _P, _P, _I, _I, _I, _I, _P, _RC_P]),
    "voltrix_launch_spmm_f16_sched_ticket": (None, [_P, _P, _P, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P, _P, _I, _P, _I, _P, _P, _RC_P]),
    "voltrix_launch_spmm_bf16_sched_ticket": (None, [_P, _P, _P, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P, _P, _I, _P, _I, _P, _P, _RC_P]),
    "voltrix_launch_combine_partials_ticket": (None, [_P, _I, _P, _P, _I, _I, _P, _P, _RC_P]),
    "voltrix_launch_spmm_panel_ticket_f16": (None, [_P, _P, _P, _P, _P, _I, _P, _I, _P, _P, _I, _I, _P, _L, _P, _I, _I, _I, _I, _I, _I, _P, _P, _RC_P]),
    "voltrix_launch_spmm_panel_ticket_bf16": (None, [_P, _P, _P, _P, _P, _I, _P, _I, _P, _P, _I, _I, _P, _L, _P, _I, _I, _I, _I, _I, _I, _P, _P, _RC_P]),
    "voltrix_launch_combine_panel_partials_ticket": (None, [_P, _I, _P, _P, _I, _I, _I, _P, _P, _RC_P]),
    "voltrix_launch_xcd_ranges_of_work": (None, [_P, _I, _I, _P, _P, _RC_P]),
    "voltrix_launch_xcd_ranges_of_windows": (None, [_P, _I, _I, _P, _P, _RC_P]),
    "voltrix_launch_xcd_ranges_of_panels": (None, [_P, _P, _I, _I, _I, _P, _P, _P, _RC_P]),
    "voltrix_panel_parts_workspace_bytes": (_L, [_I]),
    "voltrix_launch_panel_parts_count": (None, [_P, _I, _I, _P, _P, _P, _P, _RC_P]),
    "voltrix_launch_panel_parts_fill": (None, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _RC_P]),
    "voltrix_launch_spmm_fused_f16": (None, [_P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _P, _P, _I, _I, _I, _P, _P, _RC_P]),
    "voltrix_launch_spmm_fused_bf16": (None, [_P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _P, _P, _I, _I, _I, _P, _P, _RC_P]),
    "voltrix_fused_panel_geometry": (None, [_RC_P, _RC_P]),
    "voltrix_fused_records_workspace_bytes": (_L, [_I]),
    "voltrix_launch_fused_records_count": (None, [_P, _P, _I, _P, _P, _P, _RC_P]),
    "voltrix_launch_fused_records_fill": (None, [_P, _P, _P, _I, _P, _L, _P, _P, _RC_P]),
    "voltrix_panel_plan_workspace_bytes": (_L, [_I, _I, _I]),
    "voltrix_launch_panel_plan_count": (None, [_P, _P, _I, _I, _L, _I, _I, _I, _P, _P, _P, _P, _P, _RC_P]),
    "voltrix_launch_panel_plan_fill": (None, [_P, _P, _I, _I, _L, _I, _I, _I, _P, _P, _P, _L, _P, _P, _P, _P, _RC_P]),
    "voltrix_launch_panel_order": (None, [_P, _I, _I, _P, _P, _P, _RC_P]),
    "voltrix_spmm_default_tile": (None, [_I, _I, _RC_P, _RC_P, _RC_P]),
    "voltrix_spmm_num_tiles": (_I, [_I]),
    "voltrix_spmm_tile_at": (None, [_I, _I, _RC_P, _RC_P, _RC_P]),
    "voltrix_launch_window_order": (None, [_P, _I, _I, _P, _P, _RC_P]),
    "voltrix_launch_spmm_bf16": (None, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _RC_P]),
    "voltrix_launch_spmm_bf16_tile": (None, [_P, _P, _P, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P, _P, _RC_P]),
    "voltrix_launch_cast_f32_f16": (None, [_P, _P, _L, _P, _RC_P]),
    "voltrix_launch_cast_f32_f16_scaled": (None, [_P, _P, _L, _P, _P, _RC_P]),
    "voltrix_launch_scale_rows": (None, [_P, _P, _P, _L, _I, _I, _P, _RC_P]),
    "voltrix_launch_spmm_csr_rows": (None, [_P, _P, _I, _I, _P, _I, _P, _I, _P, _RC_P]),
    "voltrix_launch_spmm_csr_rows_weighted": (None, [_P, _P, _P, _I, _I, _P, _I, _P, _I, _P, _RC_P]),
    "voltrix_launch_scatter_values": (None, [_P, _P, _P, _L, _I, _P, _RC_P]),
    "voltrix_launch_sddmm_csr": (None, [_P, _P, _I, _L, _I, _P, _I, _P, _I, _P, _P, _RC_P]),
    "voltrix_edge_softmax_workspace_bytes": (_L, [_I, _L]),
    "voltrix_launch_edge_softmax_csr": (None, [_P, _I, _L, _P, _F, _P, _P, _P, _RC_P]),
    "voltrix_launch_edge_softmax_backward_csr": (None, [_P, _I, _L, _P, _P, _F, _P, _P, _P, _RC_P]),
    "voltrix_launch_sddmm_heads_csr": (None, [_P, _P, _I, _L, _I, _I, _P, _I, _P, _I, _P, _P, _RC_P]),
    "voltrix_edge_softmax_heads_workspace_bytes": (_L, [_I, _L, _I]),
    "voltrix_launch_edge_softmax_heads_csr": (None, [_P, _I, _L, _I, _P, _F, _P, _P, _P, _RC_P]),
    "voltrix_launch_edge_softmax_heads_backward_csr": (None, [_P, _I, _L, _I, _P, _P, _F, _P, _P, _P, _RC_P]),
    "voltrix_launch_spmm_csr_heads": (None, [_P, _P, _P, _I, _I, _I, _P, _I, _P, _P, _RC_P]),
    "voltrix_launch_gat_score_csr": (None, [_P, _P, _I, _L, _I, _P, _P, _F, _P, _P, _RC_P]),
    "voltrix_gat_score_workspace_bytes": (_L, [_I, _L, _I]),
    "voltrix_launch_gat_score_rowsum_csr": (None, [_P, _P, _P, _I, _L, _I, _P, _P, _P, _F, _P, _P, _P, _RC_P]),
    "voltrix_launch_gatv2_score_csr": (None, [_P, _P, _I, _L, _I, _I, _P, _P, _I, _P, _F, _P, _P, _RC_P]),
    "voltrix_launch_gatv2_rowsum_csr": (None, [_P, _P, _P, _I, _L, _I, _I, _P, _P, _I, _P, _F, _P, _P, _RC_P]),
    "voltrix_launch_attn_aggregate_csr": (None, [_P, _P, _P, _I, _L, _I, _I, _P, _I, _F, _P, _P, _P, _P, _RC_P]),
    "voltrix_launch_attn_aggregate_grad_scores_csr": (None, [_P, _P, _I, _L, _I, _I, _P, _P, _I, _P, _P, _P, _P, _F, _P, _P, _RC_P]),
    "voltrix_launch_attn_aggregate_grad_feat_csr": (None, [_P, _P, _P, _I, _L, _I, _I, _P, _I, _P, _P, _P, _F, _P, _P, _RC_P]),
    "voltrix_launch_dropout_mask": (None, [_L, _I, _U32, _U64, _U64, _P, _P, _RC_P]),
    "voltrix_launch_attn_aggregate_dropout_csr": (None, [_P, _P, _P, _I, _L, _I, _I, _P, _I, _F, _P, _P, _P, _P, _F, _P, _RC_P]),
    "voltrix_launch_attn_aggregate_dropout_grad_scores_csr": (None, [_P, _P, _I, _L, _I, _I, _P, _P, _I, _P, _P, _P, _P, _F, _P, _P, _F, _P, _RC_P]),
    "voltrix_launch_attn_aggregate_dropout_grad_feat_csr": (None, [_P, _P, _P, _I, _L, _I, _I, _P, _I, _P, _P, _P, _F, _P, _P, _F, _P, _RC_P]),
    "voltrix_launch_spmm_csr_reduce": (None, [_P, _P, _I, _I, _P, _I, _I, _P, _P, _P, _RC_P]),
    "voltrix_launch_spmm_csr_reduce_backward": (None, [_P, _P, _P, _I, _L, _I, _P, _P, _P, _P, _RC_P]),
    "voltrix_spmm_edge_csr": (_I, [_P, _P, _P, _I, _L, _I, _P, _I, _P, _I, _P, _I, _P, _P]),
    "voltrix_spmm_edge_grad_efeat_csr": (_I, [_P, _P, _I, _L, _I, _P, _P, _P, _I, _I, _P, _P]),
    "voltrix_spmm_rel_csr": (_I, [_P, _P, _P, _P, _I, _L, _I, _I, _I, _P, _I, _P, _P, _P]),
    "voltrix_spmm_rel_contract_csr": (_I, [_P, _P, _P, _P, _P, _I, _L, _I, _I, _I, _P, _P, _P, _P]),
    "voltrix_spmm_rel_dots_csr": (_I, [_P, _P, _P, _I, _L, _I, _I, _P, _P, _I, _P, _P]),
    "voltrix_quantize_fp8_rows": (_I, [_P, _I, _I, _I, _L, _P, _P, _L, _P]),
    "voltrix_spmm_fp8_csr": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _I, _I, _L, _P]),
    "voltrix_spmm_multi_csr": (_I, [_P, _P, _I, _L, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _F, _P, _P, _P, _P]),
    "voltrix_spmm_multi_backward_csr": (_I, [_P, _P, _P, _I, _L, _I, _P, _P, _P, _P, _L, _P, _P, _P, _P, _P, _P]),
    "voltrix_launch_sample_neighbors": (None, [_P, _P, _I, _P, _I, _P, _L, _I, _I, _U64, _U64, _P, _P, _P, _RC_P]),
    "voltrix_launch_block_mark": (None, [_P, _L, _I, _P, _P, _RC_P]),
    "voltrix_launch_block_mark_seeds": (None, [_P, _I, _I, _P, _P, _RC_P]),
    "voltrix_launch_block_relabel": (None, [_P, _L, _P, _I, _P, _P, _I, _I, _P, _P, _P, _RC_P]),
    "voltrix_launch_subgraph_count": (None, [_P, _P, _I, _P, _I, _P, _I, _I, _P, _P, _RC_P]),
    "voltrix_launch_subgraph_fill": (None, [_P, _P, _I, _P, _I, _P, _I, _I, _P, _L, _P, _P, _P, _RC_P]),
    "voltrix_launch_random_walk": (None, [_P, _P, _I, _P, _I, _I, _U64, _U64, _P, _P, _I, _P, _RC_P]),
    "voltrix_launch_negative_sample": (None, [_P, _P, _I, _I, _L, _P, _I, _I, _I, _I, _I, _U64, _U64, _P, _P, _RC_P]),
    "voltrix_launch_edge_endpoints": (None, [_P, _P, _I, _L, _P, _I, _P, _P, _P, _RC_P]),
    "voltrix_launch_sample_neighbors_excluding": (None, [_P, _P, _I, _P, _I, _P, _L, _I, _I, _U64, _U64, _P, _I, _P, _P, _P, _RC_P]),
    "voltrix_sample_neighbors_weighted": (None, [_P, _P, _P, _I, _P, _I, _P, _L, _I, _I, _U64, _U64, _P, _P, _P, _RC_P]),
    "voltrix_launch_find_edges": (None, [_P, _P, _I, _L, _P, _P, _I, _I, _P, _P, _RC_P]),
    "voltrix_csr_preprocess_workspace_bytes": (_L, [_I, _I, _L, _I]),
    "voltrix_launch_csr_window_count": (None, [_P, _P, _I, _I, _L, _I, _P, _P, _P, _P, _P, _RC_P]),
    "voltrix_launch_csr_fill": (None, [_P, _P, _I, _I, _L, _I, _P, _P, _P, _P, _P, _RC_P]),
    "voltrix_unit_table_workspace_bytes": (_L, [_I]),
    "voltrix_unit_table_fill_workspace_bytes": (_L, [_L]),
    "voltrix_launch_unit_table_count": (None, [_P, _I, _I, _P, _P, _P, _P, _RC_P]),
    "voltrix_launch_unit_table_fill": (None, [_P, _I, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _RC_P]),
    "voltrix_csr_transpose_workspace_bytes": (_L, [_L]),
    "voltrix_launch_csr_transpose": (None, [_P, _P, _I, _I, _L, _P, _P, _P, _P, _RC_P]),
    "voltrix_launch_bfs_seed": (None, [_I, _I, _P, _P, _P, _P, _P, _RC_P]),
    "voltrix_launch_bfs_levels": (None, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _I, _P, _RC_P]),
    "voltrix_cm_rank_workspace_bytes": (_L, [_L]),
    "voltrix_launch_cm_rank": (None, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _RC_P, _I, _I, _P, _P, _RC_P]),
    "voltrix_launch_chol_inv_transposed": (None, [_P, _I, _D, _P, _P, _RC_P]),
}
SYMBOLS = tuple(SIGNATURES)


def build(force: bool = False) -> str:
    """Compile the library for gfx950 (works without a GPU)."""
    cmd = ["make", "-s", "-C", CSRC_DIR, "-j4"]
    if force:
        subprocess.check_call(["make", "-s", "-C", CSRC_DIR, "clean"])
    subprocess.check_call(cmd)
    return LIB_PATH


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        loaded = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():   # e.g. a size function left at the default restype (int) would cut a
            fn = getattr(loaded, name)                         # size above 2^31 - 1 short, and the workspace allocated from it would
            fn.restype, fn.argtypes = restype, argtypes        # be too small for the launch
        _lib = loaded
    return _lib


class VoltrixError(RuntimeError):
    pass


_RC = {1: "bad shape / alignment", 2: "HIP launch error", 3: "tile configuration not instantiated",
       4: "int32 overflow of the block format", 5: "duplicate CSR entries"}


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise VoltrixError(f"{what}: return code {rc} ({_RC.get(rc, 'unknown')})")


def _call(name: str, *args) -> int:
    """Entry point ``name`` on ``args`` and a return-code slot of its own (the last parameter of every launcher); returns the code."""
    rc = ctypes.c_int(-1)
    getattr(lib(), name)(*args, rc)
    return rc.value


def _checked(name: str, *args) -> None:
    """The same for the wrappers that raise: ``VoltrixError`` unless the code is 0 (not through ``_call``: one frame less per launch)."""
    rc = ctypes.c_int(-1)
    getattr(lib(), name)(*args, rc)
    if rc.value != 0:
        check(rc.value, name)


def _ptr(t):
    """``t``'s address as a ``void*`` for raw calls of the library (tests, experiments): unlike a plain int it keeps its 64 bits in a
    call of a function without argument types as well.  The wrappers below pass ``data_ptr()`` itself."""
    return ctypes.c_void_p(t.data_ptr())


def _opt(t):
    """The address of an optional tensor argument: None, the null pointer, where there is none."""
    return None if t is None else t.data_ptr()


def _stream_of(stream):
    """``stream``, or torch's current stream where the caller gave None."""
    if stream is not None:
        return stream
    import torch

    return torch.cuda.current_stream().cuda_stream


_CODES = None


def _dtype_code(dtype) -> int:
    """The ``dtype`` argument of the entry points that take one: 0 fp32 / 1 fp16 / 2 bfloat16."""
    import torch

    global _CODES
    if _CODES is None:
        _CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
    return _CODES[dtype]


# ---- kernel-isolated timing hook (utils.KernelTimer / bench_kineto): a launch wrapper decorated with ``@_timed(label)`` is bracketed
# ---- by an event pair on its stream while a timer is active; free otherwise.  The stream is the wrapper's parameter named ``stream``.
def _timed(label: str):
    import functools
    import inspect

    def decorate(fn):
        stream_index = list(inspect.signature(fn).parameters).index("stream")

        @functools.wraps(fn)
        def wrapper(*args, **kwargs):
            from .utils import KernelTimer

            if KernelTimer.active is None:
                return fn(*args, **kwargs)
            stream = kwargs.get("stream")
            if stream is None and len(args) > stream_index:
                stream = args[stream_index]
            with KernelTimer.active.bracket(label, stream):
                return fn(*args, **kwargs)

        wrapper.timer_label, wrapper.stream_index = label, stream_index
        return wrapper

    return decorate


def default_tile(embedding_dim: int, is_f16: bool):
    fs, d, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    lib().voltrix_spmm_default_tile(embedding_dim, int(is_f16), fs, d, w)
    return fs.value, d.value, w.value


def tiles(is_f16: bool):
    out = []
    for i in range(lib().voltrix_spmm_num_tiles(int(is_f16))):
        fs, d, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        lib().voltrix_spmm_tile_at(int(is_f16), i, fs, d, w)
        out.append((fs.value, d.value, w.value))
    return out


CSR_PATHS = {None: -1, "auto": -1, "sort": 0, "bitmap": 1, "mixed": 2}   # `path` of the fused preprocess entry points
SLAB_AUTO, SLAB_ONE_GRID, SLAB_LAUNCHES = -1, 0, 1                       # `slab_policy` of the SpMM launchers


def csr_preprocess_workspace_bytes(num_nodes: int, num_cols: int, num_edges: int, path=None) -> int:
    return int(lib().voltrix_csr_preprocess_workspace_bytes(num_nodes, num_cols, num_edges, CSR_PATHS[path]))


@_timed("csr_window_count")
def launch_csr_window_count(indptr, indices, num_nodes, num_cols, workspace, block_partition, pointer1, status,
                            stream, path=None) -> None:
    _checked("voltrix_launch_csr_window_count", indptr.data_ptr(), indices.data_ptr(), num_nodes, num_cols, indices.numel(),
             CSR_PATHS[path], workspace.data_ptr(), block_partition.data_ptr(), pointer1.data_ptr(), status.data_ptr(), stream)


@_timed("csr_fill")
def launch_csr_fill(indptr, indices, num_nodes, num_cols, workspace, pointer1, hspa_packed, hind, stream, path=None) -> None:
    _checked("voltrix_launch_csr_fill", indptr.data_ptr(), indices.data_ptr(), num_nodes, num_cols, indices.numel(), CSR_PATHS[path],
             workspace.data_ptr(), pointer1.data_ptr(), hspa_packed.data_ptr(), hind.data_ptr(), stream)


@_timed("spmm")
def launch_spmm(blk_offsets, hspa_packed, hind, num_nodes, num_edges, embedding_dim, input_ptr, output_ptr, is_f16,
                tile, stream, window_order=0, out_scale=0) -> int:
    """Raw-pointer launch (used by bench.py and the tests); ``window_order`` is 0 (natural) or the device pointer of
    the schedule written by :func:`launch_window_order`; ``out_scale`` is 0 or the device pointer of the float written
    by :func:`launch_cast_f32_f16_scaled`.  Returns the return code."""
    if is_f16 == "bf16":  # operand kind: True = fp16, False = fp32, "bf16" = bfloat16 (same tiles as fp16)
        name = "voltrix_launch_spmm_bf16_tile"
    else:
        name = "voltrix_launch_spmm_f16_tile" if is_f16 else "voltrix_launch_spmm_f32_tile"
    return _call(name, blk_offsets, hspa_packed, hind, num_nodes, num_edges, embedding_dim, input_ptr, output_ptr, tile[0], tile[1],
                 tile[2], window_order, out_scale, stream)


@_timed("spmm")
def launch_spmm_sched(blk_offsets, hspa_packed, hind, num_nodes, num_edges, embedding_dim, input_ptr, output_ptr, tile,
                      stream, window_order=0, out_scale=0, atomic_out=False, bf16=False, table=None, partials=0,
                      row_map=0, units_per_wave=1, tickets=0) -> int:
    """16-bit operand launch with the schedule / output extensions (include/voltrix_capi.h): ``atomic_out`` = add the
    result onto a pre-zeroed output with float atomics (two-level format without a join pass); ``table`` = a
    ``voltrix.schedule.UnitTable`` (replaces ``window_order``), ``partials`` = device pointer of its partial tiles.
    ``tickets`` = device pointer of the call's ticket buffer: the ticket join (``voltrix_launch_spmm_*_sched_ticket``; no
    ``window_order``, no ``row_map``, ``atomic_out`` is implied).  Returns the return code."""
    units, unit_ptr, max_units = (table.units.data_ptr(), table.unit_ptr.data_ptr(), table.max_units_per_xcd) if table is not None \
        else (None, None, 0)
    if tickets:
        assert not window_order and not row_map, "the ticket join takes neither a window order nor a row map"
        return _call("voltrix_launch_spmm_bf16_sched_ticket" if bf16 else "voltrix_launch_spmm_f16_sched_ticket", blk_offsets,
                     hspa_packed, hind, num_nodes, num_edges, embedding_dim, input_ptr, output_ptr, tile[0], tile[1], tile[2],
                     out_scale, units, unit_ptr, max_units, partials, int(units_per_wave), tickets, stream)
    return _call("voltrix_launch_spmm_bf16_sched" if bf16 else "voltrix_launch_spmm_f16_sched", blk_offsets, hspa_packed, hind,
                 num_nodes, num_edges, embedding_dim, input_ptr, output_ptr, tile[0], tile[1], tile[2], window_order, out_scale,
                 int(atomic_out), units, unit_ptr, max_units, partials, row_map, int(units_per_wave), stream)


@_timed("combine_partials")
def launch_combine_partials(table, partials_ptr, output_ptr, num_nodes, embedding_dim, accumulate, stream,
                            row_map=0, tickets=0) -> int:
    """Sum the partial tiles of the cut windows of ``table`` (a ``voltrix.schedule.UnitTable``) into the output.  ``tickets``:
    the ticket join's buffer -- blocks no kernel wrote are stored, the others added to (``accumulate`` is implied)."""
    if tickets:
        assert not row_map
        return _call("voltrix_launch_combine_partials_ticket", table.cuts.data_ptr(), table.num_cuts, partials_ptr, output_ptr,
                     num_nodes, embedding_dim, tickets, stream)
    return _call("voltrix_launch_combine_partials", table.cuts.data_ptr(), table.num_cuts, partials_ptr, output_ptr, num_nodes,
                 embedding_dim, int(accumulate), row_map, stream)


def build_unit_table(blk_offsets, num_nodes: int, max_stages: int = 0, stream=None, xcd_ptr=None):
    """The handle's unit table through the library's two-phase builder (voltrix/unit_table.hpp): returns
    ``(units int32 [U, 4], unit_ptr int32 [9], cuts int32 [C, 4], header)`` with ``header`` = the eight ints of phase 1
    as a Python list (num_units, num_cuts, num_slots, max_units_per_xcd, max_stages, top, 0, 0).  ``xcd_ptr``: None (equal
    window ranges per XCD) or a device int32 [9] tensor of first windows (ranges of equal work).  One host sync."""
    import torch

    dev = blk_offsets.device
    stream = _stream_of(stream)
    workspace = torch.empty(max(16, int(lib().voltrix_unit_table_workspace_bytes(num_nodes))), dtype=torch.uint8, device=dev)
    header = torch.empty(8, dtype=torch.int32, device=dev)
    _checked("voltrix_launch_unit_table_count", blk_offsets.data_ptr(), num_nodes, int(max_stages), _opt(xcd_ptr),
             workspace.data_ptr(), header.data_ptr(), stream)
    head = [int(v) for v in header.tolist()]   # the sync
    num_units, num_cuts, top = head[0], head[1], head[5]
    units = torch.empty((num_units, 4), dtype=torch.int32, device=dev)
    cuts = torch.empty((num_cuts, 4), dtype=torch.int32, device=dev)
    unit_ptr = torch.empty(9, dtype=torch.int32, device=dev)
    fill_ws = torch.empty(max(16, int(lib().voltrix_unit_table_fill_workspace_bytes(num_units))), dtype=torch.uint8, device=dev)
    _checked("voltrix_launch_unit_table_fill", blk_offsets.data_ptr(), num_nodes, _opt(xcd_ptr), workspace.data_ptr(),
             fill_ws.data_ptr(), num_units, num_cuts, top, units.data_ptr(), unit_ptr.data_ptr(), cuts.data_ptr(), stream)
    return units, unit_ptr, cuts, head


def build_stream_table(blk_offsets, hspa_packed, hind, num_nodes: int, run_cost: int = 0, cut_stages: int = 0, stream=None):
    """The handle's stream tables through the library's two-phase builder (voltrix/stream_table.hpp): returns ``(units int32
    [U, 8], runs int32 [R, 4], run_ptr int32 [9], cuts int32 [C, 4], header)`` with ``header`` = (num_units, num_cuts, num_slots,
    num_runs, max_runs_per_xcd, run_cost, cut_stages).  Two host syncs (the sizes of the outputs, then the number of runs)."""
    import torch

    dev = blk_offsets.device
    stream = _stream_of(stream)
    workspace = torch.empty(max(16, int(lib().voltrix_stream_table_workspace_bytes(num_nodes))), dtype=torch.uint8, device=dev)
    header = torch.empty(8, dtype=torch.int32, device=dev)
    _checked("voltrix_launch_stream_table_count", blk_offsets.data_ptr(), hspa_packed.data_ptr(), hind.data_ptr(), num_nodes,
             int(run_cost), int(cut_stages), workspace.data_ptr(), header.data_ptr(), stream)
    num_units, num_cuts, num_slots, run_bound, rcost, cut = [int(v) for v in header.tolist()][:6]   # the sync
    units = torch.empty((num_units, 8), dtype=torch.int32, device=dev)
    cuts = torch.empty((num_cuts, 4), dtype=torch.int32, device=dev)
    runs = torch.empty((max(1, run_bound), 4), dtype=torch.int32, device=dev)
    run_ptr = torch.empty(9, dtype=torch.int32, device=dev)
    header2 = torch.empty(4, dtype=torch.int32, device=dev)
    fill_ws = torch.empty(max(16, int(lib().voltrix_stream_table_fill_workspace_bytes(num_units))), dtype=torch.uint8, device=dev)
    _checked("voltrix_launch_stream_table_fill", blk_offsets.data_ptr(), num_nodes, workspace.data_ptr(), fill_ws.data_ptr(),
             num_units, num_cuts, run_bound, max(2, rcost), units.data_ptr(), cuts.data_ptr(), runs.data_ptr(), run_ptr.data_ptr(),
             header2.data_ptr(), stream)
    num_runs, max_runs, oversized = [int(v) for v in header2.tolist()][:3]
    assert oversized == 0, "stream table with a run of more than 64 units (run_cost > 128?): the kernel cannot walk it"
    return units, runs[:num_runs], run_ptr, cuts, (num_units, num_cuts, num_slots, num_runs, max_runs, rcost, cut)


def launch_spmm_stream(hspa_packed, hind, num_nodes: int, embedding_dim: int, feat, output, table, partials, out_scale=None,
                       tile=(0, 0, 0), stream=None, input_rows: int = 0, slab_policy: int = -1) -> int:
    """``voltrix_launch_spmm_stream_f16 / _bf16`` on a ``voltrix.schedule.StreamTable`` (the stream kernel through the C-ABI)."""
    import torch

    stream = _stream_of(stream)
    name = "voltrix_launch_spmm_stream_bf16" if feat.dtype == torch.bfloat16 else "voltrix_launch_spmm_stream_f16"
    from .utils import timed_launch

    with timed_launch("spmm_stream", stream):
        return _call(name, hspa_packed.data_ptr(), hind.data_ptr(), num_nodes, embedding_dim, feat.data_ptr(), int(input_rows),
                     output.data_ptr(), table.units.data_ptr(), table.runs.data_ptr(), table.run_ptr.data_ptr(),
                     table.max_runs_per_xcd, partials.data_ptr(), _opt(out_scale), tile[0], tile[1], tile[2], int(slab_policy), stream)


def xcd_ranges_of_work(work, align: int = 1, stream=None):
    """int32 [9] on ``work``'s device: eight ranges of the int32 items ``work`` with about equal sums
    (voltrix/schedule_tables.hpp; voltrix/schedule.py::split_equal_work is the restatement).  Stream-ordered."""
    import torch

    out = torch.empty(9, dtype=torch.int32, device=work.device)
    _checked("voltrix_launch_xcd_ranges_of_work", work.data_ptr(), work.numel(), int(align), out.data_ptr(), _stream_of(stream))
    return out


def xcd_ranges_of_windows(blk_offsets, num_nodes: int, align: int = 1, stream=None):
    """int32 [9]: first window of every XCD's range, ranges of equal STAGES of the handle ``blk_offsets``."""
    import torch

    out = torch.empty(9, dtype=torch.int32, device=blk_offsets.device)
    _checked("voltrix_launch_xcd_ranges_of_windows", blk_offsets.data_ptr(), num_nodes, int(align), out.data_ptr(), _stream_of(stream))
    return out


def xcd_ranges_of_panels(panel_ptr, resid_blk_offsets, num_nodes: int, panel_rows: int, kstep_cost_x10: int, stream=None):
    """``(xcd_ptr, window_xcd_ptr)`` int32 [9] each: ranges of panels with equal work (``kstep_cost_x10 / 10`` x k-steps +
    residual stages) and the same ranges counted in windows."""
    import torch

    dev = panel_ptr.device
    out, out_w = torch.empty(9, dtype=torch.int32, device=dev), torch.empty(9, dtype=torch.int32, device=dev)
    _checked("voltrix_launch_xcd_ranges_of_panels", panel_ptr.data_ptr(), resid_blk_offsets.data_ptr(), num_nodes, panel_rows,
             int(kstep_cost_x10), out.data_ptr(), out_w.data_ptr(), _stream_of(stream))
    return out, out_w


def build_panel_parts(panel_ptr, cap: int, panel_xcd_ptr=None, stream=None):
    """The panel kernel's piece table through the library's two-phase builder (voltrix/schedule_tables.hpp): returns
    ``(parts int32 [P, 4], part_xcd_ptr int32 [9], cuts int32 [C, 4], header)`` with ``header`` = (pieces, cut panels,
    slots, pieces of the longest XCD range, cap, 0, 0, 0) as a Python list.  One host sync."""
    import torch

    dev = panel_ptr.device
    num_panels = panel_ptr.numel() - 1
    stream = _stream_of(stream)
    workspace = torch.empty(max(16, int(lib().voltrix_panel_parts_workspace_bytes(num_panels))), dtype=torch.uint8, device=dev)
    header = torch.empty(8, dtype=torch.int32, device=dev)
    _checked("voltrix_launch_panel_parts_count", panel_ptr.data_ptr(), num_panels, int(cap), _opt(panel_xcd_ptr), workspace.data_ptr(),
             header.data_ptr(), stream)
    head = [int(v) for v in header.tolist()]   # the sync
    parts = torch.empty((head[0], 4), dtype=torch.int32, device=dev)
    cuts = torch.empty((max(1, head[1]), 4), dtype=torch.int32, device=dev)
    part_xcd_ptr = torch.empty(9, dtype=torch.int32, device=dev)
    _checked("voltrix_launch_panel_parts_fill", panel_ptr.data_ptr(), num_panels, int(cap), _opt(panel_xcd_ptr), workspace.data_ptr(),
             parts.data_ptr(), part_xcd_ptr.data_ptr(), cuts.data_ptr(), stream)
    return parts, part_xcd_ptr, cuts[:head[1]], head


def spmm_f32_workspace_bytes(input_rows: int, embedding_dim: int) -> int:
    return int(lib().voltrix_spmm_f32_workspace_bytes(input_rows, embedding_dim))


@_timed("spmm_f32_as_f16")
def launch_spmm_f32_as_f16(blk_offsets, hspa_packed, hind, num_nodes, num_edges, embedding_dim, feat, output, workspace,
                           stream) -> int:
    """Route B for fp32 features: the reference's launch() arguments + a caller-owned workspace; scaled-fp16 operand on the
    default tile (include/voltrix_capi.h).  Tensors in, return code out."""
    return _call("voltrix_launch_spmm_f32_as_f16", blk_offsets.data_ptr(), hspa_packed.data_ptr(), hind.data_ptr(), num_nodes,
                 num_edges, embedding_dim, feat.data_ptr(), feat.shape[0], output.data_ptr(), workspace.data_ptr(), stream)


@_timed("spmm_panel")
def launch_spmm_panel(plan, input_ptr, output_ptr, embedding_dim, accumulate, bf16, tile, out_scale, stream,
                      input_rows: int = 0, slab_policy: int = SLAB_AUTO, partials_ptr: int = 0, tickets: int = 0) -> int:
    """Panel kernel (shared-column half of the two-level format); ``plan`` = voltrix.hybrid.PanelPlan, ``tile`` =
    (fs, depth, ksteps); ``input_rows`` = rows of the dense operand (0: the plan's rows).  A plan with a part table
    (``plan.parts``) goes through ``voltrix_launch_spmm_panel_parts_*`` with ``partials_ptr`` = the call's partial-tile
    buffer.  ``accumulate`` = 3 with ``tickets`` = the call's ticket buffer: the ticket join
    (``voltrix_launch_spmm_panel_ticket_*``).  Returns the return code."""
    panel = (plan.panel_ptr.data_ptr(), plan.panel_cols.data_ptr(), plan.panel_bits.data_ptr())
    if int(accumulate) == 3:
        parts, xcd_ptr = getattr(plan, "parts", None), getattr(plan, "xcd_ptr", None)
        if parts is not None:
            table = (None, parts.parts.data_ptr(), parts.num_parts, parts.xcd_ptr.data_ptr(), parts.max_parts_per_xcd)
        else:
            table = (_opt(plan.panel_order), None, 0, _opt(xcd_ptr), plan.max_panels_per_xcd if xcd_ptr is not None else 0)
        return _call("voltrix_launch_spmm_panel_ticket_bf16" if bf16 else "voltrix_launch_spmm_panel_ticket_f16", *panel, *table,
                     partials_ptr, tickets, plan.num_nodes, embedding_dim, input_ptr, input_rows, output_ptr, tile[0], tile[1],
                     plan.waves, plan.row_blocks, tile[2], slab_policy, out_scale, stream)
    launch = (plan.num_nodes, embedding_dim, input_ptr, input_rows, output_ptr, int(accumulate), tile[0], tile[1], plan.waves,
              plan.row_blocks, tile[2], slab_policy, out_scale, stream)
    parts = getattr(plan, "parts", None)
    if parts is not None:
        return _call("voltrix_launch_spmm_panel_parts_bf16" if bf16 else "voltrix_launch_spmm_panel_parts_f16", *panel,
                     parts.parts.data_ptr(), parts.num_parts, parts.xcd_ptr.data_ptr(), parts.max_parts_per_xcd, partials_ptr, *launch)
    xcd_ptr = getattr(plan, "xcd_ptr", None)
    return _call("voltrix_launch_spmm_panel_bf16" if bf16 else "voltrix_launch_spmm_panel_f16", *panel, _opt(plan.panel_order),
                 _opt(xcd_ptr), plan.max_panels_per_xcd if xcd_ptr is not None else 0, *launch)


def launch_combine_panel_partials(parts, partials_ptr, output_ptr, num_nodes, embedding_dim, panel_rows, accumulate,
                                  stream, tickets: int = 0) -> int:
    """``output (+)= `` the partial tiles of the cut panels, pieces in slot order (``parts`` = voltrix.hybrid.PanelParts).
    ``tickets``: the ticket join's buffer -- blocks nothing has written yet are stored, the others added to."""
    if tickets:
        return _call("voltrix_launch_combine_panel_partials_ticket", parts.cuts.data_ptr(), parts.num_cuts, partials_ptr,
                     output_ptr, num_nodes, embedding_dim, panel_rows, tickets, stream)
    return _call("voltrix_launch_combine_panel_partials", parts.cuts.data_ptr(), parts.num_cuts, partials_ptr, output_ptr, num_nodes,
                 embedding_dim, panel_rows, int(accumulate), stream)


@_timed("spmm_fused")
def launch_spmm_fused(plan, fused, input_ptr, output_ptr, embedding_dim, bf16, tile, out_scale, stream,
                      pace_blocks: int = 0) -> int:
    """The two-level product in one launch; ``plan`` = voltrix.hybrid.PanelPlan (8 waves x 4 row blocks), ``fused`` =
    voltrix.hybrid.FusedRecords (4 waves x 8 row blocks), ``tile`` = (fs, depth), ``pace_blocks`` = sync points per column
    sweep between the workgroups of an XCD (0: none).  Returns the return code."""
    xcd_ptr = getattr(plan, "xcd_ptr", None)
    return _call("voltrix_launch_spmm_fused_bf16" if bf16 else "voltrix_launch_spmm_fused_f16", plan.panel_ptr.data_ptr(),
                 plan.panel_cols.data_ptr(), plan.panel_bits.data_ptr(), _opt(plan.panel_order), _opt(xcd_ptr),
                 plan.max_panels_per_xcd if xcd_ptr is not None else 0, fused.wave_ptr.data_ptr(), fused.records.data_ptr(),
                 plan.num_nodes, embedding_dim, input_ptr, output_ptr, tile[0], tile[1], int(pace_blocks), out_scale, stream)


def fused_panel_geometry():
    """``(waves, row_blocks)`` of the one-launch kernel's 512-row panel, asked of the library (4 x 8 since round 4)."""
    waves, row_blocks = ctypes.c_int(0), ctypes.c_int(0)
    lib().voltrix_fused_panel_geometry(waves, row_blocks)
    assert waves.value * row_blocks.value * 16 == 512, (waves.value, row_blocks.value)
    return waves.value, row_blocks.value


def build_fused_records(blk_offsets, hspa_packed, hind, num_nodes: int, stream=None):
    """Stage records of the one-launch kernel through the library's two-phase builder (voltrix/fused_plan.hpp): returns
    ``(wave_ptr int32 [waves NP + 1], records uint32 [R + 1, 64], R)``.  One host sync."""
    import torch

    dev = blk_offsets.device
    stream = _stream_of(stream)
    num_waves = fused_panel_geometry()[0] * ((num_nodes + 511) // 512)
    workspace = torch.empty(max(16, int(lib().voltrix_fused_records_workspace_bytes(num_nodes))), dtype=torch.uint8, device=dev)
    wave_ptr = torch.empty(num_waves + 1, dtype=torch.int32, device=dev)
    _checked("voltrix_launch_fused_records_count", blk_offsets.data_ptr(), hspa_packed.data_ptr(), num_nodes, workspace.data_ptr(),
             wave_ptr.data_ptr(), stream)
    num_records = int(wave_ptr[-1])   # the sync
    assert 0 <= num_records <= 4 * (hspa_packed.numel() // 16 + 1), num_records   # at most one record per TC block
    records = torch.empty((num_records + 1, 64), dtype=torch.int32, device=dev).view(torch.uint32)
    _checked("voltrix_launch_fused_records_fill", blk_offsets.data_ptr(), hspa_packed.data_ptr(), hind.data_ptr(), num_nodes,
             wave_ptr.data_ptr(), num_records, records.data_ptr(), stream)
    return wave_ptr, records, num_records


def launch_panel_order(panel_ptr, num_panels: int, order_out, stream, group: int = 1, xcd_ptr=None) -> None:
    _checked("voltrix_launch_panel_order", panel_ptr.data_ptr(), num_panels, group, _opt(xcd_ptr), order_out.data_ptr(), stream)


def panel_plan_workspace_bytes(num_nodes: int, waves: int, row_blocks: int) -> int:
    return int(lib().voltrix_panel_plan_workspace_bytes(num_nodes, waves, row_blocks))


def launch_panel_plan_count(indptr, indices, num_nodes, num_cols, waves, row_blocks, tau, workspace, panel_ptr,
                            resid_indptr, status, stream) -> int:
    return _call("voltrix_launch_panel_plan_count", indptr.data_ptr(), indices.data_ptr(), num_nodes, num_cols, indices.numel(), waves,
                 row_blocks, tau, workspace.data_ptr(), panel_ptr.data_ptr(), resid_indptr.data_ptr(), status.data_ptr(), stream)


def launch_panel_plan_fill(indptr, indices, num_nodes, num_cols, waves, row_blocks, tau, workspace, panel_ptr,
                           resid_indptr, total_ksteps, resid_indices, panel_cols, panel_bits, stream) -> None:
    _checked("voltrix_launch_panel_plan_fill", indptr.data_ptr(), indices.data_ptr(), num_nodes, num_cols, indices.numel(), waves,
             row_blocks, tau, workspace.data_ptr(), panel_ptr.data_ptr(), resid_indptr.data_ptr(), total_ksteps,
             resid_indices.data_ptr(), panel_cols.data_ptr(), panel_bits.data_ptr(), stream)


@_timed("window_order")
def launch_window_order(blk_offsets, num_nodes, order_out, stream, chunk: int = 256) -> None:
    _checked("voltrix_launch_window_order", blk_offsets.data_ptr(), num_nodes, chunk, order_out.data_ptr(), stream)


@_timed("cast_f32_f16")
def launch_cast_f32_f16(src, dst, stream) -> None:
    _checked("voltrix_launch_cast_f32_f16", src.data_ptr(), dst.data_ptr(), src.numel(), stream)


@_timed("cast_f32_f16_scaled")
def launch_cast_f32_f16_scaled(src, dst, scale, stream) -> None:
    """dst = fp16(src * 2^-e), scale[0] = 2^e (``scale``: float32[2] device tensor); see include/voltrix_capi.h."""
    _checked("voltrix_launch_cast_f32_f16_scaled", src.data_ptr(), dst.data_ptr(), src.numel(), scale.data_ptr(), stream)


# ---- the CSR / attention launchers


@_timed("spmm_csr_rows")
def launch_spmm_csr_rows(indptr, indices, num_rows: int, feat, output, stream, xcd_ranges: int = 0, values=None) -> None:
    """``output = csr(ones) @ feat`` -- or ``csr(values) @ feat`` with ``values`` (device float32 [nnz], CSR order) -- with the CSR
    row-gather kernel (device int32 CSR; fp32 / fp16 / bf16 ``feat`` whose rows are a multiple of 16 bytes; fp32 ``output``
    [num_rows, F]); see include/voltrix_capi.h."""
    import torch

    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32 and indptr.numel() == num_rows + 1
    assert feat.dim() == 2 and feat.is_contiguous() and output.is_contiguous() and output.dtype == torch.float32
    assert output.shape == (num_rows, feat.shape[1])
    dtype = _dtype_code(feat.dtype)
    if values is None:
        _checked("voltrix_launch_spmm_csr_rows", indptr.data_ptr(), indices.data_ptr(), num_rows, feat.shape[1], feat.data_ptr(), dtype,
                 output.data_ptr(), int(xcd_ranges), stream)
        return
    assert values.dtype == torch.float32 and values.is_contiguous() and values.numel() == indices.numel() and values.is_cuda
    _checked("voltrix_launch_spmm_csr_rows_weighted", indptr.data_ptr(), indices.data_ptr(), values.data_ptr(), num_rows, feat.shape[1],
             feat.data_ptr(), dtype, output.data_ptr(), int(xcd_ranges), stream)


@_timed("sddmm_csr")
def launch_sddmm_csr(indptr, indices, num_rows: int, x, y, out, stream) -> None:
    """``out[e] = <x[row_e], y[indices[e]]>`` for every entry of a device int32 CSR (the sampled dense-dense product,
    voltrix/sddmm_kernels.hpp): ``x`` [num_rows, F], ``y`` [*, F], dtype pairs (fp32, fp16 / bf16 / fp32), (fp16, fp16), (bf16, bf16),
    F a multiple of 16 bytes of ``y``; ``out`` float32 [nnz] in CSR order; see include/voltrix_capi.h."""
    import torch

    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32 and indptr.numel() == num_rows + 1
    assert x.dim() == 2 and y.dim() == 2 and x.is_contiguous() and y.is_contiguous() and x.shape[0] == num_rows
    assert x.shape[1] == y.shape[1] and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == indices.numel()
    _checked("voltrix_launch_sddmm_csr", indptr.data_ptr(), indices.data_ptr(), num_rows, indices.numel(), x.shape[1], x.data_ptr(),
             _dtype_code(x.dtype), y.data_ptr(), _dtype_code(y.dtype), out.data_ptr(), stream)


def edge_softmax_workspace_bytes(num_rows: int, nnz: int) -> int:
    """Bytes of device workspace both edge softmax entry points need (a function of ``nnz`` alone; 0 for nnz == 0)."""
    return int(lib().voltrix_edge_softmax_workspace_bytes(num_rows, nnz))


@_timed("edge_softmax_csr")
def launch_edge_softmax_csr(indptr, num_rows: int, scores, scale: float, out, workspace, stream) -> None:
    """``out`` = softmax of ``scale * scores`` over every row of a device int32 CSR (voltrix/edge_softmax_kernels.hpp): ``scores`` and
    ``out`` float32 [nnz] in CSR order, ``workspace`` uint8 of ``edge_softmax_workspace_bytes`` bytes; see include/voltrix_capi.h."""
    import torch

    assert indptr.dtype == torch.int32 and indptr.numel() == num_rows + 1 and indptr.is_contiguous()
    assert scores.dtype == torch.float32 and out.dtype == torch.float32 and scores.is_contiguous() and out.is_contiguous()
    assert out.numel() == scores.numel() and workspace.numel() >= edge_softmax_workspace_bytes(num_rows, scores.numel())
    _checked("voltrix_launch_edge_softmax_csr", indptr.data_ptr(), num_rows, scores.numel(), scores.data_ptr(), float(scale),
             out.data_ptr(), workspace.data_ptr(), stream)


@_timed("edge_softmax_backward_csr")
def launch_edge_softmax_backward_csr(indptr, num_rows: int, alpha, grad_alpha, scale: float, grad_scores, workspace, stream) -> None:
    """``grad_scores = scale * alpha * (grad_alpha - rowsum(alpha * grad_alpha))`` (the edge softmax's backward), all float32 [nnz] in
    CSR order; the forward's workspace size; see include/voltrix_capi.h."""
    import torch

    assert indptr.dtype == torch.int32 and indptr.numel() == num_rows + 1 and indptr.is_contiguous()
    for t in (alpha, grad_alpha, grad_scores):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == alpha.numel()
    assert workspace.numel() >= edge_softmax_workspace_bytes(num_rows, alpha.numel())
    _checked("voltrix_launch_edge_softmax_backward_csr", indptr.data_ptr(), num_rows, alpha.numel(), alpha.data_ptr(),
             grad_alpha.data_ptr(), float(scale), grad_scores.data_ptr(), workspace.data_ptr(), stream)


# ---- multi-head forms (csrc/capi_heads.hip): node tensors [n, H, D], edge tensors [nnz, H] with the head index fastest


@_timed("sddmm_heads_csr")
def launch_sddmm_heads_csr(indptr, indices, num_rows: int, x, y, out, stream) -> None:
    """``out[e, h] = <x[row_e, h], y[indices[e], h]>`` for every entry of a device int32 CSR (voltrix/sddmm_heads_kernels.hpp): ``x``
    [num_rows, H, D], ``y`` [*, H, D], the dtype pairs of ``launch_sddmm_csr``, D a multiple of 16 bytes of ``y``; ``out`` float32
    [nnz, H]; see include/voltrix_capi.h."""
    import torch

    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32 and indptr.numel() == num_rows + 1
    assert x.dim() == 3 and y.dim() == 3 and x.is_contiguous() and y.is_contiguous() and x.shape[0] == num_rows
    assert x.shape[1:] == y.shape[1:] and out.dtype == torch.float32 and out.is_contiguous()
    assert out.shape == (indices.numel(), x.shape[1])
    _checked("voltrix_launch_sddmm_heads_csr", indptr.data_ptr(), indices.data_ptr(), num_rows, indices.numel(), x.shape[1], x.shape[2],
             x.data_ptr(), _dtype_code(x.dtype), y.data_ptr(), _dtype_code(y.dtype), out.data_ptr(), stream)


def edge_softmax_heads_workspace_bytes(num_rows: int, nnz: int, heads: int) -> int:
    """Bytes of device workspace both multi-head edge softmax entry points need (a function of ``nnz`` and ``heads`` alone; with
    ``heads == 1`` the single-head size)."""
    return int(lib().voltrix_edge_softmax_heads_workspace_bytes(num_rows, nnz, heads))


@_timed("edge_softmax_heads_csr")
def launch_edge_softmax_heads_csr(indptr, num_rows: int, scores, scale: float, out, workspace, stream) -> None:
    """``out[:, h]`` = softmax of ``scale * scores[:, h]`` over every row of a device int32 CSR, for every head
    (voltrix/edge_softmax_heads_kernels.hpp): ``scores`` and ``out`` float32 [nnz, H], ``workspace`` uint8 of
    ``edge_softmax_heads_workspace_bytes`` bytes; see include/voltrix_capi.h."""
    import torch

    assert indptr.dtype == torch.int32 and indptr.numel() == num_rows + 1 and indptr.is_contiguous()
    assert scores.dim() == 2 and scores.dtype == torch.float32 and out.dtype == torch.float32
    assert scores.is_contiguous() and out.is_contiguous() and out.shape == scores.shape
    nnz, heads = scores.shape
    assert workspace.numel() >= edge_softmax_heads_workspace_bytes(num_rows, nnz, heads)
    _checked("voltrix_launch_edge_softmax_heads_csr", indptr.data_ptr(), num_rows, nnz, heads, scores.data_ptr(), float(scale),
             out.data_ptr(), workspace.data_ptr(), stream)


@_timed("edge_softmax_heads_backward_csr")
def launch_edge_softmax_heads_backward_csr(indptr, num_rows: int, alpha, grad_alpha, scale: float, grad_scores, workspace, stream) -> None:
    """The multi-head edge softmax's backward, all float32 [nnz, H]; the forward's workspace size; see include/voltrix_capi.h."""
    import torch

    assert indptr.dtype == torch.int32 and indptr.numel() == num_rows + 1 and indptr.is_contiguous()
    for t in (alpha, grad_alpha, grad_scores):
        assert t.dim() == 2 and t.dtype == torch.float32 and t.is_contiguous() and t.shape == alpha.shape
    nnz, heads = alpha.shape
    assert workspace.numel() >= edge_softmax_heads_workspace_bytes(num_rows, nnz, heads)
    _checked("voltrix_launch_edge_softmax_heads_backward_csr", indptr.data_ptr(), num_rows, nnz, heads, alpha.data_ptr(),
             grad_alpha.data_ptr(), float(scale), grad_scores.data_ptr(), workspace.data_ptr(), stream)


@_timed("spmm_csr_heads")
def launch_spmm_csr_heads(indptr, indices, values, num_rows: int, feat, output, stream) -> None:
    """``output[r, h] = sum_{e in row r} values[e, h] * feat[indices[e], h]`` (voltrix/spmm_csr_heads_kernels.hpp): device int32 CSR,
    ``values`` float32 [nnz, H], fp32 / fp16 / bf16 ``feat`` [*, H, D] with D a multiple of 16 bytes, fp32 ``output`` [num_rows, H, D];
    see include/voltrix_capi.h."""
    import torch

    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32 and indptr.numel() == num_rows + 1
    assert feat.dim() == 3 and feat.is_contiguous() and output.is_contiguous() and output.dtype == torch.float32
    assert output.shape == (num_rows,) + tuple(feat.shape[1:])
    assert values.dtype == torch.float32 and values.is_contiguous() and values.shape == (indices.numel(), feat.shape[1])
    _checked("voltrix_launch_spmm_csr_heads", indptr.data_ptr(), indices.data_ptr(), values.data_ptr(), num_rows, feat.shape[1],
             feat.shape[2], feat.data_ptr(), _dtype_code(feat.dtype), output.data_ptr(), stream)


# ---- GAT edge scores (csrc/capi_gat_score.hip): node scalars [n, H], edge tensors [nnz, H] with the head index fastest


def gat_score_workspace_bytes(num_rows: int, nnz: int, heads: int = 1) -> int:
    """Bytes of device workspace ``launch_gat_score_rowsum_csr`` needs (a function of ``nnz`` and ``heads`` alone; 0 for nnz == 0)."""
    return int(lib().voltrix_gat_score_workspace_bytes(num_rows, nnz, heads))


@_timed("gat_score_csr")
def launch_gat_score_csr(indptr, indices, num_rows: int, el, er, slope: float, out, stream) -> None:
    """``out[e, h] = leaky_relu(el[row_e, h] + er[indices[e], h], slope)`` for every entry of a device int32 CSR
    (voltrix/gat_score_kernels.hpp): ``el`` float32 [num_rows, H], ``er`` float32 [*, H], ``out`` float32 [nnz, H]; see
    include/voltrix_capi.h."""
    import torch

    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32 and indptr.numel() == num_rows + 1
    assert indptr.is_contiguous() and indices.is_contiguous()
    for t in (el, er, out):
        assert t.dim() == 2 and t.dtype == torch.float32 and t.is_contiguous() and t.shape[1] == out.shape[1]
    assert el.shape[0] == num_rows and out.shape[0] == indices.numel()
    _checked("voltrix_launch_gat_score_csr", indptr.data_ptr(), indices.data_ptr(), num_rows, indices.numel(), out.shape[1],
             el.data_ptr(), er.data_ptr(), float(slope), out.data_ptr(), stream)


@_timed("gat_score_rowsum_csr")
def launch_gat_score_rowsum_csr(indptr, indices, order, num_rows: int, a, b, grad, slope: float, out, workspace, stream) -> None:
    """``out[r, h] = sum_{e in row r} gate(a[r, h] + b[indices[e], h]) grad[order[e] if order is not None else e, h]`` with ``gate(z) =
    1 if z > 0 else slope``: ``a`` float32 [num_rows, H], ``b`` float32 [*, H], ``grad`` float32 [nnz, H], ``order`` None or int32
    [nnz], ``out`` float32 [num_rows, H] (every element written), ``workspace`` uint8 of ``gat_score_workspace_bytes`` bytes; see
    include/voltrix_capi.h."""
    import torch

    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32 and indptr.numel() == num_rows + 1
    assert indptr.is_contiguous() and indices.is_contiguous()
    nnz, heads = grad.shape
    for t in (a, b, grad, out):
        assert t.dim() == 2 and t.dtype == torch.float32 and t.is_contiguous() and t.shape[1] == heads
    assert a.shape[0] == num_rows and out.shape[0] == num_rows and nnz == indices.numel()
    if order is not None:
        assert order.dtype == torch.int32 and order.is_contiguous() and order.numel() == nnz
    assert workspace.numel() >= gat_score_workspace_bytes(num_rows, nnz, heads)
    _checked("voltrix_launch_gat_score_rowsum_csr", indptr.data_ptr(), indices.data_ptr(), _opt(order), num_rows, nnz, heads,
             a.data_ptr(), b.data_ptr(), grad.data_ptr(), float(slope), out.data_ptr(), workspace.data_ptr(), stream)


# ---- GATv2 edge scores (csrc/capi_gatv2_score.hip): node tensors [n, H, D], a [H, D], edge tensors [nnz, H] with the head index fastest


@_timed("gatv2_score_csr")
def launch_gatv2_score_csr(indptr, indices, num_rows: int, xl, xr, a, slope: float, out, stream) -> None:
    """``out[e, h] = sum_d a[h, d] * leaky_relu(xl[row_e, h, d] + xr[indices[e], h, d], slope)`` for every entry of a device int32 CSR
    (voltrix/gatv2_score_kernels.hpp): ``xl`` [num_rows, H, D] and ``xr`` [*, H, D] of one type (fp32 / fp16 / bf16), D a multiple of
    16 bytes; ``a`` float32 [H, D]; ``out`` float32 [nnz, H]; see include/voltrix_capi.h."""
    import torch

    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32 and indptr.numel() == num_rows + 1
    assert indptr.is_contiguous() and indices.is_contiguous()
    assert xl.dim() == 3 and xr.dim() == 3 and xl.is_contiguous() and xr.is_contiguous() and xl.shape[0] == num_rows
    assert xl.shape[1:] == xr.shape[1:] and xl.dtype == xr.dtype
    assert a.dtype == torch.float32 and a.is_contiguous() and a.shape == xl.shape[1:]
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == (indices.numel(), xl.shape[1])
    _checked("voltrix_launch_gatv2_score_csr", indptr.data_ptr(), indices.data_ptr(), num_rows, indices.numel(), xl.shape[1], xl.shape[2],
             xl.data_ptr(), xr.data_ptr(), _dtype_code(xl.dtype), a.data_ptr(), float(slope), out.data_ptr(), stream)


@_timed("gatv2_rowsum_csr")
def launch_gatv2_rowsum_csr(indptr, indices, order, num_rows: int, p, q, grad, slope: float, out, stream) -> None:
    """``out[r, h, d] = sum_{e in row r} gate(p[r, h, d] + q[indices[e], h, d]) grad[order[e] if order is not None else e, h]`` with
    ``gate(z) = 1 if z > 0 else slope``: ``p`` [num_rows, H, D] and ``q`` [*, H, D] of one type, ``grad`` float32 [nnz, H], ``order``
    None or int32 [nnz], ``out`` float32 [num_rows, H, D] (every row written); see include/voltrix_capi.h."""
    import torch

    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32 and indptr.numel() == num_rows + 1
    assert indptr.is_contiguous() and indices.is_contiguous()
    assert p.dim() == 3 and q.dim() == 3 and p.is_contiguous() and q.is_contiguous() and p.shape[0] == num_rows
    assert p.shape[1:] == q.shape[1:] and p.dtype == q.dtype
    nnz, heads = grad.shape
    assert grad.dtype == torch.float32 and grad.is_contiguous() and nnz == indices.numel() and heads == p.shape[1]
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == p.shape
    if order is not None:
        assert order.dtype == torch.int32 and order.is_contiguous() and order.numel() == nnz
    _checked("voltrix_launch_gatv2_rowsum_csr", indptr.data_ptr(), indices.data_ptr(), _opt(order), num_rows, nnz, heads, p.shape[2],
             p.data_ptr(), q.data_ptr(), _dtype_code(p.dtype), grad.data_ptr(), float(slope), out.data_ptr(), stream)


# ---- edge softmax + aggregation in one launch (csrc/capi_attn_aggregate.hip): scores [nnz, H], feat [n, H, D], row statistics [n, H]


def _check_keep_mask(mask, nnz: int, heads: int) -> None:
    import torch

    assert mask.dtype == torch.int32 and mask.is_contiguous() and mask.is_cuda and mask.shape == (nnz, (heads + 31) // 32), \
        (mask.dtype, tuple(mask.shape), nnz, heads)


def launch_dropout_mask(nnz: int, heads: int, threshold: int, seed: int, offset: int, mask, stream) -> None:
    """``mask`` int32 [nnz, ceil(heads / 32)]: bit ``h & 31`` of word ``h >> 5`` of edge ``e`` set iff word ``h & 3`` of
    ``Philox4x32-10((e, h >> 2, offset lo, offset hi), (seed lo, seed hi))`` is ``>= threshold`` (voltrix/dropout_mask_kernels.hpp);
    see include/voltrix_capi.h."""
    _check_keep_mask(mask, nnz, heads)
    assert 0 <= threshold < 2 ** 32 and 0 <= seed < 2 ** 64 and 0 <= offset < 2 ** 64
    _checked("voltrix_launch_dropout_mask", nnz, heads, threshold, seed, offset, mask.data_ptr(), stream)


@_timed("attn_aggregate_csr")
def launch_attn_aggregate_csr(indptr, indices, scores, num_rows: int, feat, scale: float, out, m, l, stream, mask=None,
                              keep_scale: float = 1.0) -> None:
    """``out[r, h] = sum_{e in row r} softmax(scale * scores)[e, h] * feat[indices[e], h]`` with the row statistics ``m``, ``l``
    (voltrix/attn_aggregate_kernels.hpp): device int32 CSR, ``scores`` float32 [nnz, H], fp32 / fp16 / bf16 ``feat`` [*, H, D] with D a
    multiple of 16 bytes, fp32 ``out`` [num_rows, H, D], fp32 ``m`` and ``l`` [num_rows, H]; with ``mask`` (int32 [nnz, ceil(H / 32)] keep
    bits) the kept entries weigh ``alpha * keep_scale`` and the others nothing (``voltrix_launch_attn_aggregate_dropout_csr``); see
    include/voltrix_capi.h."""
    import torch

    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32 and indptr.numel() == num_rows + 1
    assert indptr.is_contiguous() and indices.is_contiguous()
    assert feat.dim() == 3 and feat.is_contiguous() and out.is_contiguous() and out.dtype == torch.float32
    heads = feat.shape[1]
    assert out.shape == (num_rows,) + tuple(feat.shape[1:])
    assert scores.dtype == torch.float32 and scores.is_contiguous() and scores.shape == (indices.numel(), heads)
    for t in (m, l):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == (num_rows, heads)
    args = (indptr.data_ptr(), indices.data_ptr(), scores.data_ptr(), num_rows, indices.numel(), heads, feat.shape[2], feat.data_ptr(),
            _dtype_code(feat.dtype), float(scale), out.data_ptr(), m.data_ptr(), l.data_ptr())
    if mask is not None:
        _check_keep_mask(mask, indices.numel(), heads)
        _checked("voltrix_launch_attn_aggregate_dropout_csr", *args, mask.data_ptr(), float(keep_scale), stream)
        return
    _checked("voltrix_launch_attn_aggregate_csr", *args, stream)


@_timed("attn_aggregate_grad_scores_csr")
def launch_attn_aggregate_grad_scores_csr(indptr, indices, num_rows: int, grad_out, feat, scores, m, l, delta, scale: float, out,
                                          stream, mask=None, keep_scale: float = 1.0) -> None:
    """``out[e, h] = scale * alpha[e, h] * (<grad_out[row_e, h], feat[indices[e], h]> - delta[row_e, h])`` with ``alpha`` recomputed from
    ``scores``, ``m``, ``l``: fp32 ``grad_out`` [num_rows, H, D], ``feat`` [*, H, D], fp32 ``scores`` and ``out`` [nnz, H], fp32 ``m``,
    ``l``, ``delta`` [num_rows, H]; with ``mask`` the dot product is times ``keep_scale`` for a kept entry and +0 for a dropped one; see
    include/voltrix_capi.h."""
    import torch

    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32 and indptr.numel() == num_rows + 1
    assert indptr.is_contiguous() and indices.is_contiguous()
    assert grad_out.dim() == 3 and feat.dim() == 3 and grad_out.is_contiguous() and feat.is_contiguous()
    assert grad_out.dtype == torch.float32 and grad_out.shape[0] == num_rows and grad_out.shape[1:] == feat.shape[1:]
    nnz, heads = indices.numel(), feat.shape[1]
    for t in (scores, out):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == (nnz, heads)
    for t in (m, l, delta):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == (num_rows, heads)
    args = (indptr.data_ptr(), indices.data_ptr(), num_rows, nnz, heads, feat.shape[2], grad_out.data_ptr(), feat.data_ptr(),
            _dtype_code(feat.dtype), scores.data_ptr(), m.data_ptr(), l.data_ptr(), delta.data_ptr(), float(scale), out.data_ptr())
    if mask is not None:
        _check_keep_mask(mask, nnz, heads)
        _checked("voltrix_launch_attn_aggregate_dropout_grad_scores_csr", *args, mask.data_ptr(), float(keep_scale), stream)
        return
    _checked("voltrix_launch_attn_aggregate_grad_scores_csr", *args, stream)


@_timed("attn_aggregate_grad_feat_csr")
def launch_attn_aggregate_grad_feat_csr(t_indptr, t_indices, order, num_cols: int, grad_out, scores, m, l, scale: float, out,
                                        stream, mask=None, keep_scale: float = 1.0) -> None:
    """``out[c, h] = sum_{e in row c of the transposed CSR} alpha[order[e], h] * grad_out[t_indices[e], h]`` with ``alpha`` recomputed
    from ``scores`` (CSR order), ``m``, ``l``: int32 ``order`` [nnz], fp32 / fp16 / bf16 ``grad_out`` [num_rows, H, D], fp32 ``out``
    [num_cols, H, D]; with ``mask`` (CSR order, read at ``order[e]``) the weight is ``alpha * keep_scale`` for a kept entry and a dropped
    one adds nothing; see include/voltrix_capi.h."""
    import torch

    assert t_indptr.dtype == torch.int32 and t_indices.dtype == torch.int32 and t_indptr.numel() == num_cols + 1
    assert t_indptr.is_contiguous() and t_indices.is_contiguous()
    nnz = t_indices.numel()
    assert order.dtype == torch.int32 and order.is_contiguous() and order.numel() == nnz
    assert grad_out.dim() == 3 and grad_out.is_contiguous() and out.is_contiguous() and out.dtype == torch.float32
    heads = grad_out.shape[1]
    assert out.shape == (num_cols,) + tuple(grad_out.shape[1:])
    assert scores.dtype == torch.float32 and scores.is_contiguous() and scores.shape == (nnz, heads)
    for t in (m, l):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == (grad_out.shape[0], heads)
    args = (t_indptr.data_ptr(), t_indices.data_ptr(), order.data_ptr(), num_cols, nnz, heads, grad_out.shape[2], grad_out.data_ptr(),
            _dtype_code(grad_out.dtype), scores.data_ptr(), m.data_ptr(), l.data_ptr(), float(scale), out.data_ptr())
    if mask is not None:
        _check_keep_mask(mask, nnz, heads)
        _checked("voltrix_launch_attn_aggregate_dropout_grad_feat_csr", *args, mask.data_ptr(), float(keep_scale), stream)
        return
    _checked("voltrix_launch_attn_aggregate_grad_feat_csr", *args, stream)


# ---- max / min / mean aggregation (csrc/capi_spmm_reduce.hip)

REDUCE_OPS = {"max": 0, "min": 1, "mean": 2}   # `op` of voltrix_launch_spmm_csr_reduce


def launch_spmm_csr_reduce(indptr, indices, num_rows: int, feat, op: str, output, arg, stream) -> None:
    """``output[r] = max | min | mean`` over the entries of row ``r`` of ``feat[indices[e]]`` (voltrix/spmm_csr_reduce_kernels.hpp): device
    int32 CSR, fp32 / fp16 / bf16 ``feat`` [*, F] whose rows are a multiple of 16 bytes, fp32 ``output`` [num_rows, F], ``arg`` int32
    [num_rows, F] (the CSR entry id of the winner; max / min) or None; see include/voltrix_capi.h."""
    import torch

    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32 and indptr.numel() == num_rows + 1
    assert indptr.is_contiguous() and indices.is_contiguous()
    assert feat.dim() == 2 and feat.is_contiguous() and output.is_contiguous() and output.dtype == torch.float32
    assert output.shape == (num_rows, feat.shape[1])
    assert arg is None or (arg.dtype == torch.int32 and arg.is_contiguous() and arg.shape == output.shape)
    _checked("voltrix_launch_spmm_csr_reduce", indptr.data_ptr(), indices.data_ptr(), num_rows, feat.shape[1], feat.data_ptr(),
             _dtype_code(feat.dtype), REDUCE_OPS[op], output.data_ptr(), _opt(arg), stream)


def launch_spmm_csr_reduce_backward(t_indptr, t_indices, t_order, num_cols: int, grad_out, arg, output, stream) -> None:
    """``output[c, f] = sum_{e in row c of the transposed CSR, arg[t_indices[e], f] == t_order[e]} grad_out[t_indices[e], f]``: int32
    ``t_order`` [nnz], fp32 ``grad_out`` and int32 ``arg`` [num_rows, F] with F a multiple of 4, fp32 ``output`` [num_cols, F]; see
    include/voltrix_capi.h."""
    import torch

    assert t_indptr.dtype == torch.int32 and t_indices.dtype == torch.int32 and t_indptr.numel() == num_cols + 1
    assert t_indptr.is_contiguous() and t_indices.is_contiguous()
    nnz = t_indices.numel()
    assert t_order.dtype == torch.int32 and t_order.is_contiguous() and t_order.numel() == nnz
    assert grad_out.dim() == 2 and grad_out.dtype == torch.float32 and grad_out.is_contiguous()
    assert arg.dtype == torch.int32 and arg.is_contiguous() and arg.shape == grad_out.shape
    assert output.dtype == torch.float32 and output.is_contiguous() and output.shape == (num_cols, grad_out.shape[1])
    _checked("voltrix_launch_spmm_csr_reduce_backward", t_indptr.data_ptr(), t_indices.data_ptr(), t_order.data_ptr(), num_cols, nnz,
             grad_out.shape[1], grad_out.data_ptr(), arg.data_ptr(), output.data_ptr(), stream)


# ---- aggregation with a feature vector per edge (csrc/capi_spmm_edge.hip).  The two entry points return their status code; the wrappers
# ---- are not bracketed by KernelTimer

EDGE_OPS = {"mul": 0, "add": 1, "add_relu": 2, "copy": 3, "gate": 4}   # `op` of voltrix_spmm_edge_csr; grad_efeat takes the first four


def launch_spmm_edge(indptr, indices, order, num_rows: int, feat, efeat, self_rows, op: str, output, stream, num_entries=None) -> None:
    """``output[r] = sum_{e in row r} m(feat[indices[e]], efeat[order[e] if order is given else e])`` (voltrix/spmm_edge_kernels.hpp):
    device int32 CSR, ``order`` int32 [nnz] or None, fp32 / fp16 / bf16 ``efeat`` [nnz, F] whose rows are a multiple of 16 bytes, ``feat``
    [*, F] of the same type or fp32 (None with ``"copy"``), ``self_rows`` [num_rows, F] of ``efeat``'s type with ``"gate"`` (else None),
    fp32 ``output`` [num_rows, F]; ``num_entries``: ``indices.numel()`` unless given (a pattern without entries, whose ``indices`` and
    ``efeat`` are stand-ins); see include/voltrix_capi.h."""
    import torch

    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32 and indptr.numel() == num_rows + 1
    assert indptr.is_contiguous() and indices.is_contiguous()
    num_entries = indices.numel() if num_entries is None else num_entries
    assert order is None or (order.dtype == torch.int32 and order.is_contiguous() and order.numel() == num_entries)
    assert efeat.dim() == 2 and efeat.is_contiguous() and output.is_contiguous() and output.dtype == torch.float32
    assert output.shape == (num_rows, efeat.shape[1])
    assert feat is None or (feat.dim() == 2 and feat.is_contiguous() and feat.shape[1] == efeat.shape[1])
    assert self_rows is None or (self_rows.is_contiguous() and self_rows.shape == output.shape and self_rows.dtype == efeat.dtype)
    check(lib().voltrix_spmm_edge_csr(indptr.data_ptr(), indices.data_ptr(), _opt(order), num_rows, num_entries, efeat.shape[1],
                                      _opt(feat), 0 if feat is None else _dtype_code(feat.dtype), efeat.data_ptr(),
                                      _dtype_code(efeat.dtype), _opt(self_rows), EDGE_OPS[op], output.data_ptr(), stream),
          "voltrix_spmm_edge_csr")


def launch_spmm_edge_grad_efeat(indptr, indices, num_rows: int, grad_out, feat, efeat, dtype, op: str, output, stream) -> None:
    """``output[e] = d m(feat[indices[e]], efeat[e]) / d efeat * grad_out[row_e]``: fp32 ``grad_out`` [num_rows, F], ``feat`` [*, F] and
    ``efeat`` [nnz, F] of ``dtype`` (None where the op does not read them: ``feat`` for add / copy, ``efeat`` for all but add_relu), fp32
    ``output`` [nnz, F]; see include/voltrix_capi.h."""
    import torch

    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32 and indptr.numel() == num_rows + 1
    assert indptr.is_contiguous() and indices.is_contiguous()
    assert grad_out.dim() == 2 and grad_out.dtype == torch.float32 and grad_out.is_contiguous() and grad_out.shape[0] == num_rows
    assert output.dtype == torch.float32 and output.is_contiguous() and output.shape == (indices.numel(), grad_out.shape[1])
    for t in (feat, efeat):
        assert t is None or (t.dim() == 2 and t.is_contiguous() and t.dtype == dtype and t.shape[1] == grad_out.shape[1])
    check(lib().voltrix_spmm_edge_grad_efeat_csr(indptr.data_ptr(), indices.data_ptr(), num_rows, indices.numel(), grad_out.shape[1],
                                                 grad_out.data_ptr(), _opt(feat), _opt(efeat), _dtype_code(dtype), EDGE_OPS[op],
                                                 output.data_ptr(), stream),
          "voltrix_spmm_edge_grad_efeat_csr")


# ---- relational aggregation over typed edges (csrc/capi_spmm_rel.hip).  The three entry points return their status code; the wrappers
# ---- are not bracketed by KernelTimer

REL_BASIS_TILE, REL_MAX_TYPES, REL_MAX_BASES = 8, 65536, 1024    # kRelBasisTile, kRelMaxTypes, kRelMaxBases of spmm_rel_kernels.hpp


def _rel_tables(etype, weight, coef, num_entries, num_bases):
    import torch

    assert etype.dtype == torch.int32 and etype.is_contiguous() and etype.numel() == num_entries
    assert weight is None or (weight.dtype == torch.float32 and weight.is_contiguous() and weight.numel() == num_entries)
    assert coef.dim() == 2 and coef.dtype == torch.float32 and coef.is_contiguous() and coef.shape[1] == (num_bases + 3) // 4 * 4


def launch_spmm_rel(indptr, indices, etype, weight, num_rows: int, feat, coef, num_bases: int, output, stream, num_entries=None) -> None:
    """``output[i, b] = sum_{e in row i} weight[e] * coef[etype[e], b] * feat[indices[e]]`` (voltrix/spmm_rel_kernels.hpp): device int32
    CSR and ``etype`` [nnz], fp32 ``weight`` [nnz] or None, fp32 / fp16 / bf16 ``feat`` [*, F] whose rows are a multiple of 16 bytes, fp32
    ``coef`` [R, B_pad] (``num_bases`` rounded up to 4), fp32 ``output`` [num_rows, num_bases, F]; ``num_entries``: ``indices.numel()``
    unless given (a pattern without entries, whose ``indices`` and ``etype`` are stand-ins); see include/voltrix_capi.h."""
    import torch

    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32 and indptr.numel() == num_rows + 1
    assert indptr.is_contiguous() and indices.is_contiguous()
    num_entries = indices.numel() if num_entries is None else num_entries
    if num_entries:
        _rel_tables(etype, weight, coef, num_entries, num_bases)
    assert feat.dim() == 2 and feat.is_contiguous() and output.is_contiguous() and output.dtype == torch.float32
    assert output.shape == (num_rows, num_bases, feat.shape[1])
    check(lib().voltrix_spmm_rel_csr(indptr.data_ptr(), indices.data_ptr(), etype.data_ptr(), _opt(weight), num_rows, num_entries,
                                     feat.shape[1], coef.shape[0], num_bases, feat.data_ptr(), _dtype_code(feat.dtype), coef.data_ptr(),
                                     output.data_ptr(), stream),
          "voltrix_spmm_rel_csr")


def launch_spmm_rel_contract(t_indptr, t_indices, order, etype, weight, num_cols: int, grad_out, coef, output, stream) -> None:
    """``output[c] = sum_{e in row c of the transposed CSR} sum_b weight[id] * coef[etype[id], b] * grad_out[t_indices[e], b]`` with
    ``id = order[e]`` (``order`` None: ``e``): fp32 ``grad_out`` [*, B, F] with F a multiple of 4, fp32 ``output`` [num_cols, F]; see
    include/voltrix_capi.h."""
    import torch

    assert t_indptr.dtype == torch.int32 and t_indices.dtype == torch.int32 and t_indptr.numel() == num_cols + 1
    assert t_indptr.is_contiguous() and t_indices.is_contiguous()
    nnz = t_indices.numel()
    assert order is None or (order.dtype == torch.int32 and order.is_contiguous() and order.numel() == nnz)
    assert grad_out.dim() == 3 and grad_out.dtype == torch.float32 and grad_out.is_contiguous()
    _rel_tables(etype, weight, coef, nnz, grad_out.shape[1])
    assert output.dtype == torch.float32 and output.is_contiguous() and output.shape == (num_cols, grad_out.shape[2])
    check(lib().voltrix_spmm_rel_contract_csr(t_indptr.data_ptr(), t_indices.data_ptr(), _opt(order), etype.data_ptr(), _opt(weight),
                                              num_cols, nnz, grad_out.shape[2], coef.shape[0], grad_out.shape[1], grad_out.data_ptr(),
                                              coef.data_ptr(), output.data_ptr(), stream),
          "voltrix_spmm_rel_contract_csr")


def launch_spmm_rel_dots(indptr, indices, weight, num_rows: int, grad_out, feat, output, stream) -> None:
    """``output[e, b] = weight[e] * <grad_out[row_e, b], feat[indices[e]]>``: fp32 ``grad_out`` [num_rows, B, F], ``feat`` [*, F] whose
    rows are a multiple of 16 bytes, fp32 ``output`` [nnz, B_pad], the padding written as 0; see include/voltrix_capi.h."""
    import torch

    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32 and indptr.numel() == num_rows + 1
    assert indptr.is_contiguous() and indices.is_contiguous()
    nnz = indices.numel()
    assert weight is None or (weight.dtype == torch.float32 and weight.is_contiguous() and weight.numel() == nnz)
    assert grad_out.dim() == 3 and grad_out.dtype == torch.float32 and grad_out.is_contiguous() and grad_out.shape[0] == num_rows
    assert feat.dim() == 2 and feat.is_contiguous() and feat.shape[1] == grad_out.shape[2]
    num_bases = grad_out.shape[1]
    assert output.dtype == torch.float32 and output.is_contiguous() and output.shape == (nnz, (num_bases + 3) // 4 * 4)
    check(lib().voltrix_spmm_rel_dots_csr(indptr.data_ptr(), indices.data_ptr(), _opt(weight), num_rows, nnz, feat.shape[1], num_bases,
                                          grad_out.data_ptr(), feat.data_ptr(), _dtype_code(feat.dtype), output.data_ptr(), stream),
          "voltrix_spmm_rel_dots_csr")


# ---- FP8 (e4m3fn) feature rows: the quantiser and the aggregation (csrc/capi_spmm_fp8.hip).  The two entry points return their status
# ---- code; the wrappers are not bracketed by KernelTimer


def launch_quantize_fp8_rows(feat, inv_scale, output, stream) -> None:
    """``output[i, f] = e4m3(clamp(feat[i, f] * inv_scale[f], -448, 448))`` (voltrix/spmm_fp8_kernels.hpp): fp32 / fp16 / bf16 ``feat``
    [n, F] with unit column stride and any row stride >= F, fp32 ``inv_scale`` [F16], ``output`` [n, F16] of ``torch.float8_e4m3fn``
    or uint8, F16 = F rounded up to 16, the padding written as 0x00; see include/voltrix_capi.h."""
    import torch

    assert feat.dim() == 2 and (feat.shape[1] <= 1 or feat.stride(1) == 1) and (feat.shape[0] <= 1 or feat.stride(0) >= feat.shape[1])
    width = (feat.shape[1] + 15) // 16 * 16
    assert inv_scale.dtype == torch.float32 and inv_scale.is_contiguous() and inv_scale.numel() == width
    assert output.element_size() == 1 and output.is_contiguous() and output.shape == (feat.shape[0], width)
    check(lib().voltrix_quantize_fp8_rows(feat.data_ptr(), _dtype_code(feat.dtype), feat.shape[0], feat.shape[1],
                                          feat.stride(0) if feat.shape[0] > 1 else max(feat.shape[1], 1), inv_scale.data_ptr(),
                                          output.data_ptr(), width, stream),
          "voltrix_quantize_fp8_rows")


def launch_spmm_fp8(indptr, indices, values, num_rows: int, data, scale, output, stream, xcd_ranges: int = 1, num_entries=None) -> None:
    """``output[i] = scale * sum_{e in row i} values[e] * dec(data[indices[e]])`` (voltrix/spmm_fp8_kernels.hpp): device int32 CSR, fp32
    ``values`` [nnz] or None, ``data`` [*, F16] of e4m3fn codes with F16 a multiple of 16, fp32 ``scale`` [F16], fp32 / fp16 / bf16
    ``output`` [num_rows, F16]; ``num_entries``: ``indices.numel()`` unless given (a pattern without entries, whose ``indices`` is a
    stand-in); see include/voltrix_capi.h."""
    import torch

    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32 and indptr.numel() == num_rows + 1
    assert indptr.is_contiguous() and indices.is_contiguous()
    num_entries = indices.numel() if num_entries is None else num_entries
    assert values is None or (values.dtype == torch.float32 and values.is_contiguous() and values.numel() == num_entries)
    assert data.dim() == 2 and data.element_size() == 1 and data.is_contiguous() and data.shape[1] % 16 == 0
    assert scale.dtype == torch.float32 and scale.is_contiguous() and scale.numel() == data.shape[1]
    assert output.is_contiguous() and output.shape == (num_rows, data.shape[1])
    check(lib().voltrix_spmm_fp8_csr(indptr.data_ptr(), indices.data_ptr(), _opt(values), num_rows, data.shape[1], data.data_ptr(),
                                     scale.data_ptr(), output.data_ptr(), _dtype_code(output.dtype), int(xcd_ranges), num_entries,
                                     stream),
          "voltrix_spmm_fp8_csr")


# ---- several aggregates from one gather (csrc/capi_spmm_multi.hip).  The two entry points return their status code; the wrappers are
# ---- not bracketed by KernelTimer

MULTI_AGGREGATES = ("sum", "mean", "max", "min", "var", "std")   # the order of the slot parameters of voltrix_spmm_multi_csr


def launch_spmm_multi(indptr, indices, num_rows: int, feat, slots, eps: float, output, argmax, argmin, stream, num_entries=None) -> None:
    """``output[r, slots[name]] = name over the entries of row r of feat[indices[e]]`` for every ``name`` of ``slots`` (a dict from
    ``MULTI_AGGREGATES`` to the slots ``0 .. A - 1``; voltrix/spmm_multi_kernels.hpp): device int32 CSR, fp32 / fp16 / bf16 ``feat``
    [*, F] whose rows are a multiple of 16 bytes, fp32 ``output`` [num_rows, A, F], ``argmax`` / ``argmin`` int32 [num_rows, F] or
    None; ``num_entries``: ``indices.numel()`` unless given (a pattern without entries, whose ``indices`` is a stand-in); see
    include/voltrix_capi.h."""
    import torch

    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32 and indptr.numel() == num_rows + 1
    assert indptr.is_contiguous() and indices.is_contiguous()
    assert feat.dim() == 2 and feat.is_contiguous() and output.is_contiguous() and output.dtype == torch.float32
    assert output.shape == (num_rows, len(slots), feat.shape[1])
    for arg in (argmax, argmin):
        assert arg is None or (arg.dtype == torch.int32 and arg.is_contiguous() and arg.shape == (num_rows, feat.shape[1]))
    num_entries = indices.numel() if num_entries is None else num_entries
    check(lib().voltrix_spmm_multi_csr(indptr.data_ptr(), indices.data_ptr(), num_rows, num_entries, feat.shape[1], feat.data_ptr(),
                                       _dtype_code(feat.dtype), *[slots.get(name, -1) for name in MULTI_AGGREGATES], len(slots),
                                       float(eps), output.data_ptr(), _opt(argmax), _opt(argmin), stream),
          "voltrix_spmm_multi_csr")


def launch_spmm_multi_backward(t_indptr, t_indices, t_order, num_cols: int, x, u, w, mean, g_max, argmax, g_min, argmin, output,
                               stream) -> None:
    """``output[c] = sum_{e in row c of the transposed CSR} u[r] + w[r] (x[c] - mean[r]) + [argmax[r] == t_order[e]] g_max[r] +
    [argmin[r] == t_order[e]] g_min[r]`` with ``r = t_indices[e]``: fp32 operands (int32 args) [*, F] with F a multiple of 4, each
    group -- ``u``; ``w`` with ``x`` and ``mean``; ``g_max`` with ``argmax``; ``g_min`` with ``argmin`` -- given or None; ``mean`` may
    be a column slice of a wider array (rows of ``mean.stride(0)`` floats); fp32 ``output`` [num_cols, F]; see include/voltrix_capi.h."""
    import torch

    assert t_indptr.dtype == torch.int32 and t_indices.dtype == torch.int32 and t_indptr.numel() == num_cols + 1
    assert t_indptr.is_contiguous() and t_indices.is_contiguous()
    nnz = t_indices.numel()
    assert t_order.dtype == torch.int32 and t_order.is_contiguous() and t_order.numel() == nnz
    assert output.dtype == torch.float32 and output.is_contiguous() and output.dim() == 2 and output.shape[0] == num_cols
    dim = output.shape[1]
    for t in (x, u, w, g_max, g_min):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == dim)
    for t in (argmax, argmin):
        assert t is None or (t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == dim)
    assert x is None or x.shape[0] == num_cols
    mean_ld = 0
    if mean is not None:
        assert mean.dtype == torch.float32 and mean.dim() == 2 and mean.shape[1] == dim and (mean.stride(1) == 1 or dim == 1)
        mean_ld = mean.stride(0) if mean.shape[0] > 1 else dim
    check(lib().voltrix_spmm_multi_backward_csr(t_indptr.data_ptr(), t_indices.data_ptr(), t_order.data_ptr(), num_cols, nnz, dim,
                                                _opt(x), _opt(u), _opt(w), _opt(mean), mean_ld, _opt(g_max), _opt(argmax), _opt(g_min),
                                                _opt(argmin), output.data_ptr(), stream),
          "voltrix_spmm_multi_backward_csr")


SAMPLE_ALL, SAMPLE_MAX_FANOUT = -1, 64     # `fanout` of voltrix_launch_sample_neighbors: every entry of every row; the largest fan-out


def launch_sample_neighbors(indptr, indices, num_rows: int, seeds, s_indptr, num_sampled: int, fanout: int, replace: bool, seed: int,
                            offset: int, s_indices, s_entries, stream, exclude=None) -> None:
    """At most ``fanout`` entries of every seed row of a device int32 CSR by the sampling rule of voltrix/neighbor_sample_kernels.hpp:
    ``s_indices`` / ``s_entries`` int32 [num_sampled] get the global column ids and the CSR entry ids, in the segments ``s_indptr``
    (int32 [S + 1], the prefix sum of the rule's per-seed counts) gives.  ``exclude``: ``None``, or device int32 CSR entry ids,
    strictly ascending, that no row returns (``s_indptr`` counts with ``d'`` then; the call goes through
    ``voltrix_launch_sample_neighbors_excluding``, the same launch with a list); see include/voltrix_capi.h."""
    import torch

    for t in (indptr, indices, seeds, s_indptr, s_indices, s_entries) + (() if exclude is None else (exclude,)):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda
    assert indptr.numel() == num_rows + 1 and s_indptr.numel() == seeds.numel() + 1
    assert s_indices.numel() == num_sampled == s_entries.numel()
    head = (indptr.data_ptr(), indices.data_ptr(), num_rows, seeds.data_ptr(), seeds.numel(), s_indptr.data_ptr(), num_sampled,
            int(fanout), int(bool(replace)), int(seed), int(offset))
    tail = (s_indices.data_ptr(), s_entries.data_ptr(), stream)
    if exclude is None:
        _checked("voltrix_launch_sample_neighbors", *head, *tail)
    else:
        _checked("voltrix_launch_sample_neighbors_excluding", *head, exclude.data_ptr() if exclude.numel() else None, exclude.numel(),
                 *tail)


def sample_neighbors_weighted(indptr, indices, cum, num_rows: int, seeds, s_indptr, num_sampled: int, fanout: int, replace: bool,
                              seed: int, offset: int, s_indices, s_entries, stream) -> None:
    """At most ``fanout`` entries of every seed row of a device int32 CSR, drawn by weight: the rule of
    voltrix/weighted_sample_kernels.hpp on ``cum``, device int64 [nnz], the inclusive prefix sum of the quantised weights
    (``voltrix.sampling_weights``).  ``s_indptr`` is the prefix sum of the rule's per-seed counts (with the rows' positive entries in
    place of their degrees); the other arguments are ``launch_sample_neighbors``'; see include/voltrix_capi.h."""
    import torch

    for t in (indptr, indices, seeds, s_indptr, s_indices, s_entries):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda
    assert cum.dtype == torch.int64 and cum.is_contiguous() and cum.is_cuda and cum.numel() == indices.numel()
    assert indptr.numel() == num_rows + 1 and s_indptr.numel() == seeds.numel() + 1
    assert s_indices.numel() == num_sampled == s_entries.numel()
    _checked("voltrix_sample_neighbors_weighted", indptr.data_ptr(), indices.data_ptr(), cum.data_ptr(), num_rows, seeds.data_ptr(),
             seeds.numel(), s_indptr.data_ptr(), num_sampled, int(fanout), int(bool(replace)), int(seed), int(offset),
             s_indices.data_ptr(), s_entries.data_ptr(), stream)


def launch_block_mark(cols, num_cols: int, table, stream) -> None:
    """``table[cols[e]] = 1`` (device int32; ``table`` [num_cols] zero on entry); see include/voltrix_capi.h."""
    import torch

    assert cols.dtype == torch.int32 and cols.is_contiguous() and table.dtype == torch.int32 and table.is_contiguous()
    assert table.numel() == num_cols and cols.is_cuda and table.is_cuda
    _checked("voltrix_launch_block_mark", cols.data_ptr(), cols.numel(), num_cols, table.data_ptr(), stream)


def launch_block_mark_seeds(seeds, num_cols: int, table, stream) -> None:
    """``table[seeds[i]] = -(i + 1)``, after ``launch_block_mark`` on the same stream; see include/voltrix_capi.h."""
    import torch

    assert seeds.dtype == torch.int32 and seeds.is_contiguous() and table.dtype == torch.int32 and table.is_contiguous()
    assert table.numel() == num_cols and seeds.is_cuda and table.is_cuda
    _checked("voltrix_launch_block_mark_seeds", seeds.data_ptr(), seeds.numel(), num_cols, table.data_ptr(), stream)


def launch_block_relabel(cols, seeds, table, rank, num_cols: int, local, src_ids, stream) -> None:
    """``local[e]`` = the position of ``cols[e]`` in ``src_ids`` (the seeds, then the other marked columns ascending) and ``src_ids``
    itself, from the marked ``table`` and ``rank``, the inclusive count of its positive entries; see include/voltrix_capi.h."""
    import torch

    for t in (cols, seeds, table, rank, local, src_ids):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda
    assert table.numel() == num_cols == rank.numel() and local.numel() == cols.numel() and src_ids.numel() >= seeds.numel()
    _checked("voltrix_launch_block_relabel", cols.data_ptr(), cols.numel(), seeds.data_ptr(), seeds.numel(), table.data_ptr(),
             rank.data_ptr(), num_cols, src_ids.numel(), local.data_ptr(), src_ids.data_ptr(), stream)


SUBGRAPH_GROUPS, WALK_MAX_LENGTH = (4, 8, 16, 32, 64), 2 ** 20      # the lane-group widths of the subgraph kernels; the longest walk


def launch_subgraph_count(indptr, indices, num_rows: int, rows, table, group: int, counts, stream) -> None:
    """``counts[i]`` = the number of entries of row ``rows[i]`` whose column ``table`` marks (``table[cols[j]] = -(j + 1)``), walked by
    lane groups of ``group`` lanes; see include/voltrix_capi.h."""
    import torch

    for t in (indptr, indices, rows, table, counts):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda
    assert indptr.numel() == num_rows + 1 and counts.numel() == rows.numel()
    _checked("voltrix_launch_subgraph_count", indptr.data_ptr(), indices.data_ptr(), num_rows, rows.data_ptr(), rows.numel(),
             table.data_ptr(), table.numel(), int(group), counts.data_ptr(), stream)


def launch_subgraph_fill(indptr, indices, num_rows: int, rows, table, group: int, s_indptr, s_local, s_entries, stream) -> None:
    """The kept entries of every row ``rows[i]`` into its segment of ``s_indptr`` (the prefix sum of ``launch_subgraph_count``'s
    counts): ``s_local`` the position of the column in ``cols``, ``s_entries`` the CSR entry id; see include/voltrix_capi.h."""
    import torch

    for t in (indptr, indices, rows, table, s_indptr, s_local, s_entries):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda
    assert indptr.numel() == num_rows + 1 and s_indptr.numel() == rows.numel() + 1 and s_local.numel() == s_entries.numel()
    _checked("voltrix_launch_subgraph_fill", indptr.data_ptr(), indices.data_ptr(), num_rows, rows.data_ptr(), rows.numel(),
             table.data_ptr(), table.numel(), int(group), s_indptr.data_ptr(), s_local.numel(), s_local.data_ptr(),
             s_entries.data_ptr(), stream)


def launch_random_walk(indptr, indices, num_rows: int, starts, length: int, seed: int, offset: int, nodes, entries, stream,
                       step_major: bool = False) -> None:
    """``starts.numel()`` random walks of ``length`` steps by the walk rule of voltrix/induced_subgraph_kernels.hpp into ``nodes``
    ``[W, length + 1]`` and ``entries`` ``[W, length]`` (``step_major``: ``[length + 1, W]`` and ``[length, W]``); see
    include/voltrix_capi.h."""
    import torch

    for t in (indptr, indices, starts, nodes, entries):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda
    count = starts.numel()
    assert indptr.numel() == num_rows + 1 and nodes.numel() == count * (length + 1) and entries.numel() == count * length
    _checked("voltrix_launch_random_walk", indptr.data_ptr(), indices.data_ptr(), num_rows, starts.data_ptr(), count, int(length),
             int(seed), int(offset), nodes.data_ptr(), entries.data_ptr(), int(bool(step_major)), stream)


NEGATIVE_MAX_SLOTS, NEGATIVE_MAX_TRIES = 1024, 256      # `k` and `max_tries` of voltrix_launch_negative_sample


def launch_negative_sample(indptr, indices, num_rows: int, num_cols: int, src, k: int, max_tries: int, exclude_self: bool,
                           assume_sorted: bool, seed: int, offset: int, neg, stream) -> None:
    """``neg`` int32 ``[S, k]``: for every position of ``src``, ``k`` columns that do not occur in its row, by the negative rule of
    voltrix/negative_sample_kernels.hpp (``-1`` where ``max_tries`` tries were all rejected); see include/voltrix_capi.h."""
    import torch

    for t in (indptr, indices, src, neg):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda
    assert indptr.numel() == num_rows + 1 and neg.numel() == src.numel() * k
    _checked("voltrix_launch_negative_sample", indptr.data_ptr(), indices.data_ptr(), num_rows, int(num_cols), indices.numel(),
             src.data_ptr(), src.numel(), int(k), int(max_tries), int(bool(exclude_self)), int(bool(assume_sorted)), int(seed),
             int(offset), neg.data_ptr(), stream)


def launch_edge_endpoints(indptr, indices, num_rows: int, entries, rows, cols, stream) -> None:
    """``rows[i]`` / ``cols[i]``: the row that holds CSR entry ``entries[i]`` (a search in ``indptr``) and its column; ``-1, -1`` for an
    id outside ``[0, nnz)``; see include/voltrix_capi.h."""
    import torch

    for t in (indptr, indices, entries, rows, cols):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda
    assert indptr.numel() == num_rows + 1 and rows.numel() == entries.numel() == cols.numel()
    _checked("voltrix_launch_edge_endpoints", indptr.data_ptr(), indices.data_ptr(), num_rows, indices.numel(), entries.data_ptr(),
             entries.numel(), rows.data_ptr(), cols.data_ptr(), stream)


def launch_find_edges(indptr, indices, num_rows: int, rows, cols, assume_sorted: bool, out, stream) -> None:
    """``out[i]``: the id of the first entry of row ``rows[i]`` whose column is ``cols[i]``, ``-1`` if there is none or the row is outside
    ``[0, num_rows)`` (a lower bound with ``assume_sorted``, a scan without); see include/voltrix_capi.h."""
    import torch

    for t in (indptr, indices, rows, cols, out):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda
    assert indptr.numel() == num_rows + 1 and rows.numel() == cols.numel() == out.numel()
    _checked("voltrix_launch_find_edges", indptr.data_ptr(), indices.data_ptr(), num_rows, indices.numel(), rows.data_ptr(),
             cols.data_ptr(), rows.numel(), int(bool(assume_sorted)), out.data_ptr(), stream)


def launch_scatter_values(values, slots, plane, stream) -> None:
    """``plane.view(-1)[slots[e]] = values[e]`` (device float32 values, int64 slots, fp32 / fp16 / bf16 plane); see
    include/voltrix_capi.h."""
    import torch

    assert values.dtype == torch.float32 and slots.dtype == torch.int64 and values.numel() == slots.numel()
    assert values.is_contiguous() and slots.is_contiguous() and plane.is_contiguous() and values.is_cuda and plane.is_cuda
    _checked("voltrix_launch_scatter_values", values.data_ptr(), slots.data_ptr(), plane.data_ptr(), values.numel(),
             _dtype_code(plane.dtype), stream)


@_timed("scale_rows")
def launch_scale_rows(src, scale, dst, stream) -> None:
    """dst[i, :] = src[i, :] * scale[i] (``scale`` float32 [rows]; fp32 / fp16 / bf16 rows of a 16-byte multiple; in place
    allowed); see include/voltrix_capi.h."""
    import torch

    assert src.dim() == 2 and src.is_contiguous() and dst.is_contiguous() and dst.shape == src.shape and dst.dtype == src.dtype
    assert scale.dtype == torch.float32 and scale.numel() == src.shape[0] and scale.is_contiguous()
    _checked("voltrix_launch_scale_rows", src.data_ptr(), scale.data_ptr(), dst.data_ptr(), src.shape[0], src.shape[1],
             _dtype_code(src.dtype), stream)


# ---------------------------------------------------------------------------------------------------------------------
# Cuthill-McKee row order on the device (voltrix/reorder_kernels.hpp; include/voltrix_capi.h)
def csr_transpose(indptr, indices, num_rows: int, num_cols: int, stream=None):
    """CSR of ``A^T``: int32 ``(t_indptr [num_cols + 1], t_indices [nnz])``, rows sorted, duplicates kept (a stable radix
    sort by column, voltrix/reorder_kernels.hpp).  No host sync."""
    import torch

    dev = indptr.device
    stream = _stream_of(stream)
    nnz = int(indices.numel())
    ws = torch.empty(max(16, int(lib().voltrix_csr_transpose_workspace_bytes(nnz))), dtype=torch.uint8, device=dev)
    t_indptr = torch.empty(num_cols + 1, dtype=torch.int32, device=dev)
    t_indices = torch.empty(nnz, dtype=torch.int32, device=dev)
    _checked("voltrix_launch_csr_transpose", indptr.data_ptr(), indices.data_ptr(), num_rows, num_cols, nnz, ws.data_ptr(),
             t_indptr.data_ptr(), t_indices.data_ptr(), stream)
    return t_indptr, t_indices


def chol_inv_transposed(gram, eps: float = 1e-10, stream=None):
    """``inv(chol(gram + eps trace I))^T`` of a k x k float32 Gram matrix on its device (k <= 64); no host sync."""
    import torch

    k = gram.shape[0]
    assert gram.is_cuda and gram.dtype == torch.float32 and gram.shape == (k, k) and gram.is_contiguous()
    out = torch.empty_like(gram)
    _checked("voltrix_launch_chol_inv_transposed", gram.data_ptr(), k, eps, out.data_ptr(), _stream_of(stream))
    return out


class CmSearch:
    """State of the Cuthill-McKee search of one graph: buffers the C-ABI entries work on (all int32, on the CSR's device)."""

    def __init__(self, indptr, indices, t_indptr, t_indices, num_nodes: int, t_rows: int, tie):
        import torch

        dev = indptr.device
        self.graph = (indptr, indices, t_indptr, t_indices)
        self.n, self.t_rows, self.tie = num_nodes, t_rows, tie
        self.level = torch.full((num_nodes,), -1, dtype=torch.int32, device=dev)
        self.rank = torch.full((num_nodes,), -1, dtype=torch.int32, device=dev)
        self.queue = torch.empty(num_nodes, dtype=torch.int32, device=dev)
        self.level_off = torch.zeros(num_nodes + 2, dtype=torch.int32, device=dev)
        self.ctrl = torch.zeros(8, dtype=torch.int32, device=dev)
        self.syncs = 0

    def _graph_args(self):
        return (*(t.data_ptr() for t in self.graph), self.n, self.t_rows)

    def levels(self, start: int, wide_levels: int = 4, stream=None):
        """Breadth-first levels of ``start``'s component: returns ``(nodes, levels)``; ``queue[:nodes]`` holds the component
        level by level, ``level_off[:levels + 1]`` the offsets.  One host read per `wide_levels` whole-chip levels (a graph
        whose frontiers stay narrow is walked by one launch)."""
        stream = _stream_of(stream)
        state = (self.level.data_ptr(), self.queue.data_ptr(), self.ctrl.data_ptr(), self.level_off.data_ptr())
        _checked("voltrix_launch_bfs_seed", int(start), self.n, *state, stream)
        while True:
            _checked("voltrix_launch_bfs_levels", *self._graph_args(), *state, wide_levels, stream)
            ctrl = self.ctrl.tolist()       # the sync
            self.syncs += 1
            if ctrl[4]:
                return ctrl[1], ctrl[3] + 1

    def rank_component(self, levels: int, base: int, stream=None):
        """Cuthill-McKee order inside the levels of the component in ``queue`` (in place) and ``rank`` = base + position."""
        import torch

        stream = _stream_of(stream)
        offsets = self.level_off[:levels + 1].cpu()          # the sync
        self.syncs += 1
        sizes = (offsets[1:] - offsets[:-1])
        big = int(sizes[sizes > 1024].max()) if bool((sizes > 1024).any()) else 0
        ws = torch.empty(max(16, int(lib().voltrix_cm_rank_workspace_bytes(big))), dtype=torch.uint8, device=self.level.device)
        host = (ctypes.c_int * (levels + 1))(*offsets.tolist())
        _checked("voltrix_launch_cm_rank", *self._graph_args(), self.level.data_ptr(), self.rank.data_ptr(), self.tie.data_ptr(),
                 self.queue.data_ptr(), self.level_off.data_ptr(), host, levels, int(base), ws.data_ptr(), stream)
        return offsets
