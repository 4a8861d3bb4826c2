"""CPU: the C-ABI library loads and exports every symbol include/voltrix_capi.h declares; host-only entry points
(tile enumeration, the host `preprocess` launch, argument validation) behave.  No GPU compute is called here."""
import ctypes
import inspect

import numpy as np
import pytest

from capi_header import prototypes
from conftest import load_csr_fixture

from voltrix import capi


def _declared_functions():
    return sorted(prototypes())


def test_header_and_binding_agree_in_every_type():
    """Every prototype of the header -- its name, its return type and each parameter's type -- is the binding's entry, and is what the
    loaded library's functions are set to: a wrong width or a missing argument is refused by ctypes, not passed on."""
    declared = prototypes()
    assert set(declared) == set(capi.SYMBOLS) == set(capi.SIGNATURES) and len(capi.SYMBOLS) == len(declared)
    lib = capi.lib()
    for name, (restype, params) in declared.items():
        argtypes = [ctype for ctype, _ in params]
        assert capi.SIGNATURES[name] == (restype, argtypes), name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_library_exports_every_declared_symbol():
    lib = capi.lib()
    for name in _declared_functions():
        assert hasattr(lib, name), f"libvoltrix_hip.so does not export {name}"
    assert lib.voltrix_abi_version() == 2
    from voltrix import hybrid
    assert capi.fused_panel_geometry() == (hybrid.FUSED_WAVES, hybrid.FUSED_ROW_BLOCKS) == (4, 8)


def test_every_size_function_returns_64_bits():
    """The ``*_workspace_bytes`` functions return ``int64_t``; a binding left at ctypes' default ``int`` cuts the size of a large graph's
    workspace short, and the launch then writes past the buffer allocated from it.  Three were (stream table, its fill phase, panel parts)."""
    lib = capi.lib()
    sizes = [name for name in _declared_functions() if name.endswith("_workspace_bytes")]
    assert len(sizes) >= 12
    for name in sizes:
        assert getattr(lib, name).restype is ctypes.c_int64, name
    units = 1 << 30
    assert lib.voltrix_stream_table_fill_workspace_bytes(ctypes.c_int64(units)) >= 4 * 4 * units
    assert lib.voltrix_unit_table_fill_workspace_bytes(ctypes.c_int64(units)) >= 5 * 4 * units
    assert lib.voltrix_stream_table_fill_workspace_bytes(units) >= 4 * 4 * units      # a plain int goes through argtypes whole
    assert lib.voltrix_unit_table_fill_workspace_bytes(units) >= 5 * 4 * units
    assert lib.voltrix_unit_table_fill_workspace_bytes(1 << 32) > 1 << 32


def test_a_wrong_width_or_a_missing_argument_is_refused():
    """Host code only: ctypes refuses the call before the library is entered."""
    lib = capi.lib()
    assert lib.voltrix_edge_softmax_workspace_bytes(ctypes.c_int(4), ctypes.c_int64(5)) >= 0
    with pytest.raises((ctypes.ArgumentError, TypeError)):
        lib.voltrix_edge_softmax_workspace_bytes(ctypes.c_int(4), ctypes.c_int(5))      # nnz is int64_t
    with pytest.raises((ctypes.ArgumentError, TypeError)):
        lib.voltrix_edge_softmax_workspace_bytes(4)
    rc = ctypes.c_int(-1)
    with pytest.raises((ctypes.ArgumentError, TypeError)):
        lib.voltrix_launch_cast_f32_f16(None, None, 16, rc)                             # no stream
    with pytest.raises((ctypes.ArgumentError, TypeError)):
        lib.voltrix_launch_cast_f32_f16(None, None, 16.0, None, rc)                     # a float where count is int64_t
    assert rc.value == -1


# the wrappers KernelTimer brackets and the label each is counted under (KernelTimer.summary() keys; bench.py reads them)
TIMED = {
    "launch_spmm": "spmm",
    "launch_spmm_sched": "spmm",
    "launch_spmm_panel": "spmm_panel",
    "launch_spmm_fused": "spmm_fused",
    "launch_combine_partials": "combine_partials",
    "launch_cast_f32_f16_scaled": "cast_f32_f16_scaled",
    "launch_cast_f32_f16": "cast_f32_f16",
    "launch_scale_rows": "scale_rows",
    "launch_spmm_csr_rows": "spmm_csr_rows",
    "launch_sddmm_csr": "sddmm_csr",
    "launch_edge_softmax_csr": "edge_softmax_csr",
    "launch_edge_softmax_backward_csr": "edge_softmax_backward_csr",
    "launch_sddmm_heads_csr": "sddmm_heads_csr",
    "launch_edge_softmax_heads_csr": "edge_softmax_heads_csr",
    "launch_edge_softmax_heads_backward_csr": "edge_softmax_heads_backward_csr",
    "launch_spmm_csr_heads": "spmm_csr_heads",
    "launch_gat_score_csr": "gat_score_csr",
    "launch_gat_score_rowsum_csr": "gat_score_rowsum_csr",
    "launch_gatv2_score_csr": "gatv2_score_csr",
    "launch_gatv2_rowsum_csr": "gatv2_rowsum_csr",
    "launch_attn_aggregate_csr": "attn_aggregate_csr",
    "launch_attn_aggregate_grad_scores_csr": "attn_aggregate_grad_scores_csr",
    "launch_attn_aggregate_grad_feat_csr": "attn_aggregate_grad_feat_csr",
    "launch_spmm_f32_as_f16": "spmm_f32_as_f16",
    "launch_window_order": "window_order",
    "launch_csr_window_count": "csr_window_count",
    "launch_csr_fill": "csr_fill",
}


def test_the_timed_wrappers_their_labels_and_their_stream_positions():
    timed = {name: fn for name, fn in vars(capi).items() if hasattr(fn, "timer_label")}
    assert {name: fn.timer_label for name, fn in timed.items()} == TIMED and len(TIMED) == 27
    for name, fn in timed.items():
        assert fn.__name__ == name
        for signature in (inspect.signature(fn), inspect.signature(fn.__wrapped__)):   # the public signature is the wrapped function's
            assert list(signature.parameters).index("stream") == fn.stream_index, name
    # the position counted by hand before the table existed, for three shapes of signature
    assert capi.launch_spmm.stream_index == 10 and capi.launch_cast_f32_f16.stream_index == 2
    assert capi.launch_attn_aggregate_grad_scores_csr.stream_index == 11


def test_a_timed_wrapper_brackets_its_own_stream_under_its_label(monkeypatch):
    from contextlib import contextmanager

    from voltrix.utils import KernelTimer

    seen = []

    class Recorder:
        @contextmanager
        def bracket(self, label, stream):
            seen.append((label, stream))
            yield

    monkeypatch.setattr(KernelTimer, "active", Recorder())
    z = np.zeros(64, np.uint8).ctypes.data
    assert capi.launch_spmm(z, z, z, 16, 0, 12, z, z, True, (128, 4, 1), 1234) == 1          # refused on the host: no HIP call
    assert capi.launch_spmm(z, z, z, 16, 0, 12, z, z, True, (128, 4, 1), stream=5678) == 1
    assert seen == [("spmm", 1234), ("spmm", 5678)]


def test_tile_space_enumeration_and_defaults():
    f16 = capi.tiles(True)
    f32 = capi.tiles(False)
    assert len(f16) == len(set(f16)) >= 30 and (128, 4, 1) in f16 and (256, 4, 4) not in f16
    assert (128, 2, 1) in f32 and all(fs <= 128 for fs, _, _ in f32)
    for fs, depth, waves in f16 + f32:
        assert fs in (32, 64, 128, 256) and 2 <= depth <= 4 and waves in (1, 2, 4, 8)
    for f16_flag, tiles in ((True, f16), (False, f32)):
        for dim in (8, 32, 33, 64, 100, 128, 512, 1024):
            assert capi.default_tile(dim, f16_flag) in tiles
    assert capi.default_tile(32, True) == (32, 4, 4) and capi.default_tile(64, True) == (64, 3, 4)
    assert capi.default_tile(128, True) == capi.default_tile(512, True) == (128, 3, 4)   # the measured best (profiles/HISTORY.md 5)
    assert capi.default_tile(128, False) == (64, 3, 1)


def test_host_preprocess_entry_point_matches_golden(csr_fixture):
    g = csr_fixture
    n = int(g["num_nodes"])
    indptr = np.ascontiguousarray(g["indptr"], np.int32)
    indices = np.ascontiguousarray(g["indices"], np.int32)
    w = (n + 15) // 16
    bp, e2c = np.zeros(w, np.int32), np.zeros(indices.size, np.int32)
    e2r, p1 = np.zeros(indices.size, np.int32), np.zeros(w + 1, np.int32)
    rc = ctypes.c_int(-1)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    capi.lib().voltrix_launch_preprocess(ptr(indices), ptr(indptr), ctypes.c_int(n), ptr(bp), ptr(e2c), ptr(e2r),
                                         ptr(p1), ctypes.byref(rc))
    assert rc.value == 0
    assert (bp == g["block_partition"]).all() and (p1 == g["pointer1"]).all()
    assert (e2c == g["edge_to_column"]).all() and (e2r == g["edge_to_row"]).all()


def test_host_preprocess_is_deterministic_and_equals_the_oracle(monkeypatch):
    import scipy.sparse as sp

    np.random.seed(3)
    a = sp.random(4000, 4000, density=0.02, format="csr")
    indptr, indices = a.indptr.astype(np.int32), a.indices.astype(np.int32)
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    outs = []
    for _ in range(2):     # threads over windows (hardware_concurrency): two runs, same bytes
        bp, e2c = np.zeros(250, np.int32), np.zeros(indices.size, np.int32)
        e2r, p1 = np.zeros(indices.size, np.int32), np.zeros(251, np.int32)
        rc = ctypes.c_int(-1)
        capi.lib().voltrix_launch_preprocess(ptr(indices), ptr(indptr), ctypes.c_int(4000), ptr(bp), ptr(e2c), ptr(e2r),
                                             ptr(p1), ctypes.byref(rc))
        assert rc.value == 0
        outs.append((bp, e2c, e2r, p1))
    for x, y in zip(*outs):
        assert (x == y).all()
    from oracle import oracle_c

    for x, y in zip(outs[0], oracle_c.preprocess(indptr, indices, 4000)):
        assert (x == y).all()


def test_return_codes_on_bad_arguments(monkeypatch):
    lib = capi.lib()
    rc = ctypes.c_int(-1)
    z = ctypes.c_void_p(0)
    lib.voltrix_launch_preprocess(z, z, ctypes.c_int(-1), z, z, z, z, ctypes.byref(rc))
    assert rc.value == 1
    # embedding_dim not a multiple of 8 halves / unknown tile: rejected on the host, before any HIP call
    lib.voltrix_launch_spmm_f16_tile(z, z, z, ctypes.c_int(16), ctypes.c_int(0), ctypes.c_int(12), z, z,
                                     ctypes.c_int(128), ctypes.c_int(4), ctypes.c_int(1), z, z, z, ctypes.byref(rc))
    assert rc.value == 1
    lib.voltrix_launch_spmm_f16_tile(z, z, z, ctypes.c_int(16), ctypes.c_int(0), ctypes.c_int(16), z, z,
                                     ctypes.c_int(48), ctypes.c_int(4), ctypes.c_int(1), z, z, z, ctypes.byref(rc))
    assert rc.value == 3
    lib.voltrix_launch_cast_f32_f16(z, z, ctypes.c_int64(12), z, ctypes.byref(rc))
    assert rc.value == 1
    lib.voltrix_launch_cast_f32_f16_scaled(z, z, ctypes.c_int64(16), z, z, ctypes.byref(rc))  # no scale buffer
    assert rc.value == 1
    lib.voltrix_launch_window_order(z, ctypes.c_int(64), ctypes.c_int(8192), z, z, ctypes.byref(rc))
    assert rc.value == 1  # chunk above the 4096-window LDS sort capacity
    # sort path (column universe too large for the LDS bitmap): one uint32 key per edge; bitmap path: scan scratch only
    assert capi.csr_preprocess_workspace_bytes(2449029, 2449029, 123718280) >= 4 * 123718280
    assert 0 < capi.csr_preprocess_workspace_bytes(232965, 232965, 114615892) < 1 << 20
    assert capi.csr_preprocess_workspace_bytes(232965, 232965, 114615892, "sort") >= 4 * 114615892
    with pytest.raises(capi.VoltrixError, match="return code 3"):
        capi.check(3, "x")
