"""GPU: every operator on poisoned scratch and output memory.

Every operator of the package computes in memory that no operand defines -- workspaces, partial-tile buffers, handle arrays, padded
outputs, ``out_scale``, the tables of the two-phase builders -- and the Python layer takes all of it from ``torch.empty``.  The other GPU
tests cannot tell whether the library writes every element it later reads: a fresh device allocation is usually zero, and a recycled block
of the caching allocator usually holds the previous, correct call's values.  tests/test_gpu_views.py owns the layouts; this module owns THE
CONTENTS OF MEMORY THE CALLER DID NOT DEFINE (DESIGN.md section 3.21 lists every buffer, who writes it before who reads it, and the case
below that covers it).

Every case runs its operator three times -- unpatched, under ``poisoned(0x00)`` and under ``poisoned(0xFF)`` (tests/poisoned_alloc.py:
every ``torch.empty``-family allocation filled with that byte: NaN for every float type, -1 for every integer) -- and requires

* a positive count of filled allocations in both poisoned runs;
* BIT EQUALITY of everything the call returns (outputs, handle arrays, tables, headers, ``m`` / ``l``, masks, gradients) between the two
  poisoned runs and with the unpatched run.  No path here gives different bits from run to run: the atomic join of the two-level pair adds
  two addends onto a zero (commutative), every other sum has an order fixed by the pattern;
* once per operator, the ``0xFF`` result inside that operator's own float64 / oracle check, imported from its test file with its bound
  unchanged -- three equally wrong results cannot pass.  The SpMM forms use small-integer operands, so the check is equality with the
  float64 product whatever the summation order (the atomic forms included).

``stale`` mode (entry points that take a caller-owned workspace or partial-tile buffer): the operator on input X2 with the buffer that a
call on X1 left behind -- X1 and X2 of one size class, different in exactly what the buffer caches -- against X2 on a zeroed buffer.

The environment is pinned as the per-operator tests pin it; every case names the path it selects.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest
import torch

import test_gpu_attn_aggregate as t_attn
import test_gpu_attn_dropout as t_drop
import test_gpu_edge_softmax as t_softmax
import test_gpu_gat_score as t_gat
import test_gpu_gatv2 as t_gatv2
import test_gpu_heads as t_heads
import test_gpu_preprocess as t_pre
import test_gpu_schedule as t_sched
import test_gpu_sddmm as t_sddmm
import test_gpu_spmm as t_spmm
import test_gpu_views as t_views
import test_gpu_weighted as t_weighted
import voltrix
from conftest import load_csr_fixture
from oracle import oracle_np
from poisoned_alloc import poisoned, stale
from voltrix import capi, hybrid, reorder, sidecar, weighted
from voltrix.schedule import (balanced_xcd_windows, split_equal_work, stream_tables, stream_tables_torch, unit_table,
                              unit_table_torch)

pytestmark = pytest.mark.gpu

CHUNK = 2048                 # kChunkEdges of the edge softmax and of both gat_score kernels


@pytest.fixture(autouse=True)
def _pinned(monkeypatch):
    """The untuned default tiles, the window format, no CSR side-car, the scaled cast for fp32 rows, the library's preprocess route;
    a case that selects another path sets its own values."""
    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "none")
    monkeypatch.setenv("VOLTRIX_HYBRID", "0")
    monkeypatch.setenv("VOLTRIX_FUSED", "0")
    monkeypatch.setenv("VOLTRIX_CSR_PATH", "0")
    monkeypatch.delenv("VOLTRIX_FP32_MODE", raising=False)
    monkeypatch.delenv("VOLTRIX_PREPROCESS", raising=False)
    monkeypatch.delenv("VOLTRIX_HYBRID_MIN_SHARE", raising=False)


# ---- the three runs --------------------------------------------------------------------------------------------------------------------
_SCALARS = (int, float, str, bool, type(None))


def _leaves(obj, path="result", depth=0):
    """(path, leaf) for every tensor, array and scalar a call returned: tuples, lists, dicts and the package's dataclasses (tables, plans,
    handles) are walked, anything else is an error -- nothing is skipped silently."""
    if isinstance(obj, (torch.Tensor, np.ndarray) + _SCALARS):
        yield path, obj
    elif isinstance(obj, (tuple, list)):
        for i, v in enumerate(obj):
            yield from _leaves(v, f"{path}[{i}]", depth + 1)
    elif isinstance(obj, dict):
        for k in sorted(obj, key=str):
            yield from _leaves(obj[k], f"{path}[{k!r}]", depth + 1)
    elif dataclasses.is_dataclass(obj) and depth < 6:
        for f in dataclasses.fields(obj):
            yield from _leaves(getattr(obj, f.name), f"{path}.{f.name}", depth + 1)
    else:
        raise TypeError(f"{path}: a {type(obj).__name__} among the results")


def _bytes(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _assert_same(a, b, what):
    la, lb = list(_leaves(a)), list(_leaves(b))
    assert [p for p, _ in la] == [p for p, _ in lb], what
    for (path, x), (_, y) in zip(la, lb):
        if isinstance(x, torch.Tensor):
            assert isinstance(y, torch.Tensor) and x.dtype == y.dtype and x.shape == y.shape and x.device == y.device, (what, path)
            if not torch.equal(_bytes(x), _bytes(y)):
                bad = torch.nonzero(_bytes(x) != _bytes(y)).flatten()
                first = int(bad[0]) // x.element_size()
                raise AssertionError(f"{what}: {path} {tuple(x.shape)} {x.dtype} differs in {bad.numel()} bytes, first at element {first}: "
                                     f"{x.reshape(-1)[first].item()!r} vs {y.reshape(-1)[first].item()!r}")
        elif isinstance(x, np.ndarray):
            assert np.array_equal(x, y), (what, path)
        else:
            assert x == y, (what, path, x, y)


def three_runs(call, what):
    """``call()`` unpatched, on zero-filled and on 0xFF-filled allocations: everything it returns is bit-equal; returns the 0xFF result."""
    plain = call()
    torch.cuda.synchronize()
    results = {}
    for byte in (0x00, 0xFF):
        with poisoned(byte) as state:
            results[byte] = call()
            torch.cuda.synchronize()
        assert state.filled > 0, f"{what}: no allocation of the call went through the patched torch.empty family"
    _assert_same(results[0x00], results[0xFF], f"{what}: 0x00 against 0xFF")
    _assert_same(plain, results[0xFF], f"{what}: unpatched against 0xFF")
    return results[0xFF]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(x, dtype=torch.int32):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def _poison_bytes(nbytes):
    """A caller-owned buffer of ``stale`` mode before its first use: 0xFF everywhere."""
    return torch.empty(max(16, int(nbytes)), dtype=torch.uint8, device="cuda").fill_(0xFF)


def _minus_ones(*shape):
    return torch.full(shape, -1, dtype=torch.int32, device="cuda")


# ---- graphs ------------------------------------------------------------------------------------------------------------------------------
def _form_graph_np(seed, hub_row, empty_from):
    """1,101 rows (68 full windows and one of 13 rows), up to 40 distinct columns per row; three windows without an edge; one hub row of
    900 columns, so that its window is many times the median length (cut by the unit table, the stream table and the default bounds)."""
    rng = np.random.default_rng(seed)
    n = 1101
    rows = [np.unique(rng.integers(0, n, rng.integers(0, 41))) for _ in range(n)]
    for r in range(empty_from, empty_from + 48):
        rows[r] = np.zeros(0, np.int64)
    rows[hub_row] = np.sort(rng.choice(n, 900, replace=False))
    indptr = np.zeros(n + 1, np.int32)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, np.concatenate(rows).astype(np.int32), n


@functools.lru_cache(maxsize=None)
def _form_graph(which=0):
    """``which`` = 0: the graph of the cases; 1: same rows, other window lengths (hub and empty windows elsewhere) for ``stale`` mode."""
    assert (16 * 20, 16 * 45)[which] % 16 == 0
    return _form_graph_np(21 + which, (5, 700)[which], (16 * 20, 16 * 45)[which])


@functools.lru_cache(maxsize=None)
def _form_handle(which=0):
    """The block-format handle of ``_form_graph(which)``, built once on ordinary allocations (the builder cases take it as their input)."""
    indptr, indices, n = _form_graph(which)
    handle = voltrix.csr_fused_preprocess_kernel(_dev(indptr), _dev(indices), n)[:3]
    t_pre._check(handle, indptr, indices, n)
    return handle


def _ints(shape, dtype, seed, scale=1):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randint(-3, 4, shape, device="cuda", generator=gen) * scale).to(dtype)


def _exact_product(indptr, indices, feat, n, values=None):
    """float64 ``csr(values or ones) @ feat`` on the host."""
    if values is None:
        return torch.from_numpy(oracle_np.spmm_csr(indptr, indices, feat.detach().cpu().double().numpy(), n))
    return t_weighted._oracle(indptr, indices, values.cpu(), feat.detach().cpu().float(), n, n).double()


def _assert_exact(out, indptr, indices, feat, n, what, values=None):
    want = _exact_product(indptr, indices, feat, n, values)
    assert out.shape == want.shape and out.dtype == torch.float32, (what, tuple(out.shape), out.dtype)
    assert torch.equal(out.cpu().double(), want), f"{what}: not the exact product of integer operands"


# ---- A. preprocess: voltrix.csr_preprocess, every route, the handle against the oracle byte for byte ------------------------------------------
def _preprocess_case(name):
    if name == "skewed_1005":
        g = load_csr_fixture(name)
        return g["indptr"], g["indices"], int(g["num_nodes"]), None
    if name == "huge_window_declared":       # 96 rows x 12,000 columns, the universe declared: the bitmap path's global-atomics branch
        return t_pre.CASES["huge_window"] + (12000,)
    return t_pre.CASES[name] + (None,)       # huge_window undeclared: ids beyond the universe, found on the device, redone by the sort path


@pytest.mark.parametrize("route", ["fused:sort", "fused:bitmap", "fused:mixed", "fused"])
@pytest.mark.parametrize("name", ["huge_window", "huge_window_declared", "dups_unsorted", "no_edges", "skewed_1005"])
def test_preprocess(cuda_device, name, route, monkeypatch):
    """Workspace (keys, scan scratch, the four queue counters, the queues, the range groups), ``block_partition``, ``pointer1``, ``status``
    and both handle arrays come from ``torch.empty``; huge_window has one window above the LDS sort capacity and 1,125 TC blocks."""
    monkeypatch.setenv("VOLTRIX_PREPROCESS", route)
    indptr, indices, n, num_cols = _preprocess_case(name)
    ip, ix = torch.as_tensor(np.asarray(indptr), dtype=torch.int32), torch.as_tensor(np.asarray(indices), dtype=torch.int32)
    handle = three_runs(lambda: voltrix.csr_preprocess(ip, ix, n, num_cols), f"csr_preprocess {name} {route}")
    t_pre._check(handle, indptr, indices, n)


@functools.lru_cache(maxsize=None)
def _queued_windows(which):
    """huge_window's degrees (``which`` = 0) and the same degrees on other rows (1): the same rows, columns, edges and workspace size,
    other windows above 2,048 and above 8,192 edges -- which windows are queued is what the preprocess workspace caches."""
    rng = np.random.default_rng(31 + which)
    deg = np.zeros(96, dtype=np.int64)
    if which == 0:
        deg[16:32], deg[40], deg[95] = 700, 3, 9000
    else:
        deg[64:80], deg[3], deg[20] = 700, 3, 9000
    indptr = np.concatenate([[0], np.cumsum(deg)])
    indices = np.concatenate([np.sort(rng.choice(12000, d, replace=False)) for d in deg if d > 0])
    return indptr, indices, 96


@pytest.mark.parametrize("path", ["sort", "bitmap", "mixed"])
def test_preprocess_stale_workspace(cuda_device, path):
    num_cols = 12000

    def run(which, workspace):
        indptr, indices, n = _queued_windows(which)
        ip, ix, windows = _dev(indptr), _dev(indices), (n + 15) // 16
        part, pointer1, status = _minus_ones(windows), _minus_ones(windows + 1), _minus_ones(1)
        capi.launch_csr_window_count(ip, ix, n, num_cols, workspace, part, pointer1, status, _stream(), path)
        total, outside = int(pointer1[-1]), int(status[0])
        assert outside == 0
        packed, hind = _minus_ones(4 * total).view(torch.uint32), _minus_ones(8 * total)
        capi.launch_csr_fill(ip, ix, n, num_cols, workspace, pointer1, packed, hind, _stream(), path)
        torch.cuda.synchronize()
        return pointer1, packed, hind, part

    size = capi.csr_preprocess_workspace_bytes(96, num_cols, int(_queued_windows(0)[0][-1]), path)
    assert size == capi.csr_preprocess_workspace_bytes(96, num_cols, int(_queued_windows(1)[0][-1]), path)
    got, want = stale(run, 0, 1, lambda: _poison_bytes(size))
    _assert_same(got, want, f"preprocess {path}: stale against zeroed workspace")
    t_pre._check(got[:3], *_queued_windows(1))


# ---- B. builders, against their restatements -------------------------------------------------------------------------------------------------
def _same_stream_tables(got, want):
    for field in ("run_cost", "cut_stages", "num_units", "num_runs", "num_cuts", "num_slots", "max_runs_per_xcd"):
        assert getattr(got, field) == getattr(want, field), field
    for field in ("units", "runs", "run_ptr", "cuts"):
        assert torch.equal(getattr(got, field), getattr(want, field)), field


@pytest.mark.parametrize("ranges", ["equal windows", "equal work"])
@pytest.mark.parametrize("max_stages", [None, 2])
def test_unit_table(cuda_device, max_stages, ranges):
    """Count workspace (histogram + statistics cleared by the launcher, ``k / kcut / cutflag``, three scans, scan scratch), header, fill
    workspace (sort keys and values, rocPRIM's temporary storage), ``units``, ``unit_ptr``, ``cuts``; max_stages = None takes the
    histogram / median kernels.  Windows are cut (k > 1) in every case."""
    blk, n = _form_handle()[0], _form_graph()[2]

    def call():
        xcd_ptr = balanced_xcd_windows(blk, n) if ranges == "equal work" else None
        return unit_table(blk, n, max_stages, xcd_ptr=xcd_ptr), xcd_ptr

    table, xcd_ptr = three_runs(call, f"unit_table {max_stages} {ranges}")
    assert table.num_cuts > 0 and table.num_slots > table.num_cuts
    t_sched._same(table, unit_table_torch(blk, n, max_stages, xcd_ptr=xcd_ptr))


@pytest.mark.parametrize("run_cost,cut_stages", [(None, None), (6, 3)])
def test_stream_table(cuda_device, run_cost, cut_stages):
    handle, n = _form_handle(), _form_graph()[2]
    table = three_runs(lambda: stream_tables(*handle, n, run_cost=run_cost, cut_stages=cut_stages), f"stream_tables {run_cost} {cut_stages}")
    assert table.num_cuts > 0
    _same_stream_tables(table, stream_tables_torch(*handle, n, run_cost=run_cost, cut_stages=cut_stages))


PLAN = (4, 2, 4)       # waves, row blocks, tau: 128-row panels, nine of them on the 1,101 rows


@functools.lru_cache(maxsize=None)
def _form_plan(which=0):
    indptr, indices, n = _form_graph(which)
    return hybrid.build_panel_plan(_dev(indptr), _dev(indices), n, None, *PLAN)


def test_panel_plan(cuda_device):
    """Count then fill: workspace, ``panel_ptr``, ``resid_indptr``, ``status``, ``resid_indices``, ``panel_cols`` and ``panel_bits`` in
    full, tails included, and the launch order of the plan."""
    indptr, indices, n = _form_graph()
    ip, ix = _dev(indptr), _dev(indices)
    ri, rx, plan = three_runs(lambda: hybrid.build_panel_plan(ip, ix, n, None, *PLAN), "build_panel_plan")
    o_ri, o_rx, o_ptr, o_cols, o_bits = oracle_np.panel_plan(indptr, indices, n, *PLAN)
    assert plan.num_ksteps > 0 and plan.num_resid_edges > 0
    assert np.array_equal(ri.cpu().numpy(), o_ri) and np.array_equal(rx.cpu().numpy(), o_rx)
    assert np.array_equal(plan.panel_ptr.cpu().numpy(), o_ptr) and np.array_equal(plan.panel_cols.cpu().numpy(), o_cols)
    assert plan.panel_cols.numel() == 32 * (plan.num_ksteps + 2) and plan.panel_bits.numel() == (plan.num_ksteps + 1) * PLAN[0] * 64
    assert np.array_equal(plan.panel_bits.view(torch.int32).cpu().numpy().view(np.uint32), o_bits)
    assert torch.equal(plan.panel_order.cpu(), hybrid.longest_first_order(plan.panel_ptr.cpu()))


@pytest.mark.parametrize("ranges", ["equal panels", "equal work"])
def test_panel_parts(cuda_device, ranges):
    plan = _form_plan()[2]
    nks = torch.diff(plan.panel_ptr).cpu().long()
    cap = max(1, int(nks.max()) // 3)
    xcd_ptr = split_equal_work(nks) if ranges == "equal work" else None

    def call():
        return hybrid.panel_parts(plan.panel_ptr, cap, xcd_ptr.cuda() if xcd_ptr is not None else None)

    native = three_runs(call, f"panel_parts {ranges}")
    ref = hybrid.panel_parts_torch(plan.panel_ptr.cpu(), cap, xcd_ptr)
    assert native.num_cuts > 0
    assert (native.num_parts, native.num_cuts, native.num_slots, native.max_parts_per_xcd, native.cap) == \
        (ref.num_parts, ref.num_cuts, ref.num_slots, ref.max_parts_per_xcd, ref.cap)
    assert torch.equal(native.xcd_ptr.cpu(), ref.xcd_ptr) and torch.equal(native.cuts.cpu(), ref.cuts)
    assert torch.equal(native.parts.cpu(), ref.parts)


def test_fused_records(cuda_device):
    handle, n = _form_handle(), _form_graph()[2]
    got = three_runs(lambda: hybrid.build_fused_records(*handle, n), "build_fused_records")
    want = hybrid.build_fused_records_torch(*handle, n)
    assert got.num_records == want.num_records > 0 and torch.equal(got.wave_ptr, want.wave_ptr)
    assert got.records.shape == (want.num_records + 1, 64)
    assert torch.equal(got.records.view(torch.int32), want.records.view(torch.int32))        # the padding record included


def test_orders_and_xcd_ranges(cuda_device):
    """``launch_window_order``, ``launch_panel_order`` and the three ``xcd_ranges_*``: their outputs are the only undefined memory."""
    blk, n = _form_handle()[0], _form_graph()[2]
    windows = (n + 15) // 16
    plan = _form_plan()[2]
    work = (torch.diff(blk).long() + 3) // 4
    panel_rows = PLAN[0] * PLAN[1] * 16

    def call():
        order = torch.empty(windows, dtype=torch.int32, device="cuda")
        capi.launch_window_order(blk, n, order, _stream(), 7)
        ranges = capi.xcd_ranges_of_work(work.to(torch.int32), 4)
        window_ranges = capi.xcd_ranges_of_windows(blk, n, 1)
        panel_ranges = capi.xcd_ranges_of_panels(plan.panel_ptr, blk, n, panel_rows, hybrid.KSTEP_COST_X10)
        panel_order = hybrid.longest_first_order(plan.panel_ptr, 1, panel_ranges[0])
        return order, ranges, window_ranges, panel_ranges, panel_order

    order, ranges, window_ranges, panel_ranges, panel_order = three_runs(call, "orders and XCD ranges")
    assert np.array_equal(order.cpu().numpy(), t_spmm._reference_window_order(blk.cpu().numpy(), windows, 7))
    assert torch.equal(ranges.cpu(), split_equal_work(work.cpu(), 4))
    assert torch.equal(window_ranges.cpu(), split_equal_work(work.cpu(), 1))
    ref = hybrid.xcd_ranges_of_panels_torch(plan.panel_ptr.cpu(), blk.cpu(), n, panel_rows, hybrid.KSTEP_COST_X10)
    assert torch.equal(panel_ranges[0].cpu(), ref[0]) and torch.equal(panel_ranges[1].cpu(), ref[1])
    assert torch.equal(panel_order.cpu(), hybrid.longest_first_order(plan.panel_ptr.cpu(), 1, ref[0]))


# the five two-phase entry points with a caller-owned workspace, as a C host calls them (the Python wrappers allocate their own)
def _rc():
    return ctypes.c_int(-1)


def _raw_unit_table(blk, n, max_stages, workspace, fill_workspace):
    lib, rc, s, null = capi.lib(), _rc(), ctypes.c_void_p(_stream()), ctypes.c_void_p(0)
    header = _minus_ones(8)
    lib.voltrix_launch_unit_table_count(capi._ptr(blk), ctypes.c_int(n), ctypes.c_int(max_stages), null, capi._ptr(workspace),
                                        capi._ptr(header), s, ctypes.byref(rc))
    assert rc.value == 0
    head = header.tolist()
    units, cuts, unit_ptr = _minus_ones(head[0], 4), _minus_ones(head[1], 4), _minus_ones(9)
    lib.voltrix_launch_unit_table_fill(capi._ptr(blk), ctypes.c_int(n), null, capi._ptr(workspace), capi._ptr(fill_workspace),
                                       ctypes.c_int(head[0]), ctypes.c_int(head[1]), ctypes.c_int(head[5]), capi._ptr(units),
                                       capi._ptr(unit_ptr), capi._ptr(cuts), s, ctypes.byref(rc))
    assert rc.value == 0
    torch.cuda.synchronize()
    return units, unit_ptr, cuts, head


def _raw_stream_table(handle, n, workspace, fill_workspace):
    lib, rc, s = capi.lib(), _rc(), ctypes.c_void_p(_stream())
    header = _minus_ones(8)
    lib.voltrix_launch_stream_table_count(capi._ptr(handle[0]), capi._ptr(handle[1]), capi._ptr(handle[2]), ctypes.c_int(n),
                                          ctypes.c_int(6), ctypes.c_int(3), capi._ptr(workspace), capi._ptr(header), s, ctypes.byref(rc))
    assert rc.value == 0
    num_units, num_cuts, _, run_bound, run_cost, _ = header.tolist()[:6]
    units, cuts, runs = _minus_ones(num_units, 8), _minus_ones(num_cuts, 4), _minus_ones(max(1, run_bound), 4)
    run_ptr, header2 = _minus_ones(9), _minus_ones(4)
    lib.voltrix_launch_stream_table_fill(capi._ptr(handle[0]), ctypes.c_int(n), capi._ptr(workspace), capi._ptr(fill_workspace),
                                         ctypes.c_int(num_units), ctypes.c_int(num_cuts), ctypes.c_int(run_bound), ctypes.c_int(run_cost),
                                         capi._ptr(units), capi._ptr(cuts), capi._ptr(runs), capi._ptr(run_ptr), capi._ptr(header2), s,
                                         ctypes.byref(rc))
    assert rc.value == 0
    torch.cuda.synchronize()
    return units, cuts, runs[:run_bound], run_ptr, header2, header


def _raw_panel_parts(panel_ptr, cap, workspace):
    lib, rc, s, null = capi.lib(), _rc(), ctypes.c_void_p(_stream()), ctypes.c_void_p(0)
    num_panels, header = panel_ptr.numel() - 1, _minus_ones(8)
    lib.voltrix_launch_panel_parts_count(capi._ptr(panel_ptr), ctypes.c_int(num_panels), ctypes.c_int(cap), null, capi._ptr(workspace),
                                         capi._ptr(header), s, ctypes.byref(rc))
    assert rc.value == 0
    head = header.tolist()
    parts, cuts, part_xcd_ptr = _minus_ones(head[0], 4), _minus_ones(max(1, head[1]), 4), _minus_ones(9)
    lib.voltrix_launch_panel_parts_fill(capi._ptr(panel_ptr), ctypes.c_int(num_panels), ctypes.c_int(cap), null, capi._ptr(workspace),
                                        capi._ptr(parts), capi._ptr(part_xcd_ptr), capi._ptr(cuts), s, ctypes.byref(rc))
    assert rc.value == 0
    torch.cuda.synchronize()
    return parts, part_xcd_ptr, cuts[:head[1]], head


def _raw_fused_records(handle, n, workspace):
    lib, rc, s = capi.lib(), _rc(), ctypes.c_void_p(_stream())
    wave_ptr = _minus_ones(capi.fused_panel_geometry()[0] * ((n + 511) // 512) + 1)
    lib.voltrix_launch_fused_records_count(capi._ptr(handle[0]), capi._ptr(handle[1]), ctypes.c_int(n), capi._ptr(workspace),
                                           capi._ptr(wave_ptr), s, ctypes.byref(rc))
    assert rc.value == 0
    num_records = int(wave_ptr[-1])
    records = _minus_ones(num_records + 1, 64)
    lib.voltrix_launch_fused_records_fill(capi._ptr(handle[0]), capi._ptr(handle[1]), capi._ptr(handle[2]), ctypes.c_int(n),
                                          capi._ptr(wave_ptr), ctypes.c_int64(num_records), capi._ptr(records), s, ctypes.byref(rc))
    assert rc.value == 0
    torch.cuda.synchronize()
    return wave_ptr, records


def _raw_panel_plan(which, workspace):
    indptr, indices, n = _form_graph(which)
    ip, ix = _dev(indptr), _dev(indices)
    waves, row_blocks, tau = PLAN
    num_panels = (n + waves * row_blocks * 16 - 1) // (waves * row_blocks * 16)
    panel_ptr, resid_indptr, status = _minus_ones(num_panels + 1), _minus_ones(n + 1), _minus_ones(1)
    assert capi.launch_panel_plan_count(ip, ix, n, n, waves, row_blocks, tau, workspace, panel_ptr, resid_indptr, status, _stream()) == 0
    ksteps, num_resid, bad = int(panel_ptr[-1]), int(resid_indptr[-1]), int(status[0])
    assert bad == 0
    resid_indices, panel_cols = _minus_ones(num_resid), _minus_ones(32 * (ksteps + 2))
    panel_bits = _minus_ones((ksteps + 1) * waves * 64)
    capi.launch_panel_plan_fill(ip, ix, n, n, waves, row_blocks, tau, workspace, panel_ptr, resid_indptr, ksteps, resid_indices, panel_cols,
                                panel_bits.view(torch.uint32), _stream())
    torch.cuda.synchronize()
    return resid_indptr, resid_indices, panel_ptr, panel_cols, panel_bits


def _two_buffers(first, second):
    """One caller-owned buffer holding a workspace of ``first`` bytes and one of ``second``: (new_buffer, split)."""
    first = (int(first) + 255) // 256 * 256
    return (lambda: _poison_bytes(first + second)), (lambda buffer: (buffer[:first], buffer[first:]))


def test_builders_stale_workspace(cuda_device):
    """X1 and X2: the two graphs of 1,101 rows whose long and empty windows sit elsewhere -- window lengths are what the tables' workspaces
    cache (histogram, statistics, per-window counts and scans, per-XCD totals), shared and residual counts what the plan's does."""
    lib, n = capi.lib(), _form_graph()[2]
    handles = [_form_handle(0), _form_handle(1)]
    tables = [unit_table_torch(h[0], n, 2) for h in handles]
    new, split = _two_buffers(lib.voltrix_unit_table_workspace_bytes(ctypes.c_int(n)),
                              lib.voltrix_unit_table_fill_workspace_bytes(ctypes.c_int64(max(t.num_units for t in tables))))
    for max_stages in (0, 2):
        got, want = stale(lambda which, b: _raw_unit_table(handles[which][0], n, max_stages, *split(b)), 0, 1, new)
        _assert_same(got, want, f"unit table, max_stages {max_stages}: stale against zeroed workspace")
    ref = tables[1]
    assert torch.equal(got[0], ref.units) and torch.equal(got[1], ref.unit_ptr) and torch.equal(got[2], ref.cuts)
    assert got[3][:5] == [ref.num_units, ref.num_cuts, ref.num_slots, ref.max_units_per_xcd, ref.max_stages] and got[3][6:] == [0, 0]

    streams = [stream_tables_torch(*h, n, run_cost=6, cut_stages=3) for h in handles]
    new, split = _two_buffers(lib.voltrix_stream_table_workspace_bytes(ctypes.c_int(n)),
                              lib.voltrix_stream_table_fill_workspace_bytes(ctypes.c_int64(max(t.num_units for t in streams))))
    got, want = stale(lambda which, b: _raw_stream_table(handles[which], n, *split(b)), 0, 1, new)
    _assert_same(got, want, "stream table: stale against zeroed workspace")
    ref = streams[1]
    assert torch.equal(got[0], ref.units) and torch.equal(got[1], ref.cuts) and torch.equal(got[3], ref.run_ptr)
    assert torch.equal(got[2][:ref.num_runs], ref.runs) and int(got[2][ref.num_runs:].abs().sum()) == 0       # runs past R: zero records
    assert got[4].tolist() == [ref.num_runs, ref.max_runs_per_xcd, 0, 0]

    plans = [_form_plan(0)[2], _form_plan(1)[2]]
    cap = max(1, int(torch.diff(plans[1].panel_ptr).max()) // 3)
    size = lib.voltrix_panel_parts_workspace_bytes(ctypes.c_int(plans[0].num_panels))
    got, want = stale(lambda which, b: _raw_panel_parts(plans[which].panel_ptr, cap, b), 0, 1, lambda: _poison_bytes(size))
    _assert_same(got, want, "panel parts: stale against zeroed workspace")
    ref = hybrid.panel_parts_torch(plans[1].panel_ptr.cpu(), cap)
    assert torch.equal(got[0].cpu(), ref.parts) and torch.equal(got[1].cpu(), ref.xcd_ptr) and torch.equal(got[2].cpu(), ref.cuts)

    size = lib.voltrix_fused_records_workspace_bytes(ctypes.c_int(n))
    got, want = stale(lambda which, b: _raw_fused_records(handles[which], n, b), 0, 1, lambda: _poison_bytes(size))
    _assert_same(got, want, "fused records: stale against zeroed workspace")
    ref = hybrid.build_fused_records_torch(*handles[1], n)
    assert torch.equal(got[0], ref.wave_ptr) and torch.equal(got[1], ref.records.view(torch.int32))

    size = capi.panel_plan_workspace_bytes(n, PLAN[0], PLAN[1])
    got, want = stale(_raw_panel_plan, 0, 1, lambda: _poison_bytes(size))
    _assert_same(got, want, "panel plan: stale against zeroed workspace")
    for mine, theirs in zip(got, oracle_np.panel_plan(*_form_graph(1), *PLAN)):
        assert np.array_equal(mine.cpu().numpy().astype(np.int64) & 0xFFFFFFFF, np.asarray(theirs).astype(np.int64) & 0xFFFFFFFF)


# ---- C. SpMM forms: small-integer operands, every output row and column equal to the float64 product ------------------------------------------
RAW_WIDTH = 56             # the raw launches: a multiple of 8 that is no multiple of a 16-column output slot or of a slab
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}


@pytest.mark.parametrize("dtype,mode,width", [("fp16", None, 52), ("bf16", None, 52), ("fp32", "fp16", 50), ("fp32", "exact", 50)])
def test_window_kernel(cuda_device, dtype, mode, width, monkeypatch):
    """``voltrix.csr_preprocess`` + ``voltrix.spmm``: the handle, the padded output (52 -> 56, 50 -> 56 / 52 columns), and for fp32 rows the
    fp16 operand -- whose head briefly holds the workgroup maxima -- and ``out_scale``; ``exact``: the fp32 tiles."""
    if mode is not None:
        monkeypatch.setenv("VOLTRIX_FP32_MODE", mode)
    indptr, indices, n = _form_graph()
    ip, ix = torch.from_numpy(indptr), torch.from_numpy(indices)
    feat = _ints((n, width), DTYPES[dtype], 1, scale=64 if dtype == "fp32" else 1)      # fp32: a scale 2^e with e != 0

    def call():
        handle = voltrix.csr_preprocess(ip, ix, n)
        handle[1].hash_tag = f"scratch_window_{dtype}_{mode}"
        return handle, voltrix.spmm(*handle, num_nodes=n, num_edges=ix.numel(), feat=feat)

    handle, out = three_runs(call, f"window kernel {dtype} {mode}")
    assert sidecar.lookup_csr(handle[1]) is None
    t_pre._check(handle, indptr, indices, n)
    _assert_exact(out, indptr, indices, feat, n, f"window kernel {dtype} {mode}")


@pytest.mark.parametrize("atomic", [False, True])
@pytest.mark.parametrize("units_per_wave", [1, 2])
def test_unit_table_launch(cuda_device, units_per_wave, atomic):
    """``voltrix_launch_spmm_f16_sched`` on a unit table with cut windows + ``voltrix_launch_combine_partials``: ``partials`` and (store
    mode) the output from ``torch.empty``; ``atomic``: the caller's zero fill, float atomics, integers -- any order gives these bits."""
    indptr, indices, n = _form_graph()
    handle, nnz = _form_handle(), int(indptr[-1])
    table = unit_table(handle[0], n, 2)
    feat = _ints((n, RAW_WIDTH), torch.float16, 2)

    def call():
        out = torch.zeros(n, RAW_WIDTH, device="cuda") if atomic else torch.empty(n, RAW_WIDTH, device="cuda")
        partials = torch.empty(table.num_slots * 16 * RAW_WIDTH, device="cuda")
        assert capi.launch_spmm_sched(handle[0].data_ptr(), handle[1].data_ptr(), handle[2].data_ptr(), n, nnz, RAW_WIDTH, feat.data_ptr(),
                                      out.data_ptr(), (128, 3, 4), _stream(), 0, 0, atomic, False, table, partials.data_ptr(), 0,
                                      units_per_wave) == 0
        assert capi.launch_combine_partials(table, partials.data_ptr(), out.data_ptr(), n, RAW_WIDTH, atomic, _stream()) == 0
        return out

    out = three_runs(call, f"unit-table launch, {units_per_wave} per wave, atomic {atomic}")
    assert table.num_cuts > 0
    _assert_exact(out, indptr, indices, feat, n, "unit-table launch")


def test_stream_kernel(cuda_device):
    indptr, indices, n = _form_graph()
    handle = _form_handle()
    table = stream_tables(*handle, n, run_cost=6, cut_stages=3)
    feat = _ints((n, RAW_WIDTH), torch.float16, 3)

    def call():
        out = torch.empty(n, RAW_WIDTH, device="cuda")
        partials = torch.empty(max(1, table.num_slots) * 16 * RAW_WIDTH, device="cuda")
        assert capi.launch_spmm_stream(handle[1], handle[2], n, RAW_WIDTH, feat, out, table, partials) == 0
        assert capi.launch_combine_partials(table, partials.data_ptr(), out.data_ptr(), n, RAW_WIDTH, False, _stream()) == 0
        return out

    out = three_runs(call, "stream kernel")
    assert table.num_cuts > 0
    _assert_exact(out, indptr, indices, feat, n, "stream kernel")


def test_partial_tiles_stale(cuda_device):
    """The partial-tile buffer of the unit-table launch and of the stream kernel after a call on the OTHER graph and other features: the
    cut windows, their slots and every tile differ."""
    n = _form_graph()[2]
    graphs, handles = [_form_graph(0), _form_graph(1)], [_form_handle(0), _form_handle(1)]
    feats = [_ints((n, RAW_WIDTH), torch.float16, 4, scale=5), _ints((n, RAW_WIDTH), torch.float16, 5)]
    units = [unit_table(h[0], n, 2) for h in handles]
    streams = [stream_tables(*h, n, run_cost=6, cut_stages=3) for h in handles]

    def run_units(which, partials):
        h, out = handles[which], torch.full((n, RAW_WIDTH), float("nan"), device="cuda")
        assert capi.launch_spmm_sched(h[0].data_ptr(), h[1].data_ptr(), h[2].data_ptr(), n, int(graphs[which][0][-1]), RAW_WIDTH,
                                      feats[which].data_ptr(), out.data_ptr(), (128, 3, 4), _stream(), 0, 0, False, False, units[which],
                                      partials.data_ptr(), 0, 2) == 0
        assert capi.launch_combine_partials(units[which], partials.data_ptr(), out.data_ptr(), n, RAW_WIDTH, False, _stream()) == 0
        return out

    def run_stream(which, partials):
        h, out = handles[which], torch.full((n, RAW_WIDTH), float("nan"), device="cuda")
        assert capi.launch_spmm_stream(h[1], h[2], n, RAW_WIDTH, feats[which], out, streams[which], partials.view(torch.float32)) == 0
        assert capi.launch_combine_partials(streams[which], partials.data_ptr(), out.data_ptr(), n, RAW_WIDTH, False, _stream()) == 0
        return out

    for name, run, tables in (("unit table", run_units, units), ("stream", run_stream, streams)):
        size = 4 * 16 * RAW_WIDTH * max(t.num_slots for t in tables)
        got, want = stale(run, 0, 1, lambda: _poison_bytes(size))
        _assert_same(got, want, f"{name}: stale against zeroed partial tiles")
        _assert_exact(got, *graphs[1][:2], feats[1], n, name)


@pytest.mark.parametrize("form", ["pair", "pair one stream", "one launch"])
def test_two_level(cuda_device, form, monkeypatch):
    """``csr_preprocess_hybrid`` (plan builder, residual handle, XCD ranges; ``one launch``: the stage records) and ``spmm_two_level``: the
    pair on two streams with whichever join ``hybrid.join_mode`` picks for the run (each run's ``hybrid.LAST_JOIN["mode"]`` goes into
    the failure message; None: the form has no join) -- panels in pieces, so panel partials and both combine passes run -- the
    one-stream form, and ``spmm_fused_kernel``.  52 columns: padded to 56."""
    monkeypatch.setenv("VOLTRIX_FUSED", "1" if form == "one launch" else "0")
    indptr, indices, n = _form_graph()
    ip, ix = torch.from_numpy(indptr), torch.from_numpy(indices)
    feat = _ints((n, 52), torch.float16, 6)

    joins = []

    def call():
        two = voltrix.csr_preprocess_hybrid(ip, ix, n, tau=4)
        two.hash_tag = f"scratch_two_level_{form}"
        if form != "one launch":
            cap = max(1, int(torch.diff(two.plan.panel_ptr).max()) // 3)
            two.plan.parts = hybrid.panel_parts(two.plan.panel_ptr, cap, two.plan.xcd_ptr)
        hybrid.LAST_JOIN["mode"] = None
        out = voltrix.spmm_two_level(two, feat, concurrent=form != "pair one stream")
        joins.append(hybrid.LAST_JOIN["mode"])
        return two, out

    try:
        two, out = three_runs(call, f"two-level {form}")
        assert two.plan.num_ksteps > 0 and two.plan.num_resid_edges > 0
        assert (two.fused is not None and two.fused.num_records > 0) if form == "one launch" else (two.plan.parts.num_cuts > 0)
        _assert_exact(out, indptr, indices, feat, n, f"two-level {form}")
    except AssertionError as error:
        raise AssertionError(f"{error} [join of each run: {joins}]") from error


@pytest.mark.parametrize("dtype,width", [("fp16", 52), ("fp32", 50)])
@pytest.mark.parametrize("valued", [False, True])
def test_csr_row_gather(cuda_device, dtype, width, valued, monkeypatch):
    """``VOLTRIX_CSR_PATH=1``: the CSR row-gather kernel behind ``voltrix.spmm`` and, with values, behind ``voltrix.spmm_weighted``."""
    monkeypatch.setenv("VOLTRIX_CSR_PATH", "1")
    indptr, indices, n = _form_graph()
    ip, ix = torch.from_numpy(indptr), torch.from_numpy(indices)
    feat = _ints((n, width), DTYPES[dtype], 7)
    values = _ints((ix.numel(),), torch.float32, 8) if valued else None

    def call():
        if valued:
            handle = voltrix.csr_preprocess_weighted(ip, ix, values, n, separable=False)
            assert weighted._weighted_path(handle, feat) == "csr"
            return voltrix.spmm_weighted(handle, feat, hash_tag="scratch_csr_values")
        handle = voltrix.csr_preprocess(ip, ix, n)
        handle[1].hash_tag = "scratch_csr"
        assert sidecar.lookup_csr(handle[1]) is not None
        return voltrix.spmm(*handle, num_nodes=n, num_edges=ix.numel(), feat=feat)

    out = three_runs(call, f"CSR row gather {dtype} values {valued}")
    _assert_exact(out, indptr, indices, feat, n, "CSR row gather", values)


def test_slab_launches(cuda_device, monkeypatch):
    """F = 256: two 128-column slabs, one launch each (``SLAB_POLICY`` = 1)."""
    from voltrix.jit_kernels import spmm as wrapper

    monkeypatch.setattr(wrapper, "SLAB_POLICY", 1)
    indptr, indices, n = _form_graph()
    ip, ix = torch.from_numpy(indptr), torch.from_numpy(indices)
    feat = _ints((n, 256), torch.float16, 9)

    def call():
        handle = voltrix.csr_preprocess(ip, ix, n)
        handle[1].hash_tag = "scratch_slabs"
        return voltrix.spmm(*handle, num_nodes=n, num_edges=ix.numel(), feat=feat)

    assert wrapper.slab_launches(256, 128, 2, n, 1) == 2
    _assert_exact(three_runs(call, "slab launches"), indptr, indices, feat, n, "slab launches")


def test_value_plane_and_update_edge_values(cuda_device):
    """``csr_preprocess_weighted`` (general values: the value plane), the weighted window kernel, then ``update_edge_values`` (edge slots,
    one scatter per plane) and the product with the new values.  Integer values and features: exact in the 16-bit planes."""
    indptr, indices, n = _form_graph()
    ip, ix = torch.from_numpy(indptr), torch.from_numpy(indices)
    feat = _ints((n, 52), torch.float16, 10)
    first, second = _ints((ix.numel(),), torch.float32, 11), _ints((ix.numel(),), torch.float32, 12)

    def call():
        handle = voltrix.csr_preprocess_weighted(ip, ix, first, n, separable=False)
        assert weighted._weighted_path(handle, feat) == "plane"
        before = voltrix.spmm_weighted(handle, feat, hash_tag="scratch_plane")
        voltrix.update_edge_values(handle, second)
        after = voltrix.spmm_weighted(handle, feat)
        return before, after, handle.planes[torch.float16], handle.edge_slot

    before, after, plane, _ = three_runs(call, "value plane")
    _assert_exact(before, indptr, indices, feat, n, "value plane", first)
    _assert_exact(after, indptr, indices, feat, n, "updated value plane", second)
    assert plane.shape == (int(_form_handle()[0][-1]), 16, 8)


def test_row_reordered_handle(cuda_device):
    """``csr_preprocess_reordered(method="bfs")``: the Cuthill-McKee search, the permuted CSR, the handle, ``row_map`` -- and the product
    written through the map: every row of the output comes from the kernel."""
    indptr, indices, n = _form_graph()
    ip, ix = torch.from_numpy(indptr), torch.from_numpy(indices)
    feat = _ints((n, 52), torch.float16, 13)

    def call():
        handle = voltrix.csr_preprocess_reordered(ip, ix, n, method="bfs")
        return handle, voltrix.spmm_reordered(handle, feat, hash_tag="scratch_reordered")

    handle, out = three_runs(call, "row-reordered handle")
    assert handle.row_map is not None and np.array_equal(handle.perm.cpu().numpy(), oracle_np.cm_order(indptr, indices, n))
    _assert_exact(out, indptr, indices, feat, n, "row-reordered handle")


def test_fp32_as_fp16_entry_point(cuda_device):
    """``voltrix_launch_spmm_f32_as_f16``: the caller-owned workspace holds the fp16 operand, the workgroup maxima and the scale.  Poisoned;
    and stale after features 2^20 times larger -- the maxima and the scale are what it caches."""
    indptr, indices, n = _form_graph()
    handle, nnz = _form_handle(), int(indptr[-1])
    feats = [_ints((n, RAW_WIDTH), torch.float32, 14, scale=2 ** 20), _ints((n, RAW_WIDTH), torch.float32, 15)]
    size = capi.spmm_f32_workspace_bytes(n, RAW_WIDTH)

    def run(which, workspace, out=None):
        out = torch.full((n, RAW_WIDTH), float("nan"), device="cuda") if out is None else out
        assert capi.launch_spmm_f32_as_f16(*handle, n, nnz, RAW_WIDTH, feats[which], out, workspace, _stream()) == 0
        return out

    out = three_runs(lambda: run(1, torch.empty(size, dtype=torch.uint8, device="cuda"), torch.empty(n, RAW_WIDTH, device="cuda")),
                     "spmm_f32_as_f16")
    _assert_exact(out, indptr, indices, feats[1], n, "spmm_f32_as_f16")
    got, want = stale(run, 0, 1, lambda: _poison_bytes(size))
    _assert_same(got, want, "spmm_f32_as_f16: stale against zeroed workspace")
    _assert_same(got, out, "spmm_f32_as_f16: stale against poisoned")


def test_row_sharded_world1(cuda_device):
    """voltrix/dist.py at world size 1 (no process group): the shard's handle, the kept gather buffer, the product."""
    from voltrix.dist import RowShardedSpMM

    indptr, indices, n = _form_graph()
    ip, ix = torch.from_numpy(indptr), torch.from_numpy(indices)
    feat = _ints((n, 64), torch.float16, 16)
    out = three_runs(lambda: RowShardedSpMM(ip, ix, n, hash_tag="scratch_dist")(feat), "RowShardedSpMM, world 1")
    _assert_exact(out, indptr, indices, feat, n, "RowShardedSpMM")


# ---- D. reorder ----------------------------------------------------------------------------------------------------------------------------
def test_csr_transpose(cuda_device):
    """Workspace (expanded rows, sorted columns, rocPRIM's storage), ``t_indptr``, ``t_indices``: duplicates kept; no entries at all."""
    rng = np.random.default_rng(2)
    for n, m, density in ((70, 333, 0.02), (513, 64, 0.3), (40, 40, 0.0)):
        a = rng.random((n, m)) < density
        rows = [np.nonzero(r)[0] for r in a]
        rows = [rng.permutation(np.concatenate([r, r[:1]])) if len(r) else r for r in rows]          # unsorted, a repeated entry per row
        ip = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        ix = (np.concatenate(rows) if ip[-1] else np.zeros(0)).astype(np.int32)
        d_ip, d_ix = _dev(ip), _dev(ix)
        t_ip, t_ix = three_runs(lambda: capi.csr_transpose(d_ip, d_ix, n, m), f"csr_transpose {n} x {m}")
        row_of = np.repeat(np.arange(n), np.diff(ip))
        assert np.array_equal(t_ix.cpu().numpy(), row_of[np.lexsort((row_of, ix))])
        assert np.array_equal(t_ip.cpu().numpy(), np.concatenate([[0], np.cumsum(np.bincount(ix, minlength=m))]))


@pytest.mark.parametrize("seed", [0, 1])
def test_cuthill_mckee_search(cuda_device, seed):
    """The small graphs of tests/test_gpu_reorder_search.py: the transpose, ``tie``, the search's queue, the rank workspace, ``perm``."""
    import test_gpu_reorder_search as t_search

    rng = np.random.default_rng(seed)
    for _ in range(4):
        n = int(rng.integers(1, 200))
        m = int(rng.choice([n, n, n + 9, max(1, n - 11)]))
        ip, ix = t_search._random_csr(rng, n, m, float(rng.choice([0.005, 0.02, 0.1])))
        budget = int(rng.choice([1, 3, 64]))
        d_ip, d_ix = ip.cuda(), ix.cuda()
        got = three_runs(lambda: reorder.bfs_permutation(d_ip, d_ix, n, m, max_components=budget), f"bfs_permutation {n} x {m}")
        assert np.array_equal(got.cpu().numpy(), oracle_np.cm_order(ip.numpy(), ix.numpy(), n, m, max_components=budget)), (n, m, budget)


def test_spectral_order(cuda_device):
    """The label-shuffled reddit-like stand-in at the size tests/test_reorder.py uses: the spectral order puts neighbours back side by
    side (that test's bound) whatever the allocations held."""
    import synth_graphs

    indptr, indices, _ = synth_graphs.generate("reddit_like", device="cuda", scale=0.25)
    n = indptr.numel() - 1
    s_indptr, s_indices, label = synth_graphs.shuffle_labels(indptr, indices, 101)
    perm = three_runs(lambda: reorder.spectral_permutation(s_indptr, s_indices, n), "spectral_permutation")
    assert sorted(perm.tolist()) == list(range(n))
    natural_of = torch.zeros_like(label)
    natural_of[label] = torch.arange(n, device="cuda")
    spread = (natural_of[perm][1:] - natural_of[perm][:-1]).abs().float().median().item()
    assert spread < 2048, spread


# ---- E. the attention family on test_gpu_views.chunk_pattern() plus a row of more than 64 chunks -----------------------------------------------
@functools.lru_cache(maxsize=None)
def _attention_pattern():
    """``chunk_pattern()`` (3 1/2 chunks of 2,048 edges, a row over three chunks, a partial last thread) with one more row in front of
    its last one that crosses 66 chunk boundaries: the 64-lane merge of the chunk partials takes a second trip.  ``nnz % 8`` stays 5."""
    lengths, cols, num_cols = t_views.chunk_pattern()
    rng = np.random.default_rng(12)
    long_row = 66 * CHUNK + 24
    head = int(lengths[:-1].sum())
    lengths = np.concatenate([lengths[:-1], [long_row], lengths[-1:]])
    cols = np.concatenate([cols[:head], rng.integers(0, num_cols, long_row), cols[head:]])
    ip = np.concatenate([[0], np.cumsum(lengths)])
    assert (ip[-2] - 1) // CHUNK - ip[-3] // CHUNK > 64 and ip[-1] % 8 == 5 and lengths[-1] == 1
    return lengths, cols, num_cols


@functools.lru_cache(maxsize=None)
def _attention_graph(kind="gat"):
    """``gat``: the pattern with the long row, for the operators that split their work by 2,048-edge chunks and merge chunk partials
    (edge softmax, both gat_score kernels) and for sddmm / spmm_heads.  ``gatv2`` / ``attn``: ``chunk_pattern()`` as it is -- gatv2_score,
    gatv2_rowsum and the three attn_aggregate kernels have no chunk merge for the long row to take a second trip of (a row per lane
    group, or 128-edge chunks with no partials), and their float64 oracles sum a 135,192-entry row with atomics: a minute per case."""
    if kind == "gat":
        return t_gat._Graph(*_attention_pattern())
    return {"gatv2": t_gatv2._Graph, "attn": t_attn._Graph}[kind](*t_views.chunk_pattern())


@functools.lru_cache(maxsize=None)
def _other_boundaries():
    """``stale`` mode's X1: the SAME number of edges in 40 rows of (nearly) equal length -- every chunk's first and last row, every
    crossing row and every merged partial differ from the pattern's."""
    nnz = int(_attention_pattern()[0].sum())
    lengths = np.full(40, nnz // 40, np.int64)
    lengths[-1] += nnz - int(lengths.sum())
    return _dev(np.concatenate([[0], np.cumsum(lengths)])), 40


_randn = t_views._randn


def _grads(out, leaves, grad):
    return torch.autograd.grad(out, leaves, grad_outputs=grad)


def _leaf(*tensors):
    return [t.clone().requires_grad_(True) for t in tensors]


@pytest.mark.parametrize("shape,dtype", [((64,), "fp16"), ((3, 20), "fp32"), ((3, 13), "fp16")])
def test_sddmm(cuda_device, shape, dtype):
    """2-D and heads, through ``autograd.SDDMM``: forward, and both gradients (row-gather products on the CSR and on its transpose, which
    the operator builds: ``csr_transpose``'s workspace).  (3, 13) is padded per head by the Python layer."""
    from voltrix.autograd import SDDMM

    g = _attention_graph()
    x, y = _randn((g.num_rows,) + shape, DTYPES[dtype], 1), _randn((g.num_cols,) + shape, DTYPES[dtype], 2)
    grad = _randn((g.nnz,) + shape[:-1], seed=3)

    def call():
        op = SDDMM(g.indptr, g.indices, g.num_rows, g.num_cols)
        xs = _leaf(x, y)
        out = op(*xs)
        return (out.detach(),) + _grads(out, xs, grad) + (op.t_indptr, op.t_indices, op.t_order)

    out, d_x, d_y = three_runs(call, f"SDDMM {shape} {dtype}")[:3]
    if len(shape) == 1:
        t_sddmm._check(g.indptr, g.indices, x, y, out, False)
    else:
        t_heads._check_sddmm(g.indptr, g.indices, x, y, out, False, single_head_bits=False)
    # d_x = csr(grad) @ y per head: the aggregation's own check on the gradient (fp32 result, cast to the operand's type)
    if len(shape) == 2 and dtype == "fp32":
        t_heads._check_aggregate(g.indptr, g.indices, grad, y, g.num_rows, d_x, single_head_bits=False)
        t_heads._check_aggregate(g.t_indptr, g.t_indices, grad[g.t_order.long()], x, g.num_cols, d_y, single_head_bits=False)


@pytest.mark.parametrize("heads", [None, 3])
def test_edge_softmax(cuda_device, heads):
    """Through ``autograd.EdgeSoftmax``: the workspace (rows, two partials and a merged partial per chunk and head) of the forward and of
    the backward, and both outputs."""
    from voltrix.autograd import EdgeSoftmax

    g = _attention_graph()
    shape = (g.nnz,) if heads is None else (g.nnz, heads)
    scores, grad = _randn(shape, seed=4) * 4, _randn(shape, seed=5)

    def call():
        s, = _leaf(scores)
        alpha = EdgeSoftmax(g.indptr, g.num_rows)(s, 0.5)
        return (alpha.detach(),) + _grads(alpha, [s], grad)

    alpha, back = three_runs(call, f"EdgeSoftmax {heads}")
    checks = t_softmax if heads is None else t_heads
    checks._check_forward(g.indptr, scores, 0.5, alpha)
    checks._check_backward(g.indptr, alpha, grad, 0.5, back)


@pytest.mark.parametrize("heads", [1, 3])
def test_edge_softmax_stale_workspace(cuda_device, heads):
    """X1: 40 rows of equal length, X2: the pattern -- equal ``nnz`` (one workspace size), other row boundaries in every chunk."""
    g = _attention_graph()
    other_indptr, other_rows = _other_boundaries()
    shape = (g.nnz,) if heads == 1 else (g.nnz, heads)
    scores = [_randn(shape, seed=6) * 9, _randn(shape, seed=7) * 4]
    grad = _randn(shape, seed=8)
    patterns = [(other_indptr, other_rows), (g.indptr, g.num_rows)]
    fwd = capi.launch_edge_softmax_csr if heads == 1 else capi.launch_edge_softmax_heads_csr
    bwd = capi.launch_edge_softmax_backward_csr if heads == 1 else capi.launch_edge_softmax_heads_backward_csr
    size = capi.edge_softmax_workspace_bytes(g.num_rows, g.nnz) if heads == 1 else capi.edge_softmax_heads_workspace_bytes(g.num_rows, g.nnz, heads)

    def run(which, workspace):
        indptr, rows = patterns[which]
        alpha, back = torch.full(shape, float("nan"), device="cuda"), torch.full(shape, float("nan"), device="cuda")
        fwd(indptr, rows, scores[which], 0.5, alpha, workspace, _stream())
        bwd(indptr, rows, alpha, grad, 0.5, back, workspace, _stream())
        return alpha, back

    got, want = stale(run, 0, 1, lambda: _poison_bytes(size))
    _assert_same(got, want, f"edge softmax H={heads}: stale against zeroed workspace")
    checks = t_softmax if heads == 1 else t_heads
    checks._check_forward(g.indptr, scores[1], 0.5, got[0])
    checks._check_backward(g.indptr, got[0], grad, 0.5, got[1])


def test_spmm_heads(cuda_device):
    from voltrix.autograd import SpMMHeads

    g = _attention_graph()
    feat, values = _randn((g.num_cols, 3, 20), seed=9), _randn((g.nnz, 3), seed=10)
    grad = _randn((g.num_rows, 3, 20), seed=11)

    def call():
        xs = _leaf(feat, values)
        out = SpMMHeads(g.indptr, g.indices, g.num_rows, g.num_cols)(*xs)
        return (out.detach(),) + _grads(out, xs, grad)

    out, d_feat, d_values = three_runs(call, "SpMMHeads")
    t_heads._check_aggregate(g.indptr, g.indices, values, feat, g.num_rows, out, single_head_bits=False)
    t_heads._check_aggregate(g.t_indptr, g.t_indices, values[g.t_order.long()], grad, g.num_cols, d_feat, single_head_bits=False)
    t_heads._check_sddmm(g.indptr, g.indices, grad, feat, d_values, False, single_head_bits=False)


@pytest.mark.parametrize("heads", [1, 3, 4])
def test_gat_score(cuda_device, heads):
    """Through ``autograd.GATScore``: the scores and both row sums (zero fill, chunk sums into the workspace, merge)."""
    from voltrix.autograd import GATScore

    g = _attention_graph()
    el, er, grad = _randn((g.num_rows, heads), seed=12), _randn((g.num_cols, heads), seed=13), _randn((g.nnz, heads), seed=14)

    def call():
        xs = _leaf(el, er)
        s = GATScore(g.indptr, g.indices, g.num_rows, g.num_cols)(*xs, 0.2)
        return (s.detach(),) + _grads(s, xs, grad)

    s, d_el, d_er = three_runs(call, f"GATScore H={heads}")
    ref, bound, (r_el, b_el), (r_er, b_er), _ = t_gat._oracle(g, el, er, 0.2, grad)
    t_gat._within(s, ref, bound, f"scratch: gat_score H={heads}")
    t_gat._within(d_el, r_el, b_el, f"scratch: d_el H={heads}")
    t_gat._within(d_er, r_er, b_er, f"scratch: d_er H={heads}")


def test_gat_score_rowsum_stale_workspace(cuda_device):
    g = _attention_graph()
    other_indptr, other_rows = _other_boundaries()
    heads = 3
    grads = [_randn((g.nnz, heads), seed=15) * 7, _randn((g.nnz, heads), seed=16)]
    el, er = _randn((g.num_rows, heads), seed=17), _randn((g.num_cols, heads), seed=18)
    patterns = [(other_indptr, other_rows), (g.indptr, g.num_rows)]
    size = capi.gat_score_workspace_bytes(g.num_rows, g.nnz, heads)

    def run(which, workspace):
        indptr, rows = patterns[which]
        out = torch.full((rows, heads), float("nan"), device="cuda")
        capi.launch_gat_score_rowsum_csr(indptr, g.indices, None, rows, el[:rows].contiguous(), er, grads[which], 0.2, out, workspace, _stream())
        return out

    got, want = stale(run, 0, 1, lambda: _poison_bytes(size))
    _assert_same(got, want, "gat_score row sum: stale against zeroed workspace")
    _, _, (r_el, b_el), _, _ = t_gat._oracle(g, el, er, 0.2, grads[1])
    t_gat._within(got, r_el, b_el, "scratch: stale d_el")


@pytest.mark.parametrize("heads,dim,dtype", [(3, 20, "fp32"), (4, 16, "fp16")])
def test_gatv2_score(cuda_device, heads, dim, dtype):
    """Through ``autograd.GATv2Score``: the scores and both gated row sums ``G_l`` / ``G_r``; the dense gradient formulas are torch's."""
    from voltrix.autograd import GATv2Score
    from voltrix.gatv2_score import gatv2_rowsum

    g = _attention_graph("gatv2")
    xl, xr = _randn((g.num_rows, heads, dim), DTYPES[dtype], 19), _randn((g.num_cols, heads, dim), DTYPES[dtype], 20)
    a, grad = _randn((heads, dim), seed=21), _randn((g.nnz, heads), seed=22)

    def call():
        xs = _leaf(xl, xr, a)
        s = GATv2Score(g.indptr, g.indices, g.num_rows, g.num_cols)(*xs, 0.2)
        big_l = gatv2_rowsum(g.indptr, g.indices, xl, xr, grad, 0.2)
        big_r = gatv2_rowsum(g.t_indptr, g.t_indices, xr, xl, grad, 0.2, order=g.t_order)
        return (s.detach(), big_l, big_r) + _grads(s, xs, grad)

    s, big_l, big_r = three_runs(call, f"GATv2Score H={heads} D={dim} {dtype}")[:3]
    (s_ref, s_bound), (l_ref, l_bound), (r_ref, r_bound) = t_gatv2._oracle(g, xl, xr, a, 0.2, grad)
    t_gatv2._within(s, s_ref, s_bound, "scratch: gatv2_score")
    t_gatv2._within(big_l, l_ref, l_bound, "scratch: G_l")
    t_gatv2._within(big_r, r_ref, r_bound, "scratch: G_r")


ATTN_SEED, ATTN_OFFSET = 1234, 56


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("heads,dim,dtype", [(3, 20, "fp32"), (4, 16, "fp16")])
def test_attn_aggregate(cuda_device, heads, dim, dtype, masked):
    """Through ``autograd.AttnAggregate`` (``d_s`` and ``d_feat``), with and without a keep mask (made inside the call: its words come from
    ``torch.empty`` too), and the functional calls for ``m``, ``l`` and the fp32 ``d_feat`` the bound is stated for."""
    from voltrix.attn_aggregate import attn_aggregate, attn_aggregate_grad_feat
    from voltrix.autograd import AttnAggregate
    from voltrix.dropout import unpack_mask

    g = _attention_graph("attn")
    scores, feat = 2.0 * _randn((g.nnz, heads), seed=23), _randn((g.num_cols, heads, dim), DTYPES[dtype], 24)
    grad = _randn((g.num_rows, heads, dim), seed=25)
    drop = dict(dropout_p=0.6, seed=ATTN_SEED, offset=ATTN_OFFSET) if masked else {}

    def call():
        f, s = _leaf(feat, scores)
        out = AttnAggregate(g.indptr, g.indices, g.num_rows, g.num_cols)(f, s, 1.0, **drop)
        keep = dict(mask=voltrix.dropout_mask(g.nnz, heads, 0.6, ATTN_SEED, ATTN_OFFSET), keep_scale=t_drop.KS) if masked else {}
        out2, m, big_l = attn_aggregate(g.indptr, g.indices, scores, feat, g.num_rows, 1.0, return_stats=True, **keep)
        d_feat32 = attn_aggregate_grad_feat(g.t_indptr, g.t_indices, g.t_order, grad, scores, m, big_l, g.num_cols, 1.0, **keep)
        d_feat, d_s = _grads(out, [f, s], grad)
        return (out.detach(), d_s, d_feat, out2, m, big_l, d_feat32) + ((keep["mask"],) if masked else ())

    got = three_runs(call, f"AttnAggregate H={heads} D={dim} {dtype} mask {masked}")
    out, d_s, d_feat, out2, m, big_l, d_feat32 = got[:7]
    assert t_attn._same_bits(out, out2) and d_feat.dtype == feat.dtype and torch.equal(d_feat, d_feat32.to(feat.dtype))
    if masked:
        ref = t_drop._oracle(g, scores, feat, grad, 1.0, unpack_mask(got[7], heads), t_drop.KS)
    else:
        ref = t_attn._oracle(g, scores, feat, grad, 1.0)
    t_attn._check_all(ref, (out, m, big_l, d_s, d_feat32), f"scratch H={heads} D={dim} {dtype} mask {masked}")


def test_dropout_mask_two_words(cuda_device):
    """H = 33: two words per edge, the second with one valid bit -- every word written, the bits past H zero, on any memory."""
    from test_attn_dropout_host import keep_bits, pack, threshold_of

    nnz = int(t_views.chunk_pattern()[0].sum())
    mask = three_runs(lambda: voltrix.dropout_mask(nnz, 33, 0.6, ATTN_SEED, ATTN_OFFSET), "dropout_mask H=33")
    assert mask.shape == (nnz, 2) and mask.dtype == torch.int32
    assert np.array_equal(mask.cpu().numpy().view(np.uint32), pack(keep_bits(nnz, 33, threshold_of(0.6), ATTN_SEED, ATTN_OFFSET)))
