"""GPU: the ticket join of the two-level step (voltrix/spmm_kernels.hpp "Ticket join", hybrid.join_mode) against the atomic join.

The two kernels meet in C without a zero fill: per 16-row block the first producer stores its tile, the second adds its own with
float atomics.  Two addends per element, so the result is the atomic join's bit for bit -- ``torch.equal`` treats -0.0 == 0.0, the one
difference the protocol allows.  Every case runs on a C pre-filled with NaN (a block nobody stores stays NaN and fails every check),
is held to the fp64 bound of test_gpu_spmm.py, repeated ten times, and has to leave the sticky error word of its ticket buffer at zero.

Graph (the cases of this file; test_gpu_ticket_join_matrix.py and test_gpu_ticket_join_paths.py build it at other row counts and
panel heights through ``_build``): N = 1040 rows = 65 windows; 512-row panels: two full ones and a 16-row tail panel that has no shared column at all.  F = 128
fp16, mean degree ~61, half of the edges in a band around the diagonal (+-64, +-96 in the second panel: shared columns at tau = 24),
half uniform (residual).  Rows 16..31 have no edge (a window without residual edges); rows 32..47 only reach columns nobody else in
their panel uses (a row block of a panel without a shared column).  ``hub``: row 600 reaches every column, its window is cut into
units; ``cut_panel``: the same graph with the second (longer) panel forced into two pieces, so the hub's window meets a cut panel and
its block is written by the combine passes alone."""
import numpy as np
import pytest
import torch

import voltrix
from test_gpu_spmm import _assert_close
from voltrix import capi, hybrid
from voltrix.jit_kernels.spmm import handle_unit_table
from voltrix.spmm.spmm import _operand, _run_two_level

pytestmark = pytest.mark.gpu

N, F, TAU, TAIL_TAU = 1040, 128, 24, 8
_CACHE = {}


def _graph(hub: bool, n: int = N, tail: bool = False):
    """``tail``: the rows of the last (partial) panel all reach columns 960..999, and every other row has 4 uniform edges instead of
    32, so that at ``TAIL_TAU`` the band and those columns are shared and the uniform edges stay residual."""
    rng = np.random.default_rng(7)
    rows = []
    for r in range(n):
        if 16 <= r < 32:
            rows.append(np.zeros(0, np.int64))
            continue
        if 32 <= r < 48:
            rows.append(np.sort(rng.choice(np.arange(960, n), 8, replace=False)))     # <= 16 < TAU references per column in panel 0
            continue
        half = 64 if r < 512 else 96     # the second panel's band is wider: more shared columns, more k-steps than the first
        band = rng.choice(np.arange(max(0, r - half), min(n, r + half + 1)), 32 if r < 1024 else 16, replace=False)
        far = rng.choice(900, (4 if tail else 32) if r < 1024 else 0, replace=False)     # the tail panel's rows: a short window, not cut
        if tail and r >= 1024:
            band = np.r_[band, np.arange(960, 1000)]     # n - 1024 >= TAIL_TAU references each: the tail panel has k-steps
        rows.append(np.unique(np.r_[band, far]))
    if hub:
        rows[600] = np.arange(n)         # every column: a window several times the median length, cut into units
    indptr = np.zeros(n + 1, np.int32)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, np.concatenate(rows).astype(np.int32)


def _build(name, n: int = N, row_blocks: int = 4, tag: str = None):
    """(indptr, indices, handle) of a variant, a new handle under the tuner tag ``tag``.  ``n``: 1040, or 1033 = 64 * 16 + 9 (the
    last 16-row block and the tail panel are partial); ``row_blocks``: 4 (512-row panels) or 2 (256-row panels).  Variants: ``uncut``,
    ``hub``, ``cut_panel`` (module docstring) and ``tail``: the hub graph with few uniform edges at tau = TAIL_TAU, where the tail
    panel has shared columns of its own, so that the panel kernel is a producer of the last block."""
    tail = name == "tail"
    indptr, indices = _graph(hub=name != "uncut", n=n, tail=tail)     # cut_panel: the hub's cut window lies in the cut panel
    two = voltrix.csr_preprocess_hybrid(torch.from_numpy(indptr), torch.from_numpy(indices), n, row_blocks=row_blocks,
                                        tau=TAIL_TAU if tail else TAU)
    two.hash_tag = tag or f"ticket_join_{name}" + ("" if (n, row_blocks) == (N, 4) else f"_{n}_{row_blocks}")
    panel_rows = 128 * row_blocks
    assert two.plan.panel_rows == panel_rows and two.plan.num_panels == (n + panel_rows - 1) // panel_rows == 1024 // panel_rows + 1
    assert two.plan.num_shared_edges > 0 and two.plan.num_resid_edges > 0
    nks = (two.plan.panel_ptr[1:] - two.plan.panel_ptr[:-1]).tolist()
    assert all(k > 0 for k in nks[:-1])
    assert nks[-1] > 0 if tail else nks[-1] == 0       # the tail panel (16 or 9 rows) has a shared column only in ``tail``
    if name == "cut_panel":        # forced through the plan's piece bound: the hub's (longest) panel in pieces, the shortest whole
        hub_panel = 600 // panel_rows
        assert nks[hub_panel] == max(nks)
        cap = min(nks[:-1]) if min(nks[:-1]) < nks[hub_panel] else nks[hub_panel] - 1
        two.plan.parts = hybrid.panel_parts(two.plan.panel_ptr, cap, two.plan.xcd_ptr)
        assert two.plan.parts.num_cuts > 0 and hub_panel in two.plan.parts.cuts[:, 0].tolist()
    return indptr, indices, two


def _case(name, n: int = N, row_blocks: int = 4):
    """(indptr, indices, handle, feat32) of ``_build``'s variant, built once and left unchanged."""
    key = (name, n, row_blocks)
    if key not in _CACHE:
        built = _build(name, n, row_blocks)
        torch.manual_seed(3)
        _CACHE[key] = built + (torch.randn(n, F).half().float(),)
    return _CACHE[key]


def _step(two, feat, join, monkeypatch):
    monkeypatch.setenv("VOLTRIX_TWO_LEVEL_JOIN", join)
    operand, out_scale, padded, _ = _operand(feat)
    out = torch.full((two.num_nodes, padded), float("nan"), device="cuda")
    _run_two_level(two, operand, out, out_scale)
    assert hybrid.LAST_JOIN["mode"] == join, (hybrid.LAST_JOIN["mode"], join)
    return out


@pytest.mark.parametrize("name", ["uncut", "hub", "cut_panel"])
def test_ticket_join_equals_the_atomic_join(cuda_device, name, monkeypatch):
    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "none")
    indptr, indices, two, feat32 = _case(name)
    feat = feat32.half().cuda()
    atomic = _step(two, feat, "atomic", monkeypatch)          # also the call that chooses the window kernel's tile
    if name == "hub":
        table = handle_unit_table(two.blk_offsets, two.hspa_packed, N, xcd_ptr=two.window_xcd_ptr)
        assert table.num_cuts > 0
    # variant 4, in every graph: window 1 has no residual edge (one all-zero TC block), rows 32..47 no shared column
    b1, b2 = int(two.blk_offsets[1]), int(two.blk_offsets[2])
    assert b2 - b1 == 1 and int(two.hspa_packed.view(torch.int32)[4 * b1:4 * b1 + 4].abs().sum()) == 0
    ticket = _step(two, feat, "ticket", monkeypatch)
    assert hybrid.join_error_word() == 0
    assert not torch.isnan(ticket).any()
    assert torch.equal(ticket, atomic)
    _assert_close(ticket, indptr, indices, feat32, N, "fp16")
    for _ in range(10):
        assert torch.equal(_step(two, feat, "ticket", monkeypatch), ticket)
        assert hybrid.join_error_word() == 0


@pytest.mark.parametrize("units_per_wave", [1, 2])
@pytest.mark.parametrize("name", ["hub", "cut_panel"])
def test_both_arrival_orders_on_one_stream(cuda_device, name, units_per_wave):
    """The low-level launchers on ONE stream with a shared ticket buffer: window kernel then panel kernel (the window kernel stores
    every block, the panel kernel adds) and panel kernel then window kernel (the other way round) -- the same bits, and the atomic
    join's.  ``units_per_wave`` 2: the paired window kernel the headline step runs."""
    indptr, indices, two, feat32 = _case(name)
    plan, feat = two.plan, feat32.half().cuda()
    table = handle_unit_table(two.blk_offsets, two.hspa_packed, N, pairs=units_per_wave == 2, xcd_ptr=two.window_xcd_ptr)
    stream = torch.cuda.current_stream().cuda_stream
    nnz = plan.num_resid_edges

    def window(out, partials, tickets):
        assert capi.launch_spmm_sched(two.blk_offsets.data_ptr(), two.hspa_packed.data_ptr(), two.hind.data_ptr(), N, nnz, F,
                                      feat.data_ptr(), out.data_ptr(), (128, 3, 4), stream, 0, 0, tickets is None, False, table,
                                      partials.data_ptr(), 0, units_per_wave,
                                      tickets=tickets.data_ptr() if tickets is not None else 0) == 0

    def step(order):
        ticketed = order != "atomic"
        out = torch.full((N, F), float("nan"), device="cuda") if ticketed else torch.zeros(N, F, device="cuda")
        tickets = hybrid.new_tickets(N, out.device) if ticketed else None
        partials = torch.empty(max(1, table.num_slots) * 16 * F, device="cuda")
        pending = None
        for kernel in (("window", "panel") if order != "panel_first" else ("panel", "window")):
            if kernel == "window":
                window(out, partials, tickets)
            else:
                pending = hybrid.launch_panel(plan, feat, out, accumulate=3 if ticketed else 2, defer_combine=True, tickets=tickets)
        assert capi.launch_combine_partials(table, partials.data_ptr(), out.data_ptr(), N, F, True, stream,
                                            tickets=tickets.data_ptr() if ticketed else 0) == 0
        if pending is not None:
            pending.run()
        if ticketed:
            words = tickets.cpu()
            assert int(words[0]) == 0                                              # the error word
            assert bool((words[hybrid.TICKET_HEADER:hybrid.TICKET_HEADER + (N + 15) // 16] >= 2).all())   # every block was written
        return out

    atomic, first, second = step("atomic"), step("window_first"), step("panel_first")
    assert torch.equal(first, second) and torch.equal(first, atomic)
    _assert_close(first, indptr, indices, feat32, N, "fp16")


def test_ineligible_calls_keep_the_atomic_join(cuda_device, monkeypatch):
    """F = 256 spans two column slabs of both kernels: forced ``ticket`` or not, the step takes the atomic join."""
    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "none")
    monkeypatch.setenv("VOLTRIX_TWO_LEVEL_JOIN", "ticket")
    indptr, indices, two, _ = _case("uncut")
    torch.manual_seed(5)
    feat32 = torch.randn(N, 256).half().float()
    for _ in range(2):       # the first call chooses the tile, the second knows it: FS = 128 < F either way
        out = voltrix.spmm_two_level(two, feat32.half().cuda())
        assert hybrid.LAST_JOIN["mode"] == "atomic" and hybrid.LAST_JOIN["tickets"] is None
    _assert_close(out, indptr, indices, feat32, N, "fp16")
    # the decision itself (host only): a row map, an fp32 operand, another slab width on one side, an unknown tile
    plan, op = two.plan, torch.empty(N, 128, dtype=torch.float16)
    assert hybrid.join_mode(plan, op, window_fs=128, panel_fs=128, forced="ticket") == "ticket"
    assert hybrid.join_mode(plan, op, window_fs=128, panel_fs=128, row_map=torch.zeros(1), forced="ticket") == "atomic"
    assert hybrid.join_mode(plan, op, window_fs=64, panel_fs=128, forced="ticket") == "atomic"
    assert hybrid.join_mode(plan, op, window_fs=None, panel_fs=128, forced="ticket") == "atomic"
    assert hybrid.join_mode(plan, op.float(), window_fs=128, panel_fs=128, forced="ticket") == "atomic"
    assert hybrid.join_mode(plan, op, concurrent=False, window_fs=128, panel_fs=128, forced="ticket") == "add"
    assert hybrid.join_mode(plan, op, window_fs=128, panel_fs=128, forced="atomic") == "atomic"


# ---- the one launch path: ``spmm_kernel(..., tickets=...)`` ---------------------------------------------------------------------------
def _chosen_kernel(two, feat, monkeypatch):
    """After a first (atomic) step has made the choice: the residual handle's point, the library tile and unit table it names."""
    from voltrix.jit_kernels.spmm import SCHED_PAIRS, ticket_point

    _step(two, feat, "atomic", monkeypatch)
    point = ticket_point(two.hspa_packed, feat.shape[1], feat, True)
    assert point is not None and point["SCHED"] in (4, SCHED_PAIRS)
    pairs = point["SCHED"] == SCHED_PAIRS
    table = handle_unit_table(two.blk_offsets, two.hspa_packed, N, pairs=pairs, xcd_ptr=two.window_xcd_ptr)
    return point, (point["FS"], point["DEPTH"], point["WAVES"]), table, 2 if pairs else 1


def _window_args(two, feat, out):
    return dict(num_nodes=N, num_edges=two.plan.num_resid_edges, embedding_dim=feat.shape[1], input=feat, output=out,
                atomic_out=True, beside_panel=True, defer_combine=True, xcd_ptr=two.window_xcd_ptr)


@pytest.mark.parametrize("dtype,f", [(torch.float16, 128), (torch.bfloat16, 64)], ids=["fp16-F128", "bf16-F64"])
@pytest.mark.parametrize("name", ["hub", "uncut"])
def test_jit_route_equals_the_library_route(cuda_device, name, dtype, f, monkeypatch):
    """The window kernel ALONE in the ticket join, on a NaN-filled C between sentinel words with fresh tickets: through
    ``spmm_kernel(..., tickets=...)`` and its pending combine, and through the C-ABI ticket entry points on the same cached table
    and the chosen point's tile.  Same kernel, so the same bits in C and the same ticket words."""
    from test_gpu_ticket_join_matrix import _assert_guards_intact, _guarded_nan
    from voltrix.jit_kernels.spmm import spmm_kernel, unit_scale

    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "none")
    indptr, indices, two, feat32 = _case(name)
    feat = feat32[:, :f].to(dtype).cuda()
    point, tile, table, units_per_wave = _chosen_kernel(two, feat, monkeypatch)
    assert (table.num_cuts > 0) == (name == "hub")
    guard = 16 * point["FS"]
    stream = torch.cuda.current_stream().cuda_stream

    buf_jit, out_jit = _guarded_nan(N, f, guard)
    tickets_jit = hybrid.new_tickets(N, feat.device)
    pending = spmm_kernel(two.blk_offsets, two.hspa_packed, two.hind, tickets=tickets_jit, **_window_args(two, feat, out_jit))
    assert (pending is not None) == (table.num_cuts > 0)
    if pending is not None:
        assert pending.tickets is tickets_jit
        pending.run()

    buf_lib, out_lib = _guarded_nan(N, f, guard)
    tickets_lib = hybrid.new_tickets(N, feat.device)
    partials = torch.empty(max(1, table.num_slots) * 16 * f, device="cuda")
    assert capi.launch_spmm_sched(two.blk_offsets.data_ptr(), two.hspa_packed.data_ptr(), two.hind.data_ptr(), N,
                                  two.plan.num_resid_edges, f, feat.data_ptr(), out_lib.data_ptr(), tile, stream, 0,
                                  unit_scale(feat.device).data_ptr(), False, dtype == torch.bfloat16, table, partials.data_ptr(), 0,
                                  units_per_wave, tickets=tickets_lib.data_ptr()) == 0
    accumulate, _ = hybrid.Join("ticket", tickets_lib).combine
    assert capi.launch_combine_partials(table, partials.data_ptr(), out_lib.data_ptr(), N, f, accumulate, stream,
                                        tickets=tickets_lib.data_ptr()) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(out_jit).any() and not torch.isnan(out_lib).any()
    assert torch.equal(out_jit, out_lib)
    assert torch.equal(tickets_jit, tickets_lib) and int(tickets_jit[0]) == 0
    _assert_guards_intact(buf_jit, out_jit, guard, "JIT route")
    _assert_guards_intact(buf_lib, out_lib, guard, "library route")


def test_repeated_ticket_step_uses_the_launch_plan(cuda_device, monkeypatch):
    """The first ticket step of a handle leaves a launch plan whose key carries the ticket code; the next one runs from that plan with
    a ticket tensor of its own -- the same bits, and the first call's tickets are not written again."""
    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "none")
    indptr, indices, two, feat32 = _case("hub")
    feat = feat32.half().cuda()
    _step(two, feat, "atomic", monkeypatch)
    first = _step(two, feat, "ticket", monkeypatch)
    tickets_first = hybrid.LAST_JOIN["tickets"]
    torch.cuda.synchronize()
    kept = tickets_first.clone()
    plans = two.hspa_packed._voltrix_plans
    ticket_plans = {key: plan for key, plan in plans.items() if key[6] == hybrid.WINDOW_TICKET and key[3] == F}
    assert len(ticket_plans) == 1
    second = _step(two, feat, "ticket", monkeypatch)
    tickets_second = hybrid.LAST_JOIN["tickets"]
    torch.cuda.synchronize()
    assert tickets_second is not tickets_first and tickets_second.data_ptr() != tickets_first.data_ptr()
    assert all(plans[key] is plan for key, plan in ticket_plans.items())        # launched from the plan, not rebuilt
    assert torch.equal(second, first) and not torch.isnan(second).any()
    assert torch.equal(tickets_first, kept) and torch.equal(tickets_second, kept)
    assert hybrid.join_error_word() == 0


def test_spmm_kernel_refuses_tickets_it_cannot_serve(cuda_device, monkeypatch):
    """A ticket buffer serves one launch: no ticket call before this process has chosen the kernel (it would sweep), none with a
    ``row_map``.  Nothing is launched: C and the tickets stay as they were."""
    from test_gpu_views import SENTINEL
    from voltrix.jit_kernels.spmm import spmm_kernel

    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "none")
    feat = _case("uncut")[3].half().cuda()
    out = torch.empty(N, F, device="cuda")
    out.view(torch.int32).fill_(SENTINEL)
    tickets = hybrid.new_tickets(N, feat.device)

    def assert_untouched():
        torch.cuda.synchronize()
        assert bool((out.view(torch.int32) == SENTINEL).all()) and not tickets.any()

    fresh = _build("uncut", tag="ticket_join_untuned")[2]
    fresh.hspa_packed.hash_tag = "ticket_join_untuned/residual"
    with pytest.raises(AssertionError):
        spmm_kernel(fresh.blk_offsets, fresh.hspa_packed, fresh.hind, tickets=tickets, **_window_args(fresh, feat, out))
    assert_untouched()
    two = _case("uncut")[2]
    _step(two, feat, "atomic", monkeypatch)           # chosen now
    row_map = torch.arange(16 * ((N + 15) // 16), dtype=torch.int32, device="cuda")
    with pytest.raises(AssertionError):
        spmm_kernel(two.blk_offsets, two.hspa_packed, two.hind, tickets=tickets, row_map=row_map, **_window_args(two, feat, out))
    assert_untouched()
