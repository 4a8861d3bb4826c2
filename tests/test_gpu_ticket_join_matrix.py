"""GPU: the ticket join (voltrix/spmm_kernels.hpp "Ticket join") at every slab width, both 16-bit types, partial feature widths, a
partial last row block, both panel geometries and both arrival orders -- through the low-level launchers on ONE stream with a shared
ticket buffer, the way ``test_gpu_ticket_join.py::test_both_arrival_orders_on_one_stream`` runs its one shape.

Per case three steps -- window kernel first, panel kernel first, and the atomic join onto a zero fill -- that have to agree bit for
bit (two addends per element; ``cut_panel`` adds a fourth with the two combine passes swapped, the only way the panel kernel's
combine pass meets a block nothing has written) and meet the fp64 bound of test_gpu_spmm.py.  The features are rounded to the operand type up front,
so that bound is the fp32-accumulation term alone.  The ticketed steps write a NaN-filled ``out`` that sits between two runs of
sentinel words (``_guarded_nan``; test_gpu_views.py's ``_guarded`` with a wider margin): ``store_tile_sc1`` stores 16 rows x FS
columns unless its ``row < num_nodes`` and ``col < F`` guards stop it, which is at most 15 rows or FS - F columns past ``out`` --
inside the 16 * FS sentinel floats on either side.  Afterwards the ticket buffer is read back whole: error word, header, padding, and
per block exactly the value its producers leave (3: two direct producers, 2: anything else).

Shapes: FS in {32, 64, 128} with the window tile (FS, 3, 4) and the panel tile ``default_panel_tile`` picks for that width -- (32, 6, 2),
(64, 6, 2), (128, 3, 1), and (128, 4, pipelined) on 256-row panels; F in {8, FS - 8, FS}; N in {1040, 1033}: 1033 = 64 * 16 + 9, the last
block and the tail panel are partial.  ``tail``: the variant whose tail panel has shared columns, so that the panel kernel is a producer
of the partial block (stores it when it runs first, adds to it otherwise)."""
import numpy as np
import pytest
import torch

from test_gpu_spmm import _assert_close
from test_gpu_ticket_join import _case
from test_gpu_views import SENTINEL
from voltrix import capi, hybrid
from voltrix.jit_kernels.spmm import handle_unit_table

pytestmark = pytest.mark.gpu

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _cases():
    out = []
    for fs in (32, 64, 128):
        for f in (8, fs - 8, fs):
            for dtype in ("fp16", "bf16"):
                for n in (1040, 1033):
                    for name in (("hub", "cut_panel", "tail") if fs == 128 else ("hub", "tail")):
                        if name == "tail" and n == 1040:
                            continue
                        # the paired window kernel: every width at FS = 128, F = FS - 8 at the narrower slabs
                        for upw in ((1, 2) if fs == 128 or f == fs - 8 else (1,)):
                            out.append((fs, f, dtype, n, 4, name, upw))
    for f in (120, 128):     # 256-row panels: the pipelined panel kernel beside the pair
        for dtype in ("fp16", "bf16"):
            for n in (1040, 1033):
                for name in ("hub", "cut_panel"):
                    out.append((128, f, dtype, n, 2, name, 2))
    return out


CASES = _cases()
assert len(CASES) <= 150


def _guarded_nan(n, f, guard):
    """(buffer, out): ``out`` = [n, f] floats, all NaN, 16-byte aligned, with ``guard`` sentinel words on either side."""
    buf = torch.empty(guard + n * f + guard, dtype=torch.float32, device="cuda")
    buf.view(torch.int32).fill_(SENTINEL)
    out = buf[guard:guard + n * f].view(n, f)
    assert out.data_ptr() % 16 == 0 and out.is_contiguous()
    out.fill_(float("nan"))
    return buf, out


def _assert_guards_intact(buf, out, guard, what):
    words = buf.view(torch.int32)
    for side, part in (("before", words[:guard]), ("after", words[guard + out.numel():])):
        changed = torch.nonzero(part != SENTINEL).flatten()
        assert changed.numel() == 0, f"{what}: {changed.numel()} sentinel words {side} out were written, first at {int(changed[0])}"


def _expected_tickets(two, table, n):
    """Per 16-row block: 3 where the window kernel (the window is not cut) and the panel kernel (the block's panel has k-steps and is
    not cut) both write it directly, 2 everywhere else -- one direct producer, or a combine pass."""
    plan = two.plan
    blocks = (n + 15) // 16
    window_direct = np.ones(blocks, bool)
    if table.num_cuts:
        window_direct[table.cuts[:, 0].cpu().numpy()] = False
    nks = (plan.panel_ptr[1:] - plan.panel_ptr[:-1]).cpu().numpy()
    panel_direct_of = nks > 0
    if plan.parts is not None and plan.parts.num_cuts:
        panel_direct_of[plan.parts.cuts[:, 0].cpu().numpy()] = False
    panel_direct = panel_direct_of[np.arange(blocks) * 16 // plan.panel_rows]
    return np.where(window_direct & panel_direct, 3, 2).astype(np.int32), window_direct, panel_direct


@pytest.mark.parametrize("fs,f,dtype,n,row_blocks,name,units_per_wave", CASES,
                         ids=[f"FS{c[0]}-F{c[1]}-{c[2]}-N{c[3]}-rb{c[4]}-{c[5]}-u{c[6]}" for c in CASES])
def test_ticket_join_matrix(cuda_device, fs, f, dtype, n, row_blocks, name, units_per_wave):
    indptr, indices, two, feat128 = _case(name, n, row_blocks)
    plan = two.plan
    feat32 = feat128[:, :f].to(DTYPES[dtype]).float()       # the caller's data IS fp16 / bfloat16
    feat = feat32.to(DTYPES[dtype]).cuda()
    bf16 = dtype == "bf16"
    window_tile, panel_tile = (fs, 3, 4), hybrid.default_panel_tile(fs, plan.waves, plan.row_blocks)
    assert panel_tile[0] == fs and (panel_tile[2] == hybrid.KSTEPS_PIPELINED) == (row_blocks == 2)
    table = handle_unit_table(two.blk_offsets, two.hspa_packed, n, pairs=units_per_wave == 2, xcd_ptr=two.window_xcd_ptr)
    assert table.num_cuts > 0                                # the hub's window
    want, window_direct, panel_direct = _expected_tickets(two, table, n)
    assert (want == 3).any() and (want == 2).any()
    assert not window_direct[600 // 16]
    if name == "cut_panel":
        assert not panel_direct[600 // 16]                   # the hub's block is written by the combine passes alone
    if name == "tail":
        assert n % 16 != 0 and panel_direct[-1] and window_direct[-1]   # the partial block has both producers
    stream = torch.cuda.current_stream().cuda_stream
    guard = 16 * fs
    assert guard >= 15 * f + fs                              # the furthest an unguarded tile store could reach past ``out``

    def window(out, partials, tickets):
        assert capi.launch_spmm_sched(two.blk_offsets.data_ptr(), two.hspa_packed.data_ptr(), two.hind.data_ptr(), n,
                                      plan.num_resid_edges, f, feat.data_ptr(), out.data_ptr(), window_tile, stream, 0, 0,
                                      tickets is None, bf16, table, partials.data_ptr(), 0, units_per_wave,
                                      tickets=tickets.data_ptr() if tickets is not None else 0) == 0

    def step(order):
        ticketed = order != "atomic"
        buf, out = _guarded_nan(n, f, guard) if ticketed else (None, torch.zeros(n, f, device="cuda"))
        tickets = hybrid.new_tickets(n, out.device) if ticketed else None
        partials = torch.empty(max(1, table.num_slots) * 16 * f, device="cuda")
        pending = None
        for kernel in (("window", "panel") if order != "panel_first" else ("panel", "window")):
            if kernel == "window":
                window(out, partials, tickets)
            else:
                pending = hybrid.launch_panel(plan, feat, out, accumulate=3 if ticketed else 2, tile=panel_tile, defer_combine=True,
                                              tickets=tickets)
        assert (pending is not None) == (name == "cut_panel")
        if pending is not None and order == "panel_combine_first":
            pending.run()          # the hub's block (cut window, cut panel) is still unwritten: THIS pass stores it, the next adds
        assert capi.launch_combine_partials(table, partials.data_ptr(), out.data_ptr(), n, f, True, stream,
                                            tickets=tickets.data_ptr() if ticketed else 0) == 0
        if pending is not None and order != "panel_combine_first":
            pending.run()
        torch.cuda.synchronize()
        if ticketed:
            assert not torch.isnan(out).any(), order
            _assert_guards_intact(buf, out, guard, order)
            words = tickets.cpu().numpy()
            blocks = (n + 15) // 16
            assert words.size % 4 == 0 and words.size >= hybrid.TICKET_HEADER + blocks
            assert words[0] == 0, f"{order}: error word {words[0]}"
            assert not words[1:hybrid.TICKET_HEADER].any() and not words[hybrid.TICKET_HEADER + blocks:].any(), order
            got = words[hybrid.TICKET_HEADER:hybrid.TICKET_HEADER + blocks]
            assert np.array_equal(got, want), (order, np.nonzero(got != want)[0][:8], got[got != want][:8], want[got != want][:8])
        return out

    atomic, first, second = step("atomic"), step("window_first"), step("panel_first")
    assert torch.equal(first, second) and torch.equal(first, atomic)
    if name == "cut_panel":     # the combine passes the other way round (a + b == b + a): the panel kernel's pass meets a ticket of 0
        assert torch.equal(step("panel_combine_first"), first)
    _assert_close(first, indptr, indices, feat32, n, "exact" if bf16 else "fp16")


# ---- refusals: no kernel is launched --------------------------------------------------------------------------------------------------
BAD_SHAPE = 1     # kErrBadShape


def _refusal_operands(f):
    n = 1033
    indptr, indices, two, feat128 = _case("hub", n, 4)
    feat = torch.zeros(n, f, dtype=torch.float16, device="cuda")
    buf = torch.empty(n * f + 8, dtype=torch.float32, device="cuda")
    buf.view(torch.int32).fill_(SENTINEL)
    table = handle_unit_table(two.blk_offsets, two.hspa_packed, n, xcd_ptr=two.window_xcd_ptr)
    partials = torch.empty(max(1, table.num_slots) * 16 * f, device="cuda")
    return n, two, feat, buf, table, partials, hybrid.new_tickets(n, feat.device)


def _assert_untouched(buf, tickets):
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int32) == SENTINEL).all()) and not tickets.any()


@pytest.mark.parametrize("f", [136, 12], ids=["F=FS+8", "F=12"])
def test_window_launcher_refuses_widths_the_ticket_join_cannot_store(cuda_device, f):
    """More than one column slab, and a row of C that is no whole number of 16-byte operand chunks."""
    n, two, feat, buf, table, partials, tickets = _refusal_operands(f)
    rc = capi.launch_spmm_sched(two.blk_offsets.data_ptr(), two.hspa_packed.data_ptr(), two.hind.data_ptr(), n, two.plan.num_resid_edges,
                                f, feat.data_ptr(), buf.data_ptr(), (128, 3, 4), torch.cuda.current_stream().cuda_stream, 0, 0, False,
                                False, table, partials.data_ptr(), 0, 1, tickets=tickets.data_ptr())
    assert rc == BAD_SHAPE
    _assert_untouched(buf, tickets)


def test_row_maps_are_refused_before_the_library_is_called(cuda_device):
    """The ticket entry points of the library take no row map at all (``voltrix_launch_spmm_*_sched_ticket``,
    ``voltrix_launch_combine_partials_ticket``): the wrappers refuse the combination themselves, by assertion, and launch nothing."""
    n, two, feat, buf, table, partials, tickets = _refusal_operands(128)
    row_map = torch.arange(16 * ((n + 15) // 16), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    with pytest.raises(AssertionError):
        capi.launch_spmm_sched(two.blk_offsets.data_ptr(), two.hspa_packed.data_ptr(), two.hind.data_ptr(), n, two.plan.num_resid_edges,
                               128, feat.data_ptr(), buf.data_ptr(), (128, 3, 4), stream, 0, 0, False, False, table,
                               partials.data_ptr(), row_map.data_ptr(), 1, tickets=tickets.data_ptr())
    with pytest.raises(AssertionError):
        capi.launch_combine_partials(table, partials.data_ptr(), buf.data_ptr(), n, 128, True, stream, row_map=row_map.data_ptr(),
                                     tickets=tickets.data_ptr())
    _assert_untouched(buf, tickets)


@pytest.mark.parametrize("what", ["no tickets", "F > FS", "output at 4-byte alignment"])
def test_panel_launcher_refuses(cuda_device, what):
    f = 136 if what == "F > FS" else 128
    n, two, feat, buf, table, partials, tickets = _refusal_operands(f)
    out_ptr = buf.data_ptr() + (4 if what == "output at 4-byte alignment" else 0)
    assert buf.data_ptr() % 16 == 0
    rc = capi.launch_spmm_panel(two.plan, feat.data_ptr(), out_ptr, f, 3, False, (128, 3, 1), 0, torch.cuda.current_stream().cuda_stream,
                                input_rows=n, tickets=0 if what == "no tickets" else tickets.data_ptr())
    assert rc == BAD_SHAPE
    _assert_untouched(buf, tickets)
