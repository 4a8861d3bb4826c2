"""The host-side argument contract of every entry point of libvoltrix_hip.so that launches (include/voltrix_capi.h), as ONE table: a
row per symbol of the binding that returns nothing and takes a stream and a return-code slot -- every ``voltrix_launch_*`` and
``voltrix_sample_neighbors_weighted`` --, a role per parameter, and the bad calls derived from the roles (``cases()``).
``tests/test_core_abi_host.py`` sends the cases through ``tests/core_abi_worker.py`` -- a child process that cannot see a device -- and
compares every return code; no torch, no GPU, and no test calls one of these symbols in its own process.

A row's ``params`` follow ``capi.SIGNATURES[name]`` one to one.  The roles:

    P(align)       a pointer every valid call with non-zero sizes gives at least one element: NULL is VOLTRIX_ERR_BAD_SHAPE; so is an
                   address off by less than ``align`` bytes, where the header states an alignment (None: it states none)
    O(align, ...)  an optional pointer: NULL has a documented meaning and is what the baseline passes; set, the call is still accepted
                   (``needs``: the other arguments that have to be set with it); misaligned, it is refused
    E(align)       a pointer that MAY BE EMPTY: the Python wrappers pass ``tensor.data_ptr()``, which is 0 for an empty tensor, and the
                   launcher cannot know on the host whether the array has an element (``hspa_packed`` / ``hind`` of a graph without
                   edges: the block count lives on the device in ``blk_offsets``; the edge list of a CSR without entries; a dense operand
                   whose row count is an argument).  NULL is accepted; a misaligned address is still refused
    N(v, hi, code) a size, baseline ``v``: -1 is refused; ``hi`` = its upper limit, the first value beyond it is refused with ``code``
    R(v, lo, hi)   an enum or a range: ``lo - 1`` and ``hi + 1`` are refused (None: that end is open)
    V(v)           a value without a contract of its own on the host (unused, advisory, or a default selector such as -1 / 0)
    ST, RC         the stream (NULL: the null stream) and the return-code slot

``zero``: the "nothing to do" calls and what they answer; ``extra``: everything else the launcher's code refuses -- widths off the
grid, tiles that are not instantiated, floats that are not finite, products beyond INT_MAX, combinations -- and whether a bad width,
enum or float is refused before or after "nothing to do".  Every override is ``{parameter: value}``; for a pointer the value is
``NULL``, ``SET`` (its aligned buffer), ``("off", bytes)`` or ``("same", other pointer)``.

The baseline of a row -- valid, non-zero sizes, pointers into zeroed 16-byte-aligned HOST buffers -- passes every check and reaches
the first HIP runtime call, which fails in a process without a device: VOLTRIX_ERR_LAUNCH.  ``baseline=`` names the rows that answer
something else, with the reason.
"""
OK, BAD, LAUNCH, CONFIG, OVERFLOW = 0, 1, 2, 3, 4
NULL, SET = None, "set"
INT_MAX = 2 ** 31 - 1


class Role:
    kind = "value"

    def __init__(self, value=None):
        self.value = value


class P(Role):
    kind = "pointer"

    def __init__(self, align=None, init=None):
        self.align, self.init, self.value = align, init, SET


class O(P):   # noqa: E742
    def __init__(self, align=None, needs=None):
        self.align, self.init, self.value, self.needs = align, None, NULL, dict(needs or {})


class E(P):
    pass


class N(Role):
    def __init__(self, value, hi=None, code=BAD):
        self.value, self.hi, self.code = value, hi, code


class R(Role):
    def __init__(self, value, lo=None, hi=None):
        self.value, self.lo, self.hi = value, lo, hi


class V(Role):
    pass


class _Stream(Role):
    kind = "stream"


class _Rc(Role):
    kind = "rc"


ST, RC = _Stream(), _Rc()

ROWS = {}


def row(name, params, baseline=LAUNCH, zero=(), extra=()):
    assert name not in ROWS, name
    ROWS[name] = dict(name=name, params=list(params), baseline=baseline, zero=list(zero), extra=list(extra))


def _offsets(align):
    return {16: (4, 8), 8: (4,), 4: (2,)}[align]


# ---- block-format SpMM: launch_spmm_tc16 (voltrix/spmm_kernels.hpp) behind dispatch_spmm (csrc/capi_common.hpp) ---------------------
# blk_offsets and output have an element whenever num_nodes > 0 and embedding_dim > 0, and so has input on these entry points (they take
# no input_rows: the operand has num_nodes rows or more).  hspa_packed / hind: empty for a graph without edges -- may be empty.
# Sizes are checked first, then "nothing to do" (num_nodes == 0 or embedding_dim == 0), then the width, then pointers.
def _spmm_head():
    return [("blk_offsets", P()), ("hspa_packed", E(16)), ("hind", E()), ("num_nodes", N(32)), ("num_edges", V(0)),
            ("embedding_dim", N(64)), ("input", P(16)), ("output", P())]


_SPMM_ZERO = [({"num_nodes": 0}, OK), ({"embedding_dim": 0}, OK),
              ({"num_nodes": 0, "blk_offsets": NULL, "hspa_packed": NULL, "hind": NULL, "input": NULL, "output": NULL}, OK)]


def _width(bad):   # a width off the grid is refused -- after "nothing to do": with num_nodes == 0 the same width is VOLTRIX_OK
    return [("width", {"embedding_dim": bad}, BAD), ("width_after_nothing_to_do", {"embedding_dim": bad, "num_nodes": 0}, OK)]


def _tile(fs, depth, waves):
    return [("fs", V(fs)), ("depth", V(depth)), ("waves", V(waves))]


_BAD_TILE = [("tile_not_instantiated", {"fs": 48}, CONFIG), ("tile_depth_5", {"depth": 5}, CONFIG), ("tile_waves_3", {"waves": 3}, CONFIG)]

for _name, _bad in (("voltrix_launch_spmm", 6), ("voltrix_launch_spmm_f16", 60), ("voltrix_launch_spmm_bf16", 60)):
    row(_name, _spmm_head() + [("stream", ST), ("return_code", RC)], zero=_SPMM_ZERO, extra=_width(_bad))

for _name, _bad, _t in (("voltrix_launch_spmm_f32_tile", 6, (64, 3, 1)), ("voltrix_launch_spmm_f16_tile", 60, (64, 3, 4)),
                        ("voltrix_launch_spmm_bf16_tile", 60, (64, 3, 4))):
    row(_name, _spmm_head() + _tile(*_t) + [("window_order", O()), ("out_scale", O()), ("stream", ST), ("return_code", RC)],
        zero=_SPMM_ZERO, extra=_width(_bad) + _BAD_TILE +
        ([("tile_fp32_256_wide", {"fs": 256, "depth": 2, "waves": 1}, CONFIG)] if _bad == 6 else []))

# fp32 features on the 16-bit path: the shim checks input_rows, the workspace and the width BEFORE anything else (a width of 60 is
# refused with num_nodes == 0 as well); input has input_rows rows -- an argument, so with input_rows > 0 it is required.
row("voltrix_launch_spmm_f32_as_f16",
    [("blk_offsets", P()), ("hspa_packed", E(16)), ("hind", E()), ("num_nodes", N(32)), ("num_edges", V(0)), ("embedding_dim", N(64)),
     ("input", P(16)), ("input_rows", N(32)), ("output", P()), ("workspace", P(16)), ("stream", ST), ("return_code", RC)],
    # the cast of the operand launches even for an empty operand (it writes the scale): no "nothing to do" before the runtime
    zero=[({"num_nodes": 0}, LAUNCH), ({"embedding_dim": 0}, LAUNCH), ({"input_rows": 0, "input": NULL}, LAUNCH)],
    extra=[("width", {"embedding_dim": 60}, BAD), ("width_before_nothing_to_do", {"embedding_dim": 60, "num_nodes": 0}, BAD),
           ("null_workspace_before_nothing_to_do", {"workspace": NULL, "num_nodes": 0}, BAD)])

# schedule / output extensions.  units: replaces window_order, needs unit_ptr; partials: only read for units with a slot (the table
# lives on the device) -- optional; units_per_wave: "ignored where it does not apply".
_UNITS = {"unit_ptr": SET, "max_units_per_xcd": 4}
for _name in ("voltrix_launch_spmm_f16_sched", "voltrix_launch_spmm_bf16_sched"):
    row(_name, _spmm_head() + _tile(64, 3, 4) +
        [("window_order", O()), ("out_scale", O()), ("atomic_out", R(0, 0, 2)), ("units", O(16, _UNITS)), ("unit_ptr", O()),
         ("max_units_per_xcd", V(0)), ("partials", O(needs=_UNITS | {"units": SET})), ("row_map", O()), ("units_per_wave", V(1)),
         ("stream", ST), ("return_code", RC)],
        zero=_SPMM_ZERO + [({"units": SET, "unit_ptr": SET, "max_units_per_xcd": 0}, OK)],   # a table without units on any XCD
        extra=_width(60) + _BAD_TILE + [
            ("atomic_out_1", {"atomic_out": 1}, LAUNCH),
            # atomic_out = 2 is the ticket join: this entry point has no ticket buffer to give it
            ("ticket_join_without_tickets", {"atomic_out": 2}, BAD),
            ("units_without_unit_ptr", {"units": SET, "max_units_per_xcd": 4}, BAD),
            ("units_negative_count", {"units": SET, "unit_ptr": SET, "max_units_per_xcd": -1}, BAD),
            ("units_per_wave_2", {"units": SET, "unit_ptr": SET, "max_units_per_xcd": 4, "units_per_wave": 2}, LAUNCH)])

# ticket join, window kernel: one column slab (embedding_dim <= fs), tickets and output 16-byte aligned
for _name in ("voltrix_launch_spmm_f16_sched_ticket", "voltrix_launch_spmm_bf16_sched_ticket"):
    row(_name, [("blk_offsets", P()), ("hspa_packed", E(16)), ("hind", E()), ("num_nodes", N(32)), ("num_edges", V(0)),
                ("embedding_dim", N(64)), ("input", P(16)), ("output", P(16))] + _tile(64, 3, 4) +
        [("out_scale", O()), ("units", O(16, _UNITS)), ("unit_ptr", O()), ("max_units_per_xcd", V(0)),
         ("partials", O(needs=_UNITS | {"units": SET})), ("units_per_wave", V(1)), ("tickets", P(16)), ("stream", ST),
         ("return_code", RC)],
        zero=_SPMM_ZERO,
        extra=_width(60) + _BAD_TILE + [
            ("wider_than_the_slab", {"embedding_dim": 128}, BAD),
            ("as_wide_as_the_slab", {"embedding_dim": 128, "fs": 128}, LAUNCH),
            ("units_without_unit_ptr", {"units": SET, "max_units_per_xcd": 4}, BAD)])

# combine pass of the unit table: the width is checked with the sizes, BEFORE "nothing to do"
_COMBINE_ZERO = [({"num_cuts": 0}, OK), ({"num_nodes": 0}, OK), ({"embedding_dim": 0}, OK),
                 ({"num_cuts": 0, "cuts": NULL, "partials": NULL, "output": NULL}, OK)]
row("voltrix_launch_combine_partials",
    [("cuts", P(16)), ("num_cuts", N(2)), ("partials", P(16)), ("output", P(16)), ("num_nodes", N(32)), ("embedding_dim", N(64)),
     ("accumulate", V(0)), ("row_map", O()), ("stream", ST), ("return_code", RC)],
    zero=_COMBINE_ZERO,
    extra=[("width", {"embedding_dim": 6}, BAD), ("width_before_nothing_to_do", {"embedding_dim": 6, "num_cuts": 0}, BAD),
           ("accumulate_1", {"accumulate": 1}, LAUNCH)])
row("voltrix_launch_combine_partials_ticket",
    [("cuts", P(16)), ("num_cuts", N(2)), ("partials", P(16)), ("output", P(16)), ("num_nodes", N(32)), ("embedding_dim", N(64)),
     ("tickets", P(16)), ("stream", ST), ("return_code", RC)],
    zero=_COMBINE_ZERO,
    extra=[("width", {"embedding_dim": 6}, BAD), ("width_before_nothing_to_do", {"embedding_dim": 6, "num_cuts": 0}, BAD),
           ("null_tickets_before_nothing_to_do", {"tickets": NULL, "num_cuts": 0}, BAD)])

row("voltrix_launch_window_order",
    [("blk_offsets", P()), ("num_nodes", N(32)), ("chunk", R(64, 1, 4096)), ("order_out", P()), ("stream", ST), ("return_code", RC)],
    zero=[({"num_nodes": 0}, OK), ({"num_nodes": 0, "blk_offsets": NULL, "order_out": NULL}, OK)],
    extra=[("chunk_before_nothing_to_do", {"chunk": 0, "num_nodes": 0}, BAD)])

# ---- casts and row scaling (spmm_kernels.hpp) ------------------------------------------------------------------------------------------
row("voltrix_launch_cast_f32_f16", [("src", P(16)), ("dst", P(16)), ("count", N(64)), ("stream", ST), ("return_code", RC)],
    zero=[({"count": 0}, OK), ({"count": 0, "src": NULL, "dst": NULL}, OK)],
    extra=[("count_not_a_multiple_of_8", {"count": 60}, BAD)])
# the scaled cast writes the scale even for count == 0 (scale 1): it launches, and only src / dst may then be NULL; scale: 8 bytes
row("voltrix_launch_cast_f32_f16_scaled",
    [("src", P(16)), ("dst", P(16)), ("count", N(64)), ("scale", P(8)), ("stream", ST), ("return_code", RC)],
    zero=[({"count": 0}, LAUNCH), ({"count": 0, "src": NULL, "dst": NULL}, LAUNCH)],
    extra=[("count_not_a_multiple_of_8", {"count": 60}, BAD), ("null_scale_with_nothing_to_cast", {"count": 0, "scale": NULL}, BAD)])
row("voltrix_launch_scale_rows",
    [("src", P(16)), ("scale", P(4)), ("dst", P(16)), ("rows", N(4)), ("num_feats", N(16)), ("dtype", R(1, 0, 2)), ("stream", ST),
     ("return_code", RC)],
    zero=[({"rows": 0}, OK), ({"num_feats": 0}, OK), ({"rows": 0, "src": NULL, "scale": NULL, "dst": NULL}, OK)],
    extra=[("width_16_bit", {"num_feats": 12}, BAD), ("width_fp32", {"num_feats": 6, "dtype": 0}, BAD),
           ("width_before_nothing_to_do", {"num_feats": 12, "rows": 0}, BAD), ("dtype_before_nothing_to_do", {"dtype": 3, "rows": 0}, BAD),
           ("dst_is_src", {"dst": ("same", "src")}, LAUNCH)])

# ---- CSR row-gather kernel and the value scatter (spmm_csr_kernels.hpp) --------------------------------------------------------------
# indices (and values) of a CSR without entries are empty; the header states 4-byte alignment for indptr, indices and values
_CSR_ROWS = [("num_rows", N(4)), ("embedding_dim", N(8)), ("input", P(16)), ("dtype", R(0, 0, 2)), ("output", P(16)),
             ("xcd_ranges", V(0)), ("stream", ST), ("return_code", RC)]
_CSR_ZERO = [({"num_rows": 0}, OK), ({"embedding_dim": 0}, OK)]
_CSR_EXTRA = [("width_fp32", {"embedding_dim": 6}, BAD), ("width_16_bit", {"embedding_dim": 12, "dtype": 1}, BAD),
              ("width_after_nothing_to_do", {"embedding_dim": 6, "num_rows": 0}, OK),
              ("dtype_before_nothing_to_do", {"dtype": 3, "num_rows": 0}, BAD), ("xcd_ranges_1", {"xcd_ranges": 1}, LAUNCH)]
row("voltrix_launch_spmm_csr_rows", [("indptr", P(4)), ("indices", E(4))] + _CSR_ROWS,
    zero=_CSR_ZERO + [({"num_rows": 0, "indptr": NULL, "indices": NULL, "input": NULL, "output": NULL}, OK)], extra=_CSR_EXTRA)
# values: the shim refuses NULL before anything else (NULL would select the binary kernel), "nothing to do" included
row("voltrix_launch_spmm_csr_rows_weighted", [("indptr", P(4)), ("indices", E(4)), ("values", P(4))] + _CSR_ROWS,
    zero=_CSR_ZERO, extra=_CSR_EXTRA + [("null_values_before_nothing_to_do", {"values": NULL, "num_rows": 0}, BAD)])
row("voltrix_launch_scatter_values",
    [("values", P()), ("slots", P()), ("plane", P()), ("count", N(8)), ("dtype", R(1, 0, 2)), ("stream", ST), ("return_code", RC)],
    zero=[({"count": 0}, OK), ({"count": 0, "values": NULL, "slots": NULL, "plane": NULL}, OK)],
    extra=[("dtype_before_nothing_to_do", {"dtype": 3, "count": 0}, BAD)])

# ---- the reference's preprocess (bmat_kernels.hpp) -------------------------------------------------------------------------------------
# voltrix_launch_preprocess is HOST code on HOST arrays: the baseline (four rows without edges: node_pointer all zero) runs to the end
# and answers VOLTRIX_OK.  The three per-edge arrays are empty for a graph without edges.
row("voltrix_launch_preprocess",
    [("edge_list", E()), ("node_pointer", P()), ("num_nodes", N(4)), ("block_partition", P()), ("edge_to_column", E()),
     ("edge_to_row", E()), ("pointer1", P()), ("return_code", RC)],
    baseline=OK, zero=[({"num_nodes": 0}, OK), ({"num_nodes": 0, "node_pointer": NULL, "block_partition": NULL}, OK)],
    extra=[("null_pointer1_with_nothing_to_do", {"num_nodes": 0, "pointer1": NULL}, BAD)])   # pointer1[0] is always written
# node_pointer and block_partition are not used by the launcher (the reference's list); the per-edge arrays are read when num_edges > 0
row("voltrix_launch_hmat_gen",
    [("node_pointer", E()), ("edge_list", P()), ("block_partition", E()), ("edge_to_column", P()), ("edge_to_row", P()),
     ("pointer1", P()), ("num_row_windows", N(2)), ("num_nodes", N(32)), ("num_edges", N(8)), ("hspa", P(16)), ("hind", P(16)),
     ("return_code", RC)],
    zero=[({"num_row_windows": 0}, OK), ({"num_edges": 0, "edge_list": NULL, "edge_to_column": NULL, "edge_to_row": NULL}, LAUNCH)])
row("voltrix_launch_hmat_packed_swizzle",
    [("num_row_windows", N(2)), ("pointer1", P()), ("hspa", P()), ("hspa_packed", P(16)), ("return_code", RC)],
    zero=[({"num_row_windows": 0}, OK), ({"num_row_windows": 0, "pointer1": NULL, "hspa": NULL, "hspa_packed": NULL}, OK)])

# ---- fused GPU preprocess (csr_preprocess.hpp) -----------------------------------------------------------------------------------------
# edge_list: empty for a CSR without entries.  workspace: its size comes from a size function of (sizes, path) that the caller evaluates;
# hspa_packed / hind: as for the SpMM launchers.  status / pointer1 are written even for num_nodes == 0 (a memset: the runtime).
# num_edges + windows must fit the int32 handle: VOLTRIX_ERR_OVERFLOW.
_CSR_SIZES = [("num_nodes", N(32, 1 << 28)), ("num_cols", V(32)), ("num_edges", N(8, INT_MAX - 2, OVERFLOW)), ("path", V(-1))]
row("voltrix_launch_csr_window_count",
    [("node_pointer", P()), ("edge_list", E())] + _CSR_SIZES +
    [("workspace", E(16)), ("block_partition", P()), ("pointer1", P()), ("status", P()), ("stream", ST), ("return_code", RC)],
    zero=[({"num_nodes": 0}, LAUNCH), ({"num_nodes": 0, "node_pointer": NULL, "block_partition": NULL}, LAUNCH)],
    extra=[("num_cols_above_2_28", {"num_cols": (1 << 28) + 1}, BAD), ("num_cols_unknown", {"num_cols": 0}, LAUNCH),
           ("null_status_with_nothing_to_do", {"num_nodes": 0, "status": NULL}, BAD)])
# the fill phase at num_nodes = 2^28 itself is not sent: the path chosen there raises a kernel's LDS limit first, and without a device
# that runtime call answers VOLTRIX_ERR_BAD_CONFIG -- the first value beyond the limit is refused all the same
row("voltrix_launch_csr_fill",
    [("node_pointer", P()), ("edge_list", E()), ("num_nodes", N(32))] + _CSR_SIZES[1:] +
    [("workspace", E(16)), ("pointer1", P()), ("hspa_packed", E(16)), ("hind", E(16)), ("stream", ST), ("return_code", RC)],
    zero=[({"num_nodes": 0}, OK), ({"num_nodes": 0, "node_pointer": NULL, "pointer1": NULL}, OK)],
    extra=[("num_nodes_above_2_28", {"num_nodes": (1 << 28) + 1}, BAD)])

# ---- unit table, stream table, XCD ranges, piece table (unit_table.hpp, stream_table.hpp, schedule_tables.hpp) -----------------------
# The count phases clear the header first (a memset: the runtime), so num_nodes == 0 does not answer without one.  cuts / runs: a table
# without a cut window has no row of cuts.
row("voltrix_launch_unit_table_count",
    [("blk_offsets", P()), ("num_nodes", N(32, 1 << 28)), ("max_stages", V(0)), ("xcd_ptr", O()), ("workspace", P(16)), ("header", P()),
     ("stream", ST), ("return_code", RC)],
    zero=[({"num_nodes": 0}, LAUNCH), ({"num_nodes": 0, "blk_offsets": NULL}, LAUNCH)])
row("voltrix_launch_unit_table_fill",
    [("blk_offsets", P()), ("num_nodes", N(32, 1 << 28)), ("xcd_ptr", O()), ("workspace", P(16)), ("fill_workspace", P(16)),
     ("num_units", N(2)), ("num_cuts", N(0)), ("top", N(4)), ("units", P(16)), ("unit_ptr", P()), ("cuts", E(16)), ("stream", ST),
     ("return_code", RC)],
    zero=[({"num_nodes": 0}, LAUNCH), ({"num_units": 0, "units": NULL, "fill_workspace": NULL, "blk_offsets": NULL}, LAUNCH)],
    extra=[("null_unit_ptr_with_nothing_to_do", {"num_units": 0, "unit_ptr": NULL}, BAD)])
row("voltrix_launch_stream_table_count",
    [("blk_offsets", P()), ("hspa_packed", E(16)), ("hind", E(16)), ("num_nodes", N(32, 1 << 28)), ("run_cost", R(0, None, 128)),
     ("cut_stages", V(0)), ("workspace", P(16)), ("header", P()), ("stream", ST), ("return_code", RC)],
    zero=[({"num_nodes": 0}, LAUNCH), ({"num_nodes": 0, "blk_offsets": NULL}, LAUNCH)])
row("voltrix_launch_stream_table_fill",
    [("blk_offsets", P()), ("num_nodes", N(32, 1 << 28)), ("workspace", P(16)), ("fill_workspace", P(16)), ("num_units", N(2)),
     ("num_cuts", V(0)), ("run_bound", N(2)), ("run_cost", R(6, 2, 128)), ("units", P(16)), ("cuts", E(16)), ("runs", E(16)),
     ("run_ptr", P()), ("header2", P()), ("stream", ST), ("return_code", RC)],
    zero=[({"num_nodes": 0}, LAUNCH), ({"num_units": 0, "units": NULL, "fill_workspace": NULL, "blk_offsets": NULL}, LAUNCH)])

# the range builders launch for n == 0 as well (they write all nine elements of xcd_ptr)
row("voltrix_launch_xcd_ranges_of_work",
    [("work", P()), ("num_items", N(8)), ("align", R(1, 1, None)), ("xcd_ptr", P()), ("stream", ST), ("return_code", RC)],
    zero=[({"num_items": 0}, LAUNCH), ({"num_items": 0, "work": NULL}, LAUNCH)])
row("voltrix_launch_xcd_ranges_of_windows",
    [("blk_offsets", P()), ("num_nodes", N(32)), ("align", R(1, 1, None)), ("xcd_ptr", P()), ("stream", ST), ("return_code", RC)],
    zero=[({"num_nodes": 0}, LAUNCH), ({"num_nodes": 0, "blk_offsets": NULL}, LAUNCH)])
row("voltrix_launch_xcd_ranges_of_panels",
    [("panel_ptr", P()), ("resid_blk_offsets", P()), ("num_nodes", N(512)), ("panel_rows", R(128, 16, None)), ("kstep_cost_x10", N(66)),
     ("xcd_ptr", P()), ("window_xcd_ptr", O()), ("stream", ST), ("return_code", RC)],
    zero=[({"num_nodes": 0}, LAUNCH), ({"num_nodes": 0, "panel_ptr": NULL, "resid_blk_offsets": NULL}, LAUNCH)],
    extra=[("panel_rows_not_whole_windows", {"panel_rows": 24}, BAD)])
row("voltrix_launch_panel_parts_count",
    [("panel_ptr", P()), ("num_panels", N(4)), ("cap", R(8, 1, None)), ("panel_xcd_ptr", O()), ("workspace", P(16)), ("header", P()),
     ("stream", ST), ("return_code", RC)],
    zero=[({"num_panels": 0}, LAUNCH), ({"num_panels": 0, "panel_ptr": NULL}, LAUNCH)])
row("voltrix_launch_panel_parts_fill",
    [("panel_ptr", P()), ("num_panels", N(4)), ("cap", R(8, 1, None)), ("panel_xcd_ptr", O()), ("workspace", P(16)), ("parts", P()),
     ("part_xcd_ptr", P()), ("cuts", E()), ("stream", ST), ("return_code", RC)],
    zero=[({"num_panels": 0}, LAUNCH), ({"num_panels": 0, "panel_ptr": NULL, "parts": NULL}, LAUNCH)])

# ---- stream kernel (spmm_stream_kernels.hpp) -------------------------------------------------------------------------------------------
# input: input_rows is an argument (0: num_nodes) and a rectangular operator without columns has an empty operand -- may be empty.
# partials: only the units of cut windows write them.  fs == 0 selects the default tile.
for _name in ("voltrix_launch_spmm_stream_f16", "voltrix_launch_spmm_stream_bf16"):
    row(_name,
        [("hspa_packed", E(16)), ("hind", E()), ("num_nodes", N(32)), ("embedding_dim", N(64)), ("input", E(16)), ("input_rows", V(0)),
         ("output", P(16)), ("units", P(16)), ("runs", P(16)), ("run_ptr", P()), ("max_runs_per_xcd", N(1)), ("partials", O(16)),
         ("out_scale", O())] + _tile(0, 0, 0) + [("slab_policy", V(-1)), ("stream", ST), ("return_code", RC)],
        zero=[({"num_nodes": 0}, OK), ({"embedding_dim": 0}, OK), ({"max_runs_per_xcd": 0}, OK),
              ({"num_nodes": 0, "output": NULL, "units": NULL, "runs": NULL, "run_ptr": NULL}, OK)],
        extra=_width(60) + [("explicit_tile", {"fs": 64, "depth": 2, "waves": 1}, LAUNCH),
                            ("tile_not_instantiated", {"fs": 48, "depth": 2, "waves": 1}, CONFIG),
                            ("tile_waves_4", {"fs": 64, "depth": 2, "waves": 4}, CONFIG),
                            ("tile_before_nothing_to_do", {"fs": 48, "depth": 2, "waves": 1, "num_nodes": 0}, CONFIG),
                            ("slab_launches", {"embedding_dim": 256, "slab_policy": 1}, LAUNCH)])

# ---- panel kernel (spmm_panel_kernels.hpp) ---------------------------------------------------------------------------------------------
# the plan arrays are padded by the builder (panel_cols by two k-steps, panel_bits by one), so none of them is ever empty.  input: as for
# the stream kernel.  xcd_ptr needs the length of its longest range, 1 .. number of launch positions.
_PANEL_TILE = [("fs", V(128)), ("depth", V(4)), ("waves", V(8)), ("row_blocks", V(4)), ("ksteps", V(1))]
_PANEL_BAD_TILE = [("tile_not_instantiated", {"fs": 48}, CONFIG), ("tile_row_blocks_3", {"row_blocks": 3}, CONFIG),
                   ("tile_ksteps_3", {"ksteps": 3}, CONFIG), ("tile_pipelined", {"ksteps": 17}, LAUNCH),
                   ("tile_before_nothing_to_do", {"fs": 48, "num_nodes": 0}, CONFIG)]
_PANEL_ZERO = [({"num_nodes": 0}, OK), ({"embedding_dim": 0}, OK),
               ({"num_nodes": 0, "panel_ptr": NULL, "panel_cols": NULL, "panel_bits": NULL, "input": NULL, "output": NULL}, OK)]
# 1024 rows = two panels of 512: max_panels_per_xcd may be 1 or 2
_PANEL_XCD = [("xcd_ptr_without_a_range_length", {"xcd_ptr": SET}, BAD),
              ("xcd_ptr_range_longer_than_the_launch", {"xcd_ptr": SET, "max_panels_per_xcd": 3}, BAD),
              ("xcd_ptr_negative_range_length", {"xcd_ptr": SET, "max_panels_per_xcd": -1}, BAD)]
for _name in ("voltrix_launch_spmm_panel_f16", "voltrix_launch_spmm_panel_bf16"):
    row(_name,
        [("panel_ptr", P()), ("panel_cols", P()), ("panel_bits", P()), ("panel_order", O()),
         ("xcd_ptr", O(needs={"max_panels_per_xcd": 2})), ("max_panels_per_xcd", V(0)), ("num_nodes", N(1024)), ("embedding_dim", N(128)),
         ("input", E(16)), ("input_rows", V(0)), ("output", P()), ("accumulate", R(0, 0, 2))] + _PANEL_TILE +
        [("slab_policy", V(-1)), ("out_scale", O()), ("stream", ST), ("return_code", RC)],
        zero=_PANEL_ZERO,
        extra=_width(60) + _PANEL_BAD_TILE + _PANEL_XCD + [
            ("accumulate_1", {"accumulate": 1}, LAUNCH), ("accumulate_2", {"accumulate": 2}, LAUNCH),
            ("accumulate_before_nothing_to_do", {"accumulate": 3, "num_nodes": 0}, BAD)])
_PARTS_XCD = [("xcd_ptr_without_a_range_length", {"xcd_ptr": SET}, BAD),
              ("xcd_ptr_range_longer_than_the_launch", {"xcd_ptr": SET, "max_parts_per_xcd": 4}, BAD)]
for _name in ("voltrix_launch_spmm_panel_parts_f16", "voltrix_launch_spmm_panel_parts_bf16"):
    row(_name,
        [("panel_ptr", P()), ("panel_cols", P()), ("panel_bits", P()), ("parts", P()), ("num_parts", R(3, 1, None)),
         ("xcd_ptr", O(needs={"max_parts_per_xcd": 3})), ("max_parts_per_xcd", V(0)), ("partials", O()), ("num_nodes", N(1024)),
         ("embedding_dim", N(128)), ("input", E(16)), ("input_rows", V(0)), ("output", P()), ("accumulate", R(0, 0, 2))] + _PANEL_TILE +
        [("slab_policy", V(-1)), ("out_scale", O()), ("stream", ST), ("return_code", RC)],
        zero=[({"num_nodes": 0}, OK), ({"embedding_dim": 0}, OK)],
        extra=_width(60) + _PANEL_BAD_TILE + _PARTS_XCD + [
            ("null_parts_before_nothing_to_do", {"parts": NULL, "num_nodes": 0}, BAD),
            ("num_parts_before_nothing_to_do", {"num_parts": 0, "num_nodes": 0}, BAD)])
for _name in ("voltrix_launch_spmm_panel_ticket_f16", "voltrix_launch_spmm_panel_ticket_bf16"):
    row(_name,
        [("panel_ptr", P()), ("panel_cols", P()), ("panel_bits", P()), ("panel_order", O()),
         ("parts", O(needs={"num_parts": 3})), ("num_parts", V(0)), ("xcd_ptr", O(needs={"max_per_xcd": 2})), ("max_per_xcd", V(0)),
         ("partials", O()), ("tickets", P(16)), ("num_nodes", N(1024)), ("embedding_dim", N(128)), ("input", E(16)), ("input_rows", V(0)),
         ("output", P(16))] + _PANEL_TILE + [("slab_policy", V(-1)), ("out_scale", O()), ("stream", ST), ("return_code", RC)],
        zero=_PANEL_ZERO,
        extra=_width(60) + _PANEL_BAD_TILE + [
            ("wider_than_the_slab", {"embedding_dim": 256}, BAD),
            ("wider_than_the_slab_before_nothing_to_do", {"embedding_dim": 256, "num_nodes": 0}, BAD),
            ("null_tickets_before_nothing_to_do", {"tickets": NULL, "num_nodes": 0}, BAD),
            ("parts_without_a_count", {"parts": SET}, BAD),
            ("xcd_ptr_without_a_range_length", {"xcd_ptr": SET}, BAD),
            ("xcd_ptr_range_longer_than_the_pieces", {"xcd_ptr": SET, "parts": SET, "num_parts": 3, "max_per_xcd": 4}, BAD)])

# combine pass of the piece table: sizes and panel_rows first, then "nothing to do", then the width and the pointers
_PCOMBINE = [("cuts", P()), ("num_cuts", N(2)), ("partials", P()), ("output", P()), ("num_nodes", N(1024)), ("embedding_dim", N(128)),
             ("panel_rows", R(512, 16, None))]
_PCOMBINE_ZERO = [({"num_cuts": 0}, OK), ({"num_nodes": 0}, OK), ({"embedding_dim": 0}, OK),
                  ({"num_cuts": 0, "cuts": NULL, "partials": NULL, "output": NULL}, OK)]
_PCOMBINE_EXTRA = [("width", {"embedding_dim": 6}, BAD), ("width_after_nothing_to_do", {"embedding_dim": 6, "num_cuts": 0}, OK),
                   ("panel_rows_not_whole_windows", {"panel_rows": 24}, BAD),
                   ("panel_rows_before_nothing_to_do", {"panel_rows": 24, "num_cuts": 0}, BAD)]
row("voltrix_launch_combine_panel_partials", _PCOMBINE + [("accumulate", V(0)), ("stream", ST), ("return_code", RC)],
    zero=_PCOMBINE_ZERO, extra=_PCOMBINE_EXTRA + [("accumulate_1", {"accumulate": 1}, LAUNCH)])
row("voltrix_launch_combine_panel_partials_ticket", _PCOMBINE + [("tickets", P(16)), ("stream", ST), ("return_code", RC)],
    zero=_PCOMBINE_ZERO, extra=_PCOMBINE_EXTRA + [("null_tickets_before_nothing_to_do", {"tickets": NULL, "num_cuts": 0}, BAD)])

row("voltrix_launch_panel_order",
    [("panel_ptr", P()), ("num_panels", N(4)), ("group", R(1, 1, None)), ("xcd_ptr", O()), ("order_out", P()), ("stream", ST),
     ("return_code", RC)],
    zero=[({"num_panels": 0}, OK), ({"num_panels": 0, "panel_ptr": NULL, "order_out": NULL}, OK)],
    extra=[("group_before_nothing_to_do", {"group": 0, "num_panels": 0}, BAD)])

# ---- panel plan builder (panel_plan.hpp) -----------------------------------------------------------------------------------------------
# edge_list / resid_edge_list: empty without entries / without residual entries.  Both phases write through their output pointers with
# memsets before "nothing to do".  A universe above 2^22 columns: VOLTRIX_ERR_BAD_CONFIG.
_PLAN = [("node_pointer", P()), ("edge_list", E()), ("num_nodes", N(32)), ("num_cols", N(32, 1 << 22, CONFIG)),
         ("num_edges", N(8, INT_MAX)), ("waves", R(8, 4, 8)), ("row_blocks", R(4, 2, 4)), ("tau", R(2, 1, 65535)), ("workspace", P(16))]
_PLAN_EXTRA = [("waves_6", {"waves": 6}, BAD), ("row_blocks_3", {"row_blocks": 3}, BAD)]
row("voltrix_launch_panel_plan_count",
    _PLAN + [("panel_ptr", P()), ("resid_node_pointer", P()), ("status", P()), ("stream", ST), ("return_code", RC)],
    zero=[({"num_nodes": 0}, LAUNCH), ({"num_nodes": 0, "node_pointer": NULL}, LAUNCH)], extra=_PLAN_EXTRA)
row("voltrix_launch_panel_plan_fill",
    _PLAN + [("panel_ptr", P()), ("resid_node_pointer", P()), ("total_ksteps", N(3)), ("resid_edge_list", E()), ("panel_cols", P()),
             ("panel_bits", P()), ("stream", ST), ("return_code", RC)],
    zero=[({"num_nodes": 0}, LAUNCH), ({"num_nodes": 0, "node_pointer": NULL}, LAUNCH)], extra=_PLAN_EXTRA)

# ---- the two-level format in one launch and its record builder (spmm_fused_kernels.hpp, fused_plan.hpp) ------------------------------
# no input_rows: a square entry point, input is required.  pace_blocks is clamped, not refused.
for _name in ("voltrix_launch_spmm_fused_f16", "voltrix_launch_spmm_fused_bf16"):
    row(_name,
        [("panel_ptr", P()), ("panel_cols", P()), ("panel_bits", P()), ("panel_order", O()),
         ("xcd_ptr", O(needs={"max_panels_per_xcd": 2})), ("max_panels_per_xcd", V(0)), ("wave_ptr", P()), ("records", P(16)),
         ("num_nodes", N(1024)), ("embedding_dim", N(128)), ("input", P(16)), ("output", P()), ("fs", V(128)), ("depth", V(3)),
         ("pace_blocks", V(0)), ("out_scale", O()), ("stream", ST), ("return_code", RC)],
        zero=[({"num_nodes": 0}, OK), ({"embedding_dim": 0}, OK),
              ({"num_nodes": 0, "panel_ptr": NULL, "panel_cols": NULL, "panel_bits": NULL, "wave_ptr": NULL, "records": NULL,
                "input": NULL, "output": NULL}, OK)],
        extra=_width(60) + _PANEL_XCD + [("tile_not_instantiated", {"fs": 48}, CONFIG), ("tile_depth_4_at_128", {"depth": 4}, CONFIG),
                                         ("tile_before_nothing_to_do", {"fs": 48, "num_nodes": 0}, CONFIG),
                                         ("pace_blocks_negative", {"pace_blocks": -1}, LAUNCH)])
# wave_ptr[0] and the padding record are written before "nothing to do" (memsets)
row("voltrix_launch_fused_records_count",
    [("blk_offsets", P()), ("hspa_packed", E(16)), ("num_nodes", N(32)), ("workspace", P(16)), ("wave_ptr", P()), ("stream", ST),
     ("return_code", RC)],
    zero=[({"num_nodes": 0}, LAUNCH), ({"num_nodes": 0, "blk_offsets": NULL, "workspace": NULL}, LAUNCH)],
    extra=[("null_wave_ptr_with_nothing_to_do", {"num_nodes": 0, "wave_ptr": NULL}, BAD)])
row("voltrix_launch_fused_records_fill",
    [("blk_offsets", P()), ("hspa_packed", E(16)), ("hind", E()), ("num_nodes", N(32)), ("wave_ptr", P()), ("num_records", N(2)),
     ("records", P(16)), ("stream", ST), ("return_code", RC)],
    zero=[({"num_nodes": 0}, LAUNCH), ({"num_records": 0, "blk_offsets": NULL, "wave_ptr": NULL}, LAUNCH)],
    extra=[("null_records_with_nothing_to_do", {"num_records": 0, "records": NULL}, BAD)])

# ---- reorder (reorder_kernels.hpp) -----------------------------------------------------------------------------------------------------
# transpose: with entries every array has an element; t_indptr (num_cols + 1 elements) always has.  The column bounds are launched for
# num_edges == 0 as well.  The workspace is 16-byte aligned (header).
row("voltrix_launch_csr_transpose",
    [("indptr", P()), ("indices", P()), ("num_rows", N(4)), ("num_cols", N(4)), ("num_edges", N(8, INT_MAX)), ("workspace", P(16)),
     ("t_indptr", P()), ("t_indices", P()), ("stream", ST), ("return_code", RC)],
    zero=[({"num_edges": 0}, LAUNCH), ({"num_edges": 0, "indptr": NULL, "indices": NULL, "workspace": NULL, "t_indices": NULL}, LAUNCH),
          ({"num_rows": 0, "num_cols": 0, "num_edges": 0}, LAUNCH)],
    extra=[("null_t_indptr_without_entries", {"num_edges": 0, "t_indptr": NULL}, BAD)])
row("voltrix_launch_bfs_seed",
    [("start", R(0, 0, 31)), ("num_nodes", N(32)), ("level", P()), ("queue", P()), ("ctrl", P()), ("level_off", P()), ("stream", ST),
     ("return_code", RC)],
    zero=[({"num_nodes": 0}, BAD)])    # no node to start from
# indices / t_indices: empty without entries; t_indptr has t_rows + 1 elements
_BFS = [("indptr", P()), ("indices", E()), ("t_indptr", P()), ("t_indices", E()), ("num_nodes", R(32, 1, None)), ("t_rows", N(32))]
row("voltrix_launch_bfs_levels",
    _BFS + [("level", P()), ("queue", P()), ("ctrl", P()), ("level_off", P()), ("wide_levels", N(1)), ("stream", ST), ("return_code", RC)],
    zero=[({"wide_levels": 0}, LAUNCH), ({"t_rows": 0}, LAUNCH)])
# level_off_host is read on the HOST: {0, 1, ...}; the workspace is only used for levels above 1024 nodes
row("voltrix_launch_cm_rank",
    _BFS + [("level", P()), ("rank", P()), ("tie", P()), ("queue", P()), ("level_off", P()), ("level_off_host", P(init=[0, 1, 3, 6])),
            ("num_levels", R(3, 1, None)), ("base", V(0)), ("workspace", O()), ("stream", ST), ("return_code", RC)],
    extra=[("one_level", {"num_levels": 1}, LAUNCH)])
row("voltrix_launch_chol_inv_transposed",
    [("gram", P()), ("k", R(8, 1, 64)), ("eps", V(1e-10)), ("out", P()), ("stream", ST), ("return_code", RC)],
    extra=[("k_64", {"k": 64}, LAUNCH), ("k_1", {"k": 1}, LAUNCH)])

# ==== the operators on a device CSR: attention, max / min / mean, sampling ===========================================================
# These launchers check in one order: sizes, enums, widths and floats first, then "nothing to do", then the pointers the sizes make the
# launch touch.  So a bad size or float is refused with nothing to do as well, and NULL is accepted exactly where nothing reads it.
# Baselines: 4 rows, 6 entries, 2 heads.  An edge tensor and an index array need 4 bytes, a gathered node tensor 16.
F32, F16, BF16 = 0, 1, 2
INF, NAN = float("inf"), float("nan")
NOT_FINITE = (INF, -INF, NAN)
_END = [("stream", ST), ("return_code", RC)]


def _nulls(params, but=()):
    return {p: NULL for p, role in params if role.kind == "pointer" and p not in but}


def _refused(param, values, nothing, alone=True):
    """Values of ``param`` that no role derives (a float, a list of widths): refused alone, and refused with ``nothing`` -- the
    overrides of a call with nothing to do -- as well: the check comes first.  ``alone=False``: the role derives the first already."""
    return [case for v in values for case in ([(f"{param}={v!r}", {param: v}, BAD)] if alone else []) +
            [(f"{param}={v!r},before_nothing_to_do", {param: v, **nothing}, BAD)]]


def _transposed(cases):
    """The cases of an entry point on the CSR for the one on the transposed CSR: its rows are the pattern's columns."""
    return [(what, {("num_cols" if k == "num_rows" else k): v for k, v in o.items()}, code) for what, o, code in cases]


def _off(names, bytes_off):
    return [(f"{p}+{bytes_off}", {p: ("off", bytes_off)}, BAD) for p in names]


_NNZ = ("nnz", N(6, INT_MAX))


def _beyond(**others):
    """nnz = 2^31 next to arguments other than the baseline's (the derived ``nnz=2147483648`` has the baseline's)."""
    return [("nnz=2147483648," + ",".join(f"{k}={v!r}" for k, v in others.items()), {"nnz": 2 ** 31, **others}, BAD)]


_NO_ROW = ("entries_but_no_row", {"num_rows": 0}, BAD)
# 16 bytes of the gathered operand: 8 elements when it is 16-bit, 4 when fp32
_PAIRS_REFUSED = [(f"pair_{x}_{y}", {"x_dtype": x, "y_dtype": y}, BAD) for x, y in ((F16, F32), (F16, BF16), (BF16, F16))]
_PAIRS = [(f"pair_{x}_{y}", {"x_dtype": x, "y_dtype": y}, LAUNCH) for x, y in ((F32, F32), (F32, BF16), (F16, F16), (BF16, BF16))]

# ---- sampled dense-dense product (sddmm_kernels.hpp, sddmm_heads_kernels.hpp) --------------------------------------------------------
_SDDMM = [("indptr", P(4)), ("indices", P(4)), ("num_rows", N(4)), _NNZ, ("embedding_dim", N(16)), ("x", P(16)), ("x_dtype", R(F32, 0, 2)),
          ("y", P(16)), ("y_dtype", R(F16, 0, 2)), ("out", P(4))] + _END
row("voltrix_launch_sddmm_csr", _SDDMM,
    zero=[({"nnz": 0}, OK), ({"nnz": 0, "out": NULL}, OK), ({"embedding_dim": 0}, OK), ({"nnz": 0, **_nulls(_SDDMM)}, OK)],
    extra=_PAIRS_REFUSED + _PAIRS + [
        _NO_ROW, ("width_16_bit_y", {"embedding_dim": 12}, BAD), ("width_16_bit", {"embedding_dim": 12, "x_dtype": F16}, BAD),
        ("width_fp32", {"embedding_dim": 6, "y_dtype": F32}, BAD), ("width_negative", {"embedding_dim": -8}, BAD),
        ("width_before_nothing_to_do", {"embedding_dim": 12, "nnz": 0}, BAD)] + _beyond(x_dtype=F16))
_SDDMM_HEADS = _SDDMM[:4] + [("heads", R(2, 1, None)), ("head_dim", N(16))] + _SDDMM[5:]
# heads * head_dim <= INT_MAX; heads and the sizes are checked before "nothing to do"
_HEADS_EXTRA = [("heads_negative", {"heads": -2}, BAD), ("heads_times_head_dim_above_int_max", {"heads": 2 ** 20, "head_dim": 2 ** 12}, BAD),
                ("head_dim_negative", {"head_dim": -8}, BAD)]
row("voltrix_launch_sddmm_heads_csr", _SDDMM_HEADS,
    zero=[({"nnz": 0}, OK), ({"nnz": 0, "out": NULL}, OK), ({"head_dim": 0}, OK), ({"nnz": 0, **_nulls(_SDDMM_HEADS)}, OK)],
    extra=_PAIRS_REFUSED + _PAIRS + _HEADS_EXTRA + [
        _NO_ROW, ("heads_before_nothing_to_do", {"heads": 0, "nnz": 0}, BAD), ("width_16_bit_y", {"head_dim": 12}, BAD),
        ("width_16_bit", {"head_dim": 20, "x_dtype": F16}, BAD), ("width_fp32", {"head_dim": 6, "y_dtype": F32}, BAD)] + _beyond(x_dtype=F16))

# ---- edge softmax (edge_softmax_kernels.hpp, edge_softmax_heads_kernels.hpp) ---------------------------------------------------------
# scale: any finite float (negative: +inf masks); the workspace is the one 16-byte pointer
_SOFTMAX_ZERO = [({"nnz": 0}, OK), ({"nnz": 0, "out": NULL}, OK), ({"nnz": 0, "num_rows": 0}, OK)]
_SOFTMAX_EXTRA = [_NO_ROW, ("scale_negative", {"scale": -1.5}, LAUNCH), ("scale_zero", {"scale": 0.0}, LAUNCH)] + \
    _refused("scale", NOT_FINITE, {"nnz": 0})
for _name, _heads, _in in (("voltrix_launch_edge_softmax_csr", [], [("scores", P(4))]),
                           ("voltrix_launch_edge_softmax_backward_csr", [], [("alpha", P(4)), ("grad_alpha", P(4))]),
                           ("voltrix_launch_edge_softmax_heads_csr", [("heads", R(2, 1, 65535))], [("scores", P(4))]),
                           ("voltrix_launch_edge_softmax_heads_backward_csr", [("heads", R(2, 1, 65535))],
                            [("alpha", P(4)), ("grad_alpha", P(4))])):
    _params = [("indptr", P(4)), ("num_rows", N(4)), _NNZ] + _heads + _in + [("scale", V(1.0)), ("out", P(4)), ("workspace", P(16))] + _END
    row(_name, _params, zero=_SOFTMAX_ZERO + [({"nnz": 0, **_nulls(_params)}, OK)],
        extra=_SOFTMAX_EXTRA + ([("heads_negative", {"heads": -1}, BAD),
                                 ("heads_before_nothing_to_do", {"heads": 0, "nnz": 0}, BAD)] if _heads else []))

# ---- multi-head aggregation (spmm_csr_heads_kernels.hpp): the entry count is the device's, so indices and values are required -------
_WIDTHS = [("width_fp16", {"head_dim": 12, "dtype": F16}, BAD), ("width_bf16", {"head_dim": 20, "dtype": BF16}, BAD),
           ("width_fp32", {"head_dim": 6, "dtype": F32}, BAD)]
_AGG_HEADS = [("indptr", P(4)), ("indices", P(4)), ("values", P(4)), ("num_rows", N(4)), ("heads", R(2, 1, None)), ("head_dim", N(16)),
              ("input", P(16)), ("dtype", R(F16, 0, 2)), ("output", P(16))] + _END
row("voltrix_launch_spmm_csr_heads", _AGG_HEADS,
    zero=[({"num_rows": 0}, OK), ({"num_rows": 0, "output": NULL}, OK), ({"head_dim": 0}, OK), ({"num_rows": 0, **_nulls(_AGG_HEADS)}, OK)],
    extra=_HEADS_EXTRA + _WIDTHS + [("heads=-1", {"heads": -1}, BAD), ("heads_before_nothing_to_do", {"heads": 0, "num_rows": 0}, BAD),
                                    ("width_before_nothing_to_do", {"head_dim": 12, "num_rows": 0}, BAD)])

# ---- GAT and GATv2 scores and the row sums of their backward (gat_score_kernels.hpp, gatv2_score_kernels.hpp) -----------------------
# slope: any finite float.  order: NULL has a meaning (the entries in CSR order) -- for the cases that is E: set at the baseline, NULL
# accepted, misaligned refused.  The row sums zero-fill out for nnz == 0: with rows that is a launch and needs out.
_EMPTY = {"nnz": 0, "num_rows": 0}
_GAT_EXTRA = [("heads_negative", {"heads": -3}, BAD), ("heads_before_nothing_to_do", {"heads": 0, "nnz": 0}, BAD), _NO_ROW,
              ("heads_times_num_rows_above_int_max", {"num_rows": 2 ** 20, "heads": 2 ** 12}, BAD)] + _refused("slope", NOT_FINITE, _EMPTY)
_GAT = [("indptr", P(4)), ("indices", P(4)), ("num_rows", N(4)), _NNZ, ("heads", R(2, 1, 65535)), ("el", P(4)), ("er", P(4)),
        ("slope", V(0.2)), ("out", P(4))] + _END
row("voltrix_launch_gat_score_csr", _GAT,
    zero=[(_EMPTY, OK), ({"nnz": 0}, OK), ({"nnz": 0, "out": NULL}, OK), ({"nnz": 0, **_nulls(_GAT)}, OK)],
    extra=_GAT_EXTRA + [("slope_negative", {"slope": -0.5}, LAUNCH), ("four_heads", {"heads": 4}, LAUNCH)])
_GAT_ROWSUM = [("indptr", P(4)), ("indices", P(4)), ("order", E(4)), ("num_rows", N(4)), _NNZ, ("heads", R(2, 1, 65535)), ("a", P(4)),
               ("b", P(4)), ("grad", P(4)), ("slope", V(0.2)), ("out", P(4)), ("workspace", P(16))] + _END
row("voltrix_launch_gat_score_rowsum_csr", _GAT_ROWSUM,
    zero=[(_EMPTY, OK), ({**_EMPTY, "out": NULL}, OK), ({**_EMPTY, **_nulls(_GAT_ROWSUM)}, OK), ({"nnz": 0}, LAUNCH),
          ({"nnz": 0, **_nulls(_GAT_ROWSUM, but=("out",))}, LAUNCH)],
    extra=_GAT_EXTRA + [("rows_to_zero_fill_but_nowhere_to_write", {"nnz": 0, "out": NULL}, BAD)])

# a head is a whole number of 16-byte pieces of xl / xr; dtype, width and slope are refused before "nothing to do"
_GATV2_WIDTHS = [(F16, 4), (F16, 12), (BF16, 20), (F32, 2), (F32, 6)]
_GATV2_EXTRA = [("heads_negative", {"heads": -3}, BAD), ("heads_before_nothing_to_do", {"heads": 0, **_EMPTY}, BAD), _NO_ROW,
                ("head_dim_negative", {"head_dim": -8}, BAD),
                ("heads_times_head_dim_above_int_max", {"heads": 2 ** 16, "head_dim": 2 ** 15}, BAD)] + \
    [case for d, w in _GATV2_WIDTHS for case in ((f"width_{d}_{w}", {"dtype": d, "head_dim": w}, BAD),
                                                 (f"width_{d}_{w},before_nothing_to_do", {"dtype": d, "head_dim": w, **_EMPTY}, BAD))] + \
    _refused("dtype", (-1, 3), _EMPTY, alone=False) + _refused("dtype", (7,), _EMPTY) + _refused("slope", NOT_FINITE, _EMPTY)
_GATV2_ZERO = [(_EMPTY, OK), ({**_EMPTY, "head_dim": 0}, OK)]
_GATV2 = [("indptr", P(4)), ("indices", P(4)), ("num_rows", N(4)), _NNZ, ("heads", R(2, 1, None)), ("head_dim", N(8)), ("xl", P(16)),
          ("xr", P(16)), ("dtype", R(F16, 0, 2)), ("a", P(16)), ("slope", V(0.2)), ("out", P(4))] + _END
row("voltrix_launch_gatv2_score_csr", _GATV2,
    zero=_GATV2_ZERO + [case for d in (F32, F16, BF16) for case in (({"nnz": 0, "dtype": d}, OK), ({"nnz": 0, "dtype": d, "out": NULL}, OK),
                                                                    ({"head_dim": 0, "dtype": d, "a": NULL}, OK))] +
    [({"nnz": 0, **_nulls(_GATV2)}, OK)],
    extra=_GATV2_EXTRA + _off(("xl", "xr", "a"), 2) + [("fp32_rows", {"dtype": F32}, LAUNCH), ("bf16_rows", {"dtype": BF16}, LAUNCH)] +
    _beyond(head_dim=16))
# with nnz == 0 every row is zero-filled and indices, q, grad are not read
_GATV2_ROWSUM = [("indptr", P(4)), ("indices", P(4)), ("order", E(4)), ("num_rows", N(4)), _NNZ, ("heads", R(2, 1, None)),
                 ("head_dim", N(8)), ("p", P(16)), ("q", P(16)), ("dtype", R(F16, 0, 2)), ("grad", P(4)), ("slope", V(0.2)),
                 ("out", P(16))] + _END
row("voltrix_launch_gatv2_rowsum_csr", _GATV2_ROWSUM,
    zero=_GATV2_ZERO + [({**_EMPTY, "out": NULL}, OK), ({"head_dim": 0, "out": NULL}, OK), ({**_EMPTY, **_nulls(_GATV2_ROWSUM)}, OK),
                        ({"nnz": 0}, LAUNCH), ({"nnz": 0, "indices": NULL, "order": NULL, "q": NULL, "grad": NULL}, LAUNCH)],
    extra=_GATV2_EXTRA + _off(("p", "q", "out"), 2) + [("rows_to_zero_fill_but_nowhere_to_write", {"nnz": 0, "out": NULL}, BAD)] +
    _beyond(head_dim=16))

# ---- edge softmax and aggregation in one launch, its two gradients, and the three with a keep mask (attn_aggregate_kernels.hpp,
# ---- attn_aggregate_dropout.hpp, dropout_mask_kernels.hpp) ---------------------------------------------------------------------------
# heads, the sizes, the width, dtype, scale and keep_scale are checked before "nothing to do".  keep_scale: finite and not negative
# (-2^-140 is a negative fp32 subnormal).  The mask is read where an edge is: required when nnz > 0 and the call has something to do.
_ATTN_EXTRA = _HEADS_EXTRA + _WIDTHS + [("heads_before_nothing_to_do", {"heads": 0, **_EMPTY}, BAD)] + _refused("scale", NOT_FINITE, _EMPTY)
_KEEP = _refused("keep_scale", NOT_FINITE + (-1.0, -2.0 ** -140), _EMPTY)
_KEEP_ZERO = [({"keep_scale": 0.0, **_EMPTY}, OK)]
_SIZES = [("num_rows", N(4)), _NNZ, ("heads", R(2, 1, None)), ("head_dim", N(16))]
_MASK = [("mask", P(4)), ("keep_scale", V(2.5))]

_FORWARD = [("indptr", P(4)), ("indices", P(4)), ("scores", P(4))] + _SIZES + [("feat", P(16)), ("dtype", R(F16, 0, 2)), ("scale", V(1.0)),
                                                                               ("out", P(16)), ("m", P(4)), ("l", P(4))]
_GRAD_SCORES = [("indptr", P(4)), ("indices", P(4))] + _SIZES + [
    ("grad_out", P(16)), ("feat", P(16)), ("dtype", R(F16, 0, 2)), ("scores", P(4)), ("m", P(4)), ("l", P(4)), ("delta", P(4)),
    ("scale", V(1.0)), ("grad_scores", P(4))]
# on the transposed CSR: its rows are the pattern's columns
_GRAD_FEAT = [("t_indptr", P(4)), ("t_indices", P(4)), ("order", P(4)), ("num_cols", N(4))] + _SIZES[1:] + [
    ("grad_out", P(16)), ("dtype", R(F32, 0, 2)), ("scores", P(4)), ("m", P(4)), ("l", P(4)), ("scale", V(1.0)), ("grad_feat", P(16))]
for _name, _drop in (("voltrix_launch_attn_aggregate_csr", []), ("voltrix_launch_attn_aggregate_dropout_csr", _MASK)):
    _params = _FORWARD + _drop + _END
    # nnz == 0 with rows still zero-fills out and l: the outputs (and indptr) must be valid, the operands of the edges need not be
    row(_name, _params,
        zero=[(_EMPTY, OK), ({**_EMPTY, **_nulls(_params)}, OK), ({"head_dim": 0}, OK), ({"head_dim": 0, **_nulls(_params)}, OK),
              ({"nnz": 0}, LAUNCH), ({"nnz": 0, **_nulls(_params, but=("indptr", "out", "m", "l"))}, LAUNCH)] + (_KEEP_ZERO if _drop else []),
        extra=_ATTN_EXTRA + (_KEEP + _beyond(keep_scale=1.0) if _drop else []) +
        [_NO_ROW, ("nnz_0_out+8", {"nnz": 0, "out": ("off", 8)}, BAD)] +
        [(f"nnz_0_{p}=NULL", {"nnz": 0, p: NULL}, BAD) for p in ("indptr", "out", "m", "l")])
for _name, _drop in (("voltrix_launch_attn_aggregate_grad_scores_csr", []), ("voltrix_launch_attn_aggregate_dropout_grad_scores_csr", _MASK)):
    _params = _GRAD_SCORES + _drop + _END
    row(_name, _params,
        zero=[({"nnz": 0}, OK), ({"nnz": 0, **_nulls(_params)}, OK), (_EMPTY, OK), ({"head_dim": 0}, OK),
              ({"head_dim": 0, **_nulls(_params)}, OK)] + (_KEEP_ZERO if _drop else []),
        extra=_ATTN_EXTRA + (_KEEP + _beyond(keep_scale=1.0) if _drop else []) + [_NO_ROW])
_EMPTY_T = {"nnz": 0, "num_cols": 0}
for _name, _drop in (("voltrix_launch_attn_aggregate_grad_feat_csr", []), ("voltrix_launch_attn_aggregate_dropout_grad_feat_csr", _MASK)):
    _params = _GRAD_FEAT + _drop + _END
    # nnz == 0 with rows zero-fills grad_feat and reads nothing but t_indptr
    row(_name, _params,
        zero=[(_EMPTY_T, OK), ({**_EMPTY_T, **_nulls(_params)}, OK), ({"head_dim": 0}, OK), ({"head_dim": 0, **_nulls(_params)}, OK),
              ({"nnz": 0}, LAUNCH), ({"nnz": 0, **_nulls(_params, but=("t_indptr", "grad_feat"))}, LAUNCH)] +
        ([({"keep_scale": 0.0, **_EMPTY_T}, OK)] if _drop else []),
        extra=_transposed(_ATTN_EXTRA + (_KEEP if _drop else []) + [_NO_ROW]) + _beyond(dtype=F16, **({"keep_scale": 1.0} if _drop else {})) +
        [(f"nnz_0_{p}=NULL", {"nnz": 0, p: NULL}, BAD) for p in ("t_indptr", "grad_feat")])

_DROPOUT = [_NNZ, ("heads", R(2, 1, None)), ("threshold", V(5)), ("seed", V(2 ** 63 + 1)), ("offset", V(2 ** 40)), ("mask", P(4))] + _END
row("voltrix_launch_dropout_mask", _DROPOUT, zero=[({"nnz": 0}, OK), ({"nnz": 0, "mask": NULL}, OK)],
    extra=[("heads_negative", {"heads": -1}, BAD), ("heads_before_nothing_to_do", {"heads": 0, "nnz": 0}, BAD),
           ("mask+1", {"mask": ("off", 1)}, BAD),
           ("threshold_and_counters_at_their_ends", {"threshold": 2 ** 32 - 1, "seed": 2 ** 64 - 1, "offset": 2 ** 64 - 1}, LAUNCH),
           ("33_heads", {"heads": 33}, LAUNCH)] + _beyond(seed=7, offset=9))

# ---- max / min / mean aggregation and the backward of max / min (spmm_csr_reduce_kernels.hpp) ----------------------------------------
# arg: NULL = not computed, and it must be NULL for the mean.  The width, op, dtype and "the mean has no arg" come before "nothing to
# do".  The forward's entry count is the device's: indices and input are required.  The backward with nnz == 0 reads t_indptr alone.
_REDUCE = [("indptr", P(4)), ("indices", P(4)), ("num_rows", N(4)), ("embedding_dim", N(8)), ("input", P(16)), ("dtype", R(F32, 0, 2)),
           ("op", R(0, 0, 2)), ("output", P(16)), ("arg", O(16))] + _END
row("voltrix_launch_spmm_csr_reduce", _REDUCE,
    zero=[({"num_rows": 0}, OK), ({"embedding_dim": 0}, OK), ({"num_rows": 0, **_nulls(_REDUCE)}, OK)],
    extra=[("width_negative", {"embedding_dim": -4}, BAD), ("width_fp32", {"embedding_dim": 6}, BAD),
           ("width_fp16", {"embedding_dim": 12, "dtype": F16}, BAD), ("width_bf16", {"embedding_dim": 12, "dtype": BF16}, BAD),
           ("width_before_nothing_to_do", {"embedding_dim": 6, "num_rows": 0}, BAD), ("mean", {"op": 2}, LAUNCH),
           ("min_with_arg", {"op": 1, "arg": SET}, LAUNCH), ("the_mean_has_no_arg", {"op": 2, "arg": SET}, BAD),
           ("the_mean_has_no_arg,before_nothing_to_do", {"op": 2, "arg": SET, "num_rows": 0}, BAD)] +
    [(f"{p}+4,with_arg", {p: ("off", 4), "arg": SET}, BAD) for p in ("input", "output")])
_REDUCE_BACKWARD = [("t_indptr", P(4)), ("t_indices", P(4)), ("t_order", P(4)), ("num_cols", N(4)), ("num_entries", N(6, INT_MAX)),
                    ("embedding_dim", N(8)), ("grad_out", P(16)), ("arg", P(16)), ("output", P(16))] + _END
row("voltrix_launch_spmm_csr_reduce_backward", _REDUCE_BACKWARD,
    zero=[({"num_cols": 0}, OK), ({"embedding_dim": 0}, OK), ({"num_cols": 0, **_nulls(_REDUCE_BACKWARD)}, OK), ({"num_entries": 0}, LAUNCH),
          ({"num_entries": 0, **_nulls(_REDUCE_BACKWARD, but=("t_indptr", "output"))}, LAUNCH)],
    extra=[("width_negative", {"embedding_dim": -4}, BAD), ("a_lane_owns_4_features", {"embedding_dim": 6}, BAD),
           ("width_before_nothing_to_do", {"embedding_dim": 6, "num_cols": 0}, BAD),
           ("no_entries_null_output", {"num_entries": 0, "output": NULL}, BAD)])

# ---- neighbour sampling: the plain rule, with an exclusion list, on cumulative weights (neighbor_sample_kernels.hpp,
# ---- weighted_sample_kernels.hpp) ------------------------------------------------------------------------------------------------------
# fanout: 1 .. 64 or -1 (all); sizes, fanout and replace are checked before "nothing to do" (no seeds).  indices, the weights and the
# outputs are looked at only where num_sampled > 0; an empty exclusion list may be NULL, but not misaligned.
_NO_SEEDS = {"num_seeds": 0}
_SAMPLE_TAIL = [("fanout", R(2, 1, 64)), ("replace", R(0, 0, 1)), ("seed", V(2 ** 63 + 1)), ("offset", V(2 ** 40))]
_SAMPLE = [("indptr", P(4)), ("indices", P(4)), ("num_rows", N(4)), ("seeds", P(4)), ("num_seeds", N(3)), ("s_indptr", P(4)),
           ("num_sampled", N(6, INT_MAX))] + _SAMPLE_TAIL
_SAMPLE_OUT = [("s_indices", P(4)), ("s_entries", P(4))]
_SAMPLE_EXTRA = _refused("fanout", (-2, INT_MAX, 2 ** 20), _NO_SEEDS) + _refused("fanout", (0, 65), _NO_SEEDS, alone=False) + \
    _refused("replace", (-1, 2), _NO_SEEDS, alone=False) + _refused("num_rows", (-1,), _NO_SEEDS, alone=False) + \
    _refused("num_sampled", (-1, 2 ** 31), _NO_SEEDS, alone=False) + [
    ("fanout_all", {"fanout": -1}, LAUNCH), ("with_replacement", {"replace": 1}, LAUNCH), ("fanout_64", {"fanout": 64}, LAUNCH),
    ("nothing_sampled_null_seeds", {"num_sampled": 0, "seeds": NULL}, BAD),
    ("nothing_sampled_null_indptr", {"num_sampled": 0, "indptr": NULL}, BAD)]


def _sample_zero(params, unread):
    return [(_NO_SEEDS, OK), ({**_NO_SEEDS, **_nulls(params)}, OK)] + \
        [({**_NO_SEEDS, "fanout": f, "replace": r}, OK) for f in (1, 64, -1) for r in (0, 1)] + \
        [({**_NO_SEEDS, "fanout": f, "replace": r, **_nulls(params)}, OK) for f in (1, 64, -1) for r in (0, 1)] + \
        [({"num_sampled": 0, "fanout": f, "replace": r, **{p: NULL for p in unread}}, OK) for f in (2, 1, 64, -1) for r in (0, 1)]


_params = _SAMPLE + _SAMPLE_OUT + _END
row("voltrix_launch_sample_neighbors", _params, zero=_sample_zero(_params, ("indices", "s_indices", "s_entries")), extra=_SAMPLE_EXTRA)
_params = _SAMPLE + [("exclude", P(4)), ("num_exclude", N(2))] + _SAMPLE_OUT + _END
row("voltrix_launch_sample_neighbors_excluding", _params, zero=_sample_zero(_params, ("indices", "s_indices", "s_entries")),
    extra=_SAMPLE_EXTRA + _refused("num_exclude", (-1,), _NO_SEEDS, alone=False) + [
        ("empty_list", {"num_exclude": 0}, LAUNCH), ("empty_list_may_be_null", {"num_exclude": 0, "exclude": NULL}, LAUNCH),
        ("empty_list_misaligned", {"num_exclude": 0, "exclude": ("off", 2)}, BAD),
        ("nothing_sampled_list_misaligned", {"num_sampled": 0, "exclude": ("off", 2)}, BAD),
        ("nothing_sampled_empty_list_null", {"num_sampled": 0, "num_exclude": 0, "exclude": NULL, "indices": NULL, "s_indices": NULL,
                                             "s_entries": NULL}, OK),
        ("nothing_sampled_list_null", {"num_sampled": 0, "num_exclude": 1, "exclude": NULL}, BAD),
        ("nothing_sampled_empty_list_misaligned", {"num_sampled": 0, "num_exclude": 0, "exclude": ("off", 2)}, BAD)])
# cum is int64: 8 bytes
_params = _SAMPLE[:2] + [("cum", P(8))] + _SAMPLE[2:] + _SAMPLE_OUT + _END
row("voltrix_sample_neighbors_weighted", _params, zero=_sample_zero(_params, ("indices", "cum", "s_indices", "s_entries")),
    extra=_SAMPLE_EXTRA + _off(("cum",), 2))

# ---- relabelling a sampled block (neighbor_sample_kernels.hpp): sizes before "nothing to do" -------------------------------------------
_params = [("cols", P(4)), ("num_sampled", N(6, INT_MAX)), ("num_cols", N(9)), ("table", P(4))] + _END
row("voltrix_launch_block_mark", _params,
    zero=[({"num_sampled": 0}, OK), ({"num_sampled": 0, **_nulls(_params)}, OK), ({"num_cols": 0}, OK),
          ({"num_cols": 0, **_nulls(_params)}, OK)],
    extra=[("size_before_nothing_to_do", {"num_sampled": -1, "num_cols": 0}, BAD)])
_params = [("seeds", P(4)), ("num_seeds", N(3)), ("num_cols", N(9)), ("table", P(4))] + _END
row("voltrix_launch_block_mark_seeds", _params,
    zero=[({"num_seeds": 0}, OK), ({"num_seeds": 0, **_nulls(_params)}, OK), ({"num_cols": 0}, OK), ({"num_cols": 0, **_nulls(_params)}, OK)],
    extra=[("size_before_nothing_to_do", {"num_seeds": -1, "num_cols": 0}, BAD)])
_params = [("cols", P(4)), ("num_sampled", N(6, INT_MAX)), ("seeds", P(4)), ("num_seeds", N(3)), ("table", P(4)), ("rank", P(4)),
           ("num_cols", N(9)), ("num_src", N(5)), ("local", P(4)), ("src_ids", P(4))] + _END
_NO_BLOCK = {"num_sampled": 0, "num_seeds": 0, "num_src": 0}
row("voltrix_launch_block_relabel", _params, zero=[(_NO_BLOCK, OK), ({**_NO_BLOCK, **_nulls(_params)}, OK)],
    extra=[("fewer_sources_than_seeds", {"num_src": 2}, BAD), ("as_many_sources_as_seeds", {"num_src": 3}, LAUNCH),
           ("seeds_alone", {"num_sampled": 0, "cols": NULL, "table": NULL, "rank": NULL, "local": NULL}, LAUNCH)])

# ---- induced subgraphs and random walks (induced_subgraph_kernels.hpp) ---------------------------------------------------------------
# group: one of the five widths, checked with the sizes before "nothing to do" (no rows).  The fill looks at s_local and s_entries only
# where num_selected > 0.  Walks: length <= 2^20 and num_walkers * (length + 1) <= INT_MAX; indices and entries only where length > 0.
GROUPS = (4, 8, 16, 32, 64)
_NO_ROWS = {"num_sub_rows": 0}
_SUBGRAPH = [("indptr", P(4)), ("indices", P(4)), ("num_rows", N(4)), ("rows", P(4)), ("num_sub_rows", N(3)), ("table", P(4)),
             ("num_cols", N(9)), ("group", V(8))]
_SUBGRAPH_EXTRA = _refused("group", (0, 1, 2, 3, 5, 12, 24, 48, 63, 65, 128, -4, -64), _NO_ROWS) + \
    _refused("num_rows", (-1,), _NO_ROWS, alone=False) + \
    [(f"group={g}", {"group": g}, LAUNCH) for g in GROUPS if g != 8]
for _name, _tail in (("voltrix_launch_subgraph_count", [("counts", P(4))]),
                     ("voltrix_launch_subgraph_fill",
                      [("s_indptr", P(4)), ("num_selected", N(6, INT_MAX)), ("s_local", P(4)), ("s_entries", P(4))])):
    _params = _SUBGRAPH + _tail + _END
    _fill = len(_tail) > 1
    row(_name, _params,
        zero=[case for g in GROUPS for case in (({**_NO_ROWS, "group": g}, OK), ({**_NO_ROWS, "group": g, **_nulls(_params)}, OK))] +
        ([({"num_selected": 0}, OK), ({"num_selected": 0, "s_local": NULL, "s_entries": NULL}, OK)] if _fill else []),   # nothing kept
        extra=_SUBGRAPH_EXTRA + ([("num_selected_before_nothing_to_do", {"num_selected": 2 ** 31, **_NO_ROWS}, BAD),
                                  ("nothing_kept_null_s_indptr", {"num_selected": 0, "s_indptr": NULL}, BAD)] if _fill else []))
_params = [("indptr", P(4)), ("indices", P(4)), ("num_rows", N(4)), ("starts", P(4)), ("num_walkers", N(3)), ("length", N(5, 2 ** 20)),
           ("seed", V(2 ** 63 + 1)), ("offset", V(2 ** 40)), ("nodes", P(4)), ("entries", P(4)), ("step_major", R(0, 0, 1))] + _END
_NO_WALKERS = {"num_walkers": 0}
row("voltrix_launch_random_walk", _params,
    zero=[(_NO_WALKERS, OK), ({**_NO_WALKERS, **_nulls(_params)}, OK), ({**_NO_WALKERS, "length": 2 ** 20}, OK),
          ({**_NO_WALKERS, "step_major": 1}, OK), ({"length": 0}, LAUNCH), ({"length": 0, "indices": NULL, "entries": NULL}, LAUNCH)],
    extra=[("length_before_nothing_to_do", {"length": 2 ** 20 + 1, **_NO_WALKERS}, BAD),
           ("walkers_times_steps_above_int_max", {"length": 2 ** 20, "num_walkers": 2048}, BAD),
           ("walkers_times_steps_above_int_max_short", {"num_walkers": 2 ** 30, "length": 1}, BAD),
           ("step_major", {"step_major": 1}, LAUNCH)])

# ---- negative sampling, entry -> endpoints, (row, column) -> entry (negative_sample_kernels.hpp, find_edges_kernels.hpp) -------------
# k: 1 .. 1024, max_tries: 1 .. 256, num_src * k <= INT_MAX; everything but the pointers is checked before "nothing to do".  indices
# may be NULL (not misaligned) where num_entries == 0.
_ENTRIES = ("num_entries", N(6, INT_MAX))
_NO_INDICES = [("no_entries", {"num_entries": 0}, LAUNCH), ("no_entries_null_indices", {"num_entries": 0, "indices": NULL}, LAUNCH),
               ("no_entries_misaligned_indices", {"num_entries": 0, "indices": ("off", 2)}, BAD)]
_NO_SRC = {"num_src": 0}
_params = [("indptr", P(4)), ("indices", P(4)), ("num_rows", N(4)), ("num_cols", N(9)), _ENTRIES, ("src", P(4)), ("num_src", N(3)),
           ("k", R(5, 1, 1024)), ("max_tries", R(16, 1, 256)), ("exclude_self", R(0, 0, 1)), ("assume_sorted", R(1, 0, 1)),
           ("seed", V(2 ** 63 + 1)), ("offset", V(2 ** 40)), ("neg", P(4))] + _END
row("voltrix_launch_negative_sample", _params,
    zero=[({**_NO_SRC, "assume_sorted": s, **nulls}, OK) for s in (1, 0) for nulls in ({}, _nulls(_params))] +
    [({**_NO_SRC, "k": 1024, "max_tries": 256}, OK)],
    extra=_NO_INDICES + [case for p, top in (("k", 1025), ("max_tries", 257)) for case in
                         _refused(p, (-1, 2 ** 20), _NO_SRC) + _refused(p, (0, top), _NO_SRC, alone=False)] +
    [case for p in ("num_rows", "num_cols", "num_entries") for case in _refused(p, (-1,), _NO_SRC, alone=False)] + [
        ("slots_above_int_max", {"num_src": 2 ** 21, "k": 1024}, BAD), ("slots_above_int_max_k_2", {"num_src": INT_MAX, "k": 2}, BAD),
        ("k_1024_tries_256", {"k": 1024, "max_tries": 256}, LAUNCH), ("exclude_self", {"exclude_self": 1}, LAUNCH),
        ("unsorted", {"assume_sorted": 0}, LAUNCH)])
_NO_IDS = {"num_ids": 0}
_params = [("indptr", P(4)), ("indices", P(4)), ("num_rows", N(4)), _ENTRIES, ("entries", P(4)), ("num_ids", N(3)), ("rows", P(4)),
           ("cols", P(4))] + _END
row("voltrix_launch_edge_endpoints", _params, zero=[(_NO_IDS, OK), ({**_NO_IDS, **_nulls(_params)}, OK)],
    extra=_NO_INDICES + _refused("num_rows", (-1,), _NO_IDS, alone=False) + _refused("num_entries", (2 ** 31,), _NO_IDS, alone=False))
_NO_QUERIES = {"num_queries": 0}
_params = [("indptr", P(4)), ("indices", P(4)), ("num_rows", N(4)), _ENTRIES, ("rows", P(4)), ("cols", P(4)), ("num_queries", N(3)),
           ("assume_sorted", R(1, 0, 1)), ("out", P(4))] + _END
row("voltrix_launch_find_edges", _params,
    zero=[({**_NO_QUERIES, "assume_sorted": s, **nulls}, OK) for s in (1, 0) for nulls in ({}, _nulls(_params))],
    extra=_NO_INDICES + _refused("num_rows", (-1,), _NO_QUERIES, alone=False) +
    _refused("num_entries", (-1, 2 ** 31), _NO_QUERIES, alone=False) + _refused("assume_sorted", (2, -1), _NO_QUERIES, alone=False) +
    [("unsorted", {"assume_sorted": 0}, LAUNCH)])

# ---- the size functions: (name, arguments) -> the documented answer; ALIGNED: a multiple of 16 (the workspace is 16-byte aligned) ---
ALIGNED = "a multiple of 16"
POSITIVE_ALIGNED = "a positive multiple of 16"     # the rows above that call the workspace required rely on it
SIZE_FUNCTIONS = (
    ("voltrix_spmm_f32_workspace_bytes", (-1, 8), -1), ("voltrix_spmm_f32_workspace_bytes", (8, -1), -1),
    ("voltrix_spmm_f32_workspace_bytes", (0, 64), 16), ("voltrix_spmm_f32_workspace_bytes", (32, 64), 16 + 32 * 64 * 2),
    ("voltrix_fused_records_workspace_bytes", (-1,), 0), ("voltrix_fused_records_workspace_bytes", (0,), ALIGNED),
    ("voltrix_fused_records_workspace_bytes", (32,), POSITIVE_ALIGNED),
    ("voltrix_panel_plan_workspace_bytes", (-1, 8, 4), 0), ("voltrix_panel_plan_workspace_bytes", (32, 0, 4), 0),
    ("voltrix_panel_plan_workspace_bytes", (32, 8, 0), 0), ("voltrix_panel_plan_workspace_bytes", (0, 8, 4), ALIGNED),
    ("voltrix_panel_plan_workspace_bytes", (32, 8, 4), POSITIVE_ALIGNED),
    ("voltrix_unit_table_workspace_bytes", (0,), ALIGNED), ("voltrix_unit_table_workspace_bytes", (32,), POSITIVE_ALIGNED),
    ("voltrix_unit_table_fill_workspace_bytes", (0,), ALIGNED), ("voltrix_unit_table_fill_workspace_bytes", (2,), POSITIVE_ALIGNED),
    ("voltrix_stream_table_workspace_bytes", (0,), ALIGNED), ("voltrix_stream_table_workspace_bytes", (32,), POSITIVE_ALIGNED),
    ("voltrix_stream_table_fill_workspace_bytes", (0,), ALIGNED), ("voltrix_stream_table_fill_workspace_bytes", (2,), POSITIVE_ALIGNED),
    ("voltrix_panel_parts_workspace_bytes", (0,), ALIGNED), ("voltrix_panel_parts_workspace_bytes", (4,), POSITIVE_ALIGNED),
    ("voltrix_csr_preprocess_workspace_bytes", (0, 0, 0, -1), ALIGNED), ("voltrix_csr_preprocess_workspace_bytes", (32, 32, 8, -1), ALIGNED),
    ("voltrix_csr_transpose_workspace_bytes", (0,), 0), ("voltrix_cm_rank_workspace_bytes", (0,), 0),
)


# ---- derivation ---------------------------------------------------------------------------------------------------------------------------
def _case(r, what, overrides, expect):
    return dict(id=f"{r['name']}::{what}", name=r["name"], overrides=dict(overrides), expect=expect)


def cases():
    """Every call of the contract, ``[{id, name, overrides, expect}]``, in table order: per row the baseline first."""
    out = []
    for r in ROWS.values():
        out.append(_case(r, "baseline", {}, r["baseline"]))
        for pname, role in r["params"]:
            if isinstance(role, O):
                out.append(_case(r, f"{pname}=set", {pname: SET, **role.needs}, r["baseline"]))
                for off in _offsets(role.align) if role.align else ():
                    out.append(_case(r, f"{pname}+{off}", {pname: ("off", off), **role.needs}, BAD))
            elif isinstance(role, E):
                out.append(_case(r, f"{pname}=NULL(may be empty)", {pname: NULL}, r["baseline"]))
                for off in _offsets(role.align) if role.align else ():
                    out.append(_case(r, f"{pname}+{off}", {pname: ("off", off)}, BAD))
            elif isinstance(role, P):
                out.append(_case(r, f"{pname}=NULL", {pname: NULL}, BAD))
                for off in _offsets(role.align) if role.align else ():
                    out.append(_case(r, f"{pname}+{off}", {pname: ("off", off)}, BAD))
            elif isinstance(role, N):
                out.append(_case(r, f"{pname}=-1", {pname: -1}, BAD))
                if role.hi is not None:
                    out.append(_case(r, f"{pname}={role.hi}(the limit)", {pname: role.hi}, r["baseline"]))
                    out.append(_case(r, f"{pname}={role.hi + 1}", {pname: role.hi + 1}, role.code))
            elif isinstance(role, R):
                if role.lo is not None:
                    out.append(_case(r, f"{pname}={role.lo - 1}", {pname: role.lo - 1}, BAD))
                if role.hi is not None:
                    out.append(_case(r, f"{pname}={role.hi + 1}", {pname: role.hi + 1}, BAD))
        for i, (overrides, expect) in enumerate(r["zero"]):
            out.append(_case(r, f"nothing_to_do_{i}({','.join(f'{k}={v}' for k, v in overrides.items())})", overrides, expect))
        for what, overrides, expect in r["extra"]:
            out.append(_case(r, what, overrides, expect))
    ids = [c["id"] for c in out]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    return out
