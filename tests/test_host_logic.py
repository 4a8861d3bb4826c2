"""CPU: host-side logic of the product package -- operator-API assertions, tile space, tuner key, synthetic graph
generators, roofline accounting, row-window sharding."""
import dataclasses

import numpy as np
import pytest
import torch

import synth_graphs
import voltrix
from voltrix import dist as vdist
from voltrix.jit_kernels import spmm as spmm_mod


def test_csr_preprocess_asserts_like_reference():
    indptr = torch.tensor([0, 1, 2], dtype=torch.int32)
    with pytest.raises(AssertionError):  # reference spmm.py:21-22: CPU int32 only
        voltrix.csr_preprocess(indptr.long(), torch.tensor([0, 1], dtype=torch.int32), 2)
    with pytest.raises(AssertionError):
        voltrix.csr_preprocess(indptr, torch.tensor([0, 1], dtype=torch.int64), 2)


def test_spmm_kernel_asserts_like_reference():
    t = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(AssertionError):  # reference jit_kernels/spmm.py:50-54: CUDA tensors required
        voltrix.spmm_kernel(t, t, t, num_nodes=1, num_edges=0, embedding_dim=8, input=torch.zeros(1, 8),
                            output=torch.zeros(1, 8))
    with pytest.raises(AssertionError):
        voltrix.spmm(t, t, t, 1, 0, torch.zeros(1, 8))


def test_tile_space_is_valid_and_bounded(monkeypatch):
    for mode, lo, hi in (("default", 16, 74), ("full", 36, 226), ("none", 1, 1), ("stream", 1, 1)):  # fp32: + 4 stream points
        monkeypatch.setenv("VOLTRIX_TUNE_SPACE", mode)
        for f in (16, 32, 64, 128, 512):
            for eb in (2, 4):
                space = spmm_mod.tile_space(f, eb)
                assert lo <= len(space) <= hi, (mode, f, eb, len(space))
                for p in space:
                    assert spmm_mod._lds_bytes(p["FS"], p["DEPTH"], p["WAVES"], p["EB"]) <= 160 * 1024
                    assert p["EB"] == eb and p["FS"] in (32, 64, 128, 256) and p["SCHED"] in ((0, 1, 2, 3, 4, 5, 6) if eb == 2 else (0, 1, 2, 3, 6))
                    assert p["SCHED"] != 5 or (p["WAVES"] == 4 and (p["FS"] >= 64 or f <= p["FS"]))   # paired units
                    if p["SCHED"] == 6:   # stream points: loads + stores behind a counted wait fit the 6-bit vmcnt
                        ndma, slots = 32 * p["FS"] * eb // 1024, p["FS"] // 16
                        assert eb == 2 or p["FS"] <= 64
                        assert p["WAVES"] in (1, 2) and (1 + ndma) * (p["DEPTH"] - 1) + p["DEPTH"] * slots <= 63
                # the stream kernel serves plain stores of a binary 16-bit operand only
                for kw in (dict(weighted=True), dict(max_lds=spmm_mod.TWO_LEVEL_LDS_BUDGET), dict(stream_ok=False)):
                    if eb == 2:
                        assert all(p["SCHED"] != 6 for p in spmm_mod.tile_space(f, eb, **kw)), (mode, f, kw)
    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "none")
    # the single default point = the ahead-of-time library's default tile + the unit-table schedule
    assert spmm_mod.tile_space(128, 2) == ({"FS": 128, "DEPTH": 3, "WAVES": 4, "EB": 2, "SCHED": 4, "BF16": 0, "WEIGHTED": 0},)
    assert spmm_mod.tile_space(128, 2, bf16=True) == ({"FS": 128, "DEPTH": 3, "WAVES": 4, "EB": 2, "SCHED": 4, "BF16": 1, "WEIGHTED": 0},)
    assert spmm_mod.tile_space(64, 2) == ({"FS": 64, "DEPTH": 3, "WAVES": 4, "EB": 2, "SCHED": 4, "BF16": 0, "WEIGHTED": 0},)
    # ... beside a panel workgroup (two-level format): two units per wave
    assert spmm_mod.tile_space(128, 2, max_lds=spmm_mod.TWO_LEVEL_LDS_BUDGET) == (
        {"FS": 128, "DEPTH": 3, "WAVES": 4, "EB": 2, "SCHED": 5, "BF16": 0, "WEIGHTED": 0},)
    assert spmm_mod.tile_space(128, 2, weighted=True) == ({"FS": 128, "DEPTH": 3, "WAVES": 4, "EB": 2, "SCHED": 4, "BF16": 0, "WEIGHTED": 1},)
    assert spmm_mod.tile_space(16, 4) == ({"FS": 32, "DEPTH": 3, "WAVES": 1, "EB": 4, "SCHED": 2, "BF16": 0, "WEIGHTED": 0},)


def test_feature_hash_uses_tag_then_address():
    t = torch.zeros(4, dtype=torch.int32)
    with pytest.warns(UserWarning, match="hash_tag"):
        h_addr = spmm_mod.feature_hash(t)
    t.hash_tag = "test_20_8192_0.1"
    assert spmm_mod.feature_hash(t) == voltrix.jit.hash_to_hex("test_20_8192_0.1") != h_addr


def test_synthetic_graphs_are_canonical_and_seeded():
    a = synth_graphs.generate("reddit_like", scale=0.004)
    b = synth_graphs.generate("reddit_like", scale=0.004)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    indptr, indices, cfg = a
    n = indptr.numel() - 1
    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32 and int(indptr[-1]) == indices.numel()
    ip, ix = indptr.numpy(), indices.numpy()
    for r in np.random.default_rng(0).choice(n, 50, replace=False):
        row = ix[ip[r]:ip[r + 1]]
        assert (np.diff(row) > 0).all() and row.min(initial=0) >= 0 and row.max(initial=0) < n
    assert (np.diff(ip) >= 1).all()
    # the published shapes of the BASELINE configs
    assert synth_graphs.CONFIGS["reddit_like"]["num_nodes"] == 232965
    assert synth_graphs.algorithmic_bytes(232965, 114615892, 128, 2) == 4 * (114615892 + 232966) + 232965 * 128 * 6
    assert synth_graphs.flops(114615892, 128) == 2 * 114615892 * 128


def test_partition_rows_balances_edges_on_window_boundaries():
    indptr, indices, _ = synth_graphs.generate("reddit_like", scale=0.01)
    n = indptr.numel() - 1
    for world in (1, 2, 3, 8):
        parts = vdist.partition_rows(indptr, n, world)
        assert parts[0][0] == 0 and parts[-1][1] == n and len(parts) == world
        edges = []
        for (r0, r1), nxt in zip(parts, parts[1:] + [(n, n)]):
            assert r1 == nxt[0] and r0 % 16 == 0 and r0 <= r1
            edges.append(int(indptr[r1]) - int(indptr[r0]))
        assert sum(edges) == indices.numel()
        if world > 1:
            assert max(edges) <= 1.25 * (indices.numel() / world) + 16 * 3000


def test_remap_columns_addresses_the_padded_gather_buffer():
    parts = [(0, 32), (32, 48), (48, 100)]
    rows_padded = 52
    cols = torch.tensor([0, 31, 32, 47, 48, 99], dtype=torch.int32)
    got = vdist.remap_columns(cols, parts, rows_padded).tolist()
    assert got == [0, 31, 52, 52 + 15, 104, 104 + 51]


def test_launch_plan_keeps_every_table_argument_alive():
    """A cached launch plan holds the ADDRESSES of its whole argument list: it keeps alive every tensor argument but the
    operands and partial tiles every call passes anew and ``hspa_packed`` (the plan lives on it) -- also one added later."""
    per_call = {"input", "output", "out_scale", "values", "tickets", "partials", "partials_p", "partials_s", "hspa_packed"}
    defs = spmm_mod.arg_defs_for(torch.float16) + (("new_table", torch.int32),)
    named = {name: torch.zeros(1, dtype=t) if isinstance(t, torch.dtype) else 0 for name, t in defs}
    kept = {id(t) for t in spmm_mod.plan_keepalive(named)}
    want = {name for name, t in defs if isinstance(t, torch.dtype) and name not in per_call}
    assert {name for name, value in named.items() if id(value) in kept} == want
    assert want == {"blk_offsets", "hind", "win_order_a", "win_order_b", "win_order_c", "units", "unit_ptr", "cuts", "units_p",
                    "unit_ptr_p", "cuts_p", "row_map", "s_units", "s_runs", "s_run_ptr", "cuts_s", "new_table"}
    # the argument tuple is built by name: every name of the list, no other
    assert spmm_mod._pack(defs, named) == tuple(named[name] for name, _ in defs)
    with pytest.raises(AssertionError):
        spmm_mod._pack(defs, {k: v for k, v in named.items() if k != "cuts_p"})
    with pytest.raises(AssertionError):
        spmm_mod._pack(defs, dict(named, cuts_q=0))
    # every table-driven schedule fills launch arguments of the list from attributes its table has
    from voltrix.schedule import StreamTable, UnitTable

    names = {name for name, _ in spmm_mod.arg_defs_for(torch.float16)}
    for sched, desc in spmm_mod.TABLE_SCHEDULES.items():
        table_type = StreamTable if sched == spmm_mod.SCHED_STREAM else UnitTable
        assert {arg for arg, _ in desc.fields} | {desc.partials} <= names, sched
        assert {attr for _, attr in desc.fields} <= set(table_type.__dataclass_fields__), sched


def test_tile_space_for_two_level_handles_leaves_room_for_the_panel_kernel():
    """Handles of the two-level format run beside the panel kernel: the tuner only sees window tiles whose workgroup fits
    the LDS the panel workgroup (44 KB) leaves on a CU."""
    from voltrix.jit_kernels import spmm as spmm_mod

    full = spmm_mod.tile_space(128, 2)
    fit = spmm_mod.tile_space(128, 2, max_lds=spmm_mod.TWO_LEVEL_LDS_BUDGET)
    assert fit and set(map(lambda p: tuple(sorted(p.items())), fit)) <= set(map(lambda p: tuple(sorted(p.items())), full))
    for p in fit:
        assert spmm_mod._lds_bytes(p["FS"], p["DEPTH"], p["WAVES"], p["EB"]) <= spmm_mod.TWO_LEVEL_LDS_BUDGET
        assert p["WAVES"] >= 4
    assert any(p["FS"] == 128 and p["DEPTH"] == 3 and p["WAVES"] == 4 for p in fit)


def test_every_default_panel_tile_is_instantiated():
    """voltrix.hybrid.default_panel_tile must only name tiles the ahead-of-time library instantiates
    (csrc/capi_spmm_panel.hip), for every plan geometry and feature width."""
    import os
    import re

    from conftest import PKG_ROOT
    from voltrix import hybrid

    src = open(os.path.join(PKG_ROOT, "csrc", "capi_spmm_panel.hip")).read()
    inst = {tuple(map(int, m)) for m in re.findall(r"X\((\d+), (\d+), (\d+), (\d+), (\d+)\)", src)}
    assert len(inst) > 10
    # tiles of the software-pipelined loop: X(FS, DEPTH, WAVES, RB) under ksteps = KSTEPS_PIPELINED
    pipe_space = re.search(r"#define VOLTRIX_PANEL_PIPE_SPACE\(X\)(.*)", src).group(1)
    piped = {tuple(map(int, m)) + (hybrid.KSTEPS_PIPELINED,) for m in re.findall(r"X\((\d+), (\d+), (\d+), (\d+)\)", pipe_space)}
    assert len(piped) >= 4 and f"kPipelined = {hybrid.KSTEPS_PIPELINED};" in src
    inst |= piped
    for feat in (8, 32, 48, 64, 96, 128, 200, 512):
        for waves in (4, 8):
            for rb in (2, 4):
                fs, depth, ksteps = hybrid.default_panel_tile(feat, waves, rb)
                assert (fs, depth, waves, rb, ksteps) in inst, (feat, waves, rb)


# ---- tests/test_gpu_tile_matrix.py: what its GPU cases rely on -------------------------------------------------------------
def test_shipped_tuned_defaults_lie_in_the_space_of_their_own_keys(monkeypatch):
    """The store only takes a choice that is in the space ``spmm_kernel`` computes for the call (``stored in list(space)``): a
    shipped entry outside it is silently ignored.  Windows are short (stream and two-slot points) when the bucket's mean TC
    blocks per window is at most STREAM_MAX_BLOCKS_PER_WINDOW; the half-octave that straddles the limit may be either."""
    import ast
    import math

    import tile_matrix_cases as tm

    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "default")
    store = tm.shipped_defaults()
    assert len(store) >= 100
    limit_x2 = 2 * math.log2(spmm_mod.STREAM_MAX_BLOCKS_PER_WINDOW)
    for key, point in store.items():
        keys = ast.literal_eval(key.split("|", 1)[1])
        width = 256 if keys["embedding_dim"] == "wide" else keys["embedding_dim"]
        dtype = keys["dtype"]
        eb = 4 if dtype == "torch.float32" else 2
        mean_x2 = ast.literal_eval(keys["graph_bucket"])["log2_mean_blocks_x2"]
        shorts = [s for s in (True, False) if (mean_x2 - 0.5 <= limit_x2 if s else mean_x2 + 0.5 > limit_x2)]
        spaces = [spmm_mod.tile_space(width, eb, dtype == "torch.bfloat16",
                                      spmm_mod.TWO_LEVEL_LDS_BUDGET if keys["two_level"] else None, weighted=keys["weighted"],
                                      stream_ok=short and not keys.get("row_map") and not keys["two_level"], shallow_ok=short)
                  for short in shorts]
        assert any(point in list(space) for space in spaces), (key, point)


def test_prebuild_covers_every_point_of_the_tile_matrix():
    """Every (point, dtype) the GPU tile matrix forces is built ahead of time: the GPU run compiles nothing."""
    import tile_matrix_cases as tm
    from voltrix.jit import cpp_format, generate
    from voltrix.jit_kernels import prebuild

    built = {code for name, _, code in prebuild.jobs() if name == "spmm_kernel"}
    dtypes = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
    missing = []
    for key in tm.enumerate_points():
        point = dict(key)
        code = generate(spmm_mod.includes, spmm_mod.arg_defs_for(dtypes[tm.kind_of(point)]), cpp_format(spmm_mod.template, point))
        if code not in built:
            missing.append(tm.case_id(point, 0))
    assert not missing, missing
    assert len(tm.enumerate_points()) >= 400


def test_tile_matrix_graphs_are_adversarial():
    """G1 cuts windows under all three cut schedules (unit table, paired unit table, stream table) in at least four of the
    eight XCD ranges of equal work, starts with an empty window and ends with a partial one; G2 is short-windowed
    (2-6 TC blocks per window on average), N % 16 = 1 with the single column N - 1 in its last window, three empty windows."""
    import tile_matrix_cases as tm
    from oracle import oracle_c
    from voltrix import schedule

    indptr, indices, n = tm.graph_cuts()
    assert n == 16 * 640 + 13
    p1, packed, hind = oracle_c.csr_preprocess(indptr, indices, n)
    b = torch.from_numpy(p1)
    nblk = b[1:] - b[:-1]
    nw = (n + 15) // 16
    row_deg = np.diff(indptr)
    win_edges = np.add.reduceat(row_deg, np.arange(0, n, 16))
    assert win_edges[0] == 0 and win_edges[-1] == 0 and n % 16 != 0
    assert (win_edges == 0).sum() >= 8
    assert np.median(nblk.numpy()) <= 3 and (row_deg >= 2000).sum() >= 8 + 16
    assert set(indices.tolist()) == set(range(n))                     # every row of B is gathered
    assert ((row_deg.reshape(-1)[: 16 * (n // 16)].reshape(-1, 16) >= 2000).all(1)).sum() == 1   # one window of hubs only
    nst = (nblk.long() + 3) // 4
    ranges = schedule.split_equal_work(nst).long()
    max_stages = schedule.default_max_stages(b, n)
    tables = {
        "units": schedule.unit_table_torch(b, n, xcd_ptr=ranges.int()),
        "pairs": schedule.unit_table_torch(b, n, max(8, int(spmm_mod.PAIR_UNIT_FACTOR * max_stages / 1.5)), xcd_ptr=ranges.int()),
        "stream": schedule.stream_tables_torch(b, torch.from_numpy(packed.view(np.int32)), torch.from_numpy(hind), n),
    }
    for name, table in tables.items():
        assert table.num_cuts > 0, name
        xcds = set(torch.searchsorted(ranges[1:8].contiguous(), table.cuts[:, 0].long(), right=True).tolist())
        assert len(xcds) >= 4, (name, xcds)
        assert int(table.cuts[:, 2].max()) >= 3, name               # several cuts in one window

    indptr, indices, n = tm.graph_short()
    assert n % 16 == 1 and indptr[-1] - indptr[-2] == 1 and indices[-1] == n - 1
    p1, _, _ = oracle_c.csr_preprocess(indptr, indices, n)
    nblk = np.diff(p1)
    assert 2 <= nblk.mean() <= 6
    win_edges = np.add.reduceat(np.diff(indptr), np.arange(0, n, 16))
    assert np.array_equal(np.nonzero(win_edges == 0)[0], [600, 601, 602])   # one run of three, in the middle


def test_join_names_the_codes_of_both_launchers():
    """``hybrid.Join``: one value per two-level step; the window kernel's ``atomic_out`` (spmm_kernels.hpp) and the panel kernel's
    ``accumulate`` (spmm_panel_kernels.hpp) are different encodings of the same three joins."""
    from voltrix import hybrid

    tickets = torch.zeros(8, dtype=torch.int32)
    want = {"add": (0, 1, (0, None)), "atomic": (1, 2, (1, None)), "ticket": (2, 3, (1, tickets))}
    assert set(want) == set(hybrid.JOIN_MODES)
    for mode, (window, panel, combine) in want.items():
        join = hybrid.Join(mode, tickets if mode == "ticket" else None)
        assert (join.window_out, join.panel_accumulate) == (window, panel), mode
        assert join.combine[0] == combine[0] and join.combine[1] is combine[1], mode
    assert (hybrid.WINDOW_STORE, hybrid.WINDOW_ATOMIC, hybrid.WINDOW_TICKET) == (0, 1, 2)
    assert (hybrid.PANEL_STORE, hybrid.PANEL_ADD, hybrid.PANEL_ATOMIC, hybrid.PANEL_TICKET) == (0, 1, 2, 3)
    with pytest.raises(AssertionError):
        hybrid.Join("ticket")                  # the ticket join without tickets
    for mode in ("add", "atomic"):
        with pytest.raises(AssertionError):
            hybrid.Join(mode, tickets)         # tickets nobody would read
    with pytest.raises(AssertionError):
        hybrid.Join("store")
    with pytest.raises(dataclasses.FrozenInstanceError):
        hybrid.Join("add").mode = "atomic"
