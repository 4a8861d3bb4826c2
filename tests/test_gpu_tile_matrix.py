"""GPU: every tile point the tuner can pick, forced one at a time, against a float64 oracle.

``voltrix.spmm`` runs whichever point of ``jit_kernels/spmm.py::tile_space`` the tuner picks for a handle, width and dtype, and
every point is a template instantiation of its own.  The cases (tests/tile_matrix_cases.py) are the (point, width) pairs
``tile_space`` offers over the modes none / stream / default and every flag set the operator passes, plus the shipped
``tuned_defaults.json`` points.  Each case forces its point through ``spmm_kernel`` (``tile_space`` patched to return it alone,
a hash tag of its own) and runs it on two adversarial graphs: G1 "cuts" (hub rows beside every XCD range boundary: unit tables,
pair tables and stream tables all cut windows) and G2 "short" (2-6 TC blocks per window).

Checks, output prefilled with NaN unless stated:
  * integer features in [-3, 3]: bit-exact (every fp32 order of the sum is exact);
  * random-normal features (fp16 also with values near 2^14 and subnormals): |out - ref| <= deg 2^-23 (A |B|) against the
    oracle on the same rounded operand -- the second and later calls go through the cached launch plan (replay);
  * G1 only: ``out_scale`` = 2^-3; ``atomic_out`` + ``beside_panel`` onto an integer prefill (points of the ``max_lds`` space);
    ``defer_combine`` (SCHED 4-6) then ``PendingCombine.run()``; a ``row_map`` permutation with -1 padding (SCHED 0-5);
  * WEIGHTED points: value planes of integer and of random values, against the oracle on values rounded to the plane type.
"""
import time
import zlib

import numpy as np
import pytest
import torch

import tile_matrix_cases as tm
import voltrix  # noqa: F401  (loads the library)
from voltrix.jit import compiler
from voltrix.jit_kernels import spmm as spmm_mod
from voltrix.jit_kernels.tuner import jit_tuner
from voltrix.weighted import value_plane

pytestmark = pytest.mark.gpu

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
OUT_SCALE = 2.0 ** -3
CASES = tm.cases()

_graphs, _operand_cache, _planes = {}, {}, {}


def _graph(name):
    """(indptr, indices, n) on the host, the device handle, float64 CSR of ones, degree per row."""
    if name not in _graphs:
        indptr, indices, n = tm.GRAPHS[name]()
        handle = voltrix.csr_preprocess(torch.from_numpy(indptr), torch.from_numpy(indices), n)
        a = torch.sparse_csr_tensor(torch.from_numpy(indptr).long(), torch.from_numpy(indices).long(),
                                    torch.ones(len(indices), dtype=torch.float64), (n, n))
        deg = torch.from_numpy(np.diff(indptr).astype(np.float64))
        _graphs[name] = (indptr, indices, n, handle, a, deg)
    return _graphs[name]


def _oracle(a, deg, feat, values=None):
    """(exact product in float64, element-wise bound deg 2^-23 (A |B|)) on the device; ``feat`` is the operand as the kernel sees it."""
    if values is not None:
        a = torch.sparse_csr_tensor(a.crow_indices(), a.col_indices(), values, a.shape)
        a_abs = torch.sparse_csr_tensor(a.crow_indices(), a.col_indices(), values.abs(), a.shape)
    else:
        a_abs = a
    b = feat.double().cpu()
    ref = a @ b
    bound = deg[:, None] * 2.0 ** -23 * (a_abs @ b.abs())
    return ref.cuda(), bound.cuda()


def _operands(graph, width, kind):
    """Integer, random-normal and (fp16) large / subnormal operands of the graph with their oracles, built once."""
    key = (graph, width, kind)
    if key not in _operand_cache:
        _, _, n, _, a, deg = _graph(graph)
        dtype = DTYPES[kind]
        gen = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
        ops = {}
        feat = torch.randint(-3, 4, (n, width), generator=gen).to(dtype)
        ops["int"] = (feat.cuda(),) + _oracle(a, deg, feat)
        feat = torch.randn(n, width, generator=gen).to(dtype)
        ops["normal"] = (feat.cuda(),) + _oracle(a, deg, feat)
        if kind == "f16":
            x = torch.randn(n, width, generator=gen)
            pick = torch.rand(n, width, generator=gen)
            x = torch.where(pick < 0.05, x.sign() * 2.0 ** 14 * (1 + x.abs() % 1), x)                  # around 2^14
            x = torch.where(pick > 0.9, torch.randint(-1023, 1024, (n, width), generator=gen) * 2.0 ** -24, x)  # subnormals
            feat = x.to(torch.float16)
            assert ((feat != 0) & (feat.abs() < 2.0 ** -14)).any()
            ops["extreme"] = (feat.cuda(),) + _oracle(a, deg, feat)
        _operand_cache[key] = ops
    return _operand_cache[key]


def _plane(graph, kind, which):
    """Value plane of the graph in ``kind``'s 16-bit type, of integer values in [-3, 3] or random-normal ones, and the values
    rounded to that type (float64, host) for the oracle."""
    key = (graph, kind, which)
    if key not in _planes:
        indptr, indices, n, handle, _, _ = _graph(graph)
        gen = torch.Generator().manual_seed(7 if which == "int" else 8)
        if which == "int":
            vals = torch.randint(-3, 4, (len(indices),), generator=gen).float()
        else:
            vals = torch.randn(len(indices), generator=gen)
        dtype = DTYPES[kind]
        plane = value_plane(torch.from_numpy(indptr).cuda(), torch.from_numpy(indices).cuda(), vals.cuda(), handle[0], n, n,
                            dtype=dtype)
        _planes[key] = (plane, vals.to(dtype).double())
    return _planes[key]


def _check(out, ref, bound, what):
    assert not torch.isnan(out).any(), f"{what}: {int(torch.isnan(out).any(1).sum())} rows left unwritten"
    if bound is None:
        bad = out.double() != ref
    else:
        bad = (out.double() - ref).abs() > bound
    assert not bad.any(), (f"{what}: {int(bad.sum())} elements wrong in {int(bad.any(1).sum())} rows, first row "
                           f"{int(bad.any(1).nonzero()[0])}, max |err| {float((out.double() - ref).abs().max()):.3e}")


class _Runner:
    """Calls ``spmm_kernel`` on one graph with the forced point and checks that the tuner really used it."""

    def __init__(self, graph, point, width, cid):
        self.graph, self.point, self.width, self.cid = graph, point, width, cid
        self.indptr, self.indices, self.n, self.handle, self.a, self.deg = _graph(graph)

    def __call__(self, variant, feat, out, **kw):
        hspa = self.handle[1]
        hspa.hash_tag = f"tile-matrix:{self.cid}:{self.graph}:{variant}"
        pending = spmm_mod.spmm_kernel(*self.handle, self.n, len(self.indices), self.width, feat, out, **kw)
        keys = {"feature_hash": spmm_mod.feature_hash(hspa), "embedding_dim": self.width, "dtype": str(feat.dtype),
                "device": torch.cuda.get_device_name(feat.device), "two_level": bool(kw.get("beside_panel")),
                "weighted": kw.get("values") is not None}
        if kw.get("row_map") is not None:
            keys["row_map"] = True
        assert jit_tuner.tuned_point("spmm_kernel", keys) == self.point, (self.cid, variant)
        return pending

    def nan_out(self):
        return torch.full((self.n, self.width), float("nan"), device="cuda")


def _binary_point(run, point, flags, kind, first_graph):
    ops = _operands(run.graph, run.width, kind)
    feat, ref, _ = ops["int"]
    out = run.nan_out()
    assert run("plain", feat, out) is None
    _check(out, ref, None, "integer operand")
    for name in ("normal", "extreme"):       # replays of the launch plan: new operand, new output
        if name in ops:
            feat, ref, bound = ops[name]
            out = run.nan_out()
            run("plain", feat, out)
            _check(out, ref, bound, f"{name} operand (replay)")
    if not first_graph:
        return
    feat, ref, _ = ops["int"]
    scale = torch.tensor([OUT_SCALE, 0.0], device="cuda")
    for variant in ("scale", "scale"):        # first call, then its replay
        out = run.nan_out()
        run(variant, feat, out, out_scale=scale)
        _check(out, ref * OUT_SCALE, None, "out_scale")
    if "max_lds" in flags and point["SCHED"] != spmm_mod.SCHED_STREAM:
        prefill = torch.randint(-5, 6, (run.n, run.width), device="cuda").float()
        out = prefill.clone()
        run("atomic", feat, out, atomic_out=True, beside_panel=True)
        _check(out, prefill.double() + ref, None, "atomic_out beside_panel onto a prefill")
    if point["SCHED"] in (spmm_mod.SCHED_UNITS, spmm_mod.SCHED_PAIRS, spmm_mod.SCHED_STREAM):
        out = run.nan_out()
        pending = run("defer", feat, out, defer_combine=True)
        assert pending is not None, "G1 has cut windows: a combine must be pending"
        pending.run()
        _check(out, ref, None, "defer_combine + PendingCombine.run()")
        feat_n, ref_n, bound_n = ops["normal"]    # replay of the deferred plan: new operand, new output, new partial tiles
        out = run.nan_out()
        pending = run("defer", feat_n, out, defer_combine=True)
        assert pending is not None, "G1 has cut windows: a combine must be pending (replay)"
        pending.run()
        _check(out, ref_n, bound_n, "defer_combine + PendingCombine.run() (replay)")
    if point["SCHED"] != spmm_mod.SCHED_STREAM:
        _row_map(run, feat, ref)


def _row_map(run, feat, ref, **kw):
    gen = torch.Generator().manual_seed(run.n)
    perm = torch.randperm(run.n, generator=gen)
    padded = 16 * ((run.n + 15) // 16)
    row_map = torch.cat([perm, torch.full((padded - run.n,), -1, dtype=torch.int64)]).int().cuda()
    out = run.nan_out()
    run("row_map", feat, out, row_map=row_map, **kw)
    want = torch.empty_like(ref)
    want[perm.cuda()] = ref
    _check(out, want, None, "row_map permutation")


def _weighted_point(run, point, kind, first_graph):
    ops = _operands(run.graph, run.width, kind)
    int_plane, int_vals = _plane(run.graph, kind, "int")
    feat, _, _ = ops["int"]
    ref, _ = _oracle(run.a, run.deg, feat, int_vals)
    out = run.nan_out()
    run("plain", feat, out, values=int_plane)
    _check(out, ref, None, "integer values x integer operand")
    feat_n = ops["normal"][0]
    ref_n, bound_n = _oracle(run.a, run.deg, feat_n, int_vals)
    out = run.nan_out()
    run("plain", feat_n, out, values=int_plane)           # replay
    _check(out, ref_n, bound_n, "integer values x normal operand (replay)")
    rnd_plane, rnd_vals = _plane(run.graph, kind, "normal")
    ref_r, bound_r = _oracle(run.a, run.deg, feat_n, rnd_vals)
    out = run.nan_out()
    run("plain", feat_n, out, values=rnd_plane)
    _check(out, ref_r, bound_r, "random values x normal operand")
    if not first_graph:
        return
    out = run.nan_out()
    run("scale", feat, out, values=int_plane, out_scale=torch.tensor([OUT_SCALE, 0.0], device="cuda"))
    _check(out, ref * OUT_SCALE, None, "weighted out_scale")
    if point["SCHED"] == spmm_mod.SCHED_UNITS:
        out = run.nan_out()
        pending = run("defer", feat, out, values=int_plane, defer_combine=True)
        assert pending is not None
        pending.run()
        _check(out, ref, None, "weighted defer_combine")
    _row_map(run, feat, ref, values=int_plane)


@pytest.fixture
def forced_env(cuda_device, monkeypatch, tmp_path):
    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "default")
    monkeypatch.setenv("VOLTRIX_TUNED_DEFAULTS", "0")
    monkeypatch.setenv("VOLTRIX_TUNED_STORE", str(tmp_path / "tuned.json"))
    return monkeypatch


@pytest.mark.parametrize("cid,point,width,flags,policy", CASES, ids=[c[0] for c in CASES])
def test_forced_point_matches_the_oracle(forced_env, cid, point, width, flags, policy):
    forced_env.setattr(spmm_mod, "tile_space", lambda *a, **k: (dict(point),))
    if policy is not None:
        forced_env.setattr(spmm_mod, "SLAB_POLICY", policy)
    kind = tm.kind_of(point)
    for graph in ("cuts", "short"):
        run = _Runner(graph, point, width, cid)
        if point["WEIGHTED"]:
            _weighted_point(run, point, kind, graph == "cuts")
        else:
            _binary_point(run, point, flags, kind, graph == "cuts")
    torch.cuda.synchronize()


@pytest.mark.parametrize("graph", ["cuts", "short"])
@pytest.mark.parametrize("kind", ["f16", "bf16", "f32"])
def test_tuner_sweep_on_adversarial_graphs(forced_env, graph, kind):
    """A real sweep of the default space from an empty store: the tuner's own choice matches the oracle, and no point of the
    space failed to build or returned nonzero."""
    width = max(tm.W16 if kind != "f32" else tm.W32)
    indptr, indices, n, handle, a, deg = _graph(graph)
    ops = _operands(graph, width, kind)
    before = dict(jit_tuner.stats)
    handle[1].hash_tag = f"tile-matrix-sweep:{graph}:{kind}"
    feat, ref, _ = ops["int"]
    out = torch.full((n, width), float("nan"), device="cuda")
    spmm_mod.spmm_kernel(*handle, n, len(indices), width, feat, out)
    _check(out, ref, None, "tuned choice, integer operand")
    feat, ref, bound = ops["normal"]
    out = torch.full((n, width), float("nan"), device="cuda")
    spmm_mod.spmm_kernel(*handle, n, len(indices), width, feat, out)
    _check(out, ref, bound, "tuned choice, normal operand")
    assert jit_tuner.stats["sweeps"] == before["sweeps"] + 1
    assert jit_tuner.stats["timed_candidates"] > before["timed_candidates"]
    assert jit_tuner.stats["build_failures"] == before["build_failures"]
    assert jit_tuner.stats["illegal_candidates"] == before["illegal_candidates"]


FULL_ONLY = tm.full_only_shapes()


@pytest.mark.parametrize("shape", FULL_ONLY, ids=[f"FS{s[0]}-D{s[1]}-W{s[2]}-EB{s[3]}" for s in FULL_ONLY])
def test_full_space_only_shapes_on_cut_windows(forced_env, shape):
    """(FS, DEPTH, WAVES, EB) that only ``VOLTRIX_TUNE_SPACE=full`` offers (compiled here): the unit table for 16-bit operands,
    the chunk-512 balance schedule for fp32 ones, at the widest width, on G1."""
    fs, depth, waves, eb = shape
    point = {"FS": fs, "DEPTH": depth, "WAVES": waves, "EB": eb, "SCHED": 4 if eb == 2 else 2, "BF16": 0, "WEIGHTED": 0}
    forced_env.setattr(spmm_mod, "tile_space", lambda *a, **k: (dict(point),))
    kind = "f16" if eb == 2 else "f32"
    width = max(tm.W16 if eb == 2 else tm.W32)
    compiled = compiler.build_stats["compiled"]
    t0 = time.perf_counter()
    run = _Runner("cuts", point, width, f"full-{fs}-{depth}-{waves}-{eb}")
    ops = _operands("cuts", width, kind)
    for name, (feat, ref, bound) in ops.items():
        out = run.nan_out()
        run("plain", feat, out)
        _check(out, ref, None if name == "int" else bound, f"{name} operand")
    print(f"[full-only {shape}] compiled {compiler.build_stats['compiled'] - compiled} kernel(s), {time.perf_counter() - t0:.1f} s")
