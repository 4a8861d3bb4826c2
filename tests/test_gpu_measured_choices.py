"""GPU: no outcome of a timed choice may change how ``voltrix.spmm`` rounds B.

The operators make three measured choices -- CSR row-gather kernel or block format (``_csr_choice``), window or two-level format
(``VOLTRIX_HYBRID=tune``: ``_choose_format``), CSR kernel with values or value plane (``weighted._weighted_path``).  Every outcome is
FORCED here, where the code reads it (``csr.choice``, ``two.format_choice``, ``handle.path_choice``), through a scripted stopwatch, through
the tuned store and through a stream capture, and every outcome is compared with a float64 ``torch.sparse`` product on the CPU under the
bound of its own class; the two outcomes of one choice are compared with each other under the sum of the two accumulation bounds, which an
fp16 rounding of B on one side misses by an order of magnitude (graphs, bounds: tests/measured_choice_cases.py)."""
import json

import pytest
import torch

import measured_choice_cases as mc
import synth_graphs
import voltrix
from measured_choice_cases import DT, N, U, WIDTHS
from stream_cases import capture_and_replay
from test_gpu_spmm import _assert_close
from voltrix import capi, sidecar, weighted

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _environment(monkeypatch, tmp_path):
    """The measured choices as a default process meets them, on a tuned store of this test's own."""
    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "default")       # "none" / "stream" pin the block-format kernel: no measured choice then
    monkeypatch.setenv("VOLTRIX_TUNED_STORE", str(tmp_path / "tuned.json"))
    for flag in ("VOLTRIX_FP32_MODE", "VOLTRIX_CSR_PATH", "VOLTRIX_HYBRID", "VOLTRIX_HYBRID_MIN_SHARE", "VOLTRIX_FUSED"):
        monkeypatch.delenv(flag, raising=False)


def _handle(name, tag):
    """A fresh handle of a graph, with its CSR side-car and the class the graph was made for at every width."""
    indptr, indices = (torch.from_numpy(a) for a in mc.graph(name))
    handle = voltrix.csr_preprocess(indptr, indices, N)
    handle[1].hash_tag = tag
    csr = sidecar.lookup_csr(handle[1])
    assert csr is not None and csr.num_rows == N and csr.indices.numel() == indices.numel() and csr.choice == {}
    operator = mc.operator_module()
    assert all(operator.fp32_mode(handle[1], N, width) == mc.CLASS[name] for width in WIDTHS)
    return handle, csr


_SHARED = {}


def _shared_handle(name):
    """One handle per graph for the cases that force ``csr.choice`` themselves (the tile choices of its block path are made once)."""
    if name not in _SHARED:
        _SHARED[name] = _handle(name, f"measured/{name}")
    return _SHARED[name]


def _edges(handle):
    return sidecar.lookup_csr(handle[1]).indices.numel()


def _product(handle, feat):
    return voltrix.spmm(*handle, num_nodes=N, num_edges=_edges(handle), feat=feat)


class _CsrLaunches:
    """Spy on ``capi.launch_spmm_csr_rows``: the ``indptr`` address of every launch."""

    def __init__(self, monkeypatch):
        self.pointers = []
        inner = capi.launch_spmm_csr_rows

        def wrapper(indptr, *args, **kwargs):
            self.pointers.append(indptr.data_ptr())
            return inner(indptr, *args, **kwargs)

        monkeypatch.setattr(capi, "launch_spmm_csr_rows", wrapper)

    def take(self):
        seen, self.pointers = self.pointers, []
        return seen


def _candidate(name, dtype):
    """Whether the CSR kernel reads the operand the class prescribes: not where the class rounds fp32 rows to fp16."""
    return not (dtype == "fp32" and mc.CLASS[name] == "fp16")


# ------------------------------------------------------------------------------------------------------- the binary operator, forced
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("name", ["G_exact", "G_cast"])
def test_both_outcomes_of_the_csr_choice_are_of_one_class(cuda_device, name, dtype, width, monkeypatch):
    """``csr.choice`` forced to "csr" and to "block": each within its class bound of the oracle on the operand the class prescribes, the
    two within fp32 summation order of each other; ``VOLTRIX_CSR_PATH=0 / 1`` as the cross-check.  Where the class rounds fp32 rows to
    fp16 the CSR kernel is no candidate: a remembered "csr" is not obeyed."""
    handle, csr = _shared_handle(name)
    spy = _CsrLaunches(monkeypatch)
    feat, ref = mc.features(width, dtype).cuda(), mc.reference(name, width, dtype)
    key, what = (width, str(DT[dtype])), f"{name} {dtype} F={width}"
    got = {}
    for outcome in ("block", "csr"):
        csr.choice[key] = outcome
        got[outcome] = _product(handle, feat)
        assert got[outcome].shape == (N, width) and got[outcome].dtype == torch.float32
        ran_csr = spy.take() == [csr.indptr.data_ptr()]
        assert ran_csr == (outcome == "csr" and _candidate(name, dtype)), (what, outcome)
        mc.check_outcome(outcome if ran_csr else "block", got[outcome], ref, what)
    mc.check_pair(got["csr"], got["block"], ref, what)
    del csr.choice[key]
    monkeypatch.setenv("VOLTRIX_CSR_PATH", "0")
    assert torch.equal(_product(handle, feat), got["block"]) and spy.take() == []
    monkeypatch.setenv("VOLTRIX_CSR_PATH", "1")               # the environment may pin the kernel: the rows as given, whatever the class
    pinned = _product(handle, feat)
    assert spy.take() == [csr.indptr.data_ptr()] and key not in csr.choice
    if _candidate(name, dtype):
        assert torch.equal(pinned, got["csr"])
    else:
        err = (pinned.cpu().double() - ref.given).abs()
        assert mc.ratio(err, (ref.deg + 1) * U * ref.mass) <= 1.0


# ------------------------------------------------------------------------------------------------------------------- the stopwatch
SCRIPTS = {"csr wins": ({"block": 1.0, "csr": 0.5}, "csr"), "block wins": ({"block": 0.5, "csr": 1.0}, "block"),
           "within 3 %": ({"block": 1.0, "csr": 0.98}, "block")}


@pytest.mark.parametrize("script", list(SCRIPTS))
@pytest.mark.parametrize("name,dtype", [("G_exact", "fp32"), ("G_cast", "fp16"), ("G_cast", "fp32")])
def test_scripted_stopwatch_of_the_csr_choice(cuda_device, name, dtype, script, monkeypatch):
    """The clock scripted: the recorded choice, nothing timed again on the second call, the result within its class bound.  fp32 rows
    that the class rounds: nothing is timed and nothing recorded whatever the clock would say."""
    times, expected = SCRIPTS[script]
    watch = mc.Stopwatch(times)
    monkeypatch.setattr(mc.operator_module(), "_time_ms", watch)
    spy = _CsrLaunches(monkeypatch)
    handle, csr = _handle(name, f"measured/stopwatch/{name}/{dtype}/{script}")
    width = 40
    feat, ref = mc.features(width, dtype).cuda(), mc.reference(name, width, dtype)
    key = (width, str(DT[dtype]))
    first = _product(handle, feat)
    if not _candidate(name, dtype):
        assert watch.calls == [] and csr.choice == {} and spy.take() == []
        mc.check_block(first, ref, f"{name} {dtype} {script}")
        return
    assert watch.calls == ["block", "csr"] and csr.choice == {key: expected}
    spy.take()
    second = _product(handle, feat)
    assert watch.calls == ["block", "csr"] and csr.choice == {key: expected}
    assert (spy.take() == [csr.indptr.data_ptr()]) == (expected == "csr")
    assert torch.equal(first, second)
    mc.check_outcome(expected, second, ref, f"{name} {dtype} {script}")


def test_a_candidate_that_raises_leaves_no_state_behind(cuda_device, monkeypatch):
    """An exception out of a timed candidate: no choice recorded, nothing stored, and the next call measures and works -- for the binary
    operator and for the weighted one."""
    operator = mc.operator_module()
    watch = mc.Stopwatch({"block": 1.0, "csr": 0.5, "plane": 1.0})
    monkeypatch.setattr(operator, "_time_ms", watch)
    handle, csr = _handle("G_exact", "measured/raises")
    feat, ref = mc.features(40, "fp32").cuda(), mc.reference("G_exact", 40, "fp32")

    def broken(*args, **kwargs):
        raise RuntimeError("candidate failed")

    with monkeypatch.context() as patch:
        patch.setattr(operator, "_spmm_csr", broken)
        with pytest.raises(RuntimeError, match="candidate failed"):
            _product(handle, feat)
    assert csr.choice == {} and not hasattr(operator, "_CSR_DEPTH")
    assert not any(k.startswith("spmm_csr_path") for k in operator_store())
    mc.check_csr(_product(handle, feat), ref, "after a failed candidate")
    assert csr.choice == {(40, str(torch.float32)): "csr"} and watch.calls == ["block", "csr", "block", "csr"]

    wh, values = _weighted_handle()
    with monkeypatch.context() as patch:
        patch.setattr(weighted, "_spmm_weighted_csr", broken)
        with pytest.raises(RuntimeError, match="candidate failed"):
            voltrix.spmm_weighted(wh, feat)
    assert wh.path_choice == {}
    out = voltrix.spmm_weighted(wh, feat)
    assert wh.path_choice == {(40, str(torch.float32)): "csr"}
    _check_weighted("csr", out, values, mc.features(40, "fp32"), "weighted after a failed candidate")


def operator_store():
    from voltrix.jit_kernels import jit_tuner

    return jit_tuner._read(jit_tuner._store_path())


# --------------------------------------------------------------------------------------------------------------- the persisted choice
def _store_key(handle, width, dtype, klass):
    from voltrix.jit_kernels.spmm import feature_hash

    head = (f"spmm_csr_path|{{'device': '{torch.cuda.get_device_name(handle[1].device)}', 'dtype': '{DT[dtype]}', "
            f"'embedding_dim': {width}, 'feature_hash': '{feature_hash(handle[1])}'")
    return head + (f", 'operand': '{klass}'}}" if klass else "}")


def _write_store(path, entries):
    with open(path, "w") as f:
        json.dump(entries, f)


def test_persisted_choice_is_read_validated_and_carries_the_class(cuda_device, monkeypatch, tmp_path):
    monkeypatch.setenv("VOLTRIX_TUNED_DEFAULTS", "0")
    store = str(tmp_path / "tuned.json")
    operator = mc.operator_module()
    spy = _CsrLaunches(monkeypatch)
    width, key = 40, (40, str(torch.float32))
    feat, ref = mc.features(width, "fp32").cuda(), mc.reference("G_exact", width, "fp32")
    tag = "measured/persisted/G_exact"

    def fresh(script):
        watch = mc.Stopwatch(script)
        monkeypatch.setattr(operator, "_time_ms", watch)
        return _handle("G_exact", tag) + (watch,)

    # a measured choice is written under a key that names the class
    handle, csr, watch = fresh({"block": 1.0, "csr": 0.5})
    mc.check_csr(_product(handle, feat), ref, "measured, then stored")
    assert watch.calls == ["block", "csr"]
    assert operator_store().get(_store_key(handle, width, "fp32", "exact")) == "csr"
    # a second handle object with the same tag takes the stored choice without timing -- either value
    for stored in ("csr", "block"):
        entries = operator_store()
        entries[_store_key(handle, width, "fp32", "exact")] = stored
        _write_store(store, entries)
        handle, csr, watch = fresh({"block": 0.5, "csr": 1.0} if stored == "csr" else {"block": 1.0, "csr": 0.5})
        spy.take()
        out = _product(handle, feat)
        assert watch.calls == [] and csr.choice == {key: stored}
        assert (spy.take() == [csr.indptr.data_ptr()]) == (stored == "csr")
        mc.check_outcome(stored, out, ref, f"stored {stored}")
    # a stored value that is no candidate of this choice is ignored: measured again
    entries[_store_key(handle, width, "fp32", "exact")] = "plane"
    _write_store(store, entries)
    handle, csr, watch = fresh({"block": 0.5, "csr": 1.0})
    mc.check_block(_product(handle, feat), ref, "invalid stored value")
    assert watch.calls == ["block", "csr"] and csr.choice == {key: "block"}
    # fp32 rows that the class rounds: a stored "csr" -- under the key of before the class was part of it, or under today's -- names a
    # candidate the class does not allow and is not obeyed
    cast_ref = mc.reference("G_cast", width, "fp32")
    watch = mc.Stopwatch({})
    monkeypatch.setattr(operator, "_time_ms", watch)
    handle, csr = _handle("G_cast", "measured/persisted/G_cast")
    _write_store(store, {_store_key(handle, width, "fp32", None): "csr", _store_key(handle, width, "fp32", "fp16"): "csr",
                         _store_key(handle, width, "fp32", "exact"): "csr"})
    spy.take()
    out = _product(handle, feat)
    assert watch.calls == [] and spy.take() == [] and csr.choice == {}
    mc.check_block(out, cast_ref, "stored csr against the class")


# ------------------------------------------------------------------------------------------------------------------------- capture
@pytest.mark.parametrize("name", ["G_cast", "G_exact"])
def test_capture_fixes_no_other_rounding_than_eager(cuda_device, name, monkeypatch):
    """A handle without a decision whose first product under the measured choice happens inside a stream capture (the block path is
    taken, nothing is recorded), replayed on a second set of values: within fp32 summation order of the eager result with the choice
    "csr" and of the one with "block".  The same through ``voltrix.GraphedSpMM``."""
    width, dtype = 128, "fp32"
    key = (width, str(DT[dtype]))
    handle, csr = _handle(name, f"measured/capture/{name}")
    feats = [mc.features(width, dtype, seed).cuda() for seed in (0, 1)]
    refs = [mc.reference(name, width, dtype, seed) for seed in (0, 1)]
    monkeypatch.setenv("VOLTRIX_CSR_PATH", "0")          # tile choices, tables and plans of the block path: made outside the capture
    _product(handle, feats[0])
    monkeypatch.delenv("VOLTRIX_CSR_PATH")
    assert csr.choice == {}
    first, second = capture_and_replay(lambda feat: (_product(handle, feat),), [feats[0]], [feats[1]])
    assert csr.choice == {}                               # no decision was made under capture
    captured = [first[0], second[0].clone()]
    graphed_handle, graphed_csr = _handle(name, f"measured/graphed/{name}")
    op = voltrix.GraphedSpMM(*graphed_handle, N, _edges(graphed_handle), feats[0])
    graphed = [op(feat).clone() for feat in feats]
    eager = {}
    for outcome in ("csr", "block"):
        csr.choice[key] = outcome
        eager[outcome] = [_product(handle, feat) for feat in feats]
    for k in (0, 1):
        mc.check_block(captured[k], refs[k], f"captured {name} values {k}")
        for outcome in ("csr", "block"):
            mc.check_pair(captured[k], eager[outcome][k], refs[k], f"captured {name} values {k} against eager {outcome}")
            mc.check_pair(graphed[k], eager[outcome][k], refs[k], f"GraphedSpMM {name} values {k} against eager {outcome}")


# --------------------------------------------------------------------------------------------------------------------- re-entrancy
def test_a_product_issued_while_another_handle_is_timed_keeps_its_csr_kernel(cuda_device, monkeypatch):
    """Handle A is being timed; a ``voltrix.spmm`` on handle B, whose choice is "csr", still runs the CSR kernel on B's own CSR."""
    operator = mc.operator_module()
    a, a_csr = _handle("G_exact", "measured/reentrant/A")
    b, b_csr = _handle("G_cast", "measured/reentrant/B")
    feat_a, feat_b = mc.features(40, "fp32").cuda(), mc.features(128, "fp16").cuda()
    b_csr.choice[(128, str(torch.float16))] = "csr"
    spy = _CsrLaunches(monkeypatch)
    inside = {}

    def during():
        spy.take()
        inside["out"] = _product(b, feat_b)
        inside["launches"] = spy.take()

    watch = mc.Stopwatch({"block": 1.0, "csr": 0.5}, during=during)
    monkeypatch.setattr(operator, "_time_ms", watch)
    out_a = _product(a, feat_a)
    assert watch.calls == ["block", "csr"] and a_csr.choice == {(40, str(torch.float32)): "csr"}
    assert inside["launches"] == [b_csr.indptr.data_ptr()] and b_csr.indptr.data_ptr() != a_csr.indptr.data_ptr()
    mc.check_csr(inside["out"], mc.reference("G_cast", 128, "fp16"), "B while A is timed")
    mc.check_csr(out_a, mc.reference("G_exact", 40, "fp32"), "A")
    assert not hasattr(operator, "_CSR_DEPTH")


# ------------------------------------------------------------------------------------------------------------ VOLTRIX_HYBRID=tune
@pytest.mark.parametrize("dtype,mode", [("fp16", "fp16"), ("fp32", "fp16-scaled")])
@pytest.mark.parametrize("width", [128, 200])
def test_both_formats_of_the_tuned_hybrid_read_one_operand(cuda_device, dtype, mode, width, monkeypatch):
    """``VOLTRIX_HYBRID=tune`` on a small two-level handle: the stopwatch's verdict is recorded and not asked for again; "window" and
    "two-level" forced each meet the bound tests/test_gpu_hybrid.py states, and differ by at most the two accumulation terms -- the cast
    operand is the same in both."""
    from oracle import torch_ref

    monkeypatch.setenv("VOLTRIX_HYBRID", "tune")
    monkeypatch.setenv("VOLTRIX_HYBRID_MIN_SHARE", "0")
    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "none")
    for limit, value in (("AUTO_MIN_EDGES", 1), ("AUTO_MIN_ROWS", 1), ("AUTO_MIN_MEAN_DEGREE", 0)):
        monkeypatch.setattr(voltrix.hybrid, limit, value)
    indptr, indices, _ = synth_graphs.generate("products_like", scale=0.01)      # 24 k rows, 1.2 M edges: most of them on either side
    n, e = indptr.numel() - 1, indices.numel()
    handle = voltrix.csr_preprocess(indptr, indices, n)
    handle[1].hash_tag = f"measured/tune/{dtype}/{width}"
    two = voltrix.two_level_of(handle[1])
    assert two is not None and two.plan.num_shared_edges > 0 and two.plan.num_resid_edges > 0 and two.format_choice == {}
    assert sidecar.lookup_csr(handle[1]) is None
    torch.manual_seed(width)
    feat32 = torch.randn(n, width).to(DT[dtype]).float()
    feat = feat32.to(DT[dtype]).cuda()
    watch = mc.Stopwatch({"window": 1.0, "two-level": 0.5})
    monkeypatch.setattr(mc.operator_module(), "_time_ms", watch)
    out = voltrix.spmm(*handle, num_nodes=n, num_edges=e, feat=feat)
    padded = (width + 7) // 8 * 8
    key = (padded, str(torch.float16))
    assert watch.calls == ["window", "two-level"] and two.format_choice == {key: "two-level"}
    _assert_close(out, indptr.numpy(), indices.numpy(), feat32, n, mode)
    got = {}
    for form in ("window", "two-level"):
        two.format_choice[key] = form
        with voltrix.utils.KernelTimer() as timer:
            got[form] = voltrix.spmm(*handle, num_nodes=n, num_edges=e, feat=feat)
        assert any("spmm_panel" in k for k in timer.summary()) == (form == "two-level")
        _assert_close(got[form], indptr.numpy(), indices.numpy(), feat32, n, mode)
    assert watch.calls == ["window", "two-level"]
    rounded = torch_ref.round_fp16_scaled(feat32) if dtype == "fp32" else feat32
    ones = torch.ones(e, dtype=torch.float64)
    mass = torch.sparse_csr_tensor(indptr, indices, ones, size=(n, n)) @ rounded.double().abs()
    deg = (indptr[1:] - indptr[:-1]).double()[:, None]
    diff = (got["window"].cpu().double() - got["two-level"].cpu().double()).abs()
    worst = float((diff / (2 * deg * U * mass + 1e-30)).max())
    print(f"tune {dtype} F={width}: pair max diff / bound = {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------------------ weighted
def _weighted_values():
    gen = torch.Generator().manual_seed(7)
    return torch.rand(len(mc.graph("G_exact")[1]), generator=gen) + 0.1


def _weighted_handle():
    indptr, indices = (torch.from_numpy(a) for a in mc.graph("G_exact"))
    values = _weighted_values()
    handle = voltrix.csr_preprocess_weighted(indptr, indices, values, N, separable=False)
    handle.hspa_packed.hash_tag = "measured/weighted"
    assert not handle.separable and handle.csr is not None and handle.path_choice == {}
    assert handle.hspa_packed.numel() // 4 <= weighted.WEIGHTED_CSR_MAX_BLOCKS_PER_WINDOW * ((N + 15) // 16)
    return handle, values


def _check_weighted(path, out, values, feat, what):
    """Each path against ITS OWN bound: "csr" -- fp32 values, one fused multiply-add per element: (deg + 1) 2^-23 (|A| |B|) on the
    operand as given; "plane" -- values and an fp32 B rounded to 16 bits: the bound of
    tests/test_gpu_weighted.py::test_weighted_spmm_matches_the_oracle for the dtype."""
    ref = mc.adjacency("G_exact", values) @ feat.double()
    mass = mc.adjacency("G_exact", values.abs()) @ feat.double().abs()
    deg = mc.degrees("G_exact")
    err = (out.cpu().double() - ref).abs()
    assert not torch.isnan(out).any()
    if path == "csr":
        bound = (deg + 1) * U * mass + 1e-30
    else:
        bound = ((2.0 ** -7 if feat.dtype == torch.bfloat16 else 2.0 ** -10) + (deg + 1) * U) * mass + 1e-6
    worst = float((err / bound).max())
    print(f"{what} {path}: max err / bound = {worst:.3f}")
    assert worst <= 1.0, (what, path, worst)


@pytest.mark.parametrize("width", [40, 128])
@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
def test_each_weighted_path_meets_its_own_bound(cuda_device, dtype, width, monkeypatch):
    """``handle.path_choice`` forced to "csr" and to "plane"; then the stopwatch scripted: the recorded choice, no second timing.  The
    plane rounds the values to 16 bits and the CSR kernel does not: the class of ``spmm_weighted`` is keyed on the recorded choice."""
    handle, values = _weighted_handle()
    spy = _CsrLaunches(monkeypatch)
    feat_cpu = mc.features(width, dtype)
    feat, key = feat_cpu.cuda(), (width, str(DT[dtype]))
    for path in ("csr", "plane"):
        handle.path_choice[key] = path
        out = voltrix.spmm_weighted(handle, feat)
        assert (spy.take() == [handle.csr[0].data_ptr()]) == (path == "csr")
        _check_weighted(path, out, values, feat_cpu, f"weighted {dtype} F={width}")
    for script, expected in (({"plane": 1.0, "csr": 0.5}, "csr"), ({"plane": 0.5, "csr": 1.0}, "plane"),
                             ({"plane": 1.0, "csr": 0.98}, "plane")):
        watch = mc.Stopwatch(script)
        monkeypatch.setattr(mc.operator_module(), "_time_ms", watch)
        handle.path_choice.clear()
        first = voltrix.spmm_weighted(handle, feat)
        assert watch.calls == ["plane", "csr"] and handle.path_choice == {key: expected}
        assert torch.equal(first, voltrix.spmm_weighted(handle, feat)) and watch.calls == ["plane", "csr"]
        _check_weighted(expected, first, values, feat_cpu, f"weighted {dtype} F={width} scripted")


# ---------------------------------------------------------------------------------------------------------------- the owned side-car
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_the_handle_owns_its_csr_side_car(cuda_device, dtype, monkeypatch):
    """``csr_preprocess_device`` keeps a copy of the CSR it attaches: a caller that reuses its ``indices`` buffer (other in-range ids,
    the row pointers untouched) changes neither the CSR path nor the block path -- both give the product of the ORIGINAL graph."""
    indptr_np, indices_np = mc.graph("G_exact")
    indptr, indices = torch.from_numpy(indptr_np).cuda(), torch.from_numpy(indices_np).cuda()
    handle = voltrix.csr_preprocess_device(indptr, indices, N)
    handle[1].hash_tag = "measured/owned"
    csr = sidecar.lookup_csr(handle[1])
    assert csr is not None and csr.indices.data_ptr() != indices.data_ptr() and csr.indptr.data_ptr() != indptr.data_ptr()
    indices.copy_((indices + 1) % N)
    assert int(indices.min()) >= 0 and int(indices.max()) < N
    spy = _CsrLaunches(monkeypatch)
    gen = torch.Generator().manual_seed(5)
    ints = torch.randint(-3, 4, (N, 40), generator=gen).to(DT[dtype])
    want = (mc.adjacency("G_exact") @ ints.double()).float()
    for outcome in ("csr", "block"):
        csr.choice[(40, str(DT[dtype]))] = outcome
        out = _product(handle, ints.cuda())
        assert (spy.take() == [csr.indptr.data_ptr()]) == (outcome == "csr")
        assert torch.equal(out.cpu(), want), outcome
    assert torch.equal(csr.indices.cpu(), torch.from_numpy(indices_np))
