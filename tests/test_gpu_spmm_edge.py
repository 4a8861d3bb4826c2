"""GPU: ``voltrix.spmm_edge`` (mul / add / add_relu / copy over every row's entries, a feature vector per entry), both its gradients
and ``voltrix.autograd.SpMMEdge`` against the numpy float64 oracle of tests/spmm_edge_oracle.py, from the inputs as stored (fp32, fp16
and bf16 convert to float64 exactly).  Every comparison is over every element.

Bounds, with ``u = 2^-23``.  Forward and ``grad_feat``: ``|out - ref| <= (k + 1) u sum |terms|`` for the ``k`` terms of an element -- each
term takes one rounding (within 2^-24 of it) and there are ``k - 1`` fp32 additions, so the first-order error is ``k 2^-24 sum |terms|``
and the bound is twice that, with or without contraction of a product into the sum.  ``grad_efeat``: equal to the oracle for add, copy
and add_relu (the gate has the sign of the exact sum, the result is ``g`` or 0), ``|ge - ref| <= u |ref|`` for mul.  Integer-valued
inputs in [-3, 3]: equality everywhere.
"""
import numpy as np
import pytest
import torch

import spmm_edge_oracle as oracle
from conftest import load_csr_fixture
from poisoned_alloc import poisoned

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
DEV = "cuda"
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
HALF_ULP = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
PAIRS = [("fp32", "fp32"), ("fp16", "fp16"), ("bf16", "bf16"), ("fp32", "fp16"), ("fp32", "bf16")]          # (feat, efeat)
OPS = ("mul", "add", "add_relu", "copy")


# ------------------------------------------------------------------------------------------------------------------- the patterns
class Pattern:
    """A CSR on the host (numpy) and on the device (int32), with its transpose by a stable sort by column."""

    def __init__(self, lengths, cols, num_cols):
        lengths, cols = np.asarray(lengths, np.int64), np.asarray(cols, np.int64)
        self.num_rows, self.num_cols, self.nnz = len(lengths), int(num_cols), int(lengths.sum())
        assert cols.size == self.nnz
        self.lengths, self.ip, self.cols = lengths, np.concatenate([[0], np.cumsum(lengths)]), cols
        self.rows = np.repeat(np.arange(self.num_rows), lengths)
        self.t = oracle.transpose(self.ip, cols, self.num_cols)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(DEV)     # noqa: E731
        self.indptr, self.indices = dev(self.ip), dev(cols)
        self.t_indptr, self.t_indices, self.t_order = (dev(x) for x in self.t)


_CACHE = {}


def _pattern_a():
    """203 rows (a multiple of no rows-per-group count) x 150 columns: row lengths on both sides of the 4-entry batch, one hub row of
    1,031 entries, the rest 0 .. 12; columns sorted inside a row, duplicates present (the hub holds every column about 7 times)."""
    if "a" not in _CACHE:
        rng = np.random.default_rng(17)
        lengths = [0, 1, 2, 3, 4, 5, 7, 8, 9, 0, 6, 1] + [int(v) for v in rng.integers(0, 13, 90)] + [1031]
        lengths += [int(v) for v in rng.integers(0, 13, 203 - len(lengths))]
        lengths = np.asarray(lengths, np.int64)
        assert len(lengths) == 203 and all(203 % r for r in (4, 8, 16, 32, 64, 128, 256))
        rows = np.repeat(np.arange(203), lengths)
        cols = np.sort(rows * 150 + rng.integers(0, 150, rows.size)) % 150
        assert len(np.unique(rows * 150 + cols)) < rows.size - 500                     # duplicates are present
        _CACHE["a"] = Pattern(lengths, cols, 150)
    return _CACHE["a"]


def _pattern_b():
    if "b" not in _CACHE:
        g = load_csr_fixture("toy40")
        ip = np.asarray(g["indptr"], np.int64)
        _CACHE["b"] = Pattern(ip[1:] - ip[:-1], g["indices"], int(g["num_nodes"]))
    return _CACHE["b"]


# --------------------------------------------------------------------------------------------------------------------- the inputs
def _inputs(p, tail, pair, kind, seed=0):
    """``(feat [num_cols, *tail], efeat [nnz, *tail], grad_out [num_rows, *tail] fp32)`` on the device.  "normal"; "ints": integers in
    [-3, 3] (zeros of x + w are many); "zeros": normal with ``efeat[e] = -feat[col_e]`` planted on about a fifth of the elements, in the
    stored types, so x + w is exactly 0 there; "special": normal with NaN, +inf and -inf sprinkled into both operands."""
    gen = torch.Generator(device=DEV).manual_seed(4000 + seed)
    fdt, edt = DT[pair[0]], DT[pair[1]]
    tail = tuple(tail)
    if kind == "ints":
        draw = lambda n: torch.randint(-3, 4, (n,) + tail, device=DEV, generator=gen).float()      # noqa: E731
    else:
        draw = lambda n: torch.randn((n,) + tail, device=DEV, generator=gen)                       # noqa: E731
    feat, efeat, grad = draw(p.num_cols).to(fdt), draw(p.nnz).to(edt), draw(p.num_rows)
    if kind == "zeros" and p.nnz:
        low = feat.to(edt)                                    # a value both types hold: x = low exactly, w = -low
        feat = low.to(fdt)
        plant = torch.rand((p.nnz,) + tail, device=DEV, generator=gen) < 0.2
        efeat = torch.where(plant, -low[p.indices.long()], efeat)
        assert bool(((feat.double()[p.indices.long()] + efeat.double()) == 0).any())
    if kind == "special":
        for t in (feat, efeat):
            dice = torch.rand(t.shape, device=DEV, generator=gen)
            t[dice < 0.01] = float("nan")
            t[(dice >= 0.01) & (dice < 0.02)] = float("inf")
            t[(dice >= 0.02) & (dice < 0.03)] = float("-inf")
    return feat, efeat, grad


def _np(t):
    return t.detach().double().cpu().numpy()


def _within(got, ref, bound, what):
    err = np.abs(_np(got).reshape(ref.shape) - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: max err / bound = {worst:.3f}")
    assert bool((err <= bound).all()), (what, worst)


# --------------------------------------------------------------------------------------------------------------------- the checks
def _check_forward(p, feat, efeat, exact, what):
    import voltrix

    for op in OPS:
        out = voltrix.spmm_edge(p.indptr, p.indices, None if op == "copy" else feat, efeat, p.num_rows, op=op)
        assert out.dtype == torch.float32 and out.shape == (p.num_rows,) + tuple(efeat.shape[1:])
        ref, mass, count = oracle.forward(p.ip, p.cols, None if op == "copy" else _np(feat), _np(efeat), op)
        if exact:
            assert np.array_equal(_np(out).reshape(ref.shape), ref), (what, op)
        _within(out, ref, (count[:, None] + 1) * U * mass, f"forward {op} {what}")
        assert bool((out[torch.from_numpy(p.lengths == 0).to(DEV)] == 0).all())


def _check_gradients(p, feat, efeat, grad, exact, what):
    from voltrix.spmm_edge import grad_efeat, grad_feat

    for op in OPS:
        f = None if op == "copy" else feat
        ge = grad_efeat(p.indptr, p.indices, grad, f, efeat, op)
        assert ge.dtype == torch.float32 and ge.shape == tuple(efeat.shape)
        ref = oracle.grad_efeat(p.ip, p.cols, _np(grad), None if f is None else _np(f), _np(efeat), op)
        if op == "mul" and not exact:
            _within(ge, ref, U * np.abs(ref), f"grad_efeat mul {what}")
        else:
            assert np.array_equal(_np(ge).reshape(ref.shape), ref), (what, op)
        if op == "copy":
            continue
        gf = grad_feat(p.t_indptr, p.t_indices, p.t_order, grad, feat, efeat, op, p.num_cols)
        assert gf.dtype == torch.float32 and gf.shape == (p.num_cols,) + tuple(efeat.shape[1:])
        ref, mass, count = oracle.grad_feat(p.ip, p.cols, _np(grad), _np(feat), _np(efeat), op, p.num_cols)
        if exact:
            assert np.array_equal(_np(gf).reshape(ref.shape), ref), (what, op)
        _within(gf, ref, (count[:, None] + 1) * U * mass, f"grad_feat {op} {what}")


# 260 (fp32) and 520 (16-bit): the first lane of the second slab; 1 / 12 / 20: padded for one type or both
WIDTHS = {"fp32": ((1,), (4,), (12,), (20,), (64,), (260,), (3, 8)), "fp16": ((1,), (4,), (12,), (20,), (64,), (520,), (3, 8)),
          "bf16": ((12,), (64,), (520,), (3, 8))}
CASES = [(pair, tail) for pair in PAIRS for tail in (WIDTHS[pair[1]] if pair[0] == pair[1] else ((12,), (64,), (520,)))]


@pytest.mark.parametrize("pair,tail", CASES, ids=[f"{a}-{b}-{'x'.join(map(str, t))}" for (a, b), t in CASES])
def test_forward_and_both_gradients_on_pattern_a(cuda_device, pair, tail):
    p = _pattern_a()
    for kind in ("normal", "ints", "zeros"):
        feat, efeat, grad = _inputs(p, tail, pair, kind, seed=sum(tail))
        if kind == "ints":
            grad = grad.round()
        what = f"{pair} {tail} {kind}"
        _check_forward(p, feat, efeat, kind == "ints", what)
        _check_gradients(p, feat, efeat, grad, kind == "ints", what)


@pytest.mark.parametrize("pair", PAIRS, ids=["-".join(pair) for pair in PAIRS])
def test_forward_and_both_gradients_on_the_fixture_pattern(cuda_device, pair):
    p = _pattern_b()
    for kind in ("normal", "ints", "zeros"):
        feat, efeat, grad = _inputs(p, (24,), pair, kind, seed=3)
        if kind == "ints":
            grad = grad.round()
        _check_forward(p, feat, efeat, kind == "ints", f"toy40 {pair} {kind}")
        _check_gradients(p, feat, efeat, grad, kind == "ints", f"toy40 {pair} {kind}")


@pytest.mark.parametrize("pair", [("fp32", "fp32"), ("fp16", "fp16"), ("fp32", "bf16")], ids=["fp32", "fp16", "fp32-bf16"])
def test_nan_and_inf_propagate_as_the_arithmetic_does(cuda_device, pair):
    """torch float64 on the device: ``zeros.index_add_(0, rows, m(feat[cols], efeat))`` with ``torch.relu``; a NaN equals a NaN, an inf
    the inf of its sign, and every finite element is within the bound."""
    import voltrix

    p = _pattern_a()
    feat, efeat, _ = _inputs(p, (20,), pair, "special", seed=8)
    rows, cols = torch.from_numpy(p.rows).to(DEV), torch.from_numpy(p.cols).to(DEV)
    x, w = feat.double()[cols], efeat.double()
    seen_nan = False
    for op, terms in (("mul", x * w), ("add", x + w), ("add_relu", torch.relu(x + w)), ("copy", w)):
        zeros = lambda: torch.zeros(p.num_rows, 20, dtype=torch.float64, device=DEV)     # noqa: E731
        ref = zeros().index_add_(0, rows, terms)
        bound = (torch.from_numpy(p.lengths).to(DEV)[:, None] + 1) * U * zeros().index_add_(0, rows, terms.abs())
        out = voltrix.spmm_edge(p.indptr, p.indices, None if op == "copy" else feat, efeat, p.num_rows, op=op).double()
        ok = ((out - ref).abs() <= bound) | (out == ref) | (out.isnan() & ref.isnan())
        assert bool(ok.all()), (op, int((~ok).sum()))
        assert torch.equal(out.isnan(), ref.isnan()) and torch.equal(out.isinf(), ref.isinf())
        seen_nan |= bool(ref.isnan().any()) and bool(ref.isinf().any()) and bool(ref.isfinite().any())
    assert seen_nan
    # max(NaN + w, 0) is NaN: one entry, one NaN
    one = Pattern([1], [0], 1)
    nan = torch.full((1, 4), float("nan"), device=DEV)
    assert bool(voltrix.spmm_edge(one.indptr, one.indices, nan, torch.ones(1, 4, device=DEV), 1, op="add_relu").isnan().all())
    assert bool(voltrix.spmm_edge(one.indptr, one.indices, torch.ones(1, 4, device=DEV), nan, 1, op="add_relu").isnan().all())


# ------------------------------------------------------------------------------------------------------------------------ autograd
def _composite(p, feat64, efeat64, op):
    rows, cols = torch.from_numpy(p.rows).to(DEV), torch.from_numpy(p.cols).to(DEV)
    if op == "copy":
        terms = efeat64
    else:
        x = feat64[cols]
        terms = x * efeat64 if op == "mul" else x + efeat64 if op == "add" else torch.relu(x + efeat64)
    return torch.zeros((p.num_rows,) + tuple(efeat64.shape[1:]), dtype=torch.float64, device=DEV).index_add_(0, rows, terms)


@pytest.mark.parametrize("pair", PAIRS, ids=["-".join(pair) for pair in PAIRS])
def test_autograd_operator_against_torch_float64_autograd(cuda_device, pair):
    """Gradients of ``(out * R).sum()`` for a fixed random R, against float64 autograd of the composite ``index_add_(m(feat[cols],
    efeat))``.  fp32 operands: the bounds of the module's docstring.  A 16-bit operand's gradient is cast to its type at the end: the
    type's half-ulp, ``2^-11 |ref|`` (fp16) / ``2^-8 |ref|`` (bf16), is added.  That term is relative, so the inputs keep every
    gradient that is not exactly 0 at 0.25 or above in magnitude, far from fp16's subnormal range where a half-ulp is 2^-25 whatever
    the value: R and efeat are positive with magnitudes in [0.5, 2], feat has both signs with magnitudes in [0.5, 2] (closed gates)."""
    from voltrix.autograd import SDDMM, CsrPattern, SpMMEdge

    p = _pattern_a()
    fdt, edt = DT[pair[0]], DT[pair[1]]
    shared = CsrPattern(p.indptr, p.indices, p.num_rows, p.num_cols)
    assert SDDMM(shared).pattern is shared
    op_edge = SpMMEdge(shared)
    assert op_edge.pattern is shared
    gen = torch.Generator(device=DEV).manual_seed(77)
    mag = lambda n: torch.rand(n, 24, device=DEV, generator=gen) * 1.5 + 0.5                                    # noqa: E731
    sign = torch.where(torch.rand(p.num_cols, 24, device=DEV, generator=gen) < 0.5, -1.0, 1.0)
    feat0, efeat0, weight = (mag(p.num_cols) * sign).to(fdt), mag(p.nnz).to(edt), mag(p.num_rows)
    for op in OPS:
        feat = None if op == "copy" else feat0.clone().requires_grad_(True)
        efeat = efeat0.clone().requires_grad_(True)
        out = op_edge(feat, efeat, op)
        assert out.dtype == torch.float32
        (out * weight).sum().backward()
        f64 = None if op == "copy" else feat0.double().requires_grad_(True)
        e64 = efeat0.double().requires_grad_(True)
        (_composite(p, f64, e64, op) * weight.double()).sum().backward()
        assert efeat.grad.dtype == edt and efeat.grad.shape == efeat.shape
        ref = _np(e64.grad)
        bound = U * np.abs(ref) if op == "mul" else np.zeros_like(ref)
        _within(efeat.grad, ref, bound + HALF_ULP.get(edt, 0.0) * np.abs(ref), f"autograd d_efeat {op} {pair}")
        if op == "copy":
            continue
        assert feat.grad.dtype == fdt and feat.grad.shape == feat.shape
        ref = _np(f64.grad)
        _, mass, count = oracle.grad_feat(p.ip, p.cols, _np(weight), _np(feat0), _np(efeat0), op, p.num_cols)
        _within(feat.grad, ref, (count[:, None] + 1) * U * mass + HALF_ULP.get(fdt, 0.0) * np.abs(ref), f"autograd d_feat {op} {pair}")
        if op == "add_relu":
            assert bool((feat.grad == 0).any()) and bool((feat.grad != 0).any())           # gates of both kinds


def test_autograd_computes_only_the_gradients_asked_for(cuda_device, monkeypatch):
    import sys

    import voltrix
    from voltrix.autograd import SpMMEdge

    assert callable(voltrix.spmm_edge)
    module = sys.modules["voltrix.spmm_edge"]          # the function shadows the module as an attribute of the package

    p = _pattern_b()
    op_edge = SpMMEdge(p.indptr, p.indices, p.num_rows, p.num_cols)
    feat0, efeat0, _ = _inputs(p, (8,), ("fp32", "fp32"), "normal", seed=1)
    calls = []
    for name in ("grad_efeat", "grad_feat"):
        original = getattr(module, name)
        monkeypatch.setattr(module, name, lambda *a, _n=name, _o=original: (calls.append(_n), _o(*a))[1])
    for op in ("mul", "add", "add_relu"):
        for which in ("feat", "efeat"):
            feat = feat0.clone().requires_grad_(which == "feat")
            efeat = efeat0.clone().requires_grad_(which == "efeat")
            calls.clear()
            op_edge(feat, efeat, op).sum().backward()
            assert calls == ["grad_" + which], (op, which, calls)
            assert (feat.grad is None) == (which == "efeat") and (efeat.grad is None) == (which == "feat")
    # add and copy save nothing; mul and add_relu both operands
    efeat = efeat0.clone().requires_grad_(True)
    assert len(op_edge(None, efeat, "copy").grad_fn.saved_tensors) == 0
    assert len(op_edge(feat0, efeat, "add").grad_fn.saved_tensors) == 0
    assert len(op_edge(feat0, efeat, "add_relu").grad_fn.saved_tensors) == 2


# --------------------------------------------------------------------------------------------- the same bits; degenerate patterns
def _everything(p, feat, efeat, grad, op):
    import voltrix
    from voltrix.spmm_edge import grad_efeat, grad_feat

    f = None if op == "copy" else feat
    results = [voltrix.spmm_edge(p.indptr, p.indices, f, efeat, p.num_rows, op=op), grad_efeat(p.indptr, p.indices, grad, f, efeat, op)]
    if op != "copy":
        results.append(grad_feat(p.t_indptr, p.t_indices, p.t_order, grad, feat, efeat, op, p.num_cols))
    return results


def _bits_equal(xs, ys):
    return len(xs) == len(ys) and all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(xs, ys))


def test_two_calls_give_the_same_bits(cuda_device):
    p = _pattern_a()
    for pair, tail in ((("fp32", "fp32"), (20,)), (("fp32", "fp16"), (64,))):
        feat, efeat, grad = _inputs(p, tail, pair, "normal", seed=2)
        for op in OPS:
            assert _bits_equal(_everything(p, feat, efeat, grad, op), _everything(p, feat, efeat, grad, op)), (pair, op)


def test_degenerate_calls(cuda_device):
    import voltrix
    from voltrix.spmm_edge import grad_efeat, grad_feat

    feat = torch.randn(30, 12, device=DEV)
    none = Pattern([0] * 7, [], 30)                      # rows, no entries: zeros
    zero = Pattern([], [], 30)                           # no rows
    for op in OPS:
        f = None if op == "copy" else feat
        out = voltrix.spmm_edge(none.indptr, none.indices, f, torch.empty(0, 12, device=DEV), 7, op=op)
        assert out.shape == (7, 12) and bool((out == 0).all())
        assert grad_efeat(none.indptr, none.indices, torch.ones(7, 12, device=DEV), f, torch.empty(0, 12, device=DEV), op).shape == (0, 12)
        out = voltrix.spmm_edge(zero.indptr, zero.indices, f, torch.empty(0, 12, device=DEV), 0, op=op)
        assert out.shape == (0, 12)
        if op != "copy":
            for q, rows in ((none, 7), (zero, 0)):
                d = grad_feat(q.t_indptr, q.t_indices, q.t_order, torch.ones(rows, 12, device=DEV), feat, torch.empty(0, 12, device=DEV),
                              op, 30)
                assert d.shape == (30, 12) and bool((d == 0).all())
    p = _pattern_b()                                     # F = 0
    for op in OPS:
        f = None if op == "copy" else torch.empty(p.num_cols, 0, device=DEV)
        efeat = torch.empty(p.nnz, 0, device=DEV)
        assert voltrix.spmm_edge(p.indptr, p.indices, f, efeat, p.num_rows, op=op).shape == (p.num_rows, 0)
        assert grad_efeat(p.indptr, p.indices, torch.empty(p.num_rows, 0, device=DEV), f, efeat, op).shape == (p.nnz, 0)
        if op != "copy":
            assert grad_feat(p.t_indptr, p.t_indices, p.t_order, torch.empty(p.num_rows, 0, device=DEV), f, efeat, op,
                             p.num_cols).shape == (p.num_cols, 0)


# ------------------------------------------------------------------------------------------------------ layouts, undefined memory
@pytest.mark.parametrize("pair,tail", [(("fp32", "fp32"), (20,)), (("fp16", "fp16"), (3, 8))], ids=["fp32-20", "fp16-3x8"])
def test_views_give_the_bits_of_the_contiguous_call(cuda_device, pair, tail):
    """``feat``, ``efeat`` and ``grad_out`` as offset, strided and transposed-storage views (tests/test_gpu_views.py's ``views``), one at a
    time: the bits of the call on their contiguous clones."""
    import test_gpu_views as tv

    p = _pattern_b()
    feat, efeat, grad = _inputs(p, tail, pair, "normal", seed=5)
    for op in ("mul", "add_relu"):
        want = _everything(p, feat.clone(), efeat.clone(), grad.clone(), op)
        seen = set()
        for name, t in (("feat", feat), ("efeat", efeat), ("grad", grad)):
            for label, v in tv.views(t):
                args = {"feat": feat, "efeat": efeat, "grad": grad, name: v}
                assert _bits_equal(_everything(p, args["feat"], args["efeat"], args["grad"], op), want), (op, name, label)
                seen.add(label)
        assert {"flat+1", "cols", "rows+1", "step"} <= seen and ("perm" in seen) == (len(tail) == 2)


def test_outputs_between_guard_bands(cuda_device):
    """Caller-provided outputs of both entry points at element offsets 0 and 4 of a sentinel-filled buffer: the result and untouched
    guards; off the 16-byte grid (offset 1): return code 1 from the host and a buffer that still holds nothing but the sentinel."""
    import test_gpu_views as tv
    from voltrix import capi

    p = _pattern_a()
    feat, efeat, grad = _inputs(p, (20,), ("fp32", "fp32"), "normal", seed=6)
    stream = torch.cuda.current_stream().cuda_stream
    for op in ("mul", "add_relu"):
        want = _everything(p, feat, efeat, grad, op)
        launches = (
            (want[0], lambda out: capi.launch_spmm_edge(p.indptr, p.indices, None, p.num_rows, feat, efeat, None, op, out, stream)),
            (want[1], lambda out: capi.launch_spmm_edge_grad_efeat(p.indptr, p.indices, p.num_rows, grad, feat, efeat, torch.float32, op,
                                                                   out, stream)),
            (want[2], lambda out: capi.launch_spmm_edge(p.t_indptr, p.t_indices, p.t_order, p.num_cols, grad, efeat,
                                                        feat if op == "add_relu" else None, "gate" if op == "add_relu" else "mul", out,
                                                        stream)),
        )
        for i, (expected, launch) in enumerate(launches):
            for k in (0, 4):
                buf, out = tv._guarded(tuple(expected.shape), k)
                launch(out)
                tv._check_guards(buf, out, k, (op, i))
                assert tv._same_bits(out, expected), (op, i, k)
            buf, out = tv._guarded(tuple(expected.shape), 1)
            with pytest.raises(capi.VoltrixError, match="return code 1"):
                launch(out)
            torch.cuda.synchronize()
            assert bool((buf.view(torch.int32) == tv.SENTINEL).all()), (op, i)


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_poisoned_scratch_and_output_memory(cuda_device, byte):
    """The whole operator, forward and backward through autograd, with every ``torch.empty`` filled with ``byte``: the bits of a plain run.
    Widths that need padding (12 for fp16) and that do not."""
    from voltrix.autograd import CsrPattern, SpMMEdge

    p = _pattern_a()
    op_edge = SpMMEdge(CsrPattern(p.indptr, p.indices, p.num_rows, p.num_cols))

    def run(feat0, efeat0, weight, op):
        feat = None if op == "copy" else feat0.clone().requires_grad_(True)
        efeat = efeat0.clone().requires_grad_(True)
        out = op_edge(feat, efeat, op)
        (out * weight).sum().backward()
        return [out.detach(), efeat.grad.float()] + ([] if feat is None else [feat.grad.float()])

    for pair, tail in ((("fp32", "fp32"), (20,)), (("fp16", "fp16"), (12,))):
        feat0, efeat0, weight = _inputs(p, tail, pair, "normal", seed=9)
        for op in OPS:
            want = run(feat0, efeat0, weight, op)
            with poisoned(byte) as state:
                got = run(feat0, efeat0, weight, op)
            assert state.filled > 0 and _bits_equal(got, want), (pair, op)


# -------------------------------------------------------------------------------------------------------------------------- blocks
def test_sampled_blocks_take_their_edge_features_by_entry_id(cuda_device):
    """``voltrix.sample_blocks`` on pattern A (as a square graph of 203 nodes: its columns are below 150) with fan-outs (3, 2):
    ``SpMMEdge(block.pattern)(h, efeat[block.entries], "mul")`` is the oracle on the block's CSR."""
    import voltrix
    from voltrix.autograd import SpMMEdge

    p = _pattern_a()
    gen = torch.Generator(device=DEV).manual_seed(12)
    edge_feat = torch.randn(p.nnz, 16, device=DEV, generator=gen)
    seeds = torch.arange(0, 203, 5, dtype=torch.int32, device=DEV)
    blocks = voltrix.sample_blocks(p.indptr, p.indices, seeds, (3, 2), seed=5)
    assert len(blocks) == 2 and blocks[-1].num_dst == seeds.numel()
    for block in blocks:
        h = torch.randn(block.num_src, 16, device=DEV, generator=gen)
        efeat = edge_feat[block.entries.long()]
        assert efeat.shape[0] == block.pattern.num_edges > 0
        out = SpMMEdge(block.pattern)(h, efeat, "mul")
        ip, cols = block.pattern.indptr.cpu().numpy().astype(np.int64), block.pattern.indices.cpu().numpy().astype(np.int64)
        # the block's entries are the sampled graph's: the same columns, globally
        assert np.array_equal(block.src_ids.cpu().numpy()[cols], p.cols[block.entries.cpu().numpy()])
        ref, mass, count = oracle.forward(ip, cols, _np(h), _np(efeat), "mul")
        _within(out, ref, (count[:, None] + 1) * U * mass, f"block {block.num_dst} x {block.num_src}")
