"""GPU: ``voltrix.spmm_rel`` (R-GCN's aggregation over typed edges with basis decomposition), both its gradients and
``voltrix.autograd.SpMMRel`` against the numpy float64 oracle of tests/spmm_rel_oracle.py, from the inputs as stored (fp32, fp16 and
bf16 convert to float64 exactly).  Every comparison is over every element.

Bounds, with ``u = 2^-23``, ``k`` entries in the row or column and ``m_r`` entries of type ``r``:

    forward     |out - ref| <= (k + 2) u sum |terms|
    grad_feat   |dF - ref|  <= (k B + 2) u sum |terms|
    grad_coef   |dC - ref|  <= (m_r + F + 2) u sum_e |w_e| sum_f |g x|

Each term takes at most two roundings (the coefficient ``w_e coef``, then the product) and a sum of ``n`` terms in any fixed order takes
``n - 1`` more; the bounds are twice that first-order sum.  Integer-valued inputs in [-3, 3] (``coef`` and ``weight`` too): equality.
"""
import sys

import numpy as np
import pytest
import torch

import spmm_rel_oracle as oracle
from conftest import load_csr_fixture
from poisoned_alloc import poisoned

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
DEV = "cuda"
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
HALF_ULP = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


# ------------------------------------------------------------------------------------------------------------------- the patterns
class Pattern:
    """A typed CSR on the host (numpy) and on the device (int32), with its transpose by a stable sort by column."""

    def __init__(self, lengths, cols, num_cols, etype, num_types):
        lengths, cols = np.asarray(lengths, np.int64), np.asarray(cols, np.int64)
        self.num_rows, self.num_cols, self.nnz, self.num_types = len(lengths), int(num_cols), int(lengths.sum()), int(num_types)
        assert cols.size == self.nnz == len(etype)
        self.lengths, self.ip, self.cols, self.types = lengths, np.concatenate([[0], np.cumsum(lengths)]), cols, np.asarray(etype, np.int64)
        self.rows = np.repeat(np.arange(self.num_rows), lengths)
        self.t = oracle.transpose(self.ip, cols, self.num_cols)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(DEV)     # noqa: E731
        self.indptr, self.indices, self.etype = dev(self.ip), dev(cols), dev(self.types)
        self.t_indptr, self.t_indices, self.t_order = (dev(x) for x in self.t)
        self.type_count = np.bincount(self.types, minlength=num_types)
        self._index = None

    @property
    def type_index(self):
        if self._index is None:
            import voltrix

            self._index = voltrix.spmm_rel.TypeIndex(self.etype, self.num_types)
        return self._index


_CACHE = {}
HUB = 102


def _pattern_a():
    """203 rows (a multiple of no rows-per-group count) x 150 columns: row lengths on both sides of the 4-entry batch, one hub row of
    1,031 entries, the rest 0 .. 12; columns sorted inside a row, duplicates present.  R = 7 with type 6 unused; the hub's entries are
    90 % type 2, the others uniform over 0 .. 5: type 2 has more than 2 CHUNK entries, so both levels of grad_coef's sum run with more
    than one chunk."""
    if "a" not in _CACHE:
        import voltrix

        rng = np.random.default_rng(17)
        lengths = [0, 1, 2, 3, 4, 5, 7, 8, 9, 0, 6, 1] + [int(v) for v in rng.integers(0, 13, 90)] + [1031]
        lengths += [int(v) for v in rng.integers(0, 13, 203 - len(lengths))]
        lengths = np.asarray(lengths, np.int64)
        assert len(lengths) == 203 and lengths[HUB] == 1031 and all(203 % r for r in (4, 8, 16, 32, 64, 128, 256))
        rows = np.repeat(np.arange(203), lengths)
        cols = np.sort(rows * 150 + rng.integers(0, 150, rows.size)) % 150
        assert len(np.unique(rows * 150 + cols)) < rows.size - 500                     # duplicates are present
        etype = rng.integers(0, 6, rows.size)
        hub = rows == HUB
        etype[hub] = np.where(rng.random(int(hub.sum())) < 0.9, 2, etype[hub])
        p = Pattern(lengths, cols, 150, etype, 7)
        chunk = voltrix.spmm_rel.CHUNK
        assert p.type_count[6] == 0 and p.type_count[2] > 2 * chunk, (p.type_count, chunk)
        index = p.type_index
        assert int(index.type_ptr[3] - index.type_ptr[2]) >= 3 and int((index.chunk_ptr[1:] - index.chunk_ptr[:-1]).max()) == chunk
        _CACHE["a"] = p
    return _CACHE["a"]


def _pattern_b():
    if "b" not in _CACHE:
        g = load_csr_fixture("toy40")
        ip = np.asarray(g["indptr"], np.int64)
        etype = np.random.default_rng(5).integers(0, 3, int(ip[-1]))
        _CACHE["b"] = Pattern(ip[1:] - ip[:-1], g["indices"], int(g["num_nodes"]), etype, 3)
    return _CACHE["b"]


# --------------------------------------------------------------------------------------------------------------------- the inputs
def _inputs(p, dim, bases, dtype, kind, weighted=True, seed=0):
    """``(feat [num_cols, dim], coef [R, bases] fp32, weight [nnz] fp32 or None, grad_out [num_rows, bases, dim] fp32)`` on the device.
    "normal", or "ints": integers in [-3, 3] everywhere."""
    gen = torch.Generator(device=DEV).manual_seed(5000 + seed)
    if kind == "ints":
        draw = lambda *shape: torch.randint(-3, 4, shape, device=DEV, generator=gen).float()       # noqa: E731
    else:
        draw = lambda *shape: torch.randn(shape, device=DEV, generator=gen)                        # noqa: E731
    feat = draw(p.num_cols, dim).to(DT[dtype])
    return feat, draw(p.num_types, bases), draw(p.nnz) if weighted else None, draw(p.num_rows, bases, dim)


def _np(t):
    return None if t is None else t.detach().double().cpu().numpy()


def _within(got, ref, bound, what):
    err = np.abs(_np(got).reshape(ref.shape) - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: max err / bound = {worst:.3f}")
    assert bool((err <= bound).all()), (what, worst)


def _check_all(p, feat, coef, weight, grad, exact, what):
    """The three results on one set of inputs against the oracle."""
    import voltrix
    from voltrix.spmm_rel import grad_coef, grad_feat

    bases, dim = coef.shape[1], feat.shape[1]
    out = voltrix.spmm_rel(p.indptr, p.indices, p.etype, feat, coef, p.num_rows, weight)
    assert out.dtype == torch.float32 and out.shape == (p.num_rows, bases, dim)
    ref, mass, count = oracle.forward(p.ip, p.cols, p.types, _np(feat), _np(coef), _np(weight))
    if exact:
        assert np.array_equal(_np(out), ref), what
    _within(out, ref, (count[:, None, None] + 2) * U * mass, f"forward {what}")
    assert bool((out[torch.from_numpy(p.lengths == 0).to(DEV)] == 0).all())

    gf = grad_feat(p.t_indptr, p.t_indices, p.t_order, p.etype, grad, coef, p.num_cols, weight)
    assert gf.dtype == torch.float32 and gf.shape == (p.num_cols, dim)
    ref, mass, count = oracle.grad_feat(p.ip, p.cols, p.types, _np(grad), _np(coef), p.num_cols, _np(weight))
    if exact:
        assert np.array_equal(_np(gf), ref), what
    _within(gf, ref, (count[:, None] * bases + 2) * U * mass, f"grad_feat {what}")

    gc = grad_coef(p.indptr, p.indices, p.etype, p.type_index, grad, feat, weight)
    assert gc.dtype == torch.float32 and gc.shape == (p.num_types, bases)
    ref, mass, count = oracle.grad_coef(p.ip, p.cols, p.types, _np(grad), _np(feat), p.num_types, _np(weight))
    if exact:
        assert np.array_equal(_np(gc), ref), what
    _within(gc, ref, (count[:, None] + dim + 2) * U * mass, f"grad_coef {what}")
    assert bool((gc[torch.from_numpy(p.type_count == 0).to(DEV)] == 0).all())             # a type without entries: a zero gradient


def _tile():
    import voltrix

    return voltrix.spmm_rel.BASIS_TILE


def _cases():
    """(dtype, F, B): every width at B = 3 (one tile, the 4-tile kernel) and B = BASIS_TILE + 1 (two tiles); every basis count at
    F = 12 (padded for 16-bit) and F = 64.  260 (fp32) and 520 (16-bit): the first lane of the second slab."""
    from voltrix.spmm_rel import BASIS_TILE as tile

    out = []
    for dtype in ("fp32", "fp16", "bf16"):
        widths = (1, 4, 12, 20, 64, 260 if dtype == "fp32" else 520)
        counts = (1, 3, tile, tile + 1, 2 * tile + 3)
        seen = [(f, b) for f in widths for b in (3, tile + 1)] + [(f, b) for f in (12, 64) for b in counts]
        out += [(dtype, f, b) for f, b in dict.fromkeys(seen)]
    return out


CASES = _cases()


@pytest.mark.parametrize("dtype,dim,bases", CASES, ids=[f"{d}-F{f}-B{b}" for d, f, b in CASES])
def test_forward_and_both_gradients_on_pattern_a(cuda_device, dtype, dim, bases):
    p = _pattern_a()
    for kind, weighted in (("normal", True), ("normal", False), ("ints", True)):
        feat, coef, weight, grad = _inputs(p, dim, bases, dtype, kind, weighted, seed=dim + bases)
        _check_all(p, feat, coef, weight, grad, kind == "ints", f"{dtype} F={dim} B={bases} {kind} weight={weighted}")


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
def test_forward_and_both_gradients_on_the_fixture_pattern(cuda_device, dtype):
    p = _pattern_b()
    for bases in (2, _tile() + 1):
        for kind, weighted in (("normal", True), ("ints", False)):
            feat, coef, weight, grad = _inputs(p, 24, bases, dtype, kind, weighted, seed=3)
            _check_all(p, feat, coef, weight, grad, kind == "ints", f"toy40 {dtype} B={bases} {kind} weight={weighted}")


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
def test_without_coef_it_is_the_sum_per_relation(cuda_device, dtype):
    """``coef=None`` (the identity; R = etype.max() + 1) and the number of types as an int: [num_rows, R, F], the oracle with ``I_R``."""
    import voltrix
    from voltrix.spmm_rel import grad_feat

    for p in (_pattern_a(), _pattern_b()):
        used = int(p.types.max()) + 1                               # pattern A: 6 of its 7 types occur
        feat, _, weight, _ = _inputs(p, 20, 1, dtype, "normal", True, seed=7)
        for coef, r in ((None, used), (p.num_types, p.num_types)):
            out = voltrix.spmm_rel(p.indptr, p.indices, p.etype, feat, coef, p.num_rows, weight)
            assert out.shape == (p.num_rows, r, 20)
            ref, mass, count = oracle.forward(p.ip, p.cols, p.types, _np(feat), np.eye(r), _np(weight))
            _within(out, ref, (count[:, None, None] + 2) * U * mass, f"identity {dtype} R={r}")
            # one entry, one term: a (row, type) pair without entries is exactly 0
            assert bool((out[torch.from_numpy(mass == 0).to(DEV)] == 0).all())
            grad = torch.randn(p.num_rows, r, 20, device=DEV, generator=torch.Generator(device=DEV).manual_seed(r))
            gf = grad_feat(p.t_indptr, p.t_indices, p.t_order, p.etype, grad, coef, p.num_cols, weight)
            ref, mass, count = oracle.grad_feat(p.ip, p.cols, p.types, _np(grad), np.eye(r), p.num_cols, _np(weight))
            _within(gf, ref, (count[:, None] * r + 2) * U * mass, f"identity grad_feat {dtype} R={r}")


def test_nan_and_inf_propagate_as_the_arithmetic_does(cuda_device):
    import voltrix

    p = _pattern_a()
    feat, coef, weight, _ = _inputs(p, 20, 3, "fp32", "normal", True, seed=8)
    dice = torch.rand(feat.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    feat[dice < 0.01] = float("nan")
    feat[(dice >= 0.01) & (dice < 0.02)] = float("inf")
    feat[(dice >= 0.02) & (dice < 0.03)] = float("-inf")
    rows, cols, types = (torch.from_numpy(x).to(DEV) for x in (p.rows, p.cols, p.types))
    terms = (weight.double()[:, None] * coef.double()[types])[:, :, None] * feat.double()[cols][:, None, :]
    zeros = lambda: torch.zeros(p.num_rows, 3, 20, dtype=torch.float64, device=DEV)     # noqa: E731
    ref = zeros().index_add_(0, rows, terms)
    bound = (torch.from_numpy(p.lengths).to(DEV)[:, None, None] + 2) * U * zeros().index_add_(0, rows, terms.abs())
    out = voltrix.spmm_rel(p.indptr, p.indices, p.etype, feat, coef, p.num_rows, weight).double()
    ok = ((out - ref).abs() <= bound) | (out == ref) | (out.isnan() & ref.isnan())
    assert bool(ok.all()), int((~ok).sum())
    assert torch.equal(out.isnan(), ref.isnan()) and torch.equal(out.isinf(), ref.isinf())
    assert bool(ref.isnan().any()) and bool(ref.isinf().any()) and bool(ref.isfinite().any())


# ------------------------------------------------------------------------------------------------------------------------ autograd
def _composite(p, feat64, coef64, weight64):
    rows, cols, types = (torch.from_numpy(x).to(DEV) for x in (p.rows, p.cols, p.types))
    c = coef64[types] if weight64 is None else weight64[:, None] * coef64[types]
    terms = c[:, :, None] * feat64[cols][:, None, :]
    return torch.zeros((p.num_rows, coef64.shape[1], feat64.shape[1]), dtype=torch.float64, device=DEV).index_add_(0, rows, terms)


@pytest.mark.parametrize("pair", [("fp32", "fp32"), ("fp16", "fp32"), ("bf16", "fp32"), ("fp16", "bf16")], ids="-".join)
def test_autograd_operator_against_torch_float64_autograd(cuda_device, pair):
    """Gradients of ``(out * R).sum()`` for a fixed random R, against float64 autograd of the composite ``index_add_(w coef[etype] x
    feat[cols])``; ``pair`` = the dtypes of (feat, coef).  fp32 operands: the bounds of the module's docstring.  A 16-bit operand's
    gradient is cast to its type at the end: the type's half-ulp, ``2^-11 |ref|`` (fp16) / ``2^-8 |ref|`` (bf16), is added.  That term
    is relative, so every operand is positive with magnitudes in [0.5, 2]: a gradient that is not exactly 0 stays far from fp16's
    subnormal range, where a half-ulp is 2^-25 whatever the value."""
    from voltrix.autograd import SDDMM, CsrPattern, SpMMRel

    p = _pattern_a()
    fdt, cdt = DT[pair[0]], DT[pair[1]]
    shared = CsrPattern(p.indptr, p.indices, p.num_rows, p.num_cols)
    assert SDDMM(shared).pattern is shared
    op = SpMMRel(shared, etype=p.etype, num_types=p.num_types)
    assert op.pattern is shared and op.type_index.num_chunks == p.type_index.num_chunks
    gen = torch.Generator(device=DEV).manual_seed(78)
    mag = lambda *shape: torch.rand(shape, device=DEV, generator=gen) * 1.5 + 0.5                                 # noqa: E731
    bases = _tile() + 1
    feat0, coef0, weight, r = mag(p.num_cols, 24).to(fdt), mag(p.num_types, bases).to(cdt), mag(p.nnz), mag(p.num_rows, bases, 24)
    for w in (weight, None):
        feat, coef = feat0.clone().requires_grad_(True), coef0.clone().requires_grad_(True)
        out = op(feat, coef, w)
        assert out.dtype == torch.float32 and out.shape == (p.num_rows, bases, 24)
        (out * r).sum().backward()
        f64, c64 = feat0.double().requires_grad_(True), coef0.double().requires_grad_(True)
        (_composite(p, f64, c64, None if w is None else w.double()) * r.double()).sum().backward()
        assert feat.grad.dtype == fdt and feat.grad.shape == feat.shape and coef.grad.dtype == cdt and coef.grad.shape == coef.shape
        ref = _np(f64.grad)
        _, mass, count = oracle.grad_feat(p.ip, p.cols, p.types, _np(r), _np(coef0), p.num_cols, _np(w))
        _within(feat.grad, ref, (count[:, None] * bases + 2) * U * mass + HALF_ULP.get(fdt, 0.0) * np.abs(ref), f"autograd d_feat {pair}")
        ref = _np(c64.grad)
        _, mass, count = oracle.grad_coef(p.ip, p.cols, p.types, _np(r), _np(feat0), p.num_types, _np(w))
        _within(coef.grad, ref, (count[:, None] + 24 + 2) * U * mass + HALF_ULP.get(cdt, 0.0) * np.abs(ref), f"autograd d_coef {pair}")
        assert bool((coef.grad[6] == 0).all()) and bool((coef.grad[:6] != 0).all())
    # coef=None: the identity, differentiable in feat alone
    feat = feat0.clone().requires_grad_(True)
    out = op(feat, None, weight)
    assert out.shape == (p.num_rows, p.num_types, 24)
    r7 = mag(p.num_rows, p.num_types, 24)
    (out * r7).sum().backward()
    f64 = feat0.double().requires_grad_(True)
    (_composite(p, f64, torch.eye(p.num_types, dtype=torch.float64, device=DEV), weight.double()) * r7.double()).sum().backward()
    _, mass, count = oracle.grad_feat(p.ip, p.cols, p.types, _np(r7), np.eye(p.num_types), p.num_cols, _np(weight))
    ref = _np(f64.grad)
    _within(feat.grad, ref, (count[:, None] * p.num_types + 2) * U * mass + HALF_ULP.get(fdt, 0.0) * np.abs(ref), f"autograd identity {pair}")
    with pytest.raises(ValueError, match="no gradient"):
        op(feat0, coef0, weight.clone().requires_grad_(True))


def test_autograd_computes_only_the_gradients_asked_for(cuda_device, monkeypatch):
    import voltrix
    from voltrix.autograd import SpMMRel

    assert callable(voltrix.spmm_rel)
    module = sys.modules["voltrix.spmm_rel"]           # the function shadows the module as an attribute of the package

    p = _pattern_b()
    op = SpMMRel(p.indptr, p.indices, p.num_rows, p.num_cols, etype=p.etype, num_types=p.num_types)
    built = []
    monkeypatch.setattr(module, "TypeIndex", lambda *a, **k: built.append(a) or p.type_index)
    feat0, coef0, weight, _ = _inputs(p, 8, 3, "fp32", "normal", True, seed=1)
    calls = []
    for name in ("grad_feat", "grad_coef"):
        original = getattr(module, name)
        monkeypatch.setattr(module, name, lambda *a, _n=name, _o=original: (calls.append(_n), _o(*a))[1])
    for which in ("feat", "coef"):
        feat = feat0.clone().requires_grad_(which == "feat")
        coef = coef0.clone().requires_grad_(which == "coef")
        calls.clear()
        op(feat, coef, weight).sum().backward()
        assert calls == ["grad_" + which], (which, calls)
        assert (feat.grad is None) == (which == "coef") and (coef.grad is None) == (which == "feat")
    feat, coef = feat0.clone().requires_grad_(True), coef0.clone().requires_grad_(True)
    calls.clear()
    out = op(feat, coef, weight)
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 2 and saved[0].data_ptr() == feat.data_ptr() and saved[1].data_ptr() == coef.data_ptr()    # not weight
    out.sum().backward()
    assert sorted(calls) == ["grad_coef", "grad_feat"] and not built                     # the TypeIndex was built once, by the constructor


# --------------------------------------------------------------------------------------------- the same bits; degenerate patterns
def _everything(p, feat, coef, weight, grad):
    import voltrix
    from voltrix.spmm_rel import grad_coef, grad_feat

    return [voltrix.spmm_rel(p.indptr, p.indices, p.etype, feat, coef, p.num_rows, weight),
            grad_feat(p.t_indptr, p.t_indices, p.t_order, p.etype, grad, coef, p.num_cols, weight),
            grad_coef(p.indptr, p.indices, p.etype, p.type_index, grad, feat, weight)]


def _bits_equal(xs, ys):
    return len(xs) == len(ys) and all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(xs, ys))


def test_two_calls_give_the_same_bits(cuda_device):
    p = _pattern_a()
    for dtype, dim, bases in (("fp32", 20, 3), ("fp16", 64, _tile() + 1), ("bf16", 520, 2 * _tile() + 3)):
        args = _inputs(p, dim, bases, dtype, "normal", True, seed=2)
        assert _bits_equal(_everything(p, *args), _everything(p, *args)), (dtype, dim, bases)


def test_degenerate_calls(cuda_device):
    import voltrix
    from voltrix.spmm_rel import TypeIndex, grad_coef, grad_feat

    feat, coef = torch.randn(30, 12, device=DEV), torch.randn(3, 5, device=DEV)
    none = Pattern([0] * 7, [], 30, [], 3)               # rows, no entries: zeros
    zero = Pattern([], [], 30, [], 3)                    # no rows
    for q, rows in ((none, 7), (zero, 0)):
        out = voltrix.spmm_rel(q.indptr, q.indices, q.etype, feat, coef, rows)
        assert out.shape == (rows, 5, 12) and bool((out == 0).all())
        d = grad_feat(q.t_indptr, q.t_indices, q.t_order, q.etype, torch.ones(rows, 5, 12, device=DEV), coef, 30)
        assert d.shape == (30, 12) and bool((d == 0).all())
        d = grad_coef(q.indptr, q.indices, q.etype, TypeIndex(q.etype, 3), torch.ones(rows, 5, 12, device=DEV), feat)
        assert d.shape == (3, 5) and bool((d == 0).all())
    p = _pattern_b()
    weight = torch.ones(p.nnz, device=DEV)
    for dim, bases in ((0, 5), (12, 0), (0, 0)):         # F = 0, B = 0
        feat, coef = torch.randn(p.num_cols, dim, device=DEV), torch.randn(3, bases, device=DEV)
        grad = torch.randn(p.num_rows, bases, dim, device=DEV)
        out, d_feat, d_coef = _everything(p, feat, coef, weight, grad)
        assert out.shape == (p.num_rows, bases, dim) and d_feat.shape == (p.num_cols, dim) and d_coef.shape == (3, bases)
        assert bool((d_feat == 0).all()) and bool((d_coef == 0).all())


# ------------------------------------------------------------------------------------------------------ layouts, undefined memory
@pytest.mark.parametrize("dtype,dim,bases", [("fp32", 20, 3), ("fp16", 12, 9)], ids=["fp32-20-3", "fp16-12-9"])
def test_views_give_the_bits_of_the_contiguous_call(cuda_device, dtype, dim, bases):
    """``feat``, ``coef``, ``weight`` and ``grad_out`` as offset, strided and transposed-storage views (tests/test_gpu_views.py's
    ``views``), one at a time: the bits of the call on their contiguous clones."""
    import test_gpu_views as tv

    p = _pattern_b()
    feat, coef, weight, grad = _inputs(p, dim, bases, dtype, "normal", True, seed=5)
    want = _everything(p, feat.clone(), coef.clone(), weight.clone(), grad.clone())
    seen = {}
    for name, t in (("feat", feat), ("coef", coef), ("weight", weight), ("grad", grad)):
        for label, v in tv.views(t):
            args = {"feat": feat, "coef": coef, "weight": weight, "grad": grad, name: v}
            assert _bits_equal(_everything(p, args["feat"], args["coef"], args["weight"], args["grad"]), want), (name, label)
            seen.setdefault(name, set()).add(label)
    assert {"flat+1", "cols", "rows+1", "step"} <= seen["feat"] and {"flat+1", "cols", "rows+1", "step"} <= seen["coef"]
    assert {"flat+1", "step"} <= seen["weight"] and {"flat+1", "cols", "rows+1", "step", "perm"} <= seen["grad"]


def test_outputs_between_guard_bands(cuda_device):
    """Caller-provided outputs of the three entry points at element offsets 0 and 4 of a sentinel-filled buffer: the result and
    untouched guards; off the 16-byte grid (offset 1): return code 1 from the host and a buffer that still holds nothing but the
    sentinel."""
    import test_gpu_views as tv
    from voltrix import capi

    p = _pattern_a()
    stream = torch.cuda.current_stream().cuda_stream
    for bases in (3, _tile() + 1):
        feat, coef, weight, grad = _inputs(p, 20, bases, "fp32", "normal", True, seed=6)
        padded = (bases + 3) // 4 * 4
        table = torch.nn.functional.pad(coef, (0, padded - bases)).contiguous()
        want = _everything(p, feat, coef, weight, grad)
        dots = torch.empty(p.nnz, padded, device=DEV)
        capi.launch_spmm_rel_dots(p.indptr, p.indices, weight, p.num_rows, grad, feat, dots, stream)
        assert bool((dots[:, bases:] == 0).all())                                          # the padding is written, as 0
        launches = (
            (want[0], lambda out: capi.launch_spmm_rel(p.indptr, p.indices, p.etype, weight, p.num_rows, feat, table, bases, out, stream)),
            (want[1], lambda out: capi.launch_spmm_rel_contract(p.t_indptr, p.t_indices, p.t_order, p.etype, weight, p.num_cols, grad,
                                                                table, out, stream)),
            (dots, lambda out: capi.launch_spmm_rel_dots(p.indptr, p.indices, weight, p.num_rows, grad, feat, out, stream)),
        )
        for i, (expected, launch) in enumerate(launches):
            for k in (0, 4):
                buf, out = tv._guarded(tuple(expected.shape), k)
                launch(out)
                tv._check_guards(buf, out, k, (bases, i))
                assert tv._same_bits(out, expected), (bases, i, k)
            buf, out = tv._guarded(tuple(expected.shape), 1)
            with pytest.raises(capi.VoltrixError, match="return code 1"):
                launch(out)
            torch.cuda.synchronize()
            assert bool((buf.view(torch.int32) == tv.SENTINEL).all()), (bases, i)


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_poisoned_scratch_and_output_memory(cuda_device, byte):
    """The whole operator, forward and backward through autograd, with every ``torch.empty`` filled with ``byte``: the bits of a plain
    run.  Widths that need padding (12 for fp16; B = 3 and 9 pad the coefficient table and the dots) and that do not."""
    from voltrix.autograd import CsrPattern, SpMMRel

    p = _pattern_a()
    op = SpMMRel(CsrPattern(p.indptr, p.indices, p.num_rows, p.num_cols), etype=p.etype, num_types=p.num_types)

    def run(feat0, coef0, weight, r):
        feat, coef = feat0.clone().requires_grad_(True), coef0.clone().requires_grad_(True)
        out = op(feat, coef, weight)
        (out * r).sum().backward()
        return [out.detach(), feat.grad.float(), coef.grad.float()]

    for dtype, dim, bases in (("fp32", 20, 3), ("fp16", 12, _tile() + 1), ("bf16", 64, _tile())):
        feat0, coef0, weight, r = _inputs(p, dim, bases, dtype, "normal", True, seed=9)
        want = run(feat0, coef0, weight, r)
        with poisoned(byte) as state:
            got = run(feat0, coef0, weight, r)
        assert state.filled > 0 and _bits_equal(got, want), (dtype, dim, bases)


# -------------------------------------------------------------------------------------------------------------------------- blocks
def test_sampled_blocks_take_their_edge_types_by_entry_id(cuda_device):
    """``voltrix.sample_blocks`` on pattern A (as a square graph of 203 nodes: its columns are below 150) with fan-outs (3, 2):
    ``SpMMRel(block.pattern, etype=etype[block.entries], ...)(h, coef, weight)`` is the oracle on the block's CSR."""
    import voltrix
    from voltrix.autograd import SpMMRel

    p = _pattern_a()
    gen = torch.Generator(device=DEV).manual_seed(12)
    coef = torch.randn(p.num_types, 5, device=DEV, generator=gen)
    seeds = torch.arange(0, 203, 5, dtype=torch.int32, device=DEV)
    blocks = voltrix.sample_blocks(p.indptr, p.indices, seeds, (3, 2), seed=5)
    assert len(blocks) == 2 and blocks[-1].num_dst == seeds.numel()
    for block in blocks:
        h = torch.randn(block.num_src, 16, device=DEV, generator=gen)
        etype = p.etype[block.entries.long()]
        assert etype.numel() == block.pattern.num_edges > 0
        ip, cols = block.pattern.indptr.cpu().numpy().astype(np.int64), block.pattern.indices.cpu().numpy().astype(np.int64)
        # the block's entries are the sampled graph's: the same columns and types, globally
        assert np.array_equal(block.src_ids.cpu().numpy()[cols], p.cols[block.entries.cpu().numpy()])
        assert np.array_equal(etype.cpu().numpy(), p.types[block.entries.cpu().numpy()])
        weight = voltrix.spmm_rel.type_norm(block.pattern.indptr, etype, p.num_types)
        same = np.rint(1.0 / oracle.type_norm(ip, etype.cpu().numpy())).astype(np.float32)      # entries of the row with the type
        assert np.array_equal(weight.cpu().numpy(), np.float32(1) / same) and bool((same >= 1).all())
        out = SpMMRel(block.pattern, etype=etype, num_types=p.num_types)(h, coef, weight)
        ref, mass, count = oracle.forward(ip, cols, etype.cpu().numpy(), _np(h), _np(coef), _np(weight))
        _within(out, ref, (count[:, None, None] + 2) * U * mass, f"block {block.num_dst} x {block.num_src}")
