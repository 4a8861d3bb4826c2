"""GPU: ``voltrix.spmm_multi`` (sum / mean / max / min / var / std of every row's entries from one gather), its joint backward on the
transposed CSR and ``voltrix.autograd.SpMMMulti`` against tests/spmm_multi_oracle.py: float64 torch on the device, from the inputs as
stored.

``sum`` is compared bit for bit with the CSR row-gather sum (``capi.launch_spmm_csr_rows``, fp32 output), ``mean`` / ``max`` / ``min``
and the args with ``voltrix.spmm_reduce`` (NaN positions equal, the same bits elsewhere).  ``var`` and ``std`` stay inside the oracle's
bounds (VAR), (STD) and are NaN exactly where a row holds a NaN or an infinity.  The backward equals the float64 reference on integer
inputs with ``aggrs`` from sum / max / min and stays inside the derived bound (BWD) otherwise.  Every test prints the worst
``err / bound`` it saw (``pytest -s``); profiles/spmm_multi/README.md records them.
"""
import os
import sys

import numpy as np
import pytest
import torch

import spmm_multi_oracle as oracle
from conftest import REPO, load_csr_fixture
from poisoned_alloc import poisoned

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
ALL = oracle.AGGREGATES
PNA = ("mean", "max", "min", "std")
EPS = 1e-5


# ------------------------------------------------------------------------------------------------------------------- the patterns
class Pattern:
    """A device int32 CSR and its transpose by a stable sort by column, built with numpy and torch alone."""

    def __init__(self, lengths, cols, num_cols):
        lengths, cols = np.asarray(lengths, np.int64), np.asarray(cols, np.int64)
        self.num_rows, self.num_cols, self.nnz = len(lengths), int(num_cols), int(lengths.sum())
        assert cols.size == self.nnz
        ip = np.concatenate([[0], np.cumsum(lengths)])
        rows = np.repeat(np.arange(self.num_rows), lengths)
        order = np.argsort(cols, kind="stable")
        t_ip = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=num_cols))])
        dev = lambda x, t: torch.from_numpy(np.ascontiguousarray(x)).to(t).to(DEV)     # noqa: E731
        self.lengths = lengths
        self.indptr, self.indices = dev(ip, torch.int32), dev(cols, torch.int32)
        self.cols = dev(cols, torch.int64)
        self.t_indptr, self.t_indices, self.t_order = dev(t_ip, torch.int32), dev(rows[order], torch.int32), dev(order, torch.int32)
        self.empty = dev(lengths == 0, torch.bool)
        self.deg = dev(np.maximum(lengths, 1), torch.float32)


_CACHE = {}


def _main_pattern():
    """1,003 rows over 300 columns (rectangular): row lengths 0 .. 9 on both sides of the 4-entry batch, a hub of 5,003 entries, short
    random rows; columns sorted inside a row, duplicates many."""
    if "main" not in _CACHE:
        rng = np.random.default_rng(11)
        lengths = [0, 1, 2, 3, 4, 5, 7, 8, 9, 0, 6, 1] + [int(v) for v in rng.integers(0, 13, 500)] + [5003]
        lengths += [int(v) for v in rng.integers(0, 13, 1003 - len(lengths))]
        lengths = np.asarray(lengths, np.int64)
        assert len(lengths) == 1003 and lengths.max() == 5003
        rows = np.repeat(np.arange(len(lengths)), lengths)
        cols = np.sort(rows * 300 + rng.integers(0, 300, rows.size)) % 300
        assert len(np.unique(rows * 300 + cols)) < rows.size - 1000                     # duplicates are many
        _CACHE["main"] = Pattern(lengths, cols, 300)
    return _CACHE["main"]


def _fixture_pattern(name):
    if name not in _CACHE:
        g = load_csr_fixture(name)
        ip = np.asarray(g["indptr"], np.int64)
        _CACHE[name] = Pattern(ip[1:] - ip[:-1], g["indices"], int(g["num_nodes"]))
    return _CACHE[name]


# --------------------------------------------------------------------------------------------------------------------- the inputs
def _features(p, dim, dtype, kind, seed=0):
    """[num_cols, dim] of ``dtype``: "normal"; "ints" in [-3, -1] (ties; a zero-initialised accumulator shows); "special": normal with
    NaN, +inf and -inf sprinkled in, the columns of the first 3-entry row all -inf and the column of the first 1-entry row NaN;
    "offset": 4096 + N(0, 1) in fp32, 64 + N(0, 1) / 8 for the 16-bit types (a mean far from 0: E[x^2] - E[x]^2 cancels)."""
    gen = torch.Generator(device=DEV).manual_seed(1000 + seed)
    if kind == "ints":
        return torch.randint(-3, 0, (p.num_cols, dim), device=DEV, generator=gen).to(dtype)
    feat = torch.randn(p.num_cols, dim, device=DEV, generator=gen)
    if kind == "offset":
        return (4096.0 + feat if dtype == torch.float32 else 64.0 + feat / 8).to(dtype)
    if kind == "special":
        dice = torch.rand(p.num_cols, dim, device=DEV, generator=gen)
        feat[dice < 0.01] = float("nan")
        feat[(dice >= 0.01) & (dice < 0.03)] = float("inf")
        feat[(dice >= 0.03) & (dice < 0.06)] = float("-inf")
        ip = p.indptr.tolist()
        lengths = np.asarray(p.lengths)
        if (lengths == 3).any() and (lengths == 1).any():
            three, one = int(np.flatnonzero(lengths == 3)[0]), int(np.flatnonzero(lengths == 1)[0])
            feat[p.cols[ip[three]:ip[three + 1]]] = float("-inf")
            feat[p.cols[ip[one]]] = float("nan")
    return feat.to(dtype)


KINDS = ("normal", "ints", "special", "offset")


# ------------------------------------------------------------------------------------------------------------------- comparisons
def _same_bits(got, want):
    """The same shape, NaN at the same places, the same bits everywhere else."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = got.isnan() if got.is_floating_point() else torch.zeros_like(got, dtype=torch.bool)
    if got.is_floating_point() and not torch.equal(nan, want.isnan()):
        return False
    as_int = (lambda t: t.view(torch.int32)) if got.dtype == torch.float32 else (lambda t: t)
    return torch.equal(as_int(got.contiguous())[~nan], as_int(want.contiguous())[~nan])


def _within(got, ref, bound, nan_at, what):
    """|got - ref| <= bound where ``nan_at`` is False, NaN exactly where it is True; returns the worst err / bound."""
    assert torch.equal(got.isnan(), nan_at), f"{what}: NaN at other places than the rows that hold a non-finite entry"
    err = (got.double() - ref).abs()[~nan_at]
    b = bound[~nan_at]
    worst = float((err / b.clamp_min(1e-300)).max()) if err.numel() else 0.0
    assert bool((err <= b).all()), f"{what}: worst err / bound = {worst:.3f}"
    return worst


def _row_gather_sum(p, feat):
    """The existing sum: the CSR row-gather kernel with fp32 output on the padded operand."""
    from voltrix import capi
    from voltrix.jit_kernels.spmm import _raw_stream
    from voltrix.utils import padded_last_dim, piece_width

    dim = feat.shape[1]
    padded = padded_last_dim(feat, piece_width(dim, feat.dtype))
    out = torch.empty(p.num_rows, padded.shape[1], dtype=torch.float32, device=DEV)
    capi.launch_spmm_csr_rows(p.indptr, p.indices, p.num_rows, padded, out, _raw_stream(feat.device), 1)
    return out[:, :dim].contiguous()


def _forward_checked(p, feat, what=""):
    """All six at once against the existing operators and the oracle; returns (out, state, worst var, worst std)."""
    import voltrix

    out, state = voltrix.spmm_multi(p.indptr, p.indices, feat, p.num_rows, aggrs=ALL, eps=EPS, return_state=True)
    dim = feat.shape[1]
    assert out.dtype == torch.float32 and out.shape == (p.num_rows, 6, dim) and out.is_contiguous()
    got = {name: out[:, i] for i, name in enumerate(ALL)}
    assert state.argmax.dtype == state.argmin.dtype == torch.int32 and state.argmax.shape == state.argmin.shape == (p.num_rows, dim)
    if p.nnz:
        assert _same_bits(got["sum"].contiguous(), _row_gather_sum(p, feat)), f"{what}: sum"
    assert _same_bits(got["mean"].contiguous(), voltrix.spmm_reduce(p.indptr, p.indices, feat, p.num_rows, "mean")), f"{what}: mean"
    for name, arg in (("max", state.argmax), ("min", state.argmin)):
        want, want_arg = voltrix.spmm_reduce(p.indptr, p.indices, feat, p.num_rows, name, return_arg=True)
        assert _same_bits(got[name].contiguous(), want), f"{what}: {name}"
        assert torch.equal(arg, want_arg), f"{what}: arg{name}"
    assert _same_bits(state.mean.contiguous(), got["mean"].contiguous()) and _same_bits(state.std.contiguous(), got["std"].contiguous())
    ref = oracle.forward(p.indptr, p.indices, feat, p.num_rows, EPS)
    assert torch.equal(state.argmax.long(), ref["argmax"]) and torch.equal(state.argmin.long(), ref["argmin"]), f"{what}: args"
    worst_var = _within(got["var"], ref["var"], ref["var_bound"], ref["nonfinite"], f"{what}: var")
    worst_std = _within(got["std"], ref["std"], ref["std_bound"], ref["nonfinite"], f"{what}: std")
    assert bool((out[p.empty] == 0).all()) and bool((state.argmax[p.empty] == -1).all()) and bool((state.argmin[p.empty] == -1).all())
    single = torch.from_numpy(np.asarray(p.lengths) == 1).to(DEV) & ~ref["nonfinite"].any(1)
    assert bool((got["var"][single] == 0).all()) and bool((got["std"][single] == np.float32(np.sqrt(np.float32(EPS)))).all())
    return out, state, worst_var, worst_std


# ------------------------------------------------------------------------------------------------------------------------- forward
WIDTHS = [("fp32", f) for f in (4, 12, 20, 256, 260)] + [(d, f) for d in ("fp16", "bf16") for f in (8, 24, 520)]


@pytest.mark.parametrize("dtype,dim", WIDTHS)
def test_all_six_aggregates_on_the_main_pattern(cuda_device, dtype, dim):
    p = _main_pattern()
    assert int(p.empty.sum()) > 0
    worst = {}
    for kind in KINDS:
        feat = _features(p, dim, DTYPES[dtype], kind, seed=dim)
        out, state, wv, ws = _forward_checked(p, feat, f"{dtype} {dim} {kind}")
        worst[kind] = (round(wv, 4), round(ws, 4))
        if kind == "special":
            ip = p.indptr.tolist()
            three, one = int(np.flatnonzero(p.lengths == 3)[0]), int(np.flatnonzero(p.lengths == 1)[0])
            assert bool((out[three, 2] == float("-inf")).all()) and bool((state.argmax[three] == ip[three]).all())
            assert bool(out[three, 4:].isnan().all()) and bool(out[one].isnan().all()) and bool((state.argmin[one] == ip[one]).all())
            assert bool(out[:, 4].isnan().any()) and not bool(out[:, 4].isnan().all())
    print(f"forward {dtype} F={dim}: worst err / bound (var, std) by kind: {worst}")


@pytest.mark.parametrize("name", ["toy40", "skewed_1005", "cora_like"])
def test_the_fixture_patterns(cuda_device, name):
    p = _fixture_pattern(name)
    for dtype, dim in (("fp32", 20), ("fp16", 24), ("bf16", 8)):
        for kind in KINDS:
            _forward_checked(p, _features(p, dim, DTYPES[dtype], kind, seed=7), f"{name} {dtype} {kind}")


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("dim", [1, 3, 7, 50])
def test_widths_that_need_padding(cuda_device, dtype, dim):
    p = _main_pattern()
    for kind in KINDS:
        _forward_checked(p, _features(p, dim, DTYPES[dtype], kind, seed=dim), f"{dtype} {dim} {kind}")


SUBSETS = [(a,) for a in ALL] + [("max", "min"), ("min", "max"), ("var", "std"), ("sum", "mean", "var", "std"), PNA,
                                 tuple(reversed(ALL)), ("std", "sum", "max")]


@pytest.mark.parametrize("dtype,dim", [("fp32", 20), ("fp16", 24), ("bf16", 520)])
def test_every_subset_has_the_bits_of_the_call_with_all_six(cuda_device, dtype, dim):
    import voltrix

    p = _main_pattern()
    for kind in ("special", "offset"):
        feat = _features(p, dim, DTYPES[dtype], kind, seed=3)
        whole, whole_state = voltrix.spmm_multi(p.indptr, p.indices, feat, p.num_rows, aggrs=ALL, eps=EPS, return_state=True)
        for aggrs in SUBSETS:
            out = voltrix.spmm_multi(p.indptr, p.indices, feat, p.num_rows, aggrs=aggrs, eps=EPS)
            with_state, state = voltrix.spmm_multi(p.indptr, p.indices, feat, p.num_rows, aggrs=list(aggrs), eps=EPS, return_state=True)
            assert out.shape == with_state.shape == (p.num_rows, len(aggrs), dim) and out.is_contiguous() and with_state.is_contiguous()
            for i, name in enumerate(aggrs):
                want = whole[:, ALL.index(name)].contiguous()
                assert _same_bits(out[:, i].contiguous(), want), (aggrs, name, kind)
                assert _same_bits(with_state[:, i].contiguous(), want), (aggrs, name, kind, "with state")
            assert (state.argmax is not None) == ("max" in aggrs) and (state.argmin is not None) == ("min" in aggrs)
            assert (state.mean is not None) == ("var" in aggrs or "std" in aggrs) and (state.std is not None) == ("std" in aggrs)
            for got, want in ((state.argmax, whole_state.argmax), (state.argmin, whole_state.argmin)):
                assert got is None or torch.equal(got, want), (aggrs, kind)
            for got, want in ((state.mean, whole_state.mean), (state.std, whole_state.std)):
                assert got is None or _same_bits(got.contiguous(), want.contiguous()), (aggrs, kind)
    # eps reaches the kernel: another eps moves std alone
    other = voltrix.spmm_multi(p.indptr, p.indices, feat, p.num_rows, aggrs=("var", "std"), eps=0.25)
    assert _same_bits(other[:, 0].contiguous(), whole[:, 4].contiguous()) and not torch.equal(other[:, 1], whole[:, 5])
    occupied = ~p.empty
    assert bool((other[occupied][:, 1] >= 0.5).all()) and bool((other[p.empty] == 0).all())


# ------------------------------------------------------------------------------------------------------------------------ backward
def _grad_inputs(p, aggrs, grads, state):
    """u and w as ``autograd.SpMMMulti`` forms them, with fp32 torch ops: (u, w), each None where no aggregate needs it."""
    deg = p.deg.view((-1,) + (1,) * (grads.dim() - 2))
    g = {name: grads[:, i].float() for i, name in enumerate(aggrs)}
    u = w = None
    if "mean" in g:
        u = g["mean"] / deg
    if "sum" in g:
        u = g["sum"] if u is None else u + g["sum"]
    if "var" in g:
        w = 2.0 * g["var"] / deg
    if "std" in g:
        by_std = g["std"] / (deg * state.std)
        w = by_std if w is None else w + by_std
    return u, w


def _backward(p, feat, aggrs, grads, state):
    import voltrix

    u, w = _grad_inputs(p, aggrs, grads, state)
    pick = lambda name: grads[:, aggrs.index(name)] if name in aggrs else None     # noqa: E731
    return voltrix.spmm_multi.backward(p.t_indptr, p.t_indices, p.t_order, p.num_cols, feat=feat if w is not None else None, u=u, w=w,
                                       mean=state.mean if w is not None else None, g_max=pick("max"), argmax=state.argmax,
                                       g_min=pick("min"), argmin=state.argmin)


@pytest.mark.parametrize("dtype,dim", [("fp32", 4), ("fp32", 20), ("fp32", 260), ("fp16", 24), ("bf16", 8), ("fp32", 7), ("fp16", 50)])
def test_backward_on_integers_equals_the_reference(cuda_device, dtype, dim):
    import voltrix

    p = _main_pattern()
    feat = _features(p, dim, DTYPES[dtype], "ints", seed=dim)
    gen = torch.Generator(device=DEV).manual_seed(2000 + dim)
    for aggrs in (("sum",), ("max",), ("min",), ("max", "min"), ("sum", "max", "min"), ("min", "sum")):
        grads = torch.randint(-4, 5, (p.num_rows, len(aggrs), dim), device=DEV, generator=gen).float()
        _, state = voltrix.spmm_multi(p.indptr, p.indices, feat, p.num_rows, aggrs=aggrs, return_state=True)
        got = _backward(p, feat, aggrs, grads, state)
        want, _ = oracle.backward(p.indptr, p.indices, feat, p.num_rows, {name: grads[:, i] for i, name in enumerate(aggrs)})
        assert got.dtype == torch.float32 and got.shape == (p.num_cols, dim) and torch.equal(got.double(), want), aggrs


@pytest.mark.parametrize("dtype,dim", [("fp32", 20), ("fp32", 260), ("fp16", 24), ("bf16", 520), ("fp32", 3)])
def test_backward_of_all_six_stays_inside_the_derived_bound(cuda_device, dtype, dim):
    import voltrix

    p = _main_pattern()
    gen = torch.Generator(device=DEV).manual_seed(3000 + dim)
    worst = {}
    for kind in ("normal", "offset"):
        feat = _features(p, dim, DTYPES[dtype], kind, seed=dim)
        for aggrs in (ALL, PNA, ("var",), ("std", "mean")):
            grads = torch.randn(p.num_rows, len(aggrs), dim, device=DEV, generator=gen)
            _, state = voltrix.spmm_multi(p.indptr, p.indices, feat, p.num_rows, aggrs=aggrs, eps=EPS, return_state=True)
            got = _backward(p, feat, aggrs, grads, state)
            want, bound = oracle.backward(p.indptr, p.indices, feat, p.num_rows, {n: grads[:, i] for i, n in enumerate(aggrs)}, EPS)
            err = (got.double() - want).abs()
            worst[(kind, len(aggrs))] = round(float((err / bound.clamp_min(1e-300)).max()), 4)
            assert bool(got.isfinite().all()) and bool((err <= bound).all()), (kind, aggrs, worst)
            untouched = (p.t_indptr[1:] == p.t_indptr[:-1])
            assert bool((got[untouched] == 0).all())
    print(f"backward {dtype} F={dim}: worst err / bound by (kind, aggregates): {worst}")


def test_the_same_bits_on_a_second_call(cuda_device):
    import voltrix

    p = _main_pattern()
    for dtype, dim in ((torch.float32, 260), (torch.bfloat16, 24)):
        feat = _features(p, dim, dtype, "offset", seed=8)
        grads = torch.randn(p.num_rows, 6, dim, device=DEV)
        runs = []
        for _ in range(2):
            out, state = voltrix.spmm_multi(p.indptr, p.indices, feat, p.num_rows, aggrs=ALL, return_state=True)
            runs.append((out, state.argmax, state.argmin, _backward(p, feat, ALL, grads, state)))
        for first, second in zip(*runs):
            assert _same_bits(first, second)


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
def test_autograd_operator(cuda_device, dtype):
    import voltrix
    from voltrix.autograd import CsrPattern, SpMMMulti

    p = _main_pattern()
    dt = DTYPES[dtype]
    shared = CsrPattern(p.indptr, p.indices, p.num_rows, p.num_cols)
    dim = 24
    saved_for = {("sum",): [], ("mean",): [], ("sum", "mean"): [], ("mean", "max"): ["arg"], ("min", "max"): ["arg", "arg"],
                 ("var",): ["stat", "feat"], ("std",): ["stat", "stat", "feat"], PNA: ["arg", "arg", "stat", "stat", "feat"],
                 ALL: ["arg", "arg", "stat", "stat", "feat"]}
    for aggrs, kinds in saved_for.items():
        feat = _features(p, dim, dt, "normal", seed=9).requires_grad_(True)
        op = SpMMMulti(shared, aggrs=aggrs, eps=EPS)
        assert op.pattern is shared and op.aggrs == aggrs
        out = op(feat)
        assert out.shape == (p.num_rows, len(aggrs), dim) and out.dtype == torch.float32
        saved = out.grad_fn.saved_tensors
        assert len(saved) == len(kinds), (aggrs, [tuple(t.shape) for t in saved])
        for t, kind in zip(saved, kinds):
            if kind == "arg":
                assert t.dtype == torch.int32 and t.shape == (p.num_rows, dim)
            elif kind == "stat":
                assert t.dtype == torch.float32 and t.shape == (p.num_rows, dim)
            else:
                assert t.data_ptr() == feat.data_ptr()                       # feat itself, as stored
        if "feat" not in kinds:
            assert all(t.data_ptr() != feat.data_ptr() for t in saved)       # never feat where no moment is asked for
        weight = torch.randn(p.num_rows, len(aggrs), dim, device=DEV)
        (out * weight).sum().backward()
        want_out, state = voltrix.spmm_multi(p.indptr, p.indices, feat.detach(), p.num_rows, aggrs=aggrs, eps=EPS, return_state=True)
        assert _same_bits(out.detach(), want_out)
        mine = Pattern.__new__(Pattern)
        mine.__dict__.update(p.__dict__)
        mine.t_indptr, mine.t_indices, mine.t_order = shared.t_indptr, shared.t_indices, shared.t_order
        want = _backward(mine, feat.detach(), aggrs, weight, state).to(dt)
        assert feat.grad.dtype == dt and feat.grad.shape == feat.shape and _same_bits(feat.grad, want), aggrs
    # a pattern of its own; the gradient of all six inside the bound, after the cast to feat's dtype
    feat = _features(p, dim, dt, "offset", seed=10).requires_grad_(True)
    op = SpMMMulti(p.indptr, p.indices, p.num_rows, p.num_cols, aggrs=ALL, eps=EPS)
    weight = torch.randn(p.num_rows, 6, dim, device=DEV)
    (op(feat) * weight).sum().backward()
    want, bound = oracle.backward(p.indptr, p.indices, feat.detach(), p.num_rows, {n: weight[:, i] for i, n in enumerate(ALL)}, EPS)
    rnd = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}[dt]
    cast = bound + rnd * (want.abs() + bound) + (2.0 ** -25 if dt == torch.float16 else 0.0)      # one rounding of the computed value
    assert bool(((feat.grad.double() - want).abs() <= cast).all())


def test_a_non_finite_feature_makes_the_moment_gradients_nan(cuda_device):
    from voltrix.autograd import SpMMMulti

    p = Pattern([3, 2, 0, 1], [0, 1, 2, 3, 4, 5], 7)
    feat = torch.arange(14, dtype=torch.float32, device=DEV).view(7, 2).clone()
    feat[1, 0] = float("inf")
    feat.requires_grad_(True)
    op = SpMMMulti(p.indptr, p.indices, 4, 7, aggrs=("std", "max"))
    op(feat).sum().backward()
    assert bool(feat.grad[:3, 0].isnan().all()) and bool(feat.grad[:3, 1].isfinite().all()) and bool(feat.grad[3:].isfinite().all())
    assert bool((feat.grad[6] == 0).all())                                    # a column without entries


# ----------------------------------------------------------------------------------------------- degenerate calls, layouts, memory
def test_degenerate_calls(cuda_device):
    import voltrix

    feat = torch.randn(30, 12, device=DEV) - 5.0
    # a graph of a single entry
    one = Pattern([1], [17], 30)
    out, state, _, _ = _forward_checked(one, feat, "single entry")
    assert torch.equal(out[0, 0], feat[17]) and bool((out[0, 4] == 0).all()) and bool((state.argmax == 0).all())
    grads = torch.randn(1, 6, 12, device=DEV)
    got = _backward(one, feat, ALL, grads, state)
    want = grads[0, 0] + grads[0, 1] + grads[0, 2] + grads[0, 3]              # var and std pass nothing: x - mean == 0
    assert torch.equal(got[17], want) and int(torch.count_nonzero(got)) == int(torch.count_nonzero(got[17]))
    # one row of five entries
    _forward_checked(Pattern([5], [3, 3, 7, 20, 29], 30), feat, "one row")
    # rows present, no entries (nnz == 0): zeros, args -1, zero gradients; indices and feat are not read
    none = Pattern([0] * 7, [], 30)
    for operand in (feat, torch.empty(0, 12, device=DEV)):
        out, state = voltrix.spmm_multi(none.indptr, none.indices, operand, 7, aggrs=ALL, return_state=True)
        assert out.shape == (7, 6, 12) and bool((out == 0).all()) and bool((state.argmax == -1).all()) and bool((state.argmin == -1).all())
    d = voltrix.spmm_multi.backward(none.t_indptr, none.t_indices, none.t_order, 30, feat=feat, u=torch.ones(7, 12, device=DEV),
                                    w=torch.ones(7, 12, device=DEV), mean=state.mean, g_max=torch.ones(7, 12, device=DEV),
                                    argmax=state.argmax, g_min=torch.ones(7, 12, device=DEV), argmin=state.argmin)
    assert d.shape == (30, 12) and bool((d == 0).all())
    # no rows
    zero = Pattern([], [], 30)
    out, state = voltrix.spmm_multi(zero.indptr, zero.indices, feat, 0, aggrs=PNA, return_state=True)
    assert out.shape == (0, 4, 12) and state.argmax.shape == state.mean.shape == state.std.shape == (0, 12)
    d = voltrix.spmm_multi.backward(zero.t_indptr, zero.t_indices, zero.t_order, 30, u=torch.ones(0, 12, device=DEV))
    assert d.shape == (30, 12) and bool((d == 0).all())
    # no features
    p = _main_pattern()
    out, state = voltrix.spmm_multi(p.indptr, p.indices, torch.empty(p.num_cols, 0, device=DEV), p.num_rows, aggrs=ALL, return_state=True)
    assert out.shape == (p.num_rows, 6, 0) and state.argmin.shape == state.std.shape == (p.num_rows, 0)
    wide = voltrix.spmm_multi(p.indptr, p.indices, torch.empty(p.num_cols, 3, 0, device=DEV), p.num_rows)
    assert wide.shape == (p.num_rows, 4, 3, 0)
    # other dtypes go through fp32
    ints = torch.randint(-3, 4, (30, 5), device=DEV)
    as_int = voltrix.spmm_multi(one.indptr, one.indices, ints.double(), 1, aggrs=ALL)
    assert torch.equal(as_int, voltrix.spmm_multi(one.indptr, one.indices, ints.float(), 1, aggrs=ALL))


def test_views_give_the_bits_of_the_contiguous_call(cuda_device):
    import voltrix

    p = _main_pattern()
    for dtype, dim in ((torch.float32, 20), (torch.float16, 24)):
        feat = _features(p, dim, dtype, "offset", seed=4)
        grads = torch.randn(p.num_rows, 6, dim, device=DEV)
        want, want_state = voltrix.spmm_multi(p.indptr, p.indices, feat, p.num_rows, aggrs=ALL, return_state=True)
        want_d = _backward(p, feat, ALL, grads, want_state)
        wide = torch.randn(p.num_cols, dim + 9, device=DEV).to(dtype)
        wide[:, 5:5 + dim] = feat
        flat = torch.zeros(feat.numel() + 3, dtype=dtype, device=DEV)
        flat[3:] = feat.reshape(-1)
        offset = flat[3:].view(p.num_cols, dim)
        assert offset.data_ptr() % 16 != 0 and not wide[:, 5:5 + dim].is_contiguous()
        wide_grads = torch.randn(p.num_rows, 6, dim + 3, device=DEV)
        wide_grads[:, :, 1:1 + dim] = grads
        for view in (wide[:, 5:5 + dim], offset):
            out, state = voltrix.spmm_multi(p.indptr, p.indices, view, p.num_rows, aggrs=ALL, return_state=True)
            assert _same_bits(out, want) and torch.equal(state.argmax, want_state.argmax) and torch.equal(state.argmin, want_state.argmin)
            assert _same_bits(_backward(p, view, ALL, wide_grads[:, :, 1:1 + dim], state), want_d)


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_poisoned_scratch_and_output_memory(cuda_device, byte):
    import voltrix

    p = _main_pattern()
    for dtype, dim, aggrs in ((torch.float32, 20, ALL), (torch.float16, 50, ALL), (torch.float32, 7, ("var", "max"))):
        feat = _features(p, dim, dtype, "ints", seed=6)
        grads = torch.randn(p.num_rows, len(aggrs), dim, device=DEV)
        want, want_state = voltrix.spmm_multi(p.indptr, p.indices, feat, p.num_rows, aggrs=aggrs, return_state=True)
        want_d = _backward(p, feat, aggrs, grads, want_state)
        with poisoned(byte) as poison:
            out, state = voltrix.spmm_multi(p.indptr, p.indices, feat, p.num_rows, aggrs=aggrs, return_state=True)
            d = _backward(p, feat, aggrs, grads, state)
        assert poison.filled > 0
        assert _same_bits(out, want) and torch.equal(state.argmax, want_state.argmax) and _same_bits(d, want_d)
        assert state.argmin is None or torch.equal(state.argmin, want_state.argmin)


def test_trailing_dimensions_are_the_flat_call(cuda_device):
    import voltrix

    p = _main_pattern()
    feat = _features(p, 64, torch.float16, "normal", seed=5)
    flat, flat_state = voltrix.spmm_multi(p.indptr, p.indices, feat, p.num_rows, aggrs=ALL, return_state=True)
    out, state = voltrix.spmm_multi(p.indptr, p.indices, feat.view(-1, 4, 16), p.num_rows, aggrs=ALL, return_state=True)
    assert out.shape == (p.num_rows, 6, 4, 16) and _same_bits(out.view(p.num_rows, 6, 64), flat)
    for got, want in zip(state, flat_state):
        assert got.shape == (p.num_rows, 4, 16) and _same_bits(got.reshape(p.num_rows, 64), want.contiguous())
    grads = torch.randn(p.num_rows, 6, 4, 16, device=DEV)
    d3 = _backward(p, feat.view(-1, 4, 16), ALL, grads, state)
    d2 = _backward(p, feat, ALL, grads.view(p.num_rows, 6, 64), flat_state)
    assert d3.shape == (p.num_cols, 4, 16) and _same_bits(d3.view(-1, 64), d2)
    # through autograd
    from voltrix.autograd import SpMMMulti

    x = feat.view(-1, 4, 16).clone().requires_grad_(True)
    y = SpMMMulti(p.indptr, p.indices, p.num_rows, p.num_cols, aggrs=ALL)(x)
    (y * grads).sum().backward()
    assert y.shape == (p.num_rows, 6, 4, 16) and x.grad.shape == x.shape and _same_bits(x.grad, d3.to(torch.float16))


# ------------------------------------------------------------------------------------------------------------------------ example
def test_pna_example_trains(cuda_device):
    """examples/pna_train.py's two-layer PNA on csr_cora_like: a few epochs with a finite, decreasing loss."""
    from voltrix.autograd import CsrPattern, SpMMMulti

    sys.path.insert(0, os.path.join(REPO, "examples"))
    try:
        import pna_train
    finally:
        sys.path.remove(os.path.join(REPO, "examples"))
    p = _fixture_pattern("cora_like")
    in_feats, hidden, classes = 24, 32, 7
    torch.manual_seed(9)
    op = SpMMMulti(CsrPattern(p.indptr, p.indices, p.num_rows), aggrs=pna_train.AGGREGATORS)
    scalers = pna_train.degree_scalers(p.indptr)
    assert scalers.shape == (p.num_rows, 3) and bool(scalers.isfinite().all()) and bool((scalers[p.empty, 1:] == 0).all())
    model = pna_train.PNA(op, scalers, in_feats, hidden, classes).to(DEV)
    assert model.l1.w_neigh.in_features == 12 * in_feats
    x = torch.randn(p.num_rows, in_feats, device=DEV)
    y = torch.randint(0, classes, (p.num_rows,), device=DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)       # the example's rate: a layer of 12 F inputs overshoots at 1e-2
    losses = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        logits = model(x)
        assert logits.shape == (p.num_rows, classes)
        loss = torch.nn.functional.cross_entropy(logits, y)
        loss.backward()
        assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in model.parameters())
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)) and losses[2] < losses[1] < losses[0], losses
