"""GPU: ``voltrix.spmm_reduce`` (max / min / mean over every row's entries), its backward on the transposed CSR and
``voltrix.autograd.SpMMReduce`` against torch float64 on the device, from the inputs as stored.

The oracle of max / min is ``zeros.scatter_reduce(0, rows, feat.double()[cols], "amax" | "amin", include_self=False)`` -- rows without
entries stay 0, a NaN among a row's entries gives NaN -- and the winner is the ``amin`` scatter of the entry ids where ``feat[cols] ==
ref[rows]`` or both are NaN: the lowest entry id among the ties, ``-1`` for a row without entries.  A selection does not round, so
``out`` and ``arg`` are compared for equality (``_same``: ``==`` element by element, a NaN equal to a NaN), for every dtype.

mean: ``|out - ref| <= (deg + 1) 2^-23 sum_e |feat_e| / deg`` (deg - 1 fp32 additions in CSR order and one division, each within 2^-24
of its result: (deg - 1 + 1) 2^-24 is within the bound).  Backward: float64 ``index_add`` of ``grad_out[r, f]`` at
``(indices[arg[r, f]], f)``, within ``k 2^-23 sum |terms|`` for the ``k`` terms that land on an element (k - 1 fp32 additions), equal for
integer gradients.
"""
import gc
import os
import sys

import numpy as np
import pytest
import torch

import large_offset_cases as loc
from conftest import REPO, load_csr_fixture
from poisoned_alloc import poisoned

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
BIG_ID = 2 ** 40
DEV = "cuda"
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


# ------------------------------------------------------------------------------------------------------------------- the patterns
class Pattern:
    """A device int32 CSR with its per-entry row ids and its transpose by a stable sort by column, built with torch alone."""

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
        self.rows, self.cols = dev(rows, torch.int64), dev(cols, torch.int64)
        self.t_indptr, self.t_indices, self.t_order = dev(t_ip, torch.int32), dev(rows[order], torch.int32), dev(order, torch.int32)
        self.deg = dev(lengths, torch.float64)


_CACHE = {}


def _main_pattern():
    """1,003 rows over 300 columns: row lengths 0 .. 9 on both sides of the 4-edge batch, a hub of 5,003 entries, short random rows;
    columns sorted inside a row, duplicates many (the hub holds every column about 17 times)."""
    if "main" not in _CACHE:
        rng = np.random.default_rng(11)
        lengths = [0, 1, 2, 3, 4, 5, 7, 8, 9, 0, 6, 1] + [int(v) for v in rng.integers(0, 13, 500)] + [5003]
        lengths += [int(v) for v in rng.integers(0, 13, 1003 - len(lengths))]
        lengths = np.asarray(lengths, np.int64)
        assert len(lengths) == 1003 and all(len(lengths) % r for r in (4, 8, 16, 32, 64, 128, 256))
        rows = np.repeat(np.arange(len(lengths)), lengths)
        cols = np.sort(rows * 300 + rng.integers(0, 300, rows.size)) % 300
        p = Pattern(lengths, cols, 300)
        key = rows * 300 + cols
        assert len(np.unique(key)) < key.size - 1000                     # duplicates are many
        _CACHE["main"] = p
    return _CACHE["main"]


def _fixture_pattern(name):
    if name not in _CACHE:
        g = load_csr_fixture(name)
        n = int(g["num_nodes"])
        ip = np.asarray(g["indptr"], np.int64)
        _CACHE[name] = Pattern(ip[1:] - ip[:-1], g["indices"], n)
    return _CACHE[name]


def _pattern(name):
    return _main_pattern() if name == "main" else _fixture_pattern(name)


# --------------------------------------------------------------------------------------------------------------------- the inputs
def _features(p, dim, dtype, kind, seed=0):
    """[num_cols, dim] of ``dtype``: "normal"; "ints" in [-3, -1] (all negative: a zero-initialised accumulator shows; many ties:
    first-wins shows); "special": normal with NaN, +inf and -inf sprinkled in, the columns of the first 3-entry row all -inf and the
    column of the first 1-entry row NaN."""
    gen = torch.Generator(device=DEV).manual_seed(1000 + seed)
    if kind == "ints":
        return torch.randint(-3, 0, (p.num_cols, dim), device=DEV, generator=gen).to(dtype)
    feat = torch.randn(p.num_cols, dim, device=DEV, generator=gen)
    if kind == "special":
        dice = torch.rand(p.num_cols, dim, device=DEV, generator=gen)
        feat[dice < 0.01] = float("nan")
        feat[(dice >= 0.01) & (dice < 0.03)] = float("inf")
        feat[(dice >= 0.03) & (dice < 0.06)] = float("-inf")
        ip = p.indptr.tolist()
        three = int(np.flatnonzero(p.lengths == 3)[0])
        one = int(np.flatnonzero(p.lengths == 1)[0])
        feat[p.cols[ip[three]:ip[three + 1]]] = float("-inf")
        feat[p.cols[ip[one]]] = float("nan")
    return feat.to(dtype)


# --------------------------------------------------------------------------------------------------------------------- the oracle
def _oracle(rows, cols, feat, num_rows, reduce):
    """(ref float64 [num_rows, F], arg int64 [num_rows, F]) of max / min from ``feat`` as stored; rows / cols: int64 per entry."""
    f = feat.shape[1]
    g = feat.double()[cols]
    idx = rows[:, None].expand(-1, f)
    ref = torch.zeros(num_rows, f, dtype=torch.float64, device=feat.device)
    ref = ref.scatter_reduce(0, idx, g, "amax" if reduce == "max" else "amin", include_self=False)
    won = (g == ref[rows]) | (g.isnan() & ref[rows].isnan())
    ids = torch.arange(rows.numel(), device=feat.device)[:, None].expand(-1, f)
    arg = torch.full((num_rows, f), BIG_ID, dtype=torch.int64, device=feat.device)
    arg = arg.scatter_reduce(0, idx, torch.where(won, ids, torch.full_like(ids, BIG_ID)), "amin", include_self=True)
    return ref, torch.where(arg == BIG_ID, torch.full_like(arg, -1), arg)


def _same(got, ref):
    """Equality element by element, a NaN equal to a NaN (torch.equal but for that)."""
    got, ref = got.double(), ref.double()
    return got.shape == ref.shape and bool(((got == ref) | (got.isnan() & ref.isnan())).all())


def _backward_oracle(p, arg, grad):
    """(d_feat float64 [num_cols, F], bound, count) from the forward's arg [num_rows, F] and grad [num_rows, F]."""
    f = arg.shape[1]
    valid = arg >= 0
    col = p.cols[arg.long().clamp(min=0)]
    lin = (col * f + torch.arange(f, device=arg.device)[None, :])[valid]
    g = grad.double()[valid]
    flat = lambda: torch.zeros(p.num_cols * f, dtype=torch.float64, device=arg.device)     # noqa: E731
    ref = flat().index_add_(0, lin, g).view(p.num_cols, f)
    mass = flat().index_add_(0, lin, g.abs()).view(p.num_cols, f)
    count = flat().index_add_(0, lin, torch.ones_like(g)).view(p.num_cols, f)
    return ref, count * U * mass, count


def _forward_checked(p, feat, reduce):
    """The public call with and without the argument, both against the oracle; returns (out, arg)."""
    import voltrix

    out, arg = voltrix.spmm_reduce(p.indptr, p.indices, feat, p.num_rows, reduce=reduce, return_arg=True)
    alone = voltrix.spmm_reduce(p.indptr, p.indices, feat, p.num_rows, reduce=reduce)
    assert out.dtype == torch.float32 and arg.dtype == torch.int32 and out.shape == arg.shape == (p.num_rows, feat.shape[1])
    ref, ref_arg = _oracle(p.rows, p.cols, feat, p.num_rows, reduce)
    assert _same(out, ref), (reduce, feat.dtype, tuple(feat.shape))
    assert torch.equal(arg.long(), ref_arg), (reduce, feat.dtype, tuple(feat.shape))
    assert _same(alone, out) and torch.equal(alone.isnan(), out.isnan())
    assert torch.equal(alone.view(torch.int32)[~out.isnan()], out.view(torch.int32)[~out.isnan()])      # the same bits
    return out, arg


def _backward_checked(p, arg, seed=0):
    from voltrix.spmm_reduce import spmm_reduce_backward

    gen = torch.Generator(device=DEV).manual_seed(2000 + seed)
    grad_int = torch.randint(-4, 5, arg.shape, device=DEV, generator=gen).float()
    got = spmm_reduce_backward(p.t_indptr, p.t_indices, p.t_order, grad_int, arg, p.num_cols)
    ref, _, _ = _backward_oracle(p, arg, grad_int)
    assert got.dtype == torch.float32 and torch.equal(got.double(), ref)
    grad = torch.randn(arg.shape, device=DEV, generator=gen)
    got = spmm_reduce_backward(p.t_indptr, p.t_indices, p.t_order, grad, arg, p.num_cols)
    again = spmm_reduce_backward(p.t_indptr, p.t_indices, p.t_order, grad, arg, p.num_cols)
    ref, bound, _ = _backward_oracle(p, arg, grad)
    err = (got.double() - ref).abs()
    print(f"backward {tuple(arg.shape)}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    return got


# ----------------------------------------------------------------------------------------------------------------------- max / min
WIDTHS = [("fp32", f) for f in (4, 12, 20, 256, 260)] + [(d, f) for d in ("fp16", "bf16") for f in (8, 24, 520)]


@pytest.mark.parametrize("dtype,dim", WIDTHS)
def test_max_min_and_their_backward_on_the_main_pattern(cuda_device, dtype, dim):
    p = _main_pattern()
    for kind in ("normal", "ints", "special"):
        feat = _features(p, dim, DTYPES[dtype], kind, seed=dim)
        for reduce in ("max", "min"):
            out, arg = _forward_checked(p, feat, reduce)
            if kind == "special":
                ip = p.indptr.tolist()
                three, one = int(np.flatnonzero(p.lengths == 3)[0]), int(np.flatnonzero(p.lengths == 1)[0])
                assert bool((out[three] == float("-inf")).all()) and bool((arg[three] == ip[three]).all())
                assert bool(out[one].isnan().all()) and bool((arg[one] == ip[one]).all())
                assert bool(out.isnan().any()) and bool(out.isinf().any())
            empty = torch.from_numpy(p.lengths == 0).to(DEV)
            assert bool((out[empty] == 0).all()) and bool((arg[empty] == -1).all()) and int(empty.sum()) > 0
        if kind != "normal" or dim in (4, 260, 24, 520):
            _backward_checked(p, arg, seed=dim)


@pytest.mark.parametrize("name", ["toy40", "skewed_1005", "cora_like"])
def test_the_fixture_patterns(cuda_device, name):
    p = _pattern(name)
    for dtype, dim in (("fp32", 20), ("fp16", 24), ("bf16", 8)):
        for kind in ("normal", "ints"):
            feat = _features(p, dim, DTYPES[dtype], kind, seed=7)
            for reduce in ("max", "min"):
                _, arg = _forward_checked(p, feat, reduce)
            _backward_checked(p, arg, seed=3)
            _mean_checked(p, feat)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("dim", [1, 3, 7, 50])
def test_widths_that_need_padding(cuda_device, dtype, dim):
    p = _main_pattern()
    for kind in ("normal", "ints"):
        feat = _features(p, dim, DTYPES[dtype], kind, seed=dim)
        for reduce in ("max", "min"):
            _, arg = _forward_checked(p, feat, reduce)
        _backward_checked(p, arg, seed=dim)
        _mean_checked(p, feat)


def test_trailing_dimensions_are_the_flat_call(cuda_device):
    import voltrix
    from voltrix.spmm_reduce import spmm_reduce_backward

    p = _main_pattern()
    feat = _features(p, 64, torch.float16, "normal", seed=5)
    flat, flat_arg = voltrix.spmm_reduce(p.indptr, p.indices, feat, p.num_rows, "max", return_arg=True)
    out, arg = voltrix.spmm_reduce(p.indptr, p.indices, feat.view(-1, 4, 16), p.num_rows, "max", return_arg=True)
    assert out.shape == arg.shape == (p.num_rows, 4, 16)
    assert torch.equal(out.view(p.num_rows, 64), flat) and torch.equal(arg.view(p.num_rows, 64), flat_arg)
    mean = voltrix.spmm_reduce(p.indptr, p.indices, feat.view(-1, 4, 16), p.num_rows, "mean")
    assert torch.equal(mean.view(p.num_rows, 64), voltrix.spmm_reduce(p.indptr, p.indices, feat, p.num_rows, "mean"))
    grad = torch.randn(p.num_rows, 4, 16, device=DEV)
    d3 = spmm_reduce_backward(p.t_indptr, p.t_indices, p.t_order, grad, arg, p.num_cols)
    d2 = spmm_reduce_backward(p.t_indptr, p.t_indices, p.t_order, grad.view(-1, 64), flat_arg, p.num_cols)
    assert d3.shape == (p.num_cols, 4, 16) and torch.equal(d3.view(-1, 64), d2)


def test_degenerate_calls(cuda_device):
    import voltrix
    from voltrix.spmm_reduce import spmm_reduce_backward

    feat = torch.randn(30, 12, device=DEV) - 5.0
    # one row
    one = Pattern([5], [3, 3, 7, 20, 29], 30)
    for reduce in ("max", "min"):
        _, arg = _forward_checked(one, feat, reduce)
        _backward_checked(one, arg)
    _mean_checked(one, feat)
    # rows present, no entries: zeros, arg = -1, zero gradients
    none = Pattern([0] * 7, [], 30)
    for reduce in ("max", "min"):
        out, arg = voltrix.spmm_reduce(none.indptr, none.indices, feat, 7, reduce, return_arg=True)
        assert out.shape == (7, 12) and bool((out == 0).all()) and bool((arg == -1).all())
        d = spmm_reduce_backward(none.t_indptr, none.t_indices, none.t_order, torch.ones(7, 12, device=DEV), arg, 30)
        assert d.shape == (30, 12) and bool((d == 0).all())
    assert bool((voltrix.spmm_reduce(none.indptr, none.indices, feat, 7, "mean") == 0).all())
    # no rows
    zero = Pattern([], [], 30)
    out, arg = voltrix.spmm_reduce(zero.indptr, zero.indices, feat, 0, "max", return_arg=True)
    assert out.shape == arg.shape == (0, 12)
    assert voltrix.spmm_reduce(zero.indptr, zero.indices, feat, 0, "mean").shape == (0, 12)
    d = spmm_reduce_backward(zero.t_indptr, zero.t_indices, zero.t_order, torch.ones(0, 12, device=DEV), arg, 30)
    assert d.shape == (30, 12) and bool((d == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------- mean
def _mean_checked(p, feat):
    import voltrix

    out = voltrix.spmm_reduce(p.indptr, p.indices, feat, p.num_rows, reduce="mean")
    assert out.dtype == torch.float32 and out.shape == (p.num_rows, feat.shape[1])
    g = feat.double()[p.cols]
    zeros = lambda: torch.zeros(p.num_rows, feat.shape[1], dtype=torch.float64, device=DEV)     # noqa: E731
    deg = p.deg.clamp(min=1)[:, None]
    ref = zeros().index_add_(0, p.rows, g) / deg
    bound = (p.deg[:, None] + 1) * U * zeros().index_add_(0, p.rows, g.abs()) / deg
    err = (out.double() - ref).abs()
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    assert bool((out[torch.from_numpy(p.lengths == 0).to(DEV)] == 0).all())
    return out


@pytest.mark.parametrize("dtype,dim", WIDTHS)
def test_mean_on_the_main_pattern(cuda_device, dtype, dim):
    p = _main_pattern()
    _mean_checked(p, _features(p, dim, DTYPES[dtype], "normal", seed=dim))
    _mean_checked(p, _features(p, dim, DTYPES[dtype], "ints", seed=dim))
    # integers whose row sums are multiples of the degree: every column holds one integer, so the mean is that integer, exactly
    const = torch.randint(-5, 6, (1, dim), device=DEV).float().expand(p.num_cols, dim).to(DTYPES[dtype]).contiguous()
    out = _mean_checked(p, const)
    want = torch.where(p.deg[:, None] > 0, const[:1].double().expand(p.num_rows, dim), torch.zeros((), dtype=torch.float64, device=DEV))
    assert torch.equal(out.double(), want)


# ------------------------------------------------------------------------------------------------------------------------ backward
def test_duplicates_do_not_count_twice(cuda_device):
    """An all-ones gradient: every non-empty row hands exactly one unit per feature to exactly one entry, duplicates or not."""
    import voltrix
    from voltrix.spmm_reduce import spmm_reduce_backward

    p = _main_pattern()
    nonempty = int((p.lengths > 0).sum())
    for kind in ("ints", "normal"):
        feat = _features(p, 20, torch.float32, kind, seed=1)
        for reduce in ("max", "min"):
            _, arg = voltrix.spmm_reduce(p.indptr, p.indices, feat, p.num_rows, reduce, return_arg=True)
            d = spmm_reduce_backward(p.t_indptr, p.t_indices, p.t_order, torch.ones(p.num_rows, 20, device=DEV), arg, p.num_cols)
            assert torch.equal(d.sum(0), torch.full((20,), float(nonempty), device=DEV)), (kind, reduce)


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
def test_autograd_operator(cuda_device, dtype):
    from voltrix.autograd import CsrPattern, SpMMReduce
    from voltrix.spmm_reduce import spmm_reduce, spmm_reduce_backward

    p = _main_pattern()
    dt = DTYPES[dtype]
    shared = CsrPattern(p.indptr, p.indices, p.num_rows, p.num_cols)
    # the operator's transpose is this file's, up to the order of duplicate (row, col) entries among themselves
    order = shared.t_order.long()
    assert torch.equal(shared.t_indptr, p.t_indptr) and torch.equal(shared.t_indices, p.t_indices)
    assert torch.equal(p.rows[order], p.t_indices.long()) and torch.equal(p.cols[order], p.cols[p.t_order.long()])
    assert torch.equal(order.sort().values, torch.arange(p.nnz, device=DEV))
    weight = torch.randn(p.num_rows, 24, device=DEV)
    for reduce in ("max", "min"):
        feat = _features(p, 24, dt, "normal", seed=9).requires_grad_(True)
        op = SpMMReduce(shared, reduce=reduce)
        assert op.pattern is shared
        out = op(feat)
        saved = out.grad_fn.saved_tensors
        assert len(saved) == 1 and saved[0].dtype == torch.int32 and saved[0].shape == out.shape      # arg only, never feat
        (out * weight).sum().backward()
        want_out, arg = spmm_reduce(p.indptr, p.indices, feat.detach(), p.num_rows, reduce, return_arg=True)
        want = spmm_reduce_backward(p.t_indptr, p.t_indices, p.t_order, weight, arg, p.num_cols).to(dt)
        assert torch.equal(out.detach(), want_out) and feat.grad.dtype == dt and torch.equal(feat.grad, want)
    feat = _features(p, 24, dt, "normal", seed=10).requires_grad_(True)
    op = SpMMReduce(p.indptr, p.indices, p.num_rows, p.num_cols, reduce="mean")
    out = op(feat)
    (out * weight).sum().backward()
    assert feat.grad.dtype == dt
    scaled = weight.double() / p.deg.clamp(min=1)[:, None]
    zeros = lambda: torch.zeros(p.num_cols, 24, dtype=torch.float64, device=DEV)     # noqa: E731
    ref = zeros().index_add_(0, p.cols, scaled[p.rows])
    col_deg = (p.t_indptr[1:] - p.t_indptr[:-1]).double()[:, None]
    bound = (col_deg + 1) * U * zeros().index_add_(0, p.cols, scaled[p.rows].abs())      # the division's rounding and the column's sum
    err = (feat.grad.double() - ref).abs()
    assert bool((err <= loc.cast_bound(ref, bound, dt)).all())


# ------------------------------------------------------------------------------------------------------ layouts, undefined memory
def test_views_give_the_bits_of_the_contiguous_call(cuda_device):
    import voltrix

    p = _main_pattern()
    for dtype, dim in ((torch.float32, 20), (torch.float16, 24)):
        feat = _features(p, dim, dtype, "normal", seed=4)
        want, want_arg = voltrix.spmm_reduce(p.indptr, p.indices, feat, p.num_rows, "max", return_arg=True)
        want_mean = voltrix.spmm_reduce(p.indptr, p.indices, feat, p.num_rows, "mean")
        wide = torch.randn(p.num_cols, dim + 9, device=DEV).to(dtype)
        wide[:, 5:5 + dim] = feat
        flat = torch.zeros(feat.numel() + 3, dtype=dtype, device=DEV)
        flat[3:] = feat.reshape(-1)
        offset = flat[3:].view(p.num_cols, dim)
        assert offset.data_ptr() % 16 != 0 and not wide[:, 5:5 + dim].is_contiguous()
        for view in (wide[:, 5:5 + dim], offset):
            out, arg = voltrix.spmm_reduce(p.indptr, p.indices, view, p.num_rows, "max", return_arg=True)
            assert torch.equal(out, want) and torch.equal(arg, want_arg)
            assert torch.equal(voltrix.spmm_reduce(p.indptr, p.indices, view, p.num_rows, "mean"), want_mean)


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_poisoned_scratch_and_output_memory(cuda_device, byte):
    import voltrix
    from voltrix.spmm_reduce import spmm_reduce_backward

    p = _main_pattern()
    for dtype, dim in ((torch.float32, 20), (torch.float16, 50)):
        feat = _features(p, dim, dtype, "ints", seed=6)
        grad = torch.randn(p.num_rows, dim, device=DEV)
        want, want_arg = voltrix.spmm_reduce(p.indptr, p.indices, feat, p.num_rows, "min", return_arg=True)
        want_mean = voltrix.spmm_reduce(p.indptr, p.indices, feat, p.num_rows, "mean")
        want_d = spmm_reduce_backward(p.t_indptr, p.t_indices, p.t_order, grad, want_arg, p.num_cols)
        with poisoned(byte) as state:
            out, arg = voltrix.spmm_reduce(p.indptr, p.indices, feat, p.num_rows, "min", return_arg=True)
            mean = voltrix.spmm_reduce(p.indptr, p.indices, feat, p.num_rows, "mean")
            d = spmm_reduce_backward(p.t_indptr, p.t_indices, p.t_order, grad, arg, p.num_cols)
        assert state.filled > 0
        assert torch.equal(out, want) and torch.equal(arg, want_arg) and torch.equal(mean, want_mean) and torch.equal(d, want_d)


# ---------------------------------------------------------------------------------------------------------------------- past 2^31
def _periodic_case(dim, num_cols, boundary):
    """max forward, arg and backward on a periodic pattern of short rows with ``num_rows * dim > boundary``, every element checked."""
    import voltrix
    from voltrix.spmm_reduce import spmm_reduce_backward

    rng = np.random.default_rng(21)
    lengths = np.asarray([0, 1, 2, 3, 4, 5, 7, 8, 9, 0, 6] + [int(v) for v in rng.integers(0, 10, 30)], np.int64)
    if lengths.sum() % 2 == 0:
        lengths[-1] += 1
    rows_np = np.repeat(np.arange(len(lengths)), lengths)
    cols_np = np.sort(rows_np * num_cols + rng.integers(0, num_cols // 2, rows_np.size)) % num_cols
    period_rows, period_edges = len(lengths), int(lengths.sum())
    reps = boundary // (dim * period_rows) + 1
    nnz = reps * period_edges + int(lengths[:7].sum()) + 2                 # a tail of seven whole rows and one cut to two entries
    pc = loc.Periodic(lengths, cols_np, num_cols, nnz, DEV)
    assert pc.reps == reps and pc.cut == 2 and pc.tail_rows == 8 and (pc.num_rows - pc.tail_rows) * dim > boundary
    indptr, indices = pc.indptr(), pc.indices()
    t_indptr, t_indices, t_order = pc.transposed()
    gen = torch.Generator(device=DEV).manual_seed(5)
    feat = torch.randint(-3, 4, (num_cols, dim), device=DEV, generator=gen).float()      # ties: first wins, in every period
    grad_p = torch.randint(-2, 3, (pc.P, dim), device=DEV, generator=gen).float()
    tally = loc.Tally()

    out, arg = voltrix.spmm_reduce(indptr, indices, feat, pc.num_rows, "max", return_arg=True)
    grad = pc.tile_rows(grad_p)
    d_feat = spmm_reduce_backward(t_indptr, t_indices, t_order, grad, arg, num_cols)
    del grad

    ref_p, arg_p = _oracle(pc.period.rows, pc.period.cols, feat, pc.P, "max")
    ref_t, arg_t = _oracle(pc.tail.rows, pc.tail.cols, feat, pc.tail_rows, "max")
    ok_out, _ = loc.check_tiled(out, pc.reps, (ref_p, None), (ref_t, None), "out", tally)
    del out

    # the backward's reference from the period's and the tail's winners: integer gradients, so the sums are exact
    def terms(g, won_at, grad_rows):
        won = won_at[g.rows] == torch.arange(g.nnz, device=DEV)[:, None]
        return torch.where(won, grad_rows.double()[g.rows], torch.zeros((), dtype=torch.float64, device=DEV))

    d_ref = pc.col_sum(terms(pc.period, arg_p, grad_p), terms(pc.tail, arg_t, grad_p[:pc.tail_rows]))
    assert float(d_ref.abs().max()) < 2 ** 24 and float(d_ref.abs().max()) > 0
    ok_d, _ = loc.check_whole(d_feat, d_ref, None, "d_feat", tally)
    # arg relative to its row's first entry is periodic (in place: no second tensor of its size); rows without entries keep -1
    start = indptr[:-1].clone()
    start[indptr[1:] == indptr[:-1]] = 0
    arg.sub_(start[:, None])
    first = lambda g: torch.from_numpy(g.ip[:-1] * (g.lengths > 0)).to(DEV)[:, None]     # noqa: E731
    ok_arg, _ = loc.check_tiled(arg, pc.reps, ((arg_p - first(pc.period)).double(), None),
                                ((arg_t - first(pc.tail)).double(), None), "arg", tally)
    tally.assert_complete("out", "arg", "d_feat")
    assert ok_out and ok_arg and ok_d, (ok_out, ok_arg, ok_d)


def test_element_offsets_past_2_to_31(cuda_device):
    """num_rows * F > 2^31 on a periodic pattern of short rows (tests/large_offset_cases.py): out, arg and the backward, every element.
    Peak: out, arg and grad_out of 8.1 GiB each and the comparison slabs."""
    gib = 1 << 30
    need = 3 * 8.1 + 5
    free, total = torch.cuda.mem_get_info()
    assert need <= 50 and free >= need * gib, f"this test needs {need:.1f} GiB of device memory, {free / gib:.1f} of {total / gib:.1f} GiB are free"
    try:
        _periodic_case(512, 2000, 2 ** 31)
    finally:
        gc.collect()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------------ example
@pytest.mark.parametrize("reduce", ["max", "mean"])
def test_sage_example_trains(cuda_device, reduce):
    """examples/sage_train.py's two-layer max-pool GraphSAGE on csr_cora_like: three epochs with a finite, decreasing loss.  Gradient
    parity with a dense float64 model is deliberately not asserted: a near-tie that resolves differently in fp32 and fp64 moves a
    gradient by a whole term; the exact arg checks above cover that ground."""
    from voltrix.autograd import CsrPattern, SpMMReduce

    sys.path.insert(0, os.path.join(REPO, "examples"))
    try:
        import sage_train
    finally:
        sys.path.remove(os.path.join(REPO, "examples"))
    p = _pattern("cora_like")
    in_feats, hidden, classes = 24, 32, 7
    torch.manual_seed(9)
    op = SpMMReduce(CsrPattern(p.indptr, p.indices, p.num_rows), reduce=reduce)
    model = sage_train.SAGE(op, in_feats, hidden, classes).to(DEV)
    x = torch.randn(p.num_rows, in_feats, device=DEV)
    y = torch.randint(0, classes, (p.num_rows,), device=DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
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
