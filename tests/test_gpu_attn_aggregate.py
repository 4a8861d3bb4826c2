"""GPU: edge softmax and aggregation in one launch (voltrix.attn_aggregate, attn_aggregate_kernels.hpp), the two launches of its backward
and autograd.AttnAggregate against float64 torch and against the unfused chain ``spmm_heads(edge_softmax(s, scale), feat)``.

Oracle, in float64 from the inputs as stored (fp32 / fp16 / bf16 values converted exactly) and ``float32(scale)``: ``key = sigma s``
(``sigma`` the sign of scale), ``m = scatter_reduce(amax)``, ``x = |scale| (m - key)``, ``W = exp(-x)`` (0 for ``key = -inf``), ``L`` and
every other row sum by ``index_add_`` on int64 ids (its own error, ~deg 2^-53, is nine orders below the bounds), ``alpha = W / L`` (0
where ``L = 0``), ``out = sum alpha feat``, ``delta = <dC, out>``, ``d_s = scale alpha (<dC[row], feat[col]> - delta[row])``,
``d_feat = sum_{e in column} alpha dC[row]``.

Bounds, derived from the kernels' roundings, ``u = 2^-23``, ``deg`` the row's (for d_feat the column's) entries:

* a weight ``exp(|scale| (key - m))``: the difference, the product with ``|scale|`` and the product with the rounded ``log2 e`` perturb
  the exponent by at most ``3.3 * 2^-24 x``; ``v_exp_f32`` adds one ulp: relative error ``E_e <= (2 x_e + 2) u`` (first-order slack
  included), and ``x exp(-x) <= 1/e`` bounds ``W_e x_e``.
* ``m`` is exact.  ``l`` is ``deg`` additions of such weights: ``|l - L| <= (deg + 2) u L + 2 u sum_e W_e x_e + deg 2^-126``.
* ``out = acc (1 / l)``: ``deg`` fused multiply-adds into ``acc`` (``deg 2^-24 sum W |feat|``), the weights' errors in ``acc`` and in ``l``,
  one reciprocal and one product; with ``A = sum_e alpha_e |feat_e|``, ``L >= 1`` and ``sum_e W_e x_e <= deg / e`` this is below
  ``2 (deg + 3) u A + u sum_e |feat_e| / L + 2^-126`` -- the form of the issue, constants confirmed: (1.65 deg + 4) u A + 0.65 u sum |feat| / L.
* ``alpha`` in the backward is ``W (1 / l)`` with the stored ``l``: relative error ``eta_e = E_e + bound(l) / L + 2 u``.
* ``d_s = scale (alpha (dot - delta))``: the SDDMM's ``(D + 2) u sum_d |dC| |feat|`` on ``dot``; ``delta`` is torch's fp32 product over
  ``D`` of ``dC`` and the computed ``out``, ``(D + 2) u sum_d |dC| |out| + sum_d |dC| bound(out)``; the difference and the two products
  round once each: ``|scale| alpha (bound(dot) + bound(delta) + |dot - delta| (eta + 2 u)) + 2^-126 (1 + |scale| |dot - delta|)``.
* ``d_feat``: the aggregation's ``deg_c u sum_e alpha_e |dC_e|`` plus ``sum_e alpha_e eta_e |dC_e|`` plus ``2^-126 (1 + sum_e |dC_e|)``.
* the cross-check against the unfused chain holds within the sum of both operators' bounds; the chain's is
  ``deg u sum_e alpha_e |feat_e| + sum_e bound(alpha_e) |feat_e|`` with the edge softmax's documented
  ``bound(alpha_e) = 2 alpha_e (deg + x_e + 2) u + 2^-126``.

Every test prints its maximum of error / bound (``-s``).
"""
import functools

import numpy as np
import pytest
import torch

import voltrix
from voltrix import capi
from voltrix.attn_aggregate import attn_aggregate, attn_aggregate_grad_feat, attn_aggregate_grad_scores

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
TINY = 2.0 ** -126
CHUNK = 128           # kSddmmChunkEdges: consecutive edges per lane group of d_s
HUB_COL = 7
GUARD = 64            # floats on either side of a guarded output
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
# (H, D, dtype): one head; eight narrow heads; wide heads; fp32 rows; a head above 64 pieces in d_s; two slabs; padding
SHAPES = [(1, 8, "fp16"), (8, 8, "fp16"), (4, 64, "fp16"), (3, 20, "fp32"), (2, 520, "fp16"), (16, 64, "bf16"), (3, 13, "fp16")]
IDS = [f"H{h}-D{d}-{t}" for h, d, t in SHAPES]
SCALES = [1.0, None, -1.5, 0.0]      # None: D ** -0.5


def special_lengths():
    """Rows of 0, 1, 3, 4, 5, 127, 128 and 129 edges at several offsets, a run of 200 empty rows between two rows of one chunk, a hub row
    of 1,000 edges, short random rows: about 3,000 rows and 12,000 edges (tests/test_gpu_gatv2.py's pattern)."""
    rng = np.random.default_rng(7)
    lengths = [127, 1, 128, 129, 0, 1]
    for r in range(2800):
        if r % 11 == 0:
            lengths.append(0)
        elif r in (300, 1700):
            lengths += [127, 128, 129, 0, 1]
        elif r == 900:
            lengths.append(1000)
        elif r == 1200:
            lengths += [3] + [0] * 200 + [3]
        else:
            lengths.append(int(rng.integers(1, 7)))
    return np.asarray(lengths, np.int64)


def special_pattern():
    """(lengths, cols, num_cols) of the square test pattern, on the host."""
    lengths = special_lengths()
    n, nnz = len(lengths), int(lengths.sum())
    rng = np.random.default_rng(17)
    cols = rng.integers(0, n, nnz)
    cols[rng.choice(nnz, 600, replace=False)] = HUB_COL
    ip = np.concatenate([[0], np.cumsum(lengths)])
    run = int(np.flatnonzero(lengths == 1000)[0])
    empties = next(i for i in range(n - 200) if not lengths[i:i + 200].any() and lengths[i - 1] == 3)
    assert 2900 <= n <= 3100 and 11000 <= nnz <= 13000 and nnz % CHUNK != 0, (n, nnz)
    assert ip[run + 1] // CHUNK - ip[run] // CHUNK >= 7                                   # the hub row spans 8 chunks or more
    assert (ip[empties] - 1) // CHUNK == ip[empties] // CHUNK and lengths[empties + 200] == 3   # the empty run lies inside one chunk
    assert np.bincount(cols, minlength=n)[HUB_COL] >= 600
    assert all((lengths == k).any() for k in (0, 1, 3, 4, 5, 127, 128, 129))
    return lengths, cols, n


class _Graph:
    """A CSR pattern [num_rows, num_cols] on the device, with its transpose by a stable sort by column and int64 ids for the oracle."""

    def __init__(self, lengths, cols, num_cols):
        lengths, cols = np.asarray(lengths, np.int64), np.asarray(cols, np.int64)
        self.num_rows, self.num_cols, self.nnz = len(lengths), num_cols, int(lengths.sum())
        assert cols.size == self.nnz
        ip = np.concatenate([[0], np.cumsum(lengths)])
        rows = np.repeat(np.arange(self.num_rows), lengths)
        order = np.argsort(cols, kind="stable")
        col_deg = np.bincount(cols, minlength=num_cols)
        t_ip = np.concatenate([[0], np.cumsum(col_deg)])
        self.ip, self.rows_np, self.cols_np, self.lengths = ip, rows, cols, lengths
        dev = lambda x, t=torch.int32: torch.from_numpy(np.ascontiguousarray(x)).to(t).cuda()     # noqa: E731
        self.indptr, self.indices = dev(ip), dev(cols)
        self.t_indptr, self.t_indices, self.t_order = dev(t_ip), dev(rows[order]), dev(order)
        self.rows, self.cols = dev(rows, torch.int64), dev(cols, torch.int64)
        self.row_deg, self.col_deg = dev(lengths, torch.float64), dev(col_deg, torch.float64)


@functools.lru_cache(maxsize=None)
def _special():
    return _Graph(*special_pattern())


@functools.lru_cache(maxsize=None)
def _rect():
    rng = np.random.default_rng(3)
    lengths = rng.integers(0, 12, 37)
    lengths[[4, 20]] = 0
    cols = rng.integers(0, 4, int(lengths.sum()))       # column 4 of the 5 is never used; duplicates are certain
    return _Graph(lengths, cols, 5)


@functools.lru_cache(maxsize=None)
def _empty():
    return _Graph([0] * 9, [], 4)


GRAPHS = {"special": _special, "rect": _rect, "empty": _empty}


def _row_of_length(graph, length, which=0):
    return int(np.flatnonzero(graph.lengths == length)[which])


@functools.lru_cache(maxsize=None)
def _inputs(graph_name, heads, dim, dtype, seed=0):
    """(scores [nnz, H] fp32, feat [num_cols, H, D] in ``dtype``, dC [num_rows, H, D] fp32) on the device; heads = None: the 2-D form.
    Scores are normal with standard deviation 2; one row has a spread of about 60, a few entries are -inf and one row is all -inf in a
    single head.  Shared between the tests and never written."""
    graph = GRAPHS[graph_name]()
    gen = torch.Generator(device="cuda").manual_seed(1000 * seed + 7 * dim + (heads or 0))
    h = heads or 1
    s = 2.0 * torch.randn((graph.nnz, h), device="cuda", generator=gen)
    if graph.nnz:
        wide = _row_of_length(graph, 129) if graph_name == "special" else int(np.argmax(graph.lengths))
        b, e = int(graph.ip[wide]), int(graph.ip[wide + 1])
        s[b:e] = torch.linspace(-30.0, 30.0, e - b, device="cuda")[:, None] + 0.25 * s[b:e]
        pick = torch.randint(0, graph.nnz, (12,), device="cuda", generator=gen)
        s[pick, torch.randint(0, h, (12,), device="cuda", generator=gen)] = float("-inf")
        masked = _row_of_length(graph, 5) if graph_name == "special" else int(np.flatnonzero(graph.lengths > 1)[0])
        s[int(graph.ip[masked]):int(graph.ip[masked + 1]), h - 1] = float("-inf")
    feat = torch.randn((graph.num_cols, h, dim), device="cuda", generator=gen).to(DT[dtype])
    grad = torch.randn((graph.num_rows, h, dim), device="cuda", generator=gen)
    if heads is None:
        return s.view(-1), feat.view(graph.num_cols, dim), grad.view(graph.num_rows, dim)
    return s, feat, grad


def _scale(scale, dim):
    return dim ** -0.5 if scale is None else scale


def _oracle(graph, s, feat, grad, scale):
    """float64 on the device, a dict of (value, bound) pairs in the 3-D layout: out, l, d_s, d_feat; and m, alpha, chain (the unfused
    chain's bound on out)."""
    sc = float(np.float32(scale))
    sign, a = (-1.0 if sc < 0 else 1.0), abs(sc)
    if feat.dim() == 2:
        s, feat, grad = s.unsqueeze(1), feat.unsqueeze(1), grad.unsqueeze(1)
    n, m_cols, (heads, dim) = graph.num_rows, graph.num_cols, feat.shape[1:]
    rows, cols = graph.rows, graph.cols
    key = sign * s.double()
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")     # noqa: E731
    m = torch.full((n, heads), float("-inf"), dtype=torch.float64, device="cuda")
    if graph.nnz:
        m = m.scatter_reduce(0, rows[:, None].expand(-1, heads), key, "amax", include_self=True)
    masked = key == float("-inf")
    x = torch.where(masked, 0.0, a * (m[rows] - torch.where(masked, 0.0, key)))       # |z - m| >= 0; 0 where the weight is 0
    x = torch.where(masked, torch.zeros_like(x), x)
    w = torch.where(masked, torch.zeros_like(x), torch.exp(-x))
    big_l = zeros(n, heads).index_add_(0, rows, w)
    inv = torch.where(big_l > 0, 1.0 / big_l, torch.zeros_like(big_l))
    alpha = w * inv[rows]
    deg = graph.row_deg[:, None]
    wx = zeros(n, heads).index_add_(0, rows, w * x)
    l_bound = (deg + 2) * U * big_l + 2 * U * wx + deg * TINY
    f = feat.double()[cols]                                                            # [nnz, H, D]
    out = zeros(n, heads, dim).index_add_(0, rows, alpha[:, :, None] * f)
    mass = zeros(n, heads, dim).index_add_(0, rows, alpha[:, :, None] * f.abs())
    plain = zeros(n, heads, dim).index_add_(0, rows, f.abs())
    out_bound = 2 * (deg[:, :, None] + 3) * U * mass + U * plain * inv[:, :, None] + TINY
    # the unfused chain: spmm_heads' bound with the edge softmax's bound on every alpha
    alpha_bound = 2 * alpha * (deg[rows] + x + 2) * U + TINY
    chain = deg[:, :, None] * U * mass + zeros(n, heads, dim).index_add_(0, rows, alpha_bound[:, :, None] * f.abs()) + TINY
    # backward
    eta = (2 * x + 2) * U + (l_bound * inv)[rows] + 2 * U                             # relative error of the recomputed alpha
    g = grad.double()
    dot = (g[rows] * f).sum(-1)
    dot_bound = (dim + 2) * U * (g[rows].abs() * f.abs()).sum(-1)
    delta = (g * out).sum(-1)
    delta_bound = (dim + 2) * U * (g.abs() * (out.abs() + out_bound)).sum(-1) + (g.abs() * out_bound).sum(-1)
    diff = dot - delta[rows]
    d_s = sc * alpha * diff
    d_s_bound = abs(sc) * alpha * (dot_bound + delta_bound[rows] + diff.abs() * (eta + 2 * U)) + TINY * (1 + abs(sc) * diff.abs())
    term = alpha[:, :, None] * g[rows]
    d_feat = zeros(m_cols, heads, dim).index_add_(0, cols, term)
    d_feat_bound = (graph.col_deg[:, None, None] * U * zeros(m_cols, heads, dim).index_add_(0, cols, term.abs())
                    + zeros(m_cols, heads, dim).index_add_(0, cols, (eta[:, :, None] * term.abs()))
                    + TINY * (1 + zeros(m_cols, heads, dim).index_add_(0, cols, g[rows].abs())))
    return {"out": (out, out_bound), "l": (big_l, l_bound), "d_s": (d_s, d_s_bound), "d_feat": (d_feat, d_feat_bound), "m": m,
            "alpha": alpha, "chain": chain}


def _all(graph, s, feat, grad, scale, delta=None):
    """(out, m, l, d_s, d_feat) through the functional API; delta is the dense torch product of dC and the computed out."""
    out, m, l = attn_aggregate(graph.indptr, graph.indices, s, feat, graph.num_rows, scale, return_stats=True)
    if delta is None:
        delta = (grad * out).sum(-1)
    d_s = attn_aggregate_grad_scores(graph.indptr, graph.indices, grad, feat, s, m, l, delta, scale)
    d_feat = attn_aggregate_grad_feat(graph.t_indptr, graph.t_indices, graph.t_order, grad, s, m, l, graph.num_cols, scale)
    return out, m, l, d_s, d_feat


@functools.lru_cache(maxsize=None)
def _case(graph_name, heads, dim, dtype, scale=1.0):
    """Inputs, the oracle and the five results of one (pattern, shape, scale): computed once, shared, never written."""
    graph = GRAPHS[graph_name]()
    s, feat, grad = _inputs(graph_name, heads, dim, dtype)
    if scale < 0:      # z = scale * s: with a negative scale it is +inf that masks an entry (-inf would make the row NaN, as in the chain)
        s = torch.where(torch.isinf(s), -s, s)
    return graph, (s, feat, grad), _oracle(graph, s, feat, grad, scale), _all(graph, s, feat, grad, scale)


def _within(out, ref, bound, what):
    assert out.dtype == torch.float32, (what, out.dtype)
    out = out.reshape(ref.shape)
    err = (out.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0      # (a bound of 0: an exact result, e.g. l of an empty row)
    print(f"{what}: max err / bound = {ratio:.3f}")
    assert bool((err <= bound).all()), (what, ratio)


def _same_bits(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def _check_all(ref, got, what):
    out, m, l, d_s, d_feat = got
    _within(out, *ref["out"], f"out {what}")
    assert torch.equal(m.double().reshape(ref["m"].shape), ref["m"]), f"m {what}"      # a maximum is exact
    _within(l, *ref["l"], f"l {what}")
    _within(d_s, *ref["d_s"], f"d_s {what}")
    _within(d_feat, *ref["d_feat"], f"d_feat {what}")


@pytest.mark.parametrize("graph_name", ["special", "rect"])
@pytest.mark.parametrize("heads,dim,dtype", SHAPES, ids=IDS)
def test_all_outputs_within_their_bounds(cuda_device, graph_name, heads, dim, dtype):
    graph, _, ref, got = _case(graph_name, heads, dim, dtype)
    out, m, l, d_s, d_feat = got
    assert out.shape == (graph.num_rows, heads, dim) and m.shape == l.shape == (graph.num_rows, heads)
    assert d_s.shape == (graph.nnz, heads) and d_feat.shape == (graph.num_cols, heads, dim)
    _check_all(ref, got, f"{graph_name} H={heads} D={dim} {dtype}")
    # rows without entries: +0, m = -inf, l = 0; the row whose last head is all -inf: zeros there, l = 0, zero gradients
    empty_rows = graph.row_deg == 0
    assert bool(empty_rows.any()) and _same_bits(out[empty_rows], torch.zeros_like(out[empty_rows]))
    assert bool((m[empty_rows] == float("-inf")).all()) and _same_bits(l[empty_rows], torch.zeros_like(l[empty_rows]))
    dead = (ref["l"][0] == 0) & ~empty_rows[:, None]
    assert bool(dead.any()) and bool((out[dead] == 0).all()) and bool((l[dead] == 0).all())
    assert bool((d_s[dead[graph.rows]] == 0).all()) and not bool(torch.isnan(d_s).any() | torch.isnan(d_feat).any())
    assert _same_bits(d_feat[graph.col_deg == 0], torch.zeros_like(d_feat[graph.col_deg == 0]))


@pytest.mark.parametrize("scale", SCALES, ids=lambda v: f"scale={v}")
@pytest.mark.parametrize("heads,dim,dtype", [(8, 8, "fp16"), (3, 20, "fp32")], ids=lambda v: str(v))
def test_scales(cuda_device, scale, heads, dim, dtype):
    scale = _scale(scale, dim)
    graph, (s, feat, grad), ref, got = _case("special", heads, dim, dtype, scale)
    _check_all(ref, got, f"scale={scale:.4g} H={heads} D={dim}")
    if scale == 0.0:      # the mean over the entries that are not -inf
        count = torch.zeros(graph.num_rows, heads, dtype=torch.float64, device="cuda").index_add_(0, graph.rows, (~torch.isinf(s)).double())
        assert torch.equal(got[2].double(), count)


def test_a_scale_that_is_not_finite_raises(cuda_device):
    graph = _special()
    s, feat, grad = _inputs("special", 8, 8, "fp16")
    for bad in (float("inf"), float("-inf"), float("nan")):
        with pytest.raises(ValueError):
            attn_aggregate(graph.indptr, graph.indices, s, feat, graph.num_rows, bad)
        out = torch.empty(graph.num_rows, 8, 8, device="cuda")
        stats = torch.empty(graph.num_rows, 8, device="cuda")
        with pytest.raises(capi.VoltrixError):
            capi.launch_attn_aggregate_csr(graph.indptr, graph.indices, s, graph.num_rows, feat, bad, out, stats, stats.clone(),
                                           torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("graph_name", ["special", "rect"])
@pytest.mark.parametrize("dim,dtype", [(8, "fp16"), (20, "fp32"), (13, "bf16"), (520, "fp16")])
def test_two_dimensional_form(cuda_device, graph_name, dim, dtype):
    graph, (s, feat, grad), ref, got = _case(graph_name, None, dim, dtype)
    out, m, l, d_s, d_feat = got
    assert out.shape == (graph.num_rows, dim) and m.shape == l.shape == (graph.num_rows,)
    assert d_s.shape == (graph.nnz,) and d_feat.shape == (graph.num_cols, dim)
    _check_all(ref, got, f"2-D {graph_name} D={dim} {dtype}")
    # the 2-D form is the one-head layout: the same kernels, the same bits
    three = _all(graph, s.unsqueeze(1), feat.unsqueeze(1), grad.unsqueeze(1), 1.0)
    assert all(_same_bits(x.squeeze(1), y) for x, y in zip(three, got))


@pytest.mark.parametrize("scale", [1.0, -1.5], ids=lambda v: f"scale={v}")
@pytest.mark.parametrize("heads,dim,dtype", SHAPES, ids=IDS)
def test_cross_check_against_the_unfused_chain(cuda_device, heads, dim, dtype, scale):
    graph, (s, feat, grad), ref, got = _case("special", heads, dim, dtype, scale)
    unfused = voltrix.spmm_heads(graph.indptr, graph.indices, voltrix.edge_softmax(graph.indptr, s, scale), feat, graph.num_rows)
    err = (got[0].double() - unfused.double()).abs()
    bound = ref["out"][1] + ref["chain"]
    ratio = float((err / bound).max())
    print(f"fused vs unfused H={heads} D={dim} {dtype} scale={scale}: max err / (sum of bounds) = {ratio:.3f}")
    assert bool((err <= bound).all()), ratio
    zero_rows = (unfused == 0).all(-1)
    assert torch.equal((got[0] == 0).all(-1), zero_rows)                               # the all-zero (row, head)s are identical


@pytest.mark.parametrize("heads,dim,dtype", [(8, 8, "fp16"), (3, 20, "fp32"), (2, 520, "fp16")], ids=lambda v: str(v))
def test_special_values_stay_in_their_row_and_head(cuda_device, heads, dim, dtype):
    graph, (s, feat, grad), _, (out, m, l, d_s, d_feat) = _case("special", heads, dim, dtype)
    hub = _row_of_length(graph, 1000)
    for value in (float("nan"), float("inf")):
        for e, h in ((int(graph.ip[hub]) + 500, heads - 1), (0, 0), (graph.nnz - 1, heads // 2)):
            bad = s.clone()
            bad[e, h] = value
            r = int(graph.rows_np[e])
            b_out, b_m, b_l, b_ds, b_df = _all(graph, bad, feat, grad, 1.0)
            want_out = torch.zeros_like(out, dtype=torch.bool)
            want_out[r, h, :] = True
            assert torch.equal(torch.isnan(b_out), want_out) and _same_bits(b_out[~want_out], out[~want_out]), (value, e, h)
            want_ds = torch.zeros_like(d_s, dtype=torch.bool)
            want_ds[int(graph.ip[r]):int(graph.ip[r + 1]), h] = True
            assert torch.equal(torch.isnan(b_ds), want_ds) and _same_bits(b_ds[~want_ds], d_s[~want_ds]), (value, e, h)
            want_df = torch.zeros_like(d_feat, dtype=torch.bool)
            want_df[torch.from_numpy(graph.cols_np[int(graph.ip[r]):int(graph.ip[r + 1])]).cuda(), h, :] = True
            assert torch.equal(torch.isnan(b_df), want_df) and _same_bits(b_df[~want_df], d_feat[~want_df]), (value, e, h)
            # the unfused chain puts its NaNs in the same places
            unfused = voltrix.spmm_heads(graph.indptr, graph.indices, voltrix.edge_softmax(graph.indptr, bad, 1.0), feat, graph.num_rows)
            assert torch.equal(torch.isnan(unfused), want_out), (value, e, h)


@pytest.mark.parametrize("heads,dim,dtype", SHAPES[1:], ids=IDS[1:])
def test_every_head_has_the_bits_of_the_single_head_call(cuda_device, heads, dim, dtype):
    graph, (s, feat, grad), _, got = _case("special", heads, dim, dtype)
    delta = (grad * got[0]).sum(-1)      # delta is an input of d_s: the slice of the H-head product (torch's reduction is not under test)
    for h in range(heads):
        one = _all(graph, s[:, h].contiguous(), feat[:, h].contiguous(), grad[:, h].contiguous(), 1.0, delta[:, h].contiguous())
        for name, x, y in zip(("out", "m", "l", "d_s", "d_feat"), one, got):
            assert _same_bits(x, y[:, h].contiguous()), (name, h)
    again = _all(graph, s, feat, grad, 1.0)                                            # two calls: the same bits
    assert all(_same_bits(x, y) for x, y in zip(again, got))


def test_no_edges_no_width_and_casts(cuda_device):
    graph = _empty()
    s, feat, grad = _inputs("empty", 3, 8, "fp16")
    out, m, l, d_s, d_feat = _all(graph, s, feat, grad, 1.0)
    assert _same_bits(out, torch.zeros(9, 3, 8, device="cuda")) and _same_bits(l, torch.zeros(9, 3, device="cuda"))
    assert bool((m == float("-inf")).all()) and d_s.shape == (0, 3) and _same_bits(d_feat, torch.zeros(4, 3, 8, device="cuda"))
    # D == 0: [n, H, 0], the row statistics as ever, zero d_s
    graph, (s, feat, grad), _, (_, m8, l8, _, _) = _case("rect", 2, 8, "fp16")
    out, m, l, d_s, d_feat = _all(graph, s, feat[:, :, :0], grad[:, :, :0], 1.0)
    assert out.shape == (37, 2, 0) and d_feat.shape == (5, 2, 0) and _same_bits(m, m8) and _same_bits(l, l8)
    assert _same_bits(d_s, torch.zeros(graph.nnz, 2, device="cuda"))
    # other types are cast: scores to fp32, feat to fp32 (every conversion here is exact, so the fp32 call is the reference)
    want = _all(graph, s, feat.float(), grad, 1.0)
    got = _all(graph, s.double(), feat.double(), grad, 1.0)
    assert all(_same_bits(x, y) for x, y in zip(got, want))
    # d_feat takes a 16-bit gradient as it is
    half = attn_aggregate_grad_feat(graph.t_indptr, graph.t_indices, graph.t_order, grad.half(), s, m8, l8, graph.num_cols, 1.0)
    full = attn_aggregate_grad_feat(graph.t_indptr, graph.t_indices, graph.t_order, grad.half().float(), s, m8, l8, graph.num_cols, 1.0)
    assert _same_bits(half, full)


def _guarded(shape, k):
    """A float32 output of ``shape`` that starts ``k`` floats past a 16-byte boundary, between two runs of GUARD guard words."""
    count = int(np.prod(shape))
    buf = torch.full((GUARD + k + count + GUARD,), float("nan"), device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD + k:GUARD + k + count].view(shape)


def _guards_intact(buf, out, k):
    count = out.numel()
    return bool(torch.isnan(buf[:GUARD + k]).all()) and bool(torch.isnan(buf[GUARD + k + count:]).all())


@pytest.mark.parametrize("heads,dim,dtype", SHAPES[:6], ids=IDS[:6])
def test_guarded_outputs_prefilled_with_nan_are_fully_written_and_nothing_else(cuda_device, heads, dim, dtype):
    """The launches themselves, on outputs full of NaN between guard words (these shapes need no padding, so the tensors go in as they
    are): out and d_feat on the 16-byte grid (k = 0, 4), m, l and d_s at any 4-byte offset (k = 1, 2, 3)."""
    graph, (s, feat, grad), _, (out, m, l, d_s, d_feat) = _case("special", heads, dim, dtype)
    stream = torch.cuda.current_stream().cuda_stream
    delta = (grad * out).sum(-1)
    for k16, k4 in ((0, 1), (4, 2), (4, 3)):
        b_out, g_out = _guarded(out.shape, k16)
        b_m, g_m = _guarded(m.shape, k4)
        b_l, g_l = _guarded(l.shape, k4)
        capi.launch_attn_aggregate_csr(graph.indptr, graph.indices, s, graph.num_rows, feat, 1.0, g_out, g_m, g_l, stream)
        assert _same_bits(g_out, out) and _same_bits(g_m, m) and _same_bits(g_l, l)
        assert _guards_intact(b_out, g_out, k16) and _guards_intact(b_m, g_m, k4) and _guards_intact(b_l, g_l, k4)
        b_ds, g_ds = _guarded(d_s.shape, k4)
        capi.launch_attn_aggregate_grad_scores_csr(graph.indptr, graph.indices, graph.num_rows, grad, feat, s, m, l, delta, 1.0, g_ds,
                                                   stream)
        assert _same_bits(g_ds, d_s) and _guards_intact(b_ds, g_ds, k4)
        b_df, g_df = _guarded(d_feat.shape, k16)
        capi.launch_attn_aggregate_grad_feat_csr(graph.t_indptr, graph.t_indices, graph.t_order, graph.num_cols, grad, s, m, l, 1.0, g_df,
                                                 stream)
        assert _same_bits(g_df, d_feat) and _guards_intact(b_df, g_df, k16)
    # off the 16-byte grid: refused on the host, nothing written
    b_out, g_out = _guarded(out.shape, 1)
    with pytest.raises(capi.VoltrixError):
        capi.launch_attn_aggregate_csr(graph.indptr, graph.indices, s, graph.num_rows, feat, 1.0, g_out, m.clone(), l.clone(), stream)
    assert bool(torch.isnan(b_out).all())


@pytest.mark.parametrize("heads,dim,dtype", [(8, 8, "fp16"), (3, 20, "fp32"), (3, 13, "fp16")], ids=lambda v: str(v))
def test_offset_and_strided_views_and_no_copy_of_a_conforming_operand(cuda_device, heads, dim, dtype, monkeypatch):
    graph, (s, feat, grad), _, got = _case("special", heads, dim, dtype)

    def offset(t, k=1):        # a contiguous view that starts k elements into its storage: off the 16-byte grid
        flat = torch.empty(t.numel() + k, dtype=t.dtype, device="cuda")
        flat[k:].copy_(t.reshape(-1))
        return flat[k:].view(t.shape)

    def strided(t):            # every second element along the last axis of a buffer twice as wide
        wide = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype, device="cuda")
        wide[..., ::2] = t
        return wide[..., ::2]

    for view in (offset, strided):
        sv, fv, gv = view(s), view(feat), view(grad)
        assert not (fv.is_contiguous() and fv.data_ptr() % 16 == 0)
        assert all(_same_bits(x, y) for x, y in zip(_all(graph, sv, fv, gv, 1.0), got)), view.__name__
    # a conforming operand reaches the launchers with the caller's pointer
    seen = {}
    names = ("launch_attn_aggregate_csr", "launch_attn_aggregate_grad_scores_csr", "launch_attn_aggregate_grad_feat_csr")
    for name in names:
        def wrapper(*args, _fn=getattr(capi, name), _name=name):
            seen[_name] = {t.data_ptr() for t in args if isinstance(t, torch.Tensor)}
            return _fn(*args)
        monkeypatch.setattr(capi, name, wrapper)
    if dim % (4 if dtype == "fp32" else 8) == 0:
        out, m, l = attn_aggregate(graph.indptr, graph.indices, s, feat, graph.num_rows, 1.0, return_stats=True)
        delta = (grad * out).sum(-1)
        attn_aggregate_grad_scores(graph.indptr, graph.indices, grad, feat, s, m, l, delta, 1.0)
        attn_aggregate_grad_feat(graph.t_indptr, graph.t_indices, graph.t_order, grad, s, m, l, graph.num_cols, 1.0)
        assert {s.data_ptr(), feat.data_ptr(), graph.indptr.data_ptr(), graph.indices.data_ptr()} <= seen[names[0]]
        assert {s.data_ptr(), feat.data_ptr(), grad.data_ptr(), m.data_ptr(), l.data_ptr(), delta.data_ptr()} <= seen[names[1]]
        assert {s.data_ptr(), grad.data_ptr(), m.data_ptr(), l.data_ptr(), graph.t_order.data_ptr()} <= seen[names[2]]
    else:                      # a padded operand is a copy on the 16-byte grid
        attn_aggregate(graph.indptr, graph.indices, s, feat, graph.num_rows, 1.0)
        assert feat.data_ptr() not in seen[names[0]] and s.data_ptr() in seen[names[0]]


def test_streams_sync_debug_mode_and_graph_capture(cuda_device):
    graph, (s, feat, grad), _, first = _case("special", 4, 64, "fp16")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = _all(graph, s, feat, grad, 1.0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(_same_bits(x, y) for x, y in zip(first, second))
    torch.cuda.set_sync_debug_mode("error")                  # nothing is read back on the host
    try:
        third = _all(graph, s, feat, grad, 1.0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(_same_bits(x, y) for x, y in zip(first, third))
    cuda_graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cuda_graph):
        captured = _all(graph, s, feat, grad, 1.0)
    cuda_graph.replay()
    torch.cuda.synchronize()
    assert all(_same_bits(x, y) for x, y in zip(first, captured))
    for t in captured:
        t.fill_(float("nan"))
    cuda_graph.replay()                                      # the second replay writes everything again
    torch.cuda.synchronize()
    assert all(_same_bits(x, y) for x, y in zip(first, captured))


@pytest.mark.parametrize("heads,dim", [(3, 20), (None, 8), (2, 260)], ids=lambda v: str(v))
def test_autograd_attn_aggregate(cuda_device, heads, dim):
    from voltrix.autograd import AttnAggregate

    graph = _special()
    scale = dim ** -0.5
    op = AttnAggregate(graph.indptr, graph.indices, graph.num_rows, graph.num_cols)
    assert op.t_order.dtype == torch.int32
    assert torch.equal(op.t_indptr, graph.t_indptr) and torch.equal(op.t_indices, graph.t_indices)
    s0, feat0, w = _inputs("special", heads, dim, "fp32", seed=3)
    feat, s = feat0.clone().requires_grad_(True), s0.clone().requires_grad_(True)
    out = op(feat, s, scale)
    assert _same_bits(out.detach(), attn_aggregate(graph.indptr, graph.indices, s0, feat0, graph.num_rows, scale))
    (out * w).sum().backward()
    # the float64 torch composite (rows that are all -inf: zeros, as the operator)
    sc = float(np.float32(scale))
    f64, s64 = feat0.double().requires_grad_(True), s0.double().requires_grad_(True)
    h = heads or 1
    z = (sc * s64).view(graph.nnz, h)
    top = torch.full((graph.num_rows, h), float("-inf"), dtype=torch.float64, device="cuda").scatter_reduce(
        0, graph.rows[:, None].expand(-1, h), z.detach(), "amax", include_self=True)
    top = torch.where(torch.isinf(top), torch.zeros_like(top), top)
    e = torch.exp(z - top[graph.rows])
    total = torch.zeros(graph.num_rows, h, dtype=torch.float64, device="cuda").index_add(0, graph.rows, e)
    alpha = e / total.clamp_min(1e-300)[graph.rows]
    out64 = torch.zeros(graph.num_rows, h, dim, dtype=torch.float64, device="cuda").index_add(
        0, graph.rows, alpha[:, :, None] * f64.view(graph.num_cols, h, dim)[graph.cols])
    (out64 * w.double().view(graph.num_rows, h, dim)).sum().backward()
    ref = _oracle(graph, s0, feat0, w, scale)
    _within(out.detach(), *ref["out"], f"autograd out H={heads} D={dim}")
    _within(s.grad, s64.grad.view(ref["d_s"][0].shape), ref["d_s"][1], f"autograd d_s H={heads} D={dim}")
    _within(feat.grad, f64.grad.view(ref["d_feat"][0].shape), ref["d_feat"][1], f"autograd d_feat H={heads} D={dim}")
    # the analytic oracle and float64 autograd agree far below the bounds
    assert bool(((s64.grad.view(ref["d_s"][0].shape) - ref["d_s"][0]).abs() <= 1e-3 * ref["d_s"][1] + 1e-300).all())
    # a second backward: the same bits; a side without a gradient returns None and leaves the other unchanged
    for keep in ((True, True), (True, False), (False, True)):
        some = [t.clone().requires_grad_(k) for t, k in zip((feat0, s0), keep)]
        (op(*some, scale) * w).sum().backward()
        for t, k, full in zip(some, keep, (feat, s)):
            assert (t.grad is None) if not k else _same_bits(t.grad, full.grad), keep


def test_autograd_dtypes_and_a_shared_transpose(cuda_device):
    from voltrix.autograd import AttnAggregate, SpMMHeads

    graph = _special()
    s0, feat0, w = _inputs("special", 4, 16, "fp16", seed=4)
    agg = SpMMHeads(graph.indptr, graph.indices, graph.num_rows, graph.num_cols)
    op = AttnAggregate(graph.indptr, graph.indices, graph.num_rows, graph.num_cols, transposed=(agg.t_indptr, agg.t_indices, agg.t_order))
    assert op.t_indptr is agg.t_indptr and op.t_order.dtype == torch.int32
    feat, s = feat0.clone().requires_grad_(True), s0.double().requires_grad_(True)
    (op(feat, s, 0.25) * w).sum().backward()
    assert (feat.grad.dtype, s.grad.dtype) == (torch.float16, torch.float64)
    out, m, l, d_s, d_feat = _all(graph, s0, feat0, w, 0.25)
    assert torch.equal(feat.grad, d_feat.half()) and torch.equal(s.grad, d_s.double())


def _dense_attention(graph, scores64, values64):
    """softmax over every row of the pattern (a duplicate entry counts as often as it occurs; rows without entries: zeros) times values:
    scores64 [n, m, H] dense, values64 [m, H, D] -> [n, H, D], float64."""
    n, m = graph.num_rows, graph.num_cols
    count = torch.zeros(n, m, dtype=torch.float64, device="cuda").index_put_(
        (graph.rows, graph.cols), torch.ones(graph.nnz, dtype=torch.float64, device="cuda"), accumulate=True)
    top = torch.where(count[:, :, None] > 0, scores64, torch.full_like(scores64, float("-inf"))).max(dim=1, keepdim=True).values
    top = torch.where(torch.isinf(top), torch.zeros_like(top), top)
    weight = count[:, :, None] * torch.exp(scores64 - top)
    attn = weight / weight.sum(dim=1, keepdim=True).clamp_min(1e-300)
    return torch.einsum("ijh,jhd->ihd", attn, values64)


@functools.lru_cache(maxsize=None)
def _small():
    """About 200 nodes, 1,300 edges: rows of 0 .. 14 entries, duplicates possible."""
    rng = np.random.default_rng(5)
    lengths = rng.integers(0, 15, 200)
    lengths[[3, 77]] = 0
    return _Graph(lengths, rng.integers(0, 200, int(lengths.sum())), 200)


@pytest.mark.parametrize("kind", ["sddmm", "gat"])
def test_layers_end_to_end_against_a_dense_float64_layer(cuda_device, kind):
    """SDDMM -> AttnAggregate with scale = D^-0.5 (H = 2, D = 8) and GATScore -> AttnAggregate with two heads, all fp32, on a graph of
    200 nodes, against a dense float64 attention layer.  Tolerances as tests/test_gpu_gatv2.py's layer test: the fp32 pipeline is a
    handful of sums of at most 14 terms and well-conditioned maps (softmax of O(1) scores, cross entropy), so its relative error is
    some tens of 2^-24; 1e-4 of the loss and 1e-3 of every gradient's norm leave two orders for the cancellation in the gradients."""
    from voltrix.autograd import SDDMM, AttnAggregate, GATScore

    graph = _small()
    n, in_feats, heads, d = graph.num_rows, 6, 2, 8
    score = (SDDMM if kind == "sddmm" else GATScore)(graph.indptr, graph.indices, n)
    fused = AttnAggregate(graph.indptr, graph.indices, n, transposed=(score.t_indptr, score.t_indices, score.t_order))
    torch.manual_seed(13)
    x = torch.randn(n, in_feats, device="cuda")
    y = torch.randint(0, d, (n,), device="cuda")
    names = ("wq", "wk", "wv") if kind == "sddmm" else ("wv", "al", "ar")
    shapes = {"wq": (in_feats, heads * d), "wk": (in_feats, heads * d), "wv": (in_feats, heads * d), "al": (heads, d), "ar": (heads, d)}
    params = {k: torch.randn(shapes[k], device="cuda") / shapes[k][0] ** 0.5 for k in names}

    def layer(p, x, double):
        v = (x @ p["wv"]).view(n, heads, d)
        if kind == "sddmm":
            q, k = (x @ p["wq"]).view(n, heads, d), (x @ p["wk"]).view(n, heads, d)
            if double:
                return _dense_attention(graph, float(np.float32(d ** -0.5)) * torch.einsum("ihd,jhd->ijh", q, k), v)
            return fused(v, score(q, k), d ** -0.5)
        el, er = (v * p["al"]).sum(-1), (v * p["ar"]).sum(-1)
        if double:
            return _dense_attention(graph, torch.nn.functional.leaky_relu(el[:, None] + er[None, :], float(np.float32(0.2))), v)
        return fused(v, score(el, er, 0.2))

    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    loss = torch.nn.functional.cross_entropy(layer(p, x, False).mean(1), y)
    loss.backward()
    r = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    ref_loss = torch.nn.functional.cross_entropy(layer(r, x.double(), True).mean(1), y)
    ref_loss.backward()
    print(f"{kind} layer: loss {float(loss):.7f} vs {float(ref_loss):.7f}")
    assert abs(float(loss) - float(ref_loss)) <= 1e-4 * abs(float(ref_loss))
    for name in params:
        err = float((p[name].grad.double() - r[name].grad).norm() / r[name].grad.norm())
        print(f"{kind} layer: d_{name} relative error {err:.2e}")
        assert err <= 1e-3, (name, err)
