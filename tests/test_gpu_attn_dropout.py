"""GPU: attention dropout -- the keep mask's generator against the numpy restatement of Philox4x32-10, and
voltrix.attn_aggregate / its two gradients / autograd.AttnAggregate with a mask against float64 torch and against the unfused chain
``spmm_heads(apply_dropout_mask(edge_softmax(s, scale), mask, keep_scale), feat)``.

Patterns, inputs and helpers are those of tests/test_gpu_attn_aggregate.py (imported, not edited).  The oracle is that file's with the
factor ``k[e, h] = float32 keep_scale`` where the mask keeps and 0 elsewhere, in float64 from the inputs as stored, ``float32(scale)``
and the exact mask: ``out = sum alpha k feat``, ``delta = <dC, out>``, ``d_s = scale alpha (k dot - delta)``, ``d_feat = sum alpha k dC``.

Bounds (``u = 2^-23``, ``deg`` the row's -- for d_feat the column's -- FULL degree, because ``l`` sums every entry):
3.17's three bounds with ``|feat_e| -> k_e |feat_e|``, ``|dC_e| -> k_e |dC_e|``, ``dot -> k_e dot`` and one more ``u`` per weight for the
rounding of ``w k`` (``alpha k``, ``k dot``):

* ``m`` exact, ``l`` as in 3.17 (the mask does not touch them);
* ``|out - ref| <= (2 (deg + 3) + 1) u sum_e alpha_e k_e |feat_e| + u sum_e k_e |feat_e| / L + 2^-126``;
* ``d_s``: ``|scale| alpha (k bound(dot) + u k |dot| + bound(delta) + |k dot - delta| (eta + 2 u)) + 2^-126 (1 + |scale| |k dot - delta|)``,
  ``bound(delta)`` from the dropped ``out`` and its bound;
* ``d_feat``: ``deg_c u sum_e alpha_e k_e |dC_e| + sum_e alpha_e (eta_e + u) k_e |dC_e| + 2^-126 (1 + sum_e k_e |dC_e|)``;
* the unfused chain: ``deg u sum_e alpha_e k_e |feat_e| + sum_e (bound(alpha_e) + u alpha_e) k_e |feat_e| + 2^-126``.

Every bound test prints its maximum of error / bound (``-s``)."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_attn_aggregate as base
import voltrix
from test_attn_dropout_host import keep_bits, pack, threshold_of
from voltrix import capi
from voltrix.attn_aggregate import attn_aggregate, attn_aggregate_grad_feat, attn_aggregate_grad_scores
from voltrix.dropout import unpack_mask

pytestmark = pytest.mark.gpu

U, TINY = base.U, base.TINY
# (H, D, dtype): 3.15's shapes with (33, 8, bf16) -- two mask words -- in the place of (16, 64, bf16)
SHAPES = [(1, 8, "fp16"), (8, 8, "fp16"), (4, 64, "fp16"), (3, 20, "fp32"), (2, 520, "fp16"), (33, 8, "bf16"), (3, 13, "fp16")]
IDS = [f"H{h}-D{d}-{t}" for h, d, t in SHAPES]
MASKS = ("p0.6", "ones", "zeros", "hand")
SEED, OFFSET = 2 ** 63 + 12345, 2 ** 33 + 7
KS = float(np.float32(1.0) / np.float32(1.0 - 0.6))          # keep_scale of p = 0.6, a float32


def _to_mask(keep):
    """bool [nnz, H] (numpy) -> the packed int32 mask on the device."""
    return torch.from_numpy(pack(np.asarray(keep, bool)).view(np.int32)).cuda()


@functools.lru_cache(maxsize=None)
def _mask(graph_name, heads, dim, dtype, kind, negative=False):
    """(mask int32 [nnz, W] on the device, keep bool [nnz, H] on the device, keep_scale) of one case; shared, never written.
    ``negative``: the case runs with a scale below 0, where the row maximum of ``sign(scale) * s`` is the minimum of ``s``."""
    graph = base.GRAPHS[graph_name]()
    h = heads or 1
    if kind == "p0.6":
        mask = voltrix.dropout_mask(graph.nnz, h, 0.6, SEED, OFFSET)
        ks = KS
    elif kind == "ones":
        mask, ks = _to_mask(np.ones((graph.nnz, h), bool)), 1.0
    elif kind == "zeros":
        mask, ks = _to_mask(np.zeros((graph.nnz, h), bool)), KS
    else:      # every row's maximum entry dropped in every head, and one head of one row emptied
        s = base._inputs(graph_name, heads, dim, dtype)[0].view(graph.nnz, h).cpu().numpy()
        if negative:      # what _case does to the scores, then the sign: the key the kernel takes its maximum of
            s = -np.where(np.isinf(s), -s, s)
        keep = keep_bits(graph.nnz, h, threshold_of(0.3), 99, 0)
        for r in np.flatnonzero(graph.lengths > 0):
            b, e = int(graph.ip[r]), int(graph.ip[r + 1])
            keep[b + np.argmax(s[b:e], axis=0), np.arange(h)] = False
        if graph.nnz:
            r = int(np.argmax(graph.lengths))
            keep[int(graph.ip[r]):int(graph.ip[r + 1]), 0] = False
        mask, ks = _to_mask(keep), 1.75
    return mask, unpack_mask(mask, h), ks


def _oracle(graph, s, feat, grad, scale, keep, ks):
    """tests/test_gpu_attn_aggregate.py's oracle with k = ks where keep, 0 elsewhere: (value, bound) pairs in the 3-D layout."""
    sc = float(np.float32(scale))
    sign, a = (-1.0 if sc < 0 else 1.0), abs(sc)
    if feat.dim() == 2:
        s, feat, grad = s.unsqueeze(1), feat.unsqueeze(1), grad.unsqueeze(1)
    n, m_cols, (heads, dim) = graph.num_rows, graph.num_cols, feat.shape[1:]
    rows, cols = graph.rows, graph.cols
    k = keep.double() * float(np.float32(ks))
    key = sign * s.double()
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")     # noqa: E731
    m = torch.full((n, heads), float("-inf"), dtype=torch.float64, device="cuda")
    if graph.nnz:
        m = m.scatter_reduce(0, rows[:, None].expand(-1, heads), key, "amax", include_self=True)
    masked = key == float("-inf")
    x = torch.where(masked, 0.0, a * (m[rows] - torch.where(masked, 0.0, key)))
    x = torch.where(masked, torch.zeros_like(x), x)
    w = torch.where(masked, torch.zeros_like(x), torch.exp(-x))
    big_l = zeros(n, heads).index_add_(0, rows, w)
    inv = torch.where(big_l > 0, 1.0 / big_l, torch.zeros_like(big_l))
    alpha = w * inv[rows]
    deg = graph.row_deg[:, None]
    wx = zeros(n, heads).index_add_(0, rows, w * x)
    l_bound = (deg + 2) * U * big_l + 2 * U * wx + deg * TINY
    f = feat.double()[cols]
    f = torch.where(keep[:, :, None], f, torch.zeros_like(f))                          # a dropped entry's feat is never read
    ak = (alpha * k)[:, :, None]
    out = zeros(n, heads, dim).index_add_(0, rows, ak * f)
    mass = zeros(n, heads, dim).index_add_(0, rows, ak * f.abs())
    plain = zeros(n, heads, dim).index_add_(0, rows, k[:, :, None] * f.abs())
    out_bound = (2 * (deg[:, :, None] + 3) + 1) * U * mass + U * plain * inv[:, :, None] + TINY
    alpha_bound = 2 * alpha * (deg[rows] + x + 2) * U + TINY
    chain = (deg[:, :, None] * U * mass
             + zeros(n, heads, dim).index_add_(0, rows, ((alpha_bound + U * alpha) * k)[:, :, None] * f.abs()) + TINY)
    eta = (2 * x + 2) * U + (l_bound * inv)[rows] + 2 * U
    g = grad.double()
    dot = (g[rows] * f).sum(-1)
    dot_bound = (dim + 2) * U * (g[rows].abs() * f.abs()).sum(-1)
    delta = (g * out).sum(-1)
    delta_bound = (dim + 2) * U * (g.abs() * (out.abs() + out_bound)).sum(-1) + (g.abs() * out_bound).sum(-1)
    diff = k * dot - delta[rows]
    d_s = sc * alpha * diff
    d_s_bound = (abs(sc) * alpha * (k * dot_bound + U * k * dot.abs() + delta_bound[rows] + diff.abs() * (eta + 2 * U))
                 + TINY * (1 + abs(sc) * diff.abs()))
    term = ak * g[rows]
    d_feat = zeros(m_cols, heads, dim).index_add_(0, cols, term)
    d_feat_bound = (graph.col_deg[:, None, None] * U * zeros(m_cols, heads, dim).index_add_(0, cols, term.abs())
                    + zeros(m_cols, heads, dim).index_add_(0, cols, ((eta + U)[:, :, None] * term.abs()))
                    + TINY * (1 + zeros(m_cols, heads, dim).index_add_(0, cols, k[:, :, None] * g[rows].abs())))
    return {"out": (out, out_bound), "l": (big_l, l_bound), "d_s": (d_s, d_s_bound), "d_feat": (d_feat, d_feat_bound), "m": m,
            "alpha": alpha, "chain": chain}


def _all(graph, s, feat, grad, scale, mask, ks, delta=None):
    out, m, l = attn_aggregate(graph.indptr, graph.indices, s, feat, graph.num_rows, scale, return_stats=True, mask=mask, keep_scale=ks)
    if delta is None:
        delta = (grad * out).sum(-1)
    d_s = attn_aggregate_grad_scores(graph.indptr, graph.indices, grad, feat, s, m, l, delta, scale, mask=mask, keep_scale=ks)
    d_feat = attn_aggregate_grad_feat(graph.t_indptr, graph.t_indices, graph.t_order, grad, s, m, l, graph.num_cols, scale, mask=mask,
                                      keep_scale=ks)
    return out, m, l, d_s, d_feat


@functools.lru_cache(maxsize=None)
def _case(graph_name, heads, dim, dtype, kind, scale=1.0):
    graph = base.GRAPHS[graph_name]()
    s, feat, grad = base._inputs(graph_name, heads, dim, dtype)
    if scale < 0:
        s = torch.where(torch.isinf(s), -s, s)
    mask, keep, ks = _mask(graph_name, heads, dim, dtype, kind, scale < 0)
    return graph, (s, feat, grad), (mask, keep, ks), _oracle(graph, s, feat, grad, scale, keep, ks), _all(graph, s, feat, grad, scale, mask, ks)


_same_bits, _within, _check_all = base._same_bits, base._within, base._check_all


# ---------------------------------------------------------------------------------------------------------------- the generator
@pytest.mark.parametrize("heads", [1, 3, 4, 8, 33])
def test_generator_equals_the_restatement(cuda_device, heads):
    for p in (0.0, 0.1, 0.6, 0.999):
        mask = voltrix.dropout_mask(1000, heads, p, SEED, OFFSET)
        assert mask.dtype == torch.int32 and mask.shape == (1000, (heads + 31) // 32) and mask.is_cuda
        want = pack(keep_bits(1000, heads, threshold_of(p), SEED, OFFSET))
        assert np.array_equal(mask.cpu().numpy().view(np.uint32), want), (heads, p)
        valid = np.zeros(mask.shape[1], np.uint32)
        for h in range(heads):
            valid[h >> 5] |= np.uint32(1) << np.uint32(h & 31)
        assert not (mask.cpu().numpy().view(np.uint32) & ~valid).any()                     # bits past H are zero
        if p == 0.0:
            assert np.array_equal(mask.cpu().numpy().view(np.uint32), np.broadcast_to(valid, mask.shape))   # all ones


def test_generator_is_a_function_of_seed_offset_edge_and_head(cuda_device):
    first = voltrix.dropout_mask(1000, 8, 0.6, SEED, OFFSET)
    assert torch.equal(first, voltrix.dropout_mask(1000, 8, 0.6, SEED, OFFSET))              # two runs: the same bytes
    assert not torch.equal(first, voltrix.dropout_mask(1000, 8, 0.6, SEED + 1, OFFSET))
    assert not torch.equal(first, voltrix.dropout_mask(1000, 8, 0.6, SEED, OFFSET + 1))
    assert not torch.equal(first, voltrix.dropout_mask(1000, 8, 0.6, SEED, OFFSET + 2 ** 32))   # the high word of the offset counts
    assert not torch.equal(first, voltrix.dropout_mask(1000, 8, 0.6, SEED - 2 ** 63, OFFSET))   # and the seed's
    assert torch.equal(first[:300], voltrix.dropout_mask(300, 8, 0.6, SEED, OFFSET))         # not of nnz
    assert torch.equal(first & 7, voltrix.dropout_mask(1000, 3, 0.6, SEED, OFFSET))          # not of H
    assert voltrix.dropout_mask(0, 8, 0.6, 1).shape == (0, 1)
    stream = torch.cuda.current_stream().cuda_stream
    # guarded output: every word written, nothing else
    for words, heads in ((1, 8), (2, 33)):
        buf = torch.full((64 + 1000 * words + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        out = buf[64:64 + 1000 * words].view(1000, words)
        capi.launch_dropout_mask(1000, heads, threshold_of(0.6), SEED, OFFSET, out, stream)
        assert torch.equal(out, voltrix.dropout_mask(1000, heads, 0.6, SEED, OFFSET))
        assert bool((buf[:64] == 0x5A5A5A5A).all()) and bool((buf[64 + 1000 * words:] == 0x5A5A5A5A).all())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = voltrix.dropout_mask(1000, 8, 0.6, SEED, OFFSET)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(first, second)
    torch.cuda.set_sync_debug_mode("error")                  # nothing is read back on the host
    try:
        third = voltrix.dropout_mask(1000, 8, 0.6, SEED, OFFSET)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(first, third)
    cuda_graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cuda_graph):
        captured = voltrix.dropout_mask(1000, 8, 0.6, SEED, OFFSET)
    cuda_graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, captured)


def test_python_layer_raises_value_errors(cuda_device):
    graph = base._special()
    s, feat, grad = base._inputs("special", 8, 8, "fp16")
    good = voltrix.dropout_mask(graph.nnz, 8, 0.6, 1)
    for p in (-0.5, 1.0, 2.0, float("nan")):
        with pytest.raises(ValueError):
            voltrix.dropout_mask(graph.nnz, 8, p, 1)
    for bad in (good.long(), good.float(), good[:-1], torch.cat([good, good], 1), good.cpu()):
        with pytest.raises(ValueError):
            attn_aggregate(graph.indptr, graph.indices, s, feat, graph.num_rows, 1.0, mask=bad, keep_scale=2.5)
    for ks in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            attn_aggregate(graph.indptr, graph.indices, s, feat, graph.num_rows, 1.0, mask=good, keep_scale=ks)
    out = torch.empty(graph.num_rows, 8, 8, device="cuda")
    stats = torch.empty(graph.num_rows, 8, device="cuda")
    with pytest.raises(capi.VoltrixError):
        capi.launch_attn_aggregate_csr(graph.indptr, graph.indices, s, graph.num_rows, feat, 1.0, out, stats, stats.clone(),
                                       torch.cuda.current_stream().cuda_stream, good, float("nan"))


# ---------------------------------------------------------------------------------------------------------------- bounds
@pytest.mark.parametrize("graph_name", ["special", "rect"])
@pytest.mark.parametrize("heads,dim,dtype", SHAPES, ids=IDS)
def test_all_outputs_within_their_bounds(cuda_device, graph_name, heads, dim, dtype):
    plain = base._case(graph_name, heads, dim, dtype)[3] if (heads, dim, dtype) in base.SHAPES else None
    for kind in MASKS:
        graph, (s, feat, grad), (mask, keep, ks), ref, got = _case(graph_name, heads, dim, dtype, kind)
        out, m, l, d_s, d_feat = got
        assert out.shape == (graph.num_rows, heads, dim) and m.shape == l.shape == (graph.num_rows, heads)
        assert d_s.shape == (graph.nnz, heads) and d_feat.shape == (graph.num_cols, heads, dim)
        _check_all(ref, got, f"{graph_name} H={heads} D={dim} {dtype} mask={kind}")
        assert not bool(torch.isnan(out).any() | torch.isnan(d_s).any() | torch.isnan(d_feat).any())
        # a row and head whose kept set is empty: zeros
        kept = torch.zeros(graph.num_rows, heads, device="cuda").index_add_(0, graph.rows, keep.float())
        assert bool((out[kept == 0] == 0).all())
        if kind == "hand":
            assert bool(((kept == 0) & (graph.row_deg[:, None] > 0)).any())
        if plain is not None:      # m and l are those of the call without a mask
            assert _same_bits(m, plain[1]) and _same_bits(l, plain[2]), kind
            if kind == "ones":     # every bit set, keep_scale = 1: the bits of the operator without a mask
                assert all(_same_bits(x, y) for x, y in zip(got, plain)), kind
        if kind == "zeros":
            assert _same_bits(out, torch.zeros_like(out)) and _same_bits(d_feat, torch.zeros_like(d_feat))


def test_statistics_and_all_ones_for_the_two_word_mask(cuda_device):
    """(33, 8, bf16) is not among the shapes of tests/test_gpu_attn_aggregate.py: its plain call is made here."""
    graph, (s, feat, grad), (mask, keep, ks), _, got = _case("special", 33, 8, "bf16", "ones")
    plain = base._all(graph, s, feat, grad, 1.0)
    assert mask.shape[1] == 2 and all(_same_bits(x, y) for x, y in zip(got, plain))
    dropped = _case("special", 33, 8, "bf16", "p0.6")[4]
    assert _same_bits(dropped[1], plain[1]) and _same_bits(dropped[2], plain[2])


@pytest.mark.parametrize("scale", base.SCALES, ids=lambda v: f"scale={v}")
@pytest.mark.parametrize("heads,dim,dtype", [(8, 8, "fp16"), (3, 20, "fp32")], ids=lambda v: str(v))
def test_scales(cuda_device, scale, heads, dim, dtype):
    scale = base._scale(scale, dim)
    for kind in ("p0.6", "hand"):
        _, _, _, ref, got = _case("special", heads, dim, dtype, kind, scale)
        _check_all(ref, got, f"scale={scale:.4g} H={heads} D={dim} mask={kind}")


@pytest.mark.parametrize("graph_name", ["special", "rect"])
@pytest.mark.parametrize("dim,dtype", [(8, "fp16"), (20, "fp32"), (13, "bf16")])
def test_two_dimensional_form(cuda_device, graph_name, dim, dtype):
    for kind in ("p0.6", "hand"):
        graph, (s, feat, grad), (mask, keep, ks), ref, got = _case(graph_name, None, dim, dtype, kind)
        out, m, l, d_s, d_feat = got
        assert out.shape == (graph.num_rows, dim) and m.shape == l.shape == (graph.num_rows,)
        assert d_s.shape == (graph.nnz,) and d_feat.shape == (graph.num_cols, dim) and mask.shape == (graph.nnz, 1)
        _check_all(ref, got, f"2-D {graph_name} D={dim} {dtype} mask={kind}")
        three = _all(graph, s.unsqueeze(1), feat.unsqueeze(1), grad.unsqueeze(1), 1.0, mask, ks)
        assert all(_same_bits(x.squeeze(1), y) for x, y in zip(three, got))


def test_pattern_without_edges(cuda_device):
    graph = base._empty()
    s, feat, grad = base._inputs("empty", 3, 8, "fp16")
    mask = voltrix.dropout_mask(0, 3, 0.6, 1)
    out, m, l, d_s, d_feat = _all(graph, s, feat, grad, 1.0, mask, KS)
    assert _same_bits(out, torch.zeros(9, 3, 8, device="cuda")) and _same_bits(l, torch.zeros(9, 3, device="cuda"))
    assert bool((m == float("-inf")).all()) and d_s.shape == (0, 3) and _same_bits(d_feat, torch.zeros(4, 3, 8, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------- isolation
@pytest.mark.parametrize("heads,dim,dtype", [(8, 8, "fp16"), (3, 20, "fp32"), (2, 520, "fp16")], ids=lambda v: str(v))
def test_a_dropped_entrys_feat_is_never_read(cuda_device, heads, dim, dtype):
    """NaN and +inf in the feat rows that only dropped entries point at: out and d_s stay finite and within their bounds."""
    graph, (s, feat, grad), (_, keep0, ks), _, _ = _case("special", heads, dim, dtype, "p0.6")
    poisoned = torch.from_numpy(np.random.default_rng(5).choice(graph.num_cols, 40, replace=False)).cuda()
    poisoned = torch.cat([poisoned, torch.tensor([base.HUB_COL], device="cuda")])
    hit = torch.isin(graph.cols, poisoned)
    assert 600 < int(hit.sum()) < graph.nnz // 2
    keep = keep0 & ~hit[:, None]
    mask = _to_mask(keep.cpu().numpy())
    clean = feat.clone()
    clean[poisoned] = 0
    ref = _oracle(graph, s, clean, grad, 1.0, keep, ks)
    for value in (float("nan"), float("inf")):
        bad = feat.clone()
        bad[poisoned] = value
        out, m, l, d_s, d_feat = _all(graph, s, bad, grad, 1.0, mask, ks)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(d_s).all())
        _check_all(ref, (out, m, l, d_s, d_feat), f"feat = {value} under dropped entries H={heads} D={dim}")
    # d_feat: a dropped entry's dC is not read either (the rows of dC whose every entry is dropped)
    dead_rows = torch.from_numpy(np.flatnonzero((graph.lengths > 0) & (graph.lengths < 4))[:50]).cuda()
    keep = keep0 & ~torch.isin(graph.rows, dead_rows)[:, None]
    mask = _to_mask(keep.cpu().numpy())
    out, m, l = attn_aggregate(graph.indptr, graph.indices, s, feat, graph.num_rows, 1.0, return_stats=True, mask=mask, keep_scale=ks)
    bad = grad.clone()
    bad[dead_rows] = float("nan")
    got = attn_aggregate_grad_feat(graph.t_indptr, graph.t_indices, graph.t_order, bad, s, m, l, graph.num_cols, 1.0, mask=mask, keep_scale=ks)
    want = attn_aggregate_grad_feat(graph.t_indptr, graph.t_indices, graph.t_order, grad, s, m, l, graph.num_cols, 1.0, mask=mask, keep_scale=ks)
    assert _same_bits(got, want)


def test_a_nan_score_stays_in_its_row_and_head(cuda_device):
    heads, dim, dtype = 8, 8, "fp16"
    graph, (s, feat, grad), (mask, keep, ks), _, (out, m, l, d_s, d_feat) = _case("special", heads, dim, dtype, "p0.6")
    hub = base._row_of_length(graph, 1000)
    for value in (float("nan"), float("inf")):
        for e, h in ((int(graph.ip[hub]) + 500, heads - 1), (0, 0), (graph.nnz - 1, heads // 2)):
            bad = s.clone()
            bad[e, h] = value
            r = int(graph.rows_np[e])
            b_out, b_m, b_l, b_ds, b_df = _all(graph, bad, feat, grad, 1.0, mask, ks)
            want_out = torch.zeros_like(out, dtype=torch.bool)
            want_out[r, h, :] = True
            assert torch.equal(torch.isnan(b_out), want_out) and _same_bits(b_out[~want_out], out[~want_out]), (value, e, h)
            want_ds = torch.zeros_like(d_s, dtype=torch.bool)
            want_ds[int(graph.ip[r]):int(graph.ip[r + 1]), h] = True
            assert torch.equal(torch.isnan(b_ds), want_ds) and _same_bits(b_ds[~want_ds], d_s[~want_ds]), (value, e, h)
            # d_feat: NaN where a KEPT entry of that row and head points (a dropped entry adds nothing), untouched elsewhere
            span = slice(int(graph.ip[r]), int(graph.ip[r + 1]))
            want_df = torch.zeros_like(d_feat, dtype=torch.bool)
            want_df[graph.cols[span][keep[span, h]], h, :] = True
            assert torch.equal(torch.isnan(b_df), want_df) and _same_bits(b_df[~want_df], d_feat[~want_df]), (value, e, h)


# ---------------------------------------------------------------------------------------------------------------- cross-check, bits
@pytest.mark.parametrize("scale", [1.0, -1.5], ids=lambda v: f"scale={v}")
@pytest.mark.parametrize("heads,dim,dtype", SHAPES, ids=IDS)
def test_cross_check_against_the_unfused_chain(cuda_device, heads, dim, dtype, scale):
    for kind in ("p0.6", "hand"):
        graph, (s, feat, grad), (mask, keep, ks), ref, got = _case("special", heads, dim, dtype, kind, scale)
        alpha = voltrix.apply_dropout_mask(voltrix.edge_softmax(graph.indptr, s, scale), mask, ks)
        unfused = voltrix.spmm_heads(graph.indptr, graph.indices, alpha, feat, graph.num_rows)
        err = (got[0].double() - unfused.double()).abs()
        bound = ref["out"][1] + ref["chain"]
        ratio = float((err / bound).max())
        print(f"fused vs unfused H={heads} D={dim} {dtype} scale={scale} mask={kind}: max err / (sum of bounds) = {ratio:.3f}")
        assert bool((err <= bound).all()), ratio


@pytest.mark.parametrize("heads,dim,dtype", SHAPES[1:], ids=IDS[1:])
def test_every_head_has_the_bits_of_the_single_head_call(cuda_device, heads, dim, dtype):
    graph, (s, feat, grad), (mask, keep, ks), _, got = _case("special", heads, dim, dtype, "p0.6")
    delta = (grad * got[0]).sum(-1)
    keep_np = keep.cpu().numpy()
    for h in range(heads):
        plane = _to_mask(keep_np[:, h:h + 1])                                              # that head's bit-plane: [nnz, 1]
        one = _all(graph, s[:, h].contiguous(), feat[:, h].contiguous(), grad[:, h].contiguous(), 1.0, plane, ks, delta[:, h].contiguous())
        for name, x, y in zip(("out", "m", "l", "d_s", "d_feat"), one, got):
            assert _same_bits(x, y[:, h].contiguous()), (name, h)
    again = _all(graph, s, feat, grad, 1.0, mask, ks)                                      # two calls: the same bits
    assert all(_same_bits(x, y) for x, y in zip(again, got))


# ---------------------------------------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("heads,dim,dtype", [(8, 8, "fp16"), (33, 8, "bf16"), (3, 13, "fp16")], ids=lambda v: str(v))
def test_offset_and_strided_views_of_every_operand(cuda_device, heads, dim, dtype):
    graph, (s, feat, grad), (mask, keep, ks), _, got = _case("special", heads, dim, dtype, "p0.6")

    def offset(t, k=1):
        flat = torch.empty(t.numel() + k, dtype=t.dtype, device="cuda")
        flat[k:].copy_(t.reshape(-1))
        return flat[k:].view(t.shape)

    def strided(t):
        wide = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype, device="cuda")
        wide[..., ::2] = t
        return wide[..., ::2]

    for view in (offset, strided):
        sv, fv, gv, mv = view(s), view(feat), view(grad), view(mask)
        assert not (fv.is_contiguous() and fv.data_ptr() % 16 == 0)
        assert all(_same_bits(x, y) for x, y in zip(_all(graph, sv, fv, gv, 1.0, mv, ks), got)), view.__name__


@pytest.mark.parametrize("heads,dim,dtype", SHAPES[:6], ids=IDS[:6])
def test_guarded_outputs_prefilled_with_nan_are_fully_written_and_nothing_else(cuda_device, heads, dim, dtype):
    graph, (s, feat, grad), (mask, keep, ks), _, (out, m, l, d_s, d_feat) = _case("special", heads, dim, dtype, "p0.6")
    stream = torch.cuda.current_stream().cuda_stream
    delta = (grad * out).sum(-1)
    for k16, k4 in ((0, 1), (4, 3)):
        b_out, g_out = base._guarded(out.shape, k16)
        b_m, g_m = base._guarded(m.shape, k4)
        b_l, g_l = base._guarded(l.shape, k4)
        capi.launch_attn_aggregate_csr(graph.indptr, graph.indices, s, graph.num_rows, feat, 1.0, g_out, g_m, g_l, stream, mask, ks)
        assert _same_bits(g_out, out) and _same_bits(g_m, m) and _same_bits(g_l, l)
        assert base._guards_intact(b_out, g_out, k16) and base._guards_intact(b_m, g_m, k4) and base._guards_intact(b_l, g_l, k4)
        b_ds, g_ds = base._guarded(d_s.shape, k4)
        capi.launch_attn_aggregate_grad_scores_csr(graph.indptr, graph.indices, graph.num_rows, grad, feat, s, m, l, delta, 1.0, g_ds,
                                                   stream, mask, ks)
        assert _same_bits(g_ds, d_s) and base._guards_intact(b_ds, g_ds, k4)
        b_df, g_df = base._guarded(d_feat.shape, k16)
        capi.launch_attn_aggregate_grad_feat_csr(graph.t_indptr, graph.t_indices, graph.t_order, graph.num_cols, grad, s, m, l, 1.0, g_df,
                                                 stream, mask, ks)
        assert _same_bits(g_df, d_feat) and base._guards_intact(b_df, g_df, k16)


def test_streams_sync_debug_mode_and_graph_capture(cuda_device):
    graph, (s, feat, grad), (mask, keep, ks), _, first = _case("special", 4, 64, "fp16", "p0.6")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = _all(graph, s, feat, grad, 1.0, mask, ks)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(_same_bits(x, y) for x, y in zip(first, second))
    torch.cuda.set_sync_debug_mode("error")
    try:
        third = _all(graph, s, feat, grad, 1.0, mask, ks)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(_same_bits(x, y) for x, y in zip(first, third))
    cuda_graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cuda_graph):
        captured = _all(graph, s, feat, grad, 1.0, mask, ks)       # an explicit mask=: nothing drawn during capture
    cuda_graph.replay()
    torch.cuda.synchronize()
    assert all(_same_bits(x, y) for x, y in zip(first, captured))
    for t in captured:
        t.fill_(float("nan"))
    cuda_graph.replay()
    torch.cuda.synchronize()
    assert all(_same_bits(x, y) for x, y in zip(first, captured))


# ---------------------------------------------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("heads,dim", [(3, 20), (None, 8), (33, 8)], ids=lambda v: str(v))
def test_autograd_with_dropout(cuda_device, heads, dim):
    from voltrix.autograd import AttnAggregate

    graph = base._special()
    scale, p, seed, offset = dim ** -0.5, 0.6, 4242, 3
    h = heads or 1
    op = AttnAggregate(graph.indptr, graph.indices, graph.num_rows, graph.num_cols)
    s0, feat0, w = base._inputs("special", heads, dim, "fp32", seed=3)
    feat, s = feat0.clone().requires_grad_(True), s0.clone().requires_grad_(True)
    out = op(feat, s, scale, dropout_p=p, seed=seed, offset=offset)
    keep_np = keep_bits(graph.nnz, h, threshold_of(p), seed, offset)
    keep = torch.from_numpy(keep_np).cuda()
    mask = _to_mask(keep_np)
    assert _same_bits(out.detach(), attn_aggregate(graph.indptr, graph.indices, s0, feat0, graph.num_rows, scale, mask=mask, keep_scale=KS))
    (out * w).sum().backward()
    # the float64 torch composite with the same mask and the float32 keep_scale
    sc = float(np.float32(scale))
    f64, s64 = feat0.double().requires_grad_(True), s0.double().requires_grad_(True)
    z = (sc * s64).view(graph.nnz, h)
    top = torch.full((graph.num_rows, h), float("-inf"), dtype=torch.float64, device="cuda").scatter_reduce(
        0, graph.rows[:, None].expand(-1, h), z.detach(), "amax", include_self=True)
    top = torch.where(torch.isinf(top), torch.zeros_like(top), top)
    e = torch.exp(z - top[graph.rows])
    total = torch.zeros(graph.num_rows, h, dtype=torch.float64, device="cuda").index_add(0, graph.rows, e)
    alpha = e / total.clamp_min(1e-300)[graph.rows] * (keep.double() * KS)
    out64 = torch.zeros(graph.num_rows, h, dim, dtype=torch.float64, device="cuda").index_add(
        0, graph.rows, alpha[:, :, None] * f64.view(graph.num_cols, h, dim)[graph.cols])
    (out64 * w.double().view(graph.num_rows, h, dim)).sum().backward()
    ref = _oracle(graph, s0, feat0, w, scale, keep, KS)
    _within(out.detach(), *ref["out"], f"autograd out H={heads} D={dim}")
    _within(s.grad, s64.grad.view(ref["d_s"][0].shape), ref["d_s"][1], f"autograd d_s H={heads} D={dim}")
    _within(feat.grad, f64.grad.view(ref["d_feat"][0].shape), ref["d_feat"][1], f"autograd d_feat H={heads} D={dim}")
    # the same seed: the same bits; an explicit mask: the same bits; another seed or offset: another result
    for kwargs in ({"dropout_p": p, "seed": seed, "offset": offset}, {"dropout_p": p, "mask": mask}):
        f2, s2 = feat0.clone().requires_grad_(True), s0.clone().requires_grad_(True)
        out2 = op(f2, s2, scale, **kwargs)
        (out2 * w).sum().backward()
        assert _same_bits(out2.detach(), out.detach()) and _same_bits(f2.grad, feat.grad) and _same_bits(s2.grad, s.grad), kwargs
    assert not torch.equal(op(feat0, s0, scale, dropout_p=p, seed=seed + 1, offset=offset), out.detach())
    assert not torch.equal(op(feat0, s0, scale, dropout_p=p, seed=seed, offset=offset + 1), out.detach())
    # a side without a gradient returns None and leaves the other unchanged
    for need in ((True, False), (False, True)):
        some = [t.clone().requires_grad_(k) for t, k in zip((feat0, s0), need)]
        (op(*some, scale, dropout_p=p, seed=seed, offset=offset) * w).sum().backward()
        for t, k, full in zip(some, need, (feat, s)):
            assert (t.grad is None) if not k else _same_bits(t.grad, full.grad), need


def test_autograd_without_dropout_is_the_plain_call_and_seeds_come_from_torch(cuda_device):
    from voltrix.autograd import AttnAggregate

    graph = base._special()
    op = AttnAggregate(graph.indptr, graph.indices, graph.num_rows, graph.num_cols)
    s0, feat0, w = base._inputs("special", 8, 8, "fp16", seed=4)
    plain = op(feat0, s0, 0.5)

    def allocated_by(**kwargs):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        feat, s = feat0.clone().requires_grad_(True), s0.clone().requires_grad_(True)
        out = op(feat, s, 0.5, **kwargs)                     # out and what the backward saved are alive here
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated() - before, out.detach()

    base_bytes, _ = allocated_by()
    for kwargs in ({"dropout_p": 0.6, "training": False}, {"dropout_p": 0.0}, {"dropout_p": 0.0, "seed": 5}):
        got_bytes, got = allocated_by(**kwargs)
        assert _same_bits(got, plain) and got_bytes == base_bytes, kwargs               # no mask allocated
    drop_bytes, dropped = allocated_by(dropout_p=0.6, seed=1)
    mask_bytes = 4 * graph.nnz * 1
    assert base_bytes + mask_bytes <= drop_bytes <= base_bytes + mask_bytes + 1024      # the mask (rounded up by the allocator), nothing else
    assert not torch.equal(dropped, plain)
    with pytest.raises(ValueError):
        op(feat0, s0, 0.5, dropout_p=1.0)
    # seed=None: drawn from torch's default CPU generator -- torch.manual_seed reproduces a run, and no device sync is needed
    torch.manual_seed(123)
    first = op(feat0, s0, 0.5, dropout_p=0.6)
    second = op(feat0, s0, 0.5, dropout_p=0.6)               # the generator has moved on
    torch.manual_seed(123)
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = op(feat0, s0, 0.5, dropout_p=0.6)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert _same_bits(first, again) and not torch.equal(first, second)
