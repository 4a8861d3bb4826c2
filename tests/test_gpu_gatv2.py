"""GPU: GATv2 edge scores (voltrix.gatv2_score, gatv2_score_kernels.hpp), the gated row sum of their backward and autograd.GATv2Score
against float64 torch.

Oracle, in float64 from the inputs as stored (fp32 / fp16 / bf16 values converted exactly) and ``float32(slope)``:
``z = xl[row] + xr[col]``, ``leaky(z) = z > 0 ? z : slope z``, ``s = sum_d a_d leaky(z_d)``; ``G[r] = sum_{e in r} gate(z_e) g_e`` by a
float64 ``index_add_`` (its own error, ~deg 2^-53, is nine orders below the bounds).  The patterns are small enough to materialise
[nnz, H, D] in float64.  Bounds (derived, not measured):

* forward ``|s - ref| <= (D + 2) 2^-23 sum_d |a_d| |leaky(z_d)| + 2^-149``: two roundings inside each term (the add, the product with
  slope), one per fused multiply-add and per butterfly level (at most D in all), with DESIGN.md 3.11's factor 2;
* row sum ``|G - ref| <= deg 2^-23 sum_e |term_e| + 2^-149``, ``deg`` the row's entries (the column's for ``G_r``);
* autograd, fp32 inputs so that no cast of a gradient enters: ``d_xl = a G_l`` is one more rounded product, which the factor 2 of the
  row-sum bound covers for every row with an entry (a row of ``deg`` entries has ``deg`` roundings, the bound counts ``2 deg``), so
  ``|d_x - ref| <= |a| bound(G)``; ``d_a = sum_r xl G_l + sum_c xr G_r`` propagates the row-sum bounds through the dense sums,
  ``sum_r |xl| bound(G_l) + sum_c |xr| bound(G_r)``, and adds ``n 2^-23 sum |x G|`` per side for the products and torch's fp32
  reduction over the ``n`` nodes.
"""
import functools

import numpy as np
import pytest
import torch

import voltrix
from voltrix.gatv2_score import gatv2_rowsum

pytestmark = pytest.mark.gpu

CHUNK = 128           # kSddmmChunkEdges: consecutive edges per lane group of the forward
HUB_COL = 7
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
# (H, D, dtype): one lane per head; 8 heads of one lane; 4 heads of 8 lanes; idle lanes in a head and a non-power-of-two group; 65 pieces
# per head (R = 0, a slab per head); 128 pieces (two slabs in both kernels); D padded to 16 bytes by the Python layer
SHAPES = [(1, 8, "fp16"), (8, 8, "fp16"), (4, 64, "fp16"), (3, 20, "fp32"), (2, 520, "fp16"), (16, 64, "bf16"), (3, 13, "fp16")]
IDS = [f"H{h}-D{d}-{t}" for h, d, t in SHAPES]


def special_lengths():
    """Rows of 0, 1, 127, 128 and 129 edges at several offsets, a run of 200 empty rows between two rows of one chunk, a hub row of 1,000
    edges, short random rows: about 3,000 rows and 12,000 edges."""
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
        self.ip, self.rows_np, self.cols_np = ip, rows, cols
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


@functools.lru_cache(maxsize=None)
def _inputs(graph_name, heads, dim, dtype, seed=0, integer=False):
    """(xl, xr, a, g) on the device: xl [num_rows, H, D], xr [num_cols, H, D] in ``dtype``, a [H, D] and g [nnz, H] float32; heads =
    None: the 2-D form.  Shared between the tests and never written."""
    graph = GRAPHS[graph_name]()
    gen = torch.Generator(device="cuda").manual_seed(1000 * seed + 7 * dim + (heads or 0))
    hd = (dim,) if heads is None else (heads, dim)
    gh = () if heads is None else (heads,)
    if integer:
        draw = lambda *s: torch.randint(-8, 9, s, device="cuda", generator=gen).float()     # noqa: E731
    else:
        draw = lambda *s: torch.randn(s, device="cuda", generator=gen)                       # noqa: E731
    return (draw(graph.num_rows, *hd).to(DT[dtype]), draw(graph.num_cols, *hd).to(DT[dtype]), draw(*hd), draw(graph.nnz, *gh))


def _oracle(graph, xl, xr, a, slope, g=None):
    """float64 on the device: (s, bound); with g also (G_l, bound), (G_r, bound).  Tensors come back in the inputs' layout."""
    sl = float(np.float32(slope))
    two_d = xl.dim() == 2
    if two_d:
        xl, xr, a = xl.unsqueeze(1), xr.unsqueeze(1), a.unsqueeze(0)
        g = None if g is None else g.unsqueeze(1)
    dim = xl.shape[2]
    z = xl.double()[graph.rows] + xr.double()[graph.cols]                  # [nnz, H, D]
    gate = torch.where(z > 0, 1.0, sl).double()
    lz = gate * z
    s = (a.double() * lz).sum(-1)
    s_bound = (dim + 2) * 2.0 ** -23 * (a.double().abs() * lz.abs()).sum(-1) + 2.0 ** -149
    squeeze = (lambda t: t.squeeze(1)) if two_d else (lambda t: t)
    if g is None:
        return squeeze(s), squeeze(s_bound)
    term = gate * g.double()[:, :, None]
    sides = []
    for ids, n, deg in ((graph.rows, graph.num_rows, graph.row_deg), (graph.cols, graph.num_cols, graph.col_deg)):
        total = torch.zeros((n,) + tuple(term.shape[1:]), dtype=torch.float64, device="cuda").index_add_(0, ids, term)
        mass = torch.zeros_like(total).index_add_(0, ids, term.abs())
        sides.append((squeeze(total), squeeze(deg[:, None, None] * 2.0 ** -23 * mass + 2.0 ** -149)))
    return (squeeze(s), squeeze(s_bound)), sides[0], sides[1]


@functools.lru_cache(maxsize=None)
def _case(graph_name, heads, dim, dtype, slope=0.2):
    """Inputs, the oracle and the three results of one (pattern, shape): computed once, shared, never written."""
    graph = GRAPHS[graph_name]()
    xl, xr, a, g = _inputs(graph_name, heads, dim, dtype)
    ref = _oracle(graph, xl, xr, a, slope, g)
    return graph, (xl, xr, a, g), ref, _all_three(graph, xl, xr, a, g, slope)


def _all_three(graph, xl, xr, a, g, slope):
    return (voltrix.gatv2_score(graph.indptr, graph.indices, xl, xr, a, slope),
            gatv2_rowsum(graph.indptr, graph.indices, xl, xr, g, slope),
            gatv2_rowsum(graph.t_indptr, graph.t_indices, xr, xl, g, slope, order=graph.t_order))


def _within(out, ref, bound, what):
    assert out.dtype == torch.float32 and out.shape == ref.shape, (what, out.dtype, tuple(out.shape), tuple(ref.shape))
    err = (out.double() - ref).abs()
    ratio = float((err / bound).max()) if err.numel() else 0.0
    print(f"{what}: max err / bound = {ratio:.3f}")
    assert bool((err <= bound).all()), (what, ratio)


def _same_bits(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


@pytest.mark.parametrize("graph_name", ["special", "rect"])
@pytest.mark.parametrize("heads,dim,dtype", SHAPES, ids=IDS)
def test_forward_within_the_bound(cuda_device, graph_name, heads, dim, dtype):
    graph, (xl, xr, a, g), ((s_ref, s_bound), _, _), (s, _, _) = _case(graph_name, heads, dim, dtype)
    assert s.shape == (graph.nnz, heads)
    _within(s, s_ref, s_bound, f"forward {graph_name} H={heads} D={dim} {dtype}")


@pytest.mark.parametrize("graph_name", ["special", "rect"])
@pytest.mark.parametrize("heads,dim,dtype", SHAPES, ids=IDS)
def test_row_sums_within_the_bound(cuda_device, graph_name, heads, dim, dtype):
    graph, _, (_, (l_ref, l_bound), (r_ref, r_bound)), (_, big_l, big_r) = _case(graph_name, heads, dim, dtype)
    assert big_l.shape == (graph.num_rows, heads, dim) and big_r.shape == (graph.num_cols, heads, dim)
    _within(big_l, l_ref, l_bound, f"G_l {graph_name} H={heads} D={dim} {dtype}")
    _within(big_r, r_ref, r_bound, f"G_r {graph_name} H={heads} D={dim} {dtype}")
    empty_rows = graph.row_deg == 0
    assert bool(empty_rows.any()) and _same_bits(big_l[empty_rows], torch.zeros_like(big_l[empty_rows]))     # +0, not -0
    assert _same_bits(big_r[graph.col_deg == 0], torch.zeros_like(big_r[graph.col_deg == 0]))


@pytest.mark.parametrize("slope", [0.25, 1.0, 0.0, -0.3])
def test_other_slopes(cuda_device, slope):
    graph = _special()
    xl, xr, a, g = _inputs("special", 4, 64, "fp16")
    (s_ref, s_bound), (l_ref, l_bound), (r_ref, r_bound) = _oracle(graph, xl, xr, a, slope, g)
    s, big_l, big_r = _all_three(graph, xl, xr, a, g, slope)
    _within(s, s_ref, s_bound, f"forward slope={slope}")
    _within(big_l, l_ref, l_bound, f"G_l slope={slope}")
    _within(big_r, r_ref, r_bound, f"G_r slope={slope}")


@pytest.mark.parametrize("graph_name", ["special", "rect"])
@pytest.mark.parametrize("dim,dtype", [(8, "fp16"), (20, "fp32"), (13, "bf16"), (520, "fp16")])
def test_two_dimensional_form(cuda_device, graph_name, dim, dtype):
    graph, (xl, xr, a, g), ((s_ref, s_bound), (l_ref, l_bound), (r_ref, r_bound)), (s, big_l, big_r) = _case(graph_name, None, dim, dtype)
    assert s.shape == (graph.nnz,) and big_l.shape == (graph.num_rows, dim) and big_r.shape == (graph.num_cols, dim)
    _within(s, s_ref, s_bound, f"forward 2-D {graph_name} D={dim} {dtype}")
    _within(big_l, l_ref, l_bound, f"G_l 2-D {graph_name} D={dim} {dtype}")
    _within(big_r, r_ref, r_bound, f"G_r 2-D {graph_name} D={dim} {dtype}")
    # the 2-D form is the one-head layout: the same kernel, the same bits
    s3, l3, r3 = _all_three(graph, xl.unsqueeze(1), xr.unsqueeze(1), a.unsqueeze(0), g.unsqueeze(1), 0.2)
    assert _same_bits(s3.squeeze(1), s) and _same_bits(l3.squeeze(1), big_l) and _same_bits(r3.squeeze(1), big_r)


def test_no_edges_no_columns_and_casts(cuda_device):
    graph = _empty()
    xl, xr, a, g = _inputs("empty", 3, 8, "fp16")
    s, big_l, big_r = _all_three(graph, xl, xr, a, g, 0.2)
    assert s.shape == (0, 3) and s.dtype == torch.float32
    assert _same_bits(big_l, torch.zeros(9, 3, 8, device="cuda")) and _same_bits(big_r, torch.zeros(4, 3, 8, device="cuda"))
    # D == 0: zeros [nnz, H]; row sums [n, H, 0]
    graph = _rect()
    xl, xr, a, g = _inputs("rect", 2, 8, "fp16")
    s = voltrix.gatv2_score(graph.indptr, graph.indices, xl[:, :, :0], xr[:, :, :0], a[:, :0])
    assert _same_bits(s, torch.zeros(graph.nnz, 2, device="cuda"))
    assert gatv2_rowsum(graph.indptr, graph.indices, xl[:, :, :0], xr[:, :, :0], g, 0.2).shape == (37, 2, 0)
    # a mixed or other-typed pair is cast to fp32; a is cast to fp32
    # (every conversion to fp32 is exact, so the fp32 call on the converted values is the reference; fp16 -> bf16 itself rounds)
    for pair in ((xl, xr.float()), (xl.bfloat16(), xr), (xl.double(), xr.double())):
        want = _all_three(graph, pair[0].float(), pair[1].float(), a, g, 0.2)
        got = _all_three(graph, pair[0], pair[1], a.double(), g.double(), 0.2)
        assert all(_same_bits(x, y) for x, y in zip(got, want)), (pair[0].dtype, pair[1].dtype)


@pytest.mark.parametrize("heads,dim,dtype", [(1, 8, "fp16"), (8, 8, "fp16"), (3, 20, "fp32"), (2, 520, "fp16"), (16, 64, "bf16")],
                         ids=lambda v: str(v))
def test_integer_inputs_are_exact(cuda_device, heads, dim, dtype):
    """Integers in [-8, 8] with slope 0.25: every z, product and partial sum is a multiple of 1/4 below 2^22, so the results are exact
    whatever the order."""
    for graph_name in ("special", "rect"):
        graph = GRAPHS[graph_name]()
        xl, xr, a, g = _inputs(graph_name, heads, dim, dtype, seed=1, integer=True)
        (s_ref, _), (l_ref, _), (r_ref, _) = _oracle(graph, xl, xr, a, 0.25, g)
        s, big_l, big_r = _all_three(graph, xl, xr, a, g, 0.25)
        assert torch.equal(s.double(), s_ref) and torch.equal(big_l.double(), l_ref) and torch.equal(big_r.double(), r_ref)
        assert float(s_ref.abs().max()) > 0 and float(l_ref.abs().max()) > 0


def test_z_equal_zero_takes_the_slope_branch(cuda_device):
    graph = _special()
    heads, dim = 4, 16
    _, _, a, g = _inputs("special", heads, dim, "fp16", seed=2, integer=True)
    v = torch.arange(1, heads * dim + 1, device="cuda").float().view(heads, dim) / 8          # exact in fp16
    xl = v.expand(graph.num_rows, heads, dim).half().contiguous()
    xr = (-v).expand(graph.num_cols, heads, dim).half().contiguous()                           # z == 0 on every edge
    s, big_l, big_r = _all_three(graph, xl, xr, a, g, 0.25)
    assert _same_bits(s, torch.zeros_like(s))                                                  # a * (0.25 * 0) summed: +0
    (_, _), (l_ref, _), (r_ref, _) = _oracle(graph, xl, xr, a, 0.25, g)                        # the oracle's gate: z > 0 ? 1 : slope
    plain = torch.zeros(graph.num_rows, heads, dtype=torch.float64, device="cuda").index_add_(0, graph.rows, g.double())
    assert torch.equal(l_ref, (0.25 * plain)[:, :, None].expand_as(l_ref)) and float(plain.abs().max()) > 0
    assert torch.equal(big_l.double(), l_ref) and torch.equal(big_r.double(), r_ref)           # slope * g, not g
    # one step above zero: the other branch
    xl2 = (xl.float() + 2.0 ** -7).half()
    s2, l2, _ = _all_three(graph, xl2, xr, a, g, 0.25)
    assert torch.equal(l2.double(), plain[:, :, None].expand_as(l_ref))
    assert torch.equal(s2.double(), (2.0 ** -7 * a.double().sum(-1))[None, :].expand_as(s2))


@pytest.mark.parametrize("heads,dim,dtype", [(8, 8, "fp16"), (4, 64, "fp16"), (3, 20, "fp32"), (2, 520, "fp16"), (16, 64, "bf16"),
                                             (3, 13, "fp16")], ids=lambda v: str(v))
def test_every_head_has_the_bits_of_the_single_head_call(cuda_device, heads, dim, dtype):
    graph, (xl, xr, a, g), _, (s, big_l, big_r) = _case("special", heads, dim, dtype)
    for h in range(heads):
        one = _all_three(graph, xl[:, h].contiguous(), xr[:, h].contiguous(), a[h].contiguous(), g[:, h].contiguous(), 0.2)
        assert _same_bits(one[0], s[:, h].contiguous()), h
        assert _same_bits(one[1], big_l[:, h].contiguous()) and _same_bits(one[2], big_r[:, h].contiguous()), h
    again = _all_three(graph, xl, xr, a, g, 0.2)                                               # two calls: the same bits
    assert all(_same_bits(x, y) for x, y in zip(again, (s, big_l, big_r)))


@pytest.mark.parametrize("heads,dim,dtype", SHAPES[:6], ids=IDS[:6])
def test_outputs_prefilled_with_nan_are_fully_written(cuda_device, heads, dim, dtype):
    """The launches themselves, on outputs full of NaN (these shapes need no padding, so the tensors go in as they are)."""
    from voltrix import capi

    graph, (xl, xr, a, g), _, (s, big_l, big_r) = _case("special", heads, dim, dtype)
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.full((graph.nnz, heads), float("nan"), device="cuda")
    capi.launch_gatv2_score_csr(graph.indptr, graph.indices, graph.num_rows, xl, xr, a, 0.2, out, stream)
    assert _same_bits(out, s) and not bool(torch.isnan(out).any())
    out_l = torch.full((graph.num_rows, heads, dim), float("nan"), device="cuda")
    capi.launch_gatv2_rowsum_csr(graph.indptr, graph.indices, None, graph.num_rows, xl, xr, g, 0.2, out_l, stream)
    out_r = torch.full((graph.num_cols, heads, dim), float("nan"), device="cuda")
    capi.launch_gatv2_rowsum_csr(graph.t_indptr, graph.t_indices, graph.t_order, graph.num_cols, xr, xl, g, 0.2, out_r, stream)
    assert _same_bits(out_l, big_l) and _same_bits(out_r, big_r) and not bool(torch.isnan(out_l).any() | torch.isnan(out_r).any())


@pytest.mark.parametrize("heads,dim,dtype", [(8, 8, "fp16"), (3, 20, "fp32"), (2, 520, "fp16")], ids=lambda v: str(v))
def test_special_values_stay_local(cuda_device, heads, dim, dtype):
    graph, (xl, xr, a, g), _, (s, big_l, big_r) = _case("special", heads, dim, dtype)
    hub = int(np.flatnonzero(np.diff(graph.ip) == 1000)[0])
    for r, h, d in ((hub, heads - 1, dim - 1), (0, 0, 0)):
        bad = xl.clone()
        bad[r, h, d] = float("nan")
        s_bad = voltrix.gatv2_score(graph.indptr, graph.indices, bad, xr, a, 0.2)
        want = torch.zeros_like(s, dtype=torch.bool)
        want[int(graph.ip[r]):int(graph.ip[r + 1]), h] = True
        assert torch.equal(torch.isnan(s_bad), want) and _same_bits(s_bad[~want], s[~want])
        # the gate tests only z > 0: a NaN in xl puts no NaN into any sum
        assert not bool(torch.isnan(gatv2_rowsum(graph.indptr, graph.indices, bad, xr, g, 0.2)).any())
    for e, h in ((int(graph.ip[hub]) + 500, heads - 1), (0, 0), (graph.nnz - 1, heads // 2)):
        bad = g.clone()
        bad[e, h] = float("nan")
        _, l_bad, r_bad = _all_three(graph, xl, xr, a, bad, 0.2)
        want_l, want_r = torch.zeros_like(big_l, dtype=torch.bool), torch.zeros_like(big_r, dtype=torch.bool)
        want_l[int(graph.rows_np[e]), h, :] = True
        want_r[int(graph.cols_np[e]), h, :] = True
        assert torch.equal(torch.isnan(l_bad), want_l) and _same_bits(l_bad[~want_l], big_l[~want_l])
        assert torch.equal(torch.isnan(r_bad), want_r) and _same_bits(r_bad[~want_r], big_r[~want_r])


def test_streams_and_graph_capture(cuda_device):
    graph, (xl, xr, a, g), _, first = _case("special", 4, 64, "fp16")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = _all_three(graph, xl, xr, a, g, 0.2)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(_same_bits(x, y) for x, y in zip(first, second))
    torch.cuda.set_sync_debug_mode("error")                  # nothing is read back on the host
    try:
        third = _all_three(graph, xl, xr, a, g, 0.2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(_same_bits(x, y) for x, y in zip(first, third))
    cuda_graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cuda_graph):
        captured = _all_three(graph, xl, xr, a, g, 0.2)
    cuda_graph.replay()
    torch.cuda.synchronize()
    assert all(_same_bits(x, y) for x, y in zip(first, captured))


@pytest.mark.parametrize("heads,dim", [(3, 20), (None, 8), (2, 260)], ids=lambda v: str(v))
def test_autograd_gatv2_score(cuda_device, heads, dim):
    from voltrix.autograd import GATv2Score

    graph = _special()
    slope = 0.2
    op = GATv2Score(graph.indptr, graph.indices, graph.num_rows, graph.num_cols)
    assert op.t_order.dtype == torch.int32
    assert torch.equal(op.t_indptr, graph.t_indptr) and torch.equal(op.t_indices, graph.t_indices)
    xl0, xr0, a0, w = _inputs("special", heads, dim, "fp32", seed=3)
    leaves = [t.clone().requires_grad_(True) for t in (xl0, xr0, a0)]
    s = op(*leaves, slope)
    assert _same_bits(s.detach(), voltrix.gatv2_score(graph.indptr, graph.indices, xl0, xr0, a0, slope))
    (s * w).sum().backward()
    xl, xr, a = leaves
    # the float64 torch composite
    xl64, xr64, a64 = (t.double().requires_grad_(True) for t in (xl0, xr0, a0))
    s64 = (a64 * torch.nn.functional.leaky_relu(xl64[graph.rows] + xr64[graph.cols], float(np.float32(slope)))).sum(-1)
    (s64 * w.double()).sum().backward()
    _, (l_ref, l_bound), (r_ref, r_bound) = _oracle(graph, xl0, xr0, a0, slope, w)
    a_abs = a0.double().abs()
    _within(xl.grad, xl64.grad, a_abs * l_bound, f"autograd d_xl H={heads} D={dim}")
    _within(xr.grad, xr64.grad, a_abs * r_bound, f"autograd d_xr H={heads} D={dim}")
    a_bound = ((xl0.double().abs() * l_bound).sum(0) + (xr0.double().abs() * r_bound).sum(0)
               + graph.num_rows * 2.0 ** -23 * (xl0.double() * l_ref).abs().sum(0)
               + graph.num_cols * 2.0 ** -23 * (xr0.double() * r_ref).abs().sum(0))
    _within(a.grad, a64.grad, a_bound, f"autograd d_a H={heads} D={dim}")
    # a second backward: the same bits
    again = [t.clone().requires_grad_(True) for t in (xl0, xr0, a0)]
    (op(*again, slope) * w).sum().backward()
    assert all(_same_bits(x.grad, y.grad) for x, y in zip(again, leaves))
    # a side without a gradient returns None and leaves the others unchanged
    for keep in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        some = [t.clone().requires_grad_(k) for t, k in zip((xl0, xr0, a0), keep)]
        (op(*some, slope) * w).sum().backward()
        for t, k, full in zip(some, keep, leaves):
            assert (t.grad is None) if not k else _same_bits(t.grad, full.grad), keep


def test_autograd_dtypes_shared_transpose_and_share_weights(cuda_device):
    from voltrix.autograd import GATv2Score, SpMMHeads

    graph = _special()
    xl0, xr0, a0, w = _inputs("special", 4, 16, "fp16", seed=4)
    agg = SpMMHeads(graph.indptr, graph.indices, graph.num_rows, graph.num_cols)
    op = GATv2Score(graph.indptr, graph.indices, graph.num_rows, graph.num_cols, transposed=(agg.t_indptr, agg.t_indices, agg.t_order))
    # gradients come back in the inputs' dtypes: the fp32 products a G, cast
    xl, xr, a = xl0.clone().requires_grad_(True), xr0.bfloat16().requires_grad_(True), a0.double().requires_grad_(True)
    (op(xl, xr, a) * w).sum().backward()
    assert (xl.grad.dtype, xr.grad.dtype, a.grad.dtype) == (torch.float16, torch.bfloat16, torch.float64)
    big_l = gatv2_rowsum(graph.indptr, graph.indices, xl0, xr0.bfloat16(), w, 0.2)
    assert torch.equal(xl.grad, (a0 * big_l).half())
    # share_weights: one tensor on both sides; its gradient is the sum of the two sides'
    x0 = xl0.float()
    x = x0.clone().requires_grad_(True)
    s = op(x, x, a0)
    s_ref, s_bound = _oracle(graph, x0, x0, a0, 0.2)
    _within(s.detach(), s_ref, s_bound, "forward share_weights")
    (s * w).sum().backward()
    l, r = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    (op(l, r, a0) * w).sum().backward()
    assert _same_bits(x.grad, l.grad + r.grad)


def test_two_head_gatv2_layer_against_a_dense_float64_layer(cuda_device):
    """GATv2Score -> EdgeSoftmax -> SpMMHeads on the 37 x 5 pattern with duplicates, H = 2, D = 8, all fp32, against a dense float64
    layer in which a duplicate entry counts as often as it occurs.  Tolerances: the fp32 pipeline is a handful of sums of at most 12
    terms and well-conditioned maps (softmax of O(1) scores, cross entropy), so its relative error is some tens of 2^-24; 1e-4 of the
    loss and 1e-3 of every gradient's norm leave two orders for the cancellation in the gradients.  A gate that flips between fp32 and
    float64 needs |z| < 1e-6 on one of 2,900 elements."""
    from voltrix.autograd import EdgeSoftmax, GATv2Score, SpMMHeads

    graph = _rect()
    n, m, in_feats, heads, d = graph.num_rows, graph.num_cols, 6, 2, 8
    aggregate = SpMMHeads(graph.indptr, graph.indices, n, m)
    score = GATv2Score(graph.indptr, graph.indices, n, m, transposed=(aggregate.t_indptr, aggregate.t_indices, aggregate.t_order))
    softmax = EdgeSoftmax(graph.indptr, n)
    torch.manual_seed(13)
    x_dst, x_src = torch.randn(n, in_feats, device="cuda"), torch.randn(m, in_feats, device="cuda")
    y = torch.randint(0, d, (n,), device="cuda")
    params = {"wl": torch.randn(in_feats, heads * d, device="cuda") / in_feats ** 0.5,
              "wr": torch.randn(in_feats, heads * d, device="cuda") / in_feats ** 0.5,
              "a": torch.randn(heads, d, device="cuda") / d ** 0.5}

    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    xl, xr = (x_dst @ p["wl"]).view(n, heads, d), (x_src @ p["wr"]).view(m, heads, d)
    out = aggregate(xr, softmax(score(xl, xr, p["a"], 0.2)))
    loss = torch.nn.functional.cross_entropy(out.mean(1), y)
    loss.backward()

    r = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    count = torch.zeros(n, m, dtype=torch.float64, device="cuda").index_put_((graph.rows, graph.cols),
                                                                             torch.ones(graph.nnz, dtype=torch.float64, device="cuda"),
                                                                             accumulate=True)
    xl64, xr64 = (x_dst.double() @ r["wl"]).view(n, heads, d), (x_src.double() @ r["wr"]).view(m, heads, d)
    s64 = (r["a"] * torch.nn.functional.leaky_relu(xl64[:, None] + xr64[None, :], float(np.float32(0.2)))).sum(-1)     # [n, m, H]
    weight = count[:, :, None] * torch.exp(s64 - s64.max(dim=1, keepdim=True).values)
    attn = weight / weight.sum(dim=1, keepdim=True).clamp_min(1e-300)                                       # empty rows: zeros
    out64 = torch.einsum("ijh,jhd->ihd", attn, xr64)
    ref_loss = torch.nn.functional.cross_entropy(out64.mean(1), y)
    ref_loss.backward()
    print(f"layer: loss {float(loss):.7f} vs {float(ref_loss):.7f}")
    assert abs(float(loss) - float(ref_loss)) <= 1e-4 * abs(float(ref_loss))
    for name in params:
        err = float((p[name].grad.double() - r[name].grad).norm() / r[name].grad.norm())
        print(f"layer: d_{name} relative error {err:.2e}")
        assert err <= 1e-3, (name, err)
