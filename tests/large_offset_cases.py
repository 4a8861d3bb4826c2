"""Cases of tests/test_gpu_large_offsets.py, shared with its CPU checks (tests/test_large_offset_cases.py): attention problems whose
element offsets pass 2^31, built so that the float64 reference stays small.

A big problem is one PERIOD repeated: ``P`` rows with ``P_e`` edges (row lengths, column ids, scores, gradients and every per-row
operand), ``reps`` times, then a TAIL -- the first rows of the period again, the last of them cut -- so that ``nnz`` is exactly what the
test asks for.  ``P_e`` is odd, so the periods fall at every offset against the 2,048-edge chunks of the kernels.  Everything an
operator computes per edge or per row is a function of the row alone, so the reference of the whole problem is the period's reference
``reps`` times and the tail's once; a sum over a COLUMN collects ``reps`` times the period's terms plus the tail's
(``Periodic.col_sum``).  The tail's column ids are the period's plus ``num_cols / 2``: the upper half of the columns holds the
tail's entries alone -- the edges next to and past the boundary -- so that one misplaced term among a column's few shows against a bound
that grows with the column's degree (a period column holds ``reps`` times as many).  ``check_tiled`` compares every period of a result with the one reference, a slab of periods at a time on the
result's device, counts what it visited and asserts that this is every element.

Nothing here needs a GPU: the CPU test runs the same code with the boundary moved down (a chunk of 8 edges, 2^12 in the place of
2^31) and compares it with the whole small problem worked out directly.

The oracles are float64 torch from the inputs as stored.  Their bounds are the ones the operators' own GPU tests assert, restated so
that they run on any device and on a graph given by its row and column ids (tests/test_gpu_large_offsets.py compares them with the
originals on those tests' own inputs; the one term that is not theirs is ``cast_bound``, from the number formats):

  SDDMM           tests/test_gpu_heads.py      D u |x| |y|
  edge softmax    tests/test_gpu_heads.py      alpha 2 (deg + |z - m| + 2) u + 2^-126;  backward |scale| alpha (2 |g - D_r| + (deg + 2) A_r) u + 2^-126
  aggregation     tests/test_gpu_heads.py      deg u sum |v| |feat|
  GAT scores      tests/test_gpu_gat_score.py  1.5 u |ref| + 2^-149 (2^-24 |ref| for slope 1 or a power of two);  sums deg u sum |gz| + 2^-149
  GATv2 scores    tests/test_gpu_gatv2.py      (D + 2) u sum |a| |leaky z| + 2^-149;  row sums deg u sum |term| + 2^-149
  attn_aggregate  tests/test_gpu_attn_aggregate.py, with a keep mask tests/test_gpu_attn_dropout.py

with ``u = 2^-23`` and ``deg`` the entries of the row (of the column for a sum over a column).
"""
import numpy as np
import torch

U = 2.0 ** -23
TINY = 2.0 ** -126
DENORM = 2.0 ** -149
CHUNK = 2048          # kChunkEdges of the edge softmax and the GAT kernels; the SDDMM-shaped kernels use 128, which divides it
RND = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}     # a cast to the dtype (tests/test_gpu_heads.py)


# ------------------------------------------------------------------------------------------------------------------- the pattern
def period_lengths(chunk=CHUNK, seed=5):
    """Row lengths of one period: empty rows, rows of one edge, rows of chunk - 1, chunk and chunk + 1 edges, a row longer than two
    chunks, a hub of 19 chunks, short random rows; the sum is odd."""
    rng = np.random.default_rng(seed)
    short = max(3, min(40, chunk // 2))
    lengths = [0, 1, 2 * chunk + 5, 1, chunk - 1, chunk, chunk + 1, 0, 0, 3]
    lengths += [int(v) for v in rng.integers(1, short, 20)]
    lengths += [19 * chunk + 3, 1, 0, short + 1]
    lengths += [int(v) for v in rng.integers(1, max(2, chunk // 4), 6)]
    if sum(lengths) % 2 == 0:
        lengths[-1] += 1
    return np.asarray(lengths, np.int64)


class Graph:
    """A CSR pattern given by its row lengths and column ids, as the oracles take it: int64 ``rows`` / ``cols`` per edge and float64
    ``row_deg`` on ``device``."""

    def __init__(self, lengths, cols, num_cols, device):
        lengths, cols = np.asarray(lengths, np.int64), np.asarray(cols, np.int64)
        self.num_rows, self.num_cols, self.nnz = len(lengths), int(num_cols), int(lengths.sum())
        assert cols.size == self.nnz and (self.nnz == 0 or (0 <= cols.min() and cols.max() < num_cols))
        self.lengths, self.cols_np = lengths, cols
        self.ip = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        self.rows_np = np.repeat(np.arange(self.num_rows), lengths)
        self.order_np = np.argsort(cols, kind="stable")
        self.col_deg_np = np.bincount(cols, minlength=num_cols).astype(np.int64)
        self.t_ip = np.concatenate([[0], np.cumsum(self.col_deg_np)]).astype(np.int64)
        self.device = torch.device(device)
        dev = lambda x, t=torch.int64: torch.from_numpy(np.ascontiguousarray(x)).to(t).to(self.device)     # noqa: E731
        self.rows, self.cols = dev(self.rows_np), dev(cols)
        self.row_deg = dev(lengths, torch.float64)

    def zeros(self, *shape):
        return torch.zeros(shape, dtype=torch.float64, device=self.device)

    def row_sum(self, t):
        return self.zeros(self.num_rows, *t.shape[1:]).index_add_(0, self.rows, t)

    def col_sum(self, t):
        return self.zeros(self.num_cols, *t.shape[1:]).index_add_(0, self.cols, t)


class Periodic:
    """``reps`` whole periods and a tail, ``nnz`` edges in all.  The tail is the period's first ``tail_rows`` rows, the last of them cut
    to ``cut`` edges (``cut == 0``: the tail ends with a whole row), its column ids moved up by ``num_cols / 2``: ``cols`` lie in the
    lower half of the ``num_cols`` columns.  ``period`` and ``tail`` are ``Graph``s of their own, over all the columns."""

    def __init__(self, lengths, cols, num_cols, nnz, device):
        assert num_cols % 2 == 0 and (len(cols) == 0 or np.max(cols) < num_cols // 2)
        self.period = Graph(lengths, cols, num_cols, device)
        p = self.period
        self.P, self.P_e, self.num_cols, self.nnz, self.device = p.num_rows, p.nnz, int(num_cols), int(nnz), p.device
        self.reps = self.nnz // self.P_e
        self.tail_e = self.nnz - self.reps * self.P_e
        whole = int(np.searchsorted(p.ip, self.tail_e, side="right")) - 1          # rows of the period that fit the tail whole
        self.cut = self.tail_e - int(p.ip[whole])
        tail_lengths = list(p.lengths[:whole]) + ([self.cut] if self.cut else [])
        self.tail_rows = len(tail_lengths)
        self.tail = Graph(tail_lengths, p.cols_np[:self.tail_e] + num_cols // 2, num_cols, device)
        self.num_rows = self.reps * self.P + self.tail_rows
        assert self.reps >= 1 and self.tail.nnz == self.tail_e and self.reps * self.P_e + self.tail_e == self.nnz

    # ---- the whole pattern, on the device
    def indptr(self):
        p, dev = self.period, self.device
        ip = torch.from_numpy(p.ip[:-1]).to(dev)
        whole = (ip[None, :] + torch.arange(self.reps, device=dev)[:, None] * self.P_e).reshape(-1)
        tail = torch.from_numpy(self.tail.ip).to(dev) + self.reps * self.P_e       # ends with nnz
        return torch.cat([whole, tail]).to(torch.int32)

    def indices(self):
        return torch.cat([self.period.cols.to(torch.int32).repeat(self.reps), self.tail.cols.to(torch.int32)])

    def transposed(self):
        """(t_indptr, t_indices, t_order) int32 of the whole pattern's transpose by a stable sort by column, from the stable sorts of
        the period and of the tail: column c holds the period's entries of c once per period, in the period's order, then the tail's."""
        p, t, dev = self.period, self.tail, self.device
        g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)     # noqa: E731
        deg_p, deg_t, ip_p, ip_t = g(p.col_deg_np), g(t.col_deg_np), g(p.t_ip), g(t.t_ip)
        t_indptr = self.reps * ip_p + ip_t
        pos = torch.arange(self.nnz, device=dev)
        col = torch.searchsorted(t_indptr, pos, right=True) - 1
        local = pos - t_indptr[col]
        in_periods = local < self.reps * deg_p[col]
        k = torch.where(in_periods, local // deg_p[col].clamp_min(1), torch.zeros_like(local))
        i = torch.where(in_periods, local - k * deg_p[col], local - self.reps * deg_p[col])
        del pos, local
        at_p = (ip_p[col] + i).clamp_max(max(self.P_e - 1, 0))
        at_t = (ip_t[col] + i).clamp_max(max(self.tail_e - 1, 0))
        del col, i
        e_p = g(p.order_np)[at_p]
        e_t = g(t.order_np)[at_t] if self.tail_e else torch.zeros_like(e_p)
        del at_p, at_t
        order = torch.where(in_periods, k * self.P_e + e_p, self.reps * self.P_e + e_t)
        r_t = t.rows[e_t] if self.tail_e else torch.zeros_like(e_p)
        rows = torch.where(in_periods, k * self.P + p.rows[e_p], self.reps * self.P + r_t)
        return t_indptr.to(torch.int32), rows.to(torch.int32), order.to(torch.int32)

    # ---- operands
    def tile_edges(self, x, x_tail=None):
        """[P_e, ...] -> [nnz, ...]: the period ``reps`` times, then its first ``tail_e`` entries (or ``x_tail`` [tail_e, ...])."""
        return self._tile(x, self.P_e, self.tail_e, x_tail)

    def tile_rows(self, x, x_tail=None):
        """[P, ...] -> [num_rows, ...]."""
        return self._tile(x, self.P, self.tail_rows, x_tail)

    def _tile(self, x, period, tail, x_tail):
        assert x.shape[0] == period and (x_tail is None or x_tail.shape[0] == tail)
        out = torch.empty((self.reps * period + tail,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
        out[:self.reps * period].view((self.reps, period) + tuple(x.shape[1:])).copy_(x.unsqueeze(0))
        out[self.reps * period:] = x[:tail] if x_tail is None else x_tail
        return out

    # ---- sums over the columns of the whole pattern
    def col_sum(self, term_p, term_t):
        """float64 [num_cols, ...]: ``reps`` times the column sums of the period's terms plus those of the tail's."""
        return self.reps * self.period.col_sum(term_p) + self.tail.col_sum(term_t)

    def col_deg(self):
        dev = lambda x: torch.from_numpy(x).to(torch.float64).to(self.device)     # noqa: E731
        return self.reps * dev(self.period.col_deg_np) + dev(self.tail.col_deg_np)


def make_periodic(nnz, num_cols, device, chunk=CHUNK, seed=5, last_row_crosses=False):
    """A ``Periodic`` of exactly ``nnz`` edges over ``num_cols`` columns (an even number: the period's ids uniform over the lower half,
    sorted inside every row, duplicates kept; the tail's in the upper half).  The period holds what the kernels branch on: an empty row, rows of one edge, a row longer than two chunks, rows that cross a chunk
    boundary, and its edge count is no multiple of the chunk.  ``last_row_crosses``: the hub's length is moved (by even steps) until the
    tail's cut row starts before the last chunk, which is partial, and ends in it."""
    lengths = period_lengths(chunk, seed)
    hub = int(np.argmax(lengths))
    for _ in range(4096):
        p_e = int(lengths.sum())
        ip = np.concatenate([[0], np.cumsum(lengths)])
        tail_e = nnz % p_e
        whole = int(np.searchsorted(ip, tail_e, side="right")) - 1
        cut = tail_e - int(ip[whole])
        last_chunk = (nnz - 1) // chunk * chunk
        if not last_row_crosses or (nnz % chunk != 0 and cut > 0 and nnz - cut < last_chunk):
            break
        lengths[hub] += 2
    else:
        raise AssertionError("no period length found")
    rng = np.random.default_rng(seed + 1)
    rows = np.repeat(np.arange(len(lengths)), lengths)
    cols = rng.integers(0, num_cols // 2, p_e)
    cols = np.sort(rows * num_cols + cols) % num_cols
    pc = Periodic(lengths, cols, num_cols, nnz, device)
    assert_period_properties(pc, chunk)
    return pc


def assert_period_properties(pc, chunk=CHUNK):
    lengths, ip = pc.period.lengths, pc.period.ip
    assert pc.P_e % chunk != 0 and pc.P_e % 2 == 1, pc.P_e
    assert (lengths == 0).any() and (lengths == 1).any() and (lengths > 2 * chunk).any()
    crossing = (ip[:-1] // chunk != (ip[1:] - 1) // chunk) & (lengths > 0) & (lengths <= chunk + 1)
    assert crossing.any()                                # a row shorter than a chunk and a bit that still crosses a boundary
    # the periods start at more than one offset against the chunks, and the whole pattern is a CSR of nnz edges
    assert len({(k * pc.P_e) % chunk for k in range(min(pc.reps, 8))}) == min(pc.reps, 8)
    assert pc.nnz == pc.reps * pc.P_e + pc.tail_e and 0 <= pc.tail_e < pc.P_e


# -------------------------------------------------------------------------------------------------------------- the comparison
class Tally:
    """Elements of each named output that a check has visited; ``assert_complete`` is the helper module's guard that no element of a
    big output is left unchecked."""

    def __init__(self):
        self.visited, self.sizes, self.worst = {}, {}, {}

    def add(self, what, visited, size, worst=0.0):
        self.visited[what] = self.visited.get(what, 0) + int(visited)
        self.sizes[what] = int(size)
        self.worst[what] = max(self.worst.get(what, 0.0), worst) if worst == worst else worst      # a NaN stays

    def assert_complete(self, *names):
        for what in names:
            assert what in self.visited, (what, sorted(self.visited))
        for what, size in self.sizes.items():
            assert self.visited[what] == size, (what, self.visited[what], size)


def _slabs(reps, per_period, slab_elems):
    k = max(1, slab_elems // max(1, per_period))
    return [(r, min(reps, r + k)) for r in range(0, reps, k)]


def check_tiled(out, reps, period, tail, what, tally, slab_elems=1 << 26):
    """Every period of ``out`` against ``period = (ref, bound)`` and what follows them against ``tail = (ref, bound)``, element by
    element: ``|out - ref| <= bound`` (a NaN in ``out`` fails).  Returns (all within, max of error / bound).  ``bound = None``: equality."""
    ref, bound = period
    n = ref.shape[0]
    assert out.shape[0] == reps * n + tail[0].shape[0] and out.shape[1:] == ref.shape[1:] == tail[0].shape[1:], \
        (what, tuple(out.shape), reps, tuple(ref.shape), tuple(tail[0].shape))
    ok = torch.ones((), dtype=torch.bool, device=out.device)
    worst = torch.zeros((), dtype=torch.float64, device=out.device)
    visited = 0

    def one(block, r, b):
        nonlocal ok, worst, visited
        visited += block.numel()
        if block.numel() == 0:
            return
        if b is None:
            ok = ok & (block.double() == r).all()
            return
        err = (block.double() - r).abs()
        ok = ok & (err <= b).all()
        worst = torch.maximum(worst, (err / b.clamp_min(1e-300)).max())

    for lo, hi in _slabs(reps, ref.numel(), slab_elems):
        one(out[lo * n:hi * n].view((hi - lo,) + tuple(ref.shape)), ref, bound)
    one(out[reps * n:], tail[0], tail[1])
    assert visited == out.numel(), (what, visited, out.numel())
    worst = float(worst)
    tally.add(what, visited, out.numel(), worst)
    print(f"{what}: {out.numel()} elements in {reps} periods and a tail, max err / bound = {worst:.3f}")
    return bool(ok), worst


def check_whole(out, ref, bound, what, tally):
    """A result that is not periodic (a sum over columns): every element against (ref, bound)."""
    return check_tiled(out, 0, (ref[:0], None if bound is None else bound[:0]), (ref, bound), what, tally)


# ------------------------------------------------------------------------------------------------------------------ the oracles
def f32(v):
    return float(np.float32(v))


def sddmm_oracle(g, x, y):
    """(ref, bound) [nnz, H]: x [num_rows, H, D], y [num_cols, H, D]."""
    xe, ye = x.double()[g.rows], y.double()[g.cols]
    return (xe * ye).sum(-1), x.shape[-1] * U * (xe.abs() * ye.abs()).sum(-1)


def softmax_parts(g, s, scale):
    """float64 pieces of the edge softmax of ``scale * s`` [nnz, H] per row: (alpha, x = |z - m| with 0 for a masked entry, m of
    sign(scale) s per row, L per row, w = exp(-x))."""
    sc = f32(scale)
    sign, a = (-1.0 if sc < 0 else 1.0), abs(sc)
    heads = s.shape[1]
    key = sign * s.double()
    m = torch.full((g.num_rows, heads), float("-inf"), dtype=torch.float64, device=s.device)
    if g.nnz:
        m = m.scatter_reduce(0, g.rows[:, None].expand(-1, heads), key, "amax", include_self=True)
    masked = key == float("-inf")
    x = torch.where(masked, torch.zeros_like(key), a * (m[g.rows] - torch.where(masked, torch.zeros_like(key), key)))
    w = torch.where(masked, torch.zeros_like(x), torch.exp(-x))
    big_l = g.row_sum(w)
    inv = torch.where(big_l > 0, 1.0 / big_l, torch.zeros_like(big_l))
    return w * inv[g.rows], x, m, big_l, w, inv


def softmax_oracle(g, s, scale):
    alpha, x, *_ = softmax_parts(g, s, scale)
    return alpha, alpha * 2 * (g.row_deg[g.rows][:, None] + x + 2) * U + TINY


def softmax_backward_oracle(g, alpha, grad, scale):
    """(ref, bound) of scale alpha (g - rowsum(alpha g)) from the float32 alpha and grad [nnz, H] the kernel is given."""
    sc = f32(scale)
    a, gd = alpha.double(), grad.double()
    d = g.row_sum(a * gd)[g.rows]
    aa = g.row_sum(a * gd.abs())[g.rows]
    return sc * a * (gd - d), abs(sc) * a * (2 * (gd - d).abs() + (g.row_deg[g.rows][:, None] + 2) * aa) * U + TINY


def aggregate_oracle(g, v, feat, roundings=0):
    """(ref, bound) [num_rows, H, D] of sum_e v[e, h] feat[col_e, h]; ``roundings = 1``: one more rounding for the sum's last step, the
    bound the autograd tests use for a gradient that is such a sum (tests/test_gpu_heads.py ``_grad_bound_ok``)."""
    f = feat.double()[g.cols]
    term = v.double()[:, :, None] * f
    return g.row_sum(term), (g.row_deg[:, None, None] + roundings) * U * g.row_sum(term.abs())


def aggregate_columns_oracle(g, v, x, roundings=0):
    """(ref, bound) [num_cols, H, D] of the same sum over the columns: sum_{e in column c} v[e, h] x[row_e, h] (the transposed CSR)."""
    term = v.double()[:, :, None] * x.double()[g.rows]
    deg = torch.from_numpy(g.col_deg_np).to(torch.float64).to(g.device)
    return g.col_sum(term), (deg[:, None, None] + roundings) * U * g.col_sum(term.abs())


def _pow2(slope):
    m = abs(f32(slope))
    return m == 0 or np.log2(m) == np.floor(np.log2(m))


def gat_oracle(g, el, er, slope, grad=None):
    """(s, bound) [nnz, H]; with grad [nnz, H] also (d_el, bound) per row and gz [nnz, H], the terms of d_er's sums over columns."""
    sl = f32(slope)
    z = el.double()[g.rows] + er.double()[g.cols]
    ref = torch.where(z > 0, z, sl * z)
    bound = (2.0 ** -24 if _pow2(slope) else 1.5 * U) * ref.abs() + DENORM
    if grad is None:
        return ref, bound
    gz = torch.where(z > 0, grad.double(), sl * grad.double())
    return (ref, bound), (g.row_sum(gz), g.row_deg[:, None] * U * g.row_sum(gz.abs()) + DENORM), gz


def gatv2_oracle(g, xl, xr, a, slope, grad=None):
    """(s, bound) [nnz, H]; with grad also (G_l, bound) [num_rows, H, D] and term [nnz, H, D], the terms of G_r's sums over columns."""
    sl = f32(slope)
    z = xl.double()[g.rows] + xr.double()[g.cols]
    gate = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, sl))
    lz = gate * z
    s = (a.double() * lz).sum(-1)
    s_bound = (xl.shape[-1] + 2) * U * (a.double().abs() * lz.abs()).sum(-1) + DENORM
    if grad is None:
        return s, s_bound
    term = gate * grad.double()[:, :, None]
    return (s, s_bound), (g.row_sum(term), g.row_deg[:, None, None] * U * g.row_sum(term.abs()) + DENORM), term


def column_bound(deg, mass):
    """deg u sum |term| + 2^-149: the sums over a column of gat_score_backward and gatv2_rowsum (``deg`` broadcast over ``mass``)."""
    return deg.view((-1,) + (1,) * (mass.dim() - 1)) * U * mass + DENORM


def attn_oracle(g, s, feat, grad, scale, keep=None, ks=1.0):
    """tests/test_gpu_attn_aggregate.py's oracle (with ``keep`` bool [nnz, H] and ``ks``: tests/test_gpu_attn_dropout.py's) on a graph
    given by ids: (value, bound) of out, l and d_s, m, and ``cols``: the per-edge tensors whose sums over columns make d_feat and its
    bound (``d_feat_of``).  ``grad`` is dC [num_rows, H, D]."""
    sc = f32(scale)
    dim = feat.shape[-1]
    drop = keep is not None
    extra = 1.0 if drop else 0.0                        # one more u per weight for the rounding of w k
    alpha, x, m, big_l, w, inv = softmax_parts(g, s, scale)
    k = keep.double() * f32(ks) if drop else torch.ones_like(alpha)
    deg = g.row_deg[:, None]
    l_bound = (deg + 2) * U * big_l + 2 * U * g.row_sum(w * x) + deg * TINY
    f = feat.double()[g.cols]
    if drop:
        f = torch.where(keep[:, :, None], f, torch.zeros_like(f))                      # a dropped entry's feat is never read
    ak = (alpha * k)[:, :, None]
    out = g.row_sum(ak * f)
    mass = g.row_sum(ak * f.abs())
    plain = g.row_sum(k[:, :, None] * f.abs())
    out_bound = (2 * (deg[:, :, None] + 3) + extra) * U * mass + U * plain * inv[:, :, None] + TINY
    eta = (2 * x + 2) * U + (l_bound * inv)[g.rows] + 2 * U
    gd = grad.double()
    ge = gd[g.rows]
    dot = (ge * f).sum(-1)
    dot_bound = (dim + 2) * U * (ge.abs() * f.abs()).sum(-1)
    delta = (gd * out).sum(-1)
    delta_bound = (dim + 2) * U * (gd.abs() * (out.abs() + out_bound)).sum(-1) + (gd.abs() * out_bound).sum(-1)
    diff = k * dot - delta[g.rows]
    d_s = sc * alpha * diff
    d_s_bound = (abs(sc) * alpha * (k * dot_bound + extra * U * k * dot.abs() + delta_bound[g.rows] + diff.abs() * (eta + 2 * U))
                 + TINY * (1 + abs(sc) * diff.abs()))
    term = ak * ge
    cols = {"term": term, "mass": term.abs(), "eta_mass": (eta + extra * U)[:, :, None] * term.abs(), "plain": k[:, :, None] * ge.abs()}
    return {"out": (out, out_bound), "l": (big_l, l_bound), "d_s": (d_s, d_s_bound), "m": m, "cols": cols}


def d_feat_of(col_deg, sums):
    """(d_feat, bound) [num_cols, H, D] from the column degrees and the column sums of ``attn_oracle``'s ``cols``."""
    bound = col_deg[:, None, None] * U * sums["mass"] + sums["eta_mass"] + TINY * (1 + sums["plain"])
    return sums["term"], bound


def cast_bound(ref, bound, dtype):
    """The bound of a float32 result within ``bound`` of ``ref`` once it is cast to ``dtype``: one rounding of the COMPUTED value,
    ``RND (|ref| + bound)``, and half of the type's smallest subnormal (2^-25 in fp16).  This is not the cast term of
    tests/test_gpu_heads.py's ``_grad_bound_ok``, ``RND |ref| + 1e-30``, which is looser nowhere and tighter by ``RND bound`` and by the
    subnormal half-ulp: that form rounds the reference, not what the kernel computed, and allows 1e-30 where an fp16 result below 2^-14
    can be 2^-25 off.  It holds on that test's inputs and is left as it is there; here the numbers come from the formats alone
    (2^-11 and 2^-25 for fp16), and the difference is at most a factor 1 + 2^-11 on the cast term plus 3e-8."""
    if dtype == torch.float32:
        return bound
    return bound + RND[dtype] * (ref.abs() + bound) + (2.0 ** -25 if dtype == torch.float16 else 2.0 ** -134)


def unpack_keep(mask, heads):
    """bool [n, heads] from the packed int32 mask [n, ceil(heads / 32)] (restated, not voltrix.dropout.unpack_mask)."""
    words = mask.to(torch.int64) & 0xFFFFFFFF
    h = torch.arange(heads, device=mask.device)
    return ((words[:, h // 32] >> (h % 32)[None, :]) & 1) == 1


def popcount32(words):
    """int64 number of set bits of every int32 word (as an unsigned 32-bit value)."""
    v = words.to(torch.int64) & 0xFFFFFFFF
    v = v - ((v >> 1) & 0x55555555)
    v = (v & 0x33333333) + ((v >> 2) & 0x33333333)
    v = (v + (v >> 4)) & 0x0F0F0F0F
    return ((v * 0x01010101) & 0xFFFFFFFF) >> 24


# ----------------------------------------------------------------------------------- a big node axis with a few rows in use
def axis_ids(count, stride, boundary=2 ** 31, low=(0, 1, 2, 5)):
    """Sorted ids in [0, count) of a node tensor [count, stride]: low ones, the ids on either side of the row where the element offset
    ``id * stride`` passes ``boundary / 2`` (2^32 bytes in fp32) and of the row where it passes ``boundary``, and the last id."""
    ids = set(low)
    for limit in (boundary // 2, boundary):
        first = -(-limit // stride)                      # the first id whose row starts at or past the limit
        assert 1 <= first < count - 2, (count, stride, limit)
        ids |= {first - 1, first, first + 1}
    ids.add(count - 1)
    return np.asarray(sorted(ids), np.int64)


class AxisCase:
    """A pattern between ``small`` nodes and a node axis of ``count`` ids of which only ``axis_ids`` and a few random ones have
    entries: about 2,000 entries, duplicates among them.  ``big`` = "cols": rows are the small nodes (some empty), columns the big axis;
    "rows": the transpose -- almost every row is empty.  ``real``: the int32 CSR with the real ids; ``compact``: the ``Graph`` with the
    big ids renumbered 0 .. len(used) - 1 (``used``: the sorted big ids that have entries), which is what the float64 reference runs on."""

    def __init__(self, count, stride, small, big, device, boundary=2 ** 31, seed=3):
        assert big in ("cols", "rows")
        rng = np.random.default_rng(seed)
        special = axis_ids(count, stride, boundary)
        others = rng.choice(count, 40, replace=False)
        pool = np.unique(np.concatenate([special, others]))
        n = 2000
        big_id = np.concatenate([special, rng.choice(pool, n - special.size)])      # every special id at least once
        small_id = rng.integers(0, small, n)
        small_id[small_id % 17 == 3] = 4                                           # a hub, and small nodes without entries
        big_id[:6] = special[-1]                                                   # duplicates: (4, last id) six times
        small_id[:6] = 4
        self.count, self.small, self.big, self.stride, self.boundary = count, small, big, stride, boundary
        self.used = np.unique(big_id)
        compact_id = np.searchsorted(self.used, big_id)
        if big == "cols":
            rows, cols, rows_c, cols_c = small_id, big_id, small_id, compact_id
            self.num_rows, self.num_cols, nr_c, nc_c = small, count, small, self.used.size
        else:
            rows, cols, rows_c, cols_c = big_id, small_id, compact_id, small_id
            self.num_rows, self.num_cols, nr_c, nc_c = count, small, self.used.size, small
        order = np.lexsort((cols, rows))                                           # CSR order: by row, columns sorted inside a row
        self.rows_np, self.cols_np = rows[order], cols[order]
        self.compact = Graph(np.bincount(rows_c, minlength=nr_c), cols_c[order], nc_c, device)
        assert np.array_equal(self.compact.rows_np, rows_c[order])
        ip = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=self.num_rows))])
        self.indptr = torch.from_numpy(ip.astype(np.int32)).to(device)
        self.indices = torch.from_numpy(self.cols_np.astype(np.int32)).to(device)
        self.used_t = torch.from_numpy(self.used).to(device)
        self.nnz = n

    def crosses(self):
        """True when entries lie on both sides of both limits (the element offsets of the used ids)."""
        off = self.used * self.stride
        return all((off < limit).any() and (off >= limit).any() for limit in (self.boundary // 2, self.boundary))


def check_rows(out, used, ref, bound, what, tally):
    """``out`` [count, ...]: the rows ``used`` within ``bound`` of ``ref`` [len(used), ...], every other row exactly zero (a reduction
    over the whole tensor; a NaN anywhere fails).  Returns (all within and zero elsewhere, max of error / bound)."""
    picked = out[used]
    zero_elsewhere = int(torch.count_nonzero(out)) == int(torch.count_nonzero(picked))
    err = (picked.double() - ref).abs()
    ok = bool((err <= bound).all()) and zero_elsewhere
    worst = float((err / bound.clamp_min(1e-300)).max())
    tally.add(what, out.numel(), out.numel(), worst)
    print(f"{what}: {out.numel()} elements, {used.numel()} rows in use, zero elsewhere: {zero_elsewhere}, max err / bound = {worst:.3f}")
    return ok, worst
