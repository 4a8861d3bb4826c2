"""The harness and the cases of tests/test_gpu_stream_order.py: what it takes to SEE a launch that went to the wrong stream, a host
read-back where none is promised, and a temporary that a graph capture does not recompute.

A case is a callable ``run(*operands) -> tuple of tensors`` over "late" operands -- value tensors only (features, edge features, values,
scores, gradients, coefficients; for the samplers seed and node id lists) -- plus a legal prefill for each of them: NaN for a float
operand, a DIFFERENT set of in-range ids for an id list.  The CSR structure (``indptr``, ``indices``, the transpose, ``t_order``,
``etype``, the ``TypeIndex``, an exclusion list, a ``SamplingWeights``) is closed over by ``run``: it is never late and never garbage, so
no kernel is ever handed an index it may not follow and nothing here reads out of bounds.

``delayed_producer``: the operands' buffers hold the prefill; on a side stream a calibrated device-side delay is enqueued, then the
copies of the real data, then ``run``; the default stream waits for the side stream and only then the host synchronises.  Whatever was
not ordered behind the copies -- a launch given another stream's handle, a cast or a pad made on another stream -- reads the prefill and
changes the bits.  ``capture_and_replay``: ``run`` captured once on static operands and replayed on a SECOND set of values with every
output poisoned in between; a temporary computed outside the captured work, or an element a launch does not rewrite, changes the
bits.  ``SyncCounter``: the host synchronisations of a call, counted by ``torch.cuda.set_sync_debug_mode("warn")``.

Every sync-free case also carries ``check(operands, outputs)``: its outputs against a float64 reference of the same operation
(tests/spmm_*_oracle.py, or the float64 torch composite and the bound the operator's own test uses), so that the bit comparisons hang
on a reference and not on the code under test.  The autograd wrappers are anchored to the functional operators checked that way.
"""
import collections
import functools
import warnings

import numpy as np
import torch

from conftest import load_csr_fixture
from test_hybrid_plan import _random_csr

U = 2.0 ** -23
MIN_DELAY_MS = 20.0       # three orders of magnitude above the 25-60 us of host time an eager call costs: a choice, not a measurement
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
NUM_TYPES, NUM_BASES = 5, 3
AGGREGATES = ("sum", "mean", "max", "min", "var", "std")
PNA = ("mean", "max", "min", "std")
EPS = 1e-5


# ------------------------------------------------------------------------------------------------------------------------ the harness
@functools.lru_cache(maxsize=None)
def calibrated_delay():
    """``(enqueue, kind, count, measured_ms)``, calibrated once per session with a pair of events: ``enqueue()`` puts at least
    ``MIN_DELAY_MS`` of device time on the current stream -- ``torch.cuda._sleep(count)`` (``kind == "cycles"``), or a chain of ``count``
    2048^3 matmuls where this torch has no ``_sleep`` (``kind == "matmuls"``)."""
    sleep = getattr(torch.cuda, "_sleep", None)
    if sleep is not None:
        kind, count, spin = "cycles", 1_000_000, sleep
    else:
        a = torch.full((2048, 2048), 2.0 ** -11, device="cuda")
        b = torch.empty_like(a)

        def spin(n):
            for _ in range(n):
                torch.mm(a, a, out=b)
        kind, count = "matmuls", 16

    def measure(n):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        spin(n)
        end.record()
        end.synchronize()
        return start.elapsed_time(end)

    measure(count)                                           # the first launch pays for loading the kernel
    count = int(count * 1.5 * MIN_DELAY_MS / max(measure(count), 1e-3)) + 1
    ms = measure(count)
    for _ in range(8):                                       # a clock that changed between the two measurements
        if ms >= MIN_DELAY_MS:
            break
        count *= 2
        ms = measure(count)
    assert ms >= MIN_DELAY_MS, (kind, count, ms)
    print(f"delay: {count} {kind} = {ms:.1f} ms")
    return functools.partial(spin, count), kind, count, ms


def same_bits(x, y):
    if x.dtype != y.dtype or x.shape != y.shape:
        return False
    return torch.equal(x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8))


def differing(first, second):
    """The positions of the outputs whose bits differ (the whole range where the counts differ)."""
    if len(first) != len(second):
        return list(range(max(len(first), len(second))))
    return [i for i, (x, y) in enumerate(zip(first, second)) if not same_bits(x, y)]


def poison(t):
    """NaN into a float tensor, an e4m3 NaN code into an fp8 one, the most negative value into an integer one."""
    if t.dtype == torch.float8_e4m3fn:
        t.view(torch.uint8).fill_(0x7F)
    elif t.dtype.is_floating_point:
        t.fill_(float("nan"))
    else:
        t.fill_(torch.iinfo(t.dtype).min)


def delayed_producer(run, operands, prefill, side, delay=True):
    """The outputs of ``run`` on buffers that hold ``prefill`` until copies enqueued on ``side`` behind the delay overwrite them with
    ``operands``; ``run`` is called on ``side`` right after the copies, with no synchronisation in between."""
    enqueue = calibrated_delay()[0]
    buffers = [torch.empty_like(t) for t in operands]
    for buffer, fill in zip(buffers, prefill):
        if fill is None:
            assert buffer.dtype.is_floating_point, "an id list needs a prefill of in-range ids"
            poison(buffer)
        else:
            assert fill.shape == buffer.shape and fill.dtype == buffer.dtype
            buffer.copy_(fill)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        if delay:
            enqueue()
        for buffer, real in zip(buffers, operands):
            buffer.copy_(real, non_blocking=True)
        outputs = run(*buffers)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return outputs


def capture_and_replay(run, operands, second):
    """``run`` captured on static copies of ``operands``: ``(outputs of the first replay, outputs of a replay on `second`)``, every
    output poisoned before the second replay.  One stream, one chain."""
    static = [t.clone() for t in operands]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outputs = run(*static)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in outputs]
    for buffer, value in zip(static, second):
        buffer.copy_(value)
    for t in outputs:
        poison(t)
    graph.replay()
    torch.cuda.synchronize()
    return replayed, list(outputs)


class SyncCounter:
    """``with SyncCounter() as syncs: ...; syncs.count()``: the host synchronisations torch has warned about so far inside the block
    (``set_sync_debug_mode("warn")``, every warning recorded)."""

    def __enter__(self):
        self._catch = warnings.catch_warnings(record=True)
        self._caught = self._catch.__enter__()
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        return self

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")
        self._catch.__exit__(*exc)
        return False

    def count(self):
        return sum("synchroniz" in str(w.message) for w in self._caught)


# ----------------------------------------------------------------------------------------------------------------------- the patterns
class Pattern:
    """A CSR pattern [num_rows, num_cols] on the device as a ``CsrPattern`` (with its transpose), the entry types of the relational
    operator with their ``TypeIndex``, and int64 ids and float64 degrees for the oracles."""

    def __init__(self, indptr, indices, num_rows, num_cols):
        from voltrix.autograd import CsrPattern
        from voltrix.spmm_rel import TypeIndex

        self.ip, self.ix = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
        self.num_rows, self.num_cols, self.nnz = num_rows, num_cols, len(self.ix)
        self.csr = CsrPattern(torch.from_numpy(self.ip.astype(np.int32)).cuda(), torch.from_numpy(self.ix.astype(np.int32)).cuda(),
                              num_rows, num_cols)
        for name in ("indptr", "indices", "t_indptr", "t_indices", "t_order"):
            setattr(self, name, getattr(self.csr, name))
        lengths = np.diff(self.ip)
        self.lengths = lengths
        self.rows = torch.from_numpy(np.repeat(np.arange(num_rows), lengths)).cuda()
        self.cols = torch.from_numpy(self.ix).cuda()
        self.deg = torch.from_numpy(lengths.astype(np.float64)).cuda()
        self.col_deg = torch.from_numpy(np.bincount(self.ix, minlength=num_cols).astype(np.float64)).cuda()
        self.sorted_rows = all(bool((np.diff(self.ix[b:e]) >= 0).all()) for b, e in zip(self.ip[:-1], self.ip[1:]))
        self.etype_np = np.random.default_rng(5).integers(0, NUM_TYPES, self.nnz)
        self.etype = torch.from_numpy(self.etype_np.astype(np.int32)).cuda()
        self.type_index = TypeIndex(self.etype, NUM_TYPES)


@functools.lru_cache(maxsize=None)
def pattern(name):
    if name == "skewed":           # rows of 0, 1, 3, 4, 5, 8 and 9 entries and a hub of 900
        g = load_csr_fixture("skewed_1005")
        n = int(g["num_nodes"])
        assert all((np.diff(g["indptr"]) == k).any() for k in (0, 1, 3, 4, 5, 8, 9))
        return Pattern(g["indptr"], g["indices"], n, n)
    assert name == "rect"
    indptr, indices = _random_csr(260, 30, seed=9, ncols=500)
    return Pattern(indptr, indices, 260, 500)


Shape = collections.namedtuple("Shape", ("pattern", "dtype", "tail"))
WHOLE = Shape("skewed", "fp32", (32,))         # whole 16-byte pieces: no padded copy
PADDED = Shape("rect", "fp16", (20,))          # padded to 24: a temporary is made between launches
HEADS = Shape("skewed", "fp16", (3, 20))       # trailing dimensions, padded per row
WIDE_HEADS = Shape("rect", "fp32", (3, 32))


def _id(shape):
    return f"{shape.pattern}-{shape.dtype}-" + "x".join(str(d) for d in shape.tail)


def randn(shape, dtype, seed, scale=1.0):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return (scale * torch.randn(tuple(shape), device="cuda", generator=gen)).to(dtype)


def _zeros(*shape):
    return torch.zeros(shape, dtype=torch.float64, device="cuda")


def row_sum(p, terms):
    return _zeros(p.num_rows, *terms.shape[1:]).index_add_(0, p.rows, terms)


def col_sum(p, terms):
    return _zeros(p.num_cols, *terms.shape[1:]).index_add_(0, p.cols, terms)


def within(got, ref, bound, what):
    ref = torch.as_tensor(ref, device=got.device) if isinstance(ref, np.ndarray) else ref
    bound = torch.as_tensor(bound, device=got.device) if isinstance(bound, np.ndarray) else bound
    assert got.numel() == ref.numel(), (what, tuple(got.shape), tuple(ref.shape))
    err = (got.double().reshape(ref.shape) - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: max err / bound = {worst:.3f}")
    assert bool((err <= bound).all()), (what, worst)


def cast_bound(ref, bound, dtype):
    """``bound`` plus the one rounding of the computed value to ``dtype`` (fp16: 2^-11 relative and half its smallest subnormal)."""
    rnd = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}[dtype]
    return bound + rnd * (ref.abs() + bound) + (2.0 ** -25 if dtype == torch.float16 else 0.0)


def _np(t):
    return t.detach().double().cpu().numpy()


# -------------------------------------------------------------------------------------------------------------------------- the cases
class Case:
    """``run``; ``make(seed) -> operands``; ``prefill(operands) -> list`` (None: NaN); ``check(operands, outputs)``; ``sync_free``."""

    def __init__(self, run, make, check=None, prefill=None, sync_free=True):
        self.run, self.make, self.check, self.sync_free = run, make, check, sync_free
        self._prefill = prefill
        self._operands, self._eager = {}, {}

    def operands(self, seed=0):
        """The operands of value set ``seed``: built once, shared, never written."""
        if seed not in self._operands:
            self._operands[seed] = tuple(self.make(seed))
        return self._operands[seed]

    def prefill(self):
        return [None] * len(self.operands()) if self._prefill is None else list(self._prefill())

    def eager(self, seed=0):
        """The outputs of an eager call on the default stream, synchronised: computed once, shared, never written."""
        if seed not in self._eager:
            outputs = tuple(self.run(*self.operands(seed)))
            torch.cuda.synchronize()
            self._eager[seed] = outputs
        return self._eager[seed]


REGISTRY = {}           # name -> (factory, sync_free): the names are known without a device, the cases are built on first use


def _register(name, factory, sync_free=True):
    assert name not in REGISTRY, name
    REGISTRY[name] = (factory, sync_free)


@functools.lru_cache(maxsize=None)
def get_case(name):
    factory, sync_free = REGISTRY[name]
    case = factory()
    assert case.sync_free == sync_free, name
    return case


def names(sync_free=None):
    return [name for name, (_, free) in REGISTRY.items() if sync_free is None or free == sync_free]


# ---- sddmm (2-D and heads), spmm_heads, csr_values_product
def _sddmm(shape):
    import voltrix

    p, dt, tail = pattern(shape.pattern), DT[shape.dtype], shape.tail

    def make(seed):
        return randn((p.num_rows,) + tail, dt, 10 + seed), randn((p.num_cols,) + tail, dt, 20 + seed)

    def run(x, y):
        return (voltrix.sddmm(p.indptr, p.indices, x, y),)

    def check(operands, outputs):
        x, y = (t.double() for t in operands)
        products = x[p.rows] * y[p.cols]
        within(outputs[0], products.sum(-1), tail[-1] * U * products.abs().sum(-1), f"sddmm {_id(shape)}")

    return Case(run, make, check)


def _spmm_heads(shape, heads):
    import voltrix

    p, dt, dim = pattern(shape.pattern), DT[shape.dtype], shape.tail[-1]

    def make(seed):
        return randn((p.nnz, heads), torch.float32, 30 + seed), randn((p.num_cols, heads, dim), dt, 40 + seed)

    def run(values, feat):
        return (voltrix.spmm_heads(p.indptr, p.indices, values, feat, p.num_rows),)

    def check(operands, outputs):
        values, feat = (t.double() for t in operands)
        terms = values[:, :, None] * feat[p.cols]
        within(outputs[0], row_sum(p, terms), p.deg[:, None, None] * U * row_sum(p, terms.abs()), f"spmm_heads H={heads} {_id(shape)}")

    return Case(run, make, check)


def _csr_values_product(shape):
    from voltrix.sddmm import csr_values_product

    p, dt, dim = pattern(shape.pattern), DT[shape.dtype], shape.tail[-1]

    def make(seed):
        return randn((p.nnz,), torch.float32, 50 + seed), randn((p.num_cols, dim), dt, 60 + seed)

    def run(values, feat):
        return (csr_values_product(p.indptr, p.indices, values, p.num_rows, feat),)

    def check(operands, outputs):
        values, feat = (t.double() for t in operands)
        terms = values[:, None] * feat[p.cols]
        within(outputs[0], row_sum(p, terms), p.deg[:, None] * U * row_sum(p, terms.abs()), f"csr_values_product {_id(shape)}")

    return Case(run, make, check)


# ---- spmm_reduce with both backwards
def _spmm_reduce(shape):
    import spmm_multi_oracle
    import voltrix
    from voltrix.spmm_reduce import row_degrees, spmm_mean_backward, spmm_reduce_backward

    p, dt, tail = pattern(shape.pattern), DT[shape.dtype], shape.tail

    def make(seed):
        return randn((p.num_cols,) + tail, dt, 70 + seed), randn((p.num_rows,) + tail, torch.float32, 80 + seed)

    def run(feat, grad):
        results = []
        for reduce in ("max", "min"):
            out, arg = voltrix.spmm_reduce(p.indptr, p.indices, feat, p.num_rows, reduce=reduce, return_arg=True)
            results += [out, arg, spmm_reduce_backward(p.t_indptr, p.t_indices, p.t_order, grad, arg, p.num_cols)]
        results.append(voltrix.spmm_reduce(p.indptr, p.indices, feat, p.num_rows, reduce="mean"))
        results.append(spmm_mean_backward(p.t_indptr, p.t_indices, grad, row_degrees(p.indptr), p.num_cols))
        return tuple(results)

    def check(operands, outputs):
        feat, grad = operands[0].flatten(1), operands[1].flatten(1).double()
        dim = feat.shape[1]
        lanes = torch.arange(dim, device="cuda")[None, :]
        for k, reduce in enumerate(("max", "min")):
            out, arg, d_feat = (t.flatten(1) for t in outputs[3 * k:3 * k + 3])
            ref, ref_arg = spmm_multi_oracle.select(p.rows, p.cols, feat, p.num_rows, reduce)
            assert torch.equal(out.double(), ref) and torch.equal(arg.long(), ref_arg), (reduce, _id(shape))     # a selection is exact
            won = ref_arg >= 0                                       # the gradient of an element goes to its winner's column
            lin = (p.cols[ref_arg.clamp(min=0)] * dim + lanes)[won]
            flat = lambda v: _zeros(p.num_cols * dim).index_add_(0, lin, v).view(p.num_cols, dim)     # noqa: E731
            count = flat(torch.ones_like(grad[won]))
            within(d_feat, flat(grad[won]), count * U * flat(grad[won].abs()), f"spmm_reduce_backward {reduce} {_id(shape)}")
        mean, d_mean = outputs[6].flatten(1), outputs[7].flatten(1)
        gathered = feat.double()[p.cols]
        deg = p.deg.clamp(min=1)[:, None]
        within(mean, row_sum(p, gathered) / deg, (p.deg[:, None] + 1) * U * row_sum(p, gathered.abs()) / deg, f"mean {_id(shape)}")
        scaled = (grad / deg)[p.rows]
        within(d_mean, col_sum(p, scaled), (p.col_deg[:, None] + 1) * U * col_sum(p, scaled.abs()), f"spmm_mean_backward {_id(shape)}")

    return Case(run, make, check)


# ---- spmm_edge with both gradients
def _spmm_edge(shape, op):
    import spmm_edge_oracle
    import voltrix

    p, dt, tail = pattern(shape.pattern), DT[shape.dtype], shape.tail
    copy = op == "copy"

    def make(seed):
        operands = (randn((p.num_cols,) + tail, dt, 90 + seed), randn((p.nnz,) + tail, dt, 100 + seed),
                    randn((p.num_rows,) + tail, torch.float32, 110 + seed))
        return operands[1:] if copy else operands

    def run(*operands):
        feat, efeat, grad = (None,) + operands if copy else operands
        results = [voltrix.spmm_edge(p.indptr, p.indices, feat, efeat, p.num_rows, op=op),
                   voltrix.spmm_edge.grad_efeat(p.indptr, p.indices, grad, feat, efeat, op)]
        if not copy:
            results.append(voltrix.spmm_edge.grad_feat(p.t_indptr, p.t_indices, p.t_order, grad, feat, efeat, op, p.num_cols))
        return tuple(results)

    def check(operands, outputs):
        feat, efeat, grad = (None,) + operands if copy else operands
        feat = None if feat is None else _np(feat.flatten(1))
        efeat, grad = _np(efeat.flatten(1)), _np(grad.flatten(1))
        ref, mass, count = spmm_edge_oracle.forward(p.ip, p.ix, feat, efeat, op)
        within(outputs[0].flatten(1), ref, (count[:, None] + 1) * U * mass, f"spmm_edge {op} {_id(shape)}")
        ref = spmm_edge_oracle.grad_efeat(p.ip, p.ix, grad, feat, efeat, op)
        within(outputs[1].flatten(1), ref, U * np.abs(ref) if op == "mul" else np.zeros_like(ref), f"grad_efeat {op} {_id(shape)}")
        if not copy:
            ref, mass, count = spmm_edge_oracle.grad_feat(p.ip, p.ix, grad, feat, efeat, op, p.num_cols)
            within(outputs[2].flatten(1), ref, (count[:, None] + 1) * U * mass, f"grad_feat {op} {_id(shape)}")

    return Case(run, make, check)


# ---- spmm_rel with both gradients; coef a tensor [R, B] or the identity given as the number of types
def _spmm_rel(shape, identity):
    import spmm_rel_oracle
    import voltrix

    p, dt, dim = pattern(shape.pattern), DT[shape.dtype], shape.tail[-1]
    bases = NUM_TYPES if identity else NUM_BASES

    def make(seed):
        operands = (randn((p.num_cols, dim), dt, 120 + seed), randn((NUM_TYPES, NUM_BASES), torch.float32, 130 + seed),
                    randn((p.nnz,), torch.float32, 140 + seed).abs() + 0.25, randn((p.num_rows, bases, dim), torch.float32, 150 + seed))
        return (operands[0],) + operands[2:] if identity else operands

    def run(*operands):
        feat, coef, weight, grad = (operands[0], NUM_TYPES) + operands[1:] if identity else operands
        return (voltrix.spmm_rel(p.indptr, p.indices, p.etype, feat, coef, p.num_rows, weight=weight),
                voltrix.spmm_rel.grad_feat(p.t_indptr, p.t_indices, p.t_order, p.etype, grad, coef, p.num_cols, weight=weight),
                voltrix.spmm_rel.grad_coef(p.indptr, p.indices, p.etype, p.type_index, grad, feat, weight=weight))

    def check(operands, outputs):
        feat, coef, weight, grad = (operands[0], torch.eye(NUM_TYPES)) + operands[1:] if identity else operands
        feat, coef, weight, grad = _np(feat), _np(coef), _np(weight), _np(grad)
        what = f"{'identity' if identity else 'coef'} {_id(shape)}"
        ref, mass, count = spmm_rel_oracle.forward(p.ip, p.ix, p.etype_np, feat, coef, weight)
        within(outputs[0], ref, (count[:, None, None] + 2) * U * mass, f"spmm_rel {what}")
        ref, mass, count = spmm_rel_oracle.grad_feat(p.ip, p.ix, p.etype_np, grad, coef, p.num_cols, weight)
        within(outputs[1], ref, (count[:, None] * bases + 2) * U * mass, f"spmm_rel.grad_feat {what}")
        ref, mass, count = spmm_rel_oracle.grad_coef(p.ip, p.ix, p.etype_np, grad, feat, NUM_TYPES, weight)
        within(outputs[2], ref, (count[:, None] + dim + 2) * U * mass, f"spmm_rel.grad_coef {what}")

    return Case(run, make, check)


# ---- quantize_fp8 into spmm_fp8
def _spmm_fp8(shape, scale, with_values, out_name):
    import spmm_fp8_oracle
    import voltrix

    p, dt, dim = pattern(shape.pattern), DT[shape.dtype], shape.tail[-1]
    out_dtype = DT[out_name]

    def make(seed):
        operands = (randn((p.num_cols, dim), dt, 160 + seed, scale=3.0), randn((p.nnz,), torch.float32, 170 + seed))
        return operands if with_values else operands[:1]

    def run(feat, values=None):
        rows = voltrix.quantize_fp8(feat, scale=scale)
        return rows.data, rows.scale, rows.inv_scale, voltrix.spmm_fp8(p.indptr, p.indices, rows, p.num_rows, values=values,
                                                                       out_dtype=out_dtype)

    def check(operands, outputs):
        feat, values = operands[0], (operands[1] if with_values else None)
        data, mult, inv, out = outputs
        width = (dim + 15) // 16 * 16
        assert data.shape == (p.num_cols, width) and mult.shape == inv.shape == (width,) and out.shape == (p.num_rows, dim)
        for got, want in zip((mult, inv), spmm_fp8_oracle.scales(feat, scale)):          # the documented formula where the data lives
            assert same_bits(got[:dim], want.contiguous()) and bool((got[dim:] == 1).all())
        codes = data.view(torch.uint8).cpu()
        assert torch.equal(codes, spmm_fp8_oracle.quantize(feat.cpu(), inv.cpu()[:dim])), "the codes are torch's cast"
        ref, mass, count = spmm_fp8_oracle.aggregate(p.ip, p.ix, codes.numpy(), _np(mult), None if values is None else _np(values))
        bound = (count[:, None] + 2) * U * np.abs(_np(mult)) * mass
        exact = torch.from_numpy(ref[:, :dim]).cuda()
        bound = cast_bound(exact, torch.from_numpy(bound[:, :dim]).cuda(), out_dtype)
        within(out, exact, bound, f"spmm_fp8 {scale} values={with_values} {out_name} {_id(shape)}")

    return Case(run, make, check)


# ---- spmm_multi with its backward
def _multi_weights(p, aggrs, grads, std):
    """``u = g_sum + g_mean / d`` and ``w = 2 g_var / d + g_std / (d std)`` by torch ops, as the backward's caller forms them."""
    from voltrix.spmm_reduce import row_degrees

    g = {name: grads[:, i] for i, name in enumerate(aggrs)}
    deg = row_degrees(p.indptr).view((p.num_rows,) + (1,) * (grads.dim() - 2))
    u = w = None
    if "mean" in g:
        u = g["mean"] / deg
    if "sum" in g:
        u = g["sum"] if u is None else u + g["sum"]
    if "var" in g:
        w = 2.0 * g["var"] / deg
    if "std" in g:
        w = g["std"] / (deg * std) if w is None else w + g["std"] / (deg * std)
    return g, u, w


def _spmm_multi(shape):
    import spmm_multi_oracle
    import voltrix

    p, dt, tail = pattern(shape.pattern), DT[shape.dtype], shape.tail

    def make(seed):
        return randn((p.num_cols,) + tail, dt, 180 + seed), randn((p.num_rows, len(AGGREGATES)) + tail, torch.float32, 190 + seed)

    def run(feat, grads):
        out, state = voltrix.spmm_multi(p.indptr, p.indices, feat, p.num_rows, aggrs=AGGREGATES, eps=EPS, return_state=True)
        g, u, w = _multi_weights(p, AGGREGATES, grads, state.std)
        d_feat = voltrix.spmm_multi.backward(p.t_indptr, p.t_indices, p.t_order, p.num_cols, feat=feat, u=u, w=w, mean=state.mean,
                                             g_max=g["max"], argmax=state.argmax, g_min=g["min"], argmin=state.argmin)
        return out, state.argmax, state.argmin, state.mean, state.std, d_feat

    def check(operands, outputs):
        feat, grads = operands[0].flatten(1), operands[1].flatten(2)
        out, argmax, argmin, mean, std, d_feat = outputs
        got = {name: out.flatten(2)[:, i] for i, name in enumerate(AGGREGATES)}
        ref = spmm_multi_oracle.forward(p.indptr, p.indices, feat, p.num_rows, EPS)
        what = f"spmm_multi {_id(shape)}"
        for name in ("max", "min"):
            assert torch.equal(got[name].double(), ref[name]), (what, name)
        assert torch.equal(argmax.flatten(1).long(), ref["argmax"]) and torch.equal(argmin.flatten(1).long(), ref["argmin"]), what
        mass = ref["abs_mean"] * ref["deg"].clamp(min=1)[:, None]
        within(got["sum"], ref["sum"], ref["deg"][:, None] * U * mass, f"{what} sum")
        within(got["mean"], ref["mean"], (ref["deg"][:, None] + 1) * U * ref["abs_mean"], f"{what} mean")
        within(got["var"], ref["var"], ref["var_bound"], f"{what} var")
        within(got["std"], ref["std"], ref["std_bound"], f"{what} std")
        assert same_bits(mean.flatten(1).contiguous(), got["mean"].contiguous()) and same_bits(std.flatten(1).contiguous(),
                                                                                                 got["std"].contiguous()), what
        want, bound = spmm_multi_oracle.backward(p.indptr, p.indices, feat, p.num_rows,
                                                 {name: grads[:, i] for i, name in enumerate(AGGREGATES)}, EPS)
        within(d_feat.flatten(1), want, bound, f"{what} backward")

    return Case(run, make, check)


# ---- the autograd wrappers: a forward and backward() per run, the wrapper object built beforehand
def _leaf(t):
    return t.detach().requires_grad_(True)


def _wrapper(build, make, functional):
    """A case around ``op = build()``, made before any run: ``run`` calls ``op`` on fresh leaves over the operands' storage and
    ``backward(w)`` with the last operand; ``functional(*operands) -> (out, *grads)`` is the same step through the functional operators
    (checked on their own)."""
    op = build()

    def run(*operands):
        *inputs, w = operands
        leaves = [_leaf(t) for t in inputs]
        out = op.call(*leaves)
        out.backward(w)
        return (out.detach(),) + tuple(leaf.grad for leaf in leaves)

    def check(operands, outputs):
        want = functional(*operands)
        torch.cuda.synchronize()
        assert not differing(outputs, want), (type(op).__name__, differing(outputs, want))

    return Case(run, make, check)


class _Bound:
    """An autograd wrapper with the arguments that are not operands bound."""

    def __init__(self, op, call):
        self.op, self.call = op, call


def _wrap_sddmm(shape):
    import voltrix
    from voltrix.autograd import SDDMM
    from voltrix.sddmm import csr_values_product

    p, dt, tail = pattern(shape.pattern), DT[shape.dtype], shape.tail

    def build():
        op = SDDMM(p.csr)
        return _Bound(op, op)

    def make(seed):
        return (randn((p.num_rows,) + tail, dt, 200 + seed), randn((p.num_cols,) + tail, dt, 210 + seed),
                randn((p.nnz,) + tail[:-1], torch.float32, 220 + seed))

    def functional(x, y, w):
        out = voltrix.sddmm(p.indptr, p.indices, x, y)
        if len(tail) == 2:
            return (out, voltrix.spmm_heads(p.indptr, p.indices, w, y, p.num_rows).to(dt),
                    voltrix.spmm_heads(p.t_indptr, p.t_indices, w[p.t_order.long()], x, p.num_cols).to(dt))
        return (out, csr_values_product(p.indptr, p.indices, w, p.num_rows, y).to(dt),
                csr_values_product(p.t_indptr, p.t_indices, w[p.t_order.long()], p.num_cols, x).to(dt))

    return _wrapper(build, make, functional)


def _wrap_spmm_heads(shape):
    import voltrix
    from voltrix.autograd import SpMMHeads

    p, dt, (heads, dim) = pattern(shape.pattern), DT[shape.dtype], shape.tail

    def build():
        op = SpMMHeads(p.csr)
        return _Bound(op, op)

    def make(seed):
        return (randn((p.num_cols, heads, dim), dt, 230 + seed), randn((p.nnz, heads), torch.float32, 240 + seed),
                randn((p.num_rows, heads, dim), torch.float32, 250 + seed))

    def functional(feat, values, w):
        return (voltrix.spmm_heads(p.indptr, p.indices, values, feat, p.num_rows),
                voltrix.spmm_heads(p.t_indptr, p.t_indices, values[p.t_order.long()], w, p.num_cols).to(dt),
                voltrix.sddmm(p.indptr, p.indices, w, feat))

    return _wrapper(build, make, functional)


def _wrap_spmm_reduce(shape, reduce):
    import voltrix
    from voltrix.autograd import SpMMReduce
    from voltrix.spmm_reduce import row_degrees, spmm_mean_backward, spmm_reduce_backward

    p, dt, tail = pattern(shape.pattern), DT[shape.dtype], shape.tail

    def build():
        op = SpMMReduce(p.csr, reduce=reduce)
        return _Bound(op, op)

    def make(seed):
        return randn((p.num_cols,) + tail, dt, 260 + seed), randn((p.num_rows,) + tail, torch.float32, 270 + seed)

    def functional(feat, w):
        if reduce == "mean":
            return (voltrix.spmm_reduce(p.indptr, p.indices, feat, p.num_rows, "mean"),
                    spmm_mean_backward(p.t_indptr, p.t_indices, w, row_degrees(p.indptr), p.num_cols).to(dt))
        out, arg = voltrix.spmm_reduce(p.indptr, p.indices, feat, p.num_rows, reduce, return_arg=True)
        return out, spmm_reduce_backward(p.t_indptr, p.t_indices, p.t_order, w, arg, p.num_cols).to(dt)

    return _wrapper(build, make, functional)


def _wrap_spmm_edge(shape, kind):
    import voltrix
    from voltrix.autograd import SpMMEdge

    p, dt, tail = pattern(shape.pattern), DT[shape.dtype], shape.tail

    def build():
        op = SpMMEdge(p.csr)
        return _Bound(op, lambda feat, efeat: op(feat, efeat, op=kind))

    def make(seed):
        return (randn((p.num_cols,) + tail, dt, 280 + seed), randn((p.nnz,) + tail, dt, 290 + seed),
                randn((p.num_rows,) + tail, torch.float32, 300 + seed))

    def functional(feat, efeat, w):
        return (voltrix.spmm_edge(p.indptr, p.indices, feat, efeat, p.num_rows, op=kind),
                voltrix.spmm_edge.grad_feat(p.t_indptr, p.t_indices, p.t_order, w, feat, efeat, kind, p.num_cols).to(dt),
                voltrix.spmm_edge.grad_efeat(p.indptr, p.indices, w, feat, efeat, kind).to(dt))

    return _wrapper(build, make, functional)


def _wrap_spmm_rel(shape):
    import voltrix
    from voltrix.autograd import SpMMRel

    p, dt, dim = pattern(shape.pattern), DT[shape.dtype], shape.tail[-1]
    weight = randn((p.nnz,), torch.float32, 310).abs() + 0.25          # the degree normaliser: a constant of the graph

    def build():
        op = SpMMRel(p.csr, etype=p.etype, num_types=NUM_TYPES)
        return _Bound(op, lambda feat, coef: op(feat, coef, weight))

    def make(seed):
        return (randn((p.num_cols, dim), dt, 320 + seed), randn((NUM_TYPES, NUM_BASES), torch.float32, 330 + seed),
                randn((p.num_rows, NUM_BASES, dim), torch.float32, 340 + seed))

    def functional(feat, coef, w):
        return (voltrix.spmm_rel(p.indptr, p.indices, p.etype, feat, coef, p.num_rows, weight=weight),
                voltrix.spmm_rel.grad_feat(p.t_indptr, p.t_indices, p.t_order, p.etype, w, coef, p.num_cols, weight=weight).to(dt),
                voltrix.spmm_rel.grad_coef(p.indptr, p.indices, p.etype, p.type_index, w, feat, weight=weight))

    return _wrapper(build, make, functional)


def _wrap_spmm_fp8(shape):
    import voltrix
    from voltrix.autograd import SpMMFp8
    from voltrix.sddmm import csr_values_product

    p, dt, dim = pattern(shape.pattern), DT[shape.dtype], shape.tail[-1]
    values = randn((p.nnz,), torch.float32, 350)                         # a constant of the graph: no gradient

    def build():
        op = SpMMFp8(p.csr)
        return _Bound(op, lambda feat: op(feat, values))

    def make(seed):
        return randn((p.num_cols, dim), dt, 360 + seed, scale=3.0), randn((p.num_rows, dim), torch.float32, 370 + seed)

    def functional(feat, w):                                            # straight-through: csr(values)^T w
        out = voltrix.spmm_fp8(p.indptr, p.indices, voltrix.quantize_fp8(feat), p.num_rows, values=values)
        return out, csr_values_product(p.t_indptr, p.t_indices, values[p.t_order.long()], p.num_cols, w).to(dt)

    return _wrapper(build, make, functional)


def _wrap_spmm_multi(shape):
    import voltrix
    from voltrix.autograd import SpMMMulti

    p, dt, tail = pattern(shape.pattern), DT[shape.dtype], shape.tail

    def build():
        op = SpMMMulti(p.csr, aggrs=PNA, eps=EPS)
        return _Bound(op, op)

    def make(seed):
        return randn((p.num_cols,) + tail, dt, 380 + seed), randn((p.num_rows, len(PNA)) + tail, torch.float32, 390 + seed)

    def functional(feat, w):
        out, state = voltrix.spmm_multi(p.indptr, p.indices, feat, p.num_rows, aggrs=PNA, eps=EPS, return_state=True)
        g, u, weights = _multi_weights(p, PNA, w, state.std)
        return out, voltrix.spmm_multi.backward(p.t_indptr, p.t_indices, p.t_order, p.num_cols, feat=feat, u=u, w=weights,
                                                mean=state.mean, g_max=g["max"], argmax=state.argmax, g_min=g["min"],
                                                argmin=state.argmin).to(dt)

    return _wrapper(build, make, functional)


# ---- the samplers: the id list is the late operand, the seed is fixed
def ids(count, high, seed, distinct=False):
    rng = np.random.default_rng(seed)
    picked = rng.permutation(high)[:count] if distinct else rng.integers(0, high, count)
    return torch.from_numpy(picked.astype(np.int32)).cuda()


def _sampler(run, count, distinct=False, sync_free=False, check=None, lists=1):
    """A sampler over ``lists`` id lists of ``count`` ids of the square pattern; the prefill is another draw of in-range ids."""
    n = pattern("skewed").num_rows

    def make(seed):
        return tuple(ids(count, n, 400 + 10 * seed + k, distinct) for k in range(lists))

    def prefill():
        return [ids(count, n, 450 + k, distinct) for k in range(lists)]

    return Case(run, make, check, prefill, sync_free)


def _sample_neighbors(kind):
    import voltrix

    p = pattern("skewed")
    extra = {}
    if kind == "exclude":          # every third entry, strictly ascending
        extra["exclude"] = torch.arange(0, p.nnz, 3, dtype=torch.int32, device="cuda")
    if kind == "prob":
        extra["prob"] = voltrix.sampling_weights(p.indptr, randn((p.nnz,), torch.float32, 401).abs())
    return _sampler(lambda seeds: tuple(voltrix.sample_neighbors(p.indptr, p.indices, seeds, 3, seed=11, **extra)), 64)


def _compact_block():
    from voltrix.sampling import compact_block

    p = pattern("skewed")
    return _sampler(lambda seeds, sampled: tuple(compact_block(seeds, sampled, p.num_cols)), 50, distinct=True, lists=2)


def _induced_subgraph():
    import voltrix

    p = pattern("skewed")

    def run(nodes):
        sub = voltrix.induced_subgraph(p.indptr, p.indices, nodes)
        csr = sub.pattern
        return csr.indptr, csr.indices, csr.t_indptr, csr.t_indices, csr.t_order, sub.entries

    return _sampler(run, 300, distinct=True)


def _random_walk():
    import voltrix

    p = pattern("skewed")
    return _sampler(lambda starts: tuple(voltrix.random_walk(p.indptr, p.indices, starts, 4, seed=13)), 64)


def _negative_sample():
    import voltrix

    p = pattern("skewed")

    def run(src):
        neg, exhausted = voltrix.negative_sample(p.indptr, p.indices, src, 4, seed=17, assume_sorted=p.sorted_rows)
        return neg, torch.tensor([exhausted])

    return _sampler(run, 64)


def _find_edges():
    import voltrix

    p = pattern("skewed")

    def run(rows, cols):
        return (voltrix.find_edges(p.indptr, p.indices, rows, cols, assume_sorted=p.sorted_rows),)

    def check(operands, outputs):
        rows, cols = (t.cpu().numpy() for t in operands)
        want = []
        for r, c in zip(rows, cols):
            hits = np.flatnonzero(p.ix[p.ip[r]:p.ip[r + 1]] == c)
            want.append(p.ip[r] + hits[0] if hits.size else -1)
        assert np.array_equal(outputs[0].cpu().numpy(), np.asarray(want)) and (np.asarray(want) >= 0).sum() >= 32

    def make(seed):          # half of the pairs are entries of the pattern, half are random (most of them no entry)
        picked = ids(64, p.nnz, 460 + seed).long()
        rows = torch.cat([p.rows[picked].int(), ids(64, p.num_rows, 470 + seed)])
        cols = torch.cat([p.cols[picked].int(), ids(64, p.num_cols, 480 + seed)])
        return rows, cols

    def prefill():
        return [ids(128, p.num_rows, 490), ids(128, p.num_cols, 491)]

    return Case(run, make, check, prefill, sync_free=True)


def _register_all():
    part = functools.partial
    for shape in (WHOLE, PADDED, HEADS, WIDE_HEADS):
        _register(f"sddmm-{_id(shape)}", part(_sddmm, shape))
    for shape in (HEADS, WIDE_HEADS):
        for heads in (1, 3):
            _register(f"spmm_heads-H{heads}-{_id(shape)}", part(_spmm_heads, shape, heads))
    for shape in (WHOLE, PADDED):
        _register(f"csr_values_product-{_id(shape)}", part(_csr_values_product, shape))
    for shape in (WHOLE, PADDED, HEADS):
        _register(f"spmm_reduce-{_id(shape)}", part(_spmm_reduce, shape))
        for op in ("mul", "add", "add_relu", "copy"):
            _register(f"spmm_edge-{op}-{_id(shape)}", part(_spmm_edge, shape, op))
        _register(f"spmm_multi-{_id(shape)}", part(_spmm_multi, shape))
    for shape in (WHOLE, PADDED):
        for identity in (False, True):
            _register(f"spmm_rel-{'identity' if identity else 'coef'}-{_id(shape)}", part(_spmm_rel, shape, identity))
        for scale in ("column", "tensor"):
            for with_values in (False, True):
                for out_name in ("fp32", "bf16"):
                    _register(f"spmm_fp8-{scale}-{'values' if with_values else 'ones'}-{out_name}-{_id(shape)}",
                              part(_spmm_fp8, shape, scale, with_values, out_name))
    for shape in (WHOLE, PADDED, HEADS):
        _register(f"SDDMM-{_id(shape)}", part(_wrap_sddmm, shape))
    _register(f"SpMMHeads-{_id(HEADS)}", part(_wrap_spmm_heads, HEADS))
    for shape in (WHOLE, PADDED):
        for reduce in ("max", "mean"):
            _register(f"SpMMReduce-{reduce}-{_id(shape)}", part(_wrap_spmm_reduce, shape, reduce))
        for kind in ("mul", "add_relu"):
            _register(f"SpMMEdge-{kind}-{_id(shape)}", part(_wrap_spmm_edge, shape, kind))
        _register(f"SpMMRel-{_id(shape)}", part(_wrap_spmm_rel, shape))
        _register(f"SpMMFp8-{_id(shape)}", part(_wrap_spmm_fp8, shape))
        _register(f"SpMMMulti-{_id(shape)}", part(_wrap_spmm_multi, shape))
    for kind in ("plain", "exclude", "prob"):
        _register(f"sample_neighbors-{kind}", part(_sample_neighbors, kind), sync_free=False)
    _register("compact_block", _compact_block, sync_free=False)
    _register("induced_subgraph", _induced_subgraph, sync_free=False)
    _register("random_walk", _random_walk, sync_free=False)
    _register("negative_sample", _negative_sample, sync_free=False)
    _register("find_edges", _find_edges)


_register_all()
