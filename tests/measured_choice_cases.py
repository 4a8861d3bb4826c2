"""The graphs, oracles and bounds of tests/test_gpu_measured_choices.py.

The contract under test: how ``voltrix.spmm`` rounds B is a function of (handle, width, dtype, environment), never of a clock, of an
entry in the tuned store or of stream-capture state; a measured choice only picks between candidates that differ by fp32 summation
order.  Two graphs on which a handle keeps its CSR side-car -- so that the CSR row-gather kernel and the block format are both there --
one in each class of ``fp32_mode``:

    G_exact   n = 1000, 4 distinct uniformly random columns per row, every 97th row empty: about 8 TC blocks per window, 4 gathered rows of
              B per output row -> fp32 features are multiplied as they are ("exact") at every width
    G_cast    the same with 20 columns per row: about 35 TC blocks per window (side-car limit: 48), 17.4 gathered rows per output row ->
              fp32 features are rounded to fp16 behind one scale ("fp16") at every width, the narrow ones (limit 16) included

n = 1000 leaves a row tail of 8 in the last window.  The tests assert these preconditions on the handles themselves.

Every reference is a float64 ``torch.sparse`` product on the CPU, computed once per (graph, width, dtype), shared and never written.
Bounds, element-wise, with deg the entries of the row and u = 2^-23:

    csr      (deg + 1) u (A |B'|)        against the oracle on B', the operand the class prescribes (B as given; class "fp16": fp16(B))
    block    (deg + 16) u (A |B'|)       the same, plus against the oracle on B itself the cast term of tests/test_gpu_spmm.py:
                                         (2^-11 + (deg + 16) u) (A |B|) + deg 2^-25
    pair     (2 deg + 17) u (A |B|)      |out_csr - out_block|: the sum of the two accumulation bounds and NO rounding of B -- an fp16
                                         rounded operand on one side puts nine elements in ten outside it, by up to 30-40 x
"""
import functools
import sys

import numpy as np
import torch

from oracle import torch_ref

U = 2.0 ** -23
N = 1000
WIDTHS = (8, 40, 128, 200)          # narrow; padded to 8 (16-bit) or to 4 (exact fp32); one slab; a padded width of several pieces
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
PER_ROW = {"G_exact": 4, "G_cast": 20}
CLASS = {"G_exact": "exact", "G_cast": "fp16"}


def operator_module():
    """``voltrix/spmm/spmm.py`` (the package attribute ``voltrix.spmm`` is the function)."""
    import voltrix  # noqa: F401

    return sys.modules["voltrix.spmm.spmm"]


@functools.lru_cache(maxsize=None)
def graph(name):
    """``(indptr int32 [N + 1], indices int32 [nnz])`` as numpy arrays: sorted distinct columns, every 97th row empty."""
    rng = np.random.default_rng({"G_exact": 4, "G_cast": 20}[name])
    rows = [np.sort(rng.choice(N, PER_ROW[name], replace=False)) if r % 97 else np.zeros(0, np.int64) for r in range(N)]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return indptr, np.concatenate(rows).astype(np.int32)


def degrees(name):
    return torch.from_numpy(np.diff(graph(name)[0]).astype(np.float64))[:, None]


def adjacency(name, values=None):
    indptr, indices = graph(name)
    values = torch.ones(len(indices), dtype=torch.float64) if values is None else values.double()
    return torch.sparse_csr_tensor(torch.from_numpy(indptr), torch.from_numpy(indices), values, size=(N, N))


def features(width, dtype, seed=0):
    """``randn`` [N, width] in ``dtype`` on the CPU."""
    gen = torch.Generator().manual_seed(1000 * seed + width)
    return torch.randn(N, width, generator=gen).to(DT[dtype])


def class_operand(name, feat):
    """The operand the class of (graph, dtype) prescribes, in float64: the features as given, or -- fp32 features on G_cast -- what the
    scaled cast makes of them."""
    if feat.dtype == torch.float32 and CLASS[name] == "fp16":
        return torch_ref.round_fp16_scaled(feat).double()
    return feat.double()


class Reference:
    """float64 products of one (graph, width, dtype, seed): ``given`` = A B and ``mass`` = A |B| on the features as given, ``same`` and
    ``same_mass`` on the class's operand."""

    def __init__(self, name, feat):
        a = adjacency(name)
        self.deg = degrees(name)
        self.given, self.mass = a @ feat.double(), a @ feat.double().abs()
        rounded = class_operand(name, feat)
        self.cast = not torch.equal(rounded, feat.double())
        self.same, self.same_mass = (a @ rounded, a @ rounded.abs()) if self.cast else (self.given, self.mass)


@functools.lru_cache(maxsize=None)
def reference(name, width, dtype, seed=0):
    return Reference(name, features(width, dtype, seed))


def ratio(err, bound):
    """max err / bound over the elements with a bound; elements whose bound is 0 (empty rows) must be exact."""
    assert bool((err[bound == 0] == 0).all())
    return float((err / bound.clamp_min(1e-300)).max())


def check_csr(out, ref, what):
    """The CSR kernel's class bound."""
    out = out.cpu().double()
    assert not torch.isnan(out).any(), what
    worst = ratio((out - ref.same).abs(), (ref.deg + 1) * U * ref.same_mass)
    print(f"{what}: csr max err / bound = {worst:.3f}")
    assert worst <= 1.0, (what, worst)


def check_block(out, ref, what):
    """The block format's class bound: accumulation on the class's operand, and the cast term against the features as given."""
    out = out.cpu().double()
    assert not torch.isnan(out).any(), what
    worst = ratio((out - ref.same).abs(), (ref.deg + 16) * U * ref.same_mass)
    print(f"{what}: block max err / bound = {worst:.3f}")
    assert worst <= 1.0, (what, worst)
    if ref.cast:
        bound = (2.0 ** -11 + (ref.deg + 16) * U) * ref.mass + ref.deg * 2.0 ** -25
        assert bool(((out - ref.given).abs() <= bound).all()), what


def check_pair(first, second, ref, what):
    """Two outcomes of one choice: fp32 summation order apart, no rounding of B between them."""
    worst = ratio((first.cpu().double() - second.cpu().double()).abs(), (2 * ref.deg + 17) * U * ref.mass)
    print(f"{what}: pair max diff / bound = {worst:.3f}")
    assert worst <= 1.0, (what, worst)


def check_outcome(outcome, out, ref, what):
    (check_csr if outcome == "csr" else check_block)(out, ref, f"{what} {outcome}")


class Stopwatch:
    """A scripted replacement of the operators' one stopwatch (``voltrix/spmm/spmm.py::_time_ms``): every candidate still runs once, so
    that what it raises is raised and what it tunes is tuned, and its "time" is the script's entry for its label.  ``calls`` lists the
    labels timed so far; ``during`` (a callable) runs inside the first timing, after the candidate."""

    def __init__(self, script, during=None):
        self.script, self.calls, self.during = dict(script), [], during

    def __call__(self, fn, warmup=2, reps=3, label=""):
        self.calls.append(label)
        fn()
        if self.during is not None:
            during, self.during = self.during, None
            during()
        return float(self.script[label])
