"""GPU: every operator on offset, strided, permuted and stride-0 views of its operands, on caller-provided outputs between guard
words, and with gradients that arrive as views.

Every other GPU test hands the kernels freshly allocated tensors: contiguous, their first byte aligned to 256 bytes or more.  This module
owns the layouts; the per-operator files own the numerics.

Oracle: BIT EQUALITY with the call on ``.clone()``s of the same values.  No tolerance: every kernel's reduction order is fixed by the
pattern and not by an address, the 4-byte and the 16-byte load / store paths move the same values, and ``gat_score_kernel<0>`` does the
same two rounded operations per element as ``<4>`` / ``<8>``.  No path turned out to differ.  Once per operator the aligned result is
also held against that operator's own float64 oracle and bound (imported from its test file), so that two equally wrong results cannot
pass.

Which case reaches which branch that no other test reaches (each can only give the aligned call's bits by executing it):
* edge softmax, 4-byte loads in ``edge_softmax_chunk_kernel``: ``test_edge_softmax`` with ``scores`` as ``flat+1`` (``out`` is fresh);
* edge softmax, 4-byte stores with ``all_done`` true: ``test_guarded_outputs_four_byte[edge_softmax]`` at ``k = 1`` (the rows of chunk 0);
* ``gat_score_kernel<0>`` standing in for ``<4>`` / ``<8>``: ``test_gat_score[4]`` / ``[8]`` with ``el`` as ``flat+1``;
* ``gs_load_ints``' one-by-one branch with ``nk == 8``: every ``test_gat_score`` call but the aligned one (``indices`` / ``order`` go in as
  ``flat+1``); its 16-byte branch stays with the aligned call;
* the Python layer's copy: ``test_an_aligned_operand_is_never_copied_a_misaligned_one_always``.
"""
import functools
import sys

import numpy as np
import pytest
import torch

import test_gpu_edge_softmax as t_softmax
import test_gpu_gat_score as t_gat
import test_gpu_gatv2 as t_gatv2
import test_gpu_heads as t_heads
import test_gpu_sddmm as t_sddmm
import test_gpu_weighted as t_weighted
import voltrix
from conftest import load_csr_fixture
from voltrix import capi, sidecar, weighted
from voltrix.capi import VoltrixError
from voltrix.edge_softmax import edge_softmax_backward
from voltrix.gat_score import gat_score_backward
from voltrix.gatv2_score import gatv2_rowsum
from voltrix.sddmm import csr_values_product

pytestmark = pytest.mark.gpu

CHUNK = 2048                 # kChunkEdges: edges per workgroup of the edge softmax and of both gat_score kernels
GUARD = 64                   # floats on either side of a guarded output
SENTINEL = 0x7FC0DEAD        # a quiet NaN no kernel produces
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x), _bits(y))


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------
def _flat(t, k):
    """The values of ``t`` at element offset ``k`` of a flat buffer: contiguous, its first byte off the 16-byte grid."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == (k * t.element_size()) % 16 != 0
    return v


def _expanded(t):
    """Stride 0 in every dimension (what ``.sum()``'s backward hands on): only for a tensor that holds one value everywhere."""
    assert bool((t == t.flatten()[0]).all())
    v = t.flatten()[0].expand(tuple(t.shape))
    assert set(v.stride()) == {0}
    return v


def views(t):
    """(name, view) pairs: the values of ``t`` in layouts no fresh allocation has."""
    for k in ((1, 2, 3) if t.element_size() == 4 else (1, 4)):          # 2-byte types: 2- and 8-byte alignment
        yield f"flat+{k}", _flat(t, k)
    shape = tuple(t.shape)
    if t.dim() >= 2:
        big = torch.empty(shape[:-1] + (shape[-1] + 3,), dtype=t.dtype, device=t.device)
        v = big[..., 1:1 + shape[-1]]
        v.copy_(t)
        assert not v.is_contiguous()
        yield "cols", v                                                  # a column block of a wider tensor: strided rows
        big = torch.empty((shape[0] + 1,) + shape[1:], dtype=t.dtype, device=t.device)
        big[1:].copy_(t)
        yield "rows+1", big[1:]                                          # the second piece of a torch.cat along the edges / nodes
    big = torch.empty((2 * shape[0],) + shape[1:], dtype=t.dtype, device=t.device)
    v = big[::2]
    v.copy_(t)
    yield "step", v
    if t.dim() == 3:
        big = torch.empty((shape[1], shape[0], shape[2]), dtype=t.dtype, device=t.device)
        v = big.permute(1, 0, 2)
        v.copy_(t)
        yield "perm", v                                                  # stored [H, n, D]


def _tuple(r):
    return r if isinstance(r, tuple) else (r,)


def _sweep(fn, floats, ints, constant=()):
    """``fn(**floats, **ints)`` with every float operand in every layout, one at a time, then all of them (and always all int operands)
    as ``flat+1`` at once: the bits of the call on clones.  ``constant``: operands that also go in with one value everywhere, through
    a stride-0 view.  Returns the aligned call's result(s)."""
    clones = lambda d: {k: v.clone() for k, v in d.items()}                         # noqa: E731
    aligned = _tuple(fn(**clones(floats), **clones(ints)))
    off = {k: _flat(v, 1) for k, v in ints.items()}                                # 4-byte aligned, off 16: the kernels' scalar loads
    for name, t in floats.items():
        for label, v in views(t):
            got = _tuple(fn(**{**clones(floats), name: v}, **off))
            assert all(_same_bits(a, b) for a, b in zip(got, aligned)), (name, label)
    got = _tuple(fn(**{k: _flat(v, 1) for k, v in floats.items()}, **off))
    assert all(_same_bits(a, b) for a, b in zip(got, aligned)), "every operand flat+1"
    for name in constant:
        c = torch.full_like(floats[name], 0.75)
        want = _tuple(fn(**{**clones(floats), name: c.clone()}, **clones(ints)))
        got = _tuple(fn(**{**clones(floats), name: _expanded(c)}, **off))
        assert all(_same_bits(a, b) for a, b in zip(got, want)), (name, "expand")
    return aligned if len(aligned) > 1 else aligned[0]


# ---- patterns --------------------------------------------------------------------------------------------------------------------------
def chunk_pattern():
    """(lengths, cols, num_cols) for the 2,048-edge-chunk kernels: about 3 1/2 chunks.  Chunk 0 holds a row of 300 edges wholly inside it
    between short rows and two empty rows in a row (threads whose eight edges all finish in the chunk: ``all_done``); one row crosses the
    chunk 0 / 1 boundary; one row of 4,100 edges spans chunks 1, 2 and 3; the last row has one edge and ``nnz % 8 == 5``, so the last
    thread of the last chunk is partial.  500 columns, one of them a hub."""
    rng = np.random.default_rng(11)
    lengths = [3, 1, 300, 2, 0, 0, 5]
    while sum(lengths) < 1990:
        lengths.append(int(rng.integers(1, 9)))
    crossing = len(lengths)
    lengths.append(CHUNK + 60 - sum(lengths))
    lengths.append(4100)
    while sum(lengths) < 6990:
        lengths.append(int(rng.integers(0, 9)))
    while (sum(lengths) + 1) % 8 != 5:
        lengths.append(1)
    lengths.append(1)
    lengths = np.asarray(lengths, np.int64)
    ip = np.concatenate([[0], np.cumsum(lengths)])
    nnz = int(ip[-1])
    assert ip[3] < CHUNK and lengths[2] == 300 and lengths[1] == 1 and lengths[3] == 2          # wholly inside chunk 0, short neighbours
    assert ip[crossing] < CHUNK < ip[crossing + 1]                                              # crosses the chunk 0 / 1 boundary
    assert lengths[crossing + 1] > CHUNK and ip[crossing + 2] // CHUNK - ip[crossing + 1] // CHUNK == 2      # spans three chunks
    assert lengths[4] == lengths[5] == 0 and lengths[-1] == 1 and nnz % 8 == 5 and 3 * CHUNK < nnz < 4 * CHUNK
    cols = rng.integers(0, 500, nnz)
    cols[rng.choice(nnz, 700, replace=False)] = 7
    return lengths, cols, 500


@functools.lru_cache(maxsize=None)
def _chunk_graph():
    return t_gat._Graph(*chunk_pattern())


@functools.lru_cache(maxsize=None)
def _special():
    """tests/test_gpu_gatv2.py's pattern (3,000 rows, 12,000 edges) for the 128-edge-chunk and row-per-lane-group kernels."""
    g = t_gatv2._special()
    assert g.nnz % 4 != 0 and g.num_rows % 32 != 0        # the last batch of four edges / the last group of rows is partial
    return g


def _randn(shape, dtype=torch.float32, seed=0):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, device="cuda", generator=gen).to(dtype)


# ---- A. inputs through the public Python API -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,pair", [((64,), ("fp16", "fp16")), ((64,), ("fp32", "fp32")), ((4, 16), ("fp16", "fp16")),
                                        ((3, 20), ("fp32", "fp32")), ((3, 13), ("fp16", "fp16"))])
def test_sddmm(cuda_device, shape, pair):
    """2-D and multi-head; (3, 13) is padded per head by the Python layer: the view goes in before the pad."""
    g = _special()
    x, y = _randn((g.num_rows,) + shape, DT[pair[0]], 1), _randn((g.num_cols,) + shape, DT[pair[1]], 2)
    out = _sweep(lambda x, y, indptr, indices: voltrix.sddmm(indptr, indices, x, y), dict(x=x, y=y),
                 dict(indptr=g.indptr, indices=g.indices))
    if len(shape) == 1:
        t_sddmm._check(g.indptr, g.indices, x, y, out, False)
    else:
        t_heads._check_sddmm(g.indptr, g.indices, x, y, out, False, single_head_bits=False)


@pytest.mark.parametrize("heads", [None, 3, 4, 8])
def test_edge_softmax(cuda_device, heads):
    """Forward and backward, 1-D and [nnz, H].  ``scores`` as ``flat+1`` with a fresh ``out`` is the case that takes the 4-byte loads of
    ``edge_softmax_chunk_kernel``; H = 3 as ``rows+1`` is the second graph of a batch."""
    g = _chunk_graph()
    shape = (g.nnz,) if heads is None else (g.nnz, heads)
    scores, grad = _randn(shape, seed=3) * 4, _randn(shape, seed=4)
    alpha = _sweep(lambda scores, indptr: voltrix.edge_softmax(indptr, scores, 0.5), dict(scores=scores), dict(indptr=g.indptr))
    back = _sweep(lambda alpha, grad, indptr: edge_softmax_backward(indptr, alpha, grad, 0.5), dict(alpha=alpha, grad=grad),
                  dict(indptr=g.indptr), constant=("grad",))
    checks = t_softmax if heads is None else t_heads
    checks._check_forward(g.indptr, scores, 0.5, alpha)
    checks._check_backward(g.indptr, alpha, grad, 0.5, back)


@pytest.mark.parametrize("heads", [1, 3, 4, 8])
def test_gat_score(cuda_device, heads):
    """Forward and both segment sums (with and without ``order``).  H = 4 / 8 with ``el`` off the 16-byte grid run ``gat_score_kernel<0>``
    and must give the bits of ``<4>`` / ``<8>``, which the aligned call runs; ``indices`` and ``order`` as ``flat+1`` take ``gs_load_ints``'
    one-by-one branch in every thread with eight edges."""
    g = _chunk_graph()
    el, er, grad = _randn((g.num_rows, heads), seed=5), _randn((g.num_cols, heads), seed=6), _randn((g.nnz, heads), seed=7)
    s = _sweep(lambda el, er, indptr, indices: voltrix.gat_score(indptr, indices, el, er, 0.2), dict(el=el, er=er),
               dict(indptr=g.indptr, indices=g.indices))
    d_el = _sweep(lambda a, b, grad, indptr, indices: gat_score_backward(indptr, indices, a, b, grad, 0.2), dict(a=el, b=er, grad=grad),
                  dict(indptr=g.indptr, indices=g.indices), constant=("grad",))
    d_er = _sweep(lambda a, b, grad, indptr, indices, order: gat_score_backward(indptr, indices, a, b, grad, 0.2, order=order),
                  dict(a=er, b=el, grad=grad), dict(indptr=g.t_indptr, indices=g.t_indices, order=g.t_order), constant=("grad",))
    ref, bound, (r_el, b_el), (r_er, b_er), _ = t_gat._oracle(g, el, er, 0.2, grad)
    t_gat._within(s, ref, bound, f"views: gat_score H={heads}")
    t_gat._within(d_el, r_el, b_el, f"views: d_el H={heads}")
    t_gat._within(d_er, r_er, b_er, f"views: d_er H={heads}")


@pytest.mark.parametrize("heads,dim,dtype", [(4, 16, "fp16"), (3, 20, "fp32"), (2, 520, "fp16")])
def test_gatv2_score_and_rowsum(cuda_device, heads, dim, dtype):
    """``a`` is read 16 bytes at a time and the launcher rejects any other base: as ``flat+k`` (a parameter inside a flat buffer) it is
    the Python layer's copy that makes the call work."""
    g = _special()
    xl, xr = _randn((g.num_rows, heads, dim), DT[dtype], 8), _randn((g.num_cols, heads, dim), DT[dtype], 9)
    a, grad = _randn((heads, dim), seed=10), _randn((g.nnz, heads), seed=11)
    s = _sweep(lambda xl, xr, a, indptr, indices: voltrix.gatv2_score(indptr, indices, xl, xr, a, 0.2), dict(xl=xl, xr=xr, a=a),
               dict(indptr=g.indptr, indices=g.indices))
    big_l = _sweep(lambda p, q, grad, indptr, indices: gatv2_rowsum(indptr, indices, p, q, grad, 0.2), dict(p=xl, q=xr, grad=grad),
                   dict(indptr=g.indptr, indices=g.indices), constant=("grad",))
    big_r = _sweep(lambda p, q, grad, indptr, indices, order: gatv2_rowsum(indptr, indices, p, q, grad, 0.2, order=order),
                   dict(p=xr, q=xl, grad=grad), dict(indptr=g.t_indptr, indices=g.t_indices, order=g.t_order), constant=("grad",))
    (s_ref, s_bound), (l_ref, l_bound), (r_ref, r_bound) = t_gatv2._oracle(g, xl, xr, a, 0.2, grad)
    t_gatv2._within(s, s_ref, s_bound, f"views: gatv2_score H={heads} D={dim} {dtype}")
    t_gatv2._within(big_l, l_ref, l_bound, f"views: G_l H={heads} D={dim} {dtype}")
    t_gatv2._within(big_r, r_ref, r_bound, f"views: G_r H={heads} D={dim} {dtype}")


@pytest.mark.parametrize("heads,dim,dtype", [(4, 16, "fp16"), (8, 8, "bf16"), (1, 64, "fp16")])
def test_spmm_heads_and_csr_values_product(cuda_device, heads, dim, dtype):
    g = _special()
    feat, values = _randn((g.num_cols, heads, dim), DT[dtype], 12), _randn((g.nnz, heads), seed=13)
    out = _sweep(lambda values, feat, indptr, indices: voltrix.spmm_heads(indptr, indices, values, feat, g.num_rows),
                 dict(values=values, feat=feat), dict(indptr=g.indptr, indices=g.indices), constant=("values",))
    t_heads._check_aggregate(g.indptr, g.indices, values, feat, g.num_rows, out, single_head_bits=False)
    feat2, values1 = feat[:, 0].contiguous(), values[:, 0].contiguous()
    out2 = _sweep(lambda values, feat, indptr, indices: csr_values_product(indptr, indices, values, g.num_rows, feat),
                  dict(values=values1, feat=feat2), dict(indptr=g.indptr, indices=g.indices), constant=("values",))
    t_heads._check_aggregate(g.indptr, g.indices, values1[:, None], feat2[:, None], g.num_rows, out2[:, None], single_head_bits=False)


def _skewed():
    g = load_csr_fixture("skewed_1005")
    return g, int(g["num_nodes"]), torch.from_numpy(g["indptr"]), torch.from_numpy(g["indices"])


def _product_bound(g, n, values, feat, unit, extra=1):
    """float64 ``csr(values) @ feat`` from the operand as stored and the bound of tests/test_gpu_weighted.py / test_gpu_csr_path.py:
    ``(unit + (deg + extra) 2^-23) (|A| |B|) + 1e-6`` with ``unit`` the 16-bit roundings of the path (0: exact products) and ``extra``
    the fp32 roundings beside the sum (2 on the separable path: the row factor)."""
    ref = t_weighted._oracle(g["indptr"], g["indices"], values, feat.cpu().float(), n, n)
    absref = t_weighted._oracle(g["indptr"], g["indices"], values.abs(), feat.cpu().float().abs(), n, n)
    deg = torch.from_numpy(np.diff(g["indptr"]).astype(np.float64))[:, None]
    return ref, (unit + (deg + extra) * 2.0 ** -23) * absref + 1e-6


@pytest.mark.parametrize("path", ["block", "csr", "exact"])
@pytest.mark.parametrize("width,dtype", [(64, "fp16"), (64, "bf16"), (32, "fp32")])
def test_spmm_block_format(cuda_device, path, width, dtype, monkeypatch):
    """``voltrix.spmm`` on the skewed_1005 handle: the window kernel (fp32 features through the scaled cast), the forced CSR row-gather
    kernel and the exact fp32 tiles.  A ``flat+k`` feature view reached every one of these launchers as it was and came back with
    return code 1 before ``_operand`` / ``_spmm_csr`` realigned it."""
    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "none")
    monkeypatch.setenv("VOLTRIX_CSR_PATH", "1" if path == "csr" else "0")
    if path == "exact":
        monkeypatch.setenv("VOLTRIX_FP32_MODE", "exact")
    else:
        monkeypatch.delenv("VOLTRIX_FP32_MODE", raising=False)
    g, n, indptr, indices = _skewed()
    handle = voltrix.csr_preprocess(indptr, indices, n)
    handle[1].hash_tag = f"views_{path}"
    assert (sidecar.lookup_csr(handle[1]) is not None) == (path == "csr")           # the CSR side-car is attached at preprocess
    feat = _randn((n, width), DT[dtype], 14)
    out = _sweep(lambda feat: voltrix.spmm(*handle, num_nodes=n, num_edges=indices.numel(), feat=feat), dict(feat=feat), {})
    exact = path == "csr" or dtype != "fp32" or path == "exact"       # 16-bit rows as they are; fp32 rows: only the cast path rounds
    ref, bound = _product_bound(g, n, torch.ones(indices.numel()), feat, 0.0 if exact else 2.0 ** -10)
    assert out.shape == (n, width) and bool(((out.cpu().double() - ref).abs() <= bound).all())


@pytest.mark.parametrize("kind,path", [("separable", "plane"), ("general", "plane"), ("general", "csr")])
@pytest.mark.parametrize("width,dtype", [(64, "fp16"), (32, "fp32")])
def test_spmm_weighted(cuda_device, kind, path, width, dtype, monkeypatch):
    """Separable values (two ``scale_rows`` passes around the binary operator), general values through the value plane and through
    the CSR kernel with values."""
    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "none")
    monkeypatch.setenv("VOLTRIX_CSR_PATH", "1" if path == "csr" else "0")
    monkeypatch.delenv("VOLTRIX_FP32_MODE", raising=False)
    monkeypatch.setattr(weighted, "separable_pays", lambda *a: True)       # the scalings whatever the sizes say (the fixture is tiny)
    g, n, indptr, indices = _skewed()
    torch.manual_seed(15)
    if kind == "separable":
        r, c = torch.rand(n, dtype=torch.float64) * 3 + 0.05, torch.rand(n, dtype=torch.float64) * 2 + 0.1
        rows = torch.repeat_interleave(torch.arange(n), torch.from_numpy(np.diff(g["indptr"]).astype(np.int64)))
        values = (r[rows] * c[indices.long()]).float()
    else:
        values = torch.randn(indices.numel())
    handle = voltrix.csr_preprocess_weighted(indptr, indices, values, n)
    assert handle.separable == (kind == "separable")
    assert kind == "separable" or weighted._weighted_path(handle, _randn((n, width), DT[dtype])) == path
    feat = _randn((n, width), DT[dtype], 16)
    out = _sweep(lambda feat: voltrix.spmm_weighted(handle, feat, hash_tag=f"views_{kind}_{path}"), dict(feat=feat), {})
    # value plane: the values and an fp32 operand are rounded to 16 bits; separable: the scaled operand once, and the detection's
    # tolerance 2^-13 on r_i c_j; CSR kernel with values: exact products
    unit = {"plane": 2.0 ** -10, "csr": 0.0}[path] if kind == "general" else 2.0 ** -11 + 2.0 ** -13
    ref, bound = _product_bound(g, n, values, feat, unit, extra=2 if kind == "separable" else 1)
    assert bool(((out.cpu().double() - ref).abs() <= bound).all())


@pytest.mark.parametrize("width,dtype", [(64, "fp16"), (20, "fp32"), (13, "bf16")])
def test_scale_rows(cuda_device, width, dtype):
    x, f = _randn((1003, width), DT[dtype], 17), _randn((1003,), seed=18)
    out = _sweep(lambda feat, scale: weighted.scale_rows_of(feat, scale), dict(feat=x, scale=f), {}, constant=("scale",))
    assert _same_bits(out, (x.float() * f[:, None]).to(DT[dtype]))              # one rounded product: torch's own, to the bit
    assert _same_bits(weighted.scale_rows_of(_flat(x, 1), f, in_place=True), out)     # in place "where the layout allows": here a copy


def test_an_aligned_operand_is_never_copied_a_misaligned_one_always(cuda_device, monkeypatch):
    """``utils.aligned16``: the tensor that reaches the launcher is the caller's own when it is contiguous and on the 16-byte grid --
    the fast path gained no copy -- and another one when, and only when, it is not."""
    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "none")
    monkeypatch.delenv("VOLTRIX_FP32_MODE", raising=False)
    seen = {}

    def spy(module, name, index):
        inner = getattr(module, name)

        def wrapper(*args, **kwargs):
            picked = kwargs["input"] if index is None else args[index]
            seen.setdefault(name, picked.data_ptr())           # the first launch of a call: its operand
            return inner(*args, **kwargs)

        monkeypatch.setattr(module, name, wrapper)

    spmm_module = sys.modules["voltrix.spmm.spmm"]
    spy(capi, "launch_sddmm_csr", 3)
    spy(capi, "launch_sddmm_heads_csr", 3)
    spy(capi, "launch_spmm_csr_rows", 3)
    spy(capi, "launch_spmm_csr_heads", 4)
    spy(capi, "launch_scale_rows", 0)
    spy(capi, "launch_gatv2_score_csr", 5)
    spy(spmm_module, "spmm_kernel", None)
    spy(weighted, "spmm_kernel", None)

    sg = _special()
    g, n, indptr, indices = _skewed()
    monkeypatch.setenv("VOLTRIX_CSR_PATH", "auto")
    handle = voltrix.csr_preprocess(indptr, indices, n)
    handle[1].hash_tag = "views_no_copy"
    general = voltrix.csr_preprocess_weighted(indptr, indices, torch.randn(indices.numel()), n)
    separable = voltrix.csr_preprocess_weighted(indptr, indices, None, n, row_scale=torch.rand(n) + 0.5, col_scale=torch.rand(n) + 0.5)
    monkeypatch.setattr(weighted, "separable_pays", lambda *a: True)
    y64 = _randn((sg.num_cols, 64), torch.float16, 20)
    y3 = _randn((sg.num_cols, 4, 16), torch.float16, 21)
    edge = _randn((sg.nnz,), seed=22)
    a = _randn((4, 16), seed=23)

    def block(feat):
        monkeypatch.setenv("VOLTRIX_CSR_PATH", "0")
        voltrix.spmm(*handle, num_nodes=n, num_edges=indices.numel(), feat=feat)

    def forced_csr(feat):
        monkeypatch.setenv("VOLTRIX_CSR_PATH", "1")
        voltrix.spmm(*handle, num_nodes=n, num_edges=indices.numel(), feat=feat)

    def plane(feat):
        monkeypatch.setenv("VOLTRIX_CSR_PATH", "0")
        voltrix.spmm_weighted(general, feat)

    def values_csr(feat):
        monkeypatch.setenv("VOLTRIX_CSR_PATH", "1")
        voltrix.spmm_weighted(general, feat)

    def scaled(feat):
        monkeypatch.setenv("VOLTRIX_CSR_PATH", "0")
        voltrix.spmm_weighted(separable, feat)

    feat = _randn((n, 64), torch.float16, 24)
    cases = [
        ("launch_sddmm_csr", y64, lambda t: voltrix.sddmm(sg.t_indptr, sg.t_indices, t, y64)),
        ("launch_sddmm_heads_csr", y3, lambda t: voltrix.sddmm(sg.t_indptr, sg.t_indices, t, y3)),
        ("launch_spmm_csr_rows", y64, lambda t: csr_values_product(sg.indptr, sg.indices, edge, sg.num_rows, t)),
        ("launch_spmm_csr_heads", y3, lambda t: voltrix.spmm_heads(sg.indptr, sg.indices, edge[:, None].expand(-1, 4), t, sg.num_rows)),
        ("launch_scale_rows", y64, lambda t: weighted.scale_rows_of(t, edge[:sg.num_cols].contiguous())),
        ("launch_gatv2_score_csr", a, lambda t: voltrix.gatv2_score(sg.indptr, sg.indices, y3[:sg.num_rows], y3, t)),
        ("spmm_kernel", feat, block),
        ("launch_spmm_csr_rows", feat, forced_csr),
        ("spmm_kernel", feat, plane),
        ("launch_spmm_csr_rows", feat, values_csr),
        ("launch_scale_rows", feat, scaled),
    ]
    for name, t, call in cases:
        own = t.clone()
        assert own.data_ptr() % 16 == 0
        seen.clear()
        call(own)
        assert seen[name] == own.data_ptr(), (name, "an aligned contiguous operand was copied")
        for k in (1, 4) if t.element_size() == 2 else (1, 2, 3):
            off = _flat(t, k)
            seen.clear()
            call(off)
            assert seen[name] != off.data_ptr() and seen[name] % 16 == 0, (name, k, "a misaligned operand reached the launcher")


# ---- B. caller-provided outputs between guards, through capi.launch_* ---------------------------------------------------------------------
def _guarded(shape, k):
    """(buffer, out): ``out`` = ``shape`` floats at element ``GUARD + k`` of a flat buffer filled with the sentinel."""
    numel = int(np.prod(shape))
    buf = torch.empty(GUARD + numel + GUARD + 3, dtype=torch.float32, device="cuda")
    buf.view(torch.int32).fill_(SENTINEL)
    out = buf[GUARD + k:GUARD + k + numel].view(shape)
    assert (buf.data_ptr() + 4 * GUARD) % 16 == 0 and out.is_contiguous()
    return buf, out


def _check_guards(buf, out, k, what):
    torch.cuda.synchronize()
    words = buf.view(torch.int32)
    first, past = GUARD + k, GUARD + k + out.numel()
    changed = torch.nonzero(words != SENTINEL).flatten()
    changed = changed[(changed < first) | (changed >= past)]
    if changed.numel():
        i = int(changed[0])
        where = f"{first - i} floats before out[0]" if i < first else f"{i - past + 1} floats past out[-1]"
        raise AssertionError(f"{what}, k = {k}: guard word {i} of the buffer was written, {where} ({changed.numel()} guard words changed)")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _softmax_ws(g, heads):
    size = capi.edge_softmax_workspace_bytes(g.num_rows, g.nnz) if heads == 1 else capi.edge_softmax_heads_workspace_bytes(g.num_rows, g.nnz, heads)
    return torch.empty(size, dtype=torch.uint8, device="cuda")


@functools.lru_cache(maxsize=None)
def _four_byte_cases():
    """name -> (expected, launch(out)): launchers whose ``out`` needs 4 bytes only.  Built once, never written."""
    g, cg = _special(), _chunk_graph()
    x16, y16 = _randn((g.num_rows, 64), torch.float16, 30), _randn((g.num_cols, 64), torch.float16, 31)
    x3, y3 = _randn((g.num_rows, 3, 20), seed=32), _randn((g.num_cols, 3, 20), seed=33)
    a3 = _randn((3, 20), seed=34)
    cases = {
        "sddmm": (voltrix.sddmm(g.indptr, g.indices, x16, y16),
                  lambda out: capi.launch_sddmm_csr(g.indptr, g.indices, g.num_rows, x16, y16, out, _stream())),
        "sddmm_heads": (voltrix.sddmm(g.indptr, g.indices, x3, y3),
                        lambda out: capi.launch_sddmm_heads_csr(g.indptr, g.indices, g.num_rows, x3, y3, out, _stream())),
        "gatv2_score": (voltrix.gatv2_score(g.indptr, g.indices, x3, y3, a3, 0.2),
                        lambda out: capi.launch_gatv2_score_csr(g.indptr, g.indices, g.num_rows, x3, y3, a3, 0.2, out, _stream())),
    }
    for heads in (1, 3):
        shape = (cg.nnz,) if heads == 1 else (cg.nnz, heads)
        scores, grad = _randn(shape, seed=35) * 4, _randn(shape, seed=36)
        alpha = voltrix.edge_softmax(cg.indptr, scores, 0.5)
        fwd = capi.launch_edge_softmax_csr if heads == 1 else capi.launch_edge_softmax_heads_csr
        bwd = capi.launch_edge_softmax_backward_csr if heads == 1 else capi.launch_edge_softmax_heads_backward_csr
        tag = "" if heads == 1 else "_heads"
        cases[f"edge_softmax{tag}"] = (alpha, lambda out, f=fwd, s=scores, h=heads: f(cg.indptr, cg.num_rows, s, 0.5, out, _softmax_ws(cg, h), _stream()))
        cases[f"edge_softmax_backward{tag}"] = (edge_softmax_backward(cg.indptr, alpha, grad, 0.5),
                                                lambda out, f=bwd, al=alpha, gr=grad, h=heads: f(cg.indptr, cg.num_rows, al, gr, 0.5, out,
                                                                                              _softmax_ws(cg, h), _stream()))
    for heads in (1, 3, 4, 8):
        el, er = _randn((cg.num_rows, heads), seed=37), _randn((cg.num_cols, heads), seed=38)
        cases[f"gat_score_H{heads}"] = (voltrix.gat_score(cg.indptr, cg.indices, el, er, 0.2),
                                        lambda out, el=el, er=er: capi.launch_gat_score_csr(cg.indptr, cg.indices, cg.num_rows, el, er, 0.2, out,
                                                                                            _stream()))
    el, er, grad = _randn((cg.num_rows, 3), seed=39), _randn((cg.num_cols, 3), seed=40), _randn((cg.nnz, 3), seed=41)
    cases["gat_score_rowsum"] = (
        gat_score_backward(cg.t_indptr, cg.t_indices, er, el, grad, 0.2, order=cg.t_order),
        lambda out: capi.launch_gat_score_rowsum_csr(cg.t_indptr, cg.t_indices, cg.t_order, cg.num_cols, er, el, grad, 0.2, out,
                                                     torch.empty(capi.gat_score_workspace_bytes(cg.num_cols, cg.nnz, 3), dtype=torch.uint8,
                                                                 device="cuda"), _stream()))
    return cases


FOUR_BYTE = ["sddmm", "sddmm_heads", "gatv2_score", "edge_softmax", "edge_softmax_backward", "edge_softmax_heads",
             "edge_softmax_backward_heads", "gat_score_H1", "gat_score_H3", "gat_score_H4", "gat_score_H8", "gat_score_rowsum"]


@pytest.mark.parametrize("name", FOUR_BYTE)
def test_guarded_outputs_four_byte(cuda_device, name):
    """``out`` at every 4-byte offset: the bits of the Python API's result and not one word outside ``out`` written.  ``edge_softmax``
    at ``k = 1`` is the case that takes the 4-byte stores of ``edge_softmax_chunk_kernel`` with ``all_done`` true (the rows of chunk 0)."""
    expected, launch = _four_byte_cases()[name]
    for k in (0, 1, 2, 3):
        buf, out = _guarded(tuple(expected.shape), k)
        launch(out)
        _check_guards(buf, out, k, name)
        assert _same_bits(out, expected), (name, k)


@functools.lru_cache(maxsize=None)
def _sixteen_byte_cases():
    """name -> (expected, launch(out)): launchers that require a 16-byte ``out`` and reject anything else on the host."""
    g = _special()
    p3, q3, grad = _randn((g.num_rows, 3, 20), seed=42), _randn((g.num_cols, 3, 20), seed=43), _randn((g.nnz, 3), seed=44)
    feat = _randn((g.num_cols, 20), seed=45)
    src, scale = _randn((37, 20), seed=46), _randn((37,), seed=47)
    ones = torch.ones(g.nnz, device="cuda")
    return {
        "gatv2_rowsum": (gatv2_rowsum(g.indptr, g.indices, p3, q3, grad, 0.2),
                         lambda out: capi.launch_gatv2_rowsum_csr(g.indptr, g.indices, None, g.num_rows, p3, q3, grad, 0.2, out, _stream())),
        "spmm_csr_heads": (voltrix.spmm_heads(g.indptr, g.indices, grad, q3, g.num_rows),
                           lambda out: capi.launch_spmm_csr_heads(g.indptr, g.indices, grad, g.num_rows, q3, out, _stream())),
        "spmm_csr_rows_values": (csr_values_product(g.indptr, g.indices, grad[:, 0].contiguous(), g.num_rows, feat),
                                 lambda out: capi.launch_spmm_csr_rows(g.indptr, g.indices, g.num_rows, feat, out, _stream(), 1,
                                                                       values=grad[:, 0].contiguous())),
        # the binary kernel adds b where the kernel with values adds fma(1, b, acc): the same bits
        "spmm_csr_rows": (csr_values_product(g.indptr, g.indices, ones, g.num_rows, feat),
                          lambda out: capi.launch_spmm_csr_rows(g.indptr, g.indices, g.num_rows, feat, out, _stream(), 1)),
        "scale_rows": (weighted.scale_rows_of(src, scale), lambda out: capi.launch_scale_rows(src, scale, out, _stream())),
    }


@pytest.mark.parametrize("name", ["gatv2_rowsum", "spmm_csr_heads", "spmm_csr_rows_values", "spmm_csr_rows", "scale_rows"])
def test_guarded_outputs_sixteen_byte(cuda_device, name):
    """``out`` on the 16-byte grid (k = 0, 4): the result and untouched guards.  Off it (k = 1): return code 1 from the host check,
    which precedes every HIP call in these launchers, and a buffer that still holds nothing but the sentinel."""
    expected, launch = _sixteen_byte_cases()[name]
    for k in (0, 4):
        buf, out = _guarded(tuple(expected.shape), k)
        launch(out)
        _check_guards(buf, out, k, name)
        assert _same_bits(out, expected), (name, k)
    buf, out = _guarded(tuple(expected.shape), 1)
    with pytest.raises(VoltrixError, match="return code 1"):
        launch(out)
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int32) == SENTINEL).all()), name


# ---- C. autograd: gradients that arrive as views ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _two_graphs():
    """Two small square patterns; the first has an odd number of rows and ``nnz % 4 != 0``, so the second piece of a ``torch.cat`` over
    the edges starts off the 16-byte grid for H = 1 and H = 3."""
    rng = np.random.default_rng(23)
    graphs = []
    for n in (37, 52):
        lengths = rng.integers(0, 12, n)
        lengths[[4, 20]] = 0
        cols = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in lengths])       # no duplicate entries: separable values
        graphs.append(t_gatv2._Graph(lengths, cols, n))                                           # and the CSR side-car need that
    assert graphs[0].num_rows % 2 == 1 and graphs[0].nnz % 4 != 0 and (3 * graphs[0].nnz) % 4 != 0
    return tuple(graphs)


def _leaves(tensors):
    return [t.clone().requires_grad_(True) for t in tensors]


def _through_cat(ops, inputs):
    """Both pieces of ``(torch.cat([op1(x1), op2(x2)]) * w).sum()`` get the input gradients of their own backward pass with their
    slice of ``w`` as an explicit, freshly allocated ``grad_out`` -- to the bit.  The hook proves that ``op2`` really was handed a
    contiguous view off the 16-byte grid."""
    leaves = [_leaves(xs) for xs in inputs]
    outs = [op(*xs) for op, xs in zip(ops, leaves)]
    seen = []
    outs[1].register_hook(lambda grad: seen.append((grad.is_contiguous(), grad.data_ptr() % 16)))
    w = _randn((outs[0].shape[0] + outs[1].shape[0],) + tuple(outs[0].shape[1:]), seed=50)
    (torch.cat(outs) * w).sum().backward()
    assert len(seen) == 1 and seen[0][0] and seen[0][1] != 0, seen
    cut = outs[0].shape[0]
    for op, xs, mine, part in zip(ops, inputs, leaves, (w[:cut].clone(), w[cut:].clone())):
        fresh = _leaves(xs)
        grads = torch.autograd.grad(op(*fresh), fresh, grad_outputs=part)
        assert all(_same_bits(x.grad, gr) for x, gr in zip(mine, grads))


def _through_sum(op, xs):
    """``.sum()`` hands the backward a stride-0 ``grad_out``: the gradients of an explicit, contiguous ``ones_like(out)``."""
    mine = _leaves(xs)
    out = op(*mine)
    seen = []
    out.register_hook(lambda grad: seen.append(set(grad.stride())))
    out.sum().backward()
    assert seen == [{0}], seen
    fresh = _leaves(xs)
    out = op(*fresh)
    grads = torch.autograd.grad(out, fresh, grad_outputs=torch.ones_like(out))
    assert all(_same_bits(x.grad, gr) for x, gr in zip(mine, grads))


def _edge_op_cases(name):
    from voltrix.autograd import SDDMM, EdgeSoftmax, GATScore, GATv2Score

    graphs = _two_graphs()
    if name == "edge_softmax":
        return [EdgeSoftmax(g.indptr, g.num_rows) for g in graphs], [(_randn((g.nnz,), seed=51),) for g in graphs]
    if name == "edge_softmax_heads":
        return [EdgeSoftmax(g.indptr, g.num_rows) for g in graphs], [(_randn((g.nnz, 3), seed=52),) for g in graphs]
    if name == "gat_score":
        return ([GATScore(g.indptr, g.indices, g.num_rows) for g in graphs],
                [(_randn((g.num_rows, 3), seed=53), _randn((g.num_cols, 3), seed=54)) for g in graphs])
    if name == "gatv2_score":
        return ([GATv2Score(g.indptr, g.indices, g.num_rows) for g in graphs],
                [(_randn((g.num_rows, 3, 20), seed=55), _randn((g.num_cols, 3, 20), seed=56), _randn((3, 20), seed=57)) for g in graphs])
    if name == "sddmm":
        return ([SDDMM(g.indptr, g.indices, g.num_rows) for g in graphs],
                [(_randn((g.num_rows, 16), torch.float16, 58), _randn((g.num_cols, 16), torch.float16, 59)) for g in graphs])
    assert name == "sddmm_heads"
    return ([SDDMM(g.indptr, g.indices, g.num_rows) for g in graphs],
            [(_randn((g.num_rows, 3, 20), seed=60), _randn((g.num_cols, 3, 20), seed=61)) for g in graphs])


@pytest.mark.parametrize("name", ["edge_softmax", "edge_softmax_heads", "gat_score", "gatv2_score", "sddmm", "sddmm_heads"])
def test_autograd_edge_operators_on_batched_graphs(cuda_device, name):
    ops, inputs = _edge_op_cases(name)
    _through_cat(ops, inputs)
    _through_sum(ops[0], inputs[0])


def _node_op(kind, g, monkeypatch):
    """(op, inputs) with a float32 output [n, ...] whose width needs no padding in the backward."""
    from voltrix.autograd import SpMM, SpMMHeads

    if kind == "heads":
        op = SpMMHeads(g.indptr, g.indices, g.num_rows)
        return (lambda feat, values: op(feat, values)), (_randn((g.num_cols, 3, 20), seed=62), _randn((g.nnz, 3), seed=63))
    feat = _randn((g.num_cols, 16), torch.float16, 64)
    if kind == "binary":
        op = SpMM(g.indptr, g.indices, g.num_rows, hash_tag="views_binary")
        return (lambda feat: op(feat)), (feat,)
    if kind == "separable":
        deg = torch.from_numpy(np.diff(g.ip)).double().clamp(min=1)
        values = deg.rsqrt()[torch.from_numpy(g.rows_np)].float()                     # r_i alone: separable whatever the columns
        op = SpMM(g.indptr, g.indices, g.num_rows, values=values, hash_tag="views_separable")
        assert op.weighted.separable and op.weighted_t.separable
        return (lambda feat: op(feat)), (feat,)
    op = SpMM(g.indptr, g.indices, g.num_rows, values=_randn((g.nnz,), seed=65), hash_tag=f"views_{kind}")
    assert not op.weighted.separable
    if kind == "general":
        return (lambda feat: op(feat)), (feat,)
    assert kind == "values"                                                           # values per call: they get a gradient too
    return (lambda feat, values: op(feat, values=values)), (feat, _randn((g.nnz,), seed=66))


@pytest.mark.parametrize("csr_path", ["0", "1"])
@pytest.mark.parametrize("kind", ["binary", "separable", "general", "values", "heads"])
def test_autograd_node_operators_with_a_misaligned_grad_out(cuda_device, kind, csr_path, monkeypatch):
    """``torch.cat([token, out.reshape(-1)])`` (a global token in front of the node features) hands the backward a contiguous
    ``grad_out`` one float off the 16-byte grid, of a width that needs no padding -- the only copy it can get is the realignment.  The
    binary and both weighted backwards passed it to launchers that reject it before ``_operand``, ``_spmm_csr``, ``_spmm_weighted_csr``
    and ``_spmm_separable`` realigned their operand."""
    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "none")
    monkeypatch.setenv("VOLTRIX_CSR_PATH", csr_path)
    monkeypatch.delenv("VOLTRIX_FP32_MODE", raising=False)
    monkeypatch.setattr(weighted, "separable_pays", lambda *a: True)
    g = _two_graphs()[0]
    op, xs = _node_op(kind, g, monkeypatch)
    mine = _leaves(xs)
    out = op(*mine)
    seen = []
    out.register_hook(lambda grad: seen.append((grad.is_contiguous(), grad.data_ptr() % 16)))
    w = _randn((out.numel() + 1,), seed=67)
    (torch.cat([torch.zeros(1, device="cuda"), out.reshape(-1)]) * w).sum().backward()
    assert seen == [(True, 4)], seen
    fresh = _leaves(xs)
    out = op(*fresh)
    grads = torch.autograd.grad(out, fresh, grad_outputs=w[1:].clone().view(out.shape))
    assert all(_same_bits(x.grad, gr) for x, gr in zip(mine, grads))
    _through_sum(op, xs)
