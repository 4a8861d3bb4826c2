"""GPU: ``voltrix.spmm_rel`` and its gradient for ``feat`` where the element offset ``row * B * F`` of the output (and of ``grad_out``)
passes 2^31: ``2^21 + 5`` rows of one entry each over 64 columns, ``B = 8``, ``F = 128``, fp16 features, 5 types.  The output is 8 GiB;
``grad_out`` has its size and is periodic, ``base[row % 257]``, so the oracle needs 257 rows of it.  Compared with
tests/spmm_rel_oracle.py within the bounds of tests/test_gpu_spmm_rel.py: the first 8 and the last 8 rows of ``out`` (the last five rows
start past 2^31 elements; the first rows show that nothing wrapped round onto them), and every element of ``grad_feat`` (64 x 128), whose
columns each gather about 32,768 rows of ``grad_out`` from all over it.

Peak device memory: ``out`` 8 GiB + ``grad_out`` 8 GiB + the index that builds it and the small operands: about 17 GiB."""
import gc

import numpy as np
import pytest
import torch

import spmm_rel_oracle as oracle

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
DEV = "cuda"
ROWS, COLS, B, F, TYPES, PERIOD = 2 ** 21 + 5, 64, 8, 128, 5, 257


def _case():
    import voltrix
    from voltrix.spmm_rel import grad_feat

    rng = np.random.default_rng(37)
    assert (ROWS - 5) * B * F == 2 ** 31
    ip = np.arange(ROWS + 1, dtype=np.int64)
    cols, types = rng.integers(0, COLS, ROWS), rng.integers(0, TYPES, ROWS)
    indptr, indices, etype = (torch.from_numpy(x.astype(np.int32)).to(DEV) for x in (ip, cols, types))
    gen = torch.Generator(device=DEV).manual_seed(37)
    feat = torch.randn(COLS, F, device=DEV, generator=gen).half()
    coef = torch.randn(TYPES, B, device=DEV, generator=gen)
    weight = torch.rand(ROWS, device=DEV, generator=gen) + 0.5
    base = torch.randn(PERIOD, B, F, device=DEV, generator=gen)

    out = voltrix.spmm_rel(indptr, indices, etype, feat, coef, ROWS, weight)
    assert out.shape == (ROWS, B, F) and out.dtype == torch.float32 and out.numel() > 2 ** 31
    torch.cuda.synchronize()
    feat64, coef64, weight64, base64 = (t.double().cpu().numpy() for t in (feat, coef, weight, base))
    for first, last in ((0, 8), (ROWS - 8, ROWS)):
        ref, mass, count = oracle.forward(ip[first:last + 1] - first, cols[first:last], types[first:last], feat64, coef64,
                                          weight64[first:last])
        err = np.abs(out[first:last].double().cpu().numpy() - ref)
        bound = (count[:, None, None] + 2) * U * mass
        print(f"out rows {first}..{last - 1}: max err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), (first, last)

    grad = base[torch.arange(ROWS, device=DEV) % PERIOD]
    assert grad.shape == (ROWS, B, F) and grad.is_contiguous() and grad.numel() > 2 ** 31
    t_indptr, t_indices, t_order = (torch.from_numpy(x).to(DEV) for x in oracle.transpose(ip, cols, COLS))
    d = grad_feat(t_indptr, t_indices, t_order, etype, grad, coef, COLS, weight)
    assert d.shape == (COLS, F) and d.dtype == torch.float32
    torch.cuda.synchronize()
    # the oracle through the period: dF[c] = sum_p sum_b S[c, p, b] base[p, b] with S the coefficients summed per (column, phase);
    # the mass takes |coefficient| and |base| (every term of a (c, p, b) cell has base[p, b]'s sign pattern)
    c = weight64[:, None] * coef64[types]                                             # [rows, B]
    cell = cols * PERIOD + np.arange(ROWS) % PERIOD
    sums, masses = np.zeros((COLS * PERIOD, B)), np.zeros((COLS * PERIOD, B))
    np.add.at(sums, cell, c)
    np.add.at(masses, cell, np.abs(c))
    ref = np.einsum("cpb,pbf->cf", sums.reshape(COLS, PERIOD, B), base64)
    mass = np.einsum("cpb,pbf->cf", masses.reshape(COLS, PERIOD, B), np.abs(base64))
    count = np.bincount(cols, minlength=COLS).astype(np.float64)
    err = np.abs(d.double().cpu().numpy() - ref)
    bound = (count[:, None] * B + 2) * U * mass
    print(f"grad_feat: max err / bound = {float((err / bound).max()):.3e}")
    assert bool((err <= bound).all())
    # grad_out's rows past 2^31 elements are the last five: they hold what their period says
    assert bool(torch.equal(grad[ROWS - 5:], base[torch.arange(ROWS - 5, ROWS, device=DEV) % PERIOD]))


def test_output_offsets_past_2_to_31(cuda_device):
    gib = 1 << 30
    need = 17.0
    free, total = torch.cuda.mem_get_info()
    assert free >= need * gib, f"this test needs {need:.1f} GiB of device memory, {free / gib:.1f} of {total / gib:.1f} GiB are free"
    try:
        _case()
    finally:
        gc.collect()
        torch.cuda.empty_cache()
