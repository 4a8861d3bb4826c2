"""GPU: ``voltrix.spmm_edge`` and its gradient for ``efeat`` where the element offset ``id * F`` of an entry passes 2^31:
``nnz = 2^21 + 5`` entries of ``F = 1024`` fp16 features (``efeat`` is 4 GiB), 4,099 rows of 511 or 512 entries over 64 columns, op mul.
``efeat`` is periodic, ``base[e % 257]``, so the oracle needs 257 rows of it.  Compared with tests/spmm_edge_oracle.py within the bounds
of tests/test_gpu_spmm_edge.py: the first 8 and the last 8 rows of ``out`` (the last row holds the entries past 2^31 elements; the first
rows show that nothing wrapped round onto them) and the last 4,096 entries of ``grad_efeat``.

Peak device memory: ``efeat`` 4 GiB + ``grad_efeat`` (fp32) 8 GiB + the small operands and the index that builds ``efeat``: about 14 GiB."""
import gc

import numpy as np
import pytest
import torch

import spmm_edge_oracle as oracle

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
DEV = "cuda"
NNZ, F, ROWS, COLS, PERIOD = 2 ** 21 + 5, 1024, 4099, 64, 257


def _case():
    import voltrix
    from voltrix.spmm_edge import grad_efeat

    rng = np.random.default_rng(31)
    longer = NNZ - 511 * ROWS
    assert 0 < longer < ROWS
    lengths = 511 + (np.arange(ROWS) < longer).astype(np.int64)          # 512-entry rows first (whole batches), 511 after (a tail of 3)
    ip = np.concatenate([[0], np.cumsum(lengths)])
    assert ip[-1] == NNZ and NNZ * F > 2 ** 31 and ip[-2] * F < 2 ** 31 < NNZ * F
    cols = rng.integers(0, COLS, NNZ)
    indptr = torch.from_numpy(ip.astype(np.int32)).to(DEV)
    indices = torch.from_numpy(cols.astype(np.int32)).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(31)
    feat = torch.randn(COLS, F, device=DEV, generator=gen).half()
    base = torch.randn(PERIOD, F, device=DEV, generator=gen).half()
    grad = torch.randn(ROWS, F, device=DEV, generator=gen)
    efeat = base[torch.arange(NNZ, device=DEV) % PERIOD]
    assert efeat.shape == (NNZ, F) and efeat.is_contiguous() and efeat.numel() > 2 ** 31

    out = voltrix.spmm_edge(indptr, indices, feat, efeat, ROWS, op="mul")
    ge = grad_efeat(indptr, indices, grad, feat, efeat, "mul")
    assert out.shape == (ROWS, F) and ge.shape == (NNZ, F) and ge.dtype == torch.float32
    torch.cuda.synchronize()

    feat64, base64, grad64 = (t.double().cpu().numpy() for t in (feat, base, grad))
    for first, last in ((0, 8), (ROWS - 8, ROWS)):
        lo, hi = int(ip[first]), int(ip[last])
        sub_efeat = base64[np.arange(lo, hi) % PERIOD]
        ref, mass, count = oracle.forward(ip[first:last + 1] - lo, cols[lo:hi], feat64, sub_efeat, "mul")
        err = np.abs(out[first:last].double().cpu().numpy() - ref)
        bound = (count[:, None] + 1) * U * mass
        print(f"out rows {first}..{last - 1}: max err / bound = {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (first, last)
    lo = NNZ - 4096
    first = int(np.searchsorted(ip, lo, side="right") - 1)                # the row of entry lo
    rows = oracle.entry_rows(ip[first:] - ip[first])[lo - int(ip[first]):] + first
    assert rows.size == 4096 and rows[-1] == ROWS - 1
    ref = grad64[rows] * feat64[cols[lo:]]
    err = np.abs(ge[lo:].double().cpu().numpy() - ref)
    print(f"grad_efeat entries {lo}..{NNZ - 1}: max err / |ref| = {float((err / np.maximum(np.abs(ref), 1e-300)).max()):.3e}")
    assert bool((err <= U * np.abs(ref)).all())
    # the entries past 2^31 elements are the last five: they hold what their period says, and nothing else was written over them
    assert (NNZ - 5) * F == 2 ** 31 and bool(torch.equal(efeat[NNZ - 5:], base[torch.arange(NNZ - 5, NNZ, device=DEV) % PERIOD]))


def test_entry_offsets_past_2_to_31(cuda_device):
    gib = 1 << 30
    need = 14.0
    free, total = torch.cuda.mem_get_info()
    assert free >= need * gib, f"this test needs {need:.1f} GiB of device memory, {free / gib:.1f} of {total / gib:.1f} GiB are free"
    try:
        _case()
    finally:
        gc.collect()
        torch.cuda.empty_cache()
