"""GPU: ``voltrix.quantize_fp8`` and ``voltrix.spmm_fp8`` where every element offset passes 2^31: ``2^24 + 5`` rows of one entry each over
``2^24 + 5`` columns at ``F = 128``.  The gathered offset ``col * F16`` and the output offset ``row * F16`` reach ``2^31 + 512``; the
quantiser reads ``feat`` (fp16, 4 GiB) and writes ``data`` (2 GiB) at the same offsets.  ``feat`` is periodic in the row index,
``base[row % 257]``, so the oracle needs 257 rows of it.  Row ``i`` gathers column ``i``, except that the first five rows gather the last
five columns and the last five rows the first five: an offset that wrapped round shows at both ends.  Checked against
tests/spmm_fp8_oracle.py: the first 8 and the last 8 rows of ``data`` (bit for bit) and of ``out`` (within the bound of
tests/test_gpu_spmm_fp8.py; one entry per row).

Peak device memory.  While quantising: ``feat`` 4 GiB + the int64 row index that built it 0.125 GiB + the transient ``feat.abs()``
behind the column maxima 4 GiB + ``data`` 2 GiB = 10.1 GiB.  ``feat`` and the allocator's cache are dropped before the aggregation,
which holds ``data`` 2 GiB + ``out`` (fp32) 8 GiB + ``indptr``, ``indices`` and ``values`` 0.2 GiB + the gathered end rows = 10.3 GiB.
11 GiB are asked for."""
import gc

import numpy as np
import pytest
import torch

import spmm_fp8_oracle as oracle

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
DEV = "cuda"
ROWS, F, PERIOD = 2 ** 24 + 5, 128, 257


def _case():
    import voltrix

    assert (ROWS - 5) * F == 2 ** 31
    gen = torch.Generator().manual_seed(53)
    base = (torch.randn(PERIOD, F, generator=gen) * 10.0 ** (torch.rand(1, F, generator=gen) * 2 - 1)).half()
    feat = base.to(DEV)[torch.arange(ROWS, device=DEV) % PERIOD]
    assert feat.shape == (ROWS, F) and feat.is_contiguous() and feat.numel() > 2 ** 31
    rows = voltrix.quantize_fp8(feat, "column")
    del feat
    torch.cuda.empty_cache()
    assert rows.data.shape == (ROWS, F) and rows.data.numel() > 2 ** 31
    # every residue of the period occurs, so the column maxima are those of the base
    # (the torch formula where the data lives: the device's fp32 division differs from the CPU's in the last bit)
    scale, inv = (t.cpu() for t in oracle.scales(base.to(DEV), "column"))
    assert bool(torch.equal(rows.scale.cpu(), scale)) and bool(torch.equal(rows.inv_scale.cpu(), inv))
    codes = oracle.quantize(base, inv)                                                     # [PERIOD, F]
    ends = np.concatenate([np.arange(8), np.arange(ROWS - 8, ROWS)])
    got = rows.data.view(torch.uint8)[torch.from_numpy(ends).to(DEV)].cpu()
    assert bool(torch.equal(got, codes[torch.from_numpy(ends % PERIOD)])), "data: the first 8 / last 8 rows"

    cols = np.arange(ROWS, dtype=np.int64)
    cols[:5], cols[ROWS - 5:] = np.arange(ROWS - 5, ROWS), np.arange(5)
    indptr = torch.arange(ROWS + 1, dtype=torch.int32, device=DEV)
    indices = torch.from_numpy(cols.astype(np.int32)).to(DEV)
    values = (torch.arange(ROWS, device=DEV) % 11 + 1).float() * 0.37       # rows 1 .. 4 and the last five differ in it
    out = voltrix.spmm_fp8(indptr, indices, rows, ROWS, values=values)
    assert out.shape == (ROWS, F) and out.dtype == torch.float32 and out.numel() > 2 ** 31
    torch.cuda.synchronize()
    table = oracle.decode_table()
    v = values[torch.from_numpy(ends).to(DEV)].double().cpu().numpy()
    dec = table[codes.numpy()[cols[ends] % PERIOD]]                                        # [16, F]
    ref = scale.double().numpy() * v[:, None] * dec
    err = np.abs(out[torch.from_numpy(ends).to(DEV)].double().cpu().numpy() - ref)
    bound = (1 + 2) * U * np.abs(ref)
    print(f"out, first 8 / last 8 rows: max err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    assert len({tuple(r) for r in ref}) == 16                                              # the 16 rows tell each other apart


def test_offsets_past_2_to_31(cuda_device):
    gib = 1 << 30
    need = 11.0
    free, total = torch.cuda.mem_get_info()
    assert free >= need * gib, f"this test needs {need:.1f} GiB of device memory, {free / gib:.1f} of {total / gib:.1f} GiB are free"
    try:
        _case()
    finally:
        gc.collect()
        torch.cuda.empty_cache()
