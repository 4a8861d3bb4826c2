"""GPU: ``voltrix.spmm_multi`` where ``row * A * F`` passes 2^31 elements: all six aggregates and both args on a periodic pattern of
short rows (tests/large_offset_cases.py), every element of every output checked against the float64 oracle of ONE period and of the
tail (tests/spmm_multi_oracle.py).  Integer features: sum, max, min and the args are compared for equality, mean, var and std within
the oracle's bounds (the mean's: spmm_reduce's ``(d + 1) 2^-23 sum |x| / d``)."""
import gc

import numpy as np
import pytest
import torch

import large_offset_cases as loc
import spmm_multi_oracle as oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
ALL = oracle.AGGREGATES


def _reference(g, feat, eps):
    """(ref, bound) float64 [rows, 6 F] of a ``Graph``'s rows in the layout of ``out``, and its (argmax, argmin) relative to the row's
    first entry (-1 for a row without entries)."""
    indptr, indices = torch.from_numpy(g.ip).to(DEV), g.cols
    r = oracle.forward(indptr, indices, feat, g.num_rows, eps)
    zero = torch.zeros_like(r["sum"])
    mean_bound = (r["deg"][:, None] + 1) * oracle.U * r["abs_mean"]
    bounds = {"sum": zero, "mean": mean_bound, "max": zero, "min": zero, "var": r["var_bound"], "std": r["std_bound"]}
    ref = torch.stack([r[name] for name in ALL], dim=1).flatten(1)
    bound = torch.stack([bounds[name] for name in ALL], dim=1).flatten(1)
    first = torch.from_numpy(g.ip[:-1] * (g.lengths > 0)).to(DEV)[:, None]
    return ref, bound, (r["argmax"] - first).double(), (r["argmin"] - first).double()


def _periodic_case(dim, num_cols, boundary, dtype):
    import voltrix

    eps = 1e-5
    rng = np.random.default_rng(21)
    lengths = np.asarray([0, 1, 2, 3, 4, 5, 7, 8, 9, 0, 6] + [int(v) for v in rng.integers(0, 10, 30)], np.int64)
    if lengths.sum() % 2 == 0:
        lengths[-1] += 1
    rows_np = np.repeat(np.arange(len(lengths)), lengths)
    cols_np = np.sort(rows_np * num_cols + rng.integers(0, num_cols // 2, rows_np.size)) % num_cols
    period_rows, period_edges = len(lengths), int(lengths.sum())
    reps = boundary // (len(ALL) * dim * period_rows) + 1
    nnz = reps * period_edges + int(lengths[:7].sum()) + 2                 # a tail of seven whole rows and one cut to two entries
    pc = loc.Periodic(lengths, cols_np, num_cols, nnz, DEV)
    assert pc.reps == reps and pc.cut == 2 and pc.tail_rows == 8 and (pc.num_rows - pc.tail_rows) * len(ALL) * dim > boundary
    indptr, indices = pc.indptr(), pc.indices()
    gen = torch.Generator(device=DEV).manual_seed(5)
    feat = torch.randint(-3, 4, (num_cols, dim), device=DEV, generator=gen).to(dtype)      # ties: first wins, in every period
    tally = loc.Tally()

    out, state = voltrix.spmm_multi(indptr, indices, feat, pc.num_rows, aggrs=ALL, eps=eps, return_state=True)
    assert out.shape == (pc.num_rows, len(ALL), dim) and out.numel() > boundary
    ref_p, bound_p, amax_p, amin_p = _reference(pc.period, feat, eps)
    ref_t, bound_t, amax_t, amin_t = _reference(pc.tail, feat, eps)
    ok_out, _ = loc.check_tiled(out.view(pc.num_rows, -1), pc.reps, (ref_p, bound_p), (ref_t, bound_t), "out", tally)
    assert _equal_slots(out, ref_p, pc.P, dim)
    del out
    # an arg relative to its row's first entry is periodic (in place: no second tensor of its size); rows without entries keep -1
    start = indptr[:-1].clone()
    start[indptr[1:] == indptr[:-1]] = 0
    oks = [ok_out]
    for what, arg, ref in (("argmax", state.argmax, (amax_p, amax_t)), ("argmin", state.argmin, (amin_p, amin_t))):
        arg.sub_(start[:, None])
        ok, _ = loc.check_tiled(arg, pc.reps, (ref[0], None), (ref[1], None), what, tally)
        oks.append(ok)
    tally.assert_complete("out", "argmax", "argmin")
    assert all(oks), oks


def _equal_slots(out, ref_p, period_rows, dim):
    """sum, max and min of the LAST whole period, past the boundary, for equality (their bound above is 0 as well)."""
    n = out.shape[0]
    last = (n - 8) // period_rows - 1
    block = out[last * period_rows:(last + 1) * period_rows].double()
    want = ref_p.view(period_rows, len(ALL), dim)
    return all(torch.equal(block[:, i], want[:, i]) for i in (0, 2, 3))


def test_element_offsets_past_2_to_31(cuda_device):
    """num_rows * 6 * F > 2^31 with fp16 rows of F = 128.  Peak: out of 8.1 GiB, the two args of 1.4 GiB each, the comparison slabs."""
    gib = 1 << 30
    need = 8.1 + 2 * 1.4 + 5
    free, total = torch.cuda.mem_get_info()
    assert free >= need * gib, f"this test needs {need:.1f} GiB of device memory, {free / gib:.1f} of {total / gib:.1f} GiB are free"
    try:
        _periodic_case(128, 2000, 2 ** 31, torch.float16)
    finally:
        gc.collect()
        torch.cuda.empty_cache()
