"""The float64 oracle of ``voltrix.spmm_multi`` and of its backward, with torch on CPU or device tensors, from the inputs as stored.

Forward.  max / min and their args as ``_oracle`` of tests/test_gpu_spmm_reduce.py: ``scatter_reduce`` amax / amin (a NaN among a row's
entries gives NaN), the winner the LOWEST entry id among the ties, ``-1`` and ``0`` for a row without entries.  The moments by float64
``index_add``: ``sum``, ``mean = sum / d``, ``var = sum_e (x_e - mean)^2 / d`` (two passes), ``std = sqrt(var + eps)``; a row without
entries gives 0 everywhere, a row that holds a NaN or an infinity NaN in var and std.

    |var - ref| <= (d + 4) 2^-23 (2 / d) sum_e (x_e - x_first)^2                                  (VAR)
    |std - ref| <= bound_var / ref_std + 2^-22 ref_std                                            (STD)

(VAR) was checked on the CPU with a sequential fp32 model of the shifted rule on normal, integer and 4096 + N(0, 1) data, d from 1 to
5,003: worst error / bound 0.085, while the naive ``sum x^2`` rule misses it by 93x and more on the offset data
(tests/test_spmm_multi_host.py repeats both).  (STD): the derivative of sqrt at ref_std^2 is 1 / (2 ref_std) -- the bound takes twice
that for var's error -- plus the addition of eps and the square root, each within 2^-24 of its result.

Backward.  The reference is torch float64 autograd through the composite ``x[cols]`` -> ``index_add`` -> (two-pass variance) ->
``sqrt``, with max / min taken at the ORACLE's arg entries, so ties route to the first entry in CSR order as specified.  The kernel
computes, per element of column c, ``sum_e u_r + w_r (x_c - mean_r) + [argmax] g_max_r + [argmin] g_min_r`` with
``u = g_sum + g_mean / d`` and ``w = 2 g_var / d + g_std / (d std)`` formed in fp32.  With E = 2^-23 (twice the unit roundoff):

    accumulation   k E sum |terms| for the k terms that land on an element (k - 1 fp32 additions; the product of the centred term is
                   fused into its addition)
    u              E (|g_sum| + |g_mean| / d): one division and one addition
    w              dw = 2 E (|2 g_var / d| + |b|) + |b| ds / (ref_std - ds), b = g_std / (d ref_std): a product, two divisions, one
                   addition, and the STORED std, which is within ds = (STD) of ref_std
    centred term   |w^ (x - m^) - w (x - m)| <= dw |x - m| + (|w| + dw) (dm + E (|x - m| + dm)): the STORED mean is within
                   dm = (d + 1) E sum_e |x_e| / d of m (spmm_reduce's bound), the subtraction rounds once

    bound[c, f] = sum_e (u's + the centred term's) + k E sum_e sum |terms|                         (BWD)

The selections add no error of their own: an arg is an integer and a routed gradient is passed on as it is.
"""
import torch

U = 2.0 ** -23
BIG_ID = 2 ** 40
AGGREGATES = ("sum", "mean", "max", "min", "var", "std")


def entry_rows(indptr):
    """int64 [nnz]: the row of every entry."""
    ip = indptr.long()
    return torch.repeat_interleave(torch.arange(ip.numel() - 1, device=ip.device), ip[1:] - ip[:-1])


def select(rows, cols, feat, num_rows, reduce):
    """(ref float64 [num_rows, F], arg int64 [num_rows, F]) of max / min; rows / cols: int64 per entry."""
    f = feat.shape[1]
    g = feat.double()[cols]
    idx = rows[:, None].expand(-1, f)
    ref = torch.zeros(num_rows, f, dtype=torch.float64, device=feat.device)
    ref = ref.scatter_reduce(0, idx, g, "amax" if reduce == "max" else "amin", include_self=False)
    won = (g == ref[rows]) | (g.isnan() & ref[rows].isnan())
    ids = torch.arange(rows.numel(), device=feat.device)[:, None].expand(-1, f)
    arg = torch.full((num_rows, f), BIG_ID, dtype=torch.int64, device=feat.device)
    arg = arg.scatter_reduce(0, idx, torch.where(won, ids, torch.full_like(ids, BIG_ID)), "amin", include_self=True)
    return ref, torch.where(arg == BIG_ID, torch.full_like(arg, -1), arg)


def forward(indptr, indices, feat, num_rows, eps=1e-5):
    """A dict of float64 [num_rows, F]: ``sum mean max min var std``, int64 ``argmax argmin``, the bounds ``var_bound std_bound``,
    ``deg`` [num_rows] (entries per row), ``nonfinite`` (bool [num_rows, F]: the row holds a NaN or an infinity there) and
    ``abs_mean`` (sum_e |x_e| / d, what the mean's own error scales with); ``feat`` [num_cols, F]."""
    rows, cols = entry_rows(indptr), indices.long()
    f = feat.shape[1]
    zeros = lambda: torch.zeros(num_rows, f, dtype=torch.float64, device=feat.device)      # noqa: E731
    deg = (indptr.long()[1:] - indptr.long()[:-1]).double()
    d = deg.clamp(min=1)[:, None]
    g = feat.double()[cols]
    out = {"deg": deg}
    out["max"], out["argmax"] = select(rows, cols, feat, num_rows, "max")
    out["min"], out["argmin"] = select(rows, cols, feat, num_rows, "min")
    out["sum"] = zeros().index_add_(0, rows, g)
    out["mean"] = out["sum"] / d
    out["abs_mean"] = zeros().index_add_(0, rows, g.abs()) / d
    out["nonfinite"] = zeros().index_add_(0, rows, (~g.isfinite()).double()) > 0
    nan = torch.full_like(out["sum"], float("nan"))
    var = zeros().index_add_(0, rows, (g - out["mean"][rows]) ** 2) / d
    out["var"] = torch.where(out["nonfinite"], nan, var)
    occupied = (deg > 0)[:, None].expand(-1, f)
    out["std"] = torch.where(occupied, (out["var"] + eps).sqrt(), torch.zeros_like(var))
    first = feat.double()[cols[indptr.long()[:-1].clamp(max=max(cols.numel() - 1, 0))]] if cols.numel() else zeros()
    spread = zeros().index_add_(0, rows, (g - first[rows]) ** 2)
    out["var_bound"] = (deg[:, None] + 4) * U * (2 / d) * spread
    out["std_bound"] = torch.where(occupied, out["var_bound"] / out["std"] + 2 * U * out["std"], torch.zeros_like(var))
    return out


def backward(indptr, indices, feat, num_rows, grads, eps=1e-5):
    """(d_feat float64 [num_cols, F], bound) for ``grads``: a dict from aggregate names to the gradients [num_rows, F] of the outputs;
    the reference by float64 autograd through the composite, the bound (BWD) of the module's docstring."""
    rows, cols = entry_rows(indptr), indices.long()
    num_cols, f = feat.shape
    ref = forward(indptr, indices, feat, num_rows, eps)
    zeros = lambda n: torch.zeros(n, f, dtype=torch.float64, device=feat.device)      # noqa: E731
    d = ref["deg"].clamp(min=1)[:, None]
    occupied = (ref["deg"] > 0)[:, None].expand(-1, f)
    grads = {name: g.double() for name, g in grads.items()}
    with torch.enable_grad():
        x = feat.double().clone().requires_grad_(True)
        g = x[cols]
        total = x.sum() * 0
        if "sum" in grads or "mean" in grads or "var" in grads or "std" in grads:
            s = zeros(num_rows).index_add(0, rows, g)
            mean = s / d
            if "sum" in grads:
                total = total + (s * grads["sum"]).sum()
            if "mean" in grads:
                total = total + (mean * grads["mean"]).sum()
            if "var" in grads or "std" in grads:
                var = zeros(num_rows).index_add(0, rows, (g - mean[rows]) ** 2) / d
                if "var" in grads:
                    total = total + (var * grads["var"]).sum()
                if "std" in grads:
                    total = total + ((var + eps).sqrt() * grads["std"])[occupied].sum()
        for name in ("max", "min"):
            if name in grads:
                arg = ref["arg" + name]
                taken = torch.gather(g, 0, arg.clamp(min=0))                 # [num_rows, F]: the winner's value
                total = total + (taken * grads[name])[arg >= 0].sum()
        total.backward()
    want = x.grad

    # ---- the bound
    none = zeros(num_rows)
    g = feat.double()[cols]
    g_sum, g_mean = grads.get("sum", none), grads.get("mean", none)
    a = 2 * grads.get("var", none) / d
    std = torch.where(occupied, ref["std"], torch.ones_like(ref["std"]))
    ds = torch.where(occupied, ref["std_bound"], torch.zeros_like(std))
    b = grads.get("std", none) / (d * std)
    w = a + b
    dw = 2 * U * (a.abs() + b.abs()) + b.abs() * ds / (std - ds).clamp_min(1e-300)
    dm = (ref["deg"][:, None] + 1) * U * ref["abs_mean"]
    u = g_sum + g_mean / d
    centred = (g - ref["mean"][rows]).abs()                                  # [nnz, F]
    term_err = U * (g_sum.abs() + g_mean.abs() / d)[rows]
    mass = torch.zeros_like(g)
    count = torch.zeros_like(g)
    if "sum" in grads or "mean" in grads:
        mass += u.abs()[rows]
        count += 1
    if "var" in grads or "std" in grads:
        term_err = term_err + dw[rows] * centred + (w.abs() + dw)[rows] * (dm[rows] + U * (centred + dm[rows]))
        mass += w.abs()[rows] * centred
        count += 1
    ids = torch.arange(rows.numel(), device=feat.device)[:, None]
    for name in ("max", "min"):
        if name in grads:
            hit = ref["arg" + name][rows] == ids
            mass += torch.where(hit, grads[name][rows].abs(), torch.zeros_like(g))
            count += hit.double()
    k = zeros(num_cols).index_add_(0, cols, count)
    bound = zeros(num_cols).index_add_(0, cols, term_err) + k * U * zeros(num_cols).index_add_(0, cols, mass)
    return want, bound
