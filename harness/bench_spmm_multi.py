#!/usr/bin/env python3
"""Time ``voltrix.spmm_multi`` with PNA's four aggregates (mean, max, min, std) and its fused backward against what they replace, on
synth_graphs stand-ins.

Per graph, width (F = 64, 128) and dtype (fp16, fp32), in one process on one GPU.  Every variant is timed in ``--rounds`` windows of
``--steps`` calls bracketed by device events, the variants ALTERNATING inside a round, and the median window is reported with the
spread (max - min over the median):
  forward
  * ``multi``        one ``spmm_multi`` launch, four aggregates;  ``multi_state``: the same with both args written (the training forward)
  * ``two_launch``   ``spmm_multi(("max", "min"))`` + ``spmm_multi(("mean", "std"))``: selects and moments apart, fewer registers each
  * ``existing`` (a) ``spmm_reduce`` mean + max + min and two ``spmm_csr_rows`` gathers of x and x * x for the naive std, with the
                     dense square and the fp32 ``E[x^2] - E[x]^2`` tail -- the best route before this operator (its std cancels)
  * ``max_alone`` (b) one ``spmm_reduce("max")`` call: the floor the one-gather hypothesis predicts ``multi`` stays near
  * ``torch`` (c)    ``feat[cols]`` + ``scatter_reduce`` amax / amin + ``index_add_`` mean and two-pass std (``--torch-steps`` steps; a
                     composite whose [nnz, F] temporaries do not fit is recorded as ``torch_out_of_memory``)
  backward
  * ``multi_bwd``    the dense ``u`` / ``w`` and one ``spmm_multi.backward`` launch
  * ``existing_bwd`` what it replaces: two ``spmm_reduce_backward`` launches (max, min), ``spmm_mean_backward``, and for the std the
                     uncentred form ``x A^T w - A^T (w mean)`` through two ``spmm_csr_rows`` gathers on the transpose
One JSON line per point on stdout and appended to ``--out``: milliseconds, spreads, the forward byte model 4 (n + 1) + 4 nnz + nnz F
sizeof(T) + 16 n F and its share of 8 TB/s, and the ratios."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "voltrix-spmm_amd")):
    sys.path.insert(0, p)
os.environ.setdefault("VOLTRIX_CACHE_DIR", os.path.join(REPO, "voltrix-spmm_amd", ".jit_cache"))

import torch  # noqa: E402

import synth_graphs  # noqa: E402
import voltrix  # noqa: E402
from voltrix import capi  # noqa: E402
from voltrix.autograd import CsrPattern  # noqa: E402
from voltrix.spmm_reduce import row_degrees, spmm_mean_backward, spmm_reduce_backward  # noqa: E402

DEFAULT_CASES = ("amazon0601_like", "web_berkstan_like", "reddit_like", "yeast_like")
PNA = ("mean", "max", "min", "std")
HBM_BYTES_PER_S = 8e12
DTYPES = {"fp16": torch.float16, "fp32": torch.float32}
EPS = 1e-5


def _window(fn, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / steps


def _alternating(variants, steps, warmup, rounds):
    """{name: (median ms, (max - min) / median)} of ``variants`` ({name: callable}), a window of each per round."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    seen = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            seen[name].append(_window(fn, steps))
    return {name: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for name, v in seen.items()}


def run_graph(name, widths, dtypes, steps, warmup, rounds, torch_steps, scale, sink):
    indptr, indices, _ = synth_graphs.generate(name, device="cuda", scale=scale)
    n = indptr.numel() - 1
    nnz = indices.numel()
    pattern = CsrPattern(indptr, indices, n)
    deg = indptr[1:] - indptr[:-1]
    t_deg = pattern.t_indptr[1:] - pattern.t_indptr[:-1]
    degrees = row_degrees(indptr)
    stream = torch.cuda.current_stream().cuda_stream
    t = (pattern.t_indptr, pattern.t_indices, pattern.t_order)
    for dim in widths:
        for dtype_name in dtypes:
            dtype = DTYPES[dtype_name]
            torch.manual_seed(0)
            feat = (1.0 + torch.randn(n, dim, device="cuda")).to(dtype)          # a mean of one standard deviation: after a ReLU
            grads = torch.randn(n, 4, dim, device="cuda")
            s1, s2 = torch.empty(n, dim, device="cuda"), torch.empty(n, dim, device="cuda")

            def existing():
                mean = voltrix.spmm_reduce(indptr, indices, feat, n, "mean")
                hi = voltrix.spmm_reduce(indptr, indices, feat, n, "max")
                lo = voltrix.spmm_reduce(indptr, indices, feat, n, "min")
                capi.launch_spmm_csr_rows(indptr, indices, n, feat, s1, stream, 1)
                capi.launch_spmm_csr_rows(indptr, indices, n, feat * feat, s2, stream, 1)
                m = s1 / degrees[:, None]
                return mean, hi, lo, (s2 / degrees[:, None] - m * m).clamp_min(0).add(EPS).sqrt()

            def two_launch():
                return (voltrix.spmm_multi(indptr, indices, feat, n, aggrs=("max", "min")),
                        voltrix.spmm_multi(indptr, indices, feat, n, aggrs=("mean", "std"), eps=EPS))

            forward = {"multi": lambda: voltrix.spmm_multi(indptr, indices, feat, n, aggrs=PNA, eps=EPS),
                       "multi_state": lambda: voltrix.spmm_multi(indptr, indices, feat, n, aggrs=PNA, eps=EPS, return_state=True),
                       "two_launch": two_launch, "existing": existing,
                       "max_alone": lambda: voltrix.spmm_reduce(indptr, indices, feat, n, "max")}
            out, state = forward["multi_state"]()
            naive = existing()
            for i in range(3):                                  # the shared aggregates are the existing operators' bits
                assert torch.equal(out[:, i], naive[i]), PNA[i]
            g = {a: grads[:, i].contiguous() for i, a in enumerate(PNA)}

            def multi_bwd():
                u = g["mean"] / degrees[:, None]
                w = g["std"] / (degrees[:, None] * state.std)
                return voltrix.spmm_multi.backward(*t, n, feat=feat, u=u, w=w, mean=state.mean, g_max=g["max"], argmax=state.argmax,
                                                   g_min=g["min"], argmin=state.argmin)

            def existing_bwd():
                d = spmm_reduce_backward(*t, g["max"], state.argmax, n) + spmm_reduce_backward(*t, g["min"], state.argmin, n)
                d += spmm_mean_backward(t[0], t[1], g["mean"], degrees, n)
                w = (g["std"] / (degrees[:, None] * state.std)).contiguous()
                capi.launch_spmm_csr_rows(t[0], t[1], n, w, s1, stream, 1)
                capi.launch_spmm_csr_rows(t[0], t[1], n, (w * state.mean).contiguous(), s2, stream, 1)
                return d + feat * s1 - s2

            ms = _alternating({**forward, "multi_bwd": multi_bwd, "existing_bwd": existing_bwd}, steps, warmup, rounds)
            torch_ms = None
            try:
                rows = torch.repeat_interleave(torch.arange(n, device="cuda"), deg.long())
                cols = indices.long()

                def composite():
                    gathered = feat[cols].float()
                    idx = rows[:, None].expand(-1, dim)
                    zeros = torch.zeros(n, dim, device="cuda")
                    hi = zeros.scatter_reduce(0, idx, gathered, "amax", include_self=False)
                    lo = zeros.scatter_reduce(0, idx, gathered, "amin", include_self=False)
                    mean = torch.zeros(n, dim, device="cuda").index_add_(0, rows, gathered) / degrees[:, None]
                    var = torch.zeros(n, dim, device="cuda").index_add_(0, rows, (gathered - mean[rows]) ** 2) / degrees[:, None]
                    return mean, hi, lo, (var + EPS).sqrt()

                composite()
                torch.cuda.synchronize()
                torch_ms = _window(composite, torch_steps)
                del rows, cols
            except torch.cuda.OutOfMemoryError:              # the composite's [nnz, F] temporaries do not fit: recorded, not hidden
                torch.cuda.empty_cache()
            size = feat.element_size()
            nbytes = 4 * (n + 1) + 4 * nnz + nnz * dim * size + 16 * n * dim
            line = {"graph": name, "scale": scale, "F": dim, "dtype": dtype_name, "num_rows": n, "nnz": nnz, "max_deg": int(deg.max()),
                    "max_col_deg": int(t_deg.max()), "steps": steps, "rounds": rounds, "torch_steps": torch_steps}
            for k, (v, spread) in ms.items():
                line[f"{k}_ms"] = round(v, 4)
                line[f"{k}_spread"] = round(spread, 3)
            line["multi_bytes"] = nbytes
            line["multi_share_of_8TBps"] = round(nbytes / (ms["multi"][0] * 1e-3) / HBM_BYTES_PER_S, 4)
            line["torch_ms"] = None if torch_ms is None else round(torch_ms, 4)
            line["torch_out_of_memory"] = torch_ms is None
            line["existing_over_multi"] = round(ms["existing"][0] / ms["multi"][0], 3)
            line["multi_over_max_alone"] = round(ms["multi"][0] / ms["max_alone"][0], 3)
            line["two_launch_over_multi"] = round(ms["two_launch"][0] / ms["multi"][0], 3)
            line["torch_over_multi"] = None if torch_ms is None else round(torch_ms / ms["multi"][0], 3)
            line["existing_bwd_over_multi_bwd"] = round(ms["existing_bwd"][0] / ms["multi_bwd"][0], 3)
            text = json.dumps(line)
            print(text, flush=True)
            if sink is not None:
                sink.write(text + "\n")
                sink.flush()
            del feat, grads, out, state, naive, g, s1, s2
            torch.cuda.empty_cache()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", nargs="*", default=list(DEFAULT_CASES), help="synth_graphs stand-in names")
    ap.add_argument("--widths", nargs="*", type=int, default=[64, 128])
    ap.add_argument("--dtypes", nargs="*", default=["fp16", "fp32"], choices=sorted(DTYPES))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch-steps", type=int, default=2, help="timed steps of the torch composite")
    ap.add_argument("--scale", type=float, default=1.0, help="synth_graphs scale of every stand-in")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "spmm_multi", "results.jsonl"))
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_spmm_multi.py needs a GPU"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as sink:
        for name in args.cases:
            run_graph(name, args.widths, args.dtypes, args.steps, args.warmup, args.rounds, args.torch_steps, args.scale, sink)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
