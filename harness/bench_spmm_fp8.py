#!/usr/bin/env python3
"""Time the FP8 aggregation against the two 16-bit baselines it has to beat, on synth_graphs stand-ins:

  * ``csr_rows_f16``: ``voltrix_launch_spmm_csr_rows`` on fp16 rows -- the same geometry at twice the gathered bytes;
  * ``spmm_f16``: ``voltrix.spmm`` on the fp16 handle, whatever path it picks (block format, stream, panel, row gather);
  * ``fp8_out32`` / ``fp8_out16``: ``voltrix.spmm_fp8`` on rows quantised once, fp32 and fp16 output;
  * ``quantize``: ``voltrix.quantize_fp8(feat16, "column")`` alone -- what a layer that re-quantises its activations pays on top.

Per graph and width, in one process on one GPU: ``--rounds`` windows of ``--steps`` warmed calls bracketed by device events; the median
window in milliseconds with the smallest and the largest.  One JSON line per point, with the ratios ``baseline / fp8`` (above 1: fp8 is
faster) and the byte model's expectation: per row ``deg * (F * b + 4) + F * o`` bytes for ``b`` bytes per gathered feature and ``o``
per output feature (the gather halves; the index and the output do not)."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "voltrix-spmm_amd")):
    sys.path.insert(0, p)
os.environ.setdefault("VOLTRIX_CACHE_DIR", os.path.join(REPO, "voltrix-spmm_amd", ".jit_cache"))

import torch  # noqa: E402

import synth_graphs  # noqa: E402
import voltrix  # noqa: E402
from voltrix import capi  # noqa: E402

DEFAULT_CASES = ("amazon0601_like", "dd_like", "web_berkstan_like", "reddit_like")


def _windows(fn, steps, warmup, rounds):
    """Milliseconds per call in each of ``rounds`` windows of ``steps`` calls, by device events."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(steps):
            fn()
        end.record()
        end.synchronize()
        out.append(start.elapsed_time(end) / steps)
    return out


def _stats(key, ms):
    ms = sorted(ms)
    return {f"{key}_ms": round(ms[len(ms) // 2], 4), f"{key}_ms_min": round(ms[0], 4), f"{key}_ms_max": round(ms[-1], 4)}


def run_graph(name, widths, steps, warmup, rounds, scale):
    indptr, indices, _ = synth_graphs.generate(name, device="cuda", scale=scale)
    n, nnz = indptr.numel() - 1, indices.numel()
    deg = indptr[1:] - indptr[:-1]
    handle = voltrix.csr_preprocess_device(indptr, indices, n)
    handle[1].hash_tag = f"bench_spmm_fp8/{name}/{scale}"
    stream = torch.cuda.current_stream().cuda_stream
    for dim in widths:
        torch.manual_seed(1)
        feat = torch.randn(n, dim, device="cuda").half()
        rows = voltrix.quantize_fp8(feat, "column")
        out32 = torch.empty(n, dim, device="cuda")
        line = {"graph": name, "scale": scale, "F": dim, "num_rows": n, "nnz": nnz, "mean_deg": round(nnz / n, 2), "max_deg": int(deg.max()),
                "steps": steps, "rounds": rounds}
        runs = {
            "csr_rows_f16": lambda: capi.launch_spmm_csr_rows(indptr, indices, n, feat, out32, stream, 1),
            "spmm_f16": lambda: voltrix.spmm(*handle, num_nodes=n, num_edges=nnz, feat=feat),
            "fp8_out32": lambda: voltrix.spmm_fp8(indptr, indices, rows, n),
            "fp8_out16": lambda: voltrix.spmm_fp8(indptr, indices, rows, n, out_dtype=torch.float16),
            "quantize": lambda: voltrix.quantize_fp8(feat, "column"),
        }
        # the operators compute the same product up to the quantisation: the stated bound per term, summed over the row by the same
        # kernel, plus the fp32 rounding of two sums of this length
        runs["csr_rows_f16"]()
        want = out32.clone()
        got = runs["fp8_out32"]()
        per_term = (2.0 ** -4 + 2.0 ** -20) * feat.float().abs() + 2.0 ** -10 * rows.scale[:dim]
        bound = torch.empty_like(out32)
        capi.launch_spmm_csr_rows(indptr, indices, n, per_term.contiguous(), bound, stream, 1)
        bound = bound * (1 + 1e-3) + 1e-3 * want.abs()
        err = (got - want).abs()
        assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-30)).max())
        line["fp8_vs_f16_err_over_bound"] = round(float((err / bound.clamp_min(1e-30)).max()), 3)
        del per_term, bound, err
        for key, fn in runs.items():
            line.update(_stats(key, _windows(fn, steps, warmup, rounds)))
        for base in ("csr_rows_f16", "spmm_f16"):
            for ours in ("fp8_out32", "fp8_out16"):
                line[f"{base}_over_{ours}"] = round(line[f"{base}_ms"] / line[f"{ours}_ms"], 3)
        line["quantize_over_fp8_out16"] = round(line["quantize_ms"] / line["fp8_out16_ms"], 3)
        # the byte model: gathered rows + indices + output, per row of mean degree
        d = nnz / n
        model = lambda b, o: d * (dim * b + 4) + dim * o      # noqa: E731
        line["model_f16_over_fp8_out32"] = round(model(2, 4) / model(1, 4), 3)
        line["model_f16_over_fp8_out16"] = round(model(2, 4) / model(1, 2), 3)
        print(json.dumps(line), flush=True)
        del feat, rows, out32, want, got
        torch.cuda.empty_cache()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", nargs="*", default=list(DEFAULT_CASES), help="synth_graphs stand-in names")
    ap.add_argument("--widths", nargs="*", type=int, default=[128, 512])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="synth_graphs scale of every stand-in")
    ap.add_argument("--scale-of", nargs="*", default=["reddit_like=0.25"], help="NAME=SCALE overrides of --scale")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_spmm_fp8.py needs a GPU"
    scale_of = dict(item.split("=") for item in args.scale_of)
    for name in args.cases:
        run_graph(name, args.widths, args.steps, args.warmup, args.rounds, float(scale_of.get(name, args.scale)))
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
