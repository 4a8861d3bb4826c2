#!/usr/bin/env python3
"""Time attention dropout in the fused softmax-and-aggregate operator, on synth_graphs stand-ins with self loops.

Per graph and (H, D), fp16 features, over ``--steps`` warmed steps bracketed by device events, one process, the same inputs -- forward
(no graph recorded), backward of one recorded forward, and forward + backward of
  (a) ``autograd.AttnAggregate(feat, s, D^-0.5)`` without dropout, measured twice (before and after the others): the difference of the
      two is the run-to-run spread of this process;
  (b) the same with a keep mask of p = 0.1 and p = 0.6 passed as ``mask=`` (generated once, outside the timed loop);
  (c) the unfused chain ``SpMMHeads(feat, apply_dropout_mask(EdgeSoftmax(s, D^-0.5), mask, keep_scale))`` at the same p.
The mask generator is timed alone against the ``4 nnz W`` bytes it writes.  One JSON line per (graph, H, D): milliseconds, the ratios
(c) / (b) (above 1: the fused operator is faster) and (b) - (a) beside the spread of (a) and the time of one stream over ``4 nnz W``
bytes at 8 TB/s per launch that reads the mask (one forward, two backward).  Kernel-only times come from a separate
``rocprofv3 --kernel-trace --stats`` run of this script with ``--fused-only P``."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "voltrix-spmm_amd"), os.path.join(REPO, "examples")):
    sys.path.insert(0, p)
os.environ.setdefault("VOLTRIX_CACHE_DIR", os.path.join(REPO, "voltrix-spmm_amd", ".jit_cache"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import synth_graphs  # noqa: E402
import voltrix  # noqa: E402
from bench_attn_aggregate import _three, _time  # noqa: E402
from gat_train import with_self_loops  # noqa: E402
from voltrix.autograd import AttnAggregate, CsrPattern, EdgeSoftmax, SpMMHeads  # noqa: E402

DEFAULT_CASES = ("amazon0601_like", "web_berkstan_like", "reddit_like")
DEFAULT_SHAPES = ("8x8", "8x16", "4x64")
PROBABILITIES = (0.1, 0.6)
HBM_BYTES_PER_S = 8e12
KEYS = ("fwd", "bwd", "both")
MASK_READS = {"fwd": 1, "bwd": 2, "both": 3}      # launches that read the mask


def run_case(name, fused, softmax, heads_op, heads, dim, steps, warmup):
    n, nnz = fused.num_rows, fused.num_edges
    torch.manual_seed(0)
    feat = torch.randn(n, heads, dim, device="cuda").half().requires_grad_(True)
    scores = (2.0 * torch.randn(nnz, heads, device="cuda")).requires_grad_(True)
    grad = torch.randn(n, heads, dim, device="cuda")
    scale = dim ** -0.5
    words = (heads + 31) // 32
    mask_bytes = 4 * nnz * words
    res = {"graph": name, "num_rows": n, "nnz": nnz, "heads": heads, "head_dim": dim, "mask_bytes": mask_bytes,
           "mask_stream_ms_at_8TBps": round(mask_bytes / HBM_BYTES_PER_S * 1e3, 5)}
    plain = lambda: fused(feat, scores, scale)                                                      # noqa: E731
    first = dict(zip(KEYS, _three(plain, (feat, scores), grad, steps, warmup)))
    for p in PROBABILITIES:
        tag = f"p{p}"
        mask = voltrix.dropout_mask(nnz, heads, p, 1234)
        keep_scale = float(np.float32(1.0) / np.float32(1.0 - p))
        res[f"kept_fraction_{tag}"] = round(float(voltrix.dropout.unpack_mask(mask, heads).float().mean()), 4)
        new = dict(zip(KEYS, _three(lambda: fused(feat, scores, scale, dropout_p=p, mask=mask), (feat, scores), grad, steps, warmup)))
        old = dict(zip(KEYS, _three(lambda: heads_op(feat, voltrix.apply_dropout_mask(softmax(scores, scale), mask, keep_scale)),
                                    (feat, scores), grad, steps, warmup)))
        for key in KEYS:
            res[f"fused_{tag}_{key}_ms"] = round(new[key], 4)
            res[f"unfused_{tag}_{key}_ms"] = round(old[key], 4)
            res[f"ratio_{tag}_{key}"] = round(old[key] / new[key], 3)
        res[f"mask_gen_{tag}_ms"] = round(_time(lambda: voltrix.dropout_mask(nnz, heads, p, 1234), steps, warmup), 5)
        res[f"mask_gen_{tag}_share_of_8TBps"] = round(mask_bytes / (res[f"mask_gen_{tag}_ms"] * 1e-3) / HBM_BYTES_PER_S, 4)
    second = dict(zip(KEYS, _three(plain, (feat, scores), grad, steps, warmup)))
    for key in KEYS:
        res[f"fused_plain_{key}_ms"] = round(min(first[key], second[key]), 4)
        res[f"fused_plain_{key}_spread_ms"] = round(abs(first[key] - second[key]), 4)
        allowance = res[f"fused_plain_{key}_spread_ms"] + MASK_READS[key] * res["mask_stream_ms_at_8TBps"]
        for p in PROBABILITIES:
            over = res[f"fused_p{p}_{key}_ms"] - max(first[key], second[key])
            res[f"over_plain_p{p}_{key}_ms"] = round(over, 4)
            res[f"within_allowance_p{p}_{key}"] = bool(over <= allowance)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", nargs="*", default=list(DEFAULT_CASES), help="synth_graphs stand-in names")
    ap.add_argument("--shapes", nargs="*", default=list(DEFAULT_SHAPES), help="HxD, e.g. 8x16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="synth_graphs scale of every stand-in")
    ap.add_argument("--fused-only", type=float, default=None, metavar="P",
                    help="forward + backward of the fused operator with drop probability P only (for a kernel trace)")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_attn_dropout.py needs a GPU"
    for name in args.cases:
        indptr, indices, _ = synth_graphs.generate(name, device="cuda", scale=args.scale)
        n = indptr.numel() - 1
        indptr, indices = with_self_loops(indptr.int(), indices.int(), n)
        pattern = CsrPattern(indptr, indices, n)
        heads_op, softmax, fused = SpMMHeads(pattern), EdgeSoftmax(pattern), AttnAggregate(pattern)
        for heads, dim in (tuple(int(t) for t in s.split("x")) for s in args.shapes):
            if args.fused_only is not None:
                feat = torch.randn(n, heads, dim, device="cuda").half().requires_grad_(True)
                scores = torch.randn(indices.numel(), heads, device="cuda").requires_grad_(True)
                for step in range(args.warmup + args.steps):
                    fused(feat, scores, dim ** -0.5, dropout_p=args.fused_only, seed=step).backward(torch.ones(n, heads, dim, device="cuda"))
                torch.cuda.synchronize()
                continue
            print(json.dumps(run_case(name, fused, softmax, heads_op, heads, dim, args.steps, args.warmup)), flush=True)
            torch.cuda.empty_cache()
        del fused, heads_op, softmax, pattern
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
