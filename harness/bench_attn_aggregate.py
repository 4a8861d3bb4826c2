#!/usr/bin/env python3
"""Time the fused softmax-and-aggregate operator against the unfused chain it replaces, on synth_graphs stand-ins with self loops.

Per graph and (H, D), fp16 features, over ``--steps`` warmed steps bracketed by device events, one process, the same inputs:
  * fused:   ``autograd.AttnAggregate(feat, s, D^-0.5)`` -- forward (no graph recorded), backward of one recorded forward, and forward +
    backward; the two backward launches (``d_s``, ``d_feat``) and the dense ``delta`` also on their own;
  * unfused: ``autograd.SpMMHeads(feat, autograd.EdgeSoftmax(s, D^-0.5))`` -- the same three times.  This is the yardstick.
One JSON line per (graph, H, D): milliseconds, ns per edge and head, the byte models and their share of 8 TB/s, and the ratios
unfused / fused (above 1: the fused operator is faster).  Kernel-only times come from a separate ``rocprofv3 --kernel-trace --stats`` run
of this script with ``--fused-only``.

Byte models (fp16 features, fp32 edge tensors, int32 CSR):
  forward  4 (n + 1) + 4 nnz + 4 nnz H + 2 nnz H D (gathered rows) + 4 n H D + 8 n H (m, l)
  d_s      the SDDMM's 4 (n + 1) + 4 nnz + 2 nnz H D + 4 n H D (dC, fp32) + 4 nnz H, plus 4 nnz H (the scores)"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "voltrix-spmm_amd"), os.path.join(REPO, "examples")):
    sys.path.insert(0, p)
os.environ.setdefault("VOLTRIX_CACHE_DIR", os.path.join(REPO, "voltrix-spmm_amd", ".jit_cache"))

import torch  # noqa: E402

import synth_graphs  # noqa: E402
from gat_train import with_self_loops  # noqa: E402
from voltrix.attn_aggregate import attn_aggregate, attn_aggregate_grad_feat, attn_aggregate_grad_scores  # noqa: E402
from voltrix.autograd import AttnAggregate, CsrPattern, EdgeSoftmax, SpMMHeads  # noqa: E402

DEFAULT_CASES = ("amazon0601_like", "web_berkstan_like", "reddit_like")
DEFAULT_SHAPES = ("1x64", "8x8", "8x16", "4x64")
HBM_BYTES_PER_S = 8e12


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / steps


def _three(make, leaves, grad, steps, warmup):
    """ms of ``make()`` without a graph, of the backward of one recorded forward, and of forward + backward."""
    with torch.no_grad():
        fwd = _time(make, steps, warmup)
    out = make()

    def backward():
        for t in leaves:
            t.grad = None
        out.backward(grad, retain_graph=True)

    def both():
        for t in leaves:
            t.grad = None
        make().backward(grad)

    return fwd, _time(backward, steps, warmup), _time(both, steps, warmup)


def run_case(name, fused, softmax, heads_op, heads, dim, steps, warmup):
    n, nnz = fused.num_rows, fused.num_edges
    torch.manual_seed(0)
    feat = torch.randn(n, heads, dim, device="cuda").half().requires_grad_(True)
    scores = (2.0 * torch.randn(nnz, heads, device="cuda")).requires_grad_(True)
    grad = torch.randn(n, heads, dim, device="cuda")
    scale = dim ** -0.5
    res = {"graph": name, "num_rows": n, "nnz": nnz, "max_deg": int((fused.indptr[1:] - fused.indptr[:-1]).max()), "heads": heads,
           "head_dim": dim}
    new = dict(zip(("fwd", "bwd", "both"), _three(lambda: fused(feat, scores, scale), (feat, scores), grad, steps, warmup)))
    old = dict(zip(("fwd", "bwd", "both"), _three(lambda: heads_op(feat, softmax(scores, scale)), (feat, scores), grad, steps, warmup)))
    with torch.no_grad():      # the pieces of the fused backward
        f, s = feat.detach(), scores.detach()
        out, m, l = attn_aggregate(fused.indptr, fused.indices, s, f, n, scale, return_stats=True)
        delta = (grad * out).sum(-1)
        res["fused_delta_ms"] = round(_time(lambda: (grad * out).sum(-1), steps, warmup), 4)
        res["fused_d_s_ms"] = round(_time(lambda: attn_aggregate_grad_scores(fused.indptr, fused.indices, grad, f, s, m, l, delta, scale),
                                          steps, warmup), 4)
        res["fused_d_feat_ms"] = round(_time(lambda: attn_aggregate_grad_feat(fused.t_indptr, fused.t_indices, fused.t_order, grad, s, m, l,
                                                                             n, scale), steps, warmup), 4)
    node, edge = n * heads * dim, nnz * heads
    model = {"fwd": 4 * (n + 1) + 4 * nnz + 4 * edge + 2 * edge * dim + 4 * node + 8 * n * heads,
             "d_s": 4 * (n + 1) + 4 * nnz + 2 * edge * dim + 4 * node + 4 * edge + 4 * edge}
    for key in ("fwd", "bwd", "both"):
        res[f"fused_{key}_ms"] = round(new[key], 4)
        res[f"unfused_{key}_ms"] = round(old[key], 4)
        res[f"ratio_{key}"] = round(old[key] / new[key], 3)
        res[f"fused_{key}_ns_per_edge_head"] = round(new[key] * 1e6 / edge, 5)
    res["fwd_bytes"], res["d_s_bytes"] = model["fwd"], model["d_s"]
    res["fwd_share_of_8TBps"] = round(model["fwd"] / (new["fwd"] * 1e-3) / HBM_BYTES_PER_S, 4)
    res["d_s_share_of_8TBps"] = round(model["d_s"] / (res["fused_d_s_ms"] * 1e-3) / HBM_BYTES_PER_S, 4)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", nargs="*", default=list(DEFAULT_CASES), help="synth_graphs stand-in names")
    ap.add_argument("--shapes", nargs="*", default=list(DEFAULT_SHAPES), help="HxD, e.g. 8x16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="synth_graphs scale of every stand-in")
    ap.add_argument("--fused-only", action="store_true", help="forward + backward of the fused operator only (for a kernel trace)")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_attn_aggregate.py needs a GPU"
    for name in args.cases:
        indptr, indices, _ = synth_graphs.generate(name, device="cuda", scale=args.scale)
        n = indptr.numel() - 1
        indptr, indices = with_self_loops(indptr.int(), indices.int(), n)
        pattern = CsrPattern(indptr, indices, n)
        heads_op, softmax, fused = SpMMHeads(pattern), EdgeSoftmax(pattern), AttnAggregate(pattern)
        for heads, dim in (tuple(int(t) for t in s.split("x")) for s in args.shapes):
            if args.fused_only:
                feat = torch.randn(n, heads, dim, device="cuda").half().requires_grad_(True)
                scores = torch.randn(indices.numel(), heads, device="cuda").requires_grad_(True)
                for _ in range(args.warmup + args.steps):
                    fused(feat, scores, dim ** -0.5).backward(torch.ones(n, heads, dim, device="cuda"))
                torch.cuda.synchronize()
                continue
            print(json.dumps(run_case(name, fused, softmax, heads_op, heads, dim, args.steps, args.warmup)), flush=True)
            torch.cuda.empty_cache()
        del fused, heads_op, softmax, pattern
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
