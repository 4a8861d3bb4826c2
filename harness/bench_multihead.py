#!/usr/bin/env python3
"""Time the multi-head attention operators against the loop over heads with the single-head operators, on synth_graphs stand-ins.

Per graph and (H, D), fp16 features, over ``--steps`` warmed steps bracketed by device events, one process:
  * heads: ``autograd.SDDMM`` on [n, H, D], ``autograd.EdgeSoftmax`` on [nnz, H], ``autograd.SpMMHeads`` -- forward and backward of each,
    and one whole attention layer ``SpMMHeads(EdgeSoftmax(SDDMM(q, k), D^-0.5), v)`` forward + backward;
  * loop: the same through ``autograd.SDDMM`` / ``EdgeSoftmax`` / ``SpMM(values=)`` once per head on contiguous per-head slices (the
    slicing is part of the loop: the single-head kernels take rows with stride D), results stacked back to [.., H, ..].
One JSON line per (graph, H, D): milliseconds, ns per edge and head, the byte model of every multi-head operator and its share of
8 TB/s, the loop's times and the ratios.  ``--single-head`` adds H = 1 through the new kernels beside the old ones (five repeats of the
old kernel give the run-to-run spread).  Kernel-only times come from a separate ``rocprofv3 --kernel-trace --stats`` run of this script.

Byte models (fp16 features, fp32 edge tensors, int32 CSR):
  sddmm        4 (n + 1) + 4 nnz + 2 nnz H D (gathered rows of k) + 2 n H D (q) + 4 nnz H
  softmax      forward 8 nnz H + 4 (n + 1); backward 12 nnz H + 4 (n + 1)
  aggregation  4 (n + 1) + 4 nnz + 4 nnz H + 2 nnz H D (gathered rows) + 4 n H D"""
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
from voltrix.autograd import SDDMM, EdgeSoftmax, SpMM, SpMMHeads  # noqa: E402
from voltrix.edge_softmax import edge_softmax_backward  # noqa: E402
from voltrix.sddmm import csr_values_product  # noqa: E402

DEFAULT_CASES = ("amazon0601_like", "web_berkstan_like", "reddit_like")
DEFAULT_SHAPES = ("8x8", "8x16", "4x64")
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


def _forward_backward(make, leaves, grads, steps, warmup):
    """ms of ``make()`` (forward, no graph recorded) and of the backward of one recorded forward into ``leaves``."""
    with torch.no_grad():
        fwd = _time(make, steps, warmup)
    outs = make()
    outs = list(outs) if isinstance(outs, (list, tuple)) else [outs]

    def backward():
        for t in leaves:
            t.grad = None
        torch.autograd.backward(outs, grads, retain_graph=True)

    return fwd, _time(backward, steps, warmup)


class Ops:
    """Both forms on one graph: built once (the device CSR, its transpose, and for the loop the block-format handles of A and A^T)."""

    def __init__(self, indptr, indices, n):
        self.sddmm, self.softmax, self.heads = SDDMM(indptr, indices, n), EdgeSoftmax(indptr, n), SpMMHeads(indptr, indices, n)
        self.single = SpMM(indptr, indices, n, values=torch.ones(indices.numel(), device="cuda"), hash_tag="bench_multihead")

    def layer_heads(self, q, k, v, scale):
        return self.heads(v, self.softmax(self.sddmm(q, k), scale))

    def layer_loop(self, q, k, v, scale):
        outs = []
        for h in range(q.shape[1]):
            alpha = self.softmax(self.sddmm(q[:, h].contiguous(), k[:, h].contiguous()), scale)
            outs.append(self.single(v[:, h].contiguous(), values=alpha))
        return torch.stack(outs, 1)


def run_case(name, ops, indptr, indices, heads, dim, steps, warmup):
    n, nnz = indptr.numel() - 1, indices.numel()
    torch.manual_seed(0)
    leaf = lambda *shape, dtype=torch.float32: torch.randn(*shape, device="cuda").to(dtype).requires_grad_(True)     # noqa: E731
    q, k, v = (leaf(n, heads, dim, dtype=torch.float16) for _ in range(3))
    scores, alpha_in = leaf(nnz, heads), leaf(nnz, heads)
    g_edge, g_node = torch.randn(nnz, heads, device="cuda"), torch.randn(n, heads, dim, device="cuda")
    scale = dim ** -0.5
    cols = lambda t: [t[:, h].contiguous() for h in range(heads)]      # noqa: E731
    res = {"graph": name, "num_rows": n, "nnz": nnz, "max_deg": int((indptr[1:] - indptr[:-1]).max()), "heads": heads, "head_dim": dim}
    ms = {}
    # multi-head: one launch per operator
    ms["sddmm_fwd"], ms["sddmm_bwd"] = _forward_backward(lambda: ops.sddmm(q, k), (q, k), [g_edge], steps, warmup)
    ms["softmax_fwd"], ms["softmax_bwd"] = _forward_backward(lambda: ops.softmax(scores, scale), (scores,), [g_edge], steps, warmup)
    ms["agg_fwd"], ms["agg_bwd"] = _forward_backward(lambda: ops.heads(v, alpha_in), (v, alpha_in), [g_node], steps, warmup)

    def layer(form):
        for t in (q, k, v):
            t.grad = None
        form(q, k, v, scale).backward(g_node)

    ms["layer"] = _time(lambda: layer(ops.layer_heads), steps, warmup)
    # the loop over heads with the single-head operators
    loop = {}
    loop["sddmm_fwd"], loop["sddmm_bwd"] = _forward_backward(
        lambda: [ops.sddmm(a, b) for a, b in zip(cols(q), cols(k))], (q, k), cols(g_edge), steps, warmup)
    loop["softmax_fwd"], loop["softmax_bwd"] = _forward_backward(
        lambda: [ops.softmax(s, scale) for s in cols(scores)], (scores,), cols(g_edge), steps, warmup)
    loop["agg_fwd"], loop["agg_bwd"] = _forward_backward(
        lambda: [ops.single(f, values=a) for f, a in zip(cols(v), cols(alpha_in))], (v, alpha_in), cols(g_node), steps, warmup)
    loop["layer"] = _time(lambda: layer(ops.layer_loop), steps, warmup)
    node, edge = n * heads * dim, nnz * heads
    model = {"sddmm_fwd": 4 * (n + 1) + 4 * nnz + 2 * edge * dim + 2 * node + 4 * edge,
             "softmax_fwd": 8 * edge + 4 * (n + 1), "softmax_bwd": 12 * edge + 4 * (n + 1),
             "agg_fwd": 4 * (n + 1) + 4 * nnz + 4 * edge + 2 * edge * dim + 4 * node}
    for key, value in ms.items():
        res[key + "_ms"] = round(value, 4)
        res["loop_" + key + "_ms"] = round(loop[key], 4)
        res["ratio_" + key] = round(loop[key] / value, 3)
        if key != "layer":
            res[key + "_ns_per_edge_head"] = round(value * 1e6 / edge, 5)
        if key in model:
            res[key + "_bytes"] = model[key]
            res[key + "_share_of_8TBps"] = round(model[key] / (value * 1e-3) / HBM_BYTES_PER_S, 4)
    res["agg_fwd_ns_per_edge"] = round(ms["agg_fwd"] * 1e6 / nnz, 5)
    return res


def run_single_head(name, indptr, indices, dim, steps, warmup):
    """H = 1 through the new kernels (C-ABI, heads = 1) beside the old kernels; five repeats of the old kernel give the spread."""
    from voltrix import capi
    from voltrix.jit_kernels.spmm import _raw_stream

    n, nnz = indptr.numel() - 1, indices.numel()
    torch.manual_seed(0)
    x, y = (torch.randn(n, dim, device="cuda").half() for _ in range(2))
    scores, grad = torch.randn(nnz, device="cuda") * 4, torch.randn(nnz, device="cuda")
    out = torch.empty(nnz, 1, device="cuda")
    ws = torch.empty(capi.edge_softmax_heads_workspace_bytes(n, nnz, 1), dtype=torch.uint8, device="cuda")
    stream = _raw_stream(x.device)
    alpha = voltrix.edge_softmax(indptr, scores, 0.125)
    old = {"sddmm": lambda: voltrix.sddmm(indptr, indices, x, y),
           "softmax_fwd": lambda: voltrix.edge_softmax(indptr, scores, 0.125),
           "softmax_bwd": lambda: edge_softmax_backward(indptr, alpha, grad, 0.125),
           "agg": lambda: csr_values_product(indptr, indices, scores, n, x)}
    new = {"sddmm": lambda: voltrix.sddmm(indptr, indices, x.view(n, 1, dim), y.view(n, 1, dim)),
           "softmax_fwd": lambda: capi.launch_edge_softmax_heads_csr(indptr, n, scores.view(nnz, 1), 0.125, out, ws, stream),
           "softmax_bwd": lambda: capi.launch_edge_softmax_heads_backward_csr(indptr, n, alpha.view(nnz, 1), grad.view(nnz, 1), 0.125, out,
                                                                             ws, stream),
           "agg": lambda: voltrix.spmm_heads(indptr, indices, scores.view(nnz, 1), x.view(n, 1, dim), n)}
    res = {"graph": name, "num_rows": n, "nnz": nnz, "heads": 1, "head_dim": dim}
    for key in old:
        repeats = [_time(old[key], steps, warmup) for _ in range(5)]
        res[f"old_{key}_ms"] = [round(t, 4) for t in repeats]
        res[f"new_{key}_ms"] = round(_time(new[key], steps, warmup), 4)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", nargs="*", default=list(DEFAULT_CASES), help="synth_graphs stand-in names")
    ap.add_argument("--shapes", nargs="*", default=list(DEFAULT_SHAPES), help="HxD, e.g. 8x16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="synth_graphs scale of every stand-in")
    ap.add_argument("--single-head", action="store_true", help="also H = 1 through the new kernels beside the old ones (D = 64)")
    ap.add_argument("--heads-only", action="store_true", help="one pass of the multi-head layer per case and shape (for a kernel trace)")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_multihead.py needs a GPU"
    for name in args.cases:
        indptr, indices, _ = synth_graphs.generate(name, device="cuda", scale=args.scale)
        indptr, indices = indptr.int(), indices.int()
        if args.single_head:
            print(json.dumps(run_single_head(name, indptr, indices, 64, args.steps, args.warmup)), flush=True)
        if args.heads_only:
            n = indptr.numel() - 1
            sddmm, softmax, heads_op = SDDMM(indptr, indices, n), EdgeSoftmax(indptr, n), SpMMHeads(indptr, indices, n)
            for heads, dim in (tuple(int(t) for t in s.split("x")) for s in args.shapes):
                q, k, v = (torch.randn(n, heads, dim, device="cuda").half().requires_grad_(True) for _ in range(3))
                for _ in range(args.warmup + args.steps):
                    heads_op(v, softmax(sddmm(q, k), dim ** -0.5)).backward(torch.ones(n, heads, dim, device="cuda"))
            torch.cuda.synchronize()
            continue
        ops = Ops(indptr, indices, indptr.numel() - 1)
        for heads, dim in (tuple(int(t) for t in s.split("x")) for s in args.shapes):
            print(json.dumps(run_case(name, ops, indptr, indices, heads, dim, args.steps, args.warmup)), flush=True)
            torch.cuda.empty_cache()
        del ops
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
