#!/usr/bin/env python3
"""Time the edge softmax (``voltrix.edge_softmax`` and its backward) against the torch composite it replaces, on synth_graphs stand-ins.

Per graph, over ``--steps`` warmed steps bracketed by device events:
  * forward: ``voltrix.edge_softmax(indptr, scores, scale)``; backward: ``voltrix.edge_softmax.edge_softmax_backward``;
  * the torch composite with an int64 row id per edge: ``scatter_reduce`` amax, ``exp``, ``index_add`` of the sums, a division --
    forward alone, and its backward through torch autograd.
One JSON line per graph: milliseconds, the byte models 8 nnz + 4 (n + 1) (forward) and 12 nnz + 4 (n + 1) (backward), their share of
8 TB/s, ns per edge, and the composite's times and ratios.  Kernel-only times come from a separate ``rocprofv3 --kernel-trace --stats``
run of this script."""
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
from voltrix.edge_softmax import edge_softmax_backward  # noqa: E402

DEFAULT_CASES = ("yeasth_like", "amazon0601_like", "dd_like", "web_berkstan_like", "reddit_like")
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


def torch_edge_softmax(rows, n, s):
    """The composite users write by hand (what tests/test_gpu_sddmm.py's attention layer does)."""
    m = torch.full((n,), -float("inf"), device=s.device, dtype=s.dtype).scatter_reduce(0, rows, s, "amax")
    e = torch.exp(s - m[rows])
    return e / torch.zeros(n, device=s.device, dtype=s.dtype).index_add(0, rows, e)[rows]


def run_case(name, steps, warmup, scale):
    indptr, _, _ = synth_graphs.generate(name, device="cuda", scale=scale)
    n, nnz = indptr.numel() - 1, int(indptr[-1])
    torch.manual_seed(0)
    scores = torch.randn(nnz, device="cuda") * 4
    grad = torch.randn(nnz, device="cuda")
    sc = 0.125
    alpha = voltrix.edge_softmax(indptr, scores, sc)
    fwd_ms = _time(lambda: voltrix.edge_softmax(indptr, scores, sc), steps, warmup)
    bwd_ms = _time(lambda: edge_softmax_backward(indptr, alpha, grad, sc), steps, warmup)
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), (indptr[1:] - indptr[:-1]).long())
    t_fwd_ms = _time(lambda: torch_edge_softmax(rows, n, scores * sc), steps, warmup)
    leaf = scores.clone().requires_grad_(True)
    out = torch_edge_softmax(rows, n, leaf * sc)

    def torch_backward():
        leaf.grad = None
        out.backward(grad, retain_graph=True)

    t_bwd_ms = _time(torch_backward, steps, warmup)
    del rows, out, leaf
    fwd_bytes, bwd_bytes = 8 * nnz + 4 * (n + 1), 12 * nnz + 4 * (n + 1)
    return {"graph": name, "num_rows": n, "nnz": nnz, "max_deg": int((indptr[1:] - indptr[:-1]).max()),
            "fwd_ms": round(fwd_ms, 4), "bwd_ms": round(bwd_ms, 4), "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes,
            "fwd_share_of_8TBps": round(fwd_bytes / (fwd_ms * 1e-3) / HBM_BYTES_PER_S, 4),
            "bwd_share_of_8TBps": round(bwd_bytes / (bwd_ms * 1e-3) / HBM_BYTES_PER_S, 4),
            "fwd_ns_per_edge": round(fwd_ms * 1e6 / nnz, 5), "bwd_ns_per_edge": round(bwd_ms * 1e6 / nnz, 5),
            "torch_fwd_ms": round(t_fwd_ms, 4), "torch_bwd_ms": round(t_bwd_ms, 4),
            "torch_fwd_share_of_8TBps": round(fwd_bytes / (t_fwd_ms * 1e-3) / HBM_BYTES_PER_S, 4),
            "torch_bwd_share_of_8TBps": round(bwd_bytes / (t_bwd_ms * 1e-3) / HBM_BYTES_PER_S, 4),
            "speedup_fwd": round(t_fwd_ms / fwd_ms, 3), "speedup_bwd": round(t_bwd_ms / bwd_ms, 3)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", nargs="*", default=list(DEFAULT_CASES), help="synth_graphs stand-in names")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="synth_graphs scale of every stand-in")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_edge_softmax.py needs a GPU"
    for name in args.cases:
        print(json.dumps(run_case(name, args.steps, args.warmup, args.scale)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
