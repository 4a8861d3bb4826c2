#!/usr/bin/env python3
"""Time the GAT edge scores (``voltrix.gat_score``) and the two segment sums of their backward against the torch composite they replace,
on synth_graphs stand-ins with self loops, at one and at eight heads.

Per graph and head count, over ``--steps`` warmed steps bracketed by device events:
  * forward ``voltrix.gat_score``; ``d_el`` = ``gat_score_backward`` on the CSR; ``d_er`` = the same on the transposed CSR with the
    int32 transposed edge order;
  * the torch composite with cached int64 row and column ids, ``leaky_relu(el[rows] + er[cols])`` -- forward alone, and its backward
    through torch autograd with only ``el`` or only ``er`` requiring a gradient (one ``index_add`` scatter each).
One JSON line per point: milliseconds, ns per edge and head, the byte models (forward and ``d_el``: 4 (n + 1) + 4 nnz + 4 nnz H + the node
tensors; ``d_er``: 4 nnz more for the order) and their share of 8 TB/s, and the composite's times and ratios."""
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
import voltrix  # noqa: E402
from voltrix.autograd import csr_transpose_device  # noqa: E402
from voltrix.gat_score import gat_score_backward  # noqa: E402
from voltrix.weighted import transpose_order  # noqa: E402

DEFAULT_CASES = ("amazon0601_like", "web_berkstan_like", "reddit_like")
HBM_BYTES_PER_S = 8e12
SLOPE = 0.2


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


def _torch_backward_ms(rows, cols, el, er, grad, side, steps, warmup):
    """The composite's backward through autograd with a gradient for one side only."""
    a, b = el.clone().requires_grad_(side == "el"), er.clone().requires_grad_(side == "er")
    out = torch.nn.functional.leaky_relu(a[rows] + b[cols], SLOPE)
    leaf = a if side == "el" else b

    def step():
        leaf.grad = None
        out.backward(grad, retain_graph=True)

    return _time(step, steps, warmup)


def run_graph(name, heads_list, steps, warmup, scale):
    from gat_train import with_self_loops

    indptr, indices, _ = synth_graphs.generate(name, device="cuda", scale=scale)
    n = indptr.numel() - 1
    indptr, indices = with_self_loops(indptr, indices, n)
    nnz = indices.numel()
    t_indptr, t_indices = csr_transpose_device(indptr, indices, n, n)
    t_order = transpose_order(indptr, indices, n).to(torch.int32)
    deg, t_deg = indptr[1:] - indptr[:-1], t_indptr[1:] - t_indptr[:-1]
    for heads in heads_list:
        torch.manual_seed(0)
        el, er, grad = torch.randn(n, heads, device="cuda"), torch.randn(n, heads, device="cuda"), torch.randn(nnz, heads, device="cuda")
        ms = {"fwd": _time(lambda: voltrix.gat_score(indptr, indices, el, er, SLOPE), steps, warmup),
              "d_el": _time(lambda: gat_score_backward(indptr, indices, el, er, grad, SLOPE), steps, warmup),
              "d_er": _time(lambda: gat_score_backward(t_indptr, t_indices, er, el, grad, SLOPE, order=t_order), steps, warmup)}
        rows = torch.repeat_interleave(torch.arange(n, device="cuda"), deg.long())
        cols = indices.long()
        t_ms = {"fwd": _time(lambda: torch.nn.functional.leaky_relu(el[rows] + er[cols], SLOPE), steps, warmup),
                "d_el": _torch_backward_ms(rows, cols, el, er, grad, "el", steps, warmup),
                "d_er": _torch_backward_ms(rows, cols, el, er, grad, "er", steps, warmup)}
        del rows, cols
        base = 4 * (n + 1) + 4 * nnz + 4 * nnz * heads + 8 * n * heads
        nbytes = {"fwd": base, "d_el": base + 4 * n * heads, "d_er": base + 4 * n * heads + 4 * nnz}
        line = {"graph": name, "heads": heads, "num_rows": n, "nnz": nnz, "max_deg": int(deg.max()), "max_col_deg": int(t_deg.max())}
        for k in ("fwd", "d_el", "d_er"):
            line[f"{k}_ms"] = round(ms[k], 4)
            line[f"{k}_ns_per_edge_head"] = round(ms[k] * 1e6 / (nnz * heads), 5)
            line[f"{k}_bytes"] = nbytes[k]
            line[f"{k}_share_of_8TBps"] = round(nbytes[k] / (ms[k] * 1e-3) / HBM_BYTES_PER_S, 4)
            line[f"torch_{k}_ms"] = round(t_ms[k], 4)
            line[f"speedup_{k}"] = round(t_ms[k] / ms[k], 3)
        print(json.dumps(line), flush=True)
        torch.cuda.empty_cache()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", nargs="*", default=list(DEFAULT_CASES), help="synth_graphs stand-in names")
    ap.add_argument("--heads", nargs="*", type=int, default=[1, 8])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="synth_graphs scale of every stand-in")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_gat_score.py needs a GPU"
    for name in args.cases:
        run_graph(name, args.heads, args.steps, args.warmup, args.scale)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
