#!/usr/bin/env python3
"""Time the GATv2 edge scores (``voltrix.gatv2_score``) and the two gated row sums of their backward, beside ``voltrix.sddmm`` at the same
shape and beside the torch composite they replace where that fits in memory, on synth_graphs stand-ins with self loops, in fp16.

Per graph and ``(H, D)``, over ``--steps`` warmed steps bracketed by device events:
  * forward ``voltrix.gatv2_score``; ``G_l`` = ``gatv2_rowsum`` on the CSR; ``G_r`` = the same on the transposed CSR with the int32
    transposed edge order; ``voltrix.sddmm`` on the same operands (the same bytes; the forward's reference);
  * the torch composite with cached int64 row and column ids, ``(a * leaky_relu(xl[rows] + xr[cols])).sum(-1)`` -- forward alone, and
    its backward through torch autograd with only ``xl`` or only ``xr`` requiring a gradient -- over ``--torch-steps`` steps, when its
    [nnz, H, D] intermediates fit in the free device memory; else the line says "does not fit".
One JSON line per point: milliseconds, ns per edge and head, the byte models (forward: 4 (n + 1) + 4 nnz + 2 nnz H D + 2 n H D + 4 nnz H;
row sum: 4 (n + 1) + 4 nnz [+ 4 nnz for the order] + 2 nnz H D + 4 nnz H + 6 n H D) and their share of 8 TB/s, the ratio to sddmm, and
the composite's times and ratios."""
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
from voltrix.autograd import CsrPattern  # noqa: E402
from voltrix.gatv2_score import gatv2_rowsum  # noqa: E402

DEFAULT_CASES = ("amazon0601_like", "web_berkstan_like", "reddit_like")
DEFAULT_SHAPES = ("1x64", "8x8", "4x64")
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


def _composite(rows, cols, xl, xr, a):
    return (a * torch.nn.functional.leaky_relu(xl[rows] + xr[cols], SLOPE)).sum(-1)


def _torch_backward_ms(rows, cols, xl, xr, a, grad, side, steps, warmup):
    """The composite's backward through autograd with a gradient for one side only (it keeps [nnz, H, D] alive between the passes)."""
    p, q = xl.clone().requires_grad_(side == "l"), xr.clone().requires_grad_(side == "r")
    out = _composite(rows, cols, p, q, a)
    leaf = p if side == "l" else q

    def step():
        leaf.grad = None
        out.backward(grad, retain_graph=True)

    return _time(step, steps, warmup)


def run_graph(name, shapes, steps, warmup, torch_steps, scale):
    from gat_train import with_self_loops

    indptr, indices, _ = synth_graphs.generate(name, device="cuda", scale=scale)
    n = indptr.numel() - 1
    indptr, indices = with_self_loops(indptr, indices, n)
    nnz = indices.numel()
    pattern = CsrPattern(indptr, indices, n)
    t_indptr, t_indices, t_order = pattern.t_indptr, pattern.t_indices, pattern.t_order
    deg, t_deg = indptr[1:] - indptr[:-1], t_indptr[1:] - t_indptr[:-1]
    for heads, dim in shapes:
        torch.manual_seed(0)
        xl, xr = torch.randn(n, heads, dim, device="cuda").half(), torch.randn(n, heads, dim, device="cuda").half()
        a, grad = torch.randn(heads, dim, device="cuda"), torch.randn(nnz, heads, device="cuda")
        ms = {"fwd": _time(lambda: voltrix.gatv2_score(indptr, indices, xl, xr, a, SLOPE), steps, warmup),
              "G_l": _time(lambda: gatv2_rowsum(indptr, indices, xl, xr, grad, SLOPE), steps, warmup),
              "G_r": _time(lambda: gatv2_rowsum(t_indptr, t_indices, xr, xl, grad, SLOPE, order=t_order), steps, warmup)}
        sddmm_ms = _time(lambda: voltrix.sddmm(indptr, indices, xl, xr), steps, warmup)
        hd = heads * dim
        rowsum = 4 * (n + 1) + 4 * nnz + 2 * nnz * hd + 4 * nnz * heads + 6 * n * hd
        nbytes = {"fwd": 4 * (n + 1) + 4 * nnz + 2 * nnz * hd + 2 * n * hd + 4 * nnz * heads, "G_l": rowsum, "G_r": rowsum + 4 * nnz}
        line = {"graph": name, "heads": heads, "head_dim": dim, "num_rows": n, "nnz": nnz, "max_deg": int(deg.max()),
                "max_col_deg": int(t_deg.max())}
        for k in ("fwd", "G_l", "G_r"):
            line[f"{k}_ms"] = round(ms[k], 4)
            line[f"{k}_ns_per_edge_head"] = round(ms[k] * 1e6 / (nnz * heads), 5)
            line[f"{k}_bytes"] = nbytes[k]
            line[f"{k}_share_of_8TBps"] = round(nbytes[k] / (ms[k] * 1e-3) / HBM_BYTES_PER_S, 4)
        line["sddmm_ms"] = round(sddmm_ms, 4)
        line["fwd_over_sddmm"] = round(ms["fwd"] / sddmm_ms, 3)
        # the composite: int64 ids (16 nnz) and, in fp16, xl[rows], xr[cols], their sum, its leaky_relu, the product with a (kept for the
        # backward) and one more [nnz, H, D] gradient in flight
        need = 16 * nnz + 6 * 2 * nnz * hd
        free = torch.cuda.mem_get_info()[0]
        line["torch_bytes_needed"] = need
        if torch_steps > 0 and need < 0.8 * free:
            rows = torch.repeat_interleave(torch.arange(n, device="cuda"), deg.long())
            cols = indices.long()
            ah = a.half()
            t_ms = {"fwd": _time(lambda: _composite(rows, cols, xl, xr, ah), torch_steps, 1),
                    "G_l": _torch_backward_ms(rows, cols, xl, xr, ah, grad.half(), "l", torch_steps, 1),
                    "G_r": _torch_backward_ms(rows, cols, xl, xr, ah, grad.half(), "r", torch_steps, 1)}
            del rows, cols
            for k in ("fwd", "G_l", "G_r"):
                line[f"torch_{k}_ms"] = round(t_ms[k], 4)
                line[f"speedup_{k}"] = round(t_ms[k] / ms[k], 3)
        else:
            line["torch"] = "does not fit" if torch_steps > 0 else "not run"
        print(json.dumps(line), flush=True)
        del xl, xr, grad
        torch.cuda.empty_cache()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", nargs="*", default=list(DEFAULT_CASES), help="synth_graphs stand-in names")
    ap.add_argument("--shapes", nargs="*", default=list(DEFAULT_SHAPES), help="HxD, e.g. 8x8")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--torch-steps", type=int, default=3, help="steps of the torch composite (after one warm-up); 0 skips it")
    ap.add_argument("--scale", type=float, default=1.0, help="synth_graphs scale of every stand-in")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_gatv2.py needs a GPU"
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes]
    for name in args.cases:
        run_graph(name, shapes, args.steps, args.warmup, args.torch_steps, args.scale)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
