#!/usr/bin/env python3
"""Time the aggregation with a feature vector per edge (``voltrix.spmm_edge``) and its backward against the torch composite they
replace, on synth_graphs stand-ins.

Per graph, width (F = 32, 128), dtype (fp16, fp32) and op (mul, add, add_relu, copy), over warmed steps bracketed by device events, in
one process on one GPU:
  * forward ``spmm_edge``;
  * backward: ``grad_efeat`` and ``grad_feat`` (the two launches ``autograd.SpMMEdge`` makes), timed separately and summed;
  * the torch composite with cached int64 ids, ``zeros.index_add_(0, rows, m(feat[cols], efeat))`` -- ``feat[cols]`` is a materialised
    [nnz, F] tensor -- and its backward for both operands through torch autograd.
One JSON line per point: milliseconds, the forward byte model 4 (n + 1) + 4 nnz + nnz F (sizeof TI + sizeof TE) + 4 n F (copy: no TI
term) and the bytes per second it amounts to, the composite's times and the ratios.  The composite gets ``--torch-steps`` steps; where its
temporaries do not fit the device, the point says so (``torch_out_of_memory``)."""
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
from voltrix.autograd import CsrPattern  # noqa: E402
from voltrix.spmm_edge import OPS, grad_efeat, grad_feat  # noqa: E402

DEFAULT_CASES = ("yeast_like", "dd_like", "amazon0601_like")      # two low-degree molecular / protein stand-ins, one mid-degree
DTYPES = {"fp16": torch.float16, "fp32": torch.float32}


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


def _composite(rows, cols, feat, efeat, n, op):
    if op == "copy":
        terms = efeat
    else:
        x = feat[cols]
        terms = x * efeat if op == "mul" else x + efeat if op == "add" else torch.relu(x + efeat)
    return torch.zeros(n, efeat.shape[1], dtype=efeat.dtype, device=efeat.device).index_add_(0, rows, terms)


def _composite_backward_ms(rows, cols, feat, efeat, n, op, grad, steps, warmup):
    f = None if op == "copy" else feat.clone().requires_grad_(True)
    e = efeat.clone().requires_grad_(True)
    out = _composite(rows, cols, f, e, n, op)

    def step():
        e.grad = None
        if f is not None:
            f.grad = None
        out.backward(grad, retain_graph=True)

    return _time(step, steps, warmup)


def run_graph(name, widths, dtypes, steps, warmup, torch_steps, torch_warmup, scale):
    indptr, indices, _ = synth_graphs.generate(name, device="cuda", scale=scale)
    n, nnz = indptr.numel() - 1, indices.numel()
    pattern = CsrPattern(indptr, indices, n)
    deg = indptr[1:] - indptr[:-1]
    t_deg = pattern.t_indptr[1:] - pattern.t_indptr[:-1]
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), deg.long())
    cols = indices.long()
    t = (pattern.t_indptr, pattern.t_indices, pattern.t_order)
    for dim in widths:
        for dtype_name in dtypes:
            dtype = DTYPES[dtype_name]
            torch.manual_seed(0)
            feat = torch.randn(n, dim, device="cuda").to(dtype)
            efeat = torch.randn(nnz, dim, device="cuda").to(dtype)
            grad = torch.randn(n, dim, device="cuda")
            size = feat.element_size()
            for op in OPS:
                f = None if op == "copy" else feat
                out = voltrix.spmm_edge(indptr, indices, f, efeat, n, op=op)
                want = _composite(rows, cols, None if f is None else f.double(), efeat.double(), n, op)
                worst = float(((out.double() - want).abs() / want.abs().clamp_min(1.0)).max())
                assert worst < 1e-4, (op, worst)
                del out, want
                ms = {"fwd": _time(lambda: voltrix.spmm_edge(indptr, indices, f, efeat, n, op=op), steps, warmup),
                      "bwd_efeat": _time(lambda: grad_efeat(indptr, indices, grad, f, efeat, op), steps, warmup),
                      "bwd_feat": 0.0 if op == "copy" else _time(lambda: grad_feat(*t, grad, feat, efeat, op, n), steps, warmup)}
                ms["bwd"] = ms["bwd_efeat"] + ms["bwd_feat"]
                t_ms = {}
                for k, run in (("fwd", lambda: _time(lambda: _composite(rows, cols, f, efeat, n, op), torch_steps, torch_warmup)),
                               ("bwd", lambda: _composite_backward_ms(rows, cols, feat, efeat, n, op, grad.to(dtype), torch_steps,
                                                                      torch_warmup))):
                    try:
                        t_ms[k] = run()
                    except torch.cuda.OutOfMemoryError:      # the composite's [nnz, F] temporaries do not fit: recorded, not hidden
                        t_ms[k] = None
                        torch.cuda.empty_cache()
                fwd_bytes = 4 * (n + 1) + 4 * nnz + nnz * dim * (size if op == "copy" else 2 * size) + 4 * n * dim
                line = {"graph": name, "scale": scale, "F": dim, "dtype": dtype_name, "op": op, "num_rows": n, "nnz": nnz,
                        "max_deg": int(deg.max()), "max_col_deg": int(t_deg.max()), "steps": steps, "torch_steps": torch_steps,
                        "fwd_bytes": fwd_bytes, "fwd_TB_per_s": round(fwd_bytes / (ms["fwd"] * 1e-3) / 1e12, 3)}
                for k, v in ms.items():
                    line[f"{k}_ms"] = round(v, 4)
                for k, v in t_ms.items():
                    line[f"torch_{k}_ms"] = None if v is None else round(v, 4)
                    line[f"speedup_{k}"] = None if v is None else round(v / ms[k], 3)
                line["torch_out_of_memory"] = [k for k, v in t_ms.items() if v is None]
                print(json.dumps(line), flush=True)
            del feat, efeat, grad
            torch.cuda.empty_cache()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", nargs="*", default=list(DEFAULT_CASES), help="synth_graphs stand-in names")
    ap.add_argument("--widths", nargs="*", type=int, default=[32, 128])
    ap.add_argument("--dtypes", nargs="*", default=["fp16", "fp32"], choices=sorted(DTYPES))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--torch-steps", type=int, default=3, help="timed steps of the torch composite")
    ap.add_argument("--torch-warmup", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0, help="synth_graphs scale of every stand-in")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_spmm_edge.py needs a GPU"
    for name in args.cases:
        run_graph(name, args.widths, args.dtypes, args.steps, args.warmup, args.torch_steps, args.torch_warmup, args.scale)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
