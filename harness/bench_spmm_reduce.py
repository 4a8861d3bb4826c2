#!/usr/bin/env python3
"""Time the max / mean neighbour aggregation (``voltrix.spmm_reduce``) and the max backward against the torch composite they replace
and against this package's own sum kernel, on synth_graphs stand-ins.

Per graph, width (F = 64, 128) and dtype (fp16, fp32), over warmed steps bracketed by device events, in one process on one GPU:
  * forward ``spmm_reduce(..., "max", return_arg=True)`` (writes ``out`` and ``arg``), ``"max"`` without ``arg``, and ``"mean"``;
  * the max backward ``spmm_reduce_backward`` on the transposed CSR;
  * baseline (a), the torch composite with cached int64 ids: ``zeros.scatter_reduce(0, rows, feat[cols], "amax", include_self=False)``
    -- ``feat[cols]`` is a materialised [nnz, F] tensor -- and its backward through torch autograd;
  * baseline (b), ``spmm_csr_rows`` (the sum) on the same input: it reads the same bytes and writes half as many as max with ``arg``.
One JSON line per point: milliseconds, the forward byte model 4 (n + 1) + 4 nnz + nnz F sizeof(T) + 8 n F (4 n F without ``arg``, and
for the sum) and its share of 8 TB/s, the composite's times and the ratios.  The composite gets ``--torch-steps`` steps (its [nnz, F]
temporaries make a step cost seconds on the large graph); where they do not fit the device, the point says so (``torch_out_of_memory``)."""
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
from voltrix.autograd import CsrPattern  # noqa: E402
from voltrix.spmm_reduce import spmm_reduce_backward  # noqa: E402

DEFAULT_CASES = ("amazon0601_like", "web_berkstan_like", "reddit_like")
HBM_BYTES_PER_S = 8e12
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


def _composite(rows, cols, feat, n):
    idx = rows[:, None].expand(-1, feat.shape[1])
    return torch.zeros(n, feat.shape[1], dtype=feat.dtype, device=feat.device).scatter_reduce(0, idx, feat[cols], "amax", include_self=False)


def _composite_backward_ms(rows, cols, feat, n, grad, steps, warmup):
    leaf = feat.clone().requires_grad_(True)
    out = _composite(rows, cols, leaf, n)

    def step():
        leaf.grad = None
        out.backward(grad, retain_graph=True)

    return _time(step, steps, warmup)


def run_graph(name, widths, dtypes, steps, warmup, torch_steps, torch_warmup, scale):
    indptr, indices, _ = synth_graphs.generate(name, device="cuda", scale=scale)
    n = indptr.numel() - 1
    nnz = indices.numel()
    pattern = CsrPattern(indptr, indices, n)
    deg = indptr[1:] - indptr[:-1]
    t_deg = pattern.t_indptr[1:] - pattern.t_indptr[:-1]
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), deg.long())
    cols = indices.long()
    stream = torch.cuda.current_stream().cuda_stream
    for dim in widths:
        for dtype_name in dtypes:
            dtype = DTYPES[dtype_name]
            torch.manual_seed(0)
            feat = torch.randn(n, dim, device="cuda").to(dtype)
            grad = torch.randn(n, dim, device="cuda")
            out, arg = voltrix.spmm_reduce(indptr, indices, feat, n, "max", return_arg=True)
            want = _composite(rows, cols, feat, n)
            assert torch.equal(out, want.float()), "max differs from the composite"
            del want
            sum_out = torch.empty(n, dim, device="cuda")
            ms = {"max_fwd": _time(lambda: voltrix.spmm_reduce(indptr, indices, feat, n, "max", return_arg=True), steps, warmup),
                  "max_fwd_no_arg": _time(lambda: voltrix.spmm_reduce(indptr, indices, feat, n, "max"), steps, warmup),
                  "mean_fwd": _time(lambda: voltrix.spmm_reduce(indptr, indices, feat, n, "mean"), steps, warmup),
                  "max_bwd": _time(lambda: spmm_reduce_backward(pattern.t_indptr, pattern.t_indices, pattern.t_order, grad, arg, n),
                                   steps, warmup),
                  "sum_fwd": _time(lambda: capi.launch_spmm_csr_rows(indptr, indices, n, feat, sum_out, stream, 1), steps, warmup)}
            t_ms = {}
            for k, run in (("max_fwd", lambda: _time(lambda: _composite(rows, cols, feat, n), torch_steps, torch_warmup)),
                           ("max_bwd", lambda: _composite_backward_ms(rows, cols, feat, n, grad.to(dtype), torch_steps, torch_warmup))):
                try:
                    t_ms[k] = run()
                except torch.cuda.OutOfMemoryError:      # the composite's [nnz, F] temporaries do not fit: recorded, not hidden
                    t_ms[k] = None
                    torch.cuda.empty_cache()
            size = feat.element_size()
            gathered = 4 * (n + 1) + 4 * nnz + nnz * dim * size
            nbytes = {"max_fwd": gathered + 8 * n * dim, "max_fwd_no_arg": gathered + 4 * n * dim, "mean_fwd": gathered + 4 * n * dim,
                      "sum_fwd": gathered + 4 * n * dim}
            line = {"graph": name, "scale": scale, "F": dim, "dtype": dtype_name, "num_rows": n, "nnz": nnz, "max_deg": int(deg.max()),
                    "max_col_deg": int(t_deg.max()), "steps": steps, "torch_steps": torch_steps}
            for k, v in ms.items():
                line[f"{k}_ms"] = round(v, 4)
                if k in nbytes:
                    line[f"{k}_bytes"] = nbytes[k]
                    line[f"{k}_share_of_8TBps"] = round(nbytes[k] / (v * 1e-3) / HBM_BYTES_PER_S, 4)
            for k, v in t_ms.items():
                line[f"torch_{k}_ms"] = None if v is None else round(v, 4)
                line[f"speedup_{k}"] = None if v is None else round(v / ms[k], 3)
            line["torch_out_of_memory"] = [k for k, v in t_ms.items() if v is None]
            line["max_over_sum"] = round(ms["max_fwd"] / ms["sum_fwd"], 3)
            line["max_no_arg_over_sum"] = round(ms["max_fwd_no_arg"] / ms["sum_fwd"], 3)
            line["mean_over_sum"] = round(ms["mean_fwd"] / ms["sum_fwd"], 3)
            line["bytes_max_over_sum"] = round(nbytes["max_fwd"] / nbytes["sum_fwd"], 3)
            print(json.dumps(line), flush=True)
            del feat, grad, out, arg, sum_out
            torch.cuda.empty_cache()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", nargs="*", default=list(DEFAULT_CASES), help="synth_graphs stand-in names")
    ap.add_argument("--widths", nargs="*", type=int, default=[64, 128])
    ap.add_argument("--dtypes", nargs="*", default=["fp16", "fp32"], choices=sorted(DTYPES))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--torch-steps", type=int, default=3, help="timed steps of the torch composite")
    ap.add_argument("--torch-warmup", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0, help="synth_graphs scale of every stand-in")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_spmm_reduce.py needs a GPU"
    for name in args.cases:
        run_graph(name, args.widths, args.dtypes, args.steps, args.warmup, args.torch_steps, args.torch_warmup, args.scale)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
