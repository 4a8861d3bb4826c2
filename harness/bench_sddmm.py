#!/usr/bin/env python3
"""Time the sampled dense-dense product (``voltrix.sddmm``) against the two SpMMs that gather the same rows, on synth_graphs stand-ins.

Per (graph, width), over ``--steps`` warmed steps bracketed by device events:
  * ``voltrix.sddmm`` with x fp32 and y fp16 -- the gradient of a weighted SpMM with respect to its values (dC fp32, B fp16);
  * the binary CSR row-gather SpMM (``capi.launch_spmm_csr_rows``, XCD ranges), fp16 rows -- one gathered row of B per edge, as here;
  * ``voltrix.spmm`` (forward, fp16 rows, the block format with the default tiles: VOLTRIX_TUNE_SPACE=none unless set).
One JSON line per case: milliseconds, the SDDMM's algorithmic bytes nnz (F s_y + 8) + num_rows F s_x + 4 (num_rows + 1), their share of
8 TB/s, and the ratios to the two SpMM times.  Kernel-only times come from a separate ``rocprofv3 --kernel-trace --stats`` run of this
script."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "voltrix-spmm_amd")):
    sys.path.insert(0, p)
os.environ.setdefault("VOLTRIX_CACHE_DIR", os.path.join(REPO, "voltrix-spmm_amd", ".jit_cache"))
os.environ.setdefault("VOLTRIX_TUNE_SPACE", "none")

import torch  # noqa: E402

import synth_graphs  # noqa: E402
import voltrix  # noqa: E402
from voltrix import capi  # noqa: E402

DEFAULT_CASES = ("yeasth_like:128", "amazon0601_like:128", "dd_like:128", "web_berkstan_like:128", "reddit_like:128", "reddit_like:512")
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


def run_case(name, width, steps, warmup, scale):
    indptr, indices, _ = synth_graphs.generate(name, device="cuda", scale=scale)
    n, nnz = indptr.numel() - 1, indices.numel()
    torch.manual_seed(0)
    x = torch.randn(n, width, device="cuda")                      # dC: fp32
    y = torch.randn(n, width, device="cuda").half()               # B: fp16
    out_rows = torch.empty(n, width, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    handle = voltrix.csr_preprocess_device(indptr, indices, n)
    handle[1].hash_tag = f"bench_sddmm/{name}"
    sddmm_ms = _time(lambda: voltrix.sddmm(indptr, indices, x, y), steps, warmup)
    csr_ms = _time(lambda: capi.launch_spmm_csr_rows(indptr, indices, n, y, out_rows, stream, 1), steps, warmup)
    spmm_ms = _time(lambda: voltrix.spmm(*handle, num_nodes=n, num_edges=nnz, feat=y), steps, warmup)
    nbytes = nnz * (width * 2 + 8) + n * width * 4 + 4 * (n + 1)
    return {"graph": name, "F": width, "num_rows": n, "nnz": nnz, "sddmm_ms": round(sddmm_ms, 4), "csr_spmm_ms": round(csr_ms, 4),
            "spmm_ms": round(spmm_ms, 4), "bytes": nbytes, "share_of_8TBps": round(nbytes / (sddmm_ms * 1e-3) / HBM_BYTES_PER_S, 4),
            "ratio_to_csr_spmm": round(sddmm_ms / csr_ms, 3), "ratio_to_spmm": round(sddmm_ms / spmm_ms, 3),
            "ns_per_edge": round(sddmm_ms * 1e6 / nnz, 4)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", nargs="*", default=list(DEFAULT_CASES), help="graph:width pairs")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="synth_graphs scale of every stand-in")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_sddmm.py needs a GPU"
    for case in args.cases:
        name, width = case.split(":")
        print(json.dumps(run_case(name, int(width), args.steps, args.warmup, args.scale)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
