"""How many entries ``spmm_csr_rows_fp8_kernel`` keeps in flight per lane, measured: 4, the 16-bit row-gather kernel's
batch, against 8 -- an fp8 row piece is 16 bytes for 16 features, so a batch of 4 requests half the bytes per feature that the 16-bit
kernel's does.

    python harness/experiments/exp_spmm_fp8_unroll.py build                  # two builds of csrc/capi_spmm_fp8.hip (no GPU needed):
                                                                            # as shipped (4) and VOLTRIX_SPMM_FP8_UNROLL=8
    python harness/experiments/exp_spmm_fp8_unroll.py run [workload:F ...]   # on the GPU: the builds in turn, same inputs

Per point -- graph, width, fp32 and fp16 output, without values -- the aggregation alone.  Rounds go through the builds in turn; the
median of the rounds' means is printed for each with the smallest and largest round, and the results of the builds are compared bit for
bit (both sum in CSR order).
"""
import ctypes
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(ROOT, "voltrix-spmm_amd")
BUILD = os.path.join(HERE, "build")
sys.path.insert(0, PKG)
sys.path.insert(0, ROOT)

BUILDS = {"unroll4": [], "unroll8": ["-DVOLTRIX_SPMM_FP8_UNROLL=8"]}
SYMBOL = "voltrix_spmm_fp8_csr"


def lib_path(name):
    return os.path.join(BUILD, f"libspmm_fp8_{name}.so")


def build():
    os.makedirs(BUILD, exist_ok=True)
    for name, flags in BUILDS.items():
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", *flags,
                               "-I", os.path.join(PKG, "voltrix", "include"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(PKG, "csrc", "capi_spmm_fp8.hip"), "-o", lib_path(name)])
        print("built", lib_path(name))


def run(specs):
    import torch

    import synth_graphs
    import voltrix
    from voltrix import capi

    libs = {}
    for name in BUILDS:
        lib = ctypes.CDLL(lib_path(name))
        getattr(lib, SYMBOL).restype, getattr(lib, SYMBOL).argtypes = capi.SIGNATURES[SYMBOL]
        libs[name] = lib
    stream = torch.cuda.current_stream().cuda_stream
    codes = {torch.float32: 0, torch.float16: 1}

    def timeit(fn, iters=10, warm=3):
        for _ in range(warm):
            fn()
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        t.record()
        t.synchronize()
        return s.elapsed_time(t) / iters

    for spec in specs or ["amazon0601_like:128", "amazon0601_like:512", "dd_like:128", "dd_like:512", "reddit_like@0.25:128"]:
        name, dim = spec.split(":")
        name, _, scale = name.partition("@")
        dim = int(dim)
        indptr, indices, _ = synth_graphs.generate(name, device="cuda", scale=float(scale or 1.0))
        n, nnz = indptr.numel() - 1, indices.numel()
        torch.manual_seed(0)
        rows = voltrix.quantize_fp8(torch.randn(n, dim, device="cuda").half(), "column")
        for out_dtype in (torch.float32, torch.float16):
            out = torch.empty(n, rows.data.shape[1], device="cuda", dtype=out_dtype)

            def forward(lib):
                assert getattr(lib, SYMBOL)(indptr.data_ptr(), indices.data_ptr(), None, n, rows.data.shape[1], rows.data.data_ptr(),
                                            rows.scale.data_ptr(), out.data_ptr(), codes[out_dtype], 1, nnz, stream) == 0

            results = []
            for lib in libs.values():                 # the builds compute the same bits
                out.fill_(float("nan"))
                forward(lib)
                results.append(out.clone())
            assert all(torch.equal(r.view(torch.int16), results[0].view(torch.int16)) for r in results)
            del results
            rounds = {k: [] for k in libs}
            for _ in range(5):
                for k, lib in libs.items():
                    rounds[k].append(timeit(lambda: forward(lib)))
            line = {"graph": name, "scale": float(scale or 1.0), "F": dim, "out": str(out_dtype).split(".")[1], "num_rows": n, "nnz": nnz}
            for k, v in rounds.items():
                line[f"{k}_ms"] = round(sorted(v)[2], 4)
                line[f"{k}_spread_ms"] = [round(min(v), 4), round(max(v), 4)]
            line["unroll8_over_unroll4"] = round(line["unroll8_ms"] / line["unroll4_ms"], 3)
            print(json.dumps(line), flush=True)
            del out
        del rows
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        build()
    elif len(sys.argv) > 1 and sys.argv[1] == "run":
        run(sys.argv[2:])
    else:
        raise SystemExit(__doc__)
