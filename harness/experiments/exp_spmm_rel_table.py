"""The two choices of ``spmm_rel``'s forward kernel, measured: how the ``R x B`` coefficient table reaches the lanes --
plain loads of an address the lanes of a group share, against a copy in LDS that every workgroup fills first -- and the tile of bases
a lane accumulates, 8 against 4.

    python harness/experiments/exp_spmm_rel_table.py build                  # three builds of csrc/capi_spmm_rel.hip (no GPU needed):
                                                                            # as shipped, VOLTRIX_SPMM_REL_COEF_LDS=1, VOLTRIX_SPMM_REL_TILE=4
    python harness/experiments/exp_spmm_rel_table.py run [workload:F ...]   # on the GPU: the builds in turn, same inputs

Per point -- graph, width, dtype, ``(R, B)`` = (46, 8) and (46, 30), types uniform per edge, ``weight`` given -- the forward alone.
Rounds go through the builds in turn; the median of the rounds' means is printed for each with the smallest and largest round, and the
results of the builds are compared bit for bit.
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

BUILDS = {"plain": [], "lds": ["-DVOLTRIX_SPMM_REL_COEF_LDS=1"], "tile4": ["-DVOLTRIX_SPMM_REL_TILE=4"]}
SYMBOL = "voltrix_spmm_rel_csr"


def lib_path(name):
    return os.path.join(BUILD, f"libspmm_rel_{name}.so")


def build():
    os.makedirs(BUILD, exist_ok=True)
    for name, flags in BUILDS.items():
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", *flags,
                               "-I", os.path.join(PKG, "voltrix", "include"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(PKG, "csrc", "capi_spmm_rel.hip"), "-o", lib_path(name)])
        print("built", lib_path(name))


def run(specs):
    import torch

    import synth_graphs
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

    for spec in specs or ["amazon0601_like:32", "amazon0601_like:128", "dd_like:128"]:
        name, dim = spec.split(":")
        dim = int(dim)
        indptr, indices, _ = synth_graphs.generate(name, device="cuda")
        n, nnz = indptr.numel() - 1, indices.numel()
        for relations, bases in ((46, 8), (46, 30)):
            padded = (bases + 3) // 4 * 4
            torch.manual_seed(0)
            etype = torch.randint(0, relations, (nnz,), device="cuda", dtype=torch.int32)
            weight = torch.rand(nnz, device="cuda") + 0.5
            coef = torch.nn.functional.pad(torch.randn(relations, bases, device="cuda"), (0, padded - bases)).contiguous()
            for dtype in (torch.float16, torch.float32):
                feat = torch.randn(n, dim, device="cuda").to(dtype)
                out = torch.empty(n, bases, dim, device="cuda")

                def forward(lib):
                    assert getattr(lib, SYMBOL)(indptr.data_ptr(), indices.data_ptr(), etype.data_ptr(), weight.data_ptr(), n, nnz, dim,
                                                relations, bases, feat.data_ptr(), codes[dtype], coef.data_ptr(), out.data_ptr(),
                                                stream) == 0

                results = []
                for lib in libs.values():                 # the builds compute the same bits
                    out.fill_(float("nan"))
                    forward(lib)
                    results.append(out.clone())
                assert all(torch.equal(r.view(torch.int32), results[0].view(torch.int32)) for r in results)
                del results
                rounds = {k: [] for k in libs}
                for _ in range(5):
                    for k, lib in libs.items():
                        rounds[k].append(timeit(lambda: forward(lib)))
                line = {"graph": name, "F": dim, "dtype": str(dtype).split(".")[1], "R": relations, "B": bases, "num_rows": n, "nnz": nnz}
                for k, v in rounds.items():
                    line[f"fwd_{k}_ms"] = round(sorted(v)[2], 4)
                    line[f"fwd_{k}_spread_ms"] = [round(min(v), 4), round(max(v), 4)]
                print(json.dumps(line), flush=True)
                del feat, out
                torch.cuda.empty_cache()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        build()
    elif len(sys.argv) > 1 and sys.argv[1] == "run":
        run(sys.argv[2:])
    else:
        raise SystemExit(__doc__)
