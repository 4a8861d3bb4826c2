"""Plain loads against non-temporal loads (``__builtin_nontemporal_load``) of ``efeat`` in the spmm_edge kernels: ``efeat`` [nnz, F] is
streamed exactly once while the gathered rows of ``feat`` are what should stay in L2 (``exp_gather_nt.py`` is the
precedent, for the block-format kernels' row gathers).

    python harness/experiments/exp_spmm_edge_nt.py build                    # two builds of csrc/capi_spmm_edge.hip (no GPU needed):
                                                                            # VOLTRIX_SPMM_EDGE_NT=0 / 1 -> build/libspmm_edge_nt{0,1}.so
    python harness/experiments/exp_spmm_edge_nt.py run [workload:F ...]     # on the GPU: both builds, alternating, same inputs

Per point: forward mul and add_relu, ``grad_efeat`` of add_relu (streams efeat, gathers feat) and the backward for feat of mul (the
kernel on the transposed CSR: efeat read through t_order, i.e. gathered, once).  Rounds alternate the two builds; the median of the
rounds' means is printed for each, and the results of the two builds are compared bit for bit.
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


def lib_path(nt):
    return os.path.join(BUILD, f"libspmm_edge_nt{nt}.so")


def build():
    os.makedirs(BUILD, exist_ok=True)
    for nt in (0, 1):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                               f"-DVOLTRIX_SPMM_EDGE_NT={nt}", "-I", os.path.join(PKG, "voltrix", "include"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(PKG, "csrc", "capi_spmm_edge.hip"), "-o", lib_path(nt)])
        print("built", lib_path(nt))


def run(specs):
    import torch

    import synth_graphs
    from voltrix import capi
    from voltrix.autograd import CsrPattern

    libs = []
    for nt in (0, 1):
        lib = ctypes.CDLL(lib_path(nt))
        for name in ("voltrix_spmm_edge_csr", "voltrix_spmm_edge_grad_efeat_csr"):
            getattr(lib, name).restype, getattr(lib, name).argtypes = capi.SIGNATURES[name]
        libs.append(lib)
    stream = torch.cuda.current_stream().cuda_stream
    codes = {torch.float32: 0, torch.float16: 1}

    def timeit(fn, iters=20, warm=3):
        for _ in range(warm):
            fn()
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        t.record()
        t.synchronize()
        return s.elapsed_time(t) / iters

    for spec in specs or ["yeast_like:128", "dd_like:128", "amazon0601_like:128", "amazon0601_like:32"]:
        name, dim = spec.split(":")
        dim = int(dim)
        indptr, indices, _ = synth_graphs.generate(name, device="cuda")
        n, nnz = indptr.numel() - 1, indices.numel()
        p = CsrPattern(indptr, indices, n)
        for dtype in (torch.float16, torch.float32):
            torch.manual_seed(0)
            feat = torch.randn(n, dim, device="cuda").to(dtype)
            efeat = torch.randn(nnz, dim, device="cuda").to(dtype)
            grad = torch.randn(n, dim, device="cuda")
            out, big = torch.empty(n, dim, device="cuda"), torch.empty(nnz, dim, device="cuda")
            d = codes[dtype]

            def forward(lib, op):
                assert lib.voltrix_spmm_edge_csr(indptr.data_ptr(), indices.data_ptr(), None, n, nnz, dim, feat.data_ptr(), d,
                                                 efeat.data_ptr(), d, None, op, out.data_ptr(), stream) == 0

            def backward_feat(lib):
                assert lib.voltrix_spmm_edge_csr(p.t_indptr.data_ptr(), p.t_indices.data_ptr(), p.t_order.data_ptr(), n, nnz, dim,
                                                 grad.data_ptr(), 0, efeat.data_ptr(), d, None, 0, out.data_ptr(), stream) == 0

            def backward_efeat(lib):
                assert lib.voltrix_spmm_edge_grad_efeat_csr(indptr.data_ptr(), indices.data_ptr(), n, nnz, dim, grad.data_ptr(),
                                                            feat.data_ptr(), efeat.data_ptr(), d, 2, big.data_ptr(), stream) == 0

            kernels = {"fwd_mul": lambda lib: forward(lib, 0), "fwd_add_relu": lambda lib: forward(lib, 2),
                       "bwd_feat_mul": backward_feat, "bwd_efeat_add_relu": backward_efeat}
            line = {"graph": name, "F": dim, "dtype": str(dtype).split(".")[1], "num_rows": n, "nnz": nnz}
            for label, fn in kernels.items():
                results = []
                for lib in libs:                      # the two builds compute the same bits
                    fn(lib)
                    results.append((big if label == "bwd_efeat_add_relu" else out).clone())
                assert torch.equal(results[0].view(torch.int32), results[1].view(torch.int32)), label
                rounds = [[], []]
                for _ in range(5):                    # alternate the builds
                    for nt in (0, 1):
                        rounds[nt].append(timeit(lambda: fn(libs[nt])))
                for nt in (0, 1):
                    line[f"{label}_{'nt' if nt else 'plain'}_ms"] = round(sorted(rounds[nt])[2], 4)
                    line[f"{label}_{'nt' if nt else 'plain'}_spread_ms"] = [round(min(rounds[nt]), 4), round(max(rounds[nt]), 4)]
            print(json.dumps(line), flush=True)
            del feat, efeat, grad, out, big
            torch.cuda.empty_cache()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        build()
    elif len(sys.argv) > 1 and sys.argv[1] == "run":
        run(sys.argv[2:])
    else:
        raise SystemExit(__doc__)
