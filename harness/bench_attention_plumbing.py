"""Host time per call of the attention operators: the Python and launch path around the kernels.

On a 64-row graph the kernels take a few microseconds, so 1000 back-to-back calls followed by one synchronize measure what the host
spends per call.  Every public function and the forward + backward of every autograd operator is timed five times; the median and the
spread (max - min) of the five are reported in microseconds per call.

    python harness/bench_attention_plumbing.py --out new.json                      # this tree
    python harness/bench_attention_plumbing.py --pkg <other tree>/voltrix-spmm_amd --out parent.json
    python harness/bench_attention_plumbing.py --compare parent.json [parent2.json] new.json

``--compare`` prints both tables and, per function, whether the last file's median is within the baseline's median plus the baseline's
own spread (with two baseline files: the first one's median, the larger spread).
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS, REPEATS = 1000, 5


def _cases(voltrix, torch):
    from voltrix.autograd import SDDMM, AttnAggregate, GATScore, GATv2Score, SpMMHeads

    n, heads, dim = 64, 4, 16
    g = torch.Generator().manual_seed(0)
    deg = torch.randint(0, 9, (n,), generator=g)
    indptr = torch.zeros(n + 1, dtype=torch.int32)
    indptr[1:] = torch.cumsum(deg, 0)
    nnz = int(indptr[-1])
    indices = torch.randint(0, n, (nnz,), generator=g).to(torch.int32)
    indptr, indices = indptr.cuda(), indices.cuda()

    def rand(*shape):
        return torch.randn(*shape, generator=g).cuda()

    x2, y2, x3, y3 = rand(n, dim), rand(n, dim), rand(n, heads, dim), rand(n, heads, dim)
    s1, s2 = rand(nnz), rand(nnz, heads)
    el, er, a = rand(n, heads), rand(n, heads), rand(heads, dim)
    cases = {
        "sddmm 2-D": lambda: voltrix.sddmm(indptr, indices, x2, y2),
        "sddmm 3-D": lambda: voltrix.sddmm(indptr, indices, x3, y3),
        "edge_softmax 1-D": lambda: voltrix.edge_softmax(indptr, s1, 0.5),
        "edge_softmax 2-D": lambda: voltrix.edge_softmax(indptr, s2, 0.5),
        "spmm_heads": lambda: voltrix.spmm_heads(indptr, indices, s2, x3, n),
        "gat_score": lambda: voltrix.gat_score(indptr, indices, el, er, 0.2),
        "gatv2_score": lambda: voltrix.gatv2_score(indptr, indices, x3, y3, a, 0.2),
        "attn_aggregate": lambda: voltrix.attn_aggregate(indptr, indices, s2, x3, n, 0.5),
    }

    def train(op, *tensors):
        leaves = [t.clone().requires_grad_() for t in tensors]

        def step():
            for t in leaves:
                t.grad = None
            op(*leaves).sum().backward()

        return step

    cases["SDDMM fwd+bwd"] = train(SDDMM(indptr, indices, n), x3, y3)
    cases["SpMMHeads fwd+bwd"] = train(SpMMHeads(indptr, indices, n), x3, s2)
    cases["GATScore fwd+bwd"] = train(GATScore(indptr, indices, n), el, er)
    cases["GATv2Score fwd+bwd"] = train(GATv2Score(indptr, indices, n), x3, y3, a)
    cases["AttnAggregate fwd+bwd"] = train(AttnAggregate(indptr, indices, n), x3, s2)
    return cases


def measure(pkg: str) -> dict:
    sys.path.insert(0, pkg)
    os.environ.setdefault("VOLTRIX_CACHE_DIR", os.path.join(pkg, ".jit_cache"))
    import torch
    import voltrix

    assert os.path.dirname(os.path.dirname(os.path.abspath(voltrix.__file__))) == os.path.abspath(pkg), voltrix.__file__
    result = {}
    for name, fn in _cases(voltrix, torch).items():
        for _ in range(50):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e6 / CALLS)
        result[name] = {"median_us": round(statistics.median(times), 2), "min_us": round(min(times), 2), "max_us": round(max(times), 2)}
    return result


def compare(paths) -> bool:
    runs = []
    for p in paths:
        with open(p) as f:
            runs.append(json.load(f))
    *baselines, new = runs
    ok = True
    print("| function | " + " | ".join(f"{os.path.basename(p)} median (min .. max) us" for p in paths) + " | allowed | verdict |")
    print("|---|" + "---|" * (len(paths) + 2))
    for name in new:
        spread = max(b[name]["max_us"] - b[name]["min_us"] for b in baselines)
        allowed = baselines[0][name]["median_us"] + spread
        good = new[name]["median_us"] <= allowed
        ok &= good
        cells = [f"{r[name]['median_us']:.2f} ({r[name]['min_us']:.2f} .. {r[name]['max_us']:.2f})" for r in runs]
        print(f"| {name} | " + " | ".join(cells) + f" | {allowed:.2f} | {'pass' if good else 'FAIL'} |")
    return ok


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pkg", default=os.path.join(REPO, "voltrix-spmm_amd"), help="package root to measure (holds voltrix/ and lib/)")
    ap.add_argument("--out", help="write the measurement as JSON here")
    ap.add_argument("--compare", nargs="+", metavar="JSON", help="baseline file(s), then the file to judge")
    args = ap.parse_args()
    if args.compare:
        sys.exit(0 if compare(args.compare) else 1)
    res = measure(args.pkg)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
