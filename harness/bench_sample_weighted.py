#!/usr/bin/env python3
"""Time weighted neighbour sampling (``voltrix.sample_neighbors(prob=)``) on synth_graphs stand-ins, next to the uniform launch and the
torch composite a user would write without it.

Per graph, in one process on one GPU, with ``prob = 1 / in_degree(column)`` (importance sampling by inverse degree):
  * the table build, ``voltrix.sampling_weights`` -- once per graph, host clock (it ends in its own read-back);
  * ``sample_neighbors(prob=)`` over ALL rows at fan-out 10 and 25, with and without replacement -- the whole call (torch plumbing, the
    one read-back, the HIP launch), host clock, and the HIP launch alone between device events on pre-computed segments;
  * the uniform launch on the same rows and fan-out, in the same process: what the weights cost on top;
  * baseline, the torch composite: per-entry exponential keys ``-log(u) / w``, sorted by (row, key), the first k of every row kept.  It
    materialises O(sum of degrees) keys and is not reproducible bit for bit (a transcendental function per entry).
One JSON line per graph and measurement: the median of ``--rounds`` windows of ``--steps`` calls in milliseconds, and the windows' min
and max (the spread); ``--out`` appends the lines to a file as well.  Results are checked against the rule's invariants before anything
is timed."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "voltrix-spmm_amd")):
    sys.path.insert(0, p)
os.environ.setdefault("VOLTRIX_CACHE_DIR", os.path.join(REPO, "voltrix-spmm_amd", ".jit_cache"))

import torch  # noqa: E402

import synth_graphs  # noqa: E402
import voltrix  # noqa: E402
from voltrix import capi  # noqa: E402

DEFAULT_CASES = ("amazon0601_like", "reddit_like", "products_like")
SEED = 20261020


def _windows(fn, steps, warmup, rounds, events=False):
    """Milliseconds per call in each of ``rounds`` windows of ``steps`` calls: device events, or the host clock between two
    synchronisations (for calls that synchronise themselves)."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        if events:
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(steps):
                fn()
            end.record()
            end.synchronize()
            out.append(start.elapsed_time(end) / steps)
        else:
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3 / steps)
    return out


def _stats(ms):
    ms = sorted(ms)
    return {"ms": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


def composite_sample(indptr, indices, prob, seeds, k):
    """The torch sampler a user would write: ``(s_indptr, s_indices, s_entries)`` with at most ``k`` entries per seed row, without
    replacement, by exponential keys (Efraimidis-Spirakis): the k smallest ``-log(u) / w`` of every row."""
    rows_of = seeds.long()
    begin = indptr[rows_of].long()
    deg = indptr[rows_of + 1].long() - begin
    first = torch.cumsum(deg, 0) - deg
    owner = torch.repeat_interleave(torch.arange(seeds.numel(), device=seeds.device), deg)          # a read-back of its own
    entry = begin[owner] + (torch.arange(owner.numel(), device=seeds.device) - first[owner])
    w = prob[entry].double()
    key = torch.where(w > 0, -torch.log(torch.rand(owner.numel(), device=seeds.device, dtype=torch.float64)) / w,
                      torch.full_like(w, float("inf")))
    by_key = torch.argsort(key)
    order = by_key[torch.argsort(owner[by_key], stable=True)]                                         # sorted by (row, key)
    positive = torch.zeros(seeds.numel(), dtype=torch.int64, device=seeds.device).index_add_(0, owner, (w > 0).long())
    rank = torch.arange(owner.numel(), device=seeds.device) - first[owner]                            # owner is sorted: rank in its row
    keep = rank < positive.clamp(max=k)[owner]
    taken = torch.sort(entry[order][keep]).values                                                     # rows ascending: CSR order
    s_indptr = torch.zeros(seeds.numel() + 1, dtype=torch.int32, device=seeds.device)
    s_indptr[1:] = torch.cumsum(positive.clamp(max=k), 0)
    return s_indptr, indices[taken], taken.int()


def _check_sample(indptr, indices, prob, table, seeds, k, replace, result):
    s_indptr, s_indices, s_entries = result
    p = table.positive[seeds.long()].long()
    want = torch.where(p > 0, torch.full_like(p, k), torch.zeros_like(p)) if replace else p.clamp(max=k)
    assert torch.equal((s_indptr[1:] - s_indptr[:-1]).long(), want), "segment sizes"
    owner = torch.repeat_interleave(seeds.long(), want)
    entries = s_entries.long()
    assert bool(((indptr[owner] <= entries) & (entries < indptr[owner + 1])).all()), "an entry outside its row"
    assert torch.equal(indices[entries], s_indices), "columns"
    assert bool((prob[entries] > 0).all()), "an entry of weight zero"
    if not replace:
        assert bool((entries[1:] > entries[:-1]).all()), "CSR order (the seeds here are all rows, ascending)"


def run_graph(name, scale, steps, warmup, rounds, torch_steps, emit):
    indptr, indices, _ = synth_graphs.generate(name, device="cuda", scale=scale)
    n, nnz = indptr.numel() - 1, indices.numel()
    deg = indptr[1:] - indptr[:-1]
    in_degree = torch.bincount(indices.long(), minlength=n).clamp(min=1)
    prob = (1.0 / in_degree.float())[indices.long()]
    base = {"graph": name, "scale": scale, "num_rows": n, "entries": nnz, "mean_deg": round(nnz / max(1, n), 1), "max_deg": int(deg.max()),
            "steps": steps, "rounds": rounds}
    table = voltrix.sampling_weights(indptr, prob)
    build = _windows(lambda: voltrix.sampling_weights(indptr, prob), max(1, steps // 4), 1, rounds)
    line = dict(base, measurement="sampling_weights", table_bytes=8 * nnz + 4 * n)
    line.update(_stats(build))
    emit(line)
    all_rows = torch.arange(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for k in (10, 25):
        for replace in (False, True):
            result = voltrix.sample_neighbors(indptr, indices, all_rows, k, SEED, 0, replace, prob=table)
            _check_sample(indptr, indices, prob, table, all_rows, k, replace, result)
            s_indptr, s_indices, s_entries = result
            total = s_indices.numel()
            call = _windows(lambda: voltrix.sample_neighbors(indptr, indices, all_rows, k, SEED, 0, replace, prob=table), steps, warmup,
                            rounds)
            launch = _windows(lambda: capi.sample_neighbors_weighted(indptr, indices, table.cum, n, all_rows, s_indptr, total, k, replace,
                                                                     SEED, 0, s_indices, s_entries, stream), steps, warmup, rounds, events=True)
            u_indptr, u_indices, u_entries = voltrix.sample_neighbors(indptr, indices, all_rows, k, SEED, 0, replace)
            uniform = _windows(lambda: capi.launch_sample_neighbors(indptr, indices, n, all_rows, u_indptr, u_indices.numel(), k, replace,
                                                                    SEED, 0, u_indices, u_entries, stream), steps, warmup, rounds, events=True)
            line = dict(base, measurement="sample_all_rows_weighted", fanout=k, replace=replace, num_sampled=total,
                        rows_drawn=int((table.positive > k).sum()))
            line.update({"call_" + key: v for key, v in _stats(call).items()})
            line.update({"kernel_" + key: v for key, v in _stats(launch).items()})
            line.update({"uniform_kernel_" + key: v for key, v in _stats(uniform).items()})
            line["kernel_ns_per_row"] = round(line["kernel_ms"] * 1e6 / n, 3)
            line["uniform_kernel_ns_per_row"] = round(line["uniform_kernel_ms"] * 1e6 / n, 3)
            line["kernel_over_uniform"] = round(line["kernel_ms"] / line["uniform_kernel_ms"], 2)
            del u_indptr, u_indices, u_entries
            if not replace:
                try:
                    got = composite_sample(indptr, indices, prob, all_rows, k)
                    assert torch.equal(got[0], s_indptr), "the composite's segment sizes"
                    del got
                    torch_ms = _windows(lambda: composite_sample(indptr, indices, prob, all_rows, k), torch_steps, 1, rounds)
                    line.update({"torch_" + key: v for key, v in _stats(torch_ms).items()})
                    line["speedup_call_over_torch"] = round(line["torch_ms"] / line["call_ms"], 2)
                except torch.cuda.OutOfMemoryError:          # the composite's O(entries) temporaries do not fit: recorded, not hidden
                    line["torch_ms"], line["torch_out_of_memory"] = None, True
                torch.cuda.empty_cache()
            emit(line)
            del result, s_indptr, s_indices, s_entries


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", nargs="*", default=list(DEFAULT_CASES), help="synth_graphs stand-in names")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per measurement (their min / max is the spread)")
    ap.add_argument("--torch-steps", type=int, default=2, help="timed calls of the torch composite per window")
    ap.add_argument("--scale", type=float, default=1.0, help="synth_graphs scale of every stand-in")
    ap.add_argument("--out", default=None, help="a file the JSON lines are appended to as well")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_sample_weighted.py needs a GPU"

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")

    for name in args.cases:
        run_graph(name, args.scale, args.steps, args.warmup, args.rounds, args.torch_steps, emit)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
