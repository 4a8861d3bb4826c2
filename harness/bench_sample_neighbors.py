#!/usr/bin/env python3
"""Time neighbour sampling (``voltrix.sample_neighbors``) and mini-batch blocks (``voltrix.sample_blocks``) on synth_graphs stand-ins,
against the torch composite a user would write without them.

Per graph, in one process on one GPU:
  * ``sample_neighbors`` over ALL rows at fan-out 10 and 25, with and without replacement -- the whole call (torch plumbing, the one
    read-back, the HIP launch), host clock around calls that end in their own synchronisation, and the HIP launch alone between device
    events on pre-computed segments;
  * baseline, the torch composite on the same seeds: expand the seed rows into (row, entry) pairs, draw a random key per entry, sort
    by (row, key), keep the first k of every row.  It materialises O(sum of degrees) keys; the kernel reads k entries per row;
  * a 1,024-seed two-layer ``sample_blocks`` with fan-outs (25, 10): the whole call per batch, and its phases (sampling, relabelling,
    building the pattern's transpose) bracketed by synchronisations; next to them, measured alone at this graph's size, what a batch
    pays whatever its size: the dense table's clear, the ``cumsum`` over it, and a read-back's round trip (two per layer).
One JSON line per graph and measurement: the median of ``--rounds`` windows of ``--steps`` calls in milliseconds, and the windows' min
and max (the spread).  Sampled results are checked against the rule's invariants before anything is timed."""
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
from voltrix.autograd import CsrPattern  # noqa: E402

DEFAULT_CASES = ("amazon0601_like", "reddit_like", "products_like")
SEED = 20261019


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


def composite_sample(indptr, indices, seeds, k):
    """The torch sampler this package replaces: ``(s_indptr, s_indices, s_entries)`` with at most ``k`` entries per seed row, uniform
    without replacement, rows in CSR order.  Not reproducible across runs or devices beyond torch's generator."""
    rows_of = seeds.long()
    begin = indptr[rows_of].long()
    deg = indptr[rows_of + 1].long() - begin
    first = torch.cumsum(deg, 0) - deg
    owner = torch.repeat_interleave(torch.arange(seeds.numel(), device=seeds.device), deg)          # a read-back of its own
    entry = begin[owner] + (torch.arange(owner.numel(), device=seeds.device) - first[owner])
    key = torch.rand(owner.numel(), device=seeds.device)
    by_key = torch.argsort(key)
    order = by_key[torch.argsort(owner[by_key], stable=True)]                                         # sorted by (row, key)
    keep = (torch.arange(owner.numel(), device=seeds.device) - first[owner]) < k                     # owner is sorted: rank in its row
    taken = torch.sort(entry[order][keep]).values                                                     # rows ascending: CSR order
    count = deg.clamp(max=k)
    s_indptr = torch.zeros(seeds.numel() + 1, dtype=torch.int32, device=seeds.device)
    s_indptr[1:] = torch.cumsum(count, 0)
    return s_indptr, indices[taken], taken.int()


def _check_sample(indptr, indices, seeds, k, replace, result):
    s_indptr, s_indices, s_entries = result
    deg = (indptr[seeds.long() + 1] - indptr[seeds.long()]).long()
    want = torch.where(deg > 0, torch.full_like(deg, k), torch.zeros_like(deg)) if replace else deg.clamp(max=k)
    assert torch.equal((s_indptr[1:] - s_indptr[:-1]).long(), want), "segment sizes"
    owner = torch.repeat_interleave(seeds.long(), want)
    entries = s_entries.long()
    assert bool(((indptr[owner] <= entries) & (entries < indptr[owner + 1])).all()), "an entry outside its row"
    assert torch.equal(indices[entries], s_indices), "columns"
    if not replace:
        assert bool((entries[1:] > entries[:-1]).all()), "CSR order (the seeds here are all rows, ascending)"


def run_graph(name, scale, steps, warmup, rounds, torch_steps, batch):
    indptr, indices, _ = synth_graphs.generate(name, device="cuda", scale=scale)
    n, nnz = indptr.numel() - 1, indices.numel()
    deg = indptr[1:] - indptr[:-1]
    base = {"graph": name, "scale": scale, "num_rows": n, "entries": nnz, "max_deg": int(deg.max()), "steps": steps, "rounds": rounds}
    all_rows = torch.arange(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for k in (10, 25):
        for replace in (False, True):
            result = voltrix.sample_neighbors(indptr, indices, all_rows, k, SEED, 0, replace)
            _check_sample(indptr, indices, all_rows, k, replace, result)
            s_indptr, s_indices, s_entries = result
            total = s_indices.numel()
            call = _windows(lambda: voltrix.sample_neighbors(indptr, indices, all_rows, k, SEED, 0, replace), steps, warmup, rounds)
            launch = _windows(lambda: capi.launch_sample_neighbors(indptr, indices, n, all_rows, s_indptr, total, k, replace, SEED, 0,
                                                                   s_indices, s_entries, stream), steps, warmup, rounds, events=True)
            line = dict(base, measurement="sample_all_rows", fanout=k, replace=replace, num_sampled=total,
                        rows_above_fanout=int((deg > k).sum()))
            line.update({"call_" + key: v for key, v in _stats(call).items()})
            line.update({"kernel_" + key: v for key, v in _stats(launch).items()})
            line["kernel_ns_per_row"] = round(line["kernel_ms"] * 1e6 / n, 3)
            if not replace:
                try:
                    got = composite_sample(indptr, indices, all_rows, k)
                    assert torch.equal(got[0], s_indptr), "the composite's segment sizes"
                    del got
                    torch_ms = _windows(lambda: composite_sample(indptr, indices, all_rows, k), torch_steps, 1, rounds)
                    line.update({"torch_" + key: v for key, v in _stats(torch_ms).items()})
                    line["speedup_call_over_torch"] = round(line["torch_ms"] / line["call_ms"], 2)
                except torch.cuda.OutOfMemoryError:          # the composite's O(entries) temporaries do not fit: recorded, not hidden
                    line["torch_ms"], line["torch_out_of_memory"] = None, True
                torch.cuda.empty_cache()
            print(json.dumps(line), flush=True)
            del result, s_indptr, s_indices, s_entries
    # ---- a two-layer mini-batch
    fanouts = (25, 10)
    seeds = torch.randperm(n, device="cuda", generator=torch.Generator("cuda").manual_seed(1))[:batch].int()
    blocks = voltrix.sample_blocks(indptr, indices, seeds, fanouts, SEED, 0)
    assert torch.equal(blocks[-1].dst_ids, seeds) and torch.equal(blocks[0].dst_ids, blocks[1].src_ids)
    line = dict(base, measurement="sample_blocks", batch=batch, fanouts=list(fanouts),
                num_src=[b.num_src for b in blocks], num_edges=[b.pattern.num_edges for b in blocks])
    line.update(_stats(_windows(lambda: voltrix.sample_blocks(indptr, indices, seeds, fanouts, SEED, 0), steps, warmup, rounds)))

    def phases():
        times = {"sample": 0.0, "relabel": 0.0, "pattern": 0.0}
        dst = seeds
        for layer, fanout in enumerate(reversed(fanouts)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s_indptr, s_indices, _ = voltrix.sample_neighbors(indptr, indices, dst, fanout, SEED, layer)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            src, local = voltrix.compact_block(dst, s_indices, n)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            CsrPattern(s_indptr, local, dst.numel(), src.numel())
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            times["sample"] += (t1 - t0) * 1e3
            times["relabel"] += (t2 - t1) * 1e3
            times["pattern"] += (t3 - t2) * 1e3
            dst = src
        return times

    for _ in range(warmup):
        phases()
    runs = [phases() for _ in range(steps)]
    for key in ("sample", "relabel", "pattern"):
        line[f"phase_{key}_ms"] = round(sorted(r[key] for r in runs)[len(runs) // 2], 4)
    # what a batch pays whatever its size, alone, at this graph's size: per layer one clear, one cumsum, two read-backs
    table = torch.zeros(n, dtype=torch.int32, device="cuda")
    table[::7] = 1
    pair = torch.zeros(2, dtype=torch.int64, device="cuda")
    line["table_clear_ms"] = _stats(_windows(lambda: torch.zeros(n, dtype=torch.int32, device="cuda"), steps, warmup, rounds, True))["ms"]
    line["cumsum_ms"] = _stats(_windows(lambda: torch.cumsum(table > 0, 0, dtype=torch.int32), steps, warmup, rounds, True))["ms"]
    line["read_back_ms"] = _stats(_windows(lambda: pair.tolist(), steps, warmup, rounds))["ms"]
    fixed = len(fanouts) * (line["table_clear_ms"] + line["cumsum_ms"] + 2 * line["read_back_ms"])
    line["fixed_ms_per_batch"] = round(fixed, 4)
    line["fixed_share_of_batch"] = round(fixed / line["ms"], 3)
    print(json.dumps(line), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", nargs="*", default=list(DEFAULT_CASES), help="synth_graphs stand-in names")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per measurement (their min / max is the spread)")
    ap.add_argument("--torch-steps", type=int, default=2, help="timed calls of the torch composite per window")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--scale", type=float, default=1.0, help="synth_graphs scale of every stand-in")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_sample_neighbors.py needs a GPU"
    for name in args.cases:
        run_graph(name, args.scale, args.steps, args.warmup, args.rounds, args.torch_steps, args.batch)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
