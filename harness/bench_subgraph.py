#!/usr/bin/env python3
"""Time induced subgraphs (``voltrix.subgraph_csr``), random walks (``voltrix.random_walk``) and the random-walk subgraph sampler
(``voltrix.sample_subgraph_rw``) on synth_graphs stand-ins, against the torch composite a user would write without them.

Per graph, in one process on one GPU:
  * ``subgraph_csr(rows=cols=nodes)`` over random node sets of 1 %, 10 % and 50 % of the graph (ascending ids) -- the whole call
    (the table's clear and marking, the count launch, ``cumsum``, the one read-back, the fill launch) on the host clock around calls
    that end in their own synchronisation, with ``group_for``'s width and with EVERY lane-group width, and the count + fill launches
    alone between device events, for every width;
  * baseline, the torch composite on the same node sets: expand the selected rows into (row, entry) pairs, look every column up in a
    dense int64 table, ``nonzero`` of the mask, ``bincount`` for the row pointer.  Several passes over temporaries as long as the
    selected rows' entries, with int64 ids;
  * ``random_walk`` at W = 1,000 / 100,000 walkers and length 4 / 16: the whole call, the launch alone with walker-major stores (what
    the call uses) and with step-major stores plus the transposing copies that give the same ``[W, length + 1]`` result;
  * one ``sample_subgraph_rw`` call (1,024 roots, 4 steps) and its phases bracketed by synchronisations: the walk, the distinct
    visited nodes (``compact_block``), ``subgraph_csr``, the pattern's transpose.
One JSON line per graph and measurement: the median of ``--rounds`` windows of ``--steps`` calls in milliseconds, and the windows' min
and max (the spread).  Results are checked against the composite before anything is timed."""
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
from voltrix.subgraph import GROUPS, group_for  # noqa: E402

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


def composite_subgraph(indptr, indices, rows, cols, num_cols):
    """The torch composite this package replaces: ``(s_indptr, s_local, s_entries)`` of ``voltrix.subgraph_csr``."""
    dev = rows.device
    local_of = torch.full((num_cols,), -1, dtype=torch.int64, device=dev)
    local_of[cols.long()] = torch.arange(cols.numel(), device=dev)
    wide = rows.long()
    begin = indptr[wide].long()
    deg = indptr[wide + 1].long() - begin
    first = torch.cumsum(deg, 0) - deg
    owner = torch.repeat_interleave(torch.arange(rows.numel(), device=dev), deg)                  # a read-back of its own
    entry = begin[owner] + (torch.arange(owner.numel(), device=dev) - first[owner])
    local = local_of[indices[entry].long()]
    keep = torch.nonzero(local >= 0).view(-1)                                                      # and another
    s_indptr = torch.zeros(rows.numel() + 1, dtype=torch.int32, device=dev)
    s_indptr[1:] = torch.cumsum(torch.bincount(owner[keep], minlength=rows.numel()), 0)
    return s_indptr, local[keep].int(), entry[keep].int()


def bench_subgraph(base, indptr, indices, steps, warmup, rounds, torch_steps):
    n, nnz = indptr.numel() - 1, indices.numel()
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator("cuda").manual_seed(1)
    for percent in (1, 10, 50):
        nodes = torch.sort(torch.randperm(n, device="cuda", generator=gen)[:max(1, n * percent // 100)]).values.int()
        result = voltrix.subgraph_csr(indptr, indices, nodes)
        s_indptr, s_local, s_entries = result
        line = dict(base, measurement="subgraph_csr", percent=percent, num_nodes=nodes.numel(), num_kept=s_local.numel(),
                    default_group=group_for(nnz, n))
        line.update({"call_" + key: v for key, v in _stats(_windows(lambda: voltrix.subgraph_csr(indptr, indices, nodes), steps, warmup,
                                                                    rounds)).items()})
        for group in GROUPS:
            stats = _stats(_windows(lambda: voltrix.subgraph_csr(indptr, indices, nodes, group=group), steps, warmup, rounds))
            line.update({f"call_g{group}_" + key: v for key, v in stats.items()})
        table = torch.zeros(n, dtype=torch.int32, device="cuda")
        capi.launch_block_mark_seeds(nodes, n, table, stream)
        counts = torch.empty(nodes.numel(), dtype=torch.int32, device="cuda")

        def launches(group):
            capi.launch_subgraph_count(indptr, indices, n, nodes, table, group, counts, stream)
            capi.launch_subgraph_fill(indptr, indices, n, nodes, table, group, s_indptr, s_local, s_entries, stream)

        for group in GROUPS:
            stats = _stats(_windows(lambda: launches(group), steps, warmup, rounds, events=True))
            line.update({f"kernels_g{group}_" + key: v for key, v in stats.items()})
        line["best_group"] = min(GROUPS, key=lambda group: line[f"kernels_g{group}_ms"])
        try:
            got = composite_subgraph(indptr, indices, nodes, nodes, n)
            assert all(torch.equal(a, b) for a, b in zip(got, result)), "the composite and subgraph_csr disagree"
            del got
            torch_ms = _windows(lambda: composite_subgraph(indptr, indices, nodes, nodes, n), torch_steps, 1, rounds)
            line.update({"torch_" + key: v for key, v in _stats(torch_ms).items()})
            line["speedup_call_over_torch"] = round(line["torch_ms"] / line["call_ms"], 2)
        except torch.cuda.OutOfMemoryError:                  # the composite's temporaries do not fit: recorded, not hidden
            line["torch_ms"], line["torch_out_of_memory"] = None, True
        torch.cuda.empty_cache()
        print(json.dumps(line), flush=True)
        del result, s_indptr, s_local, s_entries, table, counts


def bench_walk(base, indptr, indices, steps, warmup, rounds):
    n = indptr.numel() - 1
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator("cuda").manual_seed(2)
    for walkers in (1000, 100000):
        starts = torch.randint(0, n, (walkers,), device="cuda", generator=gen).int()
        for length in (4, 16):
            nodes, entries = voltrix.random_walk(indptr, indices, starts, length, SEED, 0)
            alive = entries >= 0
            assert torch.equal(indices[entries[alive].long()], nodes[:, 1:][alive]), "a step does not follow its entry"
            nodes_t = torch.empty(length + 1, walkers, dtype=torch.int32, device="cuda")
            entries_t = torch.empty(length, walkers, dtype=torch.int32, device="cuda")

            def step_major():
                capi.launch_random_walk(indptr, indices, n, starts, length, SEED, 0, nodes_t, entries_t, stream, step_major=True)
                return nodes_t.t().contiguous(), entries_t.t().contiguous()

            assert all(torch.equal(a, b) for a, b in zip(step_major(), (nodes, entries))), "step-major stores give another walk"
            line = dict(base, measurement="random_walk", num_walkers=walkers, length=length, ended_early=int((~alive).any(1).sum()))
            call = _windows(lambda: voltrix.random_walk(indptr, indices, starts, length, SEED, 0), steps, warmup, rounds)
            line.update({"call_" + key: v for key, v in _stats(call).items()})
            direct = _windows(lambda: capi.launch_random_walk(indptr, indices, n, starts, length, SEED, 0, nodes, entries, stream), steps,
                              warmup, rounds, events=True)
            line.update({"kernel_walker_major_" + key: v for key, v in _stats(direct).items()})
            line.update({"kernel_step_major_and_transpose_" + key: v for key, v in
                         _stats(_windows(step_major, steps, warmup, rounds, events=True)).items()})
            print(json.dumps(line), flush=True)


def bench_rw_subgraph(base, indptr, indices, steps, warmup, rounds, roots_count, length):
    n = indptr.numel() - 1
    roots = torch.randint(0, n, (roots_count,), device="cuda", generator=torch.Generator("cuda").manual_seed(3)).int()
    sub = voltrix.sample_subgraph_rw(indptr, indices, roots, length, SEED, 0)
    line = dict(base, measurement="sample_subgraph_rw", roots=roots_count, length=length, num_nodes=sub.num_nodes,
                num_edges=sub.pattern.num_edges)
    line.update(_stats(_windows(lambda: voltrix.sample_subgraph_rw(indptr, indices, roots, length, SEED, 0), steps, warmup, rounds)))
    none = torch.empty(0, dtype=torch.int32, device="cuda")

    def phases():
        marks = [time.perf_counter()]

        def mark():
            torch.cuda.synchronize()
            marks.append(time.perf_counter())

        torch.cuda.synchronize()
        marks[0] = time.perf_counter()
        nodes, _ = voltrix.random_walk(indptr, indices, roots, length, SEED, 0)
        mark()
        visited, _ = voltrix.compact_block(none, nodes.view(-1), n)
        mark()
        s_indptr, s_local, _ = voltrix.subgraph_csr(indptr, indices, visited)
        mark()
        CsrPattern(s_indptr, s_local, visited.numel(), visited.numel())
        mark()
        return dict(zip(("walk", "distinct", "subgraph", "pattern"), ((b - a) * 1e3 for a, b in zip(marks, marks[1:]))))

    for _ in range(warmup):
        phases()
    runs = [phases() for _ in range(steps)]
    for key in ("walk", "distinct", "subgraph", "pattern"):
        line[f"phase_{key}_ms"] = round(sorted(r[key] for r in runs)[len(runs) // 2], 4)
    # what a call pays whatever the batch's size, alone, at this graph's size: two table clears, one cumsum over the table, three
    # read-backs
    table = torch.zeros(n, dtype=torch.int32, device="cuda")
    table[::7] = 1
    pair = torch.zeros(2, dtype=torch.int64, device="cuda")
    line["table_clear_ms"] = _stats(_windows(lambda: torch.zeros(n, dtype=torch.int32, device="cuda"), steps, warmup, rounds, True))["ms"]
    line["cumsum_ms"] = _stats(_windows(lambda: torch.cumsum(table > 0, 0, dtype=torch.int32), steps, warmup, rounds, True))["ms"]
    line["read_back_ms"] = _stats(_windows(lambda: pair.tolist(), steps, warmup, rounds))["ms"]
    fixed = 2 * line["table_clear_ms"] + line["cumsum_ms"] + 3 * line["read_back_ms"]
    line["fixed_ms_per_call"] = round(fixed, 4)
    line["fixed_share_of_call"] = round(fixed / line["ms"], 3)
    print(json.dumps(line), flush=True)


def run_graph(name, scale, steps, warmup, rounds, torch_steps, roots, length):
    indptr, indices, _ = synth_graphs.generate(name, device="cuda", scale=scale)
    n, nnz = indptr.numel() - 1, indices.numel()
    deg = indptr[1:] - indptr[:-1]
    base = {"graph": name, "scale": scale, "num_rows": n, "entries": nnz, "max_deg": int(deg.max()), "steps": steps, "rounds": rounds}
    bench_subgraph(base, indptr, indices, steps, warmup, rounds, torch_steps)
    bench_walk(base, indptr, indices, steps, warmup, rounds)
    bench_rw_subgraph(base, indptr, indices, steps, warmup, rounds, roots, length)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", nargs="*", default=list(DEFAULT_CASES), help="synth_graphs stand-in names")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per measurement (their min / max is the spread)")
    ap.add_argument("--torch-steps", type=int, default=2, help="timed calls of the torch composite per window")
    ap.add_argument("--roots", type=int, default=1024)
    ap.add_argument("--length", type=int, default=4)
    ap.add_argument("--scale", type=float, default=1.0, help="synth_graphs scale of every stand-in")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_subgraph.py needs a GPU"
    for name in args.cases:
        run_graph(name, args.scale, args.steps, args.warmup, args.rounds, args.torch_steps, args.roots, args.length)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
