#!/usr/bin/env python3
"""Time neighbour sampling with an exclusion list (``voltrix.sample_neighbors(..., exclude=)``), the (row, column) -> entry lookup
(``voltrix.find_edges``) and edge mini-batches that keep their edges out of their blocks (``sample_edge_batch(...,
exclude_edges="reverse")``) on synth_graphs stand-ins.

Per graph, in one process on one GPU:
  * an exclusion list of 2,048 entries: 1,024 random CSR entries and, where ``find_edges`` finds them, their reverses, filled up with
    further random entries; ``sample_neighbors`` for the distinct endpoints of those edges (the rows the exclusions lie in) and 8,192
    random rows at fan-outs 10 and 25, with and without replacement: the whole call (the one read-back included) on the host clock and
    the HIP launch alone between device events, each against the plain call / launch on the same seeds and fan-outs;
  * ``find_edges`` on 2^16 pairs, half of them the reverses of random entries and half random: the call (no read-back in it) and the
    launch alone between device events, against the torch composite -- a 64-bit key ``row * num_cols + col`` and ``searchsorted``
    against the sorted keys of ALL entries, with the key array built beforehand (8 bytes per entry of the graph) -- and what building
    the keys costs; at a smaller count the linear-scan kernel (``assume_sorted=False``) as well, for the record;
  * one 1,024-edge ``sample_edge_batch`` with 5 negatives and fan-outs (10, 25): ``exclude_edges="reverse"`` and ``"self"`` against
    ``None``.
One JSON line per graph and measurement: the median of ``--rounds`` windows of ``--steps`` calls in milliseconds, and the windows' min
and max (the spread).  Results are checked against the rule's invariants before anything is timed."""
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

from bench_negative_sample import composite_keys  # noqa: E402
from bench_sample_neighbors import _stats, _windows  # noqa: E402

DEFAULT_CASES = ("amazon0601_like", "reddit_like", "products_like")
SEED = 20261020


def composite_find(keys, rows, cols, num_cols):
    """The torch lookup this package replaces: the first entry with the pair's key, -1 if there is none."""
    key = rows.long() * num_cols + cols.long()
    at = torch.searchsorted(keys, key).clamp_(max=keys.numel() - 1)
    return torch.where(keys[at] == key, at, torch.full_like(at, -1))


def run_graph(name, scale, steps, warmup, rounds, torch_steps, batch, extra_seeds, queries):
    indptr, indices, _ = synth_graphs.generate(name, device="cuda", scale=scale)
    n, nnz = indptr.numel() - 1, indices.numel()
    deg = indptr[1:] - indptr[:-1]
    base = {"graph": name, "scale": scale, "num_rows": n, "entries": nnz, "max_deg": int(deg.max()), "steps": steps, "rounds": rounds}
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator("cuda").manual_seed(1)
    entries = torch.randint(0, nnz, (batch,), device="cuda", generator=gen, dtype=torch.int32)
    src, dst = voltrix.edge_endpoints(indptr, indices, entries)
    # ---- the exclusion list: the edges, their reverses where they exist, further entries up to 2 * batch
    reverse = voltrix.find_edges(indptr, indices, dst, src)
    found = int((reverse >= 0).sum())
    spare = torch.randint(0, nnz, (4 * batch,), device="cuda", generator=gen, dtype=torch.int32)
    exclude = torch.unique(torch.cat([entries, reverse[reverse >= 0], spare]))
    order = torch.argsort(torch.isin(exclude, torch.cat([entries, reverse[reverse >= 0]])).int(), descending=True, stable=True)
    exclude = torch.sort(exclude[order[:2 * batch]]).values.contiguous()
    assert exclude.numel() == 2 * batch and bool((exclude[1:] > exclude[:-1]).all())
    seeds = torch.cat([torch.unique(torch.cat([src, dst])), torch.randint(0, n, (extra_seeds,), device="cuda", generator=gen, dtype=torch.int32)])
    seeds = seeds[torch.randperm(seeds.numel(), device="cuda", generator=gen)].contiguous()
    for fanout in (10, 25):
        for replace in (False, True):
            plain = voltrix.sample_neighbors(indptr, indices, seeds, fanout, SEED, 0, replace)
            mine = voltrix.sample_neighbors(indptr, indices, seeds, fanout, SEED, 0, replace, exclude=exclude)
            assert not bool(torch.isin(mine[2], exclude).any()), "an excluded entry was sampled"
            assert torch.equal(indices[mine[2].long()], mine[1])
            line = dict(base, measurement="sample_neighbors_exclude", num_seeds=seeds.numel(), num_exclude=exclude.numel(),
                        excluded_entries_the_plain_call_samples=int(torch.isin(plain[2], exclude).sum()),
                        reverses_found=found, fanout=fanout, replace=replace, num_sampled=mine[2].numel(), num_sampled_plain=plain[2].numel())
            for tag, kwargs in (("plain_call_", {}), ("call_", {"exclude": exclude})):
                ms = _windows(lambda: voltrix.sample_neighbors(indptr, indices, seeds, fanout, SEED, 0, replace, **kwargs), steps, warmup, rounds)
                line.update({tag + key: v for key, v in _stats(ms).items()})
            ms = _windows(lambda: capi.launch_sample_neighbors(indptr, indices, n, seeds, plain[0], plain[2].numel(), fanout, replace, SEED,
                                                               0, plain[1], plain[2], stream), steps, warmup, rounds, events=True)
            line.update({"plain_kernel_" + key: v for key, v in _stats(ms).items()})
            ms = _windows(lambda: capi.launch_sample_neighbors(indptr, indices, n, seeds, mine[0], mine[2].numel(), fanout, replace, SEED,
                                                               0, mine[1], mine[2], stream, exclude=exclude),
                          steps, warmup, rounds, events=True)
            line.update({"kernel_" + key: v for key, v in _stats(ms).items()})
            line["call_over_plain"] = round(line["call_ms"] / line["plain_call_ms"], 3)
            line["kernel_over_plain"] = round(line["kernel_ms"] / line["plain_kernel_ms"], 3)
            print(json.dumps(line), flush=True)
    # ---- find_edges
    some = torch.randint(0, nnz, (queries // 2,), device="cuda", generator=gen, dtype=torch.int32)
    q_src, q_dst = voltrix.edge_endpoints(indptr, indices, some)
    rows = torch.cat([q_dst, torch.randint(0, n, (queries - queries // 2,), device="cuda", generator=gen, dtype=torch.int32)]).contiguous()
    cols = torch.cat([q_src, torch.randint(0, n, (queries - queries // 2,), device="cuda", generator=gen, dtype=torch.int32)]).contiguous()
    ids = voltrix.find_edges(indptr, indices, rows, cols)
    line = dict(base, measurement="find_edges", num_queries=queries, num_found=int((ids >= 0).sum()),
                mean_degree_of_rows=round(float(deg[rows.long()].float().mean()), 1))
    try:
        keys = composite_keys(indptr, indices, n)
        assert torch.equal(composite_find(keys, rows, cols, n), ids.long()), "find_edges against the key search"
        keys_ms = _stats(_windows(lambda: composite_keys(indptr, indices, n), torch_steps, 1, rounds))
        ms = _windows(lambda: composite_find(keys, rows, cols, n), steps, warmup, rounds, events=True)
        line.update({"torch_" + key: v for key, v in _stats(ms).items()})
        line["torch_keys_ms"], line["torch_keys_bytes"] = keys_ms["ms"], 8 * nnz
    except torch.cuda.OutOfMemoryError:                  # the composite's 8 bytes per entry do not fit: recorded, not hidden
        keys = None
        line["torch_ms"], line["torch_out_of_memory"] = None, True
    ms = _windows(lambda: voltrix.find_edges(indptr, indices, rows, cols), steps, warmup, rounds, events=True)
    line.update({"call_" + key: v for key, v in _stats(ms).items()})
    out = torch.empty_like(ids)
    ms = _windows(lambda: capi.launch_find_edges(indptr, indices, n, rows, cols, True, out, stream), steps, warmup, rounds, events=True)
    line.update({"kernel_" + key: v for key, v in _stats(ms).items()})
    few = max(1, queries // 64)
    scan_out = torch.empty(few, dtype=torch.int32, device="cuda")
    ms = _windows(lambda: capi.launch_find_edges(indptr, indices, n, rows[:few].contiguous(), cols[:few].contiguous(), False, scan_out, stream),
                  torch_steps, 1, rounds, events=True)
    line.update({"scan_kernel_" + key: v for key, v in _stats(ms).items()})
    line["scan_queries"] = few
    assert torch.equal(scan_out, ids[:few]), "scan against the lower bound"
    if keys is not None:
        line["torch_over_call"] = round(line["torch_ms"] / line["call_ms"], 2)
        line["torch_over_kernel"] = round(line["torch_ms"] / line["kernel_ms"], 2)
    print(json.dumps(line), flush=True)
    del keys
    torch.cuda.empty_cache()
    # ---- a whole edge batch
    fanouts, negatives = (10, 25), 5
    line = dict(base, measurement="sample_edge_batch_exclude", batch=batch, num_negatives=negatives, fanouts=list(fanouts))
    for mode in (None, "self", "reverse"):
        made = voltrix.sample_edge_batch(indptr, indices, entries, negatives, fanouts, SEED, 0, exclude_edges=mode)
        held = [int(torch.isin(b.entries, entries).sum()) for b in made.blocks]
        assert mode is None or sum(held) == 0, "a batch edge in a block"
        tag = "none" if mode is None else mode
        line[f"{tag}_batch_edges_in_blocks"] = held
        line[f"{tag}_num_src"] = [b.num_src for b in made.blocks]
        ms = _windows(lambda: voltrix.sample_edge_batch(indptr, indices, entries, negatives, fanouts, SEED, 0, exclude_edges=mode),
                      steps, warmup, rounds)
        line.update({f"{tag}_" + key: v for key, v in _stats(ms).items()})
    line["reverse_over_none"] = round(line["reverse_ms"] / line["none_ms"], 3)
    line["self_over_none"] = round(line["self_ms"] / line["none_ms"], 3)
    print(json.dumps(line), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", nargs="*", default=list(DEFAULT_CASES), help="synth_graphs stand-in names")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per measurement (their min / max is the spread)")
    ap.add_argument("--torch-steps", type=int, default=2, help="timed calls of building the keys (and of the scan kernel) per window")
    ap.add_argument("--batch", type=int, default=1024, help="edges of the batch: the exclusion list holds twice as many entries")
    ap.add_argument("--extra-seeds", type=int, default=8192, help="random seed rows next to the batch's endpoints")
    ap.add_argument("--queries", type=int, default=2 ** 16, help="pairs of the find_edges measurement")
    ap.add_argument("--scale", type=float, default=1.0, help="synth_graphs scale of every stand-in")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_sample_exclude.py needs a GPU"
    for name in args.cases:
        run_graph(name, args.scale, args.steps, args.warmup, args.rounds, args.torch_steps, args.batch, args.extra_seeds, args.queries)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
