#!/usr/bin/env python3
"""Time negative sampling (``voltrix.negative_sample``), entry endpoints (``voltrix.edge_endpoints``) and edge mini-batches
(``voltrix.sample_edge_batch``) on synth_graphs stand-ins, against the torch composite a user would write without them.

Per graph, in one process on one GPU:
  * a batch of 2^16 random CSR entries; ``edge_endpoints`` on it -- the whole call (the one read-back included) on the host clock, the
    HIP launch alone between device events -- against ``torch.searchsorted(indptr, entries, right=True) - 1`` and a gather;
  * ``negative_sample`` for the sources of those entries at k = 1, 5, 25 (16 tries, binary search): the whole call and the launch alone;
    at k = 1 the linear-scan kernel (``assume_sorted=False``) as well, for the record;
  * baseline, the torch composite on the same sources: ``randint``, a 64-bit key ``row * num_cols + col``, ``searchsorted`` against the
    sorted keys of ALL entries of the graph, a host loop that redraws the rejected candidates (16 rounds at most).  Timed with the key
    array built beforehand (what a training loop would cache: 8 bytes per entry of the graph) and with building it;
  * a 1,024-edge ``sample_edge_batch`` with 5 negatives and fan-outs (10, 25): the whole call, and its phases (endpoints, negatives,
    distinct nodes, blocks, pairs) bracketed by synchronisations.
One JSON line per graph and measurement: the median of ``--rounds`` windows of ``--steps`` calls in milliseconds, and the windows' min
and max (the spread).  Results are checked against the rule's invariants before anything is timed."""
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

from bench_sample_neighbors import _stats, _windows  # noqa: E402

DEFAULT_CASES = ("amazon0601_like", "reddit_like", "products_like")
SEED = 20261019
TRIES = 16


def composite_keys(indptr, indices, num_cols):
    """The sorted int64 keys ``row * num_cols + col`` of every entry (rows ascend in the stand-ins, so no sort is needed)."""
    deg = (indptr[1:] - indptr[:-1]).long()
    rows = torch.repeat_interleave(torch.arange(deg.numel(), device=indptr.device), deg)
    return rows * num_cols + indices.long()


def composite_negative(keys, src, k, num_cols, rounds=TRIES):
    """The torch sampler this package replaces: ``neg`` int64 ``[S, k]``, uniform among the non-neighbours, -1 where ``rounds`` redraws
    did not do.  Every round reads the number of rejected candidates back.  Not reproducible across runs."""
    dev = src.device
    row_key = src.long().repeat_interleave(k) * num_cols
    neg = torch.randint(0, num_cols, (row_key.numel(),), device=dev)
    pending = torch.arange(row_key.numel(), device=dev)
    for _ in range(rounds):
        key = row_key[pending] + neg[pending]
        at = torch.searchsorted(keys, key).clamp_(max=keys.numel() - 1)
        pending = pending[keys[at] == key]                               # a read-back
        if pending.numel() == 0:
            break
        neg[pending] = torch.randint(0, num_cols, (pending.numel(),), device=dev)
    else:
        key = row_key[pending] + neg[pending]
        at = torch.searchsorted(keys, key).clamp_(max=keys.numel() - 1)
        neg[pending[keys[at] == key]] = -1
    return neg.view(-1, k)


def _check_negatives(keys, src, neg, num_cols):
    taken = neg >= 0
    key = (src.long()[:, None] * num_cols + neg.long())[taken]
    at = torch.searchsorted(keys, key).clamp_(max=keys.numel() - 1)
    assert not bool((keys[at] == key).any()), "a neighbour among the negatives"
    assert bool((neg[taken] < num_cols).all()), "a column out of range"


def run_graph(name, scale, steps, warmup, rounds, torch_steps, entries_count, batch):
    indptr, indices, _ = synth_graphs.generate(name, device="cuda", scale=scale)
    n, nnz = indptr.numel() - 1, indices.numel()
    deg = indptr[1:] - indptr[:-1]
    base = {"graph": name, "scale": scale, "num_rows": n, "entries": nnz, "max_deg": int(deg.max()), "steps": steps, "rounds": rounds}
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator("cuda").manual_seed(1)
    entries = torch.randint(0, nnz, (entries_count,), device="cuda", generator=gen, dtype=torch.int32)
    # ---- endpoints
    src, dst = voltrix.edge_endpoints(indptr, indices, entries)
    want = torch.searchsorted(indptr, entries, right=True) - 1
    assert torch.equal(src.long(), want.long()) and torch.equal(dst, indices[entries.long()]), "endpoints"
    line = dict(base, measurement="edge_endpoints", num_ids=entries_count)
    line.update({"call_" + key: v for key, v in _stats(_windows(lambda: voltrix.edge_endpoints(indptr, indices, entries), steps, warmup,
                                                                 rounds)).items()})
    rows, cols = torch.empty_like(src), torch.empty_like(dst)
    line.update({"kernel_" + key: v for key, v in _stats(_windows(
        lambda: capi.launch_edge_endpoints(indptr, indices, n, entries, rows, cols, stream), steps, warmup, rounds, events=True)).items()})
    line.update({"torch_" + key: v for key, v in _stats(_windows(
        lambda: (torch.searchsorted(indptr, entries, right=True) - 1, indices[entries.long()]), steps, warmup, rounds, events=True)).items()})
    print(json.dumps(line), flush=True)
    # ---- negatives
    mean_src_deg = float(deg[src.long()].float().mean())
    try:
        keys = composite_keys(indptr, indices, n)
        keys_ms = _stats(_windows(lambda: composite_keys(indptr, indices, n), torch_steps, 1, rounds))
    except torch.cuda.OutOfMemoryError:                  # the composite's 8 bytes per entry do not fit: recorded, not hidden
        keys, keys_ms = None, None
    for k in (1, 5, 25):
        neg, exhausted = voltrix.negative_sample(indptr, indices, src, k, SEED, 0, None, TRIES)
        if keys is not None:
            _check_negatives(keys, src, neg, n)
        line = dict(base, measurement="negative_sample", num_src=entries_count, k=k, max_tries=TRIES, num_exhausted=exhausted,
                    mean_degree_of_sources=round(mean_src_deg, 1))
        call = _windows(lambda: voltrix.negative_sample(indptr, indices, src, k, SEED, 0, None, TRIES), steps, warmup, rounds)
        launch = _windows(lambda: capi.launch_negative_sample(indptr, indices, n, n, src, k, TRIES, False, True, SEED, 0, neg, stream),
                          steps, warmup, rounds, events=True)
        line.update({"call_" + key: v for key, v in _stats(call).items()})
        line.update({"kernel_" + key: v for key, v in _stats(launch).items()})
        line["kernel_ns_per_slot"] = round(line["kernel_ms"] * 1e6 / (entries_count * k), 3)
        if k == 1:
            scan = _windows(lambda: capi.launch_negative_sample(indptr, indices, n, n, src, k, TRIES, False, False, SEED, 0, neg, stream),
                            torch_steps, 1, rounds, events=True)
            line.update({"scan_kernel_" + key: v for key, v in _stats(scan).items()})
        if keys is not None:
            _check_negatives(keys, src, composite_negative(keys, src, k, n), n)
            torch_ms = _windows(lambda: composite_negative(keys, src, k, n), torch_steps, 1, rounds)
            line.update({"torch_" + key: v for key, v in _stats(torch_ms).items()})
            line["torch_keys_ms"], line["torch_keys_bytes"] = keys_ms["ms"], 8 * nnz
            line["speedup_call_over_torch"] = round(line["torch_ms"] / line["call_ms"], 2)
            line["speedup_call_over_torch_with_keys"] = round((line["torch_ms"] + keys_ms["ms"]) / line["call_ms"], 2)
        else:
            line["torch_ms"], line["torch_out_of_memory"] = None, True
        print(json.dumps(line), flush=True)
    del keys
    torch.cuda.empty_cache()
    # ---- a whole edge batch
    fanouts, negatives = (10, 25), 5
    some = entries[:batch].contiguous()
    made = voltrix.sample_edge_batch(indptr, indices, some, negatives, fanouts, SEED, 0)
    assert torch.equal(made.blocks[-1].dst_ids, made.node_ids) and made.pairs.num_edges == batch * (negatives + 1) - made.num_exhausted
    line = dict(base, measurement="sample_edge_batch", batch=batch, num_negatives=negatives, fanouts=list(fanouts),
                num_nodes=made.node_ids.numel(), num_src=[b.num_src for b in made.blocks], num_exhausted=made.num_exhausted)
    line.update(_stats(_windows(lambda: voltrix.sample_edge_batch(indptr, indices, some, negatives, fanouts, SEED, 0), steps, warmup, rounds)))

    def phases():
        times, marks = {}, [time.perf_counter()]

        def mark(key):
            torch.cuda.synchronize()
            marks.append(time.perf_counter())
            times[key] = (marks[-1] - marks[-2]) * 1e3

        torch.cuda.synchronize()
        marks[0] = time.perf_counter()
        s, d = voltrix.edge_endpoints(indptr, indices, some)
        mark("endpoints")
        negs, _ = voltrix.negative_sample(indptr, indices, s, negatives, SEED, 0, None, TRIES, True)
        mark("negatives")
        none = torch.empty(0, dtype=torch.int32, device="cuda")
        ids, local = voltrix.compact_block(none, torch.cat([s, d, negs.view(-1)]), n)
        mark("nodes")
        voltrix.sample_blocks(indptr, indices, ids, fanouts, SEED, 0)
        mark("blocks")
        p_indptr = torch.arange(0, batch * (negatives + 1) + 1, negatives + 1, dtype=torch.int32, device="cuda")
        CsrPattern(p_indptr, local[batch:].clamp(min=0).contiguous(), batch, ids.numel())
        mark("pairs")
        return times

    for _ in range(warmup):
        phases()
    runs = [phases() for _ in range(steps)]
    for key in ("endpoints", "negatives", "nodes", "blocks", "pairs"):
        line[f"phase_{key}_ms"] = round(sorted(r[key] for r in runs)[len(runs) // 2], 4)
    print(json.dumps(line), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", nargs="*", default=list(DEFAULT_CASES), help="synth_graphs stand-in names")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per measurement (their min / max is the spread)")
    ap.add_argument("--torch-steps", type=int, default=2, help="timed calls of the torch composite (and of the scan kernel) per window")
    ap.add_argument("--entries", type=int, default=2 ** 16, help="CSR entries whose sources are sampled for")
    ap.add_argument("--batch", type=int, default=1024, help="edges of the sample_edge_batch measurement")
    ap.add_argument("--scale", type=float, default=1.0, help="synth_graphs scale of every stand-in")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_negative_sample.py needs a GPU"
    for name in args.cases:
        run_graph(name, args.scale, args.steps, args.warmup, args.rounds, args.torch_steps, args.entries, args.batch)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
