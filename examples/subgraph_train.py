"""A two-layer mean-aggregation GraphSAGE trained on SUBGRAPH mini-batches (example; no reference counterpart).

    h_i = W_s x_i + W_n mean_{j in N_B(i)} x_j,   N_B(i) = i's neighbours inside the batch B

A batch is a set of nodes; both layers run on the graph restricted to it (`voltrix.induced_subgraph`: a lane group per row, a stable
compaction through the wave's ballot) with `voltrix.autograd.SpMMReduce(sub.pattern, reduce="mean")`, and every node of the batch
contributes to the loss.  Two ways to choose the batch:

    cluster   Cluster-GCN: a contiguous chunk of `voltrix.cluster_order.cluster_permutation`'s order (clusters lie contiguously in it,
              so a chunk is a few whole clusters and the pieces at its two ends);
    rw        GraphSAINT's random-walk sampler: the nodes that `length`-step walks from `roots` random roots visit
              (`voltrix.sample_subgraph_rw`; the same batch on every run for the same seed and offset).

GraphSAINT's normalisation coefficients (the edge and node weights that make the estimator unbiased) are NOT part of this example:
the aggregator is the plain mean over the neighbours that fell into the batch.

    python examples/subgraph_train.py [cluster|rw] [workload] [hidden] [steps] [batch] [scale]

on a synthetic stand-in graph with random features and labels that are a linear function of them.
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "voltrix-spmm_amd")]
os.environ.setdefault("VOLTRIX_CACHE_DIR", os.path.join(REPO, "voltrix-spmm_amd", ".jit_cache"))

import torch  # noqa: E402

WALK_LENGTH = 4


class SubgraphSAGELayer(torch.nn.Module):
    """``W_s x_i + W_n mean_{j in N_B(i)} x_j`` on one induced subgraph; a node without neighbours in the batch gets the mean's zeros."""

    def __init__(self, in_feats, out_feats):
        super().__init__()
        self.w_self = torch.nn.Linear(in_feats, out_feats)
        self.w_neigh = torch.nn.Linear(in_feats, out_feats, bias=False)

    def forward(self, aggregate, x):
        return self.w_self(x) + self.w_neigh(aggregate(x))


class SubgraphSAGE(torch.nn.Module):
    def __init__(self, in_feats, hidden, classes):
        super().__init__()
        self.l1 = SubgraphSAGELayer(in_feats, hidden)
        self.l2 = SubgraphSAGELayer(hidden, classes)

    def forward(self, sub, x):
        """``sub``: a ``voltrix.Subgraph``; ``x``: the features of ``sub.node_ids``."""
        from voltrix.autograd import SpMMReduce

        aggregate = SpMMReduce(sub.pattern, reduce="mean")          # one pattern, one transpose, both layers
        return self.l2(aggregate, torch.relu(self.l1(aggregate, x)))


def train_step(model, opt, sub, x, y):
    """One optimiser step on the subgraph ``sub``; returns the loss (a device scalar)."""
    ids = sub.node_ids.long()
    opt.zero_grad(set_to_none=True)
    loss = torch.nn.functional.cross_entropy(model(sub, x[ids]), y[ids])
    loss.backward()
    opt.step()
    return loss.detach()


def cluster_batches(indptr, indices, batch):
    """The int32 node sets of Cluster-GCN batches: contiguous chunks of ``batch`` nodes of the cluster order."""
    from voltrix.cluster_order import cluster_permutation

    order = cluster_permutation(indptr, indices, indptr.numel() - 1).int()
    return [order[first:first + batch].contiguous() for first in range(0, order.numel(), batch)]


def main():
    import synth_graphs
    import voltrix

    mode = sys.argv[1] if len(sys.argv) > 1 else "cluster"
    workload = sys.argv[2] if len(sys.argv) > 2 else "reddit_like"
    hidden = int(sys.argv[3]) if len(sys.argv) > 3 else 128
    steps = int(sys.argv[4]) if len(sys.argv) > 4 else 30
    batch = int(sys.argv[5]) if len(sys.argv) > 5 else 4096
    scale = float(sys.argv[6]) if len(sys.argv) > 6 else 0.1
    if mode not in ("cluster", "rw"):
        raise SystemExit(f"mode must be cluster or rw, got {mode!r}")
    indptr, indices, _ = synth_graphs.generate(workload, device="cuda", scale=scale)
    n = indptr.numel() - 1
    torch.manual_seed(0)
    in_feats, classes = 128, 48
    x = torch.randn(n, in_feats, device="cuda")
    y = (x @ torch.randn(in_feats, classes, device="cuda")).argmax(1)           # labels a model can learn: the loss falls across batches
    model = SubgraphSAGE(in_feats, hidden, classes).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    if mode == "cluster":
        t0 = time.perf_counter()
        batches = cluster_batches(indptr, indices, batch)
        torch.cuda.synchronize()
        print(f"{workload} x{scale}: N={n} nnz={indices.numel()}; {len(batches)} cluster batches of {batch} nodes "
              f"(cluster order: {time.perf_counter() - t0:.2f} s, once)")
    else:
        roots = max(1, batch // (WALK_LENGTH + 1))
        print(f"{workload} x{scale}: N={n} nnz={indices.numel()}; random-walk batches: {roots} roots, {WALK_LENGTH} steps")
    times, sizes = [], []
    for step in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if mode == "cluster":
            sub = voltrix.induced_subgraph(indptr, indices, batches[step % len(batches)])
        else:
            picks = torch.randint(0, n, (roots,), device="cuda", dtype=torch.int32)
            sub = voltrix.sample_subgraph_rw(indptr, indices, picks, WALK_LENGTH, seed=1234, offset=step)
        loss = train_step(model, opt, sub, x, y)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        sizes.append((sub.num_nodes, sub.pattern.num_edges))
        if step in (0, 1, steps - 1):
            print(f"step {step}: loss {float(loss):.4f}, {sub.num_nodes} nodes, {sub.pattern.num_edges} edges, {times[-1]:.2f} ms")
    steady = sorted(times[2:])[len(times[2:]) // 2] if len(times) > 2 else times[-1]
    print(f"steady step (subgraph + forward + backward + Adam): {steady:.2f} ms; "
          f"mean batch {sum(s[0] for s in sizes) / len(sizes):.0f} nodes, {sum(s[1] for s in sizes) / len(sizes):.0f} edges")


if __name__ == "__main__":
    main()
