"""Link prediction with a two-layer GraphSAGE encoder on edge mini-batches (example; no reference counterpart).

    h = SAGE(blocks, x)                  one row per node of the batch: sources, destinations, negatives
    s(u, v) = <h_u, h_v>                 the dot-product decoder, one score per (source, candidate) pair
    loss = BCE(s, label)                 label 1 for an edge of the graph, 0 for a sampled non-neighbour

Every step takes `batch` entries of the graph's CSR as positive edges.  `voltrix.sample_edge_batch` finds their endpoints (a search in
`indptr` per entry), draws `NEGATIVES` non-neighbours per source (HIP kernels; the same batch on every run for the same seed and
offset), and samples the two-hop neighbourhood of every node involved with `voltrix.sample_blocks`.  The scores are
`voltrix.autograd.SDDMM(batch.pairs)(h[batch.src_local], h)`: the pair pattern goes into the operator as it is, and the gradient
reaches `h` through both operands.

THE BATCH STAYS OUT OF ITS BLOCKS.  Blocks drawn from the full graph would let the encoder aggregate over the very edge (and its
reverse) that it is asked to predict.  `main()` passes `exclude_edges="reverse"`: `sample_edge_batch` looks up the reverse `(v, u)`
of every positive edge `(u, v)` with `voltrix.find_edges` and samples every layer among the entries that are neither a batch edge nor
such a reverse (DGL's `exclude="reverse_id"`).  `none` as the last command-line argument gives the blocks of the full
graph, for comparison.  On the random features of this example nothing can be learnt beyond the graph's structure: the example shows
the plumbing and the cost of a step, not a result.

    python examples/linkpred_train.py [workload] [hidden] [steps] [batch] [reverse|self|none]   # synthetic stand-in graph, random features
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "voltrix-spmm_amd")]
os.environ.setdefault("VOLTRIX_CACHE_DIR", os.path.join(REPO, "voltrix-spmm_amd", ".jit_cache"))

import torch  # noqa: E402

FANOUTS = (10, 25)      # input layer first
NEGATIVES = 5


class BlockSAGELayer(torch.nn.Module):
    """``W_s x_dst + W_n mean_{j in S(i)} x_j`` on one block: ``x`` holds the block's source nodes, the first ``block.num_dst`` of
    them are its destination nodes."""

    def __init__(self, in_feats, out_feats):
        super().__init__()
        self.w_self = torch.nn.Linear(in_feats, out_feats)
        self.w_neigh = torch.nn.Linear(in_feats, out_feats, bias=False)

    def forward(self, block, x):
        from voltrix.autograd import SpMMReduce

        return self.w_self(x[:block.num_dst]) + self.w_neigh(SpMMReduce(block.pattern, reduce="mean")(x))


class LinkPredictor(torch.nn.Module):
    def __init__(self, in_feats, hidden):
        super().__init__()
        self.l1 = BlockSAGELayer(in_feats, hidden)
        self.l2 = BlockSAGELayer(hidden, hidden)

    def forward(self, batch, x):
        """``x``: the features of ``batch.blocks[0].src_ids`` -> one score per entry of ``batch.pairs``."""
        from voltrix.autograd import SDDMM

        h = self.l2(batch.blocks[1], torch.relu(self.l1(batch.blocks[0], x)))        # [len(batch.node_ids), hidden]
        return SDDMM(batch.pairs)(h[batch.src_local.long()], h)


def train_step(model, opt, indptr, indices, x, entries, seed, step, fanouts=FANOUTS, negatives=NEGATIVES, timer=None,
               exclude_edges=None):
    """One optimiser step on the positive edges ``entries`` (int32 CSR entry ids); returns the loss (a device scalar).  ``timer``: a
    list that gets the milliseconds spent in ``sample_edge_batch`` (costs a synchronisation).  ``exclude_edges``: ``sample_edge_batch``'s
    argument -- ``None`` samples the blocks from the full graph, ``"reverse"`` keeps the batch's edges and their reverses out of them."""
    import voltrix

    t0 = time.perf_counter()
    batch = voltrix.sample_edge_batch(indptr, indices, entries, negatives, fanouts, seed=seed, offset=step * len(fanouts),
                                      exclude_edges=exclude_edges)
    if timer is not None:
        torch.cuda.synchronize()
        timer.append((time.perf_counter() - t0) * 1e3)
    opt.zero_grad(set_to_none=True)
    scores = model(batch, x[batch.blocks[0].src_ids.long()])
    loss = torch.nn.functional.binary_cross_entropy_with_logits(scores, batch.labels)
    loss.backward()
    opt.step()
    return loss.detach()


def main():
    import synth_graphs

    workload = sys.argv[1] if len(sys.argv) > 1 else "reddit_like"
    hidden = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 30
    batch = int(sys.argv[4]) if len(sys.argv) > 4 else 1024
    exclude_edges = sys.argv[5] if len(sys.argv) > 5 else "reverse"
    exclude_edges = None if exclude_edges == "none" else exclude_edges
    indptr, indices, _ = synth_graphs.generate(workload, device="cuda")
    n, nnz = indptr.numel() - 1, indices.numel()
    print(f"{workload}: N={n} nnz={nnz}; batches of {batch} edges, {NEGATIVES} negatives per edge, fan-outs {FANOUTS} (input layer first), "
          f"exclude_edges={exclude_edges!r}")
    torch.manual_seed(0)
    in_feats = 128
    x = torch.randn(n, in_feats, device="cuda")
    model = LinkPredictor(in_feats, hidden).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    gen = torch.Generator(device="cuda").manual_seed(1)
    times, sampling = [], []
    for step in range(steps):
        entries = torch.randint(0, nnz, (batch,), device="cuda", generator=gen, dtype=torch.int32)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = train_step(model, opt, indptr, indices, x, entries, seed=1234, step=step, timer=sampling, exclude_edges=exclude_edges)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        if step in (0, 1, steps - 1) or step % 5 == 0:
            print(f"step {step}: loss {float(loss):.4f}, {times[-1]:.2f} ms")
    median = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    steady, sample = (median(times[2:]), median(sampling[2:])) if len(times) > 2 else (times[-1], sampling[-1])
    print(f"steady step (edge batch + forward + backward + Adam): {steady:.2f} ms per batch of {batch} edges; "
          f"sample_edge_batch {sample:.2f} ms of it ({100 * sample / steady:.0f} %)")


if __name__ == "__main__":
    main()
