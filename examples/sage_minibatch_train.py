"""The two-layer max-pool GraphSAGE of examples/sage_train.py trained on sampled mini-batches (example; no reference counterpart).

    h_i = W_s x_i + W_n max_{j in S(i)} relu(W_p x_j + b),   S(i) = at most `fanout` of i's neighbours

Every step draws `batch` output nodes, samples their two-hop neighbourhood with `voltrix.sample_blocks` (HIP kernels: Floyd's sampling
per row, a dense-table relabel; the same blocks on every run for the same seed and offset) and runs the layers on the blocks'
rectangular patterns with `voltrix.autograd.SpMMReduce(block.pattern)`.  A block's source nodes start with its destination nodes, so
the self term is `h[:block.num_dst]`.  The full graph never enters a kernel: a step touches the sampled rows only.

    python examples/sage_minibatch_train.py [workload] [hidden] [steps] [max|mean] [batch] [uniform|inverse_degree]
                                                                                              # synthetic stand-in graph, random data

The last argument chooses the neighbour draws: `uniform` (the default), or `inverse_degree` -- every neighbour j weighted by
1 / in_degree(j) through `voltrix.sampling_weights` and `sample_blocks(prob=)`.
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "voltrix-spmm_amd")]
os.environ.setdefault("VOLTRIX_CACHE_DIR", os.path.join(REPO, "voltrix-spmm_amd", ".jit_cache"))

import torch  # noqa: E402

FANOUTS = (10, 25)      # input layer first: 25 neighbours of every output node, 10 of every node those bring in


class BlockSAGEPoolLayer(torch.nn.Module):
    """``W_s x_dst + W_n aggregate_{j in S(i)} relu(W_p x_j + b)`` on one block: ``x`` holds the block's source nodes, the first
    ``block.num_dst`` of them are its destination nodes.  A node without sampled neighbours gets the aggregator's zeros."""

    def __init__(self, in_feats, out_feats, reduce="max", pool_feats=None):
        super().__init__()
        pool_feats = in_feats if pool_feats is None else pool_feats
        self.reduce = reduce
        self.pool = torch.nn.Linear(in_feats, pool_feats)
        self.w_self = torch.nn.Linear(in_feats, out_feats)
        self.w_neigh = torch.nn.Linear(pool_feats, out_feats, bias=False)

    def forward(self, block, x):
        from voltrix.autograd import SpMMReduce

        aggregate = SpMMReduce(block.pattern, reduce=self.reduce)
        return self.w_self(x[:block.num_dst]) + self.w_neigh(aggregate(torch.relu(self.pool(x))))


class BlockSAGE(torch.nn.Module):
    def __init__(self, in_feats, hidden, classes, reduce="max"):
        super().__init__()
        self.l1 = BlockSAGEPoolLayer(in_feats, hidden, reduce)
        self.l2 = BlockSAGEPoolLayer(hidden, classes, reduce)

    def forward(self, blocks, x):
        """``blocks``: the two blocks of ``voltrix.sample_blocks``, input layer first; ``x``: the features of ``blocks[0].src_ids``."""
        return self.l2(blocks[1], torch.relu(self.l1(blocks[0], x)))


def inverse_degree_weights(indptr, indices):
    """The table of ``voltrix.sampling_weights`` for ``prob[e] = 1 / in_degree(indices[e])``: neighbours that many nodes share are
    drawn less often (importance sampling by inverse degree).  Built once per graph."""
    import voltrix

    in_degree = torch.bincount(indices.long(), minlength=indptr.numel() - 1).clamp(min=1)
    return voltrix.sampling_weights(indptr, (1.0 / in_degree.float())[indices.long()])


def train_step(model, opt, indptr, indices, x, y, batch_nodes, seed, step, fanouts=FANOUTS, prob=None):
    """One optimiser step on the mini-batch of the int32 output nodes ``batch_nodes``; returns the loss (a device scalar).  ``prob``:
    ``None`` (uniform neighbour draws) or a ``voltrix.SamplingWeights`` of the graph (weighted draws)."""
    import voltrix

    blocks = voltrix.sample_blocks(indptr, indices, batch_nodes, fanouts, seed=seed, offset=step * len(fanouts), prob=prob)
    opt.zero_grad(set_to_none=True)
    logits = model(blocks, x[blocks[0].src_ids.long()])
    loss = torch.nn.functional.cross_entropy(logits, y[batch_nodes.long()])
    loss.backward()
    opt.step()
    return loss.detach()


def main():
    import synth_graphs

    workload = sys.argv[1] if len(sys.argv) > 1 else "reddit_like"
    hidden = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 30
    reduce = sys.argv[4] if len(sys.argv) > 4 else "max"
    batch = int(sys.argv[5]) if len(sys.argv) > 5 else 1024
    sampler = sys.argv[6] if len(sys.argv) > 6 else "uniform"
    if reduce not in ("max", "mean"):
        raise SystemExit(f"aggregator must be max or mean, got {reduce!r}")
    if sampler not in ("uniform", "inverse_degree"):
        raise SystemExit(f"sampler must be uniform or inverse_degree, got {sampler!r}")
    indptr, indices, _ = synth_graphs.generate(workload, device="cuda")
    n = indptr.numel() - 1
    prob = inverse_degree_weights(indptr, indices) if sampler == "inverse_degree" else None
    print(f"{workload}: N={n} nnz={indices.numel()}; batches of {batch} nodes, fan-outs {FANOUTS} (input layer first); aggregator: {reduce}; "
          f"neighbour draws: {sampler}")
    torch.manual_seed(0)
    in_feats, classes = 128, 48
    x = torch.randn(n, in_feats, device="cuda")
    y = torch.randint(0, classes, (n,), device="cuda")
    model = BlockSAGE(in_feats, hidden, classes, reduce).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    order = torch.randperm(n, device="cuda").int()
    times = []
    for step in range(steps):
        first = step * batch % max(1, n - batch + 1)
        nodes = order[first:first + batch]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = train_step(model, opt, indptr, indices, x, y, nodes, seed=1234, step=step, prob=prob)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        if step in (0, 1, steps - 1):
            print(f"step {step}: loss {float(loss):.4f}, {times[-1]:.2f} ms")
    steady = sorted(times[2:])[len(times[2:]) // 2] if len(times) > 2 else times[-1]
    print(f"steady step (sampling + relabelling + forward + backward + Adam): {steady:.2f} ms per batch of {batch}")


if __name__ == "__main__":
    main()
