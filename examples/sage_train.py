"""A two-layer max-pool GraphSAGE trained with the selecting aggregator of this package (example; no reference counterpart -- the
reference is forward-only and sums).

    h_i = W_s x_i + W_n max_{j in N(i)} relu(W_p x_j + b)        (Hamilton, Ying & Leskovec, the pooling aggregator)

The neighbour pooling is `voltrix.autograd.SpMMReduce` (one launch forward, a gather on the transposed CSR backward: no [nnz, F] tensor,
no scatter, no float atomics); the dense half is torch.  `mean` swaps the maximum for the mean of the same pooled features.

    python examples/sage_train.py [workload] [hidden] [epochs] [max|mean]     # synthetic stand-in graph, random features and labels
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "voltrix-spmm_amd")]
os.environ.setdefault("VOLTRIX_CACHE_DIR", os.path.join(REPO, "voltrix-spmm_amd", ".jit_cache"))

import torch  # noqa: E402


class SAGEPoolLayer(torch.nn.Module):
    """``W_s x_i + W_n aggregate_{j in N(i)} relu(W_p x_j + b)``; ``aggregate``: a ``voltrix.autograd.SpMMReduce``.  A node without
    neighbours gets the aggregator's zeros, i.e. ``W_s x_i`` alone."""

    def __init__(self, aggregate, in_feats, out_feats, pool_feats=None):
        super().__init__()
        pool_feats = in_feats if pool_feats is None else pool_feats
        self.aggregate = aggregate
        self.pool = torch.nn.Linear(in_feats, pool_feats)
        self.w_self = torch.nn.Linear(in_feats, out_feats)
        self.w_neigh = torch.nn.Linear(pool_feats, out_feats, bias=False)

    def forward(self, x):
        return self.w_self(x) + self.w_neigh(self.aggregate(torch.relu(self.pool(x))))


class SAGE(torch.nn.Module):
    def __init__(self, aggregate, in_feats, hidden, classes):
        super().__init__()
        self.l1 = SAGEPoolLayer(aggregate, in_feats, hidden)
        self.l2 = SAGEPoolLayer(aggregate, hidden, classes)

    def forward(self, x):
        return self.l2(torch.relu(self.l1(x)))


def main():
    import synth_graphs
    from voltrix.autograd import CsrPattern, SpMMReduce

    workload = sys.argv[1] if len(sys.argv) > 1 else "reddit_like"
    hidden = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    epochs = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    reduce = sys.argv[4] if len(sys.argv) > 4 else "max"
    if reduce not in ("max", "mean"):
        raise SystemExit(f"aggregator must be max or mean, got {reduce!r}")
    indptr, indices, _ = synth_graphs.generate(workload, device="cuda")
    n = indptr.numel() - 1
    t0 = time.perf_counter()
    op = SpMMReduce(CsrPattern(indptr, indices, n), reduce=reduce)
    torch.cuda.synchronize()
    print(f"{workload}: N={n} nnz={indices.numel()}; CSR, its transpose and the edge order built in {time.perf_counter() - t0:.2f} s; "
          f"aggregator: {reduce}")
    torch.manual_seed(0)
    in_feats, classes = 128, 48
    x = torch.randn(n, in_feats, device="cuda")
    y = torch.randint(0, classes, (n,), device="cuda")
    model = SAGE(op, in_feats, hidden, classes).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    times = []
    for epoch in range(epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(model(x), y)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        if epoch in (0, 1, epochs - 1):
            print(f"epoch {epoch}: loss {float(loss):.4f}, {times[-1]:.2f} ms")
    steady = sorted(times[2:])[len(times[2:]) // 2] if len(times) > 2 else times[-1]
    print(f"steady epoch (forward + backward + Adam, full graph): {steady:.2f} ms -- two {reduce} aggregations of width {in_feats} / "
          f"{hidden} per epoch")


if __name__ == "__main__":
    main()
