"""A two-layer GINE trained with the edge-feature aggregation of this package (example; no reference counterpart -- the reference is
forward-only and knows no edge features).

    h_i = MLP((1 + eps) x_i + sum_{j in N(i)} relu(x_j + W_e e_ij))        (Hu et al., "Strategies for Pre-training GNNs": GINE)

The aggregation is `voltrix.autograd.SpMMEdge` with op "add_relu" (one launch forward; the gradient for the projected edge attributes
by one row-parallel launch, the one for x by a gather on the transposed CSR: no [nnz, F] gather of x, no scatter, no float atomics); the
edge projection `Linear_i(e)` and the MLPs are torch.  Node classification on a synthetic graph with [nnz, 8] edge attributes.

    python examples/gine_train.py [workload] [hidden] [epochs]     # synthetic stand-in graph, random features, attributes and labels
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "voltrix-spmm_amd")]
os.environ.setdefault("VOLTRIX_CACHE_DIR", os.path.join(REPO, "voltrix-spmm_amd", ".jit_cache"))

import torch  # noqa: E402


class GINELayer(torch.nn.Module):
    """``MLP((1 + eps) x_i + sum_j relu(x_j + W_e e_ij))``; ``aggregate``: a ``voltrix.autograd.SpMMEdge``; ``eps`` is learnt.  A node
    without neighbours gets the aggregator's zeros, i.e. ``MLP((1 + eps) x_i)``."""

    def __init__(self, aggregate, in_feats, out_feats, edge_feats):
        super().__init__()
        self.aggregate = aggregate
        self.edge = torch.nn.Linear(edge_feats, in_feats)
        self.eps = torch.nn.Parameter(torch.zeros(()))
        self.mlp = torch.nn.Sequential(torch.nn.Linear(in_feats, out_feats), torch.nn.ReLU(), torch.nn.Linear(out_feats, out_feats))

    def forward(self, x, e):
        return self.mlp((1 + self.eps) * x + self.aggregate(x, self.edge(e), "add_relu"))


class GINE(torch.nn.Module):
    def __init__(self, aggregate, in_feats, hidden, classes, edge_feats):
        super().__init__()
        self.l1 = GINELayer(aggregate, in_feats, hidden, edge_feats)
        self.l2 = GINELayer(aggregate, hidden, classes, edge_feats)

    def forward(self, x, e):
        return self.l2(torch.relu(self.l1(x, e)), e)


def main():
    import synth_graphs
    from voltrix.autograd import CsrPattern, SpMMEdge

    workload = sys.argv[1] if len(sys.argv) > 1 else "dd_like"
    hidden = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    epochs = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    indptr, indices, _ = synth_graphs.generate(workload, device="cuda")
    n, nnz = indptr.numel() - 1, indices.numel()
    t0 = time.perf_counter()
    op = SpMMEdge(CsrPattern(indptr, indices, n))
    torch.cuda.synchronize()
    print(f"{workload}: N={n} nnz={nnz}; CSR, its transpose and the edge order built in {time.perf_counter() - t0:.2f} s")
    torch.manual_seed(0)
    in_feats, edge_feats, classes = 64, 8, 16
    x = torch.randn(n, in_feats, device="cuda")
    e = torch.randn(nnz, edge_feats, device="cuda")
    y = torch.randint(0, classes, (n,), device="cuda")
    model = GINE(op, in_feats, hidden, classes, edge_feats).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    times = []
    for epoch in range(epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(model(x, e), y)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        print(f"epoch {epoch}: loss {float(loss.detach()):.4f}, {times[-1]:.2f} ms")
    steady = sorted(times[2:])[len(times[2:]) // 2] if len(times) > 2 else times[-1]
    print(f"steady epoch (forward + backward + Adam, full graph): {steady:.2f} ms -- two add_relu aggregations of width {in_feats} / "
          f"{hidden} per epoch, edge attributes [nnz, {edge_feats}] projected per layer")


if __name__ == "__main__":
    main()
