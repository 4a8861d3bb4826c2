"""A two-layer PNA trained with the multi-aggregate operator of this package (example; no reference counterpart -- the reference is
forward-only and sums).

    h_i = W [ S(d_i) (x) A({x_j : j in N(i)}) ] + W_s x_i         (Corso et al., Principal Neighbourhood Aggregation)

with the aggregators A = (mean, max, min, std) and the degree scalers S = (identity, amplification log(d + 1) / delta, attenuation
delta / log(d + 1)), delta the mean of log(d + 1) over the graph.  The four aggregates are `voltrix.autograd.SpMMMulti`: ONE gather
forward, one gather on the transposed CSR backward, the std from shifted moments (no E[x^2] - E[x]^2), no [nnz, F] tensor, no scatter,
no float atomics.  The scalers are dense torch multiplications by functions of `indptr`; then one linear layer on [n, 12 F].

    python examples/pna_train.py [workload] [hidden] [epochs]     # synthetic stand-in graph, random features and labels
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "voltrix-spmm_amd")]
os.environ.setdefault("VOLTRIX_CACHE_DIR", os.path.join(REPO, "voltrix-spmm_amd", ".jit_cache"))

import torch  # noqa: E402

AGGREGATORS = ("mean", "max", "min", "std")


def degree_scalers(indptr: torch.Tensor) -> torch.Tensor:
    """float32 [n, 3]: identity, amplification and attenuation of every row; a row without entries gets 1, 0, 0."""
    log_deg = torch.log((indptr[1:] - indptr[:-1]).float() + 1.0)
    delta = log_deg.mean().clamp_min(1e-6)
    occupied = log_deg > 0
    attenuation = torch.where(occupied, delta / log_deg.clamp_min(1e-6), torch.zeros_like(log_deg))
    return torch.stack([torch.ones_like(log_deg), log_deg / delta, attenuation], dim=1)


class PNALayer(torch.nn.Module):
    """``W [scalers (x) aggregates] + W_s x``; ``aggregate``: a ``voltrix.autograd.SpMMMulti`` with the four aggregators."""

    def __init__(self, aggregate, scalers, in_feats, out_feats):
        super().__init__()
        self.aggregate = aggregate
        self.register_buffer("scalers", scalers)                     # [n, 3]
        self.w_self = torch.nn.Linear(in_feats, out_feats)
        self.w_neigh = torch.nn.Linear(3 * len(AGGREGATORS) * in_feats, out_feats, bias=False)

    def forward(self, x):
        towers = self.aggregate(x).flatten(1)                         # [n, 4 F]
        scaled = (self.scalers[:, :, None] * towers[:, None, :]).flatten(1)      # [n, 12 F]
        return self.w_self(x) + self.w_neigh(scaled)


class PNA(torch.nn.Module):
    def __init__(self, aggregate, scalers, in_feats, hidden, classes):
        super().__init__()
        self.l1 = PNALayer(aggregate, scalers, in_feats, hidden)
        self.l2 = PNALayer(aggregate, scalers, hidden, classes)

    def forward(self, x):
        return self.l2(torch.relu(self.l1(x)))


def main():
    import synth_graphs
    from voltrix.autograd import CsrPattern, SpMMMulti

    workload = sys.argv[1] if len(sys.argv) > 1 else "amazon0601_like"
    hidden = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    epochs = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    indptr, indices, _ = synth_graphs.generate(workload, device="cuda")
    n = indptr.numel() - 1
    t0 = time.perf_counter()
    op = SpMMMulti(CsrPattern(indptr, indices, n), aggrs=AGGREGATORS)
    torch.cuda.synchronize()
    print(f"{workload}: N={n} nnz={indices.numel()}; CSR, its transpose and the edge order built in {time.perf_counter() - t0:.2f} s; "
          f"aggregators: {', '.join(AGGREGATORS)}")
    torch.manual_seed(0)
    in_feats, classes = 64, 48
    x = torch.randn(n, in_feats, device="cuda")
    y = torch.randint(0, classes, (n,), device="cuda")
    model = PNA(op, degree_scalers(op.indptr), in_feats, hidden, classes).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)      # 12 F inputs per node: Adam's unit steps add up over a wide layer
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
            print(f"epoch {epoch}: loss {float(loss.detach()):.4f}, {times[-1]:.2f} ms")
    steady = sorted(times[2:])[len(times[2:]) // 2] if len(times) > 2 else times[-1]
    print(f"steady epoch (forward + backward + Adam, full graph): {steady:.2f} ms -- two four-aggregate gathers of width {in_feats} / "
          f"{hidden} per epoch")


if __name__ == "__main__":
    main()
