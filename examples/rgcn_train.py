"""A two-layer R-GCN with basis decomposition trained with the relational aggregation of this package (example; no reference
counterpart -- the reference is forward-only and knows no edge types).

    h_i' = sigma( W_0 h_i + sum_r sum_{j in N_r(i)} 1 / c_{i,r} W_r h_j ),   W_r = sum_b coef[r, b] V_b     (Schlichtkrull et al.)

Aggregate first, transform after: `voltrix.autograd.SpMMRel` gives ``agg[i, b] = sum_e norm_e coef[etype_e, b] h[col_e]`` ([n, B, F]:
one launch forward, the gradient for h by a gather on the transposed CSR, the one for coef by one row-parallel launch and two
fixed-order row sums: no [nnz, ., F] messages, no R dense products, no float atomics); ``agg.view(n, B F) @ V.view(B F, F_out)``, the
self-loop ``W_0`` and the activation are torch.  ``norm`` is `voltrix.spmm_rel.type_norm`.  Node classification on a synthetic graph
whose edge types are drawn per edge.

    python examples/rgcn_train.py [workload] [hidden] [epochs] [relations] [bases]     # synthetic stand-in graph, random features
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "voltrix-spmm_amd")]
os.environ.setdefault("VOLTRIX_CACHE_DIR", os.path.join(REPO, "voltrix-spmm_amd", ".jit_cache"))

import torch  # noqa: E402


class RGCNLayer(torch.nn.Module):
    """``W_0 h + (sum_e norm_e coef[etype_e] (x) h[col_e]).view(n, B F) @ V``; ``aggregate``: a ``voltrix.autograd.SpMMRel``.  A node
    without neighbours gets the aggregator's zeros, i.e. ``W_0 h``."""

    def __init__(self, aggregate, norm, in_feats, out_feats, relations, bases):
        super().__init__()
        self.aggregate, self.norm = aggregate, norm
        self.coef = torch.nn.Parameter(torch.randn(relations, bases) / bases ** 0.5)
        self.basis = torch.nn.Parameter(torch.randn(bases * in_feats, out_feats) / (bases * in_feats) ** 0.5)
        self.loop = torch.nn.Linear(in_feats, out_feats)

    def forward(self, h):
        agg = self.aggregate(h, self.coef, self.norm)                       # fp32 [n, B, F]
        return self.loop(h) + agg.flatten(1) @ self.basis


class RGCN(torch.nn.Module):
    def __init__(self, aggregate, norm, in_feats, hidden, classes, relations, bases):
        super().__init__()
        self.l1 = RGCNLayer(aggregate, norm, in_feats, hidden, relations, bases)
        self.l2 = RGCNLayer(aggregate, norm, hidden, classes, relations, bases)

    def forward(self, x):
        return self.l2(torch.relu(self.l1(x)))


def main():
    import synth_graphs
    import voltrix
    from voltrix.autograd import CsrPattern, SpMMRel

    workload = sys.argv[1] if len(sys.argv) > 1 else "dd_like"
    hidden = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    epochs = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    relations = int(sys.argv[4]) if len(sys.argv) > 4 else 46
    bases = int(sys.argv[5]) if len(sys.argv) > 5 else 8
    indptr, indices, _ = synth_graphs.generate(workload, device="cuda")
    n, nnz = indptr.numel() - 1, indices.numel()
    torch.manual_seed(0)
    etype = torch.randint(0, relations, (nnz,), device="cuda", dtype=torch.int32)       # a type per edge
    t0 = time.perf_counter()
    op = SpMMRel(CsrPattern(indptr, indices, n), etype=etype, num_types=relations)
    norm = voltrix.spmm_rel.type_norm(indptr, etype, relations)
    torch.cuda.synchronize()
    print(f"{workload}: N={n} nnz={nnz} R={relations} B={bases}; CSR, its transpose, the type index ({op.type_index.num_chunks} chunks) "
          f"and the normaliser built in {time.perf_counter() - t0:.2f} s")
    in_feats, classes = 64, 16
    x = torch.randn(n, in_feats, device="cuda")
    y = torch.randint(0, classes, (n,), device="cuda")
    model = RGCN(op, norm, in_feats, hidden, classes, relations, bases).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    times, losses = [], []
    for epoch in range(epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(model(x), y)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        losses.append(float(loss.detach()))
        print(f"epoch {epoch}: loss {losses[-1]:.4f}, {times[-1]:.2f} ms")
    assert losses[-1] < losses[0], "the loss did not fall"
    steady = sorted(times[2:])[len(times[2:]) // 2] if len(times) > 2 else times[-1]
    print(f"steady epoch (forward + backward + Adam, full graph): {steady:.2f} ms -- two relational aggregations of width {in_feats} / "
          f"{hidden} into {bases} bases per epoch, loss {losses[0]:.4f} -> {losses[-1]:.4f}")


if __name__ == "__main__":
    main()
