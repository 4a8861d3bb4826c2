"""A two-layer GAT (single-head by default, multi-head with the fourth argument) trained with the operators of this package (example;
no reference counterpart -- the reference is forward-only and has no edge values).

    Wh = X W,   s_ij = LeakyReLU(a_l . Wh_i + a_r . Wh_j),   alpha = edge softmax of s over every row,   H_i = sum_j alpha_ij Wh_j

(Velickovic et al.).  The per-node scalars a_l . Wh and a_r . Wh are torch matmuls; the scores are ``voltrix.autograd.GATScore`` (one
column id per edge, no row-id or int64 column-id tensor, and two segment sums instead of two atomic scatters in the backward); the softmax
over every row is ``voltrix.autograd.EdgeSoftmax`` (deterministic HIP kernels, forward and backward); the
aggregation is ``voltrix.autograd.SpMM(..., values=alpha)`` on fp16 ``Wh``, which returns ``alpha``'s gradient through the sampled
dense-dense product.  Self loops are added so that every node attends to itself.

With ``heads`` > 1 the hidden layer is H heads of ``hidden / H`` features, concatenated, and the output layer averages its H heads, as in
the paper; the scalars become [n, H], the softmax runs on [nnz, H] and the aggregation is ``voltrix.autograd.SpMMHeads`` (one launch
for all heads, no value planes).  ``heads`` = 1 is the single-head run, unchanged.

With a fifth argument ``v2`` the layers are GATv2 (Brody et al.): two linear maps, ``s_ij = a . LeakyReLU(W_l x_i + W_r x_j)`` per head
through ``voltrix.autograd.GATv2Score`` (nothing of size [nnz, H, D] exists, forward or backward), and the aggregation runs on ``W_r x``
through ``SpMMHeads`` (also with one head); score, softmax and aggregation share one transpose.  Without ``v2`` the run is unchanged.

With a trailing argument ``fused`` the multi-head and the ``v2`` layers replace ``softmax`` plus ``aggregate`` by
``voltrix.autograd.AttnAggregate``: one launch forward, the attention weights [nnz, H] are never stored and their gradient never exists.
Without ``fused`` every run is unchanged.

With a trailing token ``attn_drop=P`` the attention weights are dropped with probability ``P`` while training (GAT's own recipe uses
0.6) and left alone in evaluation.  The keep mask is one bit per edge and head (``voltrix.dropout_mask``, a fresh seed per layer and
step from torch's generator); with ``fused`` it goes into ``AttnAggregate`` (nothing of size [nnz, H] but the scores exists), without
it ``voltrix.apply_dropout_mask`` multiplies the stored ``alpha``.  Without the token every run is unchanged.

    python examples/gat_train.py [workload] [hidden] [epochs] [heads] [v2] [fused] [attn_drop=P]   # synthetic graph, random features and labels
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "voltrix-spmm_amd")]
os.environ.setdefault("VOLTRIX_CACHE_DIR", os.path.join(REPO, "voltrix-spmm_amd", ".jit_cache"))

import torch  # noqa: E402


def with_self_loops(indptr, indices, n):
    """CSR of A + I (self loops added where missing, duplicates removed, columns sorted), on ``indptr``'s device."""
    dev = indptr.device
    rows = torch.repeat_interleave(torch.arange(n, device=dev, dtype=torch.int64), (indptr[1:] - indptr[:-1]).long())
    key = torch.unique(torch.cat([rows * n + indices.long(), torch.arange(n, device=dev, dtype=torch.int64) * (n + 1)]))
    rows, cols = key // n, key % n
    new_indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    new_indptr[1:] = torch.bincount(rows, minlength=n).cumsum(0)
    return new_indptr.to(torch.int32), cols.to(torch.int32)


class Graph:
    """What both layers share: the edge scores, the edge softmax and the aggregation operator (built once: A and A^T).  ``heads`` > 1:
    the multi-head aggregation (no handle); every operator but the block-format ``SpMM`` shares one ``CsrPattern``.  ``rows`` / ``cols``
    (int64 row and column id of every edge) are built when something asks for them; the training run never does."""

    def __init__(self, indptr, indices, n, hash_tag="example_gat", heads=1, v2=False, fused=False, attn_drop=0.0):
        from voltrix.autograd import AttnAggregate, CsrPattern, EdgeSoftmax, GATScore, GATv2Score, SpMM, SpMMHeads

        assert not fused or v2 or heads > 1, "fused: the multi-head and the v2 layers"
        self.n, self.heads, self.v2, self.attn_drop = n, heads, v2, float(attn_drop)
        self._indptr, self._indices = indptr, indices
        self._rows = self._cols = None
        pattern = CsrPattern(indptr, indices, n)      # the device CSR and its transpose, once for every operator below
        self.softmax = EdgeSoftmax(pattern)
        self.score = GATv2Score(pattern) if v2 else GATScore(pattern)
        if v2 or heads > 1:     # GATv2: the multi-head aggregation for any number of heads
            self.aggregate = SpMMHeads(pattern)
        else:
            self.aggregate = SpMM(indptr, indices, n, values=torch.ones(indices.numel(), device="cuda"), hash_tag=hash_tag)
        self.fused = AttnAggregate(pattern) if fused else None      # softmax and aggregation in one operator

    def drop(self, alpha, training):
        """Attention dropout on stored weights ([nnz] or [nnz, H]): a packed keep mask, applied in torch."""
        if not training or self.attn_drop == 0.0:
            return alpha
        import voltrix

        seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        mask = voltrix.dropout_mask(alpha.shape[0], 1 if alpha.dim() == 1 else alpha.shape[1], self.attn_drop, seed, device=alpha.device)
        one, kept = torch.tensor(1.0), torch.tensor(1.0 - self.attn_drop)      # float32, the quotient AttnAggregate uses
        return voltrix.apply_dropout_mask(alpha, mask, float(one / kept))

    def attend(self, feat, s, training=False):
        """``aggregate(feat, softmax(s))``: scores [nnz, H], out [n, H, out_feats]; one operator with ``fused``.  ``training``: with
        attention dropout when the graph was built with ``attn_drop``."""
        if self.fused is not None:
            if training and self.attn_drop > 0.0:
                return self.fused(feat, s, dropout_p=self.attn_drop, training=True)
            return self.fused(feat, s)
        return self.aggregate(feat, self.drop(self.softmax(s), training))

    @property
    def rows(self):
        if self._rows is None:
            deg = (self._indptr[1:] - self._indptr[:-1]).long().cuda()
            self._rows = torch.repeat_interleave(torch.arange(self.n, device="cuda"), deg)
        return self._rows

    @property
    def cols(self):
        if self._cols is None:
            self._cols = self._indices.long().cuda()
        return self._cols


class GATLayer(torch.nn.Module):
    def __init__(self, graph, in_feats, out_feats, slope=0.2):
        super().__init__()
        self.graph, self.slope = graph, slope
        self.w = torch.nn.Linear(in_feats, out_feats, bias=False)
        self.a_l = torch.nn.Parameter(torch.randn(out_feats) / out_feats ** 0.5)
        self.a_r = torch.nn.Parameter(torch.randn(out_feats) / out_feats ** 0.5)

    def forward(self, x):
        g = self.graph
        wh = self.w(x)
        s = g.score(wh @ self.a_l, wh @ self.a_r, self.slope)
        alpha = g.drop(g.softmax(s), self.training)
        return g.aggregate(wh.half(), values=alpha)


class GATHeadsLayer(torch.nn.Module):
    """``graph.heads`` heads of ``out_feats`` features each: concatenated ([n, H * out_feats]) or averaged ([n, out_feats])."""

    def __init__(self, graph, in_feats, out_feats, concat, slope=0.2):
        super().__init__()
        self.graph, self.slope, self.concat, self.out_feats = graph, slope, concat, out_feats
        self.w = torch.nn.Linear(in_feats, graph.heads * out_feats, bias=False)
        self.a_l = torch.nn.Parameter(torch.randn(graph.heads, out_feats) / out_feats ** 0.5)
        self.a_r = torch.nn.Parameter(torch.randn(graph.heads, out_feats) / out_feats ** 0.5)

    def forward(self, x):
        g = self.graph
        wh = self.w(x).view(g.n, g.heads, self.out_feats)
        s = g.score((wh * self.a_l).sum(-1), (wh * self.a_r).sum(-1), self.slope)
        out = g.attend(wh.half(), s, self.training)           # scores, weights [nnz, H]; out [n, H, out_feats]
        return out.flatten(1) if self.concat else out.mean(1)


class GATv2HeadsLayer(torch.nn.Module):
    """GATv2: ``graph.heads`` heads of ``out_feats`` features each, two linear maps; concatenated or averaged like ``GATHeadsLayer``."""

    def __init__(self, graph, in_feats, out_feats, concat, slope=0.2):
        super().__init__()
        self.graph, self.slope, self.concat, self.out_feats = graph, slope, concat, out_feats
        self.wl = torch.nn.Linear(in_feats, graph.heads * out_feats, bias=False)
        self.wr = torch.nn.Linear(in_feats, graph.heads * out_feats, bias=False)
        self.a = torch.nn.Parameter(torch.randn(graph.heads, out_feats) / out_feats ** 0.5)

    def forward(self, x):
        g = self.graph
        xl = self.wl(x).view(g.n, g.heads, self.out_feats).half()
        xr = self.wr(x).view(g.n, g.heads, self.out_feats).half()
        s = g.score(xl, xr, self.a, self.slope)               # [nnz, H] from fp16 rows; the gradients come back in fp16
        out = g.attend(xr, s, self.training)                  # out [n, H, out_feats]
        return out.flatten(1) if self.concat else out.mean(1)


class GAT(torch.nn.Module):
    def __init__(self, graph, in_feats, hidden, classes):
        super().__init__()
        if graph.v2:
            assert hidden % graph.heads == 0, (hidden, graph.heads)
            self.l1 = GATv2HeadsLayer(graph, in_feats, hidden // graph.heads, concat=True)
            self.l2 = GATv2HeadsLayer(graph, hidden, classes, concat=False)
            return
        if graph.heads > 1:
            assert hidden % graph.heads == 0, (hidden, graph.heads)
            self.l1 = GATHeadsLayer(graph, in_feats, hidden // graph.heads, concat=True)
            self.l2 = GATHeadsLayer(graph, hidden, classes, concat=False)
            return
        self.l1 = GATLayer(graph, in_feats, hidden)
        self.l2 = GATLayer(graph, hidden, classes)

    def forward(self, x):
        return self.l2(torch.nn.functional.elu(self.l1(x)))


def main():
    import synth_graphs

    workload = sys.argv[1] if len(sys.argv) > 1 else "reddit_like"
    hidden = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    epochs = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    heads = int(sys.argv[4]) if len(sys.argv) > 4 else 1
    flags = sys.argv[5:]
    attn_drop = 0.0
    if flags and flags[-1].startswith("attn_drop="):
        attn_drop = float(flags.pop()[len("attn_drop="):])
        assert 0.0 <= attn_drop < 1.0, attn_drop
    assert flags in ([], ["v2"], ["fused"], ["v2", "fused"]), flags
    v2, fused = "v2" in flags, "fused" in flags
    indptr, indices, _ = synth_graphs.generate(workload, device="cuda")
    n = indptr.numel() - 1
    indptr, indices = with_self_loops(indptr, indices, n)
    t0 = time.perf_counter()
    graph = Graph(indptr, indices, n, hash_tag=f"example_gat/{workload}", heads=heads, v2=v2, fused=fused, attn_drop=attn_drop)
    torch.cuda.synchronize()
    print(f"{workload}: N={n} nnz={indices.numel()} (self loops added); operators built in {time.perf_counter() - t0:.2f} s")
    torch.manual_seed(0)
    in_feats, classes = 128, 48          # widths a multiple of 8: the fp16 rows stay 16-byte aligned without padding
    x = torch.randn(n, in_feats, device="cuda")
    y = torch.randint(0, classes, (n,), device="cuda")
    model = GAT(graph, in_feats, hidden, classes).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    times = []
    model.train()
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
    print(f"steady epoch (forward + backward + Adam, full graph): {steady:.2f} ms -- two attention layers, hidden {hidden}"
          + (f", {heads} heads" if heads > 1 else "") + (", GATv2" if v2 else "") + (", fused" if fused else "") + (f", attn_drop {attn_drop}" if attn_drop else "") + f"; peak memory {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB")
    if attn_drop:
        model.eval()                         # evaluation: no dropout, the same operators
        with torch.no_grad():
            print(f"evaluation loss (attention dropout off): {float(torch.nn.functional.cross_entropy(model(x), y)):.4f}")


if __name__ == "__main__":
    main()
