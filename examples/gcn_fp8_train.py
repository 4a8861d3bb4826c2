"""The two-layer GCN of examples/gcn_train.py with FP8 aggregation: `voltrix.autograd.SpMMFp8` in place of the aggregation.

    H1 = relu(Â X W1),  Y = Â H1 W2,  Â = D^-1/2 (A + I) D^-1/2   (Kipf & Welling)

Every aggregation quantises its input to e4m3 rows with one scale per feature column (re-quantised every layer and epoch: the
activations change), gathers half the bytes of the fp16 path, and passes the gradient straight through the quantiser: the backward is
the exact fp32 row-gather sum on the transposed pattern with Â's values.  Both variants -- fp8 and the existing fp16 path of
gcn_train.py (`voltrix.autograd.SpMM(..., values=)`) -- start from the same seeds and weights; the loss of both is printed per epoch.

    python examples/gcn_fp8_train.py [workload] [hidden] [epochs]      # synthetic stand-in graph, random features and labels
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "voltrix-spmm_amd"), os.path.join(REPO, "examples")]
os.environ.setdefault("VOLTRIX_CACHE_DIR", os.path.join(REPO, "voltrix-spmm_amd", ".jit_cache"))

import torch  # noqa: E402

from gcn_train import GCN, normalised_adjacency  # noqa: E402


def train(name, aggregate, dtype, x, y, hidden, classes, epochs):
    torch.manual_seed(0)                                  # the same weights for both variants
    model = GCN(aggregate, x.shape[1], hidden, classes, dtype=dtype).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    losses, times = [], []
    for _ in range(epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(model(x).float(), y)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        losses.append(float(loss.detach()))
    steady = sorted(times[2:])[len(times[2:]) // 2] if len(times) > 2 else times[-1]
    print(f"{name}: steady epoch (forward + backward + Adam, full graph) {steady:.2f} ms")
    return losses


def main():
    import synth_graphs
    from voltrix.autograd import CsrPattern, SpMM, SpMMFp8

    workload = sys.argv[1] if len(sys.argv) > 1 else "dd_like"
    hidden = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    epochs = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    indptr, indices, _ = synth_graphs.generate(workload, device="cuda")
    n = indptr.numel() - 1
    indptr, indices, values = normalised_adjacency(indptr, indices, n)
    print(f"{workload}: N={n} nnz={indices.numel()} (self loops added), hidden {hidden}, {epochs} epochs")
    torch.manual_seed(0)
    in_feats, classes = 128, 48
    x = torch.randn(n, in_feats, device="cuda")
    y = torch.randint(0, classes, (n,), device="cuda")
    fp8 = SpMMFp8(CsrPattern(indptr, indices, n))
    fp16 = SpMM(indptr, indices, n, values=values, hash_tag=f"example_gcn/{workload}")
    # fp8: the operator reads the linear layer's fp32 output as it is (no cast to fp16 in between); fp16: gcn_train.py's path
    loss8 = train("fp8 ", lambda h: fp8(h, values=values, scale="column"), torch.float32, x, y, hidden, classes, epochs)
    loss16 = train("fp16", fp16, torch.float16, x, y, hidden, classes, epochs)
    for epoch, (a, b) in enumerate(zip(loss8, loss16)):
        print(f"epoch {epoch:2d}: loss fp8 {a:.4f}   fp16 {b:.4f}   difference {a - b:+.4f}")


if __name__ == "__main__":
    main()
