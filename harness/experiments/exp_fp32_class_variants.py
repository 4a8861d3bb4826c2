"""fp32 features on handles that keep a CSR side-car: what pinning the rounding class costs.  Per graph and width, in one process:

    block     the block-format path of the handle's class (exact fp32 tiles, or the scaled fp16 cast in front of the 16-bit kernels)
    csr       the CSR row-gather kernel on the fp32 rows as they are (exact whatever the class)
    variant A class "fp16" only: the CSR kernel as a candidate ON THE CAST OPERAND -- the scaled cast, the CSR kernel on the fp16 rows,
              and a pass over C for the scale (the CSR kernel has no scale argument; ``scale_rows`` with a constant vector stands in)

and what each rule would run: ``before`` = the faster of csr / block by 3 % whatever the class (a timed choice that changes the
rounding), ``A`` = variant A against block by 3 %, ``B`` = block alone in class "fp16" (the CSR kernel is no candidate there).
python exp_fp32_class_variants.py [F ...]"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, "voltrix-spmm_amd")]
os.environ.setdefault("VOLTRIX_CACHE_DIR", os.path.join(REPO, "voltrix-spmm_amd", ".jit_cache"))

import torch  # noqa: E402

import synth_graphs  # noqa: E402
import voltrix  # noqa: E402
from voltrix import capi, sidecar  # noqa: E402

operator = sys.modules["voltrix.spmm.spmm"]
GAIN = 1.0 - operator.CSR_MIN_GAIN


def ms(fn):
    for _ in range(3):
        fn()
    t = []
    for _ in range(5):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(5):
            fn()
        e.record()
        e.synchronize()
        t.append(s.elapsed_time(e) / 5)
    return sorted(t)[2]


widths = [int(a) for a in sys.argv[1:]] or [128, 512]
print("graph F class | block csr variant-A | before A B | B / before, A / before")
worst = {"A": 1.0, "B": 1.0}
for graph in synth_graphs.EVALUATION_SET.values():
    indptr, indices, _ = synth_graphs.generate(graph, device="cuda")
    n, e = indptr.numel() - 1, indices.numel()
    handle = voltrix.csr_preprocess_device(indptr, indices, n)
    handle[1].hash_tag = f"exp_fp32_class_variants/{graph}"
    csr = sidecar.lookup_csr(handle[1])
    if csr is None:
        print(f"{graph}: no CSR side-car", flush=True)
        continue
    gen = torch.Generator(device="cuda").manual_seed(5)
    stream = torch.cuda.current_stream().cuda_stream
    for width in widths:
        feat = torch.randn(n, width, device="cuda", generator=gen)
        klass = operator.fp32_mode(handle[1], n, width)
        os.environ["VOLTRIX_CSR_PATH"] = "0"
        block = ms(lambda: voltrix.spmm(*handle, num_nodes=n, num_edges=e, feat=feat))
        os.environ["VOLTRIX_CSR_PATH"] = "1"
        exact = ms(lambda: voltrix.spmm(*handle, num_nodes=n, num_edges=e, feat=feat))
        os.environ.pop("VOLTRIX_CSR_PATH")
        variant_a = None
        if klass == "fp16":
            ones = torch.ones(n, device="cuda")

            def cast_csr_scale():
                operand, out_scale, padded, _ = operator._operand(feat, "fp16")
                out = torch.empty(n, padded, device="cuda")
                capi.launch_spmm_csr_rows(csr.indptr, csr.indices, n, operand, out, stream, 1)
                capi.launch_scale_rows(out, ones, out, stream)
                return out

            variant_a = ms(cast_csr_scale)
        before = exact if exact < GAIN * block else block
        rule_b = block if klass == "fp16" else before
        rule_a = (variant_a if variant_a < GAIN * block else block) if klass == "fp16" else before
        worst["A"], worst["B"] = max(worst["A"], rule_a / before), max(worst["B"], rule_b / before)
        print(f"{graph} {width} {klass} | {block:.4f} {exact:.4f} {'-' if variant_a is None else f'{variant_a:.4f}'} | {before:.4f} "
              f"{rule_a:.4f} {rule_b:.4f} | {rule_b / before:.3f} {rule_a / before:.3f}", flush=True)
    del handle, csr, indptr, indices
    torch.cuda.empty_cache()
print(f"worst slowdown against the rule before: variant A {worst['A']:.3f}, variant B {worst['B']:.3f}")
