#!/usr/bin/env python3
"""Time one relational (R-GCN) layer, forward + backward including the dense ``V`` product, three ways, on synth_graphs stand-ins whose
edge types are drawn uniformly per edge:

  * ``rel``: aggregate first -- ``voltrix.autograd.SpMMRel`` ([n, B, F], one launch), then ``agg.view(n, B F) @ V``; backward through
    autograd (``grad_feat``, ``grad_coef``, the two dense products);
  * ``messages``: the per-edge-message torch composite -- ``zeros.index_add_(0, rows, (norm coef[etype])[:, :, None] * h[cols][:, None,
    :])`` ([nnz, B, F] materialised, float atomics), then the same dense product, and its backward written out the way autograd runs
    it.  Forward and backward walk the entries in chunks of at most ``--message-bytes`` of messages: one chunk where they fit;
  * ``transform``: transform first on the existing kernels -- ``W_r = sum_b coef[r, b] V_b``, ``H = h W_r`` for every relation
    ([R n, F_out]), then the CSR row-gather kernel (``voltrix_launch_spmm_csr_rows_weighted``) with columns ``etype n + col``; backward: the
    same kernel on the transposed pattern, then autograd through the dense products.

Per graph, ``(R, B)`` (``B = 0``: ``coef = I_R``, the plain per-relation sums), width ``F = F_out`` and dtype of ``h``, over warmed
steps bracketed by device events, in one process on one GPU.  One JSON line per point: milliseconds forward + backward and peak device
memory (allocator high-water mark over the timed steps, operands included) for each form, the ratios, and ``spmm_rel``, ``grad_feat``
and ``grad_coef`` timed alone (``rel_fwd_ms``, ``rel_grad_feat_ms``, ``rel_grad_coef_ms``).  The forms' outputs and gradients are
compared with each other at every point."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "voltrix-spmm_amd")):
    sys.path.insert(0, p)
os.environ.setdefault("VOLTRIX_CACHE_DIR", os.path.join(REPO, "voltrix-spmm_amd", ".jit_cache"))

import torch  # noqa: E402

import synth_graphs  # noqa: E402
import voltrix  # noqa: E402
from voltrix import capi  # noqa: E402
from voltrix.autograd import CsrPattern, SpMMRel  # noqa: E402
from voltrix.spmm_rel import grad_coef, grad_feat  # noqa: E402

DEFAULT_CASES = ("amazon0601_like", "reddit_like")
DEFAULT_SHAPES = ("4x0", "46x8", "46x30")          # R x B; B = 0: the identity
DTYPES = {"fp16": torch.float16, "fp32": torch.float32}


def _measure(fn, steps, warmup):
    """(milliseconds per step, peak bytes) of ``fn`` over ``steps`` steps after ``warmup``."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / steps, torch.cuda.max_memory_allocated()


def rel_step(op, h, coef, norm, basis, grad):
    def step():
        hh = h.detach().requires_grad_(True)
        cc = None if coef is None else coef.detach().requires_grad_(True)
        vv = basis.detach().requires_grad_(True)
        out = op(hh, cc, norm).flatten(1) @ vv
        out.backward(grad)
        return out, hh.grad, None if cc is None else cc.grad, vv.grad

    return step


def messages_step(rows, cols, etype, h, coef, norm, basis, grad, n, message_bytes):
    """The composite and its backward as autograd runs them, over chunks of entries whose [chunk, B, F] fp32 messages stay below
    ``message_bytes``."""
    nnz, dim = cols.numel(), h.shape[1]
    table = torch.eye(int(etype.max()) + 1, device=h.device) if coef is None else coef
    bases = table.shape[1]
    chunk = max(1, min(nnz, message_bytes // (4 * bases * dim)))
    etype = etype.long()

    def step():
        x = h.float()
        agg = torch.zeros(n, bases, dim, device=h.device)
        for lo in range(0, nnz, chunk):
            s = slice(lo, lo + chunk)
            c = norm[s, None] * table[etype[s]]
            agg.index_add_(0, rows[s], c[:, :, None] * x[cols[s]][:, None, :])
        out = agg.flatten(1) @ basis
        d_basis = agg.flatten(1).t() @ grad
        g = (grad @ basis.t()).view(n, bases, dim)
        d_h, d_coef = torch.zeros_like(x), torch.zeros_like(table)
        for lo in range(0, nnz, chunk):
            s = slice(lo, lo + chunk)
            gm = g[rows[s]]
            c = norm[s, None] * table[etype[s]]
            d_h.index_add_(0, cols[s], (c[:, :, None] * gm).sum(1))
            if coef is not None:
                d_coef.index_add_(0, etype[s], norm[s, None] * (gm * x[cols[s]][:, None, :]).sum(2))
        return out, d_h.to(h.dtype), d_coef, d_basis

    return step, chunk


def transform_step(indptr, big, etype, h, coef, norm, basis, grad, n, relations):
    """``big``: CsrPattern of [n, R n] with columns ``etype n + col``."""
    dim, f_out = h.shape[1], basis.shape[1]
    stream = torch.cuda.current_stream().cuda_stream
    norm_t = norm[big.t_order.long()].contiguous()

    def step():
        hh = h.detach().requires_grad_(True)
        cc = None if coef is None else coef.detach().requires_grad_(True)
        vv = basis.detach().requires_grad_(True)
        if cc is None:
            w = vv.view(relations, dim, f_out)
        else:
            w = (cc @ vv.view(cc.shape[1], dim * f_out)).view(relations, dim, f_out)
        transformed = torch.einsum("nf,rfo->rno", hh.float(), w).reshape(relations * n, f_out)
        out = torch.empty(n, f_out, device=h.device)
        capi.launch_spmm_csr_rows(big.indptr, big.indices, n, transformed.detach(), out, stream, 1, norm)
        d_transformed = torch.empty(relations * n, f_out, device=h.device)
        capi.launch_spmm_csr_rows(big.t_indptr, big.t_indices, relations * n, grad, d_transformed, stream, 1, norm_t)
        transformed.backward(d_transformed)
        return out, hh.grad, None if cc is None else cc.grad, vv.grad

    return step


def run_graph(name, shapes, widths, dtypes, steps, warmup, torch_steps, torch_warmup, scale, message_bytes, forms):
    indptr, indices, _ = synth_graphs.generate(name, device="cuda", scale=scale)
    n, nnz = indptr.numel() - 1, indices.numel()
    pattern = CsrPattern(indptr, indices, n)
    deg = indptr[1:] - indptr[:-1]
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), deg.long())
    cols = indices.long()
    for shape in shapes:
        relations, bases = (int(v) for v in shape.split("x"))
        torch.manual_seed(0)
        etype = torch.randint(0, relations, (nnz,), device="cuda", dtype=torch.int32)
        op = SpMMRel(pattern, etype=etype, num_types=relations)
        norm = voltrix.spmm_rel.type_norm(indptr, etype, relations)
        big = None
        if "transform" in forms:
            big = CsrPattern(indptr, (etype.long() * n + cols).to(torch.int32), n, relations * n)
        for dim in widths:
            for dtype_name in dtypes:
                torch.manual_seed(1)
                h = torch.randn(n, dim, device="cuda").to(DTYPES[dtype_name])
                coef = None if bases == 0 else torch.randn(relations, bases, device="cuda") / bases ** 0.5
                width = relations if bases == 0 else bases
                basis = torch.randn(width * dim, dim, device="cuda") / (width * dim) ** 0.5
                grad = torch.randn(n, dim, device="cuda")
                line = {"graph": name, "scale": scale, "R": relations, "B": bases, "F": dim, "dtype": dtype_name, "num_rows": n,
                        "nnz": nnz, "max_deg": int(deg.max()), "steps": steps, "torch_steps": torch_steps}
                runs = {"rel": (rel_step(op, h, coef, norm, basis, grad), steps, warmup)}
                if "messages" in forms:
                    step, chunk = messages_step(rows, cols, etype, h, coef, norm, basis, grad, n, message_bytes)
                    runs["messages"] = (step, torch_steps, torch_warmup)
                    line["message_chunks"] = -(-nnz // chunk)
                if "transform" in forms:
                    runs["transform"] = (transform_step(indptr, big, etype, h, coef, norm, basis, grad, n, relations), steps, warmup)
                results = {}
                for form, (step, k, w) in runs.items():
                    try:
                        results[form] = step()
                        line[f"{form}_ms"], peak = _measure(step, k, w)
                        line[f"{form}_ms"], line[f"{form}_peak_GiB"] = round(line[f"{form}_ms"], 4), round(peak / 2 ** 30, 3)
                    except torch.cuda.OutOfMemoryError:       # recorded, not hidden
                        line[f"{form}_ms"] = line[f"{form}_peak_GiB"] = None
                        results.pop(form, None)
                        torch.cuda.empty_cache()
                # the three forms compute the same layer: outputs and gradients agree to fp32 rounding of sums this long
                want = results["rel"]
                for form, got in results.items():
                    for a, b in zip(got, want):
                        if a is not None and b is not None:
                            a, b = a.detach().double(), b.detach().double()
                            worst = float(((a - b).abs() / b.abs().clamp_min(1.0)).max())
                            assert worst < 2e-2, (form, worst)
                # where rel's time goes: its three operators alone (the rest is the dense products and autograd's bookkeeping)
                g3 = torch.randn(n, width, dim, device="cuda")
                t = (pattern.t_indptr, pattern.t_indices, pattern.t_order)
                table = relations if coef is None else coef
                line["rel_fwd_ms"] = round(_measure(lambda: voltrix.spmm_rel(indptr, indices, etype, h, table, n, norm), steps, warmup)[0], 4)
                line["rel_grad_feat_ms"] = round(_measure(lambda: grad_feat(*t, etype, g3, table, n, norm), steps, warmup)[0], 4)
                if coef is not None:
                    line["rel_grad_coef_ms"] = round(_measure(lambda: grad_coef(indptr, indices, etype, op.type_index, g3, h, norm), steps,
                                                              warmup)[0], 4)
                del g3
                for form in ("messages", "transform"):
                    if line.get(f"{form}_ms"):
                        line[f"{form}_over_rel"] = round(line[f"{form}_ms"] / line["rel_ms"], 3)
                print(json.dumps(line), flush=True)
                del results, want, h, basis, grad
                torch.cuda.empty_cache()
        del op, big
        torch.cuda.empty_cache()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", nargs="*", default=list(DEFAULT_CASES), help="synth_graphs stand-in names")
    ap.add_argument("--shapes", nargs="*", default=list(DEFAULT_SHAPES), help="RxB; B = 0: coef = I_R")
    ap.add_argument("--widths", nargs="*", type=int, default=[32, 128])
    ap.add_argument("--dtypes", nargs="*", default=["fp16", "fp32"], choices=sorted(DTYPES))
    ap.add_argument("--forms", nargs="*", default=["messages", "transform"], choices=["messages", "transform"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-steps", type=int, default=3, help="timed steps of the message composite")
    ap.add_argument("--torch-warmup", type=int, default=1)
    ap.add_argument("--message-bytes", type=int, default=8 << 30, help="bound on one chunk's [chunk, B, F] fp32 messages")
    ap.add_argument("--scale", type=float, default=1.0, help="synth_graphs scale of every stand-in")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_spmm_rel.py needs a GPU"
    for name in args.cases:
        run_graph(name, args.shapes, args.widths, args.dtypes, args.steps, args.warmup, args.torch_steps, args.torch_warmup, args.scale,
                  args.message_bytes, args.forms)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
