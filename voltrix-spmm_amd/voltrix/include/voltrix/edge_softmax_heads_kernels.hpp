// Voltrix-SpMM for MI355X (gfx950) -- multi-head edge softmax on a CSR pattern and its backward: the contract of
// edge_softmax_kernels.hpp applied to every column of scores[nnz, H] (head index fastest) independently.
//
// Shape.  The three launches of the single-head kernels with the head as a grid dimension and element e of head h at e H + h:
//   K1  one workgroup per (chunk of kChunkEdges edges, head).  The workgroups of one chunk are 8 apart in blockIdx.x (chunk
//       c = b % 8 + 8 (b / (8 H)), head h = (b / 8) % H), so its H heads run on one XCD at about the same time and the lines of
//       scores[chunk, :] -- every head uses 4 bytes of each 4 H -- come from HBM once and from that XCD's L2 afterwards.
//   K2  one wave per (chunk, head): grid.y = H.
//   K3  one workgroup per (chunk, head): grid.y = H.
// The rows of a chunk (rows[c]) do not depend on the head: head 0 writes them in K1.  Every head has its own partials and merged
// partials.  The in-thread reduction, the scan, the merge tree and the exponent arithmetic are the single-head ones (the Ops derive from
// SoftmaxOp / SoftmaxBackwardOp and replace only the element access), so out[:, h] has the BITS of the single-head kernels on the
// contiguous column scores[:, h] -- special values included: a NaN or a row of -inf stays in its own row AND its own head.
//
// Why a grid dimension and not H-vectors through the scan: the scan state of the forward is (m, s) per head; H = 8 would carry 16
// floats per thread per edge slot through the shuffles and the LDS (4 x the LDS of today for the two partial arrays) and cut the
// occupancy that hides the dependent indptr loads, and H is a run-time number.  The price is strided element access.
//
// No float atomics, no host synchronisation, the same bits on every launch; workspace a function of (nnz, H) alone.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "voltrix/edge_softmax_kernels.hpp"

namespace voltrix {

struct EdgeSoftmaxHeadsArgs {
  EdgeSoftmaxArgs base;  // in0 / in1 / out: [nnz, H]; parts: [H][2 * chunks]; merged: [H][chunks]; rows: [chunks]
  int heads;
};

// workspace: rows (8 B per chunk, padded to 16) + per head two partials (16 B) + merged (8 B) per chunk; heads = 1: the single-head size
inline long long edge_softmax_heads_workspace_bytes(long long nnz, int heads) {
  const long long c = edge_softmax_chunks(nnz);
  return c * 8 + (c & 1) * 8 + (long long)heads * (c * 16 + c * 8);
}

// element e of this head sits at e * H from the head's base pointers
struct SoftmaxHeadsOp : SoftmaxOp {
  long long H;
  __device__ Elem load(int e) const { return Elem{a.sign * a.in0[e * H]}; }
  __device__ void store(int e, float v) const { a.out[e * H] = v; }
};

struct SoftmaxBackwardHeadsOp : SoftmaxBackwardOp {
  long long H;
  __device__ Elem load(int e) const { return Elem{a.in0[e * H], a.in1[e * H]}; }
  __device__ void store(int e, float v) const { a.out[e * H] = v; }
};

// the single-head arguments of head h
__device__ __forceinline__ EdgeSoftmaxArgs es_head_args(const EdgeSoftmaxHeadsArgs& ha, int h) {
  EdgeSoftmaxArgs args = ha.base;
  args.in0 += h;
  args.in1 += h;
  args.out += h;
  args.parts += 2ll * h * args.chunks;
  args.merged += (long long)h * args.chunks;
  return args;
}

// K1: one (chunk, head) per workgroup.  Rows wholly inside the chunk are written; the chunk's first / last row partials go to the
// head's workspace.  edge_softmax_chunk_kernel with strided element access.
template <class Op>
static __global__ __launch_bounds__(kEdgeSoftmaxThreads) void edge_softmax_heads_chunk_kernel(const EdgeSoftmaxHeadsArgs ha) {
  using Part = typename Op::Part;
  constexpr int K = kEdgesPerThread;
  const int c = (int)(blockIdx.x % kNumXcd + kNumXcd * (blockIdx.x / (kNumXcd * ha.heads)));
  const int head = (int)(blockIdx.x / kNumXcd) % ha.heads;
  if (c >= ha.base.chunks) return;               // the whole workgroup leaves together
  const EdgeSoftmaxArgs args = es_head_args(ha, head);
  const Op op{{args}, (long long)ha.heads};
  __shared__ Part s_incl[kEdgeSoftmaxThreads];   // the scan's inclusive value (thread's last row)
  __shared__ Part s_head[kEdgeSoftmaxThreads];   // in-chunk partial of the thread's first row, through the thread's edges
  __shared__ Part s_wave[4];
  __shared__ int s_wave_flag[4];

  const int t = (int)threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const long long cb = (long long)c * kChunkEdges;
  const int chunk_begin = (int)cb;
  const int chunk_end = (int)(cb + kChunkEdges < args.nnz ? cb + kChunkEdges : args.nnz);
  const long long tb_l = cb + (long long)K * t;
  const int nk = tb_l >= chunk_end ? 0 : (chunk_end - tb_l < K ? (int)(chunk_end - tb_l) : K);
  const int tb = nk > 0 ? (int)tb_l : chunk_end;

  // the rows holding chunk_begin and chunk_end - 1: a 256-ary search by the whole workgroup
  int lo0 = 0, hi0 = args.num_rows, lo1 = 0, hi1 = args.num_rows;
  while (hi0 - lo0 > 1 || hi1 - lo1 > 1) {
    const long long len0 = hi0 - lo0, len1 = hi1 - lo1;
    const int c0 = __syncthreads_count(args.indptr[lo0 + (int)(len0 * t / kEdgeSoftmaxThreads)] <= chunk_begin);
    const int c1 = __syncthreads_count(args.indptr[lo1 + (int)(len1 * t / kEdgeSoftmaxThreads)] <= chunk_end - 1);
    if (c0 < kEdgeSoftmaxThreads) hi0 = lo0 + (int)(len0 * c0 / kEdgeSoftmaxThreads);   // samples are monotone: c >= 1 hold
    lo0 += (int)(len0 * (c0 - 1) / kEdgeSoftmaxThreads);
    if (c1 < kEdgeSoftmaxThreads) hi1 = lo1 + (int)(len1 * c1 / kEdgeSoftmaxThreads);
    lo1 += (int)(len1 * (c1 - 1) / kEdgeSoftmaxThreads);
  }
  const int r_first = lo0, r_last = lo1;

  typename Op::Elem el[K];
  int row[K], rs[K], re[K];
#pragma unroll
  for (int j = 0; j < K; ++j) el[j] = op.load(j < nk ? tb + j : (nk > 0 ? tb : 0));
  {
    int r = nk > 0 ? es_row_of(args.indptr, r_first, r_last + 1, tb) : r_last;
    int start = args.indptr[r], end = args.indptr[r + 1];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      if (j < nk && tb + j >= end) {        // the next row; past a run of empty rows a binary search, not a walk
        ++r;
        start = end;
        end = args.indptr[r + 1];
        if (tb + j >= end) {
          r = es_row_of(args.indptr, r, r_last + 1, tb + j);
          start = args.indptr[r];
          end = args.indptr[r + 1];
        }
      }
      row[j] = j < nk ? r : INT_MAX - K + j;   // distinct past the thread's edges: no segment continues into them
      rs[j] = start;
      re[j] = end;
    }
  }

  Part p[K];
  float tt[K];
  op.reduce(el, row, nk, p, tt);
  Part head_part = op.identity(), tail = op.identity();
  int tail_rs = tb, head_rs = tb;
  if (nk > 0) {
    head_part = p[0];
    head_rs = rs[0];
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {   // a chain of selects (a test of j == nk - 1 becomes an indexed load from scratch)
    tail.m = j < nk ? p[j].m : tail.m;
    tail.s = j < nk ? p[j].s : tail.s;
    tail_rs = j < nk ? rs[j] : tail_rs;
  }

  // segmented inclusive scan of (flag = the thread's last row starts in the thread, its partial) over the workgroup, in thread order
  Part v = tail;
  int f = nk == 0 || tail_rs >= tb;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    Part pv = v;
    int pf = f;
    es_shfl_up<Op>(pv, pf, d);
    if (lane >= d) {
      if (!f) v = op.merge(pv, v);
      f |= pf;
    }
  }
  if (lane == 63) {
    s_wave[wave] = v;
    s_wave_flag[wave] = f;
  }
  __syncthreads();
  if (!f) {
    for (int w = wave - 1; w >= 0; --w) {   // the preceding waves' totals, nearest first, until one holds a segment start
      v = op.merge(s_wave[w], v);
      if (s_wave_flag[w]) break;
    }
  }
  s_incl[t] = v;
  __syncthreads();
  Part h = head_part;
  if (t > 0 && nk > 0 && head_rs < tb) h = op.merge(s_incl[t - 1], head_part);
  s_head[t] = h;
  __syncthreads();

  // every row's in-chunk partial sits with the thread holding its last in-chunk edge; rows inside the chunk are finished here
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if (j >= nk) continue;
    const int last = (re[j] < chunk_end ? re[j] : chunk_end) - 1;
    const int t_last = (last - chunk_begin) / K;
    Part full;                              // selected by value: a select of addresses would put p[] in scratch
    if (t_last != t) {
      full = s_head[t_last];
    } else {
      const bool first = row[j] == row[0];
      full.m = first ? h.m : p[j].m;
      full.s = first ? h.s : p[j].s;
    }
    if (tb + j == last) {
      if (row[j] == r_first) args.parts[2 * c] = full;
      if (row[j] == r_last) args.parts[2 * c + 1] = full;
    }
    if (rs[j] < chunk_begin || re[j] > chunk_end) continue;   // crosses a chunk boundary: K3
    op.store(tb + j, op.finish(el[j], tt[j], p[j], full));
  }
  if (t == 0 && head == 0) args.rows[c] = int2{r_first, r_last};
}

// K2: one wave per (chunk, head = blockIdx.y); edge_softmax_merge_kernel on the head's partials
template <class Op>
static __global__ __launch_bounds__(kEdgeSoftmaxThreads) void edge_softmax_heads_merge_kernel(const EdgeSoftmaxHeadsArgs ha) {
  using Part = typename Op::Part;
  const EdgeSoftmaxArgs args = es_head_args(ha, (int)blockIdx.y);
  const Op op{{args}, (long long)ha.heads};
  const long long c_l = (long long)blockIdx.x * (kEdgeSoftmaxThreads / 64) + (threadIdx.x >> 6);
  if (c_l >= args.chunks) return;
  const int c = (int)c_l;
  const int lane = (int)threadIdx.x & 63;
  const int r = args.rows[c].y;
  const long long cb = (long long)c * kChunkEdges;
  const int rs = args.indptr[r], re = args.indptr[r + 1];
  if (rs < cb || re <= cb + kChunkEdges) return;       // not the owner of a crossing row (the whole wave leaves together)
  const int c_last = (int)((re - 1) / kChunkEdges);
  Part v = op.identity();
  for (int j = c + lane; j <= c_last; j += 64) v = op.merge(v, args.parts[j == c ? 2 * j + 1 : 2 * j]);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    Part o;
    o.m = __shfl_xor(v.m, m, 64);
    o.s = __shfl_xor(v.s, m, 64);
    v = (lane & m) ? op.merge(o, v) : op.merge(v, o);   // lower lanes' partial on the left
  }
  if (lane == 0) args.merged[c] = v;
}

// K3: one workgroup per (chunk, head = blockIdx.y): the chunk's first / last row segments that cross a chunk boundary
template <class Op>
static __global__ __launch_bounds__(kEdgeSoftmaxThreads) void edge_softmax_heads_boundary_kernel(const EdgeSoftmaxHeadsArgs ha) {
  using Part = typename Op::Part;
  const EdgeSoftmaxArgs args = es_head_args(ha, (int)blockIdx.y);
  const Op op{{args}, (long long)ha.heads};
  const int c = (int)blockIdx.x;
  const long long cb = (long long)c * kChunkEdges;
  const int chunk_begin = (int)cb;
  const int chunk_end = (int)(cb + kChunkEdges < args.nnz ? cb + kChunkEdges : args.nnz);
  const int2 rr = args.rows[c];
  const int rs0 = args.indptr[rr.x], re0 = args.indptr[rr.x + 1];
  if (rs0 < chunk_begin || re0 > chunk_end) {
    const Part full = args.merged[rs0 / kChunkEdges];
    const int end = re0 < chunk_end ? re0 : chunk_end;
    for (int i = (int)threadIdx.x; i < end - chunk_begin; i += kEdgeSoftmaxThreads)   // counted: e + 256 may pass INT_MAX
      op.store(chunk_begin + i, op.finish(op.load(chunk_begin + i), full));
  }
  if (rr.y != rr.x) {
    const int rs1 = args.indptr[rr.y], re1 = args.indptr[rr.y + 1];
    if (re1 > chunk_end) {
      const Part full = args.merged[c];
      for (int i = (int)threadIdx.x; i < chunk_end - rs1; i += kEdgeSoftmaxThreads) op.store(rs1 + i, op.finish(op.load(rs1 + i), full));
    }
  }
}

template <class Op>
inline int launch_edge_softmax_heads_passes(const EdgeSoftmaxHeadsArgs& a, hipStream_t stream) {
  const dim3 block(kEdgeSoftmaxThreads);
  const long long chunks8 = ((long long)a.base.chunks + kNumXcd - 1) / kNumXcd * kNumXcd;
  hipLaunchKernelGGL((edge_softmax_heads_chunk_kernel<Op>), dim3((unsigned)(chunks8 * a.heads)), block, 0, stream, a);
  if (a.base.chunks > 1) {
    hipLaunchKernelGGL((edge_softmax_heads_merge_kernel<Op>), dim3((unsigned)((a.base.chunks + 3) / 4), (unsigned)a.heads), block, 0,
                       stream, a);
    hipLaunchKernelGGL((edge_softmax_heads_boundary_kernel<Op>), dim3((unsigned)a.base.chunks, (unsigned)a.heads), block, 0, stream, a);
  }
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// Shared checks and workspace carving: edge_softmax_args on [nnz, heads] tensors.
inline int edge_softmax_heads_args(const int* indptr, int num_rows, long long nnz, int heads, const float* in0, const float* in1,
                                   float scale, float* out, void* workspace, EdgeSoftmaxHeadsArgs* args) {
  if (heads < 1 || heads > 65535) return kErrBadShape;
  const int rc = edge_softmax_args(indptr, num_rows, nnz, in0, in1, scale, out, workspace, &args->base);
  if (rc != kOk || args->base.chunks == 0) return rc;
  const long long chunks = args->base.chunks;
  if ((chunks + kNumXcd) * heads > 0x7fffffffLL) return kErrBadShape;
  args->base.merged = reinterpret_cast<SoftmaxPart*>(reinterpret_cast<char*>(args->base.parts) + (long long)heads * chunks * 16);
  args->heads = heads;
  return kOk;
}

// alpha[:, h] = edge softmax of scale * scores[:, h] over every row of a device CSR, for every head; scores and out [nnz, heads];
// workspace: edge_softmax_heads_workspace_bytes(nnz, heads) bytes, 16-byte aligned.
inline int launch_edge_softmax_heads_csr(const int* indptr, int num_rows, long long nnz, int heads, const float* scores, float scale,
                                         float* out, void* workspace, hipStream_t stream) {
  EdgeSoftmaxHeadsArgs a{};
  const int rc = edge_softmax_heads_args(indptr, num_rows, nnz, heads, scores, scores, scale, out, workspace, &a);
  if (rc != kOk || a.base.chunks == 0) return rc;
  return launch_edge_softmax_heads_passes<SoftmaxHeadsOp>(a, stream);
}

// grad_scores = scale * alpha * (grad_alpha - rowsum(alpha * grad_alpha)) per head; the same workspace.
inline int launch_edge_softmax_heads_backward_csr(const int* indptr, int num_rows, long long nnz, int heads, const float* alpha,
                                                  const float* grad_alpha, float scale, float* grad_scores, void* workspace,
                                                  hipStream_t stream) {
  EdgeSoftmaxHeadsArgs a{};
  const int rc = edge_softmax_heads_args(indptr, num_rows, nnz, heads, alpha, grad_alpha, scale, grad_scores, workspace, &a);
  if (rc != kOk || a.base.chunks == 0) return rc;
  return launch_edge_softmax_heads_passes<SoftmaxBackwardHeadsOp>(a, stream);
}

}  // namespace voltrix
