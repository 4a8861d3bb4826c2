// Voltrix-SpMM for MI355X (gfx950) -- edge softmax on a CSR pattern: the softmax of per-edge scores over every row, and its backward.
//
//   forward   alpha[e] = exp(z_e - m_r) / sum_{e' in row r} exp(z_e' - m_r),   z = scale * s,  m_r = max_{e' in row r} z_e'
//   backward  grad_s[e] = scale * alpha[e] * (g[e] - sum_{e' in row r} alpha[e'] g[e'])
//
// Why it exists.  It is the step of an attention layer between the scores (sddmm_kernels.hpp) and the aggregation with the weights
// (spmm_csr_rows_kernel with values): GAT and dot-product graph transformers.  Written in torch it takes ~8 kernels, two of them float
// atomic scatters (not deterministic), and an int64 row id per edge.
//
// Shape.  Work is split by EDGES, like the SDDMM: hub rows (84k edges) and rows of one edge cost what their edges cost.  Three launches:
//   K1  one workgroup per chunk of kChunkEdges = 256 threads x kEdgesPerThread consecutive edges.  The chunk's first and last rows come
//       from a 256-ary search of indptr by the whole workgroup (3-4 dependent loads); each thread finds the row of its first edge
//       by a binary search between them, the rows of its other edges by one step or, past empty rows, another binary search (no
//       walk: a run of empty rows costs a logarithm, not its length).  A thread reduces the segments of its edges in edge order
//       (registers), a segmented scan over the 256 threads (shuffles inside a wave, four wave totals through LDS, in thread order)
//       gives every row its in-chunk partial, and
//       rows that lie wholly inside the chunk are finished and written here.  The in-chunk partials of the chunk's first and last rows
//       go to the workspace (one pair per chunk), with the two row ids.
//   K2  one wave per chunk whose last row starts in it and runs past its end (the row's owner): the row's partials, from the owner to
//       the chunk holding its last edge, merged by 64 lanes in a fixed order (lane l takes chunks l, l + 64, ..., then an xor tree).
//   K3  one workgroup per chunk: the segments of its first and last rows that cross a chunk boundary, finished from the merged partial.
// The combine across workgroups happens at kernel boundaries only -- no flags, counters or last-block protocols.
//
// The template is shared: an Op gives the per-edge data, the in-thread segment reduction, the merge of two partials and the output.
//   forward   partial (m, s): m = max key, s = sum exp(a (key - m)), key = sign(scale) s, a = |scale| (so z - m = a (key - m): the
//             max and the difference are taken before the scaling, and a rounding of scale * s costs nothing); online-softmax merge
//   backward  partial (d): d = sum alpha g, merged by addition
//
// Special values.  Empty rows write nothing.  z = -inf gives alpha = 0; a row whose entries are all -inf gets zeros (torch's softmax
// gives NaN) and, in the backward, zero gradients.  A NaN in a row makes every alpha of that row NaN and no other row's.  scale = 0
// (or -0) gives every entry 1 / (the row's entries that are not -inf), and s = -inf still 0 (torch: 0 * -inf = NaN).
//
// Numerics.  exp is v_exp_f32 (exp2 of x log2 e).  For a row of deg_r entries,
//   |alpha_e - ref_e| <= ref_e * 2 (deg_r + |z_e - m_r| + 2) 2^-23 + 2^-126
// where ref is the exact softmax (float64 in the tests): each exponent a (key - m) carries three roundings (difference, scale, log2 e:
// 1.5 |z - m| 2^-23), v_exp_f32 and the reciprocal one ulp each, and S (>= 1: the max term is exactly 1) collects at most deg_r - 1
// additions and rescales, whose errors sum to <= 1.6 deg_r 2^-23 S because exp(-x) x <= 1/e.  The 2^-126 covers results in fp32's
// subnormal range (exponents below -87).  Backward: with D_r = sum alpha g and A_r = sum alpha |g| (float64),
//   |grad_e - ref_e| <= |scale| alpha_e (2 |g_e - D_r| + (deg_r + 2) A_r) 2^-23 + 2^-126.
// Sums run in an order fixed by the pattern (edge order inside a thread, a fixed scan tree, across chunks 64 strided lanes and a fixed xor tree): the same inputs
// give the same bits on every launch.  No float atomics.  The workspace size depends on nnz alone, nothing is read back on the host.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "voltrix/launch_geometry.hpp"
#include "voltrix/spmm_kernels.hpp"

namespace voltrix {

constexpr int kEdgeSoftmaxThreads = 256;
constexpr int kEdgesPerThread = 8;
constexpr int kChunkEdges = kEdgeSoftmaxThreads * kEdgesPerThread;   // 2048 consecutive edges per K1 workgroup

struct SoftmaxPart {
  float m, s;
};

// per chunk: rows[c] = (first row, last row), parts[c] = (in-chunk partial of the first row, of the last row), merged[c] = the merged
// partial of the row this chunk owns (written by K2 for owners only)
struct EdgeSoftmaxArgs {
  const int* indptr;     // [num_rows + 1]
  const float* in0;      // forward: scores; backward: alpha
  const float* in1;      // backward: grad_alpha
  float* out;            // [nnz]
  int2* rows;            // workspace
  SoftmaxPart* parts;    // [2 * chunks]
  SoftmaxPart* merged;   // [chunks]
  int num_rows;
  int nnz;
  int chunks;
  float scale;
  float sign;            // forward: +1 / -1 = sign of scale; key = sign * s
  float a;               // forward: |scale|
};

inline long long edge_softmax_chunks(long long nnz) { return (nnz + kChunkEdges - 1) / kChunkEdges; }

// workspace: rows (8 B) + two partials (16 B) + merged (8 B) per chunk, each array 16-byte aligned
inline long long edge_softmax_workspace_bytes(long long nnz) {
  const long long c = edge_softmax_chunks(nnz);
  const long long pad = (c & 1) * 8;
  return c * 8 + pad + c * 16 + c * 8;
}

__device__ __forceinline__ float es_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }

struct SoftmaxOp {
  using Part = SoftmaxPart;
  struct Elem {
    float key;
  };
  const EdgeSoftmaxArgs a;
  __device__ Part identity() const { return Part{-INFINITY, 0.0f}; }
  __device__ Elem load(int e) const { return Elem{a.sign * a.in0[e]}; }
  __device__ void load_vec(int e, Elem (&el)[kEdgesPerThread]) const {
    const float4* p = reinterpret_cast<const float4*>(a.in0 + e);
#pragma unroll
    for (int q = 0; q < kEdgesPerThread / 4; ++q) {
      const float4 v = p[q];
      el[4 * q + 0].key = a.sign * v.x;
      el[4 * q + 1].key = a.sign * v.y;
      el[4 * q + 2].key = a.sign * v.z;
      el[4 * q + 3].key = a.sign * v.w;
    }
  }
  // weight of a partial taken at max mi inside a merge at max m: 1 when equal (also both -inf), 0 for an empty or all -inf partial
  // below m (tested, not computed: with scale = 0, a (mi - m) would be 0 * -inf = NaN), else exp(a (mi - m))
  __device__ float weight(float mi, float m) const {
    return mi == m ? 1.0f : (mi == -INFINITY ? 0.0f : es_exp(a.a * (mi - m)));
  }
  __device__ Part merge(const Part& l, const Part& r) const {
    const float m = fmaxf(l.m, r.m);
    return Part{m, l.s * weight(l.m, m) + r.s * weight(r.m, m)};
  }
  __device__ float term(const Elem& x, float m) const { return x.key == -INFINITY ? 0.0f : es_exp(a.a * (x.key - m)); }
  // in-thread segments: every element gets its segment's partial; t[j] keeps exp(a (key_j - m_seg)) for finish()
  __device__ void reduce(const Elem (&el)[kEdgesPerThread], const int (&row)[kEdgesPerThread], int nk, Part (&p)[kEdgesPerThread],
                         float (&t)[kEdgesPerThread]) const {
    float m[kEdgesPerThread], s[kEdgesPerThread];
#pragma unroll
    for (int j = 0; j < kEdgesPerThread; ++j) {
      const bool cont = j > 0 && row[j] == row[j - 1];
      m[j] = cont ? fmaxf(m[j - 1], el[j].key) : el[j].key;
    }
#pragma unroll
    for (int j = kEdgesPerThread - 2; j >= 0; --j)
      if (j + 1 < nk && row[j + 1] == row[j]) m[j] = m[j + 1];
#pragma unroll
    for (int j = 0; j < kEdgesPerThread; ++j) {
      t[j] = term(el[j], m[j]);
      const bool cont = j > 0 && row[j] == row[j - 1];
      s[j] = cont ? s[j - 1] + t[j] : t[j];
    }
#pragma unroll
    for (int j = kEdgesPerThread - 2; j >= 0; --j)
      if (j + 1 < nk && row[j + 1] == row[j]) s[j] = s[j + 1];
#pragma unroll
    for (int j = 0; j < kEdgesPerThread; ++j) p[j] = Part{m[j], s[j]};
  }
  // local: the element's in-thread partial (its t is exp against local.m); full: the row's partial
  __device__ float finish(const Elem& x, float t, const Part& local, const Part& full) const {
    if (x.key == -INFINITY) return 0.0f * full.s;      // 0, or NaN for a row holding a NaN
    const float num = local.m == full.m ? t : es_exp(a.a * (x.key - full.m));
    return num * __builtin_amdgcn_rcpf(full.s);
  }
  __device__ float finish(const Elem& x, const Part& full) const {
    if (x.key == -INFINITY) return 0.0f * full.s;
    return es_exp(a.a * (x.key - full.m)) * __builtin_amdgcn_rcpf(full.s);
  }
};

struct SoftmaxBackwardOp {
  using Part = SoftmaxPart;   // s = sum alpha g; m unused (0)
  struct Elem {
    float alpha, g;
  };
  const EdgeSoftmaxArgs a;
  __device__ Part identity() const { return Part{0.0f, 0.0f}; }
  __device__ Elem load(int e) const { return Elem{a.in0[e], a.in1[e]}; }
  __device__ void load_vec(int e, Elem (&el)[kEdgesPerThread]) const {
    const float4* p = reinterpret_cast<const float4*>(a.in0 + e);
    const float4* q = reinterpret_cast<const float4*>(a.in1 + e);
#pragma unroll
    for (int w = 0; w < kEdgesPerThread / 4; ++w) {
      const float4 u = p[w], v = q[w];
      el[4 * w + 0] = Elem{u.x, v.x};
      el[4 * w + 1] = Elem{u.y, v.y};
      el[4 * w + 2] = Elem{u.z, v.z};
      el[4 * w + 3] = Elem{u.w, v.w};
    }
  }
  __device__ Part merge(const Part& l, const Part& r) const { return Part{0.0f, l.s + r.s}; }
  __device__ void reduce(const Elem (&el)[kEdgesPerThread], const int (&row)[kEdgesPerThread], int nk, Part (&p)[kEdgesPerThread],
                         float (&t)[kEdgesPerThread]) const {
    float s[kEdgesPerThread];
#pragma unroll
    for (int j = 0; j < kEdgesPerThread; ++j) {
      t[j] = 0.0f;
      const float v = el[j].alpha * el[j].g;
      s[j] = j > 0 && row[j] == row[j - 1] ? s[j - 1] + v : v;
    }
#pragma unroll
    for (int j = kEdgesPerThread - 2; j >= 0; --j)
      if (j + 1 < nk && row[j + 1] == row[j]) s[j] = s[j + 1];
#pragma unroll
    for (int j = 0; j < kEdgesPerThread; ++j) p[j] = Part{0.0f, s[j]};
  }
  __device__ float finish(const Elem& x, const Part& full) const { return a.scale * (x.alpha * (x.g - full.s)); }
  __device__ float finish(const Elem& x, float, const Part&, const Part& full) const { return finish(x, full); }
};

// last r in [lo, hi) with indptr[r] <= e (the row holding e when indptr[lo] <= e < indptr[hi])
__device__ __forceinline__ int es_row_of(const int* indptr, int lo, int hi, int e) {
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (indptr[mid] <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}

template <class Op>
__device__ __forceinline__ void es_shfl_up(typename Op::Part& v, int& f, int d) {
  v.m = __shfl_up(v.m, d, 64);
  v.s = __shfl_up(v.s, d, 64);
  f = __shfl_up(f, d, 64);
}

// K1: one chunk per workgroup.  Rows wholly inside the chunk are written; the chunk's first / last row partials go to the workspace.
template <class Op>
static __global__ __launch_bounds__(kEdgeSoftmaxThreads) void edge_softmax_chunk_kernel(const EdgeSoftmaxArgs args) {
  using Part = typename Op::Part;
  constexpr int K = kEdgesPerThread;
  const Op op{args};
  __shared__ Part s_incl[kEdgeSoftmaxThreads];   // the scan's inclusive value (thread's last row)
  __shared__ Part s_head[kEdgeSoftmaxThreads];   // in-chunk partial of the thread's first row, through the thread's edges
  __shared__ Part s_wave[4];
  __shared__ int s_wave_flag[4];

  const int c = (int)blockIdx.x;
  const int t = (int)threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const long long cb = (long long)c * kChunkEdges;
  const int chunk_begin = (int)cb;
  const int chunk_end = (int)(cb + kChunkEdges < args.nnz ? cb + kChunkEdges : args.nnz);
  const long long tb_l = cb + (long long)K * t;
  const int nk = tb_l >= chunk_end ? 0 : (chunk_end - tb_l < K ? (int)(chunk_end - tb_l) : K);
  const int tb = nk > 0 ? (int)tb_l : chunk_end;

  // the rows holding chunk_begin and chunk_end - 1: a 256-ary search by the whole workgroup (a few dependent loads instead of the
  // log2(num_rows) of a binary search).  Invariant: indptr[lo] <= e and the row holding e is below hi; every thread keeps the same bounds.
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
  if (nk == K && ((reinterpret_cast<uintptr_t>(args.in0) | reinterpret_cast<uintptr_t>(args.in1)) & 15) == 0) {
    op.load_vec(tb, el);
  } else {
#pragma unroll
    for (int j = 0; j < K; ++j) el[j] = op.load(j < nk ? tb + j : (nk > 0 ? tb : 0));
  }
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
  Part head = op.identity(), tail = op.identity();
  int tail_rs = tb, head_rs = tb;
  if (nk > 0) {
    head = p[0];
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
  Part h = head;
  if (t > 0 && nk > 0 && head_rs < tb) h = op.merge(s_incl[t - 1], head);
  s_head[t] = h;
  __syncthreads();

  // every row's in-chunk partial sits with the thread holding its last in-chunk edge; rows inside the chunk are finished here
  float res[K];
  bool all_done = nk == K;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    res[j] = 0.0f;
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
    if (rs[j] < chunk_begin || re[j] > chunk_end) {
      all_done = false;                     // crosses a chunk boundary: K3
      continue;
    }
    res[j] = op.finish(el[j], tt[j], p[j], full);
  }
  if (t == 0) args.rows[c] = int2{r_first, r_last};
  if (all_done && (reinterpret_cast<uintptr_t>(args.out) & 15) == 0) {
    float4* o = reinterpret_cast<float4*>(args.out + tb);
#pragma unroll
    for (int q = 0; q < K / 4; ++q) o[q] = float4{res[4 * q], res[4 * q + 1], res[4 * q + 2], res[4 * q + 3]};
  } else {
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (j < nk && rs[j] >= chunk_begin && re[j] <= chunk_end) args.out[tb + j] = res[j];
  }
}

// K2: one wave per chunk; a chunk whose last row starts in it and ends past it merges that row's partials in an
// order fixed by the pattern (lane l: chunks l, l + 64, ... in turn; then an xor tree, the lower lanes' partial on the left)
template <class Op>
static __global__ __launch_bounds__(kEdgeSoftmaxThreads) void edge_softmax_merge_kernel(const EdgeSoftmaxArgs args) {
  using Part = typename Op::Part;
  const Op op{args};
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

// K3: one workgroup per chunk: the chunk's first / last row segments that cross a chunk boundary, from the merged partials
template <class Op>
static __global__ __launch_bounds__(kEdgeSoftmaxThreads) void edge_softmax_boundary_kernel(const EdgeSoftmaxArgs args) {
  using Part = typename Op::Part;
  const Op op{args};
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
      args.out[chunk_begin + i] = op.finish(op.load(chunk_begin + i), full);
  }
  if (rr.y != rr.x) {
    const int rs1 = args.indptr[rr.y], re1 = args.indptr[rr.y + 1];
    if (re1 > chunk_end) {
      const Part full = args.merged[c];
      for (int i = (int)threadIdx.x; i < chunk_end - rs1; i += kEdgeSoftmaxThreads) args.out[rs1 + i] = op.finish(op.load(rs1 + i), full);
    }
  }
}

template <class Op>
inline int launch_edge_softmax_passes(const EdgeSoftmaxArgs& a, hipStream_t stream) {
  const dim3 block(kEdgeSoftmaxThreads);
  hipLaunchKernelGGL((edge_softmax_chunk_kernel<Op>), dim3((unsigned)a.chunks), block, 0, stream, a);
  if (a.chunks > 1) {
    hipLaunchKernelGGL((edge_softmax_merge_kernel<Op>), dim3((unsigned)((a.chunks + 3) / 4)), block, 0, stream, a);
    hipLaunchKernelGGL((edge_softmax_boundary_kernel<Op>), dim3((unsigned)a.chunks), block, 0, stream, a);
  }
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// Shared checks and workspace carving.  Returns kOk with *args filled, kOk with args->chunks == 0 for nothing to do, or an error code.
inline int edge_softmax_args(const int* indptr, int num_rows, long long nnz, const float* in0, const float* in1, float scale, float* out,
                             void* workspace, EdgeSoftmaxArgs* args) {
  if (num_rows < 0 || nnz < 0 || nnz > INT_MAX || !std::isfinite(scale)) return kErrBadShape;
  args->chunks = 0;
  if (nnz == 0) return kOk;
  if (num_rows == 0 || bad_ptr(indptr, 3) || bad_ptr(in0, 3) || bad_ptr(in1, 3) || bad_ptr(out, 3) || bad_ptr(workspace, 15))
    return kErrBadShape;
  const long long chunks = edge_softmax_chunks(nnz);
  char* ws = static_cast<char*>(workspace);
  args->indptr = indptr;
  args->in0 = in0;
  args->in1 = in1;
  args->out = out;
  args->rows = reinterpret_cast<int2*>(ws);
  args->parts = reinterpret_cast<SoftmaxPart*>(ws + chunks * 8 + (chunks & 1) * 8);
  args->merged = reinterpret_cast<SoftmaxPart*>(ws + chunks * 8 + (chunks & 1) * 8 + chunks * 16);
  args->num_rows = num_rows;
  args->nnz = (int)nnz;
  args->chunks = (int)chunks;
  args->scale = scale;
  args->sign = scale < 0.0f ? -1.0f : 1.0f;
  args->a = std::fabs(scale);
  return kOk;
}

// alpha = edge softmax of scale * scores over every row of a device CSR; workspace: edge_softmax_workspace_bytes(nnz) bytes, 16-B aligned.
// Nothing is checked on the device: indptr must be a valid CSR of num_rows rows ending at nnz.
inline int launch_edge_softmax_csr(const int* indptr, int num_rows, long long nnz, const float* scores, float scale, float* out,
                                   void* workspace, hipStream_t stream) {
  EdgeSoftmaxArgs a{};
  const int rc = edge_softmax_args(indptr, num_rows, nnz, scores, scores, scale, out, workspace, &a);
  if (rc != kOk || a.chunks == 0) return rc;
  return launch_edge_softmax_passes<SoftmaxOp>(a, stream);
}

// grad_scores = scale * alpha * (grad_alpha - rowsum(alpha * grad_alpha)); the same workspace.
inline int launch_edge_softmax_backward_csr(const int* indptr, int num_rows, long long nnz, const float* alpha, const float* grad_alpha,
                                            float scale, float* grad_scores, void* workspace, hipStream_t stream) {
  EdgeSoftmaxArgs a{};
  const int rc = edge_softmax_args(indptr, num_rows, nnz, alpha, grad_alpha, scale, grad_scores, workspace, &a);
  if (rc != kOk || a.chunks == 0) return rc;
  return launch_edge_softmax_passes<SoftmaxBackwardOp>(a, stream);
}

}  // namespace voltrix
