// Voltrix-SpMM for MI355X (gfx950) -- GAT edge scores on a CSR pattern and the two segment sums of their backward.
//
//   forward   z[e, h] = el[row_e, h] + er[col_e, h]           (one fp32 add)
//             s[e, h] = z > 0 ? z : slope z                   (torch's leaky_relu: z == 0, and a NaN, take the slope branch)
//   backward  gz[e, h] = z > 0 ? g[e, h] : slope g[e, h]      (z recomputed from el, er: s is not needed)
//             d_el[r, h] = sum_{e in row r} gz[e, h]          d_er[c, h] = sum_{e: col_e = c} gz[e, h]
//
// Why it exists.  It is the first step of a GAT layer, before the edge softmax (edge_softmax_kernels.hpp) and the aggregation.  Written in
// torch it needs an int64 row id and an int64 column id per edge, and its backward is two index_add scatters with float atomics: not
// bit-reproducible, and serialised on hub columns.  Here the forward reads one 4-byte column id per edge and the backward is two
// segment sums without atomics.
//
// Layout.  Node scalars el [num_rows, H], er [num_cols, H], edge tensors [nnz, H] in CSR order, the head index fastest, all fp32.
// Element offsets e H + h are 64-bit.
//
// Forward (gat_score_kernel).  Work is split by EDGES: one workgroup per chunk of kChunkEdges = 2048 consecutive edges.  The chunk's
// first and last rows come from a 256-ary search of indptr by the whole workgroup; each thread finds the row of its first edge by a
// binary search between them, the rows of its other seven edges by one step or, past empty rows, another binary search (no walk).  The
// (row, column) of every edge goes to LDS; `indices` is read once per edge.  Then the threads are mapped to (edge, head) with the head
// fastest, so a wave's stores to s[chunk, :] are consecutive floats (16 bytes per lane when H is a multiple of 4 and H <= 8).  el / er are
// gathered; they are [n, H] and stay in cache.  Bytes: 4 (n + 1) + 4 nnz + 4 nnz H + the node tensors.
//
// Backward (one family: gat_score_rowsum_*).  out[r, h] = sum_{e in row r} gate(a[r, h] + b[indices[e], h]) g[order ? order[e] : e, h]:
//   d_el  on the CSR with (a, b) = (el, er), no order;
//   d_er  on the transposed CSR with (a, b) = (er, el) and order = the transposed edge order (int32): fp32 addition commutes, so the
//         gate is the same bit decision as the forward's.
// Shape: the first two launches of the edge softmax, with a partial that is one float.
//   K0  out = 0 (empty rows are written by nobody else).
//   K1  one workgroup per (chunk, head).  A thread sums the segments of its eight edges in edge order, a segmented scan over the 256
//       threads (shuffles inside a wave, four wave totals through LDS, in thread order) gives every row its in-chunk sum at the thread
//       holding the row's last in-chunk edge.  A row wholly inside the chunk is written there, out[r, h]; the in-chunk sums of the
//       chunk's first and last rows that cross a chunk boundary go to the workspace (one pair per chunk and head), with the two row ids.
//   K2  one wave per (chunk, head) whose last row starts in the chunk and runs past its end (the row's owner): the row's partials merged
//       by 64 lanes in a fixed order (lane l takes chunks l, l + 64, ..., then an xor tree) and written to out[r, h].
// The output is per row, so there is no third launch.  A hub row of 67k edges costs what its edges cost: 33 chunks and one merge.
//
// Multi-head: the head is a grid dimension (not [edge, head] tiles through the scan).  The workgroups of one chunk are 8 apart in
// blockIdx.x, so its H heads run on one XCD at about the same time and the lines of g[chunk, :] come from HBM once.  The in-thread
// order, the scan and the merge tree do not depend on H, so out[:, h] of an H-head call has the BITS of the single-head call on the
// contiguous slices a[:, h], b[:, h], g[:, h].  A tile form would have to carry H floats per thread through the shuffles and make the
// tree depend on H (or fix H at compile time); the price of the grid form is 4-byte accesses at stride 4 H.
//
// Special values stay local: a NaN or +-inf in el[r, h] reaches only row r's scores of head h; a NaN in g[e, h] reaches only
// d_el[row_e, h] and d_er[col_e, h].  slope: any finite float (1: plain u_add_v; 0: ReLU; negative allowed).
//
// Numerics.  Forward: two roundings (the add, the product with float(slope)); against float64 from the fp32 inputs and float(slope),
//   |s - ref| <= 1.5 2^-23 |ref| + 2^-149,  and  2^-24 |ref| + 2^-149  for slope = 1 or a power of two;
// the sign of z is the sign of the exact sum.  Segment sums: every term is g or one rounded product, a row has deg - 1 additions in an
// order fixed by the pattern:
//   |d - ref| <= deg 2^-23 sum |gz| + 2^-149     (per row and head; deg = the row's entries, the column's for d_er).
// Integer inputs of small magnitude with slope = 0.25: every product and every sum below 2^24 is exact, whatever the order.
// No float atomics, no host synchronisation; the same inputs give the same bits on every launch; the workspace is a function of
// (nnz, H) alone.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "voltrix/edge_softmax_kernels.hpp"
#include "voltrix/launch_geometry.hpp"

namespace voltrix {

constexpr int kGatScoreThreads = kEdgeSoftmaxThreads;   // 256; a chunk is kChunkEdges = 2048 edges, kEdgesPerThread = 8 per thread
constexpr int kGatScoreMaxHeads = 65535;                // grid.y of the merge launch

struct GatScoreArgs {
  const int* indptr;    // [num_rows + 1]
  const int* indices;   // [nnz]
  const float* el;      // [num_rows, heads]
  const float* er;      // [num_cols, heads]
  float* out;           // [nnz, heads]
  int num_rows;
  int nnz;
  int heads;
  float slope;
};

struct GatRowsumArgs {
  const int* indptr;    // [num_rows + 1]
  const int* indices;   // [nnz]
  const int* order;     // [nnz] or null: g's edge of entry e
  const float* a;       // [num_rows, heads]
  const float* b;       // [*, heads], gathered by indices
  const float* g;       // [nnz, heads]
  float* out;           // [num_rows, heads]
  int2* rows;           // workspace: [chunks] (first row, last row)
  float* parts;         // workspace: [heads][2 * chunks] in-chunk sums of the chunk's first / last row
  int num_rows;
  int nnz;
  int chunks;
  int heads;
  float slope;
};

// workspace of the rowsum: rows (8 B per chunk, padded to 16) + per head two partials (4 B each) per chunk, rounded up to 16 bytes
inline long long gat_score_workspace_bytes(long long nnz, int heads) {
  const long long c = edge_softmax_chunks(nnz);
  return (c * 8 + (c & 1) * 8 + (long long)heads * c * 8 + 15) / 16 * 16;
}

__device__ __forceinline__ float gs_leaky(float z, float slope) { return z > 0.0f ? z : slope * z; }
__device__ __forceinline__ float gs_gate(float z, float g, float slope) { return z > 0.0f ? g : slope * g; }

// The rows holding edges `first` and `last` of a chunk: a 256-ary search of indptr by the whole workgroup (every thread must call it and
// gets the same result).  Invariant: indptr[lo] <= e and the row holding e is below hi.
__device__ __forceinline__ void gs_chunk_rows(const int* indptr, int num_rows, int first, int last, int t, int& r_first, int& r_last) {
  int lo0 = 0, hi0 = num_rows, lo1 = 0, hi1 = num_rows;
  while (hi0 - lo0 > 1 || hi1 - lo1 > 1) {
    const long long len0 = hi0 - lo0, len1 = hi1 - lo1;
    const int c0 = __syncthreads_count(indptr[lo0 + (int)(len0 * t / kGatScoreThreads)] <= first);
    const int c1 = __syncthreads_count(indptr[lo1 + (int)(len1 * t / kGatScoreThreads)] <= last);
    if (c0 < kGatScoreThreads) hi0 = lo0 + (int)(len0 * c0 / kGatScoreThreads);   // samples are monotone: c >= 1 hold
    lo0 += (int)(len0 * (c0 - 1) / kGatScoreThreads);
    if (c1 < kGatScoreThreads) hi1 = lo1 + (int)(len1 * c1 / kGatScoreThreads);
    lo1 += (int)(len1 * (c1 - 1) / kGatScoreThreads);
  }
  r_first = lo0;
  r_last = lo1;
}

// eight consecutive ints from p + e: two 16-byte loads when the thread has all its edges and the address allows, else clamped scalar loads
__device__ __forceinline__ void gs_load_ints(const int* p, int tb, int nk, int (&v)[kEdgesPerThread]) {
  constexpr int K = kEdgesPerThread;
  if (nk == K && (reinterpret_cast<uintptr_t>(p + tb) & 15) == 0) {
    const int4* q = reinterpret_cast<const int4*>(p + tb);
#pragma unroll
    for (int w = 0; w < K / 4; ++w) {
      const int4 u = q[w];
      v[4 * w + 0] = u.x;
      v[4 * w + 1] = u.y;
      v[4 * w + 2] = u.z;
      v[4 * w + 3] = u.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] = p[j < nk ? tb + j : (nk > 0 ? tb : 0)];
  }
}

// Forward.  kH: the number of heads at compile time (1, 4, 8: no division; 4 and 8 store 16 bytes per lane and need 16-byte aligned el,
// er, out) or 0: any number, read from the arguments.
template <int kH>
static __global__ __launch_bounds__(kGatScoreThreads) void gat_score_kernel(const GatScoreArgs args) {
#pragma clang fp contract(off)   // the add and the product are two roundings, as documented
  constexpr int K = kEdgesPerThread;
  __shared__ alignas(16) int s_row[kChunkEdges];   // written 16 bytes at a time
  __shared__ alignas(16) int s_col[kChunkEdges];

  const int c = (int)blockIdx.x;
  const int t = (int)threadIdx.x;
  const long long cb = (long long)c * kChunkEdges;
  const int chunk_begin = (int)cb;
  const int chunk_end = (int)(cb + kChunkEdges < args.nnz ? cb + kChunkEdges : args.nnz);
  const long long tb_l = cb + (long long)K * t;
  const int nk = tb_l >= chunk_end ? 0 : (chunk_end - tb_l < K ? (int)(chunk_end - tb_l) : K);
  const int tb = nk > 0 ? (int)tb_l : chunk_end;

  int r_first, r_last;
  gs_chunk_rows(args.indptr, args.num_rows, chunk_begin, chunk_end - 1, t, r_first, r_last);

  int col[K], row[K];
  gs_load_ints(args.indices, tb, nk, col);
  {
    int r = nk > 0 ? es_row_of(args.indptr, r_first, r_last + 1, tb) : r_last;
    int end = args.indptr[r + 1];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      if (j < nk && tb + j >= end) {        // the next row; past a run of empty rows a binary search, not a walk
        ++r;
        end = args.indptr[r + 1];
        if (tb + j >= end) {
          r = es_row_of(args.indptr, r, r_last + 1, tb + j);
          end = args.indptr[r + 1];
        }
      }
      row[j] = r;
    }
  }
  if (nk > 0) {                             // a thread past the chunk's end has no slot to write (the last chunk may be partial)
    int4* pr = reinterpret_cast<int4*>(s_row + K * t);
    int4* pc = reinterpret_cast<int4*>(s_col + K * t);
#pragma unroll
    for (int w = 0; w < K / 4; ++w) {
      pr[w] = int4{row[4 * w], row[4 * w + 1], row[4 * w + 2], row[4 * w + 3]};
      pc[w] = int4{col[4 * w], col[4 * w + 1], col[4 * w + 2], col[4 * w + 3]};
    }
  }
  __syncthreads();

  const int n_e = chunk_end - chunk_begin;
  const float slope = args.slope;
  if constexpr (kH == 4 || kH == 8) {
    constexpr int Q = kH / 4;                                   // 16-byte pieces per edge
    float4* out = reinterpret_cast<float4*>(args.out + cb * kH);
    for (int i = t; i < n_e * Q; i += kGatScoreThreads) {       // piece i: edge i / Q, heads 4 (i % Q) ..
      const int e = i / Q, q = i % Q;
      const float4 l = reinterpret_cast<const float4*>(args.el + (long long)s_row[e] * kH)[q];
      const float4 r = reinterpret_cast<const float4*>(args.er + (long long)s_col[e] * kH)[q];
      out[i] = float4{gs_leaky(l.x + r.x, slope), gs_leaky(l.y + r.y, slope), gs_leaky(l.z + r.z, slope), gs_leaky(l.w + r.w, slope)};
    }
  } else {
    const int H = kH ? kH : args.heads;
    float* out = args.out + cb * H;
    const int total = n_e * H;                                  // <= 2048 * 65535
    for (int i = t; i < total; i += kGatScoreThreads) {         // element i: edge i / H, head i % H
      const int e = kH == 1 ? i : i / H;
      const int h = kH == 1 ? 0 : i - e * H;
      out[i] = gs_leaky(args.el[(long long)s_row[e] * H + h] + args.er[(long long)s_col[e] * H + h], slope);
    }
  }
}

// K0 of the rowsum: out = 0
static __global__ __launch_bounds__(kGatScoreThreads) void gat_score_zero_kernel(float* out, long long count) {
  const long long i = (long long)blockIdx.x * kGatScoreThreads + threadIdx.x;
  if (i < count) out[i] = 0.0f;
}

// K1 of the rowsum: one (chunk, head) per workgroup.  Rows wholly inside the chunk are written; the in-chunk sums of the chunk's first /
// last row go to the head's workspace when the row crosses a chunk boundary.
static __global__ __launch_bounds__(kGatScoreThreads) void gat_score_rowsum_chunk_kernel(const GatRowsumArgs args) {
#pragma clang fp contract(off)   // every term is g or one rounded product: no product fused into the sum
  constexpr int K = kEdgesPerThread;
  const int c = (int)(blockIdx.x % kNumXcd + kNumXcd * (blockIdx.x / (kNumXcd * args.heads)));
  const int head = (int)(blockIdx.x / kNumXcd) % args.heads;
  if (c >= args.chunks) return;               // the whole workgroup leaves together
  const long long H = args.heads;
  const float* a = args.a + head;
  const float* b = args.b + head;
  const float* g = args.g + head;
  float* out = args.out + head;
  float* parts = args.parts + 2ll * head * args.chunks;
  __shared__ float s_incl[kGatScoreThreads];   // the scan's inclusive value (thread's last row)
  __shared__ float s_wave[4];
  __shared__ int s_wave_flag[4];

  const int t = (int)threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const long long cb = (long long)c * kChunkEdges;
  const int chunk_begin = (int)cb;
  const int chunk_end = (int)(cb + kChunkEdges < args.nnz ? cb + kChunkEdges : args.nnz);
  const long long tb_l = cb + (long long)K * t;
  const int nk = tb_l >= chunk_end ? 0 : (chunk_end - tb_l < K ? (int)(chunk_end - tb_l) : K);
  const int tb = nk > 0 ? (int)tb_l : chunk_end;

  int r_first, r_last;
  gs_chunk_rows(args.indptr, args.num_rows, chunk_begin, chunk_end - 1, t, r_first, r_last);

  // the gathers first, all in flight: b by column, g by its edge
  int col[K], ge[K];
  float bv[K], gv[K];
  gs_load_ints(args.indices, tb, nk, col);
  if (args.order != nullptr) {
    gs_load_ints(args.order, tb, nk, ge);
  } else {
#pragma unroll
    for (int j = 0; j < K; ++j) ge[j] = j < nk ? tb + j : (nk > 0 ? tb : 0);
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    bv[j] = b[col[j] * H];
    gv[j] = g[ge[j] * H];
  }

  int row[K], rs[K], re[K];
  float v[K];
  {
    int r = nk > 0 ? es_row_of(args.indptr, r_first, r_last + 1, tb) : r_last;
    int start = args.indptr[r], end = args.indptr[r + 1];
    float ar = a[r * H];
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
        ar = a[r * H];
      }
      row[j] = j < nk ? r : INT_MAX - K + j;   // distinct past the thread's edges: no segment continues into them
      rs[j] = start;
      re[j] = end;
      v[j] = j < nk ? gs_gate(ar + bv[j], gv[j], args.slope) : 0.0f;
    }
  }

  // in-thread segment sums in edge order: s[j] = the sum of j's row through j (the row's in-thread total at its last element)
  float s[K];
#pragma unroll
  for (int j = 0; j < K; ++j) s[j] = j > 0 && row[j] == row[j - 1] ? s[j - 1] + v[j] : v[j];
  float head_sum = s[0], tail = 0.0f;
  int tail_rs = tb;
  const int head_rs = nk > 0 ? rs[0] : tb;
#pragma unroll
  for (int j = 0; j < K; ++j) {   // chains of selects (an index that depends on nk becomes an indexed load from scratch)
    head_sum = j > 0 && row[j] == row[0] ? s[j] : head_sum;
    tail = j < nk ? s[j] : tail;
    tail_rs = j < nk ? rs[j] : tail_rs;
  }

  // segmented inclusive scan of (flag = the thread's last row starts in the thread, its sum) over the workgroup, in thread order
  float sc = tail;
  int f = nk == 0 || tail_rs >= tb;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float pv = __shfl_up(sc, d, 64);
    const int pf = __shfl_up(f, d, 64);
    if (lane >= d) {
      if (!f) sc = pv + sc;
      f |= pf;
    }
  }
  if (lane == 63) {
    s_wave[wave] = sc;
    s_wave_flag[wave] = f;
  }
  __syncthreads();
  if (!f) {
    for (int w = wave - 1; w >= 0; --w) {   // the preceding waves' totals, nearest first, until one holds a segment start
      sc = s_wave[w] + sc;
      if (s_wave_flag[w]) break;
    }
  }
  s_incl[t] = sc;
  __syncthreads();
  float h = head_sum;
  if (t > 0 && nk > 0 && head_rs < tb) h = s_incl[t - 1] + head_sum;

  // every row's in-chunk sum sits with the thread holding its last in-chunk edge
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if (j >= nk) continue;
    const int last = (re[j] < chunk_end ? re[j] : chunk_end) - 1;
    if (tb + j != last) continue;
    const float full = row[j] == row[0] ? h : s[j];
    if (rs[j] >= chunk_begin && re[j] <= chunk_end) {
      out[row[j] * H] = full;
    } else {                                 // crosses a chunk boundary: the chunk's first or last row (or both), finished by K2
      if (row[j] == r_first) parts[2 * c] = full;
      if (row[j] == r_last) parts[2 * c + 1] = full;
    }
  }
  if (t == 0 && head == 0) args.rows[c] = int2{r_first, r_last};
}

// K2 of the rowsum: one wave per (chunk, head = blockIdx.y); a chunk whose last row starts in it and ends past it merges that row's
// partials in an order fixed by the pattern (lane l: chunks l, l + 64, ... in turn; then an xor tree) and writes the row
static __global__ __launch_bounds__(kGatScoreThreads) void gat_score_rowsum_merge_kernel(const GatRowsumArgs args) {
  const int head = (int)blockIdx.y;
  const float* parts = args.parts + 2ll * head * args.chunks;
  const long long c_l = (long long)blockIdx.x * (kGatScoreThreads / 64) + (threadIdx.x >> 6);
  if (c_l >= args.chunks) return;
  const int c = (int)c_l;
  const int lane = (int)threadIdx.x & 63;
  const int r = args.rows[c].y;
  const long long cb = (long long)c * kChunkEdges;
  const int rs = args.indptr[r], re = args.indptr[r + 1];
  if (rs < cb || re <= cb + kChunkEdges) return;       // not the owner of a crossing row (the whole wave leaves together)
  const int c_last = (int)((re - 1) / kChunkEdges);
  float v = 0.0f;
  for (int j = c + lane; j <= c_last; j += 64) v = v + parts[j == c ? 2 * j + 1 : 2 * j];
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m, 64);
  if (lane == 0) args.out[(long long)r * args.heads + head] = v;
}

// Checks shared by both launches, on the host and before any HIP call.
inline int gat_score_check(int num_rows, long long nnz, int heads, float slope) {
  if (heads < 1 || heads > kGatScoreMaxHeads || num_rows < 0 || nnz < 0 || nnz > INT_MAX || !std::isfinite(slope)) return kErrBadShape;
  if ((long long)heads * num_rows > INT_MAX) return kErrBadShape;
  if (nnz > 0 && num_rows == 0) return kErrBadShape;
  return kOk;
}

// out[e, h] = leaky_relu(el[row_e, h] + er[indices[e], h], slope) for every entry of a device CSR; el [num_rows, heads], er [*, heads],
// out [nnz, heads].  Nothing is checked on the device: indptr must be a valid CSR of num_rows rows ending at nnz, indices inside er.
inline int launch_gat_score_csr(const int* indptr, const int* indices, int num_rows, long long nnz, int heads, const float* el,
                                const float* er, float slope, float* out, hipStream_t stream) {
  const int rc = gat_score_check(num_rows, nnz, heads, slope);
  if (rc != kOk || nnz == 0) return rc;
  if (bad_ptr(indptr, 3) || bad_ptr(indices, 3) || bad_ptr(el, 3) || bad_ptr(er, 3) || bad_ptr(out, 3))
    return kErrBadShape;
  const GatScoreArgs a{indptr, indices, el, er, out, num_rows, (int)nnz, heads, slope};
  const dim3 grid((unsigned)edge_softmax_chunks(nnz)), block(kGatScoreThreads);
  const bool wide = (((uintptr_t)el | (uintptr_t)er | (uintptr_t)out) & 15) == 0;
  if (heads == 1) hipLaunchKernelGGL((gat_score_kernel<1>), grid, block, 0, stream, a);
  else if (heads == 4 && wide) hipLaunchKernelGGL((gat_score_kernel<4>), grid, block, 0, stream, a);
  else if (heads == 8 && wide) hipLaunchKernelGGL((gat_score_kernel<8>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((gat_score_kernel<0>), grid, block, 0, stream, a);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// out[r, h] = sum_{e in row r} gate(a[r, h] + b[indices[e], h]) g[order ? order[e] : e, h], gate(z) = z > 0 ? 1 : slope; every element
// of out [num_rows, heads] is written, empty rows zero.  order: null or int32 [nnz].  workspace: gat_score_workspace_bytes(nnz, heads)
// bytes, 16-byte aligned (not touched when nnz == 0).
inline int launch_gat_score_rowsum_csr(const int* indptr, const int* indices, const int* order, int num_rows, long long nnz, int heads,
                                       const float* a, const float* b, const float* g, float slope, float* out, void* workspace,
                                       hipStream_t stream) {
  const int rc = gat_score_check(num_rows, nnz, heads, slope);
  if (rc != kOk || num_rows == 0) return rc;
  if (bad_ptr(out, 3)) return kErrBadShape;
  if (nnz > 0 && (bad_ptr(indptr, 3) || bad_ptr(indices, 3) || bad_ptr(a, 3) || bad_ptr(b, 3) ||
                  bad_ptr(g, 3) || bad_ptr(workspace, 15) || misaligned(order, 3)))
    return kErrBadShape;
  const long long chunks = edge_softmax_chunks(nnz);
  const long long chunks8 = (chunks + kNumXcd - 1) / kNumXcd * kNumXcd;
  if (chunks8 * heads > 0x7fffffffLL) return kErrBadShape;
  const dim3 block(kGatScoreThreads);
  const long long count = (long long)num_rows * heads;
  hipLaunchKernelGGL(gat_score_zero_kernel, dim3((unsigned)((count + kGatScoreThreads - 1) / kGatScoreThreads)), block, 0, stream, out,
                     count);
  if (nnz > 0) {
    char* ws = static_cast<char*>(workspace);
    const GatRowsumArgs args{indptr, indices, order, a, b, g, out, reinterpret_cast<int2*>(ws),
                             reinterpret_cast<float*>(ws + chunks * 8 + (chunks & 1) * 8), num_rows, (int)nnz, (int)chunks, heads, slope};
    hipLaunchKernelGGL(gat_score_rowsum_chunk_kernel, dim3((unsigned)(chunks8 * heads)), block, 0, stream, args);
    if (chunks > 1)
      hipLaunchKernelGGL(gat_score_rowsum_merge_kernel, dim3((unsigned)((chunks + 3) / 4), (unsigned)heads), block, 0, stream, args);
  }
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

}  // namespace voltrix
