// Voltrix-SpMM for MI355X (gfx950) -- neighbour sampling on a device CSR and the relabelling of a sampled block:
//   (s_indices, s_entries) = for every seed row, at most `fanout` of its entries (their column ids and their CSR entry ids)
//   (src_ids, local)       = the block's source nodes -- the seeds first, then the other sampled columns in ascending id -- and
//                            every sampled column as a position in src_ids
// What produces the rectangular [num_dst, num_src] patterns that every CSR operator here takes (spmm_csr_*, sddmm, attn_aggregate,
// spmm_csr_reduce): GraphSAGE-style mini-batches.  No reference counterpart.
//
// THE SAMPLING RULE (the contract; voltrix/sampling.py and DESIGN.md 3.23 restate it, tests/sample_oracle.py is the numpy restatement).
// For a seed row r (its GLOBAL row id), fan-out k, degree d = indptr[r + 1] - indptr[r], a 64-bit seed and a 64-bit offset:
//   draw(r, i)   word i & 3 of Philox4x32-10(counter = (r, (i >> 2) | 0x80000000, offset & 0xffffffff, offset >> 32),
//                key = (seed & 0xffffffff, seed >> 32)).  Bit 31 of counter word 1 separates these draws from the dropout mask's
//                (edge, h >> 2, ...) counters (dropout_mask_kernels.hpp: h >> 2 < 2^29), so one seed for both gives unrelated streams.
//   without replacement, d <= k   every entry of the row, in CSR order; no draw is used.  "all" (fan-out kSampleAll, Python's
//                fanout=None) means this for every row, with or without replacement.
//   without replacement, d > k    Floyd's algorithm on entry POSITIONS 0 .. d - 1: for i = 0 .. k - 1, j = d - k + i,
//                t = (uint64(draw(r, i)) * (j + 1)) >> 32; take t unless it is taken already, then take j.  The k positions are output
//                in ASCENDING order: a sampled row keeps CSR order, sorted rows stay sorted.  A function of (seed, offset, r, d, k)
//                only -- not of the other seeds of the batch, their order or the launch geometry.  Every k-subset is equally likely up
//                to the multiply-shift's bias: t's values differ in probability by at most a relative (j + 1) / 2^32 <= d / 2^32.
//   with replacement, d > 0       exactly k entries; entry i is at position (uint64(draw(r, i)) * d) >> 32, in draw order.  d == 0: none.
//
// sample_neighbors_kernel: one lane per seed row, 256 lanes per workgroup.  Per row O(k^2) compares and k four-byte gathers from
// `indices` -- not a function of the degree: a 67k-entry hub row costs what a row of degree k + 1 costs (no hub-row weakness, unlike the
// row-per-group kernels).  The sorted positions of Floyd's algorithm live in dynamic LDS, slot-major: slot[j * 256 + lane] -- bank
// lane mod 32 for every j, so lanes that insert at different depths do not conflict; 256 k 4 bytes, k <= 64 (64 KiB: two workgroups per
// CU).  No per-lane array in registers, hence no scratch.  The replacement path and "all" use no LDS.  "all" copies a row with its one
// lane: O(d) per lane there, the one path whose cost follows the degree.
// A seed outside [0, num_rows) has degree 0 inside the kernel (never an out-of-bounds read); a row never writes more than its segment
// s_indptr[i + 1] - s_indptr[i] holds.
//
// Relabelling: a dense table int32 [num_cols], ZERO on entry.  block_mark: table[c] = 1 for every sampled column (plain stores of one
// value); block_mark_seeds, a later launch on the same stream: table[seeds[i]] = -(i + 1) -- the seeds win.  The caller takes the
// inclusive count `rank` of the positive marks (plumbing), then block_relabel: local[e] = t < 0 ? -t - 1 : S + rank[c] - 1 with
// t = table[c], src_ids[S + rank[c] - 1] = c for marked c (duplicates store the same value), src_ids[i] = seeds[i].  So src_ids[:S] is
// the seeds in the given order and src_ids[S:] the other columns ascending: deterministic, and feat[src_ids] gathers in ascending
// addresses.  Duplicate seeds are the caller's to exclude (the later store wins: which one is not defined).
//
// No atomics anywhere; offsets that can pass 2^31 are 64-bit; entry counts are limited to INT_MAX; no host synchronisation.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "voltrix/dropout_mask_kernels.hpp"
#include "voltrix/launch_geometry.hpp"

namespace voltrix {

constexpr int kSampleMaxFanout = 64;
constexpr int kSampleAll = -1;               // the `fanout` that takes every entry of every row
constexpr uint32_t kSampleCounterBit = 0x80000000u;

// draw(r, i) for i = 0, 1, 2, ...: one Philox evaluation per four draws
struct SampleDraws {
  uint32_t r, k0, k1, off0, off1;
  Philox4 block;
  __host__ __device__ inline uint32_t operator()(int i) {
    if ((i & 3) == 0) block = philox4x32_10(r, (uint32_t)(i >> 2) | kSampleCounterBit, off0, off1, k0, k1);
    const int w = i & 3;      // selects, not an indexed read: a dynamic index would put the four words into scratch (or LDS)
    return w == 0 ? block.x[0] : w == 1 ? block.x[1] : w == 2 ? block.x[2] : block.x[3];
  }
};

// Floyd's algorithm of the rule above for d > k >= 1: leaves the k positions ascending in slot.get(0 .. k - 1).  `slot` is any object
// with `int get(int) const` and `void set(int, int)` (LDS in the kernel, an array in a host program): the same code on both sides.
template <class Slots>
__host__ __device__ inline void sample_row_positions(uint32_t r, int d, int k, uint32_t k0, uint32_t k1, uint32_t off0, uint32_t off1,
                                                     Slots& slot) {
  SampleDraws draw{r, k0, k1, off0, off1, {}};
  for (int i = 0; i < k; ++i) {
    const int j = d - k + i;
    const int t = (int)(((uint64_t)draw(i) * (uint64_t)(j + 1)) >> 32);       // in [0, j]
    int p = i;                                                                // slots [p, i) hold positions above t
    while (p > 0 && slot.get(p - 1) > t) --p;
    if (p > 0 && slot.get(p - 1) == t) {
      slot.set(i, j);                                                         // every earlier position is below j
    } else {
      for (int q = i; q > p; --q) slot.set(q, slot.get(q - 1));
      slot.set(p, t);
    }
  }
}

// position i of the replacement rule
__host__ __device__ inline int sample_replace_position(uint32_t x, int d) { return (int)(((uint64_t)x * (uint64_t)d) >> 32); }

struct SampleNeighborsArgs {
  const int* indptr;     // [num_rows + 1]
  const int* indices;    // [entries]
  const int* seeds;      // [num_seeds] global row ids
  const int* s_indptr;   // [num_seeds + 1] where every seed's entries go
  int* s_indices;        // [num_sampled] global column ids
  int* s_entries;        // [num_sampled] CSR entry ids
  int num_rows;
  int num_seeds;
  int k;                 // 1 .. 64, or INT_MAX for "all"
  uint32_t k0, k1;       // seed
  uint32_t off0, off1;   // offset
};

struct LdsSlots {
  int* base;             // this lane's column of the slot-major array
  __device__ inline int get(int j) const { return base[j * 256]; }
  __device__ inline void set(int j, int v) { base[j * 256] = v; }
};

template <bool REPLACE>
static __global__ __launch_bounds__(256) void sample_neighbors_kernel(const SampleNeighborsArgs a) {
  extern __shared__ __attribute__((aligned(16))) int sample_slots[];          // [k][256], only where a row has d > k
  const long long i = (long long)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= a.num_seeds) return;
  const int r = a.seeds[i];
  int begin = 0, d = 0;
  if (r >= 0 && r < a.num_rows) {
    begin = a.indptr[r];
    d = a.indptr[r + 1] - begin;
  }
  const long long base = a.s_indptr[i];
  const int room = a.s_indptr[i + 1] - a.s_indptr[i];
  int* const out_col = a.s_indices + base;
  int* const out_entry = a.s_entries + base;
  if (d <= 0 || room <= 0) return;
  if (a.k == INT_MAX || (!REPLACE && d <= a.k)) {    // every entry, in CSR order ("all": k = INT_MAX)
    const int count = d < room ? d : room;
    for (int j = 0; j < count; ++j) {
      out_entry[j] = begin + j;
      out_col[j] = a.indices[(long long)begin + j];
    }
    return;
  }
  const int count = a.k < room ? a.k : room;         // == k for an s_indptr made by the rule
  if constexpr (REPLACE) {
    SampleDraws draw{(uint32_t)r, a.k0, a.k1, a.off0, a.off1, {}};
    for (int j = 0; j < a.k; ++j) {
      const int e = begin + sample_replace_position(draw(j), d);
      if (j < count) {
        out_entry[j] = e;
        out_col[j] = a.indices[e];
      }
    }
  } else {
    LdsSlots slot{sample_slots + (int)threadIdx.x};
    sample_row_positions((uint32_t)r, d, a.k, a.k0, a.k1, a.off0, a.off1, slot);
    for (int j = 0; j < count; ++j) {
      const int e = begin + slot.get(j);
      out_entry[j] = e;
      out_col[j] = a.indices[e];
    }
  }
}

// fanout: 1 .. 64, or kSampleAll.  s_indptr must be the rule's: s_indptr[i + 1] - s_indptr[i] = min(d_i, fanout) without replacement,
// (d_i > 0 ? fanout : 0) with it, d_i for kSampleAll, d_i = 0 for a seed outside [0, num_rows); num_sampled = s_indptr[num_seeds].
// Every element of s_indices and s_entries is written then; neither needs initialising.  Nothing else is checked on the device.
inline int launch_sample_neighbors(const int* indptr, const int* indices, int num_rows, const int* seeds, int num_seeds,
                                   const int* s_indptr, long long num_sampled, int fanout, int replace, uint64_t seed, uint64_t offset,
                                   int* s_indices, int* s_entries, hipStream_t stream) {
  if (num_rows < 0 || num_seeds < 0 || num_sampled < 0 || num_sampled > INT_MAX) return kErrBadShape;
  if (fanout != kSampleAll && (fanout < 1 || fanout > kSampleMaxFanout)) return kErrBadShape;
  if (replace != 0 && replace != 1) return kErrBadShape;
  if (num_seeds == 0) return kOk;
  if (bad_ptr(indptr, 3) || bad_ptr(seeds, 3) || bad_ptr(s_indptr, 3)) return kErrBadShape;
  if (num_sampled > 0 && (bad_ptr(indices, 3) || bad_ptr(s_indices, 3) || bad_ptr(s_entries, 3))) return kErrBadShape;
  if (num_sampled == 0) return kOk;                  // nothing to write
  const bool all = fanout == kSampleAll;
  const SampleNeighborsArgs a{indptr, indices, seeds, s_indptr, s_indices, s_entries, num_rows, num_seeds, all ? INT_MAX : fanout,
                              (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
  const dim3 grid((unsigned)(((long long)num_seeds + 255) / 256));
  if (replace || all)
    hipLaunchKernelGGL((sample_neighbors_kernel<true>), grid, dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL((sample_neighbors_kernel<false>), grid, dim3(256), (size_t)256 * fanout * sizeof(int), stream, a);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// ---- relabelling ---------------------------------------------------------------------------------------------------------------------
// a grid of 256-lane workgroups over `total` items, capped like dropout_mask_kernel's; a lane strides
inline unsigned block_grid(long long total) {
  const long long blocks = (total + 255) / 256;
  return (unsigned)(blocks < kDropoutMaskMaxBlocks ? blocks : kDropoutMaskMaxBlocks);
}

static __global__ __launch_bounds__(256) void block_mark_kernel(const int* cols, long long count, int num_cols, int* table) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long e = (long long)blockIdx.x * 256 + (int)threadIdx.x; e < count; e += stride) {
    const int c = cols[e];
    if (c >= 0 && c < num_cols) table[c] = 1;
  }
}

static __global__ __launch_bounds__(256) void block_mark_seeds_kernel(const int* seeds, int num_seeds, int num_cols, int* table) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + (int)threadIdx.x; i < num_seeds; i += stride) {
    const int c = seeds[i];
    if (c >= 0 && c < num_cols) table[c] = -(int)(i + 1);
  }
}

struct BlockRelabelArgs {
  const int* cols;       // [count] sampled global column ids
  const int* seeds;      // [num_seeds]
  const int* table;      // [num_cols] after both mark launches
  const int* rank;       // [num_cols] inclusive count of table > 0
  int* local;            // [count]
  int* src_ids;          // [num_src]
  long long count;
  int num_seeds;
  int num_cols;
  int num_src;
};

static __global__ __launch_bounds__(256) void block_relabel_kernel(const BlockRelabelArgs a) {
  const long long stride = (long long)gridDim.x * 256;
  const long long total = a.count > a.num_seeds ? a.count : a.num_seeds;
  for (long long e = (long long)blockIdx.x * 256 + (int)threadIdx.x; e < total; e += stride) {
    if (e < a.num_seeds && e < a.num_src) a.src_ids[e] = a.seeds[e];
    if (e < a.count) {
      const int c = a.cols[e];
      int id = -1;                                   // a column outside [0, num_cols)
      if (c >= 0 && c < a.num_cols) {
        const int t = a.table[c];
        if (t < 0) {
          id = -t - 1;
        } else {
          id = a.num_seeds + a.rank[c] - 1;
          if (id >= a.num_seeds && id < a.num_src) a.src_ids[id] = c;
        }
      }
      a.local[e] = id;
    }
  }
}

// table[cols[e]] = 1 for every e < num_sampled with a column in [0, num_cols).  `table` (int32 [num_cols]) must be ZERO on entry.
inline int launch_block_mark(const int* cols, long long num_sampled, int num_cols, int* table, hipStream_t stream) {
  if (num_sampled < 0 || num_sampled > INT_MAX || num_cols < 0) return kErrBadShape;
  if (num_sampled == 0 || num_cols == 0) return kOk;
  if (bad_ptr(cols, 3) || bad_ptr(table, 3)) return kErrBadShape;
  hipLaunchKernelGGL(block_mark_kernel, dim3(block_grid(num_sampled)), dim3(256), 0, stream, cols, num_sampled, num_cols, table);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// table[seeds[i]] = -(i + 1), after launch_block_mark on the same stream
inline int launch_block_mark_seeds(const int* seeds, int num_seeds, int num_cols, int* table, hipStream_t stream) {
  if (num_seeds < 0 || num_cols < 0) return kErrBadShape;
  if (num_seeds == 0 || num_cols == 0) return kOk;
  if (bad_ptr(seeds, 3) || bad_ptr(table, 3)) return kErrBadShape;
  hipLaunchKernelGGL(block_mark_seeds_kernel, dim3(block_grid(num_seeds)), dim3(256), 0, stream, seeds, num_seeds, num_cols, table);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// num_src = num_seeds + rank[num_cols - 1].  Every element of local [num_sampled] and src_ids [num_src] is written; neither needs
// initialising.
inline int launch_block_relabel(const int* cols, long long num_sampled, const int* seeds, int num_seeds, const int* table,
                                const int* rank, int num_cols, int num_src, int* local, int* src_ids, hipStream_t stream) {
  if (num_sampled < 0 || num_sampled > INT_MAX || num_seeds < 0 || num_cols < 0 || num_src < num_seeds) return kErrBadShape;
  if (num_seeds == 0 && num_sampled == 0) return kOk;
  if (num_seeds > 0 && (bad_ptr(seeds, 3) || bad_ptr(src_ids, 3))) return kErrBadShape;
  if (num_sampled > 0 && (bad_ptr(cols, 3) || bad_ptr(local, 3) || bad_ptr(table, 3) || bad_ptr(rank, 3) || bad_ptr(src_ids, 3)))
    return kErrBadShape;
  const BlockRelabelArgs a{cols, seeds, table, rank, local, src_ids, num_sampled, num_seeds, num_cols, num_src};
  hipLaunchKernelGGL(block_relabel_kernel, dim3(block_grid(num_sampled > num_seeds ? num_sampled : num_seeds)), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

}  // namespace voltrix
