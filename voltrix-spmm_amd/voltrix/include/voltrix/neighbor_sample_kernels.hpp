// Voltrix-SpMM for MI355X (gfx950) -- neighbour sampling on a device CSR and the relabelling of a sampled block:
//   (s_indices, s_entries) = for every seed row, at most `fanout` of its entries that are not in `exclude` (their column ids and their
//                            CSR entry ids)
//   (src_ids, local)       = the block's source nodes -- the seeds first, then the other sampled columns in ascending id -- and
//                            every sampled column as a position in src_ids
// What produces the rectangular [num_dst, num_src] patterns that every CSR operator here takes (spmm_csr_*, sddmm, attn_aggregate,
// spmm_csr_reduce): GraphSAGE-style mini-batches; the exclusion list keeps the edges (and their reverses) a link-prediction decoder is
// asked to predict out of the blocks its encoder aggregates over (DGL's exclude="reverse_id").  No reference counterpart.
//
// THE SAMPLING RULE (the contract; voltrix/sampling.py and DESIGN.md 3.23 / 3.26 restate it, tests/sample_oracle.py and
// tests/exclude_oracle.py are the numpy restatements).  A seed row r (its GLOBAL row id) with begin = indptr[r], end = indptr[r + 1],
// d = end - begin; fan-out k; a 64-bit seed and a 64-bit offset; exclude: int32 [X] CSR entry ids, STRICTLY ASCENDING (sorted,
// distinct), each in [0, nnz).
//   the candidates   lo = lower_bound(exclude, begin), hi = lower_bound(exclude, end), x = hi - lo.  The excluded positions of the row
//                are q_i = exclude[lo + i] - begin, i = 0 .. x - 1, ascending; the CANDIDATES are the d' = d - x positions of the row
//                not among them, in CSR order.  Candidate number t is position cand(t) = t + #{ i : q_i - i <= t }; q_i - i does not
//                decrease, so cand(t) is one binary search over the row's slice of exclude: O(log x).  Everything below selects
//                candidate NUMBERS in 0 .. d' - 1 and outputs them through cand.
//                x = 0 -- NO LIST (null or X = 0, the plain call), or a row none of whose entries is excluded: d' = d and
//                cand(t) = t.  Such a row gets the same bits with and without a list.
//   draw(r, i)   word i & 3 of Philox4x32-10(counter = (r, (i >> 2) | 0x80000000, offset & 0xffffffff, offset >> 32),
//                key = (seed & 0xffffffff, seed >> 32)).  Bit 31 of counter word 1 separates these draws from the dropout mask's
//                (edge, h >> 2, ...) counters (dropout_mask_kernels.hpp: h >> 2 < 2^29), so one seed for both gives unrelated streams.
//   without replacement, d' <= k  every candidate, in CSR order; no draw is used.  "all" (fan-out kSampleAll, Python's fanout=None)
//                means this for every row, with or without replacement.
//   without replacement, d' > k   Floyd's algorithm on 0 .. d' - 1: for i = 0 .. k - 1, j = d' - k + i,
//                t = (uint64(draw(r, i)) * (j + 1)) >> 32; take t unless it is taken already, then take j.  The k numbers are output
//                in ASCENDING order and cand ascends: a sampled row keeps CSR order, sorted rows stay sorted.  Every k-subset is equally
//                likely up to the multiply-shift's bias: t's values differ in probability by at most a relative (j + 1) / 2^32
//                <= d / 2^32.
//   with replacement, d' > 0      exactly k entries; entry i is cand((uint64(draw(r, i)) * d') >> 32), in draw order.  d' == 0: none.
// The result is a function of (seed, offset, r, d', k) and the row's excluded positions only -- not of the other seeds of the batch,
// their order or the launch geometry; s_entries holds ids into the ORIGINAL indices.
//
// sample_neighbors_kernel<REPLACE, EXCLUDE>: one lane per seed row, 256 lanes per workgroup, one body (sample_row) for every call.
// EXCLUDE = false is what a launch without a list gets: x = 0 at compile time, so the searches and the merge fold away and the plain
// call runs the instructions it always ran (with x = 0 only at run time its launches without replacement took 2 - 8 % longer:
// DESIGN.md 3.26).  Per row O(k^2) compares and k four-byte gathers from `indices`, with a list two binary searches in exclude
// (O(log X)) and one per output entry (O(log x)) on top -- not a function of the degree: a 67k-entry hub row costs what a row of
// degree k + 1 costs (no hub-row weakness, unlike the row-per-group kernels).  The sorted numbers of Floyd's algorithm live in dynamic LDS, slot-major: slot[j * 256 + lane] -- bank lane mod 32 for every j, so lanes
// that insert at different depths do not conflict; 256 k 4 bytes, k <= 64 (64 KiB: two workgroups per CU).  No per-lane array in
// registers, hence no scratch.  The replacement path and "all" use no LDS.  "all" and d' <= k walk the row against its slice of exclude
// with the row's one lane: O(d) per lane there, the one path whose cost follows the degree.
// A seed outside [0, num_rows) has degree 0 inside the kernel (never an out-of-bounds read); a row never writes more than its segment
// s_indptr[i + 1] - s_indptr[i] holds, and with d' = max(d - x, 0) and cand(t) <= t + x every read of indices stays inside the row
// whatever exclude holds (a list that is not strictly ascending gives unspecified entries of the row, never an out-of-bounds access).
//
// KNOWN ANSWERS (tests/test_exclude_host.py): the ring with row v = {v + 1, v + 7, v + 31} mod 100, exclude = [0, 15] (the first entry
// of rows 0 and 5), seeds = [0, 5, 99, 0, 42], k = 2, seed 9, offset 0.  Rows 0 and 5 have d' = 2; rows 99 and 42 have nothing
// excluded and get the bits of the call without a list.  s_indptr = [0, 2, 4, 6, 8, 10] both times.
//   without replacement:   s_indices [7, 31, 12, 36, 6, 30, 7, 31, 43, 49], s_entries [1, 2, 16, 17, 298, 299, 1, 2, 126, 127]
//   with replacement:      s_indices [7, 31, 36, 36, 30, 6, 7, 31, 49, 49], s_entries [1, 2, 17, 17, 299, 298, 1, 2, 127, 127]
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

// the first index in [0, n) of the ascending list `list` whose value is not below v; n if there is none
__host__ __device__ inline int exclude_lower_bound(const int* list, int n, int v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (list[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// x, the number of entries of the row [begin, end) that `exclude` [num_exclude] holds, and in *first the index lo of the first of
// them: the row's slice is exclude[lo .. lo + x).  Never negative, whatever the list holds; num_exclude == 0: 0, and nothing is read.
__host__ __device__ inline int exclude_row_count(const int* exclude, int num_exclude, int begin, int end, int* first) {
  const int lo = exclude_lower_bound(exclude, num_exclude, begin);
  const int hi = lo + exclude_lower_bound(exclude + lo, num_exclude - lo, end);
  *first = lo;
  return hi - lo;
}

// cand(t): the position in the row of candidate number t.  `slice` = the row's x excluded entry ids, ascending; begin = indptr[r].
// q_i - i with q_i = slice[i] - begin does not decrease: the count of i with q_i - i <= t is the first i where it is above t.
// x == 0: t, and nothing is read.
__host__ __device__ inline int exclude_cand(const int* slice, int x, int begin, int t) {
  int lo = 0, hi = x;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (slice[mid] - begin - mid <= t) lo = mid + 1; else hi = mid;
  }
  return t + lo;
}

// One seed row by the rule above: row r = entries [begin, begin + d) with d > 0, fan-out k (INT_MAX: "all"), room > 0 elements in
// out_col / out_entry; exclude [num_exclude], (nullptr, 0) for no list.  EXCLUDE = false promises num_exclude == 0 and gives the same
// bits as EXCLUDE = true does then.  `slot` as for sample_row_positions (used only where d' > k without replacement).  The kernel and
// the host programs of the tests run this code.
template <bool REPLACE, bool EXCLUDE = true, class Slots>
__host__ __device__ inline void sample_row(const int* indices, const int* exclude, int num_exclude, uint32_t r, int begin, int d, int k,
                                           int room, uint32_t k0, uint32_t k1, uint32_t off0, uint32_t off1, Slots& slot, int* out_col,
                                           int* out_entry) {
  int first = 0;
  const int x = EXCLUDE ? exclude_row_count(exclude, num_exclude, begin, begin + d, &first) : 0;
  const int* const slice = exclude + first;          // the row's excluded entry ids
  const int dc = d - x;                              // d': the candidates
  if (dc <= 0) return;
  if (k == INT_MAX || (!REPLACE && dc <= k)) {       // every candidate, in CSR order: the row merged against its slice
    const int count = dc < room ? dc : room;
    int next = 0, written = 0;
    for (int j = 0; j < d && written < count; ++j) {
      if (next < x && slice[next] == begin + j) {
        ++next;
        continue;
      }
      out_entry[written] = begin + j;
      out_col[written] = indices[(long long)begin + j];
      ++written;
    }
    return;
  }
  const int count = k < room ? k : room;             // == k for an s_indptr made by the rule
  if constexpr (REPLACE) {
    SampleDraws draw{r, k0, k1, off0, off1, {}};
    for (int j = 0; j < k; ++j) {
      const int e = begin + exclude_cand(slice, x, begin, sample_replace_position(draw(j), dc));
      if (j < count) {
        out_entry[j] = e;
        out_col[j] = indices[e];
      }
    }
  } else {
    sample_row_positions(r, dc, k, k0, k1, off0, off1, slot);
    for (int j = 0; j < count; ++j) {
      const int e = begin + exclude_cand(slice, x, begin, slot.get(j));
      out_entry[j] = e;
      out_col[j] = indices[e];
    }
  }
}

struct SampleNeighborsArgs {
  const int* indptr;     // [num_rows + 1]
  const int* indices;    // [entries]
  const int* seeds;      // [num_seeds] global row ids
  const int* s_indptr;   // [num_seeds + 1] where every seed's entries go
  const int* exclude;    // [num_exclude] CSR entry ids, strictly ascending; may be null where num_exclude == 0
  int* s_indices;        // [num_sampled] global column ids
  int* s_entries;        // [num_sampled] CSR entry ids
  int num_rows;
  int num_seeds;
  int num_exclude;
  int k;                 // 1 .. 64, or INT_MAX for "all"
  uint32_t k0, k1;       // seed
  uint32_t off0, off1;   // offset
};

struct LdsSlots {
  int* base;             // this lane's column of the slot-major array
  __device__ inline int get(int j) const { return base[j * 256]; }
  __device__ inline void set(int j, int v) { base[j * 256] = v; }
};

template <bool REPLACE, bool EXCLUDE>
static __global__ __launch_bounds__(256) void sample_neighbors_kernel(const SampleNeighborsArgs a) {
  extern __shared__ __attribute__((aligned(16))) int sample_slots[];          // [k][256], only where a row has d' > k
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
  if (d <= 0 || room <= 0) return;
  LdsSlots slot{sample_slots + (int)threadIdx.x};
  sample_row<REPLACE, EXCLUDE>(a.indices, a.exclude, a.num_exclude, (uint32_t)r, begin, d, a.k, room, a.k0, a.k1, a.off0, a.off1, slot,
                      a.s_indices + base, a.s_entries + base);
}

// fanout: 1 .. 64, or kSampleAll.  exclude = device int32 [num_exclude], strictly ascending ids in [0, entries) (not checked on the
// device); (nullptr, 0): no list.  s_indptr must be the rule's: s_indptr[i + 1] - s_indptr[i] = min(d'_i, fanout) without
// replacement, (d'_i > 0 ? fanout : 0) with it, d'_i for kSampleAll, d'_i = 0 for a seed outside [0, num_rows); num_sampled =
// s_indptr[num_seeds].  Every element of s_indices and s_entries is written then; neither needs initialising.  Nothing else is checked
// on the device.
inline int launch_sample_neighbors(const int* indptr, const int* indices, int num_rows, const int* seeds, int num_seeds,
                                   const int* s_indptr, long long num_sampled, int fanout, int replace, uint64_t seed, uint64_t offset,
                                   const int* exclude, int num_exclude, int* s_indices, int* s_entries, hipStream_t stream) {
  if (num_rows < 0 || num_seeds < 0 || num_exclude < 0 || num_sampled < 0 || num_sampled > INT_MAX) return kErrBadShape;
  if (fanout != kSampleAll && (fanout < 1 || fanout > kSampleMaxFanout)) return kErrBadShape;
  if (replace != 0 && replace != 1) return kErrBadShape;
  if (num_seeds == 0) return kOk;
  if (bad_ptr(indptr, 3) || bad_ptr(seeds, 3) || bad_ptr(s_indptr, 3)) return kErrBadShape;
  if (num_exclude > 0 ? bad_ptr(exclude, 3) : misaligned(exclude, 3)) return kErrBadShape;
  if (num_sampled > 0 && (bad_ptr(indices, 3) || bad_ptr(s_indices, 3) || bad_ptr(s_entries, 3))) return kErrBadShape;
  if (num_sampled == 0) return kOk;                  // nothing to write
  const bool all = fanout == kSampleAll;
  const SampleNeighborsArgs a{indptr, indices, seeds, s_indptr, exclude, s_indices, s_entries, num_rows, num_seeds, num_exclude,
                              all ? INT_MAX : fanout, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
  const dim3 grid((unsigned)(((long long)num_seeds + 255) / 256));
  const size_t lds = (size_t)256 * fanout * sizeof(int);
  if (replace || all)
    hipLaunchKernelGGL((num_exclude > 0 ? sample_neighbors_kernel<true, true> : sample_neighbors_kernel<true, false>), grid, dim3(256),
                       0, stream, a);
  else
    hipLaunchKernelGGL((num_exclude > 0 ? sample_neighbors_kernel<false, true> : sample_neighbors_kernel<false, false>), grid,
                       dim3(256), lds, stream, a);
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
