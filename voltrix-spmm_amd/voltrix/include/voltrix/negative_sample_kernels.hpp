// Voltrix-SpMM for MI355X (gfx950) -- negative sampling on a device CSR and the endpoints of CSR entries: what link-prediction
// mini-batches need next to neighbor_sample_kernels.hpp (the message-passing layers) and sddmm_kernels.hpp (the scores).
//   neg [S, k]    = for every position p of `src`, k columns drawn uniformly among those that do not occur in row src[p]
//   (rows, cols)  = for every CSR entry id, the row that holds it and its column
// No reference counterpart.  voltrix/negative.py and DESIGN.md 3.25 restate both contracts, tests/negative_oracle.py is the numpy
// restatement.
//
// THE NEGATIVE RULE.  src: int32 [S] GLOBAL row ids, duplicates allowed (several positive edges of one source are the normal case).
// k in 1 .. 1024 slots per position, T = max_tries in 1 .. 256 tries per slot, a 64-bit seed and a 64-bit offset, S k <= INT_MAX.
//   draw(p, q)    word q & 3 of Philox4x32-10(counter = (p, (q >> 2) | 0x40000000, offset & 0xffffffff, offset >> 32),
//                 key = (seed & 0xffffffff, seed >> 32)).  p is the POSITION in src, not the row id: duplicate sources get different
//                 negatives (the walker index of induced_subgraph_kernels.hpp does the same).  Bit 30 set with bit 31 clear is the
//                 last free domain of counter word 1: the dropout mask uses 00 (h >> 2 < 2^29), the neighbour sampler 10
//                 ((i >> 2) | 0x80000000), the walk 11 ((t >> 2) | 0xC0000000); q >> 2 < 2^16 here.  One seed for all four gives
//                 unrelated streams.
//   slot (p, j)   uses the draws q = j T + t for the tries t = 0 .. T - 1 (j T need not be a multiple of 4: the Philox block is
//                 evaluated at a slot's first use as well as where q & 3 == 0).  Try t proposes c = (uint64(draw(p, q)) * num_cols) >> 32;
//                 it is rejected if c occurs in row src[p], and, with exclude_self, if c == src[p].  neg[p, j] is the first accepted c,
//                 or -1 if all T tries are rejected (a full row: always).
// Slots are independent: one column may appear twice in a row of neg (DGL's sampler behaves the same way).  neg[p, j] is a function of
// (seed, offset, p, j, src[p], T, the graph) only -- not of the launch geometry, k or the other sources.  The multiply-shift's bias is
// at most num_cols / 2^32 relative.  A row id outside [0, num_rows) has degree 0 inside the kernel (never an out-of-bounds read;
// callers reject it).  Entries of `indices` outside [0, num_cols) never match a proposal and are never read through.  num_cols == 0:
// no column exists, every slot is -1.
// Membership.  SORTED = true is the PRECONDITION that every row's columns ascend (duplicates allowed): a binary search, O(T log d) per
// slot -- a hub row costs log d.  SORTED = false: a linear scan by the slot's one lane, O(T d): the slow path, not tuned.  On sorted
// input both give the same bits.
// negative_sample_kernel<SORTED>: one lane per (p, j), 256 per workgroup, the four Philox words read through selects (SampleDraws
// records why).  Every element of neg [S, k] is written, the -1 included.  No LDS, no scratch, no atomics.
//
// ENTRY -> ENDPOINTS.  The package keeps no [nnz] row-id array, so the row of entry e is a search: the one r with
// indptr[r] <= e < indptr[r + 1], found as the upper bound of e in indptr minus one -- runs of empty rows before and after are stepped
// over.  cols[i] = indices[e].  An id outside [0, num_entries) writes (-1, -1).  edge_endpoints_kernel: one lane per entry id,
// O(log num_rows) reads of indptr.
//
// KNOWN ANSWERS (tests/test_negative_host.py), src = [0, 0, 5, 99] on 100 nodes:
//   the ring with row v = {v + 1, v + 7, v + 31} mod 100, k = 4, T = 16:
//     seed 9, offset 0:                   [[38, 49, 82, 73], [29, 70, 90, 20], [99, 4, 63, 22], [21, 68, 11, 37]]
//     seed 2^40 + 9, offset 2^32 + 7:     [[24, 42, 80, 16], [72, 50, 67, 9], [40, 60, 94, 56], [66, 95, 96, 73]]
//   the band with row v = {v + 1 .. v + 60} mod 100, k = 3, T = 5 (slots start at q = 0, 5, 10: mid-block, and cross a block boundary):
//     seed 9, offset 0:                   [[67, 77, -1], [62, 74, 66], [99, 67, 83], [66, 71, 63]]   (position 0 proposes 38 36 7 67 86 |
//                                         2 77 74 86 4 | 16 32 5 47 37: the fourth, the second, none)
//     seed 2^40 + 9, offset 2^32 + 7:     [[96, 91, 79], [72, 71, 85], [66, 1, 85], [66, 71, 77]]
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "voltrix/dropout_mask_kernels.hpp"
#include "voltrix/launch_geometry.hpp"

namespace voltrix {

constexpr uint32_t kNegativeCounterBits = 0x40000000u;
constexpr int kNegativeMaxSlots = 1024;      // k
constexpr int kNegativeMaxTries = 256;       // T

// draw(p, q) for any sequence of q: one Philox evaluation per block of four that is touched, the first use included (a slot starts at
// q = j T, which need not be a multiple of 4)
struct NegativeDraws {
  uint32_t p, k0, k1, off0, off1;
  int have;                   // the block that `block` holds; -1: none yet
  Philox4 block;
  __host__ __device__ inline uint32_t operator()(int q) {
    const int b = q >> 2;
    if (b != have) {
      block = philox4x32_10(p, (uint32_t)b | kNegativeCounterBits, off0, off1, k0, k1);
      have = b;
    }
    const int w = q & 3;      // selects, not an indexed read (SampleDraws)
    return w == 0 ? block.x[0] : w == 1 ? block.x[1] : w == 2 ? block.x[2] : block.x[3];
  }
};

// whether column c occurs among the d entries of a row that begins at `row` (row = indices + indptr[r])
template <bool SORTED>
__host__ __device__ inline bool row_holds(const int* row, int d, int c) {
  if constexpr (SORTED) {
    int lo = 0, hi = d;       // the first position whose column is not below c
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (row[mid] < c) lo = mid + 1; else hi = mid;
    }
    return lo < d && row[lo] == c;
  } else {
    for (int i = 0; i < d; ++i)
      if (row[i] == c) return true;
    return false;
  }
}

// Slot j of position p whose source is row r, by the rule above: the accepted column, or -1.  The kernel and a host program run this
// code.
template <bool SORTED>
__host__ __device__ inline int negative_pick(const int* indptr, const int* indices, int num_rows, int num_cols, uint32_t p, int j, int r,
                                             int tries, bool exclude_self, uint32_t k0, uint32_t k1, uint32_t off0, uint32_t off1) {
  if (num_cols <= 0) return -1;
  const int* row = indices;
  int d = 0;
  if (r >= 0 && r < num_rows) {
    const int begin = indptr[r];
    d = indptr[r + 1] - begin;
    row = indices + begin;
  }
  NegativeDraws draw{p, k0, k1, off0, off1, -1, {}};
  const int first = j * tries;                // < 1024 * 256
  for (int t = 0; t < tries; ++t) {
    const int c = (int)(((uint64_t)draw(first + t) * (uint64_t)num_cols) >> 32);      // in [0, num_cols)
    if (exclude_self && c == r) continue;
    if (d > 0 && row_holds<SORTED>(row, d, c)) continue;
    return c;
  }
  return -1;
}

// The row that holds CSR entry e: the upper bound of e in indptr [num_rows + 1], minus one; -1 for e outside [0, num_entries) (and
// where indptr does not reach num_entries: never an out-of-bounds read).  The kernel and a host program run this code.
__host__ __device__ inline int entry_row(const int* indptr, int num_rows, long long num_entries, int e) {
  if (e < 0 || e >= num_entries) return -1;
  int lo = 0, hi = num_rows;                  // the first r with indptr[r + 1] > e
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (indptr[mid + 1] > e) hi = mid; else lo = mid + 1;
  }
  return lo < num_rows ? lo : -1;
}

struct NegativeSampleArgs {
  const int* indptr;     // [num_rows + 1]
  const int* indices;    // [entries]
  const int* src;        // [num_src] global row ids
  int* neg;              // [num_src, k]
  long long total;       // num_src * k
  int num_rows;
  int num_cols;
  int k;
  int tries;
  int exclude_self;
  uint32_t k0, k1;       // seed
  uint32_t off0, off1;   // offset
};

template <bool SORTED>
static __global__ __launch_bounds__(256) void negative_sample_kernel(const NegativeSampleArgs a) {
  const long long i = (long long)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= a.total) return;
  const int p = (int)(i / a.k);
  const int j = (int)(i - (long long)p * a.k);
  a.neg[i] = negative_pick<SORTED>(a.indptr, a.indices, a.num_rows, a.num_cols, (uint32_t)p, j, a.src[p], a.tries, a.exclude_self != 0,
                                   a.k0, a.k1, a.off0, a.off1);
}

static __global__ __launch_bounds__(256) void edge_endpoints_kernel(const int* indptr, const int* indices, const int* entries, int num_rows,
                                                                    long long num_entries, int num_ids, int* rows, int* cols) {
  const long long i = (long long)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= num_ids) return;
  const int e = entries[i];
  const int r = entry_row(indptr, num_rows, num_entries, e);
  rows[i] = r;
  cols[i] = r < 0 ? -1 : indices[e];
}

// neg = device int32 [num_src, k], every element written.  num_entries = the CSR's entry count (indices may be null only where it
// is 0).  num_src == 0: kOk without a launch.
inline int launch_negative_sample(const int* indptr, const int* indices, int num_rows, int num_cols, long long num_entries, const int* src,
                                  int num_src, int k, int max_tries, int exclude_self, int assume_sorted, uint64_t seed, uint64_t offset,
                                  int* neg, hipStream_t stream) {
  if (num_rows < 0 || num_cols < 0 || num_src < 0 || num_entries < 0 || num_entries > INT_MAX) return kErrBadShape;
  if (k < 1 || k > kNegativeMaxSlots || max_tries < 1 || max_tries > kNegativeMaxTries) return kErrBadShape;
  if ((exclude_self != 0 && exclude_self != 1) || (assume_sorted != 0 && assume_sorted != 1)) return kErrBadShape;
  const long long total = (long long)num_src * k;
  if (total > INT_MAX) return kErrBadShape;
  if (num_src == 0) return kOk;
  if (bad_ptr(indptr, 3) || bad_ptr(src, 3) || bad_ptr(neg, 3)) return kErrBadShape;
  if (num_entries > 0 ? bad_ptr(indices, 3) : misaligned(indices, 3)) return kErrBadShape;
  const NegativeSampleArgs a{indptr, indices, src, neg, total, num_rows, num_cols, k, max_tries, exclude_self,
                             (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
  const dim3 grid((unsigned)((total + 255) / 256));
  if (assume_sorted)
    hipLaunchKernelGGL((negative_sample_kernel<true>), grid, dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL((negative_sample_kernel<false>), grid, dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// rows, cols = device int32 [num_ids], every element written.  num_ids == 0: kOk without a launch.
inline int launch_edge_endpoints(const int* indptr, const int* indices, int num_rows, long long num_entries, const int* entries,
                                 int num_ids, int* rows, int* cols, hipStream_t stream) {
  if (num_rows < 0 || num_ids < 0 || num_entries < 0 || num_entries > INT_MAX) return kErrBadShape;
  if (num_ids == 0) return kOk;
  if (bad_ptr(indptr, 3) || bad_ptr(entries, 3) || bad_ptr(rows, 3) || bad_ptr(cols, 3)) return kErrBadShape;
  if (num_entries > 0 ? bad_ptr(indices, 3) : misaligned(indices, 3)) return kErrBadShape;
  hipLaunchKernelGGL(edge_endpoints_kernel, dim3((unsigned)(((long long)num_ids + 255) / 256)), dim3(256), 0, stream, indptr, indices,
                     entries, num_rows, num_entries, num_ids, rows, cols);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

}  // namespace voltrix
