// Voltrix-SpMM for MI355X (gfx950) -- weighted neighbour sampling on a device CSR: for every seed row, at most `fanout` of its entries,
// drawn with probability proportional to a non-negative weight per entry (DGL's sample_neighbors(prob=)): importance sampling,
// edge-weight-biased GraphSAGE, masking entries with zero weights.  No reference counterpart.  Integers only: no transcendental function
// and no floating-point compare takes part in a draw, so a numpy restatement (tests/weighted_sample_oracle.py) reproduces every bit.
//
// THE WEIGHT TABLE (the contract; voltrix/sampling.py::sampling_weights builds it, DESIGN.md 3.27 and include/voltrix_capi.h restate
// it).  For an entry e of row r with weight w_e >= 0 (finite) and m_r = the maximum weight of the row, in float64:
//   q_e = 0                                   where w_e == 0 or m_r == 0
//   q_e = max(1, floor((w_e / m_r) * 2^30))   otherwise: one correctly rounded division, an exact multiplication, an exact floor
// so 0 <= q_e <= 2^30, a positive weight stays positive, a zero weight is never sampled, and q_e / 2^30 is within 2^-30 of w_e / m_r.
//   cum   int64 [nnz]: the inclusive prefix sum of q over the WHOLE entry array (at most nnz 2^30 < 2^61: no overflow); 8 bytes per entry
// This header reads cum only; the per-row count of positive entries reaches it through s_indptr (below).
//
// THE SAMPLING RULE.  Row r with begin = indptr[r], d = indptr[r + 1] - begin; fan-out k; a 64-bit seed and a 64-bit offset.
//   base = begin > 0 ? cum[begin - 1] : 0 (cum[-1] is never read);  c(j) = cum[begin + j] - base;  T = c(d - 1);
//   p = the number of entries of the row with q > 0.
//   draw(r, n)   word n & 3 of Philox4x32-10(counter = (r, (n >> 2) | 0xA0000000, offset & 0xffffffff, offset >> 32),
//                key = (seed & 0xffffffff, seed >> 32)), n < 128.  Bits 31 and 29 of counter word 1: a sub-domain of the neighbour
//                sampler's 10 domain that the uniform rule (0x80000000 | (i >> 2), i < 64) never enters; dropout (00), negative sampling
//                (01) and walks (11) are elsewhere.
//   x_i = (uint64(draw(r, 2 i)) << 32) | draw(r, 2 i + 1);  a uniform integer below R is umulhi64(x_i, R) = (x_i R) >> 64
//                (__umul64hi on the device, unsigned __int128 on the host): an entry's probability differs from q_e / R by less than 2^-63.
//   without replacement, p <= k   every entry with q > 0, in CSR order; no draw is used.  "all" (fan-out kSampleAll, Python's
//                fanout=None) means this for every row, with or without replacement.
//   without replacement, p > k    successive sampling: for i = 0 .. k - 1, R_i = T - (the sum of q over the entries chosen so far),
//                t = umulhi64(x_i, R_i); choose the smallest position j with g(j) > t, g(j) = c(j) - (the sum of q_s over chosen s <= j).
//                g does not decrease and is flat at chosen positions and at zero weights: j is never chosen already and never has
//                q = 0.  The k positions are output in ASCENDING order: sorted rows stay sorted, as under the uniform rule.
//   with replacement, T > 0       exactly k entries; entry i is at the smallest j with c(j) > umulhi64(x_i, T), in draw order.  T == 0: none.
// The result is a function of (seed, offset, r, k) and the row's q values only.  Equal weights do NOT reproduce the uniform rule's bits.
//
// HOW.  One lane per seed row, 256 lanes per workgroup, as sample_neighbors_kernel.  The chosen positions stay sorted in the lane's
// LdsSlots column (slot[j * 256 + lane], 256 k 4 bytes of dynamic LDS, k <= 64; the replacement path and "all" use none).  Draw i walks
// them in ascending order with the removed mass `rem`: for chosen s, q_s = c(s) - c(s - 1); if c(s) - q_s - rem > t the answer lies in
// the gap before s, else rem += q_s; after the last one the gap is (s_last, d).  Inside the gap a binary search finds the smallest j
// with c(j) > t + rem.  Per row O(k (k + log d)) loads of cum whatever the degree; no trip count depends on a draw (the bounds are k
// and ceil(log2 d)): a row dominated by one weight, on which a rejection loop would spin, costs what any row costs.  No per-lane
// register array (no scratch), no atomics.
// The kernel has no p: the caller's segment s_indptr[i + 1] - s_indptr[i] carries it.  A segment below k says p < k (every positive
// entry: each is found from the one before by a galloping search for the smallest j with c(j) > c(s), O(log gap) per entry, O(d) at
// worst for "all"); a segment of k is drawn by successive sampling, which for p == k chooses every positive entry -- the bits of the
// rule's "every entry with q > 0".  A seed outside [0, num_rows) has degree 0; a row never writes past its segment; every read of cum
// and indices stays inside the row, whatever cum and s_indptr hold (a wrong table gives unspecified entries of the row, never an
// out-of-bounds access or a longer loop).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "voltrix/neighbor_sample_kernels.hpp"

namespace voltrix {

constexpr uint32_t kWeightedCounterBits = 0xA0000000u;

__host__ __device__ inline uint64_t umulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// x_i for i = 0, 1, 2, ...: SampleDraws in the weighted sub-domain, one Philox evaluation per two 64-bit draws
struct WeightedDraws {
  uint32_t r, k0, k1, off0, off1;
  Philox4 block;
  __host__ __device__ inline uint64_t operator()(int i) {
    if ((i & 1) == 0) block = philox4x32_10(r, (uint32_t)(i >> 1) | kWeightedCounterBits, off0, off1, k0, k1);
    return (i & 1) == 0 ? ((uint64_t)block.x[0] << 32) | block.x[1] : ((uint64_t)block.x[2] << 32) | block.x[3];
  }
};

// c(j) of one row: row = cum + begin, base = cum[begin - 1] (0 for begin == 0)
struct RowMass {
  const long long* row;
  long long base;
  __host__ __device__ inline long long operator()(int j) const { return row[j] - base; }
};

// the smallest j in [lo, hi] with c(j) > v, for lo <= hi and c(hi) > v: at most ceil(log2(hi - lo + 1)) loads
__host__ __device__ inline int weighted_upper_bound(const RowMass& c, int lo, int hi, long long v) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (c(mid) > v) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// the smallest j in (s, d) with c(j) > v, d if there is none: probes s + 1, then at doubling strides, then searches the last stride --
// one load where the next entry is positive, O(log gap) otherwise; both loops run at most 32 times
__host__ __device__ inline int weighted_next_above(const RowMass& c, int s, int d, long long v) {
  int lo = s + 1, step = 1;
  if (lo >= d) return d;
  int hi = lo;
  while (c(hi) <= v) {
    lo = hi + 1;
    if (lo >= d) return d;
    hi = d - 1 - lo < step ? d - 1 : lo + step;
    if (step < (1 << 29)) step <<= 1;
  }
  return weighted_upper_bound(c, lo, hi, v);
}

// Successive sampling of the rule above: `count` positions of a row with T = c(d - 1), left ascending in slot.get(0 .. n - 1); returns
// n, which is `count` where the row has at least `count` positive entries.  `slot` as for sample_row_positions.
template <class Slots>
__host__ __device__ inline int weighted_row_positions(const RowMass& c, int d, int count, WeightedDraws& draw, Slots& slot) {
  long long remaining = c(d - 1);                    // R_i
  for (int i = 0; i < count; ++i) {
    if (remaining <= 0) return i;                    // fewer positive entries than the segment asks for: not the rule's s_indptr
    const long long t = (long long)umulhi64(draw(i), (uint64_t)remaining);
    long long rem = 0;                               // the mass of the chosen positions below the gap
    int m = 0, lo = 0, hi = d - 1;
    for (; m < i; ++m) {
      const int s = slot.get(m);
      const long long before = s > 0 ? c(s - 1) : 0;
      if (before - rem > t) {                        // g(s - 1) > t: the answer is in the gap before s
        hi = s - 1;
        break;
      }
      rem += c(s) - before;
      lo = s + 1;
    }
    int j = lo <= hi ? weighted_upper_bound(c, lo, hi, t + rem) : hi;
    j = j < 0 ? 0 : j > d - 1 ? d - 1 : j;           // a no-op on a table made by the rule
    for (int n = i; n > m; --n) slot.set(n, slot.get(n - 1));
    slot.set(m, j);
    remaining -= c(j) - (j > 0 ? c(j - 1) : 0);
  }
  return count;
}

// One seed row by the rule above: row r = entries [begin, begin + d) with d > 0, fan-out k (INT_MAX: "all"), room > 0 elements in
// out_col / out_entry (min(p, k); T > 0 ? k : 0 with replacement; p for "all").  The kernel and the host program of the tests run this.
template <bool REPLACE, class Slots>
__host__ __device__ inline void weighted_sample_row(const int* indices, const long long* cum, uint32_t r, int begin, int d, int k, int room,
                                                    uint32_t k0, uint32_t k1, uint32_t off0, uint32_t off1, Slots& slot, int* out_col,
                                                    int* out_entry) {
  const RowMass c{cum + begin, begin > 0 ? cum[(long long)begin - 1] : 0};
  const long long total = c(d - 1);                  // T
  if (total <= 0) return;
  if (k == INT_MAX || (!REPLACE && room < k)) {      // every entry with q > 0, in CSR order
    long long below = 0;
    for (int s = -1, written = 0; written < room; ++written) {
      s = weighted_next_above(c, s, d, below);
      if (s >= d) return;
      below = c(s);
      out_entry[written] = begin + s;
      out_col[written] = indices[(long long)begin + s];
    }
    return;
  }
  const int count = k < room ? k : room;             // == k for an s_indptr made by the rule
  WeightedDraws draw{r, k0, k1, off0, off1, {}};
  if constexpr (REPLACE) {
    for (int i = 0; i < count; ++i) {
      const int e = begin + weighted_upper_bound(c, 0, d - 1, (long long)umulhi64(draw(i), (uint64_t)total));
      out_entry[i] = e;
      out_col[i] = indices[e];
    }
  } else {
    const int n = weighted_row_positions(c, d, count, draw, slot);
    for (int j = 0; j < n; ++j) {
      const int e = begin + slot.get(j);
      out_entry[j] = e;
      out_col[j] = indices[e];
    }
  }
}

struct WeightedSampleArgs {
  const int* indptr;     // [num_rows + 1]
  const int* indices;    // [entries]
  const long long* cum;  // [entries] the weight table
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

template <bool REPLACE>
static __global__ __launch_bounds__(256) void sample_neighbors_weighted_kernel(const WeightedSampleArgs a) {
  extern __shared__ __attribute__((aligned(16))) int weighted_slots[];        // [k][256], only without replacement
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
  LdsSlots slot{weighted_slots + (int)threadIdx.x};
  weighted_sample_row<REPLACE>(a.indices, a.cum, (uint32_t)r, begin, d, a.k, room, a.k0, a.k1, a.off0, a.off1, slot, a.s_indices + base,
                               a.s_entries + base);
}

// the launch's dynamic LDS: the slots of the path without replacement, none elsewhere
constexpr size_t weighted_sample_lds_bytes(int fanout, int replace) {
  return replace || fanout == kSampleAll ? 0 : (size_t)256 * fanout * sizeof(int);
}

// fanout: 1 .. 64, or kSampleAll.  cum = device int64 [entries], the weight table of the rule.  s_indptr must be the rule's:
// s_indptr[i + 1] - s_indptr[i] = min(p_i, fanout) without replacement, (T_i > 0 ? fanout : 0) with it, p_i for kSampleAll, 0 for a
// seed outside [0, num_rows); num_sampled = s_indptr[num_seeds].  Every element of s_indices and s_entries is written then; neither
// needs initialising.  Nothing else is checked on the device.
inline int launch_sample_neighbors_weighted(const int* indptr, const int* indices, const long long* cum, int num_rows, const int* seeds,
                                            int num_seeds, const int* s_indptr, long long num_sampled, int fanout, int replace,
                                            uint64_t seed, uint64_t offset, int* s_indices, int* s_entries, hipStream_t stream) {
  if (num_rows < 0 || num_seeds < 0 || num_sampled < 0 || num_sampled > INT_MAX) return kErrBadShape;
  if (fanout != kSampleAll && (fanout < 1 || fanout > kSampleMaxFanout)) return kErrBadShape;
  if (replace != 0 && replace != 1) return kErrBadShape;
  if (num_seeds == 0) return kOk;
  if (bad_ptr(indptr, 3) || bad_ptr(seeds, 3) || bad_ptr(s_indptr, 3)) return kErrBadShape;
  if (num_sampled > 0 && (bad_ptr(indices, 3) || bad_ptr(cum, 7) || bad_ptr(s_indices, 3) || bad_ptr(s_entries, 3))) return kErrBadShape;
  if (num_sampled == 0) return kOk;                  // nothing to write
  const WeightedSampleArgs a{indptr, indices, cum, seeds, s_indptr, s_indices, s_entries, num_rows, num_seeds,
                             fanout == kSampleAll ? INT_MAX : fanout, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset,
                             (uint32_t)(offset >> 32)};
  const dim3 grid((unsigned)(((long long)num_seeds + 255) / 256));
  const size_t lds = weighted_sample_lds_bytes(fanout, replace);
  if (replace)
    hipLaunchKernelGGL(sample_neighbors_weighted_kernel<true>, grid, dim3(256), lds, stream, a);
  else
    hipLaunchKernelGGL(sample_neighbors_weighted_kernel<false>, grid, dim3(256), lds, stream, a);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

}  // namespace voltrix
