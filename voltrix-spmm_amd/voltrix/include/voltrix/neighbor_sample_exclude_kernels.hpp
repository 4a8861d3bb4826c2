// Voltrix-SpMM for MI355X (gfx950) -- neighbour sampling that leaves a given set of CSR entries out, and the lookup from (row, column)
// to the CSR entry id: what link-prediction mini-batches need so that the encoder does not aggregate over the edges (and their
// reverses) the decoder is asked to predict (DGL's exclude="reverse_id", edge_ids / has_edges_between).
//   (s_indices, s_entries) = for every seed row, at most `fanout` of its entries that are NOT in `exclude`
//   out [Q]                = for every query (rows[i], cols[i]), the id of the first entry of that row with that column, or -1
// No reference counterpart.  voltrix/sampling.py, voltrix/negative.py and DESIGN.md 3.26 restate both contracts,
// tests/exclude_oracle.py is the numpy restatement.
//
// THE EXCLUSION RULE.  exclude: int32 [X] CSR entry ids, STRICTLY ASCENDING (sorted, distinct), each in [0, nnz).  For a seed row r
// with begin = indptr[r], end = indptr[r + 1], d = end - begin:
//   lo = lower_bound(exclude, begin), hi = lower_bound(exclude, end), x = hi - lo
//   the excluded positions of the row are q_i = exclude[lo + i] - begin, i = 0 .. x - 1, ascending
//   the CANDIDATES are the d' = d - x positions of the row not among the q_i, in CSR order
//   candidate number t is position cand(t) = t + #{ i : q_i - i <= t }; q_i - i does not decrease, so cand(t) is one binary search
//   over the row's slice of exclude: O(log x)
// The sampling rule of neighbor_sample_kernels.hpp then applies UNCHANGED WITH d' IN PLACE OF d, every position it yields mapped
// through cand:
//   without replacement, d' <= k   every candidate, in CSR order; "all" (fan-out kSampleAll) means this for every row
//   without replacement, d' > k    Floyd's algorithm on 0 .. d' - 1: the same sample_row_positions, the same draw(r, i), the same
//                                  counter domain 10 (no new Philox domain is needed, and none is left).  cand ascends, so the output does
//   with replacement, d' > 0       k entries at cand((uint64(draw(r, i)) * d') >> 32), in draw order
//   d' = 0                         nothing
// So: a row none of whose entries is excluded gets exactly the bits the plain kernel gives it; the result is a function of
// (seed, offset, r, d', k) and the row's excluded positions only; sorted rows stay sorted; s_entries still holds ids into the
// ORIGINAL indices.
//
// sample_neighbors_excluding_kernel<REPLACE>: one lane per seed, 256 per workgroup, the dynamic-LDS slot layout of
// sample_neighbors_kernel.  It differs from that kernel by two binary searches in exclude per row (O(log X)) and one per output entry
// (O(log x)): the cost still does not follow the degree.  "all" and d' <= k are a merge walk of the row against its slice of exclude:
// O(d) by the row's one lane, as there.  A seed outside [0, num_rows) has degree 0; a row never writes more than its segment
// s_indptr[i + 1] - s_indptr[i] holds, and with d' = max(d - x, 0) and cand(t) <= t + x every read of indices stays inside the row
// whatever exclude holds (a list that is not strictly ascending gives unspecified entries of the row, never an out-of-bounds access).
//
// (ROW, COLUMN) -> ENTRY.  The package keeps no [nnz] key array, so this is a search, like entry_row:
// find_entry<SORTED>(r, c) is the id of the FIRST entry of row r whose column is c, or -1 if there is none or r is outside
// [0, num_rows).  SORTED = true is the precondition of negative_sample (every row's columns ascend, duplicates allowed): a lower
// bound, O(log d).  SORTED = false: a linear scan by the query's one lane, O(d): the slow path, not tuned.  On sorted input both give
// the same bits.  find_edges_kernel<SORTED>: one lane per query; every element of out is written.
//
// No atomics anywhere; offsets that can pass 2^31 are 64-bit; no host synchronisation.
//
// KNOWN ANSWERS (tests/test_exclude_host.py): the ring with row v = {v + 1, v + 7, v + 31} mod 100, exclude = [0, 15] (the first entry
// of rows 0 and 5), seeds = [0, 5, 99, 0, 42], k = 2, seed 9, offset 0.  Rows 0 and 5 have d' = 2; rows 99 and 42 have nothing
// excluded and get the plain rule's bits.  s_indptr = [0, 2, 4, 6, 8, 10] both times.
//   without replacement:   s_indices [7, 31, 12, 36, 6, 30, 7, 31, 43, 49], s_entries [1, 2, 16, 17, 298, 299, 1, 2, 126, 127]
//   with replacement:      s_indices [7, 31, 36, 36, 30, 6, 7, 31, 49, 49], s_entries [1, 2, 17, 17, 299, 298, 1, 2, 127, 127]
#pragma once

#include "voltrix/neighbor_sample_kernels.hpp"

namespace voltrix {

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
// them: the row's slice is exclude[lo .. lo + x).  Never negative, whatever the list holds.
__host__ __device__ inline int exclude_row_count(const int* exclude, int num_exclude, int begin, int end, int* first) {
  const int lo = exclude_lower_bound(exclude, num_exclude, begin);
  const int hi = lo + exclude_lower_bound(exclude + lo, num_exclude - lo, end);
  *first = lo;
  return hi - lo;
}

// cand(t): the position in the row of candidate number t.  `slice` = the row's x excluded entry ids, ascending; begin = indptr[r].
// q_i - i with q_i = slice[i] - begin does not decrease: the count of i with q_i - i <= t is the first i where it is above t.
__host__ __device__ inline int exclude_cand(const int* slice, int x, int begin, int t) {
  int lo = 0, hi = x;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (slice[mid] - begin - mid <= t) lo = mid + 1; else hi = mid;
  }
  return t + lo;
}

// The id of the first entry of row r whose column is c, or -1.  The kernel and a host program run this code.
template <bool SORTED>
__host__ __device__ inline int find_entry(const int* indptr, const int* indices, int num_rows, int r, int c) {
  if (r < 0 || r >= num_rows) return -1;
  const int begin = indptr[r];
  const int d = indptr[r + 1] - begin;
  const int* row = indices + begin;
  if constexpr (SORTED) {
    int lo = 0, hi = d;       // the first position whose column is not below c
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (row[mid] < c) lo = mid + 1; else hi = mid;
    }
    return lo < d && row[lo] == c ? begin + lo : -1;
  } else {
    for (int i = 0; i < d; ++i)
      if (row[i] == c) return begin + i;
    return -1;
  }
}

// One seed row by the rule above: row r = entries [begin, begin + d) with d > 0, fan-out k (INT_MAX: "all"), room > 0 elements in
// out_col / out_entry.  `slot` as for sample_row_positions (used only where d' > k without replacement).  The kernel and a host program
// run this code.
template <bool REPLACE, class Slots>
__host__ __device__ inline void sample_row_excluding(const int* indices, const int* exclude, int num_exclude, uint32_t r, int begin, int d,
                                                     int k, int room, uint32_t k0, uint32_t k1, uint32_t off0, uint32_t off1, Slots& slot,
                                                     int* out_col, int* out_entry) {
  int first = 0;
  const int x = exclude_row_count(exclude, num_exclude, begin, begin + d, &first);
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

struct SampleExcludingArgs {
  const int* indptr;     // [num_rows + 1]
  const int* indices;    // [entries]
  const int* seeds;      // [num_seeds] global row ids
  const int* s_indptr;   // [num_seeds + 1] where every seed's entries go
  const int* exclude;    // [num_exclude] CSR entry ids, strictly ascending
  int* s_indices;        // [num_sampled] global column ids
  int* s_entries;        // [num_sampled] CSR entry ids
  int num_rows;
  int num_seeds;
  int num_exclude;
  int k;                 // 1 .. 64, or INT_MAX for "all"
  uint32_t k0, k1;       // seed
  uint32_t off0, off1;   // offset
};

template <bool REPLACE>
static __global__ __launch_bounds__(256) void sample_neighbors_excluding_kernel(const SampleExcludingArgs a) {
  extern __shared__ __attribute__((aligned(16))) int sample_exclude_slots[];  // [k][256], only where a row has d' > k
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
  LdsSlots slot{sample_exclude_slots + (int)threadIdx.x};
  sample_row_excluding<REPLACE>(a.indices, a.exclude, a.num_exclude, (uint32_t)r, begin, d, a.k, room, a.k0, a.k1, a.off0, a.off1, slot,
                                a.s_indices + base, a.s_entries + base);
}

template <bool SORTED>
static __global__ __launch_bounds__(256) void find_edges_kernel(const int* indptr, const int* indices, const int* rows, const int* cols,
                                                                int num_rows, int num_queries, int* out) {
  const long long i = (long long)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= num_queries) return;
  out[i] = find_entry<SORTED>(indptr, indices, num_rows, rows[i], cols[i]);
}

// launch_sample_neighbors with an exclusion list.  exclude = device int32 [num_exclude], strictly ascending ids in [0, entries) (not
// checked on the device; may be null where num_exclude == 0, which gives the plain kernel's bits).  s_indptr must be the rule's with
// d' = d_i - x_i in place of d_i: every element of s_indices and s_entries is written then; neither needs initialising.
inline int launch_sample_neighbors_excluding(const int* indptr, const int* indices, int num_rows, const int* seeds, int num_seeds,
                                             const int* s_indptr, long long num_sampled, int fanout, int replace, uint64_t seed,
                                             uint64_t offset, const int* exclude, int num_exclude, int* s_indices, int* s_entries,
                                             hipStream_t stream) {
  if (num_rows < 0 || num_seeds < 0 || num_exclude < 0 || num_sampled < 0 || num_sampled > INT_MAX) return kErrBadShape;
  if (fanout != kSampleAll && (fanout < 1 || fanout > kSampleMaxFanout)) return kErrBadShape;
  if (replace != 0 && replace != 1) return kErrBadShape;
  if (num_seeds == 0) return kOk;
  if (bad_ptr(indptr, 3) || bad_ptr(seeds, 3) || bad_ptr(s_indptr, 3)) return kErrBadShape;
  if (num_exclude > 0 ? bad_ptr(exclude, 3) : misaligned(exclude, 3)) return kErrBadShape;
  if (num_sampled > 0 && (bad_ptr(indices, 3) || bad_ptr(s_indices, 3) || bad_ptr(s_entries, 3))) return kErrBadShape;
  if (num_sampled == 0) return kOk;                  // nothing to write
  const bool all = fanout == kSampleAll;
  const SampleExcludingArgs a{indptr, indices, seeds, s_indptr, exclude, s_indices, s_entries, num_rows, num_seeds, num_exclude,
                              all ? INT_MAX : fanout, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
  const dim3 grid((unsigned)(((long long)num_seeds + 255) / 256));
  if (replace || all)
    hipLaunchKernelGGL((sample_neighbors_excluding_kernel<true>), grid, dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL((sample_neighbors_excluding_kernel<false>), grid, dim3(256), (size_t)256 * fanout * sizeof(int), stream, a);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// out = device int32 [num_queries], every element written.  num_entries = the CSR's entry count (indices may be null only where it
// is 0).  num_queries == 0: kOk without a launch.
inline int launch_find_edges(const int* indptr, const int* indices, int num_rows, long long num_entries, const int* rows, const int* cols,
                             int num_queries, int assume_sorted, int* out, hipStream_t stream) {
  if (num_rows < 0 || num_queries < 0 || num_entries < 0 || num_entries > INT_MAX) return kErrBadShape;
  if (assume_sorted != 0 && assume_sorted != 1) return kErrBadShape;
  if (num_queries == 0) return kOk;
  if (bad_ptr(indptr, 3) || bad_ptr(rows, 3) || bad_ptr(cols, 3) || bad_ptr(out, 3)) return kErrBadShape;
  if (num_entries > 0 ? bad_ptr(indices, 3) : misaligned(indices, 3)) return kErrBadShape;
  const dim3 grid((unsigned)(((long long)num_queries + 255) / 256));
  if (assume_sorted)
    hipLaunchKernelGGL((find_edges_kernel<true>), grid, dim3(256), 0, stream, indptr, indices, rows, cols, num_rows, num_queries, out);
  else
    hipLaunchKernelGGL((find_edges_kernel<false>), grid, dim3(256), 0, stream, indptr, indices, rows, cols, num_rows, num_queries, out);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

}  // namespace voltrix
