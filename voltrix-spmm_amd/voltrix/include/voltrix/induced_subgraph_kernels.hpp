// Voltrix-SpMM for MI355X (gfx950) -- induced subgraphs and random walks on a device CSR: what subgraph mini-batch training needs
// (Cluster-GCN: a batch is a cluster; GraphSAINT-RW: a batch is the nodes a set of random walks visits).
//   (s_indptr, s_local, s_entries) = rows `rows` of the CSR restricted to the columns `cols`, on local column ids, with the CSR entry
//                                    id of every kept entry
//   (nodes, entries)               = W uniform random walks of `length` steps
// No reference counterpart.  voltrix/subgraph.py and DESIGN.md 3.24 restate both contracts, tests/subgraph_oracle.py is the numpy
// restatement.
//
// THE SUBGRAPH CONTRACT.  rows: int32 [R] global row ids, any order, duplicates allowed (a duplicate row is emitted twice).  cols:
// int32 [C] global column ids in [0, num_cols), NO duplicates.  Row i of the result is row rows[i] of the CSR with exactly those
// entries whose column is in cols, IN CSR ORDER -- a stable compaction: a sorted row stays sorted only if cols is ascending.  A column
// that appears twice in a row is kept twice.  s_local[e] is the position in cols of the entry's column (the local id of cols[j] is j,
// so feat[cols] is the subgraph's feature matrix); s_entries[e] is the entry's index in `indices` (edge values, edge features,
// arg-style bookkeeping: the meaning it has in sample_neighbors).  Columns in `indices` outside [0, num_cols) are never selected and
// never read through.  A row id outside [0, num_rows) has degree 0 inside the kernels (callers reject it earlier); a row never writes
// more than s_indptr[i + 1] - s_indptr[i].
//
// Mechanism.  A dense table int32 [num_cols], ZERO on entry, marked by launch_block_mark_seeds (neighbor_sample_kernels.hpp):
// table[cols[j]] = -(j + 1).  subgraph_kernel<GROUP, FILL>: a lane group of GROUP lanes (4, 8, 16, 32 or 64; 256 / GROUP rows per
// workgroup) owns one output row and walks its entries GROUP at a time -- coalesced 4-byte loads of `indices`, a gather of table[c] --
// and takes its slice of the 64-bit __ballot of "selected".  The count (FILL = false) adds popcount(slice) up and lane 0 stores
// counts[i]; the caller takes the prefix sum s_indptr (plumbing).  The fill (FILL = true) is the same walk: a lane's slot is
// base + running + popcount(slice below this lane), running += popcount(slice): a stable compaction without LDS and without atomics.
// One body for both.  The groups of one wave walk rows of different length: the ballot is taken under the loop's own execution mask,
// and a group's lanes leave the loop together (the trip count is the group's), so a group always sees its own slice whole.
// A hub row is walked by one group: the row-per-group weakness DESIGN 3.10 / 3.13 name.  Not solved here.
//
// THE WALK RULE.  nodes[w, 0] = starts[w].  At step t (0-based) walker w stands on node v of degree d = indptr[v + 1] - indptr[v]:
//   d == 0         the walk is over: this and every later step write -1 in nodes and in entries;
//   otherwise      the walker takes the entry at position (uint64(draw(w, t)) * d) >> 32 of row v: entries[w, t] is its CSR entry id,
//                  nodes[w, t + 1] its column;
//   draw(w, t)     word t & 3 of Philox4x32-10(counter = (w, (t >> 2) | 0xC0000000, offset & 0xffffffff, offset >> 32),
//                  key = (seed & 0xffffffff, seed >> 32)).  Bits 31 AND 30 of counter word 1 separate these draws from the neighbour
//                  sampler's ((i >> 2) | 0x80000000, i < 64) and from the dropout mask's (h >> 2 < 2^29): one seed for all three gives
//                  unrelated streams.
// A node id outside [0, num_rows) -- a column of a rectangular CSR, or a start the caller did not reject -- is recorded as it is and
// ends the walk like a dead end: it has degree 0, indptr is never read out of bounds.  w is the walker's index in starts: duplicate
// starts are different walks, and the result is a function of (seed, offset, w, starts[w], the graph) only, not of the launch geometry.
// random_walk_kernel: one lane per walker, one Philox evaluation per four steps, the four words read through selects (SampleDraws
// records why).  Every element of nodes [W, length + 1] and entries [W, length] is written, the -1 padding included.  The stores go
// through two strides each, so the same kernel writes walker-major ([W, length + 1]: a wave's stores are length + 1 words apart) or
// step-major ([length + 1, W]: coalesced) buffers; DESIGN 3.24 has the measurement.
//
// No atomics anywhere; offsets that can pass 2^31 are 64-bit; entry counts are limited to INT_MAX; no host synchronisation.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "voltrix/neighbor_sample_kernels.hpp"

namespace voltrix {

constexpr uint32_t kWalkCounterBits = 0xC0000000u;
constexpr int kWalkMaxLength = 1 << 20;

// ---- the induced subgraph ------------------------------------------------------------------------------------------------------------
struct SubgraphArgs {
  const int* indptr;     // [num_rows + 1]
  const int* indices;    // [entries]
  const int* rows;       // [num_sub_rows] global row ids
  const int* table;      // [num_cols]: -(j + 1) for cols[j], 0 elsewhere
  const int* s_indptr;   // fill: [num_sub_rows + 1]
  int* counts;           // count: [num_sub_rows]
  int* s_local;          // fill: [s_indptr[num_sub_rows]]
  int* s_entries;        // fill: the same
  int num_rows;
  int num_sub_rows;
  int num_cols;
};

template <int GROUP, bool FILL>
static __global__ __launch_bounds__(256) void subgraph_kernel(const SubgraphArgs a) {
  static_assert(GROUP == 4 || GROUP == 8 || GROUP == 16 || GROUP == 32 || GROUP == 64, "a lane group divides a wave");
  constexpr int kRowsPerBlock = 256 / GROUP;
  constexpr unsigned long long kSliceMask = GROUP == 64 ? ~0ull : (1ull << (GROUP % 64)) - 1;
  const int lane = (int)threadIdx.x & (GROUP - 1);
  const int shift = ((int)threadIdx.x & 63) & ~(GROUP - 1);                   // where this group's slice of a wave's ballot begins
  const long long i = (long long)blockIdx.x * kRowsPerBlock + (int)threadIdx.x / GROUP;
  int begin = 0, d = 0;
  if (i < a.num_sub_rows) {
    const int r = a.rows[i];
    if (r >= 0 && r < a.num_rows) {
      begin = a.indptr[r];
      d = a.indptr[r + 1] - begin;
    }
  }
  long long base = 0;
  int room = 0;
  if (FILL && i < a.num_sub_rows) {
    base = a.s_indptr[i];
    room = a.s_indptr[i + 1] - a.s_indptr[i];
  }
  int running = 0;
  for (int first = 0; first < d; first += GROUP) {                            // the same trip count for every lane of the group
    const int k = first + lane;
    int t = 0;
    if (k < d) {
      const int c = a.indices[(long long)begin + k];
      if (c >= 0 && c < a.num_cols) t = a.table[c];
    }
    const bool selected = t < 0;
    const unsigned long long slice = (__ballot(selected) >> shift) & kSliceMask;
    if constexpr (FILL) {
      const int slot = running + __popcll(slice & ((1ull << lane) - 1));
      if (selected && slot < room) {
        a.s_local[base + slot] = -t - 1;
        a.s_entries[base + slot] = begin + k;
      }
    }
    running += __popcll(slice);
  }
  if constexpr (!FILL) {
    if (lane == 0 && i < a.num_sub_rows) a.counts[i] = running;
  }
}

inline bool subgraph_group_ok(int group) { return group == 4 || group == 8 || group == 16 || group == 32 || group == 64; }

template <bool FILL>
inline void subgraph_dispatch(const SubgraphArgs& a, int group, hipStream_t stream) {
  const dim3 grid((unsigned)(((long long)a.num_sub_rows + 256 / group - 1) / (256 / group)));
  switch (group) {
    case 4: hipLaunchKernelGGL((subgraph_kernel<4, FILL>), grid, dim3(256), 0, stream, a); break;
    case 8: hipLaunchKernelGGL((subgraph_kernel<8, FILL>), grid, dim3(256), 0, stream, a); break;
    case 16: hipLaunchKernelGGL((subgraph_kernel<16, FILL>), grid, dim3(256), 0, stream, a); break;
    case 32: hipLaunchKernelGGL((subgraph_kernel<32, FILL>), grid, dim3(256), 0, stream, a); break;
    default: hipLaunchKernelGGL((subgraph_kernel<64, FILL>), grid, dim3(256), 0, stream, a); break;
  }
}

// counts[i] = the number of entries of row rows[i] whose column the table marks (table[c] < 0).  Every element of counts
// [num_sub_rows] is written.  num_sub_rows == 0: kOk without a launch.
inline int launch_subgraph_count(const int* indptr, const int* indices, int num_rows, const int* rows, int num_sub_rows,
                                 const int* table, int num_cols, int group, int* counts, hipStream_t stream) {
  if (num_rows < 0 || num_sub_rows < 0 || num_cols < 0 || !subgraph_group_ok(group)) return kErrBadShape;
  if (num_sub_rows == 0) return kOk;
  if (bad_ptr(indptr, 3) || bad_ptr(indices, 3) || bad_ptr(rows, 3) || bad_ptr(table, 3) || bad_ptr(counts, 3)) return kErrBadShape;
  const SubgraphArgs a{indptr, indices, rows, table, nullptr, counts, nullptr, nullptr, num_rows, num_sub_rows, num_cols};
  subgraph_dispatch<false>(a, group, stream);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// s_indptr must be the exclusive prefix sum of launch_subgraph_count's counts for the same arguments, num_selected = s_indptr[num_sub_rows].
// Every element of s_local and s_entries [num_selected] is written then; neither needs initialising.  kOk without a launch where
// num_sub_rows == 0 or num_selected == 0.
inline int launch_subgraph_fill(const int* indptr, const int* indices, int num_rows, const int* rows, int num_sub_rows,
                                const int* table, int num_cols, int group, const int* s_indptr, long long num_selected, int* s_local,
                                int* s_entries, hipStream_t stream) {
  if (num_rows < 0 || num_sub_rows < 0 || num_cols < 0 || num_selected < 0 || num_selected > INT_MAX || !subgraph_group_ok(group))
    return kErrBadShape;
  if (num_sub_rows == 0) return kOk;
  if (bad_ptr(indptr, 3) || bad_ptr(indices, 3) || bad_ptr(rows, 3) || bad_ptr(table, 3) || bad_ptr(s_indptr, 3)) return kErrBadShape;
  if (num_selected == 0) return kOk;                     // nothing to write
  if (bad_ptr(s_local, 3) || bad_ptr(s_entries, 3)) return kErrBadShape;
  const SubgraphArgs a{indptr, indices, rows, table, s_indptr, nullptr, s_local, s_entries, num_rows, num_sub_rows, num_cols};
  subgraph_dispatch<true>(a, group, stream);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// ---- the random walk -----------------------------------------------------------------------------------------------------------------
// draw(w, t) for t = 0, 1, 2, ...: one Philox evaluation per four steps
struct WalkDraws {
  uint32_t w, k0, k1, off0, off1;
  Philox4 block;
  __host__ __device__ inline uint32_t operator()(int t) {
    if ((t & 3) == 0) block = philox4x32_10(w, (uint32_t)(t >> 2) | kWalkCounterBits, off0, off1, k0, k1);
    const int s = t & 3;      // selects, not an indexed read (SampleDraws)
    return s == 0 ? block.x[0] : s == 1 ? block.x[1] : s == 2 ? block.x[2] : block.x[3];
  }
};

// One step of the rule from node v with the draw x: the CSR entry taken (-1: the walk is over) and, returned, the node it leads to
// (-1 likewise).  v outside [0, num_rows) -- -1 included -- has degree 0.  The kernel and a host program run this code.
__host__ __device__ inline int walk_step(const int* indptr, const int* indices, int num_rows, int v, uint32_t x, int* entry) {
  *entry = -1;
  if (v < 0 || v >= num_rows) return -1;
  const int begin = indptr[v];
  const int d = indptr[v + 1] - begin;
  if (d <= 0) return -1;
  const int e = begin + sample_replace_position(x, d);
  *entry = e;
  return indices[e];
}

// The whole walk of walker w; element (w, t) of nodes is at nodes[w * node_walker + t * node_step], of entries at
// entries[w * entry_walker + t * entry_step].
__host__ __device__ inline void walk_one(const int* indptr, const int* indices, int num_rows, uint32_t w, int start, int length,
                                         uint32_t k0, uint32_t k1, uint32_t off0, uint32_t off1, int* nodes, long long node_walker,
                                         long long node_step, int* entries, long long entry_walker, long long entry_step) {
  WalkDraws draw{w, k0, k1, off0, off1, {}};
  int* const my_nodes = nodes + (long long)w * node_walker;
  int* const my_entries = entries + (long long)w * entry_walker;
  int v = start;
  my_nodes[0] = v;
  for (int t = 0; t < length; ++t) {
    int e;
    v = walk_step(indptr, indices, num_rows, v, draw(t), &e);
    my_entries[t * entry_step] = e;
    my_nodes[(t + 1) * node_step] = v;
  }
}

struct RandomWalkArgs {
  const int* indptr;     // [num_rows + 1]
  const int* indices;    // [entries]
  const int* starts;     // [num_walkers]
  int* nodes;            // num_walkers * (length + 1)
  int* entries;          // num_walkers * length
  long long node_walker, node_step, entry_walker, entry_step;
  int num_rows;
  int num_walkers;
  int length;
  uint32_t k0, k1;       // seed
  uint32_t off0, off1;   // offset
};

static __global__ __launch_bounds__(256) void random_walk_kernel(const RandomWalkArgs a) {
  const long long w = (long long)blockIdx.x * 256 + (int)threadIdx.x;
  if (w >= a.num_walkers) return;
  walk_one(a.indptr, a.indices, a.num_rows, (uint32_t)w, a.starts[w], a.length, a.k0, a.k1, a.off0, a.off1, a.nodes, a.node_walker,
           a.node_step, a.entries, a.entry_walker, a.entry_step);
}

// step_major = 0: nodes is [num_walkers, length + 1], entries [num_walkers, length]; 1: nodes [length + 1, num_walkers], entries
// [length, num_walkers].  Every element of both is written.  num_walkers == 0: kOk without a launch.
inline int launch_random_walk(const int* indptr, const int* indices, int num_rows, const int* starts, int num_walkers, int length,
                              uint64_t seed, uint64_t offset, int* nodes, int* entries, int step_major, hipStream_t stream) {
  if (num_rows < 0 || num_walkers < 0 || length < 0 || length > kWalkMaxLength) return kErrBadShape;
  if (step_major != 0 && step_major != 1) return kErrBadShape;
  if ((long long)num_walkers * ((long long)length + 1) > INT_MAX) return kErrBadShape;
  if (num_walkers == 0) return kOk;
  if (bad_ptr(indptr, 3) || bad_ptr(starts, 3) || bad_ptr(nodes, 3)) return kErrBadShape;
  if (length > 0 && (bad_ptr(indices, 3) || bad_ptr(entries, 3))) return kErrBadShape;
  RandomWalkArgs a{indptr, indices, starts, nodes, entries, 0, 0, 0, 0, num_rows, num_walkers, length,
                   (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
  if (step_major) {
    a.node_walker = a.entry_walker = 1;
    a.node_step = a.entry_step = num_walkers;
  } else {
    a.node_walker = (long long)length + 1;
    a.entry_walker = length;
    a.node_step = a.entry_step = 1;
  }
  hipLaunchKernelGGL(random_walk_kernel, dim3((unsigned)(((long long)num_walkers + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

}  // namespace voltrix
