// Voltrix-SpMM for MI355X (gfx950) -- the packed keep mask of attention dropout: one bit per (edge, head), written once by a
// counter-based generator and read by the three kernels of attn_aggregate (attn_aggregate_kernels.hpp, DROP = true).
//
//   mask   int32 [nnz, W], W = ceil(H / 32), CSR edge order; bit h & 31 of word h >> 5 of edge e set: (e, h) is kept.
//          Bits past H are written as zeros; consumers never look at them.
//   keep   (e, h) is kept iff x >= threshold, x = word h & 3 of
//          Philox4x32-10(counter = (e, h >> 2, offset & 0xffffffff, offset >> 32), key = (seed & 0xffffffff, seed >> 32)).
//          threshold = min(2^32 - 1, floor(p 2^32)) is the caller's integer: the kept probability is 1 - threshold / 2^32,
//          threshold = 0 keeps everything.  A bit is a function of (seed, offset, e, h) and of nothing else -- not of the
//          launch geometry, not of nnz, not of H.
//
// Why a stored mask and not a generator inside the hot loops: ten Philox rounds are 40 integer multiplies (v_mul_lo_u32 +
// v_mul_hi_u32 twice per round) next to about 25 VALU operations and one gather per edge in the forward's lane; the mask costs one
// broadcast 4-byte load per edge instead, 32 times less than alpha [nnz, H] would, and it can be inspected, replayed and supplied
// by the caller (DropEdge: the same bit on every head).
//
// Kernel: one thread per (edge, word), at most eight Philox evaluations (four heads each), one coalesced 4-byte store per thread.
// No LDS, no scratch, no atomics, no host synchronisation; the offset e W + w is 64-bit.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "voltrix/launch_geometry.hpp"

namespace voltrix {

struct Philox4 {
  uint32_t x[4];
};

// Philox4x32-10 (Salmon et al., SC'11): multipliers 0xD2511F53 / 0xCD9E8D57, Weyl increments 0x9E3779B9 / 0xBB67AE85 between rounds
__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return {{c0, c1, c2, c3}};
}

// the word `word` of edge `edge`: bits of the heads [32 word, min(heads, 32 word + 32))
__host__ __device__ inline uint32_t dropout_mask_word(uint32_t edge, int word, int heads, uint32_t threshold, uint32_t k0, uint32_t k1,
                                                      uint32_t off0, uint32_t off1) {
  uint32_t bits = 0;
  for (int g = 0; g < 8; ++g) {
    const int h0 = word * 32 + g * 4;
    if (h0 >= heads) break;
    const Philox4 r = philox4x32_10(edge, (uint32_t)(h0 >> 2), off0, off1, k0, k1);
    for (int j = 0; j < 4; ++j)
      if (h0 + j < heads && r.x[j] >= threshold) bits |= 1u << (g * 4 + j);
  }
  return bits;
}

struct DropoutMaskArgs {
  uint32_t* mask;      // [nnz, words]
  long long total;     // nnz * words
  int heads;
  int words;           // ceil(heads / 32)
  uint32_t threshold;
  uint32_t k0, k1;     // seed
  uint32_t off0, off1; // offset
};

// The runtime refuses a grid of 2^32 threads or more in one dimension (nnz = 2^31 - 1 with two words per edge is 2^24 blocks of 256: a
// launch error, found by tests/test_gpu_large_offsets.py).  The grid is capped below that and a thread strides over the words: one word
// per thread for every total below 2^32 - 256, as before.
constexpr long long kDropoutMaskMaxBlocks = 0xffffff;

static __global__ __launch_bounds__(256) void dropout_mask_kernel(const DropoutMaskArgs a) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + (int)threadIdx.x; i < a.total; i += stride) {
    const long long edge = a.words == 1 ? i : i / a.words;    // one word per edge for H <= 32: no 64-bit division on that path
    const int word = (int)(i - edge * a.words);
    a.mask[i] = dropout_mask_word((uint32_t)edge, word, a.heads, a.threshold, a.k0, a.k1, a.off0, a.off1);
  }
}

// Every word of mask [nnz, ceil(heads / 32)] is written.  nnz == 0: kOk without a launch.
inline int launch_dropout_mask(long long nnz, int heads, uint32_t threshold, uint64_t seed, uint64_t offset, void* mask,
                               hipStream_t stream) {
  if (heads < 1 || nnz < 0 || nnz > INT_MAX) return kErrBadShape;
  if (nnz == 0) return kOk;
  if (bad_ptr(mask, 3)) return kErrBadShape;
  const int words = (int)(((long long)heads + 31) / 32);
  const long long total = nnz * words;
  const long long all_blocks = (total + 255) / 256;
  const long long blocks = all_blocks < kDropoutMaskMaxBlocks ? all_blocks : kDropoutMaskMaxBlocks;
  const DropoutMaskArgs a{static_cast<uint32_t*>(mask), total, heads, words, threshold, (uint32_t)seed, (uint32_t)(seed >> 32),
                          (uint32_t)offset, (uint32_t)(offset >> 32)};
  hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

}  // namespace voltrix
