// Voltrix-SpMM for MI355X (gfx950) -- aggregation of FP8 feature rows straight from the CSR, and the quantiser that makes such rows:
//   data[i, f]  = rne_e4m3(clamp(fp32(feat[i, f]) * inv_scale[f], -448, 448))                      (quantize_fp8_rows_kernel)
//   out[i, f]   = scale[f] * sum over the entries e of row i of v_e * dec(data[col_e, f])          (spmm_csr_rows_fp8_kernel)
// The format is OCP e4m3fn (torch.float8_e4m3fn): 1 sign, 4 exponent (bias 7), 3 mantissa bits, subnormals m 2^-9, no infinities,
// 0x7f / 0xff NaN, largest finite 448 -- what gfx950's v_cvt_pk_f32_fp8 / v_cvt_pk_fp8_f32 convert, NOT the MI300 e4m3fnuz encoding.
//
// Why.  Every aggregation kernel of this package is bound by gathered bytes: a row of the feature matrix per entry, at the rate the
// CUs can request lines.  An fp8 row is half the bytes of the narrowest row the other kernels read.
//
// Why the scale is per COLUMN and not per row.  A per-row scale would be a second gathered line per entry -- the bytes fp8 saves.  A
// per-column scale costs nothing in the loop: it leaves the sum and is applied once in the epilogue, 16 multiplies per lane.
//
// Aggregation, spmm_csr_rows_fp8_kernel<TO, WEIGHTED, UNROLL>: the row-gather skeleton of csr_row_gather.hpp with a piece of V = 16
// features.  A row of data is F16 bytes, F16 = F rounded up to 16: one 16-byte load per entry, 16 fp32 accumulators; grid.y walks
// slabs of 64 x 16 = 1024 columns; xcd_ranges = 0 asks for the round-robin order of workgroups.  The offsets col F16 and row F16 are
// 64-bit.  Decode: v_cvt_pk_f32_fp8 on the low and the high half of every word, eight per 16 bytes; every decoded value is exact in
// fp32.  The sum is fp32 in CSR entry order, with values one fused multiply-add per element; it starts from -0.0, the identity of IEEE
// addition, so that a row's first term arrives with its own sign (a row that gathers one -0 gives -0); a row without entries starts
// from, and gives, +0.  The epilogue loads the
// lane's 16 scales (four 16-byte loads), multiplies, and stores 64 bytes (fp32) or 32 bytes (fp16 / bf16: the fp32 result rounded to
// nearest even) in 16-byte pieces.  Every element of the output [num_rows, F16] is written.  No LDS, no atomics, no workspace, the same
// bits on every call.  |out - ref| <= (k + 2) 2^-23 |scale[f]| sum_e |v_e dec_e| for the k entries of a row against float64 on the
// same bytes; integer-valued codes and values with power-of-two scales give equality.
//
// UNROLL: 4, as in the 16-bit kernel; VOLTRIX_SPMM_FP8_UNROLL = 8 is the other build of harness/experiments/exp_spmm_fp8_unroll.py
// (DESIGN.md 3.30 has both measurements).
//
// Quantiser, quantize_fp8_rows_kernel<T>: row-major, one launch, feat read once.  The same lane groups: a lane owns 16 features of a
// slab and holds their 16 inv_scales in registers; the groups walk the rows in a grid-stride loop with 64-bit offsets.  A lane reads
// its 16 features (fp32: four, fp16 / bf16: two 16-byte loads) where the row stride keeps rows on 16-byte boundaries and the piece is
// whole, element by element otherwise (a last piece reads only what exists: the padding is written as 0x00), multiplies in fp32 --
// ONE multiply, so that a CPU oracle reproduces the bits --, clamps to +-448 (a NaN stays a NaN), packs with v_cvt_pk_fp8_f32 (round
// to nearest even, e4m3 subnormals) and stores 16 bytes.
//
// Known limit: a hub row serialises its wave, like every row-per-lane-group kernel here.  Nothing is checked on the device.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>

#include "voltrix/csr_row_gather.hpp"

#ifndef VOLTRIX_SPMM_FP8_UNROLL
#define VOLTRIX_SPMM_FP8_UNROLL 4         // entries in flight per lane: 4, or 8 (the experiment's other build)
#endif

namespace voltrix {

constexpr int kFp8Unroll = VOLTRIX_SPMM_FP8_UNROLL;
static_assert(kFp8Unroll == 4 || kFp8Unroll == 8, "unroll");
constexpr float kFp8Max = 448.0f;         // the largest finite e4m3fn

typedef float float2_t __attribute__((ext_vector_type(2)));

template <typename TO>
struct Fp8CsrArgs {
  const int* indptr;      // [num_rows + 1]
  const int* indices;     // [nnz] column ids = rows of `input`
  const float* values;    // WEIGHTED kernels: [nnz] fp32 in CSR order; else unused
  const uint8_t* input;   // [*, F16] e4m3fn codes
  const float* scale;     // [F16]
  TO* output;             // [num_rows, F16]
  int num_rows;
  int F16;                // a multiple of 16
  int lanes_per_row;      // power of two <= 64
  int groups_per_xcd;     // ceil(row groups / 8): sizes the grid; a row group = 256 / lanes_per_row rows
  int xcd_ranges;         // 1: XCD x owns a contiguous eighth of the row groups; 0: consecutive groups go round the XCDs
};

// the 16 codes of a piece as fp32 (exact): two packed conversions per word
__device__ __forceinline__ void fp8_piece_as_float(float (&x)[16], const uint4_t raw) {
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const float2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw[w], false);
    const float2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw[w], true);
    x[4 * w] = lo[0];
    x[4 * w + 1] = lo[1];
    x[4 * w + 2] = hi[0];
    x[4 * w + 3] = hi[1];
  }
}

template <bool WEIGHTED>
__device__ __forceinline__ void fp8_accumulate(float (&acc)[16], const uint4_t raw, const float v) {
  float x[16];
  fp8_piece_as_float(x, raw);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if constexpr (WEIGHTED) acc[i] = __builtin_fmaf(v, x[i], acc[i]);
    else acc[i] += x[i];
  }
}

// fp32 -> bfloat16 bits, round to nearest even, NaN kept quiet (scatter_values_kernel's rule)
__device__ __forceinline__ unsigned bf16_bits_rne(const float v) {
  const unsigned b = __builtin_bit_cast(unsigned, v);
  return (v != v) ? 0x7fc0u : (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
}

template <typename TO, bool WEIGHTED, int UNROLL = kFp8Unroll>
static __global__ __launch_bounds__(256) void spmm_csr_rows_fp8_kernel(const Fp8CsrArgs<TO> a) {
  const CsrLanePlace p = csr_lane_place<16>(a.lanes_per_row, a.groups_per_xcd, a.num_rows, a.F16, a.xcd_ranges != 0);
  if (!p.work) return;
  const long long row = p.row, col0 = p.col0;
  const int e = a.indptr[row];
  const int end = a.indptr[row + 1];
  // -0.0 is the identity of IEEE addition (x + -0 = x for every x, -0 included): the first term keeps its sign.  No entries: +0
  const float start = e < end ? -0.0f : 0.0f;
  float acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = start;
  const uint8_t* const base = a.input + col0;
  const long long F16 = a.F16;
  struct Slot {
    uint4_t raw;
    float v;
  };
  csr_for_each_batch<UNROLL, Slot>(
      e, end,
      [&](Slot& s, const int ee) {
        s.raw = *reinterpret_cast<const uint4_t*>(base + (long long)a.indices[ee] * F16);
        s.v = WEIGHTED ? a.values[ee] : 1.0f;
      },
      [&](const Slot& s, int, const bool live) {
        if (live) fp8_accumulate<WEIGHTED>(acc, s.raw, s.v);
      });
  const float4_t* const sc = reinterpret_cast<const float4_t*>(a.scale + col0);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float4_t s = sc[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[4 * i + j] *= s[j];
  }
  TO* const out = a.output + row * F16 + col0;
  if constexpr (std::is_same<TO, float>::value) {
    csr_store_piece(out, acc);
  } else if constexpr (std::is_same<TO, _Float16>::value) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      half8_t h;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        // the scaled fp32 value is pinned in its register before the conversion: the compiler otherwise folds the multiply above and
        // this cast into v_fma_mixlo_f16(acc, scale, +0), which rounds once from the exact product (not out32.to(fp16)) and turns
        // a -0 into +0
        float r = acc[8 * i + j];
        asm("" : "+v"(r));
        h[j] = (_Float16)r;                                               // v_cvt_f16_f32: round to nearest even
      }
      reinterpret_cast<half8_t*>(out)[i] = h;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      uint4_t w;
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = bf16_bits_rne(acc[8 * i + 2 * j]) | (bf16_bits_rne(acc[8 * i + 2 * j + 1]) << 16);
      reinterpret_cast<uint4_t*>(out)[i] = w;
    }
  }
}

// out_dtype: 0 fp32, 1 fp16, 2 bfloat16.  input: e4m3fn codes [*, embedding_dim16]; scale: fp32 [embedding_dim16]; output
// [num_rows, embedding_dim16] of out_dtype, every element written.  values may be NULL (1).  On a pattern without entries neither
// indices, values nor input is read (they must still be valid pointers).  Nothing is checked on the device.
inline int launch_spmm_fp8_csr(const int* indptr, const int* indices, const float* values, int num_rows, int embedding_dim16,
                               const void* input, const float* scale, void* output, int out_dtype, int xcd_ranges,
                               long long num_entries, hipStream_t stream) {
  if (num_rows < 0 || embedding_dim16 < 0 || embedding_dim16 % 16 || num_entries < 0 || num_entries > INT_MAX || out_dtype < 0 ||
      out_dtype > 2)
    return kErrBadShape;
  if (num_rows == 0 || embedding_dim16 == 0) return kOk;
  if (bad_ptr(indptr, 3) || bad_ptr(indices, 3) || misaligned(values, 3) || bad_ptr(input, 15) || bad_ptr(scale, 15) ||
      bad_ptr(output, 15))
    return kErrBadShape;
  const RowGroupGrid g = row_group_grid(num_rows, embedding_dim16 / 16);
  if (!g.ok) return kErrBadShape;
  const dim3 grid = row_group_dim3(g);
  dispatch_feature_type(out_dtype, [&](auto tag) {
    using TO = decltype(tag);
    const Fp8CsrArgs<TO> a{indptr, indices, values, static_cast<const uint8_t*>(input), scale, static_cast<TO*>(output), num_rows,
                           embedding_dim16, g.lanes, (int)g.per_xcd, xcd_ranges ? 1 : 0};
    if (values != nullptr) hipLaunchKernelGGL((spmm_csr_rows_fp8_kernel<TO, true>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((spmm_csr_rows_fp8_kernel<TO, false>), grid, dim3(256), 0, stream, a);
  });
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// ---- the quantiser ---------------------------------------------------------------------------------------------------------------------
template <typename T>
struct Fp8QuantArgs {
  const T* input;           // [num_rows, F] with a row stride of input_ld elements
  const float* inv_scale;   // [F16]
  uint8_t* output;          // [num_rows, F16] with a row stride of output_ld bytes
  long long input_ld;
  long long output_ld;
  int num_rows;
  int F;
  int lanes_per_row;
  int vector_rows;          // 1: input and every row of it are on 16-byte boundaries
};

template <typename T>
__device__ __forceinline__ float fp8_feature_as_float(const T x) {
  if constexpr (std::is_same<T, bfloat16_bits>::value) return __builtin_bit_cast(float, (unsigned)x << 16);
  else return (float)x;
}

template <typename T>
static __global__ __launch_bounds__(256) void quantize_fp8_rows_kernel(const Fp8QuantArgs<T> a) {
  constexpr int V = 16 / (int)sizeof(T);                                // elements per 16-byte load
  const int L = a.lanes_per_row;
  const int rows_per_group = 256 / L;
  const int lane = (int)threadIdx.x & (L - 1);
  const long long col0 = ((long long)blockIdx.y * 64 + lane) * 16;
  if (col0 >= (long long)(a.F + 15) / 16 * 16) return;
  const int live = a.F - col0 < 16 ? (int)(a.F - col0) : 16;           // features of this piece that exist
  float inv[16];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float4_t s = reinterpret_cast<const float4_t*>(a.inv_scale + col0)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) inv[4 * i + j] = s[j];
  }
  const bool whole = a.vector_rows && live == 16;
  const long long stride = (long long)gridDim.x * rows_per_group;
  for (long long row = (long long)blockIdx.x * rows_per_group + (int)threadIdx.x / L; row < a.num_rows; row += stride) {
    const T* const in = a.input + row * a.input_ld + col0;
    float x[16];
    if (whole) {
      uint4_t raw[16 / V];
#pragma unroll
      for (int i = 0; i < 16 / V; ++i) raw[i] = reinterpret_cast<const uint4_t*>(in)[i];
#pragma unroll
      for (int i = 0; i < 16 / V; ++i) {
        float part[V];
        csr_piece_as_float<T>(part, raw[i]);
#pragma unroll
        for (int j = 0; j < V; ++j) x[V * i + j] = part[j];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) x[i] = i < live ? fp8_feature_as_float<T>(in[i]) : 0.0f;
    }
    uint4_t packed;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      float y[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p = x[4 * w + j] * inv[4 * w + j];
        const float c = __builtin_fminf(__builtin_fmaxf(p, -kFp8Max), kFp8Max);
        y[j] = p != p ? p : c;                                          // fmin / fmax drop a NaN: keep it
      }
      int word = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
      word = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], word, true);
      packed[w] = (unsigned)word;
    }
    if (live < 16) {                                                    // the padding is 0x00 whatever inv_scale holds there
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int keep = live - 4 * w;                                  // bytes of this word that exist
        packed[w] = keep >= 4 ? packed[w] : keep <= 0 ? 0u : packed[w] & (0xffffffffu >> (32 - 8 * keep));
      }
    }
    *reinterpret_cast<uint4_t*>(a.output + row * a.output_ld + col0) = packed;
  }
}

// dtype of input: 0 fp32, 1 fp16, 2 bfloat16.  input [num_rows, embedding_dim] with rows input_ld ELEMENTS apart (>= embedding_dim);
// inv_scale fp32 [F16], F16 = embedding_dim rounded up to 16; output [num_rows, F16] e4m3fn codes with rows output_ld BYTES apart (>=
// F16, a multiple of 16), every byte of the F16 written, the padding as 0x00.
inline int launch_quantize_fp8_rows(const void* input, int dtype, int num_rows, int embedding_dim, long long input_ld,
                                    const float* inv_scale, void* output, long long output_ld, hipStream_t stream) {
  if (num_rows < 0 || embedding_dim < 0 || embedding_dim > INT_MAX - 15 || dtype < 0 || dtype > 2) return kErrBadShape;
  const int F16 = (embedding_dim + 15) / 16 * 16;
  if (input_ld < embedding_dim || output_ld < F16 || output_ld % 16) return kErrBadShape;
  if (num_rows == 0 || embedding_dim == 0) return kOk;
  if (bad_ptr(input, 15) || bad_ptr(inv_scale, 15) || bad_ptr(output, 15)) return kErrBadShape;
  const RowGroupGrid g = row_group_grid(num_rows, F16 / 16);
  if (!g.ok) return kErrBadShape;
  const long long groups = ((long long)num_rows + g.rows_per_group - 1) / g.rows_per_group;
  const unsigned blocks = (unsigned)(groups < 256 * 32 ? groups : 256 * 32);      // a grid-stride loop beyond: 32 workgroups per CU
  const dim3 grid(blocks, (unsigned)g.slabs);
  dispatch_feature_type(dtype, [&](auto tag) {
    using T = decltype(tag);
    const int vector_rows = (input_ld * (long long)sizeof(T)) % 16 == 0;
    const Fp8QuantArgs<T> a{static_cast<const T*>(input), inv_scale, static_cast<uint8_t*>(output), input_ld, output_ld, num_rows,
                            embedding_dim, g.lanes, vector_rows};
    hipLaunchKernelGGL((quantize_fp8_rows_kernel<T>), grid, dim3(256), 0, stream, a);
  });
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

}  // namespace voltrix
