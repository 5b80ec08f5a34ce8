// MFMA pieces of the transducer searches whose rows are hypotheses (rnnt_beam.hip) or streams (stateless.hip): the activation
// operand A [16, K] sits in LDS, the weight operand goes from global memory / L2 straight into the MFMA B layout -- the rows are
// K-contiguous, so a lane's fragment is ONE 16-byte load (bf16 images: v_mfma_f32_16x16x32_bf16, 8 k per lane; fp32 masters: four
// v_mfma_f32_16x16x4_f32 on the four floats of the load, A permuted alike) -- and NT * U loads per lane are in flight.
#pragma once
#include "common.h"

// per weight type: k per MFMA block and per lane (one 16-byte load)
template <typename WT> struct RbT;
template <> struct RbT<bf16_t> { static constexpr int KB = 32, V = 8; };
template <> struct RbT<float> { static constexpr int KB = 16, V = 4; };

template <typename WT> __device__ __forceinline__ f32x4 rb_mfma(u32x4 a, u32x4 b, f32x4 c);
template <> __device__ __forceinline__ f32x4 rb_mfma<bf16_t>(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x4 rb_mfma<float>(u32x4 a, u32x4 b, f32x4 c) {
  // lane group g holds k = 4g .. 4g+3 of the 16-wide block in both operands: four k-slices, summed by four instructions
#pragma unroll
  for (int i = 0; i < 4; ++i) c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[i]), __uint_as_float(b[i]), c, 0, 0, 0);
  return c;
}
template <typename WT> __device__ __forceinline__ WT rb_cvt(float v);
template <> __device__ __forceinline__ bf16_t rb_cvt<bf16_t>(float v) { return f2bf(v); }
template <> __device__ __forceinline__ float rb_cvt<float>(float v) { return v; }

// acc[t] += A[16, K] . W_t[16, K]^T for NT weight tiles that share A.  arow / wrow[t]: this lane's row (lane % 16) of the A tile in
// LDS and of each weight tile in global memory; K % V == 0, so a lane's V elements lie inside the row or are zero in BOTH operands.
// NT * U 16-byte global loads per lane are issued before the first MFMA of an iteration.
template <typename WT, int NT, int U>
__device__ __forceinline__ void rb_mma(const WT* const (&wrow)[NT], const WT* arow, int K, f32x4 (&acc)[NT]) {
  constexpr int KB = RbT<WT>::KB;
  const int kq = ((threadIdx.x & 63) >> 4) * RbT<WT>::V;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (int kb = 0; kb < K; kb += KB * U) {
    u32x4 a[U], b[U][NT];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = kb + u * KB + kq;
      const bool in = k < K;
#pragma unroll
      for (int t = 0; t < NT; ++t) b[u][t] = in ? *reinterpret_cast<const u32x4*>(wrow[t] + k) : zero;
      a[u] = in ? *reinterpret_cast<const u32x4*>(arow + k) : zero;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = rb_mfma<WT>(a[u], b[u][t], acc[t]);
  }
}
