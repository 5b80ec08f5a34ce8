// What the RNN-T loss (rnnt.hip) and the TDT loss (tdt.hip) share: both run one wave per (b,t,u) row of the joint's logits, and
// both entries take the same pitched logits / gradient / workspace arguments.  Device side: the cell of a row, the walk over a
// row, -logsumexp of a row, the zero row of a padded cell and the mapped row of the gradient.  Host side: the argument checks,
// the vector-walk flag and the cost kernel.
#pragma once
#include "common.h"

// ---- cell of a row: row = (b * T + t) * U1 + u; the utterance's own lattice is [0, Tb) x [0, Ub)
struct TrCell {
  int b, t, u, Tb, Ub;
  __device__ __forceinline__ bool padded() const { return t >= Tb || u >= Ub; }
};
__device__ __forceinline__ TrCell tr_cell(long long row, int T, int U1, const long long* __restrict__ xlen,
                                          const long long* __restrict__ ylen) {
  TrCell c;
  c.u = (int)(row % U1);
  const long long bt = row / U1;
  c.t = (int)(bt % T);
  c.b = (int)(bt / T);
  c.Tb = (int)min((long long)T, xlen[c.b]);
  c.Ub = (int)min((long long)(U1 - 1), ylen[c.b]) + 1;
  return c;
}

// ---- walk over x[0:V1].  A row starts on a 4-byte boundary only (V1 = 1025 is the common case): up to 3 head scalars bring the
// walk to a 16-byte boundary, then n4 float4 groups from x + head, then up to 3 tail scalars from tail0.  vec = 0: all scalar
// (head = V1) -- the gradient kernels' walk when the rows of acts and grads do not share their alignment.
struct TrWalk { int head, n4, tail0, ntail; };
__device__ __forceinline__ TrWalk tr_walk(const float* x, int V1, int vec) {
  TrWalk w;
  w.head = vec ? min(V1, (int)((4u - (unsigned)(((unsigned long long)x >> 2) & 3u)) & 3u)) : V1;
  w.n4 = (V1 - w.head) >> 2;
  w.tail0 = w.head + 4 * w.n4;
  w.ntail = V1 - w.tail0;
  return w;
}

// -logsumexp(x[0:V1]) by one wave, in every lane
__device__ __forceinline__ float tr_neg_lse(const float* __restrict__ x, const TrWalk& w, int lane) {
  const float4* x4 = reinterpret_cast<const float4*>(x + w.head);
  float m = -INFINITY;
  if (lane < w.head) m = x[lane];
  if (lane < w.ntail) m = fmaxf(m, x[w.tail0 + lane]);
  for (int i = lane; i < w.n4; i += 64) {
    const float4 v = x4[i];
    m = fmaxf(m, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
  }
  m = wave_max(m);
  float s = 0.f;
  if (lane < w.head) s = __expf(x[lane] - m);
  if (lane < w.ntail) s += __expf(x[w.tail0 + lane] - m);
  for (int i = lane; i < w.n4; i += 64) {  // second pass hits L2 / the TA cache: the row is a few KiB
    const float4 v = x4[i];
    s += (__expf(v.x - m) + __expf(v.y - m)) + (__expf(v.z - m) + __expf(v.w - m));
  }
  s = wave_sum(s);
  return -(m + logf(s));
}

// ---- gradient rows (TG = float or bf16_t): g[v] = 0, or g[v] = one(v, x[v]), over the walk; columns [from, ldg) zero
template <typename TG>
__device__ __forceinline__ void tr_zero_pad(TG* g, int from, long long ldg, int lane) {
  for (int i = from + lane; i < ldg; i += 64) st(g + i, 0.f);
}
template <typename TG>
__device__ __forceinline__ void tr_zero_row(TG* g, const TrWalk& w, int lane) {
  const float z[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = lane; i < w.head; i += 64) st(g + i, 0.f);
  if (lane < w.ntail) st(g + w.tail0 + lane, 0.f);
  for (int i = lane; i < w.n4; i += 64) st4(g + w.head + 4 * i, z);
}
template <typename TG, typename F>
__device__ __forceinline__ void tr_map_row(TG* g, const float* __restrict__ x, const TrWalk& w, int lane, F one) {
  for (int i = lane; i < w.head; i += 64) st(g + i, one(i, x[i]));
  if (lane < w.ntail) st(g + w.tail0 + lane, one(w.tail0 + lane, x[w.tail0 + lane]));
  const float4* x4 = reinterpret_cast<const float4*>(x + w.head);
  for (int i = lane; i < w.n4; i += 64) {
    const float4 v = x4[i];
    const int e = w.head + 4 * i;
    const float r[4] = {one(e, v.x), one(e + 1, v.y), one(e + 2, v.z), one(e + 3, v.w)};
    st4(g + e, r);
  }
}

// costs[b] = -ll[b] * factor  (RNN-T: 1 + fastemit_lambda, rnnt_helper.compute_costs_data; TDT: 1)
static __global__ void tr_cost_kernel(const float* __restrict__ ll, float* __restrict__ costs, int B, float factor) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) costs[b] = -ll[b] * factor;
}

// ---- host side
// workspace of a loss call: `per_row` floats for every (b,t,u) row, then the forward and backward log-likelihoods
static inline long long tr_ws_elems(int per_row, int B, int T, int U1) { return (long long)per_row * B * T * U1 + 2LL * B; }

// launch geometry: the row kernels put 4 rows (waves) into a 256-thread workgroup, the lattice kernels one thread per u in whole waves
struct TrGeom { long long rows; unsigned nblk; int threads; };
static inline TrGeom tr_geom(int B, int T, int U1) {
  const long long rows = (long long)B * T * U1;
  return {rows, (unsigned)((rows + 3) / 4), ((U1 + 63) / 64) * 64};
}

// The argument checks both loss entries share: pointers, sizes, blank, the lattice kernels' U1 <= 1024, the pitches against the
// row width (V1, plus the duration logits for TDT), the bf16 gradient's pitch and alignment, the workspace and the grid limit of
// the row kernels.  0 or MI_ERR_ARG.
static inline int tr_check_args(const void* acts, long long ld, const void* labels, const void* act_lens, const void* label_lens,
                                int B, int T, int U1, int V1, int width, int blank, const void* costs, const void* grads,
                                int grads_dtype, long long ldg, const void* workspace, long long workspace_elems, int ws_per_row) {
  if (grads_dtype != MI_DT_F32 && grads_dtype != MI_DT_BF16) return MI_ERR_ARG;
  if (!acts || (!labels && U1 > 1) || !act_lens || !label_lens || !costs || !workspace) return MI_ERR_ARG;
  if (B <= 0 || T <= 0 || U1 <= 0 || V1 <= 1 || blank < 0 || blank >= V1 || U1 > 1024) return MI_ERR_ARG;
  if (ld < width || (grads && ldg < width)) return MI_ERR_ARG;
  if (grads && grads_dtype == MI_DT_BF16 && ((ldg & 7) || ((uintptr_t)grads & 15))) return MI_ERR_ARG;
  if (workspace_elems < tr_ws_elems(ws_per_row, B, T, U1)) return MI_ERR_ARG;
  if (((long long)B * T * U1 + 3) / 4 > 0x7fffffffLL) return MI_ERR_ARG;
  return MI_OK;
}

// Whether the gradient kernel may take the vector walk.  bf16 gradient: every logit row starts on a 16-byte boundary (then
// head = 0 and the 4-element groups of the bf16 row are 8-byte aligned as well).  f32 gradient: the rows of acts and grads share
// their alignment.
static inline int tr_vector_walk(const void* acts, long long ld, const void* grads, int grads_dtype, long long ldg) {
  const unsigned long long a = (unsigned long long)acts, g = (unsigned long long)grads;
  if (grads_dtype == MI_DT_BF16) return ((a & 15ull) == 0ull && (ld & 3) == 0) ? 1 : 0;
  return (((a ^ g) & 15ull) == 0ull && ((ld - ldg) & 3) == 0) ? 1 : 0;
}
