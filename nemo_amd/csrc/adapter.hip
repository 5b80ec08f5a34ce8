// Linear adapter of a Conformer layer (include/mi355x_asr.h, "linear adapters"), one launch forward, three backward:
//   n = LayerNorm(x),  h = W_down . n,  a = h * sigmoid(h),  y = x + W_up . a            x, y, dy, dx: f32 rows [M, d] with a pitch
// WT = bf16_t (weight images, v_mfma_f32_16x16x32_bf16 / 16x16x16) or float (masters, v_mfma_f32_16x16x4_f32).
//
// How the work is split.  A WAVE owns 16 rows; a workgroup is 1, 2 or 4 independent waves (as many as the LDS holds) and the grid
// walks the 16-row tiles persistently.  Both projections run TRANSPOSED -- the weight rows are the MFMA A operand, the 16 activation
// rows the B operand -- so a lane's four accumulator values are four CONSECUTIVE columns of ONE row: Swish'd hidden values go to LDS
// as one 8 / 16-byte store in the layout the next product reads, and x, dy, y, dx move as 16-byte vectors straight from / to the
// accumulator layout.  The hidden [16, dim] tile lives in LDS only.
// Weights are NOT staged in LDS: the widest supported geometry (d = 1024, dim = 64) has 128 KB per bf16 matrix, two of them do not
// fit beside the row tiles, while every matrix (<= 512 KB in f32) stays in L2 and a lane's fragment is one 16-byte load that is
// already in MFMA layout (the scheme of rnnt_mma.h).  Latency is covered by several workgroups per CU instead of a prefetch.
//
// Backward.  mi355x_adapter_bwd = (1) the row kernel: recomputes n, h, a from x, forms da = dy . W_up, dh = da * swish'(h),
// dn = dh . W_down and dx = dy + LN_bwd(dn) (dn is formed twice -- K = dim, cheap -- once for the two row sums, once for the store),
// and leaves a, dh [M, dimp] and the row statistics in the workspace (3 % of the traffic of x at dim = 32); (2) the column kernel:
// the weight and LayerNorm gradients have M as their K dimension, so a workgroup owns 32 COLUMNS of d and a slice of the rows, its
// lanes load the "k = row" operands directly (lane (c, g) reads rows 4g .. 4g+3 of column c: 64-byte segments per row), every wave
// keeps its dW_up / dW_down / dgamma / dbeta tiles in registers over its whole row loop, the four waves are then summed in wave
// order through LDS and the WORKGROUP writes one partial; (3) the reduce: sums the partials in index order into the f32 gradient buffers (+=).  No atomics anywhere: two runs give the same bits.
#include <atomic>
#include <initializer_list>
#include "rnnt_mma.h"

namespace {

constexpr int AD_MAXJ = 4;                   // 16-byte row chunks per lane: d <= 64 * 4 * AD_MAXJ = 1024
constexpr int AD_MAX_D = 64 * 4 * AD_MAXJ;
constexpr int AD_LDS_LIMIT = 160 * 1024;     // gfx950: 160 KB of LDS per workgroup
constexpr int AD_CSLICE = 32;                // columns of d per workgroup of the column kernel
constexpr int AD_MAXJT = 8;                  // dim <= 128 = 8 tiles of 16

template <typename WT> struct AdT { static constexpr int PAD = 16 / sizeof(WT); };   // 16 bytes: rows 4 banks apart

__host__ __device__ inline int ad_up(int v, int m) { return (v + m - 1) / m * m; }

template <typename WT> __device__ __forceinline__ void ad_store4(WT* p, float v0, float v1, float v2, float v3);
template <> __device__ __forceinline__ void ad_store4<float>(float* p, float v0, float v1, float v2, float v3) {
  *reinterpret_cast<float4*>(p) = make_float4(v0, v1, v2, v3);
}
template <> __device__ __forceinline__ void ad_store4<bf16_t>(bf16_t* p, float v0, float v1, float v2, float v3) {
  *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf2(v0, v1), pack_bf2(v2, v3));
}

// 16 x 16 x 16 product on four values per lane (k = 4g .. 4g+3 in both operands), rounded to WT here
typedef __attribute__((ext_vector_type(4))) short ad_s16x4;
template <typename WT> __device__ __forceinline__ f32x4 ad_mk16(const float (&a)[4], const float (&b)[4], f32x4 c);
template <> __device__ __forceinline__ f32x4 ad_mk16<bf16_t>(const float (&a)[4], const float (&b)[4], f32x4 c) {
  const u32x2 pa = {pack_bf2(a[0], a[1]), pack_bf2(a[2], a[3])}, pb = {pack_bf2(b[0], b[1]), pack_bf2(b[2], b[3])};
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(ad_s16x4, pa), __builtin_bit_cast(ad_s16x4, pb), c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x4 ad_mk16<float>(const float (&a)[4], const float (&b)[4], f32x4 c) {
#pragma unroll
  for (int i = 0; i < 4; ++i) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[i], c, 0, 0, 0);
  return c;
}

// acc[r][n] = sum_k A[r][k] * B[n][k], k < Kp: A row `arow` (global, or nullptr for a zero row; k valid below ka), B row `brow` (LDS,
// zero-filled up to Kp).  The lane holds acc[4g + i][lane % 16].
template <typename WT>
__device__ __forceinline__ f32x4 ad_mma(const WT* arow, int ka, const WT* brow, int Kp) {
  constexpr int KB = RbT<WT>::KB;
  const int kq = ((threadIdx.x & 63) >> 4) * RbT<WT>::V;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int kb = 0; kb < Kp; kb += KB) {
    const int k = kb + kq;
    const u32x4 a = (arow && k < ka) ? *reinterpret_cast<const u32x4*>(arow + k) : zero;
    const u32x4 b = *reinterpret_cast<const u32x4*>(brow + k);
    acc = rb_mfma<WT>(a, b, acc);
  }
  return acc;
}

// rows m0 .. m0+15 of x -> LayerNorm -> tile [16][pitch] (WT) in LDS, zero beyond d (up to Kp) and for rows >= M; every lane leaves
// with the mean / rstd of row m0 + lane % 16.  Four rows at a time, a row's values stay in registers between the two reductions.
template <typename WT>
__device__ __forceinline__ void ad_norm_tile(const float* __restrict__ x, long long ldx, const float* __restrict__ gamma,
                                             const float* __restrict__ beta, int m0, int M, int d, int Kp, float eps, WT* tile,
                                             int pitch, float& my_mean, float& my_rstd) {
  const int lane = threadIdx.x & 63;
  const float inv_d = 1.f / (float)d;
  for (int r0 = 0; r0 < 16; r0 += 4) {
    float4 v[4][AD_MAXJ];
    float s[4], q[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int m = m0 + r0 + rr;
      s[rr] = 0.f;
#pragma unroll
      for (int j = 0; j < AD_MAXJ; ++j) {
        const int c = (lane + 64 * j) * 4;
        v[rr][j] = (m < M && c < d) ? *reinterpret_cast<const float4*>(x + (long long)m * ldx + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        s[rr] += (v[rr][j].x + v[rr][j].y) + (v[rr][j].z + v[rr][j].w);
      }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) s[rr] = wave_sum(s[rr]) * inv_d;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      q[rr] = 0.f;
#pragma unroll
      for (int j = 0; j < AD_MAXJ; ++j) {
        if ((lane + 64 * j) * 4 < d) {
          const float a = v[rr][j].x - s[rr], b = v[rr][j].y - s[rr], c = v[rr][j].z - s[rr], e = v[rr][j].w - s[rr];
          q[rr] += (a * a + b * b) + (c * c + e * e);
        }
      }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) q[rr] = rsqrtf(wave_sum(q[rr]) * inv_d + eps);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const bool row = m0 + r0 + rr < M;
#pragma unroll
      for (int j = 0; j < AD_MAXJ; ++j) {
        const int c = (lane + 64 * j) * 4;
        if (c < Kp) {
          float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
          if (row && c < d) {
            const float4 g = *reinterpret_cast<const float4*>(gamma + c), b = *reinterpret_cast<const float4*>(beta + c);
            o.x = (v[rr][j].x - s[rr]) * q[rr] * g.x + b.x; o.y = (v[rr][j].y - s[rr]) * q[rr] * g.y + b.y;
            o.z = (v[rr][j].z - s[rr]) * q[rr] * g.z + b.z; o.w = (v[rr][j].w - s[rr]) * q[rr] * g.w + b.w;
          }
          ad_store4<WT>(tile + (r0 + rr) * pitch + c, o.x, o.y, o.z, o.w);
        }
      }
      if ((lane & 15) == r0 + rr) { my_mean = s[rr]; my_rstd = q[rr]; }
    }
  }
}

struct AdP {
  const float* x; const float* dy; const float* gamma; const float* beta;
  const void* wd; const void* wu; const void* wdt; const void* wut;   // W_down [dim, d], W_up [d, dim] and their transposes
  float* y;                                                            // forward: y; backward: dx
  void* a_ws; void* dh_ws; float* mean; float* rstd; float* partial;
  long long ldx, lddy, ldy, ld_wd, ld_wu, ld_wdt, ld_wut, E;
  int M, d, dim, ntiles, P;
  float eps;
};

// LDS of one wave: the [16][Kp + PAD] row tile, the [16][dp + PAD] hidden tile (WT) and, backward, h [16][dp] in f32
template <typename WT> size_t ad_wave_lds(int d, int dim, bool bwd) {
  const int KB = RbT<WT>::KB, PAD = AdT<WT>::PAD, Kp = ad_up(d, KB), dp = ad_up(dim, KB);
  return (size_t)16 * (Kp + PAD) * sizeof(WT) + (size_t)16 * (dp + PAD) * sizeof(WT) + (bwd ? (size_t)16 * dp * sizeof(float) : 0);
}

template <typename WT, bool BWD>
__global__ __launch_bounds__(256) void adapter_rows_kernel(AdP p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ad_smem[];
  constexpr int KB = RbT<WT>::KB, PAD = AdT<WT>::PAD;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6, l16 = lane & 15, g4 = (lane >> 4) * 4;
  const int d = p.d, dim = p.dim, M = p.M, Kp = ad_up(d, KB), dp = ad_up(dim, KB), p1 = Kp + PAD, p2 = dp + PAD;
  const size_t per_wave = (size_t)16 * p1 * sizeof(WT) + (size_t)16 * p2 * sizeof(WT) + (BWD ? (size_t)16 * dp * sizeof(float) : 0);
  WT* t1 = reinterpret_cast<WT*>(ad_smem + w * per_wave);
  WT* t2 = t1 + 16 * p1;
  float* ht = reinterpret_cast<float*>(t2 + 16 * p2);
  const WT* wd = (const WT*)p.wd;
  const int nct = (d + 15) >> 4;
  for (int tile = blockIdx.x * nw + w; tile < p.ntiles; tile += gridDim.x * nw) {
    const int m0 = tile * 16, m = m0 + l16;
    float mean = 0.f, rstd = 0.f;
    ad_norm_tile<WT>(p.x, p.ldx, p.gamma, p.beta, m0, M, d, Kp, p.eps, t1, p1, mean, rstd);
    // ---- down-projection: h[j][m], Swish in the accumulators
    for (int jt = 0; jt < dp / 16; ++jt) {
      const int j = jt * 16 + l16;
      const f32x4 h = ad_mma<WT>(j < dim ? wd + (long long)j * p.ld_wd : nullptr, d, t1 + l16 * p1, Kp);
      const float a0 = swishf_(h[0]), a1 = swishf_(h[1]), a2 = swishf_(h[2]), a3 = swishf_(h[3]);
      if (!BWD) {
        ad_store4<WT>(t2 + l16 * p2 + jt * 16 + g4, a0, a1, a2, a3);
      } else {
        *reinterpret_cast<float4*>(ht + l16 * dp + jt * 16 + g4) = make_float4(h[0], h[1], h[2], h[3]);
        if (m < M) ad_store4<WT>((WT*)p.a_ws + (long long)m * dp + jt * 16 + g4, a0, a1, a2, a3);
      }
    }
    if (!BWD) {
      // ---- up-projection: u[c][m]; y = x + u as 16-byte vectors
      const WT* wu = (const WT*)p.wu;
#pragma unroll 2
      for (int ct = 0; ct < nct; ++ct) {
        const int c = ct * 16 + l16, cc = ct * 16 + g4;
        const f32x4 u = ad_mma<WT>(c < d ? wu + (long long)c * p.ld_wu : nullptr, dim, t2 + l16 * p2, dp);
        if (m < M && cc < d) {
          const float4 xv = *reinterpret_cast<const float4*>(p.x + (long long)m * p.ldx + cc);
          *reinterpret_cast<float4*>(p.y + (long long)m * p.ldy + cc) = make_float4(xv.x + u[0], xv.y + u[1], xv.z + u[2], xv.w + u[3]);
        }
      }
    } else {
      // ---- dy rows -> t1 (n is not needed any more), rounded to WT
      for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int jj = 0; jj < AD_MAXJ; ++jj) {
          const int c = (lane + 64 * jj) * 4;
          if (c < Kp) {
            const float4 v = (m0 + r < M && c < d) ? *reinterpret_cast<const float4*>(p.dy + (long long)(m0 + r) * p.lddy + c)
                                                   : make_float4(0.f, 0.f, 0.f, 0.f);
            ad_store4<WT>(t1 + r * p1 + c, v.x, v.y, v.z, v.w);
          }
        }
      }
      // ---- da[j][m] = sum_c W_up[c][j] dy[m][c];  dh = da * swish'(h)
      const WT* wut = (const WT*)p.wut;
      for (int jt = 0; jt < dp / 16; ++jt) {
        const int j = jt * 16 + l16;
        const f32x4 da = ad_mma<WT>(j < dim ? wut + (long long)j * p.ld_wut : nullptr, d, t1 + l16 * p1, Kp);
        const float4 h = *reinterpret_cast<const float4*>(ht + l16 * dp + jt * 16 + g4);
        const float e0 = da[0] * swish_grad(h.x), e1 = da[1] * swish_grad(h.y), e2 = da[2] * swish_grad(h.z), e3 = da[3] * swish_grad(h.w);
        ad_store4<WT>(t2 + l16 * p2 + jt * 16 + g4, e0, e1, e2, e3);
        if (m < M) ad_store4<WT>((WT*)p.dh_ws + (long long)m * dp + jt * 16 + g4, e0, e1, e2, e3);
      }
      // ---- dn[c][m] = sum_j W_down[j][c] dh[m][j];  t = dn * gamma;  dx = dy + rstd * (t - mean(t) - nhat * mean(t * nhat))
      const WT* wdt = (const WT*)p.wdt;
      float s1 = 0.f, s2 = 0.f;
      for (int pass = 0; pass < 2; ++pass) {
#pragma unroll 2
        for (int ct = 0; ct < nct; ++ct) {
          const int c = ct * 16 + l16, cc = ct * 16 + g4;
          const f32x4 dn = ad_mma<WT>(c < d ? wdt + (long long)c * p.ld_wdt : nullptr, dim, t2 + l16 * p2, dp);
          if (m < M && cc < d) {
            const float4 gm = *reinterpret_cast<const float4*>(p.gamma + cc);
            const float4 xv = *reinterpret_cast<const float4*>(p.x + (long long)m * p.ldx + cc);
            const float t0 = dn[0] * gm.x, t1v = dn[1] * gm.y, t2v = dn[2] * gm.z, t3 = dn[3] * gm.w;
            const float n0 = (xv.x - mean) * rstd, n1 = (xv.y - mean) * rstd, n2 = (xv.z - mean) * rstd, n3 = (xv.w - mean) * rstd;
            if (pass == 0) {
              s1 += (t0 + t1v) + (t2v + t3);
              s2 += (t0 * n0 + t1v * n1) + (t2v * n2 + t3 * n3);
            } else {
              const float4 dyv = *reinterpret_cast<const float4*>(p.dy + (long long)m * p.lddy + cc);
              *reinterpret_cast<float4*>(p.y + (long long)m * p.ldy + cc) =
                  make_float4(dyv.x + rstd * (t0 - s1 - n0 * s2), dyv.y + rstd * (t1v - s1 - n1 * s2),
                              dyv.z + rstd * (t2v - s1 - n2 * s2), dyv.w + rstd * (t3 - s1 - n3 * s2));
            }
          }
        }
        if (pass == 0) {   // the four lane groups hold the four quarters of a row's columns
          s1 += __shfl_xor(s1, 16, 64); s1 += __shfl_xor(s1, 32, 64);
          s2 += __shfl_xor(s2, 16, 64); s2 += __shfl_xor(s2, 32, 64);
          s1 *= 1.f / (float)d; s2 *= 1.f / (float)d;
        }
      }
      if (lane < 16 && m < M) { p.mean[m] = mean; p.rstd[m] = rstd; }
    }
  }
}

// the four waves of a column workgroup hold the same lane -> element map: `PUT` parks a wave's accumulators in LDS ([value][lane],
// conflict-free), !PUT adds the parked ones to this wave's
template <bool PUT>
__device__ __forceinline__ void ad_xwave(float* xw, int lane, int njt, f32x4 (&up)[2][AD_MAXJT], f32x4 (&dw)[AD_MAXJT][2],
                                         float (&dg)[2], float (&db)[2]) {
  auto mv = [&](float v, int k) -> float {
    if (PUT) { xw[k * 64 + lane] = v; return v; }
    return v + xw[k * 64 + lane];
  };
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    dg[ct] = mv(dg[ct], ct); db[ct] = mv(db[ct], 2 + ct);
#pragma unroll
    for (int jt = 0; jt < AD_MAXJT; ++jt) {
      if (jt < njt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int k = 4 + ((ct * AD_MAXJT + jt) * 4 + i) * 2;
          up[ct][jt][i] = mv(up[ct][jt][i], k); dw[jt][ct][i] = mv(dw[jt][ct][i], k + 1);
        }
      }
    }
  }
}

// Column kernel: workgroup (cs, s) = columns cs*32 .. +31 of d; its wave w walks the 16-row tiles s*4 + w, s*4 + w + P, ... with its
// tiles in registers, then the four waves are summed in wave order through LDS and the workgroup writes ONE partial,
// partial[s]: dW_down [dim, d] | dW_up [d, dim] | dgamma [d] | dbeta [d]; the workgroups of one s cover every element once.
template <typename WT>
__global__ __launch_bounds__(256) void adapter_cols_kernel(AdP p) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l16 = lane & 15, g4 = (lane >> 4) * 4;
  const int d = p.d, dim = p.dim, M = p.M, dp = ad_up(dim, RbT<WT>::KB), njt = (dim + 15) >> 4;
  const int q = blockIdx.y * 4 + w, c0 = blockIdx.x * AD_CSLICE;
  const WT* a_ws = (const WT*)p.a_ws;
  const WT* dh_ws = (const WT*)p.dh_ws;
  const WT* wdt = (const WT*)p.wdt;
  f32x4 up[2][AD_MAXJT], dw[AD_MAXJT][2];
  float dg[2] = {0.f, 0.f}, db[2] = {0.f, 0.f}, gam[2], bet[2];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int c = c0 + ct * 16 + l16;
    gam[ct] = c < d ? p.gamma[c] : 0.f; bet[ct] = c < d ? p.beta[c] : 0.f;
#pragma unroll
    for (int jt = 0; jt < AD_MAXJT; ++jt) { up[ct][jt] = f32x4{0.f, 0.f, 0.f, 0.f}; dw[jt][ct] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  }
  for (int tile = q; tile < p.ntiles; tile += p.P) {
    const int m0 = tile * 16;
    float dyv[2][4], nh[2][4], xn[2][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + g4 + i;
      const bool ok = m < M;
      const float mu = ok ? p.mean[m] : 0.f, rs = ok ? p.rstd[m] : 0.f;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const int c = c0 + ct * 16 + l16;
        const bool in = ok && c < d;
        const float xv = in ? p.x[(long long)m * p.ldx + c] : 0.f;
        dyv[ct][i] = in ? p.dy[(long long)m * p.lddy + c] : 0.f;
        nh[ct][i] = in ? (xv - mu) * rs : 0.f;
        xn[ct][i] = in ? (xv - mu) * rs * gam[ct] + bet[ct] : 0.f;
      }
    }
#pragma unroll
    for (int jt = 0; jt < AD_MAXJT; ++jt) {
      if (jt < njt) {
        float av[4], dhv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = m0 + g4 + i;
          av[i] = m < M ? ld<WT>(a_ws + (long long)m * dp + jt * 16 + l16) : 0.f;
          dhv[i] = m < M ? ld<WT>(dh_ws + (long long)m * dp + jt * 16 + l16) : 0.f;
        }
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          up[ct][jt] = ad_mk16<WT>(dyv[ct], av, up[ct][jt]);     // dW_up[c][j]   += dy[m][c] a[m][j]
          dw[jt][ct] = ad_mk16<WT>(dhv, xn[ct], dw[jt][ct]);     // dW_down[j][c] += dh[m][j] n[m][c]
        }
      }
    }
    // dn[m][c] again for this column slice (rows of the tile are the A operand): dgamma += dn * nhat, dbeta += dn
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const int c = c0 + ct * 16 + l16;
      f32x4 dn = {0.f, 0.f, 0.f, 0.f};
      for (int kb = 0; kb < njt * 16; kb += 16) {
        float av[4], bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int k = kb + g4 + i;
          av[i] = m0 + l16 < M ? ld<WT>(dh_ws + (long long)(m0 + l16) * dp + k) : 0.f;
          bv[i] = (c < d && k < dim) ? ld<WT>(wdt + (long long)c * p.ld_wdt + k) : 0.f;
        }
        dn = ad_mk16<WT>(av, bv, dn);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) { dg[ct] += dn[i] * nh[ct][i]; db[ct] += dn[i]; }
    }
  }
  __shared__ float xw[(4 + 16 * AD_MAXJT) * 64];
  for (int ww = 1; ww < 4; ++ww) {
    if (w == ww) ad_xwave<true>(xw, lane, njt, up, dw, dg, db);
    __syncthreads();
    if (w == 0) ad_xwave<false>(xw, lane, njt, up, dw, dg, db);
    __syncthreads();
  }
  if (w != 0) return;
  float* part = p.partial + (long long)blockIdx.y * p.E;
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    dg[ct] += __shfl_xor(dg[ct], 16, 64); dg[ct] += __shfl_xor(dg[ct], 32, 64);
    db[ct] += __shfl_xor(db[ct], 16, 64); db[ct] += __shfl_xor(db[ct], 32, 64);
    const int c = c0 + ct * 16 + l16;
    if (lane < 16 && c < d) { part[2LL * dim * d + c] = dg[ct]; part[2LL * dim * d + d + c] = db[ct]; }
#pragma unroll
    for (int jt = 0; jt < AD_MAXJT; ++jt) {
      if (jt < njt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int cu = c0 + ct * 16 + g4 + i, ju = jt * 16 + l16;   // up[ct][jt][i] = dW_up[cu][ju]
          if (cu < d && ju < dim) part[(long long)dim * d + (long long)cu * dim + ju] = up[ct][jt][i];
          const int jd = jt * 16 + g4 + i;                            // dw[jt][ct][i] = dW_down[jd][c]
          if (jd < dim && c < d) part[(long long)jd * d + c] = dw[jt][ct][i];
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void adapter_reduce_kernel(const float* __restrict__ partial, int P, long long E, int dim, int d,
                                                             float* __restrict__ d_wd, float* __restrict__ d_wu,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x, n = (long long)dim * d;
  if (e >= E) return;
  float s = 0.f;
  for (int q = 0; q < P; ++q) s += partial[q * E + e];
  float* t = e < n ? d_wd + e : e < 2 * n ? d_wu + (e - n) : e < 2 * n + d ? dgamma + (e - 2 * n) : dbeta + (e - 2 * n - d);
  *t += s;
}

struct AdPlan {
  int P, S, ntiles;
  long long E;
  size_t off_rstd, off_a, off_dh, off_part, bytes;
};
bool ad_aligned(std::initializer_list<const void*> ps) {
  for (const void* q : ps)
    if (!q || ((uintptr_t)q & 15)) return false;
  return true;
}
bool ad_geometry_ok(long long M, int d, int dim, int dtype) {
  if (dtype != MI_DT_F32 && dtype != MI_DT_BF16) return false;
  if (M < 1 || M > (1LL << 30) || d < 1 || d > AD_MAX_D || d % (dtype == MI_DT_BF16 ? 8 : 4)) return false;
  return dim >= 8 && dim <= 128 && dim % 8 == 0;
}
AdPlan ad_plan(long long M, int d, int dim, int dtype) {
  AdPlan pl;
  const size_t es = dtype == MI_DT_BF16 ? 2 : 4;
  const int dp = ad_up(dim, dtype == MI_DT_BF16 ? 32 : 16);
  pl.ntiles = (int)((M + 15) / 16);
  const int ncs = (d + AD_CSLICE - 1) / AD_CSLICE;
  int S = 512 / ncs;                       // about two workgroups per CU of the column kernel
  S = S > 32 ? 32 : S;
  const int by_rows = (pl.ntiles + 3) / 4;
  S = S > by_rows ? by_rows : S;
  pl.S = S < 1 ? 1 : S;
  pl.P = pl.S * 4;
  pl.E = 2LL * dim * d + 2LL * d;
  auto al = [](size_t v) { return (v + 255) / 256 * 256; };
  pl.off_rstd = al((size_t)M * 4);
  pl.off_a = pl.off_rstd + al((size_t)M * 4);
  pl.off_dh = pl.off_a + al((size_t)M * dp * es);
  pl.off_part = pl.off_dh + al((size_t)M * dp * es);
  pl.bytes = pl.off_part + (size_t)pl.S * pl.E * 4;   // one partial per column workgroup row s
  return pl;
}

// waves per workgroup (4, 2 or 1) whose tiles fit the LDS, 0: not even one
template <typename WT> int ad_waves(int d, int dim, bool bwd) {
  for (int nw = 4; nw >= 1; nw >>= 1)
    if (nw * ad_wave_lds<WT>(d, dim, bwd) <= (size_t)AD_LDS_LIMIT) return nw;
  return 0;
}

// CUs of the current device, asked once (0 until then)
int ad_cus() {
  static std::atomic<int> cus{0};
  int n = cus.load(std::memory_order_relaxed);
  if (n <= 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    cus.store(n, std::memory_order_relaxed);
  }
  return n;
}

template <typename WT, bool BWD> int ad_launch_rows(const AdP& p, int nw, hipStream_t s) {
  const size_t shm = nw * ad_wave_lds<WT>(p.d, p.dim, BWD);
  auto fn = adapter_rows_kernel<WT, BWD>;
  // the dynamic-LDS ceiling of this kernel is raised to the limit once (0 = not yet, 1 = set, 2 = refused), not per launch
  static std::atomic<int> attr{0};
  int st = attr.load(std::memory_order_acquire);
  if (!st) {
    st = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, AD_LDS_LIMIT) == hipSuccess ? 1 : 2;
    attr.store(st, std::memory_order_release);
  }
  if (st == 2) return MI_ERR_LAUNCH;
  const int wgs = (p.ntiles + nw - 1) / nw;
  const int fit = (int)(AD_LDS_LIMIT / shm), per_cu = fit > 4 ? 4 : fit;   // persistent: what the LDS lets a CU hold, at most 4
  const int cap = ad_cus() * per_cu, grid = wgs < cap ? wgs : cap;
  MI_LAUNCH(fn, dim3(grid), dim3(64 * nw), shm, s, p);
  return MI_OK;
}

}  // namespace

extern "C" long long mi355x_adapter_workspace_bytes(long long M, int d, int dim, int dtype) {
  if (!ad_geometry_ok(M, d, dim, dtype)) return -1;
  return (long long)ad_plan(M, d, dim, dtype).bytes;
}

extern "C" int mi355x_adapter_fwd(const void* x, long long ldx, const void* gamma, const void* beta, const void* w_down,
                                  long long ld_down, const void* w_up, long long ld_up, void* y, long long ldy, long long M, int d,
                                  int dim, int dtype, float eps, void* stream) {
  mi_clear_errors();
  if (!ad_aligned({x, gamma, beta, w_down, w_up, y}) || !ad_geometry_ok(M, d, dim, dtype)) return MI_ERR_ARG;
  const int wa = dtype == MI_DT_BF16 ? 8 : 4;
  if (ldx < d || ldy < d || ld_down < d || ld_up < dim || ldx % 4 || ldy % 4 || ld_down % wa || ld_up % wa) return MI_ERR_ARG;
  const int nw = dtype == MI_DT_BF16 ? ad_waves<bf16_t>(d, dim, false) : ad_waves<float>(d, dim, false);
  if (nw == 0) return MI_ERR_ARG;
  AdP p = {};
  p.x = (const float*)x; p.gamma = (const float*)gamma; p.beta = (const float*)beta; p.wd = w_down; p.wu = w_up; p.y = (float*)y;
  p.ldx = ldx; p.ldy = ldy; p.ld_wd = ld_down; p.ld_wu = ld_up;
  p.M = (int)M; p.d = d; p.dim = dim; p.ntiles = (int)((M + 15) / 16); p.eps = eps;
  const int rc = dtype == MI_DT_BF16 ? ad_launch_rows<bf16_t, false>(p, nw, (hipStream_t)stream)
                                     : ad_launch_rows<float, false>(p, nw, (hipStream_t)stream);
  return rc != MI_OK ? rc : mi_check_launch();
}

extern "C" int mi355x_adapter_bwd(const void* x, long long ldx, const void* dy, long long lddy, const void* gamma, const void* beta,
                                  const void* w_down, long long ld_down, const void* w_up_t, long long ld_up_t, const void* w_down_t,
                                  long long ld_down_t, void* dx, long long lddx, void* d_w_down, void* d_w_up, void* dgamma,
                                  void* dbeta, void* workspace, long long workspace_bytes, long long M, int d, int dim, int dtype,
                                  float eps, void* stream) {
  mi_clear_errors();
  if (!ad_aligned({x, dy, gamma, beta, w_down, w_up_t, w_down_t, dx, workspace}) || !d_w_down || !d_w_up || !dgamma || !dbeta ||
      !ad_geometry_ok(M, d, dim, dtype))
    return MI_ERR_ARG;
  const int wa = dtype == MI_DT_BF16 ? 8 : 4;
  if (ldx < d || lddy < d || lddx < d || ld_down < d || ld_up_t < d || ld_down_t < dim || ldx % 4 || lddy % 4 || lddx % 4 ||
      ld_down % wa || ld_up_t % wa || ld_down_t % wa)
    return MI_ERR_ARG;
  const AdPlan pl = ad_plan(M, d, dim, dtype);
  if (workspace_bytes < (long long)pl.bytes) return MI_ERR_ARG;
  const int nw = dtype == MI_DT_BF16 ? ad_waves<bf16_t>(d, dim, true) : ad_waves<float>(d, dim, true);
  if (nw == 0) return MI_ERR_ARG;
  char* ws = (char*)workspace;
  AdP p = {};
  p.x = (const float*)x; p.dy = (const float*)dy; p.gamma = (const float*)gamma; p.beta = (const float*)beta;
  p.wd = w_down; p.wut = w_up_t; p.wdt = w_down_t; p.y = (float*)dx;
  p.mean = (float*)ws; p.rstd = (float*)(ws + pl.off_rstd); p.a_ws = ws + pl.off_a; p.dh_ws = ws + pl.off_dh;
  p.partial = (float*)(ws + pl.off_part);
  p.ldx = ldx; p.lddy = lddy; p.ldy = lddx; p.ld_wd = ld_down; p.ld_wut = ld_up_t; p.ld_wdt = ld_down_t; p.E = pl.E;
  p.M = (int)M; p.d = d; p.dim = dim; p.ntiles = pl.ntiles; p.P = pl.P; p.eps = eps;
  hipStream_t s = (hipStream_t)stream;
  const bool bf = dtype == MI_DT_BF16;
  const int rc = bf ? ad_launch_rows<bf16_t, true>(p, nw, s) : ad_launch_rows<float, true>(p, nw, s);
  if (rc != MI_OK) return rc;
  const dim3 cgrid((d + AD_CSLICE - 1) / AD_CSLICE, pl.S);
  if (bf) MI_LAUNCH(adapter_cols_kernel<bf16_t>, cgrid, dim3(256), 0, s, p);
  else MI_LAUNCH(adapter_cols_kernel<float>, cgrid, dim3(256), 0, s, p);
  MI_LAUNCH(adapter_reduce_kernel, dim3((unsigned)((pl.E + 255) / 256)), dim3(256), 0, s, p.partial, pl.S, pl.E, dim, d,
            (float*)d_w_down, (float*)d_w_up, (float*)dgamma, (float*)dbeta);
  return mi_check_launch();
}
