// Device helpers shared by the fused rel-pos attention kernels (attention.hip: unlimited context; attention_ctx.hip: limited /
// local context): LDS-DMA staging, MFMA fragment reads, the dropout definition and the tile constants.
#pragma once
#include "common.h"

typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void glb_void_t;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4_t;

typedef __attribute__((address_space(3))) const char lds_cchar_t;
__device__ __forceinline__ uint32_t lds_addr(const void* p) { return (uint32_t)(uintptr_t)(lds_cchar_t*)p; }

// LDS-DMA by inline asm.  Behind a `__builtin_amdgcn_global_load_lds` hipcc puts `s_waitcnt vmcnt(0)` in front of LDS reads
// it cannot tell apart from the DMA's target (transpose reads, merged reads, ...): a prefetch issued at the top of a step was
// waited for at the step's first such read.  Issued by hand the compiler knows nothing about the transfer; every consumer in
// this file sits behind an explicit `s_waitcnt vmcnt` + barrier anyway.  lds_base must be wave-uniform (lane i lands at
// lds_base + 16 i).  M0 is not used by anything else in this translation unit.
__device__ __forceinline__ void dma16(const void* src, const void* lds_base) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off"
               :
               : "v"(src), "s"(__builtin_amdgcn_readfirstlane(lds_addr(lds_base)))
               : "memory");
}

__device__ __forceinline__ void dma4(const void* src, const void* lds_base) {  // lane i lands at lds_base + 4 i
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off"
               :
               : "v"(src), "s"(__builtin_amdgcn_readfirstlane(lds_addr(lds_base)))
               : "memory");
}

// head width: a template parameter of every kernel (ADK = 64: the tuned form, two workgroups per CU; ADK = 128 -- round 5, heads of
// 65..128 lanes zero-padded to 128, Squeezeformer-Medium's d_k = 81 -- the same code with 8 k-steps, 4 output tiles and one
// workgroup per CU).  Rows of every staged tile are ADK elements = ADK / 8 sixteen-byte chunks.
#define ABQ 128          // queries per workgroup (4 waves x 32)
#define ABK 32           // keys per step
#define ABAND (ABQ + ABK)  // positional band rows staged per step (159 needed)
#define SG_LD 66
#define APRING 6         // positional-band ring: blocks of 32 rows (5 in use + 1 being staged)

// Dropout of attention probabilities: keep(b,h,i,j) from full-rate integer ops only (v_mul_u32_u24, shifts, xors) so that
// it costs the same whether a lane walks keys (forward / dQ: lane = query) or queries (dK/dV: lane = key).  `akey` is a
// strong hash of (seed, site, b, h) computed once per workgroup.
__device__ __forceinline__ uint32_t attn_key(const DropCfg& d, int b, int h) {
  return mix32(mix32(d.key ^ (uint32_t)(b * 0x632BE5AB)) + (uint32_t)h * 0x9E3779B9u);
}
// Dropout on the attention probabilities, counter-based and two-level; the three loops are VALU-bound, so the definition is
// shaped by what it costs per element in BOTH register layouts ("lane = query" walking keys: forward / dQ; "lane = key"
// walking queries: dK/dV) -- 5.5 VALU ops per element where the first version needed 22 and the second 10.75:
//   * every 4x4 block (bi = i>>2, bj = j>>2) of the [T,T] matrix gets a seed = one multiply-add round over R(bi) ^ C(bj).
//     R and C are full mix32 hashes: the one that is constant per lane is hoisted out of the loop, the one that changes per
//     step is wave-uniform up to the lane-half bit, so both candidates are computed on the SCALAR unit and selected (1 op);
//   * a pair of horizontally adjacent elements (i, j&~1), (i, j|1) shares y = t ^ (t >> 15), t = seed + ((i&3)*2 + ((j&3)>>1)) * G;
//     the even column keeps iff mul24(y, KA) >= threshold, the odd one iff mul24(y, KB) >= threshold (two different odd 24-bit
//     multipliers: exhaustively over the 2^24 values of y the two decisions are independent to 1e-5, tools/attn_drop_stats.py).
//     "Lane = query" layouts need both decisions of a pair (5 ops per 2 elements), "lane = key" layouts one of them with the
//     multiplier chosen per lane (4 ops per element);
//   * the 1/(1-p) scale is not applied per element: forward folds it into the final normalisation, the backward kernels into
//     constants / the accumulators.
// attn_drop() is the scalar definition.
#define ADROP_G 0x9E3779B9u
#define ADROP_KA 0x2C1B3Du
#define ADROP_KB 0x5A2D39u
__device__ __forceinline__ uint32_t adrop_rcode(uint32_t akey, uint32_t bi) { return mix32(akey + bi * 0x9E3779B9u); }
__device__ __forceinline__ uint32_t adrop_ccode(uint32_t bj) { return mix32(bj * 0x85EBCA6Bu + 0x165667B1u); }
__device__ __forceinline__ uint32_t adrop_seed(uint32_t x) { return __umul24(x, 0x846CA7u) + (x >> 13); }  // v_mad_u32_u24
__device__ __forceinline__ uint32_t adrop_y(uint32_t t) { return t ^ (t >> 15); }
__device__ __forceinline__ bool attn_keep(const DropCfg& d, uint32_t akey, int i, int j) {
  if (d.threshold == 0u) return true;
  const uint32_t seed = adrop_seed(adrop_rcode(akey, (uint32_t)i >> 2) ^ adrop_ccode((uint32_t)j >> 2));
  const uint32_t y = adrop_y(seed + (uint32_t)((i & 3) * 2 + ((j & 3) >> 1)) * ADROP_G);
  return __umul24(y, (j & 1) ? ADROP_KB : ADROP_KA) >= d.threshold;
}
__device__ __forceinline__ float attn_drop(const DropCfg& d, uint32_t akey, int i, int j) {
  return attn_keep(d, akey, i, j) ? d.scale : 0.f;
}

template <int ADK>
__device__ __forceinline__ int a_off(int r, int chunk) { return r * ADK + ((chunk ^ ((r >> 1) & 7)) << 3); }

// rows [row0, row0+nrows) x 64 columns (col offset applied by caller) -> LDS image [nrows][64] with the (row>>1)&7 swizzle
// applied on the source side; rows are clamped into [0, rmax]; nchunks = rows * (ADK / 8)
template <int ADK>
__device__ __forceinline__ void stage_rows(const bf16_t* base, long long ld, int row0, int rmax, bf16_t* lds, int nchunks) {
  constexpr int NCH = ADK / 8;
  const int wave = threadIdx.x >> 6;
  for (int q0 = 0; q0 < nchunks; q0 += 256) {
    const int q = q0 + threadIdx.x;
    if (q0 + wave * 64 < nchunks) {  // wave-uniform
      const int r = q / NCH, ck = q % NCH;
      const int gck = ck ^ ((r >> 1) & 7);
      int gr = row0 + r;
      gr = gr < 0 ? 0 : (gr > rmax ? rmax : gr);
      // rows and pitches are far below 2^24 (the batch offset is in `base`): one full-rate 24-bit multiply instead of the
      // 64-bit sequence (2 quarter-rate v_mul_lo_u32 + v_mad_u64_u32) per address
      const bf16_t* src = base + __mul24(gr, (int)ld) + gck * 8;
      bf16_t* dst = lds + (q0 + wave * 64) * 8;
      dma16(src, dst);
    }
  }
}
// V tile [32 keys][ADK dv] kept exactly as in memory (for the transpose read), chunk swizzle c ^= (k&3)<<1
template <int ADK>
__device__ __forceinline__ void stage_v(const bf16_t* base, long long ld, int row0, int rmax, bf16_t* lds) {
  constexpr int NCH = ADK / 8;
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int q0 = 0; q0 < 32 * NCH; q0 += 256) {  // 256 chunks per pass
    const int q = q0 + threadIdx.x;
    const int k = q / NCH, cp = q % NCH;
    const int c = cp ^ ((k & 3) << 1);
    int gr = row0 + k;
    gr = gr > rmax ? rmax : gr;
    const bf16_t* src = base + __mul24(gr, (int)ld) + c * 8;
    bf16_t* dst = lds + (q0 + wave * 64) * 8;
    dma16(src, dst);
  }
}
// A fragment of V^T for the P.V product: lane (dv = dv0 + (lane&31)) gets V[key slots of (s, half)][dv]
template <int ADK>
__device__ __forceinline__ bf16x8 vt_frag(const bf16_t* vt, int dv0, int s, int lane) {
  const int t = lane & 15, g4 = (lane >> 4) & 1, lh = lane >> 5;
  const int col = dv0 + g4 * 16 + (t & 3) * 4;
  union { bf16x8 v; s16x4 h[2]; } u;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int krow = 16 * s + 8 * r + 4 * lh + (t >> 2);  // keys (4*lh + 0..3) and (8 + 4*lh + 0..3) of K16 step s
    const int off = krow * ADK + (((col >> 3) ^ ((krow & 3) << 1)) << 3) + (col & 7);
    u.h[r] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(vt + off));
  }
  return u.v;
}

__device__ __forceinline__ bf16x8 pack8(const float* v) {
  union { bf16x8 v; uint32_t w[4]; } u;
#pragma unroll
  for (int j = 0; j < 4; ++j) u.w[j] = pack_bf2(v[2 * j], v[2 * j + 1]);
  return u.v;
}

// q fragments (B operand): lane holds (q + bias)[query = lane&31][dk = kk*16 + (lane>>5)*8 + e]
template <int NKK>
__device__ __forceinline__ void load_q(const bf16_t* qrow, const float* bias, bf16x8 (&out)[NKK], bool valid, int lh) {
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk) {
    float v[8];
    const int k0 = kk * 16 + lh * 8;
    if (valid) {
      const u32x4 t = *reinterpret_cast<const u32x4*>(qrow + k0);
#pragma unroll
      for (int j = 0; j < 4; ++j) { v[2 * j] = __uint_as_float(t[j] << 16); v[2 * j + 1] = __uint_as_float(t[j] & 0xffff0000u); }
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] += bias[k0 + j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = 0.f;
    }
    out[kk] = pack8(v);
  }
}

// fragment (8 k-slots) for an MFMA A operand taken TRANSPOSED out of a row-major [row][64] image with the (row>>1)&7
// chunk swizzle: slots 0-3 <- rows ra..ra+3, slots 4-7 <- rows rb..rb+3, all at column col0 + (lane&31)
template <int ADK>
__device__ __forceinline__ bf16x8 tr_frag(const bf16_t* img, int ra, int rb, int col0, int lane) {
  const int t = lane & 15, g4 = (lane >> 4) & 1;
  const int col = col0 + g4 * 16 + (t & 3) * 4;
  union { bf16x8 v; s16x4 h[2]; } u;
  const int r0 = ra + (t >> 2), r1 = rb + (t >> 2);
  u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(img + r0 * ADK + ((((col >> 3) ^ ((r0 >> 1) & 7))) << 3) + (col & 7)));
  u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(img + r1 * ADK + ((((col >> 3) ^ ((r1 >> 1) & 7))) << 3) + (col & 7)));
  return u.v;
}
// plain row fragments of a [M, d] bf16 matrix as MFMA B operand: lane holds x[row][col0 + kk*16 + (lane>>5)*8 + e]
template <int NKK>
__device__ __forceinline__ void load_rows(const bf16_t* rowp, bf16x8 (&out)[NKK], bool valid, int lh) {
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk) {
    union { bf16x8 v; u32x4 w; } u;
    u.w = (u32x4){0u, 0u, 0u, 0u};
    if (valid) u.w = *reinterpret_cast<const u32x4*>(rowp + kk * 16 + lh * 8);
    out[kk] = u.v;
  }
}

// stage 2: the 64 positions of block pair x (disjoint between pairs), summed over the utterance chunks z
template <int ADK>
__global__ __launch_bounds__(256) void dpos_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dpos, long long ldd,
                                                          bf16_t* __restrict__ dpos_cast, int H, int T, int nz) {
  const int nT = (T + 31) / 32;
  const int x = blockIdx.x, h = blockIdx.y;
  const int P = 2 * T - 1;
  const int e = blockIdx.z * 256 + threadIdx.x;  // ADK / 4 blocks of 256 threads cover the 64 x ADK pair
  const int cl = e / ADK, dk = e % ADK;
  const int c = T - 32 + 32 * (2 * x - (nT - 1)) + cl;
  if (c < 0 || c >= P) return;
  float acc = 0.f;
  for (int z = 0; z < nz; ++z) acc += partial[(((long long)z * nT + x) * H + h) * (64 * ADK) + e];
  const float v = dpos[(long long)c * ldd + h * ADK + dk] + acc;
  dpos[(long long)c * ldd + h * ADK + dk] = v;
  // every (c, h, dk) of [0, 2T-1) x H x 64 is owned by exactly one thread of this launch, so the GEMM-operand copy of the
  // gradient (the linear_pos weight gradient's input) can be written here instead of by a cast pass of its own
  if (dpos_cast) dpos_cast[(long long)c * ldd + h * ADK + dk] = f2bf(v);
}
