// Windowed rel-pos flash attention for MI355X: the fused kernels of attention.hip for a LIMITED attention context
// (att_context_size = [left, right], style 'regular' or 'chunked_limited'; local attention runs as the regular window [w, w]).
//
// Data movement is attention.hip's (lane = query in forward / dQ, lane = key in dK/dV, mfma_f32_32x32x16_bf16, K / V tiles
// double-buffered by LDS-DMA, the positional band as a ring of six 32-row blocks, rel_shift through the wave-private [32][66]
// tile, base-2 online softmax with lazy re-scale).  What differs:
//   * a workgroup derives the range of 32-wide tiles its 128 rows can reach from the window (ctx_tiles below) and walks only
//     those: T^2 work becomes T x window.  The band ring is started at the first visited tile; ring slots are counted from
//     that tile (kr = kt - kt_lo), so the prologue still stages five adjacent blocks and a step ONE new block;
//   * a tile wholly inside the window of every query of the wave (and below the length) takes the unmasked branch; edge tiles
//     test each key against the lane's own interval [jlo, jhi] -- ctx_allows() of elementwise.hip restated as an interval,
//     clipped to the length -- with -inf into the running maximum, exactly like a padded key.  A wave whose queries see
//     nothing in a tile of the workgroup's range passes through with m_run = -inf and l_run = 0 intact;
//   * the dQ kernel writes the transient dS blocks kt_lo .. kt_hi of each query tile only, and the linear_pos gradient kernel
//     derives the same range per (utterance, query tile) and masks every other block: positions outside every window get += 0.
// No saved-probabilities mode and no packed rows here: the encoder unpacks to the padded grid in front of these kernels.
#include <stdlib.h>
#include "common.h"
#include "mi355x_asr.h"
#include "attention_common.h"

// ---- the window: ONE statement of it for the four kernels and the entry points' argument checks --------------------------
// style 1 'regular': -left <= j - i <= right, each side only if >= 0.  style 2 'chunked_limited' with right >= 0: chunk =
// right + 1, 0 <= i / chunk - j / chunk <= left / chunk (left < 0: every chunk to the left); with right < 0 the left-limited
// regular mask.  Either way the keys of a query form an interval whose two ends do not decrease with the query, and so do the
// queries of a key: the rows that 32 (or 128) consecutive rows of the other side reach are [lo(first), hi(last)], the rows ALL
// of them reach are [lo(last), hi(first)].
struct CtxWin { int style, left, right; };
#define CTX_INF (1 << 30)

__host__ __device__ inline bool ctx_args_ok(int style, int left, int right) {
  return style >= 1 && style <= 2 && left >= -1 && right >= -1;
}
// sides wider than the sequence are unlimited in effect: clamped so that the interval ends stay far from INT_MAX
__host__ __device__ inline CtxWin ctx_make(int style, int left, int right, int T) {
  return CtxWin{style, left > T ? T : left, right > T ? T : right};
}
// KEYS: the keys [lo, hi] query r sees; !KEYS: the queries [lo, hi] that see key r
template <bool KEYS>
__host__ __device__ inline void ctx_interval(const CtxWin& w, int r, int& lo, int& hi) {
  const int before = KEYS ? w.left : w.right, after = KEYS ? w.right : w.left;   // reach towards lower / higher indices
  if (w.style == 2 && w.right >= 0) {
    const int chunk = w.right + 1, rc = r / chunk;
    if (KEYS) {
      lo = w.left < 0 ? 0 : (rc - w.left / chunk > 0 ? rc - w.left / chunk : 0) * chunk;
      hi = rc * chunk + chunk - 1;
    } else {
      lo = rc * chunk;
      hi = w.left < 0 ? CTX_INF : (rc + w.left / chunk) * chunk + chunk - 1;
    }
    return;
  }
  lo = before < 0 ? 0 : (r - before > 0 ? r - before : 0);
  hi = after < 0 ? CTX_INF : r + after;
}
// 32-wide tiles [t_lo, t_hi) of the other side that rows a .. b reach, clipped to the L valid frames (a > b: none)
template <bool KEYS>
__host__ __device__ inline void ctx_tiles(const CtxWin& w, int a, int b, int L, int& t_lo, int& t_hi) {
  t_lo = t_hi = 0;
  if (a > b) return;
  int lo, hi, x;
  ctx_interval<KEYS>(w, a, lo, x);
  ctx_interval<KEYS>(w, b, x, hi);
  hi = hi < L - 1 ? hi : L - 1;
  if (lo > hi) return;
  t_lo = lo / 32;
  t_hi = hi / 32 + 1;
}

// ---- forward: one 128-query tile (lane = query) ---------------------------------------------------------------------------
template <int ADK>
__global__ __launch_bounds__(256, ADK == 64 ? 2 : 1) void relpos_flash_fwd_ctx_kernel(
    const bf16_t* __restrict__ qkv, long long ldq, const bf16_t* __restrict__ pos, long long ldp, const float* __restrict__ bias_u,
    const float* __restrict__ bias_v, const long long* __restrict__ len, bf16_t* __restrict__ ctx, bf16_t* __restrict__ ctx_lo,
    long long ldo, float* __restrict__ lse, int B, int H, int T, float scale, DropCfg drop, CtxWin win) {
  drop_resolve(drop);
  constexpr int NKK = ADK / 16, NDT = ADK / 32, NCH = ADK / 8;
  __shared__ __attribute__((aligned(16))) bf16_t s_k2[2][ABK * ADK];
  __shared__ __attribute__((aligned(16))) bf16_t s_v2[2][ABK * ADK];
  __shared__ __attribute__((aligned(16))) bf16_t s_p[APRING * 32 * ADK];
  __shared__ __attribute__((aligned(16))) float s_g[4][32 * SG_LD];

  const int b = blockIdx.z, h = blockIdx.y;
  const int i0_blk = blockIdx.x * ABQ;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = lane & 31, lh = lane >> 5;
  const int i = i0_blk + wave * 32 + q;  // this lane's query
  const int L = (int)min((long long)T, len[b]);
  const bool qvalid = i < L;
  const int P = 2 * T - 1;
  const long long row0 = (long long)b * T;
  const int Trc = T - 1;

  const bf16_t* qbase = qkv + row0 * ldq + h * ADK;
  const bf16_t* kbase = qbase + (ldq / 3);
  const bf16_t* vbase = qbase + 2 * (ldq / 3);
  const bf16_t* pbase = pos + h * ADK;

  bf16x8 qu[NKK], qv[NKK];
  load_q<NKK>(qbase + (long long)(i < T ? i : Trc) * ldq, bias_u + h * ADK, qu, i < T, lh);
  load_q<NKK>(qbase + (long long)(i < T ? i : Trc) * ldq, bias_v + h * ADK, qv, i < T, lh);

  f32x16 o[NDT];
#pragma unroll
  for (int t = 0; t < NDT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  float* sg = s_g[wave];
  const uint32_t akey = attn_key(drop, b, h);
  const uint32_t arow = adrop_rcode(akey, (uint32_t)i >> 2), erow = (uint32_t)(i & 3) * (2u * ADROP_G);
  const float c2 = scale * 1.4426950408889634f, tau = 8.f / c2;

  // key tiles of the workgroup: the union over its valid queries.  A workgroup beyond the length walks nothing and writes zeros.
  int kt_lo, kt_hi;
  ctx_tiles<true>(win, i0_blk, min(i0_blk + ABQ - 1, L - 1), L, kt_lo, kt_hi);
  // this lane's keys [jlo, jhi] (none for a padded query) and the keys EVERY query of the wave sees [f_lo, f_hi] (wave-uniform)
  int jlo, jhi, f_lo, f_hi, x_;
  ctx_interval<true>(win, i, jlo, jhi);
  jhi = min(jhi, L - 1);
  if (!qvalid) { jlo = 1; jhi = 0; }
  ctx_interval<true>(win, i0_blk + wave * 32 + 31, f_lo, x_);
  ctx_interval<true>(win, i0_blk + wave * 32, x_, f_hi);
  f_hi = min(f_hi, L - 1);

  const int c0 = T - 1 - (i0_blk + ABQ - 1);
  if (kt_lo < kt_hi) {
    stage_rows<ADK>(kbase, ldq, kt_lo * ABK, Trc, s_k2[0], ABK * NCH);
    stage_v<ADK>(vbase, ldq, kt_lo * ABK, Trc, s_v2[0]);
    stage_rows<ADK>(pbase, ldp, c0 + 32 * kt_lo, P - 1, s_p, ABAND * NCH);
  }
  for (int kt = kt_lo; kt < kt_hi; ++kt) {
    const int j0 = kt * ABK, kr = kt - kt_lo;   // kr: the step, counted from the first visited tile (buffers and ring slots)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // tile kt has landed; every wave is done reading the tile before
    if (kt + 1 < kt_hi) {
      stage_rows<ADK>(kbase, ldq, j0 + ABK, Trc, s_k2[(kr + 1) & 1], ABK * NCH);
      stage_v<ADK>(vbase, ldq, j0 + ABK, Trc, s_v2[(kr + 1) & 1]);
      stage_rows<ADK>(pbase, ldp, c0 + 32 * (kt + 5), P - 1, s_p + ((kr + 5) % APRING) * (32 * ADK), 32 * NCH);
    }
    const bf16_t* s_k = s_k2[kr & 1];
    const bf16_t* s_v = s_v2[kr & 1];
    const int slot0 = (kr + 3 - wave) % APRING, slot1 = (kr + 4 - wave) % APRING;

    // ---- S^T = K . Qu^T  and  G^T = P_band . Qv^T
    f32x16 acc_s, acc_g[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc_s[r] = 0.f; acc_g[0][r] = 0.f; acc_g[1][r] = 0.f; }
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) {
      const bf16x8 kf = *reinterpret_cast<const bf16x8*>(s_k + a_off<ADK>(q, kk * 2 + lh));
      acc_s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qu[kk], acc_s, 0, 0, 0);
#pragma unroll
      for (int gt = 0; gt < 2; ++gt) {
        const bf16x8 pf = *reinterpret_cast<const bf16x8*>(s_p + a_off<ADK>((gt ? slot1 : slot0) * 32 + q, kk * 2 + lh));
        acc_g[gt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf, qv[kk], acc_g[gt], 0, 0, 0);
      }
    }
    // ---- rel_shift through the wave-private LDS tile
#pragma unroll
    for (int gt = 0; gt < 2; ++gt)
#pragma unroll
      for (int r = 0; r < 16; ++r) sg[q * SG_LD + 32 * gt + (r & 3) + 8 * (r >> 2) + 4 * lh] = acc_g[gt][r];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    float s[16];
    float mx = -INFINITY;
    if (j0 >= f_lo && j0 + ABK - 1 <= f_hi) {
      // interior tile: every key is valid and inside the window of all 32 queries of the wave -- no masks (lanes of padded
      // queries run on finite numbers and are discarded at the end)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rho = (r & 3) + 8 * (r >> 2) + 4 * lh;
        s[r] = acc_s[r] + sg[q * SG_LD + rho + 31 - q];
        mx = fmaxf(mx, s[r]);
      }
    } else {
      // edge tile: window and length in one interval test.  A lane that sees no key here keeps mx = -inf; with m_run = -inf
      // too (nothing seen so far) the step leaves m_run, l_run and the accumulators as they are (alpha = 1, p = exp2(-inf) = 0)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rho = (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float bd = sg[q * SG_LD + rho + 31 - q];
        const bool ok = (j0 + rho) >= jlo && (j0 + rho) <= jhi;
        s[r] = ok ? acc_s[r] + bd : -INFINITY;
        mx = fmaxf(mx, s[r]);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (__builtin_amdgcn_ballot_w64(mx > m_run + tau) != 0ull) {  // lazy re-scaling (wave-uniform), see attention.hip
      const float m_new = fmaxf(m_run, mx);
      const float alpha = (m_new == -INFINITY) ? 1.f : __builtin_amdgcn_exp2f((m_run - m_new) * c2);  // m_run = -inf -> 0
      l_run *= alpha;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int t = 0; t < NDT; ++t) o[t][r] *= alpha;
      }
      m_run = m_new;
    }
    const float mc = (m_run == -INFINITY) ? 0.f : m_run * c2;
    float rs = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s[r] = __builtin_amdgcn_exp2f(fmaf(s[r], c2, -mc)); rs += s[r]; }
    rs += __shfl_xor(rs, 32, 64);
    l_run += rs;
    // ---- dropout: attn_keep's (i, j) counter on absolute indices -- the mask of the full run restricted to the window
    if (drop.threshold != 0u) {
      const uint32_t bj0 = (uint32_t)(j0 >> 2);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const uint32_t cc0 = adrop_ccode(bj0 + 2 * g), cc1 = adrop_ccode(bj0 + 2 * g + 1);
        const uint32_t seed = adrop_seed(arow ^ (lh ? cc1 : cc0)) + erow;
#pragma unroll
        for (int cp = 0; cp < 2; ++cp) {
          const uint32_t y = adrop_y(seed + cp * ADROP_G);
          s[4 * g + 2 * cp] = __umul24(y, ADROP_KA) >= drop.threshold ? s[4 * g + 2 * cp] : 0.f;
          s[4 * g + 2 * cp + 1] = __umul24(y, ADROP_KB) >= drop.threshold ? s[4 * g + 2 * cp + 1] : 0.f;
        }
      }
    }
    // ---- O^T += V^T . P^T
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      const bf16x8 pb = pack8(&s[8 * st]);
#pragma unroll
      for (int dvt = 0; dvt < NDT; ++dvt) {
        const bf16x8 vf = vt_frag<ADK>(s_v, dvt * 32, st, lane);
        o[dvt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pb, o[dvt], 0, 0, 0);
      }
    }
  }

  // ---- normalise, transpose O^T -> O through LDS and store rows (padded rows: zeros, lse = 0)
  const float inv = (qvalid && l_run > 0.f) ? (drop.threshold != 0u ? drop.scale : 1.f) / l_run : 0.f;
  __syncthreads();
  if (lse && lh == 0 && i < T) lse[((long long)b * H + h) * T + i] = qvalid ? m_run * scale + __logf(l_run) : 0.f;
#pragma unroll
  for (int half = 0; half < NDT / 2; ++half) {
#pragma unroll
    for (int dvt = 0; dvt < 2; ++dvt)
#pragma unroll
      for (int r = 0; r < 16; ++r) sg[q * SG_LD + dvt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh] = o[2 * half + dvt][r] * inv;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = it * 8 + (lane >> 3), c8 = (lane & 7) * 8, co = half * 64 + c8;
      const int ii = i0_blk + wave * 32 + row;
      if (ii < T) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = sg[row * SG_LD + c8 + j];
        u32x4 t = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
        *reinterpret_cast<u32x4*>(ctx + (row0 + ii) * ldo + h * ADK + co) = t;
        if (ctx_lo) {  // the bf16 rounding residual of O for backward's delta (see attention.hip)
          float lo[8];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            lo[2 * j] = v[2 * j] - __uint_as_float(t[j] << 16);
            lo[2 * j + 1] = v[2 * j + 1] - __uint_as_float(t[j] & 0xffff0000u);
          }
          u32x4 tl = {pack_bf2(lo[0], lo[1]), pack_bf2(lo[2], lo[3]), pack_bf2(lo[4], lo[5]), pack_bf2(lo[6], lo[7])};
          *reinterpret_cast<u32x4*>(ctx_lo + (row0 + ii) * ldo + h * ADK + co) = tl;
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
}

// ---- dQu / dQv for one 128-query tile (lane = query), and the dS blocks of the visited tiles ---------------------------------
template <int ADK>
__global__ __launch_bounds__(256, ADK == 64 ? 2 : 1) void relpos_flash_bwd_dq_ctx_kernel(
    const bf16_t* __restrict__ qu_g, const bf16_t* __restrict__ qv_g, const bf16_t* __restrict__ qkv, long long ldq,
    const bf16_t* __restrict__ pos, long long ldp, const long long* __restrict__ len, const bf16_t* __restrict__ dO,
    const float* __restrict__ lse, const float* __restrict__ delta, bf16_t* __restrict__ dqu_out,
    bf16_t* __restrict__ dqv_out, bf16_t* __restrict__ ds_out, bf16_t* __restrict__ dq_out, long long ld_dq,
    float* __restrict__ cs_partial, int B, int H, int T, int d, float scale, DropCfg drop, CtxWin win) {
  drop_resolve(drop);
  constexpr int NKK = ADK / 16, NDT = ADK / 32, NCH = ADK / 8;
  __shared__ __attribute__((aligned(16))) bf16_t s_k2[2][ABK * ADK];
  __shared__ __attribute__((aligned(16))) bf16_t s_v[ABK * ADK];
  __shared__ __attribute__((aligned(16))) bf16_t s_p[APRING * 32 * ADK];
  __shared__ __attribute__((aligned(16))) float s_g[4][32 * SG_LD];
  __shared__ __attribute__((aligned(16))) bf16_t s_carry[4][32 * 32];  // upper half of the previous step's band, per wave

  const int b = blockIdx.z, h = blockIdx.y;
  const int i0_blk = blockIdx.x * ABQ;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = lane & 31, lh = lane >> 5;
  const int i = i0_blk + wave * 32 + q;
  const int L = (int)min((long long)T, len[b]);
  const bool qvalid = i < L;
  const int P = 2 * T - 1;
  const long long row0 = (long long)b * T;
  const int Trc = T - 1;
  const long long rowi = row0 + (i < T ? i : Trc);

  const bf16_t* kbase = qkv + row0 * ldq + h * ADK + (ldq / 3);
  const bf16_t* vbase = kbase + (ldq / 3);
  const bf16_t* pbase = pos + h * ADK;

  bf16x8 qu[NKK], qv[NKK], dof[NKK];
  load_rows<NKK>(qu_g + rowi * d + h * ADK, qu, i < T, lh);
  load_rows<NKK>(qv_g + rowi * d + h * ADK, qv, i < T, lh);
  load_rows<NKK>(dO + rowi * d + h * ADK, dof, i < T, lh);
  float lse_i = qvalid ? lse[((long long)b * H + h) * T + i] : 1e30f;  // padded query: exp(. - 1e30) = 0
  float dlt_i = qvalid ? delta[((long long)b * H + h) * T + i] : 0.f;
  // (the compiler must wait for these register loads HERE, not at their first use inside the loop)
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk) { asm volatile("" : "+v"(qu[kk])); asm volatile("" : "+v"(qv[kk])); asm volatile("" : "+v"(dof[kk])); }
  asm volatile("" : "+v"(lse_i), "+v"(dlt_i));

  f32x16 dqu[NDT], dqv[NDT];
#pragma unroll
  for (int t = 0; t < NDT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dqu[t][r] = 0.f; dqv[t][r] = 0.f; }
  float* sg = s_g[wave];
  const uint32_t akey = attn_key(drop, b, h);
  const uint32_t arow = adrop_rcode(akey, (uint32_t)i >> 2), erow = (uint32_t)(i & 3) * (2u * ADROP_G);
  // P = exp2(raw * c2 - lse * log2(e)); dS = P * (keep * dP * ks - delta * scale), ks = scale / (1 - p)
  const float c2 = scale * 1.4426950408889634f, lse2 = lse_i * 1.4426950408889634f;
  const float ks = drop.threshold != 0u ? drop.scale * scale : scale, dls = dlt_i * scale;

  int kt_lo, kt_hi;   // the forward's tile range and intervals
  ctx_tiles<true>(win, i0_blk, min(i0_blk + ABQ - 1, L - 1), L, kt_lo, kt_hi);
  int jlo, jhi, f_lo, f_hi, x_;
  ctx_interval<true>(win, i, jlo, jhi);
  jhi = min(jhi, L - 1);
  if (!qvalid) { jlo = 1; jhi = 0; }
  ctx_interval<true>(win, i0_blk + wave * 32 + 31, f_lo, x_);
  ctx_interval<true>(win, i0_blk + wave * 32, x_, f_hi);
  f_hi = min(f_hi, L - 1);

  // linear_pos gradient operand: tile `itile` of (h, b) owns nT+1 blocks of 32 x 32 bf16; this kernel writes blocks kt_lo .. kt_hi
  const int nT = (T + 31) / 32, itile = blockIdx.x * 4 + wave;
  const bool xw = ds_out != nullptr && itile < nT && kt_lo < kt_hi;  // wave-uniform
  bf16_t* xbase = ds_out + ((((long long)h * B + b) * nT + itile) * (nT + 1)) * 1024;
  u32x4* carry = reinterpret_cast<u32x4*>(s_carry[wave]);
  if (xw) { carry[lane] = (u32x4){0u, 0u, 0u, 0u}; carry[64 + lane] = (u32x4){0u, 0u, 0u, 0u}; }
  const int c0 = T - 1 - (i0_blk + ABQ - 1);
  if (kt_lo < kt_hi) {
    stage_rows<ADK>(kbase, ldq, kt_lo * ABK, Trc, s_k2[0], ABK * NCH);
    stage_rows<ADK>(vbase, ldq, kt_lo * ABK, Trc, s_v, ABK * NCH);
    stage_rows<ADK>(pbase, ldp, c0 + 32 * kt_lo, P - 1, s_p, ABAND * NCH);
  }
  for (int kt = kt_lo; kt < kt_hi; ++kt) {
    const int j0 = kt * ABK, kr = kt - kt_lo;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // tile kt has landed; every wave is done with the step before
    if (kt + 1 < kt_hi) {
      stage_rows<ADK>(kbase, ldq, j0 + ABK, Trc, s_k2[(kr + 1) & 1], ABK * NCH);
      stage_rows<ADK>(pbase, ldp, c0 + 32 * (kt + 5), P - 1, s_p + ((kr + 5) % APRING) * (32 * ADK), 32 * NCH);
    }
    const bf16_t* s_k = s_k2[kr & 1];
    const int slot0 = (kr + 3 - wave) % APRING, slot1 = (kr + 4 - wave) % APRING;

    f32x16 acc_s, acc_g[2], acc_dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc_s[r] = 0.f; acc_g[0][r] = 0.f; acc_g[1][r] = 0.f; acc_dp[r] = 0.f; }
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) {
      const bf16x8 kf = *reinterpret_cast<const bf16x8*>(s_k + a_off<ADK>(q, kk * 2 + lh));
      acc_s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qu[kk], acc_s, 0, 0, 0);
      const bf16x8 vf = *reinterpret_cast<const bf16x8*>(s_v + a_off<ADK>(q, kk * 2 + lh));
      acc_dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, dof[kk], acc_dp, 0, 0, 0);  // dP^T[key][query] = V . dO^T
#pragma unroll
      for (int gt = 0; gt < 2; ++gt) {
        const bf16x8 pf = *reinterpret_cast<const bf16x8*>(s_p + a_off<ADK>((gt ? slot1 : slot0) * 32 + q, kk * 2 + lh));
        acc_g[gt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf, qv[kk], acc_g[gt], 0, 0, 0);
      }
    }
    if (kt + 1 < kt_hi) {  // (block-uniform)
      __syncthreads();     // every wave has its V fragments
      stage_rows<ADK>(vbase, ldq, j0 + ABK, Trc, s_v, ABK * NCH);
    }
    float ds[16];
#pragma unroll
    for (int gt = 0; gt < 2; ++gt)
#pragma unroll
      for (int r = 0; r < 16; ++r) sg[q * SG_LD + 32 * gt + (r & 3) + 8 * (r >> 2) + 4 * lh] = acc_g[gt][r];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (j0 >= f_lo && j0 + ABK - 1 <= f_hi) {  // interior tile; padded queries carry lse_i = +1e30 -> P = 0 without a mask
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rho = (r & 3) + 8 * (r >> 2) + 4 * lh;
        ds[r] = __builtin_amdgcn_exp2f(fmaf(acc_s[r] + sg[q * SG_LD + rho + 31 - q], c2, -lse2));  // P[i, j]
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rho = (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float bd = sg[q * SG_LD + rho + 31 - q];
        const bool ok = (j0 + rho) >= jlo && (j0 + rho) <= jhi;
        ds[r] = ok ? __builtin_amdgcn_exp2f(fmaf(acc_s[r] + bd, c2, -lse2)) : 0.f;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // dS = P * (dropmask * dP - delta) * scale
    if (drop.threshold != 0u) {
      const uint32_t bj0 = (uint32_t)(j0 >> 2);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const uint32_t cc0 = adrop_ccode(bj0 + 2 * g), cc1 = adrop_ccode(bj0 + 2 * g + 1);
        const uint32_t seed = adrop_seed(arow ^ (lh ? cc1 : cc0)) + erow;
#pragma unroll
        for (int cp = 0; cp < 2; ++cp) {
          const uint32_t y = adrop_y(seed + cp * ADROP_G);
          const int r0 = 4 * g + 2 * cp;
          const float x0 = __umul24(y, ADROP_KA) >= drop.threshold ? acc_dp[r0] : 0.f;
          const float x1 = __umul24(y, ADROP_KB) >= drop.threshold ? acc_dp[r0 + 1] : 0.f;
          ds[r0] *= fmaf(x0, ks, -dls);
          ds[r0 + 1] *= fmaf(x1, ks, -dls);
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) ds[r] *= fmaf(acc_dp[r], ks, -dls);
    }
    // ---- dQu^T += K^T . dS^T
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      const bf16x8 db = pack8(&ds[8 * st]);
#pragma unroll
      for (int dkt = 0; dkt < NDT; ++dkt) {
        const bf16x8 kt_f = tr_frag<ADK>(s_k, 16 * st + 4 * lh, 16 * st + 8 + 4 * lh, dkt * 32, lane);
        dqu[dkt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kt_f, db, dqu[dkt], 0, 0, 0);
      }
    }
    // ---- un-skew dS into the band: sg[q][c_local] = dS[q][key = c_local - 31 + q]  (zero outside)
    {
      const float2 z = make_float2(0.f, 0.f);
#pragma unroll
      for (int w2 = 0; w2 < 16; ++w2) *reinterpret_cast<float2*>(sg + q * SG_LD + 32 * lh + 2 * w2) = z;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int r = 0; r < 16; ++r) sg[q * SG_LD + (r & 3) + 8 * (r >> 2) + 4 * lh + 31 - q] = ds[r];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // ---- dQv^T += P_band^T . dG^T
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      float gv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) gv[e] = sg[q * SG_LD + 16 * s4 + 8 * lh + e];
      const bf16x8 gb = pack8(gv);
#pragma unroll
      for (int dkt = 0; dkt < NDT; ++dkt) {
        const int ra = (s4 < 2 ? slot0 : slot1) * 32 + 16 * (s4 & 1) + 8 * lh;
        const bf16x8 pt_f = tr_frag<ADK>(s_p, ra, ra + 4, dkt * 32, lane);
        dqv[dkt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pt_f, gb, dqv[dkt], 0, 0, 0);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // ---- the band -> HBM in the un-shifted layout: block kt = this step's lower half | the carried upper half of step kt - 1
    // (zero at kt_lo: the tile before it lies outside every window of the wave)
    if (xw) {
#pragma unroll
      for (int it2 = 0; it2 < 2; ++it2) {
        const int row = it2 * 16 + (lane >> 2), c8 = (lane & 3) * 8;
        float lo[8], hi[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { lo[e] = sg[row * SG_LD + c8 + e]; hi[e] = sg[row * SG_LD + 32 + c8 + e]; }
        const u32x4 cw = carry[it2 * 64 + lane];
        u32x4 t = {pack_bf2(lo[0], lo[1]) | cw.x, pack_bf2(lo[2], lo[3]) | cw.y, pack_bf2(lo[4], lo[5]) | cw.z,
                   pack_bf2(lo[6], lo[7]) | cw.w};
        *reinterpret_cast<u32x4*>(xbase + (long long)kt * 1024 + it2 * 512 + lane * 8) = t;
        carry[it2 * 64 + lane] = (u32x4){pack_bf2(hi[0], hi[1]), pack_bf2(hi[2], hi[3]), pack_bf2(hi[4], hi[5]), pack_bf2(hi[6], hi[7])};
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
  }
  if (xw) {  // block kt_hi (<= nT): the upper half of the final step
#pragma unroll
    for (int it2 = 0; it2 < 2; ++it2)
      *reinterpret_cast<u32x4*>(xbase + (long long)kt_hi * 1024 + it2 * 512 + lane * 8) = carry[it2 * 64 + lane];
  }

  // ---- write dQu, dQv rows; with dq_out their sum and the per-workgroup column sums (see attention.hip)
  __syncthreads();
  constexpr int NH = NDT / 2;
  float keep[NH][4][8], cs[2][NH][8];
#pragma unroll
  for (int hf = 0; hf < NH; ++hf)
#pragma unroll
    for (int j = 0; j < 8; ++j) { cs[0][hf][j] = 0.f; cs[1][hf][j] = 0.f; }
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    bf16_t* outp = pass == 0 ? dqu_out : dqv_out;
#pragma unroll
    for (int hf = 0; hf < NH; ++hf) {
#pragma unroll
      for (int dkt = 0; dkt < 2; ++dkt)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          sg[q * SG_LD + dkt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh] = qvalid ? (pass == 0 ? dqu[2 * hf + dkt][r] : dqv[2 * hf + dkt][r]) : 0.f;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int row = it * 8 + (lane >> 3), c8 = (lane & 7) * 8, co = hf * 64 + c8;
        const int ii = i0_blk + wave * 32 + row;
        if (ii < T) {
          float v[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = sg[row * SG_LD + c8 + j];
          if (outp) {
            u32x4 t = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
            *reinterpret_cast<u32x4*>(outp + (row0 + ii) * d + h * ADK + co) = t;
          }
          if (dq_out) {
#pragma unroll
            for (int j = 0; j < 8; ++j) cs[pass][hf][j] += v[j];
            if (pass == 0) {
#pragma unroll
              for (int j = 0; j < 8; ++j) keep[hf][it][j] = v[j];
            } else {
#pragma unroll
              for (int j = 0; j < 8; ++j) v[j] += keep[hf][it][j];
              u32x4 t = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
              *reinterpret_cast<u32x4*>(dq_out + (row0 + ii) * ld_dq + h * ADK + co) = t;
            }
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
  }
  if (dq_out && cs_partial) {
#pragma unroll
    for (int pass = 0; pass < 2; ++pass)
#pragma unroll
      for (int hf = 0; hf < NH; ++hf)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float v = cs[pass][hf][j];
          v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
          cs[pass][hf][j] = v;
        }
    if (lane < 8) {
#pragma unroll
      for (int pass = 0; pass < 2; ++pass)
#pragma unroll
        for (int hf = 0; hf < NH; ++hf)
#pragma unroll
          for (int j = 0; j < 8; ++j) sg[pass * ADK + hf * 64 + lane * 8 + j] = cs[pass][hf][j];
    }
    __syncthreads();
    if (threadIdx.x < 2 * ADK) {
      const int uv = threadIdx.x / ADK, c = threadIdx.x % ADK;
      const float t = (s_g[0][threadIdx.x] + s_g[1][threadIdx.x]) + (s_g[2][threadIdx.x] + s_g[3][threadIdx.x]);
      cs_partial[((long long)b * gridDim.x + blockIdx.x) * (2 * d) + uv * d + h * ADK + c] = t;
    }
  }
}

// ---- dK / dV for one 128-key tile (lane = key): walks the query tiles that can see its keys -----------------------------------
template <int ADK>
__global__ __launch_bounds__(256, ADK == 64 ? 2 : 1) void relpos_flash_bwd_dkv_ctx_kernel(
    const bf16_t* __restrict__ qu_g, const bf16_t* __restrict__ qv_g, const bf16_t* __restrict__ qkv, long long ldq,
    const bf16_t* __restrict__ pos, long long ldp, const long long* __restrict__ len, const bf16_t* __restrict__ dO,
    const float* __restrict__ lse, const float* __restrict__ delta, bf16_t* __restrict__ dqkv, long long ldd, int B, int H,
    int T, int d, float scale, DropCfg drop, CtxWin win) {
  drop_resolve(drop);
  constexpr int NKK = ADK / 16, NDT = ADK / 32, NCH = ADK / 8;
  constexpr int Q_BYTES = 2 * 3 * 32 * ADK * 2;            // [2][qu | qv | dO][32 * ADK]
  constexpr int P_BYTES = APRING * 32 * ADK * 2;
  constexpr int STAGE_BYTES = Q_BYTES + P_BYTES + 2 * 2 * 32 * 4;
  constexpr int OUT_BYTES = 4 * 32 * SG_LD * 4;
  __shared__ __attribute__((aligned(16))) char s_raw[STAGE_BYTES > OUT_BYTES ? STAGE_BYTES : OUT_BYTES];
  bf16_t* const s_q3 = reinterpret_cast<bf16_t*>(s_raw);
  bf16_t* const s_p = reinterpret_cast<bf16_t*>(s_raw + Q_BYTES);
  float* const s_ld = reinterpret_cast<float*>(s_raw + Q_BYTES + P_BYTES);  // [2][lse | delta][32]

  const int b = blockIdx.z, h = blockIdx.y;
  const int j0_blk = blockIdx.x * ABQ;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = lane & 31, lh = lane >> 5;
  const int j = j0_blk + wave * 32 + q;  // this lane's key
  const int L = (int)min((long long)T, len[b]);
  const bool kvalid = j < L;
  const int P = 2 * T - 1;
  const long long row0 = (long long)b * T;
  const int Trc = T - 1;
  const long long rowj = row0 + (j < T ? j : Trc);
  const bf16_t* kbase = qkv + (ldq / 3) + h * ADK;
  const bf16_t* pbase = pos + h * ADK;
  const uint32_t akey = attn_key(drop, b, h);
  const uint32_t acol = adrop_ccode((uint32_t)j >> 2), ecol = (uint32_t)((j & 3) >> 1) * ADROP_G;
  const uint32_t klane = (j & 1) ? ADROP_KB : ADROP_KA;
  const float dscale = drop.threshold != 0u ? drop.scale : 1.f;

  bf16x8 kf[NKK], vf[NKK];
  load_rows<NKK>(kbase + rowj * ldq, kf, j < T, lh);
  load_rows<NKK>(kbase + (ldq / 3) + rowj * ldq, vf, j < T, lh);
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk) { asm volatile("" : "+v"(kf[kk])); asm volatile("" : "+v"(vf[kk])); }
  f32x16 dk_acc[NDT], dv_acc[NDT];
#pragma unroll
  for (int t = 0; t < NDT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk_acc[t][r] = 0.f; dv_acc[t][r] = 0.f; }

  // the mirrored range: query tiles holding a query that sees one of the workgroup's valid keys, and per lane the queries
  // [ilo, ihi] that see its own key (none for a padded key)
  int qt_lo, qt_hi, ilo, ihi;
  ctx_tiles<false>(win, j0_blk, min(j0_blk + ABQ - 1, L - 1), L, qt_lo, qt_hi);
  ctx_interval<false>(win, j, ilo, ihi);
  ihi = min(ihi, L - 1);
  if (!kvalid) { ilo = 1; ihi = 0; }

  const bf16_t* qub = qu_g + row0 * d + h * ADK;
  const bf16_t* qvb = qv_g + row0 * d + h * ADK;
  const bf16_t* dob = dO + row0 * d + h * ADK;
  // band rows of step qt: cb0 - 32*qt .. +159; the step after needs ONE new block at the low end.  Ring slots and buffers are
  // counted from the first visited tile (qr = qt - qt_lo)
  const int cb0 = T - 1 + j0_blk - 31;
  auto stage_q = [&](int i0, int buf) {
    bf16_t* dst = s_q3 + buf * (3 * 32 * ADK);
    stage_rows<ADK>(qub, d, i0, Trc, dst, 32 * NCH);
    stage_rows<ADK>(qvb, d, i0, Trc, dst + 32 * ADK, 32 * NCH);
    stage_rows<ADK>(dob, d, i0, Trc, dst + 2 * 32 * ADK, 32 * NCH);
    if (wave == 0) {
      int ii = i0 + (lane & 31);
      ii = ii < T ? ii : T - 1;  // (rows >= len are never used: p = 0 there)
      dma4((lane < 32 ? lse : delta) + ((long long)b * H + h) * T + ii, s_ld + buf * 64);
    }
  };
  if (qt_lo < qt_hi) {
    stage_q(qt_lo * 32, 0);
    stage_rows<ADK>(pbase, ldp, cb0 - 32 * qt_lo, P - 1, s_p, ABAND * NCH);
  }
  for (int qt = qt_lo; qt < qt_hi; ++qt) {
    const int i0 = qt * 32, qr = qt - qt_lo;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // tile qt has landed; every wave is done with the step before
    if (qt + 1 < qt_hi) {
      stage_q(i0 + 32, (qr + 1) & 1);
      stage_rows<ADK>(pbase, ldp, cb0 - 32 * (qt + 1), P - 1, s_p + ((6 * 1024 - (qr + 1)) % APRING) * (32 * ADK), 32 * NCH);
    }
    const bf16_t* s_qu = s_q3 + (qr & 1) * (3 * 32 * ADK);
    const bf16_t* s_qv = s_qu + 32 * ADK;
    const bf16_t* s_do = s_qu + 2 * 32 * ADK;
    const float* s_lse = s_ld + (qr & 1) * 64;
    const float* s_dlt = s_lse + 32;
    const int slot0 = (6 * 1024 - qr + wave) % APRING, slot1 = (6 * 1024 - qr + wave + 1) % APRING;  // band blocks wave, wave + 1

    f32x16 acc_s, acc_g[2], acc_dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc_s[r] = 0.f; acc_g[0][r] = 0.f; acc_g[1][r] = 0.f; acc_dp[r] = 0.f; }
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) {
      const bf16x8 quf = *reinterpret_cast<const bf16x8*>(s_qu + a_off<ADK>(q, kk * 2 + lh));
      acc_s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(quf, kf[kk], acc_s, 0, 0, 0);     // S[query][key]
      const bf16x8 dof = *reinterpret_cast<const bf16x8*>(s_do + a_off<ADK>(q, kk * 2 + lh));
      acc_dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dof, vf[kk], acc_dp, 0, 0, 0);   // dP[query][key]
      const bf16x8 qvf = *reinterpret_cast<const bf16x8*>(s_qv + a_off<ADK>(q, kk * 2 + lh));
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const bf16x8 pf = *reinterpret_cast<const bf16x8*>(s_p + a_off<ADK>((ct ? slot1 : slot0) * 32 + q, kk * 2 + lh));
        acc_g[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qvf, pf, acc_g[ct], 0, 0, 0);  // G[query][c_local]
      }
    }
    float pd[16], ds[16];
    uint32_t w4[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};  // keep iff w >= threshold (threshold 0: dropout off)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if ((r & 3) == 0 && drop.threshold != 0u) {
        const uint32_t rr0 = adrop_rcode(akey, (uint32_t)(i0 >> 2) + 2 * (r >> 2));
        const uint32_t rr1 = adrop_rcode(akey, (uint32_t)(i0 >> 2) + 2 * (r >> 2) + 1);
        const uint32_t seed = adrop_seed((lh ? rr1 : rr0) ^ acol) + ecol;
#pragma unroll
        for (int c = 0; c < 4; ++c) w4[c] = __umul24(adrop_y(seed + c * (2u * ADROP_G)), klane);
      }
      const int rho = (r & 3) + 8 * (r >> 2) + 4 * lh;  // query row of this register
      const int sl = 31 + q - rho;                      // column of G that holds c(i, j)
      const float g0 = __shfl(acc_g[0][r], lh * 32 + (sl & 31), 64);
      const float g1 = __shfl(acc_g[1][r], lh * 32 + (sl & 31), 64);
      const float bd = sl < 32 ? g0 : g1;
      const int ii = i0 + rho;
      const bool ok = ii >= ilo && ii <= ihi;           // key and query valid, and the query sees the key
      const float p = ok ? __expf((acc_s[r] + bd) * scale - s_lse[rho]) : 0.f;
      const bool keep = w4[r & 3] >= drop.threshold;
      pd[r] = keep ? p : 0.f;
      ds[r] = p * fmaf(keep ? acc_dp[r] : 0.f, dscale, -s_dlt[rho]);  // (x scale: applied to dK at the end)
    }
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      const bf16x8 pb = pack8(&pd[8 * st]);
      const bf16x8 db = pack8(&ds[8 * st]);
      const int ra = 16 * st + 4 * lh, rb = 16 * st + 8 + 4 * lh;
#pragma unroll
      for (int t2 = 0; t2 < NDT; ++t2) {
        const bf16x8 dot_f = tr_frag<ADK>(s_do, ra, rb, t2 * 32, lane);   // dO^T[dv][query slots]
        dv_acc[t2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dot_f, pb, dv_acc[t2], 0, 0, 0);
        const bf16x8 qut_f = tr_frag<ADK>(s_qu, ra, rb, t2 * 32, lane);   // Qu^T[dk][query slots]
        dk_acc[t2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qut_f, db, dk_acc[t2], 0, 0, 0);
      }
    }
  }
  __syncthreads();  // the transposition tile below overlays the staging buffers

  // ---- write dK, dV rows of this wave's 32 keys (zeros for keys no query sees, padded ones included)
  float* st_ = reinterpret_cast<float*>(s_raw) + wave * (32 * SG_LD);
#pragma unroll
  for (int pass = 0; pass < 2 * (NDT / 2); ++pass) {
    const int kind = pass / (NDT / 2), hf = pass % (NDT / 2);
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        st_[q * SG_LD + t2 * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh] =
            kind == 0 ? dk_acc[2 * hf + t2][r] * scale : dv_acc[2 * hf + t2][r] * dscale;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = it * 8 + (lane >> 3), c8 = (lane & 7) * 8;
      const int jj = j0_blk + wave * 32 + row;
      if (jj < T) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = st_[row * SG_LD + c8 + e];
        u32x4 t = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
        *reinterpret_cast<u32x4*>(dqkv + (row0 + jj) * ldd + (kind + 1) * (ldd / 3) + h * ADK + hf * 64 + c8) = t;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
}

// ---- d linear_pos output from the dS blocks (attention.hip's product; a block is read only if the dQ kernel wrote it) -------
template <int ADK>
__global__ __launch_bounds__(256, ADK == 64 ? 2 : 1) void relpos_flash_bwd_dpos_ctx_kernel(
    const bf16_t* __restrict__ qv_g, const bf16_t* __restrict__ x_g, const long long* __restrict__ len,
    float* __restrict__ dpos, long long ldd, float* __restrict__ partial, int B, int H, int T, int d, int bchunk, CtxWin win) {
  constexpr int NDT = ADK / 32, NCH = ADK / 8;
  __shared__ __attribute__((aligned(16))) bf16_t s_x[4][2][2 * 1024];   // per wave, double-buffered
  __shared__ __attribute__((aligned(16))) bf16_t s_qv[4][2][32 * ADK];

  const int nT = (T + 31) / 32;
  const int dg = 2 * (int)blockIdx.x - (nT - 1);  // s - it of the first block; the second is dg + 1
  const int h = blockIdx.y;
  const int b_begin = blockIdx.z * bchunk, b_end = min(B, b_begin + bchunk);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = lane & 31, lh = lane >> 5;
  const int P = 2 * T - 1;
  const int cmin = T - 32 + 32 * dg;
  const int it_lo = max(0, -dg - 1), it_hi = min(nT, nT - dg + 1);

  f32x16 dp_acc[2][NDT];
#pragma unroll
  for (int t = 0; t < NDT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dp_acc[0][t][r] = 0.f; dp_acc[1][t][r] = 0.f; }

  const int npairs = it_hi - it_lo;
  const int nitems = (b_end - b_begin) * npairs;
  // a slot outside [0, nT] is clamped for the load (always inside the tile's own blocks) and skipped in the product
  auto issue = [&](int b, int it, int buf) {
    const int s0 = it + dg;
    const int sl0 = min(max(s0, 0), nT), sl1 = min(max(s0 + 1, 0), nT);
    const bf16_t* base = x_g + ((((long long)h * B + b) * nT + it) * (nT + 1)) * 1024;
    bf16_t* sx = s_x[wave][buf];
    bf16_t* sqv = s_qv[wave][buf];
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
      dma16((base + sl0 * 1024 + k2 * 512 + lane * 8), (sx + k2 * 512));
      dma16((base + sl1 * 1024 + k2 * 512 + lane * 8), (sx + 1024 + k2 * 512));
    }
    const bf16_t* qb = qv_g + (long long)b * T * d + h * ADK;
#pragma unroll
    for (int k4 = 0; k4 < 32 * NCH / 64; ++k4) {
      const int cq = k4 * 64 + lane;
      const int r = cq / NCH, ck = cq % NCH;
      int gr = 32 * it + r;
      gr = gr > T - 1 ? T - 1 : gr;
      dma16((qb + __mul24(gr, d) + ((ck ^ ((r >> 1) & 7)) << 3)), (sqv + k4 * 512));
    }
  };
  auto advance = [&](int& b, int& it, int steps) {
    it += steps;
    while (it >= it_hi) { it -= npairs; ++b; }
  };
  uint32_t xaddr, qaddr[2][NDT][2];
  {
    const int t = lane & 15, g4 = (lane >> 4) & 1;
    xaddr = lds_addr(&s_x[wave][0][0]) + (uint32_t)(((8 * lh + (t >> 2)) * 32 + g4 * 16 + (t & 3) * 4) * 2);
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int dkt = 0; dkt < NDT; ++dkt)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const int r = 16 * st + 8 * lh + 4 * hf + (t >> 2), col = dkt * 32 + g4 * 16 + (t & 3) * 4;
          qaddr[st][dkt][hf] = lds_addr(&s_qv[wave][0][0]) + (uint32_t)((r * ADK + (((col >> 3) ^ ((r >> 1) & 7)) << 3) + (col & 7)) * 2);
        }
  }
  int cb = b_begin, cit = it_lo;      // item being computed by this wave
  advance(cb, cit, wave);
  int nb = cb, nit = cit;             // item being prefetched
  if (wave < nitems) issue(cb, cit, 0);
  int buf = 0;
  for (int item = wave; item < nitems; item += 4, buf ^= 1, advance(cb, cit, 4)) {
    if (item + 4 < nitems) {
      nb = cb; nit = cit; advance(nb, nit, 4);
      issue(nb, nit, buf ^ 1);
      if constexpr (ADK == 64) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");    // (the next item's 4 + 4 loads stay in flight)
      else asm volatile("s_waitcnt vmcnt(12)" ::: "memory");                       // (4 + 8)
    } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int b = cb;
    const int it = cit, s0 = it + dg;
    const int L = (int)min((long long)T, len[b]);
    // the dQ kernel wrote slots kt_lo .. kt_hi of this tile: the key-tile range of the tile's 128-query workgroup
    const int i0_blk = (it >> 2) * ABQ;
    int kt_lo, kt_hi;
    ctx_tiles<true>(win, i0_blk, min(i0_blk + ABQ - 1, L - 1), L, kt_lo, kt_hi);
    const bool any = kt_lo < kt_hi;
    const bool v0 = any && s0 >= kt_lo && s0 <= kt_hi, v1 = any && s0 + 1 >= kt_lo && s0 + 1 <= kt_hi;
    if (32 * it >= L || !(v0 || v1)) continue;  // wave-uniform: tiles without valid queries are all zero, other slots unwritten
    const uint32_t m0 = v0 ? 0xffffffffu : 0u, m1 = v1 ? 0xffffffffu : 0u;
    const uint32_t xa = xaddr + buf * 4096u, qoff = buf * (uint32_t)(32 * ADK * 2);
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      union { bf16x8 v; s16x4 h[2]; u32x4 w; } af[2], bq[NDT];
      asm volatile(
          "ds_read_b64_tr_b16 %0, %8\n\t"
          "ds_read_b64_tr_b16 %1, %8 offset:256\n\t"
          "ds_read_b64_tr_b16 %2, %8 offset:2048\n\t"
          "ds_read_b64_tr_b16 %3, %8 offset:2304\n\t"
          "ds_read_b64_tr_b16 %4, %9\n\t"
          "ds_read_b64_tr_b16 %5, %10\n\t"
          "ds_read_b64_tr_b16 %6, %11\n\t"
          "ds_read_b64_tr_b16 %7, %12\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(af[0].h[0]), "=&v"(af[0].h[1]), "=&v"(af[1].h[0]), "=&v"(af[1].h[1]), "=&v"(bq[0].h[0]), "=&v"(bq[0].h[1]),
            "=&v"(bq[1].h[0]), "=&v"(bq[1].h[1])
          : "v"(xa + st * 1024u), "v"(qaddr[st][0][0] + qoff), "v"(qaddr[st][0][1] + qoff), "v"(qaddr[st][1][0] + qoff),
            "v"(qaddr[st][1][1] + qoff)
          : "memory");
      if constexpr (NDT == 4) {
        asm volatile(
            "ds_read_b64_tr_b16 %0, %4\n\t"
            "ds_read_b64_tr_b16 %1, %5\n\t"
            "ds_read_b64_tr_b16 %2, %6\n\t"
            "ds_read_b64_tr_b16 %3, %7\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(bq[2].h[0]), "=&v"(bq[2].h[1]), "=&v"(bq[3].h[0]), "=&v"(bq[3].h[1])
            : "v"(qaddr[st][2][0] + qoff), "v"(qaddr[st][2][1] + qoff), "v"(qaddr[st][3][0] + qoff), "v"(qaddr[st][3][1] + qoff)
            : "memory");
      }
      af[0].w &= m0;
      af[1].w &= m1;
#pragma unroll
      for (int dkt = 0; dkt < NDT; ++dkt) {
        dp_acc[0][dkt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0].v, bq[dkt].v, dp_acc[0][dkt], 0, 0, 0);
        dp_acc[1][dkt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1].v, bq[dkt].v, dp_acc[1][dkt], 0, 0, 0);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }

  // ---- combine the 4 waves through LDS: waves 2,3 park, waves 0,1 add, wave 1 parks, wave 0 adds and owns the result
  __syncthreads();
  float* slab = reinterpret_cast<float*>(&s_qv[0][0][0]);  // 512 x ADK bytes = 2 slabs of 64 x ADK floats
  constexpr int SLAB = 64 * ADK;
  if (wave >= 2) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int dkt = 0; dkt < NDT; ++dkt)
#pragma unroll
        for (int r = 0; r < 16; ++r) slab[(wave - 2) * SLAB + ((ct * NDT + dkt) * 16 + r) * 64 + lane] = dp_acc[ct][dkt][r];
  }
  __syncthreads();
  if (wave < 2) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int dkt = 0; dkt < NDT; ++dkt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dp_acc[ct][dkt][r] += slab[wave * SLAB + ((ct * NDT + dkt) * 16 + r) * 64 + lane];
  }
  __syncthreads();
  if (wave == 1) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int dkt = 0; dkt < NDT; ++dkt)
#pragma unroll
        for (int r = 0; r < 16; ++r) slab[((ct * NDT + dkt) * 16 + r) * 64 + lane] = dp_acc[ct][dkt][r];
  }
  __syncthreads();
  if (wave != 0) return;
  float* out_slab = partial ? partial + (((long long)blockIdx.z * gridDim.x + blockIdx.x) * H + h) * SLAB : nullptr;
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int dkt = 0; dkt < NDT; ++dkt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = dp_acc[ct][dkt][r] + slab[((ct * NDT + dkt) * 16 + r) * 64 + lane];
        const int cl = ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh, dk = dkt * 32 + q;
        if (out_slab) out_slab[cl * ADK + dk] = v;  // deterministic two-stage reduction (dpos_reduce_kernel)
        else {
          const int c = cmin + cl;
          if (c >= 0 && c < P) atomicAdd(dpos + (long long)c * ldd + h * ADK + dk, v);
        }
      }
}

// ---- entry points: the argument rules of the unlimited siblings (no row offsets) + the window's ---------------------------
extern "C" int mi355x_relpos_flash_fwd_ctx(const void* qkv, long long ldq, const void* pos, long long ldp, const void* bias_u,
                                           const void* bias_v, const void* len, void* ctx, void* ctx_lo, long long ldo, void* lse,
                                           int B, int H, int T, int dk, int Tp, float scale, unsigned drop_key,
                                           unsigned drop_threshold, float drop_scale, int ctx_style, int ctx_left, int ctx_right,
                                           void* stream) {
  mi_clear_errors();
  (void)Tp;
  if (!qkv || !pos || !bias_u || !bias_v || !len || !ctx || B <= 0 || H <= 0 || T <= 0) return MI_ERR_ARG;
  if (!ctx_args_ok(ctx_style, ctx_left, ctx_right)) return MI_ERR_ARG;
  if ((dk != 64 && dk != 128) || (ldq % 24) || (ldp & 7) || (ldo & 7) || ((uintptr_t)qkv & 15) || ((uintptr_t)pos & 15) ||
      ((uintptr_t)ctx & 15) || ((uintptr_t)ctx_lo & 15))
    return MI_ERR_ARG;
  DropCfg dc = mi_drop(drop_key, drop_threshold, drop_scale);
  const CtxWin win = ctx_make(ctx_style, ctx_left, ctx_right, T);
  dim3 grid((T + ABQ - 1) / ABQ, H, B);
#define FWD_LAUNCH(DK)                                                                                                       \
  MI_LAUNCH(relpos_flash_fwd_ctx_kernel<DK>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, ldq,              \
            (const bf16_t*)pos, ldp, (const float*)bias_u, (const float*)bias_v, (const long long*)len, (bf16_t*)ctx,        \
            (bf16_t*)ctx_lo, ldo, (float*)lse, B, H, T, scale, dc, win)
  if (dk == 64) { FWD_LAUNCH(64); } else { FWD_LAUNCH(128); }
#undef FWD_LAUNCH
  return mi_check_launch();
}

extern "C" int mi355x_relpos_flash_bwd_dq_ctx(const void* qu, const void* qv, const void* qkv, long long ldq, const void* pos,
                                              long long ldp, const void* len, const void* dO, const void* lse, const void* delta,
                                              void* dqu, void* dqv, void* ds_out, void* dq_out, long long ld_dq, void* bias_grads,
                                              void* cs_scratch, long long cs_scratch_elems, int B, int H, int T, int dk,
                                              long long ds_elems, float scale, unsigned drop_key, unsigned drop_threshold,
                                              float drop_scale, int ctx_style, int ctx_left, int ctx_right, void* stream) {
  mi_clear_errors();
  if (!qu || !qv || !qkv || !pos || !len || !dO || !lse || !delta || B <= 0 || H <= 0 || T <= 0) return MI_ERR_ARG;
  if (!ctx_args_ok(ctx_style, ctx_left, ctx_right)) return MI_ERR_ARG;
  if ((dk != 64 && dk != 128) || (ldq % 24) || (ldp & 7)) return MI_ERR_ARG;
  if (!dq_out && (!dqu || !dqv)) return MI_ERR_ARG;
  const long long cs_need = (long long)B * ((T + ABQ - 1) / ABQ) * 2 * H * dk;
  if (dq_out && ((ld_dq & 7) || ((uintptr_t)dq_out & 15) || (bias_grads && (!cs_scratch || cs_scratch_elems < cs_need))))
    return MI_ERR_ARG;
  if (ds_out && (((uintptr_t)ds_out & 15) || ds_elems < mi355x_relpos_ds_elems(B, H, T))) return MI_ERR_ARG;
  DropCfg dc = mi_drop(drop_key, drop_threshold, drop_scale);
  const CtxWin win = ctx_make(ctx_style, ctx_left, ctx_right, T);
  dim3 grid((T + ABQ - 1) / ABQ, H, B);
#define DQ_LAUNCH(DK)                                                                                                        \
  MI_LAUNCH(relpos_flash_bwd_dq_ctx_kernel<DK>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qu, (const bf16_t*)qv, \
            (const bf16_t*)qkv, ldq, (const bf16_t*)pos, ldp, (const long long*)len, (const bf16_t*)dO, (const float*)lse,   \
            (const float*)delta, (bf16_t*)dqu, (bf16_t*)dqv, (bf16_t*)ds_out, (bf16_t*)dq_out, ld_dq,                       \
            bias_grads ? (float*)cs_scratch : nullptr, B, H, T, H * DK, scale, dc, win)
  if (dk == 64) { DQ_LAUNCH(64); } else { DQ_LAUNCH(128); }
#undef DQ_LAUNCH
  if (dq_out && bias_grads)
    MI_LAUNCH((partials_reduce_kernel<float>), dim3((2 * H * dk + 255) / 256, 8), dim3(256), 0, (hipStream_t)stream,
              (const float*)cs_scratch, (int)(B * ((T + ABQ - 1) / ABQ)), 2 * H * dk, (float*)bias_grads);
  return mi_check_launch();
}

extern "C" int mi355x_relpos_flash_bwd_dkv_ctx(const void* qu, const void* qv, const void* qkv, long long ldq, const void* pos,
                                               long long ldp, const void* len, const void* dO, const void* lse, const void* delta,
                                               void* dqkv, long long ldd, int B, int H, int T, int dk, int Tp, float scale,
                                               unsigned drop_key, unsigned drop_threshold, float drop_scale, int ctx_style,
                                               int ctx_left, int ctx_right, void* stream) {
  mi_clear_errors();
  (void)Tp;
  if (!qu || !qv || !qkv || !pos || !len || !dO || !lse || !delta || !dqkv || B <= 0 || H <= 0 || T <= 0) return MI_ERR_ARG;
  if (!ctx_args_ok(ctx_style, ctx_left, ctx_right)) return MI_ERR_ARG;
  if ((dk != 64 && dk != 128) || (ldq % 24) || (ldp & 7) || (ldd % 24)) return MI_ERR_ARG;
  DropCfg dc = mi_drop(drop_key, drop_threshold, drop_scale);
  const CtxWin win = ctx_make(ctx_style, ctx_left, ctx_right, T);
  dim3 grid((T + ABQ - 1) / ABQ, H, B);
#define DKV_LAUNCH(DK)                                                                                                       \
  MI_LAUNCH(relpos_flash_bwd_dkv_ctx_kernel<DK>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qu, (const bf16_t*)qv, \
            (const bf16_t*)qkv, ldq, (const bf16_t*)pos, ldp, (const long long*)len, (const bf16_t*)dO, (const float*)lse,   \
            (const float*)delta, (bf16_t*)dqkv, ldd, B, H, T, H * DK, scale, dc, win)
  if (dk == 64) { DKV_LAUNCH(64); } else { DKV_LAUNCH(128); }
#undef DKV_LAUNCH
  return mi_check_launch();
}

extern "C" int mi355x_relpos_flash_bwd_dpos_ctx(const void* qv, const void* ds, const void* len, void* dpos, long long ldd,
                                                void* dpos_cast, void* partial, long long partial_elems, int B, int H, int T,
                                                int dk, long long ds_elems, int ctx_style, int ctx_left, int ctx_right,
                                                void* stream) {
  mi_clear_errors();
  if (!qv || !ds || !len || !dpos || B <= 0 || H <= 0 || T <= 0 || (dpos_cast && !partial)) return MI_ERR_ARG;
  if (!ctx_args_ok(ctx_style, ctx_left, ctx_right)) return MI_ERR_ARG;
  if ((dk != 64 && dk != 128) || ((uintptr_t)ds & 15) || ds_elems < mi355x_relpos_ds_elems(B, H, T)) return MI_ERR_ARG;
  const int nT = (T + 31) / 32;
  const int bchunk = B >= 8 ? 4 : 1;
  const int nz = (B + bchunk - 1) / bchunk;
  if (partial && partial_elems < mi355x_relpos_dpos_partial_elems(B, H, T)) return MI_ERR_ARG;
  const CtxWin win = ctx_make(ctx_style, ctx_left, ctx_right, T);
  dim3 grid(nT, H, nz);
#define DPOS_LAUNCH(DK)                                                                                                      \
  MI_LAUNCH(relpos_flash_bwd_dpos_ctx_kernel<DK>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qv,               \
            (const bf16_t*)ds, (const long long*)len, (float*)dpos, ldd, (float*)partial, B, H, T, H * DK, bchunk, win);     \
  if (partial)                                                                                                               \
    MI_LAUNCH(dpos_reduce_kernel<DK>, dim3(nT, H, DK / 4), dim3(256), 0, (hipStream_t)stream, (const float*)partial,         \
              (float*)dpos, ldd, (bf16_t*)dpos_cast, H, T, nz)
  if (dk == 64) { DPOS_LAUNCH(64); } else { DPOS_LAUNCH(128); }
#undef DPOS_LAUNCH
  return mi_check_launch();
}
