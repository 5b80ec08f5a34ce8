// Cache-aware streaming inference (ConformerEncoder.cache_aware_stream_step, conformer_encoder.py's `update_cache` paths of
// RelPositionMultiHeadAttention and CausalConv1D): the three kernels the streaming sequencer (modules/conformer_streaming.py)
// adds to the offline ones.
//
//   mi355x_stream_cache_assemble  the K/V projection's operand [B*Tk, d] = cat(cache_last_channel[l], LN(chunk)) along time, and
//                                 the next channel cache = its last C rows, in one pass
//   mi355x_stream_attn            chunk attention: Tq queries against Tk = C + Tq keys (cached frames + the chunk), the rel-pos
//                                 term from a [2Tk-1] positional band, masks for unfilled cache slots / ragged chunks /
//                                 chunked_limited; scores stay on chip (online softmax, f32)
//   mi355x_stream_dwconv          causal depthwise conv whose K-1 left taps come from cache_last_time[l]; writes the next cache
//
// Caches are f32 in the reference's layouts.  In bf16 compute they hold the bf16-ROUNDED operands (the LayerNorm output the K/V
// projection reads, the GLU output the depthwise conv reads) widened to f32: a streamed chunk sees exactly the operand values the
// offline forward sees for the same frames.
#include "common.h"

// ------------------------------------------------------------------------------------------------ cache assembly
// cache [B, C, d] f32, y [B*Tq, d] (dt) -> kv_in [B*Tk, d] (dt), cache_next [B, C, d] f32 (last C rows of cat(cache, y))
template <typename T>
__global__ __launch_bounds__(256) void stream_cache_assemble_kernel(const float* __restrict__ cache, const T* __restrict__ y,
                                                                    T* __restrict__ kv_in, float* __restrict__ cache_next, int B,
                                                                    int C, int Tq, int d) {
  const int Tk = C + Tq;
  const int d4 = d >> 2;
  const long long n_kv = (long long)B * Tk * d4, n_all = n_kv + (long long)B * C * d4;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_all; e += (long long)gridDim.x * blockDim.x) {
    const bool to_kv = e < n_kv;
    const long long f = to_kv ? e : e - n_kv;
    const int c4 = (int)(f % d4);
    const long long row = f / d4;
    const int rows_b = to_kv ? Tk : C;
    const int b = (int)(row / rows_b), r = (int)(row % rows_b);
    const int j = to_kv ? r : r + Tq;  // position on the concatenated [cache | chunk] axis
    float v[4];
    if (j < C) ld4<float>(cache + ((long long)b * C + j) * d + 4 * c4, v);
    else ld4<T>(y + ((long long)b * Tq + (j - C)) * d + 4 * c4, v);
    if (to_kv) st4<T>(kv_in + ((long long)b * Tk + j) * d + 4 * c4, v);
    else st4<float>(cache_next + ((long long)b * C + r) * d + 4 * c4, v);
  }
}

extern "C" int mi355x_stream_cache_assemble(const void* cache, const void* y, void* kv_in, void* cache_next, int dt, int B, int C,
                                            int Tq, int d, void* stream) {
  mi_clear_errors();
  if (!y || !kv_in || B <= 0 || C < 0 || Tq <= 0 || d <= 0 || (d & 3) || (C > 0 && (!cache || !cache_next)) ||
      (dt != MI_DT_F32 && dt != MI_DT_BF16))
    return MI_ERR_ARG;
  const long long n = (long long)B * (2 * C + Tq) * (d >> 2);
  const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipStream_t s = (hipStream_t)stream;
  if (dt == MI_DT_BF16)
    MI_LAUNCH((stream_cache_assemble_kernel<bf16_t>), dim3(blocks), dim3(256), 0, s, (const float*)cache, (const bf16_t*)y,
              (bf16_t*)kv_in, (float*)cache_next, B, C, Tq, d);
  else
    MI_LAUNCH((stream_cache_assemble_kernel<float>), dim3(blocks), dim3(256), 0, s, (const float*)cache, (const float*)y,
              (float*)kv_in, (float*)cache_next, B, C, Tq, d);
  return mi_check_launch();
}

// ------------------------------------------------------------------------------------------------ chunk attention
// One workgroup = (query tile of SA_QT rows, head h, utterance b); 4 waves, each wave two queries (one per 32-lane half).
// Keys go by blocks of SA_KB = 32: the block's K and V rows of head h and the positional rows the tile's (i, j) pairs touch are
// staged in LDS as f32, a lane of a half-wave owns one key (its score is a full dot product over d_k read from LDS, rows padded
// by one word so the 32 lanes hit 32 banks), the half-wave keeps the online-softmax state of its query, and the context is
// accumulated with a lane per output element (d_k <= 128 -> up to 4 per lane).
#define SA_KB 32
#define SA_QT 8
#define SA_MAX_DK 128

__device__ __forceinline__ float half_max(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <typename T>
__global__ __launch_bounds__(256) void stream_attn_kernel(const T* __restrict__ q, long long ldq, const T* __restrict__ kv,
                                                          long long ldkv, long long v_off, const T* __restrict__ pos, long long ldp,
                                                          const float* __restrict__ bias_u, const float* __restrict__ bias_v,
                                                          const long long* __restrict__ cache_len,
                                                          const long long* __restrict__ chunk_len, T* __restrict__ ctx,
                                                          long long ldo, int H, int Tq, int Tk, int dk, int chunk, int left_chunks,
                                                          float scale) {
  extern __shared__ __attribute__((aligned(16))) float sa_smem[];
  const int dkp1 = dk + 1;
  float* Ks = sa_smem;                              // [SA_KB][dk + 1]
  float* Vs = Ks + SA_KB * dkp1;                    // [SA_KB][dk]
  float* Ps = Vs + SA_KB * dk;                      // [SA_KB + SA_QT - 1][dk + 1]
  float* Qu = Ps + (SA_KB + SA_QT - 1) * dkp1;      // [SA_QT][dk]
  float* Qv = Qu + SA_QT * dk;                      // [SA_QT][dk]
  float* Pr = Qv + SA_QT * dk;                      // [SA_QT][SA_KB] probabilities of the current key block
  const int i0 = blockIdx.x * SA_QT, h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, l32 = lane & 31;
  const int qi = 2 * wave + half;                   // query of this half-wave inside the tile
  const int i = i0 + qi;
  const int C = Tk - Tq;
  const int P = 2 * Tk - 1;
  const int clen = (int)min(max(cache_len[b], 0LL), (long long)C);
  const int klen = (int)min(max(chunk_len[b], 0LL), (long long)Tq);
  const int j_lo = C - clen, j_hi = C + klen;       // visible keys: j_lo <= j < j_hi (and the chunked_limited rule)
  const long long hq = (long long)h * dk;
  // q + u, q + v of the tile (rounded to the operand dtype, as the offline path's stored q+u / q+v operands)
  for (int e = tid; e < SA_QT * dk; e += 256) {
    const int r = e / dk, c = e - r * dk;
    float qa = 0.f, qb = 0.f;
    if (i0 + r < Tq) {
      const float qq = ld<T>(q + ((long long)b * Tq + i0 + r) * ldq + hq + c);
      T ta, tb;
      st<T>(&ta, qq + bias_u[hq + c]);
      st<T>(&tb, qq + bias_v[hq + c]);
      qa = ld<T>(&ta);
      qb = ld<T>(&tb);
    }
    Qu[e] = qa;
    Qv[e] = qb;
  }
  float m = -INFINITY, l = 0.f;
  float acc[SA_MAX_DK / 32];
#pragma unroll
  for (int u = 0; u < SA_MAX_DK / 32; ++u) acc[u] = 0.f;
  const int q_chunk = chunk > 0 ? (C + i) / chunk : 0;
  for (int j0 = 0; j0 < Tk; j0 += SA_KB) {
    __syncthreads();  // (previous block's readers are done)
    for (int e = tid; e < SA_KB * dk; e += 256) {
      const int r = e / dk, c = e - r * dk;
      const int j = j0 + r;
      float kk = 0.f, vv = 0.f;
      if (j < Tk) {
        const T* row = kv + ((long long)b * Tk + j) * ldkv + hq + c;
        kk = ld<T>(row);
        vv = ld<T>(row + v_off);
      }
      Ks[r * dkp1 + c] = kk;
      Vs[r * dk + c] = vv;
    }
    // positional rows: pair (i, j) reads row j + Tq - 1 - i; the tile's pairs of this block span rows rbase .. rbase + KB + QT - 2
    const int rbase = j0 + Tq - i0 - SA_QT;
    for (int e = tid; e < (SA_KB + SA_QT - 1) * dk; e += 256) {
      const int r = e / dk, c = e - r * dk;
      const int pr = rbase + r;
      Ps[r * dkp1 + c] = (pr >= 0 && pr < P) ? ld<T>(pos + (long long)pr * ldp + hq + c) : 0.f;
    }
    __syncthreads();
    const int j = j0 + l32;
    bool vis = i < Tq && j < Tk && j >= j_lo && j < j_hi;
    if (chunk > 0) {
      const int dc = q_chunk - j / chunk;
      vis = vis && dc >= 0 && (left_chunks < 0 || dc <= left_chunks);
    }
    float s = -INFINITY;
    if (vis) {
      const float* kr = Ks + l32 * dkp1;
      const float* pr = Ps + (l32 + SA_QT - 1 - qi) * dkp1;
      const float* qa = Qu + qi * dk;
      const float* qb = Qv + qi * dk;
      float ac = 0.f, bd = 0.f;
      for (int c = 0; c < dk; ++c) {
        ac = fmaf(qa[c], kr[c], ac);
        bd = fmaf(qb[c], pr[c], bd);
      }
      s = (ac + bd) * scale;
    }
    const float mb = half_max(s);
    const float m_new = fmaxf(m, mb);
    float p = 0.f, corr = 1.f;
    if (m_new != -INFINITY) {
      p = vis ? __expf(s - m_new) : 0.f;
      corr = (m == -INFINITY) ? 0.f : __expf(m - m_new);
      m = m_new;
    }
    l = l * corr + half_sum(p);
    Pr[qi * SA_KB + l32] = p;
#pragma unroll
    for (int u = 0; u < SA_MAX_DK / 32; ++u) acc[u] *= corr;
    __syncthreads();
    const int jn = min(SA_KB, Tk - j0);
    for (int jj = 0; jj < jn; ++jj) {
      const float pj = Pr[qi * SA_KB + jj];
      const float* vr = Vs + jj * dk;
#pragma unroll
      for (int u = 0; u < SA_MAX_DK / 32; ++u) {
        const int c = l32 + 32 * u;
        if (c < dk) acc[u] = fmaf(pj, vr[c], acc[u]);
      }
    }
  }
  if (i < Tq) {
    const float inv = l > 0.f ? 1.f / l : 0.f;  // a query with no visible key writes zeros
    T* orow = ctx + ((long long)b * Tq + i) * ldo + hq;
#pragma unroll
    for (int u = 0; u < SA_MAX_DK / 32; ++u) {
      const int c = l32 + 32 * u;
      if (c < dk) st<T>(orow + c, acc[u] * inv);
    }
  }
}

static size_t stream_attn_lds(int dk) {
  return sizeof(float) * ((size_t)SA_KB * (dk + 1) + (size_t)SA_KB * dk + (size_t)(SA_KB + SA_QT - 1) * (dk + 1) +
                          2 * (size_t)SA_QT * dk + (size_t)SA_QT * SA_KB);
}

extern "C" int mi355x_stream_attn(const void* q, long long ldq, const void* kv, long long ldkv, long long v_off, const void* pos,
                                  long long ldp, const void* bias_u, const void* bias_v, const void* cache_len,
                                  const void* chunk_len, void* ctx, long long ldo, int dt, int B, int H, int Tq, int Tk, int dk,
                                  int chunk, int left_chunks, float scale, void* stream) {
  mi_clear_errors();
  if (!q || !kv || !pos || !bias_u || !bias_v || !cache_len || !chunk_len || !ctx || B <= 0 || H <= 0 || Tq <= 0 || Tk < Tq ||
      dk <= 0 || dk > SA_MAX_DK || chunk < 0 || ldq < (long long)H * dk || ldo < (long long)H * dk || ldp < (long long)H * dk ||
      ldkv < v_off + (long long)H * dk || v_off < (long long)H * dk || (dt != MI_DT_F32 && dt != MI_DT_BF16))
    return MI_ERR_ARG;
  const size_t lds = stream_attn_lds(dk);  // <= 62 KiB at d_k 128: inside the default dynamic-LDS limit
  dim3 grid((Tq + SA_QT - 1) / SA_QT, H, B), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (dt == MI_DT_BF16)
    MI_LAUNCH((stream_attn_kernel<bf16_t>), grid, block, lds, s, (const bf16_t*)q, ldq, (const bf16_t*)kv, ldkv, v_off,
              (const bf16_t*)pos, ldp, (const float*)bias_u, (const float*)bias_v, (const long long*)cache_len,
              (const long long*)chunk_len, (bf16_t*)ctx, ldo, H, Tq, Tk, dk, chunk, left_chunks, scale);
  else
    MI_LAUNCH((stream_attn_kernel<float>), grid, block, lds, s, (const float*)q, ldq, (const float*)kv, ldkv, v_off,
              (const float*)pos, ldp, (const float*)bias_u, (const float*)bias_v, (const long long*)cache_len,
              (const long long*)chunk_len, (float*)ctx, ldo, H, Tq, Tk, dk, chunk, left_chunks, scale);
  return mi_check_launch();
}

// ------------------------------------------------------------------------------------------------ depthwise conv with a time cache
// x [B*Tq, d] (dt, the GLU output with padded frames zeroed), cache [B, d, K-1] f32 -> y [B*Tq, d] (dt),
// cache_next [B, d, K-1] f32 = the last K-1 frames of cat(cache, x) along time (K - 1 may exceed Tq).
// Workgroup = 64 channels x 4 time groups of one utterance; taps read straight from global memory (each frame is read K times
// from L1 by neighbouring time groups: the chunk is a few frames).
template <typename T, int KS>
__global__ __launch_bounds__(256) void stream_dwconv_kernel(const T* __restrict__ x, const float* __restrict__ cache,
                                                            const float* __restrict__ w, const float* __restrict__ bias,
                                                            T* __restrict__ y, float* __restrict__ cache_next, int Tq, int d) {
  constexpr int KC = KS - 1;
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), tg = threadIdx.x >> 6, b = blockIdx.y;
  if (c >= d) return;
  const T* xb = x + (long long)b * Tq * d + c;
  const float* cb = cache + ((long long)b * d + c) * KC;
  float wk[KS];
#pragma unroll
  for (int k = 0; k < KS; ++k) wk[k] = w[c * KS + k];
  const float bs = bias ? bias[c] : 0.f;
  for (int t = tg; t < Tq; t += 4) {
    float a = bs;
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      const int tau = t - KC + k;  // input frame; < 0: from the cache
      a = fmaf(wk[k], tau >= 0 ? ld<T>(xb + (long long)tau * d) : cb[tau + KC], a);
    }
    st<T>(y + ((long long)b * Tq + t) * d + c, a);
  }
  float* nb = cache_next + ((long long)b * d + c) * KC;
  for (int s = tg; s < KC; s += 4) {
    const int tau = Tq - KC + s;
    nb[s] = tau >= 0 ? ld<T>(xb + (long long)tau * d) : cb[tau + KC];
  }
}

extern "C" int mi355x_stream_dwconv(const void* x, const void* cache, const void* w, const void* bias, void* y, void* cache_next,
                                    int dt, int B, int Tq, int d, int ksize, void* stream) {
  mi_clear_errors();
  if (!x || !cache || !w || !y || !cache_next || B <= 0 || Tq <= 0 || d <= 0 || cache == cache_next ||
      (dt != MI_DT_F32 && dt != MI_DT_BF16))
    return MI_ERR_ARG;
  dim3 grid((d + 63) / 64, B), block(256);
  hipStream_t s = (hipStream_t)stream;
#define SD(KS) do { if (dt == MI_DT_BF16) MI_LAUNCH((stream_dwconv_kernel<bf16_t, KS>), grid, block, 0, s, (const bf16_t*)x, \
    (const float*)cache, (const float*)w, (const float*)bias, (bf16_t*)y, (float*)cache_next, Tq, d); \
    else MI_LAUNCH((stream_dwconv_kernel<float, KS>), grid, block, 0, s, (const float*)x, (const float*)cache, (const float*)w, \
    (const float*)bias, (float*)y, (float*)cache_next, Tq, d); } while (0)
  switch (ksize) {
    case 31: SD(31); break;
    case 9: SD(9); break;
    case 5: SD(5); break;
    case 3: SD(3); break;
    default: return MI_ERR_ARG;
  }
#undef SD
  return mi_check_launch();
}
