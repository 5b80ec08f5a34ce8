// The stateless prediction network (`StatelessTransducerDecoder` / `StatelessNet`): training forward and backward, the prediction
// tables of the search, and the greedy search itself.  include/mi355x_asr.h states THE RULE (mi355x_stateless_*); these are its
// kernels.
//
// The network embeds the last C labels, one table per position (emb_i [V1, e_i], i = 0 the most recent label, row `blank` zero), and
// concatenates the results: there is no recurrence.  Two things follow for the search, neither of which the LSTM searches can have:
//   * the prediction projection of a label depends on the label alone, so W_pred . emb_i[v] is a TABLE P_i [V1, J], built once per
//     weight version (stateless_tables_kernel, MFMA tiles with M = vocabulary rows), and a step's gp is C row look-ups and adds;
//   * streams do not depend on a hidden state, so 16 of them are the 16 rows of ONE MFMA tile: a workgroup (8 waves) owns 16 streams,
//     every step builds A = relu(enc_proj[t_row] + gp_row) [16, J + pad] in LDS, the waves split the V1 (+ D) output rows, and W_out
//     goes from L2 straight into the B operand (rb_mma, rnnt_mma.h: one 16-byte load per lane, 8 in flight) -- W_out is read once
//     per step for 16 streams.  Logits go to LDS [16, (V1 + D) | 1]; a wave per two rows takes the first arg-max, the log-sum-exp
//     and the TDT duration arg-max, and its lane 0 moves the row's (t, context, sym, n, score) on and stores the token and frame.
//     Rows whose stream is finished (or beyond B) are zero rows.  A row of an MFMA result depends on its own A row only and the
//     reductions are per row, so a stream's bits do not depend on which streams share its workgroup, nor on how it is cut into
//     chunks (the resumable form).
// Training: the forward is a gather-concat-shift with the start-of-sequence blank (16-byte stores); the embedding gradient uses no
// atomics -- a workgroup per (table, 16 vocabulary rows) stages the table's context labels in LDS, each wave walks the list for its
// rows with a ballot per 64 labels and adds the matching dg rows in (b, u) order in registers, and writes each row once.
// Ordinary vector stores only, no scratch.  The device code of this translation unit is compiled to the scalar fp32 instructions
// only (the attribute below turns the packed v_pk_*_f32 forms off); they round as the packed forms do.
#include <hip/hip_runtime.h>
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "common.h"
#include "mi355x_asr.h"
#include "rnnt_mma.h"
#include "tdt.h"

#define SL_MAXC 4

// the slices of the concatenation: e_i = E / 2 / C for i > 0, e_0 = the rest; off_i = running sum
struct SlTabs {
  const float* emb[SL_MAXC];
  float* demb[SL_MAXC];
  int e[SL_MAXC], off[SL_MAXC];
  int C;
};
static inline int sl_slices(int E, int C, SlTabs* t) {
  if (C < 1 || C > SL_MAXC || E < 1) return MI_ERR_ARG;
  const int w = E / 2 / C;
  if (C > 1 && w < 1) return MI_ERR_ARG;
  for (int i = 0; i < SL_MAXC; ++i) { t->emb[i] = nullptr; t->demb[i] = nullptr; t->e[i] = 0; t->off[i] = 0; }
  t->C = C;
  t->e[0] = E - (C - 1) * w;
  for (int i = 1; i < C; ++i) { t->e[i] = w; t->off[i] = t->off[i - 1] + t->e[i - 1]; }
  return MI_OK;
}

// the label that table i sees at position u of utterance b: s[u - i] of s = [blank, y_0, ..., y_{U-1}]; -1: nothing (u - i < 0, a
// blank, or an id outside the table, which is treated as padding)
__device__ __forceinline__ int sl_label(const long long* __restrict__ targets, int b, int u, int i, int U, int V1, int blank) {
  const int q = u - i;
  if (q <= 0) return -1;
  const long long v = targets[(long long)b * U + q - 1];
  return (v < 0 || v >= V1 || v == blank) ? -1 : (int)v;
}

// ================================================================================================ training forward
// out [B, U1, E] (T): thread = V consecutive columns of one row, one 16-byte store when E % V == 0 (scalar stores otherwise)
template <typename T>
__global__ __launch_bounds__(256) void stateless_fwd_kernel(const long long* __restrict__ targets, SlTabs tb, T* __restrict__ out,
                                                            int B, int U, int E, int V1, int blank, DropCfg drop) {
  constexpr int V = VecIO<T>::V;
  drop_resolve(drop);
  const int U1 = U + 1, G = (E + V - 1) / V;
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long long)B * U1 * G) return;
  const long long row = id / G;
  const int c0 = (int)(id - row * G) * V, b = (int)(row / U1), u = (int)(row - (long long)b * U1);
  int lab[SL_MAXC];
#pragma unroll
  for (int i = 0; i < SL_MAXC; ++i) lab[i] = i < tb.C ? sl_label(targets, b, u, i, U, V1, blank) : -1;
  float v[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const int col = c0 + j;
    float x = 0.f;
#pragma unroll
    for (int i = 0; i < SL_MAXC; ++i)
      if (i < tb.C && lab[i] >= 0 && col >= tb.off[i] && col < tb.off[i] + tb.e[i]) x = tb.emb[i][(long long)lab[i] * tb.e[i] + col - tb.off[i]];
    v[j] = x;
  }
  const long long o = row * E + c0;
  if (E % V == 0) {
    if (drop.threshold) {
      float m[V];
      if constexpr (V == 8) drop_mask8u(drop, (uint32_t)o, m); else drop_mask4u(drop, (uint32_t)o, m);
#pragma unroll
      for (int j = 0; j < V; ++j) v[j] *= m[j];
    }
    VecIO<T>::store(out + o, v);
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (c0 + j < E) st<T>(out + o + j, v[j] * drop_mask(drop, (uint32_t)(o + j)));
  }
}

// ================================================================================================ embedding gradient
#define SL_BWD_THREADS 256
#define SL_BWD_ROWS 16      // vocabulary rows of a workgroup: 4 per wave
#define SL_BWD_CHUNK 4096   // labels staged at a time
#define SL_BWD_Q 4          // columns per lane and pass (64 lanes: 256 columns a pass)

template <typename T>
__global__ __launch_bounds__(SL_BWD_THREADS) void stateless_embed_bwd_kernel(const long long* __restrict__ targets,
                                                                              const T* __restrict__ dg, SlTabs tb, int accumulate,
                                                                              int B, int U, int E, int V1, int blank, DropCfg drop) {
  __shared__ int s_lab[SL_BWD_CHUNK];
  drop_resolve(drop);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, U1 = U + 1;
  const int i = blockIdx.y;
  float* dst = nullptr; int ei = 0, offi = 0;
#pragma unroll
  for (int k = 0; k < SL_MAXC; ++k) if (k == i) { dst = tb.demb[k]; ei = tb.e[k]; offi = tb.off[k]; }
  const long long n = (long long)B * U1;
  const int v0 = blockIdx.x * SL_BWD_ROWS + wave * (SL_BWD_ROWS / 4);
  for (int pass = 0; pass * 64 * SL_BWD_Q < ei; ++pass) {
    float acc[SL_BWD_ROWS / 4][SL_BWD_Q];
#pragma unroll
    for (int k = 0; k < SL_BWD_ROWS / 4; ++k)
#pragma unroll
      for (int q = 0; q < SL_BWD_Q; ++q) acc[k][q] = 0.f;
    for (long long p0 = 0; p0 < n; p0 += SL_BWD_CHUNK) {
      const int len = (int)min((long long)SL_BWD_CHUNK, n - p0);
      __syncthreads();
      for (int j = tid; j < len; j += SL_BWD_THREADS) {
        const long long p = p0 + j;
        const int b = (int)(p / U1);
        s_lab[j] = sl_label(targets, b, (int)(p - (long long)b * U1), i, U, V1, blank);
      }
      __syncthreads();
      for (int base = 0; base < len; base += 64) {
        const int lab = base + lane < len ? s_lab[base + lane] : -1;
#pragma unroll
        for (int k = 0; k < SL_BWD_ROWS / 4; ++k) {
          unsigned long long m = __ballot(lab == v0 + k);   // (a row beyond V1 matches nothing: labels are < V1)
          while (m) {   // ascending p: the (b, u) order of the rule
            const int j = __builtin_ctzll(m);
            m &= m - 1;
            const long long src = (p0 + base + j) * E + offi;
#pragma unroll
            for (int q = 0; q < SL_BWD_Q; ++q) {
              const int col = (pass * SL_BWD_Q + q) * 64 + lane;
              if (col < ei) acc[k][q] += ld<T>(dg + src + col) * drop_mask(drop, (uint32_t)(src + col));
            }
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < SL_BWD_ROWS / 4; ++k) {
      const int v = v0 + k;
      if (v >= V1) continue;
#pragma unroll
      for (int q = 0; q < SL_BWD_Q; ++q) {
        const int col = (pass * SL_BWD_Q + q) * 64 + lane;
        if (col >= ei) continue;
        float* d = dst + (long long)v * ei + col;
        if (accumulate) { if (v != blank) *d += acc[k][q]; }
        else *d = acc[k][q];   // (the blank row and rows nobody used: 0)
      }
    }
  }
}

// ================================================================================================ prediction tables
// P_i [V1, J] = emb_i . W_pred[:, off_i : off_i + e_i]^T: a wave per 16 x 16 tile, M = vocabulary rows, N = J, K = e_i.  The slices
// start at any column and have any width (28 / 6 / 6), so both operands are gathered element by element, zero beyond e_i.
#define SL_TAB_THREADS 256
template <typename WT>
__global__ __launch_bounds__(SL_TAB_THREADS) void stateless_tables_kernel(SlTabs tb, const WT* __restrict__ w_pred, long long ld_pred,
                                                                           float* __restrict__ tables, int V1, int J, int blank) {
  constexpr int V = RbT<WT>::V, KB = RbT<WT>::KB;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l16 = lane & 15, lg4 = lane >> 4;
  const int i = blockIdx.z;
  const float* emb = nullptr; int ei = 0, offi = 0;
#pragma unroll
  for (int k = 0; k < SL_MAXC; ++k) if (k == i) { emb = tb.emb[k]; ei = tb.e[k]; offi = tb.off[k]; }
  const int jt = blockIdx.y * (SL_TAB_THREADS / 64) + wave;
  if (jt * 16 >= J) return;   // (wave-uniform; no barrier follows)
  const int row = min(blockIdx.x * 16 + l16, V1 - 1), n = min(jt * 16 + l16, J - 1);
  const float* ar = emb + (long long)row * ei;
  const WT* br = w_pred + (long long)n * ld_pred + offi;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < ei; kb += KB) {
    const int k0 = kb + lg4 * V;
    u32x4 a, b;
    if constexpr (V == 8) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ka = k0 + 2 * j, kc = ka + 1;
        a[j] = pack_bf2(ka < ei ? ar[ka] : 0.f, kc < ei ? ar[kc] : 0.f);
        b[j] = (uint32_t)(ka < ei ? br[ka] : (bf16_t)0) | ((uint32_t)(kc < ei ? br[kc] : (bf16_t)0) << 16);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a[j] = __float_as_uint(k0 + j < ei ? ar[k0 + j] : 0.f);
        b[j] = __float_as_uint(k0 + j < ei ? br[k0 + j] : 0.f);
      }
    }
    acc = rb_mfma<WT>(a, b, acc);
  }
  const int col = jt * 16 + l16;
  if (col < J) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int v = blockIdx.x * 16 + lg4 * 4 + r;
      if (v < V1) tables[((long long)i * V1 + v) * J + col] = v == blank ? 0.f : acc[r];
    }
  }
}

// ================================================================================================ greedy search
#define SG_THREADS 512
#define SG_WAVES 8
#define SG_M 16   // streams of a workgroup = rows of the MFMA tile

struct SgState { int* ctx; float* score; int* frames_done; int* sym; int* skip; };
struct SgP {
  const void* f; int f_dt; long long ldf;   // encoder projection [B, T, J] (rows of pitch ldf)
  const long long* enc_len;
  const float* tab;                          // [C, V1, J]
  const float* b_pred; const void* w_out; long long ld_out; const float* b_out;
  int* tokens; int* times; int* out_len; float* score;
  SgState sin, sout;
  int B, T, J, V1, C, blank, max_symbols, max_out;
  TdtDur dur;
};

template <typename WT, bool TDT>
__global__ __launch_bounds__(SG_THREADS) void stateless_greedy_kernel(SgP p) {
  constexpr int V = RbT<WT>::V;
  extern __shared__ __attribute__((aligned(16))) unsigned char sg_smem[];
  const int J = p.J, V1 = p.V1, C = p.C, D = TDT ? p.dur.D : 0, N = V1 + D;
  const int ldj = J + V, ldl = N | 1, J4 = J >> 2;
  WT* aA = reinterpret_cast<WT*>(sg_smem);
  float* lgs = reinterpret_cast<float*>(sg_smem + (((size_t)SG_M * ldj * sizeof(WT) + 15) & ~(size_t)15));
  __shared__ int s_t[SG_M], s_len[SG_M], s_sym[SG_M], s_n[SG_M], s_live[SG_M], s_fd[SG_M], s_ctx[SG_M][SL_MAXC];
  __shared__ float s_score[SG_M];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, lg4 = lane >> 4;
  const int b0 = blockIdx.x * SG_M;

  if (tid < SG_M) {
    const int b = b0 + tid;
    int len = 0, t = 0, sym = 0, fd = 0;
    float score = 0.f;
    int ctx[SL_MAXC] = {p.blank, p.blank, p.blank, p.blank};
    if (b < p.B) {
      len = (int)min((long long)p.T, max(0LL, p.enc_len ? p.enc_len[b] : (long long)p.T));
      if (p.sin.ctx) {
#pragma unroll
        for (int c = 0; c < SL_MAXC; ++c)
          if (c < C) { const int v = p.sin.ctx[(long long)b * C + c]; ctx[c] = (v < 0 || v >= V1) ? p.blank : v; }
        score = p.sin.score[b]; fd = p.sin.frames_done[b];
        if (TDT) { sym = max(p.sin.sym[b], 0); t = max(p.sin.skip[b], 0); }   // frames an earlier duration already jumped over
      }
    }
    s_len[tid] = len; s_t[tid] = t; s_sym[tid] = sym; s_n[tid] = 0; s_fd[tid] = fd; s_score[tid] = score;
    s_live[tid] = t < len;
#pragma unroll
    for (int c = 0; c < SL_MAXC; ++c) s_ctx[tid][c] = ctx[c];
  }
  __syncthreads();
  int maxlen = 0;
#pragma unroll
  for (int k = 0; k < SG_M; ++k) maxlen = max(maxlen, s_len[k]);
  // every step moves a live row to its next frame or emits a label: RNN-T at most max_symbols joint steps per frame, the others
  // at most max_out labels
  const long long bound = (!TDT && p.max_symbols > 0) ? (long long)maxlen * p.max_symbols : (long long)maxlen + p.max_out;

  for (long long step = 0; step < bound; ++step) {
    bool any = false;   // (uniform: read behind a barrier)
#pragma unroll
    for (int k = 0; k < SG_M; ++k) any |= s_live[k] != 0;
    if (!any) break;
    // ---- A = relu(enc_proj[t] + gp), gp = ((P_0[c_0] + P_1[c_1]) + ...) + b_pred; finished rows are zero rows
    for (int i = tid; i < SG_M * J4; i += SG_THREADS) {
      const int k = i / J4, j = (i - k * J4) * 4;
      float av[4] = {0.f, 0.f, 0.f, 0.f};
      if (s_live[k]) {
        float g[4], x[4];
        ld4<float>(p.tab + (long long)s_ctx[k][0] * J + j, g);
#pragma unroll
        for (int c = 1; c < SL_MAXC; ++c)
          if (c < C) {
            ld4<float>(p.tab + ((long long)c * V1 + s_ctx[k][c]) * J + j, x);
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] += x[e];
          }
        ld4<float>(p.b_pred + j, x);
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] += x[e];
        const long long row = ((long long)(b0 + k) * p.T + s_t[k]) * p.ldf + j;
        if (p.f_dt == MI_DT_F32) ld4<float>((const float*)p.f + row, x); else ld4<bf16_t>((const bf16_t*)p.f + row, x);
#pragma unroll
        for (int e = 0; e < 4; ++e) av[e] = fmaxf(x[e] + g[e], 0.f);
      }
      st4<WT>(aA + k * ldj + j, av);
    }
    __syncthreads();
    // ---- logits = W_out . a + b_out: pairs of 16-row tiles over the V1 (+ D) output rows
    {
      const int ntiles = (N + 15) >> 4;
      for (int pr = wave; pr * 2 < ntiles; pr += SG_WAVES) {
        const WT* wr[2]; f32x4 acc[2]; int n[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          n[t] = (pr * 2 + t) * 16 + l16;
          wr[t] = (const WT*)p.w_out + (long long)min(n[t], N - 1) * p.ld_out;
          acc[t] = {0.f, 0.f, 0.f, 0.f};
        }
        rb_mma<WT, 2, 4>(wr, aA + l16 * ldj, J, acc);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          if (n[t] < N) {
            const float bv = p.b_out[n[t]];
#pragma unroll
            for (int r = 0; r < 4; ++r) lgs[(lg4 * 4 + r) * ldl + n[t]] = acc[t][r] + bv;
          }
        }
      }
    }
    __syncthreads();
    // ---- a wave per two rows: first arg-max, log-sum-exp, TDT duration; lane 0 moves the row on
    for (int rr = 0; rr < 2; ++rr) {
      const int m = wave * 2 + rr;
      if (!s_live[m]) continue;   // (wave-uniform)
      const float* lg = lgs + m * ldl;
      float bv = -INFINITY; int bi = 0x7fffffff;
      for (int v = lane; v < V1; v += 64) { const float q = lg[v]; if (q > bv) { bv = q; bi = v; } }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
      }
      float se = 0.f;
      for (int v = lane; v < V1; v += 64) se += expf(lg[v] - bv);
      se = wave_sum(se);
      if (lane == 0) {
        const int b = b0 + m, len = s_len[m];
        const int k = (bi < 0 || bi >= V1) ? p.blank : bi;   // (no logit is a number: a blank)
        int t = s_t[m], sym = s_sym[m], n = s_n[m];
        bool label = k != p.blank;
        int adv = 0;
        if constexpr (TDT) {
          int di = 0;   // first maximum wins, as for the labels
          for (int i = 1; i < D; ++i) if (lg[V1 + i] > lg[V1 + di]) di = i;
          int d = 0;
#pragma unroll
          for (int i = 0; i < TDT_MAXD; ++i) d = (i == di) ? p.dur.d[i] : d;
          if (!label) { adv = max(d, 1); sym = 0; }
          else {
            sym = d == 0 ? sym + 1 : 0;
            if (d == 0 && p.max_symbols > 0 && sym >= p.max_symbols) { d = 1; sym = 0; }
            adv = d;
          }
        } else {
          if (!label) { adv = 1; sym = 0; }
          else if (p.max_symbols > 0) { if (++sym >= p.max_symbols) { adv = 1; sym = 0; } }
          else if (n + 1 >= p.max_out) adv = len;   // unlimited symbols per frame: the output budget ends the stream
        }
        if (label) {
          if (n < p.max_out) {
            p.tokens[(long long)b * p.max_out + n] = k;
            if (p.times) p.times[(long long)b * p.max_out + n] = s_fd[m] + t;
          }
          ++n;
          s_score[m] += -logf(se);   // log-prob of the arg-max label = bv - (bv + log se)
#pragma unroll
          for (int c = SL_MAXC - 1; c > 0; --c) if (c < C) s_ctx[m][c] = s_ctx[m][c - 1];
          s_ctx[m][0] = k;
        }
        t = (int)min((long long)t + adv, (long long)len + TDT_MAXD);
        s_t[m] = t; s_sym[m] = sym; s_n[m] = n;
        s_live[m] = t < len && (!TDT || n < p.max_out);
      }
    }
    __syncthreads();
  }

  // ---- results: lengths, score, the next state; -1 behind every stream's labels
  if (tid < SG_M && b0 + tid < p.B) {
    const int b = b0 + tid, len = s_len[tid];
    p.out_len[b] = min(s_n[tid], p.max_out);
    if (p.score) p.score[b] = s_score[tid];
    if (p.sout.ctx) {
#pragma unroll
      for (int c = 0; c < SL_MAXC; ++c) if (c < C) p.sout.ctx[(long long)b * C + c] = s_ctx[tid][c];
      p.sout.score[b] = s_score[tid];
      p.sout.frames_done[b] = s_fd[tid] + len;
      p.sout.sym[b] = TDT ? s_sym[tid] : 0;
      p.sout.skip[b] = TDT ? max(s_t[tid] - len, 0) : 0;
    }
  }
  for (int i = tid; i < SG_M * p.max_out; i += SG_THREADS) {
    const int k = i / p.max_out, e = i - k * p.max_out;
    if (b0 + k < p.B && e >= s_n[k]) {
      p.tokens[(long long)(b0 + k) * p.max_out + e] = -1;
      if (p.times) p.times[(long long)(b0 + k) * p.max_out + e] = -1;
    }
  }
}

// ================================================================================================ entries
static size_t sg_lds_bytes(int wbytes, int V, int J, int N) {
  return (((size_t)SG_M * (J + V) * wbytes + 15) & ~(size_t)15) + (size_t)SG_M * (N | 1) * sizeof(float);
}

static int sl_train_args(const void* targets, const void* const* tabs, const void* act, int dtype, int B, int U, int E, int C, int V1,
                         int blank, SlTabs* tb) {
  if (!targets || !tabs || !act || B <= 0 || U < 0 || V1 <= 1 || blank < 0 || blank >= V1) return MI_ERR_ARG;
  if (dtype != MI_DT_F32 && dtype != MI_DT_BF16) return MI_ERR_ARG;
  if (sl_slices(E, C, tb)) return MI_ERR_ARG;
  for (int i = 0; i < C; ++i) if (!tabs[i] || ((size_t)tabs[i] & 3)) return MI_ERR_ARG;
  if ((size_t)act & 15 || (size_t)targets & 7) return MI_ERR_ARG;
  if ((long long)B * (U + 1) * E >= (1LL << 32)) return MI_ERR_ARG;   // (element indices of the dropout bits are 32-bit)
  return MI_OK;
}

extern "C" int mi355x_stateless_pred_fwd(const void* targets, const void* const* emb, void* out, int dtype, int B, int U, int E, int C,
                                         int V1, int blank, unsigned drop_key, unsigned drop_threshold, float drop_scale, void* stream) {
  mi_clear_errors();
  SlTabs tb;
  if (sl_train_args(targets, emb, out, dtype, B, U, E, C, V1, blank, &tb)) return MI_ERR_ARG;
  for (int i = 0; i < C; ++i) tb.emb[i] = (const float*)emb[i];
  const DropCfg drop = mi_drop(drop_key, drop_threshold, drop_scale);
  const int V = dtype == MI_DT_F32 ? 4 : 8;
  const long long n = (long long)B * (U + 1) * ((E + V - 1) / V);
  const dim3 grid((unsigned)((n + 255) / 256));
  if (dtype == MI_DT_F32)
    MI_LAUNCH(stateless_fwd_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const long long*)targets, tb, (float*)out, B, U, E, V1, blank, drop);
  else
    MI_LAUNCH(stateless_fwd_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const long long*)targets, tb, (bf16_t*)out, B, U, E, V1, blank, drop);
  return mi_check_launch();
}

extern "C" int mi355x_stateless_embed_bwd(const void* targets, const void* dg, int dtype, void* const* demb, int accumulate, int B, int U,
                                          int E, int C, int V1, int blank, unsigned drop_key, unsigned drop_threshold, float drop_scale,
                                          void* stream) {
  mi_clear_errors();
  SlTabs tb;
  if (sl_train_args(targets, (const void* const*)demb, dg, dtype, B, U, E, C, V1, blank, &tb)) return MI_ERR_ARG;
  for (int i = 0; i < C; ++i) tb.demb[i] = (float*)demb[i];
  const DropCfg drop = mi_drop(drop_key, drop_threshold, drop_scale);
  const dim3 grid((V1 + SL_BWD_ROWS - 1) / SL_BWD_ROWS, C);
  if (dtype == MI_DT_F32)
    MI_LAUNCH(stateless_embed_bwd_kernel<float>, grid, dim3(SL_BWD_THREADS), 0, (hipStream_t)stream, (const long long*)targets, (const float*)dg, tb,
              accumulate != 0, B, U, E, V1, blank, drop);
  else
    MI_LAUNCH(stateless_embed_bwd_kernel<bf16_t>, grid, dim3(SL_BWD_THREADS), 0, (hipStream_t)stream, (const long long*)targets, (const bf16_t*)dg, tb,
              accumulate != 0, B, U, E, V1, blank, drop);
  return mi_check_launch();
}

extern "C" int mi355x_stateless_tables(const void* const* emb, const void* w_pred, long long ld_pred, int w_dtype, void* tables, int E,
                                       int C, int V1, int J, int blank, void* stream) {
  mi_clear_errors();
  SlTabs tb;
  if (!emb || !w_pred || !tables || V1 <= 1 || J <= 0 || blank < 0 || blank >= V1 || ld_pred < E) return MI_ERR_ARG;
  if (w_dtype != MI_DT_F32 && w_dtype != MI_DT_BF16) return MI_ERR_ARG;
  if (sl_slices(E, C, &tb)) return MI_ERR_ARG;
  for (int i = 0; i < C; ++i) {
    if (!emb[i] || ((size_t)emb[i] & 3)) return MI_ERR_ARG;
    tb.emb[i] = (const float*)emb[i];
  }
  if (((size_t)tables & 15) || ((size_t)w_pred & (w_dtype == MI_DT_F32 ? 3 : 1))) return MI_ERR_ARG;
  const int jt = (J + 15) / 16, wpb = SL_TAB_THREADS / 64;
  const dim3 grid((V1 + 15) / 16, (jt + wpb - 1) / wpb, C);
  if (w_dtype == MI_DT_F32)
    MI_LAUNCH(stateless_tables_kernel<float>, grid, dim3(SL_TAB_THREADS), 0, (hipStream_t)stream, tb, (const float*)w_pred, ld_pred, (float*)tables, V1, J, blank);
  else
    MI_LAUNCH(stateless_tables_kernel<bf16_t>, grid, dim3(SL_TAB_THREADS), 0, (hipStream_t)stream, tb, (const bf16_t*)w_pred, ld_pred, (float*)tables, V1, J, blank);
  return mi_check_launch();
}

// every check is here; nothing is launched after a refusal
static int sg_decode_impl(const mi355x_stateless_greedy_desc* d, hipStream_t s) {
  if (!d) return MI_ERR_ARG;
  if (!d->enc_proj || !d->tables || !d->b_pred || !d->w_out || !d->b_out || !d->tokens || !d->out_len) return MI_ERR_ARG;
  const int B = d->B, J = d->J, V1 = d->V1, C = d->C;
  if (B <= 0 || d->T <= 0 || J <= 0 || V1 <= 1 || d->max_out <= 0 || d->blank < 0 || d->blank >= V1 || C < 1 || C > SL_MAXC) return MI_ERR_ARG;
  if ((d->f_dtype != MI_DT_F32 && d->f_dtype != MI_DT_BF16) || (d->w_dtype != MI_DT_F32 && d->w_dtype != MI_DT_BF16)) return MI_ERR_ARG;
  const bool bf = d->w_dtype == MI_DT_BF16;
  const int V = bf ? 8 : 4;   // elements of a 16-byte fragment
  if (J % V || d->ld_out % V || d->ld_out < J || d->ldf < J || d->ldf % 4) return MI_ERR_ARG;
  if (((size_t)d->w_out | (size_t)d->tables | (size_t)d->b_pred | (size_t)d->enc_proj) & 15) return MI_ERR_ARG;
  SgP p;
  p.dur = {};
  const bool tdt = d->D != 0 || d->durations;
  if (tdt && tdt_durations(d->D, d->durations, &p.dur)) return MI_ERR_ARG;
  p.sin = {}; p.sout = {};
  if (d->state_in && !d->state_out) return MI_ERR_ARG;
  for (int io = 0; io < 2; ++io) {   // a state is given whole or not at all
    const mi355x_stateless_stream_state* st = io ? d->state_out : d->state_in;
    if (!st) continue;
    if (!st->ctx || !st->score || !st->frames_done || !st->sym || !st->skip) return MI_ERR_ARG;
    (io ? p.sout : p.sin) = {st->ctx, st->score, st->frames_done, st->sym, st->skip};
  }
  if (p.sin.ctx && (p.sin.ctx == p.sout.ctx || p.sin.score == p.sout.score || p.sin.frames_done == p.sout.frames_done ||
                    p.sin.sym == p.sout.sym || p.sin.skip == p.sout.skip))
    return MI_ERR_ARG;
  const size_t shm = sg_lds_bytes(bf ? 2 : 4, V, J, V1 + p.dur.D);
  if (shm > 160 * 1024 - 8 * 1024) return MI_ERR_ARG;   // (the rows' scalars are static LDS)
  p.f = d->enc_proj; p.f_dt = d->f_dtype; p.ldf = d->ldf; p.enc_len = (const long long*)d->enc_len;
  p.tab = (const float*)d->tables; p.b_pred = (const float*)d->b_pred; p.w_out = d->w_out; p.ld_out = d->ld_out;
  p.b_out = (const float*)d->b_out;
  p.tokens = (int*)d->tokens; p.times = (int*)d->times; p.out_len = (int*)d->out_len; p.score = (float*)d->score;
  p.B = B; p.T = d->T; p.J = J; p.V1 = V1; p.C = C; p.blank = d->blank; p.max_symbols = d->max_symbols; p.max_out = d->max_out;
  static void (*const kernels[2][2])(SgP) = {{stateless_greedy_kernel<float, false>, stateless_greedy_kernel<float, true>},
                                            {stateless_greedy_kernel<bf16_t, false>, stateless_greedy_kernel<bf16_t, true>}};
  auto fn = kernels[bf][tdt];
  if (hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm) != hipSuccess) return MI_ERR_LAUNCH;
  MI_LAUNCH(fn, dim3((B + SG_M - 1) / SG_M), dim3(SG_THREADS), shm, s, p);
  return MI_OK;
}

extern "C" int mi355x_stateless_greedy_decode(const mi355x_stateless_greedy_desc* d, void* stream) {
  mi_clear_errors();
  const int rc = sg_decode_impl(d, (hipStream_t)stream);
  return rc != MI_OK ? rc : mi_check_launch();
}
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
