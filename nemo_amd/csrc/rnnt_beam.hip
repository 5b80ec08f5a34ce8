// Beam search of the transducer heads on the device (`strategy: malsd_batch`; RNN-T and TDT, one-shot): the whole search of a batch
// in ONE launch.  include/mi355x_asr.h states THE RULE (mi355x_transducer_beam_decode); this file is its kernel.
//
// The greedy search (rnnt_decode.hip) is a chain of matrix-VECTOR products: one hypothesis, one row, "not MFMA work".  A beam of W
// hypotheses is W rows against the same weights, so a step reads the weights once, as the greedy step does, and every product is a
// 16-row MFMA tile with the beam as M (W <= 16, unused rows zero):
//   * one workgroup per utterance, 8 waves; the waves split N: the 4H gate rows (as H/16 groups of the four gates of 16 hidden
//     units, so a wave holds i, f, g, o of its units in four accumulators and runs the cell in registers: the [16, 4H]
//     pre-activations are never stored), then the J prediction rows, then the V1 (+ D) output rows;
//   * the weight operand goes from global memory / L2 straight into the MFMA B layout: the rows are K-contiguous, so a lane's
//     fragment is ONE 16-byte load (bf16 images: v_mfma_f32_16x16x32_bf16, 8 k per lane; fp32 masters: four
//     v_mfma_f32_16x16x4_f32 on the four floats of the load, A permuted alike).  Weights never pass LDS, and 8 loads per lane are
//     in flight (rb_mma: tiles x unroll) -- the greedy search is bound by loads in flight, not bytes (profiles/rnnt_layers.md);
//   * the activation operand (A) is staged in LDS once per product, rows padded by 16 bytes against bank conflicts; K tails are
//     zero-filled in both operands, nothing is read past a row; the N tail is clamped to the last row and masked at the store;
//   * W_hh . h and W_ih . x accumulate into the same tile, the biases added where the rule's association has them;
//   * (h, c, gp) of the beam ping-pong between two halves of a caller-owned workspace (W = 16, H = 640 in float32 does not fit
//     twice into LDS next to the tiles); the gather through the parent slots is the read side of the next step;
//   * LDS: the A tiles (h, x, hn in the prediction step; relu(f + gp) in the joint step, over the same bytes), the [16, V1 + D]
//     logits (over the x / hn tiles, which are dead by then), the per-hypothesis scalars and the candidate lists;
//   * selection: each wave finds the W best candidates of the rows it owns (W rounds of "best key behind the last one": a strict
//     total order, so no taken-flags and no sort), wave 0 merges the sorted lists by their heads, a lane per row;
//   * prefix tree: (parent, token, frame) nodes in the workspace, node 1 + step * W + slot; a lane per hypothesis confirms a hash
//     match by walking both sequences, and chases its hypothesis out at the end;
//   * n-gram LM fusion (mi355x_transducer_beam_decode_fused; the LM instantiations): the wave that owns a row adds the model's
//     term to the row's label log-probabilities in place, one walk down the back-off chain per row (rb_lm_row), with a bit mask
//     per row behind the logits; the automaton state travels with the per-slot scalars.
// Ordinary vector stores and vector LDS atomics only, no scratch.
#include "common.h"
#include "ctc_beam_fusion.h"
#include "mi355x_asr.h"
#include "rnnt_mma.h"
#include "tdt.h"

#define RB_THREADS 512
#define RB_WAVES 8
#define RB_M 16        // rows of the MFMA tile = the widest beam
#define RB_NONE 0x7fffffff
#define RB_LM_CHAIN 6  // the fused search walks a back-off chain of up to 6 states before state 0 row-wise (an n-gram model of order
                       // N has chains of at most N - 1: orders up to 7, and files are built with 3 to 6); a longer chain takes
                       // the per-label look-up

struct RbP {
  const void* f; int f_dt; long long ldf;   // encoder projection [B, T, J] (rows of pitch ldf)
  const long long* enc_len;
  const float* emb;                          // [V1, H] fp32
  const void *w_ih, *w_hh, *w_pred, *w_out;  // [4H, H], [4H, H], [J, H], [V1 + D, J]
  long long ld_ih, ld_hh, ld_pred, ld_out;
  const float *b_ih, *b_hh, *b_pred, *b_out;
  int* tokens; int* times; int* out_len; float* score; int* n_hyp;
  char* ws; long long ws_per_b;              // workspace and its bytes per utterance
  int B, T, J, H, V1, blank, max_symbols, max_out, W;
  TdtDur dur;                                // TDT: duration set (dur.D = 0: RNN-T)
  ctc_beam_lm lm;                            // the fused search's model (read by the LM instantiations only)
};

// bytes of workspace per utterance: two halves of W state rows (h [H], c [H], gp [J], float32), then the prefix tree of
// 1 + W * (T + max_out) nodes of three ints
static __host__ __device__ inline long long rb_state_floats(int W, int H, int J) { return 2LL * W * (2LL * H + J); }
static inline long long rb_ws_per_b(int T, int H, int J, int W, int max_out) {
  const long long bytes = rb_state_floats(W, H, J) * 4 + (1 + (long long)W * ((long long)T + max_out)) * 12;
  return (bytes + 15) & ~15LL;
}

// lg[0 .. V1-1) += alpha * lm(s, v) for one row, by the wave that owns the row (mi355x_transducer_beam_decode_fused).  The value of
// label v is the look-up's: the back-off weights of the chain s_0 = s, s_1 = bo_next[s_0], .. summed in chain order until a state
// has an arc for v, then that arc's log-probability.  A look-up per (row, label) is V1 x depth binary searches of dependent loads;
// here the chain is walked ONCE per row from s down to state 0, the lanes take the arcs of a state 64 at a time (arc_tok / arc_logp
// coalesced), add the term in place into the row's log-probabilities and mark the label in the row's bit mask (LDS atomic-or: the
// returned word says whether a longer context had the label already, which also keeps a table with a repeated arc to one term per
// label); state 0 is dense (arc index = label) and finishes every label no longer context had.  Cost: V1 + the arcs on the chain.
// The chain is wave-uniform, so its loads are scalar.  Every index is clamped as ctc_beam_lm_lookup clamps it; a chain that does not
// reach state 0 within RB_LM_CHAIN states (a model of order > 7, or a table that breaks the rules) takes the look-up per label.
// The blank (V1 - 1) is never touched.  `msk`: (V1 + 31) / 32 words of this row.
__device__ __forceinline__ void rb_lm_row(const ctc_beam_lm& lm, int s0, float* lg, unsigned* msk, int V1, int lane) {
  const int L = V1 - 1;
  s0 = __builtin_amdgcn_readfirstlane(min(max(s0, 0), lm.n_states - 1));
  int depth = 0;
  for (int s = s0; s != 0 && depth <= RB_LM_CHAIN; ++depth) s = __builtin_amdgcn_readfirstlane(min(max(lm.bo_next[s], 0), lm.n_states - 1));
  if (depth > RB_LM_CHAIN) {   // (uniform)
    for (int v = lane; v < L; v += 64) {
      int nx;
      lg[v] += ctc_beam_alpha_lm(lm.alpha, ctc_beam_lm_lookup(lm, s0, v, nx));
    }
    return;
  }
  for (int i = lane; i * 32 < V1; i += 64) msk[i] = 0u;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  float acc = 0.f;
  int s = s0;
  for (int j = 0; j < depth; ++j) {   // the states before state 0, the longest context first
    const int lo = __builtin_amdgcn_readfirstlane(min(max(lm.arc_begin[s], 0), lm.n_arcs));
    const int end = __builtin_amdgcn_readfirstlane(min(max(lm.arc_begin[s + 1], lo), lm.n_arcs));
    for (int a = lo + lane; a < end; a += 64) {
      const int tok = lm.arc_tok[a];
      if (tok < 0 || tok >= L) continue;
      const unsigned bit = 1u << (tok & 31);
      if (atomicOr(&msk[tok >> 5], bit) & bit) continue;
      lg[tok] += ctc_beam_alpha_lm(lm.alpha, acc + lm.arc_logp[a]);
    }
    acc += lm.bo[s];
    s = __builtin_amdgcn_readfirstlane(min(max(lm.bo_next[s], 0), lm.n_states - 1));
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  for (int v = lane; v < L; v += 64)
    if (!((msk[v >> 5] >> (v & 31)) & 1u)) lg[v] += ctc_beam_alpha_lm(lm.alpha, acc + lm.arc_logp[v]);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// LM: the search of mi355x_transducer_beam_decode_fused (one n-gram model, p.lm); false: mi355x_transducer_beam_decode, whose
// instantiations hold no instruction of the model's
template <typename WT, bool TDT, bool LM>
__global__ __launch_bounds__(RB_THREADS) void rnnt_beam_kernel(RbP p) {
  constexpr int V = RbT<WT>::V;
  extern __shared__ __attribute__((aligned(16))) unsigned char rb_smem[];
  const int H = p.H, J = p.J, V1 = p.V1, W = p.W, D = TDT ? p.dur.D : 0, N = V1 + D;
  const int ldh = H + V, ldj = J + V, ldl = N | 1;
  // prediction step: hA, xA, hnA [16, ldh]; joint step: aA [16, ldj] over hA's bytes and the logits [16, ldl] behind it
  WT* hA = reinterpret_cast<WT*>(rb_smem);
  WT* xA = hA + RB_M * ldh;
  WT* hnA = xA + RB_M * ldh;
  WT* aA = reinterpret_cast<WT*>(rb_smem);
  float* lgs = reinterpret_cast<float*>(rb_smem + (((size_t)RB_M * ldj * sizeof(WT) + 15) & ~(size_t)15));
  unsigned* lmm = reinterpret_cast<unsigned*>(lgs + RB_M * ldl);   // LM: a bit per (row, label) behind the logits, (V1 + 31) / 32 words a row
  // the beam, two generations: [gen][slot]
  __shared__ float s_score[2][RB_M];
  __shared__ int s_live[2][RB_M], s_t[2][RB_M], s_sym[2][RB_M], s_n[2][RB_M], s_node[2][RB_M];
  __shared__ unsigned s_hash[2][RB_M];
  __shared__ int s_lms[2][RB_M];   // LM: the automaton state of the hypothesis
  // per parent row: its best candidates, best first (score, ordinal = (blank ? 0 : label + 1) * 8 + duration index)
  __shared__ float c_cs[RB_M][RB_M];
  __shared__ int c_ord[RB_M][RB_M], c_cnt[RB_M];
  // per new slot: its parent, whether it was extended by a label, and the label
  __shared__ int n_par[RB_M], n_ext[RB_M], n_tok[RB_M], s_any_ext, s_outlen[RB_M];

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, lg4 = lane >> 4;
  const int len = (int)min((long long)p.T, max(0LL, p.enc_len ? p.enc_len[b] : (long long)p.T));
  const int S = 2 * H + J;   // floats of a state row
  float* state = reinterpret_cast<float*>(p.ws + (long long)b * p.ws_per_b);
  int* nodes = reinterpret_cast<int*>(state + rb_state_floats(W, H, J));
  const long long n_nodes = 1 + (long long)W * ((long long)p.T + p.max_out);

  for (int i = tid; i < 3 * RB_M * ldh; i += RB_THREADS) hA[i] = rb_cvt<WT>(0.f);
  if (tid < 2 * RB_M) {
    const int g = tid >> 4, k = tid & 15;
    s_live[g][k] = (g == 0 && k == 0); s_score[g][k] = 0.f; s_t[g][k] = 0; s_sym[g][k] = 0; s_n[g][k] = 0; s_node[g][k] = 0; s_hash[g][k] = 0u;
    if constexpr (LM) s_lms[g][k] = 1;   // the state behind <s>
  }
  // the start of the search is a prediction step like any other: slot 0, "extended" from a parent row of zeros (half 1, row 0) by
  // the start-of-sequence input (no label: x = 0)
  if (tid < RB_M) { n_par[tid] = 0; n_ext[tid] = tid == 0; n_tok[tid] = -1; }
  if (tid == 0) { nodes[0] = -1; nodes[1] = -1; nodes[2] = -1; s_any_ext = 1; }
  for (int i = tid; i < 2 * H; i += RB_THREADS) state[(long long)W * S + i] = 0.f;
  __syncthreads();

  // ---- prediction step of the new generation `nx`: slots extended by a label run the LSTM cell and the prediction projection on
  // their parent's (h, c) and emb[label]; the others copy their parent's row
  auto pred_phase = [&](int nx) {
    float* dst = state + (long long)nx * W * S;
    const float* src = state + (long long)(nx ^ 1) * W * S;
    for (int i = tid; i < W * S; i += RB_THREADS) {
      const int k = i / S, e = i - k * S;
      if (s_live[nx][k] && !n_ext[k]) dst[(long long)k * S + e] = src[(long long)n_par[k] * S + e];
    }
    if (!s_any_ext) return;   // (uniform)
    for (int i = tid; i < W * H; i += RB_THREADS) {
      const int k = i / H, j = i - k * H;
      const bool ex = n_ext[k] != 0;
      hA[k * ldh + j] = rb_cvt<WT>(ex ? src[(long long)n_par[k] * S + j] : 0.f);
      xA[k * ldh + j] = rb_cvt<WT>(ex && n_tok[k] >= 0 ? p.emb[(long long)n_tok[k] * H + j] : 0.f);
    }
    __syncthreads();
    // the four gates of 16 hidden units per wave pass: z = ((W_hh . h + b_hh) + W_ih . x) + b_ih, then the cell, in registers
    for (int jt = wave; jt * 16 < H; jt += RB_WAVES) {
      const int j = jt * 16 + l16, jr = min(j, H - 1);
      const WT* wh[4]; const WT* wi[4];
      f32x4 acc[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        wh[g] = (const WT*)p.w_hh + (long long)(g * H + jr) * p.ld_hh;
        wi[g] = (const WT*)p.w_ih + (long long)(g * H + jr) * p.ld_ih;
        acc[g] = {0.f, 0.f, 0.f, 0.f};
      }
      rb_mma<WT, 4, 2>(wh, hA + l16 * ldh, H, acc);
#pragma unroll
      for (int g = 0; g < 4; ++g) { const float bv = p.b_hh[g * H + jr]; acc[g] += bv; }
      rb_mma<WT, 4, 2>(wi, xA + l16 * ldh, H, acc);
#pragma unroll
      for (int g = 0; g < 4; ++g) { const float bv = p.b_ih[g * H + jr]; acc[g] += bv; }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = lg4 * 4 + r;
        if (m < W && n_ext[m] && j < H) {
          const float c0 = src[(long long)n_par[m] * S + H + j];
          const float ig = 1.f / (1.f + expf(-acc[0][r])), fg = 1.f / (1.f + expf(-acc[1][r]));
          const float gg = tanhf(acc[2][r]), og = 1.f / (1.f + expf(-acc[3][r]));
          const float cc = fg * c0 + ig * gg, hh = og * tanhf(cc);
          dst[(long long)m * S + H + j] = cc;
          dst[(long long)m * S + j] = hh;
          hnA[m * ldh + j] = rb_cvt<WT>(hh);
        }
      }
    }
    __syncthreads();
    // gp = W_pred . hn + b_pred: pairs of 16-row tiles over J
    const int jtiles = (J + 15) >> 4;
    for (int pr = wave; pr * 2 < jtiles; pr += RB_WAVES) {
      const WT* wr[2]; f32x4 acc[2]; int n[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        n[t] = (pr * 2 + t) * 16 + l16;
        wr[t] = (const WT*)p.w_pred + (long long)min(n[t], J - 1) * p.ld_pred;
        acc[t] = {0.f, 0.f, 0.f, 0.f};
      }
      rb_mma<WT, 2, 4>(wr, hnA + l16 * ldh, H, acc);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (n[t] < J) {
          const float bv = p.b_pred[n[t]];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = lg4 * 4 + r;
            if (m < W && n_ext[m]) dst[(long long)m * S + 2 * H + n[t]] = acc[t][r] + bv;
          }
        }
      }
    }
  };

  int cur = 0;
  if (len > 0) pred_phase(0);
  __syncthreads();

  const int max_steps = len + p.max_out;
  for (int step = 0; step < max_steps; ++step) {
    bool active = false;   // (uniform)
    for (int k = 0; k < W; ++k) active |= s_live[cur][k] && s_t[cur][k] < len;
    if (!active) break;
    const int nx = cur ^ 1;
    // ---- joint: a = relu(enc_proj[t] + gp) of every live hypothesis with frames left (other rows zero), logits = W_out . a + b_out
    {
      const float* st = state + (long long)cur * W * S;
      for (int i = tid; i < RB_M * J; i += RB_THREADS) {
        const int k = i / J, j = i - k * J;
        float av = 0.f;
        if (k < W && s_live[cur][k] && s_t[cur][k] < len) {
          const long long row = ((long long)b * p.T + s_t[cur][k]) * p.ldf + j;
          const float fv = p.f_dt == MI_DT_F32 ? ((const float*)p.f)[row] : bf2f(((const bf16_t*)p.f)[row]);
          av = fmaxf(fv + st[(long long)k * S + 2 * H + j], 0.f);
        }
        aA[k * ldj + j] = rb_cvt<WT>(av);
      }
    }
    __syncthreads();
    {
      const int ntiles = (N + 15) >> 4;
      for (int pr = wave; pr * 2 < ntiles; pr += RB_WAVES) {
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
    // ---- candidates: each wave lists the W best of the rows it owns, best first
    for (int m = wave; m < W; m += RB_WAVES) {
      if (!s_live[cur][m]) { if (lane == 0) c_cnt[m] = 0; continue; }
      const float sc = s_score[cur][m];
      if (s_t[cur][m] >= len) {   // finished: offers itself
        if (lane == 0) { c_cs[m][0] = sc; c_ord[m][0] = 0; c_cnt[m] = 1; }
        continue;
      }
      float* lg = lgs + m * ldl;
      float mx = -INFINITY;
      for (int v = lane; v < V1; v += 64) mx = fmaxf(mx, lg[v]);
      mx = wave_max(mx);
      float se = 0.f;
      for (int v = lane; v < V1; v += 64) se += expf(lg[v] - mx);
      const float lse = mx + logf(wave_sum(se));
      for (int v = lane; v < V1; v += 64) lg[v] -= lse;   // lp, in place (each lane reads back its own)
      if constexpr (LM) {   // lpf over the labels, in place (lanes write each other's labels: LDS is in order within a wave)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        rb_lm_row(p.lm, s_lms[cur][m], lg, lmm + m * ((V1 + 31) >> 5), V1, lane);
      }
      float ld[TDT_MAXD];
      if constexpr (TDT) {
        float dm = -INFINITY, ds = 0.f;
#pragma unroll
        for (int i = 0; i < TDT_MAXD; ++i) { ld[i] = i < D ? lg[V1 + i] : -INFINITY; dm = fmaxf(dm, ld[i]); }
#pragma unroll
        for (int i = 0; i < TDT_MAXD; ++i) ds += i < D ? expf(ld[i] - dm) : 0.f;
        const float dl = dm + logf(ds);
#pragma unroll
        for (int i = 0; i < TDT_MAXD; ++i) ld[i] -= dl;
      }
      const bool blank_only = s_n[cur][m] >= p.max_out || (!TDT && p.max_symbols > 0 && s_sym[cur][m] >= p.max_symbols);
      float last_cs = INFINITY; int last_ord = -1, cnt = 0;
      for (int r = 0; r < W; ++r) {
        float bc = -INFINITY; int bo = RB_NONE;
        auto consider = [&](float cs, int ord) {
          if (!(cs > -INFINITY)) return;   // -inf and NaN are never kept
          if (!(cs < last_cs || (cs == last_cs && ord > last_ord))) return;
          if (cs > bc || (cs == bc && ord < bo)) { bc = cs; bo = ord; }
        };
        for (int v = lane; v < V1; v += 64) {
          if (blank_only && v != p.blank) continue;
          const int vo = (v == p.blank ? 0 : v + 1) * 8;
          if constexpr (TDT) {
#pragma unroll
            for (int i = 0; i < TDT_MAXD; ++i) if (i < D) consider(sc + (lg[v] + ld[i]), vo + i);
          } else {
            consider(sc + lg[v], vo);
          }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float oc = __shfl_xor(bc, o, 64); const int oo = __shfl_xor(bo, o, 64);
          if (oc > bc || (oc == bc && oo < bo)) { bc = oc; bo = oo; }
        }
        if (bo == RB_NONE) break;   // (uniform)
        if (lane == 0) { c_cs[m][r] = bc; c_ord[m][r] = bo; }
        last_cs = bc; last_ord = bo; ++cnt;
      }
      if (lane == 0) c_cnt[m] = cnt;
    }
    __syncthreads();
    // ---- select, merge: wave 0, lane k = new slot k
    if (wave == 0) {
      // the W best of the heads of the sorted lists (lane r < W: row r); ties: lower parent row, then lower ordinal
      int ptr = 0;
      const int cn = lane < W ? c_cnt[lane] : 0;
      float my_cs = -INFINITY; int my_po = RB_NONE;
      for (int k = 0; k < W; ++k) {
        const bool has = ptr < cn;
        float bc = has ? c_cs[lane & 15][ptr] : -INFINITY;
        int bo = has ? (lane << 20) | c_ord[lane & 15][ptr] : RB_NONE;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float oc = __shfl_xor(bc, o, 64); const int oo = __shfl_xor(bo, o, 64);
          if (oc > bc || (oc == bc && oo < bo)) { bc = oc; bo = oo; }
        }
        if (bo == RB_NONE) break;   // (uniform)
        if (lane == (bo >> 20)) ++ptr;
        if (lane == k) { my_cs = bc; my_po = bo; }
      }
      int live = my_po != RB_NONE, ext = 0, tok = -1, t = 0, sym = 0, n = 0, node = 0, pnode = 0, par = 0, frame = 0;
      unsigned hash = 0u;
      float score = my_cs;
      if (live) {
        par = my_po >> 20;
        const int ord = my_po & 0xfffff, vo = ord >> 3, di = ord & 7;
        t = s_t[cur][par]; sym = s_sym[cur][par]; n = s_n[cur][par]; pnode = s_node[cur][par]; hash = s_hash[cur][par];
        node = pnode;
        if (t < len) {
          const int v = vo == 0 ? p.blank : vo - 1;
          frame = t;
          if constexpr (TDT) {
            int d = 0;
#pragma unroll
            for (int i = 0; i < TDT_MAXD; ++i) d = (i == di) ? p.dur.d[i] : d;
            if (v == p.blank) {
              t += max(d, 1); sym = 0;
            } else {
              ext = 1;
              sym = d == 0 ? sym + 1 : 0;
              if (d == 0 && p.max_symbols > 0 && sym >= p.max_symbols) { d = 1; sym = 0; }
              t += d;
            }
          } else {
            if (v == p.blank) { t += 1; sym = 0; }
            else { ext = 1; sym += 1; }
          }
          if (ext) { tok = v; n += 1; hash = hash * 1000003u + (unsigned)(v + 1); node = 1 + step * W + lane; }
        }
      }
      // merge: `first` = the best-ranked selected slot with this slot's frame and token sequence.  The length and a rolling hash
      // screen; a match is confirmed by walking both sequences from their tails (the new label, then the parents' tree nodes,
      // all written in earlier steps) until they meet in one node.
      int first = lane;
      for (int j = 0; j < W; ++j) {
        const int lj = __shfl(live, j, 64), nj = __shfl(n, j, 64), tj = __shfl(t, j, 64), pj = __shfl(pnode, j, 64), kj = __shfl(tok, j, 64);
        const unsigned hj = __shfl(hash, j, 64);
        if (live && lj && j < lane && first == lane && n == nj && t == tj && hash == hj) {
          int na = pnode, ta = tok, nb = pj, tb = kj;
          bool same = true;
          for (int q = 0; q < n; ++q) {
            if (ta < 0 && tb < 0 && na == nb) break;
            int la, lb;
            if (ta >= 0) { la = ta; ta = -1; } else { la = nodes[3LL * na + 1]; na = nodes[3LL * na]; }
            if (tb >= 0) { lb = tb; tb = -1; } else { lb = nodes[3LL * nb + 1]; nb = nodes[3LL * nb]; }
            if (la != lb) { same = false; break; }
          }
          if (same) first = j;
        }
      }
      for (int j = 0; j < W; ++j) {   // a survivor gathers the scores merged into it, in rank order
        const int fj = __shfl(first, j, 64), lj = __shfl(live, j, 64);
        const float sj = __shfl(my_cs, j, 64);
        if (live && first == lane && lj && j > lane && fj == lane) {
          const float hi = fmaxf(score, sj), lo = fminf(score, sj);
          score = hi + log1pf(expf(lo - hi));
        }
      }
      live = live && first == lane;
      ext = ext && live;
      int lms = 1;
      if constexpr (LM) {   // a label moves the model to the state behind it; a blank and a finished hypothesis keep theirs
        if (lane < RB_M) lms = s_lms[cur][par];
        if (ext) ctc_beam_lm_lookup(p.lm, lms, tok, lms);
      }
      if (lane < RB_M) {
        s_live[nx][lane] = live; s_score[nx][lane] = score; s_t[nx][lane] = t; s_sym[nx][lane] = sym; s_n[nx][lane] = n;
        s_node[nx][lane] = node; s_hash[nx][lane] = hash;
        if constexpr (LM) s_lms[nx][lane] = lms;
        n_par[lane] = par; n_ext[lane] = ext; n_tok[lane] = ext ? tok : -1;
      }
      if (ext && node < n_nodes) { nodes[3LL * node] = pnode; nodes[3LL * node + 1] = tok; nodes[3LL * node + 2] = frame; }
      const unsigned long long any = __ballot(ext);
      if (lane == 0) s_any_ext = any != 0ull;
    }
    __syncthreads();
    pred_phase(nx);
    __syncthreads();
    cur = nx;
  }

  // ---- results: by score, best first, then by slot; a lane per hypothesis chases its sequence out of the tree
  if (tid < RB_M) s_outlen[tid] = 0;
  __syncthreads();
  if (wave == 0) {
    const int live = lane < W && s_live[cur][lane];
    const float sc = live ? s_score[cur][lane] : -INFINITY;
    int rank = 0, cnt = 0;
    for (int j = 0; j < W; ++j) {
      const int lj = __shfl(live, j, 64); const float sj = __shfl(sc, j, 64);
      cnt += lj;
      if (lj && (sj > sc || (sj == sc && j < lane))) ++rank;
    }
    if (lane == 0) p.n_hyp[b] = cnt;
    if (lane < W && lane >= cnt) { p.out_len[(long long)b * W + lane] = 0; p.score[(long long)b * W + lane] = -INFINITY; }
    if (live) {
      const int n = min(s_n[cur][lane], p.max_out);
      const long long o = ((long long)b * W + rank) * p.max_out;
      p.out_len[(long long)b * W + rank] = n; p.score[(long long)b * W + rank] = sc;
      s_outlen[rank] = n;
      int node = s_node[cur][lane];
      for (int i = n - 1; i >= 0 && node > 0; --i) {
        p.tokens[o + i] = nodes[3LL * node + 1]; p.times[o + i] = nodes[3LL * node + 2];
        node = nodes[3LL * node];
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < W * p.max_out; i += RB_THREADS) {   // -1 behind every hypothesis, and in the empty ranks
    const int r = i / p.max_out, e = i - r * p.max_out;
    if (e >= s_outlen[r]) { p.tokens[((long long)b * W + r) * p.max_out + e] = -1; p.times[((long long)b * W + r) * p.max_out + e] = -1; }
  }
}

// LDS of a launch: the larger of the prediction step's three A tiles and the joint step's A tile with the logits behind it
// (`mask_words`: the fused search's label masks behind the logits, per row)
static size_t rb_lds_bytes(int wbytes, int V, int H, int J, int N, int mask_words) {
  const size_t pred = (size_t)3 * RB_M * (H + V) * wbytes;
  const size_t joint = (((size_t)RB_M * (J + V) * wbytes + 15) & ~(size_t)15) + (size_t)RB_M * ((N | 1) + mask_words) * sizeof(float);
  return pred > joint ? pred : joint;
}

extern "C" long long mi355x_transducer_beam_workspace_bytes(int B, int T, int H, int J, int beam, int max_out) {
  if (B <= 0 || T <= 0 || H <= 0 || J <= 0 || beam < 1 || beam > RB_M || max_out <= 0) return -1;
  return (long long)B * rb_ws_per_b(T, H, J, beam, max_out);
}

// every check is here; nothing is launched after a refusal.  `fused`: the entry that takes a model (exactly one)
static int beam_decode_impl(const mi355x_transducer_beam_desc* d, const mi355x_ctc_beam_fusion* models, int n_models, bool fused,
                            hipStream_t s) {
  if (!d) return MI_ERR_ARG;
  if (fused && (!models || n_models != 1)) return MI_ERR_ARG;
  if (!d->enc_proj || !d->emb || !d->w_ih || !d->w_hh || !d->b_ih || !d->b_hh || !d->w_pred || !d->b_pred || !d->w_out || !d->b_out)
    return MI_ERR_ARG;
  if (!d->tokens || !d->times || !d->out_len || !d->score || !d->n_hyp || !d->workspace) return MI_ERR_ARG;
  const int B = d->B, H = d->H, J = d->J, V1 = d->V1, W = d->beam;
  if (B <= 0 || d->T <= 0 || J <= 0 || H <= 0 || V1 <= 1 || V1 >= (1 << 17) - 1 || d->max_out <= 0 || d->blank < 0 || d->blank >= V1)
    return MI_ERR_ARG;
  if (W < 1 || W > RB_M || (long long)W * ((long long)d->T + d->max_out) > 0x0fffffffll) return MI_ERR_ARG;
  if ((d->f_dtype != MI_DT_F32 && d->f_dtype != MI_DT_BF16) || (d->w_dtype != MI_DT_F32 && d->w_dtype != MI_DT_BF16)) return MI_ERR_ARG;
  const bool bf = d->w_dtype == MI_DT_BF16;
  const int V = bf ? 8 : 4;   // elements of a 16-byte fragment
  if (H % V || J % V || d->ld_ih % V || d->ld_hh % V || d->ld_pred % V || d->ld_out % V) return MI_ERR_ARG;
  if (d->ld_ih < H || d->ld_hh < H || d->ld_pred < H || d->ld_out < J || d->ldf < J) return MI_ERR_ARG;
  if (((size_t)d->w_ih | (size_t)d->w_hh | (size_t)d->w_pred | (size_t)d->w_out | (size_t)d->workspace) & 15) return MI_ERR_ARG;
  RbP p;
  p.dur = {};
  p.lm = {};
  if (fused) {   // an n-gram model over the labels 0 .. V1-2 (state 0's arc index is the label): the blank is the last class
    const mi355x_ctc_beam_fusion& m = models[0];
    if (!m.state_arc_begin || !m.arc_tok || !m.arc_logp || !m.arc_next || !m.state_bo || !m.state_bo_next || m.state_final) return MI_ERR_ARG;
    if (m.n_states < 2 || m.n_arcs < V1 - 1 || !(m.alpha >= 0.f) || !(m.alpha < INFINITY) || d->blank != V1 - 1) return MI_ERR_ARG;
    p.lm = {(const int*)m.state_arc_begin, (const int*)m.arc_tok, (const float*)m.arc_logp, (const int*)m.arc_next,
            (const float*)m.state_bo, (const int*)m.state_bo_next, m.n_states, m.n_arcs, m.alpha, m.ub, nullptr};
  }
  const bool tdt = d->D != 0 || d->durations;
  if (tdt && tdt_durations(d->D, d->durations, &p.dur)) return MI_ERR_ARG;
  p.ws_per_b = rb_ws_per_b(d->T, H, J, W, d->max_out);
  if (d->workspace_bytes < (long long)B * p.ws_per_b) return MI_ERR_ARG;
  const size_t shm = rb_lds_bytes(bf ? 2 : 4, V, H, J, V1 + p.dur.D, fused ? (V1 + 31) >> 5 : 0);
  if (shm > 160 * 1024 - 8 * 1024) return MI_ERR_ARG;   // (the beam's scalars and candidate lists are static LDS)
  p.f = d->enc_proj; p.f_dt = d->f_dtype; p.ldf = d->ldf; p.enc_len = (const long long*)d->enc_len; p.emb = (const float*)d->emb;
  p.w_ih = d->w_ih; p.w_hh = d->w_hh; p.w_pred = d->w_pred; p.w_out = d->w_out;
  p.ld_ih = d->ld_ih; p.ld_hh = d->ld_hh; p.ld_pred = d->ld_pred; p.ld_out = d->ld_out;
  p.b_ih = (const float*)d->b_ih; p.b_hh = (const float*)d->b_hh; p.b_pred = (const float*)d->b_pred; p.b_out = (const float*)d->b_out;
  p.tokens = (int*)d->tokens; p.times = (int*)d->times; p.out_len = (int*)d->out_len; p.score = (float*)d->score; p.n_hyp = (int*)d->n_hyp;
  p.ws = (char*)d->workspace;
  p.B = B; p.T = d->T; p.J = J; p.H = H; p.V1 = V1; p.blank = d->blank; p.max_symbols = d->max_symbols; p.max_out = d->max_out; p.W = W;
  static void (*const kernels[2][2][2])(RbP) = {
      {{rnnt_beam_kernel<float, false, false>, rnnt_beam_kernel<float, false, true>},
       {rnnt_beam_kernel<float, true, false>, rnnt_beam_kernel<float, true, true>}},
      {{rnnt_beam_kernel<bf16_t, false, false>, rnnt_beam_kernel<bf16_t, false, true>},
       {rnnt_beam_kernel<bf16_t, true, false>, rnnt_beam_kernel<bf16_t, true, true>}}};
  auto fn = kernels[bf][tdt][fused];
  if (hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm) != hipSuccess) return MI_ERR_LAUNCH;
  MI_LAUNCH(fn, dim3(B), dim3(RB_THREADS), shm, s, p);
  return MI_OK;
}

extern "C" int mi355x_transducer_beam_decode(const mi355x_transducer_beam_desc* d, void* stream) {
  mi_clear_errors();
  const int rc = beam_decode_impl(d, nullptr, 0, false, (hipStream_t)stream);
  return rc != MI_OK ? rc : mi_check_launch();
}

extern "C" int mi355x_transducer_beam_decode_fused(const mi355x_transducer_beam_desc* d, const mi355x_ctc_beam_fusion* models,
                                                   int n_models, void* stream) {
  mi_clear_errors();
  const int rc = beam_decode_impl(d, models, n_models, true, (hipStream_t)stream);
  return rc != MI_OK ? rc : mi_check_launch();
}
