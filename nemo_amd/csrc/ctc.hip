// CTC loss + gradient w.r.t. log-probabilities, one workgroup per utterance.
//   phase 1: alpha (waves 0-1) and beta (waves 2-3) recursions run CONCURRENTLY in log space over the blank-extended
//            label sequence (S = 2U+1 states, previous time-step row double-buffered in LDS, one barrier per step);
//            full lattices are written to a workspace [B, T, S] each.
//   phase 2: grad[t,c] = -exp(alpha+beta - logp + nll) summed over the states carrying class c, scaled by grad_scale
//            (1/B for 'mean_batch'); one wave per time-step, per-wave class accumulators in LDS (ds_add_f32).
// zero_infinity: an infeasible utterance gets loss 0 and zero gradient.
//
// Replaces on the reference path: torch.nn.functional.ctc_loss forward+backward called by
//   nemo/collections/asr/losses/ctc.py:68-82 (CTCLoss(blank=V, reduction='none', zero_infinity=True) + mean_batch).
#include <stdlib.h>
#include <type_traits>
#include "common.h"
#include "ctc_beam_fusion.h"
#include "mi355x_asr.h"

#define NEGINF (-INFINITY)

__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  if (m == NEGINF) return NEGINF;
  return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}
// Negative log-likelihood from the last alpha row: l1 = state S-1, l2 = state S-2 (-inf where S = 1), natural log.  Both lattice
// kernels and the gradient kernel take it from here, so the three values are bit-equal by construction.
__device__ __forceinline__ float ctc_nll(float l1, float l2) {
  const float m = fmaxf(l1, l2);
  return -((m == NEGINF) ? NEGINF : m + logf(expf(l1 - m) + expf(l2 - m)));
}

// logp [B, Tmax, C] f32 ; targets [B, Umax] i64 ; alpha/beta workspaces [B, Tmax, Smax]; grad [B, Tmax, C]
__global__ __launch_bounds__(256) void ctc_kernel(const float* __restrict__ logp, const long long* __restrict__ targets,
                                                  const long long* __restrict__ in_len, const long long* __restrict__ tgt_len,
                                                  float* __restrict__ alpha_ws, float* __restrict__ beta_ws,
                                                  float* __restrict__ nll_out, int Tmax, int C, int Umax, int Smax, int blank,
                                                  int zero_infinity) {
  extern __shared__ float sm[];
  int* ext = (int*)sm;                 // [Smax]
  float* prev_a = sm + Smax;           // [2][Smax]
  float* prev_b = prev_a + 2 * Smax;   // [2][Smax]

  const int b = blockIdx.x;
  const int T = (int)min((long long)Tmax, in_len[b]);
  const int U = (int)min((long long)Umax, tgt_len[b]);
  const int S = 2 * U + 1;
  const float* lp = logp + (long long)b * Tmax * C;
  float* aw = alpha_ws + (long long)b * Tmax * Smax;
  float* bw = beta_ws + (long long)b * Tmax * Smax;
  const int tid = threadIdx.x;

  for (int s = tid; s < S; s += 256) ext[s] = (s & 1) ? (int)targets[(long long)b * Umax + (s >> 1)] : blank;
  __syncthreads();

  if (T <= 0) {  // empty input: feasible only for an empty target
    if (tid == 0) nll_out[b] = (U == 0) ? 0.f : (zero_infinity ? 0.f : INFINITY);
    return;
  }

  // ---------------- phase 1: alpha on threads [0,128), beta on threads [128,256)
  const bool is_beta = tid >= 128;
  const int ht = tid & 127;
  float* prev = is_beta ? prev_b : prev_a;
  float* ws = is_beta ? bw : aw;
  // The emission term lp[t, ext[s]] does not depend on the recursion: it is fetched four time-steps ahead into a register
  // ring (a global load per step on the critical path was ~1 us x 501 steps = the whole kernel).  Ring slot = step & 3;
  // the loop is unrolled by 4 so that the slot is a compile-time register.
  const int cls0 = (ht < S) ? ext[ht] : blank;
  auto emit = [&](int step) -> float {
    const int t = is_beta ? (T - 1 - step) : step;
    return (step < T && ht < S) ? lp[(long long)t * C + cls0] : 0.f;
  };
  float ring[4] = {emit(0), emit(1), emit(2), emit(3)};
  for (int step0 = 0; step0 < T; step0 += 4) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int step = step0 + k;
      if (step < T) {  // uniform over the workgroup
        const float e0 = ring[k];
        ring[k] = emit(step + 4);
        const int t = is_beta ? (T - 1 - step) : step;
        float* cur = prev + ((step & 1) ? Smax : 0);
        const float* old = prev + ((step & 1) ? 0 : Smax);
        for (int s = ht; s < S; s += 128) {
          float v;
          const int cls = (s == ht) ? cls0 : ext[s];
          const float e = (s == ht) ? e0 : lp[(long long)t * C + cls];
          if (step == 0) {
            if (!is_beta) v = (s < 2) ? e : NEGINF;
            else v = (s >= S - 2) ? e : NEGINF;
          } else {
            float a = old[s], bb, c = NEGINF;
            if (!is_beta) {
              bb = (s >= 1) ? old[s - 1] : NEGINF;
              if (s >= 2 && cls != blank && cls != ext[s - 2]) c = old[s - 2];
            } else {
              bb = (s + 1 < S) ? old[s + 1] : NEGINF;
              if (s + 2 < S && cls != blank && cls != ext[s + 2]) c = old[s + 2];
            }
            const float m = lse3(a, bb, c);
            v = (m == NEGINF) ? NEGINF : m + e;
          }
          cur[s] = v;
          ws[(long long)t * Smax + s] = v;
        }
        __syncthreads();
      }
    }
  }
  // log-likelihood from the last alpha row (= row (T-1)&1 of prev_a)
  if (tid == 0) {
    const float* last = prev_a + (((T - 1) & 1) ? Smax : 0);
    float out = ctc_nll(last[S - 1], (S > 1) ? last[S - 2] : NEGINF);
    if (out == INFINITY && zero_infinity) out = 0.f;
    nll_out[b] = out;
  }
}

// ---------------- phase 1, wave-resident form (round 5).  The kernel above spends its time on one workgroup barrier + an LDS round
// trip per time-step (~0.5 us x 501 steps = 247 us at the headline shapes, on the critical path between forward and backward:
// profiles/r4_roofline_per_kernel.md).  Here a lattice row never leaves the registers of ONE wave: lane l holds the P (blank, label)
// state pairs g = l*P .. l*P+P-1 (states 2g, 2g+1; S <= 128*P) and a step needs exactly one value (alpha) / two values (beta) from the
// neighbouring lane -- a wave shuffle, no barrier, no LDS round trip of the row.  grid (B, 2): workgroup y = 0 walks alpha forward
// in time, y = 1 walks beta backward.  A workgroup is two waves: wave 0 walks, wave 1 gathers the emissions lp[t, ext[s]] of the NEXT
// chunk of CTC_TC(P) time-steps into the other half of a double-buffered LDS image (all of a chunk's loads in flight at once), so
// the walker never waits for global memory; one barrier per chunk.  The lattices are written exactly as the kernel above writes
// them (both include the emission of their own time-step).
// The walker keeps its rows in the BASE-2 log domain (emissions are scaled by log2(e) on their way into LDS, lattice rows by ln 2
// on their way out): log-sum-exp is then the bare hardware v_exp_f32 / v_log_f32 pair -- the sum lies in [1, 3], so none of the
// range handling of expf / logf is needed.
#define CTC_LOG2E 1.4426950408889634f
#define CTC_LN2 0.6931471805599453f
__device__ __forceinline__ float lse2f(float a, float b) {
  const float m = fmaxf(a, b);
  return (m == NEGINF) ? NEGINF : m + __builtin_amdgcn_logf(__builtin_amdgcn_exp2f(a - m) + __builtin_amdgcn_exp2f(b - m));
}
__device__ __forceinline__ float lse3f(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  return (m == NEGINF) ? NEGINF
                       : m + __builtin_amdgcn_logf(__builtin_amdgcn_exp2f(a - m) + __builtin_amdgcn_exp2f(b - m) + __builtin_amdgcn_exp2f(c - m));
}
// ---- the scaffold of a wave-resident walk, shared by the loss (ctc_wave_walk) and the Viterbi pass (ctc_align_wave_kernel): which
// pairs a lane holds, how the emissions reach the walker and what it gets from the neighbouring lane.  The two differ in the step.
template <int P> struct CtcTc { static constexpr int v = P <= 2 ? 64 : 128 / P; };   // time-steps per chunk (<= 64: one blank load per lane)
// per pair of a lane: the label's class, which of its two states exist, whether the skip transition into (forward walk) / out of
// (BETA: backward walk) its label state exists
template <int P> struct CtcPairs {
  int cls[P];
  bool vE[P], vO[P], skip[P];
};
template <int P, bool BETA>
__device__ __forceinline__ void ctc_pairs_setup(CtcPairs<P>& q, const long long* __restrict__ tg, int U, int blank) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int g = lane * P + p;
    q.vE[p] = g <= U;
    q.vO[p] = g < U;
    q.cls[p] = q.vO[p] ? (int)tg[g] : blank;
    if (!BETA) q.skip[p] = q.vO[p] && g >= 1 && q.cls[p] != (int)tg[g - 1];
    else q.skip[p] = g + 1 < U && q.cls[p] != (int)tg[g + 1];
  }
}
// the last row, walker wave only: l1 = state S-1 = E_U, l2 = state S-2 = O_{U-1} (-inf where U = 0), in every lane
template <int P>
__device__ __forceinline__ void ctc_wave_last_row(const float (&E)[P], const float (&O)[P], int U, float& l1, float& l2) {
  const int lane = threadIdx.x & 63;
  float eU = NEGINF, oU = NEGINF;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int g = lane * P + p;
    if (g == U) eU = E[p];
    if (g == U - 1) oU = O[p];
  }
  l1 = __shfl(eU, U / P, 64);
  l2 = (U >= 1) ? __shfl(oU, (U - 1) / P, 64) : NEGINF;
}
// loader wave: the emissions of steps c*TC .. c*TC+TC-1 (REV: counted back from frame T-1; LOG2: scaled into the base-2 domain)
// -> dst.  LDS row of a time-step: [p][lane] label emissions, then the blank emission.
template <int P, bool REV, bool LOG2>
__device__ __forceinline__ void ctc_wave_gather(float* dst, const float* __restrict__ lp, const int (&cls)[P], int T, int C, int blank,
                                                int c) {
  constexpr int TC = CtcTc<P>::v, LD = 64 * P + 1;
  const int lane = threadIdx.x & 63;
  float v[TC][P];
#pragma unroll
  for (int i = 0; i < TC; ++i) {
    int step = c * TC + i;
    step = step < T ? step : T - 1;   // (steps beyond the utterance re-read its last row: no branch, never used)
    const float* row = lp + (long long)(REV ? (T - 1 - step) : step) * C;
#pragma unroll
    for (int p = 0; p < P; ++p) v[i][p] = row[cls[p]];
  }
  float vb = 0.f;
  if (lane < TC) {
    int step = c * TC + lane;
    step = step < T ? step : T - 1;
    vb = lp[(long long)(REV ? (T - 1 - step) : step) * C + blank];
  }
#pragma unroll
  for (int i = 0; i < TC; ++i)
#pragma unroll
    for (int p = 0; p < P; ++p) dst[i * LD + p * 64 + lane] = LOG2 ? v[i][p] * CTC_LOG2E : v[i][p];
  if (lane < TC) dst[lane * LD + 64 * P] = LOG2 ? vb * CTC_LOG2E : vb;
}
// The chunk loop of a workgroup's two waves: wave 1 gathers chunk c + 1 into the other half of s_e while wave 0 walks chunk c,
// one barrier per chunk.  The walker calls step(step, e_blank, e_label[P]) for the steps 0 .. T-1 in order.
template <int P, bool REV, bool LOG2, class Step>
__device__ __forceinline__ void ctc_wave_chunks(const float* __restrict__ lp, const int (&cls)[P], int T, int C, int blank,
                                                float (*s_e)[CtcTc<P>::v * (64 * P + 1)], Step step) {
  constexpr int TC = CtcTc<P>::v, LD = 64 * P + 1;
  const int lane = threadIdx.x & 63;
  const bool loader = threadIdx.x >= 64;   // wave-uniform
  const int nchunk = (T + TC - 1) / TC;
  if (loader) ctc_wave_gather<P, REV, LOG2>(s_e[0], lp, cls, T, C, blank, 0);
  __syncthreads();
  for (int c = 0; c < nchunk; ++c) {
    if (loader) {
      if (c + 1 < nchunk) ctc_wave_gather<P, REV, LOG2>(s_e[(c + 1) & 1], lp, cls, T, C, blank, c + 1);
    } else {
      const float* src = s_e[c & 1];
      const int nstep = min(TC, T - c * TC);
      // the emissions of step i + 1 are read while step i computes (an LDS read in front of its first use costs the recursion
      // ~100 cycles per step otherwise); row TC - 1 is re-read beyond the chunk (never used)
      float eb_n = src[64 * P], el_n[P];
#pragma unroll
      for (int p = 0; p < P; ++p) el_n[p] = src[p * 64 + lane];
      for (int i = 0; i < nstep; ++i) {
        const float eb = eb_n;
        float el[P];
#pragma unroll
        for (int p = 0; p < P; ++p) el[p] = el_n[p];
        const int i1 = i + 1 < TC ? i + 1 : TC - 1;
        eb_n = src[i1 * LD + 64 * P];
#pragma unroll
        for (int p = 0; p < P; ++p) el_n[p] = src[i1 * LD + p * 64 + lane];
        step(c * TC + i, eb, el);
      }
    }
    __syncthreads();   // chunk c + 1 is in LDS; the walker is done with chunk c's half
  }
}

template <int P, bool BETA>
__device__ __forceinline__ void ctc_wave_walk(const float* __restrict__ lp, const long long* __restrict__ tg, float* __restrict__ ws,
                                              float* __restrict__ nll_out, int T, int U, int C, int Smax, int blank, int zero_infinity,
                                              float (*s_e)[CtcTc<P>::v * (64 * P + 1)]) {
  const int lane = threadIdx.x & 63;
  CtcPairs<P> q;
  ctc_pairs_setup<P, BETA>(q, tg, U, blank);
  float E[P], O[P];
#pragma unroll
  for (int p = 0; p < P; ++p) { E[p] = NEGINF; O[p] = NEGINF; }
  ctc_wave_chunks<P, BETA, true>(lp, q.cls, T, C, blank, s_e, [&](int step, float eb, const float (&el)[P]) {
    // old values of the neighbouring lane's boundary pair (alpha: its last label state; beta: its first pair)
    float x0, x1 = NEGINF;
    if (!BETA) {
      x0 = __shfl_up(O[P - 1], 1, 64);
      if (lane == 0) x0 = NEGINF;
    } else {
      x0 = __shfl_down(E[0], 1, 64);
      x1 = __shfl_down(O[0], 1, 64);
      if (lane == 63) { x0 = NEGINF; x1 = NEGINF; }
    }
    float nE[P], nO[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      float a, cc;
      if (!BETA) {
        // alpha: E_g <- lse(E_g, O_{g-1}) + e_blank ; O_g <- lse(O_g, E_g, skip ? O_{g-1} : -inf) + e_label   (old values on the right)
        const float om1 = (p == 0) ? x0 : O[p == 0 ? 0 : p - 1];
        a = lse2f(E[p], om1);
        cc = lse3f(O[p], E[p], q.skip[p] ? om1 : NEGINF);
      } else {
        // beta: E_g <- lse(E_g, O_g) + e_blank ; O_g <- lse(O_g, E_{g+1}, skip ? O_{g+1} : -inf) + e_label
        const float ep1 = (p == P - 1) ? x0 : E[p == P - 1 ? p : p + 1];
        const float op1 = (p == P - 1) ? x1 : O[p == P - 1 ? p : p + 1];
        a = lse2f(E[p], O[p]);
        cc = lse3f(O[p], ep1, q.skip[p] ? op1 : NEGINF);
      }
      nE[p] = (q.vE[p] && a != NEGINF) ? a + eb : NEGINF;
      nO[p] = (q.vO[p] && cc != NEGINF) ? cc + el[p] : NEGINF;
    }
    if (step == 0) {  // (wave-uniform) alpha_0: states 0, 1 ; beta_{T-1}: states S-1, S-2
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const int g = lane * P + p;
        nE[p] = (g == (BETA ? U : 0)) ? eb : NEGINF;
        nO[p] = (q.vO[p] && g == (BETA ? U - 1 : 0)) ? el[p] : NEGINF;
      }
    }
    float* wrow = ws + (long long)(BETA ? (T - 1 - step) : step) * Smax + 2 * lane * P;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      E[p] = nE[p]; O[p] = nO[p];
      if (q.vE[p]) wrow[2 * p] = nE[p] * CTC_LN2;      // (-inf stays -inf)
      if (q.vO[p]) wrow[2 * p + 1] = nO[p] * CTC_LN2;
    }
  });
  if (!BETA && threadIdx.x < 64) {   // log-likelihood from the last alpha row
    float l1, l2;
    ctc_wave_last_row<P>(E, O, U, l1, l2);
    if (lane == 0) {
      float out = ctc_nll(l1 * CTC_LN2, l2 * CTC_LN2);
      if (out == INFINITY && zero_infinity) out = 0.f;
      *nll_out = out;
    }
  }
}

// grid (B, 2), two waves per workgroup (walker + emission loader): blockIdx.y = 0 walks alpha, 1 walks beta
template <int P>
__global__ __launch_bounds__(128) void ctc_wave_kernel(const float* __restrict__ logp, const long long* __restrict__ targets,
                                                       const long long* __restrict__ in_len, const long long* __restrict__ tgt_len,
                                                       float* __restrict__ alpha_ws, float* __restrict__ beta_ws,
                                                       float* __restrict__ nll_out, int Tmax, int C, int Umax, int Smax, int blank,
                                                       int zero_infinity) {
  const int b = blockIdx.x;
  const int T = (int)min((long long)Tmax, in_len[b]);
  const int U = (int)min((long long)Umax, tgt_len[b]);
  if (T <= 0) {  // empty input: feasible only for an empty target
    if (threadIdx.x == 0 && blockIdx.y == 0) nll_out[b] = (U == 0) ? 0.f : (zero_infinity ? 0.f : INFINITY);
    return;
  }
  __shared__ float s_e[2][CtcTc<P>::v * (64 * P + 1)];   // double-buffered emission chunks
  const float* lp = logp + (long long)b * Tmax * C;
  const long long* tg = targets + (long long)b * Umax;
  if (blockIdx.y == 0)
    ctc_wave_walk<P, false>(lp, tg, alpha_ws + (long long)b * Tmax * Smax, nll_out + b, T, U, C, Smax, blank, zero_infinity, s_e);
  else
    ctc_wave_walk<P, true>(lp, tg, beta_ws + (long long)b * Tmax * Smax, nullptr, T, U, C, Smax, blank, zero_infinity, s_e);
}

// Which form a launch takes, for the loss and the alignment alike.  A knob that was never set (< 0) is read from its environment
// variable at the first launch: "0..." = the LDS / barrier form always, anything else = the wave-resident form where it fits.
static int ctc_knob(int& knob, const char* env) {
  if (knob < 0) {
    const char* e = getenv(env);
    knob = (e && e[0] == '0') ? 0 : 1;
  }
  return knob;
}
// pairs per lane P of the wave-resident form (Smax <= 128 P states), 0 = the LDS / barrier form
static int ctc_wave_pairs(int wave, int Smax) { return (!wave || Smax > 1024) ? 0 : Smax <= 128 ? 1 : Smax <= 256 ? 2 : Smax <= 512 ? 4 : 8; }
#define CTC_DISPATCH(P, WAVE, LDS)                                                                                                 \
  switch (P) { case 1: WAVE(1); break; case 2: WAVE(2); break; case 4: WAVE(4); break; case 8: WAVE(8); break; default: LDS; }

// MI355X_CTC_WAVE (mi355x_ctc_config): 1 (default) = the wave-resident lattice kernel for S <= 1024 states, 0 = the LDS / barrier form
static int g_ctc_wave = -1;
extern "C" int mi355x_ctc_config(int wave) {
  const int prev = g_ctc_wave;
  g_ctc_wave = wave;
  return prev;
}

// ---------------- phase 2: gradient rows.  Its own launch: the lattice phase is sequential in T and occupies one workgroup per
// utterance (32 CUs at the headline batch), the gradient rows are independent -- grid (time blocks, B), one wave per time-step.
#define CTC_GT 8  // time-steps per workgroup (4 waves x 2)
__global__ __launch_bounds__(256) void ctc_grad_kernel(const float* __restrict__ logp, const long long* __restrict__ targets,
                                                       const long long* __restrict__ in_len, const long long* __restrict__ tgt_len,
                                                       const float* __restrict__ alpha_ws, const float* __restrict__ beta_ws,
                                                       float* __restrict__ grad, int Tmax, int C, int Umax, int Smax, int blank,
                                                       float grad_scale) {
  extern __shared__ float acc[];  // [4][C]
  const int b = blockIdx.y;
  const int T = (int)min((long long)Tmax, in_len[b]);
  const int U = (int)min((long long)Umax, tgt_len[b]);
  const int S = 2 * U + 1;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* lp = logp + (long long)b * Tmax * C;
  const float* aw = alpha_ws + (long long)b * Tmax * Smax;
  float nll = INFINITY;  // the un-clamped negative log-likelihood, from the last alpha row
  if (T > 0) nll = ctc_nll(aw[(long long)(T - 1) * Smax + S - 1], (S > 1) ? aw[(long long)(T - 1) * Smax + S - 2] : NEGINF);
  const float* bw = beta_ws + (long long)b * Tmax * Smax;
  float* g = grad + (long long)b * Tmax * C;
  float* wacc = acc + wave * C;
  const bool feasible = T > 0 && nll != INFINITY;  // infeasible (zero_infinity) / empty: zero rows
  for (int t = blockIdx.x * CTC_GT + wave; t < min(Tmax, (int)(blockIdx.x + 1) * CTC_GT); t += 4) {
    if (t >= T || !feasible) {  // frames beyond the utterance stay zero
      for (int c = lane; c < C; c += 64) g[(long long)t * C + c] = 0.f;
      continue;
    }
    for (int c = lane; c < C; c += 64) wacc[c] = 0.f;
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): LDS zeroing visible before the adds of this wave
    for (int s = lane; s < S; s += 64) {
      const float ab = aw[(long long)t * Smax + s] + bw[(long long)t * Smax + s];
      if (ab != NEGINF) {
        const int cls = (s & 1) ? (int)targets[(long long)b * Umax + (s >> 1)] : blank;
        atomicAdd(&wacc[cls], expf(ab - lp[(long long)t * C + cls] + nll));
      }
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    for (int c = lane; c < C; c += 64) g[(long long)t * C + c] = -grad_scale * wacc[c];
  }
}

extern "C" int mi355x_ctc_loss(const void* logp, const void* targets, const void* in_len, const void* tgt_len, void* alpha_ws,
                               void* beta_ws, void* nll, void* grad, int B, int Tmax, int C, int Umax, int blank,
                               float grad_scale, int zero_infinity, void* stream) {
  mi_clear_errors();
  if (!logp || !targets || !in_len || !tgt_len || !alpha_ws || !beta_ws || !nll) return MI_ERR_ARG;
  if (B <= 0 || Tmax <= 0 || C <= 0 || Umax < 0 || blank < 0 || blank >= C) return MI_ERR_ARG;
  const int Smax = 2 * Umax + 1;
  const size_t shm = sizeof(float) * ((size_t)Smax * 5);
  if (shm > 60 * 1024 || sizeof(float) * 4 * (size_t)C > 60 * 1024) return MI_ERR_ARG;
#define CTC_LATTICE(kernel, grid, threads, lds)                                                                                     \
  MI_LAUNCH(kernel, grid, dim3(threads), lds, (hipStream_t)stream, (const float*)logp, (const long long*)targets,                    \
            (const long long*)in_len, (const long long*)tgt_len, (float*)alpha_ws, (float*)beta_ws, (float*)nll, Tmax, C, Umax,    \
            Smax, blank, zero_infinity)
#define CTC_WAVE(PP) CTC_LATTICE(ctc_wave_kernel<PP>, dim3(B, 2), 128, 0)
  CTC_DISPATCH(ctc_wave_pairs(ctc_knob(g_ctc_wave, "MI355X_CTC_WAVE"), Smax), CTC_WAVE, CTC_LATTICE(ctc_kernel, dim3(B), 256, shm))
#undef CTC_WAVE
#undef CTC_LATTICE
  if (grad)
    MI_LAUNCH(ctc_grad_kernel, dim3((Tmax + CTC_GT - 1) / CTC_GT, B), dim3(256), sizeof(float) * 4 * (size_t)C,
                       (hipStream_t)stream, (const float*)logp, (const long long*)targets, (const long long*)in_len,
                       (const long long*)tgt_len, (const float*)alpha_ws, (const float*)beta_ws, (float*)grad, Tmax, C, Umax,
                       Smax, blank, grad_scale);
  return mi_check_launch();
}

// ------------------------------------------------------------------------------------------------ greedy CTC decoding
// GreedyCTCInfer._greedy_decode_logprobs (parts/submodules/ctc_greedy_decoding.py:333-361) + the CTC collapse of
// AbstractCTCDecoding.decode_hypothesis (parts/submodules/ctc_decoding.py:545-575), one workgroup per utterance, no host
// round trip: per-frame argmax (first maximum, like torch.max) and its log-probability, score = sum of the log-probs of
// the non-blank frames, tokens = labels with repeats folded and blanks removed (wave ballot + prefix popcount compaction).
// One kernel at three levels; what a level adds is compiled out of the levels below it.
//   LEVEL 0 (mi355x_ctc_greedy_decode): tokens, their count and the score.
//   LEVEL 1 (_ts): and the first and the last frame of the run of equal arg-max labels behind every kept token.  A run starts at the
//     frame the compaction keeps; it ends at the frame in front of the next frame whose label differs (or at the last valid frame),
//     and the token it belongs to is the latest keep at or before that frame -- the same ballot with an inclusive prefix, so runs
//     that cross a 64-frame group need nothing more.
//   LEVEL 2 (_conf): and confidences.  The wave that walks a frame's C log-probabilities for the arg-max carries the sums of the
//     chosen measure in the same pass (log-probs are <= 0, so p^alpha = exp(alpha x) needs no shift; a -inf class adds nothing) and
//     stores the frame's confidence.  After the compaction a lane per token folds the frame confidences of its range, read back
//     from frame_conf behind the barrier (a third per-frame array in LDS would not fit at Tmax = 8192 without raising the limit);
//     tok_start / tok_end / frame_conf are read back too, so they are not __restrict__.
__device__ __forceinline__ float ctc_conf_fold(float a, float b, int agg) {
  return agg == MI355X_CONF_AGG_MIN ? fminf(a, b) : agg == MI355X_CONF_AGG_MAX ? fmaxf(a, b) : agg == MI355X_CONF_AGG_PROD ? a * b : a + b;
}
template <int LEVEL>
__global__ __launch_bounds__(256) void ctc_greedy_kernel(const float* __restrict__ logp, const long long* __restrict__ lens,
                                                         int* __restrict__ tokens, int* __restrict__ out_len,
                                                         float* __restrict__ score, int* tok_start, int* tok_end, float* frame_conf,
                                                         float* __restrict__ tok_conf, int Tmax, int C, int blank, MiConf q, int agg,
                                                         int exclude_blank) {
  constexpr bool TS = LEVEL >= 1, CONF = LEVEL >= 2;
  extern __shared__ int s_lab[];  // [Tmax] labels ; then [Tmax] log-probs (as float)
  float* s_lp = reinterpret_cast<float*>(s_lab + Tmax);
  const int b = blockIdx.x;
  const int T = (int)min((long long)Tmax, lens ? lens[b] : (long long)Tmax);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* lp = logp + (long long)b * Tmax * C;
  int* tok = tokens + (long long)b * Tmax;
  int* ts = TS ? tok_start + (long long)b * Tmax : nullptr;
  int* te = TS ? tok_end + (long long)b * Tmax : nullptr;
  float* fc = CONF ? frame_conf + (long long)b * Tmax : nullptr;
  float* tc = CONF ? tok_conf + (long long)b * Tmax : nullptr;
  const bool sums = CONF && q.method != MI355X_CONF_MAX_PROB;   // (uniform)
  for (int t = wave; t < T; t += 4) {
    float best = -INFINITY; int arg = 0x7fffffff;
    float S = 0.f, G = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float v = lp[(long long)t * C + c];
      if (v > best) { best = v; arg = c; }
      if (sums) {
        const float e = expf(q.alpha * v);
        S += e;
        G += (v == -INFINITY) ? 0.f : e * v;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, 64); const int oa = __shfl_xor(arg, o, 64);
      if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    if (sums) { S = wave_sum(S); G = wave_sum(G); }
    if (lane == 0) {
      s_lab[t] = arg; s_lp[t] = best;
      if constexpr (CONF) fc[t] = mi_conf_value(q, expf(best), S, G);
    }
  }
  if constexpr (CONF)
    for (int t = T + (int)threadIdx.x; t < Tmax; t += 256) fc[t] = 0.f;   // padding
  __syncthreads();
  if (wave == 0) {
    int base = 0; float sc = 0.f;
    for (int t0 = 0; t0 < T; t0 += 64) {
      const int t = t0 + lane;
      const int cur = t < T ? s_lab[t] : blank;
      const int prev = (t > 0 && t < T) ? s_lab[t - 1] : blank;
      const bool nonblank = t < T && cur != blank;
      const bool keep = nonblank && cur != prev;
      if (nonblank) sc += s_lp[t];
      const unsigned long long m = __ballot(keep);
      const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
      if (keep) tok[pos] = cur;
      if constexpr (TS) {
        if (keep) ts[pos] = t;
        if (nonblank && (t + 1 >= T || s_lab[t + 1] != cur))   // (2 << 63 wraps to 0: the mask of lane 63 is all ones)
          te[base + __popcll(m & ((2ull << lane) - 1ull)) - 1] = t;
      }
      base += __popcll(m);
    }
    sc = wave_sum(sc);
    if (lane == 0) { out_len[b] = base; score[b] = sc; }
    for (int t = base + lane; t < Tmax; t += 64) {  // padding
      tok[t] = -1;
      if constexpr (TS) { ts[t] = -1; te[t] = -1; }
      if constexpr (CONF) tc[t] = 0.f;
    }
  }
  if constexpr (CONF) {
    __syncthreads();   // out_len / tok_start / tok_end / frame_conf of this workgroup are visible to all of its waves
    const int n = out_len[b];   // (all of the LDS a launch may have without a raised limit is the two per-frame arrays at Tmax = 8192)
    const float id = agg == MI355X_CONF_AGG_MIN ? INFINITY : agg == MI355X_CONF_AGG_MAX ? -INFINITY : agg == MI355X_CONF_AGG_PROD ? 1.f : 0.f;
    // A lane per token: its range is a handful of frames as a rule, folded in the lane (a wave per token spent its time on the two
    // dependent loads that find the range: 122 us of 237 at B = 32, T = 501).  A range of more than 64 frames -- a long run, or with
    // exclude_blank off a long silence in front of a token -- is folded by the whole wave instead, one such token after the other.
    for (int i0 = wave * 64; i0 < n; i0 += 256) {   // (uniform over the wave; 0 <= lo <= hi < T by construction of the runs)
      const int i = i0 + lane;
      const bool valid = i < n;
      const int hi = valid ? te[i] : -1;
      const int lo = !valid ? 0 : exclude_blank ? ts[i] : (i ? te[i - 1] + 1 : 0);
      const bool wide = valid && hi - lo >= 64;
      if (valid && !wide) {
        float a = id;
        for (int t = lo; t <= hi; ++t) a = ctc_conf_fold(a, fc[t], agg);
        tc[i] = agg == MI355X_CONF_AGG_MEAN ? a / (float)(hi - lo + 1) : a;
      }
      for (unsigned long long m = __ballot(wide); m; m &= m - 1) {
        const int l = __ffsll((long long)m) - 1;
        const int wlo = __shfl(lo, l, 64), whi = __shfl(hi, l, 64);
        float a = id;
        for (int t = wlo + lane; t <= whi; t += 64) a = ctc_conf_fold(a, fc[t], agg);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a = ctc_conf_fold(a, __shfl_xor(a, o, 64), agg);
        if (lane == 0) tc[i0 + l] = agg == MI355X_CONF_AGG_MEAN ? a / (float)(whi - wlo + 1) : a;
      }
    }
  }
}

// The one launcher behind the three entries: the checks, the LDS rule (two per-frame arrays: 8 Tmax bytes <= 64 KB) and the launch.
// Level 0 accepts blank == C (no class is the blank: nothing is dropped), as its entry always has; the two levels above it want
// the blank to be a class.
static int ctc_greedy_launch(int level, const void* logp, const void* lens, void* tokens, void* out_len, void* score, void* tok_start,
                             void* tok_end, void* frame_conf, void* tok_conf, int B, int Tmax, int C, int blank, MiConf q, int agg,
                             int exclude_blank, void* stream) {
  mi_clear_errors();
  if (!logp || !tokens || !out_len || !score || (level >= 1 && (!tok_start || !tok_end)) || (level >= 2 && (!frame_conf || !tok_conf)))
    return MI_ERR_ARG;
  if (B <= 0 || Tmax <= 0 || C <= 0 || blank < 0 || blank > (level == 0 ? C : C - 1)) return MI_ERR_ARG;
  if (level >= 2 && (!mi_conf_valid(C, q.method, q.norm, q.alpha) || agg < MI355X_CONF_AGG_MEAN || agg > MI355X_CONF_AGG_PROD))
    return MI_ERR_ARG;
  const size_t shm = (size_t)Tmax * 8;
  if (shm > 64 * 1024) return MI_ERR_ARG;
#define CTC_GREEDY(LEVEL)                                                                                                          \
  MI_LAUNCH(ctc_greedy_kernel<LEVEL>, dim3(B), dim3(256), shm, (hipStream_t)stream, (const float*)logp, (const long long*)lens,       \
            (int*)tokens, (int*)out_len, (float*)score, (int*)tok_start, (int*)tok_end, (float*)frame_conf, (float*)tok_conf, Tmax,  \
            C, blank, q, agg, exclude_blank)
  if (level == 0) CTC_GREEDY(0);
  else if (level == 1) CTC_GREEDY(1);
  else CTC_GREEDY(2);
#undef CTC_GREEDY
  return mi_check_launch();
}
extern "C" int mi355x_ctc_greedy_decode(const void* logp, const void* lens, void* tokens, void* out_len, void* score, int B,
                                        int Tmax, int C, int blank, void* stream) {
  return ctc_greedy_launch(0, logp, lens, tokens, out_len, score, nullptr, nullptr, nullptr, nullptr, B, Tmax, C, blank, MiConf{}, 0, 0,
                           stream);
}
extern "C" int mi355x_ctc_greedy_decode_ts(const void* logp, const void* lens, void* tokens, void* out_len, void* score,
                                           void* tok_start, void* tok_end, int B, int Tmax, int C, int blank, void* stream) {
  return ctc_greedy_launch(1, logp, lens, tokens, out_len, score, tok_start, tok_end, nullptr, nullptr, B, Tmax, C, blank, MiConf{}, 0, 0,
                           stream);
}
extern "C" int mi355x_ctc_greedy_decode_conf(const void* logp, const void* lens, void* tokens, void* out_len, void* score,
                                             void* tok_start, void* tok_end, void* frame_conf, void* tok_conf, int B, int Tmax, int C,
                                             int blank, int method, int norm, float alpha, float k0, float k1, float k2,
                                             int aggregation, int exclude_blank, void* stream) {
  return ctc_greedy_launch(2, logp, lens, tokens, out_len, score, tok_start, tok_end, frame_conf, tok_conf, B, Tmax, C, blank,
                           MiConf{method, norm, alpha, k0, k1, k2, (float)C}, aggregation, exclude_blank, stream);
}

// ------------------------------------------------------------------------------------------------ CTC forced alignment
// Viterbi pass of the reference's forced aligner (tools/nemo_forced_aligner/utils/viterbi_decoding.py: a Python loop over T on
// [B, S] tensors) as ONE launch per batch: the forward walk over the blank-extended lattice with max instead of log-sum-exp, a 2-bit
// predecessor choice per state and step, the backtrace and the expansion of the path into first / last frames per token.  Plain
// float32 in the natural-log domain, one max + one add per state and step: score and path are bit-equal to a float32 restatement.
//   v[0][0] = e(0,0), v[0][1] = e(0,1);  v[t][s] = max(v[t-1][s], v[t-1][s-1], skip ? v[t-1][s-2] : -inf) + e(t,s)
//   ties: the first maximum in the order (stay, s-1, s-2); at the last frame state S-1 unless v[S-2] > v[S-1]
// Backpointers: one byte per (blank, label) pair g and frame, bits 0-1 = choice of state 2g, bits 2-3 = choice of state 2g+1
// (choice = how many states the predecessor lies below), rows of RS = (Umax + 8) & ~7 bytes: bp_ws is u8 [B, Tmax, RS].
// A score of -inf (no path through the lattice: too few frames, or -inf emissions on every path) marks the utterance infeasible.
#ifndef CTC_ALIGN_BACKTRACE   // benchmarks only (tools/align_bench.py): 0 = forward walk alone, 2 = single-lane chase through global memory
#define CTC_ALIGN_BACKTRACE 1
#endif
#define CTC_BT 64      // frames per backtrace chunk
#define CTC_BT_LD 17   // dwords per row of the chunk's window: the pairs [g - 64, g] from a 4-byte aligned start are <= 68 bytes

// one (blank, label) pair: old values E = v[2g], O = v[2g+1], om1 = v[2g-1] -> the maxima in front of the emission and the choice byte
__device__ __forceinline__ unsigned ctc_vit_pair(float E, float O, float om1, bool skip, float& mE, float& mO) {
  unsigned kE = 0, kO = 0;
  mE = E;
  if (om1 > mE) { mE = om1; kE = 1; }
  mO = O;
  if (E > mO) { mO = E; kO = 1; }
  if (skip && om1 > mO) { mO = om1; kO = 2; }
  return kE | (kO << 2);
}

__device__ __forceinline__ void ctc_align_fill_empty(int* path, int* ts, int* te, int Tmax, int Umax) {
  for (int t = threadIdx.x; t < Tmax; t += blockDim.x) path[t] = -1;
  for (int u = threadIdx.x; u < Umax; u += blockDim.x) { ts[u] = -1; te[u] = -1; }
}

// Backtrace and expansion, by the whole workgroup behind its forward walk.  s_path[CTC_BT] holds the state of frame T-1 (-1:
// infeasible) and the caller has synchronised.  The state of frame t-k lies within 2k states below the state of frame t, so the
// backpointers a chunk of CTC_BT frames can touch are a window of <= 65 pairs per row: all threads fetch it into LDS with every load
// in flight, one lane chases inside LDS (a chase through global memory is one dependent load per frame), then a lane per frame
// stores the path and, where the state changes between neighbouring frames, the end of one token's run and the start of the next.
__device__ __forceinline__ void ctc_align_backtrace(const unsigned char* __restrict__ bp, int RS, int T, int U, int Tmax, int Umax,
                                                    int* __restrict__ path, int* __restrict__ ts, int* __restrict__ te,
                                                    unsigned* s_bp, int* s_path) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  int s_top = s_path[CTC_BT];
  if (s_top < 0) {   // (uniform)
    ctc_align_fill_empty(path, ts, te, Tmax, Umax);
    return;
  }
  for (int t = T + tid; t < Tmax; t += nthr) path[t] = -1;
  for (int u = U + tid; u < Umax; u += nthr) { ts[u] = -1; te[u] = -1; }
#if CTC_ALIGN_BACKTRACE == 0
  return;
#elif CTC_ALIGN_BACKTRACE == 2
  if (tid == 0) {
    int s = s_top;
    path[T - 1] = s;
    if (s & 1) te[s >> 1] = T - 1;
    for (int t = T - 1; t >= 1; --t) {
      const int n = s - ((bp[(long long)t * RS + (s >> 1)] >> ((s & 1) * 2)) & 3);
      if (n != s) { if (n & 1) te[n >> 1] = t - 1; if (s & 1) ts[s >> 1] = t; }
      path[t - 1] = s = n;
    }
    if (s & 1) ts[s >> 1] = 0;
  }
  return;
#endif
  if (tid == 0) {
    path[T - 1] = s_top;
    if (s_top & 1) te[s_top >> 1] = T - 1;
  }
  for (int t_hi = T - 1; t_hi >= 1;) {
    const int n = min(CTC_BT, t_hi);   // rows t_hi .. t_hi-n+1 lead to the states of frames t_hi-1 .. t_hi-n
    const int g_hi = s_top >> 1;
    const int a_lo = max(0, g_hi - CTC_BT) & ~3;
    const int ndw = ((g_hi - a_lo) >> 2) + 1;   // <= CTC_BT_LD; the last dword ends inside the row (RS is a multiple of 4)
    for (int i = tid; i < n * ndw; i += nthr) {
      const int k = i / ndw, j = i - k * ndw;
      s_bp[k * CTC_BT_LD + j] = *reinterpret_cast<const unsigned*>(bp + (long long)(t_hi - k) * RS + a_lo + 4 * j);
    }
    __syncthreads();
    if (tid == 0) {
      const unsigned char* w = reinterpret_cast<const unsigned char*>(s_bp);
      int s = s_top;
      for (int k = 0; k < n; ++k) {
        s -= (w[k * (CTC_BT_LD * 4) + (s >> 1) - a_lo] >> ((s & 1) * 2)) & 3;
        s_path[k] = s;
      }
      s_path[CTC_BT] = s;
    }
    __syncthreads();
    for (int k = tid; k < n; k += nthr) {
      const int cur = s_path[k], next = k ? s_path[k - 1] : s_top, t = t_hi - k - 1;
      path[t] = cur;
      if (cur != next) {
        if (cur & 1) te[cur >> 1] = t;
        if (next & 1) ts[next >> 1] = t + 1;
      }
    }
    s_top = s_path[CTC_BT];   // (the next chase writes it behind the next barrier)
    t_hi -= n;
  }
  if (tid == 0 && (s_top & 1)) ts[s_top >> 1] = 0;
}

// Wave-resident form, S <= 128 P: the layout of ctc_wave_walk -- lane l holds the pairs l*P .. l*P+P-1, one shuffle per step, wave 1
// gathers the next chunk's emissions into the other half of s_e, one barrier per chunk.  A lane stores its P choice bytes per step
// as one access.  The backtrace reuses s_e.
template <int P> struct CtcBytes;
template <> struct CtcBytes<1> { typedef unsigned char t; };
template <> struct CtcBytes<2> { typedef unsigned short t; };
template <> struct CtcBytes<4> { typedef unsigned int t; };
template <> struct CtcBytes<8> { typedef unsigned long long t; };
template <int P>
__global__ __launch_bounds__(128) void ctc_align_wave_kernel(const float* __restrict__ logp, const long long* __restrict__ targets,
                                                             const long long* __restrict__ in_len, const long long* __restrict__ tgt_len,
                                                             unsigned char* __restrict__ bp_ws, int* __restrict__ path_out,
                                                             int* __restrict__ tok_start, int* __restrict__ tok_end,
                                                             float* __restrict__ score, int Tmax, int C, int Umax, int RS, int blank) {
  constexpr int TC = CtcTc<P>::v, LD = 64 * P + 1;
  static_assert(TC * LD >= CTC_BT * CTC_BT_LD + CTC_BT + 1, "the backtrace buffers live in one half of s_e");
  __shared__ float s_e[2][TC * LD];
  const int b = blockIdx.x;
  const int T = (int)max(0ll, min((long long)Tmax, in_len[b]));
  const int U = (int)max(0ll, min((long long)Umax, tgt_len[b]));
  int* path = path_out + (long long)b * Tmax;
  int* ts = tok_start + (long long)b * Umax;
  int* te = tok_end + (long long)b * Umax;
  if (T == 0) {   // no frames: the empty path, feasible only for an empty target
    ctc_align_fill_empty(path, ts, te, Tmax, Umax);
    if (threadIdx.x == 0) score[b] = (U == 0) ? 0.f : NEGINF;
    return;
  }
  const float* lp = logp + (long long)b * Tmax * C;
  const long long* tg = targets + (long long)b * Umax;
  unsigned char* bp = bp_ws + (long long)b * Tmax * RS;
  const int lane = threadIdx.x & 63;
  CtcPairs<P> q;
  ctc_pairs_setup<P, false>(q, tg, U, blank);
  float E[P], O[P];
#pragma unroll
  for (int p = 0; p < P; ++p) { E[p] = NEGINF; O[p] = NEGINF; }
  ctc_wave_chunks<P, false, false>(lp, q.cls, T, C, blank, s_e, [&](int t, float eb, const float (&el)[P]) {
    float x0 = __shfl_up(O[P - 1], 1, 64);   // the neighbouring lane's last label state
    if (lane == 0) x0 = NEGINF;
    float nE[P], nO[P];
    unsigned long long choice = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      float mE, mO;
      const unsigned k = ctc_vit_pair(E[p], O[p], (p == 0) ? x0 : O[p == 0 ? 0 : p - 1], q.skip[p], mE, mO);
      choice |= (unsigned long long)k << (8 * p);
      nE[p] = q.vE[p] ? mE + eb : NEGINF;
      nO[p] = q.vO[p] ? mO + el[p] : NEGINF;
    }
    if (t == 0) {  // (wave-uniform) states 0 and 1
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const int g = lane * P + p;
        nE[p] = (g == 0) ? eb : NEGINF;
        nO[p] = (q.vO[p] && g == 0) ? el[p] : NEGINF;
      }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) { E[p] = nE[p]; O[p] = nO[p]; }
    if (lane * P <= U)   // (row 0 is never read; lane*P + P <= RS: both are multiples of P and lane*P <= Umax < RS)
      *reinterpret_cast<typename CtcBytes<P>::t*>(bp + (long long)t * RS + lane * P) = (typename CtcBytes<P>::t)choice;
  });
  unsigned* s_bp = reinterpret_cast<unsigned*>(s_e[0]);
  int* s_path = reinterpret_cast<int*>(s_e[0]) + CTC_BT * CTC_BT_LD;
  if (threadIdx.x < 64) {   // the last row: the better of states S-1 and S-2
    float l1, l2;
    ctc_wave_last_row<P>(E, O, U, l1, l2);
    if (lane == 0) {
      const bool lab = l2 > l1;
      const float sc = lab ? l2 : l1;
      score[b] = sc;
      s_path[CTC_BT] = (sc == NEGINF) ? -1 : (lab ? 2 * U - 1 : 2 * U);
    }
  }
  __syncthreads();   // (also: the walker's backpointer stores are visible to the whole workgroup)
  ctc_align_backtrace(bp, RS, T, U, Tmax, Umax, path, ts, te, s_bp, s_path);
}

// LDS / barrier form, S <= 4097: the previous row double-buffered in LDS (rows of 2 Umax + 2 floats, so that a pair is one aligned
// 8-byte read), a thread per pair and 256 pairs per pass, one barrier per step; the emissions of step t + 1 are requested before
// step t computes.
#define CTC_ALIGN_NG 9   // pairs per thread: 2049 pairs (U = 2048) over 256 threads
__host__ __device__ static inline int ctc_align_lds_rows(int Umax) { return (2 * (2 * Umax + 2) + 3) & ~3; }   // floats, a multiple of 16 bytes
__global__ __launch_bounds__(256) void ctc_align_kernel(const float* __restrict__ logp, const long long* __restrict__ targets,
                                                        const long long* __restrict__ in_len, const long long* __restrict__ tgt_len,
                                                        unsigned char* __restrict__ bp_ws, int* __restrict__ path_out,
                                                        int* __restrict__ tok_start, int* __restrict__ tok_end,
                                                        float* __restrict__ score, int Tmax, int C, int Umax, int RS, int blank) {
  // all of the LDS is dynamic (a static array in front would move the base off the 8-byte alignment of the pair reads):
  // rows [2][2 Umax + 2], then the backtrace window and path
  extern __shared__ __attribute__((aligned(16))) float rows[];
  const int Sr = 2 * Umax + 2;
  unsigned* s_bp = reinterpret_cast<unsigned*>(rows + ctc_align_lds_rows(Umax));
  int* s_path = reinterpret_cast<int*>(s_bp + CTC_BT * CTC_BT_LD);
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = (int)max(0ll, min((long long)Tmax, in_len[b]));
  const int U = (int)max(0ll, min((long long)Umax, tgt_len[b]));
  int* path = path_out + (long long)b * Tmax;
  int* ts = tok_start + (long long)b * Umax;
  int* te = tok_end + (long long)b * Umax;
  if (T == 0) {
    ctc_align_fill_empty(path, ts, te, Tmax, Umax);
    if (tid == 0) score[b] = (U == 0) ? 0.f : NEGINF;
    return;
  }
  const float* lp = logp + (long long)b * Tmax * C;
  const long long* tg = targets + (long long)b * Umax;
  unsigned char* bp = bp_ws + (long long)b * Tmax * RS;
  int cls[CTC_ALIGN_NG];
  bool skip[CTC_ALIGN_NG];
  float el_n[CTC_ALIGN_NG];
#pragma unroll
  for (int j = 0; j < CTC_ALIGN_NG; ++j) {
    const int g = tid + 256 * j;
    cls[j] = g < U ? (int)tg[g] : blank;
    skip[j] = g < U && g >= 1 && cls[j] != (int)tg[g - 1];
    el_n[j] = (256 * j <= U) ? lp[cls[j]] : 0.f;
  }
  float eb_n = lp[blank];
  for (int t = 0; t < T; ++t) {
    float* cur = rows + (t & 1) * Sr;
    const float* old = rows + ((t & 1) ^ 1) * Sr;
    const float eb = eb_n;
    float el[CTC_ALIGN_NG];
#pragma unroll
    for (int j = 0; j < CTC_ALIGN_NG; ++j) el[j] = el_n[j];
    const float* nrow = lp + (long long)min(t + 1, T - 1) * C;
    eb_n = nrow[blank];
#pragma unroll
    for (int j = 0; j < CTC_ALIGN_NG; ++j)
      if (256 * j <= U) el_n[j] = nrow[cls[j]];   // (uniform)
#pragma unroll
    for (int j = 0; j < CTC_ALIGN_NG; ++j) {
      const int g = tid + 256 * j;
      if (g <= U) {
        float nE, nO;
        unsigned k = 0;
        if (t == 0) {
          nE = (g == 0) ? eb : NEGINF;
          nO = (g == 0 && U > 0) ? el[j] : NEGINF;
        } else {
          const float2 eo = reinterpret_cast<const float2*>(old)[g];
          float mE, mO;
          k = ctc_vit_pair(eo.x, eo.y, g ? old[2 * g - 1] : NEGINF, skip[j], mE, mO);
          nE = mE + eb;
          nO = (g < U) ? mO + el[j] : NEGINF;
        }
        reinterpret_cast<float2*>(cur)[g] = make_float2(nE, nO);
        bp[(long long)t * RS + g] = (unsigned char)k;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float* last = rows + ((T - 1) & 1) * Sr;
    const float l1 = last[2 * U], l2 = (U >= 1) ? last[2 * U - 1] : NEGINF;
    const bool lab = l2 > l1;
    const float sc = lab ? l2 : l1;
    score[b] = sc;
    s_path[CTC_BT] = (sc == NEGINF) ? -1 : (lab ? 2 * U - 1 : 2 * U);
  }
  __syncthreads();
  ctc_align_backtrace(bp, RS, T, U, Tmax, Umax, path, ts, te, s_bp, s_path);
}

// MI355X_CTC_ALIGN_WAVE (mi355x_ctc_align_config): 1 (default) = the wave-resident form where 2 Umax + 1 <= 1024, 0 = the LDS form always
static int g_ctc_align_wave = -1;
extern "C" int mi355x_ctc_align_config(int wave) {
  const int prev = g_ctc_align_wave;
  g_ctc_align_wave = wave;
  return prev;
}

extern "C" int mi355x_ctc_align(const void* logp, const void* targets, const void* in_len, const void* tgt_len, void* bp_ws,
                                void* path, void* tok_start, void* tok_end, void* score, int B, int Tmax, int C, int Umax,
                                int blank, void* stream) {
  mi_clear_errors();
  if (!logp || !targets || !in_len || !tgt_len || !bp_ws || !path || !tok_start || !tok_end || !score) return MI_ERR_ARG;
  if (B <= 0 || Tmax <= 0 || C <= 0 || Umax <= 0 || blank < 0 || blank >= C) return MI_ERR_ARG;
  if (Umax > 2048 || ((size_t)bp_ws & 7)) return MI_ERR_ARG;   // S = 2 Umax + 1 <= 4097 (CTC_ALIGN_NG pairs per thread)
  const int Smax = 2 * Umax + 1, RS = (Umax + 8) & ~7;
#define CTC_ALIGN(kernel, threads, lds)                                                                                            \
  MI_LAUNCH(kernel, dim3(B), dim3(threads), lds, (hipStream_t)stream, (const float*)logp, (const long long*)targets,                 \
            (const long long*)in_len, (const long long*)tgt_len, (unsigned char*)bp_ws, (int*)path, (int*)tok_start, (int*)tok_end,  \
            (float*)score, Tmax, C, Umax, RS, blank)
#define CTC_WAVE(PP) CTC_ALIGN(ctc_align_wave_kernel<PP>, 128, 0)
  CTC_DISPATCH(ctc_wave_pairs(ctc_knob(g_ctc_align_wave, "MI355X_CTC_ALIGN_WAVE"), Smax), CTC_WAVE,
               CTC_ALIGN(ctc_align_kernel, 256, sizeof(float) * (size_t)(ctc_align_lds_rows(Umax) + CTC_BT * CTC_BT_LD + CTC_BT + 1)))
#undef CTC_WAVE
#undef CTC_ALIGN
  return mi_check_launch();
}

// ------------------------------------------------------------------------------------------------ CTC prefix beam search
// The classic CTC prefix beam search (the `beam_batch` strategy), with or without shallow fusion of token-level back-off automata
// (ctc_beam_kernel<NM, STREAM, FINAL>: one search, eight instantiations), ONE launch per batch, one wave per utterance,
// a lane per beam: the whole search state of an utterance lives in the registers of its wave, so the frame loop has no workgroup
// barrier, and nothing of size [B, T, C] leaves the device.  include/mi355x_asr.h states the search; in short, per frame:
//   token pruning   c is considered iff lp[t,c] >= max_c lp[t,c] - threshold (float32 subtract and compare)
//   stays           stay(i).pb = tot_i + lp[blank] ; stay(i).pnb = pnb_i + lp[last_i]
//   extensions      ext(i,c).pnb = (c == last_i ? pb_i : tot_i) + lp[c] ; where the prefix of ext(i,c) is the prefix of a beam j of
//                   the current set, the value is added (log-add-exp) to stay(j).pnb instead: the two are ONE candidate
//   selection       the `beam` candidates of the largest rank = tot + beta * len, tot = logaddexp(pb, pnb) > -inf
// A beam is a node of a prefix tree.  Node 0 is the empty prefix; the extension kept in slot s of frame t becomes node
// 1 + t*beam + s and stores (parent node, token) at node_ws[t*beam + s], so the frame a token was created in is (node - 1) / beam.
// Which beam an extension would duplicate: a beam carries a 64-bit hash of its prefix and of its parent's prefix; equal hash and
// length name the candidate, and the two parent chains are then compared node by node (no load at all where the beam's parent IS
// the extended beam's node, which is the rule; a walk only where a prefix fell out of the set and came back under a new node while
// one of its children stayed).  A hash alone never merges anything.
// Candidate streaming: a frame has up to beam * (C - 1) + beam candidates (65k at C = 1025, beam = 64).  They are never stored:
// lanes 0 .. beam-1 hold a running top-`beam` (rank, key, value) IN ORDER, initialised with the sorted stays; the extensions of one
// beam are formed 64 classes at a time, a ballot keeps those that beat the last entry, and each of them is inserted at its place:
// a ballot counts the entries in front of it, the entries behind move one lane up (a DPP wave shift, no LDS) and the last one falls
// off.  The bar is the entry in lane beam-1.  A beam whose best possible extension (tot_i + max_c lp) does not beat it is skipped
// whole; the beams are in order, so the bar rises early, and at the end of the frame lane s holds slot s: nothing is sorted again.
// LDS holds two rows of log-probabilities only: see the launcher.
// Ties: candidates are ordered by (rank descending, key ascending), key = i for stay(i) and beam + i*C + c for ext(i,c), i the slot
// of the beam in the sorted set of the previous frame; the order is total, so selection and output order are deterministic.
// Arithmetic: plain float32, logaddexp(a,b) = max + log1pf(expf(-|a-b|)); beta * len is rounded on its own (no fused multiply-add).
// Fusion models (NM of the kernel template = their number, 0 .. 2: an n-gram language model, a boosting tree, or both): each is the
// back-off automaton of include/mi355x_asr.h in six global arrays, small and shared by every wave, so they stay in L2; LDS holds
// what it held.  A beam carries, per model, its automaton state and m(prefix) (`m_state[k]`, `m_sum[k]`: registers that travel with
// it in the end-of-frame shuffle; k is a constant everywhere, `CTC_BEAM_EACH_MODEL`, so they stay registers), and
//   rank = ((tot + beta * len) + alpha_0 * m_0(prefix)) + alpha_1 * m_1(prefix)     each product rounded on its own; nothing else of
// the search changes.  m(prefix . c) = m_sum + look-up(m_state, c), and a look-up <= ub, so every early-out keeps its form with
// alpha_k * (m_sum[k] + ub_k) added to the side of the candidate in the same association (`ctc_beam_bound`): rounding is monotone,
// alpha >= 0, the bar only rises.  In the streamed loop that bound, which needs no look-up, is tested first and only the lanes that
// pass it walk the tables (a binary search in the arcs of the state, a direct index at state 0); the ballot sees exact ranks.  The
// running top-W stays (rank, key, value): a kept extension repeats its look-ups at the end of the frame -- same inputs, same
// values -- to get its sums and next states.  Every chase is bounded (back-off chain: n_states steps, binary search: 32) and every
// index is clamped to its table, so tables that are not what the loader checks give a wrong score, never a hang or a stray load.
// At output a model's `state_final` table (fin; null: none) adds alpha * fin[state] to each hypothesis' score, the hypotheses are
// re-ordered inside the wave by (that score descending, slot ascending) -- a rank count over readlanes and one ds_permute, no LDS;
// the identity where no model has the table -- and chased out in that order.  FINAL compiles that in; the launcher leaves it out
// for one model without the table (the n-gram search): it runs once per launch, but the values it keeps alive change the register
// and SGPR-spill choices inside the frame loop, measured at 2.4 to 4.3 % of that search (profiles/ctc_beam_unify.md).
// STREAM: the resumable search.  The beams start from st.in and end in st.out (which hold the search's order and ranks), the tree
// and the outputs have Tcap frames per utterance, a node's frame is counted from the stream's first frame, and the outputs are not
// padded.  The frame loop is the one-shot search's: rows are indexed by the frame of the chunk, nodes by the frame of the stream.
#define CTC_BEAM_MAX 64
#define CTC_BEAM_ROOT_HASH 0x243F6A8885A308D3ull
// the bases of a window (tokens committed, frames consumed) are clamped to 0 .. this, so that no sum with a frame count (<= Tcap,
// itself <= 0x3fffffff) leaves the int range whatever a window holds
#define CTC_BEAM_BASE_MAX 0x3fffffff
__device__ __forceinline__ float ctc_lae(float a, float b) {
  const float m = fmaxf(a, b);
  return (m == NEGINF) ? NEGINF : m + log1pf(expf(-fabsf(a - b)));
}
__device__ __forceinline__ float ctc_beam_bonus(float beta, int len) {
  float bl = beta * (float)len;
  asm volatile("" : "+v"(bl));   // the product is rounded before it is added to anything
  return bl;
}
__device__ __forceinline__ float ctc_beam_rank(float tot, float beta, int len) { return tot + ctc_beam_bonus(beta, len); }
__device__ __forceinline__ unsigned long long ctc_beam_hash(unsigned long long h, int c) {
  h = (h ^ (unsigned long long)(c + 1)) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}
__device__ __forceinline__ int ctc_rl(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float ctc_rlf(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ int ctc_push(int v, int dst) { return __builtin_amdgcn_ds_permute(dst << 2, v); }
__device__ __forceinline__ float ctc_pushf(float v, int dst) { return __int_as_float(__builtin_amdgcn_ds_permute(dst << 2, __float_as_int(v))); }
// lane l <- lane l-1 over the whole wave (DPP wave_shr:1); lane 0 keeps its value
__device__ __forceinline__ int ctc_up1(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ float ctc_up1f(float v) { return __int_as_float(ctc_up1(__float_as_int(v))); }
// one value of T per fusion model in a kernel parameter: v[0 .. NM-1]; an empty record at NM = 0 (device code has no zero-length
// arrays)
template <class T, int NM> struct ctc_beam_per_model { T v[NM]; };
template <class T> struct ctc_beam_per_model<T, 0> {};
// (a fusion model, `ctc_beam_lm`, with `ctc_beam_alpha_lm` and `ctc_beam_lm_lookup`: ctc_beam_fusion.h)
// the models of a kernel.  The kernels with the output's final terms take room for two whatever NM (the second slot is not read at
// NM = 1): where the stream record lands in the argument block decides how its scalar loads are grouped and which SGPRs spill, and
// the resumable one-model kernel measured 0.6 to 0.9 % slower behind a one-model record (profiles/ctc_beam_unify.md)
template <int NM, bool FINAL> using ctc_beam_models = ctc_beam_per_model<ctc_beam_lm, (FINAL ? 2 : NM)>;
// candidate (r, k) goes in front of (wr, wk)
__device__ __forceinline__ bool ctc_beam_beats(float r, int k, float wr, int wk) { return r > wr || (r == wr && k < wk); }
// the loop over the models, unrolled by the preprocessor: the body once per model k < NM (<= 2), in model order, with k a constant
// expression, so that the per-model registers and records are indexed by constants from the first pass on and the code is what
// the same steps written out by hand per model compile to
#define CTC_BEAM_EACH_MODEL(NM, k, ...)                              \
  do {                                                               \
    if constexpr ((NM) > 0) { constexpr int k = 0; __VA_ARGS__ }     \
    if constexpr ((NM) > 1) { constexpr int k = 1; __VA_ARGS__ }     \
  } while (0)
// what no extension of a beam can rank above: `base` with the models' bounds added in model order, ((base + top_0) + top_1)
template <int NM>
__device__ __forceinline__ float ctc_beam_bound(float base, const float (&top)[NM > 0 ? NM : 1]) {
  CTC_BEAM_EACH_MODEL(NM, k, { base += top[k]; });
  return base;
}
// the state a resumable search starts from (in.node null: fresh streams) and the one it writes, with the frames the tree holds and
// one (state, sum) pointer pair in each per model, `model<k>()`: the first model's are where the C struct has them, lm_state and
// lm_sum of in / out, the pairs of the models behind it follow (fs_state / fs_sum of mi355x_ctc_beam_fused_state); nothing in the
// one-shot search
struct ctc_beam_model_state {
  const int* in_state; const float* in_sum;
  int* out_state; float* out_sum;
};
template <int NM, bool STREAM> struct ctc_beam_stream {};
template <int NM> struct ctc_beam_stream<NM, true> {
  mi355x_ctc_beam_stream_state in, out;
  int Tcap;
  ctc_beam_per_model<ctc_beam_model_state, (NM > 1 ? NM - 1 : 0)> more;
  template <int k> __device__ __forceinline__ ctc_beam_model_state model() const {
    if constexpr (k == 0) return {in.lm_state, in.lm_sum, out.lm_state, out.lm_sum};
    else return more.v[k - 1];
  }
};
// the window of a committed stream (mi355x_ctc_beam_window, read-only): behind the stream record, in a record of its own type, so
// that the kernels without a window keep the argument block they had
template <int NM> struct ctc_beam_stream_win : ctc_beam_stream<NM, true> {
  const int* tok_base; const int* frame_base; const int* kept; const int* frame_map;
};
template <int NM, bool STREAM, bool WIN>
using ctc_beam_stream_arg_t = std::conditional_t<WIN, ctc_beam_stream_win<NM>, ctc_beam_stream<NM, STREAM>>;
// are the prefixes of nodes a and b the same sequence (they have the same length)?  BOUND (resumable search: the ids come from a
// state and a tree the caller keeps): an id beyond `lim` is not followed
template <bool BOUND>
__device__ __forceinline__ bool ctc_beam_same_prefix(const int2* ws, int a, int b, int lim) {
  while (a != b) {
    if (a <= 0 || b <= 0) return false;
    if constexpr (BOUND)
      if (a > lim || b > lim) return false;
    const int2 ea = ws[a - 1], eb = ws[b - 1];
    if (ea.y != eb.y) return false;
    a = ea.x; b = eb.x;
  }
  return true;
}

template <int NM, bool STREAM, bool FINAL, bool WIN = false>
__global__ __launch_bounds__(64) void ctc_beam_kernel(const float* __restrict__ logp, const long long* __restrict__ lens, int2* node_ws,
                                                      int* __restrict__ tokens, int* __restrict__ tok_frame, int* __restrict__ hyp_len,
                                                      float* __restrict__ score, int* __restrict__ n_hyp, int Tmax, int C, int blank,
                                                      int W, float theta, float beta, ctc_beam_models<NM, FINAL> lm,
                                                      ctc_beam_stream_arg_t<NM, STREAM, WIN> st) {
  static_assert(NM >= 0 && NM <= 2, "at most two fusion models");
  static_assert(STREAM || !WIN, "a window is a stream's");
  static_assert(NM > 0 || !FINAL, "a final term is a model's");
  constexpr int NR = NM > 0 ? NM : 1;   // (per-model registers: an array of one that nothing touches at NM = 0)
  extern __shared__ float s_rows[];   // [2][C]: the log-probabilities of this frame and of the next
  const int b = blockIdx.x, lane = threadIdx.x;
  int T = (int)max(0ll, min((long long)Tmax, lens ? lens[b] : (long long)Tmax));
  const float* lp = logp + (long long)b * Tmax * C;
  int Tout = Tmax;   // frames per utterance of the tree and of tokens / tok_frame
  if constexpr (STREAM) Tout = st.Tcap;
  int2* ws = node_ws + (long long)b * Tout * W;
  const int G = (C + 63) >> 6;
  // the beam of this lane (lanes < nb are live, sorted by rank)
  int node = 0, par = -1, tok = -1, len = 0;
  unsigned long long h = CTC_BEAM_ROOT_HASH, hp = 0;
  float pb = lane == 0 ? 0.f : NEGINF, pnb = NEGINF, tot = pb, brank = pb;
  int nb = 1;
  int m_state[NR];    // per model: the automaton state of the prefix, <s> for the empty one, and m(prefix)
  float m_sum[NR];
  CTC_BEAM_EACH_MODEL(NM, k, { m_state[k] = 1; m_sum[k] = 0.f; });
  int f0 = 0;         // (STREAM) frames of the stream before this chunk
  if constexpr (STREAM) {
    if (st.in.node) {   // every value that becomes an address is clamped to its range: a state that is not one of this search's
      f0 = min(max(st.in.frames_done[b], 0), Tout);   // gives a wrong result, never a store outside the tree or the outputs
      nb = min(max(st.in.nb[b], 0), W);
      if (lane < nb) {
        const int s = b * W + lane;
        node = st.in.node[s]; par = st.in.par[s]; tok = min(max(st.in.tok[s], -1), C - 1);
        if constexpr (WIN) {   // len is the GLOBAL length (the rank's beta * len keeps its bits); the tree holds its tail
          const int tb = min(max(st.tok_base[b], 0), CTC_BEAM_BASE_MAX);
          len = tb + min(max(max(st.in.len[s], 0) - tb, 0), f0);
        } else {
          len = min(max(st.in.len[s], 0), f0);
        }
        h = st.in.h[s]; hp = st.in.hp[s];
        pb = st.in.pb[s]; pnb = st.in.pnb[s]; tot = st.in.tot[s]; brank = st.in.brank[s];
        CTC_BEAM_EACH_MODEL(NM, k, { m_state[k] = st.template model<k>().in_state[s]; m_sum[k] = st.template model<k>().in_sum[s]; });
      } else {   // a slot without a beam is what the frame loop leaves in one
        pb = NEGINF; tot = NEGINF; brank = NEGINF;
      }
    }
    T = min(T, Tout - f0);   // (the capacity clamp)
  }
  const int node_lim = Tout * W;   // (STREAM) the largest node id the tree can hold
  if (T > 0)
    for (int c = lane; c < C; c += 64) s_rows[c] = lp[c];
  for (int t = 0; t < T; ++t) {
    const float* row = s_rows + (t & 1) * C;
    float* nrow = s_rows + ((t + 1) & 1) * C;
    const bool more = t + 1 < T;   // (rows beyond the utterance are never read: they may hold anything)
    const float* nlp = lp + (long long)(t + 1) * C;
    float nx[4];   // the first 256 classes of the next row are requested here and stored to LDS behind the scan
#pragma unroll
    for (int k = 0; k < 4; ++k) nx[k] = (more && k * 64 + lane < C) ? nlp[k * 64 + lane] : 0.f;
    float mx = NEGINF;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, row[c]);
    mx = wave_max(mx);
    const float lo = mx - theta;
    const bool live = lane < nb;
    // ---- stays, with the extensions that land on them
    const float vb = row[blank];
    const float vl = (live && tok >= 0) ? row[tok] : NEGINF;
    const bool okl = live && tok >= 0 && vl >= lo;
    float spb = (live && vb >= lo) ? tot + vb : NEGINF;
    float spnb = okl ? pnb + vl : NEGINF;
    int pl = -1;   // the slot of the beam whose extension by `tok` is this beam
    for (int i = 0; i < nb; ++i) {
      const int hl = ctc_rl((int)(unsigned)h, i), hh = ctc_rl((int)(unsigned)(h >> 32), i), li = ctc_rl(len, i), ni = ctc_rl(node, i);
      if (live && pl < 0 && len == li + 1 && (int)(unsigned)hp == hl && (int)(unsigned)(hp >> 32) == hh &&
          ctc_beam_same_prefix<STREAM>(ws, par, ni, node_lim))
        pl = i;
    }
    {
      const int src = pl >= 0 ? pl : lane;
      const int tok_p = __shfl(tok, src, 64);
      const float pb_p = __shfl(pb, src, 64), tot_p = __shfl(tot, src, 64);
      if (pl >= 0 && okl) spnb = ctc_lae(spnb, ((tok == tok_p) ? pb_p : tot_p) + vl);
    }
    const float stot = ctc_lae(spb, spnb);
    // ---- the running top-W in lanes 0 .. W-1, in order: seeded with the stays (empty places: rank -inf and a key behind every
    // candidate's, each its own, so that the order is total); lanes beyond W carry along what is shifted out and are never read
    float e_rank = NEGINF, e_val = NEGINF;
    int e_key = 0x7fffffff - lane;
    if (live && stot != NEGINF) {
      e_rank = ctc_beam_rank(stot, beta, len); e_key = lane;
      CTC_BEAM_EACH_MODEL(NM, k, { e_rank += ctc_beam_alpha_lm(lm.v[k].alpha, m_sum[k]); });
    }
    {
      int pos = 0;
      for (int j = 0; j < W; ++j) pos += ctc_beam_beats(ctc_rlf(e_rank, j), ctc_rl(e_key, j), e_rank, e_key) ? 1 : 0;
      if (lane >= W) pos = lane;
      e_rank = ctc_pushf(e_rank, pos); e_key = ctc_push(e_key, pos);
    }
    const unsigned long long wmask = W == 64 ? ~0ull : (1ull << W) - 1ull;
    float wr = ctc_rlf(e_rank, W - 1);   // the bar: the last entry
    int wk = ctc_rl(e_key, W - 1);
    // ---- extensions, streamed.  The bar only rises, and float32 rounding is monotone, so what cannot beat the bar of the stays is
    // out for the whole frame: a beam whose best possible extension (tot_i + mx) ranks below it, and a class whose extension of the
    // best possible beam (the largest tot, the largest bonus) does -- a group of 64 classes with no other class is never read again.
    // per model, what alpha * m of an extension of this beam cannot exceed
    float m_top[NR], m_top_max[NR];
    CTC_BEAM_EACH_MODEL(NM, k, {
      m_top[k] = ctc_beam_alpha_lm(lm.v[k].alpha, m_sum[k] + lm.v[k].ub);
      m_top_max[k] = wave_max(live ? m_top[k] : NEGINF);
    });
    const unsigned long long beams = __ballot(live && !(ctc_beam_bound<NM>(ctc_beam_rank(tot + mx, beta, len + 1), m_top) < wr));
    const float tmax = wave_max(live ? tot : NEGINF), blmax = wave_max(live ? ctc_beam_bonus(beta, len + 1) : NEGINF);
    unsigned long long groups[2] = {0ull, 0ull};   // (G <= 128: the launcher's LDS rule)
    for (int g = 0; g < G; ++g) {
      const int c = g * 64 + lane;
      const float v = c < C ? row[c] : NEGINF;
      const bool in = c < C && c != blank && v >= lo && !(ctc_beam_bound<NM>((tmax + v) + blmax, m_top_max) < wr);
      if (__ballot(in)) groups[g >> 6] |= 1ull << (g & 63);
    }
    for (unsigned long long bm = beams; bm; bm &= bm - 1) {
      const int i = __ffsll((long long)bm) - 1;
      const int tok_i = ctc_rl(tok, i), len_i = ctc_rl(len, i);
      const float pb_i = ctc_rlf(pb, i), tot_i = ctc_rlf(tot, i);
      int m_state_i[NR];
      float m_sum_i[NR], m_top_i[NR];
      CTC_BEAM_EACH_MODEL(NM, k, {
        m_state_i[k] = ctc_rl(m_state[k], i); m_sum_i[k] = ctc_rlf(m_sum[k], i); m_top_i[k] = ctc_rlf(m_top[k], i);
      });
      if (ctc_beam_bound<NM>(ctc_beam_rank(tot_i + mx, beta, len_i + 1), m_top_i) < wr) continue;   // (the bar has risen)
      const unsigned long long kids = __ballot(live && pl == i);
      for (int hw = 0; hw < 2; ++hw)
      for (unsigned long long gm = groups[hw]; gm; gm &= gm - 1) {
        const int c = (hw * 64 + __ffsll((long long)gm) - 1) * 64 + lane;
        const float v = c < C ? row[c] : NEGINF;
        bool ok = c < C && c != blank && v >= lo;
        for (unsigned long long m = kids; m; m &= m - 1)
          if (c == ctc_rl(tok, __ffsll((long long)m) - 1)) ok = false;   // this extension is the stay of a beam of the set
        const float val = ((c == tok_i) ? pb_i : tot_i) + v;
        float rank = ctc_beam_rank(val, beta, len_i + 1);
        const int key = W + i * C + c;
        if constexpr (NM > 0) {   // the bounds, without a look-up, first; the lanes they leave walk the tables for their exact rank
          ok = ok && val != NEGINF && ctc_beam_beats(ctc_beam_bound<NM>(rank, m_top_i), key, wr, wk);
          if (ok) {
            int next;
            CTC_BEAM_EACH_MODEL(NM, k, {
              rank += ctc_beam_alpha_lm(lm.v[k].alpha, m_sum_i[k] + ctc_beam_lm_lookup(lm.v[k], m_state_i[k], c, next));
            });
          }
        }
        for (unsigned long long m = __ballot(ok && val != NEGINF && ctc_beam_beats(rank, key, wr, wk)); m; m &= m - 1) {
          const int l = __ffsll((long long)m) - 1;
          const float r = ctc_rlf(rank, l);
          const int k = ctc_rl(key, l);
          if (!ctc_beam_beats(r, k, wr, wk)) continue;   // (the bar has risen since the ballot)
          const float vv = ctc_rlf(val, l);
          const int at = __popcll(__ballot(ctc_beam_beats(e_rank, e_key, r, k)) & wmask);   // the entries in front of it
          const float u_rank = ctc_up1f(e_rank), u_val = ctc_up1f(e_val);
          const int u_key = ctc_up1(e_key);
          if (lane > at) { e_rank = u_rank; e_key = u_key; e_val = u_val; }
          else if (lane == at) { e_rank = r; e_key = k; e_val = vv; }
          wr = ctc_rlf(e_rank, W - 1); wk = ctc_rl(e_key, W - 1);
        }
      }
    }
    // ---- the new set: the entry of lane s is slot s; it fetches the beam it comes from and becomes the beam of its lane
    const bool keep = lane < W && e_rank != NEGINF;
    const bool is_ext = keep && e_key >= W;
    const int src = !keep ? lane : is_ext ? (e_key - W) / C : e_key;
    const int c_new = is_ext ? (e_key - W) - src * C : -1;
    const int node_s = __shfl(node, src, 64), par_s = __shfl(par, src, 64), tok_s = __shfl(tok, src, 64), len_s = __shfl(len, src, 64);
    const unsigned long long h_s = ((unsigned long long)(unsigned)__shfl((int)(unsigned)(h >> 32), src, 64) << 32) |
                                   (unsigned)__shfl((int)(unsigned)h, src, 64);
    const unsigned long long hp_s = ((unsigned long long)(unsigned)__shfl((int)(unsigned)(hp >> 32), src, 64) << 32) |
                                    (unsigned)__shfl((int)(unsigned)hp, src, 64);
    const float spb_s = __shfl(spb, src, 64), spnb_s = __shfl(spnb, src, 64), stot_s = __shfl(stot, src, 64);
    int n_m_state[NR];
    float n_m_sum[NR];
    CTC_BEAM_EACH_MODEL(NM, k, {
      n_m_state[k] = 1; n_m_sum[k] = 0.f;
      const int m_state_s = __shfl(m_state[k], src, 64);
      const float m_sum_s = __shfl(m_sum[k], src, 64);
      if (is_ext) {   // the look-up that ranked it, once more: its value and the state behind it
        int next = 0;
        n_m_sum[k] = m_sum_s + ctc_beam_lm_lookup(lm.v[k], m_state_s, c_new, next);
        n_m_state[k] = next;
      } else if (keep) {
        n_m_state[k] = m_state_s; n_m_sum[k] = m_sum_s;
      }
    });
    const int pos = lane;
    int n_node = 0, n_par = -1, n_tok = -1, n_len = 0;
    unsigned long long n_h = CTC_BEAM_ROOT_HASH, n_hp = 0;
    float n_pb = NEGINF, n_pnb = NEGINF, n_tot = NEGINF;
    if (is_ext) {
      int tg = t;   // the frame of the stream (f0 + T <= Tout: the store stays in the tree)
      if constexpr (STREAM) tg = f0 + t;
      n_node = 1 + tg * W + pos; n_par = node_s; n_tok = c_new; n_len = len_s + 1;
      n_h = ctc_beam_hash(h_s, c_new); n_hp = h_s;
      n_pnb = e_val; n_tot = e_val;
      ws[tg * W + pos] = make_int2(n_par, n_tok);
    } else if (keep) {
      n_node = node_s; n_par = par_s; n_tok = tok_s; n_len = len_s; n_h = h_s; n_hp = hp_s;
      n_pb = spb_s; n_pnb = spnb_s; n_tot = stot_s;
    }
    node = n_node; par = n_par; tok = n_tok; len = n_len; h = n_h; hp = n_hp;
    pb = n_pb; pnb = n_pnb; tot = n_tot;
    CTC_BEAM_EACH_MODEL(NM, k, { m_state[k] = n_m_state[k]; m_sum[k] = n_m_sum[k]; });
    brank = keep ? e_rank : NEGINF;
    nb = __popcll(__ballot(keep));
    // ---- the next row
    if (more) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k * 64 + lane < C) nrow[k * 64 + lane] = nx[k];
      for (int c = 256 + lane; c < C; c += 64) nrow[c] = nlp[c];
    }
    __threadfence_block();   // the node stores of this frame are visible to the lanes that chase them
    __syncthreads();
  }
  // ---- (FINAL: a model has a `state_final` table; without one what follows is the identity) the final terms and the order of the
  // output: lane l holds the hypothesis of output place l in o_*
  int o_node = node, o_len = len;
  float o_score = brank;
  if constexpr (FINAL) {
    const bool live = lane < nb;
    float sc = NEGINF;
    if (live) {
      sc = brank;
      CTC_BEAM_EACH_MODEL(NM, k, {
        if (lm.v[k].fin) sc += ctc_beam_alpha_lm(lm.v[k].alpha, lm.v[k].fin[min(max(m_state[k], 0), lm.v[k].n_states - 1)]);
      });
    }
    int pos = 0;
    for (int j = 0; j < nb; ++j) pos += ctc_beam_beats(ctc_rlf(sc, j), j, sc, lane) ? 1 : 0;
    if (!live) pos = lane;   // (the live lanes take the places 0 .. nb-1: a permutation)
    o_node = ctc_push(node, pos); o_len = ctc_push(len, pos); o_score = ctc_pushf(sc, pos);
  }
  if constexpr (STREAM) {
    // ---- the next state, out of place; then the n-best so far where it is asked for: no padding, Tcap positions per hypothesis
    if (lane < W) {
      const int s = b * W + lane;
      st.out.node[s] = node; st.out.par[s] = par; st.out.tok[s] = tok; st.out.len[s] = len;
      st.out.h[s] = h; st.out.hp[s] = hp;
      st.out.pb[s] = pb; st.out.pnb[s] = pnb; st.out.tot[s] = tot; st.out.brank[s] = brank;
      CTC_BEAM_EACH_MODEL(NM, k, { st.template model<k>().out_state[s] = m_state[k]; st.template model<k>().out_sum[s] = m_sum[k]; });
    }
    if (lane == 0) { st.out.nb[b] = nb; st.out.frames_done[b] = f0 + T; }
    if (!tokens) return;
    // (WIN) the tail only: the tokens behind the committed ones, and a tree frame's global frame through the window -- read here,
    // behind the frame loop, so that nothing of it is alive in the loop
    int w_kept = 0, w_base = 0;
    const int* w_map = nullptr;
    if constexpr (WIN) {
      if (st.in.node) o_len = min(max(o_len - min(max(st.tok_base[b], 0), CTC_BEAM_BASE_MAX), 0), Tout);
      w_kept = min(max(st.kept[b], 0), Tout); w_base = min(max(st.frame_base[b], 0), CTC_BEAM_BASE_MAX);
      w_map = st.frame_map + (long long)b * Tout;
    }
    if (lane < W) {
      const bool live = lane < nb;
      hyp_len[b * W + lane] = live ? o_len : 0;
      score[b * W + lane] = live ? o_score : NEGINF;
      if (live) {
        int* tk = tokens + ((long long)b * W + lane) * Tout;
        int* tf = tok_frame + ((long long)b * W + lane) * Tout;
        int id = o_node;
        for (int p = o_len - 1; p >= 0 && id > 0 && id <= node_lim; --p) {   // (len <= f0 + T <= Tout)
          const int2 e = ws[id - 1];
          tk[p] = e.y;
          int fr = (id - 1) / W;
          if constexpr (WIN) fr = fr < w_kept ? w_map[fr] : fr - w_kept + w_base;
          tf[p] = fr;
          id = e.x;
        }
      }
    }
    if (lane == 0) n_hyp[b] = nb;
    return;
  }
  // ---- output: the beams are in order; a lane per hypothesis chases its parents, tokens from position len-1 downward
  int* tk = tokens + (long long)b * W * Tmax;
  int* tf = tok_frame + (long long)b * W * Tmax;
  for (int j = 0; j < W; ++j) {   // padding, by the whole wave
    const int lj = j < nb ? ctc_rl(o_len, j) : 0;
    for (int p = lj + lane; p < Tmax; p += 64) { tk[(long long)j * Tmax + p] = -1; tf[(long long)j * Tmax + p] = -1; }
  }
  if (lane < W) {
    const bool live = lane < nb;
    hyp_len[b * W + lane] = live ? o_len : 0;
    score[b * W + lane] = live ? o_score : NEGINF;
    if (live) {
      int id = o_node;
      for (int p = o_len - 1; p >= 0 && id > 0; --p) {
        const int2 e = ws[id - 1];
        tk[(long long)lane * Tmax + p] = e.y;
        tf[(long long)lane * Tmax + p] = (id - 1) / W;
        id = e.x;
      }
    }
  }
  if (lane == 0) n_hyp[b] = nb;
}

extern "C" long long mi355x_ctc_beam_workspace_elems(int Tmax, int beam) {
  return (Tmax <= 0 || beam < 1 || beam > CTC_BEAM_MAX) ? 0 : 2ll * Tmax * beam;
}

// LDS rule: two rows of log-probabilities (this frame's and the next one's), 8 C bytes <= 64 KB, i.e. C <= 8192, whatever the beam
// width: the candidates of a frame are streamed against the running top-`beam` in registers and never stored.
// (Ttree: the frames the tree holds per utterance -- Tmax for the one-shot search, Tcap for the resumable one)
static bool ctc_beam_shape_ok(const void* logp, const void* lens, void* node_ws, int B, int Tmax, int C, int blank, int beam,
                              float threshold, float beta, int Ttree) {
  if (!logp || !lens || !node_ws) return false;
  if (B <= 0 || Tmax <= 0 || C <= 0 || blank < 0 || blank >= C || beam < 1 || beam > CTC_BEAM_MAX) return false;
  if (!(threshold > 0.f) || beta != beta || ((size_t)node_ws & 7)) return false;   // (NaN fails the first compare)
  if (Ttree < 1 || (long long)Ttree * beam > 0x3fffffffll) return false;   // node ids are 32-bit
  return (size_t)C * 8 <= 64 * 1024;
}
// State 0's arc index is the label, so a search with a model needs the blank as the last class: n_arcs >= C - 1 labels.
static bool ctc_beam_model_ok(const mi355x_ctc_beam_fusion& m, int C) {
  if (!m.state_arc_begin || !m.arc_tok || !m.arc_logp || !m.arc_next || !m.state_bo || !m.state_bo_next) return false;
  return m.n_states >= 2 && m.n_arcs >= C - 1 && m.alpha >= 0.f && m.ub == m.ub;   // (a NaN fails its compare)
}
// a state of the resumable search with n_models models is whole: the first model's arrays are beams.lm_*, the second's fs_*
static bool ctc_beam_state_ok(const mi355x_ctc_beam_fused_state* s, int n_models) {
  const mi355x_ctc_beam_stream_state& b = s->beams;
  return b.node && b.par && b.tok && b.len && b.h && b.hp && b.pb && b.pnb && b.tot && b.brank && b.nb && b.frames_done &&
         (n_models < 1 || (b.lm_state && b.lm_sum)) && (n_models < 2 || (s->fs_state && s->fs_sum));
}
template <int NM, bool FINAL>
static ctc_beam_models<NM, FINAL> ctc_beam_models_arg(const mi355x_ctc_beam_fusion* m) {
  ctc_beam_models<NM, FINAL> r = {};
  CTC_BEAM_EACH_MODEL(NM, k, {
    r.v[k] = {(const int*)m[k].state_arc_begin, (const int*)m[k].arc_tok, (const float*)m[k].arc_logp, (const int*)m[k].arc_next,
              (const float*)m[k].state_bo, (const int*)m[k].state_bo_next, m[k].n_states, m[k].n_arcs, m[k].alpha, m[k].ub,
              (const float*)m[k].state_final};
  });
  return r;
}
template <int NM, bool STREAM, bool WIN>
static ctc_beam_stream_arg_t<NM, STREAM, WIN> ctc_beam_stream_arg(const mi355x_ctc_beam_fused_state* in,
                                                                  const mi355x_ctc_beam_fused_state* out, int Tcap,
                                                                  const mi355x_ctc_beam_window* win) {
  ctc_beam_stream_arg_t<NM, STREAM, WIN> r = {};
  if constexpr (STREAM) {
    const mi355x_ctc_beam_fused_state fresh = {};   // (in null, or in->beams.node null: fresh streams, nothing of `in` is read)
    const mi355x_ctc_beam_fused_state& i = in && in->beams.node ? *in : fresh;
    r.in = i.beams; r.out = out->beams; r.Tcap = Tcap;
    if constexpr (NM > 1) r.more.v[0] = {i.fs_state, i.fs_sum, out->fs_state, out->fs_sum};
    if constexpr (WIN) { r.tok_base = win->tok_base; r.frame_base = win->frame_base; r.kept = win->kept; r.frame_map = win->frame_map; }
  }
  return r;
}

// Every entry of the search: 0 to 2 fusion models, and the resumable search where state_out is given (the one-shot search has no
// states, and its tree holds Tmax frames).  The resumable search takes its five outputs all or none, a whole state_out, and a
// state_in that is null, fresh (node null) or whole; with `win` (a whole window record) it is the search of a committed stream.
// The window is a template flag, not a null check at run time: the kernels of the entries without one are the code they were.
static int ctc_beam_launch(const void* logp, const void* lens, void* node_ws, void* tokens, void* tok_frame, void* hyp_len, void* score,
                           void* n_hyp, int B, int Tmax, int C, int blank, int beam, float threshold, float beta,
                           const mi355x_ctc_beam_fusion* models, int n_models, int Tcap, const mi355x_ctc_beam_fused_state* state_in,
                           const mi355x_ctc_beam_fused_state* state_out, void* stream, const mi355x_ctc_beam_window* win = nullptr) {
  mi_clear_errors();
  const bool streamed = state_out != nullptr;
  if (win && (!streamed || !win->tok_base || !win->frame_base || !win->kept || !win->frame_map)) return MI_ERR_ARG;
  const int outs = !!tokens + !!tok_frame + !!hyp_len + !!score + !!n_hyp;
  if (outs != 5 && !(streamed && outs == 0)) return MI_ERR_ARG;
  if (n_models < 0 || n_models > 2 || (n_models && (!models || blank != C - 1))) return MI_ERR_ARG;
  for (int k = 0; k < n_models; ++k)
    if (!ctc_beam_model_ok(models[k], C)) return MI_ERR_ARG;
  if (streamed) {
    if (!ctc_beam_state_ok(state_out, n_models)) return MI_ERR_ARG;
    if (state_in && state_in->beams.node && (!ctc_beam_state_ok(state_in, n_models) || state_in->beams.node == state_out->beams.node))
      return MI_ERR_ARG;
  }
  if (!ctc_beam_shape_ok(logp, lens, node_ws, B, Tmax, C, blank, beam, threshold, beta, streamed ? Tcap : Tmax)) return MI_ERR_ARG;
  // the output's final terms and re-ordering are compiled in where a model can bring a `state_final` table: with two models always,
  // with one where it has the table (an n-gram model has none, and the code's mere presence costs its search 2.4 to 4.3 %)
  const bool final = n_models == 2 || (n_models == 1 && models[0].state_final);
#define CTC_BEAM_LAUNCH_W(NM, STREAM, FINAL, WIN)                                                                                      \
  MI_LAUNCH((ctc_beam_kernel<NM, STREAM, FINAL, WIN>), dim3(B), dim3(64), (size_t)C * 8, (hipStream_t)stream, (const float*)logp,      \
            (const long long*)lens, (int2*)node_ws, (int*)tokens, (int*)tok_frame, (int*)hyp_len, (float*)score, (int*)n_hyp, Tmax, C, \
            blank, beam, threshold, beta, (ctc_beam_models_arg<NM, FINAL>(models)),                                                    \
            (ctc_beam_stream_arg<NM, STREAM, WIN>(state_in, state_out, Tcap, win)))
#define CTC_BEAM_LAUNCH(NM, STREAM, FINAL) CTC_BEAM_LAUNCH_W(NM, STREAM, FINAL, false)
  if (win) {
    switch (2 * n_models + final) {
      case 0: CTC_BEAM_LAUNCH_W(0, true, false, true); break;
      case 2: CTC_BEAM_LAUNCH_W(1, true, false, true); break;
      case 3: CTC_BEAM_LAUNCH_W(1, true, true, true); break;
      default: CTC_BEAM_LAUNCH_W(2, true, true, true); break;
    }
  } else
  switch (4 * n_models + 2 * streamed + final) {
    case 0: CTC_BEAM_LAUNCH(0, false, false); break;
    case 2: CTC_BEAM_LAUNCH(0, true, false); break;
    case 4: CTC_BEAM_LAUNCH(1, false, false); break;
    case 5: CTC_BEAM_LAUNCH(1, false, true); break;
    case 6: CTC_BEAM_LAUNCH(1, true, false); break;
    case 7: CTC_BEAM_LAUNCH(1, true, true); break;
    case 9: CTC_BEAM_LAUNCH(2, false, true); break;
    default: CTC_BEAM_LAUNCH(2, true, true); break;
  }
#undef CTC_BEAM_LAUNCH
#undef CTC_BEAM_LAUNCH_W
  return mi_check_launch();
}
// what an entry refuses before the launcher sees it: the launcher takes no model for the plain search, a null state_out for the
// one-shot one
static int ctc_beam_refused() {
  mi_clear_errors();
  return MI_ERR_ARG;
}
// a state of the entries without a second model, as the launcher takes it (null: fresh streams)
static mi355x_ctc_beam_fused_state ctc_beam_state_arg(const mi355x_ctc_beam_stream_state* s) {
  mi355x_ctc_beam_fused_state f = {};
  if (s) f.beams = *s;
  return f;
}

extern "C" int mi355x_ctc_beam_decode(const void* logp, const void* lens, void* node_ws, void* tokens, void* tok_frame, void* hyp_len,
                                      void* score, void* n_hyp, int B, int Tmax, int C, int blank, int beam, float threshold,
                                      float beta, void* stream) {
  return ctc_beam_launch(logp, lens, node_ws, tokens, tok_frame, hyp_len, score, n_hyp, B, Tmax, C, blank, beam, threshold, beta,
                         nullptr, 0, 0, nullptr, nullptr, stream);
}

// The same search with the n-gram model fused: one fusion model without a `state_final` table.
extern "C" int mi355x_ctc_beam_decode_lm(const void* logp, const void* lens, void* node_ws, void* tokens, void* tok_frame, void* hyp_len,
                                         void* score, void* n_hyp, int B, int Tmax, int C, int blank, int beam, float threshold,
                                         float beta, const void* state_arc_begin, const void* arc_tok, const void* arc_logp,
                                         const void* arc_next, const void* state_bo, const void* state_bo_next, int n_states,
                                         int n_arcs, float alpha, float lm_ub, void* stream) {
  const mi355x_ctc_beam_fusion m = {state_arc_begin, arc_tok, arc_logp, arc_next, state_bo, state_bo_next, nullptr, n_states, n_arcs,
                                    alpha, lm_ub};
  return ctc_beam_launch(logp, lens, node_ws, tokens, tok_frame, hyp_len, score, n_hyp, B, Tmax, C, blank, beam, threshold, beta, &m, 1,
                         0, nullptr, nullptr, stream);
}

// The two searches, resumable: one chunk from state_in to state_out over the tree the caller keeps (include/mi355x_asr.h).
extern "C" int mi355x_ctc_beam_decode_stream(const void* logp, const void* lens, void* node_ws, void* tokens, void* tok_frame,
                                             void* hyp_len, void* score, void* n_hyp, int B, int Tmax, int C, int blank, int beam,
                                             float threshold, float beta, int Tcap, const mi355x_ctc_beam_stream_state* state_in,
                                             const mi355x_ctc_beam_stream_state* state_out, void* stream) {
  if (!state_out) return ctc_beam_refused();
  const mi355x_ctc_beam_fused_state in = ctc_beam_state_arg(state_in), out = ctc_beam_state_arg(state_out);
  return ctc_beam_launch(logp, lens, node_ws, tokens, tok_frame, hyp_len, score, n_hyp, B, Tmax, C, blank, beam, threshold, beta,
                         nullptr, 0, Tcap, &in, &out, stream);
}

extern "C" int mi355x_ctc_beam_decode_lm_stream(const void* logp, const void* lens, void* node_ws, void* tokens, void* tok_frame,
                                                void* hyp_len, void* score, void* n_hyp, int B, int Tmax, int C, int blank, int beam,
                                                float threshold, float beta, const void* state_arc_begin, const void* arc_tok,
                                                const void* arc_logp, const void* arc_next, const void* state_bo,
                                                const void* state_bo_next, int n_states, int n_arcs, float alpha, float lm_ub,
                                                int Tcap, const mi355x_ctc_beam_stream_state* state_in,
                                                const mi355x_ctc_beam_stream_state* state_out, void* stream) {
  if (!state_out) return ctc_beam_refused();
  const mi355x_ctc_beam_fusion m = {state_arc_begin, arc_tok, arc_logp, arc_next, state_bo, state_bo_next, nullptr, n_states, n_arcs,
                                    alpha, lm_ub};
  const mi355x_ctc_beam_fused_state in = ctc_beam_state_arg(state_in), out = ctc_beam_state_arg(state_out);
  return ctc_beam_launch(logp, lens, node_ws, tokens, tok_frame, hyp_len, score, n_hyp, B, Tmax, C, blank, beam, threshold, beta, &m, 1,
                         Tcap, &in, &out, stream);
}

// The search with one or two fusion models, each an n-gram model or a boosting tree (a table set with `state_final`), and the final
// term at output (include/mi355x_asr.h).
extern "C" int mi355x_ctc_beam_decode_fused(const void* logp, const void* lens, void* node_ws, void* tokens, void* tok_frame,
                                            void* hyp_len, void* score, void* n_hyp, int B, int Tmax, int C, int blank, int beam,
                                            float threshold, float beta, const mi355x_ctc_beam_fusion* models, int n_models,
                                            void* stream) {
  if (!models || n_models < 1) return ctc_beam_refused();
  return ctc_beam_launch(logp, lens, node_ws, tokens, tok_frame, hyp_len, score, n_hyp, B, Tmax, C, blank, beam, threshold, beta,
                         models, n_models, 0, nullptr, nullptr, stream);
}

extern "C" int mi355x_ctc_beam_decode_fused_stream(const void* logp, const void* lens, void* node_ws, void* tokens, void* tok_frame,
                                                   void* hyp_len, void* score, void* n_hyp, int B, int Tmax, int C, int blank,
                                                   int beam, float threshold, float beta, const mi355x_ctc_beam_fusion* models,
                                                   int n_models, int Tcap, const mi355x_ctc_beam_fused_state* state_in,
                                                   const mi355x_ctc_beam_fused_state* state_out, void* stream) {
  if (!models || n_models < 1 || !state_out) return ctc_beam_refused();
  return ctc_beam_launch(logp, lens, node_ws, tokens, tok_frame, hyp_len, score, n_hyp, B, Tmax, C, blank, beam, threshold, beta,
                         models, n_models, Tcap, state_in, state_out, stream);
}

// The resumable search of a committed stream: 0 to 2 models, the tree and the state as mi355x_ctc_beam_commit left them, and the
// window it wrote (include/mi355x_asr.h).
extern "C" int mi355x_ctc_beam_decode_window_stream(const void* logp, const void* lens, void* node_ws, void* tokens, void* tok_frame,
                                                    void* hyp_len, void* score, void* n_hyp, int B, int Tmax, int C, int blank,
                                                    int beam, float threshold, float beta, const mi355x_ctc_beam_fusion* models,
                                                    int n_models, int Tcap, const mi355x_ctc_beam_fused_state* state_in,
                                                    const mi355x_ctc_beam_fused_state* state_out,
                                                    const mi355x_ctc_beam_window* window, void* stream) {
  if (!state_out || !window) return ctc_beam_refused();
  return ctc_beam_launch(logp, lens, node_ws, tokens, tok_frame, hyp_len, score, n_hyp, B, Tmax, C, blank, beam, threshold, beta,
                         models, n_models, Tcap, state_in, state_out, stream, window);
}

// ------------------------------------------------------------------------------------------------ committing a stream's stable prefix
// mi355x_ctc_beam_commit (include/mi355x_asr.h states it): a wave per stream, a lane per beam, integers only -- the float32 fields
// of a beam travel as their bits.  Out of place: (state, window, tree) -> (state', window', tree').  In order:
//   forced pruning   (stable_frames >= 0) a lane walks its chain down to the first node created before the cut: old(X); the beams
//                    whose old is slot 0's survive and close ranks (a ballot and a count)
//   common ancestor  every surviving lane holds a node of its chain, at first its own; while they differ the lanes above the
//                    smallest id step to their parent -- a parent's id is below its child's, so the ancestor is never stepped over
//   kept frames      the lanes walk from their node to the ancestor and flag the frames they pass in the frame table [Tcap]; a
//                    ballot scan turns the flags into new frame numbers and composes the new frame map
//   the new tree     the kept frames are filled with (0, -1), then the lanes walk once more and store their nodes with both ids
//                    renumbered (lanes that share a node store the same pair)
//   committed path   lane 0 walks from the ancestor to the root into the chain buffer [2 Tcap]; the wave turns it round
// A parent is followed only into an EARLIER frame of the frames the state says are done, so a chain has at most Tcap nodes and
// every walk ends, whatever the tree holds; frames_done, nb and kept are clamped as the search clamps them, tok_base and
// frame_base to 0 .. CTC_BEAM_BASE_MAX.
#define CTC_NEGINF_BITS ((int)0xff800000)
__device__ __forceinline__ int ctc_wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int ctc_wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
// the parent of node id (0 < id <= lim): followed only into an earlier frame, else the root
__device__ __forceinline__ int ctc_commit_parent(const int2* ws, int id, int W) {
  const int p = ws[id - 1].x;
  return (p > 0 && (p - 1) / W < (id - 1) / W) ? p : 0;
}
// the new id of node p: the ancestor is the new root, a node of a kept frame moves with its frame, anything else is the root
__device__ __forceinline__ int ctc_commit_remap(const int* ftab, int p, int A, int lim, int W) {
  if (p == A || p <= 0 || p > lim) return 0;
  const int f = ftab[(p - 1) / W];
  return f < 0 ? 0 : 1 + f * W + (p - 1) % W;
}

template <int NM>
__global__ __launch_bounds__(64) void ctc_beam_commit_kernel(mi355x_ctc_beam_fused_state in, mi355x_ctc_beam_window win,
                                                             const int2* __restrict__ tree_in, mi355x_ctc_beam_fused_state out,
                                                             mi355x_ctc_beam_window wout, int2* __restrict__ tree_out,
                                                             int* __restrict__ com_tokens, int* __restrict__ com_frames,
                                                             int* __restrict__ n_com, int* __restrict__ wsp, int W, int Tcap,
                                                             int S) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int fd = min(max(in.beams.frames_done[b], 0), Tcap);
  const int nb = min(max(in.beams.nb[b], 0), W);
  const int kept = min(max(win.kept[b], 0), fd);
  const int fbase = min(max(win.frame_base[b], 0), CTC_BEAM_BASE_MAX), tbase = min(max(win.tok_base[b], 0), CTC_BEAM_BASE_MAX);
  const int G = fbase + fd - kept;   // (0 <= G < 2^31, and S >= 0 below: no sum here overflows)
  const int lim = fd * W;   // the largest id of a node of a frame that is done
  const int2* ws = tree_in + (long long)b * Tcap * W;
  int2* wo = tree_out + (long long)b * Tcap * W;
  const int* fmap = win.frame_map + (long long)b * Tcap;
  int* fmap_o = wout.frame_map + (long long)b * Tcap;
  int* ftab = wsp + (long long)b * 3 * Tcap;   // [Tcap]: flag, then new number, of a tree frame
  int* chain = ftab + Tcap;                    // [2 Tcap]: (token, global frame) from the ancestor down to the root
#define CTC_GF(i) ((i) < kept ? fmap[(i)] : (i) - kept + fbase)
  const bool live = lane < nb;
  const int s = b * W + lane;
  int node = 0, par = -1;
  if (live) {
    node = in.beams.node[s]; par = in.beams.par[s];
    if (node <= 0 || node > lim) node = 0;
  }
  // ---- forced pruning
  bool surv = live;
  if (S >= 0) {
    const int cut = G - S;
    int id = node;
    while (id > 0 && CTC_GF((id - 1) / W) >= cut) id = ctc_commit_parent(ws, id, W);
    surv = live && id == ctc_rl(id, 0);
  }
  const unsigned long long smask = __ballot(surv);
  const int nb2 = __popcll(smask);
  const int slot = __popcll(smask & ((1ull << lane) - 1ull));
  // ---- the common ancestor
  int cur = node;
  int A = 0;
  if (nb2 > 0) {
    int mn = ctc_wave_min_i(surv ? cur : 0x7fffffff), mx = ctc_wave_max_i(surv ? cur : -1);
    for (long long it = 0; mn != mx && it <= (long long)Tcap * W; ++it) {
      if (surv && cur > mn) cur = ctc_commit_parent(ws, cur, W);
      mn = ctc_wave_min_i(surv ? cur : 0x7fffffff); mx = ctc_wave_max_i(surv ? cur : -1);
    }
    A = mn == mx ? mn : 0;
  }
  // ---- the frames that stay: those with a strict descendant of A on a survivor's chain
  for (int i = lane; i < fd; i += 64) ftab[i] = 0;
  __threadfence_block();
  __syncthreads();
  if (surv)
    for (int id = node; id > 0 && id != A; id = ctc_commit_parent(ws, id, W)) ftab[(id - 1) / W] = 1;
  __threadfence_block();
  __syncthreads();
  int kept2 = 0;
  for (int i0 = 0; i0 < fd; i0 += 64) {
    const int i = i0 + lane;
    const bool k = i < fd && ftab[i] != 0;
    const unsigned long long m = __ballot(k);
    const int idx = kept2 + __popcll(m & ((1ull << lane) - 1ull));
    if (i < fd) ftab[i] = k ? idx : -1;
    if (k) fmap_o[idx] = CTC_GF(i);
    kept2 += __popcll(m);
  }
  // ---- the new tree
  for (int j = lane; j < kept2 * W; j += 64) wo[j] = make_int2(0, -1);
  __threadfence_block();
  __syncthreads();
  if (surv)
    for (int id = node; id > 0 && id != A;) {
      const int p = ctc_commit_parent(ws, id, W);
      const int to = ctc_commit_remap(ftab, id, A, lim, W);   // (> 0: the walk above flagged its frame)
      if (to > 0) wo[to - 1] = make_int2(ctc_commit_remap(ftab, p, A, lim, W), ws[id - 1].y);
      id = p;
    }
  // ---- the committed tokens: root to A
  int n = 0;
  if (lane == 0)
    for (int id = A; id > 0 && n < Tcap; id = ctc_commit_parent(ws, id, W)) {
      chain[2 * n] = ws[id - 1].y; chain[2 * n + 1] = CTC_GF((id - 1) / W);
      ++n;
    }
  n = ctc_rl(n, 0);
  __threadfence_block();
  __syncthreads();
  for (int p = lane; p < n; p += 64) {
    com_tokens[(long long)b * Tcap + p] = chain[2 * (n - 1 - p)];
    com_frames[(long long)b * Tcap + p] = chain[2 * (n - 1 - p) + 1];
  }
#undef CTC_GF
  // ---- the beams: the survivors in their order, bit for bit, with their two ids renumbered; behind them what the search leaves
  // in an empty slot
  if (surv) {
    const int d = b * W + slot;
    out.beams.node[d] = ctc_commit_remap(ftab, node, A, lim, W);
    out.beams.par[d] = node == A ? -1 : ctc_commit_remap(ftab, par, A, lim, W);
    out.beams.tok[d] = in.beams.tok[s]; out.beams.len[d] = in.beams.len[s];
    out.beams.h[d] = in.beams.h[s]; out.beams.hp[d] = in.beams.hp[s];
    int* const fo[4] = {(int*)out.beams.pb, (int*)out.beams.pnb, (int*)out.beams.tot, (int*)out.beams.brank};
    const int* const fi[4] = {(const int*)in.beams.pb, (const int*)in.beams.pnb, (const int*)in.beams.tot, (const int*)in.beams.brank};
#pragma unroll
    for (int k = 0; k < 4; ++k) fo[k][d] = fi[k][s];
    if constexpr (NM > 0) { out.beams.lm_state[d] = in.beams.lm_state[s]; ((int*)out.beams.lm_sum)[d] = ((const int*)in.beams.lm_sum)[s]; }
    if constexpr (NM > 1) { out.fs_state[d] = in.fs_state[s]; ((int*)out.fs_sum)[d] = ((const int*)in.fs_sum)[s]; }
  }
  if (lane >= nb2 && lane < W) {
    const int d = b * W + lane;
    out.beams.node[d] = 0; out.beams.par[d] = -1; out.beams.tok[d] = -1; out.beams.len[d] = 0;
    out.beams.h[d] = CTC_BEAM_ROOT_HASH; out.beams.hp[d] = 0;
    ((int*)out.beams.pb)[d] = CTC_NEGINF_BITS; ((int*)out.beams.pnb)[d] = CTC_NEGINF_BITS;
    ((int*)out.beams.tot)[d] = CTC_NEGINF_BITS; ((int*)out.beams.brank)[d] = CTC_NEGINF_BITS;
    if constexpr (NM > 0) { out.beams.lm_state[d] = 1; ((int*)out.beams.lm_sum)[d] = 0; }
    if constexpr (NM > 1) { out.fs_state[d] = 1; ((int*)out.fs_sum)[d] = 0; }
  }
  if (lane == 0) {
    out.beams.nb[b] = nb2; out.beams.frames_done[b] = kept2;
    wout.tok_base[b] = tbase + n; wout.frame_base[b] = G; wout.kept[b] = kept2;
    n_com[b] = n;
  }
}

// i32 elements of workspace per stream: the frame table [Tcap] and the chain buffer [2 Tcap]
extern "C" long long mi355x_ctc_beam_commit_workspace_elems(int Tcap, int beam) {
  return (Tcap <= 0 || beam < 1 || beam > CTC_BEAM_MAX) ? 0 : 3ll * Tcap;
}

static bool ctc_beam_window_ok(const mi355x_ctc_beam_window* w) { return w && w->tok_base && w->frame_base && w->kept && w->frame_map; }

extern "C" int mi355x_ctc_beam_commit(const mi355x_ctc_beam_fused_state* state_in, const mi355x_ctc_beam_window* window_in,
                                      const void* tree_in, const mi355x_ctc_beam_fused_state* state_out,
                                      const mi355x_ctc_beam_window* window_out, void* tree_out, void* com_tokens, void* com_frames,
                                      void* n_com, void* workspace, int B, int beam, int Tcap, int n_models, int stable_frames,
                                      void* stream) {
  mi_clear_errors();
  if (!state_in || !state_out || !tree_in || !tree_out || !com_tokens || !com_frames || !n_com || !workspace) return MI_ERR_ARG;
  if (B <= 0 || beam < 1 || beam > CTC_BEAM_MAX || Tcap < 1 || (long long)Tcap * beam > 0x3fffffffll) return MI_ERR_ARG;
  if (n_models < 0 || n_models > 2 || !ctc_beam_state_ok(state_in, n_models) || !ctc_beam_state_ok(state_out, n_models))
    return MI_ERR_ARG;
  if (!ctc_beam_window_ok(window_in) || !ctc_beam_window_ok(window_out)) return MI_ERR_ARG;
  if (((size_t)tree_in & 7) || ((size_t)tree_out & 7)) return MI_ERR_ARG;
  // out of place: no array of the result is one of the input
  if (state_in->beams.node == state_out->beams.node || tree_in == tree_out || window_in->frame_map == window_out->frame_map ||
      window_in->kept == window_out->kept)
    return MI_ERR_ARG;
  const int S = stable_frames < 0 ? -1 : stable_frames;
#define CTC_COMMIT_LAUNCH(NM)                                                                                                          \
  MI_LAUNCH((ctc_beam_commit_kernel<NM>), dim3(B), dim3(64), 0, (hipStream_t)stream, *state_in, *window_in, (const int2*)tree_in,      \
            *state_out, *window_out, (int2*)tree_out, (int*)com_tokens, (int*)com_frames, (int*)n_com, (int*)workspace, beam, Tcap, S)
  switch (n_models) {
    case 0: CTC_COMMIT_LAUNCH(0); break;
    case 1: CTC_COMMIT_LAUNCH(1); break;
    default: CTC_COMMIT_LAUNCH(2); break;
  }
#undef CTC_COMMIT_LAUNCH
  return mi_check_launch();
}
