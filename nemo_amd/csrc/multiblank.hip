// Multi-blank transducer (Xu et al. 2022) loss + gradient w.r.t. the joint network's LOGITS, the softmax fused.
//
//   acts [B, T, U1, N] f32 logits, N = V + 1 + nb: labels 0 .. V-1, then the nb big blanks, the standard blank last
//   (blank = N - 1, big blank i = blank - 1 - i, consuming d_i frames, 2 <= d_0 < ... < d_{nb-1} <= 8).  lp(v) = z_v - lse(z[0:N]),
//   ONE softmax; sigma = logit under-normalisation, taken off every arc.  Arcs out of cell (t,u): label y_{u+1} to (t, u+1), the
//   standard blank to (t+1, u), big blank i to (t+d_i, u).  A path ends with a blank-like arc that lands exactly on (T_b, U_b).
//   include/mi355x_asr.h states the rule; it was written from memory of the reference (MultiblankRNNTLossNumba), parity with its
//   numbers is not claimed.
//   kernel 1  mb_row:      per (b,t,u) row (one wave, the row walk of transducer_rows.h): the denominator and the A = 2 + nb arc
//                          weights of the cell with sigma folded in, column 0 the label, 1 the blank, 2 + i big blank i -- the
//                          lattice never reads the logits
//   kernel 2  mb_lattice:  alpha (blockIdx.y = 0) and beta (= 1), one workgroup per utterance, thread = u, anti-diagonal sweep
//                          t + u.  Every label arc stays on its frame, so the ONLY cross-thread predecessor is the left neighbour's
//                          cell one diagonal back: a DPP wave shift inside a wave, one LDS slot per wave border (double-buffered:
//                          one barrier per diagonal, none at all for U1 <= 64).  Every blank-like predecessor is the thread's OWN
//                          cell 1 or d_i diagonals back: the last 8 diagonals live in registers as an unrolled shift register
//                          h[1..8].  It is walked by jump length j = 1..8 with compile-time indices; what is run-time is only
//                          the workspace column col[j] of the arc that jumps j frames (-1: no such arc), a uniform value.  No LDS
//                          ring, no register indexed at run time, no scratch.  Arc weights are fetched two diagonals ahead
//   kernel 3  mb_grad:     per row: dL/dz_v = softmax_v * occ - sum of the posteriors of the cell's arcs that carry output v, occ =
//                          the sum over all arcs of the cell, posterior = exp(alpha(src) + w + beta(dst) - ll); padded cells zero;
//                          f32 dense or the bf16 pitched operand of the joint's backward GEMMs
// The device code of this translation unit is compiled to the scalar fp32 instructions only, as csrc/stateless.hip and
// csrc/transducer_align.hip are (the attribute below turns the packed v_pk_*_f32 forms off; they round as the scalar forms do).  It
// is pushed BEFORE the runtime's header: a header function without it is not inline-compatible with a kernel that has it and
// would be called out of line (__syncthreads and __shfl_xor as real calls cost the search 1.7x per step when that was tried).
#if defined(__HIP_DEVICE_COMPILE__)   // (before the runtime's header: its inline functions take the attribute too, so they still inline)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include <hip/hip_runtime.h>
#include "common.h"
#include "mi355x_asr.h"

#include "multiblank.h"
#include "transducer_rows.h"

#define MNEG (-INFINITY)
#define MB_TERMS (MB_MAXJUMP + 1)   // the label arc and one blank-like arc per jump length 1..8

// workspace column of the blank-like arc that jumps j frames (col[1] = 1: the standard blank; col[d_i] = 2 + i; else -1)
struct MbJump { int col[MB_TERMS]; };
static inline MbJump mb_jumps(const MbDur& dur) {
  MbJump jp;
  for (int j = 0; j < MB_TERMS; ++j) jp.col[j] = -1;
  jp.col[1] = 1;
  for (int i = 0; i < dur.nb; ++i) jp.col[dur.d[i]] = 2 + i;
  return jp;
}

// log-sum-exp of the 9 terms (-inf entries allowed; all -inf -> -inf)
__device__ __forceinline__ float mb_lse(const float (&c)[MB_TERMS]) {
  float m = MNEG;
#pragma unroll
  for (int i = 0; i < MB_TERMS; ++i) m = fmaxf(m, c[i]);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MB_TERMS; ++i) s += __expf(c[i] - m);
  return m == MNEG ? MNEG : m + __logf(s);
}

// lane l <- lane l - 1 over the whole wave (DPP wave_shr:1); lane 0 takes `edge`
__device__ __forceinline__ float mb_up1(float v, float edge) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x138, 0xf, 0xf, false));
}

// ---- kernel 1: 256 threads = 4 waves = 4 rows.  Per row: denom = -lse(z[0:N]) and w[row * A + c] = lp(output of column c) - sigma
// (column 0: -inf at u = U_b, where no label is left)
__global__ __launch_bounds__(256) void mb_row_kernel(const float* __restrict__ acts, const long long* __restrict__ labels,
                                                     const long long* __restrict__ xlen, const long long* __restrict__ ylen,
                                                     float* __restrict__ denom, float* __restrict__ w, long long rows, int T, int U1,
                                                     int N, int A, int blank, float sigma, long long ld) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const TrCell c = tr_cell(row, T, U1, xlen, ylen);
  if (c.padded()) return;  // never read
  const float* x = acts + row * ld;
  const float dn = tr_neg_lse(x, tr_walk(x, N, 1), lane);
  if (lane == 0) denom[row] = dn;
  if (lane < A) {
    float v = MNEG;
    if (lane >= 1) v = dn + x[blank - (lane - 1)] - sigma;
    else if (c.u < c.Ub - 1) v = dn + x[labels[(long long)c.b * (U1 - 1) + c.u]] - sigma;
    w[row * A + lane] = v;
  }
}

// ---- kernel 2: grid (B, 2), blockDim = U1 rounded up to a wave
__global__ __launch_bounds__(1024) void mb_lattice_kernel(const float* __restrict__ w, const long long* __restrict__ xlen,
                                                          const long long* __restrict__ ylen, float* __restrict__ alphas,
                                                          float* __restrict__ betas, float* __restrict__ ll, int B, int T, int U1, int A,
                                                          MbJump jp) {
  __shared__ float border[2][16];  // [diagonal parity][wave]: the cell lane 63 of a wave computed, for lane 0 of the next wave
  const int b = blockIdx.x;
  const bool is_beta = blockIdx.y == 1;
  const int u = threadIdx.x, lane = u & 63, wave = u >> 6;
  const bool multi = blockDim.x > 64;  // (uniform)
  int col[MB_TERMS];  // (a register copy with constant indices: nothing takes the address of the by-value kernel argument)
#pragma unroll
  for (int j = 0; j < MB_TERMS; ++j) col[j] = jp.col[j];
  const int Tb = (int)min((long long)T, xlen[b]), Ub = (int)min((long long)(U1 - 1), ylen[b]) + 1;
  const long long base = (long long)b * T * U1;
  if (Tb <= 0 || Ub <= 0) {  // no frame, or a negative label length: no path
    if (u == 0) ll[(is_beta ? B : 0) + b] = MNEG;
    return;
  }
  const float* pw = w + base * A;
  float* out = (is_beta ? betas : alphas) + base;
  const int nd = Tb + Ub - 1;
  const bool active_u = u < Ub;
  const int uu = is_beta ? (Ub - 1 - u) : u;
  // arc weights of this thread's cell on diagonal g: e[0] the label arc, e[j] the blank-like arc of j frames
  //   alpha (t,u):  e[0] = w_label(t, u - 1)    e[j] = w_j(t - j, u)     (arcs INTO the cell; only cells of the utterance are read)
  //   beta  (t,u'): e[0] = w_label(t, u')       e[j] = w_j(t, u')        (arcs OUT of the cell)
  auto fetch = [&](int g, float (&e)[MB_TERMS]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < MB_TERMS; ++j) e[j] = MNEG;
    const int k = g - u;
    if (!active_u || k < 0 || k >= Tb) return;
    if (!is_beta) {
      if (uu > 0) e[0] = pw[((long long)k * U1 + uu - 1) * A];
#pragma unroll
      for (int j = 1; j < MB_TERMS; ++j)
        if (col[j] >= 0 && k - j >= 0) e[j] = pw[((long long)(k - j) * U1 + uu) * A + col[j]];
    } else {
      const float* r = pw + ((long long)(Tb - 1 - k) * U1 + uu) * A;
      e[0] = r[0];
#pragma unroll
      for (int j = 1; j < MB_TERMS; ++j)
        if (col[j] >= 0) e[j] = r[col[j]];
    }
  };
  float q0[MB_TERMS], q1[MB_TERMS];  // the weights of the next diagonal and of the one after
  fetch(0, q0);
  fetch(1, q1);
  // h[j] = the cell this thread computed j diagonals back (-inf where it had none).  Beta: the cell "one diagonal before" thread
  // 0's first one is the terminal (T_b, U_b) with beta = 0 -- a blank-like arc may land there, a label arc may not
  float h[MB_TERMS];
#pragma unroll
  for (int j = 0; j < MB_TERMS; ++j) h[j] = MNEG;
  if (is_beta && u == 0) h[1] = 0.f;
  if (multi) {
    if (u < 32) border[u >> 4][u & 15] = MNEG;
    __syncthreads();
  }
  for (int g = 0; g < nd; ++g) {
    float e[MB_TERMS];
#pragma unroll
    for (int j = 0; j < MB_TERMS; ++j) { e[j] = q0[j]; q0[j] = q1[j]; }
    fetch(g + 2, q1);
    // the left neighbour's cell of the previous diagonal: written to border[(g - 1) & 1] by the wave below
    float edge = MNEG;
    if (multi && lane == 0 && wave > 0) edge = border[(g + 1) & 1][wave - 1];
    const float left = mb_up1(h[1], edge);
    float c[MB_TERMS];
    c[0] = left + e[0];
#pragma unroll
    for (int j = 1; j < MB_TERMS; ++j) c[j] = h[j] + e[j];
    float v = mb_lse(c);
    const int k = g - u;
    const bool on = active_u && k >= 0 && k < Tb;
    if (!is_beta && g == 0) v = 0.f;  // alpha(0, 0)
    if (!on) v = MNEG;
    if (on) out[(long long)(is_beta ? Tb - 1 - k : k) * U1 + uu] = v;
#pragma unroll
    for (int j = MB_TERMS - 1; j > 1; --j) h[j] = h[j - 1];
    h[1] = v;
    if (multi) {
      if (lane == 63) border[g & 1][wave] = v;
      __syncthreads();
    }
  }
  // log-likelihoods.  forward: lse_j alpha(T_b - j, U_b) + w_j(T_b - j, U_b) over the jumps j <= T_b (thread U_b - 1's cells of
  // the last diagonals: h[j]); backward: beta(0, 0), the last cell of thread U_b - 1
  if (active_u && u == Ub - 1) {
    if (!is_beta) {
      float c[MB_TERMS];
      c[0] = MNEG;
#pragma unroll
      for (int j = 1; j < MB_TERMS; ++j) {
        c[j] = MNEG;
        if (col[j] >= 0 && Tb - j >= 0) c[j] = h[j] + pw[((long long)(Tb - j) * U1 + (Ub - 1)) * A + col[j]];
      }
      ll[b] = mb_lse(c);
    } else {
      ll[B + b] = h[1];
    }
  }
}

// ---- kernel 3: one wave per (b,t,u) row, 4 rows per workgroup.  TG = float: dense gradient rows of pitch ldg >= N; TG = bf16: the
// K-contiguous operand of the joint's backward GEMMs (ldg % 8 == 0, columns [N, ldg) zero).
template <typename TG>
__global__ __launch_bounds__(256) void mb_grad_kernel(const float* __restrict__ acts, const long long* __restrict__ labels,
                                                      const long long* __restrict__ xlen, const long long* __restrict__ ylen,
                                                      const float* __restrict__ denom, const float* __restrict__ w,
                                                      const float* __restrict__ alphas, const float* __restrict__ betas,
                                                      const float* __restrict__ ll, TG* __restrict__ grads, long long rows, int T,
                                                      int U1, int N, MbDur dur, int blank, float scale, int same_align, long long ld,
                                                      long long ldg) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const TrCell c = tr_cell(row, T, U1, xlen, ylen);
  const int b = c.b, t = c.t, u = c.u, Tb = c.Tb, Ub = c.Ub;
  const int A = 2 + dur.nb;
  TG* g = grads + row * ldg;
  const float* x = acts + row * ld;
  tr_zero_pad(g, N, ldg, lane);  // pad columns of a pitched operand row
  const TrWalk wk = tr_walk(x, N, same_align);
  if (c.padded()) {  // padded cell: zero gradient
    tr_zero_row(g, wk, lane);
    return;
  }
  const float dn = denom[row], a = alphas[row], logll = ll[b];
  const int lab = (u < Ub - 1) ? (int)labels[(long long)b * (U1 - 1) + u] : -1;
  // posterior of the arc of column `lane`: the label to (t, u + 1); a blank-like arc of f frames to (t + f, u) -- beta there, 0 at
  // the terminal (T_b, U_b), none beyond
  float post = 0.f;
  if (lane < A) {
    float bd = MNEG;
    if (lane == 0) {
      if (u < Ub - 1) bd = betas[row + 1];
    } else {
      int f = 1;
#pragma unroll
      for (int i = 0; i < MB_MAXNB; ++i) f = (lane == 2 + i) ? dur.d[i] : f;
      if (t + f < Tb) bd = betas[row + (long long)f * U1];
      else if (t + f == Tb && u == Ub - 1) bd = 0.f;
    }
    if (bd != MNEG) post = __expf((a - logll) + w[row * A + lane] + bd);
  }
  const float occ = wave_sum(post);
  float pk[MB_TERMS];  // the posteriors by column, in every lane
#pragma unroll
  for (int j = 0; j < MB_TERMS; ++j) pk[j] = __shfl(post, j, 64);
  const int first_blank = blank - (A - 2);  // outputs [first_blank, blank] are the blank-like ones: column blank - v + 1
  auto one = [&](int v, float xv) -> float {
    float gr = __expf(xv + dn) * occ;
    if (v == lab) gr -= pk[0];
    if (v >= first_blank) {
      const int col = blank - v + 1;
#pragma unroll
      for (int j = 1; j < MB_TERMS; ++j) gr -= (col == j) ? pk[j] : 0.f;
    }
    return gr * scale;
  };
  tr_map_row(g, x, wk, lane, one);
}

static int mb_ws_per_row(int nb) { return 5 + nb; }  // denom, alphas, betas; the 2 + nb arc weights
extern "C" int mi355x_multiblank_workspace_elems(int B, int T, int U1, int nb, long long* elems) {
  if (!elems || B <= 0 || T <= 0 || U1 <= 0 || nb < 1 || nb > MB_MAXNB) return MI_ERR_ARG;
  *elems = tr_ws_elems(mb_ws_per_row(nb), B, T, U1);
  return 0;
}

extern "C" int mi355x_multiblank_loss_ex(const void* acts, long long ld, const void* labels_, const void* act_lens_,
                                         const void* label_lens_, int B, int T, int U1, int N, int nb, const int* durations, int blank,
                                         float sigma, float grad_scale, void* costs_, void* grads_, int grads_dtype, long long ldg,
                                         void* workspace_, long long workspace_elems, void* stream) {
  mi_clear_errors();
  const long long* labels = (const long long*)labels_;
  const long long* act_lens = (const long long*)act_lens_;
  const long long* label_lens = (const long long*)label_lens_;
  MbDur dur;
  if (mb_durations(nb, durations, &dur)) return MI_ERR_ARG;
  if (tr_check_args(acts, ld, labels, act_lens, label_lens, B, T, U1, N, N, blank, costs_, grads_, grads_dtype, ldg, workspace_,
                    workspace_elems, mb_ws_per_row(nb)))
    return MI_ERR_ARG;
  if (blank != N - 1 || N - 1 - nb < 1) return MI_ERR_ARG;  // the blank is the last output, and there is a label
  if (!(sigma >= 0.f) || !(grad_scale == grad_scale)) return MI_ERR_ARG;
  const TrGeom q = tr_geom(B, T, U1);
  const long long rows = q.rows;
  const int A = 2 + nb;
  float* denom = (float*)workspace_;
  float* alphas = denom + rows;
  float* betas = alphas + rows;
  float* w = betas + rows;
  float* ll = w + rows * A;
  hipStream_t s = (hipStream_t)stream;
  MI_LAUNCH(mb_row_kernel, dim3(q.nblk), dim3(256), 0, s, (const float*)acts, labels, act_lens, label_lens, denom, w, rows, T, U1, N,
            A, blank, sigma, ld);
  MI_LAUNCH(mb_lattice_kernel, dim3(B, 2), dim3(q.threads), 0, s, w, act_lens, label_lens, alphas, betas, ll, B, T, U1, A,
            mb_jumps(dur));
  const int vec = tr_vector_walk(acts, ld, grads_, grads_dtype, ldg);
  auto grad = [&](auto* g) {
    MI_LAUNCH(mb_grad_kernel, dim3(q.nblk), dim3(256), 0, s, (const float*)acts, labels, act_lens, label_lens, denom, w, alphas,
              betas, ll, g, rows, T, U1, N, dur, blank, grad_scale, vec, ld, ldg);
  };
  if (grads_ && grads_dtype == MI_DT_BF16) grad((bf16_t*)grads_);
  else if (grads_) grad((float*)grads_);
  MI_LAUNCH(tr_cost_kernel, dim3((B + 63) / 64), dim3(64), 0, s, ll, (float*)costs_, B, 1.f);
  return mi_check_launch();
}

// dense form: logits and the f32 gradient in rows of N
extern "C" int mi355x_multiblank_loss(const void* acts, const void* labels, const void* act_lens, const void* label_lens, int B, int T,
                                      int U1, int N, int nb, const int* durations, int blank, float sigma, float grad_scale,
                                      void* costs, void* grads, void* workspace, long long workspace_elems, void* stream) {
  return mi355x_multiblank_loss_ex(acts, N, labels, act_lens, label_lens, B, T, U1, N, nb, durations, blank, sigma, grad_scale, costs,
                                   grads, MI_DT_F32, N, workspace, workspace_elems, stream);
}
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
