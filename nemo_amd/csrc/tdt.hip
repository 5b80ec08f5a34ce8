// Token-and-Duration Transducer (TDT, Xu et al. 2023) loss + gradient w.r.t. the joint network's LOGITS, both softmaxes fused.
//
//   acts [B, T, U1, V1 + D] f32 logits: V1 = vocabulary + blank label logits, then D duration logits for the durations
//   d_0 = 0 < d_1 < ... < d_{D-1} <= 8.  lp(v) = z_v - lse(z[0:V1]), dp(i) = z_{V1+i} - lse(z[V1:V1+D]), sigma = logit
//   under-normalisation.  Arcs out of cell (t,u): blank with duration d_i >= 1 to (t+d_i, u), weight lp(blank) + dp(i) - sigma;
//   label y_{u+1} with any duration to (t+d_i, u+1), weight lp(y_{u+1}) + dp(i) - sigma.  A path ends with a blank arc that
//   lands exactly on (T_b, U_b).
//   kernel 1  tdt_row:      per (b,t,u) row (one wave, the row walk of transducer_rows.h as in rnnt_denom): both log-softmax
//                           denominators and the 2D arc weights wb_i / wl_i with sigma folded in -- the lattice never reads the
//                           logits
//   kernel 2  tdt_lattice:  alpha (blockIdx.y = 0) and beta (= 1), one workgroup per utterance, thread = u, anti-diagonal sweep
//                           t + u.  Every predecessor lies on an earlier diagonal (a d = 0 label arc moves one diagonal on): blank
//                           predecessors are the thread's own cells d_i diagonals back, label predecessors the left neighbour's
//                           cells 1 + d_i diagonals back, both read from an LDS ring of max(d) + 2 diagonals (max(d) + 1 are read
//                           on a diagonal, one is written; a register ring indexed by the run-time durations went to scratch).
//                           One barrier per diagonal; emission terms prefetched two diagonals ahead
//   kernel 3  tdt_grad:     per row: dL/dz_v = softmax_v * occ - [v == blank] * sum(blank-arc posteriors) - [v == y_{u+1}] *
//                           sum(label-arc posteriors); dL/dz_{V1+i} = softmax^dur_i * occ - sum(posteriors of the arcs of
//                           duration i); padded cells zero; f32 dense or the bf16 pitched operand of the joint's backward GEMMs
//
// Objective of the reference's TDTLossNumba (nemo/collections/asr/parts/numba/rnnt_loss/rnnt_pytorch.py, GPUTDT in
// utils/cuda_utils/gpu_rnnt.py, compute_tdt_alphas_kernel / compute_tdt_betas_kernel / compute_tdt_grad_kernel).
#include "common.h"
#include "mi355x_asr.h"

#include "tdt.h"
#include "transducer_rows.h"

#define TNEG (-INFINITY)

// log-sum-exp of n <= 2 * TDT_MAXD terms (-inf entries allowed; all -inf -> -inf)
template <int N>
__device__ __forceinline__ float tdt_lse(const float (&c)[N]) {
  float m = TNEG;
#pragma unroll
  for (int i = 0; i < N; ++i) m = fmaxf(m, c[i]);
  if (m == TNEG) return TNEG;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) s += __expf(c[i] - m);
  return m + __logf(s);
}

// ---- kernel 1: 256 threads = 4 waves = 4 rows.  Per row: denom = -lse(label logits), ddenom = -lse(duration logits),
// wb[row * D + i] = lp(blank) + dp(i) - sigma (-inf for d_i = 0), wl[row * D + i] = lp(y_{u+1}) + dp(i) - sigma (-inf at u = U_b)
__global__ __launch_bounds__(256) void tdt_row_kernel(const float* __restrict__ acts, const long long* __restrict__ labels,
                                                      const long long* __restrict__ xlen, const long long* __restrict__ ylen,
                                                      float* __restrict__ denom, float* __restrict__ ddenom, float* __restrict__ wb,
                                                      float* __restrict__ wl, long long rows, int T, int U1, int V1, TdtDur dur,
                                                      int blank, float sigma, long long ld) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const TrCell c = tr_cell(row, T, U1, xlen, ylen);
  if (c.padded()) return;  // never read
  const int D = dur.D;
  const float* x = acts + row * ld;
  const float dn = tr_neg_lse(x, tr_walk(x, V1, 1), lane);
  // duration softmax: lane i < D holds z_{V1+i}
  const float zd = lane < D ? x[V1 + lane] : TNEG;
  const float md = wave_max(zd);
  const float sd = wave_sum(lane < D ? __expf(zd - md) : 0.f);
  const float ddn = -(md + logf(sd));
  if (lane == 0) { denom[row] = dn; ddenom[row] = ddn; }
  if (lane < D) {
    int di = 0;
#pragma unroll
    for (int j = 0; j < TDT_MAXD; ++j) di = (lane == j) ? dur.d[j] : di;
    const float dp = zd + ddn - sigma;
    wb[row * D + lane] = di >= 1 ? dn + x[blank] + dp : TNEG;
    wl[row * D + lane] = (c.u < c.Ub - 1) ? dn + x[labels[(long long)c.b * (U1 - 1) + c.u]] + dp : TNEG;
  }
}

// ---- kernel 2: grid (B, 2), blockDim = U1 rounded up to a wave.  LDS: R = max(d) + 2 rows of blockDim floats.
__global__ void tdt_lattice_kernel(const float* __restrict__ wb, const float* __restrict__ wl, const long long* __restrict__ xlen,
                                   const long long* __restrict__ ylen, float* __restrict__ alphas, float* __restrict__ betas,
                                   float* __restrict__ ll, int B, int T, int U1, TdtDur dur, int R) {
  extern __shared__ float nb[];  // [R][blockDim.x]: the cell each thread computed on the last R diagonals
  const int b = blockIdx.x;
  const bool is_beta = blockIdx.y == 1;
  const int u = threadIdx.x;
  const int D = dur.D;
  int dv[TDT_MAXD];  // (a register copy: the lambda below must not take the address of the by-value kernel argument)
#pragma unroll
  for (int i = 0; i < TDT_MAXD; ++i) dv[i] = dur.d[i];
  const int Tb = (int)min((long long)T, xlen[b]), Ub = (int)min((long long)(U1 - 1), ylen[b]) + 1;
  const long long base = (long long)b * T * U1;
  if (Tb <= 0) {
    if (u == 0) ll[(is_beta ? B : 0) + b] = TNEG;
    return;
  }
  const float* pb = wb + base * D;
  const float* pl = wl + base * D;
  float* out = (is_beta ? betas : alphas) + base;
  const int nd = Tb + Ub - 1;
  const bool active_u = u < Ub;
  const int uu = is_beta ? (Ub - 1 - u) : u;
  // emission terms of the cell of this thread on diagonal g:
  //   alpha (t,u):  eb[i] = wb_i(t - d_i, u)    el[i] = wl_i(t - d_i, u - 1)        (arcs INTO the cell)
  //   beta  (t,u'): eb[i] = wb_i(t, u')         el[i] = wl_i(t, u')                 (arcs OUT of the cell)
  auto fetch = [&](int g, float (&eb)[TDT_MAXD], float (&el)[TDT_MAXD]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < TDT_MAXD; ++i) { eb[i] = TNEG; el[i] = TNEG; }
    const int k = g - u;
    if (!active_u || k < 0 || k >= Tb) return;
    if (!is_beta) {
#pragma unroll
      for (int i = 0; i < TDT_MAXD; ++i) {
        const int ts = k - dv[i];
        if (i < D && ts >= 0) {
          const long long r = (long long)ts * U1 + uu;
          if (dv[i] >= 1) eb[i] = pb[r * D + i];
          if (uu > 0) el[i] = pl[(r - 1) * D + i];
        }
      }
    } else {
      const long long r = (long long)(Tb - 1 - k) * U1 + uu;
#pragma unroll
      for (int i = 0; i < TDT_MAXD; ++i) {
        if (i < D) { eb[i] = pb[r * D + i]; el[i] = pl[r * D + i]; }
      }
    }
  };
  // prefetch ring: (qb0, ql0) hold the terms of the next diagonal, (qb1, ql1) those of the one after
  float qb0[TDT_MAXD], ql0[TDT_MAXD], qb1[TDT_MAXD], ql1[TDT_MAXD];
  fetch(0, qb0, ql0);
  fetch(1, qb1, ql1);
  // LDS ring row (g mod R) holds every thread's cell of diagonal g (-inf where a thread has none).  Beta: the cell "one diagonal
  // before" thread 0's first cell is the terminal (T_b, U_b) with beta = 0 -- a blank arc may land there, a label arc may not
  for (int r = 0; r < R; ++r) nb[r * blockDim.x + u] = (is_beta && u == 0 && r == R - 1) ? 0.f : TNEG;
  __syncthreads();
  for (int g = 0; g < nd; ++g) {
    float eb[TDT_MAXD], el[TDT_MAXD];
#pragma unroll
    for (int i = 0; i < TDT_MAXD; ++i) { eb[i] = qb0[i]; el[i] = ql0[i]; qb0[i] = qb1[i]; ql0[i] = ql1[i]; }
    fetch(g + 2, qb1, ql1);
    const int k = g - u;
    float v = TNEG;
    if (active_u && k >= 0 && k < Tb) {
      if (!is_beta && k == 0 && u == 0) {
        v = 0.f;
      } else {
        const int slot = g % R;
        float c[2 * TDT_MAXD];
#pragma unroll
        for (int i = 0; i < TDT_MAXD; ++i) {
          c[i] = TNEG; c[TDT_MAXD + i] = TNEG;
          if (i < D) {
            const int di = dv[i];
            // blank arc: this thread's cell d_i diagonals back (d_i >= 1; eb is -inf for d_i = 0)
            if (di >= 1) {
              int s = slot - di;
              if (s < 0) s += R;
              c[i] = nb[s * blockDim.x + u] + eb[i];
            }
            // label arc: the neighbour's cell 1 + d_i diagonals back, inside the lattice (k - d_i >= 0)
            if (u > 0 && k - di >= 0) {
              int s = slot - 1 - di;
              if (s < 0) s += R;
              c[TDT_MAXD + i] = nb[s * blockDim.x + u - 1] + el[i];
            }
          }
        }
        v = tdt_lse(c);
      }
      out[(long long)(is_beta ? Tb - 1 - k : k) * U1 + uu] = v;
    }
    nb[(g % R) * blockDim.x + u] = v;
    __syncthreads();
  }
  // log-likelihoods.  forward: lse_i alpha(T_b - d_i, U_b) + wb_i(T_b - d_i, U_b) over d_i >= 1, T_b - d_i >= 0 (thread U_b - 1's
  // cells of the last diagonals, still in the ring: d_i <= max(d) < R); backward: beta(0, 0), the last cell of thread U_b - 1
  if (active_u && u == Ub - 1) {
    if (!is_beta) {
      float c[TDT_MAXD];
#pragma unroll
      for (int i = 0; i < TDT_MAXD; ++i) {
        c[i] = TNEG;
        const int di = dv[i];
        if (i < D && di >= 1 && Tb - di >= 0)
          c[i] = nb[((nd - di) % R) * blockDim.x + u] + pb[((long long)(Tb - di) * U1 + (Ub - 1)) * D + i];
      }
      ll[b] = tdt_lse(c);
    } else {
      ll[B + b] = nb[((nd - 1) % R) * blockDim.x + u];
    }
  }
}

// ---- kernel 3: one wave per (b,t,u) row, 4 rows per workgroup.  TG = float: dense gradient rows of pitch ldg >= V1 + D;
// TG = bf16: the K-contiguous operand of the joint's backward GEMMs (ldg % 8 == 0, columns [V1 + D, ldg) zero).
template <typename TG>
__global__ __launch_bounds__(256) void tdt_grad_kernel(const float* __restrict__ acts, const long long* __restrict__ labels,
                                                       const long long* __restrict__ xlen, const long long* __restrict__ ylen,
                                                       const float* __restrict__ denom, const float* __restrict__ ddenom,
                                                       const float* __restrict__ wb, const float* __restrict__ wl,
                                                       const float* __restrict__ alphas, const float* __restrict__ betas,
                                                       const float* __restrict__ ll, TG* __restrict__ grads, long long rows, int T,
                                                       int U1, int V1, TdtDur dur, int blank, float scale, int same_align,
                                                       long long ld, long long ldg) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const TrCell c = tr_cell(row, T, U1, xlen, ylen);
  const int b = c.b, t = c.t, u = c.u, Tb = c.Tb, Ub = c.Ub;
  const int D = dur.D;
  TG* g = grads + row * ldg;
  const float* x = acts + row * ld;
  tr_zero_pad(g, V1 + D, ldg, lane);  // pad columns of a pitched operand row
  const TrWalk w = tr_walk(x, V1, same_align);
  if (c.padded()) {  // padded cell: zero gradient
    tr_zero_row(g, w, lane);
    if (lane < D) st(g + V1 + lane, 0.f);
    return;
  }
  const float dn = denom[row], a = alphas[row], be = betas[row], logll = ll[b];
  const int lab = (u < Ub - 1) ? (int)labels[(long long)b * (U1 - 1) + u] : -1;
  // arc posteriors of duration lane (lane < D): blank to (t + d, u) -- beta there, 0 at the terminal (T_b, U_b), none beyond;
  // label to (t + d, u + 1), t + d < T_b
  float pbk = 0.f, plk = 0.f;
  if (lane < D) {
    int di = 0;
#pragma unroll
    for (int j = 0; j < TDT_MAXD; ++j) di = (lane == j) ? dur.d[j] : di;
    const float a_ll = a - logll;
    if (di >= 1) {
      float bd = TNEG;
      if (t + di < Tb) bd = betas[row + (long long)di * U1];
      else if (t + di == Tb && u == Ub - 1) bd = 0.f;
      if (bd != TNEG) pbk = __expf(a_ll + wb[row * D + lane] + bd);
    }
    if (u < Ub - 1 && t + di < Tb) plk = __expf(a_ll + wl[row * D + lane] + betas[row + (long long)di * U1 + 1]);
  }
  const float post_blank = wave_sum(pbk), post_label = wave_sum(plk);
  const float occ = __expf(a + be - logll);
  if (lane < D) st(g + V1 + lane, (__expf(x[V1 + lane] + ddenom[row]) * occ - (pbk + plk)) * scale);
  const float common = a + be + dn - logll;  // softmax_v * occ = exp(common + x_v)
  auto one = [&](int v, float xv) -> float {
    float gr = __expf(common + xv);
    if (v == blank) gr -= post_blank;
    if (v == lab) gr -= post_label;
    return gr * scale;
  };
  tr_map_row(g, x, w, lane, one);
}

static int tdt_ws_per_row(int D) { return 4 + 2 * D; }  // denom, ddenom, alphas, betas; wb, wl (D each)
extern "C" int mi355x_tdt_workspace_elems(int B, int T, int U1, int D, long long* elems) {
  if (!elems || B <= 0 || T <= 0 || U1 <= 0 || D < 2 || D > TDT_MAXD) return MI_ERR_ARG;
  *elems = tr_ws_elems(tdt_ws_per_row(D), B, T, U1);
  return 0;
}

extern "C" int mi355x_tdt_loss_ex(const void* acts, long long ld, const void* labels_, const void* act_lens_, const void* label_lens_,
                                  int B, int T, int U1, int V1, int D, const int* durations, int blank, float sigma, float grad_scale,
                                  void* costs_, void* grads_, int grads_dtype, long long ldg, void* workspace_,
                                  long long workspace_elems, void* stream) {
  mi_clear_errors();
  const long long* labels = (const long long*)labels_;
  const long long* act_lens = (const long long*)act_lens_;
  const long long* label_lens = (const long long*)label_lens_;
  TdtDur dur;
  if (tdt_durations(D, durations, &dur)) return MI_ERR_ARG;
  if (tr_check_args(acts, ld, labels, act_lens, label_lens, B, T, U1, V1, V1 + D, blank, costs_, grads_, grads_dtype, ldg,
                    workspace_, workspace_elems, tdt_ws_per_row(D)))
    return MI_ERR_ARG;
  if (!(sigma >= 0.f) || !(grad_scale == grad_scale)) return MI_ERR_ARG;
  const TrGeom q = tr_geom(B, T, U1);
  const long long rows = q.rows;
  float* denom = (float*)workspace_;
  float* ddenom = denom + rows;
  float* alphas = ddenom + rows;
  float* betas = alphas + rows;
  float* wb = betas + rows;
  float* wl = wb + rows * D;
  float* ll = wl + rows * D;
  hipStream_t s = (hipStream_t)stream;
  MI_LAUNCH(tdt_row_kernel, dim3(q.nblk), dim3(256), 0, s, (const float*)acts, labels, act_lens, label_lens, denom, ddenom, wb,
            wl, rows, T, U1, V1, dur, blank, sigma, ld);
  const int R = dur.d[D - 1] + 2;
  MI_LAUNCH(tdt_lattice_kernel, dim3(B, 2), dim3(q.threads), (size_t)R * q.threads * sizeof(float), s, wb, wl, act_lens,
            label_lens, alphas, betas, ll, B, T, U1, dur, R);
  const int vec = tr_vector_walk(acts, ld, grads_, grads_dtype, ldg);
  auto grad = [&](auto* g) {
    MI_LAUNCH(tdt_grad_kernel, dim3(q.nblk), dim3(256), 0, s, (const float*)acts, labels, act_lens, label_lens, denom, ddenom, wb,
              wl, alphas, betas, ll, g, rows, T, U1, V1, dur, blank, grad_scale, vec, ld, ldg);
  };
  if (grads_ && grads_dtype == MI_DT_BF16) grad((bf16_t*)grads_);
  else if (grads_) grad((float*)grads_);
  MI_LAUNCH(tr_cost_kernel, dim3((B + 63) / 64), dim3(64), 0, s, ll, (float*)costs_, B, 1.f);
  return mi_check_launch();
}
