// Forced alignment on the transducer heads: the Viterbi counterpart of the RNN-T and TDT loss lattices.  include/mi355x_asr.h
// states THE RULE (mi355x_transducer_align); these are its kernels.
//
//   align_rows_kernel     one wave per (b,t,u) row of the joint's logits (cells and row walk of transducer_rows.h, 4 rows per
//                         workgroup): R = 2 + D floats per cell -- lpb, lpl, ld[0..D) -- -inf in padded cells.  Called per
//                         sub-batch of the joint, so only one sub-batch of logits exists at a time.
//   ta_lattice_kernel     one wave per utterance, lane l owns the P = ceil(U1 / 64) consecutive columns u = l P .. l P + P - 1 and
//                         walks the anti-diagonals k = t + u.  A cell's predecessors all lie on earlier diagonals: a blank arc of
//                         duration d comes from the lane's own column d diagonals back, a label arc of duration d from the column
//                         to the left 1 + d diagonals back.  The values of the last DM + 1 diagonals (DM >= max duration) live in
//                         registers: h[s][j] for the lane's own columns, g[s] for the last column of the lane to the left -- one
//                         lane shift per diagonal brings the new value over, the columns inside a lane need none.  The ring is
//                         indexed by the DURATION, a compile-time loop 0 .. DM; which durations exist (and their index in the
//                         duration set) comes from a packed scalar argument, so nothing is indexed at run time and nothing goes
//                         to scratch.  For P <= 2 the arc weights of diagonal k + 1 are loaded before diagonal k is reduced; wider
//                         lanes load per cell.  Every cell stores one backpointer byte (0..7 blank arc of duration index i, 8..15
//                         label arc of duration index i - 8, 0xff none), diagonal-major with a pitch of 64 P bytes: a lane stores
//                         its P bytes as one access and a diagonal's stores are contiguous.
//                         Backtrace, same launch: lane 0 chases the bytes from the terminal arc back to (0, 0) through L2 -- one
//                         dependent load per arc, at most T_b + U_b of them -- and stores tok_frame / tok_dur.
// Ordinary vector stores only, no scratch (a largest duration above 4 is served up to U1 = 256: the wider instantiations did not
// fit the registers).  The device code of this translation unit is compiled to the scalar fp32 instructions
// only (the attribute below turns the packed v_pk_*_f32 forms off).
#include <hip/hip_runtime.h>
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "common.h"
#include "mi355x_asr.h"

#include "tdt.h"
#include "transducer_rows.h"

#define TA_NEG (-INFINITY)
#define TA_NONE 0xffu
#define TA_LABEL 8u   // backpointer byte: TA_LABEL + i = label arc of duration index i, i = blank arc of duration index i

// ---- rows kernel
__global__ __launch_bounds__(256) void align_rows_kernel(const float* __restrict__ acts, const long long* __restrict__ labels,
                                                         const long long* __restrict__ xlen, const long long* __restrict__ ylen,
                                                         float* __restrict__ rows_out, long long nrows, int T, int U1, int V1, int D,
                                                         int blank, long long ld) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nrows) return;
  const int lane = threadIdx.x & 63;
  const int R = 2 + D;
  const TrCell c = tr_cell(row, T, U1, xlen, ylen);
  float* o = rows_out + row * R;
  if (c.padded()) {
    if (lane < R) o[lane] = TA_NEG;
    return;
  }
  const float* x = acts + row * ld;
  const float dn = tr_neg_lse(x, tr_walk(x, V1, 1), lane);
  float zd = TA_NEG, ddn = 0.f;
  if (D > 0) {  // duration soft-max: lane i < D holds z_{V1+i}
    if (lane < D) zd = x[V1 + lane];
    const float md = wave_max(zd);
    const float sd = wave_sum(lane < D ? __expf(zd - md) : 0.f);
    ddn = -(md + logf(sd));
  }
  if (lane == 0) o[0] = x[blank] + dn;
  if (lane == 1) {
    float lpl = TA_NEG;   // the last column of the lattice has no label
    if (c.u < c.Ub - 1) {
      const long long y = labels[(long long)c.b * (U1 - 1) + c.u];
      lpl = x[min(max(y, 0LL), (long long)V1 - 1)] + dn;
    }
    o[1] = lpl;
  }
  if (lane < D) o[2 + lane] = zd + ddn;
}

// ---- lattice kernel
__host__ __device__ static inline int ta_cells(int U1) { return U1 <= 64 ? 1 : U1 <= 128 ? 2 : U1 <= 256 ? 4 : U1 <= 512 ? 8 : 16; }

// the weights of the arcs INTO one cell, by duration d: blank arc (d >= 1) lp = ba[d], duration term bc[d]; label arc la[d], lc[d].
// An arc that does not exist (duration not in the set, source outside the lattice) has lp = -inf and is never taken.
template <int DM> struct TaArcs { float ba[DM + 1], bc[DM + 1], la[DM + 1], lc[DM + 1]; };

// duration index of duration d (15: not in the set); wave-uniform
template <bool TDT> __device__ __forceinline__ unsigned ta_index(unsigned long long ipk, int d) {
  return TDT ? (unsigned)((ipk >> (4 * d)) & 15ull) : 0u;
}

// cell (t, u): `cell` = inside the lattice (or the terminal (T_b, U_b)), `labels` = label arcs may arrive (u > 0, not the terminal)
template <bool TDT, int DM>
__device__ __forceinline__ void ta_load(TaArcs<DM>& w, const float* __restrict__ rb, int t, int u, bool cell, bool labels, int U1,
                                        int R, unsigned long long ipk) {
#pragma unroll
  for (int d = 0; d <= DM; ++d) {
    w.ba[d] = TA_NEG; w.bc[d] = 0.f; w.la[d] = TA_NEG; w.lc[d] = 0.f;
    const unsigned i = ta_index<TDT>(ipk, d);
    const int ts = t - d;
    if (i != 15u && cell && ts >= 0) {
      const float* r = rb + ((long long)ts * U1 + u) * R;
      if (d >= 1) {
        w.ba[d] = r[0];
        if (TDT) w.bc[d] = r[2 + i];
      }
      if (labels && (TDT || d == 0)) {
        w.la[d] = r[1 - R];
        if (TDT) w.lc[d] = r[2 + (int)i - R];
      }
    }
  }
}

// one float32 add per arc, v + (lp + ld), and one comparison; the first maximum in the order blank arcs by ascending duration
// index, then label arcs by ascending duration index (= ascending duration).  own[s] / left[s]: the value of this column / the
// column to the left on diagonal k - 1 - s.
template <bool TDT, int DM>
__device__ __forceinline__ void ta_reduce(const TaArcs<DM>& w, const float (&own)[DM + 1], const float (&left)[DM + 1],
                                          unsigned long long ipk, float& best, unsigned& code) {
#pragma unroll
  for (int d = 1; d <= DM; ++d) {
    if (!TDT && d != 1) continue;
    const float cand = own[d - 1] + (TDT ? w.ba[d] + w.bc[d] : w.ba[d]);
    if (cand > best) { best = cand; code = ta_index<TDT>(ipk, d); }
  }
#pragma unroll
  for (int d = 0; d <= DM; ++d) {
    if (!TDT && d != 0) continue;
    const float cand = left[d] + (TDT ? w.la[d] + w.lc[d] : w.la[d]);
    if (cand > best) { best = cand; code = TA_LABEL + ta_index<TDT>(ipk, d); }
  }
}

template <int P>
__device__ __forceinline__ void ta_store_codes(unsigned char* p, const unsigned (&pk)[(P + 3) / 4]) {
  if constexpr (P == 1) *p = (unsigned char)pk[0];
  else if constexpr (P == 2) *reinterpret_cast<unsigned short*>(p) = (unsigned short)pk[0];
  else if constexpr (P == 4) *reinterpret_cast<unsigned*>(p) = pk[0];
  else if constexpr (P == 8) *reinterpret_cast<uint2*>(p) = make_uint2(pk[0], pk[1]);
  else *reinterpret_cast<uint4*>(p) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
}

// dpk: nibble i = duration d_i; ipk: nibble d = index of duration d in the set, 15 = none (TDT only)
template <bool TDT, int DM, int P>
__global__ __launch_bounds__(64) void ta_lattice_kernel(const float* __restrict__ rows, const long long* __restrict__ xlen,
                                                        const long long* __restrict__ ylen, unsigned char* bp_ws,
                                                        int* __restrict__ tok_frame, int* __restrict__ tok_dur,
                                                        float* __restrict__ score, int T, int U1, int D, unsigned dpk,
                                                        unsigned long long ipk) {
  constexpr bool PF = P <= 2;       // arc weights of the next diagonal in flight while this one is reduced
  constexpr int NW = PF ? P : 1;
  constexpr int W = 64 * P;         // bytes of one diagonal's backpointers
  const int b = blockIdx.x, lane = threadIdx.x;
  const int R = 2 + D, Umax = U1 - 1;
  const int Tb = (int)max(0LL, min((long long)T, xlen[b])), Ub = (int)max(0LL, min((long long)Umax, ylen[b]));
  const float* rb = rows + (long long)b * T * U1 * R;
  unsigned char* bp = bp_ws + (long long)b * (T + U1 - 1) * W;
  int* tf = tok_frame + (long long)b * Umax;
  int* td = tok_dur + (long long)b * Umax;
  const int u0 = lane * P;
  const int nd = Tb + Ub;           // diagonals 0 .. T_b - 1 + U_b

  float fin = TA_NEG;
  unsigned fcode = TA_NONE;
  if (Tb > 0) {
    float h[DM + 1][P], g[DM + 1];
#pragma unroll
    for (int s = 0; s <= DM; ++s) {
      g[s] = TA_NEG;
#pragma unroll
      for (int j = 0; j < P; ++j) h[s][j] = TA_NEG;
    }
    auto load = [&](TaArcs<DM>& w, int k, int j) __attribute__((always_inline)) {
      const int u = u0 + j, t = k - u;
      ta_load<TDT, DM>(w, rb, t, u, u <= Ub && t >= 0 && t < Tb, u > 0, U1, R, ipk);
    };
    TaArcs<DM> cw[NW], nw[NW];
    if (PF) {
#pragma unroll
      for (int j = 0; j < NW; ++j) load(cw[j], 0, j);
    }
    for (int k = 0; k < nd; ++k) {
      if (PF) {
#pragma unroll
        for (int j = 0; j < NW; ++j) load(nw[j], k + 1, j);
      }
      float nv[P];
      unsigned pk[(P + 3) / 4];
#pragma unroll
      for (int q = 0; q < (P + 3) / 4; ++q) pk[q] = 0u;
#pragma unroll
      for (int j = 0; j < P; ++j) {
        if (!PF) load(cw[0], k, j);
        float own[DM + 1], left[DM + 1];
#pragma unroll
        for (int s = 0; s <= DM; ++s) { own[s] = h[s][j]; left[s] = j ? h[s][j ? j - 1 : 0] : g[s]; }
        float best = (k == 0 && u0 + j == 0) ? 0.f : TA_NEG;   // v[0][0] = 0: no arc arrives there
        unsigned code = TA_NONE;
        ta_reduce<TDT, DM>(cw[PF ? j : 0], own, left, ipk, best, code);
        nv[j] = best;
        pk[j >> 2] |= code << (8 * (j & 3));
      }
      ta_store_codes<P>(bp + (long long)k * W + u0, pk);
      const float gn = __shfl_up(nv[P - 1], 1, 64);
#pragma unroll
      for (int s = DM; s >= 1; --s) {
        g[s] = g[s - 1];
#pragma unroll
        for (int j = 0; j < P; ++j) h[s][j] = h[s - 1][j];
      }
      g[0] = lane ? gn : TA_NEG;
#pragma unroll
      for (int j = 0; j < P; ++j) h[0][j] = nv[j];
      if (PF) {
#pragma unroll
        for (int j = 0; j < NW; ++j) cw[j] = nw[j];
      }
    }
    // the terminal (T_b, U_b): blank arcs only, out of column U_b's cells of the last diagonals (h[d-1] = diagonal nd - d)
#pragma unroll
    for (int j = 0; j < P; ++j) {
      if (u0 + j == Ub) {
        TaArcs<DM> w;
        ta_load<TDT, DM>(w, rb, Tb, Ub, true, false, U1, R, ipk);
        float own[DM + 1], left[DM + 1];
#pragma unroll
        for (int s = 0; s <= DM; ++s) { own[s] = h[s][j]; left[s] = TA_NEG; }
        ta_reduce<TDT, DM>(w, own, left, ipk, fin, fcode);
      }
    }
    fin = __shfl(fin, Ub / P, 64);
    fcode = __shfl(fcode, Ub / P, 64);
  } else if (Ub == 0) {
    fin = 0.f;   // T = 0 and U = 0
  }
  if (lane == 0) score[b] = fin;
  const bool feasible = fin > TA_NEG;
  for (int u = (feasible ? Ub : 0) + lane; u < Umax; u += 64) { tf[u] = -1; td[u] = -1; }
  if (!feasible || Ub == 0) return;
  __threadfence();
  __syncthreads();   // (one wave: its backpointer stores are behind this)
  if (lane != 0) return;
  const volatile unsigned char* vb = bp;
  int t = Tb, u = Ub;
  unsigned code = fcode;
  for (int n = 0; n <= nd; ++n) {   // every arc moves at least one diagonal back: at most nd + 1 arcs
    if (code == TA_NONE) break;     // (not reached on a path the walk has found; nor is a cell outside the lattice)
    const bool label = code >= TA_LABEL;
    const int d = TDT ? (int)((dpk >> (4 * (code & 7u))) & 15u) : (label ? 0 : 1);
    t -= d;                         // the arc's source cell
    if (label) --u;
    if (t < 0 || u < 0) break;
    if (label) { tf[u] = t; td[u] = d; }
    if (t == 0 && u == 0) break;
    code = vb[(long long)(t + u) * W + u];
  }
}

// ---- host side
extern "C" long long mi355x_transducer_align_workspace_bytes(int B, int T, int U1) {
  if (B < 1 || T < 1 || U1 < 1 || U1 > 1024) return -1;
  return (long long)B * (T + U1 - 1) * 64 * ta_cells(U1);
}

static inline int ta_check_lattice(int B, int T, int U1) {
  return (B < 1 || T < 1 || U1 < 1 || U1 > 1024) ? MI_ERR_ARG : MI_OK;
}

extern "C" int mi355x_transducer_align_rows(const void* acts, long long ld_acts, const void* labels, const void* act_lens,
                                            const void* label_lens, int B, int T, int U1, int V1, int D, int blank, void* rows,
                                            void* stream) {
  mi_clear_errors();
  if (!acts || (!labels && U1 > 1) || !act_lens || !label_lens || !rows) return MI_ERR_ARG;
  if (ta_check_lattice(B, T, U1) || V1 <= 1 || blank < 0 || blank >= V1) return MI_ERR_ARG;
  if (D != 0 && (D < 2 || D > TDT_MAXD)) return MI_ERR_ARG;
  if (ld_acts < V1 + D) return MI_ERR_ARG;
  const TrGeom q = tr_geom(B, T, U1);
  if ((q.rows + 3) / 4 > 0x7fffffffLL) return MI_ERR_ARG;
  MI_LAUNCH(align_rows_kernel, dim3(q.nblk), dim3(256), 0, (hipStream_t)stream, (const float*)acts, (const long long*)labels,
            (const long long*)act_lens, (const long long*)label_lens, (float*)rows, q.rows, T, U1, V1, D, blank, ld_acts);
  return mi_check_launch();
}

template <bool TDT, int DM>
static void ta_launch(int P, hipStream_t s, const float* rows, const long long* xlen, const long long* ylen, unsigned char* ws,
                      int* tok_frame, int* tok_dur, float* score, int B, int T, int U1, int D, unsigned dpk,
                      unsigned long long ipk) {
#define TA_CASE(PP)                                                                                                          \
  case PP:                                                                                                                   \
    MI_LAUNCH((ta_lattice_kernel<TDT, DM, PP>), dim3(B), dim3(64), 0, s, rows, xlen, ylen, ws, tok_frame, tok_dur, score, T, \
              U1, D, dpk, ipk);                                                                                              \
    break;
  if constexpr (DM > 4) {   // (16 columns per lane and a ring of 9 diagonals do not fit the registers: refused by the entry)
    switch (P) { TA_CASE(1) TA_CASE(2) TA_CASE(4) }
  } else {
    switch (P) { TA_CASE(1) TA_CASE(2) TA_CASE(4) TA_CASE(8) TA_CASE(16) }
  }
#undef TA_CASE
}

extern "C" int mi355x_transducer_align(const void* rows, const void* act_lens, const void* label_lens, const int* durations, int D,
                                       int B, int T, int U1, void* workspace, long long workspace_bytes, void* tok_frame,
                                       void* tok_dur, void* score, void* stream) {
  mi_clear_errors();
  if (!rows || !act_lens || !label_lens || !workspace || !tok_frame || !tok_dur || !score) return MI_ERR_ARG;
  if (ta_check_lattice(B, T, U1)) return MI_ERR_ARG;
  TdtDur dur;
  unsigned dpk = 0;
  unsigned long long ipk = ~0ull;
  if (D != 0 || durations) {   // anything but (0, NULL) must be a valid duration set
    if (tdt_durations(D, durations, &dur)) return MI_ERR_ARG;
    for (int i = 0; i < D; ++i) {
      dpk |= (unsigned)dur.d[i] << (4 * i);
      ipk = (ipk & ~(15ull << (4 * dur.d[i]))) | ((unsigned long long)i << (4 * dur.d[i]));
    }
  }
  if (((uintptr_t)workspace & 15) || workspace_bytes < mi355x_transducer_align_workspace_bytes(B, T, U1)) return MI_ERR_ARG;
  const int P = ta_cells(U1);
  if (D != 0 && dur.d[D - 1] > 4 && P > 4) return MI_ERR_ARG;   // a largest duration above 4 needs U1 <= 256
  hipStream_t s = (hipStream_t)stream;
  const float* r = (const float*)rows;
  const long long* xl = (const long long*)act_lens;
  const long long* yl = (const long long*)label_lens;
  unsigned char* ws = (unsigned char*)workspace;
  int* tf = (int*)tok_frame;
  int* td = (int*)tok_dur;
  float* sc = (float*)score;
  if (D == 0) ta_launch<false, 1>(P, s, r, xl, yl, ws, tf, td, sc, B, T, U1, 0, 0u, 0ull);
  else if (dur.d[D - 1] <= 4) ta_launch<true, 4>(P, s, r, xl, yl, ws, tf, td, sc, B, T, U1, D, dpk, ipk);
  else ta_launch<true, 8>(P, s, r, xl, yl, ws, tf, td, sc, B, T, U1, D, dpk, ipk);
  return mi_check_launch();
}
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
