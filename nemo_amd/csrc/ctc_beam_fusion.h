// The fusion model of the searches (ctc.hip: the CTC prefix beam search; rnnt_decode.hip: the fused greedy transducer search): the
// back-off automaton of mi355x_ctc_beam_fusion as a kernel sees it, the rounding of its weighted value and the look-up.
#pragma once
#include "common.h"

// a fusion model: the six tables of the back-off automaton, the fusion weight, the upper bound of a look-up and the nullable
// `state_final` table
struct ctc_beam_lm {
  const int* arc_begin; const int* arc_tok; const float* arc_logp; const int* arc_next; const float* bo; const int* bo_next;
  int n_states, n_arcs;
  float alpha, ub;
  const float* fin;
};
__device__ __forceinline__ float ctc_beam_alpha_lm(float alpha, float lm) {
  float al = alpha * lm;
  asm volatile("" : "+v"(al));   // rounded on its own, like beta * len
  return al;
}
// ln p(c | state s) and the state behind it: while c is not among the arcs of s, add the back-off of s and go to its suffix state
__device__ __forceinline__ float ctc_beam_lm_lookup(const ctc_beam_lm& lm, int s, int c, int& next) {
  float acc = 0.f;
  for (int n = 0; n < lm.n_states; ++n) {
    s = min(max(s, 0), lm.n_states - 1);
    if (s == 0) break;
    int lo = min(max(lm.arc_begin[s], 0), lm.n_arcs);
    const int end = min(max(lm.arc_begin[s + 1], lo), lm.n_arcs);
    int hi = end;
    for (int k = 0; k < 32 && lo < hi; ++k) {
      const int mid = (lo + hi) >> 1;
      if (lm.arc_tok[mid] < c) lo = mid + 1; else hi = mid;
    }
    if (lo < end && lm.arc_tok[lo] == c) { next = lm.arc_next[lo]; return acc + lm.arc_logp[lo]; }
    acc += lm.bo[s];
    s = lm.bo_next[s];
  }
  next = lm.arc_next[c];   // state 0: the arc index is the label (0 <= c < C-1 <= n_arcs)
  return acc + lm.arc_logp[c];
}
