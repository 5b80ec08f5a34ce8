// Big-blank set of the multi-blank transducer, shared by the loss (multiblank.hip) and the greedy search (rnnt_decode.hip).
#pragma once

#define MB_MAXNB 7   // big blanks
#define MB_MAXJUMP 8 // frames the largest one may consume

struct MbDur {
  int d[MB_MAXNB];  // d_0 < ... < d_{nb-1}, each in 2..8; entries >= nb are 0
  int nb;
};

// big_blank_durations: integers, strictly ascending, 2 <= d_i <= 8, 1 <= nb <= 7.  0 or MI_ERR_ARG.
static inline int mb_durations(int nb, const int* durations, MbDur* out) {
  if (!durations || nb < 1 || nb > MB_MAXNB) return MI_ERR_ARG;
  for (int i = 0; i < nb; ++i)
    if (durations[i] < 2 || durations[i] > MB_MAXJUMP || (i && durations[i] <= durations[i - 1])) return MI_ERR_ARG;
  for (int i = 0; i < MB_MAXNB; ++i) out->d[i] = i < nb ? durations[i] : 0;
  out->nb = nb;
  return 0;
}
