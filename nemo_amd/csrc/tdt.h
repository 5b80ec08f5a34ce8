// Duration set of the Token-and-Duration Transducer, shared by the loss (tdt.hip) and the greedy search (rnnt_decode.hip).
#pragma once

#define TDT_MAXD 8

struct TdtDur {
  int d[TDT_MAXD];  // durations d_0 < ... < d_{D-1}; entries >= D are 0
  int D;
};

// durations: integers, strictly ascending, d_0 = 0, d_{D-1} <= 8, D <= 8, at least one non-zero entry.  0 or MI_ERR_ARG.
static inline int tdt_durations(int D, const int* durations, TdtDur* out) {
  if (!durations || D < 2 || D > TDT_MAXD || durations[0] != 0 || durations[D - 1] > TDT_MAXD) return MI_ERR_ARG;
  for (int i = 1; i < D; ++i)
    if (durations[i] <= durations[i - 1]) return MI_ERR_ARG;
  for (int i = 0; i < TDT_MAXD; ++i) out->d[i] = i < D ? durations[i] : 0;
  out->D = D;
  return 0;
}
