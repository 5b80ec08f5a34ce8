// The multi-blank instantiations of the greedy search's kernel template (rnnt_decode.hip, MODE = RD_MB) and their launcher, in a
// translation unit of their own so that their device code is compiled to the scalar fp32 instructions only (the attribute below
// turns the packed v_pk_*_f32 forms off, as in csrc/stateless.hip) while the 40 RNN-T / TDT instantiations stay the code they
// have always been.  The attribute is pushed BEFORE the runtime's header, so that the header's inline functions (__syncthreads,
// __shfl_xor, ...) carry it too and still inline; pushed behind it they became real calls and a search step took 1.7x the time.
#if defined(__HIP_DEVICE_COMPILE__)   // (before the runtime's header: its inline functions take the attribute too, so they still inline)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include <hip/hip_runtime.h>
#define RD_MULTIBLANK_TU
#include "rnnt_decode.hip"
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
