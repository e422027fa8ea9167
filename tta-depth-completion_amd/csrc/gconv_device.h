// What the two convolution units of the generic engines' matrix-core path share (internal): gconv_x3_s1.hip and gconv_x3_strided.hip
// include it, nothing else does (gconv_mfma.hip has the map of the files).  Declarations that other files call are in ptta_kernels.h.
#pragma once
#include "ptta_common.h"
#include "ptta_kernels.h"

#pragma GCC visibility push(hidden)          // everything declared here is internal to libptta_hip.so

// three-way split a = h + m + l (8 + 8 + 8 significant bits): h and m are the two-way split's (hi, lo); l2 is what that split drops
__device__ __forceinline__ void gsplit3(float a, float b, unsigned& hi, unsigned& lo, unsigned& l2) {
    float2_t v = {a, b};
    const bf16x2_t h = __builtin_convertvector(v, bf16x2_t);
    hi = __builtin_bit_cast(unsigned, h);
    float2_t r = {a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u)};
    const bf16x2_t m = __builtin_convertvector(r, bf16x2_t);
    lo = __builtin_bit_cast(unsigned, m);
    float2_t r2 = {r[0] - __uint_as_float(lo << 16), r[1] - __uint_as_float(lo & 0xffff0000u)};
    l2 = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, bf16x2_t));
}

// (The two kernels' `activate` / `activate_cheap` lambdas have the same text and stay where they are: as helpers here, taking p.act, they
// left the stride-1 kernels' code as it was and changed the register allocation of all 54 strided kernels, profiles/gconv_split_isa.txt.)

#define GX_TH 8                                         // rows of the stride-1 kernel's 8 x 32 output tile

#pragma GCC visibility pop
