// The stride-2 and transposed kernel of the generic engines' matrix-core convolution (gconv_mfma.hip has the map of the files), the rule
// that chooses its launch form and its launcher.
#include "gconv_device.h"

namespace {

// ---- stride-2 and transposed (fractionally strided) geometries: direct A loads, no LDS ----------------------------
// One wave = 32 outputs of one output row (transposed: of one x parity, so that all lanes use the same taps) x 32
// output channels.  A fragments (8 fp32 channels of one input pixel per lane) are loaded straight from global
// memory, split into bf16 hi/lo in registers and fed to three MFMAs; weight fragments (hi and lo) stream from L1/L2.
// These layers are ~5 % of the network's multiply-accumulates (ResNet stage entries, conv6, the four decoder
// transposed convolutions and their data gradients).
//   MODE 1 (S2): y[oy][ox] = sum x[2oy+ky-pad][2ox+kx-pad] w[tap]
//   MODE 2 (T2): y[oy][ox] = sum over taps with (oy+pad-ky), (ox+pad-kx) even of x[(oy+pad-ky)/2][(ox+pad-kx)/2] w[tap]
// NCO = output-channel tiles (of 32) per wave: with two, every A fragment (uncoalesced 32-B pieces of strided pixels, split to
// bf16 in registers) feeds two weight fragments
// SIX: bf16x6 for the images below p.six_B (GX3Args), the third operand planes split in registers / streamed like the other two
// AFF: the per-channel affine + residual epilogue (GX3Args::scale).  An instantiation of its own: written as a run-time switch it cost the
// K-split stride-2 forms two registers and with them their third wave per SIMD (136 + 32 -> 138 + 32, compiler's resource usage).
// AFF 2: the same with the act_first residual form, relu(relu(fmaf(..)) + res) (GX3Args::aff_act_first) -- again its own instantiation.
// No engine prefix has an act_first BatchNorm behind a strided convolution (CostDCNet's follows the stride-1 conv2): the twelve stride-2 AFF 2
// kernels are reached through ptta_op_gconv_affine only, 12 of this file's 54 kernels in compile time and code size
template <int MODE, int KS, int KSPLIT, int NCO, bool SIX = false, int AFF = 0>
__global__ __launch_bounds__(256) void gconv_x3_direct_kernel(GX3Args p, int Hin, int Win) {
    constexpr int PAD = KS / 2, KK = KS * KS;
    // stride 2: two output rows per wave, tap-outer / row-inner, so the A loads of both rows are in flight before the
    // first MFMA and the weight fragments are fetched once per two rows; transposed: one row (its active taps depend on
    // the row parity)
    constexpr int R = MODE == 1 ? 2 : 1;
    const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int Hout = p.H, Wout = p.W;
    const int Wt = MODE == 2 ? Win : Wout;
    const int nseg = (Wt + 31) >> 5, npar = MODE == 2 ? 2 : 1, nyg = (Hout + R - 1) / R;
    const long nitems = (long)p.B * nseg * npar * nyg;
    const int nch0 = (p.C0 + 31) >> 5;
    // block -> (4 consecutive items, channel tile); channel tile fastest.  KSPLIT = 4 (few pixels, many channels: the
    // 1/8 and 1/16-resolution layers): the block's four waves share ONE item and split its K loop (chunk c goes to wave
    // c mod 4), partial accumulators are summed through LDS in a fixed order -- 4x more blocks, 4x shorter latency chains
    const int ngrp = p.nnf / NCO;
    const int nfl = (int)(blockIdx.x % ngrp) * NCO;
    const long item = KSPLIT == 4 ? (long)(blockIdx.x / ngrp) : (long)(blockIdx.x / ngrp) * 4 + wave;
    if (item >= nitems) return;
    const int nf = p.nf0 + nfl;
    long t_ = item;
    const int yg = (int)(t_ % nyg); t_ /= nyg;
    int xpar = 0;
    if (MODE == 2) { xpar = (int)(t_ & 1); t_ >>= 1; }
    const int seg = (int)(t_ % nseg);
    const int b = (int)(t_ / nseg);
    const int x0 = seg << 5, ybase = yg * R;
    const bool lane_in = (x0 + i) < Wt;
    const bool six = SIX && b < p.six_B;                 // wave-uniform
    const bool x1 = b >= p.x1_from_B;                    // wave-uniform: single-MFMA class
    f32x16 acc[NCO][R];
#pragma unroll
    for (int t = 0; t < NCO; ++t)
#pragma unroll
    for (int rr = 0; rr < R; ++rr)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][rr][r] = 0.f;
    for (int c = KSPLIT == 4 ? wave : 0; c < p.nchunks; c += KSPLIT == 4 ? 4 : 1) {
        const bool s1 = c >= nch0;
        const float* src = s1 ? p.x1 : p.x0;
        const int ld = s1 ? p.ld1 : p.ld0, Cs = s1 ? p.C1 : p.C0, cb = (s1 ? c - nch0 : c) << 5;
        const float* inb = src + (size_t)b * Hin * Win * ld + cb + 8 * h;
        const uint4* ph = p.whi + ((size_t)nf * p.nchunks + c) * (KK * 2 * 64) + lane;
        const uint4* pl = p.wlo + ((size_t)nf * p.nchunks + c) * (KK * 2 * 64) + lane;
        const uint4* p2 = SIX ? p.wl2 + ((size_t)nf * p.nchunks + c) * (KK * 2 * 64) + lane : nullptr;
        const size_t tstride = (size_t)p.nchunks * (KK * 2 * 64);                 // next output-channel tile
#pragma unroll
        for (int tap = 0; tap < KK; ++tap) {
            const int ky = tap / KS, kx = tap % KS;
            if (MODE == 2) {
                const int ty = ybase + PAD - ky, tx = xpar + PAD - kx;
                const int yi = ty >> 1;
                if ((ty & 1) || (tx & 1) || yi < 0 || yi >= Hin) continue;          // wave-uniform: 5 to 8 of 9 taps are inactive by parity
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                bf16x8 bh[NCO], bl[NCO], b2[NCO];
#pragma unroll
                for (int t = 0; t < NCO; ++t) {
                    bh[t] = __builtin_bit_cast(bf16x8, ph[t * tstride + (tap * 2 + k) * 64]);
                    bl[t] = __builtin_bit_cast(bf16x8, pl[t * tstride + (tap * 2 + k) * 64]);
                    if constexpr (SIX) b2[t] = __builtin_bit_cast(bf16x8, p2[t * tstride + (tap * 2 + k) * 64]);
                }
                bf16x8 ah[R], al[R], a2[R];
#pragma unroll
                for (int rr = 0; rr < R; ++rr) {
                    const int y = ybase + rr;
                    int yi, xi;
                    if (MODE == 1) { yi = 2 * y + ky - PAD; xi = 2 * (x0 + i) + kx - PAD; }
                    else { yi = (y + PAD - ky) >> 1; xi = x0 + i + ((xpar + PAD - kx) >> 1); }
                    // out-of-range rows / columns / channels are folded into the load predicate (zero operands): branch-free
                    const bool ok = lane_in && y < Hout && xi >= 0 && xi < Win && yi >= 0 && yi < Hin && cb + 16 * k + 8 * h < Cs;
                    // unconditional loads from a clamped (always valid) address + select: no exec-masked branch per load, so
                    // the loads of all taps can be in flight together
                    const float* q = ok ? inb + ((size_t)yi * Win + xi) * ld + 16 * k : src;
                    float4 a0 = *(const float4*)q, a1 = *(const float4*)(q + 4);
                    if (!ok) { a0 = make_float4(0.f, 0.f, 0.f, 0.f); a1 = a0; }
                    uint4 hi, lo;
                    if constexpr (SIX) {
                        uint4 l2;
                        gsplit3(a0.x, a0.y, hi.x, lo.x, l2.x); gsplit3(a0.z, a0.w, hi.y, lo.y, l2.y);
                        gsplit3(a1.x, a1.y, hi.z, lo.z, l2.z); gsplit3(a1.z, a1.w, hi.w, lo.w, l2.w);
                        a2[rr] = __builtin_bit_cast(bf16x8, l2);
                    } else {
                        split2(a0.x, a0.y, hi.x, lo.x); split2(a0.z, a0.w, hi.y, lo.y);
                        split2(a1.x, a1.y, hi.z, lo.z); split2(a1.z, a1.w, hi.w, lo.w);
                    }
                    ah[rr] = __builtin_bit_cast(bf16x8, hi); al[rr] = __builtin_bit_cast(bf16x8, lo);
                }
                if constexpr (SIX) if (six) {
#pragma unroll
                    for (int rr = 0; rr < R; ++rr)
#pragma unroll
                        for (int t = 0; t < NCO; ++t) {
                            acc[t][rr] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2[rr], bh[t], acc[t][rr], 0, 0, 0);
                            acc[t][rr] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[rr], b2[t], acc[t][rr], 0, 0, 0);
                            acc[t][rr] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[rr], bl[t], acc[t][rr], 0, 0, 0);
                        }
                }
#pragma unroll
                for (int rr = 0; rr < R; ++rr)
#pragma unroll
                    for (int t = 0; t < NCO; ++t) {
                        if (!x1) acc[t][rr] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[rr], bh[t], acc[t][rr], 0, 0, 0);
                        if (!x1 || p.x1_w2) acc[t][rr] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[rr], bl[t], acc[t][rr], 0, 0, 0);
                        acc[t][rr] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[rr], bh[t], acc[t][rr], 0, 0, 0);
                    }
            }
        }
    }
    if constexpr (KSPLIT == 4) {
        __shared__ float red[3][NCO][R][16][64];
        if (wave) {
#pragma unroll
            for (int t = 0; t < NCO; ++t)
#pragma unroll
            for (int rr = 0; rr < R; ++rr)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[wave - 1][t][rr][r][lane] = acc[t][rr][r];
        }
        __syncthreads();
        if (wave) return;
#pragma unroll
        for (int t = 0; t < NCO; ++t)
#pragma unroll
        for (int rr = 0; rr < R; ++rr)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][rr][r] = (acc[t][rr][r] + red[0][t][rr][r][lane]) + (red[1][t][rr][r][lane] + red[2][t][rr][r][lane]);
    }
    auto activate = [&](float v) {
        if (p.act == GACT_RELU) v = v > 0.f ? v : 0.f;
        else if (p.act == GACT_LRELU) v = v > 0.f ? v : 0.2f * v;
        else if (p.act == GACT_SIGMOID) v = 1.f / (1.f + expf(-v));
        return v;
    };
    auto activate_cheap = [&](float v) {                 // selects only; the sigmoid takes the scalar path below
        const float neg = p.act == GACT_LRELU ? 0.2f * v : (p.act == GACT_RELU ? 0.f : v);
        return v > 0.f ? v : neg;
    };
    const float* const ares = AFF ? p.res : nullptr;
    const bool wide = p.act != GACT_SIGMOID && !(p.ldy & 3) && !(p.Cy & 3) && !(((size_t)p.y) & 15) &&
                      !(ares && ((p.ld_res & 3) || (((size_t)ares) & 15)));
#pragma unroll
    for (int t = 0; t < NCO; ++t) {
    const int co = (nf + t) * 32 + i - p.nf0 * 32;
    const float bias = (p.bias && co < p.Cy) ? p.bias[co] : 0.f;
    if (wide) {
        // 16 B per lane in the quad-transposed layout (ptta_common.h quad_transpose): a quarter of the store instructions
        const int c4 = (nf + t) * 32 - p.nf0 * 32 + 4 * (i >> 2);
#pragma unroll
        for (int rr = 0; rr < R; ++rr) {
            const int y = ybase + rr;
            if (y >= Hout) break;
            f32x16 tt;
#pragma unroll
            for (int r = 0; r < 16; ++r) tt[r] = acc[t][rr][r] + bias;
            if constexpr (AFF) {                          // the eval affine of this lane's channel (GX3Args::scale), loaded where it is used
                const float asc = co < p.Cy ? p.scale[co] : 1.f, ash = co < p.Cy ? p.shift[co] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) tt[r] = fmaf(tt[r], asc, ash);
                if constexpr (AFF == 2) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) tt[r] = tt[r] > 0.f ? tt[r] : 0.f;
                }
            }
            quad_transpose(tt, lane);
            float* yrow = p.y + ((size_t)b * Hout + y) * Wout * p.ldy + c4;
            bool ok[4]; size_t xo[4]; float4 old[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int xl = x0 + (i & 3) + 8 * g + 4 * h;
                const int x = MODE == 2 ? 2 * xl + xpar : xl;
                ok[g] = c4 < p.Cy && xl < Wt && x < Wout;
                xo[g] = (size_t)(ok[g] ? x : 0) * p.ldy;
                if constexpr (AFF) {                      // the residual behind the affine, added before the activation like an old output
                    if (ares) old[g] = ok[g] ? *(const float4*)(ares + (((size_t)b * Hout + y) * Wout + x) * p.ld_res + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
            if (!AFF && p.accumulate) {                   // (the affine form never accumulates: ptta_gx3_affine_ok)
#pragma unroll
                for (int g = 0; g < 4; ++g) old[g] = ok[g] ? *(const float4*)(yrow + xo[g]) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float4 v = make_float4(tt[4 * g], tt[4 * g + 1], tt[4 * g + 2], tt[4 * g + 3]);
                if (AFF ? ares != nullptr : p.accumulate != 0) { v.x += old[g].x; v.y += old[g].y; v.z += old[g].z; v.w += old[g].w; }
                v.x = activate_cheap(v.x); v.y = activate_cheap(v.y); v.z = activate_cheap(v.z); v.w = activate_cheap(v.w);
                if (ok[g]) *(float4*)(yrow + xo[g]) = v;
            }
        }
        continue;
    }
    if (co >= p.Cy) continue;
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
        const int y = ybase + rr;
        if (y >= Hout) break;
        float* yrow = p.y + ((size_t)b * Hout + y) * Wout * p.ldy + co;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int xl = x0 + acc_row(r, h);
            if (xl >= Wt) continue;
            const int x = MODE == 2 ? 2 * xl + xpar : xl;
            if (MODE == 2 && x >= Wout) continue;         // odd output width: the gradient of a stride-2 conv over an odd-sized map
            float* dst = yrow + (size_t)x * p.ldy;
            float v = acc[t][rr][r] + bias;
            if constexpr (AFF) v = fmaf(v, p.scale[co], p.shift[co]);
            if constexpr (AFF == 2) v = v > 0.f ? v : 0.f;
            if (!AFF && p.accumulate) v += *dst;
            if (ares) v += ares[(((size_t)b * Hout + y) * Wout + x) * p.ld_res + co];
            *dst = activate(v);
        }
    }
    }
}

}  // namespace

// The launch form of the strided / transposed kernel, from the sizes alone (the launcher below and ptta_op_gconv's form_host both call
// this).  GX3_FORM_KSPLIT: few pixels and a long K loop (the 1/8 and 1/16-resolution layers): one item per block, K split over its
// waves, one channel tile per wave; otherwise GX3_FORM_NCO2, two channel tiles per wave, where the tile count and the kernel allow it,
// or GX3_FORM_PLAIN, one.  (measured on the NLSPN step, same box: one tile 24.83 ms, two 24.36, four 24.47)
int ptta_gconv_x3_strided_form(const GX3Args& a, int ks, int mode, int win, long* nitems_out) {
    const int Wt = mode == 2 ? win : a.W;
    const long nitems = (long)a.B * ((Wt + 31) / 32) * (mode == 2 ? 2 : 1) * (mode == 1 ? (a.H + 1) / 2 : a.H);   // stride 2: two rows per wave
    if (nitems_out) *nitems_out = nitems;
    if (a.nchunks >= 4 && ((nitems + 3) / 4) * a.nnf < 1536) return GX3_FORM_KSPLIT;
    return (ks != 3 || (a.nnf & 1)) ? GX3_FORM_PLAIN : GX3_FORM_NCO2;
}

namespace {

typedef void (*GX3DirectKernel)(GX3Args, int, int);

template <int MODE, int KS, bool SIX, int AFF>
GX3DirectKernel direct_of(int form) {
    if (form == GX3_FORM_NCO2) return gconv_x3_direct_kernel<MODE, KS, 1, 2, SIX, AFF>;
    if (form == GX3_FORM_KSPLIT) return gconv_x3_direct_kernel<MODE, KS, 4, 1, SIX, AFF>;
    return gconv_x3_direct_kernel<MODE, KS, 1, 1, SIX, AFF>;
}

// The instantiation table.  aff: 0 the plain epilogue, 1 the affine epilogue, 2 its act_first form.  bf16x3 with the plain affine in both
// geometries (the eval forward of NLSPN's meta-only mode); bf16x6 images and the act_first form on the stride-2 convolution only (the
// stage-2 prefixes hold no transposed layer): null for the transposed geometry
template <int MODE, int KS>
GX3DirectKernel direct_kernel_of(bool six, int aff, int form) {
    if (aff == 0) return six ? direct_of<MODE, KS, true, 0>(form) : direct_of<MODE, KS, false, 0>(form);
    if (aff == 1 && !six) return direct_of<MODE, KS, false, 1>(form);
    if constexpr (MODE == 1) {
        if (aff == 1) return direct_of<1, KS, true, 1>(form);
        return six ? direct_of<1, KS, true, 2>(form) : direct_of<1, KS, false, 2>(form);
    }
    return nullptr;
}

}  // namespace

// mode 1: stride-2 convolution (a.H/a.W = output size, input = hin x win); mode 2: stride-2 transposed convolution
int ptta_launch_gconv_x3_strided(const GX3Args& a, int ks, int mode, int hin, int win, hipStream_t s) {
    if ((a.C0 & 15) || (a.C1 & 15) || (a.ld0 & 3) || (a.ld1 & 3) || (ks != 1 && ks != 3) || (mode != 1 && mode != 2)) return -22;
    if (a.nchunks != (a.C0 + 31) / 32 + (a.C1 + 31) / 32 || !ptta_gx3_affine_ok(a)) return -22;
    if (a.act == GACT_ELU) return -22;     // the ELU epilogue is the stride-1 kernel's (no strided convolution of an engine has one behind it)
    long nitems = 0;
    const int form = ptta_gconv_x3_strided_form(a, ks, mode, win, &nitems);
    const int ngrp = a.nnf / (form == GX3_FORM_NCO2 ? 2 : 1);
    const long blocks = (form == GX3_FORM_KSPLIT ? nitems : (nitems + 3) / 4) * ngrp;
    if (blocks < 1 || blocks > 0x7fffffffL) return -22;
    if (a.six_B > 0 && !a.wl2) return -22;
    const bool six = a.six_B > 0;
    const int aff = !a.scale ? 0 : (a.aff_act_first ? 2 : 1);
    const GX3DirectKernel kernel = mode == 1 ? (ks == 3 ? direct_kernel_of<1, 3>(six, aff, form) : direct_kernel_of<1, 1>(six, aff, form))
                                             : (ks == 3 ? direct_kernel_of<2, 3>(six, aff, form) : direct_kernel_of<2, 1>(six, aff, form));
    if (!kernel) return -22;               // (mode 2 with bf16x6 images or act_first behind the affine)
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, hin, win);
    PTTA_CHECK_LAUNCH();
    return 0;
}
