// The stride-1 3x3 / 1x1 kernel of the generic engines' matrix-core convolution (gconv_mfma.hip has the map of the files) and its launcher.
//
// Block = 256 threads = 4 waves, output tile 8 rows x 32 pixels x 32 output channels (one MFMA column fragment).
// K loop over 16-channel sub-chunks of the source(s): the (8+2)x(32+2) halo of the sub-chunk is split into bf16 hi/lo
// while it is staged into LDS ([pixel][hi 32 B | lo 32 B | pad 16 B]: conflict-free ds_read_b128) and ALL weight
// fragments of the sub-chunk (hi and lo, 18 KB for 3x3, pre-split in global memory) are staged cooperatively next to
// it -- 45 KB of LDS and ~160 VGPRs, three blocks per CU.  Each wave owns two rows of the tile: 2 x f32x16
// accumulators live across the whole K loop; the next sub-chunk's halo and weights are loaded into registers before
// the current sub-chunk's MFMAs.  Output channel tiles of the same pixel tile are adjacent in the grid (L2 reuse).
// (Measured alternatives, all slower: hi fragments in registers per wave -- 2.5x the weight traffic through L1, the
// bottleneck by ablation; 64-channel output tiles -- re-measured in round 2 as a template variant with two accumulator sets
// per wave (8 instead of 12 ds_read_b128 per 12 MFMAs, halo staged once per 64 channels): 256 VGPRs, 64 KB of LDS, two
// blocks per CU instead of three and the NLSPN step went 26.87 -> 28.35 ms on one box, i.e. the kernel is bound by how many
// blocks overlap each other's stage -> barrier -> MFMA phases, not by LDS read bandwidth; double-buffered LDS with hi
// fragments in registers.  The ISA of THIS form drains its own register prefetch: the last weight load is conditional and the
// compiler merges its result right behind it (s_waitcnt vmcnt(0) + v_mov in front of the barrier).  A version with two explicit
// register sets and unconditional loads keeps 11 loads in flight across the MFMAs, needs 234 VGPRs (two blocks per CU) and
// measures the same: 25.73 vs 25.66 ms per NLSPN step, A/B on one box -- three non-overlapping blocks hide as much as two
// overlapping ones, and neither is bound by the loads.)
#include "gconv_device.h"

namespace {

#define GX_STR16 80                                      // LDS bytes per pixel: hi 32 | lo 32 | pad 16
// VERT: only the middle column of the 3x3 window (a 3x1x1 Conv3d viewed as a vertical 3-tap convolution over [D][H*W] images,
// gnet.h Op::rH/rW): three taps, no horizontal halo -- a third of the MFMAs of the zero-padded 3x3 form it replaces.
// TIMING: s_memtime stamps around the phases of one block's K loop, printed by two blocks of the launch (diagnostic builds of the
// launcher are compiled with -DPTTA_DIAG_STAMPS; the shipped instantiation has no stamps)
// SIX: three operand planes (GX3Args::six_B): 112 B of LDS per pixel, three weight planes, two blocks per CU; blocks of images
// >= six_B (the proxy frames) skip the three extra products
// ACTF: the affine epilogue's act_first form, relu(relu(fmaf(..)) + res) (GX3Args::aff_act_first): the inner ReLU in the register layout,
// an instantiation of its own so that the others keep their code
// ELU: the affine epilogue's ELU, v > 0 ? v : expm1f(v) behind the fmaf (gbn.hip gbn_act: CostDCNet's BatchNorm3d + ELU from constant statistics).
// Its own instantiations for the reason `activate_cheap` states below: a run-time expm1f would be evaluated for every element of every launch
template <int KS, bool VERT, bool TIMING = false, bool SIX = false, bool ACTF = false, bool ELU = false>
__global__ __launch_bounds__(256, SIX ? 2 : 3) void gconv_x3_s1_kernel(GX3Args p) {
    unsigned long long T0 = 0, ta = 0, tb = 0, tc = 0, td = 0, te = 0, tf = 0, tg = 0;
    unsigned long long dA = 0, dW = 0, dS = 0, dL = 0, dB = 0, dM = 0;
    PTTA_STAMP(T0);
    constexpr int PAD = KS / 2, PADX = VERT ? 0 : PAD, KKX = VERT ? 1 : KS, PH = GX_TH + 2 * PAD, PW = 32 + 2 * PADX, KK = KS * KKX;
    constexpr int NPIX = PH * PW;
    constexpr int NIT = (NPIX * 2 + 255) / 256;          // (pixel, 8-channel group) items per thread
    constexpr int NPL = SIX ? 3 : 2;                     // operand planes
    constexpr int STR = SIX ? 112 : GX_STR16;            // LDS bytes per pixel: hi 32 | lo 32 [| l2 32] | pad 16 (an odd number of 16-B slots)
    constexpr int NWF = KK * 64 * NPL;                   // weight uint4 per sub-chunk: [hi | lo | l2][tap][lane]
    constexpr int NW = (NWF + 255) / 256;
    constexpr int ACT = NPIX * STR;
    constexpr int LDSB = ACT + NWF * 16 > 32768 ? ACT + NWF * 16 : 32768;     // the epilogue stages 4 x 8 KB through it
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDSB + 1024];
    uint4* const wlds = (uint4*)(lds + ACT);
    const int tid = threadIdx.x, lane = tid & 63;
    const int i = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = p.H, W = p.W;
    const int ntx = (W + 31) >> 5, nty = (H + GX_TH - 1) / GX_TH;
    const unsigned bid = xcd_swizzle(blockIdx.x, gridDim.x);      // the channel tiles of one pixel tile stay on one XCD / L2
    const int nfl = (int)(bid % p.nnf);
    long t_ = bid / p.nnf;
    const int ty = (int)(t_ % nty); t_ /= nty;
    const int tx = (int)(t_ % ntx);
    const int b = (int)(t_ / ntx);
    const int y0 = ty * GX_TH, x0 = tx << 5;
    const int nf = p.nf0 + nfl;
    const int nch0 = (p.C0 + 31) >> 5;
    const int nq = 2 * p.nchunks;
    const bool six = SIX && b < p.six_B;                 // block-uniform
    const bool x1 = b >= p.x1_from_B;                    // block-uniform: images of the single-MFMA class (mixed mode: proxy frames, data gradients)

    // (weight planes: one base pointer + a per-lane byte offset to the lane's plane -- see issue_loads)
    const char* const wbase_p = (const char*)p.whi;
    const long wd_lo = (const char*)p.wlo - wbase_p, wd_l2 = SIX ? (const char*)p.wl2 - wbase_p : wd_lo;
    float4 v0[NIT], v1[NIT];
    unsigned vok = 0;                                    // bit `it`: item it of the sub-chunk in flight is inside the image and the channel range
    uint4 wr[NW];
    auto issue_loads = [&](int q) __attribute__((always_inline)) {
        const int c = q >> 1, kk = q & 1;
        const bool s1 = c >= nch0;
        const float* src = s1 ? p.x1 : p.x0;
        const int ld = s1 ? p.ld1 : p.ld0, Cs = s1 ? p.C1 : p.C0, cb = ((s1 ? c - nch0 : c) << 5) + 16 * kk;
        const float* inb = src + (size_t)b * H * W * ld;
        // UNCONDITIONAL loads from clamped addresses; zero padding is applied when the values are split into LDS (vok).  Behind
        // `if (inside) { v0 = load; v1 = load; }` hipcc waited vmcnt(0) between the items of one sub-chunk (round 5, .s): the wave
        // that issues the prefetch stalled for a memory round trip per item instead of going on to its matrix instructions.
        vok = 0;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = tid + 256 * it;
            const int g = idx & 1, pix = idx >> 1;
            const int py = pix / PW, px = pix - py * PW;
            const int gy = y0 - PAD + py, gx = x0 - PADX + px;
            const bool ok = pix < NPIX && gy >= 0 && gy < H && gx >= 0 && gx < W && cb + 8 * g < Cs;
            const float* s_ = inb + ((size_t)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1)) * ld + min(cb + 8 * g, Cs - 8);
            v0[it] = *(const float4*)s_; v1[it] = *(const float4*)(s_ + 4);
            vok |= ok ? (1u << it) : 0u;
        }
        const size_t wbase = ((size_t)nf * p.nchunks + c) * (KK * 2 * 64) + kk * 64;
        // The three weight planes are three allocations and a lane's plane index varies within one j.  Written as
        // (hl == 0 ? p.whi : hl == 1 ? p.wlo : p.wl2)[...] hipcc selects the ADDRESS of the kernel argument and loads the pointer from
        // memory -- a dependent load whose s_waitcnt vmcnt(0) also waited for the six activation loads issued just above: every wave
        // stalled for a full memory round trip per sub-chunk, twice, and the prefetch never overlapped the matrix phase (round 5, .s).
        // The plane is therefore chosen by a byte OFFSET from the hi plane's pointer (wd_lo, wd_l2: scalar differences formed once): two
        // v_cndmask on registers, the load unconditional from a clamped index.
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int idx = min(tid + 256 * j, NWF - 1);  // [hl][tap][lane]  (items beyond NWF are not written to LDS)
            const int hl = idx / (KK * 64), r = idx - hl * (KK * 64);
            const uint4* wp = (const uint4*)(wbase_p + (hl == 0 ? 0L : (hl == 1 ? wd_lo : wd_l2)));
            const uint4 t = wp[wbase + (r >> 6) * 128 + (r & 63)];
            wr[j].x = t.x; wr[j].y = t.y; wr[j].z = t.z; wr[j].w = t.w;       // (member-wise: `wr[j] = wp[...]` is a memcpy into the array, which then lives in scratch)
        }
    };
    f32x16 acc[2];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[rr][r] = 0.f;

    issue_loads(0);
    // fetched here, not in the epilogue: there its L2 round trip sat between the last MFMA and the first store (in-kernel stamps)
    const int co = nf * 32 + i - p.nf0 * 32;          // channel inside the output view
    const bool cok = co < p.Cy;
    const float bias = (cok && p.bias) ? p.bias[co] : 0.f;
    // the eval affine's two values of this lane's channel, fetched with the bias (GX3Args::scale)
    const float asc = (cok && p.scale) ? p.scale[co] : 1.f, ash = (cok && p.scale) ? p.shift[co] : 0.f;
    unsigned long long Tpro = 0; PTTA_STAMP(Tpro);
    for (int q = 0; q < nq; ++q) {
        PTTA_STAMP(ta);
        if (q) lds_barrier();                            // previous sub-chunk's MFMAs are done with the LDS tile
        PTTA_STAMP(tb);
        if constexpr (TIMING) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        PTTA_STAMP(tc);
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = tid + 256 * it;
            const int pix = idx >> 1;
            if (pix < NPIX) {
                const bool ok = (vok >> it) & 1u;
                const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 a0 = ok ? v0[it] : z4, a1 = ok ? v1[it] : z4;
                uint4 hi, lo;
                unsigned char* dst = lds + pix * STR + 16 * (idx & 1);
                if constexpr (SIX) {
                    uint4 l2;
                    gsplit3(a0.x, a0.y, hi.x, lo.x, l2.x); gsplit3(a0.z, a0.w, hi.y, lo.y, l2.y);
                    gsplit3(a1.x, a1.y, hi.z, lo.z, l2.z); gsplit3(a1.z, a1.w, hi.w, lo.w, l2.w);
                    *(uint4*)(dst + 64) = l2;
                } else {
                    split2(a0.x, a0.y, hi.x, lo.x); split2(a0.z, a0.w, hi.y, lo.y);
                    split2(a1.x, a1.y, hi.z, lo.z); split2(a1.z, a1.w, hi.w, lo.w);
                }
                *(uint4*)dst = hi;
                *(uint4*)(dst + 32) = lo;
            }
        }
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int idx = tid + 256 * j;
            if (idx < NWF) wlds[idx] = wr[j];
        }
        PTTA_STAMP(td);
        if (q + 1 < nq) issue_loads(q + 1);
        PTTA_STAMP(te);
        lds_barrier();                                   // LDS-only: the loads just issued stay in flight during the MFMAs
        PTTA_STAMP(tf);
        __builtin_amdgcn_s_setprio(1);                    // MFMA phase outranks the other blocks' staging code at issue
#pragma unroll
        for (int tap = 0; tap < KK; ++tap) {
            const int ky = tap / KKX, kx = tap % KKX;
            const bf16x8 bh = __builtin_bit_cast(bf16x8, wlds[tap * 64 + lane]);
            const bf16x8 bl = __builtin_bit_cast(bf16x8, wlds[KK * 64 + tap * 64 + lane]);
            // the two rows' MFMAs alternate: consecutive matrix instructions never accumulate into the same registers
            bf16x8 ah[2], al[2];
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const unsigned char* a = lds + ((2 * wave + rr + ky) * PW + i + kx) * STR + 16 * h;
                ah[rr] = __builtin_bit_cast(bf16x8, *(const uint4*)a);
                al[rr] = __builtin_bit_cast(bf16x8, *(const uint4*)(a + 32));
            }
            if constexpr (SIX) if (six) {                 // the 2^-16 terms first: l.h, h.l, m.m
                const bf16x8 b2 = __builtin_bit_cast(bf16x8, wlds[2 * KK * 64 + tap * 64 + lane]);
                bf16x8 a2[2];
#pragma unroll
                for (int rr = 0; rr < 2; ++rr)
                    a2[rr] = __builtin_bit_cast(bf16x8, *(const uint4*)(lds + ((2 * wave + rr + ky) * PW + i + kx) * STR + 16 * h + 64));
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2[0], bh, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2[1], bh, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[0], b2, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[1], b2, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[0], bl, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[1], bl, acc[1], 0, 0, 0);
            }
            if (!x1) {
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[0], bh, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[1], bh, acc[1], 0, 0, 0);
            }
            if (!x1 || p.x1_w2) {                          // (x1 with hi + lo WEIGHTS: the data gradients of the mixed mode, GX3Args::x1_w2)
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[0], bl, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[1], bl, acc[1], 0, 0, 0);
            }
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[0], bh, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[1], bh, acc[1], 0, 0, 0);
        }
        __builtin_amdgcn_s_setprio(0);
        PTTA_STAMP(tg);
        dA += tb - ta; dW += tc - tb; dS += td - tc; dL += te - td; dB += tf - te; dM += tg - tf;
    }
    unsigned long long Tloop = 0; PTTA_STAMP(Tloop);
    float s1 = 0.f, s2 = 0.f;
    auto activate = [&](float v) {
        if (p.act == GACT_RELU) v = v > 0.f ? v : 0.f;
        else if (p.act == GACT_LRELU) v = v > 0.f ? v : 0.2f * v;
        else if (p.act == GACT_SIGMOID) v = 1.f / (1.f + expf(-v));
        return v;
    };
    // selects only (the compiler if-converts `activate` and then evaluates expf and the division for every element of every launch:
    // 6k of a wave's 36k cycles by the in-kernel stamps); the sigmoid (one layer of the network) runs in its own uniform branch
    auto activate_cheap = [&](float v) {
        const float neg = p.act == GACT_LRELU ? 0.2f * v : (p.act == GACT_RELU ? 0.f : v);
        return v > 0.f ? v : neg;
    };
    // The accumulator layout (lane = channel, register = pixel) would store one dword per lane, 32 store instructions per wave, and
    // the vector-memory instruction path is what this kernel is bound by (in-kernel stamps: the epilogue was 35-40 % of a wave's
    // life).  Transposed through the wave's own 8 KB of the (now idle) tile buffers -- [row 2][pixel 32][channel 32] floats, written
    // conflict-free one pixel per half-wave, read back as float4 -- every lane stores 16 B: 8 store instructions per wave, each
    // covering eight pixels x 128 contiguous bytes.  Bias / activation / statistics stay in the register layout (per-lane channel);
    // a launch that accumulates adds the old values as float4 after the transpose and activates there.
    const bool sig = p.act == GACT_SIGMOID;
    const bool wide = !(p.accumulate && (p.stat_part || sig)) && !(p.ldy & 3) && !(p.Cy & 3) && !(((size_t)p.y) & 15) &&
                      !(p.res && ((p.ld_res & 3) || (((size_t)p.res) & 15)));
    // what the float4 stage adds before the activation: the old output (accumulate) or the residual behind the affine
    const float* const addp = p.accumulate ? p.y : p.res;
    const int ldadd = p.accumulate ? p.ldy : p.ld_res;
    unsigned long long E1 = 0, E2 = 0, E3 = 0;
    if (wide) {
        lds_barrier();                                    // every wave is done with the tile buffers
        PTTA_STAMP(E1);
        float* const tw = (float*)lds + wave * 2048;
        float bias_w = bias;
        if (sig) {                                        // uniform
#pragma unroll
            for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[rr][r] = 1.f / (1.f + expf(-(acc[rr][r] + bias)));
            bias_w = 0.f;
        }
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const bool yok = y0 + 2 * wave + rr < H;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int px = acc_row(r, h);
                float v = sig ? acc[rr][r] : acc[rr][r] + bias_w;
                if (p.scale) v = fmaf(v, asc, ash);
                if constexpr (ACTF) v = v > 0.f ? v : 0.f;
                if constexpr (ELU) v = v > 0.f ? v : expm1f(v);         // (activate_cheap leaves GACT_ELU's value as it is)
                if (!p.accumulate) {
                    v = (sig || p.res) ? v : activate_cheap(v);
                    if (yok && cok && x0 + px < W) { s1 += v; s2 += v * v; }
                }
                tw[(rr * 32 + px) * 32 + i] = v;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // wave-local: a wave's LDS operations execute in order
        PTTA_STAMP(E2);
        const int c4 = (lane & 7) * 4, pl = lane >> 3;
        const int cbase = nf * 32 - p.nf0 * 32 + c4;
        if (cbase < p.Cy) {
            // an accumulating launch reads the eight old values FIRST, unconditionally (clamped pixel): one load + s_waitcnt + store per
            // pixel group was eight memory round trips in a row per wave
            float4 old[8];
            if (addp) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int rr = k >> 2, px = (k & 3) * 8 + pl;
                    const int y = min(y0 + 2 * wave + rr, H - 1), x = min(x0 + px, W - 1);
                    old[k] = *(const float4*)(addp + (((size_t)b * H + y) * W + x) * ldadd + cbase);
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int rr = k >> 2, px = (k & 3) * 8 + pl;
                const int y = y0 + 2 * wave + rr, x = x0 + px;
                if (y >= H || x >= W) continue;
                float4 v = *(const float4*)(tw + (rr * 32 + px) * 32 + c4);
                float* dst = p.y + (((size_t)b * H + y) * W + x) * p.ldy + cbase;
                if (addp) {
                    const float4 o = old[k];
                    v.x = activate_cheap(v.x + o.x); v.y = activate_cheap(v.y + o.y); v.z = activate_cheap(v.z + o.z); v.w = activate_cheap(v.w + o.w);
                }
                *(float4*)dst = v;
            }
        }
    } else {
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int y = y0 + 2 * wave + rr;
        if (y >= H || !cok) continue;
        float* yrow = p.y + ((size_t)b * H + y) * W * p.ldy + co;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int x = x0 + acc_row(r, h);
            if (x >= W) continue;
            float* dst = yrow + (size_t)x * p.ldy;
            float v = acc[rr][r] + bias;
            if (p.scale) v = fmaf(v, asc, ash);
            if constexpr (ACTF) v = v > 0.f ? v : 0.f;
            if constexpr (ELU) v = v > 0.f ? v : expm1f(v);             // (no residual, no accumulate: ptta_gx3_affine_ok; `activate` passes it on)
            if (p.accumulate) v += *dst;
            if (p.res) v += p.res[(((size_t)b * H + y) * W + x) * p.ld_res + co];
            v = activate(v);
            *dst = v;
            s1 += v; s2 += v * v;
        }
    }
    }
    PTTA_STAMP(E3);
    if (p.stat_part) {
        // fused BatchNorm statistics of this tile: lane halves, then the four waves through LDS (fixed order)
        s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
        float* red = (float*)(lds + LDSB);                // [wave 4][2][32], its own 1 KB behind the tile buffers
        if (h == 0) { red[(wave * 2 + 0) * 32 + i] = s1; red[(wave * 2 + 1) * 32 + i] = s2; }
        lds_barrier();
        if (tid < 64 && (tid & 31) + nf * 32 - p.nf0 * 32 < p.Cy) {
            const int which = tid >> 5, ch = tid & 31;
            const float v = (red[(0 * 2 + which) * 32 + ch] + red[(1 * 2 + which) * 32 + ch]) + (red[(2 * 2 + which) * 32 + ch] + red[(3 * 2 + which) * 32 + ch]);
            const int bpp = p.B / p.stat_npass, pass = b / bpp;
            const long tile = ((long)(b - pass * bpp) * ntx + tx) * nty + ty;
            const long tiles_pp = (long)bpp * ntx * nty;
            p.stat_part[((pass * tiles_pp + tile) * 2 + which) * p.stat_C + (nf - p.nf0) * 32 + ch] = v;
        }
    }
    if constexpr (TIMING) {
        unsigned long long Tend = 0; PTTA_STAMP(Tend);
        if ((blockIdx.x == gridDim.x / 2 || blockIdx.x == gridDim.x / 3) && lane == 0)
            printf("blk %u/%u wave %d nq %d: life %llu pro %llu loop %llu epi %llu (barrier %llu transpose-write %llu read+store %llu stats %llu) | barA %llu vmwait %llu split %llu issue %llu barB %llu mfma %llu\n", blockIdx.x, gridDim.x, wave, nq,
                   Tend - T0, Tpro - T0, Tloop - Tpro, Tend - Tloop, E1 - Tloop, E2 - E1, E3 - E2, Tend - E3, dA, dW, dS, dL, dB, dM);
    }
}

typedef void (*GX3S1Kernel)(GX3Args);

template <int KS, bool VERT, bool ACTF = false, bool ELU = false>
GX3S1Kernel s1_of(bool six) {
    if (six) return gconv_x3_s1_kernel<KS, VERT, false, true, ACTF, ELU>;
    return gconv_x3_s1_kernel<KS, VERT, false, false, ACTF, ELU>;
}

// The one place that says which instantiation a launch runs (null: there is none).
GX3S1Kernel s1_kernel_of(int ks, bool vert, bool six, bool act_first, bool elu) {
    // relu(relu(affine) + res), asked before the ELU: its own instantiations (no vertical form: ptta_gx3_affine_ok)
    if (act_first) return ks == 3 ? s1_of<3, false, true>(six) : (ks == 1 ? s1_of<1, false, true>(six) : nullptr);
    // fmaf, then ELU: the 3-tap forms of CostDCNet's UNet3D (1x3x3 and the vertical 3x1x1), bf16x3 and bf16x6
    if (elu) return ks != 3 ? nullptr : (vert ? s1_of<3, true, false, true>(six) : s1_of<3, false, false, true>(six));
    if (ks == 3 && vert) return s1_of<3, true>(six);
#ifdef PTTA_DIAG_STAMPS      // diagnostic build (make DIAG=1): in-kernel phase stamps of the plain 3x3 launches
    if (ks == 3 && !six) return gconv_x3_s1_kernel<3, false, true>;
#endif
    if (ks == 3) return s1_of<3, false>(six);
    if (ks == 1) return s1_of<1, false>(six);             // (a 1x1 launch with `vert` set runs this kernel too)
    return nullptr;
}

long s1_tiles(long B, int H, int W) { return B * ((W + 31) / 32) * ((H + GX_TH - 1) / GX_TH); }

}  // namespace

int ptta_gconv_x3_tiles(int B, int H, int W) { return (int)s1_tiles(B, H, W); }

int ptta_launch_gconv_x3(const GX3Args& a, int ks, hipStream_t s) {
    if ((a.C0 & 7) || (a.C1 & 7) || (a.ld0 & 3) || (a.ld1 & 3)) return -22;        // channel counts: multiples of 8
    if (a.nchunks != (a.C0 + 31) / 32 + (a.C1 + 31) / 32 || !ptta_gx3_affine_ok(a)) return -22;
    const long blocks = s1_tiles(a.B, a.H, a.W) * a.nnf;       // (in long: a map whose block count passes 2^31 is refused, not wrapped)
    if (blocks < 1 || blocks > 0x7fffffffL) return -22;
    if (a.six_B > 0 && !a.wl2) return -22;
    const GX3S1Kernel kernel = s1_kernel_of(ks, a.vert != 0, a.six_B > 0, a.aff_act_first != 0, a.act == GACT_ELU);
    if (!kernel) return -22;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    PTTA_CHECK_LAUNCH();
    return 0;
}

