// A strided 32 -> 32 convolution and the stride-1 32 -> 32 convolution that consumes it, on SMALL maps, in ONE launch.
//
// On the 1/4 ... 1/16-resolution maps every convolution launch is one tile per block and its duration is a latency chain (conv32_s1.hip
// conv32_s1_small_kernel), so a (stride-2 -> stride-1) pair costs two such chains and a store -> load round trip of the map in between.
// Here a block owns a 4 x 32 tile of the STRIDE-1 output, the tile grid of conv32_s1_small_kernel: phase 1 computes the first convolution for
// the tile plus its one-pixel halo (6 x 34 intermediate pixels = seven groups of 32 pixels in row-major order, one per wave) from a
// 13 x 69 input window staged in LDS per 16-channel k-step exactly as conv32_s2_lds_kernel does (k-step outer, tap inner), applies the
// first convolution's epilogue, writes the first half's side outputs (its map, its sum, the sign-bit words of the backward's ReLU mask)
// for the pixels the tile owns, then ReLU, the zero padding of the
// SECOND convolution and the bf16 split, and leaves the result in LDS in the layout of conv32_s1_small_kernel's halo tile.  Phase 2 is that
// kernel's body and epilogue on the LDS tile.  The intermediate map makes no memory round trip between the two phases, and a block depends
// on nothing but its own loads: every global load of the block -- both k-steps of the window, both weight sets, the bilinear window --
// is issued before the first wait.
//
// Same products in the same order as the two kernels it replaces (first: conv32_s2_lds_kernel -- per (k-step, tap): xl wh, xh wl, xh wh;
// second: conv32_s1_small_kernel -- per (tap, k-step) the same three), the same roundings of the stored intermediate (narrow storage: one
// rounding to bf16, then ReLU on the packed value): every output is bit-identical to the two-launch chain (tests/test_gpu_conv_pair.py).
// The tile grid is the stride-1 kernel's on purpose: a 4 x 30 tile (an intermediate of exactly six MFMA rows) was built first and was NOT
// bit-identical -- hipcc contracts the bilinear skip's expression differently in the first of epi_tile's four unrolled pixel groups than in
// the other three, so a pixel's last bits depend on which group of its tile it falls in, and only the same column -> lane mapping gives
// the same bits (measured: 9 of 70 columns off by a few ulp with 30-wide tiles, none with 32-wide ones).
//
// Instantiated (the call sites of msgchn_forward.hip whose stride-1 half takes the small-map kernel; everything else stays two launches):
//   first  = CONV_S2, ReLU on load, no epilogue operands (map and sign bits as side outputs)
//   second = ReLU on load, bilinear x2 skip, with or without skip addends (one or two), map and / or sum output
//     depth_encoder2.enc1.1 -> enc1.3 (UP), depth_encoder2.enc2.1 -> enc2.3 (UP + ADD), depth_encoder3.enc2.1 -> enc2.3 (UP, UP + ADD),
//     T = float (the real frames) and T = bf16 (the proxy frames of the mixed mode).
//   and the three stride-2 pairs of the mixed mode's data gradients (msgchn_backward.hip; T = bf16, W2 = weights as hi + lo in both layers, no
//   ReLU): first = CONV_S2 with a ReLU-mask (sign-bit words) and one addend, whose SUM output the second layer reads; second = ReLU-mask
//     depth_decoder3.dec2.1 -> depth_encoder3.enc2.3, depth_decoder2.dec1.1 -> dec2.3, depth_decoder2.dec2.1 -> depth_encoder2.enc2.3.
//   The first layer's mask words and addend are read for the halo pixels too; its map (when wanted) and its sum are written from the
//   owned pixels.
// Not instantiated: a transposed first half (either direction), the data gradients of the all-fp32 mode, every other epilogue combination.
#include "conv32_launch.h"

#define PR_TH 4                         // output rows of a tile
#define PR_TW 32                        // output columns of a tile
#define PR_MH (PR_TH + 2)               // intermediate rows and columns: tile + halo (row pitch X3_PW = 34, the stride-1 halo tile's)
#define PR_NG ((PR_MH * X3_PW + 31) / 32)       // 32-pixel groups of the intermediate tile, one per phase-1 wave
#define PR_WH (2 * PR_MH + 1)           // input window of the 6 x 34 intermediate pixels
#define PR_WW (2 * X3_PW + 1)
#define PR_NT 512
static_assert(PR_TW + 2 == X3_PW && PR_NG * 64 <= PR_NT, "one wave per group of the intermediate tile");

// RELU: ReLU on both layers' inputs; M1 / A1: the first layer's ReLU-mask (sign-bit words) and addend (its SUM output is then what the second
// layer reads); UP / ADD / M2: the second layer's bilinear skip, addends and ReLU mask; W2: narrow storage, weights as hi + lo in both layers
template <typename T, int FIRST, bool W2, bool RELU, bool M1, bool A1, bool UP, bool ADD, bool M2>
__global__ __launch_bounds__(PR_NT, 1) void conv32_pair_small_kernel(Conv32P<T> p1, Conv32P<T> p2) {
    static_assert(FIRST == CONV_S2, "instantiated forms: see the head of this file");
    constexpr bool F32 = sizeof(T) == 4, LO = F32 || W2;             // LO: a second (lo) weight image per layer
    static_assert(!(W2 && F32) && !((M1 || A1) && F32), "the masked / summed first half exists for the narrow data gradients");
    constexpr int STR = Geo<T>::STR;                                  // intermediate pixel (the stride-1 halo tile's layout)
    constexpr int WSTR = F32 ? 80 : 48;                               // window pixel of one k-step: hi 32 B (| lo 32 B) | pad 16 B
    constexpr int NWPIX = PR_WH * PR_WW, NIT = (NWPIX * 2 + PR_NT - 1) / PR_NT;
    constexpr int WFR = 18 * 64, NWI = (WFR + PR_NT - 1) / PR_NT;      // 16-byte fragments of one weight image
    constexpr int UPH = 4, UPW = 18, NUP = UPH * UPW * Geo<T>::UPPC, NUI = UP ? (NUP + PR_NT - 1) / PR_NT : 1;
    constexpr int WIN_B = NWPIX * WSTR + 16, MID_B = PR_MH * X3_PW * STR, W1_B = (LO ? 2 : 1) * WFR * 16, W2L_B = LO ? WFR * 16 : 0;
    static_assert(!UP || UPH * UPW * Geo<T>::UPPX <= WIN_B, "the bilinear window takes the input window's place once phase 1 is over");
    __shared__ __attribute__((aligned(16))) unsigned char lds[WIN_B + MID_B + W1_B + W2L_B];
    unsigned char* const win = lds;
    unsigned char* const mid = lds + WIN_B;
    unsigned char* const w1_lds = mid + MID_B;                        // first convolution: [hi | lo][tap][k][lane]
    unsigned char* const w2l_lds = w1_lds + W1_B;                     // second convolution, fp32 storage: the lo fragments
    unsigned char* const up_lds = win;                                // (dead until phase 1 is over)
    const int tid = threadIdx.x, lane = tid & 63;
    const int i = lane & 31, h = lane >> 5;
    const float bias1 = epi_bias(p1.epi, i), bias2 = epi_bias(p2.epi, i);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Hin = p1.Hin, Win = p1.Win, Hm = p2.Hout, Wm = p2.Wout;
    const int ntx = (Wm + PR_TW - 1) / PR_TW, nty = (Hm + PR_TH - 1) / PR_TH;
    const int tile = blockIdx.x;
    const int ty = tile % nty, tx = (tile / nty) % ntx, b = tile / (nty * ntx);
    const int y0 = ty * PR_TH, x0 = tx * PR_TW;
    const float sy = up_scale(Hm >> 1, Hm), sx = up_scale(Wm >> 1, Wm);

    // ---- every global load of the block, back to back (unconditional, clamped addresses; zero-filled at staging time) ----
    const T* inb = p1.in + (size_t)(b % p1.in_nb) * Hin * Win * 32;
    Px<T> v[2][NIT];
    unsigned vok = 0;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int idx = tid + PR_NT * it;
        const int g = idx & 1, pix = idx >> 1;
        const int py = pix / PR_WW, px = pix - py * PR_WW;
        const int gy = 2 * y0 - 3 + py, gx = 2 * x0 - 3 + px;         // intermediate pixel (y0 - 1, x0 - 1) reads input (2 y0 - 3 ..., 2 x0 - 3 ...)
        if (pix < NWPIX && gy >= 0 && gy < Hin && gx >= 0 && gx < Win) vok |= 1u << it;
        const T* src = inb + ((size_t)min(max(gy, 0), Hin - 1) * Win + min(max(gx, 0), Win - 1)) * 32 + 8 * g;
        v[0][it] = px_load(src);
        v[1][it] = px_load(src + 16);
    }
    uint4 w1h[NWI], w1l[LO ? NWI : 1], w2l[LO ? NWI : 1];
#pragma unroll
    for (int k = 0; k < NWI; ++k) {
        const int idx = min(tid + PR_NT * k, WFR - 1);
        w1h[k] = ((const uint4*)p1.wpack)[idx];
        if constexpr (LO) { w1l[k] = ((const uint4*)p1.wpack2)[idx]; w2l[k] = ((const uint4*)p2.wpack2)[idx]; }
    }
    uint4 wh2[9][2];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int k = 0; k < 2; ++k) wh2[t][k] = ((const uint4*)p2.wpack)[(t * 2 + k) * 64 + lane];
    int uy0 = 0, ux0 = 0;
    // (two named registers, not an array: indexed in a loop behind the barriers hipcc kept the loop rolled and the array in scratch)
    uint4 upv0 = make_uint4(0u, 0u, 0u, 0u), upv1 = upv0;
    static_assert(NUI <= 2, "bilinear window pieces per thread");
    auto up_src = [&](const int idx_) {
        constexpr int PC = Geo<T>::UPPC;
        const int Hu = Hm >> 1, Wu = Wm >> 1;
        const int idx = min(idx_, NUP - 1);
        const int q = idx % PC, pix = idx / PC;
        const int r = pix / UPW, cc = pix - r * UPW;
        const int gy = min(uy0 + r, Hu - 1), gx = min(ux0 + cc, Wu - 1);
        return (const uint4*)(p2.epi.up + (size_t)(b % p2.epi.up_nb) * Hu * Wu * 32 + ((size_t)gy * Wu + gx) * 32 + (32 / PC) * q);
    };
    if constexpr (UP) {
        uy0 = lerp_coef(y0, Hm >> 1, sy).i0; ux0 = lerp_coef(x0, Wm >> 1, sx).i0;
        upv0 = *up_src(tid);
        if constexpr (NUI > 1) upv1 = *up_src(tid + PR_NT);
    }

    // M1 / A1: the first layer's mask words and addend of this lane's four intermediate pixels (halo pixels included), four channels each
    uint32_t mw1[M1 ? 4 : 1];
    uint2 a1v[A1 ? 4 : 1];
    if constexpr (M1 || A1) {
        const int tq_ = (i & 3) + 4 * h;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int pp = min(32 * min(wave, PR_NG - 1) + 8 * j + tq_, PR_MH * X3_PW - 1);
            const int row = pp / X3_PW, col = pp - row * X3_PW;
            const size_t cpix = (size_t)min(max(y0 - 1 + row, 0), Hm - 1) * Wm + min(max(x0 - 1 + col, 0), Wm - 1);
            if constexpr (M1) mw1[j] = p1.epi.mask_bits[(size_t)(b % p1.epi.mask_nb) * Hm * Wm + cpix];
            if constexpr (A1) a1v[j] = *(const uint2*)((const bf16_t*)p1.epi.add1 + ((size_t)(b % p1.epi.add1_nb) * Hm * Wm + cpix) * 32 + 4 * (i >> 2));
        }
    }

    auto stage_window = [&](const int q) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = tid + PR_NT * it;
            const int pix = idx >> 1;
            Px<T> x = v[q][it];
            if (!((vok >> it) & 1u)) x = px_zero<T>();
            if (pix < NWPIX) px_stage<RELU>(x, win + pix * WSTR + 16 * (idx & 1), 32);
        }
    };
    // one k-step of the first convolution for this wave's intermediate row: tap inner, as conv32_s2_lds_kernel
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int pm = min(32 * wave + i, PR_MH * X3_PW - 1);              // this lane's intermediate pixel in phase 1 (row-major, pitch 34)
    const unsigned char* const abase = win + ((2 * (pm / X3_PW)) * PR_WW + 2 * (pm % X3_PW)) * WSTR + 16 * h;
    auto first_kstep = [&](const int q) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap % 3;
            const unsigned char* a = abase + (ky * PR_WW + kx) * WSTR;
            const bf16x8 ah = __builtin_bit_cast(bf16x8, *(const uint4*)a);
            const bf16x8 bh = __builtin_bit_cast(bf16x8, *(const uint4*)(w1_lds + ((tap * 2 + q) * 64 + lane) * 16));
            if constexpr (F32) {
                const bf16x8 al = __builtin_bit_cast(bf16x8, *(const uint4*)(a + 32));
                const bf16x8 bl = __builtin_bit_cast(bf16x8, *(const uint4*)(w1_lds + ((WFR + (tap * 2 + q) * 64) + lane) * 16));
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);   // small terms first
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
            } else if constexpr (W2) {
                const bf16x8 bl = __builtin_bit_cast(bf16x8, *(const uint4*)(w1_lds + ((WFR + (tap * 2 + q) * 64) + lane) * 16));
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
        }
    };

    // ---- phase 1: the first convolution on the tile and its halo ----
    stage_window(0);
#pragma unroll
    for (int k = 0; k < NWI; ++k) {
        const int idx = tid + PR_NT * k;
        if (idx < WFR) {
            *(uint4*)(w1_lds + idx * 16) = w1h[k];
            if constexpr (LO) { *(uint4*)(w1_lds + (WFR + idx) * 16) = w1l[k]; *(uint4*)(w2l_lds + idx * 16) = w2l[k]; }
        }
    }
    lds_barrier();
    if (wave < PR_NG) first_kstep(0);
    lds_barrier();                                          // every wave is done with the first k-step's window
    stage_window(1);
    lds_barrier();
    if (wave < PR_NG) {
        first_kstep(1);
        // the first convolution's epilogue on this wave's 32 intermediate pixels: bias, side outputs for the pixels the tile owns, then what
        // the second convolution does to its input -- ReLU, ZERO outside the map (its padding), the bf16 split
        f32x16 t;
#pragma unroll
        for (int r = 0; r < 16; ++r) t[r] = acc[r] + bias1;
        quad_transpose(t, lane);                            // lane: channels c4 ... c4 + 3 of pixel 8 j + tq of the row
        const int tq = (i & 3) + 4 * h, c4 = 4 * (i >> 2);
        const bool wbits = F32 && p1.epi.bits_out != nullptr && b < p1.epi.bits_nb;       // wave-uniform
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int pp = 32 * wave + 8 * j + tq;
            const int row = pp / X3_PW, col = pp - row * X3_PW;
            const int my = y0 - 1 + row, mx = x0 - 1 + col;
            const bool inimg = pp < PR_MH * X3_PW && my >= 0 && my < Hm && mx >= 0 && mx < Wm;
            const bool own = inimg && row >= 1 && row <= PR_TH && col >= 1 && col <= PR_TW;
            const size_t opix = inimg ? ((size_t)b * Hm + my) * Wm + mx : 0;
            const float4 val = make_float4(t[4 * j], t[4 * j + 1], t[4 * j + 2], t[4 * j + 3]);
            unsigned char* dst = mid + min(pp, PR_MH * X3_PW - 1) * STR + 2 * c4;
            if constexpr (F32) {
                if (p1.epi.out_raw && own) *(float4*)((float*)p1.epi.out_raw + opix * 32 + c4) = val;
                if (wbits) {                                // (all 64 lanes reach the ballots)
                    const uint32_t word = mask_word_from_quads(val.x, val.y, val.z, val.w, i, h);
                    if (i < 4 && own) p1.epi.bits_out[opix] = word;
                }
                float4 r = RELU ? relu4(val) : val;
                if (!inimg) r = make_float4(0.f, 0.f, 0.f, 0.f);
                uint2 hi, lo;
                split2(r.x, r.y, hi.x, lo.x); split2(r.z, r.w, hi.y, lo.y);
                if (pp < PR_MH * X3_PW) { *(uint2*)dst = hi; *(uint2*)(dst + Geo<T>::LO) = lo; }
            } else {
                float4 mv = val;                            // (the narrow branch of epi_tile, step for step)
                if constexpr (M1) {
                    const uint32_t nib = mw1[j] >> c4;
                    mv.x = (nib & 1u) ? mv.x : 0.0f; mv.y = (nib & 2u) ? mv.y : 0.0f; mv.z = (nib & 4u) ? mv.z : 0.0f; mv.w = (nib & 8u) ? mv.w : 0.0f;
                }
                uint2 pk = f4_to_bf4(mv);                   // the one rounding of the stored map
                if (p1.epi.out_raw && own) *(uint2*)((bf16_t*)p1.epi.out_raw + opix * 32 + c4) = pk;
                if constexpr (A1) {                         // the SUM output: what the second layer reads
                    const float4 a = bf4_to_f4(a1v[j]);
                    mv.x += a.x; mv.y += a.y; mv.z += a.z; mv.w += a.w;
                    pk = f4_to_bf4(mv);
                    if (p1.epi.out_sum && own) *(uint2*)((bf16_t*)p1.epi.out_sum + opix * 32 + c4) = pk;
                }
                if constexpr (RELU) { pk.x = relu_pk(pk.x); pk.y = relu_pk(pk.y); }
                if (!inimg) pk = make_uint2(0u, 0u);
                if (pp < PR_MH * X3_PW) *(uint2*)dst = pk;
            }
        }
    }
    lds_barrier();                                          // the intermediate tile is complete, the input window dead
    if constexpr (UP) {
        if (tid < NUP) *(uint4*)(up_lds + (size_t)tid * 16) = upv0;
        if constexpr (NUI > 1) { if (tid + PR_NT < NUP) *(uint4*)(up_lds + (size_t)(tid + PR_NT) * 16) = upv1; }
    }

    // ---- phase 2: the body of conv32_s1_small_kernel on the LDS tile, one output row per wave ----
    const int y = y0 + wave;
    const bool rowon = wave < PR_TH && y < Hm;              // wave-uniform
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (rowon) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap % 3;
            const unsigned char* a = mid + ((wave + ky) * X3_PW + i + kx) * STR + 16 * h;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const bf16x8 ah = __builtin_bit_cast(bf16x8, *(const uint4*)(a + 32 * k));
                const bf16x8 bh = __builtin_bit_cast(bf16x8, wh2[tap][k]);
                if constexpr (F32) {
                    const bf16x8 al = __builtin_bit_cast(bf16x8, *(const uint4*)(a + 32 * k + 64));
                    const bf16x8 bl = __builtin_bit_cast(bf16x8, *(const uint4*)(w2l_lds + ((tap * 2 + k) * 64 + lane) * 16));
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);   // small terms first (as conv32_s1_small_kernel)
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
                } else if constexpr (W2) {
                    const bf16x8 bl = __builtin_bit_cast(bf16x8, *(const uint4*)(w2l_lds + ((tap * 2 + k) * 64 + lane) * 16));
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
                }
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
            }
        }
    }
    if constexpr (UP) lds_barrier();                        // every wave's pieces of the bilinear window are in LDS
    if (rowon) {
        if (UP) epi_tile<T, false, M2, ADD, true, UPW>(p2.epi, b, y, Hm, Wm, i, acc, x0, h, Wm, 1, 0, sy, sx, up_lds, uy0, ux0, &bias2);
        else epi_tile<T, false, M2, ADD>(p2.epi, b, y, Hm, Wm, i, acc, x0, h, Wm, 1, 0, sy, sx, nullptr, 0, 0, &bias2);
    }
}

template <typename T>
static int launch_pair_t(const Conv32Args& f, const Conv32Args& g, hipStream_t s) {
    const int Hm = f.Hin / 2, Wm = f.Win / 2;
    const Conv32P<T> p1 = conv32_params<T>(f, Hm, Wm), p2 = conv32_params<T>(g, Hm, Wm);
    const long tiles = conv32_tiles(f.B, Hm, Wm, PR_TH);
    if constexpr (sizeof(T) == 2) {
        if (f.w2) {            // the data gradients' form
            hipLaunchKernelGGL((conv32_pair_small_kernel<T, CONV_S2, true, false, true, true, false, false, true>), dim3((unsigned)tiles), dim3(PR_NT), 0, s, p1, p2);
            PTTA_CHECK_LAUNCH();
            return 0;
        }
    }
    with_flag(g.add1 != nullptr, [&](auto ADD) {
        hipLaunchKernelGGL((conv32_pair_small_kernel<T, CONV_S2, false, true, false, false, true, decltype(ADD)::value, false>), dim3((unsigned)tiles), dim3(PR_NT), 0, s, p1, p2);
    });
    PTTA_CHECK_LAUNCH();
    return 0;
}

// `first` and `second` as for two ptta_launch_conv32 calls (second.in is ignored: the intermediate map stays on chip; first.out_raw, when
// set, is still written).  ptta_conv32_pair_applies: the pair is one of the instantiated forms and the stride-1 half would take the
// small-map kernel; the launch returns 1 when it does not (the caller then issues the two launches).
bool ptta_conv32_pair_applies(const Conv32Args& first, const Conv32Args& second) {
    const Conv32Args &f = first, &g = second;
    if (f.mode != CONV_S2 || !conv32_pair_common(f, g)) return false;
    if (!f.w2 && !g.up) return false;                        // the forward's second half: with the bilinear skip
    const int Hm = f.Hin / 2, Wm = f.Win / 2;
    if (Hm < 2 || Wm < 2 || g.Hin != Hm || g.Win != Wm || g.B != f.B || f.B < 1) return false;
    return conv32_s1_small_map(g.B, Hm, Wm);                 // (larger maps keep the persistent kernels)
}
int ptta_launch_conv32_pair(const Conv32Args& first, const Conv32Args& second, hipStream_t s) {
    if (!ptta_conv32_pair_applies(first, second)) return 1;
    return first.bf16 ? launch_pair_t<bf16_t>(first, second, s) : launch_pair_t<float>(first, second, s);
}
