// The first two layers of an encoder stage, and the backward of a prediction head, as one launch of the persistent stride-1 body
// (ptta_launch_conv32_first; large maps only).
#include "conv32_launch.h"


// ---- the first two layers of an encoder stage in ONE launch: Conv2d(cin <= 3, 32) - ReLU - Conv2d(32, 32) (RGBEncoder.init / DepthEncoder.init,
// network_exp_msg_chn_adapt.py:172-176, :218-222) ----
// The 32-channel map between the two convolutions never makes a round trip through HBM as the second convolution's INPUT: a block
// stages the (8 + 4) x (32 + 4) window of the cin input planes (<= 5 KB instead of a 43.5-KB 32-channel halo), computes the first
// convolution for its (8 + 2) x (32 + 2) halo on the matrix cores exactly as conv_in_lds_kernel does (v_mfma_f32_32x32x2_f32 over
// k = 9 cin, the same k order: bit-identical values, 1.33 x recomputed), applies the zero padding of the SECOND convolution, ReLU and the
// bf16 split on the accumulators (lane-quad transpose: four channels of one pixel per lane, 8-byte LDS stores) and then runs the
// body of conv32_s1_x3_kernel on that LDS tile.  The pre-activation map is still written for the frames whose backward needs it as a
// ReLU mask (`a_out`, frames b < a_nb: the real frames; not at all for the RGB encoder).  The input-plane window lives in the LDS
// region of the bilinear-skip window (dead until the matrix phase); the next tile's window is prefetched into registers.
// The same construction serves the backward of a prediction head: d v = conv^T_{1 -> 32}(g) * (v > 0) followed by the data gradient of
// prdct.1 (a stride-1 32 -> 32 convolution with a ReLU-mask epilogue) -- FMASK: the first convolution's output is masked by the sign bits
// of a 32-channel map (one word per halo pixel, applied after the lane-quad transpose), RELU_MID = false: no ReLU in between, EMASK: the second convolution's
// epilogue mask.  The 55-MB d v map is neither written nor read.
// T = storage / arithmetic of the SECOND convolution and of the output (the input planes are planar fp32 either way).
struct FirstP {
    Plane pl[3]; int zero_from_b;
    const float* w1;             // [14][64] fp32 MFMA fragments of the first convolution (ptta_pack_conv_in)
    const float* bias1;          // may be null
    float* a_out; int a_nb;
    const uint32_t* fmask_bits; int fmask_nb;        // FMASK: sign bits of the first convolution's ReLU mask (one word per pixel), frames b % fmask_nb
    uint32_t* a_bits;                        // sign bits of the a_out map for the same frames (the backward's mask), or null
};
template <typename T, int CIN, bool UP, bool FMASK = false, bool RELU_MID = true, bool EMASK = false, bool EADD = false, bool W2 = false>
__global__ __launch_bounds__(256, 2) void conv32_s1_first_kernel(Conv32P<T> p, FirstP f) {
    constexpr int STR = Geo<T>::STR, WL = (sizeof(T) == 4 || W2) ? 18 * 64 * 16 : 0;
    constexpr int UPH = 6, UPW = 18;
    constexpr int K1 = 9 * CIN, NS = (K1 + 1) / 2;
    constexpr int PL_W = 36, PL_H = 12, PLANE = PL_H * PL_W;
    constexpr int PLSZ = (CIN * PLANE + 4) * 4, USZ = UP ? UPH * UPW * Geo<T>::UPPX : 0, AUX = USZ > PLSZ ? USZ : PLSZ;
    constexpr int NPJ = (PLANE + 255) / 256, NPL = CIN * NPJ;       // items per thread: NPJ of each plane (the plane index is a compile-time constant
                                                                    // of every item: f.pl[ci] stays in scalar registers -- indexed by a lane-varying
                                                                    // ci it was fetched from memory, a dependent load in front of every data load)
    __shared__ __attribute__((aligned(16))) unsigned char lds[X3_PH * X3_PW * STR + WL + AUX];
    unsigned char* const wl_lds = lds + X3_PH * X3_PW * STR;
    unsigned char* const up_lds = wl_lds + WL;
    float* const planes = (float*)up_lds;
    const int tid = threadIdx.x, lane = tid & 63;
    const int i = lane & 31, h = lane >> 5;
    const float biasv = epi_bias(p.epi, i);               // once per kernel: ptta_common.h epi_tile
    // per-lane index arithmetic is recomputed in each phase from an opaque copy of the lane id: hoisted out of the persistent tile loop it
    // becomes dozens of long-lived registers (the UP variants spilled 5 - 34) and a scratch reload between two global loads serialises them
    auto opaque = [](int v) { asm volatile("" : "+v"(v)); return v; };
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = p.Hout, W = p.Wout;
    const int ntx = (W + 31) >> 5, nty = (H + X3_TH - 1) / X3_TH;
    const long ntiles = (long)p.B * ntx * nty;
    const float sy = up_scale(H >> 1, H), sx = up_scale(W >> 1, W);
    // the window's loads are UNCONDITIONAL (clamped address) and RAW: zero padding and the optional photometric normalisation are applied when
    // the values go to LDS one tile later.  With `if (inside) { v = load; if (norm) v = ... }` every load was followed by its own
    // s_waitcnt (the normalisation consumes the value inside the branch): four memory round trips in a row in front of every tile's second
    // convolution (round 5, .s)
    float pv[NPL];
    unsigned pvok = 0;
    auto load_planes = [&](long tile) {
        int b, y0, x0;
        tile_coords<X3_TH>(tile, ntx, nty, b, y0, x0);
        const bool live = b < f.zero_from_b;
        const int tid_ = opaque(tid);
        pvok = 0;
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) {
            const Plane& pl = f.pl[ci];
            const float* pb = pl.p + (size_t)(b % pl.nb) * pl.bstride;
#pragma unroll
            for (int j = 0; j < NPJ; ++j) {
                const int r = tid_ + 256 * j;
                const int py = r / PL_W, px = r - py * PL_W;
                const int gy = y0 - 2 + py, gx = x0 - 2 + px;
                const bool ok = r < PLANE && live && gy >= 0 && gy < H && gx >= 0 && gx < W;
                pv[ci * NPJ + j] = pb[(size_t)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1)];
                pvok |= ok ? (1u << (ci * NPJ + j)) : 0u;
            }
        }
    };
    auto stage_planes = [&]() {                           // the prefetched window -> LDS: 0 outside the image / for the proxy frames, normalised inside
        const int tid_ = opaque(tid);
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) {
            const Plane& pl = f.pl[ci];
#pragma unroll
            for (int j = 0; j < NPJ; ++j) {
                const int r = tid_ + 256 * j, k = ci * NPJ + j;
                float v = pv[k];
                if (pl.norm) v = (v / pl.div - pl.mean) / pl.stdv;
                if (r < PLANE) planes[ci * PLANE + r] = ((pvok >> k) & 1u) ? v : 0.f;
            }
        }
    };
    // FMASK: the first convolution's ReLU mask comes in its sign-bit form only (fmask_bits, one word per pixel): the 12 words of this wave's
    // three halo groups are fetched one tile AHEAD, with the input planes and before the current tile's epilogue stores -- a load issued
    // after those stores cannot complete before they have drained (vmcnt is in order and counts stores), which cost ~20 us per tile round.
    // (Holding all three groups' FLOAT masks across the previous tile's main loop spilled 51 registers and was 20 us slower.)
    constexpr int NGW = FMASK ? 3 : 1;
    uint32_t mkw[NGW][4];
    auto load_masks = [&](long tile) {
        if (!FMASK) return;
        int b, y0, x0;
        tile_coords<X3_TH>(tile, ntx, nty, b, y0, x0);
        const int tq = (i & 3) + 4 * h;
        const uint32_t* mbb = f.fmask_bits + (size_t)(b % f.fmask_nb) * H * W;
#pragma unroll
        for (int gi = 0; gi < NGW; ++gi)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int pp = min(32 * (wave + 4 * gi) + 8 * j + tq, X3_PH * X3_PW - 1);
                const int py = pp / X3_PW, px = pp - py * X3_PW;
                const int gy = min(max(y0 - 1 + py, 0), H - 1), gx = min(max(x0 - 1 + px, 0), W - 1);
                mkw[gi][j] = mbb[(size_t)gy * W + gx];
            }
    };
    if (blockIdx.x < ntiles) { load_planes(blockIdx.x); load_masks(blockIdx.x); }
    uint4 wh[9][2];
    constexpr bool NARF = sizeof(T) == 2;            // narrow: the FIRST convolution on the bf16 matrix cores too (K = 9 cin <= 27 padded to 32: two
                                                     // v_mfma_f32_32x32x16_bf16 instead of fourteen v_mfma_f32_32x32x2_f32 per 32 halo pixels)
    float w1[NARF ? 1 : NS];
    uint4 w1b[2];                                    // NARF: the first convolution's weights as two bf16 B fragments (k = 16 ks + 8 h + e)
    uint4 w1l[W2 ? 2 : 1];                           // W2: their lo halves (w - bf16(w), rounded to bf16)
    load_weights<T, W2>(wh, wl_lds, p.wpack, p.wpack2, tid, lane);
    if constexpr (NARF) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            float wv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = 16 * ks + 8 * h + e;               // fp32 fragment layout (ptta_pack_conv_in): [k >> 1][lane = (k & 1) * 32 + cout]
                wv[e] = k < K1 ? f.w1[(k >> 1) * 64 + (k & 1) * 32 + i] : 0.f;
            }
            w1b[ks] = make_uint4(pack_bf2(wv[0], wv[1]), pack_bf2(wv[2], wv[3]), pack_bf2(wv[4], wv[5]), pack_bf2(wv[6], wv[7]));
            if constexpr (W2) {
                unsigned hi_[4], lo_[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) split2(wv[2 * e], wv[2 * e + 1], hi_[e], lo_[e]);
                w1b[ks] = make_uint4(hi_[0], hi_[1], hi_[2], hi_[3]);
                w1l[ks] = make_uint4(lo_[0], lo_[1], lo_[2], lo_[3]);
            }
        }
    } else {
#pragma unroll
        for (int s_ = 0; s_ < NS; ++s_) w1[s_] = f.w1[s_ * 64 + lane];
    }
    const float b1 = f.bias1 ? f.bias1[i] : 0.f;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int b, y0, x0;
        tile_coords<X3_TH>(tile, ntx, nty, b, y0, x0);
        // ---- the input-plane window (prefetched) -> LDS ----
        stage_planes();
        if (tid == 0) planes[CIN * PLANE] = 0.f;                       // the padded k of an odd 9 cin reads this word
        lds_barrier();
        // ---- first convolution on the halo: pixel p = 34 py + px of the (8 + 2) x (32 + 2) halo, 32 pixels per MFMA group ----
        const bool amap = f.a_out != nullptr && b < f.a_nb;
        const bool abits = f.a_bits != nullptr && b < f.a_nb;
        auto halo_group = [&](const int g, const uint32_t* mk) {
            const int i_ = opaque(i);
            const int tq = (i_ & 3) + 4 * h, c4 = 4 * (i_ >> 2);
            const int pm = min(32 * g + i_, X3_PH * X3_PW - 1);
            const float* base = planes + (pm / X3_PW) * PL_W + (pm % X3_PW);
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            if constexpr (NARF) {
                // A fragment of lane (pixel i_, half h), k-step ks: input values k = 16 ks + 8 h + e -> (tap, plane) at compile-time offsets per h
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    float av[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int ka = 16 * ks + e, kb = 16 * ks + 8 + e;          // the two candidates (h = 0 / 1)
                        const int oa = ka < K1 ? (ka % CIN) * PLANE + ((ka / CIN) / 3) * PL_W + (ka / CIN) % 3 : -1;
                        const int ob = kb < K1 ? (kb % CIN) * PLANE + ((kb / CIN) / 3) * PL_W + (kb / CIN) % 3 : -1;
                        const float va = oa >= 0 ? base[oa] : 0.f, vb = ob >= 0 ? base[ob] : 0.f;
                        av[e] = h ? vb : va;
                    }
                    const uint4 af = make_uint4(pack_bf2(av[0], av[1]), pack_bf2(av[2], av[3]), pack_bf2(av[4], av[5]), pack_bf2(av[6], av[7]));
                    if constexpr (W2) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af), __builtin_bit_cast(bf16x8, w1l[ks]), acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af), __builtin_bit_cast(bf16x8, w1b[ks]), acc, 0, 0, 0);
                }
            } else {
#pragma unroll
            for (int s_ = 0; s_ < NS; ++s_) {
                const int k0 = 2 * s_, k1 = 2 * s_ + 1;
                const int o0 = (k0 % CIN) * PLANE + ((k0 / CIN) / 3) * PL_W + (k0 / CIN) % 3;
                const int o1 = (k1 < K1) ? (k1 % CIN) * PLANE + ((k1 / CIN) / 3) * PL_W + (k1 / CIN) % 3 : -1;
                const float a = h ? (o1 >= 0 ? base[o1] : planes[CIN * PLANE]) : base[o0];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, w1[s_], acc, 0, 0, 0);
            }
            }
            f32x16 t;
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] = acc[r] + b1;
            quad_transpose(t, lane);                                   // lane: channels c4 ... c4 + 3 of pixel 8 j + tq of the group
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int pp = 32 * g + 8 * j + tq;
                const int py = pp / X3_PW, px = pp - py * X3_PW;
                const int gy = y0 - 1 + py, gx = x0 - 1 + px;
                const bool inimg = pp < X3_PH * X3_PW && gy >= 0 && gy < H && gx >= 0 && gx < W;
                float4 v = make_float4(t[4 * j], t[4 * j + 1], t[4 * j + 2], t[4 * j + 3]);
                if (FMASK) {
                    const uint32_t nib = mk[j] >> c4;
                    v.x = (nib & 1u) ? v.x : 0.f; v.y = (nib & 2u) ? v.y : 0.f; v.z = (nib & 4u) ? v.z : 0.f; v.w = (nib & 8u) ? v.w : 0.f;
                }
                const bool store_a = inimg && py >= 1 && py <= X3_TH && px >= 1 && px <= 32;
                if (amap && store_a) *(float4*)(f.a_out + (((size_t)b * H + gy) * W + gx) * 32 + c4) = v;
                if (abits) {                                                        // (wave-uniform; all lanes reach the ballots)
                    const uint32_t word = mask_word_from_quads(v.x, v.y, v.z, v.w, i, h);
                    if (i < 4 && store_a) f.a_bits[((size_t)b * H + gy) * W + gx] = word;
                }
                if (RELU_MID) v = relu4(v);
                if (!inimg) v = make_float4(0.f, 0.f, 0.f, 0.f);                    // the second convolution's zero padding
                if (pp < X3_PH * X3_PW) {
                    if constexpr (sizeof(T) == 4) {
                        uint2 hi, lo;
                        split2(v.x, v.y, hi.x, lo.x); split2(v.z, v.w, hi.y, lo.y);
                        *(uint2*)(lds + pp * STR + 2 * c4) = hi;
                        *(uint2*)(lds + pp * STR + 64 + 2 * c4) = lo;
                    } else {
                        *(uint2*)(lds + pp * STR + 2 * c4) = f4_to_bf4(v);
                    }
                }
            }
        };
        constexpr int NG = (X3_PH * X3_PW + 31) / 32;
        static_assert(!FMASK || NG <= 12, "three halo groups per wave");
        if (FMASK) {
            uint32_t mk[4];
#pragma unroll 1
            for (int gi = 0; gi < NGW; ++gi) {
                if (wave + 4 * gi >= NG) break;
#pragma unroll
                for (int j = 0; j < 4; ++j) mk[j] = gi == 0 ? mkw[0][j] : (gi == 1 ? mkw[NGW > 1 ? 1 : 0][j] : mkw[NGW > 2 ? 2 : 0][j]);
                halo_group(wave + 4 * gi, mk);
            }
        } else {
#pragma unroll 1
            for (int g = wave; g < NG; g += 4) halo_group(g, mkw[0]);
        }
        lds_barrier();                                                  // halo complete; the plane window is dead
        constexpr bool MWPRE = EMASK && !UP && sizeof(T) == 2;           // (as conv32_s1_x3_kernel: the epilogue's mask words in front of the prefetch)
        uint32_t mwp[2][4];
        if constexpr (MWPRE) {
            epi_mask_words<T>(p.epi, b, y0 + 2 * wave, H, W, i, x0, h, mwp[0]);
            epi_mask_words<T>(p.epi, b, y0 + 2 * wave + 1, H, W, i, x0, h, mwp[1]);
        }
        if (tile + gridDim.x < ntiles) { load_planes(tile + gridDim.x); load_masks(tile + gridDim.x); }
        int uy0 = 0, ux0 = 0;
        if (UP) {
            const int Hu = H >> 1, Wu = W >> 1;
            uy0 = lerp_coef(y0, Hu, sy).i0; ux0 = lerp_coef(x0, Wu, sx).i0;
            up_window_dma<T, UPH, UPW>(p.epi.up + (size_t)(b % p.epi.up_nb) * Hu * Wu * 32, Hu, Wu, uy0, ux0, up_lds, opaque(tid), wave);
        }
        // ---- second convolution, two rows per wave; the bilinear window lands during the first row's MFMAs and is awaited (by every
        // wave: the barrier sits outside the row test) before the first epilogue ----
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int row = 2 * wave + rr, y = y0 + row;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            if (y < H) {                                                // wave-uniform
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int ky = tap / 3, kx = tap % 3;
                    const unsigned char* a = lds + ((row + ky) * X3_PW + i + kx) * STR + 16 * h;
#pragma unroll
                    for (int k = 0; k < 2; ++k) mma_step<T, W2>(acc, a + 32 * k, wh[tap][k], wl_lds + ((tap * 2 + k) * 64 + lane) * 16);
                    if (kx == 2) __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (UP && rr == 0) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); lds_barrier(); }      // every wave's pieces of the window have landed
            if (y < H) {
                if (UP) epi_tile<T, false, EMASK, false, true, UPW>(p.epi, b, y, H, W, i, acc, x0, h, W, 1, 0, sy, sx, up_lds, uy0, ux0, &biasv);
                else epi_tile<T, false, EMASK, EADD>(p.epi, b, y, H, W, i, acc, x0, h, W, 1, 0, sy, sx, nullptr, 0, 0, &biasv, MWPRE ? mwp[rr] : nullptr);
            }
        }
        lds_barrier();          // LDS reuse by the next tile (plane window over the bilinear window, halo)
    }
}

// Conv2d(cin, 32) - ReLU - Conv2d(32, 32) in one launch (conv32_s1_first_kernel): `a` describes the SECOND convolution as for
// ptta_launch_conv32 (its `in` is ignored; a.bf16: narrow output and skip operands, one MFMA per product), `f` the first one as for
// ptta_launch_conv_in (its outputs are ignored); a_out: where the first convolution's pre-activation map is still written (frames
// b < a_nb), or null.  Returns 1 when this form does not apply (the caller then launches the two kernels): exact / naive arithmetic,
// epilogues other than the bilinear skip, small maps.
template <typename T>
static int launch_first_t(const Conv32Args& a, const ConvInArgs& f, void* a_out, int a_nb, bool bwd_form, long tiles, hipStream_t s) {
    Conv32P<T> p = conv32_params<T>(a, a.Hin, a.Win);
    p.in = nullptr; p.in_nb = 1;                               // (the second convolution reads the LDS tile)
    p.epi.add2 = nullptr; p.epi.add2_nb = 1; p.epi.bits_sum = 0;          // (add1 / out_sum: the backward form only, see ptta_launch_conv32_first)
    const int blocks = conv32_grid(tiles, kFullChipBlocks);
    FirstP q;
    for (int c = 0; c < 3; ++c) { q.pl[c] = f.pl[c]; if (q.pl[c].nb < 1) q.pl[c].nb = 1; }
    q.zero_from_b = f.zero_from_b; q.w1 = f.wfrag; q.bias1 = f.bias; q.a_out = (float*)a_out; q.a_nb = a_nb;
    q.fmask_nb = f.mask_nb > 0 ? f.mask_nb : 1; q.fmask_bits = f.mask_bits; q.a_bits = f.a_bits;
    if (bwd_form) {
        // cin = 1, the first convolution masked, no ReLU in between, the epilogue masked, with or without the summed second output
        with_flag(a.out_sum != nullptr, [&](auto EADD) {
            constexpr bool eadd = decltype(EADD)::value;
            if constexpr (sizeof(T) == 2) {                    // hi + lo weights: narrow storage only
                if (a.w2) { hipLaunchKernelGGL((conv32_s1_first_kernel<T, 1, false, true, false, true, eadd, true>), dim3(blocks), dim3(256), 0, s, p, q); return; }
            }
            hipLaunchKernelGGL((conv32_s1_first_kernel<T, 1, false, true, false, true, eadd>), dim3(blocks), dim3(256), 0, s, p, q);
        });
    } else {
        with_flag(a.up != nullptr, [&](auto UP) {
            constexpr bool up = decltype(UP)::value;
            if (f.cin == 1) hipLaunchKernelGGL((conv32_s1_first_kernel<T, 1, up>), dim3(blocks), dim3(256), 0, s, p, q);
            else if (f.cin == 2) hipLaunchKernelGGL((conv32_s1_first_kernel<T, 2, up>), dim3(blocks), dim3(256), 0, s, p, q);
            else hipLaunchKernelGGL((conv32_s1_first_kernel<T, 3, up>), dim3(blocks), dim3(256), 0, s, p, q);
        });
    }
    PTTA_CHECK_LAUNCH();
    return 0;
}
int ptta_launch_conv32_first(const Conv32Args& a, const ConvInArgs& f, void* a_out, int a_nb, hipStream_t s) {
    // two shapes: forward (ReLU between the convolutions, optional bilinear skip, no masks) and the prediction head's backward (cin = 1, the
    // first convolution masked, no ReLU in between, the second convolution's epilogue masked, no bilinear skip)
    const bool bwd_form = f.mask != nullptr;
    if (bwd_form && (!f.mask_bits || !a.mask_bits)) return 1;
    if (a.naive || (!a.bf16 && !a.x3) || a.mode != CONV_S1 || a.add2 || f.naive) return 1;
    // (a second output = masked result + one addend: the backward form only -- d z4 = d s0_2 + up2^T(d e3_0), msgchn_backward.hip backbone_backward)
    if ((a.add1 != nullptr) != (a.out_sum != nullptr) || (a.out_sum && !bwd_form)) return 1;
    if (bwd_form ? (a.relu_in || !a.mask || a.up || f.cin != 1) : (!a.relu_in || a.mask != nullptr)) return 1;
    if (f.cin < 1 || f.cin > 3 || f.up || f.add1 || f.B != a.B || f.H != a.Hin || f.W != a.Win) return 1;
    if (a.bf16 && (a_out || f.a_bits)) return 1;             // (a narrow launch has no backward of its own: nothing to keep of the first map)
    if (conv32_s1_small_map(a.B, a.Hin, a.Win)) return 1;
    const long tiles = conv32_tiles(a.B, a.Hin, a.Win, X3_TH);
    return a.bf16 ? launch_first_t<bf16_t>(a, f, a_out, a_nb, bwd_form, tiles, s) : launch_first_t<float>(a, f, a_out, a_nb, bwd_form, tiles, s);
}
