// A transposed (stride-2) 32 -> 32 convolution and the stride-1 32 -> 32 convolution that consumes it, in ONE launch, at every map size.
//
// The opposite case from conv_pair.hip: a transposed 3x3 stride-2 convolution has 1, 2, 2 or 4 active taps per output pixel (by the pixel's
// (y, x) parity; 9/4 on average), so recomputing it for a stride-1 tile plus its one-pixel halo costs about a third of one stride-1 layer's
// matrix work, and its input window is FOUR times smaller than the intermediate: an 8 x 32 tile's 10 x 34 intermediate pixels read a 6 x 18
// window of the half-resolution map.  Nothing but the stride-1 consumer reads the intermediate values (the backward takes the sign-bit
// words), so the fused launch does not have to write the 32-channel map at all: at full resolution that is a 55-MB store and a 55-MB load
// less (fp32 storage, batch 1).
//
// A block owns a TH x 32 tile of the STRIDE-1 output, the tile grid of the kernel it replaces: TH = 8, persistent blocks, where the
// stride-1 half takes conv32_s1_x3_kernel; TH = 4 where it takes conv32_s1_small_kernel.  The 32-wide column -> lane mapping of the second
// phase is the stride-1 kernels' (conv_pair.hip's header: why nothing else is bit-identical).  Per tile:
//   phase 1  the input window (prefetched into registers one tile ahead, ReLU and bf16 split while staged, zero outside the map) goes to
//            LDS, with it -- hi + lo weights -- the first layer's weight fragments (LDS-DMA); the transposed convolution of the tile + halo
//            runs on the matrix cores in groups of 32 pixels of ONE parity class (the active taps are wave-uniform), the groups dealt to
//            the four waves by their MFMA count; epilogue of the first layer (bias), its side outputs for the pixels the tile owns
//            (sign-bit words; the map only when a reader exists), then ReLU, the zero padding of the SECOND convolution and the bf16 split.
//   phase 2  the body and epilogue of the stride-1 kernel on the LDS halo tile, unchanged (fragment reads run ahead of their MFMAs).
// LDS: the window (and, fp32 storage, the first layer's 36 KB of hi + lo fragments) is dead once phase 1's accumulators are complete, the
// halo tile is not written before that, so the two share one region (results wait in registers across one barrier): fp32 storage 52.4 KB +
// the second layer's lo fragments 18.4 KB = 70.8 KB (the stride-1 kernel: 67.4 KB), narrow 27.2 + 18.4 KB -- two blocks per CU as
// before (conv32_strided.hip, the note above conv32_direct_x3_kernel: a form that does not fit beside what runs next to it loses in the step).
// The fp32 form fetches the first layer's fragments again for every tile, from L2 straight into LDS, and waits for them -- and so for the
// previous tile's stores, vmcnt is in order -- at the top of the tile.  Measured against it in the step (MI355X, full-resolution pair,
// launch by launch): the same fragments prefetched into 36 registers with the next window, in front of the tile's stores, 95.7 against
// 73.4 us (256 VGPRs, 13 spilled); the phase-1 fragment reads left to the compiler's order instead of one step ahead 74.7 us.
//
// Same products in the same order as the two launches: per intermediate pixel the active taps in ascending order, k-step 0 then 1, per
// step xl wh, xh wl, xh wh (fp32 storage) / xh wh (narrow) -- conv32_direct_x3_kernel<T, CONV_T2> -- where that kernel skips a tap whose
// input row lies outside the map this one feeds zero fragments (an accumulator that starts at +0 cannot become -0 by adding +-0); the
// same roundings of the stored intermediate (narrow: one rounding to bf16, then ReLU on the packed value).  tests/test_gpu_conv_tpair.py
// compares every output with torch.equal.
//
// Instantiated, both tile heights each:
//   the forward (ReLU on both inputs; first half without epilogue operands; second half with zero, one or two skip addends, map and / or
//   sum output, no bilinear skip, no mask), T = float and T = bf16;
//   the mixed mode's data gradients (DG: T = bf16, weights as hi + lo in both layers -- per step xh wl, xh wh -- no ReLU): first half with a
//   ReLU mask (sign-bit words) and one addend, both read for the halo pixels too, whose SUM output the second layer reads and the owned
//   pixels still write (the side upsamplings read it); second half masked.  Hi + lo weights take the fp32 form's LDS plan: 45.5 + 18.4 KB.
// Everything else stays two launches (the data gradients of the all-fp32 mode among them).
// Registers (gfx950, 256 available at two blocks per CU): <float, 8, ADD> 247 VGPRs, <float, 8> 235, <float, 4, ..> 206 - 224, narrow forward
// 177 - 202, DG <bf16, 4> 236, all without spills; DG <bf16, 8> 256 with 19 spilled (76 B of scratch per lane: mask words and addends
// held across phase 1) -- that form runs only where a block has one tile (ptta_conv32_tpair_pays).
// Where a tile's time goes, and what the waits of the tile loop looked like before the LDS-DMA wait became a builtin: DESIGN_LOG.md §19,
// profiles/tpair_fullres_before.txt / _after.txt (in-kernel stamps: make DIAG=1, tools/diag_tpair.py).
#include "conv32_launch.h"

// TIMING (make DIAG=1 only): s_memtime stamps around the phases of the tile loop, printed per wave by two blocks of the launch (tools/diag_tpair.py)
// DG: the data gradients' form (narrow storage): weights as hi + lo in both layers, no ReLU; the first layer masked by sign-bit words and
// summed with one addend -- both read on the halo pixels too -- and its SUM is what the second layer reads; the second layer masked
template <typename T, int TH, bool ADD, bool DG = false, bool TIMING = false>
__global__ __launch_bounds__(256, 2) void conv32_tpair_kernel(Conv32P<T> p1, Conv32P<T> p2) {
    static_assert(TH == 4 || TH == 8, "tile heights of the two stride-1 kernels");
    unsigned long long T0 = 0, ts = 0, tn = 0;
    unsigned dPro = 0, dStage = 0, dW1 = 0, dBar0 = 0, dPh1 = 0, dBar1 = 0, dHalo = 0, dBar2 = 0, dMfma = 0, dEpi = 0, dBar3 = 0;
    int ntl = 0;
    // one phase's cycles: since the previous stamp
    auto lap = [&](unsigned& d) __attribute__((always_inline)) { if constexpr (TIMING) { PTTA_STAMP(tn); d += (unsigned)(tn - ts); ts = tn; } };
    PTTA_STAMP(T0); ts = T0;
    constexpr bool F32 = sizeof(T) == 4, LO = F32 || DG, RELU = !DG;      // LO: a second (lo) weight image per layer
    // APRE: the second half's skip addends of an output row are requested in FRONT of that row's MFMAs -- row 0's also in front of the next
    // window's prefetch -- instead of in its epilogue (ptta_common.h epi_add_loads); the fp32 persistent form, where a block walks several
    // tiles and the epilogue's round trip is on every tile's critical path
    constexpr bool APRE = F32 && ADD && TH == 8 && !DG;
    static_assert(!DG || (!F32 && !ADD), "the masked / summed first half exists for the narrow data gradients");
    constexpr int STR = Geo<T>::STR, WL = LO ? 18 * 64 * 16 : 0;
    constexpr int PH = TH + 2;                                  // halo rows (row pitch X3_PW = 34)
    constexpr int NR = TH / 2 + 1, NC = X3_PW / 2;              // rows and columns of ONE parity class inside the halo
    constexpr int NQ = NR * NC, NGC = (NQ + 31) / 32;           // pixels and 32-pixel groups of a class; every wave computes NGC groups
    constexpr int WH = TH / 2 + 2, WW = X3_PW / 2 + 1, NWP = WH * WW;        // input window: 6 x 18 (4 x 18) pixels of the half-resolution map
    constexpr int NIT = (((NWP + 7) / 8) * 32 + 255) / 256;     // (pixel, 8-channel group) staging items per thread
    constexpr int WFR = 18 * 64;                                // 16-byte fragments of one weight image
    constexpr int NPC = (LO ? 2 : 1) * 18;                     // 1-KB pieces of the first layer's weights [hi | lo]
    constexpr int HALO_B = PH * X3_PW * STR, WIN_B = NWP * STR, W1_B = NPC * 1024;
    // hi + lo weights: the first layer's 36 KB of fragments share the halo tile's region with the window and are fetched again for every tile
    // (LDS-DMA, no registers); narrow forward: their 18 KB stay in LDS for the whole launch
    constexpr bool W1T = LO;
    constexpr int R_B = W1T ? (HALO_B > WIN_B + W1_B ? HALO_B : WIN_B + W1_B) : (HALO_B > WIN_B ? HALO_B : WIN_B);
    static_assert(WIN_B % 16 == 0 && R_B % 16 == 0, "16-byte LDS pieces");
    __shared__ __attribute__((aligned(16))) unsigned char lds[R_B + WL + (W1T ? 0 : W1_B)];
    unsigned char* const win = lds;                              // phase 1 (dead behind it): the window ...
    unsigned char* const w1_lds = W1T ? lds + WIN_B : lds + R_B; // ... and (hi + lo weights) the first layer's fragments [hi | lo][tap][k][lane]
    unsigned char* const wl_lds = lds + R_B;                     // second layer, hi + lo weights: the lo fragments (the whole launch)
    const int tid = threadIdx.x, lane = tid & 63;
    const int i = lane & 31, h = lane >> 5;
    const float bias1 = epi_bias(p1.epi, i), bias2 = epi_bias(p2.epi, i);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Hin = p1.Hin, Win = p1.Win, H = p2.Hout, W = p2.Wout;
    const int ntx = (W + 31) >> 5, nty = (H + TH - 1) / TH;
    const long ntiles = (long)p2.B * ntx * nty;
    const float sy = up_scale(H >> 1, H), sx = up_scale(W >> 1, W);
    // this wave's phase-1 groups, one nibble each: (class << 2) | group of the class; class bit 1: odd row, bit 0: odd column of the
    // intermediate (taps: 1 / 2 / 2 / 4).  TH = 8: 7, 7, 7, 6 taps per wave; TH = 4: 5, 5, 4, 4.
    const unsigned sched = TH == 8 ? (wave == 0 ? 0x04Cu : wave == 1 ? 0x18Du : wave == 2 ? 0x25Eu : 0x6A9u)
                                   : (wave == 0 ? 0x0Cu : wave == 1 ? 0x1Du : wave == 2 ? 0x54u : 0x98u);

    // the window's loads are UNCONDITIONAL (clamped address); zero outside the map when the values go to LDS one tile later
    Px<T> v[NIT];
    unsigned vok = 0;
    auto issue_loads = [&](long tile) {
        int b, y0, x0;
        tile_coords<TH>(tile, ntx, nty, b, y0, x0);
        const T* inb = p1.in + (size_t)(b % p1.in_nb) * Hin * Win * 32;
        vok = 0;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = tid + 256 * it;
            const int g = idx & 3, pix = x3_stage_pix(idx);
            const int py = pix / WW, px = pix - py * WW;
            const int gy = (y0 >> 1) - 1 + py, gx = (x0 >> 1) - 1 + px;
            if (pix < NWP && gy >= 0 && gy < Hin && gx >= 0 && gx < Win) vok |= 1u << it;
            v[it] = px_load(inb + ((size_t)min(max(gy, 0), Hin - 1) * Win + min(max(gx, 0), Win - 1)) * 32 + 8 * g);
        }
    };
    if (blockIdx.x < ntiles) issue_loads(blockIdx.x);
    uint4 wh[9][2];                                              // second layer: the hi fragments, wave-stationary
    {
        const uint4* ph = (const uint4*)p2.wpack;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int k = 0; k < 2; ++k) wh[t][k] = ph[(t * 2 + k) * 64 + lane];
        if constexpr (LO) {
            // (a copy loop through registers, each of its five turns waiting for its own round trip: 2.5 k of the prologue's 10 k cycles.
            // The same pieces by LDS-DMA, all in flight at once and covered by the first tile's wait, measured 7.5 k -- and no gain in the
            // step that the A/B could tell from noise, with the all-fp32 mode slower on two boxes of three: DESIGN_LOG.md §19)
            const uint4* pl = (const uint4*)p2.wpack2;
            for (int idx = tid; idx < WFR; idx += 256) *(uint4*)(wl_lds + idx * 16) = pl[idx];
        } else {
            const uint4* p1h = (const uint4*)p1.wpack;
            for (int idx = tid; idx < WFR; idx += 256) *(uint4*)(w1_lds + idx * 16) = p1h[idx];
        }
    }
    lap(dPro);

    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int b, y0, x0;
        tile_coords<TH>(tile, ntx, nty, b, y0, x0);
        // ---- the window (prefetched) and the first layer's weights -> LDS ----
        if constexpr (W1T) {
            // (the lane's byte offset from an opaque copy of the lane id: hoisted out of the tile loop the nine 64-bit source addresses were
            // 18 long-lived registers, spilled, and every piece waited vmcnt(0) for its address's scratch reload in front of its request)
            int lane16 = lane * 16;
            asm volatile("" : "+v"(lane16));
#pragma unroll
            for (int k = 0; k < (NPC + 3) / 4; ++k) {
                const int piece = wave + 4 * k;                      // wave-uniform
                if (piece < NPC) {
                    const unsigned char* src = (const unsigned char*)(piece < 18 ? p1.wpack : p1.wpack2) + (size_t)(piece < 18 ? piece : piece - 18) * 1024 + lane16;
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                     (__attribute__((address_space(3))) void*)(w1_lds + piece * 1024), 16, 0, 0);
                }
            }
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = tid + 256 * it;
            const int pix = x3_stage_pix(idx);
            Px<T> x = v[it];
            if (!((vok >> it) & 1u)) x = px_zero<T>();
            if (pix < NWP) px_stage<RELU>(x, win + pix * STR + 16 * (idx & 3), Geo<T>::LO);
        }
        lap(dStage);
        // DG: the first layer's mask words and addend of this lane's pixels of its groups (halo pixels included; clamped addresses), four
        // channels each -- requested in front of the wait below
        uint32_t mw1[DG ? NGC : 1][4];
        uint2 a1v[DG ? NGC : 1][4];
        if constexpr (DG) {
            const int tq_ = (i & 3) + 4 * h;
#pragma unroll
            for (int s_ = 0; s_ < NGC; ++s_) {
                const int code = (int)((sched >> (4 * s_)) & 15u);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int qc = min(32 * (code & 3) + 8 * j + tq_, NQ - 1);
                    const int rr = qc / NC, jj = qc - rr * NC;
                    const int row = 2 * rr + ((code & 8) ? 0 : 1), col = 2 * jj + ((code & 4) ? 0 : 1);
                    const size_t cpix = (size_t)min(max(y0 - 1 + row, 0), H - 1) * W + min(max(x0 - 1 + col, 0), W - 1);
                    mw1[s_][j] = p1.epi.mask_bits[(size_t)(b % p1.epi.mask_nb) * H * W + cpix];
                    a1v[s_][j] = *(const uint2*)((const bf16_t*)p1.epi.add1 + ((size_t)(b % p1.epi.add1_nb) * H * W + cpix) * 32 + 4 * (i >> 2));
                }
            }
        }
        // the weight pieces have landed.  The wait is the BUILTIN, which the compiler's own wait-count bookkeeping reads: behind a wait
        // written as inline assembly it still held the LDS-DMA for outstanding and put s_waitcnt vmcnt(0) in front of every later LDS
        // access of the region -- in front of phase 2's first fragment read (the next window's prefetch, just requested), of the second
        // row's (the first row's stores) and of the halo tile's writes (the sign-bit stores): every memory round trip of a tile exposed
        if constexpr (W1T) __builtin_amdgcn_s_waitcnt(0x0F70);                       // vmcnt(0), expcnt and lgkmcnt left alone (gfx9 encoding)
        lap(dW1);
        lds_barrier();
        lap(dBar0);

        // ---- phase 1: the transposed convolution on the tile and its halo, NGC groups of 32 same-class pixels per wave ----
        const bool wbits = F32 && p1.epi.bits_out != nullptr && b < p1.epi.bits_nb;      // wave-uniform
        const bool wmap = p1.epi.out_raw != nullptr;
        uint2 keep_hi[NGC][4], keep_lo[F32 ? NGC : 1][4];        // the halo values of this wave's groups, as they go to LDS behind the barrier
#pragma unroll
        for (int s_ = 0; s_ < NGC; ++s_) {
            const int code = (int)((sched >> (4 * s_)) & 15u);
            const bool yo = code & 8, xo = code & 4;             // odd row / odd column of the intermediate (wave-uniform)
            const int gi = code & 3;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            {
                const int q = min(32 * gi + i, NQ - 1);          // this lane's pixel of the class: row rr, column j of the class grid
                const int rr = q / NC, j = q - rr * NC;
                const unsigned char* const abase = win + (rr * WW + j) * STR + 16 * h;
                const unsigned char* const wbase = w1_lds + lane * 16;
                // output (my, mx) takes tap (ky, kx) from input ((my + 1 - ky) / 2, (mx + 1 - kx) / 2) when both are whole: an even row the
                // middle tap of its own input row, an odd row tap 0 of the row below and tap 2 of the row above (columns alike).  The class
                // is a compile-time constant of each branch, so that the fragment reads of a step can be issued ahead of the products of
                // the step before (the scheduling barriers of the stride-1 body below)
                auto mma_class = [&](auto yo_c, auto xo_c) __attribute__((always_inline)) {
                    constexpr bool YO = decltype(yo_c)::value, XO = decltype(xo_c)::value;
                    constexpr int NS = (YO ? 2 : 1) * (XO ? 2 : 1) * 2;            // (tap, k-step) steps, taps ascending
                    constexpr int AHEAD = F32 ? 1 : 2, RING = AHEAD + 1;
                    uint4 fah[RING], fbh[RING], fal[F32 ? RING : 1], fbl[LO ? RING : 1];
                    auto frag_load = [&](const int n_) __attribute__((always_inline)) {
                        const int t_ = n_ >> 1, k = n_ & 1;
                        const int ky = YO ? 2 * (t_ / (XO ? 2 : 1)) : 1, kx = XO ? 2 * (t_ % 2) : 1;
                        const int tap = ky * 3 + kx;
                        const unsigned char* a = abase + ((ky == 2 ? 0 : 1) * WW + (kx == 2 ? 0 : 1)) * STR + 32 * k;
                        fah[n_ % RING] = *(const uint4*)a;
                        fbh[n_ % RING] = *(const uint4*)(wbase + (tap * 2 + k) * 1024);
                        if constexpr (F32) fal[n_ % RING] = *(const uint4*)(a + Geo<T>::LO);
                        if constexpr (LO) fbl[n_ % RING] = *(const uint4*)(wbase + (WFR * 16 + (tap * 2 + k) * 1024));
                    };
#pragma unroll
                    for (int n_ = 0; n_ < AHEAD; ++n_) frag_load(n_);
#pragma unroll
                    for (int n_ = 0; n_ < NS; ++n_) {
                        if (n_ + AHEAD < NS) frag_load(n_ + AHEAD);
                        __builtin_amdgcn_sched_barrier(0);
                        const bf16x8 ah = __builtin_bit_cast(bf16x8, fah[n_ % RING]), bh = __builtin_bit_cast(bf16x8, fbh[n_ % RING]);
                        if constexpr (F32) {
                            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fal[n_ % RING]), bh, acc, 0, 0, 0);   // small terms first (as conv32_direct_x3_kernel)
                            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, __builtin_bit_cast(bf16x8, fbl[n_ % RING]), acc, 0, 0, 0);
                        } else if constexpr (DG) {
                            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, __builtin_bit_cast(bf16x8, fbl[n_ % RING]), acc, 0, 0, 0);
                        }
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                };
                typedef std::integral_constant<bool, true> Y_; typedef std::integral_constant<bool, false> N_;
                if (yo) { if (xo) mma_class(Y_{}, Y_{}); else mma_class(Y_{}, N_{}); }          // wave-uniform
                else { if (xo) mma_class(N_{}, Y_{}); else mma_class(N_{}, N_{}); }
            }
            // the first layer's epilogue on the group: bias, side outputs for the pixels the tile owns, then what the second convolution does
            // to its input -- ReLU, ZERO outside the map (its padding), the bf16 split
            f32x16 t;
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] = acc[r] + bias1;
            quad_transpose(t, lane);                              // lane: channels c4 ... c4 + 3 of pixel 8 j + tq of the group
            const int tq = (i & 3) + 4 * h, c4 = 4 * (i >> 2);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int qq = 32 * gi + 8 * j + tq, qc = min(qq, NQ - 1);
                const int rr = qc / NC, jj = qc - rr * NC;
                const int row = 2 * rr + (yo ? 0 : 1), col = 2 * jj + (xo ? 0 : 1);      // halo coordinates (the tile starts at an even row and column)
                const int my = y0 - 1 + row, mx = x0 - 1 + col;
                const bool inimg = qq < NQ && my >= 0 && my < H && mx >= 0 && mx < W;
                const bool own = inimg && row >= 1 && row <= TH && col >= 1 && col <= 32;
                const size_t opix = inimg ? ((size_t)b * H + my) * W + mx : 0;
                const float4 val = make_float4(t[4 * j], t[4 * j + 1], t[4 * j + 2], t[4 * j + 3]);
                if constexpr (F32) {
                    if (wmap && own) *(float4*)((float*)p1.epi.out_raw + opix * 32 + c4) = val;
                    if (wbits) {                                  // (all 64 lanes reach the ballots)
                        const uint32_t word = mask_word_from_quads(val.x, val.y, val.z, val.w, i, h);
                        if (i < 4 && own) p1.epi.bits_out[opix] = word;
                    }
                    float4 r = RELU ? relu4(val) : val;
                    if (!inimg) r = make_float4(0.f, 0.f, 0.f, 0.f);
                    split2(r.x, r.y, keep_hi[s_][j].x, keep_lo[s_][j].x); split2(r.z, r.w, keep_hi[s_][j].y, keep_lo[s_][j].y);
                } else {
                    float4 mv = val;                              // (the narrow branch of epi_tile, step for step)
                    if constexpr (DG) {
                        const uint32_t nib = mw1[s_][j] >> c4;
                        mv.x = (nib & 1u) ? mv.x : 0.0f; mv.y = (nib & 2u) ? mv.y : 0.0f; mv.z = (nib & 4u) ? mv.z : 0.0f; mv.w = (nib & 8u) ? mv.w : 0.0f;
                    }
                    uint2 pk = f4_to_bf4(mv);                     // the one rounding of the stored map
                    if (wmap && own) *(uint2*)((bf16_t*)p1.epi.out_raw + opix * 32 + c4) = pk;
                    if constexpr (DG) {                           // the SUM output: what the second layer reads
                        const float4 a = bf4_to_f4(a1v[s_][j]);
                        mv.x += a.x; mv.y += a.y; mv.z += a.z; mv.w += a.w;
                        pk = f4_to_bf4(mv);
                        if (p1.epi.out_sum && own) *(uint2*)((bf16_t*)p1.epi.out_sum + opix * 32 + c4) = pk;
                    }
                    if constexpr (RELU) { pk.x = relu_pk(pk.x); pk.y = relu_pk(pk.y); }
                    if (!inimg) pk = make_uint2(0u, 0u);
                    keep_hi[s_][j] = pk;
                }
            }
        }
        lap(dPh1);
        lds_barrier();                                            // every wave is done with the window and the weights: the region becomes the halo tile
        lap(dBar1);
#pragma unroll
        for (int s_ = 0; s_ < NGC; ++s_) {
            const int code = (int)((sched >> (4 * s_)) & 15u);
            const bool yo = code & 8, xo = code & 4;
            const int gi = code & 3;
            const int tq = (i & 3) + 4 * h, c4 = 4 * (i >> 2);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int qq = 32 * gi + 8 * j + tq, qc = min(qq, NQ - 1);
                const int rr = qc / NC, jj = qc - rr * NC;
                const int row = 2 * rr + (yo ? 0 : 1), col = 2 * jj + (xo ? 0 : 1);
                unsigned char* dst = lds + (row * X3_PW + col) * STR + 2 * c4;
                if (qq < NQ) {
                    *(uint2*)dst = keep_hi[s_][j];
                    if constexpr (F32) *(uint2*)(dst + Geo<T>::LO) = keep_lo[s_][j];
                }
            }
        }
        // the next tile's window flies during the second convolution.  APRE: behind row 0's addends, and UNCONDITIONAL (a block's last tile
        // fetches its own window again, from L2) -- behind a conditional prefetch the wait for the addends would have to be vmcnt(0)
        float4 ad[APRE ? 8 : 1];
        if constexpr (APRE) {
            epi_add_loads(p2.epi, b, y0 + 2 * wave, H, W, i, x0, h, ad);
            issue_loads(tile + gridDim.x < ntiles ? tile + gridDim.x : tile);
        } else {
            if (tile + gridDim.x < ntiles) issue_loads(tile + gridDim.x);
        }
        lap(dHalo);
        lds_barrier();
        lap(dBar2);

        // ---- phase 2: the body of the stride-1 kernel on the LDS tile, TH / 4 output rows per wave ----
        auto do_row = [&](const int row) __attribute__((always_inline)) {
            const int y = y0 + row;
            if (y >= H) return;                                   // wave-uniform
            if constexpr (APRE) { if (row & 1) epi_add_loads(p2.epi, b, y, H, W, i, x0, h, ad); }       // (row 0's: in front of the prefetch, above)
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            {
                // fragment reads AHEAD steps in front of their MFMAs, the order fixed by scheduling barriers (conv32_s1_x3_kernel)
                constexpr int AHEAD = F32 ? 1 : (DG ? 2 : 4), RING = AHEAD + 1;
                const unsigned char* const arow = lds + (row * X3_PW + i) * STR + 16 * h;
                const unsigned char* const wrow = wl_lds + lane * 16;
                uint4 fah[RING], fal[F32 ? RING : 1], fbl[LO ? RING : 1];
                auto frag_load = [&](const int n_) __attribute__((always_inline)) {
                    const unsigned char* a = arow + ((n_ / 6) * X3_PW + (n_ / 2) % 3) * STR + 32 * (n_ & 1);
                    fah[n_ % RING] = *(const uint4*)a;
                    if constexpr (F32) fal[n_ % RING] = *(const uint4*)(a + Geo<T>::LO);
                    if constexpr (LO) fbl[n_ % RING] = *(const uint4*)(wrow + n_ * 1024);
                };
#pragma unroll
                for (int s_ = 0; s_ < AHEAD; ++s_) frag_load(s_);
#pragma unroll
                for (int s_ = 0; s_ < 18; ++s_) {
                    if (s_ + AHEAD < 18) frag_load(s_ + AHEAD);
                    __builtin_amdgcn_sched_barrier(0);
                    const bf16x8 ah = __builtin_bit_cast(bf16x8, fah[s_ % RING]), bh = __builtin_bit_cast(bf16x8, wh[s_ >> 1][s_ & 1]);
                    if constexpr (F32) {
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fal[s_ % RING]), bh, acc, 0, 0, 0);   // small terms first
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, __builtin_bit_cast(bf16x8, fbl[s_ % RING]), acc, 0, 0, 0);
                    } else if constexpr (DG) {
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, __builtin_bit_cast(bf16x8, fbl[s_ % RING]), acc, 0, 0, 0);
                    }
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if constexpr (APRE) {
                // (the addends are first USED here: left visible, their sum is computed in front of the MFMAs -- eight registers fewer -- and
                // the row waits for the round trip before its matrix work instead of behind it)
#pragma unroll
                for (int g = 0; g < 8; ++g) asm volatile("" : "+v"(ad[g].x), "+v"(ad[g].y), "+v"(ad[g].z), "+v"(ad[g].w));
            }
            lap(dMfma);
            epi_tile<T, false, DG, ADD>(p2.epi, b, y, H, W, i, acc, x0, h, W, 1, 0, sy, sx, nullptr, 0, 0, &bias2, nullptr, APRE ? ad : nullptr);
            lap(dEpi);
        };
        if constexpr (APRE) {
            // (the two rows as straight-line code: inside a loop the wait-count bookkeeping merges with the back edge and the wait for row 0's
            // addends becomes vmcnt(0), that is for the prefetch issued behind them -- conv32_s1_x3_kernel's masked variants)
            do_row(2 * wave); do_row(2 * wave + 1);
        } else if constexpr (TH == 8) {
#pragma unroll 1
            for (int rr = 0; rr < 2; ++rr) do_row(2 * wave + rr);
        } else {
            do_row(wave);
        }
        lds_barrier();          // LDS reuse by the next tile's window only: this tile's stores and the prefetch stay in flight
        lap(dBar3);
        ++ntl;
    }
    if constexpr (TIMING) {
        PTTA_STAMP(tn);
        if ((blockIdx.x == 102 || blockIdx.x == 307) && lane == 0 && ntl > 0)
            printf("tpair blk %d wave %d tiles %d: life %llu pro %u | per tile: stage %u w1wait %u bar0 %u phase1 %u bar1 %u halo+issue %u bar2 %u mfma2 %u epilogue2 %u bar3 %u\n",
                   (int)blockIdx.x, wave, ntl, tn - T0, dPro, dStage / ntl, dW1 / ntl, dBar0 / ntl, dPh1 / ntl, dBar1 / ntl, dHalo / ntl, dBar2 / ntl,
                   dMfma / ntl, dEpi / ntl, dBar3 / ntl);
    }
}

template <typename T>
static int launch_tpair_t(const Conv32Args& f, const Conv32Args& g, int form, int max_blocks, hipStream_t s) {
    const int Hm = f.Hin * 2, Wm = f.Win * 2;
    const Conv32P<T> p1 = conv32_params<T>(f, Hm, Wm), p2 = conv32_params<T>(g, Hm, Wm);
    if (form == 0) form = conv32_s1_small_map(g.B, Hm, Wm) ? 1 : 2;      // as the stride-1 launch would choose its kernel
    // the persistent form's workgroups: the stride-1 kernel's share of the two-per-CU slots (conv32_launch.h kS1PersistentBlocks)
    long blocks = form == 2 ? conv32_grid(conv32_tiles(g.B, Hm, Wm, X3_TH), kS1PersistentBlocks) : conv32_grid(conv32_tiles(g.B, Hm, Wm, X3S_TH), kS1SmallBlocks);
    if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
    if constexpr (sizeof(T) == 2) {
        if (f.w2) {            // the data gradients' form
            if (form == 2) hipLaunchKernelGGL((conv32_tpair_kernel<T, 8, false, true>), dim3((unsigned)blocks), dim3(256), 0, s, p1, p2);
            else hipLaunchKernelGGL((conv32_tpair_kernel<T, 4, false, true>), dim3((unsigned)blocks), dim3(256), 0, s, p1, p2);
            PTTA_CHECK_LAUNCH();
            return 0;
        }
    }
#ifdef PTTA_DIAG_STAMPS      // diagnostic build (make DIAG=1): in-kernel phase stamps of the fp32 persistent form with addends
    if constexpr (sizeof(T) == 4) {
        if (form == 2 && g.add1) {
            hipLaunchKernelGGL((conv32_tpair_kernel<T, 8, true, false, true>), dim3((unsigned)blocks), dim3(256), 0, s, p1, p2);
            PTTA_CHECK_LAUNCH();
            return 0;
        }
    }
#endif
    with_flag(g.add1 != nullptr, [&](auto ADD) {
        if (form == 2) hipLaunchKernelGGL((conv32_tpair_kernel<T, 8, decltype(ADD)::value>), dim3((unsigned)blocks), dim3(256), 0, s, p1, p2);
        else hipLaunchKernelGGL((conv32_tpair_kernel<T, 4, decltype(ADD)::value>), dim3((unsigned)blocks), dim3(256), 0, s, p1, p2);
    });
    PTTA_CHECK_LAUNCH();
    return 0;
}

// `first` (CONV_T2) and `second` (CONV_S1) as for two ptta_launch_conv32 calls; second.in is ignored (the intermediate stays on chip) and
// first.out_raw may be null: the map is then not written at all (its sign-bit words still are).  ptta_conv32_tpair_applies: the pair is
// one of the instantiated forms; the launch returns 1 when it is not (the caller then issues the two launches).
// form: 0 = by the map size as the stride-1 launch would choose its kernel, 1 = 4 x 32 tiles, 2 = persistent 8 x 32 tiles;
// max_blocks > 0 caps the grid (a block then walks several tiles).
bool ptta_conv32_tpair_applies(const Conv32Args& first, const Conv32Args& second) {
    const Conv32Args &f = first, &g = second;
    if (f.mode != CONV_T2 || !conv32_pair_common(f, g)) return false;
    if (!f.w2 && (g.up || (g.add1 && !g.out_sum))) return false;       // the forward's second half: no bilinear skip; addends go to the sum output
    const int Hm = f.Hin * 2, Wm = f.Win * 2;
    return f.Hin >= 1 && f.Win >= 1 && g.Hin == Hm && g.Win == Wm && g.B == f.B && f.B >= 1;
}
// ... and it is faster in the step than the two launches (asked with form 0 only: the caller did not name a form).  The forward's form at
// every size.  The data gradients' form only where no block walks more than one tile: it fetches the first layer's 36 KB of fragments for
// every tile, as much as a narrow tile's own traffic, and behind the previous tile's stores.  Measured in the headline step (MI355X, batch 1,
// profiles/tpair_fusion_ab.txt): the 1/4- and 1/2-resolution pairs (110 and 418 tiles) 11.2 + 8.8 -> 16.3, 17.0 + 13.4 -> 32.2 and
// 16.0 + 13.4 -> 30.3 us launch by launch and 1.1453 -> 1.1391 ms per step together; the full-resolution pair (1672 tiles, 3.5 per block)
// 28.2 + 26.2 -> 80.2 us and 1.139 -> 1.178 ms per step: back to two launches.
bool ptta_conv32_tpair_pays(const Conv32Args& first, const Conv32Args& second) {
    if (!first.w2) return true;
    const int Hm = first.Hin * 2, Wm = first.Win * 2;
    return conv32_tiles(second.B, Hm, Wm, X3_TH) <= kS1PersistentBlocks;
}
int ptta_launch_conv32_tpair(const Conv32Args& first, const Conv32Args& second, int form, int max_blocks, hipStream_t s) {
    if (form < 0 || form > 2 || !ptta_conv32_tpair_applies(first, second)) return 1;
    if (form == 0 && !ptta_conv32_tpair_pays(first, second)) return 1;
    return first.bf16 ? launch_tpair_t<bf16_t>(first, second, form, max_blocks, s) : launch_tpair_t<float>(first, second, form, max_blocks, s);
}
