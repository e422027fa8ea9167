// The LDS-staged forms of the 3x3 32 -> 32 convolution: stride 1 as persistent 8 x 32 tiles and as one 4 x 32 tile per block (small maps),
// and stride 2.  Which form a launch takes, and its grid: conv32.hip ptta_launch_conv32.
// (conv32_s2_lds_kernel stands here and not beside the other stride-2 kernel: hipcc gives it the same machine code as before the file was
// split only in one translation unit with conv32_s1_x3_kernel, with which it shares load_weights -- profiles/conv32_split_isa.txt.)
#include "conv32_launch.h"

// ---- stride-1, LDS-staged -------------------------------------------------------------------------------------------------
// A block owns an 8x32 output tile: the (8+2)x(32+2) input halo is read from HBM once (full NHWC lines), ReLU'd and split ONCE while it is
// staged into LDS.  Each wave computes two 32-pixel rows; the hi weight fragments (72 VGPRs) stay in registers across the persistent tile
// loop, the lo fragments (fp32 storage) in LDS.  Without the bilinear epilogue the NEXT tile's global loads are issued before this tile's
// MFMAs and land while the matrix cores work (software prefetch across the persistent tile loop).
// TIMING (make DIAG=1 only): s_memtime stamps around the phases of the tile loop, printed by two blocks of the launch
template <typename T, bool RELU, bool UP, bool MASK, bool ADD, bool W2 = false, bool TIMING = false>
__global__ __launch_bounds__(256, 2) void conv32_s1_x3_kernel(Conv32P<T> p) {
    unsigned long long T0 = 0, ta = 0, tb = 0, tc = 0, td = 0, te = 0, tf = 0, tg = 0, th = 0;
    unsigned long long dWait = 0, dSplit = 0, dIssue = 0, dBar1 = 0, dMfma = 0, dEpi = 0, dBar2 = 0, dPro = 0;
    int ntl = 0;
    PTTA_STAMP(T0);
    constexpr int STR = Geo<T>::STR, WL = (sizeof(T) == 4 || W2) ? 18 * 64 * 16 : 0;
    constexpr int UPH = 6, UPW = 18;                      // an 8x32 output tile reads <= 5x17 source pixels
    __shared__ __attribute__((aligned(16))) unsigned char lds[X3_PH * X3_PW * STR + WL + (UP ? UPH * UPW * Geo<T>::UPPX : 0)];
    unsigned char* const wl_lds = lds + X3_PH * X3_PW * STR;
    unsigned char* const up_lds = wl_lds + WL;
    const int tid = threadIdx.x, lane = tid & 63;
    const int i = lane & 31, h = lane >> 5;
    const float biasv = epi_bias(p.epi, i);               // once per kernel: ptta_common.h epi_tile
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = p.Hout, W = p.Wout;
    const int ntx = (W + 31) >> 5, nty = (H + X3_TH - 1) / X3_TH;
    const long ntiles = (long)p.B * ntx * nty;
    const float sy = up_scale(H >> 1, H), sx = up_scale(W >> 1, W);

    constexpr int NIT = (((X3_PH * X3_PW + 7) / 8) * 32 + 255) / 256;     // (pixel, 8-channel group) staging items per thread
    constexpr bool PREFETCH = !UP;       // (the bilinear epilogue leaves no registers for it: 13 spills and no gain when forced)
    Px<T> v[NIT];
    auto issue_loads = [&](long tile) {
        int b, y0, x0;
        tile_coords<X3_TH>(tile, ntx, nty, b, y0, x0);
        const T* inb = p.in + (size_t)(b % p.in_nb) * H * W * 32;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = tid + 256 * it;
            const int g = idx & 3, pix = x3_stage_pix(idx);
            const int py = pix / X3_PW, px = pix - py * X3_PW;
            const int gy = y0 - 1 + py, gx = x0 - 1 + px;
            v[it] = px_zero<T>();
            if (pix < X3_PH * X3_PW && gy >= 0 && gy < H && gx >= 0 && gx < W) v[it] = px_load(inb + ((size_t)gy * W + gx) * 32 + 8 * g);
        }
    };
    if (PREFETCH && blockIdx.x < ntiles) issue_loads(blockIdx.x);
    // weight fragments: loaded AFTER the first tile's loads were issued so that the two L2 round trips overlap
    uint4 wh[9][2];
    load_weights<T, W2>(wh, wl_lds, p.wpack, p.wpack2, tid, lane);
    PTTA_STAMP(ta); dPro = ta - T0;

    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int b, y0, x0;
        tile_coords<X3_TH>(tile, ntx, nty, b, y0, x0);
        int uy0 = 0, ux0 = 0;
        PTTA_STAMP(ta);
        if constexpr (TIMING) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
        PTTA_STAMP(tb);
        if (UP) {
            // issued FIRST so that it flies while this tile's halo is split and written; drained before the next tile's register prefetch
            // is issued (vmcnt is in order: a later wait for the window would also wait for that prefetch)
            const int Hu = H >> 1, Wu = W >> 1;
            uy0 = lerp_coef(y0, Hu, sy).i0; ux0 = lerp_coef(x0, Wu, sx).i0;
            up_window_dma<T, UPH, UPW>(p.epi.up + (size_t)(b % p.epi.up_nb) * Hu * Wu * 32, Hu, Wu, uy0, ux0, up_lds, tid, wave);
        }
        if (!PREFETCH) issue_loads(tile);
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = tid + 256 * it;
            const int pix = x3_stage_pix(idx);
            if (pix < X3_PH * X3_PW) px_stage<RELU>(v[it], lds + pix * STR + 16 * (idx & 3), Geo<T>::LO);
        }
        PTTA_STAMP(tc);
        if (UP) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the window has landed (and this tile's halo loads before it)
        // narrow masked epilogue: both rows' mask words are requested BEFORE the next tile's prefetch (ptta_common.h epi_mask_words)
        constexpr bool MWPRE = MASK && sizeof(T) == 2;
        uint32_t mwp0[4], mwp1[4];         // (two arrays and a select below: the row loop is not unrolled, an array indexed by the row lives in scratch)
        if constexpr (MWPRE) {
            epi_mask_words<T>(p.epi, b, y0 + 2 * wave, H, W, i, x0, h, mwp0);
            epi_mask_words<T>(p.epi, b, y0 + 2 * wave + 1, H, W, i, x0, h, mwp1);
        }
        if (PREFETCH && tile + gridDim.x < ntiles) issue_loads(tile + gridDim.x);
        PTTA_STAMP(td);
        lds_barrier();          // LDS-only: the next tile's global loads (issued above) stay in flight during the MFMAs
        PTTA_STAMP(te);
        // ---- two output rows per wave ------------------------------------------------------------
        auto do_row = [&](const int rr) __attribute__((always_inline)) {
            const int row = 2 * wave + rr;
            const int y = y0 + row;
            if (y >= H) return;                                     // wave-uniform
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            // The fragment reads run AHEAD steps in front of their MFMAs (one step = the (tap, k) pair's reads and products).  Left to hipcc each
            // ds_read_b128 is issued right in front of the MFMA that consumes it, behind s_waitcnt lgkmcnt(0): the LDS latency exposed every two or
            // three matrix instructions, 65 - 75 cycles per MFMA instead of 32 (in-kernel stamps, round 6: the MFMA phase was 7 - 8 k of a tile's
            // 14 k cycles).  The order is fixed by scheduling barriers around each step; the waits are the compiler's own counted lgkmcnt.
            {
                constexpr int AHEAD = sizeof(T) == 4 ? 1 : (W2 ? 2 : 4), RING = AHEAD + 1;
                const unsigned char* const arow = lds + (row * X3_PW + i) * STR + 16 * h;
                const unsigned char* const wrow = wl_lds + lane * 16;
                FragSet<T, W2> fr[RING];
#pragma unroll
                for (int s_ = 0; s_ < AHEAD; ++s_) frag_load<T, W2>(fr[s_], arow + ((s_ / 6) * X3_PW + (s_ / 2) % 3) * STR + 32 * (s_ & 1), wrow + s_ * 1024);
#pragma unroll
                for (int s_ = 0; s_ < 18; ++s_) {
                    if (s_ + AHEAD < 18) {
                        const int n_ = s_ + AHEAD;
                        frag_load<T, W2>(fr[n_ % RING], arow + ((n_ / 6) * X3_PW + (n_ / 2) % 3) * STR + 32 * (n_ & 1), wrow + n_ * 1024);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    frag_mma<T, W2>(acc, fr[s_ % RING], wh[s_ >> 1][s_ & 1]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if constexpr (TIMING) { PTTA_STAMP(tf); dMfma += tf - (rr ? tg : te); }
            // (conv + bias) + bilinear, in the reference's order; the skip comes from the LDS window, added after the quad transpose
            if (UP) epi_tile<T, false, MASK, ADD, true, UPW>(p.epi, b, y, H, W, i, acc, x0, h, W, 1, 0, sy, sx, up_lds, uy0, ux0, &biasv);
            else {
                uint32_t mws[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) mws[g] = MWPRE ? (rr ? mwp1[g] : mwp0[g]) : 0u;
                epi_tile<T, false, MASK, ADD>(p.epi, b, y, H, W, i, acc, x0, h, W, 1, 0, sy, sx, nullptr, 0, 0, &biasv, MWPRE ? mws : nullptr);
            }
            if constexpr (TIMING) { PTTA_STAMP(tg); dEpi += tg - tf; }
        };
        // (narrow masked variants: the two rows as straight-line code -- inside a loop the compiler's wait-count bookkeeping merges with the
        // back edge and waits vmcnt(0) for the preloaded mask words, i.e. for the prefetch issued behind them)
        if constexpr (MWPRE) { do_row(0); do_row(1); }
        else {
#pragma unroll 1
            for (int rr = 0; rr < 2; ++rr) do_row(rr);
        }
        lds_barrier();          // LDS reuse only: do not wait for this tile's stores (nor the prefetch) to drain
        if constexpr (TIMING) { PTTA_STAMP(th); dWait += tb - ta; dSplit += tc - tb; dIssue += td - tc; dBar1 += te - td; dBar2 += th - tg; ++ntl; }
    }
    if constexpr (TIMING) {
        PTTA_STAMP(th);
        if (wave == 0 && lane == 0 && (blockIdx.x < 20 || (blockIdx.x >= 256 && blockIdx.x < 276))) {
            unsigned hwid, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            printf("x3map blk %d xcc %u se %u sh %u cu %u simd %u waveslot %u\n", (int)blockIdx.x, xcc & 15, (hwid >> 13) & 7, (hwid >> 12) & 1, (hwid >> 8) & 15, (hwid >> 4) & 3, hwid & 15);
        }
        if ((blockIdx.x == 102 || blockIdx.x == 307) && lane == 0 && ntl > 0)
            printf("x3 blk %d wave %d tiles %d: life %llu pro %llu | per tile: vmwait %llu split+write %llu issue %llu barrier1 %llu mfma %llu epilogue %llu barrier2 %llu\n",
                   (int)blockIdx.x, wave, ntl, th - T0, dPro, dWait / ntl, dSplit / ntl, dIssue / ntl, dBar1 / ntl, dMfma / ntl, dEpi / ntl, dBar2 / ntl);
    }
}

// ---- the same convolution for SMALL maps (at most ~256 tiles of 8x32: the 1/4 ... 1/16-resolution layers, 18 launches of a step) ----
// Those launches are one tile per block and their duration is a latency chain, not bandwidth (in-kernel stamps of the kernel above on a
// one-tile launch: 26k cycles = weights -> LDS 5.9k + first loads 3.7k + split 2.6k + 108 MFMAs with LDS-fed lo fragments 6.1k + epilogue
// 2.6k).  This form shortens the chain: a 4x32 tile (one output row per wave: twice the blocks -- the chip is mostly idle at these sizes),
// EVERY weight fragment in registers (fp32 storage: hi and lo, 144 VGPRs: no global -> LDS -> barrier hop for the lo half), every global
// load of the block -- halo, weight fragments, bilinear window -- issued before the first wait.  Same products in the same order as
// conv32_s1_x3_kernel: bit-identical outputs.
template <typename T, bool RELU, bool UP, bool MASK, bool ADD, bool W2 = false>
__global__ __launch_bounds__(256, 1) void conv32_s1_small_kernel(Conv32P<T> p) {
    constexpr int STR = Geo<T>::STR;
    constexpr bool F32 = sizeof(T) == 4;
    constexpr int UPH = 4, UPW = 18;                      // a 4x32 output tile reads <= 3x17 source pixels of the half-resolution map
    __shared__ __attribute__((aligned(16))) unsigned char lds[X3S_PH * X3_PW * STR + (UP ? UPH * UPW * Geo<T>::UPPX : 0)];
    unsigned char* const up_lds = lds + X3S_PH * X3_PW * STR;
    const int tid = threadIdx.x, lane = tid & 63;
    const int i = lane & 31, h = lane >> 5;
    const float biasv = epi_bias(p.epi, i);               // once per kernel: ptta_common.h epi_tile
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = p.Hout, W = p.Wout;
    const int ntx = (W + 31) >> 5, nty = (H + X3S_TH - 1) / X3S_TH;
    const int ntiles = p.B * ntx * nty;
    const float sy = up_scale(H >> 1, H), sx = up_scale(W >> 1, W);
    constexpr int NPIX = X3S_PH * X3_PW;                  // 204 halo pixels
    constexpr int NIT = (((NPIX + 7) / 8) * 32 + 255) / 256;      // (pixel, 8-channel group) items per thread
    bool wloaded = false;
    uint4 wh[9][2], wl[(F32 || W2) ? 9 : 1][2];
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int ty = tile % nty, tx = (tile / nty) % ntx, b = tile / (nty * ntx);
        const int y0 = ty * X3S_TH, x0 = tx << 5;
        const T* inb = p.in + (size_t)(b % p.in_nb) * H * W * 32;
        // UNCONDITIONAL loads from clamped addresses, zero-filled at staging time: behind `if (inside) v = load` hipcc waited vmcnt(0) at the
        // join of every one of the four branches (the select with the zero needs the value) -- four L2 round trips in a row in a kernel whose
        // whole duration is a latency chain (round 5, .s)
        Px<T> v[NIT];
        bool vok[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = tid + 256 * it;
            const int g = idx & 3, pix = x3_stage_pix(idx);
            const int py = pix / X3_PW, px = pix - py * X3_PW;
            const int gy = y0 - 1 + py, gx = x0 - 1 + px;
            vok[it] = pix < NPIX && gy >= 0 && gy < H && gx >= 0 && gx < W;
            v[it] = px_load(inb + ((size_t)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1)) * 32 + 8 * g);
        }
        if (!wloaded) {                                   // block-uniform; in flight together with the halo
            const uint4* ph = (const uint4*)p.wpack;
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int k = 0; k < 2; ++k) wh[t][k] = ph[(t * 2 + k) * 64 + lane];
            if constexpr (F32 || W2) {
                const uint4* pl = (const uint4*)p.wpack2;
#pragma unroll
                for (int t = 0; t < 9; ++t)
#pragma unroll
                    for (int k = 0; k < 2; ++k) wl[t][k] = pl[(t * 2 + k) * 64 + lane];
            }
            wloaded = true;
        }
        int uy0 = 0, ux0 = 0;
        if (UP) {
            const int Hu = H >> 1, Wu = W >> 1;
            uy0 = lerp_coef(y0, Hu, sy).i0; ux0 = lerp_coef(x0, Wu, sx).i0;
            const T* ub = p.epi.up + (size_t)(b % p.epi.up_nb) * Hu * Wu * 32;
            constexpr int PC = Geo<T>::UPPC;
            for (int idx = tid; idx < UPH * UPW * PC; idx += 256) {
                const int q = idx % PC, pix = idx / PC;
                const int r = pix / UPW, cc = pix - r * UPW;
                const int gy = min(uy0 + r, Hu - 1), gx = min(ux0 + cc, Wu - 1);
                *(uint4*)(up_lds + (size_t)idx * 16) = *(const uint4*)(ub + ((size_t)gy * Wu + gx) * 32 + (32 / PC) * q);
            }
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = tid + 256 * it;
            const int pix = x3_stage_pix(idx);
            if (!vok[it]) v[it] = px_zero<T>();
            if (pix < NPIX) px_stage<RELU>(v[it], lds + pix * STR + 16 * (idx & 3), Geo<T>::LO);
        }
        lds_barrier();
        const int y = y0 + wave;
        if (y < H) {                                      // wave-uniform
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int ky = tap / 3, kx = tap % 3;
                const unsigned char* a = lds + ((wave + ky) * X3_PW + i + kx) * STR + 16 * h;
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const bf16x8 ah = __builtin_bit_cast(bf16x8, *(const uint4*)(a + 32 * k));
                    const bf16x8 bh = __builtin_bit_cast(bf16x8, wh[tap][k]);
                    if constexpr (F32) {
                        const bf16x8 al = __builtin_bit_cast(bf16x8, *(const uint4*)(a + 32 * k + 64));
                        const bf16x8 bl = __builtin_bit_cast(bf16x8, wl[tap][k]);
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);   // small terms first (as conv32_s1_x3_kernel)
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
                    } else if constexpr (W2) {
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, __builtin_bit_cast(bf16x8, wl[tap][k]), acc, 0, 0, 0);
                    }
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
                }
            }
            if (UP) epi_tile<T, false, MASK, ADD, true, UPW>(p.epi, b, y, H, W, i, acc, x0, h, W, 1, 0, sy, sx, up_lds, uy0, ux0, &biasv);
            else epi_tile<T, false, MASK, ADD>(p.epi, b, y, H, W, i, acc, x0, h, W, 1, 0, sy, sx, nullptr, 0, 0, &biasv);
        }
        if (tile + (int)gridDim.x < ntiles) lds_barrier();   // LDS reuse by the next tile
    }
}


// ---- stride-2 convolution, LDS-staged: the (2*4+1) x (2*32+1) input window of a 4 x 32 output tile is read
// ONCE as whole pixel lines (every input pixel crosses the vector-memory path 1.14 times) instead of as
// per-tap fragment loads (1.8 times, a quarter of every line touched per instruction).  Same structure as the stride-1
// kernel with two differences: the K loop is split into the two 16-channel k-steps (the window of all 32 channels would not fit
// two blocks per CU in fp32 storage), and a wave owns one output row whose A fragments are read from LDS with a two-pixel stride.
// Accumulation order: k-step outer, tap inner.  The next stage's loads are issued before the current stage's MFMAs (one register set; a
// two-set ring with loads two stages ahead needed 254-256 VGPRs, spilled in the mask / add variants and measured slower:
// 34.4 vs 33.7 us at full resolution, 9.9 vs 8.8 us at 1/8).
#define S2_PH (2 * S2_TH + 1)
#define S2_PW 65
#define S2_STR 80                                      // per pixel and k-step: hi 32 B | lo 32 B (fp32 storage) | pad 16 B
template <typename T, bool RELU, bool MASK, bool ADD, bool W2 = false>
__global__ __launch_bounds__(256, 2) void conv32_s2_lds_kernel(Conv32P<T> p) {
    constexpr bool F32 = sizeof(T) == 4;
    constexpr int NPIX = S2_PH * S2_PW, NIT = (NPIX * 2 + 255) / 256;
    constexpr int WL = (F32 || W2) ? 18 * 64 * 16 : 0;
    constexpr int STR = F32 ? S2_STR : 48;                          // narrow: hi 32 B | pad 16 B per pixel and k-step (three blocks per CU)
    __shared__ __attribute__((aligned(16))) unsigned char lds[NPIX * STR + WL + 16];
    unsigned char* const wl_lds = lds + NPIX * STR;
    const int tid = threadIdx.x, lane = tid & 63;
    const int i = lane & 31, h = lane >> 5;
    const float biasv = epi_bias(p.epi, i);               // once per kernel: ptta_common.h epi_tile
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Hin = p.Hin, Win = p.Win, Ho = p.Hout, Wo = p.Wout;
    const int ntx = (Wo + 31) >> 5, nty = (Ho + S2_TH - 1) / S2_TH;
    const long nstages = 2L * p.B * ntx * nty;                      // (tile, k-step) pairs
    Px<T> v[NIT];
    auto coords = [&](long tile, int& b, int& oy0, int& ox0) {
        long t_ = tile;
        const int ty = (int)(t_ % nty); t_ /= nty;
        const int tx = (int)(t_ % ntx);
        b = (int)(t_ / ntx); oy0 = ty * S2_TH; ox0 = tx << 5;
    };
    auto issue_loads = [&](long stage) {
        int b, oy0, ox0;
        coords(stage >> 1, b, oy0, ox0);
        const T* inb = p.in + (size_t)(b % p.in_nb) * Hin * Win * 32 + 16 * (int)(stage & 1);
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = tid + 256 * it;
            const int g = idx & 1, pix = idx >> 1;
            const int py = pix / S2_PW, px = pix - py * S2_PW;
            const int gy = 2 * oy0 - 1 + py, gx = 2 * ox0 - 1 + px;
            v[it] = px_zero<T>();
            if (pix < NPIX && gy >= 0 && gy < Hin && gx >= 0 && gx < Win) v[it] = px_load(inb + ((size_t)gy * Win + gx) * 32 + 8 * g);
        }
    };
    const long first = 2L * blockIdx.x, sstride = 2L * gridDim.x;       // this block's stages: 2t, 2t+1 of its tiles
    if (first < nstages) issue_loads(first);
    uint4 wh[9][2];
    load_weights<T, W2>(wh, wl_lds, p.wpack, p.wpack2, tid, lane);
    f32x16 acc;
    bool started = false;
    for (long base = first; base < nstages; base += sstride) {
        int b, oy0, ox0;
        coords(base >> 1, b, oy0, ox0);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if (started) lds_barrier();                  // the previous stage's MFMAs are done with the window
            started = true;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int idx = tid + 256 * it;
                const int pix = idx >> 1;
                if (pix < NPIX) px_stage<RELU>(v[it], lds + pix * STR + 16 * (idx & 1), 32);
            }
            {   // next stage's loads: the other k-step of this tile, or the first k-step of the block's next tile
                const long nxt = q == 0 ? base + 1 : base + sstride;
                if (nxt < nstages) issue_loads(nxt);
            }
            lds_barrier();                               // LDS-only: the loads just issued stay in flight during the MFMAs
            if (q == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            }
            if (oy0 + wave < Ho) {                       // wave-uniform
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int ky = tap / 3, kx = tap % 3;
                    const unsigned char* a = lds + ((2 * wave + ky) * S2_PW + 2 * i + kx) * STR + 16 * h;
                    const bf16x8 ah = __builtin_bit_cast(bf16x8, *(const uint4*)a);
                    const bf16x8 bh = __builtin_bit_cast(bf16x8, wh[tap][q]);
                    if constexpr (F32) {
                        const bf16x8 al = __builtin_bit_cast(bf16x8, *(const uint4*)(a + 32));
                        const bf16x8 bl = __builtin_bit_cast(bf16x8, *(const uint4*)(wl_lds + ((tap * 2 + q) * 64 + lane) * 16));
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);   // small terms first
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
                    } else if constexpr (W2) {
                        const bf16x8 bl = __builtin_bit_cast(bf16x8, *(const uint4*)(wl_lds + ((tap * 2 + q) * 64 + lane) * 16));
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
                    }
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
                }
                if (q == 1) epi_tile<T, false, MASK, ADD>(p.epi, b, oy0 + wave, Ho, Wo, i, acc, ox0, h, Wo, 1, 0, 0.f, 0.f, nullptr, 0, 0, &biasv);
            }
        }
    }
}


// ---- host entries (conv32_launch.h): the epilogue flags and ReLU on load -> kernel instance ----
template <typename T>
static int launch_s1_x3_t(const Conv32P<T>& p, int flags, bool relu, bool w2, int blocks, hipStream_t s) {
    if (w2 && (relu || sizeof(T) != 2)) return -22;
    with_flags(flags, relu, [&](auto U, auto M, auto A, auto R) {
        constexpr bool u = decltype(U)::value, m = decltype(M)::value, a = decltype(A)::value, r = decltype(R)::value;
        if constexpr (sizeof(T) == 2 && !r) {              // hi + lo weights: narrow storage, no ReLU on load (the data gradients)
            if (w2) { hipLaunchKernelGGL((conv32_s1_x3_kernel<T, false, u, m, a, true>), dim3(blocks), dim3(256), 0, s, p); return; }
        }
#ifdef PTTA_DIAG_STAMPS      // diagnostic build (make DIAG=1): in-kernel phase stamps of the plain launches (tools/bench_chain.py prints them)
        if constexpr (!u && !m && !a && r) {
            if (!w2) { hipLaunchKernelGGL((conv32_s1_x3_kernel<T, true, false, false, false, false, true>), dim3(blocks), dim3(256), 0, s, p); return; }
        }
#endif
        hipLaunchKernelGGL((conv32_s1_x3_kernel<T, r, u, m, a>), dim3(blocks), dim3(256), 0, s, p);
    });
    PTTA_CHECK_LAUNCH();
    return 0;
}
template <typename T>
static int launch_s1_small_t(const Conv32P<T>& p, int flags, bool relu, bool w2, int blocks, hipStream_t s) {
    if (w2 && (relu || sizeof(T) != 2)) return -22;
    with_flags(flags, relu, [&](auto U, auto M, auto A, auto R) {
        constexpr bool u = decltype(U)::value, m = decltype(M)::value, a = decltype(A)::value, r = decltype(R)::value;
        if constexpr (sizeof(T) == 2 && !r) {              // hi + lo weights: as above
            if (w2) { hipLaunchKernelGGL((conv32_s1_small_kernel<T, false, u, m, a, true>), dim3(blocks), dim3(256), 0, s, p); return; }
        }
        hipLaunchKernelGGL((conv32_s1_small_kernel<T, r, u, m, a>), dim3(blocks), dim3(256), 0, s, p);
    });
    PTTA_CHECK_LAUNCH();
    return 0;
}
int conv32_launch_s1_x3(const Conv32P<float>& p, int flags, bool relu, bool w2, int blocks, hipStream_t s) { return launch_s1_x3_t(p, flags, relu, false, blocks, s); }
int conv32_launch_s1_x3(const Conv32P<bf16_t>& p, int flags, bool relu, bool w2, int blocks, hipStream_t s) { return launch_s1_x3_t(p, flags, relu, w2, blocks, s); }
int conv32_launch_s1_small(const Conv32P<float>& p, int flags, bool relu, bool w2, int blocks, hipStream_t s) { return launch_s1_small_t(p, flags, relu, false, blocks, s); }
int conv32_launch_s1_small(const Conv32P<bf16_t>& p, int flags, bool relu, bool w2, int blocks, hipStream_t s) { return launch_s1_small_t(p, flags, relu, w2, blocks, s); }
template <typename T>
static int launch_s2_lds(const Conv32P<T>& p, int flags, bool relu, bool w2, int blocks, hipStream_t s) {
    if ((flags & 1) || (w2 && (relu || sizeof(T) != 2))) return -22;
    with_flags(flags, relu, [&](auto U, auto M, auto A, auto R) {
        constexpr bool m = decltype(M)::value, a = decltype(A)::value, r = decltype(R)::value;
        if constexpr (!decltype(U)::value) {               // (this kernel has no bilinear epilogue: a stride-2 launch with the skip takes the direct kernel)
            if constexpr (sizeof(T) == 2 && !r) {          // hi + lo weights: as above
                if (w2) { hipLaunchKernelGGL((conv32_s2_lds_kernel<T, false, m, a, true>), dim3(blocks), dim3(256), 0, s, p); return; }
            }
            hipLaunchKernelGGL((conv32_s2_lds_kernel<T, r, m, a>), dim3(blocks), dim3(256), 0, s, p);
        }
    });
    PTTA_CHECK_LAUNCH();
    return 0;
}
int conv32_launch_s2_lds(const Conv32P<float>& p, int flags, bool relu, bool w2, int blocks, hipStream_t s) { return launch_s2_lds(p, flags, relu, false, blocks, s); }
int conv32_launch_s2_lds(const Conv32P<bf16_t>& p, int flags, bool relu, bool w2, int blocks, hipStream_t s) { return launch_s2_lds(p, flags, relu, w2, blocks, s); }
