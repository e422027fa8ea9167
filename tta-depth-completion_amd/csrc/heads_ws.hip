// The heads' wave-specialised bf16x3 GEMM for N = 512 (heads.hip has the map of the heads' files), with the heads-v2 forms that never
// materialise the 512-wide hidden of proj (PRO 3 / EPI 3 / PRO 4) and, in the diagnostic build (make DIAG=1), its stamped instantiation.
#include <type_traits>
#include "heads_device.h"

// ---- N = 512, wave-specialised: block = 128 rows x 256 columns, 8 waves = 4 MFMA waves (2 x 2, each 64 x 128 outputs,
// 128 accumulator VGPRs) + 4 STAGING waves.  The staging waves own all data movement and the fused prologue (global ->
// registers two K slices ahead -> BN+ReLU -> bf16 hi/lo split -> ds_write into the other LDS stage); the MFMA waves only
// read fragments and issue MFMAs.  One LDS-only barrier per K slice; on every SIMD an MFMA wave and a staging wave are
// co-resident, so the matrix cores run while the next slice is transformed.  Measured against the round-1 kernel (256x256
// tile, 8 lock-step waves, two LDS stages: 24 % MFMA duty, 68 % of wave cycles parked) and against two independent 128x256
// blocks per CU: 85 / 92 / 95 us per 26752x512x512 GEMM; ablations (profiles/r02_gemm_ablation.txt): stores 20 us, loads 16 us,
// MFMAs 16 us, everything else 34 us and nothing overlaps across the block's single K loop -> the shape is bound by
// per-block latency chains, not by the matrix cores (DESIGN_LOG.md §8).
#define GSTAMP(v) do { if (TIMING) { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); v = t_; } } while (0)
template <int PRO, int EPI, bool TIMING = false>
__global__ __launch_bounds__(512, 1) void gemm_x3_ws_kernel(GemmX3P q) {
    unsigned long long T0 = 0, Ta = 0, Tb = 0, Tc = 0, Td = 0, dStore = 0, dLoad = 0, dBar = 0, dMfma = 0, Tloop = 0, Tend = 0;
    GSTAMP(T0);
    constexpr int BM = 128, BN = 256, TM = 2, TN = 4;
    constexpr int STAGE = (2 * BM + 2 * BN) * X3_ROW;         // 61,440 B
    const GemmP& p = q.g;
    __shared__ __attribute__((aligned(16))) unsigned char sm[2 * STAGE];
    __shared__ __attribute__((aligned(16))) float cst[PRO == 3 ? 3 * 512 : 4];       // PRO 3: BatchNorm scale | shift | first Linear's bias, per hidden unit
    float* red = (float*)sm;                                  // [2][2][BN], used after the K loop
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = lane & 31, h = lane >> 5;
    const int n0 = blockIdx.x * BN;
    const long row0 = (long)blockIdx.y * BM;
    const int nslices = p.K >> 5;

    if (wave >= 4) {
        // ================= staging waves =================
        const int tid = threadIdx.x - 256;
        // one K slice in flight: [item][half] (PRO 3: the four W0 fragments), B hi / lo, prologue scale / shift (PRO 3: + the first Linear's bias)
        struct Regs { float4 a[2][2]; uint4 bh[4], bl[4]; float4 sc[2], sh[2]; float4 e[PRO == 4 ? 2 : 1][2]; };
        Regs r0, r1;
        float cg_ie[2] = {0.f, 0.f}, cg_ir[2] = {0.f, 0.f}, cg_pj[2] = {0.f, 0.f}, cg_coef = 0.f;
        if (PRO == 4) {            // this lane's two rows are the same in every K slice: their constants once per block
            cg_coef = q.coef[0];
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                long gr = row0 + stage_row(tid + 256 * it);
                if (gr >= p.R) gr = p.R - 1;
                const float ne = q.rowstats[3 * gr], nr = q.rowstats[3 * gr + 1], cc = q.rowstats[3 * gr + 2];
                cg_ie[it] = 1.f / ne; cg_ir[it] = 1.f / nr; cg_pj[it] = (nr > 1e-12f) ? cc : 0.f;       // as loss.hip cos_grad_body
            }
        }
        // PRO 3: A[row][k] = relu(bn(x[row] . W0[k] + b0[k])) is COMPUTED here, on the matrix cores, as the 32 x 32 tile D = W0[slice] x^T
        // (M = hidden unit, N = row, K = 32 input channels: 2 k-steps x 3 bf16 products): this wave owns rows 32 (wave - 4) ... + 31, its x
        // fragments (B operand: lane = row, 8 consecutive channels) are split once per block; a lane then holds 4 x 4 consecutive hidden
        // units of ONE row -> BatchNorm + ReLU -> split -> 8-byte LDS stores.  The 55-MB hidden map is neither written nor read.
        uint4 xh[2], xl[2];
        if (PRO == 3) {
            long gr = row0 + 32 * (wave - 4) + i;
            if (gr >= p.R) gr = p.R - 1;
            const float* xs = q.X + gr * 32 + 8 * h;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const float4 x0 = *(const float4*)(xs + 16 * ks), x1 = *(const float4*)(xs + 16 * ks + 4);
                split2(x0.x, x0.y, xh[ks].x, xl[ks].x); split2(x0.z, x0.w, xh[ks].y, xl[ks].y);
                split2(x1.x, x1.y, xh[ks].z, xl[ks].z); split2(x1.z, x1.w, xh[ks].w, xl[ks].w);
            }
        }
        auto load_slice = [&](int sl, Regs& rr) {
            const int k0 = sl << 5;
            if (PRO == 3) {
                const uint4* wf = q.W0frag + (size_t)sl * 256 + lane;               // [slice][kstep][hi, lo][lane]
                rr.a[0][0] = __builtin_bit_cast(float4, wf[0]); rr.a[0][1] = __builtin_bit_cast(float4, wf[64]);
                rr.a[1][0] = __builtin_bit_cast(float4, wf[128]); rr.a[1][1] = __builtin_bit_cast(float4, wf[192]);
            } else {
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int idx = tid + 256 * it;
                long gr = row0 + stage_row(idx);
                if (gr >= p.R) gr = p.R - 1;                                  // clamped (rows beyond R are never stored)
                const float* src = (const float*)p.A + gr * p.K + k0 + 8 * (idx & 3);
                rr.a[it][0] = *(const float4*)src; rr.a[it][1] = *(const float4*)(src + 4);
                if (PRO == 4) {
                    const float* sr = q.Bref + gr * p.K + k0 + 8 * (idx & 3);
                    rr.e[it][0] = *(const float4*)sr; rr.e[it][1] = *(const float4*)(sr + 4);
                }
            }
            }
            if (PRO == 1) {     // fetched WITH the slice (both items of a thread share the 8 columns): a load inside store_slice is the
                                // youngest one there and waiting for it (vmcnt(0)) drains the prefetch of the next slice as well
                const int k = k0 + 8 * (tid & 3);
                rr.sc[0] = *(const float4*)(p.pscale + k); rr.sc[1] = *(const float4*)(p.pscale + k + 4);
                rr.sh[0] = *(const float4*)(p.pshift + k); rr.sh[1] = *(const float4*)(p.pshift + k + 4);
            }
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int idx = tid + 256 * it;
                const long off = ((long)(n0 + stage_row(idx)) * nslices + sl) * 64 + 8 * (idx & 3);
                rr.bh[it] = *(const uint4*)(q.Wil + off);
                rr.bl[it] = *(const uint4*)(q.Wil + off + 32);
            }
        };
        auto store_slice = [&](int stage, const Regs& rr, int sl_ = 0) {
            unsigned char* const Ahi = sm + stage * STAGE; unsigned char* const Alo = Ahi + BM * X3_ROW;
            unsigned char* const Bhi = Alo + BM * X3_ROW; unsigned char* const Blo = Bhi + BN * X3_ROW;
            if (PRO == 3) {
                // per-hidden-unit constants from LDS (cst: [scale | shift | b0][512]); accumulator rows 4 j ... 4 j + 3 = hidden units k0 + 8 j + 4 h ...
                // two independent accumulation chains (one per k-step, added afterwards): the producer's MFMAs queue behind the MFMA wave's
                // stream on this SIMD, and a dependent chain of six would wait for each one's full latency
                f32x16 hacc, hac2;
                float4 csc[4], csh[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = (sl_ << 5) + 8 * j + 4 * h;
                    const float4 b0v = *(const float4*)(cst + 1024 + k);
                    csc[j] = *(const float4*)(cst + k); csh[j] = *(const float4*)(cst + 512 + k);
                    hacc[4 * j] = b0v.x; hacc[4 * j + 1] = b0v.y; hacc[4 * j + 2] = b0v.z; hacc[4 * j + 3] = b0v.w;
                    hac2[4 * j] = 0.f; hac2[4 * j + 1] = 0.f; hac2[4 * j + 2] = 0.f; hac2[4 * j + 3] = 0.f;
                }
                {
                    const bf16x8 wh0 = __builtin_bit_cast(bf16x8, rr.a[0][0]), wl0 = __builtin_bit_cast(bf16x8, rr.a[0][1]);
                    const bf16x8 wh1 = __builtin_bit_cast(bf16x8, rr.a[1][0]), wl1 = __builtin_bit_cast(bf16x8, rr.a[1][1]);
                    const bf16x8 xh0 = __builtin_bit_cast(bf16x8, xh[0]), xl0 = __builtin_bit_cast(bf16x8, xl[0]);
                    const bf16x8 xh1 = __builtin_bit_cast(bf16x8, xh[1]), xl1 = __builtin_bit_cast(bf16x8, xl[1]);
                    hacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl0, xh0, hacc, 0, 0, 0);      // small terms first
                    hac2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl1, xh1, hac2, 0, 0, 0);
                    hacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh0, xl0, hacc, 0, 0, 0);
                    hac2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh1, xl1, hac2, 0, 0, 0);
                    hacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh0, xh0, hacc, 0, 0, 0);
                    hac2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh1, xh1, hac2, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 16; ++r) hacc[r] += hac2[r];
                }
                const int row = 32 * (wave - 4) + i;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v0 = fmaxf(fmaf(hacc[4 * j], csc[j].x, csh[j].x), 0.f), v1 = fmaxf(fmaf(hacc[4 * j + 1], csc[j].y, csh[j].y), 0.f);
                    const float v2 = fmaxf(fmaf(hacc[4 * j + 2], csc[j].z, csh[j].z), 0.f), v3 = fmaxf(fmaf(hacc[4 * j + 3], csc[j].w, csh[j].w), 0.f);
                    uint2 hi, lo;
                    split2(v0, v1, hi.x, lo.x); split2(v2, v3, hi.y, lo.y);
                    *(uint2*)(Ahi + row * X3_ROW + 16 * j + 8 * h) = hi;
                    *(uint2*)(Alo + row * X3_ROW + 16 * j + 8 * h) = lo;
                }
            } else {
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int idx = tid + 256 * it;
                const int row = stage_row(idx), kq = idx & 3;
                float v[8] = {rr.a[it][0].x, rr.a[it][0].y, rr.a[it][0].z, rr.a[it][0].w, rr.a[it][1].x, rr.a[it][1].y, rr.a[it][1].z, rr.a[it][1].w};
                if (PRO == 4) {
                    const float b[8] = {rr.e[it][0].x, rr.e[it][0].y, rr.e[it][0].z, rr.e[it][0].w, rr.e[it][1].x, rr.e[it][1].y, rr.e[it][1].z, rr.e[it][1].w};
                    const float ie = cg_ie[it], ir = cg_ir[it], pj = cg_pj[it];
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = cos_grad_elem(cg_coef, v[e], b[e], ie, ir, pj);
                }
                if (PRO == 1) {
                    const float4 s0 = rr.sc[0], s1 = rr.sc[1], t0 = rr.sh[0], t1 = rr.sh[1];
                    const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w}, sh[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = fmaxf(fmaf(v[e], sc[e], sh[e]), 0.f);
                }
                uint4 hi, lo;
                split2(v[0], v[1], hi.x, lo.x); split2(v[2], v[3], hi.y, lo.y);
                split2(v[4], v[5], hi.z, lo.z); split2(v[6], v[7], hi.w, lo.w);
                *(uint4*)(Ahi + row * X3_ROW + 16 * kq) = hi;
                *(uint4*)(Alo + row * X3_ROW + 16 * kq) = lo;
            }
            }
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int idx = tid + 256 * it;
                const int row = stage_row(idx), kq = idx & 3;
                *(uint4*)(Bhi + row * X3_ROW + 16 * kq) = rr.bh[it];
                *(uint4*)(Blo + row * X3_ROW + 16 * kq) = rr.bl[it];
            }
        };
        // Every load and every store below is UNCONDITIONAL (slice indices past the end are clamped to the last slice; the extra
        // stores go to the stage nobody reads): with `if (sl + 3 < nslices) load_slice(...)` the compiler must pick one s_waitcnt
        // immediate that is valid on both paths and falls back to vmcnt(0) at the top of every store_slice, which drained the
        // prefetch of the following slice each time (in-kernel stamps: 70 % of the staging waves' loop was that wait).
        const int last = nslices - 1;
        load_slice(0, r0);
        load_slice(min(1, last), r1);
        if (PRO == 3) {
            for (int idx = tid; idx < 512; idx += 256) { cst[idx] = p.pscale[idx]; cst[512 + idx] = p.pshift[idx]; cst[1024 + idx] = q.b0[idx]; }
            lds_barrier();                                          // (matched by the MFMA waves' extra barrier at their start)
        }
        store_slice(0, r0, 0);
        load_slice(min(2, last), r0);
        lds_barrier();                                              // slice 0 staged
        GSTAMP(Tloop);
        for (int sl = 0; sl + 1 < nslices; sl += 2) {
            // during the MFMAs of slice sl: stage slice sl+1 (ring 1), refill ring 1 with slice sl+3
            GSTAMP(Ta);
            store_slice(1, r1, min(sl + 1, last)); GSTAMP(Tb); load_slice(min(sl + 3, last), r1);
            GSTAMP(Tc);
            lds_barrier();
            GSTAMP(Td);
            dStore += Tb - Ta; dLoad += Tc - Tb; dBar += Td - Tc;
            // during the MFMAs of slice sl+1: stage slice sl+2 (ring 0), refill ring 0 with slice sl+4
            GSTAMP(Ta);
            store_slice(0, r0, min(sl + 2, last)); GSTAMP(Tb); load_slice(min(sl + 4, last), r0);
            GSTAMP(Tc);
            lds_barrier();
            GSTAMP(Td);
            dStore += Tb - Ta; dLoad += Tc - Tb; dBar += Td - Tc;
        }
        if (nslices & 1) lds_barrier();                             // odd slice count: the last slice's hand-back
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // the clamped tail loads land before the registers die
        if (EPI == 3) {
            // The MFMA waves hand over, in two passes of 128 columns, the masked gradient x gamma x invstd of this block as bf16 hi / lo
            // planes [row][column]; this wave contracts its 32 rows with W0 over those columns: P[row][ch] += dy[row][j] W0[j][ch]
            // (A = the LDS plane, B = W0^T fragments from L2: lane = channel, 8 consecutive hidden units), 24 MFMAs per pass.
            unsigned char* const DYhi = sm + 4096; unsigned char* const DYlo = DYhi + BM * DY_ROW;
            const int sw = wave - 4;
            f32x16 pacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) pacc[r] = 0.f;
#pragma unroll 1
            for (int pass = 0; pass < 2; ++pass) {
                uint4 th[8], tl[8];
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) {
                    const int j0 = n0 + (kk >= 4 ? 128 : 0) + pass * 64 + 16 * (kk & 3) + 8 * h;
                    th[kk] = *(const uint4*)(q.W0thi + (size_t)i * 512 + j0);
                    tl[kk] = *(const uint4*)(q.W0tlo + (size_t)i * 512 + j0);
                }
                lds_barrier();                                          // this pass's planes are complete
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) {
                    const int off = (32 * sw + i) * DY_ROW + 32 * kk + 16 * h;
                    const bf16x8 ah = __builtin_bit_cast(bf16x8, *(const uint4*)(DYhi + off));
                    const bf16x8 al = __builtin_bit_cast(bf16x8, *(const uint4*)(DYlo + off));
                    const bf16x8 bh = __builtin_bit_cast(bf16x8, th[kk]), bl = __builtin_bit_cast(bf16x8, tl[kk]);
                    pacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, pacc, 0, 0, 0);
                    pacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, pacc, 0, 0, 0);
                    pacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, pacc, 0, 0, 0);
                }
                lds_barrier();                                          // the planes may be overwritten
            }
            quad_transpose(pacc, lane);
            const int tq = (i & 3) + 4 * h;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const long row = row0 + 32 * sw + 8 * g + tq;
                if (row < p.R) *(float4*)(q.P + ((size_t)blockIdx.x * p.R + row) * 32 + 4 * (i >> 2)) = make_float4(pacc[4 * g], pacc[4 * g + 1], pacc[4 * g + 2], pacc[4 * g + 3]);
            }
        }
        GSTAMP(Tend);
        if (TIMING && (blockIdx.y == 50 || blockIdx.y == 150) && blockIdx.x == 0 && lane == 0)
            printf("stg blk %d wave %d: life %llu pro %llu loop %llu | store(+vmwait) %llu loadissue %llu barrier %llu\n", blockIdx.y, wave, Tend - T0, Tloop - T0, Tend - Tloop, dStore, dLoad, dBar);
    } else {
        // ================= MFMA waves =================
        const int wm = wave >> 1, wn = wave & 1;
        f32x16 acc[TM][TN];
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int b = 0; b < TN; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
        if (PRO == 3) lds_barrier();                                // the staging waves' constants are in LDS
        lds_barrier();                                              // slice 0 staged
        GSTAMP(Tloop);
        for (int sl = 0; sl < nslices; ++sl) {
            GSTAMP(Ta);
            const unsigned char* Ahi = sm + (sl & 1) * STAGE; const unsigned char* Alo = Ahi + BM * X3_ROW;
            const unsigned char* Bhi = Alo + BM * X3_ROW; const unsigned char* Blo = Bhi + BN * X3_ROW;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 ah[TM], al[TM];
#pragma unroll
                for (int a = 0; a < TM; ++a) {
                    const int off = ((wm * TM + a) * 32 + i) * X3_ROW + 32 * ks + 16 * h;
                    ah[a] = __builtin_bit_cast(bf16x8, *(const uint4*)(Ahi + off));
                    al[a] = __builtin_bit_cast(bf16x8, *(const uint4*)(Alo + off));
                }
#pragma unroll
                for (int b = 0; b < TN; ++b) {
                    const int off = ((wn * TN + b) * 32 + i) * X3_ROW + 32 * ks + 16 * h;
                    const bf16x8 bh = __builtin_bit_cast(bf16x8, *(const uint4*)(Bhi + off));
                    const bf16x8 bl = __builtin_bit_cast(bf16x8, *(const uint4*)(Blo + off));
#pragma unroll
                    for (int a = 0; a < TM; ++a) {
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[a], bh, acc[a][b], 0, 0, 0);
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bl, acc[a][b], 0, 0, 0);
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bh, acc[a][b], 0, 0, 0);
                    }
                }
            }
            GSTAMP(Tb);
            lds_barrier();          // hand the stage back; the other stage is complete
            GSTAMP(Tc);
            dMfma += Tb - Ta; dBar += Tc - Tb;
        }
        GSTAMP(Td);
        // ---- epilogue (MFMA waves only): N = 512 is a compile-time row stride, one base pointer per wave, and a block that
        // lies fully inside the R rows (always, when R is a multiple of 128) stores without per-element bounds branches ----
        constexpr int NC = 512;
        const bool full = row0 + BM <= p.R;
        const long wrow = row0 + wm * TM * 32;
        // Global accesses run in the quad-transposed layout (ptta_common.h quad_transpose): 16 B per lane, four instructions per
        // 32x32 accumulator instead of sixteen; bias, ReLU mask and the column statistics stay in the accumulator layout (lane =
        // column), so the arithmetic and its order are unchanged.  The mask input eH is fetched as float4 and transposed back.
        const int tq = (i & 3) + 4 * h, tc = 4 * (i >> 2);           // row offset within a group of eight, first of four columns
        float* const cw = p.C + wrow * NC + n0 + wn * TN * 32 + tc;
        const float* const hw = EPI == 2 ? p.eH + wrow * NC + n0 + wn * TN * 32 + tc : nullptr;
        // per-column constants of all four column tiles are fetched before the first store, and a block that lies fully inside the
        // R rows runs a branch-free body: a load behind a store (or any branch around either) makes the compiler wait vmcnt(0),
        // i.e. for the stores of the previous tile to be acknowledged -- the epilogue was 25-30 % of an MFMA wave's life that way
        float bias_[TN], esc_[TN], esh_[TN], emu_[TN], eiv_[TN];
#pragma unroll
        for (int b = 0; b < TN; ++b) {
            const int col = n0 + (wn * TN + b) * 32 + i;
            bias_[b] = p.bias ? p.bias[col] : 0.f;
            esc_[b] = esh_[b] = emu_[b] = eiv_[b] = 0.f;
            if (EPI >= 2) { esc_[b] = p.escale[col]; esh_[b] = p.eshift[col]; emu_[b] = p.emean[col]; eiv_[b] = p.einv[col]; }
        }
        auto load_h = [&](auto fullc, int ab, f32x16& hh) {
            constexpr bool FULL = decltype(fullc)::value;
            const int b = ab / TM, a = ab % TM;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int lr = a * 32 + 8 * g + tq;
                const float4 q = (FULL || wrow + lr < p.R) ? *(const float4*)(hw + (long)lr * NC + b * 32) : make_float4(0.f, 0.f, 0.f, 0.f);
                hh[4 * g] = q.x; hh[4 * g + 1] = q.y; hh[4 * g + 2] = q.z; hh[4 * g + 3] = q.w;
            }
        };
        auto epilogue = [&](auto fullc) {
            constexpr bool FULL = decltype(fullc)::value;
            f32x16 hnext;
            if (EPI == 2) load_h(fullc, 0, hnext);
#pragma unroll
            for (int b = 0; b < TN; ++b) {
                const int cl = (wn * TN + b) * 32 + i;
                const float bias = bias_[b], esc = esc_[b], esh = esh_[b], emu = emu_[b], eiv = eiv_[b];
                float s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int a = 0; a < TM; ++a) {
                    f32x16 hh;
                    if (EPI == 2) {
                        hh = hnext;
                        if (b * TM + a + 1 < TN * TM) load_h(fullc, b * TM + a + 1, hnext);     // next tile's mask input ahead of this tile's stores
                        quad_transpose(hh, lane);
                    }
                    f32x16 t;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int lr = a * 32 + acc_row(r, h);
                        const bool ok = FULL || wrow + lr < p.R;
                        float v = acc[a][b][r] + bias;
                        if (EPI == 2) v = (fmaf(hh[r], esc, esh) > 0.f) ? v : 0.f;
                        if (ok) {
                            if (EPI == 1 || EPI == 4) { s1 += v; s2 += v * v; }
                            if (EPI == 2) { s1 += v; s2 += v * (hh[r] - emu) * eiv; }
                        }
                        t[r] = v;
                    }
                    if (EPI != 4) {
                    quad_transpose(t, lane);
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int lr = a * 32 + 8 * g + tq;
                        if (FULL || wrow + lr < p.R) *(float4*)(cw + (long)lr * NC + b * 32) = make_float4(t[4 * g], t[4 * g + 1], t[4 * g + 2], t[4 * g + 3]);
                    }
                    }
                }
                if (EPI != 0) {
                    s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
                    if (h == 0) { red[(wm * 2 + 0) * BN + cl] = s1; red[(wm * 2 + 1) * BN + cl] = s2; }
                }
            }
        };
        if (EPI == 3) {
            // ---- data gradient through proj.3 WITHOUT the stored hidden: h = x W0^T + b0 of this wave's 64 x 128 outputs is recomputed on
            // the matrix cores in the accumulator layout (A = x rows, B = W0 rows of the column tile: K = 32), the ReLU mask and the two
            // BatchNorm-backward column sums are taken as in EPI 2, and the masked gradient x gamma x invstd goes to the LDS planes the
            // staging waves contract with W0 (above) instead of to a [R][512] tensor ----
            unsigned char* const DYhi = sm + 4096; unsigned char* const DYlo = DYhi + BM * DY_ROW;
            uint4 xh[TM][2], xl[TM][2];
#pragma unroll
            for (int a = 0; a < TM; ++a) {
                long gr = wrow + 32 * a + i;
                if (gr >= p.R) gr = p.R - 1;
                const float* xs = q.X + gr * 32 + 8 * h;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const float4 x0 = *(const float4*)(xs + 16 * ks), x1 = *(const float4*)(xs + 16 * ks + 4);
                    split2(x0.x, x0.y, xh[a][ks].x, xl[a][ks].x); split2(x0.z, x0.w, xh[a][ks].y, xl[a][ks].y);
                    split2(x1.x, x1.y, xh[a][ks].z, xl[a][ks].z); split2(x1.z, x1.w, xh[a][ks].w, xl[a][ks].w);
                }
            }
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
                for (int bb = 0; bb < 2; ++bb) {
                    const int b = 2 * pass + bb;
                    const int cl = (wn * TN + b) * 32 + i, col = n0 + cl;
                    uint4 wh[2], wl[2];
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        wh[ks] = *(const uint4*)(q.W0hi + (size_t)col * 32 + 16 * ks + 8 * h);
                        wl[ks] = *(const uint4*)(q.W0lo + (size_t)col * 32 + 16 * ks + 8 * h);
                    }
                    const float b0c = q.b0[col], esc = esc_[b], esh = esh_[b], emu = emu_[b], eiv = eiv_[b];
                    float s1 = 0.f, s2 = 0.f;
#pragma unroll
                    for (int a = 0; a < TM; ++a) {
                        f32x16 hh, hh2;                               // (the forward's association: one chain per k-step, bias in the first, then added)
#pragma unroll
                        for (int r = 0; r < 16; ++r) { hh[r] = b0c; hh2[r] = 0.f; }
                        {
                            const bf16x8 axh0 = __builtin_bit_cast(bf16x8, xh[a][0]), axl0 = __builtin_bit_cast(bf16x8, xl[a][0]);
                            const bf16x8 axh1 = __builtin_bit_cast(bf16x8, xh[a][1]), axl1 = __builtin_bit_cast(bf16x8, xl[a][1]);
                            const bf16x8 bwh0 = __builtin_bit_cast(bf16x8, wh[0]), bwl0 = __builtin_bit_cast(bf16x8, wl[0]);
                            const bf16x8 bwh1 = __builtin_bit_cast(bf16x8, wh[1]), bwl1 = __builtin_bit_cast(bf16x8, wl[1]);
                            hh = __builtin_amdgcn_mfma_f32_32x32x16_bf16(axh0, bwl0, hh, 0, 0, 0);
                            hh2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(axh1, bwl1, hh2, 0, 0, 0);
                            hh = __builtin_amdgcn_mfma_f32_32x32x16_bf16(axl0, bwh0, hh, 0, 0, 0);
                            hh2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(axl1, bwh1, hh2, 0, 0, 0);
                            hh = __builtin_amdgcn_mfma_f32_32x32x16_bf16(axh0, bwh0, hh, 0, 0, 0);
                            hh2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(axh1, bwh1, hh2, 0, 0, 0);
#pragma unroll
                            for (int r = 0; r < 16; ++r) hh[r] += hh2[r];
                        }
                        f32x16 t;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int lr = a * 32 + acc_row(r, h);
                            const bool ok = full || wrow + lr < p.R;
                            float v = acc[a][b][r];
                            v = (fmaf(hh[r], esc, esh) > 0.f) ? v : 0.f;
                            if (ok) { s1 += v; s2 += v * (hh[r] - emu) * eiv; }
                            t[r] = v * esc;                                  // x gamma x invstd (escale = gamma * invstd)
                        }
                        quad_transpose(t, lane);
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const int row = (wm * TM + a) * 32 + 8 * g + tq, cp = wn * 64 + bb * 32 + tc;
                            uint2 hi, lo;
                            split2(t[4 * g], t[4 * g + 1], hi.x, lo.x); split2(t[4 * g + 2], t[4 * g + 3], hi.y, lo.y);
                            *(uint2*)(DYhi + row * DY_ROW + 2 * cp) = hi;
                            *(uint2*)(DYlo + row * DY_ROW + 2 * cp) = lo;
                        }
                    }
                    s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
                    if (h == 0) { red[(wm * 2 + 0) * BN + cl] = s1; red[(wm * 2 + 1) * BN + cl] = s2; }
                }
                lds_barrier();                                          // planes complete: the staging waves contract them
                lds_barrier();                                          // ... and are done with them
            }
        } else {
        if (full) epilogue(std::true_type{}); else epilogue(std::false_type{});
        }
        GSTAMP(Tend);
        if (TIMING && (blockIdx.y == 50 || blockIdx.y == 150) && blockIdx.x == 0 && lane == 0)
            printf("mma blk %d wave %d: life %llu pro %llu loop %llu epi %llu | mfma %llu barrier %llu\n", blockIdx.y, wave, Tend - T0, Tloop - T0, Td - Tloop, Tend - Td, dMfma, dBar);
    }
    if (EPI != 0) {
        __syncthreads();
        for (int t = threadIdx.x; t < 2 * BN; t += 512) {
            const int which = t / BN, c = t % BN;
            p.part[((long)blockIdx.y * 2 + which) * p.N + n0 + c] = red[(0 * 2 + which) * BN + c] + red[(1 * 2 + which) * BN + c];
        }
    }
}

// key = pro * 10 + epi
int heads_launch_ws(const GemmX3P& q, int key, dim3 grid, hipStream_t s) {
#define GS_(PRO, EPI) hipLaunchKernelGGL((gemm_x3_ws_kernel<PRO, EPI>), grid, dim3(512), 0, s, q)
#ifdef PTTA_DIAG_STAMPS      // diagnostic build (make DIAG=1): in-kernel phase stamps of the PRO 1 / EPI 0 launch
    if (key == 10) { hipLaunchKernelGGL((gemm_x3_ws_kernel<1, 0, true>), grid, dim3(512), 0, s, q); PTTA_CHECK_LAUNCH(); return 0; }
#endif
    switch (key) {
        case 0: GS_(0, 0); break; case 1: GS_(0, 1); break; case 2: GS_(0, 2); break;
        case 10: GS_(1, 0); break; case 11: GS_(1, 1); break;
        case 30: GS_(3, 0); break; case 31: GS_(3, 1); break; case 3: GS_(0, 3); break;       // heads v2
        case 4: GS_(0, 4); break;                                                              // column statistics only (no C)
        case 43: GS_(4, 3); break;                                                             // heads v2 backward from emb / ref (no gradient tensor)
        default: return -22;
    }
#undef GS_
    PTTA_CHECK_LAUNCH();
    return 0;
}
