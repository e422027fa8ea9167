// The heads' tiled bf16x3 GEMM (heads.hip has the map of the heads' files), in two tile shapes: 128 x 128 (<2,2,2,2>) and, for an N
// that is no multiple of 128, 128 x 32 (<4,1,1,1>).
#include "heads_device.h"

// ---- bf16x3 variant: fp32-faithful products on the bf16 matrix cores -------------------------------
// a = ah + al (split while the A tile is staged, after the fused prologue), w = wh + wl (split once
// at load time); a*w ~= al*wh + ah*wl + ah*wh, fp32 accumulate (v_mfma_f32_32x32x16_bf16).
// Block tile (WGM*TM*32) x (WGN*TN*32), 4 waves, K slices of 32 staged through LDS as separate
// hi / lo bf16 planes with an 80-byte row stride (conflict-free ds_read_b128).
template <int WGM, int WGN, int TM, int TN, int PRO, int EPI>
__global__ __launch_bounds__(256) void gemm_x3_kernel(GemmX3P q) {
    constexpr int BM = WGM * TM * 32, BN = WGN * TN * 32;
    static_assert(BM == 128, "row-block partials assume 128-row blocks");
    const GemmP& p = q.g;
    __shared__ __attribute__((aligned(16))) unsigned char sm[(2 * BM + 2 * BN) * X3_ROW + 4 * 2 * BN * 4];
    unsigned char* Ahi = sm; unsigned char* Alo = Ahi + BM * X3_ROW;
    unsigned char* Bhi = Alo + BM * X3_ROW; unsigned char* Blo = Bhi + BN * X3_ROW;
    float* red = (float*)(Blo + BN * X3_ROW);                 // [WGM][2][BN]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int wm = wave / WGN, wn = wave % WGN;
    const int n0 = blockIdx.x * BN;
    const long row0 = (long)blockIdx.y * BM;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    for (int k0 = 0; k0 < p.K; k0 += 32) {
        // ---- A: 128 rows x 32 k fp32 -> prologue -> split -> LDS (8 k per thread-item) -----------
#pragma unroll
        for (int it = 0; it < BM * 4 / 256; ++it) {
            const int idx = tid + 256 * it;
            const int row = stage_row(idx), kq = idx & 3;
            const long gr = row0 + row;
            const int k = k0 + 8 * kq;
            float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (gr < p.R) {
                const float4 x0 = *(const float4*)((const float*)p.A + gr * p.K + k);
                const float4 x1 = *(const float4*)((const float*)p.A + gr * p.K + k + 4);
                v[0] = x0.x; v[1] = x0.y; v[2] = x0.z; v[3] = x0.w; v[4] = x1.x; v[5] = x1.y; v[6] = x1.z; v[7] = x1.w;
                if (PRO == 1) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = fmaxf(fmaf(v[e], p.pscale[k + e], p.pshift[k + e]), 0.f);
                } else if (PRO == 2) {
                    const float4 h0 = *(const float4*)(p.A2 + gr * p.K + k), h1 = *(const float4*)(p.A2 + gr * p.K + k + 4);
                    const float hh[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        v[e] = p.pscale[k + e] * (v[e] - p.pc1[k + e] - (hh[e] - p.pmean[k + e]) * p.pinv[k + e] * p.pc2[k + e]);
                }
            }
            uint4 hi, lo;
            split2(v[0], v[1], hi.x, lo.x); split2(v[2], v[3], hi.y, lo.y);
            split2(v[4], v[5], hi.z, lo.z); split2(v[6], v[7], hi.w, lo.w);
            *(uint4*)(Ahi + row * X3_ROW + 16 * kq) = hi;
            *(uint4*)(Alo + row * X3_ROW + 16 * kq) = lo;
        }
        // ---- B: BN rows x 32 k, pre-split bf16 planes ---------------------------------------------
#pragma unroll
        for (int it = 0; it < (BN * 4 + 255) / 256; ++it) {
            const int idx = tid + 256 * it;
            if (idx < BN * 4) {
                const int row = stage_row(idx), kq = idx & 3;
                const long off = (long)(n0 + row) * p.K + k0 + 8 * kq;
                *(uint4*)(Bhi + row * X3_ROW + 16 * kq) = *(const uint4*)(q.Whi + off);
                *(uint4*)(Blo + row * X3_ROW + 16 * kq) = *(const uint4*)(q.Wlo + off);
            }
        }
        __syncthreads();
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
        __syncthreads();
    }

    // ---- epilogue (same fusions as the exact kernel) ----------------------------------------------
#pragma unroll
    for (int b = 0; b < TN; ++b) {
        const int cl = (wn * TN + b) * 32 + i;          // column within the block tile
        const int col = n0 + cl;
        const float bias = p.bias ? p.bias[col] : 0.f;
        float s1 = 0.f, s2 = 0.f;
        float esc = 0.f, esh = 0.f, emu = 0.f, eiv = 0.f;
        if (EPI == 2) { esc = p.escale[col]; esh = p.eshift[col]; emu = p.emean[col]; eiv = p.einv[col]; }
#pragma unroll
        for (int a = 0; a < TM; ++a) {
            // global accesses in the quad-transposed layout (16 B per lane), arithmetic in the accumulator layout (see the
            // wave-specialised kernel, heads_ws.hip)
            const int tq = (i & 3) + 4 * h, tc = n0 + (wn * TN + b) * 32 + 4 * (i >> 2);
            const long arow = row0 + (wm * TM + a) * 32;
            f32x16 hh;
            if (EPI == 2) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    long row = arow + 8 * g + tq;
                    if (row >= p.R) row = p.R - 1;
                    const float4 q = *(const float4*)(p.eH + row * p.N + tc);
                    hh[4 * g] = q.x; hh[4 * g + 1] = q.y; hh[4 * g + 2] = q.z; hh[4 * g + 3] = q.w;
                }
                quad_transpose(hh, lane);
            }
            f32x16 t;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long row = arow + acc_row(r, h);
                float v = acc[a][b][r] + bias;
                if (EPI == 2) v = (fmaf(hh[r], esc, esh) > 0.f) ? v : 0.f;
                if (row < p.R) {
                    if (EPI == 1) { s1 += v; s2 += v * v; }
                    if (EPI == 2) { s1 += v; s2 += v * (hh[r] - emu) * eiv; }
                }
                t[r] = v;
            }
            quad_transpose(t, lane);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const long row = arow + 8 * g + tq;
                if (row < p.R) *(float4*)(p.C + row * p.N + tc) = make_float4(t[4 * g], t[4 * g + 1], t[4 * g + 2], t[4 * g + 3]);
            }
        }
        if (EPI != 0) {
            s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
            if (h == 0) { red[(wm * 2 + 0) * BN + cl] = s1; red[(wm * 2 + 1) * BN + cl] = s2; }
        }
    }
    if (EPI != 0) {
        __syncthreads();
        for (int t = tid; t < 2 * BN; t += 256) {
            const int which = t / BN, c = t % BN;
            float v = 0.f;
#pragma unroll
            for (int w = 0; w < WGM; ++w) v += red[(w * 2 + which) * BN + c];
            p.part[((long)blockIdx.y * 2 + which) * p.N + n0 + c] = v;
        }
    }
}

// key = pro * 10 + epi
int heads_launch_x3(const GemmX3P& q, bool cols128, int key, dim3 grid, hipStream_t s) {
    if (cols128) {
#define GX_(PRO, EPI) hipLaunchKernelGGL((gemm_x3_kernel<2, 2, 2, 2, PRO, EPI>), grid, dim3(256), 0, s, q)
        switch (key) {
            case 0: GX_(0, 0); break; case 1: GX_(0, 1); break; case 2: GX_(0, 2); break;
            case 10: GX_(1, 0); break; case 11: GX_(1, 1); break;
            case 20: GX_(2, 0); break;                  // BN-backward prologue into a 512-wide layer (stage-2 head trainer)
            default: return -22;
        }
#undef GX_
    } else {
#define GX_(PRO, EPI) hipLaunchKernelGGL((gemm_x3_kernel<4, 1, 1, 1, PRO, EPI>), grid, dim3(256), 0, s, q)
        switch (key) {
            case 0: GX_(0, 0); break; case 20: GX_(2, 0); break;
            default: return -22;
        }
#undef GX_
    }
    PTTA_CHECK_LAUNCH();
    return 0;
}
