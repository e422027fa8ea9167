// The heads' exact-fp32 GEMM (heads.hip has the map of the heads' files): C[R][N] = op(A)[R][K] * W[N][K]^T, 128 x (32 NT) block
// tiles, K staged through LDS in 32-deep slices (row stride padded to 36 floats => conflict-free ds_read_b128), fp32 in / fp32
// accumulate (v_mfma_f32_32x32x2_f32), with the fused prologues and epilogues heads.hip describes.
#include "heads_device.h"

template <int NT, int PRO, int EPI, bool ABF16>
__global__ __launch_bounds__(256) void gemm_mfma_kernel(GemmP p) {
    constexpr int BN = 32 * NT;
    __shared__ __attribute__((aligned(16))) float As[GEMM_BM * GEMM_LDS_STRIDE];
    __shared__ __attribute__((aligned(16))) float Bs[BN * GEMM_LDS_STRIDE];
    __shared__ float red[4][2][BN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int n0 = blockIdx.x * BN;
    const long row0 = (long)blockIdx.y * GEMM_BM;

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    for (int k0 = 0; k0 < p.K; k0 += GEMM_BK) {
        // ---- stage A (with the fused prologue) and B -----------------------------------------
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = tid + 256 * q;
            const int row = idx >> 3, kq = idx & 7;
            const long gr = row0 + row;
            const int k = k0 + 4 * kq;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gr < p.R) {
                if (ABF16) {
                    const uint2 u = *(const uint2*)((const bf16_t*)p.A + gr * p.K + k);
                    v.x = __uint_as_float(u.x << 16); v.y = __uint_as_float(u.x & 0xffff0000u);
                    v.z = __uint_as_float(u.y << 16); v.w = __uint_as_float(u.y & 0xffff0000u);
                } else {
                    v = *(const float4*)((const float*)p.A + gr * p.K + k);
                }
                if (PRO == 1) {
                    const float4 sc = *(const float4*)(p.pscale + k), sh = *(const float4*)(p.pshift + k);
                    v.x = fmaxf(fmaf(v.x, sc.x, sh.x), 0.f); v.y = fmaxf(fmaf(v.y, sc.y, sh.y), 0.f);
                    v.z = fmaxf(fmaf(v.z, sc.z, sh.z), 0.f); v.w = fmaxf(fmaf(v.w, sc.w, sh.w), 0.f);
                } else if (PRO == 2) {
                    // BatchNorm1d backward: dh = gamma*invstd * (g - mean(g) - xhat * mean(g*xhat))
                    const float4 hh = *(const float4*)(p.A2 + gr * p.K + k);
                    const float4 mu = *(const float4*)(p.pmean + k), iv = *(const float4*)(p.pinv + k);
                    const float4 gs = *(const float4*)(p.pscale + k);
                    const float4 c1 = *(const float4*)(p.pc1 + k), c2 = *(const float4*)(p.pc2 + k);
                    v.x = gs.x * (v.x - c1.x - (hh.x - mu.x) * iv.x * c2.x);
                    v.y = gs.y * (v.y - c1.y - (hh.y - mu.y) * iv.y * c2.y);
                    v.z = gs.z * (v.z - c1.z - (hh.z - mu.z) * iv.z * c2.z);
                    v.w = gs.w * (v.w - c1.w - (hh.w - mu.w) * iv.w * c2.w);
                }
            }
            *(float4*)(As + row * GEMM_LDS_STRIDE + 4 * kq) = v;
        }
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            const int idx = tid + 256 * q;
            const int row = idx >> 3, kq = idx & 7;
            *(float4*)(Bs + row * GEMM_LDS_STRIDE + 4 * kq) =
                *(const float4*)(p.W + (long)(n0 + row) * p.K + k0 + 4 * kq);
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float4 a = *(const float4*)(As + (32 * wave + i) * GEMM_LDS_STRIDE + 8 * c + 4 * h);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float4 b = *(const float4*)(Bs + (32 * t + i) * GEMM_LDS_STRIDE + 8 * c + 4 * h);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc[t], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // ---- epilogue ------------------------------------------------------------------------------
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = n0 + 32 * t + i;
        const float bias = p.bias ? p.bias[col] : 0.f;
        float s1 = 0.f, s2 = 0.f;
        float esc = 0.f, esh = 0.f, emu = 0.f, eiv = 0.f;
        if (EPI == 2) { esc = p.escale[col]; esh = p.eshift[col]; emu = p.emean[col]; eiv = p.einv[col]; }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long row = row0 + 32 * wave + acc_row(r, h);
            if (row >= p.R) continue;
            float v = acc[t][r] + bias;
            if (EPI == 1) { s1 += v; s2 += v * v; }
            if (EPI == 2) {
                const float hh = p.eH[row * p.N + col];
                v = (fmaf(hh, esc, esh) > 0.f) ? v : 0.f;
                s1 += v; s2 += v * (hh - emu) * eiv;
            }
            p.C[row * p.N + col] = v;
        }
        if (EPI != 0) {
            s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
            if (h == 0) { red[wave][0][32 * t + i] = s1; red[wave][1][32 * t + i] = s2; }
        }
    }
    if (EPI != 0) {
        __syncthreads();
        if (tid < 2 * BN) {
            const int which = tid / BN, c = tid % BN;
            const float v = red[0][which][c] + red[1][which][c] + red[2][which][c] + red[3][which][c];
            p.part[((long)blockIdx.y * 2 + which) * p.N + n0 + c] = v;
        }
    }
}

// key = pro * 100 + epi * 10 + a_bf16
int heads_launch_f32(const GemmP& p, int nt, int key, dim3 grid, hipStream_t s) {
#define GL_(NT, PRO, EPI, BF) hipLaunchKernelGGL((gemm_mfma_kernel<NT, PRO, EPI, BF>), grid, dim3(256), 0, s, p)
    if (nt == 2) {
        switch (key) {
            case 0: GL_(2, 0, 0, false); break;
            case 10: GL_(2, 0, 1, false); break;
            case 11: GL_(2, 0, 1, true); break;
            case 100: GL_(2, 1, 0, false); break;
            case 110: GL_(2, 1, 1, false); break;
            case 20: GL_(2, 0, 2, false); break;
            case 200: GL_(2, 2, 0, false); break;
            default: return -22;
        }
    } else {
        switch (key) {
            case 0: GL_(1, 0, 0, false); break;
            case 200: GL_(1, 2, 0, false); break;
            default: return -22;
        }
    }
#undef GL_
    PTTA_CHECK_LAUNCH();
    return 0;
}
