// The heads' fp64 moment kernels and BatchNorm1d finalisers (heads.hip has the map of the heads' files): the batch statistics of the
// never-materialised hidden layer, the finish of the data gradient through it, and the reduction of the GEMM epilogues' row-block
// partials into BatchNorm1d (train) statistics and BatchNorm-backward means.  Both precision modes launch them (heads_n.hip's GEMMs leave
// partials in the same layout).
#include "ptta_common.h"
#include "ptta_kernels.h"

// Batch statistics of h = X W0^T + b0 from the second moments of X: one block per HM_ROWS rows and pass, fp64 throughout on
// v_mfma_f64_16x16x4_f64 (A: lane = (m = lane & 15, k = lane >> 4), B: (n = lane & 15, k = lane >> 4), C/D: col = lane & 15,
// row = (lane >> 4) + 4 reg).  Phase 1: S = X^T X (32 x 32 = 2 x 2 tiles, K = rows) and the column sums, the block's rows split over
// the 8 waves, per-wave partials reduced through LDS in a fixed order.  Phase 2: T = W0 S (M = hidden unit: 32 tiles, 4 per wave), then
// per hidden unit sum h^2 = sum_b T[j][b] w_j[b] + 2 b_j (w_j . sx) + n b_j^2 and sum h = n b_j + w_j . sx.
typedef double d4_t __attribute__((ext_vector_type(4)));
#define HM_ROWS 256
int ptta_head_moment_blocks(long R) { return (int)((R + HM_ROWS - 1) / HM_ROWS); }
__device__ __forceinline__ double shfl_xor_d(double v, int m) { return __shfl_xor(v, m); }
__global__ __launch_bounds__(512) void head_moments_kernel(const float* __restrict__ X, long R, const float* __restrict__ W0,
                                                           const float* __restrict__ b0, float* __restrict__ part) {
    __shared__ double Sw[8][32][32];                  // per-wave partial second moments
    __shared__ double sxw[8][32];
    __shared__ double S[32][33];                      // S[a][b] = sum x_a x_b, S[a][32] = sum x_a
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int nb = gridDim.x, blk = blockIdx.x, pass = blockIdx.y;
    const float* Xp = X + (size_t)pass * R * 32;
    const long r0 = (long)blk * HM_ROWS, r1 = min(r0 + (long)HM_ROWS, R);
    d4_t c00 = {0, 0, 0, 0}, c01 = c00, c10 = c00, c11 = c00;
    double sa0 = 0.0, sa1 = 0.0;
#pragma unroll
    for (int s = 0; s < HM_ROWS / 8 / 4; ++s) {
        const long row = r0 + (HM_ROWS / 8) * wave + 4 * s + lk;
        const bool ok = row < r1;
        const float* xr = Xp + (size_t)(ok ? row : r0) * 32;
        const double x0 = ok ? (double)xr[li] : 0.0, x1 = ok ? (double)xr[16 + li] : 0.0;
        c00 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, x0, c00, 0, 0, 0);
        c01 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, x1, c01, 0, 0, 0);
        c10 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, x0, c10, 0, 0, 0);
        c11 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, x1, c11, 0, 0, 0);
        sa0 += x0; sa1 += x1;
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        Sw[wave][lk + 4 * v][li] = c00[v]; Sw[wave][lk + 4 * v][16 + li] = c01[v];
        Sw[wave][16 + lk + 4 * v][li] = c10[v]; Sw[wave][16 + lk + 4 * v][16 + li] = c11[v];
    }
    sa0 += shfl_xor_d(sa0, 16); sa0 += shfl_xor_d(sa0, 32); sa1 += shfl_xor_d(sa1, 16); sa1 += shfl_xor_d(sa1, 32);
    if (lk == 0) { sxw[wave][li] = sa0; sxw[wave][16 + li] = sa1; }
    __syncthreads();
    for (int e = t; e < 1024; e += 512) {
        const int a = e >> 5, b = e & 31;
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < 8; ++w) v += Sw[w][a][b];
        S[a][b] = v;
    }
    if (t < 32) { double v = 0.0; for (int w = 0; w < 8; ++w) v += sxw[w][t]; S[t][32] = v; }
    __syncthreads();
    const double n = (double)(r1 - r0);
    float* out = part + ((size_t)(pass * nb + blk) * 2) * 512;
#pragma unroll 1
    for (int qd = 0; qd < 4; ++qd) {
        const int j0 = 16 * (4 * wave + qd);
        d4_t T0 = {0, 0, 0, 0}, T1 = T0;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const double aw = (double)W0[(size_t)(j0 + li) * 32 + 4 * s + lk];
            T0 = __builtin_amdgcn_mfma_f64_16x16x4f64(aw, S[4 * s + lk][li], T0, 0, 0, 0);
            T1 = __builtin_amdgcn_mfma_f64_16x16x4f64(aw, S[4 * s + lk][16 + li], T1, 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int jj = j0 + lk + 4 * v;
            const double w0 = (double)W0[(size_t)jj * 32 + li], w1 = (double)W0[(size_t)jj * 32 + 16 + li];
            double q = T0[v] * w0 + T1[v] * w1, wsx = w0 * S[li][32] + w1 * S[16 + li][32];
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) { q += shfl_xor_d(q, m); wsx += shfl_xor_d(wsx, m); }
            if (li == 0) {
                const double bj = (double)b0[jj];
                out[jj] = (float)(n * bj + wsx);
                out[512 + jj] = (float)(q + 2.0 * bj * wsx + n * bj * bj);
            }
        }
    }
}
int ptta_launch_head_moments(const float* X, long R, int npass, const float* W0, const float* b0, float* part, hipStream_t s) {
    if (!X || !W0 || !b0 || !part || R < 1 || npass < 1) return -22;
    hipLaunchKernelGGL(head_moments_kernel, dim3(ptta_head_moment_blocks(R), npass), dim3(512), 0, s, X, R, W0, b0, part);
    PTTA_CHECK_LAUNCH();
    return 0;
}

// dX = sum_j gs_j (dy_j - c1_j - xhat_j c2_j) w_j with xhat_j = (x . w_j + b_j - mu_j) inv_j
//    = P - u - x M,   M[a][ch] = sum_j k2_j w_j[a] w_j[ch] (k2 = gs c2 inv),   u[ch] = sum_j (gs_j c1_j + k2_j (b_j - mu_j)) w_j[ch]
// (P = sum_j gs_j dy_j w_j comes out of the epi-3 GEMM in two column-block halves).  One launch: every block of 128 rows derives M and u
// itself (32 x 32 x 512 on v_mfma_f64_16x16x4_f64, the 512 hidden units split over the 8 waves, fixed-order reduction through LDS:
// identical in every block) and applies them to its rows.
__global__ __launch_bounds__(512) void head_bwd_finish_kernel(const double* __restrict__ k12, const float* __restrict__ W0, const float* __restrict__ P,
                                                              const float* __restrict__ X, long R, void* __restrict__ dX_, int halves, int dX_bf16) {
    __shared__ double Mw[8][32][32];
    __shared__ double uw[8][32];
    __shared__ float Ms[32][33];
    __shared__ float us[32];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int ch = t & 31;
    const long base = (long)blockIdx.x * 128;
    // this thread's rows of the apply phase, fetched up front (in flight during the M / u phase)
    float xv[8], pv[8];
#pragma unroll
    for (int ps = 0; ps < 8; ++ps) {
        const long row = base + 16 * ps + (t >> 5);
        const long rr = row < R ? row : R - 1;
        xv[ps] = X[rr * 32 + ch];
        pv[ps] = halves == 2 ? P[rr * 32 + ch] + P[(R + rr) * 32 + ch] : P[rr * 32 + ch];
    }
    d4_t m00 = {0, 0, 0, 0}, m01 = m00, m10 = m00, m11 = m00;
    double u0 = 0.0, u1 = 0.0;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int j = 64 * wave + 4 * s + lk;
        const double k1 = k12[j], k2 = k12[512 + j];
        const double x0 = (double)W0[(size_t)j * 32 + li], x1 = (double)W0[(size_t)j * 32 + 16 + li];
        m00 = __builtin_amdgcn_mfma_f64_16x16x4f64(k2 * x0, x0, m00, 0, 0, 0);
        m01 = __builtin_amdgcn_mfma_f64_16x16x4f64(k2 * x0, x1, m01, 0, 0, 0);
        m10 = __builtin_amdgcn_mfma_f64_16x16x4f64(k2 * x1, x0, m10, 0, 0, 0);
        m11 = __builtin_amdgcn_mfma_f64_16x16x4f64(k2 * x1, x1, m11, 0, 0, 0);
        u0 += k1 * x0; u1 += k1 * x1;
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        Mw[wave][lk + 4 * v][li] = m00[v]; Mw[wave][lk + 4 * v][16 + li] = m01[v];
        Mw[wave][16 + lk + 4 * v][li] = m10[v]; Mw[wave][16 + lk + 4 * v][16 + li] = m11[v];
    }
    u0 += shfl_xor_d(u0, 16); u0 += shfl_xor_d(u0, 32); u1 += shfl_xor_d(u1, 16); u1 += shfl_xor_d(u1, 32);
    if (lk == 0) { uw[wave][li] = u0; uw[wave][16 + li] = u1; }
    __syncthreads();
    for (int e = t; e < 1024; e += 512) {
        const int a = e >> 5, b = e & 31;
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < 8; ++w) v += Mw[w][a][b];
        Ms[a][b] = (float)v;
    }
    if (t < 32) { double v = 0.0; for (int w = 0; w < 8; ++w) v += uw[w][t]; us[t] = (float)v; }
    __syncthreads();
    float mc[32];
#pragma unroll
    for (int a = 0; a < 32; ++a) mc[a] = Ms[a][ch];
    const float uc = us[ch];
#pragma unroll
    for (int ps = 0; ps < 8; ++ps) {
        const long row = base + 16 * ps + (t >> 5);                // rows come in multiples of 16 (H/4 x W/4 of sizes divisible by 16)
        float acc = 0.f;
#pragma unroll
        for (int a = 0; a < 32; ++a) acc = fmaf(__shfl(xv[ps], (lane & 32) + a, 64), mc[a], acc);
        if (row < R) {
            if (dX_bf16) ((bf16_t*)dX_)[row * 32 + ch] = f2bf(pv[ps] - acc - uc);
            else ((float*)dX_)[row * 32 + ch] = pv[ps] - acc - uc;
        }
    }
}
int ptta_launch_head_bwd_finish(const double* k12, const float* W0, const float* P, const float* X, long R, void* dX, hipStream_t s, int halves, int dX_bf16) {
    hipLaunchKernelGGL(head_bwd_finish_kernel, dim3((int)((R + 127) / 128)), dim3(512), 0, s, k12, W0, P, X, R, dX, halves, dX_bf16);
    PTTA_CHECK_LAUNCH();
    return 0;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// one wave per column: lanes stride over the row-block partials (fixed order per lane, then a
// butterfly: deterministic)
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ part, int row_blocks, int R, int N,
                                   const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float momentum,
                                   float* running_mean, float* running_var, long long* nbt,
                                   float* mean, float* invstd, float* scale, float* shift) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c == 0 && lane == 0 && nbt) *nbt += 1;
    if (c >= N) return;
    double s1 = 0.0, s2 = 0.0;
    for (int rb = lane; rb < row_blocks; rb += 64) {
        s1 += (double)part[((long)rb * 2 + 0) * N + c];
        s2 += (double)part[((long)rb * 2 + 1) * N + c];
    }
    s1 = wave_sum_d(s1); s2 = wave_sum_d(s2);
    if (lane != 0) return;
    const double mu = s1 / R;
    double var = s2 / R - mu * mu;
    if (var < 0.0) var = 0.0;
    const float iv = (float)(1.0 / sqrt(var + (double)eps));
    mean[c] = (float)mu; invstd[c] = iv;
    const float sc = gamma[c] * iv;
    scale[c] = sc; shift[c] = beta[c] - (float)mu * sc;
    if (running_mean) {
        const double unb = R > 1 ? var * (double)R / (double)(R - 1) : var;
        running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mu;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unb;
    }
}

int ptta_launch_bn_finalize(const float* part, int row_blocks, int R, int N, const float* gamma, const float* beta,
                            float eps, float momentum, float* running_mean, float* running_var, long long* nbt,
                            float* mean, float* invstd, float* scale, float* shift, hipStream_t s) {
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((N + 3) / 4), dim3(256), 0, s, part, row_blocks, R, N, gamma, beta,
                       eps, momentum, running_mean, running_var, nbt, mean, invstd, scale, shift);
    PTTA_CHECK_LAUNCH();
    return 0;
}

__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* __restrict__ part, int row_blocks, int R, int N,
                                       const float* __restrict__ gamma, const float* __restrict__ invstd,
                                       float* gscale, float* c1, float* c2, float* dgamma, float* dbeta,
                                       double* k12 = nullptr, const float* __restrict__ b0 = nullptr, const float* __restrict__ mean = nullptr,
                                       float dscale = 1.f) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= N) return;
    double s1 = 0.0, s2 = 0.0;
    for (int rb = lane; rb < row_blocks; rb += 64) {
        s1 += (double)part[((long)rb * 2 + 0) * N + c];
        s2 += (double)part[((long)rb * 2 + 1) * N + c];
    }
    s1 = wave_sum_d(s1); s2 = wave_sum_d(s2);
    if (lane != 0) return;
    c1[c] = (float)(s1 / R); c2[c] = (float)(s2 / R);
    gscale[c] = gamma[c] * invstd[c];
    if (dgamma) { dgamma[c] = (float)(s2 * dscale); dbeta[c] = (float)(s1 * dscale); }     // d gamma = sum g * xhat, d beta = sum g (stage-2 head trainer)
    if (k12) {      // heads v2 (head_bwd_finish_kernel): k2 = gs c2 inv, k1 = gs c1 + k2 (b0 - mean), in double
        const double gs = (double)gamma[c] * (double)invstd[c];
        const double k2 = gs * (s2 / R) * (double)invstd[c];
        k12[c] = gs * (s1 / R) + k2 * ((double)b0[c] - (double)mean[c]); k12[N + c] = k2;
    }
}

int ptta_launch_bn_bwd_finalize(const float* part, int row_blocks, int R, int N, const float* gamma, const float* invstd,
                                float* gscale, float* c1, float* c2, hipStream_t s, float* dgamma, float* dbeta,
                                double* k12, const float* b0, const float* mean, float dscale) {
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((N + 3) / 4), dim3(256), 0, s, part, row_blocks, R, N, gamma,
                       invstd, gscale, c1, c2, dgamma, dbeta, k12, b0, mean, dscale);
    PTTA_CHECK_LAUNCH();
    return 0;
}
