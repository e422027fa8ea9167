// Projection / prediction MLP heads of ProxyTTA (network_exp_msg_chn_adapt.py:1031-1036,1089-1098:
// Linear - BatchNorm1d(train) - ReLU - Linear, 32 -> 512 -> 512 and 512 -> 512 -> 512) and the
// backward through the one `proj` application that carries gradient (:554).
//
// These are the true dense contractions of the step (37 % of forward MACs), so
// they run on the matrix cores: C[R][N] = op(A)[R][K] * W[N][K]^T, 128x64 block tiles, K staged
// through LDS in 32-deep slices (row stride padded to 36 floats => conflict-free ds_read_b128),
// fp32 in / fp32 accumulate (v_mfma_f32_32x32x2_f32, exact fp32).
// Fusions: BatchNorm+ReLU of the previous layer is applied while the A tile is staged (never
// materialised), the train-mode batch statistics of the produced layer come out of the epilogue
// as per-row-block partial column sums (deterministic two-stage reduction, no atomics), and in
// the backward the ReLU mask / BatchNorm-backward reductions are fused the same way.
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include "ptta_common.h"
#include "ptta_kernels.h"

#define GEMM_BM 128
#define GEMM_BK 32
#define GEMM_LDS_STRIDE 36

struct GemmP {
    const void* A; const float* A2; const float* W; const float* bias; float* C;
    int R, K, N;
    const float* pscale; const float* pshift; const float* pmean; const float* pinv; const float* pc1; const float* pc2;
    const float* eH; const float* escale; const float* eshift; const float* emean; const float* einv;
    float* part;
};

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

// ---- bf16x3 variant: fp32-faithful products on the bf16 matrix cores -------------------------------
// a = ah + al (split while the A tile is staged, after the fused prologue), w = wh + wl (split once
// at load time); a*w ~= al*wh + ah*wl + ah*wh, fp32 accumulate (v_mfma_f32_32x32x16_bf16).
// Block tile (WGM*TM*32) x (WGN*TN*32), 4 waves, K slices of 32 staged through LDS as separate
// hi / lo bf16 planes with an 80-byte row stride (conflict-free ds_read_b128).
#define X3_ROW 80            // bytes per LDS row: 32 bf16 + 16 pad

typedef __bf16 hbf16x2 __attribute__((ext_vector_type(2)));
typedef float hfloat2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void hsplit2(float a, float b, unsigned& hi, unsigned& lo) {
    hfloat2 v = {a, b};
    hi = __builtin_bit_cast(unsigned, __builtin_convertvector(v, hbf16x2));
    hfloat2 r = {a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u)};
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(r, hbf16x2));
}

// staging item -> (row, 8-k chunk): the 8 lanes of one ds_write_b128 group take rows r and r+4 (not r and
// r+1), whose 64-B footprints do not share banks at the 80-B row stride; each row's 128 B of global
// memory is still fetched by 4 adjacent lanes
__device__ __forceinline__ int stage_row(int idx) { return ((idx >> 5) << 3) + (((idx >> 2) & 1) << 2) + ((idx >> 3) & 3); }

struct GemmX3P {
    GemmP g;
    const bf16_t* Whi; const bf16_t* Wlo;
    const bf16_t* Wil;           // interleaved [n][k/32][hi 32 | lo 32] (wide kernel)
    // heads v2 (GemmArgs): PRO 3 / EPI 3 of the wave-specialised kernel
    const float* X; const uint4* W0frag; const float* b0;
    const bf16_t* W0hi; const bf16_t* W0lo; const bf16_t* W0thi; const bf16_t* W0tlo;
    float* P;
    // PRO 4: A = d loss_cos / d ref computed while it is staged: A[r][k] = coef (e[r][k] / |e_r| - c_r ref[r][k] / |ref_r|) / |ref_r| from
    // emb (g.A), ref (Bref), the per-row statistics of the loss forward (rowstats: |e|, |ref|, cos) and the gated weight (coef[0])
    const float* Bref; const float* rowstats; const float* coef;
};
#define DY_ROW 272           // bytes per row of the EPI 3 gradient planes: 128 bf16 + 16 pad (conflict-free ds_read_b128)

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
            hsplit2(v[0], v[1], hi.x, lo.x); hsplit2(v[2], v[3], hi.y, lo.y);
            hsplit2(v[4], v[5], hi.z, lo.z); hsplit2(v[6], v[7], hi.w, lo.w);
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
            // wave-specialised kernel below)
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
                hsplit2(x0.x, x0.y, xh[ks].x, xl[ks].x); hsplit2(x0.z, x0.w, xh[ks].y, xl[ks].y);
                hsplit2(x1.x, x1.y, xh[ks].z, xl[ks].z); hsplit2(x1.z, x1.w, xh[ks].w, xl[ks].w);
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
                    hsplit2(v0, v1, hi.x, lo.x); hsplit2(v2, v3, hi.y, lo.y);
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
                hsplit2(v[0], v[1], hi.x, lo.x); hsplit2(v[2], v[3], hi.y, lo.y);
                hsplit2(v[4], v[5], hi.z, lo.z); hsplit2(v[6], v[7], hi.w, lo.w);
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
                    hsplit2(x0.x, x0.y, xh[a][ks].x, xl[a][ks].x); hsplit2(x0.z, x0.w, xh[a][ks].y, xl[a][ks].y);
                    hsplit2(x1.x, x1.y, xh[a][ks].z, xl[a][ks].z); hsplit2(x1.z, x1.w, xh[a][ks].w, xl[a][ks].w);
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
                            hsplit2(t[4 * g], t[4 * g + 1], hi.x, lo.x); hsplit2(t[4 * g + 2], t[4 * g + 3], hi.y, lo.y);
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

// split an fp32 [N][K] weight into bf16 hi / lo planes
__global__ void split_weight_kernel(const float* __restrict__ w, bf16_t* __restrict__ hi, bf16_t* __restrict__ lo,
                                    bf16_t* __restrict__ il, long n, int K) {
    for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long)gridDim.x * blockDim.x) {
        const float v = w[k];
        const bf16_t hh = f2bf(v), ll = f2bf(v - bf2f(hh));
        hi[k] = hh; lo[k] = ll;
        if (il && (K & 31) == 0) {
            const long row = k / K; const int kk = (int)(k % K);
            const long base = (row * (K >> 5) + (kk >> 5)) * 64 + (kk & 31);
            il[base] = hh; il[base + 32] = ll;
        }
    }
}
void ptta_split_weight(const float* w, bf16_t* hi, bf16_t* lo, bf16_t* il, long n, int K, hipStream_t s) {
    long b = (n + 255) / 256; if (b > 1024) b = 1024;
    hipLaunchKernelGGL(split_weight_kernel, dim3((int)b), dim3(256), 0, s, w, hi, lo, il, n, K);
}

// ---- heads v2: support kernels ------------------------------------------------------------------------------------------------
__global__ void pack_w0_frag_kernel(const float* __restrict__ W0, uint4* __restrict__ frag) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;            // ((slice * 2 + kstep) * 2 + hl) * 64 + lane
    if (idx >= 16 * 2 * 2 * 64) return;
    const int lane = idx & 63, hl = (idx >> 6) & 1, ks = (idx >> 7) & 1, sl = idx >> 8;
    const float* src = W0 + (size_t)(32 * sl + (lane & 31)) * 32 + 16 * ks + 8 * (lane >> 5);
    unsigned w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        unsigned hi, lo;
        hsplit2(src[2 * e], src[2 * e + 1], hi, lo);
        w[e] = hl ? lo : hi;
    }
    frag[idx] = make_uint4(w[0], w[1], w[2], w[3]);
}
void ptta_pack_w0_frag(const float* W0, void* frag, hipStream_t s) {
    hipLaunchKernelGGL(pack_w0_frag_kernel, dim3(16), dim3(256), 0, s, W0, (uint4*)frag);
}

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

int ptta_gemm_row_blocks(int R) { return (R + GEMM_BM - 1) / GEMM_BM; }
// number of row-block partials the launch of `a` writes (every kernel here uses 128-row blocks)
int ptta_gemm_part_blocks(const GemmArgs& a) { return ptta_gemm_row_blocks(a.R); }

int ptta_launch_gemm(const GemmArgs& a, hipStream_t s) {
    if (a.K % GEMM_BK || a.N % 32) return -22;
    GemmP p;
    p.A = a.A; p.A2 = a.A2; p.W = a.W; p.bias = a.bias; p.C = a.C; p.R = a.R; p.K = a.K; p.N = a.N;
    p.pscale = a.pscale; p.pshift = a.pshift; p.pmean = a.pmean; p.pinv = a.pinv; p.pc1 = a.pc1; p.pc2 = a.pc2;
    p.eH = a.eH; p.escale = a.escale; p.eshift = a.eshift; p.emean = a.emean; p.einv = a.einv; p.part = a.part;
    if (a.x3 && !a.a_bf16) {
        GemmX3P q; q.g = p; q.Whi = a.Whi; q.Wlo = a.Wlo; q.Wil = a.Wil;
        q.X = a.X; q.W0frag = (const uint4*)a.W0frag; q.b0 = a.b0; q.W0hi = a.W0hi; q.W0lo = a.W0lo; q.W0thi = a.W0thi; q.W0tlo = a.W0tlo; q.P = a.P;
        q.Bref = a.Bref; q.rowstats = a.rowstats; q.coef = a.coef;
        if (a.pro == 4 && (!a.Bref || !a.rowstats || !a.coef || a.epi != 3)) return -22;
        const int key3 = a.pro * 10 + a.epi;
        if ((a.pro == 3 && (!a.X || !a.W0frag || !a.b0 || !a.pscale || !a.pshift)) ||
            (a.epi == 3 && (!a.X || !a.b0 || !a.W0hi || !a.W0lo || !a.W0thi || !a.W0tlo || !a.P || !a.escale || !a.part))) return -22;
        if ((a.pro == 3 || a.epi == 3) && !(a.N == 512 && a.K == 512 && a.Wil)) return -22;
        // (K = 32, the first Linear of proj: routed to the 128x128-tile kernel instead, the step is unchanged within noise --
        //  2.317 vs 2.318 ms A/B on one box: that launch is bound by its 55 MB of fp32 stores, not by the tiling)
        if (a.N == 512 && a.Wil && a.pro != 2) {
            dim3 grid(2, (a.R + 127) / 128);
#define GS_(PRO, EPI) hipLaunchKernelGGL((gemm_x3_ws_kernel<PRO, EPI>), grid, dim3(512), 0, s, q)
#ifdef PTTA_DIAG_STAMPS      // diagnostic build (make DIAG=1): in-kernel phase stamps of the PRO 1 / EPI 0 launch
            if (key3 == 10) { hipLaunchKernelGGL((gemm_x3_ws_kernel<1, 0, true>), grid, dim3(512), 0, s, q); PTTA_CHECK_LAUNCH(); return 0; }
#endif
            switch (key3) {
                case 0: GS_(0, 0); break; case 1: GS_(0, 1); break; case 2: GS_(0, 2); break;
                case 10: GS_(1, 0); break; case 11: GS_(1, 1); break;
                case 30: GS_(3, 0); break; case 31: GS_(3, 1); break; case 3: GS_(0, 3); break;       // heads v2
                case 4: GS_(0, 4); break;                                                              // column statistics only (no C)
                case 43: GS_(4, 3); break;                                                             // heads v2 backward from emb / ref (no gradient tensor)
                default: return -22;
            }
#undef GS_
        } else if (a.N % 128 == 0) {
            dim3 grid(a.N / 128, ptta_gemm_row_blocks(a.R));
#define GX_(PRO, EPI) hipLaunchKernelGGL((gemm_x3_kernel<2, 2, 2, 2, PRO, EPI>), grid, dim3(256), 0, s, q)
            switch (key3) {
                case 0: GX_(0, 0); break; case 1: GX_(0, 1); break; case 2: GX_(0, 2); break;
                case 10: GX_(1, 0); break; case 11: GX_(1, 1); break;
                case 20: GX_(2, 0); break;                  // BN-backward prologue into a 512-wide layer (stage-2 head trainer)
                default: return -22;
            }
#undef GX_
        } else {
            dim3 grid(a.N / 32, ptta_gemm_row_blocks(a.R));
#define GX_(PRO, EPI) hipLaunchKernelGGL((gemm_x3_kernel<4, 1, 1, 1, PRO, EPI>), grid, dim3(256), 0, s, q)
            switch (key3) {
                case 0: GX_(0, 0); break; case 20: GX_(2, 0); break;
                default: return -22;
            }
#undef GX_
        }
        PTTA_CHECK_LAUNCH();
        return 0;
    }
    const int nt = (a.N % 64 == 0) ? 2 : 1;
    dim3 grid(a.N / (32 * nt), ptta_gemm_row_blocks(a.R));
#define GL_(NT, PRO, EPI, BF) hipLaunchKernelGGL((gemm_mfma_kernel<NT, PRO, EPI, BF>), grid, dim3(256), 0, s, p)
    const int key = a.pro * 100 + a.epi * 10 + (a.a_bf16 ? 1 : 0);
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
