// The validation kernels of the 3x3 32 -> 32 convolution -- exact fp32 MFMA arithmetic (PTTA_ARITH=exact) and the direct kernel
// (PTTA_CONV_IMPL=naive) -- and the weight packing.  The mapping of the exact kernel: conv32.hip, head of the file.
#include "conv32_launch.h"

template <typename T> struct Frag;
template <> struct Frag<float> { typedef float4 A; };
template <> struct Frag<bf16_t> { typedef uint4 A; };

template <typename T, int MODE, bool RELU, bool UP, bool MASK, bool ADD>
__global__ __launch_bounds__(256) void conv32_mfma_kernel(Conv32P<T> p) {
    constexpr bool F32 = sizeof(T) == 4;
    constexpr int NA = F32 ? 4 : 2;                  // 16-byte A fragments per tap
    typedef typename Frag<T>::A AF;
    const int lane = threadIdx.x & 63;
    const int i = lane & 31, h = lane >> 5;
    const float biasv = epi_bias(p.epi, i);               // once per kernel: ptta_common.h epi_tile
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));

    // ---- wave-stationary weights -------------------------------------------------------------
    AF w[9][NA];
    {
        const AF* wp = (const AF*)p.wpack;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int g = 0; g < NA; ++g) w[t][g] = wp[(t * NA + g) * 64 + lane];
    }

    const int Wt = (MODE == CONV_T2) ? p.Win : p.Wout;     // tile domain along x
    const int nseg = (Wt + 31) >> 5;
    const int npar = (MODE == CONV_T2) ? 2 : 1;
    const long nitems = (long)p.B * nseg * npar * p.Hout;
    const float sy = up_scale(p.Hout >> 1, p.Hout), sx = up_scale(p.Wout >> 1, p.Wout);

    for (long item = (long)blockIdx.x * 4 + wave; item < nitems; item += (long)gridDim.x * 4) {
        long t_ = item;
        const int y = (int)(t_ % p.Hout); t_ /= p.Hout;
        int xpar = 0;
        if (MODE == CONV_T2) { xpar = (int)(t_ & 1); t_ >>= 1; }
        const int seg = (int)(t_ % nseg);
        const int b = (int)(t_ / nseg);
        const int x0 = seg << 5;
        const bool lane_in = (x0 + i) < Wt;
        const T* inb = p.in + (size_t)(b % p.in_nb) * p.Hin * p.Win * 32;

        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;

#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap % 3;
            bool active = true;
            int yi, xi;
            if (MODE == CONV_S1) { yi = y + ky - 1; xi = x0 + i + kx - 1; }
            else if (MODE == CONV_S2) { yi = 2 * y + ky - 1; xi = 2 * (x0 + i) + kx - 1; }
            else {
                const int ty = y + 1 - ky, tx = xpar + 1 - kx;
                active = ((ty & 1) == 0) && ((tx & 1) == 0);
                yi = ty >> 1; xi = x0 + i + (tx >> 1);
            }
            active = active && (yi >= 0) && (yi < p.Hin);
            if (!active) continue;                                    // wave-uniform
            const bool ok = lane_in && (xi >= 0) && (xi < p.Win);
            const T* src = inb + ((size_t)yi * p.Win + (ok ? xi : 0)) * 32;
            AF a[NA];
#pragma unroll
            for (int g = 0; g < NA; ++g) {
                if (F32) {
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (ok) v = *(const float4*)((const float*)src + 8 * g + 4 * h);
                    if (RELU) v = relu4(v);
                    a[g] = *(AF*)&v;
                } else {
                    uint4 v = make_uint4(0, 0, 0, 0);
                    if (ok) v = *(const uint4*)((const bf16_t*)src + 16 * g + 8 * h);
                    if (RELU) v = relu8(v);
                    a[g] = *(AF*)&v;
                }
            }
#pragma unroll
            for (int g = 0; g < NA; ++g) {
                if (F32) {
                    const float4 av = *(float4*)&a[g];
                    const float4 wv = *(float4*)&w[tap][g];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, wv.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, wv.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, wv.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, wv.w, acc, 0, 0, 0);
                } else {
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[g]),
                                                                  __builtin_bit_cast(bf16x8, w[tap][g]),
                                                                  acc, 0, 0, 0);
                }
            }
        }

        // ---- epilogue: lane = channel (lane&31), registers = 16 pixels of the tile --------------
        epi_tile<T, UP, MASK, ADD>(p.epi, b, y, p.Hout, p.Wout, i, acc, x0, h, Wt, MODE == CONV_T2 ? 2 : 1, xpar, sy, sx, nullptr, 0, 0, &biasv);
    }
}

// ---- reference-style direct kernel (one thread per output element), same epilogue ------------
// Selected with PTTA_CONV_IMPL=naive: keeps the whole pipeline testable independently of the MFMA
// fragment packing.  Weights in canonical float layout Wc[tap][cin][cout].
template <typename T, int MODE, bool RELU>
__global__ void conv32_naive_kernel(Conv32P<T> p) {
    const long total = (long)p.B * p.Hout * p.Wout * 32;
    const float* wc = (const float*)p.wpack;
    const float sy = up_scale(p.Hout >> 1, p.Hout), sx = up_scale(p.Wout >> 1, p.Wout);
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int co = (int)(idx & 31);
        long t_ = idx >> 5;
        const int x = (int)(t_ % p.Wout); t_ /= p.Wout;
        const int y = (int)(t_ % p.Hout);
        const int b = (int)(t_ / p.Hout);
        const T* inb = p.in + (size_t)(b % p.in_nb) * p.Hin * p.Win * 32;
        float acc = 0.f;
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap % 3;
            int yi, xi;
            if (MODE == CONV_S1) { yi = y + ky - 1; xi = x + kx - 1; }
            else if (MODE == CONV_S2) { yi = 2 * y + ky - 1; xi = 2 * x + kx - 1; }
            else {
                const int ty = y + 1 - ky, tx = x + 1 - kx;
                if ((ty & 1) || (tx & 1)) continue;
                yi = ty >> 1; xi = tx >> 1;
            }
            if (yi < 0 || yi >= p.Hin || xi < 0 || xi >= p.Win) continue;
            const T* src = inb + ((size_t)yi * p.Win + xi) * 32;
            for (int ci = 0; ci < 32; ++ci) {
                float v = ld(src + ci);
                if (RELU) v = fmaxf(v, 0.f);
                acc = fmaf(v, wc[(tap * 32 + ci) * 32 + co], acc);
            }
        }
        Lerp ly = {0, 0, 0.f, 0.f}, lx = {0, 0, 0.f, 0.f};
        if (p.epi.up) { ly = lerp_coef(y, p.Hout >> 1, sy); lx = lerp_coef(x, p.Wout >> 1, sx); }
        epi_store<T>(p.epi, b, y, x, p.Hout, p.Wout, co, acc, ly, lx);
    }
}

// ---- weight packing (device side, so adapted parameters can be re-packed every step) ----------
// src: a Conv2d weight [out][in][3][3] or ConvTranspose2d weight [in][out][3][3] (fp32, NCHW).
// in_major: src is indexed [cin_eff][cout_eff]; flip: use tap (2-ky, 2-kx).  See DESIGN.md §5 for
// which (in_major, flip) pair each forward/backward use needs.
__global__ void pack_conv32_kernel(const float* __restrict__ src, float* mf32, bf16_t* mbf16, bf16_t* mlo, float* canon,
                                   int in_major, int flip, int row_stride, int col_off) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;          // over tap*32*32
    if (idx >= 9 * 32 * 32) return;
    const int co = idx & 31, ci = (idx >> 5) & 31, tap = idx >> 10;
    const int st = flip ? 8 - tap : tap;
    // row_stride / col_off select a 32x32 block out of a wider weight (the 32->128->32 meta layer)
    const float v = in_major ? src[((size_t)ci * row_stride + col_off + co) * 9 + st] : src[((size_t)co * row_stride + col_off + ci) * 9 + st];
    canon[(tap * 32 + ci) * 32 + co] = v;
    {   // fp32 fragments: [tap][g][lane][s], lane = h*32 + cout, cin = 8g + 4h + s
        const int g = ci >> 3, hh = (ci >> 2) & 1, s = ci & 3;
        mf32[((tap * 4 + g) * 64 + hh * 32 + co) * 4 + s] = v;
    }
    {   // bf16 fragments: [tap][kk][lane][e], cin = 16kk + 8h + e
        const int kk = ci >> 4, hh = (ci >> 3) & 1, e = ci & 7;
        const bf16_t hi = f2bf(v);
        mbf16[((tap * 2 + kk) * 64 + hh * 32 + co) * 8 + e] = hi;
        mlo[((tap * 2 + kk) * 64 + hh * 32 + co) * 8 + e] = f2bf(v - bf2f(hi));     // bf16x3 split: v ~= hi + lo
    }
}

void ptta_pack_conv32(const float* src, const ConvW& w, int in_major, int flip, hipStream_t s, int row_stride, int col_off) {
    hipLaunchKernelGGL(pack_conv32_kernel, dim3(36), dim3(256), 0, s, src, w.mf32, w.mbf16, w.mlo, w.canon, in_major, flip, row_stride, col_off);
}


// ---- host entries (conv32_launch.h) ----
template <int MODE>
static void launch_exact_t(const Conv32P<float>& p, int flags, bool relu, int blocks, hipStream_t s) {
    with_flags(flags, relu, [&](auto U, auto M, auto A, auto R) {
        hipLaunchKernelGGL((conv32_mfma_kernel<float, MODE, decltype(R)::value, decltype(U)::value, decltype(M)::value, decltype(A)::value>), dim3(blocks), dim3(256), 0, s, p);
    });
}
int conv32_launch_exact(const Conv32P<float>& p, int mode, int flags, bool relu, int blocks, hipStream_t s) {
    if (mode == CONV_S1) launch_exact_t<CONV_S1>(p, flags, relu, blocks, s);
    else if (mode == CONV_S2) launch_exact_t<CONV_S2>(p, flags, relu, blocks, s);
    else launch_exact_t<CONV_T2>(p, flags, relu, blocks, s);
    PTTA_CHECK_LAUNCH();
    return 0;
}
template <typename T>
static int launch_naive(const Conv32P<T>& p, int mode, bool relu, int blocks, hipStream_t s) {
    with_flag(relu, [&](auto R) {
        constexpr bool r = decltype(R)::value;
        if (mode == CONV_S1) hipLaunchKernelGGL((conv32_naive_kernel<T, CONV_S1, r>), dim3(blocks), dim3(256), 0, s, p);
        else if (mode == CONV_S2) hipLaunchKernelGGL((conv32_naive_kernel<T, CONV_S2, r>), dim3(blocks), dim3(256), 0, s, p);
        else hipLaunchKernelGGL((conv32_naive_kernel<T, CONV_T2, r>), dim3(blocks), dim3(256), 0, s, p);
    });
    PTTA_CHECK_LAUNCH();
    return 0;
}
int conv32_launch_naive(const Conv32P<float>& p, int mode, bool relu, int blocks, hipStream_t s) { return launch_naive(p, mode, relu, blocks, s); }
int conv32_launch_naive(const Conv32P<bf16_t>& p, int mode, bool relu, int blocks, hipStream_t s) { return launch_naive(p, mode, relu, blocks, s); }
