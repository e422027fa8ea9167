// The strided geometries of the 3x3 32 -> 32 convolution with direct loads: stride 2 with the bilinear skip, and transposed.  (The
// LDS-staged stride-2 kernel lives in conv32_s1.hip.)  Which of the two a stride-2 launch takes, and the grids: conv32.hip ptta_launch_conv32.
#include "conv32_launch.h"

// ---- stride-2 / transposed geometries, direct loads ----------------------------------------------------------------------
// Same per-wave tiling as conv32_mfma_kernel (32 outputs of one row / one x-parity), but each A fragment (8 channels of one input pixel)
// goes from L1/L2 straight into registers (fp32 storage: split into bf16 hi/lo there and fed to three bf16 MFMAs).  The weight fragments
// sit in LDS, loaded once per block -- the registers go to the activation loads that are in flight ahead of the MFMAs.  Input lines are
// re-read from L1/L2 by neighbouring taps (2.25x for stride 2), which is cheaper here than an 84 KB halo tile in LDS.  Round 2 built the
// LDS-staged, input-stationary transposed form (8x32 input tile, four parity accumulators per input row, 16 instead of 36 ds_reads):
// faster kernel by kernel (forward 35 -> 18 us at full resolution) but SLOWER in the replayed step (2.396 vs 2.384 ms, same
// box): its 79 KB of LDS cannot share a CU with the 120 KB GEMM blocks of the heads that run beside decoder 3, this
// form's 18 KB can -- reverted.
template <typename T, int MODE, bool RELU, bool UP, bool MASK, bool ADD, bool W2 = false>
__global__ __launch_bounds__(256, sizeof(T) == 2 ? 3 : 2) void conv32_direct_x3_kernel(Conv32P<T> p) {
    constexpr bool F32 = sizeof(T) == 4;
    __shared__ __attribute__((aligned(16))) unsigned char wl_lds[((F32 || W2) ? 2 : 1) * 18 * 64 * 16];     // [hi | lo][tap][k][lane] weight fragments
    const int tid = threadIdx.x, lane = tid & 63;
    const int i = lane & 31, h = lane >> 5;
    const float biasv = epi_bias(p.epi, i);               // once per kernel: ptta_common.h epi_tile
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Wt = (MODE == CONV_T2) ? p.Win : p.Wout;
    const int nseg = (Wt + 31) >> 5;
    const int npar = (MODE == CONV_T2) ? 2 : 1;
    const long nitems = (long)p.B * nseg * npar * p.Hout;
    const float sy = up_scale(p.Hout >> 1, p.Hout), sx = up_scale(p.Wout >> 1, p.Wout);

    // item state (one item = 32 outputs of one row / x parity), decoded before its first loads
    int y = 0, xpar = 0, b = 0, x0 = 0;
    bool lane_in = false;
    const T* inb = p.in;
    auto decode = [&](long item) __attribute__((always_inline)) {
        long t_ = item;
        y = (int)(t_ % p.Hout); t_ /= p.Hout;
        xpar = 0;
        if (MODE == CONV_T2) { xpar = (int)(t_ & 1); t_ >>= 1; }
        const int seg = (int)(t_ % nseg);
        b = (int)(t_ / nseg);
        x0 = seg << 5;
        lane_in = (x0 + i) < Wt;
        inb = p.in + (size_t)(b % p.in_nb) * p.Hin * p.Win * 32;
    };
    // Loads are UNCONDITIONAL (clamped address + select) and issued three taps ahead of their MFMAs: with a per-load
    // `if (ok)` every one of the 36 loads of an item waited for the previous one (s_waitcnt behind each exec branch), which
    // at the 1/8 and 1/16-resolution layers -- one item per wave -- was the whole kernel: 12.3 us whatever the size.
    Px<T> v[9][2];                                   // [tap][k-step]: channels 16 k + 8 h ... + 7 of the tap's pixel
    bool act[9], okl[9];
    auto fetch = [&](int tap) __attribute__((always_inline)) {
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
        act[tap] = active;                                          // wave-uniform
        okl[tap] = active && lane_in && (xi >= 0) && (xi < p.Win);
        if (!active) return;
        const T* src = inb + ((size_t)yi * p.Win + (okl[tap] ? xi : 0)) * 32 + 8 * h;
        v[tap][0] = px_load(src); v[tap][1] = px_load(src + 16);
    };
    long item = (long)blockIdx.x * 4 + wave;
    // the first item's loads go out BEFORE the weight fragments are staged: one memory round trip for both instead of two in a row
    // (the 1/8 and 1/16-resolution launches are one item per wave: their duration is this latency chain)
    if (item < nitems) { decode(item); fetch(0); fetch(1); fetch(2); fetch(3); fetch(4); fetch(5); }
    {
        const uint4* ph = (const uint4*)p.wpack;
        for (int idx = tid; idx < 18 * 64; idx += 256) *(uint4*)(wl_lds + idx * 16) = ph[idx];
        if constexpr (F32 || W2) {
            const uint4* pl = (const uint4*)p.wpack2;
            for (int idx = tid; idx < 18 * 64; idx += 256) *(uint4*)(wl_lds + (18 * 64 + idx) * 16) = pl[idx];
        }
    }
    lds_barrier();
    while (item < nitems) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        auto compute = [&](int tap) __attribute__((always_inline)) {
            if (!act[tap]) return;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const bf16x8 bh = __builtin_bit_cast(bf16x8, *(const uint4*)(wl_lds + ((tap * 2 + k) * 64 + lane) * 16));
                if constexpr (F32) {
                    float4 q0 = v[tap][k].a, q1 = v[tap][k].b;
                    if (!okl[tap]) { q0 = make_float4(0.f, 0.f, 0.f, 0.f); q1 = q0; }
                    if (RELU) { q0 = relu4(q0); q1 = relu4(q1); }
                    uint4 hi, lo;
                    split2(q0.x, q0.y, hi.x, lo.x); split2(q0.z, q0.w, hi.y, lo.y);
                    split2(q1.x, q1.y, hi.z, lo.z); split2(q1.z, q1.w, hi.w, lo.w);
                    const bf16x8 ah = __builtin_bit_cast(bf16x8, hi), al = __builtin_bit_cast(bf16x8, lo);
                    const bf16x8 bl = __builtin_bit_cast(bf16x8, *(const uint4*)(wl_lds + ((18 + tap * 2 + k) * 64 + lane) * 16));
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
                } else {
                    uint4 hi = v[tap][k].a;
                    if (!okl[tap]) hi = make_uint4(0u, 0u, 0u, 0u);
                    if (RELU) { hi.x = relu_pk(hi.x); hi.y = relu_pk(hi.y); hi.z = relu_pk(hi.z); hi.w = relu_pk(hi.w); }
                    if constexpr (W2) {
                        const bf16x8 bl = __builtin_bit_cast(bf16x8, *(const uint4*)(wl_lds + ((18 + tap * 2 + k) * 64 + lane) * 16));
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, hi), bl, acc, 0, 0, 0);
                    }
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, hi), bh, acc, 0, 0, 0);
                }
            }
        };
        compute(0); compute(1); compute(2);
        fetch(6); fetch(7); fetch(8);
        compute(3); compute(4); compute(5);
        compute(6); compute(7); compute(8);
        epi_tile<T, UP, MASK, ADD>(p.epi, b, y, p.Hout, p.Wout, i, acc, x0, h, Wt, MODE == CONV_T2 ? 2 : 1, xpar, sy, sx, nullptr, 0, 0, &biasv);
        item += (long)gridDim.x * 4;
        if (item < nitems) { decode(item); fetch(0); fetch(1); fetch(2); fetch(3); fetch(4); fetch(5); }
    }
}


// ---- host entries (conv32_launch.h): the epilogue flags and ReLU on load -> kernel instance ----
template <typename T, int MODE>
static void launch_direct_t(const Conv32P<T>& p, int flags, bool relu, bool w2, int blocks, hipStream_t s) {
    with_flags(flags, relu, [&](auto U, auto M, auto A, auto R) {
        constexpr bool u = decltype(U)::value, m = decltype(M)::value, a = decltype(A)::value, r = decltype(R)::value;
        if constexpr (sizeof(T) == 2 && !r) {              // hi + lo weights: narrow storage, no ReLU on load (the data gradients)
            if (w2) { hipLaunchKernelGGL((conv32_direct_x3_kernel<T, MODE, false, u, m, a, true>), dim3(blocks), dim3(256), 0, s, p); return; }
        }
        hipLaunchKernelGGL((conv32_direct_x3_kernel<T, MODE, r, u, m, a>), dim3(blocks), dim3(256), 0, s, p);
    });
}
template <typename T>
static int launch_direct(const Conv32P<T>& p, int mode, int flags, bool relu, bool w2, int blocks, hipStream_t s) {
    if ((mode != CONV_S2 && mode != CONV_T2) || (w2 && (relu || sizeof(T) != 2))) return -22;
    if (mode == CONV_S2) launch_direct_t<T, CONV_S2>(p, flags, relu, w2, blocks, s); else launch_direct_t<T, CONV_T2>(p, flags, relu, w2, blocks, s);
    PTTA_CHECK_LAUNCH();
    return 0;
}
int conv32_launch_direct(const Conv32P<float>& p, int mode, int flags, bool relu, bool w2, int blocks, hipStream_t s) { return launch_direct(p, mode, flags, relu, false, blocks, s); }
int conv32_launch_direct(const Conv32P<bf16_t>& p, int mode, int flags, bool relu, bool w2, int blocks, hipStream_t s) { return launch_direct(p, mode, flags, relu, w2, blocks, s); }
