// Host-side rules of the 32 -> 32 convolution launches, each written once (internal): the Conv32Args -> kernel-parameter builder, the
// tile counts and grid caps, the runtime-flag -> kernel-instance dispatcher, the predicate the two one-launch pair forms share, and the
// entry points of the kernel families (one translation unit each, so that every kernel is instantiated exactly once).
// Used by conv32.hip (ptta_launch_conv32: the family and geometry decision), conv32_first.hip, conv32_loop.hip, conv_pair.hip, conv_tpair.hip.
#pragma once
#include <type_traits>
#include "conv32_device.h"
#include "ptta_kernels.h"

// ---- Conv32Args -> Conv32P<T> ---------------------------------------------------------------------------------------------------
// The tuned kernels' parameters: bf16 hi fragments, and the lo fragments where the arithmetic reads them (fp32 storage, or narrow storage
// with hi + lo weights).  Every batch count is at least 1 (the kernels index b % nb).  A caller with other operands (the naive and exact
// kernels' weight image, the first-layer and layer-loop forms' own input and epilogue) overrides those fields after the call.
template <typename T>
static Conv32P<T> conv32_params(const Conv32Args& a, int Hout, int Wout) {
    auto nb = [](int n) { return n > 0 ? n : 1; };
    Conv32P<T> p;
    p.in = (const T*)a.in; p.in_nb = nb(a.in_nb);
    p.wpack = a.w->mbf16; p.wpack2 = (sizeof(T) == 4 || a.w2) ? a.w->mlo : nullptr;
    p.epi.bias = a.bias;
    p.epi.up = (const T*)a.up; p.epi.up_nb = nb(a.up_nb);
    p.epi.mask = (const T*)a.mask; p.epi.mask_nb = nb(a.mask_nb);
    p.epi.add1 = (const T*)a.add1; p.epi.add1_nb = nb(a.add1_nb);
    p.epi.add2 = (const T*)a.add2; p.epi.add2_nb = nb(a.add2_nb);
    p.epi.out_raw = (T*)a.out_raw; p.epi.out_sum = (T*)a.out_sum;
    p.epi.mask_bits = a.mask_bits; p.epi.bits_out = a.bits_out; p.epi.bits_nb = a.bits_nb; p.epi.bits_sum = a.bits_sum;
    p.B = a.B; p.Hin = a.Hin; p.Win = a.Win; p.Hout = Hout; p.Wout = Wout;
    return p;
}

// ---- tile counts, the kernel form of a stride-1 map, grid caps ------------------------------------------------------------------------
// TH x 32 tiles of B maps of H x W
static inline long conv32_tiles(int B, int H, int W, int TH) { return (long)B * ((W + 31) / 32) * ((H + TH - 1) / TH); }
// Small maps -- at most 256 tiles of 8 x 32: the 1/4 ... 1/16-resolution layers -- take the one-tile-per-block, latency-chain form of the
// stride-1 kernel (conv32_s1.hip conv32_s1_small_kernel) and its one-launch pairs; larger maps keep the persistent kernels.
static constexpr long kConv32SmallMapTiles = 256;
static inline bool conv32_s1_small_map(int B, int H, int W) { return conv32_tiles(B, H, W, X3_TH) <= kConv32SmallMapTiles; }
// Workgroups of a persistent full-chip launch.  The stride-1 kernel takes 480 of the 512 slots (two 256-VGPR blocks per CU): a launch that
// owns every register of the chip keeps every kernel of the other queues (the tiny BatchNorm finalizes between the heads' GEMMs, the next
// frame's prefix) waiting until it retires, and 32 CUs with a single block break the lock-step of the rest.  Round 4, same box, graph
// replay, pipelined / call by call: 512 1.698 / 1.819, 496 1.699, 480 1.681 / 1.803, 464 1.698, 448 1.73, 416 1.81; the first-layer /
// strided / transposed kernels stay at 512 (480 there: 1.689 vs 1.688).
static constexpr int kFullChipBlocks = 512;
static constexpr int kS1PersistentBlocks = 480;       // conv32_s1_x3_kernel and the persistent form of conv32_tpair_kernel
static constexpr int kS1SmallBlocks = 1024;           // the 4 x 32 one-tile forms: a block walks more than one tile only beyond this grid
// narrow kernels (half the LDS tile, ~160 VGPRs): three resident blocks per CU
static constexpr int kNarrowBlocks = 768;             // (the direct kernel only: <= 160 VGPRs, 18 KB LDS)
static inline int conv32_grid(long work, int cap) { return (int)(work > cap ? cap : work); }

// ---- runtime flags -> kernel instance -----------------------------------------------------------------------------------------------------
// The epilogue flags (bit 0 bilinear skip, bit 1 ReLU mask, bit 2 skip addends) and ReLU-on-load as compile-time constants:
//   with_flags(flags, relu, [&](auto U, auto M, auto A, auto R) { ... kernel<T, decltype(R)::value, decltype(U)::value, ...> ... });
// The body is instantiated for all sixteen combinations; a family that has fewer forms says so with `if constexpr` in its body.
template <bool V> using Flag = std::integral_constant<bool, V>;
template <typename F> static void with_flag(bool v, F&& f) { if (v) f(Flag<true>{}); else f(Flag<false>{}); }
static inline int conv32_flags(const Conv32Args& a) { return (a.up ? 1 : 0) | (a.mask ? 2 : 0) | (a.add1 ? 4 : 0); }
template <typename F> static void with_flags(int flags, bool relu, F&& f) {
    with_flag(flags & 1, [&](auto U) { with_flag(flags & 2, [&](auto M) { with_flag(flags & 4, [&](auto A) { with_flag(relu, [&](auto R) { f(U, M, A, R); }); }); }); });
}

// ---- the kernel families' entry points: launch on `s` with `blocks` workgroups, 0 or the launch error (-22: a form that does not exist) ----
// w2: narrow storage with hi + lo weights (Conv32Args::w2; ignored for fp32 storage) -- instantiated without ReLU on load only
// conv32_s1.hip
int conv32_launch_s1_x3(const Conv32P<float>& p, int flags, bool relu, bool w2, int blocks, hipStream_t s);
int conv32_launch_s1_x3(const Conv32P<bf16_t>& p, int flags, bool relu, bool w2, int blocks, hipStream_t s);
int conv32_launch_s1_small(const Conv32P<float>& p, int flags, bool relu, bool w2, int blocks, hipStream_t s);
int conv32_launch_s1_small(const Conv32P<bf16_t>& p, int flags, bool relu, bool w2, int blocks, hipStream_t s);
int conv32_launch_s2_lds(const Conv32P<float>& p, int flags, bool relu, bool w2, int blocks, hipStream_t s);       // (no bilinear skip: -22 with flags & 1)
int conv32_launch_s2_lds(const Conv32P<bf16_t>& p, int flags, bool relu, bool w2, int blocks, hipStream_t s);
// conv32_strided.hip; mode: CONV_S2 or CONV_T2
int conv32_launch_direct(const Conv32P<float>& p, int mode, int flags, bool relu, bool w2, int blocks, hipStream_t s);
int conv32_launch_direct(const Conv32P<bf16_t>& p, int mode, int flags, bool relu, bool w2, int blocks, hipStream_t s);
// conv32_ref.hip: the validation kernels (p.wpack: ConvW::mf32 / ConvW::canon); exact arithmetic exists for fp32 storage only
int conv32_launch_exact(const Conv32P<float>& p, int mode, int flags, bool relu, int blocks, hipStream_t s);
int conv32_launch_naive(const Conv32P<float>& p, int mode, bool relu, int blocks, hipStream_t s);
int conv32_launch_naive(const Conv32P<bf16_t>& p, int mode, bool relu, int blocks, hipStream_t s);

// ---- what the two one-launch pair forms (conv_pair.hip, conv_tpair.hip) ask of their halves alike --------------------------------------------
// first = f (strided or transposed: the caller checks the mode), second = g (stride 1).  Left to each form: the first half's mode, whether
// the second half's bilinear skip is required or forbidden, the output-sum rule and the size rule.
static inline bool conv32_pair_common(const Conv32Args& f, const Conv32Args& g) {
    if (!f.w || !g.w || !f.in) return false;
    if (g.mode != CONV_S1 || f.bf16 != g.bf16 || f.naive || g.naive || (!f.bf16 && (!f.x3 || !g.x3)) || f.w2 != g.w2) return false;
    if (f.bits_out && (f.bits_sum || f.bf16)) return false;
    if (g.bits_out && g.bf16) return false;
    if (f.w2) {
        // the data gradients (narrow maps, hi + lo weights, no ReLU): first = mask . conv, sum = that + one addend; second reads the SUM, masked
        if (!f.bf16 || f.relu_in || g.relu_in || f.up || g.up || f.bits_out || g.bits_out) return false;
        if (!f.mask || !f.mask_bits || !f.add1 || f.add2 || !f.out_sum) return false;
        if (!g.mask || !g.mask_bits || g.add1 || g.add2 || g.out_sum || !g.out_raw) return false;
    } else {
        // the forward: ReLU on both inputs, first without epilogue operands, second unmasked with up to two addends
        if (!f.relu_in || f.up || f.mask || f.add1 || f.add2 || f.out_sum || f.mask_bits) return false;
        if (!g.relu_in || g.mask || g.mask_bits || (g.add2 && !g.add1) || (!g.out_raw && !g.out_sum)) return false;
    }
    return true;
}
