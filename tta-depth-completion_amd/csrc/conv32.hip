// 3x3, 32 -> 32 channel convolutions of the MSG_CHN cascade as implicit GEMMs on the matrix cores.
//
// Replaces, for the hot path, every nn.Conv2d(32,32,3) / nn.ConvTranspose2d(32,32,3,s=2) call of
// RGBEncoder / DepthEncoder / DepthDecoder (network_exp_msg_chn_adapt.py:166-311), the meta layer
// conv1_rgb_meta (:1065-1071) and, with re-packed weights, their input gradients (autograd's
// conv backward-data in the reference, src/tta_main.py:632).
//
// Mapping (one wave64 = one 32-pixel x 32-channel output tile, K = 9 taps x 32 input channels):
//   D[pixel][cout] += A[pixel][k] * B[k][cout]
//   fp32 : v_mfma_f32_32x32x2_f32  (exact fp32 FMA chain), 144 MFMAs per tile
//   bf16 : v_mfma_f32_32x32x16_bf16 (fp32 accumulate),      18 MFMAs per tile
// Weights are wave-stationary: the whole 3x3x32x32 filter lives in VGPRs (144 fp32 / 72 bf16
// registers per lane) for the lifetime of a persistent wave that walks over many tiles, so the
// only per-tile traffic is the NHWC input lines (full 128-B / 64-B lines per pixel) and the
// output lines.  ReLU-before-conv, bias, bilinear x2 skip, ReLU-mask (backward) and the decoder's
// skip additions are fused (ptta_common.h Epi).
//
// Three geometries share the body: CONV_S1 (stride 1, pad 1), CONV_S2 (stride 2, pad 1) and
// CONV_T2 (transposed, stride 2, pad 1, output_padding 1; a tile = 32 outputs of one x-parity so
// that the active taps are wave-uniform).
//
// One translation unit per kernel family; this one holds ptta_launch_conv32 alone -- which family a launch takes, its geometry and
// its grid:
//   conv32_ref.hip      conv32_mfma_kernel (exact fp32 MFMA) and conv32_naive_kernel, the validation kernels; the weight packing
//   conv32_s1.hip       the LDS-staged kernels: conv32_s1_x3_kernel (stride 1, persistent 8 x 32 tiles), conv32_s1_small_kernel (stride 1,
//                       small maps) and conv32_s2_lds_kernel (stride 2)
//   conv32_strided.hip  conv32_direct_x3_kernel: stride 2 with the bilinear skip, and transposed
//   conv32_first.hip    conv32_s1_first_kernel: Conv2d(cin <= 3, 32) - ReLU - Conv2d(32, 32) in one launch (ptta_launch_conv32_first)
//   conv32_loop.hip     the layer-loop trial (ptta_launch_conv32_loop)
//   conv32_device.h     the device helpers they share with conv_pair.hip and conv_tpair.hip; conv32_launch.h: the host-side rules
#include "conv32_launch.h"

template <typename T>
static int launch_conv32_t(const Conv32Args& a, hipStream_t s) {
    constexpr bool NAR = sizeof(T) == 2;
    const int mode = a.mode == CONV_S1 ? CONV_S1 : (a.mode == CONV_S2 ? CONV_S2 : CONV_T2);
    const int Hout = mode == CONV_S1 ? a.Hin : (mode == CONV_S2 ? a.Hin / 2 : a.Hin * 2);
    const int Wout = mode == CONV_S1 ? a.Win : (mode == CONV_S2 ? a.Win / 2 : a.Win * 2);
    Conv32P<T> p = conv32_params<T>(a, Hout, Wout);
    if (a.add2 && !a.add1) return -22;
    const int flags = conv32_flags(a);
    const bool relu = a.relu_in != 0;
    // a narrow launch with a ReLU mask takes it as sign bits (the mask map itself is an fp32 map of the real frames)
    if (NAR && a.mask && !a.mask_bits) return -22;
    // one item of the per-row kernels (exact, direct): 32 outputs of one row -- transposed: of one x parity; four items per block and turn
    const int Wt = mode == CONV_T2 ? p.Win : p.Wout;
    const long items = (long)p.B * ((Wt + 31) / 32) * (mode == CONV_T2 ? 2 : 1) * p.Hout;
    if (a.naive) {
        p.wpack = a.w->canon; p.wpack2 = nullptr;
        return conv32_launch_naive(p, mode, relu, conv32_grid(((long)p.B * p.Hout * p.Wout * 32 + 255) / 256, 8192), s);
    }
    if (!NAR && !a.x3) {
        // exact arithmetic (validation): v_mfma_f32_32x32x2_f32, fp32 storage only
        if constexpr (!NAR) {
            p.wpack = (const void*)a.w->mf32; p.wpack2 = nullptr;
            return conv32_launch_exact(p, mode, flags, relu, conv32_grid((items + 3) / 4, kFullChipBlocks), s);
        }
    }
    // the tuned kernels: fp32 storage with bf16x3 arithmetic, or narrow storage (one bf16 MFMA per product; Conv32Args::w2: the weight
    // as hi + lo, the data gradients of the mixed mode -- no ReLU on load, no bilinear skip: the other forms are not instantiated)
    const bool w2 = NAR && a.w2;
    if (w2 && ((flags & 1) || relu)) return -22;
    if (mode == CONV_S1) {
        if (conv32_s1_small_map(p.B, p.Hout, p.Wout))         // the latency-chain form, one 4 x 32 tile per block
            return conv32_launch_s1_small(p, flags, relu, w2, conv32_grid(conv32_tiles(p.B, p.Hout, p.Wout, X3S_TH), kS1SmallBlocks), s);
        return conv32_launch_s1_x3(p, flags, relu, w2, conv32_grid(conv32_tiles(p.B, p.Hout, p.Wout, X3_TH), kS1PersistentBlocks), s);     // 2 resident blocks per CU, persistent
    }
    if (mode == CONV_S2 && !(flags & 1))                      // (the LDS-staged stride-2 kernel has no bilinear epilogue)
        return conv32_launch_s2_lds(p, flags, relu, w2, conv32_grid(conv32_tiles(p.B, p.Hout, p.Wout, S2_TH), kFullChipBlocks), s);
    return conv32_launch_direct(p, mode, flags, relu, w2, conv32_grid((items + 3) / 4, NAR ? kNarrowBlocks : kFullChipBlocks), s);
}

int ptta_launch_conv32(const Conv32Args& a, hipStream_t s) {
    return a.bf16 ? launch_conv32_t<bf16_t>(a, s) : launch_conv32_t<float>(a, s);
}
