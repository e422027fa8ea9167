// Device pieces that more than one translation unit of the 32 -> 32 convolutions needs (internal): conv32_ref.hip, conv32_s1.hip,
// conv32_first.hip, conv32_strided.hip, conv32_loop.hip, conv_pair.hip, conv_tpair.hip.  Everything here is __device__ __forceinline__.
// Text that LOOKS shared but is written out per kernel (the register weight-fragment load, the 4 x 32 tile's halo load, staging and 9-tap
// row of conv32_s1_small_kernel and the layer loop, tile_coords of conv32_s2_lds_kernel) stays so on purpose: behind a helper hipcc
// allocated registers differently in those kernels (tools/isa_diff.py, profiles/conv32_split_isa.txt).
#pragma once
#include "ptta_common.h"

// tile heights: the persistent stride-1 kernels walk 8 x 32 tiles (X3_TH, ptta_common.h), the small-map form owns one 4 x 32 tile per
// block (6 halo rows), the LDS-staged stride-2 kernel 4 x 32 output tiles
#define X3S_TH 4
#define X3S_PH 6
#define S2_TH 4

__device__ __forceinline__ unsigned relu_bf2(unsigned v) {
    unsigned neg = (v >> 15) & 0x00010001u;        // sign bit of each packed bf16
    return v & ~(neg * 0xffffu);
}
__device__ __forceinline__ uint4 relu8(uint4 v) {
    v.x = relu_bf2(v.x); v.y = relu_bf2(v.y); v.z = relu_bf2(v.z); v.w = relu_bf2(v.w);
    return v;
}

// ======================================================================================================================
// The tuned kernels.  Every one is a template over the STORAGE type T of its input, output and skip operands:
//   T = float   fp32 maps, "bf16x3" arithmetic: x = xh + xl, w = wh + wl (each half a bf16), x*w ~= xl*wh + xh*wl + xh*wh (the dropped
//               xl*wl term is 2^-16 relative), fp32 accumulate -- the REAL frames' forward, whose output is the scored depth map;
//   T = bf16_t  narrow maps, ONE bf16 MFMA per product ("x1"), fp32 accumulate, one rounding per stored value -- the tensors the reference
//               computes under no_grad / detaches (the zero-image proxy pass, network_exp_msg_chn_adapt.py:509-532) and the data gradients
//               of loss.backward() (src/tta_main.py:632), which reach the scored depth only through an lr-sized Adam move
//               (profiles/r05_precision_budget.txt).  Half the bytes per pixel, a third of the MFMAs, no operand split, no lo planes.
// The two instantiations share every line of tile geometry, prefetch and epilogue structure; they differ in Px<T> (8 channels of a pixel in
// registers), px_stage (ReLU + split while a pixel is written to LDS) and the number of MFMAs per fragment pair.
// ======================================================================================================================

// one (tap, k-step) of the implicit GEMM: a = the lane's A fragment in the LDS tile (hi at a, lo at a + LO); the hi weight fragment is
// wave-stationary in registers (wh), the lo fragment (fp32 storage) comes from LDS (wl).
// (Round 5 measured the narrow kernels with their ONLY weight fragment in LDS as well -- 72 registers less, three resident blocks per CU
// without spills: the full-resolution masked stride-1 launch went from 16.2 to 19.3 us.  At one MFMA per fragment pair the A fragment's
// 1 KB per wave and matrix instruction already takes half of the LDS's 256 B/clk; a second KB for the B fragment saturates it.)
// W2 (narrow storage only): the WEIGHT operand as hi + lo (two MFMAs per product, a . w_lo first) -- the data gradients of the mixed mode.
// A bf16-rounded weight is a SYSTEMATIC 2^-9 error of the gradient's direction, the same for every pixel and every step (a rounded gradient
// value is noise that the sum over the pixels averages out): over a 150-step horizon it was what separated the mixed mode from the
// reference (profiles/r06_drift.txt; CPU simulation tools/precision_sim.py bwd=xw vs bwd=xas).
template <typename T, bool W2 = false>
__device__ __forceinline__ void mma_step(f32x16& acc, const unsigned char* a, const uint4& wh, const unsigned char* wl) {
    const bf16x8 ah = __builtin_bit_cast(bf16x8, *(const uint4*)a);
    const bf16x8 bh = __builtin_bit_cast(bf16x8, wh);
    if constexpr (sizeof(T) == 2 && W2) {
        const bf16x8 bl = __builtin_bit_cast(bf16x8, *(const uint4*)wl);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
    }
    if constexpr (sizeof(T) == 4) {
        const bf16x8 al = __builtin_bit_cast(bf16x8, *(const uint4*)(a + Geo<T>::LO));
        const bf16x8 bl = __builtin_bit_cast(bf16x8, *(const uint4*)wl);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);   // small terms first
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
}
// the block's weight fragments: hi in registers (wh); fp32 storage: lo in LDS
template <typename T, bool W2 = false>
__device__ __forceinline__ void load_weights(uint4 (&wh)[9][2], unsigned char* wl_lds, const void* wpack, const void* wpack2, int tid, int lane) {
    const uint4* ph = (const uint4*)wpack;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int k = 0; k < 2; ++k) wh[t][k] = ph[(t * 2 + k) * 64 + lane];
    if constexpr (sizeof(T) == 4 || W2) {
        const uint4* pl = (const uint4*)wpack2;
        for (int idx = tid; idx < 18 * 64; idx += 256) *(uint4*)(wl_lds + idx * 16) = pl[idx];
    }
}

// the LDS operands of one (tap, k) step in registers and its products -- mma_step split in two so that the reads of a later step can be issued
// in front of the MFMAs of an earlier one (same products in the same order as mma_step)
template <typename T, bool W2> struct FragSet { uint4 ah, al, bl; };
template <typename T, bool W2>
__device__ __forceinline__ void frag_load(FragSet<T, W2>& f, const unsigned char* a, const unsigned char* wl) {
    f.ah = *(const uint4*)a;
    if constexpr (sizeof(T) == 4) { f.al = *(const uint4*)(a + Geo<T>::LO); f.bl = *(const uint4*)wl; }
    else if constexpr (W2) f.bl = *(const uint4*)wl;
}
template <typename T, bool W2>
__device__ __forceinline__ void frag_mma(f32x16& acc, const FragSet<T, W2>& f, const uint4& wh) {
    const bf16x8 ah = __builtin_bit_cast(bf16x8, f.ah), bh = __builtin_bit_cast(bf16x8, wh);
    if constexpr (sizeof(T) == 2 && W2) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, __builtin_bit_cast(bf16x8, f.bl), acc, 0, 0, 0);
    if constexpr (sizeof(T) == 4) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, f.al), bh, acc, 0, 0, 0);   // small terms first
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, __builtin_bit_cast(bf16x8, f.bl), acc, 0, 0, 0);
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
}

// bilinear x2 skip: the half-resolution source window of a tile goes global -> LDS by LDS-DMA (global_load_lds_dwordx4: no registers,
// one 1-KB piece = 8 (fp32) / 16 (narrow) source pixels per wave instruction, lane-linear image [pixel][32 channels], clamped at the borders)
template <typename T, int UPH, int UPW>
__device__ __forceinline__ void up_window_dma(const T* ub, int Hu, int Wu, int uy0, int ux0, unsigned char* up_lds, int tid, int wave) {
    constexpr int PC = Geo<T>::UPPC, N = UPH * UPW * PC;
#pragma unroll
    for (int k = 0; k < (N + 255) / 256; ++k) {
        const int idx = tid + 256 * k;
        if (idx < N) {
            const int q = idx % PC, pix = idx / PC;
            const int r = pix / UPW, cc = pix - r * UPW;
            const int gy = min(uy0 + r, Hu - 1), gx = min(ux0 + cc, Wu - 1);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ub + ((size_t)gy * Wu + gx) * 32 + (32 / PC) * q),
                                             (__attribute__((address_space(3))) void*)(up_lds + (size_t)(256 * k + 64 * wave) * 16), 16, 0, 0);
        }
    }
}


// tile index -> frame and first row / column of its TH x 32 tile (nty x ntx tiles per frame); y fastest: neighbouring blocks share halo
// (window) rows in L2
template <int TH>
__device__ __forceinline__ void tile_coords(long tile, int ntx, int nty, int& b, int& y0, int& x0) {
    long t_ = tile;
    const int ty = (int)(t_ % nty); t_ /= nty;
    const int tx = (int)(t_ % ntx);
    b = (int)(t_ / ntx); y0 = ty * TH; x0 = tx << 5;
}
