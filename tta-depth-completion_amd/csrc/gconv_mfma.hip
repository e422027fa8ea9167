// Matrix-core path of the generic NHWC convolution (NLSPN backbone): stride-1 3x3 (and 1x1) convolutions with any
// channel counts that are multiples of 8, one or two channel-concatenated sources, fp32 storage, bf16x3 arithmetic
// (x = xh + xl, w = wh + wl; xl*wh + xh*wl + xh*wh on v_mfma_f32_32x32x16_bf16, fp32 accumulate) -- the same
// arithmetic as the MSG_CHN hot path (conv32.hip and its kernel files conv32_*.hip), generalised over input-channel chunks and output-channel tiles.
// One translation unit per kernel family, each with the launcher that owns its instantiation table:
//   gconv_x3_s1.hip       gconv_x3_s1_kernel (stride 1, LDS-staged), ptta_gconv_x3_tiles, ptta_launch_gconv_x3
//   gconv_x3_strided.hip  gconv_x3_direct_kernel (stride 2 and transposed), ptta_gconv_x3_strided_form, ptta_launch_gconv_x3_strided
//   gwgrad_mfma.hip       the 3x3 weight gradient (fp32-MFMA, bf16x3, their reducer), ptta_launch_gwgrad_mfma / _f32mfma
//   gconv_device.h        what the two convolution units share
// This file keeps the packer of the weight fragments that the two convolution kernels read.
#include "ptta_common.h"
#include "ptta_kernels.h"

namespace {

// fragment (nf, chunk, tap, kk): lane l holds column co = 32 nf + (l & 31), rows ci = 32 chunk + 16 kk + 8 (l >> 5) + e
__global__ void gfrag_pack_kernel(const float* __restrict__ canon, long wld, long wts, int KK, int C0, int C1, int c0_0, int c0_1,
                                  int Co, int nchunks, int nf_total, bf16_t* __restrict__ hi, bf16_t* __restrict__ lo, bf16_t* __restrict__ l2) {
    const long total = (long)nf_total * nchunks * KK * 2 * 64 * 8;
    const int nch0 = (C0 + 31) / 32;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int e = (int)(idx & 7); long t_ = idx >> 3;
        const int lane = (int)(t_ & 63); t_ >>= 6;
        const int kk = (int)(t_ & 1); t_ >>= 1;
        const int t = (int)(t_ % KK); t_ /= KK;
        const int c = (int)(t_ % nchunks); const int nf = (int)(t_ / nchunks);
        const int s = c < nch0 ? 0 : 1;
        const int cl = (s == 0 ? c : c - nch0) * 32 + kk * 16 + (lane >> 5) * 8 + e;
        const int Cs = s == 0 ? C0 : C1;
        const int co = nf * 32 + (lane & 31);
        float v = 0.f;
        if (cl < Cs && co < Co) v = canon[(long)t * wts + (long)((s == 0 ? c0_0 : c0_1) + cl) * wld + co];
        const bf16_t h = f2bf(v);
        const float r = v - bf2f(h);
        const bf16_t m = f2bf(r);
        hi[idx] = h; lo[idx] = m;
        if (l2) l2[idx] = f2bf(r - bf2f(m));
    }
}

}  // namespace

void ptta_gfrag_pack(const float* canon, long wld, long wts, int KK, int C0, int C1, int c0_0, int c0_1, int Co, bf16_t* hi, bf16_t* lo,
                     hipStream_t s, bf16_t* l2) {
    const int nchunks = (C0 + 31) / 32 + (C1 + 31) / 32, nf_total = (Co + 31) / 32;
    const long total = (long)nf_total * nchunks * KK * 2 * 64 * 8;
    long blocks = (total + 255) / 256; if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(gfrag_pack_kernel, dim3((int)blocks), dim3(256), 0, s, canon, wld, wts, KK, C0, C1, c0_0, c0_1, Co, nchunks, nf_total, hi, lo, l2);
}
long ptta_gfrag_elems(int KK, int C0, int C1, int Co) {
    return (long)((Co + 31) / 32) * ((C0 + 31) / 32 + (C1 + 31) / 32) * KK * 2 * 64 * 8;
}
