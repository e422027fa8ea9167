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
//
// Files (each kernel beside the one table that launches it; heads_device.h holds what they share):
//   heads.hip      this file: the weight packers and ptta_launch_gemm -- validate, choose the form, compute the grid
//   heads_f32.hip  gemm_mfma_kernel, the exact-fp32 GEMM described above
//   heads_x3.hip   gemm_x3_kernel, the tiled bf16x3 GEMM (128- and 32-column tiles)
//   heads_ws.hip   gemm_x3_ws_kernel, the wave-specialised bf16x3 GEMM for N = 512 (and its make DIAG=1 instantiation)
//   heads_bn.hip   the fp64 moment kernels and the BatchNorm1d finalisers
// (heads_n.hip, the narrow heads of the mixed mode, stands on its own.)
#include "heads_device.h"

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
        split2(src[2 * e], src[2 * e + 1], hi, lo);
        w[e] = hl ? lo : hi;
    }
    frag[idx] = make_uint4(w[0], w[1], w[2], w[3]);
}
void ptta_pack_w0_frag(const float* W0, void* frag, hipStream_t s) {
    hipLaunchKernelGGL(pack_w0_frag_kernel, dim3(16), dim3(256), 0, s, W0, (uint4*)frag);
}

int ptta_gemm_row_blocks(int R) { return (R + GEMM_BM - 1) / GEMM_BM; }
// number of row-block partials the launch of `a` writes (every kernel here uses 128-row blocks)
int ptta_gemm_part_blocks(const GemmArgs& a) { return ptta_gemm_row_blocks(a.R); }

static GemmP gemm_params_of_args(const GemmArgs& a) {
    GemmP p;
    p.A = a.A; p.A2 = a.A2; p.W = a.W; p.bias = a.bias; p.C = a.C; p.R = a.R; p.K = a.K; p.N = a.N;
    p.pscale = a.pscale; p.pshift = a.pshift; p.pmean = a.pmean; p.pinv = a.pinv; p.pc1 = a.pc1; p.pc2 = a.pc2;
    p.eH = a.eH; p.escale = a.escale; p.eshift = a.eshift; p.emean = a.emean; p.einv = a.einv; p.part = a.part;
    return p;
}
static GemmX3P gemm_x3_params_of_args(const GemmArgs& a) {
    GemmX3P q; q.g = gemm_params_of_args(a); q.Whi = a.Whi; q.Wlo = a.Wlo; q.Wil = a.Wil;
    q.X = a.X; q.W0frag = (const uint4*)a.W0frag; q.b0 = a.b0; q.W0hi = a.W0hi; q.W0lo = a.W0lo; q.W0thi = a.W0thi; q.W0tlo = a.W0tlo; q.P = a.P;
    q.Bref = a.Bref; q.rowstats = a.rowstats; q.coef = a.coef;
    return q;
}

enum GemmForm { GEMM_F32, GEMM_X3_COLS128, GEMM_X3_COLS32, GEMM_WS };
// which kernel runs `a`: exact fp32 unless bf16x3 arithmetic is asked for on an fp32 A; of the bf16x3 kernels the wave-specialised one
// for N = 512 with an interleaved weight, except behind the BN-backward prologue, which only the tiled kernel has
// (K = 32, the first Linear of proj: routed to the 128x128-tile kernel instead, the step is unchanged within noise --
//  2.317 vs 2.318 ms A/B on one box: that launch is bound by its 55 MB of fp32 stores, not by the tiling)
static GemmForm gemm_form(const GemmArgs& a) {
    if (!(a.x3 && !a.a_bf16)) return GEMM_F32;
    if (a.N == 512 && a.Wil && a.pro != 2) return GEMM_WS;
    return a.N % 128 == 0 ? GEMM_X3_COLS128 : GEMM_X3_COLS32;
}

int ptta_launch_gemm(const GemmArgs& a, hipStream_t s) {
    if (a.K % GEMM_BK || a.N % 32) return -22;
    const GemmForm form = gemm_form(a);
    if (form == GEMM_F32) {
        const int nt = (a.N % 64 == 0) ? 2 : 1;
        return heads_launch_f32(gemm_params_of_args(a), nt, a.pro * 100 + a.epi * 10 + (a.a_bf16 ? 1 : 0),
                                dim3(a.N / (32 * nt), ptta_gemm_row_blocks(a.R)), s);
    }
    if (a.pro == 4 && (!a.Bref || !a.rowstats || !a.coef || a.epi != 3)) return -22;
    if ((a.pro == 3 && (!a.X || !a.W0frag || !a.b0 || !a.pscale || !a.pshift)) ||
        (a.epi == 3 && (!a.X || !a.b0 || !a.W0hi || !a.W0lo || !a.W0thi || !a.W0tlo || !a.P || !a.escale || !a.part))) return -22;
    if ((a.pro == 3 || a.epi == 3) && !(a.N == 512 && a.K == 512 && a.Wil)) return -22;
    const GemmX3P q = gemm_x3_params_of_args(a);
    const int key = a.pro * 10 + a.epi;
    switch (form) {
        case GEMM_WS: return heads_launch_ws(q, key, dim3(2, (a.R + 127) / 128), s);
        case GEMM_X3_COLS128: return heads_launch_x3(q, true, key, dim3(a.N / 128, ptta_gemm_row_blocks(a.R)), s);
        default: return heads_launch_x3(q, false, key, dim3(a.N / 32, ptta_gemm_row_blocks(a.R)), s);
    }
}
