// Entry points that take no handle: outlier removal, evaluation metrics, the modulated deformable convolution, and the
// stand-alone operator launches tests and tools/ time (ptta_op_conv32, ptta_op_gwgrad, ptta_op_gconv, ptta_op_gconv_affine, ptta_op_gbn, ptta_op_conv32_chain,
// CostDCNet's own kernels: ptta_cd_sparse_*, ptta_op_cd_sparse_conv, ptta_op_cd_sbn, ptta_op_cd_densify, ptta_op_cd_dense, and the MSG_CHN
// step's first-layer / prediction convolutions, resamplings and loss: ptta_op_conv_in, ptta_op_conv_out1, ptta_op_prep, ptta_op_up2_1ch,
// ptta_op_up2t_1ch, ptta_op_up2t_32, ptta_op_loss; NLSPN's propagation gradients in both forms: ptta_op_nl_prop_bwd, ptta_op_nl_affinity_bwd;
// the mixed mode's narrow heads: ptta_op_hn_gemm, ptta_op_hn_moments, ptta_op_hn_untile, ptta_op_head_bwd_finish).
#include "msgchn_ctx.h"
#include "gnet.h"
#include "costdc.h"

using namespace msgchn;

namespace {
// the four packed images of one 32 -> 32 weight, owned for the length of a stand-alone operator call
struct ScratchConvW {
    ConvW w{};
    bool ok;
    ScratchConvW() {
        ok = hipMalloc((void**)&w.mf32, 9 * 4 * 64 * 4 * 4) == hipSuccess && hipMalloc((void**)&w.mbf16, 9 * 2 * 64 * 8 * 2) == hipSuccess &&
             hipMalloc((void**)&w.canon, 9216 * 4) == hipSuccess && hipMalloc((void**)&w.mlo, 9 * 2 * 64 * 8 * 2) == hipSuccess;
    }
    ~ScratchConvW() { (void)hipFree(w.mf32); (void)hipFree(w.mbf16); (void)hipFree(w.mlo); (void)hipFree(w.canon); }
    ScratchConvW(const ScratchConvW&) = delete;
    ScratchConvW& operator=(const ScratchConvW&) = delete;
};

// ptta_op_gbn's stand-in for the SyncBatchNorm collective: every rank holds the same data, so the sum over `world` ranks is a product
__global__ void op_scale_f64_kernel(double* buf, long long n, double f) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) buf[i] *= f;
}
int op_gbn_exchange(void* user, double* buf, long long count, void* stream) {
    long long blocks = (count + 255) / 256; if (blocks > 1024) blocks = 1024; if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(op_scale_f64_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, buf, count, (double)*(const int*)user);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
}  // namespace

extern "C" {

int ptta_outlier_removal(const float* sparse, const float* validity, float* sparse_out, float* validity_out, int n, int height,
                         int width, int kernel_size, float threshold, float* scratch, ptta_stream s) {
    if (!sparse || !validity || !sparse_out || !validity_out || !scratch || n < 1 || height < 1 || width < 1 || kernel_size < 1 ||
        (kernel_size & 1) == 0) return -22;
    return ptta_launch_outlier_removal(sparse, validity, sparse_out, validity_out, n, height, width, kernel_size, threshold, scratch,
                                       (hipStream_t)s);
}

int ptta_eval_metrics(const float* depth, const float* ground_truth, int64_t numel, float min_evaluate_depth, float max_evaluate_depth,
                      void* scratch, float* metrics_out, ptta_stream s) {
    if (!depth || !ground_truth || !scratch || !metrics_out || numel < 1) return -22;
    return ptta_launch_eval_metrics(depth, ground_truth, numel, min_evaluate_depth, max_evaluate_depth, (double*)scratch, metrics_out,
                                    (hipStream_t)s);
}

static void dcn_args(DcnArgs& a, const float* input, const float* weight, const float* bias, const float* offset, const float* mask,
                     int b, int c, int h, int w, int c_out, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int group, int dg) {
    a.in = input; a.weight = weight; a.bias = bias; a.offset = offset; a.mask = mask;
    a.B = b; a.C = c; a.H = h; a.W = w; a.Co = c_out; a.kh = kh; a.kw = kw; a.sh = sh; a.sw = sw; a.ph = ph; a.pw = pw;
    a.dh = dh; a.dw = dw; a.group = group; a.dg = dg;
}

int ptta_mdconv_forward(const float* input, const float* weight, const float* bias, const float* offset, const float* mask, float* output,
                        int b, int c, int h, int w, int c_out, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                        int group, int deformable_group, ptta_stream s) {
    if (!input || !weight || !offset || !mask || !output) return -22;
    DcnArgs a; dcn_args(a, input, weight, bias, offset, mask, b, c, h, w, c_out, kh, kw, sh, sw, ph, pw, dh, dw, group, deformable_group);
    a.out = output;
    return ptta_launch_dcn_forward(a, (hipStream_t)s);
}

int ptta_mdconv_backward(const float* input, const float* weight, const float* bias, const float* offset, const float* mask,
                         const float* grad_output, float* grad_input, float* grad_offset, float* grad_mask, float* grad_weight,
                         float* grad_bias, int b, int c, int h, int w, int c_out, int kh, int kw, int sh, int sw, int ph, int pw,
                         int dh, int dw, int group, int deformable_group, ptta_stream s) {
    if (!input || !weight || !offset || !mask || !grad_output) return -22;
    DcnArgs a; dcn_args(a, input, weight, bias, offset, mask, b, c, h, w, c_out, kh, kw, sh, sw, ph, pw, dh, dw, group, deformable_group);
    a.gout = grad_output; a.gin = grad_input; a.goff = grad_offset; a.gmask = grad_mask; a.gweight = grad_weight; a.gbias = grad_bias;
    return ptta_launch_dcn_backward(a, (hipStream_t)s);
}

// Stand-alone 32->32 3x3 convolution on fp32 NHWC buffers (tests only): packs `weight`, converts
// to the requested storage type, runs the hot-path kernel and converts back.
int ptta_op_conv32(const float* in, const float* weight, const float* bias, float* out, int b, int hin, int win, int mode,
                   int relu_in, int in_major, int flip, int dtype, int naive, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    ScratchConvW sw; ConvW& w = sw.w;
    void *tin = nullptr, *tout = nullptr;
    const int ho = mode == CONV_S1 ? hin : (mode == CONV_S2 ? hin / 2 : hin * 2), wo = mode == CONV_S1 ? win : (mode == CONV_S2 ? win / 2 : win * 2);
    const long nin = (long)b * hin * win * 32, nout = (long)b * ho * wo * 32;
    int rc = 0;
    if (!sw.ok || hipMalloc(&tin, nin * 2) != hipSuccess || hipMalloc(&tout, nout * 2) != hipSuccess) rc = -12;
    if (rc == 0) {
        ptta_pack_conv32(weight, w, in_major, flip, s);
        Conv32Args a; a.w = &w; a.bias = bias; a.B = b; a.Hin = hin; a.Win = win; a.mode = mode; a.relu_in = relu_in; a.naive = naive & 1; a.x3 = (naive >> 1) & 1;
        if (dtype != PTTA_DTYPE_F32) {             // narrow storage (bf16 maps, one MFMA per product): the kernels of the mixed mode
            from_f32_launch(in, (bf16_t*)tin, nin, s);
            a.in = tin; a.in_nb = b; a.out_raw = tout; a.bf16 = 1;
            rc = ptta_launch_conv32(a, s);
            to_f32_launch((const bf16_t*)tout, out, nout, s);
        } else {
            a.in = in; a.in_nb = b; a.out_raw = out; a.bf16 = 0;
            rc = ptta_launch_conv32(a, s);
        }
        (void)hipStreamSynchronize(s);
    }
    (void)hipFree(tin); (void)hipFree(tout);
    return rc;
}

// Stand-alone (strided -> stride-1) pair of 32->32 3x3 convolutions on fp32 NHWC buffers (tests only), as the engine issues such a pair:
// first layer: optional ReLU-mask (sign-bit words mask1_bits [b][hm][wm]) and addend add0 [b][hm][wm][32] -- its SUM is then what the second
// layer reads; second layer: bilinear x2 skip `up` [b][hm/2][wm/2][32], skip addends add1 / add2, ReLU-mask mask2_bits (each may be null).
// fused = 1: the one-launch form where it applies (conv_pair.hip), else -- and with fused = 0 -- the two launches; *fused_host tells which ran.
// Outputs (each may be null): the second layer's map and sum, the first layer's map, sum and -- PTTA_DTYPE_F32 -- its sign-bit words.
// (tform < 0: the one-launch form of conv_pair.hip; tform 0 / 1 / 2: that of conv_tpair.hip in this form, its grid capped at max_blocks)
static int op_conv32_pair_body(const float* in, const float* weight1, const float* bias1, const float* weight2, const float* bias2, const float* up,
                               const float* add0, const float* add1, const float* add2, const uint32_t* mask1_bits, const uint32_t* mask2_bits,
                               float* out_raw, float* out_sum, float* mid_raw, float* mid_sum, uint32_t* mid_bits, int b, int in_nb,
                               int hin, int win, int first_mode, int relu1, int relu2, int in_major, int flip, int dtype, int w2, int fused,
                               int* fused_host, int tform, int max_blocks, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!in || !weight1 || !weight2 || (!out_raw && !out_sum) || b < 1 || in_nb < 1 || in_nb > b || hin < 1 || win < 1 ||
        (first_mode != CONV_S2 && first_mode != CONV_T2) || (add2 && !add1) || (add1 && !out_sum)) return -22;
    const bool nar = dtype != PTTA_DTYPE_F32;
    if (w2 && (!nar || relu1 || relu2 || up)) return -22;           // (the hi + lo weight form exists for the narrow data gradients only)
    const int hm = first_mode == CONV_S2 ? hin / 2 : hin * 2, wm = first_mode == CONV_S2 ? win / 2 : win * 2;
    if (hm < 1 || wm < 1) return -22;
    const long nin = (long)in_nb * hin * win * 32, nm = (long)b * hm * wm * 32, nu = (long)b * (hm / 2) * (wm / 2) * 32;
    ScratchConvW sw1, sw2;
    // device buffers in the storage type: [0] in, [1] up, [2] add0, [3] add1, [4] add2, [5] mid, [6] mid sum, [7] out_raw, [8] out_sum
    void* t[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const long cnt[9] = {nin, up ? nu : 0, add0 ? nm : 0, add1 ? nm : 0, add2 ? nm : 0, nm, add0 ? nm : 0, out_raw ? nm : 0, out_sum ? nm : 0};
    const float* src[5] = {in, up, add0, add1, add2};
    const int es = nar ? 2 : 4;
    int rc = (sw1.ok && sw2.ok) ? 0 : -12;
    for (int k = 0; k < 9 && !rc; ++k) if (cnt[k] > 0 && hipMalloc(&t[k], (size_t)cnt[k] * es) != hipSuccess) rc = -12;
    if (!rc) {
        ptta_pack_conv32(weight1, sw1.w, in_major, flip, s);
        ptta_pack_conv32(weight2, sw2.w, 0, 0, s);
        for (int k = 0; k < 5; ++k) {
            if (cnt[k] <= 0) continue;
            if (nar) from_f32_launch(src[k], (bf16_t*)t[k], cnt[k], s);
            else if (hipMemcpyAsync(t[k], src[k], (size_t)cnt[k] * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) rc = -5;
        }
        (void)hipMemsetAsync(t[5], 0xff, (size_t)nm * es, s);         // (a fused launch that skipped a pixel of a side output shows as NaN)
        if (t[6]) (void)hipMemsetAsync(t[6], 0xff, (size_t)nm * es, s);
    }
    if (!rc) {
        Conv32Args f, g;
        f.in = t[0]; f.in_nb = in_nb; f.w = &sw1.w; f.bias = bias1; f.out_raw = t[5]; f.B = b; f.Hin = hin; f.Win = win; f.mode = first_mode;
        f.relu_in = relu1; f.bf16 = nar ? 1 : 0; f.x3 = 1; f.w2 = w2;
        if (add0) { f.add1 = t[2]; f.add1_nb = b; f.out_sum = t[6]; }
        if (mask1_bits) { f.mask = mask1_bits; f.mask_nb = b; f.mask_bits = mask1_bits; }      // (the kernels read the bit plane only)
        if (!nar && mid_bits) { f.bits_out = mid_bits; f.bits_nb = b; }
        g.in = add0 ? t[6] : t[5]; g.in_nb = b; g.w = &sw2.w; g.bias = bias2; g.up = t[1]; g.up_nb = b;
        g.add1 = t[3]; g.add1_nb = b; g.add2 = t[4]; g.add2_nb = b;
        if (mask2_bits) { g.mask = mask2_bits; g.mask_nb = b; g.mask_bits = mask2_bits; }
        g.out_raw = t[7]; g.out_sum = t[8]; g.B = b; g.Hin = hm; g.Win = wm; g.mode = CONV_S1; g.relu_in = relu2; g.bf16 = nar ? 1 : 0; g.x3 = 1; g.w2 = w2;
        int did = 0;
        if (!fused) rc = 1;
        else if (tform < 0) rc = ptta_launch_conv32_pair(f, g, s);
        else {
            Conv32Args ff = f;
            if (!mid_raw) ff.out_raw = nullptr;                      // (no reader of the first half's map: the one-launch form does not write it)
            rc = ptta_launch_conv32_tpair(ff, g, tform, max_blocks, s);
        }
        if (rc == 0) did = 1;
        if (rc == 0 && tform >= 0 && !mid_raw) {
            // the one-launch form was told not to write the first half's map: its buffer must still hold the fill
            std::vector<unsigned char> hb((size_t)nm * es);
            if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(hb.data(), t[5], hb.size(), hipMemcpyDeviceToHost) != hipSuccess) rc = -5;
            else for (unsigned char ch : hb) if (ch != 0xff) { rc = -14; break; }
        }
        if (rc == 1) { rc = ptta_launch_conv32(f, s); if (!rc) rc = ptta_launch_conv32(g, s); }
        if (fused_host) *fused_host = did;
    }
    if (!rc) {
        float* dst[4] = {mid_raw, mid_sum, out_raw, out_sum};
        for (int k = 0; k < 4; ++k) {
            if (!dst[k] || !t[5 + k]) continue;
            if (nar) to_f32_launch((const bf16_t*)t[5 + k], dst[k], nm, s);
            else if (hipMemcpyAsync(dst[k], t[5 + k], (size_t)nm * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) rc = -5;
        }
    }
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    for (int k = 0; k < 9; ++k) (void)hipFree(t[k]);
    return rc;
}

int ptta_op_conv32_pair(const float* in, const float* weight1, const float* bias1, const float* weight2, const float* bias2, const float* up,
                        const float* add0, const float* add1, const float* add2, const uint32_t* mask1_bits, const uint32_t* mask2_bits,
                        float* out_raw, float* out_sum, float* mid_raw, float* mid_sum, uint32_t* mid_bits, int b, int in_nb,
                        int hin, int win, int first_mode, int relu1, int relu2, int in_major, int flip, int dtype, int w2, int fused,
                        int* fused_host, ptta_stream s_) {
    return op_conv32_pair_body(in, weight1, bias1, weight2, bias2, up, add0, add1, add2, mask1_bits, mask2_bits, out_raw, out_sum, mid_raw, mid_sum,
                               mid_bits, b, in_nb, hin, win, first_mode, relu1, relu2, in_major, flip, dtype, w2, fused, fused_host, -1, 0, s_);
}
// The same pair with the one-launch form of conv_tpair.hip (a TRANSPOSED first half): form 0 = as the step would choose by the map size,
// 1 = 4 x 32 one-tile blocks, 2 = persistent 8 x 32 tiles; max_blocks > 0 caps the grid so that a small map makes a block walk several
// tiles.  With mid_raw null the one-launch form does not write the first half's map (its sign-bit words still are).
int ptta_op_conv32_tpair(const float* in, const float* weight1, const float* bias1, const float* weight2, const float* bias2, const float* up,
                         const float* add0, const float* add1, const float* add2, const uint32_t* mask1_bits, const uint32_t* mask2_bits,
                         float* out_raw, float* out_sum, float* mid_raw, float* mid_sum, uint32_t* mid_bits, int b, int in_nb,
                         int hin, int win, int first_mode, int relu1, int relu2, int in_major, int flip, int dtype, int w2, int fused,
                         int form, int max_blocks, int* fused_host, ptta_stream s_) {
    if (form < 0 || form > 2 || max_blocks < 0) return -22;
    return op_conv32_pair_body(in, weight1, bias1, weight2, bias2, up, add0, add1, add2, mask1_bits, mask2_bits, out_raw, out_sum, mid_raw, mid_sum,
                               mid_bits, b, in_nb, hin, win, first_mode, relu1, relu2, in_major, flip, dtype, w2, fused, fused_host, form, max_blocks, s_);
}

// ---- MSG_CHN's first-layer / prediction convolutions, resamplings and loss, stand-alone (tests/test_gpu_msgchn_elementwise.py) ----------
// device allocations of one hook call, freed when it returns
struct OpBufs {
    std::vector<void*> v; bool ok = true;
    void* get(size_t bytes) {
        void* p = nullptr;
        if (!ok || hipMalloc(&p, bytes ? bytes : 4) != hipSuccess) { ok = false; return nullptr; }
        v.push_back(p);
        return p;
    }
    ~OpBufs() { for (void* p : v) (void)hipFree(p); }
};
static bool op_al(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }
// a 32-channel fp32 map in the launch's storage type: itself, or a narrow copy
static const void* op_narrow_in(OpBufs& m, const float* src, long n, bool nar, hipStream_t s) {
    if (!src || !nar) return src;
    void* t = m.get((size_t)n * 2);
    if (t) from_f32_launch(src, (bf16_t*)t, n, s);
    return t;
}
// ... and an output: the caller's buffer, or a NaN-filled narrow one converted back by op_narrow_back
static void* op_narrow_out(OpBufs& m, float* dst, long n, bool nar, hipStream_t s) {
    if (!dst || !nar) return dst;
    void* t = m.get((size_t)n * 2);
    if (t) (void)hipMemsetAsync(t, 0xff, (size_t)n * 2, s);
    return t;
}
static void op_narrow_back(const void* t, float* dst, long n, bool nar, hipStream_t s) {
    if (dst && nar && t) to_f32_launch((const bf16_t*)t, dst, n, s);
}

int ptta_op_conv_in(const ptta_conv_in_args* a, int* form_host, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!a || !a->weight || (!a->out_raw && !a->out_sum) || a->cin < 1 || a->cin > 3 || a->b < 1 || a->h < 1 || a->w < 1 || a->zero_from_b < 0 ||
        a->max_blocks < 0 || a->a_bits_nb < 0 || a->a_bits_nb > a->b) return -22;
    if (a->transpose_flip ? a->cin != 1 : (a->cin_first < 0 || a->cin_total < 1 || a->cin_first + a->cin > a->cin_total)) return -22;
    for (int c = 0; c < a->cin; ++c)
        if (!a->pl[c].p || !op_al(a->pl[c].p, 4) || a->pl[c].nb < 1 || a->pl[c].nb > a->b) return -22;
    const bool nar = a->dtype != PTTA_DTYPE_F32, hasmask = a->mask || a->mask_bits;
    if (a->up && ((a->h & 1) || (a->w & 1) || a->up_nb < 1 || a->up_nb > a->b)) return -22;
    if (hasmask && (a->mask_nb < 1 || a->mask_nb > a->b)) return -22;
    if (a->add1 && (a->add1_nb < 1 || a->add1_nb > a->b || !a->out_sum)) return -22;
    if (nar && a->mask && !a->mask_bits) return -22;            // the launcher's own refusal, ahead of the allocations
    ConvInArgs k;
    k.cin = a->cin; k.naive = a->naive ? 1 : 0; k.up = a->up; k.add1 = a->add1;
    k.mask = a->mask ? (const void*)a->mask : (const void*)a->mask_bits;          // (non-null selects the masked kernels; a narrow launch reads the words only)
    const int form = ptta_conv_in_form(k);
    const bool lds = form == CONV_IN_FORM_LDS || form == CONV_IN_FORM_LDS_MASK;
    if (!lds && hasmask && (nar || !a->mask)) return -22;      // the direct and naive kernels read the mask as a map of the storage type
    if (a->a_bits && a->a_bits_nb > 0 && (nar || !lds)) return -22;
    if (!op_al(a->up, 16) || !op_al(a->mask, 16) || !op_al(a->add1, 16) || !op_al(a->out_raw, 16) || !op_al(a->out_sum, 16) ||
        !op_al(a->mask_bits, 4) || !op_al(a->a_bits, 4) || !op_al(a->weight, 4) || !op_al(a->bias, 4)) return -22;
    const long plane = (long)a->h * a->w, nmap = (long)a->b * plane * 32;
    OpBufs m;
    float* wfrag = (float*)m.get(14 * 64 * 4);
    float* wcanon = (float*)m.get(27 * 32 * 4);
    if (wcanon) (void)hipMemsetAsync(wcanon, 0xff, 27 * 32 * 4, s);
    k.up = op_narrow_in(m, a->up, (long)a->up_nb * (a->h / 2) * (a->w / 2) * 32, nar, s); k.up_nb = a->up_nb;
    k.add1 = op_narrow_in(m, a->add1, (long)a->add1_nb * plane * 32, nar, s); k.add1_nb = a->add1_nb;
    k.out_raw = op_narrow_out(m, a->out_raw, nmap, nar, s);
    k.out_sum = op_narrow_out(m, a->out_sum, nmap, nar, s);
    if (!m.ok) return -12;
    ptta_pack_conv_in(a->weight, a->cin_total, a->cin_first, a->cin, a->transpose_flip, wfrag, wcanon, s);
    for (int c = 0; c < a->cin; ++c) {
        Plane& p = k.pl[c];
        p.p = a->pl[c].p; p.nb = a->pl[c].nb; p.bstride = plane; p.norm = a->pl[c].norm ? 1 : 0;
        p.div = a->pl[c].div; p.mean = a->pl[c].mean; p.stdv = a->pl[c].stdv;
    }
    k.zero_from_b = a->zero_from_b; k.wfrag = wfrag; k.wcanon = wcanon; k.bias = a->bias;
    k.mask_nb = hasmask ? a->mask_nb : 1; k.mask_bits = a->mask_bits;
    k.B = a->b; k.H = a->h; k.W = a->w; k.bf16 = nar ? 1 : 0;
    k.a_bits = a->a_bits; k.a_bits_nb = a->a_bits ? a->a_bits_nb : 0; k.max_blocks = a->max_blocks;
    int rc = ptta_launch_conv_in(k, s);
    if (rc > 0) rc = -5;
    if (!rc) { op_narrow_back(k.out_raw, a->out_raw, nmap, nar, s); op_narrow_back(k.out_sum, a->out_sum, nmap, nar, s); }
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    if (form_host) *form_host = form;
    return rc;
}

int ptta_op_conv_out1(const ptta_conv_out1_args* a, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!a || !a->in || !a->weight || !a->out || a->b < 1 || a->h < 1 || a->w < 1 || a->in_nb < 1 || a->in_nb > a->b || a->max_blocks < 0) return -22;
    if (a->add && (a->add_nb < 1 || a->add_nb > a->b)) return -22;
    if (a->from_conv_in && (a->src_cin_total < 1 || a->src_cin_index < 0 || a->src_cin_index >= a->src_cin_total)) return -22;
    if (!op_al(a->in, 16) || !op_al(a->weight, 4) || !op_al(a->bias, 4) || !op_al(a->add, 4) || !op_al(a->out, 4)) return -22;
    const bool nar = a->dtype != PTTA_DTYPE_F32;
    OpBufs m;
    float* w = (float*)m.get(288 * 4);
    ConvOut1Args k;
    k.in = op_narrow_in(m, a->in, (long)a->in_nb * a->h * a->w * 32, nar, s); k.in_nb = a->in_nb;
    if (!m.ok) return -12;
    ptta_pack_conv_out1(a->weight, a->src_cin_total, a->src_cin_index, a->from_conv_in ? 1 : 0, w, s);
    k.w = w; k.bias = a->bias; k.add = a->add; k.add_nb = a->add ? a->add_nb : 1; k.out = a->out;
    k.B = a->b; k.H = a->h; k.W = a->w; k.relu_in = a->relu_in ? 1 : 0; k.bf16 = nar ? 1 : 0; k.max_blocks = a->max_blocks;
    int rc = ptta_launch_conv_out1(k, s);
    if (rc > 0) rc = -5;
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    return rc;
}

int ptta_op_prep(const float* sparse, float max_input_depth, float* dclamp, float* d12, float* d14, int n, int h, int w, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!sparse || !dclamp || !d12 || !d14 || n < 1 || h < 4 || w < 4 || (h & 3) || (w & 3) || !op_al(sparse, 16) || !op_al(dclamp, 16) ||
        !op_al(d12, 4) || !op_al(d14, 4)) return -22;
    int rc = ptta_launch_prep(sparse, max_input_depth, dclamp, d12, d14, n, h, w, s);
    if (rc > 0) rc = -5;
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    return rc;
}

// (one block row per map row, one block plane per image: both are grid dimensions)
static bool op_up2_ok(const void* a, const void* b, int n, int hin, int win) {
    return a && b && n >= 1 && n <= 65535 && hin >= 1 && 2 * (long)hin <= 65535 && win >= 1 && win <= (1 << 20);
}
int ptta_op_up2_1ch(const float* in, float* out, int b, int hin, int win, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!op_up2_ok(in, out, b, hin, win) || !op_al(in, 4) || !op_al(out, 4)) return -22;
    int rc = ptta_launch_up2_1ch(in, out, b, hin, win, s);
    if (rc > 0) rc = -5;
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    return rc;
}
int ptta_op_up2t_1ch(const float* gout, float* gin, int b, int hin, int win, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!op_up2_ok(gout, gin, b, hin, win) || !op_al(gout, 4) || !op_al(gin, 4)) return -22;
    int rc = ptta_launch_up2T_1ch(gout, gin, b, hin, win, s);
    if (rc > 0) rc = -5;
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    return rc;
}
int ptta_op_up2t_32(const float* gout, const float* add, float* gin, int b, int hin, int win, int dtype, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!op_up2_ok(gout, gin, b, hin, win) || !op_al(gout, 16) || !op_al(add, 16) || !op_al(gin, 16)) return -22;
    const bool nar = dtype != PTTA_DTYPE_F32;
    const long nin = (long)b * hin * win * 32;
    OpBufs m;
    const void* g = op_narrow_in(m, gout, 4 * nin, nar, s);
    const void* ad = op_narrow_in(m, add, nin, nar, s);
    void* o = op_narrow_out(m, gin, nin, nar, s);
    if (!m.ok) return -12;
    int rc = ptta_launch_up2T_32(g, ad, o, b, hin, win, nar ? 1 : 0, s);
    if (rc > 0) rc = -5;
    if (!rc) op_narrow_back(o, gin, nin, nar, s);
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    return rc;
}

int ptta_op_loss(const ptta_loss_args* a, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!a || !a->depth || !a->image || !a->sparse || a->n < 1 || a->n > 65535 || a->h < 2 || a->w < 2 || a->fwd < PTTA_LOSS_FWD_MERGED ||
        a->fwd > PTTA_LOSS_FWD_SPLIT_NARROW || a->bwd < PTTA_LOSS_BWD_NONE || a->bwd > PTTA_LOSS_BWD_COUNTED) return -22;
    const bool cos = a->fwd != PTTA_LOSS_FWD_NOCOS, split = a->fwd >= PTTA_LOSS_FWD_SPLIT, nar = a->fwd == PTTA_LOSS_FWD_SPLIT_NARROW;
    if (cos && (!a->emb || !a->ref || a->r < 1 || a->d < 4 || a->d % (nar ? 8 : 4) != 0 || !op_al(a->emb, 16) || !op_al(a->ref, 16) || !op_al(a->gref, 16))) return -22;
    if (!cos && (a->gref || a->rowstats)) return -22;
    if ((a->bwd == PTTA_LOSS_BWD_FUSED && split) || (a->bwd == PTTA_LOSS_BWD_COUNTED && !split)) return -22;
    if (a->bwd != PTTA_LOSS_BWD_NONE ? !a->gdepth : (a->gdepth || a->gref)) return -22;
    const int N = a->n, H = a->h, W = a->w, D = a->d;
    const long R = cos ? (long)a->r : 0;
    if ((double)N * H * W > 2.0e9 || (double)R * D > 2.0e9 || ptta_loss_ws_rows_off(N) + 3.0 * R > 2.0e9) return -22;
    const long plane = (long)H * W, nws = ptta_loss_ws_floats(N, H, W, R);
    OpBufs m;
    float* ws = (float*)m.get((size_t)nws * 4);
    float* w3 = (float*)m.get(16);
    float* info = (float*)m.get(16);
    float* gscratch = (a->bwd == PTTA_LOSS_BWD_COUNTED && a->gref) ? (float*)m.get((size_t)N * plane * 4) : nullptr;
    const void *en = a->emb, *rn = a->ref;
    if (nar) { en = op_narrow_in(m, a->emb, R * D, true, s); rn = op_narrow_in(m, a->ref, R * D, true, s); }
    if (!m.ok) return -12;
    (void)hipMemsetAsync(ws, 0xff, (size_t)nws * 4, s);
    (void)hipMemsetAsync(info, 0xff, 16, s);
    const float w3h[3] = {a->w_sd, a->w_sm, a->w_cos};
    const float *e = cos ? a->emb : nullptr, *r = cos ? a->ref : nullptr;
    const float maxd = a->max_input_depth;
    int rc = ptta_launch_set_floats(w3, w3h, 3, s);
#define OPL_(call) do { if (!rc) rc = (call); } while (0)
    if (a->bwd != PTTA_LOSS_BWD_COUNTED) {
        const int fused = a->bwd == PTTA_LOSS_BWD_FUSED;
        if (!split) OPL_(ptta_launch_loss_forward(a->depth, a->image, a->sparse, a->validity, maxd, e, r, R, D, w3, N, H, W, ws, info, s, fused));
        else {
            OPL_(ptta_launch_loss_depth_part(a->depth, a->image, a->sparse, a->validity, maxd, N, H, W, ws, s));
            OPL_(ptta_launch_loss_cos_part(en, rn, R, D, N, ws, s, nar ? 1 : 0));
            OPL_(ptta_launch_loss_finalize(ws, N, H, W, R, 1, w3, info, s));
        }
        if (a->bwd == PTTA_LOSS_BWD_UNFUSED)
            OPL_(ptta_launch_loss_backward(a->depth, a->image, a->sparse, a->validity, maxd, e, r, R, D, N, H, W, ws, a->gdepth, a->gref, s));
        if (fused)
            OPL_(ptta_launch_loss_backward(a->depth, a->image, a->sparse, a->validity, maxd, e, r, R, D, N, H, W, ws, a->gdepth, a->gref, s, w3, info));
    } else {
        // the thru step (msgchn_step.hip step_tail): the valid-weight partials first, the cosine rows and their coefficient, the depth gradient
        // from the partials alone; the loss VALUES behind it (msgchn_backward.hip) -- in front of it beyond PTTA_LOSS_FIN_MAXN, where the
        // gradient launch reads the finalised workspace
        OPL_(ptta_launch_loss_valid_count(a->sparse, a->validity, N, H, W, ws, s));
        OPL_(ptta_launch_loss_cos_part(en, rn, R, D, N, ws, s, nar ? 1 : 0));
        OPL_(ptta_launch_loss_cos_coef(ws, N, R, w3, s));
        if (!rc && a->coef && hipMemcpyAsync(a->coef + 3 + N, ws + PTTA_LOSS_WS_SCAL, 4, hipMemcpyDeviceToDevice, s) != hipSuccess) rc = -5;
        for (int pass = 0; pass < 2; ++pass) {
            if ((N > PTTA_LOSS_FIN_MAXN) == (pass == 0)) {
                OPL_(ptta_launch_loss_depth_part(a->depth, a->image, a->sparse, a->validity, maxd, N, H, W, ws, s));
                OPL_(ptta_launch_loss_finalize(ws, N, H, W, R, 1, w3, info, s));
            }
            if (pass == 0)
                OPL_(ptta_launch_loss_backward(a->depth, a->image, a->sparse, a->validity, maxd, nullptr, nullptr, R, D, N, H, W, ws, a->gdepth, nullptr, s,
                                               w3, nullptr, 1, 1));
        }
        // the cosine gradient kernel reading the coefficient and the row statistics from the workspace (its depth half goes to scratch)
        if (a->gref) OPL_(ptta_launch_loss_backward(a->depth, a->image, a->sparse, a->validity, maxd, a->emb, a->ref, R, D, N, H, W, ws, gscratch, a->gref, s));
    }
#undef OPL_
    if (rc > 0) rc = -5;
    auto d2d = [&](float* dst, const float* src, long n) { if (!rc && dst && n > 0 && hipMemcpyAsync(dst, src, (size_t)n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) rc = -5; };
    d2d(a->loss_info, info, 4);
    if (cos) d2d(a->rowstats, ws + ptta_loss_ws_rows_off(N), 3 * R);
    if (a->coef) { d2d(a->coef, ws + PTTA_LOSS_WS_SCAL, 3); d2d(a->coef + 3, ws + PTTA_LOSS_WS_SD, N); }
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    return rc;
}

// Stand-alone weight + bias gradient of a stride-1 3x3 convolution on dense fp32 NHWC maps (tests, tools/bench_gwgrad_wide.py): the
// engine's launcher (impl 0), the fp32-MFMA form (1) or the direct fp32 form of PTTA_CONV_IMPL=naive (2), then `reps` more launches of
// the same form timed with hipEvents on `s`.
int ptta_op_gwgrad(const float* x, const float* gy, float* gw, float* gb, int b, int h, int w, int ci, int co, int impl, int reps,
                   float* us_per_call_host, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!x || !gy || !gw || b < 1 || h < 1 || w < 1 || ci < 1 || co < 1 || ci > 256 || co > 256 || impl < 0 || impl > 2 || reps < 0 ||
        (reps > 0 && !us_per_call_host)) return -22;
    GView xv, gv;
    xv.p = (float*)x; xv.B = b; xv.H = h; xv.W = w; xv.C = ci; xv.ld = ci;
    gv.p = (float*)gy; gv.B = b; gv.H = h; gv.W = w; gv.C = co; gv.ld = co;
    const long P = (long)b * h * w;
    const size_t nm = (size_t)ptta_gwgrad_mfma_part_floats(P, ci, co), nn = (size_t)ptta_gwgrad_slabs(P) * (9 * ci * co + co);
    float* part = nullptr;
    if (hipMalloc((void**)&part, (impl == 2 ? nn : nm) * 4) != hipSuccess) return -12;
    auto run = [&]() {
        return impl == 0 ? ptta_launch_gwgrad_mfma(xv, gv, part, gw, gb, s)
                         : (impl == 1 ? ptta_launch_gwgrad_f32mfma(xv, gv, part, gw, gb, s) : ptta_launch_gwgrad(xv, gv, part, gw, gb, s));
    };
    int rc = run();
    if (!rc && reps > 0) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) rc = -5;
        if (!rc) {
            (void)hipEventRecord(e0, s);
            for (int r = 0; r < reps && !rc; ++r) rc = run();
            (void)hipEventRecord(e1, s);
            (void)hipEventSynchronize(e1);
            float ms = 0.f; (void)hipEventElapsedTime(&ms, e0, e1);
            *us_per_call_host = 1e3f * ms / (float)reps;
        }
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    (void)hipFree(part);
    return rc;
}

// Stand-alone convolution of the generic engine on fp32 NHWC device views (tests): the weight is packed by the engine's own code
// (gnet::pack_conv_weight / pack_vcol_weight) and launched ONCE the way GNet::run_conv_fwd / run_conv_bwd launch it -- the matrix-core
// form (impl 0) or the direct fp32 form (impl 1, one launch per source).  include/ptta.h states the arguments.
// affine: ptta_op_gconv_affine's epilogue (scale / shift / res / ld_res; the matrix-core forms only), refused before the first launch
static int op_gconv(const float* x0, int c0, int ld0, const float* x1, int c1, int ld1, const float* weight, const float* bias, float* y, int co,
                    int ldy, int b, int hin, int win, int hout, int wout, int k, int geom, int act, int accumulate, int impl, int flags,
                    int six_b, int x1_from_b, int stat_npass, double* stat_host, int* form_host, bool affine, const float* scale, const float* shift,
                    const float* res, int ld_res, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (affine) {
        const int cm = geom == PTTA_GCONV_S1 ? 7 : 15;          // channel counts the matrix-core forms take (ptta_launch_gconv_x3 / _strided)
        if (!scale || !shift || (((size_t)scale | (size_t)shift) & 15) || (res != nullptr) != (ld_res != 0) || (res && ld_res < co) ||
            impl != 0 || accumulate || stat_npass || six_b < 0 || six_b > b || (flags & PTTA_GCONV_DGRAD) ||
            (act != GACT_NONE && act != GACT_RELU && act != GACT_LRELU && act != GACT_ELU) ||
            c0 < 1 || c1 < 0 || (c0 & cm) || (c1 & cm)) return -22;
        // the residual forms, as ptta_gbn_switches_ok has them: act_first takes a residual and ReLU, the plain residual no activation
        const bool af = flags & PTTA_GCONV_AFF_ACT_FIRST, rp = flags & PTTA_GCONV_AFF_RES_PLAIN;
        if ((af && rp) || (af && (!res || act != GACT_RELU || (flags & PTTA_GCONV_VERT))) || (rp && (!res || act != GACT_NONE))) return -22;
        // the transposed geometry has the plain bf16x3 epilogue only (ptta_launch_gconv_x3_strided)
        if (geom == PTTA_GCONV_T2 && (af || six_b > 0)) return -22;
        // ELU: behind the stride-1 3-tap kernels only (square or PTTA_GCONV_VERT), never with a residual
        if (act == GACT_ELU && (geom != PTTA_GCONV_S1 || k != 3 || res || af || rp)) return -22;
    } else if (flags & (PTTA_GCONV_AFF_ACT_FIRST | PTTA_GCONV_AFF_RES_PLAIN)) return -22;
    const bool vert = flags & PTTA_GCONV_VERT, dgrad = flags & PTTA_GCONV_DGRAD;
    if (!x0 || !weight || !y || b < 1 || hin < 1 || win < 1 || hout < 1 || wout < 1 || c0 < 1 || c1 < 0 || co < 1 || ld0 < c0 || ldy < co ||
        (c1 > 0) != (x1 != nullptr) || (c1 > 0 && ld1 < c1) || (k != 1 && k != 3) || geom < PTTA_GCONV_S1 || geom > PTTA_GCONV_T2 ||
        act < GACT_NONE || act > (affine ? GACT_ELU : GACT_SIGMOID) || impl < 0 || impl > 1 || (flags & ~31) || six_b < 0 || six_b > b || x1_from_b < 0 ||
        stat_npass < 0 || stat_npass > 2 || (accumulate & ~1)) return -22;
    if (vert && (k != 3 || geom != PTTA_GCONV_S1)) return -22;
    if (dgrad && (c1 > 0 || six_b > 0)) return -22;
    if (stat_npass > 0 && (!stat_host || geom != PTTA_GCONV_S1 || impl != 0 || dgrad || (b % stat_npass))) return -22;
    // the geometry that runs: a data gradient is the other strided geometry with the same weight tensor (gconv.hip)
    const int run = !dgrad ? geom : (geom == PTTA_GCONV_S2 ? PTTA_GCONV_T2 : (geom == PTTA_GCONV_T2 ? PTTA_GCONV_S2 : PTTA_GCONV_S1));
    const bool size_ok = run == PTTA_GCONV_S1 ? (hout == hin && wout == win)
                       : run == PTTA_GCONV_S2 ? (hout == (hin + 1) / 2 && wout == (win + 1) / 2)
                       // (the gradient of a stride-2 convolution over an odd-sized map: 2 hin - 1)
                       : ((hout == 2 * hin || (dgrad && hout == 2 * hin - 1)) && (wout == 2 * win || (dgrad && wout == 2 * win - 1)));
    if (!size_ok) return -22;
    if (impl == 0 && ((((size_t)x0 | (size_t)x1) & 15) || (ld0 & 3) || (ld1 & 3))) return -22;   // the matrix-core kernels load 16 B
    if (form_host) *form_host = -1;

    gnet::GConvW cw;                                   // of the FORWARD convolution `weight` belongs to
    cw.k = k; cw.stride = geom == PTTA_GCONV_S1 ? 1 : 2; cw.transposed = geom == PTTA_GCONV_T2 ? 1 : 0; cw.vcol = vert ? 1 : 0;
    if (!dgrad) { cw.Ci = c0 + c1; cw.Co = co; cw.C0 = c0; cw.C1 = c1; }
    else { cw.Ci = co; cw.Co = c0; cw.C0 = co; cw.C1 = 0; }
    cw.mf = impl == 0 && !dgrad; cw.mb = impl == 0 && dgrad;
    const int KK = k * k;
    const size_t nw = (size_t)KK * cw.Ci * cw.Co;
    const size_t nfrag = cw.mf ? (size_t)ptta_gfrag_elems(KK, cw.C0, cw.C1, cw.Co) : (cw.mb ? (size_t)ptta_gfrag_elems(KK, cw.Co, 0, cw.Ci) : 0);
    const int tiles_pp = stat_npass ? ptta_gconv_x3_tiles(b / stat_npass, hout, wout) : 0;
    const size_t nstat = (size_t)stat_npass * tiles_pp * 2 * co;
    float* wbuf = nullptr; bf16_t* fbuf = nullptr; float* stat = nullptr;
    int rc = 0;
    if (hipMalloc((void**)&wbuf, 2 * nw * sizeof(float)) != hipSuccess || (nfrag && hipMalloc((void**)&fbuf, 3 * nfrag * sizeof(bf16_t)) != hipSuccess) ||
        (nstat && hipMalloc((void**)&stat, nstat * sizeof(float)) != hipSuccess)) rc = -12;
    if (!rc && (hipMemsetAsync(wbuf, 0, 2 * nw * sizeof(float), s) != hipSuccess || (nstat && hipMemsetAsync(stat, 0, nstat * sizeof(float), s) != hipSuccess))) rc = -5;
    if (!rc) {
        cw.wf = wbuf; cw.wb = wbuf + nw;
        if (cw.mf) { cw.ff_hi = fbuf; cw.ff_lo = fbuf + nfrag; if (six_b > 0) cw.ff_l2 = fbuf + 2 * nfrag; }
        if (cw.mb) { cw.fb_hi = fbuf; cw.fb_lo = fbuf + nfrag; }
        if (vert) gnet::pack_vcol_weight(cw, weight, s); else gnet::pack_conv_weight(cw, weight, s);
        GView xv[2], yv;
        xv[0].p = (float*)x0; xv[0].C = c0; xv[0].ld = ld0; xv[1].p = (float*)x1; xv[1].C = c1; xv[1].ld = ld1;
        for (GView& v : xv) { v.B = b; v.H = hin; v.W = win; }
        yv.p = y; yv.B = b; yv.H = hout; yv.W = wout; yv.C = co; yv.ld = ldy;
        if (impl == 0) {
            GX3Args a;
            a.x0 = x0; a.C0 = c0; a.ld0 = ld0;
            if (c1 > 0) { a.x1 = x1; a.C1 = c1; a.ld1 = ld1; }
            a.B = b; a.H = hout; a.W = wout;
            a.whi = (const uint4*)(dgrad ? cw.fb_hi : cw.ff_hi); a.wlo = (const uint4*)(dgrad ? cw.fb_lo : cw.ff_lo);
            a.nchunks = (a.C0 + 31) / 32 + (a.C1 + 31) / 32; a.nf0 = 0; a.nnf = (co + 31) / 32;
            a.y = y; a.ldy = ldy; a.Cy = co; a.bias = bias; a.act = act; a.accumulate = accumulate; a.vert = vert ? 1 : 0;
            if (six_b > 0) { a.wl2 = (const uint4*)cw.ff_l2; a.six_B = six_b; }
            a.x1_from_B = x1_from_b; a.x1_w2 = (flags & PTTA_GCONV_X1_W2) ? 1 : 0;
            if (stat) { a.stat_part = stat; a.stat_C = co; a.stat_npass = stat_npass; }
            if (affine) {
                a.scale = scale; a.shift = shift; a.res = res; a.ld_res = ld_res;
                a.aff_act_first = (flags & PTTA_GCONV_AFF_ACT_FIRST) ? 1 : 0; a.aff_res_plain = (flags & PTTA_GCONV_AFF_RES_PLAIN) ? 1 : 0;
            }
            if (run == PTTA_GCONV_S1) rc = ptta_launch_gconv_x3(a, k, s);
            else {
                const int mode = run == PTTA_GCONV_T2 ? 2 : 1;
                if (form_host) *form_host = ptta_gconv_x3_strided_form(a, k, mode, win);
                rc = ptta_launch_gconv_x3_strided(a, k, mode, hin, win, s);
            }
        } else {
            for (int sidx = 0; sidx < (c1 > 0 ? 2 : 1) && !rc; ++sidx) {
                GConvArgs a;
                a.x = xv[sidx]; a.y = yv; a.k = k;
                if (!dgrad) {                          // GNet::run_conv_fwd: bias with the first source, the activation after the last
                    a.w = cw.wf + (size_t)(sidx ? c0 : 0) * cw.Co; a.wld = cw.Co; a.wts = (long)cw.Ci * cw.Co;
                    a.bias = sidx == 0 ? bias : nullptr;
                    a.stride = cw.stride; a.transposed = cw.transposed;
                    a.accumulate = (sidx > 0 || accumulate) ? 1 : 0; a.act = sidx == (c1 > 0 ? 1 : 0) ? act : GACT_NONE;
                } else {                               // GNet::run_conv_bwd
                    a.w = cw.wb; a.wld = cw.Ci; a.wts = (long)cw.Co * cw.Ci;
                    a.bias = bias; a.act = act; a.accumulate = accumulate;
                    a.stride = run == PTTA_GCONV_S1 ? 1 : 2; a.transposed = run == PTTA_GCONV_T2 ? 1 : 0;
                }
                rc = ptta_launch_gconv_direct(a, s);
            }
        }
    }
    std::vector<float> hstat;
    if (!rc && nstat) {
        hstat.resize(nstat);
        if (hipMemcpyAsync(hstat.data(), stat, nstat * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess) rc = -5;
    }
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    if (!rc && nstat) {                                // [pass][tile][2][co] -> [pass][2][co], tiles summed in fp64
        for (int pass = 0; pass < stat_npass; ++pass)
            for (int j = 0; j < 2 * co; ++j) {
                double v = 0.0;
                for (int t = 0; t < tiles_pp; ++t) v += (double)hstat[((size_t)pass * tiles_pp + t) * 2 * co + j];
                stat_host[(size_t)pass * 2 * co + j] = v;
            }
    }
    (void)hipFree(wbuf); (void)hipFree(fbuf); (void)hipFree(stat);
    return rc;
}
int ptta_op_gconv(const float* x0, int c0, int ld0, const float* x1, int c1, int ld1, const float* weight, const float* bias, float* y, int co,
                  int ldy, int b, int hin, int win, int hout, int wout, int k, int geom, int act, int accumulate, int impl, int flags,
                  int six_b, int x1_from_b, int stat_npass, double* stat_host, int* form_host, ptta_stream s_) {
    return op_gconv(x0, c0, ld0, x1, c1, ld1, weight, bias, y, co, ldy, b, hin, win, hout, wout, k, geom, act, accumulate, impl, flags, six_b, x1_from_b,
                    stat_npass, stat_host, form_host, false, nullptr, nullptr, nullptr, 0, s_);
}
// the same convolution with the eval-BatchNorm epilogue (the meta-only eval forward, the stage-2 head trainer): y = act(fmaf(conv + bias, scale[c], shift[c]) [+ res])
// and, by flag, relu(relu(fmaf(..)) + res) or fmaf(..) + res
int ptta_op_gconv_affine(const float* x0, int c0, int ld0, const float* x1, int c1, int ld1, const float* weight, const float* bias, float* y, int co,
                         int ldy, int b, int hin, int win, int hout, int wout, int k, int geom, int act, int accumulate, int impl, int flags,
                         int six_b, int x1_from_b, int stat_npass, double* stat_host, int* form_host, const float* scale, const float* shift,
                         const float* res, int ld_res, ptta_stream s_) {
    return op_gconv(x0, c0, ld0, x1, c1, ld1, weight, bias, y, co, ldy, b, hin, win, hout, wout, k, geom, act, accumulate, impl, flags, six_b, x1_from_b,
                    stat_npass, stat_host, form_host, true, scale, shift, res, ld_res, s_);
}

// Stand-alone BatchNorm of the generic engine on fp32 NHWC device views (tests): the launchers of gbn.hip called as GNet::run_bn_fwd /
// run_bn_bwd call them, with the engine's scratch sizes.  include/ptta.h states the arguments.
int ptta_op_gbn(const ptta_gbn_args* a, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!a || a->mode < PTTA_GBN_TRAIN || a->mode > PTTA_GBN_BACKWARD) return -22;
    const bool train = a->mode == PTTA_GBN_TRAIN, eval = a->mode == PTTA_GBN_EVAL, bwd = a->mode == PTTA_GBN_BACKWARD;
    const int C = a->x.c;
    auto view_ok = [&](const ptta_gbn_view& v) { return v.p && v.c == C && v.ld >= C && !(v.ld & 3) && !((size_t)v.p & 15); };
    auto table_ok = [](const void* p) { return p && !((size_t)p & 15); };
    if (a->b < 1 || a->h < 1 || a->w < 1 || C < 4 || (C & 3) || (a->npass != 1 && a->npass != 2) || (a->b % a->npass) || a->world < 1 ||
        (a->act != GACT_NONE && a->act != GACT_RELU && a->act != GACT_LRELU && a->act != GACT_ELU) || ((a->act_first | a->res_relu | a->acc_gx | a->acc_gres) & ~1) ||
        !(a->eps > 0.f)) return -22;
    if (!view_ok(a->x) || !view_ok(a->y) || !table_ok(a->gamma) || !table_ok(a->st)) return -22;
    if (eval && a->npass != 1) return -22;
    if (!bwd) {
        if ((a->res.p && !view_ok(a->res)) || !table_ok(a->beta)) return -22;
        // the switch combinations are the launchers' to refuse (before their first launch); the eval affine is launched ahead of the apply
        // launcher, so that mode asks their predicate here
        if (eval && !ptta_gbn_switches_ok(a->res.p != nullptr, a->act, a->res_relu, a->act_first)) return -22;
        if ((a->rm != nullptr) != (a->rv != nullptr) || (eval && !a->rm)) return -22;
        if (a->rm && (!table_ok(a->rm) || !table_ok(a->rv) || a->repeats < 1 || (a->st_eval && !table_ok(a->st_eval)))) return -22;
        if (train && a->part_in && a->nblocks_in < 1) return -22;
    } else {
        if (!view_ok(a->g) || !view_ok(a->gx) || (a->gres.p && !view_ok(a->gres))) return -22;
    }
    auto gv = [&](const ptta_gbn_view& v, int B) { GView o; o.p = v.p; o.B = B; o.H = a->h; o.W = a->w; o.C = v.c; o.ld = v.ld; return o; };
    const int nb_in = (train && a->part_in) ? a->nblocks_in : 0;
    size_t npart = (size_t)ptta_gbn_part_floats(C, a->npass);
    if ((size_t)a->npass * nb_in * 2 * C > npart) npart = (size_t)a->npass * nb_in * 2 * C;       // (a fused BatchNorm owns its partials: GNet Op::part)
    float *part = nullptr, *bw = nullptr; double* xbuf = nullptr;
    const long long xcap = (long long)a->npass * 2 * C;
    int world = a->world, rc = 0;
    if (!eval && hipMalloc((void**)&part, npart * sizeof(float)) != hipSuccess) rc = -12;
    if (!rc && bwd && hipMalloc((void**)&bw, (size_t)3 * C * sizeof(float)) != hipSuccess) rc = -12;
    if (!rc && world > 1 && hipMalloc((void**)&xbuf, (size_t)xcap * sizeof(double)) != hipSuccess) rc = -12;
    PttaStatSync sy;
    if (world > 1) { sy.fn = op_gbn_exchange; sy.user = &world; sy.buf = xbuf; sy.cap = (long)xcap; sy.world = world; }
    if (!rc && nb_in &&
        hipMemcpyAsync(part, a->part_in, (size_t)a->npass * nb_in * 2 * C * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) rc = -5;
    if (!rc) {
        const GView x = gv(a->x, a->b), y = gv(a->y, a->b);
        GView res; if (!bwd && a->res.p) res = gv(a->res, a->b);
        if (train)
            rc = ptta_launch_gbn_forward(x, res, y, a->npass, a->act, a->eps, a->gamma, a->beta, part, a->st, s, nb_in, a->act_first, &sy, a->rm, a->rv,
                                         a->rm ? a->nbt : nullptr, a->momentum, a->repeats, a->rm ? a->st_eval : nullptr, a->res_relu);
        else if (eval) {
            rc = ptta_launch_gbn_eval_affine(a->gamma, a->beta, a->rm, a->rv, a->eps, C, a->st, s);
            if (!rc) rc = ptta_launch_gbn_apply(x, res, y, 1, a->act, a->st, a->res_relu, s, a->act_first);
        } else {
            const int per = a->b / a->npass;
            GView gres; if (a->gres.p) gres = gv(a->gres, per);
            rc = ptta_launch_gbn_backward(x, gv(a->g, per), y, gv(a->gx, per), gres, a->npass, a->act, (a->gres.p && a->res_relu) ? 1 : 0, a->acc_gx,
                                          a->acc_gres, a->gamma, a->st, part, bw, a->dgamma, a->dbeta, s, a->act_first, &sy);
        }
    }
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    (void)hipFree(part); (void)hipFree(bw); (void)hipFree(xbuf);
    return rc;
}

// ---- CostDCNet's own kernels (costdc_kernels.hip) on caller-supplied device buffers (tests): every hook calls the launchers of costdc.h
// as costdc_api.hip calls them.  include/ptta.h states the arguments.
struct ptta_cd_sparse {
    CdSparse q;
    long cap = 0;
    ~ptta_cd_sparse() {
        for (int l = 0; l < 3; ++l) { (void)hipFree(q.vol[l]); (void)hipFree(q.coords[l]); }
        (void)hipFree(q.cnt); (void)hipFree(q.rowcnt); (void)hipFree(q.rowoff); (void)hipFree(q.feat_in); (void)hipFree(q.bn_part); (void)hipFree(q.bn_st);
    }
};
// sized as costdc_engine::build_sparse() sizes it
int ptta_cd_sparse_create(ptta_cd_sparse** out, int n, int h, int w) {
    if (!out) return -22;
    *out = nullptr;
    if (n < 1 || h < 4 || w < 4 || (h & 3) || (w & 3) || (long)n * 16 * h * w > 0x7fffffffL) return -22;   // level 2 halves twice; the row kernels index with int
    ptta_cd_sparse* p = new ptta_cd_sparse();
    CdSparse& q = p->q;
    q.N = n; q.H = h; q.W = w; p->cap = (long)n * h * w;
    bool ok = true;
    for (int l = 0; l < 3 && ok; ++l)
        ok = hipMalloc((void**)&q.vol[l], (size_t)n * 16 * (h >> l) * (w >> l) * sizeof(int)) == hipSuccess &&
             hipMalloc((void**)&q.coords[l], (size_t)p->cap * sizeof(int4)) == hipSuccess;
    ok = ok && hipMalloc((void**)&q.cnt, 4 * sizeof(int)) == hipSuccess && hipMemset(q.cnt, 0, 4 * sizeof(int)) == hipSuccess &&
         hipMalloc((void**)&q.rowcnt, (size_t)n * 16 * h * sizeof(int)) == hipSuccess && hipMalloc((void**)&q.rowoff, (size_t)n * 16 * h * sizeof(int)) == hipSuccess &&
         hipMalloc((void**)&q.feat_in, (size_t)p->cap * sizeof(float)) == hipSuccess && hipMalloc((void**)&q.bn_part, (size_t)256 * 2 * 64 * sizeof(float)) == hipSuccess &&
         hipMalloc((void**)&q.bn_st, 4 * 64 * sizeof(float)) == hipSuccess;
    if (!ok) { delete p; return -12; }
    *out = p;
    return 0;
}
void ptta_cd_sparse_destroy(ptta_cd_sparse* p) { delete p; }
int ptta_cd_sparse_build(ptta_cd_sparse* p, const float* sparse, float z_step, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!p || !sparse || !(z_step > 0.f)) return -22;
    int rc = cd_sparse_levels_build(p->q, sparse, z_step, s);
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    return rc;
}
int ptta_cd_sparse_read(ptta_cd_sparse* p, int level, int* cnt_host, int* coords_host, long long coords_cap, int* vol_host, float* feat_in_host, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!p || level < 0 || level > 2 || coords_cap < 0 || (feat_in_host && level != 0) || ((coords_host || feat_in_host) && coords_cap < 1)) return -22;
    const CdSparse& q = p->q;
    int cnt[3];
    if (hipMemcpyAsync(cnt, q.cnt, 3 * sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return -5;
    if (cnt_host) for (int l = 0; l < 3; ++l) cnt_host[l] = cnt[l];
    long long rows = cnt[level] < 0 ? 0 : cnt[level];
    if (rows > coords_cap) rows = coords_cap;
    if (rows > p->cap) rows = p->cap;
    int rc = 0;
    if (coords_host && rows && hipMemcpyAsync(coords_host, q.coords[level], (size_t)rows * sizeof(int4), hipMemcpyDeviceToHost, s) != hipSuccess) rc = -5;
    if (!rc && feat_in_host && rows && hipMemcpyAsync(feat_in_host, q.feat_in, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess) rc = -5;
    if (!rc && vol_host &&
        hipMemcpyAsync(vol_host, q.vol[level], (size_t)q.N * 16 * (q.H >> level) * (q.W >> level) * sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess) rc = -5;
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    return rc;
}
int ptta_op_cd_sparse_conv(ptta_cd_sparse* p, const float* x, const float* wk, float* y, int lin, int lout, int ksize, int ci, int co, int backward, int acc,
                           ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!p || !x || !wk || !y || lin < 0 || lout < lin || lout > 2 || lout - lin > 1 || (ksize != 1 && ksize != 3) || ci < 1 || co < 1 || (backward & ~1) || (acc & ~1) ||
        (!backward && acc) || (backward ? ci : co) > 64) return -22;
    int rc = backward ? cd_launch_sparse_conv_bwd(p->q, x, lin, lout, wk, ksize, ci, co, y, acc, s) : cd_launch_sparse_conv(p->q, x, lin, lout, wk, ksize, ci, co, y, s);
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    return rc;
}
int ptta_op_cd_sbn(ptta_cd_sparse* p, const ptta_cd_sbn_args* a, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!p || !a || a->mode < PTTA_GBN_TRAIN || a->mode > PTTA_GBN_BACKWARD || a->level < 0 || a->level > 2 || a->c < 1 || a->c > 64 || (a->relu & ~1) ||
        (a->acc_res & ~1) || a->world < 1 || !a->f || !a->gamma || !a->st) return -22;
    const bool bwd = a->mode == PTTA_GBN_BACKWARD, train = a->mode == PTTA_GBN_TRAIN;
    if (!bwd && (!a->beta || !a->out || (a->rm != nullptr) != (a->rv != nullptr) || (!train && !a->rm) || (train && a->rm && a->repeats < 1) || (!train && a->world > 1)))
        return -22;
    if (bwd && (!a->y || !a->g || !a->gx || !a->dgamma || !a->dbeta)) return -22;
    const int C = a->c;
    int world = a->world, rc = 0;
    double* xbuf = nullptr; float* bw = nullptr;
    if (world > 1 && hipMalloc((void**)&xbuf, (size_t)(2 * C + 1) * sizeof(double)) != hipSuccess) rc = -12;
    if (!rc && bwd && hipMalloc((void**)&bw, (size_t)3 * 64 * sizeof(float)) != hipSuccess) rc = -12;
    PttaStatSync sy;
    if (world > 1) { sy.fn = op_gbn_exchange; sy.user = &world; sy.buf = xbuf; sy.cap = 2 * C + 1; sy.world = world; }
    if (!rc) {
        if (!bwd)
            rc = cd_launch_sparse_bn(p->q, a->f, a->res, a->level, C, a->gamma, a->beta, a->rm, a->rv, a->rm ? a->nbt : nullptr, train ? 1 : 0, a->repeats, a->relu, a->out,
                                     s, &sy, a->st);
        else
            rc = cd_launch_sparse_bn_bwd(p->q, a->f, a->y, a->g, a->level, C, a->gamma, a->st, a->relu, a->dgamma, a->dbeta, a->gx, a->gres, a->acc_res, bw, s, &sy);
    }
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    (void)hipFree(xbuf); (void)hipFree(bw);
    return rc;
}
int ptta_op_cd_densify(ptta_cd_sparse* p, const float* in, float* out, int c, int backward, int ldv, int c0, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!p || !in || !out || c < 1 || (backward & ~1) || (backward && (c0 < 0 || ldv < c0 + c))) return -22;
    int rc = backward ? cd_launch_densify_bwd(p->q, in, ldv, c0, c, out, s) : cd_launch_densify(p->q, in, c, out, s);
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    return rc;
}
int ptta_op_cd_dense(int op, const float* a, const float* b, float* out, float* out2, const int* d, const float* f, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!a || !out || !d || op < PTTA_CD_PAD_DUAL || op > PTTA_CD_ROWS_BWD) return -22;
    auto pos = [&](int k0, int k1) { for (int k = k0; k < k1; ++k) if (d[k] < 1) return false; return true; };
    auto al16 = [](const void* q) { return !((size_t)q & 15); };
    int rc = -22;
    switch (op) {
    case PTTA_CD_PAD_DUAL: {             // d = {N, C, H, W, Hp, Wp, pt, pr, norm}; f = {div, mean[3], std[3]}
        if (!pos(0, 6) || d[6] < 0 || d[7] < 0 || (d[8] & ~1) || (d[8] && (d[1] != 3 || !f))) break;
        rc = cd_launch_pad_dual(a, out, d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], s, d[8], d[8] ? f[0] : 1.f, d[8] ? f + 1 : nullptr, d[8] ? f + 4 : nullptr);
        break; }
    case PTTA_CD_CROP_AVG:               // d = {N, H, W, Hp, Wp, pt, pr}: reads rows y + pt and columns x + pr of the padded frame
        if (!pos(0, 5) || d[5] < 0 || d[6] < 0 || d[1] + d[5] > d[3] || d[2] + d[6] > d[4]) break;
        rc = cd_launch_crop_avg(a, out, d[0], d[1], d[2], d[3], d[4], d[5], d[6], s);
        break;
    case PTTA_CD_SCATTER_DUAL_GRAD:      // d = {N, H, W, Hp, Wp, pt, pr}
        if (!pos(0, 5) || d[5] < 0 || d[6] < 0) break;
        rc = cd_launch_scatter_dual_grad(a, out, d[0], d[1], d[2], d[3], d[4], d[5], d[6], s);
        break;
    case PTTA_CD_STAGE:                  // d = {N, passes, H, W, C, norm}; f = {div, mean[3], std[3]} (read even when norm = 0)
        if (!b || !f || !pos(0, 4) || d[1] > 2 || (d[4] != 4 && d[4] != 16) || (d[5] & ~1) || !al16(out)) break;
        rc = cd_launch_stage(a, b, out, d[0], d[1], d[2], d[3], d[4], d[5], f[0], f + 1, f + 4, s);
        break;
    case PTTA_CD_CLAMP:                  // d = {n}; f = {max depth (< 0: copy)}
        if (!f || d[0] < 1) break;
        rc = cd_launch_clamp(a, out, (long)d[0], f[0], s);
        break;
    case PTTA_CD_FUSION_FWD:             // d = {N, passes, h, w}
        if (!b || !out2 || !pos(0, 4) || d[1] > 2 || !al16(a) || !al16(b) || !al16(out)) break;
        rc = cd_launch_fusion_fwd(a, b, out, out2, d[0], d[1], d[2], d[3], s);
        break;
    case PTTA_CD_FUSION_BWD:             // d = {N, h, w}
        if (!b || !pos(0, 3)) break;
        rc = cd_launch_fusion_bwd(a, b, out, d[0], d[1], d[2], s);
        break;
    case PTTA_CD_POOL_FWD:               // d = {items_out, H, W, C}: reads 2 items_out planes
        if (!pos(0, 4) || (d[3] & 3) || !al16(a) || !al16(out)) break;
        rc = cd_launch_pool_fwd(a, out, (long)d[0], d[1], d[2], d[3], s);
        break;
    case PTTA_CD_POOL_BWD:               // d = {items_in, H, W, C, acc}: plane pairs, so items_in is even
        if (!b || !pos(0, 4) || (d[0] & 1) || (d[4] & ~1)) break;
        rc = cd_launch_pool_bwd(a, b, out, (long)d[0], d[1], d[2], d[3], d[4], s);
        break;
    case PTTA_CD_UP_FWD:                 // d = {frames, Di, Hi, Wi, Do, Ho, Wo, C}
        if (!pos(0, 8) || (d[7] & 3) || !al16(a) || !al16(out)) break;
        rc = cd_launch_up_fwd(a, out, (long)d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], s);
        break;
    case PTTA_CD_UP_BWD:                 // d = {frames, Di, Hi, Wi, Do, Ho, Wo, C, acc}
        if (!pos(0, 8) || (d[8] & ~1)) break;
        rc = cd_launch_up_bwd(a, out, (long)d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], s);
        break;
    case PTTA_CD_REGRESS_FWD:            // d = {N, h, w}; f = {z_step}
        if (!f || !pos(0, 3)) break;
        rc = cd_launch_regress_fwd(a, out, d[0], d[1], d[2], f[0], s);
        break;
    case PTTA_CD_REGRESS_BWD:
        if (!b || !f || !pos(0, 3)) break;
        rc = cd_launch_regress_bwd(a, b, out, d[0], d[1], d[2], f[0], s);
        break;
    case PTTA_CD_ROWS_FWD:               // d = {N, D, h, w, C}
        if (!pos(0, 5)) break;
        rc = cd_launch_rows_fwd(a, out, d[0], d[1], d[2], d[3], d[4], s);
        break;
    case PTTA_CD_ROWS_BWD:               // d = {N, D, h, w, C, acc}
        if (!pos(0, 5) || (d[5] & ~1)) break;
        rc = cd_launch_rows_bwd(a, out, d[0], d[1], d[2], d[3], d[4], d[5], s);
        break;
    }
    if (rc == -22) return rc;
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    return rc;
}

// Diagnostic: `reps` DEPENDENT launches of one 32 -> 32 stride-1 convolution (ping-pong between two buffers, optional ReLU mask / skip
// addition epilogue reading a third) captured into ONE hipGraph and replayed: microseconds per launch as it costs INSIDE a replayed graph
// (rocprofv3 adds ~3-5 us to every kernel and a host-timed single launch measures the launch path).  tools/bench_chain.py.
int ptta_op_conv32_chain(const float* in, const float* weight, const float* bias, float* buf_a, float* buf_b, const float* aux, int b, int h, int w,
                         int relu_in, int epi_flags, int reps, int replays, float* us_per_launch_host, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!in || !weight || !buf_a || !buf_b || reps < 1 || replays < 1 || !us_per_launch_host) return -22;
    ScratchConvW sw; ConvW& wv = sw.w;
    if (!sw.ok) return -12;
    ptta_pack_conv32(weight, wv, 0, 0, s);
    (void)hipStreamSynchronize(s);
    auto chain_step = [&](int r, hipStream_t st) {       // launch r of the chain: ping-pong between the two buffers
        Conv32Args a; a.w = &wv; a.bias = bias; a.B = b; a.Hin = h; a.Win = w; a.mode = CONV_S1; a.relu_in = relu_in; a.x3 = 1;
        a.in = r == 0 ? in : ((r & 1) ? buf_a : buf_b); a.in_nb = b; a.out_raw = (r & 1) ? buf_b : buf_a;
        if ((epi_flags & 2) && aux) { a.mask = aux; a.mask_nb = b; }
        if ((epi_flags & 4) && aux) { a.add1 = aux; a.add1_nb = b; }
        return ptta_launch_conv32(a, st);
    };
    if (epi_flags & 16) {                  // the layer loop: `reps` dependent layers per LAUNCH, a device-wide barrier between layers (conv32_loop.hip)
        hipEvent_t d0 = nullptr, d1 = nullptr;
        unsigned* ctr = nullptr; int* err = nullptr;
        int rcd = (hipEventCreate(&d0) != hipSuccess || hipEventCreate(&d1) != hipSuccess) ? -5 : (hipMalloc((void**)&ctr, 256) != hipSuccess ? -12 : 0);
        if (!rcd) {
            err = (int*)(ctr + 32);
            (void)hipMemsetAsync(ctr, 0, 256, s);
            unsigned base = 0;
            for (int k = 0; k < replays + 2 && !rcd; ++k) {
                if (k == 2) (void)hipEventRecord(d0, s);
                Conv32Args a; a.w = &wv; a.bias = bias; a.B = b; a.Hin = h; a.Win = w; a.mode = CONV_S1; a.relu_in = relu_in; a.x3 = 1;
                a.in = in; a.in_nb = b;
                rcd = ptta_launch_conv32_loop(a, buf_a, buf_b, reps, ctr, &base, err, (epi_flags & 64) ? 2 : ((epi_flags & 32) ? 1 : 0), s);
            }
            (void)hipEventRecord(d1, s); (void)hipStreamSynchronize(s);
            float ms = 0.f; (void)hipEventElapsedTime(&ms, d0, d1);
            *us_per_launch_host = 1e3f * ms / ((float)replays * (float)reps);
            int herr = 0; (void)hipMemcpy(&herr, err, sizeof(int), hipMemcpyDeviceToHost);
            if (!rcd && herr) rcd = -62;       // a bounded spin ran out (ETIME): the values are not a chain's
        }
        if (d0) (void)hipEventDestroy(d0);
        if (d1) (void)hipEventDestroy(d1);
        (void)hipFree(ctr);
        return rcd;
    }
    if (epi_flags & 8) {                   // the same chain launched directly (no graph): what a dependent launch costs in the default form
        hipEvent_t d0 = nullptr, d1 = nullptr;
        int rcd = (hipEventCreate(&d0) != hipSuccess || hipEventCreate(&d1) != hipSuccess) ? -5 : 0;
        if (!rcd) {
            for (int k = 0; k < replays + 2 && !rcd; ++k) {
                if (k == 2) (void)hipEventRecord(d0, s);
                for (int r = 0; r < reps && !rcd; ++r) rcd = chain_step(r, s);
            }
            (void)hipEventRecord(d1, s); (void)hipStreamSynchronize(s);
            float ms = 0.f; (void)hipEventElapsedTime(&ms, d0, d1);
            *us_per_launch_host = 1e3f * ms / ((float)replays * (float)reps);
        }
        if (d0) (void)hipEventDestroy(d0);
        if (d1) (void)hipEventDestroy(d1);
        return rcd;
    }
    hipStream_t cs = nullptr; hipGraph_t g = nullptr; hipGraphExec_t ge = nullptr; hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = 0;
    if (hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess) rc = -5;
    if (!rc && hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) != hipSuccess) rc = -5;
    if (!rc) {
        for (int r = 0; r < reps && !rc; ++r) rc = chain_step(r, cs);
        if (hipStreamEndCapture(cs, &g) != hipSuccess || !g) rc = rc ? rc : -5;
    }
    if (!rc && hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) != hipSuccess) rc = -5;
    if (!rc && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) rc = -5;
    if (!rc) {
        (void)hipGraphLaunch(ge, s); (void)hipGraphLaunch(ge, s);           // warm
        (void)hipEventRecord(e0, s);
        for (int k = 0; k < replays; ++k) (void)hipGraphLaunch(ge, s);
        (void)hipEventRecord(e1, s);
        (void)hipStreamSynchronize(s);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        *us_per_launch_host = 1e3f * ms / ((float)replays * (float)reps);
    }
    if (ge) (void)hipGraphExecDestroy(ge);
    if (g) (void)hipGraphDestroy(g);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (cs) (void)hipStreamDestroy(cs);
    return rc;
}

// ---- NLSPN's propagation gradients, stand-alone (tests/test_gpu_nlspn_det_elementwise.py, tools/bench_nlspn_deterministic.py) ----------------
// form 0: the float-atomic kernels of the default step; form 1: the fixed-point forms of option "deterministic", launched as the engine's
// backward launches them.  scratch: ptta_nl_det_scratch_bytes(b, h, w) bytes, 8-byte aligned (form 1 only).
int64_t ptta_nl_det_scratch_bytes(int b, int h, int w) { return (b < 1 || h < 1 || w < 1) ? -22 : (int64_t)ptta_nl_det_ws_bytes(b, h, w); }

static bool op_nl_ok(int b, int h, int w, int form, const void* scratch) {
    return b >= 1 && h >= 1 && w >= 1 && (double)b * h * w < 2.0e9 && form >= 0 && form <= 1 && (form == 0 || (scratch && op_al(scratch, 8)));
}
int ptta_op_nl_prop_bwd(const float* pinned, const float* fix, const float* off9, const float* aff9, const float* gout, float* gfeat,
                        float* goff9, float* gaff9, int b, int h, int w, int form, void* scratch, int reps, float* us_per_call_host,
                        ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!pinned || !fix || !off9 || !aff9 || !gout || !gfeat || !goff9 || !gaff9 || !op_nl_ok(b, h, w, form, scratch) || reps < 0 ||
        (reps > 0 && !us_per_call_host)) return -22;
    const long n = (long)b * h * w;
    unsigned* mx = (unsigned*)scratch;
    unsigned long long* acc = (unsigned long long*)((char*)scratch + PTTA_NL_DET_SLOTS * sizeof(unsigned));
    int rc = 0;
    if (form == 1) {            // the maxima the engine keeps per backward: of sum|aff9| and of this sweep's gout
        if (hipMemsetAsync(scratch, 0, ptta_nl_det_ws_bytes(b, h, w), s) != hipSuccess) rc = -5;
        if (!rc) rc = ptta_launch_nl_affsum_max(aff9, b, h, w, mx, s);
        if (!rc) rc = ptta_launch_nl_absmax(gout, n, mx + 1, s);
    }
    auto run = [&]() {
        if (form == 1) return ptta_launch_nl_prop_bwd_det(pinned, fix, off9, aff9, gout, gfeat, goff9, gaff9, b, h, w, acc, mx, mx + 1, mx + 2, s);
        if (hipMemsetAsync(gfeat, 0, (size_t)n * sizeof(float), s) != hipSuccess) return -5;
        return ptta_launch_nl_prop_bwd(pinned, fix, off9, aff9, gout, gfeat, goff9, gaff9, b, h, w, s);
    };
    if (!rc) rc = run();
    if (!rc && reps > 0) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) rc = -5;
        if (!rc) {
            (void)hipEventRecord(e0, s);
            for (int r = 0; r < reps && !rc; ++r) rc = run();
            (void)hipEventRecord(e1, s);
            (void)hipEventSynchronize(e1);
            float ms = 0.f; (void)hipEventElapsedTime(&ms, e0, e1);
            *us_per_call_host = 1e3f * ms / (float)reps;
        }
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    if (rc > 0) rc = -5;
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    return rc;
}

int ptta_op_nl_affinity_bwd(const float* oa_nhwc, const float* conf, const float* aff_scale, int legacy, const float* goff9, const float* gaff9,
                            float* goa_nhwc, float* gconf, int b, int h, int w, int form, void* scratch, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!oa_nhwc || !conf || !aff_scale || !goff9 || !gaff9 || !goa_nhwc || !gconf || !op_nl_ok(b, h, w, form, scratch)) return -22;
    GView oa, goa;
    oa.p = (float*)oa_nhwc; oa.B = b; oa.H = h; oa.W = w; oa.C = 24; oa.ld = 24;
    goa = oa; goa.p = goa_nhwc;
    int rc = 0;
    if (form == 1) {
        if (hipMemsetAsync(scratch, 0, ptta_nl_det_ws_bytes(b, h, w), s) != hipSuccess) rc = -5;
        if (!rc) rc = ptta_launch_nl_affinity_bwd_det(oa, conf, aff_scale, legacy ? 1 : 0, goff9, gaff9, goa, gconf,
                                                      (unsigned long long*)((char*)scratch + PTTA_NL_DET_SLOTS * sizeof(unsigned)), (unsigned*)scratch, s);
    } else {
        if (hipMemsetAsync(gconf, 0, (size_t)b * h * w * sizeof(float), s) != hipSuccess) rc = -5;
        if (!rc) rc = ptta_launch_nl_affinity_bwd(oa, conf, aff_scale, legacy ? 1 : 0, goff9, gaff9, goa, gconf, s);
    }
    if (rc > 0) rc = -5;
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    return rc;
}

// ---- the narrow heads of the mixed mode and head_bwd_finish, stand-alone (tests/test_gpu_heads_n_elementwise.py) --------------------------
// Thin: convert the fp32 weights the way msgchn_build.hip does, launch, synchronise, return the launcher's code.  include/ptta.h states the
// arguments and layouts.
long long ptta_op_hn_tiled_elems(long long r) { return r < 1 ? -22 : (long long)ptta_hn_tiled_elems((long)r); }

// the hi plane of ptta_split_weight for an fp32 [n] weight (NULL stays NULL); `lo` is the split's other output, shared scratch of n elements
static const bf16_t* op_hn_hi(OpBufs& m, const float* w, long n, bf16_t* lo, hipStream_t s) {
    if (!w) return nullptr;
    bf16_t* hi = (bf16_t*)m.get((size_t)n * 2);
    if (hi && lo) ptta_split_weight(w, hi, lo, nullptr, n, 512, s);
    return hi;
}

int ptta_op_hn_gemm(const ptta_hn_gemm_args* a, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!a) return -22;
    OpBufs m;
    HnGemmArgs g;
    g.pro = a->pro; g.epi = a->epi; g.x_bf16 = a->x_bf16; g.cpart_n = a->cpart_n; g.R = (long)a->r;
    g.A = (const bf16_t*)a->A; g.Af = a->Af; g.Bref = (const bf16_t*)a->Bref; g.rowstats = a->rowstats; g.coef = a->coef; g.X = a->X;
    g.b0 = a->b0; g.pscale = a->pscale; g.pshift = a->pshift; g.bias = a->bias;
    g.C = (bf16_t*)a->C; g.part = a->part; g.E = (const bf16_t*)a->E; g.rs = a->rs; g.rowstats_out = a->rowstats_out; g.cpart = a->cpart;
    g.escale = a->escale; g.eshift = a->eshift; g.emean = a->emean; g.einv = a->einv; g.P = a->P;
    bf16_t* lo = (bf16_t*)m.get((size_t)512 * 512 * 2);
    const bf16_t* whi = op_hn_hi(m, a->W, 512L * 512, lo, s);
    g.W0 = op_hn_hi(m, a->W0, 512L * 32, lo, s);
    g.W0t = op_hn_hi(m, a->W0t, 32L * 512, lo, s);
    bf16_t* wsl = a->W ? (bf16_t*)m.get((size_t)512 * 512 * 2) : nullptr;
    if (!m.ok) return -12;
    if (wsl) ptta_hn_pack_w(whi, wsl, 512, s);
    g.W = wsl;
    int rc = ptta_launch_hn_gemm(g, s);
    if (rc > 0) rc = -5;
    if (!rc && a->w_image && hipMemcpyAsync(a->w_image, wsl, (size_t)512 * 512 * 2, hipMemcpyDeviceToDevice, s) != hipSuccess) rc = -5;
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    return rc;
}

int ptta_op_hn_moments(const ptta_hn_moments_args* a, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!a) return -22;
    if (a->bn && (!a->gamma || !a->beta || !a->mean || !a->inv || !a->scale || !a->shift || (a->rm != nullptr) != (a->rv != nullptr))) return -22;
    OpBufs m;
    double* scratch = nullptr;
    if (a->r >= 1 && a->npass >= 1 && (double)a->r * a->npass < 2.0e9) {
        scratch = (double*)m.get((size_t)a->npass * (size_t)ptta_hn_moment_scratch((long)a->r) * sizeof(double));
        if (!m.ok) return -12;
    }
    HnBnOut bo;
    bo.gamma = a->gamma; bo.beta = a->beta; bo.eps = a->eps; bo.momentum = a->momentum; bo.rm = a->rm; bo.rv = a->rv; bo.nbt = a->nbt;
    bo.mean = a->mean; bo.inv = a->inv; bo.scale = a->scale; bo.shift = a->shift;
    int rc = ptta_launch_hn_moments(a->X, a->x_bf16, (long)a->r, a->npass, a->W0, a->b0, scratch, a->part, a->bn ? &bo : nullptr, s);
    if (rc > 0) rc = -5;
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    return rc;
}

int ptta_op_hn_untile(const void* src_tiled, float* dst, long long r, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!src_tiled || !dst || r < 1 || (double)r * 512 > 2.0e9) return -22;
    int rc = ptta_launch_hn_untile(src_tiled, dst, (long)r, s);
    if (rc > 0) rc = -5;
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    return rc;
}

int ptta_op_head_bwd_finish(const double* k12, const float* W0, const float* P, const float* X, long long r, void* dX, int halves, int dx_bf16,
                            ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!k12 || !W0 || !P || !X || !dX || r < 1 || (double)r * 32 > 2.0e9 || (halves != 1 && halves != 2)) return -22;
    int rc = ptta_launch_head_bwd_finish(k12, W0, P, X, (long)r, dX, s, halves, dx_bf16 ? 1 : 0);
    if (rc > 0) rc = -5;
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    return rc;
}

}  // extern "C"
