// Entry points that take no handle: outlier removal, evaluation metrics, the modulated deformable convolution, and the
// stand-alone operator launches tests and tools/ time (ptta_op_conv32, ptta_op_gwgrad, ptta_op_conv32_chain).
#include "msgchn_ctx.h"

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
    if (epi_flags & 16) {                  // the layer loop: `reps` dependent layers per LAUNCH, a device-wide barrier between layers (conv32.hip)
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

}  // extern "C"
