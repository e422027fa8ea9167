// libptta_hip: handle, workspace, weight registry and the launch schedule of one ProxyTTA step
// for the MSG_CHN backbone (C-ABI in include/ptta.h).
//
// Schedule = the dataflow of network_adapt._rgbd_meta_contrast
// (external_src/MSG_CHN/workspace/exp_msg_chn/network_exp_msg_chn_adapt.py:463-557) with
//   * the grad pass and the no-grad proxy (zero image) pass batched into ONE launch per layer
//     (batch = [real frames | proxy frames]); the depth-only encoder of stage 1 is shared,
//   * every elementwise op of the graph (pre-activation ReLU, bias, decoder skip additions,
//     bilinear x2 skip, final residual) fused into the producing/consuming conv,
//   * the minimal backward: data gradients only along paths that reach conv1_rgb_meta, weight
//     gradient only for conv1_rgb_meta, then Adam on device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ptta.h"
#include "ptta_common.h"
#include "ptta_kernels.h"
#include "nlspn.h"

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return c->fail(std::string(#x) + ": " + hipGetErrorString(e_), -100 - (int)e_); } while (0)
// (the message keeps the chain of failing calls: "outer failed <- inner failed <- reason")
#define RUN(x) do { int r_ = (x); if (r_ != 0) return c->fail_chain(std::string(#x) + " failed", r_ < 0 ? r_ : -r_); } while (0)

namespace {

// Diagnostic (option "stamps", tools/step_stamps.py): wall-clock stamps written by one-thread nodes of the step's graph (ticks since
// stamp 0) -- where a replayed step's branches start and end WITHOUT a profiler attached (rocprofv3 slows the host enough to reorder them)
// device-to-device copies of the step (the next frame into the handle's staging buffers, the depth map and the four loss scalars out): a
// kernel on the step's stream instead of hipMemcpyAsync -- the runtime's copy carries system-scope fences (what the host may read), these
// are read by later work of the same device
static __global__ void d2d_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, long n4, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) ((float4*)dst)[i] = ((const float4*)src)[i];
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) dst[4 * n4 + threadIdx.x] = src[4 * n4 + threadIdx.x];
}
static hipError_t d2d_copy(void* dst, const void* src, size_t bytes, hipStream_t s) {
    if ((bytes & 3) || (((uintptr_t)dst | (uintptr_t)src) & 15)) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s);
    const long n = (long)(bytes / 4), n4 = n / 4;
    long blocks = (n4 + 255) / 256; if (blocks < 1) blocks = 1; if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(d2d_copy_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const float*)src, (float*)dst, n4, n);
    return hipGetLastError();
}
// events that order the handle's own streams among themselves (fork / join inside a step, prefix -> step): no timing, no system-scope fence --
// nothing the host or another device reads is published by them (ev_replay, which the host waits on before it destroys a graph, keeps the default)
static constexpr unsigned kStepEvent = hipEventDisableTiming | hipEventDisableSystemFence;
static __global__ void stamp_kernel(float* out, unsigned long long* base, int i) {
    const unsigned long long t = wall_clock64();
    if (i == 0) { *base = t; out[0] = 0.f; } else out[i] = (float)(long long)(t - *base);
}
struct L32 { ConvW f{}, b{}; float* bias = nullptr; int transposed = 0; };
struct LIn { float *wfrag = nullptr, *wcanon = nullptr, *bias = nullptr, *bw = nullptr; int cin = 1; };
struct LOut { float *w = nullptr, *bias = nullptr, *bfrag = nullptr, *bcanon = nullptr; };
struct Lin { float *W = nullptr, *Wt = nullptr, *bias = nullptr; bf16_t *Whi = nullptr, *Wlo = nullptr, *Wthi = nullptr, *Wtlo = nullptr, *Wil = nullptr, *Wtil = nullptr;
             bf16_t *Wsl = nullptr, *Wtsl = nullptr;      // slice-major bf16 images of W / W^T for the narrow heads (heads_n.hip), 512 x 512 layers
             int N = 0, K = 0; };
struct BNorm { float *gamma = nullptr, *beta = nullptr, *rm = nullptr, *rv = nullptr; long long* nbt = nullptr;
               float *mean = nullptr, *inv = nullptr, *scale = nullptr, *shift = nullptr; };
struct Dbg { const void* p; long numel; int is_act; };

}  // namespace

struct ImgNorm { int on; float div; float mean[3]; float stdv[3]; };

struct ptta_ctx {
    GNet* nl = nullptr;              // backbones on the generic layer-graph engine (NLSPN, CostDCNet): every entry point forwards to it
    int N = 1, H = 0, W = 0, Hp = 0, Wp = 0, pt = 0, pr = 0, dual = 0, Nn = 1;
    int bf16 = 0, naive = 0, es = 4, x3 = 1;
    // MIXED storage / arithmetic (PTTA_DTYPE_MIXED, BASELINE config 2): the REAL frames' forward -- what produces the scored depth map -- stays
    // fp32 storage + bf16x3 arithmetic; every tensor the reference computes under no_grad / detaches (the zero-image proxy pass,
    // network_exp_msg_chn_adapt.py:509-532) and every data gradient of loss.backward() (src/tta_main.py:632) is a NARROW map: bf16 storage,
    // one bf16 MFMA per product, fp32 accumulate.  The two passes are separate launch chains (real on the caller's stream, proxy on the
    // auxiliary one); a [real | proxy] fp32 map `p` has a narrow twin for its proxy frames (tw(p)); masks reach the backward as sign bits.
    int mixed = 0;
    // the three narrow classes of the mixed mode, individually switchable for the precision budget (include/ptta.h PTTA_MIXED_KEEP_*):
    // nar_proxy: the proxy chain on narrow maps (two launch chains); nar_bwd: narrow gradient maps; nar_heads: heads_n.hip
    int nar_proxy = 0, nar_bwd = 0, nar_heads = 0;
    std::unordered_map<const void*, void*> ntwin;
    void* tw(const void* p) const { auto it = ntwin.find(p); return it == ntwin.end() ? nullptr : it->second; }
    void twin_alloc(const void* p, int nb, int h, int w) { if (nar_proxy && p) ntwin[p] = dalloc((size_t)nb * h * w * 32 * 2); }
    float *dm_f32 = nullptr;          // fp32 copy of the meta layer's output gradient (the weight-gradient kernels take fp32 operands)
    ptta_hparams hp{};
    std::string err;
    std::vector<void*> allocs;
    std::map<std::string, L32> l32;
    std::map<std::string, LIn> lin_in;
    std::map<std::string, LOut> lout;
    std::map<std::string, Lin> fc;
    std::map<std::string, BNorm> bn;
    std::map<std::string, Dbg> dbg;
    // adapted parameters (bound, caller-owned) in state_dict order; g = internal gradient buffer
    int meta_mode = 0;
    struct Adapted { std::string name; long n = 0; float *p = nullptr, *m = nullptr, *v = nullptr, *g = nullptr; };
    std::vector<Adapted> adapted;
    // stage-2 head trainer: the twelve proj / pred parameters (bound like the adapted ones) + the six
    // proj_t parameters the EMA writes; everything below is allocated by the first ptta_head_bind
    struct HeadT { bool ready = false; std::vector<Adapted> prm, tgt; bool has_grad[12] = {};
                   float *hyper = nullptr, *tau2 = nullptr, *loss = nullptr, *loss_part = nullptr, *wpart = nullptr, *bpart = nullptr, *dp = nullptr;
                   float *sv_mean = nullptr, *sv_inv = nullptr, *sv_scale = nullptr, *sv_shift = nullptr;     // proj BatchNorm state of its FIRST application
                   int* step = nullptr; unsigned* ticket = nullptr; PttaAdamEntry *tab = nullptr, *etab = nullptr;
                   std::vector<PttaAdamEntry> tab_host, etab_host; int tab_n = 0; long tab_total = 0, etab_total = 0; int tab_mode = -1; bool etab_dirty = true;
                   int reverse = 1; bool fwd_ok = false, bwd_ok = false;
                   float* garena = nullptr; long garena_n = 0;      // the twelve gradients, one arena: the gradient mean is ONE message
                   int form = 0; bool stepped = false; } head;    // PTTA_HEAD_FORM_* (ptta_head_set_form); a head forward ran: the form is fixed
    int skip_dec3 = 0;               // stage-2 head forward: no depth output
    int head_swap = 0;               // heads_forward order: 0 = emb from the proxy pass (TTA, stage-2 reverse), 1 = emb from the real pass
    float *meta_w = nullptr, *meta_b = nullptr;      // 1layer aliases of adapted[0].p / adapted[1].p
    float *gW = nullptr, *gB = nullptr;
    // 2layers meta layer (Res_Conv(32,128)): four 32-channel groups
    struct Meta2 {
        ConvW w1f[4], w2f[4], w2b[4];
        void *h[4] = {}, *a1[4] = {}, *t = nullptr, *dt = nullptr, *da1 = nullptr, *dh = nullptr;
        float *st1 = nullptr, *st2 = nullptr;          // [pass 2][mean, inv, scale, shift][C]
        float *rm1 = nullptr, *rv1 = nullptr, *rm2 = nullptr, *rv2 = nullptr; long long *nbt1 = nullptr, *nbt2 = nullptr;
        float *cs_part = nullptr, *bw = nullptr;       // statistics partials; [gscale, c1, c2, scratch] x 32
        // generic-layer path (default arithmetic): the 128-channel hidden map as ONE NHWC-128 tensor, one launch per conv
        bool generic = false;
        float *gh = nullptr, *ga1 = nullptr, *gt = nullptr, *gdt = nullptr, *gda1 = nullptr, *gdh = nullptr;
        float *w1c = nullptr, *w2c = nullptr, *w2bc = nullptr;                       // canonical [tap][cin][cout] packs of the adapted weights
        bf16_t *w1hi = nullptr, *w1lo = nullptr, *w2hi = nullptr, *w2lo = nullptr, *w2bhi = nullptr, *w2blo = nullptr;
        float *gst1 = nullptr, *gst2 = nullptr, *part1 = nullptr, *part2 = nullptr, *gbw = nullptr, *gpart = nullptr, *wgp = nullptr;
    } m2;
    float* hyper = nullptr;      // device: lr b1 b2 eps wd | w_sd w_sm w_cos
    float* w3_tmp = nullptr;     // device: loss weights of the standalone loss call
    int* step_dev = nullptr; float* stamp_f = nullptr; unsigned long long* stamp_base = nullptr; int stamps = 0;
    void stamp(int i, hipStream_t s) { if (stamps) hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(1), 0, s, stamp_f, stamp_base, i); }
    PttaAdamEntry* adam_tab = nullptr; unsigned* adam_ticket = nullptr; bool adam_tab_dirty = true;
    std::vector<PttaAdamEntry> adam_host;        // stays alive: the upload reads it
    bool fwd_valid = false;
    PttaStatSync stat_sync;          // SyncBatchNorm exchange across ranks (ptta_set_stat_sync); world == 1: off
    bool proxy_rgb_valid = false;   // proxy half of c0..c4 holds the zero-image encoder outputs for the current weights
    // emb = pred(proj(feat_zero)): proj.3 and pred.0 are two Linear layers with nothing between them (network_exp_msg_chn_adapt.py:551-554)
    // -> ONE 512x512 GEMM with W' = W_pred0 W_proj3, b' = W_pred0 b_proj3 + b_pred0 (both frozen during TTA; derived in double on load)
    Lin fused_pp; bool fused_pp_valid = false; int fuse_heads = 1;
    // heads v2 (PTTA_HEADS_V2=0 restores the materialised form): proj's 512-wide hidden is never written -- its BatchNorm statistics come
    // from the second moments of the 32-channel input, the hidden is recomputed inside the 512x512 GEMMs (forward: A-operand producer;
    // backward: mask / BatchNorm-backward sums + the contraction with W0 inside the block)
    int heads_v2 = 1;
    // the fused step without a join between forward and backward: the depth terms of the loss and decoder 3's backward follow decoder 3 on the
    // main stream, the cosine rows, the finalisation and the heads' backward follow the heads on the auxiliary one; they meet where the
    // backward needs d feat (PTTA_THRU=0: join after the forward, loss launches, fork again)
    int thru = 1; bool thru_active = false;
    // option "adam_in_wgrad": the 1layer weight gradient's reduction applies Adam itself (one launch less at the end of the step) when no
    // gradient exchange sits between the two; adam_fuse_req: set by step_tail around its backward, adam_fused: the launch took it
    int adam_in_wgrad = 1; bool adam_fuse_req = false, adam_fused = false;
    // option "bwd_w2" (mixed mode): the narrow data-gradient launches take their weights as hi + lo (two MFMAs per product); 0 = one MFMA on
    // bf16-rounded weights -- round 5's form, whose systematic 2^-9 weight error separates the adapted parameters from the reference's over a
    // long horizon (profiles/r06_drift.txt)
    int bwd_w2 = 1;
    // thru step: the valid-weight partials of the loss are computed at the start of the auxiliary stream's work (backbone), from the loss inputs
    // step_body leaves here; the loss VALUES are reduced and reported on the auxiliary stream beside the backward (backbone_backward)
    const float *cnt_sparse = nullptr, *cnt_validity = nullptr;
    struct { const float *image = nullptr, *sparse = nullptr, *validity = nullptr; bool on = false; } loss_report;
    hipEvent_t ev_loss = nullptr;
    hipEvent_t ev_dpart = nullptr;
    int fuse_first = 1, fuse_head_bwd = 1;
    int cos_grad_fused = 1;          // PTTA_COS_IN_GEMM=0: the fused step writes d loss / d ref as a tensor (loss.hip cos_grad_body) instead
    bool cos_in_gemm = false;        // (set around the fused step's backward only: ptta_backward with a caller's gradient keeps the tensor form)
    void* w0frag = nullptr; float *hm_part = nullptr, *headP = nullptr; double* head_k12 = nullptr;
    // per-kernel-class HIP-event timing of the conv32 launches (bench.py roofline leg)
    // classes (include/ptta.h PTTA_PROF_*): 0/1 stride-1 32->32 conv with ReLU on load, maps above / up to 1/4 resolution; 2/3 the same
    // without ReLU (data gradients); 4/5 stride-2 / transposed; 6 the MLP heads; 7 first-layer / prediction convs (Cin <= 3 or Cout = 1)
    // and their gradients; 8 everything else (resampling, loss, weight gradient, Adam, packing: 0 algorithmic bytes by SURVEY 8d's rule)
    struct ProfClass { std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; size_t used = 0; double bytes = 0, macs = 0; long launches = 0; };
    bool prof_on = false;
    static constexpr int NPROF = 9;
    ProfClass prof[NPROF];
    std::vector<std::pair<int, size_t>> prof_seq;      // launch order of the profiling leg: (class, index into prof[class].ev) -- debug tensor "prof_seq"
    // hipGraph replay of the whole step (inputs are first copied to fixed staging buffers so that
    // the captured pointers never change); one graph per (validity given, separate loss image)
    int use_graph = 0;           // option "graph": 1 = ptta_step / ptta_step_pipelined replay captured hipGraphs; 0 (default since round 5) = they enqueue
                                 // their kernels directly on the caller's stream and the handle's own streams -- measured faster
    void* grad_comm = nullptr;       // RCCL communicator of the gradient all-reduce inside ptta_step (ptta_set_grad_sync_rccl)
    float* grad_arena = nullptr; long grad_arena_n = 0;
    int pre_sync_graph = -1, pre_sync_aux = -1;      // use_graph / use_aux as they were before ptta_set_stat_sync switched them off (-1: untouched)
    hipGraphExec_t gexec[4] = {nullptr, nullptr, nullptr, nullptr};
    hipGraph_t graph[4] = {nullptr, nullptr, nullptr, nullptr};
    hipStream_t cap_stream = nullptr;    // private stream to capture on (the caller's may be the un-capturable null stream)
    // ---- frame pipelining (ptta_step_pipelined) ----
    // Everything UPSTREAM of the adapted layer -- clamp / pooling of the sparse depth, the frozen RGB encoder, the depth-only head of the
    // stage-1 encoder -- does not depend on the parameters the previous frame's Adam step writes, so the prefix of frame k+1 runs on its own
    // stream BESIDE the rest of frame k.  Its outputs (and the staged inputs) exist twice; a set's pointers are swapped into the members the
    // launches read, and every graph is captured once per set.
    struct PreSet {
        void *c0 = nullptr, *c1 = nullptr, *c2 = nullptr, *c3 = nullptr, *c4 = nullptr, *e1_0a = nullptr, *e1_0 = nullptr, *e1_1a = nullptr;
        void *c0a = nullptr, *c1a = nullptr, *c2a = nullptr, *c3a = nullptr, *c4a = nullptr;     // the RGB encoder's intermediates: a prefix on pre_stream writes them too
        void *e1_1 = nullptr, *y1 = nullptr, *e1_2a = nullptr, *y2 = nullptr, *t1 = nullptr, *y3 = nullptr, *s1_1 = nullptr, *u1 = nullptr;
        float *dclamp = nullptr, *d12 = nullptr, *d14 = nullptr, *in_image = nullptr, *in_loss_image = nullptr, *in_sparse = nullptr, *in_validity = nullptr;
        bool proxy_valid = false, prepared = false, rest_recorded = false;
        // Frames are recognised by the caller's TOKEN (ptta.h: non-zero, one per frame content), never by pointer identity: a caller that
        // refills one staging buffer gives the new content a new token and gets a fresh prefix.
        uint64_t prep_token = 0;        // the frame whose prefix has been started into this set (0: none)
        uint64_t last_token = 0;        // the frame whose step last ran from this set: its prefix is still valid (0: none / overwritten)
    };
    PreSet pset[2];
    int cur_set = 0, pipe_cur = 0, pipe_last = 0;        // set in the members now / of the next pipelined frame / of the last processed frame
    bool pipe_ready = false, pipe_active = false, skip_prefix = false;
    const float *fb_image = nullptr, *fb_sparse = nullptr;   // frame of the last ptta_step_pipelined call that fell back to ptta_step (ptta_forward_eval_last)
    hipStream_t pre_stream = nullptr;
    hipEvent_t ev_prefix[2] = {nullptr, nullptr}, ev_rest[2] = {nullptr, nullptr}, ev_entry = nullptr;
    hipStream_t pipe_stream = nullptr; bool pipe_stream_set = false;      // the stream of the last ptta_step_pipelined call
    hipGraph_t pgraph[2] = {nullptr, nullptr}, rgraph[4][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
    hipGraphExec_t pexec[2] = {nullptr, nullptr}, rexec[4][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
    // intra-step concurrency: the MLP heads run on a second stream beside decoder 3 (forward) and beside
    // the first decoder-3 gradients (backward); fork/join with events (graph edges under capture)
    int use_aux = 1;
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_real = nullptr;
    hipEvent_t ev_side[4] = {nullptr, nullptr, nullptr, nullptr};        // backbone_backward: transposed upsamplings beside the main chain
    // profiling leg (ptta_profile): the SAME schedule with the caller's stream standing in for the second one -- every fork / join becomes an
    // event recorded and awaited on one stream (a no-op), the enqueue order is a valid serial order (a wait is always enqueued behind its
    // record), and the bracketed launches are exactly the ones the timed step runs (round 5's leg took the one-stream FALLBACK forms: two
    // extra widening launches and the fp32 loss kernels, 36 us of `rest` at batch 1 that the step does not contain)
    hipStream_t aux(hipStream_t caller) {
        if (!use_aux) return nullptr;
        if (!aux_stream) {
            if (hipStreamCreateWithFlags(&aux_stream, hipStreamNonBlocking) != hipSuccess) return nullptr;
            if (hipEventCreateWithFlags(&ev_fork, kStepEvent) != hipSuccess ||
                hipEventCreateWithFlags(&ev_join, kStepEvent) != hipSuccess ||
                hipEventCreateWithFlags(&ev_real, kStepEvent) != hipSuccess ||
                hipEventCreateWithFlags(&ev_side[0], kStepEvent) != hipSuccess || hipEventCreateWithFlags(&ev_side[1], kStepEvent) != hipSuccess ||
                hipEventCreateWithFlags(&ev_side[2], kStepEvent) != hipSuccess || hipEventCreateWithFlags(&ev_side[3], kStepEvent) != hipSuccess) { (void)hipStreamDestroy(aux_stream); aux_stream = nullptr; return nullptr; }
        }
        return prof_on ? caller : aux_stream;
    }
    float *in_image = nullptr, *in_loss_image = nullptr, *in_sparse = nullptr, *in_validity = nullptr;
    hipEvent_t ev_replay = nullptr;      // recorded after every hipGraphLaunch: a graph is only destroyed once its last replay is done
    void drop_graphs() {
        if (ev_replay) (void)hipEventSynchronize(ev_replay);
        if (pre_stream) (void)hipStreamSynchronize(pre_stream);
        for (int k = 0; k < 4; ++k) {
            if (gexec[k]) { (void)hipGraphExecDestroy(gexec[k]); gexec[k] = nullptr; }
            if (graph[k]) { (void)hipGraphDestroy(graph[k]); graph[k] = nullptr; }
            for (int p = 0; p < 2; ++p) {
                if (rexec[k][p]) { (void)hipGraphExecDestroy(rexec[k][p]); rexec[k][p] = nullptr; }
                if (rgraph[k][p]) { (void)hipGraphDestroy(rgraph[k][p]); rgraph[k][p] = nullptr; }
            }
        }
        for (int p = 0; p < 2; ++p) {
            if (pexec[p]) { (void)hipGraphExecDestroy(pexec[p]); pexec[p] = nullptr; }
            if (pgraph[p]) { (void)hipGraphDestroy(pgraph[p]); pgraph[p] = nullptr; }
            pset[p].prepared = false; pset[p].prep_token = pset[p].last_token = 0;
        }
        fb_image = fb_sparse = nullptr;
    }

    int err_code = 0;
    int fail(const std::string& m, int code) { err = m; err_code = code; return code; }
    int fail_chain(const std::string& m, int code) { err = (err_code == code && !err.empty() && err.size() < 600) ? m + " <- " + err : m; err_code = code; return code; }

    bool oom = false;
    void* dalloc(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) { oom = true; return nullptr; }
        allocs.push_back(p);
        if (hipMemset(p, 0, bytes ? bytes : 16) != hipSuccess) { oom = true; return nullptr; }
        return p;
    }
    float* falloc(size_t n) { return (float*)dalloc(n * sizeof(float)); }
    void* act(const char* name, int nb, int h, int w) {
        void* p = dalloc((size_t)nb * h * w * 32 * es);
        dbg[name] = Dbg{p, (long)nb * h * w * 32, 1};
        if (nar_proxy && nb == 2 * Nn) twin_alloc(p, Nn, h, w);          // [real | proxy] map: narrow twin of the proxy frames
        return p;
    }
    // gradient map of the backward (real frames only): narrow in the mixed mode
    void* gact(const char* name, int nb, int h, int w) {
        const int e = nar_bwd ? 2 : es;
        void* p = dalloc((size_t)nb * h * w * 32 * e);
        dbg[name] = Dbg{p, (long)nb * h * w * 32, nar_bwd ? 2 : 1};
        return p;
    }
    // Sign-bit masks (ptta_common.h Epi): for every pre-activation map the backward uses as a ReLU mask, one word per pixel of the REAL
    // frames, written by the forward epilogue that writes the map and read by the backward epilogue instead of the 128-B fp32 pixel.
    // fp32 storage, MFMA kernels (PTTA_MASK_BITS=0: float masks everywhere).  Keyed by the map's base pointer: conv32() looks its
    // output / mask operands up, so the schedule code does not name the bit planes.
    int mask_bits_on = 1;            // option "mask_bits" (0: float masks; the planes stay allocated, 4 B per pixel)
    std::unordered_map<const void*, uint32_t*> mbits;
    void mask_plane(const void* map, int nb, int h, int w) {
        if (bf16 || naive) return;
        if (mbits.count(map)) return;
        mbits[map] = (uint32_t*)dalloc((size_t)nb * h * w * sizeof(uint32_t));
    }
    uint32_t* bits_of(const void* map) const {
        if (!map || !mask_bits_on) return nullptr;
        auto it = mbits.find(map);
        return it == mbits.end() ? nullptr : it->second;
    }
    float* map1(const char* name, int nb, int h, int w) {
        float* p = falloc((size_t)nb * h * w);
        dbg[name] = Dbg{p, (long)nb * h * w, 0};
        return p;
    }

    // ---- workspace (see build_workspace) ----
    int H2, W2, H4, W4, H8, W8, H16, W16;
    long Rg = 0;                 // embedding rows = Nn * H4 * W4
    float *img_pad = nullptr, *sp_pad = nullptr, *zero_plane = nullptr;
    ImgNorm img_norm = ImgNorm{0, 1.f, {0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}};
    float *dclamp, *d12, *d14, *out1, *p12, *q, *p11, *depth_net, *depth_final, *validity_tmp;
    void *c0a, *c0, *c1a, *c1, *c2a, *c2, *m, *c3a, *c3, *c4a, *c4;
    void *e1_0a, *e1_0, *e1_1a, *e1_1, *e1_2a, *y1, *y2, *t1, *y3, *s1_1, *u1, *y4, *s0_1, *v1;
    void *e2_0a, *e2_0, *e2_1a, *e2_1, *e2_2a, *z2, *t2, *z3, *s1_2, *u2, *z4, *s0_2, *v2;
    void *e3_0a, *e3_0, *e3_1a, *e3_1, *e3_2a, *feat, *w2, *t3, *s1_3, *u3, *s0_3, *v3;
    float *h1z, *pz, *h2, *emb, *h1, *ref, *gref_buf, *gmask, *bn_part;
    double* hn_msc = nullptr;         // per-block second moments of the feature rows ([pass][block][32][33])
    float* hn_rs = nullptr;           // |emb row|^2 from the emb GEMM's epilogue
    bool cos_rows_done = false;      // the ref GEMM's epilogue produced the cosine term's row statistics and block partials (heads_n.hip EPI 5)
    bf16_t *emb_n = nullptr, *ref_n = nullptr, *h2_n = nullptr;       // mixed mode: the heads' narrow [R][512] tensors (heads_n.hip)
    float *bnb_gscale, *bnb_c1, *bnb_c2;
    float *loss_ws, *loss_info, *g_final, *g_net;
    float* loss_info_dst = nullptr;      // direct launches: the caller's loss_info_out for the step being enqueued (no 16-byte copy launch behind Adam); else loss_info
    // backward
    void *dv3, *ds0_3, *du3, *ds1_3, *dt3, *dw2, *dfeat_tot, *dz2_up, *de3_2a, *de3_1, *de3_1a, *de3_0, *de3_0a;
    void *up4_t, *up3_t, *dv2, *ds0_2, *dz4, *du2, *ds1_2, *dz3, *dt2, *dz2, *de2_2a, *de2_1, *de2_1a, *de2_0, *de2_0a, *dv1, *dm_total, *g_feat;
    float *dp11, *dq, *dp12, *dout1, *g_feat_f32;
    float* wgrad_part;
};

namespace {

// ---- small utility kernels ---------------------------------------------------------------------
__global__ void transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)rows * cols) return;
    const int r = (int)(idx / cols), cc = (int)(idx % cols);
    dst[(long)cc * rows + r] = src[idx];
}
// dual-corner zero padding (src/msg_chn_model_adapt.py:75-103): item k=0 pads top/right, k=1 bottom/left
__global__ void pad_dual_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int C, int H, int W,
                                int Hp, int Wp, int pt, int pr, ImgNorm nm = ImgNorm{0, 1.f, {0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}}) {
    const long total = (long)2 * N * C * Hp * Wp;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % Wp); long t_ = idx / Wp;
        const int y = (int)(t_ % Hp); t_ /= Hp;
        const int ch = (int)(t_ % C); t_ /= C;
        const int n = (int)(t_ % N); const int k = (int)(t_ / N);
        const int sy = k == 0 ? y - pt : y, sx = k == 0 ? x : x - pr;
        float v = 0.f;
        if (sy >= 0 && sy < H && sx >= 0 && sx < W) {
            v = src[(((long)n * C + ch) * H + sy) * W + sx];
            if (nm.on) v = (v / nm.div - nm.mean[ch]) / nm.stdv[ch];     // the reference normalises before it pads
        }
        dst[idx] = v;
    }
}
// crop both paddings and average (src/msg_chn_model_adapt.py:107-123)
__global__ void crop_avg_kernel(const float* __restrict__ net, float* __restrict__ out, int N, int H, int W, int Hp, int Wp,
                                int pt, int pr) {
    const long total = (long)N * H * W;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % W); long t_ = idx / W;
        const int y = (int)(t_ % H); const int n = (int)(t_ / H);
        const float a = net[((long)n * Hp + y + pt) * Wp + x];
        const float b = net[((long)(N + n) * Hp + y) * Wp + x + pr];
        out[idx] = (a + b) / 2.0f;
    }
}
__global__ void scatter_dual_grad_kernel(const float* __restrict__ g, float* __restrict__ gnet, int N, int H, int W, int Hp,
                                         int Wp, int pt, int pr) {
    const long total = (long)2 * N * Hp * Wp;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % Wp); long t_ = idx / Wp;
        const int y = (int)(t_ % Hp); t_ /= Hp;
        const int n = (int)(t_ % N); const int k = (int)(t_ / N);
        const int sy = k == 0 ? y - pt : y, sx = k == 0 ? x : x - pr;
        float v = 0.f;
        if (sy >= 0 && sy < H && sx >= 0 && sx < W) v = 0.5f * g[((long)n * H + sy) * W + sx];
        gnet[idx] = v;
    }
}
__global__ void validity_kernel(const float* __restrict__ sparse, float* __restrict__ v, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float s = sparse[i];
        v[i] = s > 0.f ? 1.f : s;              // torch.where(sd > 0, 1, sd), src/tta_main.py:583-586
    }
}

template <typename T>
__global__ void to_f32_kernel(const T* __restrict__ src, float* __restrict__ dst, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) dst[i] = ld(src + i);
}
template <typename T>
__global__ void from_f32_kernel(const float* __restrict__ src, T* __restrict__ dst, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) st(dst + i, src[i]);
}
inline int nblk(long n, int cap = 4096) { long b = (n + 255) / 256; return (int)(b > cap ? cap : (b < 1 ? 1 : b)); }

int pad16(int n) { return n % 16 == 0 ? 0 : (n / 16 + 1) * 16 - n; }

ConvW alloc_convw(ptta_ctx* c) {
    ConvW w;
    w.mf32 = c->falloc(9 * 4 * 64 * 4);
    w.mbf16 = (bf16_t*)c->dalloc(9 * 2 * 64 * 8 * sizeof(bf16_t));
    w.mlo = (bf16_t*)c->dalloc(9 * 2 * 64 * 8 * sizeof(bf16_t));
    w.canon = c->falloc(9 * 32 * 32);
    return w;
}

const char* kRgb32[] = {"rgb_encoder.init.2", "rgb_encoder.enc1.1", "rgb_encoder.enc1.3", "rgb_encoder.enc2.1", "rgb_encoder.enc2.3",
                        "rgb_encoder.enc3.1", "rgb_encoder.enc3.3", "rgb_encoder.enc4.1", "rgb_encoder.enc4.3"};

void build_registry(ptta_ctx* c) {
    auto add32 = [&](const std::string& n, int transposed, bool need_bwd) {
        L32 l; l.f = alloc_convw(c); if (need_bwd) l.b = alloc_convw(c);
        l.bias = c->falloc(32); l.transposed = transposed;
        c->l32[n] = l;
    };
    for (const char* n : kRgb32) add32(n, 0, false);
    for (int s = 1; s <= 3; ++s) {
        const std::string e = "depth_encoder" + std::to_string(s), d = "depth_decoder" + std::to_string(s);
        const bool bw = s >= 2;
        add32(e + ".init.2", 0, bw);
        for (const char* k : {".enc1.1", ".enc1.3", ".enc2.1", ".enc2.3"}) add32(e + k, 0, bw);
        add32(d + ".dec2.1", 1, bw); add32(d + ".dec2.3", 0, bw);
        add32(d + ".dec1.1", 1, bw); add32(d + ".dec1.3", 0, bw);
        add32(d + ".prdct.1", 0, true);
        LIn li; li.cin = (s == 1) ? 1 : 2;
        li.wfrag = c->falloc(14 * 64); li.wcanon = c->falloc(9 * 3 * 32); li.bias = c->falloc(32); li.bw = c->falloc(288);
        c->lin_in[e + ".init.0"] = li;
        LOut lo; lo.w = c->falloc(288); lo.bias = c->falloc(1); lo.bfrag = c->falloc(14 * 64); lo.bcanon = c->falloc(9 * 3 * 32);
        c->lout[d + ".prdct.3"] = lo;
    }
    {
        LIn li; li.cin = 3;
        li.wfrag = c->falloc(14 * 64); li.wcanon = c->falloc(9 * 3 * 32); li.bias = c->falloc(32); li.bw = c->falloc(288);
        c->lin_in["rgb_encoder.init.0"] = li;
    }
    {   // the adapted layer: forward fragments are re-packed from the bound parameter every forward
        L32 l; l.f = alloc_convw(c); l.bias = nullptr; c->l32["conv1_rgb_meta"] = l;
    }
    for (const char* p : {"proj", "pred"}) {
        const int din = std::string(p) == "proj" ? 32 : 512;
        Lin a; a.N = 512; a.K = din; a.W = c->falloc((size_t)512 * din); a.Wt = c->falloc((size_t)512 * din); a.bias = c->falloc(512);
        Lin b; b.N = 512; b.K = 512; b.W = c->falloc(512 * 512); b.Wt = c->falloc(512 * 512); b.bias = c->falloc(512);
        for (Lin* l : {&a, &b}) {
            const size_t ne = (size_t)l->N * l->K;
            l->Whi = (bf16_t*)c->dalloc(ne * 2); l->Wlo = (bf16_t*)c->dalloc(ne * 2);
            l->Wthi = (bf16_t*)c->dalloc(ne * 2); l->Wtlo = (bf16_t*)c->dalloc(ne * 2);
            l->Wil = (bf16_t*)c->dalloc(ne * 4); l->Wtil = (bf16_t*)c->dalloc(ne * 4);
            if (l->K == 512) { l->Wsl = (bf16_t*)c->dalloc(ne * 2); l->Wtsl = (bf16_t*)c->dalloc(ne * 2); }
        }
        c->fc[std::string(p) + ".0"] = a; c->fc[std::string(p) + ".3"] = b;
        if (std::string(p) == "proj") {
            Lin& f = c->fused_pp; f.N = 512; f.K = 512; f.W = c->falloc(512 * 512); f.bias = c->falloc(512);
            f.Whi = (bf16_t*)c->dalloc(512 * 512 * 2); f.Wlo = (bf16_t*)c->dalloc(512 * 512 * 2); f.Wil = (bf16_t*)c->dalloc(512 * 512 * 4);
            f.Wsl = (bf16_t*)c->dalloc(512 * 512 * 2);
        }
        if (std::string(p) == "proj") c->w0frag = c->dalloc(16 * 2 * 2 * 64 * 16);
        BNorm n; n.gamma = c->falloc(512); n.beta = c->falloc(512);
        n.mean = c->falloc(512); n.inv = c->falloc(512); n.scale = c->falloc(512); n.shift = c->falloc(512);
        c->bn[std::string(p) + ".1"] = n;
    }
}

void build_workspace(ptta_ctx* c) {
    const int Nn = c->Nn, B2 = 2 * Nn;
    const int H1 = c->Hp, W1 = c->Wp;
    c->H2 = H1 / 2; c->W2 = W1 / 2; c->H4 = H1 / 4; c->W4 = W1 / 4; c->H8 = H1 / 8; c->W8 = W1 / 8; c->H16 = H1 / 16; c->W16 = W1 / 16;
    const int H2 = c->H2, W2 = c->W2, H4 = c->H4, W4 = c->W4, H8 = c->H8, W8 = c->W8, H16 = c->H16, W16 = c->W16;
    c->Rg = (long)Nn * H4 * W4;
    if (c->dual) { c->img_pad = c->falloc((size_t)Nn * 3 * H1 * W1); c->sp_pad = c->falloc((size_t)Nn * H1 * W1); }
#define A_(name, nb, h, w) c->name = c->act(#name, nb, h, w)
#define M_(name, nb, h, w) c->name = c->map1(#name, nb, h, w)
    M_(dclamp, Nn, H1, W1); M_(d12, Nn, H2, W2); M_(d14, Nn, H4, W4);
    M_(out1, B2, H4, W4); M_(p12, B2, H2, W2); M_(q, B2, H2, W2); M_(p11, B2, H1, W1);
    M_(depth_net, Nn, H1, W1); M_(depth_final, c->N, c->H, c->W); M_(validity_tmp, c->N, c->H, c->W);
    A_(c0a, B2, H1, W1); A_(c0, B2, H1, W1); A_(c1a, B2, H2, W2); A_(c1, B2, H2, W2);
    A_(c2a, B2, H4, W4); A_(c2, B2, H4, W4); A_(m, B2, H4, W4);
    A_(c3a, B2, H8, W8); A_(c3, B2, H8, W8); A_(c4a, B2, H16, W16); A_(c4, B2, H16, W16);
    A_(e1_0a, Nn, H4, W4); A_(e1_0, Nn, H4, W4); A_(e1_1a, Nn, H8, W8); A_(e1_1, B2, H8, W8); A_(e1_2a, Nn, H16, W16);
    A_(y1, B2, H8, W8); A_(y2, B2, H16, W16); A_(t1, B2, H8, W8); A_(y3, B2, H8, W8); A_(s1_1, B2, H8, W8);
    A_(u1, B2, H4, W4); A_(y4, B2, H4, W4); A_(s0_1, B2, H4, W4); A_(v1, B2, H4, W4);
    A_(e2_0a, B2, H2, W2); A_(e2_0, B2, H2, W2); A_(e2_1a, B2, H4, W4); A_(e2_1, B2, H4, W4); A_(e2_2a, B2, H8, W8);
    A_(z2, B2, H8, W8); A_(t2, B2, H4, W4); A_(z3, B2, H4, W4); A_(s1_2, B2, H4, W4); A_(u2, B2, H2, W2);
    A_(z4, B2, H2, W2); A_(s0_2, B2, H2, W2); A_(v2, B2, H2, W2);
    A_(e3_0a, B2, H1, W1); A_(e3_0, B2, H1, W1); A_(e3_1a, B2, H2, W2); A_(e3_1, B2, H2, W2); A_(e3_2a, B2, H4, W4);
    A_(feat, B2, H4, W4); A_(w2, B2, H4, W4);
    A_(t3, Nn, H2, W2); A_(s1_3, Nn, H2, W2); A_(u3, Nn, H1, W1); A_(s0_3, Nn, H1, W1); A_(v3, Nn, H1, W1);
    {   // the ReLU masks of backbone_backward (real frames).  v1 is not listed: its only reader is the unfused conv^T_{1->32} kernel
        // (float mask); e*_0a only when the fused init block (conv32_first) is what writes them for every launch shape.
#define MB_(name, h, w) c->mask_plane(c->name, Nn, h, w)
        MB_(v3, H1, W1); MB_(s0_3, H1, W1); MB_(u3, H1, W1); MB_(e3_0, H1, W1);
        MB_(s1_3, H2, W2); MB_(t3, H2, W2); MB_(e3_1, H2, W2); MB_(e3_1a, H2, W2); MB_(v2, H2, W2); MB_(s0_2, H2, W2); MB_(u2, H2, W2); MB_(e2_0, H2, W2);
        MB_(w2, H4, W4); MB_(e3_2a, H4, W4); MB_(s1_2, H4, W4); MB_(t2, H4, W4); MB_(e2_1, H4, W4); MB_(e2_1a, H4, W4); MB_(s0_1, H4, W4);
        MB_(z2, H8, W8); MB_(e2_2a, H8, W8);
        // (the fused init block and the unfused first-layer kernel both write the planes of e*_0a; mixed mode: EVERY mask of the backward
        // is a bit plane -- a narrow launch cannot read an fp32 mask map -- so decoder 1's v1 gets one too)
        MB_(e3_0a, H1, W1); MB_(e2_0a, H2, W2);
        if (c->nar_bwd) MB_(v1, H4, W4);
#undef MB_
    }
    // heads
    const size_t RD = (size_t)c->Rg * 512;
    c->h1z = c->falloc(RD); c->pz = c->falloc(RD); c->h2 = c->falloc(RD); c->emb = c->falloc(RD);
    c->h1 = c->falloc(RD); c->ref = c->falloc(RD); c->gref_buf = c->falloc(RD); c->gmask = c->falloc(RD);
    c->dbg["emb"] = Dbg{c->emb, (long)RD, 0}; c->dbg["ref"] = Dbg{c->ref, (long)RD, 0};
    if (c->nar_heads) {
        const size_t te = (size_t)ptta_hn_tiled_elems(c->Rg) * 2;          // tiled layout, padded to whole 128-row blocks (heads_n.hip)
        c->emb_n = (bf16_t*)c->dalloc(te); c->ref_n = (bf16_t*)c->dalloc(te); c->h2_n = (bf16_t*)c->dalloc(te);
        c->hn_rs = c->falloc((size_t)c->Rg);
        c->hn_msc = (double*)c->dalloc((size_t)2 * ptta_hn_moment_scratch(c->Rg) * sizeof(double));
        c->dbg["emb"] = Dbg{c->emb_n, (long)RD, 3}; c->dbg["ref"] = Dbg{c->ref_n, (long)RD, 3};
    }
    c->dbg["h1"] = Dbg{c->h1, (long)RD, 0}; c->dbg["gmask"] = Dbg{c->gmask, (long)RD, 0}; c->dbg["gref"] = Dbg{c->gref_buf, (long)RD, 0};
    c->bn_part = c->falloc((size_t)ptta_gemm_row_blocks((int)c->Rg) * 2 * 512);
    c->bnb_gscale = c->falloc(512); c->bnb_c1 = c->falloc(512); c->bnb_c2 = c->falloc(512);
    c->hm_part = c->falloc((size_t)2 * ptta_gemm_row_blocks((int)c->Rg) * 2 * 512);       // statistics partials of proj.0's output, [real | proxy] rows
    c->headP = c->falloc((size_t)2 * c->Rg * 32); c->head_k12 = (double*)c->dalloc(1024 * sizeof(double));
    c->loss_ws = c->falloc((size_t)ptta_loss_ws_floats(c->N, c->H, c->W, c->Rg));
    c->loss_info = c->falloc(4);
    M_(g_final, c->N, c->H, c->W); M_(g_net, Nn, H1, W1);
    // backward (gradient maps: narrow in the mixed mode)
#define G_(name, nb, h, w) c->name = c->gact(#name, nb, h, w)
    G_(dv3, Nn, H1, W1); G_(ds0_3, Nn, H1, W1); G_(du3, Nn, H1, W1); G_(ds1_3, Nn, H2, W2); G_(dt3, Nn, H2, W2);
    G_(dw2, Nn, H4, W4); G_(dfeat_tot, Nn, H4, W4); G_(dz2_up, Nn, H8, W8); G_(de3_2a, Nn, H4, W4);
    G_(de3_1, Nn, H2, W2); G_(de3_1a, Nn, H2, W2); G_(de3_0, Nn, H1, W1); G_(de3_0a, Nn, H1, W1);
    G_(dv2, Nn, H2, W2); G_(ds0_2, Nn, H2, W2); G_(dz4, Nn, H2, W2); G_(du2, Nn, H2, W2); G_(ds1_2, Nn, H4, W4);
    G_(dz3, Nn, H4, W4); G_(dt2, Nn, H4, W4); G_(dz2, Nn, H8, W8); G_(de2_2a, Nn, H8, W8); G_(de2_1, Nn, H4, W4);
    G_(de2_1a, Nn, H4, W4); G_(de2_0, Nn, H2, W2); G_(de2_0a, Nn, H2, W2); G_(dv1, Nn, H4, W4); G_(dm_total, Nn, H4, W4);
    G_(g_feat, Nn, H4, W4); G_(up4_t, Nn, H2, W2); G_(up3_t, Nn, H4, W4);
#undef G_
    if (c->nar_bwd) c->dm_f32 = c->falloc((size_t)Nn * H4 * W4 * 32);
    if (c->nar_proxy) {
        // depth-only maps of the stage-1 encoder that the proxy chain reads (held once, fp32): narrow copies made in the prefix
        c->twin_alloc(c->e1_0, Nn, H4, W4); c->twin_alloc(c->e1_1a, Nn, H8, W8); c->twin_alloc(c->e1_2a, Nn, H16, W16);
    }
    M_(dp11, Nn, H1, W1); M_(dq, Nn, H2, W2); M_(dp12, Nn, H2, W2); M_(dout1, Nn, H4, W4);
    c->g_feat_f32 = c->falloc((size_t)c->Rg * 32);
    c->dbg["g_feat_f32"] = Dbg{c->g_feat_f32, c->Rg * 32, 0};
    { const size_t a = (size_t)ptta_wgrad_chunks(c->Rg) * 10 * 1024, b = (size_t)ptta_gwgrad_mfma_part_floats(c->Rg, 32, 32);
      c->wgrad_part = c->falloc(a > b ? a : b); }
    {
        const char* p2 = "conv1_rgb_meta.conv1_meta.";
        std::vector<std::pair<std::string, long>> names;
        if (c->meta_mode == PTTA_META_2LAYERS)
            names = {{std::string(p2) + "0.0.weight", 128L * 32 * 9}, {std::string(p2) + "0.1.weight", 128}, {std::string(p2) + "0.1.bias", 128},
                     {std::string(p2) + "1.weight", 32L * 128 * 9}, {std::string(p2) + "1.bias", 32}, {std::string(p2) + "2.weight", 32},
                     {std::string(p2) + "2.bias", 32}};
        else names = {{"conv1_rgb_meta.weight", 9216}, {"conv1_rgb_meta.bias", 32}};
        // one arena for every adapted gradient: the shared-parameter step all-reduces it as ONE message (ptta_set_grad_sync_rccl)
        long gtot = 0; for (auto& nm : names) gtot += (nm.second + 3) & ~3L;
        c->grad_arena = c->falloc((size_t)gtot); c->grad_arena_n = gtot;
        long goff = 0;
        for (auto& nm : names) { ptta_ctx::Adapted ad; ad.name = nm.first; ad.n = nm.second; ad.g = c->grad_arena + goff; goff += (nm.second + 3) & ~3L; c->adapted.push_back(ad); }
        if (c->meta_mode == PTTA_META_2LAYERS) {
            auto& m2 = c->m2;
            for (int g = 0; g < 4; ++g) {
                m2.w1f[g] = alloc_convw(c); m2.w2f[g] = alloc_convw(c); m2.w2b[g] = alloc_convw(c);
                m2.h[g] = c->act(("meta_h" + std::to_string(g)).c_str(), B2, H4, W4);
                m2.a1[g] = c->act(("meta_a" + std::to_string(g)).c_str(), B2, H4, W4);
            }
            m2.t = c->act("meta_t", B2, H4, W4); m2.dt = c->act("meta_dt", Nn, H4, W4);
            m2.da1 = c->act("meta_da1", Nn, H4, W4); m2.dh = c->act("meta_dh", Nn, H4, W4);
            m2.st1 = c->falloc(2 * 4 * 128); m2.st2 = c->falloc(2 * 4 * 32);
            m2.cs_part = c->falloc((size_t)ptta_chan_stats_blocks() * 2 * 32); m2.bw = c->falloc(4 * 32);
            m2.generic = !c->bf16 && !c->naive && c->x3;
            if (m2.generic) {
                const size_t px2 = (size_t)B2 * H4 * W4, px1 = (size_t)Nn * H4 * W4;
                m2.gh = c->falloc(px2 * 128); m2.ga1 = c->falloc(px2 * 128); m2.gt = c->falloc(px2 * 32);
                m2.gdt = c->falloc(px1 * 32); m2.gda1 = c->falloc(px1 * 128); m2.gdh = c->falloc(px1 * 128);
                m2.w1c = c->falloc(9 * 32 * 128); m2.w2c = c->falloc(9 * 128 * 32); m2.w2bc = c->falloc(9 * 32 * 128);
                m2.w1hi = (bf16_t*)c->dalloc(2 * ptta_gfrag_elems(9, 32, 0, 128)); m2.w1lo = (bf16_t*)c->dalloc(2 * ptta_gfrag_elems(9, 32, 0, 128));
                m2.w2hi = (bf16_t*)c->dalloc(2 * ptta_gfrag_elems(9, 128, 0, 32)); m2.w2lo = (bf16_t*)c->dalloc(2 * ptta_gfrag_elems(9, 128, 0, 32));
                m2.w2bhi = (bf16_t*)c->dalloc(2 * ptta_gfrag_elems(9, 32, 0, 128)); m2.w2blo = (bf16_t*)c->dalloc(2 * ptta_gfrag_elems(9, 32, 0, 128));
                m2.gst1 = c->falloc(4 * 2 * 128); m2.gst2 = c->falloc(4 * 2 * 32);
                const size_t tiles = (size_t)ptta_gconv_x3_tiles(B2, H4, W4);
                m2.part1 = c->falloc(tiles * 2 * 128); m2.part2 = c->falloc(tiles * 2 * 32);
                m2.gbw = c->falloc(3 * 128); m2.gpart = c->falloc((size_t)ptta_gbn_part_floats(128, 1));
                m2.wgp = c->falloc((size_t)ptta_gwgrad_mfma_part_floats((long)px1, 128, 32));
            }
        }
    }
    c->gW = c->adapted[0].g; c->gB = c->adapted[1].g;
    c->dbg["gW"] = Dbg{c->gW, 9216, 0}; c->dbg["gB"] = Dbg{c->gB, 32, 0};
    c->in_image = c->falloc((size_t)c->N * 3 * c->H * c->W); c->in_loss_image = c->falloc((size_t)c->N * 3 * c->H * c->W);
    c->in_sparse = c->falloc((size_t)c->N * c->H * c->W); c->in_validity = c->falloc((size_t)c->N * c->H * c->W);
    c->hyper = c->falloc(16); c->w3_tmp = c->falloc(4);
    c->step_dev = (int*)c->dalloc(16); c->stamp_f = c->falloc(16); c->stamp_base = (unsigned long long*)c->dalloc(8); c->dbg["stamps"] = Dbg{c->stamp_f, 16, 0};
    c->adam_tab = (PttaAdamEntry*)c->dalloc(8 * sizeof(PttaAdamEntry)); c->adam_ticket = (unsigned*)c->dalloc(16);
#undef A_
#undef M_
}

// one bracketed group of launches of the profiling leg (ptta_profile): events on the launch stream, nothing when profiling is off
struct ProfScope {
    ptta_ctx::ProfClass* pc = nullptr; hipStream_t s;
    ProfScope(ptta_ctx* c, int klass, hipStream_t s_, double bytes, double macs, int launches) : s(s_) {
        if (!c->prof_on) return;
        pc = &c->prof[klass];
        if (pc->used == pc->ev.size()) {
            hipEvent_t e0, e1;
            if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { pc = nullptr; return; }
            pc->ev.push_back({e0, e1});
        }
        pc->bytes += bytes; pc->macs += macs; pc->launches += launches;
        c->prof_seq.push_back({klass, pc->used});
        (void)hipEventRecord(pc->ev[pc->used].first, s);
    }
    ~ProfScope() { if (pc) { (void)hipEventRecord(pc->ev[pc->used].second, s); pc->used++; } }
};
// first-layer / prediction convolutions (class 7): Cin <= 3 -> 32 and 32 -> 1, forward and as each other's data gradient
int conv_in_p(ptta_ctx* c, const ConvInArgs& a_, hipStream_t s) {
    ConvInArgs a = a_;
    const double px = (double)a.B * a.H * a.W;
    ProfScope ps(c, 7, s, px * (a.cin * 4 + 32 * (a.bf16 ? 2 : c->es)) + 9.0 * a.cin * 32 * 4, px * 9.0 * a.cin * 32, 1);
    if (!c->mbits.empty()) {
        // sign-bit planes: a masked launch reads its mask's plane when there is one (a narrow launch must); a launch that starts at frame 0
        // of a map the backward masks with writes that map's plane for the real frames
        if (!a.mask_bits) a.mask_bits = c->bits_of(a.mask);
        if (!a.bf16 && !a.a_bits) { a.a_bits = c->bits_of(a.out_raw); a.a_bits_nb = c->Nn; }
    }
    return ptta_launch_conv_in(a, s);
}
int conv_out1_p(ptta_ctx* c, const ConvOut1Args& a, hipStream_t s) {
    const double px = (double)a.B * a.H * a.W;
    ProfScope ps(c, 7, s, px * (32 * (a.bf16 ? 2 : c->es) + 4) + 288 * 4, px * 288.0, 1);
    return ptta_launch_conv_out1(a, s);
}
#define REST_(s_, call) do { ProfScope ps_(c, 8, (s_), 0, 0, 1); RUN(call); } while (0)

struct E { const void* up = nullptr; int up_nb = 1; const void* mask = nullptr; int mask_nb = 1;
           const void* add1 = nullptr; int add1_nb = 1; const void* add2 = nullptr; int add2_nb = 1;
           void* raw = nullptr; void* sum = nullptr;
           bool nar = false; };      // nar: a launch over NARROW maps (mixed mode: the proxy chain; every backward launch is one anyway)

int conv32(ptta_ctx* c, hipStream_t s, const std::string& layer, bool bwd, int mode, const void* in, int in_nb,
           int B, int Hin, int Win, bool relu, const E& e) {
    auto it = c->l32.find(layer);
    if (it == c->l32.end()) return c->fail("unknown 32->32 layer " + layer, -2);
    Conv32Args a;
    a.in = in; a.in_nb = in_nb; a.w = bwd ? &it->second.b : &it->second.f;
    a.bias = bwd ? nullptr : (layer == "conv1_rgb_meta" ? c->meta_b : it->second.bias);
    a.up = e.up; a.up_nb = e.up_nb; a.mask = e.mask; a.mask_nb = e.mask_nb;
    a.add1 = e.add1; a.add1_nb = e.add1_nb; a.add2 = e.add2; a.add2_nb = e.add2_nb;
    a.out_raw = e.raw; a.out_sum = e.sum;
    const bool nar = e.nar || (bwd && c->nar_bwd);
    const int es_l = nar ? 2 : c->es;
    a.B = B; a.Hin = Hin; a.Win = Win; a.mode = mode; a.relu_in = relu ? 1 : 0; a.bf16 = nar ? 1 : c->bf16; a.naive = c->naive; a.x3 = c->x3;
    a.w2 = (bwd && c->nar_bwd && c->bwd_w2) ? 1 : 0;
    if (!c->mbits.empty()) {
        // sign-bit masks: the backward reads the bits of its mask; a forward launch that starts at frame 0 of a map the backward masks
        // with writes that map's bits for the real frames (launches over the proxy half start at an offset pointer: no entry, no bits)
        a.mask_bits = c->bits_of(e.mask);
        if (!bwd && !nar) {
            uint32_t* bs = c->bits_of(e.sum); uint32_t* br = c->bits_of(e.raw);
            if (bs && br) return c->fail("conv32: both outputs of " + layer + " are registered masks", -22);
            if (bs || br) { a.bits_out = bs ? bs : br; a.bits_sum = bs ? 1 : 0; a.bits_nb = c->Nn; }
        }
    }
    // profiling leg (bench.py roofline): bracket this launch with events on ITS stream; algorithmic bytes = input + output + weight
    // elements x element size, MACs = output pixels x 9 x 32 x 32 (SURVEY.md 8d counting rule)
    const long pin = (long)B * Hin * Win;
    const long pout = mode == CONV_S1 ? pin : (mode == CONV_S2 ? pin / 4 : pin * 4);
    const bool small = (long)Hin * Win <= (long)c->H4 * c->W4 * (mode == CONV_S2 ? 4 : 1);
#ifdef PTTA_EXP_SKIP_PAIRED_S1
    // timing-only (wrong values): the stride-1 half of every (stride-2 | transposed) -> stride-1 pair on maps <= 1/4 resolution is NOT launched --
    // the upper bound of fusing each such pair into one launch
    if (mode == CONV_S1 && small && layer.size() > 2 && layer.compare(layer.size() - 2, 2, ".3") == 0 && layer.find("prdct") == std::string::npos) return 0;
#endif
    ProfScope ps(c, (mode == CONV_S1 ? (relu ? 0 : 2) : 4) + (small ? 1 : 0), s, (double)((pin + pout) * 32 + 9216) * es_l,
                 (double)(mode == CONV_T2 ? pin : pout) * 9.0 * 32.0 * 32.0, 1);
    return ptta_launch_conv32(a, s);
}

int conv32w(ptta_ctx* c, hipStream_t s, const ConvW* w, const float* bias, const void* in, int in_nb, int B, int H, int W, const E& e) {
    Conv32Args a;
    a.in = in; a.in_nb = in_nb; a.w = w; a.bias = bias;
    a.add1 = e.add1; a.add1_nb = e.add1_nb; a.out_raw = e.raw; a.out_sum = e.sum;
    a.B = B; a.Hin = H; a.Win = W; a.mode = CONV_S1; a.relu_in = 0; a.bf16 = c->bf16; a.naive = c->naive; a.x3 = c->x3;
    return ptta_launch_conv32(a, s);
}

// Conv2d(cin <= 3, 32) - ReLU - Conv2d(32, 32) of an encoder stage's `init` block: ONE launch where the fused form applies
// (conv32.hip conv32_s1_first_kernel; PTTA_FUSE_FIRST=0 or any other mode: the two launches).  `f`: the first convolution (out_raw = where
// its pre-activation map goes), a_nb: how many leading frames of that map are still needed (the backward's ReLU mask), 0: none.
int conv32_first(ptta_ctx* c, hipStream_t s, const std::string& layer, ConvInArgs& f, int a_nb, int B, int H, int W, const E& e) {
    auto it = c->l32.find(layer);
    if (it == c->l32.end()) return c->fail("unknown 32->32 layer " + layer, -2);
    const long tiles = (long)B * ((W + 31) / 32) * ((H + 7) / 8);
    const bool nar = e.nar;
    f.bf16 = nar ? 1 : c->bf16;
    if (c->fuse_first >= (f.cin == 3 ? 2 : 1) && !c->bf16 && !c->naive && c->x3 && tiles > 256 && !e.mask && !e.add1 && !e.add2 && !e.sum) {
        Conv32Args a;
        a.in = nullptr; a.in_nb = B; a.w = &it->second.f; a.bias = it->second.bias;
        a.up = e.up; a.up_nb = e.up_nb; a.out_raw = e.raw;
        a.B = B; a.Hin = H; a.Win = W; a.mode = CONV_S1; a.relu_in = 1; a.bf16 = nar ? 1 : 0; a.naive = 0; a.x3 = 1;
        const double px = (double)B * H * W;
        // (both layers' algorithmic bytes and MACs: the launch executes both; the input planes are fp32, the 32-channel maps es_l wide)
        const int es_l = nar ? 2 : c->es;
        ProfScope ps(c, 0, s, (px * f.cin + 9.0 * f.cin * 32) * 4 + (px * 96 + 9216) * es_l, px * 9.0 * (f.cin * 32 + 1024), 1);
        // the first convolution's pre-activation map is the backward's ReLU mask and nothing else: with a bit plane only its sign bits are
        // written (a_bits), not the 128-B pixels (PTTA_KEEP_FIRST_MAP=1 writes both)
        f.a_bits = (a_nb > 0 && !nar) ? c->bits_of(f.out_raw) : nullptr;
        if (!c->mbits.empty() && !nar) { uint32_t* br = c->bits_of(e.raw); if (br) { a.bits_out = br; a.bits_nb = c->Nn; } }
        const int rc = ptta_launch_conv32_first(a, f, (a_nb > 0 && !nar && !f.a_bits) ? f.out_raw : nullptr, a_nb, s);
        return rc == 1 ? c->fail("conv32_first: fused form refused a case its caller accepted", -22) : rc;
    }
    RUN(conv_in_p(c, f, s));
    return conv32(c, s, layer, false, CONV_S1, f.out_raw, B, B, H, W, true, e);
}

// Backward of a prediction head in one launch: d v = conv^T_{1->32}(g) * (v > 0) formed per halo tile and consumed by the data gradient of
// prdct.1 (mask epilogue) -- the d v map is never written (conv32.hip conv32_s1_first_kernel<1, false, true, false, true>).  Large maps only.
int conv32_first_bwd(ptta_ctx* c, hipStream_t s, const std::string& layer, ConvInArgs& f, int B, int H, int W, const E& e) {
    auto it = c->l32.find(layer);
    if (it == c->l32.end()) return c->fail("unknown 32->32 layer " + layer, -2);
    const long tiles = (long)B * ((W + 31) / 32) * ((H + 7) / 8);
    const bool nar = c->nar_bwd != 0;
    f.bf16 = nar ? 1 : c->bf16;
    if (c->fuse_head_bwd && c->bits_of(f.mask) && c->bits_of(e.mask) && c->fuse_first >= 1 && !c->bf16 && !c->naive && c->x3 && tiles > 256 && e.mask && e.raw && (e.add1 != nullptr) == (e.sum != nullptr) && !e.add2 && !e.up) {
        Conv32Args a;
        a.in = nullptr; a.in_nb = B; a.w = &it->second.b; a.bias = nullptr;
        a.mask = e.mask; a.mask_nb = e.mask_nb; a.out_raw = e.raw; a.add1 = e.add1; a.add1_nb = e.add1_nb; a.out_sum = e.sum;
        a.mask_bits = c->bits_of(e.mask); f.mask_bits = c->bits_of(f.mask);
        a.B = B; a.Hin = H; a.Win = W; a.mode = CONV_S1; a.relu_in = 0; a.bf16 = nar ? 1 : 0; a.naive = 0; a.x3 = 1;
        a.w2 = (nar && c->bwd_w2) ? 1 : 0;
        const double px = (double)B * H * W;
        const int es_l = nar ? 2 : c->es;
        ProfScope ps(c, 2, s, (px + 9.0 * 32) * 4 + (px * 96 + 9216) * es_l, px * 9.0 * (32 + 1024), 1);
        const int rc = ptta_launch_conv32_first(a, f, nullptr, 0, s);
        return rc == 1 ? c->fail("conv32_first_bwd: fused form refused a case its caller accepted", -22) : rc;
    }
    RUN(conv_in_p(c, f, s));
    return conv32(c, s, layer, true, CONV_S1, f.out_raw, B, B, H, W, false, e);
}

inline float* st_ptr(float* base, int C, int pass, int kind) { return base + ((size_t)pass * 4 + kind) * C; }   // kind: 0 mean 1 inv 2 scale 3 shift

// conv1_rgb_meta forward.  1layer: one conv (:1065-1071).  2layers: Res_Conv(32,128) (:28-36); in training
// mode each pass (real frames, proxy frames) is a separate forward call in the reference, so BatchNorm
// statistics are per pass and the running statistics are updated once per pass, real frames first.
int meta_forward(ptta_ctx* c, bool train, int B, hipStream_t s) {
    const int H4 = c->H4, W4 = c->W4, Nn = c->Nn;
    if (c->meta_mode == PTTA_META_1LAYER) {
        E e; e.raw = c->m;
        if (c->nar_proxy && train && B == 2 * Nn) {      // real frames here (fp32); the proxy frames' narrow launch is meta_forward_proxy()
            return conv32(c, s, "conv1_rgb_meta", false, CONV_S1, c->c2, Nn, Nn, H4, W4, false, e);
        }
        return conv32(c, s, "conv1_rgb_meta", false, CONV_S1, c->c2, B, B, H4, W4, false, e);
    }
    auto& m2 = c->m2;
    const ptta_ctx::Adapted* A = c->adapted.data();          // 0 W1, 1 g1, 2 b1, 3 W2, 4 bias2, 5 g2, 6 b2
    const long P = (long)Nn * H4 * W4;                         // pixels per pass
    const int npass = train ? B / Nn : 1;
    if (m2.generic) {
        // one matrix-core launch per convolution on NHWC-128 tensors (gconv_mfma.hip), BatchNorm statistics reduced in the
        // conv epilogues, one finalize per pass (running statistics: real frames first, then proxy frames), one apply
        if (!train && (!m2.rm1 || !m2.rv1 || !m2.rm2 || !m2.rv2)) return c->fail("meta BatchNorm running statistics not loaded", -3);
        GView x; x.p = (float*)c->c2; x.B = B; x.H = H4; x.W = W4; x.C = 32; x.ld = 32;
        GView hv = x; hv.p = m2.gh; hv.C = 128; hv.ld = 128;
        GView av = hv; av.p = m2.ga1;
        GView tv = x; tv.p = m2.gt;
        GView mv = x; mv.p = (float*)c->m;
        const int tiles_pp = ptta_gconv_x3_tiles(B / npass, H4, W4);
        auto finalize = [&](float* part, int C, const float* gamma, const float* beta, float* rm, float* rv, long long* nbt, float* st) -> int {
            if (!train) return ptta_launch_bn_eval_affine(gamma, beta, rm, rv, 1e-5f, st + 2 * C, st + 3 * C, C, s);       // npass == 1
            if (ptta_stat_sync(&c->stat_sync, part, tiles_pp, C, npass, s)) return -5;
            const int wmul = c->stat_sync.world > 1 ? c->stat_sync.world : 1;
            for (int pass = 0; pass < npass; ++pass)
                if (ptta_launch_bn_finalize(part + (size_t)pass * tiles_pp * 2 * C, tiles_pp, (int)P * wmul, C, gamma, beta, 1e-5f, 0.1f, rm, rv, nbt,
                                            st + pass * C, st + (npass + pass) * C, st + (2 * npass + pass) * C, st + (3 * npass + pass) * C, s)) return -5;
            return 0;
        };
        GX3Args a;
        a.x0 = x.p; a.C0 = 32; a.ld0 = 32; a.B = B; a.H = H4; a.W = W4;
        a.whi = (const uint4*)m2.w1hi; a.wlo = (const uint4*)m2.w1lo; a.nchunks = 1; a.nf0 = 0; a.nnf = 4;
        a.y = hv.p; a.ldy = 128; a.Cy = 128;
        if (train) { a.stat_part = m2.part1; a.stat_C = 128; a.stat_npass = npass; }
        RUN(ptta_launch_gconv_x3(a, 3, s));
        RUN(finalize(m2.part1, 128, A[1].p, A[2].p, m2.rm1, m2.rv1, m2.nbt1, m2.gst1));
        RUN(ptta_launch_gbn_apply(hv, GView(), av, npass, GACT_LRELU, m2.gst1, 0, s));
        GX3Args b2;
        b2.x0 = av.p; b2.C0 = 128; b2.ld0 = 128; b2.B = B; b2.H = H4; b2.W = W4;
        b2.whi = (const uint4*)m2.w2hi; b2.wlo = (const uint4*)m2.w2lo; b2.nchunks = 4; b2.nf0 = 0; b2.nnf = 1;
        b2.y = tv.p; b2.ldy = 32; b2.Cy = 32; b2.bias = A[4].p;
        if (train) { b2.stat_part = m2.part2; b2.stat_C = 32; b2.stat_npass = npass; }
        RUN(ptta_launch_gconv_x3(b2, 3, s));
        RUN(finalize(m2.part2, 32, A[5].p, A[6].p, m2.rm2, m2.rv2, m2.nbt2, m2.gst2));
        RUN(ptta_launch_gbn_apply(tv, x, mv, npass, GACT_NONE, m2.gst2, 0, s));            // + x, no activation (Res_Conv.forward :35-36)
        return 0;
    }
    const int nblk = ptta_chan_stats_blocks();
    for (int g = 0; g < 4; ++g) { E e; e.raw = m2.h[g]; RUN(conv32w(c, s, &m2.w1f[g], nullptr, c->c2, B, B, H4, W4, e)); }
    if (train) {
        for (int pass = 0; pass < npass; ++pass)
            for (int g = 0; g < 4; ++g) {
                RUN(ptta_launch_chan_stats32(m2.h[g], nullptr, c->bf16, pass * P, P, nullptr, nullptr, nullptr, nullptr, -1.f, m2.cs_part, s));
                RUN(ptta_launch_bn_finalize(m2.cs_part, nblk, (int)P, 32, A[1].p + 32 * g, A[2].p + 32 * g, 1e-5f, 0.1f,
                                            m2.rm1 ? m2.rm1 + 32 * g : nullptr, m2.rv1 ? m2.rv1 + 32 * g : nullptr, g == 0 ? m2.nbt1 : nullptr,
                                            st_ptr(m2.st1, 128, pass, 0) + 32 * g, st_ptr(m2.st1, 128, pass, 1) + 32 * g,
                                            st_ptr(m2.st1, 128, pass, 2) + 32 * g, st_ptr(m2.st1, 128, pass, 3) + 32 * g, s));
            }
    } else {
        if (!m2.rm1 || !m2.rv1 || !m2.rm2 || !m2.rv2) return c->fail("meta BatchNorm running statistics not loaded", -3);
        RUN(ptta_launch_bn_eval_affine(A[1].p, A[2].p, m2.rm1, m2.rv1, 1e-5f, st_ptr(m2.st1, 128, 0, 2), st_ptr(m2.st1, 128, 0, 3), 128, s));
    }
    for (int g = 0; g < 4; ++g)
        RUN(ptta_launch_bn_apply32(m2.h[g], nullptr, m2.a1[g], c->bf16, (long)B * H4 * W4, train ? P : (long)B * H4 * W4,
                                   st_ptr(m2.st1, 128, 0, 2) + 32 * g, st_ptr(m2.st1, 128, 0, 3) + 32 * g, 4 * 128, 0.2f, s));
    for (int g = 0; g < 4; ++g) {
        E e;
        if (g == 0) e.raw = m2.t; else { e.add1 = m2.t; e.add1_nb = B; e.sum = m2.t; }
        RUN(conv32w(c, s, &m2.w2f[g], g == 0 ? A[4].p : nullptr, m2.a1[g], B, B, H4, W4, e));
    }
    if (train) {
        for (int pass = 0; pass < npass; ++pass) {
            RUN(ptta_launch_chan_stats32(m2.t, nullptr, c->bf16, pass * P, P, nullptr, nullptr, nullptr, nullptr, -1.f, m2.cs_part, s));
            RUN(ptta_launch_bn_finalize(m2.cs_part, nblk, (int)P, 32, A[5].p, A[6].p, 1e-5f, 0.1f, m2.rm2, m2.rv2, m2.nbt2,
                                        st_ptr(m2.st2, 32, pass, 0), st_ptr(m2.st2, 32, pass, 1), st_ptr(m2.st2, 32, pass, 2), st_ptr(m2.st2, 32, pass, 3), s));
        }
    } else {
        RUN(ptta_launch_bn_eval_affine(A[5].p, A[6].p, m2.rm2, m2.rv2, 1e-5f, st_ptr(m2.st2, 32, 0, 2), st_ptr(m2.st2, 32, 0, 3), 32, s));
    }
    RUN(ptta_launch_bn_apply32(m2.t, c->c2, c->m, c->bf16, (long)B * H4 * W4, train ? P : (long)B * H4 * W4,
                               st_ptr(m2.st2, 32, 0, 2), st_ptr(m2.st2, 32, 0, 3), 4 * 32, -1.f, s));
    return 0;
}

// gradients of the seven 2layers parameters from d m (= c->dm_total, real frames, pass 0 statistics)
int meta2_backward(ptta_ctx* c, hipStream_t s) {
    auto& m2 = c->m2;
    ptta_ctx::Adapted* A = c->adapted.data();
    const int H4 = c->H4, W4 = c->W4, Nn = c->Nn;
    const long P = (long)Nn * H4 * W4;
    if (m2.generic) {
        const int npass = 2;                                   // layout of the training forward's statistics
        GView x; x.p = (float*)c->c2; x.B = Nn; x.H = H4; x.W = W4; x.C = 32; x.ld = 32;
        GView hv = x; hv.p = m2.gh; hv.C = 128; hv.ld = 128;
        GView av = hv; av.p = m2.ga1;
        GView tv = x; tv.p = m2.gt;
        GView gm = x; gm.p = c->nar_bwd ? c->dm_f32 : (float*)c->dm_total;
        GView dt = x; dt.p = m2.gdt;
        GView da1 = hv; da1.p = m2.gda1;
        GView dh = hv; dh.p = m2.gdh;
        // BatchNorm2d(32) (no activation, the residual branch carries no adapted parameter): d gamma2, d beta2, d t
        RUN(ptta_launch_gbn_backward(tv, gm, tv, dt, GView(), npass, GACT_NONE, 0, 0, 0, A[5].p, m2.gst2, m2.gpart, m2.gbw, A[5].g, A[6].g, s, 0, &c->stat_sync));
        // conv2: weight + bias gradient (one launch over the 128 input channels), data gradient to the hidden map
        RUN(ptta_launch_gwgrad_mfma(av, dt, m2.wgp, A[3].g, A[4].g, s));
        GX3Args a;
        a.x0 = dt.p; a.C0 = 32; a.ld0 = 32; a.B = Nn; a.H = H4; a.W = W4;
        a.whi = (const uint4*)m2.w2bhi; a.wlo = (const uint4*)m2.w2blo; a.nchunks = 1; a.nf0 = 0; a.nnf = 4;
        a.y = da1.p; a.ldy = 128; a.Cy = 128;
        RUN(ptta_launch_gconv_x3(a, 3, s));
        // LeakyReLU(0.2) + BatchNorm2d(128): d gamma1, d beta1, d h; conv1 weight gradient
        RUN(ptta_launch_gbn_backward(hv, da1, av, dh, GView(), npass, GACT_LRELU, 0, 0, 0, A[1].p, m2.gst1, m2.gpart, m2.gbw, A[1].g, A[2].g, s, 0, &c->stat_sync));
        RUN(ptta_launch_gwgrad_mfma(x, dh, m2.wgp, A[0].g, nullptr, s));
        return 0;
    }
    const int nblk = ptta_chan_stats_blocks();
    float *gsc = m2.bw, *c1 = m2.bw + 32, *c2 = m2.bw + 64, *scr = m2.bw + 96;
    // BatchNorm2d(32) backward: d gamma2, d beta2, d t
    RUN(ptta_launch_chan_stats32(m2.t, c->dm_total, c->bf16, 0, P, nullptr, nullptr, st_ptr(m2.st2, 32, 0, 0), st_ptr(m2.st2, 32, 0, 1), -1.f, m2.cs_part, s));
    RUN(ptta_launch_bn2d_bwd_finalize(m2.cs_part, nblk, P, A[5].p, st_ptr(m2.st2, 32, 0, 1), A[5].g, A[6].g, gsc, c1, c2, s));
    RUN(ptta_launch_bn_bwd_apply32(m2.t, c->dm_total, m2.dt, c->bf16, P, nullptr, nullptr, st_ptr(m2.st2, 32, 0, 0), st_ptr(m2.st2, 32, 0, 1), gsc, c1, c2, -1.f, s));
    // conv2 bias gradient = per-channel sum of d t (analytically 0: the bias feeds a BatchNorm)
    RUN(ptta_launch_chan_stats32(m2.dt, nullptr, c->bf16, 0, P, nullptr, nullptr, nullptr, nullptr, -1.f, m2.cs_part, s));
    RUN(ptta_launch_bn2d_bwd_finalize(m2.cs_part, nblk, P, A[5].p, st_ptr(m2.st2, 32, 0, 1), nullptr, A[4].g, scr, scr, scr, s));
    for (int g = 0; g < 4; ++g) {
        // conv2 weight gradient, input-channel group g
        RUN(ptta_launch_wgrad32(m2.a1[g], m2.dt, c->bf16, Nn, H4, W4, c->wgrad_part, A[3].g + (size_t)32 * g * 9, nullptr, s, 128 * 9));
        // d a1_g, then LeakyReLU + BatchNorm2d(128) backward for this group
        { E e; e.raw = m2.da1; RUN(conv32w(c, s, &m2.w2b[g], nullptr, m2.dt, Nn, Nn, H4, W4, e)); }
        const float* sc1 = st_ptr(m2.st1, 128, 0, 2) + 32 * g; const float* sh1 = st_ptr(m2.st1, 128, 0, 3) + 32 * g;
        const float* mu1 = st_ptr(m2.st1, 128, 0, 0) + 32 * g; const float* iv1 = st_ptr(m2.st1, 128, 0, 1) + 32 * g;
        RUN(ptta_launch_chan_stats32(m2.h[g], m2.da1, c->bf16, 0, P, sc1, sh1, mu1, iv1, 0.2f, m2.cs_part, s));
        RUN(ptta_launch_bn2d_bwd_finalize(m2.cs_part, nblk, P, A[1].p + 32 * g, iv1, A[1].g + 32 * g, A[2].g + 32 * g, gsc, c1, c2, s));
        RUN(ptta_launch_bn_bwd_apply32(m2.h[g], m2.da1, m2.dh, c->bf16, P, sc1, sh1, mu1, iv1, gsc, c1, c2, 0.2f, s));
        // conv1 weight gradient, output-channel group g
        RUN(ptta_launch_wgrad32(c->c2, m2.dh, c->bf16, Nn, H4, W4, c->wgrad_part, A[0].g + (size_t)g * 9216, nullptr, s, 32 * 9));
    }
    return 0;
}

// mixed mode: the adapted layer on the proxy frames (narrow).  1layer: the same convolution on the narrow copy of the zero-image features;
// 2layers: the fp32 Res_Conv block above ran on both passes (its BatchNorm statistics are per pass), the proxy half is narrowed here.
int to_narrow(ptta_ctx* c, const void* src_f32, void* dst, long n, hipStream_t s) {
    if (!src_f32 || !dst) return c->fail("to_narrow: missing narrow twin", -22);
    ProfScope ps_(c, 8, s, 0, 0, 1);
    hipLaunchKernelGGL((from_f32_kernel<bf16_t>), dim3(nblk(n)), dim3(256), 0, s, (const float*)src_f32, (bf16_t*)dst, n);
    return 0;
}
int to_wide(ptta_ctx* c, const void* src_nar, float* dst, long n, hipStream_t s) {
    if (!src_nar || !dst) return c->fail("to_wide: missing operand", -22);
    ProfScope ps_(c, 8, s, 0, 0, 1);
    hipLaunchKernelGGL((to_f32_kernel<bf16_t>), dim3(nblk(n)), dim3(256), 0, s, (const bf16_t*)src_nar, dst, n);
    return 0;
}
int meta_forward_proxy(ptta_ctx* c, hipStream_t s) {
    const int H4 = c->H4, W4 = c->W4, Nn = c->Nn;
    const long half = (long)Nn * H4 * W4 * 32;
    if (c->meta_mode == PTTA_META_1LAYER) {
        E e; e.raw = c->tw(c->m); e.nar = true;
        return conv32(c, s, "conv1_rgb_meta", false, CONV_S1, c->tw(c->c2), Nn, Nn, H4, W4, false, e);
    }
    return to_narrow(c, (const float*)c->m + half, c->tw(c->m), half, s);
}

int heads_forward(ptta_ctx* c, hipStream_t s, int part = 0);
static bool heads_v2_on(const ptta_ctx* c);
static int pipe_quiesce(ptta_ctx* c);
static void pipe_use(ptta_ctx* c, int p);
// a full forward (ptta_forward_eval / ptta_forward_train) has written an arbitrary frame's prefix into set p: whatever was prepared into it
// or adapted from it is gone.  (Set p is pipe_last; when a prefix of the SAME frame was kept there for another step -- inner_iter > 1 --
// the step that follows recomputes it in line.)
static void pipe_overwritten(ptta_ctx* c, int p) {
    ptta_ctx::PreSet& P = c->pset[p];
    if (c->pipe_cur == p) { P.prepared = false; P.prep_token = 0; }
    P.last_token = 0;
}

// RGBEncoder.forward (:252-264) on `nb` frames written at batch offset `boff` of the c0..c4 buffers; frames with index
// >= zero_from_b see a zero image (the proxy pass's torch.zeros_like(rgb), :511).
int rgb_encoder(ptta_ctx* c, const float* image, int nb, int boff, int zero_from_b, hipStream_t s) {
    const int H1 = c->Hp, W1 = c->Wp, H2 = c->H2, W2 = c->W2, H4 = c->H4, W4 = c->W4, H8 = c->H8, W8 = c->W8, H16 = c->H16, W16 = c->W16;
    auto at = [&](void* base, int h, int w) { return (void*)((char*)base + (size_t)boff * h * w * 32 * c->es); };
    auto e_raw = [](void* raw) { E e; e.raw = raw; return e; };
#define CV(...) RUN(conv32(c, s, __VA_ARGS__))
    {
        const LIn& li = c->lin_in["rgb_encoder.init.0"];
        ConvInArgs a; a.cin = 3; a.zero_from_b = zero_from_b;
        for (int ch = 0; ch < 3; ++ch) {
            a.pl[ch].p = image + (size_t)ch * H1 * W1; a.pl[ch].nb = c->Nn; a.pl[ch].bstride = 3L * H1 * W1;
            if (c->img_norm.on && !c->dual) {            // dual-corner padding normalises while it pads
                a.pl[ch].norm = 1; a.pl[ch].div = c->img_norm.div; a.pl[ch].mean = c->img_norm.mean[ch]; a.pl[ch].stdv = c->img_norm.stdv[ch];
            }
        }
        a.wfrag = li.wfrag; a.wcanon = li.wcanon; a.bias = li.bias; a.out_raw = at(c->c0a, H1, W1);
        a.B = nb; a.H = H1; a.W = W1; a.bf16 = c->bf16; a.naive = c->naive;
        RUN(conv32_first(c, s, "rgb_encoder.init.2", a, 0, nb, H1, W1, e_raw(at(c->c0, H1, W1))));       // (nothing reads the map in between)
    }
    CV("rgb_encoder.enc1.1", false, CONV_S2, at(c->c0, H1, W1), nb, nb, H1, W1, true, e_raw(at(c->c1a, H2, W2)));
    CV("rgb_encoder.enc1.3", false, CONV_S1, at(c->c1a, H2, W2), nb, nb, H2, W2, true, e_raw(at(c->c1, H2, W2)));
    CV("rgb_encoder.enc2.1", false, CONV_S2, at(c->c1, H2, W2), nb, nb, H2, W2, true, e_raw(at(c->c2a, H4, W4)));
    CV("rgb_encoder.enc2.3", false, CONV_S1, at(c->c2a, H4, W4), nb, nb, H4, W4, true, e_raw(at(c->c2, H4, W4)));
    CV("rgb_encoder.enc3.1", false, CONV_S2, at(c->c2, H4, W4), nb, nb, H4, W4, true, e_raw(at(c->c3a, H8, W8)));
    CV("rgb_encoder.enc3.3", false, CONV_S1, at(c->c3a, H8, W8), nb, nb, H8, W8, true, e_raw(at(c->c3, H8, W8)));
    CV("rgb_encoder.enc4.1", false, CONV_S2, at(c->c3, H8, W8), nb, nb, H8, W8, true, e_raw(at(c->c4a, H16, W16)));
    CV("rgb_encoder.enc4.3", false, CONV_S1, at(c->c4a, H16, W16), nb, nb, H16, W16, true, e_raw(at(c->c4, H16, W16)));
#undef CV
    return 0;
}

// The proxy pass feeds torch.zeros_like(rgb) through the frozen RGB encoder (:509-515): its c0..c4 depend only on the
// encoder weights and the frame size, so they are computed ONCE per (handle, weights) into the proxy half of the
// buffers instead of in every step (the eval forward only writes the real half).  Never runs inside a graph capture.
__global__ void fuse_linear_kernel(const float* __restrict__ Wb, const float* __restrict__ bb, const float* __restrict__ Wa, const float* __restrict__ ba,
                                   float* __restrict__ W, float* __restrict__ bias, int N, int M, int K) {
    // y = (x Wa^T + ba) Wb^T + bb = x (Wb Wa)^T + (Wb ba + bb);  Wb: [N][M], Wa: [M][K] -> W: [N][K]
    const int k = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y;
    if (k >= K) return;
    double acc = 0.0;
    for (int m = 0; m < M; ++m) acc += (double)Wb[(long)n * M + m] * (double)Wa[(long)m * K + k];
    W[(long)n * K + k] = (float)acc;
    if (k == 0) {
        double b = (double)bb[n];
        for (int m = 0; m < M; ++m) b += (double)Wb[(long)n * M + m] * (double)ba[m];
        bias[n] = (float)b;
    }
}
int ensure_fused_heads(ptta_ctx* c, hipStream_t s) {
    if (c->fused_pp_valid || !c->fuse_heads) return 0;
    Lin& f = c->fused_pp; const Lin& a = c->fc["proj.3"]; const Lin& b = c->fc["pred.0"];
    hipLaunchKernelGGL(fuse_linear_kernel, dim3(2, 512), dim3(256), 0, s, b.W, b.bias, a.W, a.bias, f.W, f.bias, 512, 512, 512);
    ptta_split_weight(f.W, f.Whi, f.Wlo, f.Wil, 512L * 512, 512, s);
    ptta_hn_pack_w(f.Whi, f.Wsl, 512, s);
    c->fused_pp_valid = true;
    return 0;
}

int ensure_proxy_rgb(ptta_ctx* c, const float* any_image, hipStream_t s) {
    RUN(ensure_fused_heads(c, s));
    if (c->proxy_rgb_valid) return 0;
    RUN(rgb_encoder(c, any_image, c->Nn, c->Nn, 0, s));
    if (c->nar_proxy) {      // what the proxy chain reads of it: the skip operands c1 .. c4 and the adapted layer's input c2, as narrow maps
        const int Nn = c->Nn;
        struct { void* p; int h, w; } maps[4] = {{c->c1, c->H2, c->W2}, {c->c2, c->H4, c->W4}, {c->c3, c->H8, c->W8}, {c->c4, c->H16, c->W16}};
        for (auto& m_ : maps) {
            const long half = (long)Nn * m_.h * m_.w * 32;
            RUN(to_narrow(c, (const float*)m_.p + half, c->tw(m_.p), half, s));
        }
    }
    c->proxy_rgb_valid = true;
    return 0;
}

// The depth-only head of the stage-1 encoder (DepthEncoder.forward :218-232 up to the first skip addition): nothing of the RGB branch in it
int enc1_head_fn(ptta_ctx* c, hipStream_t st) {
    const int Nn = c->Nn, H4 = c->H4, W4 = c->W4;
    const LIn& li = c->lin_in["depth_encoder1.init.0"];
    ConvInArgs a; a.cin = 1; a.pl[0].p = c->d14; a.pl[0].nb = Nn; a.pl[0].bstride = (long)H4 * W4;
    a.wfrag = li.wfrag; a.wcanon = li.wcanon; a.bias = li.bias; a.out_raw = c->e1_0a;
    a.B = Nn; a.H = H4; a.W = W4; a.bf16 = c->bf16; a.naive = c->naive;
    RUN(conv_in_p(c, a, st));
    { E e; e.raw = c->e1_0; RUN(conv32(c, st, "depth_encoder1.init.2", false, CONV_S1, c->e1_0a, Nn, Nn, H4, W4, true, e)); }
    { E e; e.raw = c->e1_1a; RUN(conv32(c, st, "depth_encoder1.enc1.1", false, CONV_S2, c->e1_0, Nn, Nn, H4, W4, true, e)); }
    return 0;
}

// The rest of the stage-1/4 cascade that the adapted layer does not reach: the encoder's two skip additions with the RGB features
// (:487-489) and decoder 1 down to its last transposed convolution (DepthDecoder.forward :296-305) -- conv1_rgb_meta's output enters
// at dec1.3.  B2 = images per launch ([real | proxy] in a training forward).
int stage1_independent(ptta_ctx* c, int B2, hipStream_t s) {
    const int Nn = c->Nn, H4 = c->H4, W4 = c->W4, H8 = c->H8, W8 = c->W8, H16 = c->H16, W16 = c->W16;
    const bool two = c->nar_proxy && B2 == 2 * Nn;        // mixed training forward: real frames fp32 here, proxy frames narrow below
    const int Bf = two ? Nn : B2;
    { E e; e.raw = c->e1_1; e.sum = c->y1; e.add1 = c->c3; e.add1_nb = B2;                      // y1 = e1_1 + c3
      RUN(conv32(c, s, "depth_encoder1.enc1.3", false, CONV_S1, c->e1_1a, Nn, Bf, H8, W8, true, e)); }
    { E e; e.raw = c->e1_2a; RUN(conv32(c, s, "depth_encoder1.enc2.1", false, CONV_S2, c->e1_1, B2, Nn, H8, W8, true, e)); }
    { E e; e.sum = c->y2; e.add1 = c->c4; e.add1_nb = B2;                                         // y2 = e1_2 + c4
      RUN(conv32(c, s, "depth_encoder1.enc2.3", false, CONV_S1, c->e1_2a, Nn, Bf, H16, W16, true, e)); }
    { E e; e.raw = c->t1; RUN(conv32(c, s, "depth_decoder1.dec2.1", false, CONV_T2, c->y2, B2, Bf, H16, W16, true, e)); }
    { E e; e.raw = c->y3; e.sum = c->s1_1; e.add1 = c->y1; e.add1_nb = B2;
      RUN(conv32(c, s, "depth_decoder1.dec2.3", false, CONV_S1, c->t1, B2, Bf, H8, W8, true, e)); }
    { E e; e.raw = c->u1; RUN(conv32(c, s, "depth_decoder1.dec1.1", false, CONV_T2, c->s1_1, B2, Bf, H8, W8, true, e)); }
    if (!two) return 0;
    // ---- the same six layers for the proxy frames, narrow: the depth-only inputs (held once, fp32) are narrowed first ----
    RUN(to_narrow(c, c->e1_0, c->tw(c->e1_0), (long)Nn * H4 * W4 * 32, s));
    RUN(to_narrow(c, c->e1_1a, c->tw(c->e1_1a), (long)Nn * H8 * W8 * 32, s));
    RUN(to_narrow(c, c->e1_2a, c->tw(c->e1_2a), (long)Nn * H16 * W16 * 32, s));
    { E e; e.nar = true; e.sum = c->tw(c->y1); e.add1 = c->tw(c->c3); e.add1_nb = Nn;
      RUN(conv32(c, s, "depth_encoder1.enc1.3", false, CONV_S1, c->tw(c->e1_1a), Nn, Nn, H8, W8, true, e)); }
    { E e; e.nar = true; e.sum = c->tw(c->y2); e.add1 = c->tw(c->c4); e.add1_nb = Nn;
      RUN(conv32(c, s, "depth_encoder1.enc2.3", false, CONV_S1, c->tw(c->e1_2a), Nn, Nn, H16, W16, true, e)); }
    { E e; e.nar = true; e.raw = c->tw(c->t1); RUN(conv32(c, s, "depth_decoder1.dec2.1", false, CONV_T2, c->tw(c->y2), Nn, Nn, H16, W16, true, e)); }
    { E e; e.nar = true; e.raw = c->tw(c->y3); e.sum = c->tw(c->s1_1); e.add1 = c->tw(c->y1); e.add1_nb = Nn;
      RUN(conv32(c, s, "depth_decoder1.dec2.3", false, CONV_S1, c->tw(c->t1), Nn, Nn, H8, W8, true, e)); }
    { E e; e.nar = true; e.raw = c->tw(c->u1); RUN(conv32(c, s, "depth_decoder1.dec1.1", false, CONV_T2, c->tw(c->s1_1), Nn, Nn, H8, W8, true, e)); }
    return 0;
}

// One encoder-decoder cascade.  train: batch = [Nn real | Nn proxy(zero image)], D3 only on the real half;
// the MLP heads (which only need depth_encoder3's output) run on the auxiliary stream beside decoder 3.
// Mixed mode (train): the two passes are two launch chains -- the real frames (fp32 maps, bf16x3) on `s`, the proxy frames (narrow maps,
// one MFMA per product) on the auxiliary stream from the adapted layer on; the heads follow the proxy chain there once the real chain's
// depth_encoder3 output exists.
int backbone(ptta_ctx* c, const float* image, bool train, hipStream_t s) {
    hipStream_t s2 = train ? c->aux(s) : nullptr;
    const int Nn = c->Nn, B2 = train ? 2 * Nn : Nn;
    const bool two = train && c->nar_proxy;
    const int H1 = c->Hp, W1 = c->Wp, H2 = c->H2, W2 = c->W2, H4 = c->H4, W4 = c->W4, H8 = c->H8, W8 = c->W8, H16 = c->H16, W16 = c->W16;
#define CV(...) RUN(conv32(c, s, __VA_ARGS__))
    auto e_raw = [](void* raw) { E e; e.raw = raw; return e; };
    // ---- RGB encoder (RGBEncoder.forward :252-264) + meta layer (:481-482) ----
    // train: the proxy half of c0..c4 (zero image through frozen weights) is a constant of the handle, computed once by
    // ensure_proxy_rgb(); only the real frames go through the encoder here
    if (!c->skip_prefix) RUN(rgb_encoder(c, image, Nn, 0, Nn, s));
    RUN(meta_forward(c, train, B2, s));
    // ---- stage 1/4 (:487-489): depth-only encoder shared by both passes ----
    if (!c->skip_prefix) { RUN(enc1_head_fn(c, s)); RUN(stage1_independent(c, B2, s)); }

    // ---- decoder 1, stage 1/2, encoder of stage 1/1: `Bl` frames starting at batch index b0 of the [real | proxy] batch (nar: the
    // proxy frames as narrow maps, tw(...) of each [real | proxy] map).  Tensors that hold the batch once (e1_0, d12, dclamp:
    // depth-only) are indexed modulo their own batch count and take no offset.
    auto region = [&](hipStream_t st, int b0, int Bl, bool nar) -> int {
        auto A = [&](void* p_, int h, int w) -> void* { return nar ? c->tw(p_) : (void*)((char*)p_ + (size_t)b0 * h * w * 32 * c->es); };
        auto P1 = [&](float* p_, int h, int w) { return p_ + (size_t)b0 * h * w; };
        auto raw = [&](void* r) { E e; e.raw = r; e.nar = nar; return e; };
        const void* e1_0 = nar ? c->tw(c->e1_0) : c->e1_0;
#define CR(...) RUN(conv32(c, st, __VA_ARGS__))
        // decoder 1 (DepthDecoder.forward :296-311); its first three launches are in stage1_independent()
        { E e; e.nar = nar; e.raw = A(c->y4, H4, W4); e.sum = A(c->s0_1, H4, W4); e.add1 = e1_0; e.add1_nb = Nn; e.add2 = A(c->m, H4, W4); e.add2_nb = Bl;
          CR("depth_decoder1.dec1.3", false, CONV_S1, A(c->u1, H4, W4), Bl, Bl, H4, W4, true, e); }
        CR("depth_decoder1.prdct.1", false, CONV_S1, A(c->s0_1, H4, W4), Bl, Bl, H4, W4, true, raw(A(c->v1, H4, W4)));
        {
            const LOut& lo = c->lout["depth_decoder1.prdct.3"];
            ConvOut1Args a; a.in = A(c->v1, H4, W4); a.in_nb = Bl; a.w = lo.w; a.bias = lo.bias; a.out = P1(c->out1, H4, W4);
            a.B = Bl; a.H = H4; a.W = W4; a.relu_in = 1; a.bf16 = nar ? 1 : c->bf16;
            RUN(conv_out1_p(c, a, st));
        }
        // ---- stage 1/2 (:491-498) ----
        REST_(st, ptta_launch_up2_1ch(P1(c->out1, H4, W4), P1(c->p12, H2, W2), Bl, H4, W4, st));
        {
            const LIn& li = c->lin_in["depth_encoder2.init.0"];
            ConvInArgs a; a.cin = 2;
            a.pl[0].p = c->d12; a.pl[0].nb = Nn; a.pl[0].bstride = (long)H2 * W2;
            a.pl[1].p = P1(c->p12, H2, W2); a.pl[1].nb = Bl; a.pl[1].bstride = (long)H2 * W2;
            a.wfrag = li.wfrag; a.wcanon = li.wcanon; a.bias = li.bias; a.out_raw = A(c->e2_0a, H2, W2);
            a.B = Bl; a.H = H2; a.W = W2; a.bf16 = c->bf16; a.naive = c->naive;
            // (the pre-activation map is the backward's ReLU mask for the real frames only: batch indices below Nn of a launch that starts at b0 = 0)
            E e; e.nar = nar; e.raw = A(c->e2_0, H2, W2); e.up = A(c->y4, H4, W4); e.up_nb = Bl;
            RUN(conv32_first(c, st, "depth_encoder2.init.2", a, (b0 == 0 && !nar) ? Nn : 0, Bl, H2, W2, e));
        }
        CR("depth_encoder2.enc1.1", false, CONV_S2, A(c->e2_0, H2, W2), Bl, Bl, H2, W2, true, raw(A(c->e2_1a, H4, W4)));
        { E e; e.nar = nar; e.raw = A(c->e2_1, H4, W4); e.up = A(c->y3, H8, W8); e.up_nb = Bl; CR("depth_encoder2.enc1.3", false, CONV_S1, A(c->e2_1a, H4, W4), Bl, Bl, H4, W4, true, e); }
        CR("depth_encoder2.enc2.1", false, CONV_S2, A(c->e2_1, H4, W4), Bl, Bl, H4, W4, true, raw(A(c->e2_2a, H8, W8)));
        { E e; e.nar = nar; e.sum = A(c->z2, H8, W8); e.up = A(c->y2, H16, W16); e.up_nb = Bl; e.add1 = A(c->c3, H8, W8); e.add1_nb = Bl;            // z2 = e2_2 + c3
          CR("depth_encoder2.enc2.3", false, CONV_S1, A(c->e2_2a, H8, W8), Bl, Bl, H8, W8, true, e); }
        CR("depth_decoder2.dec2.1", false, CONV_T2, A(c->z2, H8, W8), Bl, Bl, H8, W8, true, raw(A(c->t2, H4, W4)));
        { E e; e.nar = nar; e.raw = A(c->z3, H4, W4); e.sum = A(c->s1_2, H4, W4); e.add1 = A(c->e2_1, H4, W4); e.add1_nb = Bl; e.add2 = A(c->m, H4, W4); e.add2_nb = Bl;
          CR("depth_decoder2.dec2.3", false, CONV_S1, A(c->t2, H4, W4), Bl, Bl, H4, W4, true, e); }
        CR("depth_decoder2.dec1.1", false, CONV_T2, A(c->s1_2, H4, W4), Bl, Bl, H4, W4, true, raw(A(c->u2, H2, W2)));
        { E e; e.nar = nar; e.raw = A(c->z4, H2, W2); e.sum = A(c->s0_2, H2, W2); e.add1 = A(c->e2_0, H2, W2); e.add1_nb = Bl; e.add2 = A(c->c1, H2, W2); e.add2_nb = Bl;
          CR("depth_decoder2.dec1.3", false, CONV_S1, A(c->u2, H2, W2), Bl, Bl, H2, W2, true, e); }
        CR("depth_decoder2.prdct.1", false, CONV_S1, A(c->s0_2, H2, W2), Bl, Bl, H2, W2, true, raw(A(c->v2, H2, W2)));
        {
            const LOut& lo = c->lout["depth_decoder2.prdct.3"];
            ConvOut1Args a; a.in = A(c->v2, H2, W2); a.in_nb = Bl; a.w = lo.w; a.bias = lo.bias; a.add = P1(c->p12, H2, W2); a.add_nb = Bl; a.out = P1(c->q, H2, W2);
            a.B = Bl; a.H = H2; a.W = W2; a.relu_in = 1; a.bf16 = nar ? 1 : c->bf16;                           // q = out2 + p12
            RUN(conv_out1_p(c, a, st));
        }
        // ---- stage 1/1 (:500-506) ----
        REST_(st, ptta_launch_up2_1ch(P1(c->q, H2, W2), P1(c->p11, H1, W1), Bl, H2, W2, st));
        {
            const LIn& li = c->lin_in["depth_encoder3.init.0"];
            ConvInArgs a; a.cin = 2;
            a.pl[0].p = c->dclamp; a.pl[0].nb = Nn; a.pl[0].bstride = (long)H1 * W1;
            a.pl[1].p = P1(c->p11, H1, W1); a.pl[1].nb = Bl; a.pl[1].bstride = (long)H1 * W1;
            a.wfrag = li.wfrag; a.wcanon = li.wcanon; a.bias = li.bias; a.out_raw = A(c->e3_0a, H1, W1);
            a.B = Bl; a.H = H1; a.W = W1; a.bf16 = c->bf16; a.naive = c->naive;
            E e; e.nar = nar; e.raw = A(c->e3_0, H1, W1); e.up = A(c->z4, H2, W2); e.up_nb = Bl;
            RUN(conv32_first(c, st, "depth_encoder3.init.2", a, (b0 == 0 && !nar) ? Nn : 0, Bl, H1, W1, e));
        }
        CR("depth_encoder3.enc1.1", false, CONV_S2, A(c->e3_0, H1, W1), Bl, Bl, H1, W1, true, raw(A(c->e3_1a, H2, W2)));
        { E e; e.nar = nar; e.raw = A(c->e3_1, H2, W2); e.up = A(c->z3, H4, W4); e.up_nb = Bl; CR("depth_encoder3.enc1.3", false, CONV_S1, A(c->e3_1a, H2, W2), Bl, Bl, H2, W2, true, e); }
        CR("depth_encoder3.enc2.1", false, CONV_S2, A(c->e3_1, H2, W2), Bl, Bl, H2, W2, true, raw(A(c->e3_2a, H4, W4)));
        { E e; e.nar = nar; e.raw = A(c->feat, H4, W4); e.up = A(c->z2, H8, W8); e.up_nb = Bl; e.add1 = A(c->m, H4, W4); e.add1_nb = Bl;   // w2 = feat + m
          if (!nar) e.sum = A(c->w2, H4, W4); else e.add1 = nullptr;         // (the proxy pass stops at depth_encoder3: its w2 feeds nothing)
          CR("depth_encoder3.enc2.3", false, CONV_S1, A(c->e3_2a, H4, W4), Bl, Bl, H4, W4, true, e); }
#undef CR
        return 0;
    };
    if (two) {
        // real frames on s, proxy frames (narrow) on the auxiliary stream; the heads (both passes' depth_encoder3 outputs) follow there
        hipStream_t sp = s2 ? s2 : s;
        if (s2) { HIPCHK(hipEventRecord(c->ev_fork, s)); HIPCHK(hipStreamWaitEvent(s2, c->ev_fork, 0)); }
        c->stamp(3, sp);
        if (s2 && c->thru_active && c->cnt_sparse) REST_(s2, ptta_launch_loss_valid_count(c->cnt_sparse, c->cnt_validity, c->N, c->H, c->W, c->loss_ws, s2));
        RUN(meta_forward_proxy(c, sp));
        c->stamp(1, s);
        RUN(region(s, 0, Nn, false));
        c->stamp(2, s);
        RUN(region(sp, Nn, Nn, true));
        c->stamp(4, sp);
        const bool hn = c->nar_heads && heads_v2_on(c);              // narrow heads: the proxy half needs nothing of the real chain
        // (the fp32 heads -- PTTA_MIXED_KEEP_HEADS, or a configuration without heads v2 -- take fp32 features: the proxy rows are widened)
        if (!hn) RUN(to_wide(c, c->tw(c->feat), (float*)c->feat + (size_t)c->Rg * 32, c->Rg * 32, sp));
        if (s2) {
            if (hn) RUN(heads_forward(c, s2, 1));
            c->stamp(5, s2);
            HIPCHK(hipEventRecord(c->ev_real, s)); HIPCHK(hipStreamWaitEvent(s2, c->ev_real, 0));
            RUN(heads_forward(c, s2, hn ? 2 : 0));
            c->stamp(6, s2);
            HIPCHK(hipEventRecord(c->ev_join, s2));
        }
    } else {
        RUN(region(s, 0, B2, false));
        if (train && s2) {
            HIPCHK(hipEventRecord(c->ev_fork, s)); HIPCHK(hipStreamWaitEvent(s2, c->ev_fork, 0));
            if (c->thru_active && c->cnt_sparse) REST_(s2, ptta_launch_loss_valid_count(c->cnt_sparse, c->cnt_validity, c->N, c->H, c->W, c->loss_ws, s2));
            RUN(heads_forward(c, s2));
            HIPCHK(hipEventRecord(c->ev_join, s2));
        }
    }
    // decoder 3: real frames only (the proxy pass stops at depth_encoder3, :509-532); the stage-2 head forward stops at
    // depth_encoder3 for both passes (:652,:676)
    if (!c->skip_dec3) {
    CV("depth_decoder3.dec2.1", false, CONV_T2, c->w2, B2, Nn, H4, W4, true, e_raw(c->t3));
    { E e; e.sum = c->s1_3; e.add1 = c->e3_1; e.add1_nb = B2; e.add2 = c->c1; e.add2_nb = B2;
      CV("depth_decoder3.dec2.3", false, CONV_S1, c->t3, Nn, Nn, H2, W2, true, e); }
    CV("depth_decoder3.dec1.1", false, CONV_T2, c->s1_3, Nn, Nn, H2, W2, true, e_raw(c->u3));
    { E e; e.sum = c->s0_3; e.add1 = c->e3_0; e.add1_nb = B2; e.add2 = c->c0; e.add2_nb = B2;
      CV("depth_decoder3.dec1.3", false, CONV_S1, c->u3, Nn, Nn, H1, W1, true, e); }
    CV("depth_decoder3.prdct.1", false, CONV_S1, c->s0_3, Nn, Nn, H1, W1, true, e_raw(c->v3));
    {
        const LOut& lo = c->lout["depth_decoder3.prdct.3"];
        ConvOut1Args a; a.in = c->v3; a.in_nb = Nn; a.w = lo.w; a.bias = lo.bias; a.add = c->p11; a.add_nb = B2; a.out = c->depth_net;
        a.B = Nn; a.H = H1; a.W = W1; a.relu_in = 1; a.bf16 = c->bf16;                           // output = out3 + p11 (:506)
        RUN(conv_out1_p(c, a, s));
    }
    }
    c->stamp(7, s);
#undef CV
    if (train) {
        if (s2) { if (!c->thru_active) HIPCHK(hipStreamWaitEvent(s, c->ev_join, 0)); }      // (thru: the heads' stream goes on into the loss and the backward)
        else RUN(heads_forward(c, s));
    }
    return 0;
}

static bool heads_v2_on(const ptta_ctx* c) {
    return c->heads_v2 && c->fuse_heads && c->fused_pp_valid && c->x3 && !c->bf16 && !c->naive && !c->skip_dec3 && !c->head_swap;
}

// proj / pred heads (:551-554): emb = pred(proj(feat_zero)), ref = proj(feat); BN1d in train mode.
int mlp_forward(ptta_ctx* c, const std::string& name, const void* A, int a_bf16, int K, float* hidden, float* out, hipStream_t s) {
    const Lin& l0 = c->fc[name + ".0"]; const Lin& l3 = c->fc[name + ".3"]; BNorm& bn = c->bn[name + ".1"];
    const int R = (int)c->Rg;
    GemmArgs g; g.A = A; g.a_bf16 = a_bf16; g.W = l0.W; g.bias = l0.bias; g.C = hidden; g.R = R; g.K = K; g.N = 512; g.epi = 1; g.part = c->bn_part;
    g.x3 = c->x3; g.Whi = l0.Whi; g.Wlo = l0.Wlo; g.Wil = l0.Wil;
    RUN(ptta_launch_gemm(g, s));
    RUN(ptta_stat_sync(&c->stat_sync, c->bn_part, ptta_gemm_part_blocks(g), 512, 1, s));
    RUN(ptta_launch_bn_finalize(c->bn_part, ptta_gemm_part_blocks(g), R * (c->stat_sync.world > 1 ? c->stat_sync.world : 1), 512, bn.gamma, bn.beta, 1e-5f, 0.1f, bn.rm, bn.rv, bn.nbt,
                                bn.mean, bn.inv, bn.scale, bn.shift, s));
    GemmArgs g2; g2.A = hidden; g2.W = l3.W; g2.bias = l3.bias; g2.C = out; g2.R = R; g2.K = 512; g2.N = 512; g2.pro = 1;
    g2.pscale = bn.scale; g2.pshift = bn.shift;
    g2.x3 = c->x3; g2.Whi = l3.Whi; g2.Wlo = l3.Wlo; g2.Wil = l3.Wil;
    RUN(ptta_launch_gemm(g2, s));
    return 0;
}

int heads_forward(ptta_ctx* c, hipStream_t s, int part) {      // part (heads v2 only): 0 both passes, 1 the proxy pass, 2 the real pass
    if (part != 1) c->cos_rows_done = false;
    // profiling class 6: 3 applications of Linear(32,512) / Linear(512,512) pairs (proj on both passes, pred on the proxy pass; proj.3 and
    // pred.0 run merged) = per row 2 x (32 + 512) + 4 x (512 + 512) elements by SURVEY 8d's rule as the REFERENCE executes it (6 linears)
    // (bytes at the STORED width: the 32-wide feature rows are fp32 in both modes, the 512-wide activations and the weights bf16 in the narrow heads)
    const double esh = (c->nar_heads && heads_v2_on(c)) ? 2.0 : 4.0;
    ProfScope ps_(c, 6, s, (double)c->Rg * 2 * 32 * 4 + ((double)c->Rg * (2 * 512 + 4 * 1024) + 2 * 16384.0 + 4 * 262144.0) * esh,
                  (double)c->Rg * (2 * 16384.0 + 4 * 262144.0), heads_v2_on(c) ? 7 : 8);
    const size_t half = (size_t)c->Rg * 32 * c->es;          // feat of the proxy frames follows the real frames
    const void* feat_zero = (const char*)c->feat + half;
    if (c->nar_heads && heads_v2_on(c)) {
        // ---- mixed mode: narrow heads (heads_n.hip).  BatchNorm1d batch statistics of Linear(32,512) from the second moments of the fp32 feature
        // rows (head_moments_kernel, fp64; the proxy rows are the widened copy of the narrow features), the three 512 x 512 GEMMs on narrow
        // operands with the hidden of proj computed on the fly.  part 1: the proxy pass (emb), part 2: the real pass (ref), 0: both.
        const Lin& l0 = c->fc["proj.0"]; const Lin& lf = c->fused_pp; const Lin& lp3 = c->fc["pred.3"]; const Lin& l3 = c->fc["proj.3"];
        BNorm& b1 = c->bn["proj.1"]; BNorm& b2 = c->bn["pred.1"];
        const long R = c->Rg; const int Rw = (int)R * (c->stat_sync.world > 1 ? c->stat_sync.world : 1);
        const int nbh = 2, nb = ptta_hn_row_blocks(R);           // (the moments path hands the finalize two partial "blocks": value + rounding remainder)
        float* part_real = c->hm_part; float* part_zero = c->hm_part + (size_t)nbh * 2 * 512;
        double* msc_real = c->hn_msc; double* msc_zero = c->hn_msc + (size_t)ptta_hn_moment_scratch(R);
        HnBnOut bo1; bo1.gamma = b1.gamma; bo1.beta = b1.beta; bo1.rm = b1.rm; bo1.rv = b1.rv; bo1.nbt = b1.nbt;
        bo1.mean = b1.mean; bo1.inv = b1.inv; bo1.scale = b1.scale; bo1.shift = b1.shift;
        auto gemm_h = [&](const void* x, int x_bf16, const Lin& w, bf16_t* out, int epi) {
            HnGemmArgs g; g.pro = 3; g.epi = epi; g.X = x; g.x_bf16 = x_bf16; g.W0 = l0.Whi; g.b0 = l0.bias; g.pscale = b1.scale; g.pshift = b1.shift;
            g.W = w.Wsl; g.bias = w.bias; g.C = out; g.part = c->bn_part; g.R = R;
            return g;
        };
        if (part != 2) {
            // proxy pass first: the running statistics are updated in the reference's order (proj(feat_zero), then proj(feat), :551-554)
            const void* xz = c->nar_proxy ? (const void*)c->tw(c->feat) : (const void*)((const float*)c->feat + (size_t)R * 32);
            if (!c->stat_sync.on()) RUN(ptta_launch_hn_moments(xz, c->nar_proxy ? 1 : 0, R, 1, l0.W, l0.bias, msc_zero, nullptr, &bo1, s));
            else {
            RUN(ptta_launch_hn_moments(xz, c->nar_proxy ? 1 : 0, R, 1, l0.W, l0.bias, msc_zero, part_zero, nullptr, s));
            RUN(ptta_stat_sync(&c->stat_sync, part_zero, nbh, 512, 1, s));
            RUN(ptta_launch_bn_finalize(part_zero, nbh, Rw, 512, b1.gamma, b1.beta, 1e-5f, 0.1f, b1.rm, b1.rv, b1.nbt, b1.mean, b1.inv, b1.scale, b1.shift, s));
            }
            if (c->nar_proxy) RUN(ptta_launch_hn_gemm(gemm_h(c->tw(c->feat), 1, lf, c->h2_n, 1), s));
            else RUN(ptta_launch_hn_gemm(gemm_h((const float*)c->feat + (size_t)R * 32, 0, lf, c->h2_n, 1), s));
            RUN(ptta_stat_sync(&c->stat_sync, c->bn_part, nb, 512, 1, s));
            RUN(ptta_launch_bn_finalize(c->bn_part, nb, Rw, 512, b2.gamma, b2.beta, 1e-5f, 0.1f, b2.rm, b2.rv, b2.nbt, b2.mean, b2.inv, b2.scale, b2.shift, s));
            HnGemmArgs g3; g3.pro = 1; g3.epi = 2; g3.A = c->h2_n; g3.pscale = b2.scale; g3.pshift = b2.shift; g3.W = lp3.Wsl; g3.bias = lp3.bias; g3.C = c->emb_n; g3.R = R;
            g3.rs = c->hn_rs;                              // |e_r|^2 for the cosine term (the ref GEMM's epilogue completes it)
            RUN(ptta_launch_hn_gemm(g3, s));
        }
        if (part != 1) {
            // real pass last: its BatchNorm statistics are the ones the backward needs
            if (!c->stat_sync.on()) RUN(ptta_launch_hn_moments(c->feat, 0, R, 1, l0.W, l0.bias, msc_real, nullptr, &bo1, s));
            else {
            RUN(ptta_launch_hn_moments(c->feat, 0, R, 1, l0.W, l0.bias, msc_real, part_real, nullptr, s));
            RUN(ptta_stat_sync(&c->stat_sync, part_real, nbh, 512, 1, s));
            RUN(ptta_launch_bn_finalize(part_real, nbh, Rw, 512, b1.gamma, b1.beta, 1e-5f, 0.1f, b1.rm, b1.rv, b1.nbt, b1.mean, b1.inv, b1.scale, b1.shift, s));
            }
            HnGemmArgs gr = gemm_h(c->feat, 0, l3, c->ref_n, 5);
            gr.E = c->emb_n; gr.rs = c->hn_rs; gr.rowstats_out = c->loss_ws + ptta_loss_ws_rows_off(c->N);
            gr.cpart = c->loss_ws + ptta_loss_ws_cos_off(c->N, c->Rg); gr.cpart_n = ptta_loss_cos_blocks(c->Rg);
            RUN(ptta_launch_hn_gemm(gr, s));
            c->cos_rows_done = true;
        }
        return 0;
    }
    if (c->head_swap) {
        // stage 2 without `reverse` (network_exp_msg_chn_adapt.py:681-684): emb = pred(proj(feat)), ref = proj(feat_zero); the
        // BatchNorm state of proj's FIRST application is what its backward needs, the second one overwrites it -> saved aside
        RUN(mlp_forward(c, "proj", c->feat, c->bf16, 32, c->h1, c->pz, s));
        BNorm& bn = c->bn["proj.1"];
        const float* src[4] = {bn.mean, bn.inv, bn.scale, bn.shift}; float* dst[4] = {c->head.sv_mean, c->head.sv_inv, c->head.sv_scale, c->head.sv_shift};
        for (int k = 0; k < 4; ++k) HIPCHK(hipMemcpyAsync(dst[k], src[k], 512 * 4, hipMemcpyDeviceToDevice, s));
        RUN(mlp_forward(c, "pred", c->pz, 0, 512, c->h2, c->emb, s));
        RUN(mlp_forward(c, "proj", feat_zero, c->bf16, 32, c->h1z, c->ref, s));
        return 0;
    }
    if (heads_v2_on(c)) {
        // heads v2: emb = pred.3(relu(bn(fused_pp(relu(bn(proj.0 x_zero)))))), ref = proj.3(relu(bn(proj.0 x))) with proj.0's output never
        // materialised.  BatchNorm1d batch statistics of Linear(32,512) are analytic in the input's second moments (one fp64 pass over the
        // 26,752 x 32 features of both passes); the 512x512 GEMMs compute their A operand relu(bn(x W0^T + b0)) on the fly.
        const Lin& l0 = c->fc["proj.0"]; const Lin& lf = c->fused_pp; const Lin& lp3 = c->fc["pred.3"]; const Lin& l3 = c->fc["proj.3"];
        BNorm& b1 = c->bn["proj.1"]; BNorm& b2 = c->bn["pred.1"];
        const int R = (int)c->Rg, Rw = R * (c->stat_sync.world > 1 ? c->stat_sync.world : 1), nbm = ptta_gemm_row_blocks(R);
        float* part_real = c->hm_part; float* part_zero = c->hm_part + (size_t)nbm * 2 * 512;
        {   // BatchNorm1d batch statistics of proj.0's output: the K = 32 GEMM with its column sums and NO store -- both passes in one launch
            // over rows [0, R) = real frames, [R, 2R) = proxy frames when the 128-row blocks do not straddle the two, else one per pass
            GemmArgs g; g.A = c->feat; g.W = l0.W; g.bias = l0.bias; g.R = 2 * R; g.K = 32; g.N = 512; g.epi = 4; g.part = c->hm_part;
            g.x3 = 1; g.Whi = l0.Whi; g.Wlo = l0.Wlo; g.Wil = l0.Wil;
            if (R % 128 == 0) RUN(ptta_launch_gemm(g, s));
            else {
                g.R = R;
                RUN(ptta_launch_gemm(g, s));
                g.A = feat_zero; g.part = part_zero;
                RUN(ptta_launch_gemm(g, s));
            }
        }
        BNorm& bz = b1;
        auto gemm_h = [&](const void* x, const BNorm& bn_, const Lin& w, float* out, int epi) {
            GemmArgs g; g.X = (const float*)x; g.W0frag = c->w0frag; g.b0 = l0.bias; g.pscale = bn_.scale; g.pshift = bn_.shift; g.pro = 3;
            g.W = w.W; g.bias = w.bias; g.C = out; g.R = R; g.K = 512; g.N = 512; g.epi = epi; g.part = c->bn_part;
            g.x3 = 1; g.Whi = w.Whi; g.Wlo = w.Wlo; g.Wil = w.Wil;
            return g;
        };
        {
            // proxy pass first: the running statistics are updated in the reference's order (proj(feat_zero), then proj(feat), :551-554)
            RUN(ptta_stat_sync(&c->stat_sync, part_zero, nbm, 512, 1, s));
            RUN(ptta_launch_bn_finalize(part_zero, nbm, Rw, 512, b1.gamma, b1.beta, 1e-5f, 0.1f, b1.rm, b1.rv, b1.nbt, bz.mean, bz.inv, bz.scale, bz.shift, s));
            const GemmArgs gf = gemm_h(feat_zero, bz, lf, c->h2, 1);
            RUN(ptta_launch_gemm(gf, s));
            RUN(ptta_stat_sync(&c->stat_sync, c->bn_part, ptta_gemm_part_blocks(gf), 512, 1, s));
            RUN(ptta_launch_bn_finalize(c->bn_part, ptta_gemm_part_blocks(gf), Rw, 512, b2.gamma, b2.beta, 1e-5f, 0.1f, b2.rm, b2.rv, b2.nbt, b2.mean, b2.inv, b2.scale, b2.shift, s));
            GemmArgs g3; g3.A = c->h2; g3.W = lp3.W; g3.bias = lp3.bias; g3.C = c->emb; g3.R = R; g3.K = 512; g3.N = 512; g3.pro = 1;
            g3.pscale = b2.scale; g3.pshift = b2.shift; g3.x3 = 1; g3.Whi = lp3.Whi; g3.Wlo = lp3.Wlo; g3.Wil = lp3.Wil;
            RUN(ptta_launch_gemm(g3, s));
        }
        {
            // real pass last: its BatchNorm statistics are the ones the backward needs
            RUN(ptta_stat_sync(&c->stat_sync, part_real, nbm, 512, 1, s));
            RUN(ptta_launch_bn_finalize(part_real, nbm, Rw, 512, b1.gamma, b1.beta, 1e-5f, 0.1f, b1.rm, b1.rv, b1.nbt, b1.mean, b1.inv, b1.scale, b1.shift, s));
            RUN(ptta_launch_gemm(gemm_h(c->feat, b1, l3, c->ref, 0), s));
        }
        return 0;
    }
    if (part != 0) return c->fail("heads_forward: split passes are the narrow heads' form", -22);
    if (c->fuse_heads && c->fused_pp_valid && c->x3 && !c->bf16 && !c->skip_dec3) {      // (the stage-2 head trainer needs proj's output itself)
        // emb = pred.3(relu(bn(pred.0(proj.3(relu(bn(proj.0 x))))))) with proj.3 / pred.0 merged into one GEMM (ptta_ctx::fused_pp)
        const Lin& l0 = c->fc["proj.0"]; const Lin& lf = c->fused_pp; const Lin& l3 = c->fc["pred.3"];
        BNorm& b1 = c->bn["proj.1"]; BNorm& b2 = c->bn["pred.1"];
        const int R = (int)c->Rg, Rw = R * (c->stat_sync.world > 1 ? c->stat_sync.world : 1);
        GemmArgs g; g.A = feat_zero; g.a_bf16 = 0; g.W = l0.W; g.bias = l0.bias; g.C = c->h1z; g.R = R; g.K = 32; g.N = 512; g.epi = 1; g.part = c->bn_part;
        g.x3 = 1; g.Whi = l0.Whi; g.Wlo = l0.Wlo; g.Wil = l0.Wil;
        RUN(ptta_launch_gemm(g, s));
        RUN(ptta_stat_sync(&c->stat_sync, c->bn_part, ptta_gemm_part_blocks(g), 512, 1, s));
        RUN(ptta_launch_bn_finalize(c->bn_part, ptta_gemm_part_blocks(g), Rw, 512, b1.gamma, b1.beta, 1e-5f, 0.1f, b1.rm, b1.rv, b1.nbt, b1.mean, b1.inv, b1.scale, b1.shift, s));
        GemmArgs gf; gf.A = c->h1z; gf.W = lf.W; gf.bias = lf.bias; gf.C = c->h2; gf.R = R; gf.K = 512; gf.N = 512; gf.pro = 1; gf.epi = 1; gf.part = c->bn_part;
        gf.pscale = b1.scale; gf.pshift = b1.shift; gf.x3 = 1; gf.Whi = lf.Whi; gf.Wlo = lf.Wlo; gf.Wil = lf.Wil;
        RUN(ptta_launch_gemm(gf, s));
        RUN(ptta_stat_sync(&c->stat_sync, c->bn_part, ptta_gemm_part_blocks(gf), 512, 1, s));
        RUN(ptta_launch_bn_finalize(c->bn_part, ptta_gemm_part_blocks(gf), Rw, 512, b2.gamma, b2.beta, 1e-5f, 0.1f, b2.rm, b2.rv, b2.nbt, b2.mean, b2.inv, b2.scale, b2.shift, s));
        GemmArgs g3; g3.A = c->h2; g3.W = l3.W; g3.bias = l3.bias; g3.C = c->emb; g3.R = R; g3.K = 512; g3.N = 512; g3.pro = 1;
        g3.pscale = b2.scale; g3.pshift = b2.shift; g3.x3 = 1; g3.Whi = l3.Whi; g3.Wlo = l3.Wlo; g3.Wil = l3.Wil;
        RUN(ptta_launch_gemm(g3, s));
    } else {
        RUN(mlp_forward(c, "proj", feat_zero, c->bf16, 32, c->h1z, c->pz, s));
        RUN(mlp_forward(c, "pred", c->pz, 0, 512, c->h2, c->emb, s));
    }
    RUN(mlp_forward(c, "proj", c->feat, c->bf16, 32, c->h1, c->ref, s));     // last: its BN statistics are kept for backward
    return 0;
}

// d ref -> d feat through proj = Linear(32,512) - BN1d - ReLU - Linear(512,512)
int heads_backward(ptta_ctx* c, const float* gref, hipStream_t s) {
    const double esh = (c->nar_heads && heads_v2_on(c)) ? 2.0 : 4.0;       // (stored widths, as heads_forward)
    ProfScope ps_(c, 6, s, (double)c->Rg * 32 * (c->nar_bwd ? 2 : 4) + ((double)c->Rg * (1024 + 512) + 16384.0 + 262144.0) * esh,
                  (double)c->Rg * (16384.0 + 262144.0), 3);   // data gradient through proj once
    const Lin& l0 = c->fc["proj.0"]; const Lin& l3 = c->fc["proj.3"]; BNorm& bn = c->bn["proj.1"];
    const int R = (int)c->Rg;
    if (c->nar_heads && heads_v2_on(c)) {
        // mixed mode (heads_n.hip): one block holds full rows, so the contraction with W0 is complete per block (one P half)
        HnGemmArgs g; g.epi = 3; g.R = R; g.W = l3.Wtsl;
        if (c->cos_in_gemm) { g.pro = 4; g.A = c->emb_n; g.Bref = c->ref_n; g.rowstats = c->loss_ws + ptta_loss_ws_rows_off(c->N); g.coef = c->loss_ws; }
        else { g.pro = 5; g.Af = gref; }
        g.X = c->feat; g.x_bf16 = 0; g.W0 = l0.Whi; g.W0t = l0.Wthi; g.b0 = l0.bias;
        g.escale = bn.scale; g.eshift = bn.shift; g.emean = bn.mean; g.einv = bn.inv; g.part = c->bn_part; g.P = c->headP;
        RUN(ptta_launch_hn_gemm(g, s));
        const int nb = ptta_hn_row_blocks(R);
        RUN(ptta_stat_sync(&c->stat_sync, c->bn_part, nb, 512, 1, s));
        RUN(ptta_launch_bn_bwd_finalize(c->bn_part, nb, R * (c->stat_sync.world > 1 ? c->stat_sync.world : 1), 512, bn.gamma, bn.inv, c->bnb_gscale, c->bnb_c1, c->bnb_c2, s,
                                        nullptr, nullptr, c->head_k12, l0.bias, bn.mean));
        RUN(ptta_launch_head_bwd_finish(c->head_k12, l0.W, c->headP, (const float*)c->feat, R, c->g_feat, s, 1, c->nar_bwd ? 1 : 0));
        return 0;
    }
    if (heads_v2_on(c)) {
        // d ref -> d feat without the stored hidden: the GEMM recomputes h = x W0^T + b0 for the ReLU mask and the BatchNorm-backward sums and
        // contracts the masked gradient (x gamma x invstd) with W0 inside the block (P: [column block 2][R][32]); the BatchNorm-backward
        // correction terms are linear in x: d x = P[0] + P[1] - x M - u (heads.hip head_bwd_mat_kernel)
        GemmArgs g; g.A = gref; g.W = l3.Wt; g.R = R; g.K = 512; g.N = 512; g.epi = 3;
        if (c->cos_in_gemm) {       // fused step: the gradient of the cosine term is formed while the GEMM stages its A operand (no [R][512] tensor)
            g.A = c->emb; g.Bref = c->ref; g.rowstats = c->loss_ws + ptta_loss_ws_rows_off(c->N); g.coef = c->loss_ws; g.pro = 4;
        }
        g.escale = bn.scale; g.eshift = bn.shift; g.emean = bn.mean; g.einv = bn.inv; g.part = c->bn_part;
        g.x3 = 1; g.Whi = l3.Wthi; g.Wlo = l3.Wtlo; g.Wil = l3.Wtil;
        g.X = (const float*)c->feat; g.b0 = l0.bias; g.W0hi = l0.Whi; g.W0lo = l0.Wlo; g.W0thi = l0.Wthi; g.W0tlo = l0.Wtlo; g.P = c->headP;
        RUN(ptta_launch_gemm(g, s));
        RUN(ptta_stat_sync(&c->stat_sync, c->bn_part, ptta_gemm_part_blocks(g), 512, 1, s));
        RUN(ptta_launch_bn_bwd_finalize(c->bn_part, ptta_gemm_part_blocks(g), R * (c->stat_sync.world > 1 ? c->stat_sync.world : 1), 512, bn.gamma, bn.inv, c->bnb_gscale, c->bnb_c1, c->bnb_c2, s,
                                        nullptr, nullptr, c->head_k12, l0.bias, bn.mean));
        RUN(ptta_launch_head_bwd_finish(c->head_k12, l0.W, c->headP, (const float*)c->feat, R, c->nar_bwd ? c->g_feat_f32 : (float*)c->g_feat, s));
        if (c->nar_bwd) RUN(to_narrow(c, c->g_feat_f32, c->g_feat, c->Rg * 32, s));          // the backward's gradient maps are narrow
        return 0;
    }
    GemmArgs g; g.A = gref; g.W = l3.Wt; g.C = c->gmask; g.R = R; g.K = 512; g.N = 512; g.epi = 2;
    g.eH = c->h1; g.escale = bn.scale; g.eshift = bn.shift; g.emean = bn.mean; g.einv = bn.inv; g.part = c->bn_part;
    g.x3 = c->x3; g.Whi = l3.Wthi; g.Wlo = l3.Wtlo; g.Wil = l3.Wtil;
    RUN(ptta_launch_gemm(g, s));
    RUN(ptta_stat_sync(&c->stat_sync, c->bn_part, ptta_gemm_part_blocks(g), 512, 1, s));
    RUN(ptta_launch_bn_bwd_finalize(c->bn_part, ptta_gemm_part_blocks(g), R * (c->stat_sync.world > 1 ? c->stat_sync.world : 1), 512, bn.gamma, bn.inv, c->bnb_gscale, c->bnb_c1, c->bnb_c2, s));
    GemmArgs g2; g2.A = c->gmask; g2.A2 = c->h1; g2.W = l0.Wt; g2.C = (c->bf16 || c->nar_bwd) ? c->g_feat_f32 : (float*)c->g_feat; g2.R = R; g2.K = 512; g2.N = 32; g2.pro = 2;   // fp32 storage: straight into the gradient map (no copy launch)
    g2.pscale = c->bnb_gscale; g2.pmean = bn.mean; g2.pinv = bn.inv; g2.pc1 = c->bnb_c1; g2.pc2 = c->bnb_c2;
    g2.x3 = c->x3; g2.Whi = l0.Wthi; g2.Wlo = l0.Wtlo;
    RUN(ptta_launch_gemm(g2, s));
    if (c->bf16 || c->nar_bwd) hipLaunchKernelGGL((from_f32_kernel<bf16_t>), dim3(nblk(c->Rg * 32)), dim3(256), 0, s, c->g_feat_f32, (bf16_t*)c->g_feat, c->Rg * 32);
    return 0;
}

const float* final_depth(ptta_ctx* c);
// data gradients from d(depth_net) [Nn,1,Hp,Wp] and d(feat) down to conv1_rgb_meta, then its wgrad
int backbone_backward(ptta_ctx* c, const float* g_net, hipStream_t s, bool join_aux) {
    const int Nn = c->Nn, B2 = 2 * Nn;
    const int nbf = c->nar_bwd ? 1 : c->bf16;            // gradient maps: narrow in the mixed mode (conv32() routes every bwd launch there itself)
    const int H1 = c->Hp, W1 = c->Wp, H2 = c->H2, W2 = c->W2, H4 = c->H4, W4 = c->W4, H8 = c->H8, W8 = c->W8;
#define CV(...) RUN(conv32(c, s, __VA_ARGS__))
    auto out1_args = [&](const std::string& layer, const float* g, const void* mask, void* out, int H, int W) {
        const LOut& lo = c->lout[layer];
        ConvInArgs a; a.cin = 1; a.pl[0].p = g; a.pl[0].nb = Nn; a.pl[0].bstride = (long)H * W;
        a.wfrag = lo.bfrag; a.wcanon = lo.bcanon; a.mask = mask; a.mask_nb = B2; a.out_raw = out;
        a.B = Nn; a.H = H; a.W = W; a.bf16 = c->nar_bwd ? 1 : c->bf16; a.naive = c->naive;
        return a;
    };
    auto dgrad_out1 = [&](const std::string& layer, const float* g, const void* mask, void* out, int H, int W) -> int {
        ConvInArgs a = out1_args(layer, g, mask, out, H, W);
        return conv_in_p(c, a, s);
    };
    // prediction head backward: prdct.3^T then prdct.1's data gradient, one launch on large maps
    auto head_bwd = [&](const std::string& l3, const std::string& l1, const float* g, const void* v, void* dv, int H, int W, const E& e) -> int {
        ConvInArgs a = out1_args(l3, g, v, dv, H, W);
        return conv32_first_bwd(c, s, l1, a, Nn, H, W, e);
    };
    auto dgrad_in_ch1 = [&](const std::string& layer, const void* g, const float* add, float* out, int H, int W) -> int {
        const LIn& li = c->lin_in[layer];
        ConvOut1Args a; a.in = g; a.in_nb = Nn; a.w = li.bw; a.add = add; a.add_nb = Nn; a.out = out;
        a.B = Nn; a.H = H; a.W = W; a.relu_in = 0; a.bf16 = c->nar_bwd ? 1 : c->bf16;
        return conv_out1_p(c, a, s);
    };
    auto em = [](void* raw, const void* mask, int mask_nb) { E e; e.raw = raw; e.mask = mask; e.mask_nb = mask_nb; return e; };
    // ---- decoder 3 ----
    RUN(head_bwd("depth_decoder3.prdct.3", "depth_decoder3.prdct.1", g_net, c->v3, c->dv3, H1, W1, em(c->ds0_3, c->s0_3, Nn)));
    CV("depth_decoder3.dec1.3", true, CONV_S1, c->ds0_3, Nn, Nn, H1, W1, false, em(c->du3, c->u3, Nn));
    CV("depth_decoder3.dec1.1", true, CONV_S2, c->du3, Nn, Nn, H1, W1, false, em(c->ds1_3, c->s1_3, Nn));
    CV("depth_decoder3.dec2.3", true, CONV_S1, c->ds1_3, Nn, Nn, H2, W2, false, em(c->dt3, c->t3, Nn));
    if (join_aux) HIPCHK(hipStreamWaitEvent(s, c->ev_join, 0));       // d feat from the heads (auxiliary stream)
    { E e; e.raw = c->dw2; e.mask = c->w2; e.mask_nb = B2; e.sum = c->dfeat_tot; e.add1 = c->g_feat; e.add1_nb = Nn;
      CV("depth_decoder3.dec2.1", true, CONV_S2, c->dt3, Nn, Nn, H2, W2, false, e); }
    // The three transposed bilinear upsamplings of the backward (d z2 += up2^T(d feat_tot), d z3 = d s1_2 + up2^T(d e3_1), d z4 = d s0_2 + up2^T(d e3_0))
    // do not lie on the chain d feat_tot -> encoder 3 -> decoder 2: they run on the second stream, and each
    // result enters the chain as the addend of a convolution epilogue (out_sum = masked result + addend; fp32: the same two operands of the
    // same addition as `add + up2^T(...)` in the upsampling kernel).  One join, in front of decoder 2's prediction head.
    hipStream_t sd = join_aux ? c->aux(s) : nullptr;
    if (!sd) sd = s;
    // ---- encoder 3 ----
    CV("depth_encoder3.enc2.3", true, CONV_S1, c->dfeat_tot, Nn, Nn, H4, W4, false, em(c->de3_2a, c->e3_2a, B2));
    { E e; e.sum = c->de3_1; e.mask = c->e3_1; e.mask_nb = B2; e.add1 = c->ds1_3; e.add1_nb = Nn;
      CV("depth_encoder3.enc2.1", true, CONV_T2, c->de3_2a, Nn, Nn, H4, W4, false, e); }
    CV("depth_encoder3.enc1.3", true, CONV_S1, c->de3_1, Nn, Nn, H2, W2, false, em(c->de3_1a, c->e3_1a, B2));
    { E e; e.sum = c->de3_0; e.mask = c->e3_0; e.mask_nb = B2; e.add1 = c->ds0_3; e.add1_nb = Nn;
      CV("depth_encoder3.enc1.1", true, CONV_T2, c->de3_1a, Nn, Nn, H2, W2, false, e); }
    // all three sources exist: ONE fork (every event on the main stream is a packet in front of its next kernel), the three launches run
    // beside the next three of the chain
    if (sd != s) { HIPCHK(hipEventRecord(c->ev_side[0], s)); HIPCHK(hipStreamWaitEvent(sd, c->ev_side[0], 0)); }
    REST_(sd, ptta_launch_up2T_32(c->de3_0, nullptr, c->up4_t, Nn, H2, W2, nbf, sd));
    REST_(sd, ptta_launch_up2T_32(c->de3_1, nullptr, c->up3_t, Nn, H4, W4, nbf, sd));
    REST_(sd, ptta_launch_up2T_32(c->dfeat_tot, nullptr, c->dz2_up, Nn, H8, W8, nbf, sd));
    if (sd != s) HIPCHK(hipEventRecord(c->ev_side[3], sd));
    if (c->loss_report.on) {             // (sd == s: the profiling leg)
        // the loss VALUES (thru step): depth terms reduced here, behind the upsamplings the main chain waits for, then the one-block finalisation
        // that writes the four reported scalars; main joins in front of the weight gradient (ev_loss)
        REST_(sd, ptta_launch_loss_depth_part(final_depth(c), c->loss_report.image, c->loss_report.sparse, c->loss_report.validity, c->hp.max_input_depth,
                                              c->N, c->H, c->W, c->loss_ws, sd));
        REST_(sd, ptta_launch_loss_finalize(c->loss_ws, c->N, c->H, c->W, c->Rg, 1, c->hyper + 5, c->loss_info_dst ? c->loss_info_dst : c->loss_info, sd));
        HIPCHK(hipEventRecord(c->ev_loss, sd));
    }
    CV("depth_encoder3.init.2", true, CONV_S1, c->de3_0, Nn, Nn, H1, W1, false, em(c->de3_0a, c->e3_0a, B2));
    RUN(dgrad_in_ch1("depth_encoder3.init.0", c->de3_0a, g_net, c->dp11, H1, W1));       // d p11 = conv^T + d output
    REST_(s, ptta_launch_up2T_1ch(c->dp11, c->dq, Nn, H2, W2, s));                              // d(out2 + p12)
    // ---- decoder 2 ----
    if (sd != s) HIPCHK(hipStreamWaitEvent(s, c->ev_side[3], 0));
    { E e = em(c->ds0_2, c->s0_2, B2); e.sum = c->dz4; e.add1 = c->up4_t; e.add1_nb = Nn;      // d z4 = d s0_2 + up2^T(d e3_0)
      RUN(head_bwd("depth_decoder2.prdct.3", "depth_decoder2.prdct.1", c->dq, c->v2, c->dv2, H2, W2, e)); }
    CV("depth_decoder2.dec1.3", true, CONV_S1, c->dz4, Nn, Nn, H2, W2, false, em(c->du2, c->u2, B2));
    { E e = em(c->ds1_2, c->s1_2, B2); e.sum = c->dz3; e.add1 = c->up3_t; e.add1_nb = Nn;      // d z3 = d s1_2 + up2^T(d e3_1)
      CV("depth_decoder2.dec1.1", true, CONV_S2, c->du2, Nn, Nn, H2, W2, false, e); }
    CV("depth_decoder2.dec2.3", true, CONV_S1, c->dz3, Nn, Nn, H4, W4, false, em(c->dt2, c->t2, B2));
    { E e; e.sum = c->dz2; e.mask = c->z2; e.mask_nb = B2; e.add1 = c->dz2_up; e.add1_nb = Nn;
      CV("depth_decoder2.dec2.1", true, CONV_S2, c->dt2, Nn, Nn, H4, W4, false, e); }
    // ---- encoder 2 ----
    CV("depth_encoder2.enc2.3", true, CONV_S1, c->dz2, Nn, Nn, H8, W8, false, em(c->de2_2a, c->e2_2a, B2));
    { E e; e.sum = c->de2_1; e.mask = c->e2_1; e.mask_nb = B2; e.add1 = c->ds1_2; e.add1_nb = Nn;
      CV("depth_encoder2.enc2.1", true, CONV_T2, c->de2_2a, Nn, Nn, H8, W8, false, e); }
    CV("depth_encoder2.enc1.3", true, CONV_S1, c->de2_1, Nn, Nn, H4, W4, false, em(c->de2_1a, c->e2_1a, B2));
    { E e; e.sum = c->de2_0; e.mask = c->e2_0; e.mask_nb = B2; e.add1 = c->ds0_2; e.add1_nb = Nn;
      CV("depth_encoder2.enc1.1", true, CONV_T2, c->de2_1a, Nn, Nn, H4, W4, false, e); }
    CV("depth_encoder2.init.2", true, CONV_S1, c->de2_0, Nn, Nn, H2, W2, false, em(c->de2_0a, c->e2_0a, B2));
    RUN(dgrad_in_ch1("depth_encoder2.init.0", c->de2_0a, c->dq, c->dp12, H2, W2));       // d p12 = conv^T + d q
    REST_(s, ptta_launch_up2T_1ch(c->dp12, c->dout1, Nn, H4, W4, s));
    // ---- decoder 1: only the prediction head reaches the meta layer (y0 = e1_0 + m) ----
    RUN(dgrad_out1("depth_decoder1.prdct.3", c->dout1, c->v1, c->dv1, H4, W4));
    { E e; e.sum = c->dm_total; e.mask = c->s0_1; e.mask_nb = B2; e.add1 = c->dw2; e.add1_nb = Nn; e.add2 = c->ds1_2; e.add2_nb = Nn;
      CV("depth_decoder1.prdct.1", true, CONV_S1, c->dv1, Nn, Nn, H4, W4, false, e); }
#undef CV
    if (sd != s && c->loss_report.on) HIPCHK(hipStreamWaitEvent(s, c->ev_loss, 0));       // (signalled ~200 us ago: the caller's loss_info is ordered on `s`)
    // ---- weight gradient of the meta layer: input = c2 of the real frames ----
    // (mixed mode, 2layers meta block: its BatchNorm / weight-gradient kernels take fp32 operands -- the 1/4-resolution gradient map is widened
    // once, 3.4 MB; the 1layer weight gradient reads the narrow map itself)
    if (c->nar_bwd && c->meta_mode == PTTA_META_2LAYERS) RUN(to_wide(c, c->dm_total, c->dm_f32, (long)Nn * H4 * W4 * 32, s));
    if (c->meta_mode == PTTA_META_2LAYERS) return meta2_backward(c, s);
    if (!c->bf16 && c->x3 && !c->naive) {
        // default arithmetic: the bf16x3 reduction-GEMM form (gconv_mfma.hip gwgrad_x3_kernel, single-pair mode)
        GView xv; xv.p = (float*)c->c2; xv.B = Nn; xv.H = H4; xv.W = W4; xv.C = 32; xv.ld = 32;
        GView gv; gv.p = (float*)c->dm_total; gv.B = Nn; gv.H = H4; gv.W = W4; gv.C = 32; gv.ld = 32;
        GwAdam ga;
        const bool fuse = c->adam_fuse_req && c->adam_in_wgrad && !c->grad_comm && c->adapted.size() == 2 && c->adapted[0].p && c->adapted[0].m && c->adapted[0].v &&
                          c->adapted[1].p && c->adapted[1].m && c->adapted[1].v && c->adapted[0].g == c->gW && c->adapted[1].g == c->gB;
        if (fuse) { ga.pw = c->adapted[0].p; ga.mw = c->adapted[0].m; ga.vw = c->adapted[0].v; ga.pb = c->adapted[1].p; ga.mb = c->adapted[1].m; ga.vb = c->adapted[1].v;
                    ga.hyper = c->hyper; ga.step = c->step_dev; ga.ticket = c->adam_ticket; }
        REST_(s, ptta_launch_gwgrad_mfma(xv, gv, c->wgrad_part, c->gW, c->gB, s, c->nar_bwd ? 1 : 0, fuse ? &ga : nullptr));
        c->adam_fused = fuse;
        return 0;
    }
    REST_(s, ptta_launch_wgrad32(c->c2, c->dm_total, c->bf16, Nn, H4, W4, c->wgrad_part, c->gW, c->gB, s));
    return 0;
}

int push_hparams(ptta_ctx* c, hipStream_t s) {
    const float h[8] = {c->hp.lr, c->hp.beta1, c->hp.beta2, c->hp.eps, c->hp.weight_decay,
                        c->hp.w_sparse_depth, c->hp.w_smoothness, c->hp.w_cos};
    RUN(ptta_launch_set_floats(c->hyper, h, 8, s));      // by kernel argument: no host sync
    return 0;
}

int forward_common(ptta_ctx* c, const float* image, const float* sparse, bool train, hipStream_t s) {
    for (auto& ad : c->adapted) if (!ad.p) return c->fail("adapted parameter " + ad.name + " not bound (ptta_bind_adapted)", -3);
    const float* img = image; const float* sp = sparse;
    if (c->dual) {
        hipLaunchKernelGGL(pad_dual_kernel, dim3(nblk((long)c->Nn * 3 * c->Hp * c->Wp)), dim3(256), 0, s, image, c->img_pad, c->N, 3, c->H, c->W, c->Hp, c->Wp, c->pt, c->pr, c->img_norm);
        hipLaunchKernelGGL(pad_dual_kernel, dim3(nblk((long)c->Nn * c->Hp * c->Wp)), dim3(256), 0, s, sparse, c->sp_pad, c->N, 1, c->H, c->W, c->Hp, c->Wp, c->pt, c->pr);
        img = c->img_pad; sp = c->sp_pad;
    }
    if (!c->skip_prefix) {                     // (ptta_step_pipelined ran this part ahead, beside the previous frame's step)
        if (train) RUN(ensure_proxy_rgb(c, img, s));
        REST_(s, ptta_launch_prep(sp, c->hp.max_input_depth, c->dclamp, c->d12, c->d14, c->Nn, c->Hp, c->Wp, s));
    }
    if (c->meta_mode == PTTA_META_2LAYERS && c->m2.generic) {
        auto& m2 = c->m2;
        const float* W1 = c->adapted[0].p; const float* W2 = c->adapted[3].p;       // (128,32,3,3), (32,128,3,3)
        ptta_gpack(W1, m2.w1c, 9, 32, 128, 9, 32L * 9, 0, s);                        // forward  P[t][ci][co]
        ptta_gfrag_pack(m2.w1c, 128, 32L * 128, 9, 32, 0, 0, 0, 128, m2.w1hi, m2.w1lo, s);
        ptta_gpack(W2, m2.w2c, 9, 128, 32, 9, 128L * 9, 0, s);
        ptta_gfrag_pack(m2.w2c, 32, 128L * 32, 9, 128, 0, 0, 0, 32, m2.w2hi, m2.w2lo, s);
        ptta_gpack(W2, m2.w2bc, 9, 32, 128, 128L * 9, 9, 1, s);                      // data gradient  P[t][co][ci] = W2[co][ci][8-t]
        ptta_gfrag_pack(m2.w2bc, 128, 32L * 128, 9, 32, 0, 0, 0, 128, m2.w2bhi, m2.w2blo, s);
    } else if (c->meta_mode == PTTA_META_2LAYERS) {
        for (int g = 0; g < 4; ++g) {
            ptta_pack_conv32(c->adapted[0].p + (size_t)g * 9216, c->m2.w1f[g], 0, 0, s);            // W1 rows 32g..32g+31
            ptta_pack_conv32(c->adapted[3].p, c->m2.w2f[g], 0, 0, s, 128, 32 * g);                 // W2 columns 32g..
            ptta_pack_conv32(c->adapted[3].p, c->m2.w2b[g], 1, 1, s, 128, 32 * g);                 // its input gradient
        }
    } else {
        c->stamp(0, s);
        const L32& ml = c->l32["conv1_rgb_meta"];
        { ProfScope ps_(c, 8, s, 0, 0, 1); ptta_pack_conv32(c->meta_w, ml.f, 0, 0, s); }
    }
    RUN(backbone(c, img, train, s));
    if (c->dual)
        hipLaunchKernelGGL(crop_avg_kernel, dim3(nblk((long)c->N * c->H * c->W)), dim3(256), 0, s, c->depth_net, c->depth_final, c->N, c->H, c->W, c->Hp, c->Wp, c->pt, c->pr);
    return 0;
}

const float* final_depth(ptta_ctx* c) { return c->dual ? c->depth_final : c->depth_net; }

}  // namespace

extern "C" {

int ptta_version(void) { return PTTA_ABI_VERSION; }

const char* ptta_last_error(ptta_handle h) { return h ? (h->nl && h->err.empty() ? h->nl->err.c_str() : h->err.c_str()) : "null handle"; }
// calls forwarded to a GNet engine clear the wrapper-level message, so the engine's later message is not masked by a stale one
#define NLFWD(call) do { if (c && c->nl) { c->err.clear(); return (call); } } while (0)

int ptta_create(ptta_handle* out, int backbone_id, int meta_mode, int n, int height, int width, int dtype, const ptta_hparams* hp) {
    if (!out) return -1;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return -19;          // no HIP device: fail loudly
    // generic engine (NLSPN, CostDCNet): PTTA_DTYPE_MIXED = fp32 storage, single-MFMA products for the proxy frames and the data gradients
    // (PTTA_MIXED_KEEP_PROXY / _BACKWARD keep a class at bf16x3); the heads of those backbones are 0.4 % of their step and stay bf16x3
    // (round 6: the data gradients keep their WEIGHTS as hi + lo -- two MFMAs, GX3Args::x1_w2; PTTA_MIXED_BWD_ROUNDED_W = round 5's one-MFMA form,
    // whose rounded weights tilt the gradient systematically: NLSPN's scored depth drifted 6e-5 per step with it)
    const int gmix = (dtype & 0xff) == PTTA_DTYPE_MIXED ? ((((dtype >> 8) & 1) ? 0 : 1) | (((dtype >> 8) & 2) ? 0 : (((dtype >> 8) & 8) ? 2 : 4))) : 0;
    if (backbone_id != PTTA_BACKBONE_MSG_CHN && (dtype & 0xff) == PTTA_DTYPE_MIXED) dtype = PTTA_DTYPE_F32;
    if (backbone_id == PTTA_BACKBONE_NLSPN) {
        // 2layers: the Res_Conv(48, 256) block (nlspn_api.hip), fp32 and mixed; not with the adapted set of the DDP run (its repeat structure differs)
        const int meta = meta_mode & ~(PTTA_NLSPN_LEGACY_OFFSET | PTTA_NLSPN_SYNCBN_ADAPT);
        if ((meta != PTTA_META_1LAYER && meta != PTTA_META_2LAYERS) || dtype != PTTA_DTYPE_F32) return -38;
        if (meta == PTTA_META_2LAYERS && (meta_mode & PTTA_NLSPN_SYNCBN_ADAPT)) return -38;
        int rc = 0;
        GNet* e = nlspn_create(n, height, width, hp, ((meta_mode & PTTA_NLSPN_LEGACY_OFFSET) ? 1 : 0) | ((meta_mode & PTTA_NLSPN_SYNCBN_ADAPT) ? 2 : 0) |
                               (meta == PTTA_META_2LAYERS ? 4 : 0), &rc);
        if (!e) return rc ? rc : -12;
        e->mixed = e->naive ? 0 : gmix;
        ptta_ctx* c = new ptta_ctx();
        c->nl = e; c->N = n; c->H = height; c->W = width; c->hp = *hp;
        *out = c;
        return 0;
    }
    if (backbone_id == PTTA_BACKBONE_COSTDCNET) {
        // (no mixed mode for CostDCNet: with single-MFMA data gradients its scored depth leaves the tolerance -- 2.0e-3 / 1.7e-3 at 480x640 /
        // 320x400, with hi + lo weights in them still 1.1e-3 / 1.2e-3, with single-MFMA proxy frames alone 8.9e-4 at 320x400, for 2 - 3 % of
        // the step: profiles/r06_nlspn_costdcnet_mixed.txt -- its argmax over the cost volume amplifies any change of the update)
        // 2layers: the Res_Conv(16, 64) block (costdc_api.hip), fp32 only, not with PTTA_SYNCBN_ADAPT
        const int meta = meta_mode & ~PTTA_SYNCBN_ADAPT;
        if ((meta != PTTA_META_1LAYER && meta != PTTA_META_2LAYERS) || dtype != PTTA_DTYPE_F32 || !hp || gmix) return -38;
        if (meta == PTTA_META_2LAYERS && (meta_mode & PTTA_SYNCBN_ADAPT)) return -38;
        int rc = 0;
        GNet* e = costdc_create(n, height, width, hp, hp->max_predict_depth, ((meta_mode & PTTA_SYNCBN_ADAPT) ? 1 : 0) | (meta == PTTA_META_2LAYERS ? 2 : 0), &rc);
        if (!e) return rc ? rc : -12;
        e->mixed = e->naive ? 0 : gmix;
        ptta_ctx* c = new ptta_ctx();
        c->nl = e; c->N = n; c->H = height; c->W = width; c->hp = *hp;
        *out = c;
        return 0;
    }
    if (backbone_id != PTTA_BACKBONE_MSG_CHN || (meta_mode != PTTA_META_1LAYER && meta_mode != PTTA_META_2LAYERS)) return -38;
    const int keep = (dtype >> 8) & 7;                 // PTTA_MIXED_KEEP_*: classes kept at fp32 / bf16x3 (precision budget)
    dtype &= 0xff;
    if (n < 1 || height < 16 || width < 16 || (dtype != PTTA_DTYPE_F32 && dtype != PTTA_DTYPE_MIXED) || !hp) return -22;
    ptta_ctx* c = new ptta_ctx();
    c->meta_mode = meta_mode;
    c->N = n; c->H = height; c->W = width; c->pt = pad16(height); c->pr = pad16(width);
    c->Hp = height + c->pt; c->Wp = width + c->pr; c->dual = (c->pt || c->pr) ? 1 : 0; c->Nn = c->dual ? 2 * n : n;
    c->mixed = dtype == PTTA_DTYPE_MIXED ? 1 : 0;
    c->nar_proxy = c->mixed && !(keep & 1); c->nar_bwd = c->mixed && !(keep & 2); c->nar_heads = c->mixed && !(keep & 4);
    const PttaCreateEnv env = ptta_create_env();         // (the three validation switches; everything else: ptta_set_option)
    c->naive = env.naive;
    c->use_graph = env.graph == 1 ? 1 : 0;
    c->x3 = env.exact ? 0 : 1;
    if (c->mixed) {
        // the mixed mode is defined on the matrix-core kernels with sign-bit masks; the validation arithmetic modes belong to PTTA_DTYPE_F32
        if (c->naive || !c->x3) { delete c; return -38; }
    }
    c->hp = *hp;
    build_registry(c);
    build_workspace(c);
    if (c->oom || !c->step_dev) { ptta_destroy(c); return -12; }
    const float h8[8] = {hp->lr, hp->beta1, hp->beta2, hp->eps, hp->weight_decay, hp->w_sparse_depth, hp->w_smoothness, hp->w_cos};
    if (hipMemcpy(c->hyper, h8, sizeof(h8), hipMemcpyHostToDevice) != hipSuccess) { ptta_destroy(c); return -5; }
    *out = c;
    return 0;
}

void ptta_destroy(ptta_handle h) {
    if (!h) return;
    if (h->nl) { delete h->nl; delete h; return; }
    h->drop_graphs();
    if (h->ev_replay) (void)hipEventDestroy(h->ev_replay);
    if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
    if (h->pre_stream) {
        (void)hipStreamDestroy(h->pre_stream); (void)hipEventDestroy(h->ev_entry);
        for (int p = 0; p < 2; ++p) { (void)hipEventDestroy(h->ev_prefix[p]); (void)hipEventDestroy(h->ev_rest[p]); }
    }
    if (h->ev_dpart) (void)hipEventDestroy(h->ev_dpart);
    if (h->ev_loss) (void)hipEventDestroy(h->ev_loss);
    if (h->aux_stream) { (void)hipStreamDestroy(h->aux_stream); (void)hipEventDestroy(h->ev_fork); (void)hipEventDestroy(h->ev_join); (void)hipEventDestroy(h->ev_real); for (auto& e_ : h->ev_side) if (e_) (void)hipEventDestroy(e_); }
    for (void* p : h->allocs) if (p) (void)hipFree(p);
    for (auto& pc : h->prof) for (auto& e : pc.ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    delete h;
}

int ptta_set_hparams(ptta_handle c, const ptta_hparams* hp, ptta_stream s) {
    NLFWD(c->nl->set_hparams(hp, (hipStream_t)s));

    if (!c || !hp) return -1;
    if (hp->max_input_depth != c->hp.max_input_depth) c->drop_graphs();     // baked into kernel arguments
    c->hp = *hp;
    return push_hparams(c, (hipStream_t)s);
}

static long shape_numel(const int64_t* shape, int ndim) { long n = 1; for (int i = 0; i < ndim; ++i) n *= shape[i]; return n; }

int ptta_load_weights(ptta_handle c, const char* name_, const void* tensor, const int64_t* shape, int ndim, ptta_stream s_) {
    NLFWD((name_ && tensor) ? c->nl->load(name_, tensor, shape, ndim, (hipStream_t)s_) : -1);

    if (!c || !name_ || !tensor) return -1;
    c->drop_graphs();
    RUN(pipe_quiesce(c));
    c->proxy_rgb_valid = false; c->fused_pp_valid = false; c->pset[0].proxy_valid = false; c->pset[1].proxy_valid = false;
    hipStream_t s = (hipStream_t)s_;
    const std::string name(name_);
    const long numel = shape_numel(shape, ndim);
    auto ends = [&](const char* suf) { const size_t n = strlen(suf); return name.size() >= n && name.compare(name.size() - n, n, suf) == 0; };
    if (name.rfind("proj_t.", 0) == 0) return 0;                     // EMA target head: unused in stage 3 (:551-554)
    if (name.rfind("conv1_rgb_meta", 0) == 0) {
        auto ends2 = [&](const char* suf) { const size_t n = strlen(suf); return name.size() >= n && name.compare(name.size() - n, n, suf) == 0; };
        if (c->meta_mode == PTTA_META_2LAYERS) {           // BatchNorm2d buffers of Res_Conv: bound, updated in place
            const bool first = name.find("conv1_meta.0.1.") != std::string::npos, second = name.find("conv1_meta.2.") != std::string::npos;
            if ((first || second) && ends2(".running_mean")) { (first ? c->m2.rm1 : c->m2.rm2) = (float*)tensor; return 0; }
            if ((first || second) && ends2(".running_var")) { (first ? c->m2.rv1 : c->m2.rv2) = (float*)tensor; return 0; }
            if ((first || second) && ends2(".num_batches_tracked")) { (first ? c->m2.nbt1 : c->m2.nbt2) = (long long*)tensor; return 0; }
        }
        return c->fail("adapted parameter " + name + " must be bound with ptta_bind_adapted", -4);
    }
    const std::string base = name.substr(0, name.rfind('.'));
    const bool is_w = ends(".weight"), is_b = ends(".bias");
    const float* src = (const float*)tensor;
    if (c->l32.count(base)) {
        L32& l = c->l32[base];
        if (is_w) {
            if (numel != 9216) return c->fail("bad shape for " + name, -22);
            if (!l.transposed) {          // Conv2d weight [out][in][3][3]
                ptta_pack_conv32(src, l.f, 0, 0, s);
                // backward: stride-1 conv -> stride-1 conv (transposed + flipped); stride-2 conv -> transposed conv
                const bool s2 = base.find("enc1.1") != std::string::npos || base.find("enc2.1") != std::string::npos ||
                                base.find("enc3.1") != std::string::npos || base.find("enc4.1") != std::string::npos;
                if (l.b.mf32) ptta_pack_conv32(src, l.b, 1, s2 ? 0 : 1, s);
            } else {                      // ConvTranspose2d weight [in][out][3][3]
                ptta_pack_conv32(src, l.f, 1, 0, s);
                if (l.b.mf32) ptta_pack_conv32(src, l.b, 0, 0, s);   // backward = stride-2 conv
            }
        } else if (is_b) {
            if (numel != 32) return c->fail("bad shape for " + name, -22);
            HIPCHK(hipMemcpyAsync(l.bias, src, 32 * 4, hipMemcpyDeviceToDevice, s));
        } else return c->fail("unknown key " + name, -2);
        return 0;
    }
    if (c->lin_in.count(base)) {
        LIn& l = c->lin_in[base];
        if (is_w) {
            if (numel != 32L * l.cin * 9) return c->fail("bad shape for " + name, -22);
            ptta_pack_conv_in(src, l.cin, 0, l.cin, 0, l.wfrag, l.wcanon, s);
            if (l.cin == 2) ptta_pack_conv_out1(src, 2, 1, 1, l.bw, s);      // gradient w.r.t. the predicted-depth plane
        } else if (is_b) { HIPCHK(hipMemcpyAsync(l.bias, src, 32 * 4, hipMemcpyDeviceToDevice, s)); }
        else return c->fail("unknown key " + name, -2);
        return 0;
    }
    if (c->lout.count(base)) {
        LOut& l = c->lout[base];
        if (is_w) {
            if (numel != 288) return c->fail("bad shape for " + name, -22);
            ptta_pack_conv_out1(src, 0, 0, 0, l.w, s);
            ptta_pack_conv_in(src, 1, 0, 1, 1, l.bfrag, l.bcanon, s);
        } else if (is_b) { HIPCHK(hipMemcpyAsync(l.bias, src, 4, hipMemcpyDeviceToDevice, s)); }
        else return c->fail("unknown key " + name, -2);
        return 0;
    }
    if (c->fc.count(base)) {
        Lin& l = c->fc[base];
        if (is_w) {
            if (numel != (long)l.N * l.K) return c->fail("bad shape for " + name, -22);
            HIPCHK(hipMemcpyAsync(l.W, src, (size_t)numel * 4, hipMemcpyDeviceToDevice, s));
            hipLaunchKernelGGL(transpose_kernel, dim3(nblk(numel)), dim3(256), 0, s, src, l.Wt, l.N, l.K);
            ptta_split_weight(l.W, l.Whi, l.Wlo, l.Wil, numel, l.K, s);            // [N][K]
            ptta_split_weight(l.Wt, l.Wthi, l.Wtlo, l.Wtil, numel, l.N, s);        // transposed: [K][N]
            if (l.Wsl) { ptta_hn_pack_w(l.Whi, l.Wsl, 512, s); ptta_hn_pack_w(l.Wthi, l.Wtsl, 512, s); }
            if (base == "proj.0") ptta_pack_w0_frag(l.W, c->w0frag, s);
        } else if (is_b) { HIPCHK(hipMemcpyAsync(l.bias, src, (size_t)l.N * 4, hipMemcpyDeviceToDevice, s)); }
        else return c->fail("unknown key " + name, -2);
        return 0;
    }
    if (c->bn.count(base)) {
        BNorm& b = c->bn[base];
        if (is_w) { HIPCHK(hipMemcpyAsync(b.gamma, src, 512 * 4, hipMemcpyDeviceToDevice, s)); }
        else if (is_b) { HIPCHK(hipMemcpyAsync(b.beta, src, 512 * 4, hipMemcpyDeviceToDevice, s)); }
        else if (ends(".running_mean")) b.rm = (float*)tensor;               // bound, updated in place
        else if (ends(".running_var")) b.rv = (float*)tensor;
        else if (ends(".num_batches_tracked")) b.nbt = (long long*)tensor;
        else return c->fail("unknown key " + name, -2);
        return 0;
    }
    return c->fail("unknown key " + name, -2);
}

int ptta_bind_adapted(ptta_handle c, const char* name_, float* param, float* exp_avg, float* exp_avg_sq) {
    NLFWD(c->nl->bind_adapted(name_, param, exp_avg, exp_avg_sq));

    if (!c || !name_ || !param) return -1;
    c->drop_graphs();
    const std::string name(name_);
    for (size_t k = 0; k < c->adapted.size(); ++k)
        if (c->adapted[k].name == name) {
            c->adapted[k].p = param; c->adapted[k].m = exp_avg; c->adapted[k].v = exp_avg_sq;
            c->adam_tab_dirty = true;
            if (c->meta_mode == PTTA_META_1LAYER) { if (k == 0) c->meta_w = param; else c->meta_b = param; }
            return 0;
        }
    return c->fail("not an adapted parameter: " + name, -2);
}

int ptta_adapted_count(ptta_handle c) { return c ? (c->nl ? c->nl->adapted_count() : (int)c->adapted.size()) : 0; }
const char* ptta_adapted_name(ptta_handle c, int index, int64_t* numel) {
    NLFWD(c->nl->adapted_name(index, numel));

    if (!c || index < 0 || index >= (int)c->adapted.size()) return nullptr;
    if (numel) *numel = c->adapted[index].n;
    return c->adapted[index].name.c_str();
}
int ptta_adapted_repeat(ptta_handle c, int index) {
    if (!c) return 0;
    if (c->nl) return c->nl->adapted_repeat(index);
    return (index >= 0 && index < (int)c->adapted.size()) ? 1 : 0;
}
int ptta_get_grad(ptta_handle c, const char* name, float* dst, int64_t capacity, ptta_stream s) {
    NLFWD(c->nl->get_grad(name, dst, capacity, (hipStream_t)s));

    if (!c || !name || !dst) return -1;
    for (auto& ad : c->adapted)
        if (ad.name == name) {
            if (capacity < ad.n) return c->fail("capacity too small", -22);
            HIPCHK(hipMemcpyAsync(dst, ad.g, (size_t)ad.n * 4, hipMemcpyDeviceToDevice, (hipStream_t)s));
            return 0;
        }
    return c->fail(std::string("not an adapted parameter: ") + name, -2);
}

int ptta_set_grad(ptta_handle c, const char* name, const float* src, int64_t numel, ptta_stream s) {
    NLFWD(c->nl->set_grad(name, src, numel, (hipStream_t)s));
    if (!c || !name || !src) return -1;
    for (auto& ad : c->adapted)
        if (ad.name == name) {
            if (numel != ad.n) return c->fail("ptta_set_grad: size mismatch", -22);
            HIPCHK(hipMemcpyAsync(ad.g, src, (size_t)ad.n * 4, hipMemcpyDeviceToDevice, (hipStream_t)s));
            return 0;
        }
    return c->fail(std::string("not an adapted parameter: ") + name, -2);
}

int ptta_set_adam_step(ptta_handle c, int step, ptta_stream s) {
    NLFWD(c->nl->set_adam_step(step, (hipStream_t)s));

    if (!c) return -1;
    RUN(ptta_launch_set_int(c->step_dev, step, (hipStream_t)s));
    return 0;
}
int ptta_get_adam_step(ptta_handle c, int* step, ptta_stream s) {
    NLFWD(c->nl->get_adam_step(step, (hipStream_t)s));

    if (!c || !step) return -1;
    HIPCHK(hipMemcpyAsync(step, c->step_dev, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)s));
    HIPCHK(hipStreamSynchronize((hipStream_t)s));
    return 0;
}

int64_t ptta_embedding_rows(ptta_handle c) { return c ? (c->nl ? c->nl->rows() : c->Rg) : 0; }

int ptta_forward_train(ptta_handle c, const float* image, const float* sparse, float* depth_out, float* emb_out, float* ref_out, ptta_stream s_) {
    if (c) c->err_code = 0;
    NLFWD(c->nl->forward_train(image, sparse, depth_out, emb_out, ref_out, (hipStream_t)s_));

    if (!c || !image || !sparse) return -1;
    hipStream_t s = (hipStream_t)s_;
    if (c->pipe_active && !c->skip_prefix) {              // never the buffer set a prefix may be writing (ptta_step_pipelined) ...
        pipe_use(c, c->pipe_last);
        pipe_overwritten(c, c->pipe_last);               // ... and the set it DOES overwrite no longer holds the frame it was prepared for / adapted from
    }
    c->fwd_valid = false; c->head.fwd_ok = false; c->fb_image = c->fb_sparse = nullptr;
    RUN(forward_common(c, image, sparse, true, s));      // includes the heads (beside decoder 3)
    const size_t dbytes = (size_t)c->N * c->H * c->W * 4, ebytes = (size_t)c->Rg * 512 * 4;
    if (depth_out) HIPCHK(d2d_copy(depth_out, final_depth(c), dbytes, s));
    if (c->nar_heads && heads_v2_on(c)) {       // the caller's tensors are fp32: widened copies of the narrow embeddings
        if (emb_out) RUN(ptta_launch_hn_untile(c->emb_n, emb_out, c->Rg, s));
        if (ref_out) RUN(ptta_launch_hn_untile(c->ref_n, ref_out, c->Rg, s));
    } else {
    if (emb_out) HIPCHK(hipMemcpyAsync(emb_out, c->emb, ebytes, hipMemcpyDeviceToDevice, s));
    if (ref_out) HIPCHK(hipMemcpyAsync(ref_out, c->ref, ebytes, hipMemcpyDeviceToDevice, s));
    }
    c->fwd_valid = true;
    return 0;
}

int ptta_forward_eval(ptta_handle c, const float* image, const float* sparse, float* depth_out, ptta_stream s_) {
    if (c) c->err_code = 0;
    NLFWD(c->nl->forward_eval(image, sparse, depth_out, (hipStream_t)s_));

    if (!c || !image || !sparse || !depth_out) return -1;
    hipStream_t s = (hipStream_t)s_;
    if (c->pipe_active) { pipe_use(c, c->pipe_last); pipe_overwritten(c, c->pipe_last); }       // as ptta_forward_train
    c->fwd_valid = false; c->head.fwd_ok = false;        // the eval pass overwrites the saved activations
    c->fb_image = c->fb_sparse = nullptr;                // (ptta_forward_eval_last's fallback restores them around its own call)
    RUN(forward_common(c, image, sparse, false, s));
    HIPCHK(d2d_copy(depth_out, final_depth(c), (size_t)c->N * c->H * c->W * 4, s));
    return 0;
}

// The scored forward (src/tta_main.py:729-736) of the frame the last ptta_step_pipelined call adapted: the parameter-independent prefix of
// that frame is still in its buffer set (nothing in the step writes those tensors), so only the part downstream of the adapted layer runs.
int ptta_forward_eval_last(ptta_handle c, float* depth_out, ptta_stream s_) {
    if (!c || !depth_out) return -1;
    if (c->nl) return c->fail("ptta_forward_eval_last follows ptta_step_pipelined (MSG_CHN handles)", -38);
    if (!c->pipe_active) {
        // the last ptta_step_pipelined call ran as a plain ptta_step (no graph replay, profiling, SyncBatchNorm / gradient exchange, padded
        // sizes, bf16 storage ...): no prefix is held, so this is a full eval forward of that call's frame (its buffers are still the caller's)
        if (!c->fb_image || !c->fb_sparse) return c->fail("ptta_forward_eval_last: no frame adapted by ptta_step_pipelined since the last reset", -3);
        const float *im = c->fb_image, *sp = c->fb_sparse;
        const int rc = ptta_forward_eval(c, im, sp, depth_out, s_);
        c->fb_image = im; c->fb_sparse = sp;          // (still the last adapted frame: the call may be repeated)
        return rc;
    }
    if (!c->pset[c->pipe_last].last_token) return c->fail("ptta_forward_eval_last: no frame adapted by ptta_step_pipelined since the last reset", -3);
    hipStream_t s = (hipStream_t)s_;
    pipe_use(c, c->pipe_last);
    c->fwd_valid = false; c->head.fwd_ok = false;
    c->skip_prefix = true;
    const int rc = forward_common(c, c->in_image, c->in_sparse, false, s);
    c->skip_prefix = false;
    if (rc) return rc;
    HIPCHK(d2d_copy(depth_out, final_depth(c), (size_t)c->N * c->H * c->W * 4, s));
    return 0;
}

int ptta_loss_forward(ptta_handle c, const float* loss_image, const float* depth, const float* sparse, const float* validity,
                      const float* emb, const float* ref, int64_t rows, float w_sd, float w_sm, float w_cos,
                      float* loss_info_out, ptta_stream s_) {
    NLFWD(c->nl->loss_forward(loss_image, depth, sparse, validity, emb, ref, rows, w_sd, w_sm, w_cos, loss_info_out, (hipStream_t)s_));

    if (!c || !loss_image || !depth || !sparse || !validity || !loss_info_out) return -1;
    if (rows > c->Rg) return c->fail("rows exceeds the handle's embedding rows", -22);
    hipStream_t s = (hipStream_t)s_;
    const float w3[3] = {w_sd, w_sm, w_cos};
    RUN(ptta_launch_set_floats(c->w3_tmp, w3, 3, s));
    RUN(ptta_launch_loss_forward(depth, loss_image, sparse, validity, c->hp.max_input_depth, emb, ref, rows, 512, c->w3_tmp,
                                 c->N, c->H, c->W, c->loss_ws, loss_info_out, s));
    return 0;
}

int ptta_loss_backward(ptta_handle c, const float* loss_image, const float* depth, const float* sparse, const float* validity,
                       const float* emb, const float* ref, int64_t rows, float* gdepth, float* gref, ptta_stream s_) {
    NLFWD(c->nl->loss_backward(loss_image, depth, sparse, validity, emb, ref, rows, gdepth, gref, (hipStream_t)s_));

    if (!c || !loss_image || !depth || !sparse || !validity || !gdepth) return -1;
    RUN(ptta_launch_loss_backward(depth, loss_image, sparse, validity, c->hp.max_input_depth, emb, ref, rows, 512,
                                  c->N, c->H, c->W, c->loss_ws, gdepth, gref, (hipStream_t)s_));
    return 0;
}

int ptta_backward(ptta_handle c, const float* grad_depth, const float* grad_ref, float* gw_out, float* gb_out, ptta_stream s_) {
    NLFWD(grad_depth ? c->nl->backward_from(grad_depth, grad_ref, (hipStream_t)s_) : -1);   // gradients: ptta_get_grad

    if (!c || !grad_depth) return -1;
    if (!c->fwd_valid) return c->fail("ptta_backward without a preceding ptta_forward_train", -3);
    hipStream_t s = (hipStream_t)s_;
    const float* g_net = grad_depth;
    if (c->dual) {
        hipLaunchKernelGGL(scatter_dual_grad_kernel, dim3(nblk((long)c->Nn * c->Hp * c->Wp)), dim3(256), 0, s, grad_depth, c->g_net,
                           c->N, c->H, c->W, c->Hp, c->Wp, c->pt, c->pr);
        g_net = c->g_net;
    }
    bool join_aux = false;
    if (grad_ref) {
        hipStream_t s2 = c->aux(s);
        if (s2) {
            HIPCHK(hipEventRecord(c->ev_fork, s)); HIPCHK(hipStreamWaitEvent(s2, c->ev_fork, 0));
            RUN(heads_backward(c, grad_ref, s2));
            HIPCHK(hipEventRecord(c->ev_join, s2));
            join_aux = true;
        } else RUN(heads_backward(c, grad_ref, s));
    } else HIPCHK(hipMemsetAsync(c->g_feat, 0, (size_t)c->Rg * 32 * (c->nar_bwd ? 2 : c->es), s));
    RUN(backbone_backward(c, g_net, s, join_aux));
    if (c->meta_mode == PTTA_META_1LAYER) {
        if (gw_out) HIPCHK(hipMemcpyAsync(gw_out, c->gW, 9216 * 4, hipMemcpyDeviceToDevice, s));
        if (gb_out) HIPCHK(hipMemcpyAsync(gb_out, c->gB, 32 * 4, hipMemcpyDeviceToDevice, s));
    }
    return 0;
}

// pointer table of the adapted tensors for the one-launch Adam; uploaded after ptta_bind_adapted only, never inside a capture
static int ensure_adam_table(ptta_ctx* c, hipStream_t s) {
    if (!c->adam_tab_dirty) return 0;
    for (auto& ad : c->adapted) if (!ad.p || !ad.m || !ad.v) return 0;          // reported by ptta_adam_step
    c->adam_host.resize(c->adapted.size());
    long off = 0;
    for (size_t k = 0; k < c->adapted.size(); ++k) { auto& ad = c->adapted[k]; c->adam_host[k] = PttaAdamEntry{ad.p, ad.m, ad.v, ad.g, ad.n, off}; off += ad.n; }
    HIPCHK(hipMemcpyAsync(c->adam_tab, c->adam_host.data(), c->adam_host.size() * sizeof(PttaAdamEntry), hipMemcpyHostToDevice, s));
    c->adam_tab_dirty = false;
    return 0;
}

int ptta_adam_step(ptta_handle c, const float* gw, const float* gb, ptta_stream s_) {
    if (c && c->nl) return (gw || gb) ? c->fail("explicit gradients are an MSG_CHN 1layer convenience", -22) : c->nl->adam_step((hipStream_t)s_);

    if (!c) return -1;
    for (auto& ad : c->adapted) if (!ad.p || !ad.m || !ad.v) return c->fail("Adam state of " + ad.name + " not bound", -3);
    if ((gw || gb) && c->meta_mode != PTTA_META_1LAYER) return c->fail("explicit gradients are a 1layer convenience; use the internal ones", -22);
    hipStream_t s = (hipStream_t)s_;
    if (!gw && !gb) {                       // the internal gradients: every adapted tensor + the step count in one launch
        RUN(ensure_adam_table(c, s));
        long total = 0; for (auto& ad : c->adapted) total += ad.n;
        REST_(s, ptta_launch_adam_multi(c->adam_tab, (int)c->adapted.size(), total, c->hyper, c->step_dev, c->adam_ticket, s));
        return 0;
    }
    RUN(ptta_launch_step_inc(c->step_dev, s));
    for (size_t k = 0; k < c->adapted.size(); ++k) {
        auto& ad = c->adapted[k];
        const float* g = ad.g;
        if (c->meta_mode == PTTA_META_1LAYER) { if (k == 0 && gw) g = gw; if (k == 1 && gb) g = gb; }
        RUN(ptta_launch_adam(ad.p, ad.m, ad.v, g, ad.n, c->hyper, c->step_dev, s));
    }
    return 0;
}

static int step_tail(ptta_handle c, const float* loss_image, const float* sparse, const float* validity, ptta_stream s_);
static bool thru_ok(ptta_ctx* c, hipStream_t s) {
    return c->thru && c->cos_grad_fused && heads_v2_on(c) && c->N <= 16 && c->aux(s) != nullptr;
}
static int step_body(ptta_handle c, const float* image, const float* loss_image, const float* sparse, const float* validity,
                     ptta_stream s_) {
    RUN(ensure_fused_heads(c, (hipStream_t)s_));             // (before thru_ok: the direct-launch step would otherwise take the joined tail on its first call only)
    c->thru_active = thru_ok(c, (hipStream_t)s_);
    c->cnt_sparse = c->thru_active ? sparse : nullptr; c->cnt_validity = validity;
    const int rc = ptta_forward_train(c, image, sparse, nullptr, nullptr, nullptr, s_);
    if (rc) { c->thru_active = false; c->cnt_sparse = nullptr; return rc; }
    const int rc2 = step_tail(c, loss_image, sparse, validity, s_);
    c->thru_active = false; c->cnt_sparse = nullptr; c->loss_report.on = false;
    return rc2;
}
// loss + backward + (gradient all-reduce) + Adam: everything of the step behind the forward
static int step_tail(ptta_handle c, const float* loss_image, const float* sparse, const float* validity, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (c->thru_active) {
        hipStream_t s2 = c->aux(s);
        if (!c->ev_dpart) HIPCHK(hipEventCreateWithFlags(&c->ev_dpart, kStepEvent));
        // auxiliary stream, behind the heads' forward: cosine rows (mixed mode: the ref GEMM's epilogue already left the row statistics and the
        // block partials in the loss workspace), the gated coefficient, the heads' backward -- none of it waits for decoder 3 or the depth terms
        if (!(c->nar_heads && heads_v2_on(c) && c->cos_rows_done)) REST_(s2, ptta_launch_loss_cos_part(c->emb, c->ref, c->Rg, 512, c->N, c->loss_ws, s2));
        HIPCHK(hipEventRecord(c->ev_dpart, s2));                // (the cosine partials exist)
        REST_(s2, ptta_launch_loss_cos_coef(c->loss_ws, c->N, c->Rg, c->hyper + 5, s2));
        // main stream: the depth gradient at once -- its coefficients come from the valid-weight partials the auxiliary stream computed at the
        // start of the step (backbone; ev_dpart lies behind them on that stream); the loss VALUES (depth terms + finalisation: the four reported
        // scalars) are reduced on the auxiliary stream beside the backward (backbone_backward), not in front of it
        HIPCHK(hipStreamWaitEvent(s, c->ev_dpart, 0));
        if (!c->ev_loss) HIPCHK(hipEventCreateWithFlags(&c->ev_loss, kStepEvent));
        c->loss_report.image = loss_image; c->loss_report.sparse = sparse; c->loss_report.validity = validity; c->loss_report.on = true;
        REST_(s, ptta_launch_loss_backward(final_depth(c), loss_image, sparse, validity, c->hp.max_input_depth, nullptr, nullptr, c->Rg, 512,
                                           c->N, c->H, c->W, c->loss_ws, c->g_final, nullptr, s, c->hyper + 5, nullptr, 1, 1));
        c->cos_in_gemm = true;
        const int rc_h = heads_backward(c, c->gref_buf, s2);
        c->cos_in_gemm = false;
        if (rc_h) return rc_h;
        c->stamp(8, s2);
        HIPCHK(hipEventRecord(c->ev_join, s2));
        const float* g_net = c->g_final;
        if (c->dual) {
            hipLaunchKernelGGL(scatter_dual_grad_kernel, dim3(nblk((long)c->Nn * c->Hp * c->Wp)), dim3(256), 0, s, c->g_final, c->g_net,
                               c->N, c->H, c->W, c->Hp, c->Wp, c->pt, c->pr);
            g_net = c->g_net;
        }
        c->adam_fuse_req = true; c->adam_fused = false;
        const int rc_bb = backbone_backward(c, g_net, s, true);
        c->adam_fuse_req = false;
        if (rc_bb) return rc_bb;
        if (c->grad_comm && ptta_rccl_allreduce_mean_f32(c->grad_comm, c->grad_arena, c->grad_arena_n, s_)) return c->fail(std::string("gradient all-reduce: ") + ptta_rccl_last_error(), -5);
        c->stamp(9, s);
        if (!c->adam_fused) RUN(ptta_adam_step(c, nullptr, nullptr, s_));
        c->stamp(10, s);
        return 0;
    }
    // validity == NULL: where(sparse > 0, 1, sparse) is evaluated inside the loss kernels; the loss finalisation runs inside
    // the two gradient kernels (no 1-block launch between forward and backward)
    if (c->nar_heads && heads_v2_on(c)) {       // (one-stream fallback of the mixed mode -- profiling leg, no second stream: the fp32 loss kernels on widened copies)
        RUN(ptta_launch_hn_untile(c->emb_n, c->emb, c->Rg, s));
        RUN(ptta_launch_hn_untile(c->ref_n, c->ref, c->Rg, s));
    }
    REST_(s, ptta_launch_loss_forward(final_depth(c), loss_image, sparse, validity, c->hp.max_input_depth, c->emb, c->ref, c->Rg, 512,
                                      c->hyper + 5, c->N, c->H, c->W, c->loss_ws, c->loss_info_dst ? c->loss_info_dst : c->loss_info, s, 1));
    const bool cig = c->cos_grad_fused && heads_v2_on(c) && c->N <= 16;          // (N <= LOSS_FIN_MAXN: the gradient launch finalises the loss)
    REST_(s, ptta_launch_loss_backward(final_depth(c), loss_image, sparse, validity, c->hp.max_input_depth, c->emb, c->ref, c->Rg, 512,
                                       c->N, c->H, c->W, c->loss_ws, c->g_final, cig ? nullptr : c->gref_buf, s, c->hyper + 5, c->loss_info_dst ? c->loss_info_dst : c->loss_info));
    c->cos_in_gemm = cig;
    c->adam_fuse_req = true; c->adam_fused = false;
    const int rc_b = ptta_backward(c, c->g_final, c->gref_buf, nullptr, nullptr, s_);
    c->cos_in_gemm = false; c->adam_fuse_req = false;
    if (rc_b) return rc_b;
    // shared-parameter run (the reference's DDP, src/tta_main.py:354,631-633): mean of the adapted gradients over the ranks, one message
    if (c->grad_comm && ptta_rccl_allreduce_mean_f32(c->grad_comm, c->grad_arena, c->grad_arena_n, s_)) return c->fail(std::string("gradient all-reduce: ") + ptta_rccl_last_error(), -5);
    if (!c->adam_fused) RUN(ptta_adam_step(c, nullptr, nullptr, s_));
    return 0;
}

int ptta_step(ptta_handle c, const float* image, const float* loss_image, const float* sparse, const float* validity,
              float* depth_out, float* loss_info_out, ptta_stream s_) {
    if (c) c->err_code = 0;
    if (!c || !image || !sparse) return -1;
    if (c->nl) return c->nl->step(image, loss_image, sparse, validity, depth_out, loss_info_out, (hipStream_t)s_);
    RUN(pipe_quiesce(c));
    hipStream_t s = (hipStream_t)s_;
    if (!loss_image) loss_image = image;
    const size_t ibytes = (size_t)c->N * 3 * c->H * c->W * 4, pbytes = (size_t)c->N * c->H * c->W * 4;
    if (c->use_graph && !c->prof_on) {
        // replay path: stage the inputs at fixed addresses, then one hipGraphLaunch
        const int key = (validity ? 2 : 0) | (loss_image != image ? 1 : 0);
        HIPCHK(d2d_copy(c->in_image, image, ibytes, s));
        HIPCHK(d2d_copy(c->in_sparse, sparse, pbytes, s));
        if (key & 1) HIPCHK(d2d_copy(c->in_loss_image, loss_image, ibytes, s));
        if (key & 2) HIPCHK(d2d_copy(c->in_validity, validity, pbytes, s));
        RUN(ensure_fused_heads(c, s));
        {
        if (!c->gexec[key]) {
            RUN(ensure_proxy_rgb(c, c->in_image, s));        // outside the capture: the graph holds the real-frame encoder only
            RUN(ensure_adam_table(c, s));
            if (!c->cap_stream) HIPCHK(hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking));
            HIPCHK(hipStreamBeginCapture(c->cap_stream, hipStreamCaptureModeThreadLocal));
            const int rc = step_body(c, c->in_image, (key & 1) ? c->in_loss_image : c->in_image, c->in_sparse,
                                     (key & 2) ? c->in_validity : nullptr, (ptta_stream)c->cap_stream);
            hipGraph_t g = nullptr;
            const hipError_t e = hipStreamEndCapture(c->cap_stream, &g);
            if (rc != 0) { if (g) (void)hipGraphDestroy(g); return rc; }
            if (e != hipSuccess || !g) return c->fail(std::string("hipStreamEndCapture: ") + hipGetErrorString(e), -100 - (int)e);
            c->graph[key] = g;
            HIPCHK(hipGraphInstantiate(&c->gexec[key], g, nullptr, nullptr, 0));
        }
        HIPCHK(hipGraphLaunch(c->gexec[key], s));
        }
        if (!c->ev_replay) HIPCHK(hipEventCreateWithFlags(&c->ev_replay, hipEventDisableTiming));
        HIPCHK(hipEventRecord(c->ev_replay, s));
        c->fwd_valid = true;
    } else {
        c->loss_info_dst = loss_info_out;                  // (written by the loss kernel itself)
        const int rc = step_body(c, image, loss_image, sparse, validity, s_);
        c->loss_info_dst = nullptr;
        if (rc) return rc;
        if (depth_out) HIPCHK(d2d_copy(depth_out, final_depth(c), pbytes, s));
        return 0;
    }
    if (depth_out) HIPCHK(d2d_copy(depth_out, final_depth(c), pbytes, s));
    if (loss_info_out) HIPCHK(d2d_copy(loss_info_out, c->loss_info, 16, s));
    return 0;
}

}  // extern "C"

// ---- frame pipelining -------------------------------------------------------------------------------------------------------
namespace {
static void pipe_save(ptta_ctx* c, ptta_ctx::PreSet& P) {
    P.c0 = c->c0; P.c1 = c->c1; P.c2 = c->c2; P.c3 = c->c3; P.c4 = c->c4; P.e1_0a = c->e1_0a; P.e1_0 = c->e1_0; P.e1_1a = c->e1_1a;
    P.c0a = c->c0a; P.c1a = c->c1a; P.c2a = c->c2a; P.c3a = c->c3a; P.c4a = c->c4a;
    P.e1_1 = c->e1_1; P.y1 = c->y1; P.e1_2a = c->e1_2a; P.y2 = c->y2; P.t1 = c->t1; P.y3 = c->y3; P.s1_1 = c->s1_1; P.u1 = c->u1;
    P.dclamp = c->dclamp; P.d12 = c->d12; P.d14 = c->d14;
    P.in_image = c->in_image; P.in_loss_image = c->in_loss_image; P.in_sparse = c->in_sparse; P.in_validity = c->in_validity;
    P.proxy_valid = c->proxy_rgb_valid;
}
static void pipe_use(ptta_ctx* c, int p) {
    if (p == c->cur_set) return;
    pipe_save(c, c->pset[c->cur_set]);
    const ptta_ctx::PreSet& P = c->pset[p];
    c->c0 = P.c0; c->c1 = P.c1; c->c2 = P.c2; c->c3 = P.c3; c->c4 = P.c4; c->e1_0a = P.e1_0a; c->e1_0 = P.e1_0; c->e1_1a = P.e1_1a;
    c->c0a = P.c0a; c->c1a = P.c1a; c->c2a = P.c2a; c->c3a = P.c3a; c->c4a = P.c4a;
    c->e1_1 = P.e1_1; c->y1 = P.y1; c->e1_2a = P.e1_2a; c->y2 = P.y2; c->t1 = P.t1; c->y3 = P.y3; c->s1_1 = P.s1_1; c->u1 = P.u1;
    c->dclamp = P.dclamp; c->d12 = P.d12; c->d14 = P.d14;
    c->in_image = P.in_image; c->in_loss_image = P.in_loss_image; c->in_sparse = P.in_sparse; c->in_validity = P.in_validity;
    c->proxy_rgb_valid = P.proxy_valid;
    c->cur_set = p;
}
static int pipe_init(ptta_ctx* c) {
    if (c->pipe_ready) return 0;
    const int Nn = c->Nn, B2 = 2 * Nn, H1 = c->Hp, W1 = c->Wp;
    const size_t es = c->es;
    auto A = [&](int nb, int h, int w) { return c->dalloc((size_t)nb * h * w * 32 * es); };
    pipe_save(c, c->pset[c->cur_set]);                       // the set the handle was built with (0)
    ptta_ctx::PreSet& Q = c->pset[1];
    Q.c0 = A(B2, H1, W1); Q.c1 = A(B2, c->H2, c->W2); Q.c2 = A(B2, c->H4, c->W4); Q.c3 = A(B2, c->H8, c->W8); Q.c4 = A(B2, c->H16, c->W16);
    Q.c0a = A(B2, H1, W1); Q.c1a = A(B2, c->H2, c->W2); Q.c2a = A(B2, c->H4, c->W4); Q.c3a = A(B2, c->H8, c->W8); Q.c4a = A(B2, c->H16, c->W16);
    Q.e1_0a = A(Nn, c->H4, c->W4); Q.e1_0 = A(Nn, c->H4, c->W4); Q.e1_1a = A(Nn, c->H8, c->W8);
    Q.e1_1 = A(B2, c->H8, c->W8); Q.y1 = A(B2, c->H8, c->W8); Q.e1_2a = A(Nn, c->H16, c->W16); Q.y2 = A(B2, c->H16, c->W16);
    Q.t1 = A(B2, c->H8, c->W8); Q.y3 = A(B2, c->H8, c->W8); Q.s1_1 = A(B2, c->H8, c->W8); Q.u1 = A(B2, c->H4, c->W4);
    Q.dclamp = c->falloc((size_t)Nn * H1 * W1); Q.d12 = c->falloc((size_t)Nn * c->H2 * c->W2); Q.d14 = c->falloc((size_t)Nn * c->H4 * c->W4);
    Q.in_image = c->falloc((size_t)c->N * 3 * c->H * c->W); Q.in_loss_image = c->falloc((size_t)c->N * 3 * c->H * c->W);
    Q.in_sparse = c->falloc((size_t)c->N * c->H * c->W); Q.in_validity = c->falloc((size_t)c->N * c->H * c->W);
    if (c->nar_proxy) {      // narrow twins of the second set's prefix outputs (proxy frames) and of its depth-only maps
        for (auto& t_ : {std::make_pair(Q.c1, std::make_pair(c->H2, c->W2)), std::make_pair(Q.c2, std::make_pair(c->H4, c->W4)),
                         std::make_pair(Q.c3, std::make_pair(c->H8, c->W8)), std::make_pair(Q.c4, std::make_pair(c->H16, c->W16)),
                         std::make_pair(Q.y1, std::make_pair(c->H8, c->W8)), std::make_pair(Q.y2, std::make_pair(c->H16, c->W16)),
                         std::make_pair(Q.t1, std::make_pair(c->H8, c->W8)), std::make_pair(Q.y3, std::make_pair(c->H8, c->W8)),
                         std::make_pair(Q.s1_1, std::make_pair(c->H8, c->W8)), std::make_pair(Q.u1, std::make_pair(c->H4, c->W4)),
                         std::make_pair(Q.e1_0, std::make_pair(c->H4, c->W4)), std::make_pair(Q.e1_1a, std::make_pair(c->H8, c->W8)),
                         std::make_pair(Q.e1_2a, std::make_pair(c->H16, c->W16))})
            c->twin_alloc(t_.first, Nn, t_.second.first, t_.second.second);
    }
    if (c->oom) return c->fail("out of device memory (second prefix buffer set)", -12);
    HIPCHK(hipStreamCreateWithFlags(&c->pre_stream, hipStreamNonBlocking));
    for (int p = 0; p < 2; ++p) {
        HIPCHK(hipEventCreateWithFlags(&c->ev_prefix[p], kStepEvent));
        HIPCHK(hipEventCreateWithFlags(&c->ev_rest[p], kStepEvent));
    }
    // ev_entry also publishes what the CALLER queued before the call (the next frame's H2D / peer copy) to the prefix stream: a plain
    // event (system-scope release), unlike the handle-internal fork / join events
    HIPCHK(hipEventCreateWithFlags(&c->ev_entry, hipEventDisableTiming));
    c->pipe_ready = true;
    return 0;
}
// any entry point that is not ptta_step_pipelined: wait for a prefix in flight, forget it, go back to buffer set 0
static int pipe_quiesce(ptta_ctx* c) {
    c->fb_image = c->fb_sparse = nullptr;          // (the frame of a ptta_step_pipelined call that ran as ptta_step: forgotten with the rest)
    if (!c->pipe_active) return 0;
    HIPCHK(hipStreamSynchronize(c->pre_stream));
    for (int p = 0; p < 2; ++p) { c->pset[p].prepared = false; c->pset[p].prep_token = c->pset[p].last_token = 0; }
    pipe_use(c, 0);
    c->pipe_cur = 0; c->pipe_last = 0; c->pipe_active = false;
    return 0;
}
static int prefix_body(ptta_ctx* c, const float* image, const float* sparse, hipStream_t s) {
    c->stamp(11, s);
    RUN(ptta_launch_prep(sparse, c->hp.max_input_depth, c->dclamp, c->d12, c->d14, c->Nn, c->Hp, c->Wp, s));
    RUN(rgb_encoder(c, image, c->Nn, 0, c->Nn, s));
    c->stamp(12, s);
    RUN(enc1_head_fn(c, s));
    RUN(stage1_independent(c, 2 * c->Nn, s));
    c->stamp(13, s);
    return 0;
}
template <class F>
static int pipe_capture(ptta_ctx* c, hipGraph_t* g_out, hipGraphExec_t* e_out, F body);
template <class F>
static int pipe_capture(ptta_ctx* c, hipGraph_t* g_out, hipGraphExec_t* e_out, F body) {
    if (!c->cap_stream) HIPCHK(hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking));
    HIPCHK(hipStreamBeginCapture(c->cap_stream, hipStreamCaptureModeThreadLocal));
    const int rc = body(c->cap_stream);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(c->cap_stream, &g);
    if (rc != 0) { if (g) (void)hipGraphDestroy(g); return rc; }
    if (e != hipSuccess || !g) return c->fail(std::string("hipStreamEndCapture: ") + hipGetErrorString(e), -100 - (int)e);
    *g_out = g;
    HIPCHK(hipGraphInstantiate(e_out, g, nullptr, nullptr, 0));
    return 0;
}

}  // namespace

extern "C" {

// The stream ptta_step_pipelined runs the next frame's prefix on (created on first use): a host that produces that frame asynchronously
// (an H2D copy on its own stream) orders the copy's event on THIS stream instead of delaying the current frame's step with it.
int ptta_pipeline_stream(ptta_handle c, ptta_stream* out) {
    if (!c || !out) return -1;
    if (c->nl) return c->fail("frame pipelining is built for MSG_CHN handles", -38);
    RUN(pipe_init(c));
    *out = (ptta_stream)c->pre_stream;
    return 0;
}

// One TTA step on (image, sparse) AND, beside it, the parameter-independent prefix of the NEXT frame (next_image, next_sparse; NULL: none).
// Same results as ptta_step call by call.  Frames are named by caller-chosen TOKENS (non-zero, a new one for every new frame CONTENT): the
// prefix prepared for `next_token` is used by the following call iff that call's `frame_token` equals it -- never by pointer identity, so a
// caller that refills one staging buffer is safe as long as the refill gets a new token.  The announced frame is copied to the handle's own
// staging buffers when it is announced: the caller's buffers only have to hold it until this call's copies have run on the prefix stream.
int ptta_step_pipelined(ptta_handle c, const float* image, const float* loss_image, const float* sparse, const float* validity, uint64_t frame_token,
                        const float* next_image, const float* next_sparse, uint64_t next_token, float* depth_out, float* loss_info_out, ptta_stream s_) {
    if (c) c->err_code = 0;
    if (!c || !image || !sparse) return -1;
    if (c->nl || c->prof_on || c->dual || c->stat_sync.on() || c->grad_comm || c->naive || c->bf16) {
        const int rc = ptta_step(c, image, loss_image, sparse, validity, depth_out, loss_info_out, s_);
        if (!c->nl) { c->fb_image = rc ? nullptr : image; c->fb_sparse = rc ? nullptr : sparse; }       // for ptta_forward_eval_last
        return rc;
    }
    hipStream_t s = (hipStream_t)s_;
    if (!loss_image) loss_image = image;
    RUN(pipe_init(c));
    c->pipe_active = true;
    const size_t ibytes = (size_t)c->N * 3 * c->H * c->W * 4, pbytes = (size_t)c->N * c->H * c->W * 4;
    const int p = c->pipe_cur, q = 1 - p;
    const int key = (validity ? 2 : 0) | (loss_image != image ? 1 : 0);
    // (a caller that moves to another stream: the steps queued on the previous one come first -- everything below orders against `s` only)
    if (c->pipe_stream_set && c->pipe_stream != s) { HIPCHK(hipEventRecord(c->ev_rest[0], c->pipe_stream)); HIPCHK(hipStreamWaitEvent(s, c->ev_rest[0], 0)); }
    c->pipe_stream = s; c->pipe_stream_set = true;
    HIPCHK(hipEventRecord(c->ev_entry, s));                   // what the caller queued before this call (the next frame's data, too) -- and every earlier step
    pipe_use(c, p);
    RUN(ensure_fused_heads(c, s));                            // (ptta_head_reload / ptta_head_step invalidate the merged head GEMM only)
    if (!c->proxy_rgb_valid) RUN(ensure_proxy_rgb(c, c->in_image, s));
    RUN(ensure_adam_table(c, s));
    ptta_ctx::PreSet& P = c->pset[p];
    if (P.prepared && frame_token != 0 && P.prep_token == frame_token) {
        HIPCHK(hipStreamWaitEvent(s, c->ev_prefix[p], 0));
    } else {                                                  // first call, or the caller did not announce this frame: prefix in line
        HIPCHK(hipStreamSynchronize(c->pre_stream));          // (a prefix of another frame may still be writing this set) -- the ONE host wait of this path
        HIPCHK(d2d_copy(c->in_image, image, ibytes, s));
        HIPCHK(d2d_copy(c->in_sparse, sparse, pbytes, s));
        if (!c->use_graph) RUN(prefix_body(c, c->in_image, c->in_sparse, s));
        else {
        if (!c->pexec[p]) RUN(pipe_capture(c, &c->pgraph[p], &c->pexec[p], [&](hipStream_t cs) { return prefix_body(c, c->in_image, c->in_sparse, cs); }));
        HIPCHK(hipGraphLaunch(c->pexec[p], s));
        }
    }
    P.prepared = false; P.prep_token = 0;
    if (key & 1) HIPCHK(d2d_copy(c->in_loss_image, loss_image, ibytes, s));
    if (key & 2) HIPCHK(d2d_copy(c->in_validity, validity, pbytes, s));
    if (!c->use_graph) {
        c->skip_prefix = true; c->loss_info_dst = loss_info_out;
        const int rc = step_body(c, c->in_image, (key & 1) ? c->in_loss_image : c->in_image, c->in_sparse, (key & 2) ? c->in_validity : nullptr, (ptta_stream)s);
        c->skip_prefix = false; c->loss_info_dst = nullptr;
        if (rc) return rc;
    } else {
    if (!c->rexec[key][p]) {
        c->skip_prefix = true;
        const int rc = pipe_capture(c, &c->rgraph[key][p], &c->rexec[key][p], [&](hipStream_t cs) {
            return step_body(c, c->in_image, (key & 1) ? c->in_loss_image : c->in_image, c->in_sparse, (key & 2) ? c->in_validity : nullptr, (ptta_stream)cs);
        });
        c->skip_prefix = false;
        if (rc) return rc;
    }
    HIPCHK(hipGraphLaunch(c->rexec[key][p], s));
    }
    c->pipe_last = p; P.last_token = frame_token ? frame_token : ~(uint64_t)0;      // (an unnamed frame is still the one ptta_forward_eval_last scores)
    if (c->use_graph) {                                       // (direct launches: nothing to keep alive)
        if (!c->ev_replay) HIPCHK(hipEventCreateWithFlags(&c->ev_replay, hipEventDisableTiming));
        HIPCHK(hipEventRecord(c->ev_replay, s));
    }
    c->fwd_valid = true;
    if (depth_out) HIPCHK(d2d_copy(depth_out, final_depth(c), pbytes, s));
    if (loss_info_out && c->use_graph) HIPCHK(d2d_copy(loss_info_out, c->loss_info, 16, s));       // (direct launches: the loss kernel wrote it)
    if (next_token != 0 && next_token == frame_token) {
        // another step on the SAME frame (inner_iter > 1): its prefix is the one just used -- nothing in the step writes those tensors
        HIPCHK(hipEventRecord(c->ev_prefix[p], s));
        P.prepared = true; P.prep_token = frame_token;
    } else if (next_image && next_sparse && next_token != 0) {
        // the next frame's prefix into the other set, on its own stream: after the caller's data is there and after the step that last read
        // that set (two calls ago) is done with it.  (Queued AFTER this frame's remainder; handing it to the GPU before the remainder moves
        // it to the head of the step -- rocprofv3 timeline -- and changes nothing: 1.691 vs 1.693 ms.)
        pipe_use(c, q);
        ptta_ctx::PreSet& Q = c->pset[q];
        hipStream_t ps = c->pre_stream;
        HIPCHK(hipStreamWaitEvent(ps, c->ev_entry, 0));
        if (!c->proxy_rgb_valid) { HIPCHK(hipStreamSynchronize(ps)); RUN(ensure_proxy_rgb(c, c->in_image, s)); HIPCHK(hipStreamSynchronize(s)); }   // once per set
        HIPCHK(d2d_copy(c->in_image, next_image, ibytes, ps));
        HIPCHK(d2d_copy(c->in_sparse, next_sparse, pbytes, ps));
        if (!c->use_graph) RUN(prefix_body(c, c->in_image, c->in_sparse, ps));
        else {
        if (!c->pexec[q]) RUN(pipe_capture(c, &c->pgraph[q], &c->pexec[q], [&](hipStream_t cs) { return prefix_body(c, c->in_image, c->in_sparse, cs); }));
        HIPCHK(hipGraphLaunch(c->pexec[q], ps));
        }
        HIPCHK(hipEventRecord(c->ev_prefix[q], ps));
        Q.prepared = true; Q.prep_token = next_token; Q.last_token = 0;
        c->pipe_cur = q;
        pipe_use(c, p);                                       // the members point at the frame just processed (what final_depth etc. read)
    }
    return 0;
}


// ============================ stage-2 head trainer =============================================
// src/head_main.py:464-480 with loss_type 'head_selfsup_seq_ema[_reverse]' (network_exp_msg_chn_adapt.py:610-699): EMA of the
// target head, both backbone passes without gradient, heads forward with train-mode BatchNorm1d, prepare_loss, backward into
// pred (and proj when not `reverse`), Adam over the parameters that received a gradient.
static const char* const HEAD_NAMES[12] = {"proj.0.weight", "proj.0.bias", "proj.1.weight", "proj.1.bias", "proj.3.weight", "proj.3.bias",
                                           "pred.0.weight", "pred.0.bias", "pred.1.weight", "pred.1.bias", "pred.3.weight", "pred.3.bias"};
static long head_numel(int k) { return k == 0 ? 512L * 32 : (k == 4 || k == 6 || k == 10) ? 512L * 512 : 512L; }

static int head_init(ptta_ctx* c) {
    if (c->head.ready) return 0;
    if (c->nl) return c->fail("the stage-2 head trainer is built for MSG_CHN handles", -38);
    if (c->bf16) return c->fail("the stage-2 head trainer needs an fp32 handle", -38);
    if (c->dual) return c->fail("stage 2 runs on sizes divisible by 16 (the reference pads only in the 'adapt' forward, src/msg_chn_model_adapt.py:54-140)", -38);
    if (c->stat_sync.world > 1 && c->head.form != PTTA_HEAD_FORM_SYNCBN) return c->fail("the plain form of the stage-2 head trainer has no SyncBatchNorm exchange (ptta_head_set_form)", -38);
    auto& h = c->head;
    h.prm.resize(12); h.tgt.resize(6);
    h.garena_n = 0; for (int k = 0; k < 12; ++k) h.garena_n += head_numel(k);
    h.garena = c->falloc((size_t)h.garena_n);
    long goff = 0;
    for (int k = 0; k < 12; ++k) { h.prm[k].name = HEAD_NAMES[k]; h.prm[k].n = head_numel(k); h.prm[k].g = h.garena + goff; goff += h.prm[k].n; }
    for (int k = 0; k < 6; ++k) { h.tgt[k].name = std::string("proj_t.") + (HEAD_NAMES[k] + 5); h.tgt[k].n = head_numel(k); }
    h.hyper = c->falloc(8); h.tau2 = c->falloc(2); h.loss = c->falloc(1); h.loss_part = c->falloc(1024);
    const int chunks = ptta_linear_wgrad_chunks(c->Rg, nullptr);
    h.wpart = c->falloc((size_t)chunks * 512 * 512); h.bpart = c->falloc((size_t)chunks * 512);
    h.dp = c->falloc((size_t)c->Rg * 512);
    h.sv_mean = c->falloc(512); h.sv_inv = c->falloc(512); h.sv_scale = c->falloc(512); h.sv_shift = c->falloc(512);
    h.step = (int*)c->dalloc(4); h.ticket = (unsigned*)c->dalloc(4);
    h.tab = (PttaAdamEntry*)c->dalloc(12 * sizeof(PttaAdamEntry)); h.etab = (PttaAdamEntry*)c->dalloc(6 * sizeof(PttaAdamEntry));
    if (c->oom) return c->fail("out of device memory (head trainer workspace)", -12);
    const float hy[7] = {1e-3f, 0.9f, 0.999f, 1e-8f, 0.f, 0.f, 0.f};
    RUN(ptta_launch_set_floats(h.hyper, hy, 5, nullptr));
    const float t2[2] = {0.999f, (float)(1.0 - 0.999)};
    RUN(ptta_launch_set_floats(h.tau2, t2, 2, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));                 // creation-time only
    h.ready = true;
    return 0;
}

// re-derive the library's packed copies of one head tensor from its bound parameter (what ptta_load_weights does for it)
static int head_reload(ptta_ctx* c, int k, hipStream_t s) {
    const auto& e = c->head.prm[k];
    if (!e.p) return 0;
    c->fused_pp_valid = false;
    const std::string name = e.name, base = name.substr(0, name.rfind('.'));
    const bool is_w = name.size() > 7 && name.compare(name.size() - 7, 7, ".weight") == 0;
    if (c->fc.count(base)) {
        Lin& l = c->fc[base];
        if (is_w) {
            HIPCHK(hipMemcpyAsync(l.W, e.p, (size_t)e.n * 4, hipMemcpyDeviceToDevice, s));
            hipLaunchKernelGGL(transpose_kernel, dim3(nblk(e.n)), dim3(256), 0, s, (const float*)e.p, l.Wt, l.N, l.K);
            ptta_split_weight(l.W, l.Whi, l.Wlo, l.Wil, e.n, l.K, s);
            ptta_split_weight(l.Wt, l.Wthi, l.Wtlo, l.Wtil, e.n, l.N, s);
            if (l.Wsl) { ptta_hn_pack_w(l.Whi, l.Wsl, 512, s); ptta_hn_pack_w(l.Wthi, l.Wtsl, 512, s); }
            if (base == "proj.0") ptta_pack_w0_frag(l.W, c->w0frag, s);
        } else HIPCHK(hipMemcpyAsync(l.bias, e.p, (size_t)e.n * 4, hipMemcpyDeviceToDevice, s));
    } else {
        BNorm& b = c->bn[base];
        HIPCHK(hipMemcpyAsync(is_w ? b.gamma : b.beta, e.p, 512 * 4, hipMemcpyDeviceToDevice, s));
    }
    return 0;
}

int ptta_head_set_form(ptta_handle c, int form) {
    if (!c) return -1;
    NLFWD(c->nl->head_set_form(form));
    if (form != PTTA_HEAD_FORM_PLAIN && form != PTTA_HEAD_FORM_SYNCBN) return c->fail("ptta_head_set_form: PTTA_HEAD_FORM_PLAIN or PTTA_HEAD_FORM_SYNCBN", -22);
    if (c->head.stepped) return c->fail("ptta_head_set_form: the form is chosen before the first head step", -3);
    if (form == PTTA_HEAD_FORM_SYNCBN && c->mixed) return c->fail("the SyncBatchNorm form of the stage-2 head trainer needs an fp32 handle", -38);
    c->head.form = form;
    return 0;
}

int ptta_head_bind(ptta_handle c, const char* name_, float* param, float* exp_avg, float* exp_avg_sq) {
    if (!c || !name_ || !param) return -1;
    NLFWD(c->nl->head_bind(name_, param, exp_avg, exp_avg_sq));
    RUN(head_init(c));
    const std::string name(name_);
    auto& h = c->head;
    for (auto& e : h.prm) if (e.name == name) {
        if (!exp_avg || !exp_avg_sq) return c->fail("Adam moments of " + name + " are required", -22);
        e.p = param; e.m = exp_avg; e.v = exp_avg_sq; h.tab_mode = -1; h.etab_dirty = true; h.fwd_ok = h.bwd_ok = false;
        return 0;
    }
    for (auto& e : h.tgt) if (e.name == name) { e.p = param; h.etab_dirty = true; return 0; }
    return c->fail("not a head parameter: " + name, -2);
}

int ptta_head_set_hparams(ptta_handle c, float lr, float beta1, float beta2, float eps, float weight_decay, float tau, int adam_step,
                          ptta_stream s_) {
    if (!c) return -1;
    NLFWD(c->nl->head_set_hparams(lr, beta1, beta2, eps, weight_decay, tau, adam_step, (hipStream_t)s_));
    RUN(head_init(c));
    hipStream_t s = (hipStream_t)s_;
    const float hy[5] = {lr, beta1, beta2, eps, weight_decay};
    RUN(ptta_launch_set_floats(c->head.hyper, hy, 5, s));
    const float t2[2] = {tau, (float)(1.0 - (double)tau)};
    RUN(ptta_launch_set_floats(c->head.tau2, t2, 2, s));
    if (adam_step >= 0) RUN(ptta_launch_set_int(c->head.step, adam_step, s));
    return 0;
}

int ptta_head_reload(ptta_handle c, ptta_stream s) {
    if (!c) return -1;
    NLFWD(c->nl->head_reload((hipStream_t)s));
    RUN(head_init(c));
    c->drop_graphs();
    for (int k = 0; k < 12; ++k) RUN(head_reload(c, k, (hipStream_t)s));
    return 0;
}

int ptta_head_forward(ptta_handle c, const float* image, const float* sparse, int reverse, float* emb_out, float* ref_out, ptta_stream s_) {
    if (!c || !image || !sparse) return -1;
    NLFWD(c->nl->head_forward(image, sparse, reverse, emb_out, ref_out, (hipStream_t)s_));
    RUN(head_init(c));
    auto& h = c->head;
    hipStream_t s = (hipStream_t)s_;
    if (c->stat_sync.world > 1 && h.form != PTTA_HEAD_FORM_SYNCBN) return c->fail("the plain form of the stage-2 head trainer has no SyncBatchNorm exchange (ptta_head_set_form)", -38);
    for (int k = (reverse ? 6 : 0); k < 12; ++k) if (!h.prm[k].p) return c->fail(std::string("head parameter not bound: ") + HEAD_NAMES[k], -3);
    h.stepped = true;
    // _update_head(): proj_t <- tau proj_t + (1 - tau) proj, BEFORE the heads run (network_exp_msg_chn_adapt.py:682,691)
    int nt = 0; for (auto& e : h.tgt) nt += e.p ? 1 : 0;
    if (nt != 0 && nt != 6) return c->fail("bind all six proj_t parameters or none", -3);
    if (nt == 6) {
        if (h.etab_dirty) {
            h.etab_host.resize(6); long off = 0;
            for (int k = 0; k < 6; ++k) {
                if (!h.prm[k].p) return c->fail("the EMA needs the proj parameters bound too", -3);
                h.etab_host[k] = PttaAdamEntry{h.tgt[k].p, nullptr, nullptr, h.prm[k].p, h.tgt[k].n, off}; off += h.tgt[k].n;
            }
            h.etab_total = off;
            HIPCHK(hipMemcpyAsync(h.etab, h.etab_host.data(), 6 * sizeof(PttaAdamEntry), hipMemcpyHostToDevice, s));
            h.etab_dirty = false;
        }
        RUN(ptta_launch_ema_multi(h.etab, 6, h.etab_total, h.tau2, s));
    }
    h.reverse = reverse ? 1 : 0; h.bwd_ok = false;
    c->head_swap = reverse ? 0 : 1; c->skip_dec3 = 1;
    const int rc = ptta_forward_train(c, image, sparse, nullptr, emb_out, ref_out, s_);
    c->head_swap = 0; c->skip_dec3 = 0;
    c->fwd_valid = false;              // no decoder-3 activations: not a forward ptta_backward may follow
    if (rc != 0) return rc;
    h.fwd_ok = true;
    return 0;
}

int ptta_head_backward(ptta_handle c, float* loss_out, ptta_stream s_) {
    if (!c) return -1;
    NLFWD(c->nl->head_backward(loss_out, (hipStream_t)s_));
    auto& h = c->head;
    if (!h.ready || !h.fwd_ok) return c->fail("ptta_head_backward needs the activations of the last ptta_head_forward", -3);
    hipStream_t s = (hipStream_t)s_;
    const long R = c->Rg;
    float* g_emb = c->gref_buf;
    RUN(ptta_launch_prepare_loss(c->emb, c->ref, R, 512, g_emb, h.loss_part, h.loss, s));
    if (loss_out) HIPCHK(hipMemcpyAsync(loss_out, h.loss, 4, hipMemcpyDeviceToDevice, s));
    for (int k = 0; k < 12; ++k) h.has_grad[k] = false;
    auto G = [&](int k) { h.has_grad[k] = true; return h.prm[k].g; };
    // the SyncBatchNorm form with an exchange bound (the forward's mlp_forward exchanges the moments whenever one is)
    const bool sync = h.form == PTTA_HEAD_FORM_SYNCBN && c->stat_sync.on();
    const int world = c->stat_sync.world > 1 ? c->stat_sync.world : 1;
    // one MLP: out = Linear3(relu(BN(Linear0(x)))).  g: d out; hid: pre-BN hidden; x: MLP input (K wide); st_*: BN state of THIS application
    auto mlp_backward = [&](const char* name, int k0, const float* g, const float* hid, const void* x, int K,
                            const float* st_mean, const float* st_inv, const float* st_scale, const float* st_shift, float* dx) -> int {
        const Lin& l0 = c->fc[std::string(name) + ".0"]; const Lin& l3 = c->fc[std::string(name) + ".3"]; BNorm& bn = c->bn[std::string(name) + ".1"];
        LinWgradArgs w3; w3.G = g; w3.X = hid; w3.xscale = st_scale; w3.xshift = st_shift; w3.Wpart = h.wpart; w3.bpart = h.bpart; w3.R = R; w3.O = 512; w3.I = 512;
        RUN(ptta_launch_linear_wgrad(w3, G(k0 + 4), G(k0 + 5), s));
        GemmArgs ga; ga.A = g; ga.W = l3.Wt; ga.C = c->gmask; ga.R = (int)R; ga.K = 512; ga.N = 512; ga.epi = 2;
        ga.eH = hid; ga.escale = st_scale; ga.eshift = st_shift; ga.emean = st_mean; ga.einv = st_inv; ga.part = c->bn_part;
        ga.x3 = c->x3; ga.Whi = l3.Wthi; ga.Wlo = l3.Wtlo; ga.Wil = l3.Wtil;
        RUN(ptta_launch_gemm(ga, s));
        if (sync) {       // SyncBatchNorm backward: the two sums of the GLOBAL batch; d gamma / d beta keep the local share (DDP averages them)
            RUN(ptta_stat_sync(&c->stat_sync, c->bn_part, ptta_gemm_part_blocks(ga), 512, 1, s));
            RUN(ptta_launch_bn_bwd_finalize(c->bn_part, ptta_gemm_part_blocks(ga), (int)R * world, 512, bn.gamma, st_inv, c->bnb_gscale, c->bnb_c1, c->bnb_c2, s,
                                            G(k0 + 2), G(k0 + 3), nullptr, nullptr, nullptr, 1.f / (float)world));
        } else
        RUN(ptta_launch_bn_bwd_finalize(c->bn_part, ptta_gemm_part_blocks(ga), (int)R, 512, bn.gamma, st_inv, c->bnb_gscale, c->bnb_c1, c->bnb_c2, s,
                                        G(k0 + 2), G(k0 + 3)));
        LinWgradArgs w0; w0.G = c->gmask; w0.Gh = hid; w0.gscale = c->bnb_gscale; w0.gc1 = c->bnb_c1; w0.gc2 = c->bnb_c2; w0.gmean = st_mean; w0.ginv = st_inv;
        w0.X = (const float*)x; w0.Wpart = h.wpart; w0.bpart = h.bpart; w0.R = R; w0.O = 512; w0.I = K;
        RUN(ptta_launch_linear_wgrad(w0, G(k0), G(k0 + 1), s));
        if (dx) {
            GemmArgs g2; g2.A = c->gmask; g2.A2 = hid; g2.W = l0.Wt; g2.C = dx; g2.R = (int)R; g2.K = 512; g2.N = K; g2.pro = 2;
            g2.pscale = c->bnb_gscale; g2.pmean = st_mean; g2.pinv = st_inv; g2.pc1 = c->bnb_c1; g2.pc2 = c->bnb_c2;
            g2.x3 = c->x3; g2.Whi = l0.Wthi; g2.Wlo = l0.Wtlo;
            RUN(ptta_launch_gemm(g2, s));
        }
        return 0;
    };
    BNorm& bp = c->bn["pred.1"];
    // pred consumed c->pz in both modes (reverse: proj(feat_zero), otherwise proj(feat))
    RUN(mlp_backward("pred", 6, g_emb, c->h2, c->pz, 512, bp.mean, bp.inv, bp.scale, bp.shift, h.reverse ? nullptr : h.dp));
    if (!h.reverse)       // emb = pred(proj(feat)): continue into proj's first application (its BatchNorm state was saved aside)
        RUN(mlp_backward("proj", 0, h.dp, c->h1, c->feat, 32, h.sv_mean, h.sv_inv, h.sv_scale, h.sv_shift, nullptr));
    h.bwd_ok = true;
    return 0;
}

int ptta_head_adam_step(ptta_handle c, ptta_stream s_) {
    if (!c) return -1;
    NLFWD(c->nl->head_adam_step((hipStream_t)s_));
    auto& h = c->head;
    if (!h.ready || !h.bwd_ok) return c->fail("ptta_head_adam_step needs the gradients of ptta_head_backward", -3);
    hipStream_t s = (hipStream_t)s_;
    const int k0 = h.reverse ? 6 : 0;                         // torch.optim.Adam skips parameters whose .grad is None
    if (h.tab_mode != h.reverse) {
        h.tab_host.clear(); long off = 0;
        for (int k = k0; k < 12; ++k) { auto& e = h.prm[k]; h.tab_host.push_back(PttaAdamEntry{e.p, e.m, e.v, e.g, e.n, off}); off += e.n; }
        h.tab_n = 12 - k0; h.tab_total = off;
        HIPCHK(hipMemcpyAsync(h.tab, h.tab_host.data(), h.tab_host.size() * sizeof(PttaAdamEntry), hipMemcpyHostToDevice, s));
        h.tab_mode = h.reverse;
    }
    if (h.form == PTTA_HEAD_FORM_SYNCBN) {                    // DistributedDataParallel: the mean of the head gradients over the ranks, ONE message
        if (c->grad_comm) { if (ptta_rccl_allreduce_mean_f32(c->grad_comm, h.garena, h.garena_n, s_)) return c->fail(std::string("head gradient all-reduce: ") + ptta_rccl_last_error(), -5); }
        else if (c->stat_sync.on() && c->stat_sync.world > 1) RUN(ptta_grad_mean_sync(&c->stat_sync, h.garena, h.garena_n, s));      // the exchange's callback or communicator
    }
    RUN(ptta_launch_adam_multi(h.tab, h.tab_n, h.tab_total, h.hyper, h.step, h.ticket, s));
    c->drop_graphs();                                         // the TTA graph holds no head weights by value, but stay conservative
    for (int k = k0; k < 12; ++k) RUN(head_reload(c, k, s));
    h.bwd_ok = false;
    return 0;
}

int ptta_head_step(ptta_handle c, const float* image, const float* sparse, int reverse, float* loss_out, ptta_stream s) {
    if (c && c->nl) {
        c->err.clear();
        int rc = c->nl->head_forward(image, sparse, reverse, nullptr, nullptr, (hipStream_t)s);
        if (!rc) rc = c->nl->head_backward(loss_out, (hipStream_t)s);
        return rc ? rc : c->nl->head_adam_step((hipStream_t)s);
    }
    RUN(ptta_head_forward(c, image, sparse, reverse, nullptr, nullptr, s));
    RUN(ptta_head_backward(c, loss_out, s));
    return ptta_head_adam_step(c, s);
}

int ptta_head_get_grad(ptta_handle c, const char* name, float* dst, int64_t capacity, int* has_grad_host, ptta_stream s) {
    if (!c || !name) return -1;
    NLFWD(c->nl->head_get_grad(name, dst, capacity, has_grad_host, (hipStream_t)s));
    auto& h = c->head;
    if (!h.ready) return c->fail("no head parameter bound", -3);
    for (int k = 0; k < 12; ++k) if (h.prm[k].name == name) {
        if (has_grad_host) *has_grad_host = h.has_grad[k] ? 1 : 0;
        if (dst && h.has_grad[k]) {
            if (capacity < h.prm[k].n) return c->fail("capacity too small", -22);
            HIPCHK(hipMemcpyAsync(dst, h.prm[k].g, (size_t)h.prm[k].n * 4, hipMemcpyDeviceToDevice, (hipStream_t)s));
        }
        return 0;
    }
    return c->fail(std::string("not a trainable head parameter: ") + name, -2);
}

int ptta_set_image_norm(ptta_handle c, float divisor, const float* mean, const float* stdv) {
    NLFWD(c->nl->set_image_norm(divisor, mean, stdv));

    if (!c) return -1;
    if (!(divisor > 0.f)) return c->fail("ptta_set_image_norm: divisor must be positive", -22);
    ImgNorm nm = ImgNorm{0, divisor, {0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}};
    for (int k = 0; k < 3; ++k) {
        if (mean) nm.mean[k] = mean[k];
        if (stdv) { if (!(stdv[k] > 0.f)) return c->fail("ptta_set_image_norm: std must be positive", -22); nm.stdv[k] = stdv[k]; }
    }
    nm.on = !(divisor == 1.f && nm.mean[0] == 0.f && nm.mean[1] == 0.f && nm.mean[2] == 0.f && nm.stdv[0] == 1.f &&
              nm.stdv[1] == 1.f && nm.stdv[2] == 1.f);
    c->img_norm = nm;
    c->drop_graphs();          // the constants are kernel arguments of the captured launches
    return 0;
}

int ptta_set_stat_sync(ptta_handle c, ptta_allreduce_fn fn, void* user, double* exchange_buf, int64_t capacity, int world_size) {
    if (!c || world_size < 1 || (world_size > 1 && (!fn || !exchange_buf || capacity < 2 * 1024))) return -22;
    PttaStatSync sy; sy.fn = (ptta_allreduce_cb)fn; sy.user = user; sy.buf = exchange_buf; sy.cap = (long)capacity; sy.world = world_size;
    if (c->nl) { c->err.clear(); c->nl->drop_graphs(); c->nl->stat_sync = sy; return 0; }
    if (world_size > 1 && c->meta_mode == PTTA_META_2LAYERS && !c->m2.generic) return c->fail("SyncBatchNorm needs the default arithmetic for the 2layers meta layer", -38);
    c->stat_sync = sy;
    c->drop_graphs();
    if (world_size > 1) {               // the step contains host-driven collectives: no graph replay, one stream
        if (c->pre_sync_graph < 0) { c->pre_sync_graph = c->use_graph; c->pre_sync_aux = c->use_aux; }
        c->use_graph = 0; c->use_aux = 0;
    } else if (c->pre_sync_graph >= 0) {     // exchange switched off again: back to the replayed, two-stream step
        c->use_graph = c->pre_sync_graph; c->use_aux = c->pre_sync_aux; c->pre_sync_graph = c->pre_sync_aux = -1;
    }
    return 0;
}

// The same exchange on the library's own RCCL communicator (rccl_sync.hip): the collectives are enqueued by the library on the
// step's stream, so they are captured into the step's hipGraph like any kernel -- graph replay stays on; only the second stream
// is given up (collectives of one communicator are kept in one stream order).  comm == NULL or world_size == 1 with comm == NULL: off.
int ptta_set_stat_sync_rccl(ptta_handle c, void* comm, double* exchange_buf, int64_t capacity, int world_size) {
    if (!c || world_size < 1 || (comm && (!exchange_buf || capacity < 2 * 1024))) return -22;
    PttaStatSync sy; sy.comm = comm; sy.buf = exchange_buf; sy.cap = (long)capacity; sy.world = world_size;
    if (c->nl) { c->err.clear(); c->nl->drop_graphs(); c->nl->stat_sync = sy; return 0; }
    if (comm && c->meta_mode == PTTA_META_2LAYERS && !c->m2.generic) return c->fail("SyncBatchNorm needs the default arithmetic for the 2layers meta layer", -38);
    c->stat_sync = sy;
    c->drop_graphs();
    if (comm) {
        if (c->pre_sync_graph < 0) { c->pre_sync_graph = c->use_graph; c->pre_sync_aux = c->use_aux; }
        else c->use_graph = c->pre_sync_graph;         // coming from the callback mode: the graph is available again
        c->use_aux = 0;
    } else if (c->pre_sync_graph >= 0) {
        c->use_graph = c->pre_sync_graph; c->use_aux = c->pre_sync_aux; c->pre_sync_graph = c->pre_sync_aux = -1;
    }
    return 0;
}

// DistributedDataParallel's gradient averaging (src/msg_chn_model_adapt.py:476-480) for the fused ptta_step: between backward and
// Adam the adapted gradients (one arena: 37 KB for MSG_CHN 1layer) are averaged over the communicator's ranks with ONE
// ncclAllReduce enqueued on the step's stream (captured into the hipGraph).  comm == NULL: off.
int ptta_set_grad_sync_rccl(ptta_handle c, void* comm) {
    if (!c) return -1;
    if (c->nl) { c->nl->drop_graphs(); c->nl->grad_comm = comm; return 0; }
    c->grad_comm = comm;
    c->drop_graphs();
    return 0;
}

// Per-handle switches (include/ptta.h documents the keys).  The defaults are the shipped step; every other value is a correct,
// slower form kept for validation (tests/test_gpu_options.py: bit-identical to the default unless noted) or as the fallback a
// configuration takes by itself (small maps, SyncBatchNorm exchange, N > 16).
int ptta_set_option(ptta_handle c, const char* key, int value) {
    if (!c || !key) return -1;
    const std::string k(key);
    if (k == "graph") return ptta_set_graph(c, value);
    if (c->nl) return -38;                         // the generic engine has the one switch
    int* f = nullptr; int lo = 0, hi = 1;
    if (k == "aux_stream") f = &c->use_aux;
    else if (k == "thru") f = &c->thru;
    else if (k == "adam_in_wgrad") f = &c->adam_in_wgrad;
    else if (k == "bwd_w2") f = &c->bwd_w2;
    else if (k == "fuse_first") { f = &c->fuse_first; hi = 2; }
    else if (k == "fuse_head_bwd") f = &c->fuse_head_bwd;
    else if (k == "fuse_heads") f = &c->fuse_heads;
    else if (k == "heads_v2") f = &c->heads_v2;
    else if (k == "cos_in_gemm") f = &c->cos_grad_fused;
    else if (k == "mask_bits") f = &c->mask_bits_on;
    else if (k == "stamps") f = &c->stamps;
    else return c->fail("ptta_set_option: unknown key '" + k + "'", -22);
    if (value < lo || value > hi) return c->fail("ptta_set_option: value out of range for '" + k + "'", -22);
    if (c->mixed && k != "aux_stream" && k != "thru" && k != "adam_in_wgrad" && k != "bwd_w2" && k != "stamps" && value != 1)
        return c->fail("ptta_set_option: the mixed mode is defined on the default kernels ('" + k + "' stays 1)", -38);
    if (k == "aux_stream" && c->pre_sync_graph >= 0) { c->pre_sync_aux = value; return 0; }      // statistics exchange active: takes effect when it ends
    if (*f == value) return 0;
    RUN(pipe_quiesce(c));
    c->drop_graphs();
    *f = value;
    return 0;
}

int ptta_get_option(ptta_handle c, const char* key, int* value) {
    if (!c || !key || !value) return -1;
    const std::string k(key);
    // read-only: 1 when ptta_step_pipelined would run as itself on this handle as it is configured now, 0 when it degrades to ptta_step
    // call by call (generic-engine backbones, the dual-corner padded path, a statistics exchange or gradient communicator bound, validation
    // arithmetic, the profiling leg)
    if (k == "pipelined_active") { *value = !(c->nl || c->prof_on || c->dual || c->stat_sync.on() || c->grad_comm || c->naive || c->bf16); return 0; }
    // read-only: 1 when the step takes the two-stream `thru` schedule (loss gradient from the valid-weight partials), as far as it can be known
    // without the caller's stream (the second stream is created on first use)
    if (k == "thru_active") { *value = c->nl ? 0 : (c->thru && c->cos_grad_fused && heads_v2_on(c) && c->use_aux); return 0; }
    if (c->nl) { if (k != "graph") return -38; *value = c->nl->use_graph; return 0; }
    if (k == "graph") *value = c->use_graph;
    else if (k == "aux_stream") *value = c->use_aux;
    else if (k == "thru") *value = c->thru;
    else if (k == "adam_in_wgrad") *value = c->adam_in_wgrad;
    else if (k == "bwd_w2") *value = c->bwd_w2;
    else if (k == "fuse_first") *value = c->fuse_first;
    else if (k == "fuse_head_bwd") *value = c->fuse_head_bwd;
    else if (k == "fuse_heads") *value = c->fuse_heads;
    else if (k == "heads_v2") *value = c->heads_v2;
    else if (k == "cos_in_gemm") *value = c->cos_grad_fused;
    else if (k == "mask_bits") *value = c->mask_bits_on;
    else if (k == "stamps") *value = c->stamps;
    else return -22;
    return 0;
}

int ptta_set_graph(ptta_handle c, int enable) {
    if (c && c->nl) { c->nl->use_graph = enable ? 1 : 0; if (!enable) c->nl->drop_graphs(); return 0; }

    if (!c) return -1;
    if (enable && c->stat_sync.on() && !c->stat_sync.comm) return c->fail("graph replay is not available with SyncBatchNorm exchange (ptta_set_stat_sync)", -38);
    c->use_graph = enable ? 1 : 0;
    if (!enable) c->drop_graphs();
    return 0;
}

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

int ptta_profile(ptta_handle c, int enable) {
    if (c && c->nl) return c->fail("not available for the NLSPN / CostDCNet backbones: use ptta_step / ptta_forward_*", -38);

    if (!c) return -1;
    c->prof_on = enable != 0;
    for (auto& pc : c->prof) { pc.used = 0; pc.bytes = 0; pc.macs = 0; pc.launches = 0; }
    c->prof_seq.clear();
    return 0;
}

int ptta_profile_read(ptta_handle c, int klass, double* ms_total, double* alg_bytes, double* macs, int64_t* launches, ptta_stream s_) {
    if (c && c->nl) return c->fail("not available for the NLSPN / CostDCNet backbones: use ptta_step / ptta_forward_*", -38);

    if (!c || klass < 0 || klass >= ptta_ctx::NPROF) return -1;
    HIPCHK(hipStreamSynchronize((hipStream_t)s_));
    ptta_ctx::ProfClass& pc = c->prof[klass];
    double ms = 0;
    for (size_t k = 0; k < pc.used; ++k) {
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, pc.ev[k].first, pc.ev[k].second));
        ms += t;
    }
    if (ms_total) *ms_total = ms;
    if (alg_bytes) *alg_bytes = pc.bytes;
    if (macs) *macs = pc.macs;
    if (launches) *launches = (int64_t)pc.launches;
    return 0;
}

int ptta_debug_tensor(ptta_handle c, const char* name, float* dst, int64_t capacity, int64_t* numel_host, ptta_stream s_) {
    NLFWD(c->nl->debug_tensor(name, dst, capacity, numel_host, (hipStream_t)s_));

    if (!c || !name) return -1;
    if (std::string(name) == "prof_seq") {
        // the profiling leg's bracketed launches in launch order: [class, microseconds] pairs (tools/tail_launches.py)
        HIPCHK(hipStreamSynchronize((hipStream_t)s_));
        const int64_t n = 2 * (int64_t)c->prof_seq.size();
        if (numel_host) *numel_host = n;
        if (!dst) return 0;
        if (capacity < n) return c->fail("capacity too small", -22);
        std::vector<float> h((size_t)n);
        for (size_t k = 0; k < c->prof_seq.size(); ++k) {
            const auto& q = c->prof_seq[k];
            float t = 0.f;
            HIPCHK(hipEventElapsedTime(&t, c->prof[q.first].ev[q.second].first, c->prof[q.first].ev[q.second].second));
            h[2 * k] = (float)q.first; h[2 * k + 1] = 1e3f * t;
        }
        HIPCHK(hipMemcpy(dst, h.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        return 0;
    }
    auto it = c->dbg.find(name);
    if (it == c->dbg.end()) return c->fail(std::string("no debug tensor ") + name, -2);
    if (numel_host) *numel_host = it->second.numel;
    if (!dst) return 0;
    if (capacity < it->second.numel) return c->fail("capacity too small", -22);
    hipStream_t s = (hipStream_t)s_;
    const long n = it->second.numel;
    if (it->second.is_act == 3) RUN(ptta_launch_hn_untile(it->second.p, dst, n / 512, s));
    else if ((it->second.is_act == 1 && c->bf16) || it->second.is_act == 2) hipLaunchKernelGGL((to_f32_kernel<bf16_t>), dim3(nblk(n)), dim3(256), 0, s, (const bf16_t*)it->second.p, dst, n);
    else HIPCHK(hipMemcpyAsync(dst, it->second.p, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

// Stand-alone 32->32 3x3 convolution on fp32 NHWC buffers (tests only): packs `weight`, converts
// to the requested storage type, runs the hot-path kernel and converts back.
int ptta_op_conv32(const float* in, const float* weight, const float* bias, float* out, int b, int hin, int win, int mode,
                   int relu_in, int in_major, int flip, int dtype, int naive, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    ConvW w{};
    void *tin = nullptr, *tout = nullptr;
    const int ho = mode == CONV_S1 ? hin : (mode == CONV_S2 ? hin / 2 : hin * 2), wo = mode == CONV_S1 ? win : (mode == CONV_S2 ? win / 2 : win * 2);
    const long nin = (long)b * hin * win * 32, nout = (long)b * ho * wo * 32;
    int rc = 0;
    if (hipMalloc((void**)&w.mf32, 9 * 4 * 64 * 4 * 4) != hipSuccess || hipMalloc((void**)&w.mbf16, 9 * 2 * 64 * 8 * 2) != hipSuccess ||
        hipMalloc((void**)&w.canon, 9216 * 4) != hipSuccess || hipMalloc((void**)&w.mlo, 9 * 2 * 64 * 8 * 2) != hipSuccess || hipMalloc(&tin, nin * 2) != hipSuccess || hipMalloc(&tout, nout * 2) != hipSuccess)
        rc = -12;
    if (rc == 0) {
        ptta_pack_conv32(weight, w, in_major, flip, s);
        Conv32Args a; a.w = &w; a.bias = bias; a.B = b; a.Hin = hin; a.Win = win; a.mode = mode; a.relu_in = relu_in; a.naive = naive & 1; a.x3 = (naive >> 1) & 1;
        if (dtype != PTTA_DTYPE_F32) {             // narrow storage (bf16 maps, one MFMA per product): the kernels of the mixed mode
            hipLaunchKernelGGL((from_f32_kernel<bf16_t>), dim3(nblk(nin)), dim3(256), 0, s, in, (bf16_t*)tin, nin);
            a.in = tin; a.in_nb = b; a.out_raw = tout; a.bf16 = 1;
            rc = ptta_launch_conv32(a, s);
            hipLaunchKernelGGL((to_f32_kernel<bf16_t>), dim3(nblk(nout)), dim3(256), 0, s, (const bf16_t*)tout, out, nout);
        } else {
            a.in = in; a.in_nb = b; a.out_raw = out; a.bf16 = 0;
            rc = ptta_launch_conv32(a, s);
        }
        (void)hipStreamSynchronize(s);
    }
    (void)hipFree(w.mf32); (void)hipFree(w.mbf16); (void)hipFree(w.mlo); (void)hipFree(w.canon); (void)hipFree(tin); (void)hipFree(tout);
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
    ConvW wv{};
    if (hipMalloc((void**)&wv.mf32, 9 * 4 * 64 * 4 * 4) != hipSuccess || hipMalloc((void**)&wv.mbf16, 9 * 2 * 64 * 8 * 2) != hipSuccess ||
        hipMalloc((void**)&wv.canon, 9216 * 4) != hipSuccess || hipMalloc((void**)&wv.mlo, 9 * 2 * 64 * 8 * 2) != hipSuccess) return -12;
    ptta_pack_conv32(weight, wv, 0, 0, s);
    (void)hipStreamSynchronize(s);
    if (epi_flags & 16) {                  // the layer loop: `reps` dependent layers per LAUNCH, a device-wide barrier between layers (conv32.hip)
        hipEvent_t d0 = nullptr, d1 = nullptr;
        unsigned* ctr = nullptr; int* err = nullptr;
        if (hipEventCreate(&d0) != hipSuccess || hipEventCreate(&d1) != hipSuccess) return -5;
        if (hipMalloc((void**)&ctr, 256) != hipSuccess) return -12;
        err = (int*)(ctr + 32);
        (void)hipMemsetAsync(ctr, 0, 256, s);
        unsigned base = 0;
        int rcd = 0;
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
        (void)hipEventDestroy(d0); (void)hipEventDestroy(d1); (void)hipFree(ctr);
        (void)hipFree(wv.mf32); (void)hipFree(wv.mbf16); (void)hipFree(wv.mlo); (void)hipFree(wv.canon);
        return rcd;
    }
    if (epi_flags & 8) {                   // the same chain launched directly (no graph): what a dependent launch costs in the default form
        hipEvent_t d0 = nullptr, d1 = nullptr;
        if (hipEventCreate(&d0) != hipSuccess || hipEventCreate(&d1) != hipSuccess) return -5;
        int rcd = 0;
        for (int k = 0; k < replays + 2 && !rcd; ++k) {
            if (k == 2) (void)hipEventRecord(d0, s);
            for (int r = 0; r < reps && !rcd; ++r) {
                Conv32Args a; a.w = &wv; a.bias = bias; a.B = b; a.Hin = h; a.Win = w; a.mode = CONV_S1; a.relu_in = relu_in; a.x3 = 1;
                a.in = r == 0 ? in : ((r & 1) ? buf_a : buf_b); a.in_nb = b; a.out_raw = (r & 1) ? buf_b : buf_a;
                if ((epi_flags & 2) && aux) { a.mask = aux; a.mask_nb = b; }
                if ((epi_flags & 4) && aux) { a.add1 = aux; a.add1_nb = b; }
                rcd = ptta_launch_conv32(a, s);
            }
        }
        (void)hipEventRecord(d1, s); (void)hipStreamSynchronize(s);
        float ms = 0.f; (void)hipEventElapsedTime(&ms, d0, d1);
        *us_per_launch_host = 1e3f * ms / ((float)replays * (float)reps);
        (void)hipEventDestroy(d0); (void)hipEventDestroy(d1);
        (void)hipFree(wv.mf32); (void)hipFree(wv.mbf16); (void)hipFree(wv.mlo); (void)hipFree(wv.canon);
        return rcd;
    }
    hipStream_t cs = nullptr; hipGraph_t g = nullptr; hipGraphExec_t ge = nullptr; hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = 0;
    if (hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess) rc = -5;
    if (!rc && hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) != hipSuccess) rc = -5;
    if (!rc) {
        for (int r = 0; r < reps && !rc; ++r) {
            Conv32Args a; a.w = &wv; a.bias = bias; a.B = b; a.Hin = h; a.Win = w; a.mode = CONV_S1; a.relu_in = relu_in; a.x3 = 1;
            a.in = r == 0 ? in : ((r & 1) ? buf_a : buf_b); a.in_nb = b; a.out_raw = (r & 1) ? buf_b : buf_a;
            if ((epi_flags & 2) && aux) { a.mask = aux; a.mask_nb = b; }
            if ((epi_flags & 4) && aux) { a.add1 = aux; a.add1_nb = b; }
            rc = ptta_launch_conv32(a, cs);
        }
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
    (void)hipFree(wv.mf32); (void)hipFree(wv.mbf16); (void)hipFree(wv.mlo); (void)hipFree(wv.canon);
    return rc;
}

}  // extern "C"
