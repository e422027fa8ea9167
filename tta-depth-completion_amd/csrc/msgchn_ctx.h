// The MSG_CHN handle (struct ptta_ctx), its helper structs and macros, and the declarations of the functions that cross the
// translation units it is built from (msgchn_*.hip, ptta_api.hip, ptta_ops.hip).  Private to csrc/: declarations only.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/ptta.h"
#include "ptta_common.h"
#include "ptta_kernels.h"
#include "nlspn.h"

#pragma GCC visibility push(hidden)          // everything declared here is internal to libptta_hip.so

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return c->fail(std::string(#x) + ": " + hipGetErrorString(e_), -100 - (int)e_); } while (0)
// (the message keeps the chain of failing calls: "outer failed <- inner failed <- reason")
#define RUN(x) do { int r_ = (x); if (r_ != 0) return c->fail_chain(std::string(#x) + " failed", r_ < 0 ? r_ : -r_); } while (0)

// calls forwarded to a GNet engine clear the wrapper-level message, so the engine's later message is not masked by a stale one
#define NLFWD(call) do { if (c && c->nl) { c->err.clear(); return (call); } } while (0)

// the source-model handle (include/ptta.h PTTA_MSGCHN_PLAIN) has the eval forward only: what it refuses, in the words of the other two
// backbones' source handles
#define PLAIN_NO_TRAIN(what) do { if (c && !c->nl && c->plain) return c->fail(std::string(what) + ": the source model (PTTA_MSGCHN_PLAIN) adapts nothing: it has the eval forward only", -38); } while (0)
#define PLAIN_NO_HEADS(what) do { if (c && !c->nl && c->plain) return c->fail(std::string(what) + ": PTTA_MSGCHN_PLAIN: this handle runs the network without the meta layer and has no heads (no stage-2 head trainer)", -38); } while (0)
#define PLAIN_ONE_RANK(what) do { if (c && !c->nl && c->plain) return c->fail(std::string(what) + ": PTTA_MSGCHN_PLAIN: more than one rank is not offered (no statistics or gradient exchange)", -38); } while (0)

struct ImgNorm { int on; float div; float mean[3]; float stdv[3]; };

// ---- the small utility kernels (msgchn_kernels.hip) behind host functions: each kernel is compiled once ----
namespace msgchn {
hipError_t d2d_copy(void* dst, const void* src, size_t bytes, hipStream_t s);
void stamp_launch(float* out, unsigned long long* base, int i, hipStream_t s);
void transpose_launch(const float* src, float* dst, int rows, int cols, hipStream_t s);
void pad_dual_launch(const float* src, float* dst, int N, int C, int H, int W, int Hp, int Wp, int pt, int pr, hipStream_t s,
                     ImgNorm nm = ImgNorm{0, 1.f, {0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}});
void crop_avg_launch(const float* net, float* out, int N, int H, int W, int Hp, int Wp, int pt, int pr, hipStream_t s);
void scatter_dual_grad_launch(const float* g, float* gnet, int N, int H, int W, int Hp, int Wp, int pt, int pr, hipStream_t s);
void to_f32_launch(const bf16_t* src, float* dst, long n, hipStream_t s);
void from_f32_launch(const float* src, bf16_t* dst, long n, hipStream_t s);
void fuse_linear_launch(const float* Wb, const float* bb, const float* Wa, const float* ba, float* W, float* bias, int N, int M, int K, hipStream_t s);
}  // namespace msgchn

// events that order the handle's own streams among themselves (fork / join inside a step, prefix -> step): no timing, no system-scope fence --
// nothing the host or another device reads is published by them (ev_replay, which the host waits on before it destroys a graph, keeps the default)
static constexpr unsigned kStepEvent = hipEventDisableTiming | hipEventDisableSystemFence;
struct L32 { ConvW f{}, b{}; float* bias = nullptr; int transposed = 0; };
struct LIn { float *wfrag = nullptr, *wcanon = nullptr, *bias = nullptr, *bw = nullptr; int cin = 1; };
struct LOut { float *w = nullptr, *bias = nullptr, *bfrag = nullptr, *bcanon = nullptr; };
struct Lin { float *W = nullptr, *Wt = nullptr, *bias = nullptr; bf16_t *Whi = nullptr, *Wlo = nullptr, *Wthi = nullptr, *Wtlo = nullptr, *Wil = nullptr, *Wtil = nullptr;
             bf16_t *Wsl = nullptr, *Wtsl = nullptr;      // slice-major bf16 images of W / W^T for the narrow heads (heads_n.hip), 512 x 512 layers
             int N = 0, K = 0; };
struct BNorm { float *gamma = nullptr, *beta = nullptr, *rm = nullptr, *rv = nullptr; long long* nbt = nullptr;
               float *mean = nullptr, *inv = nullptr, *scale = nullptr, *shift = nullptr; };
struct Dbg { const void* p; long numel; int is_act; };

// The buffers frame pipelining holds twice (ptta_ctx::PreSet): the outputs of everything upstream of the adapted layer and the staged inputs.
// The handle's launches read them as its own members; a set is swapped in or out by one assignment of this struct (msgchn_step.hip).
struct PrefixBufs {
    void *c0 = nullptr, *c1 = nullptr, *c2 = nullptr, *c3 = nullptr, *c4 = nullptr, *e1_0a = nullptr, *e1_0 = nullptr, *e1_1a = nullptr;
    void *c0a = nullptr, *c1a = nullptr, *c2a = nullptr, *c3a = nullptr, *c4a = nullptr;     // the RGB encoder's intermediates: a prefix on pre_stream writes them too
    void *e1_1 = nullptr, *y1 = nullptr, *e1_2a = nullptr, *y2 = nullptr, *t1 = nullptr, *y3 = nullptr, *s1_1 = nullptr, *u1 = nullptr;
    float *dclamp = nullptr, *d12 = nullptr, *d14 = nullptr, *in_image = nullptr, *in_loss_image = nullptr, *in_sparse = nullptr, *in_validity = nullptr;
    bool proxy_valid = false;       // proxy half of c0..c4 holds the zero-image encoder outputs for the current weights
};

struct ptta_ctx : PrefixBufs {
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
    // the source model (include/ptta.h PTTA_MSGCHN_PLAIN): no meta layer (its three readers take c2), one pass, no heads; eval forward only
    int plain = 0;
    void* meta_out() const { return plain ? c2 : m; }       // what depth_decoder1.dec1.3, depth_decoder2.dec2.3 and depth_encoder3.enc2.3 add
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
    void stamp(int i, hipStream_t s) { if (stamps) msgchn::stamp_launch(stamp_f, stamp_base, i, s); }
    PttaAdamEntry* adam_tab = nullptr; unsigned* adam_ticket = nullptr; bool adam_tab_dirty = true;
    std::vector<PttaAdamEntry> adam_host;        // stays alive: the upload reads it
    bool fwd_valid = false;
    PttaStatSync stat_sync;          // SyncBatchNorm exchange across ranks (ptta_set_stat_sync); world == 1: off
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
    int pair_fuse = 1;               // option "pair_fuse": each small-map stride-2 -> stride-1 layer pair as one launch (conv_pair.hip)
    int pair_fuse_count = 0;         // fused pair launches issued by the last step (read-only option "pair_fuse_count")
    int tpair_fuse = 1;              // option "tpair_fuse": each transposed -> stride-1 layer pair of the forward as one launch (conv_tpair.hip)
    int tpair_fuse_count = 0;        // fused transposed-pair launches issued by the last step (read-only option "tpair_fuse_count")
    std::unordered_set<const void*> tpair_unwritten;     // intermediate maps the last fused launches did NOT write (ptta_debug_tensor refuses them)
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
    struct PreSet : PrefixBufs {
        bool prepared = false, rest_recorded = false;
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
    float *out1, *p12, *q, *p11, *depth_net, *depth_final, *validity_tmp;
    void *m, *y4, *s0_1, *v1;              // (c0 .. c4, e1_*, y1 .. y3, t1, s1_1, u1: PrefixBufs)
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
#define REST_(s_, call) do { ProfScope ps_(c, 8, (s_), 0, 0, 1); RUN(call); } while (0)
#define CV(...) RUN(conv32(c, s, __VA_ARGS__))

struct E { const void* up = nullptr; int up_nb = 1; const void* mask = nullptr; int mask_nb = 1;
           const void* add1 = nullptr; int add1_nb = 1; const void* add2 = nullptr; int add2_nb = 1;
           void* raw = nullptr; void* sum = nullptr;
           bool nar = false; };      // nar: a launch over NARROW maps (mixed mode: the proxy chain; every backward launch is one anyway)

inline float* st_ptr(float* base, int C, int pass, int kind) { return base + ((size_t)pass * 4 + kind) * C; }   // kind: 0 mean 1 inv 2 scale 3 shift

namespace msgchn {
// msgchn_build.hip
int pad16(int n);
void build_registry(ptta_ctx* c);
void build_workspace(ptta_ctx* c);
int load_weight(ptta_ctx* c, const std::string& name, const void* tensor, const int64_t* shape, int ndim, hipStream_t s);
// msgchn_forward.hip
int conv_in_p(ptta_ctx* c, const ConvInArgs& a_, hipStream_t s);
int conv_out1_p(ptta_ctx* c, const ConvOut1Args& a, hipStream_t s);
int conv32(ptta_ctx* c, hipStream_t s, const std::string& layer, bool bwd, int mode, const void* in, int in_nb,
           int B, int Hin, int Win, bool relu, const E& e);
int conv32_pair(ptta_ctx* c, hipStream_t s, bool bwd, const std::string& first, const void* in, int in_nb, int B, int Hin, int Win, const E& fe,
                const std::string& second, int mid_nb, const E& se);
int conv32_tpair(ptta_ctx* c, hipStream_t s, bool bwd, const std::string& first, const void* in, int in_nb, int B, int Hin, int Win, const E& fe,
                 const std::string& second, int mid_nb, const E& se);
bool conv32_tpair_takes(ptta_ctx* c, bool bwd, const std::string& first, const void* in, int in_nb, int B, int Hin, int Win, const E& fe,
                        const std::string& second, int mid_nb, const E& se);
int conv32w(ptta_ctx* c, hipStream_t s, const ConvW* w, const float* bias, const void* in, int in_nb, int B, int H, int W, const E& e);
int conv32_first_bwd(ptta_ctx* c, hipStream_t s, const std::string& layer, ConvInArgs& f, int B, int H, int W, const E& e);
int to_narrow(ptta_ctx* c, const void* src_f32, void* dst, long n, hipStream_t s);
int to_wide(ptta_ctx* c, const void* src_nar, float* dst, long n, hipStream_t s);
int rgb_encoder(ptta_ctx* c, const float* image, int nb, int boff, int zero_from_b, hipStream_t s);
int ensure_fused_heads(ptta_ctx* c, hipStream_t s);
int ensure_proxy_rgb(ptta_ctx* c, const float* any_image, hipStream_t s);
int enc1_head_fn(ptta_ctx* c, hipStream_t st);
int stage1_independent(ptta_ctx* c, int B2, hipStream_t s);
bool heads_v2_on(const ptta_ctx* c);
int heads_forward(ptta_ctx* c, hipStream_t s, int part = 0);
int push_hparams(ptta_ctx* c, hipStream_t s);
int forward_common(ptta_ctx* c, const float* image, const float* sparse, bool train, hipStream_t s);
const float* final_depth(ptta_ctx* c);
// msgchn_backward.hip
int heads_backward(ptta_ctx* c, const float* gref, hipStream_t s);
int backbone_backward(ptta_ctx* c, const float* g_net, hipStream_t s, bool join_aux);
// msgchn_step.hip
void pipe_use(ptta_ctx* c, int p);
void pipe_overwritten(ptta_ctx* c, int p);
int pipe_quiesce(ptta_ctx* c);
// ptta_api.hip
int ensure_adam_table(ptta_ctx* c, hipStream_t s);
}  // namespace msgchn
#pragma GCC visibility pop
