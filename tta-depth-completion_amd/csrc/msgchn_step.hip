// The fused MSG_CHN step (forward + loss + backward + gradient all-reduce + Adam in one call: ptta_step) and frame
// pipelining (ptta_step_pipelined: the parameter-independent prefix of the next frame beside the current frame's step).
#include "msgchn_ctx.h"

using namespace msgchn;

namespace msgchn {

// ---- frame pipelining -------------------------------------------------------------------------------------------------------
// a full forward (ptta_forward_eval / ptta_forward_train) has written an arbitrary frame's prefix into set p: whatever was prepared into it
// or adapted from it is gone.  (Set p is pipe_last; when a prefix of the SAME frame was kept there for another step -- inner_iter > 1 --
// the step that follows recomputes it in line.)
void pipe_overwritten(ptta_ctx* c, int p) {
    ptta_ctx::PreSet& P = c->pset[p];
    if (c->pipe_cur == p) { P.prepared = false; P.prep_token = 0; }
    P.last_token = 0;
}

static void pipe_save(ptta_ctx* c, ptta_ctx::PreSet& P) { static_cast<PrefixBufs&>(P) = *c; }
void pipe_use(ptta_ctx* c, int p) {
    if (p == c->cur_set) return;
    pipe_save(c, c->pset[c->cur_set]);
    static_cast<PrefixBufs&>(*c) = c->pset[p];
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
int pipe_quiesce(ptta_ctx* c) {
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

}  // namespace msgchn

// loss + backward + (gradient all-reduce) + Adam: everything of the step behind the forward
static int step_tail(ptta_handle c, const float* loss_image, const float* sparse, const float* validity, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    // shared-parameter run (the reference's DDP, src/tta_main.py:354,631-633): mean of the adapted gradients over the ranks, one message;
    // then Adam, unless the weight gradient's reduction applied it (stamp9: the thru branch's stamp between the two)
    auto sync_and_adam = [&](bool stamp9) -> int {
        if (c->grad_comm && ptta_rccl_allreduce_mean_f32(c->grad_comm, c->grad_arena, c->grad_arena_n, s_)) return c->fail(std::string("gradient all-reduce: ") + ptta_rccl_last_error(), -5);
        if (stamp9) c->stamp(9, s);
        if (!c->adam_fused) RUN(ptta_adam_step(c, nullptr, nullptr, s_));
        return 0;
    };
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
            scatter_dual_grad_launch(c->g_final, c->g_net, c->N, c->H, c->W, c->Hp, c->Wp, c->pt, c->pr, s);
            g_net = c->g_net;
        }
        c->adam_fuse_req = true; c->adam_fused = false;
        const int rc_bb = backbone_backward(c, g_net, s, true);
        c->adam_fuse_req = false;
        if (rc_bb) return rc_bb;
        const int rc_a = sync_and_adam(true);
        if (rc_a) return rc_a;
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
    return sync_and_adam(false);
}

static bool thru_ok(ptta_ctx* c, hipStream_t s) {
    return c->thru && c->cos_grad_fused && heads_v2_on(c) && c->N <= 16 && c->aux(s) != nullptr;
}
static int step_body(ptta_handle c, const float* image, const float* loss_image, const float* sparse, const float* validity,
                     ptta_stream s_) {
    c->pair_fuse_count = 0;                                  // (option "pair_fuse_count": the fused pair launches of this step as enqueued or captured)
    c->tpair_fuse_count = 0;                                 // (option "tpair_fuse_count", likewise)
    RUN(ensure_fused_heads(c, (hipStream_t)s_));             // (before thru_ok: the direct-launch step would otherwise take the joined tail on its first call only)
    c->thru_active = thru_ok(c, (hipStream_t)s_);
    c->cnt_sparse = c->thru_active ? sparse : nullptr; c->cnt_validity = validity;
    const int rc = ptta_forward_train(c, image, sparse, nullptr, nullptr, nullptr, s_);
    if (rc) { c->thru_active = false; c->cnt_sparse = nullptr; return rc; }
    const int rc2 = step_tail(c, loss_image, sparse, validity, s_);
    c->thru_active = false; c->cnt_sparse = nullptr; c->loss_report.on = false;
    return rc2;
}

extern "C" {

int ptta_step(ptta_handle c, const float* image, const float* loss_image, const float* sparse, const float* validity,
              float* depth_out, float* loss_info_out, ptta_stream s_) {
    if (c) c->err_code = 0;
    if (!c || !image || !sparse) return -1;
    if (c->nl) return c->nl->step(image, loss_image, sparse, validity, depth_out, loss_info_out, (hipStream_t)s_);
    PLAIN_NO_TRAIN("ptta_step");
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
        if (!c->gexec[key]) {
            RUN(ensure_proxy_rgb(c, c->in_image, s));        // outside the capture: the graph holds the real-frame encoder only
            RUN(ensure_adam_table(c, s));
            const int rc = pipe_capture(c, &c->graph[key], &c->gexec[key], [&](hipStream_t cs) {
                return step_body(c, c->in_image, (key & 1) ? c->in_loss_image : c->in_image, c->in_sparse, (key & 2) ? c->in_validity : nullptr, (ptta_stream)cs);
            });
            if (rc) return rc;
        }
        HIPCHK(hipGraphLaunch(c->gexec[key], s));
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

// The stream ptta_step_pipelined runs the next frame's prefix on (created on first use): a host that produces that frame asynchronously
// (an H2D copy on its own stream) orders the copy's event on THIS stream instead of delaying the current frame's step with it.
int ptta_pipeline_stream(ptta_handle c, ptta_stream* out) {
    if (!c || !out) return -1;
    if (c->nl) return c->fail("frame pipelining is built for MSG_CHN handles", -38);
    PLAIN_NO_TRAIN("ptta_pipeline_stream");
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
    PLAIN_NO_TRAIN("ptta_step_pipelined");
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
    if (!c->proxy_valid) RUN(ensure_proxy_rgb(c, c->in_image, s));
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
        if (!c->proxy_valid) { HIPCHK(hipStreamSynchronize(ps)); RUN(ensure_proxy_rgb(c, c->in_image, s)); HIPCHK(hipStreamSynchronize(s)); }   // once per set
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

}  // extern "C"
