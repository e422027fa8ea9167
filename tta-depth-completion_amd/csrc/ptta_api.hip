// libptta_hip: the C-ABI of include/ptta.h for an MSG_CHN handle -- life cycle, dispatch to the generic engine (NLSPN,
// CostDCNet), hyper-parameters, weights and bindings, the separate forward / loss / backward / Adam calls, statistics and
// gradient sync, options, the profiling leg and debug tensors.  The handle itself: msgchn_ctx.h; registry and workspace:
// msgchn_build.hip; the launch schedule: msgchn_forward.hip, msgchn_backward.hip; the fused and the pipelined step:
// msgchn_step.hip; the stage-2 head trainer: msgchn_head.hip; entry points without a handle: ptta_ops.hip.
#include "msgchn_ctx.h"

using namespace msgchn;

// pointer table of the adapted tensors for the one-launch Adam; uploaded after ptta_bind_adapted only, never inside a capture
int msgchn::ensure_adam_table(ptta_ctx* c, hipStream_t s) {
    if (!c->adam_tab_dirty) return 0;
    for (auto& ad : c->adapted) if (!ad.p || !ad.m || !ad.v) return 0;          // reported by ptta_adam_step
    c->adam_host.resize(c->adapted.size());
    long off = 0;
    for (size_t k = 0; k < c->adapted.size(); ++k) { auto& ad = c->adapted[k]; c->adam_host[k] = PttaAdamEntry{ad.p, ad.m, ad.v, ad.g, ad.n, off}; off += ad.n; }
    HIPCHK(hipMemcpyAsync(c->adam_tab, c->adam_host.data(), c->adam_host.size() * sizeof(PttaAdamEntry), hipMemcpyHostToDevice, s));
    c->adam_tab_dirty = false;
    return 0;
}

extern "C" {

int ptta_version(void) { return PTTA_ABI_VERSION; }

// why the calling thread's last ptta_create refused a configuration (there is no handle to ask then): ptta_last_error(NULL)
static thread_local std::string g_create_err;
static int create_refused(const std::string& why) { g_create_err = why; return -38; }
// the same slot for a handle-free entry point that refuses its arguments (score.hip)
extern "C++" int ptta_refuse_args(const char* why) { g_create_err = why; return -22; }

const char* ptta_last_error(ptta_handle h) {
    if (!h) return g_create_err.empty() ? "null handle" : g_create_err.c_str();
    return h->nl && h->err.empty() ? h->nl->err.c_str() : h->err.c_str();
}

// a created generic engine (NLSPN, CostDCNet) as a handle: every entry point forwards to it
static int wrap_gnet(ptta_handle* out, GNet* e, int rc, int gmix, int n, int height, int width, const ptta_hparams* hp) {
    if (!e) return rc ? rc : -12;
    e->mixed = e->naive ? 0 : gmix;
    ptta_ctx* c = new ptta_ctx();
    c->nl = e; c->N = n; c->H = height; c->W = width; c->hp = *hp;
    *out = c;
    return 0;
}

int ptta_create(ptta_handle* out, int backbone_id, int meta_mode, int n, int height, int width, int dtype, const ptta_hparams* hp) {
    if (!out) return -1;
    *out = nullptr;
    g_create_err.clear();
    // MSG_CHN's source model (include/ptta.h PTTA_MSGCHN_PLAIN): `_forward` in fp32 on one rank, the eval forward only; refused before anything
    // is allocated
    if (meta_mode & PTTA_MSGCHN_PLAIN) {
        if (backbone_id != PTTA_BACKBONE_MSG_CHN) return create_refused("PTTA_MSGCHN_PLAIN: the flag belongs to the MSG_CHN backbone (NLSPN has PTTA_META_NONE, CostDCNet PTTA_COSTDC_PLAIN)");
        if ((meta_mode & 0xff) != PTTA_META_1LAYER) return create_refused("PTTA_MSGCHN_PLAIN with PTTA_META_2LAYERS or PTTA_META_NONE: the flag itself takes the meta layer out, its base mode is PTTA_META_1LAYER");
        if ((dtype & 0xff) == PTTA_DTYPE_MIXED) return create_refused("PTTA_MSGCHN_PLAIN with PTTA_DTYPE_MIXED: the scored forward of the mixed mode is the fp32 one already");
    }
    // no meta layer (include/ptta.h PTTA_META_NONE): NLSPN's `_forward` in fp32 on one rank -- the BatchNorm-adaptation baseline, or with
    // PTTA_ADAPT_META_ONLY the source model; refused before anything is allocated
    if ((meta_mode & 0xff) == PTTA_META_NONE) {
        if (backbone_id != PTTA_BACKBONE_NLSPN) return create_refused("PTTA_META_NONE: the network without the meta layer is built for the NLSPN backbone only");
        if ((dtype & 0xff) == PTTA_DTYPE_MIXED) return create_refused("PTTA_META_NONE with PTTA_DTYPE_MIXED: no bound has been measured for it");
        if (meta_mode & PTTA_NLSPN_SYNCBN_ADAPT) return create_refused("PTTA_META_NONE with PTTA_NLSPN_SYNCBN_ADAPT: there are no heads to append to the adapted list");
    }
    // CostDCNet without the meta layer (include/ptta.h PTTA_COSTDC_PLAIN): `_forward` in fp32 on one rank -- the BatchNorm-adaptation baseline, or
    // with PTTA_ADAPT_META_ONLY the source model; refused before anything is allocated
    if (meta_mode & PTTA_COSTDC_PLAIN) {
        if (backbone_id != PTTA_BACKBONE_COSTDCNET) return create_refused("PTTA_COSTDC_PLAIN: the flag belongs to the CostDCNet backbone (NLSPN has PTTA_META_NONE)");
        if ((meta_mode & 0xff) != PTTA_META_1LAYER) return create_refused("PTTA_COSTDC_PLAIN with PTTA_META_2LAYERS or PTTA_META_NONE: the flag itself takes the meta layer out, its base mode is PTTA_META_1LAYER");
        if (meta_mode & PTTA_SYNCBN_ADAPT) return create_refused("PTTA_COSTDC_PLAIN with PTTA_SYNCBN_ADAPT: there are no heads to append to the adapted list");
        if ((dtype & 0xff) == PTTA_DTYPE_MIXED) return create_refused("PTTA_COSTDC_PLAIN with PTTA_DTYPE_MIXED: no bound has been measured for it");
    }
    // the meta-only adapted list is built for NLSPN's 1layer meta conv in fp32 (include/ptta.h PTTA_ADAPT_META_ONLY); refused before anything is allocated
    if ((meta_mode & PTTA_ADAPT_META_ONLY) && !(meta_mode & PTTA_COSTDC_PLAIN)) {
        if (backbone_id != PTTA_BACKBONE_NLSPN) return create_refused("PTTA_ADAPT_META_ONLY: only the NLSPN adapter has adapt_mode 'meta'");
        if ((meta_mode & 0xff) == PTTA_META_2LAYERS) return create_refused("PTTA_ADAPT_META_ONLY with PTTA_META_2LAYERS: the block's own BatchNorm2d under 'meta' is not built");
        if ((dtype & 0xff) == PTTA_DTYPE_MIXED) return create_refused("PTTA_ADAPT_META_ONLY with PTTA_DTYPE_MIXED: no bound has been measured for it");
        if (meta_mode & PTTA_NLSPN_SYNCBN_ADAPT) return create_refused("PTTA_ADAPT_META_ONLY with PTTA_NLSPN_SYNCBN_ADAPT: the SyncBatchNorm form of this mode is not offered");
    }
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
        const int meta = meta_mode & ~(PTTA_NLSPN_LEGACY_OFFSET | PTTA_NLSPN_SYNCBN_ADAPT | PTTA_ADAPT_META_ONLY);
        if ((meta != PTTA_META_1LAYER && meta != PTTA_META_2LAYERS && meta != PTTA_META_NONE) || dtype != PTTA_DTYPE_F32) return -38;
        if (meta == PTTA_META_2LAYERS && (meta_mode & PTTA_NLSPN_SYNCBN_ADAPT)) return -38;
        int rc = 0;
        GNet* e = nlspn_create(n, height, width, hp, ((meta_mode & PTTA_NLSPN_LEGACY_OFFSET) ? 1 : 0) | ((meta_mode & PTTA_NLSPN_SYNCBN_ADAPT) ? 2 : 0) |
                               (meta == PTTA_META_2LAYERS ? 4 : 0) | ((meta_mode & PTTA_ADAPT_META_ONLY) ? 8 : 0) | (meta == PTTA_META_NONE ? 16 : 0), &rc);
        return wrap_gnet(out, e, rc, gmix, n, height, width, hp);
    }
    if (backbone_id == PTTA_BACKBONE_COSTDCNET) {
        // (no mixed mode for CostDCNet: with single-MFMA data gradients its scored depth leaves the tolerance -- 2.0e-3 / 1.7e-3 at 480x640 /
        // 320x400, with hi + lo weights in them still 1.1e-3 / 1.2e-3, with single-MFMA proxy frames alone 8.9e-4 at 320x400, for 2 - 3 % of
        // the step: profiles/r06_nlspn_costdcnet_mixed.txt -- its argmax over the cost volume amplifies any change of the update)
        // 2layers: the Res_Conv(16, 64) block (costdc_api.hip), fp32 only, not with PTTA_SYNCBN_ADAPT
        const int plain = (meta_mode & PTTA_COSTDC_PLAIN) ? 1 : 0;         // (PTTA_ADAPT_META_ONLY without it was refused above)
        const int meta = meta_mode & ~(PTTA_SYNCBN_ADAPT | (plain ? (PTTA_COSTDC_PLAIN | PTTA_ADAPT_META_ONLY) : 0));
        if ((meta != PTTA_META_1LAYER && meta != PTTA_META_2LAYERS) || dtype != PTTA_DTYPE_F32 || !hp || gmix) return -38;
        if (meta == PTTA_META_2LAYERS && (meta_mode & PTTA_SYNCBN_ADAPT)) return -38;
        int rc = 0;
        GNet* e = costdc_create(n, height, width, hp, hp->max_predict_depth, ((meta_mode & PTTA_SYNCBN_ADAPT) ? 1 : 0) | (meta == PTTA_META_2LAYERS ? 2 : 0) |
                                (plain ? 4 : 0) | ((plain && (meta_mode & PTTA_ADAPT_META_ONLY)) ? 8 : 0), &rc);
        return wrap_gnet(out, e, rc, gmix, n, height, width, hp);
    }
    const int plain = (meta_mode & PTTA_MSGCHN_PLAIN) ? 1 : 0;          // (its backbone, base mode and dtype were checked above)
    meta_mode &= ~PTTA_MSGCHN_PLAIN;
    if (plain && meta_mode != PTTA_META_1LAYER) return create_refused("PTTA_MSGCHN_PLAIN takes no other flag beside it");
    if (backbone_id != PTTA_BACKBONE_MSG_CHN || (meta_mode != PTTA_META_1LAYER && meta_mode != PTTA_META_2LAYERS)) return -38;
    const int keep = (dtype >> 8) & 7;                 // PTTA_MIXED_KEEP_*: classes kept at fp32 / bf16x3 (precision budget)
    dtype &= 0xff;
    if (n < 1 || height < 16 || width < 16 || (dtype != PTTA_DTYPE_F32 && dtype != PTTA_DTYPE_MIXED) || !hp) return -22;
    ptta_ctx* c = new ptta_ctx();
    c->meta_mode = meta_mode; c->plain = plain;
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

int ptta_load_weights(ptta_handle c, const char* name_, const void* tensor, const int64_t* shape, int ndim, ptta_stream s_) {
    NLFWD((name_ && tensor) ? c->nl->load(name_, tensor, shape, ndim, (hipStream_t)s_) : -1);

    if (!c || !name_ || !tensor) return -1;
    c->drop_graphs();
    RUN(pipe_quiesce(c));
    c->proxy_valid = false; c->fused_pp_valid = false; c->pset[0].proxy_valid = false; c->pset[1].proxy_valid = false;
    return load_weight(c, name_, tensor, shape, ndim, (hipStream_t)s_);
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
    PLAIN_NO_TRAIN("ptta_forward_train");
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
    PLAIN_NO_TRAIN("ptta_forward_eval_last");
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
    PLAIN_NO_TRAIN("ptta_loss_forward");
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
    PLAIN_NO_TRAIN("ptta_loss_backward");
    RUN(ptta_launch_loss_backward(depth, loss_image, sparse, validity, c->hp.max_input_depth, emb, ref, rows, 512,
                                  c->N, c->H, c->W, c->loss_ws, gdepth, gref, (hipStream_t)s_));
    return 0;
}

int ptta_backward(ptta_handle c, const float* grad_depth, const float* grad_ref, float* gw_out, float* gb_out, ptta_stream s_) {
    NLFWD(grad_depth ? c->nl->backward_from(grad_depth, grad_ref, (hipStream_t)s_) : -1);   // gradients: ptta_get_grad

    if (!c || !grad_depth) return -1;
    PLAIN_NO_TRAIN("ptta_backward");
    if (!c->fwd_valid) return c->fail("ptta_backward without a preceding ptta_forward_train", -3);
    hipStream_t s = (hipStream_t)s_;
    const float* g_net = grad_depth;
    if (c->dual) {
        scatter_dual_grad_launch(grad_depth, c->g_net, c->N, c->H, c->W, c->Hp, c->Wp, c->pt, c->pr, s);
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

int ptta_adam_step(ptta_handle c, const float* gw, const float* gb, ptta_stream s_) {
    if (c && c->nl) { c->err.clear(); return (gw || gb) ? c->fail("explicit gradients are an MSG_CHN 1layer convenience", -22) : c->nl->adam_step_checked((hipStream_t)s_); }

    if (!c) return -1;
    PLAIN_NO_TRAIN("ptta_adam_step");
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

// One exchange description into the handle.  `on`: an exchange is bound; `keeps_graph`: its collectives are enqueued by the library on the
// step's stream and are captured like any kernel (RCCL) -- otherwise they are host-driven and the step cannot be replayed.  Either way the
// second stream is given up while an exchange is on (collectives of one communicator are kept in one stream order).
static int set_stat_sync(ptta_ctx* c, const PttaStatSync& sy, bool on, bool keeps_graph) {
    if (c->nl && !c->nl->one_rank_why.empty()) { c->err.clear(); return c->nl->fail(c->nl->one_rank_why, -38); }
    if (c->nl && c->nl->meta_only) { c->err.clear(); return c->nl->fail("the SyncBatchNorm form of the meta-only adaptation mode is not offered (PTTA_ADAPT_META_ONLY)", -38); }
    if (c->nl) { c->err.clear(); c->nl->drop_graphs(); c->nl->stat_sync = sy; return 0; }
    PLAIN_ONE_RANK("statistics exchange");
    if (on && c->meta_mode == PTTA_META_2LAYERS && !c->m2.generic) return c->fail("SyncBatchNorm needs the default arithmetic for the 2layers meta layer", -38);
    c->stat_sync = sy;
    c->drop_graphs();
    if (on) {
        if (c->pre_sync_graph < 0) { c->pre_sync_graph = c->use_graph; c->pre_sync_aux = c->use_aux; }
        else if (keeps_graph) c->use_graph = c->pre_sync_graph;         // coming from the callback mode: the graph is available again
        if (!keeps_graph) c->use_graph = 0;
        c->use_aux = 0;
    } else if (c->pre_sync_graph >= 0) {     // exchange switched off again: back to the replayed, two-stream step
        c->use_graph = c->pre_sync_graph; c->use_aux = c->pre_sync_aux; c->pre_sync_graph = c->pre_sync_aux = -1;
    }
    return 0;
}

// the exchange through the caller's callback: the step contains host-driven collectives -- no graph replay, one stream
int ptta_set_stat_sync(ptta_handle c, ptta_allreduce_fn fn, void* user, double* exchange_buf, int64_t capacity, int world_size) {
    if (!c || world_size < 1 || (world_size > 1 && (!fn || !exchange_buf || capacity < 2 * 1024))) return -22;
    PttaStatSync sy; sy.fn = (ptta_allreduce_cb)fn; sy.user = user; sy.buf = exchange_buf; sy.cap = (long)capacity; sy.world = world_size;
    return set_stat_sync(c, sy, world_size > 1, false);
}

// The same exchange on the library's own RCCL communicator (rccl_sync.hip): the collectives are enqueued by the library on the
// step's stream, so they are captured into the step's hipGraph like any kernel -- graph replay stays on; only the second stream
// is given up.  comm == NULL or world_size == 1 with comm == NULL: off.
int ptta_set_stat_sync_rccl(ptta_handle c, void* comm, double* exchange_buf, int64_t capacity, int world_size) {
    if (!c || world_size < 1 || (comm && (!exchange_buf || capacity < 2 * 1024))) return -22;
    PttaStatSync sy; sy.comm = comm; sy.buf = exchange_buf; sy.cap = (long)capacity; sy.world = world_size;
    return set_stat_sync(c, sy, comm != nullptr, true);
}

// DistributedDataParallel's gradient averaging (src/msg_chn_model_adapt.py:476-480) for the fused ptta_step: between backward and
// Adam the adapted gradients (one arena: 37 KB for MSG_CHN 1layer) are averaged over the communicator's ranks with ONE
// ncclAllReduce enqueued on the step's stream (captured into the hipGraph).  comm == NULL: off.
int ptta_set_grad_sync_rccl(ptta_handle c, void* comm) {
    if (!c) return -1;
    if (c->nl && !c->nl->one_rank_why.empty()) { c->err.clear(); return c->nl->fail(c->nl->one_rank_why, -38); }
    if (c->nl && c->nl->meta_only) { c->err.clear(); return c->nl->fail("no gradient exchange in the meta-only adaptation mode: more than one rank is not offered (PTTA_ADAPT_META_ONLY)", -38); }
    if (c->nl) { c->nl->drop_graphs(); c->nl->grad_comm = comm; return 0; }
    PLAIN_ONE_RANK("ptta_set_grad_sync_rccl");
    c->grad_comm = comm;
    c->drop_graphs();
    return 0;
}

// Per-handle switches (include/ptta.h documents the keys).  The defaults are the shipped step; every other value is a correct,
// slower form kept for validation (tests/test_gpu_options.py: bit-identical to the default unless noted) or as the fallback a
// configuration takes by itself (small maps, SyncBatchNorm exchange, N > 16).
// ("graph" is not in the table: ptta_set_graph, which the generic engine has too)
struct Option { const char* key; int ptta_ctx::*member; int hi; bool mixed_free; };      // values 0 .. hi; mixed_free: may differ from 1 in the mixed mode
static const Option kOptions[] = {
    {"aux_stream", &ptta_ctx::use_aux, 1, true},        {"thru", &ptta_ctx::thru, 1, true},
    {"adam_in_wgrad", &ptta_ctx::adam_in_wgrad, 1, true}, {"bwd_w2", &ptta_ctx::bwd_w2, 1, true},
    {"fuse_first", &ptta_ctx::fuse_first, 2, false},    {"fuse_head_bwd", &ptta_ctx::fuse_head_bwd, 1, false},
    {"fuse_heads", &ptta_ctx::fuse_heads, 1, false},    {"heads_v2", &ptta_ctx::heads_v2, 1, false},
    {"cos_in_gemm", &ptta_ctx::cos_grad_fused, 1, false}, {"mask_bits", &ptta_ctx::mask_bits_on, 1, false},
    {"stamps", &ptta_ctx::stamps, 1, true},             {"pair_fuse", &ptta_ctx::pair_fuse, 1, true},
    {"tpair_fuse", &ptta_ctx::tpair_fuse, 1, true},
};
static const Option* find_option(const std::string& k) {
    for (const Option& o : kOptions) if (k == o.key) return &o;
    return nullptr;
}
int ptta_set_option(ptta_handle c, const char* key, int value) {
    if (!c || !key) return -1;
    const std::string k(key);
    if (k == "graph") return ptta_set_graph(c, value);
    if (k == "eval_bn_fused_count") return c->nl ? (c->err.clear(), c->nl->fail("ptta_set_option: 'eval_bn_fused_count' is read-only", -22))
                                                 : c->fail("ptta_set_option: 'eval_bn_fused_count' is read-only", -22);
    if (k == "eval_bn_fused") {                    // meta-only handles (NLSPN, CostDCNet's source model): the eval BatchNorm in the convolution epilogue (1) or as its own launch (0)
        if (!c->nl || !c->nl->meta_only) return c->nl ? (c->err.clear(), c->nl->fail("ptta_set_option: 'eval_bn_fused' belongs to PTTA_ADAPT_META_ONLY handles", -38))
                                                      : c->fail("ptta_set_option: 'eval_bn_fused' belongs to PTTA_ADAPT_META_ONLY handles", -38);
        c->err.clear();
        if (value < 0 || value > 1) return c->nl->fail("ptta_set_option: value out of range for 'eval_bn_fused'", -22);
        if (c->nl->eval_bn_fused != value) { c->nl->drop_graphs(); c->nl->eval_bn_fused = value; }
        return 0;
    }
    if (k == "head_bn_fused" || k == "head_bn_fused_count") {   // NLSPN / CostDCNet: the stage-2 head trainer's frozen BatchNorm2d in the convolution epilogue
        if (!c->nl) return c->fail("ptta_set_option: '" + k + "' belongs to the generic engine's handles (MSG_CHN has no BatchNorm2d)", -38);
        c->err.clear();
        if (k == "head_bn_fused_count") return c->nl->fail("ptta_set_option: 'head_bn_fused_count' is read-only", -22);
        if (value < 0 || value > 1) return c->nl->fail("ptta_set_option: value out of range for 'head_bn_fused'", -22);
        if (c->nl->head_bn_fused != value) { c->nl->drop_graphs(); c->nl->head_bn_fused = value; }
        return 0;
    }
    if (k == "deterministic") {                    // NLSPN handles that train: the propagation gradients' scatters in fixed point, no float atomics
        if (!c->nl) return c->fail("ptta_set_option: 'deterministic' belongs to NLSPN handles (MSG_CHN's step is bit-reproducible as it is)", -38);
        c->err.clear();
        return c->nl->set_deterministic(value);
    }
    if (c->nl) return -38;                         // the generic engine has no other switch
    if (k == "pair_fuse_count" || k == "tpair_fuse_count") return c->fail("ptta_set_option: '" + k + "' is read-only", -22);
    const Option* o = find_option(k);
    if (!o) return c->fail("ptta_set_option: unknown key '" + k + "'", -22);
    int* f = &(c->*(o->member));
    if (value < 0 || value > o->hi) return c->fail("ptta_set_option: value out of range for '" + k + "'", -22);
    if (c->mixed && !o->mixed_free && value != 1)
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
    if (k == "pipelined_active") { *value = !(c->nl || c->plain || c->prof_on || c->dual || c->stat_sync.on() || c->grad_comm || c->naive || c->bf16); return 0; }
    // read-only: 1 when the step takes the two-stream `thru` schedule (loss gradient from the valid-weight partials), as far as it can be known
    // without the caller's stream (the second stream is created on first use)
    if (k == "thru_active") { *value = c->nl ? 0 : (c->thru && c->cos_grad_fused && heads_v2_on(c) && c->use_aux); return 0; }
    if (k == "eval_bn_fused") { if (!c->nl || !c->nl->meta_only) return -38; *value = c->nl->eval_bn_fused; return 0; }
    // read-only: how many BatchNorm of the eval forward ride in a convolution epilogue as configured now (0 with "eval_bn_fused" at 0)
    if (k == "eval_bn_fused_count") { if (!c->nl || !c->nl->meta_only) return -38; *value = c->nl->eval_bn_fused_count(); return 0; }
    if (k == "head_bn_fused" || k == "head_bn_fused_count") {
        if (!c->nl) return -38;
        *value = k == "head_bn_fused" ? c->nl->head_bn_fused : c->nl->head_bn_fused_count();
        return 0;
    }
    if (k == "deterministic") return c->nl ? c->nl->get_deterministic(value) : -38;
    if (c->nl) { if (k != "graph") return -38; *value = c->nl->use_graph; return 0; }
    if (k == "graph") { *value = c->use_graph; return 0; }
    // read-only: how many (stride-2 -> stride-1) layer pairs the last step issued as ONE launch (a replayed graph: as it was captured)
    if (k == "pair_fuse_count") { *value = c->pair_fuse_count; return 0; }
    // read-only: the same count for the (transposed -> stride-1) pairs of option "tpair_fuse"
    if (k == "tpair_fuse_count") { *value = c->tpair_fuse_count; return 0; }
    const Option* o = find_option(k);
    if (!o) return -22;
    *value = c->*(o->member);
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
    if (c->tpair_unwritten.count(it->second.p))
        return c->fail(std::string("debug tensor ") + name + " is not written while option 'tpair_fuse' is 1 (the fused launch keeps it on chip): set it to 0", -38);
    if (capacity < it->second.numel) return c->fail("capacity too small", -22);
    hipStream_t s = (hipStream_t)s_;
    const long n = it->second.numel;
    if (it->second.is_act == 3) RUN(ptta_launch_hn_untile(it->second.p, dst, n / 512, s));
    else if ((it->second.is_act == 1 && c->bf16) || it->second.is_act == 2) to_f32_launch((const bf16_t*)it->second.p, dst, n, s);
    else HIPCHK(hipMemcpyAsync(dst, it->second.p, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

}  // extern "C"
