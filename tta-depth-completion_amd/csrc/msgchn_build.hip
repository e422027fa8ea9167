// Weight registry and workspace of an MSG_CHN handle (what ptta_create allocates) and the packing of one loaded tensor
// into the layouts the kernels read (ptta_load_weights).
#include "msgchn_ctx.h"

using namespace msgchn;

namespace msgchn {

int pad16(int n) { return n % 16 == 0 ? 0 : (n / 16 + 1) * 16 - n; }

static ConvW alloc_convw(ptta_ctx* c) {
    ConvW w;
    w.mf32 = c->falloc(9 * 4 * 64 * 4);
    w.mbf16 = (bf16_t*)c->dalloc(9 * 2 * 64 * 8 * sizeof(bf16_t));
    w.mlo = (bf16_t*)c->dalloc(9 * 2 * 64 * 8 * sizeof(bf16_t));
    w.canon = c->falloc(9 * 32 * 32);
    return w;
}

static const char* kRgb32[] = {"rgb_encoder.init.2", "rgb_encoder.enc1.1", "rgb_encoder.enc1.3", "rgb_encoder.enc2.1", "rgb_encoder.enc2.3",
                        "rgb_encoder.enc3.1", "rgb_encoder.enc3.3", "rgb_encoder.enc4.1", "rgb_encoder.enc4.3"};

void build_registry(ptta_ctx* c) {
    auto add32 = [&](const std::string& n, int transposed, bool need_bwd) {
        L32 l; l.f = alloc_convw(c); if (need_bwd && !c->plain) l.b = alloc_convw(c);        // (the source model has no backward)
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
    if (c->plain) return;       // the source model (PTTA_MSGCHN_PLAIN): no meta layer, no heads
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
    // [real | proxy] maps hold 2 Nn frames; the source model (PTTA_MSGCHN_PLAIN) has one pass: every map holds Nn
    const int Nn = c->Nn, B2 = c->plain ? Nn : 2 * Nn;
    const int H1 = c->Hp, W1 = c->Wp;
    c->H2 = H1 / 2; c->W2 = W1 / 2; c->H4 = H1 / 4; c->W4 = W1 / 4; c->H8 = H1 / 8; c->W8 = W1 / 8; c->H16 = H1 / 16; c->W16 = W1 / 16;
    const int H2 = c->H2, W2 = c->W2, H4 = c->H4, W4 = c->W4, H8 = c->H8, W8 = c->W8, H16 = c->H16, W16 = c->W16;
    c->Rg = c->plain ? 0 : (long)Nn * H4 * W4;
    if (c->dual) { c->img_pad = c->falloc((size_t)Nn * 3 * H1 * W1); c->sp_pad = c->falloc((size_t)Nn * H1 * W1); }
#define A_(name, nb, h, w) c->name = c->act(#name, nb, h, w)
#define M_(name, nb, h, w) c->name = c->map1(#name, nb, h, w)
    M_(dclamp, Nn, H1, W1); M_(d12, Nn, H2, W2); M_(d14, Nn, H4, W4);
    M_(out1, B2, H4, W4); M_(p12, B2, H2, W2); M_(q, B2, H2, W2); M_(p11, B2, H1, W1);
    M_(depth_net, Nn, H1, W1); M_(depth_final, c->N, c->H, c->W); M_(validity_tmp, c->N, c->H, c->W);
    A_(c0a, B2, H1, W1); A_(c0, B2, H1, W1); A_(c1a, B2, H2, W2); A_(c1, B2, H2, W2);
    A_(c2a, B2, H4, W4); A_(c2, B2, H4, W4);
    if (c->plain) c->m = nullptr; else A_(m, B2, H4, W4);            // (ptta_ctx::meta_out: the source model reads c2 where the others read m)
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
    if (c->plain) {
        // the eval forward's maps are all the source model has: no ReLU masks, heads' workspace, loss workspace, gradient maps, weight-gradient
        // partials, gradient arena, staged inputs or Adam table -- only the few words the shared entry points write
        c->hyper = c->falloc(16); c->step_dev = (int*)c->dalloc(16);
        c->stamp_f = c->falloc(16); c->stamp_base = (unsigned long long*)c->dalloc(8); c->dbg["stamps"] = Dbg{c->stamp_f, 16, 0};
        return;
    }
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

static long shape_numel(const int64_t* shape, int ndim) { long n = 1; for (int i = 0; i < ndim; ++i) n *= shape[i]; return n; }

// one tensor of the state_dict (ptta_load_weights): packed into the layouts the kernels read; BatchNorm buffers are bound, not copied
int load_weight(ptta_ctx* c, const std::string& name, const void* tensor, const int64_t* shape, int ndim, hipStream_t s) {
    const long numel = shape_numel(shape, ndim);
    auto ends = [&](const char* suf) { const size_t n = strlen(suf); return name.size() >= n && name.compare(name.size() - n, n, suf) == 0; };
    if (name.rfind("proj_t.", 0) == 0) return 0;                     // EMA target head: unused in stage 3 (:551-554)
    // the source model runs none of what _prepare_head adds: a stage-3 checkpoint's meta layer (1layer or 2layers keys) and heads are ignored
    if (c->plain && (name.rfind("conv1_rgb_meta", 0) == 0 || name.rfind("proj", 0) == 0 || name.rfind("pred", 0) == 0)) return 0;
    if (name.rfind("conv1_rgb_meta", 0) == 0) {
        if (c->meta_mode == PTTA_META_2LAYERS) {           // BatchNorm2d buffers of Res_Conv: bound, updated in place
            const bool first = name.find("conv1_meta.0.1.") != std::string::npos, second = name.find("conv1_meta.2.") != std::string::npos;
            if ((first || second) && ends(".running_mean")) { (first ? c->m2.rm1 : c->m2.rm2) = (float*)tensor; return 0; }
            if ((first || second) && ends(".running_var")) { (first ? c->m2.rv1 : c->m2.rv2) = (float*)tensor; return 0; }
            if ((first || second) && ends(".num_batches_tracked")) { (first ? c->m2.nbt1 : c->m2.nbt2) = (long long*)tensor; return 0; }
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
            transpose_launch(src, l.Wt, l.N, l.K, s);
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

}  // namespace msgchn
