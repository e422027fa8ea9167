// The backward half of the MSG_CHN step's launch schedule (the minimal backward described at the top of msgchn_forward.hip: data gradients
// only along paths that reach conv1_rgb_meta, then its weight gradient): the heads, the cascades, the 2layers meta block.
#include "msgchn_ctx.h"

using namespace msgchn;

namespace msgchn {

// gradients of the seven 2layers parameters from d m (= c->dm_total, real frames, pass 0 statistics)
static int meta2_backward(ptta_ctx* c, hipStream_t s) {
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
    if (c->bf16 || c->nar_bwd) from_f32_launch(c->g_feat_f32, (bf16_t*)c->g_feat, c->Rg * 32, s);
    return 0;
}

// data gradients from d(depth_net) [Nn,1,Hp,Wp] and d(feat) down to conv1_rgb_meta, then its wgrad
int backbone_backward(ptta_ctx* c, const float* g_net, hipStream_t s, bool join_aux) {
    const int Nn = c->Nn, B2 = 2 * Nn;
    const int nbf = c->nar_bwd ? 1 : c->bf16;            // gradient maps: narrow in the mixed mode (conv32() routes every bwd launch there itself)
    const int H1 = c->Hp, W1 = c->Wp, H2 = c->H2, W2 = c->W2, H4 = c->H4, W4 = c->W4, H8 = c->H8, W8 = c->W8;
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
    // (each stride-2 data gradient and the stride-1 one that reads its sum: one launch on small maps, conv32_pair -- here with
    // depth_encoder3.enc2.3 below, whose ordering against the side upsamplings is unchanged: they read what both halves wrote)
    { E e; e.raw = c->dw2; e.mask = c->w2; e.mask_nb = B2; e.sum = c->dfeat_tot; e.add1 = c->g_feat; e.add1_nb = Nn;
      RUN(conv32_pair(c, s, true, "depth_decoder3.dec2.1", c->dt3, Nn, Nn, H2, W2, e, "depth_encoder3.enc2.3", Nn, em(c->de3_2a, c->e3_2a, B2))); }
    // The three transposed bilinear upsamplings of the backward (d z2 += up2^T(d feat_tot), d z3 = d s1_2 + up2^T(d e3_1), d z4 = d s0_2 + up2^T(d e3_0))
    // do not lie on the chain d feat_tot -> encoder 3 -> decoder 2: they run on the second stream, and each
    // result enters the chain as the addend of a convolution epilogue (out_sum = masked result + addend; fp32: the same two operands of the
    // same addition as `add + up2^T(...)` in the upsampling kernel).  One join, in front of decoder 2's prediction head.
    hipStream_t sd = join_aux ? c->aux(s) : nullptr;
    if (!sd) sd = s;
    // ---- encoder 3 ----
    // (each transposed data gradient and the stride-1 one that reads its sum: one launch where the form applies, conv32_tpair; the sums
    // d e3_1, d e3_0 are still written for the side upsamplings below)
    { E e; e.sum = c->de3_1; e.mask = c->e3_1; e.mask_nb = B2; e.add1 = c->ds1_3; e.add1_nb = Nn;
      RUN(conv32_tpair(c, s, true, "depth_encoder3.enc2.1", c->de3_2a, Nn, Nn, H4, W4, e, "depth_encoder3.enc1.3", Nn, em(c->de3_1a, c->e3_1a, B2))); }
    // (depth_encoder3.enc1.1 -> init.2 likewise where the one launch pays: small frames; at the headline size it does not, and the two launches
    // keep their places on either side of the fork below, init.2 beside the side upsamplings)
    bool init2_done = false;
    { E e; e.sum = c->de3_0; e.mask = c->e3_0; e.mask_nb = B2; e.add1 = c->ds0_3; e.add1_nb = Nn;
      const E se = em(c->de3_0a, c->e3_0a, B2);
      init2_done = conv32_tpair_takes(c, true, "depth_encoder3.enc1.1", c->de3_1a, Nn, Nn, H2, W2, e, "depth_encoder3.init.2", Nn, se);
      if (init2_done) RUN(conv32_tpair(c, s, true, "depth_encoder3.enc1.1", c->de3_1a, Nn, Nn, H2, W2, e, "depth_encoder3.init.2", Nn, se));
      else CV("depth_encoder3.enc1.1", true, CONV_T2, c->de3_1a, Nn, Nn, H2, W2, false, e); }
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
    if (!init2_done) CV("depth_encoder3.init.2", true, CONV_S1, c->de3_0, Nn, Nn, H1, W1, false, em(c->de3_0a, c->e3_0a, B2));
    RUN(dgrad_in_ch1("depth_encoder3.init.0", c->de3_0a, g_net, c->dp11, H1, W1));       // d p11 = conv^T + d output
    REST_(s, ptta_launch_up2T_1ch(c->dp11, c->dq, Nn, H2, W2, s));                              // d(out2 + p12)
    // ---- decoder 2 ----
    if (sd != s) HIPCHK(hipStreamWaitEvent(s, c->ev_side[3], 0));
    { E e = em(c->ds0_2, c->s0_2, B2); e.sum = c->dz4; e.add1 = c->up4_t; e.add1_nb = Nn;      // d z4 = d s0_2 + up2^T(d e3_0)
      RUN(head_bwd("depth_decoder2.prdct.3", "depth_decoder2.prdct.1", c->dq, c->v2, c->dv2, H2, W2, e)); }
    CV("depth_decoder2.dec1.3", true, CONV_S1, c->dz4, Nn, Nn, H2, W2, false, em(c->du2, c->u2, B2));
    { E e = em(c->ds1_2, c->s1_2, B2); e.sum = c->dz3; e.add1 = c->up3_t; e.add1_nb = Nn;      // d z3 = d s1_2 + up2^T(d e3_1)
      RUN(conv32_pair(c, s, true, "depth_decoder2.dec1.1", c->du2, Nn, Nn, H2, W2, e, "depth_decoder2.dec2.3", Nn, em(c->dt2, c->t2, B2))); }
    { E e; e.sum = c->dz2; e.mask = c->z2; e.mask_nb = B2; e.add1 = c->dz2_up; e.add1_nb = Nn;
      RUN(conv32_pair(c, s, true, "depth_decoder2.dec2.1", c->dt2, Nn, Nn, H4, W4, e, "depth_encoder2.enc2.3", Nn, em(c->de2_2a, c->e2_2a, B2))); }
    // ---- encoder 2 ----
    { E e; e.sum = c->de2_1; e.mask = c->e2_1; e.mask_nb = B2; e.add1 = c->ds1_2; e.add1_nb = Nn;
      RUN(conv32_tpair(c, s, true, "depth_encoder2.enc2.1", c->de2_2a, Nn, Nn, H8, W8, e, "depth_encoder2.enc1.3", Nn, em(c->de2_1a, c->e2_1a, B2))); }
    { E e; e.sum = c->de2_0; e.mask = c->e2_0; e.mask_nb = B2; e.add1 = c->ds0_2; e.add1_nb = Nn;
      RUN(conv32_tpair(c, s, true, "depth_encoder2.enc1.1", c->de2_1a, Nn, Nn, H4, W4, e, "depth_encoder2.init.2", Nn, em(c->de2_0a, c->e2_0a, B2))); }
    RUN(dgrad_in_ch1("depth_encoder2.init.0", c->de2_0a, c->dq, c->dp12, H2, W2));       // d p12 = conv^T + d q
    REST_(s, ptta_launch_up2T_1ch(c->dp12, c->dout1, Nn, H4, W4, s));
    // ---- decoder 1: only the prediction head reaches the meta layer (y0 = e1_0 + m) ----
    RUN(dgrad_out1("depth_decoder1.prdct.3", c->dout1, c->v1, c->dv1, H4, W4));
    { E e; e.sum = c->dm_total; e.mask = c->s0_1; e.mask_nb = B2; e.add1 = c->dw2; e.add1_nb = Nn; e.add2 = c->ds1_2; e.add2_nb = Nn;
      CV("depth_decoder1.prdct.1", true, CONV_S1, c->dv1, Nn, Nn, H4, W4, false, e); }
    if (sd != s && c->loss_report.on) HIPCHK(hipStreamWaitEvent(s, c->ev_loss, 0));       // (signalled ~200 us ago: the caller's loss_info is ordered on `s`)
    // ---- weight gradient of the meta layer: input = c2 of the real frames ----
    // (mixed mode, 2layers meta block: its BatchNorm / weight-gradient kernels take fp32 operands -- the 1/4-resolution gradient map is widened
    // once, 3.4 MB; the 1layer weight gradient reads the narrow map itself)
    if (c->nar_bwd && c->meta_mode == PTTA_META_2LAYERS) RUN(to_wide(c, c->dm_total, c->dm_f32, (long)Nn * H4 * W4 * 32, s));
    if (c->meta_mode == PTTA_META_2LAYERS) return meta2_backward(c, s);
    if (!c->bf16 && c->x3 && !c->naive) {
        // default arithmetic: the bf16x3 reduction-GEMM form (gwgrad_mfma.hip gwgrad_x3_kernel, single-pair mode)
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

}  // namespace msgchn
