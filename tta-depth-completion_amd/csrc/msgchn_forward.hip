// The forward half of the launch schedule of one ProxyTTA step for the MSG_CHN backbone: the conv32 / conv_in / conv_out1
// launch wrappers, the meta layer, the RGB encoder, the three cascades and the MLP heads.
//
// Schedule = the dataflow of network_adapt._rgbd_meta_contrast
// (external_src/MSG_CHN/workspace/exp_msg_chn/network_exp_msg_chn_adapt.py:463-557) with
//   * the grad pass and the no-grad proxy (zero image) pass batched into ONE launch per layer
//     (batch = [real frames | proxy frames]); the depth-only encoder of stage 1 is shared,
//   * every elementwise op of the graph (pre-activation ReLU, bias, decoder skip additions,
//     bilinear x2 skip, final residual) fused into the producing/consuming conv,
//   * the minimal backward: data gradients only along paths that reach conv1_rgb_meta, weight
//     gradient only for conv1_rgb_meta, then Adam on device.
#include "msgchn_ctx.h"

using namespace msgchn;

namespace msgchn {

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

// the launch arguments of one 32 -> 32 layer as conv32() issues it
static int conv32_args(ptta_ctx* c, Conv32Args& a, const std::string& layer, bool bwd, int mode, const void* in, int in_nb,
                       int B, int Hin, int Win, bool relu, const E& e) {
    auto it = c->l32.find(layer);
    if (it == c->l32.end()) return c->fail("unknown 32->32 layer " + layer, -2);
    a.in = in; a.in_nb = in_nb; a.w = bwd ? &it->second.b : &it->second.f;
    a.bias = bwd ? nullptr : (layer == "conv1_rgb_meta" ? c->meta_b : it->second.bias);
    a.up = e.up; a.up_nb = e.up_nb; a.mask = e.mask; a.mask_nb = e.mask_nb;
    a.add1 = e.add1; a.add1_nb = e.add1_nb; a.add2 = e.add2; a.add2_nb = e.add2_nb;
    a.out_raw = e.raw; a.out_sum = e.sum;
    const bool nar = e.nar || (bwd && c->nar_bwd);
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
    return 0;
}

// algorithmic bytes and MACs of one 32 -> 32 launch (SURVEY.md 8d counting rule): input + output + weight elements x element size,
// output pixels x 9 x 32 x 32
static void conv32_cost(int mode, int B, int Hin, int Win, int es_l, double& bytes, double& macs) {
    const long pin = (long)B * Hin * Win;
    const long pout = mode == CONV_S1 ? pin : (mode == CONV_S2 ? pin / 4 : pin * 4);
    bytes = (double)((pin + pout) * 32 + 9216) * es_l;
    macs = (double)(mode == CONV_T2 ? pin : pout) * 9.0 * 32.0 * 32.0;
}

int conv32(ptta_ctx* c, hipStream_t s, const std::string& layer, bool bwd, int mode, const void* in, int in_nb,
           int B, int Hin, int Win, bool relu, const E& e) {
    Conv32Args a;
    { const int rc = conv32_args(c, a, layer, bwd, mode, in, in_nb, B, Hin, Win, relu, e); if (rc) return rc; }
    const bool nar = e.nar || (bwd && c->nar_bwd);
    const int es_l = nar ? 2 : c->es;
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

// A stride-2 layer and the stride-1 layer that consumes its output (`fe.sum` when the first layer has one, else `fe.raw`; both stay side
// outputs), forward (ReLU on both inputs) or data gradients (bwd, no ReLU): ONE launch where the stride-1
// half would take the small-map kernel, the arithmetic is the default one, option "pair_fuse" is on and the pair's epilogue combination is
// instantiated (conv_pair.hip); otherwise exactly the two conv32() calls.
int conv32_pair(ptta_ctx* c, hipStream_t s, bool bwd, const std::string& first, const void* in, int in_nb, int B, int Hin, int Win, const E& fe,
                const std::string& second, int mid_nb, const E& se) {
    const int Hm = Hin / 2, Wm = Win / 2;
    const bool relu = !bwd;
    void* const mid = fe.sum ? fe.sum : fe.raw;
    const bool nar = fe.nar || (bwd && c->nar_bwd);
    if (c->pair_fuse && !c->naive && (c->x3 || c->bf16 || nar) && fe.nar == se.nar && mid) {
        Conv32Args f, g;
        { const int rc = conv32_args(c, f, first, bwd, CONV_S2, in, in_nb, B, Hin, Win, relu, fe); if (rc) return rc; }
        { const int rc = conv32_args(c, g, second, bwd, CONV_S1, mid, mid_nb, B, Hm, Wm, relu, se); if (rc) return rc; }
        if (mid_nb == B && ptta_conv32_pair_applies(f, g)) {
            const int es_l = nar ? 2 : c->es;
            double b1, m1, b2, m2;
            conv32_cost(CONV_S2, B, Hin, Win, es_l, b1, m1); conv32_cost(CONV_S1, B, Hm, Wm, es_l, b2, m2);
            // (both layers' algorithmic bytes and MACs as counted for the two launches: the launch executes both)
            ProfScope ps(c, 5, s, b1 + b2, m1 + m2, 1);
            const int rc = ptta_launch_conv32_pair(f, g, s);
            if (rc == 1) return c->fail("conv32_pair: fused form refused a case its own test accepted", -22);
            if (rc == 0) c->pair_fuse_count++;
            return rc;
        }
    }
    { const int rc = conv32(c, s, first, bwd, CONV_S2, in, in_nb, B, Hin, Win, relu, fe); if (rc) return rc; }
    return conv32(c, s, second, bwd, CONV_S1, mid, mid_nb, B, Hm, Wm, relu, se);
}

// A transposed layer and the stride-1 layer that consumes its output (`fe.sum` when the first layer has one, else `fe.raw`), forward (ReLU
// on both inputs) or data gradients (bwd, no ReLU): ONE launch at every map size where the arithmetic is the default one, option
// "tpair_fuse" is on and the pair's epilogue combination is instantiated (conv_tpair.hip); otherwise exactly the two conv32() calls.
// Forward: nothing but the stride-1 layer reads the VALUES of the intermediate map -- the backward masks with its sign-bit words (real
// frames, written by the fused launch as by the transposed one) and no other launch names it -- so the fused launch writes the map only
// where the backward would read it as a float mask (no bit plane: option "mask_bits" 0); ptta_debug_tensor refuses such a map while
// that holds (ptta_ctx::tpair_unwritten).  Data gradients: the first layer's SUM is still written (the side upsamplings read it).
// (f, g: the two launches' arguments; returns whether the pair takes the one launch as the handle is configured now)
static bool tpair_takes(ptta_ctx* c, Conv32Args& f, Conv32Args& g, bool bwd, const std::string& first, const void* in, int in_nb, int B, int Hin, int Win,
                        const E& fe, const std::string& second, int mid_nb, const E& se) {
    void* const mid = fe.sum ? fe.sum : fe.raw;
    const bool nar = fe.nar || (bwd && c->nar_bwd);
    if (!(c->tpair_fuse && !c->naive && (c->x3 || c->bf16 || nar) && fe.nar == se.nar && mid)) return false;
    if (conv32_args(c, f, first, bwd, CONV_T2, in, in_nb, B, Hin, Win, !bwd, fe)) return false;
    if (conv32_args(c, g, second, bwd, CONV_S1, mid, mid_nb, B, Hin * 2, Win * 2, !bwd, se)) return false;
    return mid_nb == B && ptta_conv32_tpair_applies(f, g) && ptta_conv32_tpair_pays(f, g);
}
bool conv32_tpair_takes(ptta_ctx* c, bool bwd, const std::string& first, const void* in, int in_nb, int B, int Hin, int Win, const E& fe,
                        const std::string& second, int mid_nb, const E& se) {
    Conv32Args f, g;
    return tpair_takes(c, f, g, bwd, first, in, in_nb, B, Hin, Win, fe, second, mid_nb, se);
}
int conv32_tpair(ptta_ctx* c, hipStream_t s, bool bwd, const std::string& first, const void* in, int in_nb, int B, int Hin, int Win, const E& fe,
                 const std::string& second, int mid_nb, const E& se) {
    const int Hm = Hin * 2, Wm = Win * 2;
    const bool relu = !bwd;
    void* const mid = fe.sum ? fe.sum : fe.raw;
    const bool nar = fe.nar || (bwd && c->nar_bwd);
    {
        Conv32Args f, g;
        if (tpair_takes(c, f, g, bwd, first, in, in_nb, B, Hin, Win, fe, second, mid_nb, se)) {
            // the map's only other reader is a backward that masks with the float map: fp32 storage without a bit plane (where there is one it
            // covers the real frames, the only ones the backward masks); the source model has no backward: it never writes the map
            if (!bwd && (nar || f.bits_out != nullptr || c->plain)) { f.out_raw = nullptr; c->tpair_unwritten.insert(fe.raw); }
            else if (!bwd) c->tpair_unwritten.erase(fe.raw);
            const int es_l = nar ? 2 : c->es;
            double b1, m1, b2, m2;
            conv32_cost(CONV_T2, B, Hin, Win, es_l, b1, m1); conv32_cost(CONV_S1, B, Hm, Wm, es_l, b2, m2);
            // (both layers' algorithmic bytes and MACs as counted for the two launches: the launch executes both)
            const bool small = (long)Hin * Win <= (long)c->H4 * c->W4;
            ProfScope ps(c, 4 + (small ? 1 : 0), s, b1 + b2, m1 + m2, 1);
            const int rc = ptta_launch_conv32_tpair(f, g, 0, 0, s);
            if (rc == 1) return c->fail("conv32_tpair: fused form refused a case its own test accepted", -22);
            if (rc == 0) c->tpair_fuse_count++;
            return rc;
        }
    }
    if (!bwd) c->tpair_unwritten.erase(fe.raw);
    { const int rc = conv32(c, s, first, bwd, CONV_T2, in, in_nb, B, Hin, Win, relu, fe); if (rc) return rc; }
    return conv32(c, s, second, bwd, CONV_S1, mid, mid_nb, B, Hm, Wm, relu, se);
}

int conv32w(ptta_ctx* c, hipStream_t s, const ConvW* w, const float* bias, const void* in, int in_nb, int B, int H, int W, const E& e) {
    Conv32Args a;
    a.in = in; a.in_nb = in_nb; a.w = w; a.bias = bias;
    a.add1 = e.add1; a.add1_nb = e.add1_nb; a.out_raw = e.raw; a.out_sum = e.sum;
    a.B = B; a.Hin = H; a.Win = W; a.mode = CONV_S1; a.relu_in = 0; a.bf16 = c->bf16; a.naive = c->naive; a.x3 = c->x3;
    return ptta_launch_conv32(a, s);
}

// Conv2d(cin <= 3, 32) - ReLU - Conv2d(32, 32) of an encoder stage's `init` block: ONE launch where the fused form applies
// (conv32_first.hip conv32_s1_first_kernel; PTTA_FUSE_FIRST=0 or any other mode: the two launches).  `f`: the first convolution (out_raw = where
// its pre-activation map goes), a_nb: how many leading frames of that map are still needed (the backward's ReLU mask), 0: none.
static int conv32_first(ptta_ctx* c, hipStream_t s, const std::string& layer, ConvInArgs& f, int a_nb, int B, int H, int W, const E& e) {
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
// prdct.1 (mask epilogue) -- the d v map is never written (conv32_first.hip conv32_s1_first_kernel<1, false, true, false, true>).  Large maps only.
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


// conv1_rgb_meta forward.  1layer: one conv (:1065-1071).  2layers: Res_Conv(32,128) (:28-36); in training
// mode each pass (real frames, proxy frames) is a separate forward call in the reference, so BatchNorm
// statistics are per pass and the running statistics are updated once per pass, real frames first.
static int meta_forward(ptta_ctx* c, bool train, int B, hipStream_t s) {
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
        // one matrix-core launch per convolution on NHWC-128 tensors (gconv_x3_s1.hip), BatchNorm statistics reduced in the
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


// mixed mode: the adapted layer on the proxy frames (narrow).  1layer: the same convolution on the narrow copy of the zero-image features;
// 2layers: the fp32 Res_Conv block above ran on both passes (its BatchNorm statistics are per pass), the proxy half is narrowed here.
int to_narrow(ptta_ctx* c, const void* src_f32, void* dst, long n, hipStream_t s) {
    if (!src_f32 || !dst) return c->fail("to_narrow: missing narrow twin", -22);
    ProfScope ps_(c, 8, s, 0, 0, 1);
    from_f32_launch((const float*)src_f32, (bf16_t*)dst, n, s);
    return 0;
}
int to_wide(ptta_ctx* c, const void* src_nar, float* dst, long n, hipStream_t s) {
    if (!src_nar || !dst) return c->fail("to_wide: missing operand", -22);
    ProfScope ps_(c, 8, s, 0, 0, 1);
    to_f32_launch((const bf16_t*)src_nar, dst, n, s);
    return 0;
}
static int meta_forward_proxy(ptta_ctx* c, hipStream_t s) {
    const int H4 = c->H4, W4 = c->W4, Nn = c->Nn;
    const long half = (long)Nn * H4 * W4 * 32;
    if (c->meta_mode == PTTA_META_1LAYER) {
        E e; e.raw = c->tw(c->m); e.nar = true;
        return conv32(c, s, "conv1_rgb_meta", false, CONV_S1, c->tw(c->c2), Nn, Nn, H4, W4, false, e);
    }
    return to_narrow(c, (const float*)c->m + half, c->tw(c->m), half, s);
}


// RGBEncoder.forward (:252-264) on `nb` frames written at batch offset `boff` of the c0..c4 buffers; frames with index
// >= zero_from_b see a zero image (the proxy pass's torch.zeros_like(rgb), :511).
int rgb_encoder(ptta_ctx* c, const float* image, int nb, int boff, int zero_from_b, hipStream_t s) {
    const int H1 = c->Hp, W1 = c->Wp, H2 = c->H2, W2 = c->W2, H4 = c->H4, W4 = c->W4, H8 = c->H8, W8 = c->W8, H16 = c->H16, W16 = c->W16;
    auto at = [&](void* base, int h, int w) { return (void*)((char*)base + (size_t)boff * h * w * 32 * c->es); };
    auto e_raw = [](void* raw) { E e; e.raw = raw; return e; };
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
    return 0;
}

// The proxy pass feeds torch.zeros_like(rgb) through the frozen RGB encoder (:509-515): its c0..c4 depend only on the
// encoder weights and the frame size, so they are computed ONCE per (handle, weights) into the proxy half of the
// buffers instead of in every step (the eval forward only writes the real half).  Never runs inside a graph capture.
int ensure_fused_heads(ptta_ctx* c, hipStream_t s) {
    if (c->fused_pp_valid || !c->fuse_heads) return 0;
    Lin& f = c->fused_pp; const Lin& a = c->fc["proj.3"]; const Lin& b = c->fc["pred.0"];
    fuse_linear_launch(b.W, b.bias, a.W, a.bias, f.W, f.bias, 512, 512, 512, s);
    ptta_split_weight(f.W, f.Whi, f.Wlo, f.Wil, 512L * 512, 512, s);
    ptta_hn_pack_w(f.Whi, f.Wsl, 512, s);
    c->fused_pp_valid = true;
    return 0;
}

int ensure_proxy_rgb(ptta_ctx* c, const float* any_image, hipStream_t s) {
    RUN(ensure_fused_heads(c, s));
    if (c->proxy_valid) return 0;
    RUN(rgb_encoder(c, any_image, c->Nn, c->Nn, 0, s));
    if (c->nar_proxy) {      // what the proxy chain reads of it: the skip operands c1 .. c4 and the adapted layer's input c2, as narrow maps
        const int Nn = c->Nn;
        struct { void* p; int h, w; } maps[4] = {{c->c1, c->H2, c->W2}, {c->c2, c->H4, c->W4}, {c->c3, c->H8, c->W8}, {c->c4, c->H16, c->W16}};
        for (auto& m_ : maps) {
            const long half = (long)Nn * m_.h * m_.w * 32;
            RUN(to_narrow(c, (const float*)m_.p + half, c->tw(m_.p), half, s));
        }
    }
    c->proxy_valid = true;
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
static int backbone(ptta_ctx* c, const float* image, bool train, hipStream_t s) {
    hipStream_t s2 = train ? c->aux(s) : nullptr;
    const int Nn = c->Nn, B2 = train ? 2 * Nn : Nn;
    const bool two = train && c->nar_proxy;
    const int H1 = c->Hp, W1 = c->Wp, H2 = c->H2, W2 = c->W2, H4 = c->H4, W4 = c->W4, H8 = c->H8, W8 = c->W8, H16 = c->H16, W16 = c->W16;
    auto e_raw = [](void* raw) { E e; e.raw = raw; return e; };
    // ---- RGB encoder (RGBEncoder.forward :252-264) + meta layer (:481-482) ----
    // train: the proxy half of c0..c4 (zero image through frozen weights) is a constant of the handle, computed once by
    // ensure_proxy_rgb(); only the real frames go through the encoder here
    if (!c->skip_prefix) RUN(rgb_encoder(c, image, Nn, 0, Nn, s));
    if (!c->plain) RUN(meta_forward(c, train, B2, s));      // (the source model: the three readers of `m` take c2, ptta_ctx::meta_out)
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
        { E e; e.nar = nar; e.raw = A(c->y4, H4, W4); e.sum = A(c->s0_1, H4, W4); e.add1 = e1_0; e.add1_nb = Nn; e.add2 = A(c->meta_out(), H4, W4); e.add2_nb = Bl;
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
            RUN(conv32_first(c, st, "depth_encoder2.init.2", a, (b0 == 0 && !nar && !c->plain) ? Nn : 0, Bl, H2, W2, e));
        }
        // (each stride-2 layer and the stride-1 layer behind it: one launch on small maps, conv32_pair)
        { E e; e.nar = nar; e.raw = A(c->e2_1, H4, W4); e.up = A(c->y3, H8, W8); e.up_nb = Bl;
          RUN(conv32_pair(c, st, false, "depth_encoder2.enc1.1", A(c->e2_0, H2, W2), Bl, Bl, H2, W2, raw(A(c->e2_1a, H4, W4)), "depth_encoder2.enc1.3", Bl, e)); }
        { E e; e.nar = nar; e.sum = A(c->z2, H8, W8); e.up = A(c->y2, H16, W16); e.up_nb = Bl; e.add1 = A(c->c3, H8, W8); e.add1_nb = Bl;            // z2 = e2_2 + c3
          RUN(conv32_pair(c, st, false, "depth_encoder2.enc2.1", A(c->e2_1, H4, W4), Bl, Bl, H4, W4, raw(A(c->e2_2a, H8, W8)), "depth_encoder2.enc2.3", Bl, e)); }
        // (each transposed layer and the stride-1 layer behind it: one launch, conv32_tpair)
        { E e; e.nar = nar; e.raw = A(c->z3, H4, W4); e.sum = A(c->s1_2, H4, W4); e.add1 = A(c->e2_1, H4, W4); e.add1_nb = Bl; e.add2 = A(c->meta_out(), H4, W4); e.add2_nb = Bl;
          RUN(conv32_tpair(c, st, false, "depth_decoder2.dec2.1", A(c->z2, H8, W8), Bl, Bl, H8, W8, raw(A(c->t2, H4, W4)), "depth_decoder2.dec2.3", Bl, e)); }
        { E e; e.nar = nar; e.raw = A(c->z4, H2, W2); e.sum = A(c->s0_2, H2, W2); e.add1 = A(c->e2_0, H2, W2); e.add1_nb = Bl; e.add2 = A(c->c1, H2, W2); e.add2_nb = Bl;
          RUN(conv32_tpair(c, st, false, "depth_decoder2.dec1.1", A(c->s1_2, H4, W4), Bl, Bl, H4, W4, raw(A(c->u2, H2, W2)), "depth_decoder2.dec1.3", Bl, e)); }
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
            RUN(conv32_first(c, st, "depth_encoder3.init.2", a, (b0 == 0 && !nar && !c->plain) ? Nn : 0, Bl, H1, W1, e));
        }
        CR("depth_encoder3.enc1.1", false, CONV_S2, A(c->e3_0, H1, W1), Bl, Bl, H1, W1, true, raw(A(c->e3_1a, H2, W2)));
        { E e; e.nar = nar; e.raw = A(c->e3_1, H2, W2); e.up = A(c->z3, H4, W4); e.up_nb = Bl; CR("depth_encoder3.enc1.3", false, CONV_S1, A(c->e3_1a, H2, W2), Bl, Bl, H2, W2, true, e); }
        { E e; e.nar = nar; e.raw = A(c->feat, H4, W4); e.up = A(c->z2, H8, W8); e.up_nb = Bl; e.add1 = A(c->meta_out(), H4, W4); e.add1_nb = Bl;   // w2 = feat + m
          if (!nar) e.sum = A(c->w2, H4, W4); else e.add1 = nullptr;         // (the proxy pass stops at depth_encoder3: its w2 feeds nothing)
          RUN(conv32_pair(c, st, false, "depth_encoder3.enc2.1", A(c->e3_1, H2, W2), Bl, Bl, H2, W2, raw(A(c->e3_2a, H4, W4)), "depth_encoder3.enc2.3", Bl, e)); }
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
    { E e; e.sum = c->s1_3; e.add1 = c->e3_1; e.add1_nb = B2; e.add2 = c->c1; e.add2_nb = B2;
      RUN(conv32_tpair(c, s, false, "depth_decoder3.dec2.1", c->w2, B2, Nn, H4, W4, e_raw(c->t3), "depth_decoder3.dec2.3", Nn, e)); }
    { E e; e.sum = c->s0_3; e.add1 = c->e3_0; e.add1_nb = B2; e.add2 = c->c0; e.add2_nb = B2;
      RUN(conv32_tpair(c, s, false, "depth_decoder3.dec1.1", c->s1_3, Nn, Nn, H2, W2, e_raw(c->u3), "depth_decoder3.dec1.3", Nn, e)); }
    CV("depth_decoder3.prdct.1", false, CONV_S1, c->s0_3, Nn, Nn, H1, W1, true, e_raw(c->v3));
    {
        const LOut& lo = c->lout["depth_decoder3.prdct.3"];
        ConvOut1Args a; a.in = c->v3; a.in_nb = Nn; a.w = lo.w; a.bias = lo.bias; a.add = c->p11; a.add_nb = B2; a.out = c->depth_net;
        a.B = Nn; a.H = H1; a.W = W1; a.relu_in = 1; a.bf16 = c->bf16;                           // output = out3 + p11 (:506)
        RUN(conv_out1_p(c, a, s));
    }
    }
    c->stamp(7, s);
    if (train) {
        if (s2) { if (!c->thru_active) HIPCHK(hipStreamWaitEvent(s, c->ev_join, 0)); }      // (thru: the heads' stream goes on into the loss and the backward)
        else RUN(heads_forward(c, s));
    }
    return 0;
}

bool heads_v2_on(const ptta_ctx* c) {
    return c->heads_v2 && c->fuse_heads && c->fused_pp_valid && c->x3 && !c->bf16 && !c->naive && !c->skip_dec3 && !c->head_swap;
}

// proj / pred heads (:551-554): emb = pred(proj(feat_zero)), ref = proj(feat); BN1d in train mode.
static int mlp_forward(ptta_ctx* c, const std::string& name, const void* A, int a_bf16, int K, float* hidden, float* out, hipStream_t s) {
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
        pad_dual_launch(image, c->img_pad, c->N, 3, c->H, c->W, c->Hp, c->Wp, c->pt, c->pr, s, c->img_norm);
        pad_dual_launch(sparse, c->sp_pad, c->N, 1, c->H, c->W, c->Hp, c->Wp, c->pt, c->pr, s);
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
    } else if (!c->plain) {
        c->stamp(0, s);
        const L32& ml = c->l32["conv1_rgb_meta"];
        { ProfScope ps_(c, 8, s, 0, 0, 1); ptta_pack_conv32(c->meta_w, ml.f, 0, 0, s); }
    }
    RUN(backbone(c, img, train, s));
    if (c->dual)
        crop_avg_launch(c->depth_net, c->depth_final, c->N, c->H, c->W, c->Hp, c->Wp, c->pt, c->pr, s);
    return 0;
}

const float* final_depth(ptta_ctx* c) { return c->dual ? c->depth_final : c->depth_net; }

}  // namespace msgchn
