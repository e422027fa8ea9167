// Stand-alone launches of the update half of a step, for tests (include/ptta.h states the arguments and the -22 rules): the weight
// gradients (ptta_op_wgrad32, ptta_op_gwgrad_view, ptta_op_linear_wgrad, ptta_op_glinear_wgrad) and the optimizer (ptta_op_adam,
// ptta_op_adam_multi, ptta_op_ema_multi).  Each hook passes its arguments through to the launcher the engines call, owns the partial
// buffers and device tables for the length of the call, and synchronises.
#include <vector>

#include "../../include/ptta.h"
#include "ptta_common.h"
#include "ptta_kernels.h"

namespace {
// device memory owned for the length of one call
struct Scratch {
    void* p = nullptr;
    bool ok;
    explicit Scratch(size_t bytes) { ok = hipMalloc(&p, bytes ? bytes : 4) == hipSuccess; }
    ~Scratch() { if (p) (void)hipFree(p); }
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
};
int finish(int rc, hipStream_t s) {
    if (rc > 0) rc = -5;
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = -5;
    return rc;
}
// the device PttaAdamEntry table of host arrays, offsets running as msgchn::ensure_adam_table lays them out
int upload_table(const std::vector<PttaAdamEntry>& host, const Scratch& tab, hipStream_t s) {
    if (hipMemcpyAsync(tab.p, host.data(), host.size() * sizeof(PttaAdamEntry), hipMemcpyHostToDevice, s) != hipSuccess) return -5;
    return hipStreamSynchronize(s) == hipSuccess ? 0 : -5;          // (the host vector may go before the copy is read otherwise)
}
}  // namespace

extern "C" {

int ptta_op_wgrad32(const void* x, const void* gy, int bf16, int b, int h, int w, float* gw, float* gb, int co_stride, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!x || !gy || !gw || b < 1 || h < 1 || w < 1 || co_stride < 288 || (double)b * h * w * 32 > 2.0e9) return -22;
    Scratch part((size_t)ptta_wgrad_chunks((long)b * h * w) * 10 * 1024 * 4);
    if (!part.ok) return -12;
    return finish(ptta_launch_wgrad32(x, gy, bf16 ? 1 : 0, b, h, w, (float*)part.p, gw, gb, s, co_stride), s);
}

int ptta_op_gwgrad_view(const ptta_gwgrad_view_args* a, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!a || !a->x || !a->gy || !a->gw || a->b < 1 || a->h < 1 || a->w < 1 || a->ci < 1 || a->co < 1 || a->ci > 256 || a->co > 256 ||
        a->ldx < a->ci || a->ldg < a->co) return -22;
    if (a->pw && (!a->mw || !a->vw || !a->hyper || !a->step || !a->ticket || (a->pb && (!a->mb || !a->vb)))) return -22;
    GView xv, gv;
    xv.p = (float*)a->x; xv.B = a->b; xv.H = a->h; xv.W = a->w; xv.C = a->ci; xv.ld = a->ldx;
    gv.p = (float*)a->gy; gv.B = a->b; gv.H = a->h; gv.W = a->w; gv.C = a->co; gv.ld = a->ldg;      // (gy_bf16: bf16 elements behind the pointer)
    Scratch part((size_t)ptta_gwgrad_mfma_part_floats((long)a->b * a->h * a->w, a->ci, a->co) * 4);
    if (!part.ok) return -12;
    GwAdam ad;
    ad.pw = a->pw; ad.mw = a->mw; ad.vw = a->vw; ad.pb = a->pb; ad.mb = a->mb; ad.vb = a->vb; ad.hyper = a->hyper; ad.step = a->step; ad.ticket = a->ticket;
    return finish(ptta_launch_gwgrad_mfma(xv, gv, (float*)part.p, a->gw, a->gb, s, a->gy_bf16 ? 1 : 0, a->pw ? &ad : nullptr), s);
}

int ptta_op_adam(float* p, float* m, float* v, const float* g, long long n, const float* hyper, int* step, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!p || !m || !v || !g || !hyper || !step || n < 1) return -22;
    int rc = ptta_launch_step_inc(step, s);
    if (!rc) rc = ptta_launch_adam(p, m, v, g, (long)n, hyper, step, s);
    return finish(rc, s);
}

int ptta_op_adam_multi(int nt, float* const* p, float* const* m, float* const* v, const float* const* g, const long long* n, const int* rep,
                       const float* hyper, int* step, unsigned* ticket, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (nt < 1 || !p || !m || !v || !g || !n || !hyper || !step || !ticket) return -22;
    std::vector<PttaAdamEntry> host((size_t)nt);
    long off = 0;
    for (int k = 0; k < nt; ++k) {
        const int r = rep ? rep[k] : 1;
        if (n[k] < 1 || r < 0 || (r != 0 && (!p[k] || !m[k] || !v[k] || !g[k]))) return -22;
        host[k] = PttaAdamEntry{p[k], m[k], v[k], g[k], (long)n[k], off, r};
        off += (long)n[k];
    }
    Scratch tab(host.size() * sizeof(PttaAdamEntry));
    if (!tab.ok) return -12;
    int rc = upload_table(host, tab, s);
    if (!rc) rc = ptta_launch_adam_multi((const PttaAdamEntry*)tab.p, nt, off, hyper, step, ticket, s);
    return finish(rc, s);
}

int ptta_op_ema_multi(int nt, float* const* p, const float* const* g, const long long* n, const float* tau_dev, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (nt < 1 || !p || !g || !n || !tau_dev) return -22;
    std::vector<PttaAdamEntry> host((size_t)nt);
    long off = 0;
    for (int k = 0; k < nt; ++k) {
        if (n[k] < 1 || !p[k] || !g[k]) return -22;
        host[k] = PttaAdamEntry{p[k], nullptr, nullptr, g[k], (long)n[k], off, 1};
        off += (long)n[k];
    }
    Scratch tab(host.size() * sizeof(PttaAdamEntry));
    if (!tab.ok) return -12;
    int rc = upload_table(host, tab, s);
    if (!rc) rc = ptta_launch_ema_multi((const PttaAdamEntry*)tab.p, nt, off, tau_dev, s);
    return finish(rc, s);
}

int ptta_op_linear_wgrad(const ptta_linear_wgrad_args* a, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!a || !a->G || !a->X || !a->dW || a->o < 1 || a->i < 1) return -22;
    if (a->Gh && (!a->gscale || !a->gc1 || !a->gc2 || !a->gmean || !a->ginv)) return -22;
    if (a->xscale && !a->xshift) return -22;
    const int chunks = a->r > 0 ? ptta_linear_wgrad_chunks((long)a->r, nullptr) : 1;
    Scratch wpart((size_t)chunks * a->o * a->i * 4), bpart((size_t)chunks * a->o * 4);
    if (!wpart.ok || !bpart.ok) return -12;
    LinWgradArgs l;
    l.G = a->G; l.Gh = a->Gh; l.gscale = a->gscale; l.gc1 = a->gc1; l.gc2 = a->gc2; l.gmean = a->gmean; l.ginv = a->ginv;
    l.X = a->X; l.xscale = a->xscale; l.xshift = a->xshift; l.Wpart = (float*)wpart.p; l.bpart = (float*)bpart.p;
    l.R = (long)a->r; l.O = a->o; l.I = a->i;
    return finish(ptta_launch_linear_wgrad(l, a->dW, a->db, s), s);
}

int ptta_op_glinear_wgrad(const float* x, int ldx, int i, const float* gy, int ldg, int o, long long r, float* gw, float* gb, ptta_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    if (!x || !gy || i < 1 || o < 1 || ldx < i || ldg < o || r > 2000000000LL) return -22;
    GView xv, gv;
    xv.p = (float*)x; xv.B = 1; xv.H = 1; xv.W = (int)r; xv.C = i; xv.ld = ldx;
    gv.p = (float*)gy; gv.B = 1; gv.H = 1; gv.W = (int)r; gv.C = o; gv.ld = ldg;
    return finish(ptta_launch_glinear_wgrad(xv, gv, gw, gb, s), s);
}

}  // extern "C"
