// The weight gradient of a stride-1 3x3 convolution on the matrix cores (gconv_mfma.hip has the map of the files): the fp32-MFMA form, the
// bf16x3 forms, the fixed-order reducer they share and the launcher that chooses among them.  The generic engines and the MSG_CHN step
// (msgchn_backward.hip) both launch it.
#include "ptta_common.h"
#include "ptta_kernels.h"

namespace {

// ---- weight gradient of a stride-1 3x3 convolution with up to 64 x 64 channels (the adapted conv1_rgb_meta,
// Conv2d(48,48,3,1,1), nlspnmodel_adapt.py:1371) on the fp32 matrix cores: dW[co][ci][tap] = sum_p gy[p][co] x[p+tap][ci].
// One wave per (pixel chunk, 32x32 channel-block pair): nine 32x32 accumulators (one per tap) + one for the bias,
// K = pixels, two pixels per v_mfma_f32_32x32x2_f32; a second fixed-order pass sums the chunk partials.
#define GWG_PART (10 * 1024)
__global__ __launch_bounds__(64) void gwgrad_mfma_kernel(GView x, GView gy, int nchunks, int ncib, float* __restrict__ part) {
    const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
    const int H = x.H, W = x.W;
    const long P = (long)x.B * H * W;
    const long per = ((P + nchunks - 1) / nchunks + 7) & ~7L;
    const long p0 = (long)blockIdx.x * per;
    long p1 = p0 + per; if (p1 > P) p1 = P;
    const int cob = blockIdx.y / ncib, cib = blockIdx.y % ncib;
    const int co = cob * 32 + i, ci = cib * 32 + i;
    const bool cov = co < gy.C, civ = ci < x.C;
    f32x16 acc[10];
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    for (long pp = p0; pp < p1; pp += 8) {
        float a[4], bv[4][9];
        bool pv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long pix = pp + 2 * u + h;
            pv[u] = pix < p1;
            int px = 0, py = 0;
            a[u] = 0.f;
            if (pv[u]) {
                px = (int)(pix % W); py = (int)((pix / W) % H);
                if (cov) a[u] = gy.p[pix * gy.ld + co];
            }
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int yy = py + tap / 3 - 1, xx = px + tap % 3 - 1;
                bv[u][tap] = 0.f;
                if (pv[u] && civ && yy >= 0 && yy < H && xx >= 0 && xx < W) bv[u][tap] = x.p[(pix + (long)(tap / 3 - 1) * W + (tap % 3 - 1)) * x.ld + ci];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) acc[tap] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], bv[u][tap], acc[tap], 0, 0, 0);
            acc[9] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], pv[u] ? 1.f : 0.f, acc[9], 0, 0, 0);
        }
    }
    float* out = part + ((long)blockIdx.x * gridDim.y + blockIdx.y) * GWG_PART;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(tap * 32 + acc_row(r, h)) * 32 + i] = acc[tap][r];
    if (i == 0)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[9 * 1024 + acc_row(r, h)] = acc[9][r];
}

// ---- the same weight gradient on the bf16 matrix cores (bf16x3), for Ci, Co <= 64: dW[co][ci][tap] = sum_p gy[p][co] x[p+tap][ci] as a
// reduction-GEMM over pixels, like head_train.hip's Linear gradient: an MFMA lane holds 8 consecutive k for one m, and with
// k = pixel, m = channel those are 8 consecutive PIXELS of one channel -- 8 dword loads per fragment, straight from global.
// Block = 4 waves = the (co tile, ci tile) pairs of a 64 x 64 problem; a K step is 16 consecutive pixels of one image row.
// Per row offset dy the lane loads x[row + dy][p - 1 .. p + 8] ONCE (10 loads) and the three horizontal taps are register
// renames of it (v[0..7], v[1..8], v[2..9]): 38 loads per step instead of 80.  Nine 32 x 32 accumulators per wave; the next
// step's loads are issued before the current step's 27 MFMAs.  Partials in the layout of gwgrad_mfma_kernel (same reducer).
// 352x1216, Conv2d(48,48,3): 876 -> see DESIGN.md (the fp32 form alternated a 40-load phase and a 40-MFMA phase per 8 pixels).
// single = 1 (Ci, Co <= 32): one tile pair; the four waves take different items instead and write a partial each.
// BLKRED (single only): the four waves' partial tiles are summed inside the block in a fixed tree ((w0 + w2) + (w1 + w3)) through LDS and the
// block writes ONE partial -- four times the waves for the same partial traffic: the launch is a latency chain of ~2 us per item and wave
// (38 strided loads, then 27 MFMAs), so its duration is the items per wave.
// WIDE (channel counts up to 256 x 256 outside the forms above: NLSPN's 48 <-> 256 and CostDCNet's 16 -> 64 of the 2layers meta block):
// grid (item chunks, pair groups); the ncib x ncob tile pairs, pair = cob * ncib + cib, are taken four per block (blockIdx.y = group of
// four consecutive pairs; waves past the last pair return), or -- fewer than four pairs -- wpp = 4 / npairs waves per pair that split its
// items.  Partials [chunk = blockIdx.x * wpp + sub][pair], the layout of gwgrad_mfma_kernel (same reducer, npairs of them per chunk).
template <bool GY16, bool BLKRED = false, bool WIDE = false>  // GY16: gy.p points at bf16 values (the narrow gradient maps of the MSG_CHN mixed mode): widened on load, the same products
__global__ __launch_bounds__(256) void gwgrad_x3_kernel(GView x, GView gy, int nitems_x, int single, int ncib, float* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, hg = lane >> 5;
    const int npairs = WIDE ? ncib * ((gy.C + 31) >> 5) : 4;
    const int wpp = WIDE && npairs < 4 ? 4 / npairs : 1;                   // waves per pair (WIDE only)
    const int pair = WIDE ? (int)blockIdx.y * (4 / wpp) + wave / wpp : wave, sub = WIDE ? wave % wpp : 0;
    if (WIDE && pair >= npairs) return;                                   // (wave-uniform; no barrier in this form)
    // the four waves of a block = the four (ci tile, co tile) pairs: 2 x 2 (<= 64 x 64 channels), 1 x 4 (32 -> 128) or 4 x 1 (128 -> 32)
    const int cob = single ? 0 : pair / ncib, cib = single ? 0 : pair % ncib;
    const int H = x.H, W = x.W;
    const int co = cob * 32 + c, ci = cib * 32 + c;
    const bool cov = co < gy.C, civ = ci < x.C;
    // Addresses = uniform base + 32-bit BYTE offset (maps < 4 GB, checked by the launcher).  The item is wave-uniform (scalar row / image
    // arithmetic), a lane adds its channel and its half's eight pixels; clamps are selects between precomputed offsets.  The first form --
    // 64-bit element indices from a lane-varying item, clamp, multiply by the row pitch per load -- spent ~190 quarter-rate integer
    // multiplies per item: 3 k of the ~4.5 k cycles an item took (round 5, .s).
    constexpr unsigned GE = GY16 ? 2u : 4u;
    const unsigned gld = (unsigned)gy.ld * GE, xld = (unsigned)x.ld * 4u;
    const unsigned glane = (unsigned)(cov ? co : 0) * GE + (hg ? 8u * gld : 0u), xlane = (unsigned)(civ ? ci : 0) * 4u + (hg ? 8u * xld : 0u);
    const char* const gbase = (const char*)gy.p;
    const char* const xbase = (const char*)x.p;
    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float bsum = 0.f;
    const int nitems = x.B * H * nitems_x;                            // item = 16 consecutive pixels of one row
    struct Regs { float g[8]; float v[3][10]; unsigned gm, vm[3]; };      // raw loads + validity bits (zero-fill happens at use: no wait at the load)
    auto fetch = [&](int item, Regs& r) __attribute__((always_inline)) {
        const int xs = item % nitems_x; const int t_ = item / nitems_x;
        const int y = t_ % H; const int b = t_ / H;
        const int p0 = xs * 16 + 8 * hg;                               // this lane's first pixel of the step
        const unsigned rowpix = (unsigned)((b * H + y) * W);
        const unsigned g0 = (rowpix + (unsigned)(xs * 16)) * gld + glane;
        const unsigned glast = (rowpix + (unsigned)(W - 1)) * gld + (unsigned)(cov ? co : 0) * GE;
        r.gm = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool ok = p0 + j < W;
            const unsigned off = ok ? g0 + (unsigned)j * gld : glast;
            if constexpr (GY16) r.g[j] = __uint_as_float((unsigned)*(const bf16_t*)(gbase + off) << 16);
            else r.g[j] = *(const float*)(gbase + off);
            r.gm |= (ok && cov) ? (1u << j) : 0u;
        }
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int yy = y + dy - 1;
            const bool rok = yy >= 0 && yy < H;
            const unsigned rp = (unsigned)((b * H + min(max(yy, 0), H - 1)) * W);
            const unsigned x0 = (rp + (unsigned)(xs * 16)) * xld + xlane;          // pixel p0 of the row
            const unsigned xfirst = rp * xld + (unsigned)(civ ? ci : 0) * 4u, xlast = (rp + (unsigned)(W - 1)) * xld + (unsigned)(civ ? ci : 0) * 4u;
            r.vm[dy] = 0;
#pragma unroll
            for (int j = 0; j < 10; ++j) {
                const int px = p0 + j - 1;
                const bool lo_ok = px >= 0, hi_ok = px < W;
                const unsigned off = !lo_ok ? xfirst : (!hi_ok ? xlast : x0 + (unsigned)(j - 1) * xld);
                r.v[dy][j] = *(const float*)(xbase + off);
                r.vm[dy] |= (rok && civ && lo_ok && hi_ok) ? (1u << j) : 0u;
            }
        }
    };
    auto mma = [&](const Regs& rr_) __attribute__((always_inline)) {
        Regs r = rr_;
#pragma unroll
        for (int j = 0; j < 8; ++j) if (!((r.gm >> j) & 1u)) r.g[j] = 0.f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int j = 0; j < 10; ++j) if (!((r.vm[dy] >> j) & 1u)) r.v[dy][j] = 0.f;
        uint4 gh, gl;
        split8(r.g, gh, gl);
        const bf16x8 ah = __builtin_bit_cast(bf16x8, gh), al = __builtin_bit_cast(bf16x8, gl);
#pragma unroll
        for (int j = 0; j < 8; ++j) bsum += r.g[j];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            // the row's ten values are split ONCE: packed hi / lo of the five even-aligned pairs (0,1) .. (8,9) and the four odd-aligned pairs
            // (1,2) .. (7,8); tap dx = 0 / 2 takes even pairs 0..3 / 1..4, dx = 1 the odd ones.  Same conversions as split8 of the three
            // shifted windows (hi = RNE(v), lo = RNE(v - hi)): identical fragments, 38 instead of 72 conversions.
            const float* v = r.v[dy];
            unsigned eh[5], el[5], oh[4], ol[4];
            float res[10];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                float2_t pr = {v[2 * k], v[2 * k + 1]};
                eh[k] = __builtin_bit_cast(unsigned, __builtin_convertvector(pr, bf16x2_t));
                res[2 * k] = v[2 * k] - __uint_as_float(eh[k] << 16);
                res[2 * k + 1] = v[2 * k + 1] - __uint_as_float(eh[k] & 0xffff0000u);
                float2_t rr2 = {res[2 * k], res[2 * k + 1]};
                el[k] = __builtin_bit_cast(unsigned, __builtin_convertvector(rr2, bf16x2_t));
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // hi halves of values 2k+1, 2k+2 are already in eh[k] (upper half) and eh[k+1] (lower half)
                oh[k] = (eh[k] >> 16) | (eh[k + 1] << 16);
                float2_t rr2 = {res[2 * k + 1], res[2 * k + 2]};
                ol[k] = __builtin_bit_cast(unsigned, __builtin_convertvector(rr2, bf16x2_t));
            }
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const uint4 xh = dx == 1 ? make_uint4(oh[0], oh[1], oh[2], oh[3]) : (dx == 0 ? make_uint4(eh[0], eh[1], eh[2], eh[3]) : make_uint4(eh[1], eh[2], eh[3], eh[4]));
                const uint4 xl = dx == 1 ? make_uint4(ol[0], ol[1], ol[2], ol[3]) : (dx == 0 ? make_uint4(el[0], el[1], el[2], el[3]) : make_uint4(el[1], el[2], el[3], el[4]));
                const bf16x8 bh = __builtin_bit_cast(bf16x8, xh), bl = __builtin_bit_cast(bf16x8, xl);
                const int t = dy * 3 + dx;
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[t], 0, 0, 0);
            }
        }
    };
    Regs r0, r1;
    const int stride = single ? (int)gridDim.x * 4 : (int)gridDim.x * wpp;
    int item = single ? (int)blockIdx.x * 4 + wave : (int)blockIdx.x * wpp + sub;
    if (item < nitems) fetch(item, r0);
    while (item < nitems) {
        const int n1 = item + stride;
        if (n1 < nitems) fetch(n1, r1);
        mma(r0);
        if (n1 >= nitems) break;
        const int n2 = n1 + stride;
        if (n2 < nitems) fetch(n2, r0);
        mma(r1);
        item = n2;
    }
    bsum += __shfl_xor(bsum, 32);
    if constexpr (BLKRED) {
        __shared__ float red[2][9 * 1024 + 32];
        auto put = [&](float* dst) __attribute__((always_inline)) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int r = 0; r < 16; ++r) dst[(tap * 32 + acc_row(r, hg)) * 32 + c] = acc[tap][r];
            if (hg == 0) dst[9 * 1024 + c] = bsum;
        };
        auto add = [&](const float* src) __attribute__((always_inline)) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[tap][r] += src[(tap * 32 + acc_row(r, hg)) * 32 + c];
            bsum += src[9 * 1024 + c];
        };
        if (wave >= 2) put(red[wave - 2]);
        __syncthreads();
        if (wave < 2) add(red[wave]);                                  // w0 += w2, w1 += w3
        __syncthreads();
        if (wave == 1) put(red[0]);
        __syncthreads();
        if (wave != 0) return;
        add(red[0]);
        put(part + (long)blockIdx.x * GWG_PART);
        return;
    }
    // pair index = cob * ncib + cib = wave; single: chunk index; WIDE: chunk blockIdx.x * wpp + sub, npairs partials per chunk
    float* out = part + (WIDE ? ((long)blockIdx.x * wpp + sub) * npairs + pair : (long)blockIdx.x * 4 + wave) * GWG_PART;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(tap * 32 + acc_row(r, hg)) * 32 + c] = acc[tap][r];
    if (hg == 0) out[9 * 1024 + c] = bsum;                            // bias partial of channel co (read from the pairs with cib == 0)
}

// Fixed-order second stage.  A block owns 64 consecutive elements; thread (e = tid & 63, g = tid >> 6) sums the chunks g, g + 16, ... of
// its element in fp64 -- the 64 lanes of a wave read 64 consecutive floats of one partial tile (ci is the fastest index of both the
// element order and the tile) -- eight loads in flight per thread; the sixteen group sums are combined in a fixed order through LDS.
// (Four groups with four loads in flight: 16 dependent rounds over 256 partials, 9 us; this form: two.)
#define GWR_G 16
// `ad` (ad.pw != null; MSG_CHN 1layer fused step without a gradient exchange): the thread that finishes an element's sum applies Adam to it at
// once -- the arithmetic of adam_multi_kernel (wgrad_adam.hip) on the value just stored in gw / gb, t = *step + 1 read by every block, the step
// count written by the last block to finish: the same parameters and moments bit for bit, one dependent launch less at the very end of the step.
__global__ __launch_bounds__(64 * GWR_G) void gwgrad_mfma_reduce_kernel(const float* __restrict__ part, int nchunks, int npairs, int ncib, int Ci, int Co,
                                                                       float* __restrict__ gw, float* __restrict__ gb, GwAdam ad) {
    __shared__ double red[GWR_G][64];
    const int el = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long e = (long)blockIdx.x * 64 + el;
    const long nw = 9L * Co * Ci;
    const bool live = e < nw + Co;
    int tap = 0, co = 0, ci = 0;
    if (live) {
        if (e < nw) { tap = (int)(e / ((long)Co * Ci)); const int r = (int)(e % ((long)Co * Ci)); co = r / Ci; ci = r % Ci; }
        else co = (int)(e - nw);
    }
    const int pair = (co >> 5) * ncib + (e < nw ? (ci >> 5) : 0);
    const long off = e < nw ? ((long)tap * 32 + (co & 31)) * 32 + (ci & 31) : 9 * 1024 + (co & 31);
    const float* p0 = part + (long)pair * GWG_PART + off;
    const long cs = (long)npairs * GWG_PART;                   // floats between consecutive chunks of one element
    double s = 0.0;
    if (live) {
        int k = g;
        for (; k + 7 * GWR_G < nchunks; k += 8 * GWR_G) {
            float a[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = p0[(long)(k + j * GWR_G) * cs];
#pragma unroll
            for (int j = 0; j < 8; ++j) s += (double)a[j];
        }
        for (; k < nchunks; k += GWR_G) s += (double)p0[(long)k * cs];
    }
    red[g][el] = s;
    __syncthreads();
    if (g == 0 && live) {
        s = 0.0;
#pragma unroll
        for (int j = 0; j < GWR_G; ++j) s += red[j][el];
        const float gv = (float)s;
        const bool isw = e < nw;
        if (isw) gw[((long)co * Ci + ci) * 9 + tap] = gv;
        else if (gb) gb[co] = gv;
        if (ad.pw && (isw || ad.pb)) {
            const float lr = ad.hyper[0], b1 = ad.hyper[1], b2 = ad.hyper[2], eps = ad.hyper[3], wd = ad.hyper[4];
            const int t = *ad.step + 1;
            const double bc1 = 1.0 - pow((double)b1, (double)t), bc2 = 1.0 - pow((double)b2, (double)t);
            const float step_size = (float)((double)lr / bc1);
            const float bc2s = (float)sqrt(bc2);
            const long k = isw ? ((long)co * Ci + ci) * 9 + tap : co;
            float* P = isw ? ad.pw : ad.pb; float* M = isw ? ad.mw : ad.mb; float* V = isw ? ad.vw : ad.vb;
            float pk = P[k], mk = M[k], vk = V[k];
            ptta_adam_update(pk, mk, vk, gv, wd, b1, b2, eps, step_size, bc2s);
            M[k] = mk; V[k] = vk; P[k] = pk;
        }
    }
    if (ad.pw) {
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned done = atomicAdd(ad.ticket, 1u);
            if (done == gridDim.x - 1) { *ad.step = *ad.step + 1; *ad.ticket = 0u; }
        }
    }
}

// the reducer's launch, for every form: one thread group per element of dW (9 Ci Co) and db (Co)
void launch_reduce(const GView& x, const GView& gy, const float* part, int nchunks, int npairs, int ncib, float* gw, float* gb, const GwAdam& adam,
                   hipStream_t s) {
    const long n = 9L * x.C * gy.C + gy.C;
    hipLaunchKernelGGL(gwgrad_mfma_reduce_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64 * GWR_G), 0, s, part, nchunks, npairs, ncib, x.C, gy.C, gw, gb, adam);
}

}  // namespace

int ptta_gwgrad_mfma_chunks(long pixels) { long n = (pixels + 127) / 128; return (int)(n > 1024 ? 1024 : (n < 1 ? 1 : n)); }
long ptta_gwgrad_mfma_part_floats(long pixels, int Ci, int Co) {
    const long np = (long)((Ci + 31) / 32) * ((Co + 31) / 32);
    const long a = (long)ptta_gwgrad_mfma_chunks(pixels) * np * GWG_PART;
    const long b = 256L * (np > 4 ? np : 4) * GWG_PART;                  // gwgrad_x3_kernel: 256 blocks x 4 tile pairs; WIDE: 256 chunks x npairs
    return a > b ? a : b;
}
int ptta_launch_gwgrad_mfma(const GView& x, const GView& gy, float* part, float* gw, float* gb, hipStream_t s, int gy_bf16, const GwAdam* adam) {
    const GwAdam noad{};
    const bool sq = x.C <= 64 && gy.C <= 64, wide_out = x.C <= 32 && gy.C <= 128, wide_in = x.C <= 128 && gy.C <= 32;
    // (the bf16x3 kernel addresses its maps with 32-bit byte offsets)
    const bool small_maps = (double)x.B * x.H * x.W * x.ld * 4.0 < 4294967296.0 && (double)gy.B * gy.H * gy.W * gy.ld * 4.0 < 4294967296.0;
    const int ncib = (x.C + 31) / 32, npairs = ncib * ((gy.C + 31) / 32);
    const bool narrow_form = (sq || wide_out || wide_in) && x.C > 16;
    // the Adam fused into the reduction exists for the single-pair form only: asked for anywhere else it is an error, not a silent no-update
    if (adam && adam->pw && !(narrow_form && small_maps && x.C <= 32 && gy.C <= 32)) return -22;
    // the bf16x3 forms' item: 16 consecutive pixels of one row
    const int nx = (x.W + 15) / 16;
    const long nitems = (long)x.B * x.H * nx;
    // the WIDE form takes exactly the shapes that had only the fp32-MFMA form: channel counts multiples of 16 up to 256, at least two tile
    // pairs (a single 16-channel pair -- CostDCNet's 1layer Conv2d(16, 16, 3) -- keeps the fp32-MFMA form)
    if (!narrow_form && !gy_bf16 && small_maps && npairs >= 2 && !(x.C & 15) && !(gy.C & 15) && x.C <= 256 && gy.C <= 256) {
        const int wpp = npairs < 4 ? 4 / npairs : 1, ngrp = npairs < 4 ? 1 : (npairs + 3) / 4;
        const long want = (nitems + wpp - 1) / wpp;
        const int nblk = (int)(want < 256 ? want : 256);
        hipLaunchKernelGGL((gwgrad_x3_kernel<false, false, true>), dim3(nblk, ngrp), dim3(256), 0, s, x, gy, nx, 0, ncib, part);
        launch_reduce(x, gy, part, nblk * wpp, npairs, ncib, gw, gb, noad, s);
        PTTA_CHECK_LAUNCH();
        return 0;
    }
    if (narrow_form && small_maps) {
        // bf16x3 form: blocks of four waves = four 32x32 channel-tile pairs (2 x 2, or 1 x 4 / 4 x 1 for the 32 <-> 128 layers of the
        // 2layers meta block), partials [block][4 pairs]; <= 32 x 32 channels: one pair, the waves split the items and the block sums
        // their partials in LDS, partials [block]
        const int single = (x.C <= 32 && gy.C <= 32) ? 1 : 0;
        const int kcib = sq ? 2 : (wide_out ? 1 : 4);
        const long cap = 256;       // (single: measured 64 / 128 / 256 / 336 / 418 blocks on the MSG_CHN step: 1.213 / 1.207 / 1.201 / 1.208 / 1.209 ms)
        const long want = single ? (nitems + 3) / 4 : nitems;
        const int nblk = (int)(want < cap ? want : cap);
        if (single) {
            if (gy_bf16) hipLaunchKernelGGL((gwgrad_x3_kernel<true, true>), dim3(nblk), dim3(256), 0, s, x, gy, nx, single, kcib, part);
            else hipLaunchKernelGGL((gwgrad_x3_kernel<false, true>), dim3(nblk), dim3(256), 0, s, x, gy, nx, single, kcib, part);
            launch_reduce(x, gy, part, nblk, 1, 1, gw, gb, adam ? *adam : noad, s);
        } else {
            if (gy_bf16) hipLaunchKernelGGL(gwgrad_x3_kernel<true>, dim3(nblk), dim3(256), 0, s, x, gy, nx, single, kcib, part);
            else hipLaunchKernelGGL(gwgrad_x3_kernel<false>, dim3(nblk), dim3(256), 0, s, x, gy, nx, single, kcib, part);
            launch_reduce(x, gy, part, nblk, 4, kcib, gw, gb, noad, s);
        }
        PTTA_CHECK_LAUNCH();
        return 0;
    }
    if (gy_bf16) return -22;          // (the fp32-MFMA form takes fp32 gradients)
    return ptta_launch_gwgrad_f32mfma(x, gy, part, gw, gb, s);
}
int ptta_launch_gwgrad_f32mfma(const GView& x, const GView& gy, float* part, float* gw, float* gb, hipStream_t s) {
    const int nchunks = ptta_gwgrad_mfma_chunks((long)x.B * x.H * x.W);
    const int ncib = (x.C + 31) / 32, ncob = (gy.C + 31) / 32, npairs = ncib * ncob;
    hipLaunchKernelGGL(gwgrad_mfma_kernel, dim3(nchunks, npairs), dim3(64), 0, s, x, gy, nchunks, ncib, part);
    launch_reduce(x, gy, part, nchunks, npairs, ncib, gw, gb, GwAdam{}, s);
    PTTA_CHECK_LAUNCH();
    return 0;
}
