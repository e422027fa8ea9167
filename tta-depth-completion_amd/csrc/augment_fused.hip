// The augmented inner loop's frame set through one draw in ONE launch (include/ptta.h ptta_augment_frames; src/tta_main.py:595-604): the
// staged chain of augment.hip -- crop_flip_kernel -> rotate_kernel -> resize_crop_kernel per tensor, then photo_pass1_kernel on the image --
// composed backwards from the output pixel.  One thread per output pixel computes that pixel of every output: the geometry of the image
// (loss_image) and of the one-channel maps, and image1 = loss_image truncated to 0..255 and brightness-adjusted, with the grey sums the
// second photometric pass (photo_pass2_full_kernel, unchanged, reached through ptta_launch_photo_pass2_full) takes its contrast mean from.
//
// Equality with the staged path is bit for bit, so the arithmetic below is the staged kernels' as hipcc COMPILED them: contraction is
// off for this whole file and every multiply-add the staged kernels' ISA fuses is spelled __builtin_fmaf, every one it keeps apart is a
// plain operator.  What the ISA of augment.hip shows (hipcc --save-temps, gfx950), restated where it is used:
//   rotate_kernel        gx = fma(yc, t10, xc * t00);  ix = 0.5 * fma(gx + 1, W, -1);  v = fma(w_nw, s_nw, 0), then fma(w_k, s_k, v) per tap
//   resize_crop_kernel   fy = fma(scy, Y + 0.5, -0.5).  Its channel loop is vectorised by two, so a 3-channel image takes TWO forms:
//                        channels 0, 1   row0 = fma(lx0, a, lx1 * b);  row1 = fma(lx0, c, lx1 * d);  v = fma(ly0, row0, ly1 * row1)
//                        channel 2       row0 = fma(lx1, b, lx0 * a);  row1 = fma(lx0, c, lx1 * d);  v = ly0 * row0 + ly1 * row1
//   photo_pass1_kernel   grey = floor(fma(0.114, b, fma(0.2989, r, 0.587 * g)));  brightness is one multiply
// tests/test_gpu_augment_fused.py holds every output to the staged calls with torch.equal (a flat image of 200.0 interpolates to 200 or
// to 200 minus one ulp depending on exactly these choices, and image1 is its floor).
//
// Grid: ceil(crop_height * crop_width / 256) x n blocks of 256 threads, whatever the frame's size (photo_pass1_kernel's 256 blocks per
// sample would leave a gather kernel with up to 48 loads per pixel at one block per CU for n = 1).  The second pass reads 256 partial sums
// per sample, so the blocks' sums are combined inside the launch: thread 0 of a block stores its sum and adds one to the sample's arrival
// counter, the block whose add came last adds the stored sums into the 256 slots (slot k: blocks k, k + 256, ...; unused slots zero) and
// resets the counter.  Every shared word is an 8- or 4-byte agent-scope atomic on both sides, the store is waited for before the add, and the
// last block's loads come behind an agent-scope acquire and a workgroup barrier; no block waits for another.  The sums are of integers
// below 2^53: exact in fp64 in any order, so the result does not depend on which block came last.
#include "ptta_common.h"
#include "ptta_kernels.h"
#include "../../include/ptta.h"
#pragma clang fp contract(off)

#define AUG_THREADS 256
#define AUG_SLOTS 256            // the partial sums photo_pass2_full_kernel reads per sample (augment.hip PH_BLOCKS)

static_assert(sizeof(ptta_augment_draw) == 52, "ptta_augment_draw is packed: proxytta/augment.py mirrors it field by field");

struct AugGeo {                  // one sample's draw, as the staged kernels derive their constants from it
    int W, h, w;                 // frame width; the cropped window every stage behind the crop works on
    int y0, x0;                  // crop start, clamped into the frame
    bool hf, vf, rot, rs;
    float t00, t10, t01, t11, xc0, yc0, fw, fh;
    int sy, sx;
    float scy, scx, div;
};
struct AugK {                    // the launch's arguments
    const float *image, *map[3];
    float *loss_image, *map_out[3], *image1;
    const ptta_augment_draw* draws;
    int n, H, W, h, w, bilinear, scale_depth, nb;
    double* part; unsigned long long* blockpart; float* tabf; unsigned char* tabu; unsigned* ticket;
};

// source pixel (index into one H x W plane) of pixel (y, x) of the cropped and flipped window: crop_flip_kernel's arithmetic.  The
// coordinates are clamped into the window first -- a no-op for every coordinate a valid draw produces -- so that no record can make a
// thread form an address outside its sample
__device__ __forceinline__ int aug_src(const AugGeo& g, int y, int x) {
    y = min(max(y, 0), g.h - 1); x = min(max(x, 0), g.w - 1);
    return (g.y0 + (g.vf ? g.h - 1 - y : y)) * g.W + g.x0 + (g.hf ? g.w - 1 - x : x);
}
// float -> int for a coordinate that is in range for every valid draw: the clamp (NaN -> lo) keeps a wild record's conversion defined
__device__ __forceinline__ int aug_int(float v, float lo) { return (int)fminf(fmaxf(v, lo), 1.0e9f); }
// rotate_kernel's sampling position of output pixel (y, x)
__device__ __forceinline__ void aug_rot_pos(const AugGeo& g, int y, int x, float& ix, float& iy) {
    const float xc = g.xc0 + (float)x, yc = g.yc0 + (float)y;
    const float gx = __builtin_fmaf(yc, g.t10, xc * g.t00), gy = __builtin_fmaf(yc, g.t11, xc * g.t01);
    ix = 0.5f * __builtin_fmaf(gx + 1.f, g.fw, -1.f);
    iy = 0.5f * __builtin_fmaf(gy + 1.f, g.fh, -1.f);
}
// nearest mode: the source pixel of pixel (y, x) of the rotated window, -1 where rotate_kernel writes a zero
__device__ __forceinline__ int aug_rot_nearest(const AugGeo& g, int y, int x) {
    if (!g.rot) return aug_src(g, y, x);
    float ix, iy;
    aug_rot_pos(g, y, x, ix, iy);
    const float rx = nearbyintf(ix), ry = nearbyintf(iy);
    const bool ok = rx >= 0.f && rx <= (float)(g.w - 1) && ry >= 0.f && ry <= (float)(g.h - 1);
    return ok ? aug_src(g, (int)ry, (int)rx) : -1;
}
// bilinear mode: pixel (y, x) of the rotated window, three channels (grid_sample's nw, ne, sw, se accumulation)
__device__ __forceinline__ void aug_rot_bilinear(const AugGeo& g, const float* __restrict__ s, long plane, int y, int x, float v[3]) {
    if (!g.rot) {
        const int si = aug_src(g, y, x);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch] = s[ch * plane + si];
        return;
    }
    float ix, iy;
    aug_rot_pos(g, y, x, ix, iy);
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = aug_int(fx, -4.f), y0 = aug_int(fy, -4.f), x1 = x0 + 1, y1 = y0 + 1;
    const float wx1 = ix - fx, wx0 = 1.f - wx1, wy1 = iy - fy, wy0 = 1.f - wy1;
    const bool okx0 = x0 >= 0 && x0 < g.w, okx1 = x1 >= 0 && x1 < g.w, oky0 = y0 >= 0 && y0 < g.h, oky1 = y1 >= 0 && y1 < g.h;
    const float wnw = wx0 * wy0, wne = wx1 * wy0, wsw = wx0 * wy1, wse = wx1 * wy1;
    const int inw = aug_src(g, y0, x0), ine = aug_src(g, y0, x1), isw = aug_src(g, y1, x0), ise = aug_src(g, y1, x1);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float* p = s + ch * plane;
        float a = 0.f;
        if (oky0 && okx0) a = __builtin_fmaf(wnw, p[inw], a);
        if (oky0 && okx1) a = __builtin_fmaf(wne, p[ine], a);
        if (oky1 && okx0) a = __builtin_fmaf(wsw, p[isw], a);
        if (oky1 && okx1) a = __builtin_fmaf(wse, p[ise], a);
        v[ch] = a;
    }
}
__device__ __forceinline__ float aug_u8trunc(float v) { v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v); return floorf(v); }

__global__ __launch_bounds__(AUG_THREADS) void augment_frames_kernel(const AugK k) {
    __shared__ double red[5];    // four wave sums, then "this block's add came last"
    const int b = blockIdx.y, tid = threadIdx.x;
    const ptta_augment_draw d = k.draws[b];
    AugGeo g;
    g.W = k.W; g.h = k.h; g.w = k.w;
    g.y0 = min(max(d.crop_y, 0), k.H - k.h); g.x0 = min(max(d.crop_x, 0), k.W - k.w);
    g.hf = d.flags & PTTA_AUG_HFLIP; g.vf = d.flags & PTTA_AUG_VFLIP; g.rot = d.flags & PTTA_AUG_ROTATE; g.rs = d.flags & PTTA_AUG_RESIZE;
    g.fw = (float)k.w; g.fh = (float)k.h;
    g.xc0 = -0.5f * g.fw + 0.5f; g.yc0 = -0.5f * g.fh + 0.5f;
    g.t00 = g.t10 = g.t01 = g.t11 = 0.f;
    if (g.rot) {                 // rotate_kernel: math.radians / cos / sin in double, then the float32 theta over half the window's size
        const double a = (double)d.angle_deg * 3.14159265358979323846 / 180.0;
        const float m0 = (float)cos(a), m1 = (float)(-sin(a)), m3 = (float)sin(a), m4 = (float)cos(a);
        g.t00 = m0 / (0.5f * g.fw); g.t10 = m1 / (0.5f * g.fw); g.t01 = m3 / (0.5f * g.fh); g.t11 = m4 / (0.5f * g.fh);
    }
    g.sy = d.resize_y; g.sx = d.resize_x;
    g.scy = g.fh / (float)d.resize_height; g.scx = g.fw / (float)d.resize_width;
    g.div = (float)d.resize_width / g.fw;
    const bool divide = g.rs && k.scale_depth;

    const long plane = (long)k.H * k.W;
    const int hw = k.h * k.w;
    const int i = blockIdx.x * AUG_THREADS + tid;
    const bool active = i < hw;
    double grey = 0.0;
    if (active) {
        const int oy = i / k.w, ox = i - oy * k.w;
        const long o1 = (long)b * hw + i, o3 = (long)b * 3 * hw + i;
        const float* img = k.image + (long)b * 3 * plane;
        // ---- nearest chain: the pixel of the resized window is one pixel of the rotated window is one source pixel or a zero ----
        int Y = oy, X = ox;
        if (g.rs) {              // resize_crop_kernel: min(floor(dst * in / out), in - 1)
            Y = min(aug_int(floorf((float)(oy + g.sy) * g.scy), 0.f), k.h - 1);
            X = min(aug_int(floorf((float)(ox + g.sx) * g.scx), 0.f), k.w - 1);
        }
        const int si = aug_rot_nearest(g, Y, X);
#pragma unroll
        for (int m = 0; m < 3; ++m)
            if (k.map[m]) {
                const float v = si >= 0 ? k.map[m][(long)b * plane + si] : 0.f;
                k.map_out[m][o1] = divide ? v / g.div : v;
            }
        // ---- the image ----
        float v[3];
        if (!k.bilinear) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[ch] = si >= 0 ? img[ch * plane + si] : 0.f;
        } else if (!g.rs) {
            aug_rot_bilinear(g, img, plane, oy, ox, v);
        } else {                 // resize_crop_kernel's 4 taps, each a pixel of the rotated window
            float fy = __builtin_fmaf(g.scy, (float)(oy + g.sy) + 0.5f, -0.5f), fx = __builtin_fmaf(g.scx, (float)(ox + g.sx) + 0.5f, -0.5f);
            fy = fy < 0.f ? 0.f : fy; fx = fx < 0.f ? 0.f : fx;
            const int y0 = aug_int(fy, 0.f), x0 = aug_int(fx, 0.f);
            const int y1 = y0 + (y0 < k.h - 1 ? 1 : 0), x1 = x0 + (x0 < k.w - 1 ? 1 : 0);
            const float ly1 = fy - (float)y0, ly0 = 1.f - ly1, lx1 = fx - (float)x0, lx0 = 1.f - lx1;
            float a[3], bb[3], c[3], dd[3];
            aug_rot_bilinear(g, img, plane, y0, x0, a);
            aug_rot_bilinear(g, img, plane, y0, x1, bb);
            aug_rot_bilinear(g, img, plane, y1, x0, c);
            aug_rot_bilinear(g, img, plane, y1, x1, dd);
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {         // the vectorised pair of resize_crop_kernel's channel loop
                const float row0 = __builtin_fmaf(lx0, a[ch], lx1 * bb[ch]), row1 = __builtin_fmaf(lx0, c[ch], lx1 * dd[ch]);
                v[ch] = __builtin_fmaf(ly0, row0, ly1 * row1);
            }
            {                                        // its scalar remainder
                const float row0 = __builtin_fmaf(lx1, bb[2], lx0 * a[2]), row1 = __builtin_fmaf(lx0, c[2], lx1 * dd[2]);
                v[2] = ly0 * row0 + ly1 * row1;
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) k.loss_image[o3 + (long)ch * hw] = v[ch];
        // ---- photo_pass1_kernel: .to(torch.uint8), then _blend(img, zeros, f) ----
        if (k.image1) {
            const bool on = d.flags & PTTA_AUG_BRIGHTNESS;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float x = aug_u8trunc(v[ch]);
                if (on) x = aug_u8trunc(d.brightness * x);
                v[ch] = x; k.image1[o3 + (long)ch * hw] = x;
            }
            grey = (double)floorf(__builtin_fmaf(0.114f, v[2], __builtin_fmaf(0.2989f, v[0], 0.587f * v[1])));
        }
    }
    if (!k.image1) return;       // (uniform: a kernel argument)
    // ---- the grey sums of the sample, in the 256 slots the second pass reads ----
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) grey += __shfl_xor(grey, m);
    if ((tid & 63) == 0) red[tid >> 6] = grey;
    __syncthreads();
    if (tid == 0) {
        const double sum = (red[0] + red[1]) + (red[2] + red[3]);
        __hip_atomic_store(k.blockpart + (long)b * k.nb + blockIdx.x, (unsigned long long)__double_as_longlong(sum), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                     // the sum has left before the counter says so
        const unsigned arrived = __hip_atomic_fetch_add(k.ticket + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = arrived == (unsigned)k.nb - 1u;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        red[4] = last ? 1.0 : 0.0;
        if (blockIdx.x == 0) {   // the second launch's per-sample tables (the kernel takes one array per option)
            const unsigned bits[4] = {PTTA_AUG_CONTRAST, PTTA_AUG_GAMMA, PTTA_AUG_HUE, PTTA_AUG_SATURATION};
            const float f[4] = {d.contrast, d.gamma, d.hue, d.saturation};
#pragma unroll
            for (int q = 0; q < 4; ++q) { k.tabu[q * k.n + b] = (d.flags & bits[q]) ? 1 : 0; k.tabf[q * k.n + b] = f[q]; }
        }
    }
    __syncthreads();
    if (red[4] != 0.0) {
        double s = 0.0;
        for (int j = tid; j < k.nb; j += AUG_SLOTS)
            s += __longlong_as_double((long long)__hip_atomic_load(k.blockpart + (long)b * k.nb + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        k.part[(long)b * AUG_SLOTS + tid] = s;
        if (tid == 0) __hip_atomic_store(k.ticket + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
static_assert(AUG_THREADS == AUG_SLOTS, "the last block fills one slot per thread");

// scratch layout: [part 256 n doubles][block sums nb n x 8 bytes][factor tables 4 n floats][flag tables 4 n bytes, padded to 8][counters n x 4 bytes]
static long aug_blocks(int h, int w) { return ((long)h * w + AUG_THREADS - 1) / AUG_THREADS; }
static long aug_pad8(long v) { return (v + 7) / 8 * 8; }
extern "C" int64_t ptta_augment_scratch_bytes(int n, int crop_height, int crop_width) {
    if (n < 1 || n > 65535 || crop_height < 1 || crop_width < 1 || (long)crop_height * crop_width >= (1L << 31)) return -22;
    return (int64_t)(8L * AUG_SLOTS * n + 8L * aug_blocks(crop_height, crop_width) * n + aug_pad8(16L * n) + aug_pad8(4L * n) + aug_pad8(4L * n));
}

extern "C" int ptta_augment_frames(const ptta_augment_args* a, ptta_stream stream) {
    if (!a) return ptta_refuse_args("ptta_augment_frames: NULL args");
    if (!a->image || !a->loss_image || !a->draws) return ptta_refuse_args("ptta_augment_frames: image, loss_image and draws are required");
    if (a->n < 1 || a->n > 65535) return ptta_refuse_args("ptta_augment_frames: n outside 1..65535");
    if (a->height < 1 || a->width < 1 || a->crop_height < 1 || a->crop_width < 1) return ptta_refuse_args("ptta_augment_frames: a size below 1");
    if (a->crop_height > a->height || a->crop_width > a->width) return ptta_refuse_args("ptta_augment_frames: the crop is larger than the frame");
    if (3L * a->height * a->width >= (1L << 31)) return ptta_refuse_args("ptta_augment_frames: a frame of 2^31 values or more");
    const float* in[3] = {a->sparse_depth, a->validity_map, a->ground_truth};
    float* out[3] = {a->sparse_depth_out, a->validity_map_out, a->ground_truth_out};
    for (int m = 0; m < 3; ++m)
        if ((in[m] == nullptr) != (out[m] == nullptr)) return ptta_refuse_args("ptta_augment_frames: a map and its output are given together or not at all");
    const long plane = (long)a->height * a->width, hw = (long)a->crop_height * a->crop_width;
    const int64_t need = ptta_augment_scratch_bytes(a->n, a->crop_height, a->crop_width);
    if (a->image1 && (!a->scratch || a->scratch_bytes < need || ((uintptr_t)a->scratch & 7) != 0))
        return ptta_refuse_args("ptta_augment_frames: image1 needs ptta_augment_scratch_bytes(n, crop_height, crop_width) bytes of 8-byte aligned scratch");
    // no two buffers may overlap (inputs are read while every output is written)
    struct Span { const char* p; long bytes; } spans[12];
    int ns = 0;
    auto add = [&](const void* p, long bytes) { if (p) spans[ns++] = Span{(const char*)p, bytes}; };
    add(a->image, 12L * a->n * plane); add(a->loss_image, 12L * a->n * hw); add(a->image1, 12L * a->n * hw);
    for (int m = 0; m < 3; ++m) { add(in[m], 4L * a->n * plane); add(out[m], 4L * a->n * hw); }
    add(a->draws, (long)sizeof(ptta_augment_draw) * a->n);
    if (a->image1) add(a->scratch, (long)need);
    for (int p = 0; p < ns; ++p)
        for (int q = p + 1; q < ns; ++q)
            if (spans[p].p < spans[q].p + spans[q].bytes && spans[q].p < spans[p].p + spans[p].bytes)
                return ptta_refuse_args("ptta_augment_frames: two buffers overlap");

    AugK k;
    k.image = a->image; k.loss_image = a->loss_image; k.image1 = a->image1; k.draws = a->draws;
    for (int m = 0; m < 3; ++m) { k.map[m] = in[m]; k.map_out[m] = out[m]; }
    k.n = a->n; k.H = a->height; k.W = a->width; k.h = a->crop_height; k.w = a->crop_width;
    k.bilinear = a->image_bilinear ? 1 : 0; k.scale_depth = a->scale_depth ? 1 : 0; k.nb = (int)aug_blocks(a->crop_height, a->crop_width);
    k.part = nullptr; k.blockpart = nullptr; k.tabf = nullptr; k.tabu = nullptr; k.ticket = nullptr;
    if (a->image1) {
        char* s = (char*)a->scratch;
        k.part = (double*)s; s += 8L * AUG_SLOTS * a->n;
        k.blockpart = (unsigned long long*)s; s += 8L * k.nb * a->n;
        k.tabf = (float*)s; s += aug_pad8(16L * a->n);
        k.tabu = (unsigned char*)s; s += aug_pad8(4L * a->n);
        k.ticket = (unsigned*)s;
    }
    hipLaunchKernelGGL(augment_frames_kernel, dim3((unsigned)k.nb, a->n), dim3(AUG_THREADS), 0, (hipStream_t)stream, k);
    if (hipGetLastError() != hipSuccess) return -5;
    if (a->image1 && a->pass2) {
        const unsigned char* u = k.tabu; const float* f = k.tabf; const int n = a->n;
        return ptta_launch_photo_pass2_full(a->image1, n, a->crop_height, a->crop_width, k.part, u, f, u + n, f + n, u + 2 * n, f + 2 * n, u + 3 * n, f + 3 * n,
                                            (hipStream_t)stream);
    }
    return 0;
}
