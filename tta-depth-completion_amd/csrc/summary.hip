// The summary panels of log_summary composed on device (src/external_model_adapt.py:662-909, src/log_utils.py:53-80; include/ptta.h
// ptta_summary_compose).  The reference copies up to five fp32 maps to the host, colours each through matplotlib in a Python loop, and
// runs torch.cat, make_grid and the writer's float -> uint8 pass there.  All of it is element-wise arithmetic and a 256-entry table lookup
// on maps that are resident in HBM: one launch here writes the finished grid and one copy of it leaves the card.
//   work   the grid is cut into SPANS: (grid row gy, panel i, half): the `width` columns of the left or the right half of panel i in
//          row gy, plus the make_grid padding next to them (the 2 columns in front of a panel go with its left half, the 2 behind
//          the last panel with its right half; the 4 padding rows are spans of zeros).  Spans tile the grid: every element is
//          written exactly once and nothing is cleared first.  blockIdx.x = half and block along the span, y = grid rows (strided), z = panel.
//   lanes  a lane owns 4 consecutive pixels of a span and computes their three channels from ONE read of each input, so a depth pixel
//          costs one table index and the error maps are read once, not once per channel.
//   stores a panel starts 2 floats into the row when n_show > 1 and the row pitch GW is only even, so a span's first element sits at
//          any offset m of a 16-byte line.  The lanes' groups are laid on the DESTINATION's 16-byte grid: lane k takes pixels
//          4 k - m ... 4 k - m + 3, the first and the last lane of a span store their 1-3 pixels one by one, every other lane one
//          16-byte store per channel plane.  That needs one m for the three planes: GH GW % 4 == 0 and a 16-byte-aligned base;
//          anything else takes the one-pixel-per-lane path.  The uint8 HWC form packs a lane's 4 pixels into 12 bytes at a 4-byte
//          boundary under the same grouping.  The sources are then read at the span's own (mis)alignment, 4 bytes per load, contiguous
//          across the wave: the kernel is bound by its 24 bytes written per pixel and row, not by the 4-12 read.
//   tables the two 256 x 3 fp64 tables are arguments; a block converts them once to fp32 (the rounding the reference's
//          .astype(np.float32) does) into 8 KB of LDS, one 16-byte entry per index, and keeps them for all its rows.
// Arithmetic: each value is a table entry or a chain of single fp32 operations; contraction is off for this file and csrc/Makefile leaves
// hipcc's correctly rounded division on, so `/` is the IEEE quotient and results equal the CPU reference's bit for bit.
#include <stdint.h>

#include <cmath>

#include "ptta_common.h"
#include "../../include/ptta.h"

#pragma clang fp contract(off)

namespace {

enum { SEG_ZERO = 0, SEG_IMAGE = 1, SEG_VIRIDIS = 2, SEG_ERR_SPARSE = 3, SEG_ERR_GT = 4 };
enum { ROW_IMAGE = 0, ROW_OUTPUT = 1, ROW_SPARSE = 2, ROW_GT = 3 };
constexpr int MAX_ROWS = PTTA_SUMMARY_MAX_IMAGES + 3;
constexpr int FLAG_BLOCKS = PTTA_SUMMARY_FLAG_WORDS - 1;
constexpr int BLOCK_BUDGET = 2048;            // blocks of one compose launch: 8 per CU, each converts the tables once

struct SummaryArgs {
    const float* image[PTTA_SUMMARY_MAX_IMAGES];
    const int* div255[PTTA_SUMMARY_MAX_IMAGES];
    const float* output;
    const float* sparse;
    const float* validity;
    const float* gt;
    const double* viridis;
    const double* inferno;
    void* out;
    int ns, H, W, R, GH, GW, pad, xb, normalize;
    float maxd;
    float rm[3], rs[3];
    unsigned char kind[MAX_ROWS];
};

struct Rgb { float r, g, b; };

// log_utils.colorize -> matplotlib's Colormap.__call__ on a float32 array
__device__ __forceinline__ Rgb colorize(const float4* lut, float x) {
    const float t = x * 256.0f;
    const int idx = (t >= 0.0f && t < 256.0f) ? (int)t : (t >= 256.0f ? 255 : 0);          // (NaN takes index 0 here and is zeroed below)
    const float4 e = lut[idx];
    const bool bad = t != t;
    return Rgb{bad ? 0.0f : e.x, bad ? 0.0f : e.y, bad ? 0.0f : e.z};
}

// the three channels of source pixel (b, y, x) of one span
template <int SEG>
__device__ __forceinline__ Rgb pixel(const SummaryArgs& a, const float4* viridis, const float4* inferno, const float* src, bool div, size_t px, size_t plane) {
    if (SEG == SEG_IMAGE) {
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            v[c] = src[px + c * plane];
            if (div) v[c] = v[c] / 255.0f;
            if (a.normalize) v[c] = (v[c] - a.rm[c]) / a.rs[c];
        }
        return Rgb{v[0], v[1], v[2]};
    }
    if (SEG == SEG_VIRIDIS) return colorize(viridis, src[px] / a.maxd);
    if (SEG == SEG_ERR_SPARSE) {
        const float o = a.output[px], s = a.sparse[px], v = a.validity[px];
        const float e = v > 0.0f ? fabsf(o - s) / (s + 1e-8f) : v;
        return colorize(inferno, e / 0.05f);
    }
    if (SEG == SEG_ERR_GT) {
        const float o = a.output[px], g = a.gt[px];
        const float e = g > 0.0f ? (fabsf(o - g) + 1e-8f) / (g + 1e-8f) : 0.0f;
        return colorize(inferno, e / 0.05f);
    }
    return Rgb{0.0f, 0.0f, 0.0f};
}

// torch.utils.tensorboard's float image -> uint8: (v * 255).clip(0, 255) truncated; NaN -> 0
__device__ __forceinline__ unsigned to_u8(float v) {
    const float s = v * 255.0f;
    return s > 0.0f ? (s < 255.0f ? (unsigned)s : 255u) : 0u;
}

template <bool U8>
__device__ __forceinline__ void store_px(const SummaryArgs& a, size_t at, size_t gplane, const Rgb& v) {          // at = gy GW + column
    if (U8) {
        unsigned char* o = (unsigned char*)a.out + 3 * at;
        o[0] = (unsigned char)to_u8(v.r); o[1] = (unsigned char)to_u8(v.g); o[2] = (unsigned char)to_u8(v.b);
    } else {
        float* o = (float*)a.out + at;
        o[0] = v.r; o[gplane] = v.g; o[2 * gplane] = v.b;
    }
}

struct alignas(4) Bytes12 { unsigned a, b, c; };

// one span of `W` source pixels whose first lands at grid element `at0` (= gy GW + column)
template <bool VEC, bool U8, int SEG>
__device__ __forceinline__ void span(const SummaryArgs& a, const float4* viridis, const float4* inferno, const float* src, bool div, size_t row_px,
                                     size_t plane, size_t at0, size_t gplane, int bx) {
    const int W = a.W;
    if (VEC) {
        const int m = (int)(at0 & 3u);                  // the span's offset inside a 16-byte line (4 pixels of 12 bytes in the uint8 form)
        for (int k = bx * blockDim.x + threadIdx.x; 4 * (long)k - m < W; k += a.xb * blockDim.x) {
            const int x0 = 4 * k - m;
            Rgb v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {               // a partial lane reads a pixel of its own span again; it is not stored
                const int x = min(max(x0 + j, 0), W - 1);
                v[j] = pixel<SEG>(a, viridis, inferno, src, div, row_px + x, plane);
            }
            if (x0 >= 0 && x0 + 3 < W) {
                if (U8) {
                    unsigned q[12];
#pragma unroll
                    for (int j = 0; j < 4; ++j) { q[3 * j] = to_u8(v[j].r); q[3 * j + 1] = to_u8(v[j].g); q[3 * j + 2] = to_u8(v[j].b); }
                    Bytes12 w;
                    w.a = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
                    w.b = q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24);
                    w.c = q[8] | (q[9] << 8) | (q[10] << 16) | (q[11] << 24);
                    *(Bytes12*)((unsigned char*)a.out + 3 * (at0 + x0)) = w;
                } else {
                    float* o = (float*)a.out + at0 + x0;
                    *(float4*)o = make_float4(v[0].r, v[1].r, v[2].r, v[3].r);
                    *(float4*)(o + gplane) = make_float4(v[0].g, v[1].g, v[2].g, v[3].g);
                    *(float4*)(o + 2 * gplane) = make_float4(v[0].b, v[1].b, v[2].b, v[3].b);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x0 + j >= 0 && x0 + j < W) store_px<U8>(a, at0 + x0 + j, gplane, v[j]);
            }
        }
    } else {
        for (int x = bx * blockDim.x + threadIdx.x; x < W; x += a.xb * blockDim.x)
            store_px<U8>(a, at0 + x, gplane, pixel<SEG>(a, viridis, inferno, src, div, row_px + x, plane));
    }
}

// grid: x = 2 xb blocks (left half, right half), y = grid rows (strided), z = panels (strided)
template <bool VEC, bool U8>
__global__ __launch_bounds__(512) void summary_compose_kernel(const SummaryArgs a) {
    __shared__ float4 lut[2][256];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) {
        if (a.viridis) lut[0][i] = make_float4((float)a.viridis[3 * i], (float)a.viridis[3 * i + 1], (float)a.viridis[3 * i + 2], 0.0f);
        if (a.inferno) lut[1][i] = make_float4((float)a.inferno[3 * i], (float)a.inferno[3 * i + 1], (float)a.inferno[3 * i + 2], 0.0f);
    }
    __syncthreads();
    const int half = (int)blockIdx.x >= a.xb ? 1 : 0, bx = (int)blockIdx.x - half * a.xb;
    const int W = a.W, H = a.H, pad = a.pad;
    const size_t plane = (size_t)H * W, gplane = (size_t)a.GH * a.GW;
    const Rgb zero{0.0f, 0.0f, 0.0f};
    for (int i = blockIdx.z; i < a.ns; i += gridDim.z) {
        const int c0 = i * (2 * W + pad) + pad + half * W;                  // grid column of the span's first pixel
        for (int gy = blockIdx.y; gy < a.GH; gy += gridDim.y) {
            const size_t grow = (size_t)gy * a.GW;
            const int py = gy - pad;
            const bool last = half && i == a.ns - 1;
            if (py < 0 || py >= a.R * H) {                                  // a padding row: the span and the padding columns that go with it
                const int lo = half ? c0 : c0 - pad, hi = c0 + W + (last ? pad : 0);
                for (int c = lo + bx * blockDim.x + threadIdx.x; c < hi; c += a.xb * blockDim.x) store_px<U8>(a, grow + c, gplane, zero);
                continue;
            }
            if (bx == 0 && (int)threadIdx.x < pad) {
                if (!half) store_px<U8>(a, grow + c0 - pad + threadIdx.x, gplane, zero);
                if (last) store_px<U8>(a, grow + c0 + W + threadIdx.x, gplane, zero);
            }
            const int r = py / H, y = py - r * H, kind = a.kind[r];
            const size_t at0 = grow + c0;
            const size_t row1 = ((size_t)i * H + y) * W;                    // the row in an N x 1 x H x W map
#define SPAN(SEG, SRC, DIV, ROW, PLANE) span<VEC, U8, SEG>(a, lut[0], lut[1], SRC, DIV, ROW, PLANE, at0, gplane, bx)
            if (kind == ROW_IMAGE) {
                if (half) SPAN(SEG_ZERO, nullptr, false, 0, 0);
                else SPAN(SEG_IMAGE, a.image[r], a.div255[r] != nullptr && *a.div255[r] != 0, ((size_t)i * 3 * H + y) * W, plane);
            } else if (kind == ROW_OUTPUT) {
                if (half) SPAN(SEG_ZERO, nullptr, false, 0, 0);
                else SPAN(SEG_VIRIDIS, a.output, false, row1, 0);
            } else if (kind == ROW_SPARSE) {
                if (half) SPAN(SEG_ERR_SPARSE, nullptr, false, row1, 0);
                else SPAN(SEG_VIRIDIS, a.sparse, false, row1, 0);
            } else {
                if (half) SPAN(SEG_ERR_GT, nullptr, false, row1, 0);
                else SPAN(SEG_VIRIDIS, a.gt, false, row1, 0);
            }
#undef SPAN
        }
    }
}

__device__ __forceinline__ int flag_bits(float v) { return (v > 10.0f ? 1 : 0) | (v != v ? 2 : 0); }

// bit 0: some element > 10; bit 1: some element is NaN.  One word per block; a union, so the order of the elements cannot matter.
__global__ __launch_bounds__(256) void summary_flag_partial_kernel(const float* __restrict__ x, long count, int* __restrict__ partial) {
    const long head = min(count, (long)(((16u - (unsigned)((uintptr_t)x & 15u)) & 15u) / 4u));          // elements in front of the first 16-byte line
    const long nvec = (count - head) / 4, tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nthr = (long)gridDim.x * blockDim.x;
    const float4* xv = (const float4*)(x + head);
    int bits = 0;
    for (long i = tid; i < nvec; i += nthr) {
        const float4 v = xv[i];
        bits |= flag_bits(v.x) | flag_bits(v.y) | flag_bits(v.z) | flag_bits(v.w);
    }
    for (long i = tid; i < head; i += nthr) bits |= flag_bits(x[i]);
    for (long i = head + 4 * nvec + tid; i < count; i += nthr) bits |= flag_bits(x[i]);
    const int above = __syncthreads_or(bits & 1), nan = __syncthreads_or(bits & 2);
    if (threadIdx.x == 0) partial[blockIdx.x] = (above ? 1 : 0) | (nan ? 2 : 0);
}
__global__ __launch_bounds__(FLAG_BLOCKS) void summary_flag_final_kernel(const int* __restrict__ partial, int nblocks, int* __restrict__ flag) {
    const int bits = (int)threadIdx.x < nblocks ? partial[threadIdx.x] : 0;
    const int above = __syncthreads_or(bits & 1), nan = __syncthreads_or(bits & 2);
    if (threadIdx.x == 0) flag[0] = (above && !nan) ? 1 : 0;
}

constexpr int64_t LIMIT = (int64_t)1 << 31;

// 0 and the grid's sizes, or -22: an argument below 1, or 3 GH GW >= 2^31
int grid_shape(int n_show, int height, int width, int n_rows, int64_t* gh, int64_t* gw) {
    if (n_show < 1 || height < 1 || width < 1 || n_rows < 1) return -22;
    if ((int64_t)width >= LIMIT / 2) return -22;                               // GW >= 2 width; below, n_show (2 width + 2) < 2^62
    const int64_t h = (int64_t)n_rows * height + (n_show > 1 ? 4 : 0);
    const int64_t w = n_show > 1 ? (int64_t)n_show * (2 * (int64_t)width + 2) + 2 : 2 * (int64_t)width;
    if (h >= LIMIT || w >= LIMIT || h * w >= (LIMIT + 2) / 3) return -22;      // h w < 2^62; 3 h w >= 2^31 <=> h w >= ceil(2^31 / 3)
    *gh = h; *gw = w;
    return 0;
}

template <bool VEC>
void launch(dim3 grid, int threads, hipStream_t stream, const SummaryArgs& k, bool u8) {
    if (u8) hipLaunchKernelGGL((summary_compose_kernel<VEC, true>), grid, dim3(threads), 0, stream, k);
    else hipLaunchKernelGGL((summary_compose_kernel<VEC, false>), grid, dim3(threads), 0, stream, k);
}

}  // namespace

extern "C" int ptta_summary_grid_shape(int n_show, int height, int width, int n_rows, int64_t* grid_height_host, int64_t* grid_width_host) {
    int64_t h = 0, w = 0;
    const int rc = grid_shape(n_show, height, width, n_rows, &h, &w);
    if (rc != 0) return rc;
    if (grid_height_host) *grid_height_host = h;
    if (grid_width_host) *grid_width_host = w;
    return 0;
}

extern "C" int ptta_summary_image_flag(const float* image, int64_t count, int32_t* flag, ptta_stream stream) {
    if (!image || !flag || count < 1 || ((uintptr_t)image & 3u) || ((uintptr_t)flag & 3u)) return -22;
    const int64_t want = (count + 256 * 16 - 1) / (256 * 16);                  // four 16-byte loads per lane before a block is added
    const int nblocks = (int)(want > FLAG_BLOCKS ? FLAG_BLOCKS : want);
    hipLaunchKernelGGL(summary_flag_partial_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, image, (long)count, (int*)flag + 1);
    hipLaunchKernelGGL(summary_flag_final_kernel, dim3(1), dim3(FLAG_BLOCKS), 0, (hipStream_t)stream, (const int*)flag + 1, nblocks, (int*)flag);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int ptta_summary_compose(const ptta_summary_args* a, ptta_stream stream) {
    if (!a || !a->out) return -22;
    if (a->n_images < 0 || a->n_images > PTTA_SUMMARY_MAX_IMAGES) return -22;
    const int known = PTTA_SUMMARY_ROW_OUTPUT | PTTA_SUMMARY_ROW_SPARSE | PTTA_SUMMARY_ROW_GT;
    if (a->rows & ~known) return -22;
    if (a->out_dtype != PTTA_SUMMARY_OUT_F32_CHW && a->out_dtype != PTTA_SUMMARY_OUT_U8_HWC) return -22;
    const bool r_out = a->rows & PTTA_SUMMARY_ROW_OUTPUT, r_sp = a->rows & PTTA_SUMMARY_ROW_SPARSE, r_gt = a->rows & PTTA_SUMMARY_ROW_GT;
    SummaryArgs k = {};
    int R = 0;
    for (int i = 0; i < a->n_images; ++i) {
        if (!a->image[i]) return -22;
        k.image[i] = a->image[i]; k.div255[i] = (const int*)a->image_div255[i]; k.kind[R++] = ROW_IMAGE;
    }
    if (r_out) k.kind[R++] = ROW_OUTPUT;
    if (r_sp) k.kind[R++] = ROW_SPARSE;
    if (r_gt) k.kind[R++] = ROW_GT;
    if (R == 0) return -22;
    if ((r_out && !a->output_depth) || (r_sp && (!r_out || !a->sparse_depth || !a->validity_map)) || (r_gt && (!r_out || !a->ground_truth))) return -22;
    if (!(a->max_predict_depth > 0.f) || !std::isfinite(a->max_predict_depth)) return -22;
    if ((r_out && !a->viridis) || ((r_sp || r_gt) && !a->inferno)) return -22;
    int64_t gh = 0, gw = 0;
    if (grid_shape(a->n_show, a->height, a->width, R, &gh, &gw) != 0) return -22;
    k.output = a->output_depth; k.sparse = a->sparse_depth; k.validity = a->validity_map; k.gt = a->ground_truth;
    k.viridis = r_out ? a->viridis : nullptr; k.inferno = (r_sp || r_gt) ? a->inferno : nullptr;
    k.out = a->out;
    k.ns = a->n_show; k.H = a->height; k.W = a->width; k.R = R; k.GH = (int)gh; k.GW = (int)gw; k.pad = a->n_show > 1 ? 2 : 0;
    k.normalize = a->normalize ? 1 : 0; k.maxd = a->max_predict_depth;
    for (int c = 0; c < 3; ++c) { k.rm[c] = a->rev_mean[c]; k.rs[c] = a->rev_std[c]; }
    const bool u8 = a->out_dtype == PTTA_SUMMARY_OUT_U8_HWC;
    // one misalignment for a span's three channel planes: the plane size a multiple of 4 elements on a 16-byte-aligned base; the uint8
    // form keeps a pixel's channels together and needs only a 4-byte-aligned base
    const bool vec = u8 ? ((uintptr_t)a->out & 3u) == 0 : (((uintptr_t)a->out & 15u) == 0 && (gh * gw) % 4 == 0);
    const int units = vec ? (a->width + 3) / 4 + 1 : a->width;                 // lanes a span needs (+ 1: the groups lie on the destination's grid)
    const int threads = units >= 512 ? 256 : (units + 63) / 64 * 64;
    const long xb = ((long)units + threads - 1) / threads;
    k.xb = (int)(xb > 16384 ? 16384 : xb);
    const unsigned gz = (unsigned)(a->n_show > 65535 ? 65535 : a->n_show);
    long gyb = BLOCK_BUDGET / (2L * k.xb * gz);
    gyb = gyb < 1 ? 1 : (gyb > gh ? gh : gyb);
    dim3 grid((unsigned)(2 * k.xb), (unsigned)(gyb > 65535 ? 65535 : gyb), gz);
    if (vec) launch<true>(grid, threads, (hipStream_t)stream, k, u8);
    else launch<false>(grid, threads, (hipStream_t)stream, k, u8);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
