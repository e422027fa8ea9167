// Raw-frame egress on device: the inverse of ingest.hip, prediction -> the 16-bit map the datasets store.  The reference does this on the
// host, per frame: save_depth = np.uint32(z * multiplier) written as a 16-bit PNG (src/data_utils.py:236-251), save_validity_map = v > 0 ->
// 256 (:283-298), save_image = np.uint8(255 * image) transposed to HWC (:29-78), after a 4-byte-per-pixel copy of the fp32 map to the host.
// Here one launch makes the stored frames on the card and 2 bytes per pixel (2 + 2 + 3 with validity and image) leave it:
//   depth_u16[b, sy + y, sx + x]     = p > 0 ? (uint16) min(trunc(p), 65535) : 0     p = depth[b, 0, y, x] * multiplier, one fp32 multiply
//   validity_u16[b, sy + y, sx + x]  = validity[b, 0, y, x] > 0 ? 256 : 0
//   image_u8[b, sy + y, sx + x, c]   = q > 0 ? (uint8) min(trunc(q), 255) : 0        q = image[b, c, y, x] * image_scale
// and every element of the dst_height x dst_width frame outside the window [sy : sy + h, sx : sx + w] is 0.
// Where the reference is defined (0 <= p < 2^31: np.uint32 truncates, Pillow's 16-bit PNG writer stores 65535 for everything at or above
// 65536; 0 <= q < 256: np.uint8 truncates) the bits are the reference's.  Outside it the reference's result is an accident of casts (a
// negative or NaN float -> unsigned cast is undefined in numpy, p >= 2^31 turns negative in Pillow's signed mode 'I', np.uint8 wraps) and
// the project defines: negative, -0 and NaN give 0; at or above the top of the range, +inf included, gives the top (65535 / 255).
// A pure stream: 4-20 B read and 2-7 B written per window pixel, so the access shape is the work.  One block of whole waves per OUTPUT
// row (blocks of 256 lanes side by side once a row needs 512 lanes; beyond BLOCK_BUDGET blocks a block strides over several rows); the
// border is written in the same pass as the window: every output byte exactly once, nothing cleared first, no byte outside the outputs
// written and none outside the inputs read.
//   16-bit planes  a row starts 2 (b H W + y W) bytes from its base: any even alignment.  The lanes' groups are laid on the DESTINATION's
//           16-byte grid (as summary.hip lays its spans): with m = the row's offset inside a 16-byte line in pixels, lane k takes pixels
//           8 k - m ... 8 k - m + 7; the first and the last lane of a row store their 1-7 pixels one by one (the scalar head and tail),
//           every other lane one aligned 16-byte store.  m is per plane: the two bases need not share an alignment.
//   image   a lane takes 4 pixels = 12 bytes, three 32-bit stores when the row's first byte is word-aligned (3 (b H W + y W) and the
//           base: uniform over the block), byte stores otherwise and for the last 1-3 pixels of a row.
//   loads   a lane whose pixels all lie inside the window reads them as 16-byte loads at the source's own 4-byte alignment (the window's
//           offset shifts them against the stores); a lane on the window's edge reads pixel by pixel and only inside the window.
// Plain stores only; each output element has one writer, so results are bit-identical from run to run.
#include <stdint.h>

#include <cmath>

#include "ptta_common.h"
#include "ptta_kernels.h"
#include "../../include/ptta.h"

#pragma clang fp contract(off)

namespace {

struct EgressArgs {
    const float* depth;              // [n][1][h][w]
    const float* validity;
    const float* image;              // [n][3][h][w]
    unsigned short* depth_out;       // [n][H][W]
    unsigned short* validity_out;
    unsigned char* image_out;        // [n][H][W][3]
    const int* start_y;
    const int* start_x;
    int n, H, W, h, w;
    float multiplier, image_scale;
};

constexpr int BLOCK_BUDGET = 2048;            // blocks of one launch: 8 per CU (as summary.hip)

struct alignas(4) Floats4 { float v[4]; };          // a 16-byte load that only promises the 4-byte alignment a float array has
struct alignas(4) Bytes12 { unsigned a, b, c; };

__device__ __forceinline__ unsigned depth_u16(float z, float multiplier) {
    const float p = z * multiplier;
    return p > 0.0f ? (p < 65535.0f ? (unsigned)p : 65535u) : 0u;          // NaN compares false: 0
}
__device__ __forceinline__ unsigned validity_u16(float v) { return v > 0.0f ? 256u : 0u; }
__device__ __forceinline__ unsigned image_u8(float c, float scale) {
    const float q = c * scale;
    return q > 0.0f ? (q < 255.0f ? (unsigned)q : 255u) : 0u;
}

// CNT pixels of a source row (NULL: a border row) from window column xs on; columns outside [0, w) read as 0, which every rule maps to 0
template <int CNT>
__device__ __forceinline__ void load_px(const float* row, long xs, int w, float (&v)[CNT]) {
    if (row != nullptr && xs >= 0 && xs + CNT <= w) {
#pragma unroll
        for (int j = 0; j < CNT; j += 4) {
            const Floats4 f = *(const Floats4*)(row + xs + j);
            v[j] = f.v[0]; v[j + 1] = f.v[1]; v[j + 2] = f.v[2]; v[j + 3] = f.v[3];
        }
    } else {
#pragma unroll
        for (int j = 0; j < CNT; ++j) v[j] = (row != nullptr && xs + j >= 0 && xs + j < w) ? row[xs + j] : 0.0f;
    }
}

// pixels X0 ... X0 + 7 of a 16-bit output row; X0 is a multiple of 8 pixels from a 16-byte line, partial at the row's two ends
__device__ __forceinline__ void store_u16x8(unsigned short* orow, long X0, int W, const unsigned (&q)[8]) {
    if (X0 >= 0 && X0 + 8 <= W) {
        *(uint4*)(orow + X0) = make_uint4(q[0] | (q[1] << 16), q[2] | (q[3] << 16), q[4] | (q[5] << 16), q[6] | (q[7] << 16));
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (X0 + j >= 0 && X0 + j < W) orow[X0 + j] = (unsigned short)q[j];
    }
}

// grid: x = blocks along a row, y = output rows, z = samples (the last two strided: any H and n)
// DEP / VAL / IMG: which planes the call has (one straight-line body per combination: its loads are issued together)
template <bool DEP, bool VAL, bool IMG>
__global__ __launch_bounds__(512) void egress_raw_kernel(const EgressArgs a) {
    const size_t src_plane = (size_t)a.h * a.w, dst_plane = (size_t)a.H * a.W;
    const int W = a.W, w = a.w;
    const long units16 = (W + 7) / 8 + 1, units_img = (W + 3) / 4;          // (+ 1: the groups lie on the destination's grid)
    const long units = (DEP || VAL) ? (IMG && units_img > units16 ? units_img : units16) : units_img;
    for (int b = blockIdx.z; b < a.n; b += gridDim.z) {
        int y0 = a.start_y ? a.start_y[b] : 0, x0 = a.start_x ? a.start_x[b] : 0;
        y0 = min(max(y0, 0), a.H - a.h); x0 = min(max(x0, 0), W - w);         // as ptta_ingest_raw and ptta_crop_flip clamp
        for (int Y = blockIdx.y; Y < a.H; Y += gridDim.y) {
            const size_t dst_row = (size_t)b * dst_plane + (size_t)Y * W;       // the row's first element in a one-channel output
            const int y = Y - y0;
            const bool inside = y >= 0 && y < a.h;
            const size_t src_row = (size_t)b * src_plane + (size_t)(inside ? y : 0) * w;
            const float* drow = (DEP && inside) ? a.depth + src_row : nullptr;
            const float* vrow = (VAL && inside) ? a.validity + src_row : nullptr;
            const float* irow = (IMG && inside) ? a.image + 2 * (size_t)b * src_plane + src_row : nullptr;      // channel 0; 3 planes per sample
            unsigned short* dout = a.depth_out + dst_row;
            unsigned short* vout = a.validity_out + dst_row;
            unsigned char* iout = a.image_out + 3 * dst_row;
            const int md = DEP ? (int)(((uintptr_t)dout & 15u) >> 1) : 0, mv = VAL ? (int)(((uintptr_t)vout & 15u) >> 1) : 0;
            const bool iword = IMG && ((uintptr_t)iout & 3u) == 0;
            for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < units; k += (long)gridDim.x * blockDim.x) {
                const long Xd = 8 * k - md, Xv = 8 * k - mv, Xi = 4 * k;
                const bool do_d = DEP && Xd < W, do_v = VAL && Xv < W, do_i = IMG && Xi < W;
                float zd[8], zv[8], zi[3][4];
                if (do_d) load_px<8>(drow, Xd - x0, w, zd);                    // every load first, then the stores
                if (do_v) load_px<8>(vrow, Xv - x0, w, zv);
                if (do_i) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) load_px<4>(irow ? irow + c * src_plane : nullptr, Xi - x0, w, zi[c]);
                }
                if (do_d) {
                    unsigned q[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) q[j] = depth_u16(zd[j], a.multiplier);
                    store_u16x8(dout, Xd, W, q);
                }
                if (do_v) {
                    unsigned q[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) q[j] = validity_u16(zv[j]);
                    store_u16x8(vout, Xv, W, q);
                }
                if (do_i) {
                    unsigned q[12];                                             // r g b r | g b r g | b r g b
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int c = 0; c < 3; ++c) q[3 * j + c] = image_u8(zi[c][j], a.image_scale);
                    if (iword && Xi + 4 <= W) {
                        Bytes12 o;
                        o.a = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
                        o.b = q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24);
                        o.c = q[8] | (q[9] << 8) | (q[10] << 16) | (q[11] << 24);
                        *(Bytes12*)(iout + 3 * Xi) = o;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (Xi + j < W) {
                                unsigned char* o = iout + 3 * (Xi + j);
                                o[0] = (unsigned char)q[3 * j]; o[1] = (unsigned char)q[3 * j + 1]; o[2] = (unsigned char)q[3 * j + 2];
                            }
                    }
                }
            }
        }
    }
}

void launch(dim3 grid, int threads, hipStream_t stream, const EgressArgs& a) {
#define EGRESS_CASE(D, V, I)                                                                                                    \
    if ((a.depth != nullptr) == D && (a.validity != nullptr) == V && (a.image != nullptr) == I)                                 \
        hipLaunchKernelGGL((egress_raw_kernel<D, V, I>), grid, dim3(threads), 0, stream, a)
    EGRESS_CASE(true, true, true); EGRESS_CASE(true, true, false); EGRESS_CASE(true, false, true); EGRESS_CASE(true, false, false);
    EGRESS_CASE(false, true, true); EGRESS_CASE(false, true, false); EGRESS_CASE(false, false, true);
#undef EGRESS_CASE
}

}  // namespace

extern "C" int ptta_egress_raw(const float* depth, const float* validity, const float* image, uint16_t* depth_u16, uint16_t* validity_u16,
                               uint8_t* image_u8, int n, int height, int width, int dst_height, int dst_width, const int32_t* start_y,
                               const int32_t* start_x, float multiplier, float image_scale, ptta_stream stream) {
    if (!depth && !validity && !image) return ptta_refuse_args("ptta_egress_raw: no input plane (depth, validity and image are all NULL)");
    if (!depth != !depth_u16 || !validity != !validity_u16 || !image != !image_u8)
        return ptta_refuse_args("ptta_egress_raw: an input and its output come together (depth / depth_u16, validity / validity_u16, image / image_u8)");
    if (n < 1) return ptta_refuse_args("ptta_egress_raw: n must be at least 1");
    if (height < 1 || width < 1 || dst_height < 1 || dst_width < 1) return ptta_refuse_args("ptta_egress_raw: every size must be at least 1");
    if (height > dst_height || width > dst_width) return ptta_refuse_args("ptta_egress_raw: the height x width window does not fit the dst_height x dst_width frame");
    if (!(multiplier > 0.f) || !std::isfinite(multiplier)) return ptta_refuse_args("ptta_egress_raw: multiplier must be a positive finite number");
    if (!(image_scale > 0.f) || !std::isfinite(image_scale)) return ptta_refuse_args("ptta_egress_raw: image_scale must be a positive finite number");
    if ((((uintptr_t)depth_u16 | (uintptr_t)validity_u16) & 1u) != 0) return ptta_refuse_args("ptta_egress_raw: depth_u16 and validity_u16 must be 2-byte aligned");
    EgressArgs a;
    a.depth = depth; a.validity = validity; a.image = image;
    a.depth_out = depth_u16; a.validity_out = validity_u16; a.image_out = image_u8;
    a.start_y = start_y; a.start_x = start_x;
    a.n = n; a.H = dst_height; a.W = dst_width; a.h = height; a.w = width; a.multiplier = multiplier; a.image_scale = image_scale;
    const long units16 = ((long)dst_width + 7) / 8 + 1, units_img = ((long)dst_width + 3) / 4;          // lanes a row needs, as the kernel counts them
    const long units = (depth || validity) ? (image && units_img > units16 ? units_img : units16) : units_img;
    const int threads = units >= 512 ? 256 : (int)((units + 63) / 64 * 64);       // one block per row up to 511 lanes, whole waves
    long xb = (units + threads - 1) / threads;
    xb = xb > 65535 ? 65535 : xb;
    const long gz = n > 65535 ? 65535 : n;
    // a block per row while the launch stays within BLOCK_BUDGET blocks; beyond it a block strides over several rows, so that its
    // prologue (the kernel arguments, the sample's starts) is paid once for all of them
    long gy = BLOCK_BUDGET / (xb * gz);
    gy = gy < 1 ? 1 : (gy > dst_height ? dst_height : gy);
    dim3 grid((unsigned)xb, (unsigned)gy, (unsigned)gz);
    launch(grid, threads, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
