// Raw-frame ingest on device: the first link of the chain, decoded file -> frame the step can read.  The reference does this on the
// host, per frame and before collation: load_image(normalize=False, 'CHW') = np.asarray(image, np.float32) + np.transpose(image, (2, 0, 1))
// (src/data_utils.py:150-158, called at src/datasets.py:399-407), load_depth = z / multiplier (:219-223), load_depth_with_validity_map =
// z / 256.0 and v[z > 0] = 1 (:182-188), then the random / bottom crop on the float arrays (src/datasets.py:83-170).  Here the decoded
// uint8 H x W x 3 image and the 16-bit depth maps travel as they are (5 bytes per pixel instead of 16) and one launch writes the fp32 planes:
//   image_out[b, c, y, x]  = (float) image_u8[b, sy + y, sx + x, c]                      0..255, exact
//   sparse_out[b, 0, y, x] = (float) sparse_u16[b, sy + y, sx + x] / multiplier          one IEEE division (a 16-bit integer converts exactly)
//   validity_out           = sparse_out > 0 ? 1 : 0                                      gt_out / gt_validity_out: the same from gt_u16
// A pure stream: up to 5 B read and 20 B written per pixel, so the access shape is the work.  One block of whole waves per output row (blocks of
// 256 lanes side by side once a row needs 512 lanes: 2,048 pixels with 16-byte stores).
//   stores  width % 4 == 0 and 16-byte-aligned output bases: a lane owns 4 consecutive pixels of a row and writes one 16-byte store per
//           plane (a wave: 1 KiB contiguous per plane).  Anything else takes the one-pixel-per-lane path.
//   loads   a lane's 12 image bytes start at row start + 12 lane, and the row starts at 3 (sx + ...) of a pitch of 3 src_width bytes: any
//           alignment, but the SAME misalignment for every lane of the row (12 = 0 mod 4; the 8 bytes of a 16-bit plane likewise).  A lane
//           reads the aligned 32-bit words that cover its bytes -- 3, plus a 4th when the row is not word-aligned (2 plus a 3rd for a
//           16-bit plane) -- all of them issued before the first is used, and v_alignbyte_b32 shifts the bytes into place by the row's
//           (wave-uniform) offset.  Neighbouring lanes share the straddled word.
//   bounds  the words that cover a row lie inside the row's own array unless the row begins within 3 bytes of the array's first byte and
//           that base is not word-aligned, or ends within 3 bytes of its last byte and that end is not word-aligned -- the last pixels of
//           the last row of the last sample, when the window reaches them.  Those (at most two) rows are recognised per block,
//           `words_inside` below, and read byte by byte; every other row reads only words that lie wholly inside [base, base + bytes).
//           No byte outside the three source arrays is ever read.
// Division: csrc/Makefile leaves hipcc's correctly rounded fp32 division on (no fast-math flag), so `/` below is the IEEE quotient.
#include <stdint.h>

#include <cmath>

#include "ptta_common.h"
#include "../../include/ptta.h"

namespace {

struct IngestArgs {
    const unsigned char* image;      // [n][H][W][3]
    const unsigned char* sparse;     // [n][H][W] uint16, addressed in bytes
    const unsigned char* gt;
    float* image_out;                // [n][3][h][w]
    float* sparse_out;               // [n][1][h][w]
    float* validity_out;
    float* gt_out;
    float* gt_validity_out;
    const int* start_y;
    const int* start_x;
    int n, H, W, h, w;
    float multiplier;
};

// the aligned words covering the row [row, row + bytes) lie inside the array [base, base + total)
__device__ __forceinline__ bool words_inside(const unsigned char* base, size_t total, const unsigned char* row, size_t bytes) {
    const uintptr_t lo = (uintptr_t)base, hi = lo + total, r0 = (uintptr_t)row & ~(uintptr_t)3, r1 = ((uintptr_t)row + bytes + 3) & ~(uintptr_t)3;
    return r0 >= lo && r1 <= hi;
}
// the NW (+1 when off != 0) aligned words that cover the 4 NW bytes at p; off = p & 3 is uniform over the row
template <int NW>
__device__ __forceinline__ void load_words(const unsigned char* p, unsigned off, unsigned (&wd)[NW + 1]) {
    const unsigned* q = (const unsigned*)(p - off);
#pragma unroll
    for (int k = 0; k < NW; ++k) wd[k] = q[k];
    wd[NW] = q[off ? NW : NW - 1];          // branch-free: an aligned row reads its last word twice and the shift by 0 ignores it
}
template <int NW>
__device__ __forceinline__ void load_bytes(const unsigned char* p, unsigned (&wd)[NW + 1]) {
#pragma unroll
    for (int k = 0; k < NW; ++k)
        wd[k] = (unsigned)p[4 * k] | ((unsigned)p[4 * k + 1] << 8) | ((unsigned)p[4 * k + 2] << 16) | ((unsigned)p[4 * k + 3] << 24);
    wd[NW] = 0u;
}
template <int NW>
__device__ __forceinline__ void align_words(unsigned (&wd)[NW + 1], unsigned off) {
#pragma unroll
    for (int k = 0; k < NW; ++k) wd[k] = __builtin_amdgcn_alignbyte(wd[k + 1], wd[k], off);      // ({wd[k+1], wd[k]} >> 8 off), low word
}
__device__ __forceinline__ float4 depth4(const unsigned (&r)[3], float multiplier) {
    return make_float4((float)(r[0] & 0xffffu) / multiplier, (float)(r[0] >> 16) / multiplier,
                       (float)(r[1] & 0xffffu) / multiplier, (float)(r[1] >> 16) / multiplier);
}
__device__ __forceinline__ float4 valid4(const float4& d) {
    return make_float4(d.x > 0.f ? 1.f : 0.f, d.y > 0.f ? 1.f : 0.f, d.z > 0.f ? 1.f : 0.f, d.w > 0.f ? 1.f : 0.f);
}

// grid: x = blocks along a row, y = rows, z = samples (the last two strided: any h and n)
// IMG / SP / GT: which inputs the call has (one straight-line body per combination: its loads are issued together)
template <bool VEC, bool IMG, bool SP, bool GT>
__global__ __launch_bounds__(512) void ingest_raw_kernel(const IngestArgs a) {
    const size_t src_plane = (size_t)a.H * a.W, dst_plane = (size_t)a.h * a.w;
    for (int b = blockIdx.z; b < a.n; b += gridDim.z) {
        int y0 = a.start_y ? a.start_y[b] : 0, x0 = a.start_x ? a.start_x[b] : 0;
        y0 = min(max(y0, 0), a.H - a.h); x0 = min(max(x0, 0), a.W - a.w);     // as ptta_crop_flip: an out-of-range start never leaves the sample
        for (int y = blockIdx.y; y < a.h; y += gridDim.y) {
            const size_t src_px = (size_t)b * src_plane + (size_t)(y0 + y) * a.W + x0;          // first source pixel of the row
            const size_t dst_row = (size_t)b * dst_plane + (size_t)y * a.w;                     // its place in a one-channel output
            if (VEC) {
                const unsigned char* irow = a.image + 3 * src_px;
                const unsigned char* srow = a.sparse + 2 * src_px;
                const unsigned char* grow = a.gt + 2 * src_px;
                const unsigned ioff = (unsigned)((uintptr_t)irow & 3u), soff = (unsigned)((uintptr_t)srow & 3u), goff = (unsigned)((uintptr_t)grow & 3u);
                const bool words = (!IMG || words_inside(a.image, 3 * src_plane * a.n, irow, 3 * (size_t)a.w)) &&
                                   (!SP || words_inside(a.sparse, 2 * src_plane * a.n, srow, 2 * (size_t)a.w)) &&
                                   (!GT || words_inside(a.gt, 2 * src_plane * a.n, grow, 2 * (size_t)a.w));
                // (unsigned: the last stride past a width near 2^31 still fits)
                for (unsigned x = 4u * (blockIdx.x * blockDim.x + threadIdx.x); x < (unsigned)a.w; x += 4u * gridDim.x * blockDim.x) {
                    unsigned ri[4], rs[3], rg[3];
                    if (words) {                                    // every load first, then the shifts
                        if (IMG) load_words<3>(irow + 3 * (size_t)x, ioff, ri);
                        if (SP) load_words<2>(srow + 2 * (size_t)x, soff, rs);
                        if (GT) load_words<2>(grow + 2 * (size_t)x, goff, rg);
                        if (IMG) align_words<3>(ri, ioff);
                        if (SP) align_words<2>(rs, soff);
                        if (GT) align_words<2>(rg, goff);
                    } else {                                        // a row at an end of an array that is not word-aligned there
                        if (IMG) load_bytes<3>(irow + 3 * (size_t)x, ri);
                        if (SP) load_bytes<2>(srow + 2 * (size_t)x, rs);
                        if (GT) load_bytes<2>(grow + 2 * (size_t)x, rg);
                    }
                    if (IMG) {                                  // 12 bytes: r g b r | g b r g | b r g b
                        float* o = a.image_out + 3 * (size_t)b * dst_plane + (size_t)y * a.w + x;
                        *(float4*)o = make_float4((float)(ri[0] & 0xffu), (float)(ri[0] >> 24), (float)((ri[1] >> 16) & 0xffu), (float)((ri[2] >> 8) & 0xffu));
                        *(float4*)(o + dst_plane) = make_float4((float)((ri[0] >> 8) & 0xffu), (float)(ri[1] & 0xffu), (float)(ri[1] >> 24), (float)((ri[2] >> 16) & 0xffu));
                        *(float4*)(o + 2 * dst_plane) = make_float4((float)((ri[0] >> 16) & 0xffu), (float)((ri[1] >> 8) & 0xffu), (float)(ri[2] & 0xffu), (float)(ri[2] >> 24));
                    }
                    if (SP) {
                        const float4 d = depth4(rs, a.multiplier);
                        *(float4*)(a.sparse_out + dst_row + x) = d;
                        if (a.validity_out) *(float4*)(a.validity_out + dst_row + x) = valid4(d);
                    }
                    if (GT) {
                        const float4 d = depth4(rg, a.multiplier);
                        *(float4*)(a.gt_out + dst_row + x) = d;
                        if (a.gt_validity_out) *(float4*)(a.gt_validity_out + dst_row + x) = valid4(d);
                    }
                }
            } else {
                for (unsigned x = blockIdx.x * blockDim.x + threadIdx.x; x < (unsigned)a.w; x += gridDim.x * blockDim.x) {
                    if (IMG) {
                        const unsigned char* p = a.image + 3 * (src_px + x);
                        float* o = a.image_out + 3 * (size_t)b * dst_plane + (size_t)y * a.w + x;
                        o[0] = (float)p[0]; o[dst_plane] = (float)p[1]; o[2 * dst_plane] = (float)p[2];
                    }
                    if (SP) {
                        const float d = (float)((const unsigned short*)a.sparse)[src_px + x] / a.multiplier;
                        a.sparse_out[dst_row + x] = d;
                        if (a.validity_out) a.validity_out[dst_row + x] = d > 0.f ? 1.f : 0.f;
                    }
                    if (GT) {
                        const float d = (float)((const unsigned short*)a.gt)[src_px + x] / a.multiplier;
                        a.gt_out[dst_row + x] = d;
                        if (a.gt_validity_out) a.gt_validity_out[dst_row + x] = d > 0.f ? 1.f : 0.f;
                    }
                }
            }
        }
    }
}

template <bool VEC>
void launch(dim3 grid, int threads, hipStream_t stream, const IngestArgs& a) {
#define INGEST_CASE(I, S, G)                                                                                                    \
    if ((a.image != nullptr) == I && (a.sparse != nullptr) == S && (a.gt != nullptr) == G)                                      \
        hipLaunchKernelGGL((ingest_raw_kernel<VEC, I, S, G>), grid, dim3(threads), 0, stream, a)
    INGEST_CASE(true, true, true); INGEST_CASE(true, true, false); INGEST_CASE(true, false, true); INGEST_CASE(true, false, false);
    INGEST_CASE(false, true, true); INGEST_CASE(false, true, false); INGEST_CASE(false, false, true);
#undef INGEST_CASE
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int ptta_ingest_raw(const uint8_t* image_u8, const uint16_t* sparse_u16, const uint16_t* gt_u16, float* image_out,
                               float* sparse_out, float* validity_out, float* gt_out, float* gt_validity_out, int n, int src_height,
                               int src_width, int height, int width, const int32_t* start_y, const int32_t* start_x, float multiplier,
                               ptta_stream stream) {
    if (!image_u8 && !sparse_u16 && !gt_u16) return -22;
    if (!image_u8 != !image_out || !sparse_u16 != !sparse_out || !gt_u16 != !gt_out) return -22;      // an input and its plane come together
    if ((validity_out && !sparse_u16) || (gt_validity_out && !gt_u16)) return -22;
    if (n < 1 || src_height < 1 || src_width < 1 || height < 1 || width < 1 || height > src_height || width > src_width) return -22;
    if (!(multiplier > 0.f) || !std::isfinite(multiplier)) return -22;
    IngestArgs a;
    a.image = image_u8; a.sparse = (const unsigned char*)sparse_u16; a.gt = (const unsigned char*)gt_u16;
    a.image_out = image_out; a.sparse_out = sparse_out; a.validity_out = validity_out; a.gt_out = gt_out; a.gt_validity_out = gt_validity_out;
    a.start_y = start_y; a.start_x = start_x;
    a.n = n; a.H = src_height; a.W = src_width; a.h = height; a.w = width; a.multiplier = multiplier;
    // 16-byte stores need every row of every plane on a 16-byte boundary: width % 4 == 0 (plane sizes follow) and aligned bases;
    // the 16-bit planes are read as words there, so a row's misalignment must be 0 or 2: even bases (they are uint16 arrays)
    const bool vec = width % 4 == 0 && aligned16(image_out) && aligned16(sparse_out) && aligned16(validity_out) && aligned16(gt_out) &&
                     aligned16(gt_validity_out) && (((uintptr_t)sparse_u16 | (uintptr_t)gt_u16) & 1u) == 0;
    const int units = vec ? width / 4 : width;                 // lanes a row needs
    const int threads = units >= 512 ? 256 : (units + 63) / 64 * 64;        // one block per row up to 511 lanes, whole waves
    const long xb = ((long)units + threads - 1) / threads;
    dim3 grid((unsigned)(xb > 65535 ? 65535 : xb), (unsigned)(height > 65535 ? 65535 : height), (unsigned)(n > 65535 ? 65535 : n));
    if (vec) launch<true>(grid, threads, (hipStream_t)stream, a);
    else launch<false>(grid, threads, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
