// Eval-time hole filling of the NLSPN adapter on the device (src/nlspn_model_adapt.py:124-127 -> skimage.restoration.inpaint_biharmonic,
// restated on scipy in proxytta/inpaint.py, which is the definition this file follows).  Per sample of an N x 1 x H x W fp32 map:
//   holes   M = {depth == 0};  lo, hi = fp32 min / max of the pixels outside M
//   row     for p in M the box B_p = [py-2, py+3) x [px-2, px+3) clipped to the image; c_p = L_B(L_B(delta_p)), L_B the 5-point Laplacian
//           on the BOX with the edge value replicated at the box's edges (scipy.ndimage.laplace, 'reflect').  With the 1-D clipped
//           Laplacian's column a1 at p and the column a2 of its square, per axis,
//             c_p[y, x] = a2_y[y] [x == px] + 2 a1_y[y] a1_x[x] + [y == py] a2_x[x]
//           a1 spans 3 entries and a2 five, so a row has the same 13 places everywhere (a cross of radius 2 plus the 3 x 3 block);
//           only the values change at an image border (the uncut row: 20, -8, 2, 1)
//   system  sum_{q in M} c_p[q] x_q = - sum_{q not in M} c_p[q] (double) depth[q], in fp64; depth[p] = (float) clip(x_p, lo, hi)
// Two holes of different connected regions of the host code share no non-zero coefficient, so one joint system per sample is the same
// system.  It is symmetric and, in every case tried, positive definite: plain conjugate gradients from x = 0, stopped at
// |r| <= rtol |b|.  Positive definiteness is observed, not proven, so nothing here relies on it to end: the loop is bounded by max_iter
// and p.Ap <= 0 or a non-finite scalar ends it with status -1 and the map as it was (x lives in the scratch until the solve succeeded).
//
// Launch 1 (compact): one workgroup of 16 waves per sample.  Wave w owns the contiguous pixel range [w S, (w+1) S): it counts its holes
//   and takes min / max, the 16 counts are scanned through LDS, and a second pass over the same range hands out the raster-order index
//   with a ballot per 64 pixels.  No atomics: the numbering is the raster order whatever the timing.  Writes the H x W index map
//   (-1: known), the unknown list, count / lo / hi, and the status of a sample that needs no solve (0, -2, -3).
// Launch 2 (solve): one workgroup per sample, because everything a CG iteration shares -- two dot products and the vector p -- then
//   stays inside one workgroup: __syncthreads() is the only synchronisation, there is no grid-wide barrier and no workgroup waits on another.
//   A thread owns the unknowns tid, tid + 1024, ...; x, r, Ap are touched by their owner alone, p is read by the 13 neighbours after a
//   barrier.  A row (13 neighbour indices + 13 coefficients, column-major so a wave's loads are contiguous) is built once.  With at most
//   1024 unknowns -- one per thread -- rows and vector entries stay in registers and p goes through 8 KiB of LDS instead.  Each dot
//   product: per-thread partial in index order, a 64-lane butterfly, 16 wave sums through LDS added in wave order by every thread --
//   a fixed order, no fp64 atomics, so the result is bit-identical from run to run and every thread takes the same branch.
// Scratch per sample (ptta_inpaint_scratch_bytes; cap = min(max_unknowns, H W)):
//   [ 64 B header: count, solve flag, lo, hi | H W int32 index map | cap int32 list | 13 cap int32 neighbours | 13 cap float coefficients |
//     x, r, p, Ap: 4 cap doubles ]    each part rounded up to 16 bytes.  A few hundred unknowns stay in L2 throughout.
#include <stdint.h>

#include <cmath>

#include "ptta_common.h"
#include "../../include/ptta.h"

namespace {

constexpr int THREADS = 1024, WAVES = THREADS / 64, NB = 13;

struct Layout {
    int64_t map, list, nbr, coef, vec, total;      // byte offsets inside one sample's part; total: its size
    int cap;
};

__host__ __device__ inline int64_t round16(int64_t b) { return (b + 15) & ~(int64_t)15; }
__host__ __device__ inline Layout layout(int height, int width, int max_unknowns) {
    Layout l;
    const int64_t hw = (int64_t)height * width;
    l.cap = (int)(hw < max_unknowns ? hw : max_unknowns);
    l.map = 64;
    l.list = l.map + round16(4 * hw);
    l.nbr = l.list + round16(4 * (int64_t)l.cap);
    l.coef = l.nbr + round16(4 * (int64_t)NB * l.cap);
    l.vec = l.coef + round16(4 * (int64_t)NB * l.cap);
    l.total = l.vec + round16(8 * (int64_t)4 * l.cap);
    return l;
}

struct InpaintArgs {
    float* depth;
    char* scratch;
    int32_t* status;
    int height, width, max_unknowns, max_iter;
    double rtol;
};

__global__ __launch_bounds__(THREADS) void inpaint_compact_kernel(const InpaintArgs a) {
    __shared__ int s_cnt[WAVES];
    __shared__ float s_lo[WAVES], s_hi[WAVES];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int hw = a.height * a.width;                       // the entry point holds H W below 2^31
    const Layout l = layout(a.height, a.width, a.max_unknowns);
    const float* d = a.depth + (size_t)b * hw;
    char* base = a.scratch + (size_t)b * l.total;
    int32_t* hdr = (int32_t*)base;
    int32_t* map = (int32_t*)(base + l.map);
    int32_t* list = (int32_t*)(base + l.list);
    const int64_t seg = (((int64_t)hw + WAVES - 1) / WAVES + 63) / 64 * 64;
    const int64_t start = (int64_t)wave * seg < hw ? (int64_t)wave * seg : hw, end = start + seg < hw ? start + seg : hw;

    int cnt = 0;
    float lo = INFINITY, hi = -INFINITY;
#pragma unroll 8
    for (int64_t i = start + lane; i < end; i += 64) {
        const float v = d[i];
        if (v == 0.f) ++cnt;
        else { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o);
        const float l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
        lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
    }
    if (lane == 0) { s_cnt[wave] = cnt; s_lo[wave] = lo; s_hi[wave] = hi; }
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < WAVES; ++w) {
        if (w < wave) before += s_cnt[w];
        total += s_cnt[w];
        lo = s_lo[w] < lo ? s_lo[w] : lo; hi = s_hi[w] > hi ? s_hi[w] : hi;
    }
    if (threadIdx.x == 0) {
        const bool solve = total > 0 && total < hw && total <= a.max_unknowns;
        hdr[0] = total; hdr[1] = solve ? 1 : 0;
        ((float*)hdr)[2] = lo; ((float*)hdr)[3] = hi;
        a.status[b] = total == 0 ? 0 : total == hw ? -2 : total > a.max_unknowns ? -3 : -1;      // -1 until the solve has converged
    }
    int running = before;
    for (int64_t i0 = start; i0 < end; i0 += 64) {
        const int64_t i = i0 + lane;
        const bool hole = i < end && d[i] == 0.f;
        const unsigned long long m = __ballot(hole);
        const int id = running + __popcll(m & ((1ull << lane) - 1ull));
        if (i < end) map[i] = hole ? id : -1;
        if (hole && id < l.cap) list[id] = (int32_t)i;
        running += __popcll(m);
    }
}

// column `o` of the 1-D Laplacian on o + 1 + r points (edge value replicated: the diagonal is -1 at an end, -2 inside) and of its square,
// indexed by the distance to the point + 2; zero outside the box
__device__ __forceinline__ void columns(int o, int r, double (&a1)[5], double (&a2)[5]) {
    const int n = o + 1 + r;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int i = o + k - 2;                              // place inside the box
        a1[k] = (i < 0 || i >= n) ? 0.0 : k == 2 ? -2.0 + (i == 0) + (i == n - 1) : (k == 1 || k == 3) ? 1.0 : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int i = o + k - 2;
        const double diag = -2.0 + (i == 0) + (i == n - 1);
        const double v = diag * a1[k] + (k > 0 ? a1[k - 1] : 0.0) + (k < 4 ? a1[k + 1] : 0.0);
        a2[k] = (i < 0 || i >= n) ? 0.0 : v;
    }
}

// the sum of one value per thread over the workgroup, the same bits in every thread; `s` is used by one call at a time (the callers alternate
// between two arrays, and a barrier of the next call lies between a thread's reads here and the next writes to the same array)
__device__ __forceinline__ double block_sum(double v, double* s) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) t += s[w];
    return t;
}

// SMALL: at most THREADS unknowns, one per thread.  The thread keeps its row (13 indices, 13 coefficients) and its entries of x, r, p, Ap in
// registers and p is shared through LDS: an iteration touches no global memory.  Otherwise a thread strides over the unknowns and rows and
// vectors live in the scratch.  The arithmetic and its order are the same in both forms.
template <bool SMALL>
__device__ __forceinline__ void solve(const InpaintArgs& a, const Layout& l, char* base, float* d, int K, int b, double* s_a, double* s_b, double* s_p) {
    const int tid = threadIdx.x, H = a.height, W = a.width;
    const int32_t* hdr = (const int32_t*)base;
    const double lo = (double)((const float*)hdr)[2], hi = (double)((const float*)hdr)[3];
    const int32_t* map = (const int32_t*)(base + l.map);
    const int32_t* list = (const int32_t*)(base + l.list);
    int32_t* nbr = (int32_t*)(base + l.nbr);
    float* coef = (float*)(base + l.coef);
    double* x = (double*)(base + l.vec);
    double* r = x + l.cap;
    double* p = r + l.cap;
    double* Ap = p + l.cap;
    int nq[NB];                                               // SMALL: the thread's row and vector entries
    float cq[NB];
    double xk = 0.0, rk = 0.0, pk = 0.0, apk = 0.0;

    // rows and right-hand side; x = 0, r = p = b
    constexpr int DY[NB] = {-2, -1, -1, -1, 0, 0, 0, 0, 0, 1, 1, 1, 2};
    constexpr int DX[NB] = {0, -1, 0, 1, -2, -1, 0, 1, 2, -1, 0, 1, 0};
    double part = 0.0;
    for (int k = tid; k < K; k += THREADS) {
        const int pix = list[k], py = pix / W, px = pix - py * W;
        double a1y[5], a2y[5], a1x[5], a2x[5];
        columns(py < 2 ? py : 2, H - 1 - py < 2 ? H - 1 - py : 2, a1y, a2y);
        columns(px < 2 ? px : 2, W - 1 - px < 2 ? W - 1 - px : 2, a1x, a2x);
        double rhs = 0.0;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int y = py + DY[j], xx = px + DX[j];
            const double c = (DX[j] == 0 ? a2y[DY[j] + 2] : 0.0) + 2.0 * a1y[DY[j] + 2] * a1x[DX[j] + 2] + (DY[j] == 0 ? a2x[DX[j] + 2] : 0.0);
            int q = -1;
            float cf = 0.f;
            if (y >= 0 && y < H && xx >= 0 && xx < W && c != 0.0) {
                q = map[y * W + xx];
                if (q >= 0) cf = (float)c;                    // small integers: exact
                else rhs -= c * (double)d[y * W + xx];
            }
            if (SMALL) { nq[j] = q; cq[j] = cf; }
            else { nbr[(size_t)j * l.cap + k] = q; coef[(size_t)j * l.cap + k] = cf; }
        }
        if (SMALL) { rk = rhs; pk = rhs; s_p[k] = rhs; }
        else { x[k] = 0.0; r[k] = rhs; p[k] = rhs; }
        part += rhs * rhs;
    }
    double rr = block_sum(part, s_b);
    const double tol2 = a.rtol * a.rtol * rr;                  // |r| <= rtol |b|, squared
    int status = -1;
    if (!(rr == rr) || fabs(rr) == INFINITY) status = -1;
    else if (rr == 0.0) status = 0;                            // b = 0: x = 0 in 0 iterations
    else {
        for (int it = 1; it <= a.max_iter; ++it) {
            __syncthreads();                                   // every entry of p of the last update (or of the set-up) is written
            part = 0.0;
            for (int k = tid; k < K; k += THREADS) {
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    const int q = SMALL ? nq[j] : nbr[(size_t)j * l.cap + k];
                    const double c = (double)(SMALL ? cq[j] : coef[(size_t)j * l.cap + k]);
                    if (q >= 0) s += c * (SMALL ? s_p[q] : p[q]);
                }
                if (SMALL) apk = s; else Ap[k] = s;
                part += (SMALL ? pk : p[k]) * s;
            }
            const double pAp = block_sum(part, s_a);
            if (!(pAp > 0.0) || fabs(pAp) == INFINITY) break;  // breakdown: not positive definite along p, or not finite
            const double alpha = rr / pAp;
            part = 0.0;
            for (int k = tid; k < K; k += THREADS) {
                if (SMALL) {
                    xk += alpha * pk;
                    rk -= alpha * apk;
                    part += rk * rk;
                } else {
                    x[k] += alpha * p[k];
                    const double rn = r[k] - alpha * Ap[k];
                    r[k] = rn;
                    part += rn * rn;
                }
            }
            const double rr_new = block_sum(part, s_b);
            if (!(rr_new == rr_new) || fabs(rr_new) == INFINITY) break;
            if (rr_new <= tol2) { status = it; break; }
            const double beta = rr_new / rr;
            rr = rr_new;
            // (the last read of p in this iteration lies before the two barriers of the sums above)
            for (int k = tid; k < K; k += THREADS) {
                if (SMALL) { pk = rk + beta * pk; s_p[k] = pk; }
                else p[k] = r[k] + beta * p[k];
            }
        }
    }
    if (status < 0) return;                                    // status[b] is -1 from the first launch; the map is as it was
    for (int k = tid; k < K; k += THREADS) {
        double v = SMALL ? xk : x[k];
        v = v < lo ? lo : v; v = v > hi ? hi : v;
        d[list[k]] = (float)v;
    }
    if (tid == 0) a.status[b] = status;
}

__global__ __launch_bounds__(THREADS) void inpaint_solve_kernel(const InpaintArgs a) {
    __shared__ double s_a[WAVES], s_b[WAVES], s_p[THREADS];
    const int b = blockIdx.x;
    const Layout l = layout(a.height, a.width, a.max_unknowns);
    char* base = a.scratch + (size_t)b * l.total;
    const int32_t* hdr = (const int32_t*)base;
    if (hdr[1] != 1) return;                                   // no holes, or the status the first launch wrote; the same in every thread
    const int K = hdr[0];
    float* d = a.depth + (size_t)b * a.height * a.width;
    if (K <= THREADS) solve<true>(a, l, base, d, K, b, s_a, s_b, s_p);
    else solve<false>(a, l, base, d, K, b, s_a, s_b, s_p);
}

}  // namespace

extern "C" int64_t ptta_inpaint_scratch_bytes(int n, int height, int width, int max_unknowns) {
    if (n < 1 || height < 5 || width < 5 || max_unknowns < 1 || (int64_t)height * width > INT32_MAX) return -22;
    const int64_t per_sample = layout(height, width, max_unknowns).total;       // at most 2^31 x 120 bytes
    if (n > INT64_MAX / per_sample) return -22;
    return (int64_t)n * per_sample;
}

extern "C" int ptta_inpaint_biharmonic(float* depth, int n, int height, int width, int max_unknowns, int max_iter, double rtol, void* scratch,
                                       int64_t scratch_bytes, int32_t* status, ptta_stream stream) {
    if (!depth || !scratch || !status) return -22;
    if (n < 1 || height < 5 || width < 5 || max_unknowns < 1 || max_iter < 1) return -22;
    if (!(rtol > 0.0) || !std::isfinite(rtol)) return -22;
    if ((int64_t)height * width > INT32_MAX || ((uintptr_t)scratch & 15u) != 0) return -22;      // int32 pixel indices; 16-byte-aligned parts
    if (scratch_bytes < ptta_inpaint_scratch_bytes(n, height, width, max_unknowns)) return -22;
    InpaintArgs a;
    a.depth = depth; a.scratch = (char*)scratch; a.status = status;
    a.height = height; a.width = width; a.max_unknowns = max_unknowns; a.max_iter = max_iter; a.rtol = rtol;
    hipLaunchKernelGGL(inpaint_compact_kernel, dim3((unsigned)n), dim3(THREADS), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(inpaint_solve_kernel, dim3((unsigned)n), dim3(THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
