// Scoring a run on the device (include/ptta.h ptta_score_accumulate; the reference's scoring tails, src/tta_main.py:755-809 and :975-1030).
// The reference slices output and ground truth to the dataset's window, copies both to the host, masks them and takes four means per
// frame; the driver then keeps `metric * batch_size` sums and divides by n_sample.  Here the window is an argument, the sums live in a
// state in device memory, and nothing is read back until the run's result is asked for.
//   partial  grid (B, n): workgroup (b, s) owns the units b 256 + tid, + B 256, ... of sample s's window; a unit is one pixel, or four
//            consecutive pixels of a row on the 16-byte path (width, win_x, win_width multiples of 4 and both bases aligned, so every
//            group of a window row is one aligned 16-byte line of the map).  B = ceil(units / 1024) capped at 64: a function of the
//            window's size alone.  A thread keeps count and the four sums in fp64 in unit order; 64 lanes are added by a butterfly, the 4
//            waves through LDS in wave order.  One 48-byte partial per workgroup, inside the state.
//   final    ONE workgroup: wave w takes samples w, w + 4, ...: lane l loads partial l of the sample (zero past B), the same butterfly,
//            lane 0 writes the sample's sums and its optional outputs.  After a barrier thread 0 adds the n samples in index order (the
//            pooled sums), forms the batch's metrics and updates the run.
// Order of every addition is fixed by (window, n) alone: no atomics, no workgroup waits on another, every loop is bounded by the arguments,
// so results are bit-identical from run to run.  Only pixels inside the window are read; only the state and the optional outputs written.
// Arithmetic per pixel is a chain of single fp32 operations; contraction is off for this file and csrc/Makefile leaves hipcc's correctly
// rounded division on, so every element equals numpy's bit for bit and only the fp64 summation order is ours.
// The size of a state is known to the host alone (a size cannot be read from device memory without a synchronisation): ptta_score_reset
// records (pointer, bytes) in a small table, and the later calls look the pointer up.
#include <stdint.h>

#include <cmath>
#include <mutex>
#include <unordered_map>

#include "ptta_common.h"
#include "ptta_kernels.h"
#include "../../include/ptta.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int MAX_BLOCKS = 64;                  // partials per sample: one per lane of the finalizing wave
constexpr int UNITS_PER_BLOCK = 4 * THREADS;    // before a workgroup is added
constexpr int64_t HEADER = 128, SAMPLE_BYTES = 48, PARTIAL_BYTES = 48;
constexpr int64_t PER_SAMPLE = SAMPLE_BYTES + MAX_BLOCKS * PARTIAL_BYTES;

struct Sums { double cnt, ad, dd, ai, ii; };

// the state's header (include/ptta.h): 128 bytes
struct Header {
    double sum[4];
    long long frames, batches, empty_batches, pixels;
    double last[5];
    double pad[3];
};
static_assert(sizeof(Header) == HEADER, "score state header");

struct ScoreArgs {
    const float* depth;
    const float* gt;
    int n, H, W, wy, wx, wh, ww, rule, nblocks;
    float lo, hi;
    double* sample;          // state + HEADER: n x 6
    double* partial;         // behind the max_n sample rows: n x MAX_BLOCKS x 6
    Header* head;
    float* batch_out;
    float* sample_out;
    int32_t* count_out;
};

__device__ __forceinline__ void add_pixel(Sums& a, float out, float gt, float lo, float hi, int rule) {
    const bool in = rule == PTTA_SCORE_RULE_ADAPT ? (gt > 0.0f && !(gt < lo) && !(gt > hi)) : (gt > 0.0f && gt > lo && gt < hi);
    if (!in) return;
    const float d = 1000.0f * gt - 1000.0f * out;
    const float i = 1.0f / (0.001f * gt + 1e-9f) - 1.0f / (0.001f * out + 1e-9f);
    const float d2 = d * d, i2 = i * i;
    a.cnt += 1.0; a.ad += (double)fabsf(d); a.dd += (double)d2; a.ai += (double)fabsf(i); a.ii += (double)i2;
}

__device__ __forceinline__ double shfl_xor_f64(double v, int m) {
    const long long b = __double_as_longlong(v);
    const int lo = __shfl_xor((int)(b & 0xffffffffll), m, 64), hi = __shfl_xor((int)(b >> 32), m, 64);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// every lane ends with the sum of the 64 lanes, added in the butterfly's fixed order
__device__ __forceinline__ void wave_sum(Sums& a) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        a.cnt += shfl_xor_f64(a.cnt, m); a.ad += shfl_xor_f64(a.ad, m); a.dd += shfl_xor_f64(a.dd, m);
        a.ai += shfl_xor_f64(a.ai, m); a.ii += shfl_xor_f64(a.ii, m);
    }
}
__device__ __forceinline__ void put(double* p, const Sums& a) { p[0] = a.cnt; p[1] = a.ad; p[2] = a.dd; p[3] = a.ai; p[4] = a.ii; p[5] = 0.0; }

// grid: x = nblocks, y = n
template <bool VEC>
__global__ __launch_bounds__(THREADS) void score_partial_kernel(const ScoreArgs a) {
    __shared__ double red[WAVES][5];
    const int s = blockIdx.y;
    const long uw = VEC ? a.ww / 4 : a.ww, units = (long)a.wh * uw;      // units per window row, per sample
    const size_t base = ((size_t)s * a.H + a.wy) * a.W + a.wx;           // the window's first pixel in sample s
    Sums acc = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (long u = (long)blockIdx.x * THREADS + threadIdx.x; u < units; u += (long)a.nblocks * THREADS) {
        const long row = u / uw, col = u - row * uw;
        const size_t at = base + (size_t)row * a.W + (size_t)col * (VEC ? 4 : 1);
        if (VEC) {
            const float4 o = *(const float4*)(a.depth + at), g = *(const float4*)(a.gt + at);
            add_pixel(acc, o.x, g.x, a.lo, a.hi, a.rule); add_pixel(acc, o.y, g.y, a.lo, a.hi, a.rule);
            add_pixel(acc, o.z, g.z, a.lo, a.hi, a.rule); add_pixel(acc, o.w, g.w, a.lo, a.hi, a.rule);
        } else {
            add_pixel(acc, a.depth[at], a.gt[at], a.lo, a.hi, a.rule);
        }
    }
    wave_sum(acc);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave][0] = acc.cnt; red[wave][1] = acc.ad; red[wave][2] = acc.dd; red[wave][3] = acc.ai; red[wave][4] = acc.ii; }
    __syncthreads();
    if (threadIdx.x == 0) {
        Sums t = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int w = 0; w < WAVES; ++w) { t.cnt += red[w][0]; t.ad += red[w][1]; t.dd += red[w][2]; t.ai += red[w][3]; t.ii += red[w][4]; }
        put(a.partial + ((size_t)s * MAX_BLOCKS + blockIdx.x) * 6, t);
    }
}

// MAE, RMSE, iMAE, iRMSE of one set of sums; 0 / 0 = NaN for an empty mask
__device__ __forceinline__ void metrics(const Sums& t, double (&m)[4]) {
    m[0] = t.ad / t.cnt; m[1] = sqrt(t.dd / t.cnt); m[2] = t.ai / t.cnt; m[3] = sqrt(t.ii / t.cnt);
}

__global__ __launch_bounds__(THREADS) void score_final_kernel(const ScoreArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int s = wave; s < a.n; s += WAVES) {                            // wave-uniform
        Sums t = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (lane < a.nblocks) {
            const double* p = a.partial + ((size_t)s * MAX_BLOCKS + lane) * 6;
            t.cnt = p[0]; t.ad = p[1]; t.dd = p[2]; t.ai = p[3]; t.ii = p[4];
        }
        wave_sum(t);
        if (lane == 0) {
            put(a.sample + (size_t)s * 6, t);
            if (a.sample_out) {
                double m[4];
                metrics(t, m);
                for (int k = 0; k < 4; ++k) a.sample_out[(size_t)s * 4 + k] = (float)m[k];
            }
            if (a.count_out) a.count_out[s] = (int32_t)t.cnt;
        }
    }
    __syncthreads();                                                     // the sample rows above are read by thread 0 below
    if (threadIdx.x != 0) return;
    Sums t = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < a.n; ++s) {
        const double* p = a.sample + (size_t)s * 6;
        t.cnt += p[0]; t.ad += p[1]; t.dd += p[2]; t.ai += p[3]; t.ii += p[4];
    }
    double m[4];
    metrics(t, m);
    Header* h = a.head;
    for (int k = 0; k < 4; ++k) {
        h->sum[k] += m[k] * (double)a.n;
        if (a.batch_out) a.batch_out[k] = (float)m[k];
    }
    h->frames += a.n; h->batches += 1; h->pixels += (long long)t.cnt; h->empty_batches += t.cnt == 0.0 ? 1 : 0;
    h->last[0] = t.cnt; h->last[1] = t.ad; h->last[2] = t.dd; h->last[3] = t.ai; h->last[4] = t.ii;
}

__global__ void score_result_kernel(const Header* h, long long n_sample, double* out8) {
    const double div = n_sample > 0 ? (double)n_sample : (double)h->frames;
    for (int k = 0; k < 4; ++k) out8[k] = h->sum[k] / div;
    out8[4] = (double)h->frames; out8[5] = (double)h->batches; out8[6] = (double)h->empty_batches; out8[7] = (double)h->pixels;
}

int64_t state_bytes(int max_n) { return HEADER + PER_SAMPLE * (int64_t)max_n; }

// states handed to ptta_score_reset: pointer -> max_n.  An entry is replaced when the address is reset again.
std::mutex g_lock;
std::unordered_map<const void*, int> g_states;

int known_max_n(const void* state) {
    std::lock_guard<std::mutex> hold(g_lock);
    const auto it = g_states.find(state);
    return it == g_states.end() ? 0 : it->second;
}

}  // namespace

extern "C" int64_t ptta_score_state_bytes(int max_n) {
    if (max_n < 1 || max_n > PTTA_SCORE_MAX_N) return ptta_refuse_args("ptta_score_state_bytes: max_n outside 1 .. PTTA_SCORE_MAX_N");
    return state_bytes(max_n);
}

extern "C" int ptta_score_reset(void* state, int64_t bytes, ptta_stream stream) {
    if (!state) return ptta_refuse_args("ptta_score_reset: NULL state");
    if ((uintptr_t)state & 15u) return ptta_refuse_args("ptta_score_reset: the state is not 16-byte aligned");
    if (bytes < state_bytes(1)) return ptta_refuse_args("ptta_score_reset: state_bytes is below ptta_score_state_bytes(1)");
    int64_t max_n = (bytes - HEADER) / PER_SAMPLE;
    if (max_n > PTTA_SCORE_MAX_N) max_n = PTTA_SCORE_MAX_N;
    if (hipMemsetAsync(state, 0, HEADER, (hipStream_t)stream) != hipSuccess) return -5;
    std::lock_guard<std::mutex> hold(g_lock);
    g_states[state] = (int)max_n;
    return 0;
}

extern "C" int ptta_score_accumulate(const ptta_score_args* a, ptta_stream stream) {
    if (!a) return ptta_refuse_args("ptta_score_accumulate: NULL args");
    if (!a->depth || !a->ground_truth) return ptta_refuse_args("ptta_score_accumulate: NULL depth or ground_truth");
    if (!a->state) return ptta_refuse_args("ptta_score_accumulate: NULL state");
    if ((uintptr_t)a->state & 15u) return ptta_refuse_args("ptta_score_accumulate: the state is not 16-byte aligned");
    if (((uintptr_t)a->depth | (uintptr_t)a->ground_truth) & 3u) return ptta_refuse_args("ptta_score_accumulate: a map is not 4-byte aligned");
    if (a->n < 1 || a->height < 1 || a->width < 1) return ptta_refuse_args("ptta_score_accumulate: n, height or width below 1");
    if (a->win_height < 1 || a->win_width < 1) return ptta_refuse_args("ptta_score_accumulate: empty window");
    if (a->win_y < 0 || a->win_x < 0 || (int64_t)a->win_y + a->win_height > a->height || (int64_t)a->win_x + a->win_width > a->width)
        return ptta_refuse_args("ptta_score_accumulate: the window leaves the sample");
    if (!std::isfinite(a->min_evaluate_depth) || !std::isfinite(a->max_evaluate_depth)) return ptta_refuse_args("ptta_score_accumulate: a bound is not finite");
    if (a->min_evaluate_depth > a->max_evaluate_depth) return ptta_refuse_args("ptta_score_accumulate: min_evaluate_depth > max_evaluate_depth");
    if (a->rule != PTTA_SCORE_RULE_ADAPT && a->rule != PTTA_SCORE_RULE_VALIDATE) return ptta_refuse_args("ptta_score_accumulate: unknown rule");
    const int max_n = known_max_n(a->state);
    if (max_n < 1) return ptta_refuse_args("ptta_score_accumulate: the state was not handed to ptta_score_reset");
    if (a->n > max_n) return ptta_refuse_args("ptta_score_accumulate: n is above the max_n the state was sized for");
    const bool vec = a->width % 4 == 0 && a->win_x % 4 == 0 && a->win_width % 4 == 0 && (((uintptr_t)a->depth | (uintptr_t)a->ground_truth) & 15u) == 0;
    const int64_t units = (int64_t)a->win_height * (vec ? a->win_width / 4 : a->win_width);
    const int64_t want = (units + UNITS_PER_BLOCK - 1) / UNITS_PER_BLOCK;
    ScoreArgs k = {};
    k.depth = a->depth; k.gt = a->ground_truth;
    k.n = a->n; k.H = a->height; k.W = a->width; k.wy = a->win_y; k.wx = a->win_x; k.wh = a->win_height; k.ww = a->win_width;
    k.rule = a->rule; k.nblocks = (int)(want > MAX_BLOCKS ? MAX_BLOCKS : want);
    k.lo = a->min_evaluate_depth; k.hi = a->max_evaluate_depth;
    k.head = (Header*)a->state;
    k.sample = (double*)((char*)a->state + HEADER);
    k.partial = (double*)((char*)a->state + HEADER + SAMPLE_BYTES * (int64_t)max_n);
    k.batch_out = a->batch_out; k.sample_out = a->sample_out; k.count_out = a->sample_count_out;
    const dim3 grid((unsigned)k.nblocks, (unsigned)a->n);
    if (vec) hipLaunchKernelGGL(score_partial_kernel<true>, grid, dim3(THREADS), 0, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(score_partial_kernel<false>, grid, dim3(THREADS), 0, (hipStream_t)stream, k);
    hipLaunchKernelGGL(score_final_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, k);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int ptta_score_result(const void* state, int64_t n_sample, double* out8, ptta_stream stream) {
    if (!state || !out8) return ptta_refuse_args("ptta_score_result: NULL state or output");
    if (((uintptr_t)state & 15u) || ((uintptr_t)out8 & 7u)) return ptta_refuse_args("ptta_score_result: misaligned state or output");
    if (known_max_n(state) < 1) return ptta_refuse_args("ptta_score_result: the state was not handed to ptta_score_reset");
    hipLaunchKernelGGL(score_result_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (const Header*)state, (long long)n_sample, out8);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
