// The ten small utility kernels of the MSG_CHN path (copies, stamps, transposition, dual-corner padding and its inverse,
// width conversion, the merged-head weight product) and the host functions the other translation units launch them through.
#include "msgchn_ctx.h"

using namespace msgchn;

namespace {

// device-to-device copies of the step (the next frame into the handle's staging buffers, the depth map and the four loss scalars out): a
// kernel on the step's stream instead of hipMemcpyAsync -- the runtime's copy carries system-scope fences (what the host may read), these
// are read by later work of the same device
static __global__ void d2d_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, long n4, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) ((float4*)dst)[i] = ((const float4*)src)[i];
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) dst[4 * n4 + threadIdx.x] = src[4 * n4 + threadIdx.x];
}
// Diagnostic (option "stamps", tools/step_stamps.py): wall-clock stamps written by one-thread nodes of the step's graph (ticks since
// stamp 0) -- where a replayed step's branches start and end WITHOUT a profiler attached (rocprofv3 slows the host enough to reorder them)
static __global__ void stamp_kernel(float* out, unsigned long long* base, int i) {
    const unsigned long long t = wall_clock64();
    if (i == 0) { *base = t; out[0] = 0.f; } else out[i] = (float)(long long)(t - *base);
}
__global__ void transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)rows * cols) return;
    const int r = (int)(idx / cols), cc = (int)(idx % cols);
    dst[(long)cc * rows + r] = src[idx];
}
// dual-corner zero padding (src/msg_chn_model_adapt.py:75-103): item k=0 pads top/right, k=1 bottom/left
__global__ void pad_dual_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int C, int H, int W,
                                int Hp, int Wp, int pt, int pr, ImgNorm nm = ImgNorm{0, 1.f, {0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}}) {
    const long total = (long)2 * N * C * Hp * Wp;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % Wp); long t_ = idx / Wp;
        const int y = (int)(t_ % Hp); t_ /= Hp;
        const int ch = (int)(t_ % C); t_ /= C;
        const int n = (int)(t_ % N); const int k = (int)(t_ / N);
        const int sy = k == 0 ? y - pt : y, sx = k == 0 ? x : x - pr;
        float v = 0.f;
        if (sy >= 0 && sy < H && sx >= 0 && sx < W) {
            v = src[(((long)n * C + ch) * H + sy) * W + sx];
            if (nm.on) v = (v / nm.div - nm.mean[ch]) / nm.stdv[ch];     // the reference normalises before it pads
        }
        dst[idx] = v;
    }
}
// crop both paddings and average (src/msg_chn_model_adapt.py:107-123)
__global__ void crop_avg_kernel(const float* __restrict__ net, float* __restrict__ out, int N, int H, int W, int Hp, int Wp,
                                int pt, int pr) {
    const long total = (long)N * H * W;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % W); long t_ = idx / W;
        const int y = (int)(t_ % H); const int n = (int)(t_ / H);
        const float a = net[((long)n * Hp + y + pt) * Wp + x];
        const float b = net[((long)(N + n) * Hp + y) * Wp + x + pr];
        out[idx] = (a + b) / 2.0f;
    }
}
__global__ void scatter_dual_grad_kernel(const float* __restrict__ g, float* __restrict__ gnet, int N, int H, int W, int Hp,
                                         int Wp, int pt, int pr) {
    const long total = (long)2 * N * Hp * Wp;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % Wp); long t_ = idx / Wp;
        const int y = (int)(t_ % Hp); t_ /= Hp;
        const int n = (int)(t_ % N); const int k = (int)(t_ / N);
        const int sy = k == 0 ? y - pt : y, sx = k == 0 ? x : x - pr;
        float v = 0.f;
        if (sy >= 0 && sy < H && sx >= 0 && sx < W) v = 0.5f * g[((long)n * H + sy) * W + sx];
        gnet[idx] = v;
    }
}
__global__ void validity_kernel(const float* __restrict__ sparse, float* __restrict__ v, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float s = sparse[i];
        v[i] = s > 0.f ? 1.f : s;              // torch.where(sd > 0, 1, sd), src/tta_main.py:583-586
    }
}

template <typename T>
__global__ void to_f32_kernel(const T* __restrict__ src, float* __restrict__ dst, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) dst[i] = ld(src + i);
}
template <typename T>
__global__ void from_f32_kernel(const float* __restrict__ src, T* __restrict__ dst, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) st(dst + i, src[i]);
}
inline int nblk(long n, int cap = 4096) { long b = (n + 255) / 256; return (int)(b > cap ? cap : (b < 1 ? 1 : b)); }

__global__ void fuse_linear_kernel(const float* __restrict__ Wb, const float* __restrict__ bb, const float* __restrict__ Wa, const float* __restrict__ ba,
                                   float* __restrict__ W, float* __restrict__ bias, int N, int M, int K) {
    // y = (x Wa^T + ba) Wb^T + bb = x (Wb Wa)^T + (Wb ba + bb);  Wb: [N][M], Wa: [M][K] -> W: [N][K]
    const int k = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y;
    if (k >= K) return;
    double acc = 0.0;
    for (int m = 0; m < M; ++m) acc += (double)Wb[(long)n * M + m] * (double)Wa[(long)m * K + k];
    W[(long)n * K + k] = (float)acc;
    if (k == 0) {
        double b = (double)bb[n];
        for (int m = 0; m < M; ++m) b += (double)Wb[(long)n * M + m] * (double)ba[m];
        bias[n] = (float)b;
    }
}

}  // namespace

namespace msgchn {

hipError_t d2d_copy(void* dst, const void* src, size_t bytes, hipStream_t s) {
    if ((bytes & 3) || (((uintptr_t)dst | (uintptr_t)src) & 15)) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s);
    const long n = (long)(bytes / 4), n4 = n / 4;
    long blocks = (n4 + 255) / 256; if (blocks < 1) blocks = 1; if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(d2d_copy_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const float*)src, (float*)dst, n4, n);
    return hipGetLastError();
}
void stamp_launch(float* out, unsigned long long* base, int i, hipStream_t s) { hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(1), 0, s, out, base, i); }
void transpose_launch(const float* src, float* dst, int rows, int cols, hipStream_t s) {
    hipLaunchKernelGGL(transpose_kernel, dim3(nblk((long)rows * cols)), dim3(256), 0, s, src, dst, rows, cols);
}
// (the three dual-corner kernels: one thread per element of the larger side, grid capped by nblk)
void pad_dual_launch(const float* src, float* dst, int N, int C, int H, int W, int Hp, int Wp, int pt, int pr, hipStream_t s, ImgNorm nm) {
    hipLaunchKernelGGL(pad_dual_kernel, dim3(nblk((long)2 * N * C * Hp * Wp)), dim3(256), 0, s, src, dst, N, C, H, W, Hp, Wp, pt, pr, nm);
}
void crop_avg_launch(const float* net, float* out, int N, int H, int W, int Hp, int Wp, int pt, int pr, hipStream_t s) {
    hipLaunchKernelGGL(crop_avg_kernel, dim3(nblk((long)N * H * W)), dim3(256), 0, s, net, out, N, H, W, Hp, Wp, pt, pr);
}
void scatter_dual_grad_launch(const float* g, float* gnet, int N, int H, int W, int Hp, int Wp, int pt, int pr, hipStream_t s) {
    hipLaunchKernelGGL(scatter_dual_grad_kernel, dim3(nblk((long)2 * N * Hp * Wp)), dim3(256), 0, s, g, gnet, N, H, W, Hp, Wp, pt, pr);
}
void to_f32_launch(const bf16_t* src, float* dst, long n, hipStream_t s) {
    hipLaunchKernelGGL((to_f32_kernel<bf16_t>), dim3(nblk(n)), dim3(256), 0, s, src, dst, n);
}
void from_f32_launch(const float* src, bf16_t* dst, long n, hipStream_t s) {
    hipLaunchKernelGGL((from_f32_kernel<bf16_t>), dim3(nblk(n)), dim3(256), 0, s, src, dst, n);
}
void fuse_linear_launch(const float* Wb, const float* bb, const float* Wa, const float* ba, float* W, float* bias, int N, int M, int K, hipStream_t s) {
    hipLaunchKernelGGL(fuse_linear_kernel, dim3((K + 255) / 256, N), dim3(256), 0, s, Wb, bb, Wa, ba, W, bias, N, M, K);
}
}  // namespace msgchn
