// Patch scores of a PatchGAN discriminator (gfx950, MI355X): per logit map the mean logit and the mean adversarial term against target 0 and against
// target 1 -- what DiscriminatorLoss (compound_losses.py:33-50) evaluates with torch's MSELoss / BCEWithLogitsLoss over torch.full(shape, target) --
// and the same three means over the batch.  The maps are a few thousand values: the terms are evaluated and added in double, every lane sums a fixed
// strided subset, the lanes are merged by a fixed tree, the images in index order.  No atomics; bit-identical from run to run.
#include "gdt_common.h"

namespace {

constexpr int PS_THREADS = 256;

__device__ __forceinline__ double ps_term(double x, double t, int kind) {
    if (kind == 0) return (x - t) * (x - t);
    return fmax(x, 0.0) - x * t + log1p(exp(-fabs(x)));          // torch's stable form of -[t log s(x) + (1 - t) log(1 - s(x))]
}

// grid n: per_image[img][0..2] = (mean logit, mean term vs 0, mean term vs 1) of map img
__global__ __launch_bounds__(PS_THREADS) void patch_score_kernel(const float* __restrict__ logits, int hw, int kind, double* __restrict__ per_image) {
    __shared__ double red[3][PS_THREADS];
    const int img = blockIdx.x, tid = threadIdx.x;
    const float* x = logits + (long)img * hw;
    double s = 0.0, l0 = 0.0, l1 = 0.0;
    for (int i = tid; i < hw; i += PS_THREADS) {
        const double v = (double)x[i];
        s += v; l0 += ps_term(v, 0.0, kind); l1 += ps_term(v, 1.0, kind);
    }
    red[0][tid] = s; red[1][tid] = l0; red[2][tid] = l1;
    __syncthreads();
    for (int step = PS_THREADS / 2; step > 0; step >>= 1) {
        if (tid < step) {
#pragma unroll
            for (int k = 0; k < 3; ++k) red[k][tid] += red[k][tid + step];
        }
        __syncthreads();
    }
    if (tid < 3) per_image[(long)img * 3 + tid] = red[tid][0] / (double)hw;
}

// one workgroup: total[k] = mean over the images of per_image[.][k] (all maps have hw values), added in index order
__global__ __launch_bounds__(64) void patch_score_total_kernel(const double* __restrict__ per_image, int n, double* __restrict__ total) {
    const int k = threadIdx.x;
    if (k >= 3) return;
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += per_image[(long)i * 3 + k];
    total[k] = s / (double)n;
}

}  // namespace

extern "C" int gdt_patch_score(const float* logits, int n, int hw, int kind, double* per_image, double* total, void* stream) {
    GDT_REQUIRE(logits && per_image && total, "gdt_patch_score: null buffer");
    GDT_REQUIRE(n >= 1 && hw >= 1 && (long)n * hw < (1L << 31), "gdt_patch_score: n >= 1 maps of hw >= 1 values");
    GDT_REQUIRE(kind == 0 || kind == 1, "gdt_patch_score: kind 0 mse, 1 bce_with_logits");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(patch_score_kernel, dim3(n), dim3(PS_THREADS), 0, st, logits, hw, kind, per_image);
    GDT_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(patch_score_total_kernel, dim3(1), dim3(64), 0, st, (const double*)per_image, n, total);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}
