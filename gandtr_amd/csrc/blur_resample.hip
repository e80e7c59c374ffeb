// The anti-aliased sampling layers of ResnetGenerator(no_antialias=False / no_antialias_up=False) on the graph's NHWC tensors (gdt_net_blur_resample):
//   blur_down   Downsample(C): ReflectionPad2d(1) + depthwise 3x3 conv, stride 2, weights outer([1,2,1],[1,2,1]) / 16          -> ceil(H/2) x ceil(W/2)
//   blur_up     Upsample(C): replicate pad + depthwise transposed 4x4 conv, stride 2 + crop = bilinear x 2 (align_corners=False)  -> 2H x 2W
// One lane handles one 8-channel vector (16-byte accesses in fp16, two in fp32), fp32 arithmetic, ONE store in the tensor's type.  Both are memory-bound and
// separable, and both keep the vertical reuse in registers: a lane owns one output column (down) / one input column (up) and walks ROWS rows of it, carrying the
// horizontally filtered rows it needs again.  Down: output row oy reads the input rows 2 oy - 1, 2 oy, 2 oy + 1 and the last of them is the next output row's
// first, so a step loads two rows (6 vectors) instead of three (9).  Up: the outputs 2 iy and 2 iy + 1 read the rows iy - 1, iy, iy + 1, a window that slides by
// one row per step (3 vectors for four stores).  The horizontal reuse -- neighbouring lanes read the same pixels -- is served by the CU's vector L1: the lanes of
// a workgroup cover a contiguous stripe of one row.  What HBM sees is the output once and the input once, plus the rows read again at the chunk seams: one in
// 2 ROWS_DOWN, two in ROWS_UP (the up kernel's input is a fifth of its traffic).
// NORM: the producer's InstanceNorm folded in -- (x - mean) * rstd, then the ReLU, in fp32 on every tap as it is read (the formula of in_apply_kernel, so that
// the result is the one the unfolded graph computes from the fp32 tensor that pass would have stored).
// The down weights are dyadic: every product is exact and only the eight additions round.  The up weights are not (0.75 x needs one more bit): each axis is ONE
// explicit fma(0.75, a, 0.25 b), the same instruction in every form of the kernel.
#include "aux_kernels.h"

namespace {

constexpr int ROWS_DOWN = 8, ROWS_UP = 8;       // output rows (down) / input rows (up) one lane walks

// one tap: the stored vector, normalised (+ ReLU) when the producer's InstanceNorm is folded in
template <typename T, bool NORM>
__device__ __forceinline__ void tap8(const T* p, const float (&m)[8], const float (&r)[8], int relu, float (&v)[8]) {
    load8(p, v);
    if (NORM) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float f = (v[e] - m[e]) * r[e];
            v[e] = relu ? fmaxf(f, 0.f) : f;
        }
    }
}
__device__ __forceinline__ void load_norm(const float* mean_rstd, long nc, float (&m)[8], float (&r)[8]) {
    const float4* q = (const float4*)(mean_rstd + nc * 2);       // [N][C][2], 8 channels = 64 contiguous bytes
#pragma unroll
    for (int k = 0; k < 4; ++k) { const float4 t = q[k]; m[2 * k] = t.x; r[2 * k] = t.y; m[2 * k + 1] = t.z; r[2 * k + 1] = t.w; }
}

// work item -> (channel vector, column, row chunk, image); false past the end
__device__ __forceinline__ bool item_of(long i, long total, int c8n, int cols, int chunks, int& c8, int& col, int& chunk, int& n) {
    if (i >= total) return false;
    c8 = (int)(i % c8n); i /= c8n;
    col = (int)(i % cols); i /= cols;
    chunk = (int)(i % chunks); n = (int)(i / chunks);
    return true;
}

// ---- down: h(row)[ox] = x[row][r(2 ox - 1)] + 2 x[row][2 ox] + x[row][r(2 ox + 1)];  y[oy][ox] = (h(r(2 oy - 1)) + 2 h(2 oy) + h(r(2 oy + 1))) / 16
template <typename T, bool NORM>
__global__ __launch_bounds__(256) void blur_down_kernel(const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ mean_rstd, int relu,
                                                        int H, int W, int C, int OH, int OW, int chunks, long total) {
    int c8, ox, chunk, n;
    if (!item_of((long)blockIdx.x * 256 + threadIdx.x, total, C >> 3, OW, chunks, c8, ox, chunk, n)) return;
    float m[8], r[8];
    if (NORM) load_norm(mean_rstd, (long)n * C + c8 * 8, m, r);
    // reflection without the edge pixel; W >= 2 keeps both inside
    const int xc = 2 * ox, xl = xc == 0 ? 1 : xc - 1, xr = xc + 1 >= W ? 2 * W - 3 - xc : xc + 1;
    const T* img = x + (long)n * H * W * C + c8 * 8;
    auto hrow = [&](int row, float (&h)[8]) {
        const T* p = img + (long)row * W * C;
        float a[8], b[8], c[8];
        tap8<T, NORM>(p + (long)xl * C, m, r, relu, a);
        tap8<T, NORM>(p + (long)xc * C, m, r, relu, b);
        tap8<T, NORM>(p + (long)xr * C, m, r, relu, c);
#pragma unroll
        for (int e = 0; e < 8; ++e) h[e] = (a[e] + 2.f * b[e]) + c[e];
    };
    const int oy0 = chunk * ROWS_DOWN, oy1 = min(OH, oy0 + ROWS_DOWN);
    float hp[8];
    hrow(oy0 == 0 ? 1 : 2 * oy0 - 1, hp);
    T* out = y + (((long)n * OH + oy0) * OW + ox) * C + c8 * 8;
    for (int oy = oy0; oy < oy1; ++oy, out += (long)OW * C) {
        const int yc = 2 * oy, yn = yc + 1 >= H ? 2 * H - 3 - yc : yc + 1;
        float h0[8], h1[8], v[8];
        hrow(yc, h0);
        hrow(yn, h1);
#pragma unroll
        for (int e = 0; e < 8; ++e) { v[e] = ((hp[e] + 2.f * h0[e]) + h1[e]) * 0.0625f; hp[e] = h1[e]; }
        store8(out, v);
    }
}

// ---- up: per axis out[2 i] = 0.75 in[i] + 0.25 in[max(i - 1, 0)], out[2 i + 1] = 0.75 in[i] + 0.25 in[min(i + 1, last)]
__device__ __forceinline__ float lerp34(float a, float b) { return __fmaf_rn(0.75f, a, 0.25f * b); }

template <typename T, bool NORM>
__global__ __launch_bounds__(256) void blur_up_kernel(const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ mean_rstd, int relu,
                                                      int H, int W, int C, int chunks, long total) {
    int c8, ix, chunk, n;
    if (!item_of((long)blockIdx.x * 256 + threadIdx.x, total, C >> 3, W, chunks, c8, ix, chunk, n)) return;
    float m[8], r[8];
    if (NORM) load_norm(mean_rstd, (long)n * C + c8 * 8, m, r);
    const int xl = max(ix - 1, 0), xr = min(ix + 1, W - 1);
    const T* img = x + (long)n * H * W * C + c8 * 8;
    // the two output columns of one input row: hl = column 2 ix, hr = column 2 ix + 1
    auto hrow = [&](int row, float (&hl)[8], float (&hr)[8]) {
        const T* p = img + (long)row * W * C;
        float a[8], b[8], c[8];
        tap8<T, NORM>(p + (long)xl * C, m, r, relu, a);
        tap8<T, NORM>(p + (long)ix * C, m, r, relu, b);
        tap8<T, NORM>(p + (long)xr * C, m, r, relu, c);
#pragma unroll
        for (int e = 0; e < 8; ++e) { hl[e] = lerp34(b[e], a[e]); hr[e] = lerp34(b[e], c[e]); }
    };
    const int iy0 = chunk * ROWS_UP, iy1 = min(H, iy0 + ROWS_UP);
    const long orow = (long)2 * W * C;
    float pl[8], pr[8], cl[8], cr[8], nl[8], nr[8], v[8];
    hrow(max(iy0 - 1, 0), pl, pr);
    hrow(iy0, cl, cr);
    T* out = y + (((long)n * 2 * H + 2 * iy0) * 2 * W + 2 * ix) * C + c8 * 8;
    for (int iy = iy0; iy < iy1; ++iy, out += 2 * orow) {
        hrow(min(iy + 1, H - 1), nl, nr);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = lerp34(cl[e], pl[e]);
        store8(out, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = lerp34(cr[e], pr[e]);
        store8(out + C, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = lerp34(cl[e], nl[e]);
        store8(out + orow, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = lerp34(cr[e], nr[e]);
        store8(out + orow + C, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) { pl[e] = cl[e]; pr[e] = cr[e]; cl[e] = nl[e]; cr[e] = nr[e]; }
    }
}

// form of a launch: element type x (plain | norm-folded)
#define BLUR_LAUNCH(kernel, f32, norm, grid, st, ...)                                                                                  \
    do {                                                                                                                               \
        if (f32) { if (norm) hipLaunchKernelGGL((kernel<float, true>), grid, dim3(256), 0, st, (const float*)x, (float*)y, __VA_ARGS__);   \
                   else hipLaunchKernelGGL((kernel<float, false>), grid, dim3(256), 0, st, (const float*)x, (float*)y, __VA_ARGS__); }     \
        else { if (norm) hipLaunchKernelGGL((kernel<f16, true>), grid, dim3(256), 0, st, (const f16*)x, (f16*)y, __VA_ARGS__);             \
               else hipLaunchKernelGGL((kernel<f16, false>), grid, dim3(256), 0, st, (const f16*)x, (f16*)y, __VA_ARGS__); }               \
    } while (0)

}  // namespace

int gdt_k_blur_down(const void* x, void* y, int f32, int N, int H, int W, int C, const float* mean_rstd, int relu, hipStream_t st) {
    GDT_REQUIRE(x && y && C >= 8 && C % 8 == 0 && N >= 1, "blur_down needs C % 8 == 0 and a batch");
    GDT_REQUIRE(H >= 2 && W >= 2, "the anti-aliased Downsample needs a map of at least 2 x 2 (reflection padding)");
    GDT_REQUIRE(gdt_offsets_fit(N, H, W, C), "blur_down: N * H * W * C must stay below 2^32");
    const int OH = (H + 1) / 2, OW = (W + 1) / 2, chunks = (OH + ROWS_DOWN - 1) / ROWS_DOWN;
    const long total = (long)N * chunks * OW * (C / 8), blocks = (total + 255) / 256;
    GDT_REQUIRE(blocks < (1L << 31), "blur_down: grid too large");
    BLUR_LAUNCH(blur_down_kernel, f32, mean_rstd != nullptr, dim3((unsigned)blocks), st, mean_rstd, relu, H, W, C, OH, OW, chunks, total);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

int gdt_k_blur_up(const void* x, void* y, int f32, int N, int H, int W, int C, const float* mean_rstd, int relu, hipStream_t st) {
    GDT_REQUIRE(x && y && C >= 8 && C % 8 == 0 && N >= 1 && H >= 1 && W >= 1, "blur_up needs C % 8 == 0 and a non-empty map");
    GDT_REQUIRE(H < (1 << 30) && W < (1 << 30) && gdt_offsets_fit(N, 2 * H, 2 * W, C), "blur_up: N * 2H * 2W * C must stay below 2^32");
    const int chunks = (H + ROWS_UP - 1) / ROWS_UP;
    const long total = (long)N * chunks * W * (C / 8), blocks = (total + 255) / 256;
    GDT_REQUIRE(blocks < (1L << 31), "blur_up: grid too large");
    BLUR_LAUNCH(blur_up_kernel, f32, mean_rstd != nullptr, dim3((unsigned)blocks), st, mean_rstd, relu, H, W, C, chunks, total);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}
