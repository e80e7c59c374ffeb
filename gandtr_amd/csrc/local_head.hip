// The local head: the descriptor at every position of the trunk's map, in the reference's layout, and its L2-norm attention (extract_ssl,
// imageretrievalnet.py:426-427: net.norm(net.features(x)).view(D, -1); L2NormAttention, layers/attention.py:10-15).
//
//   desc[n][c][p] = x[n][p][c] / (sqrt(sum_c x^2) + eps)            fp32 [N][D][H W]
//   att[n][p]     = sqrt(sum_c x^2 + 1e-10)                          fp32 [N][H W], divided by the image's maximum when normalize_max
//
// local_desc_kernel<T>: one workgroup per (slab of TP consecutive positions, image).  The map is NHWC, so a slab is one contiguous piece of memory: it is
// read ONCE, with 16-byte loads, into LDS ([position][D], row pitch D + 4 bytes: the transposed read below then meets every bank once).  A wave sums
// the squares of a position as pixel_norm_kernel does (a lane the 16-byte pieces lane, lane + 64, .. ascending, fmaf, the xor butterfly: an order
// fixed by D alone, and the same bits as gdt_pixel_attention).  Then the slab is written out transposed: consecutive threads take consecutive
// positions of one channel, so a wave stores whole runs of TP floats.  TP = 32 where the slab fits 64 KB, else 16 (up to 128 KB), 8 or 4.
// With normalize_max the workgroup's largest attention goes to partial[n][slab] (a maximum is exact in any order; no atomics) and
// local_scale_kernel divides.
#include <algorithm>

#include "../../include/gandtr_hip.h"
#include "aux_kernels.h"
#include "gdt_common.h"

namespace {

constexpr int LH_THREADS = 256;
constexpr int LH_LDS_MAX = 128 * 1024 + 32 * 4 + 2 * 32 * 4 + 16;

inline int lh_positions(int D, int f32) {
    const size_t row = (size_t)D * (f32 ? 4 : 2);
    if (32 * row <= 64 * 1024) return 32;
    if (16 * row <= 128 * 1024) return 16;
    if (8 * row <= 128 * 1024) return 8;
    return 4;
}

template <typename T>
__global__ __launch_bounds__(LH_THREADS) void local_desc_kernel(const T* __restrict__ x, float* __restrict__ desc, float* __restrict__ att,
                                                                float* __restrict__ partial, long HW, int D, int TP, float eps, int maxp) {
    constexpr int E = 16 / sizeof(T);            // elements of a 16-byte piece
    extern __shared__ __attribute__((aligned(16))) char lh_smem[];
    const int pitch = D * (int)sizeof(T) + 4;    // bytes; a multiple of 4
    float* sden = (float*)(lh_smem + (size_t)TP * pitch);      // [TP]
    float* satt = sden + TP;                                   // [TP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.y, pieces = D / E;
    const long p0 = (long)blockIdx.x * TP;
    const int tp = (int)(HW - p0 < TP ? HW - p0 : TP);         // positions of this slab
    const T* src = x + ((size_t)n * HW + p0) * D;

    for (int i = tid; i < tp * pieces; i += LH_THREADS) {
        const int j = i / pieces, pc = i - j * pieces;
        const uint4 v = *(const uint4*)(src + (size_t)i * E);
        unsigned* dst = (unsigned*)(lh_smem + (size_t)j * pitch + (size_t)pc * 16);
        dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
    }
    __syncthreads();

    for (int j = wave; j < tp; j += LH_THREADS / 64) {
        float acc = 0.f;
        for (int pc = lane; pc < pieces; pc += 64) {
            const unsigned* w = (const unsigned*)(lh_smem + (size_t)j * pitch + (size_t)pc * 16);
            uint4 v; v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
            const T* t = (const T*)&v;
#pragma unroll
            for (int e = 0; e < E; ++e) { const float f = (float)t[e]; acc = fmaf(f, f, acc); }
        }
#pragma unroll
        for (int k = 32; k > 0; k >>= 1) acc += __shfl_xor(acc, k);
        if (lane == 0) { sden[j] = sqrtf(acc) + eps; satt[j] = sqrtf(acc + 1e-10f); }
    }
    __syncthreads();

    if (tid < tp) att[(size_t)n * HW + p0 + tid] = satt[tid];
    if (maxp && tid == 0) {
        float m = 0.f;
        for (int j = 0; j < tp; ++j) m = fmaxf(m, satt[j]);
        partial[(size_t)n * gridDim.x + blockIdx.x] = m;
    }
    // transposed write: thread -> (position j = tid % TP, channel tid / TP + k * (256 / TP)); TP is a power of two <= 32
    const int j = tid & (TP - 1), c0 = tid / TP, cstep = LH_THREADS / TP;
    if (j < tp) {
        const float den = sden[j];
        const T* row = (const T*)(lh_smem + (size_t)j * pitch);
        float* o = desc + (size_t)n * D * HW + p0 + j;
        for (int c = c0; c < D; c += cstep) o[(size_t)c * HW] = (float)row[c] / den;
    }
}

// a[n][p] /= max_g partial[n][g]: a division, as the reference's m / m.max(); grid (blocks over the positions, N)
__global__ __launch_bounds__(256) void local_scale_kernel(float* __restrict__ a, const float* __restrict__ partial, long HW, int G) {
    __shared__ float red[4];
    const int n = blockIdx.y;
    float m = 0.f;
    for (int g = threadIdx.x; g < G; g += 256) m = fmaxf(m, partial[(size_t)n * G + g]);
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) m = fmaxf(m, __shfl_xor(m, k));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    const float M = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float* an = a + (size_t)n * HW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long)gridDim.x * 256) an[i] = an[i] / M;
}

}  // namespace

size_t gdt_local_head_partial_floats(int N, long HW, int D, int f32) {
    const int TP = lh_positions(D, f32);
    return (size_t)N * ((HW + TP - 1) / TP);
}

int gdt_k_local_descriptors(const void* x, int f32, int N, long HW, int D, float eps, int normalize_max, float* desc, float* att, float* partial,
                            hipStream_t st) {
    GDT_REQUIRE(N >= 1 && N <= 65535 && HW >= 1 && D >= 64 && D % 64 == 0 && D <= 8192, "local descriptors need D % 64 == 0, D <= 8192 and at most 65535 images");
    GDT_REQUIRE((size_t)N * HW * D < ((size_t)1 << 40), "local descriptors: map too large");
    GDT_REQUIRE(!normalize_max || partial, "local descriptors: the maximum needs its workspace");
    GDT_REQUIRE(eps >= 0.f, "local descriptors: eps >= 0");
    const int TP = lh_positions(D, f32);
    const long G = (HW + TP - 1) / TP;
    GDT_REQUIRE(G < (1l << 31), "local descriptors: too many positions for one launch");
    const size_t lds = (size_t)TP * ((size_t)D * (f32 ? 4 : 2) + 4) + 2 * TP * sizeof(float);
    GDT_REQUIRE(lds <= (size_t)LH_LDS_MAX, "local descriptors: slab beyond the LDS budget");
    int unused = 0;
    if (f32) {
        GDT_CHECK((GdtKernel<local_desc_kernel<float>, LH_LDS_MAX>::figure(unused)));
        hipLaunchKernelGGL(local_desc_kernel<float>, dim3((unsigned)G, N), dim3(LH_THREADS), lds, st, (const float*)x, desc, att, partial, HW, D, TP, eps,
                           normalize_max);
    } else {
        GDT_CHECK((GdtKernel<local_desc_kernel<f16>, LH_LDS_MAX>::figure(unused)));
        hipLaunchKernelGGL(local_desc_kernel<f16>, dim3((unsigned)G, N), dim3(LH_THREADS), lds, st, (const f16*)x, desc, att, partial, HW, D, TP, eps,
                           normalize_max);
    }
    GDT_CHECK_HIP(hipGetLastError());
    if (!normalize_max) return GDT_OK;
    const int blocks = (int)std::min<long>((HW + 255) / 256, 64);
    hipLaunchKernelGGL(local_scale_kernel, dim3(blocks, N), dim3(256), 0, st, att, (const float*)partial, HW, (int)G);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

extern "C" {

int gdt_local_descriptors_workspace_bytes(int n, int h, int w, int d, int f32, size_t* bytes) {
    GDT_REQUIRE(bytes && n >= 1 && h >= 1 && w >= 1 && d >= 64 && d % 64 == 0 && d <= 8192, "local descriptors: n, h, w >= 1, d % 64 == 0, d <= 8192");
    *bytes = gdt_local_head_partial_floats(n, (long)h * w, d, f32) * sizeof(float);
    return GDT_OK;
}

int gdt_local_descriptors(const void* fmap, int f32, int n, int h, int w, int d, float eps, int normalize_max, float* desc, float* att, void* workspace,
                          size_t workspace_bytes, void* stream) {
    GDT_REQUIRE(fmap && desc && att, "null buffer");
    GDT_REQUIRE(n >= 1 && h >= 1 && w >= 1 && d >= 64 && d % 64 == 0 && d <= 8192, "local descriptors: n, h, w >= 1, d % 64 == 0, d <= 8192");
    GDT_REQUIRE((uintptr_t)fmap % 16 == 0, "local descriptors: the map must be 16-byte aligned");
    if (normalize_max && (!workspace || workspace_bytes < gdt_local_head_partial_floats(n, (long)h * w, d, f32) * sizeof(float))) {
        gdt_set_error("workspace too small for the maxima (gdt_local_descriptors_workspace_bytes)");
        return GDT_ERR_WORKSPACE;
    }
    return gdt_k_local_descriptors(fmap, f32, n, (long)h * w, d, eps, normalize_max ? 1 : 0, desc, att, (float*)workspace, (hipStream_t)stream);
}

}  // extern "C"
