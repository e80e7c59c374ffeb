// Geometric-median pooling of the retrieval embedder (gfx950, MI355X): GeometricMedianWeiszfeld / WeightedGeometricMedianWeiszfeld of
// mdir/components/model/layers/pooling.py:44-95 on an NHWC map, per image.
//
//   y_i = s_i * x_i,  w_i = a_i  (s, a: optional fp32 arrays, one value per position; absent = 1)
//   T times:  m = sum_i w_i y_i / sum_i w_i ;  w_i = a_i / sqrt(sum_c (y_ic - m_c)^2 + 1e-10)
//   result:   m = sum_i w_i y_i / sum_i w_i
//
// The reference evaluates an iteration with six full passes of torch ops over the map and materialises x * weights.  Here an iteration is ONE read of the map:
// a wave takes a pixel's D channels into registers (lane l holds the 16-byte pieces l, l + 64, ..), reduces sum (y - m)^2 over its registers and across the
// lanes, and folds the SAME registers, times the weight, into its per-lane accumulators of sum w y.  The squared distance is evaluated as written above, never as
// |y|^2 - 2 y.m + |m|^2: the positions close to the median are the ones with the large weights.  A position equal to the median gets a_i * 1e5: no special case.
//
// Order of the sums (no atomics): an image's pixels are cut into G contiguous ranges, G a function of H * W alone; a workgroup takes one range, its four waves
// every fourth pixel of it in ascending order; the waves' sums are added in wave order, the workgroups' partials ([G][D] and [G]) by median_finish_kernel in
// range order, and the division by sum w is a division, as the reference's.  Two runs give the same bits; image k of a batch gives the bits it gives alone.
#include <type_traits>

#include "../../include/gandtr_hip.h"
#include "aux_kernels.h"
#include "gdt_common.h"

namespace {

constexpr int MED_MAX_GROUPS = 64;      // workgroups per image at most
constexpr int MED_GROUP_PX = 32;        // pixels a workgroup takes at least (while the image has them)
constexpr int MED_MAX_D = 4096;         // channels at most: 16 pieces of 16 bytes per lane in fp32

int median_groups(long HW) { return (int)std::min<long>(std::max<long>(HW / MED_GROUP_PX, 1), MED_MAX_GROUPS); }

// The sum of a value over the 64 lanes, the same bits for every lane, in a fixed order: inside a row of 16 lanes by four DPP adds (lane xor 1, lane xor 2, then
// the rotations by 4 and by 8 as lane 0 of the row sees them), then the four rows' sums, read from their first lanes, as (r0 + r1) + (r2 + r3).  No LDS
// traffic: a butterfly of __shfl_xor is six round trips through ds_bpermute per pixel, which is what a pass over the map then waits for.
__device__ __forceinline__ float dpp_add(float v, float moved) { return v + moved; }
template <int CTRL>
__device__ __forceinline__ float dpp_move(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float wave_sum(float v) {
    v = dpp_add(v, dpp_move<0xB1>(v));        // quad_perm [1, 0, 3, 2]
    v = dpp_add(v, dpp_move<0x4E>(v));        // quad_perm [2, 3, 0, 1]
    v = dpp_add(v, dpp_move<0x124>(v));       // row_ror 4
    v = dpp_add(v, dpp_move<0x128>(v));       // row_ror 8
    const int b = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
    return (r0 + r1) + (r2 + r3);
}

// grid (G, N), 256 threads.  PP: 16-byte pieces a lane holds of a pixel (pieces lane + 64 k, k < PP, those below D / E exist); PREV: weights from the distance to
// mprev[n][D], else the first pass (w = a).  part[n][g][D], wpart[n][g]: the workgroup's sums.  Dynamic LDS: 3 * D floats (the sums of waves 1..3).
template <typename T, int PP, bool PREV>
__global__ __launch_bounds__(256) void median_pass_kernel(const T* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ prior,
                                                          const float* __restrict__ mprev, float* __restrict__ part, float* __restrict__ wpart, long HW, int D) {
    constexpr int E = 16 / sizeof(T);                                           // elements of a 16-byte piece
    constexpr int RING = PP >= 8 ? 2 : PP == 4 ? 3 : 4;                         // pixels a wave has in flight, as loaded (16 bytes per piece and lane)
    using Raw = typename std::conditional<sizeof(T) == 2, f16x8, f32x4>::type;
    extern __shared__ float wsum_lds[];
    __shared__ float wred[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.y, g = blockIdx.x, G = gridDim.x, pieces = D / E;
    const long p_begin = (long)g * HW / G, p_end = (long)(g + 1) * HW / G;       // (G <= HW: no range is empty)
    const T* img = x + (size_t)n * HW * D;
    const float* sc = scale ? scale + (size_t)n * HW : nullptr;
    const float* pr = prior ? prior + (size_t)n * HW : nullptr;

    float m[PP][E], acc[PP][E];
#pragma unroll
    for (int k = 0; k < PP; ++k)
#pragma unroll
        for (int e = 0; e < E; ++e) {
            acc[k][e] = 0.f;
            m[k][e] = PREV && lane + 64 * k < pieces ? mprev[(size_t)n * D + (size_t)(lane + 64 * k) * E + e] : 0.f;
        }
    float wsum = 0.f;                                                           // (the same bits in every lane of the wave)

    // The wave's pixels are p_begin + wave + 4 i, i = 0 .. count - 1, taken in ascending order.  RING of them are in flight: a slot is loaded again, with the
    // pixel RING further on, as soon as its pixel has been folded in, so that the loads of the next pixels are under way while one is reduced.
    const long count = p_begin + wave < p_end ? (p_end - p_begin - wave + 3) / 4 : 0;
    Raw ring[RING][PP];
    float ring_s[RING], ring_a[RING];
    auto load = [&](int r, long i) {
        const long px = p_begin + wave + 4 * i;                                  // (i < count: inside the range)
#pragma unroll
        for (int k = 0; k < PP; ++k) {
            const int pc = lane + 64 * k;
            if (pc < pieces) ring[r][k] = *(const Raw*)(img + (size_t)px * D + (size_t)pc * E);
            else ring[r][k] = Raw{};
        }
        ring_s[r] = sc ? sc[px] : 1.f;
        ring_a[r] = pr ? pr[px] : 1.f;
    };
#pragma unroll
    for (int r = 0; r < RING; ++r)
        if (r < count) load(r, r);
    for (long base = 0; base < count; base += RING) {
#pragma unroll
        for (int r = 0; r < RING; ++r) {
            if (base + r >= count) break;                                        // (wave-uniform)
            const float s = ring_s[r];
            float w = ring_a[r];
            if (PREV) {
                float d2 = 0.f;
#pragma unroll
                for (int k = 0; k < PP; ++k)
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        const float df = (float)ring[r][k][e] * s - m[k][e];
                        d2 = fmaf(df, df, d2);
                    }
                w = w / sqrtf(wave_sum(d2) + 1e-10f);
            }
            wsum += w;
#pragma unroll
            for (int k = 0; k < PP; ++k)
#pragma unroll
                for (int e = 0; e < E; ++e) acc[k][e] = fmaf(w, (float)ring[r][k][e] * s, acc[k][e]);
            if (base + r + RING < count) load(r, base + r + RING);
        }
    }

    // the waves' sums, in wave order
    if (wave > 0) {
#pragma unroll
        for (int k = 0; k < PP; ++k)
            if (lane + 64 * k < pieces)
#pragma unroll
                for (int e = 0; e < E; ++e) wsum_lds[(size_t)(wave - 1) * D + (size_t)(lane + 64 * k) * E + e] = acc[k][e];
    }
    if (lane == 0) wred[wave] = wsum;
    __syncthreads();
    if (wave > 0) return;
    float* dst = part + ((size_t)n * G + g) * D;
#pragma unroll
    for (int k = 0; k < PP; ++k)
        if (lane + 64 * k < pieces)
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const size_t c = (size_t)(lane + 64 * k) * E + e;
                dst[c] = ((acc[k][e] + wsum_lds[c]) + wsum_lds[(size_t)D + c]) + wsum_lds[2 * (size_t)D + c];
            }
    if (lane == 0) wpart[(size_t)n * G + g] = ((wred[0] + wred[1]) + wred[2]) + wred[3];
}

// out[n][c] = (sum_g part[n][g][c]) / (sum_g wpart[n][g]), g ascending; grid (ceil(D / 256), N)
__global__ __launch_bounds__(256) void median_finish_kernel(const float* __restrict__ part, const float* __restrict__ wpart, float* __restrict__ out, int G, int D) {
    const int n = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= D) return;
    float s = 0.f, ws = 0.f;
    for (int g = 0; g < G; ++g) {
        s += part[((size_t)n * G + g) * D + c];
        ws += wpart[(size_t)n * G + g];
    }
    out[(size_t)n * D + c] = s / ws;
}

template <typename T, int PP>
void launch_pass(bool prev, dim3 grid, size_t lds, hipStream_t st, const T* x, const float* scale, const float* prior, const float* mprev, float* part,
                 float* wpart, long HW, int D) {
    if (prev) hipLaunchKernelGGL((median_pass_kernel<T, PP, true>), grid, dim3(256), lds, st, x, scale, prior, mprev, part, wpart, HW, D);
    else hipLaunchKernelGGL((median_pass_kernel<T, PP, false>), grid, dim3(256), lds, st, x, scale, prior, mprev, part, wpart, HW, D);
}

template <typename T>
void launch_pass_pp(int pp, bool prev, dim3 grid, size_t lds, hipStream_t st, const T* x, const float* scale, const float* prior, const float* mprev,
                    float* part, float* wpart, long HW, int D) {
    switch (pp) {
        case 1: launch_pass<T, 1>(prev, grid, lds, st, x, scale, prior, mprev, part, wpart, HW, D); break;
        case 2: launch_pass<T, 2>(prev, grid, lds, st, x, scale, prior, mprev, part, wpart, HW, D); break;
        case 4: launch_pass<T, 4>(prev, grid, lds, st, x, scale, prior, mprev, part, wpart, HW, D); break;
        case 8: launch_pass<T, 8>(prev, grid, lds, st, x, scale, prior, mprev, part, wpart, HW, D); break;
        default:                                                                 // (fp32 alone: D <= 4096 is at most 8 pieces per lane in fp16)
            if constexpr (sizeof(T) == 4) launch_pass<T, 16>(prev, grid, lds, st, x, scale, prior, mprev, part, wpart, HW, D);
            break;
    }
}

}  // namespace

// the workgroups' partial sums [N][G][D] and [N][G], and the previous median [N][D]
size_t gdt_geometric_median_scratch_floats(int N, long HW, int D) {
    const size_t G = (size_t)median_groups(HW);
    return (size_t)N * G * D + (size_t)N * G + (size_t)N * D;
}

int gdt_geometric_median_check(int n, int h, int w, int d, int iterations) {
    GDT_REQUIRE(n >= 1 && n <= 65535 && h >= 1 && w >= 1 && h <= 32767 && w <= 32767, "geometric median: map size 1..32767, at most 65535 images");
    GDT_REQUIRE(d >= 64 && d % 64 == 0 && d <= MED_MAX_D, "geometric median needs D % 64 == 0 and D <= 4096");
    GDT_REQUIRE(iterations >= 0 && iterations <= GDT_MEDIAN_MAX_ITERATIONS, "geometric median: 0..64 iterations");
    return GDT_OK;
}

// T + 1 passes over the map, each followed by its finishing step: 2 (T + 1) launches whatever N
int gdt_k_geometric_median(const void* x, int f32, int N, long HW, int D, int iterations, const float* scale, const float* prior, float* out, float* scratch,
                           hipStream_t st) {
    GDT_REQUIRE(D >= 64 && D % 64 == 0 && D <= MED_MAX_D && N >= 1 && N <= 65535 && HW >= 1, "geometric median needs D % 64 == 0 and D <= 4096");
    GDT_REQUIRE(iterations >= 0 && iterations <= GDT_MEDIAN_MAX_ITERATIONS, "geometric median: 0..64 iterations");
    const int G = median_groups(HW);
    float* part = scratch; float* wpart = part + (size_t)N * G * D; float* m = wpart + (size_t)N * G;
    const int pieces = D / (f32 ? 4 : 8);
    int pp = 1;
    while (64 * pp < pieces) pp *= 2;
    const size_t lds = 3 * (size_t)D * sizeof(float);                            // (<= 48 KB)
    for (int t = 0; t <= iterations; ++t) {
        if (f32) launch_pass_pp<float>(pp, t > 0, dim3(G, N), lds, st, (const float*)x, scale, prior, m, part, wpart, HW, D);
        else launch_pass_pp<f16>(pp, t > 0, dim3(G, N), lds, st, (const f16*)x, scale, prior, m, part, wpart, HW, D);
        GDT_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(median_finish_kernel, dim3((D + 255) / 256, N), dim3(256), 0, st, (const float*)part, (const float*)wpart, t == iterations ? out : m, G, D);
        GDT_CHECK_HIP(hipGetLastError());
    }
    return GDT_OK;
}

size_t gdt_median_head_scratch_floats(int N, long HW, int D) { return gdt_geometric_median_scratch_floats(N, HW, D) + 3 * (size_t)N * D; }

// The head behind the map with this pooling, as ImageRetrievalNet.forward runs it: median -> l2n -> (whiten -> l2n).  `scale`: the attention net's weights.
int gdt_k_median_head(const void* x, int f32, int N, long HW, int D, int iterations, const float* scale, const float* fw, const float* fb, float eps_l2,
                      float* scratch, float* out, hipStream_t st) {
    float* P = scratch + gdt_geometric_median_scratch_floats(N, HW, D); float* U = P + (size_t)N * D; float* V = U + (size_t)N * D;
    int rc = gdt_k_geometric_median(x, f32, N, HW, D, iterations, scale, nullptr, P, scratch, st);
    if (rc != GDT_OK) return rc;
    rc = gdt_k_l2n_rows(P, fw ? U : out, N, D, eps_l2, st);
    if (rc != GDT_OK || !fw) return rc;
    rc = gdt_k_linear_rows(U, fw, fb, V, N, D, D, st);
    if (rc == GDT_OK) rc = gdt_k_l2n_rows(V, out, N, D, eps_l2, st);
    return rc;
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" {

int gdt_geometric_median_workspace_bytes(int n, int h, int w, int d, size_t* bytes) {
    GDT_REQUIRE(bytes != nullptr, "geometric median: bytes");
    const int rc = gdt_geometric_median_check(n, h, w, d, 0);
    if (rc != GDT_OK) return rc;
    *bytes = gdt_geometric_median_scratch_floats(n, (long)h * w, d) * sizeof(float);
    return GDT_OK;
}

int gdt_geometric_median(const void* fmap, int f32, int n, int h, int w, int d, int iterations, const float* scale, const float* prior, float* out,
                         void* workspace, size_t workspace_bytes, void* stream) {
    GDT_REQUIRE(fmap && out && (f32 == 0 || f32 == 1), "geometric_median arguments");
    const int rc = gdt_geometric_median_check(n, h, w, d, iterations);
    if (rc != GDT_OK) return rc;
    GDT_REQUIRE(workspace && workspace_bytes >= gdt_geometric_median_scratch_floats(n, (long)h * w, d) * sizeof(float), "geometric_median: workspace too small");
    return gdt_k_geometric_median(fmap, f32, n, (long)h * w, d, iterations, scale, prior, out, (float*)workspace, (hipStream_t)stream);
}

}  // extern "C"
