// The descriptor head of the retrieval embedder behind the trunk (gfx950, MI355X): every pooling of cirtorch's POOLING table, global or regional,
// with the regional and the final whitening layers (mdir/external/cirtorch/networks/imageretrievalnet.py:101-123).
//
//   gdt_rpool_regions     the R-MAC region grid of LF.roipool / LF.rmac (layers/functional.py:26-123) -- host code, float32 like the reference's tensors
//   pool_regions_kernel   max / mean / GeM / per-channel GeM of EVERY region of an image in ONE pass over the map (layers/pooling.py:12-61 per region)
//   linear_rows_kernel    rows through an nn.Linear, fp32 FMA (the regional and the final whitening, imageretrievalnet.py:236, :254)
//   region_sum_kernel     sum over an image's regions (+ l2n): Rpool.forward (layers/pooling.py:105-108), the tail of LF.rmac (functional.py:73)
//   pixel_norm_kernel, attention_scale_kernel
//                         L2NormAttention (mdir/components/model/layers/attention.py:10-15): one weight per position, reduced across the channels; the weighted
//                         form of pool_regions_kernel folds it into the pooling pass (CirRetrievalNetAttention.forward, mdir/components/model/network/cirnet.py:116-125)
//
// The reference pools region by region (one narrow + pool call each, 15 to 51 per forward, GeM's pow once per region a pixel lies in).  Here a region is
// (row range) x (column band); a pixel's value -- for GeM: max(x, eps)^p, evaluated once -- is folded into the few column bands that contain x, and at
// the end of a row the band partials are folded into the regions whose row range contains y.  Max and sum are associative, so the result is exact for
// max and a fixed-order sum otherwise: two runs give the same bits.  No atomics.
#include <cmath>
#include <vector>

#include "../../include/gandtr_hip.h"
#include "aux_kernels.h"
#include "gdt_common.h"

// ------------------------------------------------------------------------------------------------ region grid (host)
// The reference computes the grid with float32 TENSORS: `b = (max(H, W) - w) / (steps - 1)` is Tensor.__rtruediv__, i.e. reciprocal(steps - 1) * n, the
// overlap test runs in float32 against float32(0.4), and a level's offsets are floor(wl2 + arange * float32(b)) with the product and the sum rounded
// separately.  Every intermediate below is a `volatile float` so that no step is contracted into an FMA or carried in higher precision.
int gdt_pool_grid(int H, int W, int L, std::vector<GdtPoolBox>& boxes) {
    GDT_REQUIRE(H >= 1 && W >= 1 && H <= 32767 && W <= 32767 && L >= 0 && L <= 16, "region grid: map size 1..32767, levels 0..16");
    boxes.clear();
    boxes.push_back(GdtPoolBox{0, 0, H, W});
    if (L == 0) return GDT_OK;
    const int w = std::min(H, W);
    int idx = 0;
    float best = 0.f;
    for (int s = 0; s < 6; ++s) {
        volatile float rcp = 1.0f / (float)(s + 1);                      // reciprocal(steps - 1), steps = 2..7
        volatile float b = rcp * (float)(std::max(H, W) - w);
        volatile float wb = (float)w * b;
        volatile float num = (float)(w * w) - wb;
        volatile float q = num / (float)(w * w);
        volatile float d = q - 0.4f;
        const float a = std::fabs(d);
        if (s == 0 || a < best) { best = a; idx = s; }                   // torch.min: the first of equal minima
    }
    const int Wd = H < W ? idx + 1 : 0, Hd = H > W ? idx + 1 : 0;
    for (int l = 1; l <= L; ++l) {
        const int wl = 2 * w / (l + 1);
        if (wl == 0) continue;
        const int wl2 = wl / 2 - 1;                                      // floor(wl / 2 - 1)
        auto offsets = [&](int extent, int count, std::vector<int>& out) {
            volatile float b = count == 1 ? 0.f : (float)((double)(extent - wl) / (double)(count - 1));
            out.resize(count);
            for (int i = 0; i < count; ++i) {
                volatile float prod = (float)i * b;
                volatile float sum = (float)wl2 + prod;
                out[i] = (int)std::floor(sum) - wl2;
            }
        };
        std::vector<int> ys, xs;
        offsets(W, l + Wd, xs);
        offsets(H, l + Hd, ys);
        for (int y : ys)
            for (int x : xs) {
                GDT_REQUIRE(y >= 0 && x >= 0 && y + wl <= H && x + wl <= W, "region grid: a region leaves the map");
                boxes.push_back(GdtPoolBox{y, x, wl, wl});
            }
    }
    return GDT_OK;
}

// boxes -> the kernel's (row range, column band) form
int gdt_pool_regions_of(const std::vector<GdtPoolBox>& boxes, GdtPoolRegions& g) {
    GDT_REQUIRE(!boxes.empty() && (int)boxes.size() <= GDT_POOL_MAX_REGIONS, "pooling regions: 1..64 regions per image");
    g.R = (int)boxes.size(); g.B = 0;
    for (int r = 0; r < g.R; ++r) {
        const GdtPoolBox& bx = boxes[r];
        int b = 0;
        while (b < g.B && !(g.bx0[b] == bx.x0 && g.bw[b] == bx.w)) ++b;
        if (b == g.B) { g.bx0[b] = (short)bx.x0; g.bw[b] = (short)bx.w; ++g.B; }      // (B <= R <= 64)
        g.ry0[r] = (short)bx.y0; g.rh[r] = (short)bx.h; g.rband[r] = (short)b;
    }
    return GDT_OK;
}

namespace {

// ------------------------------------------------------------------------------------------------ one-pass region pooling
// grid (D / 64, N), NW waves of 64 lanes; a lane owns a channel (a wave's load of a pixel is one 128-byte line of fp16, two of fp32), the waves split
// the rows.  LDS: per wave R region accumulators and B band partials of 64 floats; a lane only ever touches its own column of them, so nothing is
// shared inside a wave and the only barrier is the one before the waves' partials are combined (in wave order).
// Which bands contain x / which regions contain y: lane b holds band b's range, lane r region r's -- one compare + ballot gives the set as a mask.
// WEIGHTED: the value folded into the bands is x * wts[n][y][x] (one fp32 multiply in front of GeM's clamp and power: the pooling of CirRetrievalNetAttention sees
// feats * att); the weight of a pixel is the same for every lane of the wave, and the unweighted instantiation is the kernel it was.
template <typename T, int KIND, bool WEIGHTED>
__global__ __launch_bounds__(256) void pool_regions_kernel(const T* __restrict__ x, float* __restrict__ out, int H, int W, int D, float p,
                                                            const float* __restrict__ p_channels, float eps, const GdtPoolRegions g,
                                                            const float* __restrict__ wts) {
    extern __shared__ float acc[];
    constexpr bool MAX = KIND == GDT_POOL_MAX;
    const float ident = MAX ? -INFINITY : 0.f;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, NW = blockDim.x >> 6;
    const int n = blockIdx.y, d0 = blockIdx.x * 64;
    const int R = g.R, B = g.B;
    float* racc = acc + (size_t)wave * (R + B) * 64 + lane;
    float* bacc = racc + R * 64;
    for (int i = 0; i < R + B; ++i) racc[i * 64] = ident;
    const int bx0 = lane < B ? g.bx0[lane] : 0, bx1 = lane < B ? bx0 + g.bw[lane] : 0;
    const int ry0 = lane < R ? g.ry0[lane] : 0, ry1 = lane < R ? ry0 + g.rh[lane] : 0;
    float pc = p;
    if (KIND == GDT_POOL_GEMMP) pc = p_channels[d0 + lane];
    const bool cube = KIND == GDT_POOL_GEM && p == 3.0f;
    const T* img = x + (size_t)n * H * W * D + d0 + lane;
    for (int y = wave; y < H; y += NW) {
        const T* row = img + (size_t)y * W * D;
        const float* wrow = WEIGHTED ? wts + ((size_t)n * H + y) * W : nullptr;
        for (int x0 = 0; x0 < W; x0 += 8) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = x0 + j < W ? (float)row[(size_t)(x0 + j) * D] : 0.f;      // eight loads in flight per lane
            if (WEIGHTED) {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = x0 + j < W ? v[j] * wrow[x0 + j] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int xx = x0 + j;
                if (xx >= W) break;
                float f = v[j];
                if (KIND == GDT_POOL_GEM || KIND == GDT_POOL_GEMMP) {
                    f = fmaxf(f, eps);
                    f = cube ? f * f * f : powf(f, pc);
                }
                unsigned long long m = __ballot(xx >= bx0 && xx < bx1);
                while (m) {
                    const int b = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const float a = bacc[b * 64];
                    bacc[b * 64] = MAX ? fmaxf(a, f) : a + f;
                }
            }
        }
        unsigned long long m = __ballot(y >= ry0 && y < ry1);
        while (m) {
            const int r = __ffsll((long long)m) - 1;
            m &= m - 1;
            const float a = racc[r * 64], bnd = bacc[g.rband[r] * 64];
            racc[r * 64] = MAX ? fmaxf(a, bnd) : a + bnd;
        }
        for (int b = 0; b < B; ++b) bacc[b * 64] = ident;
    }
    __syncthreads();
    for (int r = wave; r < R; r += NW) {
        float t = acc[(size_t)r * 64 + lane];
        for (int k = 1; k < NW; ++k) {
            const float o = acc[((size_t)k * (R + B) + r) * 64 + lane];
            t = MAX ? fmaxf(t, o) : t + o;
        }
        const float cnt = (float)((int)g.rh[r] * (int)g.bw[g.rband[r]]);
        if (KIND == GDT_POOL_MEAN) t = t / cnt;
        if (KIND == GDT_POOL_GEM || KIND == GDT_POOL_GEMMP) t = powf(t / cnt, 1.0f / pc);
        out[((size_t)n * R + r) * D + d0 + lane] = t;
    }
}

// ------------------------------------------------------------------------------------------------ rows through a Linear
// out[r][o] = bias[o] + sum_k a[r][k] * w[o][k]  (nn.Linear: both operands K-contiguous).  64 x 64 output tile per workgroup, 4 x 4 per thread, K in
// steps of 16 through LDS (transposed while staging so that the inner loop reads float4s); fp32 FMA, k ascending: the same bits on every run.
__global__ __launch_bounds__(256) void linear_rows_kernel(const float* __restrict__ a, const float* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ out, int rows, int K, int Dout) {
    __shared__ float As[16][68], Ws[16][68];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int r0 = blockIdx.y * 64, o0 = blockIdx.x * 64;
    const int lr = tid >> 2, lk = (tid & 3) * 4;                 // staging: row of the tile, first of four k
    float c[4][4] = {};
    const bool a_ok = r0 + lr < rows;
    const float* ap = a + (size_t)(a_ok ? r0 + lr : 0) * K + lk;
    const float* wp = w + (size_t)(o0 + lr) * K + lk;
    for (int k0 = 0; k0 < K; k0 += 16) {
        const float4 av = a_ok ? *(const float4*)(ap + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 wv = *(const float4*)(wp + k0);
        __syncthreads();
        As[lk][lr] = av.x; As[lk + 1][lr] = av.y; As[lk + 2][lr] = av.z; As[lk + 3][lr] = av.w;
        Ws[lk][lr] = wv.x; Ws[lk + 1][lr] = wv.y; Ws[lk + 2][lr] = wv.z; Ws[lk + 3][lr] = wv.w;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const float4 a4 = *(const float4*)&As[kk][ty * 4], w4 = *(const float4*)&Ws[kk][tx * 4];
            const float av4[4] = {a4.x, a4.y, a4.z, a4.w}, wv4[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) c[i][j] = fmaf(av4[i], wv4[j], c[i][j]);
        }
    }
    const float4 b4 = *(const float4*)(bias + o0 + tx * 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + ty * 4 + i;
        if (r < rows) *(float4*)(out + (size_t)r * Dout + o0 + tx * 4) = make_float4(c[i][0] + b4.x, c[i][1] + b4.y, c[i][2] + b4.z, c[i][3] + b4.w);
    }
}

// ------------------------------------------------------------------------------------------------ sum over an image's regions (+ l2n)
// y[n][:] = sum_r v[n][r][:] (r ascending, as the reference's `v += vt` / `o.sum(1)`), then y / (||y||_2 + eps) when `l2n`; one workgroup per image
__global__ __launch_bounds__(256) void region_sum_kernel(const float* __restrict__ v, float* __restrict__ y, int R, int D, float eps, int l2n) {
    __shared__ float red[4];
    const float* vn = v + (size_t)blockIdx.x * R * D;
    float* yn = y + (size_t)blockIdx.x * D;
    float ss = 0.f;
    for (int i = threadIdx.x; i < D; i += 256) {
        float s = 0.f;
        for (int r = 0; r < R; ++r) s += vn[(size_t)r * D + i];
        yn[i] = s;
        ss += s * s;
    }
    if (!l2n) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    const float nrm = sqrtf(red[0] + red[1] + red[2] + red[3]) + eps;
    for (int i = threadIdx.x; i < D; i += 256) yn[i] = yn[i] / nrm;          // (each thread rescales the entries it wrote itself)
}

template <typename T, bool WEIGHTED>
void launch_pool(int kind, dim3 grid, dim3 block, size_t lds, hipStream_t st, const T* x, float* out, int H, int W, int D, float p, const float* pch,
                 float eps, const GdtPoolRegions& g, const float* wts) {
    switch (kind) {
        case GDT_POOL_MAX: hipLaunchKernelGGL((pool_regions_kernel<T, GDT_POOL_MAX, WEIGHTED>), grid, block, lds, st, x, out, H, W, D, p, pch, eps, g, wts); break;
        case GDT_POOL_MEAN: hipLaunchKernelGGL((pool_regions_kernel<T, GDT_POOL_MEAN, WEIGHTED>), grid, block, lds, st, x, out, H, W, D, p, pch, eps, g, wts); break;
        case GDT_POOL_GEM: hipLaunchKernelGGL((pool_regions_kernel<T, GDT_POOL_GEM, WEIGHTED>), grid, block, lds, st, x, out, H, W, D, p, pch, eps, g, wts); break;
        default: hipLaunchKernelGGL((pool_regions_kernel<T, GDT_POOL_GEMMP, WEIGHTED>), grid, block, lds, st, x, out, H, W, D, p, pch, eps, g, wts); break;
    }
}

// ------------------------------------------------------------------------------------------------ pixel attention (L2NormAttention)
// out[n][pixel] = sqrt(sum_c x_c^2 + 1e-10).  A pixel's D channels are contiguous: a wave takes ATT_PX pixels at a time, a lane the 16-byte pieces lane, lane + 64, ..
// of each (ascending), squares accumulated in fp32, then the xor butterfly across the lanes: the order of the sum is fixed by D alone, and every lane ends with the
// same bits.  grid (G, N): workgroup g of an image takes the wave-chunks g, g + G, ..; with MAXP the workgroup's maximum goes to partial[n][g] (a maximum is exact in
// any order; no atomics) and attention_scale_kernel finishes: maximum of the G partials, then a / M -- a division, as the reference's m / m.max().
constexpr int ATT_PX = 4;             // pixels a wave has in flight
constexpr int ATT_MAX_GROUPS = 256;   // workgroups per image at most

template <typename T>
__global__ __launch_bounds__(256) void pixel_norm_kernel(const T* __restrict__ x, float* __restrict__ out, float* __restrict__ partial, long HW, int D, int maxp) {
    constexpr int E = 16 / sizeof(T);            // elements of a 16-byte piece
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.y, pieces = D / E;
    const T* img = x + (size_t)n * HW * D;
    float* o = out + (size_t)n * HW;
    float wmax = 0.f;
    for (long p0 = ((long)blockIdx.x * 4 + wave) * ATT_PX; p0 < HW; p0 += (long)gridDim.x * 4 * ATT_PX) {
        float acc[ATT_PX];
#pragma unroll
        for (int j = 0; j < ATT_PX; ++j) acc[j] = 0.f;
        for (int pc = lane; pc < pieces; pc += 64) {
            float v[ATT_PX][E];
#pragma unroll
            for (int j = 0; j < ATT_PX; ++j) {
                const long px = p0 + j < HW ? p0 + j : HW - 1;            // (a chunk past the end repeats the last pixel: loads stay inside the map)
                const T* src = img + (size_t)px * D + (size_t)pc * E;
                if constexpr (sizeof(T) == 2) {
                    const f16x8 t = *(const f16x8*)src;
#pragma unroll
                    for (int e = 0; e < E; ++e) v[j][e] = (float)t[e];
                } else {
                    const float4 t = *(const float4*)src;
                    v[j][0] = t.x; v[j][1] = t.y; v[j][2] = t.z; v[j][3] = t.w;
                }
            }
#pragma unroll
            for (int j = 0; j < ATT_PX; ++j)
#pragma unroll
                for (int e = 0; e < E; ++e) acc[j] = fmaf(v[j][e], v[j][e], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < ATT_PX; ++j) {
            float s = acc[j];
#pragma unroll
            for (int k = 32; k > 0; k >>= 1) s += __shfl_xor(s, k);
            const float m = sqrtf(s + 1e-10f);
            if (p0 + j < HW) {
                wmax = fmaxf(wmax, m);
                if (lane == j) o[p0 + j] = m;
            }
        }
    }
    if (!maxp) return;
    if (lane == 0) red[wave] = wmax;
    __syncthreads();
    if (threadIdx.x == 0) partial[(size_t)n * gridDim.x + blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// a[n][pixel] /= max_g partial[n][g]; grid (blocks over the pixels, N), G <= ATT_MAX_GROUPS = one partial per thread at most
__global__ __launch_bounds__(256) void attention_scale_kernel(float* __restrict__ a, const float* __restrict__ partial, long HW, int G) {
    __shared__ float red[4];
    const int n = blockIdx.y;
    float m = threadIdx.x < G ? partial[(size_t)n * G + threadIdx.x] : 0.f;
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) m = fmaxf(m, __shfl_xor(m, k));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    const float M = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float* an = a + (size_t)n * HW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long)gridDim.x * 256) an[i] = an[i] / M;
}

int attention_groups(long HW) {
    const long chunks = (HW + 4 * ATT_PX - 1) / (4 * ATT_PX);
    return (int)std::min<long>(std::max<long>(chunks, 1), ATT_MAX_GROUPS);
}

}  // namespace

size_t gdt_pixel_attention_partial_floats(int N, long HW) { return (size_t)N * attention_groups(HW); }

int gdt_k_pixel_attention(const void* x, int f32, int N, long HW, int D, int normalize_max, float* out, float* partial, hipStream_t st) {
    GDT_REQUIRE(N >= 1 && N <= 65535 && HW >= 1 && D >= 64 && D % 64 == 0, "pixel attention needs D % 64 == 0 and at most 65535 images");
    GDT_REQUIRE(!normalize_max || partial, "pixel attention: the maximum needs its workspace");
    const int G = attention_groups(HW);
    if (f32) hipLaunchKernelGGL(pixel_norm_kernel<float>, dim3(G, N), dim3(256), 0, st, (const float*)x, out, partial, HW, D, normalize_max);
    else hipLaunchKernelGGL(pixel_norm_kernel<f16>, dim3(G, N), dim3(256), 0, st, (const f16*)x, out, partial, HW, D, normalize_max);
    GDT_CHECK_HIP(hipGetLastError());
    if (!normalize_max) return GDT_OK;
    const int blocks = (int)std::min<long>((HW + 255) / 256, 64);
    hipLaunchKernelGGL(attention_scale_kernel, dim3(blocks, N), dim3(256), 0, st, out, (const float*)partial, HW, G);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

int gdt_k_pool_regions(const void* x, int f32, float* out, int N, int H, int W, int D, int kind, float p, const float* p_channels, float eps,
                       const GdtPoolRegions& g, hipStream_t st, const float* weights) {
    GDT_REQUIRE(D % 64 == 0, "region pooling needs D % 64 == 0");
    GDT_REQUIRE(kind >= GDT_POOL_MAX && kind <= GDT_POOL_GEMMP, "pooling kind 0..3 (max, mean, GeM, per-channel GeM)");
    GDT_REQUIRE(kind != GDT_POOL_GEMMP || p_channels, "per-channel GeM needs its exponents");
    GDT_REQUIRE(kind < GDT_POOL_GEM || kind == GDT_POOL_GEMMP || p > 0.f, "GeM exponent must be positive");
    GDT_REQUIRE(g.R >= 1 && g.R <= GDT_POOL_MAX_REGIONS && g.B >= 1 && g.B <= g.R, "pooling regions: 1..64 regions per image");
    for (int r = 0; r < g.R; ++r) {           // every region inside the map: the kernel trusts the table
        const int b = g.rband[r];
        GDT_REQUIRE(b >= 0 && b < g.B && g.ry0[r] >= 0 && g.rh[r] >= 1 && g.ry0[r] + g.rh[r] <= H && g.bx0[b] >= 0 && g.bw[b] >= 1 && g.bx0[b] + g.bw[b] <= W,
                    "pooling regions: a region leaves the map");
    }
    // four waves where their accumulators fit 48 KB of LDS (R + B <= 48: every map but the extreme aspect ratios), else two (R + B <= 128: 64 KB)
    const size_t per_wave = (size_t)(g.R + g.B) * 64 * sizeof(float);
    const int nw = 4 * per_wave <= 49152 ? 4 : 2;
    const dim3 grid(D / 64, N), block(64 * nw);
    if (weights) {
        if (f32) launch_pool<float, true>(kind, grid, block, per_wave * nw, st, (const float*)x, out, H, W, D, p, p_channels, eps, g, weights);
        else launch_pool<f16, true>(kind, grid, block, per_wave * nw, st, (const f16*)x, out, H, W, D, p, p_channels, eps, g, weights);
    } else {
        if (f32) launch_pool<float, false>(kind, grid, block, per_wave * nw, st, (const float*)x, out, H, W, D, p, p_channels, eps, g, nullptr);
        else launch_pool<f16, false>(kind, grid, block, per_wave * nw, st, (const f16*)x, out, H, W, D, p, p_channels, eps, g, nullptr);
    }
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

int gdt_k_linear_rows(const float* a, const float* w, const float* bias, float* out, int rows, int K, int Dout, hipStream_t st) {
    GDT_REQUIRE(rows >= 1 && K % 16 == 0 && Dout % 64 == 0, "linear rows: K % 16 == 0 and outputs % 64 == 0");
    hipLaunchKernelGGL(linear_rows_kernel, dim3(Dout / 64, (rows + 63) / 64), dim3(256), 0, st, a, w, bias, out, rows, K, Dout);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

int gdt_k_region_sum(const float* v, float* y, int N, int R, int D, float eps, int l2n, hipStream_t st) {
    hipLaunchKernelGGL(region_sum_kernel, dim3(N), dim3(256), 0, st, v, y, R, D, eps, l2n);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

size_t gdt_pool_head_scratch_floats(int N, int R, int D) { return 2 * (size_t)N * R * D + 2 * (size_t)N * D; }

// The head behind the map, as ImageRetrievalNet.forward runs it: pool -> l2n -> (whiten -> l2n).  `aggregate`: the pooled vectors are regions to be
// l2-normalised one by one and summed -- 1 = R-MAC (no l2n of the sum inside the pool), 2 = Rpool (optional regional whitening + l2n per region, l2n of
// the sum); the net's own l2n follows either.  The number of launches depends on the layers present, not on N or R; the map is read by the first only.
int gdt_k_pool_head(const void* x, int f32, int N, int H, int W, int D, const GdtPoolHead& hd, const GdtPoolRegions& g, float* scratch, float* out,
                    hipStream_t st) {
    const int R = g.R;
    GDT_REQUIRE(hd.aggregate >= 0 && hd.aggregate <= 2 && (hd.aggregate || R == 1), "pool head: regions need an aggregation");
    GDT_REQUIRE(!hd.rw || hd.aggregate == 2, "pool head: the regional whitening belongs to a regional pooling");
    float* P = scratch; float* Q = P + (size_t)N * R * D; float* U = Q + (size_t)N * R * D; float* V = U + (size_t)N * D;
    int rc = gdt_k_pool_regions(x, f32, P, N, H, W, D, hd.kind, hd.p, hd.p_channels, hd.eps, g, st, hd.weights);
    if (rc != GDT_OK) return rc;
    float* cur;                             // the [N][D] vector after the net's first l2n
    if (!hd.aggregate) {
        cur = hd.fw ? U : out;
        rc = gdt_k_l2n_rows(P, cur, N, D, hd.eps_l2, st);
    } else {
        rc = gdt_k_l2n_rows(P, Q, N * R, D, hd.eps_l2, st);
        if (rc == GDT_OK && hd.rw) {
            rc = gdt_k_linear_rows(Q, hd.rw, hd.rb, P, N * R, D, D, st);
            if (rc == GDT_OK) rc = gdt_k_l2n_rows(P, Q, N * R, D, hd.eps_l2, st);
        }
        if (rc != GDT_OK) return rc;
        if (hd.aggregate == 1) {            // R-MAC: the sum, then the net's l2n
            cur = hd.fw ? U : out;
            rc = gdt_k_region_sum(Q, cur, N, R, D, hd.eps_l2, 1, st);
        } else {                            // Rpool: l2n of the sum inside the pool, then the net's
            cur = hd.fw ? V : out;
            rc = gdt_k_region_sum(Q, U, N, R, D, hd.eps_l2, 1, st);
            if (rc == GDT_OK) rc = gdt_k_l2n_rows(U, cur, N, D, hd.eps_l2, st);
        }
    }
    if (rc != GDT_OK || !hd.fw) return rc;
    float* t = cur == U ? V : U;
    rc = gdt_k_linear_rows(cur, hd.fw, hd.fb, t, N, D, D, st);
    if (rc == GDT_OK) rc = gdt_k_l2n_rows(t, out, N, D, hd.eps_l2, st);
    return rc;
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" {

int gdt_rpool_regions(int h, int w, int levels, int* boxes, int capacity, int* count) {
    GDT_REQUIRE(count && (boxes || capacity == 0) && capacity >= 0, "region grid buffers");
    std::vector<GdtPoolBox> bx;
    const int rc = gdt_pool_grid(h, w, levels, bx);
    if (rc != GDT_OK) return rc;
    *count = (int)bx.size();
    GDT_REQUIRE(capacity == 0 || capacity >= (int)bx.size(), "region grid: capacity too small (count holds the number of regions)");
    if (capacity)
        for (size_t r = 0; r < bx.size(); ++r) { boxes[4 * r] = bx[r].y0; boxes[4 * r + 1] = bx[r].x0; boxes[4 * r + 2] = bx[r].h; boxes[4 * r + 3] = bx[r].w; }
    return GDT_OK;
}

int gdt_pool_regions(const void* fmap, int f32, int n, int h, int w, int d, int kind, float p, const float* p_channels, float eps, int levels,
                     float* out, void* stream) {
    GDT_REQUIRE(fmap && out && n >= 1 && d >= 1 && (f32 == 0 || f32 == 1), "pool_regions arguments");
    std::vector<GdtPoolBox> bx;
    int rc = gdt_pool_grid(h, w, levels, bx);
    if (rc != GDT_OK) return rc;
    GdtPoolRegions g{};
    rc = gdt_pool_regions_of(bx, g);
    if (rc != GDT_OK) return rc;
    return gdt_k_pool_regions(fmap, f32, out, n, h, w, d, kind, p, p_channels, eps, g, (hipStream_t)stream);
}

int gdt_pool_regions_weighted(const void* fmap, int f32, int n, int h, int w, int d, int kind, float p, const float* p_channels, float eps, int levels,
                              const float* weights, float* out, void* stream) {
    GDT_REQUIRE(fmap && out && weights && n >= 1 && d >= 1 && (f32 == 0 || f32 == 1), "pool_regions_weighted arguments");
    std::vector<GdtPoolBox> bx;
    int rc = gdt_pool_grid(h, w, levels, bx);
    if (rc != GDT_OK) return rc;
    GdtPoolRegions g{};
    rc = gdt_pool_regions_of(bx, g);
    if (rc != GDT_OK) return rc;
    return gdt_k_pool_regions(fmap, f32, out, n, h, w, d, kind, p, p_channels, eps, g, (hipStream_t)stream, weights);
}

int gdt_pixel_attention_workspace_bytes(int n, int h, int w, size_t* bytes) {
    GDT_REQUIRE(bytes && n >= 1 && h >= 1 && w >= 1 && h <= 32767 && w <= 32767, "pixel attention geometry");
    *bytes = gdt_pixel_attention_partial_floats(n, (long)h * w) * sizeof(float);
    return GDT_OK;
}

int gdt_pixel_attention(const void* fmap, int f32, int n, int h, int w, int d, int normalize_max, float* out, void* workspace, size_t workspace_bytes,
                        void* stream) {
    GDT_REQUIRE(fmap && out && n >= 1 && h >= 1 && w >= 1 && h <= 32767 && w <= 32767 && d >= 1 && (f32 == 0 || f32 == 1), "pixel_attention arguments");
    GDT_REQUIRE(normalize_max == 0 || normalize_max == 1, "pixel_attention: normalize_max is 0 or 1");
    GDT_REQUIRE(d % 64 == 0 && n <= 65535, "pixel attention needs D % 64 == 0 and at most 65535 images");
    if (normalize_max)
        GDT_REQUIRE(workspace && workspace_bytes >= gdt_pixel_attention_partial_floats(n, (long)h * w) * sizeof(float), "pixel_attention: workspace too small");
    return gdt_k_pixel_attention(fmap, f32, n, (long)h * w, d, normalize_max, out, (float*)workspace, (hipStream_t)stream);
}

}  // extern "C"
