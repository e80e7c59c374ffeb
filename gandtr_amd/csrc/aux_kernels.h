// Launchers of the helper kernels in aux_kernels.hip (internal to the library; the public ABI is include/gandtr_hip.h).
// `f32` selects the activation element type: 0 = fp16 NHWC (default), 1 = fp32 NHWC ("f16x3" / "f16c" precision modes);
// gdt_k_pack_input also takes 2 = fp16 NHWC8 pixel words augmented with their own rounding residuals (conv_stem.hip, f16c form).
#pragma once
#include <vector>

#include "gdt_common.h"

// ---- device side, shared by the helper kernels (aux_kernels.hip, blur_resample.hip)
// activation element access: 8 consecutive channels as fp32, for fp16 (default) and fp32 ("f16x3" precision mode) tensors
__device__ __forceinline__ void load8(const f16* p, float (&v)[8]) {
    const f16x8 t = *(const f16x8*)p;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)t[e];
}
__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
    const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void store8(f16* p, const float (&v)[8]) {
    f16x8 t;
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = (f16)v[e];
    *(f16x8*)p = t;
}
__device__ __forceinline__ void store8(float* p, const float (&v)[8]) {
    *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
    *(float4*)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// A per-pixel function of the input pack, applied in fp32 behind resize, permutation and affine and in front of the rounding to fp16.  kind 1 = EdgeFilter
// (mdir/components/model/layers/preprocessing.py:18-25): w * max(x, eps)^p / (exp(min(-beta * (x - tau), 50)) + 1); tau is clamped by whoever fills this.
struct GdtInputFilter { int kind = 0; float w = 0.f, p = 0.f, beta = 0.f, tau = 0.f, eps = 0.f; };
enum { GDT_FILTER_NONE = 0, GDT_FILTER_EDGE = 1 };
int gdt_k_pack_input(const float* x, void* y, int f32, int N, int C, int H, int W, int OH, int OW, float rscale, int resize,
                     const int* perm, const float* scale, const float* shift, hipStream_t st, const GdtInputFilter* filter = nullptr);
int gdt_in_stats_chunks(int HW);
int gdt_k_instance_norm(const void* x, const void* res, void* y, int f32, float* partial, float* mean_rstd, int N, int HW, int C,
                        float eps, int relu, hipStream_t st, float leaky = 0.f);      // leaky: LeakyReLU slope applied instead of ReLU (0: none)
int gdt_k_instance_norm_fused(const void* x, const void* res, void* y, int f32, const float* tile_partials, int tiles_per_image,
                              int nphase, float* mean_rstd, int N, int HW, int C, float eps, int relu, hipStream_t st);
int gdt_k_instance_norm_stats(const void* x, int f32, int fused, float* partial, int tiles_per_image, int nphase, float* mean_rstd,
                              int N, int HW, int C, float eps, hipStream_t st);
int gdt_k_maxpool(const void* x, void* y, int f32, int N, int H, int W, int C, int OH, int OW, int k, int s, int p, hipStream_t st);
// F.interpolate(x [N][H][W][C], size=(OH, OW), mode 0 "bilinear" (align_corners=False) | 1 "nearest") -> y [N][OH][OW][C]
int gdt_k_resize(const void* x, void* y, int f32, int N, int H, int W, int C, int OH, int OW, int mode, hipStream_t st);
// The anti-aliased sampling of gdt_net_blur_resample (blur_resample.hip): x [N][H][W][C] -> y [N][ceil(H/2)][ceil(W/2)][C] (down; H, W >= 2) / [N][2H][2W][C] (up).
// mean_rstd == null: the plain form.  Else the norm-folded form: (x - mean) * rstd of the InstanceNorm's [N][C][2] slab, then the ReLU when `relu`, on every tap as it is read.
int gdt_k_blur_down(const void* x, void* y, int f32, int N, int H, int W, int C, const float* mean_rstd, int relu, hipStream_t st);
int gdt_k_blur_up(const void* x, void* y, int f32, int N, int H, int W, int C, const float* mean_rstd, int relu, hipStream_t st);
// y[.., 0 .. ca) = a (+ ReLU), y[.., ca .. ca + cb) = b, zero up to C: torch.cat along the channels of NHWC tensors with channel strides Ca / Cb
int gdt_k_concat(const void* a, const void* b, void* y, int f32, long NP, int Ca, int ca, int Cb, int cb, int C, int relu_a, hipStream_t st);
int gdt_k_gem_l2n(const void* x, int f32, float* pooled, float* out, int N, int HW, int D, float p, float eps_gem, float eps_l2,
                  hipStream_t st);
int gdt_k_gem_l2n_nchw(const float* x, float* pooled, float* out, int N, int D, int HW, float p, float eps_gem, float eps_l2, hipStream_t st);
int gdt_k_l2n_rows(const float* x, float* y, int N, int D, float eps, hipStream_t st);
int gdt_k_ms_aggregate(const float* x, float* y, int S, int N, int D, float msp, hipStream_t st);
int gdt_k_whiten(const float* P, const float* m, const float* v, float* tmp, float* out, int N, int D, int dims,
                 hipStream_t st);
int gdt_k_whiten_f64(const double* P, const double* m, const double* v, double* tmp, double* out, int N, int D, int dims, hipStream_t st);
int gdt_k_unpack_output(const void* x, int f32, float* y, const float* bias, int N, int HW, int C, hipStream_t st);
int gdt_k_rowsplit_combine(const void* P, int f32, const float* bias, float* out, int N, int H, int W, int cp, int cout, int kw,
                           int pad, int reflect, int act, hipStream_t st);
int gdt_k_hed_score(const void* x, int f32, const float* w, float bias, float* score, long NP, int C, hipStream_t st);
int gdt_k_hed_fuse(const float* const* score, const int* h, const int* w, const float* fw, float fb, float* out, int N, int H,
                   int W, int sigmoid, hipStream_t st);
// RCF head: one stage's score map from its 1-3 tensors (x[j] fp16 / fp32 NHWC with C channels, v[j] fp32 [C]); the fusion of the five maps
int gdt_k_rcf_stage_score(const void* const* x, const float* const* v, int nx, int f32, float bias, float* score, long NP, int C, hipStream_t st);
int gdt_k_rcf_fuse(const float* const* score, const int* h, const int* w, const float* const* filt, const int* stride, const int* crop, const float* fw,
                   float fb, float* out, int N, int H, int W, int sigmoid, hipStream_t st);
int gdt_conv_bn(int Cout);

// ---- descriptor head (pool_head.hip) ----
enum { GDT_POOL_MAX = 0, GDT_POOL_MEAN = 1, GDT_POOL_GEM = 2, GDT_POOL_GEMMP = 3 };      // the `kind` of include/gandtr_hip.h
constexpr int GDT_POOL_MAX_REGIONS = 64;
struct GdtPoolBox { int y0, x0, h, w; };
// the regions of one map size as the pooling kernel takes them (by value): region r = rows [ry0, ry0 + rh) x column band rband[r]; band b = columns
// [bx0, bx0 + bw).  Regions that share their columns share a band.
struct GdtPoolRegions {
    int R, B;
    short ry0[GDT_POOL_MAX_REGIONS], rh[GDT_POOL_MAX_REGIONS], rband[GDT_POOL_MAX_REGIONS];
    short bx0[GDT_POOL_MAX_REGIONS], bw[GDT_POOL_MAX_REGIONS];
};
struct GdtPoolHead {
    int kind = GDT_POOL_GEM; float p = 3.f; const float* p_channels = nullptr; float eps = 1e-6f, eps_l2 = 1e-6f;
    int aggregate = 0;                                      // 0: one vector per image, 1: R-MAC, 2: Rpool (gdt_k_pool_head)
    const float *rw = nullptr, *rb = nullptr, *fw = nullptr, *fb = nullptr;     // regional / final whitening (device, fp32 [D][D] and [D])
    const float* weights = nullptr;                         // attention head: one fp32 weight per pixel [N][H * W], folded into the pooling pass
};
int gdt_pool_grid(int H, int W, int L, std::vector<GdtPoolBox>& boxes);          // the whole map, then the L levels of LF.roipool (host)
int gdt_pool_regions_of(const std::vector<GdtPoolBox>& boxes, GdtPoolRegions& g);
int gdt_k_pool_regions(const void* x, int f32, float* out, int N, int H, int W, int D, int kind, float p, const float* p_channels, float eps,
                       const GdtPoolRegions& g, hipStream_t st, const float* weights = nullptr);     // weights: pools x * weights[n][pixel]
// L2NormAttention (mdir/components/model/layers/attention.py:10-15): out[n][pixel] = sqrt(sum_c x^2 + 1e-10), divided by the image's maximum when
// normalize_max; `partial`: gdt_pixel_attention_partial_floats(N, HW) floats (the workgroups' maxima), unused without normalize_max
size_t gdt_pixel_attention_partial_floats(int N, long HW);
int gdt_k_pixel_attention(const void* x, int f32, int N, long HW, int D, int normalize_max, float* out, float* partial, hipStream_t st);
// The local head (local_head.hip): desc [N][D][HW] = x / (||x||_2 + eps) per position, transposed through LDS; att [N][HW] = sqrt(sum x^2 + 1e-10), divided by the
// image's maximum when normalize_max; `partial`: gdt_local_head_partial_floats floats (the workgroups' maxima), unused without normalize_max.  One read of the map
size_t gdt_local_head_partial_floats(int N, long HW, int D, int f32);
int gdt_k_local_descriptors(const void* x, int f32, int N, long HW, int D, float eps, int normalize_max, float* desc, float* att, float* partial, hipStream_t st);
int gdt_k_linear_rows(const float* a, const float* w, const float* bias, float* out, int rows, int K, int Dout, hipStream_t st);
int gdt_k_region_sum(const float* v, float* y, int N, int R, int D, float eps, int l2n, hipStream_t st);
size_t gdt_pool_head_scratch_floats(int N, int R, int D);
int gdt_k_pool_head(const void* x, int f32, int N, int H, int W, int D, const GdtPoolHead& hd, const GdtPoolRegions& g, float* scratch, float* out,
                    hipStream_t st);

// ---- geometric-median pooling (median_pool.hip) ----
// Weiszfeld's iteration per image: y = scale * x, weights from `prior` (either may be null: ones; fp32 [N][HW]); out fp32 [N][D];
// scratch: gdt_geometric_median_scratch_floats(N, HW, D) floats
int gdt_geometric_median_check(int n, int h, int w, int d, int iterations);       // the argument limits, before any HIP call
size_t gdt_geometric_median_scratch_floats(int N, long HW, int D);
int gdt_k_geometric_median(const void* x, int f32, int N, long HW, int D, int iterations, const float* scale, const float* prior, float* out, float* scratch,
                           hipStream_t st);
// the head with this pooling: median -> l2n -> (whiten -> l2n); scratch: gdt_median_head_scratch_floats(N, HW, D) floats
size_t gdt_median_head_scratch_floats(int N, long HW, int D);
int gdt_k_median_head(const void* x, int f32, int N, long HW, int D, int iterations, const float* scale, const float* fw, const float* fb, float eps_l2,
                      float* scratch, float* out, hipStream_t st);
