// Device helpers of the Lab colour conversions shared by clahe.hip and photometric.hip: OpenCV's float32 COLOR_RGB2LAB / COLOR_LAB2RGB as the direct
// CIE formulas (sRGB D65 matrices, white point (0.950456, 1, 1.088754), thresholds 0.008856 / 7.787 / 903.3, the exact sRGB transfer curve);
// oracle/clahe_oracle.py holds the restatement.  Reference: rgb2normspace / normspace2rgb, mdir/components/data/transform/functional.py:28-36 / :55-63.
#pragma once
#include "gdt_common.h"

// OpenCV evaluates the exact steps (and numpy the oracle) with separately rounded float32 multiplies and adds.  hipcc's default
// -ffp-contract=fast would fuse them -- also through HIP's __fmul_rn / __fadd_rn, which are plain operators compiled under that
// default -- so the exact steps use the local helpers below, compiled with contraction off.
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }

#pragma clang fp contract(fast)      // everything that is not written with the helpers above may fuse

struct LabParams {
    float in_scale[3], in_shift[3];             // rgb = x * in_scale + in_shift
    float out_mean[3], out_std[3];              // y = (rgb - out_mean) * out_std   (out_std = 1 / std)
    float fwd[9], inv[9];                       // RGB -> XYZ / white, XYZ * white -> RGB (row-major)
};

__device__ __forceinline__ float fast_pow(float x, float e) { return __builtin_amdgcn_exp2f(e * __builtin_amdgcn_logf(x)); }

__device__ __forceinline__ float srgb_to_linear(float c) {
    c = fminf(fmaxf(c, 0.f), 1.f);
    return c <= 0.04045f ? c * (1.0f / 12.92f) : fast_pow((c + 0.055f) * (1.0f / 1.055f), 2.4f);
}
__device__ __forceinline__ float linear_to_srgb(float c) {
    c = fminf(fmaxf(c, 0.f), 1.f);
    return c <= 0.0031308f ? c * 12.92f : fast_pow(c, 1.0f / 2.4f) * 1.055f - 0.055f;
}
__device__ __forceinline__ float lab_f(float v) { return v > 0.008856f ? fast_pow(v, 1.0f / 3.0f) : 7.787f * v + (16.0f / 116.0f); }

// L in [0, 100] of one pixel: the input affine, the sRGB curve, the Y row of the matrix and one cube root, in separately rounded steps.  The ONE
// statement of the lightness: the 8-bit plane of CLAHE, the lightness plane and the fused photometric kernels all go through it.
__device__ __forceinline__ float lab_lightness100(float r, float g, float b, const LabParams& p) {
    const float lr = srgb_to_linear(add_rn(mul_rn(r, p.in_scale[0]), p.in_shift[0]));
    const float lg = srgb_to_linear(add_rn(mul_rn(g, p.in_scale[1]), p.in_shift[1]));
    const float lb = srgb_to_linear(add_rn(mul_rn(b, p.in_scale[2]), p.in_shift[2]));
    const float y = add_rn(add_rn(mul_rn(p.fwd[3], lr), mul_rn(p.fwd[4], lg)), mul_rn(p.fwd[5], lb));
    return y > 0.008856f ? sub_rn(mul_rn(116.0f, lab_f(y)), 16.0f) : mul_rn(903.3f, y);
}
// normalised lightness L / 100, functional.py:35
__device__ __forceinline__ float lab_lightness_norm(float r, float g, float b, const LabParams& p) { return div_rn(lab_lightness100(r, g, b, p), 100.0f); }
// 8-bit lightness: (L / 100 * 255) truncated, functional.py:148
__device__ __forceinline__ unsigned lightness_u8(float r, float g, float b, const LabParams& p) {
    const float q = mul_rn(div_rn(lab_lightness100(r, g, b, p), 100.0f), 255.0f);
    return (unsigned)min(max((int)q, 0), 255);
}

// a / 500 and b / 200 of one pixel.  Nothing here has to be bit-exact, so the arithmetic may fuse.
__device__ __forceinline__ void lab_chroma(const float c[3], const LabParams& p, float& a500, float& b200) {
    float lin[3], f[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) lin[ch] = srgb_to_linear(c[ch] * p.in_scale[ch] + p.in_shift[ch]);
#pragma unroll
    for (int i = 0; i < 3; ++i) f[i] = lab_f(p.fwd[3 * i] * lin[0] + p.fwd[3 * i + 1] * lin[1] + p.fwd[3 * i + 2] * lin[2]);
    // (the reference's (a + 128) / 255 * 255 - 128 round trip between the conversions, functional.py:36,60, is the identity up to
    // 1e-5 in a / b and is not replayed; constant divisions are reciprocal multiplies -- this half is compared with a tolerance)
    a500 = f[0] - f[1];
    b200 = f[1] - f[2];
}

// Lab (L in [0, 100], a / 500, b / 200) -> RGB -> the output affine
__device__ __forceinline__ void lab_to_rgb(float L, float a500, float b200, const LabParams& p, float out[3]) {
    const float fth = 7.787f * 0.008856f + 16.0f / 116.0f;
    float yv, fy;
    if (L <= 0.008856f * 903.3f) { yv = L * (1.0f / 903.3f); fy = 7.787f * yv + 16.0f / 116.0f; }
    else { fy = (L + 16.0f) * (1.0f / 116.0f); yv = fy * fy * fy; }
    const float fx = a500 + fy, fz = fy - b200;
    const float xv = fx <= fth ? (fx - 16.0f / 116.0f) * (1.0f / 7.787f) : fx * fx * fx;
    const float zv = fz <= fth ? (fz - 16.0f / 116.0f) * (1.0f / 7.787f) : fz * fz * fz;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float rgb = linear_to_srgb(p.inv[3 * ch] * xv + p.inv[3 * ch + 1] * yv + p.inv[3 * ch + 2] * zv);
        out[ch] = (rgb - p.out_mean[ch]) * p.out_std[ch];       // out_std holds 1 / std
    }
}

inline void lab_fill_matrices(LabParams& p) {
    // OpenCV color_lab.cpp: sRGB D65 primaries and white point
    static const double rgb2xyz[9] = {0.412453, 0.357580, 0.180423, 0.212671, 0.715160, 0.072169, 0.019334, 0.119193, 0.950227};
    static const double xyz2rgb[9] = {3.240479, -1.53715, -0.498535, -0.969256, 1.875991, 0.041556, 0.055648, -0.204043, 1.057311};
    static const double white[3] = {0.950456, 1.0, 1.088754};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            p.fwd[3 * i + j] = (float)(rgb2xyz[3 * i + j] / white[i]);
            p.inv[3 * i + j] = (float)(xyz2rgb[3 * i + j] * white[j]);
        }
}

// the four host float[3] affines of an entry point (NULL = identity) into the kernel's parameter block; false when a std is zero
inline bool lab_fill_affines(LabParams& p, const float* in_scale, const float* in_shift, const float* out_mean, const float* out_std) {
    for (int c = 0; c < 3; ++c) {
        p.in_scale[c] = in_scale ? in_scale[c] : 1.f;
        p.in_shift[c] = in_shift ? in_shift[c] : 0.f;
        p.out_mean[c] = out_mean ? out_mean[c] : 0.f;
        if (out_std && out_std[c] == 0.f) return false;
        p.out_std[c] = out_std ? 1.f / out_std[c] : 1.f;
    }
    lab_fill_matrices(p);
    return true;
}

}  // namespace
