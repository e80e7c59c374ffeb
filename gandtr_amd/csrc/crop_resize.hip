// Batched crop + bilinear resize + normalise of decoded 8-bit RGB images (the GAN scenarios' `scalecrop` / `centerscalecrop` / `center_crop` /
// `square_crop` / `mirror` followed by `totensor | normalize`): gdt_crop_resize_u8_batch (include/gandtr_hip.h).
//
// Reference: RandomScaleCrop._crop_downscale = cv2.resize(pic[y0:y1, x0:x1], (ow, oh)) on the float32 [0, 1] image (augmentation_transforms.py:136-144),
// i.e. INTER_LINEAR's float path.  Per axis, n_in = crop extent, n_out = output extent: scale = n_in / (double) n_out; output index d reads
// f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s, clamped to the CROP BOX (s < 0: s = 0, f = 0; s >= n_in - 1: s = n_in - 1, f = 0), taps s and
// min(s + 1, n_in - 1) with the float weights 1.f - f and f; horizontal blend first, then the vertical one, in fp32.
//
// The float32 cast of the coordinate is part of the reference's result, so the tap tables are built HERE ON THE HOST in doubles exactly as above (one
// entry per output column and per output row of every item; neighbours with the same geometry share a table) and uploaded behind the item descriptors in
// one copy; the kernel only blends.  Entries hold ABSOLUTE source columns / rows of the whole image, so the crop offset and both flips are folded into the
// tables and the kernel knows nothing of them:
// flip_src reverses the source index inside the box, flip_dst hands output column d the entry of column out_w - 1 - d.  A box of the output's size gives
// identity tables (f = 0 everywhere): v * 1.f + v' * 0.f = v, the kernel is then a crop + convert, bit-identical to ((u8 / 255.f) - mean) / std.
//
// Kernel: one launch for the list (blockIdx.z = item).  A lane owns four consecutive output pixels of a row: 2 x 2 taps x 3 byte loads each (the row start
// x0 * 3 is arbitrarily aligned: byte loads only), one 16-byte store per colour plane (scalar stores for a row tail, a width that is no multiple of 4 or a
// destination that is not 16-byte aligned).  A wave covers 256 output columns of one row, so its source bytes are one contiguous run of a row pair.  No LDS.
#include "gdt_common.h"
#include "../../include/gandtr_hip.h"
#include <math.h>
#include <vector>

namespace {

struct CropTap { int i0, i1; float f; int pad; };              // source index of the two taps (absolute in the image), weight of the second
static_assert(sizeof(CropTap) == 16, "one 16-byte load per entry");

struct CropDev {
    const unsigned char* src;          // whole image, [h][w][3]
    float* dst;                        // [3][oh][ow]
    const CropTap* xt;                 // [ow]
    const CropTap* yt;                 // [oh]
    int w;                             // pixels per source row
    int vec;                           // 1: ow % 4 == 0 and dst 16-byte aligned -> float4 stores
};

constexpr size_t ALIGN = 256;

__global__ __launch_bounds__(256) void crop_resize3_kernel(const CropDev* __restrict__ items, int ow, int oh, float m0, float m1, float m2, float s0,
                                                            float s1, float s2) {
    const CropDev it = items[blockIdx.z];
    const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= ow || y >= oh) return;
    const CropTap ty = it.yt[y];
    const unsigned char* r0 = it.src + (size_t)ty.i0 * it.w * 3;
    const unsigned char* r1 = it.src + (size_t)ty.i1 * it.w * 3;
    const float wy1 = ty.f, wy0 = 1.f - ty.f;
    const int nx = min(4, ow - x);
    const float mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
    float o[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const CropTap tx = it.xt[min(x + j, ow - 1)];           // (a tail lane recomputes the row's last pixel and does not store it)
        const float wx1 = tx.f, wx0 = 1.f - tx.f;
        const unsigned char *a0 = r0 + (size_t)tx.i0 * 3, *a1 = r0 + (size_t)tx.i1 * 3, *b0 = r1 + (size_t)tx.i0 * 3, *b1 = r1 + (size_t)tx.i1 * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // unfused on purpose: the reference rounds every product and sum (hresize, then vresize)
            const float top = __fadd_rn(__fmul_rn((float)a0[c] / 255.0f, wx0), __fmul_rn((float)a1[c] / 255.0f, wx1));
            const float bot = __fadd_rn(__fmul_rn((float)b0[c] / 255.0f, wx0), __fmul_rn((float)b1[c] / 255.0f, wx1));
            const float v = __fadd_rn(__fmul_rn(top, wy0), __fmul_rn(bot, wy1));
            o[c][j] = (v - mean[c]) / stdv[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* d = it.dst + ((size_t)c * oh + y) * ow + x;
        if (it.vec) {
            *(f32x4*)d = f32x4{o[c][0], o[c][1], o[c][2], o[c][3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nx) d[j] = o[c][j];
        }
    }
}

// cv2's INTER_LINEAR float path for one axis: output index d of n_out over a source extent n_in -> first tap (inside the extent) and second weight
void linear_tap(int d, int n_in, int n_out, int& s, float& f) {
    const double scale = (double)n_in / (double)n_out;
    f = (float)((d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= n_in - 1) { s = n_in - 1; f = 0.f; }
}

size_t align_up(size_t v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }
size_t desc_bytes(int n) { return align_up((size_t)n * sizeof(CropDev)); }
size_t total_bytes(int n, int ow, int oh) { return ALIGN + desc_bytes(n) + (size_t)n * ((size_t)ow + oh) * sizeof(CropTap); }

int check_shape(int n, int out_w, int out_h) {
    GDT_REQUIRE(n >= 1 && n <= 65535, "crop_resize: 1..65535 items");
    GDT_REQUIRE(out_w >= 1 && out_h >= 1 && out_w <= (1 << 16) && out_h <= (1 << 16), "crop_resize: output extents 1..65536");
    return GDT_OK;
}

}  // namespace

extern "C" {

int gdt_crop_resize_workspace_bytes(int n, int out_w, int out_h, size_t* bytes) {
    GDT_REQUIRE(bytes != nullptr, "bytes");
    GDT_CHECK(check_shape(n, out_w, out_h));
    *bytes = total_bytes(n, out_w, out_h);
    return GDT_OK;
}

int gdt_crop_resize_u8_batch(const gdt_crop_item* items, int n, int out_w, int out_h, const float* mean, const float* std, void* workspace,
                             size_t workspace_bytes, void* stream) {
    GDT_CHECK(check_shape(n, out_w, out_h));
    GDT_REQUIRE(items != nullptr, "crop_resize: null item list");
    for (int i = 0; i < n; ++i) {
        const gdt_crop_item& it = items[i];
        GDT_REQUIRE(it.src != nullptr && it.dst_chw != nullptr, "crop_resize: null buffer");
        GDT_REQUIRE(it.h >= 1 && it.w >= 1, "crop_resize: empty image");
        GDT_REQUIRE(it.cw >= 1 && it.ch >= 1, "crop_resize: empty crop box");
        GDT_REQUIRE(it.x0 >= 0 && it.y0 >= 0 && it.x0 <= it.w - it.cw && it.y0 <= it.h - it.ch, "crop_resize: crop box outside the image");
        GDT_REQUIRE(((uintptr_t)it.dst_chw & 3) == 0, "crop_resize: unaligned fp32 output");
    }
    GDT_REQUIRE(workspace != nullptr, "crop_resize: null workspace");
    if (std) for (int c = 0; c < 3; ++c) GDT_REQUIRE(std[c] != 0.f, "crop_resize: zero std");
    if (workspace_bytes < total_bytes(n, out_w, out_h)) { gdt_set_error("crop_resize: workspace too small"); return GDT_ERR_WORKSPACE; }

    // descriptors, then the tap tables; every index below is inside the item's box by construction.  An item whose column (row) geometry equals its
    // predecessor's -- the two pics of a pair share one box -- points at the predecessor's table instead of building and uploading a second one.
    // The staging buffer outlives the call (the upload below is asynchronous for the caller's stream) and is reused by this thread's next call.
    char* ws = (char*)(((uintptr_t)workspace + ALIGN - 1) / ALIGN * ALIGN);
    static thread_local std::vector<char> host;
    host.resize(desc_bytes(n) + (size_t)n * ((size_t)out_w + out_h) * sizeof(CropTap));
    CropDev* desc = (CropDev*)host.data();
    CropTap* taps = (CropTap*)(host.data() + desc_bytes(n));
    const CropTap* dev_taps = (const CropTap*)(ws + desc_bytes(n));
    size_t used = 0;                                            // entries written so far
    for (int i = 0; i < n; ++i) {
        const gdt_crop_item& it = items[i];
        const gdt_crop_item* prev = i ? &items[i - 1] : nullptr;
        if (prev && prev->x0 == it.x0 && prev->cw == it.cw && !prev->flip_src == !it.flip_src && !prev->flip_dst == !it.flip_dst) {
            desc[i].xt = desc[i - 1].xt;
        } else {
            CropTap* xt = taps + used;
            for (int d = 0; d < out_w; ++d) {
                int s; float f;
                linear_tap(it.flip_dst ? out_w - 1 - d : d, it.cw, out_w, s, f);
                const int s1 = s + 1 < it.cw ? s + 1 : it.cw - 1;
                xt[d] = CropTap{it.x0 + (it.flip_src ? it.cw - 1 - s : s), it.x0 + (it.flip_src ? it.cw - 1 - s1 : s1), f, 0};
            }
            desc[i].xt = dev_taps + used;
            used += out_w;
        }
        if (prev && prev->y0 == it.y0 && prev->ch == it.ch) {
            desc[i].yt = desc[i - 1].yt;
        } else {
            CropTap* yt = taps + used;
            for (int d = 0; d < out_h; ++d) {
                int s; float f;
                linear_tap(d, it.ch, out_h, s, f);
                yt[d] = CropTap{it.y0 + s, it.y0 + (s + 1 < it.ch ? s + 1 : it.ch - 1), f, 0};
            }
            desc[i].yt = dev_taps + used;
            used += out_h;
        }
        desc[i].src = it.src;
        desc[i].dst = it.dst_chw;
        desc[i].w = it.w;
        desc[i].vec = out_w % 4 == 0 && ((uintptr_t)it.dst_chw & 15) == 0;
    }
    const size_t upload = desc_bytes(n) + used * sizeof(CropTap);
    hipStream_t s = (hipStream_t)stream;
    GDT_CHECK_HIP(hipMemcpyAsync(ws, host.data(), upload, hipMemcpyHostToDevice, s));
    float m[3] = {0, 0, 0}, sd[3] = {1, 1, 1};
    for (int c = 0; c < 3; ++c) { if (mean) m[c] = mean[c]; if (std) sd[c] = std[c]; }
    hipLaunchKernelGGL(crop_resize3_kernel, dim3(((out_w + 3) / 4 + 63) / 64, (out_h + 3) / 4, n), dim3(256), 0, s, (const CropDev*)ws, out_w, out_h, m[0],
                       m[1], m[2], sd[0], sd[1], sd[2]);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

}  // extern "C"
