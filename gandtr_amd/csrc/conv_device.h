// Device-side building blocks shared by the conv kernel files (conv*.hip): each is written here ONCE.
// The functions are __device__ __forceinline__ and written so that, after inlining, a kernel sees the statements in the order its own copy had them:
// these kernels sit on a register knife edge, and a helper is adopted by a file only when every kernel of the file disassembles exactly as before
// (tools/kernel_diff.py).  A file that keeps local code for one of these items says so in a one-line comment.
#pragma once
#include "gdt_common.h"

typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v6i __attribute__((ext_vector_type(6)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v2i __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ---- s_memtime stamps of the diagnostic builds ----
// A kernel file maps its own build flag onto GDT_STAMP_ON in front of this include (-DGDT_C_STAMP, -DGDT_XEXP_STAMP, -DGDT_BNECK_STAMP); the kernel
// declares the accumulators and the running stamp `st_t`.  Off, the macro is empty.
#ifdef GDT_STAMP_ON
#define GDT_STAMP(acc) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); acc += now_ - st_t; st_t = now_; }
#else
#define GDT_STAMP(acc)
#endif

// ---- global -> LDS DMA, LDS-only barrier ----
#define GDT_GLOBAL_AS __attribute__((address_space(1)))
#define GDT_LDS_AS __attribute__((address_space(3)))
// 16 bytes per lane straight into LDS (global_load_lds_dwordx4: no VGPR round trip); the LDS image is linear per wave instruction
__device__ __forceinline__ void gdt_glds16(const void* gsrc, char* lds_dst) {
    __builtin_amdgcn_global_load_lds((const GDT_GLOBAL_AS void*)gsrc, (GDT_LDS_AS void*)lds_dst, 16, 0, 0);
}
// LDS-only workgroup barrier (no global-memory fence: global stores / loads stay in flight across it)
__device__ __forceinline__ void gdt_lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// ---- workgroup -> tile ----
// Workgroup -> (M tile, N tile).  Workgroups are dealt round-robin over the 8 XCDs (observed, MI355X_MICROARCH.md), each
// with a private L2.  Every XCD therefore gets ONE contiguous span of M tiles: spatially adjacent tiles (which share input
// rows through the kernel taps / halos) and the N tiles of one M tile (which share the whole A operand) meet in the same L2.
// With tiles interleaved over the XCDs instead, the 7x1 head conv of the generator fetched its 537 MB input 6.7 times
// (FETCH_SIZE 3.6 GB per launch).  Placement only affects speed, never results.  Grid size: gdt_grid_for_tiles().
__device__ __forceinline__ bool gdt_tile_of_block(int b, int ntm, int ntn, int& tile_m, int& tile_n) {
    const int mchunk = (ntm + 7) >> 3;
    const int xcd = b & 7, j = b >> 3;
    tile_n = j % ntn;
    const int lm = j / ntn;
    tile_m = xcd * mchunk + lm;
    return lm < mchunk && tile_m < ntm;
}
// Virtual block vb of a persistent kernel's tile walk (vb = workgroup, + grid size, ...; `vblocks` of them): its tile, or valid = false
// with tile (0, 0) -- the walk goes on fetching for a "next tile" that does not exist, so that its loads stay unconditional.
struct GdtTile { int tile_m, tile_n; bool valid; };
__device__ __forceinline__ GdtTile gdt_tile_at(int vb, int vblocks, int ntm, int ntn) {
    GdtTile t;
    t.valid = vb < vblocks && gdt_tile_of_block(vb, ntm, ntn, t.tile_m, t.tile_n);
    if (!t.valid) { t.tile_m = 0; t.tile_n = 0; }
    return t;
}
// ... of the patch kernels: M tile = patch of PH rows x 16 columns, `tpi` patches per image in rows of `tiles_x`; (y0, x0) = its first pixel in image n
struct GdtPatch { int n, y0, x0, tile_m, tile_n; bool valid; };
__device__ __forceinline__ GdtPatch gdt_patch_at(int vb, int vblocks, int ntm, int ntn, int tpi, int tiles_x, int PH) {
    GdtPatch t;
    t.valid = vb < vblocks && gdt_tile_of_block(vb, ntm, ntn, t.tile_m, t.tile_n);
    if (!t.valid) { t.tile_m = 0; t.tile_n = 0; }
    t.n = t.tile_m / tpi;
    const int tr = t.tile_m - t.n * tpi;
    t.y0 = (tr / tiles_x) * PH; t.x0 = (tr % tiles_x) << 4;
    return t;
}

// ---- halo addressing ----
// row h of a halo of HW columns -> (hy, hx) = (h / HW, h % HW) by multiply-shift, exact for h < 2^11
template <int HW>
__device__ __forceinline__ void gdt_halo_yx(int h, int& hy, int& hx) {
    constexpr int MAGIC = 65536 / HW + 1;            // 3641 (18 columns), 3856 (17)
    static_assert((MAGIC * HW - 65536) * 2048 < 65536, "multiply-shift division by the halo width");
    hy = (h * MAGIC) >> 16; hx = h - hy * HW;
}
// One loader round of the (PH + 2) x HW halo of a PH x 16 patch, 64-channel chunk `chunk`, taken from `d.in` (chunks 0 .. nca - 1) or from `d.in2` (the rest): the
// channel concatenation of the two tensors is never materialised (conv4x4t_halo.hip, conv3x3_cat_halo.hip).  Round r stages halo rows r * RPR .. + RPR - 1 of the
// HROWS (padded to HROWS_PAD) into `stage_base`, eight lanes per row (one 16-byte channel group each); the zero ring, ragged edges and pad rows read `d.zeros`,
// and the swizzle chunk' = chunk ^ ((halo column >> 1) & 7) is applied to the SOURCE channel group (conv3x3_halo.hip).  (y0 - 1, x0 - 1) = halo position (0, 0).
template <int HW, int HROWS, int HROWS_PAD, int RPR>
__device__ __forceinline__ void gdt_stage_halo_cat(const ConvLaunch& d, char* stage_base, int n, int y0, int x0, int nca, int chunk, int r, int wave, int lane, int lrow) {
    if (r * RPR + wave * 8 >= HROWS_PAD) return;               // wave-uniform: rows beyond the padded halo
    const int h = r * RPR + lrow;
    int hy, hx;
    gdt_halo_yx<HW>(h, hy, hx);
    const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
    const bool ok = (h < HROWS) & ((unsigned)iy < (unsigned)d.H) & ((unsigned)ix < (unsigned)d.W);      // zero ring, ragged edges, pad rows: zeros
    const int q = (lane & 7) ^ ((hx >> 1) & 7);
    const long pix = ((long)n * d.H + (ok ? iy : 0)) * d.W + (ok ? ix : 0);
    const bool second = chunk >= nca;                          // (wave-uniform)
    const f16* base = second ? d.in2 : d.in;
    const int cs = second ? d.in2_cin : d.Cin, cc = second ? chunk - nca : chunk;
    const f16* src = base + (pix * cs + (cc * 8 + q) * 8);
    gdt_glds16(ok ? src : d.zeros, stage_base + (r * RPR + wave * 8) * 128);
}
// Input coordinate (iy, ix) of an H x W image under reflect padding -> (ry, rx): BOTH reflections first, then (GDT_REFLECT_CLAMP) both clamps.  In
// bounds the reflection is the identity; the clamp makes the address valid for any coordinate (zero padding, rows past the halo), whose data the
// caller then replaces by zeros.  Macros, not functions: as a function -- two coordinates through references, through an int2, or one coordinate
// per call in this statement order -- every file that was tried compiled to different code (operand orders, register counts); the text pasted in
// place is what each kernel had.
#define GDT_REFLECT(iy, ix, H, W, ry, rx)                                                                                            \
    {                                                                                                                                \
        ry = (iy) < 0 ? -(iy) : ((iy) >= (H) ? 2 * (H) - 2 - (iy) : (iy));                                                           \
        rx = (ix) < 0 ? -(ix) : ((ix) >= (W) ? 2 * (W) - 2 - (ix) : (ix));                                                           \
    }
#define GDT_REFLECT_CLAMP(iy, ix, H, W, ry, rx)                                                                                      \
    {                                                                                                                                \
        GDT_REFLECT(iy, ix, H, W, ry, rx)                                                                                            \
        ry = min(max(ry, 0), (H) - 1); rx = min(max(rx, 0), (W) - 1);                                                                \
    }

// ---- the producer's InstanceNorm applied while staging ----
// (mean, rstd) pairs of image n's C channels -> (scale, shift) = (rstd, -mean * rstd) in slot `slot` (512 floats each) of an LDS table;
// thread t of `stride` converts float4s (2 channels) t, t + stride, ...
__device__ __forceinline__ void gdt_stage_norm(float* table, int slot, const float* in_norm, int C, int n, int t, int stride) {
    for (int i = t; i < C / 2; i += stride) {
        const float4 v = *(const float4*)(in_norm + (long)n * C * 2 + i * 4);
        *(float4*)(table + slot * 512 + i * 4) = make_float4(v.y, -v.x * v.y, v.w, -v.z * v.w);
    }
}
// two fp16 lanes of `raw` -> fp16 pair { raw.lo * s0 + h0, raw.hi * s1 + h1 }, each an fp32 fma rounded once to fp16:
// v_fma_mix{lo,hi}_f16 convert the fp16 source, do the fp32 fma and write the fp16 half in ONE instruction (the compiler's own
// choice for the C expression is 2 cvt + packed fma + cvt_pk + register moves: 3x the VALU work in the staging path)
__device__ __forceinline__ unsigned gdt_norm_pair(unsigned raw, float s0, float h0, float s1, float h1) {
    unsigned o;
    asm("v_fma_mixlo_f16 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(o) : "v"(raw), "v"(s0), "v"(h0));
    asm("v_fma_mixhi_f16 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(o) : "v"(raw), "v"(s1), "v"(h1));
    return o;
}
// ... the same with a ReLU floor and a residual: { max(raw.lo * s0 + h0, lo) + res.lo, ... } in fp32, rounded once
__device__ __forceinline__ unsigned gdt_norm_res_pair(unsigned raw, unsigned res, float s0, float h0, float s1, float h1, float lo) {
    float t0, t1;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(t0) : "v"(raw), "v"(s0), "v"(h0));
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(t1) : "v"(raw), "v"(s1), "v"(h1));
    t0 = fmaxf(t0, lo); t1 = fmaxf(t1, lo);
    unsigned o;
    asm("v_fma_mixlo_f16 %0, %1, 1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(o) : "v"(res), "v"(t0));
    asm("v_fma_mixhi_f16 %0, %1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(o) : "v"(res), "v"(t1));
    return o;
}

// ---- "f16c" correction operands, activation side (conv3x3_halo_c.hip, conv3x3_halo_c16.hip, conv_head7.hip) ----
// A staged halo pixel's 64 channels are held 8 per lane by 8 consecutive lanes.  Its scale exponent e is the exponent of max|a| over them,
// clamped to the fp16 normal range: a_hi is stored as fp4(a_hi * 2^(2 - e)) (|a_hi| <= 2^(e + 1): the e2m1 range, 6 saturating),
// a_lo = a - fp16(a) as fp4(a_lo * 2^(13 - e)) (|a_lo| <= 2^(e - 11): <= 4).  The scale follows the data, so the correction holds at
// any activation magnitude and scaling the input by 2^s scales the result by exactly 2^s.  The byte kept per pixel is the E8M0 scale
// of the a_lo operand, 127 + e - 13; the a_hi operand's is 11 more.
constexpr int GDT_C_HI_SCALE_OFF = 11;
__device__ __forceinline__ int gdt_c_pixel_exp(const float (&a)[8]) {
    const float m = fmaxf(fmaxf(fmaxf(fabsf(a[0]), fabsf(a[1])), fmaxf(fabsf(a[2]), fabsf(a[3]))),
                          fmaxf(fmaxf(fabsf(a[4]), fabsf(a[5])), fmaxf(fabsf(a[6]), fabsf(a[7]))));
    int b = __float_as_int(m);                                             // (non-negative: orders as an integer)
    b = max(b, __builtin_amdgcn_mov_dpp(b, 0xB1, 0xF, 0xF, false));     // quad_perm [1, 0, 3, 2]
    b = max(b, __builtin_amdgcn_mov_dpp(b, 0x4E, 0xF, 0xF, false));     // quad_perm [2, 3, 0, 1]
    b = max(b, __builtin_amdgcn_mov_dpp(b, 0x141, 0xF, 0xF, false));    // row_half_mirror: the other quad of the 8 lanes
    return min(max((b >> 23) - 127, -14), 15);
}
__device__ __forceinline__ float gdt_exp2i(int e) { return __int_as_float((e + 127) << 23); }      // 2^e, -126 <= e <= 127
// The split of one channel pair (a0, a1), dword K of the lane's 8 channels: w = fp16 pair (round to nearest even, two per instruction),
// a_lo = a - fp16(a) in ONE v_fma_mix_f32 each (fp16 source read in place), both planes quantised to fp4 by the scaled converts (the convert
// divides by its scale operand) into byte K of qlo / qhi, at the pixel's own scale: lo_scale = 2^(e - 13), hi_scale = 2^(e - 2).
// K is a template argument because the converts take the byte select as a literal.
__device__ __forceinline__ unsigned gdt_pk_f16(float a0, float a1) {
    unsigned w;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(w) : "v"(a0), "v"(a1));
    return w;
}
__device__ __forceinline__ void gdt_pk_f16_rest(unsigned w, float a0, float a1, float& l0, float& l1) {      // a - fp16(a)
    asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(l0) : "v"(w), "v"(a0));
    asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(l1) : "v"(w), "v"(a1));
}
template <int K>
__device__ __forceinline__ void gdt_c_quant(unsigned w, float a0, float a1, float lo_scale, float hi_scale, unsigned& qlo, unsigned& qhi) {
    float l0, l1;
    gdt_pk_f16_rest(w, a0, a1, l0, l1);
    qlo = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(qlo, l0, l1, lo_scale, K);
    qhi = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(qhi, __builtin_bit_cast(f16x2, w), hi_scale, K);
}
template <int K>
__device__ __forceinline__ void gdt_c_split(float a0, float a1, float lo_scale, float hi_scale, unsigned& w, unsigned& qlo, unsigned& qhi) {
    w = gdt_pk_f16(a0, a1);
    gdt_c_quant<K>(w, a0, a1, lo_scale, hi_scale, qlo, qhi);
}
