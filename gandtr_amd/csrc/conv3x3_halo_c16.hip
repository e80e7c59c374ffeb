// 3x3 / stride-1 / pad-1 convolution of the "f16c" precision mode (conv3x3_halo_c.hip explains the arithmetic: fp32 NHWC activations,
// a*w ~= fp16(a)*fp16(w) on the fp16 MFMA + one block-scaled fp4 x fp6 MFMA that carries both rounding residuals) on the 16 x 16 MFMA SHAPES:
//     v_mfma_f32_16x16x32_f16 (two per 64 k-values)  +  v_mfma_scale_f32_16x16x128_f8f6f4 (one per 64 k-values, four 32-wide K blocks:
//     [a_lo | a_hi | a_lo' | a_hi']_fp4 . [w_hi | w_lo | w_hi' | w_lo']_fp6 for the two halves of the 64 k-values).
//
// Why a second kernel for the same layer (ResnetBlock convs of the generator, p2p_networks.py:480-494): the chip runs this kernel against its
// power governor, not against its issue slots -- whatever the loop does, the socket sits at ~1.15 kW and the clock settles where that
// power is reached (conv3x3_halo_c: 63 % matrix-pipe busy at 1.94 GHz; a tighter loop returns as a lower clock).  Per FLOP the 16 x 16 x 32
// shape reads and writes HALF the accumulator registers of 32 x 32 x 16 (K = 32 per accumulation instead of 16) and the governor lets it
// clock higher: profiles/experiments/mfma_shape_probe.hip, this instruction mix, operands in registers: 1194 vs 1045 TFLOP/s
// (1.79 vs 1.56 GHz), fp16 only 1860 vs 1600.  Cycles per FLOP are the same for both shapes.
//
// Structure (shared with conv3x3_halo_c.hip: persistent workgroups walking an XCD-chunked tile list, 16 x 16 output patch x 256 output
// channels, 18 x 18 fp32 halo per 64-channel chunk read through registers, InstanceNorm (+ReLU / + residual / + write-back) of the producer
// applied in fp32 while staging (MODE bits), split into an fp16 plane (128-byte rows) and an fp4 plane (64-byte rows) in LDS, two stages;
// weights streamed L2 -> registers in fragment order; swapped MFMA operands D[cout][pixel]):
//   * 4 waves, one per SIMD, 1 x 4: a wave owns all 256 pixels x 64 output channels = 16 pixel blocks (the patch's rows) x 4 channel blocks
//     of 16 x 16, 256 accumulator registers;
//   * pixel <-> MFMA column: lane column n holds pixel x = PIX(n) of its patch row (even x on columns 0-3 and 12-15, odd x on 4-11), so that
//     the 16 lanes a ds_read_b128 serves per cycle read eight even and eight odd pixels: with the row swizzles of the planes every fragment read
//     is bank-conflict-free for all three tap columns (with the identity map two of the three collide two-way);
//   * an fp16 activation fragment (one patch row x 32 channels) feeds the wave's 4 channel blocks, a weight fragment (16 channels x 32 k) the
//     16 pixel blocks: the same operand bytes per FLOP as the 32 x 32 kernel's 1 x 4 layout;
//   * per tap and chunk: 2 x 64 fp16 MFMAs, then 64 MX MFMAs whose activation operand is ONE 16-byte read (a pixel's whole fp4 row);
//   * epilogue straight from the accumulators: a lane holds 4 consecutive output channels of one pixel per block = one 16-byte store; the
//     four lane groups of a pixel make 64 contiguous bytes per instruction, two blocks a 128-byte line.  No LDS transpose, no epilogue
//     patches.  InstanceNorm statistics: per lane over the 16 patch rows, then a DPP rotate butterfly over the 16 pixel lanes: fixed
//     order, deterministic; one 256-row record per wave (the second 128-row record of the slab layout is written as zeros).
// Full 16 x 16 patches and 256-column tiles only (the generator's resblocks at any batch that fills the chip); everything else stays on
// conv3x3_halo_c.hip.
#include <cstdio>
#include <cstdlib>

#include <vector>

#ifdef GDT_C_STAMP                 // diagnostic build: GDT_STAMP is live
#define GDT_STAMP_ON
#endif
#include "conv_device.h"

#ifndef GDT_C16_ABL
#define GDT_C16_ABL 0           // timing-only ablations: 1 no halo staging   2 no MX MFMAs / loads   4 no fp16 weight re-loads   8 no fp4 fragment re-loads   16 no MX weight re-loads   64 MX weights fetched into an unused set   128 every weight fetch from one hot 7 KB window   256 no output stores
#endif

namespace {

constexpr int ROWB = 128;          // bytes per row of the fp16 plane (64 halves of K)
constexpr int QROWB = 64;          // bytes per row of the fp4 plane
constexpr int HW_ = 18, HROWS = HW_ * HW_, HROWS_PAD = 328;
constexpr int A_BYTES = HROWS_PAD * ROWB;                  // 41984
constexpr int Q_BYTES = HROWS_PAD * QROWB;                 // 20992
constexpr int STAGE_BYTES = A_BYTES + Q_BYTES;             // 62976
constexpr int NORM_BYTES = 4096 + 64;
constexpr int E_OFF = 2 * STAGE_BYTES + NORM_BYTES;        // scale bytes of the fp4 plane: one per halo row and stage (gdt_c_pixel_exp)
constexpr size_t LDS_BYTES = 2 * (size_t)STAGE_BYTES + NORM_BYTES + 2 * HROWS_PAD;
constexpr int NT = 256, RPR = NT / 8, NR = (HROWS_PAD + RPR - 1) / RPR;      // threads, halo rows per loader round, rounds per chunk (11)
constexpr int NTAP = 9, SLOTS = NTAP * 3;      // per tap: two fp16 half-steps + the MX run
constexpr int SPR = 2;                         // loader round r: loaded at slot SPR * r, written to LDS at slot SPR * (r + SDIST)
#ifndef GDT_C16_SDIST
#define GDT_C16_SDIST 2
#endif
constexpr int SDIST = GDT_C16_SDIST;           // rounds in flight per thread: a round is consumed SDIST * SPR slots (~2400 cycles at 2) after its loads --
                                               // with one, ~1300 cycles, every round began with a wait for HBM (13-25 k cycles per tile, stamped)
static_assert((NR + SDIST) * SPR <= SLOTS, "halo rounds are spread over the slots of the previous chunk");

// The MFMAs as inline asm with the accumulator tied to an AGPR tuple ("+a"): for the four-pass 16 x 16 shapes the compiler does not tie vdst
// to src2, lets the 64 accumulator tuples wander through the 256 AGPRs -- all of which they occupy -- and moves them through VGPRs and scratch
// around every MFMA (first build: 1580 v_accvgpr_read + 1520 v_accvgpr_write + 250 scratch operations per chunk).  Operands arrive from LDS /
// global loads (the compiler's s_waitcnt covers asm operands); the accumulators are read by VALU only behind the tile-end barrier, far
// beyond the MFMA -> VALU wait states nothing pads inside asm.
// Volatile and with a memory clobber: each keeps its place between the sched_barrier fences, ahead of the (volatile) pins of the work laid
// behind it and ahead of the loads and LDS reads laid behind it.
__device__ __forceinline__ void mfma16(f32x4& acc, const f16x8& a, const f16x8& b) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b) : "memory");
}
__device__ __forceinline__ void mfma16_mx(f32x4& acc, const v6i& a6, const v4i& b4, int sa, int sb) {      // A: 32 e2m3 values per lane, B: 32 e2m1
    asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0] cbsz:2 blgp:4" : "+a"(acc) : "v"(a6), "v"(b4), "v"(sa), "v"(sb) : "memory");
}
// max(|a|, |b|, |c|) / max(|a|, |b|) in one instruction each (the C expression canonicalises every pinned input first: two instructions more per
// maximum).  Same value as fmaxf of the absolute values for every input but a signalling NaN, which no kernel of the path produces and which the
// MFMAs would turn into NaN outputs either way.
__device__ __forceinline__ float gdt_max3_abs(float a, float b, float c) {
    float m;
    asm("v_max3_f32 %0, |%1|, |%2|, |%3|" : "=v"(m) : "v"(a), "v"(b), "v"(c));
    return m;
}
__device__ __forceinline__ float gdt_max_abs(float a, float b) {
    float m;
    asm("v_max_f32_e64 %0, |%1|, |%2|" : "=v"(m) : "v"(a), "v"(b));
    return m;
}

// MODE bits: 1 = the producer's InstanceNorm (+ReLU) is applied while staging; 2 = ... plus a residual; 4 = the transformed tensor is written back
template <int MODE>
__global__ __launch_bounds__(NT) void conv3x3_halo_c16_kernel(const ConvLaunch d, const int vblocks) {
    constexpr bool NORM = (MODE & 1) != 0, RES = (MODE & 2) != 0, WB = (MODE & 4) != 0;
    constexpr int RING = 3;                  // ring of fp16 weight fragments: half-step u + RING - 1 is fetched during half-step u
    static_assert(18 % RING == 0, "ring slot of a half-step must not depend on the chunk");
    constexpr int AW = 8, QW = 4;            // activation fragment windows (fp16 plane / fp4 plane): register sets re-loaded AW / QW pixel blocks ahead
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float* __restrict__ inf = (const float*)d.in;
    const float* __restrict__ resf = (const float*)d.in_res;
    float* __restrict__ wbf = (float*)d.in_out;

    const int tiles_x = d.W >> 4, tiles_y = d.H >> 4;
    const int tpi = tiles_x * tiles_y, ntm = d.N * tpi, ntn = d.CoutPad >> 8;
    auto tile_at = [&](int vb) -> GdtPatch { return gdt_patch_at(vb, vblocks, ntm, ntn, tpi, tiles_x, 16); };
    int vb = blockIdx.x;
    GdtPatch cur = tile_at(vb);
    if (!cur.valid) return;

    // ---- halo loader: through registers, branch-free (conv3x3_halo_c.hip)
    const int lrow = tid >> 3;
    const bool refl = d.pad_reflect != 0;
    struct Pend { float4 r0, r1, s0, s1; unsigned goff; bool ok; };
    auto load_piece = [&](const GdtPatch& ta, int chunk, int r) -> Pend {
        int lr = lrow;
        asm volatile("" : "+v"(lr));
        const int h = min(r * RPR + lr, HROWS_PAD - 1);
        int hy, hx;
        gdt_halo_yx<HW_>(h, hy, hx);
        const int q = lane & 7;
        const int iy = ta.y0 - 1 + hy, ix = ta.x0 - 1 + hx;
        const int cbyte = (chunk * 8 + q) * 32;
        int ry, rx;
        GDT_REFLECT_CLAMP(iy, ix, d.H, d.W, ry, rx)
        const bool inb = ((unsigned)iy < (unsigned)d.H) & ((unsigned)ix < (unsigned)d.W);
        Pend p;
        p.goff = (((unsigned)((ta.n * d.H + ry) * d.W + rx) << (d.lc8 + 5)) + cbyte);      // byte offset (< 2^32, checked on the host)
        p.ok = (h < HROWS) & (inb | refl);
        p.r0 = *(const float4*)((const char*)inf + p.goff); p.r1 = *(const float4*)((const char*)inf + p.goff + 16);
        if (RES) { p.s0 = *(const float4*)((const char*)resf + p.goff); p.s1 = *(const float4*)((const char*)resf + p.goff + 16); }
        return p;
    };
    Pend pendv[SDIST];            // main loop: the rounds in flight
    float* nlds = (float*)(smem + 2 * STAGE_BYTES);
    auto stage_norm = [&](const GdtPatch& ta, int slot) {
        gdt_stage_norm(nlds, slot, d.in_norm, d.Cin, ta.n, tid, NT);
    };
    float4 nf[4];
    auto load_nf = [&](int slot, int chunk) {
        if (!NORM) return;
        const float4* np4 = (const float4*)(nlds + slot * 512 + (chunk * 8 + (lane & 7)) * 16);
#pragma unroll
        for (int k = 0; k < 4; ++k) nf[k] = np4[k];
    };
    auto store_piece = [&](int stage_off, int r, const Pend& p) {
        const int row = min(r * RPR + lrow, HROWS_PAD - 1);
        int phy, phx;
        gdt_halo_yx<HW_>(row, phy, phx);
        float a[8] = {p.r0.x, p.r0.y, p.r0.z, p.r0.w, p.r1.x, p.r1.y, p.r1.z, p.r1.w};
        if (NORM) {
            const float lo = d.in_relu ? 0.f : -3.0e38f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 v = nf[k];
                a[2 * k] = fmaxf(fmaf(a[2 * k], v.x, v.y), lo);
                a[2 * k + 1] = fmaxf(fmaf(a[2 * k + 1], v.z, v.w), lo);
            }
            if (RES) {
                a[0] += p.s0.x; a[1] += p.s0.y; a[2] += p.s0.z; a[3] += p.s0.w;
                a[4] += p.s1.x; a[5] += p.s1.y; a[6] += p.s1.z; a[7] += p.s1.w;
            }
        }
        if (WB) {      // every piece stores the value of its clamped source pixel: identical bits from neighbouring patches, no branch
            *(float4*)((char*)wbf + p.goff) = make_float4(a[0], a[1], a[2], a[3]);
            *(float4*)((char*)wbf + p.goff + 16) = make_float4(a[4], a[5], a[6], a[7]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = p.ok ? a[e] : 0.f;
        const int ex = gdt_c_pixel_exp(a);                       // the pixel's scale: the converts divide by it
        const float lo_scale = gdt_exp2i(ex - 13), hi_scale = gdt_exp2i(ex - 2);
        unsigned ou[4], qlo = 0, qhi = 0;
        gdt_c_split<0>(a[0], a[1], lo_scale, hi_scale, ou[0], qlo, qhi);
        gdt_c_split<1>(a[2], a[3], lo_scale, hi_scale, ou[1], qlo, qhi);
        gdt_c_split<2>(a[4], a[5], lo_scale, hi_scale, ou[2], qlo, qhi);
        gdt_c_split<3>(a[6], a[7], lo_scale, hi_scale, ou[3], qlo, qhi);
        const u32x4 ov = {ou[0], ou[1], ou[2], ou[3]};
        const int q = lane & 7;
        // fp16 plane: source chunk q (8 channels) at 16-byte position q ^ key, key = (x >> 1) & 7
        *(f16x8*)(smem + stage_off + row * ROWB + ((q ^ ((phx >> 1) & 7)) << 4)) = __builtin_bit_cast(f16x8, ov);
        // fp4 plane: a row = [lo 0-31][hi 0-31][lo 32-63][hi 32-63], 16-byte position p at p ^ key2, key2 = (x >> 2) & 3; this thread holds
        // channels 8q .. 8q+7: dword q & 3 of the lo / hi part of half q >> 2
        const int key2 = (phx >> 2) & 3;
        const int qo = stage_off + A_BYTES + row * QROWB + ((((q >> 2) << 1) ^ key2) << 4) + ((q & 3) << 2);
        *(unsigned*)(smem + qo) = qlo;
        *(unsigned*)(smem + (qo ^ 16)) = qhi;
        smem[E_OFF + (stage_off ? HROWS_PAD : 0) + row] = (char)(127 + ex - 13);      // (the row's 8 lanes store the same byte)
    };

    // The same work in MICRO-PHASES for the main loop: the MFMAs there are inline asm, which the compiler neither schedules around nor sees as
    // long operations -- left alone it sinks every LDS read to just in front of its MFMA and runs the ~100 staging instructions of a round in one
    // piece.  So the loop body is laid out by hand, per MFMA, fenced by sched_barrier: with one wave per SIMD and in-order issue every MFMA
    // but the first of a patch row waits ~12 cycles for the pipe with nothing to issue, so each of the row's four gets a little work behind it:
    // the first the row's vector-memory instruction (a weight load), the second and third one micro-phase of the staging each (stage_micro:
    // <= 3 VALU instructions, or one load / store / LDS write), the fourth the row's LDS reads (the window slot they refill is read by all
    // four MFMAs).  A round spreads over both slots of its pair: 64 micro-phase positions, position mp = 2 * (row of the pair) + g, of which
    // a round uses 47-57; no gap holds 12 instructions, 0.5-0.7 k issue cycles per chunk stay uncovered (tests/test_c16_layout_cpu.py).  A step's
    // weights are loaded ahead of the halo loads consumed after them, a round's loads SDIST rounds ahead of its store, its LDS writes ahead
    // of the chunk barrier.  Predecessor: the row layout (a row's four MFMAs back to back, then its companion work in one piece; 5.4-6.1 k
    // cycles per chunk uncovered, the same output bit for bit); commit `2b4e7c4` holds it.  Measured: DESIGN.md section 4, "per-MFMA layout".
    // Every micro-phase pins its inputs AND its results (empty asm volatile), so that its instructions stay between the two sched_barrier
    // fences around it: pure VALU instructions carry no ordering against the fences when the block is linearised, and the compiler otherwise
    // runs the normalisation right behind the loads -- with the wait for them.  The arithmetic is store_piece's, value for value; what differs
    // is integer bookkeeping with the same result: the scale exponent is carried biased (e + 127), and the reflected coordinate is
    // min(|i|, 2 (H - 1) - |i|) -- |i| reflects i = -1, the other operand i >= H, in bounds the minimum is i itself -- clamped like before.
    float sa[8];
    unsigned sou[4], sqlo = 0, sqhi = 0;
    int sex = 0;                      // the pixel's scale exponent (gdt_c_pixel_exp), biased, and the converts' scales
    float slo_scale = 1.f, shi_scale = 1.f;
    int mh = 0, mt = 0, my = 0, mx = 0, ma = 0, mb = 0;      // load side: halo row, its coordinates
    int wrow = 0, wx = 0, wa = 0, wq = 0;                    // store side: LDS addresses
    float mu = 0.f, ml0 = 0.f, ml1 = 0.f;
    int mbits = 0;
    int gy0 = 0, gx0 = 0;                // first halo pixel of the patch being loaded (set per chunk, in front of its first MFMA)
    int wes = E_OFF + HROWS_PAD;         // scale bytes of the stage being WRITTEN (the other one than `ve`'s), flipped with it (flip_stage)
    auto stage_micro = [&](const GdtPatch& ta, int chunk, int stage_off, int sl, int row, int g) {
        if (GDT_C16_ABL & 1) return;
        const int r = sl / SPR, mp = ((sl % SPR) * 16 + row) * 2 + g;
        const bool st = r >= SDIST && r - SDIST < NR, ld = r < NR;
        Pend& pend = pendv[r % SDIST];      // (the round stored now and the round loaded behind it share a buffer)
        constexpr int P_NORM = 0, P_RES = P_NORM + (NORM ? 8 : 1), P_WB = P_RES + (NORM && RES ? 3 : 0), P_MASK = P_WB + (WB ? 2 : 0), P_MAX = P_MASK + 3,
                      P_DPP = P_MAX + 2, P_EXP = P_DPP + 3, P_SPLIT = P_EXP + 2, P_ADDR = P_SPLIT + 10, P_WRITE = P_ADDR + 7, P_GADDR = P_WRITE + 4,
                      P_LOAD = P_GADDR + 9, P_END = P_LOAD + (RES ? 4 : 2);
        static_assert(P_END <= SPR * 16 * 2, "a round's micro-phases fit the positions of its slot pair");
#define GDT_PIN1(a) asm volatile("" : "+v"(a))
#define GDT_PIN2(a, b) asm volatile("" : "+v"(a), "+v"(b))
#define GDT_PIN3(a, b, c) asm volatile("" : "+v"(a), "+v"(b), "+v"(c))
#define GDT_PIN4(a, b, c, e) asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(e))
        auto f4 = [](float4& v, int i) -> float& { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); };
        auto pr = [&](int e) -> float& { return e < 4 ? f4(pend.r0, e) : f4(pend.r1, e - 4); };
        auto ps = [&](int e) -> float& { return e < 4 ? f4(pend.s0, e) : f4(pend.s1, e - 4); };
        // ---- the round stored now
        if (st && !NORM && mp == P_NORM) {
#pragma unroll
            for (int e = 0; e < 8; ++e) sa[e] = pr(e);
            GDT_PIN4(sa[0], sa[1], sa[2], sa[3]); GDT_PIN4(sa[4], sa[5], sa[6], sa[7]);
        }
        if (st && NORM && mp >= P_NORM && mp < P_NORM + 8) {        // normalise: one channel per micro-phase
            const int e = mp - P_NORM;
            const float lo = d.in_relu ? 0.f : -3.0e38f;
            const float4 v = nf[e >> 1];
            float x = pr(e);
            GDT_PIN1(x);
            x = fmaxf(fmaf(x, (e & 1) ? v.z : v.x, (e & 1) ? v.w : v.y), lo);
            GDT_PIN1(x);
            sa[e] = x;
        }
        if (st && NORM && RES && mp >= P_RES && mp < P_RES + 3) {     // residual: three channels
            const int e = 3 * (mp - P_RES);
            float y0 = ps(e), y1 = ps(e + 1), y2 = ps(e + 2 < 8 ? e + 2 : e);
            if (e + 2 < 8) { GDT_PIN3(sa[e], sa[e + 1], sa[e + 2]); GDT_PIN3(y0, y1, y2); } else { GDT_PIN2(sa[e], sa[e + 1]); GDT_PIN2(y0, y1); }
            sa[e] += y0; sa[e + 1] += y1;
            if (e + 2 < 8) { sa[e + 2] += y2; GDT_PIN3(sa[e], sa[e + 1], sa[e + 2]); } else GDT_PIN2(sa[e], sa[e + 1]);
        }
        if (st && WB && mp == P_WB) {
            GDT_PIN4(sa[0], sa[1], sa[2], sa[3]);
            *(float4*)((char*)wbf + pend.goff) = make_float4(sa[0], sa[1], sa[2], sa[3]);
        }
        if (st && WB && mp == P_WB + 1) {
            GDT_PIN4(sa[4], sa[5], sa[6], sa[7]);
            *(float4*)((char*)wbf + pend.goff + 16) = make_float4(sa[4], sa[5], sa[6], sa[7]);
        }
        if (st && mp >= P_MASK && mp < P_MASK + 3) {                  // rows beyond the halo / zero padding: three channels
            const int e = 3 * (mp - P_MASK);
            if (e + 2 < 8) GDT_PIN3(sa[e], sa[e + 1], sa[e + 2]); else GDT_PIN2(sa[e], sa[e + 1]);
            sa[e] = pend.ok ? sa[e] : 0.f; sa[e + 1] = pend.ok ? sa[e + 1] : 0.f;
            if (e + 2 < 8) { sa[e + 2] = pend.ok ? sa[e + 2] : 0.f; GDT_PIN3(sa[e], sa[e + 1], sa[e + 2]); } else GDT_PIN2(sa[e], sa[e + 1]);
        }
        // gdt_c_pixel_exp in pieces: max |a| over the lane's 8 channels (any order gives the same value), then the three DPP steps one per
        // micro-phase (the MFMA between two of them stands where the DPP wait states would)
        if (st && mp == P_MAX) {
            GDT_PIN4(sa[0], sa[1], sa[2], sa[3]); GDT_PIN1(sa[4]);
            mu = gdt_max3_abs(gdt_max3_abs(sa[0], sa[1], sa[2]), sa[3], sa[4]);
            GDT_PIN1(mu);
        }
        if (st && mp == P_MAX + 1) {
            GDT_PIN4(mu, sa[5], sa[6], sa[7]);
            mu = gdt_max_abs(gdt_max3_abs(mu, sa[5], sa[6]), sa[7]);
            mbits = __float_as_int(mu);
            sqlo = 0; sqhi = 0;
            GDT_PIN3(mbits, sqlo, sqhi);
        }
        if (st && mp >= P_DPP && mp < P_DPP + 3) {
            GDT_PIN1(mbits);
            if (mp == P_DPP) mbits = max(mbits, __builtin_amdgcn_mov_dpp(mbits, 0xB1, 0xF, 0xF, false));         // quad_perm [1, 0, 3, 2]
            if (mp == P_DPP + 1) mbits = max(mbits, __builtin_amdgcn_mov_dpp(mbits, 0x4E, 0xF, 0xF, false));     // quad_perm [2, 3, 0, 1]
            if (mp == P_DPP + 2) mbits = max(mbits, __builtin_amdgcn_mov_dpp(mbits, 0x141, 0xF, 0xF, false));    // row_half_mirror
            GDT_PIN1(mbits);
        }
        if (st && mp == P_EXP) {
            GDT_PIN1(mbits);
            sex = min(max(mbits >> 23, 127 - 14), 127 + 15);      // biased
            GDT_PIN1(sex);
        }
        if (st && mp == P_EXP + 1) {
            GDT_PIN1(sex);
            slo_scale = __int_as_float((sex - 13) << 23); shi_scale = __int_as_float((sex - 2) << 23);
            GDT_PIN2(slo_scale, shi_scale);
        }
        // gdt_c_split of the four channel pairs, two instructions per micro-phase: instruction i of pair K = 0 the fp16 pair, 1 / 2 the two
        // remainders a - fp16(a), 3 / 4 the fp4 converts of the fp16 pair and of the remainders
        if (st && mp >= P_SPLIT && mp < P_SPLIT + 10) {
            GDT_PIN4(sqlo, sqhi, ml0, ml1);
#pragma unroll
            for (int i = 2 * (mp - P_SPLIT); i < 2 * (mp - P_SPLIT) + 2; ++i) {
                const int K = i / 5, w = i - 5 * K;
                GDT_PIN2(sa[2 * K], sa[2 * K + 1]);
                if (w > 0) GDT_PIN1(sou[K]);
                if (w == 0) sou[K] = gdt_pk_f16(sa[2 * K], sa[2 * K + 1]);
                if (w == 1) asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(ml0) : "v"(sou[K]), "v"(sa[2 * K]));
                if (w == 2) asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(ml1) : "v"(sou[K]), "v"(sa[2 * K + 1]));
                if (w == 3) {
                    GDT_PIN1(shi_scale);
                    if (K == 0) sqhi = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(sqhi, __builtin_bit_cast(f16x2, sou[K]), shi_scale, 0);
                    if (K == 1) sqhi = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(sqhi, __builtin_bit_cast(f16x2, sou[K]), shi_scale, 1);
                    if (K == 2) sqhi = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(sqhi, __builtin_bit_cast(f16x2, sou[K]), shi_scale, 2);
                    if (K == 3) sqhi = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(sqhi, __builtin_bit_cast(f16x2, sou[K]), shi_scale, 3);
                }
                if (w == 4) {
                    GDT_PIN1(slo_scale);
                    if (K == 0) sqlo = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(sqlo, ml0, ml1, slo_scale, 0);
                    if (K == 1) sqlo = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(sqlo, ml0, ml1, slo_scale, 1);
                    if (K == 2) sqlo = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(sqlo, ml0, ml1, slo_scale, 2);
                    if (K == 3) sqlo = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(sqlo, ml0, ml1, slo_scale, 3);
                }
                GDT_PIN1(sou[K]);
            }
            GDT_PIN4(sqlo, sqhi, ml0, ml1);
        }
        // the LDS addresses (store_piece explains the planes), then the four writes
        const int q = lane & 7;
        if (st && mp == P_ADDR) {
            int lr = lrow;
            GDT_PIN1(lr);
            wrow = min((r - SDIST) * RPR + lr, HROWS_PAD - 1);
            GDT_PIN1(wrow);
        }
        if (st && mp == P_ADDR + 1) {
            GDT_PIN1(wrow);
            wx = wrow - ((wrow * (65536 / HW_ + 1)) >> 16) * HW_;
            GDT_PIN1(wx);
        }
        if (st && mp == P_ADDR + 2) {
            GDT_PIN1(wx);
            wa = q ^ ((wx >> 1) & 7);
            GDT_PIN1(wa);
        }
        if (st && mp == P_ADDR + 3) {
            GDT_PIN2(wrow, wa);
            wa = stage_off + wrow * ROWB + (wa << 4);
            GDT_PIN1(wa);
        }
        if (st && mp == P_ADDR + 4) {
            GDT_PIN1(wx);
            wx = ((q >> 2) << 1) ^ ((wx >> 2) & 3);
            GDT_PIN1(wx);
        }
        if (st && mp == P_ADDR + 5) {
            GDT_PIN1(wx);
            wq = (wx << 4) + ((q & 3) << 2);
            GDT_PIN1(wq);
        }
        if (st && mp == P_ADDR + 6) {
            GDT_PIN2(wrow, wq);
            wq = stage_off + A_BYTES + wrow * QROWB + wq;
            GDT_PIN1(wq);
        }
        if (st && mp == P_WRITE) {
            GDT_PIN1(wa); GDT_PIN4(sou[0], sou[1], sou[2], sou[3]);
            const u32x4 ov = {sou[0], sou[1], sou[2], sou[3]};
            *(f16x8*)(smem + wa) = __builtin_bit_cast(f16x8, ov);
        }
        if (st && mp == P_WRITE + 1) {
            GDT_PIN2(wq, sqlo);
            *(unsigned*)(smem + wq) = sqlo;
        }
        if (st && mp == P_WRITE + 2) {
            GDT_PIN2(wq, sqhi);
            *(unsigned*)(smem + (wq ^ 16)) = sqhi;
        }
        if (st && mp == P_WRITE + 3) {
            GDT_PIN2(wrow, sex);
            smem[wes + wrow] = (char)(sex - 13);      // (the row's 8 lanes store the same byte)
        }
        // ---- the round loaded now: load_piece's address in pieces, then one load per micro-phase
        if (ld && mp == P_GADDR) {
            int lr = lrow;
            GDT_PIN1(lr);
            mh = min(r * RPR + lr, HROWS_PAD - 1);
            GDT_PIN1(mh);
        }
        if (ld && mp == P_GADDR + 1) {
            GDT_PIN1(mh);
            mt = (mh * (65536 / HW_ + 1)) >> 16;
            GDT_PIN2(mh, mt);
        }
        if (ld && mp == P_GADDR + 2) {
            GDT_PIN2(mh, mt);
            my = gy0 + mt; mx = gx0 + (mh - mt * HW_);
            GDT_PIN3(mh, my, mx);
        }
        if (ld && mp == P_GADDR + 3) {
            GDT_PIN3(mh, my, mx);
            const bool inb = ((unsigned)my < (unsigned)d.H) & ((unsigned)mx < (unsigned)d.W);
            pend.ok = (mh < HROWS) & (inb | refl);
        }
        if (ld && mp == P_GADDR + 4) {
            GDT_PIN1(my);
            ma = max(my, -my); mb = 2 * d.H - 2 - ma;
            GDT_PIN2(ma, mb);
        }
        if (ld && mp == P_GADDR + 5) {
            GDT_PIN2(ma, mb);
            my = min(max(min(ma, mb), 0), d.H - 1);
            GDT_PIN1(my);
        }
        if (ld && mp == P_GADDR + 6) {
            GDT_PIN1(mx);
            ma = max(mx, -mx); mb = 2 * d.W - 2 - ma;
            GDT_PIN2(ma, mb);
        }
        if (ld && mp == P_GADDR + 7) {
            GDT_PIN2(ma, mb);
            mx = min(max(min(ma, mb), 0), d.W - 1);
            GDT_PIN1(mx);
        }
        if (ld && mp == P_GADDR + 8) {
            GDT_PIN2(my, mx);
            pend.goff = (((unsigned)((ta.n * d.H + my) * d.W + mx) << (d.lc8 + 5)) + (chunk * 8 + q) * 32);      // byte offset (< 2^32, checked on the host)
            GDT_PIN1(pend.goff);
        }
        if (ld && mp == P_LOAD) pend.r0 = *(const float4*)((const char*)inf + pend.goff);
        if (ld && mp == P_LOAD + 1) pend.r1 = *(const float4*)((const char*)inf + pend.goff + 16);
        if (ld && RES && mp == P_LOAD + 2) pend.s0 = *(const float4*)((const char*)resf + pend.goff);
        if (ld && RES && mp == P_LOAD + 3) pend.s1 = *(const float4*)((const char*)resf + pend.goff + 16);
#undef GDT_PIN1
#undef GDT_PIN2
#undef GDT_PIN3
#undef GDT_PIN4
    };

    // ---- weights, streamed L2 -> registers in fragment order (net_build.hip pack_mx16): per 64 output channels (a wave's slice)
    //   w_c16 [cout/64][K/32][4 blocks][64 lanes][16 B]: lane (n, g) = W[cout block * 16 + n][k = 32 step + 8 g ..+7]
    //   wmx16_a [cout/64][K/64][4][64][16 B] + wmx16_b [..][8 B] + wmx16_s [..][4 B]: lane (n, blk): 32 e2m3 values + E8M0 scale of
    //   blk 0: fp16(w) of k 0-31, 1: w - fp16(w) of k 0-31, 2 / 3: the same of k 32-63 (of the 64 k-values of a (tap, chunk))
    auto wgrp = [&](int tile_n) -> long { return (long)tile_n * 4 + wave; };
    const int nms = d.Kpad >> 6, cin64 = d.Cin >> 6;
    f16x8 bw[RING][4];
    // MX weights: ONE register set, fetched behind the previous tap's MX run (a second set, fetched a tap ahead, measured no faster -- the weight
    // stream is throughput-, not latency-bound -- and costs 28 registers that the second halo round in flight needs more).  Ablation 64 adds a
    // set that nothing loads in the loop and lets the MFMAs read that one.
    constexpr int BQ_MFMA = (GDT_C16_ABL & 64) ? 1 : 0;        // the set the MX MFMAs read
    v6i bq[1 + BQ_MFMA][4];
    v4i bqs[1 + BQ_MFMA];                                      // E8M0 scales of the four channel blocks (one dwordx4 per lane)
    auto lane_bytes = [&](int per_lane) -> unsigned {
        unsigned v = lane * per_lane;
        asm volatile("" : "+v"(v));
        return v;
    };
    unsigned lo16 = lane_bytes(16), lo8 = lane_bytes(8), lo4 = lane_bytes(4);
    // ONE record of 15 KB per (64 output channels, 64 k-values): [fp16 step 0: 4 KB][fp16 step 1: 4 KB][MX 16-byte parts: 4 KB][MX 8-byte parts: 2 KB]
    // [scales: 1 KB] -- a wave's whole weight stream is one sequential region
    constexpr long WREC = 15360;
    auto load_bw = [&](int rs, int cb, int tile_n, long ks) {        // ks: uniform index of the 32-k step
        // (the record's offset in 32 bits -- gdt_conv_halo_c16_eligible -- : half the scalar address work)
        const char* wb = (const char*)d.w_c16 + (unsigned)(((tile_n * 4 + wave) * nms + (int)(ks >> 1)) * (int)WREC + (int)(ks & 1) * 4096);
        bw[rs][cb] = *(const f16x8*)(wb + lo16 + cb * 1024);
    };
    // MX weights of a (tap, chunk): nine loads, ONE per patch row of MFMAs (a vector-memory instruction takes the wave ~16-20 issue cycles, a patch
    // row's four 16-cycle MFMAs cover one of them; three in a row cost 46 cycles each, measured): part 2 cb = the first 16 bytes of block cb's
    // operand tuple, 2 cb + 1 = its last 8 (both loaded INTO the tuple), part 8 = the four blocks' scales
    auto load_bq_part = [&](int set, int part, int tile_n, long ms) {          // ms: uniform index of the 64-k group
        const long f0 = (GDT_C16_ABL & 128) ? 0 : wgrp(tile_n) * nms + ms;      // (ablation 128: every fetch from the same 7 KB)
        const char* rec = (const char*)d.w_c16 + (unsigned)((int)f0 * (int)WREC);
        const int cb = part >> 1;
        if (part == 8) bqs[set] = *(const v4i*)(rec + 14336 + lo16);
        else if ((part & 1) == 0) {
            const v4i qa = *(const v4i*)(rec + 8192 + lo16 + cb * 1024);
            bq[set][cb] = __builtin_shufflevector(__builtin_shufflevector(qa, qa, 0, 1, 2, 3, -1, -1), bq[set][cb], 0, 1, 2, 3, 10, 11);
        } else {
            const v2i qb = *(const v2i*)(rec + 12288 + lo8 + cb * 512);
            bq[set][cb] = __builtin_shufflevector(bq[set][cb], __builtin_shufflevector(qb, qb, 0, 1, -1, -1, -1, -1), 0, 1, 2, 3, 6, 7);
        }
    };

    // ---- activation fragment addresses: lane (n = lane & 15, g = lane >> 4) holds pixel x = PIX(n) of a patch row, k-slot g
    const int fn = lane & 15, fg = lane >> 4;
    const int px = fn < 4 ? 2 * fn : (fn < 12 ? 2 * (fn - 4) + 1 : 2 * (fn - 8));
    int vt[3], vq[3];
#pragma unroll
    for (int tx = 0; tx < 3; ++tx) {
        vt[tx] = px * ROWB + ((fg ^ (((px + tx) >> 1) & 7)) << 4);
        vq[tx] = A_BYTES + px * QROWB + ((fg ^ (((px + tx) >> 2) & 3)) << 4);
    }
    // fp16 fragment of patch row pb, tap (ty, tx), 32-channel half s of the chunk: chunk position (4 s + g) ^ key = ((g ^ key) ^ 4 s)
    auto a_frag = [&](int pb, int ty, int tx, int s) -> f16x8 {
        return *(const f16x8*)(smem + (vt[tx] ^ (s << 6)) + ((pb + ty) * HW_ + tx) * ROWB);
    };
    auto a_qfrag = [&](int pb, int ty, int tx) -> v4i {
        return *(const v4i*)(smem + vq[tx] + ((pb + ty) * HW_ + tx) * QROWB);
    };
    int ve = E_OFF + px;                 // scale byte of the fp4 fragment's pixel
    auto a_efrag = [&](int pb, int ty, int tx) -> int {
        return *(const unsigned char*)(smem + ve + (pb + ty) * HW_ + tx);
    };
    auto flip_stage = [&](int delta) {
        ve += delta > 0 ? HROWS_PAD : -HROWS_PAD;
        wes -= delta > 0 ? HROWS_PAD : -HROWS_PAD;
#pragma unroll
        for (int k = 0; k < 3; ++k) { vt[k] += delta; vq[k] += delta; }
    };
    // E8M0 scales of the activation side: blocks 0 / 2 carry a_lo, 1 / 3 a_hi, of their pixel (scale byte + this)
    const int a_scale_off = (fg & 1) ? GDT_C_HI_SCALE_OFF : 0;
    constexpr bool AE_PRE = !(GDT_C16_ABL & (2 | 8));      // added a row ahead of the MFMAs, in a gap of its own

    const int nchunks = d.Cin >> 6;
    // ---- prologue
#pragma unroll
    for (int u = 0; u < RING - 1; ++u)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) load_bw(u, cb, cur.tile_n, u);
    if (NORM) {
        stage_norm(cur, 0);
        __syncthreads();
    }
    load_nf(0, 0);
#pragma unroll
    for (int r = 0; r < NR; ++r) store_piece(0, r, load_piece(cur, 0, r));
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SDIST; ++k) pendv[k] = load_piece(cur, 0, 0);      // (placeholder values: overwritten before their first use)

    f16x8 afr[AW];
    v4i aq[QW];
    int ae[QW];                   // their scale bytes
    if (GDT_C16_ABL & 8) { for (int i = 0; i < QW; ++i) { aq[i] = a_qfrag(i, 0, 0); ae[i] = a_efrag(i, 0, 0); } }
    if (GDT_C16_ABL & (16 | 64)) { for (int st = 0; st < 1 + BQ_MFMA; ++st) for (int part = 0; part < 9; ++part) load_bq_part(st, part, cur.tile_n, 0); }
#pragma unroll
    for (int i = 0; i < AW; ++i) afr[i] = a_frag(i, 0, 0, 0);

    int so = 0;                   // LDS offset of the halo stage of the current chunk (0 or STAGE_BYTES)
    int slot = 0;                 // (scale, shift) slot of the current tile
#ifdef GDT_C_STAMP
    unsigned long long st_body = 0, st_cbar = 0, st_tbar = 0, st_epi = 0, st_t = __builtin_amdgcn_s_memtime(), st_n = 0;
    const unsigned long long st_begin = st_t;
#endif
    for (;;) {
        const GdtPatch nxt = tile_at(vb + gridDim.x);
        f32x4 acc[16][4];
#pragma unroll
        for (int i = 0; i < 16; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.f;

        for (int c = 0; c < nchunks; ++c) {
            const bool last = c + 1 == nchunks;
            const bool to_next = last && nxt.valid;
            const GdtPatch sta = to_next ? nxt : cur;
            const int sc = last ? 0 : c + 1, sslot = to_next ? slot ^ 1 : slot;
            if (NORM && nxt.valid && c == nchunks - 2) stage_norm(nxt, slot ^ 1);
            load_nf(sslot, sc);                 // (the table of the next tile was written during the previous chunk, a barrier ago)
            lo16 = lane_bytes(16); lo8 = lane_bytes(8); lo4 = lane_bytes(4);
            // 32-k step index / tile of half-step u of this chunk; u >= 18: the first half-steps of the chunk staged now (after the very
            // last chunk this fetches the first slices again: unconditional loads keep the code straight-line)
            auto ks_of = [&](int u) -> long { return u < 18 ? (long)(((u >> 1) * cin64 + c) * 2 + (u & 1)) : (long)(sc * 2 + (u - 18)); };
            auto tn_of = [&](int u) -> int { return (u >= 18 && last) ? nxt.tile_n : cur.tile_n; };
            gy0 = sta.y0 - 1; gx0 = sta.x0 - 1;       // (the chunk's set-up stays in front of its first MFMA)
            asm volatile("" : "+s"(gy0), "+s"(gx0));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < NTAP; ++t) {
                const int ty = t / 3, tx = t - ty * 3;
                const int nty = (t + 1) / 3, ntx = (t + 1) - nty * 3;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int u = 2 * t + s;
#pragma unroll
                    for (int pb = 0; pb < 16; ++pb) {
                        // behind the row's MFMA cb: (0) its weight load, (1, 2) a staging micro-phase each, (3) its LDS reads
#pragma unroll
                        for (int cb = 0; cb < 4; ++cb) {
                            mfma16(acc[pb][cb], bw[u % RING][cb], afr[pb % AW]);     // D[cout][pixel]
                            if (cb == 0) {       // the row's weight load: at most one per patch row (load_bq_part says why)
                                if (AE_PRE && s == 1 && pb == 15) { asm volatile("" : "+v"(ae[0])); ae[0] += a_scale_off; asm volatile("" : "+v"(ae[0])); }
                                // weights of half-step u + RING - 1 into the ring slot half-step u - 1 has finished with
                                if (!(GDT_C16_ABL & 4) && (pb & 3) == 2) load_bw((u + RING - 1) % RING, pb >> 2, tn_of(u + RING - 1), ks_of(u + RING - 1));
                                // MX weights of this tap (read by the MX run behind the second half-step; the previous run has finished with them):
                                // one part per second patch row of the first half-step, the scales in the second
                                if (!(GDT_C16_ABL & (2 | 16)) && (pb & 1) == 1 && (s == 0 || pb == 1)) load_bq_part(0, s == 0 ? pb >> 1 : 8, cur.tile_n, (long)(t * cin64 + c));
                            } else if (cb < 3) {
                                stage_micro(sta, sc, STAGE_BYTES - so, 3 * t + s, pb, cb - 1);
                            } else {
                                // the window slot just used takes the fragment AW patch rows on: of this half-step or of the next one
                                if (pb + AW < 16) afr[pb % AW] = a_frag(pb + AW, ty, tx, s);
                                else if (s == 0) afr[pb % AW] = a_frag(pb + AW - 16, ty, tx, 1);
                                else if (t < NTAP - 1) afr[pb % AW] = a_frag(pb + AW - 16, nty, ntx, 0);
                                // the first fp4 fragments of the MX run
                                if (!(GDT_C16_ABL & (2 | 8)) && s == 1 && pb >= 16 - QW) { aq[pb - (16 - QW)] = a_qfrag(pb - (16 - QW), ty, tx); ae[pb - (16 - QW)] = a_efrag(pb - (16 - QW), ty, tx); }
                            }
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                }
                // the correction product of the tap's 64 k-values
#pragma unroll
                for (int pb = 0; pb < 16; ++pb) {
#pragma unroll
                    for (int cb = 0; cb < 4; ++cb) {
                        if (!(GDT_C16_ABL & 2)) {
                            mfma16_mx(acc[pb][cb], bq[BQ_MFMA][cb], aq[pb % QW], bqs[BQ_MFMA][cb], AE_PRE ? ae[pb % QW] : ae[pb % QW] + a_scale_off);
                            // (the next row's scale byte gets its a_hi offset here, off the gap of the LDS reads)
                            if (cb == 0 && AE_PRE && pb + 1 < 16) { asm volatile("" : "+v"(ae[(pb + 1) % QW])); ae[(pb + 1) % QW] += a_scale_off; asm volatile("" : "+v"(ae[(pb + 1) % QW])); }
                            if (cb == 3 && !(GDT_C16_ABL & 8) && pb + QW < 16) { aq[pb % QW] = a_qfrag(pb + QW, ty, tx); ae[pb % QW] = a_efrag(pb + QW, ty, tx); }
                        }
                        if (cb == 1 || cb == 2) stage_micro(sta, sc, STAGE_BYTES - so, 3 * t + 2, pb, cb - 1);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            if (GDT_C16_ABL & 64) {       // keep the (unused) loads of the working set alive
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) asm volatile("" :: "v"(bq[0][cb]));
                asm volatile("" :: "v"(bqs[0]));
            }
            GDT_STAMP(st_body)
            if (!last) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                GDT_STAMP(st_cbar)
                flip_stage(STAGE_BYTES - 2 * so);
                so = STAGE_BYTES - so;
#pragma unroll
                for (int i = 0; i < AW; ++i) afr[i] = a_frag(i, 0, 0, 0);
            }
        }

        // ------------------------------------------------------------ tile end: all waves are done with the last halo stage and
        // the next tile's first stage (written during the last chunk) is visible
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        GDT_STAMP(st_tbar)
        // the next tile's first fragments are requested before the epilogue: its stores drain under the next tile's first MFMAs
        const int so_next = STAGE_BYTES - so;

        // ------------------------------------------------------------ epilogue, straight from the accumulators (header)
        {
            float* __restrict__ outp = (float*)d.out;
            const float* __restrict__ resp = (const float*)d.res;
            int lane_e = lane;
            asm volatile("" : "+v"(lane_e));             // (opaque copy: keeps the epilogue's addresses out of the loop's invariant set)
            const int n_e = lane_e & 15, g_e = lane_e >> 4;
            const int x_e = n_e < 4 ? 2 * n_e : (n_e < 12 ? 2 * (n_e - 4) + 1 : 2 * (n_e - 8));
            const int ch = cur.tile_n * 256 + wave * 64 + 4 * g_e;            // + 16 * channel block
            unsigned o = (unsigned)((cur.n * d.H + cur.y0) * d.W + cur.x0 + x_e) * (unsigned)d.Cout + (unsigned)ch;
            const unsigned rowstep = (unsigned)d.W * (unsigned)d.Cout;
            const bool lowhalf = n_e < 8;
            const int n_p = n_e ^ 8, x_p = n_p < 4 ? 2 * n_p : (n_p < 12 ? 2 * (n_p - 4) + 1 : 2 * (n_p - 8));      // the partner lane's pixel
            const unsigned o_p = o + (unsigned)((x_p - x_e) * d.Cout);
            unsigned oA = (lowhalf ? o : o_p) + (lowhalf ? 0u : 16u), oB = (lowhalf ? o_p : o) + (lowhalf ? 0u : 16u);
            const float lo = d.relu ? 0.f : -__builtin_inff();
            constexpr bool EPI_RES = MODE == 0;
            const bool has_res = EPI_RES && resp != nullptr;
            float4 bv[4], s1[4], s2[4];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                bv[cb] = d.bias ? *(const float4*)(d.bias + ch + cb * 16) : make_float4(0.f, 0.f, 0.f, 0.f);
                s1[cb] = make_float4(0.f, 0.f, 0.f, 0.f); s2[cb] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            float4 rcur[4], rnxt[4];
            if (has_res) {
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) rcur[cb] = *(const float4*)(resp + o + cb * 16);
            }
#pragma unroll
            for (int pb = 0; pb < 16; ++pb) {
                asm volatile("" : "+v"(o));
                if (has_res && pb + 1 < 16) {
#pragma unroll
                    for (int cb = 0; cb < 4; ++cb) rnxt[cb] = *(const float4*)(resp + o + rowstep + cb * 16);
                }
                float4 tv[4];
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    const f32x4& a = acc[pb][cb];
                    float4 t = make_float4(a[0] + bv[cb].x, a[1] + bv[cb].y, a[2] + bv[cb].z, a[3] + bv[cb].w);
                    s1[cb].x += t.x; s1[cb].y += t.y; s1[cb].z += t.z; s1[cb].w += t.w;
                    s2[cb].x += t.x * t.x; s2[cb].y += t.y * t.y; s2[cb].z += t.z * t.z; s2[cb].w += t.w * t.w;
                    if (has_res) { t.x += rcur[cb].x; t.y += rcur[cb].y; t.z += rcur[cb].z; t.w += rcur[cb].w; }
                    t.x = fmaxf(t.x, lo); t.y = fmaxf(t.y, lo); t.z = fmaxf(t.z, lo); t.w = fmaxf(t.w, lo);
                    tv[cb] = t;
                }
                if (GDT_C16_ABL & 256) {      // (ablation 256: no output stores)
#pragma unroll
                    for (int cb = 0; cb < 4; ++cb) asm volatile("" :: "v"(tv[cb].x), "v"(tv[cb].y), "v"(tv[cb].z), "v"(tv[cb].w));
                } else {
                    // Whole lines: as the registers stand an instruction writes 64 bytes (the four lane groups) of each of its 16 pixels.  The pixel
                    // lanes n and n ^ 8 swap one block of a pair (2p, 2p + 1): lanes n < 8 hand over block 2p + 1 and receive block 2p of the partner,
                    // so that instruction A writes blocks 2p | 2p + 1 = 128 contiguous bytes of the pixels on lanes 0-7, B those of lanes 8-15.
                    auto ror8 = [](float v) -> float { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false)); };
#pragma unroll
                    for (int p2 = 0; p2 < 2; ++p2) {
                        const float4 t0 = tv[2 * p2], t1 = tv[2 * p2 + 1];
                        // (component-wise selects: a ?: on the float4 structs becomes an indexed scratch array)
                        const float rx = ror8(lowhalf ? t1.x : t0.x), ry = ror8(lowhalf ? t1.y : t0.y), rz = ror8(lowhalf ? t1.z : t0.z), rw = ror8(lowhalf ? t1.w : t0.w);
                        *(float4*)(outp + oA + p2 * 32) = make_float4(lowhalf ? t0.x : rx, lowhalf ? t0.y : ry, lowhalf ? t0.z : rz, lowhalf ? t0.w : rw);
                        *(float4*)(outp + oB + p2 * 32) = make_float4(lowhalf ? rx : t1.x, lowhalf ? ry : t1.y, lowhalf ? rz : t1.z, lowhalf ? rw : t1.w);
                    }
                    oA += rowstep; oB += rowstep;
                }
                o += rowstep;
                if (has_res) {
#pragma unroll
                    for (int cb = 0; cb < 4; ++cb) rcur[cb] = rnxt[cb];
                }
            }
            if (d.stats) {
                // sum over the 16 pixel lanes of a lane group (a DPP row): rotate butterfly, every lane ends with the total, fixed order
                auto merge = [](float v) -> float {
                    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));    // row_ror:8
                    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));    // row_ror:4
                    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false));    // row_ror:2
                    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false));    // row_ror:1
                    return v;
                };
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    s1[cb].x = merge(s1[cb].x); s1[cb].y = merge(s1[cb].y); s1[cb].z = merge(s1[cb].z); s1[cb].w = merge(s1[cb].w);
                    s2[cb].x = merge(s2[cb].x); s2[cb].y = merge(s2[cb].y); s2[cb].z = merge(s2[cb].z); s2[cb].w = merge(s2[cb].w);
                }
                if (n_e == 0) {
                    // slab layout of the 256-row patch kernels: two 128-row records per patch; this wave's 256 rows go into the first one
                    float* dst = d.stats + ((long)(d.stats_tile_base + cur.tile_m * 2) * 2) * d.Cout + ch;
#pragma unroll
                    for (int cb = 0; cb < 4; ++cb) {
                        *(float4*)(dst + cb * 16) = s1[cb];
                        *(float4*)(dst + d.Cout + cb * 16) = s2[cb];
                        *(float4*)(dst + 2l * d.Cout + cb * 16) = make_float4(0.f, 0.f, 0.f, 0.f);
                        *(float4*)(dst + 3l * d.Cout + cb * 16) = make_float4(0.f, 0.f, 0.f, 0.f);
                    }
                }
            }
        }
#ifdef GDT_C_STAMP
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // (diagnostic only: the epilogue's stores are charged to the epilogue)
        GDT_STAMP(st_epi)
        ++st_n;
#endif
        if (!nxt.valid) break;
        cur = nxt; vb += gridDim.x; slot ^= 1;
        flip_stage(so_next - so);
        so = so_next;
#pragma unroll
        for (int i = 0; i < AW; ++i) afr[i] = a_frag(i, 0, 0, 0);
    }
#ifdef GDT_C_STAMP
    if (lane == 0 && d.stamp_out) {
        unsigned long long* o = d.stamp_out + ((long)blockIdx.x * 4 + wave) * 8;
        o[0] = st_body; o[1] = st_cbar; o[2] = st_tbar; o[3] = st_epi; o[4] = __builtin_amdgcn_s_memtime() - st_begin; o[5] = st_n;
    }
#endif
}

template <int MODE>
int launch_c16(const ConvLaunch& d, hipStream_t stream) {
    using K = GdtKernel<conv3x3_halo_c16_kernel<MODE>, (int)LDS_BYTES>;
    int cus = 0;
    GDT_CHECK(K::figure(cus));
    const int vblocks = gdt_grid_for_tiles(d.N * (d.W >> 4) * (d.H >> 4), d.CoutPad >> 8);
    const int grid = vblocks < cus ? vblocks : cus;
#ifdef GDT_C_STAMP
    static unsigned long long* stamp_buf = nullptr;
    static int stamp_calls = 0;
    ConvLaunch ds = d;
    if (!stamp_buf) GDT_CHECK_HIP(hipMalloc((void**)&stamp_buf, (size_t)cus * 4 * 8 * sizeof(unsigned long long)));
    GDT_CHECK_HIP(hipMemsetAsync(stamp_buf, 0, (size_t)cus * 4 * 8 * sizeof(unsigned long long), stream));
    ds.stamp_out = stamp_buf;
    GDT_CHECK(K::launch(grid, NT, stream, ds, vblocks));
    if (++stamp_calls % 200 < 20) {
        GDT_CHECK_HIP(hipStreamSynchronize(stream));
        std::vector<unsigned long long> h((size_t)grid * 4 * 8);
        GDT_CHECK_HIP(hipMemcpy(h.data(), stamp_buf, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        double s[6] = {0, 0, 0, 0, 0, 0};
        for (size_t w = 0; w < (size_t)grid * 4; ++w) for (int k = 0; k < 6; ++k) s[k] += (double)h[w * 8 + k];
        const double nw = grid * 4.0, nt = s[5] / nw;
        fprintf(stderr, "[c stamp] MODE %d FORM 16 BN 256 waves 4: tiles/wave %.1f; per tile: chunk bodies %.0f, chunk barriers %.0f, tile barrier %.0f, epilogue %.0f cycles; total per wave %.0f\n",
                MODE, nt, s[0] / nw / nt, s[1] / nw / nt, s[2] / nw / nt, s[3] / nw / nt, s[4] / nw);
    }
    return GDT_OK;
#else
    return K::launch(grid, NT, stream, d, vblocks);
#endif
}

GDT_KNOB_LATCHED(knob_mode, "GDT_CONV_HALO_C16", 1)          // 0 off

}  // namespace

// Eligible: what conv3x3_halo_c.hip's 256-column form takes (gdt_conv_halo_c_eligible is checked by the caller), restricted to whole 16 x 16
// patches and whole 256-column tiles, with the 16 x 16 fragment-ordered weights present.
bool gdt_conv_halo_c16_eligible(const ConvLaunch& d) {
    if (knob_mode() == 0 || !d.w_c16) return false;
    if (!gdt_conv_halo_c_eligible(d) || gdt_conv_halo_c_columns(d) != 256) return false;
    if ((d.H & 15) || (d.W & 15) || d.Cout != d.CoutPad || (d.Cout & 255)) return false;
    if (d.res && d.in_norm) return false;
    if ((unsigned long long)(d.CoutPad >> 6) * (unsigned long long)(d.Kpad >> 6) * 15360ull >= (1ull << 32)) return false;      // weight records are addressed in 32 bits (WREC)
    return true;
}

// every fold mode is instantiated here
int gdt_launch_conv_halo_c16(const ConvLaunch& d, hipStream_t stream) {
    switch (gdt_fold_mode(d)) {
        case 0: return launch_c16<0>(d, stream);
        case 1: return launch_c16<1>(d, stream);
        case 3: return launch_c16<3>(d, stream);
        case 5: return launch_c16<5>(d, stream);
        default: return launch_c16<7>(d, stream);
    }
}
