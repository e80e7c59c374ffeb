// Whole ResNet BasicBlock (identity form, 64 channels) in ONE launch, fp16 mode:
//     y = ReLU( x + BN2( W_2 (*) ReLU( BN1( W_1 (*) x ))))        torchvision BasicBlock as restated in components/model/network/backbones.py
// with W_1, W_2: 3x3 / stride 1 / zero pad 1, 64 -> 64, BatchNorm(eval) folded into the weights / biases at pack time.  ResNet-18 / 34 layer1 (256 x 256 maps at a
// 1024^2 input).
//
// Why: layer by layer a block moves x (in) + h + h + x (residual) + y, five tensors as large as the block's input (268 MB each at batch 32); fused, h never leaves
// the CU: x in (+ halo), y out.  The price is conv1 recomputed on a one-pixel ring: 18 x 18 = 324 (352 computed) instead of 256 pixels per patch, 1.27x (1.375x) its
// FLOPs.  Whether that pays at 64 channels is a measurement (tools/resnet_basic_bench.py), and the default of GDT_CONV_BASIC follows it.
//
// One persistent 512-thread workgroup per CU walks XCD-chunked 16 x 16 output patches (the schedule of conv_bneck.hip):
//   stage    the 20 x 20 x 64 input halo (two pixels wide) goes global -> registers -> LDS, zero outside the image (conv1 pads x); the loads of the NEXT patch are
//            requested before conv2 starts and land while it runs;
//   conv1    h = ReLU(W_1 (*) x + b_1) on the 18 x 18 ring-extended patch: 11 blocks of 32 pixels x 2 blocks of 32 channels = 22 tiles, three per wave (the 24th and
//            the rows past 324 repeat the last pixel and are not stored); h is ZERO outside the image (conv2 pads h, not x: ring positions outside the image are
//            zeroed after bias and ReLU) and is written to LDS as fp16;
//   conv2    acc = W_2 (*) h + b_2 from the LDS-resident h: 8 pixel blocks x 2 channel blocks, two per wave; the residual x comes from the halo already in LDS and
//            is added in fp32, ReLU, ONE fp16 rounding; every 32 x 32 block is transposed through a 2.5 KB patch of the wave's own so that lanes store 16 bytes
//            (four lanes = the wave's 64 bytes of a pixel).
//   Weights: the fragment-ordered copies of net_build.hip ([cout/32][K/16][64 lanes][8 halves], K = tap * 64 + channel), streamed from L2 into registers six taps
//            (24 fragments) ahead of their use, as in conv3x3_halo_rb.hip: 2 x 73.7 KB do not fit beside the tensors.  A wave needs the half of its channel block.
//   LDS:     20 x 20 x 128 B (x) + 352 x 128 B (h) + 8 x 2.5 KB (store patches) = 114 KB: one workgroup per CU.
//   MFMA operands are swapped (D = W A^T): a lane holds 4 consecutive channels of one pixel.  No atomics; a patch is computed from its own image only, so an
//   image's bits do not depend on its batch position.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "conv_device.h"

namespace {

constexpr int NT = 512, NWAVE = 8, C = 64, PH = 16, PW = 16;
constexpr int XW = PW + 4, XPIX = (PH + 4) * XW;                   // x halo: 20 x 20 pixels
constexpr int HW_ = PW + 2, HPIX = (PH + 2) * HW_;                 // h ring: 18 x 18 pixels
constexpr int HB = (HPIX + 31) / 32, HPAD = HB * 32;               // ... in 11 blocks of 32 (352 rows)
constexpr int PB = PH * PW / 32;                                   // output pixel blocks (a block = two patch rows)
constexpr int KS = 9 * (C / 16);                                   // k-steps of a 3x3 conv: 36, four per tap
constexpr int XBYTES = XPIX * 128, HBYTES = HPAD * 128;
constexpr int PROW = 80, PATCH = 32 * PROW;                        // store patch of a wave: 32 pixels x 64 bytes, rows 80 bytes apart
constexpr int H_OFF = XBYTES, P_OFF = XBYTES + HBYTES, LDS = P_OFF + NWAVE * PATCH;
constexpr int NPX = (XPIX * 8 + NT - 1) / NT;                      // 16-byte units of the x halo per thread: 7
static_assert(HB <= 12 && PB == 8 && LDS <= 160 * 1024, "tiles per wave, LDS layout");

// (as conv_bneck.hip: both candidates through uniform addresses, the lane picks by fh)
__device__ __forceinline__ float4 bias4(const float* __restrict__ b, int base_uniform, int g, int fh) {
    const float4 lo = *(const float4*)(b + base_uniform + 8 * g), hi = *(const float4*)(b + base_uniform + 8 * g + 4);
    return fh ? hi : lo;
}

struct BasicLaunch {
    const f16* x; f16* y;
    const f16* w1; const f16* w2;         // fragment order [2][36][64 lanes][8 halves]
    const float* b1; const float* b2;     // folded BatchNorm shifts (or the plain biases)
    int N, H, W;
};

// (the body takes its workgroup index and grid size as arguments: the kernel below hands it blockIdx.x and gridDim.x)
__device__ __forceinline__ void conv3x3_basic_body(const BasicLaunch& d, const int ntiles, const int bid, const int gdim) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const xbuf = smem;
    char* const hbuf = smem + H_OFF;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles_x = (d.W + PW - 1) / PW, tiles_y = (d.H + PH - 1) / PH, tpi = tiles_x * tiles_y;

    // XCD-chunked persistent schedule (conv_bneck.hip): the CUs of one XCD hold neighbouring patches, whose halos overlap in its L2
    const int per_xcd = (ntiles + 7) >> 3, S = gdim >> 3;
    const int xcd = bid & 7, slot = bid >> 3;
    const int span_lo = xcd * per_xcd, span_hi = min(span_lo + per_xcd, ntiles);
    int tile = span_lo + slot;
    if (tile >= span_hi) return;

    // ---- x halo, global -> registers -> LDS.  Unit e = tid + k * NT: halo pixel e >> 3, 16-byte piece e & 7, stored at piece position (e & 7) ^ swizzle(pixel) of
    // its 128-byte LDS row.  Pixels outside the image are loaded from a clamped (valid) address and stored as zeros.
    struct XRegs { f16x8 v[NPX]; };
    auto load_x = [&](int tl, XRegs& xr) {
        const int n = tl / tpi, r = tl - n * tpi;
        const int y0 = (r / tiles_x) * PH, x0 = (r % tiles_x) * PW;
        int t = tid;
        asm volatile("" : "+v"(t));
#pragma unroll
        for (int k = 0; k < NPX; ++k) {
            const int e = min(t + k * NT, XPIX * 8 - 1);
            const int hp = e >> 3;
            const int hy = hp / XW, hx = hp - hy * XW;
            const int iy = min(max(y0 - 2 + hy, 0), d.H - 1), ix = min(max(x0 - 2 + hx, 0), d.W - 1);
            xr.v[k] = *(const f16x8*)(d.x + ((size_t)((n * d.H + iy) * d.W + ix) * C + (e & 7) * 8));
        }
    };
    auto store_x = [&](int tl, const XRegs& xr) {
        const int r = tl % tpi;
        const int y0 = (r / tiles_x) * PH, x0 = (r % tiles_x) * PW;
        int t = tid;
        asm volatile("" : "+v"(t));
#pragma unroll
        for (int k = 0; k < NPX; ++k) {
            const int e = t + k * NT;
            const int row = e >> 3;
            const int hy = row / XW, hx = row - hy * XW;
            const bool inb = ((unsigned)(y0 - 2 + hy) < (unsigned)d.H) & ((unsigned)(x0 - 2 + hx) < (unsigned)d.W);
            f16x8 v = xr.v[k];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = inb ? v[q] : (f16)0.f;
            if (e < XPIX * 8) *(f16x8*)(xbuf + row * 128 + (((e & 7) ^ ((row >> 1) & 7)) << 4)) = v;
        }
    };

    // ---- per-wave tiles: channel block cmb (32 of the 64 output channels) of pixel blocks grp + 4 j -- j < 3 of the 11 (12) h blocks, j < 2 of the 8 output blocks
    const int cmb = wave & 1, grp = wave >> 1;

    // ---- weights: ONE stream of 18 taps per patch (9 of W_1, 9 of W_2; the next patch starts over), four 1 KB fragments per tap and channel block, through a
    // ring of WD taps in registers: a slot is re-loaded right after its last MFMA has issued (conv3x3_halo_rb.hip), WD taps ahead of its next use.  Vector-memory
    // operations retire in issue order, so a weight load queues behind the HBM loads of the next halo and the stores of y: six taps (~4000 cycles of MFMAs) cover that.
    constexpr int WD = 6;
    static_assert(18 % WD == 0, "a tap's ring slot is the same in every patch");
    f16x8 wq[WD][4];
    unsigned lo16 = lane * 16;
    auto wload = [&](int s) {                                      // stream position s (0 .. 17; compile-time after unrolling)
        const char* wb = (const char*)(s < 9 ? d.w1 : d.w2) + ((cmb * KS + (s % 9) * 4) << 10);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) wq[s % WD][ks] = *(const f16x8*)(wb + (ks << 10) + lo16);
    };
#pragma unroll
    for (int s = 0; s < WD; ++s) wload(s);

    XRegs xr;
    load_x(tile, xr);
    store_x(tile, xr);
    gdt_lds_barrier();

    for (;;) {
        asm volatile("" : "+v"(lo16));     // (uniform base + 32-bit lane offset behind an opaque copy, refreshed per patch: conv_bneck.hip)
        const int n = tile / tpi, rr = tile - n * tpi;
        const int y0 = (rr / tiles_x) * PH, x0 = (rr % tiles_x) * PW;
        const int next = tile + S;
        const bool has_next = next < span_hi;

        // ================================================================ conv1: h = ReLU(W_1 (*) x + b_1) on the 18 x 18 ring
        {
            f32x16 acc[3];
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
            int lane_t = lane;                                       // (opaque copy: the fragment addresses are functions of the lane only, i.e. invariants of
            asm volatile("" : "+v"(lane_t));                         //  the persistent patch loop -- hoisted, they are spilled: conv_bneck.hip)
            const int fr = lane_t & 31, fh = lane_t >> 5;
            int xb[3];                                               // x halo row of tap (0, 0) of this lane's h pixel
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int r = min((grp + 4 * j) * 32 + fr, HPIX - 1);    // (rows past the ring repeat its last pixel: computed, not stored)
                const int hy = r / HW_, hx = r - hy * HW_;
                xb[j] = hy * XW + hx;
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int ty = t / 3, tx = t - ty * 3;
                int a0[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int xrow = xb[j] + ty * XW + tx;
                    a0[j] = xrow * 128 + ((fh ^ ((xrow >> 1) & 7)) << 4);
                }
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const f16x8 af = *(const f16x8*)(xbuf + (a0[j] ^ (ks << 5)));
                        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wq[t % WD][ks], af, acc[j], 0, 0, 0);
                    }
                }
                wload((t + WD) % 18);
                __builtin_amdgcn_sched_barrier(0);
            }
            // h -> LDS (fp16): lane holds pixel `row`, channels cmb * 32 + 8 g + 4 fh + {0..3}; zero outside the image and past the ring
            float4 bv[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) bv[g] = bias4(d.b1, cmb * 32, g, fh);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int pb = grp + 4 * j;
                if (pb < HB) {
                    const int row = pb * 32 + fr;
                    const int hy = row / HW_, hx = row - hy * HW_;
                    const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
                    const bool inside = (row < HPIX) & ((unsigned)iy < (unsigned)d.H) & ((unsigned)ix < (unsigned)d.W);
                    char* hp = hbuf + row * 128;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float4 b = bv[g];
                        f16x4 v;
                        v[0] = (f16)(inside ? fmaxf(acc[j][4 * g] + b.x, 0.f) : 0.f);
                        v[1] = (f16)(inside ? fmaxf(acc[j][4 * g + 1] + b.y, 0.f) : 0.f);
                        v[2] = (f16)(inside ? fmaxf(acc[j][4 * g + 2] + b.z, 0.f) : 0.f);
                        v[3] = (f16)(inside ? fmaxf(acc[j][4 * g + 3] + b.w, 0.f) : 0.f);
                        *(f16x4*)(hp + (((cmb * 4 + g) ^ ((row >> 1) & 7)) << 4) + fh * 8) = v;
                    }
                }
            }
        }
        gdt_lds_barrier();                 // h complete

        // ================================================================ conv2: y = ReLU(W_2 (*) h + b_2 + x)
        {
            f32x16 acc[2];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
            int lane_t = lane;                                       // (opaque copy, as in conv1)
            asm volatile("" : "+v"(lane_t));
            const int fr = lane_t & 31, fh = lane_t >> 5;
            int hb[2];                                               // h ring row of tap (0, 0) of this lane's output pixel
#pragma unroll
            for (int j = 0; j < 2; ++j) hb[j] = ((grp + 4 * j) * 2 + (fr >> 4)) * HW_ + (fr & 15);
            // the x halo of the NEXT patch is requested now (behind the weights of the next six taps): the memory system works through conv2, which itself
            // touches LDS and the L2-resident weights only.  Unconditional (the last patch fetches its own halo again, never stored): a conditional memory
            // operation in here turns the counted waits for the weights into vmcnt(0)
            load_x(has_next ? next : tile, xr);
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int ty = t / 3, tx = t - ty * 3;
                int a0[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int hrow = hb[j] + ty * HW_ + tx;
                    a0[j] = hrow * 128 + ((fh ^ ((hrow >> 1) & 7)) << 4);
                }
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const f16x8 af = *(const f16x8*)(hbuf + (a0[j] ^ (ks << 5)));
                        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wq[(9 + t) % WD][ks], af, acc[j], 0, 0, 0);
                    }
                }
                wload((9 + t + WD) % 18);                            // (the last six: the next patch's first taps -- the same addresses when there is none)
                __builtin_amdgcn_sched_barrier(0);
            }
            // + bias + residual (the pixel's own row of the x halo, fp32), ReLU, one rounding; through the wave's patch to 16-byte stores
            // (wave-private patch: the wave's own LDS operations are executed in order, no barrier)
            char* patch = smem + P_OFF + wave * PATCH;
            float4 bv[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) bv[g] = bias4(d.b2, cmb * 32, g, fh);
            const int pl = lane_t >> 2, pc = lane_t & 3;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int pb = grp + 4 * j;
                const int xrow = (pb * 2 + (fr >> 4) + 2) * XW + (fr & 15) + 2;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f16x4 res = *(const f16x4*)(xbuf + xrow * 128 + (((cmb * 4 + g) ^ ((xrow >> 1) & 7)) << 4) + fh * 8);
                    const float4 b = bv[g];
                    f16x4 v;
                    v[0] = (f16)fmaxf(acc[j][4 * g] + b.x + (float)res[0], 0.f);
                    v[1] = (f16)fmaxf(acc[j][4 * g + 1] + b.y + (float)res[1], 0.f);
                    v[2] = (f16)fmaxf(acc[j][4 * g + 2] + b.z + (float)res[2], 0.f);
                    v[3] = (f16)fmaxf(acc[j][4 * g + 3] + b.w + (float)res[3], 0.f);
                    *(f16x4*)(patch + fr * PROW + g * 16 + fh * 8) = v;
                }
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int pr = pl + 16 * i;                      // pixel of the block: patch row pb * 2 + i, column pl
                    const f16x8 o = *(const f16x8*)(patch + pr * PROW + pc * 16);
                    const int y = y0 + pb * 2 + i, x = x0 + pl;
                    if ((y < d.H) & (x < d.W)) *(f16x8*)(d.y + ((size_t)((n * d.H + y) * d.W + x) * C + cmb * 32 + pc * 8)) = o;
                }
            }
        }
        if (!has_next) break;
        tile = next;
        gdt_lds_barrier();                 // every wave has left conv2: x (residual rows) and h may be rewritten
        store_x(tile, xr);
        gdt_lds_barrier();
    }
}

__global__ __launch_bounds__(NT) void conv3x3_basic_kernel(const BasicLaunch d, const int ntiles) {
    conv3x3_basic_body(d, ntiles, blockIdx.x, gridDim.x);
}

// Read whenever a geometry is planned.  The fused and the layer-by-layer route use the same layout (the tensor between the two convs is laid out on both).
// Default 0: the measured default -- the whole forwards of GeM-ResNet-18 / 34 tie or lose with the fused route (profiles/resnet_basic_1gpu.json)
GDT_KNOB_LAUNCH(knob_mode, "GDT_CONV_BASIC", 0)              // 0 never, 1 with enough patches, 2 whatever the patch count
GDT_KNOB_LATCHED(knob_min_tiles, "GDT_BASIC_MIN_TILES", 256)

}  // namespace

// Eligible: the two convs of an identity BasicBlock (checked by the planner in net_plan.hip) with 64 channels, offsets within 31 bits, and -- unless the knob
// is 2 -- enough patches to fill the chip, of which at most 15 % of the area may hang over the image
bool gdt_basic_eligible(int C_, int N, int H, int W) {
    const int mode = knob_mode();
    if (mode <= 0 || C_ != C || N < 1 || H < 1 || W < 1) return false;
    if (!gdt_offsets_fit(N, H, W, C, 31)) return false;
    if (mode >= 2) return true;
    if (gdt_useful_area(H, W, PH, PW) < GDT_MIN_USEFUL_AREA) return false;
    return gdt_enough_tiles(gdt_patches(N, H, W, PH, PW), 1, knob_min_tiles());
}

int gdt_launch_basic(const f16* x, f16* y, const f16* w1, const f16* w2, const float* b1, const float* b2, int N, int H, int W, hipStream_t stream) {
    GDT_REQUIRE(x && y && w1 && w2 && b1 && b2 && N >= 1 && H >= 1 && W >= 1 && gdt_offsets_fit(N, H, W, C, 31), "BasicBlock geometry");
    using K = GdtKernel<conv3x3_basic_kernel, LDS>;
    int cus = 0;
    GDT_CHECK(K::figure(cus));
    const BasicLaunch d{x, y, w1, w2, b1, b2, N, H, W};
    const int ntiles = (int)gdt_patches(N, H, W, PH, PW);
    return K::launch(std::min(cus, (ntiles + 7) / 8 * 8), NT, stream, d, ntiles);
}
