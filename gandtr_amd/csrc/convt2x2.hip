// ConvTranspose2d(k2, s2, p0) as ONE GEMM whose depth-to-space is the store pattern (gfx950, MI355X): the up-convolutions of OrigUNet
// (components/model/network/unet.py, SkipConnBlock.convT).
//
// Kernel size = stride, so the layer has no overlap: every output pixel has exactly one source pixel,
//   out[n, 2y + dy, 2x + dx, :] = b + in[n, y, x, :] . W[:, :, dy, dx].
// GEMM: M = N H W pixel rows of K = Cin contiguous halves (NHWC), columns [dy][dx][co] (4 Cout of them), weights packed [4 Cout][Cin] (BatchNorm folded).
// With that column order the two dx phases of one (pixel, dy) are 2 Cout CONTIGUOUS halves of output row 2y + dy, starting at pixel 2x: a tile of 128 columns
// (Cout % 64 == 0, so it never straddles a dy) is 256 contiguous bytes per pixel row, written as sixteen 16-byte stores.  No second pass, no scattered halves.
//
// One workgroup (4 wavefronts, 2 x 2) owns 128 pixel rows x 128 columns; a wave holds 64 x 64 = four 32x32 fp32 accumulator tiles (v_mfma_f32_32x32x16_f16).
// K runs in chunks of 64: the pixel tile and the weight tile (16 KB each) go global -> registers -> LDS, two stages, the next chunk's loads in flight while this
// one's 16 MFMAs per wave run, one barrier per chunk.  LDS rows are 128 bytes with the 16-byte group swizzled by (row & 7), so the fragment reads of 32 rows
// spread over the banks.  Rows past M (ragged last tile) read pixel M - 1 and are not stored.  Epilogue: + bias (per column: the channel's shift repeated for
// the four phases), optional ReLU, fp16 through an LDS transpose, 16-byte stores.  Fixed summation order: bit-identical run to run.
//
// What bounds it (derived): 128 -> 64 moves 256 B in and 512 B out per input pixel for 65.5 kFLOP, about 85 FLOP/B, far below the chip's ridge: the outer layers
// are HBM-bound, and the form is chosen for bytes in flight (4 x 16 B loads per lane and chunk ahead of the MFMAs) and whole-line stores, not MFMA scheduling.
// The N tiles of one M tile are neighbours in the grid (gdt_tile_of_block), so the pixel tile is fetched from HBM once and re-read from L2.
// 148 VGPRs, no AGPRs, no scratch, 65 536 B of LDS: two workgroups per CU (-Rpass-analysis=kernel-resource-usage).
// MEASURED (tools/orig_unet_bench.py -> profiles/orig_unet_1gpu.json; MI355X, orig_unet with default arguments, per-op events, five profiled forwards per
// route alternating in one process, median (min .. max) ms; generic route = four 1 x 1 phase launches, GDT_CONVT2X2=0; torch = F.conv_transpose2d, fp16
// channels-last).  At 4 x 3 x 1024^2:
//   128 -> 64  @ 4 x 512^2 (805 MB):  0.276 (0.276 .. 0.283), 2.91 TB/s   generic 0.425 (0.422 .. 0.440)   1.54x   torch 0.717
//   256 -> 128 @ 4 x 256^2 (403 MB):  0.183 (0.177 .. 0.184), 2.20 TB/s   generic 0.213 (0.212 .. 0.214)   1.16x   torch 0.522
//   512 -> 256 @ 4 x 128^2 (202 MB):  0.121 (0.119 .. 0.124), 1.67 TB/s   generic 0.129 (0.126 .. 0.133)   1.06x   torch 0.229
//   1024 -> 512 @ 4 x 64^2 (105 MB):  0.105 (0.102 .. 0.110), 1.00 TB/s   generic 0.154 (0.152 .. 0.157)   1.47x   torch 0.220
// and the same within 2 % at 64 x 3 x 256^2 (same pixels per layer).  Routing by measurement: every eligible shape of the net beats the generic route with the
// two ranges apart, so all of them run here; 512 -> 256 is the narrowest (0.008 ms between the medians, ranges 0.002 ms apart at one geometry and 0.006 ms at the
// other) -- a shape to re-measure before anything is built on it.  No eligible shape measured slower.  The outer layer reaches 2.9 TB/s of the bytes it must
// move, the inner ones are launch- and latency-sized (0.1 ms for 105 MB): what the waves wait on there has NOT been profiled.  Whole f16 forward: 7.04 ms
// against 7.20 ms on the generic route (6166 GFLOP, ranges apart).  NOT MEASURED (not built): LDS DMA staging (global_load_lds) instead of the register round
// trip; a persistent form that keeps a weight tile resident across M tiles.
#include "gdt_common.h"
#include "conv_device.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64, NT = 256;
constexpr int ROWB = BK * 2;                        // bytes per LDS row (64 halves of K)
constexpr int TILE_BYTES = BM * ROWB;               // pixel tile and weight tile alike (BM == BN)
constexpr int STAGE_BYTES = 2 * TILE_BYTES;
constexpr int CP = BN + 8;                          // padded C-tile row (halves)
constexpr int LDS_BYTES = 2 * STAGE_BYTES;
static_assert(BM == BN && BM * CP * 2 <= LDS_BYTES, "the C tile reuses the staging buffers");

__global__ __launch_bounds__(NT, 2) void convt2x2_kernel(const ConvLaunch d) {
    constexpr int LQ = BM * 8 / NT;                 // 16-byte groups per thread and tile
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, fr = lane & 31, fh = lane >> 5;

    const int ntm = (d.M + BM - 1) / BM, ntn = d.CoutPad / BN;
    int tile_m, tile_n;
    if (!gdt_tile_of_block(blockIdx.x, ntm, ntn, tile_m, tile_n)) return;      // XCD-chunked, see conv_device.h

    // ---- loaders: thread -> rows (tid >> 3) + 32 q, 16-byte group tid & 7 of the chunk
    const int g = tid & 7;
    const f16* asrc[LQ]; const f16* bsrc[LQ];
    int ldst[LQ];
#pragma unroll
    for (int q = 0; q < LQ; ++q) {
        const int row = q * 32 + (tid >> 3);
        int p = tile_m * BM + row;
        p = p < d.M ? p : d.M - 1;                                             // ragged last tile: a pixel that exists, never stored
        asrc[q] = d.in + ((long)p * d.Cin + g * 8);
        bsrc[q] = d.w + ((long)(tile_n * BN + row) * d.Kpad + g * 8);
        ldst[q] = row * ROWB + ((g ^ (row & 7)) << 4);
    }
    const int nk = d.Cin / BK;
    f16x8 ra[LQ], rb[LQ];
    auto fetch = [&](int c) {
#pragma unroll
        for (int q = 0; q < LQ; ++q) { ra[q] = *(const f16x8*)(asrc[q] + c * BK); rb[q] = *(const f16x8*)(bsrc[q] + c * BK); }
    };
    auto stash = [&](int stage) {
#pragma unroll
        for (int q = 0; q < LQ; ++q) {
            *(f16x8*)(smem + stage * STAGE_BYTES + ldst[q]) = ra[q];
            *(f16x8*)(smem + stage * STAGE_BYTES + TILE_BYTES + ldst[q]) = rb[q];
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    int a_ad[2], b_ad[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int ar = wm * 64 + i * 32 + fr, br = wn * 64 + i * 32 + fr;
        a_ad[i] = ar * ROWB + ((fh ^ (ar & 7)) << 4);
        b_ad[i] = TILE_BYTES + br * ROWB + ((fh ^ (br & 7)) << 4);
    }

    fetch(0);
    stash(0);
    for (int c = 0; c < nk; ++c) {
        __syncthreads();                             // stage c & 1 is written; every wave is done reading the other stage
        const char* st = smem + (c & 1) * STAGE_BYTES;
        const bool more = c + 1 < nk;
        if (more) fetch(c + 1);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            f16x8 af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) { af[i] = *(const f16x8*)(st + (a_ad[i] ^ (kk << 5))); bf[i] = *(const f16x8*)(st + (b_ad[i] ^ (kk << 5))); }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        if (more) stash((c + 1) & 1);
    }

    // ---- epilogue: C layout of the MFMA -- column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    __syncthreads();                                 // all fragment reads of the staging buffers are done
    f16* Ct = (f16*)smem;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = wn * 64 + j * 32 + fr;
        const float bv = d.bias ? d.bias[tile_n * BN + col] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
                float v = acc[i][j][e] + bv;
                if (d.relu) v = fmaxf(v, 0.f);
                Ct[row * CP + col] = (f16)v;
            }
    }
    __syncthreads();
    // the tile's 128 columns = halves r .. r + 127 of the 2 Cout that pixel row (2y + dy, 2x .. 2x + 1) holds
    const int cout = d.phase_cout, col0 = tile_n * BN;
    const int dy = col0 / (2 * cout), r = col0 - dy * 2 * cout;
    for (int id = tid; id < BM * (BN / 8); id += NT) {
        const int row = id >> 4, ch = id & 15;
        const int p = tile_m * BM + row;
        if (p >= d.M) continue;
        const int q = p / d.W, x = p - q * d.W;      // q = n * H + y
        const int n = q / d.H, y = q - n * d.H;
        const long o = (((long)n * d.OH + 2 * y + dy) * d.OW + 2 * x) * cout + r + ch * 8;
        *(f16x8*)(d.out + o) = *(const f16x8*)(Ct + row * CP + ch * 8);
    }
}

GDT_KNOB_LAUNCH(knob_mode, "GDT_CONVT2X2", 1)                // 0: the layer runs as four 1 x 1 phase launches of the generic implicit GEMM (A/B inside one process)

}  // namespace

// Eligibility: ConvTranspose2d(k2, s2, p0) as its own plain launch in the f16 mode -- Cin and Cout multiples of 64, the weights packed [4 Cout][Cin] in the
// column order above, fp16 NHWC output of 2H x 2W, nothing in the epilogue but bias and ReLU.  Any map size, down to 1 x 1.
bool gdt_convt2x2_eligible(const ConvLaunch& d) {
    const bool shape = d.ntaps == 1 && d.sy == 1 && d.sx == 1 && d.osy == 2 && d.osx == 2 && !d.pad_reflect && d.Cin >= 64 && d.Cin % 64 == 0 && d.Kpad == d.Cin &&
                       d.phase_cout >= 64 && d.phase_cout % 64 == 0 && d.Cout == 4 * d.phase_cout && d.CoutPad == d.Cout &&
                       d.OHg == d.H && d.OWg == d.W && d.OH == 2 * d.H && d.OW == 2 * d.W && d.H >= 1 && d.W >= 1 && d.N >= 1;
    if (!shape || !d.in || !d.w || !d.out || d.out_f32 || d.w_lo) return false;
    if (d.in_norm || d.in_res || d.in_out || d.stats || d.res || d.pool2 || d.pair_cout || d.x3_form || d.in_f32 || d.in2 || d.leaky != 0.f || d.act) return false;
    if ((long)d.N * d.H * d.W != (long)d.M || (long)d.M + BM >= (1L << 31) || (long)d.Kpad * d.CoutPad >= (1L << 31)) return false;
    return knob_mode() != 0;
}

int gdt_launch_convt2x2(const ConvLaunch& d, hipStream_t stream, int* variant) {
    GDT_REQUIRE(gdt_convt2x2_eligible(d), "convt2x2: not an eligible launch");
    if (variant) *variant = 902128;
    using K = GdtKernel<convt2x2_kernel, LDS_BYTES>;
    int unused = 0;
    GDT_CHECK(K::figure(unused));
    return K::launch(gdt_grid_for_tiles((d.M + BM - 1) / BM, d.CoutPad / BN), NT, stream, d);
}
