// Conv2d(k3, s1, p1) of the channel concatenation of two tensors, with an LDS-resident input halo and weights streamed into registers (gfx950, MI355X):
// the Conv2d(128, 64, 3, padding=1) that AlignedP2pUNet applies to [x, nested(x)] at full image resolution (unet.py, AlignedP2pUNet.__init__).
//
// House form of conv4x4t_halo.hip.  One workgroup owns a patch of 8 x 16 pixels of one image and BN output channels (a 128-row accumulator tile).  Per
// 64-channel chunk it stages the 10 x 18 input halo ONCE (global -> LDS DMA; the zero ring and ragged edges resolved in the per-lane source address, swizzle of
// conv3x3_halo.hip: gdt_stage_halo_cat, conv_device.h) and walks its 9 taps by offsetting the fragment row.  Chunks 0 .. Cin / 64 - 1 come from `in`, the rest
// from `in2`: torch.cat([x, nested(x)], 1) is never materialised.  Two halo stages: the next chunk lands while this one's taps run; one barrier per chunk.
// Weights: [Cout/32][K/16][64 lanes][8] with k = (chunk * 9 + tap) * 64 + channel, so a wave's stream is sequential; each register is re-loaded for the next
// tap right after its last MFMA of this one.  Epilogue: conv_epilogue.h (shift with BatchNorm folded, optional ReLU, fp16 NHWC through the LDS transpose).
//
// Form: BN = 64 on 4 wavefronts (2 x 2), a wave holds 64 rows x 32 columns = 32 fp32 accumulators.  159 VGPRs, no AGPRs, no scratch, 47104 bytes of LDS,
// 3 waves per SIMD: three workgroups per CU (-Rpass-analysis=kernel-resource-usage).
// MEASURED (tools/p2p_unet_bench.py, MI355X, aligned_p2p_unet with nested_levels 7, per-op events, five profiled forwards per route alternating in one process;
// profiles/p2p_unet_1gpu.json): the net's 64 + 64 -> 64 layer, 618.5 GFLOP, takes 0.762 ms at 4 x 3 x 1024^2 (812 TFLOP/s, 0.32 of the 2.5 PFLOP/s floor; spread
// 0.005 ms) and 0.764 ms at 64 x 3 x 256^2 (spread 0.047) against 1.089 / 1.065 ms on the generic route (0.39 ms copy of the concatenation + 0.70 ms
// conv3x3_halo_rb.hip; spread 0.022 / 0.026): 1.43 x / 1.39 x, so the shape is routed here; whole forward 6.55 against 6.90 ms ("The
// normalisation U-Nets").  The kernel itself is slower than the one-tensor kernel on the same FLOPs (0.76 against 0.70 ms): it wins by the copy it saves.
// Other shapes (the family has only this one): see the routing rule at gdt_conv3x3_cat_halo_eligible.  NOT MEASURED: 128-column tiles for cout >= 128; a 16-row patch, which would stage 1.27 halo pixels
// per output pixel instead of 1.41.
#include "conv_epilogue.h"
#include "conv_device.h"

namespace {

constexpr int ROWB = 128;          // bytes per LDS row (64 halves of K)
constexpr int PH = 8, HW_ = 18, HROWS = (PH + 2) * HW_, HROWS_PAD = (HROWS + 7) / 8 * 8, A_BYTES = HROWS_PAD * ROWB;
constexpr int BM = PH * 16;

template <int BN, int WGM, int WGN>
constexpr size_t cc_lds_bytes() {
    constexpr size_t staging = 2 * (size_t)A_BYTES;
    constexpr size_t epilogue = conv_epilogue_lds_bytes<BM, BN, WGM, WGN, WGM * WGN * 64>();
    return staging > epilogue ? staging : epilogue;
}

template <int BN, int WGM, int WGN>
__global__ __launch_bounds__(WGM * WGN * 64, 2) void conv3x3_cat_halo_kernel(const ConvLaunch d) {
    constexpr int NT = WGM * WGN * 64, RPR = NT / 8;           // threads, halo rows staged per loader round
    constexpr int NR = (HROWS_PAD + RPR - 1) / RPR;            // halo staging rounds per chunk
    static_assert(NR <= 9, "halo rounds are spread over the 9 taps of the previous chunk");
    constexpr int WTM = BM / WGM, WTN = BN / WGN;
    constexpr int TM = WTM / 32, TN = WTN / 32;
    static_assert(TM >= 1 && TN >= 1 && WTM % 32 == 0 && WTN % 32 == 0, "tile shape");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;

    const int tiles_x = (d.W + 15) >> 4, tiles_y = (d.H + PH - 1) / PH;
    const int tpi = tiles_x * tiles_y, ntm = d.N * tpi, ntn = d.CoutPad / BN;
    int tile_m, tile_n;
    if (!gdt_tile_of_block(blockIdx.x, ntm, ntn, tile_m, tile_n)) return;      // XCD-chunked, see conv_device.h
    const int n = tile_m / tpi, tr = tile_m - n * tpi;
    const int y0 = (tr / tiles_x) * PH, x0 = (tr % tiles_x) << 4;              // first pixel of the patch; halo position (0, 0) = (y0 - 1, x0 - 1)

    const int nca = d.Cin >> 6, nchunks = (d.Cin + d.in2_cin) >> 6;

    const int lrow = tid >> 3;
    auto issue_a = [&](int chunk, int stage, int r) {
        gdt_stage_halo_cat<HW_, HROWS, HROWS_PAD, RPR>(d, smem + stage * A_BYTES, n, y0, x0, nca, chunk, r, wave, lane, lrow);
    };

    // ---- weights: fragment (column block cb, k-step ks) = 64 lanes x 16 bytes; step q = chunk * 9 + tap covers k-steps 4 q .. 4 q + 3
    const int nks = d.Kpad >> 4, nsteps = nchunks * 9;
    const f16x8* wf = (const f16x8*)d.w_frag + lane;
    int cb0[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) cb0[j] = ((tile_n * BN + wn * WTN) >> 5) + j;
    auto load_b = [&](int q, int kk, int j) -> f16x8 { return wf[((long)cb0[j] * nks + (q * 4 + kk)) * 64]; };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // fragment rows: tile row m = (ly, lx) -> halo row ly * HW + lx, + the tap; the k-substep kk is applied with ONE xor (kk << 5) (conv3x3_halo.hip)
    const int fr = lane & 31, fh = lane >> 5;
    int a_h0[TM], a_lx[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = wm * WTM + i * 32 + fr;
        a_lx[i] = m & 15; a_h0[i] = (m >> 4) * HW_ + a_lx[i];
    }

    f16x8 bfr[4][TN];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int j = 0; j < TN; ++j) bfr[kk][j] = load_b(0, kk, j);
#pragma unroll
    for (int r = 0; r < NR; ++r) issue_a(0, 0, r);

    for (int c = 0; c < nchunks; ++c) {
        __syncthreads();                                          // the chunk's halo has landed (the barrier's fence drains the LDS DMA), and every wave is done
                                                                  // with the other stage, which the taps below refill
        const int stage = c & 1;
        const bool halo_more = c + 1 < nchunks;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int ty = t / 3, tx = t % 3;
            f16x8 afr[4][TM];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int a_ad = stage * A_BYTES + (a_h0[i] + ty * HW_ + tx) * ROWB + ((fh ^ (((a_lx[i] + tx) >> 1) & 7)) << 4);
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) afr[kk][i] = *(const f16x8*)(smem + (a_ad ^ (kk << 5)));
            }
            if (halo_more && t < NR) issue_a(c + 1, (c + 1) & 1, t);      // one halo round of the next chunk per tap
            const int q = c * 9 + t, qn = q + 1 < nsteps ? q + 1 : q;     // (past the last step: a harmless reload of a fragment that exists)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(afr[kk][i], bfr[kk][j], acc[i][j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < TN; ++j) bfr[kk][j] = load_b(qn, kk, j);      // the next tap's fragment, a whole tap ahead of its use
            }
        }
    }

    conv_epilogue_f16<BM, BN, WGM, WGN, NT, TM, TN>(d, acc, smem, tile_m, tile_n, [&](int row, bool& ok) -> long {
        const int y = y0 + (row >> 4), x = x0 + (row & 15);
        ok = (y < d.H) & (x < d.W);
        return ((long)n * d.H + y) * d.W + x;
    });
}

template <int BN, int WGM, int WGN>
int launch_cc(const ConvLaunch& d, hipStream_t stream) {
    using K = GdtKernel<conv3x3_cat_halo_kernel<BN, WGM, WGN>, (int)cc_lds_bytes<BN, WGM, WGN>()>;
    int unused = 0;
    GDT_CHECK(K::figure(unused));
    return K::launch(gdt_grid_for_tiles((int)gdt_patches(d.N, d.H, d.W, PH), d.CoutPad / BN), WGM * WGN * 64, stream, d);
}

GDT_KNOB_LAUNCH(knob_mode, "GDT_CONV3X3_CAT_HALO", 1)        // 0: the layer runs as a copy that writes the concatenation + the conv of one tensor; 1: the kernel where it
                                                             // measured faster (below); 2: wherever eligible (A/B inside one process)

}  // namespace

// Eligibility: Conv2d(k3, s1, p1, zero padding) of two tensors as its own plain launch -- both channel counts multiples of 64, the fragment-ordered weights in
// the step order above, fp16 NHWC output in whole 64-column tiles, nothing in the epilogue but bias and ReLU.  Any map size: ragged patches at the right and
// bottom edges and maps smaller than a patch (down to 1 x 1) are the kernel's business.
// Routing, by measurement (profiles/p2p_unet_1gpu.json, "cat_conv_sweep"; generic route / kernel, spreads 0.0002 - 0.011 ms): the copy costs the generic route a share of
// its time that falls with cout, and the 256-column form of conv3x3_halo_rb.hip is about a tenth faster per FLOP than this kernel.  The kernel wins at 64 output
// channels (1.39 - 2.17 x, 64 + 64 channels on 4 x 1024^2 down to 1 x 64^2) and at 128 (128 + 128 -> 128 on 4 x 512^2: 1.11 x); where the concatenation is no power of two, so
// that the generic route pads it (64 + 128 -> 256 on 4 x 256^2: 1.15 x); and where the one-tensor conv has too few patches for conv3x3_halo_rb.hip (512 + 512 -> 512 on 1 x 16^2:
// 2.13 x).  It loses at 256 + 256 -> 256 on 4 x 256^2 (0.90 x) and 512 + 512 -> 512 on 4 x 64^2 (0.81 x): those go to the generic route.
bool gdt_conv3x3_cat_halo_eligible(const ConvLaunch& d) {
    const bool shape = d.ntaps == 9 && d.TW == 3 && d.sy == 1 && d.sx == 1 && d.dy0 == -1 && d.dx0 == -1 && d.dys == 1 && d.dxs == 1 && d.osy == 1 && d.osx == 1 &&
                       d.ooy == 0 && d.oox == 0 && !d.pad_reflect && d.Cin >= 64 && d.Cin % 64 == 0 && d.in2_cin >= 64 && d.in2_cin % 64 == 0 && d.in2 != nullptr &&
                       d.in2_stride == 1 && d.in2_h == d.H && d.in2_w == d.W && d.Kpad == 9 * (d.Cin + d.in2_cin) && d.OHg == d.H && d.OWg == d.W && d.OH == d.H &&
                       d.OW == d.W && d.H >= 1 && d.W >= 1 && d.N >= 1;
    if (!shape || !d.in || !d.w_frag || !d.out || !d.zeros || d.out_f32 || d.Cout % 8 != 0 || d.CoutPad % 64 != 0 || d.CoutPad < d.Cout) return false;
    if (d.in_norm || d.in_relu || d.in_res || d.in_out || d.stats || d.res || d.pool2 || d.phase_cout || d.pair_cout || d.x3_form || d.in_f32 || d.leaky != 0.f) return false;
    if (!gdt_offsets_fit(d.N, d.H, d.W, d.Cin > d.in2_cin ? d.Cin : d.in2_cin, 62) || !gdt_offsets_fit(d.N, d.OH, d.OW, 1, 31) || (long)d.Kpad * d.CoutPad >= (1L << 31)) return false;
    const int mode = knob_mode();
    if (mode != 1) return mode != 0;
    const int cin = d.Cin + d.in2_cin, bn = d.CoutPad % 256 == 0 ? 256 : (d.CoutPad % 128 == 0 ? 128 : 64);
    const bool padded = (cin & (cin - 1)) != 0;                                                       // the generic route rounds the concatenation up to a power of two
    const bool few = !gdt_enough_tiles(gdt_patches(d.N, d.H, d.W), d.CoutPad / bn, 16);                // the rule of gdt_conv_halo_eligible for fragment-ordered weights
    return d.CoutPad <= 128 || padded || few;
}

int gdt_launch_conv3x3_cat_halo(const ConvLaunch& d, hipStream_t stream, int* variant) {
    GDT_REQUIRE(gdt_conv3x3_cat_halo_eligible(d), "conv3x3_cat_halo: not an eligible launch");
    if (variant) *variant = 908064;
    return launch_cc<64, 2, 2>(d, stream);
}
