// ConvTranspose2d(k4, s2, p1) of one tensor or of the channel concatenation of two, with an LDS-resident input halo and weights streamed into registers
// (gfx950, MI355X): the up-convolutions of the pix2pix U-Net (UnetSkipConnectionBlock, p2p_networks.py:205-221), two thirds of its FLOPs.
//
// The layer is the adjoint of conv4x4_halo.hip's stride-2 form and shares its property: at stride 2 the 4x4 kernel is a dense 2x2 convolution per output
// parity, every one of the 16 taps meets every input pixel exactly once and no product is wasted.  Output pixel (2y + py, 2x + px) reads input rows
//   py = 0: (iy = y, ky = 1), (iy = y - 1, ky = 3)        py = 1: (iy = y, ky = 2), (iy = y + 1, ky = 0)          (columns alike).
// One workgroup owns a patch of 8 x 16 INPUT pixels of one image and BN output channels = 16 x 32 output pixels, as four 128-row accumulator tiles (one per
// parity).  Per 64-channel chunk it stages the 10 x 18 input halo ONCE (global -> LDS DMA, the zero ring and ragged edges resolved in the per-lane source
// address, swizzle of conv3x3_halo.hip) and walks its 9 shifts (sy, sx): the A fragments of a shift are read from LDS once and feed every parity that meets the
// shift -- the centre four, an edge two, a corner one: 16 (shift, parity) steps, gdt_t4_step (gdt_common.h).  Chunks 0 .. Cin / 64 - 1 come from `in`, the
// rest from `in2`: the skip connection torch.cat([x, model(x)], 1) is never materialised.  The ReLU in front of the layer (uprelu) is applied to the `in`
// chunks as a packed fp16 max on the A fragments after the LDS read -- the DMA cannot transform data, and the skip tensor is stored once, as the next
// down-convolution reads it (LeakyReLU applied: relu(leaky(x)) = relu(x)).  Two halo stages: the next chunk lands while this one's steps run; one barrier
// per chunk.  Weights: [Cout/32][K/16][64 lanes][8] with k = (chunk * 16 + step) * 64 + channel, so a wave's stream is sequential; each register is
// re-loaded for the next step right after its last MFMA of this one.  Epilogue: conv_epilogue.h once per parity (shift with BatchNorm folded, optional ReLU,
// fp16 NHWC through the LDS transpose).
//
// Form: BN = 64 on 4 wavefronts (2 x 2), two workgroups per CU; a wave holds 4 parities x 64 rows x 32 columns = 128 fp32 accumulators.  232 VGPRs, no AGPRs, no
// scratch, 47104 bytes of LDS, 2 waves per SIMD (-Rpass-analysis=kernel-resource-usage).
// MEASURED (tools/unet_bench.py, MI355X, 64 x 3 x 256^2, num_downs 8, ngf 64, per-op events, five profiled forwards per variant alternating in one process;
// profiles/unet_bench_1gpu.json has the run of the committed form): every up-convolution takes 0.20 - 0.22 ms here against 0.30 - 0.47 ms on the generic route
// (copy of the concatenation + four phase launches), run-to-run spread 0.003 - 0.007 ms: 1.5 - 2.2 x on the three 137-GFLOP layers (636 - 687 TFLOP/s, 0.25 -
// 0.28 of the 2.5 PFLOP/s floor), and 1.5 x on the small inner ones, so every eligible shape is routed here ("The U-Net generator").
// The time is nearly the same for a 4-GFLOP and a 137-GFLOP layer (every CU walks about 256 steps of 8 MFMAs per wave either way), so the MFMA pipe does not
// set it; a step's weight fragments are fetched only one step ahead, which is the suspect, but what the waves wait on has NOT been profiled.
// REJECTED by measurement: (a) BN = 128 on 8 wavefronts (2 x 4, one halo staging per 128 columns) wherever Cout allows: 0.205 against 0.195 ms per layer, whole
// forward 3.10 against 2.99 ms (ranges of 20 alternating forwards apart); (b) all halo rounds of the next chunk issued at the head of the chunk instead of one
// per shift: 0.21 against 0.20 ms.  NOT MEASURED (not built): a workgroup that takes the two parities of one py and stages the halo twice; weight fragments
// fetched two or more steps ahead (needs the A fragments read per k-substep to stay inside 256 registers).
#include "conv_epilogue.h"
#include "conv_device.h"

namespace {

constexpr int ROWB = 128;          // bytes per LDS row (64 halves of K)
constexpr int PH = 8, HW_ = 18, HROWS = (PH + 2) * HW_, HROWS_PAD = (HROWS + 7) / 8 * 8, A_BYTES = HROWS_PAD * ROWB;
constexpr int BM = PH * 16;

template <int BN, int WGM, int WGN>
constexpr size_t t4_lds_bytes() {
    constexpr size_t staging = 2 * (size_t)A_BYTES;
    constexpr size_t epilogue = conv_epilogue_lds_bytes<BM, BN, WGM, WGN, WGM * WGN * 64>();
    return staging > epilogue ? staging : epilogue;
}

template <int BN, int WGM, int WGN>
__global__ __launch_bounds__(WGM * WGN * 64, 2) void conv4x4t_halo_kernel(const ConvLaunch d) {
    constexpr int NT = WGM * WGN * 64, RPR = NT / 8;           // threads, halo rows staged per loader round
    constexpr int NR = (HROWS_PAD + RPR - 1) / RPR;            // halo staging rounds per chunk
    static_assert(NR <= 9, "halo rounds are spread over the 9 shifts of the previous chunk");
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
    const int y0 = (tr / tiles_x) * PH, x0 = (tr % tiles_x) << 4;              // first INPUT pixel of the patch; halo position (0, 0) = (y0 - 1, x0 - 1)

    const int nca = d.Cin >> 6, nchunks = (d.Cin + d.in2_cin) >> 6;

    // ---- halo loader: round r stages halo rows r * RPR .. + RPR - 1, eight lanes per row (one 16-byte channel group each); the swizzle
    // chunk' = chunk ^ ((halo column >> 1) & 7) is applied to the SOURCE channel group (conv3x3_halo.hip).  Local code: the same statements as
    // gdt_stage_halo_cat (conv_device.h), which this kernel does not call -- through the helper it compiles to another schedule (238 VGPRs against 232)
    const int lrow = tid >> 3;
    auto issue_a = [&](int chunk, int stage, int r) {
        if (r * RPR + wave * 8 >= HROWS_PAD) return;               // wave-uniform: rows beyond the padded halo
        const int h = r * RPR + lrow;
        int hy, hx;
        gdt_halo_yx<HW_>(h, hy, hx);
        const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
        const bool ok = (h < HROWS) & ((unsigned)iy < (unsigned)d.H) & ((unsigned)ix < (unsigned)d.W);      // zero ring, ragged edges, pad rows: zeros
        const int q = (lane & 7) ^ ((hx >> 1) & 7);
        const long pix = ((long)n * d.H + (ok ? iy : 0)) * d.W + (ok ? ix : 0);
        const bool second = chunk >= nca;                          // (wave-uniform)
        const f16* base = second ? d.in2 : d.in;
        const int cs = second ? d.in2_cin : d.Cin, cc = second ? chunk - nca : chunk;
        const f16* src = base + (pix * cs + (cc * 8 + q) * 8);
        gdt_glds16(ok ? src : d.zeros, smem + stage * A_BYTES + (r * RPR + wave * 8) * ROWB);
    };

    // ---- weights: fragment (column block cb, k-step ks) = 64 lanes x 16 bytes; step q = chunk * 16 + s covers k-steps 4 q .. 4 q + 3
    const int nks = d.Kpad >> 4, nsteps = nchunks * 16;
    const f16x8* wf = (const f16x8*)d.w_frag + lane;
    int cb0[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) cb0[j] = ((tile_n * BN + wn * WTN) >> 5) + j;
    auto load_b = [&](int q, int kk, int j) -> f16x8 { return wf[((long)cb0[j] * nks + (q * 4 + kk)) * 64]; };

    f32x16 acc[4][TM][TN];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[p][i][j][e] = 0.f;

    // fragment rows: tile row m = (ly, lx) -> halo row ly * HW + lx, + the shift; the k-substep kk is applied with ONE xor (kk << 5) (conv3x3_halo.hip)
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
                                                                  // with the other stage, which the shifts below refill
        const int stage = c & 1;
        const bool halo_more = c + 1 < nchunks;
        // ReLU on read: max(a, 0) for the chunks of `in`, max(a, -inf) = a elsewhere
        const f16 fl = (d.in_relu && c < nca) ? (f16)0.f : -__builtin_inff16();
        const f16x8 floor8 = {fl, fl, fl, fl, fl, fl, fl, fl};
        int s = 0;
#pragma unroll
        for (int sy = 0; sy < 3; ++sy)
#pragma unroll
            for (int sx = 0; sx < 3; ++sx) {
                f16x8 afr[4][TM];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int a_ad = stage * A_BYTES + (a_h0[i] + sy * HW_ + sx) * ROWB + ((fh ^ (((a_lx[i] + sx) >> 1) & 7)) << 4);
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk)
                        afr[kk][i] = __builtin_elementwise_max(*(const f16x8*)(smem + (a_ad ^ (kk << 5))), floor8);
                }
                if (halo_more && sy * 3 + sx < NR) issue_a(c + 1, (c + 1) & 1, sy * 3 + sx);      // one halo round of the next chunk per shift
#pragma unroll
                for (int py = 0; py < 2; ++py)
#pragma unroll
                    for (int px = 0; px < 2; ++px) {
                        if (!(gdt_t4_meets(sy, py) && gdt_t4_meets(sx, px))) continue;
                        const int p = py * 2 + px;
                        const int q = c * 16 + s, qn = q + 1 < nsteps ? q + 1 : q;     // (past the last step: a harmless reload of a fragment that exists)
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
                            for (int i = 0; i < TM; ++i)
#pragma unroll
                                for (int j = 0; j < TN; ++j)
                                    acc[p][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(afr[kk][i], bfr[kk][j], acc[p][i][j], 0, 0, 0);
#pragma unroll
                            for (int j = 0; j < TN; ++j) bfr[kk][j] = load_b(qn, kk, j);      // the next step's fragment, a whole step ahead of its use
                        }
                        ++s;
                    }
            }
    }

#pragma unroll
    for (int p = 0; p < 4; ++p)
        conv_epilogue_f16<BM, BN, WGM, WGN, NT, TM, TN>(d, acc[p], smem, tile_m, tile_n, [&](int row, bool& ok) -> long {
            const int y = y0 + (row >> 4), x = x0 + (row & 15);
            ok = (y < d.H) & (x < d.W);
            return ((long)n * d.OH + 2 * y + (p >> 1)) * d.OW + 2 * x + (p & 1);
        });
}

template <int BN, int WGM, int WGN>
int launch_t4(const ConvLaunch& d, hipStream_t stream) {
    using K = GdtKernel<conv4x4t_halo_kernel<BN, WGM, WGN>, (int)t4_lds_bytes<BN, WGM, WGN>()>;
    int unused = 0;
    GDT_CHECK(K::figure(unused));
    return K::launch(gdt_grid_for_tiles((int)gdt_patches(d.N, d.H, d.W, PH), d.CoutPad / BN), WGM * WGN * 64, stream, d);
}

GDT_KNOB_LAUNCH(knob_mode, "GDT_CONV4X4T_HALO", 1)           // 0: the layer runs as four phase launches of the generic implicit GEMM over the concatenated input (A/B
                                                             // inside one process)

}  // namespace

// Eligibility: ConvTranspose2d(k4, s2, p1) as its own plain launch -- both inputs' channel counts multiples of 64 (the second may be absent), the
// fragment-ordered weights in the step order above, fp16 NHWC output in whole 64-column tiles, nothing in the epilogue but bias and ReLU.  Any map size: ragged
// patches at the right and bottom edges and maps smaller than a patch (down to 1 x 1) are the kernel's business.
bool gdt_conv4x4t_halo_eligible(const ConvLaunch& d) {
    const bool shape = d.ntaps == 16 && d.TW == 4 && d.sy == 1 && d.sx == 1 && d.osy == 2 && d.osx == 2 && !d.pad_reflect && d.Cin >= 64 && d.Cin % 64 == 0 &&
                       d.in2_cin >= 0 && d.in2_cin % 64 == 0 && (d.in2 != nullptr) == (d.in2_cin > 0) && d.Kpad == 16 * (d.Cin + d.in2_cin) &&
                       d.OHg == d.H && d.OWg == d.W && d.OH == 2 * d.H && d.OW == 2 * d.W && d.H >= 1 && d.W >= 1 && d.N >= 1;
    if (!shape || !d.in || !d.w_frag || !d.out || !d.zeros || d.out_f32 || d.Cout % 8 != 0 || d.CoutPad % 64 != 0 || d.CoutPad < d.Cout) return false;
    if (d.in_norm || d.in_res || d.in_out || d.stats || d.res || d.pool2 || d.phase_cout || d.pair_cout || d.x3_form || d.in_f32 || d.leaky != 0.f) return false;
    if (!gdt_offsets_fit(d.N, d.H, d.W, d.Cin > d.in2_cin ? d.Cin : d.in2_cin, 62) || !gdt_offsets_fit(d.N, d.OH, d.OW, 1, 31) || (long)d.Kpad * d.CoutPad >= (1L << 31)) return false;
    return knob_mode() != 0;
}

int gdt_launch_conv4x4t_halo(const ConvLaunch& d, hipStream_t stream, int* variant) {
    GDT_REQUIRE(gdt_conv4x4t_halo_eligible(d), "conv4x4t_halo: not an eligible launch");
    if (variant) *variant = 907064;
    return launch_t4<64, 2, 2>(d, stream);
}
