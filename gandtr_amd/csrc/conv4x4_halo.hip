// 4x4 / zero-pad-1 convolution at stride 1 or 2 with an LDS-resident input halo and weights streamed into registers (gfx950, MI355X).
//
// Layers: the three middle convs of the PatchGAN discriminator (NLayerDiscriminator, p2p_networks.py:539-561): 64 -> 128 and 128 -> 256 at stride 2,
// 256 -> 512 at stride 1 -- 98 % of its FLOPs.  The generic implicit GEMM stages the A operand once per tap, sixteen times here.
//
// One workgroup owns a patch of PH x 16 OUTPUT pixels of one image and BN output channels.  Per 64-channel chunk it stages the input halo of the patch ONCE
// (global -> LDS DMA, zero padding and ragged image edges resolved in the per-lane source address) and runs all 16 taps against it by offsetting the fragment
// row: output pixel (py, px), tap (ty, tx) reads halo pixel (S py + ty, S px + tx).
//   stride 1: halo (PH + 3) x 19 pixels; PH = 16, two halo stages (the next chunk lands while this one's taps run), 8 wavefronts, one workgroup per CU.
//   stride 2: halo (2 PH + 2) x 34 pixels.  With pad 1 the 4x4 kernel at stride 2 is a dense 2x2 convolution over the four input parities -- every (shift,
//             parity) block of the 16 is a real tap, none is zero -- so the halo is read exactly once per tap and nothing is skipped (the stride-2 3x3 form
//             fetches 16 blocks for 9).  PH = 8, ONE 77 KB halo stage, 4 wavefronts: two workgroups share a CU and cover each other's staging.
// The weights are the fragment-ordered copy the builder packs for every fp16 conv with Cin % 64 == 0 ([Cout/32][K/16][64 lanes][8], k = tap * Cin + c:
// net_build.hip frag_order): one wave-wide 16-byte load is a 1 KB line that lands in the B operand of v_mfma_f32_32x32x16_f16; each register is re-loaded for
// the next (chunk, tap) step right after its last MFMA of this step.  Barriers: one per chunk (two with a single stage).  LDS swizzle of the halo image and
// the epilogue (bias with BatchNorm folded, optional ReLU / LeakyReLU, fp16 NHWC through an LDS transpose) are those of conv3x3_halo.hip / conv_epilogue.h.
#include "conv_epilogue.h"
#include "conv_device.h"

namespace {

constexpr int ROWB = 128;          // bytes per LDS row (64 halves of K)

template <int S, int PH> constexpr int halo_w() { return S * 15 + 4; }                      // 19 / 34 columns
template <int S, int PH> constexpr int halo_rows() { return (S * (PH - 1) + 4) * halo_w<S, PH>(); }
template <int S, int PH> constexpr int a_bytes() { return (halo_rows<S, PH>() + 7) / 8 * 8 * ROWB; }

template <int S, int PH, int BN, int WGM, int WGN>
constexpr size_t c4_lds_bytes() {
    constexpr size_t staging = (S == 1 ? 2 : 1) * (size_t)a_bytes<S, PH>();
    constexpr size_t epilogue = conv_epilogue_lds_bytes<PH * 16, BN, WGM, WGN, WGM * WGN * 64>();
    return staging > epilogue ? staging : epilogue;
}

template <int S, int PH, int BN, int WGM, int WGN>
// (two waves per SIMD: 256 registers -- the four-wave forms run two workgroups per CU)
__global__ __launch_bounds__(WGM * WGN * 64, 2) void conv4x4_halo_kernel(const ConvLaunch d) {
    constexpr int NT = WGM * WGN * 64, RPR = NT / 8;           // threads, halo rows staged per loader round
    constexpr int BM = PH * 16;
    constexpr int STAGES = S == 1 ? 2 : 1;
    constexpr int HW_ = halo_w<S, PH>(), HROWS = halo_rows<S, PH>(), HROWS_PAD = (HROWS + 7) / 8 * 8, A_BYTES = a_bytes<S, PH>();
    constexpr int NR = (HROWS_PAD + RPR - 1) / RPR;            // halo staging rounds per chunk
    static_assert(STAGES == 1 || NR <= 16, "halo rounds are spread over the 16 taps of the previous chunk");
    constexpr int WTM = BM / WGM, WTN = BN / WGN;
    constexpr int TM = WTM / 32, TN = WTN / 32;
    static_assert(TM >= 1 && TN >= 1 && WTM % 32 == 0 && WTN % 32 == 0, "tile shape");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;

    const int tiles_x = (d.OW + 15) >> 4, tiles_y = (d.OH + PH - 1) / PH;
    const int tpi = tiles_x * tiles_y, ntm = d.N * tpi, ntn = d.CoutPad / BN;
    int tile_m, tile_n;
    if (!gdt_tile_of_block(blockIdx.x, ntm, ntn, tile_m, tile_n)) return;      // XCD-chunked, see conv_device.h
    const int n = tile_m / tpi, tr = tile_m - n * tpi;
    const int y0 = (tr / tiles_x) * PH, x0 = (tr % tiles_x) << 4;              // first output pixel of the patch
    const int iy0 = S * y0 - 1, ix0 = S * x0 - 1;                               // input pixel of halo position (0, 0)

    // ---- halo loader: round r stages halo rows r * RPR .. + RPR - 1, eight lanes per row (one 16-byte channel group each); the wave's 64 lanes fill 1 KB of
    // LDS linearly, the swizzle chunk' = chunk ^ ((halo column >> 1) & 7) is applied to the SOURCE channel group (conv3x3_halo.hip)
    const int lrow = tid >> 3;
    auto issue_a = [&](int chunk, int stage, int r) {
        if (r * RPR + wave * 8 >= HROWS_PAD) return;               // wave-uniform: rows beyond the padded halo
        const int h = r * RPR + lrow;
        int hy, hx;
        gdt_halo_yx<HW_>(h, hy, hx);
        const int iy = iy0 + hy, ix = ix0 + hx;
        const bool ok = (h < HROWS) & ((unsigned)iy < (unsigned)d.H) & ((unsigned)ix < (unsigned)d.W);      // zero padding, ragged edges, pad rows: zeros
        const int q = (lane & 7) ^ ((hx >> 1) & 7);
        const long pix = ((long)n * d.H + (ok ? iy : 0)) * d.W + (ok ? ix : 0);
        const f16* src = d.in + ((pix << (d.lc8 + 3)) + (chunk * 8 + q) * 8);
        gdt_glds16(ok ? src : d.zeros, smem + stage * A_BYTES + (r * RPR + wave * 8) * ROWB);
    };

    // ---- weights: fragment (column block cb, k-step ks) = 64 lanes x 16 bytes; step (chunk c, tap t) covers k-steps (t * Cin + c * 64) / 16 .. + 3
    const int nks = d.Kpad >> 4;
    const f16x8* wf = (const f16x8*)d.w_frag + lane;
    int cb0[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) cb0[j] = ((tile_n * BN + wn * WTN) >> 5) + j;
    auto load_b = [&](int c, int t, int kk, int j) -> f16x8 {
        const int ks = ((t * d.Cin + (c << 6)) >> 4) + kk;
        return wf[((long)cb0[j] * nks + ks) * 64];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // fragment rows: tile row m = (py, px) -> halo row (S py) * HW + S px; the k-substep kk is applied with ONE xor (kk << 5) (conv3x3_halo.hip)
    const int fr = lane & 31, fh = lane >> 5;
    int a_h0[TM], a_hx[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = wm * WTM + i * 32 + fr;
        a_hx[i] = S * (m & 15); a_h0[i] = S * (m >> 4) * HW_ + a_hx[i];
    }

    const int nchunks = d.Cin >> 6;
    f16x8 bfr[4][TN];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int j = 0; j < TN; ++j) bfr[kk][j] = load_b(0, 0, kk, j);
    if (STAGES == 2) {
#pragma unroll
        for (int r = 0; r < NR; ++r) issue_a(0, 0, r);
    }

    for (int c = 0; c < nchunks; ++c) {
        if (STAGES == 1) {
            if (c > 0) __syncthreads();                           // every wave has read the last tap of the previous chunk
#pragma unroll
            for (int r = 0; r < NR; ++r) issue_a(c, 0, r);
        }
        __syncthreads();                                          // the chunk's halo has landed (the barrier's fence drains the LDS DMA); two stages: and every
                                                                  // wave is done with the other stage, which the taps below refill
        const int stage = STAGES == 2 ? (c & 1) : 0;
        const bool halo_more = STAGES == 2 && c + 1 < nchunks;
#pragma unroll 1
        for (int t = 0; t < 16; ++t) {
            const int ty = t >> 2, tx = t & 3;
            int nc = c, nt = t + 1;
            if (nt == 16) { nt = 0; nc = c + 1 < nchunks ? c + 1 : c; }       // (past the last step: a harmless reload of a fragment that exists)
            int a_ad[TM];
#pragma unroll
            for (int i = 0; i < TM; ++i)
                a_ad[i] = stage * A_BYTES + (a_h0[i] + ty * HW_ + tx) * ROWB + ((fh ^ (((a_hx[i] + tx) >> 1) & 7)) << 4);
            f16x8 afr[2][TM];
#pragma unroll
            for (int i = 0; i < TM; ++i) afr[0][i] = *(const f16x8*)(smem + a_ad[i]);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int cur = kk & 1, nxt = cur ^ 1;
                if (kk + 1 < 4) {
#pragma unroll
                    for (int i = 0; i < TM; ++i) afr[nxt][i] = *(const f16x8*)(smem + (a_ad[i] ^ ((kk + 1) << 5)));
                }
                if (kk == 1 && halo_more && t < NR) issue_a(c + 1, (c + 1) & 1, t);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(afr[cur][i], bfr[kk][j], acc[i][j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < TN; ++j) bfr[kk][j] = load_b(nc, nt, kk, j);      // the next step's fragment, a whole step ahead of its use
            }
        }
    }

    conv_epilogue_f16<BM, BN, WGM, WGN, NT, TM, TN>(d, acc, smem, tile_m, tile_n, [&](int row, bool& ok) -> long {
        const int y = y0 + (row >> 4), x = x0 + (row & 15);
        ok = (y < d.OH) & (x < d.OW);
        return ((long)n * d.OH + y) * d.OW + x;
    });
}

template <int S, int PH, int BN, int WGM, int WGN>
int launch_c4(const ConvLaunch& d, hipStream_t stream) {
    using K = GdtKernel<conv4x4_halo_kernel<S, PH, BN, WGM, WGN>, (int)c4_lds_bytes<S, PH, BN, WGM, WGN>()>;
    int unused = 0;
    GDT_CHECK(K::figure(unused));
    return K::launch(gdt_grid_for_tiles((int)gdt_patches(d.N, d.OH, d.OW, PH), d.CoutPad / BN), WGM * WGN * 64, stream, d);
}

GDT_KNOB_LAUNCH(knob_mode, "GDT_CONV4X4_HALO", 1)            // 0: the 4x4 convs stay on the generic implicit GEMM (A/B inside one process)

}  // namespace

// Eligibility: Conv2d(k4, zero pad 1) at stride 1 or 2 as its own plain launch -- Cin a multiple of 64, the fragment-ordered weights, fp16 NHWC output of
// whole 256 (stride 1) / 128 (stride 2) column tiles, nothing folded into the staging or the epilogue but bias and activation.  Any map size: ragged patches
// at the right and bottom edges and maps smaller than a patch are the kernel's business.
bool gdt_conv4x4_halo_eligible(const ConvLaunch& d) {
    const bool shape = d.ntaps == 16 && d.TW == 4 && d.dy0 == -1 && d.dx0 == -1 && d.dys == 1 && d.dxs == 1 && d.sy == d.sx && (d.sy == 1 || d.sy == 2) &&
                       d.osy == 1 && d.osx == 1 && d.ooy == 0 && d.oox == 0 && !d.pad_reflect && d.Cin % 64 == 0 && d.Kpad == 16 * d.Cin &&
                       d.OHg == d.OH && d.OWg == d.OW && d.OH == (d.H - 2) / d.sy + 1 && d.OW == (d.W - 2) / d.sx + 1 && d.H >= 2 && d.W >= 2;
    if (!shape || !d.w_frag || !d.out || d.out_f32 || d.Cout % 8 != 0 || d.CoutPad % (d.sy == 1 ? 256 : 128) != 0) return false;
    if (d.in_norm || d.in_res || d.in_out || d.stats || d.res || d.pool2 || d.phase_cout || d.pair_cout || d.x3_form || d.in_f32 || d.in2) return false;
    if (!gdt_offsets_fit(d.N, d.H, d.W, d.Cin, 62) || !gdt_offsets_fit(d.N, d.OH, d.OW, 1, 31)) return false;
    return knob_mode() != 0;
}

int gdt_launch_conv4x4_halo(const ConvLaunch& d, hipStream_t stream, int* variant) {
    GDT_REQUIRE(gdt_conv4x4_halo_eligible(d), "conv4x4_halo: not an eligible launch");
    if (d.sy == 1) { if (variant) *variant = 905256; return launch_c4<1, 16, 256, 2, 4>(d, stream); }
    if (d.CoutPad % 256 == 0) { if (variant) *variant = 906256; return launch_c4<2, 8, 256, 1, 4>(d, stream); }
    if (variant) *variant = 906128;
    return launch_c4<2, 8, 128, 2, 2>(d, stream);
}
