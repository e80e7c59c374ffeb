// 3x3 / stride-1 / pad-1 convolution, LDS-resident input halo + weights streamed straight into registers (gfx950, MI355X).
//
// Second generation of conv3x3_halo.hip for the hottest layers (the 18 ResnetBlock convs of the generator,
// p2p_networks.py:480-494, and the 256/512-channel 3x3 convs of VGG16 / ResNet-101).  The first kernel keeps both operands in
// LDS and measures out LDS-bound: per (chunk, tap) step a 256x256 tile reads 8 waves x 4 k-substeps x 6 fragments x 1 KB
// = 192 KB from LDS and the DMA writes another 32 KB of weights into it -- ~1800 of the 2048 cycles the MFMAs of the step
// take at 128 B/clk -- and it pays a workgroup barrier per step because the weight tile is shared through LDS.
//
// Here only the activations go through LDS (they are reused by the 9 taps).  The weights are pre-packed on the host in MFMA
// B-fragment order ([cout/32][K/16][lane][8], see net_build.hip) so that one wave-wide 16-byte load is a contiguous 1 KB line
// fetch that lands directly in the B operand registers of v_mfma_f32_32x32x16_f16; each register is re-loaded for the next
// step right after its last MFMA of the current step has issued, a full step (~2000 cycles) ahead of its use.
//   * LDS traffic per step: 128 KB of A fragments (was 224 KB), no weight stages in LDS;
//   * barriers: one per 64-channel chunk (when the halo stage flips) instead of one per tap;
//   * the chunk barrier waits with a COUNTED vmcnt (the 4*TN weight loads of the next step stay in flight).
// The A side (halo staging by LDS-DMA or, with the producer's InstanceNorm folded in, through registers), the swizzle and
// the epilogue are those of conv3x3_halo.hip.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "conv_epilogue.h"
#include "conv_device.h"

namespace {

constexpr int ROWB = 128;          // bytes per LDS row (64 halves of K)
constexpr int HALO_W = 18;
constexpr int PH = 16;
constexpr int HALO_ROWS = (PH + 2) * HALO_W;               // 324
constexpr int HALO_ROWS_PAD = (HALO_ROWS + 7) / 8 * 8;     // 328
constexpr int A_BYTES = HALO_ROWS_PAD * ROWB;
constexpr int NORM_BYTES = 4096 + 64;                      // (scale, shift): two slots of up to 256 input channels + a zero entry
constexpr int BM = PH * 16; static_assert(BM == 256, "16 x 16 patches at file scope");

constexpr int C_OFF = 2 * A_BYTES + NORM_BYTES;            // epilogue transpose patches (one per wave), disjoint from the halo stages

// PHT = 16: two halo stages, the (scale, shift) tables, eight wave-private transpose patches.  PHT = 32 (tall 16 x 32 patches, 64-channel layers): the two
// 77 KB stages fill the LDS; the patches alias the stage the tile has just finished with (one more workgroup barrier per tile)
// SINGLE (one 64-channel chunk per tile, i.e. Cin = 64): ONE halo stage per workgroup and two workgroups per CU instead of a double-buffered one -- a tile is only
// nine tap steps long, so with one wave per SIMD the staging and the epilogue of a lone workgroup lie bare; two of them cover each other's.  (With more chunks the
// accumulators are live while a chunk is staged and all-loads-in-flight staging spills: those shapes keep the double-buffered form.)
template <int BN, int PHT = 16, bool SINGLE = false>
constexpr size_t rb_lds_bytes() {
    if (SINGLE) return PHT == 16 ? (size_t)HALO_ROWS_PAD * ROWB + (size_t)4 * 32 * (64 + 8) * 2 : (size_t)(((PHT + 2) * HALO_W + 7) / 8 * 8) * ROWB;
    return PHT == 16 ? (size_t)C_OFF + (size_t)8 * 32 * (BN / 4 + 8) * 2 : (size_t)2 * (((PHT + 2) * HALO_W + 7) / 8 * 8) * ROWB;
}

// PERSISTENT: the grid is one workgroup per CU; workgroup b walks the virtual block ids b, b + G, b + 2G, ... of the XCD-chunked
// tile mapping (gdt_tile_of_block; G is a multiple of 8, so a workgroup's tiles stay on its XCD).  The chunk pipeline runs
// straight across tile boundaries: the first halo chunk and the first weight slice of the NEXT tile are fetched during the
// last chunk of the current one, and the epilogue's global stores drain while the next tile's MFMAs run (with one workgroup
// per tile every CU reached its epilogue at the same moment: 33 MB of stores in one burst, ~13k idle cycles per tile).
// MODE bits: 1 = the producer's InstanceNorm (+ReLU) is applied while staging; 2 = ... plus a residual; 4 = the transformed
// tensor is written back (it has further consumers).  Built: 0, 1, 5 (norm + write-back), 7 (norm + residual + write-back:
// the ResnetBlock output folded into the next block's first conv).
// CT = true: ConvTranspose2d(k3, s2, p1, op1) (p2p_networks.py:289-300) on the same machinery.  The 16x16 patch is a patch of
// INPUT pixels with a 17x17 halo (one extra row / column, zero past the image); the "taps" are the four input shifts (dy, dx);
// the GEMM columns are the four sub-pixel phases x cout in the paired order of gdt_ctf_column() (weights: Op::ctf in net_internal.h),
// and a wave skips the (shift, phase) blocks that are all zero; the epilogue scatters column blocks to output pixels
// (2y + py, 2x + px).  MODE 3 (norm + residual, no write-back) exists for this form: y9 = y8 + IN(.) feeds only the first
// transposed conv.
// (the body takes its workgroup index and grid size as arguments: the kernel below hands it blockIdx.x and gridDim.x)
template <int BN, int WGM, int WGN, int MODE, bool CT = false, int PHT = 16, bool SINGLE = false>
__device__ __forceinline__ void conv3x3_halo_rb_body(const ConvLaunch& d, const int vblocks, const int bid, const int gdim) {
    constexpr int PH = PHT, BM = PHT * 16;                              // (shadow the 16-row constants of the file scope)
    constexpr bool ALIAS = PHT > 16;                                    // transpose patches inside the consumed halo stage
    static_assert(!SINGLE || (MODE == 0 && !CT && WGM * WGN == 4), "single-stage form: plain input, four waves");
    constexpr bool NORM = (MODE & 1) != 0, RES = (MODE & 2) != 0, WB = (MODE & 4) != 0;
    constexpr int NT = WGM * WGN * 64, RPR = NT / 8;   // threads, halo rows staged per loader round
    constexpr int HW_ = CT ? 17 : HALO_W;                               // halo width / height
    constexpr int HROWS = (CT ? HW_ : PHT + 2) * HW_, HROWS_PAD = (HROWS + 7) / 8 * 8;   // 324 / 328, 289 / 296 (CT), 612 / 616 (tall patches)
    constexpr int A_BYTES = PHT == 16 ? HALO_ROWS_PAD * ROWB : HROWS_PAD * ROWB;         // (shadows the file-scope constant)
    constexpr int NTAP = CT ? 4 : 9;                                    // steps per chunk
    constexpr int NR = (HROWS_PAD + RPR - 1) / RPR;
    constexpr int RPS = (NR + NTAP - 2) / (NTAP - 1);                   // staging rounds per step (1 with eight waves, 2 / 3 with four)
    static_assert(NR <= (NTAP - 1) * RPS && HROWS_PAD * ROWB <= A_BYTES && !(CT && PHT != 16), "halo rounds are spread over the steps of the previous chunk");
    constexpr int WTM = BM / WGM, WTN = BN / WGN;
    constexpr int TM = WTM / 32, TN = WTN / 32;
    static_assert(TM >= 2 && TM % 2 == 0 && TN >= 1 && WTM == 128, "tile shape (one 128-row statistics record per wave row)");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WGN, wn = wave % WGN;

    const int tiles_x = (d.W + 15) >> 4, tiles_y = (d.H + PH - 1) / PH;
    const int tpi = tiles_x * tiles_y, ntm = d.N * tpi, ntn = d.CoutPad / BN;
    auto tile_at = [&](int vb) -> GdtPatch { return gdt_patch_at(vb, vblocks, ntm, ntn, tpi, tiles_x, PH); };
    int vb = bid;
    GdtPatch cur = tile_at(vb);
    if (!cur.valid) return;                   // (validity is monotone in vb: nothing later either)

    // ---- halo loader (column swizzle as conv3x3_halo.hip: chunk' = chunk ^ ((halo column >> 1) & 7)).
    // The halo goes through REGISTERS in every mode (16-byte global load in one tap step, LDS write in the next), not
    // through LDS-DMA: a global_load_lds in flight makes the compiler treat vmcnt as out-of-order ("pending flat") and turn
    // every later wait into vmcnt(0), which would drain the weight prefetch six times per chunk.  For the same reason the
    // whole staging path is branch-free (clamped rows, selected addresses, idempotent duplicate work instead of skipped
    // work): conditional memory operations in the loop body also end in vmcnt(0).
    const int lrow = tid >> 3;
    const bool refl = d.pad_reflect != 0;
    struct Pend { f16x8 raw, res; unsigned goff; bool ok; };
    auto load_piece = [&](const GdtPatch& ta, int chunk, int r) -> Pend {
        // (the empty asm keeps this address arithmetic from being hoisted out of the chunk loop: hoisted, its dozen values per
        // round get spilled, and every scratch reload is a vmcnt(0) of its own)
        int lr = lrow;
        asm volatile("" : "+v"(lr));
        const int h = min(r * RPR + lr, HROWS_PAD - 1);            // rows past the padded halo repeat its last (all-zero) row
        int hy, hx;
        gdt_halo_yx<HW_>(h, hy, hx);
        const int iy = ta.y0 - (CT ? 0 : 1) + hy, ix = ta.x0 - (CT ? 0 : 1) + hx;
        int ry, rx;
        GDT_REFLECT_CLAMP(iy, ix, d.H, d.W, ry, rx)          // always a valid pixel
        const bool inb = ((unsigned)iy < (unsigned)d.H) & ((unsigned)ix < (unsigned)d.W);
        const int q = (lane & 7) ^ ((hx >> 1) & 7);
        Pend p;
        p.goff = ((unsigned)((ta.n * d.H + ry) * d.W + rx) << (d.lc8 + 3)) + (chunk * 8 + q) * 8;      // element offset (< 2^32, checked on the host)
        p.ok = (h < HROWS) & (inb | refl);
        p.raw = *(const f16x8*)(d.in + p.goff);
        if (RES) p.res = *(const f16x8*)(d.in_res + p.goff);
        return p;
    };
    // Fused InstanceNorm (+ReLU, + residual, + write-back) of the producer (p2p_networks.py:29,:272,:505).  (scale, shift) =
    // (rstd, -mean * rstd) of all input channels of the tile's image: two 2 KB slots (Cin <= 256), flipped per tile, and one
    // all-zero entry that padded positions are pointed at (so that they come out as exactly zero without a select).
    float* nlds = (float*)(smem + 2 * A_BYTES);
    constexpr int ZERO_ENTRY = 2 * 512;                            // floats
    auto stage_norm = [&](const GdtPatch& ta, int slot) {
        gdt_stage_norm(nlds, slot, d.in_norm, d.Cin, ta.n, tid, NT);
        if (tid < 4) *(float4*)(nlds + ZERO_ENTRY + tid * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto store_piece = [&](int slot, int stage_off, int r, const Pend& p) {
        const int row = min(r * RPR + lrow, HROWS_PAD - 1);
        f16x8 o, z;
#pragma unroll
        for (int e = 0; e < 8; ++e) z[e] = (f16)0.f;
        if (!NORM) {
            o = p.ok ? p.raw : z;
        } else {
            const int cq = (p.goff >> 3) & ((1 << d.lc8) - 1);                     // chunk * 8 + q
            // (write-back needs the true value of the clamped pixel for the write-back and zeroes the LDS copy afterwards)
            const float4* np4 = (const float4*)(nlds + ((WB || p.ok) ? slot * 512 + cq * 16 : ZERO_ENTRY));
            const float lo = d.in_relu ? 0.f : -3.0e38f;
            const u32x4 rawu = __builtin_bit_cast(u32x4, p.raw), resu = __builtin_bit_cast(u32x4, p.res);
            u32x4 ou;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 v = np4[k];
                ou[k] = RES ? gdt_norm_res_pair(rawu[k], resu[k], v.x, v.y, v.z, v.w, lo) : gdt_norm_pair(rawu[k], v.x, v.y, v.z, v.w);
            }
            o = __builtin_bit_cast(f16x8, ou);
            if (!RES) {                              // ReLU on the packed halves (rounding is monotone and 0 is exact)
                f16x8 lo8;
#pragma unroll
                for (int e = 0; e < 8; ++e) lo8[e] = d.in_relu ? (f16)0.f : (f16)-65504.f;
                o = __builtin_elementwise_max(o, lo8);
            }
        }
        // The transformed tensor is materialised as a side effect (MODE bit 4).  EVERY piece stores the value of its (clamped,
        // reflected) source pixel, halo pieces included: neighbouring patches write identical bits to the same place, which
        // is cheaper than a conditional store (27 % more store traffic, no branch in the loop).
        if (WB) *(f16x8*)(d.in_out + p.goff) = o;
        if (WB || RES) o = p.ok ? o : z;        // (the zero table entry does not cancel a residual)
        *(f16x8*)(smem + stage_off + row * ROWB + ((lane & 7) << 4)) = o;
    };

    // ---- weights: B fragments straight from the fragment-ordered copy (uniform base + lane * 16 bytes)
    const int nks = d.Kpad >> 4, cin16 = d.Cin >> 4;
    const unsigned lane_off = lane * 8;
    f16x8 b[4][TN];
    auto load_b = [&](int kk, int tile_n, long koff) {      // koff: uniform offset (halves) of the step's first k-step
        const f16* wb = d.w_frag + (long)((tile_n * BN + wn * WTN) / 32) * nks * 512;       // uniform
#pragma unroll
        for (int j = 0; j < TN; ++j) b[kk][j] = *(const f16x8*)(wb + ((long)j * nks * 512 + koff + kk * 512) + lane_off);
    };

    // A fragment address = per-lane base (3 values, one per tap column: the swizzle depends on px + tx) ^ (kk << 5)
    //                      + a compile-time offset (tile row block i, tap) that rides in the ds_read offset field
    const int fr = lane & 31, fh = lane >> 5;
    int vt[3];
#pragma unroll
    for (int tx = 0; tx < 3; ++tx)
        vt[tx] = ((wm * (WTM / 16) + (fr >> 4)) * HW_ + (fr & 15)) * ROWB + ((fh ^ ((((fr & 15) + tx) >> 1) & 7)) << 4);
    auto a_frag = [&](int stage_off, int i, int ty, int tx, int kk) -> f16x8 {
        return *(const f16x8*)(smem + ((vt[tx] + stage_off) ^ (kk << 5)) + (i * 2 * HW_ + ty * HW_ + tx) * ROWB);
    };

    const int nchunks = d.Cin >> 6;
    // ---- prologue: weights of step 0, halo of chunk 0 of the first tile
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) load_b(kk, cur.tile_n, 0);
    if (NORM) {
        stage_norm(cur, 0);
        __syncthreads();
    }
    Pend pend[RPS];
    f16x8 afr[2][TM];
    if (!SINGLE) {
#pragma unroll
        for (int r = 0; r < NR; ++r) store_piece(0, 0, r, load_piece(cur, 0, r));
        __syncthreads();
#pragma unroll
        for (int u = 0; u < RPS; ++u) pend[u] = load_piece(cur, 0, 0);      // (placeholder values: overwritten before their first use)
#pragma unroll
        for (int i = 0; i < TM; ++i) afr[0][i] = a_frag(0, i, 0, 0, 0);
    }

    int so = 0;                   // LDS offset of the halo stage of the current chunk (0 or A_BYTES)
    int slot = 0;                 // (scale, shift) slot of the current tile
    for (;;) {
        const GdtPatch nxt = tile_at(vb + gdim);
        if (SINGLE) {                    // the tile's whole halo: every load issued before the first is consumed, then the LDS writes, then the barrier
            Pend pp[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) pp[r] = load_piece(cur, 0, r);
#pragma unroll
            for (int r = 0; r < NR; ++r) store_piece(0, 0, r, pp[r]);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
#pragma unroll
            for (int i = 0; i < TM; ++i) afr[0][i] = a_frag(0, i, 0, 0, 0);
        }
        f32x16 acc[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

        for (int c = 0; c < (SINGLE ? 1 : nchunks); ++c) {
            const bool last = c + 1 == nchunks;
            // the chunk staged during this one: the next chunk of this tile, chunk 0 of the next tile, or -- when nothing
            // follows -- chunk 0 of this tile once more (idempotent, never read)
            const bool to_next = last && nxt.valid;
            const GdtPatch sta = to_next ? nxt : cur;
            const int sc = last ? 0 : c + 1, sslot = to_next ? slot ^ 1 : slot;
            // the next tile's (scale, shift) table goes in one chunk ahead of its first use (published by this chunk's barrier)
            if (NORM && nxt.valid && c == nchunks - 2) stage_norm(nxt, slot ^ 1);
            // (CT) which of this wave's two column blocks have a non-zero weight block for input shift t
            const int ct_pair = CT ? (((cur.tile_n * WGN + wn) / (d.phase_cout >> 5)) & 1) : 0;
            const unsigned ct_m0 = ct_pair == 0 ? 0x1u : 0x3u, ct_m1 = ct_pair == 0 ? 0xFu : 0x5u;
#pragma unroll
            for (int t = 0; t < NTAP; ++t) {
                const int ty = CT ? (t >> 1) : t / 3, tx = CT ? (t & 1) : t - ty * 3;
                const int nty = CT ? ((t + 1) >> 1) : (t + 1) / 3, ntx = CT ? ((t + 1) & 1) : (t + 1) - nty * 3;     // next tap of this chunk
                // K offset of the next step's weight slice
                // (after the very last step this fetches the first slice again: unconditional loads keep the code straight-line,
                // which is what lets the compiler wait with exact vmcnt counts instead of vmcnt(0))
                const long noff = (long)(t < NTAP - 1 ? (t + 1) * cin16 + c * 4 : sc * 4) * 512;
                const int ntile_n = (t == NTAP - 1 && last) ? nxt.tile_n : cur.tile_n;         // (tile_at: 0 when there is no next tile)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const int cu = kk & 1, nx = cu ^ 1;
                    if (kk < 3) {
#pragma unroll
                        for (int i = 0; i < TM; ++i) afr[nx][i] = a_frag(so, i, ty, tx, kk + 1);
                    } else if (t < NTAP - 1) {            // first fragments of the next tap: same halo stage, no barrier between
#pragma unroll
                        for (int i = 0; i < TM; ++i) afr[nx][i] = a_frag(so, i, nty, ntx, 0);
                    }
                    if (!SINGLE && kk == 2) {    // halo of the next chunk: RPS pieces per step, written a step after their load
#pragma unroll
                        for (int u = 0; u < RPS; ++u) {
                            if (t >= 1 && (t - 1) * RPS + u < NR) store_piece(sslot, A_BYTES - so, (t - 1) * RPS + u, pend[u]);
                            if (t * RPS + u < NR) pend[u] = load_piece(sta, sc, t * RPS + u);
                        }
                    }
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        if (!CT || (((j == 0 ? ct_m0 : ct_m1) >> t) & 1u)) {           // (wave-uniform; no memory operation inside)
#pragma unroll
                            for (int i = 0; i < TM; ++i)
                                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(b[kk][j], afr[cu][i], acc[i][j], 0, 0, 0);     // D[cout][pixel]
                        }
                    load_b(kk, ntile_n, noff);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (!last) {
                // the other halo stage becomes current: own DMA rounds landed (everything older than the 4*TN weight loads
                // of the next step), own LDS writes done, then the workgroup barrier
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                so = A_BYTES - so;
#pragma unroll
                for (int i = 0; i < TM; ++i) afr[0][i] = a_frag(so, i, 0, 0, 0);
            }
        }

        // ------------------------------------------------------------ tile end.  One barrier, as at every chunk end: all waves
        // are done with the last halo stage, and the next tile's first stage (written during the last chunk) is visible.
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");

        // ------------------------------------------------------------ epilogue, WAVE-PRIVATE: no workgroup barrier in it, so a
        // wave runs through it and on into the next tile on its own.  MFMA operands are swapped (D = W * A^T): lane (fr, fh)
        // holds pixel fr of row block i and, in registers 4g .. 4g+3, the four consecutive output channels 8g + 4fh .. +3 of
        // column block j.  Per 32-pixel row block (= two patch rows) the wave transposes its 32 x 64 slice through a private
        // 4.6 KB LDS patch (8-byte writes, 16-byte reads) and stores one full 128-byte line per pixel; bias, ReLU, residual
        // (+ReLU), fused MaxPool2d(2,2), sub-pixel scatter (CT) on the way.  InstanceNorm statistics: the wave's 128 rows are
        // one record; each lane owns an 8-channel group, sums the fp16 values it stores, lanes sharing a group are merged by a
        // fixed butterfly -- no cross-wave step (the four waves of a row write disjoint channel ranges of the record).
        if (!(d.dbg & 4)) {
            constexpr int PCP = WTN + 8;                                   // halves per patch row (64 + 8)
            f16* patch = (f16*)(smem + (ALIAS ? so : (SINGLE ? A_BYTES : C_OFF))) + wave * (32 * PCP);
            const bool relu_now = d.relu && !d.res;
            const bool has_res = d.res != nullptr;
            int fr_e = fr, fh_e = fh, lane_e = lane;            // (opaque copies: keeps the epilogue's addresses out of the
            asm volatile("" : "+v"(fr_e), "+v"(fh_e), "+v"(lane_e));  //  persistent loop's invariant set, where they would spill)
            const int ch = lane_e & 7;                           // this lane's 8-channel group within the wave's 64 columns
            const int col = cur.tile_n * BN + wn * WTN + ch * 8; // first GEMM column of the group
            int ct_ph = 0, ct_co = 0;
            if (CT) gdt_ctf_column(col, d.phase_cout, ct_ph, ct_co);
            float st1[8], st2[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) { st1[e] = 0.f; st2[e] = 0.f; }
            float4 bvs[TN][4];                                   // bias of this lane's channels, fetched once per tile
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    bvs[j][g] = d.bias ? *(const float4*)(d.bias + cur.tile_n * BN + wn * WTN + j * 32 + 8 * g + 4 * fh_e) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int i = 0; i < TM; ++i) {
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int c4 = j * 32 + 8 * g + 4 * fh_e;
                        const float4 bv = bvs[j][g];
                        const f32x16& a = acc[i][j];
                        float v0 = a[4 * g] + bv.x, v1 = a[4 * g + 1] + bv.y, v2 = a[4 * g + 2] + bv.z, v3 = a[4 * g + 3] + bv.w;
                        if (relu_now) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f); }
                        f16x4 h; h[0] = (f16)v0; h[1] = (f16)v1; h[2] = (f16)v2; h[3] = (f16)v3;
                        *(f16x4*)(patch + fr_e * PCP + c4) = h;
                    }
                const int prow = wm * (WTM / 16) + 2 * i;                  // first of the block's two patch rows
                if (!CT && d.pool2) {
                    // fused MaxPool2d(2, 2): the block's two patch rows give one pooled row of 8 pixels x 8 channel groups
                    const int pc = lane_e >> 3;
                    const f16* r0 = patch + (2 * pc) * PCP + ch * 8;
                    f16x8 v = __builtin_elementwise_max(*(const f16x8*)r0, *(const f16x8*)(r0 + PCP));
                    v = __builtin_elementwise_max(v, __builtin_elementwise_max(*(const f16x8*)(r0 + 16 * PCP), *(const f16x8*)(r0 + 17 * PCP)));
                    const int y = cur.y0 + prow, x = cur.x0 + 2 * pc;
                    if ((y + 1 < d.H) & (x + 1 < d.W) & (col < d.Cout))        // (odd H / W: the last row / column has no partner and is dropped, as MaxPool2d(2, 2) does)
                        *(f16x8*)(d.out + ((long)((cur.n * (d.H >> 1) + (y >> 1)) * (d.W >> 1) + (x >> 1)) * d.Cout + col)) = v;
                    continue;
                }
                unsigned offs[4];
                f16x8 rv[4];
                unsigned okmask = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int px = (lane_e >> 3) + 8 * q;                // pixel of the block: patch row prow + (px >> 4), column px & 15
                    const int y = cur.y0 + prow + (px >> 4), x = cur.x0 + (px & 15);
                    const bool ok = (y < d.H) & (x < d.W) & (col < d.Cout);
                    if (!CT) offs[q] = ok ? (unsigned)(((cur.n * d.H + y) * d.W + x) * d.Cout + col) : 0u;
                    else offs[q] = ok ? (unsigned)(((cur.n * d.OH + 2 * y + (ct_ph >> 1)) * d.OW + 2 * x + (ct_ph & 1)) * d.phase_cout + ct_co) : 0u;
                    okmask |= (ok ? 1u : 0u) << q;
                    if (has_res) rv[q] = *(const f16x8*)(d.res + offs[q]);        // offset 0 is a valid address for masked pieces
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int px = (lane_e >> 3) + 8 * q;
                    f16x8 v = *(const f16x8*)(patch + px * PCP + ch * 8);
                    if (d.stats && ((okmask >> q) & 1u)) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) { const float f = (float)v[e]; st1[e] += f; st2[e] += f * f; }
                    }
                    if (has_res) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            float t = (float)v[e] + (float)rv[q][e];
                            if (d.relu) t = fmaxf(t, 0.f);
                            v[e] = (f16)t;
                        }
                    }
                    if ((okmask >> q) & 1u) *(f16x8*)(d.out + offs[q]) = v;
                }
            }
            if (d.stats) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
#pragma unroll
                    for (int msk = 8; msk < 64; msk <<= 1) { st1[e] += __shfl_xor(st1[e], msk); st2[e] += __shfl_xor(st2[e], msk); }
                    if (CT) { st1[e] += __shfl_xor(st1[e], 4); st2[e] += __shfl_xor(st2[e], 4); }       // the wave's two sub-pixel phases of a channel
                }
                if (!CT && lane_e < 8 && col < d.Cout) {
                    float* dst = d.stats + ((long)(d.stats_tile_base + cur.tile_m * WGM + wm) * 2) * d.Cout + col;
#pragma unroll
                    for (int e = 0; e < 8; ++e) { dst[e] = st1[e]; dst[d.Cout + e] = st2[e]; }
                }
                if (CT && lane_e < 4) {
                    // one record set per phase pair (gdt_ctf_column: pair 0 = phases 0 + 3, pair 1 = phases 1 + 2); the finalize
                    // kernel sums the two sets
                    const int pair = ((cur.tile_n * WGN + wn) / (d.phase_cout >> 5)) & 1;
                    float* dst = d.stats + ((long)(pair * (ntm * WGM) + cur.tile_m * WGM + wm) * 2) * d.phase_cout + ct_co;
#pragma unroll
                    for (int e = 0; e < 8; ++e) { dst[e] = st1[e]; dst[d.phase_cout + e] = st2[e]; }
                }
            }
        } else {                         // ablation: no epilogue (keep the accumulators observable)
            float sacc = 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) sacc += acc[i][j][0] + acc[i][j][15];
            if (sacc == 12345.678f) d.out[0] = (f16)sacc;
        }
        if (!nxt.valid) break;
        if (ALIAS) {                     // the patches lie in the stage the next tile stages its second chunk (or its successor's first) into
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
        cur = nxt; vb += gdim; slot ^= 1;
        if (!SINGLE) {
            so = A_BYTES - so;
#pragma unroll
            for (int i = 0; i < TM; ++i) afr[0][i] = a_frag(so, i, 0, 0, 0);
        }
    }
}

template <int BN, int WGM, int WGN, int MODE, bool CT = false, int PHT = 16, bool SINGLE = false>
__global__ __launch_bounds__(WGM * WGN * 64, SINGLE ? 2 : 1) void conv3x3_halo_rb_kernel(const ConvLaunch d, const int vblocks) {
    conv3x3_halo_rb_body<BN, WGM, WGN, MODE, CT, PHT, SINGLE>(d, vblocks, blockIdx.x, gridDim.x);
}

GDT_KNOB_LATCHED(knob_mode, "GDT_CONV_RB", 1)                // 0 off
GDT_KNOB_LATCHED(knob_narrow, "GDT_CONV_RB128", 1)           // 0: no 128- / 64-column four-wave forms
GDT_KNOB_LATCHED(knob_single, "GDT_CONV_RB_SINGLE", 1)       // 0: no single-stage form (two workgroups per CU) for Cin == 64
GDT_KNOB_LATCHED(knob_split_below, "GDT_RB_SPLIT_BELOW", 192)
GDT_KNOB_LATCHED(knob_persist, "GDT_RB_PERSIST", 1)          // 0: one workgroup per tile; n > 1: n / 2 workgroups per CU
GDT_KNOB_LATCHED(knob_cu_limit, "GDT_CU_LIMIT", 0)           // dev: persistent grid on part of the chip (concurrent-stream experiments)
GDT_KNOB_LATCHED(knob_dbg, "GDT_RB_DBG", 0)                  // timing-only ablation
GDT_KNOB_LATCHED(knob_ct_mode, "GDT_CONV_HALO_CT", 1)        // 0 off
GDT_KNOB_LATCHED(knob_ct_min_tiles, "GDT_CONV_MIN_TILES", 128)   // (batch-1 sweeps: 64-128 best; 512 loses 25 % on a 1024^2 image)

template <int BN, int WGM, int WGN, int MODE, bool CT = false, int PHT = 16, bool SINGLE = false>
int launch_rb(const ConvLaunch& d, hipStream_t stream) {
    constexpr size_t lds = rb_lds_bytes<BN, PHT, SINGLE>();
    static_assert(!SINGLE || 2 * lds <= 160 * 1024, "two workgroups per CU");
    using K = GdtKernel<conv3x3_halo_rb_kernel<BN, WGM, WGN, MODE, CT, PHT, SINGLE>, (int)lds>;
    int cus = 0;
    GDT_CHECK(K::figure(cus));
    const int vblocks = gdt_grid_for_tiles((int)gdt_patches(d.N, d.H, d.W, PHT), d.CoutPad / BN);
    const int persist = knob_persist(), cu_limit = knob_cu_limit();
    int grid = (vblocks < cus || !persist) ? vblocks : cus * (persist > 1 ? persist : 1) / (persist > 1 ? 2 : 1);
    if (cu_limit > 0 && grid > cu_limit) grid = cu_limit;
    if (SINGLE) grid = vblocks < 2 * cus ? vblocks : 2 * cus;
    return K::launch(grid, WGM * WGN * 64, stream, d, vblocks);
}

// the fold modes this file instantiates: the 256-column eight-wave form, plain / norm / norm + write-back / norm + residual + write-back; transposed
// (CT): plain / norm / norm + residual
template <bool CT>
int launch_rb_fold(const ConvLaunch& d, hipStream_t stream) {
    const int mode = gdt_fold_mode(d);
    if (mode == 0) return launch_rb<256, 2, 4, 0, CT>(d, stream);
    if (mode == 1) return launch_rb<256, 2, 4, 1, CT>(d, stream);
    if constexpr (CT) {
        if (mode == 3) return launch_rb<256, 2, 4, 3, true>(d, stream);
    } else {
        if (mode == 5) return launch_rb<256, 2, 4, 5>(d, stream);
        if (mode == 7) return launch_rb<256, 2, 4, 7>(d, stream);
    }
    return gdt_fold_refused(mode);
}

}  // namespace

// Eligible when the LDS-resident form is (gdt_conv_halo_eligible), the fragment-ordered weights exist, the output tile is
// 256 channels wide and -- with a folded InstanceNorm -- the (scale, shift) tables of two images fit their 4 KB and there
// are at least two channel chunks (the next tile's table is staged one chunk ahead).
bool gdt_conv_halo_rb_eligible(const ConvLaunch& d) {
    // 128 output channels (VGG16 conv2_x, HED): the four-wave form, 2 x 2 waves of the same 128 x 64 wave tile (plain input only)
    const int narrow = knob_narrow();
    const bool plain = !d.in_norm && !d.in_res && !d.in_out && !d.stats;
    bool n128 = narrow && d.CoutPad == 128 && plain;
    // 64 output channels (VGG16 conv1_2, HED): 4 x 1 waves on a tall 16 x 32 patch; at most 15 % of the patch rows may hang over the image
    if (narrow && d.CoutPad == 64 && plain && (double)d.H / ((d.H + 31) / 32 * 32) >= 0.85) n128 = true;
    if (knob_mode() == 0 || !d.w_frag || (d.CoutPad % 256 != 0 && !n128)) return false;
    if (d.in_norm && (d.Cin > 256 || d.Cin < 128)) return false;
    if (!gdt_offsets_fit(d.N, d.H, d.W, d.Cin) || !gdt_offsets_fit(d.N, d.H, d.W, d.Cout)) return false;
    return gdt_conv_halo_eligible(d);
}

int gdt_launch_conv_halo_rb(const ConvLaunch& d_in, hipStream_t stream) {
    ConvLaunch d = d_in;
    d.dbg = knob_dbg();
    const int single = knob_single();
    if (d.CoutPad == 128) return (single && d.Cin == 64) ? launch_rb<128, 2, 2, 0, false, 16, true>(d, stream) : launch_rb<128, 2, 2, 0>(d, stream);
    if (d.CoutPad == 64) return (single && d.Cin == 64) ? launch_rb<64, 4, 1, 0, false, 32, true>(d, stream) : launch_rb<64, 4, 1, 0, false, 32>(d, stream);
    if (!d.in_norm) {
        // few patches (small images / small batches: ResNet layer3 / 4 on 256^2 inputs, the small levels of a pyramid): 128-column tiles of the four-wave form
        // double the number of workgroups -- every CU gets one wave per SIMD instead of half the CUs getting two
        const long tiles256 = gdt_patches(d.N, d.H, d.W) * (d.CoutPad / 256);
        // ... and so do tile counts that leave the last round of the persistent walk half empty (384 patches on 256 CUs: two rounds for 1.5 rounds of work):
        // the narrow form is ~0.85x as efficient per tile but its 2x finer grain can more than make up for that
        static const int cus = [] { int dev = 0, n = 256; if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 256; return n / 8 * 8; }();
        auto fill = [&](long t) { return (double)t / (double)((t + cus - 1) / cus * cus); };
        const bool tail = fill(tiles256) < 0.85 * fill(2 * tiles256) - 0.02;
        if (knob_narrow() && (tiles256 < knob_split_below() || tail) && !d.in_res && !d.in_out && !d.stats) return launch_rb<128, 2, 2, 0>(d, stream);
    }
    return launch_rb_fold<false>(d, stream);
}

// Transposed form (CT): fused ConvTranspose2d(k3,s2,p1,op1) launch (phase_cout > 0, weights of Op::ctf), 64 or 128 channels per
// phase, enough patches to fill the chip, at most 15 % padding waste; with statistics whole 16x16 patches; a folded InstanceNorm
// needs 128 <= Cin <= 256 (table slots, staged one chunk ahead).
bool gdt_conv_halo_ct_eligible(const ConvLaunch& d) {
    if (knob_ct_mode() == 0 || !d.phase_cout || !d.w_frag || !d.out || d.out_f32 || d.res || d.in_out) return false;
    if ((d.phase_cout != 64 && d.phase_cout != 128) || d.Cout != 4 * d.phase_cout || d.CoutPad != d.Cout || d.Cin % 64 != 0) return false;
    if (d.ntaps != 4 || d.TW != 2 || d.Kpad != 4 * d.Cin || d.pad_reflect) return false;
    if (d.in_norm && (d.Cin > 256 || d.Cin < 128)) return false;
    if (d.in_res && !d.in_norm) return false;
    if (d.stats && ((d.H & 15) || (d.W & 15))) return false;
    if (!gdt_offsets_fit(d.N, d.H, d.W, d.Cin) || !gdt_offsets_fit(d.N, d.OH, d.OW, d.phase_cout)) return false;
    return gdt_enough_tiles(gdt_patches(d.N, d.H, d.W), d.CoutPad / 256, knob_ct_min_tiles()) && gdt_useful_area(d.H, d.W) >= GDT_MIN_USEFUL_AREA;
}

int gdt_launch_conv_halo_ct(const ConvLaunch& d_in, hipStream_t stream) {
    ConvLaunch d = d_in;
    d.dbg = 0;
    return launch_rb_fold<true>(d, stream);
}
