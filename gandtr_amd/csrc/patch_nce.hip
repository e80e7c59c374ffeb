// CUT's contrastive head (gfx950, MI355X): PatchSampleF (mdir/components/model/network/p2p_networks.py:595-671) and PatchNCELoss / MultilayerPatchNCELoss
// (mdir/components/optim/criterion/compound_losses.py:113-173), forward only.  Three launches for any number of layers and any batch:
//
//   patch_sample_kernel   one workgroup (4 waves) per (layer, tile of 32 sampled rows): gathers the rows feat[b, :, id] of an fp32 NCHW map into LDS,
//                         runs Linear(C, nc) -> ReLU -> Linear(nc, nc) on v_mfma_f32_32x32x2_f32 (exact fp32: every output is one k-ordered fmaf chain
//                         that starts at the bias), keeps the hidden activations in LDS, writes the rows, then divides them by sqrt(sum x^2) + 1e-7.
//                         use_mlp off: the gathered rows are normalised and written as they are.
//   patch_nce_kernel      one workgroup per (layer, group, tile of 64 q rows): the q tile sits in LDS, every wave streams 32-row blocks of the group's k
//                         (wave w takes blocks w, w + 4, ..), forms the 64 x 32 logits with the same MFMA and folds them into a running (max, sum) per
//                         lane and row.  The [n][n] logits are never written.  The diagonal logit is kept as out_0 and replaced by -10 / T.
//   patch_nce_total_kernel  one workgroup: per layer the row losses added in double (thread t takes t, t + 256, .., then a fixed LDS tree), the mean times
//                         the weight, and the mean over the layers.
//
// GATHER LAYOUT.  A sampled row is strided by H*W in memory and the positions are a random draw, so no arrangement of the lanes makes the reads
// contiguous: every element costs its own cache line.  The 32 lanes of a half-wave take the 32 POSITIONS of the tile in ONE channel (the two halves take
// two neighbouring channels).  Their addresses then scatter over one channel plane (H*W*4 bytes, 16-64 KB), which spreads them over the memory channels and
// lets positions that share a line share the fetch; lanes along the channels of one position would stride by a power-of-two plane size and land on the
// same few channels and cache sets.  The LDS image is [row][channel] (pitch + 4 floats), from which a lane reads its MFMA operand as one 16-byte word.
//
// OPERANDS.  v_mfma_f32_32x32x2_f32 takes A[i = lane & 31][k = lane >> 5] and B[k = lane >> 5][j = lane & 31].  Both operands are read as float4 at
// k = kb + 4 (lane >> 5) .. + 3, so the four MFMAs of an 8-wide k step visit k in the order kb, kb + 4, kb + 1, kb + 5, ..: a fixed permutation, the same
// for every row.  Weights ([out][in], torch's layout) and k rows are read straight from memory (they live in L2): lane (j, h) reads 16 bytes of ITS row.
// Ragged sizes (C, nc or d not a multiple of 4, or unaligned bases) take guarded scalar loads; rows, columns and k beyond the end are zeros.
//
// ORDER.  Every sum has an order fixed by (C, nc, d, n) alone: the fmaf chains by k, the squared norm by 8 threads per row (columns t, t + 8, ..) and a
// fixed xor tree, the log-sum-exp by block order per wave, a fixed xor tree over the 32 lanes, the four waves in index order, out_0 last.  No atomics;
// a row's result does not depend on its tile, on the grid or on the other layers of the launch: bit-identical from run to run, layers batched or alone.
// The kernels trust the device-side ids (the entry cannot see them; the binding checks ids that come from the host).
#include "../../include/gandtr_hip.h"
#include "gdt_common.h"

namespace {

constexpr int PN_THREADS = 256, PN_BM = 32, PN_KC = 64, PN_XP = PN_KC + 4, PN_QM = 64, PN_MAX_DIM = 512;
constexpr float PN_NEG = -3.0e38f;

struct PatchSampleArgs {
    gdt_patch_layer lay[GDT_PATCH_MAX_LAYERS];
    int first_tile[GDT_PATCH_MAX_LAYERS + 1];
    int n_layers, nc, use_mlp;
};
struct PatchNceArgs {
    gdt_patchnce_layer lay[GDT_PATCH_MAX_LAYERS];
    int first_tile[GDT_PATCH_MAX_LAYERS + 1];
    int n_layers;
    float inv_t, weight;
};
static_assert(sizeof(PatchSampleArgs) <= 4096 && sizeof(PatchNceArgs) <= 4096, "kernel arguments are limited to 4 KB");

// four consecutive values row[k .. k + 3] of a row of `len` floats; beyond the end (or for a missing row) zeros
__device__ __forceinline__ float4 pn_load4(const float* __restrict__ row, int k, int len, bool vec, bool valid) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!valid) return v;
    if (vec && k + 4 <= len) return *(const float4*)(row + k);
    if (k < len) v.x = row[k];
    if (k + 1 < len) v.y = row[k + 1];
    if (k + 2 < len) v.z = row[k + 2];
    if (k + 3 < len) v.w = row[k + 3];
    return v;
}

__device__ __forceinline__ f32x16 pn_mfma4(const float4 a, const float4 b, f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
    return acc;
}

// row of accumulator register r in a 32 x 32 MFMA result, lane half h (the column is lane & 31)
__device__ __forceinline__ int pn_acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// A k range of one Linear layer on a 32-row tile: acc[c] += sum_k src[i][k] w[n][k0 + k], k < kn, for the 256 columns n0 .. n0 + 255 (wave w, block c:
// n0 + 64 w + 32 c .. + 31).  src: LDS [32][pitch], zeros beyond the layer's K up to a multiple of 8.
__device__ __forceinline__ void pn_linear(const float* src, int pitch, int k0, int kn, const float* __restrict__ w, int K, int N, int n0, bool vec,
                                          f32x16 (&acc)[2]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
    const float* a_row = src + j * pitch + 4 * h;
    for (int kb = 0; kb < kn; kb += 8) {
        const float4 a = *(const float4*)(a_row + kb);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int n = n0 + wave * 64 + c * 32 + j;
            const float4 b = pn_load4(w + (size_t)n * K, k0 + kb + 4 * h, K, vec, n < N);
            acc[c] = pn_mfma4(a, b, acc[c]);
        }
    }
}

__global__ __launch_bounds__(PN_THREADS) void patch_sample_kernel(const PatchSampleArgs args) {
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    int l = 0;
    while (l + 1 < args.n_layers && (int)blockIdx.x >= args.first_tile[l + 1]) ++l;
    const gdt_patch_layer L = args.lay[l];
    const int C = L.channels, P = L.patches, rows = L.batch * P, nc = args.nc;
    const int row0 = ((int)blockIdx.x - args.first_tile[l]) * PN_BM;
    const int width = args.use_mlp ? nc : C;
    float* out = L.out;
    // this thread gathers for ONE row of the tile (tid & 31): lanes 0-31 take the 32 positions of one channel, lanes 32-63 those of the next channel
    const int gi = tid & 31, grow = row0 + gi;
    const float* gsrc = grow < rows ? L.feat + (size_t)(grow / P) * C * L.hw + L.ids[grow % P] : nullptr;

    if (args.use_mlp) {
        const int ncp = (nc + 7) & ~7, hp = ncp + 4;
        float* xs = lds;                       // [32][PN_XP]   one 64-channel chunk of the gathered rows
        float* hs = lds + PN_BM * PN_XP;       // [32][hp]      hidden activations
        const bool vec1 = C % 4 == 0 && (uintptr_t)L.w1 % 16 == 0, vec2 = nc % 4 == 0 && (uintptr_t)L.w2 % 16 == 0;
        // zero the k padding of the hidden tile once (columns nc .. ncp - 1)
        for (int e = tid; e < PN_BM * (ncp - nc); e += PN_THREADS) hs[(e / (ncp - nc)) * hp + nc + e % (ncp - nc)] = 0.f;
        for (int n0 = 0; n0 < nc; n0 += 256) {                                   // ---- Linear(C, nc) + ReLU -> hs
            f32x16 acc[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int n = n0 + wave * 64 + c * 32 + j;
                const float b = n < nc ? L.b1[n] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[c][r] = b;
            }
            for (int c0 = 0; c0 < C; c0 += PN_KC) {
                __syncthreads();                                                   // the previous chunk has been read
#pragma unroll
                for (int it = 0; it < PN_KC * 32 / PN_THREADS; ++it) {
                    const int cc = (tid >> 5) + it * (PN_THREADS / 32);
                    xs[gi * PN_XP + cc] = (gsrc && c0 + cc < C) ? gsrc[(size_t)(c0 + cc) * L.hw] : 0.f;
                }
                __syncthreads();
                const int kn = C - c0 < PN_KC ? (C - c0 + 7) & ~7 : PN_KC;
                pn_linear(xs, PN_XP, c0, kn, L.w1, C, nc, n0, vec1, acc);
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int n = n0 + wave * 64 + c * 32 + j;
                if (n < nc) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) hs[pn_acc_row(r, h) * hp + n] = fmaxf(acc[c][r], 0.f);
                }
            }
        }
        __syncthreads();
        for (int n0 = 0; n0 < nc; n0 += 256) {                                   // ---- Linear(nc, nc) -> out (not yet normalised)
            f32x16 acc[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int n = n0 + wave * 64 + c * 32 + j;
                const float b = n < nc ? L.b2[n] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[c][r] = b;
            }
            pn_linear(hs, hp, 0, ncp, L.w2, nc, nc, n0, vec2, acc);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int n = n0 + wave * 64 + c * 32 + j;
                if (n < nc) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = row0 + pn_acc_row(r, h);
                        if (row < rows) out[(size_t)row * nc + n] = acc[c][r];
                    }
                }
            }
        }
    } else {
        if (gsrc)                                                                 // the gathered rows as they are
            for (int c = tid >> 5; c < C; c += PN_THREADS / 32) out[(size_t)grow * C + c] = gsrc[(size_t)c * L.hw];
    }
    __syncthreads();                                       // the rows above are this workgroup's own global stores: visible after the barrier
    {                                                      // ---- x / (sqrt(sum x^2) + 1e-7): 8 threads per row
        const int row = row0 + (tid >> 3), t = tid & 7;
        float* y = out + (size_t)(row < rows ? row : 0) * width;
        float ss = 0.f;
        if (row < rows)
            for (int c = t; c < width; c += 8) ss = fmaf(y[c], y[c], ss);
        for (int m = 4; m >= 1; m >>= 1) ss += __shfl_xor(ss, m);
        const float den = sqrtf(ss) + 1e-7f;
        if (row < rows)
            for (int c = t; c < width; c += 8) y[c] = y[c] / den;
    }
}

// (m, s) <- (m, s) + (m2, s2) of a running log-sum-exp: s counts exp(x - m).  One exp: the larger maximum keeps its sum as it is.
__device__ __forceinline__ void pn_merge(float& m, float& s, float m2, float s2) {
    const float e = expf(-fabsf(m - m2));
    s = m2 > m ? fmaf(s, e, s2) : fmaf(s2, e, s);
    m = fmaxf(m, m2);
}

__global__ __launch_bounds__(PN_THREADS) void patch_nce_kernel(const PatchNceArgs args) {
    extern __shared__ __align__(16) float lds[];
    __shared__ float part_m[4][PN_QM], part_s[4][PN_QM], pos[PN_QM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    int l = 0;
    while (l + 1 < args.n_layers && (int)blockIdx.x >= args.first_tile[l + 1]) ++l;
    const gdt_patchnce_layer L = args.lay[l];
    const int d = L.d, n = L.rows / L.groups, tiles = (n + PN_QM - 1) / PN_QM;
    const int t = (int)blockIdx.x - args.first_tile[l], g = t / tiles, i0 = (t % tiles) * PN_QM;
    const int dp = (d + 7) & ~7, qp = dp + 4;
    const float* q = L.q + (size_t)g * n * d;
    const float* k = L.k + (size_t)g * n * d;
    const bool vec = d % 4 == 0 && (uintptr_t)L.k % 16 == 0;
    const float inv_t = args.inv_t;

    for (int e = tid; e < PN_QM * dp; e += PN_THREADS) {                           // q tile -> LDS, zeros beyond the rows and beyond d
        const int i = e / dp, c = e % dp;
        lds[i * qp + c] = (i0 + i < n && c < d) ? q[(size_t)(i0 + i) * d + c] : 0.f;
    }
    __syncthreads();

    float rm[2][16], rs[2][16];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) { rm[b][r] = PN_NEG; rs[b][r] = 0.f; }
    const float* a0 = lds + j * qp + 4 * h;
    const float* a1 = a0 + 32 * qp;
    for (int j0 = wave * 32; j0 < n; j0 += 128) {
        f32x16 acc[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[0][r] = 0.f; acc[1][r] = 0.f; }
        const int col = j0 + j;
        const float* krow = k + (size_t)(col < n ? col : 0) * d;
#pragma unroll 4
        for (int kb = 0; kb < dp; kb += 8) {
            const float4 b = pn_load4(krow, kb + 4 * h, d, vec, col < n);
            acc[0] = pn_mfma4(*(const float4*)(a0 + kb), b, acc[0]);
            acc[1] = pn_mfma4(*(const float4*)(a1 + kb), b, acc[1]);
        }
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int il = b * 32 + pn_acc_row(r, h);
                float x = acc[b][r] * inv_t;
                if (i0 + il == col) {                                              // the diagonal: out_0 of its row, then masked
                    pos[il] = x;
                    x = -10.0f * inv_t;
                }
                if (col < n) pn_merge(rm[b][r], rs[b][r], x, 1.f);
            }
    }
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float m = rm[b][r], s = rs[b][r];
            for (int x = 1; x <= 16; x <<= 1) pn_merge(m, s, __shfl_xor(m, x), __shfl_xor(s, x));
            if (j == 0) {
                part_m[wave][b * 32 + pn_acc_row(r, h)] = m;
                part_s[wave][b * 32 + pn_acc_row(r, h)] = s;
            }
        }
    __syncthreads();
    if (tid < PN_QM && i0 + tid < n) {
        float m = part_m[0][tid], s = part_s[0][tid];
        for (int w = 1; w < 4; ++w) pn_merge(m, s, part_m[w][tid], part_s[w][tid]);
        const float p = pos[tid];
        pn_merge(m, s, p, 1.f);
        L.row_loss[(size_t)g * n + i0 + tid] = (m + logf(s)) - p;
    }
}

__global__ __launch_bounds__(PN_THREADS) void patch_nce_total_kernel(const PatchNceArgs args, double* __restrict__ totals) {
    __shared__ double part[PN_THREADS];
    double all = 0.0;
    for (int l = 0; l < args.n_layers; ++l) {
        const float* x = args.lay[l].row_loss;
        const int rows = args.lay[l].rows;
        double acc = 0.0;
        for (int i = threadIdx.x; i < rows; i += PN_THREADS) acc += (double)x[i];
        __syncthreads();
        part[threadIdx.x] = acc;
        __syncthreads();
        for (int m = PN_THREADS / 2; m >= 1; m >>= 1) {
            if ((int)threadIdx.x < m) part[threadIdx.x] += part[threadIdx.x + m];
            __syncthreads();
        }
        const double mean = part[0] * (double)args.weight / (double)rows;
        if (threadIdx.x == 0) totals[l] = mean;
        all += mean;
    }
    if (threadIdx.x == 0) totals[args.n_layers] = all / (double)args.n_layers;
}

}  // namespace

extern "C" {

int gdt_patch_sample(const gdt_patch_layer* layers, int n_layers, int nc, int use_mlp, void* stream) {
    GDT_REQUIRE(layers != nullptr, "gdt_patch_sample: null layer table");
    GDT_REQUIRE(n_layers >= 1 && n_layers <= GDT_PATCH_MAX_LAYERS, "gdt_patch_sample: 1 .. GDT_PATCH_MAX_LAYERS layers");
    GDT_REQUIRE(!use_mlp || (nc >= 1 && nc <= PN_MAX_DIM), "gdt_patch_sample: 1 <= nc <= 512");
    PatchSampleArgs a = {};
    a.n_layers = n_layers; a.nc = nc; a.use_mlp = use_mlp ? 1 : 0;
    long tiles = 0;
    for (int l = 0; l < n_layers; ++l) {
        const gdt_patch_layer& L = layers[l];
        GDT_REQUIRE(L.feat && L.ids && L.out, "gdt_patch_sample: null buffer");
        GDT_REQUIRE(!use_mlp || (L.w1 && L.b1 && L.w2 && L.b2), "gdt_patch_sample: null weights");
        GDT_REQUIRE(L.batch >= 1 && L.channels >= 1 && L.hw >= 1 && L.patches >= 1, "gdt_patch_sample: positive sizes");
        GDT_REQUIRE(L.patches <= L.hw, "gdt_patch_sample: more patches than positions");
        GDT_REQUIRE((long)L.batch * L.channels * L.hw < (1L << 40) && (long)L.batch * L.patches < (1L << 24), "gdt_patch_sample: sizes too large");
        GDT_REQUIRE((uintptr_t)L.feat % 4 == 0 && (uintptr_t)L.ids % 4 == 0 && (uintptr_t)L.out % 4 == 0 && (uintptr_t)L.w1 % 4 == 0 &&
                    (uintptr_t)L.w2 % 4 == 0 && (uintptr_t)L.b1 % 4 == 0 && (uintptr_t)L.b2 % 4 == 0, "gdt_patch_sample: buffer alignment");
        a.lay[l] = L;
        a.first_tile[l] = (int)tiles;
        tiles += ((long)L.batch * L.patches + PN_BM - 1) / PN_BM;
    }
    GDT_REQUIRE(tiles < (1L << 30), "gdt_patch_sample: too many rows");
    a.first_tile[n_layers] = (int)tiles;
    constexpr int LDS = (PN_BM * PN_XP + PN_BM * (PN_MAX_DIM + 4)) * 4;
    int unused = 0;
    GDT_CHECK((GdtKernel<patch_sample_kernel, LDS>::figure(unused)));
    const int lds = use_mlp ? (PN_BM * PN_XP + PN_BM * (((nc + 7) & ~7) + 4)) * 4 : 0;
    hipLaunchKernelGGL(patch_sample_kernel, dim3((unsigned)tiles), dim3(PN_THREADS), lds, (hipStream_t)stream, a);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

int gdt_patchnce_loss(const gdt_patchnce_layer* layers, int n_layers, float inv_temperature, float weight, double* totals, void* stream) {
    GDT_REQUIRE(layers != nullptr && totals != nullptr, "gdt_patchnce_loss: null buffer");
    GDT_REQUIRE(n_layers >= 1 && n_layers <= GDT_PATCH_MAX_LAYERS, "gdt_patchnce_loss: 1 .. GDT_PATCH_MAX_LAYERS layers");
    GDT_REQUIRE(inv_temperature == inv_temperature && inv_temperature > 0.f && weight == weight, "gdt_patchnce_loss: 1 / temperature > 0, weight a number");
    GDT_REQUIRE((uintptr_t)totals % 8 == 0, "gdt_patchnce_loss: buffer alignment");
    PatchNceArgs a = {};
    a.n_layers = n_layers; a.inv_t = inv_temperature; a.weight = weight;
    long tiles = 0;
    int dmax = 1;
    for (int l = 0; l < n_layers; ++l) {
        const gdt_patchnce_layer& L = layers[l];
        GDT_REQUIRE(L.q && L.k && L.row_loss, "gdt_patchnce_loss: null buffer");
        GDT_REQUIRE(L.rows >= 1 && L.d >= 1 && L.groups >= 1, "gdt_patchnce_loss: positive sizes");
        GDT_REQUIRE(L.d <= PN_MAX_DIM, "gdt_patchnce_loss: d <= 512");
        GDT_REQUIRE(L.rows % L.groups == 0, "gdt_patchnce_loss: rows is a multiple of groups");
        GDT_REQUIRE(L.rows < (1 << 24), "gdt_patchnce_loss: too many rows");
        GDT_REQUIRE((uintptr_t)L.q % 4 == 0 && (uintptr_t)L.k % 4 == 0 && (uintptr_t)L.row_loss % 4 == 0, "gdt_patchnce_loss: buffer alignment");
        a.lay[l] = L;
        a.first_tile[l] = (int)tiles;
        tiles += (long)L.groups * ((L.rows / L.groups + PN_QM - 1) / PN_QM);
        if (L.d > dmax) dmax = L.d;
    }
    a.first_tile[n_layers] = (int)tiles;
    constexpr int LDS = PN_QM * (PN_MAX_DIM + 4) * 4;
    int unused = 0;
    GDT_CHECK((GdtKernel<patch_nce_kernel, LDS>::figure(unused)));
    const int lds = PN_QM * (((dmax + 7) & ~7) + 4) * 4;
    hipLaunchKernelGGL(patch_nce_kernel, dim3((unsigned)tiles), dim3(PN_THREADS), lds, (hipStream_t)stream, a);
    GDT_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(patch_nce_total_kernel, dim3(1), dim3(PN_THREADS), 0, (hipStream_t)stream, a, totals);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

}  // extern "C"
