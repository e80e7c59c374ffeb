// Codebooks on the device: the nearest centroids of every local descriptor without the features x centroids distance matrix, the aggregation of the
// descriptors of an image over their centroids (the dense [centroids][dim] descriptor of the reference's grouping layers, grouping.py:104-124) and
// the k-means update built from the two.
//
//   cb_sqnorm_kernel        xx_i = sum_k x_ik^2 (and cc_j): one wave per row, lane l adds components l, l + 64, .. ascending by fmaf, then a fixed
//                           xor tree: an order fixed by D alone, computed ONCE into the workspace, so every tile and slice sees the same bits.
//   cb_scan_kernel<NB, MA>  one workgroup (4 waves) per (tile of 32 NB features, centroid slice).  The tile walk, the staging and the arithmetic are
//                           those of retrieval_topk.hip: centroids are the MFMA rows (128 per tile, 32 per wave), features the columns, x_i . c_j is
//                           one k-ordered fp32 accumulation on v_mfma_f32_32x32x2_f32 (exact products), operands staged through LDS ([row][k], pitch
//                           36 floats) with the next chunk's global loads in flight under the MFMAs; k beyond D is loaded as zeros.
//                           d2 = max(0, fmaf(-2, x.c, xx + cc)).
//   cb_merge_kernel         one wave per feature: the `slices` sorted lists of a feature -> its ma best, dists = sqrtf(d2).
//
// SELECTION.  After a tile every lane holds 16 NB values of d2: 16 centroids for each of NB features (MFMA column lane & 31).  Unlike the k <= 256
// LDS lists of the top-k kernel a lane keeps, per feature, a sorted list of MA (d2, id) pairs in registers (MA = 1, 4 or 8 >= ma) and inserts only
// what beats the list's worst.  A lane meets its centroids in ascending id, so inside a lane "d2 strictly smaller" IS the strict order (d2
// ascending, id ascending).  At the end of the slice the 8 lists of a feature (4 waves x 2 lane halves) meet in LDS (in place of the operand
// tiles); every entry's rank = the number of entries that come before it in the strict order; ranks below ma are written to the workspace.  A list
// always holds the MA best of what its lane saw, so the result is a function of the strict order alone: the same bits for any number of slices
// and any tile walk.  A centroid whose d2 is NaN (a NaN in its row) or +inf is never inserted; an empty slot is (+inf, id 2^31 - 1) and comes out
// as id -1, distance +inf.
//
// AGGREGATION.  Members (feature, slot) with a valid id are brought into (image, centroid, member index) order by a counting sort: integer-atomic
// histogram, exclusive scan, integer-atomic placement, and then every member's rank inside its bin by counting the smaller member indices (they
// are unique, so the order no longer depends on the atomics).  ag_sum_kernel<T, CH>: one workgroup per (image, centroid); thread t owns components
// t, t + T, ..; members are added in member order by one fmaf chain per component; norms by per-thread partial sums (components ascending), the
// xor tree of a wave and the waves in order.  Every (image, centroid) row of `grouped` and of the statistics is written exactly once, untouched
// rows included; no float atomics, two runs give the same bits, an image's rows do not depend on the other images.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/gandtr_hip.h"
#include "gdt_common.h"

namespace {

constexpr size_t ALIGN = 256;
inline size_t align_up(size_t v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }

constexpr int CB_THREADS = 256, CB_ROWS = 128, CB_KC = 32, CB_PITCH = CB_KC + 4;
constexpr int CB_MAX_MA = 8, CB_MAX_D = 8192, CB_MAX_SLICES = 1024;
constexpr int CB_EMPTY = 0x7fffffff;                 // id of "no entry": loses every tie
constexpr int CB_CUS = 256;                          // MI355X
constexpr int CB_TARGET_GROUPS = 2 * CB_CUS;
constexpr int CB_AUTO_SLICES_MAX = 64;
constexpr int CB_LDS_MAX = 64 * 1024;                // 128 features x 8 lists x 8 entries x 8 bytes; the operand tiles need 37.4 KB

#define CB_INF (__builtin_inff())

inline int cb_macap(int ma) { return ma == 1 ? 1 : ma <= 4 ? 4 : 8; }

struct CbPlan { int nb, macap, qtiles, slices; long rows_per_slice; size_t xx, cc, part_d, part_i, total; };

int cb_plan(long F, long K, int D, int ma, int slices, CbPlan& P) {
    GDT_REQUIRE(F >= 1 && F < (1l << 31) && K >= 1 && K < (1l << 31), "nearest needs 1 <= F < 2^31 features and 1 <= K < 2^31 centroids");
    GDT_REQUIRE(D >= 1 && D <= CB_MAX_D, "1 <= D <= 8192");
    GDT_REQUIRE(ma >= 1 && ma <= CB_MAX_MA, "1 <= ma <= 8");
    GDT_REQUIRE(slices >= 0 && slices <= CB_MAX_SLICES, "0 <= slices <= 1024 (0: chosen by the library)");
    P.macap = cb_macap(ma);
    const long blocks = (F + 31) / 32, tiles = (K + CB_ROWS - 1) / CB_ROWS;
    // the widest feature tile; with few features the library narrows it until the (tile, slice) pairs cover the CUs once
    for (int nb = 4; nb >= 1; nb >>= 1) {
        P.nb = nb;
        P.qtiles = (int)((blocks + nb - 1) / nb);
        if (slices != 0) { P.slices = slices; break; }
        long s = std::max<long>(CB_TARGET_GROUPS / P.qtiles, 1);
        s = std::min<long>(s, std::max<long>(tiles / 4, 1));          // at least four centroid tiles per slice
        P.slices = (int)std::min<long>(s, CB_AUTO_SLICES_MAX);
        if ((long)P.qtiles * P.slices >= CB_CUS) break;
    }
    P.rows_per_slice = ((K + P.slices - 1) / P.slices + CB_ROWS - 1) / CB_ROWS * CB_ROWS;
    const size_t lists = (size_t)F * P.slices;
    size_t off = 0;
    P.xx = off; off += align_up((size_t)F * sizeof(float));
    P.cc = off; off += align_up((size_t)K * sizeof(float));
    P.part_d = off; off += align_up(lists * ma * sizeof(float));
    P.part_i = off; off += align_up(lists * ma * sizeof(int));
    P.total = off + ALIGN;
    return GDT_OK;
}

// the strict total order on (d2, id), with the slot as the last word so that empty entries (equal in d2 and id) have unique ranks too
__device__ __forceinline__ bool cb_before(float s, int i, int a, float t, int j, int b) { return s < t || (s == t && (i < j || (i == j && a < b))); }

// four consecutive values row[k .. k + 3] of a row of `len` floats; beyond the end zeros
__device__ __forceinline__ float4 cb_load4(const float* __restrict__ row, int k, int len, bool vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vec && k + 4 <= len) return *(const float4*)(row + k);
    if (k < len) v.x = row[k];
    if (k + 1 < len) v.y = row[k + 1];
    if (k + 2 < len) v.z = row[k + 2];
    if (k + 3 < len) v.w = row[k + 3];
    return v;
}

__device__ __forceinline__ f32x16 cb_mfma4(const float4 a, const float4 b, f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
    return acc;
}

// row of accumulator register r in a 32 x 32 MFMA result, lane half h (the column is lane & 31)
__device__ __forceinline__ int cb_acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__global__ __launch_bounds__(256) void cb_sqnorm_kernel(const float* __restrict__ v, float* __restrict__ out, long n, int d) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const float* p = v + (size_t)row * d;
    float s = 0.f;
    for (int k = lane; k < d; k += 64) s = fmaf(p[k], p[k], s);
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) out[row] = s;
}

template <int NB, int MA>
__global__ __launch_bounds__(CB_THREADS) void cb_scan_kernel(const float* __restrict__ cen, const float* __restrict__ x, const float* __restrict__ cc,
                                                             const float* __restrict__ xx, float* __restrict__ part_d, int* __restrict__ part_i, int K,
                                                             int F, int d, int ma, int slices, long rows_per_slice, int vec_a, int vec_b) {
    constexpr int QT = 32 * NB;
    extern __shared__ __attribute__((aligned(16))) char cb_smem[];
    float* sA = (float*)cb_smem;                       // [128][36]
    float* sB = sA + CB_ROWS * CB_PITCH;               // [QT][36]
    float* sCC = sB + QT * CB_PITCH;                   // [128]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    const int slice = (int)(blockIdx.x % (unsigned)slices), q0 = (int)(blockIdx.x / (unsigned)slices) * QT;
    const long r0l = (long)slice * rows_per_slice;
    const int r0 = (int)(r0l < K ? r0l : K), r1 = (int)(r0l + rows_per_slice < K ? r0l + rows_per_slice : K);
    const int nchunks = (d + CB_KC - 1) / CB_KC;

    float ld[NB][MA];
    int li[NB][MA];
    float xq[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) {
        const int q = q0 + c * 32 + j;
        xq[c] = xx[q < F ? q : F - 1];
#pragma unroll
        for (int m = 0; m < MA; ++m) { ld[c][m] = CB_INF; li[c][m] = CB_EMPTY; }
    }

    // staging: a chunk of A is 128 rows x 8 float4 (thread t: rows t / 8 + 32 m, float4 t % 8), of B 32 NB rows x 8 float4
    const int srow = tid >> 3, sc4 = (tid & 7) * 4;

    for (int rb = r0; rb < r1; rb += CB_ROWS) {
        f32x16 acc[NB];
#pragma unroll
        for (int c = 0; c < NB; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
        // a centroid or feature past the end re-reads the last one: its values are computed and never looked at
        float4 pa[4], pb[NB];
        const float* ga[4];
        const float* gb[NB];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int row = rb + srow + 32 * m;
            ga[m] = cen + (size_t)(row < r1 ? row : r1 - 1) * d;
        }
#pragma unroll
        for (int m = 0; m < NB; ++m) {
            const int q = q0 + srow + 32 * m;
            gb[m] = x + (size_t)(q < F ? q : F - 1) * d;
        }
        auto fetch = [&](int kc) {
            const int k0 = kc * CB_KC + sc4;
            const bool whole = (kc + 1) * CB_KC <= d;
            if (whole && vec_a) {
#pragma unroll
                for (int m = 0; m < 4; ++m) pa[m] = *(const float4*)(ga[m] + k0);
            } else {
#pragma unroll
                for (int m = 0; m < 4; ++m) pa[m] = cb_load4(ga[m], k0, d, vec_a);
            }
            if (whole && vec_b) {
#pragma unroll
                for (int m = 0; m < NB; ++m) pb[m] = *(const float4*)(gb[m] + k0);
            } else {
#pragma unroll
                for (int m = 0; m < NB; ++m) pb[m] = cb_load4(gb[m], k0, d, vec_b);
            }
        };
        fetch(0);
        const float ccv = tid < CB_ROWS ? cc[rb + tid < r1 ? rb + tid : r1 - 1] : 0.f;
        for (int kc = 0; kc < nchunks; ++kc) {
            __syncthreads();                                           // the previous chunk's (or the selection's) LDS reads are done
#pragma unroll
            for (int m = 0; m < 4; ++m) *(float4*)(sA + (srow + 32 * m) * CB_PITCH + sc4) = pa[m];
#pragma unroll
            for (int m = 0; m < NB; ++m) *(float4*)(sB + (srow + 32 * m) * CB_PITCH + sc4) = pb[m];
            if (kc == 0 && tid < CB_ROWS) sCC[tid] = ccv;
            __syncthreads();
            if (kc + 1 < nchunks) fetch(kc + 1);
            const float* a_row = sA + (wave * 32 + j) * CB_PITCH + 4 * h;
            const float* b_row = sB + j * CB_PITCH + 4 * h;
#pragma unroll
            for (int kb = 0; kb < CB_KC; kb += 8) {
                const float4 a = *(const float4*)(a_row + kb);
#pragma unroll
                for (int c = 0; c < NB; ++c) acc[c] = cb_mfma4(a, *(const float4*)(b_row + c * 32 * CB_PITCH + kb), acc[c]);
            }
        }

        // selection: acc[c][r] is x . c of centroid rb + 32 wave + cb_acc_row(r, h) and feature q0 + 32 c + j; ids ascend with r and with rb
        const int row_base = rb + wave * 32;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lr = cb_acc_row(r, h);
            const int row = row_base + lr;
            const float ccr = sCC[wave * 32 + lr];
            const bool rok = row < r1;
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                const float v = fmaf(-2.f, acc[c][r], xq[c] + ccr);
                const float d2 = v > 0.f ? v : 0.f;
                if (rok && v == v && d2 < ld[c][MA - 1]) {
#pragma unroll
                    for (int m = MA - 1; m >= 1; --m) {
                        if (d2 < ld[c][m - 1]) { ld[c][m] = ld[c][m - 1]; li[c][m] = li[c][m - 1]; }
                        else if (d2 < ld[c][m]) { ld[c][m] = d2; li[c][m] = row; }
                    }
                    if (d2 < ld[c][0]) { ld[c][0] = d2; li[c][0] = row; }
                }
            }
        }
    }

    // the 8 lists of a feature meet in LDS, in place of the operand tiles
    __syncthreads();
    float* Ld = (float*)cb_smem;                       // [QT][8][MA]
    int* Li = (int*)(Ld + QT * 8 * MA);
#pragma unroll
    for (int c = 0; c < NB; ++c)
#pragma unroll
        for (int m = 0; m < MA; ++m) {
            const int e = ((c * 32 + j) * 8 + wave * 2 + h) * MA + m;
            Ld[e] = ld[c][m];
            Li[e] = li[c][m];
        }
    __syncthreads();
    for (int e = tid; e < QT * 8 * MA; e += CB_THREADS) {
        const int ql = e / (8 * MA), slot = e % (8 * MA), l = slot / MA, p = slot % MA;
        const int q = q0 + ql;
        if (q >= F) continue;
        const float s = Ld[e];
        const int i = Li[e];
        const float* Lq = Ld + ql * 8 * MA;
        const int* Iq = Li + ql * 8 * MA;
        int rank = p;
        for (int l2 = 0; l2 < 8; ++l2) {
            if (l2 == l) continue;
            for (int p2 = 0; p2 < MA; ++p2) {
                if (!cb_before(Lq[l2 * MA + p2], Iq[l2 * MA + p2], l2 * MA + p2, s, i, slot)) break;      // a list is sorted: nothing further comes before
                ++rank;
            }
        }
        if (rank < ma) {
            const size_t o = ((size_t)q * slices + slice) * ma + rank;
            part_d[o] = s;
            part_i[o] = i;
        }
    }
}

// One wave per feature.  Every list is sorted, so the rank of an entry is its position in its own list plus, per other list, the length of the
// prefix that comes before it.
__global__ __launch_bounds__(256) void cb_merge_kernel(const float* __restrict__ part_d, const int* __restrict__ part_i, int* __restrict__ ids,
                                                       float* __restrict__ dists, int F, int ma, int slices) {
    const long q = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (q >= F) return;
    const int total = slices * ma;
    const float* S = part_d + (size_t)q * total;
    const int* I = part_i + (size_t)q * total;
    for (int e = lane; e < total; e += 64) {
        const int l = e / ma, p = e % ma;
        const float s = S[e];
        const int i = I[e];
        int rank = p;
        for (int l2 = 0; l2 < slices && rank < ma; ++l2) {
            if (l2 == l) continue;
            for (int p2 = 0; p2 < ma; ++p2) {
                if (!cb_before(S[l2 * ma + p2], I[l2 * ma + p2], l2 * ma + p2, s, i, e)) break;
                ++rank;
            }
        }
        if (rank < ma) {
            ids[(size_t)q * ma + rank] = i == CB_EMPTY ? -1 : i;
            dists[(size_t)q * ma + rank] = i == CB_EMPTY ? CB_INF : sqrtf(s);
        }
    }
}

template <int NB, int MA>
int cb_launch_scan(const CbPlan& P, const float* cen, const float* x, const float* cc, const float* xx, float* part_d, int* part_i, long K, long F, int d,
                   int ma, hipStream_t st) {
    const size_t ops = (size_t)(CB_ROWS + 32 * NB) * CB_PITCH * sizeof(float) + CB_ROWS * sizeof(float), lists = (size_t)32 * NB * 8 * MA * 8;
    const size_t lds = std::max(ops, lists);
    int unused = 0;
    GDT_CHECK((GdtKernel<cb_scan_kernel<NB, MA>, CB_LDS_MAX>::figure(unused)));
    GDT_REQUIRE(lds <= (size_t)CB_LDS_MAX, "candidate lists beyond the LDS budget");
    const int vec_a = d % 4 == 0 && (uintptr_t)cen % 16 == 0, vec_b = d % 4 == 0 && (uintptr_t)x % 16 == 0;
    hipLaunchKernelGGL((cb_scan_kernel<NB, MA>), dim3((unsigned)((size_t)P.qtiles * P.slices)), dim3(CB_THREADS), lds, st, cen, x, cc, xx, part_d, part_i,
                       (int)K, (int)F, d, ma, P.slices, P.rows_per_slice, vec_a, vec_b);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

template <int NB>
int cb_launch_scan_ma(const CbPlan& P, const float* cen, const float* x, const float* cc, const float* xx, float* part_d, int* part_i, long K, long F, int d,
                      int ma, hipStream_t st) {
    switch (P.macap) {
        case 1: return cb_launch_scan<NB, 1>(P, cen, x, cc, xx, part_d, part_i, K, F, d, ma, st);
        case 4: return cb_launch_scan<NB, 4>(P, cen, x, cc, xx, part_d, part_i, K, F, d, ma, st);
        default: return cb_launch_scan<NB, 8>(P, cen, x, cc, xx, part_d, part_i, K, F, d, ma, st);
    }
}

// ---------------------------------------------------------------- aggregation ----------------------------------------------------------------

constexpr int AG_THREADS = 256, AG_CHUNK = 2048;      // a scan block: 256 threads x 8 bins
enum { AG_IDEN = 0, AG_ATT, AG_RES, AG_RESATT, AG_NORMRES, AG_NORMRESATT, AG_NORMRESATT2, AG_FEATURE_FNS };
enum { AG_L2NORM = 0, AG_NORMSIGN, AG_SIGMOID, AG_DESCRIPTOR_FNS, AG_MEAN = AG_DESCRIPTOR_FNS };       // AG_MEAN: the k-means update, not part of the public ids

struct AgPlan { long M, B; int nblocks; size_t counts, cursor, start, bsum, tmp, sorted, offsets, total; };

int ag_plan(long F, long K, int ma, int I, AgPlan& P) {
    GDT_REQUIRE(F >= 0 && K >= 1 && I >= 1, "aggregate needs F >= 0 features, K >= 1 centroids and I >= 1 images");
    GDT_REQUIRE(ma >= 1 && ma <= CB_MAX_MA, "1 <= ma <= 8");
    GDT_REQUIRE(F * ma < (1l << 31), "F * ma members must fit an int32");
    GDT_REQUIRE((long)I * K < (1l << 31), "I * K (image, centroid) rows must fit one launch");
    P.M = F * ma;
    P.B = (long)I * K;
    P.nblocks = (int)((P.B + AG_CHUNK - 1) / AG_CHUNK);
    size_t off = 0;
    P.counts = off; off += align_up((size_t)P.B * sizeof(int));
    P.cursor = off; off += align_up((size_t)P.B * sizeof(int));
    P.start = off; off += align_up((size_t)(P.B + 1) * sizeof(int));
    P.bsum = off; off += align_up((size_t)(P.nblocks + 1) * sizeof(int));
    P.tmp = off; off += align_up((size_t)std::max<long>(P.M, 1) * sizeof(int));
    P.sorted = off; off += align_up((size_t)std::max<long>(P.M, 1) * sizeof(int));
    P.offsets = off; off += align_up(2 * sizeof(long long));
    P.total = off + ALIGN;
    return GDT_OK;
}

// the (image, centroid) bin of member e, or -1: an id outside the codebook or a feature outside every image adds nothing
__device__ __forceinline__ long ag_bin(const int* __restrict__ ids, const long long* __restrict__ off, long e, int ma, int I, long K) {
    const int id = ids[e];
    if (id < 0 || id >= K) return -1;
    const long long f = e / ma;
    if (f < off[0] || f >= off[I]) return -1;
    int lo = 0, hi = I - 1;                                           // the last image whose offset is <= f (empty images share an offset)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= f) lo = mid; else hi = mid - 1;
    }
    return (long)lo * K + id;
}

__global__ __launch_bounds__(AG_THREADS) void ag_count_kernel(const int* __restrict__ ids, const long long* __restrict__ off, int* __restrict__ counts,
                                                              long M, int ma, int I, long K) {
    const long e = (long)blockIdx.x * AG_THREADS + threadIdx.x;
    if (e >= M) return;
    const long b = ag_bin(ids, off, e, ma, I, K);
    if (b >= 0) atomicAdd(&counts[b], 1);
}

// exclusive scan of the B counts in three launches: sums of blocks of 2048, their scan by one workgroup, the blocks again
__global__ __launch_bounds__(AG_THREADS) void ag_scan_sums_kernel(const int* __restrict__ counts, int* __restrict__ bsum, long B) {
    __shared__ int red[AG_THREADS];
    const long base = (long)blockIdx.x * AG_CHUNK + threadIdx.x * 8;
    int s = 0;
    for (int m = 0; m < 8; ++m) s += base + m < B ? counts[base + m] : 0;
    red[threadIdx.x] = s;
    __syncthreads();
    for (int m = AG_THREADS / 2; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(1024) void ag_scan_top_kernel(int* __restrict__ bsum, int* __restrict__ start, int nblocks, long B) {
    __shared__ int buf[1024];
    __shared__ int carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nblocks; b0 += 1024) {
        const int v = b0 + tid < nblocks ? bsum[b0 + tid] : 0;
        buf[tid] = v;
        __syncthreads();
        for (int m = 1; m < 1024; m <<= 1) {
            const int t = tid >= m ? buf[tid - m] : 0;
            __syncthreads();
            buf[tid] += t;
            __syncthreads();
        }
        const int c = carry;
        if (b0 + tid < nblocks) bsum[b0 + tid] = c + buf[tid] - v;
        __syncthreads();
        if (tid == 1023) carry = c + buf[1023];
        __syncthreads();
    }
    if (tid == 0) start[B] = carry;
}

__global__ __launch_bounds__(AG_THREADS) void ag_scan_apply_kernel(const int* __restrict__ counts, const int* __restrict__ bsum, int* __restrict__ start,
                                                                   long B) {
    __shared__ int buf[AG_THREADS];
    const int tid = threadIdx.x;
    const long base = (long)blockIdx.x * AG_CHUNK + tid * 8;
    int v[8], s = 0;
    for (int m = 0; m < 8; ++m) { v[m] = base + m < B ? counts[base + m] : 0; s += v[m]; }
    buf[tid] = s;
    __syncthreads();
    for (int m = 1; m < AG_THREADS; m <<= 1) {
        const int t = tid >= m ? buf[tid - m] : 0;
        __syncthreads();
        buf[tid] += t;
        __syncthreads();
    }
    int run = bsum[blockIdx.x] + buf[tid] - s;
    for (int m = 0; m < 8; ++m) {
        if (base + m < B) start[base + m] = run;
        run += v[m];
    }
}

__global__ __launch_bounds__(AG_THREADS) void ag_place_kernel(const int* __restrict__ ids, const long long* __restrict__ off, const int* __restrict__ start,
                                                              int* __restrict__ cursor, int* __restrict__ tmp, long M, int ma, int I, long K) {
    const long e = (long)blockIdx.x * AG_THREADS + threadIdx.x;
    if (e >= M) return;
    const long b = ag_bin(ids, off, e, ma, I, K);
    if (b >= 0) tmp[start[b] + atomicAdd(&cursor[b], 1)] = (int)e;
}

// member indices are unique: the rank of a member inside its bin is the number of smaller ones, whatever order the atomics left
__global__ __launch_bounds__(AG_THREADS) void ag_rank_kernel(const int* __restrict__ ids, const long long* __restrict__ off, const int* __restrict__ start,
                                                             const int* __restrict__ tmp, int* __restrict__ sorted, long M, int ma, int I, long K) {
    const long e = (long)blockIdx.x * AG_THREADS + threadIdx.x;
    if (e >= M) return;
    const long b = ag_bin(ids, off, e, ma, I, K);
    if (b < 0) return;
    const int s0 = start[b], s1 = start[b + 1];
    int rank = 0;
    for (int p = s0; p < s1; ++p) rank += tmp[p] < (int)e ? 1 : 0;
    sorted[s0 + rank] = (int)e;
}

__global__ void ag_single_image_kernel(long long* off, long long F) { off[0] = 0; off[1] = F; }

// the sum of v over the workgroup, the same bits in every thread: the xor tree of a wave, then the waves in order
template <int T>
__device__ __forceinline__ float ag_block_sum(float v, float* red) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    if (T == 64) return v;
    __syncthreads();                                                  // the previous use's reads are done
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = red[0];
    for (int w = 1; w < T / 64; ++w) s += red[w];
    return s;
}

template <int T, int CH>
__global__ __launch_bounds__(T) void ag_sum_kernel(const float* __restrict__ x, const float* __restrict__ att, const float* cen,
                                                   const float* __restrict__ assign, const int* __restrict__ sorted, const int* __restrict__ start,
                                                   float* grouped, float* __restrict__ stats, int* __restrict__ status, long K, int D, int ma, long B,
                                                   int ffn, int dfn, float dparam) {
    __shared__ float red[4];
    const long bin = blockIdx.x;
    const int tid = threadIdx.x;
    const int s0 = start[bin], n = start[bin + 1] - s0;
    const float* cr = cen + (size_t)(bin % K) * D;
    float acc[CH];
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) acc[ch] = 0.f;
    float maxw = 0.f, sumw = 0.f, maxwa = 0.f, sumwa = 0.f, sumwa2 = 0.f;
    const bool needc = ffn >= AG_RES, neednorm = ffn >= AG_NORMRES;
    for (int m = 0; m < n; ++m) {
        const int e = sorted[s0 + m];
        const int f = e / ma;
        const float w = assign ? assign[e] : 1.f;
        const float a = att ? att[f] : 1.f;
        const float* xr = x + (size_t)f * D;
        float v[CH];
        float ss = 0.f;
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) {
            const int d = tid + ch * T;
            v[ch] = d < D ? (needc ? xr[d] - cr[d] : xr[d]) : 0.f;
            ss = fmaf(v[ch], v[ch], ss);
        }
        float mult = 1.f;
        if (ffn == AG_ATT || ffn == AG_RESATT || ffn == AG_NORMRESATT) mult = a;
        if (ffn == AG_NORMRESATT2) mult = a * a;
        if (neednorm) {
            const float den = sqrtf(ag_block_sum<T>(ss, red)) + 1e-6f;
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) v[ch] = v[ch] / den;
        }
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) acc[ch] = fmaf(w, mult * v[ch], acc[ch]);
        const float wa = w * a;
        maxw = fmaxf(maxw, w);
        sumw += w;
        maxwa = fmaxf(maxwa, wa);
        sumwa += wa;
        sumwa2 += w * (a * a);
    }
    float ss = 0.f;
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) ss = fmaf(acc[ch], acc[ch], ss);      // components past D are zeros
    const float nrm = sqrtf(ag_block_sum<T>(ss, red));
    float* out = grouped + (size_t)bin * D;
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
        const int d = tid + ch * T;
        if (d >= D) continue;
        const float s = acc[ch];
        float o;
        if (dfn == AG_L2NORM) o = s / (nrm + 1e-6f);
        else if (dfn == AG_NORMSIGN) o = (s > 0.f ? 1.f : s < 0.f ? -1.f : s) / dparam;
        else if (dfn == AG_SIGMOID) o = 2.f * (1.f / (1.f + expf(-(dparam * s)))) - 1.f;
        else o = n > 0 ? s / (float)n : cr[d];                           // AG_MEAN: a cluster without members keeps its centroid
        out[d] = o;
    }
    if (tid == 0) {
        if (stats) {
            stats[0 * B + bin] = (float)n;
            stats[1 * B + bin] = maxw;
            stats[2 * B + bin] = sumw;
            stats[3 * B + bin] = maxwa;
            stats[4 * B + bin] = sumwa;
            stats[5 * B + bin] = sumwa2;
            stats[6 * B + bin] = nrm;
        }
        if (dfn == AG_MEAN && n == 0) atomicOr(status, 1);
    }
}

int ag_run(const AgPlan& P, const float* x, const float* att, const float* cen, const int* ids, const float* assign, const long long* offsets, float* grouped,
           float* stats, int* status, long K, int D, int ma, int I, int ffn, int dfn, float dparam, char* ws, hipStream_t st) {
    int* counts = (int*)(ws + P.counts);
    int* cursor = (int*)(ws + P.cursor);
    int* start = (int*)(ws + P.start);
    int* bsum = (int*)(ws + P.bsum);
    int* tmp = (int*)(ws + P.tmp);
    int* sorted = (int*)(ws + P.sorted);
    GDT_CHECK_HIP(hipMemsetAsync(ws + P.counts, 0, P.cursor - P.counts + (size_t)P.B * sizeof(int), st));      // the histogram and the cursors
    const unsigned mblocks = (unsigned)((P.M + AG_THREADS - 1) / AG_THREADS);
    if (P.M > 0) hipLaunchKernelGGL(ag_count_kernel, dim3(mblocks), dim3(AG_THREADS), 0, st, ids, offsets, counts, P.M, ma, I, K);
    hipLaunchKernelGGL(ag_scan_sums_kernel, dim3(P.nblocks), dim3(AG_THREADS), 0, st, (const int*)counts, bsum, P.B);
    hipLaunchKernelGGL(ag_scan_top_kernel, dim3(1), dim3(1024), 0, st, bsum, start, P.nblocks, P.B);
    hipLaunchKernelGGL(ag_scan_apply_kernel, dim3(P.nblocks), dim3(AG_THREADS), 0, st, (const int*)counts, (const int*)bsum, start, P.B);
    if (P.M > 0) {
        hipLaunchKernelGGL(ag_place_kernel, dim3(mblocks), dim3(AG_THREADS), 0, st, ids, offsets, (const int*)start, cursor, tmp, P.M, ma, I, K);
        hipLaunchKernelGGL(ag_rank_kernel, dim3(mblocks), dim3(AG_THREADS), 0, st, ids, offsets, (const int*)start, (const int*)tmp, sorted, P.M, ma, I, K);
    }
    GDT_CHECK_HIP(hipGetLastError());
#define AG_LAUNCH(T, CH)                                                                                                                              \
    hipLaunchKernelGGL((ag_sum_kernel<T, CH>), dim3((unsigned)P.B), dim3(T), 0, st, x, att, cen, assign, (const int*)sorted, (const int*)start, grouped, \
                       stats, status, K, D, ma, P.B, ffn, dfn, dparam)
    if (D <= 128) AG_LAUNCH(64, 2);
    else if (D <= 512) AG_LAUNCH(64, 8);
    else if (D <= 2048) AG_LAUNCH(256, 8);
    else AG_LAUNCH(256, 32);
#undef AG_LAUNCH
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

}  // namespace

extern "C" {

int gdt_codebook_nearest_workspace_bytes(long F, long K, int D, int ma, int slices, size_t* bytes) {
    GDT_REQUIRE(bytes != nullptr, "bytes");
    CbPlan P;
    GDT_CHECK(cb_plan(F, K, D, ma, slices, P));
    *bytes = P.total;
    return GDT_OK;
}

int gdt_codebook_nearest(const float* x, const float* c, int* ids, float* dists, long F, long K, int D, int ma, int slices, void* workspace,
                         size_t workspace_bytes, void* stream) {
    GDT_REQUIRE(x && c && ids && dists && workspace, "null buffer");
    CbPlan P;
    GDT_CHECK(cb_plan(F, K, D, ma, slices, P));
    GDT_REQUIRE((long)P.qtiles * P.slices < (1l << 31), "too many (feature tile, slice) pairs for one launch");
    if (P.total > workspace_bytes) {
        gdt_set_error("workspace too small: need " + std::to_string(P.total) + " bytes, got " + std::to_string(workspace_bytes));
        return GDT_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)(((uintptr_t)workspace + ALIGN - 1) / ALIGN * ALIGN);
    float* xx = (float*)(ws + P.xx);
    float* cc = (float*)(ws + P.cc);
    float* part_d = (float*)(ws + P.part_d);
    int* part_i = (int*)(ws + P.part_i);
    hipLaunchKernelGGL(cb_sqnorm_kernel, dim3((unsigned)((F + 3) / 4)), dim3(256), 0, st, x, xx, F, D);
    hipLaunchKernelGGL(cb_sqnorm_kernel, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, st, c, cc, K, D);
    GDT_CHECK_HIP(hipGetLastError());
    int rc;
    switch (P.nb) {
        case 1: rc = cb_launch_scan_ma<1>(P, c, x, cc, xx, part_d, part_i, K, F, D, ma, st); break;
        case 2: rc = cb_launch_scan_ma<2>(P, c, x, cc, xx, part_d, part_i, K, F, D, ma, st); break;
        default: rc = cb_launch_scan_ma<4>(P, c, x, cc, xx, part_d, part_i, K, F, D, ma, st); break;
    }
    if (rc != GDT_OK) return rc;
    hipLaunchKernelGGL(cb_merge_kernel, dim3((unsigned)((F + 3) / 4)), dim3(256), 0, st, (const float*)part_d, (const int*)part_i, ids, dists, (int)F, ma,
                       P.slices);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

int gdt_codebook_aggregate_workspace_bytes(long F, long K, int ma, int n_images, size_t* bytes) {
    GDT_REQUIRE(bytes != nullptr, "bytes");
    AgPlan P;
    GDT_CHECK(ag_plan(F, K, ma, n_images, P));
    *bytes = P.total;
    return GDT_OK;
}

int gdt_codebook_aggregate(const float* x, const float* att, const float* c, const int* ids, const float* assign, const long long* image_offsets,
                           float* grouped, float* stats, long F, long K, int D, int ma, int n_images, int feature_fn, int descriptor_fn,
                           float descriptor_param, void* workspace, size_t workspace_bytes, void* stream) {
    GDT_REQUIRE(c && image_offsets && grouped && stats && workspace, "null buffer");
    GDT_REQUIRE(F == 0 || (x && ids), "null buffer");
    GDT_REQUIRE(D >= 1 && D <= CB_MAX_D, "1 <= D <= 8192");
    GDT_REQUIRE(feature_fn >= 0 && feature_fn < AG_FEATURE_FNS, "feature function: 0 iden, 1 att, 2 res, 3 resatt, 4 normres, 5 normresatt, 6 normresatt2");
    GDT_REQUIRE(descriptor_fn >= 0 && descriptor_fn < AG_DESCRIPTOR_FNS, "descriptor function: 0 l2norm, 1 normsign, 2 sigmoid");
    AgPlan P;
    GDT_CHECK(ag_plan(F, K, ma, n_images, P));
    if (P.total > workspace_bytes) {
        gdt_set_error("workspace too small: need " + std::to_string(P.total) + " bytes, got " + std::to_string(workspace_bytes));
        return GDT_ERR_WORKSPACE;
    }
    char* ws = (char*)(((uintptr_t)workspace + ALIGN - 1) / ALIGN * ALIGN);
    const float dparam = descriptor_fn == AG_NORMSIGN ? (float)sqrt((double)D) : descriptor_param;
    return ag_run(P, x, att, c, ids, assign, image_offsets, grouped, stats, nullptr, K, D, ma, n_images, feature_fn, descriptor_fn, dparam, ws,
                  (hipStream_t)stream);
}

int gdt_kmeans_update_workspace_bytes(long F, long K, size_t* bytes) {
    GDT_REQUIRE(bytes != nullptr, "bytes");
    AgPlan P;
    GDT_CHECK(ag_plan(F, K, 1, 1, P));
    *bytes = P.total;
    return GDT_OK;
}

int gdt_kmeans_update(const float* x, const int* ids, float* c, int* status, long F, long K, int D, void* workspace, size_t workspace_bytes, void* stream) {
    GDT_REQUIRE(x && ids && c && status && workspace, "null buffer");
    GDT_REQUIRE(F >= 1, "k-means needs at least one point");
    GDT_REQUIRE(D >= 1 && D <= CB_MAX_D, "1 <= D <= 8192");
    AgPlan P;
    GDT_CHECK(ag_plan(F, K, 1, 1, P));
    if (P.total > workspace_bytes) {
        gdt_set_error("workspace too small: need " + std::to_string(P.total) + " bytes, got " + std::to_string(workspace_bytes));
        return GDT_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)(((uintptr_t)workspace + ALIGN - 1) / ALIGN * ALIGN);
    long long* off = (long long*)(ws + P.offsets);
    hipLaunchKernelGGL(ag_single_image_kernel, dim3(1), dim3(1), 0, st, off, (long long)F);
    return ag_run(P, x, nullptr, c, ids, nullptr, off, c, nullptr, status, K, D, 1, 1, AG_IDEN, AG_MEAN, 0.f, ws, st);
}

}  // extern "C"
