// Streaming top-k retrieval and query expansion on the device: per query the k best database rows without the nq x ndb score matrix, and the
// weighted aggregation that alpha query expansion (aQE) and database-side augmentation (DBA) put on top of it (Radenovic et al., TPAMI 2018).
//
//   topk_scan_kernel<NB>   one workgroup (4 waves) per (tile of 32 NB queries, database slice).  It walks its slice in tiles of 128 rows (32 per
//                          wave); per tile the scores of 128 rows x 32 NB queries are accumulated in registers over d in chunks of 32, both
//                          operands staged through LDS ([row][k], pitch 36 floats) with the next chunk's global loads in flight under the MFMAs.
//                          k beyond d is loaded as zeros (any d, no padded copy); a row or query beyond the end repeats the last one and is
//                          masked at the selection.
//   topk_merge_kernel      one workgroup per query: the `slices` sorted lists of a query -> its k best, sorted.
//
// ARITHMETIC.  v_mfma_f32_32x32x2_f32 on the fp32 descriptors as they are: exact fp32 products, one k-ordered fp32 accumulation per score.  The
// alternative of retrieval.hip (three fp16 MFMA passes on split operands) has about five times the matrix rate but needs hi / lo copies of BOTH
// operands per call (the database included: 2 x ndb x d fp16 written and read again) and a power-of-two friendly K; with f32 inputs the workspace
// holds no operand copy at all and the ranking of near ties never sees an 11-bit operand.  profiles/topk_qe_1gpu.json records this kernel against
// the f16x3 scores GEMM at the same shapes (the GEMM floor); the split variant was not built.
//
// CANDIDATE LISTS.  Per query of the tile a list of `cap` = roundup64(k + 16) (score, row) pairs in LDS, a fill count and the threshold = the
// list's k-th entry at its last compaction (-inf before it holds k).  After a tile every lane holds 16 NB scores of ONE query (MFMA column
// lane & 31); a score that beats the threshold in the strict order (score descending, row ascending) is appended through an LDS counter.  A list
// that would overflow sets a flag; then every list longer than k is compacted by one wave (each entry's rank = the number of entries that beat it,
// counted against the appends and read off the sorted front by binary search: ranks are unique, the k best land sorted at the front, the
// threshold tightens) and the lanes retry what they still hold.  Whatever the order of
// the appends, a list always contains the k best of the rows seen so far, so the result is a function of the strict order alone: the same bits for
// any number of slices and any tile walk.  At the end of the slice every list is compacted once more and written to the workspace.
//
// LDS: operands 128 x 36 + 32 NB x 36 floats (<= 36 KB), lists 32 NB x cap x 8 bytes <= 96 KB, so NB = 4 up to k = 48, 3 up to 112, 2 up to 176,
// else 1: one workgroup per CU.  Registers: 16 NB accumulators + (4 + NB) float4 of prefetch per lane.
//
// SLICES.  A forced number (1 .. 1024) is taken as it is, with the widest query tile.  Left to the library: about two workgroups per CU, at least
// four row tiles per slice, at most 128 slices and at most 15360 list entries per query (the merge's LDS copy); with so few queries that this
// leaves CUs idle the query tile is narrowed (NB 3 -> 2 -> 1), which re-reads the database from L2 but puts every CU to work.
#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/gandtr_hip.h"
#include "gdt_common.h"

namespace {

constexpr size_t ALIGN = 256;
inline size_t align_up(size_t v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }

constexpr int TK_THREADS = 256, TK_ROWS = 128, TK_KC = 32, TK_PITCH = TK_KC + 4;
constexpr int TK_MAX_K = 256, TK_MAX_D = 8192, TK_MAX_SLICES = 1024;
constexpr int TK_LIST_BYTES = 96 * 1024;
constexpr int TK_SCAN_LDS_MAX = (TK_ROWS + 128) * TK_PITCH * 4 + TK_LIST_BYTES + 128 * 16;
constexpr int TK_PER_LANE = 5;                      // cap <= 320 entries, 64 lanes
constexpr int TK_EMPTY = 0x7fffffff;                 // row of "no entry": loses every tie
constexpr int TK_CUS = 256;                          // MI355X
constexpr int TK_TARGET_GROUPS = 2 * TK_CUS;         // workgroups the library aims at when it chooses the slices
constexpr int TK_AUTO_SLICES_MAX = 128;
constexpr int TK_MERGE_THREADS = 1024;
constexpr int TK_MERGE_LDS_ENTRIES = 15360;         // 120 KB of (score, row) pairs: up to this many the merge works on an LDS copy of the lists

#define TK_NEG_INF (-__builtin_inff())

inline int tk_cap(int k) { return (k + 16 + 63) / 64 * 64; }
inline int tk_max_nb(int k) { return std::min(4, TK_LIST_BYTES / (tk_cap(k) * 8 * 32)); }

struct TkPlan { int nb, qtiles, slices, cap; long rows_per_slice; size_t part_s, part_i, part_n, total; };

int tk_plan(long ndb, int nq, int d, int k, int slices, TkPlan& P) {
    GDT_REQUIRE(ndb >= 1 && ndb < (1l << 31) && nq >= 1, "top-k needs 1 <= ndb < 2^31 database rows and nq >= 1 queries");
    GDT_REQUIRE(d >= 1 && d <= TK_MAX_D, "1 <= d <= 8192");
    GDT_REQUIRE(k >= 1 && k <= TK_MAX_K, "1 <= k <= 256");
    GDT_REQUIRE(slices >= 0 && slices <= TK_MAX_SLICES, "0 <= slices <= 1024 (0: chosen by the library)");
    P.cap = tk_cap(k);
    const int blocks = (nq + 31) / 32;
    const long tiles = (ndb + TK_ROWS - 1) / TK_ROWS;
    // the widest query tile the lists allow; with few queries the library narrows it until the (tile, slice) pairs cover the CUs once
    for (int nbmax = tk_max_nb(k); nbmax >= 1; --nbmax) {
        P.qtiles = (blocks + nbmax - 1) / nbmax;
        P.nb = (blocks + P.qtiles - 1) / P.qtiles;
        if (slices != 0) { P.slices = slices; break; }
        long s = std::max(TK_TARGET_GROUPS / P.qtiles, 1);            // rounded down: whole rounds of workgroups over the CUs
        s = std::min<long>(s, std::max<long>(tiles / 4, 1));          // at least four row tiles per slice
        s = std::min<long>(s, TK_MERGE_LDS_ENTRIES / k);               // the merge holds a query's lists in LDS
        P.slices = (int)std::min<long>(s, TK_AUTO_SLICES_MAX);
        if ((long)P.qtiles * P.slices >= TK_CUS) break;
    }
    slices = P.slices;
    P.rows_per_slice = ((ndb + slices - 1) / slices + TK_ROWS - 1) / TK_ROWS * TK_ROWS;
    const size_t lists = (size_t)nq * slices;
    size_t off = 0;
    P.part_s = off; off += align_up(lists * k * sizeof(float));
    P.part_i = off; off += align_up(lists * k * sizeof(int));
    P.part_n = off; off += align_up(lists * sizeof(int));
    P.total = off + ALIGN;
    return GDT_OK;
}

// the strict total order: (s, i) comes before (t, j)
__device__ __forceinline__ bool tk_beats(float s, int i, float t, int j) { return s > t || (s == t && i < j); }

// four consecutive values row[k .. k + 3] of a row of `len` floats; beyond the end (or for a missing row) zeros
__device__ __forceinline__ float4 tk_load4(const float* __restrict__ row, int k, int len, bool vec, bool valid) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!valid) return v;
    if (vec && k + 4 <= len) return *(const float4*)(row + k);
    if (k < len) v.x = row[k];
    if (k + 1 < len) v.y = row[k + 1];
    if (k + 2 < len) v.z = row[k + 2];
    if (k + 3 < len) v.w = row[k + 3];
    return v;
}

__device__ __forceinline__ f32x16 tk_mfma4(const float4 a, const float4 b, f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
    return acc;
}

// row of accumulator register r in a 32 x 32 MFMA result, lane half h (the column is lane & 31)
__device__ __forceinline__ int tk_acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// One wave brings a list of n (<= cap) entries into order and keeps the best min(n, k) at the front.  The first k0 entries are sorted already (what
// the last compaction left), the rest are the appends since.  Ranks by counting, unique in the strict order: an old entry moves down by the number
// of new ones that beat it; a new entry's rank is the number of new ones that beat it plus the length of the sorted prefix that does (binary
// search).  So a compaction costs n x (n - k0) comparisons, not n x n.  Lane l owns entries l, l + 64, ..: nper = cap / 64 of them.  Every lane
// reads all it needs into registers before any lane writes (one instruction stream, LDS in order).  The lane that holds the k-th entry
// publishes the threshold.
__device__ __forceinline__ void tk_compact(float* ls, int* li, int n, int k, int k0, int nper, int lane, float* thr_s, int* thr_i, int* cnt,
                                           int* srt) {
    float es[TK_PER_LANE];
    int ei[TK_PER_LANE], er[TK_PER_LANE];
#pragma unroll
    for (int m = 0; m < TK_PER_LANE; ++m) {
        const int e = lane + 64 * m;
        const bool live = m < nper && e < n;
        es[m] = live ? ls[e] : TK_NEG_INF;
        ei[m] = live ? li[e] : TK_EMPTY;
        er[m] = e < k0 ? e : 0;
    }
#pragma unroll 4
    for (int j = k0; j < n; ++j) {
        const float t = ls[j];
        const int tj = li[j];
#pragma unroll
        for (int m = 0; m < TK_PER_LANE; ++m)
            if (m < nper) er[m] += tk_beats(t, tj, es[m], ei[m]) ? 1 : 0;
    }
#pragma unroll
    for (int m = 0; m < TK_PER_LANE; ++m) {
        const int e = lane + 64 * m;
        if (m < nper && e >= k0 && e < n) {
            int lo = 0, hi = k0;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (tk_beats(ls[mid], li[mid], es[m], ei[m])) lo = mid + 1; else hi = mid;
            }
            er[m] += lo;
        }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int m = 0; m < TK_PER_LANE; ++m) {
        const int e = lane + 64 * m;
        if (m < nper && e < n && er[m] < k) {
            ls[er[m]] = es[m];
            li[er[m]] = ei[m];
            if (er[m] == k - 1) { *thr_s = es[m]; *thr_i = ei[m]; }
        }
    }
    if (lane == 0) { *cnt = n < k ? n : k; *srt = n < k ? n : k; }
}

template <int NB>
__global__ __launch_bounds__(TK_THREADS) void topk_scan_kernel(const float* __restrict__ vecs, const float* __restrict__ qvecs,
                                                               float* __restrict__ part_s, int* __restrict__ part_i, int* __restrict__ part_n,
                                                               int ndb, int nq, int d, int k, int cap, long self_base, int slices,
                                                               long rows_per_slice, int vec_a, int vec_b) {
    constexpr int QT = 32 * NB;
    extern __shared__ __attribute__((aligned(16))) char tk_smem[];
    float* sA = (float*)tk_smem;                       // [128][36]
    float* sB = sA + TK_ROWS * TK_PITCH;               // [QT][36]
    float* ls = sB + QT * TK_PITCH;                    // [QT][cap]
    int* li = (int*)(ls + QT * cap);                   // [QT][cap]
    int* cnt = li + QT * cap;                          // [QT]
    float* thr_s = (float*)(cnt + QT);                 // [QT]
    int* thr_i = (int*)(thr_s + QT);                   // [QT]
    int* srt = thr_i + QT;                             // [QT] length of the sorted prefix

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    const int slice = (int)(blockIdx.x % (unsigned)slices), q0 = (int)(blockIdx.x / (unsigned)slices) * QT;
    const long r0l = (long)slice * rows_per_slice;
    const int r0 = (int)(r0l < ndb ? r0l : ndb), r1 = (int)(r0l + rows_per_slice < ndb ? r0l + rows_per_slice : ndb);
    const int nchunks = (d + TK_KC - 1) / TK_KC;

    for (int e = tid; e < QT; e += TK_THREADS) { cnt[e] = 0; srt[e] = 0; thr_s[e] = TK_NEG_INF; thr_i[e] = TK_EMPTY; }
    __syncthreads();

    // staging: a chunk of A is 128 rows x 8 float4 (thread t: rows t / 8 + 32 m, float4 t % 8), of B 32 NB rows x 8 float4
    const int srow = tid >> 3, sc4 = (tid & 7) * 4;
    // excluded row of this lane's queries (self_base + query), -1 where there is none
    int self_row[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) {
        const long s = self_base >= 0 ? self_base + q0 + c * 32 + j : -1;
        self_row[c] = s >= 0 && s < ndb ? (int)s : -1;
    }

    for (int rb = r0; rb < r1; rb += TK_ROWS) {
        f32x16 acc[NB];
#pragma unroll
        for (int c = 0; c < NB; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
        // a row or query past the end re-reads the last one: its scores are computed and never looked at (the selection masks them), so the
        // loads of a chunk that lies inside d are plain float4 loads with no branch; only the last, partial chunk (or an unaligned block) is guarded
        float4 pa[4], pb[NB];
        const float* ga[4];
        const float* gb[NB];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int row = rb + srow + 32 * m;
            ga[m] = vecs + (size_t)(row < r1 ? row : r1 - 1) * d;
        }
#pragma unroll
        for (int m = 0; m < NB; ++m) {
            const int q = q0 + srow + 32 * m;
            gb[m] = qvecs + (size_t)(q < nq ? q : nq - 1) * d;
        }
        auto fetch = [&](int kc) {
            const int k0 = kc * TK_KC + sc4;
            const bool whole = (kc + 1) * TK_KC <= d;
            if (whole && vec_a) {
#pragma unroll
                for (int m = 0; m < 4; ++m) pa[m] = *(const float4*)(ga[m] + k0);
            } else {
#pragma unroll
                for (int m = 0; m < 4; ++m) pa[m] = tk_load4(ga[m], k0, d, vec_a, true);
            }
            if (whole && vec_b) {
#pragma unroll
                for (int m = 0; m < NB; ++m) pb[m] = *(const float4*)(gb[m] + k0);
            } else {
#pragma unroll
                for (int m = 0; m < NB; ++m) pb[m] = tk_load4(gb[m], k0, d, vec_b, true);
            }
        };
        fetch(0);
        for (int kc = 0; kc < nchunks; ++kc) {
            __syncthreads();                                           // the previous chunk's (or the selection's) LDS reads are done
#pragma unroll
            for (int m = 0; m < 4; ++m) *(float4*)(sA + (srow + 32 * m) * TK_PITCH + sc4) = pa[m];
#pragma unroll
            for (int m = 0; m < NB; ++m) *(float4*)(sB + (srow + 32 * m) * TK_PITCH + sc4) = pb[m];
            __syncthreads();
            if (kc + 1 < nchunks) fetch(kc + 1);
            const float* a_row = sA + (wave * 32 + j) * TK_PITCH + 4 * h;
            const float* b_row = sB + j * TK_PITCH + 4 * h;
#pragma unroll
            for (int kb = 0; kb < TK_KC; kb += 8) {
                const float4 a = *(const float4*)(a_row + kb);
#pragma unroll
                for (int c = 0; c < NB; ++c) acc[c] = tk_mfma4(a, *(const float4*)(b_row + c * 32 * TK_PITCH + kb), acc[c]);
            }
        }

        // selection: acc[c][r] is the score of row rb + 32 wave + tk_acc_row(r, h) for query q0 + 32 c + j
        unsigned long long done = 0;
        const int row_base = rb + wave * 32;
        for (;;) {
            int over = 0;
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                const int ql = c * 32 + j;
                const bool qok = q0 + ql < nq;
                const float ts = thr_s[ql];
                const int ti = thr_i[ql];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned long long bit = 1ull << (c * 16 + r);
                    if (done & bit) continue;
                    const int row = row_base + tk_acc_row(r, h);
                    const float s = acc[c][r];
                    if (qok && row < r1 && row != self_row[c] && tk_beats(s, row, ts, ti)) {
                        const int pos = atomicAdd(&cnt[ql], 1);
                        if (pos < cap) {
                            ls[ql * cap + pos] = s;
                            li[ql * cap + pos] = row;
                            done |= bit;
                        } else {
                            over = 1;
                        }
                    } else {
                        done |= bit;
                    }
                }
            }
            if (!__syncthreads_or(over)) break;
            for (int ql = wave; ql < QT; ql += TK_THREADS / 64) {
                const int n = cnt[ql] < cap ? cnt[ql] : cap;
                if (n > k) tk_compact(ls + ql * cap, li + ql * cap, n, k, srt[ql], cap >> 6, lane, thr_s + ql, thr_i + ql, cnt + ql, srt + ql);
                else if (lane == 0) cnt[ql] = n;
            }
            __syncthreads();
        }
    }

    __syncthreads();
    for (int ql = wave; ql < QT; ql += TK_THREADS / 64) {
        const int q = q0 + ql;
        if (q >= nq) continue;
        const int n = cnt[ql] < cap ? cnt[ql] : cap;
        tk_compact(ls + ql * cap, li + ql * cap, n, k, srt[ql], cap >> 6, lane, thr_s + ql, thr_i + ql, cnt + ql, srt + ql);
        __builtin_amdgcn_wave_barrier();
        const int keep = n < k ? n : k;
        const size_t list = (size_t)q * slices + slice;
        for (int e = lane; e < keep; e += 64) {
            part_s[list * k + e] = ls[ql * cap + e];
            part_i[list * k + e] = li[ql * cap + e];
        }
        if (lane == 0) part_n[list] = keep;
    }
}

// One workgroup per query.  Every list is sorted, so the rank of an entry is its position in its own list plus, per other list, the length of the
// prefix that beats it (binary search); entry e is (list e % slices, position e / slices), so the lanes of a wave sit at about the same depth and
// leave the loop together once the rank reaches k.
__global__ __launch_bounds__(TK_MERGE_THREADS) void topk_merge_kernel(const float* __restrict__ part_s, const int* __restrict__ part_i,
                                                                      const int* __restrict__ part_n, int* __restrict__ ids,
                                                                      float* __restrict__ scores, int k, int slices, int index_base, int in_lds) {
    extern __shared__ __attribute__((aligned(16))) char tk_smem[];
    __shared__ int mn[TK_MAX_SLICES];
    __shared__ int wsum[TK_MERGE_THREADS / 64];
    const int q = blockIdx.x, tid = threadIdx.x;
    const size_t base = (size_t)q * slices;
    const float* S = part_s + base * k;
    const int* I = part_i + base * k;
    int mine = 0;
    for (int l = tid; l < slices; l += TK_MERGE_THREADS) { mn[l] = part_n[base + l]; mine += mn[l]; }
    for (int m = 32; m >= 1; m >>= 1) mine += __shfl_xor(mine, m);
    if ((tid & 63) == 0) wsum[tid >> 6] = mine;
    __syncthreads();
    const int total = slices * k;
    if (in_lds) {
        float* s_l = (float*)tk_smem;
        int* i_l = (int*)(s_l + total);
        for (int e = tid; e < total; e += TK_MERGE_THREADS)
            if (e % k < mn[e / k]) { s_l[e] = S[e]; i_l[e] = I[e]; }                           // slots past a list's count were never written
        S = s_l;
        I = i_l;
    }
    __syncthreads();
    int valid = 0;
    for (int w = 0; w < TK_MERGE_THREADS / 64; ++w) valid += wsum[w];
    for (int e = tid; e < total; e += TK_MERGE_THREADS) {
        const int l = e % slices, p = e / slices;
        if (p >= mn[l]) continue;
        const float s = S[l * k + p];
        const int i = I[l * k + p];
        int rank = p;
        for (int l2 = 0; l2 < slices && rank < k; ++l2) {
            if (l2 == l) continue;
            int lo = 0, hi = mn[l2] < k - rank ? mn[l2] : k - rank;      // a longer prefix puts the rank at k or beyond either way
            const float* s2 = S + l2 * k;
            const int* i2 = I + l2 * k;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (tk_beats(s2[mid], i2[mid], s, i)) lo = mid + 1; else hi = mid;
            }
            rank += lo;
        }
        if (rank < k) {
            ids[(size_t)q * k + rank] = index_base + i;
            scores[(size_t)q * k + rank] = s;
        }
    }
    for (int e = valid + tid; e < k; e += TK_MERGE_THREADS) {           // fewer than k rows in all: the tail
        ids[(size_t)q * k + e] = -1;
        scores[(size_t)q * k + e] = TK_NEG_INF;
    }
}

// out[q] = l2n((base ? base[q] : 0) + sum_j w_j vecs[ids[q][j] - index_base]): one workgroup per query, thread t owns components t, t + 256, ..;
// per component one fmaf chain over j ascending, the norm from per-thread partial sums (components ascending) and a fixed tree over the threads.
constexpr int EX_THREADS = 256;

__global__ __launch_bounds__(EX_THREADS) void expand_kernel(const float* __restrict__ vecs, const float* __restrict__ base, const int* __restrict__ ids,
                                                            const float* __restrict__ scores, float* __restrict__ out, long ndb, int d, int k,
                                                            int index_base, float alpha) {
    __shared__ float x[TK_MAX_D];
    __shared__ float w[TK_MAX_K];
    __shared__ int row[TK_MAX_K];
    __shared__ float red[EX_THREADS];
    const int q = blockIdx.x, tid = threadIdx.x;
    for (int jn = tid; jn < k; jn += EX_THREADS) {
        const int id = ids[(size_t)q * k + jn];
        const long r = (long)id - index_base;
        const bool ok = id >= 0 && r >= 0 && r < ndb;                   // -1 marks a missing entry; an id outside the database is skipped like it
        row[jn] = ok ? (int)r : -1;
        w[jn] = alpha == 0.f ? 1.f : powf(fmaxf(scores[(size_t)q * k + jn], 0.f), alpha);
    }
    __syncthreads();
    float ss = 0.f;
    for (int c = tid; c < d; c += EX_THREADS) {
        float v = base ? base[(size_t)q * d + c] : 0.f;
        for (int jn = 0; jn < k; ++jn) {
            const int r = row[jn];
            if (r >= 0) v = fmaf(w[jn], vecs[(size_t)r * d + c], v);
        }
        x[c] = v;
        ss = fmaf(v, v, ss);
    }
    red[tid] = ss;
    __syncthreads();
    for (int m = EX_THREADS / 2; m >= 1; m >>= 1) {
        if (tid < m) red[tid] += red[tid + m];
        __syncthreads();
    }
    const float den = sqrtf(red[0]) + 1e-6f;
    for (int c = tid; c < d; c += EX_THREADS) out[(size_t)q * d + c] = x[c] / den;
}

template <int NB>
int tk_launch_scan(const TkPlan& P, const float* vecs, const float* qvecs, float* part_s, int* part_i, int* part_n, long ndb, int nq, int d, int k,
                   long self_base, hipStream_t st) {
    const size_t lds = (size_t)(TK_ROWS + 32 * NB) * TK_PITCH * sizeof(float) + (size_t)32 * NB * P.cap * 8 + (size_t)32 * NB * 16;
    int unused = 0;                                                    // the per-device dynamic-LDS set-up of this instantiation, once
    GDT_CHECK((GdtKernel<topk_scan_kernel<NB>, TK_SCAN_LDS_MAX>::figure(unused)));
    GDT_REQUIRE(lds <= (size_t)TK_SCAN_LDS_MAX, "candidate lists beyond the LDS budget");
    const int vec_a = d % 4 == 0 && (uintptr_t)vecs % 16 == 0, vec_b = d % 4 == 0 && (uintptr_t)qvecs % 16 == 0;
    hipLaunchKernelGGL(topk_scan_kernel<NB>, dim3((unsigned)((size_t)P.qtiles * P.slices)), dim3(TK_THREADS), lds, st, vecs, qvecs, part_s, part_i,
                       part_n, (int)ndb, nq, d, k, P.cap, self_base, P.slices, P.rows_per_slice, vec_a, vec_b);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

}  // namespace

extern "C" {

int gdt_retrieval_topk_workspace_bytes(long ndb, int nq, int d, int k, int slices, size_t* bytes) {
    GDT_REQUIRE(bytes != nullptr, "bytes");
    TkPlan P;
    int rc = tk_plan(ndb, nq, d, k, slices, P);
    if (rc != GDT_OK) return rc;
    *bytes = P.total;
    return GDT_OK;
}

int gdt_retrieval_topk(const float* vecs, const float* qvecs, int* ids, float* scores, long ndb, int nq, int d, int k, int index_base, long self_base,
                       int slices, void* workspace, size_t workspace_bytes, void* stream) {
    GDT_REQUIRE(vecs && qvecs && ids && scores && workspace, "null buffer");
    TkPlan P;
    int rc = tk_plan(ndb, nq, d, k, slices, P);
    if (rc != GDT_OK) return rc;
    GDT_REQUIRE(index_base >= 0 && (long)index_base + ndb <= 0x7fffffffl, "index_base + ndb must fit an int32 id");
    GDT_REQUIRE(self_base >= -1, "self_base is a database row or -1");
    GDT_REQUIRE((long)P.qtiles * P.slices < (1l << 31), "too many (query tile, slice) pairs for one launch");
    if (P.total > workspace_bytes) {
        gdt_set_error("workspace too small: need " + std::to_string(P.total) + " bytes, got " + std::to_string(workspace_bytes));
        return GDT_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)(((uintptr_t)workspace + ALIGN - 1) / ALIGN * ALIGN);
    float* part_s = (float*)(ws + P.part_s);
    int* part_i = (int*)(ws + P.part_i);
    int* part_n = (int*)(ws + P.part_n);
    switch (P.nb) {
        case 1: rc = tk_launch_scan<1>(P, vecs, qvecs, part_s, part_i, part_n, ndb, nq, d, k, self_base, st); break;
        case 2: rc = tk_launch_scan<2>(P, vecs, qvecs, part_s, part_i, part_n, ndb, nq, d, k, self_base, st); break;
        case 3: rc = tk_launch_scan<3>(P, vecs, qvecs, part_s, part_i, part_n, ndb, nq, d, k, self_base, st); break;
        default: rc = tk_launch_scan<4>(P, vecs, qvecs, part_s, part_i, part_n, ndb, nq, d, k, self_base, st); break;
    }
    if (rc != GDT_OK) return rc;
    const int in_lds = (long)P.slices * k <= TK_MERGE_LDS_ENTRIES;
    const size_t lds = in_lds ? (size_t)P.slices * k * 8 : 0;
    int unused = 0;
    GDT_CHECK((GdtKernel<topk_merge_kernel, TK_MERGE_LDS_ENTRIES * 8>::figure(unused)));
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)nq), dim3(TK_MERGE_THREADS), lds, st, (const float*)part_s, (const int*)part_i, (const int*)part_n,
                       ids, scores, k, P.slices, index_base, in_lds);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

int gdt_retrieval_expand(const float* vecs, const float* base, const int* ids, const float* scores, float* out, long ndb, int nq, int d, int k,
                         int index_base, float alpha, void* stream) {
    GDT_REQUIRE(vecs && ids && scores && out, "null buffer");
    GDT_REQUIRE(ndb >= 1 && nq >= 1, "ndb, nq >= 1");
    GDT_REQUIRE(d >= 1 && d <= TK_MAX_D, "1 <= d <= 8192");
    GDT_REQUIRE(k >= 1 && k <= TK_MAX_K, "1 <= k <= 256");
    GDT_REQUIRE(alpha >= 0.f, "alpha >= 0 (0: unweighted)");
    hipLaunchKernelGGL(expand_kernel, dim3((unsigned)nq), dim3(EX_THREADS), 0, (hipStream_t)stream, vecs, base, ids, scores, out, ndb, d, k, index_base,
                       alpha);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

}  // extern "C"
