// Retrieval scoring on the device: the immediate consumer of the all-gathered descriptors.
// Replaces   scores = np.dot(vecs.T, qvecs); ranks = np.argsort(-scores, axis=0)
//   mdir/components/optim/score/cirscore.py:71-73 (evaluation), mdir/external/cirtorch/datasets/traindataset.py:246-279
//   (hard-negative mining: torch.mm + torch.sort).
// scores: one f16x3 GEMM (split-fp16, fp32-class accuracy -- the ranking of near-ties must not depend on 11-bit operands)
// run by the 1x1 path of conv_igemm_x3.hip with M = database size, K = D, N = queries, written directly as [nq][ndb];
// ranks: rocPRIM segmented radix sort (descending) of (score, database index) pairs, one segment per query.
#include <algorithm>
#include <cstring>
#include <string.h>

#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "../../include/gandtr_hip.h"
#include "gdt_common.h"

namespace {

constexpr size_t ALIGN = 256;
inline size_t align_up(size_t v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }

// q [nq][d] fp32 -> hi / lo fp16 [nq_pad][kpad], zero padded
__global__ __launch_bounds__(256) void split_rows_kernel(const float* __restrict__ q, f16* __restrict__ hi, f16* __restrict__ lo, int nq,
                                                         int d, int nq_pad, int kpad) {
    const long total = (long)nq_pad * kpad;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int r = (int)(i / kpad), c = (int)(i % kpad);
        const float x = (r < nq && c < d) ? q[(long)r * d + c] : 0.f;
        const f16 h = (f16)x;
        hi[i] = h;
        lo[i] = (f16)((x - (float)h) * 2048.f);
    }
}

__global__ __launch_bounds__(256) void iota_segments_kernel(int* __restrict__ idx, int* __restrict__ offsets, int nseg, int len, int base) {
    const long total = (long)nseg * len;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) idx[i] = base + (int)(i % len);
    if (blockIdx.x == 0)
        for (int s = threadIdx.x; s <= nseg; s += 256) offsets[s] = s * len;
}

struct Layout { size_t hi, lo, idx, keys, offs, tmp, tmp_bytes, total; int nq_pad, kpad; };

int plan(int ndb, int nq, int d, bool ranks, Layout& L) {
    GDT_REQUIRE(ndb >= 1 && nq >= 1 && d >= 8 && (d & (d - 1)) == 0, "retrieval needs ndb, nq >= 1 and a power-of-two descriptor size >= 8");
    GDT_REQUIRE((long)ndb * nq < (1l << 31), "ndb * nq must stay below 2^31");
    const int bn = gdt_conv_bn(nq);
    L.nq_pad = (nq + bn - 1) / bn * bn;
    L.kpad = (d + 63) / 64 * 64;
    size_t off = 0;
    L.hi = off; off += align_up((size_t)L.nq_pad * L.kpad * sizeof(f16));
    L.lo = off; off += align_up((size_t)L.nq_pad * L.kpad * sizeof(f16));
    L.idx = L.keys = L.offs = L.tmp = off; L.tmp_bytes = 0;
    if (ranks) {
        L.idx = off; off += align_up((size_t)nq * ndb * sizeof(int));
        L.keys = off; off += align_up((size_t)nq * ndb * sizeof(float));
        L.offs = off; off += align_up((size_t)(nq + 1) * sizeof(int));
        size_t tb = 0;
        hipError_t e = rocprim::segmented_radix_sort_pairs_desc(nullptr, tb, (const float*)nullptr, (float*)nullptr, (const int*)nullptr,
                                                                 (int*)nullptr, (unsigned)((size_t)nq * ndb), (unsigned)nq,
                                                                 (const int*)nullptr, (const int*)nullptr, 0, 32, (hipStream_t)0);
        GDT_CHECK_HIP(e);
        L.tmp = off; L.tmp_bytes = tb; off += align_up(tb);
    }
    L.total = off + ALIGN;
    return GDT_OK;
}


// Cluster-aware hard-negative selection (mdir/external/cirtorch/datasets/traindataset.py:256-275): per query walk its ranked pool from the
// best score down and take the first `nnum` images that belong neither to the query's cluster nor to the cluster of an image already taken;
// the statistic of the reference, ||q - p + 1e-6||_2 per chosen negative, is evaluated by the whole wave.  One wave per query: lane 0 walks
// (a dependent chain of two small loads per step), all lanes compute the distances.
__global__ __launch_bounds__(64) void select_negatives_kernel(const int* __restrict__ ranks_t, const int* __restrict__ pool_cluster,
                                                              const int* __restrict__ query_cluster, const float* __restrict__ vecs,
                                                              const float* __restrict__ qvecs, int* __restrict__ neg_pos, float* __restrict__ neg_dist,
                                                              int* __restrict__ status, int ndb, int nq, int d, int nnum, int index_base) {
    const int q = blockIdx.x, lane = threadIdx.x;
    if (q >= nq) return;
    __shared__ int chosen[64];
    if (lane == 0) {
        int used[65];
        int nused = 1, n = 0;
        used[0] = query_cluster[q];
        const int* rk = ranks_t + (size_t)q * ndb;
        for (int r = 0; r < ndb && n < nnum; ++r) {
            const int p = rk[r] - index_base;
            const int c = pool_cluster[p];
            bool seen = false;
            for (int k = 0; k < nused; ++k) seen |= used[k] == c;
            if (!seen) { chosen[n++] = p; used[nused++] = c; }
        }
        for (int k = n; k < nnum; ++k) chosen[k] = -1;
        if (n < nnum) atomicOr(status, 1);          // the pool ran out of clusters: the reference's loop would index past the ranks
    }
    __syncthreads();
    for (int k = 0; k < nnum; ++k) {
        const int p = chosen[k];
        float acc = 0.f;
        if (p >= 0)
            for (int i = lane; i < d; i += 64) {
                const float df = qvecs[(size_t)q * d + i] - vecs[(size_t)p * d + i] + 1e-6f;
                acc += df * df;
            }
        for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
        if (lane == 0) { neg_pos[(size_t)q * nnum + k] = p < 0 ? -1 : p + index_base; neg_dist[(size_t)q * nnum + k] = p < 0 ? 0.f : sqrtf(acc); }
    }
}

// Average precision / precision@k from ranks (mdir/external/cirtorch/utils/evaluate.py:3-118).  A unit is one (setup, query) pair.
//   1. inv[q][ranks[q][r]] = r (the inverse permutation; a value out of range or a slot left unfilled flags status bit 0);
//   2. per unit, the positive / junk ids are flagged in POSITION space: one bit per rank in two bitmasks (set semantics for free);
//   3. per unit one workgroup scans the bitmasks in rank order: a positive at position p is the j-th positive and has k = popcount of the
//      junk bits below p (the reference's strict pos[ip] > junk[ij]); its trapezoid goes to terms[j], its adjusted rank p - k to adj[j];
//   4. one lane adds the terms in rank order (the reference's `ap +=` loop: the same doubles in the same order) and reads precision@k
//      off the adjusted ranks, which never decrease.
// No cap below ndb: terms / adj live in the workspace at the unit's CSR offset, so a query may have every database image as a positive.
constexpr int AP_MAX_KAPPAS = 16;
constexpr int AP_THREADS = 256;
struct Kappas { int k[AP_MAX_KAPPAS]; };

struct ApLayout { size_t inv, pmask, jmask, terms, adj, total; int nwords; };

int ap_plan(int ndb, int nq, int nsetups, long n_ok, ApLayout& L) {
    GDT_REQUIRE(ndb >= 1 && nq >= 1 && nsetups >= 1, "average precision needs ndb, nq, nsetups >= 1");
    GDT_REQUIRE((long)ndb * nq < (1l << 31), "ndb * nq must stay below 2^31");
    GDT_REQUIRE((long)nsetups * nq < (1l << 31), "nsetups * nq must stay below 2^31");
    GDT_REQUIRE(n_ok >= 0, "n_ok >= 0");
    const size_t units = (size_t)nsetups * nq;
    L.nwords = (ndb + 31) / 32;
    size_t off = 0;
    L.inv = off; off += align_up((size_t)nq * ndb * sizeof(int));
    L.pmask = off; off += align_up(units * L.nwords * sizeof(unsigned));
    L.jmask = off; off += align_up(units * L.nwords * sizeof(unsigned));
    L.terms = off; off += align_up((size_t)std::max<long>(n_ok, 1) * sizeof(double));
    L.adj = off; off += align_up((size_t)std::max<long>(n_ok, 1) * sizeof(int));
    L.total = off + ALIGN;
    return GDT_OK;
}

__global__ __launch_bounds__(256) void ap_inverse_kernel(const int* __restrict__ ranks_t, int* __restrict__ inv, int* __restrict__ status, int ndb,
                                                         long total) {
    bool bad = false;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long q = i / ndb;
        const int v = ranks_t[i];
        if (v >= 0 && v < ndb) inv[q * ndb + v] = (int)(i - q * ndb);
        else bad = true;
    }
    if (bad) atomicOr(status, 1);
}

__global__ __launch_bounds__(256) void ap_check_kernel(const int* __restrict__ inv, int* __restrict__ status, long total) {
    bool bad = false;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) bad |= inv[i] < 0;
    if (bad) atomicOr(status, 1);           // ndb values in range and every slot filled: a permutation
}

__device__ inline void ap_mark(const int* __restrict__ inv_q, const int* __restrict__ ids, int lo, int hi, unsigned* __restrict__ mask, int ndb) {
    for (int i = lo + (int)threadIdx.x; i < hi; i += AP_THREADS) {
        const int id = ids[i];
        if (id < 0 || id >= ndb) continue;                       // np.in1d: an id outside the database matches nothing
        const int p = inv_q[id];
        if (p >= 0) atomicOr(mask + (p >> 5), 1u << (p & 31));
    }
}

__global__ __launch_bounds__(AP_THREADS) void ap_mark_kernel(const int* __restrict__ inv, const int* __restrict__ ok_off, const int* __restrict__ ok_ids,
                                                             const int* __restrict__ junk_off, const int* __restrict__ junk_ids,
                                                             unsigned* __restrict__ pmask, unsigned* __restrict__ jmask, int ndb, int nq, int nwords) {
    const int u = blockIdx.x;
    const int* inv_q = inv + (size_t)(u % nq) * ndb;
    ap_mark(inv_q, ok_ids, ok_off[u], ok_off[u + 1], pmask + (size_t)u * nwords, ndb);
    ap_mark(inv_q, junk_ids, junk_off[u], junk_off[u + 1], jmask + (size_t)u * nwords, ndb);
}

__global__ __launch_bounds__(AP_THREADS) void ap_terms_kernel(const unsigned* __restrict__ pmask, const unsigned* __restrict__ jmask,
                                                              const int* __restrict__ ok_off, double* __restrict__ terms, int* __restrict__ adj,
                                                              double* __restrict__ ap, double* __restrict__ prk, int* __restrict__ status,
                                                              int nwords, Kappas kappas, int nk) {
#pragma clang fp contract(off)
    const int u = blockIdx.x, t = threadIdx.x;
    const unsigned* pm = pmask + (size_t)u * nwords;
    const unsigned* jm = jmask + (size_t)u * nwords;
    const int base = ok_off[u], nres = ok_off[u + 1] - base;
    const int chunk = (nwords + AP_THREADS - 1) / AP_THREADS;
    const int w0 = t * chunk < nwords ? t * chunk : nwords, w1 = w0 + chunk < nwords ? w0 + chunk : nwords;
    int cp = 0, cj = 0;
    for (int w = w0; w < w1; ++w) { cp += __popc(pm[w]); cj += __popc(jm[w]); }
    // exclusive scan of the per-thread counts: positives and junk before this thread's words
    __shared__ int sp[AP_THREADS], sj[AP_THREADS];
    sp[t] = cp; sj[t] = cj;
    __syncthreads();
    for (int d = 1; d < AP_THREADS; d <<= 1) {
        const int a = t >= d ? sp[t - d] : 0, b = t >= d ? sj[t - d] : 0;
        __syncthreads();
        sp[t] += a; sj[t] += b;
        __syncthreads();
    }
    const int npos = sp[AP_THREADS - 1];
    int j = sp[t] - cp, kj = sj[t] - cj;
    const double rs = 1.0 / (double)nres;                          // recall_step = 1. / nres
    for (int w = w0; w < w1; ++w) {
        unsigned pw = pm[w];
        const unsigned jw = jm[w];
        while (pw) {
            const int b = __ffs(pw) - 1;
            pw &= pw - 1;
            const int rank = w * 32 + b - (kj + __popc(jw & ((1u << b) - 1u)));
            const double p0 = rank == 0 ? 1.0 : (double)j / (double)rank;
            const double p1 = (double)(j + 1) / (double)(rank + 1);
            terms[base + j] = (p0 + p1) * rs / 2.0;
            adj[base + j] = rank;
            ++j;
        }
        kj += __popc(jw);
    }
    __syncthreads();
    if (t != 0) return;
    const double nan = __builtin_nan("");
    if (nres == 0) {                                               // no positive images: NaN, excluded from the mean
        ap[u] = nan;
        for (int i = 0; i < nk; ++i) prk[(size_t)u * nk + i] = nan;
        return;
    }
    double s = 0.0;
    for (int i = 0; i < npos; ++i) s = s + terms[base + i];       // in rank order, one lane: the reference's sum
    ap[u] = s;
    if (npos == 0) {
        if (nk > 0) atomicOr(status, 2);
        for (int i = 0; i < nk; ++i) prk[(size_t)u * nk + i] = nan;
        return;
    }
    const int* a = adj + base;
    const long maxpos = (long)a[npos - 1] + 1;                     // max(pos) after pos += 1
    for (int i = 0; i < nk; ++i) {
        const long kq = maxpos < kappas.k[i] ? maxpos : (long)kappas.k[i];
        int lo = 0, hi = npos;                                     // count of a[] + 1 <= kq: a[] never decreases
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((long)a[mid] + 1 <= kq) lo = mid + 1; else hi = mid;
        }
        prk[(size_t)u * nk + i] = (double)lo / (double)kq;
    }
}

// Diverse-anchor selection (mdir/components/data/dataset/cirtorch_datasets.py:77-100): a greedy chain of nsel - 1 dependent steps.  The reference
// grows a [nq][t] matrix of similarities, takes its row maximum and argsorts it every step; the chain only needs the running maximum.  Per step two
// launches in stream order (no host round trip, no wait between workgroups):
//   1. da_update_kernel: ms[i] = max(ms[i], <vecs[i], vecs[out_idx[t]]>) for every row, fp32 FMA, DA_ROWS rows per wave in flight, the pivot row
//      staged in LDS in chunks of DA_CHUNK floats (any d), float4 loads where d and the base address allow them;
//   2. da_select_kernel: one workgroup finds the entry at ascending position target_rank[t] of ms -- a radix select over order-preserving uint32
//      keys (4 passes of 8 bits, LDS histogram), then the index among the entries that share the selected key (lower index first).
// The summation order of a dot product is fixed by (d, lane), so two runs give the same bits.
constexpr int DA_THREADS = 256, DA_ROWS = 4, DA_CHUNK = 4096, DA_ROWS_PER_BLOCK = DA_THREADS / 64 * DA_ROWS;
constexpr int DS_THREADS = 1024, DS_WAVES = DS_THREADS / 64;

template <bool VEC4>
__global__ __launch_bounds__(DA_THREADS) void da_update_kernel(const float* __restrict__ vecs, float* __restrict__ ms, int* out_idx, int nq, int d,
                                                               int t, int first_idx) {
    __shared__ __attribute__((aligned(16))) float piv[DA_CHUNK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int p = t == 0 ? first_idx : out_idx[t];
    p = p < 0 ? 0 : (p >= nq ? nq - 1 : p);                        // written by da_select_kernel, always in range: the clamp only guards the loads
    if (t == 0 && blockIdx.x == 0 && threadIdx.x == 0) out_idx[0] = p;
    const int row0 = blockIdx.x * DA_ROWS_PER_BLOCK + wave * DA_ROWS;
    const float* rows[DA_ROWS];
    float acc[DA_ROWS];
#pragma unroll
    for (int r = 0; r < DA_ROWS; ++r) {
        const int row = row0 + r < nq ? row0 + r : nq - 1;         // a row past the end re-reads the last one and is not written
        rows[r] = vecs + (size_t)row * d;
        acc[r] = 0.f;
    }
    const float* prow = vecs + (size_t)p * d;
    for (int c0 = 0; c0 < d; c0 += DA_CHUNK) {
        const int n = d - c0 < DA_CHUNK ? d - c0 : DA_CHUNK;
        if (c0) __syncthreads();
        if (VEC4) {
            for (int i = threadIdx.x * 4; i < n; i += DA_THREADS * 4) *(float4*)(piv + i) = *(const float4*)(prow + c0 + i);
        } else {
            for (int i = threadIdx.x; i < n; i += DA_THREADS) piv[i] = prow[c0 + i];
        }
        __syncthreads();
        if (VEC4) {
            for (int i = lane * 4; i < n; i += 256) {
                const float4 b = *(const float4*)(piv + i);
                float4 a[DA_ROWS];
#pragma unroll
                for (int r = 0; r < DA_ROWS; ++r) a[r] = *(const float4*)(rows[r] + c0 + i);
#pragma unroll
                for (int r = 0; r < DA_ROWS; ++r) {
                    acc[r] = fmaf(a[r].x, b.x, acc[r]);
                    acc[r] = fmaf(a[r].y, b.y, acc[r]);
                    acc[r] = fmaf(a[r].z, b.z, acc[r]);
                    acc[r] = fmaf(a[r].w, b.w, acc[r]);
                }
            }
        } else {
            for (int i = lane; i < n; i += 64) {
                const float b = piv[i];
#pragma unroll
                for (int r = 0; r < DA_ROWS; ++r) acc[r] = fmaf(rows[r][c0 + i], b, acc[r]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < DA_ROWS; ++r) {
        float v = acc[r];
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
        const int row = row0 + r;
        if (lane == 0 && row < nq) ms[row] = t == 0 ? v : fmaxf(ms[row], v);
    }
}

// ascending float order == ascending unsigned order of the key (-0.f below +0.f; NaNs at the two ends by their sign)
__device__ inline unsigned da_key(float x) {
    const unsigned u = __float_as_uint(x);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

__global__ __launch_bounds__(DS_THREADS) void da_select_kernel(const float* ms, const int* __restrict__ target_rank, int* out_idx, float* out_score,
                                                               int nq, int t) {
    __shared__ unsigned hist[256];
    __shared__ unsigned s_prefix, s_k;
    __shared__ int wave_count[DS_WAVES];
    __shared__ int s_found;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) {
        const int k = target_rank[t];
        s_k = (unsigned)(k < 0 ? 0 : (k >= nq ? nq - 1 : k));      // checked on the host before the upload; clamped so that the search below always ends inside ms
        s_prefix = 0;
        s_found = 0;
    }
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        const unsigned prefix = s_prefix, k = s_k;
        const unsigned himask = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
        for (int base = 0; base < nq; base += DS_THREADS) {
            const int i = base + tid;
            bool live = false;
            unsigned bin = 0;
            if (i < nq) {
                const unsigned key = da_key(ms[i]);
                live = (key & himask) == prefix;
                bin = (key >> shift) & 255u;
            }
            if (shift == 24) {
                // similarities crowd into a few sign/exponent bins: one LDS add per distinct bin of the wave instead of one per lane
                unsigned long long todo = __ballot(live);
                while (todo) {
                    const int leader = __ffsll((long long)todo) - 1;
                    const unsigned b = (unsigned)__shfl((int)bin, leader);
                    const unsigned long long same = __ballot(live && bin == b);
                    if (lane == leader) atomicAdd(&hist[b], (unsigned)__popcll(same));
                    todo &= ~same;
                }
            } else if (live) {
                atomicAdd(&hist[bin], 1u);
            }
        }
        __syncthreads();
        if (wave == 0) {                                           // the bin in which the running count passes k: lane l owns bins 4l .. 4l+3
            const unsigned c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
            const unsigned own = c0 + c1 + c2 + c3;
            unsigned incl = own;
            for (int m = 1; m < 64; m <<= 1) {
                const unsigned up = (unsigned)__shfl_up((int)incl, m);
                if (lane >= m) incl += up;
            }
            const unsigned long long hit = __ballot(k < incl);     // never empty: k is below the number of live entries
            const int owner = hit ? __ffsll((long long)hit) - 1 : 63;
            if (lane == owner) {
                unsigned below = incl - own, b = 4 * lane;
                if (k >= below + c0) { below += c0; ++b;
                    if (k >= below + c1) { below += c1; ++b;
                        if (k >= below + c2) { below += c2; ++b; } } }
                s_prefix = prefix | (b << shift);
                s_k = k - below;
            }
        }
        __syncthreads();
    }
    // s_prefix is the key at the target position, s_k the position among the entries that carry it, in index order
    const unsigned key = s_prefix;
    const int want = (int)s_k;
    int seen = 0;
    for (int base = 0; base < nq; base += DS_THREADS) {
        const int i = base + tid;
        const bool m = i < nq && da_key(ms[i]) == key;
        const unsigned long long b = __ballot(m);
        if (lane == 0) wave_count[wave] = __popcll(b);
        __syncthreads();
        int before = seen, total = seen;
        for (int w = 0; w < DS_WAVES; ++w) {
            const int c = wave_count[w];
            if (w < wave) before += c;
            total += c;
        }
        if (m && before + __popcll(b & ((1ull << lane) - 1ull)) == want) {
            out_idx[t + 1] = i;
            out_score[t] = ms[i];
            s_found = 1;
        }
        seen = total;
        __syncthreads();
        if (s_found) break;
    }
}

struct DaLayout { size_t ms, total; };

int da_plan(int nq, int d, int nsel, DaLayout& L) {
    GDT_REQUIRE(nq >= 2 && d >= 1, "diverse anchors need nq >= 2 descriptors of size d >= 1");
    GDT_REQUIRE(nsel >= 2 && nsel <= nq, "2 <= nsel <= nq");
    L.ms = 0;
    L.total = align_up((size_t)nq * sizeof(float)) + ALIGN;
    return GDT_OK;
}

}  // namespace

extern "C" {

int gdt_retrieval_workspace_bytes(int ndb, int nq, int d, int with_ranks, size_t* bytes) {
    GDT_REQUIRE(bytes != nullptr, "bytes");
    Layout L;
    int rc = plan(ndb, nq, d, with_ranks != 0, L);
    if (rc != GDT_OK) return rc;
    *bytes = L.total;
    return GDT_OK;
}

int gdt_retrieval_scores_ranks(const float* vecs, const float* qvecs, float* scores_t, int* ranks_t, int ndb, int nq, int d,
                               int index_base, void* workspace, size_t workspace_bytes, void* stream) {
    GDT_REQUIRE(vecs && qvecs && scores_t && workspace, "null buffer");
    Layout L;
    int rc = plan(ndb, nq, d, ranks_t != nullptr, L);
    if (rc != GDT_OK) return rc;
    if (L.total > workspace_bytes) {
        gdt_set_error("workspace too small: need " + std::to_string(L.total) + " bytes, got " + std::to_string(workspace_bytes));
        return GDT_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)(((uintptr_t)workspace + ALIGN - 1) / ALIGN * ALIGN);
    f16* hi = (f16*)(ws + L.hi);
    f16* lo = (f16*)(ws + L.lo);
    {
        const long total = (long)L.nq_pad * L.kpad;
        const int grid = (int)std::min<long>((total + 255) / 256, 4096);
        hipLaunchKernelGGL(split_rows_kernel, dim3(grid), dim3(256), 0, st, qvecs, hi, lo, nq, d, L.nq_pad, L.kpad);
        GDT_CHECK_HIP(hipGetLastError());
    }
    // scores_t[q][i] = <vecs[i], qvecs[q]>: a 1x1 "convolution" over ndb positions with d input and nq output channels
    ConvLaunch c{};
    c.in = (const f16*)vecs; c.w = hi; c.w_lo = lo; c.out_f32 = scores_t; c.zeros = hi;
    c.N = 1; c.H = 1; c.W = ndb; c.Cin = d; c.lc8 = 0; while ((8 << c.lc8) < d) ++c.lc8;
    c.Cout = nq; c.CoutPad = L.nq_pad; c.Kpad = L.kpad; c.nk = L.kpad / 32;
    c.OHg = 1; c.OWg = ndb; c.OH = 1; c.OW = ndb; c.sy = c.sx = 1; c.osy = c.osx = 1;
    c.ntaps = 1; c.TW = 1; c.invTW = 65536; c.dys = c.dxs = 1;
    c.M = ndb;
    rc = gdt_launch_conv_x3(c, st, nullptr);
    if (rc != GDT_OK || !ranks_t) return rc;
    int* idx = (int*)(ws + L.idx);
    int* offs = (int*)(ws + L.offs);
    {
        const long total = (long)nq * ndb;
        const int grid = (int)std::min<long>((total + 255) / 256, 4096);
        hipLaunchKernelGGL(iota_segments_kernel, dim3(grid), dim3(256), 0, st, idx, offs, nq, ndb, index_base);
        GDT_CHECK_HIP(hipGetLastError());
    }
    size_t tb = L.tmp_bytes;
    GDT_CHECK_HIP(rocprim::segmented_radix_sort_pairs_desc((void*)(ws + L.tmp), tb, (const float*)scores_t, (float*)(ws + L.keys),
                                                            (const int*)idx, ranks_t, (unsigned)((size_t)nq * ndb), (unsigned)nq,
                                                            (const int*)offs, (const int*)(offs + 1), 0, 32, st));
    return GDT_OK;
}

int gdt_retrieval_select_negatives(const int* ranks_t, const int* pool_cluster, const int* query_cluster, const float* vecs, const float* qvecs,
                                   int* neg_pos, float* neg_dist, int* status, int ndb, int nq, int d, int nnum, int index_base, void* stream) {
    GDT_REQUIRE(ranks_t && pool_cluster && query_cluster && vecs && qvecs && neg_pos && neg_dist && status, "null buffer");
    GDT_REQUIRE(ndb >= 1 && nq >= 1 && d >= 1 && nnum >= 1 && nnum <= 64, "1 <= nnum <= 64 negatives per query");
    hipStream_t st = (hipStream_t)stream;
    GDT_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int), st));
    hipLaunchKernelGGL(select_negatives_kernel, dim3(nq), dim3(64), 0, st, ranks_t, pool_cluster, query_cluster, vecs, qvecs, neg_pos, neg_dist, status,
                       ndb, nq, d, nnum, index_base);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

int gdt_retrieval_ap_workspace_bytes(int ndb, int nq, int nsetups, int n_ok, size_t* bytes) {
    GDT_REQUIRE(bytes != nullptr, "bytes");
    ApLayout L;
    int rc = ap_plan(ndb, nq, nsetups, n_ok, L);
    if (rc != GDT_OK) return rc;
    *bytes = L.total;
    return GDT_OK;
}

int gdt_retrieval_average_precision(const int* ranks_t, int ndb, int nq, int nsetups, const int* ok_offsets, const int* ok_ids,
                                    const int* junk_offsets, const int* junk_ids, const int* ok_offsets_host, const int* junk_offsets_host,
                                    const int* kappas, int nk, double* ap, double* prk, int* status, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    GDT_REQUIRE(ok_offsets_host && junk_offsets_host, "null host offsets");
    GDT_REQUIRE(nk >= 0 && nk <= AP_MAX_KAPPAS, "0 <= nk <= 16 kappas");
    GDT_REQUIRE(nk == 0 || kappas != nullptr, "null kappas");
    Kappas K{};
    for (int i = 0; i < nk; ++i) {
        GDT_REQUIRE(kappas[i] >= 1, "kappas >= 1");
        K.k[i] = kappas[i];
    }
    ApLayout L;
    GDT_REQUIRE(ndb >= 1 && nq >= 1 && nsetups >= 1 && (long)nsetups * nq < (1l << 31), "ndb, nq, nsetups >= 1");
    const long units = (long)nsetups * nq;
    const int* offs[2] = {ok_offsets_host, junk_offsets_host};
    for (const int* o : offs) {
        GDT_REQUIRE(o[0] == 0, "offsets start at 0");
        for (long u = 0; u < units; ++u) GDT_REQUIRE(o[u + 1] >= o[u], "offsets never decrease");
    }
    int rc = ap_plan(ndb, nq, nsetups, ok_offsets_host[units], L);
    if (rc != GDT_OK) return rc;
    GDT_REQUIRE(ranks_t && ok_offsets && junk_offsets && ap && status && (nk == 0 || prk) && workspace, "null buffer");
    GDT_REQUIRE(ok_offsets_host[units] == 0 || ok_ids, "null ok_ids");
    GDT_REQUIRE(junk_offsets_host[units] == 0 || junk_ids, "null junk_ids");
    if (L.total > workspace_bytes) {
        gdt_set_error("workspace too small: need " + std::to_string(L.total) + " bytes, got " + std::to_string(workspace_bytes));
        return GDT_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)(((uintptr_t)workspace + ALIGN - 1) / ALIGN * ALIGN);
    int* inv = (int*)(ws + L.inv);
    unsigned* pmask = (unsigned*)(ws + L.pmask);
    unsigned* jmask = (unsigned*)(ws + L.jmask);
    const long total = (long)nq * ndb;
    GDT_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int), st));
    GDT_CHECK_HIP(hipMemsetAsync(inv, 0xff, (size_t)total * sizeof(int), st));
    GDT_CHECK_HIP(hipMemsetAsync(pmask, 0, L.terms - L.pmask, st));          // both bitmasks
    const int grid = (int)std::min<long>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(ap_inverse_kernel, dim3(grid), dim3(256), 0, st, ranks_t, inv, status, ndb, total);
    GDT_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(ap_check_kernel, dim3(grid), dim3(256), 0, st, (const int*)inv, status, total);
    GDT_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(ap_mark_kernel, dim3((unsigned)units), dim3(AP_THREADS), 0, st, (const int*)inv, ok_offsets, ok_ids, junk_offsets, junk_ids,
                       pmask, jmask, ndb, nq, L.nwords);
    GDT_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(ap_terms_kernel, dim3((unsigned)units), dim3(AP_THREADS), 0, st, (const unsigned*)pmask, (const unsigned*)jmask, ok_offsets,
                       (double*)(ws + L.terms), (int*)(ws + L.adj), ap, prk, status, L.nwords, K, nk);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

int gdt_retrieval_diverse_anchors_workspace_bytes(int nq, int d, int nsel, size_t* bytes) {
    GDT_REQUIRE(bytes != nullptr, "bytes");
    DaLayout L;
    int rc = da_plan(nq, d, nsel, L);
    if (rc != GDT_OK) return rc;
    *bytes = L.total;
    return GDT_OK;
}

int gdt_retrieval_diverse_anchors(const float* vecs, int nq, int d, const int* target_rank, int nsel, int first_idx, int* out_idx,
                                  float* out_score, void* workspace, size_t workspace_bytes, void* stream) {
    GDT_REQUIRE(vecs && target_rank && out_idx && out_score && workspace, "null buffer");
    DaLayout L;
    int rc = da_plan(nq, d, nsel, L);
    if (rc != GDT_OK) return rc;
    GDT_REQUIRE(first_idx >= 0 && first_idx < nq, "0 <= first_idx < nq");
    GDT_REQUIRE(workspace_bytes >= L.total, "workspace too small (gdt_retrieval_diverse_anchors_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)(((uintptr_t)workspace + ALIGN - 1) / ALIGN * ALIGN);
    float* ms = (float*)(ws + L.ms);
    const bool vec4 = d % 4 == 0 && (uintptr_t)vecs % 16 == 0;
    const dim3 grid((unsigned)((nq + DA_ROWS_PER_BLOCK - 1) / DA_ROWS_PER_BLOCK));
    for (int t = 0; t < nsel - 1; ++t) {
        if (vec4) hipLaunchKernelGGL(da_update_kernel<true>, grid, dim3(DA_THREADS), 0, st, vecs, ms, out_idx, nq, d, t, first_idx);
        else hipLaunchKernelGGL(da_update_kernel<false>, grid, dim3(DA_THREADS), 0, st, vecs, ms, out_idx, nq, d, t, first_idx);
        hipLaunchKernelGGL(da_select_kernel, dim3(1), dim3(DS_THREADS), 0, st, (const float*)ms, target_rank, out_idx, out_score, nq, t);
    }
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

}  // extern "C"
