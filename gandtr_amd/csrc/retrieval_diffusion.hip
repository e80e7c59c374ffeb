// Diffusion re-ranking on the mutual kNN graph (Iscen et al., CVPR 2017; the "DFS" row of the revisited Oxford / Paris benchmark, Radenovic et al.,
// CVPR 2018): the consumer of the kNN lists that gdt_retrieval_topk writes, and the ranking of a score matrix the library did not compute.
//
// ARITHMETIC.  ids[i][s], scores[i][s], s < k: the kNN lists of n database vectors (self excluded, -1 = missing; an id outside [0, n) is a missing
// entry too: no id is dereferenced unchecked).
//   edge affinity      a_is = powf(max(scores[i][s], 0), gamma)
//   mutual weight      j = ids[i][s]:  w_is = min(a_is, a_jt) if 0 <= j < n and row j lists i at some slot t (the first such t), else 0.  The mutual
//                      graph is a subset of each row's own list: same [n][k] shape, same ids.
//   degree             deg_i = sum_s w_is, float64, s ascending;  r_i = (float)(1 / sqrt(deg_i)), 1 where deg_i == 0 (an isolated row)
//   normalised weight  S_is = w_is * (r_i * r_j), fp32, the product r_i * r_j formed first: min and that product commute, S is symmetric bit for bit
//   system             (I - alpha S) f_q = y_q per query column q, 0 < alpha < 1;  y_q[seed_ids[q][t]] += seed_w[q][t] in slot order (duplicate ids
//                      add, an id outside [0, n) adds nothing)
//   solver             conjugate gradients from f = 0, the columns independent of each other.  A column stops, and its state freezes, when
//                      ||r|| <= tol ||y|| or after max_iter iterations; y = 0 returns exactly 0 with 0 iterations.  Products are fp32 (fmaf chains
//                      over s ascending); every dot product is a sum of fp32 products accumulated in float64 in an order fixed by n alone; the
//                      step lengths are float64 quotients rounded to fp32 once.  No float atomics.
//
// KERNELS.  aff_mutual_kernel (one thread per edge; the search for i in row j is a scan of at most 256 ids), aff_norm_kernel (one thread per row),
// aff_scale_kernel (one thread per edge, in place).  The solver works on column blocks of B <= 64 queries stored [n][Bp], Bp = B rounded up to a
// power of two, the query index contiguous: a neighbour's row of P is one contiguous read of up to 256 B.  A workgroup owns DF_ROWS = 64 rows with
// min(1024, max(256, 64 Bp)) threads; thread t is column t % Bp of row slot t / Bp, so with Bp < 64 a wave holds 64 / Bp rows and no lane idles
// down to Bp = 4; with Bp = 64 a wave walks 4 rows.  Per iteration:
//   df_spmv_kernel     AP = P - alpha S P: per row the k gathers in groups of 8 independent loads (j and S_is uniform per row slot), and the fp32
//                      products p AP of the workgroup's rows, summed per column over the rows ascending into one float64 partial per (row block, column)
//   df_finish_kernel   one workgroup: partials in chunks of 64 row blocks, chunk totals ascending -> the step length a per column
//   df_update_kernel   X += a P, R -= a AP on the active columns, and the partials of r r
//   df_finish_kernel   -> b = rr' / rr, the iteration count, the stopping rule, and the block's `done` flag
//   df_pupdate_kernel  P = R + b P on the active columns
// The order of every sum is (row in block, block in chunk, chunk): a function of n alone, and a column's arithmetic never looks at another column, so
// a column's bits do not depend on B, on its position in the block, or on the run.  The dots are finished by a launch of their own, not by every
// workgroup of the next kernel: the n / 64 partials per column would be re-read by each of the n / 64 workgroups.  Flags, step lengths and counts
// live on the device (DfCtl); the host enqueues max_iter iterations without a synchronisation and the launches of a finished block return at once.
//
// RANKING.  gdt_retrieval_rank_scores: rocPRIM's segmented radix sort (descending, stable) of (score, database index) pairs, one segment per query,
// as gdt_retrieval_scores_ranks runs it, on a copy of the scores with -0.0f replaced by +0.0f: the radix order separates the two zeros, the
// module's strict order (score descending, id ascending) does not.
#include <algorithm>
#include <cstdint>
#include <string>

#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "../../include/gandtr_hip.h"
#include "gdt_common.h"

namespace {

constexpr size_t ALIGN = 256;
inline size_t align_up(size_t v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }

constexpr int DF_MAX_K = 256, DF_MAX_BLOCK = 64, DF_MAX_ITER = 1000;
constexpr int DF_THREADS = 1024, DF_ROWS = 64;       // the widest workgroup; rows of a workgroup = rows of one float64 partial
constexpr int DF_CHUNK = 64;                         // row blocks per chunk of the second summation level
constexpr int DF_FIN_THREADS = 1024;
constexpr int DF_GATHERS = 8;                        // independent neighbour rows in flight per thread

// ---- affinity

__global__ __launch_bounds__(256) void aff_mutual_kernel(const int* __restrict__ ids, const float* __restrict__ scores, float* __restrict__ w, int n,
                                                         int k, float gamma) {
    const long total = (long)n * k;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int i = (int)(e / k);
        const int j = ids[e];
        float v = 0.f;
        if (j >= 0 && j < n) {
            const int* rj = ids + (size_t)j * k;
            int t = 0;
            while (t < k && rj[t] != i) ++t;
            if (t < k) v = fminf(powf(fmaxf(scores[e], 0.f), gamma), powf(fmaxf(scores[(size_t)j * k + t], 0.f), gamma));
        }
        w[e] = v;
    }
}

__global__ __launch_bounds__(256) void aff_norm_kernel(const float* __restrict__ w, float* __restrict__ r, int n, int k) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double deg = 0.0;
    for (int s = 0; s < k; ++s) deg += (double)w[(size_t)i * k + s];
    r[i] = deg == 0.0 ? 1.f : (float)(1.0 / sqrt(deg));
}

__global__ __launch_bounds__(256) void aff_scale_kernel(const int* __restrict__ ids, const float* __restrict__ r, float* __restrict__ w, int n, int k) {
    const long total = (long)n * k;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int j = ids[e];
        w[e] = (j >= 0 && j < n) ? __fmul_rn(w[e], __fmul_rn(r[e / k], r[j])) : 0.f;
    }
}

// ---- conjugate gradients on a column block

struct DfCtl {
    double rr[DF_MAX_BLOCK], yy[DF_MAX_BLOCK];
    float a[DF_MAX_BLOCK], b[DF_MAX_BLOCK];
    int active[DF_MAX_BLOCK], iters[DF_MAX_BLOCK];
    int done;
};

// y of the block's columns into R: one thread per column walks its seeds in slot order
__global__ __launch_bounds__(64) void df_seed_kernel(const int* __restrict__ seed_ids, const float* __restrict__ seed_w, float* __restrict__ R, int n, int kq,
                                                     int q0, int B, int lb) {
    const int col = threadIdx.x;
    if (col >= B) return;
    const size_t base = (size_t)(q0 + col) * kq;
    for (int t = 0; t < kq; ++t) {
        const int id = seed_ids[base + t];
        if (id >= 0 && id < n) R[((size_t)id << lb) + col] += seed_w[base + t];
    }
}

// the fp32 products of the workgroup's rows -> one float64 partial per column: rows ascending
__device__ __forceinline__ void df_block_partial(const float* prod, double* __restrict__ part, int bp) {
    __syncthreads();
    if ((int)threadIdx.x < bp) {
        double s = 0.0;
        for (int rl = 0; rl < DF_ROWS; ++rl) s += (double)prod[rl * bp + threadIdx.x];
        part[(size_t)blockIdx.x * bp + threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(DF_THREADS) void df_spmv_kernel(const int* __restrict__ ids, const float* __restrict__ S, const float* __restrict__ P,
                                                             float* __restrict__ AP, double* __restrict__ part, const DfCtl* __restrict__ ctl, int n,
                                                             int k, int lb, float alpha) {
#pragma clang fp contract(off)
    if (ctl->done) return;
    __shared__ float prod[DF_ROWS * DF_MAX_BLOCK];
    const int bp = 1 << lb, col = threadIdx.x & (bp - 1), slot = threadIdx.x >> lb, nslots = (int)blockDim.x >> lb;
    const int row0 = blockIdx.x * DF_ROWS;
    for (int rl = slot; rl < DF_ROWS; rl += nslots) {
        const int i = row0 + rl;
        float pr = 0.f;
        if (i < n) {
            const int* ri = ids + (size_t)i * k;
            const float* si = S + (size_t)i * k;
            float acc = 0.f;
            // groups of DF_GATHERS slots: the ids / weights of the next group are requested before the gathers of this one, so a group costs one
            // round trip to memory, not two in a row
            const int kg = k / DF_GATHERS * DF_GATHERS;
            int jn[DF_GATHERS];
            float wn[DF_GATHERS];
            if (kg) {
#pragma unroll
                for (int u = 0; u < DF_GATHERS; ++u) { jn[u] = ri[u]; wn[u] = si[u]; }
            }
            int s = 0;
            for (; s < kg; s += DF_GATHERS) {
                int j[DF_GATHERS];
                float sv[DF_GATHERS], pv[DF_GATHERS];
#pragma unroll
                for (int u = 0; u < DF_GATHERS; ++u) { j[u] = jn[u]; sv[u] = wn[u]; }
                if (s + DF_GATHERS < kg) {
#pragma unroll
                    for (int u = 0; u < DF_GATHERS; ++u) { jn[u] = ri[s + DF_GATHERS + u]; wn[u] = si[s + DF_GATHERS + u]; }
                }
#pragma unroll
                for (int u = 0; u < DF_GATHERS; ++u) {
                    const bool ok = j[u] >= 0 && j[u] < n;                 // a missing entry reads the row itself with weight 0
                    sv[u] = ok ? sv[u] : 0.f;
                    pv[u] = P[((size_t)(ok ? j[u] : i) << lb) + col];
                }
#pragma unroll
                for (int u = 0; u < DF_GATHERS; ++u) acc = fmaf(sv[u], pv[u], acc);
            }
            for (; s < k; ++s) {
                const int j = ri[s];
                const bool ok = j >= 0 && j < n;
                acc = fmaf(ok ? si[s] : 0.f, P[((size_t)(ok ? j : i) << lb) + col], acc);
            }
            const size_t e = ((size_t)i << lb) + col;
            const float pi = P[e];
            const float ap = fmaf(-alpha, acc, pi);
            AP[e] = ap;
            pr = pi * ap;
        }
        prod[rl * bp + col] = pr;
    }
    df_block_partial(prod, part, bp);
}

__global__ __launch_bounds__(DF_THREADS) void df_update_kernel(float* __restrict__ X, float* __restrict__ R, const float* __restrict__ P,
                                                               const float* __restrict__ AP, double* __restrict__ part, const DfCtl* __restrict__ ctl,
                                                               int n, int lb, int first) {
#pragma clang fp contract(off)
    if (ctl->done) return;
    __shared__ float prod[DF_ROWS * DF_MAX_BLOCK];
    const int bp = 1 << lb, col = threadIdx.x & (bp - 1), slot = threadIdx.x >> lb, nslots = (int)blockDim.x >> lb;
    const int row0 = blockIdx.x * DF_ROWS;
    const bool act = !first && ctl->active[col] != 0;
    const float a = ctl->a[col];
    for (int rl = slot; rl < DF_ROWS; rl += nslots) {
        const int i = row0 + rl;
        float pr = 0.f;
        if (i < n) {
            const size_t e = ((size_t)i << lb) + col;
            float r = R[e];
            if (act) {
                X[e] = fmaf(a, P[e], X[e]);
                r = fmaf(-a, AP[e], r);
                R[e] = r;
            }
            pr = r * r;
        }
        prod[rl * bp + col] = pr;
    }
    df_block_partial(prod, part, bp);
}

__global__ __launch_bounds__(256) void df_pupdate_kernel(float* __restrict__ P, const float* __restrict__ R, const DfCtl* __restrict__ ctl, size_t total,
                                                         int lb) {
    if (ctl->done) return;
    const int bp = 1 << lb;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int col = (int)(e & (size_t)(bp - 1));
        if (ctl->active[col]) P[e] = fmaf(ctl->b[col], P[e], R[e]);
    }
}

// v[b0 * pitch] + v[(b0 + 1) * pitch] + .. in that order; the loads of 16 terms are in flight together, the additions stay sequential
__device__ __forceinline__ double df_sum_in_order(const double* v, int b0, int b1, int pitch) {
    double s = 0.0;
    int b = b0;
    for (; b + 16 <= b1; b += 16) {
        double t[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) t[u] = v[(size_t)(b + u) * pitch];
#pragma unroll
        for (int u = 0; u < 16; ++u) s += t[u];
    }
    for (; b < b1; ++b) s += v[(size_t)b * pitch];
    return s;
}

// mode 0: the total is p.Ap -> a.  mode 1: the total is y.y -> rr = yy, 0 iterations, the stopping rule.  mode 2: the total is the new r.r -> b, the
// iteration count, the stopping rule.  Modes 1 and 2 raise `done` when no column of the block is active any more.
enum { DF_FIN_PAP = 0, DF_FIN_FIRST = 1, DF_FIN_RR = 2 };

__global__ __launch_bounds__(DF_FIN_THREADS) void df_finish_kernel(const double* __restrict__ part, double* chunk_tot, DfCtl* ctl, int nblk, int lb,
                                                                   int mode, float tol, int max_iter) {
    if (ctl->done) return;
    const int bp = 1 << lb, tid = threadIdx.x;
    const int nchunks = (nblk + DF_CHUNK - 1) / DF_CHUNK;
    for (int p = tid; p < nchunks * bp; p += DF_FIN_THREADS) {
        const int col = p & (bp - 1), b0 = (p >> lb) * DF_CHUNK, b1 = b0 + DF_CHUNK < nblk ? b0 + DF_CHUNK : nblk;
        chunk_tot[p] = df_sum_in_order(part + col, b0, b1, bp);
    }
    __threadfence_block();
    __syncthreads();
    if (tid >= 64) return;
    bool act = false;
    if (tid < bp) {
        const double tot = df_sum_in_order(chunk_tot + tid, 0, nchunks, bp);
        if (mode == DF_FIN_PAP) {
            act = ctl->active[tid] != 0;
            ctl->a[tid] = act && tot > 0.0 ? (float)(ctl->rr[tid] / tot) : 0.f;
        } else if (mode == DF_FIN_FIRST) {
            ctl->rr[tid] = tot;
            ctl->yy[tid] = tot;
            ctl->iters[tid] = 0;
            act = tot > 0.0 && sqrt(tot) > (double)tol * sqrt(tot);
            ctl->active[tid] = act;
        } else if (ctl->active[tid]) {
            ctl->b[tid] = (float)(tot / ctl->rr[tid]);
            ctl->rr[tid] = tot;
            const int it = ++ctl->iters[tid];
            act = it < max_iter && sqrt(tot) > (double)tol * sqrt(ctl->yy[tid]);
            ctl->active[tid] = act;
        }
    }
    if (mode != DF_FIN_PAP && __ballot(act) == 0 && tid == 0) ctl->done = 1;
}

// X [n][bp] -> scores_t [nq][n] rows q0 .. q0 + B - 1 through an LDS tile (both sides contiguous), and the block's iteration counts / residuals
__global__ __launch_bounds__(256) void df_output_kernel(const float* __restrict__ X, const DfCtl* __restrict__ ctl, float* __restrict__ scores_t,
                                                        int* __restrict__ iterations, float* __restrict__ residual, int n, int q0, int B, int lb) {
    __shared__ float tile[DF_MAX_BLOCK * 65];
    const int bp = 1 << lb, row0 = blockIdx.x * 64;
    for (int e = threadIdx.x; e < 64 * bp; e += 256) {
        const int rl = e >> lb, col = e & (bp - 1), i = row0 + rl;
        tile[col * 65 + rl] = i < n ? X[((size_t)i << lb) + col] : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 64 * B; e += 256) {
        const int col = e >> 6, rl = e & 63, i = row0 + rl;
        if (i < n) scores_t[(size_t)(q0 + col) * n + i] = tile[col * 65 + rl];
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < B) {
        const int c = threadIdx.x;
        iterations[q0 + c] = ctl->iters[c];
        residual[q0 + c] = ctl->yy[c] > 0.0 ? (float)(sqrt(ctl->rr[c]) / sqrt(ctl->yy[c])) : 0.f;
    }
}

struct DfLayout { size_t x, r, p, ap, part, chunk, ctl, total; int lb, nblk, nchunks; };

inline int df_log2_up(int b) { int lb = 0; while ((1 << lb) < b) ++lb; return lb; }

int df_plan(int n, int nq, int block, DfLayout& L) {
    GDT_REQUIRE(n >= 1 && nq >= 1, "diffusion needs n >= 1 database rows and nq >= 1 query columns");
    GDT_REQUIRE(block >= 1 && block <= DF_MAX_BLOCK, "1 <= block <= 64 columns");
    L.lb = df_log2_up(std::min(block, nq));
    L.nblk = (int)(((long)n + DF_ROWS - 1) / DF_ROWS);
    L.nchunks = (L.nblk + DF_CHUNK - 1) / DF_CHUNK;
    const size_t vec = align_up(((size_t)n << L.lb) * sizeof(float));
    size_t off = 0;
    L.x = off; off += vec;
    L.r = off; off += vec;
    L.p = off; off += vec;
    L.ap = off; off += vec;
    L.part = off; off += align_up(((size_t)L.nblk << L.lb) * sizeof(double));
    L.chunk = off; off += align_up(((size_t)L.nchunks << L.lb) * sizeof(double));
    L.ctl = off; off += align_up(sizeof(DfCtl));
    L.total = off + ALIGN;
    return GDT_OK;
}

int df_check(int n, int k, int nq, int kq, int block, float alpha, float tol, int max_iter, DfLayout& L) {
    GDT_CHECK(df_plan(n, nq, block, L));
    GDT_REQUIRE(k >= 1 && k <= DF_MAX_K, "1 <= k <= 256");
    GDT_REQUIRE(kq >= 1 && kq <= DF_MAX_K, "1 <= kq <= 256");
    GDT_REQUIRE(alpha > 0.f && alpha < 1.f, "0 < alpha < 1");
    GDT_REQUIRE(tol > 0.f, "tol > 0");
    GDT_REQUIRE(max_iter >= 1 && max_iter <= DF_MAX_ITER, "1 <= max_iter <= 1000");
    return GDT_OK;
}

// ---- ranking of a given score matrix

__global__ __launch_bounds__(256) void rk_prepare_kernel(const float* __restrict__ scores, float* __restrict__ keys, int* __restrict__ idx,
                                                         int* __restrict__ offsets, int nseg, int len, int base) {
    const long total = (long)nseg * len;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const float x = scores[i];
        keys[i] = x == 0.f ? 0.f : x;                                      // -0.0f -> +0.0f
        idx[i] = base + (int)(i % len);
    }
    if (blockIdx.x == 0)
        for (int s = threadIdx.x; s <= nseg; s += 256) offsets[s] = s * len;
}

struct RkLayout { size_t idx, keys_in, keys_out, offs, tmp, tmp_bytes, total; };

int rk_plan(int n, int nq, RkLayout& L) {
    GDT_REQUIRE(n >= 1 && nq >= 1, "ranking needs n >= 1 scores per query and nq >= 1 queries");
    GDT_REQUIRE((long)n * nq < (1l << 31), "n * nq must stay below 2^31");
    const size_t total = (size_t)n * nq;
    size_t off = 0;
    L.idx = off; off += align_up(total * sizeof(int));
    L.keys_in = off; off += align_up(total * sizeof(float));
    L.keys_out = off; off += align_up(total * sizeof(float));
    L.offs = off; off += align_up((size_t)(nq + 1) * sizeof(int));
    size_t tb = 0;
    GDT_CHECK_HIP(rocprim::segmented_radix_sort_pairs_desc(nullptr, tb, (const float*)nullptr, (float*)nullptr, (const int*)nullptr, (int*)nullptr,
                                                           (unsigned)total, (unsigned)nq, (const int*)nullptr, (const int*)nullptr, 0, 32,
                                                           (hipStream_t)0));
    L.tmp = off; L.tmp_bytes = tb; off += align_up(tb);
    L.total = off + ALIGN;
    return GDT_OK;
}

inline int workspace_short(size_t need, size_t got) {
    gdt_set_error("workspace too small: need " + std::to_string(need) + " bytes, got " + std::to_string(got));
    return GDT_ERR_WORKSPACE;
}

}  // namespace

extern "C" {

int gdt_retrieval_knn_affinity(const int* ids, const float* scores, float* weights, float* rnorm, int n, int k, float gamma, void* stream) {
    GDT_REQUIRE(ids && scores && weights && rnorm, "null buffer");
    GDT_REQUIRE(weights != scores, "weights must not alias scores");
    GDT_REQUIRE(n >= 1, "n >= 1");
    GDT_REQUIRE(k >= 1 && k <= DF_MAX_K, "1 <= k <= 256");
    GDT_REQUIRE(gamma >= 0.f, "gamma >= 0");
    hipStream_t st = (hipStream_t)stream;
    const long total = (long)n * k;
    const int grid = (int)std::min<long>((total + 255) / 256, 65536);
    hipLaunchKernelGGL(aff_mutual_kernel, dim3(grid), dim3(256), 0, st, ids, scores, weights, n, k, gamma);
    hipLaunchKernelGGL(aff_norm_kernel, dim3((unsigned)(((long)n + 255) / 256)), dim3(256), 0, st, (const float*)weights, rnorm, n, k);
    hipLaunchKernelGGL(aff_scale_kernel, dim3(grid), dim3(256), 0, st, ids, (const float*)rnorm, weights, n, k);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

int gdt_retrieval_diffuse_workspace_bytes(int n, int nq, int block, size_t* bytes) {
    GDT_REQUIRE(bytes != nullptr, "bytes");
    DfLayout L;
    GDT_CHECK(df_plan(n, nq, block, L));
    *bytes = L.total;
    return GDT_OK;
}

int gdt_retrieval_diffuse(const int* ids, const float* weights, const int* seed_ids, const float* seed_w, float* scores_t, int* iterations,
                          float* residual, int n, int k, int nq, int kq, int block, float alpha, float tol, int max_iter, void* workspace,
                          size_t workspace_bytes, void* stream) {
    GDT_REQUIRE(ids && weights && seed_ids && seed_w && scores_t && iterations && residual && workspace, "null buffer");
    DfLayout L;
    GDT_CHECK(df_check(n, k, nq, kq, block, alpha, tol, max_iter, L));
    if (L.total > workspace_bytes) return workspace_short(L.total, workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)(((uintptr_t)workspace + ALIGN - 1) / ALIGN * ALIGN);
    float* X = (float*)(ws + L.x);
    float* R = (float*)(ws + L.r);
    float* P = (float*)(ws + L.p);
    float* AP = (float*)(ws + L.ap);
    double* part = (double*)(ws + L.part);
    double* chunk = (double*)(ws + L.chunk);
    DfCtl* ctl = (DfCtl*)(ws + L.ctl);
    const dim3 rows((unsigned)L.nblk), fin(DF_FIN_THREADS);
    for (int q0 = 0; q0 < nq; q0 += block) {
        const int B = std::min(block, nq - q0), lb = df_log2_up(B);          // lb <= L.lb: the block fits the planned buffers
        const size_t total = (size_t)n << lb;
        const dim3 wg((unsigned)std::min(DF_THREADS, std::max(256, DF_ROWS << lb)));   // one thread per (row, column) up to 1024: no idle row slot
        const unsigned egrid = (unsigned)std::min<size_t>((total + 255) / 256, 65536);
        GDT_CHECK_HIP(hipMemsetAsync(X, 0, total * sizeof(float), st));
        GDT_CHECK_HIP(hipMemsetAsync(R, 0, total * sizeof(float), st));
        GDT_CHECK_HIP(hipMemsetAsync(ctl, 0, sizeof(DfCtl), st));
        hipLaunchKernelGGL(df_seed_kernel, dim3(1), dim3(64), 0, st, seed_ids, seed_w, R, n, kq, q0, B, lb);
        GDT_CHECK_HIP(hipMemcpyAsync(P, R, total * sizeof(float), hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(df_update_kernel, rows, wg, 0, st, X, R, (const float*)P, (const float*)AP, part, (const DfCtl*)ctl, n, lb, 1);
        hipLaunchKernelGGL(df_finish_kernel, dim3(1), fin, 0, st, (const double*)part, chunk, ctl, L.nblk, lb, (int)DF_FIN_FIRST, tol, max_iter);
        for (int it = 0; it < max_iter; ++it) {
            hipLaunchKernelGGL(df_spmv_kernel, rows, wg, 0, st, ids, weights, (const float*)P, AP, part, (const DfCtl*)ctl, n, k, lb, alpha);
            hipLaunchKernelGGL(df_finish_kernel, dim3(1), fin, 0, st, (const double*)part, chunk, ctl, L.nblk, lb, (int)DF_FIN_PAP, tol, max_iter);
            hipLaunchKernelGGL(df_update_kernel, rows, wg, 0, st, X, R, (const float*)P, (const float*)AP, part, (const DfCtl*)ctl, n, lb, 0);
            hipLaunchKernelGGL(df_finish_kernel, dim3(1), fin, 0, st, (const double*)part, chunk, ctl, L.nblk, lb, (int)DF_FIN_RR, tol, max_iter);
            hipLaunchKernelGGL(df_pupdate_kernel, dim3(egrid), dim3(256), 0, st, P, (const float*)R, (const DfCtl*)ctl, total, lb);
        }
        hipLaunchKernelGGL(df_output_kernel, dim3((unsigned)(((long)n + 63) / 64)), dim3(256), 0, st, (const float*)X, (const DfCtl*)ctl, scores_t,
                           iterations, residual, n, q0, B, lb);
        GDT_CHECK_HIP(hipGetLastError());
    }
    return GDT_OK;
}

int gdt_retrieval_rank_scores_workspace_bytes(int n, int nq, size_t* bytes) {
    GDT_REQUIRE(bytes != nullptr, "bytes");
    RkLayout L;
    GDT_CHECK(rk_plan(n, nq, L));
    *bytes = L.total;
    return GDT_OK;
}

int gdt_retrieval_rank_scores(const float* scores_t, int* ranks_t, int n, int nq, int index_base, void* workspace, size_t workspace_bytes,
                              void* stream) {
    GDT_REQUIRE(scores_t && ranks_t && workspace, "null buffer");
    GDT_REQUIRE(n >= 1 && nq >= 1 && (long)n * nq < (1l << 31), "n, nq >= 1 and n * nq below 2^31");
    GDT_REQUIRE(index_base >= 0 && (long)index_base + n <= 0x7fffffffl, "index_base + n must fit an int32 id");
    RkLayout L;
    GDT_CHECK(rk_plan(n, nq, L));
    if (L.total > workspace_bytes) return workspace_short(L.total, workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)(((uintptr_t)workspace + ALIGN - 1) / ALIGN * ALIGN);
    int* idx = (int*)(ws + L.idx);
    int* offs = (int*)(ws + L.offs);
    float* keys_in = (float*)(ws + L.keys_in);
    const long total = (long)n * nq;
    hipLaunchKernelGGL(rk_prepare_kernel, dim3((unsigned)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0, st, scores_t, keys_in, idx, offs, nq, n,
                       index_base);
    GDT_CHECK_HIP(hipGetLastError());
    size_t tb = L.tmp_bytes;
    GDT_CHECK_HIP(rocprim::segmented_radix_sort_pairs_desc((void*)(ws + L.tmp), tb, (const float*)keys_in, (float*)(ws + L.keys_out), (const int*)idx,
                                                           ranks_t, (unsigned)total, (unsigned)nq, (const int*)offs, (const int*)(offs + 1), 0, 32, st));
    return GDT_OK;
}

}  // extern "C"
