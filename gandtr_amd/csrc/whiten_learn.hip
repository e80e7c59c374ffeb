// Learned whitening ("Lw") on the device, in float64: produces the {m, P} that CirtorchWhiten consumes.
//   whitenlearn / cholesky      mdir/external/cirtorch/utils/whiten.py:37-70
//   learn_lw_whitening          mdir/stages/whiten.py:30-75 (values.astype(float64).T, query / positive index lists)
// Reference (numpy, float64):  m = mean(X[:, q]);  S = df df^T / n  with  df = X[:, q] - X[:, p];  P0 = inv(cholesky(S))  (with
// a growing diagonal jitter until S is positive definite);  D = (P0 (X - m)) (P0 (X - m))^T;  eigen-decomposition of D, eigenvalues
// in decreasing order;  P = eigvec^T P0.
// Here:  the two O(d^2 N) covariance products are one tiled float64 GEMM kernel reading the float32 descriptor rows directly
// (pair differences / mean-centred rows formed on the fly, fixed summation order => deterministic and exactly symmetric);
// with C = sum (x - m)(x - m)^T the reference's d x N product is never materialised: the matrix to decompose is P0 C P0^T = G G^T for
// G = P0 chol(C), and its eigenpairs are the left singular vectors / squared singular values of G, found by a one-sided (Hestenes)
// Jacobi with both columns of a pair in LDS (one pass over the matrix per round, HBM-bound at 5.9 TB/s); a two-sided cyclic Jacobi
// on P0 C P0^T is the fallback when C is singular.  Cholesky and the triangular inverse run as d short launches each (d <= 2048: a
// few tens of ms).  Eigenvectors are defined up to sign, so P's rows are too.
// PCA whitening and the PCA projection of pasted descriptors (second half of the file) reuse the same pieces:
//   pcawhitenlearn              mdir/external/cirtorch/utils/whiten.py:14-35
//   learn_pca_whitening, paste_pca_normalize, l2_normalize      mdir/stages/whiten.py:78-135
// their covariance / Gram product launches only the 64 x 64 tiles on and below the diagonal and mirrors them.
#include <math.h>
#include <string.h>

#include "../../include/gandtr_hip.h"
#include "gdt_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- GEMM
// C[m][n] = scale * sum_k A(k, m) * B(k, n)   (both operands K-major), 64 x 64 tile per workgroup, 4 x 4 per lane, K-step 16.
// Operand sources: MAT  = double matrix [K][ld];  DIFF = float rows X[q[k]] - X[p[k]];  CENT = float row X[k] - mean;
// DCENT = double rows V[k] - mean[0] (a scalar), columns >= xd read as zero (the padding column of an odd width);
// DROWS = the same matrix taken row-major on the OUTPUT side, A(k, m) = V[m][k] - mean[0] (operand a of gemm_rows_kernel only).
enum { SRC_MAT = 0, SRC_DIFF = 1, SRC_CENT = 2, SRC_DCENT = 3, SRC_DROWS = 4 };
struct Operand {
    int kind;
    const double* mat; int ld;          // SRC_MAT / SRC_DCENT / SRC_DROWS
    const float* x; int xd;             // SRC_DIFF / SRC_CENT: rows of xd floats;  SRC_DCENT / SRC_DROWS: valid columns
    const int* q; const int* p;         // SRC_DIFF
    const double* mean;                 // SRC_CENT (per column), SRC_DCENT / SRC_DROWS (one scalar)
};

__device__ __forceinline__ double fetch(const Operand& o, int k, int m) {
    if (o.kind == SRC_MAT) return o.mat[(size_t)k * o.ld + m];
    if (o.kind == SRC_DIFF) return (double)o.x[(size_t)o.q[k] * o.xd + m] - (double)o.x[(size_t)o.p[k] * o.xd + m];
    if (o.kind == SRC_DCENT) return m < o.xd ? o.mat[(size_t)k * o.ld + m] - o.mean[0] : 0.0;
    if (o.kind == SRC_DROWS) return k < o.xd ? o.mat[(size_t)m * o.ld + k] - o.mean[0] : 0.0;
    return (double)o.x[(size_t)k * o.xd + m] - o.mean[m];
}

// one 64 x 64 tile at (m0, n0).  ROWS_A: operand a is row-major on the output side (SRC_DROWS), so its 16 x 64 stage is read with k
// fastest across lanes.  mirror: also store the transposed tile (lower-triangle launches of a symmetric product, M = N = ldc).
template <bool ROWS_A>
__device__ __forceinline__ void gemm_tile(const Operand& a, const Operand& b, double* __restrict__ c, int M, int N, int K, int ldc, double scale,
                                          int m0, int n0, bool mirror) {
    __shared__ double as[16][64 + 1];
    __shared__ double bs[16][64 + 1];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    double acc[4][4] = {};
    for (int k0 = 0; k0 < K; k0 += 16) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {                       // 16 x 64 elements per operand, 4 per lane
            const int e = tid + i * 256, kk = e >> 6, mm = e & 63;
            const bool ok = k0 + kk < K;
            if (ROWS_A) {
                const int ka = e & 15, ma = e >> 4;
                as[ka][ma] = (k0 + ka < K && m0 + ma < M) ? fetch(a, k0 + ka, m0 + ma) : 0.0;
            } else {
                as[kk][mm] = (ok && m0 + mm < M) ? fetch(a, k0 + kk, m0 + mm) : 0.0;
            }
            bs[kk][mm] = (ok && n0 + mm < N) ? fetch(b, k0 + kk, n0 + mm) : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            double av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { av[i] = as[kk][ty * 4 + i]; bv[i] = bs[kk][tx * 4 + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fma(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = m0 + ty * 4 + i, n = n0 + tx * 4 + j;
            if (m < M && n < N) {
                c[(size_t)m * ldc + n] = acc[i][j] * scale;
                if (mirror) c[(size_t)n * ldc + m] = acc[i][j] * scale;
            }
        }
}

__global__ __launch_bounds__(256) void gemm_kk_kernel(Operand a, Operand b, double* __restrict__ c, int M, int N, int K, double scale) {
    gemm_tile<false>(a, b, c, M, N, K, N, scale, blockIdx.y * 64, blockIdx.x * 64, false);
}
// symmetric product A^T A (both operands the same, M x M): workgroup t computes tile (r, c) of the lower triangle, c <= r, t = r (r + 1) / 2 + c,
// and stores it at both places; a diagonal tile is computed whole (element (m, n) and (n, m) run the same fma chain, so they are equal bits).
__global__ __launch_bounds__(256) void gemm_lower_kernel(Operand a, double* __restrict__ c, int M, int K, double scale) {
    const int t = blockIdx.x;
    int r = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while ((r + 1) * (r + 2) / 2 <= t) ++r;
    while (r * (r + 1) / 2 > t) --r;
    const int col = t - r * (r + 1) / 2;
    gemm_tile<false>(a, a, c, M, M, K, M, scale, r * 64, col * 64, col != r);
}
// out[m][n] = sum_k A(k, m) B(k, n) with operand a row-major on the output side (SRC_DROWS); row stride of c: ldc
__global__ __launch_bounds__(256) void gemm_rows_kernel(Operand a, Operand b, double* __restrict__ c, int M, int N, int K, int ldc) {
    gemm_tile<true>(a, b, c, M, N, K, ldc, 1.0, blockIdx.y * 64, blockIdx.x * 64, false);
}

__global__ __launch_bounds__(256) void transpose_kernel(const double* __restrict__ a, double* __restrict__ t, int d) {
    __shared__ double tile[32][33];
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y0 = blockIdx.y * 32;
    for (int r = threadIdx.x >> 5; r < 32; r += 8)
        if (x < d && y0 + r < d) tile[r][threadIdx.x & 31] = a[(size_t)(y0 + r) * d + x];
    __syncthreads();
    const int xt = blockIdx.y * 32 + (threadIdx.x & 31), yt0 = blockIdx.x * 32;
    for (int r = threadIdx.x >> 5; r < 32; r += 8)
        if (xt < d && yt0 + r < d) t[(size_t)(yt0 + r) * d + xt] = tile[threadIdx.x & 31][r];
}

// m[c] = mean over the query rows, sequential in pair order (one lane per column)
__global__ __launch_bounds__(256) void mean_kernel(const float* __restrict__ x, const int* __restrict__ q, int n, int d, double* __restrict__ m) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += (double)x[(size_t)q[i] * d + c];
    m[c] = s / (double)n;
}

// ---------------------------------------------------------------------------------------------------------------- Cholesky
// a: working copy of S (+ alpha I), overwritten by L in its lower triangle.  Right-looking, one column per step.
__global__ __launch_bounds__(256) void chol_column_kernel(double* __restrict__ a, int d, int k, int* __restrict__ fail) {
    const double piv = a[(size_t)k * d + k];           // stays in place until chol_diag_kernel: every workgroup of this launch reads it
    if (!(piv > 0.0)) { if (threadIdx.x == 0 && blockIdx.x == 0) *fail = 1; return; }
    const double l = sqrt(piv);
    const int i = k + 1 + blockIdx.x * 256 + threadIdx.x;
    if (i < d) a[(size_t)i * d + k] /= l;
}
__global__ __launch_bounds__(256) void chol_diag_kernel(double* __restrict__ a, int d) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < d) a[(size_t)k * d + k] = sqrt(a[(size_t)k * d + k]);
}
// a <- (a + a^T) / 2 (the two triple products are equal only up to rounding)
__global__ __launch_bounds__(256) void symmetrise_kernel(double* __restrict__ a, int d) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)d * d) return;
    const int r = (int)(i / d), c = (int)(i % d);
    if (c <= r) return;
    const double v = 0.5 * (a[(size_t)r * d + c] + a[(size_t)c * d + r]);
    a[(size_t)r * d + c] = v; a[(size_t)c * d + r] = v;
}
__global__ __launch_bounds__(256) void chol_update_kernel(double* __restrict__ a, int d, int k, const int* __restrict__ fail) {
    if (*fail) return;
    const int j = k + 1 + blockIdx.x * 64 + (threadIdx.x & 63), i = k + 1 + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= d || j > i) return;                                       // lower triangle only
    a[(size_t)i * d + j] -= a[(size_t)i * d + k] * a[(size_t)j * d + k];
}
__global__ __launch_bounds__(256) void add_diag_copy_kernel(const double* __restrict__ s, double* __restrict__ a, int d, double alpha) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)d * d) return;
    const int r = (int)(i / d), c = (int)(i % d);
    a[i] = s[i] + (r == c ? alpha : 0.0);
}
// X = L^-1 (lower triangular), one row per step: X[k][j] = (delta_kj - sum_{j<=t<k} L[k][t] X[t][j]) / L[k][k].  The sum over t is
// split into TRI_PARTS fixed chunks (one workgroup each, partial sums in `part`), combined in chunk order by the second kernel.
constexpr int TRI_PARTS = 16;
__global__ __launch_bounds__(256) void tri_inverse_partial_kernel(const double* __restrict__ l, const double* __restrict__ x,
                                                                  double* __restrict__ part, int d, int k) {
    const int j = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (j >= d) return;
    const int len = (k + TRI_PARTS - 1) / TRI_PARTS, t0 = max(c * len, j), t1 = min((c + 1) * len, k);     // X[t][j] = 0 for t < j
    double s = 0.0;
    for (int t = t0; t < t1; ++t) s += l[(size_t)k * d + t] * x[(size_t)t * d + j];
    part[(size_t)c * d + j] = s;
}
__global__ __launch_bounds__(256) void tri_inverse_finish_kernel(const double* __restrict__ l, double* __restrict__ x,
                                                                 const double* __restrict__ part, int d, int k) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d) return;
    double s = 0.0;
    if (j <= k) {
        s = (j == k) ? 1.0 : 0.0;
#pragma unroll
        for (int c = 0; c < TRI_PARTS; ++c) s -= part[(size_t)c * d + j];
        s /= l[(size_t)k * d + k];
    }
    x[(size_t)k * d + j] = s;
}

// ---------------------------------------------------------------------------------------------------------------- Jacobi
// round-robin tournament on d players (d even): round r, pair k -> (p, q), p < q
__device__ __forceinline__ void pair_of(int d, int r, int k, int& p, int& q) {
    const int n1 = d - 1;
    int a, b;
    if (k == 0) { a = n1; b = r % n1; }
    else { a = (r + k) % n1; b = (r - k + n1) % n1; }
    p = min(a, b); q = max(a, b);
}
__global__ __launch_bounds__(256) void jacobi_angles_kernel(const double* __restrict__ a, int d, int r, double* __restrict__ cs) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= d / 2) return;
    int p, q;
    pair_of(d, r, k, p, q);
    const double apq = a[(size_t)p * d + q], app = a[(size_t)p * d + p], aqq = a[(size_t)q * d + q];
    double c = 1.0, s = 0.0;
    if (fabs(apq) > 1e-300 && fabs(apq) > 1e-18 * sqrt(fabs(app * aqq))) {
        const double tau = (aqq - app) / (2.0 * apq);
        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
        c = 1.0 / sqrt(1.0 + t * t);
        s = t * c;
    }
    cs[2 * k] = c; cs[2 * k + 1] = s;
}
// A <- J^T A: rows p and q of every pair, coalesced over the columns
__global__ __launch_bounds__(256) void jacobi_rows_kernel(double* __restrict__ a, int d, int r, const double* __restrict__ cs) {
    const int k = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d) return;
    int p, q;
    pair_of(d, r, k, p, q);
    const double c = cs[2 * k], s = cs[2 * k + 1];
    const double ap = a[(size_t)p * d + j], aq = a[(size_t)q * d + j];
    a[(size_t)p * d + j] = c * ap - s * aq;
    a[(size_t)q * d + j] = s * ap + c * aq;
}
// M <- M J for M = A (rows 0..d-1) and V (rows d..2d-1): one workgroup per row, the row held in LDS
__global__ __launch_bounds__(256) void jacobi_cols_kernel(double* __restrict__ a, double* __restrict__ v, int d, int r,
                                                          const double* __restrict__ cs) {
    extern __shared__ double row[];
    double* m = (blockIdx.x < (unsigned)d) ? a + (size_t)blockIdx.x * d : v + (size_t)(blockIdx.x - d) * d;
    for (int j = threadIdx.x; j < d; j += 256) row[j] = m[j];
    __syncthreads();
    for (int k = threadIdx.x; k < d / 2; k += 256) {
        int p, q;
        pair_of(d, r, k, p, q);
        const double c = cs[2 * k], s = cs[2 * k + 1];
        const double mp = row[p], mq = row[q];
        row[p] = c * mp - s * mq;
        row[q] = s * mp + c * mq;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < d; j += 256) m[j] = row[j];
}
// out[0] = sum of squared off-diagonal entries, out[1] = sum of squared diagonal entries (fixed order: one workgroup)
__global__ __launch_bounds__(1024) void offdiag_kernel(const double* __restrict__ a, int d, double* __restrict__ out) {
    __shared__ double so[1024], sd[1024];
    double o = 0.0, g = 0.0;
    for (size_t i = threadIdx.x; i < (size_t)d * d; i += 1024) {
        const double v = a[i];
        if (i / d == i % d) g += v * v; else o += v * v;
    }
    so[threadIdx.x] = o; sd[threadIdx.x] = g;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { so[threadIdx.x] += so[threadIdx.x + s]; sd[threadIdx.x] += sd[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[0] = so[0]; out[1] = sd[0]; }
}
__global__ __launch_bounds__(256) void identity_kernel(double* __restrict__ v, int d) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)d * d) v[i] = (i / d == i % d) ? 1.0 : 0.0;
}
// values a[i * stride] (the diagonal of A: stride d + 1); order[i] = index of the i-th largest (ties by index): O(d^2) ranking, d <= a few thousand
__global__ __launch_bounds__(256) void rank_desc_kernel(const double* __restrict__ a, size_t stride, int d, int* __restrict__ order,
                                                        double* __restrict__ eig) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d) return;
    const double li = a[(size_t)i * stride];
    int rank = 0;
    for (int j = 0; j < d; ++j) {
        const double lj = a[(size_t)j * stride];
        rank += (lj > li) || (lj == li && j < i);
    }
    order[rank] = i;
    if (eig) eig[rank] = li;
}
// vs[k][i] = v[k][order[i]]
__global__ __launch_bounds__(256) void gather_cols_kernel(const double* __restrict__ v, const int* __restrict__ order, double* __restrict__ vs, int d) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)d * d) return;
    const int k = (int)(i / d), c = (int)(i % d);
    vs[i] = v[(size_t)k * d + order[c]];
}

// ---------------------------------------------------------------------------------------------------------------- one-sided Jacobi
// With C = Lc Lc^T the matrix D = P0 C P0^T is G G^T for G = P0 Lc, so the eigenvectors of D are the left singular vectors of G and
// the eigenvalues the squared singular values: Hestenes' one-sided Jacobi orthogonalises the COLUMNS of G by plane rotations.  gt
// holds G transposed (row i = column i of G, contiguous).  One workgroup per pair: both columns (2 x d doubles) sit in LDS between
// the dot products and the rotation, so a round moves the matrix once (the two-sided form below moves A and V three times).
__global__ __launch_bounds__(256) void hestenes_round_kernel(double* __restrict__ gt, int d, int r, int* __restrict__ changed, double tol2) {
    extern __shared__ double cols[];                 // [2][d]
    __shared__ double part[3][4];
    int p, q;
    pair_of(d, r, blockIdx.x, p, q);
    double* rp = gt + (size_t)p * d;
    double* rq = gt + (size_t)q * d;
    double a = 0.0, b = 0.0, g = 0.0;
    for (int j = threadIdx.x; j < d; j += 256) {
        const double x = rp[j], y = rq[j];
        cols[j] = x; cols[d + j] = y;
        a = fma(x, x, a); b = fma(y, y, b); g = fma(x, y, g);
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) { a += __shfl_xor(a, m); b += __shfl_xor(b, m); g += __shfl_xor(g, m); }      // fixed butterfly order
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = a; part[1][threadIdx.x >> 6] = b; part[2][threadIdx.x >> 6] = g; }
    __syncthreads();
    a = (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
    b = (part[1][0] + part[1][1]) + (part[1][2] + part[1][3]);
    g = (part[2][0] + part[2][1]) + (part[2][2] + part[2][3]);
    if (!(g * g > tol2 * a * b)) return;             // already orthogonal to working precision (uniform across the workgroup)
    if (threadIdx.x == 0) *changed = 1;
    const double zeta = (b - a) / (2.0 * g);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
    for (int j = threadIdx.x; j < d; j += 256) {
        const double x = cols[j], y = cols[d + j];
        rp[j] = c * x - s * y;
        rq[j] = s * x + c * y;
    }
}
// lam[i] = |row i|^2 (one workgroup per row, fixed reduction order)
__global__ __launch_bounds__(256) void row_norm2_kernel(const double* __restrict__ gt, int d, double* __restrict__ lam) {
    __shared__ double part[4];
    const double* row = gt + (size_t)blockIdx.x * d;
    double a = 0.0;
    for (int j = threadIdx.x; j < d; j += 256) a = fma(row[j], row[j], a);
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) a += __shfl_xor(a, m);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) lam[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}
// us[k][i] = gt[order[i]][k] / sqrt(lam[order[i]]): unit left singular vectors as columns, in eigenvalue order
__global__ __launch_bounds__(256) void unit_columns_kernel(const double* __restrict__ gt, const double* __restrict__ lam,
                                                           const int* __restrict__ order, double* __restrict__ us, int d) {
    __shared__ double tile[32][33];
    const int i0 = blockIdx.y * 32, k0 = blockIdx.x * 32, tx = threadIdx.x & 31;
    for (int r = threadIdx.x >> 5; r < 32; r += 8) {
        const int i = i0 + r, k = k0 + tx;
        if (i < d && k < d) { const int src = order[i]; tile[r][tx] = gt[(size_t)src * d + k] / sqrt(lam[src]); }
    }
    __syncthreads();
    for (int r = threadIdx.x >> 5; r < 32; r += 8) {
        const int k = k0 + r, i = i0 + tx;
        if (i < d && k < d) us[(size_t)k * d + i] = tile[tx][r];
    }
}
__global__ __launch_bounds__(256) void zero_upper_kernel(double* __restrict__ a, int d) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)d * d && (int)(i % d) > (int)(i / d)) a[i] = 0.0;
}

constexpr size_t ALIGN = 256;
inline size_t align_up(size_t v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }
struct Layout { size_t s, l, p0, t1, t2, a, v, cs, flag, red, order, total; };
int plan(int n_vec, int d, int n_pairs, Layout& L) {
    GDT_REQUIRE(n_vec >= 1 && n_pairs >= 1, "whiten_learn: empty input");
    GDT_REQUIRE(d >= 2 && d % 2 == 0 && d <= 8192, "whiten_learn: descriptor size must be even and <= 8192");
    const size_t dd = align_up((size_t)d * d * sizeof(double));
    size_t off = 0;
    L.s = off; off += dd; L.l = off; off += dd; L.p0 = off; off += dd; L.t1 = off; off += dd; L.t2 = off; off += dd;
    L.a = off; off += dd; L.v = off; off += dd;
    L.cs = off; off += align_up((size_t)d * sizeof(double));
    L.flag = off; off += ALIGN; L.red = off; off += ALIGN;
    L.order = off; off += align_up((size_t)d * sizeof(int));
    L.total = off + ALIGN;
    return GDT_OK;
}

// in-place right-looking Cholesky of the lower triangle of `a`; failed = 1 when a pivot is not positive (synchronises the stream)
int cholesky_inplace(hipStream_t st, double* a, int d, int* flag, int& failed) {
    GDT_CHECK_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
    for (int k = 0; k < d; ++k) {
        hipLaunchKernelGGL(chol_column_kernel, dim3((d - k - 1 + 255) / 256 + (k == d - 1 ? 1 : 0)), dim3(256), 0, st, a, d, k, flag);
        if (k + 1 < d)
            hipLaunchKernelGGL(chol_update_kernel, dim3((d - k - 1 + 63) / 64, (d - k - 1 + 3) / 4), dim3(256), 0, st, a, d, k, flag);
    }
    hipLaunchKernelGGL(chol_diag_kernel, dim3((d + 255) / 256), dim3(256), 0, st, a, d);
    failed = 0;
    GDT_CHECK_HIP(hipMemcpyAsync(&failed, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    GDT_CHECK_HIP(hipStreamSynchronize(st));
    return GDT_OK;
}

Operand mat(const double* m, int ld) { Operand o = {}; o.kind = SRC_MAT; o.mat = m; o.ld = ld; return o; }

void gemm(hipStream_t st, const Operand& a, const Operand& b, double* c, int M, int N, int K, double scale) {
    hipLaunchKernelGGL(gemm_kk_kernel, dim3((N + 63) / 64, (M + 63) / 64), dim3(256), 0, st, a, b, c, M, N, K, scale);
}

// Hestenes sweeps over the rows of gt until a sweep rotates nothing (at most 60); synchronises the stream once per sweep
int hestenes_sweeps(hipStream_t st, double* gt, int d, int* flag, int& sweeps, bool& converged) {
    for (; sweeps < 60; ++sweeps) {
        GDT_CHECK_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
        for (int r = 0; r < d - 1; ++r)
            hipLaunchKernelGGL(hestenes_round_kernel, dim3(d / 2), dim3(256), (size_t)2 * d * sizeof(double), st, gt, d, r, flag, 1e-28);
        int changed = 0;
        GDT_CHECK_HIP(hipMemcpyAsync(&changed, flag, sizeof(int), hipMemcpyDeviceToHost, st));
        GDT_CHECK_HIP(hipStreamSynchronize(st));
        if (!changed) { ++sweeps; converged = true; break; }
    }
    return GDT_OK;
}
// two-sided cyclic Jacobi sweeps on the symmetric A, V accumulating the rotations, until the off-diagonal norm is below 1e-13 of the diagonal's (at most 40)
int jacobi_sweeps(hipStream_t st, double* A, double* V, int d, double* cs, double* red, int& sweeps, bool& converged) {
    for (; sweeps < 40; ++sweeps) {
        hipLaunchKernelGGL(offdiag_kernel, dim3(1), dim3(1024), 0, st, A, d, red);
        double h[2];
        GDT_CHECK_HIP(hipMemcpyAsync(h, red, sizeof(h), hipMemcpyDeviceToHost, st));
        GDT_CHECK_HIP(hipStreamSynchronize(st));
        if (!(h[0] > 1e-26 * h[1])) { converged = true; break; }
        for (int r = 0; r < d - 1; ++r) {
            hipLaunchKernelGGL(jacobi_angles_kernel, dim3((d / 2 + 255) / 256), dim3(256), 0, st, A, d, r, cs);
            hipLaunchKernelGGL(jacobi_rows_kernel, dim3((d + 255) / 256, d / 2), dim3(256), 0, st, A, d, r, cs);
            hipLaunchKernelGGL(jacobi_cols_kernel, dim3(2 * d), dim3(256), (size_t)d * sizeof(double), st, A, V, d, r, cs);
        }
    }
    return GDT_OK;
}


// ---------------------------------------------------------------------------------------------------------------- PCA whitening
// column sums of rows [c * len, (c + 1) * len) of x (MEAN_PARTS fixed chunks, one lane per column), combined in chunk order below
constexpr int MEAN_PARTS = 64;
__global__ __launch_bounds__(256) void mean_all_partial_kernel(const float* __restrict__ x, int n, int d, double* __restrict__ part) {
    const int c = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (c >= d) return;
    const int len = (n + MEAN_PARTS - 1) / MEAN_PARTS, i0 = min(k * len, n), i1 = min(i0 + len, n);
    double s = 0.0;
    for (int i = i0; i < i1; ++i) s += (double)x[(size_t)i * d + c];
    part[(size_t)k * d + c] = s;
}
__global__ __launch_bounds__(256) void mean_all_finish_kernel(const double* __restrict__ part, int n, int d, double* __restrict__ m) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    double s = 0.0;
    for (int k = 0; k < MEAN_PARTS; ++k) s += part[(size_t)k * d + c];
    m[c] = s / (double)n;
}
// sum of all entries of v in two fixed stages: SUM_BLOCKS workgroups of strided partial sums, then one workgroup; out[0] = sum / count
constexpr int SUM_BLOCKS = 256;
__device__ __forceinline__ double block_sum_256(double a, double* part) {      // part: 4 doubles of LDS; result valid in every lane
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) a += __shfl_xor(a, m);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}
__global__ __launch_bounds__(256) void sum_partial_kernel(const double* __restrict__ v, size_t count, double* __restrict__ part) {
    __shared__ double red[4];
    double a = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)SUM_BLOCKS * 256) a += v[i];
    a = block_sum_256(a, red);
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}
__global__ __launch_bounds__(256) void sum_finish_kernel(const double* __restrict__ part, size_t count, double* __restrict__ out) {
    __shared__ double red[4];
    const double a = block_sum_256(threadIdx.x < SUM_BLOCKS ? part[threadIdx.x] : 0.0, red);
    if (threadIdx.x == 0) out[0] = a / (double)count;
}
// out[i] = v[i] / |v[i]|_2, no epsilon (one workgroup per row, fixed reduction order; in place allowed)
__global__ __launch_bounds__(256) void l2n_rows_f64_kernel(const double* v, double* out, int d) {
    __shared__ double red[4];
    const double* row = v + (size_t)blockIdx.x * d;
    double* dst = out + (size_t)blockIdx.x * d;
    double a = 0.0;
    for (int j = threadIdx.x; j < d; j += 256) a = fma(row[j], row[j], a);
    const double norm = sqrt(block_sum_256(a, red));
    for (int j = threadIdx.x; j < d; j += 256) dst[j] = row[j] / norm;
}
// rows[i][k] = gt[order[i]][k] / sqrt(lam[order[i]]): the unit left singular vectors as ROWS, in eigenvalue order
__global__ __launch_bounds__(256) void unit_rows_kernel(const double* __restrict__ gt, const double* __restrict__ lam, const int* __restrict__ order,
                                                        double* __restrict__ rows, int d) {
    const int src = order[blockIdx.x];
    const double s = sqrt(lam[src]);
    for (int j = threadIdx.x; j < d; j += 256) rows[(size_t)blockIdx.x * d + j] = gt[(size_t)src * d + j] / s;
}
__global__ void set_value_kernel(double* __restrict__ a, double value) { a[0] = value; }
// Arun's shrinkage (cirtorch/utils/whiten.py:28-31): lamp[i] = (1 - b) eig[i] + b with b = eig[shrink - 1] (shrink = 0: lamp = eig).  bad[0] = the first
// index whose value is not above d 2^-52 lamp[0] (or is not finite), -1 when there is none; bad_value[0] = that value.  One lane: d <= 8192.
__global__ void pca_shrink_kernel(const double* __restrict__ eig, int d, int shrink, double* __restrict__ lamp, int* __restrict__ bad, double* __restrict__ bad_value) {
    const double b = shrink ? eig[shrink - 1] : 0.0;
    int first = -1;
    double thr = 0.0;
    for (int i = 0; i < d; ++i) {
        const double l = shrink ? (1.0 - b) * eig[i] + b : eig[i];
        lamp[i] = l;
        if (i == 0) thr = (double)d * 2.220446049250313e-16 * l;
        if (first < 0 && !(l > thr && isfinite(l))) { first = i; bad_value[0] = l; }
    }
    bad[0] = first;
}
// P[i][j] = rows[i][j] / sqrt(lamp[i])
__global__ __launch_bounds__(256) void pca_scale_rows_kernel(const double* __restrict__ rows, const double* __restrict__ lamp, double* __restrict__ p, int d) {
    const double s = sqrt(lamp[blockIdx.x]);
    for (int j = threadIdx.x; j < d; j += 256) p[(size_t)blockIdx.x * d + j] = rows[(size_t)blockIdx.x * d + j] / s;
}

void gemm_lower(hipStream_t st, const Operand& a, double* c, int M, int K, double scale) {
    const int t = (M + 63) / 64;
    hipLaunchKernelGGL(gemm_lower_kernel, dim3(t * (t + 1) / 2), dim3(256), 0, st, a, c, M, K, scale);
}

// Eigenpairs of the symmetric d x d matrix C (d even): unit eigenvectors as the ROWS of *rows_out (one of the buffers below), eigenvalues decreasing in
// eig.  Cholesky C = Lc Lc^T and Hestenes on Lc when C is positive definite and two columns fit in LDS, else the two-sided cyclic Jacobi on C.  padded:
// the last row / column of C is zero padding (its eigenvalue 0 is made to rank last whatever the rounding of the other zero eigenvalues).
struct EigBuffers { double *A, *V, *T1, *cs, *red, *eig; int *flag, *order; };
int sym_eig(hipStream_t st, const double* C, int d, bool padded, const EigBuffers& w, double** rows_out, int& sweeps, bool& one_sided, bool& converged) {
    const unsigned dd_blocks = (unsigned)(((size_t)d * d + 255) / 256);
    const dim3 tgrid((d + 31) / 32, (d + 31) / 32);
    int rc, c_failed = 1;
    sweeps = 0; converged = false;
    hipLaunchKernelGGL(add_diag_copy_kernel, dim3(dd_blocks), dim3(256), 0, st, C, w.A, d, 0.0);
    if (!padded && (size_t)2 * d * sizeof(double) <= 64 * 1024) {
        rc = cholesky_inplace(st, w.A, d, w.flag, c_failed);
        if (rc != GDT_OK) return rc;
        if (c_failed) hipLaunchKernelGGL(add_diag_copy_kernel, dim3(dd_blocks), dim3(256), 0, st, C, w.A, d, 0.0);
    }
    one_sided = !c_failed;
    if (one_sided) {
        hipLaunchKernelGGL(zero_upper_kernel, dim3(dd_blocks), dim3(256), 0, st, w.A, d);                       // A = Lc
        hipLaunchKernelGGL(transpose_kernel, tgrid, dim3(256), 0, st, w.A, w.V, d);                              // V = Lc^T: row i = column i of Lc
        rc = hestenes_sweeps(st, w.V, d, w.flag, sweeps, converged);
        if (rc != GDT_OK) return rc;
        hipLaunchKernelGGL(row_norm2_kernel, dim3(d), dim3(256), 0, st, w.V, d, w.cs);
        hipLaunchKernelGGL(rank_desc_kernel, dim3((d + 255) / 256), dim3(256), 0, st, w.cs, (size_t)1, d, w.order, w.eig);
        hipLaunchKernelGGL(unit_rows_kernel, dim3(d), dim3(256), 0, st, w.V, w.cs, w.order, w.T1, d);
        *rows_out = w.T1;
    } else {
        hipLaunchKernelGGL(identity_kernel, dim3(dd_blocks), dim3(256), 0, st, w.V, d);
        rc = jacobi_sweeps(st, w.A, w.V, d, w.cs, w.red, sweeps, converged);
        if (rc != GDT_OK) return rc;
        // the padding column never rotates (its off-diagonal entries are exact zeros): it is still eigenvector d - 1
        if (padded) hipLaunchKernelGGL(set_value_kernel, dim3(1), dim3(1), 0, st, w.A + (size_t)(d - 1) * (d + 1), -1.7976931348623157e308);
        hipLaunchKernelGGL(rank_desc_kernel, dim3((d + 255) / 256), dim3(256), 0, st, w.A, (size_t)d + 1, d, w.order, w.eig);
        hipLaunchKernelGGL(gather_cols_kernel, dim3(dd_blocks), dim3(256), 0, st, w.V, w.order, w.T1, d);       // T1[k][i] = V[k][order[i]]
        hipLaunchKernelGGL(transpose_kernel, tgrid, dim3(256), 0, st, w.T1, w.A, d);                             // A[i][k]: eigenvectors as rows
        *rows_out = w.A;
    }
    return GDT_OK;
}

struct PcaLayout { size_t c, a, v, t1, m2, cs, eig, lamp, part, flag, red, order, total; };
int pca_plan(int n, int d, bool pad_odd, const char* what, PcaLayout& L, int& dp) {
    if (n < 1) { gdt_set_error(std::string(what) + ": empty input"); return GDT_ERR_INVALID; }
    dp = d + ((pad_odd && d % 2) ? 1 : 0);
    if (d < 1 || dp < 2 || dp % 2 != 0 || dp > 8192) {
        gdt_set_error(std::string(what) + (pad_odd ? ": width must be 1..8191" : ": descriptor size must be even and <= 8192"));
        return GDT_ERR_INVALID;
    }
    const size_t dd = align_up((size_t)dp * dp * sizeof(double)), dv = align_up((size_t)dp * sizeof(double));
    size_t off = 0;
    L.c = off; off += dd; L.a = off; off += dd; L.v = off; off += dd; L.t1 = off; off += dd;
    L.m2 = off; off += pad_odd ? dd : 0;                                          // the projector V_k V_k^T
    L.cs = off; off += dv; L.eig = off; off += dv; L.lamp = off; off += dv;
    L.part = off; off += align_up(((size_t)MEAN_PARTS * dp > (size_t)SUM_BLOCKS ? (size_t)MEAN_PARTS * dp : (size_t)SUM_BLOCKS) * sizeof(double));
    L.flag = off; off += ALIGN; L.red = off; off += ALIGN;
    L.order = off; off += align_up((size_t)dp * sizeof(int));
    L.total = off + ALIGN;
    return GDT_OK;
}
EigBuffers eig_buffers(char* ws, const PcaLayout& L) {
    EigBuffers w;
    w.A = (double*)(ws + L.a); w.V = (double*)(ws + L.v); w.T1 = (double*)(ws + L.t1); w.cs = (double*)(ws + L.cs);
    w.red = (double*)(ws + L.red); w.eig = (double*)(ws + L.eig); w.flag = (int*)(ws + L.flag); w.order = (int*)(ws + L.order);
    return w;
}
int not_converged(const char* what, int sweeps) {
    gdt_set_error(std::string(what) + ": the Jacobi eigensolver stopped at its sweep cap (" + std::to_string(sweeps) + " sweeps) without converging");
    return GDT_ERR_NOT_CONVERGED;
}

}  // namespace

extern "C" {

int gdt_whiten_learn_workspace_bytes(int n_vec, int d, int n_pairs, size_t* bytes) {
    GDT_REQUIRE(bytes != nullptr, "bytes");
    Layout L;
    int rc = plan(n_vec, d, n_pairs, L);
    if (rc != GDT_OK) return rc;
    *bytes = L.total;
    return GDT_OK;
}

int gdt_whiten_learn(const float* x, const int* qidx, const int* pidx, int n_vec, int d, int n_pairs, double* m_out, double* p_out,
                     double* eig_out, int* info, void* workspace, size_t workspace_bytes, void* stream_) {
    Layout L;
    int rc = plan(n_vec, d, n_pairs, L);
    if (rc != GDT_OK) return rc;
    GDT_REQUIRE(x && qidx && pidx && m_out && p_out && workspace, "whiten_learn: null buffer");
    if (workspace_bytes < L.total) { gdt_set_error("whiten_learn: workspace too small"); return GDT_ERR_WORKSPACE; }
    hipStream_t st = (hipStream_t)stream_;
    char* ws = (char*)(((uintptr_t)workspace + ALIGN - 1) / ALIGN * ALIGN);
    double *S = (double*)(ws + L.s), *Lm = (double*)(ws + L.l), *P0 = (double*)(ws + L.p0), *T1 = (double*)(ws + L.t1),
           *T2 = (double*)(ws + L.t2), *A = (double*)(ws + L.a), *V = (double*)(ws + L.v), *cs = (double*)(ws + L.cs),
           *red = (double*)(ws + L.red);
    int* flag = (int*)(ws + L.flag);
    int* order = (int*)(ws + L.order);
    const unsigned dd_blocks = (unsigned)(((size_t)d * d + 255) / 256);

    // m = mean of the query vectors; S = df df^T / n
    hipLaunchKernelGGL(mean_kernel, dim3((d + 255) / 256), dim3(256), 0, st, x, qidx, n_pairs, d, m_out);
    Operand df = {}; df.kind = SRC_DIFF; df.x = x; df.xd = d; df.q = qidx; df.p = pidx;
    gemm(st, df, df, S, d, d, n_pairs, 1.0 / (double)n_pairs);

    // L = cholesky(S + alpha I), alpha = 0, 1e-10, 1e-9, ... until positive definite (whiten.py:55-70)
    double alpha = 0.0;
    int jitter_steps = 0;
    for (;;) {
        hipLaunchKernelGGL(add_diag_copy_kernel, dim3(dd_blocks), dim3(256), 0, st, S, Lm, d, alpha);
        int failed = 0;
        rc = cholesky_inplace(st, Lm, d, flag, failed);
        if (rc != GDT_OK) return rc;
        if (!failed) break;
        alpha = alpha == 0.0 ? 1e-10 : alpha * 10.0;
        ++jitter_steps;
        if (jitter_steps > 40) { gdt_set_error("whiten_learn: matrix is not positive definite"); return GDT_ERR_INVALID; }
    }
    // P0 = L^-1
    for (int k = 0; k < d; ++k) {
        hipLaunchKernelGGL(tri_inverse_partial_kernel, dim3((d + 255) / 256, TRI_PARTS), dim3(256), 0, st, Lm, P0, T1, d, k);      // T1: scratch
        hipLaunchKernelGGL(tri_inverse_finish_kernel, dim3((d + 255) / 256), dim3(256), 0, st, Lm, P0, T1, d, k);
    }

    // C = sum (x - m)(x - m)^T over ALL vectors; D = P0 C P0^T
    Operand ce = {}; ce.kind = SRC_CENT; ce.x = x; ce.xd = d; ce.mean = m_out;
    gemm(st, ce, ce, T1, d, d, n_vec, 1.0);                                                    // T1 = C (symmetric)
    hipLaunchKernelGGL(transpose_kernel, dim3((d + 31) / 32, (d + 31) / 32), dim3(256), 0, st, P0, T2, d);      // T2 = P0^T  ([k][i] = P0[i][k])
    // preferred: one-sided Jacobi on G = P0 Lc (needs C positive definite and both columns of a pair in LDS)
    int sweeps = 0;
    int c_failed = 1;
    bool converged = false;
    if ((size_t)2 * d * sizeof(double) <= 64 * 1024) {
        hipLaunchKernelGGL(add_diag_copy_kernel, dim3(dd_blocks), dim3(256), 0, st, T1, A, d, 0.0);
        rc = cholesky_inplace(st, A, d, flag, c_failed);
        if (rc != GDT_OK) return rc;
    }
    if (!c_failed) {
        hipLaunchKernelGGL(zero_upper_kernel, dim3(dd_blocks), dim3(256), 0, st, A, d);                        // A = Lc
        gemm(st, mat(A, d), mat(T2, d), V, d, d, d, 1.0);                 // V = G^T: V[i][k] = sum_j Lc[j][i] P0[k][j]
        rc = hestenes_sweeps(st, V, d, flag, sweeps, converged);
        if (rc != GDT_OK) return rc;
        hipLaunchKernelGGL(row_norm2_kernel, dim3(d), dim3(256), 0, st, V, d, cs);                              // cs = eigenvalues (unordered)
        hipLaunchKernelGGL(rank_desc_kernel, dim3((d + 255) / 256), dim3(256), 0, st, cs, (size_t)1, d, order, eig_out);
        hipLaunchKernelGGL(unit_columns_kernel, dim3((d + 31) / 32, (d + 31) / 32), dim3(256), 0, st, V, cs, order, T1, d);
    } else {
        // fallback (C singular, or d too large for the LDS form): two-sided cyclic Jacobi on A = P0 C P0^T, V accumulates the rotations
        gemm(st, mat(T2, d), mat(T1, d), A, d, d, d, 1.0);                                         // A = P0 C        (sum_k P0[i][k] C[k][j])
        hipLaunchKernelGGL(transpose_kernel, dim3((d + 31) / 32, (d + 31) / 32), dim3(256), 0, st, A, T1, d);       // T1 = (P0 C)^T
        gemm(st, mat(T1, d), mat(T2, d), A, d, d, d, 1.0);                                         // A = (P0 C) P0^T (sum_k (P0C)[i][k] P0[j][k])
        hipLaunchKernelGGL(symmetrise_kernel, dim3(dd_blocks), dim3(256), 0, st, A, d);
        hipLaunchKernelGGL(identity_kernel, dim3(dd_blocks), dim3(256), 0, st, V, d);
        rc = jacobi_sweeps(st, A, V, d, cs, red, sweeps, converged);
        if (rc != GDT_OK) return rc;
        hipLaunchKernelGGL(rank_desc_kernel, dim3((d + 255) / 256), dim3(256), 0, st, A, (size_t)d + 1, d, order, eig_out);
        hipLaunchKernelGGL(gather_cols_kernel, dim3(dd_blocks), dim3(256), 0, st, V, order, T1, d);            // T1[k][i] = V[k][order[i]]
    }
    // P = eigvec^T P0 (eigenvectors = columns of T1, eigenvalues decreasing)
    gemm(st, mat(T1, d), mat(P0, d), p_out, d, d, d, 1.0);                                                      // P[i][j] = sum_k T1[k][i] P0[k][j]
    GDT_CHECK_HIP(hipGetLastError());
    GDT_CHECK_HIP(hipStreamSynchronize(st));
    if (info) { info[0] = jitter_steps; info[1] = c_failed ? -sweeps : sweeps; }      // negative: the two-sided fallback ran
    if (!converged) {          // the outputs are written (best effort), but the caller must not take them for an eigen-decomposition
        gdt_set_error("whiten_learn: the Jacobi eigensolver stopped at its sweep cap (" + std::to_string(sweeps) + " sweeps) without converging");
        return GDT_ERR_NOT_CONVERGED;
    }
    return GDT_OK;
}

int gdt_pca_whiten_learn_workspace_bytes(int n_vec, int d, size_t* bytes) {
    GDT_REQUIRE(bytes != nullptr, "bytes");
    PcaLayout L; int dp;
    int rc = pca_plan(n_vec, d, false, "pca_whiten_learn", L, dp);
    if (rc != GDT_OK) return rc;
    *bytes = L.total;
    return GDT_OK;
}

int gdt_pca_whiten_learn(const float* x, int n_vec, int d, int shrink, double* m_out, double* p_out, double* eig_out, int* info, void* workspace,
                         size_t workspace_bytes, void* stream_) {
    PcaLayout L; int dp;
    int rc = pca_plan(n_vec, d, false, "pca_whiten_learn", L, dp);
    if (rc != GDT_OK) return rc;
    GDT_REQUIRE(shrink >= 0 && shrink <= d, "pca_whiten_learn: shrink must be 0 (none) or 1..d");
    GDT_REQUIRE(x && m_out && p_out && workspace, "pca_whiten_learn: null buffer");
    if (workspace_bytes < L.total) { gdt_set_error("pca_whiten_learn: workspace too small"); return GDT_ERR_WORKSPACE; }
    hipStream_t st = (hipStream_t)stream_;
    char* ws = (char*)(((uintptr_t)workspace + ALIGN - 1) / ALIGN * ALIGN);
    double *C = (double*)(ws + L.c), *part = (double*)(ws + L.part), *lamp = (double*)(ws + L.lamp);
    const EigBuffers w = eig_buffers(ws, L);

    // m = mean over ALL vectors; C = sum (x - m)(x - m)^T / n: the tiles on and below the diagonal, mirrored
    hipLaunchKernelGGL(mean_all_partial_kernel, dim3((d + 255) / 256, MEAN_PARTS), dim3(256), 0, st, x, n_vec, d, part);
    hipLaunchKernelGGL(mean_all_finish_kernel, dim3((d + 255) / 256), dim3(256), 0, st, part, n_vec, d, m_out);
    Operand ce = {}; ce.kind = SRC_CENT; ce.x = x; ce.xd = d; ce.mean = m_out;
    gemm_lower(st, ce, C, d, n_vec, 1.0 / (double)n_vec);

    double* rows = nullptr;
    int sweeps = 0;
    bool one_sided = false, converged = false;
    rc = sym_eig(st, C, d, false, w, &rows, sweeps, one_sided, converged);
    if (rc != GDT_OK) return rc;
    if (eig_out) GDT_CHECK_HIP(hipMemcpyAsync(eig_out, w.eig, (size_t)d * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (info) info[0] = one_sided ? sweeps : -sweeps;                               // negative: the two-sided form ran
    if (!converged) { GDT_CHECK_HIP(hipStreamSynchronize(st)); return not_converged("pca_whiten_learn", sweeps); }

    // shrinkage, the positive-definiteness test on the (shrunk) eigenvalues, P[i] = v_i^T / sqrt(lambda'_i)
    hipLaunchKernelGGL(pca_shrink_kernel, dim3(1), dim3(1), 0, st, w.eig, d, shrink, lamp, w.flag, w.red);
    int bad = -1;
    double bad_value = 0.0;
    GDT_CHECK_HIP(hipMemcpyAsync(&bad, w.flag, sizeof(int), hipMemcpyDeviceToHost, st));
    GDT_CHECK_HIP(hipMemcpyAsync(&bad_value, w.red, sizeof(double), hipMemcpyDeviceToHost, st));
    GDT_CHECK_HIP(hipStreamSynchronize(st));
    if (bad >= 0) {
        char value[64];
        snprintf(value, sizeof(value), "%.6g", bad_value);
        gdt_set_error("pca_whiten_learn: the covariance is numerically not positive definite: eigenvalue " + std::to_string(bad) + " of " +
                      std::to_string(d) + (shrink ? " (after shrinkage) is " : " is ") + value +
                      ", not above d * 2^-52 times the largest; its whitening row would be infinite or NaN -- pass shrink (1..d) to regularise");
        return GDT_ERR_INVALID;
    }
    hipLaunchKernelGGL(pca_scale_rows_kernel, dim3(d), dim3(256), 0, st, rows, lamp, p_out, d);
    GDT_CHECK_HIP(hipGetLastError());
    GDT_CHECK_HIP(hipStreamSynchronize(st));
    return GDT_OK;
}

int gdt_pca_project_normalize_workspace_bytes(int n, int d, size_t* bytes) {
    GDT_REQUIRE(bytes != nullptr, "bytes");
    PcaLayout L; int dp;
    int rc = pca_plan(n, d, true, "pca_project_normalize", L, dp);
    if (rc != GDT_OK) return rc;
    *bytes = L.total;
    return GDT_OK;
}

int gdt_pca_project_normalize(const double* v, int n, int d, int dims, double* out, int* info, void* workspace, size_t workspace_bytes, void* stream_) {
    PcaLayout L; int dp;
    int rc = pca_plan(n, d, true, "pca_project_normalize", L, dp);
    if (rc != GDT_OK) return rc;
    GDT_REQUIRE(dims >= 1 && dims <= d, "pca_project_normalize: dims must be 1..d");
    GDT_REQUIRE(v && out && workspace, "pca_project_normalize: null buffer");
    if (workspace_bytes < L.total) { gdt_set_error("pca_project_normalize: workspace too small"); return GDT_ERR_WORKSPACE; }
    hipStream_t st = (hipStream_t)stream_;
    char* ws = (char*)(((uintptr_t)workspace + ALIGN - 1) / ALIGN * ALIGN);
    double *C = (double*)(ws + L.c), *M2 = (double*)(ws + L.m2), *part = (double*)(ws + L.part), *mean = (double*)(ws + L.lamp);
    const EigBuffers w = eig_buffers(ws, L);

    // the scalar mean of all entries; Gram matrix of the centred rows (dp x dp: an odd width gets one zero column)
    const size_t count = (size_t)n * d;
    hipLaunchKernelGGL(sum_partial_kernel, dim3(SUM_BLOCKS), dim3(256), 0, st, v, count, part);
    hipLaunchKernelGGL(sum_finish_kernel, dim3(1), dim3(256), 0, st, part, count, mean);
    Operand ce = {}; ce.kind = SRC_DCENT; ce.mat = v; ce.ld = d; ce.xd = d; ce.mean = mean;
    gemm_lower(st, ce, C, dp, n, 1.0);

    double* rows = nullptr;
    int sweeps = 0;
    bool one_sided = false, converged = false;
    rc = sym_eig(st, C, dp, dp != d, w, &rows, sweeps, one_sided, converged);
    if (rc != GDT_OK) return rc;
    if (info) info[0] = one_sided ? sweeps : -sweeps;
    if (!converged) { GDT_CHECK_HIP(hipStreamSynchronize(st)); return not_converged("pca_project_normalize", sweeps); }

    // M = V_k V_k^T from the dims leading eigenvector rows; out = (v - mean) M; rows to unit length
    gemm_lower(st, mat(rows, dp), M2, dp, dims, 1.0);
    Operand vr = {}; vr.kind = SRC_DROWS; vr.mat = v; vr.ld = d; vr.xd = d; vr.mean = mean;
    hipLaunchKernelGGL(gemm_rows_kernel, dim3((d + 63) / 64, (n + 63) / 64), dim3(256), 0, st, vr, mat(M2, dp), out, n, d, dp, d);
    hipLaunchKernelGGL(l2n_rows_f64_kernel, dim3(n), dim3(256), 0, st, out, out, d);
    GDT_CHECK_HIP(hipGetLastError());
    GDT_CHECK_HIP(hipStreamSynchronize(st));
    return GDT_OK;
}

int gdt_l2n_rows_f64(const double* v, double* out, int n, int d, void* stream_) {
    GDT_REQUIRE(n >= 0 && d >= 1, "l2n_rows_f64: n >= 0 and d >= 1");
    if (n == 0) return GDT_OK;
    GDT_REQUIRE(v && out, "l2n_rows_f64: null buffer");
    hipLaunchKernelGGL(l2n_rows_f64_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream_, v, out, d);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

// measurement aid: the covariance product of gdt_pca_whiten_learn on its own, as the lower-tile launch or as the full grid gdt_whiten_learn uses
int gdt_pca_covariance(const float* x, int n_vec, int d, const double* mean, double* c, int lower, void* stream_) {
    GDT_REQUIRE(n_vec >= 1 && d >= 1 && d <= 8192, "pca_covariance: n_vec >= 1 and d in 1..8192");
    GDT_REQUIRE(x && mean && c, "pca_covariance: null buffer");
    hipStream_t st = (hipStream_t)stream_;
    Operand ce = {}; ce.kind = SRC_CENT; ce.x = x; ce.xd = d; ce.mean = mean;
    if (lower) gemm_lower(st, ce, c, d, n_vec, 1.0 / (double)n_vec);
    else gemm(st, ce, ce, c, d, d, n_vec, 1.0 / (double)n_vec);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

}  // extern "C"
