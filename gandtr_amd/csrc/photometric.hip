// Photometric normalisation of the lightness channel on the device: histogram equalisation / matching and gamma equalisation, the training targets and
// classical baselines of the normalisation U-Nets.  The reference runs them per image through numpy and cv2:
//   channel_histogram_matching          mdir/components/data/transform/functional.py:96-101   (np.histogram, np.cumsum, two np.interp)
//   channel2channel_histogram_matching  functional.py:106-109
//   channel_gamma_matching              functional.py:116-130  (scipy.optimize.newton without fprime = the secant iteration, a full-image np.power per step)
//   image_histogram_matching / image_gamma_matching   functional.py:103-104 / :132-133  (apply_lightness_transform :81-85, "lab": :28-36 / :55-63)
//   MatchHistogram, ReplaceChannelWithHistogram, GammaEqualize   photometric_transforms.py:56-104
//   ToColorspace, AddIntensityFromRgb   channel_transforms.py:67-89;   AddClaheFromRgb   photometric_transforms.py:10-25
// The histogram has np.histogram's semantics exactly (257 float64 edges, the value compared as a double, last bin closed, values outside dropped) and the
// tables np.interp's (float64, separately rounded slope / multiply / add, the last knot of an equal run); edges and centres are computed ONCE by the host with
// numpy and handed in as `grid` (257 edges then 256 centres, device doubles), never re-derived here.
// Histogram matching of an image batch, three launches (+ one memset):
//   1. photo_hist_kernel:      RGB -> L / 100 (lab_device.h, the one statement of the lightness), binned into four wave-private LDS histograms (integer atomics:
//                              order-independent), merged into the image's 256 global counters.  Four pixels per lane, 16-byte loads.
//   2. photo_table_kernel:     one wave per image: integer scan, cdf = cumsum / size, table = cdf * centres[255] ("eq") or interp(cdf, target cdf, centres).
//   3. photo_apply_lab_kernel: RGB -> Lab with L RECOMPUTED through the same device function (no L plane is stored), L mapped through interp(L, centres, table),
//                              Lab -> RGB, output affine; four pixels per lane, 16-byte loads / stores, a scalar form when the plane is no multiple of 4.
// Algorithmic bytes per pixel: 12 (read RGB) in pass 1, 12 + 12 in pass 3 = 36 B.
// Gamma equalisation: pass 1 writes the fp32 L plane instead (4 B / pixel), photo_gamma_kernel solves mean(L^gamma) = target per image, pass 3 applies L^gamma.
//   The solve is ONE launch with ONE workgroup of 1024 lanes per image: every function evaluation walks the image's L plane (L2-resident at the sizes in use) and
//   sums L^gamma (float64, exp(gamma * log L): pow_sum below) in an order fixed by h * w alone (lane-sequential partial sums, a butterfly per wave, the 16 wave sums in index order; no
//   float atomics), so an image's gamma does not depend on its batch or on the run.  With few images this leaves most of the chip idle -- accepted: a batch of
//   training crops has one workgroup per CU or more, and splitting an image over workgroups would need a grid-wide hand-off per evaluation.
#include <string.h>

#include "../../include/gandtr_hip.h"
#include "gdt_common.h"
#include "lab_device.h"

// np.interp evaluates slope * (x - xp[j]) + fp[j] in separately rounded float64 steps
#pragma clang fp contract(off)

namespace {

// np.interp's value at x for the knot index j = the largest index with xp[j] <= x (xp[0] <= x <= xp[255] is the caller's business)
__device__ __forceinline__ double interp_at(double x, int j, const double* xp, const double* fp) {
    if (j >= 255) return fp[255];
    if (xp[j] == x) return fp[j];
    const double slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]);
    return slope * (x - xp[j]) + fp[j];
}

#pragma clang fp contract(fast)

constexpr int EDGES = 257, BINS = 256;

// np.histogram(chan, edges): the bin of v, or -1 when it lies outside [edges[0], edges[256]] (NaN too).  The guess is corrected against the edges themselves.
__device__ __forceinline__ int hist_bin(float v, const double* e) {
    const double d = (double)v;
    if (!(d >= e[0] && d <= e[BINS])) return -1;
    int k = min(max((int)floor(d * 255.0 + 0.5), 0), BINS - 1);
    while (k > 0 && d < e[k]) --k;
    while (k < BINS - 1 && d >= e[k + 1]) ++k;
    return k;
}

// np.interp(v, centres, table) in float64, rounded to float32 once
__device__ __forceinline__ float map_value(float v, const double* cen, const double* tab) {
    const double d = (double)v;
    if (d != d) return v;
    if (d < cen[0]) return (float)tab[0];
    if (d > cen[BINS - 1]) return (float)tab[BINS - 1];
    int j = min(max((int)(d * 255.0), 0), BINS - 1);
    while (j > 0 && d < cen[j]) --j;
    while (j < BINS - 1 && d >= cen[j + 1]) ++j;
    return (float)interp_at(d, j, cen, tab);
}

// Pass 1.  RGB: x = [n][3][plane] images and the value is their normalised lightness; else x = [n][plane] planes.  HIST: count into hist [n][256];
// WRITE_L: store the lightness to lplane [n][plane].  VEC = 4 needs plane % 4 == 0 and 16-byte aligned buffers.  blockIdx.y = image.
template <bool RGB, bool HIST, bool WRITE_L, int VEC>
__global__ __launch_bounds__(256) void photo_hist_kernel(const float* __restrict__ x, LabParams p, unsigned plane, const double* __restrict__ grid,
                                                         float* __restrict__ lplane, unsigned* __restrict__ hist) {
    __shared__ unsigned sh[4][BINS];
    __shared__ double edges[EDGES];
    const int tid = threadIdx.x, wave = tid >> 6;
    if (HIST) {
#pragma unroll
        for (int k = 0; k < 4; ++k) sh[k][tid] = 0;
        for (int k = tid; k < EDGES; k += 256) edges[k] = grid[k];
        __syncthreads();
    }
    const float* px = x + (size_t)blockIdx.y * (RGB ? 3 : 1) * plane;
    float* pl = lplane + (size_t)blockIdx.y * plane;
    const unsigned nq = plane / VEC;
    for (unsigned q = blockIdx.x * 256u + tid; q < nq; q += gridDim.x * 256u) {
        const unsigned pix = q * VEC;
        float c[3][VEC], v[VEC];
        if (VEC == 4) {
#pragma unroll
            for (int ch = 0; ch < (RGB ? 3 : 1); ++ch) *(f32x4*)c[ch] = *(const f32x4*)(px + (pix + ch * plane));
        } else {
#pragma unroll
            for (int ch = 0; ch < (RGB ? 3 : 1); ++ch) c[ch][0] = px[pix + ch * plane];
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            v[k] = RGB ? lab_lightness_norm(c[0][k], c[1][k], c[2][k], p) : c[0][k];
            if (HIST) {
                const int bin = hist_bin(v[k], edges);
                if (bin >= 0) atomicAdd(&sh[wave][bin], 1u);
            }
        }
        if (WRITE_L) {
            if (VEC == 4) *(f32x4*)(pl + pix) = *(f32x4*)v;
            else pl[pix] = v[0];
        }
    }
    if (HIST) {
        __syncthreads();
        const unsigned s = sh[0][tid] + sh[1][tid] + sh[2][tid] + sh[3][tid];
        if (s) atomicAdd(&hist[(size_t)blockIdx.y * BINS + tid], s);
    }
}

// full normalised Lab: (L / 100, (a + 128) / 255, (b + 128) / 255), functional.py:35
template <int VEC>
__global__ __launch_bounds__(256) void photo_rgb2lab_kernel(const float* __restrict__ x, LabParams p, unsigned plane, float* __restrict__ out) {
    const unsigned q = blockIdx.x * 256u + threadIdx.x;
    if (q >= plane / VEC) return;
    const unsigned pix = q * VEC;
    const float* px = x + (size_t)blockIdx.y * 3 * plane;
    float* po = out + (size_t)blockIdx.y * 3 * plane;
    float c[3][VEC];
    if (VEC == 4) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) *(f32x4*)c[ch] = *(const f32x4*)(px + (pix + ch * plane));
    } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch][0] = px[pix + ch * plane];
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const float px3[3] = {c[0][k], c[1][k], c[2][k]};
        float a500, b200;
        lab_chroma(px3, p, a500, b200);
        c[0][k] = lab_lightness_norm(px3[0], px3[1], px3[2], p);
        c[1][k] = (500.0f * a500 + 128.0f) * (1.0f / 255.0f);
        c[2][k] = (200.0f * b200 + 128.0f) * (1.0f / 255.0f);
    }
    if (VEC == 4) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) *(f32x4*)(po + (pix + ch * plane)) = *(f32x4*)c[ch];
    } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) po[pix + ch * plane] = c[ch][0];
    }
}

enum { MODE_EQ = 0, MODE_TARGET = 1, MODE_PLANE = 2 };

// inclusive integer scan of a wave's 256 counters (lane l owns bins 4 l .. 4 l + 3) -> cdf [256] = cumsum / size, as np.cumsum(hist) / chan.size
__device__ __forceinline__ void cdf_of(const unsigned* __restrict__ hist, double size, double* cdf) {
    const int lane = threadIdx.x;
    const uint4 hv = *(const uint4*)(hist + 4 * lane);
    long long c[4] = {(long long)hv.x, (long long)hv.x + hv.y, (long long)hv.x + hv.y + hv.z, (long long)hv.x + hv.y + hv.z + hv.w};
    long long run = c[3];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const long long t = __shfl_up(run, m);
        if (lane >= m) run += t;
    }
    const long long base = run - c[3];
#pragma unroll
    for (int j = 0; j < 4; ++j) cdf[4 * lane + j] = (double)(base + c[j]) / size;
}

// Pass 2: one wave per image.  hist1 / size1: the second plane's histogram (MODE_PLANE); target_cdf: 256 doubles (MODE_TARGET).
__global__ __launch_bounds__(64) void photo_table_kernel(const unsigned* __restrict__ hist0, double size0, const unsigned* __restrict__ hist1, double size1,
                                                         const double* __restrict__ target_cdf, int mode, const double* __restrict__ grid,
                                                         double* __restrict__ table) {
    __shared__ __attribute__((aligned(16))) double cdf0[BINS], xp[BINS], cen[BINS];
    const int lane = threadIdx.x;
    cdf_of(hist0 + (size_t)blockIdx.x * BINS, size0, cdf0);
    if (mode == MODE_PLANE) cdf_of(hist1 + (size_t)blockIdx.x * BINS, size1, xp);
    for (int k = lane; k < BINS; k += 64) {
        cen[k] = grid[EDGES + k];
        if (mode == MODE_TARGET) xp[k] = target_cdf[k];
    }
    __syncthreads();
    double* out = table + (size_t)blockIdx.x * BINS;
    for (int k = lane; k < BINS; k += 64) {
        const double v = cdf0[k];
        double r;
        if (mode == MODE_EQ) r = v * cen[BINS - 1];
        else if (v != v) r = v;
        else if (v < xp[0]) r = cen[0];
        else if (v > xp[BINS - 1]) r = cen[BINS - 1];
        else {
            int lo = 0, hi = BINS;                      // first index with v < xp[i]
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (v >= xp[mid]) lo = mid + 1;
                else hi = mid;
            }
            r = interp_at(v, lo - 1, xp, cen);
        }
        out[k] = r;
    }
}

// x^g for the sums of the solve: exp(g * log x) in float64, about 2.5 times cheaper than pow() and within |g ln x| * 2^-52 relative of it -- nine orders below
// the solve's tolerance; the two products 0 * inf that pow defines as 1 (x^0 and 1^g) are taken out by hand.  The OUTPUT pixels go through pow().
__device__ __forceinline__ double pow_sum(double x, double g) { return (x == 1.0 || g == 0.0) ? 1.0 : exp(g * log(x)); }

// The secant iteration of scipy.optimize.newton(func, x0, tol = 1e-4, maxiter = 50) without fprime, on func(g) = mean(L^g) - target, then the reference's
// fall-back and clip (functional.py:116-129).  One workgroup per image; every lane carries the same state.
__global__ __launch_bounds__(1024) void photo_gamma_kernel(const float* __restrict__ lplane, unsigned plane, double target, double* __restrict__ gamma_out,
                                                           int* __restrict__ evals_out) {
    __shared__ double part[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* lp = lplane + (size_t)blockIdx.x * plane;
    const bool vec = ((uintptr_t)lp % 16) == 0;
    const unsigned nq = (plane + 3) / 4;
    int evals = 0;
    // mean over the plane of L^g (power) or of L: quad q of the plane belongs to lane q % 1024, which adds its pixels in ascending order
    auto mean_of = [&](double g, bool power) -> double {
        double s = 0.0;
        for (unsigned q = tid; q < nq; q += 1024) {
            const unsigned pix = 4 * q, left = plane - pix;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (left >= 4 && vec) *(f32x4*)v = *(const f32x4*)(lp + pix);
            else
                for (unsigned k = 0; k < 4 && k < left; ++k) v[k] = lp[pix + k];
            for (unsigned k = 0; k < 4 && k < left; ++k) s += power ? pow_sum((double)v[k], g) : (double)v[k];
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
        __syncthreads();
        if (lane == 0) part[wave] = s;
        __syncthreads();
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < 16; ++w) t += part[w];
        ++evals;
        return t / (double)plane;
    };
    auto func = [&](double g) -> double { return mean_of(g, true) - target; };
    const double tol = 1e-4;
    auto close = [&](double a, double b) -> bool {          // np.isclose(a, b, rtol = 0, atol = tol)
        if (isfinite(a) && isfinite(b)) return fabs(a - b) <= tol;
        return a == b;
    };
    double p0 = log(target) / log(mean_of(0.0, false));
    double p1 = p0 * (1.0 + 1e-4);
    p1 += (p1 >= 0.0 ? 1e-4 : -1e-4);
    double q0 = func(p0), q1 = func(p1), sol = 0.0;
    if (fabs(q1) < fabs(q0)) {
        double t = p0; p0 = p1; p1 = t;
        t = q0; q0 = q1; q1 = t;
    }
    bool solved = false;
    for (int itr = 0; itr < 50; ++itr) {
        double p;
        if (q1 == q0) {
            if (p1 != p0) break;                            // "Tolerance reached": a RuntimeError in the reference
            sol = (p1 + p0) / 2.0;
            solved = true;
            break;
        }
        if (fabs(q1) > fabs(q0)) p = (-q0 / q1 * p1 + p0) / (1.0 - q0 / q1);
        else p = (-q1 / q0 * p0 + p1) / (1.0 - q1 / q0);
        if (close(p, p1)) { sol = p; solved = true; break; }
        if (p != p) break;                                  // a NaN iterate stays NaN to the last iteration
        p0 = p1; q0 = q1;
        p1 = p;
        q1 = func(p1);
    }
    if (!solved) sol = fabs(func(0.1)) < fabs(func(10.0)) ? 0.1 : 10.0;
    sol = fmin(fmax(sol, 0.1), 10.0);
    if (tid == 0) {
        gamma_out[blockIdx.x] = sol;
        if (evals_out) evals_out[blockIdx.x] = evals;
    }
}

// Pass 3, channel form: out = float32(interp(double(chan), centres, table)) or float32(pow(double(chan), gamma)); blockIdx.y = plane index
template <int VEC, bool GAMMA>
__global__ __launch_bounds__(256) void photo_apply_chan_kernel(const float* __restrict__ chan, float* __restrict__ out, unsigned plane,
                                                               const double* __restrict__ grid, const double* __restrict__ table,
                                                               const double* __restrict__ gamma) {
    __shared__ double cen[BINS], tab[BINS];
    double g = 0.0;
    if (GAMMA) g = gamma[blockIdx.y];
    else {
        cen[threadIdx.x] = grid[EDGES + threadIdx.x];
        tab[threadIdx.x] = table[(size_t)blockIdx.y * BINS + threadIdx.x];
        __syncthreads();
    }
    const unsigned q = blockIdx.x * 256u + threadIdx.x;
    if (q >= plane / VEC) return;
    const unsigned pix = q * VEC;
    const float* ps = chan + (size_t)blockIdx.y * plane;
    float* pd = out + (size_t)blockIdx.y * plane;
    float v[VEC];
    if (VEC == 4) *(f32x4*)v = *(const f32x4*)(ps + pix);
    else v[0] = ps[pix];
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = GAMMA ? (float)pow((double)v[k], g) : map_value(v[k], cen, tab);
    if (VEC == 4) *(f32x4*)(pd + pix) = *(f32x4*)v;
    else pd[pix] = v[0];
}

// Pass 3, image form: fp32 NCHW RGB in / out; L recomputed through lab_lightness_norm, so it equals the plane / histogram of pass 1 bit for bit
template <int VEC, bool GAMMA>
__global__ __launch_bounds__(256) void photo_apply_lab_kernel(const float* __restrict__ x, float* __restrict__ out, unsigned plane, LabParams p,
                                                              const double* __restrict__ grid, const double* __restrict__ table,
                                                              const double* __restrict__ gamma) {
    __shared__ double cen[BINS], tab[BINS];
    double g = 0.0;
    if (GAMMA) g = gamma[blockIdx.y];
    else {
        cen[threadIdx.x] = grid[EDGES + threadIdx.x];
        tab[threadIdx.x] = table[(size_t)blockIdx.y * BINS + threadIdx.x];
        __syncthreads();
    }
    const unsigned q = blockIdx.x * 256u + threadIdx.x;
    if (q >= plane / VEC) return;
    const unsigned pix = q * VEC;                                   // 3 * plane * 4 bytes < 2^32 (checked by the launcher)
    const float* px = x + (size_t)blockIdx.y * 3 * plane;
    float* po = out + (size_t)blockIdx.y * 3 * plane;
    float c[3][VEC];
    if (VEC == 4) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) *(f32x4*)c[ch] = *(const f32x4*)(px + (pix + ch * plane));
    } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch][0] = px[pix + ch * plane];
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const float px3[3] = {c[0][k], c[1][k], c[2][k]};
        float a500, b200, rgb[3];
        lab_chroma(px3, p, a500, b200);
        const float ln = lab_lightness_norm(px3[0], px3[1], px3[2], p);
        const float mapped = GAMMA ? (float)pow((double)ln, g) : map_value(ln, cen, tab);
        lab_to_rgb(mapped * 100.0f, a500, b200, p, rgb);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch][k] = rgb[ch];
    }
    if (VEC == 4) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) *(f32x4*)(po + (pix + ch * plane)) = *(f32x4*)c[ch];
    } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) po[pix + ch * plane] = c[ch][0];
    }
}

constexpr size_t ALIGN = 256;
inline size_t align_up(size_t v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }
inline char* aligned_base(void* ws) { return (char*)(((uintptr_t)ws + ALIGN - 1) / ALIGN * ALIGN); }

struct Layout { size_t hist0, hist1, table, lplane, total; };

int plan(int n, long count, Layout& L) {
    GDT_REQUIRE(n >= 1 && count >= 1, "photometric: needs a non-empty batch of planes");
    GDT_REQUIRE(count < (1l << 28) && n <= 65535, "photometric: at most 2^28 pixels per image and 65535 images per call");
    size_t off = 0;
    L.hist0 = off; off += align_up((size_t)n * BINS * sizeof(unsigned));
    L.hist1 = off; off += align_up((size_t)n * BINS * sizeof(unsigned));        // (directly behind hist0: one memset clears both)
    L.table = off; off += align_up((size_t)n * BINS * sizeof(double));
    L.lplane = off; off += align_up((size_t)n * count * sizeof(float));
    L.total = off + ALIGN;
    return GDT_OK;
}

inline bool aligned16(const void* a, const void* b = nullptr) { return (uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0; }
inline dim3 flat_grid(long count, int vec, int n) { return dim3((unsigned)((count / vec + 255) / 256), (unsigned)n); }
// pass 1: ~16 pixels per lane, at most 1024 workgroups per image (the kernel strides over the rest)
inline dim3 hist_grid(long count, int n) {
    const long g = (count + 4095) / 4096;
    return dim3((unsigned)(g < 1 ? 1 : (g > 1024 ? 1024 : g)), (unsigned)n);
}

template <bool RGB, bool HIST, bool WRITE_L>
void launch_hist(const float* x, const LabParams& p, int n, long count, const double* grid, float* lplane, unsigned* hist, hipStream_t stream) {
    const bool vec = count % 4 == 0 && aligned16(x, lplane);
    if (vec) hipLaunchKernelGGL((photo_hist_kernel<RGB, HIST, WRITE_L, 4>), hist_grid(count, n), dim3(256), 0, stream, x, p, (unsigned)count, grid, lplane, hist);
    else hipLaunchKernelGGL((photo_hist_kernel<RGB, HIST, WRITE_L, 1>), hist_grid(count, n), dim3(256), 0, stream, x, p, (unsigned)count, grid, lplane, hist);
}

template <bool GAMMA>
void launch_apply_lab(const float* x, float* y, const LabParams& p, int n, long count, const double* grid, const double* table, const double* gamma,
                      hipStream_t stream) {
    if (count % 4 == 0 && aligned16(x, y))
        hipLaunchKernelGGL((photo_apply_lab_kernel<4, GAMMA>), flat_grid(count, 4, n), dim3(256), 0, stream, x, y, (unsigned)count, p, grid, table, gamma);
    else hipLaunchKernelGGL((photo_apply_lab_kernel<1, GAMMA>), flat_grid(count, 1, n), dim3(256), 0, stream, x, y, (unsigned)count, p, grid, table, gamma);
}

template <bool GAMMA>
void launch_apply_chan(const float* x, float* y, int n, long count, const double* grid, const double* table, const double* gamma, hipStream_t stream) {
    if (count % 4 == 0 && aligned16(x, y))
        hipLaunchKernelGGL((photo_apply_chan_kernel<4, GAMMA>), flat_grid(count, 4, n), dim3(256), 0, stream, x, y, (unsigned)count, grid, table, gamma);
    else hipLaunchKernelGGL((photo_apply_chan_kernel<1, GAMMA>), flat_grid(count, 1, n), dim3(256), 0, stream, x, y, (unsigned)count, grid, table, gamma);
}

int check_mode(int mode, const void* target_cdf) {
    GDT_REQUIRE(mode == MODE_EQ || mode == MODE_TARGET || mode == MODE_PLANE, "photometric: mode is 0 (eq), 1 (target cdf) or 2 (second plane)");
    GDT_REQUIRE(mode != MODE_TARGET || target_cdf != nullptr, "photometric: mode 1 needs a target cdf");
    return GDT_OK;
}

int check_workspace(const Layout& L, const void* workspace, size_t workspace_bytes) {
    GDT_REQUIRE(workspace != nullptr, "photometric: null workspace");
    if (workspace_bytes < L.total) { gdt_set_error("photometric: workspace too small"); return GDT_ERR_WORKSPACE; }
    return GDT_OK;
}

}  // namespace

extern "C" {

int gdt_photometric_workspace_bytes(int n, int h, int w, size_t* bytes) {
    GDT_REQUIRE(bytes != nullptr, "bytes");
    GDT_REQUIRE(h >= 1 && w >= 1, "photometric: needs a non-empty batch of planes");
    Layout L;
    GDT_CHECK(plan(n, (long)h * w, L));
    *bytes = L.total;
    return GDT_OK;
}

int gdt_lab_lightness_f32(const float* x, float* lightness, int n, int h, int w, const float* in_scale, const float* in_shift, void* stream_) {
    Layout L;
    GDT_REQUIRE(h >= 1 && w >= 1, "photometric: needs a non-empty batch of planes");
    GDT_CHECK(plan(n, (long)h * w, L));
    GDT_REQUIRE(x != nullptr && lightness != nullptr, "photometric: null buffer");
    LabParams p;
    lab_fill_affines(p, in_scale, in_shift, nullptr, nullptr);
    launch_hist<true, false, true>(x, p, n, (long)h * w, nullptr, lightness, nullptr, (hipStream_t)stream_);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

int gdt_rgb2lab_f32(const float* x, float* lab, int n, int h, int w, const float* in_scale, const float* in_shift, void* stream_) {
    Layout L;
    GDT_REQUIRE(h >= 1 && w >= 1, "photometric: needs a non-empty batch of planes");
    const long count = (long)h * w;
    GDT_CHECK(plan(n, count, L));
    GDT_REQUIRE(x != nullptr && lab != nullptr, "photometric: null buffer");
    LabParams p;
    lab_fill_affines(p, in_scale, in_shift, nullptr, nullptr);
    hipStream_t stream = (hipStream_t)stream_;
    if (count % 4 == 0 && aligned16(x, lab)) hipLaunchKernelGGL(photo_rgb2lab_kernel<4>, flat_grid(count, 4, n), dim3(256), 0, stream, x, p, (unsigned)count, lab);
    else hipLaunchKernelGGL(photo_rgb2lab_kernel<1>, flat_grid(count, 1, n), dim3(256), 0, stream, x, p, (unsigned)count, lab);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

int gdt_hist256_f32(const float* chan, int n, long count, const double* grid, unsigned* hist, void* stream_) {
    Layout L;
    GDT_CHECK(plan(n, count, L));
    GDT_REQUIRE(chan != nullptr && grid != nullptr && hist != nullptr, "photometric: null buffer");
    hipStream_t stream = (hipStream_t)stream_;
    GDT_CHECK_HIP(hipMemsetAsync(hist, 0, (size_t)n * BINS * sizeof(unsigned), stream));
    LabParams p = {};
    launch_hist<false, true, false>(chan, p, n, count, grid, nullptr, hist, stream);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

int gdt_match_channel_f32(const float* chan, float* out, int n, long count, int mode, const double* target_cdf, const float* chan1, long count1,
                          const double* grid, void* workspace, size_t workspace_bytes, void* stream_) {
    Layout L, L1;
    GDT_CHECK(plan(n, count, L));
    GDT_CHECK(check_mode(mode, target_cdf));
    GDT_REQUIRE(mode != MODE_PLANE || chan1 != nullptr, "photometric: mode 2 needs a second plane");
    if (mode == MODE_PLANE) GDT_CHECK(plan(n, count1, L1));
    GDT_REQUIRE(chan != nullptr && out != nullptr && grid != nullptr, "photometric: null buffer");
    GDT_CHECK(check_workspace(L, workspace, workspace_bytes));
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = aligned_base(workspace);
    unsigned* hist0 = (unsigned*)(ws + L.hist0);
    unsigned* hist1 = (unsigned*)(ws + L.hist1);
    double* table = (double*)(ws + L.table);
    GDT_CHECK_HIP(hipMemsetAsync(hist0, 0, L.table - L.hist0, stream));
    LabParams p = {};
    launch_hist<false, true, false>(chan, p, n, count, grid, nullptr, hist0, stream);
    if (mode == MODE_PLANE) launch_hist<false, true, false>(chan1, p, n, count1, grid, nullptr, hist1, stream);
    hipLaunchKernelGGL(photo_table_kernel, dim3(n), dim3(64), 0, stream, hist0, (double)count, hist1, (double)count1, target_cdf, mode, grid, table);
    launch_apply_chan<false>(chan, out, n, count, grid, table, nullptr, stream);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

int gdt_match_histogram_lab_f32(const float* x, float* y, int n, int h, int w, const float* in_scale, const float* in_shift, const float* out_mean,
                                const float* out_std, int mode, const double* target_cdf, const double* grid, void* workspace, size_t workspace_bytes,
                                void* stream_) {
    Layout L;
    GDT_REQUIRE(h >= 1 && w >= 1, "photometric: needs a non-empty batch of planes");
    const long count = (long)h * w;
    GDT_CHECK(plan(n, count, L));
    GDT_CHECK(check_mode(mode, target_cdf));
    GDT_REQUIRE(mode != MODE_PLANE, "photometric: the image form matches to 'eq' or to a target cdf");
    GDT_REQUIRE(x != nullptr && y != nullptr && grid != nullptr, "photometric: null buffer");
    LabParams p;
    GDT_REQUIRE(lab_fill_affines(p, in_scale, in_shift, out_mean, out_std), "photometric: zero output std");
    GDT_CHECK(check_workspace(L, workspace, workspace_bytes));
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = aligned_base(workspace);
    unsigned* hist0 = (unsigned*)(ws + L.hist0);
    double* table = (double*)(ws + L.table);
    GDT_CHECK_HIP(hipMemsetAsync(hist0, 0, (size_t)n * BINS * sizeof(unsigned), stream));
    launch_hist<true, true, false>(x, p, n, count, grid, nullptr, hist0, stream);
    hipLaunchKernelGGL(photo_table_kernel, dim3(n), dim3(64), 0, stream, hist0, (double)count, (const unsigned*)nullptr, 1.0, target_cdf, mode, grid, table);
    launch_apply_lab<false>(x, y, p, n, count, grid, table, nullptr, stream);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

int gdt_gamma_channel_f32(const float* chan, float* out, int n, long count, double target, double* gamma, int* evaluations, void* stream_) {
    Layout L;
    GDT_CHECK(plan(n, count, L));
    GDT_REQUIRE(target > 0.0 && target < 1.0, "photometric: the gamma target lies strictly between 0 and 1");
    GDT_REQUIRE(chan != nullptr && out != nullptr && gamma != nullptr, "photometric: null buffer");
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(photo_gamma_kernel, dim3(n), dim3(1024), 0, stream, chan, (unsigned)count, target, gamma, evaluations);
    launch_apply_chan<true>(chan, out, n, count, nullptr, nullptr, gamma, stream);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

int gdt_gamma_equalize_lab_f32(const float* x, float* y, int n, int h, int w, const float* in_scale, const float* in_shift, const float* out_mean,
                               const float* out_std, double target, double* gamma, int* evaluations, void* workspace, size_t workspace_bytes,
                               void* stream_) {
    Layout L;
    GDT_REQUIRE(h >= 1 && w >= 1, "photometric: needs a non-empty batch of planes");
    const long count = (long)h * w;
    GDT_CHECK(plan(n, count, L));
    GDT_REQUIRE(target > 0.0 && target < 1.0, "photometric: the gamma target lies strictly between 0 and 1");
    GDT_REQUIRE(x != nullptr && y != nullptr && gamma != nullptr, "photometric: null buffer");
    LabParams p;
    GDT_REQUIRE(lab_fill_affines(p, in_scale, in_shift, out_mean, out_std), "photometric: zero output std");
    GDT_CHECK(check_workspace(L, workspace, workspace_bytes));
    hipStream_t stream = (hipStream_t)stream_;
    float* lplane = (float*)(aligned_base(workspace) + L.lplane);
    launch_hist<true, false, true>(x, p, n, count, nullptr, lplane, nullptr, stream);
    hipLaunchKernelGGL(photo_gamma_kernel, dim3(n), dim3(1024), 0, stream, (const float*)lplane, (unsigned)count, target, gamma, evaluations);
    launch_apply_lab<true>(x, y, p, n, count, nullptr, nullptr, gamma, stream);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

}  // extern "C"
