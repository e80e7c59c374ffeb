// L1 / MSE terms of the GAN scenarios' objectives over pairs of maps (gfx950, MI355X): mean |a - b| or mean (a - b)^2 per image, per pair and the weighted
// sum of a call's pairs -- what torch's L1Loss / MSELoss (base_losses.py:5-14) return inside MultiheadLoss (compound_losses.py:65-92), for up to 16 pairs in
// the same two launches.  b may be a constant (the target tensor of an adversarial MSE), and a sigmoid may be applied to both maps (the edge-consistency
// term from pre-sigmoid detector maps).
//
// Order of additions: an image is cut into chunks of ML_CHUNK values (chunks restart at every image); element e of a chunk belongs to lane (e / 4) % 256,
// which adds its elements in increasing e; the 256 lanes are merged by a fixed tree; that is the chunk's partial.  The finish adds an image's partials in
// index order, the images in index order, the pairs in index order.  All of it is a function of (count, n_images) alone: the partials kernel's grid only
// decides which workgroup evaluates a chunk.  Terms, sigmoid and sums in double; no atomics.  A chunk whose first element is 16-byte aligned in both maps
// is read with 16-byte loads, any other with 4-byte loads of the same elements by the same lanes: the bits do not depend on the alignment.
//
// The finish is one workgroup and each image's partials are added by ONE lane (that is what "in index order" costs): it is sized for the scenarios' pairs --
// 64 images of 24 chunks at 64 x 3 x 256^2 -- where it is a few microseconds.  A pair that is one very large image (n_images 1, count in the hundreds of
// millions: up to 2^30 / 8192 partials) makes it a long serial loop on one lane; the result is still right, and such a caller does better to pass the map as
// several images.  The lane's pair index selects its entry of the by-value table (kernel arguments, read through scalar loads per distinct index).
#include "gdt_common.h"
#include "../../include/gandtr_hip.h"

namespace {

constexpr int ML_THREADS = 256;
constexpr int ML_SLOTS = 8;                                   // 16-byte loads per lane and map, all issued before the first term: 64 KB in flight per workgroup
constexpr int ML_CHUNK = ML_THREADS * 4 * ML_SLOTS;           // 8192 values
constexpr int ML_MAX_GRID = 65536;

struct MlPair {
    const float* a; const float* b;
    long per_image;                                           // values per image
    double weight;
    float target;
    int kind, flags, n_images;
    int chunks_per_image, chunk_base, image_base;             // first chunk / first image of the pair among the call's
};
struct MlTable {
    int n_pairs, total_chunks, total_images;
    MlPair p[GDT_MAP_LOSS_MAX_PAIRS];
};
static_assert(sizeof(MlTable) <= 2048, "kernel arguments");

__device__ __forceinline__ double ml_sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }

__device__ __forceinline__ double ml_term(float a, float b, int kind, int sig, bool b_is_map) {
    double x = (double)a, y = (double)b;
    if (sig) {
        x = ml_sigmoid(x);
        if (b_is_map) y = ml_sigmoid(y);
    }
    const double d = x - y;
    return kind == 0 ? fabs(d) : __dmul_rn(d, d);                 // a rounded product: never contracted into the running sum
}

// partial[c] = sum of the terms of chunk c
__global__ __launch_bounds__(ML_THREADS) void map_loss_partial_kernel(const MlTable t, double* __restrict__ partial) {
    __shared__ double red[ML_THREADS];
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < t.total_chunks; c += gridDim.x) {
        int k = 0;
        while (k + 1 < t.n_pairs && c >= t.p[k + 1].chunk_base) ++k;
        const MlPair& p = t.p[k];
        const int local = c - p.chunk_base;
        const int img = local / p.chunks_per_image, ch = local - img * p.chunks_per_image;
        const long start = (long)img * p.per_image + (long)ch * ML_CHUNK;
        const long left = p.per_image - (long)ch * ML_CHUNK;
        const int len = left < ML_CHUNK ? (int)left : ML_CHUNK;
        const float* a = p.a + start;
        const float* b = p.b ? p.b + start : nullptr;
        const bool wide = (((uintptr_t)a | (uintptr_t)b) & 15) == 0;            // uniform over the workgroup
        float va[ML_SLOTS][4], vb[ML_SLOTS][4];
#pragma unroll
        for (int s = 0; s < ML_SLOTS; ++s) {
            const int e = (s * ML_THREADS + tid) * 4;
            if (wide && e + 4 <= len) {
                const float4 x = *reinterpret_cast<const float4*>(a + e);
                va[s][0] = x.x; va[s][1] = x.y; va[s][2] = x.z; va[s][3] = x.w;
                if (b) {
                    const float4 y = *reinterpret_cast<const float4*>(b + e);
                    vb[s][0] = y.x; vb[s][1] = y.y; vb[s][2] = y.z; vb[s][3] = y.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool in = e + j < len;
                    va[s][j] = in ? a[e + j] : 0.f;
                    vb[s][j] = in && b ? b[e + j] : 0.f;
                }
            }
        }
        const int sig = p.flags & 1;
        double acc = 0.0;
#pragma unroll
        for (int s = 0; s < ML_SLOTS; ++s) {
            const int e = (s * ML_THREADS + tid) * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double term = ml_term(va[s][j], b ? vb[s][j] : p.target, p.kind, sig, b != nullptr);
                acc += e + j < len ? term : 0.0;                               // terms are >= 0: adding +0 changes no bit
            }
        }
        red[tid] = acc;
        __syncthreads();
        for (int step = ML_THREADS / 2; step > 0; step >>= 1) {
            if (tid < step) red[tid] += red[tid + step];
            __syncthreads();
        }
        if (tid == 0) partial[c] = red[0];
        __syncthreads();
    }
}

// one workgroup: image sums (a thread per image, its partials in index order), pair sums (a thread per pair, its images in index order), the total
__global__ __launch_bounds__(ML_THREADS) void map_loss_finish_kernel(const MlTable t, const double* __restrict__ partial, double* __restrict__ image_sum,
                                                                     double* __restrict__ per_image, double* __restrict__ per_pair, double* __restrict__ total) {
    __shared__ double pair_mean[GDT_MAP_LOSS_MAX_PAIRS];
    const int tid = threadIdx.x;
    for (int i = tid; i < t.total_images; i += ML_THREADS) {
        int k = 0;
        while (k + 1 < t.n_pairs && i >= t.p[k + 1].image_base) ++k;
        const MlPair& p = t.p[k];
        const double* src = partial + p.chunk_base + (long)(i - p.image_base) * p.chunks_per_image;
        double s = 0.0;
        for (int c = 0; c < p.chunks_per_image; ++c) s += src[c];
        image_sum[i] = s;
        per_image[i] = s / (double)p.per_image;
    }
    __syncthreads();
    if (tid < t.n_pairs) {
        const MlPair& p = t.p[tid];
        double s = 0.0;
        for (int i = 0; i < p.n_images; ++i) s += image_sum[p.image_base + i];
        pair_mean[tid] = s / ((double)p.per_image * (double)p.n_images);
        per_pair[tid] = pair_mean[tid];
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int k = 0; k < t.n_pairs; ++k) s += t.p[k].weight * pair_mean[k];
        total[0] = s;
    }
}

// argument checks and the chunk / image layout of a call; no HIP call
int ml_table(const gdt_map_loss_pair* pairs, int n_pairs, MlTable& t) {
    GDT_REQUIRE(pairs, "gdt_map_loss: null pair table");
    GDT_REQUIRE(n_pairs >= 1 && n_pairs <= GDT_MAP_LOSS_MAX_PAIRS, "gdt_map_loss: 1 .. GDT_MAP_LOSS_MAX_PAIRS pairs");
    long chunks = 0, images = 0;
    for (int k = 0; k < n_pairs; ++k) {
        const gdt_map_loss_pair& s = pairs[k];
        GDT_REQUIRE(s.a, "gdt_map_loss: null map a");
        GDT_REQUIRE(s.count >= 1 && s.count < (1L << 40), "gdt_map_loss: count >= 1 values");
        GDT_REQUIRE(s.n_images >= 1 && s.n_images <= (1 << 20) && s.count % s.n_images == 0, "gdt_map_loss: count is n_images >= 1 maps of one size");
        GDT_REQUIRE(s.kind == 0 || s.kind == 1, "gdt_map_loss: kind 0 l1, 1 mse");
        GDT_REQUIRE((s.flags & ~1) == 0, "gdt_map_loss: flags bit 0 sigmoid, no other");
        GDT_REQUIRE(((uintptr_t)s.a & 3) == 0 && ((uintptr_t)s.b & 3) == 0, "gdt_map_loss: maps are 4-byte aligned");
        MlPair& p = t.p[k];
        p.a = s.a; p.b = s.b; p.target = s.target; p.kind = s.kind; p.flags = s.flags; p.n_images = s.n_images; p.weight = s.weight;
        p.per_image = s.count / s.n_images;
        const long cpi = (p.per_image + ML_CHUNK - 1) / ML_CHUNK;
        p.chunks_per_image = (int)cpi; p.chunk_base = (int)chunks; p.image_base = (int)images;
        chunks += cpi * s.n_images; images += s.n_images;
        GDT_REQUIRE(chunks < (1L << 30), "gdt_map_loss: too many values in one call");
    }
    t.n_pairs = n_pairs; t.total_chunks = (int)chunks; t.total_images = (int)images;
    return GDT_OK;
}

}  // namespace

extern "C" int gdt_map_loss_workspace_bytes(const gdt_map_loss_pair* pairs, int n_pairs, size_t* bytes) {
    GDT_REQUIRE(bytes, "gdt_map_loss_workspace_bytes: null output");
    MlTable t;
    GDT_CHECK(ml_table(pairs, n_pairs, t));
    *bytes = ((size_t)t.total_chunks + (size_t)t.total_images) * sizeof(double);
    return GDT_OK;
}

extern "C" int gdt_map_loss(const gdt_map_loss_pair* pairs, int n_pairs, double* per_image, double* per_pair, double* total, void* workspace,
                            size_t workspace_bytes, void* stream) {
    MlTable t;
    GDT_CHECK(ml_table(pairs, n_pairs, t));
    GDT_REQUIRE(per_image && per_pair && total, "gdt_map_loss: null output");
    GDT_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "gdt_map_loss: workspace is 8-byte aligned device memory");
    GDT_REQUIRE(workspace_bytes >= ((size_t)t.total_chunks + (size_t)t.total_images) * sizeof(double),
                "gdt_map_loss: workspace too small (gdt_map_loss_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    double* partial = (double*)workspace;
    const int grid = t.total_chunks < ML_MAX_GRID ? t.total_chunks : ML_MAX_GRID;
    hipLaunchKernelGGL(map_loss_partial_kernel, dim3(grid), dim3(ML_THREADS), 0, st, t, partial);
    GDT_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(map_loss_finish_kernel, dim3(1), dim3(ML_THREADS), 0, st, t, (const double*)partial, partial + t.total_chunks, per_image, per_pair, total);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}
