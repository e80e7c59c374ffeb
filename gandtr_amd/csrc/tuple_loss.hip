// Contrastive / triplet loss of retrieval tuples over an index table (include/gandtr_hip.h: gdt_tuple_loss).
//
// The reference scores one tuple per call (mdir/learning/validation.py:93-107 -> mdir/components/optim/criterion/cirlosses.py ->
// mdir/external/cirtorch/layers/functional.py:141-173): it gathers the anchor S - 1 times, subtracts, and reduces with about ten small torch ops.
// Here every tuple is a row of indices into ONE descriptor matrix [n_vec][d] and all tuples are scored by one launch:
//   tuple_loss_kernel   one workgroup per tuple, one wavefront per (anchor, other) pair (a wave takes pairs wave, wave + nw, ..).  Lane l sums the
//                       elements l, l + 64, .. (four at a time with 16-byte loads where d and the base address allow them) with fp32 FMAs, the 64
//                       partial sums are added by a fixed xor tree, lane 0 stores the pair's value.  The anchor row is fetched from memory once
//                       per tuple: the waves of a workgroup share the CU's vector cache.  After the barrier thread 0 adds the tuple's pair terms
//                       in index order.
//   tuple_total_kernel  one workgroup adds the tuple losses in double: thread t takes t, t + 256, .. in order, then a fixed LDS tree.
// Every sum has an order fixed by (d, s, n_tuples) alone -- no atomics, nothing depends on the grid or on which wave ran first -- so two calls give
// the same bits and a permuted table gives the permuted losses.  The kernel trusts the indices (the entry cannot see a device table; the binding
// checks a host table before it uploads it) and clamps nothing.
#include "../../include/gandtr_hip.h"
#include "gdt_common.h"

namespace {

constexpr int TL_MAX_WAVES = 8, TT_THREADS = 256;

// sum over the row of (a - b + eps)^2 held by this lane; the same order for every pair of a given d
template <bool VEC4>
__device__ inline float tl_lane_sum(const float* __restrict__ a, const float* __restrict__ b, int d, float eps, int lane) {
    float acc = 0.f;
    if (VEC4) {
#pragma unroll 4
        for (int i = lane * 4; i < d; i += 256) {
            const float4 x = *(const float4*)(a + i), y = *(const float4*)(b + i);
            const float t0 = x.x - y.x + eps, t1 = x.y - y.y + eps, t2 = x.z - y.z + eps, t3 = x.w - y.w + eps;
            acc = fmaf(t0, t0, acc);
            acc = fmaf(t1, t1, acc);
            acc = fmaf(t2, t2, acc);
            acc = fmaf(t3, t3, acc);
        }
    } else {
#pragma unroll 4
        for (int i = lane; i < d; i += 64) {
            const float t0 = a[i] - b[i] + eps;
            acc = fmaf(t0, t0, acc);
        }
    }
    return acc;
}

// KIND 0: contrastive -- value = D = sqrt(sum (a - b + eps)^2), term = 0.5 D^2 (pair 0, the positive) or 0.5 max(margin - D, 0)^2
// KIND 1: triplet     -- value = sum (a - b)^2; the tuple's loss is sum_j max(value[0] - value[j] + margin, 0) over the negatives j >= 1
template <bool VEC4, int KIND>
__global__ __launch_bounds__(TL_MAX_WAVES * 64) void tuple_loss_kernel(const float* __restrict__ vecs, const int* __restrict__ tuples, int d, int s,
                                                                      float margin, float eps, float* __restrict__ pair_dist,
                                                                      float* terms, float* __restrict__ tuple_loss) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6, np = s - 1;
    const size_t t = blockIdx.x;
    const int* row = tuples + t * s;
    const float* a = vecs + (size_t)row[0] * d;
    float* term = terms + t * np;
    for (int p = wave; p < np; p += nw) {
        const float* b = vecs + (size_t)row[p + 1] * d;
        float v = tl_lane_sum<VEC4>(a, b, d, KIND == 0 ? eps : 0.f, lane);
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
        if (lane == 0) {
            if (KIND == 0) {
                const float D = sqrtf(v), h = fmaxf(margin - D, 0.f);
                term[p] = p == 0 ? 0.5f * (D * D) : 0.5f * (h * h);
                if (pair_dist) pair_dist[t * np + p] = D;
            } else {
                term[p] = v;
                if (pair_dist) pair_dist[t * np + p] = v;
            }
        }
    }
    __syncthreads();                                       // the terms above are this workgroup's own global stores: visible after the barrier
    if (threadIdx.x == 0) {
        float sum = 0.f;
        if (KIND == 0) {
            for (int p = 0; p < np; ++p) sum += term[p];
        } else {
            const float dp = term[0];
            for (int p = 1; p < np; ++p) sum += fmaxf(dp - term[p] + margin, 0.f);
        }
        tuple_loss[t] = sum;
    }
}

__global__ __launch_bounds__(TT_THREADS) void tuple_total_kernel(const float* __restrict__ tuple_loss, int n, double* __restrict__ total) {
    __shared__ double part[TT_THREADS];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += TT_THREADS) acc += (double)tuple_loss[i];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int m = TT_THREADS / 2; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) part[threadIdx.x] += part[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = part[0];
}

int tl_check_sizes(int n_vec, int d, int n_tuples, int s) {
    GDT_REQUIRE(n_vec >= 1, "n_vec >= 1");
    GDT_REQUIRE(d >= 1, "d >= 1");
    GDT_REQUIRE(n_tuples >= 1, "n_tuples >= 1");
    GDT_REQUIRE(s >= 2, "s >= 2 (anchor and positive)");
    return GDT_OK;
}

}  // namespace

extern "C" {

int gdt_tuple_loss_workspace_bytes(int n_tuples, int s, size_t* bytes) {
    GDT_REQUIRE(bytes != nullptr, "bytes");
    GDT_CHECK(tl_check_sizes(1, 1, n_tuples, s));
    *bytes = (size_t)n_tuples * (size_t)(s - 1) * sizeof(float);
    return GDT_OK;
}

int gdt_tuple_loss(const float* vecs, const int* tuples, int n_vec, int d, int n_tuples, int s, int kind, float margin, float eps, float* pair_dist,
                   float* tuple_loss, double* total, void* workspace, size_t workspace_bytes, void* stream) {
    GDT_REQUIRE(vecs && tuples && tuple_loss && total && workspace, "null buffer");
    GDT_CHECK(tl_check_sizes(n_vec, d, n_tuples, s));
    GDT_REQUIRE(kind == 0 || kind == 1, "kind: 0 contrastive, 1 triplet");
    GDT_REQUIRE(margin == margin && eps == eps && eps >= 0.f, "margin and eps are numbers, eps >= 0");
    GDT_REQUIRE((uintptr_t)vecs % 4 == 0 && (uintptr_t)tuples % 4 == 0 && (uintptr_t)tuple_loss % 4 == 0 && (uintptr_t)workspace % 4 == 0 &&
                (uintptr_t)pair_dist % 4 == 0 && (uintptr_t)total % 8 == 0, "buffer alignment");
    GDT_REQUIRE(workspace_bytes >= (size_t)n_tuples * (size_t)(s - 1) * sizeof(float), "workspace too small (gdt_tuple_loss_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    const bool vec4 = d % 4 == 0 && (uintptr_t)vecs % 16 == 0;
    const int waves = s - 1 < TL_MAX_WAVES ? s - 1 : TL_MAX_WAVES;
    const dim3 grid((unsigned)n_tuples), block((unsigned)waves * 64);
    float* terms = (float*)workspace;
#define TL_LAUNCH(V, K) hipLaunchKernelGGL((tuple_loss_kernel<V, K>), grid, block, 0, st, vecs, tuples, d, s, margin, eps, pair_dist, terms, tuple_loss)
    if (kind == 0) {
        if (vec4) TL_LAUNCH(true, 0); else TL_LAUNCH(false, 0);
    } else {
        if (vec4) TL_LAUNCH(true, 1); else TL_LAUNCH(false, 1);
    }
#undef TL_LAUNCH
    GDT_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(tuple_total_kernel, dim3(1), dim3(TT_THREADS), 0, st, (const float*)tuple_loss, n_tuples, total);
    GDT_CHECK_HIP(hipGetLastError());
    return GDT_OK;
}

}  // extern "C"
