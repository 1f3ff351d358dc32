// k-means and cluster centroids on the device (engine.kmeans / kmeans_assign / cluster_centroids).
// The assignment step is engine.search's: the distance GEMM in column blocks of the centroids and grl_topk_block at
// k = 1.  This file is the other half of Lloyd's iteration: labels from the top-1 lists, the clusters' member lists
// as a CSR, the segmented row sum and the centroid finish.  Integer atomics count (cluster sizes, changed labels,
// empty clusters, slots of the member scatter); no floating-point atomic anywhere, and no output depends on the
// order in which the integer atomics land, so every result is the same bits on every run.
//
// Member lists.  counts -> grl_rrs_scan -> mptr [k+1]; every assigned sample takes a slot of its cluster's range by
// an integer atomic (arrival order), then one workgroup row per cluster moves every entry to "the number of the
// cluster's samples below it": a sample is in a cluster once, so that place depends on the set alone.
//
// Row sum (the hot path, normative order).  One 256-thread workgroup per (cluster, slab of 256 columns).  Wave w
// walks the members m_w, m_{w+4}, m_{w+8}, ..; every lane owns four columns of the slab (V = 4: one 16-byte load, a
// wave reads 1 KiB of a feature row; V = 1: four single floats 64 columns apart, each load of the wave a contiguous
// 256-byte run) and keeps a sequential fp32 sum from +0.0f.  The loads of four members are issued before the four
// dependent adds.  The four waves' partials meet in LDS: sum = (p0 + p1) + (p2 + p3).  Each assigned row is read
// once and k x d floats are written: the kernel is bound by HBM.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include "../../include/grl_hip.h"
#include "common.h"

namespace {

constexpr int KM_THREADS = 256;
constexpr int KM_WAVES = KM_THREADS / 64;
constexpr int KM_SLAB = 256;                   // columns of a workgroup: 64 lanes x 4
constexpr int KM_UNROLL = 4;                   // members in flight per wave
constexpr int KM_RANK_CHUNK = 1024;            // members of a cluster staged in LDS at a time
constexpr int KM_MAX_GROUPS = 4096;

// labels[i] = the index of the top-1 composite (-1: a NaN best distance, an empty slot, an index outside 0..k-1);
// counts[label] += 1; *changed += the labels that differ from prev (all of them without prev)
__global__ __launch_bounds__(KM_THREADS) void km_relabel_kernel(const uint64_t* __restrict__ run_key,
                                                                const float* __restrict__ run_val, int n, int k,
                                                                const int32_t* __restrict__ prev,
                                                                int32_t* __restrict__ labels,
                                                                int32_t* __restrict__ counts,
                                                                int32_t* __restrict__ changed) {
    int diff = 0;
    for (int i = blockIdx.x * KM_THREADS + threadIdx.x; i < n; i += gridDim.x * KM_THREADS) {
        const float v = run_val[i];
        const uint32_t idx = (uint32_t)(run_key[i] & 0xffffffffu);
        const int l = (v != v || idx >= (uint32_t)k) ? -1 : (int)idx;
        if (l >= 0) atomicAdd(counts + l, 1);
        diff += prev ? (prev[i] != l ? 1 : 0) : 1;
        labels[i] = l;
    }
    if (diff) atomicAdd(changed, diff);
}

__global__ __launch_bounds__(KM_THREADS) void km_count_kernel(const int32_t* __restrict__ labels, int n, int k,
                                                              int32_t* __restrict__ counts) {
    for (int i = blockIdx.x * KM_THREADS + threadIdx.x; i < n; i += gridDim.x * KM_THREADS) {
        const int l = labels[i];
        if ((unsigned)l < (unsigned)k) atomicAdd(counts + l, 1);
    }
}

// every assigned sample takes a slot of its cluster's range; the order inside a range is that of arrival
__global__ __launch_bounds__(KM_THREADS) void km_scatter_kernel(const int32_t* __restrict__ labels, int n, int k,
                                                                const int64_t* __restrict__ mptr,
                                                                int32_t* __restrict__ cursor,
                                                                int32_t* __restrict__ tmp) {
    for (int i = blockIdx.x * KM_THREADS + threadIdx.x; i < n; i += gridDim.x * KM_THREADS) {
        const int l = labels[i];
        if ((unsigned)l >= (unsigned)k) continue;
        const int64_t s = mptr[l], L = mptr[l + 1] - s;
        const int slot = atomicAdd(cursor + l, 1);
        if (slot < L && s + slot < n) tmp[s + slot] = i;    // (always: the counts come from the same labels)
    }
}

// blockIdx.x = the cluster, blockIdx.y strides over its entries 256 at a time: an entry's final place is the number
// of the cluster's members below it
__global__ __launch_bounds__(KM_THREADS) void km_order_kernel(const int64_t* __restrict__ mptr,
                                                              const int32_t* __restrict__ tmp, int n,
                                                              int32_t* __restrict__ mem) {
    __shared__ int rows[KM_RANK_CHUNK];
    const int64_t s = mptr[blockIdx.x];
    const int64_t L = min(mptr[blockIdx.x + 1], (int64_t)n) - s;
    const int tid = threadIdx.x;
    for (int64_t a0 = (int64_t)blockIdx.y * KM_THREADS; a0 < L; a0 += (int64_t)gridDim.y * KM_THREADS) {
        const int64_t a = a0 + tid;
        const int r = a < L ? tmp[s + a] : 0;
        int64_t below = 0;
        for (int64_t c0 = 0; c0 < L; c0 += KM_RANK_CHUNK) {
            const int m = (int)min((int64_t)KM_RANK_CHUNK, L - c0);
            __syncthreads();
            for (int t = tid; t < m; t += KM_THREADS) rows[t] = tmp[s + c0 + t];
            __syncthreads();
            if (a < L)
                for (int t = 0; t < m; ++t) below += rows[t] < r;
        }
        if (a < L) mem[s + below] = r;
    }
}

template <int V>
struct KmCols {                                 // a lane's four columns of one member row
    float v[4];
};

// the lane's four columns of row `m`; columns at or beyond d read as +0 (never stored)
template <int V>
__device__ __forceinline__ KmCols<V> km_load(const float* __restrict__ x, int64_t ld, int m, int c0, int lane, int d) {
    KmCols<V> r;
    const float* row = x + (int64_t)m * ld;
    if constexpr (V == 4) {
        const int c = c0 + 4 * lane;
        if (c < d) {                                             // d % 4 == 0: all four or none
            const f32x4 t = *reinterpret_cast<const f32x4*>(row + c);
            r.v[0] = t[0]; r.v[1] = t[1]; r.v[2] = t[2]; r.v[3] = t[3];
        } else {
            r.v[0] = r.v[1] = r.v[2] = r.v[3] = 0.f;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = c0 + lane + 64 * e;
            r.v[e] = c < d ? row[c] : 0.f;
        }
    }
    return r;
}

template <int V>
__global__ __launch_bounds__(KM_THREADS) void km_rowsum_kernel(const float* __restrict__ x, int64_t ld, int n,
                                                               const int64_t* __restrict__ mptr,
                                                               const int32_t* __restrict__ mem, int64_t nmem, int d,
                                                               float* __restrict__ sum, int64_t lds) {
    __shared__ float part[KM_WAVES][KM_SLAB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = blockIdx.x, c0 = blockIdx.y * KM_SLAB;
    const int64_t s = mptr[j], e = min(mptr[j + 1], nmem);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int64_t p = s + wave;
    for (; p + (KM_UNROLL - 1) * KM_WAVES < e; p += KM_UNROLL * KM_WAVES) {
        int m[KM_UNROLL];
#pragma unroll
        for (int u = 0; u < KM_UNROLL; ++u) {
            m[u] = mem[p + u * KM_WAVES];
            if ((unsigned)m[u] >= (unsigned)n) m[u] = -1;
        }
        KmCols<V> r[KM_UNROLL];
#pragma unroll
        for (int u = 0; u < KM_UNROLL; ++u)
            if (m[u] >= 0) r[u] = km_load<V>(x, ld, m[u], c0, lane, d);
#pragma unroll
        for (int u = 0; u < KM_UNROLL; ++u)
            if (m[u] >= 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] += r[u].v[q];
            }
    }
    for (; p < e; p += KM_WAVES) {
        const int m = mem[p];
        if ((unsigned)m >= (unsigned)n) continue;
        const KmCols<V> r = km_load<V>(x, ld, m, c0, lane, d);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += r.v[q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) part[wave][V == 4 ? 4 * lane + q : lane + 64 * q] = acc[q];
    __syncthreads();
    const int c = c0 + tid;
    if (c < d) sum[(int64_t)j * lds + c] = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
}

// out[j] = sum[j] ('sum'), sum[j] / count ('mean'), sum[j] * (1 / sqrt(sq[j])) ('unit'); an empty cluster (no
// member; 'unit': a norm that is zero or not finite) takes prev[j] or zeros and is counted in *empty
__global__ __launch_bounds__(KM_THREADS) void km_finish_kernel(const float* __restrict__ sum, int64_t lds,
                                                               const int32_t* __restrict__ counts,
                                                               const float* __restrict__ sq,
                                                               const float* __restrict__ prev, int64_t ldp, int d,
                                                               int reduce, float* __restrict__ out, int64_t ldo,
                                                               int32_t* __restrict__ empty) {
    const int j = blockIdx.x;
    const int cnt = counts[j];
    bool is_empty = cnt <= 0;
    float scale = 1.f;
    if (reduce == GRL_KMEANS_UNIT && !is_empty) {
        const float s = sq[j];
        if (!(s > 0.f) || isinf(s)) is_empty = true;             // zero, NaN or +inf
        else scale = 1.f / sqrtf(s);
    }
    const float fc = (float)cnt;
    for (int c = threadIdx.x; c < d; c += KM_THREADS) {
        float v;
        if (is_empty) v = prev ? prev[(int64_t)j * ldp + c] : 0.f;
        else {
            v = sum[(int64_t)j * lds + c];
            if (reduce == GRL_KMEANS_MEAN) v = v / fc;
            else if (reduce == GRL_KMEANS_UNIT) v = v * scale;
        }
        out[(int64_t)j * ldo + c] = v;
    }
    if (is_empty && threadIdx.x == 0) atomicAdd(empty, 1);
}

inline int km_groups(int n) { return min(max(grl_ceil_div(n, KM_THREADS), 1), KM_MAX_GROUPS); }

}  // namespace

extern "C" int grl_kmeans_relabel(const uint64_t* run_key, const float* run_val, int n, int k,
                                  const int32_t* prev_labels, int32_t* labels, int32_t* counts, int32_t* changed,
                                  void* stream) {
    GRL_REQUIRE(n >= 0 && k >= 1, "kmeans_relabel: n >= 0, k >= 1");
    GRL_REQUIRE(counts && changed, "kmeans_relabel: null");
    if (n == 0) return GRL_OK;
    GRL_REQUIRE(run_key && run_val && labels, "kmeans_relabel: null");
    hipLaunchKernelGGL(km_relabel_kernel, dim3(km_groups(n)), dim3(KM_THREADS), 0, (hipStream_t)stream, run_key,
                       run_val, n, k, prev_labels, labels, counts, changed);
    return grl_check_launch("grl_kmeans_relabel");
}

extern "C" int grl_kmeans_label_counts(const int32_t* labels, int n, int k, int32_t* counts, void* stream) {
    GRL_REQUIRE(n >= 0 && k >= 1, "kmeans_label_counts: n >= 0, k >= 1");
    GRL_REQUIRE(counts, "kmeans_label_counts: null");
    if (n == 0) return GRL_OK;
    GRL_REQUIRE(labels, "kmeans_label_counts: null");
    hipLaunchKernelGGL(km_count_kernel, dim3(km_groups(n)), dim3(KM_THREADS), 0, (hipStream_t)stream, labels, n, k,
                       counts);
    return grl_check_launch("grl_kmeans_label_counts");
}

extern "C" int grl_kmeans_members(const int32_t* labels, int n, int k, const int64_t* mptr, int32_t* cursor,
                                  int32_t* tmp, int32_t* mem, void* stream) {
    GRL_REQUIRE(n >= 0 && k >= 1, "kmeans_members: n >= 0, k >= 1");
    if (n == 0) return GRL_OK;
    GRL_REQUIRE(labels && mptr && cursor && tmp && mem, "kmeans_members: null");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(km_scatter_kernel, dim3(km_groups(n)), dim3(KM_THREADS), 0, st, labels, n, k, mptr, cursor, tmp);
    // the y blocks share a large cluster's entries; small clusters leave all but the first at once
    const int gy = max(1, min(grl_ceil_div(n, KM_THREADS), 8192 / k));
    hipLaunchKernelGGL(km_order_kernel, dim3(k, gy), dim3(KM_THREADS), 0, st, mptr, tmp, n, mem);
    return grl_check_launch("grl_kmeans_members");
}

extern "C" int grl_segment_rowsum(const float* x, int64_t ld, int n, const int64_t* mptr, const int32_t* mem,
                                  int64_t nmem, int k, int d, float* sum, int64_t lds, void* stream) {
    GRL_REQUIRE(n >= 0 && k >= 0 && d >= 1 && nmem >= 0 && nmem <= n, "segment_rowsum: bad shape");
    GRL_REQUIRE(ld >= d && lds >= d, "segment_rowsum: ld and lds must be >= d");
    if (k == 0) return GRL_OK;
    GRL_REQUIRE(mptr && sum && (n == 0 || x) && (nmem == 0 || mem), "segment_rowsum: null");
    const int slabs = grl_ceil_div(d, KM_SLAB);
    GRL_REQUIRE(slabs <= 65535, "segment_rowsum: d beyond 65535 slabs of 256 columns");
    const bool vec = aligned16(x) && (ld & 3) == 0 && (d & 3) == 0;
    const dim3 grid(k, slabs), block(KM_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(km_rowsum_kernel<4>, grid, block, 0, st, x, ld, n, mptr, mem, nmem, d, sum, lds);
    else hipLaunchKernelGGL(km_rowsum_kernel<1>, grid, block, 0, st, x, ld, n, mptr, mem, nmem, d, sum, lds);
    return grl_check_launch("grl_segment_rowsum");
}

extern "C" int grl_kmeans_finish(const float* sum, int64_t lds, const int32_t* counts, const float* sq,
                                 const float* prev, int64_t ldp, int k, int d, int reduce, float* out, int64_t ldo,
                                 int32_t* empty, void* stream) {
    GRL_REQUIRE(k >= 0 && d >= 1 && lds >= d && ldo >= d, "kmeans_finish: bad shape");
    GRL_REQUIRE(reduce == GRL_KMEANS_SUM || reduce == GRL_KMEANS_MEAN || reduce == GRL_KMEANS_UNIT,
                "kmeans_finish: reduce must be GRL_KMEANS_SUM, _MEAN or _UNIT");
    GRL_REQUIRE(empty, "kmeans_finish: null");
    if (k == 0) return GRL_OK;
    GRL_REQUIRE(sum && counts && out, "kmeans_finish: null");
    GRL_REQUIRE(reduce != GRL_KMEANS_UNIT || sq, "kmeans_finish: 'unit' needs the squared norms");
    GRL_REQUIRE(!prev || ldp >= d, "kmeans_finish: ldp must be >= d");
    hipLaunchKernelGGL(km_finish_kernel, dim3(k), dim3(KM_THREADS), 0, (hipStream_t)stream, sum, lds, counts, sq, prev,
                       ldp, d, reduce, out, ldo, empty);
    return grl_check_launch("grl_kmeans_finish");
}
