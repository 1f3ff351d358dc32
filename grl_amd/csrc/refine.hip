// Exact refinement of a shortlist against stored feature rows (engine.RefineStore / refine_dist / refine_lists /
// refine_search): the second stage behind pq_search / ivf_search.  For every query the distances to the
// R candidates of its list are recomputed from the rows of a feature store (fp32, or bf16 widened to fp32) and the list
// is re-sorted by them; the cost is a gather of nq * R rows, not a scan of the gallery.
//
// grl_refine_scan, the hot path.  A workgroup of 256 lanes owns one query and a slab of REFINE_SLAB consecutive list
// positions; the query row is staged once in LDS (d * 4 bytes).  Wave w takes the positions w, w + 4, .. of the slab,
// REFINE_ROWS candidates at a time: lane l owns the columns 256 t + 4 l + e of every row, one 16-byte load (fp32 store)
// or one 8-byte load (bf16 store) per 256 columns, so a wave-instruction covers 1 KiB / 512 contiguous bytes of a row,
// and the loads of REFINE_ROWS rows x 2 column chunks are issued before the first is consumed.  The summation
// order is the normative one of include/grl_hip.h (four sequential partials per lane, their join, common.h's
// wave_sum): it depends on d alone, so the same bits come out for every slab, batch and launch.  Products and sums are
// rounded one by one (no fma: -ffp-contract=off and the pragma below).  A padding entry (id < 0 or >= n) writes +inf / -1
// and never touches the store.  No atomics, plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include "../../include/grl_hip.h"
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int REFINE_THREADS = 256;
constexpr int REFINE_WAVES = REFINE_THREADS / 64;
#ifndef GRL_REFINE_SLAB
#define GRL_REFINE_SLAB 32                          // (a multiple of 4 * GRL_REFINE_ROWS; the result does not depend on either)
#endif
#ifndef GRL_REFINE_ROWS
#define GRL_REFINE_ROWS 4
#endif
constexpr int REFINE_SLAB = GRL_REFINE_SLAB;        // list positions per workgroup
constexpr int REFINE_ROWS = GRL_REFINE_ROWS;        // store rows in flight per wave
#ifndef GRL_REFINE_TU_BF16
#define GRL_REFINE_TU_BF16 2                        // (4 was measured slower: 120 VGPRs, one wave per SIMD fewer; EXPERIMENTS.md)
#endif
// column chunks of every row in flight: 2 x 16 bytes per lane and row from an fp32 store, 2 x 8 bytes from a bf16 store
template <typename T> struct RefineTu { static constexpr int value = 2; };
template <> struct RefineTu<uint16_t> { static constexpr int value = GRL_REFINE_TU_BF16; };
static_assert(REFINE_SLAB % (REFINE_WAVES * REFINE_ROWS) == 0, "a slab is whole batches of every wave");

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// the 4 columns of lane `lane` in chunk t of a store row, widened to fp32
__device__ __forceinline__ f32x4 load4(const float* __restrict__ row, int col) {
    return *reinterpret_cast<const f32x4*>(row + col);
}
__device__ __forceinline__ f32x4 load4(const uint16_t* __restrict__ row, int col) {
    const u32x2 v = *reinterpret_cast<const u32x2*>(row + col);
    return f32x4{__uint_as_float(v[0] << 16), __uint_as_float(v[0] & 0xffff0000u), __uint_as_float(v[1] << 16),
                 __uint_as_float(v[1] & 0xffff0000u)};
}

template <int METRIC>
__device__ __forceinline__ void accumulate(f32x4& a, const f32x4 q, const f32x4 x) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (METRIC == GRL_PQ_COSINE) {
            const float p = q[e] * x[e];
            a[e] = a[e] + p;
        } else {
            const float df = q[e] - x[e];
            const float p = df * df;
            a[e] = a[e] + p;
        }
    }
}

template <typename T, int METRIC>
__global__ __launch_bounds__(REFINE_THREADS) void refine_scan_kernel(const float* __restrict__ qf, int64_t ldq,
                                                                     const T* __restrict__ store, int64_t lds,
                                                                     const int64_t* __restrict__ cand, int64_t ldc,
                                                                     float* __restrict__ out, int32_t* __restrict__ cidx,
                                                                     int64_t ldo, int L, int64_t n, int d) {
    extern __shared__ __attribute__((aligned(16))) float s_q[];    // [d] the query row
    constexpr int REFINE_TU = RefineTu<T>::value;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.y;
    const int j0 = blockIdx.x * REFINE_SLAB;                       // < L by the grid
    const int64_t* __restrict__ crow = cand + (int64_t)q * ldc;
    float* __restrict__ orow = out + (int64_t)q * ldo;
    int32_t* __restrict__ irow = cidx + (int64_t)q * ldo;

    const float* __restrict__ qrow = qf + (int64_t)q * ldq;
    for (int c = tid * 4; c < d; c += REFINE_THREADS * 4)
        *reinterpret_cast<f32x4*>(s_q + c) = *reinterpret_cast<const f32x4*>(qrow + c);
    __syncthreads();

    const int full = d >> 8;                                       // chunks in which every lane has its 4 columns
    const int lc = 4 * lane;
    const bool tail = (full << 8) + lc < d;                        // this lane's part of the ragged last chunk (d % 4 == 0)

    for (int b = 0; b < REFINE_SLAB / (REFINE_WAVES * REFINE_ROWS); ++b) {
        const int jb = j0 + (b * REFINE_ROWS) * REFINE_WAVES + wave;   // this wave's positions jb, jb + 4, ..
        if (jb >= L) break;                                        // (wave-uniform)
        const T* row[REFINE_ROWS];
        int id[REFINE_ROWS];                                       // -1: padding, -2: beyond the list
        bool any = false;
#pragma unroll
        for (int u = 0; u < REFINE_ROWS; ++u) {
            const int j = jb + u * REFINE_WAVES;
            id[u] = -2;
            row[u] = store;
            if (j < L) {
                const int64_t g = crow[j];                         // one address per wave
                const bool ok = g >= 0 && g < n;
                id[u] = __builtin_amdgcn_readfirstlane(ok ? (int)g : -1);      // (n < 2^31)
                if (id[u] >= 0) { row[u] = store + (int64_t)id[u] * lds; any = true; }
            }
        }
        f32x4 acc[REFINE_ROWS];
#pragma unroll
        for (int u = 0; u < REFINE_ROWS; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};

        if (any) {
            int t = 0;
            for (; t + REFINE_TU <= full; t += REFINE_TU) {
                f32x4 x[REFINE_TU][REFINE_ROWS];
#pragma unroll
                for (int s = 0; s < REFINE_TU; ++s)
#pragma unroll
                    for (int u = 0; u < REFINE_ROWS; ++u)
                        x[s][u] = id[u] >= 0 ? load4(row[u], ((t + s) << 8) + lc) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < REFINE_TU; ++s) {
                    const f32x4 qv = *reinterpret_cast<const f32x4*>(s_q + ((t + s) << 8) + lc);
#pragma unroll
                    for (int u = 0; u < REFINE_ROWS; ++u) accumulate<METRIC>(acc[u], qv, x[s][u]);
                }
            }
            for (; t < full; ++t) {
                f32x4 x[REFINE_ROWS];
#pragma unroll
                for (int u = 0; u < REFINE_ROWS; ++u)
                    x[u] = id[u] >= 0 ? load4(row[u], (t << 8) + lc) : f32x4{0.f, 0.f, 0.f, 0.f};
                const f32x4 qv = *reinterpret_cast<const f32x4*>(s_q + (t << 8) + lc);
#pragma unroll
                for (int u = 0; u < REFINE_ROWS; ++u) accumulate<METRIC>(acc[u], qv, x[u]);
            }
            if (tail) {                                            // columns >= d are skipped
                f32x4 x[REFINE_ROWS];
#pragma unroll
                for (int u = 0; u < REFINE_ROWS; ++u)
                    x[u] = id[u] >= 0 ? load4(row[u], (full << 8) + lc) : f32x4{0.f, 0.f, 0.f, 0.f};
                const f32x4 qv = *reinterpret_cast<const f32x4*>(s_q + (full << 8) + lc);
#pragma unroll
                for (int u = 0; u < REFINE_ROWS; ++u) accumulate<METRIC>(acc[u], qv, x[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < REFINE_ROWS; ++u) {
            if (id[u] == -2) continue;                             // (wave-uniform)
            const int j = jb + u * REFINE_WAVES;
            if (id[u] < 0) {
                if (lane == 0) { orow[j] = INFINITY; irow[j] = -1; }
                continue;
            }
            const float v = (acc[u][0] + acc[u][1]) + (acc[u][2] + acc[u][3]);
            const float S = wave_sum(v);
            float dist;
            if (METRIC == GRL_PQ_COSINE) dist = -S;
            else dist = sqrtf(S > 1e-12f ? S : 1e-12f);            // (a NaN fails the comparison: 1e-12, as the EUCLID epilogue)
            if (dist != dist) dist = __int_as_float(0x7fc00000);
            if (lane == 0) { orow[j] = dist; irow[j] = id[u]; }
        }
    }
}

// round to nearest even; every NaN -> 0x7fc0; +-inf and +-0 keep their bits; a finite value above the bf16 range rounds to inf
__device__ __forceinline__ uint16_t pack_bf16(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)0x7fc0;
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// one lane per 8 elements (two 16-byte loads, one 16-byte store) when VECTOR, the ragged end element by element
template <bool VECTOR>
__global__ __launch_bounds__(256) void refine_pack_kernel(const float* __restrict__ x, uint16_t* __restrict__ out, int64_t count) {
    const int64_t groups = VECTOR ? count >> 3 : 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t g = first; g < groups; g += stride) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(x + 8 * g), b = *reinterpret_cast<const f32x4*>(x + 8 * g + 4);
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        u32x4 r;
        r[0] = (uint32_t)pack_bf16(a[0]) | ((uint32_t)pack_bf16(a[1]) << 16);
        r[1] = (uint32_t)pack_bf16(a[2]) | ((uint32_t)pack_bf16(a[3]) << 16);
        r[2] = (uint32_t)pack_bf16(b[0]) | ((uint32_t)pack_bf16(b[1]) << 16);
        r[3] = (uint32_t)pack_bf16(b[2]) | ((uint32_t)pack_bf16(b[3]) << 16);
        *reinterpret_cast<u32x4*>(out + 8 * g) = r;
    }
    for (int64_t i = 8 * groups + first; i < count; i += stride) out[i] = pack_bf16(x[i]);
}

template <typename T>
void refine_launch(int metric, dim3 grid, size_t lds_bytes, hipStream_t st, const float* q, int64_t ldq, const T* store,
                   int64_t lds, const int64_t* cand, int64_t ldc, float* out, int32_t* cidx, int64_t ldo, int L, int64_t n,
                   int d) {
    if (metric == GRL_PQ_COSINE)
        hipLaunchKernelGGL((refine_scan_kernel<T, GRL_PQ_COSINE>), grid, dim3(REFINE_THREADS), lds_bytes, st, q, ldq, store, lds,
                           cand, ldc, out, cidx, ldo, L, n, d);
    else
        hipLaunchKernelGGL((refine_scan_kernel<T, GRL_PQ_EUCLIDEAN>), grid, dim3(REFINE_THREADS), lds_bytes, st, q, ldq, store,
                           lds, cand, ldc, out, cidx, ldo, L, n, d);
}

}  // namespace

extern "C" int grl_refine_scan(const float* q, int64_t ldq, const void* store, int64_t lds, int store_type, const int64_t* cand,
                               int64_t ldc, float* out, int32_t* cidx, int64_t ldo, int nq, int L, int64_t n, int d, int metric,
                               void* stream) {
    GRL_REQUIRE(q && store && cand && out && cidx, "refine_scan: null");
    GRL_REQUIRE(nq >= 0 && L >= 0 && n >= 0 && n <= INT_MAX, "refine_scan: nq, L >= 0 and 0 <= n < 2^31");
    GRL_REQUIRE(d >= 1 && d <= GRL_REFINE_D_MAX && d % 4 == 0, "refine_scan: d must be a multiple of 4 in 1..GRL_REFINE_D_MAX");
    GRL_REQUIRE(store_type == GRL_REFINE_F32 || store_type == GRL_REFINE_BF16, "refine_scan: store_type is not one of GRL_REFINE_*");
    GRL_REQUIRE(metric == GRL_PQ_COSINE || metric == GRL_PQ_EUCLIDEAN, "refine_scan: metric is not one of GRL_PQ_*");
    GRL_REQUIRE(ldq >= d && lds >= d && ldc >= L && ldo >= L, "refine_scan: ldq >= d, lds >= d, ldc >= L and ldo >= L");
    GRL_REQUIRE(ldq % 4 == 0 && lds % 4 == 0, "refine_scan: ldq and lds must be multiples of 4");
    GRL_REQUIRE(nq <= 65535, "refine_scan: at most 65535 queries per call");
    GRL_REQUIRE(aligned16(q) && ((uintptr_t)store & (store_type == GRL_REFINE_F32 ? 15u : 7u)) == 0,
                "refine_scan: q and an fp32 store must be 16-byte aligned, a bf16 store 8-byte aligned");
    GRL_REQUIRE(((uintptr_t)cand & 7u) == 0 && ((uintptr_t)out & 3u) == 0 && ((uintptr_t)cidx & 3u) == 0,
                "refine_scan: cand must be 8-byte aligned, out and cidx 4-byte aligned");
    if (nq == 0 || L == 0) return GRL_OK;
    const dim3 grid((unsigned)((L + REFINE_SLAB - 1) / REFINE_SLAB), (unsigned)nq);
    const size_t lds_bytes = (size_t)d * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    if (store_type == GRL_REFINE_F32)
        refine_launch(metric, grid, lds_bytes, st, q, ldq, (const float*)store, lds, cand, ldc, out, cidx, ldo, L, n, d);
    else
        refine_launch(metric, grid, lds_bytes, st, q, ldq, (const uint16_t*)store, lds, cand, ldc, out, cidx, ldo, L, n, d);
    return grl_check_launch("grl_refine_scan");
}

extern "C" int grl_refine_pack_bf16(const float* x, uint16_t* out, int64_t count, void* stream) {
    GRL_REQUIRE(x && out, "refine_pack_bf16: null");
    GRL_REQUIRE(count >= 0, "refine_pack_bf16: count >= 0");
    GRL_REQUIRE(((uintptr_t)x & 3u) == 0 && ((uintptr_t)out & 1u) == 0,
                "refine_pack_bf16: x must be 4-byte aligned, out 2-byte aligned");
    if (count == 0) return GRL_OK;
    hipStream_t st = (hipStream_t)stream;
    if (aligned16(x) && aligned16(out))
        hipLaunchKernelGGL(refine_pack_kernel<true>, dim3(grid_for((count + 7) / 8)), dim3(256), 0, st, x, out, count);
    else
        hipLaunchKernelGGL(refine_pack_kernel<false>, dim3(grid_for(count)), dim3(256), 0, st, x, out, count);
    return grl_check_launch("grl_refine_pack_bf16");
}
