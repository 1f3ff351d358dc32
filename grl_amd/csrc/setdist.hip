// Set-to-set distances between tracklets from a block of the clip x clip distance matrix (engine.set_dist / set_search /
// set_metrics_streaming / set_pair_roc).  The scratch e [rows][ld] holds the clip distances of the query
// tracklets a0 .. a0 + na against the gallery tracklets b0 .. b0 + nb as the distance GEMM wrote them; the cell of the
// pair (a, b) is the m x p rectangle of a's clips (rows, ld apart) and b's clips (columns, contiguous), and this kernel
// folds every cell into one float: min, mean, chamfer or Hausdorff (include/grl_hip.h has the normative definitions).
//
// Mapping.  One wave per cell, cells in row-major order over the waves, so the four waves of a workgroup read
// neighbouring column ranges of the same scratch rows.  A wave covers W columns and R = 64 / W rows with one load: W = 64
// for p > 32, else the smallest power of two >= p -- a MARS tracklet has ~15 clips, and 16 x 4 fills the wave where 64 x 1
// would use 15 lanes.  lane = (i % R) * W + (j % 64).  A cell wider than 64 columns is walked in pieces of 64 columns,
// all rows of a piece before the next piece; every element is read once, four loads in flight per lane.
//
// min and max are exact selections, taken on an order-preserving integer image of the float (-0 below +0), so no
// summation order exists for them; a NaN is kept apart as a flag and makes the cell the canonical NaN.  rowmin[i]: log2 W
// xor-shuffles per load, carried across the 64-column pieces in LDS (1024 words per wave); colmin[j]: lane-local over
// the rows, joined across the R row groups by log2 R shuffles at the end of a piece, stored in LDS as well.  The two
// chamfer sums then run sequentially over those LDS arrays in ascending index, one lane each.  mean keeps one fp32
// partial per lane (its elements in ascending piece, then ascending row) and ends in the halving tree of
// grl_silhouette_block.  All of it depends on (m, p) alone: not on where the cell lies in the scratch, on the grid or on
// the other cells.  Adds only for the sums, no atomics of any kind.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include "../../include/grl_hip.h"
#include "common.h"

namespace {

constexpr int SD_THREADS = 256;
constexpr int SD_WAVES = SD_THREADS / 64;
constexpr int SD_MAX_CLIPS = GRL_SET_MAX_CLIPS;
constexpr int SD_UNROLL = 4;                       // loads in flight per lane
constexpr int SD_MAX_GRID = 1 << 20;               // workgroups; the cells beyond are reached by the grid stride

// order-preserving image of a float that is not NaN: a < b (with -0 < +0) <=> key(a) < key(b) as unsigned
__device__ __forceinline__ uint32_t sd_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sd_unkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
__device__ __forceinline__ float sd_canonical(float v) { return v != v ? __uint_as_float(0x7fc00000u) : v; }

// part[l] += part[l + s] for l < s, s = 32 .. 1 (grl_silhouette_block's tree); every lane receives part[0]
__device__ __forceinline__ float sd_tree(float v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s);      // (lanes >= s hold values nobody reads)
    return __shfl(v, 0);
}

// sequential fp32 sum from +0.0f of the n keyed values of s, in ascending index (reads batched, adds in order)
__device__ __forceinline__ float sd_seq_sum(const uint32_t* s, int n) {
    float acc = 0.f;
    int i = 0;
    for (; i + 8 <= n; i += 8) {
        uint32_t k[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) k[u] = s[i + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += sd_unkey(k[u]);
    }
    for (; i < n; ++i) acc += sd_unkey(s[i]);
    return acc;
}

template <int RED>
__global__ __launch_bounds__(SD_THREADS) void setdist_kernel(const float* __restrict__ e, int64_t ld,
                                                             const int64_t* __restrict__ qptr, int a0, int na,
                                                             const int64_t* __restrict__ gptr, int b0, int nb,
                                                             float* __restrict__ out, int64_t ldo) {
    constexpr bool MINS = RED == GRL_SET_CHAMFER || RED == GRL_SET_HAUSDORFF;
    __shared__ uint32_t s_row[MINS ? SD_WAVES : 1][MINS ? SD_MAX_CLIPS : 1];
    __shared__ uint32_t s_col[MINS ? SD_WAVES : 1][MINS ? SD_MAX_CLIPS : 1];
    const int lane = threadIdx.x & 63;
    // (the wave index is the same in all 64 lanes: everything derived from it stays in scalar registers)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t* __restrict__ srow = s_row[MINS ? wave : 0];
    uint32_t* __restrict__ scol = s_col[MINS ? wave : 0];
    const int64_t ncells = (int64_t)na * nb;
    const int64_t q0 = qptr[a0], g0 = gptr[b0];

    for (int64_t cell = (int64_t)blockIdx.x * SD_WAVES + wave; cell < ncells; cell += (int64_t)gridDim.x * SD_WAVES) {
        const int a = (int)(cell / nb), b = (int)(cell - (int64_t)a * nb);
        const int64_t qa = qptr[a0 + a], gb = gptr[b0 + b];
        const int m = (int)(qptr[a0 + a + 1] - qa), p = (int)(gptr[b0 + b + 1] - gb);     // 1 .. 1024 (checked on the host)
        int lw = 6;                                                // W = 1 << lw columns, R = 64 >> lw rows per load
        if (p <= 32) { lw = 0; while ((1 << lw) < p) ++lw; }
        const int W = 1 << lw, R = 64 >> lw;
        const int ri = lane >> lw, j0 = lane & (W - 1);
        const float* __restrict__ base = e + (qa - q0) * ld + (gb - g0);

        bool nan = false;
        uint32_t gmin = 0xffffffffu;                               // MIN
        float part = 0.f;                                          // MEAN: this lane's partial
        for (int cb = 0; cb < p; cb += 64) {
            const int j = cb + j0;
            const bool jv = j < p;
            uint32_t cmin = 0xffffffffu;
            for (int i0 = 0; i0 < m; i0 += SD_UNROLL * R) {
                float v[SD_UNROLL];
                bool ok[SD_UNROLL];
#pragma unroll
                for (int u = 0; u < SD_UNROLL; ++u) {
                    const int i = i0 + u * R + ri;
                    ok[u] = jv && i < m;
                    v[u] = 0.f;
                    if (ok[u]) v[u] = base[(int64_t)i * ld + j];
                }
#pragma unroll
                for (int u = 0; u < SD_UNROLL; ++u) {
                    if (RED == GRL_SET_MEAN) {
                        if (ok[u]) part += v[u];
                        continue;
                    }
                    const uint32_t k = ok[u] ? sd_key(v[u]) : 0xffffffffu;
                    nan = nan || (ok[u] && v[u] != v[u]);
                    if (RED == GRL_SET_MIN) { gmin = min(gmin, k); continue; }
                    if (i0 + u * R >= m) continue;                  // (uniform: no row of this load exists)
                    cmin = min(cmin, k);
                    uint32_t rk = k;
                    for (int s = W >> 1; s > 0; s >>= 1) rk = min(rk, (uint32_t)__shfl_xor((int)rk, s));
                    const int i = i0 + u * R + ri;
                    if (j0 == 0 && i < m) {
                        if (cb) rk = min(rk, srow[i]);               // (written by this same lane in the piece before)
                        srow[i] = rk;
                    }
                }
            }
            if (MINS) {
                for (int s = W; s < 64; s <<= 1) cmin = min(cmin, (uint32_t)__shfl_xor((int)cmin, s));
                if (ri == 0 && jv) scol[j] = cmin;
            }
        }

        float res;
        if (RED == GRL_SET_MIN) {
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) gmin = min(gmin, (uint32_t)__shfl_xor((int)gmin, s));
            res = sd_unkey(gmin);
        } else if (RED == GRL_SET_MEAN) {
            res = sd_tree(part) / (float)(m * p);
        } else {
            // srow / scol were written by other lanes of this wave: LDS operations of a wave complete in order
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (RED == GRL_SET_HAUSDORFF) {
                uint32_t mx = 0u;
                for (int i = lane; i < m; i += 64) mx = max(mx, srow[i]);
                for (int j = lane; j < p; j += 64) mx = max(mx, scol[j]);
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, s));
                res = sd_unkey(mx);
            } else {
                float sum = 0.f;                                     // lane 0: the rows' sum, lane 1: the columns', side by side
                if (lane < 2) sum = sd_seq_sum(lane == 0 ? srow : scol, lane == 0 ? m : p);
                const float sr = __shfl(sum, 0), sc = __shfl(sum, 1);
                res = 0.5f * (sr / (float)m + sc / (float)p);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the next cell of this wave overwrites both arrays
            __builtin_amdgcn_wave_barrier();
        }
        if (RED != GRL_SET_MEAN && __ballot(nan)) res = NAN;
        if (lane == 0) out[(int64_t)a * ldo + b] = sd_canonical(res);
    }
}

// the tracklets t0 .. t0 + nt of a host ptr array: every count >= 1 (which is also monotonic); the largest count
int sd_check_ptr(const int64_t* ptr, int t0, int nt, int64_t* longest) {
    if (ptr[t0] < 0) return 1;
    for (int t = t0; t < t0 + nt; ++t) {
        const int64_t c = ptr[t + 1] - ptr[t];
        if (c < 1) return 1;
        if (c > *longest) *longest = c;
    }
    return 0;
}

}  // namespace

extern "C" int grl_setdist_block(const float* e, int64_t ld, const int64_t* qptr_host, const int64_t* qptr, int a0, int na,
                                 const int64_t* gptr_host, const int64_t* gptr, int b0, int nb, int reduce, float* out,
                                 int64_t ldo, void* stream) {
    GRL_REQUIRE(e && qptr_host && qptr && gptr_host && gptr && out, "setdist_block: null");
    GRL_REQUIRE(a0 >= 0 && na >= 0 && b0 >= 0 && nb >= 0 && ld >= 0, "setdist_block: a0, na, b0, nb, ld >= 0");
    GRL_REQUIRE(a0 <= INT_MAX - 1 - na && b0 <= INT_MAX - 1 - nb, "setdist_block: a0 + na, b0 + nb beyond int32");
    GRL_REQUIRE(ldo >= nb, "setdist_block: ldo >= nb");
    GRL_REQUIRE(reduce == GRL_SET_MIN || reduce == GRL_SET_MEAN || reduce == GRL_SET_CHAMFER ||
                reduce == GRL_SET_HAUSDORFF, "setdist_block: reduce is not one of GRL_SET_*");
    int64_t longest = 0;
    GRL_REQUIRE(!sd_check_ptr(qptr_host, a0, na, &longest),
                "setdist_block: qptr must start at >= 0 and give every tracklet at least one clip");
    GRL_REQUIRE(!sd_check_ptr(gptr_host, b0, nb, &longest),
                "setdist_block: gptr must start at >= 0 and give every tracklet at least one clip");
    GRL_REQUIRE(ld >= gptr_host[b0 + nb] - gptr_host[b0], "setdist_block: ld is smaller than the block's clip columns");
    if (longest > GRL_SET_MAX_CLIPS)
        return grl_fail(GRL_EUNSUPPORTED, "setdist_block: a tracklet of %lld clips (at most %d)", (long long)longest,
                        GRL_SET_MAX_CLIPS);
    if (na == 0 || nb == 0) return GRL_OK;
    const int64_t groups = ((int64_t)na * nb + SD_WAVES - 1) / SD_WAVES;
    const dim3 grid((unsigned)(groups < SD_MAX_GRID ? groups : SD_MAX_GRID)), block(SD_THREADS);
    hipStream_t st = (hipStream_t)stream;
    switch (reduce) {
    case GRL_SET_MIN:
        hipLaunchKernelGGL(setdist_kernel<GRL_SET_MIN>, grid, block, 0, st, e, ld, qptr, a0, na, gptr, b0, nb, out, ldo);
        break;
    case GRL_SET_MEAN:
        hipLaunchKernelGGL(setdist_kernel<GRL_SET_MEAN>, grid, block, 0, st, e, ld, qptr, a0, na, gptr, b0, nb, out, ldo);
        break;
    case GRL_SET_CHAMFER:
        hipLaunchKernelGGL(setdist_kernel<GRL_SET_CHAMFER>, grid, block, 0, st, e, ld, qptr, a0, na, gptr, b0, nb, out,
                           ldo);
        break;
    default:
        hipLaunchKernelGGL(setdist_kernel<GRL_SET_HAUSDORFF>, grid, block, 0, st, e, ld, qptr, a0, na, gptr, b0, nb, out,
                           ldo);
        break;
    }
    return grl_check_launch("grl_setdist_block");
}
