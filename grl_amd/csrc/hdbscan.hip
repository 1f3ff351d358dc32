// The minimum spanning forest of the mutual-reachability graph over column blocks of the distance matrix
// (engine.mutual_reachability_mst / hdbscan / hdbscan_matrix).  The n x n matrix is never whole: one
// Boruvka round is one pass over the column blocks, and every block is folded into two words per row -- the row's
// lightest edge that leaves its component.
//
// Pair {lo < hi}: dist = the entry of the block as it is, or, with rinv given, the cosine form of d = -dot made
// symmetric: v = (d * rinv[lo]) * rinv[hi] (the smaller index first, whichever of the two is the row), dist = 1.0f + v,
// dist < 0 ? 0 : dist.  w = dist; if (core[lo] > w) w = core[lo]; if (core[hi] > w) w = core[hi].  An edge needs both
// core distances finite and w < +inf (a NaN is no edge).  Total order of the edges: (w by float <, lo, hi); for a fixed
// row i that is (w, j), because every j < i gives lo = j < i and every j > i gives lo = i.
//
// Mapping.  One wave per row, lane l takes the columns l, l + 64, .. of the block: every load of the row is one
// coalesced 256-byte run, and comp[j], core[j], rinv[j] are coalesced reads of three arrays that stay in L2.  A lane
// keeps its best (w, j) under strict <, which keeps the smaller j of equal weights because its j ascend; the wave joins
// the 64 lexicographically by shuffles and folds the result into the row's best of the earlier blocks, comparing j
// there too, so neither the lane a column falls on nor the block cuts show in the result.  No LDS, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include "../../include/grl_hip.h"
#include "common.h"

namespace {

constexpr int HDB_THREADS = 256;
constexpr int HDB_WAVES = HDB_THREADS / 64;

__device__ __forceinline__ bool hdb_finite(float v) { return fabsf(v) < INFINITY; }        // (false for a NaN)

// the cosine form of d = -dot for the pair (i, j): the smaller index multiplies first
__device__ __forceinline__ float hdb_cosine(float d, int i, int j, float ri, float rj) {
    float v = j < i ? (d * rj) * ri : (d * ri) * rj;
    v = 1.0f + v;
    return v < 0.f ? 0.f : v;                                      // (a NaN stays)
}

// (w, j) before (bw, bj): lighter, or as light with the smaller index; j = -1 (nothing yet) is the largest index
__device__ __forceinline__ bool hdb_before(float w, int j, float bw, int bj) {
    return w < bw || (w == bw && (unsigned)j < (unsigned)bj);
}

template <bool COS>
__global__ __launch_bounds__(HDB_THREADS) void hdb_minedge_kernel(const float* __restrict__ d, int64_t ld, int nrows,
                                                                  int row0, int c0, int ncols,
                                                                  const float* __restrict__ core,
                                                                  const int32_t* __restrict__ comp,
                                                                  const float* __restrict__ rinv,
                                                                  float* __restrict__ best_w,
                                                                  int32_t* __restrict__ best_j) {
    const int lane = threadIdx.x & 63;
    // (the wave index is the same in all 64 lanes: the row's comp / core / rinv stay in scalar registers)
    const int r = blockIdx.x * HDB_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= nrows) return;
    const int i = row0 + r;
    const float ci = core[i];
    if (!hdb_finite(ci)) {                                         // a sample without a core distance has no edges
        if (c0 == 0 && lane == 0) { best_w[i] = INFINITY; best_j[i] = -1; }
        return;
    }
    const int mi = comp[i];
    const float ri = COS ? rinv[i] : 0.f;
    const float* __restrict__ drow = d + (int64_t)r * ld;
    float bw = INFINITY;
    int bj = -1;
    for (int col = lane; col < ncols; col += 64) {
        const int j = c0 + col;
        float w = drow[col];
        const int mj = comp[j];
        const float cj = core[j];
        if (COS) w = hdb_cosine(w, i, j, ri, rinv[j]);
        const float clo = j < i ? cj : ci, chi = j < i ? ci : cj;
        if (clo > w) w = clo;
        if (chi > w) w = chi;
        if (mj != mi && hdb_finite(cj) && w < bw) { bw = w; bj = j; }      // (bw <= +inf: a NaN or +inf w never enters)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ow = __shfl_xor(bw, o);
        const int oj = __shfl_xor(bj, o);
        if (hdb_before(ow, oj, bw, bj)) { bw = ow; bj = oj; }
    }
    if (lane == 0) {
        if (c0 != 0) {                                             // the row's best of the earlier blocks
            const float pw = best_w[i];
            const int pj = best_j[i];
            if (!hdb_before(bw, bj, pw, pj)) { bw = pw; bj = pj; }
        }
        best_w[i] = bw; best_j[i] = bj;
    }
}

__global__ __launch_bounds__(HDB_THREADS) void hdb_cosine_kernel(float* __restrict__ d, int64_t ld, int nrows, int row0,
                                                                 int c0, int ncols, const float* __restrict__ rinv) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * HDB_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= nrows) return;
    const int i = row0 + r;
    const float ri = rinv[i];
    float* __restrict__ drow = d + (int64_t)r * ld;
    for (int col = lane; col < ncols; col += 64) drow[col] = hdb_cosine(drow[col], i, c0 + col, ri, rinv[c0 + col]);
}

}  // namespace

extern "C" int grl_hdbscan_minedge_block(const float* d, int64_t ld, int n, int nrows, int row0, int c0, int ncols,
                                         const float* core, const int32_t* comp, const float* rinv, float* best_w,
                                         int32_t* best_j, void* stream) {
    GRL_REQUIRE(n >= 0 && nrows >= 0 && row0 >= 0 && c0 >= 0, "hdbscan_minedge_block: n, nrows, row0, c0 >= 0");
    GRL_REQUIRE(ncols >= 1 && ld >= ncols, "hdbscan_minedge_block: ncols >= 1 and ld >= ncols");
    GRL_REQUIRE(row0 <= n - nrows && c0 <= n - ncols, "hdbscan_minedge_block: rows or columns beyond n");
    GRL_REQUIRE(d && core && comp && best_w && best_j, "hdbscan_minedge_block: null");
    if (nrows == 0) return GRL_OK;
    const dim3 grid(grl_ceil_div(nrows, HDB_WAVES)), block(HDB_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (rinv)
        hipLaunchKernelGGL(hdb_minedge_kernel<true>, grid, block, 0, st, d, ld, nrows, row0, c0, ncols, core, comp, rinv,
                           best_w, best_j);
    else
        hipLaunchKernelGGL(hdb_minedge_kernel<false>, grid, block, 0, st, d, ld, nrows, row0, c0, ncols, core, comp, rinv,
                           best_w, best_j);
    return grl_check_launch("grl_hdbscan_minedge_block");
}

extern "C" int grl_hdbscan_cosine_block(float* d, int64_t ld, int n, int nrows, int row0, int c0, int ncols,
                                        const float* rinv, void* stream) {
    GRL_REQUIRE(n >= 0 && nrows >= 0 && row0 >= 0 && c0 >= 0, "hdbscan_cosine_block: n, nrows, row0, c0 >= 0");
    GRL_REQUIRE(ncols >= 1 && ld >= ncols, "hdbscan_cosine_block: ncols >= 1 and ld >= ncols");
    GRL_REQUIRE(row0 <= n - nrows && c0 <= n - ncols, "hdbscan_cosine_block: rows or columns beyond n");
    GRL_REQUIRE(d && rinv, "hdbscan_cosine_block: null");
    if (nrows == 0) return GRL_OK;
    hipLaunchKernelGGL(hdb_cosine_kernel, dim3(grl_ceil_div(nrows, HDB_WAVES)), dim3(HDB_THREADS), 0,
                       (hipStream_t)stream, d, ld, nrows, row0, c0, ncols, rinv);
    return grl_check_launch("grl_hdbscan_cosine_block");
}
