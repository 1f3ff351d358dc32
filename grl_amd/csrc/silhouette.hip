// Silhouette coefficients of a clustering over column blocks of the distance matrix (engine.silhouette /
// silhouette_matrix).  The n x n matrix is never whole: a block holds the columns of the positions
// [c0, c0 + ncols) of the MEMBER ORDER (grl_kmeans_members: cluster 0's samples ascending, then cluster 1's, ..), so
// every cluster is a run of consecutive columns and a row's sum towards it is a segmented sum along the row.
//
// Sum of row i towards cluster c (normative order, independent of the block cuts).  64 partial sums; partial l is the
// sequential fp32 sum from +0.0f, in ascending position, of the distances at the cluster's positions p with
// p % 64 == l, the position of sample i itself left out (by index, not by value); then the tree
// part[l] += part[l + s], l < s, for s = 32, 16, 8, 4, 2, 1.  Adds only, no atomics of any kind.
//
// Mapping.  One wave per row, lane = p % 64: a chunk of 64 positions is one coalesced 256-byte load of the row.  The
// lane partials of the cluster in progress live in one register per lane; at every cluster end inside the chunk the
// wave runs the tree (six cross-lane adds), divides, and folds the mean into a(i) or the running minimum b(i).  A
// cluster that lies inside one chunk takes the same path: its lanes hold one distance each and the others +0.0f,
// which is the order above.  A cluster of ONE member needs neither tree nor division (its sum and its mean are the one
// distance): a run of them inside a chunk is found with one 64-wide load of mptr and a ballot, and every lane folds its
// own candidate into a lane-local minimum that joins b(i) at the end of the block.  The minimum is a total order (-0
// below +0, NaN absorbing), so the order in which candidates meet does not show.  Between the blocks of a pass the
// state is O(n): the 64 partials of the one cluster that straddles the block edge, a and bmin.  The kernel reads every
// distance once; the GEMM that makes the block costs d multiply-adds per distance.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include "../../include/grl_hip.h"
#include "common.h"

namespace {

constexpr int SIL_THREADS = 256;
constexpr int SIL_WAVES = SIL_THREADS / 64;

// the cluster whose positions hold p: the largest c in 0..k-1 with mptr[c] <= p (0 <= p < mptr[k]); never empty
__device__ __forceinline__ int sil_cluster_of(const int64_t* __restrict__ mptr, int k, int64_t p) {
    int lo = 0, hi = k;                            // mptr[lo] <= p < mptr[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (mptr[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// the smaller of two means, -0 below +0, NaN as soon as one of them is NaN: associative and commutative, so the order
// in which the candidates for b(i) meet does not show in the bits
__device__ __forceinline__ float sil_min(float b, float m) {
    if (b != b || m != m) return NAN;
    return (m < b || (m == b && signbit(m) && !signbit(b))) ? m : b;
}

// part[l] += part[l + s] for l < s, s = 32 .. 1; every lane receives part[0]
__device__ __forceinline__ float sil_tree(float v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s);      // (lanes >= s hold values nobody reads)
    return __shfl(v, 0);
}

template <bool COS>
__global__ __launch_bounds__(SIL_THREADS) void sil_block_kernel(const float* __restrict__ d, int64_t ld, int nrows,
                                                                int row0, int64_t c0, int ncols,
                                                                const int32_t* __restrict__ mem,
                                                                const int64_t* __restrict__ mptr, int k,
                                                                const int32_t* __restrict__ labels,
                                                                const float* __restrict__ rinv_row,
                                                                const float* __restrict__ rinv_pos,
                                                                float* __restrict__ part, float* __restrict__ a,
                                                                float* __restrict__ bmin) {
    const int lane = threadIdx.x & 63;
    // (the wave index is the same in all 64 lanes: everything derived from it stays in scalar registers)
    const int r = blockIdx.x * SIL_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= nrows) return;
    const int i = row0 + r;
    const int lab = labels[i];
    if ((unsigned)lab >= (unsigned)k) return;                     // nobody's: neither a row nor a column
    const int64_t m = mptr[k];
    const int64_t pb = c0, pe = min(c0 + (int64_t)ncols, m);
    if (pb >= pe) return;
    // the position of sample i itself: a cluster's samples ascend in mem
    const int64_t le = min(mptr[lab + 1], m);
    int64_t self = lower_bound<int64_t>(mem, mptr[lab], le, i);
    if (self >= le || mem[self] != i) self = -1;

    int c = sil_cluster_of(mptr, k, pb);
    int64_t cs = mptr[c], ce = mptr[c + 1];
    float acc = pb == cs ? 0.f : part[(int64_t)i * 64 + lane];     // the cluster began in an earlier block
    float av = 0.f, bv = INFINITY;
    if (pb != 0) { av = a[i]; bv = bmin[i]; }
    float bl = INFINITY;                                           // the lane's own candidates (one-member clusters)
    const float ri = COS ? rinv_row[i] : 0.f;
    const float* __restrict__ drow = d + (int64_t)r * ld;

    for (int64_t base = pb & ~(int64_t)63; base < pe && c < k; base += 64) {
        const int64_t p = base + lane;
        const bool valid = p >= pb && p < pe;
        float v = 0.f;
        if (valid) {
            v = drow[p - c0];
            if (COS) {
                v = (v * ri) * rinv_pos[p];
                v = 1.0f + v;
                v = v < 0.f ? 0.f : v;                             // (a NaN stays)
            }
        }
        const int64_t lim = min(base + 64, pe);
        for (;;) {
            if (ce == cs + 1) {
                // A run of one-member clusters c, c + 1, .. inside this chunk: their sums are the single distance
                // (+0.0f + v, and the tree adds +0.0f), their means the same value: every lane folds its own
                // candidate, no tree, no division.  The run = the leading lanes l with mptr[c + 1 + l] == cs + l + 1.
                const int64_t q = c + 1 + lane <= k ? mptr[c + 1 + lane] : -1;
                const unsigned long long run = __ballot(q == cs + lane + 1);
                const int64_t len = min((int64_t)(~run ? __builtin_ctzll(~run) : 64), lim - cs);
                if (valid && p >= cs && p < cs + len && p != self) bl = sil_min(bl, 0.f + v);
                if (lab >= c && lab < c + len) av = 0.f;            // the row's own cluster of one
                c += (int)len; cs += len;
                while (c < k && mptr[c + 1] == cs) ++c;            // empty clusters are no candidates
                if (c >= k) break;
                ce = mptr[c + 1];
                if (cs >= lim) break;
                continue;
            }
            if (valid && p >= cs && p < ce && p != self) acc += v;
            if (ce > lim) break;                                   // goes on in the next chunk or block
            const float tot = sil_tree(acc);
            const int64_t nc = ce - cs;
            if (c == lab) {
                av = nc > 1 ? tot / (float)(nc - 1) : 0.f;
            } else {
                const float mean = tot / (float)nc;
                bv = sil_min(bv, mean);
            }
            acc = 0.f;
            do { ++c; } while (c < k && mptr[c + 1] == mptr[c]);   // empty clusters are no candidates
            if (c >= k) break;
            cs = mptr[c]; ce = mptr[c + 1];
            if (cs >= lim) break;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bl = sil_min(bl, __shfl_xor(bl, o));
    if (lane == 0) { a[i] = av; bmin[i] = sil_min(bv, bl); }
    if (c < k) part[(int64_t)i * 64 + lane] = acc;
}

__global__ __launch_bounds__(SIL_THREADS) void sil_finish_kernel(float* __restrict__ a, float* __restrict__ bmin,
                                                                 const int32_t* __restrict__ labels,
                                                                 const int32_t* __restrict__ counts, int n, int k,
                                                                 float* __restrict__ s) {
    for (int i = blockIdx.x * SIL_THREADS + threadIdx.x; i < n; i += gridDim.x * SIL_THREADS) {
        const int lab = labels[i];
        float out;
        if ((unsigned)lab >= (unsigned)k) {                       // nobody's
            a[i] = 0.f; bmin[i] = 0.f; out = 0.f;
        } else if (counts[lab] <= 1) {                            // a cluster of one
            a[i] = 0.f; out = 0.f;
        } else {
            const float av = a[i], bv = bmin[i];
            const float mx = av > bv ? av : bv;
            if (av != av || bv != bv) out = NAN;
            else if (mx == 0.f) out = 0.f;
            else out = (bv - av) / mx;
        }
        s[i] = out;
    }
}

__global__ __launch_bounds__(SIL_THREADS) void sil_rinv_kernel(const float* __restrict__ sq, int n,
                                                               float* __restrict__ rinv) {
    for (int i = blockIdx.x * SIL_THREADS + threadIdx.x; i < n; i += gridDim.x * SIL_THREADS)
        rinv[i] = 1.0f / sqrtf(sq[i]);
}

}  // namespace

extern "C" int grl_silhouette_block(const float* d, int64_t ld, int nrows, int row0, int64_t c0, int ncols,
                                    const int32_t* mem, const int64_t* mptr, int k, const int32_t* labels,
                                    const float* rinv_row, const float* rinv_pos, float* part, float* a, float* bmin,
                                    void* stream) {
    GRL_REQUIRE(nrows >= 0 && row0 >= 0 && c0 >= 0 && k >= 1, "silhouette_block: nrows, row0, c0 >= 0, k >= 1");
    GRL_REQUIRE(ncols >= 1 && ld >= ncols, "silhouette_block: ncols >= 1 and ld >= ncols");
    GRL_REQUIRE(row0 <= INT_MAX - nrows, "silhouette_block: row0 + nrows beyond int32");
    GRL_REQUIRE(d && mem && mptr && labels && part && a && bmin, "silhouette_block: null");
    GRL_REQUIRE((rinv_row == nullptr) == (rinv_pos == nullptr),
                "silhouette_block: rinv_row and rinv_pos go together");
    if (nrows == 0) return GRL_OK;
    const dim3 grid(grl_ceil_div(nrows, SIL_WAVES)), block(SIL_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (rinv_row)
        hipLaunchKernelGGL(sil_block_kernel<true>, grid, block, 0, st, d, ld, nrows, row0, c0, ncols, mem, mptr, k,
                           labels, rinv_row, rinv_pos, part, a, bmin);
    else
        hipLaunchKernelGGL(sil_block_kernel<false>, grid, block, 0, st, d, ld, nrows, row0, c0, ncols, mem, mptr, k,
                           labels, rinv_row, rinv_pos, part, a, bmin);
    return grl_check_launch("grl_silhouette_block");
}

extern "C" int grl_silhouette_finish(float* a, float* bmin, const int32_t* labels, const int32_t* counts, int n, int k,
                                     float* s, void* stream) {
    GRL_REQUIRE(n >= 0 && k >= 1, "silhouette_finish: n >= 0, k >= 1");
    if (n == 0) return GRL_OK;
    GRL_REQUIRE(a && bmin && labels && counts && s, "silhouette_finish: null");
    hipLaunchKernelGGL(sil_finish_kernel, dim3(grid_for(n, SIL_THREADS)), dim3(SIL_THREADS), 0, (hipStream_t)stream, a,
                       bmin, labels, counts, n, k, s);
    return grl_check_launch("grl_silhouette_finish");
}

extern "C" int grl_silhouette_rinv(const float* sq, int n, float* rinv, void* stream) {
    GRL_REQUIRE(n >= 0, "silhouette_rinv: n >= 0");
    if (n == 0) return GRL_OK;
    GRL_REQUIRE(sq && rinv, "silhouette_rinv: null");
    hipLaunchKernelGGL(sil_rinv_kernel, dim3(grid_for(n, SIL_THREADS)), dim3(SIL_THREADS), 0, (hipStream_t)stream, sq,
                       n, rinv);
    return grl_check_launch("grl_silhouette_rinv");
}
