// The parts the batch-hard triplet kernels of loss.hip and soft_triplet.hip share: the distance of two rows by one wave,
// the distance row of an anchor, the hardest positive / negative, and the gather-form backward.  One definition each, so
// that both translation units produce the same bits from the same operands (-ffp-contract=off: every * and + rounds once).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"

namespace {

// sum_k (a_k - b_k)^2 over D4 f32x4 by one wave: lane l takes the vectors l + 64 t, adds the four squares of each left to
// right and its trips in sequence from 0, then the wave64 xor tree.  Every lane receives the sum.
__device__ __forceinline__ float tri_wave_sqdist(const f32x4* __restrict__ a, const f32x4* __restrict__ b, int D4,
                                                 int lane) {
    float s = 0.f;
    for (int k = lane; k < D4; k += 64) {
        const f32x4 d = a[k] - b[k];
        s += d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3];
    }
    return wave_sum(s);
}

__device__ __forceinline__ float tri_dist_of(float sq) { return sqrtf(sq + 1e-12f); }

// The n distances of anchor i into drow (LDS) and dist[i][.]: one wave per j, four waves.  The caller's barrier
// publishes drow.
__device__ __forceinline__ void tri_dist_row(const float* __restrict__ f, int i, int n, int D, float* drow,
                                             float* __restrict__ dist) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const f32x4* fi = reinterpret_cast<const f32x4*>(f + (int64_t)i * D);
    const int D4 = D >> 2;
    for (int j = wave; j < n; j += 4) {
        const float s = tri_wave_sqdist(fi, reinterpret_cast<const f32x4*>(f + (int64_t)j * D), D4, lane);
        if (lane == 0) {
            const float d = tri_dist_of(s);
            drow[j] = d;
            dist[(int64_t)i * n + j] = d;
        }
    }
}

// torch's value formulas and first-index tie rule:  pos value = dist * [same id, j != i],  neg value = dist + 1e5 * [same id]
struct TriSel {
    float z;        // fl(vp - vn)
    int jp, jn;     // first index at the maximum / the minimum, both in [0, n)
    bool has_pos;   // the maximum sits on a real positive (else it is a masked zero and carries no gradient)
};

__device__ __forceinline__ TriSel tri_select(const float* drow, const int64_t* __restrict__ ids, int i, int n) {
    const int64_t yi = ids[i];
    float vp = -INFINITY, vn = INFINITY;
    int jp = 0, jn = 0;
    for (int j = 0; j < n; ++j) {
        const bool same = ids[j] == yi;
        const float p = drow[j] * ((same && j != i) ? 1.f : 0.f);
        const float q = drow[j] + 1e5f * (same ? 1.f : 0.f);
        if (p > vp) { vp = p; jp = j; }
        if (q < vn) { vn = q; jn = j; }
    }
    TriSel s;
    s.z = vp - vn;
    s.jp = jp;
    s.jn = jn;
    s.has_pos = ids[jp] == yi && jp != i;
    return s;
}

// dfeat[r] = sum over anchors i (index order) of the three ways row r enters z_i = d(i,p_i) - d(i,n_i);  gz_of(i) is
// d (sum_i dloss_i loss_i) / d z_i.  Grid (ceil(D4 / 256), n), 256 lanes.
template <typename GZ>
__device__ __forceinline__ void tri_bwd_rows(const float* __restrict__ f, const float* __restrict__ dist,
                                             const int32_t* __restrict__ sel, float* __restrict__ df, int n, int D4,
                                             GZ gz_of) {
    const int r = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    if (k >= D4) return;
    const f32x4* F = reinterpret_cast<const f32x4*>(f);
    const f32x4 fr = F[(int64_t)r * D4 + k];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < n; ++i) {
        const int p = sel[2 * i], q = sel[2 * i + 1];
        if (i != r && p != r && q != r) continue;      // workgroup-uniform
        const float gz = gz_of(i);
        const f32x4 fi = F[(int64_t)i * D4 + k];
        if (i == r) {
            if (p >= 0) acc += (fr - F[(int64_t)p * D4 + k]) * (gz / dist[(int64_t)i * n + p]);
            acc -= (fr - F[(int64_t)q * D4 + k]) * (gz / dist[(int64_t)i * n + q]);
        }
        if (p == r && i != r) acc -= (fi - fr) * (gz / dist[(int64_t)i * n + r]);
        if (q == r && i != r) acc += (fi - fr) * (gz / dist[(int64_t)i * n + r]);
    }
    reinterpret_cast<f32x4*>(df)[(int64_t)r * D4 + k] = acc;
}

}  // namespace
