// Cluster-memory update of cluster-contrast training (grl_amd/reid/loss/cluster_memory.py): per cluster present in the
// batch, ONE blend of the centroid row -- with the batch's least similar member (hard) or with the members' mean -- and
// its renormalisation.  The per-sample rule is oim_update_kernel of train_head.hip, whose shape and arithmetic this
// follows: one workgroup per batch row, the workgroup of a label's FIRST row is the only writer of that centroid row,
// fixed summation order (f32x4 strided trip, dot4, block_sum), no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grl_hip.h"
#include "common.h"

namespace {

__device__ __forceinline__ float dot4(f32x4 a, f32x4 b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]; }

// Every branch below depends on labels, blockIdx and block_sum totals only: uniform across the workgroup.
__global__ __launch_bounds__(256) void cmem_update_kernel(float* __restrict__ cent, const float* __restrict__ x,
                                                          const int64_t* __restrict__ labels, int n, int D, int K,
                                                          float m, int mode, int32_t* __restrict__ sel) {
    __shared__ float red[16];
    const int i = blockIdx.x;
    const int64_t y = labels[i];
    if (y < 0 || y >= K) {                                // a label outside the memory updates nothing
        if (sel && threadIdx.x == 0) sel[i] = 0;
        return;
    }
    for (int j = 0; j < i; ++j)
        if (labels[j] == y) return;                       // not the first row of this label: its leader writes sel[i]
    float* row = cent + y * (int64_t)D;
    int pick = i, count = 0;
    if (mode == 0) {
        // the least similar member against the row as it is before this launch (this workgroup is its only writer)
        float best = 0.f;
        for (int j = i; j < n; ++j) {
            if (labels[j] != y) continue;
            float s = 0.f;
            for (int c = threadIdx.x * 4; c < D; c += 1024)
                s += dot4(*reinterpret_cast<const f32x4*>(x + (int64_t)j * D + c), *reinterpret_cast<const f32x4*>(row + c));
            s = block_sum(s, red);
            if (j == i) best = s;
            else if (s < best) { best = s; pick = j; }    // strict: the first member wins ties, a NaN never replaces
        }
    } else {
        for (int j = i; j < n; ++j) count += labels[j] == y;
    }
    if (sel && threadIdx.x == 0)
        for (int j = i; j < n; ++j)
            if (labels[j] == y) sel[j] = mode == 0 ? (j == pick) : 1;
    const float cnt = (float)count;
    float ss = 0.f;
    // a pass over the members covers TRIPS column trips of a lane, so the labels are scanned once per 4096 columns;
    // every element still adds its members in ascending j, and ss its trips in ascending c
    constexpr int TRIPS = 4;
    for (int c0 = threadIdx.x * 4; c0 < D; c0 += 1024 * TRIPS) {
        f32x4 v[TRIPS];
        if (mode == 0) {
#pragma unroll
            for (int t = 0; t < TRIPS; ++t)
                if (c0 + 1024 * t < D) v[t] = *reinterpret_cast<const f32x4*>(x + (int64_t)pick * D + c0 + 1024 * t);
        } else {
#pragma unroll
            for (int t = 0; t < TRIPS; ++t) v[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int j = i; j < n; ++j) {
                if (labels[j] != y) continue;
#pragma unroll
                for (int t = 0; t < TRIPS; ++t)
                    if (c0 + 1024 * t < D) v[t] += *reinterpret_cast<const f32x4*>(x + (int64_t)j * D + c0 + 1024 * t);
            }
#pragma unroll
            for (int t = 0; t < TRIPS; ++t) v[t] = v[t] / cnt;
        }
#pragma unroll
        for (int t = 0; t < TRIPS; ++t) {
            const int c = c0 + 1024 * t;
            if (c >= D) break;
            f32x4 r = *reinterpret_cast<const f32x4*>(row + c) * m + v[t] * (1.f - m);
            *reinterpret_cast<f32x4*>(row + c) = r;
            ss += dot4(r, r);
        }
    }
    ss = block_sum(ss, red);
    const float inv = 1.f / sqrtf(ss);
    for (int c = threadIdx.x * 4; c < D; c += 1024)
        *reinterpret_cast<f32x4*>(row + c) = *reinterpret_cast<const f32x4*>(row + c) * inv;
}

}  // namespace

extern "C" int grl_cmem_update(float* cent, const float* x, const int64_t* labels, int n, int D, int K, float momentum,
                               int mode, int32_t* sel, void* stream) {
    GRL_REQUIRE(cent && x && labels && n > 0 && D > 0 && D % 4 == 0 && K > 0, "cmem_update: bad args");
    GRL_REQUIRE(mode == 0 || mode == 1, "cmem_update: mode is 0 (hard) or 1 (mean)");
    GRL_REQUIRE(aligned16(cent) && aligned16(x), "cmem_update: cent and x must be 16-byte aligned");
    hipLaunchKernelGGL(cmem_update_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, cent, x, labels, n, D, K, momentum,
                       mode, sel);
    return grl_check_launch("grl_cmem_update");
}
