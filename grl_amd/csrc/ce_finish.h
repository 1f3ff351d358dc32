// Second launch of the cross entropies whose rows can be INVALID (proxy.hip, hybrid.hip): the first launch leaves per
// row its loss, hit and valid flag in rows [3][n] and dlogits without the 1 / nv.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// nv = the valid rows (every workgroup re-derives it from the same flags, serially: n is small); dlogits *= fl(1 / nv);
// workgroup 0 adds the rows' fl(fl(1 / nv) L_i) and hits in index order.
__global__ __launch_bounds__(256) void ce_finish_kernel(const float* __restrict__ rows, int n, int P,
                                                        float* __restrict__ loss, float* __restrict__ correct,
                                                        float* __restrict__ dz, int64_t ldd) {
    float nv = 0.f;
    for (int r = 0; r < n; ++r) nv += rows[2 * n + r];
    const float inv = nv > 0.f ? 1.f / nv : 0.f;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        float s = 0.f, h = 0.f;
        for (int r = 0; r < n; ++r) { s += inv * rows[r]; h += rows[n + r]; }     // (term by term as grl_softmax_ce's rows)
        loss[0] = s;
        if (correct) correct[0] = h;
    }
    if (!dz) return;
    float* d = dz + (int64_t)blockIdx.y * ldd;            // grid: (1024-column blocks, rows)
    for (int j = blockIdx.x * 1024 + threadIdx.x; j < min(P, (int)(blockIdx.x + 1) * 1024); j += 256) d[j] = inv * d[j];
}

}  // namespace
