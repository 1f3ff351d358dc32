// Exponential moving average of a whole model in ONE launch (grl_amd/reid/train/teacher.py): for every
// (dst, src, numel) entry of a device table, dst = alpha * dst + (1 - alpha) * src, element by element.  The train step
// is bound by its launch count and a model has ~330 tensors: a launch per tensor is not an option.
// The tensors are cut into chunks of GRL_EMA_CHUNK floats; chunk_first[e] is the number of chunks before entry e, a
// workgroup finds the entry of its chunk by binary search in that table, and a capped grid strides over the chunks.
// Memory bound: 16-byte loads and stores where the chunk's dst and src are 16-byte aligned, scalar otherwise and for the
// tail.  Every element has one writer, no atomics, plain C++ and vector stores.  -ffp-contract=off: two products and one
// sum, each rounded once.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grl_hip.h"
#include "common.h"

namespace {

constexpr int EMA_GRID = 2048;              // 8 workgroups per CU on 256 CUs; the rest of the chunks is strided
constexpr int EMA_VEC = GRL_EMA_CHUNK / 1024;   // float4 per lane and full chunk

__device__ __forceinline__ float ema1(float d, float s, float a, float b) { return a * d + b * s; }

__global__ __launch_bounds__(256) void ema_update_kernel(const GrlEmaEntry* __restrict__ table,
                                                         const int64_t* __restrict__ chunk_first, int count, float a,
                                                         float b) {
    const int tid = threadIdx.x;
    const int64_t total = chunk_first[count];
    for (int64_t ch = blockIdx.x; ch < total; ch += gridDim.x) {
        // the last entry e with chunk_first[e] <= ch (entries without a chunk are stepped over); uniform in the workgroup
        int lo = 0, hi = count;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (chunk_first[mid] <= ch) lo = mid; else hi = mid;
        }
        const GrlEmaEntry e = table[lo];
        const int64_t off = (ch - chunk_first[lo]) * (int64_t)GRL_EMA_CHUNK;
        if (off >= e.numel) continue;                    // (a table that disagrees with its entries writes nothing)
        const int64_t left = e.numel - off;
        const int len = left < GRL_EMA_CHUNK ? (int)left : GRL_EMA_CHUNK;
        float* __restrict__ d = e.dst + off;
        const float* __restrict__ s = e.src + off;
        if ((((uintptr_t)d | (uintptr_t)s) & 15u) == 0) {
            if (len == GRL_EMA_CHUNK) {                  // all loads of the lane in flight before the first store
                f32x4 dv[EMA_VEC], sv[EMA_VEC];
#pragma unroll
                for (int k = 0; k < EMA_VEC; ++k) {
                    dv[k] = *reinterpret_cast<const f32x4*>(d + 4 * (tid + 256 * k));
                    sv[k] = *reinterpret_cast<const f32x4*>(s + 4 * (tid + 256 * k));
                }
#pragma unroll
                for (int k = 0; k < EMA_VEC; ++k) {
                    f32x4 r;
#pragma unroll
                    for (int c = 0; c < 4; ++c) r[c] = ema1(dv[k][c], sv[k][c], a, b);
                    *reinterpret_cast<f32x4*>(d + 4 * (tid + 256 * k)) = r;
                }
            } else {
                const int n4 = len >> 2;
                for (int v = tid; v < n4; v += 256) {
                    const f32x4 dv = *reinterpret_cast<const f32x4*>(d + 4 * v);
                    const f32x4 sv = *reinterpret_cast<const f32x4*>(s + 4 * v);
                    f32x4 r;
#pragma unroll
                    for (int c = 0; c < 4; ++c) r[c] = ema1(dv[c], sv[c], a, b);
                    *reinterpret_cast<f32x4*>(d + 4 * v) = r;
                }
                for (int j = 4 * n4 + tid; j < len; j += 256) d[j] = ema1(d[j], s[j], a, b);
            }
        } else {
            for (int j = tid; j < len; j += 256) d[j] = ema1(d[j], s[j], a, b);
        }
    }
}

}  // namespace

extern "C" int grl_ema_update(const GrlEmaEntry* table_dev, const int64_t* chunk_first_dev, int count, float alpha,
                              float one_minus_alpha, void* stream) {
    GRL_REQUIRE(table_dev && chunk_first_dev, "ema_update: a required pointer is NULL");
    GRL_REQUIRE(count >= 1, "ema_update: bad args (count >= 1)");
    hipLaunchKernelGGL(ema_update_kernel, dim3(EMA_GRID), dim3(256), 0, (hipStream_t)stream, table_dev, chunk_first_dev,
                       count, alpha, one_minus_alpha);
    return grl_check_launch("grl_ema_update");
}
