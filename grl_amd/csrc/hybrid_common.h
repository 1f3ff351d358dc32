// The parts the hybrid-memory cross entropies of hybrid.hip and soft_hybrid.hip share: a class's logit through the CSR
// table, the student's pass over the classes (class logits into LDS, maximum, first arg-max, lse), the row of an invalid
// target and the scatter of the class gradients to the columns.  One definition each, so that both translation units
// produce the same bits from the same operands (-ffp-contract=off: every * and + rounds once).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"

namespace {

constexpr int HYB_NONE = 0x7fffffff;

// z_c of one row: the members' logits added one by one in list order from the first, divided by (float)|c| -- a
// singleton's is its logit, bit for bit.  (classes are non-empty)
__device__ __forceinline__ float hyb_class_logit(const float* __restrict__ zi, const int32_t* __restrict__ cptr,
                                                 const int32_t* __restrict__ cmem, int c) {
    const int e0 = cptr[c], e1 = cptr[c + 1];
    float s = zi[cmem[e0]];
    for (int e = e0 + 1; e < e1; ++e) s += zi[cmem[e]];
    return s / (float)(e1 - e0);
}

struct HybRow {
    float mx, lse;        // maximum of the class logits; logf of the sum of the shifted exponentials
    int arg;              // first class attaining the maximum (grl_softmax_ce's tie rule); HYB_NONE for a row of NaN
};

// Lane t takes the classes t + 256 k: the class logits into sz (LDS, [C]), then max, arg-max and sum as a wave64 xor tree
// followed by the four waves in sequence.  On return every lane may read all of sz (block_sum's barriers publish it).
__device__ __forceinline__ HybRow hyb_student_pass(const float* __restrict__ zi, const int32_t* __restrict__ cptr,
                                                   const int32_t* __restrict__ cmem, int C, float* sz, float* red,
                                                   int* arg_s) {
    const int tid = threadIdx.x;
    float m = -INFINITY;
    int am = HYB_NONE;
    for (int c = tid; c < C; c += 256) {                  // (a lane reads back only the entries it wrote until the first barrier)
        const float v = hyb_class_logit(zi, cptr, cmem, c);
        sz[c] = v;
        if (v > m) { m = v; am = c; }
    }
    HybRow r;
    r.mx = block_max(m, red);
    int cand = (m == r.mx) ? am : HYB_NONE;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o));
    if ((tid & 63) == 0) arg_s[tid >> 6] = cand;
    float s = 0.f;
    for (int c = tid; c < C; c += 256) s += expf(sz[c] - r.mx);
    s = block_sum(s, red);                                // (its barriers also publish arg_s and sz)
    r.arg = min(min(arg_s[0], arg_s[1]), min(arg_s[2], arg_s[3]));
    r.lse = logf(s);                                      // of the shifted class logits
    return r;
}

// A row whose target is outside [0, C): zeros in dlogits, nothing for loss, hit or nv.
__device__ __forceinline__ void hyb_invalid_row(float* __restrict__ rows, int n, int i, float* __restrict__ dz,
                                                int64_t ldd, int N) {
    const int tid = threadIdx.x;
    if (dz)
        for (int j = tid; j < N; j += 256) dz[(int64_t)i * ldd + j] = 0.f;
    if (tid == 0) { rows[i] = 0.f; rows[n + i] = 0.f; rows[2 * n + i] = 0.f; }
}

// Lane t takes the COLUMNS t + 256 k; sz holds every class's gradient (the caller's barrier published it).
__device__ __forceinline__ void hyb_scatter(float* __restrict__ di, const float* sz, const int32_t* __restrict__ icls,
                                            int N) {
    for (int j = threadIdx.x; j < N; j += 256) di[j] = sz[icls[j]];
}

}  // namespace
