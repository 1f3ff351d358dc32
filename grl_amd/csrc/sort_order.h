// The one total order of float32 distances in libgrl_hip.so: grl_row_argsort (pointwise.hip), the top-k search and
// the streaming rank counts (search.hip), the re-ranking lists built from them (rerank_stream.hip) and the bins of
// the pair histograms (roc.hip) all take it from here, so "bit-equal to rank_rows(D)[:, :k]" cannot drift.
//
// Keys are compared as order-preserving unsigned integers so that the comparator is a strict total order for every
// input: NaN of any sign becomes the canonical NaN 0x7fc00000 and sorts after +inf as in numpy, -0 == +0, ascending
// otherwise; ties go to the smaller index = np.argsort(kind='stable') (numpy's default introsort leaves ties
// unspecified).  Every key is below 0xffffffff, which pads a sorting network after every real element.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

static __device__ __forceinline__ unsigned order_key(float v) {
    unsigned u = __float_as_uint(v);
    if (v != v) u = 0x7fc00000u;                       // canonical NaN
    else if (v == 0.f) u = 0u;                         // -0 -> +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// (key << 32) | index: unique per row, so "before" (smaller key, then smaller index) is a plain integer compare
static __device__ __forceinline__ uint64_t composite(unsigned key, int index) {
    return ((uint64_t)key << 32) | (uint32_t)index;
}

// The ROC bins follow the same order, except that NaN of either sign takes the largest key: a NaN is
// never accepted before anything else, so it belongs in the last bin whatever `bits` is (order_key's NaN, 0xffc00000,
// reaches the last bin only while bits <= 10).
static __device__ __forceinline__ unsigned roc_key(float v) { return v != v ? 0xffffffffu : order_key(v); }

// Ascending bitonic sort of n (a power of two) LDS entries by one workgroup, optionally carrying a float payload.
// Callers synchronise before; the last stage ends with a barrier.
template <typename T>
static __device__ void bitonic_lds(T* c, float* payload, int n) {
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (n >> 1); t += blockDim.x) {
                const int i = 2 * j * (t / j) + (t % j), l = i + j;
                const bool asc = (i & k) == 0;
                const T ci = c[i], cl = c[l];
                if ((ci > cl) == asc) {
                    c[i] = cl; c[l] = ci;
                    if (payload) { const float f = payload[i]; payload[i] = payload[l]; payload[l] = f; }
                }
            }
            __syncthreads();
        }
    }
}
