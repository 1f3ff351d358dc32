// The parts the camera-aware proxy cross entropies of proxy.hip and soft_proxy.hip share: the set flags of a row's
// columns, the row's own proxy, the bitwise top-k threshold over the columns of other clusters and the admission of the
// selected negatives, and the row without a proxy of its own.  One definition each, so that both translation units select
// the same columns and produce the same bits from the same operands.
//
// The selection must not depend on timing: the threshold is the k-th largest order_key (sort_order.h: an order-preserving
// uint32, -0 == +0) among the columns of other clusters, built bit by bit from the top -- 32 exact integer counts "how
// many keys are >= the candidate" -- and the columns that EQUAL it are admitted by a prefix count in index order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grl_hip.h"
#include "common.h"
#include "sort_order.h"

namespace {

constexpr int PROXY_NONE = 0x7fffffff;
constexpr int PROXY_MAX_TRIPS = GRL_PROXY_MAX_P / 256;     // column trips of a lane
constexpr unsigned F_A = 1u, F_POS = 2u, F_NEG = 4u;       // set flags of a column

__device__ __forceinline__ int wave_isum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// block-wide integer sum / min of 4 waves; all threads receive it
__device__ __forceinline__ int block_isum(int v, int* red) {
    v = wave_isum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ int block_imin(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return min(min(red[0], red[1]), min(red[2], red[3]));
}

// The LDS a proxy kernel hands to proxy_select: the row [P] and one byte of flags per column behind it (dynamic), and the
// reduction scratch (static).
struct ProxyLds {
    float* sz;                 // [P] the row
    unsigned char* fl;         // [P] the flags
    float* red;                // [16]
    int* redi;                 // [4]
    int* cnt_gt;               // [PROXY_MAX_TRIPS * 4] per (trip, wave): columns above the threshold
    int* cnt_eq;               // [PROXY_MAX_TRIPS * 4] ... and at it
};

struct ProxySel {
    int own;                   // the row's own proxy; PROXY_NONE: the row is invalid and nothing below is set
    int arg;                   // first index attaining the maximum over all columns
    int npos, k;               // |Pos_i|, |Neg_i|
    float mxA;                 // maximum over A_i
};

// A row without a proxy of its own (the noise label, or a pair without a proxy): zeros, -1s, nothing for loss, hit or nv.
__device__ __forceinline__ void proxy_invalid_row(float* __restrict__ rows, int n, int i, int P, int k_neg,
                                                  float* __restrict__ dz, int64_t ldd, int64_t* __restrict__ own_out,
                                                  int32_t* __restrict__ negsel) {
    const int tid = threadIdx.x;
    if (dz)
        for (int j = tid; j < P; j += 256) dz[(int64_t)i * ldd + j] = 0.f;
    if (negsel)
        for (int t = tid; t < k_neg; t += 256) negsel[(int64_t)i * k_neg + t] = -1;
    if (tid == 0) {
        rows[i] = 0.f; rows[n + i] = 0.f; rows[2 * n + i] = 0.f;
        if (own_out) own_out[i] = -1;
    }
}

// Stage row i of z into LDS with its flags F_A / F_POS, find the own proxy, the arg-max, the maximum over A, |Pos|, then
// select Neg_i: F_NEG set in the flags, negsel row i written (ascending j, padded with -1).  Every branch on `own`, k, thr
// or a block total is uniform across the workgroup.  Ends on a barrier: every lane may read all of sz and fl.
__device__ __forceinline__ ProxySel proxy_select(const float* __restrict__ zi, int64_t y, int64_t cam,
                                                 const int32_t* __restrict__ pcl, const int32_t* __restrict__ pcm, int i,
                                                 int P, int k_neg, const ProxyLds& L, int32_t* __restrict__ negsel) {
    float* sz = L.sz;
    unsigned char* fl = L.fl;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntrips = (P + 255) >> 8;
    ProxySel r;

    // ---- stage the row; own proxy, arg-max over all columns, max over A, |Pos| ----
    float m = -INFINITY, mA = -INFINITY;
    int am = PROXY_NONE, ownc = PROXY_NONE, npos = 0;
    for (int j = tid; j < P; j += 256) {
        const float v = zi[j];
        const bool a = (int64_t)pcm[j] == cam, p = (int64_t)pcl[j] == y;
        sz[j] = v;
        fl[j] = (unsigned char)((a ? F_A : 0u) | (p ? F_POS : 0u));
        if (v > m) { m = v; am = j; }
        if (a) mA = fmaxf(mA, v);
        if (a && p) ownc = min(ownc, j);
        npos += p;
    }
    r.own = block_imin(ownc, L.redi);
    if (r.own == PROXY_NONE) return r;                    // invalid row: the caller writes it (proxy_invalid_row)
    const float mx = block_max(m, L.red);
    r.arg = block_imin(m == mx ? am : PROXY_NONE, L.redi);
    r.mxA = block_max(mA, L.red);
    npos = block_isum(npos, L.redi);
    const int k = min(k_neg, P - npos);                   // |Neg_i|
    r.npos = npos;
    r.k = k;

    // ---- the k-th largest key of N_i ----
    unsigned thr = 0u;                                    // k == |N_i|: every key is above 0 (order_key gives none below 0x003fffff)
    if (k > 0 && k < P - npos) {
        for (int bit = 31; bit >= 0; --bit) {
            const unsigned cand = thr | (1u << bit);
            int c = 0;
            for (int j = tid; j < P; j += 256) c += !(fl[j] & F_POS) && order_key(sz[j]) >= cand;
            if (block_isum(c, L.redi) >= k) thr = cand;
        }
    }
    // ---- admit: every column above the threshold, and the first k - (that many) columns AT it, in index order ----
    if (k > 0) {
        int* cnt_gt = L.cnt_gt;
        int* cnt_eq = L.cnt_eq;
        for (int t = 0; t < ntrips; ++t) {                // (trip count uniform: the ballots see whole waves)
            const int j = t * 256 + tid;
            const bool inN = j < P && !(fl[j] & F_POS);
            const unsigned key = inN ? order_key(sz[j]) : 0u;
            const unsigned long long bg = __ballot(inN && key > thr), be = __ballot(inN && key == thr);
            if (lane == 0) { cnt_gt[t * 4 + wave] = __popcll(bg); cnt_eq[t * 4 + wave] = __popcll(be); }
        }
        __syncthreads();
        int total_gt = 0;
        for (int e = 0; e < ntrips * 4; ++e) total_gt += cnt_gt[e];
        const int room = k - total_gt;                    // places left for columns at the threshold (>= 1 unless k == |N_i|)
        const unsigned long long below = (1ull << lane) - 1ull;
        int run_gt = 0, run_eq = 0;
        for (int t = 0; t < ntrips; ++t) {
            const int j = t * 256 + tid;
            const bool inN = j < P && !(fl[j] & F_POS);
            const unsigned key = inN ? order_key(sz[j]) : 0u;
            const bool gt = inN && key > thr, eq = inN && key == thr;
            const unsigned long long bg = __ballot(gt), be = __ballot(eq);
            int g0 = run_gt, e0 = run_eq;
            for (int w = 0; w < 4; ++w) {
                const int cg = cnt_gt[t * 4 + w], ce = cnt_eq[t * 4 + w];
                if (w < wave) { g0 += cg; e0 += ce; }
                run_gt += cg; run_eq += ce;
            }
            g0 += __popcll(bg & below);                   // columns above / at the threshold before j
            e0 += __popcll(be & below);
            if (gt || (eq && e0 < room)) {
                fl[j] = (unsigned char)(fl[j] | F_NEG);   // (this lane is the column's only writer)
                const int rank = g0 + min(e0, max(room, 0));
                if (negsel && rank < k_neg) negsel[(int64_t)i * k_neg + rank] = j;
            }
        }
    }
    if (negsel)
        for (int t = k + tid; t < k_neg; t += 256) negsel[(int64_t)i * k_neg + t] = -1;
    __syncthreads();
    return r;
}

}  // namespace
