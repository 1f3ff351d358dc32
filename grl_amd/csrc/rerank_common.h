// Device helpers shared by the materialised (rerank.hip) and the streaming (rerank_stream.hip) k-reciprocal
// re-ranking: the limits, numpy's pairwise sum, the k-reciprocal test and the expanded neighbour list of a sample.
// Both translation units compile these same bodies with the same flags, so they produce the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int RR_LMAX = 256;          // k-reciprocal expansion list: (k1+1) + (k1+1)*(k1/2+1) <= 256 for k1 <= 20
constexpr int RR_K1MAX = 20;
constexpr int RR_K2MAX = 8;
constexpr int RR_SLOTS = 64;          // gallery columns per lane in the Jaccard pass: N <= 256 * 64

// numpy's pairwise summation of a contiguous float32 array (np.sum, n <= 256 here)
__device__ float np_pairwise_sum(const float* a, int n) {
    if (n < 8) {
        float r = 0.f;
        for (int i = 0; i < n; ++i) r += a[i];
        return r;
    }
    if (n <= 128) {
        float r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        int i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_sum(a, n2) + np_pairwise_sum(a + n2, n - n2);
}

// k-reciprocal neighbours of `s` among its top (k+1): members f of rank[s][0..k] whose own top (k+1)
// contains s.  One wave; returns the ballot mask over the first k+1 lanes (order = rank order).
__device__ __forceinline__ unsigned long long krecip_mask(const int32_t* __restrict__ rank, int64_t ld, int s, int k,
                                                         int lane, int& f_out) {
    bool member = false;
    int f = -1;
    if (lane <= k) {
        f = rank[(int64_t)s * ld + lane];
        const int32_t* rf = rank + (int64_t)f * ld;
        for (int c = 0; c <= k; ++c) member |= (rf[c] == s);
    }
    f_out = f;
    return __ballot(member);
}

// Expanded neighbour list of sample i (one wave, lanes 0..63): its k1-reciprocal set, extended by the
// half-reciprocal set of every member that overlaps it by more than 2/3, sorted and unique (np.unique) in
// raw[0..return).  rank holds each sample's ascending neighbour order (row stride ld, at least k1 + 1 valid
// entries).  base [RR_K1MAX + 1], raw / srt [RR_LMAX] and n_raw are LDS of the caller.
__device__ int rr_expansion_list(const int32_t* __restrict__ rank, int64_t ld, int i, int k1, int half, int lane,
                                 int* base, int* raw, int* srt, int* n_raw) {
    const unsigned long long below = (1ull << lane) - 1ull;
    int f;
    const unsigned long long mb = krecip_mask(rank, ld, i, k1, lane, f);
    const int nb = __popcll(mb);
    if ((mb >> lane) & 1ull) {
        const int p = __popcll(mb & below);
        base[p] = f;
        raw[p] = f;
    }
    if (lane == 0) *n_raw = nb;
    __syncthreads();
    for (int b = 0; b < nb; ++b) {
        const int cand = base[b];
        int f2;
        const unsigned long long mc = krecip_mask(rank, ld, cand, half, lane, f2);
        const int nc = __popcll(mc);
        bool in_base = false;
        if ((mc >> lane) & 1ull)
            for (int t = 0; t < nb; ++t) in_base |= (base[t] == f2);
        const int inter = __popcll(__ballot(in_base));
        // len(intersect1d(cand_set, base)) > 2./3 * len(cand_set), evaluated in double as numpy does
        if ((double)inter > 2.0 / 3.0 * (double)nc) {
            const int off = *n_raw;
            if ((mc >> lane) & 1ull) raw[off + __popcll(mc & below)] = f2;
            __syncthreads();
            if (lane == 0) *n_raw = off + nc;
        }
        __syncthreads();
    }
    const int L = *n_raw;
    // np.unique: sort by (value, position), drop repeats
    for (int a = lane; a < L; a += 64) {
        const int va = raw[a];
        int p = 0;
        for (int b = 0; b < L; ++b) p += (raw[b] < va || (raw[b] == va && b < a)) ? 1 : 0;
        srt[p] = va;
    }
    __syncthreads();
    int n_u = 0;                                   // ordered compaction, 64 entries per round
    for (int a0 = 0; a0 < L; a0 += 64) {
        const int a = a0 + lane;
        const bool keep = a < L && (a == 0 || srt[a] != srt[a - 1]);
        const unsigned long long mk = __ballot(keep);
        const int v = a < L ? srt[a] : 0;
        __syncthreads();                            // every lane has read srt[a], srt[a-1] of this round
        if (keep) raw[n_u + __popcll(mk & below)] = v;
        n_u += __popcll(mk);
    }
    __syncthreads();
    return n_u;
}

}  // namespace
