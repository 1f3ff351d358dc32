// Camera-aware proxy cross entropy of unsupervised training (grl_amd/reid/loss/proxy_memory.py): per row a
// cross entropy over the proxies of the row's camera and one over the row's own cluster's proxies plus the k hardest
// proxies of other clusters -- loss, gradient, top-1 hit, own proxy and the selected negatives from one call.
// The shape is softmax_ce_kernel's (loss.hip): one 256-lane workgroup per row (n is at most a few hundred), lane t takes
// the columns t + 256 k, fixed-order reductions, no atomics, plain C++ and vector stores.  The row and one byte of set
// flags per column sit in LDS (5 P bytes <= 40 KB).
//
// The selection must not depend on timing: the threshold is the k-th largest order_key (sort_order.h: an order-preserving
// uint32, -0 == +0) among the columns of other clusters, built bit by bit from the top -- 32 exact integer counts "how
// many keys are >= the candidate" -- and the columns that EQUAL it are admitted by a prefix count in index order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grl_hip.h"
#include "common.h"
#include "sort_order.h"
#include "ce_finish.h"

namespace {

constexpr int NONE = 0x7fffffff;
constexpr int MAX_TRIPS = GRL_PROXY_MAX_P / 256;           // column trips of a lane
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

// One workgroup per row.  Every branch on `own`, k, thr or a block total is uniform across the workgroup.  dlogits comes
// out WITHOUT the 1 / nv of the contract (ce_finish_kernel applies it): a row does not know the other rows' validity.
__global__ __launch_bounds__(256) void proxy_ce_kernel(const float* __restrict__ z, int64_t ld,
                                                       const int64_t* __restrict__ labels,
                                                       const int64_t* __restrict__ cams,
                                                       const int32_t* __restrict__ pcl, const int32_t* __restrict__ pcm,
                                                       int n, int P, int k_neg, float w_intra, float w_inter,
                                                       float* __restrict__ rows,      // [3][n]: loss, hit, valid
                                                       float* __restrict__ dz, int64_t ldd, int64_t* __restrict__ own_out,
                                                       int32_t* __restrict__ negsel) {
    extern __shared__ __attribute__((aligned(16))) float sz[];         // [P] the row, then [P] bytes of flags
    __shared__ float red[16];
    __shared__ int redi[4];
    __shared__ int cnt_gt[MAX_TRIPS * 4], cnt_eq[MAX_TRIPS * 4];       // per (trip, wave): columns above / at the threshold
    unsigned char* fl = reinterpret_cast<unsigned char*>(sz + P);
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntrips = (P + 255) >> 8;
    const float* zi = z + (int64_t)i * ld;
    const int64_t y = labels[i], cam = cams[i];

    // ---- stage the row; own proxy, arg-max over all columns, max over A, |Pos| ----
    float m = -INFINITY, mA = -INFINITY;
    int am = NONE, ownc = NONE, npos = 0;
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
    const int own = block_imin(ownc, redi);
    if (own == NONE) {                                    // invalid row: the noise label, or a pair without a proxy
        if (dz)
            for (int j = tid; j < P; j += 256) dz[(int64_t)i * ldd + j] = 0.f;
        if (negsel)
            for (int t = tid; t < k_neg; t += 256) negsel[(int64_t)i * k_neg + t] = -1;
        if (tid == 0) {
            rows[i] = 0.f; rows[n + i] = 0.f; rows[2 * n + i] = 0.f;
            if (own_out) own_out[i] = -1;
        }
        return;
    }
    const float mx = block_max(m, red);
    const int arg = block_imin(m == mx ? am : NONE, redi);            // first index attaining the maximum
    const float mxA = block_max(mA, red);
    npos = block_isum(npos, redi);
    const int k = min(k_neg, P - npos);                   // |Neg_i|

    // ---- the k-th largest key of N_i ----
    unsigned thr = 0u;                                    // k == |N_i|: every key is above 0 (order_key gives none below 0x003fffff)
    if (k > 0 && k < P - npos) {
        for (int bit = 31; bit >= 0; --bit) {
            const unsigned cand = thr | (1u << bit);
            int c = 0;
            for (int j = tid; j < P; j += 256) c += !(fl[j] & F_POS) && order_key(sz[j]) >= cand;
            if (block_isum(c, redi) >= k) thr = cand;
        }
    }
    // ---- admit: every column above the threshold, and the first k - (that many) columns AT it, in index order ----
    if (k > 0) {
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

    // ---- the two cross entropies ----
    float mU = -INFINITY;
    for (int j = tid; j < P; j += 256)
        if (fl[j] & (F_POS | F_NEG)) mU = fmaxf(mU, sz[j]);
    const float mxU = block_max(mU, red);
    float sA = 0.f, sU = 0.f, sP = 0.f;
    for (int j = tid; j < P; j += 256) {
        const unsigned f = fl[j];
        const float v = sz[j];
        if (f & F_A) sA += expf(v - mxA);
        if (f & (F_POS | F_NEG)) sU += expf(v - mxU);
        if (f & F_POS) sP += v - mxU;
    }
    sA = block_sum(sA, red);
    sU = block_sum(sU, red);
    sP = block_sum(sP, red);
    const float lseA = logf(sA), lseU = logf(sU);         // of the shifted sets
    const float ipos = 1.f / (float)npos;
    if (dz) {
        float* di = dz + (int64_t)i * ldd;
        for (int j = tid; j < P; j += 256) {
            const unsigned f = fl[j];
            const float v = sz[j];
            float ga = 0.f, gu = 0.f;
            if (f & F_A) ga = w_intra * (expf(v - mxA - lseA) - (j == own ? 1.f : 0.f));
            if (f & (F_POS | F_NEG)) gu = w_inter * (expf(v - mxU - lseU) - ((f & F_POS) ? ipos : 0.f));
            di[j] = ga + gu;
        }
    }
    if (tid == 0) {
        rows[i] = w_intra * (lseA - (sz[own] - mxA)) + w_inter * (lseU - sP * ipos);
        rows[n + i] = (arg < P && (int64_t)pcl[arg] == y) ? 1.f : 0.f;      // (a row of NaN has no arg-max)
        rows[2 * n + i] = 1.f;
        if (own_out) own_out[i] = own;
    }
}

}  // namespace

extern "C" int grl_proxy_ce(const float* logits, int64_t ld, const int64_t* labels, const int64_t* cams,
                            const int32_t* proxy_cluster, const int32_t* proxy_cam, int n, int P, int k_neg, float w_intra,
                            float w_inter, float* loss, float* correct, float* dlogits, int64_t ldd, int64_t* own,
                            int32_t* negsel, float* ws, void* stream) {
    GRL_REQUIRE(logits && labels && cams && proxy_cluster && proxy_cam && loss && ws, "proxy_ce: a required pointer is NULL");
    GRL_REQUIRE(n > 0 && P > 0 && ld >= P, "proxy_ce: bad args (n >= 1, P >= 1, ld >= P)");
    GRL_REQUIRE(P <= GRL_PROXY_MAX_P, "proxy_ce: more than GRL_PROXY_MAX_P = 8192 proxies");
    GRL_REQUIRE(k_neg >= 0 && k_neg <= P, "proxy_ce: k_neg outside 0 .. P");
    GRL_REQUIRE(!dlogits || ldd >= P, "proxy_ce: ldd < P");
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)P * sizeof(float) + (size_t)((P + 3) & ~3);
    hipLaunchKernelGGL(proxy_ce_kernel, dim3(n), dim3(256), lds, s, logits, ld, labels, cams, proxy_cluster, proxy_cam, n, P,
                       k_neg, w_intra, w_inter, ws, dlogits, ldd, own, k_neg > 0 ? negsel : nullptr);
    hipLaunchKernelGGL(ce_finish_kernel, dlogits ? dim3(grl_ceil_div(P, 1024), n) : dim3(1), dim3(256), 0, s, ws, n, P,
                       loss, correct, dlogits, ldd);
    return grl_check_launch("grl_proxy_ce");
}
