// Camera-aware proxy cross entropy of unsupervised training (grl_amd/reid/loss/proxy_memory.py): per row a
// cross entropy over the proxies of the row's camera and one over the row's own cluster's proxies plus the k hardest
// proxies of other clusters -- loss, gradient, top-1 hit, own proxy and the selected negatives from one call.
// The shape is softmax_ce_kernel's (loss.hip): one 256-lane workgroup per row (n is at most a few hundred), lane t takes
// the columns t + 256 k, fixed-order reductions, no atomics, plain C++ and vector stores.  The row and one byte of set
// flags per column sit in LDS (5 P bytes <= 40 KB).
//
// The set flags and the selection -- a bitwise top-k threshold, ties admitted in index order, nothing that depends on
// timing -- are proxy_common.h's, shared with soft_proxy.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grl_hip.h"
#include "common.h"
#include "proxy_common.h"
#include "ce_finish.h"

namespace {

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
    __shared__ int cnt_gt[PROXY_MAX_TRIPS * 4], cnt_eq[PROXY_MAX_TRIPS * 4];
    unsigned char* fl = reinterpret_cast<unsigned char*>(sz + P);
    const int i = blockIdx.x, tid = threadIdx.x;
    const int64_t y = labels[i];

    // ---- the row, its flags, own proxy and selected negatives (proxy_common.h) ----
    const ProxyLds lds = {sz, fl, red, redi, cnt_gt, cnt_eq};
    const ProxySel sel = proxy_select(z + (int64_t)i * ld, y, cams[i], pcl, pcm, i, P, k_neg, lds, negsel);
    const int own = sel.own;
    if (own == PROXY_NONE) {                              // invalid row: the noise label, or a pair without a proxy
        proxy_invalid_row(rows, n, i, P, k_neg, dz, ldd, own_out, negsel);
        return;
    }
    const float mxA = sel.mxA;

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
    const float ipos = 1.f / (float)sel.npos;
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
        rows[n + i] = (sel.arg < P && (int64_t)pcl[sel.arg] == y) ? 1.f : 0.f;      // (a row of NaN has no arg-max)
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
