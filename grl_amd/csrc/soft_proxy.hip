// Camera-aware proxy cross entropy against hard targets blended with a teacher's softmaxes
// (grl_amd/reid/loss/soft_proxy_memory.py; CAP, Wang et al. 2021 with MMT's soft target, Ge et al. 2020):
// proxy.hip's two cross entropies -- over the proxies of the row's camera, and over the row's own cluster's proxies plus
// the k hardest proxies of other clusters -- each against (1 - w) its hard target + w the teacher's softmax over the SAME
// set.  The sets, the own proxy, the selected negatives and the top-1 hit come from the STUDENT's row (proxy_common.h,
// shared with proxy.hip); the teacher is read at the student's selection.
// The shape is proxy_ce_kernel's: one 256-lane workgroup per row, lane t takes the columns t + 256 k, fixed-order
// reductions, no atomics, plain C++ and vector stores.  The student's row and the flags sit in LDS as in proxy.hip; the
// teacher's row stays in global memory (as both rows do in softce.hip), so GRL_PROXY_MAX_P and the LDS budget are
// proxy.hip's.  With w_soft = 0 the teacher's row is never read and every intermediate is proxy_ce_kernel's, bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grl_hip.h"
#include "common.h"
#include "proxy_common.h"
#include "ce_finish.h"

namespace {

// One workgroup per row.  Every branch on `own`, k, w or a block total is uniform across the workgroup.  dlogits comes
// out WITHOUT the 1 / nv of the contract (ce_finish_kernel applies it): a row does not know the other rows' validity.
__global__ __launch_bounds__(256) void soft_proxy_ce_kernel(const float* __restrict__ z, int64_t ld,
                                                            const float* __restrict__ tz, int64_t ldt,
                                                            const int64_t* __restrict__ labels,
                                                            const int64_t* __restrict__ cams,
                                                            const int32_t* __restrict__ pcl,
                                                            const int32_t* __restrict__ pcm, float w, float omw, int n,
                                                            int P, int k_neg, float w_intra, float w_inter,
                                                            float* __restrict__ rows,      // [3][n]: loss, hit, valid
                                                            float* __restrict__ dz, int64_t ldd,
                                                            int64_t* __restrict__ own_out, int32_t* __restrict__ negsel) {
    extern __shared__ __attribute__((aligned(16))) float sz[];         // [P] the row, then [P] bytes of flags
    __shared__ float red[16];
    __shared__ int redi[4];
    __shared__ int cnt_gt[PROXY_MAX_TRIPS * 4], cnt_eq[PROXY_MAX_TRIPS * 4];
    unsigned char* fl = reinterpret_cast<unsigned char*>(sz + P);
    const int i = blockIdx.x, tid = threadIdx.x;
    const int64_t y = labels[i];

    // ---- the student's row, its flags, own proxy and selected negatives: proxy_ce_kernel's (proxy_common.h) ----
    const ProxyLds lds = {sz, fl, red, redi, cnt_gt, cnt_eq};
    const ProxySel sel = proxy_select(z + (int64_t)i * ld, y, cams[i], pcl, pcm, i, P, k_neg, lds, negsel);
    const int own = sel.own;
    if (own == PROXY_NONE) {                              // invalid row: the noise label, or a pair without a proxy
        proxy_invalid_row(rows, n, i, P, k_neg, dz, ldd, own_out, negsel);
        return;
    }
    const float mxA = sel.mxA;
    const bool soft = w != 0.f;

    // ---- the student's two cross entropies: proxy_ce_kernel term for term ----
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

    // ---- the teacher at the student's sets: q^A = softmax_A(t), q^U = softmax_U(t), and the two cross terms ----
    const float* ti = soft ? tz + (int64_t)i * ldt : nullptr;
    float mtA = 0.f, mtU = 0.f, ltA = 0.f, ltU = 0.f, crossA = 0.f, crossU = 0.f;
    if (soft) {
        float a = -INFINITY, u = -INFINITY;
        for (int j = tid; j < P; j += 256) {
            const unsigned f = fl[j];
            const float t = ti[j];
            if (f & F_A) a = fmaxf(a, t);
            if (f & (F_POS | F_NEG)) u = fmaxf(u, t);
        }
        mtA = block_max(a, red);
        mtU = block_max(u, red);
        float s2A = 0.f, s2U = 0.f;
        for (int j = tid; j < P; j += 256) {
            const unsigned f = fl[j];
            const float t = ti[j];
            if (f & F_A) s2A += expf(t - mtA);
            if (f & (F_POS | F_NEG)) s2U += expf(t - mtU);
        }
        ltA = logf(block_sum(s2A, red));
        ltU = logf(block_sum(s2U, red));
        float xA = 0.f, xU = 0.f;
        for (int j = tid; j < P; j += 256) {
            const unsigned f = fl[j];
            const float t = ti[j], v = sz[j];
            if (f & F_A) xA += expf(t - mtA - ltA) * (v - mxA);
            if (f & (F_POS | F_NEG)) xU += expf(t - mtU - ltU) * (v - mxU);
        }
        crossA = block_sum(xA, red);
        crossU = block_sum(xU, red);
    }

    if (dz) {
        float* di = dz + (int64_t)i * ldd;
        for (int j = tid; j < P; j += 256) {
            const unsigned f = fl[j];
            const float v = sz[j];
            float ga = 0.f, gu = 0.f;
            if (f & F_A) {
                float g = expf(v - mxA - lseA) - omw * (j == own ? 1.f : 0.f);
                if (soft) g = g - w * expf(ti[j] - mtA - ltA);
                ga = w_intra * g;
            }
            if (f & (F_POS | F_NEG)) {
                float g = expf(v - mxU - lseU) - omw * ((f & F_POS) ? ipos : 0.f);
                if (soft) g = g - w * expf(ti[j] - mtU - ltU);
                gu = w_inter * g;
            }
            di[j] = ga + gu;
        }
    }
    if (tid == 0) {
        float LA = lseA - omw * (sz[own] - mxA), LU = lseU - omw * (sP * ipos);
        if (soft) { LA = LA - w * crossA; LU = LU - w * crossU; }
        rows[i] = w_intra * LA + w_inter * LU;
        rows[n + i] = (sel.arg < P && (int64_t)pcl[sel.arg] == y) ? 1.f : 0.f;      // (a row of NaN has no arg-max)
        rows[2 * n + i] = 1.f;
        if (own_out) own_out[i] = own;
    }
}

}  // namespace

extern "C" int grl_soft_proxy_ce(const float* logits, int64_t ld, const float* tlogits, int64_t ldt, const int64_t* labels,
                                 const int64_t* cams, const int32_t* proxy_cluster, const int32_t* proxy_cam, float w_soft,
                                 int n, int P, int k_neg, float w_intra, float w_inter, float* loss, float* correct,
                                 float* dlogits, int64_t ldd, int64_t* own, int32_t* negsel, float* ws, void* stream) {
    GRL_REQUIRE(logits && labels && cams && proxy_cluster && proxy_cam && loss && ws,
                "soft_proxy_ce: a required pointer is NULL");
    GRL_REQUIRE(n > 0 && P > 0 && ld >= P, "soft_proxy_ce: bad args (n >= 1, P >= 1, ld >= P)");
    GRL_REQUIRE(P <= GRL_PROXY_MAX_P, "soft_proxy_ce: more than GRL_PROXY_MAX_P = 8192 proxies");
    GRL_REQUIRE(k_neg >= 0 && k_neg <= P, "soft_proxy_ce: k_neg outside 0 .. P");
    GRL_REQUIRE(!dlogits || ldd >= P, "soft_proxy_ce: ldd < P");
    GRL_REQUIRE(w_soft >= 0.f && w_soft <= 1.f, "soft_proxy_ce: w_soft outside [0, 1]");
    GRL_REQUIRE(w_soft == 0.f || (tlogits && ldt >= P), "soft_proxy_ce: w_soft != 0 needs tlogits with ldt >= P");
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)P * sizeof(float) + (size_t)((P + 3) & ~3);
    hipLaunchKernelGGL(soft_proxy_ce_kernel, dim3(n), dim3(256), lds, s, logits, ld, tlogits, ldt, labels, cams,
                       proxy_cluster, proxy_cam, w_soft, 1.f - w_soft, n, P, k_neg, w_intra, w_inter, ws, dlogits, ldd, own,
                       k_neg > 0 ? negsel : nullptr);
    hipLaunchKernelGGL(ce_finish_kernel, dlogits ? dim3(grl_ceil_div(P, 1024), n) : dim3(1), dim3(256), 0, s, ws, n, P,
                       loss, correct, dlogits, ldd);
    return grl_check_launch("grl_soft_proxy_ce");
}
