// Cross entropy against a hard label blended with a teacher's softmax (grl_amd/reid/loss/soft_memory.py, DESIGN.md 4al;
// Mean Teacher, Tarvainen & Valpola 2017; MMT, Ge et al. 2020): the student's and the teacher's scaled similarities to
// the same memory rows, loss, gradient and top-1 hit from one call.
// The shape is softmax_ce_kernel's (loss.hip): one 256-lane workgroup per row, lane t takes the columns t + 256 k, the
// same fixed-order reductions, no atomics, plain C++ and vector stores -- with w_soft = 0 the teacher's row is never read
// and every intermediate is softmax_ce_kernel's, bit for bit.  Both rows stay in global memory: c has no limit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grl_hip.h"
#include "common.h"
#include "ce_finish.h"

namespace {

// One workgroup per row.  The branches on the label and on w are uniform across the workgroup.  dlogits comes out WITHOUT
// the 1 / nv of the contract (ce_finish_kernel applies it): a row does not know the other rows' validity.
__global__ __launch_bounds__(256) void soft_ce_kernel(const float* __restrict__ z, int64_t ld,
                                                      const float* __restrict__ tz, int64_t ldt,
                                                      const int64_t* __restrict__ labels, float w, float omw, int n, int c,
                                                      float* __restrict__ rows,        // [3][n]: loss, hit, valid
                                                      float* __restrict__ dz, int64_t ldd) {
    __shared__ float red[16];
    __shared__ int arg_s[4];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int64_t y = labels[i];
    if (y < 0 || y >= c) {                                // invalid row
        if (dz)
            for (int j = tid; j < c; j += 256) dz[(int64_t)i * ldd + j] = 0.f;
        if (tid == 0) { rows[i] = 0.f; rows[n + i] = 0.f; rows[2 * n + i] = 0.f; }
        return;
    }
    const float* zi = z + (int64_t)i * ld;
    const bool soft = w != 0.f;
    const float* ti = soft ? tz + (int64_t)i * ldt : nullptr;

    // ---- the student's row: softmax_ce_kernel term for term ----
    float m = -INFINITY;
    int am = 0x7fffffff;
    for (int j = tid; j < c; j += 256) {
        const float v = zi[j];
        if (v > m) { m = v; am = j; }
    }
    const float mx = block_max(m, red);
    int cand = (m == mx) ? am : 0x7fffffff;               // first index attaining the maximum
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o));
    if ((tid & 63) == 0) arg_s[tid >> 6] = cand;
    float s = 0.f;
    for (int j = tid; j < c; j += 256) s += expf(zi[j] - mx);
    s = block_sum(s, red);                                // (its barriers also publish arg_s)
    const int arg = min(min(arg_s[0], arg_s[1]), min(arg_s[2], arg_s[3]));
    const float lse = logf(s);                            // of the shifted row

    // ---- the teacher's row: q = softmax(t), and the cross term sum_j q_j (z_j - mx) ----
    float mt = 0.f, lt = 0.f, cross = 0.f;
    if (soft) {
        float m2 = -INFINITY;
        for (int j = tid; j < c; j += 256) m2 = fmaxf(m2, ti[j]);
        mt = block_max(m2, red);
        float s2 = 0.f;
        for (int j = tid; j < c; j += 256) s2 += expf(ti[j] - mt);
        lt = logf(block_sum(s2, red));
        float x = 0.f;
        for (int j = tid; j < c; j += 256) x += expf(ti[j] - mt - lt) * (zi[j] - mx);
        cross = block_sum(x, red);
    }

    if (dz) {
        float* di = dz + (int64_t)i * ldd;
        for (int j = tid; j < c; j += 256) {
            const float p = expf(zi[j] - mx - lse);
            float g = p - omw * (j == (int)y ? 1.f : 0.f);
            if (soft) g = g - w * expf(ti[j] - mt - lt);
            di[j] = g;
        }
    }
    if (tid == 0) {
        float L = lse - omw * (zi[y] - mx);
        if (soft) L = L - w * cross;
        rows[i] = L;
        rows[n + i] = arg == (int)y ? 1.f : 0.f;          // (a row of NaN has no arg-max)
        rows[2 * n + i] = 1.f;
    }
}

}  // namespace

extern "C" int grl_soft_ce(const float* logits, int64_t ld, const float* tlogits, int64_t ldt, const int64_t* labels,
                           float w_soft, int n, int c, float* loss, float* correct, float* dlogits, int64_t ldd,
                           float* ws, void* stream) {
    GRL_REQUIRE(logits && labels && loss && ws, "soft_ce: a required pointer is NULL");
    GRL_REQUIRE(n > 0 && c > 0 && ld >= c, "soft_ce: bad args (n >= 1, c >= 1, ld >= c)");
    GRL_REQUIRE(!dlogits || ldd >= c, "soft_ce: ldd < c");
    GRL_REQUIRE(w_soft >= 0.f && w_soft <= 1.f, "soft_ce: w_soft outside [0, 1]");
    GRL_REQUIRE(w_soft == 0.f || (tlogits && ldt >= c), "soft_ce: w_soft != 0 needs tlogits with ldt >= c");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(soft_ce_kernel, dim3(n), dim3(256), 0, s, logits, ld, tlogits, ldt, labels, w_soft, 1.f - w_soft, n,
                       c, ws, dlogits, ldd);
    hipLaunchKernelGGL(ce_finish_kernel, dlogits ? dim3(grl_ceil_div(c, 1024), n) : dim3(1), dim3(256), 0, s, ws, n, c,
                       loss, correct, dlogits, ldd);
    return grl_check_launch("grl_soft_ce");
}
