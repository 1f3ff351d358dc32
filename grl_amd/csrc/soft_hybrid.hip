// Hybrid-memory cross entropy against a hard class blended with a teacher's softmax over the same classes
// (grl_amd/reid/loss/soft_hybrid_memory.py; SpCL, Ge et al. 2020 with MMT's soft target, Ge et al. 2020):
// hybrid.hip's classes -- sets of columns, a class's logit the mean of its members' -- and softce.hip's target.  Loss,
// gradient and top-1 hit from one call.
// The shape is hybrid_ce_kernel's, and the student's pass IS hybrid_ce_kernel's (hybrid_common.h): one 256-lane workgroup
// per row, lane t takes the classes t + 256 k, the same fixed-order reductions, no atomics, plain C++ and vector stores.
// The student's class logits fill the LDS budget, so the teacher's go to caller-provided scratch (C floats per row): lane
// t writes and reads back the entries t + 256 k only -- no other lane ever touches them, so no barrier orders them.  With
// w_soft = 0 the teacher's row and the scratch are never touched and every intermediate is hybrid_ce_kernel's, bit for bit;
// with singleton classes in identity order every intermediate is soft_ce_kernel's (softce.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grl_hip.h"
#include "common.h"
#include "hybrid_common.h"
#include "ce_finish.h"

namespace {

// One workgroup per row.  The branches on the target and on w are uniform across the workgroup.  dlogits comes out WITHOUT
// the 1 / nv of the contract (ce_finish_kernel applies it): a row does not know the other rows' validity.
__global__ __launch_bounds__(256) void soft_hybrid_ce_kernel(const float* __restrict__ z, int64_t ld,
                                                             const float* __restrict__ tz, int64_t ldt,
                                                             const int64_t* __restrict__ targets,
                                                             const int32_t* __restrict__ cptr,
                                                             const int32_t* __restrict__ cmem,
                                                             const int32_t* __restrict__ icls, float w, float omw, int n,
                                                             int N, int C,
                                                             float* __restrict__ rows,     // [3][n]: loss, hit, valid
                                                             float* tcl,                   // [n][C] teacher scratch (w != 0)
                                                             float* __restrict__ dz, int64_t ldd) {
    extern __shared__ __attribute__((aligned(16))) float sz[];         // [C] the class logits, then the class gradients
    __shared__ float red[16];
    __shared__ int arg_s[4];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int64_t y = targets[i];
    if (y < 0 || y >= C) {                                // invalid row
        hyb_invalid_row(rows, n, i, dz, ldd, N);
        return;
    }
    const bool soft = w != 0.f;

    // ---- the student's classes: hybrid_ce_kernel term for term ----
    const HybRow r = hyb_student_pass(z + (int64_t)i * ld, cptr, cmem, C, sz, red, arg_s);
    const float mx = r.mx, lse = r.lse;
    const float zy = sz[y];

    // ---- the teacher's classes: q = softmax_C(t), and the cross term sum_c q_c (z_c - mx); q stays in the scratch ----
    float cross = 0.f;
    float* tq = soft ? tcl + (int64_t)i * C : nullptr;
    if (soft) {
        const float* ti = tz + (int64_t)i * ldt;
        float m2 = -INFINITY;
        for (int c = tid; c < C; c += 256) {
            const float v = hyb_class_logit(ti, cptr, cmem, c);
            tq[c] = v;
            m2 = fmaxf(m2, v);
        }
        const float mt = block_max(m2, red);
        float s2 = 0.f;
        for (int c = tid; c < C; c += 256) s2 += expf(tq[c] - mt);
        const float lt = logf(block_sum(s2, red));
        float x = 0.f;
        for (int c = tid; c < C; c += 256) {
            const float q = expf(tq[c] - mt - lt);
            tq[c] = q;
            x += q * (sz[c] - mx);
        }
        cross = block_sum(x, red);
    }

    // ---- every class's gradient once, in place; then the columns look their class up ----
    if (dz) {
        __syncthreads();                                  // every lane holds zy
        for (int c = tid; c < C; c += 256) {
            const float p = expf(sz[c] - mx - lse);
            float g = p - omw * (c == (int)y ? 1.f : 0.f);
            if (soft) g = g - w * tq[c];
            sz[c] = g / (float)(cptr[c + 1] - cptr[c]);
        }
        __syncthreads();
        hyb_scatter(dz + (int64_t)i * ldd, sz, icls, N);
    }
    if (tid == 0) {
        float L = lse - omw * (zy - mx);
        if (soft) L = L - w * cross;
        rows[i] = L;
        rows[n + i] = r.arg == (int)y ? 1.f : 0.f;        // (a row of NaN has no arg-max)
        rows[2 * n + i] = 1.f;
    }
}

}  // namespace

extern "C" int grl_soft_hybrid_ce(const float* logits, int64_t ld, const float* tlogits, int64_t ldt,
                                  const int64_t* targets, const int32_t* class_ptr, const int32_t* class_members,
                                  const int32_t* inst_class, float w_soft, int n, int N, int C, float* loss, float* correct,
                                  float* dlogits, int64_t ldd, float* ws, void* stream) {
    GRL_REQUIRE(logits && targets && class_ptr && class_members && inst_class && loss && ws,
                "soft_hybrid_ce: a required pointer is NULL");
    GRL_REQUIRE(n > 0 && N > 0 && C > 0 && C <= N && ld >= N, "soft_hybrid_ce: bad args (n >= 1, 1 <= C <= N, ld >= N)");
    GRL_REQUIRE(C <= GRL_HYBRID_MAX_CLASSES, "soft_hybrid_ce: more than GRL_HYBRID_MAX_CLASSES = 15360 classes");
    GRL_REQUIRE(!dlogits || ldd >= N, "soft_hybrid_ce: ldd < N");
    GRL_REQUIRE(w_soft >= 0.f && w_soft <= 1.f, "soft_hybrid_ce: w_soft outside [0, 1]");
    GRL_REQUIRE(w_soft == 0.f || (tlogits && ldt >= N), "soft_hybrid_ce: w_soft != 0 needs tlogits with ldt >= N");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(soft_hybrid_ce_kernel, dim3(n), dim3(256), (size_t)C * sizeof(float), s, logits, ld, tlogits, ldt,
                       targets, class_ptr, class_members, inst_class, w_soft, 1.f - w_soft, n, N, C, ws, ws + 3 * (int64_t)n,
                       dlogits, ldd);
    hipLaunchKernelGGL(ce_finish_kernel, dlogits ? dim3(grl_ceil_div(N, 1024), n) : dim3(1), dim3(256), 0, s, ws, n, N,
                       loss, correct, dlogits, ldd);
    return grl_check_launch("grl_soft_hybrid_ce");
}
