// Hybrid-memory cross entropy of self-paced unsupervised training (grl_amd/reid/loss/hybrid_memory.py, DESIGN.md 4ak;
// SpCL, Ge et al. 2020): the columns of a logits row are the rows of an INSTANCE memory, the classes of the cross entropy
// are sets of columns -- the clusters, and every unclustered instance as a class of its own -- and a class's logit is the
// mean of its members' logits.  Loss, gradient and top-1 hit from one call.
// The shape is softmax_ce_kernel's (loss.hip) with classes in the place of columns: one 256-lane workgroup per row, lane t
// takes the classes t + 256 k, the same fixed-order reductions, no atomics, plain C++ and vector stores -- with singleton
// classes in identity order every intermediate is softmax_ce_kernel's, bit for bit.  The class logits sit in LDS (4 C
// bytes <= 60 KB); the logits row stays in global memory and every logit is read once, through the CSR table.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grl_hip.h"
#include "common.h"
#include "hybrid_common.h"
#include "ce_finish.h"

namespace {

// One workgroup per row.  The branch on the target is uniform across the workgroup.  dlogits comes out WITHOUT the 1 / nv
// of the contract (ce_finish_kernel applies it): a row does not know the other rows' validity.
__global__ __launch_bounds__(256) void hybrid_ce_kernel(const float* __restrict__ z, int64_t ld,
                                                        const int64_t* __restrict__ targets,
                                                        const int32_t* __restrict__ cptr, const int32_t* __restrict__ cmem,
                                                        const int32_t* __restrict__ icls, int n, int N, int C,
                                                        float* __restrict__ rows,      // [3][n]: loss, hit, valid
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

    // ---- pass A: the class logits, their maximum, arg-max and lse (hybrid_common.h) ----
    const HybRow r = hyb_student_pass(z + (int64_t)i * ld, cptr, cmem, C, sz, red, arg_s);
    const float mx = r.mx, lse = r.lse;
    const float zy = sz[y];

    // ---- pass B: every class's gradient once, in place; then the columns look their class up ----
    if (dz) {
        __syncthreads();                                  // every lane holds zy
        for (int c = tid; c < C; c += 256) {
            const float p = expf(sz[c] - mx - lse);
            sz[c] = (p - (c == (int)y ? 1.f : 0.f)) / (float)(cptr[c + 1] - cptr[c]);
        }
        __syncthreads();
        hyb_scatter(dz + (int64_t)i * ldd, sz, icls, N);
    }
    if (tid == 0) {
        rows[i] = lse - (zy - mx);
        rows[n + i] = r.arg == (int)y ? 1.f : 0.f;        // (a row of NaN has no arg-max)
        rows[2 * n + i] = 1.f;
    }
}

}  // namespace

extern "C" int grl_hybrid_ce(const float* logits, int64_t ld, const int64_t* targets, const int32_t* class_ptr,
                             const int32_t* class_members, const int32_t* inst_class, int n, int N, int C, float* loss,
                             float* correct, float* dlogits, int64_t ldd, float* ws, void* stream) {
    GRL_REQUIRE(logits && targets && class_ptr && class_members && inst_class && loss && ws,
                "hybrid_ce: a required pointer is NULL");
    GRL_REQUIRE(n > 0 && N > 0 && C > 0 && C <= N && ld >= N, "hybrid_ce: bad args (n >= 1, 1 <= C <= N, ld >= N)");
    GRL_REQUIRE(C <= GRL_HYBRID_MAX_CLASSES, "hybrid_ce: more than GRL_HYBRID_MAX_CLASSES = 15360 classes");
    GRL_REQUIRE(!dlogits || ldd >= N, "hybrid_ce: ldd < N");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(hybrid_ce_kernel, dim3(n), dim3(256), (size_t)C * sizeof(float), s, logits, ld, targets, class_ptr,
                       class_members, inst_class, n, N, C, ws, dlogits, ldd);
    hipLaunchKernelGGL(ce_finish_kernel, dlogits ? dim3(grl_ceil_div(N, 1024), n) : dim3(1), dim3(256), 0, s, ws, n, N,
                       loss, correct, dlogits, ldd);
    return grl_check_launch("grl_hybrid_ce");
}
