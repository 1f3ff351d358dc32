// Batch-hard soft-margin triplet loss blended with a mean teacher's soft target (grl_amd/reid/loss/soft_triplet.py,
// DESIGN.md 4am; MMT's SoftTripletLoss, Ge et al. 2020).  With z_i = d(i,p_i) - d(i,n_i) from the STUDENT's batch-hard
// selection and t_i the same difference of the TEACHER's distances at the student's indices, MMT's
// (1 - w) L_hard + w L_soft is
//     L_i = log(1 + exp(z_i)) - w sigmoid(t_i) z_i,        dL_i / dz_i = sigmoid(z_i) - w sigmoid(t_i).
// The shape is triplet_fwd_kernel's / triplet_bwd_kernel's (loss.hip): the distance row, the selection and the backward's
// gather are triplet_common.h's, so dist, sel and z are grl_triplet_fwd's bit for bit, and with w_soft = 0 the teacher's
// rows and q are never touched and loss and dfeat are too.  Plain C++, no atomics, fixed order: the same bits every run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grl_hip.h"
#include "common.h"
#include "triplet_common.h"

namespace {

// One workgroup per anchor.  The branch on w is uniform across the grid.
__global__ __launch_bounds__(256) void soft_triplet_fwd_kernel(const float* __restrict__ f, const float* __restrict__ tf,
                                                               const int64_t* __restrict__ ids, int n, int D, float w,
                                                               float* __restrict__ loss, float* __restrict__ dist,
                                                               int32_t* __restrict__ sel, float* __restrict__ zout,
                                                               float* __restrict__ qout) {
    extern __shared__ float drow[];                    // [n]
    __shared__ int pick[2];                            // jp, jn
    __shared__ float td[2];                            // td(i, jp), td(i, jn)
    const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    tri_dist_row(f, i, n, D, drow, dist);
    __syncthreads();
    // ---- the student's part: triplet_fwd_kernel (soft = 1) term for term ----
    TriSel s;
    if (threadIdx.x == 0) {
        s = tri_select(drow, ids, i, n);
        zout[i] = s.z;
        sel[2 * i] = s.has_pos ? s.jp : -1;
        sel[2 * i + 1] = s.jn;
        if (w == 0.f) loss[i] = logf(1.f + expf(s.z));
        pick[0] = s.jp;
        pick[1] = s.jn;
    }
    if (w == 0.f) return;
    __syncthreads();
    // ---- the teacher's two distances at the student's indices: wave 0 takes jp, wave 1 takes jn ----
    if (wave < 2) {
        const int j = pick[wave];
        const float sq = tri_wave_sqdist(reinterpret_cast<const f32x4*>(tf + (int64_t)i * D),
                                         reinterpret_cast<const f32x4*>(tf + (int64_t)j * D), D >> 2, lane);
        if (lane == 0) td[wave] = tri_dist_of(sq);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // the student's masks mirrored: no positive -> 0, a same-id "negative" -> + 1e5
        const float tp = s.has_pos ? td[0] : 0.f;
        const float tn = td[1] + 1e5f * (ids[s.jn] == ids[i] ? 1.f : 0.f);
        const float t = tp - tn;
        const float q = 1.f / (1.f + expf(-t));        // finite at both ends: t = -1e5 gives 0
        qout[i] = q;
        const float wq = w * q;
        loss[i] = logf(1.f + expf(s.z)) - wq * s.z;
    }
}

__global__ __launch_bounds__(256) void soft_triplet_bwd_kernel(const float* __restrict__ f, const float* __restrict__ dist,
                                                               const int32_t* __restrict__ sel,
                                                               const float* __restrict__ z, const float* __restrict__ q,
                                                               const float* __restrict__ dloss, float w,
                                                               float* __restrict__ df, int n, int D4) {
    tri_bwd_rows(f, dist, sel, df, n, D4, [&](int i) {
        const float ez = expf(z[i]);
        const float sg = ez / (1.f + ez);
        if (w == 0.f) return dloss[i] * sg;
        const float wq = w * q[i];
        return dloss[i] * (sg - wq);
    });
}

}  // namespace

extern "C" int grl_soft_triplet_fwd(const float* feat, const float* tfeat, const int64_t* ids, int n, int D, float w_soft,
                                    float* loss, float* dist, int32_t* sel, float* z, float* q, void* stream) {
    GRL_REQUIRE(feat && ids && loss && dist && sel && z && n > 0 && n <= 16384 && D > 0 && D % 4 == 0,
                "soft_triplet_fwd: bad args (D % 4, n <= 16384)");
    GRL_REQUIRE(w_soft >= 0.f && w_soft <= 1.f, "soft_triplet_fwd: w_soft outside [0, 1]");
    GRL_REQUIRE(w_soft == 0.f || (tfeat && q), "soft_triplet_fwd: w_soft != 0 needs tfeat and q");
    hipLaunchKernelGGL(soft_triplet_fwd_kernel, dim3(n), dim3(256), (size_t)n * sizeof(float), (hipStream_t)stream, feat,
                       tfeat, ids, n, D, w_soft, loss, dist, sel, z, q);
    return grl_check_launch("grl_soft_triplet_fwd");
}

extern "C" int grl_soft_triplet_bwd(const float* feat, const float* dist, const int32_t* sel, const float* z,
                                    const float* q, const float* dloss, float w_soft, float* dfeat, int n, int D,
                                    void* stream) {
    GRL_REQUIRE(feat && dist && sel && z && dloss && dfeat && n > 0 && n <= 16384 && D > 0 && D % 4 == 0,
                "soft_triplet_bwd: bad args (D % 4, n <= 16384)");
    GRL_REQUIRE(w_soft >= 0.f && w_soft <= 1.f, "soft_triplet_bwd: w_soft outside [0, 1]");
    GRL_REQUIRE(w_soft == 0.f || q, "soft_triplet_bwd: w_soft != 0 needs q");
    hipLaunchKernelGGL(soft_triplet_bwd_kernel, dim3(grl_ceil_div(D / 4, 256), n), dim3(256), 0, (hipStream_t)stream, feat,
                       dist, sel, z, q, dloss, w_soft, dfeat, n, D / 4);
    return grl_check_launch("grl_soft_triplet_bwd");
}
