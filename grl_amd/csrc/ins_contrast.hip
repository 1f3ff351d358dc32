// Hard instance contrast and soft instance consistency against a mean teacher (grl_amd/reid/loss/ins_contrast.py,
// DESIGN.md 4ao; the two instance terms of ICE, Chen et al. 2021).  With u_i = f_i / max(|f_i|, 1e-12) the student's rows,
// v_j = m_j / max(|m_j|, 1e-12) the teacher's, c_ij = <u_i, v_j> and t_ij = <v_i, v_j>, anchor i selects ONE column per
// distinct id of the batch -- of its own id (i included) the member with the smallest c_ij, the hard positive p_i, of every
// other id the member with the largest, the lowest column index among equal values -- and over that set K_i
//     P = softmax(c_ik / tau),   Q = softmax(t_ik / tau_t),   L_i = - w_hard log P_p - w_soft sum_k Q_k log P_k,
//     g_ik = dL_i / d(c_ik / tau) = w_hard (P_k - [k = p_i]) + w_soft (P_k - Q_k).
// The teacher carries no gradient, so dL_i / df depends on row i alone:
//     gu_i = (1 / tau) sum_k g_ik v_k,      df_i = dloss_i (gu_i - u_i <u_i, gu_i>) / max(|f_i|, 1e-12),
// and a row whose norm is under the clamp (|f_i| < 1e-12, a zero row) gets df_i = 0.
// Plain C++, no atomics, every sum in a fixed order (grl_hip.h states them): the same bits every run.  LDS is touched with
// 32-bit accesses only (the int64 ids live there as two int32 halves).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/grl_hip.h"
#include "common.h"

namespace {

constexpr int INS_MAX_N = 2048;         // forward LDS: 6 n words (5 n with w_soft = 0) = 48 KiB at the cap

// sum_k a_k b_k over D4 f32x4 by one wave, tri_wave_sqdist's shape: lane l takes the vectors l + 64 t, adds the four products of
// each left to right and its trips in sequence from 0, then the wave64 xor tree.  Every lane receives the sum.
__device__ __forceinline__ float ins_wave_dot(const f32x4* __restrict__ a, const f32x4* __restrict__ b, int D4, int lane) {
    float s = 0.f;
    for (int k = lane; k < D4; k += 64) {
        const f32x4 x = a[k], y = b[k];
        s += x[0] * y[0] + x[1] * y[1] + x[2] * y[2] + x[3] * y[3];
    }
    return wave_sum(s);
}

// F.normalize's clamp
__device__ __forceinline__ float ins_inv_norm(float ss) { return 1.f / fmaxf(sqrtf(ss), 1e-12f); }

// One workgroup per anchor.  SOFT = (w_soft != 0): without it the teacher's similarities t are never computed.
template <bool SOFT>
__global__ __launch_bounds__(256) void ins_fwd_kernel(const float* __restrict__ f, const float* __restrict__ tf,
                                                      const int64_t* __restrict__ ids, int n, int D, float tau, float tau_t,
                                                      float wh, float ws, float* __restrict__ loss, float* __restrict__ cosm,
                                                      int32_t* __restrict__ sel, float* __restrict__ coef) {
    extern __shared__ float lds[];
    float* crow = lds;                                  // [n] c_ij
    float* erow = crow + n;                             // [n] expf(c_ik / tau - max) on K_i, 0 elsewhere
    int* idlo = reinterpret_cast<int*>(erow + n);       // [n] the ids' low and
    int* idhi = idlo + n;                               // [n] high words
    int* flag = idhi + n;                               // [n] 0 / 1 / 2, what sel receives
    float* trow = reinterpret_cast<float*>(flag + n);   // [n] SOFT only: t_ij, then the teacher's exponentials, then Q_k nl_k
    __shared__ float red[16];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, D4 = D >> 2;
    const f32x4* fi = reinterpret_cast<const f32x4*>(f + (int64_t)i * D);
    const f32x4* mi = reinterpret_cast<const f32x4*>(tf + (int64_t)i * D);
    for (int j = tid; j < n; j += 256) {
        const int64_t y = ids[j];
        idlo[j] = (int)(uint32_t)y;
        idhi[j] = (int)(y >> 32);
    }
    // ---- the similarity row: one wave per column, four waves; the inverse norms are computed per workgroup ----
    const float invf = ins_inv_norm(ins_wave_dot(fi, fi, D4, lane));
    float invmi = 0.f;
    if (SOFT) invmi = ins_inv_norm(ins_wave_dot(mi, mi, D4, lane));
    for (int j = wave; j < n; j += 4) {
        const f32x4* mj = reinterpret_cast<const f32x4*>(tf + (int64_t)j * D);
        float sd = 0.f, sm = 0.f, st = 0.f;
        for (int k = lane; k < D4; k += 64) {
            const f32x4 y = mj[k], x = fi[k];
            sd += x[0] * y[0] + x[1] * y[1] + x[2] * y[2] + x[3] * y[3];
            sm += y[0] * y[0] + y[1] * y[1] + y[2] * y[2] + y[3] * y[3];
            if (SOFT) {
                const f32x4 z = mi[k];
                st += z[0] * y[0] + z[1] * y[1] + z[2] * y[2] + z[3] * y[3];
            }
        }
        sd = wave_sum(sd);
        const float invmj = ins_inv_norm(wave_sum(sm));
        if (SOFT) st = wave_sum(st);
        if (lane == 0) {
            const float c = (sd * invf) * invmj;
            crow[j] = c;
            cosm[(int64_t)i * n + j] = c;
            if (SOFT) trow[j] = (st * invmi) * invmj;
        }
    }
    __syncthreads();
    // ---- the selection: lane j decides whether column j is the winner of its id, over the LDS row ----
    const int ilo = idlo[i], ihi = idhi[i];
    float mx = -INFINITY, my = -INFINITY;
    for (int j = tid; j < n; j += 256) {
        const int ylo = idlo[j], yhi = idhi[j];
        const bool own = ylo == ilo && yhi == ihi;
        const float cj = crow[j];
        bool win = true;
        for (int o = 0; o < n; ++o) {
            if (idlo[o] != ylo || idhi[o] != yhi) continue;
            const float co = crow[o];
            if ((own ? co < cj : co > cj) || (co == cj && o < j)) win = false;
        }
        const int fl = win ? (own ? 2 : 1) : 0;
        flag[j] = fl;
        sel[(int64_t)i * n + j] = fl;
        if (fl) {
            mx = fmaxf(mx, cj / tau);
            if (SOFT) my = fmaxf(my, trow[j] / tau_t);
        }
    }
    mx = block_max(mx, red);
    if (SOFT) my = block_max(my, red);
    for (int j = tid; j < n; j += 256) {
        const int fl = flag[j];
        erow[j] = fl ? expf(crow[j] / tau - mx) : 0.f;
        if (SOFT) trow[j] = fl ? expf(trow[j] / tau_t - my) : 0.f;
    }
    __syncthreads();
    // ---- the two partition sums, ascending column index (the zeros outside K_i add exactly), by every lane ----
    float S = 0.f, T = 0.f;
    for (int k = 0; k < n; ++k) {
        S += erow[k];
        if (SOFT) T += trow[k];
    }
    const float logS = logf(S);
    __syncthreads();                                    // trow is overwritten below
    for (int j = tid; j < n; j += 256) {
        const int fl = flag[j];
        float g = 0.f, term = 0.f;
        if (fl) {
            const float P = erow[j] / S;
            g = wh * (P - (fl == 2 ? 1.f : 0.f));
            if (SOFT) {
                const float Q = trow[j] / T;
                g = g + ws * (P - Q);
                term = Q * (logS - (crow[j] / tau - mx));
            }
        }
        coef[(int64_t)i * n + j] = g;
        if (SOFT) trow[j] = term;
    }
    if (SOFT) __syncthreads();
    if (tid == 0) {
        int p = i;
        for (int k = 0; k < n; ++k)
            if (flag[k] == 2) p = k;
        const float hard = logS - (crow[p] / tau - mx);
        if (SOFT) {
            float A = 0.f;
            for (int k = 0; k < n; ++k) A += trow[k];
            loss[i] = wh * hard + ws * A;
        } else {
            loss[i] = wh * hard;
        }
    }
}

// One workgroup per row; every element of dfeat is written by one lane (first gu, then the result over it).
__global__ __launch_bounds__(256) void ins_bwd_kernel(const float* __restrict__ f, const float* __restrict__ tf,
                                                      const float* __restrict__ coef, const float* __restrict__ dloss, float tau,
                                                      float* df, int n, int D4) {
    extern __shared__ float wrow[];                     // [n] g_ik / max(|m_k|, 1e-12), 0 where g_ik = 0
    __shared__ float red[16];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const f32x4* fi = reinterpret_cast<const f32x4*>(f) + (int64_t)i * D4;
    const f32x4* M = reinterpret_cast<const f32x4*>(tf);
    f32x4* dfi = reinterpret_cast<f32x4*>(df) + (int64_t)i * D4;
    const float nf = sqrtf(ins_wave_dot(fi, fi, D4, lane));
    const float invf = 1.f / fmaxf(nf, 1e-12f);
    for (int k = wave; k < n; k += 4) {
        const float g = coef[(int64_t)i * n + k];       // wave-uniform
        float w = 0.f;
        if (g != 0.f) w = g * ins_inv_norm(ins_wave_dot(M + (int64_t)k * D4, M + (int64_t)k * D4, D4, lane));
        if (lane == 0) wrow[k] = w;
    }
    __syncthreads();
    const float rt = 1.f / tau, dl = dloss[i];
    float part = 0.f;
    for (int c = tid; c < D4; c += 256) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < n; ++k) {
            const float w = wrow[k];
            if (w != 0.f) acc += M[(int64_t)k * D4 + c] * w;        // workgroup-uniform
        }
        const f32x4 gu = acc * rt, u = fi[c] * invf;
        part += u[0] * gu[0] + u[1] * gu[1] + u[2] * gu[2] + u[3] * gu[3];
        dfi[c] = gu;
    }
    const float dot = block_sum(part, red);
    const bool clamped = nf < 1e-12f;                   // the norm is under F.normalize's clamp: no gradient
    for (int c = tid; c < D4; c += 256) {
        const f32x4 gu = dfi[c], u = fi[c] * invf;
        const f32x4 r = ((gu - u * dot) * invf) * dl;
        dfi[c] = clamped ? f32x4{0.f, 0.f, 0.f, 0.f} : r;
    }
}

bool ins_temp_ok(float t) { return t > 0.f && isfinite(t); }

}  // namespace

extern "C" int grl_ins_contrast_fwd(const float* feat, const float* tfeat, const int64_t* ids, int n, int D, float tau,
                                    float tau_t, float w_hard, float w_soft, float* loss, float* cos, int32_t* sel,
                                    float* coef, void* stream) {
    GRL_REQUIRE(feat && tfeat && ids && loss && cos && sel && coef, "ins_contrast_fwd: NULL pointer");
    GRL_REQUIRE(n >= 1 && n <= INS_MAX_N && D >= 4 && D % 4 == 0, "ins_contrast_fwd: bad shape (1 <= n <= 2048, D >= 4, D % 4)");
    GRL_REQUIRE(ins_temp_ok(tau) && ins_temp_ok(tau_t), "ins_contrast_fwd: tau and tau_t must be finite and > 0");
    GRL_REQUIRE(w_hard >= 0.f && w_soft >= 0.f && isfinite(w_hard) && isfinite(w_soft) && (w_hard > 0.f || w_soft > 0.f),
                "ins_contrast_fwd: the weights must be finite, >= 0 and not both 0");
    const bool soft = w_soft != 0.f;
    const size_t lds = (size_t)(soft ? 6 : 5) * n * sizeof(float);
    if (soft)
        hipLaunchKernelGGL((ins_fwd_kernel<true>), dim3(n), dim3(256), lds, (hipStream_t)stream, feat, tfeat, ids, n, D, tau,
                           tau_t, w_hard, w_soft, loss, cos, sel, coef);
    else
        hipLaunchKernelGGL((ins_fwd_kernel<false>), dim3(n), dim3(256), lds, (hipStream_t)stream, feat, tfeat, ids, n, D, tau,
                           tau_t, w_hard, w_soft, loss, cos, sel, coef);
    return grl_check_launch("grl_ins_contrast_fwd");
}

extern "C" int grl_ins_contrast_bwd(const float* feat, const float* tfeat, const float* coef, const float* dloss, float tau,
                                    float* dfeat, int n, int D, void* stream) {
    GRL_REQUIRE(feat && tfeat && coef && dloss && dfeat, "ins_contrast_bwd: NULL pointer");
    GRL_REQUIRE(n >= 1 && n <= INS_MAX_N && D >= 4 && D % 4 == 0, "ins_contrast_bwd: bad shape (1 <= n <= 2048, D >= 4, D % 4)");
    GRL_REQUIRE(ins_temp_ok(tau), "ins_contrast_bwd: tau must be finite and > 0");
    hipLaunchKernelGGL(ins_bwd_kernel, dim3(n), dim3(256), (size_t)n * sizeof(float), (hipStream_t)stream, feat, tfeat, coef,
                       dloss, tau, dfeat, n, D / 4);
    return grl_check_launch("grl_ins_contrast_bwd");
}
