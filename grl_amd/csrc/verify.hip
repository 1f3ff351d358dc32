// Ranking by the Siamese verification head (engine.verify_metric / verify_dist).  In eval mode the head
// BatchNorm1d -> Linear on (p - g)^2 is affine in (p - g)^2, so the class-1 minus class-0 logit is one weighted squared
// distance s(p, g) = sum_d w_d (p_d - g_d)^2 + c, and the blend F = (1 - beta)(-q.g) + beta(-s) is
//     F(q, g) = -q'.g - (rq + rg),   rq = beta (a_q + c),  rg = beta a_g,  a_x = sum_d w_d x_d^2 over the head's slice,
// with q' = (1 - beta) q outside the slice and ((1 - beta) - 2 beta w) q inside.  -q'.g is the existing NEGDOT GEMM;
// this file holds the three small passes around it: the fold (w, c), the row terms (a_x, q') and the finish.
//
// Rounding contract.  fold and rows compute in fp64 and round once to fp32 where they store fp32; every fp64 sum has a
// fixed order that does not depend on the launch geometry (a lane's elements in ascending d, then a tree of fixed
// shape).  finish is two fp32 operations per entry, s = rq + rg, then D - s, and reads nothing but the entry itself.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grl_hip.h"
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int FOLD_THREADS = 256;
constexpr int ROWS_THREADS = 256;                               // 4 waves: one feature row per wave
constexpr int FINISH_THREADS = 256;
constexpr int FINISH_COLS = FINISH_THREADS * 4;                 // columns of one row per workgroup

// One workgroup.  Thread t owns d = t, t + 256, ... (ascending); the 256 partial sums of c meet in an LDS tree of
// fixed shape (128, 64, ..., 1), so c has one value whatever the device.
__global__ __launch_bounds__(FOLD_THREADS) void verify_fold_kernel(const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta,
                                                                   const float* __restrict__ mean,
                                                                   const float* __restrict__ var, double eps,
                                                                   const float* __restrict__ W,
                                                                   const float* __restrict__ b, int D,
                                                                   float* __restrict__ w, double* __restrict__ c64,
                                                                   float* __restrict__ c32) {
    __shared__ double red[FOLD_THREADS];
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int d = t; d < D; d += FOLD_THREADS) {
        const double dw = (double)W[D + d] - (double)W[d];
        const double sd = sqrt((double)var[d] + eps);
        const double g = (double)gamma[d];
        w[d] = (float)(dw * g / sd);
        acc = acc + dw * ((double)beta[d] - g * (double)mean[d] / sd);
    }
    red[t] = acc;
    __syncthreads();
    for (int s = FOLD_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = red[t] + red[t + s];
        __syncthreads();
    }
    if (t == 0) {
        const double c = red[0] + (double)b[1] - (double)b[0];
        *c64 = c;
        *c32 = (float)c;
    }
}

// One wave per row.  Lane l owns the 4 consecutive slice elements 4 (l + 64 j), j = 0, 1, ...: per element
// acc = acc + w * (x * x) in fp64 (x * x is exact there), ascending d; the 64 lane sums meet in an xor tree
// (32, 16, ..., 1), in which every lane adds the same pairs.  r = fp32(beta * (sum + c)), c = 0 without `c64`.
// With `qout` the lane also stores the modified query elements, each computed in fp64 and rounded once:
// ((1 - beta) - 2 beta w) x inside the slice -- at column col0 + e of a full-width row (FULL), at column e of a
// Dv-wide row otherwise -- and, FULL only, (1 - beta) x outside the slice.
template <bool FULL>
__global__ __launch_bounds__(ROWS_THREADS) void verify_rows_kernel(const float* __restrict__ x, int64_t ldx, int n,
                                                                   int d, int col0, int Dv,
                                                                   const float* __restrict__ w, double beta,
                                                                   const double* __restrict__ c64,
                                                                   float* __restrict__ r, float* __restrict__ qout,
                                                                   int64_t ldq) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (ROWS_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= n) return;                                       // whole waves leave: no shuffle below is cut
    const float* xr = x + row * ldx;
    float* qr = qout ? qout + row * ldq : nullptr;
    const double keep = 1.0 - beta, twob = 2.0 * beta;
    double acc = 0.0;
    for (int e = lane * 4; e < Dv; e += 64 * 4) {
        const float4 xv = *reinterpret_cast<const float4*>(xr + col0 + e);
        const float4 wv = *reinterpret_cast<const float4*>(w + e);
        const double x0 = xv.x, x1 = xv.y, x2 = xv.z, x3 = xv.w;
        const double w0 = wv.x, w1 = wv.y, w2 = wv.z, w3 = wv.w;
        acc = acc + w0 * (x0 * x0);
        acc = acc + w1 * (x1 * x1);
        acc = acc + w2 * (x2 * x2);
        acc = acc + w3 * (x3 * x3);
        if (qr) {
            float4 o;
            o.x = (float)((keep - twob * w0) * x0);
            o.y = (float)((keep - twob * w1) * x1);
            o.z = (float)((keep - twob * w2) * x2);
            o.w = (float)((keep - twob * w3) * x3);
            *reinterpret_cast<float4*>(qr + (FULL ? col0 : 0) + e) = o;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o);
    if (lane == 0) r[row] = (float)(beta * (acc + (c64 ? *c64 : 0.0)));
    if (FULL && qr) {
        const int rest = d - Dv;                                // columns outside the slice, in row order
        for (int e = lane * 4; e < rest; e += 64 * 4) {
            const int col = e < col0 ? e : e + Dv;
            const float4 xv = *reinterpret_cast<const float4*>(xr + col);
            float4 o;
            o.x = (float)(keep * (double)xv.x);
            o.y = (float)(keep * (double)xv.y);
            o.z = (float)(keep * (double)xv.z);
            o.w = (float)(keep * (double)xv.w);
            *reinterpret_cast<float4*>(qr + col) = o;
        }
    }
}

// D[q][j] = D[q][j] - (rq[q] + rg[c0 + j]) in place, j < n.  blockIdx.y walks the rows (grid-stride), blockIdx.x the
// 1024-column chunks of a row.  A row starts `head` elements before its first 16-byte boundary (ld need not be a
// multiple of 4: a ragged last block has ld = n); those and the ragged end go element by element, the rest in
// 16-byte accesses.  rg is read 16 bytes at a time when rg + c0 + j falls on a boundary too.
__global__ __launch_bounds__(FINISH_THREADS) void verify_finish_kernel(float* __restrict__ D, int64_t ld, int nq, int n,
                                                                       const float* __restrict__ rq,
                                                                       const float* __restrict__ rg, int64_t c0) {
    const float* rgc = rg + c0;
    for (int q = blockIdx.y; q < nq; q += gridDim.y) {
        float* row = D + (int64_t)q * ld;
        const float a = rq[q];
        int head = (int)((4u - (unsigned)(((uintptr_t)row >> 2) & 3u)) & 3u);
        if (head > n) head = n;
        if (blockIdx.x == 0 && (int)threadIdx.x < head) {
            const int j = threadIdx.x;
            row[j] = row[j] - (a + rgc[j]);
        }
        const int64_t j64 = (int64_t)head + ((int64_t)blockIdx.x * FINISH_THREADS + threadIdx.x) * 4;
        if (j64 >= n) continue;
        const int j = (int)j64;
        if (j + 4 <= n) {
            float4 v = *reinterpret_cast<float4*>(row + j);
            float4 g;
            if ((((uintptr_t)(rgc + j)) & 15u) == 0) {
                g = *reinterpret_cast<const float4*>(rgc + j);
            } else {
                g.x = rgc[j]; g.y = rgc[j + 1]; g.z = rgc[j + 2]; g.w = rgc[j + 3];
            }
            v.x = v.x - (a + g.x);
            v.y = v.y - (a + g.y);
            v.z = v.z - (a + g.z);
            v.w = v.w - (a + g.w);
            *reinterpret_cast<float4*>(row + j) = v;
        } else {
            for (int t = j; t < n; ++t) row[t] = row[t] - (a + rgc[t]);
        }
    }
}

}  // namespace

extern "C" int grl_verify_fold(const float* bn_weight, const float* bn_bias, const float* bn_mean, const float* bn_var,
                               const double* eps, const float* W, const float* b, int D, float* w, double* c64,
                               float* c32, void* stream) {
    GRL_REQUIRE(bn_weight && bn_bias && bn_mean && bn_var && eps && W && b && w && c64 && c32, "verify_fold: null");
    if (D <= 0 || D % 4) return grl_fail(GRL_EINVAL, "verify_fold: D = %d (a positive multiple of 4)", D);
    hipLaunchKernelGGL(verify_fold_kernel, dim3(1), dim3(FOLD_THREADS), 0, (hipStream_t)stream, bn_weight, bn_bias,
                       bn_mean, bn_var, *eps, W, b, D, w, c64, c32);
    return grl_check_launch("grl_verify_fold");
}

extern "C" int grl_verify_rows(const float* x, int64_t ldx, int n, int d, int col0, int Dv, const float* w,
                               const double* beta_host, const double* c64, float* r, float* qout, int64_t ldq, int full,
                               void* stream) {
    GRL_REQUIRE(x && w && r && beta_host, "verify_rows: null");
    const double beta = *beta_host;
    if (n <= 0 || d <= 0 || Dv <= 0 || col0 < 0 || (int64_t)col0 + Dv > d || ldx < d)
        return grl_fail(GRL_EINVAL, "verify_rows: slice [%d, %d + %d) of %d rows [%d], ld %lld", col0, col0, Dv, n, d,
                        (long long)ldx);
    if (d % 4 || col0 % 4 || Dv % 4 || ldx % 4 || !aligned16(x) || !aligned16(w))
        return grl_fail(GRL_EINVAL, "verify_rows: d, col0, Dv, ldx must be multiples of 4 and x, w 16-byte aligned");
    if (qout) {
        const int wq = full ? d : Dv;
        if (ldq < wq || ldq % 4 || !aligned16(qout))
            return grl_fail(GRL_EINVAL, "verify_rows: qout needs ld >= %d, ld %% 4 == 0, 16-byte alignment", wq);
        const uintptr_t a0 = (uintptr_t)x, a1 = a0 + (size_t)((int64_t)(n - 1) * ldx + d) * sizeof(float);
        const uintptr_t b0 = (uintptr_t)qout, b1 = b0 + (size_t)((int64_t)(n - 1) * ldq + wq) * sizeof(float);
        GRL_REQUIRE(!(a0 < b1 && b0 < a1), "verify_rows: qout overlaps x");
    }
    if (!(beta > 0.0 && beta <= 1.0)) return grl_fail(GRL_EINVAL, "verify_rows: beta = %g (0 < beta <= 1)", beta);
    const dim3 grid((unsigned)grl_ceil_div(n, ROWS_THREADS / 64));
    if (full)
        hipLaunchKernelGGL(verify_rows_kernel<true>, grid, dim3(ROWS_THREADS), 0, (hipStream_t)stream, x, ldx, n, d,
                           col0, Dv, w, beta, c64, r, qout, ldq);
    else
        hipLaunchKernelGGL(verify_rows_kernel<false>, grid, dim3(ROWS_THREADS), 0, (hipStream_t)stream, x, ldx, n, d,
                           col0, Dv, w, beta, c64, r, qout, ldq);
    return grl_check_launch("grl_verify_rows");
}

extern "C" int grl_verify_finish(float* D, int64_t ld, int nq, int n, const float* rq, const float* rg, int64_t c0,
                                 void* stream) {
    GRL_REQUIRE(D && rq && rg, "verify_finish: null");
    if (nq <= 0 || n <= 0 || ld < n || c0 < 0)
        return grl_fail(GRL_EINVAL, "verify_finish: block [%d, %d], ld %lld, c0 %lld", nq, n, (long long)ld, (long long)c0);
    GRL_REQUIRE(((uintptr_t)D & 3u) == 0, "verify_finish: D is not a float pointer");
    // + 1 chunk: a row's vector part starts up to 3 elements in
    const dim3 grid((unsigned)grl_ceil_div((int64_t)n + 3, FINISH_COLS), (unsigned)(nq < 65535 ? nq : 65535));
    hipLaunchKernelGGL(verify_finish_kernel, grid, dim3(FINISH_THREADS), 0, (hipStream_t)stream, D, ld, nq, n, rq, rg, c0);
    return grl_check_launch("grl_verify_finish");
}
