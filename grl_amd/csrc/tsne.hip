// The 2-d t-SNE map of a feature set (engine.tsne / tsne_affinities / tsne_gradient / tsne_from_affinities,
// DESIGN.md 4y): the conditional affinities of every sample over its K nearest neighbours, the joint affinities as a
// CSR over the union pattern, and the gradient loop with the EXACT repulsive term -- an n-body sum over all pairs,
// computed on the fly: no tree, no approximation, nothing n x n.
//
// Every sum below has one fp32 order, the "wave order" of DESIGN.md 4w: 64 partial sums, partial l the sequential sum
// from +0.0f, in ascending position, of the terms at the positions p with p % 64 == l (a term that is left out is
// skipped, not added as zero); then part[l] += part[l ^ s] for s = 32, 16, 8, 4, 2, 1, which leaves in every lane what
// the fold part[l] += part[l + s], l < s, leaves in lane 0 (fp32 addition commutes).  A position is the place in the
// neighbour list (perplexity), the sample index j (repulsion, Z) or the place in the CSR row (attraction, KL), so no
// result depends on the launch geometry.  Plain IEEE division, no contraction (the library's flags), no atomics.
//
// Mapping.  One wave per row everywhere, four rows per workgroup, the row index scalar (readfirstlane).  The
// repulsion kernel is the hot one: lane l takes j = l, l + 64, ..: y[j] is one coalesced 8-byte load per lane (512
// bytes per wave) of an array that stays in L2 (8 n bytes), three accumulators, six xor-shuffle steps, no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/grl_hip.h"
#include "common.h"

namespace {

constexpr int TS_THREADS = 256;
constexpr int TS_WAVES = TS_THREADS / 64;
constexpr int TS_KMAX = 1023;                      // neighbours of a sample: search's 1024 less the sample itself
constexpr int TS_SLOTS = (TS_KMAX + 63) / 64;      // list entries a lane holds

__device__ __forceinline__ bool ts_finite(float v) { return fabsf(v) < INFINITY; }        // (false for a NaN)

// the wave order's fold: every lane receives the total
__device__ __forceinline__ float ts_fold(float v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

__device__ __forceinline__ int ts_row() {
    // (the wave index is the same in all 64 lanes: everything derived from it stays in scalar registers)
    return blockIdx.x * TS_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
}

// q = 1 / (1 + |y_i - y_j|^2) and the two differences
__device__ __forceinline__ float ts_q(f32x2 yi, f32x2 yj, float& dx0, float& dx1) {
    dx0 = yi[0] - yj[0];
    dx1 = yi[1] - yj[1];
    const float r = dx0 * dx0 + dx1 * dx1;
    return 1.0f / (1.0f + r);
}

__global__ __launch_bounds__(TS_THREADS) void ts_square_kernel(float* __restrict__ d, int64_t ld, int nrows, int ncols) {
    const int lane = threadIdx.x & 63;
    const int r = ts_row();
    if (r >= nrows) return;
    float* __restrict__ drow = d + (int64_t)r * ld;
    for (int col = lane; col < ncols; col += 64) { const float s = drow[col]; drow[col] = s * s; }
}

// scikit-learn's bisection on beta (_binary_search_perplexity) in fp32 over the K distances of one row, shifted
__global__ __launch_bounds__(TS_THREADS) void ts_perplexity_kernel(const float* __restrict__ e, int n, int K,
                                                                   float log_perp, float* __restrict__ cond,
                                                                   float* __restrict__ beta_out,
                                                                   uint8_t* __restrict__ iso) {
    const int lane = threadIdx.x & 63;
    const int i = ts_row();
    if (i >= n) return;
    const float* __restrict__ erow = e + (int64_t)i * K;
    float* __restrict__ crow = cond + (int64_t)i * K;
    float ev[TS_SLOTS], pv[TS_SLOTS];
    bool bad = false;
#pragma unroll
    for (int m = 0; m < TS_SLOTS; ++m) {
        const int k = lane + 64 * m;
        ev[m] = k < K ? erow[k] : 0.f;
        pv[m] = 0.f;
        bad = bad || !ts_finite(ev[m]);
    }
    if (__ballot(bad)) {                                           // an isolated sample: no affinities
#pragma unroll
        for (int m = 0; m < TS_SLOTS; ++m) if (lane + 64 * m < K) crow[lane + 64 * m] = 0.f;
        if (lane == 0) { beta_out[i] = NAN; iso[i] = 1; }
        return;
    }
    // the distances less the list's first (its smallest: the list ascends): the same p and H, and exp never underflows
    // in every term at once, as it would in fp32 at e beta > 87 -- a list of nearly equal distances needs such a beta
    const float e0 = erow[0];
#pragma unroll
    for (int m = 0; m < TS_SLOTS; ++m) ev[m] = ev[m] - e0;
    float beta = 1.0f, used = 1.0f, bmin = -INFINITY, bmax = INFINITY;
    for (int step = 0; step < 100; ++step) {
        used = beta;
        float part = 0.f;
#pragma unroll
        for (int m = 0; m < TS_SLOTS; ++m)                         // (64 * m < K is the same in every lane: a scalar branch)
            if (64 * m < K && lane + 64 * m < K) { pv[m] = expf(-(ev[m] * beta)); part += pv[m]; }
        const float sum = ts_fold(part);                           // (>= 1: the first term is exp(-0))
        part = 0.f;
#pragma unroll
        for (int m = 0; m < TS_SLOTS; ++m)
            if (64 * m < K && lane + 64 * m < K) { pv[m] = pv[m] / sum; part += ev[m] * pv[m]; }
        const float h = logf(sum) + beta * ts_fold(part);
        const float diff = h - log_perp;
        if (fabsf(diff) <= 1e-5f) break;
        if (diff > 0.f) {
            bmin = beta;
            beta = bmax == INFINITY ? beta * 2.0f : (beta + bmax) * 0.5f;
        } else {
            bmax = beta;
            beta = bmin == -INFINITY ? beta * 0.5f : (beta + bmin) * 0.5f;
        }
    }
    // (the probabilities of the last step that was evaluated, and that step's beta)
#pragma unroll
    for (int m = 0; m < TS_SLOTS; ++m) if (lane + 64 * m < K) crow[lane + 64 * m] = pv[m];
    if (lane == 0) { beta_out[i] = used; iso[i] = 0; }
}

// Row i of the joint affinities: the union of A = row i of the conditional matrix (acol ascending, entries < 0 in
// front are no entries) and B = its column i (csc_row ascending).  An entry's place is its rank in the union:
// (its place in its own list) + (the entries of the other list below it) - (the pairs present in both lists below
// it); a pair present in both is written from A.
__global__ __launch_bounds__(TS_THREADS) void ts_joint_kernel(const int32_t* __restrict__ acol,
                                                              const float* __restrict__ aval, int K,
                                                              const int64_t* __restrict__ csc_ptr,
                                                              const int32_t* __restrict__ csc_row,
                                                              const float* __restrict__ csc_val, int n, float den,
                                                              const int64_t* __restrict__ row_ptr,
                                                              int32_t* __restrict__ cnt, int32_t* __restrict__ col,
                                                              float* __restrict__ val) {
    const int lane = threadIdx.x & 63;
    const int i = ts_row();
    if (i >= n) return;
    const int32_t* __restrict__ A = acol + (int64_t)i * K;
    const float* __restrict__ Av = aval + (int64_t)i * K;
    const int a0 = lower_bound<int>(A, 0, K, 0);
    A += a0; Av += a0;
    const int LA = K - a0;
    const int64_t bs = csc_ptr[i];
    const int LB = (int)(csc_ptr[i + 1] - bs);
    const int32_t* __restrict__ B = csc_row + bs;
    const float* __restrict__ Bv = csc_val + bs;
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;       // the lanes under this one
    const int64_t out = row_ptr ? row_ptr[i] : 0;
    int dups = 0;
    for (int base = 0; base < LA; base += 64) {
        const int a = base + lane;
        bool dup = false;
        int x = 0, pb = 0;
        if (a < LA) {
            x = A[a];
            pb = lower_bound<int>(B, 0, LB, x);
            dup = pb < LB && B[pb] == x;
        }
        const unsigned long long mask = __ballot(dup);
        if (row_ptr && a < LA) {
            const int64_t pos = out + a + pb - (dups + __popcll(mask & below));
            col[pos] = x;
            val[pos] = (Av[a] + (dup ? Bv[pb] : 0.f)) / den;
        }
        dups += __popcll(mask);
    }
    if (!row_ptr) {
        if (lane == 0) cnt[i] = LA + LB - dups;
        return;
    }
    dups = 0;
    for (int base = 0; base < LB; base += 64) {
        const int b = base + lane;
        bool dup = false;
        int x = 0, pa = 0;
        if (b < LB) {
            x = B[b];
            pa = lower_bound<int>(A, 0, LA, x);
            dup = pa < LA && A[pa] == x;
        }
        const unsigned long long mask = __ballot(dup);
        if (b < LB && !dup) {
            const int64_t pos = out + b + pa - (dups + __popcll(mask & below));
            col[pos] = x;
            val[pos] = (0.f + Bv[b]) / den;
        }
        dups += __popcll(mask);
    }
}

// rep[i] = sum over the live j != i of q^2 (y_i - y_j), rowz[i] = sum of q: the exact repulsive term
__global__ __launch_bounds__(TS_THREADS) void ts_repulsion_kernel(const f32x2* __restrict__ y,
                                                                  const uint8_t* __restrict__ iso, int n,
                                                                  f32x2* __restrict__ rep, float* __restrict__ rowz) {
    const int lane = threadIdx.x & 63;
    const int i = ts_row();
    if (i >= n) return;
    if (iso && iso[i]) {                                           // exerts no force and feels none
        if (lane == 0) { rep[i] = f32x2{0.f, 0.f}; rowz[i] = 0.f; }
        return;
    }
    const f32x2 yi = y[i];
    float r0 = 0.f, r1 = 0.f, z = 0.f;
    for (int j = lane; j < n; j += 64) {
        const f32x2 yj = y[j];
        const bool live = j != i && !(iso && iso[j]);
        float dx0, dx1;
        const float q = ts_q(yi, yj, dx0, dx1);
        const float qq = q * q;
        if (live) { r0 += qq * dx0; r1 += qq * dx1; z += q; }
    }
    r0 = ts_fold(r0); r1 = ts_fold(r1); z = ts_fold(z);
    if (lane == 0) { rep[i] = f32x2{r0, r1}; rowz[i] = z; }
}

// Z = the sum of rowz in the wave order: one wave
__global__ __launch_bounds__(64) void ts_z_kernel(const float* __restrict__ rowz, int n, float* __restrict__ z) {
    const int lane = threadIdx.x;
    float s = 0.f;
#pragma unroll 8                                                   // (the loads of eight steps in flight; the adds keep their order)
    for (int j = lane; j < n; j += 64) s += rowz[j];
    s = ts_fold(s);
    if (lane == 0) z[0] = s;
}

// att[i] over the row's CSR entries, grad = 4 (att - rep / Z), and (update != NULL) scikit-learn's update rule
__global__ __launch_bounds__(TS_THREADS) void ts_update_kernel(const int64_t* __restrict__ row_ptr,
                                                               const int32_t* __restrict__ col,
                                                               const float* __restrict__ val,
                                                               const f32x2* __restrict__ y,
                                                               const uint8_t* __restrict__ iso, int n, float alpha,
                                                               const f32x2* __restrict__ rep,
                                                               const float* __restrict__ zp, f32x2* __restrict__ grad,
                                                               f32x2* __restrict__ gains, f32x2* __restrict__ update,
                                                               f32x2* __restrict__ y_out, float momentum, float lr) {
    const int lane = threadIdx.x & 63;
    const int i = ts_row();
    if (i >= n) return;
    const f32x2 yi = y[i];
    if (iso && iso[i]) {
        if (lane == 0) {
            if (grad) grad[i] = f32x2{0.f, 0.f};
            if (update) y_out[i] = yi;
        }
        return;
    }
    const int64_t s = row_ptr[i];
    const int64_t len = row_ptr[i + 1] - s;
    float a0 = 0.f, a1 = 0.f;
    for (int64_t p = lane; p < len; p += 64) {
        const int j = col[s + p];
        if (iso && iso[j]) continue;
        float dx0, dx1;
        const float q = ts_q(yi, y[j], dx0, dx1);
        const float w = (alpha * val[s + p]) * q;
        a0 += w * dx0; a1 += w * dx1;
    }
    a0 = ts_fold(a0); a1 = ts_fold(a1);
    if (lane != 0) return;
    const float z = zp[0];
    const f32x2 rp = rep[i];
    const float g[2] = {4.0f * (a0 - rp[0] / z), 4.0f * (a1 - rp[1] / z)};
    if (grad) grad[i] = f32x2{g[0], g[1]};
    if (!update) return;
    const f32x2 gn = gains[i], up = update[i];
    f32x2 ngn, nup, ny;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        float gc = up[c] * g[c] < 0.f ? gn[c] + 0.2f : gn[c] * 0.8f;
        gc = gc < 0.01f ? 0.01f : gc;
        const float u = momentum * up[c] - lr * (gc * g[c]);
        ngn[c] = gc; nup[c] = u; ny[c] = yi[c] + u;
    }
    gains[i] = ngn; update[i] = nup; y_out[i] = ny;
}

// rowkl[i] = the sum over the row's stored entries with P > 0 of P log(P Z / q), the logarithm taken in fp64 and rounded
__global__ __launch_bounds__(TS_THREADS) void ts_kl_kernel(const int64_t* __restrict__ row_ptr,
                                                           const int32_t* __restrict__ col,
                                                           const float* __restrict__ val, const f32x2* __restrict__ y,
                                                           const uint8_t* __restrict__ iso, int n,
                                                           const float* __restrict__ zp, float* __restrict__ rowkl) {
    const int lane = threadIdx.x & 63;
    const int i = ts_row();
    if (i >= n) return;
    float acc = 0.f;
    if (!(iso && iso[i])) {
        const f32x2 yi = y[i];
        const float z = zp[0];
        const int64_t s = row_ptr[i];
        const int64_t len = row_ptr[i + 1] - s;
        for (int64_t p = lane; p < len; p += 64) {
            const int j = col[s + p];
            const float pij = val[s + p];
            if ((iso && iso[j]) || !(pij > 0.f)) continue;
            float dx0, dx1;
            const float q = ts_q(yi, y[j], dx0, dx1);
            acc += pij * (float)log((double)((pij * z) / q));      // (the fp32 logarithm correctly rounded: once a run)
        }
    }
    acc = ts_fold(acc);
    if (lane == 0) rowkl[i] = acc;
}

}  // namespace

extern "C" int grl_tsne_square_block(float* d, int64_t ld, int nrows, int ncols, void* stream) {
    GRL_REQUIRE(nrows >= 0 && ncols >= 1 && ld >= ncols, "tsne_square_block: nrows >= 0, ncols >= 1, ld >= ncols");
    GRL_REQUIRE(d, "tsne_square_block: null");
    if (nrows == 0) return GRL_OK;
    hipLaunchKernelGGL(ts_square_kernel, dim3(grl_ceil_div(nrows, TS_WAVES)), dim3(TS_THREADS), 0, (hipStream_t)stream,
                       d, ld, nrows, ncols);
    return grl_check_launch("grl_tsne_square_block");
}

extern "C" int grl_tsne_perplexity(const float* e, int n, int K, float log_perplexity, float* cond, float* beta,
                                   uint8_t* isolated, void* stream) {
    GRL_REQUIRE(n >= 0 && K >= 1 && K <= TS_KMAX, "tsne_perplexity: n >= 0 and 1 <= K <= 1023");
    GRL_REQUIRE(log_perplexity == log_perplexity, "tsne_perplexity: log_perplexity is NaN");
    if (n == 0) return GRL_OK;
    GRL_REQUIRE(e && cond && beta && isolated, "tsne_perplexity: null");
    hipLaunchKernelGGL(ts_perplexity_kernel, dim3(grl_ceil_div(n, TS_WAVES)), dim3(TS_THREADS), 0, (hipStream_t)stream,
                       e, n, K, log_perplexity, cond, beta, isolated);
    return grl_check_launch("grl_tsne_perplexity");
}

extern "C" int grl_tsne_joint(const int32_t* acol, const float* aval, int K, const int64_t* csc_ptr,
                              const int32_t* csc_row, const float* csc_val, int n, float den, const int64_t* row_ptr,
                              int32_t* cnt, int32_t* col, float* val, void* stream) {
    GRL_REQUIRE(n >= 1 && K >= 1 && K <= TS_KMAX, "tsne_joint: n >= 1 and 1 <= K <= 1023");
    GRL_REQUIRE(acol && aval && csc_ptr && csc_row && csc_val, "tsne_joint: null");
    GRL_REQUIRE(row_ptr ? (col && val) : (cnt != nullptr), "tsne_joint: count needs cnt, fill needs col and val");
    GRL_REQUIRE(den > 0.f, "tsne_joint: den > 0");
    hipLaunchKernelGGL(ts_joint_kernel, dim3(grl_ceil_div(n, TS_WAVES)), dim3(TS_THREADS), 0, (hipStream_t)stream, acol,
                       aval, K, csc_ptr, csc_row, csc_val, n, den, row_ptr, cnt, col, val);
    return grl_check_launch("grl_tsne_joint");
}

extern "C" int grl_tsne_repulsion(const float* y, const uint8_t* isolated, int n, float* rep, float* rowz,
                                  void* stream) {
    GRL_REQUIRE(n >= 0, "tsne_repulsion: n >= 0");
    if (n == 0) return GRL_OK;
    GRL_REQUIRE(y && rep && rowz, "tsne_repulsion: null");
    GRL_REQUIRE((((uintptr_t)y | (uintptr_t)rep) & 7u) == 0, "tsne_repulsion: y and rep must be 8-byte aligned");
    hipLaunchKernelGGL(ts_repulsion_kernel, dim3(grl_ceil_div(n, TS_WAVES)), dim3(TS_THREADS), 0, (hipStream_t)stream,
                       (const f32x2*)y, isolated, n, (f32x2*)rep, rowz);
    return grl_check_launch("grl_tsne_repulsion");
}

extern "C" int grl_tsne_z(const float* rowz, int n, float* z, void* stream) {
    GRL_REQUIRE(n >= 0 && z && (rowz || n == 0), "tsne_z: bad args");
    hipLaunchKernelGGL(ts_z_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, rowz, n, z);
    return grl_check_launch("grl_tsne_z");
}

extern "C" int grl_tsne_update(const int64_t* row_ptr, const int32_t* col, const float* val, const float* y,
                               const uint8_t* isolated, int n, float alpha, const float* rep, const float* z,
                               float* grad, float* gains, float* update, float* y_out, float momentum,
                               float learning_rate, void* stream) {
    GRL_REQUIRE(n >= 0, "tsne_update: n >= 0");
    if (n == 0) return GRL_OK;
    GRL_REQUIRE(row_ptr && col && val && y && rep && z, "tsne_update: null");
    GRL_REQUIRE(update ? (gains && y_out && y_out != y) : (grad != nullptr),
                "tsne_update: a step needs gains, update and a y_out other than y; without update, grad");
    GRL_REQUIRE((((uintptr_t)y | (uintptr_t)rep | (uintptr_t)grad | (uintptr_t)gains | (uintptr_t)update |
                  (uintptr_t)y_out) & 7u) == 0, "tsne_update: the [n, 2] arrays must be 8-byte aligned");
    hipLaunchKernelGGL(ts_update_kernel, dim3(grl_ceil_div(n, TS_WAVES)), dim3(TS_THREADS), 0, (hipStream_t)stream,
                       row_ptr, col, val, (const f32x2*)y, isolated, n, alpha, (const f32x2*)rep, z, (f32x2*)grad,
                       (f32x2*)gains, (f32x2*)update, (f32x2*)y_out, momentum, learning_rate);
    return grl_check_launch("grl_tsne_update");
}

extern "C" int grl_tsne_kl(const int64_t* row_ptr, const int32_t* col, const float* val, const float* y,
                           const uint8_t* isolated, int n, const float* z, float* rowkl, void* stream) {
    GRL_REQUIRE(n >= 0, "tsne_kl: n >= 0");
    if (n == 0) return GRL_OK;
    GRL_REQUIRE(row_ptr && col && val && y && z && rowkl, "tsne_kl: null");
    GRL_REQUIRE(((uintptr_t)y & 7u) == 0, "tsne_kl: y must be 8-byte aligned");
    hipLaunchKernelGGL(ts_kl_kernel, dim3(grl_ceil_div(n, TS_WAVES)), dim3(TS_THREADS), 0, (hipStream_t)stream, row_ptr,
                       col, val, (const f32x2*)y, isolated, n, z, rowkl);
    return grl_check_launch("grl_tsne_kl");
}
