// Diffusion (manifold ranking) on the gallery's mutual-kNN graph (engine.diffusion_graph / diffusion_solve /
// diffusion_search): the graph in a fixed-width ELL layout [n][k], a sparse x dense product with many
// right-hand sides and a batched conjugate-gradient loop for (I - alpha S) f = y, one column per query.
//
// The arithmetic is fixed so that a numpy float32 host model (tests/diffusion_ref.py) gives the same bits: only
// + - x / sqrt, each correctly rounded, no fma (-ffp-contract=off and the pragma below), every sum in a prescribed
// order.  Dot products are reduced without float atomics: every wave sums DIFF_WAVE_ROWS consecutive rows in row order,
// a workgroup adds its DIFF_WAVES wave sums in wave order into one partial per DIFF_ROWS rows, and a finishing kernel adds
// the partials in row order.  Two runs give the same bits.
//
// The state of the solver (x, r, p, Ap) is [n][B], node-major with the B query columns of a node contiguous: the gather
// of a neighbour's row in the product is one coalesced read, and the row's slots (idx, S) are wave-uniform scalars.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grl_hip.h"
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int DIFF_K_MAX = 128;                                 // graph neighbours per row
constexpr int DIFF_GAMMA_MAX = 8;
constexpr int DIFF_THREADS = 256;
constexpr int DIFF_WAVES = DIFF_THREADS / 64;
constexpr int DIFF_WAVE_ROWS = 16;                              // consecutive rows one wave owns
constexpr int DIFF_ROWS = DIFF_WAVES * DIFF_WAVE_ROWS;          // rows per workgroup = rows per dot-product partial
constexpr int DIFF_BATCH = 4;                                   // neighbour rows in flight per lane

__device__ __forceinline__ float diff_weight(float dist, int gamma) {
    const float s = dist < 0.f ? -dist : 0.f;                   // NaN: the comparison is false -> 0
    float w = s;
    for (int a = 1; a < gamma; ++a) w = w * s;
    return w;
}

// ---- the mutual graph ------------------------------------------------------------------------------------------------
// One wave per row i, four rows per workgroup.  sidx / sdist [n][ldl] are the k + 1 entries of search(gf, gf, k + 1).
// Slot t of row i is search position t + (t >= selfpos), selfpos = the first position holding i (k when there is none:
// the last entry is dropped).  An index outside [0, n), or a further entry equal to i, is padding (-1, weight 0).
// For slot t with neighbour j the wave scans row j's k + 1 entries (64 at a time, one coalesced read): i is in row j's
// kept list when it occurs at position p and (j occurs in its own list or p < k); then a = min(w_ij, w_ji) with w_ji from
// sdist[j][p], else 0.  Lane t & 63 keeps a; deg[i] is the sum of the k values in slot order by lane 0.
__global__ __launch_bounds__(DIFF_THREADS) void diff_mutual_kernel(const int64_t* __restrict__ sidx,
                                                                   const float* __restrict__ sdist, int64_t ldl, int n,
                                                                   int k, int gamma, int32_t* __restrict__ idx,
                                                                   float* __restrict__ a, int64_t ldo,
                                                                   float* __restrict__ deg) {
    __shared__ int sj[DIFF_WAVES][DIFF_K_MAX];
    __shared__ float sw[DIFF_WAVES][DIFF_K_MAX];
    __shared__ float sa[DIFF_WAVES][DIFF_K_MAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * DIFF_WAVES + wave;
    const bool active = row < n;

    int selfpos = k;
    if (active) {
        bool found = false;
        for (int base = 0; base <= k; base += 64) {
            const int p = base + lane;
            const bool hit = p <= k && sidx[(int64_t)row * ldl + p] == (int64_t)row;
            const unsigned long long m = __ballot(hit);
            if (!found && m) { selfpos = base + __ffsll((long long)m) - 1; found = true; }
        }
    }
    for (int t = lane; t < DIFF_K_MAX; t += 64) {
        int j = -1;
        float w = 0.f;
        if (active && t < k) {
            const int p = t + (t >= selfpos ? 1 : 0);
            const int64_t v = sidx[(int64_t)row * ldl + p];
            if (v >= 0 && v < n && v != row) {
                j = (int)v;
                w = diff_weight(sdist[(int64_t)row * ldl + p], gamma);
            }
        }
        sj[wave][t] = j;
        sw[wave][t] = w;
    }
    __syncthreads();

    float a0 = 0.f, a1 = 0.f;
    for (int t = 0; t < k; ++t) {
        const int j = __builtin_amdgcn_readfirstlane(sj[wave][t]);
        float av = 0.f;
        if (j >= 0) {
            const int64_t* lj = sidx + (int64_t)j * ldl;
            int pos = -1;
            bool self_j = false;
            for (int base = 0; base <= k; base += 64) {
                const int p = base + lane;
                const int64_t v = p <= k ? lj[p] : (int64_t)-2;
                const unsigned long long mi = __ballot(v == (int64_t)row);
                const unsigned long long mj = __ballot(v == (int64_t)j);
                if (pos < 0 && mi) pos = base + __ffsll((long long)mi) - 1;
                if (mj) self_j = true;
            }
            if (pos >= 0 && (self_j || pos < k)) {
                const float wij = sw[wave][t];
                const float wji = diff_weight(sdist[(int64_t)j * ldl + pos], gamma);
                av = wji < wij ? wji : wij;
            }
        }
        if (lane == (t & 63)) { if (t < 64) a0 = av; else a1 = av; }
    }
    sa[wave][lane] = a0;
    sa[wave][lane + 64] = a1;
    __syncthreads();
    if (!active) return;
    for (int t = lane; t < k; t += 64) {
        idx[(int64_t)row * ldo + t] = sj[wave][t];
        a[(int64_t)row * ldo + t] = sa[wave][t];
    }
    if (lane == 0) {
        float d = 0.f;
        for (int t = 0; t < k; ++t) d = d + sa[wave][t];
        deg[row] = d;
    }
}

// S = a / (sqrt(deg_i) * sqrt(deg_j)) in place, 0 where a is 0 (a != 0 implies a valid j and deg_i, deg_j >= a > 0)
__global__ __launch_bounds__(DIFF_THREADS) void diff_normalise_kernel(const int32_t* __restrict__ idx,
                                                                      float* __restrict__ a, int64_t ldo, int n, int k,
                                                                      const float* __restrict__ deg) {
    const int64_t total = (int64_t)n * k;
    for (int64_t e = (int64_t)blockIdx.x * DIFF_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * DIFF_THREADS) {
        const int64_t i = e / k;
        const int64_t at = i * ldo + (e - i * k);
        const float av = a[at];
        if (av == 0.f) continue;
        const int j = idx[at];
        const float den = sqrtf(deg[i]) * sqrtf(deg[j]);
        a[at] = __fdiv_rn(av, den);
    }
}

// ---- the product and the CG updates: one thread mapping ---------------------------------------------------------------
// blockIdx.x = block of DIFF_ROWS rows, blockIdx.y = tile of 64 * VEC columns.  Wave w owns the rows
// blockIdx.x * DIFF_ROWS + w * DIFF_WAVE_ROWS .. + DIFF_WAVE_ROWS - 1 and walks them in order; a lane owns VEC consecutive
// columns (VEC = 4: B % 4 == 0 and 16-byte aligned pointers, one dwordx4 access per row).  A lane's partial dot product is
// the sum over its wave's rows in row order from +0; block_partial adds the four wave sums in wave order.
template <int VEC>
struct Cols {
    float v[VEC];
};

template <int VEC>
__device__ __forceinline__ Cols<VEC> ld_cols(const float* p) {
    Cols<VEC> c;
    if (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        c.v[0] = q.x; c.v[1 % VEC] = q.y; c.v[2 % VEC] = q.z; c.v[3 % VEC] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) c.v[e] = p[e];
    }
    return c;
}

template <int VEC>
__device__ __forceinline__ void st_cols(float* p, const Cols<VEC>& c) {
    if (VEC == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(c.v[0], c.v[1 % VEC], c.v[2 % VEC], c.v[3 % VEC]);
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) p[e] = c.v[e];
    }
}

// part[blockIdx.x][c0 .. c0 + VEC) = ((wave 0 + wave 1) + wave 2) + wave 3 of the lanes' sums
template <int VEC>
__device__ __forceinline__ void block_partial(const Cols<VEC>& dot, float* sd, int c0, bool col_ok, int B,
                                              float* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < VEC; ++e) sd[(wave * 64 + lane) * VEC + e] = dot.v[e];
    __syncthreads();
    if (wave == 0 && col_ok) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            float s = sd[lane * VEC + e];
#pragma unroll
            for (int w = 1; w < DIFF_WAVES; ++w) s = s + sd[(w * 64 + lane) * VEC + e];
            part[(int64_t)blockIdx.x * B + c0 + e] = s;
        }
    }
}

// Ap[i][b] = p[i][b] - alpha * sum_t S[i][t] * p[idx[i][t]][b] over the slots with S != 0 (and a valid index) in slot
// order, acc from +0: acc = acc + (S * p_j), Ap = p - (alpha * acc).  part = the partials of p . Ap.
template <int VEC>
__global__ __launch_bounds__(DIFF_THREADS) void diff_apply_kernel(const int32_t* __restrict__ idx,
                                                                  const float* __restrict__ S, int64_t ldg, int n, int k,
                                                                  const float* __restrict__ p, int B, float alpha,
                                                                  float* __restrict__ Ap, float* __restrict__ part) {
    __shared__ float sd[DIFF_THREADS * VEC];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c0 = (blockIdx.y * 64 + lane) * VEC;
    const bool col_ok = c0 < B;
    const int r0 = blockIdx.x * DIFF_ROWS + wave * DIFF_WAVE_ROWS;
    Cols<VEC> dot;
#pragma unroll
    for (int e = 0; e < VEC; ++e) dot.v[e] = 0.f;
    if (col_ok) {
        for (int i = r0; i < min(r0 + DIFF_WAVE_ROWS, n); ++i) {
            const int32_t* ji = idx + (int64_t)i * ldg;
            const float* si = S + (int64_t)i * ldg;
            const Cols<VEC> pv = ld_cols<VEC>(p + (int64_t)i * B + c0);
            Cols<VEC> acc;
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc.v[e] = 0.f;
            for (int t0 = 0; t0 < k; t0 += DIFF_BATCH) {
                float s[DIFF_BATCH];
                Cols<VEC> nb[DIFF_BATCH];
#pragma unroll
                for (int u = 0; u < DIFF_BATCH; ++u) {
                    s[u] = 0.f;
                    if (t0 + u < k) {
                        const int j = ji[t0 + u];
                        const float sv = si[t0 + u];
                        if (sv != 0.f && (unsigned)j < (unsigned)n) {
                            s[u] = sv;
                            nb[u] = ld_cols<VEC>(p + (int64_t)j * B + c0);
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < DIFF_BATCH; ++u) {
                    if (s[u] != 0.f) {
#pragma unroll
                        for (int e = 0; e < VEC; ++e) acc.v[e] = acc.v[e] + (s[u] * nb[u].v[e]);
                    }
                }
            }
            Cols<VEC> out;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                out.v[e] = pv.v[e] - (alpha * acc.v[e]);
                dot.v[e] = dot.v[e] + (pv.v[e] * out.v[e]);
            }
            st_cols<VEC>(Ap + (int64_t)i * B + c0, out);
        }
    }
    block_partial<VEC>(dot, sd, c0, col_ok, B, part);
}

// MODE 0: part = partials of r . r.
// MODE 1: per column c that is not frozen x = x + (a_c * p), r = r - (a_c * Ap); part = partials of r . r (new r).
// MODE 2: per column c that is not frozen p = r + (b_c * p).
template <int VEC, int MODE>
__global__ __launch_bounds__(DIFF_THREADS) void diff_update_kernel(float* __restrict__ x, float* __restrict__ r,
                                                                   float* __restrict__ p, const float* __restrict__ Ap,
                                                                   const float* __restrict__ coef,
                                                                   const int32_t* __restrict__ frozen, int n, int B,
                                                                   float* __restrict__ part) {
    __shared__ float sd[DIFF_THREADS * VEC];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c0 = (blockIdx.y * 64 + lane) * VEC;
    const bool col_ok = c0 < B;
    const int r0 = blockIdx.x * DIFF_ROWS + wave * DIFF_WAVE_ROWS;
    Cols<VEC> dot;
#pragma unroll
    for (int e = 0; e < VEC; ++e) dot.v[e] = 0.f;
    if (col_ok) {
        float cf[VEC];
        bool live[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            cf[e] = MODE == 0 ? 0.f : coef[c0 + e];
            live[e] = MODE != 0 && frozen[c0 + e] == 0;
        }
        for (int i = r0; i < min(r0 + DIFF_WAVE_ROWS, n); ++i) {
            const int64_t at = (int64_t)i * B + c0;
            Cols<VEC> rv = ld_cols<VEC>(r + at);
            if (MODE == 1) {
                const Cols<VEC> pv = ld_cols<VEC>(p + at), av = ld_cols<VEC>(Ap + at);
                Cols<VEC> xv = ld_cols<VEC>(x + at);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    if (live[e]) {
                        xv.v[e] = xv.v[e] + (cf[e] * pv.v[e]);
                        rv.v[e] = rv.v[e] - (cf[e] * av.v[e]);
                    }
                }
                st_cols<VEC>(x + at, xv);
                st_cols<VEC>(r + at, rv);
            }
            if (MODE == 2) {
                Cols<VEC> pv = ld_cols<VEC>(p + at);
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    if (live[e]) pv.v[e] = rv.v[e] + (cf[e] * pv.v[e]);
                st_cols<VEC>(p + at, pv);
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) dot.v[e] = dot.v[e] + (rv.v[e] * rv.v[e]);
            }
        }
    }
    if (MODE != 2) block_partial<VEC>(dot, sd, c0, col_ok, B, part);
}

// One thread per column: sum = the nblk partials in row order from +0.
// MODE 0 (start): rr = sum, frozen = 0.
// MODE 1 (after the product, sum = p . Ap): a column freezes when r . r is not a positive finite number or p . Ap is
//         <= 0 or not finite; coef = frozen ? 0 : rr / sum.
// MODE 2 (after the update, sum = the new r . r): coef = frozen ? 0 : sum / rr; rr = sum.
template <int MODE>
__global__ __launch_bounds__(DIFF_THREADS) void diff_finish_kernel(const float* __restrict__ part, int nblk, int B,
                                                                   float* __restrict__ rr, float* __restrict__ coef,
                                                                   int32_t* __restrict__ frozen) {
    const int c = blockIdx.x * DIFF_THREADS + threadIdx.x;
    if (c >= B) return;
    float sum = 0.f;
    for (int g = 0; g < nblk; ++g) sum = sum + part[(int64_t)g * B + c];
    if (MODE == 0) {
        rr[c] = sum;
        frozen[c] = 0;
        return;
    }
    const float old = rr[c];
    int fz = frozen[c];
    if (MODE == 1) {
        if (!(old > 0.f) || !(old < __builtin_huge_valf()) || !(sum > 0.f) || !(sum < __builtin_huge_valf())) fz = 1;
        frozen[c] = fz;
        coef[c] = fz ? 0.f : __fdiv_rn(old, sum);
    } else {
        coef[c] = fz ? 0.f : __fdiv_rn(sum, old);
        rr[c] = sum;
    }
}

// y[idx[q][t]][q] = val (gamma == 0) or max(-val, 0)^gamma (gamma >= 1: val is search's cosine distance), t in list order
// (a repeated index keeps its last value); an index outside [0, n) is padding.  y is zero-filled by the caller.
__global__ __launch_bounds__(DIFF_THREADS) void diff_seed_kernel(const int64_t* __restrict__ sidx,
                                                                 const float* __restrict__ sval, int64_t lds, int B, int kq,
                                                                 int n, int gamma, float* __restrict__ y) {
    const int q = blockIdx.x * DIFF_THREADS + threadIdx.x;
    if (q >= B) return;
    for (int t = 0; t < kq; ++t) {
        const int64_t j = sidx[(int64_t)q * lds + t];
        if (j < 0 || j >= n) continue;
        const float v = sval[(int64_t)q * lds + t];
        y[j * B + q] = gamma == 0 ? v : diff_weight(v, gamma);
    }
}

// out[b][i] = x[i][b] (negate: -x[i][b]); x [n][B], out [B][ldo].  64 x 64 tiles through LDS.
__global__ __launch_bounds__(DIFF_THREADS) void diff_transpose_kernel(const float* __restrict__ x, int n, int B, int negate,
                                                                      float* __restrict__ out, int64_t ldo) {
    __shared__ float tile[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int i0 = blockIdx.x * 64, b0 = blockIdx.y * 64;
    for (int rr = ty; rr < 64; rr += DIFF_WAVES) {
        const int i = i0 + rr, b = b0 + tx;
        tile[rr][tx] = (i < n && b < B) ? x[(int64_t)i * B + b] : 0.f;
    }
    __syncthreads();
    for (int rr = ty; rr < 64; rr += DIFF_WAVES) {
        const int b = b0 + rr, i = i0 + tx;
        if (b < B && i < n) {
            const float v = tile[tx][rr];
            out[(int64_t)b * ldo + i] = negate ? -v : v;
        }
    }
}

inline bool vec4_ok(int B, const void* a, const void* b, const void* c, const void* d) {
    return B % 4 == 0 && B >= 256 && aligned16(a) && aligned16(b) && aligned16(c) && aligned16(d);
}

inline dim3 state_grid(int n, int B, int vec) { return dim3((unsigned)grl_ceil_div(n, DIFF_ROWS), (unsigned)grl_ceil_div(B, 64 * vec)); }

void launch_apply(const int32_t* idx, const float* S, int64_t ldg, int n, int k, const float* p, int B, float alpha,
                  float* Ap, float* part, hipStream_t s) {
    if (vec4_ok(B, p, Ap, p, Ap))
        hipLaunchKernelGGL(diff_apply_kernel<4>, state_grid(n, B, 4), dim3(DIFF_THREADS), 0, s, idx, S, ldg, n, k, p, B,
                           alpha, Ap, part);
    else
        hipLaunchKernelGGL(diff_apply_kernel<1>, state_grid(n, B, 1), dim3(DIFF_THREADS), 0, s, idx, S, ldg, n, k, p, B,
                           alpha, Ap, part);
}

template <int MODE>
void launch_update(float* x, float* r, float* p, const float* Ap, const float* coef, const int32_t* frozen, int n, int B,
                   float* part, hipStream_t s) {
    if (vec4_ok(B, x, r, p, Ap))
        hipLaunchKernelGGL((diff_update_kernel<4, MODE>), state_grid(n, B, 4), dim3(DIFF_THREADS), 0, s, x, r, p, Ap, coef,
                           frozen, n, B, part);
    else
        hipLaunchKernelGGL((diff_update_kernel<1, MODE>), state_grid(n, B, 1), dim3(DIFF_THREADS), 0, s, x, r, p, Ap, coef,
                           frozen, n, B, part);
}

template <int MODE>
void launch_finish(const float* part, int nblk, int B, float* rr, float* coef, int32_t* frozen, hipStream_t s) {
    hipLaunchKernelGGL(diff_finish_kernel<MODE>, dim3((unsigned)grl_ceil_div(B, DIFF_THREADS)), dim3(DIFF_THREADS), 0, s,
                       part, nblk, B, rr, coef, frozen);
}

inline int64_t pad4(int64_t v) { return (v + 3) / 4 * 4; }                 // keeps every workspace array 16-byte aligned

inline bool graph_args_ok(int n, int k, int64_t ldg) { return n > 0 && k >= 1 && k <= DIFF_K_MAX && ldg >= k; }

}  // namespace

extern "C" int grl_diffusion_part_rows(void) { return DIFF_ROWS; }

extern "C" int grl_diffusion_mutual(const int64_t* sidx, const float* sdist, int64_t ldl, int n, int k, int gamma,
                                    int32_t* idx, float* weight, int64_t ldo, float* deg, void* stream) {
    GRL_REQUIRE(sidx && sdist && idx && weight && deg, "diffusion_mutual: null");
    if (k < 1 || k > DIFF_K_MAX) return grl_fail(GRL_EINVAL, "diffusion_mutual: k = %d (1..%d)", k, DIFF_K_MAX);
    if (gamma < 1 || gamma > DIFF_GAMMA_MAX)
        return grl_fail(GRL_EINVAL, "diffusion_mutual: gamma = %d (1..%d)", gamma, DIFF_GAMMA_MAX);
    GRL_REQUIRE(n > 0 && ldl >= (int64_t)k + 1 && ldo >= k, "diffusion_mutual: bad shape");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(diff_mutual_kernel, dim3((unsigned)grl_ceil_div(n, DIFF_WAVES)), dim3(DIFF_THREADS), 0, s, sidx,
                       sdist, ldl, n, k, gamma, idx, weight, ldo, deg);
    hipLaunchKernelGGL(diff_normalise_kernel, dim3((unsigned)grid_for((int64_t)n * k, DIFF_THREADS)), dim3(DIFF_THREADS), 0,
                       s, idx, weight, ldo, n, k, deg);
    return grl_check_launch("grl_diffusion_mutual");
}

extern "C" int grl_diffusion_apply(const int32_t* idx, const float* S, int64_t ldg, int n, int k, const float* p, int B,
                                   float alpha, float* Ap, float* part, void* stream) {
    GRL_REQUIRE(idx && S && p && Ap && part, "diffusion_apply: null");
    GRL_REQUIRE(graph_args_ok(n, k, ldg) && B > 0, "diffusion_apply: bad shape");
    GRL_REQUIRE(p != Ap, "diffusion_apply: Ap must not be p");
    launch_apply(idx, S, ldg, n, k, p, B, alpha, Ap, part, (hipStream_t)stream);
    return grl_check_launch("grl_diffusion_apply");
}

extern "C" int grl_diffusion_seed(const int64_t* seed_idx, const float* seed_val, int64_t lds, int B, int kq, int n,
                                  int gamma, float* y, void* stream) {
    GRL_REQUIRE(seed_idx && seed_val && y, "diffusion_seed: null");
    GRL_REQUIRE(n > 0 && B > 0 && kq >= 1 && lds >= kq, "diffusion_seed: bad shape");
    if (gamma < 0 || gamma > DIFF_GAMMA_MAX)
        return grl_fail(GRL_EINVAL, "diffusion_seed: gamma = %d (0..%d)", gamma, DIFF_GAMMA_MAX);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(y, 0, (size_t)n * B * sizeof(float), s) != hipSuccess)
        return grl_fail(GRL_ELAUNCH, "diffusion_seed: hipMemsetAsync failed");
    hipLaunchKernelGGL(diff_seed_kernel, dim3((unsigned)grl_ceil_div(B, DIFF_THREADS)), dim3(DIFF_THREADS), 0, s, seed_idx,
                       seed_val, lds, B, kq, n, gamma, y);
    return grl_check_launch("grl_diffusion_seed");
}

extern "C" int64_t grl_diffusion_workspace_floats(int n, int B) {
    if (n <= 0 || B <= 0) return 0;
    const int64_t nb = pad4((int64_t)n * B), nblk = grl_ceil_div(n, DIFF_ROWS);
    return 2 * nb + pad4(nblk * B) + 3 * pad4(B);
}

extern "C" int grl_diffusion_solve(const int32_t* idx, const float* S, int64_t ldg, int n, int k, float* y, int B,
                                   float alpha, int n_iter, float* x, float* ws, void* stream) {
    GRL_REQUIRE(idx && S && y && x && ws, "diffusion_solve: null");
    GRL_REQUIRE(graph_args_ok(n, k, ldg) && B > 0, "diffusion_solve: bad shape");
    if (!(alpha >= 0.f && alpha < 1.f)) return grl_fail(GRL_EINVAL, "diffusion_solve: alpha = %g ([0, 1))", (double)alpha);
    if (n_iter < 0) return grl_fail(GRL_EINVAL, "diffusion_solve: n_iter = %d (>= 0)", n_iter);
    GRL_REQUIRE(aligned16(ws), "diffusion_solve: the workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = (int64_t)n * B;
    const int nblk = grl_ceil_div(n, DIFF_ROWS);
    float* r = y;                                                // r0 = y, in place
    float* p = ws;
    float* Ap = p + pad4(nb);
    float* part = Ap + pad4(nb);
    float* rr = part + pad4((int64_t)nblk * B);
    float* coef = rr + pad4(B);
    int32_t* frozen = reinterpret_cast<int32_t*>(coef + pad4(B));
    if (hipMemsetAsync(x, 0, (size_t)nb * sizeof(float), s) != hipSuccess)
        return grl_fail(GRL_ELAUNCH, "diffusion_solve: hipMemsetAsync failed");
    if (n_iter == 0) return grl_check_launch("grl_diffusion_solve");
    if (hipMemcpyAsync(p, y, (size_t)nb * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
        return grl_fail(GRL_ELAUNCH, "diffusion_solve: hipMemcpyAsync failed");
    launch_update<0>(x, r, p, Ap, coef, frozen, n, B, part, s);
    launch_finish<0>(part, nblk, B, rr, coef, frozen, s);
    for (int it = 0; it < n_iter; ++it) {
        launch_apply(idx, S, ldg, n, k, p, B, alpha, Ap, part, s);
        launch_finish<1>(part, nblk, B, rr, coef, frozen, s);
        launch_update<1>(x, r, p, Ap, coef, frozen, n, B, part, s);
        if (it + 1 == n_iter) break;                             // the last p is never used
        launch_finish<2>(part, nblk, B, rr, coef, frozen, s);
        launch_update<2>(x, r, p, Ap, coef, frozen, n, B, part, s);
    }
    return grl_check_launch("grl_diffusion_solve");
}

extern "C" int grl_diffusion_transpose(const float* x, int n, int B, int negate, float* out, int64_t ldo, void* stream) {
    GRL_REQUIRE(x && out, "diffusion_transpose: null");
    GRL_REQUIRE(n > 0 && B > 0 && ldo >= n, "diffusion_transpose: bad shape");
    hipLaunchKernelGGL(diff_transpose_kernel, dim3((unsigned)grl_ceil_div(n, 64), (unsigned)grl_ceil_div(B, 64)),
                       dim3(DIFF_THREADS), 0, (hipStream_t)stream, x, n, B, negate, out, ldo);
    return grl_check_launch("grl_diffusion_transpose");
}
