// The small dense linear algebra of the randomised subspace-iteration PCA (engine.pca / pca_eigh / pca_orthonormalize,
// DESIGN.md 4z).  The two tall products of a fit are the library's fp32 GEMMs (grl_conv_gemm_f32, grl_conv_wgrad_f32);
// what is here sits between them, on matrices with L <= 512 rows: the Cholesky factor of a Gram matrix, the triangular
// solve that orthonormalises the rows with it (CholeskyQR), the cyclic Jacobi eigensolver of the L x L Rayleigh-Ritz
// matrix, and the rank-one corrections that stand in for a centred copy of the features.
//
// No grid-wide barrier anywhere: a factorisation is ONE workgroup synchronised by __syncthreads() (whose fence orders
// the workgroup's global stores before its later loads: the L x L matrix lives in global memory, 1 MB at most, and
// stays in L2), the tall work (grl_pca_trsm, the corrections) is independent per column.  Every loop has a bound fixed
// at launch.  Every sum has one stated fp32 order, every operation is rounded on its own (no contraction: the
// library's flags), a division and a square root are IEEE's; no atomics.  The same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/grl_hip.h"
#include "common.h"

namespace {

constexpr int PC_LMAX = GRL_PCA_LMAX;
constexpr int PC_NB = 32;                  // panel width of the Cholesky factorisation and the triangular solve
constexpr int PC_LD = PC_NB + 1;           // LDS row pitch of a 32-wide panel: rows 33 floats apart fall on different banks
constexpr int PC_THREADS = 1024;           // the one workgroup of a factorisation
constexpr int PC_WAVES = PC_THREADS / 64;
constexpr int PC_SWEEPS = GRL_PCA_MAX_SWEEPS;

__device__ __forceinline__ bool pc_finite(float v) { return fabsf(v) < INFINITY; }        // (false for a NaN)

// ---- Cholesky --------------------------------------------------------------------------------------------------
// G = R R^T in place on the lower triangle (the strict upper triangle is neither read nor written), left-looking by
// panels of 32 columns.  R[i][k] = (G[i][k] - sum_{j<k} R[i][j] * R[k][j]) / R[k][k] for i > k and R[k][k] = sqrtf(G[k][k]
// - sum_{j<k} R[k][j] * R[k][j]): the sum is taken term by term in ascending j, each product rounded, then subtracted
// from the running value that starts at G[i][k].  The panel [L - k0][32] sits in LDS; the columns left of it stream
// through a second LDS array 32 at a time (both of L rows: 2 * 512 * 33 * 4 = 135168 bytes at L = 512).
__global__ __launch_bounds__(PC_THREADS) void pc_cholesky_kernel(float* g, int ldg, int L, float rel_tol,
                                                                 GrlPcaRecord* rec) {
    extern __shared__ float pc_smem[];
    float* P = pc_smem;                    // the panel:           P[i * 33 + c] = column k0 + c of row i
    float* A = pc_smem + L * PC_LD;        // the earlier columns: A[i * 33 + jj] = column j0 + jj of row i
    __shared__ float s_diag[PC_LMAX], s_red[PC_LMAX];          // G's own diagonal, kept for the pivot test; its maximum
    __shared__ float s_dmax, s_min, s_r;
    __shared__ int s_bad, s_badk;
    const int tid = threadIdx.x;

    // the largest diagonal entry of G (a maximum has no order; a NaN is passed over and met again as a pivot)
    for (int i = tid; i < PC_LMAX; i += PC_THREADS) s_diag[i] = s_red[i] = i < L ? g[(int64_t)i * ldg + i] : -INFINITY;
    __syncthreads();
    for (int s = PC_LMAX / 2; s > 0; s >>= 1) {
        if (tid < s) s_red[tid] = fmaxf(s_red[tid], s_red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) { s_dmax = s_red[0]; s_min = INFINITY; s_bad = 0; s_badk = -1; }
    __syncthreads();
    const float dmax = s_dmax;

    for (int k0 = 0; k0 < L; k0 += PC_NB) {
        const int nb = min(PC_NB, L - k0), rows = L - k0;
        for (int e = tid; e < rows * PC_NB; e += PC_THREADS) {
            const int i = k0 + e / PC_NB, c = e % PC_NB;
            P[i * PC_LD + c] = c < nb ? g[(int64_t)i * ldg + k0 + c] : 0.f;
        }
        for (int j0 = 0; j0 < k0; j0 += PC_NB) {
            __syncthreads();               // (the panel is loaded, the previous chunk is read)
            for (int e = tid; e < rows * PC_NB; e += PC_THREADS) {
                const int i = k0 + e / PC_NB, jj = e % PC_NB;
                A[i * PC_LD + jj] = g[(int64_t)i * ldg + j0 + jj];
            }
            __syncthreads();
            for (int e = tid; e < rows * PC_NB; e += PC_THREADS) {
                const int i = k0 + e / PC_NB, c = e % PC_NB;
                if (c >= nb || k0 + c > i) continue;
                const float* ai = A + i * PC_LD;
                const float* ak = A + (k0 + c) * PC_LD;
                float v = P[i * PC_LD + c];
#pragma unroll
                for (int jj = 0; jj < PC_NB; ++jj) v -= ai[jj] * ak[jj];
                P[i * PC_LD + c] = v;
            }
        }
        __syncthreads();
        // the panel's own columns, one at a time
        for (int c = 0; c < nb; ++c) {
            const int k = k0 + c;
            if (tid == 0) {
                const float piv = P[k * PC_LD + c];
                const bool fin = pc_finite(piv) && pc_finite(dmax);
                if (fin && dmax > 0.f) s_min = fminf(s_min, piv / dmax);
                if (fin && piv > 0.f && piv > rel_tol * s_diag[k]) s_r = sqrtf(piv);
                else { s_bad = fin ? GRL_PCA_PIVOT_SMALL : GRL_PCA_PIVOT_NONFINITE; s_badk = k; }
            }
            __syncthreads();
            if (s_bad) break;              // (uniform: every thread reads the same word)
            const float r = s_r;
            for (int i = k + 1 + tid; i < L; i += PC_THREADS) P[i * PC_LD + c] = P[i * PC_LD + c] / r;
            if (tid == 0) P[k * PC_LD + c] = r;
            __syncthreads();
            for (int e = tid; e < (L - k - 1) * PC_NB; e += PC_THREADS) {
                const int i = k + 1 + e / PC_NB, c2 = e % PC_NB;
                if (c2 > c && c2 < nb && i >= k0 + c2)
                    P[i * PC_LD + c2] -= P[i * PC_LD + c] * P[(k0 + c2) * PC_LD + c];
            }
            __syncthreads();
        }
        const int bad = s_bad, badk = s_badk;
        // A bad pivot ends the factorisation: column badk and all after it become the identity's, so that the solve
        // that follows stays finite on finite input (rows badk.. come out orthogonal to the rows before, not normalised).
        for (int e = tid; e < rows * PC_NB; e += PC_THREADS) {
            const int i = k0 + e / PC_NB, c = e % PC_NB;
            if (c >= nb || k0 + c > i) continue;
            g[(int64_t)i * ldg + k0 + c] = (bad && k0 + c >= badk) ? (i == k0 + c ? 1.f : 0.f) : P[i * PC_LD + c];
        }
        if (bad) {
            for (int64_t e = tid; e < (int64_t)L * L; e += PC_THREADS) {
                const int i = (int)(e / L), c = (int)(e % L);
                if (c >= k0 + PC_NB && c <= i) g[(int64_t)i * ldg + c] = i == c ? 1.f : 0.f;
            }
            break;
        }
        __syncthreads();                   // (the factor's columns are in global memory for the next panel)
    }
    if (tid == 0) {                        // the sticky record: the smallest ratio of all calls, the first failure
        rec->min_pivot = fminf(rec->min_pivot, s_min);
        if (rec->status == 0 && s_bad) { rec->status = s_bad; rec->index = s_badk; rec->call = rec->calls; }
        rec->calls += 1;
    }
}

// ---- triangular solve ------------------------------------------------------------------------------------------
// W <- R^-1 W by forward substitution, one lane per column of W: y_i = (w_i - sum_{k<i} R[i][k] * y_k) / R[i][i], the
// sum term by term in ascending k.  32 rows at a time in registers; the rows above are the lane's own earlier stores,
// read back from global memory (coalesced across the wave, as every access to W is); R comes through LDS in 32 x 32
// blocks, read as broadcasts.  One wave per workgroup: the barriers cost nothing and the columns spread over the grid.
__global__ __launch_bounds__(64) void pc_trsm_kernel(const float* __restrict__ r, int ldr, float* w, int64_t ldw, int L,
                                                     int m) {
    __shared__ float Rs[PC_NB][PC_LD];
    const int lane = threadIdx.x;
    const int64_t col = (int64_t)blockIdx.x * 64 + lane;
    const bool active = col < m;
    float* wc = w + (active ? col : 0);
    for (int i0 = 0; i0 < L; i0 += PC_NB) {
        float acc[PC_NB];
#pragma unroll
        for (int ii = 0; ii < PC_NB; ++ii) acc[ii] = (active && i0 + ii < L) ? wc[(int64_t)(i0 + ii) * ldw] : 0.f;
        for (int k0 = 0; k0 < i0; k0 += PC_NB) {
            __syncthreads();
            for (int e = lane; e < PC_NB * PC_NB; e += 64) {
                const int ii = e / PC_NB, kk = e % PC_NB;
                Rs[ii][kk] = i0 + ii < L ? r[(int64_t)(i0 + ii) * ldr + k0 + kk] : 0.f;
            }
            __syncthreads();
#pragma unroll 2
            for (int kk = 0; kk < PC_NB; ++kk) {
                const float y = active ? wc[(int64_t)(k0 + kk) * ldw] : 0.f;
#pragma unroll
                for (int ii = 0; ii < PC_NB; ++ii) acc[ii] -= Rs[ii][kk] * y;
            }
        }
        __syncthreads();
        for (int e = lane; e < PC_NB * PC_NB; e += 64) {
            const int ii = e / PC_NB, kk = e % PC_NB;
            Rs[ii][kk] = (i0 + ii < L && kk <= ii) ? r[(int64_t)(i0 + ii) * ldr + i0 + kk] : (ii == kk ? 1.f : 0.f);
        }
        __syncthreads();
#pragma unroll
        for (int ii = 0; ii < PC_NB; ++ii) {
#pragma unroll
            for (int kk = 0; kk < ii; ++kk) acc[ii] -= Rs[ii][kk] * acc[kk];
            acc[ii] = acc[ii] / Rs[ii][ii];
        }
#pragma unroll
        for (int ii = 0; ii < PC_NB; ++ii)
            if (active && i0 + ii < L) wc[(int64_t)(i0 + ii) * ldw] = acc[ii];
    }
}

// ---- Jacobi ----------------------------------------------------------------------------------------------------
// The block order of a sum over positions e = 0, 1, ..: 1024 partial sums, partial t the sequential sum from +0.0f in
// ascending e of the terms with e % 1024 == t, then part[t] += part[t + s], t < s, for s = 512, 256, .., 1.
__device__ __forceinline__ float pc_block_fold(float v, float* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = PC_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// the sum of the squares of the entries of a [L][L] (with_diag) or of its off-diagonal entries, in the block order over
// the position e = i * L + j (a diagonal entry that is left out is skipped)
__device__ __forceinline__ float pc_sumsq(const float* a, int lda, int L, bool with_diag, float* red) {
    float part = 0.f;
    for (int e = threadIdx.x; e < L * L; e += PC_THREADS) {
        const int i = e / L, j = e % L;
        if (with_diag || i != j) { const float v = a[(int64_t)i * lda + j]; part += v * v; }
    }
    return pc_block_fold(part, red);
}

// Cyclic Jacobi on the symmetric a [L][L] (its upper triangle is what is read: the lower one is overwritten with it),
// destroyed; vt = the transposed eigenvector matrix (rows = eigenvectors), then sorted into lam / vt_out.
// A sweep is ne - 1 rounds (ne = L, or L + 1 when L is odd: the extra index pairs with nobody) of ne / 2 disjoint pairs,
// the round-robin of the circle method: in round r pair 0 is {ne - 1, r}, pair k is {(r + k) % (ne - 1), (r - k + ne - 1)
// % (ne - 1)}; p < q.  A pair with |a_pq| <= thr = (|A|_F * 2^-26) / L is passed over; otherwise theta = (a_qq - a_pp) /
// (2 a_pq), t = sign(theta) / (|theta| + sqrtf(theta * theta + 1)), c = 1 / sqrtf(t * t + 1), s = t * c, tau = s / (1 + c).
// The round's rotations commute (disjoint pairs): first every row pair of a and vt, (x_p, x_q) <- (x_p - s * (x_q + tau *
// x_p), x_q + s * (x_p - tau * x_q)), then every column pair of a the same way, the four entries of the pair itself set
// to a_pp - t a_pq, a_qq + t a_pq and 0.  (The form with tau is Rutishauser's: 1 - c = s tau is kept to full precision,
// where c itself rounds to 1 for |t| < 2^-12 and c x_p - s x_q would stretch the vectors by t^2 / 2 per rotation -- 2e-5
// of accumulated length at L = 130 in the numpy model, 5e-7 in this form.)  The loop ends after the first sweep that
// rotates nothing, or after 30.
__global__ __launch_bounds__(PC_THREADS) void pc_eigh_kernel(float* a, int lda, float* vt, int ldv, int L,
                                                             float* __restrict__ lam, float* __restrict__ vt_out,
                                                             int ldo, GrlPcaEighInfo* info) {
    __shared__ float red[PC_THREADS];
    __shared__ float s_tau[PC_LMAX / 2], s_s[PC_LMAX / 2], s_pp[PC_LMAX / 2], s_qq[PC_LMAX / 2];
    __shared__ int s_p[PC_LMAX / 2], s_q[PC_LMAX / 2], s_rank[PC_LMAX];
    __shared__ int s_any;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int e = tid; e < L * L; e += PC_THREADS) {
        const int i = e / L, j = e % L;
        vt[(int64_t)i * ldv + j] = i == j ? 1.f : 0.f;
        if (i > j) a[(int64_t)i * lda + j] = a[(int64_t)j * lda + i];
    }
    if (tid == 0) s_any = 0;
    __syncthreads();
    const float fro = sqrtf(pc_sumsq(a, lda, L, true, red));
    const float thr = (fro * 0x1p-26f) / (float)L;          // (a NaN or infinite norm: no pair passes, no rotation)
    const int ne = L + (L & 1), npairs = ne / 2, nrounds = ne - 1;
    int sweeps = 0;
    for (int sw = 0; sw < PC_SWEEPS; ++sw) {
        for (int r = 0; r < nrounds; ++r) {
            if (tid < npairs) {
                const int k = tid;
                const int x = k == 0 ? ne - 1 : (r + k) % (ne - 1);
                const int y = k == 0 ? r : (r + ne - 1 - k) % (ne - 1);
                const int p = min(x, y), q = max(x, y);
                int pp = -1;
                if (q < L) {
                    const float apq = a[(int64_t)p * lda + q];
                    if (fabsf(apq) > thr && pc_finite(apq)) {
                        const float app = a[(int64_t)p * lda + p], aqq = a[(int64_t)q * lda + q];
                        const float theta = (aqq - app) / (2.f * apq);
                        const float t = copysignf(1.f, theta) / (fabsf(theta) + sqrtf(theta * theta + 1.f));
                        const float c = 1.f / sqrtf(t * t + 1.f);
                        s_s[k] = t * c; s_tau[k] = (t * c) / (1.f + c);
                        s_pp[k] = app - t * apq; s_qq[k] = aqq + t * apq;
                        pp = p;
                        s_any = 1;                             // (every writer stores the same word)
                    }
                }
                s_p[k] = pp; s_q[k] = q;
            }
            __syncthreads();
            for (int k = wave; k < npairs; k += PC_WAVES) {   // rows p and q of a and of vt: a wave per pair
                const int p = s_p[k];
                if (p < 0) continue;
                const float tau = s_tau[k], s = s_s[k];
                float* ap = a + (int64_t)p * lda;
                float* aq = a + (int64_t)s_q[k] * lda;
                float* vp = vt + (int64_t)p * ldv;
                float* vq = vt + (int64_t)s_q[k] * ldv;
                for (int j = lane; j < L; j += 64) {
                    const float xp = ap[j], xq = aq[j];
                    ap[j] = xp - s * (xq + tau * xp);
                    aq[j] = xq + s * (xp - tau * xq);
                    const float yp = vp[j], yq = vq[j];
                    vp[j] = yp - s * (yq + tau * yp);
                    vq[j] = yq + s * (yp - tau * yq);
                }
            }
            __syncthreads();
            for (int i = wave; i < L; i += PC_WAVES) {        // columns p and q of a: a wave per row, a lane per pair
                float* ai = a + (int64_t)i * lda;
                for (int k = lane; k < npairs; k += 64) {
                    const int p = s_p[k];
                    if (p < 0) continue;
                    const int q = s_q[k];
                    if (i == p) { ai[p] = s_pp[k]; ai[q] = 0.f; }
                    else if (i == q) { ai[p] = 0.f; ai[q] = s_qq[k]; }
                    else {
                        const float tau = s_tau[k], s = s_s[k];
                        const float xp = ai[p], xq = ai[q];
                        ai[p] = xp - s * (xq + tau * xp);
                        ai[q] = xq + s * (xp - tau * xq);
                    }
                }
            }
            __syncthreads();
        }
        const int any = s_any;
        __syncthreads();
        if (tid == 0) s_any = 0;
        __syncthreads();
        if (!any) break;
        ++sweeps;
    }
    const float off = sqrtf(pc_sumsq(a, lda, L, false, red));
    // eigenvalues descending, equal ones by their index; a NaN sorts last
    if (tid < L) { const float v = a[(int64_t)tid * lda + tid]; red[tid] = v == v ? v : -INFINITY; }
    __syncthreads();
    if (tid < L) {
        const float v = red[tid];
        int rank = 0;
        for (int j = 0; j < L; ++j) rank += (red[j] > v || (red[j] == v && j < tid)) ? 1 : 0;
        s_rank[tid] = rank;
        lam[rank] = a[(int64_t)tid * lda + tid];
    }
    __syncthreads();
    for (int i = wave; i < L; i += PC_WAVES)
        for (int j = lane; j < L; j += 64) vt_out[(int64_t)s_rank[i] * ldo + j] = vt[(int64_t)i * ldv + j];
    if (tid == 0) { info->sweeps = sweeps; info->off = off; info->fro = fro; info->reserved = 0; }
}

// ---- the small kernels -----------------------------------------------------------------------------------------
// out[i] = the sum of row i of w [rows][ld] over its m columns in the wave order of DESIGN.md 4w (64 partial sums by
// column % 64, each sequential from +0.0f, folded part[l] += part[l ^ s], s = 32 .. 1): a wave per row
__global__ __launch_bounds__(256) void pc_rowsum_kernel(const float* __restrict__ w, int64_t ld, int rows, int m,
                                                        float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (i >= rows) return;
    const float* __restrict__ wr = w + (int64_t)i * ld;
    float part = 0.f;
    for (int j = lane; j < m; j += 64) part += wr[j];
    part = wave_sum(part);
    if (lane == 0) out[i] = part;
}

// w[i][j] = w[i][j] - s[i] * mu[j]: the rank-one term that a product with the centred features differs by
__global__ __launch_bounds__(256) void pc_rank1_kernel(float* __restrict__ w, int64_t ld, int rows, int m,
                                                       const float* __restrict__ s, const float* __restrict__ mu) {
    const int i = blockIdx.y;
    const float si = s[i];
    float* __restrict__ wr = w + (int64_t)i * ld;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < m; j += gridDim.x * 256) wr[j] = wr[j] - si * mu[j];
}

// row i of c [rows][ld] times -1 when its entry of largest magnitude (the lowest column among equals) is negative
__global__ __launch_bounds__(256) void pc_sign_kernel(float* __restrict__ c, int64_t ld, int d) {
    __shared__ float s_v[256];
    __shared__ int s_j[256];
    float* __restrict__ cr = c + (int64_t)blockIdx.x * ld;
    const int tid = threadIdx.x;
    float best = -1.f;
    int bj = d;
    for (int j = tid; j < d; j += 256) {
        const float v = fabsf(cr[j]);
        if (v > best) { best = v; bj = j; }                    // (ascending j: the first of equals stays)
    }
    s_v[tid] = best; s_j[tid] = bj;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s && (s_v[tid + s] > s_v[tid] || (s_v[tid + s] == s_v[tid] && s_j[tid + s] < s_j[tid]))) {
            s_v[tid] = s_v[tid + s]; s_j[tid] = s_j[tid + s];
        }
        __syncthreads();
    }
    const int j0 = s_j[0];
    if (j0 >= d || !(cr[j0] < 0.f)) return;                    // (uniform: every thread reads the same entry)
    __syncthreads();
    for (int j = tid; j < d; j += 256) cr[j] = -cr[j];
}

// scale[i] = lam ? 1 / sqrtf(lam[i]) : 1, shift[i] = -(cm[i] * scale[i]): the GEMM epilogue of the transform
__global__ __launch_bounds__(256) void pc_affine_kernel(const float* __restrict__ cm, const float* __restrict__ lam,
                                                        int r, float* __restrict__ scale, float* __restrict__ shift) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= r) return;
    const float sc = lam ? 1.0f / sqrtf(lam[i]) : 1.0f;
    scale[i] = sc;
    shift[i] = -(cm[i] * sc);
}

// out[i][j] = y[i][j] * sqrtf(lam[j]): the whitening undone
__global__ __launch_bounds__(256) void pc_colscale_kernel(const float* __restrict__ y, int64_t ldy, int rows, int r,
                                                          const float* __restrict__ lam, float* __restrict__ out,
                                                          int64_t ldo) {
    const int64_t total = (int64_t)rows * r;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t i = e / r;
        const int j = (int)(e % r);
        out[i * ldo + j] = y[i * ldy + j] * sqrtf(lam[j]);
    }
}

// scikit-learn's init='pca' scaling of y [rows][2]: mean = sum(y[:, 0]) / rows, var = sum((y[i][0] - mean)^2) / rows
// (both sums in the block order over i), out = y / sqrtf(var) * 1e-4f
__global__ __launch_bounds__(PC_THREADS) void pc_tsne_init_kernel(const float* __restrict__ y, int64_t ldy, int rows,
                                                                  float* __restrict__ out) {
    __shared__ float red[PC_THREADS];
    float part = 0.f;
    for (int i = threadIdx.x; i < rows; i += PC_THREADS) part += y[(int64_t)i * ldy];
    const float mean = pc_block_fold(part, red) / (float)rows;
    part = 0.f;
    for (int i = threadIdx.x; i < rows; i += PC_THREADS) { const float t = y[(int64_t)i * ldy] - mean; part += t * t; }
    const float sd = sqrtf(pc_block_fold(part, red) / (float)rows);
    for (int e = threadIdx.x; e < 2 * rows; e += PC_THREADS)
        out[e] = y[(int64_t)(e >> 1) * ldy + (e & 1)] / sd * 1e-4f;
}

}  // namespace

extern "C" int grl_pca_cholesky(float* g, int ldg, int L, float rel_tol, GrlPcaRecord* record, void* stream) {
    GRL_REQUIRE(L >= 1 && L <= PC_LMAX && ldg >= L, "pca_cholesky: 1 <= L <= 512 and ldg >= L");
    GRL_REQUIRE(g && record, "pca_cholesky: null");
    GRL_REQUIRE(rel_tol >= 0.f, "pca_cholesky: rel_tol >= 0");
    const int lds = 2 * L * PC_LD * (int)sizeof(float);
    if (lds > 48 * 1024)
        (void)hipFuncSetAttribute((const void*)pc_cholesky_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(pc_cholesky_kernel, dim3(1), dim3(PC_THREADS), lds, (hipStream_t)stream, g, ldg, L, rel_tol, record);
    return grl_check_launch("grl_pca_cholesky");
}

extern "C" int grl_pca_trsm(const float* r, int ldr, float* w, int64_t ldw, int L, int m, void* stream) {
    GRL_REQUIRE(L >= 1 && L <= PC_LMAX && ldr >= L && m >= 0 && ldw >= m, "pca_trsm: 1 <= L <= 512, ldr >= L, ldw >= m >= 0");
    if (m == 0) return GRL_OK;
    GRL_REQUIRE(r && w, "pca_trsm: null");
    hipLaunchKernelGGL(pc_trsm_kernel, dim3(grl_ceil_div(m, 64)), dim3(64), 0, (hipStream_t)stream, r, ldr, w, ldw, L, m);
    return grl_check_launch("grl_pca_trsm");
}

extern "C" int grl_pca_eigh(float* a, int lda, float* vt_work, int ldv, int L, float* lam, float* vt, int ldvt,
                            GrlPcaEighInfo* info, void* stream) {
    GRL_REQUIRE(L >= 1 && L <= PC_LMAX && lda >= L && ldv >= L && ldvt >= L, "pca_eigh: 1 <= L <= 512 and every ld >= L");
    GRL_REQUIRE(a && vt_work && lam && vt && info, "pca_eigh: null");
    GRL_REQUIRE(vt_work != vt && vt_work != a && vt != a, "pca_eigh: a, vt_work and vt are three buffers");
    hipLaunchKernelGGL(pc_eigh_kernel, dim3(1), dim3(PC_THREADS), 0, (hipStream_t)stream, a, lda, vt_work, ldv, L, lam, vt,
                       ldvt, info);
    return grl_check_launch("grl_pca_eigh");
}

extern "C" int grl_pca_rowsum(const float* w, int64_t ld, int rows, int m, float* out, void* stream) {
    GRL_REQUIRE(rows >= 0 && m >= 0 && ld >= m, "pca_rowsum: rows >= 0 and ld >= m >= 0");
    if (rows == 0) return GRL_OK;
    GRL_REQUIRE(out && (w || m == 0), "pca_rowsum: null");
    hipLaunchKernelGGL(pc_rowsum_kernel, dim3(grl_ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, w, ld, rows, m, out);
    return grl_check_launch("grl_pca_rowsum");
}

extern "C" int grl_pca_rank1(float* w, int64_t ld, int rows, int m, const float* s, const float* mu, void* stream) {
    GRL_REQUIRE(rows >= 0 && rows <= 65535 && m >= 0 && ld >= m, "pca_rank1: 0 <= rows <= 65535 and ld >= m >= 0");
    if (rows == 0 || m == 0) return GRL_OK;
    GRL_REQUIRE(w && s && mu, "pca_rank1: null");
    hipLaunchKernelGGL(pc_rank1_kernel, dim3(grid_for(m), rows), dim3(256), 0, (hipStream_t)stream, w, ld, rows, m, s, mu);
    return grl_check_launch("grl_pca_rank1");
}

extern "C" int grl_pca_sign(float* c, int64_t ld, int rows, int d, void* stream) {
    GRL_REQUIRE(rows >= 0 && d >= 1 && ld >= d, "pca_sign: rows >= 0 and ld >= d >= 1");
    if (rows == 0) return GRL_OK;
    GRL_REQUIRE(c, "pca_sign: null");
    hipLaunchKernelGGL(pc_sign_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, c, ld, d);
    return grl_check_launch("grl_pca_sign");
}

extern "C" int grl_pca_affine(const float* cm, const float* lam, int r, float* scale, float* shift, void* stream) {
    GRL_REQUIRE(r >= 1 && cm && scale && shift, "pca_affine: r >= 1, cm, scale and shift");
    hipLaunchKernelGGL(pc_affine_kernel, dim3(grl_ceil_div(r, 256)), dim3(256), 0, (hipStream_t)stream, cm, lam, r, scale,
                       shift);
    return grl_check_launch("grl_pca_affine");
}

extern "C" int grl_pca_colscale(const float* y, int64_t ldy, int rows, int r, const float* lam, float* out, int64_t ldo,
                                void* stream) {
    GRL_REQUIRE(rows >= 0 && r >= 1 && ldy >= r && ldo >= r, "pca_colscale: rows >= 0, r >= 1, ldy and ldo >= r");
    if (rows == 0) return GRL_OK;
    GRL_REQUIRE(y && lam && out, "pca_colscale: null");
    hipLaunchKernelGGL(pc_colscale_kernel, dim3(grid_for((int64_t)rows * r)), dim3(256), 0, (hipStream_t)stream, y, ldy,
                       rows, r, lam, out, ldo);
    return grl_check_launch("grl_pca_colscale");
}

extern "C" int grl_pca_tsne_init(const float* y, int64_t ldy, int rows, float* out, void* stream) {
    GRL_REQUIRE(rows >= 1 && ldy >= 2 && rows <= (1 << 30), "pca_tsne_init: 1 <= rows <= 2^30 and ldy >= 2");
    GRL_REQUIRE(y && out, "pca_tsne_init: null");
    hipLaunchKernelGGL(pc_tsne_init_kernel, dim3(1), dim3(PC_THREADS), 0, (hipStream_t)stream, y, ldy, rows, out);
    return grl_check_launch("grl_pca_tsne_init");
}
