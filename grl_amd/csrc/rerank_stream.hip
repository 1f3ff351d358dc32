// Streaming k-reciprocal re-ranking (engine.rerank_search / engine.rerank_metrics_streaming):
// the result of rerank.hip without the (q+g)^2 matrices D, V, V2T or an nq x ng array.
//
//   pass A1  per block of samples [i0, i1): the columns S[:, i0:i1] come from the distance GEMM in pieces
//            ("segments", each on one side of the query/gallery boundary); colmax and the D rows are written
//            here with rerank.hip's arithmetic, and grl_topk_block keeps each row's first K = max(k1+1, k2)
//   lists    each sample's expanded k-reciprocal list from the [N][K] rank lists (rr_expansion_list)
//   pass A2  the same segments again: the weights V[i][lidx[i][a]] = exp(-D) / sum, kept sparse [N][256]
//   expand   V2 rows as CSR (sorted union of the k2 nearest samples' lists, zero entries dropped)
//   assemble row_ptr by an exclusive scan of the row counts, shards of other ranks placed at their offsets, and the
//            gallery rows' CSC by a counting transpose whose result does not depend on the order of arrival
//   final    per column block of the q x g distances: F = (1-lambda) * jaccard + lambda * D, in place
//
// Every value is produced by the same fp32 operations, in the same order, as in rerank.hip (the library
// is built with -ffp-contract=off), so the final distances carry its bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "../../include/grl_hip.h"
#include "common.h"
#include "rerank_common.h"
#include "sort_order.h"

namespace {

constexpr int RRS_CHUNK = 2048;               // gallery columns per workgroup of the final pass (LDS accumulator)
constexpr int RRS_UNION = RR_K2MAX * RR_LMAX; // longest concatenation of k2 expansion lists

// One segment of the sample columns [i0, i0 + w): S[r][i0 + c] = up[r * ldu + c] for r < nq, and
// lo[(r - nq) * lrs + c * lcs] for r >= nq (a column block of g x g or the transpose of a row block of q x g).
struct Seg {
    const float* up;
    int64_t ldu;
    const float* lo;
    int64_t lrs, lcs;
    int nq, ng, w;
};

__device__ __forceinline__ float seg_elem(const Seg& s, int r, int c) {
    return r < s.nq ? s.up[(int64_t)r * s.ldu + c] : s.lo[(int64_t)(r - s.nq) * s.lrs + (int64_t)c * s.lcs];
}

// colmax[c] = max_r S[r][i0+c]^2; 64 columns per workgroup, 4 row phases (rr_colmax_kernel)
__global__ __launch_bounds__(256) void rrs_colmax_kernel(Seg s, float* __restrict__ colmax) {
    __shared__ float red[4][64];
    const int N = s.nq + s.ng, c = blockIdx.x * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6;
    float m = -INFINITY;
    if (c < s.w)
        for (int r = ph; r < N; r += 4) {
            const float v = seg_elem(s, r, c);
            m = fmaxf(m, v * v);
        }
    red[ph][threadIdx.x & 63] = m;
    __syncthreads();
    if (ph == 0 && c < s.w) colmax[c] = fmaxf(fmaxf(red[0][threadIdx.x], red[1][threadIdx.x]),
                                              fmaxf(red[2][threadIdx.x], red[3][threadIdx.x]));
}

// D rows: drows[c][j] = S[j][i0+c]^2 / colmax[c], 32 x 32 tiles transposed through LDS (rr_build_kernel)
__global__ __launch_bounds__(256) void rrs_build_kernel(Seg s, const float* __restrict__ colmax,
                                                        float* __restrict__ drows, int64_t ldd) {
    __shared__ float tile[32][33];
    const int N = s.nq + s.ng;
    const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int rr = ty; rr < 32; rr += 8) {
        const int r = j0 + rr, c = i0 + tx;
        float v = 0.f;
        if (r < N && c < s.w) {
            v = seg_elem(s, r, c);
            v = v * v;
        }
        tile[rr][tx] = v;
    }
    __syncthreads();
    for (int rr = ty; rr < 32; rr += 8) {
        const int c = i0 + rr, j = j0 + tx;
        if (c < s.w && j < N) drows[(int64_t)c * ldd + j] = tile[tx][rr] / colmax[c];
    }
}

// One wave per sample: the expanded neighbour list from the rank lists (rr_krecip_kernel without the weights)
__global__ __launch_bounds__(64) void rrs_lists_kernel(const int32_t* __restrict__ rank, int64_t ld, int k1, int half,
                                                       int32_t* __restrict__ lcnt, int32_t* __restrict__ lidx) {
    __shared__ int base[RR_K1MAX + 1];
    __shared__ int raw[RR_LMAX], srt[RR_LMAX];
    __shared__ int n_raw;
    const int i = blockIdx.x, lane = threadIdx.x;
    const int n_u = rr_expansion_list(rank, ld, i, k1, half, lane, base, raw, srt, &n_raw);
    int32_t* li = lidx + (int64_t)i * RR_LMAX;
    for (int a = lane; a < n_u; a += 64) li[a] = raw[a];
    if (lane == 0) lcnt[i] = n_u;
}

// One wave per sample i0 + c of the segment: lval[i][a] = exp(-D[i][e]) / sum over the list, e = lidx[i][a],
// D[i][e] = S[e][i]^2 / colmax[i] (rr_build_kernel, then rr_krecip_kernel)
__global__ __launch_bounds__(64) void rrs_weights_kernel(Seg s, int i0, const float* __restrict__ colmax,
                                                         const int32_t* __restrict__ lcnt,
                                                         const int32_t* __restrict__ lidx, float* __restrict__ lval) {
    __shared__ float w[RR_LMAX];
    const int c = blockIdx.x, i = i0 + c, lane = threadIdx.x;
    const int n_u = lcnt[i];
    const float cm = colmax[i];
    const int32_t* li = lidx + (int64_t)i * RR_LMAX;
    for (int a = lane; a < n_u; a += 64) {
        float v = seg_elem(s, li[a], c);
        v = v * v;
        const float d = v / cm;
        w[a] = expf(-d);
    }
    __syncthreads();
    float total = 0.f;
    if (lane == 0) total = np_pairwise_sum(w, n_u);
    total = __shfl(total, 0);
    float* vi = lval + (int64_t)i * RR_LMAX;
    for (int a = lane; a < n_u; a += 64) vi[a] = w[a] / total;
}

// V[row][e] from the sparse row: the weight, or 0 when e is not in the row's list
__device__ __forceinline__ float sparse_at(const int32_t* __restrict__ lcnt, const int32_t* __restrict__ lidx,
                                           const float* __restrict__ lval, int row, int e) {
    const int32_t* li = lidx + (int64_t)row * RR_LMAX;
    const int lo = lower_bound(li, 0, lcnt[row], e);
    return (lo < lcnt[row] && li[lo] == e) ? lval[(int64_t)row * RR_LMAX + lo] : 0.f;
}

// One workgroup per sample i: V2[i] over the sorted union of its k2 nearest samples' lists,
// V2[i][e] = (sum_u V[rows[u]][e]) / k2 in u order (rr_expand_kernel), non-zero entries only.
// row_ptr == NULL: count them into cnt[i]; otherwise write them to col / val from row_ptr[i] on.  The grid covers
// the samples row0 .. row0 + gridDim.x - 1; cnt and row_ptr are indexed by the sample.
__global__ __launch_bounds__(256) void rrs_expand_kernel(const int32_t* __restrict__ rank, int64_t ld,
                                                         const int32_t* __restrict__ lcnt,
                                                         const int32_t* __restrict__ lidx,
                                                         const float* __restrict__ lval, int k2, int row0,
                                                         const int64_t* __restrict__ row_ptr, int32_t* __restrict__ cnt,
                                                         int32_t* __restrict__ col, float* __restrict__ val) {
    __shared__ int rows[RR_K2MAX];
    __shared__ int offs[RR_K2MAX + 1];
    __shared__ int es[RRS_UNION];
    __shared__ int wcnt[4];
    const int i = row0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) {
        int o = 0;
        for (int t = 0; t < k2; ++t) {
            rows[t] = k2 == 1 ? i : rank[(int64_t)i * ld + t];
            offs[t] = o;
            o += lcnt[rows[t]];
        }
        offs[k2] = o;
    }
    __syncthreads();
    const int total = offs[k2];
    int P = 1;
    while (P < total) P <<= 1;
    for (int a = tid; a < P; a += 256) {
        int e = 0x7fffffff;
        if (a < total) {
            int t = 0;
            while (a >= offs[t + 1]) ++t;
            e = lidx[(int64_t)rows[t] * RR_LMAX + (a - offs[t])];
        }
        es[a] = e;
    }
    __syncthreads();
    bitonic_lds(es, nullptr, P);
    const unsigned long long below = (1ull << lane) - 1ull;
    int n = 0;
    for (int a0 = 0; a0 < total; a0 += 256) {           // ordered compaction, 256 entries per round
        const int a = a0 + tid;
        bool keep = a < total && (a == 0 || es[a] != es[a - 1]);
        float v = 0.f;
        int e = 0;
        if (keep) {
            e = es[a];
            float sum = sparse_at(lcnt, lidx, lval, rows[0], e);
            for (int u = 1; u < k2; ++u) sum += sparse_at(lcnt, lidx, lval, rows[u], e);
            v = k2 == 1 ? sum : sum / (float)k2;
            keep = v != 0.f;
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int p = n;
        for (int w = 0; w < wave; ++w) p += wcnt[w];
        if (keep && row_ptr) {
            const int64_t o = row_ptr[i] + p + __popcll(m & below);
            col[o] = e;
            val[o] = v;
        }
        n += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
    if (tid == 0 && !row_ptr) cnt[i] = n;
}

// One wave per (query q, chunk of RRS_CHUNK columns of the block).  The block holds q x g distances x
// (cosin_dist) of gallery entries col0 .. col0 + ncols; each becomes
//   F = (1 - t / (2 - t)) * one_minus + (x * x / colmax[q]) * lam,
//   t = sum over the non-zero k of V2[q], ascending, of min(V2[q][k], V2[nq + g][k])  (rr_jaccard_kernel).
// The CSC lists of k (gallery samples j with V2[j][k] != 0, ascending j) are cut to the chunk by binary
// search, 64 k at a time (one per lane).  Within one k every j appears once, so the lanes update distinct LDS
// slots; the barrier between two k keeps the ascending-k order of every column's sum.
__global__ __launch_bounds__(64) void rrs_final_kernel(float* __restrict__ d, int64_t ld, int nq, int col0, int ncols,
                                                       const float* __restrict__ colmax,
                                                       const int64_t* __restrict__ q_ptr,
                                                       const int32_t* __restrict__ q_col,
                                                       const float* __restrict__ q_val,
                                                       const int64_t* __restrict__ csc_ptr,
                                                       const int32_t* __restrict__ csc_row,
                                                       const float* __restrict__ csc_val, float lam, float one_minus) {
    __shared__ float acc[RRS_CHUNK];
    const int q = blockIdx.x, lane = threadIdx.x;
    const int c0 = blockIdx.y * RRS_CHUNK, n = min(RRS_CHUNK, ncols - c0);
    const int jlo = nq + col0 + c0, jhi = jlo + n;
    for (int c = lane; c < n; c += 64) acc[c] = 0.f;
    __syncthreads();
    const int64_t qs = q_ptr[q], qe = q_ptr[q + 1];
    for (int64_t a0 = qs; a0 < qe; a0 += 64) {
        const int64_t a = a0 + lane;
        int64_t lo = 0, hi = 0;
        float v = 0.f;
        if (a < qe) {
            const int k = q_col[a];
            v = q_val[a];
            lo = lower_bound(csc_row, csc_ptr[k], csc_ptr[k + 1], jlo);
            hi = lower_bound(csc_row, lo, csc_ptr[k + 1], jhi);
        }
        const int m = (int)min((int64_t)64, qe - a0);
        for (int t = 0; t < m; ++t) {
            const int64_t lt = __shfl(lo, t), ht = __shfl(hi, t);
            const float vt = __shfl(v, t);
            for (int64_t e = lt + lane; e < ht; e += 64) {
                const int c = csc_row[e] - jlo;
                acc[c] = acc[c] + fminf(vt, csc_val[e]);
            }
            __syncthreads();
        }
    }
    const float cm = colmax[q];
    float* dq = d + (int64_t)q * ld + c0;
    for (int c = lane; c < n; c += 64) {
        const float x = dq[c];
        const float sq = x * x;
        const float dist = sq / cm;
        const float t = acc[c];
        const float jac = 1.f - t / (2.f - t);
        dq[c] = jac * one_minus + dist * lam;
    }
}

// ---- CSR / CSC assembly ----------------------------------------------------------------------------------
constexpr int RRS_SCAN_T = 1024;              // one workgroup walks the counts, 1024 per step
constexpr int RRS_RANK_CHUNK = 1024;          // rows of a CSC column staged in LDS at a time

// ptr[i] = cnt[0] + .. + cnt[i-1], i <= n: shuffle scan inside each wave, the 16 wave totals through LDS and a
// running carry from step to step.
__global__ __launch_bounds__(RRS_SCAN_T) void rrs_scan_kernel(const int32_t* __restrict__ cnt, int n,
                                                              int64_t* __restrict__ ptr) {
    __shared__ long long wsum[RRS_SCAN_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long carry = 0;
    for (int base = 0; base < n; base += RRS_SCAN_T) {
        const int i = base + tid;
        const long long v = i < n ? (long long)cnt[i] : 0;
        long long inc = v;
        for (int d = 1; d < 64; d <<= 1) {
            const long long t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        long long off = 0, tot = 0;
        for (int w = 0; w < RRS_SCAN_T / 64; ++w) {
            const long long sw = wsum[w];
            if (w < wave) off += sw;
            tot += sw;
        }
        if (i < n) ptr[i] = carry + off + inc - v;
        carry += tot;
        __syncthreads();
    }
    if (tid == 0) ptr[n] = carry;
}

// The entries of the rows row0 .. row1 - 1, packed from src[0] on, go to col / val at row_ptr[row0]
__global__ __launch_bounds__(256) void rrs_place_kernel(const int32_t* __restrict__ src_col,
                                                        const float* __restrict__ src_val, int64_t cap,
                                                        const int64_t* __restrict__ row_ptr, int row0, int row1,
                                                        int32_t* __restrict__ col, float* __restrict__ val) {
    const int64_t o = row_ptr[row0], n = min(row_ptr[row1] - o, cap);
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        col[o + e] = src_col[e];
        val[o + e] = src_val[e];
    }
}

// One wave per gallery sample j = nq + ..: ccnt[k] += 1 for every column k of its row (integer atomics: the counts
// do not depend on the order)
__global__ __launch_bounds__(256) void rrs_csc_count_kernel(const int64_t* __restrict__ row_ptr,
                                                            const int32_t* __restrict__ col, int nq, int N,
                                                            int32_t* __restrict__ ccnt) {
    const int j = nq + blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= N) return;
    for (int64_t e = row_ptr[j] + lane; e < row_ptr[j + 1]; e += 64) {
        const int k = col[e];
        if ((unsigned)k < (unsigned)N) atomicAdd(&ccnt[k], 1);
    }
}

// The same walk: every entry takes a slot of its column's range [csc_ptr[k], csc_ptr[k+1]) by counting ccnt[k]
// down, so the column's entries arrive in no particular order; rrs_csc_order_kernel puts them in theirs.
__global__ __launch_bounds__(256) void rrs_csc_scatter_kernel(const int64_t* __restrict__ row_ptr,
                                                              const int32_t* __restrict__ col,
                                                              const float* __restrict__ val, int nq, int N,
                                                              const int64_t* __restrict__ csc_ptr,
                                                              int32_t* __restrict__ ccnt, int32_t* __restrict__ tmp_row,
                                                              float* __restrict__ tmp_val) {
    const int j = nq + blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= N) return;
    for (int64_t e = row_ptr[j] + lane; e < row_ptr[j + 1]; e += 64) {
        const int k = col[e];
        if ((unsigned)k >= (unsigned)N) continue;
        const int slot = atomicSub(&ccnt[k], 1) - 1;
        if (slot < 0) continue;                           // cannot happen: the column was counted by the same walk
        const int64_t o = csc_ptr[k] + slot;
        tmp_row[o] = j;
        tmp_val[o] = val[e];
    }
}

// One workgroup per column k: a sample appears at most once in a column, so an entry's place in the ascending
// order is the number of the column's samples below its own.  That number depends on the column's set of entries
// alone, not on where the scatter left them.
__global__ __launch_bounds__(256) void rrs_csc_order_kernel(const int64_t* __restrict__ csc_ptr,
                                                            const int32_t* __restrict__ tmp_row,
                                                            const float* __restrict__ tmp_val,
                                                            int32_t* __restrict__ csc_row, float* __restrict__ csc_val) {
    __shared__ int rows[RRS_RANK_CHUNK];
    const int64_t s = csc_ptr[blockIdx.x], L = csc_ptr[blockIdx.x + 1] - s;
    const int tid = threadIdx.x;
    for (int64_t a0 = 0; a0 < L; a0 += 256) {
        const int64_t a = a0 + tid;
        const int r = a < L ? tmp_row[s + a] : 0;
        int64_t below = 0;
        for (int64_t c0 = 0; c0 < L; c0 += RRS_RANK_CHUNK) {
            const int n = (int)min((int64_t)RRS_RANK_CHUNK, L - c0);
            if (a0 == 0 || L > RRS_RANK_CHUNK) {          // a column of one chunk stays in LDS for every a0
                __syncthreads();
                for (int t = tid; t < n; t += 256) rows[t] = tmp_row[s + c0 + t];
                __syncthreads();
            }
            if (a < L)
                for (int t = 0; t < n; ++t) below += rows[t] < r;
        }
        if (a < L) {
            csc_row[s + below] = r;
            csc_val[s + below] = tmp_val[s + a];
        }
    }
}

Seg make_seg(const float* up, int64_t ldu, const float* lo, int64_t lrs, int64_t lcs, int nq, int ng, int w) {
    Seg s;
    s.up = up; s.ldu = ldu; s.lo = lo; s.lrs = lrs; s.lcs = lcs; s.nq = nq; s.ng = ng; s.w = w;
    return s;
}

}  // namespace

extern "C" int grl_rrs_segment_rows(const float* up, int64_t ldu, const float* lo, int64_t lo_rs, int64_t lo_cs, int nq,
                                    int ng, int w, float* colmax, float* drows, int64_t ldd, void* stream) {
    GRL_REQUIRE(up && lo && colmax && drows && nq > 0 && ng > 0 && w > 0 && ldu >= w && ldd >= (int64_t)nq + ng,
                "rrs_segment_rows: bad args");
    const Seg s = make_seg(up, ldu, lo, lo_rs, lo_cs, nq, ng, w);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rrs_colmax_kernel, dim3(grl_ceil_div(w, 64)), dim3(256), 0, st, s, colmax);
    hipLaunchKernelGGL(rrs_build_kernel, dim3(grl_ceil_div(nq + ng, 32), grl_ceil_div(w, 32)), dim3(256), 0, st, s,
                       colmax, drows, ldd);
    return grl_check_launch("grl_rrs_segment_rows");
}

extern "C" int grl_rrs_lists(const int32_t* rank, int64_t ld, int N, int k1, int32_t* lcnt, int32_t* lidx,
                             void* stream) {
    GRL_REQUIRE(rank && lcnt && lidx && N > 0, "rrs_lists: bad args");
    GRL_REQUIRE(k1 >= 1 && k1 <= RR_K1MAX && k1 < N && ld >= k1 + 1, "rrs_lists: 1 <= k1 <= 20, k1 < N, ld > k1");
    int half = k1 / 2;                                  // int(np.around(k1 / 2.)): round half to even
    if (k1 % 2 == 1 && (half % 2 == 1)) half += 1;
    hipLaunchKernelGGL(rrs_lists_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, rank, ld, k1, half, lcnt, lidx);
    return grl_check_launch("grl_rrs_lists");
}

extern "C" int grl_rrs_weights(const float* up, int64_t ldu, const float* lo, int64_t lo_rs, int64_t lo_cs, int nq,
                               int ng, int w, int i0, const float* colmax, const int32_t* lcnt, const int32_t* lidx,
                               float* lval, void* stream) {
    GRL_REQUIRE(up && lo && colmax && lcnt && lidx && lval && nq > 0 && ng > 0 && w > 0 && i0 >= 0 &&
                (int64_t)i0 + w <= (int64_t)nq + ng && ldu >= w, "rrs_weights: bad args");
    const Seg s = make_seg(up, ldu, lo, lo_rs, lo_cs, nq, ng, w);
    hipLaunchKernelGGL(rrs_weights_kernel, dim3(w), dim3(64), 0, (hipStream_t)stream, s, i0, colmax, lcnt, lidx, lval);
    return grl_check_launch("grl_rrs_weights");
}

extern "C" int grl_rrs_expand_rows(const int32_t* rank, int64_t ld, const int32_t* lcnt, const int32_t* lidx,
                                   const float* lval, int N, int k2, int row0, int nrows, const int64_t* row_ptr,
                                   int32_t* cnt, int32_t* col, float* val, void* stream) {
    GRL_REQUIRE(rank && lcnt && lidx && lval && N > 0, "rrs_expand: bad args");
    GRL_REQUIRE(k2 >= 1 && k2 <= RR_K2MAX && k2 <= N && ld >= k2, "rrs_expand: 1 <= k2 <= 8, k2 <= N, ld >= k2");
    GRL_REQUIRE(row_ptr ? (col && val) : (cnt != nullptr), "rrs_expand: count needs cnt, fill needs col and val");
    GRL_REQUIRE(row0 >= 0 && nrows >= 0 && (int64_t)row0 + nrows <= N, "rrs_expand: rows outside 0..N");
    if (nrows == 0) return GRL_OK;
    hipLaunchKernelGGL(rrs_expand_kernel, dim3(nrows), dim3(256), 0, (hipStream_t)stream, rank, ld, lcnt, lidx, lval,
                       k2, row0, row_ptr, cnt, col, val);
    return grl_check_launch("grl_rrs_expand");
}

extern "C" int grl_rrs_expand(const int32_t* rank, int64_t ld, const int32_t* lcnt, const int32_t* lidx,
                              const float* lval, int N, int k2, const int64_t* row_ptr, int32_t* cnt, int32_t* col,
                              float* val, void* stream) {
    return grl_rrs_expand_rows(rank, ld, lcnt, lidx, lval, N, k2, 0, N, row_ptr, cnt, col, val, stream);
}

extern "C" int grl_rrs_scan(const int32_t* cnt, int n, int64_t* ptr, void* stream) {
    GRL_REQUIRE(ptr && n >= 0 && (cnt || n == 0), "rrs_scan: bad args");
    hipLaunchKernelGGL(rrs_scan_kernel, dim3(1), dim3(RRS_SCAN_T), 0, (hipStream_t)stream, cnt, n, ptr);
    return grl_check_launch("grl_rrs_scan");
}

extern "C" int grl_rrs_place(const int32_t* src_col, const float* src_val, int64_t cap, const int64_t* row_ptr, int row0,
                             int row1, int32_t* col, float* val, void* stream) {
    GRL_REQUIRE(row_ptr && col && val && cap >= 0 && row0 >= 0 && row1 >= row0, "rrs_place: bad args");
    if (cap == 0 || row1 == row0) return GRL_OK;
    GRL_REQUIRE(src_col && src_val, "rrs_place: null source");
    const int blocks = (int)std::min<int64_t>((cap + 255) / 256, 65535);
    hipLaunchKernelGGL(rrs_place_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src_col, src_val, cap,
                       row_ptr, row0, row1, col, val);
    return grl_check_launch("grl_rrs_place");
}

extern "C" int grl_rrs_transpose(const int64_t* row_ptr, const int32_t* col, const float* val, int nq, int N,
                                 int32_t* ccnt, int32_t* tmp_row, float* tmp_val, int64_t* csc_ptr, int32_t* csc_row,
                                 float* csc_val, void* stream) {
    GRL_REQUIRE(row_ptr && col && val && ccnt && tmp_row && tmp_val && csc_ptr && csc_row && csc_val,
                "rrs_transpose: null");
    GRL_REQUIRE(nq >= 0 && N > nq, "rrs_transpose: needs 0 <= nq < N");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ccnt, 0, sizeof(int32_t) * (size_t)N, st) != hipSuccess)
        return grl_fail(GRL_ELAUNCH, "rrs_transpose: hipMemsetAsync failed");
    const int blocks = grl_ceil_div(N - nq, 4);
    hipLaunchKernelGGL(rrs_csc_count_kernel, dim3(blocks), dim3(256), 0, st, row_ptr, col, nq, N, ccnt);
    hipLaunchKernelGGL(rrs_scan_kernel, dim3(1), dim3(RRS_SCAN_T), 0, st, ccnt, N, csc_ptr);
    hipLaunchKernelGGL(rrs_csc_scatter_kernel, dim3(blocks), dim3(256), 0, st, row_ptr, col, val, nq, N, csc_ptr, ccnt,
                       tmp_row, tmp_val);
    hipLaunchKernelGGL(rrs_csc_order_kernel, dim3(N), dim3(256), 0, st, csc_ptr, tmp_row, tmp_val, csc_row, csc_val);
    return grl_check_launch("grl_rrs_transpose");
}

extern "C" int grl_rrs_final(float* d, int64_t ld, int nq, int col0, int ncols, const float* colmax,
                             const int64_t* q_ptr, const int32_t* q_col, const float* q_val, const int64_t* csc_ptr,
                             const int32_t* csc_row, const float* csc_val, float lambda_value, float one_minus_lambda,
                             void* stream) {
    GRL_REQUIRE(d && colmax && q_ptr && q_col && q_val && csc_ptr && csc_row && csc_val, "rrs_final: null");
    GRL_REQUIRE(nq > 0 && ncols > 0 && col0 >= 0 && ld >= ncols, "rrs_final: bad shape");
    hipLaunchKernelGGL(rrs_final_kernel, dim3(nq, grl_ceil_div(ncols, RRS_CHUNK)), dim3(64), 0, (hipStream_t)stream, d,
                       ld, nq, col0, ncols, colmax, q_ptr, q_col, q_val, csc_ptr, csc_row, csc_val, lambda_value,
                       one_minus_lambda);
    return grl_check_launch("grl_rrs_final");
}
