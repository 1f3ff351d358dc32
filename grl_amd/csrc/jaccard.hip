// The eps-graph of the k-reciprocal Jaccard distance of one sample set (engine.jaccard_graph / cluster_jaccard,
// DESIGN.md 4v), straight from the sparse V2 of rerank_stream.hip: no n x n pass.
//
//   t[i][j] = sum over the k with V2[i][k] != 0, ascending, of min(V2[i][k], V2[j][k])      (rrs_final_kernel's order)
//   J[i][j] = 1 - t / (2 - t);   edge i -> j iff j != i and J <= eps (eps < 1; a NaN never passes)
//
// For eps < 1 only the j with t > 0 can be edges: the samples that share a non-zero column with i.  They are exactly
// the entries of the CSC lists of row i's columns, so a row is the min-sum product of its <= 2048 non-zeros with those
// lists: about 10^4 terms where the row has n columns.
//
// One workgroup per row.  The fp32 sums of a WINDOW of columns live in LDS; the windows of a row are walked in ascending
// order, so a running count places a row's edges in ascending column order with plain stores (count / scan / fill, as
// cluster.hip).  Every non-zero k of the row keeps a cursor into its CSC list (ascending samples), advanced as the
// windows pass: no window needs a search, and a window in which no cursor has an entry is skipped (the next window is
// the one of the smallest sample under any cursor).  Inside a window the k are applied in ascending order, one barrier
// between two k; within one k a sample occurs once, so the lanes add to distinct slots.  The sum of a slot is therefore
// the contract's, whatever the window width: no float atomics, the same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include "../../include/grl_hip.h"
#include "common.h"
#include "rerank_common.h"

namespace {

constexpr int JC_THREADS = 256;
constexpr int JC_WAVES = JC_THREADS / 64;
constexpr int JC_NZMAX = RR_K2MAX * RR_LMAX;    // longest V2 row grl_rrs_expand makes (2048)
constexpr int JC_WINDOW_MAX = 8192;             // 32 KB of sums + 40 KB of row state: two workgroups in a CU's 160 KB
constexpr int JC_WINDOW_DEFAULT = JC_WINDOW_MAX;

template <bool FILL>
__global__ __launch_bounds__(JC_THREADS) void jaccard_edges_kernel(const int64_t* __restrict__ q_ptr,
                                                                   const int32_t* __restrict__ q_col,
                                                                   const float* __restrict__ q_val,
                                                                   const int64_t* __restrict__ csc_ptr,
                                                                   const int32_t* __restrict__ csc_row,
                                                                   const float* __restrict__ csc_val, int n, float eps,
                                                                   int window, int32_t* __restrict__ cnt,
                                                                   const int64_t* __restrict__ out_ptr,
                                                                   int32_t* __restrict__ out_col,
                                                                   float* __restrict__ out_val) {
    __shared__ float acc[JC_WINDOW_MAX];
    __shared__ long long pos[JC_NZMAX], end[JC_NZMAX];  // cursor and end of every non-zero's CSC list
    __shared__ float kval[JC_NZMAX];
    __shared__ int wtot[2][JC_WAVES];
    __shared__ int wmin[JC_WAVES];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t qs = q_ptr[i];
    const int nz = (int)min((int64_t)JC_NZMAX, max((int64_t)0, q_ptr[i + 1] - qs));
    for (int a = tid; a < nz; a += JC_THREADS) {
        const int k = q_col[qs + a];
        const bool ok = (unsigned)k < (unsigned)n;          // a column outside 0..n-1 has no list
        pos[a] = ok ? csc_ptr[k] : 0;
        end[a] = ok ? csc_ptr[k + 1] : 0;
        kval[a] = q_val[qs + a];
    }
    int64_t out0 = 0, out_end = 0;
    if (FILL) {
        out0 = out_ptr[i];
        out_end = out_ptr[i + 1];                           // never write past the row the count pass sized
    }
    int base = 0;                                           // the row's edges in the windows before this one
    int par = 0;
    __syncthreads();
    for (;;) {
        // the next window: the one of the smallest sample under any cursor
        int m = INT_MAX;
        for (int a = tid; a < nz; a += JC_THREADS)
            if (pos[a] < end[a]) m = min(m, csc_row[pos[a]]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
        if (lane == 0) wmin[wave] = m;
        __syncthreads();
        m = min(min(wmin[0], wmin[1]), min(wmin[2], wmin[3]));
        if ((unsigned)m >= (unsigned)n) break;              // every list is used up (or holds a sample outside 0..n-1)
        const int w0 = m / window * window;
        const int64_t whi = min((int64_t)w0 + window, (int64_t)n);
        const int wn = (int)(whi - w0);
        for (int c = tid; c < wn; c += JC_THREADS) acc[c] = 0.f;
        __syncthreads();                                    // (also: everyone has read wmin)
        for (int a = 0; a < nz; ++a) {
            const int64_t p = pos[a], e = end[a];
            if (p >= e) continue;                           // (the same for every thread)
            const float v = kval[a];
            int64_t moved = -1;
            for (int64_t x = p + tid; x < e; x += JC_THREADS) {
                const int r = csc_row[x];
                if (r >= whi) break;
                if (r >= w0) acc[r - w0] = acc[r - w0] + fminf(v, csc_val[x]);
                if (x + 1 >= e || csc_row[x + 1] >= whi) moved = x + 1;      // the list's last entry below whi
            }
            __syncthreads();                                // the next k adds after this one; everyone has read pos[a]
            if (moved >= 0) pos[a] = moved;
        }
        // threshold and ordered compaction, 256 columns per round (eps_edges_kernel's pattern)
        for (int c0 = 0; c0 < wn; c0 += JC_THREADS, par ^= 1) {
            const int c = c0 + tid, j = w0 + c;
            float jac = 0.f;
            bool hit = false;
            if (c < wn) {
                const float t = acc[c];
                jac = 1.f - t / (2.f - t);
                hit = j != i && jac <= eps;                 // NaN <= eps is false
            }
            const unsigned long long b = __ballot(hit);
            if (lane == 0) wtot[par][wave] = __popcll(b);
            __syncthreads();
            int woff = 0, tot = 0;
#pragma unroll
            for (int w = 0; w < JC_WAVES; ++w) {
                const int t = wtot[par][w];
                if (w < wave) woff += t;
                tot += t;
            }
            if (FILL && hit) {
                const int64_t o = out0 + base + woff + __popcll(b & below);
                if (o < out_end) {
                    out_col[o] = j;
                    if (out_val) out_val[o] = jac;
                }
            }
            base += tot;
        }
        __syncthreads();                                    // acc, pos and wmin are rewritten for the next window
    }
    if (!FILL && tid == 0) cnt[i] = base;
}

}  // namespace

extern "C" int grl_jaccard_edges(const int64_t* row_ptr_v2, const int32_t* col_v2, const float* val_v2,
                                 const int64_t* csc_ptr, const int32_t* csc_row, const float* csc_val, int n, float eps,
                                 int window, int32_t* cnt, const int64_t* out_row_ptr, int32_t* out_col, float* out_val,
                                 void* stream) {
    GRL_REQUIRE(row_ptr_v2 && col_v2 && val_v2 && csc_ptr && csc_row && csc_val, "jaccard_edges: null");
    GRL_REQUIRE(out_row_ptr ? out_col != nullptr : (cnt != nullptr && !out_col && !out_val),
                "jaccard_edges: the count pass needs cnt alone, the fill pass out_row_ptr and out_col");
    GRL_REQUIRE(n >= 2, "jaccard_edges: n >= 2");
    GRL_REQUIRE(window >= 0 && window % 256 == 0 && window <= JC_WINDOW_MAX,
                "jaccard_edges: window must be 0 or a multiple of 256 up to 8192");
    GRL_REQUIRE(isfinite(eps) && eps < 1.f, "jaccard_edges: eps must be finite and < 1");
    if (window == 0) window = JC_WINDOW_DEFAULT;
    hipStream_t st = (hipStream_t)stream;
    if (out_row_ptr)
        hipLaunchKernelGGL((jaccard_edges_kernel<true>), dim3(n), dim3(JC_THREADS), 0, st, row_ptr_v2, col_v2, val_v2,
                           csc_ptr, csc_row, csc_val, n, eps, window, cnt, out_row_ptr, out_col, out_val);
    else
        hipLaunchKernelGGL((jaccard_edges_kernel<false>), dim3(n), dim3(JC_THREADS), 0, st, row_ptr_v2, col_v2, val_v2,
                           csc_ptr, csc_row, csc_val, n, eps, window, cnt, out_row_ptr, out_col, out_val);
    return grl_check_launch("grl_jaccard_edges");
}
