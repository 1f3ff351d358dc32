// Gallery search and exact ranking metrics over column blocks of the query x gallery distance matrix
// (engine.search / engine.rank_metrics_streaming).  The distances of a block come from the
// NEGDOT / EUCLID GEMM (gemm_f32.hip), which computes every entry by the same fma chain whatever N is, so
// a block holds exactly the same bits as the same columns of the full matrix.  Everything here is
// selection, gathering and integer counting; nothing needs the whole matrix.
//
// Total order: the one of grl_row_argsort (sort_order.h order_key): canonical NaN, -0 -> +0, ascending
// key, ties to the smaller gallery index = np.argsort(kind='stable').  An entry is the 64-bit composite
// (key << 32) | gallery index, unique per row, so "before" is a plain integer compare.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grl_hip.h"
#include "common.h"
#include "sort_order.h"

namespace {

constexpr int SEARCH_THREADS = 256;
constexpr int TOPK_MAX = 1024;
constexpr int MATCH_LIST_MAX = 8192;      // candidates (gallery entries of one pid) per query: one LDS sort
constexpr int COUNT_CHUNK = 4096;         // gallery columns per workgroup of the rank-count pass
constexpr uint64_t PAD = ~0ull;           // above every real composite (the largest key is 0xffc00000, NaN)

// One workgroup per query row.  LDS holds the row's running list in [0, P) (sorted, the first k entries
// valid, the rest padding) and a candidate buffer in [P, 2P).  A column enters the buffer only if it comes
// before the current k-th entry; when the buffer cannot take another 256-column chunk, the 2P entries are
// sorted and the best P stay in front.  The result is the first k entries of the union under the total
// order, whatever order the buffer was filled in.
//
// FILTER (grl_topk_block_filtered): a column whose gallery entry shares pid AND camera with the query is junk
// (eva_functions.py:151-155) and never enters the buffer.  The predicate sits behind the threshold test, so only
// the columns that would have been admitted read g_pids / g_cams: every column while the list is still filling
// (thr is padding, junk must not take a slot and set the threshold), a few per chunk afterwards.  The query's
// own pid and camera are wave-uniform: one load before the loop, held in scalar registers for the whole row.
// Without FILTER the branch does not exist and the four pointers are never read.
template <bool FILTER>
__global__ __launch_bounds__(SEARCH_THREADS) void topk_block_kernel(const float* __restrict__ d, int64_t ld,
                                                                    const int32_t* __restrict__ cidx, int64_t ldc,
                                                                    int ncols, int col0, int k, int P,
                                                                    uint64_t* __restrict__ run_key,
                                                                    float* __restrict__ run_val,
                                                                    const int32_t* __restrict__ q_pids,
                                                                    const int32_t* __restrict__ q_cams,
                                                                    const int32_t* __restrict__ g_pids,
                                                                    const int32_t* __restrict__ g_cams) {
    extern __shared__ __attribute__((aligned(16))) uint64_t sm_topk[];
    uint64_t* c = sm_topk;                                  // [2P]
    float* v = reinterpret_cast<float*>(sm_topk + 2 * P);   // [2P]
    __shared__ int cnt;
    const int q = blockIdx.x, tid = threadIdx.x;
    const float* dr = d + (int64_t)q * ld;
    uint64_t* rk = run_key + (int64_t)q * k;
    float* rv = run_val + (int64_t)q * k;
    for (int i = tid; i < 2 * P; i += SEARCH_THREADS) {
        c[i] = i < k ? rk[i] : PAD;
        v[i] = i < k ? rv[i] : __int_as_float(0x7f800000);
    }
    if (tid == 0) cnt = 0;
    int qp = 0, qc = 0;
    if constexpr (FILTER) { qp = q_pids[q]; qc = q_cams[q]; }
    __syncthreads();
    for (int base = 0; base < ncols; base += SEARCH_THREADS) {
        const uint64_t thr = c[k - 1];
        const int j = base + tid;
        if (j < ncols) {
            const int g = cidx ? cidx[(int64_t)q * ldc + j] : col0 + j;
            if (g >= 0) {
                const float x = dr[j];
                const uint64_t cc = composite(order_key(x), g);
                bool take = cc < thr;
                if constexpr (FILTER) take = take && !(g_pids[g] == qp && g_cams[g] == qc);
                if (take) {
                    const int pos = atomicAdd(&cnt, 1);         // < P: the buffer had room for a whole chunk
                    c[P + pos] = cc;
                    v[P + pos] = x;
                }
            }
        }
        __syncthreads();
        const int n = cnt;
        __syncthreads();                                         // every lane has read cnt before the next chunk adds to it
        if (n > 0 && (n > P - SEARCH_THREADS || base + SEARCH_THREADS >= ncols)) {
            bitonic_lds(c, v, 2 * P);
            for (int i = P + tid; i < 2 * P; i += SEARCH_THREADS) { c[i] = PAD; v[i] = __int_as_float(0x7f800000); }
            if (tid == 0) cnt = 0;
            __syncthreads();
        }
    }
    for (int i = tid; i < k; i += SEARCH_THREADS) { rk[i] = c[i]; rv[i] = v[i]; }
}

// One workgroup per query: the keys of the query's candidates (gallery entries with its pid, junk
// included) that fall in [col0, col0 + ncols).  Candidate j of query q (j-th entry of its pid's ascending
// gallery list) lands in cand_key[cand_off[q] + j]; every candidate is written by exactly one block.
__global__ __launch_bounds__(SEARCH_THREADS) void match_gather_kernel(const float* __restrict__ d, int64_t ld,
                                                                      int col0, int ncols,
                                                                      const int32_t* __restrict__ q_slot,
                                                                      const int32_t* __restrict__ pid_ptr,
                                                                      const int32_t* __restrict__ pid_list,
                                                                      const int64_t* __restrict__ cand_off,
                                                                      uint32_t* __restrict__ cand_key) {
    const int q = blockIdx.x;
    const int s = q_slot[q];
    if (s < 0) return;
    const int lo = pid_ptr[s], hi = pid_ptr[s + 1];
    const int a = lower_bound(pid_list, lo, hi, col0);
    const int b = lower_bound(pid_list, a, hi, col0 + ncols);
    const float* dr = d + (int64_t)q * ld;
    uint32_t* out = cand_key + cand_off[q] - lo;
    for (int j = a + threadIdx.x; j < b; j += SEARCH_THREADS) out[j] = order_key(dr[pid_list[j] - col0]);
}

// One workgroup per query: keep the candidates from another camera (the query's matches; same pid AND
// camera is junk) and sort them by (key, gallery index).  match_key[cand_off[q] + i], i < n_match[q].
__global__ __launch_bounds__(SEARCH_THREADS) void match_sort_kernel(const int32_t* __restrict__ q_slot,
                                                                    const int32_t* __restrict__ pid_ptr,
                                                                    const int32_t* __restrict__ pid_list,
                                                                    const int32_t* __restrict__ q_cams,
                                                                    const int32_t* __restrict__ g_cams,
                                                                    const int64_t* __restrict__ cand_off,
                                                                    const uint32_t* __restrict__ cand_key, int P,
                                                                    uint64_t* __restrict__ match_key,
                                                                    int32_t* __restrict__ n_match) {
    extern __shared__ __attribute__((aligned(16))) uint64_t sm_match[];
    __shared__ int kept;
    const int q = blockIdx.x, tid = threadIdx.x;
    const int s = q_slot[q];
    if (s < 0) {
        if (tid == 0) n_match[q] = 0;
        return;
    }
    const int lo = pid_ptr[s], L = pid_ptr[s + 1] - lo;
    const int qc = q_cams[q];
    const uint32_t* ck = cand_key + cand_off[q];
    if (tid == 0) kept = 0;
    __syncthreads();
    int mine = 0;
    for (int j = tid; j < P; j += SEARCH_THREADS) {
        uint64_t e = PAD;
        if (j < L) {
            const int g = pid_list[lo + j];
            if (g_cams[g] != qc) { e = composite(ck[j], g); ++mine; }
        }
        sm_match[j] = e;
    }
    if (mine) atomicAdd(&kept, mine);
    __syncthreads();
    bitonic_lds(sm_match, nullptr, P);
    const int n = kept;
    uint64_t* out = match_key + cand_off[q];
    for (int i = tid; i < n; i += SEARCH_THREADS) out[i] = sm_match[i];
    if (tid == 0) n_match[q] = n;
}

// grid (query, COUNT_CHUNK columns of the block).  For every kept non-match g (another pid) of the chunk,
// p(g) = number of the query's matches strictly before g; h[p] is built in LDS and added to the query's
// global histogram with integer atomics (order-independent).  p == n_match (after the last match) is not
// needed by the finish and is not counted.
__global__ __launch_bounds__(SEARCH_THREADS) void rank_count_kernel(const float* __restrict__ d, int64_t ld,
                                                                    int col0, int ncols,
                                                                    const int32_t* __restrict__ q_pids,
                                                                    const int32_t* __restrict__ g_pids,
                                                                    const int64_t* __restrict__ cand_off,
                                                                    const uint64_t* __restrict__ match_key,
                                                                    const int32_t* __restrict__ n_match,
                                                                    int max_match,
                                                                    int32_t* __restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) uint64_t sm_cnt[];
    uint64_t* mk = sm_cnt;                                       // [max_match]
    int* h = reinterpret_cast<int*>(sm_cnt + max_match);         // [max_match]
    const int q = blockIdx.x, tid = threadIdx.x;
    const int n = n_match[q];
    if (n == 0) return;
    const int64_t off = cand_off[q];
    for (int i = tid; i < n; i += SEARCH_THREADS) { mk[i] = match_key[off + i]; h[i] = 0; }
    __syncthreads();
    const uint64_t last = mk[n - 1];
    const int qp = q_pids[q];
    const float* dr = d + (int64_t)q * ld;
    const int j0 = blockIdx.y * COUNT_CHUNK, j1 = min(ncols, j0 + COUNT_CHUNK);
    for (int j = j0 + tid; j < j1; j += SEARCH_THREADS) {
        const int g = col0 + j;
        if (g_pids[g] == qp) continue;                           // a match or junk: not a kept non-match
        const uint64_t cc = composite(order_key(dr[j]), g);
        if (cc > last) continue;                                 // after every match (cc != last: indices differ)
        int lo = 0, len = n;
        while (len > 0) {
            const int half = len >> 1;
            if (mk[lo + half] < cc) { lo += half + 1; len -= half + 1; } else len = half;
        }
        atomicAdd(&h[lo], 1);
    }
    __syncthreads();
    for (int i = tid; i < n; i += SEARCH_THREADS)
        if (h[i]) atomicAdd(&hist[off + i], h[i]);
}

// One thread per query: rank_i = i + sum_{p <= i} h[p] is the i-th match's 0-based rank among the kept
// entries; AP = (1/n) sum_i (i + 1) / (rank_i + 1) in fp64, summed in ascending i.
__global__ __launch_bounds__(SEARCH_THREADS) void rank_finish_kernel(int nq, const int64_t* __restrict__ cand_off,
                                                                     const int32_t* __restrict__ n_match,
                                                                     const int32_t* __restrict__ hist,
                                                                     int32_t* __restrict__ first_hit,
                                                                     int32_t* __restrict__ n_hits,
                                                                     double* __restrict__ ap) {
    const int q = blockIdx.x * SEARCH_THREADS + threadIdx.x;
    if (q >= nq) return;
    const int n = n_match[q];
    const int32_t* h = hist + cand_off[q];
    int cum = 0, first = -1;
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
        cum += h[i];
        const int pos = i + cum;
        if (i == 0) first = pos;
        sum += (double)(i + 1) / (double)(pos + 1);
    }
    n_hits[q] = n;
    first_hit[q] = first;
    ap[q] = n > 0 ? sum / (double)n : 0.0;
}

int pow2_at_least(int x) {
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

}  // namespace

extern "C" int grl_topk_block(const float* d, int64_t ld, const int32_t* cidx, int64_t ldc, int nq, int ncols,
                              int col0, int k, uint64_t* run_key, float* run_val, void* stream) {
    GRL_REQUIRE(d && run_key && run_val, "topk_block: null");
    GRL_REQUIRE(nq > 0 && ncols > 0 && ld >= ncols && col0 >= 0 && (!cidx || ldc >= ncols), "topk_block: bad shape");
    if (k < 1 || k > TOPK_MAX) return grl_fail(GRL_EUNSUPPORTED, "topk_block: k = %d (1..%d)", k, TOPK_MAX);
    const int P = max(SEARCH_THREADS, pow2_at_least(k));
    const size_t lds = (size_t)2 * P * (sizeof(uint64_t) + sizeof(float));
    hipLaunchKernelGGL(topk_block_kernel<false>, dim3(nq), dim3(SEARCH_THREADS), lds, (hipStream_t)stream, d, ld, cidx,
                       ldc, ncols, col0, k, P, run_key, run_val, (const int32_t*)nullptr, (const int32_t*)nullptr,
                       (const int32_t*)nullptr, (const int32_t*)nullptr);
    return grl_check_launch("grl_topk_block");
}

extern "C" int grl_topk_block_filtered(const float* d, int64_t ld, const int32_t* cidx, int64_t ldc, int nq, int ncols,
                                       int col0, int k, uint64_t* run_key, float* run_val, const int32_t* q_pids,
                                       const int32_t* q_cams, const int32_t* g_pids, const int32_t* g_cams,
                                       void* stream) {
    GRL_REQUIRE(d && run_key && run_val && q_pids && q_cams && g_pids && g_cams, "topk_block_filtered: null");
    GRL_REQUIRE(nq > 0 && ncols > 0 && ld >= ncols && col0 >= 0 && (!cidx || ldc >= ncols),
                "topk_block_filtered: bad shape");
    if (k < 1 || k > TOPK_MAX) return grl_fail(GRL_EUNSUPPORTED, "topk_block_filtered: k = %d (1..%d)", k, TOPK_MAX);
    const int P = max(SEARCH_THREADS, pow2_at_least(k));
    const size_t lds = (size_t)2 * P * (sizeof(uint64_t) + sizeof(float));
    hipLaunchKernelGGL(topk_block_kernel<true>, dim3(nq), dim3(SEARCH_THREADS), lds, (hipStream_t)stream, d, ld, cidx,
                       ldc, ncols, col0, k, P, run_key, run_val, q_pids, q_cams, g_pids, g_cams);
    return grl_check_launch("grl_topk_block_filtered");
}

extern "C" int grl_match_gather(const float* d, int64_t ld, int nq, int col0, int ncols, const int32_t* q_slot,
                                const int32_t* pid_ptr, const int32_t* pid_list, const int64_t* cand_off,
                                uint32_t* cand_key, void* stream) {
    GRL_REQUIRE(d && q_slot && pid_ptr && pid_list && cand_off && cand_key, "match_gather: null");
    GRL_REQUIRE(nq > 0 && ncols > 0 && ld >= ncols && col0 >= 0, "match_gather: bad shape");
    hipLaunchKernelGGL(match_gather_kernel, dim3(nq), dim3(SEARCH_THREADS), 0, (hipStream_t)stream, d, ld, col0, ncols,
                       q_slot, pid_ptr, pid_list, cand_off, cand_key);
    return grl_check_launch("grl_match_gather");
}

extern "C" int grl_match_sort(int nq, const int32_t* q_slot, const int32_t* pid_ptr, const int32_t* pid_list,
                              const int32_t* q_cams, const int32_t* g_cams, const int64_t* cand_off,
                              const uint32_t* cand_key, int max_list, uint64_t* match_key, int32_t* n_match,
                              void* stream) {
    GRL_REQUIRE(q_slot && pid_ptr && pid_list && q_cams && g_cams && cand_off && cand_key && match_key && n_match,
                "match_sort: null");
    GRL_REQUIRE(nq > 0 && max_list >= 0, "match_sort: bad shape");
    if (max_list > MATCH_LIST_MAX)
        return grl_fail(GRL_EUNSUPPORTED, "match_sort: %d gallery entries share one query's pid (at most %d)", max_list,
                        MATCH_LIST_MAX);
    const int P = pow2_at_least(max(max_list, 2));
    hipLaunchKernelGGL(match_sort_kernel, dim3(nq), dim3(SEARCH_THREADS), (size_t)P * sizeof(uint64_t),
                       (hipStream_t)stream, q_slot, pid_ptr, pid_list, q_cams, g_cams, cand_off, cand_key, P, match_key,
                       n_match);
    return grl_check_launch("grl_match_sort");
}

extern "C" int grl_rank_count_block(const float* d, int64_t ld, int nq, int col0, int ncols, const int32_t* q_pids,
                                    const int32_t* g_pids, const int64_t* cand_off, const uint64_t* match_key,
                                    const int32_t* n_match, int max_match, int32_t* hist, void* stream) {
    GRL_REQUIRE(d && q_pids && g_pids && cand_off && match_key && n_match && hist, "rank_count_block: null");
    GRL_REQUIRE(nq > 0 && ncols > 0 && ld >= ncols && col0 >= 0 && max_match > 0, "rank_count_block: bad shape");
    if (max_match > MATCH_LIST_MAX)
        return grl_fail(GRL_EUNSUPPORTED, "rank_count_block: %d matches per query (at most %d)", max_match,
                        MATCH_LIST_MAX);
    const size_t lds = (size_t)max_match * (sizeof(uint64_t) + sizeof(int));
    hipLaunchKernelGGL(rank_count_kernel, dim3(nq, (ncols + COUNT_CHUNK - 1) / COUNT_CHUNK), dim3(SEARCH_THREADS), lds,
                       (hipStream_t)stream, d, ld, col0, ncols, q_pids, g_pids, cand_off, match_key, n_match, max_match,
                       hist);
    return grl_check_launch("grl_rank_count_block");
}

extern "C" int grl_rank_finish(int nq, const int64_t* cand_off, const int32_t* n_match, const int32_t* hist,
                               int32_t* first_hit, int32_t* n_hits, double* ap, void* stream) {
    GRL_REQUIRE(cand_off && n_match && hist && first_hit && n_hits && ap, "rank_finish: null");
    GRL_REQUIRE(nq > 0, "rank_finish: bad shape");
    hipLaunchKernelGGL(rank_finish_kernel, dim3((nq + SEARCH_THREADS - 1) / SEARCH_THREADS), dim3(SEARCH_THREADS), 0,
                       (hipStream_t)stream, nq, cand_off, n_match, hist, first_hit, n_hits, ap);
    return grl_check_launch("grl_rank_finish");
}
