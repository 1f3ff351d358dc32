// Pair-level (verification) histograms of a column block of the query x gallery distance matrix
// (engine.pair_roc / rerank_pair_roc / pair_roc_matrix).  Every entry is classified by the id arrays
// (same pid AND camera: dropped; same pid, another camera: positive; another pid: negative), mapped to the
// order-preserving uint32 key of its float32 (sort_order.h roc_key) and counted in bin = key >> (32 - bits) of its
// class's histogram.
// The counts are integers: they do not depend on the order of the adds, the block width or the sharding.
//
// Contention.  More than 99 % of the entries are negatives that fall into a few hundred neighbouring bins, so a
// global atomic per entry would serialise on a handful of addresses.  A workgroup instead counts in LDS: a table of
// ROC_SLOTS (tag, 32-bit count) pairs, slot = (bin + class * ROC_SLOTS / 2) mod ROC_SLOTS, claimed by the first
// (class, bin) that asks for it (compare-and-swap on the tag).  A run of neighbouring bins maps to neighbouring slots,
// so a cluster of up to ROC_SLOTS bins -- wherever it lies, and however many clusters there are (a cosine distance
// around zero has one on each side of the sign) -- is counted without leaving the CU; an entry whose slot belongs to
// another bin goes to the global histogram with one 64-bit atomic.  At the end the workgroup adds every non-zero
// slot to the global histogram with one 64-bit atomic.  No pre-pass over the block is needed to place a window.
//
// Bound: a slot's 32-bit count cannot overflow while a workgroup handles fewer than 2^32 entries.  A workgroup takes
// ROC_COLS columns of every gridDim.y-th row: at most ROC_COLS * ceil(nq / gridDim.y) entries, checked by the launcher.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grl_hip.h"
#include "common.h"
#include "sort_order.h"

namespace {

constexpr int ROC_THREADS = 256;
constexpr int ROC_COLS = 4 * ROC_THREADS;      // columns per workgroup: 16 bytes per lane and row
constexpr int ROC_SLOTS = 4096;                // LDS table: 4096 x (tag, count) = 32 KiB
constexpr int ROC_TARGET_GROUPS = 1024;        // ~4 workgroups per CU: the flush is paid once per workgroup
constexpr unsigned ROC_EMPTY = 0xffffffffu;    // above every tag (a tag has at most 21 bits)

__device__ __forceinline__ void roc_count(float v, int cls, int shift, unsigned* tags, unsigned* cnt,
                                          unsigned long long* pos_hist, unsigned long long* neg_hist) {
    const unsigned bin = roc_key(v) >> shift;
    const unsigned tag = ((unsigned)cls << 20) | bin;
    const unsigned slot = (bin + (unsigned)cls * (ROC_SLOTS / 2)) & (ROC_SLOTS - 1);
    // a tag is written once (EMPTY -> tag) and never changes before the flush: a stale EMPTY only costs the swap
    unsigned t = __hip_atomic_load(&tags[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (t == ROC_EMPTY) {
        t = atomicCAS(&tags[slot], ROC_EMPTY, tag);
        if (t == ROC_EMPTY) t = tag;
    }
    if (t == tag) atomicAdd(&cnt[slot], 1u);
    else atomicAdd((cls ? pos_hist : neg_hist) + bin, 1ull);
}

// grid (column chunk of ROC_COLS, row group).  A lane owns four neighbouring columns: their gallery ids stay in
// registers for all rows, a row costs one 16-byte load (VEC: d and ld allow it) and the query's two ids, which are
// wave-uniform.  Ragged last chunk and unaligned blocks: element by element.
template <bool VEC>
__global__ __launch_bounds__(ROC_THREADS) void pair_hist_kernel(const float* __restrict__ d, int64_t ld, int nq,
                                                                int col0, int ncols,
                                                                const int32_t* __restrict__ q_pids,
                                                                const int32_t* __restrict__ q_cams,
                                                                const int32_t* __restrict__ g_pids,
                                                                const int32_t* __restrict__ g_cams, int shift,
                                                                unsigned long long* __restrict__ pos_hist,
                                                                unsigned long long* __restrict__ neg_hist) {
    __shared__ unsigned tags[ROC_SLOTS];
    __shared__ unsigned cnt[ROC_SLOTS];
    const int tid = threadIdx.x;
    for (int s = tid; s < ROC_SLOTS; s += ROC_THREADS) { tags[s] = ROC_EMPTY; cnt[s] = 0u; }
    const int j0 = blockIdx.x * ROC_COLS + 4 * tid;
    const int nv = min(4, max(0, ncols - j0));                   // this lane's columns inside the block
    int gp[4], gc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        gp[e] = e < nv ? g_pids[(int64_t)col0 + j0 + e] : 0;
        gc[e] = e < nv ? g_cams[(int64_t)col0 + j0 + e] : 0;
    }
    __syncthreads();
    for (int q = blockIdx.y; q < nq; q += gridDim.y) {
        const int qp = q_pids[q], qc = q_cams[q];
        const float* dr = d + (int64_t)q * ld + j0;
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (VEC && nv == 4) {
            const float4 v = *reinterpret_cast<const float4*>(dr);
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < nv) x[e] = dr[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e >= nv) continue;
            const bool same = gp[e] == qp;
            if (same && gc[e] == qc) continue;                   // junk: same pid AND camera
            roc_count(x[e], same ? 1 : 0, shift, tags, cnt, pos_hist, neg_hist);
        }
    }
    __syncthreads();
    for (int s = tid; s < ROC_SLOTS; s += ROC_THREADS) {
        const unsigned c = cnt[s];
        if (c) {
            const unsigned tag = tags[s];
            atomicAdd(((tag >> 20) ? pos_hist : neg_hist) + (tag & 0xfffffu), (unsigned long long)c);
        }
    }
}

}  // namespace

extern "C" int grl_pair_hist_block(const float* d, int64_t ld, int nq, int col0, int ncols, const int32_t* q_pids,
                                   const int32_t* q_cams, const int32_t* g_pids, const int32_t* g_cams, int bits,
                                   int64_t* pos_hist, int64_t* neg_hist, void* stream) {
    GRL_REQUIRE(d && q_pids && q_cams && g_pids && g_cams && pos_hist && neg_hist, "pair_hist_block: null");
    GRL_REQUIRE(nq >= 0 && ncols >= 1 && ld >= ncols && col0 >= 0, "pair_hist_block: bad shape");
    if (bits < 8 || bits > 20) return grl_fail(GRL_EINVAL, "pair_hist_block: bits = %d (8..20)", bits);
    if (nq == 0) return GRL_OK;
    const int chunks = grl_ceil_div(ncols, ROC_COLS);
    const int groups = min(nq, max(1, ROC_TARGET_GROUPS / chunks));
    // the LDS counts are 32-bit: a workgroup must handle fewer than 2^32 entries
    if ((int64_t)ROC_COLS * grl_ceil_div(nq, groups) >= ((int64_t)1 << 32))
        return grl_fail(GRL_EUNSUPPORTED, "pair_hist_block: %d query rows over %d row groups: a workgroup's 32-bit "
                        "counts could overflow (split the rows)", nq, groups);
    const bool vec = (reinterpret_cast<uintptr_t>(d) & 15) == 0 && (ld & 3) == 0;
    auto* pos = reinterpret_cast<unsigned long long*>(pos_hist);
    auto* neg = reinterpret_cast<unsigned long long*>(neg_hist);
    const dim3 grid(chunks, groups);
    if (vec)
        hipLaunchKernelGGL(pair_hist_kernel<true>, grid, dim3(ROC_THREADS), 0, (hipStream_t)stream, d, ld, nq, col0,
                           ncols, q_pids, q_cams, g_pids, g_cams, 32 - bits, pos, neg);
    else
        hipLaunchKernelGGL(pair_hist_kernel<false>, grid, dim3(ROC_THREADS), 0, (hipStream_t)stream, d, ld, nq, col0,
                           ncols, q_pids, q_cams, g_pids, g_cams, 32 - bits, pos, neg);
    return grl_check_launch("grl_pair_hist_block");
}
