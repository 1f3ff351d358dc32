// DBSCAN over column blocks of a distance matrix (engine.eps_graph / cluster / cluster_matrix / cluster_from_graph,
// DESIGN.md 4s): the eps-graph as a CSR without the n x n matrix, then core flags, connected components of the core
// points, border points and labels.  Everything is integer work: no float atomics, every output is deterministic bit
// for bit (the graph) or by construction (labels: a component's root is its smallest core index, whatever the order
// in which the hooks land).
//
// eps-graph.  Edge i -> j (j != i) iff D[i][j] <= eps; a NaN never passes.  Two passes over the block source, the
// count / scan / fill pattern of rerank_stream.hip: pass 1 adds every block's per-row edge count to deg, grl_rrs_scan
// turns deg into row_ptr, pass 2 recomputes the blocks and appends the column indices.  One workgroup owns a row per
// launch and the blocks of a pass are stream-ordered, so the per-row counter is a plain add; it is also the fill
// pass's cursor (zeroed between the passes), which makes the columns of a row ascend across blocks.  Inside a block a
// chunk of columns is ordered by one ballot per lane column (a lane's prefix = popcount of the ballots below its lane)
// and the four waves' totals meet in LDS.
//
// Components.  parent[i] = i at first; a round hooks, for every stored edge between two core points, the larger of
// the two roots under the smaller (integer atomicMin) and then points every core node at its root (pointer jumping).
// A hook can overwrite another hook of the same round; the edge that lost still has two roots in the next round and
// hooks again, so "no edge saw two roots" is the fixed point: every component is one tree, and because parent[x] <= x
// always, its root is its smallest member.  The host repeats rounds until the device flag stays 0.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include "../../include/grl_hip.h"
#include "common.h"

namespace {

constexpr int CL_THREADS = 256;
constexpr int CL_WAVES = CL_THREADS / 64;
constexpr int CL_MAX_GROUPS = 4096;            // grid-stride beyond: ~2 waves of workgroups on 256 CUs

// One workgroup per row (grid-stride), V columns per lane and chunk: V = 4 reads a row in 16-byte loads (d and ld
// allow it), V = 1 is the element path (neighbouring lanes read neighbouring floats).  FILL = false: cnt[row] += the
// block's edges of the row.  FILL = true: the same, and the column indices go to col[row_ptr[row] + cnt[row] ..].
template <int V, bool FILL>
__global__ __launch_bounds__(CL_THREADS) void eps_edges_kernel(const float* __restrict__ d, int64_t ld, int nrows,
                                                               int row0, int col0, int ncols, float eps,
                                                               int32_t* __restrict__ cnt,
                                                               const int64_t* __restrict__ row_ptr,
                                                               int32_t* __restrict__ col) {
    __shared__ int wtot[2][CL_WAVES];
    constexpr int CHUNK = V * CL_THREADS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    int par = 0;                                                 // which half of wtot this chunk uses: one barrier a chunk
    for (int r = blockIdx.x; r < nrows; r += gridDim.x) {
        const int gi = row0 + r;
        const float* dr = d + (int64_t)r * ld;
        int64_t out0 = 0, end = 0;
        if (FILL) {
            out0 = row_ptr[gi] + cnt[gi];                        // (read by all before the first barrier, written after)
            end = row_ptr[gi + 1];                               // never write past the row the count pass sized
        }
        int base = 0;                                            // the row's edges in the chunks before this one
        for (int c = 0; c < ncols; c += CHUNK, par ^= 1) {
            const int j0 = c + V * tid;
            float x[V];
            bool loaded = false;
            if constexpr (V == 4) {
                if (j0 + 3 < ncols) {
                    const float4 v = *reinterpret_cast<const float4*>(dr + j0);
                    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
                    loaded = true;
                }
            }
            if (!loaded) {                                       // element path, and the ragged end of a vector row
#pragma unroll
                for (int e = 0; e < V; ++e) x[e] = j0 + e < ncols ? dr[j0 + e] : 0.f;
            }
            bool hit[V];
            int before = 0, mine = 0;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                hit[e] = j0 + e < ncols && col0 + j0 + e != gi && x[e] <= eps;      // NaN <= eps is false
                const unsigned long long b = __ballot(hit[e]);
                before += __popcll(b & below);                   // edges of the lower lanes, all their columns
                mine += __popcll(b);
            }
            if (lane == 0) wtot[par][wave] = mine;
            __syncthreads();
            int woff = 0, tot = 0;
#pragma unroll
            for (int w = 0; w < CL_WAVES; ++w) {
                const int t = wtot[par][w];
                if (w < wave) woff += t;
                tot += t;
            }
            if (FILL) {
                int64_t o = out0 + base + woff + before;
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (hit[e] && o < end) col[o++] = col0 + j0 + e;
            }
            base += tot;
        }
        if (tid == 0) cnt[gi] += base;
    }
}

__global__ __launch_bounds__(CL_THREADS) void cluster_init_kernel(const int32_t* __restrict__ deg, int n,
                                                                  int min_samples, uint8_t* __restrict__ core,
                                                                  int32_t* __restrict__ parent,
                                                                  int32_t* __restrict__ border) {
    for (int i = blockIdx.x * CL_THREADS + threadIdx.x; i < n; i += gridDim.x * CL_THREADS) {
        core[i] = (int64_t)deg[i] + 1 >= (int64_t)min_samples ? 1 : 0;         // a point counts itself
        parent[i] = i;
        border[i] = INT_MAX;
    }
}

// parent[x] < x for every node that is not a root, so the walk ends; a value another lane is just lowering is still an
// ancestor-or-older link of the same component
__device__ __forceinline__ int cl_find(const int32_t* parent, int x) {
    for (;;) {
        const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;
    }
}

// one wave per row, lanes over the row's stored edges
__global__ __launch_bounds__(CL_THREADS) void cluster_hook_kernel(const int64_t* __restrict__ row_ptr,
                                                                  const int32_t* __restrict__ col,
                                                                  const uint8_t* __restrict__ core,
                                                                  int32_t* __restrict__ parent, int n,
                                                                  int32_t* __restrict__ changed) {
    const int lane = threadIdx.x & 63;
    const int nw = gridDim.x * CL_WAVES;
    bool any = false;
    for (int i = blockIdx.x * CL_WAVES + (threadIdx.x >> 6); i < n; i += nw) {
        if (!core[i]) continue;
        int ri = cl_find(parent, i);
        const int64_t k1 = row_ptr[i + 1];
        for (int64_t k = row_ptr[i] + lane; k < k1; k += 64) {
            const int j = col[k];
            if (j == i || !core[j]) continue;
            const int rj = cl_find(parent, j);
            ri = cl_find(parent, ri);
            if (ri != rj) {
                atomicMin(parent + max(ri, rj), min(ri, rj));
                any = true;
            }
        }
    }
    if (any) atomicOr(changed, 1);
}

__global__ __launch_bounds__(CL_THREADS) void cluster_jump_kernel(const uint8_t* __restrict__ core,
                                                                  int32_t* __restrict__ parent, int n) {
    for (int i = blockIdx.x * CL_THREADS + threadIdx.x; i < n; i += gridDim.x * CL_THREADS)
        if (core[i]) {
            const int r = cl_find(parent, i);
            __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
}

// Both directions of every stored edge: core i, non-core j -> border[j] = min(.., root(i)); non-core i, core j -> the
// same for i (the wave's minimum, one atomic).  parent holds roots (after a round that changed nothing).
__global__ __launch_bounds__(CL_THREADS) void cluster_border_kernel(const int64_t* __restrict__ row_ptr,
                                                                    const int32_t* __restrict__ col,
                                                                    const uint8_t* __restrict__ core,
                                                                    const int32_t* __restrict__ parent, int n,
                                                                    int32_t* __restrict__ border) {
    const int lane = threadIdx.x & 63;
    const int nw = gridDim.x * CL_WAVES;
    for (int i = blockIdx.x * CL_WAVES + (threadIdx.x >> 6); i < n; i += nw) {
        const bool ci = core[i] != 0;
        const int ri = parent[i];
        int best = INT_MAX;
        const int64_t k1 = row_ptr[i + 1];
        for (int64_t k = row_ptr[i] + lane; k < k1; k += 64) {
            const int j = col[k];
            if (j == i) continue;
            const bool cj = core[j] != 0;
            if (ci && !cj) atomicMin(border + j, ri);
            else if (!ci && cj) best = min(best, parent[j]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
        if (lane == 0 && best != INT_MAX) atomicMin(border + i, best);
    }
}

__global__ __launch_bounds__(CL_THREADS) void cluster_roots_kernel(const uint8_t* __restrict__ core,
                                                                   const int32_t* __restrict__ parent, int n,
                                                                   int32_t* __restrict__ is_root) {
    for (int i = blockIdx.x * CL_THREADS + threadIdx.x; i < n; i += gridDim.x * CL_THREADS)
        is_root[i] = core[i] && parent[i] == i ? 1 : 0;
}

__global__ __launch_bounds__(CL_THREADS) void cluster_labels_kernel(const uint8_t* __restrict__ core,
                                                                    const int32_t* __restrict__ parent,
                                                                    const int32_t* __restrict__ border,
                                                                    const int64_t* __restrict__ root_id, int n,
                                                                    int64_t* __restrict__ labels) {
    for (int i = blockIdx.x * CL_THREADS + threadIdx.x; i < n; i += gridDim.x * CL_THREADS) {
        const int r = core[i] ? parent[i] : border[i];
        labels[i] = r == INT_MAX ? (int64_t)-1 : root_id[r];
    }
}

inline int node_groups(int n) { return min(max(grl_ceil_div(n, CL_THREADS), 1), CL_MAX_GROUPS); }
inline int row_groups(int n) { return min(max(grl_ceil_div(n, CL_WAVES), 1), CL_MAX_GROUPS); }

}  // namespace

extern "C" int grl_cluster_edges_block(const float* d, int64_t ld, int nrows, int row0, int col0, int ncols, float eps,
                                       int32_t* cnt, const int64_t* row_ptr, int32_t* col, void* stream) {
    GRL_REQUIRE(d && cnt, "cluster_edges_block: null");
    GRL_REQUIRE(row_ptr ? col != nullptr : col == nullptr, "cluster_edges_block: the fill pass needs row_ptr and col");
    GRL_REQUIRE(nrows >= 0 && ncols >= 1 && ld >= ncols && row0 >= 0 && col0 >= 0, "cluster_edges_block: bad shape");
    GRL_REQUIRE((int64_t)row0 + nrows <= INT_MAX && (int64_t)col0 + ncols <= INT_MAX,
                "cluster_edges_block: sample index beyond int32");
    GRL_REQUIRE(eps == eps, "cluster_edges_block: eps is NaN");
    if (nrows == 0) return GRL_OK;
    if (eps > FLT_MAX) eps = FLT_MAX;                 // +inf: everything finite (and -inf) is a neighbour
    const bool vec = (reinterpret_cast<uintptr_t>(d) & 15) == 0 && (ld & 3) == 0;
    const dim3 grid(min(nrows, CL_MAX_GROUPS)), block(CL_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (col) {
        if (vec) hipLaunchKernelGGL((eps_edges_kernel<4, true>), grid, block, 0, st, d, ld, nrows, row0, col0, ncols,
                                    eps, cnt, row_ptr, col);
        else hipLaunchKernelGGL((eps_edges_kernel<1, true>), grid, block, 0, st, d, ld, nrows, row0, col0, ncols, eps,
                                cnt, row_ptr, col);
    } else {
        if (vec) hipLaunchKernelGGL((eps_edges_kernel<4, false>), grid, block, 0, st, d, ld, nrows, row0, col0, ncols,
                                    eps, cnt, row_ptr, col);
        else hipLaunchKernelGGL((eps_edges_kernel<1, false>), grid, block, 0, st, d, ld, nrows, row0, col0, ncols, eps,
                                cnt, row_ptr, col);
    }
    return grl_check_launch("grl_cluster_edges_block");
}

extern "C" int grl_cluster_init(const int32_t* deg, int n, int min_samples, uint8_t* core, int32_t* parent,
                                int32_t* border, void* stream) {
    GRL_REQUIRE(n >= 0 && min_samples >= 1, "cluster_init: n >= 0, min_samples >= 1");
    if (n == 0) return GRL_OK;
    GRL_REQUIRE(deg && core && parent && border, "cluster_init: null");
    hipLaunchKernelGGL(cluster_init_kernel, dim3(node_groups(n)), dim3(CL_THREADS), 0, (hipStream_t)stream, deg, n,
                       min_samples, core, parent, border);
    return grl_check_launch("grl_cluster_init");
}

extern "C" int grl_cluster_round(const int64_t* row_ptr, const int32_t* col, const uint8_t* core, int32_t* parent,
                                 int n, int32_t* changed, void* stream) {
    GRL_REQUIRE(n >= 0 && changed, "cluster_round: n >= 0, changed not null");
    if (n == 0) return GRL_OK;
    GRL_REQUIRE(row_ptr && core && parent, "cluster_round: null");   // (col may be null: a graph without edges)
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cluster_hook_kernel, dim3(row_groups(n)), dim3(CL_THREADS), 0, st, row_ptr, col, core, parent, n,
                       changed);
    hipLaunchKernelGGL(cluster_jump_kernel, dim3(node_groups(n)), dim3(CL_THREADS), 0, st, core, parent, n);
    return grl_check_launch("grl_cluster_round");
}

extern "C" int grl_cluster_border(const int64_t* row_ptr, const int32_t* col, const uint8_t* core,
                                  const int32_t* parent, int n, int32_t* border, void* stream) {
    GRL_REQUIRE(n >= 0, "cluster_border: n >= 0");
    if (n == 0) return GRL_OK;
    GRL_REQUIRE(row_ptr && core && parent && border, "cluster_border: null");
    hipLaunchKernelGGL(cluster_border_kernel, dim3(row_groups(n)), dim3(CL_THREADS), 0, (hipStream_t)stream, row_ptr,
                       col, core, parent, n, border);
    return grl_check_launch("grl_cluster_border");
}

extern "C" int grl_cluster_roots(const uint8_t* core, const int32_t* parent, int n, int32_t* is_root, void* stream) {
    GRL_REQUIRE(n >= 0, "cluster_roots: n >= 0");
    if (n == 0) return GRL_OK;
    GRL_REQUIRE(core && parent && is_root, "cluster_roots: null");
    hipLaunchKernelGGL(cluster_roots_kernel, dim3(node_groups(n)), dim3(CL_THREADS), 0, (hipStream_t)stream, core,
                       parent, n, is_root);
    return grl_check_launch("grl_cluster_roots");
}

extern "C" int grl_cluster_labels(const uint8_t* core, const int32_t* parent, const int32_t* border,
                                  const int64_t* root_id, int n, int64_t* labels, void* stream) {
    GRL_REQUIRE(n >= 0, "cluster_labels: n >= 0");
    if (n == 0) return GRL_OK;
    GRL_REQUIRE(core && parent && border && root_id && labels, "cluster_labels: null");
    hipLaunchKernelGGL(cluster_labels_kernel, dim3(node_groups(n)), dim3(CL_THREADS), 0, (hipStream_t)stream, core,
                       parent, border, root_id, n, labels);
    return grl_check_launch("grl_cluster_labels");
}
