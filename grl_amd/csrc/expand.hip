// Query expansion and database-side augmentation (engine.expand_from_lists / engine.expand_features):
// out[i] = (x[i] + sum_p w_p * bank[j_p]) / (1 + sum_p w_p) over the first m kept entries (j_p, dist_p) of row i's
// neighbour list, w_p = max(-dist_p, 0)^alpha (alpha == 0: 1).  A gather and a weighted sum over feature rows: the
// n x m x d tensor of `bank[idx]` never exists.
//
// The arithmetic is fixed so that a numpy float32 host model (tests/expand_ref.py) gives the same bits: per element
// acc = x; per kept neighbour in list order acc = acc + (w * bank), both roundings kept (no fma: -ffp-contract=off
// and the pragma below); wsum = 1 + w_0 + w_1 + ... in list order; out = acc / wsum, IEEE division; w = s * s * ... * s
// left to right.  The one thing IEEE leaves open, the sign and payload of a NaN, is closed by storing every NaN as
// 0x7fc00000 (search.hip's canonical NaN).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grl_hip.h"
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int EXPAND_THREADS = 256;
constexpr int EXPAND_VEC = 4;                                   // elements per lane: one 16-byte load per feature row
constexpr int EXPAND_SLICE = EXPAND_THREADS * EXPAND_VEC;       // elements of d per workgroup
constexpr int EXPAND_M_MAX = 4096;                              // kept neighbours per row: 32 KiB of LDS
constexpr int EXPAND_BATCH = 4;                                 // feature rows in flight per lane

__device__ __forceinline__ float expand_weight(float dist, int alpha) {
    const float s = dist < 0.f ? -dist : 0.f;                   // NaN: the comparison is false -> 0
    if (alpha == 0) return 1.0f;
    float w = s;
    for (int a = 1; a < alpha; ++a) w = w * s;
    return w;
}

__device__ __forceinline__ float canonical(float v) { return v != v ? __int_as_float(0x7fc00000) : v; }

// One workgroup per (row, 1024-element slice of d); blockIdx.x = row * slices + slice, so the slices of a row run next
// to each other and share its list in L2.  A launch covers the rows from row0 on (the host splits n so that a grid
// stays below 2^32 threads).
//
// Pass 1 (the whole workgroup, 256 list entries at a time): entry t is kept if 0 <= idx < nb and, with skip_self,
// idx != row; its position among the kept entries is a wave ballot prefix plus the earlier waves' counts, and the
// first m kept (index, weight) pairs land in LDS in list order.  An index >= nb can only come from a caller's bug; it
// is skipped like padding rather than read.
// Pass 2: every lane owns 4 consecutive elements.  (index, weight) are LDS broadcasts; the bank rows of 4 neighbours
// are loaded before the first of them is added, which keeps 4 x 16 bytes per lane in flight.  VECTOR: every pointer
// and leading dimension is 16-byte aligned, so a lane whose 4 elements are inside d uses one dwordx4 access per row;
// the ragged end of d (and every lane when VECTOR is false) goes element by element.
template <bool VECTOR>
__global__ __launch_bounds__(EXPAND_THREADS) void expand_rows_kernel(const float* __restrict__ x, int64_t ldx,
                                                                     const float* __restrict__ bank, int64_t ldb,
                                                                     const int64_t* __restrict__ idx,
                                                                     const float* __restrict__ dist, int64_t ldl,
                                                                     int nb, int d, int L, int m, int alpha,
                                                                     int skip_self, int slices, int row0,
                                                                     float* __restrict__ out, int64_t ldo) {
    extern __shared__ __attribute__((aligned(16))) int sm_expand[];
    int* sj = sm_expand;                                        // [m] kept bank rows
    float* sw = reinterpret_cast<float*>(sm_expand + m);        // [m] their weights
    __shared__ int wave_cnt[EXPAND_THREADS / 64];
    const int blk = blockIdx.x / slices, slice = blockIdx.x - blk * slices;
    const int row = row0 + blk;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t* li = idx + (int64_t)row * ldl;
    const float* ldist = dist + (int64_t)row * ldl;

    int kept = 0;                                               // workgroup-uniform
    for (int base = 0; base < L && kept < m; base += EXPAND_THREADS) {
        const int t = base + tid;
        int64_t j = -1;
        float w = 0.f;
        if (t < L) {
            j = li[t];
            if (j >= nb || (skip_self && j == row)) j = -1;
            if (j >= 0) w = expand_weight(ldist[t], alpha);
        }
        const unsigned long long mask = __ballot(j >= 0);
        if (lane == 0) wave_cnt[wave] = __popcll(mask);
        __syncthreads();
        int pos = kept + __popcll(mask & ((1ull << lane) - 1ull));
        int total = 0;
#pragma unroll
        for (int v = 0; v < EXPAND_THREADS / 64; ++v) {
            const int c = wave_cnt[v];
            if (v < wave) pos += c;
            total += c;
        }
        if (j >= 0 && pos < m) { sj[pos] = (int)j; sw[pos] = w; }
        kept += total;
        __syncthreads();                                        // wave_cnt is rewritten by the next chunk
    }
    if (kept > m) kept = m;

    const int e0 = slice * EXPAND_SLICE + tid * EXPAND_VEC;
    if (e0 >= d) return;
    const float* xr = x + (int64_t)row * ldx;
    float* orow = out + (int64_t)row * ldo;
    float wsum = 1.0f;
    if (VECTOR && e0 + EXPAND_VEC <= d) {
        float4 acc = *reinterpret_cast<const float4*>(xr + e0);
        int p = 0;
        for (; p + EXPAND_BATCH <= kept; p += EXPAND_BATCH) {
            float4 b[EXPAND_BATCH];
            float w[EXPAND_BATCH];
#pragma unroll
            for (int u = 0; u < EXPAND_BATCH; ++u) {
                b[u] = *reinterpret_cast<const float4*>(bank + (int64_t)sj[p + u] * ldb + e0);
                w[u] = sw[p + u];
            }
#pragma unroll
            for (int u = 0; u < EXPAND_BATCH; ++u) {
                acc.x = acc.x + (w[u] * b[u].x);
                acc.y = acc.y + (w[u] * b[u].y);
                acc.z = acc.z + (w[u] * b[u].z);
                acc.w = acc.w + (w[u] * b[u].w);
                wsum = wsum + w[u];
            }
        }
        for (; p < kept; ++p) {
            const float4 b = *reinterpret_cast<const float4*>(bank + (int64_t)sj[p] * ldb + e0);
            const float w = sw[p];
            acc.x = acc.x + (w * b.x);
            acc.y = acc.y + (w * b.y);
            acc.z = acc.z + (w * b.z);
            acc.w = acc.w + (w * b.w);
            wsum = wsum + w;
        }
        float4 r;
        r.x = canonical(__fdiv_rn(acc.x, wsum));
        r.y = canonical(__fdiv_rn(acc.y, wsum));
        r.z = canonical(__fdiv_rn(acc.z, wsum));
        r.w = canonical(__fdiv_rn(acc.w, wsum));
        *reinterpret_cast<float4*>(orow + e0) = r;
        return;
    }
    const int ne = min(EXPAND_VEC, d - e0);
    float acc[EXPAND_VEC];
#pragma unroll
    for (int c = 0; c < EXPAND_VEC; ++c) acc[c] = c < ne ? xr[e0 + c] : 0.f;
    for (int p = 0; p < kept; ++p) {
        const float* br = bank + (int64_t)sj[p] * ldb + e0;
        const float w = sw[p];
#pragma unroll
        for (int c = 0; c < EXPAND_VEC; ++c)
            if (c < ne) acc[c] = acc[c] + (w * br[c]);
        wsum = wsum + w;
    }
#pragma unroll
    for (int c = 0; c < EXPAND_VEC; ++c)
        if (c < ne) orow[e0 + c] = canonical(__fdiv_rn(acc[c], wsum));
}

// [p, p + (rows - 1) * ld + d) floats
inline bool overlaps(const float* a, int64_t a_rows, int64_t a_ld, const float* b, int64_t b_rows, int64_t b_ld, int d) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (size_t)((a_rows - 1) * a_ld + d) * sizeof(float);
    const uintptr_t b0 = (uintptr_t)b, b1 = b0 + (size_t)((b_rows - 1) * b_ld + d) * sizeof(float);
    return a0 < b1 && b0 < a1;
}

}  // namespace

extern "C" int grl_expand_rows(const float* x, int64_t ldx, const float* bank, int64_t ldb, const int64_t* idx,
                               const float* dist, int64_t ldl, int n, int nb, int d, int L, int m, int alpha,
                               int skip_self, float* out, int64_t ldo, void* stream) {
    GRL_REQUIRE(x && bank && idx && dist && out, "expand_rows: null");
    GRL_REQUIRE(n > 0 && nb > 0 && d > 0 && L > 0 && ldx >= d && ldb >= d && ldo >= d && ldl >= L,
                "expand_rows: bad shape");
    if (m < 1 || m > L) return grl_fail(GRL_EINVAL, "expand_rows: m = %d (1..L = %d)", m, L);
    if (alpha < 0 || alpha > 8) return grl_fail(GRL_EINVAL, "expand_rows: alpha = %d (0..8)", alpha);
    GRL_REQUIRE(!skip_self || n == nb, "expand_rows: skip_self needs x and bank to have the same rows");
    GRL_REQUIRE(!overlaps(out, n, ldo, x, n, ldx, d) && !overlaps(out, n, ldo, bank, nb, ldb, d),
                "expand_rows: out overlaps x or bank");
    if (m > EXPAND_M_MAX) return grl_fail(GRL_EUNSUPPORTED, "expand_rows: m = %d (at most %d)", m, EXPAND_M_MAX);
    const int slices = grl_ceil_div(d, EXPAND_SLICE);
    const bool vec = aligned16(x) && aligned16(bank) && aligned16(out) && ldx % 4 == 0 && ldb % 4 == 0 && ldo % 4 == 0;
    const size_t lds = (size_t)m * (sizeof(int) + sizeof(float));
    const int rows_per_launch = max(1, (1 << 23) / slices);          // rows * slices * 256 threads < 2^32
    for (int row0 = 0; row0 < n; row0 += rows_per_launch) {
        const dim3 grid((unsigned)(min(rows_per_launch, n - row0) * slices));
        if (vec)
            hipLaunchKernelGGL(expand_rows_kernel<true>, grid, dim3(EXPAND_THREADS), lds, (hipStream_t)stream, x, ldx,
                               bank, ldb, idx, dist, ldl, nb, d, L, m, alpha, skip_self, slices, row0, out, ldo);
        else
            hipLaunchKernelGGL(expand_rows_kernel<false>, grid, dim3(EXPAND_THREADS), lds, (hipStream_t)stream, x, ldx,
                               bank, ldb, idx, dist, ldl, nb, d, L, m, alpha, skip_self, slices, row0, out, ldo);
    }
    return grl_check_launch("grl_expand_rows");
}
