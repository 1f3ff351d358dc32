// IVF-PQ gallery index: the per-query scan of inverted lists and its small companions (engine.ivf_* / IvfPqCodebook /
// IvfPqIndex).  The gallery is split into nlist inverted lists by a coarse quantiser; inside a list the rows
// sit in ascending gallery index, and their product-quantiser codes (of the RESIDUAL to the list centroid) are kept in the
// scan layout of pq.hip, in list order.  A query scans only the lists it probes.
//
// grl_ivf_scan, the hot path.  Every query sees a VIRTUAL ROW: the lists of its probe ranks [0, np) of the chunk, one after
// the other; off [nq][np + 1] holds the prefix sums of their lengths.  A workgroup of 256 lanes owns one query and a slab
// of IVF_CPT * 256 consecutive virtual columns, lane l the columns slab + c * 256 + l: work is balanced whatever the list
// lengths are, and lanes that are consecutive inside a list read consecutive dwords of the codes.  A column is mapped to
// (probe rank j, list position p) by a binary search over the <= 1025 offsets, staged in LDS once.  The query's table is
// walked in chunks of IVF_MC = 16 subspaces (16 * ksub * 4 bytes, 16 KiB at ksub = 256; with 116 VGPRs four workgroups
// share a CU, four waves per SIMD, which 4-byte LDS gathers need to reach their rate).  Byte b of every code dword belongs
// to partial b and a partial meets its subspaces in ascending order whatever the chunk is: the 4 * IVF_CPT sums stay in
// registers across the chunks and chunking changes no bit.  A slab at or beyond the query's total writes its padding and
// leaves before any staging.  Adds only (and the one exact doubling of the Euclidean form), no atomics, plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include "../../include/grl_hip.h"
#include "common.h"

namespace {

constexpr int IVF_THREADS = 256;
#ifndef GRL_IVF_MC
#define GRL_IVF_MC 16                              // (-DGRL_IVF_MC=8 / 32 builds the variants EXPERIMENTS.md compares)
#endif
constexpr int IVF_MC = GRL_IVF_MC;                 // subspaces per LDS chunk (a multiple of 4: whole code dwords)
static_assert(IVF_MC >= 4 && IVF_MC % 4 == 0 && IVF_MC <= 64, "IVF_MC: whole code dwords, at most 64 KiB of tables");
constexpr int IVF_CPT = 8;                         // virtual columns per lane
constexpr int IVF_SLAB = IVF_THREADS * IVF_CPT;
constexpr int IVF_KSUB_MAX = 256;
constexpr int IVF_NPROBE_MAX = GRL_IVF_NPROBE_MAX;

template <int METRIC>
__global__ __launch_bounds__(IVF_THREADS) void ivf_scan_kernel(const float* __restrict__ lut, const uint32_t* __restrict__ codes4,
                                                               const int32_t* __restrict__ ids, const int64_t* __restrict__ list_ptr,
                                                               const int32_t* __restrict__ probe, const float* __restrict__ g0,
                                                               int64_t ldp, int np, const int32_t* __restrict__ off,
                                                               const float* __restrict__ xn, const float* __restrict__ rn,
                                                               float* __restrict__ out, int32_t* __restrict__ cidx, int64_t ldo,
                                                               int width, int64_t n, int nlist, int M, int ksub) {
    __shared__ float s_lut[IVF_MC * IVF_KSUB_MAX];                 // entry (ml, c) of the chunk = s_lut[ml * ksub + c]
    __shared__ int32_t s_off[IVF_NPROBE_MAX + 1];
    const int tid = threadIdx.x;
    const int q = blockIdx.y;
    const int64_t col0 = (int64_t)blockIdx.x * IVF_SLAB + tid;
    const int32_t* __restrict__ qoff = off + (int64_t)q * (np + 1);
    const int total = qoff[np];
    float* __restrict__ orow = out + (int64_t)q * ldo;
    int32_t* __restrict__ crow = cidx + (int64_t)q * ldo;

    if ((int64_t)blockIdx.x * IVF_SLAB >= total) {                 // (uniform) nothing of this query's lists in the slab
#pragma unroll
        for (int c = 0; c < IVF_CPT; ++c) {
            const int64_t col = col0 + c * IVF_THREADS;
            if (col < width) { orow[col] = INFINITY; crow[col] = -1; }
        }
        return;
    }
    for (int e = tid; e <= np; e += IVF_THREADS) s_off[e] = qoff[e];
    __syncthreads();

    int pos[IVF_CPT];                                              // list-order position of the column's row (n < 2^31)
    float gq[IVF_CPT];                                             // g0 of the column's probe
    bool live[IVF_CPT];
#pragma unroll
    for (int c = 0; c < IVF_CPT; ++c) {
        const int64_t col = col0 + c * IVF_THREADS;
        live[c] = col < total;
        pos[c] = 0;
        gq[c] = 0.f;
        if (live[c]) {
            int lo = 0, hi = np;                                   // first i in (0, np] with s_off[i] > col; its probe is i - 1
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_off[mid + 1] > (int)col) hi = mid; else lo = mid + 1;
            }
            int l = probe[(int64_t)q * ldp + lo];
            l = l < 0 ? 0 : (l < nlist ? l : nlist - 1);           // (callers pass search's lists; this only keeps a wrong call inside)
            const int64_t p = list_ptr[l] + (col - s_off[lo]);
            pos[c] = (int)(p < 0 ? 0 : (p < n ? p : n - 1));
            gq[c] = g0[(int64_t)q * ldp + lo];
        }
    }

    float acc[IVF_CPT][4];                                         // [column][partial]
#pragma unroll
    for (int c = 0; c < IVF_CPT; ++c)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[c][b] = 0.f;

    const float* __restrict__ qlut = lut + (int64_t)q * M * ksub;
    for (int m0 = 0; m0 < M; m0 += IVF_MC) {
        const int mc = M - m0 < IVF_MC ? M - m0 : IVF_MC;
        const int cnt = mc * ksub;
        __syncthreads();                                           // the chunk before has been read by every wave
        for (int e = tid; e < cnt; e += IVF_THREADS) s_lut[e] = qlut[(int64_t)m0 * ksub + e];
        __syncthreads();
        for (int w = 0; w < (mc + 3) / 4; ++w) {
            const uint32_t* __restrict__ cw = codes4 + (int64_t)(m0 / 4 + w) * n;
            uint32_t code[IVF_CPT];
#pragma unroll
            for (int c = 0; c < IVF_CPT; ++c) code[c] = live[c] ? cw[pos[c]] : 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (4 * w + b >= mc) break;                        // (uniform: M is not a multiple of 4)
                const float* __restrict__ tab = s_lut + (4 * w + b) * ksub;
#pragma unroll
                for (int c = 0; c < IVF_CPT; ++c) acc[c][b] += tab[(code[c] >> (8 * b)) & (uint32_t)(ksub - 1)];
            }
        }
    }

    const float r = METRIC == GRL_PQ_EUCLIDEAN ? rn[q] : 0.f;
#pragma unroll
    for (int c = 0; c < IVF_CPT; ++c) {
        const int64_t col = col0 + c * IVF_THREADS;
        if (col >= width) continue;
        if (!live[c]) { orow[col] = INFINITY; crow[col] = -1; continue; }
        const float s = (acc[c][0] + acc[c][1]) + (acc[c][2] + acc[c][3]);
        float t = gq[c] + s;
        if (METRIC == GRL_PQ_EUCLIDEAN) {
            const float u = xn[pos[c]] + 2.f * t;
            const float v = r + u;
            t = sqrtf(v > 1e-12f ? v : 1e-12f);                    // (a NaN fails the comparison: 1e-12, as the EUCLID epilogue)
        }
        orow[col] = t;
        crow[col] = ids[pos[c]];
    }
}

// out[i][c] = x[i][c] - coarse[labels[i]][c]: one rounded subtraction per element
__global__ __launch_bounds__(256) void ivf_residual_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ labels,
                                                           const float* __restrict__ coarse, int nlist, float* __restrict__ out,
                                                           int64_t ldo, int64_t rows, int d) {
    const int64_t total = rows * d;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / d;
        const int c = (int)(i - r * d);
        int l = labels[r];
        l = l < 0 ? 0 : (l < nlist ? l : nlist - 1);               // (callers check the labels; this only keeps a wrong call inside coarse)
        out[r * ldo + c] = x[r * ldx + c] - coarse[(int64_t)l * d + c];
    }
}

// out[i][m * dsub + j] = coarse[labels[i]][m * dsub + j] + cb[m][codes[i][m]][j]: one rounded add per element
__global__ __launch_bounds__(256) void ivf_reconstruct_kernel(const float* __restrict__ coarse, const float* __restrict__ cb,
                                                              const int32_t* __restrict__ labels, const uint8_t* __restrict__ codes,
                                                              float* __restrict__ out, int64_t rows, int nlist, int M, int ksub,
                                                              int dsub, int64_t ldo) {
    const int d = M * dsub;
    const int64_t total = rows * d;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / d;
        const int c = (int)(i - r * d), m = c / dsub, j = c - m * dsub;
        int l = labels[r];
        l = l < 0 ? 0 : (l < nlist ? l : nlist - 1);
        int code = codes[r * M + m];
        code = code < ksub ? code : ksub - 1;
        out[r * ldo + c] = coarse[(int64_t)l * d + c] + cb[((int64_t)m * ksub + code) * dsub + j];
    }
}

// *flag |= 1 when a label is outside 0..nlist-1
__global__ __launch_bounds__(256) void ivf_check_labels_kernel(const int32_t* __restrict__ labels, int64_t n, int nlist,
                                                               int32_t* __restrict__ flag) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        bad |= (uint32_t)labels[i] >= (uint32_t)nlist;             // (a negative label is a huge unsigned one)
    if (bad) atomicOr(flag, 1);
}

bool ivf_ksub_ok(int ksub) { return ksub == 16 || ksub == 32 || ksub == 64 || ksub == 128 || ksub == 256; }

}  // namespace

extern "C" int grl_ivf_scan(const float* lut, const uint32_t* codes4, const int32_t* ids, const int64_t* list_ptr,
                            const int32_t* probe, const float* g0, int64_t ldp, int np, const int32_t* off, const float* xn,
                            const float* rn, float* out, int32_t* cidx, int64_t ldo, int width, int nq, int64_t n, int nlist,
                            int M, int ksub, int metric, void* stream) {
    GRL_REQUIRE(lut && codes4 && ids && list_ptr && probe && g0 && off && out && cidx, "ivf_scan: null");
    GRL_REQUIRE(nq >= 0 && n >= 0 && n <= INT_MAX && width >= 0, "ivf_scan: nq, width >= 0 and 0 <= n < 2^31");
    GRL_REQUIRE(nlist >= 1 && nlist <= GRL_IVF_NLIST_MAX, "ivf_scan: nlist must be in 1..GRL_IVF_NLIST_MAX");
    GRL_REQUIRE(np >= 1 && np <= GRL_IVF_NPROBE_MAX && np <= nlist, "ivf_scan: np must be in 1..min(nlist, GRL_IVF_NPROBE_MAX)");
    GRL_REQUIRE(M >= 1 && M <= GRL_PQ_M_MAX, "ivf_scan: M must be in 1..GRL_PQ_M_MAX");
    GRL_REQUIRE(ivf_ksub_ok(ksub), "ivf_scan: ksub must be 16, 32, 64, 128 or 256");
    GRL_REQUIRE(metric == GRL_PQ_COSINE || metric == GRL_PQ_EUCLIDEAN, "ivf_scan: metric is not one of GRL_PQ_*");
    GRL_REQUIRE(metric == GRL_PQ_COSINE || (xn && rn), "ivf_scan: GRL_PQ_EUCLIDEAN needs xn and rn");
    GRL_REQUIRE(ldp >= np && ldo >= width, "ivf_scan: ldp >= np and ldo >= width");
    GRL_REQUIRE(nq <= 65535, "ivf_scan: at most 65535 queries per call");
    GRL_REQUIRE(((uintptr_t)lut & 3u) == 0 && ((uintptr_t)codes4 & 3u) == 0 && ((uintptr_t)out & 3u) == 0 &&
                ((uintptr_t)cidx & 3u) == 0 && ((uintptr_t)list_ptr & 7u) == 0,
                "ivf_scan: lut, codes, out and cidx must be 4-byte aligned, list_ptr 8-byte aligned");
    GRL_REQUIRE(((uintptr_t)ids & 3u) == 0 && ((uintptr_t)probe & 3u) == 0 && ((uintptr_t)g0 & 3u) == 0 &&
                ((uintptr_t)off & 3u) == 0 && ((uintptr_t)xn & 3u) == 0 && ((uintptr_t)rn & 3u) == 0,
                "ivf_scan: ids, probe, g0, off, xn and rn must be 4-byte aligned");
    if (nq == 0 || width == 0 || n == 0) return GRL_OK;
    const dim3 grid((unsigned)((width + IVF_SLAB - 1) / IVF_SLAB), (unsigned)nq), block(IVF_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (metric == GRL_PQ_COSINE)
        hipLaunchKernelGGL(ivf_scan_kernel<GRL_PQ_COSINE>, grid, block, 0, st, lut, codes4, ids, list_ptr, probe, g0, ldp, np, off,
                           xn, rn, out, cidx, ldo, width, n, nlist, M, ksub);
    else
        hipLaunchKernelGGL(ivf_scan_kernel<GRL_PQ_EUCLIDEAN>, grid, block, 0, st, lut, codes4, ids, list_ptr, probe, g0, ldp, np,
                           off, xn, rn, out, cidx, ldo, width, n, nlist, M, ksub);
    return grl_check_launch("grl_ivf_scan");
}

extern "C" int grl_ivf_residual(const float* x, int64_t ldx, const int32_t* labels, const float* coarse, int nlist, float* out,
                                int64_t ldo, int64_t rows, int d, void* stream) {
    GRL_REQUIRE(x && labels && coarse && out, "ivf_residual: null");
    GRL_REQUIRE(rows >= 0 && d >= 1, "ivf_residual: rows >= 0, d >= 1");
    GRL_REQUIRE(nlist >= 1 && nlist <= GRL_IVF_NLIST_MAX, "ivf_residual: nlist must be in 1..GRL_IVF_NLIST_MAX");
    GRL_REQUIRE(ldx >= d && ldo >= d, "ivf_residual: ldx >= d and ldo >= d");
    if (rows == 0) return GRL_OK;
    hipLaunchKernelGGL(ivf_residual_kernel, dim3(grid_for(rows * d)), dim3(256), 0, (hipStream_t)stream, x, ldx, labels, coarse,
                       nlist, out, ldo, rows, d);
    return grl_check_launch("grl_ivf_residual");
}

extern "C" int grl_ivf_reconstruct(const float* coarse, const float* codebooks, const int32_t* labels, const uint8_t* codes,
                                   float* out, int64_t rows, int nlist, int M, int ksub, int dsub, int64_t ldo, void* stream) {
    GRL_REQUIRE(coarse && codebooks && labels && codes && out, "ivf_reconstruct: null");
    GRL_REQUIRE(rows >= 0, "ivf_reconstruct: rows >= 0");
    GRL_REQUIRE(nlist >= 1 && nlist <= GRL_IVF_NLIST_MAX, "ivf_reconstruct: nlist must be in 1..GRL_IVF_NLIST_MAX");
    GRL_REQUIRE(M >= 1 && M <= GRL_PQ_M_MAX, "ivf_reconstruct: M must be in 1..GRL_PQ_M_MAX");
    GRL_REQUIRE(ivf_ksub_ok(ksub), "ivf_reconstruct: ksub must be 16, 32, 64, 128 or 256");
    GRL_REQUIRE(dsub >= 1 && (int64_t)M * dsub <= INT_MAX / 4, "ivf_reconstruct: dsub >= 1 and M * dsub < 2^29");
    GRL_REQUIRE(ldo >= (int64_t)M * dsub, "ivf_reconstruct: ldo >= M * dsub");
    if (rows == 0) return GRL_OK;
    hipLaunchKernelGGL(ivf_reconstruct_kernel, dim3(grid_for(rows * M * dsub)), dim3(256), 0, (hipStream_t)stream, coarse,
                       codebooks, labels, codes, out, rows, nlist, M, ksub, dsub, ldo);
    return grl_check_launch("grl_ivf_reconstruct");
}

extern "C" int grl_ivf_check_labels(const int32_t* labels, int64_t n, int nlist, int32_t* flag, void* stream) {
    GRL_REQUIRE(labels && flag, "ivf_check_labels: null");
    GRL_REQUIRE(n >= 0, "ivf_check_labels: n >= 0");
    GRL_REQUIRE(nlist >= 1 && nlist <= GRL_IVF_NLIST_MAX, "ivf_check_labels: nlist must be in 1..GRL_IVF_NLIST_MAX");
    if (n == 0) return GRL_OK;
    hipLaunchKernelGGL(ivf_check_labels_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, labels, n, nlist, flag);
    return grl_check_launch("grl_ivf_check_labels");
}
