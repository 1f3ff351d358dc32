// Product-quantised gallery index: the ADC scan and its small companions (engine.pq_* / PqCodebook / PqIndex, DESIGN.md
// 4ac).  A gallery row is M bytes, code m the nearest of the ksub centroids of subspace m; a query's table lut [M][ksub]
// holds its distance term to every centroid, and the distance of a pair is the sum of the M entries its codes select
// (include/grl_hip.h has the normative order: four partials, p_w over m = w, w + 4, .. ascending, (p0 + p1) + (p2 + p3)).
//
// grl_pq_scan, the hot path, is an LDS gather.  A workgroup of 256 lanes owns PQ_Q = 4 queries and a slab of
// PQ_CPT * 256 gallery columns, lane l the columns slab + c * 256 + l.  The tables are walked in chunks of PQ_MC = 16
// subspaces: the chunk's entries of the four queries are staged side by side, one float4 per (m, c) (16 * ksub * 16 bytes,
// 64 KiB at ksub = 256, two workgroups per CU), so ONE ds_read_b128 feeds four accumulators and one dword of the
// scan-layout codes (uint32 [ceil(M / 4)][n], byte b = subspace 4 * w + b, coalesced along the columns) feeds four
// subspaces of four queries.  Byte b of every dword belongs to partial b, and a partial meets its subspaces in ascending
// order whatever the chunk is: the 4 * 4 * PQ_CPT sums stay in registers across the chunks and chunking changes no bit.
// The staging loop reads the public [nq][M][ksub] tables, four coalesced dword loads per entry (one per query), and
// writes consecutive float4s; a missing query (nq % 4) stages +0 and is not stored, a column >= n gathers entry 0 and is not
// stored, a subspace >= M is skipped by a wave-uniform branch.  Adds only, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include "../../include/grl_hip.h"
#include "common.h"

namespace {

constexpr int PQ_THREADS = 256;
constexpr int PQ_Q = 4;                            // queries side by side in one LDS entry
constexpr int PQ_MC = 16;                          // subspaces per LDS chunk (a multiple of 4: whole code dwords)
constexpr int PQ_CPT = 8;                          // gallery columns per lane
constexpr int PQ_SLAB = PQ_THREADS * PQ_CPT;
constexpr int PQ_KSUB_MAX = 256;

template <int METRIC>
__global__ __launch_bounds__(PQ_THREADS) void pq_scan_kernel(const float* __restrict__ lut, const uint32_t* __restrict__ codes4,
                                                             float* __restrict__ out, int nq, int64_t n, int M, int ksub,
                                                             int64_t ldo, const float* __restrict__ rn) {
    // entry (ml, c) of the chunk = s_lut[ml * ksub + c]; ml * ksub + c <= 15 * ksub + 255 < 4096 for every byte c
    __shared__ f32x4 s_lut[PQ_MC * PQ_KSUB_MAX];
    const int tid = threadIdx.x;
    const int q0 = blockIdx.y * PQ_Q;
    const int64_t g0 = (int64_t)blockIdx.x * PQ_SLAB + tid;
    const int64_t row = (int64_t)M * ksub;                         // floats of one query's table
    const int nqv = nq - q0 < PQ_Q ? nq - q0 : PQ_Q;               // 1 .. 4 queries of this workgroup exist

    float acc[PQ_CPT][4][PQ_Q];                                    // [column][partial][query]
#pragma unroll
    for (int c = 0; c < PQ_CPT; ++c)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int j = 0; j < PQ_Q; ++j) acc[c][b][j] = 0.f;

    for (int m0 = 0; m0 < M; m0 += PQ_MC) {
        const int mc = M - m0 < PQ_MC ? M - m0 : PQ_MC;
        const int cnt = mc * ksub;
        __syncthreads();                                           // the chunk before has been read by every wave
        for (int e = tid; e < cnt; e += PQ_THREADS) {
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < PQ_Q; ++j)
                if (j < nqv) v[j] = lut[(q0 + j) * row + (int64_t)m0 * ksub + e];
            s_lut[e] = v;                                          // (consecutive lanes, consecutive 16 bytes: no bank conflict)
        }
        __syncthreads();
        for (int w = 0; w < (mc + 3) / 4; ++w) {
            const uint32_t* __restrict__ cw = codes4 + (int64_t)(m0 / 4 + w) * n;
            uint32_t code[PQ_CPT];
#pragma unroll
            for (int c = 0; c < PQ_CPT; ++c) {
                const int64_t g = g0 + (int64_t)c * PQ_THREADS;
                code[c] = g < n ? cw[g] : 0u;
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (4 * w + b >= mc) break;                        // (uniform: M is not a multiple of 4)
                const f32x4* __restrict__ tab = s_lut + (4 * w + b) * ksub;
#pragma unroll
                for (int c = 0; c < PQ_CPT; ++c) {
                    const f32x4 e = tab[(code[c] >> (8 * b)) & 255u];
#pragma unroll
                    for (int j = 0; j < PQ_Q; ++j) acc[c][b][j] += e[j];
                }
            }
        }
    }

#pragma unroll
    for (int j = 0; j < PQ_Q; ++j) {
        if (j >= nqv) break;
        const float r = METRIC == GRL_PQ_EUCLIDEAN ? rn[q0 + j] : 0.f;
#pragma unroll
        for (int c = 0; c < PQ_CPT; ++c) {
            const int64_t g = g0 + (int64_t)c * PQ_THREADS;
            float s = (acc[c][0][j] + acc[c][1][j]) + (acc[c][2][j] + acc[c][3][j]);
            if (METRIC == GRL_PQ_EUCLIDEAN) {
                s = r + s;
                s = sqrtf(s > 1e-12f ? s : 1e-12f);                // (a NaN fails the comparison: 1e-12, as the EUCLID epilogue)
            }
            if (g < n) out[(q0 + j) * ldo + g] = s;
        }
    }
}

// lut[q][m][c] = cn[m][c] + 2 * lut[q][m][c]: one exact multiply, one add
__global__ __launch_bounds__(256) void pq_lut_finish_kernel(float* __restrict__ lut, const float* __restrict__ cn, int64_t total,
                                                            int64_t row) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const float g2 = 2.f * lut[i];
        lut[i] = cn[i % row] + g2;
    }
}

// one lane per (code dword w, gallery row g): the four labels (or the four bytes of caller-supplied codes) of subspaces
// 4w .. 4w + 3 -> the dword of the scan layout, the bytes of the public layout, and the range flag
__global__ __launch_bounds__(256) void pq_pack_kernel(const int32_t* __restrict__ labels, uint8_t* __restrict__ codes,
                                                      uint32_t* __restrict__ codes4, int64_t n, int M, int ksub,
                                                      int32_t* __restrict__ flag) {
    const int nw = (M + 3) / 4;
    const int64_t total = (int64_t)nw * n;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int w = (int)(i / n);
        const int64_t g = i - (int64_t)w * n;
        uint32_t word = 0u;
        for (int b = 0; b < 4; ++b) {
            const int m = 4 * w + b;
            if (m >= M) break;
            uint32_t v;
            if (labels) {
                v = (uint32_t)labels[(int64_t)m * n + g];            // (a negative label is a huge unsigned one: flagged)
                if (v >= (uint32_t)ksub) { bad = true; v = 0u; }
                codes[g * M + m] = (uint8_t)v;
            } else {
                v = codes[g * M + m];
                if (v >= (uint32_t)ksub) { bad = true; v = 0u; }
            }
            word |= v << (8 * b);
        }
        codes4[i] = word;
    }
    if (bad) atomicOr(flag, 1);
}

// out[i][m * dsub ..] = C[m][codes[i][m]][..]: one lane per 16 bytes
__global__ __launch_bounds__(256) void pq_decode_kernel(const float* __restrict__ cb, const uint8_t* __restrict__ codes,
                                                        float* __restrict__ out, int64_t n, int M, int ksub, int dsub,
                                                        int64_t ldo) {
    const int qs = dsub / 4, qd = M * qs;                          // 16-byte pieces per subspace, per row
    const int64_t total = n * qd;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / qd;
        const int p = (int)(i - r * qd), m = p / qs, j = p - m * qs;
        int c = codes[r * M + m];
        c = c < ksub ? c : ksub - 1;                               // (callers check the codes; this only keeps a wrong call inside cb)
        const f32x4 v = *reinterpret_cast<const f32x4*>(cb + ((int64_t)m * ksub + c) * dsub + 4 * j);
        *reinterpret_cast<f32x4*>(out + r * ldo + (int64_t)m * dsub + 4 * j) = v;
    }
}

bool pq_ksub_ok(int ksub) { return ksub == 16 || ksub == 32 || ksub == 64 || ksub == 128 || ksub == 256; }

}  // namespace

extern "C" int grl_pq_scan(const float* lut, const uint32_t* codes4, float* out, int nq, int64_t n, int M, int ksub,
                           int64_t ldo, int metric, const float* rn, void* stream) {
    GRL_REQUIRE(lut && codes4 && out, "pq_scan: null");
    GRL_REQUIRE(nq >= 0 && n >= 0, "pq_scan: nq, n >= 0");
    GRL_REQUIRE(M >= 1 && M <= GRL_PQ_M_MAX, "pq_scan: M must be in 1..GRL_PQ_M_MAX");
    GRL_REQUIRE(pq_ksub_ok(ksub), "pq_scan: ksub must be 16, 32, 64, 128 or 256");
    GRL_REQUIRE(metric == GRL_PQ_COSINE || metric == GRL_PQ_EUCLIDEAN, "pq_scan: metric is not one of GRL_PQ_*");
    GRL_REQUIRE(metric == GRL_PQ_COSINE || rn, "pq_scan: GRL_PQ_EUCLIDEAN needs rn");
    GRL_REQUIRE(ldo >= n, "pq_scan: ldo >= n");
    GRL_REQUIRE(((uintptr_t)lut & 3u) == 0 && ((uintptr_t)codes4 & 3u) == 0 && ((uintptr_t)out & 3u) == 0,
                "pq_scan: lut, codes and out must be 4-byte aligned");
    if (nq == 0 || n == 0) return GRL_OK;
    const int64_t slabs = (n + PQ_SLAB - 1) / PQ_SLAB;
    GRL_REQUIRE(slabs <= INT_MAX && (nq + PQ_Q - 1) / PQ_Q <= 65535, "pq_scan: at most 262140 queries per call");
    const dim3 grid((unsigned)slabs, (unsigned)((nq + PQ_Q - 1) / PQ_Q)), block(PQ_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (metric == GRL_PQ_COSINE)
        hipLaunchKernelGGL(pq_scan_kernel<GRL_PQ_COSINE>, grid, block, 0, st, lut, codes4, out, nq, n, M, ksub, ldo, rn);
    else
        hipLaunchKernelGGL(pq_scan_kernel<GRL_PQ_EUCLIDEAN>, grid, block, 0, st, lut, codes4, out, nq, n, M, ksub, ldo, rn);
    return grl_check_launch("grl_pq_scan");
}

extern "C" int grl_pq_lut_finish(float* lut, const float* cn, int nq, int M, int ksub, void* stream) {
    GRL_REQUIRE(lut && cn, "pq_lut_finish: null");
    GRL_REQUIRE(nq >= 0, "pq_lut_finish: nq >= 0");
    GRL_REQUIRE(M >= 1 && M <= GRL_PQ_M_MAX, "pq_lut_finish: M must be in 1..GRL_PQ_M_MAX");
    GRL_REQUIRE(pq_ksub_ok(ksub), "pq_lut_finish: ksub must be 16, 32, 64, 128 or 256");
    if (nq == 0) return GRL_OK;
    const int64_t row = (int64_t)M * ksub, total = row * nq;
    hipLaunchKernelGGL(pq_lut_finish_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, lut, cn, total, row);
    return grl_check_launch("grl_pq_lut_finish");
}

extern "C" int grl_pq_pack(const int32_t* labels, uint8_t* codes, uint32_t* codes4, int64_t n, int M, int ksub, int32_t* flag,
                           void* stream) {
    GRL_REQUIRE(codes && codes4 && flag, "pq_pack: null");
    GRL_REQUIRE(n >= 0, "pq_pack: n >= 0");
    GRL_REQUIRE(M >= 1 && M <= GRL_PQ_M_MAX, "pq_pack: M must be in 1..GRL_PQ_M_MAX");
    GRL_REQUIRE(pq_ksub_ok(ksub), "pq_pack: ksub must be 16, 32, 64, 128 or 256");
    GRL_REQUIRE(((uintptr_t)codes4 & 3u) == 0, "pq_pack: codes4 must be 4-byte aligned");
    if (n == 0) return GRL_OK;
    hipLaunchKernelGGL(pq_pack_kernel, dim3(grid_for((int64_t)((M + 3) / 4) * n)), dim3(256), 0, (hipStream_t)stream, labels,
                       codes, codes4, n, M, ksub, flag);
    return grl_check_launch("grl_pq_pack");
}

extern "C" int grl_pq_decode(const float* codebooks, const uint8_t* codes, float* out, int64_t n, int M, int ksub, int dsub,
                             int64_t ldo, void* stream) {
    GRL_REQUIRE(codebooks && codes && out, "pq_decode: null");
    GRL_REQUIRE(n >= 0, "pq_decode: n >= 0");
    GRL_REQUIRE(M >= 1 && M <= GRL_PQ_M_MAX, "pq_decode: M must be in 1..GRL_PQ_M_MAX");
    GRL_REQUIRE(pq_ksub_ok(ksub), "pq_decode: ksub must be 16, 32, 64, 128 or 256");
    GRL_REQUIRE(dsub >= 4 && dsub % 4 == 0 && (int64_t)M * dsub <= INT_MAX / 4, "pq_decode: dsub must be a multiple of 4");
    GRL_REQUIRE(ldo >= (int64_t)M * dsub && ldo % 4 == 0, "pq_decode: ldo >= M * dsub and a multiple of 4");
    GRL_REQUIRE(aligned16(codebooks) && aligned16(out), "pq_decode: codebooks and out must be 16-byte aligned");
    if (n == 0) return GRL_OK;
    hipLaunchKernelGGL(pq_decode_kernel, dim3(grid_for(n * (int64_t)M * (dsub / 4))), dim3(256), 0, (hipStream_t)stream,
                       codebooks, codes, out, n, M, ksub, dsub, ldo);
    return grl_check_launch("grl_pq_decode");
}
