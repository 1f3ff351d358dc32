// Binary hash codes of a gallery: bit packing, the Hamming scan and the asymmetric tables (engine.bin_* / BinaryCodebook /
// BinaryIndex).  A gallery row is nbits bits, bit b = (z[b] > 0) of its projection z; a pair is scored by
// one XOR and one population count per 32 bits (include/grl_hip.h has the layouts).
//
// grl_bin_scan, the hot path.  A workgroup of 256 lanes owns BIN_Q = 8 queries and a slab of BIN_CPT * 256 gallery
// columns, lane l the columns slab + c * 256 + l.  Per code word w the lane loads its BIN_CPT dwords of the scan layout
// (uint32 [W][ldw], coalesced along the columns), once, and reuses them from registers for the eight queries; the query
// words are the same for every lane of the workgroup, so they are read through the scalar cache (no LDS at all) and
// enter v_xor as a scalar operand.  The 8 * BIN_CPT counts are integers in registers (v_bcnt_u32_b32 adds its second
// operand: one instruction per popcount-and-accumulate), converted once at the store.  No atomics; a query >= nq reads
// the last query's words and is not stored, a column >= n reads nothing and is not stored.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include "../../include/grl_hip.h"
#include "common.h"

namespace {

constexpr int BIN_THREADS = 256;
constexpr int BIN_Q = 8;                           // queries per workgroup
constexpr int BIN_CPT = 4;                         // gallery columns per lane
constexpr int BIN_SLAB = BIN_THREADS * BIN_CPT;
static_assert(BIN_SLAB == GRL_BIN_SLAB, "include/grl_hip.h names the slab");

__global__ __launch_bounds__(BIN_THREADS) void bin_scan_kernel(const uint32_t* __restrict__ qwords,
                                                               const uint32_t* __restrict__ words, float* __restrict__ out,
                                                               int nq, int64_t n, int W, int64_t ldw, int64_t ldo) {
    const int tid = threadIdx.x;
    const int q0 = blockIdx.y * BIN_Q;
    const int64_t g0 = (int64_t)blockIdx.x * BIN_SLAB + tid;
    const uint32_t* __restrict__ qrow[BIN_Q];                      // (uniform: blockIdx alone)
#pragma unroll
    for (int j = 0; j < BIN_Q; ++j) qrow[j] = qwords + (int64_t)(q0 + j < nq ? q0 + j : nq - 1) * W;

    int acc[BIN_CPT][BIN_Q];
#pragma unroll
    for (int c = 0; c < BIN_CPT; ++c)
#pragma unroll
        for (int j = 0; j < BIN_Q; ++j) acc[c][j] = 0;

    uint32_t next[BIN_CPT];                                        // word w + 1 is in flight while word w is counted
#pragma unroll
    for (int c = 0; c < BIN_CPT; ++c) {
        const int64_t g = g0 + (int64_t)c * BIN_THREADS;
        next[c] = g < n ? words[g] : 0u;
    }
    for (int w = 0; w < W; ++w) {
        uint32_t code[BIN_CPT];
#pragma unroll
        for (int c = 0; c < BIN_CPT; ++c) code[c] = next[c];
        if (w + 1 < W) {
            const uint32_t* __restrict__ cw = words + (int64_t)(w + 1) * ldw;
#pragma unroll
            for (int c = 0; c < BIN_CPT; ++c) {
                const int64_t g = g0 + (int64_t)c * BIN_THREADS;
                if (g < n) next[c] = cw[g];
            }
        }
#pragma unroll
        for (int j = 0; j < BIN_Q; ++j) {
            const uint32_t qw = qrow[j][w];
#pragma unroll
            for (int c = 0; c < BIN_CPT; ++c) acc[c][j] += __popc(code[c] ^ qw);
        }
    }

#pragma unroll
    for (int j = 0; j < BIN_Q; ++j) {
        if (q0 + j >= nq) break;
#pragma unroll
        for (int c = 0; c < BIN_CPT; ++c) {
            const int64_t g = g0 + (int64_t)c * BIN_THREADS;
            if (g < n) out[(q0 + j) * ldo + g] = (float)acc[c][j];
        }
    }
}

// One wave per (block of 64 rows, chunk of 64 projection columns): row by row the wave reads its 64 columns coalesced and
// ballots z > 0 (NaN, -0 and +0 give 0); lane i keeps the mask of row i of the block, so that the two words of the scan
// layout leave coalesced along the rows.  nbits % 64 == 32: the last chunk has one word.
__global__ __launch_bounds__(256) void bin_pack_kernel(const float* __restrict__ z, int64_t ldz, uint8_t* __restrict__ codes,
                                                       uint32_t* __restrict__ words, int64_t ldw, float* __restrict__ signs,
                                                       int64_t lds, int64_t n, int nbits) {
    const int lane = threadIdx.x & 63;
    const int nch = (nbits + 63) / 64, W = nbits / 32;
    const int64_t ntask = ((n + 63) / 64) * nch;
    const int64_t nwave = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t task = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); task < ntask; task += nwave) {
        const int64_t r0 = (task / nch) * 64;
        const int ch = (int)(task % nch);
        const int col = ch * 64 + lane;
        const int rows = n - r0 < 64 ? (int)(n - r0) : 64;
        unsigned long long mine = 0ull;
        for (int i = 0; i < rows; ++i) {                           // (uniform trip count: every lane reaches the ballot)
            const bool bit = col < nbits && z[(r0 + i) * ldz + col] > 0.f;
            if (signs && col < nbits) signs[(r0 + i) * lds + col] = bit ? 1.f : -1.f;
            const unsigned long long m = __ballot(bit);
            if (lane == i) mine = m;
        }
        if (lane < rows) {
            const int64_t r = r0 + lane;
            const uint32_t lo = (uint32_t)mine, hi = (uint32_t)(mine >> 32);
            const bool two = 2 * ch + 1 < W;
            if (words) {
                words[(int64_t)(2 * ch) * ldw + r] = lo;
                if (two) words[(int64_t)(2 * ch + 1) * ldw + r] = hi;
            }
            if (codes) {                                           // (rows of nbits / 8 bytes, a multiple of 4: dword stores)
                uint32_t* __restrict__ crow = reinterpret_cast<uint32_t*>(codes + r * (nbits / 8)) + 2 * ch;
                crow[0] = lo;
                if (two) crow[1] = hi;
            }
        }
    }
}

// one lane per (word w, gallery row g): the four public bytes 4w .. 4w + 3 of the row, little endian
__global__ __launch_bounds__(256) void bin_words_kernel(const uint8_t* __restrict__ codes, uint32_t* __restrict__ words,
                                                        int64_t ldw, int64_t n, int W) {
    const int64_t total = (int64_t)W * n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int w = (int)(i / n);
        const int64_t g = i - (int64_t)w * n;
        words[(int64_t)w * ldw + g] = reinterpret_cast<const uint32_t*>(codes + g * (4 * (int64_t)W))[w];
    }
}

// one lane per table entry (q, m, c): the sequential sum from +0 of -+z[q][8m + j], j = 0 .. 7 (adds and negations only)
__global__ __launch_bounds__(256) void bin_lut_kernel(const float* __restrict__ z, int64_t ldz, float* __restrict__ lut, int nq,
                                                      int M) {
    const int64_t total = (int64_t)nq * M * 256;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i & 255);
        const int64_t qm = i >> 8;
        const int64_t q = qm / M;
        const int m = (int)(qm - q * M);
        const float* __restrict__ zr = z + q * ldz + 8 * m;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = zr[j];
            s += (c >> j) & 1 ? -v : v;
        }
        lut[i] = s;
    }
}

bool bin_nbits_ok(int nbits) { return nbits >= 32 && nbits <= GRL_BIN_NBITS_MAX && nbits % 32 == 0; }
bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }

}  // namespace

extern "C" int grl_bin_scan(const uint32_t* qwords, const uint32_t* words, int64_t ldw, float* out, int64_t ldo, int nq,
                            int64_t n, int nbits, void* stream) {
    GRL_REQUIRE(qwords && words && out, "bin_scan: null");
    GRL_REQUIRE(nq >= 0 && n >= 0, "bin_scan: nq, n >= 0");
    GRL_REQUIRE(bin_nbits_ok(nbits), "bin_scan: nbits must be a multiple of 32 in 32..GRL_BIN_NBITS_MAX");
    GRL_REQUIRE(ldw >= n && ldo >= n, "bin_scan: ldw >= n and ldo >= n");
    GRL_REQUIRE(aligned4(qwords) && aligned4(words) && aligned4(out), "bin_scan: qwords, words and out must be 4-byte aligned");
    GRL_REQUIRE(nq <= GRL_BIN_NQ_MAX, "bin_scan: at most GRL_BIN_NQ_MAX = 524280 queries per call");
    if (nq == 0 || n == 0) return GRL_OK;
    const int64_t slabs = (n + BIN_SLAB - 1) / BIN_SLAB;
    GRL_REQUIRE(slabs <= INT_MAX, "bin_scan: n is too large");
    const dim3 grid((unsigned)slabs, (unsigned)((nq + BIN_Q - 1) / BIN_Q)), block(BIN_THREADS);
    hipLaunchKernelGGL(bin_scan_kernel, grid, block, 0, (hipStream_t)stream, qwords, words, out, nq, n, nbits / 32, ldw, ldo);
    return grl_check_launch("grl_bin_scan");
}

extern "C" int grl_bin_pack(const float* z, int64_t ldz, uint8_t* codes, uint32_t* words, int64_t ldw, float* signs, int64_t lds,
                            int64_t n, int nbits, void* stream) {
    GRL_REQUIRE(z && (codes || words || signs), "bin_pack: null");
    GRL_REQUIRE(n >= 0, "bin_pack: n >= 0");
    GRL_REQUIRE(bin_nbits_ok(nbits), "bin_pack: nbits must be a multiple of 32 in 32..GRL_BIN_NBITS_MAX");
    GRL_REQUIRE(ldz >= nbits, "bin_pack: ldz >= nbits");
    GRL_REQUIRE(!words || ldw >= n, "bin_pack: ldw >= n");
    GRL_REQUIRE(!signs || lds >= nbits, "bin_pack: lds >= nbits");
    GRL_REQUIRE(aligned4(z) && aligned4(codes) && aligned4(words) && aligned4(signs),
                "bin_pack: z, codes, words and signs must be 4-byte aligned");
    if (n == 0) return GRL_OK;
    const int64_t ntask = ((n + 63) / 64) * ((nbits + 63) / 64);
    hipLaunchKernelGGL(bin_pack_kernel, dim3(grid_for(ntask, 4)), dim3(256), 0, (hipStream_t)stream, z, ldz, codes, words, ldw,
                       signs, lds, n, nbits);
    return grl_check_launch("grl_bin_pack");
}

extern "C" int grl_bin_words(const uint8_t* codes, uint32_t* words, int64_t ldw, int64_t n, int nbits, void* stream) {
    GRL_REQUIRE(codes && words, "bin_words: null");
    GRL_REQUIRE(n >= 0, "bin_words: n >= 0");
    GRL_REQUIRE(bin_nbits_ok(nbits), "bin_words: nbits must be a multiple of 32 in 32..GRL_BIN_NBITS_MAX");
    GRL_REQUIRE(ldw >= n, "bin_words: ldw >= n");
    GRL_REQUIRE(aligned4(codes) && aligned4(words), "bin_words: codes and words must be 4-byte aligned");
    if (n == 0) return GRL_OK;
    hipLaunchKernelGGL(bin_words_kernel, dim3(grid_for((int64_t)(nbits / 32) * n)), dim3(256), 0, (hipStream_t)stream, codes,
                       words, ldw, n, nbits / 32);
    return grl_check_launch("grl_bin_words");
}

extern "C" int grl_bin_lut(const float* z, int64_t ldz, float* lut, int nq, int nbits, void* stream) {
    GRL_REQUIRE(z && lut, "bin_lut: null");
    GRL_REQUIRE(nq >= 0, "bin_lut: nq >= 0");
    GRL_REQUIRE(bin_nbits_ok(nbits), "bin_lut: nbits must be a multiple of 32 in 32..GRL_BIN_NBITS_MAX");
    GRL_REQUIRE(ldz >= nbits, "bin_lut: ldz >= nbits");
    GRL_REQUIRE(aligned4(z) && aligned4(lut), "bin_lut: z and lut must be 4-byte aligned");
    if (nq == 0) return GRL_OK;
    hipLaunchKernelGGL(bin_lut_kernel, dim3(grid_for((int64_t)nq * (nbits / 8) * 256)), dim3(256), 0, (hipStream_t)stream, z,
                       ldz, lut, nq, nbits / 8);
    return grl_check_launch("grl_bin_lut");
}
