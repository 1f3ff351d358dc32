// int8 scalar-quantised gallery: the quantiser, its decode and the integer-MFMA scan (engine.sq8_* / Sq8Codebook / Sq8Index,
// DESIGN.md 4ah; include/grl_hip.h has the normative arithmetic and the layouts).
//
// grl_sq8_scan, the hot path: an int8 x int8 -> int32 GEMM of the query codes [nq][dpad] against the gallery codes
// [n][dpad], both rows of K-contiguous bytes.  A workgroup of 256 lanes owns a 128 x 128 tile of the output; its four waves
// sit 2 x 2 and own 64 x 64 each: 2 x 2 accumulator tiles of v_mfma_i32_32x32x32_i8 (64 accumulator registers).  K advances
// in steps of 128 bytes: every lane carries four 16-byte chunks of each operand from global memory into registers, the
// step's 2 x 16 KiB go to LDS with rows padded to 144 bytes (16 consecutive rows then start on 16 different 16-byte bank
// slots), and the NEXT step's global loads are issued before the current step's 16 MFMAs per wave.  A fragment is 16
// consecutive bytes of a row per lane (lane l: row l & 31, bytes 16 (l >> 5) ..): both operands are read the same way, so
// the pairing of their k inside the instruction cannot matter.  The queries are the A operand: the C/D layout then has
// the gallery column on lane & 31 and a row's 32 results leave as one 128-byte store.  Integer accumulation is exact; the
// epilogue converts once and applies scale / bias / norms in registers.  No atomics, no inline assembly.
// The 1-d grid walks the query tiles fastest: the workgroups that are resident together share gallery tiles in L2 and
// the (small) query code matrix stays cached, so the gallery codes stream from memory about once.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <float.h>
#include "../../include/grl_hip.h"
#include "common.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int SQ_THREADS = 256;
constexpr int SQ_T = 128;                          // output tile, both ways
constexpr int SQ_BK = 128;                         // bytes of K per step
constexpr int SQ_LD = SQ_BK + 16;                  // LDS row stride in bytes
static_assert(SQ_T == GRL_SQ8_TILE, "include/grl_hip.h names the tile");

enum { SQ_COSINE = 0, SQ_EUCLID = 1, SQ_RAW = 2 };

template <int MODE>
__global__ __launch_bounds__(SQ_THREADS) void sq8_scan_kernel(const int8_t* __restrict__ qcodes, int64_t ldqc,
                                                              const int8_t* __restrict__ codes, int64_t ldc,
                                                              const float* __restrict__ scale, const float* __restrict__ bias,
                                                              const float* __restrict__ qq, const float* __restrict__ gg,
                                                              void* __restrict__ outv, int64_t ldo, int nq, int64_t n, int dpad,
                                                              int nqt) {
    __shared__ __attribute__((aligned(16))) int8_t sa[SQ_T * SQ_LD];
    __shared__ __attribute__((aligned(16))) int8_t sb[SQ_T * SQ_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int q0 = (int)(blockIdx.x % (unsigned)nqt) * SQ_T;
    const int64_t g0 = (int64_t)(blockIdx.x / (unsigned)nqt) * SQ_T;

    // staging: chunk i of a lane is row (tid >> 3) + 32 i, bytes kc .. kc + 15 of the step.  A row beyond the operand is read
    // as the operand's last row (in bounds; its results are never stored), and in the half step that ends a dpad with
    // dpad % 128 == 64 the lanes of the upper half re-read the lower half (in bounds; the MFMAs of that step stop at 64).
    const int srow = tid >> 3, kc = (tid & 7) * 16;
    const int8_t* __restrict__ pa[4];
    const int8_t* __restrict__ pb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int qr = q0 + srow + 32 * i;
        const int64_t gr = g0 + srow + 32 * i;
        pa[i] = qcodes + (int64_t)(qr < nq ? qr : nq - 1) * ldqc + kc;
        pb[i] = codes + (gr < n ? gr : n - 1) * ldc + kc;
    }
    v4i ra[4], rb[4];
    auto load = [&](int k0) {
        const int k = k0 + kc < dpad ? k0 : k0 - 64;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ra[i] = *reinterpret_cast<const v4i*>(pa[i] + k);
            rb[i] = *reinterpret_cast<const v4i*>(pb[i] + k);
        }
    };

    v16i acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][c][r] = 0;

    const int8_t* fa = sa + (wr * 64 + (lane & 31)) * SQ_LD + (lane >> 5) * 16;
    const int8_t* fb = sb + (wc * 64 + (lane & 31)) * SQ_LD + (lane >> 5) * 16;

    load(0);
    for (int k0 = 0; k0 < dpad; k0 += SQ_BK) {
        __syncthreads();                                           // the previous step's fragments have been read
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<v4i*>(sa + (srow + 32 * i) * SQ_LD + kc) = ra[i];
            *reinterpret_cast<v4i*>(sb + (srow + 32 * i) * SQ_LD + kc) = rb[i];
        }
        __syncthreads();
        if (k0 + SQ_BK < dpad) load(k0 + SQ_BK);                   // in flight under this step's MFMAs
        const int nks = dpad - k0 >= SQ_BK ? 4 : 2;                // (uniform)
        for (int ks = 0; ks < nks; ++ks) {
            v4i a[2], b[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                a[m] = *reinterpret_cast<const v4i*>(fa + m * 32 * SQ_LD + ks * 32);
                b[m] = *reinterpret_cast<const v4i*>(fb + m * 32 * SQ_LD + ks * 32);
            }
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int c = 0; c < 2; ++c) acc[m][c] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[m], b[c], acc[m][c], 0, 0, 0);
        }
    }

    // C/D layout of the 32 x 32 shape: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int64_t g = g0 + wc * 64 + c * 32 + (lane & 31);
        if (g >= n) continue;
        float gn = 0.f;
        if (MODE == SQ_EUCLID) gn = gg[g];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int q = q0 + wr * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (q >= nq) continue;
                const int isum = acc[m][c][r];
                if (MODE == SQ_RAW) {
                    static_cast<int32_t*>(outv)[(int64_t)q * ldo + g] = isum;
                } else {
                    const float dot = scale[q] * (float)isum + bias[q];
                    float v;
                    if (MODE == SQ_COSINE) {
                        v = -dot;
                    } else {
                        const float t = (qq[q] + gn) - 2.0f * dot;
                        v = sqrtf(t > 1e-12f ? t : 1e-12f);
                    }
                    static_cast<float*>(outv)[(int64_t)q * ldo + g] = v;
                }
            }
        }
    }
}

// amax[j] = max_i |x[i][j] - mean[j]|: a lane owns a column over a slab of rows; the bits of non-negative floats order as
// unsigned integers, so the slabs meet in an integer atomic max (order free).  NaN never compares greater.
__global__ __launch_bounds__(256) void sq8_absmax_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ mean,
                                                         unsigned int* __restrict__ amax, int64_t n, int d, int64_t rows_per) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= d) return;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per;
    const int64_t r1 = r0 + rows_per < n ? r0 + rows_per : n;
    const float m = mean[col];
    float best = 0.f;
    for (int64_t r = r0; r < r1; ++r) {
        const float v = fabsf(x[r * ldx + col] - m);
        if (v > best) best = v;
    }
    if (r0 < r1) atomicMax(amax + col, __float_as_uint(best));
}

__global__ __launch_bounds__(256) void sq8_steps_kernel(const float* __restrict__ amax, float* __restrict__ delta,
                                                        float* __restrict__ inv, int d) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d) return;
    if (amax) {
        const float a = amax[j];
        delta[j] = a / 127.0f;
        inv[j] = a == 0.f ? 0.f : 127.0f / a;
    } else {
        const float dl = delta[j];
        inv[j] = dl == 0.f ? 0.f : 127.0f / (127.0f * dl);
    }
}

__device__ __forceinline__ int sq8_round(float v) {               // NaN -> 0, else rint clamped to -127 .. 127
    if (v != v) return 0;
    const float r = rintf(v);
    return r >= 127.f ? 127 : r <= -127.f ? -127 : (int)r;
}

// one lane per dword of a code row: columns 4w .. 4w + 3, the columns >= d as 0
__global__ __launch_bounds__(256) void sq8_encode_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ mean,
                                                         const float* __restrict__ inv, int8_t* __restrict__ codes, int64_t ldc,
                                                         int64_t n, int d, int wpr) {
    const int64_t total = n * wpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / wpr;
        const int w = (int)(i - row * wpr);
        uint32_t word = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = 4 * w + b;
            if (j < d) word |= (uint32_t)(uint8_t)(int8_t)sq8_round((x[row * ldx + j] - mean[j]) * inv[j]) << (8 * b);
        }
        *reinterpret_cast<uint32_t*>(codes + row * ldc + 4 * w) = word;
    }
}

__global__ __launch_bounds__(256) void sq8_decode_kernel(const int8_t* __restrict__ codes, int64_t ldc, const float* __restrict__ mean,
                                                         const float* __restrict__ delta, float* __restrict__ out, int64_t ldo,
                                                         int64_t n, int d) {
    const int64_t total = n * d;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / d;
        const int j = (int)(i - row * d);
        const float t = delta[j] * (float)codes[row * ldc + j];
        out[row * ldo + j] = mean[j] + t;
    }
}

// one workgroup per query row: the maximum of the finite |w| (order free), then the codes
__global__ __launch_bounds__(256) void sq8_query_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ delta,
                                                        int8_t* __restrict__ qcodes, int64_t ldc, float* __restrict__ scale, int d,
                                                        int dpad) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const float* __restrict__ qr = q + (int64_t)blockIdx.x * ldq;
    float s = 0.f;
    for (int j = tid; j < d; j += 256) {
        const float a = fabsf(qr[j] * delta[j]);
        if (a <= FLT_MAX && a > s) s = a;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float t = __shfl_xor(s, o);
        if (t > s) s = t;
    }
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    s = red[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (red[w] > s) s = red[w];
    const float r = 127.0f / s;
    int8_t* __restrict__ crow = qcodes + (int64_t)blockIdx.x * ldc;
    for (int w = tid; w < dpad / 4; w += 256) {
        uint32_t word = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = 4 * w + b;
            if (j < d && s != 0.f) {
                const float wv = qr[j] * delta[j];
                if (fabsf(wv) <= FLT_MAX) word |= (uint32_t)(uint8_t)(int8_t)sq8_round(wv * r) << (8 * b);
            }
        }
        *reinterpret_cast<uint32_t*>(crow + 4 * w) = word;
    }
    if (tid == 0) scale[blockIdx.x] = s / 127.0f;
}

bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }
bool sq8_d_ok(int d) { return d >= 1 && d <= GRL_SQ8_D_MAX; }
int sq8_dpad(int d) { return (d + 63) / 64 * 64; }

template <int MODE>
int sq8_scan_launch(const int8_t* qcodes, int64_t ldqc, const int8_t* codes, int64_t ldc, const float* scale, const float* bias,
                    const float* qq, const float* gg, void* out, int64_t ldo, int nq, int64_t n, int dpad, hipStream_t st,
                    const char* what) {
    const int64_t nqt = (nq + SQ_T - 1) / SQ_T, ngt = (n + SQ_T - 1) / SQ_T;
    if (nqt * ngt > INT_MAX) return grl_fail(GRL_EINVAL, "sq8_scan: nq * n is too large for one launch");
    hipLaunchKernelGGL(sq8_scan_kernel<MODE>, dim3((unsigned)(nqt * ngt)), dim3(SQ_THREADS), 0, st, qcodes, ldqc, codes, ldc,
                       scale, bias, qq, gg, out, ldo, nq, n, dpad, (int)nqt);
    return grl_check_launch(what);
}

}  // namespace

#define SQ8_SCAN_REQUIRE(name)                                                                                               \
    GRL_REQUIRE(qcodes && codes && out, name ": null");                                                                      \
    GRL_REQUIRE(nq >= 0 && n >= 0, name ": nq, n >= 0");                                                                     \
    GRL_REQUIRE(dpad >= 64 && dpad <= GRL_SQ8_D_MAX && dpad % 64 == 0, name ": dpad must be a multiple of 64 in 64..GRL_SQ8_D_MAX"); \
    GRL_REQUIRE(ldqc >= dpad && ldc >= dpad && ldqc % 16 == 0 && ldc % 16 == 0,                                              \
                name ": ldqc and ldc must be >= dpad and multiples of 16");                                                  \
    GRL_REQUIRE(ldo >= n, name ": ldo >= n");                                                                                \
    GRL_REQUIRE(aligned16(qcodes) && aligned16(codes), name ": qcodes and codes must be 16-byte aligned");                   \
    GRL_REQUIRE(nq <= GRL_SQ8_NQ_MAX, name ": at most GRL_SQ8_NQ_MAX = 1048576 queries per call")

extern "C" int grl_sq8_scan(const int8_t* qcodes, int64_t ldqc, const int8_t* codes, int64_t ldc, const float* scale,
                            const float* bias, const float* qq, const float* gg, float* out, int64_t ldo, int nq, int64_t n,
                            int dpad, int metric, void* stream) {
    SQ8_SCAN_REQUIRE("sq8_scan");
    GRL_REQUIRE(scale && bias, "sq8_scan: null");
    GRL_REQUIRE(metric == GRL_PQ_COSINE || metric == GRL_PQ_EUCLIDEAN, "sq8_scan: unknown metric");
    GRL_REQUIRE(metric == GRL_PQ_COSINE || (qq && gg), "sq8_scan: GRL_PQ_EUCLIDEAN needs qq and gg");
    GRL_REQUIRE(aligned4(scale) && aligned4(bias) && aligned4(qq) && aligned4(gg) && aligned4(out),
                "sq8_scan: scale, bias, qq, gg and out must be 4-byte aligned");
    if (nq == 0 || n == 0) return GRL_OK;
    if (metric == GRL_PQ_COSINE)
        return sq8_scan_launch<SQ_COSINE>(qcodes, ldqc, codes, ldc, scale, bias, qq, gg, out, ldo, nq, n, dpad, (hipStream_t)stream,
                                          "grl_sq8_scan");
    return sq8_scan_launch<SQ_EUCLID>(qcodes, ldqc, codes, ldc, scale, bias, qq, gg, out, ldo, nq, n, dpad, (hipStream_t)stream,
                                      "grl_sq8_scan");
}

extern "C" int grl_sq8_scan_i32(const int8_t* qcodes, int64_t ldqc, const int8_t* codes, int64_t ldc, int32_t* out, int64_t ldo,
                                int nq, int64_t n, int dpad, void* stream) {
    SQ8_SCAN_REQUIRE("sq8_scan_i32");
    GRL_REQUIRE(aligned4(out), "sq8_scan_i32: out must be 4-byte aligned");
    if (nq == 0 || n == 0) return GRL_OK;
    return sq8_scan_launch<SQ_RAW>(qcodes, ldqc, codes, ldc, nullptr, nullptr, nullptr, nullptr, out, ldo, nq, n, dpad,
                                   (hipStream_t)stream, "grl_sq8_scan_i32");
}

extern "C" int grl_sq8_absmax(const float* x, int64_t ldx, const float* mean, float* amax, int64_t n, int d, void* stream) {
    GRL_REQUIRE(x && mean && amax, "sq8_absmax: null");
    GRL_REQUIRE(n >= 0, "sq8_absmax: n >= 0");
    GRL_REQUIRE(sq8_d_ok(d), "sq8_absmax: d must be in 1..GRL_SQ8_D_MAX");
    GRL_REQUIRE(ldx >= d, "sq8_absmax: ldx >= d");
    GRL_REQUIRE(aligned4(x) && aligned4(mean) && aligned4(amax), "sq8_absmax: x, mean and amax must be 4-byte aligned");
    if (hipMemsetAsync(amax, 0, sizeof(float) * (size_t)d, (hipStream_t)stream) != hipSuccess)
        return grl_fail(GRL_ELAUNCH, "sq8_absmax: hipMemsetAsync failed");
    if (n == 0) return GRL_OK;
    int64_t slabs = (n + 255) / 256;
    if (slabs > 1024) slabs = 1024;
    const int64_t rows_per = (n + slabs - 1) / slabs;
    hipLaunchKernelGGL(sq8_absmax_kernel, dim3((unsigned)((d + 255) / 256), (unsigned)slabs), dim3(256), 0, (hipStream_t)stream, x,
                       ldx, mean, reinterpret_cast<unsigned int*>(amax), n, d, rows_per);
    return grl_check_launch("grl_sq8_absmax");
}

extern "C" int grl_sq8_steps(const float* amax, float* delta, float* inv, int d, void* stream) {
    GRL_REQUIRE(delta && inv, "sq8_steps: null");
    GRL_REQUIRE(sq8_d_ok(d), "sq8_steps: d must be in 1..GRL_SQ8_D_MAX");
    GRL_REQUIRE(aligned4(amax) && aligned4(delta) && aligned4(inv), "sq8_steps: amax, delta and inv must be 4-byte aligned");
    hipLaunchKernelGGL(sq8_steps_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, (hipStream_t)stream, amax, delta, inv, d);
    return grl_check_launch("grl_sq8_steps");
}

extern "C" int grl_sq8_encode(const float* x, int64_t ldx, const float* mean, const float* inv, int8_t* codes, int64_t ldc,
                              int64_t n, int d, void* stream) {
    GRL_REQUIRE(x && mean && inv && codes, "sq8_encode: null");
    GRL_REQUIRE(n >= 0, "sq8_encode: n >= 0");
    GRL_REQUIRE(sq8_d_ok(d), "sq8_encode: d must be in 1..GRL_SQ8_D_MAX");
    GRL_REQUIRE(ldx >= d, "sq8_encode: ldx >= d");
    GRL_REQUIRE(ldc >= sq8_dpad(d) && ldc % 16 == 0, "sq8_encode: ldc must be >= dpad and a multiple of 16");
    GRL_REQUIRE(aligned4(x) && aligned4(mean) && aligned4(inv), "sq8_encode: x, mean and inv must be 4-byte aligned");
    GRL_REQUIRE(aligned16(codes), "sq8_encode: codes must be 16-byte aligned");
    if (n == 0) return GRL_OK;
    const int wpr = sq8_dpad(d) / 4;
    hipLaunchKernelGGL(sq8_encode_kernel, dim3(grid_for(n * wpr)), dim3(256), 0, (hipStream_t)stream, x, ldx, mean, inv, codes, ldc,
                       n, d, wpr);
    return grl_check_launch("grl_sq8_encode");
}

extern "C" int grl_sq8_decode(const int8_t* codes, int64_t ldc, const float* mean, const float* delta, float* out, int64_t ldo,
                              int64_t n, int d, void* stream) {
    GRL_REQUIRE(codes && mean && delta && out, "sq8_decode: null");
    GRL_REQUIRE(n >= 0, "sq8_decode: n >= 0");
    GRL_REQUIRE(sq8_d_ok(d), "sq8_decode: d must be in 1..GRL_SQ8_D_MAX");
    GRL_REQUIRE(ldc >= d && ldo >= d, "sq8_decode: ldc >= d and ldo >= d");
    GRL_REQUIRE(aligned4(mean) && aligned4(delta) && aligned4(out), "sq8_decode: mean, delta and out must be 4-byte aligned");
    if (n == 0) return GRL_OK;
    hipLaunchKernelGGL(sq8_decode_kernel, dim3(grid_for(n * d)), dim3(256), 0, (hipStream_t)stream, codes, ldc, mean, delta, out,
                       ldo, n, d);
    return grl_check_launch("grl_sq8_decode");
}

extern "C" int grl_sq8_query(const float* q, int64_t ldq, const float* delta, int8_t* qcodes, int64_t ldc, float* scale, int nq,
                             int d, void* stream) {
    GRL_REQUIRE(q && delta && qcodes && scale, "sq8_query: null");
    GRL_REQUIRE(nq >= 0, "sq8_query: nq >= 0");
    GRL_REQUIRE(sq8_d_ok(d), "sq8_query: d must be in 1..GRL_SQ8_D_MAX");
    GRL_REQUIRE(ldq >= d, "sq8_query: ldq >= d");
    GRL_REQUIRE(ldc >= sq8_dpad(d) && ldc % 16 == 0, "sq8_query: ldc must be >= dpad and a multiple of 16");
    GRL_REQUIRE(aligned4(q) && aligned4(delta) && aligned4(scale), "sq8_query: q, delta and scale must be 4-byte aligned");
    GRL_REQUIRE(aligned16(qcodes), "sq8_query: qcodes must be 16-byte aligned");
    GRL_REQUIRE(nq <= GRL_SQ8_NQ_MAX, "sq8_query: at most GRL_SQ8_NQ_MAX = 1048576 queries per call");
    if (nq == 0) return GRL_OK;
    hipLaunchKernelGGL(sq8_query_kernel, dim3((unsigned)nq), dim3(256), 0, (hipStream_t)stream, q, ldq, delta, qcodes, ldc, scale, d,
                       sq8_dpad(d));
    return grl_check_launch("grl_sq8_query");
}
