// Shared helpers for the libgrl_hip.so translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

int grl_fail(int code, const char* fmt, ...);          // sets the thread-local message
int grl_check_launch(const char* what);                 // hipGetLastError -> GRL_ELAUNCH

static inline int grl_ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// argument check of an extern "C" entry point
#define GRL_REQUIRE(cond, msg) do { if (!(cond)) return grl_fail(GRL_EINVAL, msg); } while (0)

// workgroups of a grid-stride launch over n items: 1 .. 8192
static inline int grid_for(int64_t n, int block = 256) {
    int64_t g = (n + block - 1) / block;
    return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

static __device__ __forceinline__ float sigmoidf_(float z) { return 1.f / (1.f + expf(-z)); }

// 8 channels of a bf16-storage tensor (16 bytes) <-> fp32 registers; 8 consecutive floats (32-byte aligned vectors)
static __device__ __forceinline__ f32x8 zero8() { return f32x8{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; }
static __device__ __forceinline__ f32x8 ld8(const __bf16* p) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
    f32x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (float)v[e];
    return r;
}
static __device__ __forceinline__ void st8(__bf16* p, const f32x8 v) {
    bf16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (__bf16)v[e];
    *reinterpret_cast<bf16x8*>(p) = r;
}
static __device__ __forceinline__ f32x8 ld8f(const float* p) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
    return f32x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}
static __device__ __forceinline__ void st8f(float* p, const f32x8 v) {
    *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
}

// first position in [lo, hi) of the ascending array a whose value is >= x
template <typename I>
static __device__ __forceinline__ I lower_bound(const int32_t* __restrict__ a, I lo, I hi, int x) {
    while (lo < hi) {
        const I mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// wave64 sum (all lanes receive the total)
static __device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// block-wide sum for <= 16 waves; `red` is >= 16 floats of LDS. All threads get the total.
static __device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < nw; ++i) t += red[i];
    return t;
}

// wave64 max (all lanes receive it)
static __device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// block-wide max for <= 16 waves; all threads receive it.
static __device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float t = red[0];
    for (int i = 1; i < nw; ++i) t = fmaxf(t, red[i]);
    return t;
}

// gemm_bf16.hip: 256 x 256 bf16-storage tile. 1 = launched, 0 = shape not covered (use the
// 128 x 128 family), < 0 = error.
struct GrlGemm;
int grl_gemm_bf16_256(const GrlGemm& d, hipStream_t s);
bool grl_gemm_bf16_256_takes(const GrlGemm& d);        // would it?  (same predicate)
int grl_gemm_bf16_256_stat_rows(const GrlGemm& d);     // rows of the statistics slab it writes (2 per 256-row tile)
int grl_gemm_validate(const GrlGemm& d);               // gemm_f32.hip: the argument checks of grl_conv_gemm_f32 (GRL_OK or grl_fail)
// gemm_mxfp8.hip: the GRL_MATH_MXFP8 datapath of grl_conv_gemm_f32 (quantise A into splitk_ws, then the MX GEMM)
int grl_gemm_mxfp8(const GrlGemm& d, hipStream_t s);
int64_t grl_gemm_mxfp8_workspace_floats(const GrlGemm& d);     // floats of scratch it needs (0: K or C not a multiple of 32)

// train.hip: BatchNorm-backward finalize over an fp32 partial slab (shared with the bf16-storage kernels of train_bf16.hip)
int grl_launch_bn_bwd_finalize(const float* slab, int rows, int C, double count, float* dgamma, float* dbeta, float* coef,
                               hipStream_t s);

// train_bnfuse.hip: BatchNorm finalize inside the apply pass (rows <= 64 slab rows, C % 64 == 0): the backward entry points of
// train.hip / train_bf16.hip launch it instead of bn_bwd_finalize + bn_bwd_apply
bool grl_bn_finapply_takes(int rows, int C);
int grl_launch_bn_bwd_finapply(int b16, const float* slab, int rows, int C, double count, float* dgamma, float* dbeta, const void* dy,
                               const void* z, const void* act, const float* mean, const float* invstd, const float* gamma, void* dz,
                               int M, void* gres, int gres_accumulate, const float* mscale, const float* mbeta, const uint8_t* bits,
                               hipStream_t s);
