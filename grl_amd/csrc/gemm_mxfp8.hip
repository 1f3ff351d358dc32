// GRL_MATH_MXFP8: the conv / linear GEMM of the bf16-storage eval pipeline on MX-FP8 operands (OCP MX v1.0, e4m3fn
// elements, one E8M0 scale per 32 consecutive k) through gfx950's block-scaled MFMA v_mfma_scale_f32_32x32x64_f8f6f4.
//
// Two launches per GEMM:
//   1. mx_quant_kernel: the bf16 activations (dense A [M][lda], or the conv input image [pixels][C]) -> an MX image in
//      the caller's scratch (GrlGemm.splitk_ws): one thread per (row, 32-k block) takes the block amax in registers and
//      writes 32 e4m3 bytes + the scale byte.  For a conv the image is quantised per (pixel, 32-channel block): with
//      C % 32 == 0 every 32-k block of the implicit-GEMM row (K ordered tap, channel) is one such block, or padding
//      (all zero), so this is the same quantisation as per (row, 32-k block) of the im2col matrix -- done once per
//      pixel instead of once per tap and per N tile.
//   2. mx_gemm_kernel: 128 x 128 tiles, 256 threads (2 x 2 waves of 64 x 64), 128 k per stage: both operands' e4m3
//      bytes and scale bytes staged global -> registers -> LDS (double buffer, one barrier per stage), four
//      32x32x64 MFMAs per wave and 64 k; fp32 accumulation, the bf16s affine epilogue, bf16 store.
//
// Why not quantise A inside the GEMM's staging: one (row, block) costs ~100 VALU instructions (amax, exponent, 32
// conversions) and is then used by only BN = 128 columns -- 8 e4m3 MFMAs of 64 cycles per wave per stage against
// ~600 VALU cycles of conversion: a 5-10x VALU-bound kernel.  The separate pass converts every element once.
//
// Numerics (the contract of include/grl_hip.h; tests/mx_ref.py is its model): the conversion below is integer-only, so
// it does not depend on the fp32 denormal mode, and the host build of the same function is what the CPU tests pin.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/grl_hip.h"
#include "common.h"

#ifndef GRL_MX_QIN
#define GRL_MX_QIN 0
#endif

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int MX_BM = 128, MX_BN = 128, MX_BK = 128;     // tile rows, tile columns, k per stage (4 blocks)
constexpr int MX_LDS_ROW = MX_BK + 16;                   // LDS row pitch of an operand tile (bytes)

__host__ __device__ inline int mx_scale_pad(int kb) { return (kb + 3) & ~3; }

// e of the contract from the largest |x| bits of a block (NaNs excluded): floor(log2 amax) - 8, clamped to
// [-127, 127]; zero and fp32-subnormal maxima give -127, +inf counts as 2^128
__host__ __device__ inline int mx_block_exp(uint32_t amax_bits) {
    if (amax_bits < 0x00800000u) return -127;
    const int e = (int)(amax_bits >> 23) - 127 - 8;
    return e < -127 ? -127 : (e > 127 ? 127 : e);
}

// e4m3fn code of x * 2^-e: round to nearest even, saturated to +-448, NaN -> 0x7F (sign kept), integer arithmetic only
__host__ __device__ inline uint32_t mx_e4m3(uint32_t xb, int e) {
    const uint32_t s = (xb >> 24) & 0x80u;
    const uint32_t a = xb & 0x7fffffffu;
    const bool norm = a >= 0x00800000u;
    const uint32_t m = norm ? ((a & 0x7fffffu) | 0x800000u) : a;            // x = m * 2^(ex)
    const int ex = norm ? (int)(a >> 23) - 150 : -149;
    const int lg = norm ? ex + 23 : (a ? 31 - __builtin_clz(a | 1u) : -64) + ex;   // floor(log2 |x|)
    const int ef = lg - e;                                                   // floor(log2 |f|)
    const int qe = (ef < -6 ? -6 : ef) - 3;                                  // quantum of f's e4m3 binade
    const int sh = qe - (ex - e);                                            // q = RNE(m >> sh); sh >= 13 here
    const uint32_t q = sh > 25 ? 0u : (m + (1u << (sh - 1)) - 1u + ((m >> sh) & 1u)) >> sh;
    int code = ef < -6 ? (int)q : ((ef + 7) << 3) + (int)q - 8;              // q == 16 carries into the exponent
    code = (ef > 8 || code > 0x7E) ? 0x7E : code;
    code = a == 0 ? 0 : code;
    return s | (a > 0x7f800000u ? 0x7Fu : (a == 0x7f800000u ? 0x7Eu : (uint32_t)code));
}

// one block of 32 fp32 bit patterns -> 8 words of e4m3 codes (element i in byte i % 4 of word i / 4); returns e
__device__ inline int mx_quant_block(const uint32_t (&xb)[32], uint32_t (&w)[8]) {
    uint32_t amax = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const uint32_t a = xb[i] & 0x7fffffffu;
        amax = (a <= 0x7f800000u && a > amax) ? a : amax;
    }
    const int e = mx_block_exp(amax);
#pragma unroll
    for (int i = 0; i < 8; ++i)
        w[i] = mx_e4m3(xb[4 * i], e) | (mx_e4m3(xb[4 * i + 1], e) << 8) | (mx_e4m3(xb[4 * i + 2], e) << 16) |
               (mx_e4m3(xb[4 * i + 3], e) << 24);
    return e;
}

// bf16 pairs (element 2j in the low half of word j) -> fp32 bit patterns
__device__ inline void bf16_bits(const uint4 (&v)[4], uint32_t (&xb)[32]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t u[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
        for (int k = 0; k < 4; ++k) { xb[8 * i + 2 * k] = u[k] << 16; xb[8 * i + 2 * k + 1] = u[k] & 0xffff0000u; }
    }
}

// One thread per (row, 32-k block) of x [rows][ld] -> elements q [rows][K] (row pitch K) and scale bytes
// sc [rows][mx_scale_pad(K/32)]; the padding scale bytes are written 0.  The block is read as raw bits in 16-byte
// loads (rows 16-byte aligned: ld % 8 == 0 for bf16, % 4 for fp32): no floating-point operation touches it, so fp32 /
// bf16 subnormals reach the integer rules as they are, whatever the denormal mode.
template <typename T>
__global__ __launch_bounds__(256) void mx_quant_kernel(const T* __restrict__ x, int64_t rows, int K, int ld,
                                                       uint8_t* __restrict__ q, uint8_t* __restrict__ sc) {
    const int KB = K / 32, SK = mx_scale_pad(KB);
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= rows * SK) return;
    const int64_t r = u / SK;
    const int kb = (int)(u - r * SK);
    if (kb >= KB) { sc[u] = 0; return; }
    constexpr int NV = 32 * (int)sizeof(T) / 16;                  // 16-byte loads per block
    const uint4* src = reinterpret_cast<const uint4*>(x + r * ld + kb * 32);
    uint32_t raw[4 * NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const uint4 v = src[i];
        raw[4 * i] = v.x; raw[4 * i + 1] = v.y; raw[4 * i + 2] = v.z; raw[4 * i + 3] = v.w;
    }
    uint32_t xb[32];
#pragma unroll
    for (int i = 0; i < 32; ++i)
        xb[i] = sizeof(T) == 4 ? raw[i] : ((i & 1) ? raw[i >> 1] & 0xffff0000u : raw[i >> 1] << 16);
    uint32_t w[8];
    const int e = mx_quant_block(xb, w);
    uint4* dst = reinterpret_cast<uint4*>(q + r * K + kb * 32);
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
    sc[u] = (uint8_t)(e + 127);
}

template <typename T>
int launch_quant(const T* x, int64_t rows, int K, int ld, uint8_t* out, hipStream_t s) {
    const int64_t units = rows * mx_scale_pad(K / 32);
    hipLaunchKernelGGL(mx_quant_kernel<T>, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, x, rows, K, ld, out,
                       out + rows * K);
    return grl_check_launch("mx_quant");
}

struct MxArgs {
    const uint8_t* aq;      // A elements: dense [M][K]; conv: the image [pixels][C]
    const uint8_t* as;      // A scales:   dense [M][SKA]; conv [pixels][SKA]   (SKA = scale_pad(K/32) or scale_pad(C/32))
    const uint8_t* wq;      // W elements [N][K]
    const uint8_t* ws;      // W scales [N][scale_pad(K/32)]
    __bf16* y;
    const float* scale;
    const float* shift;
    const __bf16* res;
    const float* gbias;
    const float* rowscale;
    int M, N, K, ska, skw, ldy, ldres, rpg, relu;
    int conv, H, W, C, Ho, Wo, kw, stride, pad;
    float inv_c, inv_kw;    // 1/C, 1/kw (exact integer quotients for the ranges used: see fdiv)
    int tiles_n;
    const uint16_t* a16;    // QIN: the bf16 activations themselves (dense [M][lda], conv [pixels][C])
    int lda;
};

// floor(k / d) for 0 <= k < 2^20, 1 <= d <= 4096 from a float reciprocal: (k + 0.5) / d is at least 0.5 / d away
// from an integer, far more than the float error of the product
__device__ inline int fdiv(int k, float inv) { return (int)(((float)k + 0.5f) * inv); }

// Operand fragment of one 64-k step of v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3), as measured on gfx950 with exact
// integer data: lane l (r = l % 32, h = l / 32) holds row r, bytes 0-15 = k 16h ... 16h + 15 and bytes 16-31 =
// k 32 + 16h ... 32 + 16h + 15 (the same map for A rows and B columns); its scale operand is the E8M0 byte of row r,
// block h (k 32h ... 32h + 31), picked by opsel (0 here).  So a lane's two pieces lie in different blocks and its scale
// is not that of its own bytes: a per-lane "32 contiguous k" map gives right answers with unit scales only.
// The C/D map is the bf16 one (col = l % 32, row = (i & 3) + 8 (i >> 2) + 4h).
__device__ inline i32x8 ld_frag(const uint8_t* step_row, int h) {
    const uint4 p0 = *reinterpret_cast<const uint4*>(step_row + 16 * h);
    const uint4 p1 = *reinterpret_cast<const uint4*>(step_row + 32 + 16 * h);
    return i32x8{(int)p0.x, (int)p0.y, (int)p0.z, (int)p0.w, (int)p1.x, (int)p1.y, (int)p1.z, (int)p1.w};
}

// QIN = false: A arrives quantised (the pass above); QIN = true: A is read as bf16 and quantised per (row, block) while it
// is staged, between the wait for the stage's loads and its LDS store (GRL_MX_QUANT_IN_STAGING=1; measured slower:
// EXPERIMENTS.md, 'MX-FP8 eval datapath').
template <bool QIN>
__global__ __launch_bounds__(256, 2) void mx_gemm_kernel(const MxArgs p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    constexpr int OPB = MX_BM * MX_LDS_ROW;                       // one operand tile
    constexpr int SCB = MX_BM * 4;                                // one operand's scale bytes (4 blocks per row)
    constexpr int BUF = 2 * OPB + 2 * SCB;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tm = blockIdx.x / p.tiles_n, tn = blockIdx.x - tm * p.tiles_n;
    const int m0 = tm * MX_BM, n0 = tn * MX_BN;

    // staging role: thread t stages row t / 2 of both operand tiles, k bytes 64 * (t & 1) ... + 63 (blocks 2(t&1), +1)
    const int sr = t >> 1, sh2 = t & 1;
    const int am = m0 + sr, wn = n0 + sr;
    const bool a_ok = am < p.M, w_ok = wn < p.N;
    const uint8_t* wrow = p.wq + (int64_t)(w_ok ? wn : 0) * p.K;
    const uint8_t* wsrow = p.ws + (int64_t)(w_ok ? wn : 0) * p.skw;
    // conv geometry of this thread's A row
    int img = 0, oy = 0, ox = 0;
    if (p.conv) {
        const int hw = p.Ho * p.Wo;
        const int mm = a_ok ? am : 0;
        img = mm / hw;
        const int rem = mm - img * hw;
        oy = rem / p.Wo;
        ox = rem - oy * p.Wo;
    }

    uint4 ra[4], rw[4];
    uint4 rb[QIN ? 8 : 1];                                        // QIN: the two blocks' raw bf16
    uint32_t rsa[2], rsw[2];
    auto load_stage = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = k0 + 64 * sh2 + 32 * j;                 // first k of the block
            const bool kin = k < p.K;
            const int kc = kin ? k : 0;
            // W block
            const uint4* wsrc = reinterpret_cast<const uint4*>(wrow + kc);
            const uint4 w0 = wsrc[0], w1 = wsrc[1];
            const uint32_t wsb = wsrow[kc >> 5];
            const bool wv = w_ok && kin;
            rw[2 * j] = wv ? w0 : make_uint4(0, 0, 0, 0);
            rw[2 * j + 1] = wv ? w1 : make_uint4(0, 0, 0, 0);
            rsw[j] = wv ? wsb : 0u;
            // A block: dense row, or the pixel of this k's tap
            int64_t aoff, soff;
            bool av = a_ok && kin;
            if (p.conv) {
                const int tap = fdiv(kc, p.inv_c);
                const int c = kc - tap * p.C;
                const int ty = fdiv(tap, p.inv_kw), tx = tap - ty * p.kw;
                const int iy = oy * p.stride - p.pad + ty, ix = ox * p.stride - p.pad + tx;
                av = av && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
                const int64_t pix = av ? ((int64_t)img * p.H + iy) * p.W + ix : 0;
                aoff = pix * p.C + (av ? c : 0);
                soff = pix * p.ska + (av ? c >> 5 : 0);
            } else {
                aoff = (int64_t)(a_ok ? am : 0) * p.K + kc;
                soff = (int64_t)(a_ok ? am : 0) * p.ska + (kc >> 5);
            }
            if constexpr (QIN) {
                const int64_t boff = p.conv ? aoff : (int64_t)(a_ok ? am : 0) * p.lda + kc;
                const uint4* bsrc = reinterpret_cast<const uint4*>(p.a16 + boff);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint4 v = bsrc[i];
                    rb[4 * j + i] = av ? v : make_uint4(0, 0, 0, 0);
                }
                (void)soff;
            } else {
                const uint4* asrc = reinterpret_cast<const uint4*>(p.aq + aoff);
                const uint4 a0 = asrc[0], a1 = asrc[1];
                const uint32_t asb = p.as[soff];
                ra[2 * j] = av ? a0 : make_uint4(0, 0, 0, 0);
                ra[2 * j + 1] = av ? a1 : make_uint4(0, 0, 0, 0);
                rsa[j] = av ? asb : 0u;
            }
        }
    };
    auto store_stage = [&](int buf) {
        if constexpr (QIN) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const uint4 v[4] = {rb[4 * j], rb[4 * j + 1], rb[4 * j + 2], rb[4 * j + 3]};
                uint32_t xb[32], w[8];
                bf16_bits(v, xb);
                rsa[j] = (uint32_t)(mx_quant_block(xb, w) + 127);
                ra[2 * j] = make_uint4(w[0], w[1], w[2], w[3]);
                ra[2 * j + 1] = make_uint4(w[4], w[5], w[6], w[7]);
            }
        }
        uint8_t* base = lds + buf * BUF;
        uint4* da = reinterpret_cast<uint4*>(base + sr * MX_LDS_ROW + 64 * sh2);
        uint4* dw = reinterpret_cast<uint4*>(base + OPB + sr * MX_LDS_ROW + 64 * sh2);
#pragma unroll
        for (int i = 0; i < 4; ++i) { da[i] = ra[i]; dw[i] = rw[i]; }
        uint16_t* sa = reinterpret_cast<uint16_t*>(base + 2 * OPB + sr * 4 + 2 * sh2);
        uint16_t* sw = reinterpret_cast<uint16_t*>(base + 2 * OPB + SCB + sr * 4 + 2 * sh2);
        *sa = (uint16_t)(rsa[0] | (rsa[1] << 8));
        *sw = (uint16_t)(rsw[0] | (rsw[1] << 8));
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{};

    const int wm = wave >> 1, wnn = wave & 1;
    const int fr = lane & 31, fh = lane >> 5;
    const int nst = (p.K + MX_BK - 1) / MX_BK;
    load_stage(0);
    for (int st = 0; st < nst; ++st) {
        const int buf = st & 1;
        store_stage(buf);
        __syncthreads();
        const int nx = st + 1 < nst ? st + 1 : st;                // (the last iteration re-loads its own stage: no branch)
        load_stage(nx * MX_BK);
        const uint8_t* base = lds + buf * BUF;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int kb = 2 * ks + fh;                           // the block of this lane's scale operand
            i32x8 af[2], bf[2];
            int sa[2], sb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int ar = wm * 64 + i * 32 + fr, br = wnn * 64 + i * 32 + fr;
                af[i] = ld_frag(base + ar * MX_LDS_ROW + 64 * ks, fh);
                bf[i] = ld_frag(base + OPB + br * MX_LDS_ROW + 64 * ks, fh);
                sa[i] = base[2 * OPB + ar * 4 + kb];
                sb[i] = base[2 * OPB + SCB + br * 4 + kb];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[i], bf[j], acc[i][j], 0, 0, 0, sa[i], 0,
                                                                                  sb[j]);
        }
    }

    // epilogue (the bf16s one): v = acc * rs + gbias; v = v * scale + shift (+ res); ReLU that keeps NaN (a compare
    // and select: fmaxf(NaN, 0) is 0) and maps -0 to +0
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wnn * 64 + j * 32 + fr;
        if (n >= p.N) continue;
        const float sc = p.scale ? p.scale[n] : 1.f, sf = p.shift ? p.shift[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
                if (m >= p.M) continue;
                float v = acc[i][j][r];
                if (p.rowscale) v = v * p.rowscale[m];
                if (p.gbias) v = v + p.gbias[(int64_t)(m / p.rpg) * p.N + n];
                v = v * sc + sf;
                if (p.res) v = v + (float)p.res[(int64_t)m * p.ldres + n];
                v = (p.relu && !(v > 0.f) && v == v) ? 0.f : v;
                p.y[(int64_t)m * p.ldy + n] = (__bf16)v;
            }
        }
    }
}

int64_t act_rows(const GrlGemm& d) { return d.conv ? (int64_t)(d.M / (d.Ho * d.Wo)) * d.H * d.W : d.M; }
int act_k(const GrlGemm& d) { return d.conv ? d.C : d.K; }

int64_t ws_bytes(const GrlGemm& d) {
    const int64_t rows = act_rows(d);
    const int k = act_k(d);
    return rows * k + rows * mx_scale_pad(k / 32);
}

int unsupported(const char* what) { return grl_fail(GRL_EUNSUPPORTED, "gemm mxfp8: %s", what); }

int validate_mx(const GrlGemm& d) {
    if (d.epilogue == GRL_EPI_EUCLID || d.epilogue == GRL_EPI_NEGDOT) return unsupported("EUCLID / NEGDOT epilogues are not built");
    if (d.epilogue == GRL_EPI_SQDIFF) return unsupported("the SQDIFF epilogue is not built (grl_sqdiff_mean_bf16 is the route)");
    if (d.epilogue != GRL_EPI_AFFINE) return grl_fail(GRL_EINVAL, "gemm: unknown epilogue");
    if (d.stats) return unsupported("statistics are not built (eval-only datapath)");
    if (d.bn_z) return unsupported("bn_z is not built (eval-only datapath)");
    if (d.kblock) return unsupported("kblock is an fp32 datapath option");
    if (d.out_f32) return unsupported("out_f32 is not built (bf16 output only)");
    if (d.K <= 0 || d.K % 32) return unsupported("K must be a positive multiple of 32");
    if (d.conv && d.C % 32) return unsupported("conv needs C % 32 == 0 (a 32-k block inside one tap)");
    if (!d.a || !d.w || !d.y) return grl_fail(GRL_EINVAL, "gemm mxfp8: null operand");
    if (d.M <= 0 || d.N <= 0) return grl_fail(GRL_EINVAL, "gemm mxfp8: empty shape");
    if (d.gbias && d.rows_per_group <= 0) return grl_fail(GRL_EINVAL, "gemm mxfp8: rows_per_group");
    if (d.conv) {
        if (d.K != d.kh * d.kw * d.C || d.Ho <= 0 || d.Wo <= 0 || d.M % (d.Ho * d.Wo) || d.stride <= 0 || d.kw > 4096)
            return grl_fail(GRL_EINVAL, "gemm mxfp8: conv geometry (K == kh*kw*C, M == nimg*Ho*Wo)");
        if (d.K >= (1 << 20)) return grl_fail(GRL_EINVAL, "gemm mxfp8: conv K >= 2^20");
    } else if (d.lda < d.K || d.lda % 8) {
        return grl_fail(GRL_EINVAL, "gemm mxfp8: dense A needs lda >= K, lda %% 8 == 0, a 16-byte aligned");
    }
    if (((uintptr_t)d.w & 15) || ((uintptr_t)d.a & 15))
        return grl_fail(GRL_EINVAL, "gemm mxfp8: a and the MX weight image must be 16-byte aligned");
    if (d.ldy < d.N || (d.res && d.ldres < d.N)) return grl_fail(GRL_EINVAL, "gemm mxfp8: ldy / ldres < N");
    if (!d.splitk_ws || d.splitk_ws_floats * 4 < ws_bytes(d) || ((uintptr_t)d.splitk_ws & 15))
        return grl_fail(GRL_EINVAL, "gemm mxfp8: splitk_ws must hold grl_conv_gemm_f32_workspace_floats() floats, 16-byte aligned");
    return GRL_OK;
}

}  // namespace

int64_t grl_gemm_mxfp8_workspace_floats(const GrlGemm& d) {
    if (d.K <= 0 || d.K % 32 || (d.conv && (d.C % 32 || d.Ho <= 0 || d.Wo <= 0))) return 0;
    return (ws_bytes(d) + 3) / 4;
}

int grl_gemm_mxfp8(const GrlGemm& d, hipStream_t s) {
    if (int e = validate_mx(d)) return e;
    uint8_t* ws = reinterpret_cast<uint8_t*>(d.splitk_ws);
    const int64_t rows = act_rows(d);
    const int ak = act_k(d);
    const __bf16* a = reinterpret_cast<const __bf16*>(d.a);
    // measurement only (a library built with -DGRL_MX_QIN=1, run with GRL_MX_QUANT_IN_STAGING=1): quantise A inside the
    // GEMM's staging instead of the pass (same bytes, same result).  Not in the default build: at 256 VGPRs that kernel
    // spills inside its k loop (tools/isa_lint.py) and was measured slower (EXPERIMENTS.md, 'MX-FP8 eval datapath')
#if GRL_MX_QIN
    static const bool qin = [] { const char* e = getenv("GRL_MX_QUANT_IN_STAGING"); return e && atoi(e) != 0; }();
#else
    constexpr bool qin = false;
#endif
    if (!qin)
        if (int e = launch_quant<__bf16>(a, rows, ak, d.conv ? d.C : d.lda, ws, s)) return e;
    MxArgs p;
    p.a16 = reinterpret_cast<const uint16_t*>(d.a);
    p.lda = d.lda;
    p.aq = ws;
    p.as = ws + rows * ak;
    p.ska = mx_scale_pad(ak / 32);
    p.wq = reinterpret_cast<const uint8_t*>(d.w);
    p.ws = p.wq + (int64_t)d.N * d.K;
    p.skw = mx_scale_pad(d.K / 32);
    p.y = reinterpret_cast<__bf16*>(d.y);
    p.scale = d.scale;
    p.shift = d.shift;
    p.res = reinterpret_cast<const __bf16*>(d.res);
    p.gbias = d.gbias;
    p.rowscale = d.rowscale;
    p.M = d.M; p.N = d.N; p.K = d.K; p.ldy = d.ldy; p.ldres = d.ldres; p.rpg = d.rows_per_group; p.relu = d.relu;
    p.conv = d.conv; p.H = d.H; p.W = d.W; p.C = d.C; p.Ho = d.Ho; p.Wo = d.Wo; p.kw = d.kw; p.stride = d.stride; p.pad = d.pad;
    p.inv_c = d.conv ? 1.f / (float)d.C : 0.f;
    p.inv_kw = d.conv ? 1.f / (float)d.kw : 0.f;
    const int tiles_m = (d.M + MX_BM - 1) / MX_BM;
    p.tiles_n = (d.N + MX_BN - 1) / MX_BN;
    constexpr size_t lds = 2 * (2 * MX_BM * MX_LDS_ROW + 2 * MX_BM * 4);
    static const bool attr = [] {
        (void)hipFuncSetAttribute((const void*)mx_gemm_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
#if GRL_MX_QIN
        (void)hipFuncSetAttribute((const void*)mx_gemm_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
#endif
        return true;
    }();
    (void)attr;
#if GRL_MX_QIN
    if (qin) hipLaunchKernelGGL(mx_gemm_kernel<true>, dim3((unsigned)(tiles_m * p.tiles_n)), dim3(256), lds, s, p);
    else
#endif
    hipLaunchKernelGGL(mx_gemm_kernel<false>, dim3((unsigned)(tiles_m * p.tiles_n)), dim3(256), lds, s, p);
    return grl_check_launch("grl_conv_gemm_f32 (mxfp8)");
}

extern "C" int grl_mx_pack_weights(const float* w, int N, int K, int ldw, uint8_t* out, void* stream) {
    if (!w || !out || N <= 0 || K <= 0 || ldw < K) return grl_fail(GRL_EINVAL, "mx_pack_weights: null pointer or bad shape");
    if (K % 32) return grl_fail(GRL_EUNSUPPORTED, "mx_pack_weights: K must be a multiple of 32");
    if (((uintptr_t)out & 15) || ((uintptr_t)w & 15) || ldw % 4)
        return grl_fail(GRL_EINVAL, "mx_pack_weights: w, out 16-byte aligned, ldw %% 4 == 0");
    return launch_quant<float>(w, N, K, ldw, out, (hipStream_t)stream);
}

extern "C" int grl_mx_quantize_rows(const void* x, int M, int K, int ldx, uint8_t* out, void* stream) {
    if (!x || !out || M <= 0 || K <= 0 || ldx < K) return grl_fail(GRL_EINVAL, "mx_quantize_rows: null pointer or bad shape");
    if (K % 32) return grl_fail(GRL_EUNSUPPORTED, "mx_quantize_rows: K must be a multiple of 32");
    if (((uintptr_t)out & 15) || ((uintptr_t)x & 15) || ldx % 8)
        return grl_fail(GRL_EINVAL, "mx_quantize_rows: x, out 16-byte aligned, ldx %% 8 == 0");
    return launch_quant<__bf16>(reinterpret_cast<const __bf16*>(x), M, K, ldx, out, (hipStream_t)stream);
}

extern "C" int64_t grl_mx_image_bytes(int rows, int K) {
    if (rows <= 0 || K <= 0 || K % 32) return 0;
    return (int64_t)rows * K + (int64_t)rows * mx_scale_pad(K / 32);
}

// host build of the element / exponent rule (tests/test_mx_cpu.py pins it against tests/mx_ref.py without a GPU)
extern "C" int grl_mx_e4m3_host(int32_t xbits, int e) { return (int)mx_e4m3((uint32_t)xbits, e); }
extern "C" int grl_mx_block_exp_host(int32_t amax_bits) { return mx_block_exp((uint32_t)amax_bits); }
