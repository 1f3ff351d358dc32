/*
 * grl_hip.h -- C ABI of libgrl_hip.so: the MI355X (gfx950) kernels behind the
 * GRL per-clip forward/backward path and the evaluator distance matrix.
 *
 * The reference (flysnowtiger/GRL) has no FFI layer: every op on this path is a
 * stock PyTorch op called from Python.  Each entry point below names the
 * reference call site(s) it replaces (paths relative to /root/reference).
 * The Python host (grl_amd/engine.py) binds these with ctypes; see
 * INTEGRATION.md for the binding a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every buffer is caller-owned DEVICE memory
 *     (fp32, contiguous unless a leading dimension is given); the library never
 *     allocates and keeps no global state;
 *   - activations are channels-last: an activation of N images, HxW pixels and C
 *     channels is the row-major matrix [N*H*W][C];
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued, not waited;
 *   - return 0 on success, a negative GRL_E* code otherwise; grl_last_error()
 *     returns a thread-local message for the last failure.
 */
#ifndef GRL_HIP_H
#define GRL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GRL_OK          0
#define GRL_EINVAL     -1   /* bad shape / pointer / alignment */
#define GRL_ELAUNCH    -2   /* hipLaunch failed; message has the HIP error string */

const char* grl_last_error(void);
/* Bumped on every incompatible change of a struct layout or an argument list below; grl_amd/_lib.py refuses a
 * library whose version differs from the one it was written against (round 1: 1, round 2: 2 -- GrlGemm / GrlWgrad
 * grew, grl_bn_bwd gained two pointers -- round 3: 3, then 4 with grl_stem_wgrad, relu_bits, 5: GrlGemm.bn_*;
 * round 4: 6 with grl_bottleneck_tail_bf16, 7 grl_gemm_force_tile; round 5: 8 with grl_conv_gemm_f32_group;
 * round 6: 9 with the grl_jpeg_* entry points; 10: GRL_MATH_MXFP8 and the grl_mx_* entry points, additive only).
 * The column-block search / ranking entry points grl_topk_block .. grl_rank_finish were added at 10: they change no
 * struct layout or argument list, and a library without them fails to bind in _lib.load.  So were the streaming
 * re-ranking entry points grl_rrs_*, the CSR / CSC assembly of its sharded form (grl_rrs_expand_rows, grl_rrs_scan,
 * grl_rrs_place, grl_rrs_transpose) among them, grl_topk_block_filtered, grl_expand_rows, the grl_verify_* entry points,
 * grl_pair_hist_block, the clustering entry points grl_cluster_*, the k-means entry points grl_kmeans_* /
 * grl_segment_rowsum, grl_jaccard_edges, the silhouette entry points grl_silhouette_*, the HDBSCAN entry points
 * grl_hdbscan_*, the t-SNE entry points grl_tsne_*, the PCA entry points grl_pca_*, the diffusion entry points
 * grl_diffusion_*, grl_setdist_block and the product-quantisation entry points grl_pq_*. */
#define GRL_ABI_VERSION 10
int grl_abi_version(void);
/* `waiter` (a hipStream_t) waits for everything enqueued on `signaler` so far: hipEventRecord + hipStreamWaitEvent on a
 * pooled event, one call instead of the host framework's Event / stream-context objects (round 6: the train step is
 * host-bound in bf16 storage; this is the side-stream hand-off of the weight-gradient launches).  Not a reference op. */
int grl_stream_wait_stream(void* waiter, void* signaler);

/* epilogue selector of grl_conv_gemm_f32 */
#define GRL_EPI_AFFINE  0   /* y = relu?( rs[m]*(acc + gbias[m/rpg][n])*scale[n] + shift[n] + res[m][n] ) */
#define GRL_EPI_NEGDOT  1   /* y = -acc                                     (attevaluator.py:44-46)  */
#define GRL_EPI_EUCLID  2   /* y = sqrt(max(rnorm[m]+cnorm[n]-2acc,1e-12))  (attevaluator.py:33-41)  */
#define GRL_EPI_SQDIFF  3   /* TRL step (grl_model.py:146-149): v = relu(acc*scale + shift) is NOT stored;
                               y[m/32][n] = sum over the 32 rows of (v - res[row'][n])^2, row' = (m/res_rows)*
                               res_gstride + m%res_rows -- the conv_f1 output never reaches HBM.  fp32 storage,
                               128 x 128 tiles (M % 128 == 0), y is [M/32][ldy] fp32 partial sums            */

/* multiplier datapath of grl_conv_gemm_f32 (operands are fp32 in HBM in every mode) */
#define GRL_MATH_F32     0  /* exact fp32 MFMA: the documented fmaf chain (default)              */
#define GRL_MATH_BF16    1  /* operands rounded to bf16 while staging, bf16 MFMA (BASELINE cfg 2) */
#define GRL_MATH_BF16X3  3  /* split-bf16: hi*hi + hi*lo + lo*hi on the bf16 MFMA, ~2^-16 rel.   */
#define GRL_MATH_BF16S   2  /* bf16 STORAGE: a, w, res and y are bf16 arrays (lda/ldw/ldy/ldres in
                             * elements), fp32 accumulate + epilogue; `out_f32` keeps y fp32      */
#define GRL_MATH_MXFP8   4  /* MX-FP8 operands (eval only; see "MX-FP8 datapath" below): a, res, y bf16
                             * as in GRL_MATH_BF16S, w an MX weight image (grl_mx_pack_weights)  */

/*
 * MX-FP8 datapath (GRL_MATH_MXFP8, gemm_mxfp8.hip): the bf16-storage GEMM on the block-scaled MFMA
 * v_mfma_scale_f32_32x32x64_f8f6f4.  EXPERIMENTAL: correct to the contract below, but measured slower than
 * GRL_MATH_BF16S on every pipeline shape (EXPERIMENTS.md, 'MX-FP8 eval datapath').  Numerics contract (OCP MX v1.0; model: tests/mx_ref.py):
 *   - a block is 32 consecutive elements along K (of one row of A, one row of W);
 *   - shared exponent e = floor(log2(amax)) - 8 (8 = emax of e4m3), clamped to [-127, 127]; amax is the block's
 *     largest |x| with NaNs ignored and +inf counting as 2^128; the E8M0 scale byte is e + 127;
 *   - an all-zero block gets scale byte 0 and zero elements;
 *   - element = e4m3fn (OCP, not fnuz) of x * 2^-e, rounded to nearest even, saturated to +-448; a NaN element is
 *     0x7F (sign kept), and the MFMA turns it into NaN in every output of its row (A) or column (W);
 *   - W is quantised from the fp32 packed weight once per plan (grl_mx_pack_weights); A (bf16) is quantised per
 *     (row, 32-k block) by a pass in front of the GEMM into the caller's scratch.  Implicit-GEMM convs need
 *     C % 32 == 0: a block then lies inside one tap, so the pass quantises the input image per (pixel, 32-channel
 *     block) -- the same bytes as per (row, block) of the im2col matrix; padding taps are all-zero blocks;
 *   - fp32 accumulation; the GRL_MATH_BF16S affine epilogue in its order: v = acc * rowscale[m] + gbias, then
 *     v * scale + shift, + bf16 res, ReLU that keeps NaN; bf16 store.
 * Because the scales are per row and block, a clip's quantisation never depends on the other clips of its batch.
 *
 * MX image (weights from grl_mx_pack_weights, and the activation scratch): for R rows of K elements,
 *   bytes [0, R*K)                     e4m3 elements, row r at r*K (row pitch K, whatever the source's ld was);
 *   bytes [R*K, R*K + R*SK)            E8M0 scale bytes, row r at R*K + r*SK, SK = K/32 rounded up to a multiple of
 *                                      4 (the padding bytes are 0).
 * grl_mx_image_bytes(R, K) is its size.
 *
 * GrlGemm with math = GRL_MATH_MXFP8:
 *   - a: bf16 (dense [M][lda], lda % 8 == 0, or the conv image [nimg][H][W][C]); res, y: bf16 as in GRL_MATH_BF16S;
 *   - w: the MX image of the [N][K] weight (ldw is not read: the image is dense);
 *   - splitk_ws / splitk_ws_floats: REQUIRED scratch for A's MX image, at least grl_conv_gemm_f32_workspace_floats()
 *     floats, 16-byte aligned (GRL_EINVAL otherwise);
 *   - epilogue GRL_EPI_AFFINE, dense or conv; K % 32 == 0 (and C % 32 == 0 for a conv).
 *   GRL_EUNSUPPORTED (-3), before any launch: EUCLID / NEGDOT / SQDIFF epilogues, stats, bn_z, kblock, out_f32,
 *   K % 32 != 0, conv C % 32 != 0.
 */

/*
 * One fp32 MFMA GEMM  Y[M][N] = epilogue( A[M][K] . W[N][K]^T ), K-contiguous on
 * both operands.  With conv geometry set, A is gathered on the fly from a
 * channels-last image tensor (implicit GEMM): K = kh*kw*C, ordered tap-major then
 * channel, zero padding outside the image.
 *
 * Replaces: nn.Conv2d + eval-mode nn.BatchNorm2d + ReLU + residual add in
 *   reid/models/resnets1.py:76-91 (Bottleneck), reid/models/basebranch.py:42-50,61-62
 *   (GCE convs), reid/models/grl_model.py:71-83 (memo block), :146-147,160-161
 *   (f1/f2 biased convs); nn.Linear+BatchNorm1d in basebranch.py:38-40 and
 *   Siamese.py:84-94; torch.mm / addmm_ in reid/evaluator/attevaluator.py:33-46.
 *
 * Numerics: each output element is one fp32 accumulator updated by a k-ordered
 * chain of fused multiply-adds (v_mfma_f32_32x32x2_f32); the k order is documented
 * in DESIGN.md and reproduced bit-exactly by oracle/ref_c.
 */
typedef struct GrlGemm {
    const float* a;        /* dense: [M][lda]; conv: images [nimg][H][W][C]               */
    const float* w;        /* [N][ldw], K-contiguous (3x3 weights packed [N][tap][C])     */
    float*       y;        /* [M][ldy]                                                    */
    const float* scale;    /* [N] or NULL (=1)                                            */
    const float* shift;    /* [N] or NULL (=0)                                            */
    const float* res;      /* [M][ldres] residual or NULL                                 */
    const float* gbias;    /* [M/rows_per_group][N] added to acc before scale, or NULL    */
    const float* rowscale; /* [M] multiplies acc first, or NULL                           */
    const float* rnorm;    /* EUCLID: |a_m|^2 [M]                                         */
    const float* cnorm;    /* EUCLID: |w_n|^2 [N]                                         */
    float*       stats;    /* train mode: per-channel partial sums [gridM][2][N], or NULL */
    int32_t M, N, K;
    int32_t lda, ldw, ldy, ldres;
    int32_t rows_per_group;
    int32_t relu;
    int32_t epilogue;      /* GRL_EPI_*                                                   */
    /* conv geometry; conv == 0 means dense A */
    int32_t conv, H, W, C, Ho, Wo, kh, kw, stride, pad;
    int32_t math;          /* GRL_MATH_*: multiplier datapath (accumulation is always fp32)   */
    int32_t out_f32;       /* GRL_MATH_BF16S only: write y as fp32                            */
    int32_t res_rows, res_gstride;   /* GRL_EPI_SQDIFF: row mapping of `res` (rows per group, row stride between groups) */
    int32_t kblock;        /* GRL_MATH_F32 only: 1 = cut the accumulation chain every 512 k and sum the
                              segments (K-blocked accumulation: the accuracy class of a blocked CPU
                              sgemm; ~4 % slower on K >= 1024).  The train-mode forward sets it -- ReLU
                              masks, hence parameter gradients, agree with the reference's only as well
                              as the forward does; 0 = ONE k-ordered fmaf chain (eval path, evaluator). */
    /* Optional split-K scratch (round 3).  A skinny K-blocked GEMM (M <= 256, a handful of tiles: the per-clip
     * linears of GCE / TRL / the Siamese heads in train mode) walks K = 1024..2048 in ONE workgroup per tile --
     * latency-bound, ~60 us at 1 % MFMA busy.  With scratch the 512-k segments of the K-blocked chain run as
     * separate workgroups (grid.y = segments) writing raw partials [segment][M][N], and a second kernel adds them
     * in segment order and applies the epilogue: bit-identical to the one-workgroup K-blocked result.  NULL or
     * fewer floats than grl_conv_gemm_f32_workspace_floats() asks for: the one-workgroup form runs. */
    float*  splitk_ws;
    int64_t splitk_ws_floats;
    /* Optional BatchNorm-BACKWARD reduce in the epilogue (round 3; fp32 storage, AFFINE epilogue, 16-byte aligned
     * rows): when this GEMM produces the last contribution to the gradient of y = relu?(bn(z) (+res)) -- a data-
     * gradient GEMM whose output (+ `res`, the contributions so far) IS that gradient -- the epilogue masks it,
     * g = v * mask, writes g to `y` and leaves the two column sums of the BatchNorm backward in `stats`:
     * stats[tile][0][n] = sum_rows g, stats[tile][1][n] = sum_rows g * (z - mean) * invstd -- what
     * grl_bn_bwd's reduce pass computes, without re-reading the gradient (grl_bn_bwd_finish does the rest).
     * mask: bn_bits (the forward's recorded (y > 0) bytes, grl_bn_apply_centered) if given, else
     * ((z - mean) * bn_mscale + bn_mbeta > 0) if bn_mscale is given, else none.  bn_z NULL = off.
     * Round 5: GRL_MATH_BF16S too -- bn_z is then a bf16 [M][N] tensor, bn_bits one byte per EIGHT outputs, the sums are
     * taken from the fp32 value before it is rounded to bf16; needs M % 128 == 0 and N % 128 == 0 (or N == 64): the
     * reduce lives in the branch-free interior epilogue of the 128-row tile family (grl_bn_bwd_finish_bf16 does the rest). */
    const float*   bn_z;       /* [M][N] (row stride N) */
    const float*   bn_mean;    /* [N] */
    const float*   bn_invstd;  /* [N] */
    const float*   bn_mscale;  /* [N] or NULL */
    const float*   bn_mbeta;   /* [N] or NULL */
    const uint8_t* bn_bits;    /* [M * N / 4] (bf16 storage: [M * N / 8]) or NULL */
} GrlGemm;

int grl_conv_gemm_f32(const GrlGemm* desc, void* stream);
/* floats of split-K scratch the call above can use for this shape (0: it would not split) */
int64_t grl_conv_gemm_f32_workspace_floats(const GrlGemm* desc);
/* Kernel-tuning / test hook of the GRL_MATH_BF16S datapath: which launches take the 256 x 256
 * LDS-DMA tile (gemm_bf16.hip): -1 = automatic (enough tiles to fill the chip; the default),
 * 0 = never, 1 = whenever the shape is legal.  Returns the previous mode; results do not depend
 * on it (same MFMA, same k order).  Not thread-safe. */
int grl_gemm_bf16_tile_mode(int mode);
/* Kernel-tuning / test hook of the fp32-storage datapaths: force the workgroup tile of the following grl_conv_gemm_f32
 * calls to bm x bn (128x128, 128x64 or 64x64); (0, 0) returns to the per-shape rule.  Returns the previous setting as
 * (bm << 16) | bn (0 = automatic), GRL_EINVAL for any other pair.  Results never depend on the tile (one k-ordered
 * chain per output; the parity tests run every shape on every tile through this).  TEST HOOK: process-wide state,
 * not synchronised -- single-threaded callers only.  A forced tile is final: the statistics GEMMs' promotion to the
 * 128 x 128 tile (choose_tile) does not apply while one is set. */
int grl_gemm_force_tile(int bm, int bn);
/* rows of the stats slab the call above writes (= number of M tiles it will use) */
int grl_conv_gemm_f32_stat_rows(const GrlGemm* desc);
/* n (1..4) GEMMs in ONE launch where the kernels allow it (round 5): the same result, bit for bit, as n calls of
 * grl_conv_gemm_f32 in order -- which is also what runs when they do not (different shapes or flags, fp32 storage,
 * conv geometry, statistics ...).  Grouped today: GRL_MATH_BF16S dense GEMMs of one shape with the plain affine
 * epilogue (scale, shift, optional res, relu) that differ only in a, w, y, scale, shift, res.
 * Replaces: the conv1 / conv2 1x1 convolutions of the forward AND the backward memo block of one TRL step
 * (reid/models/grl_model.py:56-64 called at :155 and :167) -- two independent 8192-row GEMMs of the same shape that
 * each fill half a chip.  GRL_GEMM_GROUP=0: always n separate launches. */
int grl_conv_gemm_f32_group(const GrlGemm* descs, int n, void* stream);

/* fp32 weight w [N][ldw] (K used columns, K % 32 == 0) -> its MX image (out: grl_mx_image_bytes(N, K) bytes, 16-byte
 * aligned; see "MX-FP8 datapath").  Eval packing of GRL_MATH_MXFP8; replaces nothing in the reference. */
int grl_mx_pack_weights(const float* w, int N, int K, int ldw, uint8_t* out, void* stream);
/* TEST HOOK: bf16 x [M][ldx] -> its MX image, with the device code the GRL_MATH_MXFP8 GEMM quantises A with. */
int grl_mx_quantize_rows(const void* x, int M, int K, int ldx, uint8_t* out, void* stream);
/* bytes of the MX image of rows x K (0 when K is not a positive multiple of 32) */
int64_t grl_mx_image_bytes(int rows, int K);
/* TEST HOOKS (host code, no device): the quantiser's element rule -- e4m3fn code of x * 2^-e for the fp32 bit pattern
 * xbits -- and its exponent rule (e from the bits of a block's largest |x|, NaN excluded) */
int grl_mx_e4m3_host(int32_t xbits, int e);
int grl_mx_block_exp_host(int32_t amax_bits);

/* [N][C][kh][kw] (torch layout) -> [N][kh*kw][C]; replaces nothing in the
 * reference (layout packing for the implicit GEMM). */
int grl_pack_conv_weight(const float* w, float* out, int N, int C, int kh, int kw, void* stream);

/* eval-mode BatchNorm folding: scale = g/sqrt(var+eps), shift = b - mean*scale
 * (+ scale*bias when the producing layer has a bias).  nn.BatchNorm{1,2}d in eval
 * mode everywhere on the path (e.g. resnets1.py:77,81,85). Any of gamma/beta NULL
 * means 1/0; mean/var NULL means 0/1 (plain bias -> shift). */
int grl_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var,
                const float* bias, float eps, float* scale, float* shift, int C, void* stream);

/* Stem: 7x7 stride-2 pad-3 conv on NCHW input [n][3][H][W], y = relu?(conv*scale+shift) ->
 * channels-last [n][H/2][W/2][64]   (resnets1.py:101-103 / basebranch.py:28-30).
 * Every launcher of the stem / max-pool family (the stems, grl_stem_pool_*, grl_maxpool3x3s2*, grl_bn_relu_maxpool3x3s2*,
 * grl_stem_im2col*) returns GRL_EINVAL before anything is launched for n <= 0, H <= 0 or W <= 0. */
int grl_stem_conv7x7(const float* x, const float* w /*[64][3][7][7]*/, const float* scale,
                     const float* shift, float* y, int n, int H, int W, int relu,
                     const float* wp /* optional: [64][164] image from grl_stem_pack_weight */,
                     void* stream);
/* the same stem reading RAW u8 pixels [n][3][H][W] and normalising them while the input patch
 * is staged in LDS: (u/255 - mean[c]) / std[c] with mean_std = {mean[3], std[3]} -- the fp32
 * operations of ToTensor + Normalize (reid/data/seqtransforms.py:190,195-216; constants
 * reid/data/dataloader.py:20), so the result is bit-identical to normalising on the host first.
 * a quarter of the input bytes over PCIe and HBM. */
int grl_stem_conv7x7_u8(const uint8_t* x, const float* mean_std, const float* w, const float* scale,
                        const float* shift, float* y, int n, int H, int W, int relu, const float* wp,
                        void* stream);
/* the normalisation alone (train mode keeps a float clip for the stem's weight gradient):
 * y[n][3][plane] = (x/255 - mean[c]) / std[c] */
int grl_normalize_u8(const uint8_t* x, const float* mean_std, float* y, int n, int64_t plane, void* stream);
/* Training input pipeline on the device (replaces the per-frame PIL transforms of
 * reid/data/seqtransforms.py:92-190 as composed in reid/data/dataloader.py:51-57): RandomHorizontalFlip
 * (per clip) + RandomSizedEarser (per frame: a constant-colour w x h patch pasted at (left, top) of the
 * flipped frame) + ToTensor + Normalize, raw uint8 clips [n_clips][T][3][H][W] -> float32.
 * params: int32 [n_clips][1 + 8*T] = {flip, T x {erase, left, top, w, h, R, G, B}}, the reference's
 * random draws made on the host (grl_amd/reid/data/augment.py).  W % 4 == 0. */
int grl_augment_normalize_u8(const uint8_t* x, const int32_t* params, const float* mean_std, float* y,
                             int n_clips, int T, int H, int W, void* stream);
/* RectScale (reid/data/seqtransforms.py:30-47: `frame.resize((W, H), Image.BILINEAR)`) on uint8 planes
 * [planes][Hin][Win] -> [planes][Hout][Wout], bit-identical to Pillow: horizontal pass, rounding to
 * uint8, vertical pass, 22-bit fixed-point taps.  bounds_*: int32 [out][2] = (first input index, taps);
 * coefs_*: int32 [out][k*]; both from grl_amd/reid/data/augment.py:pil_bilinear_coeffs. */
int grl_resize_bilinear_u8(const uint8_t* x, uint8_t* y, const int32_t* bounds_h, const int32_t* coefs_h, int kh,
                           const int32_t* bounds_v, const int32_t* coefs_v, int kv, int64_t planes, int Hin,
                           int Win, int Hout, int Wout, void* stream);
/* the stem's LDS weight image (K padded 147 -> 160, rows padded to 164 floats), made once per
 * weight version so that every workgroup copies it with 16-byte loads */
int grl_stem_pack_weight(const float* w, float* wp /* 64*164 floats */, void* stream);

/* 3x3 stride-2 pad-1 max pool, channels-last (resnets1.py:104). */
int grl_maxpool3x3s2(const float* x, float* y, int n, int H, int W, int C, void* stream);

/* Stem + max-pool in ONE launch, exact fp32 (round 5; eval: resnets1.py:101-104, basebranch.py:27-36): NCHW input
 * [n][3][H][128] (fp32, or raw u8 with mean_std as in grl_stem_conv7x7_u8) -> y = maxpool3x3s2(relu(conv7x7s2 * scale +
 * shift)) channels-last [n][H/4][32][64]; the stem map is neither written nor re-read.  W must be 128, H % 4 == 0.
 * wq: the register image of the weights from grl_stem_pack_weight_pool (64 * 168 floats).  Same products as
 * grl_stem_conv7x7 in another fp32 summation order (k-steps pair kx with kx + 4). */
int grl_stem_pack_weight_pool(const float* w /*[64][3][7][7]*/, float* wq /* 64*168 floats */, void* stream);
int grl_stem_pool_f32(const void* x, int x_is_u8, const float* mean_std, const float* scale, const float* shift, float* y,
                      int n, int H, int W, const float* wq, void* stream);

/* mean over `rows` consecutive rows: x [groups][rows][C] -> y [groups][ldy>=C]
 * (x.mean(-1).mean(-1)[.mean(1)] in basebranch.py:58, grl_model.py:151,165,178). */
int grl_group_mean(const float* x, float* y, int groups, int rows, int C, int ldy,
                   float out_scale, int accumulate, void* stream);

/* GCE tail (basebranch.py:49-50,62-66): map = sigmoid(bn(h[m].w3)); x_corr = x*map,
 * x_uncorr = x*(1-map).  h [M][256], x [M][C]. */
int grl_gce_gate(const float* h, const float* w3, const float* bn_scale, const float* bn_shift,
                 const float* x, float* corr_map, float* x_corr, float* x_uncorr,
                 int M, int Ch, int C, void* stream);

/* mean over T of x [b][T][rows*C] -> [b][rows*C]  (grl_model.py:137-138). */
int grl_temporal_mean(const float* x, float* y, int b, int T, int64_t inner, void* stream);

/* d[b][c] = mean_px (f1[b][px][c] - f2[b*f2_bstride + px][c])^2  (grl_model.py:149,163) */
int grl_sqdiff_mean(const float* f1, const float* f2, float* d, int b, int rows, int C,
                    int64_t f2_clip_stride, void* stream);

/* channel attention MLP: c = sigmoid(W2 relu(W1 d))  (grl_model.py:103-108,149,163);
 * then f_step[b][c] (+)= (1 + c) * gap[b][c]   (grl_model.py:150-151,164-165). */
int grl_channel_atte(const float* d, const float* w1 /*[Hd][C]*/, const float* w2t /*[Hd][C] = W2^T*/,
                     const float* gap, int64_t gap_stride, float* catte, float* fstep,
                     int64_t fstep_stride, int accumulate, int b, int C, int Hd,
                     float* hid_ws /* workspace [b][Hd] */, void* stream);

/* y = a + b elementwise (grl_model.py:68, memo + x_uncorr_t); b rows strided per clip */
int grl_add_strided(const float* a, const float* b, float* y, int nb, int64_t inner,
                    int64_t b_clip_stride, void* stream);

/* y[row] = l2normalize(x[row]*scale + shift)   (corr_bn/uncorr_bn + F.normalize,
 * grl_model.py:222-226); out rows strided so they can land inside a feature row. */
int grl_affine_l2norm(const float* x, const float* scale, const float* shift, float* y,
                      int rows, int C, int64_t ldy, void* stream);

/* Siamese.self_attention tail (Siamese.py:87-104): qk [b*T][2*D] (folded-BN Q|K),
 * x [b][T][C] -> pooled [b][ldy].  T <= 16. */
int grl_siamese_attn(const float* qk, const float* x, float* pooled, int b, int T, int D, int C,
                     int64_t ldy, void* stream);

/* y[b][c] = mean_T x[b][T][c] into a strided destination (attevaluator.py:112). */
int grl_mean_T(const float* x, float* y, int b, int T, int C, int64_t ldy, void* stream);

/* Pair verification head, eval mode (Siamese.py:127-140, Siamese_video.py:169-182):
 * out[i][j][c] = bias[c] + sum_k W[c][k]*(scale[k]*(p[i][k]-g[j][k])^2 + shift[k]). */
int grl_pair_verify(const float* p, const float* g, const float* scale, const float* shift,
                    const float* w, const float* bias, float* out, int np, int ng, int K,
                    int ncls, void* stream);

/* Row-wise ascending argsort of a distance matrix d [rows][ld] (first n columns), int32
 * indices out [rows][n]; ties go to the smaller index.  Replaces np.argsort(distmat, axis=1)
 * in reid/evaluator/eva_functions.py:139.  n <= 16384. */
int grl_row_argsort(const float* d, int64_t ld, int rows, int n, int32_t* idx, void* stream);
/* the same ranking for rows wider than one LDS network (16384 < n <= 2^24): the bitonic network cut at
 * the LDS size -- 16384-entry chunks sorted in LDS, the long-distance steps as global passes over
 * (key, index) pairs kept in `workspace` (grl_row_argsort_workspace_bytes(rows, n) bytes).  Same total
 * order (distance, then index) = np.argsort(kind='stable') of eva_functions.py:139. */
int64_t grl_row_argsort_workspace_bytes(int rows, int n);
int grl_row_argsort_wide(const float* d, int64_t ld, int rows, int n, int32_t* idx, void* workspace,
                         void* stream);

/* |x_row|^2 for the Euclidean epilogue (attevaluator.py:37-38). */
int grl_row_sqnorm(const float* x, float* out, int rows, int K, int ld, void* stream);

/* ------------------------------------------------------------------------------------
 * bf16-STORAGE pipeline (BASELINE configs[2]; engine math mode 'bf16s', GRL_MATH_BF16S):
 * bf16 twins of the bandwidth-bound kernels above -- activations are bf16 arrays (void*),
 * per-channel / per-clip vectors and all reductions stay fp32.  Same reference call sites.
 * ---------------------------------------------------------------------------------- */
int grl_cast_bf16(const float* x, void* y, int64_t n, void* stream);            /* n % 8 == 0 */
int grl_stem_conv7x7_bf16(const float* x, const float* w, const float* scale, const float* shift,
                          void* y, int n, int H, int W, int relu,
                          const void* wp /* optional: image from grl_stem_pack_weight_bf16 */, void* stream);
int grl_stem_conv7x7_u8_bf16(const uint8_t* x, const float* mean_std, const float* w, const float* scale,
                             const float* shift, void* y, int n, int H, int W, int relu, const void* wp,
                             void* stream);                                      /* u8 input, as grl_stem_conv7x7_u8 */
int grl_stem_pack_weight_bf16(const float* w, void* wp /* 64*184 bf16: rows of 368 bytes, k ordered (channel, ky, kx padded to 8) + zero pad */, void* stream);
int grl_maxpool3x3s2_bf16(const void* x, void* y, int n, int H, int W, int C, void* stream);
int grl_group_mean_bf16(const void* x, float* y, int groups, int rows, int C, int ldy,
                        float out_scale, int accumulate, void* stream);
int grl_sqdiff_mean_bf16(const void* f1, const void* f2, float* d, int b, int rows, int C,
                         int64_t f2_clip_stride, void* stream);
int grl_gce_gate_bf16(const void* h, const float* w3, const float* bn_scale, const float* bn_shift,
                      const void* x, float* corr_map, void* x_corr, void* x_uncorr, int M, int Ch,
                      int C, void* stream);
int grl_temporal_mean_bf16(const void* x, void* y, int b, int T, int64_t inner, void* stream);
int grl_add_strided_bf16(const void* a, const void* b, void* y, int nb, int64_t inner,
                         int64_t b_clip_stride, void* stream);

/* ------------------------------------------------------------------------------------
 * Train mode: batch-statistics BatchNorm and the backward pass (autograd of the modules
 * above, driven by reid/train/trainer.py:54 `loss.backward()`).
 * ---------------------------------------------------------------------------------- */

/* column partials of x [M][C] (row stride ld): slab [grl_col_stats_rows(M)][2][C] = sum, sum sq of
 * (x - pivot[c]); pivot NULL = 0.  For BatchNorm statistics pass a row of x (and the same vector to
 * grl_bn_stats_finalize): the shifted moments keep the variance when |mean| >> spread. */
int grl_col_stats_rows(int M);
int grl_col_stats(const float* x, float* slab, int M, int C, int ld, const float* pivot, void* stream);
/* out[c] (+)= sum_r slab[r*stride + c]  (bias gradients, partial reductions) */
int grl_slab_sum(const float* slab, int rows, int64_t stride, int C, float* out, int accumulate,
                 void* stream);

/* nn.BatchNorm forward in training mode, step 1: from a partial slab [rows][2][C]
 * (written by grl_conv_gemm_f32's `stats` or by grl_col_stats) to batch mean / invstd,
 * folded scale/shift and the running-stat update (momentum, unbiased running var;
 * num_batches_tracked, if given, is incremented -- torch's int64 buffer). */
int grl_bn_stats_finalize(const float* slab, int rows, int C, int64_t count, const float* gamma,
                          const float* beta, float* running_mean, float* running_var,
                          int64_t* num_batches_tracked, float momentum, float eps, float* mean,
                          float* invstd, float* scale, float* shift,
                          const float* pivot /* the grl_col_stats pivot, or NULL */, void* stream);
/* step 2: y = relu?(z*scale + shift + res) */
int grl_bn_apply(const float* z, const float* scale, const float* shift, const float* res,
                 float* y, int64_t M, int C, int relu, void* stream);
/* BatchNorm finalize INSIDE the apply pass (round 6; train_bnfuse.hip): grl_bn_stats_finalize + grl_bn_apply_centered as ONE
 * launch for layers whose statistics slab is small (rows <= 64, i.e. M <= 8192 pixel rows -- the TRL memo bottleneck of
 * grl_model.py:93-128,186-205 --, C % 64 == 0): every workgroup of the apply pass reduces the slab columns of its own 64
 * channels, in the order of grl_bn_stats_finalize, so mean / invstd / scale / shift / running statistics and y are
 * bit-identical to the two-launch form.  Arguments: those of the two calls.  The backward entry points (grl_bn_bwd*,
 * grl_bn_bwd_finish*) take the same form by themselves when the slab allows it.  OFF unless GRL_BN_FINAPPLY=1 (or
 * grl_bn_finalize_apply_mode(1)): measured 0.4-0.9 ms per step slower than the separate launches (EXPERIMENTS.md round 6). */
int grl_bn_finalize_apply_takes(int rows, int C);      /* 1 if the fused form covers the layer */
int grl_bn_finalize_apply_mode(int on);                 /* test hook: 0 / 1 = off / on for the process, -1 = query; returns the previous setting */
int grl_bn_finalize_apply(const float* slab, int rows, int C, int64_t count, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                          float* mean, float* invstd, float* scale, float* shift, const float* pivot, const float* z,
                          const float* res, float* y, int M, int relu, uint8_t* relu_bits, void* stream);
int grl_bn_finalize_apply_bf16(const float* slab, int rows, int C, int64_t count, const float* gamma, const float* beta,
                               float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                               float* mean, float* invstd, float* scale, float* shift, const float* pivot, const void* z,
                               const void* res, void* y, int M, int relu, uint8_t* relu_bits, void* stream);
/* step 2, train-mode form: y = relu?((z - mean)*scale + beta + res), centred before the multiply as
 * torch's training kernel does (F.batch_norm(training=True); resnets1.py:76-91, grl_model.py:222-226):
 * exact where the folded form cancels (BatchNorm1d over a few similar rows).  beta may be NULL. */
int grl_bn_apply_centered(const float* z, const float* mean, const float* scale, const float* beta,
                          const float* res, float* y, int64_t M, int C, int relu,
                          uint8_t* relu_bits /* may be NULL: M*C/4 bytes, bit e of byte i = (y[4i + e] > 0) */,
                          void* stream);

/* BatchNorm (+ReLU) backward: g = dy*(act>0) (act NULL: no mask -- unless mask_scale is given: then the ReLU
 * mask of y = relu((z - mean)*mask_scale + mask_beta) is RECOMPUTED from z with the forward's own three fp32
 * operations (grl_bn_apply_centered without a residual), so the activation is not read at all);
 * dgamma += sum g*xhat; dbeta += sum g; dz = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)).
 * slab_ws: grl_col_stats_rows(M)*2*C floats, coef_ws: 2*C floats. gamma/dgamma/dbeta may be NULL.
 * gres (may be NULL): gradient of the residual input of y = relu(bn(z) + res), which is the same
 * masked g: gres (+)= g in the same pass (resnets1.py:88-91).  gres == dy with act given and gres_accumulate == 0:
 * IN-PLACE form -- the reduce pass overwrites dy with g (dy is NOT const then) and the apply pass reads it back, so
 * the caller's dy buffer becomes the residual's gradient: the activation is read once and no second tensor is written.
 * relu_bits (may be NULL): the mask bytes grl_bn_apply_centered recorded in the forward; they replace `act` (which
 * is then not read at all -- 1/16 of its bytes): same mask, same result. */
int grl_bn_bwd(const float* dy, const float* z, const float* act, const float* mean,
               const float* invstd, const float* gamma, float* dz, float* dgamma, float* dbeta,
               float* slab_ws, float* coef_ws, int M, int C, float* gres, int gres_accumulate,
               const float* mask_scale, const float* mask_beta, const uint8_t* relu_bits, void* stream);
/* The second half of grl_bn_bwd for a gradient that is ALREADY masked and reduced (GrlGemm.bn_z: the producing
 * data-gradient GEMM's epilogue left g in `g` and the partial sums in `slab`, `rows` of them): finalize (dgamma,
 * dbeta, the two means) and apply dz = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)); gres (+)= g as in grl_bn_bwd. */
int grl_bn_bwd_finish(const float* g, const float* z, const float* mean, const float* invstd, const float* gamma,
                      float* dz, float* dgamma, float* dbeta, const float* slab, int rows, float* coef_ws, int M, int C,
                      float* gres, int gres_accumulate, void* stream);
/* the bf16-storage twin (g, z, dz, gres bf16; round 5): the tail of grl_bn_bwd_bf16 behind a GrlGemm.bn_z GEMM */
int grl_bn_bwd_finish_bf16(const void* g, const void* z, const float* mean, const float* invstd, const float* gamma,
                           void* dz, float* dgamma, float* dbeta, const float* slab, int rows, float* coef_ws, int M, int C,
                           void* gres, int gres_accumulate, void* stream);

/* out (+)= dy * (act > 0)   (ReLU backward; act NULL = plain copy/accumulate) */
int grl_relu_bwd(const float* dy, const float* act, float* out, int64_t n, int accumulate, void* stream);
/* y = alpha*a + beta*b (b may be NULL) */
int grl_axpby(const float* a, const float* b, float* y, float alpha, float beta, int64_t n, void* stream);

/* dst[b*dst_stride + i] (+)= alpha*src[b*src_stride + i], i < inner (gradient accumulation
 * into one frame of a [b][T][...] tensor) */
int grl_axpy_strided(float* dst, int64_t dst_stride, const float* src, int64_t src_stride, int nb,
                     int64_t inner, float alpha, int accumulate, void* stream);
/* y[C][R] = x[R][C]^T (weights for the data-gradient GEMM of 1x1 convs / linears) */
int grl_transpose(const float* x, float* y, int R, int C, int ldx, void* stream);
/* [N][C][kh][kw] -> [C][flipped tap][N]: data gradient of a kxk conv as a conv over dz */
int grl_pack_dgrad_weight(const float* w, float* out, int N, int C, int kh, int kw, void* stream);
/* zero-stuffing of a stride-2 conv's output gradient: up[img][2oy+oy_off][2ox+ox_off] =
 * dz[img][oy][ox], zero elsewhere; accumulate == 1: += at those pixels, accumulate == 2: = at those
 * pixels, and nothing else is touched either way (the data gradient of a stride-2 conv is computed
 * at OUTPUT resolution, one GEMM per input-pixel parity class, and scattered this way) */
int grl_dilate2(const float* dz, float* up, int n, int Ho, int Wo, int H, int W, int C, int accumulate,
                int oy_off, int ox_off, void* stream);
/* nn.MaxPool2d(3,2,1) backward (first-maximum rule, deterministic gather form) */
int grl_maxpool3x3s2_bwd(const float* x, const float* dy, float* dx, int n, int H, int W, int C,
                         void* stream);
/* Stem tail of the training forward in one pass: y = maxpool3x3/s2/p1(relu((z - mean) * scale + beta)) (resnets1.py:108-
 * 110 in train mode: bn1, relu, maxpool) plus idx[pixel][C] (uint8: ky*3 + kx of the window's FIRST maximum in scan
 * order, torch's argmax rule) -- the post-ReLU map is never written.  grl_maxpool3x3s2_bwd_idx routes dy through idx
 * (dx = gradient of the post-ReLU map, H x W = the map's size); the ReLU mask then comes from grl_bn_bwd's mask_scale
 * form.  idx: 4-byte aligned (bf16: 8-byte). */
int grl_bn_relu_maxpool3x3s2(const float* z, const float* mean, const float* scale, const float* beta, float* y,
                             uint8_t* idx, int n, int H, int W, int C, void* stream);
int grl_maxpool3x3s2_bwd_idx(const uint8_t* idx, const float* dy, float* dx, int n, int H, int W, int C, void* stream);
/* Weight gradient of the 7x7/s2/p3 stem conv (resnets1.py:106-107 / basebranch.py:27) straight from the NCHW clip:
 * dw[64][3][7][7] (+)= sum over output pixels of dz[pixel][64] (x) the pixel's 147 input taps -- no im2col matrix
 * (grl_stem_im2col + grl_conv_wgrad_f32 write and re-read 671 MB per 32 x 4 step).  x: fp32 [n][3][H][W]; dz: fp32, or
 * bf16 when dz_bf16 (converted exactly); exact fp32 products.  ws: grl_stem_wgrad_workspace_floats(n, H, W) floats
 * (one partial [64][160] per persistent workgroup, summed in workgroup order: deterministic). */
int64_t grl_stem_wgrad_workspace_floats(int n, int H, int W);
int grl_stem_wgrad(const float* x, const void* dz, int dz_bf16, float* dw, float* ws, int n, int H, int W,
                   int accumulate, void* stream);
/* im2col of the NCHW stem input for the 7x7 weight gradient: [n*H/2*W/2][Kp], 147 real columns */
int grl_stem_im2col(const float* x, float* col, int n, int H, int W, int Kp, void* stream);

/* Weight gradient  dW[n][k] (+)= sum_m dz[m][n] * X[m][k]  as an fp32 MFMA GEMM with the
 * pixel reduction split over workgroups (deterministic slab reduction).  conv != 0: X is
 * gathered from channels-last images and dW is written in torch layout [N][C][kh][kw]. */
typedef struct GrlWgrad {
    const float* dz;        /* [M][ldz]                                   */
    const float* x;         /* dense [M][ldx] or images [nimg][H][W][C]   */
    float*       dw;        /* [N][k_out] (dense) or [N][C][kh][kw]       */
    float*       workspace; /* grl_wgrad_workspace_floats(desc) floats    */
    int32_t M, N, K, ldz, ldx;
    int32_t k_out;          /* dense: columns of dw actually written (0 = K) */
    int32_t accumulate;
    int32_t conv, H, W, C, Ho, Wo, kh, kw, stride, pad;
    int32_t math;           /* GRL_MATH_F32 (exact), GRL_MATH_BF16X3 (split-bf16 products) or GRL_MATH_BF16: the
                               bf16 MFMA datapaths apply to 128 x 128 tiles (N >= 128, C or K % 128 == 0), other
                               shapes run exact fp32; accumulation and the slab reduction are always fp32 */
    int32_t in_bf16;        /* 1: dz and x are bf16 tensors (ldz / ldx in elements; train_engine math 'bf16s'): plain
                               bf16 products on 128 x 128 tiles for every shape (N, K, ld % 8 == 0), fp32 dW */
} GrlWgrad;
int64_t grl_wgrad_workspace_floats(const GrlWgrad* desc);
int grl_conv_wgrad_f32(const GrlWgrad* desc, void* stream);

/* GCE gate in train mode (logit already batch-normalised, first column of y[M][ldy]):
 * map = sigmoid(y), x_corr = x*map, x_uncorr = x*(1-map)          (basebranch.py:63-66) */
int grl_gate_apply(const float* y, int ldy, const float* x, float* cmap, float* xc, float* xu,
                   int M, int C, void* stream);
/* its backward: dx (+)= dxc*map + dxu*(1-map); dy[m*ldy] = map(1-map) sum_c (dxc-dxu)*x */
int grl_gate_bwd(const float* dxc, const float* dxu, const float* x, const float* cmap, float* dx,
                 int accumulate, float* dy, int ldy, int M, int C, void* stream);
/* dst[m][c] (+)= v[m / rows_per_group][c] * scale: backward of every mean over rows
 * (GAP, global descriptor, temporal mean with C = a whole frame) */
int grl_add_rowbcast(float* dst, const float* v, int64_t M, int64_t C, int64_t rows_per_group,
                     float scale, int accumulate, void* stream);
/* backward of grl_sqdiff_mean: df1 = 2(f1-f2)dd/rows, df2 (+)= -df1 */
int grl_sqdiff_bwd(const float* f1, const float* f2, const float* dd, float* df1, float* df2,
                   int b, int rows, int C, int64_t f2_clip_stride, int accumulate_df2, void* stream);
/* backward of f_step = gap*c + gap through the sigmoid: ds = dfs*gap*c(1-c), dgap (+)= dfs*(1+c) */
int grl_catte_bwd(const float* dfs, int64_t dfs_stride, const float* gap, int64_t gap_stride,
                  const float* catte, float* ds, float* dgap, int64_t dgap_stride, int accumulate,
                  int b, int C, void* stream);
/* backward of y = v/|v| (F.normalize, grl_model.py:223,226): dv = (dy - y(y.dy))/|v| */
int grl_l2norm_bwd(const float* dy, int64_t lddy, const float* y, int64_t ldy, const float* v,
                   float* dv, int rows, int C, void* stream);
/* backward of grl_siamese_attn: gradients of the (BN-ed) Q|K rows and of the frame features */
int grl_siamese_attn_bwd(const float* qk, const float* x, const float* out, int64_t ldo,
                         const float* dout, int64_t lddo, float* dqk, float* dx, int dx_accumulate,
                         int b, int T, int D, int C, void* stream);
/* verification head, train mode: diff[i*ng+j] = (p_i - g_j)^2 and its backward (Siamese.py:133-137) */
int grl_pair_sqdiff(const float* p, const float* g, float* diff, int np, int ng, int K, void* stream);
int grl_pair_sqdiff_bwd(const float* p, const float* g, const float* ddiff, float* dp, float* dg,
                        int np, int ng, int K, void* stream);

/* OIM look-up-table update performed inside OIM.backward (reid/loss/oim.py:24-26): per sample,
 * in batch order, lut[y] = m*lut[y] + (1-m)*x, then renormalise the row.  labels: int64; a
 * label outside [0, num_classes) updates nothing (lut is [num_classes][D]). */
int grl_oim_update(float* lut, const float* x, const int64_t* labels, int n, int D, int num_classes,
                   float momentum, void* stream);

/* Cluster-memory update of cluster-contrast training (cmem.hip, ClusterMemoryLoss).  Additive:
 * GRL_ABI_VERSION stays 10.  cent [K][D] is updated in place, x is [n][D], labels int64 [n]; D % 4 == 0, n >= 1, K >= 1,
 * cent and x 16-byte aligned.  A label outside [0, K) updates nothing (DBSCAN's noise label -1).  For every label y
 * present, its members are the ascending j with labels[j] == y.
 *   mode 0 (hard): s_j = sum_c x[j][c] * cent[y][c] on the row as it is BEFORE this launch; j* = the member with the
 *     smallest s_j under a strict < against a running best that starts at the first member (the first member wins ties, a
 *     NaN never replaces the running best); v = x[j*].
 *   mode 1 (mean): v = (sum over the members of x[j], added in ascending j from 0) / (float)count.
 *   then, as grl_oim_update: cent[y] = momentum * cent[y] + (1 - momentum) * v, and the row is scaled by
 *     1 / sqrtf(sum c^2) (a zero-norm row becomes NaN, as there).
 * sel (int32 [n], may be NULL): 1 where row i contributed (hard: the selected member; mean: every member), 0 elsewhere
 * and on rows whose label is out of range.
 * One 256-lane workgroup per batch row; the workgroup of a label's first row is the only writer of that centroid row
 * and of its members' sel.  Every dot product and sum of squares: lane t adds dot4 of the floats 4 t + 1024 k .. + 3 for
 * k = 0, 1, ..., the wave's 64 partials meet in an xor tree, the four waves' totals are added in sequence from 0.  No
 * atomics: the result is the same bits on every run, and a row's result does not depend on the batch's other labels. */
int grl_cmem_update(float* cent, const float* x, const int64_t* labels, int n, int D, int K, float momentum, int mode,
                    int32_t* sel, void* stream);

/* Camera-aware proxy cross entropy of unsupervised training (proxy.hip, ProxyMemoryLoss): a cross entropy
 * over per-row sets of columns with a deterministic top-k selection of hard negatives, forward and gradient in one call.
 * Additive: GRL_ABI_VERSION stays 10.  logits [n][ld] (P columns used) are the scaled similarities of the n rows to the
 * P proxies; labels / cams int64 [n] are the row's cluster id and camera id; proxy_cluster / proxy_cam int32 [P] say
 * which (cluster, camera) pair every proxy stands for.
 * Row i:
 *   own_i = the smallest j with proxy_cluster[j] == labels[i] and proxy_cam[j] == cams[i].  If there is none (the noise
 *     label -1, a pair without a proxy) the row is INVALID: own[i] = -1, its dlogits row is zeros, its negsel row is -1,
 *     and it adds nothing to loss or correct.
 *   For a valid row:  A_i = {j : proxy_cam[j] == cams[i]},  Pos_i = {j : proxy_cluster[j] == labels[i]} (holds own_i),
 *     N_i = {j : proxy_cluster[j] != labels[i]},  Neg_i = the first min(k_neg, |N_i|) members of N_i in the order
 *     logit descending, then index ascending -- compared as fp32 values as given (-0 == +0),  U_i = Pos_i + Neg_i.
 *   L_i = w_intra (lse_{A_i}(z) - z[own_i]) + w_inter (lse_{U_i}(z) - (1 / |Pos_i|) sum_{j in Pos_i} z[j]);
 *     each lse is shifted by the maximum over its own set, and the mean over Pos_i is taken of the shifted logits.
 * nv = the number of valid rows.  loss[0] = (sum over the valid rows of L_i) / nv, 0 if nv = 0: the terms fl(fl(1 / nv) L_i)
 * are added in index order from 0, as the rows of grl_softmax_ce.
 * dlogits[i][j] (may be NULL) = (1 / nv) ( w_intra [j in A_i] (p^A_j - [j == own_i])
 *                                        + w_inter [j in U_i] (p^U_j - [j in Pos_i] / |Pos_i|) ),  p^S the softmax over S.
 * correct[0] (may be NULL) = the number of valid rows with proxy_cluster[arg] == labels[i], arg the arg-max over all P
 *   columns (first index on ties, as grl_softmax_ce).
 * own (int64 [n], may be NULL) = own_i.  negsel (int32 [n][k_neg], may be NULL; ignored when k_neg = 0) = Neg_i in
 *   ascending j, padded with -1.  k_neg = 0: no negatives.
 * ws: 3 * n floats of scratch.
 * Limits, each refused with GRL_EINVAL before anything is launched: n < 1, P < 1, k_neg outside 0 .. P, ld < P,
 * dlogits given and ldd < P, a NULL logits / labels / cams / proxy_cluster / proxy_cam / loss / ws, P > GRL_PROXY_MAX_P
 * (the row and its set flags live in LDS, under the 64 KB a workgroup gets without an opt-in).
 * A NaN logit gives unspecified values, never an access outside the arrays.
 * Two launches.  First one 256-lane workgroup per row: lane t takes the columns t + 256 k; every max, sum and count is
 * a wave64 xor tree followed by the four waves' totals in sequence; the selection threshold is the k-th largest
 * order-preserving key of N_i, found bit by bit from exact integer counts, and the columns that equal it are admitted by a
 * prefix count in index order.  Then the rows' losses, hits and valid flags are added in index order, every workgroup of
 * that launch re-derives nv from the same flags, and dlogits is scaled by fl(1 / nv).  No atomics: the same bits on every run. */
#define GRL_PROXY_MAX_P 8192
int grl_proxy_ce(const float* logits, int64_t ld, const int64_t* labels, const int64_t* cams,
                 const int32_t* proxy_cluster, const int32_t* proxy_cam, int n, int P, int k_neg, float w_intra,
                 float w_inter, float* loss, float* correct, float* dlogits, int64_t ldd, int64_t* own,
                 int32_t* negsel, float* ws, void* stream);

/* Hybrid-memory cross entropy of self-paced unsupervised training (hybrid.hip, HybridMemoryLoss; SpCL, Ge
 * et al. 2020): a cross entropy whose classes are SETS of columns, forward and gradient in one call.  Additive:
 * GRL_ABI_VERSION stays 10.  logits [n][ld] (N columns used) are the scaled similarities of the n rows to the N rows of an
 * instance memory; targets int64 [n] is the class of every row.
 * The classes: class_ptr int32 [C + 1], class_members int32 [N] and inst_class int32 [N] describe a partition of 0 .. N - 1
 * into C non-empty classes -- the members of class c are class_members[class_ptr[c] .. class_ptr[c + 1]), in ascending
 * index, and inst_class[j] is the class of column j (the inverse of the two).  The caller validates the tables
 * (HybridMemoryLoss.reset does); the kernel assumes a valid partition.
 * A row whose target is outside [0, C) is INVALID: its dlogits row is zeros and it adds nothing to loss or correct.
 * For a valid row i with target y:
 *   z_c = (sum of logits[i][j] over the members j of c, added one by one in list order starting from the first member)
 *         / (float)|c| -- a singleton's z_c is its logit, bit for bit.
 *   L_i = lse_C(z) - z_y, the lse shifted by the maximum of z;  p = softmax_C(z).
 * nv = the number of valid rows.  loss[0] = (sum over the valid rows of L_i) / nv, 0 if nv = 0: the terms fl(fl(1 / nv) L_i)
 * are added in index order from 0, as the rows of grl_softmax_ce.
 * dlogits[i][j] (may be NULL) = fl(1 / nv) * fl((p_c - [c == y]) / (float)|c|) with c = inst_class[j].
 * correct[0] (may be NULL) = the number of valid rows whose arg-max CLASS equals y (first class index on ties).
 * ws: 3 * n floats of scratch.
 * With C = N singleton classes in identity order, loss, dlogits and correct are grl_softmax_ce's (weight = NULL) bit for bit.
 * Limits, each refused with GRL_EINVAL before anything is launched: n < 1, N < 1, C < 1, C > N, ld < N, dlogits given and
 * ldd < N, a NULL logits / targets / class_ptr / class_members / inst_class / loss / ws, C > GRL_HYBRID_MAX_CLASSES (z lives
 * in LDS next to the reduction scratch, under the 64 KB a workgroup gets without an opt-in; MARS has 8298 training
 * tracklets).  The logits row stays in global memory: N has no limit of its own.
 * A NaN logit gives unspecified values, never an access outside the arrays.
 * Two launches.  First one 256-lane workgroup per row: lane t takes the classes t + 256 k, sums each class's members
 * through the table (every logit is read once) and keeps z in LDS; max, sum and arg-max are a wave64 xor tree followed by
 * the four waves' totals in sequence, as grl_softmax_ce; every class's gradient is computed once, then lane t takes the
 * COLUMNS t + 256 k and writes dlogits through inst_class.  The second launch is grl_proxy_ce's: the rows' losses, hits
 * and valid flags are added in index order, every workgroup re-derives nv, dlogits is scaled by fl(1 / nv).  No atomics:
 * the same bits on every run. */
#define GRL_HYBRID_MAX_CLASSES 15360
int grl_hybrid_ce(const float* logits, int64_t ld, const int64_t* targets, const int32_t* class_ptr,
                  const int32_t* class_members, const int32_t* inst_class, int n, int N, int C, float* loss,
                  float* correct, float* dlogits, int64_t ldd, float* ws, void* stream);

/* Cross entropy against a hard label blended with a teacher's softmax (softce.hip, SoftClusterMemoryLoss, DESIGN.md 4al;
 * Mean Teacher, Tarvainen & Valpola 2017; MMT, Ge et al. 2020), forward and gradient in one call.  Additive:
 * GRL_ABI_VERSION stays 10.  logits [n][ld] and tlogits [n][ldt] (c columns used of each) are the student's and the
 * teacher's scaled similarities to the same c memory rows; labels int64 [n].
 * A row whose label is outside [0, c) is INVALID: its dlogits row is +0 and it adds nothing to loss or correct.
 * For a valid row i with label y, z = logits[i], t = tlogits[i], w = w_soft, omw = fl(1 - w):
 *   mx = max_j z_j;  lse = logf(sum_j expf(z_j - mx));  p_j = expf(fl(fl(z_j - mx) - lse))
 *   mt = max_j t_j;  lt  = logf(sum_j expf(t_j - mt));  q_j = expf(fl(fl(t_j - mt) - lt))
 *   X   = sum_j fl(q_j * fl(z_j - mx))
 *   L_i = fl(fl(lse - fl(omw * fl(z_y - mx))) - fl(w * X))
 *       = lse(z) - (1 - w) z_y - w sum_j q_j z_j: the cross-entropy form of MMT (not the KL divergence: the two differ by
 *         the teacher's entropy, a constant in the student), the shift mx cancelling because (1 - w) + w sum_j q_j = 1
 *   d_ij = fl(fl(p_j - fl(omw * [j == y])) - fl(w * q_j))
 * With w = 0 the terms in w are not evaluated and tlogits is never read (it may be NULL).
 * nv = the number of valid rows.  loss[0] = sum over the valid rows of fl(fl(1 / nv) L_i), added in index order from 0
 * (0 if nv = 0), as the rows of grl_softmax_ce.  dlogits[i][j] (may be NULL) = fl(fl(1 / nv) d_ij).
 * correct[0] (may be NULL) = the number of valid rows whose arg-max of the STUDENT row is y (first index on ties).
 * ws: 3 * n floats of scratch.
 * With w_soft = 0, loss, dlogits and correct are grl_softmax_ce's (weight = NULL) bit for bit.
 * Limits, each refused with GRL_EINVAL before anything is launched: n < 1, c < 1, ld < c, dlogits given and ldd < c, a
 * NULL logits / labels / loss / ws, w_soft outside [0, 1] (a NaN included), w_soft != 0 with tlogits NULL or ldt < c.
 * A NaN logit gives unspecified values, never an access outside the arrays.
 * Two launches.  First one 256-lane workgroup per row: lane t takes the columns t + 256 k, adding its terms in that
 * order from 0; every max and sum is a wave64 xor tree followed by the four waves' totals in sequence, as
 * grl_softmax_ce.  Both rows stay in global memory: c has no limit of its own.  The second launch is grl_proxy_ce's: the
 * rows' losses, hits and valid flags are added in index order, every workgroup re-derives nv, dlogits is scaled by
 * fl(1 / nv).  No atomics: the same bits on every run. */
int grl_soft_ce(const float* logits, int64_t ld, const float* tlogits, int64_t ldt, const int64_t* labels,
                float w_soft, int n, int c, float* loss, float* correct, float* dlogits, int64_t ldd,
                float* ws, void* stream);

/* Hybrid-memory cross entropy against a hard class blended with a teacher's softmax over the same classes
 * (soft_hybrid.hip, SoftHybridMemoryLoss): grl_hybrid_ce's classes with grl_soft_ce's target, forward and
 * gradient in one call.  Additive: GRL_ABI_VERSION stays 10.  logits [n][ld] and tlogits [n][ldt] (N columns used of
 * each) are the student's and the teacher's scaled similarities to the same N instance-memory rows; targets and the class
 * tables are grl_hybrid_ce's, with the same validity rule and the same caller-side validation.
 * For a valid row i with target y, w = w_soft, omw = fl(1 - w):
 *   z_c = grl_hybrid_ce's: logits[i][j] over the members j of c, added one by one in list order from the first member,
 *         / (float)|c|;  t_c = the same formula on tlogits[i].
 *   mx = max_c z_c;  lse = logf(sum_c expf(z_c - mx));  p_c = expf(fl(fl(z_c - mx) - lse))
 *   mt = max_c t_c;  lt  = logf(sum_c expf(t_c - mt));  q_c = expf(fl(fl(t_c - mt) - lt))
 *   X   = sum_c fl(q_c * fl(z_c - mx))
 *   L_i = fl(fl(lse - fl(omw * fl(z_y - mx))) - fl(w * X))
 *   d_c = fl(fl(p_c - fl(omw * [c == y])) - fl(w * q_c))
 * With w = 0 the terms in w are not evaluated, tlogits is never read (it may be NULL) and only the first 3 n floats of ws
 * are touched.
 * nv = the number of valid rows.  loss[0] = sum over the valid rows of fl(fl(1 / nv) L_i), added in index order from 0
 * (0 if nv = 0).  dlogits[i][j] (may be NULL) = fl(fl(1 / nv) * fl(d_c / (float)|c|)) with c = inst_class[j]; the teacher
 * gets no gradient.
 * correct[0] (may be NULL) = the number of valid rows whose arg-max CLASS of the STUDENT equals y (first class on ties).
 * ws: 3 * n floats of scratch when w_soft = 0, 3 * n + n * C floats otherwise -- the student's z fills the LDS budget, so
 *   the teacher's class logits (then q) of row i live in ws[3 n + i C ..); lane t writes and reads back the entries
 *   t + 256 k only.
 * With w_soft = 0, loss, dlogits and correct are grl_hybrid_ce's bit for bit.  With C = N singleton classes in identity
 * order they are grl_soft_ce's bit for bit, as grl_hybrid_ce's are grl_softmax_ce's.
 * Limits, each refused with GRL_EINVAL before anything is launched: everything grl_hybrid_ce refuses (C >
 * GRL_HYBRID_MAX_CLASSES included: no LDS opt-in is taken), w_soft outside [0, 1] (a NaN included), w_soft != 0 with
 * tlogits NULL or ldt < N.
 * A NaN logit gives unspecified values, never an access outside the arrays.
 * Two launches.  First one 256-lane workgroup per row: lane t takes the classes t + 256 k, adding its terms in that order
 * from 0; every max and sum is a wave64 xor tree followed by the four waves' totals in sequence, as grl_hybrid_ce.  The
 * second launch is grl_proxy_ce's.  No atomics: the same bits on every run. */
int grl_soft_hybrid_ce(const float* logits, int64_t ld, const float* tlogits, int64_t ldt, const int64_t* targets,
                       const int32_t* class_ptr, const int32_t* class_members, const int32_t* inst_class, float w_soft,
                       int n, int N, int C, float* loss, float* correct, float* dlogits, int64_t ldd, float* ws,
                       void* stream);

/* Camera-aware proxy cross entropy against hard targets blended with a teacher's softmaxes (soft_proxy.hip,
 * SoftProxyMemoryLoss): grl_proxy_ce's two cross entropies, each against (1 - w) its hard target + w the
 * teacher's softmax over the same set.  Additive: GRL_ABI_VERSION stays 10.  tlogits [n][ldt] (P columns used) are the
 * teacher's scaled similarities to the same P proxies; every other argument is grl_proxy_ce's.
 * own_i, A_i, Pos_i, N_i, Neg_i, U_i, negsel and correct come from the STUDENT's logits exactly as in grl_proxy_ce; the
 * teacher is read at the student's selection (the rule of grl_soft_triplet_fwd).
 * For a valid row, z = logits[i], t = tlogits[i], w = w_soft, omw = fl(1 - w), S one of A_i, U_i:
 *   mx_S = max_{j in S} z_j;  lse_S = logf(sum_{j in S} expf(z_j - mx_S));  p^S_j = expf(fl(fl(z_j - mx_S) - lse_S))
 *   mt_S = max_{j in S} t_j;  lt_S  = logf(sum_{j in S} expf(t_j - mt_S));  q^S_j = expf(fl(fl(t_j - mt_S) - lt_S))
 *   X_S  = sum_{j in S} fl(q^S_j * fl(z_j - mx_S))
 *   h_A  = fl(z[own_i] - mx_A);   h_U = fl((sum_{j in Pos_i} fl(z_j - mx_U)) * fl(1 / |Pos_i|))
 *   L_S  = fl(fl(lse_S - fl(omw * h_S)) - fl(w * X_S))
 *   L_i  = fl(fl(w_intra * L_A) + fl(w_inter * L_U))
 *        = w_intra (lse_A(z) - (1 - w) z[own] - w sum_A q^A_j z_j) + w_inter (lse_U(z) - (1 - w) mean_Pos z - w sum_U q^U_j z_j):
 *          both target vectors sum to 1, so the shifts cancel.
 *   g^A_j = fl(fl(p^A_j - fl(omw * [j == own_i])) - fl(w * q^A_j)),
 *   g^U_j = fl(fl(p^U_j - fl(omw * ([j in Pos_i] ? fl(1 / |Pos_i|) : 0))) - fl(w * q^U_j))
 *   d_ij  = fl([j in A_i] fl(w_intra * g^A_j) + [j in U_i] fl(w_inter * g^U_j))
 * With w = 0 the terms in w are not evaluated and tlogits is never read (it may be NULL).
 * loss, dlogits (= fl(fl(1 / nv) d_ij)), correct, own, negsel and ws (3 * n floats) are laid out as grl_proxy_ce's.
 * With w_soft = 0 every output is grl_proxy_ce's bit for bit.
 * Limits, each refused with GRL_EINVAL before anything is launched: everything grl_proxy_ce refuses, w_soft outside
 * [0, 1] (a NaN included), w_soft != 0 with tlogits NULL or ldt < P.  The teacher's row stays in global memory:
 * GRL_PROXY_MAX_P and the LDS budget are grl_proxy_ce's.
 * A NaN logit gives unspecified values, never an access outside the arrays.
 * Two launches, as grl_proxy_ce: lane t takes the columns t + 256 k, adding its terms in that order from 0; every max, sum
 * and count is a wave64 xor tree followed by the four waves' totals in sequence.  No atomics: the same bits on every run. */
int grl_soft_proxy_ce(const float* logits, int64_t ld, const float* tlogits, int64_t ldt, const int64_t* labels,
                      const int64_t* cams, const int32_t* proxy_cluster, const int32_t* proxy_cam, float w_soft, int n,
                      int P, int k_neg, float w_intra, float w_inter, float* loss, float* correct, float* dlogits,
                      int64_t ldd, int64_t* own, int32_t* negsel, float* ws, void* stream);

/* Exponential moving average of a set of tensors in ONE launch (ema.hip, MeanTeacher).  Additive:
 * GRL_ABI_VERSION stays 10.  table_dev: `count` entries in DEVICE memory, built once per model by the host; for every
 * entry and every element
 *   dst[k] = fl(fl(alpha * dst[k]) + fl(one_minus_alpha * src[k]))
 * (both factors from the host, as lambda_value / one_minus_lambda below; two products and one sum, no fused multiply-add:
 * a float32 restatement reproduces the bits).  alpha = 0 copies src, alpha = 1 leaves the finite values of dst as they
 * are (numerically: -0 becomes +0 against a finite positive src), NaN and inf propagate as the formula says.
 * The tensors are cut into chunks of GRL_EMA_CHUNK = 4096 floats (16 KB of dst and of src: four 16-byte loads of each
 * per lane, all in flight before the first store).  chunk_first_dev: int64 [count + 1] in device memory,
 * chunk_first[e] = sum over e' < e of ceil(numel[e'] / GRL_EMA_CHUNK), so chunk_first[count] is the number of chunks.  A
 * workgroup of 256 lanes finds the entry of its chunk by binary search in chunk_first; the grid is capped (2048
 * workgroups) and strides over the chunks.  16-byte loads and stores where the chunk's dst and src are both 16-byte
 * aligned, scalar ones otherwise and for the last numel % 4 floats.  Every element has one writer: no atomics, the same
 * bits on every run.
 * The entries are device memory and are NOT validated here: the caller guarantees that every dst / src holds numel
 * floats, that no dst overlaps another dst or any src, and that chunk_first matches the entries (MeanTeacher checks
 * what it puts into the table).
 * GRL_EINVAL, before anything is launched: count < 1, a NULL table_dev, a NULL chunk_first_dev. */
#define GRL_EMA_CHUNK 4096
typedef struct GrlEmaEntry { float* dst; const float* src; int64_t numel; } GrlEmaEntry;
int grl_ema_update(const GrlEmaEntry* table_dev, const int64_t* chunk_first_dev, int count,
                   float alpha, float one_minus_alpha, void* stream);

/* ---- the trainer's loss block, forward and backward on the device ---- */
/* F.cross_entropy of OIMLoss.forward (reid/loss/oim.py:52; mean reduction, optional class
 * weight): loss[0] = sum_i w[y_i] (logsumexp(z_i) - z_i[y_i]) / sum_i w[y_i];
 * dlogits[i][j] = d loss[0] / d z_i[j] (may be NULL); correct[0] (may be NULL) = number of rows
 * whose arg-max (first index on ties, as topk in eva_functions.py:118-131) equals the label.
 * Labels outside [0,c) carry weight 0 (torch's ignore_index).  ws: 2*n floats of scratch. */
int grl_softmax_ce(const float* logits, int64_t ld, const int64_t* labels, const float* weight, int n,
                   int c, float* loss, float* correct, float* dlogits, int64_t ldd, float* ws,
                   void* stream);
/* OIM.backward's input gradient (oim.py:22) with the scalar of oim.py:50 and the upstream
 * gradient g[0] (device scalar, NULL = 1) folded in: dx = alpha*g * dlogits . lut */
int grl_oim_grad(const float* dlogits, int64_t ldd, const float* lut, const float* g, float alpha,
                 float* dx, int n, int c, int D, void* stream);
/* TripletLoss('soft', batch_hard=True).forward, mode 'id', dis_func 'eu' (reid/loss/triplet.py:16-76,
 * cdist :78-90): dist[i][j] = sqrt(sum_k (f_i-f_j)^2 + 1e-12); z_i = max_j dist*[same id, j != i]
 * - min_j (dist + 1e5*[same id]); loss[i] = soft ? log(1 + exp(z_i)) : max(z_i + margin, 0).
 * sel[i] = {arg-max or -1 when the maximum is a masked zero, arg-min} (first index on ties) for
 * the backward. */
int grl_triplet_fwd(const float* feat, const int64_t* ids, int n, int D, int soft, float margin,
                    float* loss, float* dist, int32_t* sel, float* z, void* stream);
int grl_triplet_bwd(const float* feat, const float* dist, const int32_t* sel, const float* z,
                    const float* dloss, int soft, float margin, float* dfeat, int n, int D,
                    void* stream);
/* The soft-margin batch-hard triplet loss blended with a mean teacher's soft target (soft_triplet.hip, SoftTripletLoss,
 * DESIGN.md 4am; MMT's SoftTripletLoss, Ge et al. 2020).  Additive: GRL_ABI_VERSION stays 10.
 * Student part: dist, sel and z are what grl_triplet_fwd(feat, ids, n, D, soft = 1, ...) writes, bit for bit (the same
 * distance row, masks, first-index tie rule and sel[2i] = -1 rule; jp, jn below are the arg-max / arg-min it found).
 * Teacher part (only when w_soft != 0), from tfeat [n][D], the teacher's rows of the same samples:
 *   td(i, j) = sqrtf(sum_k (tf_i - tf_j)^2 + 1e-12f), in the student loop's lane stride and wave reduction,
 *   tp = sel[2i] >= 0 ? td(i, jp) : 0,    tn = fl(td(i, jn) + 1e5f [ids[jn] == ids[i]]),    t = fl(tp - tn),
 *   q[i] = 1 / (1 + expf(-t))             (finite at both ends: t = -1e5 gives 0),
 * the student's masks mirrored; where every anchor has a positive and a different-id negative this is MMT's plain gather.
 *   loss[i] = fl( logf(1 + expf(z)) - fl( fl(w_soft q) z ) )        -- in this order, no fused multiply-add.
 * With w_soft = 0 tfeat is never read, q is not written (both may be NULL) and loss is grl_triplet_fwd's bit for bit.
 * Backward: grl_triplet_bwd's gather form and term order with
 *   gz = dloss[i] * fl( ez / (1 + ez) - fl(w_soft q[i]) ),   ez = expf(z[i]);
 * with w_soft = 0 q is not read and dfeat is grl_triplet_bwd's (soft = 1) bit for bit.  The teacher gets no gradient.
 * Limits, each refused with GRL_EINVAL before anything is launched: D % 4 != 0, n < 1, n > 16384, a NULL feat / ids /
 * loss / dist / sel / z / dloss / dfeat, w_soft outside [0, 1] (a NaN included), w_soft != 0 with tfeat or q NULL.
 * Forward: one launch, one 256-lane workgroup per anchor, LDS = n floats + 4 words.  Backward: one launch.  No atomics. */
int grl_soft_triplet_fwd(const float* feat, const float* tfeat, const int64_t* ids, int n, int D, float w_soft,
                         float* loss, float* dist, int32_t* sel, float* z, float* q, void* stream);
int grl_soft_triplet_bwd(const float* feat, const float* dist, const int32_t* sel, const float* z, const float* q,
                         const float* dloss, float w_soft, float* dfeat, int n, int D, void* stream);
/* Hard instance contrast and soft instance consistency against a mean teacher (ins_contrast.hip, InstanceContrastLoss,
 * DESIGN.md 4ao; the instance terms of ICE, Chen et al. 2021).  Additive: GRL_ABI_VERSION stays 10.
 * feat [n][D] the student's rows, tfeat [n][D] the teacher's rows of the same samples (no gradient), ids [n] int64 of any value.
 *   u_i = f_i / max(|f_i|, 1e-12),  v_j = m_j / max(|m_j|, 1e-12)   (F.normalize's clamp),  c_ij = <u_i, v_j>,  t_ij = <v_i, v_j>.
 * Selection, per anchor i: one column per distinct id of the batch -- of the anchor's own id (i counts as a member) the member
 * with the SMALLEST c_ij, the hard positive p_i; of every other id the member with the LARGEST c_ij; among equal values the lowest
 * column index.  K_i is the selected set.  Over K_i, the row maximum subtracted in both softmaxes:
 *   P = softmax(c_ik / tau),  Q = softmax(t_ik / tau_t)      (the teacher's similarities at the STUDENT's selection),
 *   loss[i] = fl( fl(w_hard nl_p) + fl(w_soft sum_k fl(Q_k nl_k)) ),   nl_k = -log P_k = fl( logf(S) - fl(fl(c_ik / tau) - max) ),
 *   coef[i][k] = g_ik = dloss_i / d(c_ik / tau) = fl( fl(w_hard fl(P_k - [k = p_i])) + fl(w_soft fl(P_k - Q_k)) ),
 * with P_k = e_k / S, e_k = expf(fl(c_ik / tau) - max), S = sum_k e_k, and Q_k likewise from t and tau_t.  With w_soft = 0 t, Q
 * and the w_soft terms are never computed.  A batch with one id gives loss = 0 and coef = 0 exactly.
 * Outputs: loss [n]; cos [n][n] = c_ij; sel [n][n] int32 = 0 unselected / 1 a selected negative / 2 the hard positive;
 * coef [n][n] = g_ik, 0 where unselected.
 * Orders (no atomics, no fused multiply-add, the same bits every run): every dot product over D is one wave's -- lane l takes the
 * float4 l + 64 t, adds its four products left to right and its trips in sequence from 0, then the wave64 xor tree (offsets 32 ..
 * 1), the shape of the triplet kernels' distance -- and c_ij = fl(fl(<f_i, m_j> inv_f_i) inv_m_j) with inv = 1 / max(sqrtf(ss),
 * 1e-12f); the inverse norms are recomputed by every workgroup, none is stored.  S, the teacher's sum and sum_k Q_k nl_k run over
 * ascending column index.
 * Backward, one 256-lane workgroup per row, every element of dfeat written by one lane:
 *   w_k = fl(coef[i][k] inv_m_k),  gu = fl( (sum over ascending k with w_k != 0 of fl(m_k w_k)) fl(1 / tau) ),  u = fl(f_i inv_f_i),
 *   dot = <u, gu> (lane l takes the float4 l + 256 t, four products left to right, trips in sequence, wave tree, the four waves
 *   added in sequence),   dfeat[i] = fl( fl( fl(gu - fl(u dot)) inv_f_i ) dloss[i] );
 * a row under the clamp (sqrtf(|f_i|^2) < 1e-12f, a zero row) gets dfeat[i] = 0.
 * Limits, each refused with GRL_EINVAL before anything is launched: a NULL pointer, n < 1, n > 2048 (the forward keeps 6 n words
 * of LDS: 48 KiB at the cap), D < 4, D % 4 != 0, tau or tau_t not > 0 or not finite, a negative or non-finite weight, both
 * weights 0.  One launch each; LDS is touched with 32-bit accesses only. */
int grl_ins_contrast_fwd(const float* feat, const float* tfeat, const int64_t* ids, int n, int D, float tau, float tau_t,
                         float w_hard, float w_soft, float* loss, float* cos, int32_t* sel, float* coef, void* stream);
int grl_ins_contrast_bwd(const float* feat, const float* tfeat, const float* coef, const float* dloss, float tau, float* dfeat,
                         int n, int D, void* stream);
/* prob[t] = softmax(scores[t][0..1])[1] (reid/train/trainer.py:146-148; prob0, optional, keeps the
 * class-0 probability for the backward) and its backward, term for term as torch's softmax backward */
int grl_softmax2(const float* scores, float* prob, float* prob0, int64_t m, void* stream);
int grl_softmax2_bwd(const float* prob, const float* prob0, const float* dprob, float* dscores, int64_t m,
                     void* stream);
/* PairLoss.forward (reid/loss/pairloss.py:18-45): label[a][b] = [tar_probe[b] == tar_gallery[a]];
 * loss[0] = BCE(prob, label) (mean, logs clamped at -100); prec[0] (may be NULL) = top-1 precision of
 * the (1-s, s) pseudo-logits; dprob (may be NULL) = d loss[0] / d prob. */
int grl_pair_bce(const float* prob, const int64_t* tar_probe, const int64_t* tar_gallery, int n,
                 float* loss, float* prec, float* dprob, void* stream);
/* y = alpha * g[0] * x with g a device scalar (chains an upstream loss gradient without a host sync) */
int grl_scale_dev(const float* x, const float* g, float alpha, float* y, int64_t n, void* stream);

/* per-query ranking metrics of eva_functions.evaluate (reid/evaluator/eva_functions.py:134-184)
 * over a row-wise argsort (grl_row_argsort): gallery entries with the query's pid AND camera are
 * dropped; first_hit[q] = 0-based rank of the first match among the kept entries (-1: the
 * identity never appears, the query is skipped upstream), n_hits[q] = matches kept,
 * ap[q] = (1/n_hits) sum over hits of (hits so far)/(rank+1) in fp64.  CMC[r] = mean over valid
 * queries of [first_hit <= r]; mAP = mean of ap over valid queries (host, nq numbers). */
int grl_rank_metrics(const int32_t* idx, int64_t ld, const int32_t* q_pids, const int32_t* q_cams,
                     const int32_t* g_pids, const int32_t* g_cams, int nq, int ng, int32_t* first_hit,
                     int32_t* n_hits, double* ap, void* stream);

/* ---- gallery search and exact ranking metrics over column blocks (search.hip, engine.search /
 * engine.rank_metrics_streaming).  ``d`` is a column block [nq][ld] (ncols used) of the query x gallery
 * distance matrix whose first column is gallery entry col0.  Order: that of grl_row_argsort (canonical NaN,
 * -0 -> +0, ascending, ties to the smaller gallery index); an entry is the composite (key << 32) | index. */
/* running top-k per query: run_key [nq][k] (composites, sorted; initialised to all-ones = empty) and run_val
 * [nq][k] (the distances' own bits; initialised to +inf) become the first k of their union with the block.
 * cidx (may be NULL) [nq][ldc] gives each column's gallery index (< 0: skipped) instead of col0 + column.
 * k <= 1024 (GRL_EUNSUPPORTED beyond). */
int grl_topk_block(const float* d, int64_t ld, const int32_t* cidx, int64_t ldc, int nq, int ncols, int col0, int k,
                   uint64_t* run_key, float* run_val, void* stream);
/* grl_topk_block that skips junk as eva_functions.evaluate does: a column whose gallery index g (col0 + column, or
 * cidx[q][column]) has g_pids[g] == q_pids[q] && g_cams[g] == q_cams[q] is skipped as cidx < 0 is.  q_pids / q_cams
 * [nq]; g_pids / g_cams are indexed by the gallery index, so they cover the whole gallery, not the block.  Order,
 * padding and the limit on k are grl_topk_block's. */
int grl_topk_block_filtered(const float* d, int64_t ld, const int32_t* cidx, int64_t ldc, int nq, int ncols, int col0,
                            int k, uint64_t* run_key, float* run_val, const int32_t* q_pids, const int32_t* q_cams,
                            const int32_t* g_pids, const int32_t* g_cams, void* stream);
/* candidates of query q = gallery entries with its pid: q_slot[q] indexes the CSR pid_ptr / pid_list (ascending
 * gallery indices per pid; -1 = the pid is not in the gallery).  The keys of those inside the block go to
 * cand_key[cand_off[q] + j] (j = position in the pid's list). */
int grl_match_gather(const float* d, int64_t ld, int nq, int col0, int ncols, const int32_t* q_slot,
                     const int32_t* pid_ptr, const int32_t* pid_list, const int64_t* cand_off, uint32_t* cand_key,
                     void* stream);
/* keep the candidates from another camera (same pid AND camera = junk) and sort them: match_key[cand_off[q] + i],
 * i < n_match[q].  max_list = longest pid list, at most 8192 (GRL_EUNSUPPORTED beyond). */
int grl_match_sort(int nq, const int32_t* q_slot, const int32_t* pid_ptr, const int32_t* pid_list,
                   const int32_t* q_cams, const int32_t* g_cams, const int64_t* cand_off, const uint32_t* cand_key,
                   int max_list, uint64_t* match_key, int32_t* n_match, void* stream);
/* for each non-match g (another pid) of the block, p(g) = matches strictly before g; hist[cand_off[q] + p] += 1
 * for p < n_match[q] (integer atomics; hist zero-filled by the caller).  max_match = max over q of n_match. */
int grl_rank_count_block(const float* d, int64_t ld, int nq, int col0, int ncols, const int32_t* q_pids,
                         const int32_t* g_pids, const int64_t* cand_off, const uint64_t* match_key,
                         const int32_t* n_match, int max_match, int32_t* hist, void* stream);
/* rank_i = i + sum_{p <= i} hist[p]: first_hit / n_hits / ap as grl_rank_metrics gives them (ap summed in
 * ascending i, fp64) */
int grl_rank_finish(int nq, const int64_t* cand_off, const int32_t* n_match, const int32_t* hist,
                    int32_t* first_hit, int32_t* n_hits, double* ap, void* stream);

/* ---- pair-level (verification) histograms of a distance block (roc.hip, engine.pair_roc) ----
 * ``d`` [nq][ld] (ncols used) is a column block as above.  Entry (q, j), gallery index g = col0 + j: dropped when
 * g_pids[g] == q_pids[q] && g_cams[g] == q_cams[q] (junk), positive when only the pids agree, negative otherwise.
 * key = order-preserving uint32 of the float32 (-0 -> +0; sign clear: bits ^ 0x80000000, else ~bits; NaN of either
 * sign: 0xffffffff); bin = key >> (32 - bits); pos_hist / neg_hist [2^bits] int64 += 1 (integer atomics; zero-filled
 * by the caller before the first block, accumulated over blocks).  g_pids / g_cams are indexed by the gallery index.
 * Any ld >= ncols, ncols >= 1, nq >= 0; 16-byte loads when d and ld allow.  GRL_EINVAL: bits outside 8..20, a null
 * pointer, a negative size.  A workgroup counts in 32-bit LDS slots and handles at most 1024 * ceil(nq / row groups)
 * entries; GRL_EUNSUPPORTED if that could reach 2^32 (nq >= 2^22 in one call). */
int grl_pair_hist_block(const float* d, int64_t ld, int nq, int col0, int ncols, const int32_t* q_pids,
                        const int32_t* q_cams, const int32_t* g_pids, const int32_t* g_cams, int bits,
                        int64_t* pos_hist, int64_t* neg_hist, void* stream);

/* ---- DBSCAN over column blocks (cluster.hip, engine.eps_graph / cluster / cluster_from_graph) ----
 * The eps-graph of n samples as a CSR, without the n x n matrix.  ``d`` [nrows][ld] (ncols used) is a block of the
 * distance matrix: its row r is sample row0 + r, its column j is sample col0 + j.  Edge i -> j iff i != j and
 * d <= eps (a NaN never passes; eps = +inf is taken as FLT_MAX, the block's own infinities are compared as they are).
 * Count pass (row_ptr = col = NULL): cnt[row0 + r] += the row's edges in the block.  Fill pass (row_ptr [n+1] from
 * grl_rrs_scan of the counts, col [E]): the column indices go to col[row_ptr[i] + cnt[i] ..] in ascending order and
 * cnt[i] += their number, so cnt (int32 [n], zeroed by the caller before each pass) is the row's cursor and the
 * blocks of a pass must be enqueued in ascending column order on one stream, every row at most once per call.  No
 * atomics: col is the same bit for bit on every run.  16-byte loads when d and ld allow, single floats otherwise.
 * GRL_EINVAL: a null pointer, a negative size, ncols < 1, ld < ncols, a NaN eps, row_ptr without col or col without
 * row_ptr. */
int grl_cluster_edges_block(const float* d, int64_t ld, int nrows, int row0, int col0, int ncols, float eps,
                            int32_t* cnt, const int64_t* row_ptr, int32_t* col, void* stream);
/* core[i] = deg[i] + 1 >= min_samples (a point counts itself), parent[i] = i, border[i] = INT32_MAX.
 * GRL_EINVAL: min_samples < 1, n < 0, a null pointer with n > 0. */
int grl_cluster_init(const int32_t* deg, int n, int min_samples, uint8_t* core, int32_t* parent, int32_t* border,
                     void* stream);
/* One round of connected components over the core points of a CSR (row_ptr [n+1] int64, col int32 in 0..n-1, any
 * order, duplicates and self-loops allowed; an edge stored in one direction joins both ends): every stored edge with
 * two core ends and two different roots hooks the larger root under the smaller (atomicMin) and sets *changed to 1,
 * then every core node points at its root.  The caller zeroes *changed and repeats until a round leaves it 0: then
 * parent[i] of a core point is the smallest core index of its component.  parent of a non-core point stays i. */
int grl_cluster_round(const int64_t* row_ptr, const int32_t* col, const uint8_t* core, int32_t* parent, int n,
                      int32_t* changed, void* stream);
/* after convergence: border[j] = the smallest root among the core points adjacent to the non-core point j through an
 * edge stored in either direction (INT32_MAX: none, noise) */
int grl_cluster_border(const int64_t* row_ptr, const int32_t* col, const uint8_t* core, const int32_t* parent, int n,
                       int32_t* border, void* stream);
/* is_root[i] = core[i] && parent[i] == i (int32, for grl_rrs_scan: root_id [n+1], root_id[n] = the cluster count) */
int grl_cluster_roots(const uint8_t* core, const int32_t* parent, int n, int32_t* is_root, void* stream);
/* labels[i] = root_id[parent[i]] (core), root_id[border[i]] (border point), -1 (noise): ids ascend with the root */
int grl_cluster_labels(const uint8_t* core, const int32_t* parent, const int32_t* border, const int64_t* root_id, int n,
                       int64_t* labels, void* stream);

/* ---- eps-graph of the k-reciprocal Jaccard distance of one sample set (jaccard.hip, engine.jaccard_graph /
 * cluster_jaccard) ----
 * row_ptr_v2 / col_v2 / val_v2: V2 of all n samples as CSR (grl_rrs_expand: ascending columns, no zeros, at most 2048
 * entries a row); csc_ptr / csc_row / csc_val: its transpose over ALL rows (grl_rrs_transpose with nq = 0).
 * t[i][j] = the fp32 sum over row i's entries k, ascending, of min(V2[i][k], V2[j][k]); J = 1 - t / (2 - t); edge
 * i -> j iff j != i and J <= eps.  Count pass (out_row_ptr = out_col = out_val = NULL): cnt[i] = the edges of row i.
 * Fill pass (out_row_ptr [n+1] = grl_rrs_scan of cnt): out_col gets every row's columns in ascending order and
 * out_val, when not NULL, their J.  ``window`` = columns of a row whose sums are held in LDS at a time: 0 (the
 * library's choice, 8192) or a multiple of 256 up to 8192; the result does not depend on it.  No float atomics: the
 * same bits on every run.  GRL_EINVAL, before any launch: a null pointer, n < 2, eps not finite or >= 1, a window that
 * is negative, no multiple of 256 or above 8192, cnt missing in the count pass, out_col missing in the fill pass. */
int grl_jaccard_edges(const int64_t* row_ptr_v2, const int32_t* col_v2, const float* val_v2, const int64_t* csc_ptr,
                      const int32_t* csc_row, const float* csc_val, int n, float eps, int window, int32_t* cnt,
                      const int64_t* out_row_ptr, int32_t* out_col, float* out_val, void* stream);

/* ---- k-means and cluster centroids (kmeans.hip, engine.kmeans / kmeans_assign / cluster_centroids) ----
 * The assignment is grl_topk_block at k = 1 over column blocks of the sample x centroid distance matrix; these entry
 * points are the update.  Integer atomics only: every output is the same bit for bit on every run.
 * labels[i] = the index in run_key[i] (the k = 1 composite of sample i), or -1 when run_val[i] is NaN, the slot is
 * empty or the index is outside 0..k-1; counts[label] += 1 (int32 [k], zeroed by the caller); *changed += the number
 * of labels that differ from prev_labels (NULL: every label counts). */
int grl_kmeans_relabel(const uint64_t* run_key, const float* run_val, int n, int k, const int32_t* prev_labels,
                       int32_t* labels, int32_t* counts, int32_t* changed, void* stream);
/* counts[l] += 1 for every label l in 0..k-1 (others belong to nobody); counts zeroed by the caller */
int grl_kmeans_label_counts(const int32_t* labels, int n, int k, int32_t* counts, void* stream);
/* The clusters' member lists as a CSR: mptr [k+1] = grl_rrs_scan of the counts, mem [mptr[k]] (allocated for n) =
 * every cluster's samples in ASCENDING order.  cursor [k] int32 zeroed by the caller, tmp int32 [n] scratch.  A slot
 * is taken by an integer atomic; the final place of a sample is the number of its cluster's samples below it, so mem
 * does not depend on the order of arrival. */
int grl_kmeans_members(const int32_t* labels, int n, int k, const int64_t* mptr, int32_t* cursor, int32_t* tmp,
                       int32_t* mem, void* stream);
/* sum[j][c] (row stride lds) = the sum of x[m][c] (x [n][ld]) over cluster j's members m = mem[mptr[j] .. mptr[j+1]),
 * in this fixed order: four partial sums p_w, w = 0..3, each the sequential fp32 sum from +0.0f of the members
 * m_w, m_{w+4}, m_{w+8}, .. (positions in the list), then (p0 + p1) + (p2 + p3).  Adds only, no atomics.  One
 * workgroup per (cluster, 256 columns); 16-byte loads when x is 16-byte aligned and ld and d are multiples of 4,
 * single floats otherwise.  Entries of mem outside 0..n-1 and list positions at or beyond nmem are skipped. */
int grl_segment_rowsum(const float* x, int64_t ld, int n, const int64_t* mptr, const int32_t* mem, int64_t nmem, int k,
                       int d, float* sum, int64_t lds, void* stream);
#define GRL_KMEANS_SUM  0
#define GRL_KMEANS_MEAN 1
#define GRL_KMEANS_UNIT 2
/* out[j] = sum[j] (SUM), sum[j] / float(counts[j]) (MEAN), sum[j] * (1 / sqrt(sq[j])) (UNIT; sq = grl_row_sqnorm of
 * sum).  A cluster with counts[j] == 0, or (UNIT) with sq[j] zero or not finite, is empty: out[j] = prev[j] (row
 * stride ldp) or zeros when prev is NULL, and *empty += 1 (int32, zeroed by the caller).  Plain stores. */
int grl_kmeans_finish(const float* sum, int64_t lds, const int32_t* counts, const float* sq, const float* prev,
                      int64_t ldp, int k, int d, int reduce, float* out, int64_t ldo, int32_t* empty, void* stream);

/* ---- silhouette coefficients over column blocks (silhouette.hip, engine.silhouette / silhouette_matrix) ----
 * Member order: mem [m] int32 holds cluster 0's samples in ascending sample index, then cluster 1's, ..; mptr [k+1]
 * int64, mptr[c] = the first position of cluster c, mptr[k] = m (grl_kmeans_label_counts, grl_rrs_scan,
 * grl_kmeans_members).  labels int32 [n]: a sample whose label is outside 0..k-1 is nobody's -- it is not in mem, and
 * its row is skipped.  ``d`` [nrows][ld] (ncols used) is a block of the distance matrix: row r is sample row0 + r,
 * column j is POSITION c0 + j of the member order, that is sample mem[c0 + j]; columns at or beyond mptr[k] are ignored.
 * Distance of an entry: the value of d as it is (rinv_row = rinv_pos = NULL), or, with rinv_row [n] and rinv_pos [m]
 * (= rinv_row[mem[p]]) given, the cosine form of d = -dot: v = (d * rinv_row[i]) * rinv_pos[p], dist = 1.0f + v,
 * dist < 0 ? 0 : dist -- single fp32 operations, no fma; a NaN stays NaN.
 * Sum of row i towards cluster c, in this fixed order whatever the block cuts: 64 partial sums, partial l = the
 * sequential fp32 sum from +0.0f, in ascending position, of the distances at the cluster's positions p with
 * p % 64 == l, the position with mem[p] == i left out (by index, not by value); then part[l] += part[l + s], l < s, for
 * s = 32, 16, 8, 4, 2, 1.  mean = sum / float(count), count = n_c - 1 for the row's own cluster (n_c = 1: a = 0) and
 * n_c otherwise.  a[i] = the own cluster's mean; bmin[i] = the minimum of the other non-empty clusters' means (-0 below
 * +0; from +inf), NaN as soon as one of them is NaN.  Adds only, no atomics of any kind: the same bits on
 * every run and for every block width.
 * State between the blocks of a pass, all float32: part [n][64] (the lane partials of the one cluster that straddles
 * the block edge), a [n], bmin [n]; none needs initialising -- the block with c0 == 0 starts them.  The blocks of a
 * pass are enqueued in ascending position order on one stream, every row at most once per call.  One wave per row.
 * GRL_EINVAL, before any launch: a null pointer, a negative size, k < 1, ncols < 1, ld < ncols, one of rinv_row /
 * rinv_pos without the other. */
int grl_silhouette_block(const float* d, int64_t ld, int nrows, int row0, int64_t c0, int ncols, const int32_t* mem,
                         const int64_t* mptr, int k, const int32_t* labels, const float* rinv_row,
                         const float* rinv_pos, float* part, float* a, float* bmin, void* stream);
/* After the last block: s[i] = 0 for a sample that is nobody's (a = bmin = 0 are stored) or whose cluster has one
 * member (counts[label] <= 1; a = 0 is stored: scikit-learn's rule), NaN when a or bmin is NaN, 0 when max(a, bmin)
 * == 0, otherwise (bmin - a) / max(a, bmin), both operations rounded.  counts int32 [k] = the clusters' sizes. */
int grl_silhouette_finish(float* a, float* bmin, const int32_t* labels, const int32_t* counts, int n, int k, float* s,
                          void* stream);
/* rinv[i] = 1.0f / sqrtf(sq[i]) (sq = grl_row_sqnorm), both correctly rounded: the factors of the cosine form */
int grl_silhouette_rinv(const float* sq, int n, float* rinv, void* stream);

/* ---- HDBSCAN: the mutual-reachability minimum spanning forest over column blocks (hdbscan.hip,
 * engine.mutual_reachability_mst / hdbscan / hdbscan_matrix) ----
 * ``d`` [nrows][ld] (ncols used) is a block of the n x n distance matrix: row r is sample row0 + r, column c is sample
 * c0 + c.  Distance of the pair {lo < hi}: the entry as it is (rinv = NULL; the matrix must be symmetric bit for bit),
 * or, with rinv [n] (grl_silhouette_rinv) given, the cosine form of d = -dot made symmetric: v = (d * rinv[lo]) *
 * rinv[hi], the smaller index first whichever of the two is the row, dist = 1.0f + v, dist < 0 ? 0 : dist (a NaN stays).
 * Edge weight: w = dist; if (core[lo] > w) w = core[lo]; if (core[hi] > w) w = core[hi], with core [n] the core
 * distances.  A sample whose core distance is not finite has no edges, and a w that is NaN or +inf is no edge.
 * One Boruvka round: for every row i, (best_w[i], best_j[i]) = the smallest (w, j) -- w by float <, then j -- over the
 * columns j with comp[j] != comp[i] (comp int32 [n]: the component ids; this skips j == i), or (+inf, -1) when there is
 * none.  The block with c0 == 0 starts the pair, every later block folds into it, so the blocks of a round are enqueued
 * in ascending order on one stream, every row at most once per call; the result does not depend on the cuts.  One wave
 * per row, no atomics.  GRL_EINVAL, before any launch: a null pointer (rinv may be NULL), a negative size, ncols < 1,
 * ld < ncols, row0 + nrows > n or c0 + ncols > n. */
int grl_hdbscan_minedge_block(const float* d, int64_t ld, int n, int nrows, int row0, int c0, int ncols,
                              const float* core, const int32_t* comp, const float* rinv, float* best_w, int32_t* best_j,
                              void* stream);
/* The cosine form above applied to a block of d = -dot in place (before grl_topk_block ranks it for the core
 * distances): d[r][c] = max(0, 1.0f + (d[r][c] * rinv[lo]) * rinv[hi]) for the pair {row0 + r, c0 + c}. */
int grl_hdbscan_cosine_block(float* d, int64_t ld, int n, int nrows, int row0, int c0, int ncols, const float* rinv,
                             void* stream);

/* ---- t-SNE: the 2-d map of a feature set (tsne.hip, engine.tsne / tsne_affinities / tsne_gradient /
 * tsne_from_affinities) ----
 * THE WAVE ORDER of a sum over positions p = 0, 1, ..: 64 partial sums, partial l the sequential fp32 sum from +0.0f, in
 * ascending p, of the terms with p % 64 == l (a term that is left out is skipped); then part[l] += part[l + s], l < s,
 * for s = 32, 16, 8, 4, 2, 1.  Every sum of this section runs in it, every operation is rounded to fp32 on its own, a
 * division is IEEE's.  One wave per row, no atomics, no LDS: the same bits on every run and for every launch geometry.
 * d[r][c] = d[r][c] * d[r][c] in place on a block [nrows][ld] (ncols used): the squared distance of 'euclidean'. */
int grl_tsne_square_block(float* d, int64_t ld, int nrows, int ncols, void* stream);
/* The conditional affinities of every row of e [n][K] (the distances to its K neighbours, 1 <= K <= 1023) by
 * scikit-learn's bisection on beta, on the distances less the list's first, t_k = e_k - e_0 (the list ascends; the
 * same p and H as on e_k, without the underflow of every term at once that fp32 meets at e beta > 87): beta = 1, at
 * most 100 steps of  p_k = expf(-(t_k * beta)), S = sum p_k, p_k = p_k / S, H = logf(S) + beta * sum(t_k * p_k)  (both
 * sums in the wave order over k), stop when
 * |H - log_perplexity| <= 1e-5f, otherwise H too large: beta doubles, or halves the way to the upper bound once there is
 * one; H too small: beta halves, or halves the way to the lower bound.  cond [n][K] = the p_k of the last step, beta [n]
 * its beta.  A row with a distance that is not finite is ISOLATED: isolated[i] = 1 (0 otherwise), cond = +0, beta = NaN. */
int grl_tsne_perplexity(const float* e, int n, int K, float log_perplexity, float* cond, float* beta, uint8_t* isolated,
                        void* stream);
/* Row i of the joint affinities as a CSR over the union pattern.  acol / aval [n][K]: row i of the conditional matrix,
 * columns ASCENDING, entries with a column < 0 (in front) are none; csc_ptr / csc_row / csc_val: its transpose
 * (grl_rrs_transpose with nq = 0: column i's rows ascending).  P[i][j] = (a + b) / den, a = the row's value at j or +0,
 * b = the column's value at j or +0.  Count pass (row_ptr = NULL): cnt[i] = the entries of row i.  Fill pass (row_ptr
 * [n+1] = grl_rrs_scan of cnt): col ascending, every pair once per direction, val.  A row may hold up to n - 1 entries. */
int grl_tsne_joint(const int32_t* acol, const float* aval, int K, const int64_t* csc_ptr, const int32_t* csc_row,
                   const float* csc_val, int n, float den, const int64_t* row_ptr, int32_t* cnt, int32_t* col, float* val,
                   void* stream);
/* The exact repulsive term at y [n][2] (8-byte aligned).  For the pair (i, j): dx = y[i] - y[j], r = dx0 * dx0 + dx1 *
 * dx1, q = 1.0f / (1.0f + r).  rep[i] = sum over j of (q * q) * dx, rowz[i] = sum over j of q, both in the wave order
 * over the position j, j = i and the isolated j (isolated [n] uint8, NULL = none) left out; an isolated i gets zeros. */
int grl_tsne_repulsion(const float* y, const uint8_t* isolated, int n, float* rep, float* rowz, void* stream);
/* z[0] = the sum of rowz [n] in the wave order over the position i: one wave, whatever n */
int grl_tsne_z(const float* rowz, int n, float* z, void* stream);
/* att[i] = sum over the entries p of CSR row i (wave order over the place in the row, entries towards an isolated
 * sample left out) of ((alpha * val[p]) * q) * dx; g = 4.0f * (att - rep[i] / z[0]); grad[i] = g when grad is not NULL
 * (an isolated i: +0).  With update [n][2] given, scikit-learn's step per coordinate: gains = update * g < 0 ? gains +
 * 0.2f : gains * 0.8f, at least 0.01f; update = momentum * update - learning_rate * (gains * g); y_out[i] = y[i] +
 * update (an isolated i: y_out[i] = y[i], gains and update untouched).  y_out must not be y: other rows read y. */
int grl_tsne_update(const int64_t* row_ptr, const int32_t* col, const float* val, const float* y, const uint8_t* isolated,
                    int n, float alpha, const float* rep, const float* z, float* grad, float* gains, float* update,
                    float* y_out, float momentum, float learning_rate, void* stream);
/* rowkl[i] = sum over the entries of CSR row i with val > 0 (wave order over the place in the row, isolated ends left
 * out) of val * (float)log((double)((val * z[0]) / q)) -- the fp32 logarithm correctly rounded, by way of fp64 -- : the
 * row's share of the Kullback-Leibler divergence */
int grl_tsne_kl(const int64_t* row_ptr, const int32_t* col, const float* val, const float* y, const uint8_t* isolated,
                int n, const float* z, float* rowkl, void* stream);

/* ---- PCA: the small dense linear algebra of the randomised subspace iteration (pca.hip, engine.pca / pca_eigh /
 * pca_orthonormalize) ----
 * The tall products of a fit are grl_conv_gemm_f32 and grl_conv_wgrad_f32 in GRL_MATH_F32; these entry points work on
 * matrices of L <= GRL_PCA_LMAX rows.  A factorisation is one workgroup (no grid-wide barrier, no cooperative launch),
 * every loop is bounded at launch, every operation is rounded to fp32 on its own, divisions and square roots are IEEE's,
 * no atomics: the same bits on every run. */
#define GRL_PCA_LMAX 512
#define GRL_PCA_MAX_SWEEPS 30
#define GRL_PCA_PIVOT_SMALL 1        /* a pivot <= rel_tol * (its own diagonal entry of G): the row depends on the rows before it in fp32 */
#define GRL_PCA_PIVOT_NONFINITE 2    /* a pivot (or the largest diagonal entry) that is NaN or infinite */
/* The pivot record of grl_pca_cholesky, STICKY over calls: the caller sets {+inf, 0, -1, -1, 0} once and reads it back
 * after the last call.  min_pivot: the smallest pivot / (largest diagonal entry of that call's input) met so far, a
 * failing pivot included; status / index / call: 0, or the kind, the pivot index and the call number (from 0) of the
 * FIRST failure; calls: how many factorisations the record has seen. */
typedef struct GrlPcaRecord {
    float   min_pivot;
    int32_t status, index, call, calls;
    int32_t reserved[3];
} GrlPcaRecord;
/* G = R R^T in place on the lower triangle of g [L][ldg] (the strict upper triangle is neither read nor written):
 * R[i][k] = (G[i][k] - sum_{j<k} R[i][j] * R[k][j]) / R[k][k], R[k][k] = sqrtf(G[k][k] - sum_{j<k} R[k][j] * R[k][j]), each
 * sum term by term in ascending j from the G entry.  A pivot that is not finite or not > rel_tol * G[k][k] (the entry it
 * started from: the test does not depend on the scale of the rows) ENDS the
 * factorisation and is recorded: its column and all later ones are set to the identity's, so grl_pca_trsm stays finite on
 * finite input.  One workgroup of 1024, the panel of 32 columns in LDS (2 * L * 33 floats of dynamic LDS). */
int grl_pca_cholesky(float* g, int ldg, int L, float rel_tol, GrlPcaRecord* record, void* stream);
/* W <- R^-1 W for w [L][ldw] (m columns used) and the lower triangle R of r [L][ldr]: forward substitution, y_i = (w_i -
 * sum_{k<i} R[i][k] * y_k) / R[i][i], the sum term by term in ascending k; one lane per column of W. */
int grl_pca_trsm(const float* r, int ldr, float* w, int64_t ldw, int L, int m, void* stream);
typedef struct GrlPcaEighInfo {
    int32_t sweeps;      /* sweeps that rotated at least one pair (<= GRL_PCA_MAX_SWEEPS) */
    float   off;         /* the Frobenius norm of the off-diagonal part that is left */
    float   fro;         /* the Frobenius norm of the input */
    int32_t reserved;
} GrlPcaEighInfo;
/* Cyclic Jacobi on the symmetric a [L][lda] (the upper triangle is read; a is destroyed): lam [L] descending (equal ones by
 * their original index, a NaN last), vt [L][ldvt] with row i the unit eigenvector of lam[i]; vt_work [L][ldv] is scratch.
 * Round-robin pairing (pca.hip), so the rotation order depends on L alone; a pair with |a_pq| <= (|a|_F * 2^-26) / L is
 * passed over; the loop ends after the first sweep without a rotation or after GRL_PCA_MAX_SWEEPS.  Converged means
 * info->off <= 2^-26 |a|_F.  A 1 x 1 or diagonal input: no rotation, sweeps = 0.  One workgroup of 1024. */
int grl_pca_eigh(float* a, int lda, float* vt_work, int ldv, int L, float* lam, float* vt, int ldvt, GrlPcaEighInfo* info,
                 void* stream);
/* out[i] = the sum of the m used columns of row i of w [rows][ld] in the wave order (the t-SNE section above) over the column */
int grl_pca_rowsum(const float* w, int64_t ld, int rows, int m, float* out, void* stream);
/* w[i][j] = w[i][j] - s[i] * mu[j] on w [rows][ld] (m columns used): the rank-one term of a product with centred rows */
int grl_pca_rank1(float* w, int64_t ld, int rows, int m, const float* s, const float* mu, void* stream);
/* every row of c [rows][ld] (d used) whose entry of largest magnitude -- the lowest column among equals -- is negative is
 * multiplied by -1 */
int grl_pca_sign(float* c, int64_t ld, int rows, int d, void* stream);
/* scale[i] = lam ? 1.0f / sqrtf(lam[i]) : 1.0f; shift[i] = -(cm[i] * scale[i]), i < r: the epilogue of the transform GEMM */
int grl_pca_affine(const float* cm, const float* lam, int r, float* scale, float* shift, void* stream);
/* out[i][j] = y[i][j] * sqrtf(lam[j]) (the whitening undone), y [rows][ldy], out [rows][ldo], r columns */
int grl_pca_colscale(const float* y, int64_t ldy, int rows, int r, const float* lam, float* out, int64_t ldo, void* stream);
/* scikit-learn's init='pca' of t-SNE: out [rows][2] = y[i][0..1] / sqrtf(var) * 1e-4f, var = sum_i (y[i][0] - mean)^2 / rows,
 * mean = sum_i y[i][0] / rows; both sums: 1024 partial sums by i % 1024, each sequential from +0.0f, folded part[t] +=
 * part[t + s], s = 512 .. 1.  One workgroup. */
int grl_pca_tsne_init(const float* y, int64_t ldy, int rows, float* out, void* stream);

/* ---- query expansion / database-side augmentation (expand.hip, engine.expand_from_lists / expand_features) ----
 * out[i] = (x[i] + sum_p w_p * bank[j_p]) / (1 + sum_p w_p): a gather and a weighted sum over feature rows, without
 * the n x m x d tensor of bank[idx].  x [n][ldx], bank [nb][ldb], out [n][ldo] fp32 (d used); idx int64 / dist fp32
 * [n][ldl] (L used) are the neighbour lists of grl_topk_block as engine.search returns them (index -1 = padding).
 * Kept neighbours of row i: walk the list left to right, skip idx < 0 (and idx >= nb), with skip_self skip idx == i
 * (n == nb then), keep the first m that remain -- fewer may.  Weight: s = dist < 0 ? -dist : 0 (NaN -> 0; for the
 * 'cosine' lists dist = -dot); alpha == 0: w = 1; alpha in 1..8: w = s, then alpha - 1 times w = w * s.  Per element,
 * in exactly this order: acc = x[i][e], wsum = 1; per kept neighbour in list order acc = acc + (w * bank[j][e])
 * (product rounded, then the sum: no fma) and wsum = wsum + w; out[i][e] = acc / wsum, correctly rounded.  A NaN
 * result is stored as 0x7fc00000.  tests/expand_ref.py is this paragraph in numpy float32, bit for bit.
 * Any d, leading dimensions >= d; 16-byte accesses when every pointer and leading dimension allows them.
 * GRL_EINVAL: m < 1, m > L, alpha outside 0..8, out overlapping x or bank (DBA reads the bank it replaces), skip_self
 * with n != nb; GRL_EUNSUPPORTED: m > 4096. */
int grl_expand_rows(const float* x, int64_t ldx, const float* bank, int64_t ldb, const int64_t* idx, const float* dist,
                    int64_t ldl, int n, int nb, int d, int L, int m, int alpha, int skip_self, float* out, int64_t ldo,
                    void* stream);

/* ---- diffusion (manifold ranking) on the gallery's mutual-kNN graph (diffusion.hip, engine.diffusion_graph /
 * diffusion_solve / diffusion_search) ----
 * The graph is a fixed-width ELL layout: idx int32 / S fp32 [n][ldg] (k used, 1 <= k <= 128).  The solver's state is
 * [n][B] fp32, node-major, the B query columns of a node contiguous.  Every operation is one of + - x / sqrt, correctly
 * rounded, no fma; every sum has a prescribed order; tests/diffusion_ref.py is this section in numpy float32, bit for bit.
 * Dot products over the rows: a wave sums 16 consecutive rows in row order from +0, a workgroup adds its 4 wave sums in
 * wave order into one partial per grl_diffusion_part_rows() = 64 rows, the partials are added in row order from +0.
 *
 * grl_diffusion_mutual: sidx int64 / sdist fp32 [n][ldl] hold the k + 1 entries per row of engine.search(gf, gf, k + 1)
 * by cosine (distinct indices, -1 = padding).  Slot t of row i is list position t + (t >= selfpos), selfpos = the first
 * position that holds i (k when there is none: the last entry is dropped); an index outside [0, n), or a further entry
 * equal to i, is padding (idx -1).  w = s, then gamma - 1 times w = w * s, s = dist < 0 ? -dist : 0 (gamma in 1..8).
 * a[i][t] = min(w_ij, w_ji), j = idx[i][t], if i occurs in row j's list at a position that row j keeps (its first
 * occurrence counts), else 0; deg[i] = a[i][0] + a[i][1] + ... from +0; weight[i][t] = a / (sqrt(deg[i]) * sqrt(deg[j])),
 * 0 where a is 0.  Columns of idx / weight beyond k are left untouched. */
int grl_diffusion_mutual(const int64_t* sidx, const float* sdist, int64_t ldl, int n, int k, int gamma, int32_t* idx,
                         float* weight, int64_t ldo, float* deg, void* stream);
int grl_diffusion_part_rows(void);
/* Ap[i][b] = p[i][b] - (alpha * acc), acc = the sum over the slots t with S[i][t] != 0 (and 0 <= idx[i][t] < n) in slot
 * order from +0 of S[i][t] * p[idx[i][t]][b].  part [ceil(n / 64)][B] = the partials of p . Ap per column (see above).
 * Ap must not be p.  16-byte accesses when B % 4 == 0, B >= 256 and both pointers allow them. */
int grl_diffusion_apply(const int32_t* idx, const float* S, int64_t ldg, int n, int k, const float* p, int B, float alpha,
                        float* Ap, float* part, void* stream);
/* y [n][B] = 0, then per column q and entry t < kq in list order y[seed_idx[q][t]][q] = v (gamma == 0) or
 * max(-v, 0)^gamma by gamma - 1 products (gamma in 1..8: v is search's cosine distance), v = seed_val[q][t]; an index
 * outside [0, n) is padding.  seed_idx int64 / seed_val fp32 [B][lds]. */
int grl_diffusion_seed(const int64_t* seed_idx, const float* seed_val, int64_t lds, int B, int kq, int n, int gamma,
                       float* y, void* stream);
/* Plain conjugate gradients on (I - alpha S) x = y per column: x0 = 0, r0 = p0 = y, exactly n_iter iterations of
 *   Ap (grl_diffusion_apply), a = rr / (p . Ap), x = x + (a * p), r = r - (a * Ap), b = rr' / rr, p = r + (b * p)
 * with rr = r . r reduced as above.  A column whose rr is not a positive finite number, or whose p . Ap is <= 0 or not
 * finite, freezes: its x, r and p are no longer written.  y is overwritten (it becomes r); x [n][B] is the result; ws holds
 * grl_diffusion_workspace_floats(n, B) floats, 16-byte aligned.  alpha in [0, 1), n_iter >= 0 (0: x = 0). */
int64_t grl_diffusion_workspace_floats(int n, int B);
int grl_diffusion_solve(const int32_t* idx, const float* S, int64_t ldg, int n, int k, float* y, int B, float alpha,
                        int n_iter, float* x, float* ws, void* stream);
/* out [B][ldo] (n used) = x [n][B] transposed, negated when negate != 0: the rows grl_topk_block / grl_row_argsort rank */
int grl_diffusion_transpose(const float* x, int n, int B, int negate, float* out, int64_t ldo, void* stream);

/* ---- tracklet set distances from a block of clip distances (setdist.hip, engine.set_dist / set_search /
 * set_metrics_streaming / set_pair_roc) ----
 * A tracklet set is its clips' rows and a ptr array, int64 [n + 1]: tracklet t owns the clips ptr[t] .. ptr[t + 1].
 * ``e`` [rows][ld] is a block of the clip x clip distance matrix as the distance GEMM wrote it (GRL_EPI_NEGDOT or
 * GRL_EPI_EUCLID): row r is query clip qptr[a0] + r, column c is gallery clip gptr[b0] + c, for the query tracklets
 * a0 .. a0 + na (qptr[a0 + na] - qptr[a0] rows) and the gallery tracklets b0 .. b0 + nb.  out[a - a0][b - b0] (row
 * stride ldo) is the set distance of the pair.  With e[i][j], i < m, j < p, the cell of a pair, rowmin[i] = min_j e[i][j]
 * and colmin[j] = min_i e[i][j]:
 *   GRL_SET_MIN        min_i rowmin[i]                                            (the closest clip pair)
 *   GRL_SET_MEAN       sum_ij e[i][j] / float(m * p)
 *   GRL_SET_CHAMFER    0.5f * (sum_i rowmin[i] / float(m) + sum_j colmin[j] / float(p))
 *   GRL_SET_HAUSDORFF  max(max_i rowmin[i], max_j colmin[j])
 * min and max are exact selections in the total order of the floats with -0 below +0 (grl_silhouette_block's bmin).  A
 * NaN anywhere in the cell makes the cell the canonical NaN (0x7fc00000) under all four, and so does a sum that is NaN.
 * The two sums of CHAMFER: sequential fp32 from +0.0f in ascending index, then the two divisions, one add, one multiply,
 * each rounded (no fma).  The sum of MEAN: W = 64 for p > 32, else the smallest power of two >= p; R = 64 / W; 64
 * partials, partial l = the sequential fp32 sum from +0.0f of the elements (i, j) with (i % R) * W + j % 64 == l, in
 * ascending j / 64, then ascending i; then part[l] += part[l + s], l < s, for s = 32, 16, 8, 4, 2, 1
 * (grl_silhouette_block's tree); one division.  Adds only, no atomics of any kind.  Every order depends on (m, p) alone --
 * not on where the scratch was cut, on the launch or on the other tracklets of the block -- so a cell has the same bits
 * on every run and for every blocking; tests/setdist_ref.py is this paragraph in numpy float32, bit for bit.
 * The ptr arrays are passed twice: ``qptr_host`` / ``gptr_host`` are read by the argument checks, ``qptr`` / ``gptr`` are
 * the same values on the device (the kernel's); only the entries a0 .. a0 + na and b0 .. b0 + nb are read.  One wave per
 * cell; every element of e is read once, coalesced along the columns.
 * GRL_EINVAL, before any launch: a null pointer, a negative size, a negative ptr, a tracklet without clips or a ptr
 * that is not ascending, ld smaller than the block's clip columns gptr[b0 + nb] - gptr[b0], ldo < nb, an unknown reduce.
 * GRL_EUNSUPPORTED, before any launch: a tracklet of more than GRL_SET_MAX_CLIPS clips. */
#define GRL_SET_MIN        0
#define GRL_SET_MEAN       1
#define GRL_SET_CHAMFER    2
#define GRL_SET_HAUSDORFF  3
#define GRL_SET_MAX_CLIPS  1024
int grl_setdist_block(const float* e, int64_t ld, const int64_t* qptr_host, const int64_t* qptr, int a0, int na,
                      const int64_t* gptr_host, const int64_t* gptr, int b0, int nb, int reduce, float* out, int64_t ldo,
                      void* stream);

/* ---- product-quantised gallery index: ADC scan, table fix-up, code packing, decode (pq.hip, engine.pq_* / PqCodebook /
 * PqIndex) ----
 * d feature columns in M subspaces of dsub = d / M columns, ksub = 2^nbits centroids per subspace (nbits 4..8: ksub 16,
 * 32, 64, 128 or 256); a gallery row is M codes, one byte each whatever nbits is.  A query's table lut [M][ksub] holds its
 * distance term to every centroid (GRL_PQ_COSINE: the NEGDOT GEMM's -q_m . C[m][c]; GRL_PQ_EUCLIDEAN: cn[m][c] + 2 * that,
 * cn = grl_row_sqnorm of the centroids).  The ADC sum of a pair with codes c_m, normative: four partials p_0 .. p_3, p_w
 * the sequential fp32 sum from +0.0f of lut[m][c_m] over m = w, w + 4, w + 8, .. ascending (+0.0f when M <= w), and
 * S = (p_0 + p_1) + (p_2 + p_3).  Adds only (no fma, no atomics); NaN and infinities follow IEEE through the adds.
 * GRL_PQ_COSINE: dist = S.  GRL_PQ_EUCLIDEAN: t = rn[q] + S, dist = sqrtf(t > 1e-12f ? t : 1e-12f) (a NaN t gives
 * 1e-12f, as GRL_EPI_EUCLID does).  The order depends on M alone: the same bits on every run, for every n, nq, ldo and
 * launch; tests/pq_ref.py is this paragraph in numpy float32.
 * grl_pq_scan: out[q][g] (row stride ldo >= n; only the first n columns of a row are written), q < nq, g < n, from the
 * tables lut [nq][M][ksub] and the SCAN LAYOUT of the codes: uint32 [ceil(M / 4)][n], byte b (bits 8b .. 8b + 7) of word
 * [w][g] = the code of subspace 4w + b of gallery row g, bytes of subspaces >= M zero (grl_pq_pack writes it).  rn [nq]
 * is read by GRL_PQ_EUCLIDEAN only.  The codes must be < ksub (grl_pq_pack's flag); a larger byte reads some other entry
 * of the staged tables, never outside them.  64 KiB of LDS per workgroup.
 * grl_pq_lut_finish: lut[q][m][c] = cn[m][c] + 2.0f * lut[q][m][c] in place (the multiply is exact, one rounded add).
 * grl_pq_pack: labels int32 [M][n] (the top-1 centroid of every row per subspace) -> codes uint8 [n][M] and the scan
 * layout codes4; with labels == NULL, codes is the INPUT and only codes4 is written.  *flag (int32, zeroed by the
 * caller) is set to 1 when a label or code is outside 0..ksub-1 (stored as 0).
 * grl_pq_decode: out[i][m * dsub + j] = codebooks[m][codes[i][m]][j] (codebooks [M][ksub][dsub]), 16-byte copies.
 * GRL_EINVAL, before any launch: a null pointer, a negative size, M outside 1..GRL_PQ_M_MAX, ksub not one of the five,
 * an unknown metric, GRL_PQ_EUCLIDEAN without rn, ldo too small, a pointer that is not aligned (4 bytes: lut, out,
 * codes4; 16 bytes: codebooks and out of grl_pq_decode, whose dsub and ldo must be multiples of 4), nq > 262140. */
#define GRL_PQ_COSINE     0
#define GRL_PQ_EUCLIDEAN  1
#define GRL_PQ_M_MAX      4096
int grl_pq_scan(const float* lut, const uint32_t* codes4, float* out, int nq, int64_t n, int M, int ksub, int64_t ldo,
                int metric, const float* rn, void* stream);
int grl_pq_lut_finish(float* lut, const float* cn, int nq, int M, int ksub, void* stream);
int grl_pq_pack(const int32_t* labels, uint8_t* codes, uint32_t* codes4, int64_t n, int M, int ksub, int32_t* flag,
                void* stream);
int grl_pq_decode(const float* codebooks, const uint8_t* codes, float* out, int64_t n, int M, int ksub, int dsub,
                  int64_t ldo, void* stream);

/* ---- IVF-PQ gallery index: inverted lists over residual product-quantiser codes (ivf.hip, engine.ivf_* / IvfPqCodebook /
 * IvfPqIndex).  Additive: GRL_ABI_VERSION stays 10. ----
 * A coarse quantiser coarse [nlist][d] splits the gallery into nlist inverted lists; list l holds the rows at the LIST
 * POSITIONS list_ptr[l] .. list_ptr[l + 1] (int64 [nlist + 1]) in ascending gallery index, ids [n] (int32) is the gallery
 * index at every position, and the codes -- of the residual row - coarse[list], by a product quantiser as above -- sit in
 * the scan layout uint32 [ceil(M / 4)][n] in list order.  The query tables lut [nq][M][ksub] are the GRL_PQ_COSINE ones
 * (-q_m . R[m][c]) under both metrics.
 * grl_ivf_scan serves the probe ranks of one chunk: probe [nq][ldp] (np used) are the probed lists of every query, g0
 * [nq][ldp] the query's coarse term -q . coarse[list] of each, off [nq][np + 1] (int32) the prefix sums of the probed lists'
 * lengths (off[q][0] = 0).  Query q's VIRTUAL ROW is its probed lists one after the other in probe-rank order; column col
 * with off[q][j] <= col < off[q][j + 1] is list position p = list_ptr[probe[q][j]] + col - off[q][j].  Normative distance:
 * S = the ADC sum above over the codes at p; t = g0[q][j] + S; GRL_PQ_COSINE: dist = t; GRL_PQ_EUCLIDEAN: u = xn[p] +
 * 2.0f * t (the multiply is exact), w = rn[q] + u, dist = sqrtf(w > 1e-12f ? w : 1e-12f) (xn [n] = grl_row_sqnorm of the
 * reconstructed rows in list order, rn [nq] that of the queries).  out[q][col] = dist and cidx[q][col] = ids[p] for col <
 * off[q][np]; the columns from there to width get +inf and -1 (grl_topk_block skips them).  Rows of out and cidx have
 * stride ldo >= width.  Adds only, no atomics: the same bits on every run and for every chunking of the probes.  20 KiB of
 * LDS per workgroup.
 * grl_ivf_residual: out[i][c] = x[i][c] - coarse[labels[i]][c] for a block of rows (one rounded subtraction).
 * grl_ivf_reconstruct: out[i][m * dsub + j] = coarse[labels[i]][m * dsub + j] + codebooks[m][codes[i][m]][j] (one rounded
 * add) for the given labels int32 [rows] and codes uint8 [rows][M].
 * grl_ivf_check_labels: *flag (int32, zeroed by the caller) is set to 1 when a label is outside 0..nlist-1.
 * GRL_EINVAL, before any launch: a null pointer, a negative size, n >= 2^31, nlist outside 1..GRL_IVF_NLIST_MAX, np outside
 * 1..min(nlist, GRL_IVF_NPROBE_MAX), M, ksub or metric as grl_pq_scan refuses them, GRL_PQ_EUCLIDEAN without xn and rn, a
 * stride that is too small, a pointer that is not aligned (8 bytes: list_ptr; 4 bytes: every other array), nq > 65535. */
#define GRL_IVF_NLIST_MAX   65536
#define GRL_IVF_NPROBE_MAX  1024
int grl_ivf_scan(const float* lut, const uint32_t* codes4, const int32_t* ids, const int64_t* list_ptr, const int32_t* probe,
                 const float* g0, int64_t ldp, int np, const int32_t* off, const float* xn, const float* rn, float* out,
                 int32_t* cidx, int64_t ldo, int width, int nq, int64_t n, int nlist, int M, int ksub, int metric,
                 void* stream);
int grl_ivf_residual(const float* x, int64_t ldx, const int32_t* labels, const float* coarse, int nlist, float* out,
                     int64_t ldo, int64_t rows, int d, void* stream);
int grl_ivf_reconstruct(const float* coarse, const float* codebooks, const int32_t* labels, const uint8_t* codes, float* out,
                        int64_t rows, int nlist, int M, int ksub, int dsub, int64_t ldo, void* stream);
int grl_ivf_check_labels(const int32_t* labels, int64_t n, int nlist, int32_t* flag, void* stream);

/* ---- exact refinement of a shortlist from a feature store (refine.hip, engine.RefineStore / refine_dist / refine_lists /
 * refine_search).  Additive: GRL_ABI_VERSION stays 10. ----
 * The store holds the n gallery rows of d columns, d % 4 == 0, 1 <= d <= GRL_REFINE_D_MAX (the query row is staged in
 * LDS: d * 4 bytes, 64 KiB at the maximum), as fp32 (GRL_REFINE_F32, row stride lds floats) or as bf16 (GRL_REFINE_BF16,
 * uint16 [n][lds]); a row's VALUE is the fp32 widening of what is stored.  With u = 2^-24:
 * Pair distance, normative.  For query row q and store row x, per column c: GRL_PQ_COSINE p_c = fl(q_c * x_c);
 * GRL_PQ_EUCLIDEAN e_c = fl(q_c - x_c), p_c = fl(e_c * e_c).  Every rounding is kept (no fma).  Lane l (0..63) owns the
 * columns 256 t + 4 l + e, e = 0..3, t = 0, 1, ..:
 *   1. its four partials a_e are the sequential fp32 sums from +0.0f of p_c over t ascending; columns >= d are skipped
 *      (the same as adding +0.0f: a partial that starts at +0.0f is never -0.0f, so a model may pad with zeros);
 *   2. v_l = (a_0 + a_1) + (a_2 + a_3);
 *   3. v_l = v_l + v_{l xor o} for o = 32, 16, 8, 4, 2, 1 (common.h's wave_sum): every lane ends with the same bits S;
 *   4. GRL_PQ_COSINE: dist = -S.  GRL_PQ_EUCLIDEAN: dist = sqrtf(S > 1e-12f ? S : 1e-12f) (a NaN S gives 1e-12f, as
 *      GRL_EPI_EUCLID does); the difference is taken first, so no norm arrays are needed and nothing cancels;
 *   5. a NaN result is stored as 0x7fc00000.
 * No atomics of any kind: the same bits on every run, for every nq, L, slab and launch; tests/refine_ref.py is this
 * paragraph in numpy float32, bit for bit.
 * grl_refine_scan: cand int64 [nq][ldc] (L used) are index lists as grl_topk_block's callers return them; out[q][j] =
 * dist(q, cand[q][j]) and cidx[q][j] = (int32) cand[q][j], rows of stride ldo >= L.  An entry < 0 or >= n is padding: it
 * is never dereferenced, out = +inf and cidx = -1 (grl_topk_block skips it).  A repeated id is a candidate twice.
 * grl_refine_pack_bf16: out[i] = bf16(x[i]), i < count: round to nearest even on the upper 16 bits, every NaN becomes
 * 0x7fc0, +-inf and +-0 keep their bits, a finite value beyond the bf16 range rounds to infinity.  One lane per 8 elements
 * (16-byte accesses when both pointers are 16-byte aligned), the ragged end element by element.
 * GRL_EINVAL, before any launch: a null pointer, a negative size, n >= 2^31, d outside 1..GRL_REFINE_D_MAX or no multiple of
 * 4, an unknown store type or metric, a stride that is too small or (ldq, lds) no multiple of 4, a pointer that is not
 * aligned (16 bytes: q and an fp32 store; 8 bytes: a bf16 store and cand; 4 bytes: out, cidx and x; 2 bytes: the bf16
 * output), nq > 65535. */
#define GRL_REFINE_F32    0
#define GRL_REFINE_BF16   1
#define GRL_REFINE_D_MAX  16384
int grl_refine_scan(const float* q, int64_t ldq, const void* store, int64_t lds, int store_type, const int64_t* cand,
                    int64_t ldc, float* out, int32_t* cidx, int64_t ldo, int nq, int L, int64_t n, int d, int metric,
                    void* stream);
int grl_refine_pack_bf16(const float* x, uint16_t* out, int64_t count, void* stream);

/* ---- kNN-graph gallery index with beam search (nng.hip, engine.nng_knn / nng_optimize / NnGraphIndex / nng_build /
 * nng_search).  Additive: GRL_ABI_VERSION stays 10. ----
 * All ids are row numbers of a feature store of n rows as above, n < 2^31.  "Live" means 0 <= id < n; anything else is
 * padding, is never dereferenced and is skipped wherever it stands.  tests/nng_ref.py is this text in numpy.
 *
 * Graph optimisation (integers only, exact).  Input knn int32 [n][K]: row i lists the candidate neighbours of i, nearest
 * first.  An entry equal to i, a non-live entry and every repeat of an id after its first position are padding.  With
 * t_x = knn[i][x]:
 *   Detours.  For a live position b, det[i][b] = #{a < b, a live : t_b in {knn[t_a][r] : r < b, r live in row t_a}} (the
 *     rank-based 2-hop count of CAGRA); det of a padding position is -1.
 *   Pruned forward lists.  F[i] = the ids at the first D of row i's live positions in the order (det, b), padded with -1.
 *   Reverse lists.  rev[j] = every i with j in F[i], ordered by (position of j in F[i], i).
 *   Merge.  N[i] = the first D ids, without repeats, of the sequence below, padded with -1:
 *     1. F[i][0 : D/2];
 *     2. the entries of rev[i], in order, that are not yet present, until D/2 of them have been taken;
 *     3. F[i][D/2 : D], those not yet present;
 *     4. the rest of rev[i], those not yet present.
 *   Domain: 2 <= K <= GRL_NNG_K_MAX, D even, 2 <= D <= min(K, GRL_NNG_D_MAX).
 * grl_nng_detours writes det [n][K] (one workgroup per node: row i and the rows it points to in LDS, at most 64 of them
 * at a time).  grl_nng_merge: fwd = F int32 [n][D], rev in CSR form (rev_off int64 [n + 1], rev int32 in the order
 * above), out = N int32 [n][D]; one lane per node.
 *
 * Beam search.  For each query q, with the neighbour table N int32 [n][D], S seeds, itopk size L, search width w and
 * iteration cap T:
 *     visited = {}; C = []                               # C: entries (dist, id, expanded)
 *     for s in seeds (in any order): if s live and s not in visited: visited += s; C += (dist(q, s), s, False)
 *     C = first L of C sorted by (order_key(dist), id)
 *     for it in 0 .. T-1:
 *         P = the first w entries of C, in C's order, with expanded == False;  if P is empty: stop
 *         mark them expanded;  new = []
 *         for p in P, e in 0 .. D-1:  v = N[p.id][e];  if v live and v not in visited: visited += v; new += (dist(q, v), v, False)
 *         C = first L of (C u new) sorted by (order_key(dist), id)
 *     result = C                                          # at most L entries, padded with +inf / -1
 * dist is exactly the pair distance above, steps 1-5, for both metrics and both store types; order_key is
 * grl_row_argsort's (canonical NaN after +inf, -0 == +0).  visited is an exact set: an id that ever entered it is never
 * scored again, even after it fell out of C.  The ids of C are unique, so the order is total, and the result does not
 * depend on the order in which `new` is produced nor on which of two lanes claims a shared neighbour.  No floating-point
 * atomics (an integer atomicCAS claims an id in the visited table), plain vector stores: the same bits from run to run
 * and for any split of the queries into calls.  stats int32 [nq][2], both exact: |visited|, and the number of iterations
 * that expanded at least one parent.
 * Domain: L a power of two in GRL_NNG_L_MIN..GRL_NNG_L_MAX, 1 <= w <= GRL_NNG_W_MAX, w * D <= GRL_NNG_WD_MAX, T >= 1,
 * 1 <= S <= L, d as the store takes it.  seeds int32 [nq][seed_stride] (S used), or shared by all queries with
 * seed_stride = 0.  out float [nq][L], oidx int32 [nq][L].  At most 65535 queries per call.
 * One workgroup per query holds in LDS the query row (4 d bytes), the sort buffer (8 bytes times the power of two >=
 * L + w * D), the visited table and the iteration's id list (4 max(S, w * D) bytes, plus 64).  The table never drops an id:
 * it has a power of two >= max(64, 2 min(S + T * w * D, n)) slots of 4 bytes (a call cannot visit more than n rows).
 * grl_nng_search_lds_bytes returns the total (-1 outside the domain); above GRL_NNG_LDS_MAX = 64 KiB, the most a launch
 * takes without the kernel's max-dynamic-LDS attribute, grl_nng_search is GRL_EINVAL and its message names both numbers.
 * The defaults L = 64, w = 1, T = 64, D = 32 at d = 6144 take 58688 bytes.
 * GRL_EINVAL, before any launch: a null pointer, a size outside the domain, an unknown store type or metric, a stride
 * that is too small or (ldq, lds) no multiple of 4, a seed_stride that is neither 0 nor >= S, a pointer that is not
 * aligned (as grl_refine_scan; 4 bytes for the int32 arrays, 8 for rev_off), nq > 65535, the LDS limit. */
#define GRL_NNG_K_MAX    128
#define GRL_NNG_D_MAX    64
#define GRL_NNG_L_MIN    8
#define GRL_NNG_L_MAX    512
#define GRL_NNG_W_MAX    8
#define GRL_NNG_WD_MAX   256
#define GRL_NNG_LDS_MAX  65536
int64_t grl_nng_search_lds_bytes(int64_t n, int d, int D, int L, int w, int64_t T, int S);
int grl_nng_search(const float* q, int64_t ldq, const void* store, int64_t lds, int store_type, const int32_t* nbr,
                   const int32_t* seeds, int64_t seed_stride, float* out, int32_t* oidx, int32_t* stats, int nq, int64_t n,
                   int d, int D, int L, int w, int T, int S, int metric, void* stream);
int grl_nng_detours(const int32_t* knn, int32_t* det, int64_t n, int K, void* stream);
int grl_nng_merge(const int32_t* fwd, const int64_t* rev_off, const int32_t* rev, int32_t* out, int64_t n, int D, void* stream);

/* ---- binary hash codes: bit packing, Hamming scan, asymmetric tables (bin.hip, engine.bin_* / BinaryCodebook /
 * BinaryIndex).  Additive: GRL_ABI_VERSION stays 10. ----
 * A gallery row is nbits bits, nbits a multiple of 32 in 32..GRL_BIN_NBITS_MAX, W = nbits / 32 words.  The projection,
 * normative: z[i][b] = (x_i . proj[b]) + shift[b], the fp32 GEMM (grl_conv_gemm_f32, GRL_MATH_F32 whatever the math mode is).
 * Bit b of row i is z[i][b] > 0: NaN, -0 and +0 give 0.  PUBLIC LAYOUT: codes uint8 [n][nbits / 8], bit j of byte m =
 * projection column 8m + j (numpy.packbits(bits, axis=1, bitorder='little')).  SCAN LAYOUT: uint32 [W][ldw], ldw >= n, word
 * [w][g] = the bytes 4w .. 4w + 3 of public row g, little endian (bit t of the word = column 32w + t) -- exactly grl_pq_pack's
 * scan layout for M = nbits / 8, ksub = 256 when ldw = n, so one copy serves grl_bin_scan and grl_pq_scan.  Query codes of the
 * symmetric scan: uint32 [nq][W], the public bytes of the query rows reinterpreted.
 * grl_bin_scan: out[q][g] = (float) sum_w popcount(qwords[q][w] ^ words[w][g]) for q < nq, g < n (row stride ldo >= n; only
 * the first n columns of a row are written): the Hamming distance, an exact integer in 0..nbits.  Integer accumulators, no
 * atomics, one conversion at the store; a workgroup scores 8 queries against a slab of GRL_BIN_SLAB columns.
 * grl_bin_pack: z [n][ldz] -> codes (public layout), words (scan layout) and signs float [n][lds] (+1.0f where the bit
 * is set, -1.0f elsewhere), in one launch; each of the three may be NULL (not all).  grl_bin_words: codes -> words.
 * grl_bin_lut: the asymmetric tables lut [nq][nbits / 8][256] of the query projections z [nq][ldz]: entry [q][m][c] is the
 * sequential fp32 sum from +0.0f over j = 0 .. 7 of t_j, t_j = -z[q][8m + j] when bit j of c is set, else +z[q][8m + j]
 * (adds and exact negations only).  The asymmetric distance of a pair is grl_pq_scan over these tables and the scan words
 * (M = nbits / 8, ksub = 256, GRL_PQ_COSINE, ldw = n): -sum_b z_q[b] s_g[b], s = +-1, in the ADC sum's normative order.
 * GRL_EINVAL, before any launch: a null pointer, a negative size, nbits not a multiple of 32 or outside the range, ldz or
 * lds < nbits, ldw or ldo < n, a pointer that is not 4-byte aligned, nq > GRL_BIN_NQ_MAX (the grid's limit: 8 * 65535). */
#define GRL_BIN_NBITS_MAX  1024
#define GRL_BIN_SLAB       1024
#define GRL_BIN_NQ_MAX     524280
int grl_bin_scan(const uint32_t* qwords, const uint32_t* words, int64_t ldw, float* out, int64_t ldo, int nq, int64_t n,
                 int nbits, void* stream);
int grl_bin_pack(const float* z, int64_t ldz, uint8_t* codes, uint32_t* words, int64_t ldw, float* signs, int64_t lds,
                 int64_t n, int nbits, void* stream);
int grl_bin_words(const uint8_t* codes, uint32_t* words, int64_t ldw, int64_t n, int nbits, void* stream);
int grl_bin_lut(const float* z, int64_t ldz, float* lut, int nq, int nbits, void* stream);

/* ---- int8 scalar-quantised gallery: quantiser, decode and the integer-MFMA scan (sq8.hip, engine.sq8_* / Sq8Codebook /
 * Sq8Index).  Additive: GRL_ABI_VERSION stays 10. ----
 * Normative; every operation is one fp32 operation, nothing is contracted, rint rounds half to even (tests/sq8_ref.py is the
 * numpy model).  d <= GRL_SQ8_D_MAX columns, dpad = d rounded up to a multiple of 64.
 * CODEBOOK: mean[d], delta[d] >= 0, inv[d].  grl_sq8_steps with amax: delta[j] = amax[j] / 127.0f, inv[j] = 127.0f / amax[j],
 * 0 where amax[j] == 0; without (amax NULL, delta read): inv[j] = 127.0f / (127.0f * delta[j]), 0 where delta[j] == 0.
 * grl_sq8_absmax: amax[j] = max_i |x[i][j] - mean[j]| (a NaN difference is ignored; 0 for n = 0), an integer atomic max
 * on the bits of the non-negative floats after the entry point has cleared amax: a maximum has no order.
 * ROW CODE (grl_sq8_encode): v = (x[i][j] - mean[j]) * inv[j]; c = 0 when v is NaN, else rint(v) clamped to -127 .. 127.
 * codes int8 [n][ldc], ldc >= dpad a multiple of 16; the columns d .. dpad of a row are written 0 (a zero column adds
 * exactly 0 to every sum).  Caller-supplied codes may hold -128.
 * VALUE OF A STORED ROW (grl_sq8_decode): out[i][j] = mean[j] + delta[j] * (float)c[i][j] for j < d: one multiply, one add.
 * QUERY (grl_sq8_query): w[j] = q[j] * delta[j]; s = the maximum of |w[j]| over the FINITE w[j] (0 if there is none);
 * r = 127.0f / s; cq[j] = 0 when w[j] is NaN or infinite or fl(w[j] * r) is NaN, else rint(w[j] * r) clamped to
 * -127 .. 127; scale = s / 127.0f.  s == 0: every code 0, scale 0.  qcodes int8 [nq][ldc] with the zero tail up to dpad.
 * SCAN (grl_sq8_scan): isum = sum_j cq[q][j] * c[g][j], exact in int32 (dpad * 128^2 <= 2^28); dot = scale[q] *
 * (float)isum + bias[q] (the conversion rounds to nearest even; bias[q] = q . mean comes from the fp32 GEMM);
 * GRL_PQ_COSINE: out[q][g] = -dot; GRL_PQ_EUCLIDEAN: t = (qq[q] + gg[g]) - 2.0f * dot, out = sqrtf(t > 1e-12f ? t :
 * 1e-12f) (a NaN t gives 1e-12f, as grl_pq_scan's).  qq, gg = grl_row_sqnorm of the query and of the decoded row, read by
 * GRL_PQ_EUCLIDEAN only.  grl_sq8_scan_i32 stores isum itself.  Both operands are rows of K-contiguous bytes with a row
 * stride, so a block of gallery rows is a pointer offset.  A workgroup of 256 lanes owns a GRL_SQ8_TILE x GRL_SQ8_TILE
 * tile of out through v_mfma_i32_32x32x32_i8; rows >= n and queries >= nq are neither loaded nor stored.
 * GRL_EINVAL, before any launch: a null pointer, a negative size, d outside 1..GRL_SQ8_D_MAX, dpad not a multiple of 64 or
 * above GRL_SQ8_D_MAX, a row stride below its extent (or, for codes, not a multiple of 16), a pointer that is not aligned
 * (16 bytes: codes and qcodes; 4 bytes: floats and int32), nq > GRL_SQ8_NQ_MAX, an unknown metric, GRL_PQ_EUCLIDEAN
 * without qq and gg. */
#define GRL_SQ8_D_MAX    16384
#define GRL_SQ8_TILE     128
#define GRL_SQ8_NQ_MAX   1048576
int grl_sq8_absmax(const float* x, int64_t ldx, const float* mean, float* amax, int64_t n, int d, void* stream);
int grl_sq8_steps(const float* amax, float* delta, float* inv, int d, void* stream);
int grl_sq8_encode(const float* x, int64_t ldx, const float* mean, const float* inv, int8_t* codes, int64_t ldc, int64_t n,
                   int d, void* stream);
int grl_sq8_decode(const int8_t* codes, int64_t ldc, const float* mean, const float* delta, float* out, int64_t ldo,
                   int64_t n, int d, void* stream);
int grl_sq8_query(const float* q, int64_t ldq, const float* delta, int8_t* qcodes, int64_t ldc, float* scale, int nq, int d,
                  void* stream);
int grl_sq8_scan(const int8_t* qcodes, int64_t ldqc, const int8_t* codes, int64_t ldc, const float* scale, const float* bias,
                 const float* qq, const float* gg, float* out, int64_t ldo, int nq, int64_t n, int dpad, int metric,
                 void* stream);
int grl_sq8_scan_i32(const int8_t* qcodes, int64_t ldqc, const int8_t* codes, int64_t ldc, int32_t* out, int64_t ldo, int nq,
                     int64_t n, int dpad, void* stream);

/* ---- ranking by the Siamese verification head (verify.hip, engine.verify_metric / verify_dist) ----
 * In eval mode classifierBN -> classifierlinear on (p - g)^2 is affine in (p - g)^2; the class-1 minus class-0 logit is
 * s(p, g) = sum_d w_d (p_d - g_d)^2 + c.  The ranking distance F = (1 - beta)(-q.g) + beta(-s), p / g = columns
 * [col0, col0 + Dv) of the rows q / g, is  F = -q'.g - (rq + rg):  one NEGDOT GEMM (grl_conv_gemm_f32, unchanged) on
 * the modified queries q' and the pass grl_verify_finish, with rq = beta (a_q + c), rg = beta a_g,
 * a_x = sum_d w_d x_d^2 over the slice.
 *
 * grl_verify_fold: w[d] = fp32((W[1][d] - W[0][d]) * gamma[d] / sqrt(var[d] + eps)), c = sum_d (W[1][d] - W[0][d]) *
 *   (beta[d] - gamma[d] * mean[d] / sqrt(var[d] + eps)) + b[1] - b[0], all in fp64 in exactly this operation order
 *   (tests/verify_ref.py); c is stored as fp64 (*c64) and rounded to fp32 (*c32).  One workgroup: thread t adds its
 *   d = t, t + 256, ... in ascending order, the 256 sums meet in a binary tree.  W is [2][D], D % 4 == 0.
 * grl_verify_rows: r[i] = fp32(beta * (sum_d w[d] * x[i][col0 + d]^2 + (c64 ? *c64 : 0))) for n rows x [n][ldx] of d
 *   columns.  fp64; one wave per row, lane l adds elements 4 (l + 64 j) .. + 3 for j = 0, 1, ... in ascending order, the
 *   64 sums meet in an xor tree: no dependence on the launch.  With qout, the modified query rows, every element
 *   computed in fp64 and rounded once: full != 0: qout [n][ldq] has d columns, ((1 - beta) - 2 beta w[e]) x inside the
 *   slice and (1 - beta) x outside; full == 0: qout has Dv columns, column e = ((1 - beta) - 2 beta w[e]) x[col0 + e]
 *   (beta = 1: -2 w x; the GEMM then runs over K = Dv against the gallery slice in place, ldw = the gallery's ld).
 *   d, col0, Dv, ldx, ldq % 4 == 0, 16-byte aligned pointers, 0 < beta <= 1, qout must not overlap x.
 *   `eps` (fold) and `beta` (rows) point to one double in HOST memory, read during the call: the two scalars keep
 *   their fp64 value across the ABI.  Every other pointer is device memory.
 * grl_verify_finish: in place on a distance block D [nq][ld] (n columns used, any ld >= n):
 *   D[q][j] = D[q][j] - (rq[q] + rg[c0 + j]), the fp32 sum first, then the fp32 difference.  An entry depends on
 *   nothing but itself, so a column block holds the full matrix's bits.  16-byte accesses from a row's first 16-byte
 *   boundary on, element by element before it and at the ragged end. */
int grl_verify_fold(const float* bn_weight, const float* bn_bias, const float* bn_mean, const float* bn_var,
                    const double* eps, const float* W, const float* b, int D, float* w, double* c64, float* c32, void* stream);
int grl_verify_rows(const float* x, int64_t ldx, int n, int d, int col0, int Dv, const float* w, const double* beta,
                    const double* c64, float* r, float* qout, int64_t ldq, int full, void* stream);
int grl_verify_finish(float* D, int64_t ld, int nq, int n, const float* rq, const float* rg, int64_t c0, void* stream);

/* ---- k-reciprocal re-ranking on the device (reid/evaluator/rerank.py:37-104) ----
 * N = nq + ng samples (<= 16384).  All matrices fp32 row-major, caller-owned:
 *   D [N][N], rank int32 [N][N] (grl_row_argsort of D), V / V2T [N][N] and V2q [nq][N]
 *   ZERO-FILLED by the caller, lcnt int32 [N], lidx int32 [N][256]. */
/* :41-47  D[i][j] = S[j][i] / max_r S[r][i],  S = [[q_q, q_g], [q_g^T, g_g]] squared */
int grl_rerank_build(const float* q_g, const float* q_q, const float* g_g, int nq, int ng, float* D,
                     float* colmax_ws /* N floats */, void* stream);
/* :55-75  k-reciprocal set of every sample (k1 <= 20), its 2/3-overlap expansion by the
 * int(around(k1/2))-reciprocal sets, V[i][e] = exp(-D[i][e]) / sum (np.sum's pairwise order);
 * lidx[i][0..lcnt[i]) = the sorted unique expansion indices */
int grl_rerank_krecip(const float* D, const int32_t* rank, int N, int k1, float* V, int32_t* lcnt,
                      int32_t* lidx, void* stream);
/* :77-83  local query expansion V2[i] = mean_{t<k2} V[rank[i][t]] (k2 <= 8; k2 == 1: V itself),
 * stored transposed V2T[e][i] and, for i < nq, as dense rows V2q[i][e] */
int grl_rerank_expand(const float* V, const int32_t* rank, const int32_t* lcnt, const int32_t* lidx,
                      int N, int nq, int k2, float* V2T, float* V2q, void* stream);
/* :86-104 out[i][j-nq] = (1-lambda) * (1 - t/(2-t)) + lambda * D[i][j],
 * t = sum over the non-zero k of V2[i] (ascending) of min(V2[i][k], V2[j][k]);  out [nq][ng] */
int grl_rerank_jaccard(const float* V2q, const float* V2T, const float* D, int N, int nq,
                       float lambda_value, float one_minus_lambda, float* out, void* stream);

/* ---- streaming k-reciprocal re-ranking (rerank_stream.hip, engine.rerank_search / engine.rerank_metrics_streaming,
 * DESIGN.md 4o): the values of the entry points above without any N x N or nq x ng array.  Same limits (k1 <= 20,
 * k2 <= 8), no limit on N.  A SEGMENT is w sample columns [i0, i0 + w) on one side of the query/gallery boundary:
 * S[r][i0 + c] = up[r * ldu + c] for r < nq and lo[(r - nq) * lo_rs + c * lo_cs] for r >= nq (unsquared distances). */
/* colmax[c] = max_r S[r][i0+c]^2 and the D rows drows[c][j] = S[j][i0+c]^2 / colmax[c], j < nq + ng, bit-equal to
 * grl_rerank_build's (colmax and drows point at sample i0) */
int grl_rrs_segment_rows(const float* up, int64_t ldu, const float* lo, int64_t lo_rs, int64_t lo_cs, int nq, int ng,
                         int w, float* colmax, float* drows, int64_t ldd, void* stream);
/* lidx[i][0..lcnt[i]) = grl_rerank_krecip's sorted expansion list of every sample, from rank [N][ld] (the first
 * ld >= k1 + 1 entries of each row of grl_row_argsort(D)) */
int grl_rrs_lists(const int32_t* rank, int64_t ld, int N, int k1, int32_t* lcnt, int32_t* lidx, void* stream);
/* lval[i][a] = V[i][lidx[i][a]] of grl_rerank_krecip for the segment's samples i = i0 .. i0 + w - 1 (colmax [N],
 * lcnt / lidx / lval [N][256] indexed from sample 0) */
int grl_rrs_weights(const float* up, int64_t ldu, const float* lo, int64_t lo_rs, int64_t lo_cs, int nq, int ng,
                    int w, int i0, const float* colmax, const int32_t* lcnt, const int32_t* lidx, float* lval,
                    void* stream);
/* V2 = grl_rerank_expand's rows as CSR over all N samples, non-zero entries in ascending column order, bit-equal.
 * row_ptr == NULL: cnt[i] = entries of row i; otherwise row_ptr [N+1] (int64 prefix sum of cnt) and col / val are
 * filled. */
int grl_rrs_expand(const int32_t* rank, int64_t ld, const int32_t* lcnt, const int32_t* lidx, const float* lval, int N,
                   int k2, const int64_t* row_ptr, int32_t* cnt, int32_t* col, float* val, void* stream);
/* grl_rrs_expand for the samples row0 .. row0 + nrows - 1 only (a rank's share); cnt [N] and row_ptr [N+1] stay
 * indexed by the sample, so a fill with the global row_ptr writes the rows at their final place in col / val */
int grl_rrs_expand_rows(const int32_t* rank, int64_t ld, const int32_t* lcnt, const int32_t* lidx, const float* lval,
                        int N, int k2, int row0, int nrows, const int64_t* row_ptr, int32_t* cnt, int32_t* col,
                        float* val, void* stream);
/* ptr [n+1] = exclusive prefix sum of cnt [n] (>= 0) in 64 bits, ptr[n] = the total: row_ptr from grl_rrs_expand's
 * counts */
int grl_rrs_scan(const int32_t* cnt, int n, int64_t* ptr, void* stream);
/* the CSR entries of the rows row0 .. row1 - 1, packed from src_col[0] / src_val[0] on (a shard received from
 * another rank, cap = entries the source buffers hold), are copied to col / val at row_ptr[row0]; at most cap and
 * at most row_ptr[row1] - row_ptr[row0] entries move */
int grl_rrs_place(const int32_t* src_col, const float* src_val, int64_t cap, const int64_t* row_ptr, int row0, int row1,
                  int32_t* col, float* val, void* stream);
/* The inverted index grl_rrs_final reads: the CSR rows nq .. N-1 transposed.  csc_ptr [N+1] (int64), and for every
 * column k its samples j in ASCENDING order in csc_row with their values in csc_val (row_ptr[N] - row_ptr[nq]
 * entries).  Integer atomics count the columns and hand out slots; the final place of an entry is the number of
 * its column's samples below its own, so the result does not depend on the order of arrival.  Workspaces: ccnt [N]
 * int32, tmp_row / tmp_val as large as csc_row / csc_val.  Column indices outside 0..N-1 are skipped. */
int grl_rrs_transpose(const int64_t* row_ptr, const int32_t* col, const float* val, int nq, int N, int32_t* ccnt,
                      int32_t* tmp_row, float* tmp_val, int64_t* csc_ptr, int32_t* csc_row, float* csc_val,
                      void* stream);
/* in place: d [nq][ld] holds cosin_dist for gallery entries col0 .. col0 + ncols; each becomes grl_rerank_jaccard's
 * out value.  q_ptr / q_col / q_val: the CSR of V2 (rows 0..nq-1 are read); csc_ptr [N+1] / csc_row / csc_val: for
 * every k, the gallery samples j >= nq with V2[j][k] != 0 in ascending j and those values. */
int grl_rrs_final(float* d, int64_t ld, int nq, int col0, int ncols, const float* colmax, const int64_t* q_ptr,
                  const int32_t* q_col, const float* q_val, const int64_t* csc_ptr, const int32_t* csc_row,
                  const float* csc_val, float lambda_value, float one_minus_lambda, void* stream);

/* All weight re-layouts (and bf16 casts) of one training step in one launch: a table of gathers
 * dst[j] = src[base + i0*strides[0] + i1*strides[1] + i2*strides[2] + i3*strides[3]], j = ((i0*dims[1] + i1)*dims[2] +
 * i2)*dims[3] + i3, fp32 in, fp32 or bf16 out; `tiled` = a 2-D transpose (dims[0] = dims[1] = 1, strides[2] = 1)
 * through LDS tiles.  The table is DEVICE memory (built once per model by the host); it replaces, per step, the
 * grl_pack_conv_weight / grl_transpose / grl_pack_dgrad_weight / grl_cast_bf16 launches of
 * resnets1.py:62-68's and grl_model.py:95-121's weights. */
typedef struct GrlPrepEntry {
    const float* src;
    void*        dst;
    int64_t      base;
    int64_t      strides[4];
    int32_t      dims[4];
    int32_t      tiled, out_bf16;
} GrlPrepEntry;
int grl_weight_prep(const GrlPrepEntry* table_dev, int count, void* stream);

/* ---- bf16-STORAGE training (train_engine.set_math('bf16s'); BASELINE configs[2] as a training batch) -------------
 * The twins of the train-mode kernels above for bf16 activations / saved tensors / activation gradients in HBM
 * (`void*` = bf16 tensor); statistics, per-channel vectors and parameter gradients stay fp32.  Same reference call
 * sites as the fp32 entry points they mirror (resnets1.py:76-91, basebranch.py:38-66, grl_model.py:71-83,131-180
 * and their autograd backward, trainer.py:54).  C % 8 == 0, 16-byte aligned tensors. */
int grl_bn_apply_centered_bf16(const void* z, const float* mean, const float* scale, const float* beta,
                               const void* res, void* y, int64_t M, int C, int relu,
                               uint8_t* relu_bits /* may be NULL: M*C/8 bytes, one bit per stored output */, void* stream);
/* pivot: an fp32 VECTOR [C] (or NULL), not a row of x as in grl_col_stats */
int grl_col_stats_bf16(const void* x, float* slab, int M, int C, int ld, const float* pivot, void* stream);
int grl_bn_bwd_bf16(const void* dy, const void* z, const void* act, const float* mean, const float* invstd,
                    const float* gamma, void* dz, float* dgamma, float* dbeta, float* slab_ws, float* coef_ws,
                    int M, int C, void* gres, int gres_accumulate, const float* mask_scale,
                    const float* mask_beta, const uint8_t* relu_bits, void* stream);
int grl_relu_bwd_bf16(const void* dy, const void* act, void* out, int64_t n, int accumulate, void* stream);
int grl_axpby_bf16(const void* a, const void* b, void* y, float alpha, float beta, int64_t n, void* stream);
int grl_axpy_strided_bf16(void* dst, int64_t dst_stride, const void* src, int64_t src_stride, int nb,
                          int64_t inner, float alpha, int accumulate, void* stream);
int grl_dilate2_bf16(const void* dz, void* up, int n, int Ho, int Wo, int H, int W, int C, int accumulate,
                     int oy_off, int ox_off, void* stream);
int grl_maxpool3x3s2_bwd_bf16(const void* x, const void* dy, void* dx, int n, int H, int W, int C, void* stream);
int grl_bn_relu_maxpool3x3s2_bf16(const void* z, const float* mean, const float* scale, const float* beta, void* y,
                                  uint8_t* idx, int n, int H, int W, int C, void* stream);
int grl_maxpool3x3s2_bwd_idx_bf16(const uint8_t* idx, const void* dy, void* dx, int n, int H, int W, int C, void* stream);
/* fp32 clip in, bf16 im2col columns out (the stem's weight gradient) */
int grl_stem_im2col_bf16(const float* x, void* col, int n, int H, int W, int Kp, void* stream);
int grl_gate_apply_bf16(const void* y, int ldy, const void* x, float* cmap, void* xc, void* xu, int M, int C,
                        void* stream);
int grl_gate_bwd_bf16(const void* dxc, const void* dxu, const void* x, const float* cmap, void* dx,
                      int accumulate, void* dy, int ldy, int M, int C, void* stream);
/* v: fp32 per-group vectors, or (v_is_bf16) a bf16 tensor -- the temporal-mean backward */
int grl_add_rowbcast_bf16(void* dst, const void* v, int64_t M, int64_t C, int64_t rows_per_group, float scale,
                          int accumulate, int v_is_bf16, void* stream);
int grl_sqdiff_bwd_bf16(const void* f1, const void* f2, const float* dd, void* df1, void* df2, int b, int rows,
                        int C, int64_t f2_clip_stride, int accumulate_df2, void* stream);
/* bf16 -> fp32 (n % 8 == 0) */
int grl_cast_f32(const void* x, float* y, int64_t n, void* stream);

/* ---- cross-layer fusion of the bf16-storage trunk (round 4, fuse_bf16.hip) -------------------------------------
 * END of one ResNet bottleneck + START of the next in one launch (layers 1-2, where both 1x1 convolutions are
 * HBM-bound):   y = relu(bn3(conv3(t2)) + res)         reid/models/resnets1.py:86-91
 *               u = relu(bn1'(conv1'(y)))               reid/models/resnets1.py:76-78 of the next block
 * y (the widest tensor of the block) is written once and never re-read; a pixel's 4P outputs are contracted against
 * conv1' in the registers of the wave that produced them.  All activations / weights bf16 (row-major, channels
 * last), per-channel vectors fp32 (eval-folded BatchNorm: grl_bn_fold), fp32 accumulate, epilogues term for term
 * those of grl_conv_gemm_f32's bf16-storage datapath.  w1n must be in the chained k order: grl_bneck_perm32.
 * Shapes: (P, C4) = (64, 256) with Pn in {0, 64, 128}; (128, 512) with Pn in {0, 128, 256}; Pn = 0: no chain. */
typedef struct GrlBneckTail {
    const void*  t2;        /* [M][P]  bf16: conv2's output (after bn2 + ReLU)              */
    const void*  w3;        /* [C4][P] bf16: conv3 weight                                   */
    const float* scale3;    /* [C4] or NULL (= 1)                                           */
    const float* shift3;    /* [C4] or NULL (= 0)                                           */
    const void*  res;       /* [M][C4] bf16: the block's input (or its downsample branch)   */
    void*        y;         /* [M][C4] bf16 out                                             */
    const void*  w1n;       /* [Pn][C4] bf16, k-permuted (grl_bneck_perm32), or NULL        */
    const float* scale1n;   /* [Pn] or NULL                                                 */
    const float* shift1n;   /* [Pn] or NULL                                                 */
    void*        u;         /* [M][Pn] bf16 out, or NULL                                    */
    int32_t M, P, C4, Pn;
    /* Kd > 0: the residual is the block's DOWNSAMPLE branch computed in the same launch (resnets1.py:83-84, the first
     * block of a layer): res = bf16(scaled * (wd . x0) + shiftd); `res` is ignored.  (P, C4, Pn, Kd) = (64, 256, 64, 64). */
    const void*  x0;        /* [M][Kd] bf16: the block's input                              */
    const void*  wd;        /* [C4][Kd] bf16: downsample conv weight                        */
    const float* scaled;    /* [C4] or NULL                                                 */
    const float* shiftd;    /* [C4] or NULL                                                 */
    int32_t Kd, reserved;
} GrlBneckTail;
int grl_bottleneck_tail_bf16(const GrlBneckTail* desc, void* stream);
int grl_bottleneck_tail_bf16_supported(int P, int C4, int Pn);      /* 1 if the shape has a kernel */
/* w [Pn][C4] (fp32 if !w_is_bf16) -> out [Pn][C4] bf16 in the k order the chained MFMA of grl_bottleneck_tail_bf16 consumes */
int grl_bneck_perm32(const void* w, int w_is_bf16, void* out, int Pn, int C4, void* stream);

/* Stem + max-pool in ONE launch (eval, bf16 storage; resnets1.py:101-104: conv 7x7/s2 + folded bn1 + ReLU + MaxPool2d(3, 2, 1)):
 * x [n][3][H][W] fp32 (or raw uint8 with mean_std, normalised while the patch is staged), W == 128, H % 4 == 0;
 * y [n*(H/4)*(W/4)][64] bf16 = the POOLED map; the stem map itself never reaches HBM.  wp: grl_stem_pack_weight_bf16. */
int grl_stem_pool_bf16(const void* x, int x_is_u8, const float* mean_std, const float* scale, const float* shift, void* y,
                       int n, int H, int W, const void* wp, void* stream);

/* Layer 1's 3x3 / stride 1 convolution (64 -> 64 channels, maps W == 32 wide, H % 8 == 0; resnets1.py:79-81) + folded
 * BatchNorm + optional ReLU, bf16 storage: weights LDS-resident, every input pixel staged once per tile (fuse_bf16.hip).
 * x [n_img][H][W][64] bf16, w [64][9*64] bf16 packed tap-major (grl_pack_conv_weight + grl_cast_bf16), y [n_img*H*W][64]. */
int grl_conv3x3_c64_bf16(const void* x, const void* w, const float* scale, const float* shift, void* y, int n_img, int H, int W,
                         int relu, void* stream);

/* The same fusion for the EXACT-fp32 trunk (BASELINE configs[1]; fuse_f32.hip): all operands fp32.  Results are BIT-IDENTICAL
 * to grl_conv_gemm_f32 (GRL_MATH_F32, one chain) run on conv3 (+res, ReLU) and then on conv1' -- the transposed MFMA
 * keeps that kernel's documented k-ordered fmaf chain.  w1n is the plain [Pn][C4] weight (no permutation).
 * Shapes: (P, C4) = (64, 256) with Pn in {0, 64, 128}; (128, 512) with Pn in {0, 128}. */
typedef struct GrlBneckTailF32 {
    const float* t2;        /* [M][P]                                                       */
    const float* w3;        /* [C4][P]                                                      */
    const float* scale3;    /* [C4] or NULL (= 1)                                           */
    const float* shift3;    /* [C4] or NULL (= 0)                                           */
    const float* res;       /* [M][C4]                                                      */
    float*       y;         /* [M][C4] out                                                  */
    const float* w1n;       /* [Pn][C4] or NULL                                             */
    const float* scale1n;   /* [Pn] or NULL                                                 */
    const float* shift1n;   /* [Pn] or NULL                                                 */
    float*       u;         /* [M][Pn] out, or NULL                                         */
    int32_t M, P, C4, Pn;
} GrlBneckTailF32;
int grl_bottleneck_tail_f32(const GrlBneckTailF32* desc, void* stream);
int grl_bottleneck_tail_f32_supported(int P, int C4, int Pn);

/* ------------------------------------------------------------------------------------------------------------------
 * Frame decode on the device (round 6).  Replaces the per-frame
 * `Image.open(img_path).convert('RGB')` of reid/data/video_loader.py:124-141 (and :91-96, :108-113): baseline JPEG
 * -> uint8 RGB, BIT-IDENTICAL to Pillow / libjpeg-turbo with libjpeg's defaults (ISLOW integer IDCT, fancy
 * upsampling): 0xFF00 unstuffing, Huffman decoding (one 256-lane workgroup per frame over self-synchronising
 * subsequences of the bit stream; one lane per frame for scans with restart intervals or frames too large for the
 * workgroup form), dequantisation + jidctint's integer IDCT (one lane per 8 x 8 block), triangle-filter chroma
 * upsampling + YCbCr -> RGB (one lane per pixel).
 * Scope: 8-bit baseline / extended-sequential Huffman, one interleaved scan whose selectors list the components in
 * SOF order, 1 or 3 components (unique ids), luma sampling 1x1, 2x1 or 2x2 (4:4:4, 4:2:2, 4:2:0 -- MARS' frames are
 * 256 x 128 4:2:0), table ids 0..1, 8-bit quantisers (Pq = 0, as T.81 requires with 8-bit samples), restart
 * intervals, width x height <= 64 Mpx.  Colour space by libjpeg's rule: JFIF -> YCbCr; else an Adobe marker decides
 * (transform 0 -> RGB, 1 -> YCbCr); else component ids 'R', 'G', 'B' -> RGB; else YCbCr.  Adobe transform 2 (YCCK)
 * is refused even where a JFIF marker would make libjpeg read YCbCr.  The IDCT is jidctint.c's in the integer widths of
 * libjpeg-turbo's SIMD form, which Pillow runs (16-bit dequantisation and sums, saturating packs): bit-identical for
 * any coefficient under any 8-bit quantiser, also past the values an encoder of 8-bit samples writes.
 * Anything else is refused by the parser with GRL_EUNSUPPORTED: the caller (grl_amd/reid/data/jpeg.py) says so
 * loudly -- it does not decode on the host behind the caller's back.
 */
#define GRL_EUNSUPPORTED -3  /* a valid JPEG outside the scope above (progressive, arithmetic, CMYK, 12-bit, 4:4:0 ...) */

typedef struct GrlJpegFrame {      /* one parsed frame: filled on the host by grl_jpeg_parse, read by the kernels */
    uint32_t scan_off;             /* entropy-coded segment: offset into the batch's byte buffer, length */
    uint32_t scan_len;
    uint16_t width, height;
    uint16_t restart_interval;     /* MCUs between RSTn markers, 0 = none */
    uint8_t  ncomp, hmax, vmax, rgb;   /* rgb: components are R, G, B (libjpeg's rule above): no colour conversion */
    uint8_t  hs[4], vs[4];         /* sampling factors per component */
    uint8_t  tq[4], td[4], ta[4];  /* quantisation / DC / AC table of each component */
    uint16_t tabset;               /* index of this frame's Huffman table set inside its batch (grl_jpeg_assign_tables) */
    uint8_t  pad_[8];              /* (q starts at byte 48; sizeof == 2160 == 16 * 135: 16-byte loads of q rows) */
    uint16_t q[4][64];             /* quantisation tables, natural (row-major) order */
    int32_t  maxcode[4][18];       /* Huffman tables [DC0, DC1, AC0, AC1]: largest code of each length (-1: none) */
    int32_t  valoff[4][18];        /*   symbol index = code + valoff[length] */
    uint8_t  vals[4][256];         /*   symbols in code order */
} GrlJpegFrame;

/* HOST function (no GPU call): parse the headers of ONE JPEG stream `data[0..len)` that will sit at byte `base_off` of
 * the batch buffer.  Returns GRL_OK, GRL_EINVAL (not a JPEG / truncated) or GRL_EUNSUPPORTED. */
int grl_jpeg_parse(const uint8_t* data, int64_t len, int64_t base_off, GrlJpegFrame* out);
/* test / A-B hook: 1 (default) = entropy decoding by one 256-lane workgroup per frame (self-synchronising subsequences),
 * 0 = one lane per frame; -1 = query.  Same coefficients either way.  Returns the previous setting. */
int grl_jpeg_parallel_mode(int on);
/* HOST function: number the Huffman table sets of a batch (frames[i].tabset).  Up to 4 distinct sets get shared
 * look-ahead tables in LDS (frames of one encoder share ONE set); beyond that every frame keeps its own.  Returns
 * the number of sets (> 0) or a negative GRL_E* code.  Call after grl_jpeg_parse, before the descriptors are copied. */
int grl_jpeg_assign_tables(GrlJpegFrame* frames, int n);
/* HOST function: grl_jpeg_parse for the n streams of one batch buffer (stream i = buf[offsets[i] .. offsets[i+1])), then
 * grl_jpeg_assign_tables.  On failure *bad_index is the offending frame and the return value its code. */
int grl_jpeg_parse_batch(const uint8_t* buf, const int64_t* offsets, int n, GrlJpegFrame* frames, int* bad_index);
/* bytes of device scratch grl_jpeg_decode_batch needs for the n parsed frames of a batch (coefficients, planes,
 * look-ahead tables, unstuffed streams); GRL_EUNSUPPORTED for a frame above the size caps */
int64_t grl_jpeg_workspace_bytes(const GrlJpegFrame* frames_host, int n);
/* n frames of ONE geometry (width, height, components, sampling: as frames[0]; frames_host is checked) ->
 * out uint8 [n][3][height][width] (planar RGB: the layout the clip tensors [B][T][3][H][W] have).
 * bytes: the concatenated streams (device) -- the buffer grl_jpeg_parse's base_off values refer to: it must hold
 * every frames[i].scan_off + scan_len (like every pointer of this ABI its extent is the caller's contract; the kernels
 * read no byte outside the scans); frames_dev: the n parsed descriptors (device copy of frames_host). */
int grl_jpeg_decode_batch(const uint8_t* bytes, const GrlJpegFrame* frames_dev, const GrlJpegFrame* frames_host, int n,
                          uint8_t* out, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GRL_HIP_H */
