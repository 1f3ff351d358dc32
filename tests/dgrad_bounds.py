"""Shapes, inputs, first-order rounding-error bounds and fp32 restatements of the summation order for the convolution
backward of train_engine.conv_param_and_input_grads -- shared by test_dgrad_ref_cpu.py (no GPU) and
test_gpu_dgrad_float64.py.  U, SAFETY, check, RATIOS, dump_ratios, K_GEMM_STATS and bf16_round are bn_bounds' own,
rng_for, f32 and near are head_bounds'.

Bounds are derived per element, none is fitted (u = 2^-24; the library is built with -ffp-contract=off and the exact-fp32
MFMA neither fuses nor reorders a product into its accumulator):
  a GEMM output is a sum of K exact-to-one-rounding fp32 products accumulated in fp32 in SOME order -- one chain, or the
  K-blocked kernels' 512-k segments added afterwards --: every term passes through at most K roundings (its product, then at
  most K - 1 additions): K u abs_terms.  K is the number of terms the route really sums: cout (routes A, B), 9 cout (C, E),
  (1 + py)(1 + px) cout for the parity class (py, px) of route D.  (Read from train_engine.conv_param_and_input_grads: the K
  argument of each gemm() call.  Taps that fall outside the map and the zeros of route E's stuffed operand add exact zeros.)
  Each further fp32 addition adds u |result|: `+ res` in the GEMM epilogue (gemm_f32.hip: `v = v * sc + sh` with sc = 1,
  sh = 0 is exact, then `v += res`), grl_dilate2 mode 1's `v += up[i]` (train.hip dilate2_kernel).
  Weight gradient: M = n Ho Wo terms per element, in any order (split over workgroups and reduced): M u abs_terms, and
  u |result| for the accumulation into the parameter's gradient buffer.
  Fused epilogue (gemm_f32.hip, `if (p.bn_z)`): g carries its GEMM bound where the mask keeps it and is exactly 0 elsewhere;
  a tile's column sums are K_GEMM_STATS = 34 additions deep (a lane over at most 32 rows `ssum += v`, the xor-shuffle levels
  and the two wave rows through LDS: bn_bounds), the test adds the tiles in float64; sum g * xhat: xhat = fl(fl(z - mean) *
  invstd) and the product round three times per term (`ssq += v * (zc * bis)`), xhat itself is 2 u relative; both sums
  also carry the sum of their terms' own bounds.
SAFETY (2: the dropped u^2 terms) is applied once, at the end.

bf16 storage: every value rounded to bf16 adds 2^-9 |value|; with SAFETY that is 2^-8 |value|, exactly the unit roundoff of
8 significand bits, so these stages may come close to a ratio of 1 where a value sits just above a power of two.  ASSUMED, not read:
that the bf16-storage GEMM (MFMA bf16 products, fp32 accumulation) forms each product exactly -- a product of two 8-bit
significands has 16 bits and fits fp32 -- so that the fp32 rule above holds for its accumulator."""
import numpy as np

import dgrad_ref as R
from bn_bounds import U, SAFETY, check, RATIOS, dump_ratios, K_GEMM_STATS, bf16_round                        # noqa: F401
# (bn_bounds.b_sum_g / b_sum_gx are not used for the fused sums: their depth is k_bwd_reduce(C), grl_bn_bwd's own reduce, 12 to
#  34 additions; the GEMM epilogue is K_GEMM_STATS = 34 deep whatever C is -- fused_bounds below states their rule at that depth)
from head_bounds import rng_for, f32, near                                                                    # noqa: F401

UB = 2.0 ** -9                  # one rounding to bf16, relative
KBLOCK_ROWS = 256               # train_engine.gemm: K-blocked accumulation in the backward iff the GEMM's M <= 256 ...
KBLOCK_K = 512                  # ... and gemm_f32.hip launch_math: the segmented kernel only runs for K > SEG_STAGES * BK = 512
GRID_CAP = 8192 * 256           # float4 items one pass of train.hip's grid_even launch covers (grid_for caps at 8192 x 256)

# (cin, cout, k, stride, H, W, n, why).  `rows` in the comments is the M of the data-gradient GEMM (input rows for routes A,
# C, E; OUTPUT rows for B and D, whose GEMMs run at output resolution), K its K.  'seg' marks the entries that reach the
# K-blocked (segmented) kernel: rows <= 256 and K > 512; 'chain' the ones with K > 512 that must not.
SWEEP = (
    (32, 32, 1, 1, 3, 5, 1, 'A: 15 rows, one ragged 64-row tile'),
    (64, 96, 1, 1, 13, 7, 3, 'A: 273 rows > 256, past two 128-row tiles'),
    (32, 64, 1, 1, 4, 4, 2, 'A: 32 rows, cout = 64: the A entry the bf16-storage GEMM accepts (K % 64 == 0)'),
    (64, 96, 1, 2, 6, 4, 2, 'B: even map, 12 output rows'),
    (64, 96, 1, 2, 7, 5, 2, 'B: odd map, H == 2 Ho - 1, W == 2 Wo - 1'),
    (32, 64, 1, 2, 24, 24, 2, 'B: 288 output rows > 256 (the list had no B entry on that side)'),
    (32, 64, 3, 1, 5, 3, 3, 'C: 45 rows, K = 576: seg'),
    (96, 32, 3, 1, 9, 13, 2, 'C: 234 rows <= 256, cin = 96: a ragged second 64-column tile'),
    (96, 32, 3, 1, 9, 13, 3, 'C: 351 rows > 256'),
    (64, 64, 3, 1, 17, 17, 1, 'C: 289 rows > 256, K = 576: chain (the list had no K > 512 entry past 256 rows, and no C entry '
                              'whose weight gradient the library accepts: cin % 64 == 0)'),
    (32, 32, 3, 2, 2, 2, 1, 'D: Ho = Wo = 1, every a + 1 tap is outside the map'),
    (64, 32, 3, 2, 6, 10, 3, 'D: 45 output rows'),
    (32, 96, 3, 2, 10, 26, 1, 'D: 260 input rows, 65 output rows'),
    (32, 32, 3, 2, 24, 46, 1, 'D: 276 OUTPUT rows > 256 (the GEMMs of route D run at output resolution)'),
    (32, 160, 3, 2, 4, 4, 1, 'D: class (1, 1) has K = 640: seg; classes (0, 1), (1, 0): K = 320'),
    (64, 64, 3, 2, 4, 6, 2, 'D: 12 output rows, cout = 64: the D entry the bf16-storage GEMM accepts (C % 64 == 0)'),
    (32, 32, 3, 2, 7, 5, 2, 'E: odd x odd, 70 rows'),
    (64, 64, 3, 2, 9, 4, 1, 'E: odd x even, 36 rows, K = 576: seg'),
    (32, 32, 3, 2, 1, 1, 5, 'E: a 1 x 1 map'),
    (32, 32, 3, 2, 17, 17, 1, 'E: 289 rows > 256'),
)
CASES = tuple(c[:7] for c in SWEEP)
CLASSES = ('a', 'b', 't')
TAG_PIXELS = ('corner', 'last row', 'last column', 'interior')
# the subset the 128-row LDS-DMA conv gather (gemm_f32.hip: CAN_DMA_CONV, the per-row tap mask `cmask`) is run on through
# grl_gemm_force_tile(128, 64): the tile rule never picks a 128-row tile below 448 tiles, i.e. ~57 000 rows
FORCED_TILE_CASES = tuple(c for c in CASES if c[2] == 3 and c[:7] in (
    (32, 64, 3, 1, 5, 3, 3), (96, 32, 3, 1, 9, 13, 3), (32, 32, 3, 2, 2, 2, 1), (64, 32, 3, 2, 6, 10, 3), (32, 32, 3, 2, 7, 5, 2),
    (32, 32, 3, 2, 1, 1, 5)))


def route(k, stride, H, W):
    """conv_param_and_input_grads' rule restated: which of the five data-gradient routes a layer takes"""
    Ho, Wo = (H, W) if (k == 1 and stride == 1) else R.out_hw(H, W, k, stride)
    if k == 1:
        return 'A' if stride == 1 else 'B'
    if stride == 1:
        return 'C'
    if k == 3 and stride == 2 and H == 2 * Ho and W == 2 * Wo:
        return 'D'
    return 'E'


def geometry(case):
    cin, cout, k, stride, H, W, n = case
    Ho, Wo = (H, W) if (k == 1 and stride == 1) else R.out_hw(H, W, k, stride)
    return Ho, Wo, k // 2


def gemm_calls(case):
    """(M, N, K) of every data-gradient GEMM the route issues, in order"""
    cin, cout, k, stride, H, W, n = case
    Ho, Wo, _ = geometry(case)
    r = route(k, stride, H, W)
    if r == 'A':
        return [(n * H * W, cin, cout)]
    if r == 'B':
        return [(n * Ho * Wo, cin, cout)]
    if r in 'CE':
        return [(n * H * W, cin, 9 * cout)]
    return [(n * Ho * Wo, cin, (1 + py) * (1 + px) * cout) for py in (0, 1) for px in (0, 1)]


def wgrad_accepts(case):
    """grl_conv_wgrad_f32 (train.hip): a conv-mode weight gradient needs C = cin % 64 == 0 -- every convolution of the model
    behind the stem has it; the dense one of a 1x1 stride-1 layer takes any cin % 4.  The data-gradient entries with cin = 32
    or 96 (a GEMM narrower than its 64-column tile, a ragged second tile) run with the weight gradient left to a stack that
    is not full yet (conv_param_and_input_grads' `wstack`), as a layer inside a _WgradStack does."""
    cin, cout, k, stride, H, W, n = case
    return (k == 1 and stride == 1) or cin % 64 == 0


def takes_segmented_kernel(M, K):
    return M <= KBLOCK_ROWS and K > KBLOCK_K


def launches(case, accumulate, fused=False):
    """the launch sequence of the route, as the table of the issue names it: ('gemm', conv?, res?, stats?) and
    ('grl_dilate2', mode, oy_off, ox_off); the weight re-layouts (cached per tape) come first"""
    cin, cout, k, stride, H, W, n = case
    r = route(k, stride, H, W)
    acc = bool(accumulate)
    if r == 'A':
        return [('grl_transpose',), ('gemm', False, acc, fused)]
    if r == 'B':
        return [('grl_transpose',), ('gemm', False, False, False), ('grl_dilate2', 1 if acc else 0, 0, 0)]
    if r == 'C':
        return [('grl_pack_dgrad_weight',), ('gemm', True, acc, fused)]
    if r == 'D':
        out = []
        for py in (0, 1):
            for px in (0, 1):
                out += [('gemm', True, False, False), ('grl_dilate2', 1 if acc else 2, py, px)]
        return out
    return [('grl_dilate2', 0, 0, 0), ('grl_pack_dgrad_weight',), ('gemm', True, acc, False)]


# ----------------------------------------------------------------------------------------------------------------------
# inputs
def tag_pixel(case, index):
    """the output pixel (img, oy, ox) class (t) lights: corner, last row, last column, interior in turn over the sweep"""
    Ho, Wo, _ = geometry(case)
    n = case[6]
    which = TAG_PIXELS[index % 4]
    oy, ox = {'corner': (0, 0), 'last row': (Ho - 1, Wo // 2), 'last column': (Ho // 2, Wo - 1),
              'interior': (Ho // 2, Wo // 2)}[which]
    return n - 1, oy, ox, which


def make_inputs(case, cls):
    """fp32 dz[n Ho Wo][cout], w[cout][cin][k][k], x[n H W][cin], G0[n H W][cin].
    (a) dz ~ N(0, 1), w ~ N(0, 1) / sqrt(k k cin);
    (b) cancelling: w[:, c] equal across o up to 1e-3 and every row of dz sums to ~0 over o: |dx| << abs_terms;
    (t) tagged: dz of (a), zero except at ONE output pixel (tag_pixel): every nonzero of dx names one tap of that pixel."""
    cin, cout, k, stride, H, W, n = case
    Ho, Wo, _ = geometry(case)
    r = rng_for('dgrad', *case, cls)
    dz = r.standard_normal((n * Ho * Wo, cout))
    w = r.standard_normal((cout, cin, k, k)) / np.sqrt(k * k * cin)
    if cls == 'b':
        w = near(r, np.broadcast_to(w[:1], w.shape))
        dz = dz - dz.mean(1, keepdims=True)
    if cls == 't':
        img, oy, ox, _ = tag_pixel(case, CASES.index(tuple(case)))
        keep = np.zeros((n, Ho, Wo, 1))
        keep[img, oy, ox] = 1.0
        dz = (dz.reshape(n, Ho, Wo, cout) * keep).reshape(-1, cout)
    return dict(dz=f32(dz), w=f32(w), x=f32(r.standard_normal((n * H * W, cin))), g0=f32(r.standard_normal((n * H * W, cin))))


def tagged_footprint(case, index):
    """number of input pixels the tagged output pixel reaches: the taps (ky, kx) whose input pixel lies inside the map"""
    cin, cout, k, stride, H, W, n = case
    _, oy, ox, _ = tag_pixel(case, index)
    pad = k // 2
    ys = [ky for ky in range(k) if 0 <= stride * oy - pad + ky < H]
    xs = [kx for kx in range(k) if 0 <= stride * ox - pad + kx < W]
    return len(ys) * len(xs)


def to_bf16(a):
    return f32(bf16_round(a))


# ----------------------------------------------------------------------------------------------------------------------
# bounds
def k_terms(case):
    """[n H W][1]: the number of terms the route sums into each input pixel's gradient (the K of the GEMM that owns it)"""
    cin, cout, k, stride, H, W, n = case
    r = route(k, stride, H, W)
    if r in 'AB':
        return np.full((n * H * W, 1), float(cout))
    if r in 'CE':
        return np.full((n * H * W, 1), 9.0 * cout)
    t = np.zeros((n, H, W, 1))
    for py in (0, 1):
        for px in (0, 1):
            t[:, py::2, px::2] = (1 + py) * (1 + px) * cout
    return t.reshape(-1, 1)


def e_dx(case, abs_terms, result, accumulate):
    """fresh: K u abs_terms.  accumulate: + u |result| for the one further addition (`+ res` in the epilogue for A, C, E;
    grl_dilate2 mode 1 for B and D) -- only where a term arrives: elsewhere G0 + 0 is exact, or the pixel is not touched."""
    e = k_terms(case) * U * abs_terms
    if accumulate:
        e = e + np.where(abs_terms > 0, U * np.abs(result), 0.0)
    return e


def b_dx(case, abs_terms, result, accumulate):
    return SAFETY * e_dx(case, abs_terms, result, accumulate)


def b_dw(M, abs_terms, result):
    return SAFETY * (M * U * abs_terms + U * np.abs(result))


def bf16_roundings(case, accumulate):
    """roundings to bf16 on the way to an element of dx, counted from conv_param_and_input_grads with bf16 tensors: the
    GEMM's store (every route: into dx for A, C, E, into `small` for B and D -- for those it is the only store when dx is
    fresh, grl_dilate2_bf16 copies), and mode 1's sum v + up rounded again (B, D, accumulate)."""
    r = route(case[2], case[3], case[4], case[5])
    return 1 + (1 if (accumulate and r in 'BD') else 0)


def b_dx_bf16(case, abs_terms, result, term, accumulate):
    """fp32 bound + 2^-9 |value| per rounding to bf16: the GEMM's stored value (`term` for B and D, whose GEMM output is the
    convolution term alone; the result for A, C, E, whose epilogue adds res in fp32 before the one store) and, for B and D
    in the accumulate form, the sum."""
    e = e_dx(case, abs_terms, result, accumulate)
    r = route(case[2], case[3], case[4], case[5])
    touched = abs_terms > 0
    if r in 'BD':
        e = e + UB * np.abs(term) + (np.where(touched, UB * np.abs(result), 0.0) if accumulate else 0.0)
    else:
        e = e + (np.where(touched, UB * np.abs(result), 0.0) if accumulate else UB * np.abs(term))
    return SAFETY * e


def bf16_accepts(case):
    """validate() of gemm_f32.hip for the bf16-storage datapath: K % 64 == 0 and, conv mode, C % 64 == 0 (C = the per-tap
    channel count = cout); lda, ldw % 8 hold whenever these do.  Route D's class (0, 0) has K = cout."""
    return case[1] % 64 == 0


def fused_bounds(ep, K, abs_terms, has_res):
    """g, sum g, sum g xhat of the fused epilogue against dgrad_ref.fused_epilogue (see the module docstring; the tiles'
    partial sums are added in float64 by the caller, so nothing is charged across tiles)."""
    e_v = K * U * abs_terms + (U * np.abs(ep['v']) if has_res else 0.0)
    e_g = np.where(ep['mask'], e_v, 0.0)
    g, xh = ep['g'], ep['xhat']
    gx = g * xh
    e_sg = K_GEMM_STATS * U * np.abs(g).sum(0) + e_g.sum(0)
    e_sgx = (K_GEMM_STATS + 3) * U * np.abs(gx).sum(0) + (e_g * np.abs(xh)).sum(0)
    return dict(g=SAFETY * e_g, sum_g=SAFETY * e_sg, sum_gx=SAFETY * e_sgx, e_g=e_g)


def b_mask_margin(z, mean, mscale, mbeta):
    """how far the fp32 pre-activation fl(fl(fl(z - mean) * mscale) + mbeta) can be from the float64 one: three roundings on
    |z - mean| |mscale| + |mbeta| (times SAFETY)"""
    zc = np.abs(R.f64(z) - R.f64(mean)[None, :])
    return SAFETY * 3 * U * (zc * np.abs(R.f64(mscale))[None, :] + np.abs(R.f64(mbeta))[None, :])


# ----------------------------------------------------------------------------------------------------------------------
# fp32 restatements of a sum of K products in the orders the bounds cover (numpy, CPU): the bounds are satisfiable
F = np.float32


def dot_sequential_f32(a, b):
    """[M][K] . [K][N] with one fp32 chain per output, k ascending"""
    a, b = F(a), F(b)
    acc = np.zeros((a.shape[0], b.shape[1]), F)
    for k in range(a.shape[1]):
        acc = acc + a[:, k:k + 1] * b[k:k + 1, :]
    return acc


def dot_blocked_f32(a, b, block=32):
    """... in blocks of `block` k, each its own chain from zero, the block sums then added in sequence (the K-blocked
    kernels' shape, with a short block so that small K has several)"""
    a, b = F(a), F(b)
    tot = np.zeros((a.shape[0], b.shape[1]), F)
    for k0 in range(0, a.shape[1], block):
        tot = tot + dot_sequential_f32(a[:, k0:k0 + block], b[k0:k0 + block])
    return tot


def dot_numpy_f32(a, b):
    return F(a) @ F(b)
