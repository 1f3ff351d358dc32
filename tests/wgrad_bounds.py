"""Host rules, sweep, inputs, first-order rounding-error bounds and fp32 restatements of the summation order for the
weight-gradient kernels of grl_amd/csrc/train.hip (grl_conv_wgrad_f32, grl_stem_wgrad) -- shared by test_wgrad_ref_cpu.py
(no GPU) and test_gpu_wgrad_float64.py.  U, SAFETY, check, RATIOS, dump_ratios and bf16_round are bn_bounds' own, rng_for,
f32 and near are head_bounds'.

Bounds are derived per element, none is fitted (u = 2^-24; the library is built with -ffp-contract=off and the exact-fp32
MFMA neither fuses nor reorders a product into its accumulator).  SAFETY (2: the dropped second-order terms) is the only
factor and is applied once, at the end.
  fp32 datapath: the pixel range is cut into `real_splits` ranges of `chunk` rows; a workgroup sums its range into its slab in
  one fp32 chain per element, wgrad_reduce_kernel adds the slabs in slab order.  A term passes through its product's
  rounding, at most min(terms, chunk) - 1 additions of its range's chain (a zero row adds exactly, so only the non-zero terms
  count) and at most real_splits additions of the slab sum: (min(terms, chunk) + real_splits) u abs_terms.  The accumulate
  form `dw = dw + s` adds u |result| (where no term arrives, dw + 0 is exact: the bound is 0 and the value must not move).
  bf16 operands in memory: the same rule.  ASSUMED, as dgrad_bounds assumes it of the bf16-storage GEMM, not read: that
  v_mfma_f32_32x32x16_bf16 forms each product of two bf16 values exactly -- two 8-bit significands give 16 bits, which fit
  fp32 -- and adds it into the fp32 accumulator with one rounding per addition at the worst, in some order.
  math = bf16 on fp32 operands (split_store, MATH == 1): both operands are rounded to bf16; the term is charged
  (2 2^-9 + 2^-18) |a b|, then the rule above.  (2^-9 is the convention of dgrad_bounds' UB.  bf16 keeps 8 significand bits,
  so a rounding can reach 2^-8 |v|, at significands just above a power of two; SAFETY makes the charged 2 2^-9 exactly that
  first-order worst case, 2 2^-8, and the depth term covers what is left unless both operands sit at that extreme.)
  math = bf16x3 (split_store, MATH == 3): hi = bf16(v), lo = bf16(v - hi).  With ub = 2^-8, the unit roundoff of 8
  significand bits: v - hi is exact in fp32 and at most ub |v|, so v = hi + lo + r with |lo| <= ub (1 + ub) |v| and
  |r| <= ub^2 |v|.  The kernel adds hi hi + lo hi + hi lo and drops lo lo: a b - (those three) = al bl + ah rb + al rb +
  ra b, at most 3 ub^2 (1 + 2 ub) |a b|.  Three accumulations per term, each of an exact product, on partial terms that sum
  to at most ((1 + ub)^2 + 2 ub (1 + ub)) |a b| <= (1 + 5 ub) |a b|:
  (3 min(terms, chunk) + real_splits) u (1 + 5 ub) abs_terms on top of the representation error.
  Stem (stem_wgrad_kernel): a wave adds its quarter (32 pixels) of every tile its workgroup takes into one chain per lane --
  32 trips additions at the most --, the four quarters are added in order through LDS (3 additions) and the workgroups'
  slabs in slab order (at most `wgs` additions): min(terms, 32 trips + 3 + wgs) u abs_terms; products are exact fp32
  products rounded once in every math mode (a bf16 dz is converted exactly)."""
from collections import namedtuple
import math

import numpy as np

import wgrad_ref as R
from bn_bounds import U, SAFETY, check, RATIOS, dump_ratios, bf16_round                        # noqa: F401
from head_bounds import rng_for, f32, near                                                    # noqa: F401

UB = 2.0 ** -9                  # one rounding to bf16 as dgrad_bounds charges it (SAFETY doubles it)
UB8 = 2.0 ** -8                 # the unit roundoff of bf16's 8 significand bits: the bf16x3 split is derived with it
F = np.float32
MATH_F32, MATH_BF16, MATH_BF16X3 = 0, 1, 3          # GrlWgrad.math (include/grl_hip.h)

# kind: 'dense' | 'conv' | 'stem'.  geom: conv (n, H, W, C, k, stride, pad); stem (n, H, W); dense None.
# b16: both operands bf16 in memory (dense, conv: GrlWgrad.in_bf16) or a bf16 dz (stem).
E = namedtuple('E', 'kind M N K ldz ldx k_out geom math b16 why')


def _dense(M, N, K, why, ldz=0, ldx=0, k_out=0, math=MATH_F32, b16=0):
    return E('dense', M, N, K, ldz or N, ldx or K, k_out, None, math, b16, why)


def _conv(n, H, W, C, N, k, stride, pad, why, math=MATH_F32, b16=0):
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return E('conv', n * Ho * Wo, N, k * k * C, N, C, 0, (n, H, W, C, k, stride, pad), math, b16, why)


def _stem(n, H, W, b16, why):
    return E('stem', n * (H // 2) * (W // 2), 64, 160, 64, 0, 147, (n, H, W), MATH_F32, b16, why)


SWEEP = (
    # dense fp32: the four tile shapes
    _dense(65, 40, 72, '64 x 64 tiles, ragged in N and K, three stages, the last one 1 row'),
    _dense(65, 64, 128, '64 x 128 tile'),
    _dense(65, 136, 160, '128 x 64: a ragged second row tile, a 32-column last tile, k_out = 147', k_out=147),
    _dense(65, 128, 256, '128 x 128, two full tiles'),
    _dense(65, 200, 128, '128 x 128, ragged second row tile'),
    _dense(33, 40, 72, 'ldz > N and ldx > K', ldz=48, ldx=80),
    # dense fp32: the pixel count
    _dense(1, 40, 72, 'M = 1'),
    _dense(2, 40, 72, 'M = 2: one MFMA k-step'),
    _dense(31, 40, 72, 'M = 31: one ragged stage'),
    _dense(32, 40, 72, 'M = 32: one full stage'),
    _dense(33, 40, 72, 'M = 33: a second stage of one row'),
    _dense(257, 128, 256, '2 splits, chunk 160'),
    _dense(257, 40, 72, '2 splits on 64 x 64 tiles'),
    _dense(513, 128, 256, '3 splits'),
    _dense(1000, 128, 256, '4 splits: the unrolled-by-4 loop of the reduce, no tail'),
    _dense(1025, 128, 256, '5 splits: the unrolled loop and a tail of one'),
    _dense(2049, 128, 256, '9 splits, the last one a single row'),
    # conv fp32, lin (same-size stride-1 window, Wo divides 32): all four tile shapes
    _conv(2, 4, 16, 64, 40, 3, 1, 1, 'lin, 64 x 64'),
    _conv(1, 2, 32, 128, 64, 3, 1, 1, 'lin, 64 x 128, Wo = 32: one image row per stage'),
    _conv(2, 16, 4, 64, 136, 3, 1, 1, 'lin, 128 x 64, Wo = 4: eight image rows per stage'),
    _conv(5, 4, 16, 128, 136, 3, 1, 1, 'lin, 128 x 128, M = 320: the split boundary lies inside image 2'),
    # conv fp32, generic
    _conv(2, 11, 6, 64, 40, 3, 1, 1, 'generic: Wo = 6 does not divide 32'),
    _conv(2, 16, 16, 64, 64, 3, 2, 1, 'generic: 3x3 s2 p1, 16 x 16 -> 8 x 8'),
    _conv(3, 16, 16, 128, 136, 3, 2, 1, 'generic on 128 x 128 tiles, 192 pixels'),
    # conv fp32, small_img (fewer than 64 output pixels per image)
    _conv(4, 8, 8, 64, 40, 1, 2, 0, '1x1 s2 p0, 8 x 8 -> 4 x 4: 16 output pixels, so small_img, not generic'),
    _conv(3, 4, 8, 64, 40, 3, 1, 1, 'small_img: 32 pixels, one image per stage'),
    _conv(9, 3, 3, 64, 64, 3, 1, 1, 'small_img: 9 pixels, several images per stage'),
    _conv(5, 1, 1, 64, 40, 3, 1, 1, 'small_img: 1 x 1 maps, only the centre tap is inside'),
    # XCD tile map
    _dense(40, 512, 2048, '4 x 16 tiles: tile map mode 1'),
    _dense(40, 2048, 512, '16 x 4 tiles: tile map mode 2'),
    # math = bf16 / bf16x3 on fp32 operands
    _dense(40, 128, 128, 'bf16 MFMA, one tile', math=MATH_BF16),
    _dense(40, 128, 128, 'bf16x3, one tile', math=MATH_BF16X3),
    _dense(300, 136, 256, 'bf16 MFMA, ragged N, 2 splits', math=MATH_BF16),
    _dense(300, 136, 256, 'bf16x3, ragged N, 2 splits', math=MATH_BF16X3),
    _conv(2, 4, 16, 128, 128, 3, 1, 1, 'bf16 MFMA, implicit GEMM', math=MATH_BF16),
    _conv(2, 4, 16, 128, 128, 3, 1, 1, 'bf16x3, implicit GEMM', math=MATH_BF16X3),
    _dense(40, 64, 128, 'math = bf16 on a 64 x 128 tile: falls back to the exact-fp32 kernel', math=MATH_BF16),
    _dense(40, 64, 128, 'math = bf16x3 on a 64 x 128 tile: falls back to the exact-fp32 kernel', math=MATH_BF16X3),
    # bf16 operands in memory, 128 x 128 tile
    _dense(33, 64, 64, 'bf16-in, half a tile each way', b16=1),
    _dense(260, 264, 520, 'bf16-in, N K < 2^19: 128-wide, ragged both, 2 splits', b16=1),
    _dense(65, 64, 160, 'bf16-in, k_out = 147', k_out=147, b16=1),
    _conv(2, 4, 16, 64, 64, 3, 1, 1, 'bf16-in, C = 64: two taps per tile', b16=1),
    _conv(2, 16, 16, 64, 64, 3, 2, 1, 'bf16-in, 3x3 s2', b16=1),
    _conv(4, 8, 8, 64, 64, 1, 2, 0, 'bf16-in, 1x1 s2', b16=1),
    # bf16 operands in memory, 256 x 256 tile with its three-buffer ring
    _dense(20, 520, 1032, 'bf16-in 256: ragged both, 1 stage', b16=1),
    _dense(64, 520, 1032, 'bf16-in 256: 2 stages', b16=1),
    _dense(96, 520, 1032, 'bf16-in 256: 3 stages, the ring wraps', b16=1),
    _dense(100, 520, 1032, 'bf16-in 256: 4 stages, the last one ragged', b16=1),
    _dense(257, 520, 1032, 'bf16-in 256: 2 splits', b16=1),
    _conv(2, 4, 8, 64, 1024, 3, 1, 1, 'bf16-in 256: four taps per tile, a 64-column last tile', b16=1),
    _conv(5, 4, 16, 128, 512, 3, 1, 1, 'bf16-in 256: two taps per tile, 2 splits', b16=1),
    # stem
    _stem(1, 2, 2, 0, 'one output pixel'), _stem(1, 2, 2, 1, 'one output pixel, bf16 dz'),
    _stem(1, 16, 32, 0, 'one full tile'), _stem(1, 16, 32, 1, 'one full tile, bf16 dz'),
    _stem(2, 36, 20, 0, 'ragged: a two-row third tile row, 10 columns'), _stem(2, 36, 20, 1, 'the same, bf16 dz'),
    _stem(1, 18, 34, 0, 'one-row and one-column tiles'), _stem(1, 18, 34, 1, 'the same, bf16 dz'),
    _stem(520, 16, 32, 0, '520 tiles: workgroups 0..7 take two'), _stem(520, 16, 32, 1, 'the same, bf16 dz'),
    _stem(1030, 6, 10, 0, '1030 ragged tiles: workgroups 0..5 take three'), _stem(1030, 6, 10, 1, 'the same, bf16 dz'),
)
TAG_PIXELS = ('corner', 'last row', 'last column', 'interior')
MUTATIONS = ('drop_last_row', 'late_stage', 'shift_tap', 'wrap_tap', 'no_lo_hi', 'xcd_swap', 'stale_patch')


# ----------------------------------------------------------------------------------------------------------------------
# the host rules of train.hip, restated (line numbers: grl_amd/csrc/train.hip)
def out_hw(e):
    n, H, W, C, k, stride, pad = e.geom
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def wgrad_tile(e):
    """wgrad_tile (train.hip:1941): bf16-in 256 x 256 iff N >= 256, K >= 256 and N K >= 2^19, else 128 x 128; fp32 operands
    bm = 128 iff N >= 128, bn = 128 iff the per-tap channel count (conv: C, dense: K) is a multiple of 128."""
    if e.b16:
        t = 256 if (e.N >= 256 and e.K >= 256 and e.N * e.K >= (1 << 19)) else 128
        return t, t
    cdiv = e.geom[3] if e.kind == 'conv' else e.K
    return (128 if e.N >= 128 else 64), (128 if cdiv % 128 == 0 else 64)


def tiles_nk(e):
    bm, bn = wgrad_tile(e)
    return (e.N + bm - 1) // bm, (e.K + bn - 1) // bn


def wgrad_splits(e):
    """wgrad_splits (train.hip:1917), without GRL_WGRAD_SPLITS: the slab count the workspace is sized for"""
    bm, bn = wgrad_tile(e)
    tn, tk = tiles_nk(e)
    tiles = tn * tk
    max_splits = max(1, (e.M + 255) // 256)
    slots = 1024.0 if (bm == 64 and bn == 64) else (256.0 if bm == 256 else 512.0)
    smax = min(int(3.0 * slots / float(tiles)) + 1, max_splits)
    best, best_cost = 1, 1e30
    for s in range(1, smax + 1):
        rounds = math.ceil(float(tiles) * float(s) / slots)
        stages = float(e.M) / (32.0 * float(s))
        cost = rounds * (stages + 8.0) + 0.012 * float(s) * float(tiles)
        if cost < best_cost * 0.999:
            best_cost, best = cost, s
    return best


def chunk(e):
    """pixels per split, a multiple of 32 (grl_conv_wgrad_f32, train.hip:1994: a.chunk)"""
    s = wgrad_splits(e)
    return ((e.M + s - 1) // s + 31) // 32 * 32


def real_splits(e):
    """gridDim.y and the slabs the reduce reads (train.hip:1997)"""
    return (e.M + chunk(e) - 1) // chunk(e)


def split_rows(e):
    c = chunk(e)
    return [(z * c, min(e.M, (z + 1) * c)) for z in range(real_splits(e))]


def wgrad_tile_mode(tn, tk):
    """wgrad_tile_mode (train.hip:893), GRL_WGRAD_XCD unset"""
    if tn * tk < 64:
        return 0
    m1, m2 = tn % 2 == 0 and tk % 4 == 0, tn % 4 == 0 and tk % 2 == 0
    if m1 and m2:
        return 1 if (tn // 2 + tk // 4) <= (tn // 4 + tk // 2) else 2
    return 1 if m1 else 2 if m2 else 0


def wgrad_tile_of(bid, tn, tk, mode):
    """wgrad_tile_of (train.hip:879): workgroup id -> (tile_n, tile_k)"""
    if mode == 0:
        return bid // tk, bid % tk
    gn = 2 if mode == 1 else 4
    gk = 8 // gn
    rn, rk = tn // gn, tk // gk
    xcd, slot = bid & 7, bid >> 3
    return (xcd // gk) * rn + slot // rk, (xcd % gk) * rk + slot % rk


def datapath(e):
    """the dispatch of grl_conv_wgrad_f32 (train.hip:2009-2031): 'b16in_256', 'b16in_128', 'bf16x3', 'bf16' or 'f32' -- a
    bf16 / bf16x3 request on anything but a 128 x 128 tile SILENTLY runs the exact-fp32 kernel"""
    if e.kind == 'stem':
        return 'stem'
    bm, bn = wgrad_tile(e)
    if e.b16:
        return 'b16in_256' if bm == 256 else 'b16in_128'
    if (bm, bn) == (128, 128) and e.math == MATH_BF16X3:
        return 'bf16x3'
    if (bm, bn) == (128, 128) and e.math == MATH_BF16:
        return 'bf16'
    return 'f32'


def kernel_body(e):
    p = datapath(e)
    cv = 'true' if e.kind == 'conv' else 'false'
    if p == 'stem':
        return 'stem_wgrad_kernel<%s>' % ('true' if e.b16 else 'false')
    if p == 'b16in_256':
        return 'wgrad_b16in_256_kernel<%s>' % cv
    if p == 'b16in_128':
        return 'wgrad_b16in_kernel<%s>' % cv
    return 'wgrad_kernel<%d, %d, %s, %d>' % (wgrad_tile(e) + (cv, {'f32': 0, 'bf16': 1, 'bf16x3': 3}[p]))


def conv_path(e):
    """the gather of wgrad_kernel<.., true, 0> (train.hip:926, 998): 'small_img' (fewer than 64 output pixels per image:
    32 rows can span several images), 'lin' (same-size stride-1 window whose Wo divides 32: the source is linear in the
    pixel index) or 'generic'.  None for everything else (the other kernels resolve every item's tap and pixel)."""
    if e.kind != 'conv' or datapath(e) != 'f32':
        return None
    n, H, W, C, k, stride, pad = e.geom
    Ho, Wo = out_hw(e)
    if Ho * Wo < 64:
        return 'small_img'
    return 'lin' if (stride == 1 and Ho == H and Wo == W and 32 % Wo == 0) else 'generic'


def stages_per_split(e):
    return [(m1 - m0 + 31) // 32 for m0, m1 in split_rows(e)]


def workspace_floats(e):
    """grl_wgrad_workspace_floats / grl_stem_wgrad_workspace_floats: sized for wgrad_splits slabs (the launch may use
    fewer: real_splits), or one [64][160] slab per stem workgroup"""
    return stem_wgs(e) * 64 * 160 if e.kind == 'stem' else wgrad_splits(e) * e.N * e.K


SW_TH, SW_TW, SW_WGS = 8, 16, 512       # train.hip:703, 706


def stem_tiles(e):
    """stem_wgrad_wgs (train.hip:1887): (tiles per image column, per image row, total) of 8 x 16 output pixels"""
    n, H, W = e.geom
    ty, tx = (H // 2 + SW_TH - 1) // SW_TH, (W // 2 + SW_TW - 1) // SW_TW
    return ty, tx, n * ty * tx


def stem_wgs(e):
    return min(stem_tiles(e)[2], SW_WGS)


def stem_trips(e, wg=0):
    """trips of `for (t = blockIdx.x; t < tiles; t += gridDim.x)` (train.hip:779) for workgroup wg"""
    return len(range(wg, stem_tiles(e)[2], stem_wgs(e)))


# ----------------------------------------------------------------------------------------------------------------------
# inputs
def classes(e):
    """'a' N(0, 1); 'b' cancelling; 't' tagged; 'u' a second tagged pixel where the pixel range is split"""
    return ('a', 'b', 't', 'u') if (e.kind != 'stem' and real_splits(e) > 1) else ('a', 'b', 't')


def tag_row(e, cls, index):
    """The one row of dz (output pixel) class (t) / (u) lights, and what it is.  Split pixel ranges: the last pixel of split 0
    (t) and the first of split 1 (u).  A stem whose workgroups take several tiles: an interior pixel of a second-trip
    tile.  Otherwise, in turn over the sweep: a corner, the last row, the last column, an interior pixel (of the last
    image; dense: rows 0, M - 1, the last row of the first stage, M / 2)."""
    if e.kind != 'stem' and real_splits(e) > 1:
        return (chunk(e) - 1, 'last pixel of split 0') if cls == 't' else (chunk(e), 'first pixel of split 1')
    which = TAG_PIXELS[index % 4]
    if e.kind == 'dense':
        return {'corner': 0, 'last row': e.M - 1, 'last column': min(e.M, 32) - 1, 'interior': e.M // 2}[which], which
    Ho, Wo = (e.geom[1] // 2, e.geom[2] // 2) if e.kind == 'stem' else out_hw(e)
    oy, ox = {'corner': (0, 0), 'last row': (Ho - 1, Wo // 2), 'last column': (Ho // 2, Wo - 1),
              'interior': (Ho // 2, Wo // 2)}[which]
    img = e.geom[0] - 1
    if e.kind == 'stem' and stem_trips(e) > 1:
        ty, tx, _ = stem_tiles(e)
        t = stem_wgs(e) + 2                                  # workgroup 2's second tile
        img, tr = t // (ty * tx), t % (ty * tx)
        oy, ox = (tr // tx) * SW_TH + min(Ho, SW_TH) // 2, (tr % tx) * SW_TW + min(Wo, SW_TW) // 2
        which = 'second-trip tile'
    return (img * Ho + oy) * Wo + ox, which


def to_bf16(a):
    return f32(bf16_round(a))


def make_inputs(e, cls):
    """fp32 dz[M][ldz], x (dense [M][ldx]; conv [n H W][C]; stem [n][3][H][W]) and g0, the preload of the accumulate form,
    in the result's shape.  (a) N(0, 1); (b) cancelling: x equal over the pixels up to 1e-3 and every column of dz sums to
    ~0 over the pixels, |dW| << abs_terms; (t, u) tagged: dz of (a), zero except one row (tag_row).  bf16-operand entries:
    rounded to bf16 (the stem: dz only)."""
    index = SWEEP.index(e)
    r = rng_for('wgrad', index, e.M, e.N, e.K, cls)
    dz = r.standard_normal((e.M, e.ldz))
    if e.kind == 'dense':
        xshape, out = (e.M, e.ldx), (e.N, e.k_out or e.K)
    elif e.kind == 'conv':
        n, H, W, C, k, stride, pad = e.geom
        xshape, out = (n * H * W, C), (e.N, C, k, k)
    else:
        n, H, W = e.geom
        xshape, out = (n, 3, H, W), (64, 3, 7, 7)
    x = r.standard_normal(xshape)
    if cls == 'b':
        first = x[:1] if e.kind != 'stem' else x[:, :, :1, :1]
        x = near(r, np.broadcast_to(first, x.shape))
        dz = dz - dz.mean(0, keepdims=True)
    if cls in 'tu':
        keep = np.zeros((e.M, 1))
        keep[tag_row(e, cls, index)[0]] = 1.0
        dz = dz * keep
    g0 = f32(r.standard_normal(out))
    dz, x = f32(dz), f32(x)
    if e.b16:
        dz = to_bf16(dz)
        if e.kind != 'stem':
            x = to_bf16(x)
    return dict(dz=dz, x=x, g0=g0)


def reference(e, d):
    """(result, abs_terms, terms) of wgrad_ref for the entry, in the library's output layout"""
    if e.kind == 'dense':
        return R.dense(d['dz'], d['x'], e.N, e.K, e.k_out)
    if e.kind == 'conv':
        n, H, W, C, k, stride, pad = e.geom
        Ho, Wo = out_hw(e)
        return R.conv(d['dz'][:, :e.N], d['x'], n, H, W, Ho, Wo, k, stride, pad)
    return R.stem(d['dz'], d['x'], *e.geom)


# ----------------------------------------------------------------------------------------------------------------------
# bounds
def depth(e, terms):
    """roundings a term passes through at the most (see the module docstring)"""
    if e.kind == 'stem':
        return np.minimum(terms, 32.0 * stem_trips(e) + 3 + stem_wgs(e))
    per = 3.0 if datapath(e) == 'bf16x3' else 1.0
    return per * np.minimum(terms, float(chunk(e))) + real_splits(e)


def representation(e):
    """relative error of a term before any accumulation: the operands' rounding to bf16 (math = bf16), the dropped lo x lo
    product and the two lo roundings (bf16x3); 0 for fp32 products and for operands that are bf16 already"""
    return {'bf16': 2 * UB + UB * UB, 'bf16x3': 3 * UB8 * UB8 * (1 + 2 * UB8)}.get(datapath(e), 0.0)


def bound(e, abs_terms, terms, result, accumulate, as_fp32=False):
    """per element; `result` includes the preload in the accumulate form.  as_fp32: the exact-fp32 rule whatever the
    entry's math mode asks for (which datapath really ran)"""
    if as_fp32:
        err = (np.minimum(terms, float(chunk(e))) + real_splits(e)) * U * abs_terms
    else:
        grow = 1 + 5 * UB8 if datapath(e) == 'bf16x3' else 1.0
        err = (depth(e, terms) * U * grow + representation(e)) * abs_terms
    if accumulate:
        err = err + np.where(abs_terms > 0, U * np.abs(result), 0.0)
    return SAFETY * err


# ----------------------------------------------------------------------------------------------------------------------
# fp32 restatements in the kernels' orders (numpy, CPU): the bounds are satisfiable -- and, with a mutation, sharp
def gather(e, x, mutate=None):
    """the implicit-GEMM operand Xg[m][t C + c] of a conv entry (fp32).  Mutations: 'shift_tap' reads tap kx = 0 one column
    further left for the pixels of the last output column; 'wrap_tap' reads a tap whose column falls outside the image from
    the linear pixel index -- the neighbouring row -- instead of zero."""
    n, H, W, C, k, stride, pad = e.geom
    Ho, Wo = out_hw(e)
    m = np.arange(e.M)
    img, oy, ox = m // (Ho * Wo), (m // Wo) % Ho, m % Wo
    xs = np.asarray(x, F).reshape(n * H * W, C)
    out = np.zeros((e.M, k * k, C), F)
    for ky in range(k):
        for kx in range(k):
            iy, ix = stride * oy - pad + ky, stride * ox - pad + kx
            if mutate == 'shift_tap' and kx == 0:
                ix = np.where(ox == Wo - 1, ix - 1, ix)
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            lin = (img * H + iy) * W + ix
            if mutate == 'wrap_tap':
                ok = (iy >= 0) & (iy < H) & (lin >= 0) & (lin < n * H * W)
            out[ok, ky * k + kx] = xs[lin[ok]]
    return out.reshape(e.M, k * k * C)


def _chain(acc, a, b):
    """acc[n][k] += a[m][n] * b[m][k], m ascending, one fp32 chain per element (rows of zeros skipped: they add exactly)"""
    for m in np.flatnonzero((a != 0).any(1)):
        acc += a[m][:, None] * b[m][None, :]
    return acc


def _split(v):
    hi = to_bf16(v)
    return hi, to_bf16(v - hi)


def restate(e, d, accumulate, mutate=None):
    """grl_conv_wgrad_f32 for a dense / conv entry in fp32 numpy: per split one chain per element over its pixel range
    (math = bf16: on operands rounded to bf16; bf16x3: per 16-row MFMA step hi hi, then lo hi, then hi lo), the tiles
    stored into NaN-filled slabs through the tile map, the slabs added in order, the result scattered to torch's layout.
    Mutations (see MUTATIONS): 'drop_last_row' leaves out the last row of split 0; 'late_stage' starts split 1 one 32-row
    stage late; 'no_lo_hi' omits bf16x3's lo x hi product; 'xcd_swap' exchanges the tile rows of two workgroups of the XCD
    map (one tile computed twice, one never); 'shift_tap' / 'wrap_tap': gather()."""
    a = np.asarray(d['dz'], F)[:, :e.N]
    b = gather(e, d['x'], mutate) if e.kind == 'conv' else np.asarray(d['x'], F)[:, :e.K]
    path = datapath(e)
    if path == 'bf16':
        a, b = to_bf16(a), to_bf16(b)
    if path == 'bf16x3':
        (ah, al), (bh, bl) = _split(a), _split(b)
    bm, bn = wgrad_tile(e)
    tn, tk = tiles_nk(e)
    mode = wgrad_tile_mode(tn, tk)
    total = np.zeros((e.N, e.K), F)
    for z, (m0, m1) in enumerate(split_rows(e)):
        if mutate == 'drop_last_row' and z == 0:
            m1 -= 1
        if mutate == 'late_stage' and z == 1:
            m0 += 32
        acc = np.zeros((e.N, e.K), F)
        if path == 'bf16x3':
            for s0 in range(m0, m1, 16):
                s1 = min(m1, s0 + 16)
                _chain(acc, ah[s0:s1], bh[s0:s1])
                if mutate != 'no_lo_hi':
                    _chain(acc, al[s0:s1], bh[s0:s1])
                _chain(acc, ah[s0:s1], bl[s0:s1])
        else:
            _chain(acc, a[m0:m1], b[m0:m1])
        slab = np.full((e.N, e.K), np.nan, F)
        for bid in range(tn * tk):
            i, j = wgrad_tile_of(bid, tn, tk, mode)
            if mutate == 'xcd_swap' and mode != 0 and bid in (0, tn * tk - 1):
                i = wgrad_tile_of(tn * tk - 1 - bid, tn, tk, mode)[0]
            slab[i * bm:(i + 1) * bm, j * bn:(j + 1) * bn] = acc[i * bm:(i + 1) * bm, j * bn:(j + 1) * bn]
        total = total + slab
    if e.kind == 'conv':
        k = e.geom[4]
        total = R.to_torch_layout(total, e.N, e.geom[3], k * k).reshape(e.N, e.geom[3], k, k)
    elif e.k_out:
        total = total[:, :e.k_out]
    return accumulated(d['g0'], total) if accumulate else total


def accumulated(g0, total):
    """wgrad_reduce_kernel's accumulate form: dw = dw + s, one fp32 addition"""
    return np.asarray(g0, F) + np.asarray(total, F)


def restate_stem(e, d, accumulate, mutate=None, channels=None):
    """stem_wgrad_kernel + wgrad_reduce_kernel in fp32 numpy, for the output channels `channels` (all when None): every
    workgroup walks its tiles; per tile the four pixel quarters (tile rows 2 q, 2 q + 1) each add their 32 pixels in order
    into their own chain, which runs on over the workgroup's trips; the quarters are added in order, then the workgroups'
    slabs in order.  Mutation 'stale_patch': from the second trip on the gathered operand is the PREVIOUS tile's."""
    n, H, W = e.geom
    Ho, Wo = H // 2, W // 2
    ty, tx, tiles = stem_tiles(e)
    G = stem_wgs(e)
    ch = np.arange(64) if channels is None else np.asarray(channels)
    dz = np.asarray(d['dz'], F)[:, ch]
    x = np.asarray(d['x'], F)
    acc = np.zeros((G, 4, len(ch), 147), F)
    q = np.arange(4)[None, :]
    for r in range(stem_trips(e)):
        t = np.arange(G) + r * G
        live = (t < tiles)[:, None]
        tt = np.minimum(t, tiles - 1)
        ts = tt - G if (mutate == 'stale_patch' and r >= 1) else tt

        def origin(tl):
            img, tr = tl // (ty * tx), tl % (ty * tx)
            return img[:, None], ((tr // tx) * SW_TH)[:, None], ((tr % tx) * SW_TW)[:, None]
        (img, oy0, ox0), (simg, soy0, sox0) = origin(tt), origin(ts)
        for step in range(32):
            dy, dx = 2 * q + step // 16, step % 16
            oy, ox = oy0 + dy, ox0 + dx
            ok = live & (oy < Ho) & (ox < Wo)
            if not ok.any():
                continue
            pix = np.where(ok, (img * Ho + oy) * Wo + ox, 0)
            a = np.where(ok[..., None], dz[pix], F(0))                                  # [G][4][ch]
            spix = (simg * Ho + np.minimum(soy0 + dy, Ho - 1)) * Wo + np.minimum(sox0 + dx, Wo - 1)
            b = R.stem_columns(x, n, H, W, np.where(ok, spix, 0).reshape(-1)).reshape(G, 4, 147)
            acc += a[..., None] * b[:, :, None, :]
    slabs = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    total = np.zeros((len(ch), 147), F)
    for g in range(G):
        total = total + slabs[g]
    total = total.reshape(len(ch), 3, 7, 7)
    return accumulated(np.asarray(d['g0'])[ch], total) if accumulate else total
