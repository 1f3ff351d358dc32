"""Launch rules, sweep, inputs, first-order rounding-error bounds and fp32 restatements for the stem and max-pool kernels
(pointwise.hip, pointwise_bf16.hip, train.hip, train_bf16.hip) -- shared by test_stem_ref_cpu.py (no GPU) and
test_gpu_stem_float64.py.  U, SAFETY, check, RATIOS, dump_ratios, bf16_round, bf16_ulp, apply_f32 and b_apply are bn_bounds'
own, DIV_ULP, ULP, rng_for and f32 are head_bounds'.

Bounds are derived per element, none is fitted (u = 2^-24; the build uses -ffp-contract=off, every * and + rounds once).
A sum whose every term passes through at most k roundings is off by at most k u sum|terms|; k is read from the kernel:
  stem_mfma_kernel      `for (q = 0; q < SM_K / 8; ++q)` x `for (s = 0; s < 4; ++s)`, two k per MFMA: SM_K = 160 k-steps,
                        one accumulator rounding each (the 13 padded steps add exact zeros; counted all the same), and
                        every product rounds once:                                              K_MFMA = 160, + 1
  stem_pool_f32_kernel  `for (chunk = 0; chunk < 21; ++chunk)` x `for (u = 0; u < 4; ++u)`, two k per MFMA:
                        21 x 8 k-steps:                                                         K_POOL_F32 = 168, + 1
  stem_conv7x7_kernel   `acc[o] = fmaf(v, wk[o * 147], acc[o])` over 3 x 7 x 7 taps: one rounding per term, the
                        product is not rounded:                                                 K_VALU = 147, + 0
  stem_b16_kernel, stem_pool_b16_kernel, stem_pool2_b16_kernel
                        `for (s = 0; s < SB_K / 16; ++s)`, SB_K = 176: the products of two bf16 are exact in fp32, the
                        fp32 accumulation passes through at most 176 roundings:                 K_BF16 = 176, + 0
The affine epilogue `acc * scale + shift` adds two roundings, relative to |acc scale| + |shift|; the ReLU is 1-Lipschitz.
A bf16 store rounds once: half of bf16_ulp(reference), on top of the fp32 bound carried through it.
Raw-u8 input: `((float)u / 255.f - mean) / std` -- two divisions (DIV_ULP ulp each: ASSUMED, as in head_bounds, not derived)
and a subtraction; the bf16 kernels round the normalised pixel to bf16 once more (2^-9 relative).  These input errors
reach the output through sum e_x |w| (stem_ref.stem's E).
max is 1-Lipschitz in the sup norm, |max_i a_i - max_i b_i| <= max_i |a_i - b_i|: the bound of a pooled element of the fused
stem + pool kernels is the largest stem bound in its window, nothing looser.
Max-pool forward and im2col copy: bit for bit.  A max-pool backward element is a sum of at most four dy, added to 0.f in
sequence (`g[u][v][e] += d[e]`): the first addition is exact, three more round: 3 u sum|dy|."""
import functools

import numpy as np

import stem_ref as R
from bn_bounds import U, SAFETY, check, RATIOS, dump_ratios, bf16_round, bf16_ulp, apply_f32, b_apply      # noqa: F401
from head_bounds import DIV_ULP, ULP, rng_for, f32                                                             # noqa: F401

U16 = 2.0 ** -9                 # unit roundoff of bf16
K_MFMA, K_POOL_F32, K_VALU, K_BF16 = 160, 168, 147, 176
MEAN_STD = np.array([0.485, 0.456, 0.406, 0.229, 0.224, 0.225], np.float32)

# ----------------------------------------------------------------------------------------------------------------------
# the launch rules, restated from the launchers
GRID_CAP = 8192                 # common.h grid_for


def grid_for(items):
    g = (items + 255) // 256
    return 1 if g < 1 else min(g, GRID_CAP)


def grid_even(items):
    g = grid_for(items)
    return (g + 1) & ~1 if g > 1 else g


def past_one_pass(items, grid):
    """does the `i += gridDim.x * blockDim.x` tail of a grid-stride kernel run?"""
    return items > grid * 256


def stem_tiles(H, W, th, tw):
    """tiles (x, y) of a two-launch stem: th x tw output pixels each (8 x 16: stem_mfma_kernel and, per step of its 32-row
    walk, stem_b16_kernel; 16 x 16: stem_conv7x7_kernel)"""
    return -(-(W // 2) // tw), -(-(H // 2) // th)


def tile_kinds(H, W, th, tw):
    """which of {'full', 'x', 'y', 'xy'} occur: tiles whose `ox < Wo` guard cuts only, whose `oy < Ho` guard cuts only, both"""
    Ho, Wo = H // 2, W // 2
    tx, ty = stem_tiles(H, W, th, tw)
    kinds = set()
    for j in range(ty):
        for i in range(tx):
            sx, sy = (i + 1) * tw > Wo, (j + 1) * th > Ho
            kinds.add('xy' if sx and sy else 'x' if sx else 'y' if sy else 'full')
    return kinds


def b16_walk(H):
    """stem_b16_kernel: workgroups in y (SB_TPW = 4 tiles of 8 rows each) and the tiles the last one walks"""
    Ho = H // 2
    wgs = -(-Ho // 32)
    return wgs, -(-(Ho - 32 * (wgs - 1)) // 8)


def pool_f32_rule(n, H):
    """grl_stem_pool_f32: (strips asked for, pooled rows per strip, workgroups per frame)"""
    Hp = H // 4
    strips = 1
    while strips * 2 <= Hp // 4 and n * strips < 512:
        strips *= 2
    strip_prows = (Hp + strips - 1) // strips
    return strips, strip_prows, -(-Hp // strip_prows)


def pool_b16_form(H):
    """grl_stem_pool_bf16: 2 = stem_pool2_b16_kernel (Ho % 4 == 0, i.e. H % 8 == 0), 1 = stem_pool_b16_kernel (H % 8 == 4)"""
    return 2 if (H // 2) % 4 == 0 else 1


def pool_b16_rule(n, H):
    """grl_stem_pool_bf16: (strips asked for, stem rows per strip, workgroups per frame); the first form has fixed strips of
    SP_TPW * SP_TH = 32 stem rows"""
    Ho = H // 2
    if pool_b16_form(H) == 1:
        return -(-Ho // 32), 32, -(-Ho // 32)
    strips = 1
    while strips * 2 <= Ho // 8 and n * strips < 512:
        strips *= 2
    strip_rows = (Ho // 4 + strips - 1) // strips * 4
    return strips, strip_rows, -(-Ho // strip_rows)


def last_strip_rows(total, per_strip, grid):
    return total - per_strip * (grid - 1)


# ----------------------------------------------------------------------------------------------------------------------
# the sweep
STEM_SHAPES = ((1, 2, 2), (2, 6, 4), (1, 14, 30), (1, 16, 32), (2, 18, 34), (1, 66, 36), (3, 130, 2))
POOL_H = (4, 8, 12, 20, 36, 40, 68, 72, 132, 136)
POOL_W = 128


def _cap_n(H):
    """the smallest n at which `n * strips < 512` caps the strip count of both fused launchers at this H"""
    n = 1
    while pool_f32_rule(n, H)[0] == pool_f32_rule(1, H)[0] or pool_b16_rule(n, H)[0] == pool_b16_rule(1, H)[0]:
        n *= 2
    return n


POOL_N_CAP = _cap_n(POOL_H[-1])
POOL_CASES = tuple((n, H) for H in POOL_H for n in (1, 3)) + ((POOL_N_CAP, POOL_H[-1]),)
POOL_DISTINCT = 4               # the capped case repeats this many different frames (the reference is built once per frame)

MP_SIZES = (1, 2, 3, 4, 5, 8, 9)
MP_C32, MP_C16 = (4, 36, 64, 68), (8, 40, 64, 72)


def _mp_pairs():
    odd, even = (1, 3, 5, 9), (2, 4, 8)
    out = []
    for i, v in enumerate(MP_SIZES):
        for p in (odd[i % 4], even[i % 3]):
            for hw in ((v, p), (p, v)):
                if hw not in out:
                    out.append(hw)
    return tuple(out)


MP_PAIRS = _mp_pairs()
# (n, H, W, index into MP_C32 / MP_C16)
MP_CASES = tuple((1 + i % 3, H, W, (i + i // 4) % 4) for i, (H, W) in enumerate(MP_PAIRS))
MP_CLASSES = ('a', 'b', 'c')
IM2COL_KP = (160, 192)

# one case per grid-stride kernel just past one pass of the capped grid (8192 x 256 items: the `i += gridDim.x * blockDim.x`
# tail runs), and the same layout at a few items as its stand-in for the CPU file
BIG = dict(mp32=(32769, 3, 3, 64), mp16=(65537, 3, 3, 64), im2col32=(1, 232, 228, 160), im2col16=(8, 232, 228, 160))
BIG_CPU = dict(mp32=(3, 3, 3, 4), mp16=(3, 3, 3, 8), im2col32=(1, 6, 4, 160), im2col16=(1, 6, 4, 160))


def big_items(name, case):
    """items (lanes' worth of work) of the launch: float4 / 8 x bf16 vectors of the pooled map or of the 2 x 2 input blocks
    (the same count); elements (fp32) or 8-element chunks (bf16) of the im2col matrix"""
    if name.startswith('mp'):
        n, H, W, C = case
        Ho, Wo = R.pooled_size(H, W)
        return n * Ho * Wo * (C // (4 if name == 'mp32' else 8))
    n, H, W, Kp = case
    return n * (H // 2) * (W // 2) * (Kp if name == 'im2col32' else Kp // 8)


# ----------------------------------------------------------------------------------------------------------------------
# inputs
def to_bf16(a):
    return f32(bf16_round(a))


def stem_params(key, b16):
    """w [64][147], scale (both signs), shift"""
    r = rng_for('stemw', *key)
    w = f32(r.standard_normal((64, 147)) / np.sqrt(147.0))
    scale = f32(r.uniform(0.5, 1.5, 64) * r.choice([-1.0, 1.0], 64))
    scale[:2] = (0.75, -0.75)
    return dict(w=to_bf16(w) if b16 else w, scale=scale, shift=f32(r.uniform(-0.7, 0.7, 64)))


def stem_image(n, H, W, cls, u8, b16):
    """float: (a) Gaussian, (m) a per-channel mean much larger than the spread of the pixels (bf16-representable for the bf16
    kernels: their operand rounding then is exact).  u8: (a) uniform bytes with runs of 0 and of 255, (m) a narrow band of
    bytes around a per-channel level."""
    r = rng_for('stemx', n, H, W, cls, int(u8), int(b16))
    if u8:
        if cls == 'a':
            x = r.randint(0, 256, (n, 3, H, W))
            x[r.random_sample(x.shape) < 0.15] = 0
            x[r.random_sample(x.shape) < 0.15] = 255
            x[:, :, 0, 0], x[:, :, H - 1, W - 1] = 0, 255
        else:
            x = r.randint(200, 206, (n, 3, 1, 1)) + r.randint(-2, 3, (n, 3, H, W))
        return np.ascontiguousarray(x, dtype=np.uint8)
    if cls == 'a':
        x = r.standard_normal((n, 3, H, W))
    else:
        x = (r.choice([-1.0, 1.0], (1, 3, 1, 1)) * r.uniform(50.0, 100.0, (1, 3, 1, 1))) + 1e-2 * r.standard_normal((n, 3, H, W))
    return to_bf16(x) if b16 else f32(x)


def e_normalize(u8, mean_std=MEAN_STD):
    """first-order absolute error of a normalised pixel, `((float)u / 255.f - mean) / std` (pointwise.hip load_patch /
    store_row): q = fl(u / 255): DIV_ULP ulp of |q|; t = fl(q - mean): u |t|; v = fl(t / std): DIV_ULP ulp of |v|"""
    ms = R.f64(mean_std)
    m, s = ms[:3][None, :, None, None], ms[3:6][None, :, None, None]
    q = R.f64(u8) / 255.0
    t = q - m
    return (DIV_ULP * ULP * np.abs(q) + U * np.abs(t)) / np.abs(s) + DIV_ULP * ULP * np.abs(t / s)


@functools.lru_cache(maxsize=2)
def stem_case(n, H, W, cls, u8, b16, distinct=0):
    """inputs, the float64 reference (pre-ReLU, ReLU applied by the caller) and the input-error map of one stem case.
    distinct > 0: only `distinct` different frames, repeated in turn: x holds all n, the reference the first `distinct`, and
    `reps` = n / distinct says how often it repeats (tile() lays a view of it over the n frames)."""
    m = distinct if distinct else n
    p = stem_params((H, W, cls, int(u8), int(b16)), b16)
    x = stem_image(m, H, W, cls, u8, b16)
    if u8:
        xr = R.normalize(x, MEAN_STD)
        ex = e_normalize(x)
        if b16:                                    # `patch[i] = (__bf16)pv[it]` / store_row's `(__bf16)`
            ex = ex + U16 * (np.abs(xr) + ex)
    else:
        xr, ex = R.f64(x), None
    ref = R.stem(xr, p['w'], p['scale'], p['shift'], 0, ex)
    if distinct:
        rep = np.arange(n) % m
        assert n % m == 0
        x = np.ascontiguousarray(x[rep])
    return dict(x=x, ref=ref, reps=n // m, **p)


def tile(a, reps):
    """a [rows][C] of `distinct` frames as a read-only view [reps][rows][C]: frame i of the launch is frame i % distinct"""
    a = np.asarray(a)
    return np.broadcast_to(a[None], (reps,) + a.shape)


def mp_map(n, H, W, C, cls, b16, seed=0):
    """[n][H][W][C] maps: (a) Gaussian; (b) post-ReLU with about half zeros, a whole 3 x 3 window of one constant, channel 1
    all-equal in every image and the last image all-equal in every channel: ties, the first-maximum rule; (c) all negative:
    a pad value that is not -inf shows."""
    r = rng_for('mp', n, H, W, C, cls, seed)
    a = r.standard_normal((n, H, W, C))
    if cls == 'b':
        a = np.maximum(a, 0.0)
        a[:, :3, :3, :] = 1.5
        a[..., 1] = 0.75
        if n > 1:
            a[n - 1] = 0.25
    elif cls == 'c':
        a = -np.abs(a) - 0.125
    return to_bf16(a) if b16 else f32(a)


def mp_vectors(C, seed=0):
    """mean, scale (both signs), beta of grl_bn_relu_maxpool3x3s2"""
    r = rng_for('mpv', C, seed)
    return dict(mean=f32(0.3 * r.standard_normal(C)), scale=f32(r.uniform(0.5, 1.5, C) * r.choice([-1.0, 1.0], C)),
                beta=f32(r.uniform(-0.5, 0.5, C)))


def mp_dy(n, H, W, C, b16, seed=0):
    Ho, Wo = R.pooled_size(H, W)
    d = rng_for('mpdy', n, H, W, C, seed).standard_normal((n, Ho, Wo, C))
    return to_bf16(d) if b16 else f32(d)


def big_map(n, H, W, C):
    """small integers (exact in bf16, cheap to draw, ties in most windows)"""
    return f32(rng_for('bigmp', n, H, W, C).randint(-8, 9, (n, H, W, C)))


# ----------------------------------------------------------------------------------------------------------------------
# bounds (every b_* carries SAFETY)
def b_stem_f32(ref, scale, shift, k, prod):
    """fp32 stems: SAFETY ((k + prod) u A |scale| + E |scale| + 2 u (|acc scale| + |shift|))"""
    sc, sh = np.abs(R.f64(scale)), np.abs(R.f64(shift))
    e_acc = (k + prod) * U * ref['A'] + (ref['E'] if ref['E'] is not None else 0.0)
    return SAFETY * (sc * e_acc + 2 * U * (np.abs(ref['acc']) * sc + sh))


def b_stem_bf16(ref, scale, shift, y):
    """bf16 stems: the fp32 bound at K_BF16 with exact products, and half a bf16 spacing of the reference y for the store"""
    return 0.5 * bf16_ulp(y) + b_stem_f32(ref, scale, shift, K_BF16, 0)


def pool_bound(b, n, Ho, Wo):
    """the largest stem bound in every 3 x 3 / stride 2 / pad 1 window"""
    return R.maxpool(np.asarray(b, np.float64).reshape(n, Ho, Wo, -1))[0]


def b_pool_bwd(S, ref=None):
    """3 u sum|dy| (+ half a bf16 spacing of the reference for the bf16 store)"""
    return SAFETY * 3 * U * S + (0.0 if ref is None else 0.5 * bf16_ulp(ref) * (S > 0))


def b_bn_relu(z, mean, scale, beta):
    """the fused kernel's three fp32 operations per element: bn_bounds.b_apply on |z - mean| |scale| + |beta|"""
    return b_apply(np.abs(R.f64(z) - R.f64(mean)) * np.abs(R.f64(scale)) + (0.0 if beta is None else np.abs(R.f64(beta))))


# ----------------------------------------------------------------------------------------------------------------------
# fp32 restatements (numpy float32, CPU): the bounds are satisfiable
F = np.float32


def _steps(order):
    """the taps (c, ky, kx) of every accumulator update, in one plausible order of each kernel"""
    if order == 'valu':             # (c, ky, kx), one fmaf each
        return [[(c, ky, kx)] for c in range(3) for ky in range(7) for kx in range(7)]
    if order == 'mfma':             # k = (c, ky, kx) flat, padded to 160: an MFMA takes k = 8 q + s and 8 q + 4 + s
        flat = [(c, ky, kx) for c in range(3) for ky in range(7) for kx in range(7)] + [None] * 13
        return [[flat[8 * q + s], flat[8 * q + 4 + s]] for q in range(20) for s in range(4)]
    # 'pool': chunks (c, ky) with kx padded to 8: an MFMA takes kx = u and 4 + u
    return [[(c, ky, u), (c, ky, 4 + u) if u < 3 else None] for c in range(3) for ky in range(7) for u in range(4)]


def stem_f32(x, w, scale, shift, relu, order):
    """the fp32 stem with every product and every accumulator update rounded to fp32 ('valu': the product of an fmaf is
    exact, the sum rounds once), the affine epilogue and the ReLU as the kernels state them"""
    x, w = F(x), F(w).reshape(64, 3, 7, 7)
    n, _, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    xp = np.zeros((n, 3, H + 6, W + 6), F)
    xp[:, :, 3:H + 3, 3:W + 3] = x
    acc = np.zeros((n, Ho, Wo, 64), F)
    for step in _steps(order):
        for tap in step:
            if tap is None:
                continue
            c, ky, kx = tap
            p = xp[:, c, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2][..., None]
            if order == 'valu':
                acc = (acc.astype(np.float64) + p.astype(np.float64) * w[:, c, ky, kx].astype(np.float64)).astype(F)
            else:
                acc = acc + p * w[:, c, ky, kx]
    y = acc * F(scale) + F(shift)
    return (np.maximum(y, F(0)) if relu else y).reshape(n * Ho * Wo, 64)


def normalize_f32(u8, mean_std=MEAN_STD):
    ms = F(mean_std)
    return (F(u8) / F(255) - ms[:3][None, :, None, None]) / ms[3:6][None, :, None, None]


def bn_relu_maxpool_f32(z, mean, scale, beta, b16):
    """grl_bn_relu_maxpool3x3s2(_bf16): a = relu(fl(fl(fl(z - mean) * scale) + beta)) (bn_bounds.apply_f32), rounded to bf16
    in the bf16 twin (`(float)(__bf16)(...)`), then the window's maximum and the position of its first occurrence
    (`if (a > m[e])`, m = -inf at the start).  Returns (a, pooled, positions)."""
    a = apply_f32(z, mean, scale, beta, None, True)
    if b16:
        a = to_bf16(a)
    y, pos = R.maxpool(a)
    return a, y.astype(F), pos
