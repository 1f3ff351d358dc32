"""Shapes, inputs, first-order rounding-error bounds and fp32 restatements of the summation order for the gate, TRL and
Siamese head kernels (train_head.hip, pointwise.hip) -- shared by test_head_ref_cpu.py (no GPU) and
test_gpu_head_float64.py.  U, SAFETY, check, RATIOS and dump_ratios are bn_bounds' own.

Bounds are derived per element, none is fitted.  The build uses -ffp-contract=off: every * and + rounds once (u = 2^-24).
A sum whose every term passes through at most k roundings is off by at most k u sum|terms|; k is read from the kernel:
  one wave per row, lane stride 256 floats:  product (1) + the four-element dot (3) + lane trips + six wave_sum levels;
  one workgroup per row, stride 1024:        the same with trips of 1024, + the four sequential adds of block_sum;
  16 waves over the rows of a slab (red16):  ceil(rows / 16) sequential rows per wave + the (a+b)+(c+d) tree (2) + 4 adds.
An elementwise expression adds (its roundings) u (its largest term).  Errors of one stage that feed the next are carried
through the derivative.  Everything is multiplied by SAFETY (2: the dropped u^2 terms) once, at the end.

expf, sqrtf and the division are the one thing that cannot be read from the kernel text: EXPF_ULP, SQRT_ULP, DIV_ULP below
are ASSUMED (no copy of the ROCm math-function accuracy tables was at hand), not measured and not tuned against the kernels:
2 ulp for expf, 1 ulp for sqrtf and for the division; an ulp is at most 2 u relative."""
import numpy as np

import head_ref as H
from bn_bounds import U, SAFETY, check, RATIOS, dump_ratios          # noqa: F401  (re-exported to the two test files)

EXPF_ULP = 2.0      # assumed
SQRT_ULP = 1.0      # assumed
DIV_ULP = 1.0       # assumed
ULP = 2.0 * U       # one unit in the last place, relative, at most
GRID_CAP = 8192 * 256           # float4 items one pass of a capped grid-stride launch covers (common.h grid_for)

# ----------------------------------------------------------------------------------------------------------------------
# the sweep
WAVE_ROWS = (1, 3, 4, 5, 37)                    # one wave per row, four rows per workgroup
WAVE_WIDTH = (4, 252, 256, 260, 516)            # lane stride 256
PAIR_COUNTS = ((1, 1), (2, 3), (5, 1), (4, 2))  # pair_verify: np x ng  (4 x 2: the only one whose last workgroup is full)
BLOCK_ROWS = (1, 3)                             # one workgroup per row
BLOCK_WIDTH = (4, 1020, 1024, 1028, 2052)       # stride 1024
RED_ROWS = (1, 15, 16, 17, 33)                  # 16 waves share the rows
RED_WIDTH = (4, 252, 256, 260)
RED_GROUPS = (1, 3)
EW_B, EW_ROWS, EW_C, EW_T, EW_RPG = (1, 3), (1, 5), (4, 260), (1, 2, 5), (1, 5)
PAIR_BWD_COUNTS = ((1, 1), (1, 3), (3, 1), (2, 5))
PAIR_BWD_K = (4, 128, 1028)
CATTE_B, CATTE_HD, CATTE_C, CATTE_T = (1, 3), (1, 3, 4, 5, 128), (4, 1020, 1024, 1028, 2048), 3
ATT_B, ATT_T, ATT_D, ATT_C = (1, 3), (1, 2, 3, 4, 5, 16), (4, 128, 252, 260), (4, 1020, 1028, 2048)


def gate_ldys(C):
    return (1, 3, C + 4)


# (M, C, ldy): every M with every C, the three ldy in turn
GATE_CASES = tuple((M, C, gate_ldys(C)[(i + j) % 3]) for i, M in enumerate(WAVE_ROWS) for j, C in enumerate(WAVE_WIDTH))
# (M, Ch, C): every M with every reduced width Ch; the streamed width C runs through the same list
GCE_CASES = tuple((M, Ch, WAVE_WIDTH[(i + 2 * j + 1) % 5]) for i, M in enumerate(WAVE_ROWS) for j, Ch in enumerate(WAVE_WIDTH))
PAIR_VERIFY_CASES = tuple((n, g, K) for n, g in PAIR_COUNTS for K in WAVE_WIDTH)
# (rows, C, ld): ld = C or C + 8
BLOCK_CASES = tuple((r, C, C + 8 * ((i + j) % 2)) for i, r in enumerate(BLOCK_ROWS) for j, C in enumerate(BLOCK_WIDTH)) + \
    tuple((r, C, C + 8 * ((i + j + 1) % 2)) for i, r in enumerate(BLOCK_ROWS) for j, C in enumerate(BLOCK_WIDTH))
# (groups, rows, C, ldy_extra, f2 stride multiple)
RED_CASES = tuple((RED_GROUPS[(i + j) % 2], rows, C, 8 * ((i + j // 2) % 2), 1 + (i + j) % 2)
                  for i, rows in enumerate(RED_ROWS) for j, C in enumerate(RED_WIDTH)) + \
    ((3, 33, 260, 8, 1), (1, 33, 260, 0, 2), (3, 1, 4, 0, 2), (1, 17, 252, 8, 1), (3, 15, 256, 0, 1), (1, 16, 256, 8, 2))
EW_CASES = tuple((b, rows, C) for b in EW_B for rows in EW_ROWS for C in EW_C)          # x T or rows_per_group in the tests
# the one case per grid-stride kernel whose float4 count is just above 8192 * 256 (the `i += gridDim.x * blockDim.x` tail runs),
# and its stand-in for the CPU file (2 * 256 * 4 + 4 floats)
BIG = dict(sqdiff_bwd=(2, 1025, 4096), add_rowbcast=(2097155, 4, 5), catte_bwd=(2049, 4096), temporal_mean=(1, 2, 4 * 2097156),
           add_strided=(2, 4 * 1048578), mean_T=(2049, 2, 4096), pair_sqdiff=(683, 3, 4096))
BIG_CPU = dict(sqdiff_bwd=(1, 513, 4), add_rowbcast=(513, 4, 5), catte_bwd=(1, 2052), temporal_mean=(1, 2, 2052),
               add_strided=(1, 2052), mean_T=(1, 2, 2052), pair_sqdiff=(1, 1, 2052))
ROWBCAST_SHORT = (7, 4, 5)                      # M = 7, rows_per_group = 5: the last group is short
PAIR_BWD_CASES = tuple((n, g, K) for n, g in PAIR_BWD_COUNTS for K in PAIR_BWD_K)
CATTE_CASES = tuple((b, Hd, C) for b in CATTE_B for Hd in CATTE_HD for C in CATTE_C)
# (b, T, D, C, extra of ldy / ldo, extra of lddo): every T at one (D, C), every (D, C) at T = 1 and 5, T = 16 at the largest
ATT_CASES = tuple((ATT_B[i % 2], T, 128, 1028, 8 * (i % 2), 8 * ((i // 2) % 2)) for i, T in enumerate(ATT_T)) + \
    tuple((ATT_B[(i + j + t) % 2], T, D, C, 8 * ((i + j) % 2), 8 * ((i + t) % 2))
          for t, T in enumerate((1, 5)) for i, D in enumerate(ATT_D) for j, C in enumerate(ATT_C)) + ((3, 16, 260, 2048, 8, 0),)
CLASSES = ('a', 'b')


def big_items(name, case):
    """float4 items of a grid-stride launch (the wrappers' total4)."""
    n = {'sqdiff_bwd': lambda b, rows, C: b * rows * C, 'add_rowbcast': lambda M, C, rpg: M * C,
         'catte_bwd': lambda b, C: b * C, 'temporal_mean': lambda b, T, inner: b * inner,
         'add_strided': lambda nb, inner: nb * inner, 'mean_T': lambda b, T, C: b * C,
         'pair_sqdiff': lambda n_, g, K: n_ * g * K}[name](*case)
    return n // 4


# the kernels' branch rules, restated (test_head_ref_cpu asserts that the sweep takes both sides of each)
def last_workgroup_has_idle_waves(rows):
    """one wave per row, four per workgroup: `if (m >= M) return` is taken iff rows % 4 != 0"""
    return rows % 4 != 0


def lane_trips(width, stride):
    """(fewest, most) trips of a lane through `for (c = lane * 4; c < width; c += stride)`, over the stride / 4 lanes"""
    return width // stride, (width + stride - 1) // stride


def trips(width, stride):
    return max(1, (width + stride - 1) // stride)


def red16_rows_per_wave(rows):
    """(fewest, most) rows one of the 16 waves adds"""
    return rows // 16, (rows + 15) // 16


def att_rows_per_wave(T):
    """(fewest, most) of the 2 T norm rows a wave of the four takes"""
    return (2 * T) // 4, (2 * T + 3) // 4


# ----------------------------------------------------------------------------------------------------------------------
# inputs: (a) well conditioned, (b) cancelling / saturating
GATE_LOGITS = np.array([-30.0, -8.0, 0.0, 8.0, 30.0])


def rng_for(*key):
    h = 17
    for k in key:
        h = (h * 1000003 + (sum(ord(ch) for ch in k) if isinstance(k, str) else int(k))) % (2 ** 31 - 1)
    return np.random.RandomState(h)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def normal(rng, shape, cls, offset=1000.0, spread=1e-2):
    """(a) standard normal; (b) a large common offset of either sign with a small spread."""
    if cls == 'a':
        return f32(rng.standard_normal(shape))
    return f32(rng.choice([-1.0, 1.0]) * offset + spread * rng.standard_normal(shape))


def post_relu(rng, shape, cls):
    """features that are post-ReLU in the model: |N(0,1)| + 0.1; (b): 1000 + 1e-2 N(0,1)"""
    if cls == 'a':
        return f32(np.abs(rng.standard_normal(shape)) + 0.1)
    return f32(1000.0 + 1e-2 * rng.standard_normal(shape))


def near(rng, a, rel=1e-3):
    """a second operand equal to ``a`` up to ``rel`` relative"""
    return f32(np.asarray(a, np.float64) * (1.0 + rel * rng.standard_normal(np.shape(a))))


def logits(rng, n, cls):
    if cls == 'a':
        return f32(2.0 * rng.standard_normal(n))
    return f32(GATE_LOGITS[(np.arange(n) + rng.randint(5)) % 5])


def in_gate(M, C, ldy, cls):
    """gate_apply / gate_bwd: the logits sit in column 0 of a [M][ldy] buffer; (b): saturating logits, dxc ~ dxu"""
    r = rng_for('gate', M, C, ldy, cls)
    y = f32(r.standard_normal(M * ldy))
    y[np.arange(M) * ldy] = logits(r, M, cls)
    dxc = normal(r, (M, C), cls)
    return dict(y=y, x=normal(r, (M, C), 'a'), dxc=dxc, dxu=near(r, dxc) if cls == 'b' else normal(r, (M, C), 'a'),
                dx0=normal(r, (M, C), 'a'), dy0=f32(r.standard_normal(M * ldy)))


def in_gce(M, Ch, C, cls):
    """gce_gate; (b): the rows of h are rescaled so that the logits land on GATE_LOGITS"""
    r = rng_for('gce', M, Ch, C, cls)
    h, w3 = r.standard_normal((M, Ch)), r.standard_normal(Ch) / np.sqrt(Ch)
    bsc, bsh = (1.3, -0.4) if cls == 'a' else (2.0, -1.0)
    if cls == 'b':
        target = (logits(r, M, 'b').astype(np.float64) - bsh) / bsc
        h = h * (target / (h @ w3))[:, None]
    return dict(h=f32(h), w3=f32(w3), bsc=f32([bsc]), bsh=f32([bsh]), x=normal(r, (M, C), 'a'))


F2_OFFSET = 8           # floats: f2 / df2 are views that start inside a wider buffer


def in_red(groups, rows, C, f2_mult, cls):
    """group_mean, sqdiff_mean, sqdiff_bwd: f2 = window `groups x rows x C` (clip stride f2_mult * rows * C) of a wider
    buffer, starting F2_OFFSET floats in; (b): f2 ~ f1 up to 1e-3 relative on a common offset"""
    r = rng_for('red', groups, rows, C, f2_mult, cls)
    stride = f2_mult * rows * C
    f1 = normal(r, (groups, rows, C), cls)
    n = F2_OFFSET + groups * stride + 4
    f2buf, df2buf = f32(r.standard_normal(n)), f32(r.standard_normal(n))
    for g in range(groups):
        w = near(r, f1[g]) if cls == 'b' else normal(r, (rows, C), 'a')
        f2buf[F2_OFFSET + g * stride:F2_OFFSET + g * stride + rows * C] = w.reshape(-1)
    return dict(x=normal(r, (groups, rows, C), cls), f1=f1, f2buf=f2buf, df2buf=df2buf, stride=stride,
                dd=normal(r, (groups, C), 'a'))


def in_catte(b, Hd, C, cls, T=CATTE_T):
    """channel_atte / catte_bwd: gap, fstep, dfs, dgap are rows `i * T * C + C` of [b][T][C] buffers (T = CATTE_T, step 1);
    (b): the second layer is scaled up so that the sigmoid saturates"""
    r = rng_for('catte', b, Hd, C, cls)
    n = b * T * C
    return dict(d=post_relu(r, (b, C), 'a'), w1=f32(r.standard_normal((Hd, C)) / np.sqrt(C)),
                w2t=f32(r.standard_normal((Hd, C)) * ((1.0 if cls == 'a' else 8.0) / np.sqrt(Hd))),
                gapbuf=post_relu(r, n, cls), fstepbuf=f32(r.standard_normal(n)), dfsbuf=f32(r.standard_normal(n)),
                dgapbuf=f32(r.standard_normal(n)))


def in_l2(rows, C, cls):
    r = rng_for('l2', rows, C, cls)
    return dict(x=normal(r, (rows, C), cls), scale=f32(r.uniform(0.5, 1.5, C)), shift=f32(r.uniform(-0.7, 0.7, C)),
                dy=normal(r, (rows, C), 'a'))


def in_att(b, T, D, C, cls):
    """siamese_attn: x is post-ReLU; (b): Q and K share an offset (scores near 1, a flat softmax), x = 1000 + small"""
    r = rng_for('att', b, T, D, C, cls)
    return dict(qk=normal(r, (b, T, 2 * D), cls, offset=3.0, spread=1.0), x=post_relu(r, (b, T, C), cls),
                dout=normal(r, (b, C), 'a'), dx0=normal(r, (b, T, C), 'a'))


def in_pair(np_, ng, K, cls):
    """pair_sqdiff / pair_verify; (b): every p_i and g_j equals one common vector (offset 1000) up to 1e-3 relative"""
    r = rng_for('pair', np_, ng, K, cls)
    if cls == 'a':
        p, g = normal(r, (np_, K), 'a'), normal(r, (ng, K), 'a')
    else:
        base = normal(r, (1, K), 'b')
        p, g = near(r, np.repeat(base, np_, 0)), near(r, np.repeat(base, ng, 0))
    return dict(p=p, g=g, dd=normal(r, (np_ * ng, K), 'a'), scale=f32(r.uniform(0.5, 1.5, K)), shift=f32(r.uniform(-0.7, 0.7, K)),
                w=f32(r.standard_normal((4, K)) / np.sqrt(K)), bias=f32(r.standard_normal(4)))


# ----------------------------------------------------------------------------------------------------------------------
# summation depths
def k_wave_dot(width):
    return 1 + 3 + trips(width, 256) + 6


def k_block_dot(width):
    return 1 + 3 + trips(width, 1024) + 6 + 4


def k_red16(rows):
    return (rows + 15) // 16 + 2 + 4


# ----------------------------------------------------------------------------------------------------------------------
# bounds.  e_* : first-order error, WITHOUT SAFETY (they compose);  b_* : what a test compares against (with SAFETY).
def e_sigmoid(z, e_z=0.0):
    """g = 1 / (1 + expf(-z)): the argument's error and expf's reach g through dg/dz = g (1 - g); the addition rounds once and
    the division DIV_ULP ulp, both relative to g."""
    g = H.sigmoid(z)
    return g * (1.0 - g) * (e_z + EXPF_ULP * ULP) + g * (U + DIV_ULP * ULP)


def gate_forward_bounds(x, g, e_g):
    """cmap; xc = fl(x g): |x| e_g + u |xc|;  gu = fl(1 - g): e_g + u (1 - g);  xu = fl(x gu): |x| e_gu + u |xu|."""
    ax = np.abs(H.f64(x))
    g, e_g = np.asarray(g)[:, None], np.asarray(e_g)[:, None]
    e_gu = e_g + U * (1.0 - g)
    return dict(cmap=SAFETY * e_g[:, 0], xc=SAFETY * (ax * e_g + U * ax * g), xu=SAFETY * (ax * e_gu + U * ax * (1.0 - g)))


def b_gate_apply(ref, x):
    return gate_forward_bounds(x, ref['cmap'], e_sigmoid(ref['logit']))


def e_gce_logit(ref, bn_scale, Ch):
    """s: a wave dot of Ch terms; logit = fl(fl(s * scale) + shift): |scale| e_s + 2 u (|s scale| + |shift|)"""
    return abs(float(bn_scale)) * k_wave_dot(Ch) * U * ref['abs_s'] + 2 * U * ref['abs_logit']


def b_gce_gate(ref, x, bn_scale, Ch):
    return gate_forward_bounds(x, ref['cmap'], e_sigmoid(ref['logit'], e_gce_logit(ref, bn_scale, Ch)))


def b_gate_bwd(ref, C, accumulate, e_g=None, dxc=None, dxu=None):
    """dx = fl(fl(a g) + fl(b fl(1 - g))) (+ dx0): the longest chain (1 - g, the product, the sum, the accumulate) has
    3 + accumulate roundings on |a g| + |b (1 - g)| (+ |dx0|).   dy = fl(fl(s g) gu): s is a wave dot of fl(a - b) x
    (k_wave_dot + 1 for the subtraction), then 1 - g and two products: 3 u |dy|.
    e_g (end to end: the map is the forward's, off by e_g): dx moves by |a - b| e_g, dy by |s| |1 - 2 g| e_g."""
    e_dx = (3 + (1 if accumulate else 0)) * U * ref['abs_dx']
    e_dy = (k_wave_dot(C) + 1) * U * ref['abs_s'] * ref['gg'] + 3 * U * np.abs(ref['dy_col'])
    if e_g is not None:
        e_dx = e_dx + np.abs(H.f64(dxc) - H.f64(dxu)) * np.asarray(e_g)[:, None]
        e_dy = e_dy + np.abs(ref['s']) * np.abs(1.0 - 2.0 * ref['g']) * e_g
    return dict(dx=SAFETY * e_dx, dy=SAFETY * e_dy)


def b_group_mean(ref, rows, accumulate):
    """red16 sum, times mul = fl(out_scale / rows) (two roundings), (+ y: one more, relative to the result)"""
    return SAFETY * U * ((k_red16(rows) + 2) * ref['abs_mean'] + (np.abs(ref['val']) if accumulate else 0.0))


def b_sqdiff_mean(ref, rows):
    """t = fl(f1 - f2), fl(t t): 3 roundings per term; red16; times fl(1 / rows): 2"""
    return SAFETY * U * (3 + k_red16(rows) + 2) * ref['d']


def b_sqdiff_bwd(ref, accumulate):
    """g = fl(fl(fl(f1 - f2) dd) fl(2 / rows)): 4 u |g|;  df2 = -g (+ df2): one more, relative to the result"""
    b1 = SAFETY * 4 * U * np.abs(ref['df1'])
    return dict(df1=b1, df2=b1 + (SAFETY * U * np.abs(ref['df2_val']) if accumulate else 0.0))


def b_mean_over_T(abs_mean, T):
    """T - 1 additions, fl(1 / T), the product"""
    return SAFETY * (T + 1) * U * abs_mean


def b_add_strided(ref):
    return SAFETY * U * np.abs(ref['y'])


def b_add_rowbcast(ref, accumulate):
    return SAFETY * U * (np.abs(ref['term']) + (np.abs(ref['dst']) if accumulate else 0.0))


def channel_atte_bounds(ref, C, Hd, accumulate):
    """hid = relu(wave dot of C terms) (the ReLU is 1-Lipschitz);  logit[n] = sum_j w2t[j][n] hid[j], Hd sequential
    multiply-adds: (Hd + 1) u sum|w2t hid| + sum|w2t| e_hid;  catte: the sigmoid;  fstep = fl(fl(g a) + g) (+ fstep)."""
    e_hid = k_wave_dot(C) * U * ref['abs_hid']
    aw = np.abs(ref['w2t'])
    e_z = (Hd + 1) * U * (ref['hid'] @ aw) + e_hid @ aw
    e_a = e_sigmoid(ref['logit'], e_z)
    ag = np.abs(ref['gap'])
    e_f = ag * e_a + U * ag * ref['a'] + U * np.abs(ref['term']) + (U * np.abs(ref['fstep_val']) if accumulate else 0.0)
    return dict(hid=SAFETY * e_hid, catte=SAFETY * e_a, fstep=SAFETY * e_f, e_catte=e_a)


def b_catte_bwd(ref, catte, accumulate, e_a=None):
    """ds = fl(fl(fl(d g) a) fl(1 - a)): 4 u |ds|;  dgap = fl(d fl(1 + a)) (+ dgap): 2 u |term| + u |result|.
    e_a (end to end): ds moves by |d g| |1 - 2 a| e_a, dgap by |d| e_a."""
    a = H.f64(catte).reshape(ref['ds'].shape)
    e_ds = 4 * U * np.abs(ref['ds'])
    e_dg = 2 * U * np.abs(ref['term']) + (U * np.abs(ref['dgap_val']) if accumulate else 0.0)
    if e_a is not None:
        e_ds = e_ds + np.abs(ref['dfs'] * ref['gap']) * np.abs(1.0 - 2.0 * a) * e_a
        e_dg = e_dg + np.abs(ref['dfs']) * e_a
    return dict(ds=SAFETY * e_ds, dgap=SAFETY * e_dg)


def e_inv_norm(ss, e_ss):
    """inv = 1 / sqrtf(ss) from a sum of squares off by e_ss: sqrt halves the relative error and adds SQRT_ULP ulp, the
    division DIV_ULP ulp"""
    nrm = np.sqrt(ss)
    e_nrm = e_ss / (2.0 * nrm) + SQRT_ULP * ULP * nrm
    return e_nrm / (nrm * nrm) + DIV_ULP * ULP / nrm


def affine_l2norm_bounds(ref, C, affine):
    """v = fl(fl(x s) + t): 2 u (|x s| + |t|);  ss = block dot of v v: sum 2 |v| e_v + k u ss;  y = fl(v inv)."""
    e_v = 2 * U * ref['abs_v'] if affine else np.zeros_like(ref['v'])
    e_ss = (2 * np.abs(ref['v']) * e_v).sum(1) + k_block_dot(C) * U * ref['ss']
    e_inv = e_inv_norm(ref['ss'], e_ss)[:, None]
    inv = 1.0 / np.sqrt(ref['ss'])[:, None]
    e_y = e_v * inv + np.abs(ref['v']) * e_inv + U * np.abs(ref['val'])
    return dict(y=SAFETY * e_y, e_y=e_y)


def b_l2norm_bwd(ref, C, e_y=None):
    """dot = block dot of dy y; inv from the block dot of v v; dv = fl(fl(a - fl(b dot)) inv): 3 u (|a| + |b dot|) inv
    + |b| e_dot inv + |a - b dot| e_inv.   e_y (end to end): dot moves by sum |dy| e_y, dv by (e_y |dot| + |y| that) inv."""
    a, b = ref['dy'], ref['y']
    dot = ref['dot'][:, None]
    e_dot = (k_block_dot(C) * U * ref['abs_dot'])[:, None]
    e_b = 0.0
    if e_y is not None:
        e_dot = e_dot + (np.abs(a) * e_y).sum(1)[:, None]
        e_b = e_y
    inv = 1.0 / np.sqrt(ref['ss'])[:, None]
    e_inv = e_inv_norm(ref['ss'], k_block_dot(C) * U * ref['ss'])[:, None]
    return SAFETY * (3 * U * (np.abs(a) + np.abs(b * dot)) * inv + (np.abs(b) * e_dot + e_b * np.abs(dot)) * inv
                     + np.abs(a - b * dot) * e_inv)


def b_row_sqnorm(ref, K):
    return SAFETY * k_block_dot(K) * U * ref['out']


def attn_forward_errors(fw, T, D, C):
    """siamese_attn, stage by stage (see the module docstring for the depths):
    inv norms: relative r = k_wave_dot(D) u / 2 + (SQRT_ULP + DIV_ULP) ulp;
    S_ij = fl(fl(dot inv_i) inv_j): (k_wave_dot(D) u + 2 r + 2 u) sum|qh kh|;
    e_ij = expf(fl(S_ij - mx)): the softmax does not depend on mx, so only S_ij's own error, u |S_ij - mx| <= 2 u and expf's
    EXPF_ULP ulp count: relative r_e;  P_ij = fl(e_ij fl(1 / sum)): r_e_ij + sum_k P_ik r_e_ik + T u (the sum) + DIV_ULP ulp + u;
    w_j = sum_i P_ij: T additions;  raw = sum_j fl(x_j w_j): (T + 1) u;  |raw|^2: block dot;  out = fl(raw inv)."""
    r = 0.5 * k_wave_dot(D) * U + (SQRT_ULP + DIV_ULP) * ULP
    e_S = (k_wave_dot(D) * U + 2 * r + 2 * U) * fw['abs_S']
    r_e = e_S + 2 * U + EXPF_ULP * ULP
    P, w, x = fw['P'], fw['w'], fw['x']
    e_P = P * (r_e + (P * r_e).sum(2, keepdims=True) + (T + 1) * U + DIV_ULP * ULP)
    e_w = e_P.sum(1) + T * U * w
    e_raw = np.einsum('bj,bjc->bc', e_w + (T + 1) * U * w, np.abs(x))
    ss = fw['nraw'] ** 2
    e_ss = (2 * np.abs(fw['raw']) * e_raw).sum(1) + k_block_dot(C) * U * ss
    e_invr = e_inv_norm(ss, e_ss)
    e_out = e_raw / fw['nraw'][:, None] + np.abs(fw['raw']) * e_invr[:, None] + U * np.abs(fw['out'])
    return dict(r=r, e_S=e_S, e_P=e_P, e_w=e_w, e_raw=e_raw, e_invr=e_invr, e_out=e_out)


def b_siamese_attn(fw, T, D, C):
    return SAFETY * attn_forward_errors(fw, T, D, C)['e_out']


def b_siamese_attn_bwd(bw, T, D, C, accumulate, e_out=None):
    """siamese_attn_bwd recomputes P, w and |raw| (attn_forward_errors) and then, with `out` as handed in:
    od = block dot of out dout;  draw = fl(fl(dout - fl(out od)) inv): 3 roundings;  dx_j = fl(draw w_j) (+ dx);
    dw_j = block dot of draw x_j;  s_i = sum_k fl(P_ik dw_k): T + 1;  dS_ij = fl(P_ij fl(dw_j - s_i));
    dqh_i = sum_o fl(kh-row fl(dS_io inv_o)): T + 2 roundings and inv's r;  dot_i = wave dot of dqh qh (one more product, r);
    dQ = fl(fl(dqh - fl(fl(q inv) dot)) inv).   e_out (end to end): `out` itself is off by e_out."""
    fw = bw['fw']
    fe = attn_forward_errors(fw, T, D, C)
    r, e_P, e_w = fe['r'], fe['e_P'], fe['e_w']
    o, do, od = bw['out'], bw['dout'], bw['od'][:, None]
    nraw = fw['nraw'][:, None]
    e_o = np.zeros_like(o) if e_out is None else e_out
    e_od = (k_block_dot(C) * U * np.abs(o * do).sum(1) + (np.abs(do) * e_o).sum(1))[:, None]
    e_draw = (3 * U * (np.abs(do) + np.abs(o * od)) + np.abs(o) * e_od + np.abs(od) * e_o) / nraw + \
        np.abs(do - o * od) * fe['e_invr'][:, None]
    draw, x, w = bw['draw'], fw['x'], fw['w']
    e_dx = e_draw[:, None, :] * w[:, :, None] + np.abs(draw)[:, None, :] * e_w[:, :, None] + U * np.abs(bw['dx_term']) + \
        (U * np.abs(bw['dx']) if accumulate else 0.0)
    dw, P, sp = bw['dw'], fw['P'], bw['sp']
    e_dw = np.einsum('bc,bjc->bj', e_draw, np.abs(x)) + k_block_dot(C) * U * np.einsum('bc,bjc->bj', np.abs(draw), np.abs(x))
    e_sp = (e_P * np.abs(dw)[:, None, :] + P * e_dw[:, None, :]).sum(2) + (T + 1) * U * (P * np.abs(dw)[:, None, :]).sum(2)
    diff = dw[:, None, :] - sp[:, :, None]
    e_dS = e_P * np.abs(diff) + P * (e_dw[:, None, :] + e_sp[:, :, None] + U * (np.abs(dw)[:, None, :] + np.abs(sp)[:, :, None])) + \
        U * np.abs(bw['dS'])
    c = e_dS + np.abs(bw['dS']) * (r + (T + 2) * U)
    out = []
    for hat, other, dhat, nrm, ein in ((fw['qh'], fw['kh'], bw['dqh'], fw['nq'], 'bij,bjd->bid'),
                                       (fw['kh'], fw['qh'], bw['dkh'], fw['nk'], 'bij,bid->bjd')):
        e_dh = np.einsum(ein, c, np.abs(other))
        t = np.abs(dhat * hat).sum(2, keepdims=True)
        dot = (dhat * hat).sum(2, keepdims=True)
        e_dot = (np.abs(hat) * e_dh).sum(2, keepdims=True) + ((k_wave_dot(D) + 1) * U + r) * t
        hd = np.abs(hat * dot)
        res = (dhat - hat * dot) / nrm[..., None]
        out.append((e_dh + np.abs(hat) * e_dot + hd * (r + 2 * U) + U * (np.abs(dhat) + hd)) / nrm[..., None] + np.abs(res) * (r + U))
    return dict(dx=SAFETY * e_dx, dqk=SAFETY * np.stack(out, 2))


def b_pair_sqdiff(ref):
    """d = fl(p - g), fl(d d): 3 u"""
    return SAFETY * 3 * U * ref['diff']


def b_pair_sqdiff_bwd(ref, np_, ng):
    """s += fl(fl(p - g) dd): 2 roundings and ng (np) sequential additions; the final * 2 is exact"""
    return dict(dp=SAFETY * (ng + 2) * U * ref['abs_dp'], dg=SAFETY * (np_ + 2) * U * ref['abs_dg'])


def b_pair_verify(ref, K, affine, bias):
    """d d: 3 roundings (+ 2 for fl(fl(d s) + t)), a wave dot of K terms with W, (+ bias: u |out|)"""
    return SAFETY * U * ((k_wave_dot(K) + (5 if affine else 3)) * ref['abs_out'] + (np.abs(ref['out']) if bias else 0.0))


# ----------------------------------------------------------------------------------------------------------------------
# fp32 restatements of the reductions, in the kernels' order (numpy, CPU): the bounds are satisfiable
F = np.float32


def _dot4(p):
    return ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]


def _butterfly(v):
    """wave_sum: v += v[lane ^ o], o = 32 .. 1, over the last axis (64 lanes)"""
    o = 32
    while o:
        v = v + v[..., np.arange(64) ^ o]
        o >>= 1
    return v[..., 0]


def _lanes(prod, stride):
    """products [..., W] -> per-lane partial sums [..., stride / 4]: s += dot4 per trip (zero padding adds exactly 0)"""
    W = prod.shape[-1]
    pad = (-W) % stride
    p = np.concatenate([prod, np.zeros(prod.shape[:-1] + (pad,), F)], -1).reshape(prod.shape[:-1] + (-1, stride // 4, 4))
    s = np.zeros(p.shape[:-3] + (stride // 4,), F)
    for t in range(p.shape[-3]):
        s = s + _dot4(p[..., t, :, :])
    return s


def wave_dot_f32(a, b):
    """sum over the last axis as one wave computes it (lane stride 256, dot4, wave_sum)"""
    return _butterfly(_lanes(F(a) * F(b), 256))


def block_dot_f32(a, b):
    """... as a 256-thread workgroup computes it (stride 1024, dot4, wave_sum per wave, block_sum's four additions)"""
    lanes = _lanes(F(a) * F(b), 1024)
    red = _butterfly(lanes.reshape(lanes.shape[:-1] + (4, 64)))
    t = np.zeros(red.shape[:-1], F)
    for i in range(4):
        t = t + red[..., i]
    return t


def red16_f32(terms):
    """terms [rows][C] -> [C] as group_mean_kernel / sqdiff_mean_kernel add them: wave w takes rows w, w + 16, ...;
    then ((r0 + r1) + (r2 + r3)) per four waves, added in sequence"""
    terms = F(terms)
    red = np.zeros((16,) + terms.shape[1:], F)
    for w in range(16):
        for r in range(w, terms.shape[0], 16):
            red[w] = red[w] + terms[r]
    t = np.zeros(terms.shape[1:], F)
    for w in range(0, 16, 4):
        t = t + ((red[w] + red[w + 1]) + (red[w + 2] + red[w + 3]))
    return t


def sigmoid_f32(z):
    return F(1) / (F(1) + np.exp(-F(z)).astype(F))


def gce_gate_f32(h, w3, bsc, bsh, x):
    s = wave_dot_f32(h, F(w3)[None, :])
    g = sigmoid_f32(s * F(bsc) + F(bsh))
    return dict(cmap=g, xc=F(x) * g[:, None], xu=F(x) * (F(1) - g)[:, None])


def gate_bwd_dy_f32(dxc, dxu, x, cmap):
    g = F(cmap)
    return wave_dot_f32(F(dxc) - F(dxu), x) * g * (F(1) - g)


def group_mean_f32(x, rows, out_scale, y0=None):
    """x [groups][rows][C]"""
    mul = F(out_scale) / F(rows)
    t = np.stack([red16_f32(g) for g in F(x)]) * mul
    return t if y0 is None else t + F(y0)


def sqdiff_mean_f32(f1, f2, rows):
    out = []
    for a, b in zip(F(f1), F(f2)):
        t = a - b
        out.append(red16_f32(t * t) * (F(1) / F(rows)))
    return np.stack(out)


def affine_l2norm_f32(x, scale, shift):
    v = F(x) if scale is None else F(x) * F(scale) + F(shift)
    inv = F(1) / np.sqrt(block_dot_f32(v, v))
    return v * inv[:, None]


def l2norm_bwd_f32(dy, y, v):
    dot = block_dot_f32(dy, y)
    inv = F(1) / np.sqrt(block_dot_f32(v, v))
    return (F(dy) - F(y) * dot[:, None]) * inv[:, None]


def siamese_attn_f32(qk, x, b, T, D, C):
    """scores, softmax, pooling weights, pooling and the final normalisation in the kernel's order"""
    qk = F(qk).reshape(b, T, 2, D)
    x = F(x).reshape(b, T, C)
    q, k = qk[:, :, 0], qk[:, :, 1]
    iq, ik = F(1) / np.sqrt(wave_dot_f32(q, q)), F(1) / np.sqrt(wave_dot_f32(k, k))
    S = wave_dot_f32(q[:, :, None, :], k[:, None, :, :]) * iq[:, :, None] * ik[:, None, :]
    e = np.exp(S - S.max(2, keepdims=True)).astype(F)
    tot = np.zeros((b, T), F)
    for j in range(T):
        tot = tot + e[:, :, j]
    P = e * (F(1) / tot)[:, :, None]
    w = np.zeros((b, T), F)
    for i in range(T):
        w = w + P[:, i, :]
    raw = np.zeros((b, C), F)
    for j in range(T):
        raw = raw + x[:, j] * w[:, j, None]
    inv = F(1) / np.sqrt(block_dot_f32(raw, raw))
    return raw * inv[:, None]
