"""Shapes, inputs, first-order rounding-error bounds and fp32 restatements of the summation order for the OIM, triplet and
pair-verification loss kernels (loss.hip, oim_update_kernel of train_head.hip) -- shared by test_loss_ref_cpu.py (no GPU) and
test_gpu_loss_float64.py.  U, SAFETY, check, RATIOS, dump_ratios are bn_bounds' own; rng_for, normal, near, f32, the libm
constants EXPF_ULP, SQRT_ULP, DIV_ULP, e_inv_norm and k_block_dot are head_bounds' own.

Bounds are derived per element, none is fitted: depth of the fp32 chain read from the kernel x u x sum|terms| (u = 2^-24,
-ffp-contract=off: every * and + rounds once; the one explicit fmaf of oim_grad_kernel rounds once per step), errors of a
stage that feed the next carried through the derivative, SAFETY (2) once at the end.  s(t) below is the number of strided
trips a lane makes: trips(width, stride).

LOGF_ULP is ASSUMED (no copy of the ROCm math-function accuracy tables was at hand), not measured and not tuned against the
kernels: 2 ulp for logf, an ulp at most 2 u relative -- as EXPF_ULP, SQRT_ULP, DIV_ULP of head_bounds.py.

TINY = 2^-126, the smallest normal fp32, is added wherever a result may fall below it: the device may flush such a result to
zero where float64 keeps it (exp(-240) is 5.9e-105 in float64 and exactly 0 in fp32)."""
import numpy as np

import loss_ref as R
from bn_bounds import U, SAFETY, check, RATIOS, dump_ratios                                     # noqa: F401
from head_bounds import (rng_for, normal, near, f32, trips, lane_trips, EXPF_ULP, SQRT_ULP, DIV_ULP, ULP,     # noqa: F401
                         e_inv_norm, k_block_dot, block_dot_f32, _butterfly)

LOGF_ULP = 2.0      # assumed
TINY = 2.0 ** -126
F = np.float32

# ----------------------------------------------------------------------------------------------------------------------
# the sweep (the smallest shapes that reach each branch)
CE_N = (1, 3, 9)
CE_C = (1, 3, 63, 64, 65, 255, 256, 257, 513, 1027)
CE_LABELS = ('valid', 'mixed', 'none')      # all valid / one -100 and one c (just out of range) among valid / all invalid
CE_CLASSES = ('a', 'b', 't')
CE_TIES = ((3, 259), (5, 70), (200, 100))   # same lane, second trip / two waves / the later index first in memory order
# (n, c, cls): (a) and (b) on every n x c; the tie class where a pair fits, with 3 and 9 rows (9: every pair x label position)
CE_CASES = tuple((n, c, cls) for n in CE_N for c in CE_C for cls in ('a', 'b')) + \
    tuple((n, c, 't') for n in (3, 9) for c in (257, 513, 1027))


# (ld > c, weight, dlogits, correct): every case and label pattern launches all sixteen
CE_FLAGS = tuple((bool(v & 1), bool(v & 2), bool(v & 4), bool(v & 8)) for v in range(16))


OG_N = (1, 7, 8, 9, 17)
OG_C = (1, 3, 4, 5, 2048, 2049, 5120)
OG_D = (1, 4, 255, 256, 257, 513)
OG_ROWS, OG_LDS_OPT_IN, OG_MAX_C = 8, 65536, 5120
# (n, c, D, ldd - c, g given): every value of each axis at least once, c >= 2048 only with n <= 9
OG_CASES = ((1, 1, 1, 0, True), (7, 3, 4, 3, False), (8, 4, 255, 0, True), (9, 5, 256, 3, False), (17, 5, 257, 0, True),
            (17, 3, 513, 3, True), (8, 2048, 257, 3, False), (9, 2049, 4, 0, True), (7, 2049, 256, 3, False),
            (1, 5120, 257, 3, True), (9, 5120, 1, 0, False), (9, 2048, 513, 0, True))

TRI_N = (1, 2, 3, 4, 5, 9)
TRI_D = (4, 252, 256, 260, 1028)
TRI_IDS = ('distinct', 'equal', 'pairs', 'singleton')
TRI_MARGINS = ('soft', 0.3)
TRI_CLASSES = ('a', 'b', 't')
TRI_CASES = tuple((n, D) for n in TRI_N for D in TRI_D)

SM2_M = (1, 255, 256, 257, 513)
PAIR_N = (1, 2, 15, 16, 17, 23)
PAIR_CLASSES = ('a', 'b')                   # (b) holds the ties too: s = 0.5 with y = 0 and y = 1
PAIR_EDGE = (0.0, 1e-30, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24, 1.0)
SCALE_N = (1, 255, 257)
SCALE_BIG = 1048576 + 260                   # 4096 workgroups x 256 threads cover 1 048 576 items: the stride loop's second pass
SCALE_BIG_CPU = 2 * 256 + 4
SCALE_GRID_CAP = 4096

UPD_D = (4, 1020, 1024, 1028, 2052)
UPD_CLASSES_N = 6
UPD_MOMENTA = (0.5, 0.0)
UPD_LABELS = ((2,), (5, 5, 5), (3, 1, 3, 0, 1, 3), (2, 10 ** 6, -100, 2, 5))
CLASSES = ('a', 'b')


# the kernels' branch rules, restated (test_loss_ref_cpu asserts that the sweep takes both sides of each)
def og_lds_bytes(c):
    return OG_ROWS * ((c + 3) // 4 * 4) * 4


def tri_wave_columns(n):
    """(fewest, most) columns j one of the four waves of triplet_fwd_kernel takes"""
    return n // 4, (n + 3) // 4


def pair_lane_trips(n):
    return lane_trips(n * n, 256)


# ----------------------------------------------------------------------------------------------------------------------
# inputs
def ce_labels(rng, n, c, pattern):
    y = rng.randint(0, c, n).astype(np.int64)
    if pattern == 'none':
        y[:] = np.where(np.arange(n) % 2 == 0, -100, c)
    elif pattern == 'mixed':
        if n == 1:
            y[0] = c
        else:
            y[0], y[n - 1] = -100, c
    return y


def in_softmax_ce(n, c, ld, cls, pattern):
    """(a) 30 cos(.) in [-30, 30]; (b) rows in turn: all equal / one class at +1e4 and the rest at -1e4 / the label's logit
    1e-3 below the maximum; (t) as (a) with the row maximum planted twice (CE_TIES, those that fit) and the label on the first,
    the second or neither.  The logits live in an ld-wide buffer whose columns past c hold large values a kernel must not read."""
    r = rng_for('ce', n, c, ld, cls, pattern)
    z = f32(30.0 * np.cos(r.uniform(0.0, 2.0 * np.pi, (n, c))))
    y = ce_labels(r, n, c, pattern)
    ok = (y >= 0) & (y < c)
    for i in range(n):
        if cls == 'b':
            kind = i % 3
            if kind == 0:
                z[i] = z[i, 0]
            elif kind == 1:
                z[i] = -1e4
                z[i, r.randint(c)] = 1e4
            elif ok[i] and c > 1:
                j = (y[i] + 1 + r.randint(c - 1)) % c
                z[i, j] = 31.0
                z[i, y[i]] = F(31.0 - 1e-3)
        elif cls == 't':
            fits = [p for p in CE_TIES if max(p) < c]
            a, b = fits[i % len(fits)]
            z[i, a] = z[i, b] = 31.0
            if ok[i]:
                where = (i // 3) % 3
                y[i] = (min(a, b), max(a, b), (max(a, b) + 1) % c)[where]
    buf = f32(np.full((n, ld), 1e30))
    buf[:, :c] = z
    return dict(logits=buf.reshape(-1), labels=y, weight=f32(r.uniform(0.5, 1.5, c)))


def unit_rows(a):
    a = np.asarray(a, np.float64)
    return f32(a / np.sqrt((a * a).sum(-1, keepdims=True)))


def in_oim_grad(n, c, D, ldd, cls):
    """(a) dl ~ 1e-2 N(0,1), unit-norm LUT rows; (b) cancelling: dl = softmax - onehot (rows sum to 0) against LUT rows that
    all equal one unit vector up to 1e-3"""
    r = rng_for('og', n, c, D, ldd, cls)
    dl = f32(np.full((n, ldd), 1e30))
    if cls == 'a':
        dl[:, :c] = 1e-2 * r.standard_normal((n, c))
        lut = unit_rows(r.standard_normal((c, D)))
    else:
        e = np.exp(2.0 * r.standard_normal((n, c)))
        p = e / e.sum(1, keepdims=True)
        p[np.arange(n), r.randint(0, c, n)] -= 1.0
        dl[:, :c] = p
        lut = unit_rows(r.standard_normal((1, D)) + 1e-3 * r.standard_normal((c, D)))
    return dict(dl=dl.reshape(-1), lut=lut, g=f32([r.uniform(0.5, 1.5)]), alpha=30.0)


def tri_ids(n, pattern):
    i = np.arange(n, dtype=np.int64)
    if pattern == 'distinct':
        return i * 7 + 3
    if pattern == 'equal':
        return np.full(n, 11, np.int64)
    if pattern == 'pairs':
        return i // 2 + 40
    return np.where(i == 0, 999, (i - 1) // 2 + 40)          # one singleton, then pairs


def in_triplet(n, D, cls, pattern, seed=0):
    """(a) 0.05 N(0,1); (b) a +-1e3 offset with 1e-2 spread; (t) as (a) with rows duplicated exactly (row 1 = row 0, the last
    row = row 2, ...): two candidates have bit-identical distances."""
    r = rng_for('tri', n, D, cls, pattern, seed)
    if cls == 'b':
        f = normal(r, (n, D), 'b')
    else:
        f = f32(0.05 * r.standard_normal((n, D)))
    if cls == 't':
        for dst, src in ((1, 0), (n - 1, 2), (3, 0)):
            if 0 <= src < dst < n:
                f[dst] = f[src]
    return dict(f=f, ids=tri_ids(n, pattern), dloss=f32(r.uniform(0.5, 1.5, n)))


def in_softmax2(m, cls):
    r = rng_for('sm2', m, cls)
    if cls == 'a':
        s = f32(3.0 * r.standard_normal((m, 2)))
    else:
        s = f32(np.array([(120.0, -120.0), (-120.0, 120.0), (7.25, 7.25)])[(np.arange(m) + r.randint(3)) % 3])
    return dict(scores=s, dp=f32(r.standard_normal(m)))


def in_pair(n, cls):
    """(a) probabilities in [0.02, 0.98]; (b) drawn from PAIR_EDGE, and every edge value planted once under y = 0 and once under
    y = 1 as far as the batch has elements of that kind (0.5, the tie, first; n >= 15 holds all twelve combinations).
    ids: three identities and one gallery id nobody has"""
    r = rng_for('pairbce', n, cls)
    tp = (np.arange(n) % 3).astype(np.int64)
    tg = (np.arange(n)[::-1] % 3).astype(np.int64)
    if n > 3:
        tg[3] = 99
    if cls == 'a':
        s = f32(r.uniform(0.02, 0.98, (n, n)))
    else:
        s = f32(np.array(PAIR_EDGE)[r.randint(0, len(PAIR_EDGE), (n, n))])
        y = tp[None, :] == tg[:, None]
        for want in (False, True):
            idx = np.argwhere(y == want)
            for k, v in enumerate((0.5,) + tuple(e for e in PAIR_EDGE if e != 0.5)):
                if k < len(idx):
                    s[tuple(idx[k])] = v
    return dict(prob=s, tp=tp, tg=tg)


def in_oim_update(D, labels, momentum, cls):
    """(a) unit-norm table and samples; (b) every sample nearly anti-parallel to the (initial) row of its label: at momentum 0.5
    the blend cancels to ~1e-2 of its terms before it is normalised"""
    r = rng_for('upd', D, len(labels), sum(abs(l) % 97 for l in labels), int(momentum * 10), cls)
    lut = unit_rows(r.standard_normal((UPD_CLASSES_N, D)))
    n = len(labels)
    x = unit_rows(r.standard_normal((n, D)))
    if cls == 'b':
        for j, y in enumerate(labels):
            if 0 <= y < UPD_CLASSES_N:
                x[j] = f32(-0.99 * lut[y].astype(np.float64) + 1e-3 * r.standard_normal(D))
    return dict(lut=lut, x=x, labels=np.asarray(labels, np.int64))


# ----------------------------------------------------------------------------------------------------------------------
# bounds.  e_* : first-order error, WITHOUT SAFETY (they compose);  b_* : what a test compares against (with SAFETY).
def k_ce_rowsum(c):
    """softmax_ce_kernel's sum of exponentials: s(t) strided trips of 256 + 6 shuffle levels + the 4 additions of block_sum"""
    return trips(c, 256) + 6 + 4


def b_softmax_ce(ref, n, c):
    """t_j = fl(z_j - mx): u |t_j| (mx itself is exact);  e_j = expf(t_j): relative u |t_j| + EXPF_ULP ulp;
    s = sum e_j: k_ce_rowsum;  lse = logf(s): e_s / s + LOGF_ULP ulp |lse| -- absolute: with one dominant class fp32 has s = 1 and
    lse = 0 exactly where the true value is about e^t;
    wsum: n - 1 serial additions of positive weights, gscale = wy / wsum: relative (n - 1) u + DIV_ULP ulp;
    row = fl(gscale fl(lse - fl(z_y - mx))): gscale (e_lse + u |t_y| + u (|lse| + |t_y|)) + |row| (r_gscale + u);
    loss: n - 1 serial additions in rows_sum_kernel;
    p = expf(fl(fl(z_j - mx) - lse)): relative u |t_j| + e_lse + u |t_j - lse| + EXPF_ULP ulp;
    dz = fl(gscale fl(p - onehot)): gscale (p r_p + u |p - onehot|) + |dz| (r_gscale + u)."""
    at = np.abs(ref['t'])
    e_s = (ref['e'] * (U * at + EXPF_ULP * ULP)).sum(1) + k_ce_rowsum(c) * U * ref['s'] + TINY
    e_lse = e_s / ref['s'] + LOGF_ULP * ULP * np.abs(ref['lse'])
    r_g = (n - 1) * U + DIV_ULP * ULP
    g, aty = ref['gscale'], np.abs(ref['ty'])
    e_row = np.where(ref['ok'], g * (e_lse + U * aty + U * (np.abs(ref['lse']) + aty)) + np.abs(ref['rows']) * (r_g + U), 0.0)
    e_loss = e_row.sum() + (n - 1) * U * np.abs(ref['rows']).sum()
    r_p = U * at + e_lse[:, None] + U * np.abs(ref['t'] - ref['lse'][:, None]) + EXPF_ULP * ULP
    pm = np.abs(ref['p'] - ref['onehot'])
    e_dz = g[:, None] * (ref['p'] * r_p + U * pm + TINY) + np.abs(ref['dz_val']) * (r_g + U)
    return dict(rows=SAFETY * e_row, loss=SAFETY * e_loss, dz=SAFETY * e_dz)


def b_oim_grad(ref, c):
    """c sequential fmaf steps (one rounding each) on sum |dl lut|, a = fl(alpha g) and the product: 2 more"""
    return SAFETY * (c + 2) * U * ref['abs_dx']


def k_tri_dist(D):
    """per term: fl(f_i - f_j) enters squared (2), the product (1), the four-term dot's additions (3), the lane's s(t) trips of
    256 floats, 6 shuffle levels"""
    return 2 + 1 + 3 + trips(D, 256) + 6


def e_tri_dist(ref, D):
    """s + 1e-12f: the constant is fp32 (u 1e-12) and the addition rounds (u (s + 1e-12)); sqrtf halves the relative error and
    adds SQRT_ULP ulp"""
    ss = ref['ss']
    e_ss = k_tri_dist(D) * U * ss + U * R.EPS_DIST + U * (ss + R.EPS_DIST)
    return e_ss / (2.0 * ref['dist']) + SQRT_ULP * ULP * ref['dist']


def b_tri_dist(ref, D):
    return SAFETY * e_tri_dist(ref, D)


def e_tri_loss(z, soft, margin32, e_z=0.0):
    """soft: e = expf(z): e (e_z + EXPF_ULP ulp); 1 + e rounds (u (1 + e)); logf: that / (1 + e) + LOGF_ULP ulp |loss| --
    absolute: for z << 0 fp32 has log(1) = 0 where the true value is about e^z.   hinge: fl(z + margin): e_z + u |z + margin|."""
    z = np.asarray(z, np.float64)
    if soft:
        e = np.exp(np.minimum(z, 80.0))
        loss = np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))
        return (e * (e_z + EXPF_ULP * ULP) + U * (1.0 + e)) / (1.0 + e) + LOGF_ULP * ULP * loss + TINY
    return e_z + U * np.abs(z + float(margin32))


def r_gz(soft):
    """relative error of gz = dloss * (ez / (1 + ez)) given z: expf (its error reaches the quotient through 1 - sigmoid <= 1),
    the addition, the division, the product;  the hinge's dloss * 1 is exact"""
    return EXPF_ULP * ULP + 2 * U + DIV_ULP * ULP if soft else 0.0


def b_tri_bwd(ref, soft, e_gz=None, e_dist=None, dist=None, sel=None):
    """per contributing term (f_r - f_o) * (gz / d): the subtraction, gz (r_gz), the division, the product; then one addition
    per term on the same chain: (1 + r_gz + DIV_ULP ulp + 1 + terms) u-units on the element's sum of absolute terms.
    End to end (e_gz, e_dist given): the terms of anchor i move by |term| (e_gz_i / |gz_i| + e_d / d) -- bounded here by the
    largest such factor over the anchors."""
    rel = 2 * U + r_gz(soft) + DIV_ULP * ULP + ref['terms'][:, None] * U
    e = ref['abs_df'] * rel
    if e_gz is not None:
        n = ref['gz'].size
        sel = np.asarray(sel).reshape(n, 2)
        worst = 0.0
        for i in range(n):
            for o in sel[i]:
                if o >= 0:
                    gzr = e_gz[i] / abs(ref['gz'][i]) if ref['gz'][i] != 0 else 0.0
                    worst = max(worst, gzr + e_dist[i, o] / dist[i, o])
        e = e + ref['abs_df'] * worst
    return SAFETY * (e + TINY)


def e_tri_z(full, e_dist):
    """end to end: z = fl(vp - fl(d_n + 1e5 [same])): the two distances' errors, the +1e5 rounding, the subtraction"""
    n = full['z'].size
    sel = full['sel'].reshape(n, 2)
    r = np.arange(n)
    e_p = np.where(sel[:, 0] >= 0, e_dist[r, np.maximum(sel[:, 0], 0)], 0.0)
    e_n = e_dist[r, sel[:, 1]] + np.where(full['same_n'], U * np.abs(full['vn']), 0.0)
    return e_p + e_n + U * np.abs(full['z'])


def tri_gap_ok(full, e_dist, margin32=None):
    """The condition under which the fp32 selection must equal the float64 one: for every anchor the float64 gap between the
    best and the second-best candidate exceeds twice the candidates' bound -- the distance bound, and for the negative (whose
    candidates are fl(d + 1e5 [same])) the rounding of that addition, u (d + 1e5), on top.  With a hinge the sign of
    z + margin must be as safe."""
    b = SAFETY * e_dist.max(1)
    bn = b + np.where(full['same_n'], SAFETY * U * (1e5 + full['dist'].max(1)), 0.0)
    ok = (full['gap_p'] > 2 * b).all() and (full['gap_n'] > 2 * bn).all()
    if margin32 is not None:
        ok = ok and (np.abs(full['z'] + float(margin32)) > 2 * SAFETY * e_tri_z(full, e_dist)).all()
    return bool(ok)


def e_softmax2(ref):
    """ta = fl(a - mx): u |ta|; ea = expf(ta): relative r_a = u |ta| + EXPF_ULP ulp; sum = fl(ea + eb); p = fl(eb / sum):
    relative r_b + (ea r_a + eb r_b) / (ea + eb) + u + DIV_ULP ulp; TINY: exp(-240) is 0 in fp32"""
    ra, rb = U * np.abs(ref['ta']) + EXPF_ULP * ULP, U * np.abs(ref['tb']) + EXPF_ULP * ULP
    mix = (ref['ea'] * ra + ref['eb'] * rb) / (ref['ea'] + ref['eb']) + U + DIV_ULP * ULP
    return dict(p=ref['p'] * (rb + mix) + TINY, p0=ref['p0'] * (ra + mix) + TINY)


def b_softmax2(ref):
    e = e_softmax2(ref)
    return dict(p=SAFETY * e['p'], p0=SAFETY * e['p0'])


def b_softmax2_bwd(ref, e_p=None, e_p0=None):
    """gp = fl(g p);  ds0 = fl(fl(0 - gp) p0): 2 u |ds0|;  ds1 = fl(fl(g - gp) p): p (u |gp| + u |g - gp|) + u |ds1|.
    End to end: ds0 moves by |g| (p0 e_p + p e_p0), ds1 by |g| |1 - 2 p| e_p."""
    g, p, p0, gp = np.abs(ref['g']), ref['p'], ref['p0'], np.abs(ref['gp'])
    e0 = 2 * U * np.abs(ref['ds'][:, 0]) + TINY
    e1 = p * (U * gp + U * np.abs(ref['g'] - ref['gp'])) + U * np.abs(ref['ds'][:, 1]) + TINY
    if e_p is not None:
        e0 = e0 + g * (p0 * e_p + p * e_p0)
        e1 = e1 + g * np.abs(1.0 - 2.0 * p) * e_p
    return SAFETY * np.stack([e0, e1], 1)


def k_pair_sum(n):
    """pair_bce_kernel: s(t) lane trips of 256 over n^2 + 6 shuffle levels + the 4 additions of block_sum"""
    return trips(n * n, 256) + 6 + 4


def b_pair_bce(ref, n):
    """term: y = 1: logf(s): LOGF_ULP ulp |log|;  y = 0: fl(1 - s) (relative u: u in the log) and logf; the clamp at -100 is
    1-Lipschitz; the products with y and 1 - y and the sum of the two are exact (one of them is 0).
    loss = fl(sum * fl(1 / n^2)): k_pair_sum u sum|term|, then DIV_ULP ulp + u relative.   prec = fl(hits * fl(1 / n^2)): the
    count is an exact integer.   dprob = fl(fl(fl(s - y) / max(fl(fl(1 - s) s), 1e-12f)) * inv): u + 2 u + u (the fp32 constant)
    + DIV_ULP ulp, + DIV_ULP ulp + u for inv and the product."""
    N = float(n * n)
    e_term = LOGF_ULP * ULP * np.abs(ref['log_used']) + np.where(ref['y'] > 0, 0.0, U)
    r_inv = DIV_ULP * ULP + U
    e_loss = (e_term.sum() + k_pair_sum(n) * U * np.abs(ref['term']).sum()) / N + abs(ref['loss']) * r_inv
    return dict(loss=SAFETY * e_loss, prec=SAFETY * ref['prec'] * r_inv,
                dprob=SAFETY * (np.abs(ref['dprob']) * (4 * U + DIV_ULP * ULP + r_inv) + TINY))


def b_scale_dev(ref):
    """a = fl(alpha g), y = fl(a x)"""
    return SAFETY * 2 * U * np.abs(ref['y'])


def b_oim_update(ref, D, momentum):
    """per replayed sample: r = fl(fl(row m) + fl(x fl(1 - m))): u (|row m| + 2 |x (1 - m)|) + u |r| and m times what the row
    carries from the replay before;  |r|^2: a block dot of r r (k_block_dot: stride 1024, + 4 for block_sum);
    inv = 1 / sqrtf (e_inv_norm);  row = fl(r inv).   Returns {row: per-element bound after the last replay}."""
    m = float(momentum)
    carried, out = {}, {}
    for st in ref['steps']:
        y, r = st['row'], st['r']
        x_term = np.abs(r - m * st['before'])
        e_r = m * carried.get(y, 0.0) + U * (np.abs(m * st['before']) + 2 * x_term) + U * np.abs(r)
        e_ss = (2 * np.abs(r) * e_r).sum() + k_block_dot(D) * U * st['ss']
        e_inv = e_inv_norm(st['ss'], e_ss)
        e_row = e_r / np.sqrt(st['ss']) + np.abs(r) * e_inv + U * np.abs(st['after'])
        carried[y] = e_row
        out[y] = SAFETY * e_row
    return out


# ----------------------------------------------------------------------------------------------------------------------
# fp32 restatements of the reductions, in the kernels' order (numpy, CPU): the bounds are satisfiable.  numpy's exp / log stand
# in for the device's expf / logf (they round differently: the CPU column of the table is not the device's).
def _block_sum_f32(per_thread):
    """[..., 256] per-thread partials -> wave_sum per wave, then block_sum's four sequential additions from 0"""
    red = _butterfly(per_thread.reshape(per_thread.shape[:-1] + (4, 64)))
    t = np.zeros(red.shape[:-1], F)
    for i in range(4):
        t = t + red[..., i]
    return t


def _strided_f32(v):
    """[..., W] -> [..., 256]: thread t adds v[t], v[t + 256], ... in sequence from 0"""
    W = v.shape[-1]
    pad = (-W) % 256
    p = np.concatenate([v, np.zeros(v.shape[:-1] + (pad,), F)], -1).reshape(v.shape[:-1] + (-1, 256))
    s = np.zeros(v.shape[:-1] + (256,), F)
    for t in range(p.shape[-2]):
        s = s + p[..., t, :]
    return s


def softmax_ce_f32(logits, ld, labels, weight, n, c):
    z = F(logits).reshape(n, ld)[:, :c]
    y = np.asarray(labels, np.int64)
    ok = (y >= 0) & (y < c)
    ys = np.where(ok, y, 0)
    w = np.ones(c, F) if weight is None else F(weight)
    wsum = F(0)
    for r in range(n):
        wsum = wsum + (w[ys[r]] if ok[r] else F(0))
    mx = z.max(1)
    t = z - mx[:, None]
    s = _block_sum_f32(_strided_f32(np.exp(t).astype(F)))
    lse = np.log(s).astype(F)
    gscale = np.where(ok, w[ys], F(0)) / wsum if wsum > 0 else np.zeros(n, F)
    rows = np.where(ok, gscale * (lse - t[np.arange(n), ys]), F(0)).astype(F)
    onehot = np.zeros((n, c), F)
    onehot[np.arange(n)[ok], ys[ok]] = 1
    dz = gscale[:, None] * (np.exp(t - lse[:, None]).astype(F) - onehot)
    loss = F(0)
    for r in range(n):
        loss = loss + rows[r]
    return dict(rows=rows, loss=loss, dz=dz.astype(F))


def oim_grad_f32(dl, ldd, lut, g, alpha, n, c, D):
    """the class loop as a chain of fused multiply-adds: the fp32 product is exact in float64, the float64 sum rounds to fp32"""
    d = F(dl).reshape(n, ldd)[:, :c].astype(np.float64)
    L = F(lut).reshape(c, D).astype(np.float64)
    acc = np.zeros((n, D), F)
    for j in range(c):
        acc = (d[:, j, None] * L[j][None, :] + acc.astype(np.float64)).astype(F)
    a = F(alpha) * (F(1) if g is None else F(g).reshape(-1)[0])
    return a * acc


def triplet_dist_f32(f, n, D):
    f = F(f).reshape(n, D)
    d = f[:, None, :] - f[None, :, :]
    sq = (d * d).reshape(n, n, -1, 4)
    q = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3]           # [n][n][D/4]
    pad = (-q.shape[-1]) % 64
    q = np.concatenate([q, np.zeros((n, n, pad), F)], -1).reshape(n, n, -1, 64)
    s = np.zeros((n, n, 64), F)
    for t in range(q.shape[2]):
        s = s + q[:, :, t]
    return np.sqrt(_butterfly(s) + F(1e-12))


def pair_bce_f32(prob, tp, tg, n):
    s = F(prob).reshape(-1)
    y = (np.asarray(tp)[None, :] == np.asarray(tg)[:, None]).reshape(-1)
    with np.errstate(divide='ignore'):
        ls = np.maximum(np.log(s).astype(F), F(-100))
        l1 = np.maximum(np.log(F(1) - s).astype(F), F(-100))
    term = -np.where(y, ls, l1)
    inv = F(1) / F(n * n)
    loss = _block_sum_f32(_strided_f32(term[None, :]))[0] * inv
    dprob = (s - y.astype(F)) / np.maximum((F(1) - s) * s, F(1e-12)) * inv
    return dict(loss=loss, dprob=dprob.reshape(n, n))


def oim_update_f32(lut, x, labels, D, num_classes, momentum):
    L, X, m = F(lut).reshape(num_classes, D).copy(), F(x).reshape(-1, D), F(momentum)
    for j, y in enumerate(labels):
        if 0 <= y < num_classes:
            r = L[y] * m + X[j] * (F(1) - m)
            inv = F(1) / np.sqrt(block_dot_f32(r[None, :], r[None, :]))[0]
            L[y] = r * inv
    return L
