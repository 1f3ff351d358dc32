"""Shapes, inputs, first-order rounding-error bounds and an fp32 restatement of the summation order for the train-mode
BatchNorm kernels -- shared by test_bn_ref_cpu.py (no GPU) and test_gpu_bn_float64.py.

All bounds are derived, none is fitted: u = 2^-24 is the unit roundoff of fp32 (round to nearest; the library is built
with -ffp-contract=off, so every * and + rounds once), a sum whose every term passes through at most k additions is off
by at most k u sum|terms| (Higham, Accuracy and Stability of Numerical Algorithms, 4.2), an elementwise expression by
(number of roundings) u (sum of absolute terms).  SAFETY = 2 covers the dropped u^2 terms; it is the only factor."""
import numpy as np

import bn_ref as R

U = 2.0 ** -24
U64 = 2.0 ** -53
SAFETY = 2.0
CHUNK = 128                     # rows per fp32 partial of the column reductions (train.hip)

M_LIST = (1, 2, 3, 5, 7, 127, 128, 129, 130, 4 * 128 + 1)
C_LIST = (4, 12, 20, 60, 64, 68, 124, 128, 132, 252, 256, 260, 512)
# every M with three (or four) C, every C with three M, and the one larger case 513 x 260
SHAPES = (
    (1, 4), (1, 64), (1, 260), (1, 60),
    (2, 12), (2, 128), (2, 512), (2, 68),
    (3, 20), (3, 68), (3, 256), (3, 124),
    (5, 60), (5, 124), (5, 252), (5, 128),
    (7, 4), (7, 132), (7, 512), (7, 252), (7, 20),
    (127, 12), (127, 64), (127, 260), (127, 132),
    (128, 20), (128, 128), (128, 252),
    (129, 60), (129, 68), (129, 256), (129, 20),
    (130, 124), (130, 132), (130, 512),
    (513, 4), (513, 12), (513, 64), (513, 256), (513, 260),
)
CLASSES = ('a', 'b', 'c')


def grid_for(n, block=256):
    """train.hip's grid_for: ceil(n / 256) workgroups, at most 8192, made even when more than one."""
    g = (n + block - 1) // block
    g = 1 if g < 1 else min(g, 8192)
    return (g + 1) & ~1 if g > 1 else g


def apply_takes_fast_branch(M, C):
    """bn_apply_centered_kernel / bn_bwd_apply_kernel keep a thread's channel vectors in registers iff the launch's thread
    count is a multiple of the row's C/4 channel groups (`step % C4 == 0`)."""
    return (grid_for(M * C // 4) * 256) % (C // 4) == 0


def chunks(M):
    return (M + CHUNK - 1) // CHUNK


def chunk_sums(a):
    """[chunks][C] sums of a[M][C] over the kernels' 128-row chunks (float64)."""
    return np.add.reduceat(np.asarray(a, np.float64), np.arange(0, a.shape[0], CHUNK), axis=0)


# ------------------------------------------------------------------------------------------------------------------
# inputs
def make_inputs(M, C, cls, seed=0):
    """fp32 inputs of one case.  (a) well conditioned: per-channel mean in [-3, 3] std, std in [0.5, 2];
    (b) ill conditioned: per-channel mean ~ +-1e3, spread 1e-2 -- the regime the pivot exists for -- and channel 1
    exactly constant (1000.0: var = 0, invstd = 1 / sqrt(eps), y = beta); (c) as (a): the callers move half of the
    pre-activations to within a few ulp of zero once the statistics are known (near_zero_residual / near_zero_z)."""
    rng = np.random.RandomState(1000003 * M + 101 * C + ord(cls) + seed)
    if cls == 'b':
        mean = rng.choice([-1.0, 1.0], C) * 1e3 * rng.uniform(0.5, 1.5, C)
        z = mean[None, :] + 1e-2 * rng.standard_normal((M, C))
        z[:, 1] = 1000.0
    else:
        std = rng.uniform(0.5, 2.0, C)
        z = std[None, :] * (rng.standard_normal((M, C)) + rng.uniform(-3.0, 3.0, C)[None, :])
    d = dict(z=z.astype(np.float32), gamma=rng.uniform(0.5, 1.5, C).astype(np.float32),
             beta=rng.uniform(-0.7, 0.7, C).astype(np.float32), res=rng.standard_normal((M, C)).astype(np.float32),
             dy=rng.standard_normal((M, C)).astype(np.float32), gres0=rng.standard_normal((M, C)).astype(np.float32),
             rm=rng.standard_normal(C).astype(np.float32), rv=rng.uniform(0.5, 2.0, C).astype(np.float32),
             dgamma0=rng.standard_normal(C).astype(np.float32), dbeta0=rng.standard_normal(C).astype(np.float32))
    return d


def _near_zero_pick(shape, rng):
    return rng.random_sample(shape) < 0.5, rng.randint(-3, 4, shape)


def near_zero_residual(z, mean, scale, beta, res, seed=7):
    """Class (c) with a residual: for about half of the elements res := -fl32((z - mean) scale + beta) + j ulp, j in -3..3
    -- the pre-activation lands within a few ulp (of its largest term) of zero, on either side or on it."""
    rng = np.random.RandomState(seed + z.size)
    t = R.apply_centered(z, mean, scale, beta)
    pick, j = _near_zero_pick(z.shape, rng)
    r32 = (-t['pre']).astype(np.float32)
    r32 = (r32.astype(np.float64) + j * np.spacing(np.abs(r32)).astype(np.float64)).astype(np.float32)
    return np.where(pick, r32, np.asarray(res, np.float32)), pick


def near_zero_z(z, mean, scale, beta, seed=11):
    """Class (c) without a residual: about half of the elements of z move to fl32(mean - beta / scale) + j ulp, so that
    (z - mean) scale + beta is a few ulp of |beta| away from zero.  (The statistics vectors stay the ones given: the apply
    and backward stages take them as arguments.)"""
    rng = np.random.RandomState(seed + z.size)
    pick, j = _near_zero_pick(z.shape, rng)
    m, s, b = R.f64(mean), R.f64(scale), R.f64(beta)
    z0 = np.broadcast_to((m - b / s)[None, :], z.shape).astype(np.float32)
    z0 = (z0.astype(np.float64) + j * np.spacing(np.abs(z0)).astype(np.float64)).astype(np.float32)
    return np.where(pick, z0, np.asarray(z, np.float32)), pick


# ------------------------------------------------------------------------------------------------------------------
# summation depths, read from the kernel sources
# col_stats_kernel: a wave takes every 4th row of a 128-row chunk: 32 sequential additions per lane, then the four waves
# by a two-level tree through LDS.
K_COL_STATS = 32 + 2


def k_bwd_reduce(C):
    """bn_bwd_reduce_kernel<LPR>: a wave owns 32 rows of the chunk and reads 64 / LPR of them per instruction: a lane adds
    32 LPR / 64 terms in sequence, then log2(64 / LPR) xor-shuffle levels, then the two-level tree over the waves.
    LPR = 16 (C <= 64): 8 + 2 + 2; 32 (C <= 128): 16 + 1 + 2; 64: 32 + 0 + 2."""
    lpr = 16 if C <= 64 else 32 if C <= 128 else 64
    return 32 * lpr // 64 + {16: 2, 32: 1, 64: 0}[lpr] + 2


def lpr_bf16(C):
    """train_bf16.hip lpr_for: lanes per row (8 channels per lane), at most 32."""
    return min(32, C // 8)


def k_bf16_reduce(C):
    """col_stats_b16_kernel / bn_bwd_reduce_b16_kernel: 256 / LPR lane groups ("parts") take the chunk's rows round robin --
    ceil(128 / parts) sequential additions -- and part 0 then adds the other parts' partials one after the other:
    parts - 1 further additions on the same chain."""
    parts = 256 // lpr_bf16(C)
    return (CHUNK + parts - 1) // parts + parts - 1


# GEMM statistics epilogue (gemm_f32.hip): a tile has at most 128 rows; a lane adds at most 32 of them in sequence, the
# lanes / waves owning the same column combine in at most 2 further levels (shuffle + LDS, or LDS + LDS)
K_GEMM_STATS = 32 + 2


# ------------------------------------------------------------------------------------------------------------------
# bounds (per channel or per element; every one already carries SAFETY)
def b_col_sum(abs_d, result, k=K_COL_STATS):
    """sum of d = fl(x - pivot): the subtraction rounds once (u |d| per term), then k additions."""
    return SAFETY * ((k + 1) * U * abs_d + U * np.abs(result))


def b_col_sumsq(sq_d, result, k=K_COL_STATS):
    """sum of fl(d * d): d carries u, its square 2 u, the multiplication rounds once more (3 u d^2 per term), then k
    additions."""
    return SAFETY * ((k + 3) * U * sq_d + U * np.abs(result))


def b_slab_sum(total, result):
    """slab_sum_kernel adds in fp64, rounds the total to fp32 once (u |total|) and adds it to out (or to 0.f: exact)
    in fp32 (u |result|)."""
    return SAFETY * U * (np.abs(total) + np.abs(result))


def finalize_bounds(S, Q, count, pivot, gamma, beta, rm, rv, momentum, eps, prev_rm_bound=0.0, prev_rv_bound=0.0):
    """bn_stats_finalize_kernel from the float64 slab totals S, Q.  Its fp64 part (md = S / count,
    var = Q / count - md^2, mu = md + pivot) is charged 4 * 2^-53 (Q / count + md^2) on var and 2 * 2^-53 |mu| on mu.
    invstd = fl32(1 / sqrt(var + eps)): u |invstd| + |d invstd / d var| B_var, d invstd / d var = invstd^3 / 2.
    mean = fl32(mu): u |mu|.   scale = fl(g * invstd): |g| B_is + u |scale|.
    shift = fl(b - fl(fl(mean_f * g) * is_f)): mean_f carries u, two products round (3 u |mu g is|), is_f carries B_is,
    the subtraction rounds once (u (|b| + |mu g is|)).
    running = fl(fl(fl(1 - m) * r) + fl(m * fl32(stat))): fl(1 - m) and the product round (2 u |(1 - m) r|), the cast and
    the product round (2 u |m stat|), the sum rounds (u |result|); the previous call's bound enters times (1 - m); the
    variance's B_var enters times m count / (count - 1)."""
    md = S / count
    var = np.maximum(Q / count - md * md, 0.0)
    mu = md + (0.0 if pivot is None else R.f64(pivot))
    g = np.ones_like(mu) if gamma is None else R.f64(gamma)
    b = np.zeros_like(mu) if beta is None else R.f64(beta)
    ref = R.finalize(mu, var, count, gamma, beta, rm, rv, momentum, eps)
    is_ = ref['invstd']
    b_var = 4 * U64 * (Q / count + md * md)
    b_is = U * is_ + 0.5 * is_ ** 3 * b_var
    mgi = np.abs(mu * g * is_)
    out = dict(ref=ref, mu=mu, var=var,
               mean=SAFETY * (U * np.abs(mu) + 2 * U64 * np.abs(mu)),
               invstd=SAFETY * b_is,
               scale=SAFETY * (np.abs(g) * b_is + U * np.abs(ref['scale'])),
               shift=SAFETY * (np.abs(mu * g) * b_is + 3 * U * mgi + U * (np.abs(b) + mgi)))
    if rm is not None:
        m = float(momentum)
        unb = count / (count - 1.0) if count > 1 else 1.0
        out['running_mean'] = (1 - m) * prev_rm_bound + SAFETY * (
            2 * U * np.abs((1 - m) * R.f64(rm)) + 2 * U * np.abs(m * mu) + U * np.abs(ref['running_mean']))
        out['running_var'] = (1 - m) * prev_rv_bound + SAFETY * (
            2 * U * np.abs((1 - m) * R.f64(rv)) + 2 * U * np.abs(m * ref['unbiased']) + m * unb * b_var
            + U * np.abs(ref['running_var']))
    return out


def b_apply(abs_terms):
    """y = fl(fl(fl(fl(z - mean) * scale) + beta) + res): four roundings, each relative to a partial sum that is at most
    the sum of absolute terms |z - mean| |scale| + |beta| + |res|.  The ReLU is 1-Lipschitz: it cannot enlarge an error."""
    return SAFETY * 4 * U * abs_terms


def b_sum_g(abs_g_chunks, res_chunks, C):
    """sum g over the chunks: g = dy or 0 is exact, k additions per chunk, fp64 across chunks."""
    return SAFETY * (k_bwd_reduce(C) * U * abs_g_chunks.sum(0) + U * np.abs(res_chunks).sum(0))


def b_sum_gx(abs_gx_chunks, res_chunks, C):
    """sum g * xhat: xhat = fl(fl(z - mean) * invstd) and the product g * xhat: three roundings per term, then k
    additions."""
    return SAFETY * ((k_bwd_reduce(C) + 3) * U * abs_gx_chunks.sum(0) + U * np.abs(res_chunks).sum(0))


def b_accumulate(b_total, total, init):
    """dgamma / dbeta: fl(init + fl32(total)): the total's own bound, its cast (u |total|) and the addition (u |result|)."""
    return b_total + SAFETY * U * (np.abs(total) + np.abs(init + total))


def b_coef(b_total, total, M):
    """coef = fl32(total / M)."""
    return b_total / M + SAFETY * U * np.abs(total / M)


def b_dz(bw, b_k0, b_k1):
    """dz = fl(gm * fl(fl(g - k0) - fl(fl(fl(z - mean) * invstd) * k1))), gm = fl(invstd * gamma): the longest chain of
    roundings through the expression is 7 (z - mean, * invstd, * k1, g - k0, the second subtraction, gm, the last product),
    on terms of at most abs_terms; the reduced coefficients k0, k1 bring their own bounds, times |gm| and |gm xhat|."""
    gm = np.abs(bw['gm'])[None, :]
    return SAFETY * 7 * U * bw['abs_terms'] + gm * (b_k0[None, :] + np.abs(bw['xhat']) * b_k1[None, :])


def bf16_round(a):
    """float64 / fp32 -> nearest bf16 (ties to even), returned as float64."""
    a32 = np.asarray(a, np.float32)
    bits = a32.view(np.uint32).astype(np.uint64)
    bits = ((bits + 0x7fff + ((bits >> 16) & 1)) >> 16) << 16
    return bits.astype(np.uint32).view(np.float32).astype(np.float64)


def bf16_ulp(a):
    """spacing of bf16 (8 significand bits) at |a|; the smallest normal's spacing below it."""
    a = np.maximum(np.abs(np.asarray(a, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 7)


# ------------------------------------------------------------------------------------------------------------------
# fp32 restatement of the kernels' summation order (numpy, CPU): the bounds and inputs are satisfiable
def _tree4(p):
    return (p[0] + p[1]) + (p[2] + p[3])


def col_stats_f32(x, pivot=None):
    """col_stats_kernel: slab[chunk][0|1][C] in fp32."""
    x = np.asarray(x, np.float32)
    M, C = x.shape
    pv = np.zeros(C, np.float32) if pivot is None else np.asarray(pivot, np.float32)
    slab = np.zeros((chunks(M), 2, C), np.float32)
    for ch in range(chunks(M)):
        r0, r1 = ch * CHUNK, min(M, (ch + 1) * CHUNK)
        s = np.zeros((4, C), np.float32); q = np.zeros((4, C), np.float32)
        for w in range(4):
            for r in range(r0 + w, r1, 4):
                v = x[r] - pv
                s[w] += v; q[w] += v * v
        slab[ch, 0], slab[ch, 1] = _tree4(s), _tree4(q)
    return slab


def bwd_reduce_f32(dy, z, mask, mean, invstd):
    """bn_bwd_reduce_kernel<LPR>: slab[chunk][0|1][C] in fp32 (sum g, sum g * xhat)."""
    dy, z = np.asarray(dy, np.float32), np.asarray(z, np.float32)
    M, C = z.shape
    lpr = 16 if C <= 64 else 32 if C <= 128 else 64
    rpw = 64 // lpr
    mu, is_ = np.asarray(mean, np.float32), np.asarray(invstd, np.float32)
    g_all = dy if mask is None else np.where(mask, dy, np.float32(0))
    slab = np.zeros((chunks(M), 2, C), np.float32)
    for ch in range(chunks(M)):
        r1 = min(M, (ch + 1) * CHUNK)
        ws = np.zeros((4, C), np.float32); wq = np.zeros((4, C), np.float32)
        for w in range(4):
            s = np.zeros((rpw, C), np.float32); q = np.zeros((rpw, C), np.float32)
            rend = min(r1, ch * CHUNK + (w + 1) * 32)
            for sub in range(rpw):
                for r in range(ch * CHUNK + w * 32 + sub, rend, rpw):
                    xh = (z[r] - mu) * is_
                    s[sub] += g_all[r]; q[sub] += g_all[r] * xh
            o = 1
            while o < rpw:                              # xor-shuffle levels: lane group i += lane group i ^ o
                s = s + s[np.arange(rpw) ^ o]; q = q + q[np.arange(rpw) ^ o]
                o <<= 1
            ws[w], wq[w] = s[0], q[0]
        slab[ch, 0], slab[ch, 1] = _tree4(ws), _tree4(wq)
    return slab


def apply_f32(z, mean, scale, beta, res, relu):
    v = (np.asarray(z, np.float32) - np.asarray(mean, np.float32)) * np.asarray(scale, np.float32)
    if beta is not None:
        v = v + np.asarray(beta, np.float32)
    if res is not None:
        v = v + np.asarray(res, np.float32)
    return np.maximum(v, np.float32(0)) if relu else v


def finalize_f32(S, Q, count, pivot, gamma, beta, rm, rv, momentum, eps):
    """bn_stats_finalize_kernel: fp64 from the slab totals, fp32 where the kernel is."""
    f = np.float32
    md = S / count
    var = np.maximum(Q / count - md * md, 0.0)
    mu = md + (0.0 if pivot is None else R.f64(pivot))
    is_ = (1.0 / np.sqrt(var + float(f(eps)))).astype(f)
    g = np.ones_like(is_) if gamma is None else np.asarray(gamma, f)
    b = np.zeros_like(is_) if beta is None else np.asarray(beta, f)
    out = dict(mean=mu.astype(f), invstd=is_, scale=g * is_, shift=b - mu.astype(f) * g * is_)
    if rm is not None:
        unb = var * count / (count - 1.0) if count > 1 else var
        m = f(momentum)
        out['running_mean'] = (f(1) - m) * np.asarray(rm, f) + m * mu.astype(f)
        out['running_var'] = (f(1) - m) * np.asarray(rv, f) + m * unb.astype(f)
    return out


def bwd_apply_f32(dy, z, mask, mean, invstd, gamma, k0, k1):
    f = np.float32
    g = np.asarray(dy, f) if mask is None else np.where(mask, np.asarray(dy, f), f(0))
    zc = np.asarray(z, f) - np.asarray(mean, f)
    is_ = np.asarray(invstd, f)
    gm = is_ if gamma is None else is_ * np.asarray(gamma, f)
    return gm * (g - np.asarray(k0, f) - (zc * is_) * np.asarray(k1, f))


# ------------------------------------------------------------------------------------------------------------------
# comparison: per element / per channel against that element's or channel's bound -- never a norm over the tensor
RATIOS = {}                     # stage -> largest observed |error| / bound (EXPERIMENTS.md records them)


def check(stage, got, ref, bound, what=''):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
    assert got.shape == ref.shape, (stage, what, got.shape, ref.shape)
    assert np.isfinite(got).all(), (stage, what, 'non-finite output')
    err = np.abs(got - ref)
    ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    RATIOS[stage] = max(RATIOS.get(stage, 0.0), worst)
    if worst > 1.0:
        i = np.unravel_index(int(ratio.argmax()), ratio.shape)
        raise AssertionError('%s %s: |error| / bound = %.3g at %s (got %r, reference %r, bound %.3g); %d of %d over' % (
            stage, what, worst, i, got[i], ref[i], bound[i], int((ratio > 1).sum()), ratio.size))
    return worst


def dump_ratios(title):
    """the table EXPERIMENTS.md records (shown with pytest -s)"""
    print('\n%s: largest |error| / bound per stage' % title)
    for k in sorted(RATIOS):
        print('  %-28s %.3f' % (k, RATIOS[k]))
