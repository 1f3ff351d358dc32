"""The cluster-memory update (grl_cmem_update, grl_amd/csrc/cmem.hip) and the loss that carries it (ClusterMemoryLoss,
grl_amd/reid/loss/cluster_memory.py) restated in float64 (numpy only), with the sweep, the inputs, the first-order bounds
and an fp32 restatement of the kernel's summation order -- shared by test_cmem_cpu.py (no GPU) and test_gpu_cmem.py.

Written from the contract in include/grl_hip.h, not from the kernel body.  The conventions are loss_ref's / loss_bounds':
bounds are derived per element, none is fitted: depth of the fp32 chain read from the kernel x u x sum|terms| (u = 2^-24,
-ffp-contract=off: every * and + rounds once), errors of a stage that feed the next carried through the derivative, SAFETY
(2: the dropped u^2 terms) once at the end.  U, SAFETY, check, dump_ratios are bn_bounds' own; k_block_dot, e_inv_norm,
block_dot_f32, rng_for are head_bounds'; b_softmax_ce, b_oim_grad, unit_rows are loss_bounds'.

The ABI carries the momentum as fp32: the model blends with m = float(float32(momentum)) (0.2 is no fp32 number), and the
kernel's fl(1 - m) is one of the roundings the bound counts.

Depths read from cmem.hip:
  a member's similarity s_j and the blended row's sum of squares: the f32x4 strided trip (stride 1024 floats), dot4, the
    xor tree of wave_sum, block_sum's four additions: head_bounds.k_block_dot(D) = 1 + 3 + trips(D, 1024) + 6 + 4.
  the mean: v = fl(fl(x_j0 + x_j1 + ..) / (float)count): the members are added one after the other from 0 (the first addition
    is exact), count - 1 roundings on the element's sum of absolute terms, then one division (DIV_ULP ulp).
  the blend r = fl(fl(row m) + fl(v fl(1 - m))) and row = fl(r inv), inv = 1 / sqrtf(ss): as oim_update_kernel
    (loss_bounds.b_oim_update), one replay.
The logits of the loss come from the fp32 GEMM with the scale in its epilogue: a sum of D products in SOME order, every
term passes through at most D roundings, and one more for the scale: (D + 1) u sum|terms| (the rule of dgrad_bounds.py)."""
import numpy as np

import loss_ref as LR
from head_ref import flat, view
from bn_bounds import U, SAFETY, check, RATIOS, dump_ratios                                        # noqa: F401
from head_bounds import rng_for, f32, k_block_dot, e_inv_norm, block_dot_f32, DIV_ULP, ULP         # noqa: F401
from loss_bounds import unit_rows, b_softmax_ce, b_oim_grad                                        # noqa: F401

F = np.float32
HARD, MEAN = 0, 1
MODES = (HARD, MEAN)
GAP_FACTOR = 4.0                # the selection-gap condition: gap > 4 x the bound of one similarity

# ----------------------------------------------------------------------------------------------------------------------
# the sweep
UPD_N = (1, 2, 9, 33)
UPD_D = (4, 252, 256, 260, 1024, 1028, 2052) # stride 1024: lanes with no trip, one, two, three; D / 4 not a multiple of 64
UPD_K = (1, 3, 70)
UPD_PATTERNS = ('equal', 'distinct', 'pairs', 'mixed')
UPD_MOMENTA = (0.2, 0.0)
UPD_CASES = tuple((n, D) for n in UPD_N for D in UPD_D)
LOSS_N, LOSS_D, LOSS_K, LOSS_TEMP, LOSS_MOMENTUM = 9, 256, (3, 70), 0.05, 0.2
SEED = 0
TIE_D = (256, 2052)


def labels_for(n, K, pattern, rng=None):
    """equal: one cluster takes the batch; distinct: 0, 1, .. (those >= K fall outside the memory); pairs: (i // 2) mod K --
    with a small K a cluster's members are not adjacent; mixed: random valid labels with -1 first and K last."""
    i = np.arange(n, dtype=np.int64)
    if pattern == 'equal':
        return np.full(n, K // 2, np.int64)
    if pattern == 'distinct':
        return i
    if pattern == 'pairs':
        return (i // 2) % K
    y = rng.randint(0, K, n).astype(np.int64)
    y[0] = -1
    if n > 1:
        y[n - 1] = K
    return y


def in_update(n, D, K, pattern, seed=SEED):
    """unit-norm memory rows and samples, seeded by the case (the momentum and the mode take the same inputs)"""
    r = rng_for('cmem', n, D, K, pattern, seed)
    return dict(cent=unit_rows(r.standard_normal((K, D))), x=unit_rows(r.standard_normal((n, D))),
                labels=labels_for(n, K, pattern, r))


def in_tie(D, K=3, seed=SEED):
    """six samples of cluster 1 (and one of cluster 0 between them); samples 2 and 5 are the same bits, the row's negative:
    the least similar member twice -- the first index has to win.  Sample 4 is a duplicate of sample 0 (a tie that is not
    the minimum)."""
    r = rng_for('cmem tie', D, K, seed)
    cent = unit_rows(r.standard_normal((K, D)))
    x = unit_rows(r.standard_normal((7, D)))
    x[2] = -cent[1]
    x[5] = x[2]
    x[4] = x[0]
    return dict(cent=cent, x=x, labels=np.array([1, 1, 1, 0, 1, 1, 1], np.int64), first=2, second=5)


def in_loss(K, seed=SEED, tag='loss'):
    """n = 9 unit rows against a unit memory; row 4 carries the noise label -1"""
    r = rng_for('cmem', tag, K, seed)
    y = r.randint(0, K, LOSS_N).astype(np.int64)
    y[4] = -1
    return dict(cent=unit_rows(r.standard_normal((K, LOSS_D))), x=unit_rows(r.standard_normal((LOSS_N, LOSS_D))), labels=y)


PLANT_IDS, PLANT_PER, PLANT_D, PLANT_OUTLIERS = 6, 10, 64, 3
PLANT_COSINE = dict(eps=-0.7, min_samples=4)                # cosin_dist = -dot: within an identity < -0.85, across > -0.38
PLANT_JACCARD = dict(eps=0.5, min_samples=4, k1=9, k2=1)    # k1 = the identity's other rows; no expansion over the neighbours


def planted(seed=0):
    """(unit rows [63, 64], pids): 6 identities x 10 rows around a direction on the sphere (spread 0.3 of the unit noise) and
    3 far outliers (random directions, pids 100 ..), shuffled"""
    g = np.random.Generator(np.random.PCG64(seed))
    c = g.standard_normal((PLANT_IDS, PLANT_D))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    pids = np.repeat(np.arange(PLANT_IDS), PLANT_PER)
    x = c[pids] + 0.3 * g.standard_normal((pids.size, PLANT_D)) / np.sqrt(PLANT_D)
    x = np.concatenate((x, g.standard_normal((PLANT_OUTLIERS, PLANT_D))))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    pids = np.concatenate((pids, 100 + np.arange(PLANT_OUTLIERS)))
    order = g.permutation(pids.size)
    return x[order].astype(np.float32), pids[order]


def hard_cases():
    """every (inputs, n, D, K) the GPU file launches in hard mode with a float64 selection to compare with: the sweep, the
    loss cases and the two uses of the twice-in-one-graph case"""
    for n, D in UPD_CASES:
        for K in UPD_K:
            for pattern in UPD_PATTERNS:
                yield ('update', n, D, K, pattern), in_update(n, D, K, pattern), n, D, K
    for K in LOSS_K:
        yield ('loss', K), in_loss(K), LOSS_N, LOSS_D, K
        yield ('loss twice', K), in_loss(K, tag='second'), LOSS_N, LOSS_D, K


# ----------------------------------------------------------------------------------------------------------------------
# the float64 model
def m32(momentum):
    return float(F(momentum))


def pick_least(s):
    """strict < against a running best that starts at the first member: the first member wins ties, a NaN never replaces"""
    best, pick = s[0], 0
    for j in range(1, len(s)):
        if s[j] < best:
            best, pick = s[j], j
    return pick


def cmem_update(cent, x, labels, n, D, K, momentum, mode):
    """-> dict(cent [K][D], sel int32 [n], steps).  One step per label present, in the order of the labels' first rows:
    row, members, s and abs_s (hard: the similarities and their sums of absolute terms), gap (hard: second smallest s minus the
    smallest; inf with one member), pick (hard), count, v, abs_sum (mean: the element-wise sum of |x_j|), before, r, ss, after."""
    C = view(flat(cent).copy(), K, D, D)
    X = view(flat(x), n, D, D)
    y = np.asarray(labels, np.int64).reshape(-1)[:n]
    m = m32(momentum)
    sel = np.zeros(n, np.int32)
    steps, seen = [], set()
    for i in range(n):
        lab = int(y[i])
        if lab < 0 or lab >= K or lab in seen:
            continue
        seen.add(lab)
        mem = np.flatnonzero(y == lab)
        before = C[lab].copy()
        st = dict(row=lab, members=mem, count=mem.size, before=before)
        if mode == HARD:
            s = (X[mem] * before[None, :]).sum(1)          # (row by row: bit-identical rows give bit-identical sums; BLAS need not)
            pick = pick_least(s)
            srt = np.sort(s)
            st.update(s=s, abs_s=np.abs(X[mem]) @ np.abs(before), pick=int(mem[pick]),
                      gap=float(srt[1] - srt[0]) if mem.size > 1 else np.inf)
            v = X[mem[pick]].copy()
            sel[mem[pick]] = 1
        else:
            v = X[mem].sum(0) / mem.size
            st.update(abs_sum=np.abs(X[mem]).sum(0))
            sel[mem] = 1
        r = m * before + (1.0 - m) * v
        ss = (r * r).sum()
        C[lab] = r / np.sqrt(ss)
        st.update(v=v, r=r, ss=ss, after=C[lab].copy())
        steps.append(st)
    return dict(cent=C, sel=sel, steps=steps)


def loss(x, cent, labels, n, D, K, temp, g=1.0):
    """ClusterMemoryLoss.forward and the gradient of its backward, for the memory as given: logits = scalar x . cent^T with
    scalar = float32(1 / temp), F.cross_entropy (labels outside [0, K) ignored) and dx = g scalar dlogits . cent."""
    X, C = view(flat(x), n, D, D), view(flat(cent), K, D, D)
    scalar = float(F(1.0 / temp))
    logits = scalar * (X @ C.T)
    ce = LR.softmax_ce(logits.reshape(-1), K, labels, None, n, K)
    og = LR.oim_grad(ce['dz_val'].reshape(-1), K, C, [g], scalar, n, K, D)
    return dict(logits=logits, abs_logits=scalar * (np.abs(X) @ np.abs(C).T), ce=ce, loss=ce['loss'], dz=ce['dz_val'],
                dx=og['dx'], og=og, scalar=scalar)


# ----------------------------------------------------------------------------------------------------------------------
# bounds.  e_* : first-order error, WITHOUT SAFETY (they compose);  b_* : what a test compares against (with SAFETY).
def e_similarity(st, D):
    """one similarity of the hard selection: k_block_dot(D) u sum|terms|"""
    return k_block_dot(D) * U * st['abs_s']


def gap_ok(ref, D):
    """The condition under which the fp32 selection must equal the float64 one: in every cluster the float64 gap between the
    smallest and the second smallest similarity exceeds GAP_FACTOR x the largest bound of one similarity of that cluster."""
    return all(st['gap'] > GAP_FACTOR * float(e_similarity(st, D).max()) for st in ref['steps'])


def e_row(st, D, momentum, mode, e_before=0.0):
    """the blended, renormalised row of one step (loss_bounds.b_oim_update, one replay): e_before is what the row carried
    into the launch"""
    m = m32(momentum)
    r = st['r']
    if mode == HARD:
        e_v = 0.0                                         # a copy of one sample
    else:
        e_v = (st['count'] - 1) * U * st['abs_sum'] / st['count'] + DIV_ULP * ULP * np.abs(st['v'])
    e_r = m * e_before + (1.0 - m) * e_v + U * (np.abs(m * st['before']) + 2 * np.abs((1.0 - m) * st['v'])) + U * np.abs(r)
    e_ss = (2 * np.abs(r) * e_r).sum() + k_block_dot(D) * U * st['ss']
    return e_r / np.sqrt(st['ss']) + np.abs(r) * e_inv_norm(st['ss'], e_ss) + U * np.abs(st['after'])


def b_cmem_update(ref, D, momentum, mode):
    """{row: per-element bound} of the rows the launch writes"""
    return {st['row']: SAFETY * e_row(st, D, momentum, mode) for st in ref['steps']}


def b_unit_norm2(D):
    """|sum row^2 - 1| of a row the launch wrote: the fp32 sum of squares is k_block_dot(D) u relative (its terms are all
    positive), sqrtf halves that and adds SQRT_ULP ulp, the division DIV_ULP ulp, the product r inv one rounding per element;
    the square doubles the relative error of the norm"""
    from head_bounds import SQRT_ULP
    return SAFETY * 2 * (k_block_dot(D) * U / 2 + (SQRT_ULP + DIV_ULP) * ULP + U)


def e_logits(ref, D):
    return (D + 1) * U * ref['abs_logits']


def b_loss(ref, n, D, K):
    """end to end from the inputs: the cross entropy's own bound on exact logits (loss_bounds.b_softmax_ce) plus the logits'
    error through the derivatives: d loss / d z_ij = gs_i (p_ij - onehot_ij); d dz_ij / d z_ik = gs_i p_ij ([j = k] - p_ik);
    dx = a dz . cent: its own chain (loss_bounds.b_oim_grad) plus a e_dz . |cent|."""
    ce, e_z = ref['ce'], e_logits(ref, D)
    own = b_softmax_ce(ce, n, K)
    gs, p = ce['gscale'][:, None], ce['p']
    e_loss = (gs * np.abs(p - ce['onehot']) * e_z).sum()
    e_dz = gs * p * (e_z + (p * e_z).sum(1, keepdims=True))
    return dict(logits=SAFETY * e_z, loss=own['loss'] + SAFETY * e_loss, dz=own['dz'] + SAFETY * e_dz)


def b_dx(og, K, b_dz, cent):
    """dx = a dz . cent from a dz that is off by b_dz (SAFETY already in it) and the memory the backward read, taken as given"""
    return b_oim_grad(og, K) + abs(og['a']) * (b_dz @ np.abs(np.asarray(cent, np.float64)))


# ----------------------------------------------------------------------------------------------------------------------
# fp32 restatement of the kernel, in its summation order (numpy, CPU): the bounds are satisfiable
def cmem_update_f32(cent, x, labels, n, D, K, momentum, mode):
    C, X, m = F(cent).reshape(K, D).copy(), F(x).reshape(n, D), F(momentum)
    y = np.asarray(labels, np.int64).reshape(-1)[:n]
    sel = np.zeros(n, np.int32)
    seen = set()
    for i in range(n):
        lab = int(y[i])
        if lab < 0 or lab >= K or lab in seen:
            continue
        seen.add(lab)
        mem = np.flatnonzero(y == lab)
        if mode == HARD:
            s = block_dot_f32(X[mem], np.broadcast_to(C[lab], (mem.size, D)))
            j = mem[pick_least(s)]
            v = X[j]
            sel[j] = 1
        else:
            v = np.zeros(D, F)
            for j in mem:
                v = v + X[j]
            v = v / F(mem.size)
            sel[mem] = 1
        r = C[lab] * m + v * (F(1) - m)
        inv = F(1) / np.sqrt(block_dot_f32(r[None, :], r[None, :]))[0]
        C[lab] = r * inv
    return dict(cent=C, sel=sel)
