"""The hybrid-memory cross entropy (grl_hybrid_ce, grl_amd/csrc/hybrid.hip) and the loss that carries it (HybridMemoryLoss,
grl_amd/reid/loss/hybrid_memory.py) restated in float64 (numpy only), with the sweep, the inputs and the first-order bounds --
shared by test_hybrid_cpu.py (no GPU) and test_gpu_hybrid.py.  The brute-force models of HybridLabels and of the self-paced
filter (which DO build n x n set matrices) are here too.

Written from the contract in include/grl_hip.h, not from the kernel body.  The conventions are loss_bounds' / cmem_ref's /
proxy_ref's: bounds are derived per element, none is fitted: depth of the fp32 chain x u x sum|terms| (u = 2^-24,
-ffp-contract=off: every * and + rounds once), errors of a stage that feed the next carried through the derivative, SAFETY (2)
once at the end.  EXPF_ULP, LOGF_ULP, DIV_ULP, TINY are loss_bounds' (assumed libm accuracies, not tuned).

Chains, for a valid row with target y over C classes:
  z_c = fl(S_c / |c|), S_c the members' logits added one by one: charged |c| additions on sum|logits of c| and one division
    (DIV_ULP ulp of |z_c|) -- e_z[c], to which the caller adds what the logits themselves carry (the mean of the members').
  From z on the chain is softmax_ce_kernel's over C columns (loss_bounds.b_softmax_ce): t_c = fl(z_c - mx): u |t_c|;
    e_c = expf(t_c): relative u |t_c| + EXPF_ULP ulp;  s = sum e_c: a lane's trips(C, 256) strided additions, the 6 levels of
    the xor tree, block_sum's 4 additions (loss_bounds.k_ce_rowsum(C));  lse = logf(s): e_s / s + LOGF_ULP ulp |lse|, absolute.
  L = fl(lse - fl(z_y - mx));  row = fl(inv L), inv = fl(1 / nv): DIV_ULP ulp (nv is a sum of ones: exact);  loss: n - 1 serial
    additions of the rows.
  p_c = expf(fl(t_c - lse)): relative u |t_c| + e_lse + u |t_c - lse| + EXPF_ULP ulp;  g_c = fl(fl(p_c - [c = y]) / |c|): one
    subtraction, DIV_ULP ulp;  dz_j = fl(inv g_c(j)).
  e_z reaches L and p through the derivatives: d L / d z_c = p_c - [c = y];  d p_c / d z_k = p_c ([c = k] - p_k).

The arg-max is a function of the z GIVEN: on fp32 z whose two largest values are closer than their errors the kernel's
class and the model's may differ.  `gap_ok`: the float64 gap between the largest z and every other z exceeds GAP_FACTOR x the
larger of the two classes' e_z (the two largest z decide it); test_hybrid_cpu.py asserts it for every case the GPU file compares `correct` on."""
import numpy as np

import loss_ref as LR
import cmem_ref as CM
from head_ref import flat, view
from bn_bounds import U, SAFETY, check, RATIOS, dump_ratios                                     # noqa: F401
from head_bounds import rng_for, f32, trips, EXPF_ULP, DIV_ULP, ULP                             # noqa: F401
from loss_bounds import unit_rows, k_ce_rowsum, LOGF_ULP, TINY, _block_sum_f32, _strided_f32    # noqa: F401
from cmem_ref import GAP_FACTOR

F = np.float32
MAX_CLASSES = 15360

# ----------------------------------------------------------------------------------------------------------------------
# the sweep
CE_N = (1, 2, 9, 33)
CE_COLS = (1, 3, 70, 257, 1025)     # one lane busy, under a wave, under a workgroup, one column past a trip, five trips
CE_LAYOUTS = ('identity', 'one', 'random', 'big')
CE_CASES = tuple((n, N) for n in CE_N for N in CE_COLS)
BIG = 300                           # members of the 'big' layout's class where N admits it (N >= 400): more than a trip of lanes
LOSS_N, LOSS_COLS, LOSS_D, LOSS_TEMP, LOSS_MOMENTUM = 9, 70, (256, 1028), 0.05, 0.2
LOSS_WIDE = 5200                    # memory rows past grl_oim_grad's 5120 columns: HybridMemoryLoss's blocked backward


def tables(inst_class):
    """(class_ptr [C + 1], class_members [N], inst_class [N]) int32 from the class of every column, the slow way"""
    ic = np.asarray(inst_class, np.int64)
    C = int(ic.max()) + 1
    members = [np.flatnonzero(ic == c).tolist() for c in range(C)]          # ascending
    assert all(members), 'an empty class'
    ptr = np.cumsum([0] + [len(m) for m in members])
    return ptr.astype(np.int32), np.array([j for m in members for j in m], np.int32), ic.astype(np.int32)


def layout(N, name, rng):
    """inst_class int64 [N].
    identity: column j is class j.            one: one class holds everything.
    random:   about N / 3 classes of random sizes, their members interleaved, the class numbering permuted.
    big:      one class of BIG random columns (N >= 400; half the columns below that) in the middle of the numbering, the
              other columns singletons in a permuted numbering."""
    if name == 'identity':
        return np.arange(N, dtype=np.int64)
    if name == 'one':
        return np.zeros(N, np.int64)
    if name == 'random':
        raw = rng.randint(0, max(1, N // 3), N)
        ids = np.unique(raw)
        return rng.permutation(ids.size)[np.searchsorted(ids, raw)].astype(np.int64)
    size = BIG if N >= 400 else (N + 1) // 2
    cols = rng.permutation(N)
    C = N - size + 1
    numbering = rng.permutation(C)
    ic = np.empty(N, np.int64)
    ic[cols[:size]] = numbering[C // 2]
    ic[cols[size:]] = np.delete(numbering, C // 2)
    return ic


def targets_for(n, ic, rng):
    """int64 [n]: the class of a random column (large classes are drawn more often), row 1 = -1 and row 3 = C -- just out of
    range on either side -- as far as n reaches"""
    y = ic[rng.randint(0, ic.size, n)].astype(np.int64)
    if n > 1:
        y[1] = -1
    if n > 3:
        y[3] = int(ic.max()) + 1
    return y


def in_ce(n, N, name, seed=0, wide=None):
    """logits 14 cos(.) in an ld-wide buffer whose columns past N hold values a kernel must not read (ld = N + 3 for odd n)"""
    r = rng_for('hybrid', n, N, name, seed)
    ic = layout(N, name, r)
    cp, cm, ic32 = tables(ic)
    wide = (n % 2 == 1) if wide is None else wide
    ld = N + 3 if wide else N
    buf = f32(np.full((n, ld), 1e30))
    buf[:, :N] = 14.0 * np.cos(r.uniform(0.0, 2.0 * np.pi, (n, N)))
    return dict(logits=buf.reshape(-1), ld=ld, ldd=N + 5 if wide else N, targets=targets_for(n, ic, r), cp=cp, cm=cm, ic=ic32,
                C=cp.size - 1)


def ce_seed(n, N, name):
    """the first seed whose rows all satisfy the arg-max gap condition (test_hybrid_cpu.py asserts one exists below 64)"""
    for seed in range(64):
        d = in_ce(n, N, name, seed)
        if gap_ok(hybrid_ce(d['logits'], d['ld'], d['targets'], d['cp'], d['cm'], d['ic'], n, N, d['C'])):
            return seed
    raise AssertionError('no seed below 64 satisfies the gap condition for n = %d, N = %d, %s' % (n, N, name))


TIE_COLS = 300


def in_ties():
    """Two rows over 300 columns at -5: classes 0 .. 3 are the pairs (0, 299), (1, 298), (2, 297), (3, 296), the rest
    singletons 4 .. 295 of the columns 4 .. 295.  Row 0: the classes 1 and 3 both have the mean 6 (as 5 + 7 and 4 + 8: exact in
    fp32) and the singleton class 200 holds 6 too -- three classes at the maximum, class 1 wins; target 1: a hit.  Row 1: the
    singleton classes 260 and 70 hold 9 and the pair class 2 has 9 as 9 + 9: class 2 wins; target 70: no hit."""
    N = TIE_COLS
    ic = np.arange(N, dtype=np.int64)
    ic[[299, 298, 297, 296]] = [0, 1, 2, 3]
    z = f32(np.full((2, N), -5.0))
    z[0, [1, 298]] = [5.0, 7.0]
    z[0, [3, 296]] = [4.0, 8.0]
    z[0, 200] = 6.0
    z[1, [260, 70]] = 9.0
    z[1, [2, 297]] = 9.0
    cp, cm, ic32 = tables(ic)
    return dict(logits=z.reshape(-1), ld=N, ldd=N, targets=np.array([1, 70], np.int64), cp=cp, cm=cm, ic=ic32, C=cp.size - 1,
                want_arg=[1, 2], want_correct=1.0)


def in_loss(D, seed=0, tag='loss', singletons=False, N=None):
    """n = 9 unit rows against a unit instance memory of 70 rows in the 'random' classes (``singletons``: identity classes);
    every row's index is a member of its target class; row 4 carries the target -1 (its index stays valid: the update is by
    index), row 7 the index -1 (its target stays valid)"""
    r = rng_for('hybrid', tag, D, seed)
    N = LOSS_COLS if N is None else N
    ic = layout(N, 'identity' if singletons else 'random', r)
    cp, cm, ic32 = tables(ic)
    index = r.randint(0, N, LOSS_N).astype(np.int64)
    y = ic[index].astype(np.int64)
    y[4] = -1
    index[7] = -1
    return dict(mem=unit_rows(r.standard_normal((N, D))), x=unit_rows(r.standard_normal((LOSS_N, D))), targets=y, index=index,
                cp=cp, cm=cm, ic=ic32, C=cp.size - 1)


def loss_seed(D, tag='loss'):
    for seed in range(64):
        d = in_loss(D, seed, tag)
        if gap_ok(loss(d, D)['ce'], e_in=e_logits(loss(d, D), D)):
            return seed
    raise AssertionError('no seed below 64 satisfies the gap condition for D = %d' % D)


# ----------------------------------------------------------------------------------------------------------------------
# the float64 model
def hybrid_ce(logits, ld, targets, cp, cm, ic, n, N, C):
    """grl_hybrid_ce of include/grl_hip.h -> valid, nv, z [n][C], L, rows (L_i / nv), loss, correct, arg, dz [n][N] and the
    intermediates the bounds are built from."""
    x = view(flat(logits), n, N, ld).astype(np.float64)
    y = np.asarray(targets, np.int64)[:n]
    cp, cm, ic = (np.asarray(a, np.int64) for a in (cp, cm, ic))
    size = np.diff(cp).astype(np.float64)
    z, abs_sum = np.zeros((n, C)), np.zeros((n, C))
    for c in range(C):
        mem = cm[cp[c]:cp[c + 1]]
        z[:, c] = x[:, mem].sum(1) / size[c]
        abs_sum[:, c] = np.abs(x[:, mem]).sum(1)
    valid = (y >= 0) & (y < C)
    ys = np.where(valid, y, 0)
    nv = int(valid.sum())
    mx = z.max(1)
    t = z - mx[:, None]
    e = np.exp(t)
    s = e.sum(1)
    lse = np.log(s)
    p = np.exp(t - lse[:, None])
    onehot = np.zeros((n, C))
    onehot[np.arange(n)[valid], ys[valid]] = 1.0
    ty = t[np.arange(n), ys]
    L = np.where(valid, lse - ty, 0.0)
    rows = L / nv if nv else np.zeros(n)
    arg = z.argmax(1)                                       # numpy: the first index at the maximum
    g = (p - onehot) / size[None, :] * valid[:, None]
    dz = g[:, ic] / nv if nv else np.zeros((n, N))
    return dict(valid=valid, nv=nv, z=z, abs_sum=abs_sum, size=size, t=t, e=e, s=s, lse=lse, p=p, onehot=onehot, ty=ty, L=L,
                rows=rows, loss=rows.sum(), arg=arg, correct=float((valid & (arg == ys)).sum()), g=g, dz=dz, ic=ic,
                cp=cp, cm=cm)


def loss(d, D, g=1.0, mem=None):
    """HybridMemoryLoss.forward and the gradient of its backward for the memory as given (``mem``: the memory the backward
    reads, default the forward's): logits = scalar x . mem^T with scalar = float32(1 / temp), hybrid_ce, dx = g scalar dz . mem."""
    n, N = LOSS_N, d['mem'].shape[0]
    X, M = view(flat(d['x']), n, D, D), view(flat(d['mem']), N, D, D)
    scalar = float(F(1.0 / LOSS_TEMP))
    logits = scalar * (X @ M.T)
    ce = hybrid_ce(logits.reshape(-1), N, d['targets'], d['cp'], d['cm'], d['ic'], n, N, d['C'])
    Mb = M if mem is None else view(flat(mem), N, D, D)
    og = LR.oim_grad(ce['dz'].reshape(-1), N, Mb, [g], scalar, n, N, D)
    return dict(logits=logits, abs_logits=scalar * (np.abs(X) @ np.abs(M).T), ce=ce, loss=ce['loss'], dz=ce['dz'], dx=og['dx'],
                og=og, scalar=scalar)


# ----------------------------------------------------------------------------------------------------------------------
# bounds.  e_* : first-order error, WITHOUT SAFETY (they compose);  b_* : what a test compares against (with SAFETY).
def e_class_logits(ref, e_in=None):
    """[n][C]: |c| additions on sum|members| and one division; ``e_in`` [n][N]: what the logits carry, through the mean"""
    e = ref['size'][None, :] * U * ref['abs_sum'] / ref['size'][None, :] + DIV_ULP * ULP * np.abs(ref['z'])
    if e_in is not None:
        for c in range(ref['z'].shape[1]):
            e[:, c] += e_in[:, ref['cm'][ref['cp'][c]:ref['cp'][c + 1]]].sum(1) / ref['size'][c]
    return e


def gap_ratios(ref, e_in=None):
    """per valid row of more than one class: the smallest, over the classes c other than the arg-max a, of (z_a - z_c) /
    max(e_z[a], e_z[c]) -- the two largest z are the pair that decides it unless a far larger class carries a far larger bound"""
    e_z, z = e_class_logits(ref, e_in), ref['z']
    out = []
    for i in np.flatnonzero(ref['valid']):
        a = int(ref['arg'][i])
        others = np.delete(np.arange(z.shape[1]), a)
        if others.size:
            out.append(float(((z[i, a] - z[i, others]) / np.maximum(e_z[i, a], e_z[i, others])).min()))
    return np.array(out)


def gap_ok(ref, e_in=None):
    """the condition under which the fp32 arg-max class must equal the float64 one: every ratio above GAP_FACTOR"""
    return bool(np.all(gap_ratios(ref, e_in) > GAP_FACTOR))


def b_hybrid_ce(ref, n, N, C, e_in=None):
    """-> dict(z [n][C], rows [n], loss, dz [n][N])"""
    nv, valid = ref['nv'], ref['valid']
    e_z = e_class_logits(ref, e_in)
    p, t, lse, size = ref['p'], ref['t'], ref['lse'], ref['size'][None, :]
    at = np.abs(t)
    e_s = (ref['e'] * (U * at + EXPF_ULP * ULP)).sum(1) + k_ce_rowsum(C) * U * ref['s'] + TINY
    e_lse = e_s / ref['s'] + LOGF_ULP * ULP * np.abs(lse)
    r_inv = DIV_ULP * ULP
    aty = np.abs(ref['ty'])
    pm = np.abs(p - ref['onehot'])
    e_L = e_lse + U * aty + U * (np.abs(lse) + aty) + (pm * e_z).sum(1)
    inv = 1.0 / nv if nv else 0.0
    e_rows = np.where(valid, e_L * inv + np.abs(ref['rows']) * (r_inv + U), 0.0)
    e_loss = e_rows.sum() + (n - 1) * U * np.abs(ref['rows']).sum()
    r_p = U * at + e_lse[:, None] + U * np.abs(t - lse[:, None]) + EXPF_ULP * ULP
    e_p = p * r_p + p * (e_z + (p * e_z).sum(1, keepdims=True))
    e_g = (e_p + U * pm + TINY) / size + np.abs(ref['g']) * DIV_ULP * ULP
    e_dz = np.where(valid[:, None], e_g[:, ref['ic']] * inv + np.abs(ref['dz']) * (r_inv + U), 0.0)
    return dict(z=SAFETY * e_z, rows=SAFETY * e_rows, loss=SAFETY * e_loss, dz=SAFETY * e_dz)


def e_logits(ref, D):
    """the fp32 GEMM with the scale in its epilogue: a sum of D products in some order and one more rounding (cmem_ref)"""
    return (D + 1) * U * ref['abs_logits']


def b_loss(ref, n, D, N, C):
    """end to end from the inputs: b_hybrid_ce with the logits' own error carried through the class means"""
    e_z = e_logits(ref, D)
    own = b_hybrid_ce(ref['ce'], n, N, C, e_in=e_z)
    return dict(logits=SAFETY * e_z, loss=own['loss'], dz=own['dz'])


b_dx = CM.b_dx


# ----------------------------------------------------------------------------------------------------------------------
# fp32 restatement of the kernel, in its summation order (numpy, CPU): the bounds are satisfiable.  numpy's exp / log stand in
# for the device's expf / logf.
def hybrid_ce_f32(logits, ld, targets, cp, cm, ic, n, N, C):
    x = F(logits).reshape(n, ld)[:, :N]
    y = np.asarray(targets, np.int64)
    valid = (y >= 0) & (y < C)
    ys = np.where(valid, y, 0)
    z = np.zeros((n, C), F)
    for c in range(C):
        mem = cm[cp[c]:cp[c + 1]]
        s = x[:, mem[0]].copy()
        for j in mem[1:]:
            s = s + x[:, j]
        z[:, c] = s / F(mem.size)
    mx = z.max(1)
    t = z - mx[:, None]
    s = _block_sum_f32(_strided_f32(np.exp(t).astype(F)))
    lse = np.log(s).astype(F)
    nv = F(valid.sum())
    inv = F(1) / nv if nv > 0 else F(0)
    L = (lse - t[np.arange(n), ys]).astype(F)
    rows = np.where(valid, inv * L, F(0)).astype(F)
    onehot = np.zeros((n, C), F)
    onehot[np.arange(n)[valid], ys[valid]] = 1
    g = ((np.exp(t - lse[:, None]).astype(F) - onehot) / np.diff(cp).astype(F)[None, :]).astype(F)
    dz = np.where(valid[:, None], inv * g[:, ic], F(0)).astype(F)
    total = F(0)
    for r in range(n):
        total = total + rows[r]
    return dict(z=z, rows=rows, loss=total, dz=dz, correct=float((valid & (z.argmax(1) == ys)).sum()))


# ----------------------------------------------------------------------------------------------------------------------
# HybridLabels and the self-paced filter on the host, the slow way
def hybrid_numbering(labels):
    """(sample_class, n_classes) as the contract of PseudoLabels.hybrid: clusters keep 0 .. K - 1 (compact ids), the noise
    samples become K, K + 1, .. in ascending sample index"""
    ids = sorted(set(int(l) for l in labels if l >= 0))
    out, nxt = [], len(ids)
    for l in labels:
        if l >= 0:
            out.append(ids.index(int(l)))
        else:
            out.append(nxt)
            nxt += 1
    return np.array(out, np.int64), nxt


def _same_set(labels):
    """bool [n][n]: i and j are in one set, a noise sample being a set of its own"""
    l = np.asarray(labels, np.int64)
    return ((l[:, None] == l[None, :]) & (l[:, None] >= 0)) | np.eye(l.size, dtype=bool)


def self_paced_brute(labels, tight, loose, tau=None):
    """the filter of pseudo.self_paced_filter from the n x n set matrices -> (labels int64 [n], tau)"""
    l = np.asarray(labels, np.int64)
    I, T, L = _same_set(l), _same_set(tight), _same_set(loose)
    r_indep = (I & L).sum(1) / (I | L).sum(1)
    r_comp = (I & T).sum(1) / (I | T).sum(1)
    ids = sorted(set(int(c) for c in l if c >= 0))
    indep = {c: max(r_indep[i] for i in range(l.size) if l[i] == c) for c in ids}
    comp = {c: max(r_comp[i] for i in range(l.size) if l[i] == c) for c in ids}
    if tau is None and ids:
        ranked = sorted(indep.values(), reverse=True)
        tau = ranked[min(len(ids) - 1, int(round(0.9 * len(ids))))]
    out = np.array([c if c >= 0 and indep[int(c)] >= tau and r_comp[i] >= comp[int(c)] else -1 for i, c in enumerate(l)], np.int64)
    return out, tau
