"""The camera-aware proxy cross entropy (grl_proxy_ce, grl_amd/csrc/proxy.hip) and the loss that carries it (ProxyMemoryLoss,
grl_amd/reid/loss/proxy_memory.py) restated in float64 (numpy only), with the sweep, the inputs and the first-order bounds --
shared by test_proxy_cpu.py (no GPU) and test_gpu_proxy.py.

Written from the contract in include/grl_hip.h, not from the kernel body.  The conventions are loss_bounds' / cmem_ref's:
bounds are derived per element, none is fitted: depth of the fp32 chain read from the kernel x u x sum|terms| (u = 2^-24,
-ffp-contract=off: every * and + rounds once), errors of a stage that feed the next carried through the derivative, SAFETY (2)
once at the end.  EXPF_ULP, LOGF_ULP, DIV_ULP, TINY are loss_bounds' (assumed libm accuracies, not tuned).

The selection is a function of the values GIVEN: the model sorts the logits it receives (value descending, index ascending;
-0 == +0), whatever their dtype.  On the kernel sweep it receives the kernel's own fp32 logits and the selection must be
EQUAL; behind the GEMM of ProxyMemoryLoss it receives float64 logits, and the comparison holds under the gap condition
(`gap_ok`) that test_proxy_cpu.py asserts for every such case.

Chains read from proxy.hip, for a set S of columns (A_i or U_i) with maximum mx (exact):
  t_j = fl(z_j - mx): u |t_j|;  e_j = expf(t_j): relative u |t_j| + EXPF_ULP ulp;  s = sum e_j: a lane's trips(P, 256) strided
    additions, the 6 levels of the xor tree, block_sum's 4 additions (loss_bounds.k_ce_rowsum(P));  lse = logf(s): e_s / s +
    LOGF_ULP ulp |lse|, absolute.
  intra = fl(lseA - fl(z_own - mxA)).
  sP = sum over Pos of fl(z_j - mxU), the same tree; ipos = fl(1 / |Pos|): DIV_ULP ulp; mean = fl(sP ipos);
    inter = fl(lseU - mean).
  L = fl(fl(w_intra intra) + fl(w_inter inter));  row = fl(inv L), inv = fl(1 / nv): DIV_ULP ulp;  loss: n - 1 serial
    additions of the rows.
  p_j = expf(fl(t_j - lse)): relative u |t_j| + e_lse + u |t_j - lse| + EXPF_ULP ulp;  ga = fl(w_intra fl(pA - [own])),
    gu = fl(w_inter fl(pU - [Pos] ipos)), dz = fl(inv fl(ga + gu))."""
import numpy as np

import loss_ref as LR
import cmem_ref as CM
from head_ref import flat, view
from bn_bounds import U, SAFETY, check, RATIOS, dump_ratios                                     # noqa: F401
from head_bounds import rng_for, f32, trips, EXPF_ULP, DIV_ULP, ULP                             # noqa: F401
from loss_bounds import unit_rows, k_ce_rowsum, LOGF_ULP, TINY, b_oim_grad                      # noqa: F401
from cmem_ref import GAP_FACTOR

F = np.float32
MAX_P = 8192

# ----------------------------------------------------------------------------------------------------------------------
# the sweep
CE_N = (1, 2, 9, 33)
CE_P = (1, 3, 70, 257, 1025)    # one lane busy, under a wave, under a workgroup, one column past a trip, five trips
CE_K = (0, 1, 3, 50)            # clamped to P
CE_CAMS = (1, 2, 6)
CE_WEIGHTS = ((1.0, 0.5), (1.0, 0.0), (0.0, 1.0))
CE_TABLES = ('spread', 'mixed', 'one')
CE_CASES = tuple((n, P) for n in CE_N for P in CE_P)
LOSS_N, LOSS_D, LOSS_TEMP, LOSS_MOMENTUM, LOSS_CAMS = 9, 256, 0.05, 0.2, 3
# (P, k_neg, mode): P = 3 admits every negative; P = 70 cuts among 64 or more
LOSS_CASES = ((3, 3, 'instance'), (70, 1, 'hard'), (70, 3, 'instance'), (70, 3, 'hard'), (70, 50, 'mean'))
LOSS_W = (1.0, 0.5)


def table(P, C, pattern, rng):
    """(proxy_cluster, proxy_cam) int32 [P].
    spread: proxy j = (j // C, j % C), ascending as PseudoLabels.proxies numbers them; the last cluster may miss cameras.
    mixed:  cluster 0 lives in camera 0 only; camera C - 1 holds ONE proxy, (1, C - 1) (C >= 2); the other clusters take random
            non-empty subsets of the cameras 0 .. max(C - 2, 0); the table is shuffled (the contract asks for no order).
    one:    every proxy belongs to cluster 0, camera j % C: no negatives, and pairs that occur more than once."""
    if pattern == 'spread':
        j = np.arange(P)
        return (j // C).astype(np.int32), (j % C).astype(np.int32)
    if pattern == 'one':
        return np.zeros(P, np.int32), (np.arange(P) % C).astype(np.int32)
    pairs = [(0, 0)]
    if C >= 2:
        pairs += [(1, 0), (1, C - 1)]
    cl = 2
    while len(pairs) < P:
        cams = np.flatnonzero(rng.randint(0, 2, max(C - 1, 1)))
        if cams.size == 0:
            cams = np.array([rng.randint(max(C - 1, 1))])
        pairs += [(cl, int(c)) for c in cams]
        cl += 1
    pairs = np.array(pairs[:P], np.int32)[rng.permutation(P)]
    return np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])


def missing_pair(pcl, pcm, C):
    """a (cluster, camera) pair without a proxy whose cluster exists: a camera < C if there is one, else camera C"""
    have = set(zip(pcl.tolist(), pcm.tolist()))
    for cl in sorted(set(pcl.tolist())):
        for cam in range(C):
            if (cl, cam) not in have:
                return cl, cam
    return int(pcl[0]), C


def rows_for(n, pcl, pcm, C, pattern, rng):
    """(labels, cams) int64 [n]: every row the pair of a random proxy, then row 1 = the noise label -1, row 3 = a pair
    without a proxy, and on the mixed table row 2 = (1, C - 1) (the camera whose only proxy is the row's own) and row 4 =
    (0, 0) (the cluster that lives in one camera) -- as far as n reaches."""
    j = rng.randint(0, pcl.size, n)
    y, cam = pcl[j].astype(np.int64), pcm[j].astype(np.int64)
    if n > 1:
        y[1] = -1
    if n > 3:
        y[3], cam[3] = missing_pair(pcl, pcm, C)
    if pattern == 'mixed' and C >= 2 and pcl.size >= 3:
        if n > 2:
            y[2], cam[2] = 1, C - 1
        if n > 4:
            y[4], cam[4] = 0, 0
    return y, cam


def in_ce(n, P, C, pattern, wide=None, seed=0):
    """logits 14 cos(.) in an ld-wide buffer whose columns past P hold values a kernel must not read (ld = P + 3 for odd n)"""
    r = rng_for('proxy', n, P, C, pattern, seed)
    pcl, pcm = table(P, C, pattern, r)
    y, cam = rows_for(n, pcl, pcm, C, pattern, r)
    wide = (n % 2 == 1) if wide is None else wide
    ld = P + 3 if wide else P
    buf = f32(np.full((n, ld), 1e30))
    buf[:, :P] = 14.0 * np.cos(r.uniform(0.0, 2.0 * np.pi, (n, P)))
    return dict(logits=buf.reshape(-1), ld=ld, ldd=P + 5 if wide else P, labels=y, cams=cam, pcl=pcl, pcm=pcm)


TIE_P, TIE_K = 300, 6


def in_ties():
    """One valid row of cluster 0 (own proxy 0, one camera) against 299 proxies of other clusters at -5, with planted values.
    Descending: 9 (j = 280 and 17: a pair wholly inside), 7 (j = 5), then 3 at j = 290, 40, 260, 41, 100 -- five copies for the
    three places left: the lowest indices 40, 41, 100 win -- and 1 (j = 50 and 270: a pair wholly outside).  The second row is
    the same with +0.0 / -0.0 as the duplicated value (they compare equal): -0.0 at 40 and 100, +0.0 at 41, 260, 290."""
    z = f32(np.full((2, TIE_P), -5.0))
    for row, (v, w) in enumerate(((3.0, 3.0), (0.0, -0.0))):
        z[row, 0] = 2.0
        z[row, [280, 17]] = 9.0
        z[row, 5] = 7.0
        z[row, [41, 260, 290]] = v
        z[row, [40, 100]] = w
        z[row, [50, 270]] = -1.0 if row else 1.0
    pcl = np.arange(TIE_P).astype(np.int32)
    return dict(logits=z.reshape(-1), ld=TIE_P, ldd=TIE_P, labels=np.zeros(2, np.int64), cams=np.zeros(2, np.int64), pcl=pcl,
                pcm=np.zeros(TIE_P, np.int32), want=[5, 17, 40, 41, 100, 280])


def loss_table(P):
    pcl, pcm = table(P, LOSS_CAMS, 'spread', None)
    if P == 3:
        pcl, pcm = np.array([0, 0, 1], np.int32), np.array([0, 1, 0], np.int32)
    return pcl, pcm


def in_loss(P, k, seed=0, tag='loss'):
    """n = 9 unit rows against a unit memory of P proxies over 3 cameras; row 4 carries the noise label, row 7 a pair without a
    proxy"""
    r = rng_for('proxy', tag, P, LOSS_CAMS, seed)
    pcl, pcm = loss_table(P)
    j = r.randint(0, P, LOSS_N)
    y, cam = pcl[j].astype(np.int64), pcm[j].astype(np.int64)
    y[4] = -1
    y[7], cam[7] = missing_pair(pcl, pcm, LOSS_CAMS)
    return dict(mem=unit_rows(r.standard_normal((P, LOSS_D))), x=unit_rows(r.standard_normal((LOSS_N, LOSS_D))), labels=y,
                cams=cam, pcl=pcl, pcm=pcm)


def loss_seed(P, k, tag='loss'):
    """the first seed whose float64 selection has, in every row, a gap above GAP_FACTOR x the bound of one logit
    (test_proxy_cpu.py asserts that one exists below 64 and that the case then has no exclusion)"""
    for seed in range(64):
        d = in_loss(P, k, seed, tag)
        if gap_ok(loss(d, P, k, LOSS_W), LOSS_D):
            return seed
    raise AssertionError('no seed below 64 satisfies the gap condition for P = %d, k = %d' % (P, k))


# ----------------------------------------------------------------------------------------------------------------------
# the float64 model
def proxy_ce(logits, ld, labels, cams, pcl, pcm, n, P, k_neg, w_intra, w_inter):
    """grl_proxy_ce of include/grl_hip.h -> own [n], negsel [n][k_neg], valid, rows (L_i / nv), loss, correct, dz [n][P] and
    per valid row the sets and intermediates the bounds are built from (``r``)."""
    z = view(flat(logits), n, P, ld).astype(np.float64)
    y, cam = np.asarray(labels, np.int64)[:n], np.asarray(cams, np.int64)[:n]
    pcl, pcm = np.asarray(pcl, np.int64)[:P], np.asarray(pcm, np.int64)[:P]
    wa, wu = float(F(w_intra)), float(F(w_inter))
    own = np.full(n, -1, np.int64)
    negsel = np.full((n, k_neg), -1, np.int32)
    dz, L, hit = np.zeros((n, P)), np.zeros(n), np.zeros(n)
    recs = {}
    for i in range(n):
        mine = np.flatnonzero((pcl == y[i]) & (pcm == cam[i]))
        if mine.size == 0:
            continue
        own[i] = mine[0]
        A, Pos = pcm == cam[i], pcl == y[i]
        N = np.flatnonzero(~Pos)
        order = N[np.lexsort((N, -z[i, N]))]                # value descending, then index ascending (-0 == +0)
        k = min(k_neg, N.size)
        neg = np.sort(order[:k])
        negsel[i, :k] = neg
        gap = float(z[i, order[k - 1]] - z[i, order[k]]) if 0 < k < N.size else np.inf
        Um = Pos.copy()
        Um[neg] = True
        rec = dict(A=A, Pos=Pos, U=Um, npos=int(Pos.sum()), gap=gap, N=N)
        for name, S in (('A', A), ('U', Um)):
            mx = z[i, S].max()
            t = np.where(S, z[i] - mx, -np.inf)
            e = np.exp(t)
            s = e.sum()
            lse = np.log(s)
            rec.update({'t' + name: t, 'e' + name: e, 's' + name: s, 'lse' + name: lse, 'p' + name: np.exp(t - lse), 'mx' + name: mx})
        rec['intra'] = rec['lseA'] - rec['tA'][own[i]]
        rec['mean'] = rec['tU'][Pos].sum() / rec['npos']
        rec['inter'] = rec['lseU'] - rec['mean']
        rec['ga'] = wa * (rec['pA'] - (np.arange(P) == own[i]))  * A
        rec['gu'] = wu * (rec['pU'] - Pos / rec['npos']) * Um
        L[i] = wa * rec['intra'] + wu * rec['inter']
        hit[i] = float(pcl[int(np.argmax(z[i]))] == y[i])   # numpy: the first index at the maximum
        recs[i] = rec
    valid = own >= 0
    nv = int(valid.sum())
    rows = L / nv if nv else np.zeros(n)
    for i, rec in recs.items():
        dz[i] = (rec['ga'] + rec['gu']) / nv
    return dict(own=own, negsel=negsel, valid=valid, nv=nv, L=L, rows=rows, loss=rows.sum(), correct=float(hit.sum()), dz=dz,
                r=recs, wa=wa, wu=wu, z=z)


def loss(d, P, k, w, g=1.0, mem=None):
    """ProxyMemoryLoss.forward and the gradient of its backward for the memory as given (``mem``: the memory the backward
    reads, default the forward's): logits = scalar x . mem^T with scalar = float32(1 / temp), proxy_ce, dx = g scalar dz . mem."""
    n, D = LOSS_N, LOSS_D
    X, M = view(flat(d['x']), n, D, D), view(flat(d['mem']), P, D, D)
    scalar = float(F(1.0 / LOSS_TEMP))
    logits = scalar * (X @ M.T)
    ce = proxy_ce(logits.reshape(-1), P, d['labels'], d['cams'], d['pcl'], d['pcm'], n, P, min(k, P), w[0], w[1])
    Mb = M if mem is None else view(flat(mem), P, D, D)
    og = LR.oim_grad(ce['dz'].reshape(-1), P, Mb, [g], scalar, n, P, D)
    return dict(logits=logits, abs_logits=scalar * (np.abs(X) @ np.abs(M).T), ce=ce, loss=ce['loss'], dz=ce['dz'], dx=og['dx'],
                og=og, scalar=scalar)


# ----------------------------------------------------------------------------------------------------------------------
# bounds.  e_* : first-order error, WITHOUT SAFETY (they compose);  b_* : what a test compares against (with SAFETY).
def _e_lse(rec, name, P):
    S = rec[name]
    at = np.where(S, np.abs(rec['t' + name]), 0.0)
    e_s = (rec['e' + name] * (U * at + EXPF_ULP * ULP)).sum() + k_ce_rowsum(P) * U * rec['s' + name] + TINY
    return e_s / rec['s' + name] + LOGF_ULP * ULP * abs(rec['lse' + name]), at


def b_proxy_ce(ref, n, P):
    """-> dict(loss, rows [n], dz [n][P]) for exact logits"""
    nv, wa, wu = ref['nv'], abs(ref['wa']), abs(ref['wu'])
    e_rows, e_dz = np.zeros(n), np.zeros((n, P))
    r_inv = DIV_ULP * ULP
    for i, rec in ref['r'].items():
        own, Pos, npos = int(ref['own'][i]), rec['Pos'], rec['npos']
        e_lA, atA = _e_lse(rec, 'A', P)
        e_lU, atU = _e_lse(rec, 'U', P)
        e_intra = e_lA + U * atA[own] + U * (abs(rec['lseA']) + atA[own])
        e_sP = U * atU[Pos].sum() + k_ce_rowsum(P) * U * atU[Pos].sum()
        e_mean = e_sP / npos + abs(rec['mean']) * (DIV_ULP * ULP + U)
        e_inter = e_lU + e_mean + U * (abs(rec['lseU']) + abs(rec['mean']))
        ta, tu = wa * abs(rec['intra']), wu * abs(rec['inter'])
        e_L = wa * e_intra + wu * e_inter + 2 * U * (ta + tu)
        e_rows[i] = e_L / nv + abs(ref['rows'][i]) * (r_inv + U)
        r_pA = U * atA + e_lA + U * np.where(rec['A'], np.abs(rec['tA'] - rec['lseA']), 0.0) + EXPF_ULP * ULP
        r_pU = U * atU + e_lU + U * np.where(rec['U'], np.abs(rec['tU'] - rec['lseU']), 0.0) + EXPF_ULP * ULP
        onehot = (np.arange(P) == own).astype(np.float64)
        e_ga = rec['A'] * (wa * (rec['pA'] * r_pA + U * np.abs(rec['pA'] - onehot) + TINY) + U * np.abs(rec['ga']))
        e_gu = rec['U'] * (wu * (rec['pU'] * r_pU + Pos * (DIV_ULP * ULP / npos) + U * np.abs(rec['pU'] - Pos / npos) + TINY)
                           + U * np.abs(rec['gu']))
        e_g = e_ga + e_gu + U * (np.abs(rec['ga']) + np.abs(rec['gu']))
        e_dz[i] = e_g / nv + np.abs(ref['dz'][i]) * (r_inv + U)
    e_loss = e_rows.sum() + (n - 1) * U * np.abs(ref['rows']).sum()
    return dict(rows=SAFETY * e_rows, loss=SAFETY * e_loss, dz=SAFETY * e_dz)


def e_logits(ref, D):
    """the fp32 GEMM with the scale in its epilogue: a sum of D products in some order and one more rounding (cmem_ref)"""
    return (D + 1) * U * ref['abs_logits']


def gaps(ref, D):
    """per valid row with a cut inside N_i: (float64 gap between the last admitted and the first refused negative, the bound of
    one logit of that row's N_i -- its largest)"""
    e_z = e_logits(ref, D)
    return [(rec['gap'], float(e_z[i, rec['N']].max())) for i, rec in sorted(ref['ce']['r'].items()) if np.isfinite(rec['gap'])]


def gap_ok(ref, D):
    return all(gap > GAP_FACTOR * bound for gap, bound in gaps(ref, D))


def b_loss(ref, n, D, P):
    """end to end from the inputs, the selection being the float64 one (gap_ok): the cross entropy's own bound on exact logits
    plus the logits' error through the derivatives: d loss / d z_ij = dz_ij;  d dz_ij / d z_ik = (1 / nv) (w_intra [j, k in A]
    pA_j ([j = k] - pA_k) + w_inter [j, k in U] pU_j ([j = k] - pU_k))."""
    ce, e_z = ref['ce'], e_logits(ref, D)
    own = b_proxy_ce(ce, n, P)
    e_loss = (np.abs(ce['dz']) * e_z).sum()
    e_dz = np.zeros((n, P))
    for i, rec in ce['r'].items():
        for name, w in (('A', abs(ce['wa'])), ('U', abs(ce['wu']))):
            S, p = rec[name], rec['p' + name]
            e_dz[i] += w * S * p * (e_z[i] + (S * p * e_z[i]).sum()) / ce['nv']
    return dict(logits=SAFETY * e_z, loss=own['loss'] + SAFETY * e_loss, dz=own['dz'] + SAFETY * e_dz)


b_dx = CM.b_dx


# ----------------------------------------------------------------------------------------------------------------------
# PseudoLabels.proxies on the host
def proxy_numbering(labels, cams):
    """(proxy_cluster, proxy_cam, sample_proxy) as the contract of PseudoLabels.proxies, the slow way"""
    pairs = sorted(set((int(l), int(c)) for l, c in zip(labels, cams) if l >= 0))
    index = {p: j for j, p in enumerate(pairs)}
    sp = np.array([index[(int(l), int(c))] if l >= 0 else -1 for l, c in zip(labels, cams)], np.int64)
    return np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32), sp
