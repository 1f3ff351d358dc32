"""Float64 models, fp32 restatements, inputs and per-element error bounds of the two soft memory cross entropies --
grl_soft_hybrid_ce (grl_amd/csrc/soft_hybrid.hip) and grl_soft_proxy_ce (grl_amd/csrc/soft_proxy.hip) -- and of the losses that
carry them (SoftHybridMemoryLoss, SoftProxyMemoryLoss); shared by test_soft_memory_cpu.py (no GPU) and test_gpu_soft_memory.py.
The hard parts -- class tables, proxy tables, the selection, the student's chain -- are hybrid_ref's and proxy_ref's; the soft
target's chain is teacher_ref.b_soft_ce's, restated here per SET of columns so that it serves the classes of the hybrid memory
and the two sets of the proxy memory alike.

Written from the contracts in include/grl_hip.h.  Bounds are derived per element, none is fitted: the fp32 chain x u x |terms|
(u = 2^-24, -ffp-contract=off: every * and + rounds once), the errors of a stage carried into the next through the derivative,
SAFETY (2) once at the end.  EXPF_ULP, LOGF_ULP, DIV_ULP, TINY are loss_bounds' (assumed libm accuracies, not tuned).

The chain of one set S of columns (``e_soft_set``), student values z, teacher values tz, hard target h (sums to 1 over S: a
one-hot, or [Pos] / |Pos|), w handed over as an fp32 value (exact), omw = fl(1 - w): u |omw|:
  t_j = fl(z_j - mx): u |t_j| (mx exact);  e_j = expf(t_j): relative u |t_j| + EXPF_ULP ulp;  s = sum_S e_j: k_ce_rowsum(width) u s;
  lse = logf(s): e_s / s + LOGF_ULP ulp |lse|, absolute.  The teacher's the same: e_lt.
  q_j = expf(fl(fl(tz_j - mt) - lt)): relative r_q = u |tt_j| + e_lt + u |tt_j - lt| + EXPF_ULP ulp;  e_q = q r_q + TINY
  X = sum_S fl(q_j t_j): per term |t_j| e_q + q_j u |t_j| + u |q_j t_j|, the sum k_ce_rowsum(width) u sum |q t|
  H = the hard term on the shifted logits (t_own, or the mean over Pos), its own error e_H given by the caller
  L = fl(fl(lse - fl(omw H)) - fl(w X)): e_lse + omw e_H + 2 u omw |H| + u |lse - omw H| + w e_X + u w |X| + u |L|
  p_j = expf(fl(t_j - lse)): relative u |t_j| + e_lse + u |t_j - lse| + EXPF_ULP ulp;  e_p = p r_p + TINY
  g_j = fl(fl(p_j - fl(omw h_j)) - fl(w q_j)): e_p + omw h_j (2 u + r_h) + u |p - omw h| + w e_q + u w q + u |g|,
        r_h the relative error of h_j itself (0 for a one-hot, DIV_ULP ulp for fl(1 / |Pos|))."""
import numpy as np

import hybrid_ref as HR
import proxy_ref as PR
import loss_ref as LR
from head_ref import flat, view
from bn_bounds import U, SAFETY, check, RATIOS, dump_ratios                                     # noqa: F401
from head_bounds import rng_for, f32, EXPF_ULP, DIV_ULP, ULP                                    # noqa: F401
from loss_bounds import k_ce_rowsum, LOGF_ULP, TINY, _block_sum_f32, _strided_f32, unit_rows    # noqa: F401

F = np.float32
W_SWEEP = (0.0, 0.5, 1.0)
MAG = 14.0                          # |logits| of the kernel sweeps, as hybrid_ref.in_ce / proxy_ref.in_ce

# ----------------------------------------------------------------------------------------------------------------------
# the sweeps
HY_N = (1, 5)
HY_COLS = (1, 7, 300, 1030)         # one lane busy, under a wave, past the 256-lane stride, past 1024 (ce_finish's column block)
HY_LAYOUTS = ('identity', 'big', 'random')      # all singletons; one class of > 64 members beside singletons; interleaved members
HY_CASES = tuple((n, N) for n in HY_N for N in HY_COLS)
PX_N = (1, 5)
PX_P = (1, 5, 257, 1100)
PX_K = (0, 1, 50, 'P')
PX_WEIGHTS = ((1.0, 0.5), (1.0, 0.0), (0.0, 1.0))
PX_CASES = tuple((n, P) for n in PX_N for P in PX_P)
LOSS_W = 0.5


def teacher_like(z, rng, mag=MAG):
    """a teacher that mostly agrees: the student's values + 0.2 mag N(0, 1), clipped to the same range"""
    return f32(np.clip(np.asarray(z, np.float64) + 0.2 * mag * rng.standard_normal(np.shape(z)), -mag, mag))


def in_hybrid(n, N, name, seed=0):
    """hybrid_ref.in_ce's logits, tables and targets (row 1 = -1 and row 3 = C where n reaches) with BIG = 300 members in the
    'big' class where N >= 400 and (N + 1) // 2 below (N = 300: 150 members, more than a wave), always in wide buffers:
    ld = N + 3, ldt = N + 6, ldd = N + 5, 1e30 in the gaps."""
    d = HR.in_ce(n, N, name, seed, wide=True)
    r = rng_for('soft-hybrid', n, N, name, seed)
    ldt = N + 6
    tb = f32(np.full((n, ldt), 1e30))
    tb[:, :N] = teacher_like(d['logits'].reshape(n, d['ld'])[:, :N], r)
    return dict(d, tlogits=tb.reshape(-1), ldt=ldt)


def hy_seed(n, N, name):
    """the first seed whose student rows all satisfy hybrid_ref's arg-max gap condition"""
    for seed in range(64):
        d = in_hybrid(n, N, name, seed)
        if HR.gap_ok(HR.hybrid_ce(d['logits'], d['ld'], d['targets'], d['cp'], d['cm'], d['ic'], n, N, d['C'])):
            return seed
    raise AssertionError('no seed below 64 satisfies the gap condition for n = %d, N = %d, %s' % (n, N, name))


def in_proxy(n, P, C, pattern, seed=0, ties=False):
    """proxy_ref.in_ce's logits, tables and rows in wide buffers (ld = P + 3, ldt = P + 6, ldd = P + 5).  ``ties``: the values
    are rounded to multiples of 2, so that many columns are tied across any selection threshold (index order decides)."""
    d = PR.in_ce(n, P, C, pattern, wide=True, seed=seed)
    r = rng_for('soft-proxy', n, P, C, pattern, seed)
    if ties:
        z = d['logits'].reshape(n, d['ld'])
        z[:, :P] = 2.0 * np.round(z[:, :P] / 2.0)
    ldt = P + 6
    tb = f32(np.full((n, ldt), 1e30))
    tb[:, :P] = teacher_like(d['logits'].reshape(n, d['ld'])[:, :P], r)
    return dict(d, tlogits=tb.reshape(-1), ldt=ldt)


# ----------------------------------------------------------------------------------------------------------------------
# one set of columns: float64 model and first-order error
def soft_set(z, tz, S, h, w, omw):
    """z, tz [W] float64, S bool [W] (non-empty), h [W] the hard target (0 outside S, sums to 1).  Values outside S are 0."""
    mx = z[S].max()
    t = np.where(S, z - mx, 0.0)
    e = np.where(S, np.exp(t), 0.0)
    s = e.sum()
    lse = np.log(s)
    p = np.where(S, np.exp(t - lse), 0.0)
    H = float((h * t).sum())
    rec = dict(S=S, h=h, mx=mx, t=t, e=e, s=s, lse=lse, p=p, H=H)
    if w != 0.0:
        mt = tz[S].max()
        tt = np.where(S, tz - mt, 0.0)
        et = np.where(S, np.exp(tt), 0.0)
        st = et.sum()
        lt = np.log(st)
        q = np.where(S, np.exp(tt - lt), 0.0)
    else:
        tt = et = q = np.zeros_like(t)
        st, lt = 1.0, 0.0
    X = float((q * t).sum())
    L = lse - omw * H - w * X
    rec.update(tt=tt, et=et, st=st, lt=lt, q=q, X=X, absX=float((q * np.abs(t)).sum()), L=L, g=np.where(S, p - omw * h - w * q, 0.0))
    return rec


def e_soft_set(rec, width, w, omw, e_H, r_h):
    """-> (e_L, e_g [W], e_lse, e_lt) of one set, WITHOUT SAFETY; the chain of the module docstring"""
    S, t, tt = rec['S'], rec['t'], rec['tt']
    at, att = np.abs(t), np.abs(tt)
    k = k_ce_rowsum(width)
    e_s = (rec['e'] * (U * at + EXPF_ULP * ULP)).sum() + k * U * rec['s'] + TINY
    e_lse = e_s / rec['s'] + LOGF_ULP * ULP * abs(rec['lse'])
    if w != 0.0:
        e_st = (rec['et'] * (U * att + EXPF_ULP * ULP)).sum() + k * U * rec['st'] + TINY
        e_lt = e_st / rec['st'] + LOGF_ULP * ULP * abs(rec['lt'])
        r_q = U * att + e_lt + U * np.abs(tt - rec['lt']) + EXPF_ULP * ULP
        e_q = np.where(S, rec['q'] * r_q + TINY, 0.0)
    else:
        e_lt, e_q = 0.0, np.zeros_like(t)
    e_X = (at * e_q + 2 * U * rec['q'] * at).sum() + k * U * rec['absX']
    H = rec['H']
    e_L = (e_lse + omw * e_H + 2 * U * omw * abs(H) + U * abs(rec['lse'] - omw * H) + w * e_X + U * w * abs(rec['X'])
           + U * abs(rec['L']))
    r_p = U * at + e_lse + U * np.abs(t - rec['lse']) + EXPF_ULP * ULP
    e_p = rec['p'] * r_p + TINY
    h = rec['h']
    e_g = np.where(S, e_p + omw * h * (2 * U + r_h) + U * np.abs(rec['p'] - omw * h) + w * e_q + U * w * rec['q'] + U * np.abs(rec['g']),
                   0.0)
    return e_L, e_g, e_lse, e_lt


# ----------------------------------------------------------------------------------------------------------------------
# grl_soft_hybrid_ce
def class_means(x, cp, cm, C):
    n = x.shape[0]
    z, abs_sum = np.zeros((n, C)), np.zeros((n, C))
    for c in range(C):
        mem = cm[cp[c]:cp[c + 1]]
        z[:, c] = x[:, mem].sum(1) / float(mem.size)
        abs_sum[:, c] = np.abs(x[:, mem]).sum(1)
    return z, abs_sum


def soft_hybrid_ce(logits, ld, tlogits, ldt, targets, cp, cm, ic, w, n, N, C):
    """grl_soft_hybrid_ce of include/grl_hip.h in float64 on the inputs given.  ``hard``: hybrid_ref.hybrid_ce of the student
    (valid, nv, z, the tables, arg, correct); ``r``: per valid row the set record over the C classes; L, rows, loss, g [n][C]
    (the class gradients, divided by |c|), dz [n][N].  tlogits may be None when w = 0."""
    hard = HR.hybrid_ce(logits, ld, targets, cp, cm, ic, n, N, C)
    w = float(F(w))
    omw = 1.0 - w
    cp64, cm64 = hard['cp'], hard['cm']
    if w != 0.0:
        tz, tabs = class_means(view(flat(tlogits), n, N, ldt).astype(np.float64), cp64, cm64, C)
    else:
        tz, tabs = np.zeros((n, C)), np.zeros((n, C))
    y = np.asarray(targets, np.int64)[:n]
    nv = hard['nv']
    inv = 1.0 / nv if nv else 0.0
    every = np.ones(C, bool)
    recs, L, g = {}, np.zeros(n), np.zeros((n, C))
    for i in np.flatnonzero(hard['valid']):
        h = (np.arange(C) == y[i]).astype(np.float64)
        rec = soft_set(hard['z'][i], tz[i], every, h, w, omw)
        recs[int(i)] = rec
        L[i] = rec['L']
        g[i] = rec['g'] / hard['size']
    rows = inv * L
    return dict(hard=hard, r=recs, w=w, omw=omw, tz=tz, tabs=tabs, L=L, rows=rows, loss=rows.sum(), g=g, dz=inv * g[:, hard['ic']],
                nv=nv, inv=inv, valid=hard['valid'], correct=hard['correct'])


def e_teacher_classes(ref, e_in=None):
    """hybrid_ref.e_class_logits for the teacher's class logits"""
    hard = ref['hard']
    return HR.e_class_logits(dict(hard, z=ref['tz'], abs_sum=ref['tabs']), e_in)


def b_soft_hybrid_ce(ref, n, N, C, e_in=None, e_tin=None):
    """-> dict(rows [n], loss, dz [n][N]).  Per valid row: the set chain over the C classes (H = t_y: u |t_y|, a one-hot), plus
    what the class logits themselves carry (hybrid_ref.e_class_logits; ``e_in`` / ``e_tin``: the errors of the logits given,
    through the class means) through the derivatives
      d L / d z_c = g_c,   d L / d tz_c = -w q_c (t_c - X),
      d g_c / d z_k = p_c ([c = k] - p_k),   d g_c / d tz_k = -w q_c ([c = k] - q_k);
    then gc = fl(g_c / |c|): DIV_ULP ulp;  row = fl(inv L), dz = fl(inv gc), inv = fl(1 / nv): DIV_ULP ulp;  loss: n - 1 serial
    additions.  Invalid rows are exact zeros (bound 0)."""
    hard, w, omw, inv = ref['hard'], ref['w'], ref['omw'], ref['inv']
    e_z = HR.e_class_logits(hard, e_in)
    e_tz = e_teacher_classes(ref, e_tin) if w != 0.0 else np.zeros_like(e_z)
    size = hard['size']
    r_inv = DIV_ULP * ULP
    e_rows, e_dz = np.zeros(n), np.zeros((n, N))
    for i, rec in ref['r'].items():
        e_L, e_g, _, _ = e_soft_set(rec, C, w, omw, U * abs(rec['H']), 0.0)
        p, q, t = rec['p'], rec['q'], rec['t']
        e_L = e_L + (np.abs(rec['g']) * e_z[i]).sum() + w * (q * np.abs(t - rec['X']) * e_tz[i]).sum()
        e_g = e_g + p * (e_z[i] + (p * e_z[i]).sum()) + w * q * (e_tz[i] + (q * e_tz[i]).sum())
        e_gc = e_g / size + np.abs(ref['g'][i]) * DIV_ULP * ULP
        e_rows[i] = inv * e_L + abs(ref['rows'][i]) * (r_inv + U)
        e_dz[i] = inv * e_gc[hard['ic']] + np.abs(ref['dz'][i]) * (r_inv + U) + TINY
    e_loss = e_rows.sum() + (n - 1) * U * np.abs(ref['rows']).sum()
    return dict(rows=SAFETY * e_rows, loss=SAFETY * e_loss, dz=SAFETY * e_dz)


def soft_hybrid_ce_f32(logits, ld, tlogits, ldt, targets, cp, cm, ic, w, n, N, C):
    """fp32 restatement in the kernel's term order (numpy's exp / log stand in for expf / logf)"""
    x = F(logits).reshape(n, ld)[:, :N]
    y = np.asarray(targets, np.int64)
    valid = (y >= 0) & (y < C)
    ys = np.where(valid, y, 0)
    w = F(w)
    omw = F(1) - w

    def classes(a):
        z = np.zeros((n, C), F)
        for c in range(C):
            mem = cm[cp[c]:cp[c + 1]]
            s = a[:, mem[0]].copy()
            for j in mem[1:]:
                s = s + a[:, j]
            z[:, c] = s / F(mem.size)
        return z
    z = classes(x)
    t = z - z.max(1)[:, None]
    lse = np.log(_block_sum_f32(_strided_f32(np.exp(t).astype(F)))).astype(F)
    p = np.exp(t - lse[:, None]).astype(F)
    onehot = np.zeros((n, C), F)
    onehot[np.arange(n)[valid], ys[valid]] = 1
    g = p - omw * onehot
    L = lse - omw * t[np.arange(n), ys]
    if w != 0:
        tz = classes(F(tlogits).reshape(n, ldt)[:, :N])
        tt = tz - tz.max(1)[:, None]
        lt = np.log(_block_sum_f32(_strided_f32(np.exp(tt).astype(F)))).astype(F)
        q = np.exp(tt - lt[:, None]).astype(F)
        L = L - w * _block_sum_f32(_strided_f32(q * t))
        g = g - w * q
    g = (g / np.diff(cp).astype(F)[None, :]).astype(F)
    nv = F(valid.sum())
    inv = F(1) / nv if nv > 0 else F(0)
    loss = F(0)
    for r in range(n):
        loss = loss + inv * (L[r] if valid[r] else F(0))
    dz = np.where(valid[:, None], inv * g[:, ic], F(0)).astype(F)
    return dict(loss=loss, dz=dz, correct=float((valid & (z.argmax(1) == ys)).sum()))


def torch_soft_hybrid(z, tz, y, cp, cm, w):
    """the same loss from torch float64 tensors (autograd reaches z): the valid rows' mean of
    -(1 - w) log_softmax_C(zc)[y] - w sum_c softmax_C(tc)_c log_softmax_C(zc)_c, zc / tc the class means"""
    import torch
    C, N = len(cp) - 1, z.shape[1]
    M = torch.zeros((N, C), dtype=torch.float64)
    for c in range(C):
        mem = np.asarray(cm[cp[c]:cp[c + 1]], np.int64)
        M[mem, c] = 1.0 / mem.size
    ok = (y >= 0) & (y < C)
    if not bool(ok.any()):
        return z.sum() * 0.0
    ls = torch.log_softmax(z[ok] @ M, 1)
    q = torch.softmax(tz[ok] @ M, 1)
    hard = -ls[torch.arange(int(ok.sum())), y[ok]]
    return ((1.0 - w) * hard - w * (q * ls).sum(1)).mean()


# ----------------------------------------------------------------------------------------------------------------------
# grl_soft_proxy_ce
def soft_proxy_ce(logits, ld, tlogits, ldt, labels, cams, pcl, pcm, w, n, P, k_neg, w_intra, w_inter):
    """grl_soft_proxy_ce of include/grl_hip.h in float64 on the inputs given.  ``hard``: proxy_ref.proxy_ce of the student (own,
    negsel, valid, nv, correct and per valid row the sets A, Pos, U); ``r``: per valid row the two set records 'A' and 'U'; L,
    rows, loss, dz [n][P].  The teacher is read at the student's sets.  tlogits may be None when w = 0."""
    hard = PR.proxy_ce(logits, ld, labels, cams, pcl, pcm, n, P, k_neg, w_intra, w_inter)
    w = float(F(w))
    omw = 1.0 - w
    z = hard['z']
    tz = view(flat(tlogits), n, P, ldt).astype(np.float64) if w != 0.0 else np.zeros((n, P))
    wa, wu, nv = hard['wa'], hard['wu'], hard['nv']
    inv = 1.0 / nv if nv else 0.0
    recs, L, dz = {}, np.zeros(n), np.zeros((n, P))
    for i, hrec in hard['r'].items():
        own, Pos, npos = int(hard['own'][i]), hrec['Pos'], hrec['npos']
        a = soft_set(z[i], tz[i], hrec['A'], (np.arange(P) == own).astype(np.float64), w, omw)
        u = soft_set(z[i], tz[i], hrec['U'], Pos / float(npos), w, omw)
        ga, gu = wa * a['g'], wu * u['g']
        recs[i] = dict(A=a, U=u, ga=ga, gu=gu, Pos=Pos, npos=npos, own=own)
        L[i] = wa * a['L'] + wu * u['L']
        dz[i] = inv * (ga + gu)
    rows = inv * L
    return dict(hard=hard, r=recs, w=w, omw=omw, wa=wa, wu=wu, L=L, rows=rows, loss=rows.sum(), dz=dz, nv=nv, inv=inv,
                valid=hard['valid'], own=hard['own'], negsel=hard['negsel'], correct=hard['correct'])


def b_soft_proxy_ce(ref, n, P, e_in=None, e_tin=None):
    """-> dict(rows [n], loss, dz [n][P]) for the selection of the model.  Per valid row the set chain of A (H = t_own: u |t_own|,
    a one-hot) and of U (H = fl(sP ipos), sP the tree sum over Pos of t_j: (1 + k_ce_rowsum(P)) u sum |t_j|, ipos = fl(1 / |Pos|):
    DIV_ULP ulp, one product; h_j = ipos: r_h = DIV_ULP ulp), then as proxy_ref.b_proxy_ce:
      L = fl(fl(w_intra L_A) + fl(w_inter L_U)): w_intra e_LA + w_inter e_LU + 2 u (w_intra |L_A| + w_inter |L_U|)
      d = fl(fl(w_intra g_A) + fl(w_inter g_U)): w_intra e_gA + w_inter e_gU + 2 u (|ga| + |gu|)
      row = fl(inv L), dz = fl(inv d), inv = fl(1 / nv): DIV_ULP ulp;  loss: n - 1 serial additions.
    ``e_in`` / ``e_tin`` [n][P]: what the logits given carry, through d L / d z_j = d_j, d L / d tz_j = -w sum_S w_S q^S_j (t_j - X_S),
    d g^S_j / d z_k = p_j ([j = k] - p_k), d g^S_j / d tz_k = -w q_j ([j = k] - q_k)."""
    w, omw, inv = ref['w'], ref['omw'], ref['inv']
    wa, wu = abs(ref['wa']), abs(ref['wu'])
    r_inv = DIV_ULP * ULP
    k = k_ce_rowsum(P)
    e_rows, e_dz = np.zeros(n), np.zeros((n, P))
    for i, rec in ref['r'].items():
        a, u, Pos, npos = rec['A'], rec['U'], rec['Pos'], rec['npos']
        e_LA, e_gA, _, _ = e_soft_set(a, P, w, omw, U * abs(a['H']), 0.0)
        sabs = np.abs(u['t'][Pos]).sum()
        e_mean = (1 + k) * U * sabs / npos + abs(u['H']) * (DIV_ULP * ULP + U)
        e_LU, e_gU, _, _ = e_soft_set(u, P, w, omw, e_mean, DIV_ULP * ULP)
        for srec, name in ((a, 'A'), (u, 'U')):
            ez = np.zeros(P) if e_in is None else np.where(srec['S'], e_in[i], 0.0)
            et = np.zeros(P) if e_tin is None or w == 0.0 else np.where(srec['S'], e_tin[i], 0.0)
            p, q = srec['p'], srec['q']
            add_L = (np.abs(srec['g']) * ez).sum() + w * (q * np.abs(srec['t'] - srec['X']) * et).sum()
            add_g = p * (ez + (p * ez).sum()) + w * q * (et + (q * et).sum())
            if name == 'A':
                e_LA, e_gA = e_LA + add_L, e_gA + add_g
            else:
                e_LU, e_gU = e_LU + add_L, e_gU + add_g
        e_L = wa * e_LA + wu * e_LU + 2 * U * (wa * abs(a['L']) + wu * abs(u['L']))
        e_rows[i] = inv * e_L + abs(ref['rows'][i]) * (r_inv + U)
        e_d = wa * e_gA + wu * e_gU + 2 * U * (np.abs(rec['ga']) + np.abs(rec['gu']))
        e_dz[i] = inv * e_d + np.abs(ref['dz'][i]) * (r_inv + U) + TINY
    e_loss = e_rows.sum() + (n - 1) * U * np.abs(ref['rows']).sum()
    return dict(rows=SAFETY * e_rows, loss=SAFETY * e_loss, dz=SAFETY * e_dz)


def soft_proxy_ce_f32(logits, ld, tlogits, ldt, ref, w, n, P):
    """fp32 restatement in the kernel's term order for the sets of ``ref`` (a soft_proxy_ce result: the selection is exact integer
    work and is the model's); numpy's exp / log stand in for expf / logf.  A column outside a set adds +0 to a lane's sum."""
    z = F(logits).reshape(n, ld)[:, :P]
    w = F(w)
    omw = F(1) - w
    wa, wu = F(ref['wa']), F(ref['wu'])
    tz = F(tlogits).reshape(n, ldt)[:, :P] if w != 0 else None
    valid = ref['valid']
    nv = F(valid.sum())
    inv = F(1) / nv if nv > 0 else F(0)
    L, d = np.zeros(n, F), np.zeros((n, P), F)

    def tree(v):
        return _block_sum_f32(_strided_f32(v.astype(F)[None, :]))[0]
    for i, rec in ref['r'].items():
        own, Pos, ipos = rec['own'], rec['Pos'], F(1) / F(rec['npos'])
        parts = []
        for name in ('A', 'U'):
            S = rec[name]['S']
            mx = z[i][S].max()
            t = np.where(S, z[i] - mx, F(0)).astype(F)
            lse = F(np.log(tree(np.where(S, np.exp(t), F(0)))))
            p = np.exp(t - lse).astype(F)
            if name == 'A':
                h, H = (np.arange(P) == own).astype(F), t[own]
            else:
                h, H = np.where(Pos, ipos, F(0)).astype(F), tree(np.where(Pos, t, F(0))) * ipos
            Ls = lse - omw * H
            g = p - omw * h
            if w != 0:
                mt = tz[i][S].max()
                tt = np.where(S, tz[i] - mt, F(0)).astype(F)
                lt = F(np.log(tree(np.where(S, np.exp(tt), F(0)))))
                q = np.exp(tt - lt).astype(F)
                Ls = Ls - w * tree(np.where(S, q * t, F(0)))
                g = g - w * q
            parts.append((F(Ls), np.where(S, g, F(0)).astype(F)))
        L[i] = wa * parts[0][0] + wu * parts[1][0]
        d[i] = wa * parts[0][1] + wu * parts[1][1]
    loss = F(0)
    for r in range(n):
        loss = loss + inv * (L[r] if valid[r] else F(0))
    return dict(loss=loss, dz=(inv * d).astype(F))


def torch_soft_proxy(z, tz, ref, w):
    """the same loss from torch float64 tensors for the sets of ``ref`` (autograd reaches z; the selection is a constant): per
    valid row w_intra (-(1 - w) lsA[own] - w sum_A qA lsA) + w_inter (-(1 - w) mean_Pos lsU - w sum_U qU lsU), lsS / qS the
    log_softmax of z / the softmax of tz over S; the valid rows' mean"""
    import torch
    total = z.sum() * 0.0
    for i, rec in ref['r'].items():
        for name, ws in (('A', ref['wa']), ('U', ref['wu'])):
            S = torch.from_numpy(np.flatnonzero(rec[name]['S']))
            ls = torch.log_softmax(z[i][S], 0)
            q = torch.softmax(tz[i][S], 0)
            h = torch.from_numpy(rec[name]['h'])[S]
            total = total + ws * (-(1.0 - w) * (h * ls).sum() - w * (q * ls).sum())
    return total / ref['nv'] if ref['nv'] else total


# ----------------------------------------------------------------------------------------------------------------------
# the losses: from the rows and the memory
def e_gemm(abs_logits, D):
    """the fp32 GEMM with the scale in its epilogue: a sum of D products in some order and one more rounding (cmem_ref)"""
    return (D + 1) * U * abs_logits


def hybrid_loss(d, teacher, D, w, g=1.0, temp=HR.LOSS_TEMP):
    """SoftHybridMemoryLoss.forward and the gradient of its backward on the memory as given (hybrid_ref.in_loss inputs):
    logits = scalar x . mem^T, tlogits = scalar teacher . mem^T, soft_hybrid_ce, dx = g scalar dz . mem"""
    n, N = np.shape(d['x'])[0], d['mem'].shape[0]
    X, T, M = view(flat(d['x']), n, D, D), view(flat(teacher), n, D, D), view(flat(d['mem']), N, D, D)
    scalar = float(F(1.0 / temp))
    z, tz = scalar * (X @ M.T), scalar * (T @ M.T)
    ce = soft_hybrid_ce(z.reshape(-1), N, tz.reshape(-1), N, d['targets'], d['cp'], d['cm'], d['ic'], w, n, N, d['C'])
    og = LR.oim_grad(ce['dz'].reshape(-1), N, M, [g], scalar, n, N, D)
    e_z, e_t = e_gemm(scalar * (np.abs(X) @ np.abs(M).T), D), e_gemm(scalar * (np.abs(T) @ np.abs(M).T), D)
    bd = b_soft_hybrid_ce(ce, n, N, d['C'], e_in=e_z, e_tin=e_t)
    return dict(ce=ce, loss=ce['loss'], logits=z, dz=ce['dz'], dx=og['dx'], og=og, b_logits=SAFETY * e_z, b_loss=bd['loss'],
                b_dz=bd['dz'])


def proxy_loss(d, teacher, P, k, wts, w, g=1.0, temp=PR.LOSS_TEMP):
    """SoftProxyMemoryLoss.forward and the gradient of its backward on the memory as given (proxy_ref.in_loss inputs)"""
    n, D = np.shape(d['x'])[0], np.shape(d['x'])[1]
    X, T, M = view(flat(d['x']), n, D, D), view(flat(teacher), n, D, D), view(flat(d['mem']), P, D, D)
    scalar = float(F(1.0 / temp))
    z, tz = scalar * (X @ M.T), scalar * (T @ M.T)
    ce = soft_proxy_ce(z.reshape(-1), P, tz.reshape(-1), P, d['labels'], d['cams'], d['pcl'], d['pcm'], w, n, P, min(k, P), *wts)
    og = LR.oim_grad(ce['dz'].reshape(-1), P, M, [g], scalar, n, P, D)
    e_z, e_t = e_gemm(scalar * (np.abs(X) @ np.abs(M).T), D), e_gemm(scalar * (np.abs(T) @ np.abs(M).T), D)
    bd = b_soft_proxy_ce(ce, n, P, e_in=e_z, e_tin=e_t)
    return dict(ce=ce, loss=ce['loss'], logits=z, abs_logits=scalar * (np.abs(X) @ np.abs(M).T), dz=ce['dz'], dx=og['dx'], og=og,
                b_logits=SAFETY * e_z, b_loss=bd['loss'], b_dz=bd['dz'])


def proxy_loss_seed(P, k, tag='soft'):
    """the first seed whose float64 selection satisfies proxy_ref's gap condition (the selection behind the GEMM is then the
    model's)"""
    for seed in range(64):
        d = PR.in_loss(P, k, seed, tag)
        if PR.gap_ok(PR.loss(d, P, k, PR.LOSS_W), PR.LOSS_D):
            return seed
    raise AssertionError('no seed below 64 satisfies the gap condition for P = %d, k = %d' % (P, k))


def teacher_rows(x, tag):
    """unit teacher rows near the student's: x + 0.3 N(0, 1) / sqrt(D), renormalised"""
    r = rng_for('soft-teacher', tag, x.shape[0], x.shape[1])
    return unit_rows(np.asarray(x, np.float64) + 0.3 * r.standard_normal(x.shape) / np.sqrt(x.shape[1]))
