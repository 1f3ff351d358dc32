"""Float64 model, fp32 numpy restatements, inputs and per-element error bounds for the mean-teacher kernels: grl_soft_ce
(grl_amd/csrc/softce.hip) and grl_ema_update (grl_amd/csrc/ema.hip) -- shared by test_teacher_cpu.py (no GPU) and
test_gpu_teacher.py.  U, SAFETY, check, RATIOS, dump_ratios are bn_bounds' own; the libm constants, TINY, trips, k_ce_rowsum and
the restated reductions are loss_bounds' / head_bounds' own.

grl_ema_update has no bound: dst = fl(fl(a dst) + fl(b src)) is two products and one sum, each rounded once (-ffp-contract=off),
which numpy float32 arithmetic reproduces BIT FOR BIT (``ema_f32``).

The bounds of grl_soft_ce are derived per element the way loss_bounds.b_softmax_ce is, none is fitted: the fp32 chain read from
the kernel x u x |terms| (u = 2^-24, every * and + rounds once), the errors of a stage carried into the next through the
derivative, SAFETY (2) once at the end (``b_soft_ce``'s docstring has the chain).  w is handed over as an fp32 value and is
exact; omw = fl(1 - w) carries one rounding."""
import numpy as np

from loss_bounds import (U, SAFETY, check, RATIOS, dump_ratios, EXPF_ULP, LOGF_ULP, DIV_ULP, ULP, TINY, trips,     # noqa: F401
                         k_ce_rowsum, rng_for, f32, _block_sum_f32, _strided_f32)

F = np.float32
EMA_CHUNK = 4096                # GRL_EMA_CHUNK of include/grl_hip.h

# ----------------------------------------------------------------------------------------------------------------------
# the sweeps
CE_N = (1, 2, 9, 33)
CE_C = (1, 2, 255, 256, 257, 1030)
CE_W = (0.5, 1.0)
CE_MAG = 20.0                   # 1 / temp at temp 0.05: the largest scaled similarity of unit rows
CE_CASES = tuple((n, c, 'mixed') for n in CE_N for c in CE_C) + ((9, 257, 'none'), (2, 2, 'none'))
CE_LD = (3, 5, 1)               # ld - c, ldt - c, ldd - c: larger than c and different from each other

EMA_NUMEL = (1, 3, 4, 5, 1023, 1024, 1025, EMA_CHUNK - 1, EMA_CHUNK, EMA_CHUNK + 1, 3 * EMA_CHUNK + 3)
EMA_COUNTS = (1, 37)
EMA_ALPHAS = (0.0, 0.5, 0.999, 1.0)
EMA_SENTINEL = 12345.0
EMA_SENT = 4                    # sentinel floats between the tensors (a multiple of 4: the offsets below decide the alignment)


# ----------------------------------------------------------------------------------------------------------------------
# inputs
def ce_tie(c):
    """the two columns of the planted tie: the same lane on its second trip where the row is long enough, else the ends"""
    return (3, 259) if c > 259 else (0, c - 1)


def in_soft_ce(n, c, pattern):
    """Student logits 20 cos(.) in [-20, 20], teacher logits = the student's + 4 N(0, 1) clipped to the same range (a teacher
    that mostly agrees), both in wider buffers whose gaps hold 1e30.  Labels: 'mixed' -- valid, with -1 in row 1 and c in the
    last row when n >= 3, one of the two in row 1 when n = 2; 'none' -- no valid row.  c >= 2: row 0 holds the row maximum twice
    (ce_tie) with the label on the FIRST of the two, and with n >= 9 row 2 holds it with the label on the SECOND."""
    r = rng_for('softce', n, c, pattern)
    z = f32(CE_MAG * np.cos(r.uniform(0.0, 2.0 * np.pi, (n, c))))
    t = f32(np.clip(z.astype(np.float64) + 4.0 * r.standard_normal((n, c)), -CE_MAG, CE_MAG))
    y = r.randint(0, c, n).astype(np.int64)
    if pattern == 'none':
        y[:] = np.where(np.arange(n) % 2 == 0, -1, c)
    else:
        if n >= 3:
            y[1], y[n - 1] = -1, c
        elif n == 2:
            y[1] = -1 if c % 2 else c
        if c >= 2:
            a, b = ce_tie(c)
            z[0, a] = z[0, b] = F(CE_MAG + 1.0)
            y[0] = a
            if n >= 9:
                z[2, a] = z[2, b] = F(CE_MAG + 1.0)
                y[2] = b
    ld, ldt = c + CE_LD[0], c + CE_LD[1]
    zb, tb = f32(np.full((n, ld), 1e30)), f32(np.full((n, ldt), 1e30))
    zb[:, :c], tb[:, :c] = z, t
    return dict(logits=zb.reshape(-1), tlogits=tb.reshape(-1), labels=y, ld=ld, ldt=ldt, ldd=c + CE_LD[2])


def ema_layout(count, seed=0):
    """[(numel, dst offset, src offset)] of a table of ``count`` tensors inside one dst and one src buffer, with the buffers'
    lengths: numel runs through EMA_NUMEL, EMA_SENT sentinel floats lie between neighbours, and the offsets are 16-byte
    aligned except where i % 4 says otherwise -- i % 4 == 1: dst one float off, i % 4 == 2: src one float off."""
    r = rng_for('ema', count, seed)
    order = list(EMA_NUMEL) if count >= len(EMA_NUMEL) else [EMA_NUMEL[-1]]
    while len(order) < count:
        order.append(EMA_NUMEL[r.randint(len(EMA_NUMEL))])
    out, od, os_ = [], EMA_SENT, EMA_SENT
    for i, numel in enumerate(order[:count]):
        d0 = od + (1 if i % 4 == 1 else 0)
        s0 = os_ + (1 if i % 4 == 2 else 0)
        out.append((numel, d0, s0))
        od = (d0 + numel + EMA_SENT + 3) // 4 * 4
        os_ = (s0 + numel + EMA_SENT + 3) // 4 * 4
    return out, od + EMA_SENT, os_ + EMA_SENT


def in_ema(count, seed=0):
    """dst and src buffers of ema_layout, N(0, 1) in the tensors and the sentinel EMA_SENTINEL around them; one NaN and one inf
    in src (the first element of the first tensor, the last of the largest)."""
    lay, nd, ns = ema_layout(count, seed)
    r = rng_for('ema-in', count, seed)
    dst, src = f32(np.full(nd, EMA_SENTINEL)), f32(np.full(ns, EMA_SENTINEL))
    for numel, d0, s0 in lay:
        dst[d0:d0 + numel] = r.standard_normal(numel)
        src[s0:s0 + numel] = r.standard_normal(numel)
    big = max(range(count), key=lambda i: lay[i][0])
    src[lay[big][2] + lay[big][0] - 1] = np.inf
    src[lay[0][2]] = np.nan
    return dict(layout=lay, dst=dst, src=src)


def chunk_first(numels):
    out = [0]
    for m in numels:
        out.append(out[-1] + (m + EMA_CHUNK - 1) // EMA_CHUNK)
    return np.asarray(out, np.int64)


# ----------------------------------------------------------------------------------------------------------------------
# float64 model
def soft_ce(logits, ld, tlogits, ldt, labels, w, n, c):
    """grl_soft_ce in float64 on the fp32 inputs.  L_i = lse(z_i) - (1 - w) z_i[y] - w sum_j softmax(t_i)_j z_i[j] over the valid
    rows (label in [0, c)), loss = sum L_i / nv, dz = (softmax(z) - (1 - w) onehot - w softmax(t)) / nv, correct = the valid rows
    whose FIRST arg-max of z is the label.  tlogits may be None when w = 0."""
    z = np.asarray(logits, np.float64).reshape(n, ld)[:, :c]
    w = float(F(w))
    tz = np.asarray(tlogits, np.float64).reshape(n, ldt)[:, :c] if w != 0.0 else z
    y = np.asarray(labels, np.int64)[:n]
    ok = (y >= 0) & (y < c)
    ys = np.where(ok, y, 0)
    nv = int(ok.sum())
    inv = 1.0 / nv if nv else 0.0
    omw = 1.0 - w
    mx, mt = z.max(1), tz.max(1)
    t, tt = z - mx[:, None], tz - mt[:, None]
    e, et = np.exp(t), np.exp(tt)
    s, st = e.sum(1), et.sum(1)
    lse, lt = np.log(s), np.log(st)
    p, q = np.exp(t - lse[:, None]), np.exp(tt - lt[:, None])
    cross = (q * t).sum(1)
    ty = t[np.arange(n), ys]
    L = np.where(ok, lse - omw * ty - w * cross, 0.0)
    rows = inv * L
    onehot = np.zeros((n, c))
    onehot[np.arange(n)[ok], ys[ok]] = 1.0
    d = np.where(ok[:, None], p - omw * onehot - w * q, 0.0)
    hit = ok & (z.argmax(1) == ys)
    return dict(loss=rows.sum(), rows=rows, L=L, correct=float(hit.sum()), ok=ok, nv=nv, inv=inv, w=w, omw=omw, t=t, tt=tt, e=e,
                et=et, s=s, st=st, lse=lse, lt=lt, p=p, q=q, cross=cross, abs_cross=(q * np.abs(t)).sum(1), ty=ty, onehot=onehot,
                d=d, dz_val=inv * d)


def torch_soft_ce(z, tz, y, w):
    """the same loss from torch float64 tensors (autograd reaches z and tz): the valid rows' mean of
    -(1 - w) log_softmax(z)[y] - w sum_j softmax(tz)_j log_softmax(z)_j"""
    import torch
    c = z.shape[1]
    ok = (y >= 0) & (y < c)
    if not bool(ok.any()):
        return z.sum() * 0.0
    ls = torch.log_softmax(z[ok], 1)
    q = torch.softmax(tz[ok], 1)
    hard = -ls[torch.arange(int(ok.sum())), y[ok]]
    soft = -(q * ls).sum(1)
    return ((1.0 - w) * hard + w * soft).mean()


# ----------------------------------------------------------------------------------------------------------------------
# the bound
def b_soft_ce(ref, n, c):
    """Student row, as b_softmax_ce: t_j = fl(z_j - mx): u |t_j| (mx is exact); e_j = expf(t_j): relative u |t_j| + EXPF_ULP ulp;
    s = sum e_j: k_ce_rowsum(c) u s; lse = logf(s): e_s / s + LOGF_ULP ulp |lse|, absolute.  The teacher's row the same: e_lt.
      q_j = expf(fl(fl(tz_j - mt) - lt)): relative r_q = u |tt_j| + e_lt + u |tt_j - lt| + EXPF_ULP ulp;  e_q = q r_q + TINY
      X = sum_j fl(q_j t_j): per term |t_j| e_q + q_j u |t_j| (t's own rounding) + u |q_j t_j|, the sum k_ce_rowsum(c) u sum |q t|
      omw = fl(1 - w): u |omw|
      L = fl(fl(lse - fl(omw t_y)) - fl(w X)):
          e_lse + (u omw |t_y| [omw] + u omw |t_y| [t_y] + u omw |t_y| [product]) + u |lse - omw t_y| + w e_X + u w |X| + u |L|
      inv = fl(1 / nv): relative r_inv = DIV_ULP ulp (nv is an exact integer);  row = fl(inv L): inv e_L + |row| (r_inv + u)
      loss: n - 1 serial additions of the rows
      p_j = expf(fl(t_j - lse)): relative u |t_j| + e_lse + u |t_j - lse| + EXPF_ULP ulp;  e_p = p r_p + TINY
      d_j = fl(fl(p_j - fl(omw [j = y])) - fl(w q_j)): e_p + 2 u omw [j = y] + u |p - omw [j = y]| + w e_q + u w q + u |d|
      dz = fl(inv d): inv e_d + |dz| (r_inv + u) + TINY.
    Invalid rows are exact zeros (bound 0)."""
    w, omw, inv, ok = ref['w'], ref['omw'], ref['inv'], ref['ok']
    at, att = np.abs(ref['t']), np.abs(ref['tt'])
    k = k_ce_rowsum(c)
    e_s = (ref['e'] * (U * at + EXPF_ULP * ULP)).sum(1) + k * U * ref['s'] + TINY
    e_lse = e_s / ref['s'] + LOGF_ULP * ULP * np.abs(ref['lse'])
    e_st = (ref['et'] * (U * att + EXPF_ULP * ULP)).sum(1) + k * U * ref['st'] + TINY
    e_lt = e_st / ref['st'] + LOGF_ULP * ULP * np.abs(ref['lt'])
    if w == 0.0:
        e_lt = np.zeros_like(e_lt)
    r_q = U * att + e_lt[:, None] + U * np.abs(ref['tt'] - ref['lt'][:, None]) + EXPF_ULP * ULP
    e_q = ref['q'] * r_q + TINY
    e_x = (at * e_q + 2 * U * ref['q'] * at).sum(1) + k * U * ref['abs_cross']
    aty = np.abs(ref['ty'])
    e_L = (e_lse + 3 * U * omw * aty + U * np.abs(ref['lse'] - omw * ref['ty']) + w * e_x + U * w * np.abs(ref['cross'])
           + U * np.abs(ref['L']))
    r_inv = DIV_ULP * ULP
    e_row = np.where(ok, inv * e_L + np.abs(ref['rows']) * (r_inv + U), 0.0)
    e_loss = e_row.sum() + (n - 1) * U * np.abs(ref['rows']).sum()
    r_p = U * at + e_lse[:, None] + U * np.abs(ref['t'] - ref['lse'][:, None]) + EXPF_ULP * ULP
    e_p = ref['p'] * r_p + TINY
    oh = ref['onehot']
    e_d = (e_p + 2 * U * omw * oh + U * np.abs(ref['p'] - omw * oh) + w * e_q + U * w * ref['q'] + U * np.abs(ref['d']))
    e_dz = np.where(ok[:, None], inv * e_d + np.abs(ref['dz_val']) * (r_inv + U) + TINY, 0.0)
    return dict(rows=SAFETY * e_row, loss=SAFETY * e_loss, dz=SAFETY * e_dz)


def memory_loss(x, teacher, cent, labels, w, n, D, K, temp):
    """SoftClusterMemoryLoss.forward for the memory as given: z = scalar x . cent^T and tz = scalar teacher . cent^T with
    scalar = float32(1 / temp), then ``soft_ce`` on the float64 logits."""
    X, T = np.asarray(x, np.float64).reshape(n, D), np.asarray(teacher, np.float64).reshape(n, D)
    C = np.asarray(cent, np.float64).reshape(K, D)
    scalar = float(F(1.0 / temp))
    z, tz = scalar * (X @ C.T), scalar * (T @ C.T)
    ce = soft_ce(z.reshape(-1), K, tz.reshape(-1), K, labels, w, n, K)
    return dict(ce=ce, loss=ce['loss'], logits=z, tlogits=tz, abs_logits=scalar * (np.abs(X) @ np.abs(C).T),
                abs_tlogits=scalar * (np.abs(T) @ np.abs(C).T), scalar=scalar)


def b_memory_loss(ref, n, D, K):
    """end to end from the rows and the memory: grl_soft_ce's own bound on exact logits plus the two logits' errors -- (D + 1) u
    sum |terms| each, cmem_ref.e_logits: D products and additions of the K-blocked GEMM and the scale -- through the derivatives
    d L_i / d z_ij = d_ij and d L_i / d tz_ik = -w q_ik (t_ik - X_i)."""
    ce = ref['ce']
    e_z, e_t = (D + 1) * U * ref['abs_logits'], (D + 1) * U * ref['abs_tlogits']
    own = b_soft_ce(ce, n, K)
    thru = ce['inv'] * (np.abs(ce['d']) * e_z + ce['w'] * ce['q'] * np.abs(ce['t'] - ce['cross'][:, None]) * e_t)
    return dict(loss=own['loss'] + SAFETY * np.where(ce['ok'][:, None], thru, 0.0).sum(), logits=SAFETY * e_z)


# ----------------------------------------------------------------------------------------------------------------------
# fp32 restatements in the kernels' order (numpy's exp / log stand in for the device's expf / logf)
def soft_ce_f32(logits, ld, tlogits, ldt, labels, w, n, c):
    z = F(logits).reshape(n, ld)[:, :c]
    y = np.asarray(labels, np.int64)[:n]
    ok = (y >= 0) & (y < c)
    ys = np.where(ok, y, 0)
    w = F(w)
    omw = F(1) - w
    mx = z.max(1)
    t = z - mx[:, None]
    lse = np.log(_block_sum_f32(_strided_f32(np.exp(t).astype(F)))).astype(F)
    p = np.exp(t - lse[:, None]).astype(F)
    onehot = np.zeros((n, c), F)
    onehot[np.arange(n)[ok], ys[ok]] = 1
    d = p - omw * onehot
    L = lse - omw * t[np.arange(n), ys]
    if w != 0:
        tz = F(tlogits).reshape(n, ldt)[:, :c]
        tt = tz - tz.max(1)[:, None]
        lt = np.log(_block_sum_f32(_strided_f32(np.exp(tt).astype(F)))).astype(F)
        q = np.exp(tt - lt[:, None]).astype(F)
        cross = _block_sum_f32(_strided_f32(q * t))
        L = L - w * cross
        d = d - w * q
    nv = F(0)
    for r in range(n):
        nv = nv + F(ok[r])
    inv = F(1) / nv if nv > 0 else F(0)
    loss = F(0)
    for r in range(n):
        loss = loss + inv * (L[r] if ok[r] else F(0))
    dz = np.where(ok[:, None], inv * d, F(0)).astype(F)
    hit = ok & (z.argmax(1) == ys)
    return dict(loss=loss, dz=dz, correct=float(hit.sum()))


def ema_f32(dst, src, a, b):
    """dst = fl(fl(a dst) + fl(b src)), a and b the fp32 factors the kernel receives: the kernel's bits"""
    with np.errstate(invalid='ignore', over='ignore'):
        return (F(a) * F(dst)).astype(F) + (F(b) * F(src)).astype(F)


def ema_expected(d, a, b):
    """the dst buffer of ``in_ema`` after one launch with the factors (a, b): every tensor of the layout through ema_f32, the
    sentinels as they were"""
    out = d['dst'].copy()
    for numel, d0, s0 in d['layout']:
        out[d0:d0 + numel] = ema_f32(d['dst'][d0:d0 + numel], d['src'][s0:s0 + numel], a, b)
    return out


def ema_alpha(step, alpha):
    """MMT's ramp, restated: (a, 1 - a) as fp32"""
    a = min(1.0 - 1.0 / (step + 1), alpha)
    return F(a), F(1.0 - a)
