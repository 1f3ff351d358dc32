"""The OIM, triplet and pair-verification loss kernels restated in float64 (numpy only): the independent reference of the fp32
kernels of grl_amd/csrc/loss.hip and of oim_update_kernel in train_head.hip.

One function per C ABI wrapper (include/grl_hip.h), in the conventions of tests/head_ref.py: device buffers are flat arrays
that start where the pointer points, leading dimensions are taken as the wrapper takes them, a destination that is written
through a leading dimension is handed over with its contents before the call (``*0``) and comes back whole, an output whose
pointer may be NULL is asked for with a flag.  Next to its results every function returns the sums of absolute terms that
the bounds of tests/loss_bounds.py are built from.

Written from the formulas of the reference losses -- reid/loss/oim.py (F.cross_entropy over scalar * x . LUT^T, its gradient,
the look-up-table update), reid/loss/triplet.py (batch-hard, soft margin or hinge), reid/loss/pairloss.py and
reid/train/trainer.py (softmax over two scores, BCELoss and its clamps, top-1 precision) -- not from the kernel bodies.

Two places restate fp32 arithmetic instead of float64, because they are exact predicates / selections on fp32 inputs and a
float64 answer would be a different function: ``triplet_select`` (the selection on a given fp32 distance matrix, with torch's
value formulas d * mask and fl(d + 1e5 * same)) and the decision ``s > 1 - s`` of ``pair_bce``."""
import numpy as np

from head_ref import f64, flat, view

F32 = np.float32


def _labels(a):
    return np.asarray(a, dtype=np.int64).reshape(-1)


# ----------------------------------------------------------------------------------------------------------------------
# OIM: cross entropy, its gradient, the gradient of the features, the table update
def softmax_ce(logits, ld, labels, weight, n, c, dz0=None, ldd=0):
    """F.cross_entropy(logits, labels, weight, reduction='mean') with every label outside [0, c) ignored, the number of
    valid rows whose FIRST arg-max is the label, and (dz0 given: the destination's contents before the call) the gradient
    of the loss in the n x c window of the ldd-wide destination.  No valid label: loss, correct and gradient are 0."""
    z = view(flat(logits), n, c, ld)
    y = _labels(labels)[:n]
    ok = (y >= 0) & (y < c)
    ys = np.where(ok, y, 0)
    w = np.ones(c) if weight is None else flat(weight)[:c]
    wy = np.where(ok, w[ys], 0.0)
    wsum = wy.sum()
    gscale = wy / wsum if wsum > 0 else np.zeros(n)
    mx = z.max(1)
    t = z - mx[:, None]                                 # <= 0
    e = np.exp(t)
    s = e.sum(1)
    lse = np.log(s)
    ty = t[np.arange(n), ys]
    nll = lse - ty                                      # -log softmax at the label
    rows = np.where(ok, gscale * nll, 0.0)
    arg = z.argmax(1)                                   # numpy: the first index at the maximum
    hit = ok & (arg == ys)
    p = np.exp(t - lse[:, None])
    onehot = np.zeros((n, c))
    onehot[np.arange(n)[ok], ys[ok]] = 1.0
    dzv = gscale[:, None] * (p - onehot)
    out = dict(loss=rows.sum(), rows=rows, correct=float(hit.sum()), hits=hit.astype(np.float64), ok=ok, gscale=gscale, wsum=wsum,
               t=t, e=e, s=s, lse=lse, ty=ty, nll=nll, p=p, onehot=onehot, dz_val=dzv)
    if dz0 is not None:
        buf = flat(dz0).copy()
        view(buf, n, c, ldd)[:] = dzv
        out['dz'] = buf
    return out


def oim_grad(dlogits, ldd, lut, g, alpha, n, c, D):
    """dx = (alpha g) dl[:, :c] @ lut; g None (a NULL pointer): 1."""
    dl = view(flat(dlogits), n, c, ldd)
    L = view(flat(lut), c, D, D)
    a = float(alpha) * (1.0 if g is None else float(flat(g)[0]))
    return dict(dx=a * (dl @ L), abs_dx=abs(a) * (np.abs(dl) @ np.abs(L)), a=a)


def oim_update(lut, x, labels, n, D, num_classes, momentum):
    """for every sample, in batch order: lut[y] = m lut[y] + (1 - m) x; lut[y] /= |lut[y]|.  A label outside the table is
    skipped.  `steps`: per replayed sample (row, the sample, the row before, the blend r, |r|^2) for the bounds."""
    L = view(flat(lut).copy(), num_classes, D, D)
    X = view(flat(x), n, D, D)
    m = float(momentum)
    steps = []
    for j, y in enumerate(_labels(labels)[:n]):
        if y < 0 or y >= num_classes:
            continue
        before = L[y].copy()
        r = m * before + (1.0 - m) * X[j]
        ss = (r * r).sum()
        L[y] = r / np.sqrt(ss)
        steps.append(dict(row=int(y), j=j, before=before, r=r, ss=ss, after=L[y].copy()))
    return dict(lut=L, steps=steps)


# ----------------------------------------------------------------------------------------------------------------------
# the batch-hard triplet loss
EPS_DIST = 1e-12


def triplet_dist(f, n, D):
    """dist[i][j] = sqrt(sum (f_i - f_j)^2 + 1e-12); ss: the sums of squares"""
    f = view(flat(f), n, D, D)
    d = f[:, None, :] - f[None, :, :]
    ss = (d * d).sum(2)
    return dict(dist=np.sqrt(ss + EPS_DIST), ss=ss)


def _soft_or_hinge(z, soft, margin32):
    z = f64(z)
    if soft:                                            # log(1 + exp(z)), stable
        return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))
    return np.maximum(z + float(margin32), 0.0)


def triplet_select(dist32, ids, n, soft, margin):
    """The selection, bit for bit, in fp32 on the fp32 matrix handed in: hardest positive = first index at the maximum of
    p = d * [same id, j != i], hardest negative = first index at the minimum of q = fl(d + 1e5 * [same id]); sel[2i] = -1
    when the maximum sits on a masked candidate (no positive in the batch: no gradient); z = fl(vp - vn).  The loss is the
    float64 function of that fp32 z."""
    d = np.asarray(dist32, dtype=F32).reshape(n, n)
    y = _labels(ids)[:n]
    same = y[:, None] == y[None, :]
    pos = same & ~np.eye(n, dtype=bool)
    p = d * pos.astype(F32)
    q = d + F32(1e5) * same.astype(F32)
    assert p.dtype == F32 and q.dtype == F32
    jp, jn = p.argmax(1), q.argmin(1)                   # first index at the extremum
    r = np.arange(n)
    vp, vn = p[r, jp], q[r, jn]
    z = vp - vn
    assert z.dtype == F32
    sel = np.empty((n, 2), np.int32)
    sel[:, 0] = np.where(pos[r, jp], jp, -1)
    sel[:, 1] = jn
    return dict(sel=sel.reshape(-1), z=z, vp=vp, vn=vn, loss=_soft_or_hinge(z, soft, F32(margin)))


def gz_of(z32, dloss, soft, margin):
    """d loss_i / d z_i times the upstream gradient: sigmoid(z), or the fp32 predicate fl(z + margin) > 0"""
    z32 = np.asarray(z32, dtype=F32).reshape(-1)
    dl = flat(dloss)[:z32.size]
    if soft:
        zz = f64(z32)
        e = np.exp(-np.abs(zz))
        return dl * np.where(zz >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return dl * ((z32 + F32(margin)) > F32(0)).astype(np.float64)


def triplet_bwd(f, dist, sel, z32, dloss, soft, margin, n, D, gz=None):
    """The gradient of sum_i dloss_i loss_i given the selection: anchor i pulls (f_i - f_p) gz / d_ip and pushes
    -(f_i - f_n) gz / d_in on itself, and the opposite on p and n.  abs: the sum of the absolute terms of every element,
    terms: how many terms it has."""
    f = view(flat(f), n, D, D)
    dist = f64(dist).reshape(n, n)
    sel = np.asarray(sel, dtype=np.int64).reshape(n, 2)
    gz = gz_of(z32, dloss, soft, margin) if gz is None else f64(gz)
    df, ab, cnt = np.zeros((n, D)), np.zeros((n, D)), np.zeros(n, np.int64)

    def add(r, t):
        df[r] += t; ab[r] += np.abs(t); cnt[r] += 1

    for i in range(n):
        p, q = sel[i]
        if p >= 0:
            t = (f[i] - f[p]) * (gz[i] / dist[i, p])
            add(i, t)
            if p != i:
                add(p, -t)
        t = (f[i] - f[q]) * (gz[i] / dist[i, q])
        add(i, -t)
        if q != i:
            add(q, t)
    return dict(df=df, abs_df=ab, terms=cnt, gz=gz)


def triplet_full(f, ids, n, D, soft, margin, dloss=None):
    """Everything in float64: distances, the selection by the plain expressions (dist * pos).max(1), (dist + 1e5 same).min(1),
    the loss and, with dloss, the gradient.  gap_p / gap_n: the distance between the best and the second-best candidate."""
    dd = triplet_dist(f, n, D)
    dist = dd['dist']
    y = _labels(ids)[:n]
    same = y[:, None] == y[None, :]
    pos = same & ~np.eye(n, dtype=bool)
    p, q = dist * pos, dist + 1e5 * same
    jp, jn = p.argmax(1), q.argmin(1)
    r = np.arange(n)
    vp, vn = p[r, jp], q[r, jn]
    z = vp - vn
    sel = np.empty((n, 2), np.int32)
    sel[:, 0] = np.where(pos[r, jp], jp, -1)
    sel[:, 1] = jn
    if n > 1:
        ps, qs = np.sort(p, 1), np.sort(q, 1)
        # an anchor without a positive has no decision to make on that side: every candidate is the masked 0
        gap_p = np.where(pos.any(1), ps[:, -1] - ps[:, -2], np.inf)
        gap_n = qs[:, 1] - qs[:, 0]
    else:
        gap_p, gap_n = np.full(n, np.inf), np.full(n, np.inf)
    out = dict(dist=dist, ss=dd['ss'], sel=sel.reshape(-1), z=z, vp=vp, vn=vn, same_n=same[r, jn], gap_p=gap_p, gap_n=gap_n,
               loss=_soft_or_hinge(z, soft, F32(margin)))
    if dloss is not None:
        dl = flat(dloss)[:n]
        if soft:
            e = np.exp(-np.abs(z))
            gz = dl * np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        else:
            gz = dl * (z + float(F32(margin)) > 0)
        out.update(triplet_bwd(f, dist, sel, None, None, soft, margin, n, D, gz=gz))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# pair verification
def softmax2(scores, m):
    """p1, p0 of the softmax over the two scores of each of the m pairs (stable)"""
    s = view(flat(scores), m, 2, 2)
    mx = s.max(1)
    ta, tb = s[:, 0] - mx, s[:, 1] - mx
    ea, eb = np.exp(ta), np.exp(tb)
    return dict(p=eb / (ea + eb), p0=ea / (ea + eb), ta=ta, tb=tb, ea=ea, eb=eb)


def softmax2_bwd(p, p0, dp, m):
    """softmax backward with g = (0, dp) on the probabilities handed in: ds0 = -g p1 p0, ds1 = (g - g p1) p1"""
    p, p0, g = flat(p)[:m], flat(p0)[:m], flat(dp)[:m]
    gp = g * p
    return dict(ds=np.stack([-gp * p0, (g - gp) * p], 1), gp=gp, g=g, p=p, p0=p0)


def pair_bce(prob, tar_probe, tar_gallery, n):
    """BCELoss(mean) of prob[a][b] against y_ab = [tp[b] == tg[a]] with torch's clamps (logs at -100, the backward's
    denominator at 1e-12), d loss / d prob, and the share of elements whose decision fl32(s) > fl32(1 - s) equals y."""
    s32 = np.asarray(prob, dtype=F32).reshape(-1)[:n * n].reshape(n, n)
    s = f64(s32)
    tp, tg = _labels(tar_probe)[:n], _labels(tar_gallery)[:n]
    y = (tp[None, :] == tg[:, None]).astype(np.float64)
    with np.errstate(divide='ignore'):
        ls, l1 = np.maximum(np.log(s), -100.0), np.maximum(np.log1p(-s), -100.0)
    term = -(y * ls + (1.0 - y) * l1)
    N = float(n * n)
    dec = (s32 > F32(1) - s32).astype(np.float64)
    hits = float((dec == y).sum())
    den = np.maximum((1.0 - s) * s, 1e-12)
    return dict(loss=term.sum() / N, term=term, y=y, hits=hits, prec=hits / N, dprob=(s - y) / den / N, log_used=np.where(y > 0, ls, l1))


def scale_dev(x, g, alpha, n):
    return dict(y=(float(alpha) * float(flat(g)[0])) * flat(x)[:n])
