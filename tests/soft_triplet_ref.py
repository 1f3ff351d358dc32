"""The soft softmax-triplet kernels (grl_amd/csrc/soft_triplet.hip) restated: the float64 model of the teacher
part, the loss and the gradient, an fp32 restatement of the discrete and ordered parts, the sweep and the per-element
bounds -- shared by test_soft_triplet_cpu.py (no GPU) and test_gpu_soft_triplet.py.

The student part is loss.hip's own: the distances, the selection, the gather-form backward, their inputs, bounds and fp32
restatement are tests/loss_ref.py's and tests/loss_bounds.py's, reused as they stand.  What is added:

  t_i = tp - tn,  tp = [anchor has a positive] td(i, jp),  tn = td(i, jn) + 1e5 [ids[jn] == ids[i]]     (teacher distances at
                                                                                         the STUDENT's indices, its masks mirrored)
  q_i = sigmoid(t_i),      L_i = log(1 + exp(z_i)) - w q_i z_i,      gz_i = dloss_i (sigmoid(z_i) - w q_i)

w is the fp32 value the kernel receives.  Bounds are derived per element the way loss_bounds derives its own, none is fitted:
depth of the fp32 chain x u x sum|terms| (every * and + rounds once), the error of a stage that feeds the next carried through
the derivative, EXPF_ULP / DIV_ULP / LOGF_ULP as they stand, SAFETY once at the end, TINY wherever a result may fall under
the smallest normal.

  t   the two teacher distances' e_tri_dist, the rounding of + 1e5 where it applies (u |tn|), the subtraction (u |t|)
  q   e = expf(-t) moves by e (e_t + EXPF_ULP ulp) and reaches q = 1 / (1 + e) through e / (1 + e)^2 = q (1 - q); the
      addition and the division: q (u + DIV_ULP ulp)
  L   the student term is e_tri_loss; the cross term fl(fl(w q) z): |w z| e_q, two products (2 u |w q z|), end to end
      |w q| e_z; the subtraction u |L|; a flushed w q costs TINY |z|
  gz  s = ez / (1 + ez): s (EXPF_ULP ulp + u + DIV_ULP ulp), end to end s (1 - s) e_z;  fl(w q): w e_q + u w q;  the
      subtraction u |s - w q|; the product with dloss u |gz|
  df  b_tri_bwd on the sum of absolute terms, plus per term |f_i - f_o| / d x e_gz_i (absolute: gz may cancel to 0) and, end
      to end, |term| e_d / d"""
import numpy as np

import loss_ref as R
import loss_bounds as B
from loss_ref import triplet_dist, triplet_select, triplet_bwd, triplet_full                                   # noqa: F401
from loss_bounds import (in_triplet, tri_gap_ok, e_tri_dist, e_tri_z, e_tri_loss, b_tri_bwd, b_tri_dist,      # noqa: F401
                         triplet_dist_f32, TRI_CASES, TRI_IDS, TRI_CLASSES, U, ULP, SAFETY, TINY, EXPF_ULP, DIV_ULP,
                         LOGF_ULP, rng_for, f32, check, dump_ratios, RATIOS)
from head_ref import f64

F = np.float32
W_SOFT = (0.0, 0.8, 1.0)
ZERO = F(0.0)


def in_soft_triplet(n, D, cls, pattern):
    """in_triplet's student rows, ids and dloss plus the teacher's rows tf: standard normal, unrelated to the student's, so
    that q spreads over (0, 1) (a teacher at f + 0.02 N gives q in 0.48 .. 0.54 only) and the duplicated student rows of
    class (t) have different teacher rows: a wrong tie rule shows up in q."""
    d = in_triplet(n, D, cls, pattern)
    d['tf'] = f32(rng_for('softtri', n, D, cls, pattern, 'far').standard_normal((n, D)))
    return d


def w_of(w):
    """the weight as the kernel receives it"""
    return float(F(w))


def sigmoid(x):
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def softplus(z):
    z = np.asarray(z, np.float64)
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


# ----------------------------------------------------------------------------------------------------------------------
# the float64 model
def soft_triplet(tf, ids, sel, z, w, n, D, dloss=None, q=None):
    """The teacher part, the loss and gz in float64 AT A GIVEN selection and z (the kernel's fp32 ones stage-wise, the float64
    ones of triplet_full end to end).  q given: the loss and gz are evaluated on that q instead of the model's."""
    td = triplet_dist(tf, n, D)
    y = np.asarray(ids, np.int64).reshape(-1)[:n]
    sel = np.asarray(sel, np.int64).reshape(n, 2)
    r = np.arange(n)
    has_pos = sel[:, 0] >= 0
    jp, jn = np.maximum(sel[:, 0], 0), sel[:, 1]
    same_n = y[jn] == y
    tp = np.where(has_pos, td['dist'][r, jp], 0.0)
    tn = td['dist'][r, jn] + 1e5 * same_n
    t = tp - tn
    qm = sigmoid(t)
    qq = qm if q is None else f64(q).reshape(-1)
    zz = f64(z).reshape(-1)
    ww = w_of(w)
    out = dict(td=td, has_pos=has_pos, same_n=same_n, jp=jp, jn=jn, tp=tp, tn=tn, t=t, q_model=qm, q=qq, z=zz, w=ww,
               sp=softplus(zz), loss=softplus(zz) - ww * qq * zz)
    if dloss is not None:
        dl = f64(dloss).reshape(-1)[:n]
        sg = sigmoid(zz)
        out.update(dl=dl, sg=sg, gz=dl * (sg - ww * qq))
    return out


def soft_triplet_full(f, tf, ids, w, n, D, dloss):
    """End to end in float64: triplet_full's distances and selection, the teacher part at that selection, the gradient."""
    full = triplet_full(f, ids, n, D, 1, ZERO, dloss)
    m = soft_triplet(tf, ids, full['sel'], full['z'], w, n, D, dloss)
    bw = triplet_bwd(f, full['dist'], full['sel'], None, None, 1, ZERO, n, D, gz=m['gz'])
    return full, m, bw


# ----------------------------------------------------------------------------------------------------------------------
# bounds (no SAFETY inside the e_*; the b_* carry it)
def e_t(m, D):
    e_td = e_tri_dist(m['td'], D)
    r = np.arange(m['t'].size)
    e_p = np.where(m['has_pos'], e_td[r, m['jp']], 0.0)
    e_n = e_td[r, m['jn']] + np.where(m['same_n'], U * np.abs(m['tn']), 0.0)
    return e_p + e_n + U * np.abs(m['t'])


def e_q(m, D):
    q = m['q_model']
    return q * (1.0 - q) * (e_t(m, D) + EXPF_ULP * ULP) + q * (U + DIV_ULP * ULP) + TINY


def e_soft_loss(m, eq=0.0, e_z=0.0):
    """eq = 0: the loss given the q it read (stage-wise); e_z = 0: given the z it read"""
    z, q, w = m['z'], m['q'], m['w']
    cross = np.abs(w * z) * eq + 2 * U * np.abs(w * q * z) + np.abs(w * q) * e_z + TINY * np.abs(z)
    return e_tri_loss(z, 1, ZERO, e_z) + cross + U * np.abs(m['loss']) + TINY


def e_soft_gz(m, eq=0.0, e_z=0.0):
    sg, q, w, dl = m['sg'], m['q'], m['w'], m['dl']
    e_s = sg * (EXPF_ULP * ULP + U + DIV_ULP * ULP) + sg * (1.0 - sg) * e_z + TINY
    e_wq = w * eq + U * w * q + TINY
    return np.abs(dl) * (e_s + e_wq + U * np.abs(sg - w * q)) + U * np.abs(m['gz']) + TINY


def b_soft_bwd(bw, f, dist, sel, e_gz, n, D, e_dist=None):
    """b_tri_bwd's roundings of the terms and their sum, plus what every anchor's e_gz (absolute) and, end to end, its
    distances' errors move in the rows it touches"""
    f = f64(f).reshape(n, D)
    dist = f64(dist).reshape(n, n)
    sel = np.asarray(sel, np.int64).reshape(n, 2)
    gz = bw['gz']
    err = np.zeros((n, D))
    for i in range(n):
        for o in sel[i]:
            if o < 0:
                continue
            unit = np.abs(f[i] - f[o]) / dist[i, o]
            e = unit * e_gz[i]
            if e_dist is not None:
                e = e + unit * np.abs(gz[i]) * e_dist[i, o] / dist[i, o]
            err[i] += e
            if o != i:
                err[o] += e
    return b_tri_bwd(bw, 1) + SAFETY * err


# ----------------------------------------------------------------------------------------------------------------------
# fp32 restatement (numpy, CPU): the discrete and ordered parts in the kernels' order; numpy's exp / log stand in for the
# device's expf / logf
def triplet_bwd_f32(f, dist32, sel, gz32, n, D):
    """tri_bwd_rows: per row r the anchors in index order, within an anchor the positive term before the negative one"""
    f = F(f).reshape(n, D)
    d = F(dist32).reshape(n, n)
    sel = np.asarray(sel, np.int64).reshape(n, 2)
    gz = F(gz32).reshape(-1)
    df = np.zeros((n, D), F)
    for r in range(n):
        acc = np.zeros(D, F)
        for i in range(n):
            p, q = sel[i]
            if i == r:
                if p >= 0:
                    acc = acc + (f[r] - f[p]) * (gz[i] / d[i, p])
                acc = acc - (f[r] - f[q]) * (gz[i] / d[i, q])
            if p == r and i != r:
                acc = acc - (f[i] - f[r]) * (gz[i] / d[i, r])
            if q == r and i != r:
                acc = acc + (f[i] - f[r]) * (gz[i] / d[i, r])
        assert acc.dtype == F
        df[r] = acc
    return df


def soft_triplet_f32(f, tf, ids, dloss, w, n, D):
    d32 = triplet_dist_f32(f, n, D)
    s = triplet_select(d32, ids, n, 1, ZERO)
    sel, z = s['sel'], s['z']
    y = np.asarray(ids, np.int64).reshape(-1)[:n]
    dl = F(dloss).reshape(-1)[:n]
    wf = F(w)
    with np.errstate(over='ignore'):
        ez = np.exp(z)
        sp = np.log(F(1) + ez)
        sg = ez / (F(1) + ez)
        out = dict(dist=d32, sel=sel, z=z)
        if wf == 0:
            out.update(q=None, loss=sp, gz=dl * sg)
        else:
            td32 = triplet_dist_f32(tf, n, D)
            s2 = sel.reshape(n, 2)
            r = np.arange(n)
            jp, jn = np.maximum(s2[:, 0], 0), s2[:, 1]
            tp = np.where(s2[:, 0] >= 0, td32[r, jp], F(0))
            tn = td32[r, jn] + F(1e5) * (y[jn] == y).astype(F)
            t = tp - tn
            q = F(1) / (F(1) + np.exp(-t))
            wq = wf * q
            out.update(td=td32, q=q, loss=sp - wq * z, gz=dl * (sg - wq))
    for k in ('loss', 'gz'):
        assert out[k].dtype == F, k
    assert out['q'] is None or out['q'].dtype == F
    out['df'] = triplet_bwd_f32(f, d32, sel, out['gz'], n, D)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the checks both test files run: `got` holds fp32 dist [n][n], sel [2n], z [n], q [n] (None with w = 0), loss [n], df [n][D]
def check_stagewise(got, d, w, n, D, what):
    """Every stage against the float64 model evaluated on the fp32 values that stage read: q at got's sel; the loss on got's
    z and q; df on got's dist, sel, z and q."""
    zk, selk, dk = got['z'], got['sel'], got['dist']
    m = soft_triplet(d['tf'], d['ids'], selk, zk, w, n, D, d['dloss'])
    if w_of(w) != 0:
        check('soft triplet q', got['q'], m['q_model'], SAFETY * e_q(m, D), what)
        m = soft_triplet(d['tf'], d['ids'], selk, zk, w, n, D, d['dloss'], q=got['q'])
    check('soft triplet loss', got['loss'], m['loss'], SAFETY * e_soft_loss(m), what)
    bw = triplet_bwd(d['f'], dk, selk, None, None, 1, ZERO, n, D, gz=m['gz'])
    check('soft triplet dfeat', got['df'], bw['df'], b_soft_bwd(bw, d['f'], dk, selk, e_soft_gz(m), n, D), what)
    return m


def check_end_to_end(got, d, w, n, D, what, require_gap=True):
    """Nothing taken from the fp32 side: sel equals the float64 selection under the gap condition, the loss and df inside
    the bounds that carry the distances' errors through z and q.  Returns False (nothing compared) when the gap condition
    does not hold and is not required."""
    full, m, bw = soft_triplet_full(d['f'], d['tf'], d['ids'], w, n, D, d['dloss'])
    e_dist = e_tri_dist(full, D)
    ok = tri_gap_ok(full, e_dist)
    if not ok:
        assert not require_gap, what
        return False
    assert np.array_equal(got['sel'], full['sel']), what
    e_z = e_tri_z(full, e_dist)
    eq = e_q(m, D) if w_of(w) != 0 else 0.0
    check('end to end soft triplet loss', got['loss'], m['loss'], SAFETY * e_soft_loss(m, eq, e_z), what)
    if got.get('df') is not None:
        check('end to end soft triplet dfeat', got['df'], bw['df'],
              b_soft_bwd(bw, d['f'], full['dist'], full['sel'], e_soft_gz(m, eq, e_z), n, D, e_dist), what)
    return True
