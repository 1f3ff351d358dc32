"""Host model of the t-SNE contract in numpy, for the tests of engine.tsne / tsne_affinities /
tsne_gradient / tsne_from_affinities.  float32 operation by operation where the contract says bit for bit (``*32``), and
the same definitions in float64 without any prescribed order (``*64``).

THE WAVE ORDER of a sum over positions p = 0, 1, ..: 64 partial sums, partial l the sequential float32 sum from +0.0, in
ascending p, of the terms with p % 64 == l; then part[l] += part[l + s], l < s, for s = 32 .. 1 (silhouette_ref.tree).  A
term that is left out is skipped; a partial that starts at +0.0 is never -0.0, so adding +0.0 in its place gives the same
bits, which is what the vectorised ``wave_sum`` does.

Distance e(i, j): 'cosine' = hdbscan_ref.cosine_matrix (the symmetric chain), 'euclidean' = fl(s * s).  Neighbours: K =
min(n - 1, floor(3 * perplexity) + 1); row i of search's top-(K + 1) list on e (value with -0 == +0 and NaN last, then
index) with the entry of index i deleted, or the last entry if it is not there.  Conditional affinities: scikit-learn's
bisection on beta, on the distances less the list's first one: the same p and H, and float32's exp cannot underflow in
every term at once (``conditional32``).  A sample with a non-finite distance in its list is isolated.  Joint affinities:
P[i][j] = fl(fl(a + b) / float32(2 * n_live)) over the union pattern, pairs with an isolated end dropped.  Gradient, update
and KL: ``gradient32``, ``step32``, ``kl32``."""
import math

import numpy as np

import search_ref
import silhouette_ref as SR

F = np.float32


def n_neighbours(n, perplexity):
    return min(n - 1, int(math.floor(3.0 * perplexity)) + 1)


def wave_sum(terms):
    """[.., L] float32 terms in position order -> [..] float32 in the wave order."""
    terms = np.asarray(terms, dtype=F)
    L = terms.shape[-1]
    chunks = -(-L // 64) if L else 0
    part = np.zeros(terms.shape[:-1] + (64,), dtype=F)
    with np.errstate(invalid='ignore', over='ignore'):
        for c in range(chunks):
            seg = terms[..., 64 * c:64 * c + 64]
            part[..., :seg.shape[-1]] = part[..., :seg.shape[-1]] + seg
        return SR.tree(part)


def squared(euc):
    with np.errstate(invalid='ignore', over='ignore'):
        s = np.asarray(euc, dtype=F)
        return (s * s).astype(F)


def neighbours(e, K):
    """(idx int32 [n, K], dist float32 [n, K]) of the float32 [n, n] matrix e."""
    e = np.asarray(e, dtype=F)
    n = e.shape[0]
    comp = search_ref.composite(search_ref.sort_key(e), np.arange(n)[None, :])
    top = np.argsort(comp, axis=1, kind='stable')[:, :K + 1]
    idx = np.empty((n, K), dtype=np.int32)
    for i in range(n):
        row = top[i].tolist()
        if i in row:
            row.remove(i)
        else:
            row.pop()
        idx[i] = row
    return idx, np.take_along_axis(e, idx.astype(np.int64), 1)


def conditional32(e, perplexity):
    """(cond float32 [n, K], beta float32 [n], isolated bool [n], steps int [n]): the bisection in float32."""
    e = np.asarray(e, dtype=F)
    n, K = e.shape
    target = F(math.log(perplexity))
    isolated = ~np.isfinite(e).all(1)
    cond = np.zeros((n, K), dtype=F)
    used = np.full(n, np.nan, dtype=F)
    steps = np.zeros(n, dtype=np.int64)
    beta = np.ones(n, dtype=F)
    bmin = np.full(n, -np.inf, dtype=F)
    bmax = np.full(n, np.inf, dtype=F)
    active = ~isolated
    with np.errstate(all='ignore'):
        t = (e - e[:, :1]).astype(F)                             # less the list's first entry, its smallest
        for _ in range(100):
            r = np.flatnonzero(active)
            if r.size == 0:
                break
            b = beta[r]
            p = np.exp(-(t[r] * b[:, None]).astype(F)).astype(F)
            s = wave_sum(p)
            p = (p / s[:, None]).astype(F)
            h = (np.log(s).astype(F) + (b * wave_sum((t[r] * p).astype(F))).astype(F)).astype(F)
            diff = (h - target).astype(F)
            cond[r], used[r] = p, b
            steps[r] += 1
            done = np.abs(diff) <= F(1e-5)
            up = diff > 0
            lo_r, hi_r = r[up & ~done], r[~up & ~done]
            bmin[lo_r] = beta[lo_r]
            beta[lo_r] = np.where(np.isinf(bmax[lo_r]), beta[lo_r] * F(2.0), (beta[lo_r] + bmax[lo_r]) * F(0.5)).astype(F)
            bmax[hi_r] = beta[hi_r]
            beta[hi_r] = np.where(np.isinf(bmin[hi_r]), beta[hi_r] * F(0.5), (beta[hi_r] + bmin[hi_r]) * F(0.5)).astype(F)
            active[r[done]] = False
    return cond, used, isolated, steps


def conditional64(e, perplexity):
    """The same bisection in float64 on the float32 distances: (cond float64 [n, K], beta, isolated)."""
    e = np.asarray(e, dtype=np.float64)
    n, K = e.shape
    target = math.log(perplexity)
    isolated = ~np.isfinite(e).all(1)
    cond = np.zeros((n, K))
    used = np.full(n, np.nan)
    for i in np.flatnonzero(~isolated):
        beta, bmin, bmax = 1.0, -np.inf, np.inf
        for _ in range(100):
            t = e[i] - e[i, 0]
            p = np.exp(-t * beta)
            s = p.sum()
            p = p / s
            h = math.log(s) + beta * float((t * p).sum())
            cond[i], used[i] = p, beta
            diff = h - target
            if abs(diff) <= 1e-5:
                break
            if diff > 0:
                bmin = beta
                beta = beta * 2.0 if bmax == np.inf else (beta + bmax) / 2.0
            else:
                bmax = beta
                beta = beta / 2.0 if bmin == -np.inf else (beta + bmin) / 2.0
    return cond, used, isolated


def perplexity_of(cond):
    """2 ** entropy (base e: exp of the Shannon entropy) of every row of conditional probabilities, in float64."""
    p = np.asarray(cond, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.exp(-np.where(p > 0, p * np.log(p), 0.0).sum(1))


def _dense(idx, cond, isolated, dtype):
    n = idx.shape[0]
    a = np.zeros((n, n), dtype=dtype)
    m = np.zeros((n, n), dtype=bool)
    rows = np.repeat(np.arange(n), idx.shape[1])
    cols = np.asarray(idx, dtype=np.int64).ravel()
    keep = ~isolated[rows] & ~isolated[cols]
    a[rows[keep], cols[keep]] = np.asarray(cond, dtype=dtype).ravel()[keep]
    m[rows[keep], cols[keep]] = True
    return a, m


def joint32(idx, cond, isolated):
    """(row_ptr int64 [n + 1], col int32, val float32) of the joint affinities, columns ascending."""
    isolated = np.asarray(isolated, dtype=bool)
    a, m = _dense(idx, cond, isolated, F)
    den = F(2 * int((~isolated).sum()))
    val = ((a + a.T).astype(F) / den).astype(F)
    return to_csr(val, m | m.T)


def joint64(idx, cond, isolated):
    """The dense float64 P [n, n] and its pattern."""
    isolated = np.asarray(isolated, dtype=bool)
    a, m = _dense(idx, cond, isolated, np.float64)
    return (a + a.T) / (2.0 * int((~isolated).sum())), m | m.T


def to_csr(dense, mask):
    n = dense.shape[0]
    rows, cols = np.nonzero(mask)                            # row-major: columns ascend within a row
    row_ptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=n)))).astype(np.int64)
    return row_ptr, cols.astype(np.int32), dense[rows, cols]


def to_dense(row_ptr, col, val, dtype=np.float64):
    n = len(row_ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    p = np.zeros((n, n), dtype=dtype)
    p[rows, np.asarray(col, dtype=np.int64)] = np.asarray(val, dtype=dtype)
    return p


def _live(n, isolated):
    return np.ones(n, dtype=bool) if isolated is None else ~np.asarray(isolated, dtype=bool)


def _pairs32(y):
    y = np.asarray(y, dtype=F)
    with np.errstate(all='ignore'):
        dx = (y[:, None, :] - y[None, :, :]).astype(F)
        r = ((dx[..., 0] * dx[..., 0]).astype(F) + (dx[..., 1] * dx[..., 1]).astype(F)).astype(F)
        q = (F(1.0) / (F(1.0) + r).astype(F)).astype(F)
    return dx, q


def repulsion32(y, isolated=None):
    """(rep float32 [n, 2], rowz float32 [n], z float32): the exact repulsive term in the wave order over j."""
    n = y.shape[0]
    live = _live(n, isolated)
    dx, q = _pairs32(y)
    take = live[None, :] & ~np.eye(n, dtype=bool)
    with np.errstate(all='ignore'):
        qq = (q * q).astype(F)
        rep = np.stack([wave_sum(np.where(take, (qq * dx[..., c]).astype(F), F(0))) for c in (0, 1)], 1)
        rowz = wave_sum(np.where(take, q, F(0)))
    rep[~live] = 0
    rowz[~live] = 0
    return rep.astype(F), rowz.astype(F), wave_sum(rowz)


def _padded_rows(row_ptr, col, val):
    """The CSR rows side by side: (cols int64 [n, L], vals float32 [n, L], present bool [n, L]), place = position in the row."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    n = row_ptr.size - 1
    lens = np.diff(row_ptr)
    L = int(lens.max()) if n and lens.size else 0
    place = np.arange(max(L, 1))[None, :]
    present = place < lens[:, None]
    at = np.where(present, row_ptr[:-1, None] + place, 0)
    col, val = np.asarray(col, dtype=np.int64), np.asarray(val, dtype=F)
    if col.size == 0:
        return np.zeros_like(at), np.zeros(at.shape, dtype=F), present
    return col[at], val[at], present


def gradient32(row_ptr, col, val, y, alpha=1.0, isolated=None):
    """(grad float32 [n, 2], z float32) at y, bit for bit the contract's gradient."""
    y = np.asarray(y, dtype=F)
    n = y.shape[0]
    live = _live(n, isolated)
    rep, _, z = repulsion32(y, isolated)
    cols, vals, present = _padded_rows(row_ptr, col, val)
    take = present & live[cols]
    with np.errstate(all='ignore'):
        dx = (y[:, None, :] - y[cols]).astype(F)
        r = ((dx[..., 0] * dx[..., 0]).astype(F) + (dx[..., 1] * dx[..., 1]).astype(F)).astype(F)
        q = (F(1.0) / (F(1.0) + r).astype(F)).astype(F)
        w = ((F(alpha) * vals).astype(F) * q).astype(F)
        att = np.stack([wave_sum(np.where(take, (w * dx[..., c]).astype(F), F(0))) for c in (0, 1)], 1)
        grad = (F(4.0) * (att - (rep / z).astype(F)).astype(F)).astype(F)
    grad[~live] = 0
    return grad, z


def gradient64(p, y, alpha=1.0, isolated=None):
    """(grad float64 [n, 2], z) of a dense float64 P at y."""
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    live = _live(n, isolated)
    d0, d1 = y[:, None, 0] - y[None, :, 0], y[:, None, 1] - y[None, :, 1]
    take = live[None, :] & live[:, None] & ~np.eye(n, dtype=bool)
    q = np.where(take, 1.0 / (1.0 + d0 * d0 + d1 * d1), 0.0)
    z = q.sum()
    w = alpha * np.where(take, p, 0.0) * q - q * q / z
    return 4.0 * np.stack(((w * d0).sum(1), (w * d1).sum(1)), 1), z


def step32(y, update, gains, grad, momentum, lr, isolated=None):
    """One update, elementwise in float32: (y, update, gains) after it."""
    y, update, gains, grad = (np.asarray(a, dtype=F) for a in (y, update, gains, grad))
    live = _live(y.shape[0], isolated)[:, None]
    with np.errstate(all='ignore'):
        inc = (update * grad).astype(F) < 0
        g = np.where(inc, (gains + F(0.2)).astype(F), (gains * F(0.8)).astype(F)).astype(F)
        g = np.where(g < F(0.01), F(0.01), g).astype(F)
        u = ((F(momentum) * update).astype(F) - (F(lr) * (g * grad).astype(F)).astype(F)).astype(F)
        ny = (y + u).astype(F)
    return np.where(live, ny, y), np.where(live, u, update), np.where(live, g, gains)


def schedule(it, early_exaggeration=12.0, exaggeration_iter=250):
    """(alpha, momentum) of iteration ``it`` (0-based)."""
    return (early_exaggeration, 0.5) if it < exaggeration_iter else (1.0, 0.8)


def auto_learning_rate(n_live, early_exaggeration=12.0):
    return max(n_live / early_exaggeration / 4.0, 50.0)


def init_random(n, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    return g.standard_normal((n, 2)).astype(F) * F(1e-4)


def run32(row_ptr, col, val, y, n_iter, lr, early_exaggeration=12.0, exaggeration_iter=250, isolated=None, first=0,
          update=None, gains=None):
    """``n_iter`` iterations first, first + 1, ..: (y, update, gains) in float32, bit for bit the device's loop."""
    y = np.asarray(y, dtype=F).copy()
    update = np.zeros_like(y) if update is None else np.asarray(update, dtype=F)
    gains = np.ones_like(y) if gains is None else np.asarray(gains, dtype=F)
    for it in range(first, first + n_iter):
        alpha, momentum = schedule(it, early_exaggeration, exaggeration_iter)
        grad, _ = gradient32(row_ptr, col, val, y, alpha, isolated)
        y, update, gains = step32(y, update, gains, grad, momentum, lr, isolated)
    return y, update, gains


def run64(p, y, n_iter, lr, early_exaggeration=12.0, exaggeration_iter=250, isolated=None):
    """The same loop in float64 on a dense P: the final y."""
    y = np.asarray(y, dtype=np.float64).copy()
    update, gains = np.zeros_like(y), np.ones_like(y)
    live = _live(y.shape[0], isolated)[:, None]
    for it in range(n_iter):
        alpha, momentum = schedule(it, early_exaggeration, exaggeration_iter)
        grad, _ = gradient64(p, y, alpha, isolated)
        inc = update * grad < 0
        g = np.maximum(np.where(inc, gains + 0.2, gains * 0.8), 0.01)
        u = momentum * update - lr * (g * grad)
        y, update, gains = np.where(live, y + u, y), np.where(live, u, update), np.where(live, g, gains)
    return y


def kl32(row_ptr, col, val, y, isolated=None):
    """The KL divergence as the device evaluates it: float32 per-row sums in the wave order of P * log(P Z / q), the
    logarithm of the float32 quotient taken in float64 and rounded to float32; float64 over the rows."""
    y = np.asarray(y, dtype=F)
    n = y.shape[0]
    live = _live(n, isolated)
    _, _, z = repulsion32(y, isolated)
    cols, vals, present = _padded_rows(row_ptr, col, val)
    take = present & live[cols] & live[:, None] & (vals > 0)
    with np.errstate(all='ignore'):
        dx = (y[:, None, :] - y[cols]).astype(F)
        r = ((dx[..., 0] * dx[..., 0]).astype(F) + (dx[..., 1] * dx[..., 1]).astype(F)).astype(F)
        q = (F(1.0) / (F(1.0) + r).astype(F)).astype(F)
        term = (vals * np.log(((vals * z).astype(F) / q).astype(F).astype(np.float64)).astype(F)).astype(F)
        rows = wave_sum(np.where(take, term, F(0)))
    return float(rows.astype(np.float64).sum())


def kl64(p, y, isolated=None):
    """sum over P > 0 of P log(P Z / q) in float64 on a dense P."""
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    live = _live(n, isolated)
    dx = y[:, None, :] - y[None, :, :]
    q = 1.0 / (1.0 + (dx ** 2).sum(2))
    take = live[None, :] & live[:, None] & ~np.eye(n, dtype=bool)
    z = np.where(take, q, 0.0).sum()
    use = take & (p > 0)
    return float((p[use] * np.log(p[use] * z / q[use])).sum())
