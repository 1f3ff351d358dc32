"""The numpy model of engine.pca's contract, parametrised by dtype: the same steps in the same order --
mean, host-drawn start, CholeskyQR2 with the kernel's summation orders and pivot record, the power iteration with both
halves orthonormalised and the centring as rank-one terms, Rayleigh-Ritz, the sign rule, the total variance.  What it
does NOT mirror is the k-order of the MFMA GEMMs (numpy's dot stands in) and the Jacobi kernel (LAPACK's eigh stands in
inside ``model``; ``jacobi`` below is the kernel's algorithm on its own).  ``exact`` is the PCA by LAPACK's SVD in
float64, the yardstick of the well-separated cases."""
import numpy as np

PIVOT_SMALL, PIVOT_NONFINITE = 1, 2
MAX_SWEEPS = 30

# (n, d, k, decay, r, p, unit rows): the smallest shapes that straddle the wave width (64), the GEMMs' 32-column padding and
# the 32-wide LDS panel of the Cholesky and solve kernels.  A: r <= k, gaps >= 1.4e-2; B: r > k, the tail is noise.
CASES = {
    'A1': (65, 33, 6, 0.7, 6, 10, False),
    'A2': (257, 70, 12, 0.8, 8, 10, False),
    'B1': (129, 200, 40, 0.93, 54, 10, False),
    'B2': (300, 96, 48, 0.95, 55, 10, True),
    'B3': (600, 160, 100, 0.97, 120, 10, False),
}


def planted(n, d, k, decay, unit=False, noise=0.02, seed=1):
    """float32 [n, d]: k orthonormal directions with latent scales decay**i, noise * N(0, 1) added, offset +0.5."""
    g = np.random.Generator(np.random.PCG64(seed))
    basis = np.linalg.qr(g.standard_normal((d, k)))[0].T
    latent = g.standard_normal((n, k)) * decay ** np.arange(k)
    x = latent @ basis + noise * g.standard_normal((n, d)) + 0.5
    if unit:
        x = x / np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x.astype(np.float32))


_cache = {}


def case(name):
    """(x float32 [n, d], r, p) of a named case, built once."""
    if name not in _cache:
        n, d, k, decay, r, p, unit = CASES[name]
        x = planted(n, d, k, decay, unit)
        x.setflags(write=False)
        _cache[name] = (x, r, p)
    return _cache[name]


def start(L, d, seed):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((L, d)).astype(np.float32)


def pivot_tol(L):
    return float(L) * 2.0 ** -23


def new_record():
    return {'min_pivot': np.inf, 'status': 0, 'index': -1, 'call': -1, 'calls': 0}


def cholesky(g, dtype, rec, rel_tol=None):
    """The lower factor R of g = R R^T as grl_pca_cholesky computes it: R[i][k] = (g[i][k] - sum_{j<k} R[i][j] R[k][j]) /
    R[k][k], every sum term by term in ascending j (the outer-product form below subtracts the same terms in the same
    order).  A pivot that is not finite or not > rel_tol * g[k][k] ends it: the identity from that column on."""
    a = np.array(g, dtype=dtype)
    L = a.shape[0]
    rel_tol = pivot_tol(L) if rel_tol is None else rel_tol
    dmax = dtype(np.nanmax(np.diag(a))) if not np.all(np.isnan(np.diag(a))) else dtype(-np.inf)
    diag = np.diag(a).copy()
    out = np.zeros((L, L), dtype)
    smin, bad, badk = np.inf, 0, -1
    with np.errstate(all='ignore'):
        for k in range(L):
            piv = a[k, k]
            fin = bool(np.isfinite(piv) and np.isfinite(dmax))
            if fin and dmax > 0:
                smin = min(smin, float(dtype(piv / dmax)))
            if not (fin and piv > 0 and piv > dtype(rel_tol) * diag[k]):
                bad, badk = (PIVOT_SMALL if fin else PIVOT_NONFINITE), k
                break
            r = np.sqrt(piv)
            out[k, k] = r
            col = a[k + 1:, k] / r
            out[k + 1:, k] = col
            a[k + 1:, k + 1:] -= np.outer(col, col)
    if bad:
        for k in range(badk, L):
            out[k:, k] = 0
            out[k, k] = 1
    rec['min_pivot'] = min(rec['min_pivot'], smin)
    if rec['status'] == 0 and bad:
        rec['status'], rec['index'], rec['call'] = bad, badk, rec['calls']
    rec['calls'] += 1
    return out


def trsm(r, w, dtype):
    """R^-1 w by forward substitution, y_i = (w_i - sum_{k<i} R[i][k] y_k) / R[i][i] in ascending k (grl_pca_trsm)."""
    y = np.array(w, dtype=dtype)
    with np.errstate(all='ignore'):
        for k in range(y.shape[0]):
            y[k] = y[k] / r[k, k]
            y[k + 1:] -= np.outer(r[k + 1:, k], y[k])
    return y


def orthonormalize(w, dtype, rec):
    """CholeskyQR2 on the rows of w."""
    w = np.array(w, dtype=dtype)
    for _ in range(2):
        with np.errstate(all='ignore'):
            g = w @ w.T
        w = trsm(cholesky(g, dtype, rec), w, dtype)
    return w


def sign_fix(c):
    """Each row times -1 when its entry of largest magnitude (the lowest column among equals) is negative."""
    c = np.array(c)
    for i in range(c.shape[0]):
        j = int(np.argmax(np.abs(c[i])))           # (argmax returns the first of equals)
        if c[i, j] < 0:
            c[i] = -c[i]
    return c


def model(x, r, p=10, q=4, seed=0, dtype=np.float64):
    """The contract in ``dtype``.  Returns a dict: mean, components [r, d], explained_variance [r], total_variance,
    explained_variance_ratio, record (the sticky pivot record), b (the Rayleigh-Ritz matrix), q (the final basis)."""
    x = np.asarray(x, dtype=dtype)
    n, d = x.shape
    L = r + p
    rec = new_record()
    mu = (x.sum(axis=0) / dtype(n)).astype(dtype)
    qm = orthonormalize(start(L, d, seed).astype(dtype), dtype, rec)

    def project(qm):
        with np.errstate(all='ignore'):
            return (x @ qm.T + (-(mu @ qm.T))[None, :]).astype(dtype)

    for _ in range(q):
        zt = orthonormalize(project(qm).T, dtype, rec)
        with np.errstate(all='ignore'):
            qm = (zt @ x - np.outer(zt.sum(axis=1), mu)).astype(dtype)
        qm = orthonormalize(qm, dtype, rec)
    z = project(qm)
    with np.errstate(all='ignore'):
        b = ((z.T @ z) * (dtype(1) / dtype(n - 1))).astype(dtype)
    out = {'mean': mu, 'record': rec, 'b': b, 'q': qm}
    if rec['status'] or not np.all(np.isfinite(b)):
        return out
    lam, v = np.linalg.eigh(b)
    order = np.argsort(-lam, kind='stable')
    lam, v = lam[order], v[:, order]
    comps = sign_fix((v.T[:r] @ qm).astype(dtype))
    total = (dtype((x * x).sum()) - dtype(n) * dtype((mu * mu).sum())) / dtype(n - 1)
    out.update(components=comps, explained_variance=lam[:r].astype(dtype), total_variance=float(total),
               explained_variance_ratio=(lam[:r] * (dtype(1) / dtype(total))).astype(dtype))
    return out


def exact(x):
    """PCA by LAPACK's SVD in float64: mean, components [min(n, d), d] (sign rule applied), explained_variance,
    total_variance, cov (the sample covariance [d, d])."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    mu = x.mean(axis=0)
    xc = x - mu
    _, s, vt = np.linalg.svd(xc, full_matrices=False)
    lam = s * s / (n - 1)
    return {'mean': mu, 'components': sign_fix(vt), 'explained_variance': lam, 'total_variance': float(lam.sum()),
            'cov': xc.T @ xc / (n - 1)}


def residual(cov, comps, lam):
    """max_i |cov c_i - lam_i c_i|_2 / lam_1 in float64."""
    c = np.asarray(comps, np.float64)
    lam = np.asarray(lam, np.float64)
    return float(np.linalg.norm(c @ cov - lam[:, None] * c, axis=1).max() / lam[0])


def transform(x, mu, comps, lam=None):
    """(x - mu) C^T in float64, column i over sqrt(lam_i) when lam is given."""
    y = (np.asarray(x, np.float64) - np.asarray(mu, np.float64)) @ np.asarray(comps, np.float64).T
    return y / np.sqrt(np.asarray(lam, np.float64)) if lam is not None else y


def tsne_init(y):
    """scikit-learn's init='pca' scaling (sklearn/manifold/_t_sne.py: X_embedded / np.std(X_embedded[:, 0]) * 1e-4)."""
    y = np.asarray(y)[:, :2]
    return y / np.std(y[:, 0]) * 1e-4


def round_robin(L):
    """The pairing of grl_pca_eigh: rounds of disjoint pairs (p < q) by the circle method on ne = L (+1 when odd)
    players; a pair with the extra player is left out."""
    ne = L + (L & 1)
    rounds = []
    for r in range(ne - 1):
        pairs = []
        for k in range(ne // 2):
            a = ne - 1 if k == 0 else (r + k) % (ne - 1)
            b = r if k == 0 else (r + ne - 1 - k) % (ne - 1)
            if max(a, b) < L:
                pairs.append((min(a, b), max(a, b)))
        rounds.append(pairs)
    return rounds


def jacobi(b, dtype=np.float32):
    """grl_pca_eigh's algorithm: (lam descending, v with columns the eigenvectors, sweeps, off, fro)."""
    a = np.array(b, dtype=dtype)
    L = a.shape[0]
    a = np.triu(a) + np.triu(a, 1).T
    vt = np.eye(L, dtype=dtype)
    fro = np.sqrt(dtype((a * a).sum()))
    thr = fro * dtype(2.0 ** -26) / dtype(L)
    rounds = round_robin(L)
    sweeps = 0
    with np.errstate(all='ignore'):
        for _ in range(MAX_SWEEPS):
            rotated = False
            for pairs in rounds:
                if not pairs:
                    continue
                p = np.array([pq[0] for pq in pairs])
                q = np.array([pq[1] for pq in pairs])
                apq = a[p, q]
                go = (np.abs(apq) > thr) & np.isfinite(apq)
                if not go.any():
                    continue
                rotated = True
                p, q, apq = p[go], q[go], apq[go]
                app, aqq = a[p, p], a[q, q]
                theta = (aqq - app) / (dtype(2) * apq)
                t = np.copysign(dtype(1), theta) / (np.abs(theta) + np.sqrt(theta * theta + dtype(1)))
                c = dtype(1) / np.sqrt(t * t + dtype(1))
                s = t * c
                tau = s / (dtype(1) + c)
                for m in (a, vt):
                    xp, xq = m[p].copy(), m[q].copy()
                    m[p] = xp - s[:, None] * (xq + tau[:, None] * xp)
                    m[q] = xq + s[:, None] * (xp - tau[:, None] * xq)
                xp, xq = a[:, p].copy(), a[:, q].copy()
                a[:, p] = xp - s[None, :] * (xq + tau[None, :] * xp)
                a[:, q] = xq + s[None, :] * (xp - tau[None, :] * xq)
                a[p, p], a[q, q] = app - t * apq, aqq + t * apq
                a[p, q] = a[q, p] = 0
            if not rotated:
                break
            sweeps += 1
    lam = np.diag(a).copy()
    off = np.sqrt(dtype(((a - np.diag(lam)) ** 2).sum()))
    key = np.where(np.isnan(lam), -np.inf, lam)
    order = np.argsort(-key, kind='stable')
    return lam[order], vt[order].T.copy(), sweeps, float(off), float(fro)
