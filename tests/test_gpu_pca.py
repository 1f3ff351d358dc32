"""engine.pca / pca_eigh / pca_orthonormalize on the device against the numpy model of the contract (tests/pca_ref.py)
and LAPACK.

THE TOLERANCE RULE of every float comparison here: |device - yardstick| <= max(16 * max|float32 model - yardstick|,
(d + L) * 2^-24 * scale).  The yardstick is the float64 model or LAPACK in float64, never the code under test; the first
term is what the same algorithm loses in fp32 (the factor 16 covers the MFMA k-order of the GEMMs and Jacobi in place
of LAPACK, neither of which the model has), the floor is the worst-case fp32 dot product of the length in play (the
form of test_gpu_kmeans.py); scale = lambda_1 for variances and entries of B, 1 for unit vectors and ratios.  Every
test prints the ratio error / bound it measured."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import pca_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
F, D = np.float32, np.float64
EPS = 2.0 ** -24

_cache = {}


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)              # (a copy: the shared cases are read-only arrays)


def host(t):
    return t.cpu().numpy()


def bits(t):
    return np.ascontiguousarray(host(t) if torch.is_tensor(t) else t, dtype=np.float32).view(np.uint32)


def bound(model32, yard, length, scale):
    """the rule's bound for one quantity: ``model32`` and ``yard`` are the float32 model's and the yardstick's values"""
    return max(16.0 * float(np.max(np.abs(np.asarray(model32, D) - np.asarray(yard, D)))), length * EPS * scale)


def check(name, got, yard, tol):
    err = float(np.max(np.abs(np.asarray(got, D) - np.asarray(yard, D))))
    print('%-34s err %.3e  bound %.3e  ratio %.3f' % (name, err, tol, err / tol))
    assert err <= tol, '%s: error %g above the bound %g' % (name, err, tol)


def fitted(name):
    """(x, r, p, exact, model64, model32, device fit) of a named case, computed once and left unchanged."""
    from grl_amd import engine
    if name not in _cache:
        x, r, p = R.case(name)
        _cache[name] = (x, r, p, R.exact(x), R.model(x, r, p, dtype=D), R.model(x, r, p, dtype=F),
                        engine.pca(dev(x), r, p))
    return _cache[name]


# ----------------------------------------------------------------------------
# 1. pca_eigh
# ----------------------------------------------------------------------------
def planted_spectrum(L, seed=3):
    """B = V diag(lam) V^T in float64, rounded: a repeated pair on top, a 1e-6 lambda_1 tail, a zero."""
    g = np.random.Generator(np.random.PCG64(seed + L))
    lam = np.sort(g.uniform(0.1, 1.0, L))[::-1].copy()
    if L >= 3:
        lam[1] = lam[0]
    if L >= 16:
        lam[3 * L // 4:] = 1e-6 * lam[0] * g.uniform(0.5, 1.0, L - 3 * L // 4)
    if L >= 2:
        lam[-1] = 0.0
    v = np.linalg.qr(g.standard_normal((L, L)))[0]
    return ((v * lam) @ v.T).astype(F)


def check_eigh(b, lam, v, sweeps):
    L = b.shape[0]
    b64 = b.astype(D)
    want = np.linalg.eigvalsh(b64)[::-1]
    l32, v32 = np.linalg.eigh(b)
    l32, v32 = l32[::-1].astype(D), v32[:, ::-1].astype(D)
    l1 = max(abs(want[0]), abs(want[-1]))
    lam, v = host(lam).astype(D), host(v).astype(D)
    assert lam.shape == (L,) and v.shape == (L, L) and np.all(np.diff(lam) <= 0)
    assert 0 <= sweeps < 30
    check('eigh L=%d eigenvalues' % L, lam, want, bound(l32, want, 2 * L, l1))
    res32 = np.abs(b64 @ v32 - v32 * l32).max()
    check('eigh L=%d |BV - V lam|' % L, np.abs(b64 @ v - v * lam).max(), 0.0, bound(res32, 0.0, 2 * L, l1))
    orth32 = np.abs(v32.T @ v32 - np.eye(L)).max()
    check('eigh L=%d |V^T V - I|' % L, np.abs(v.T @ v - np.eye(L)).max(), 0.0, bound(orth32, 0.0, 2 * L, 1.0))


@pytest.mark.parametrize('L', [1, 2, 3, 16, 63, 64, 65, 130])
def test_eigh_against_float64_lapack(L):
    from grl_amd import engine
    b = planted_spectrum(L)
    lam, v, sweeps = engine.pca_eigh(dev(b))
    print('L = %d: %d sweeps' % (L, sweeps))
    check_eigh(b, lam, v, sweeps)
    lam2, v2, sweeps2 = engine.pca_eigh(dev(b))
    assert sweeps2 == sweeps and np.array_equal(bits(lam), bits(lam2)) and np.array_equal(bits(v), bits(v2))


def test_eigh_at_the_largest_size():
    from grl_amd import engine
    b = planted_spectrum(512)
    lam, v, sweeps = engine.pca_eigh(dev(b))
    print('L = 512: %d sweeps' % sweeps)
    check_eigh(b, lam, v, sweeps)


def test_eigh_of_a_diagonal_matrix_takes_no_rotation():
    from grl_amd import engine
    g = np.random.Generator(np.random.PCG64(9))
    diag = g.standard_normal(65).astype(F)
    diag[7] = diag[40]                                         # equal values: the lower index first
    lam, v, sweeps = engine.pca_eigh(dev(np.diag(diag)))
    order = np.argsort(-diag, kind='stable')
    assert sweeps == 0 and np.array_equal(bits(lam), bits(diag[order]))
    want = np.zeros((65, 65), F)
    want[order, np.arange(65)] = 1.0
    assert np.array_equal(host(v), want)
    lam, v, sweeps = engine.pca_eigh(dev(np.array([[-2.5]], F)))
    assert sweeps == 0 and host(lam).tolist() == [-2.5] and host(v).tolist() == [[1.0]]


# ----------------------------------------------------------------------------
# 2. pca_orthonormalize
# ----------------------------------------------------------------------------
def gaussian_rows(L, m):
    g = np.random.Generator(np.random.PCG64(100 * L + m))
    return (g.standard_normal((L, m)) * 0.9 ** np.arange(L)[:, None]).astype(F)


ORTH_SHAPES = [(L, m) for L in (1, 2, 18, 64, 65, 130) for m in (33, 70, 257, 1025) if L <= m]


@pytest.mark.parametrize('L,m', ORTH_SHAPES)
def test_orthonormalize_against_the_model(L, m):
    from grl_amd import engine
    w = gaussian_rows(L, m)
    res = engine.pca_orthonormalize(dev(w))
    q, min_pivot = res
    assert res.status == 0 and res.index == -1 and tuple(q.shape) == (L, m)
    q = host(q).astype(D)
    w64 = w.astype(D)
    r64, r32 = R.new_record(), R.new_record()
    R.orthonormalize(w, D, r64)
    q32 = R.orthonormalize(w, F, r32).astype(D)
    eye = np.eye(L)
    check('orth %dx%d |QQ^T - I|' % (L, m), np.abs(q @ q.T - eye).max(), 0.0,
          bound(np.abs(q32 @ q32.T - eye).max(), 0.0, m + L, 1.0))
    scale = np.linalg.norm(w64, axis=1).max()                  # (a row's residual is relative to the row's length)
    check('orth %dx%d |W - (WQ^T)Q|' % (L, m), np.abs(w64 - (w64 @ q.T) @ q).max(), 0.0,
          bound(np.abs(w64 - (w64 @ q32.T) @ q32).max(), 0.0, m + L, scale))
    check('orth %dx%d min_pivot' % (L, m), min_pivot, r64['min_pivot'], bound(r32['min_pivot'], r64['min_pivot'], m + L, 1.0))
    again = engine.pca_orthonormalize(dev(w))
    assert np.array_equal(bits(again[0]), bits(res[0])) and again[1] == min_pivot


def test_orthonormalize_records_a_duplicated_row_and_returns():
    from grl_amd import engine
    w = gaussian_rows(18, 70)
    w[11] = w[4]
    res = engine.pca_orthonormalize(dev(w))
    q, min_pivot = res
    q = host(q)
    print('duplicated row: status %r, pivot %d of call %d, min_pivot %.3e' % (res.status, res.index, res.call, min_pivot))
    assert res.status == 'small' and (res.index, res.call) == (11, 0) and min_pivot <= R.pivot_tol(18)
    assert np.all(np.isfinite(q))
    head = q[:11].astype(D)
    assert np.abs(head @ head.T - np.eye(11)).max() <= 88 * EPS          # the rows before it are orthonormal
    rec = R.new_record()
    R.orthonormalize(w, F, rec)
    assert (rec['status'], rec['index'], rec['call']) == (R.PIVOT_SMALL, 11, 0)
    # ... and the device is fine afterwards
    assert engine.pca_orthonormalize(dev(gaussian_rows(2, 33))).status == 0


# ----------------------------------------------------------------------------
# 3. engine.pca
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['A1', 'A2'])
def test_separated_cases_against_the_exact_pca(name):
    from grl_amd import engine
    x, r, p, ex, m64, m32, fit = fitted(name)
    n, d = x.shape
    L = r + p
    xd = dev(x)
    mean = engine.cluster_centroids(xd, torch.zeros(n, dtype=torch.int64, device=DEV), 1, 'mean')[0][0]
    assert np.array_equal(bits(fit.mean), bits(mean))
    l1 = ex['explained_variance'][0]
    assert tuple(fit.components.shape) == (r, d) and tuple(fit.explained_variance.shape) == (r,)
    check(name + ' eigenvalues', host(fit.explained_variance), ex['explained_variance'][:r],
          bound(m32['explained_variance'], ex['explained_variance'][:r], d + L, l1))
    comps = host(fit.components)
    for i in range(r):                                         # every component, none left out
        check(name + ' component %d' % i, comps[i], ex['components'][i],
              bound(m32['components'][i], ex['components'][i], d + L, 1.0))
    assert np.array_equal(comps, R.sign_fix(comps))
    j = np.argmax(np.abs(comps), axis=1)
    assert np.all(comps[np.arange(r), j] > 0)
    check(name + ' total_variance', fit.total_variance, ex['total_variance'],
          bound(m32['total_variance'], ex['total_variance'], d + L, l1))
    ratio = ex['explained_variance'][:r] / ex['total_variance']
    check(name + ' explained_variance_ratio', host(fit.explained_variance_ratio), ratio,
          bound(m32['explained_variance_ratio'], ratio, d + L, 1.0))
    assert (fit.n_samples, fit.n_iter, fit.seed, fit.oversample) == (n, 4, 0, p) and 0 < fit.sweeps < 30
    check(name + ' min_pivot', fit.min_pivot, m64['record']['min_pivot'],
          bound(m32['record']['min_pivot'], m64['record']['min_pivot'], d + L, 1.0))


@pytest.mark.parametrize('name', ['B1', 'B2', 'B3'])
def test_noise_tail_cases_against_the_float64_model(name):
    x, r, p, ex, m64, m32, fit = fitted(name)
    n, d = x.shape
    L = r + p
    l1 = m64['explained_variance'][0]
    lam = host(fit.explained_variance).astype(D)
    check(name + ' eigenvalues', lam, m64['explained_variance'], bound(m32['explained_variance'], m64['explained_variance'], d + L, l1))
    comps = host(fit.components).astype(D)
    res64, res32 = (R.residual(ex['cov'], m['components'], m['explained_variance']) for m in (m64, m32))
    got = R.residual(ex['cov'], comps, lam)
    tol = bound(res32, res64, d + L, 1.0)
    print('%-34s device %.3e  model %.3e  slack %.3e' % (name + ' residual / lambda_1', got, res64, tol))
    assert got <= res64 + tol
    c32 = m32['components'].astype(D)
    check(name + ' |CC^T - I|', np.abs(comps @ comps.T - np.eye(r)).max(), 0.0,
          bound(np.abs(c32 @ c32.T - np.eye(r)).max(), 0.0, d + L, 1.0))
    check(name + ' sum of eigenvalues', lam.sum(), m64['explained_variance'].sum(),
          bound(m32['explained_variance'].astype(D).sum(), m64['explained_variance'].sum(), d + L, l1))
    assert np.all(np.diff(lam) <= 0) and 0 < fit.sweeps < 30
    print('%s: %d sweeps, min_pivot %.3e (model %.3e)' % (name, fit.sweeps, fit.min_pivot, m64['record']['min_pivot']))


@pytest.mark.parametrize('name', ['A1', 'B2'])
def test_transform_is_the_gemm_and_follows_float64(name):
    from grl_amd import engine
    x, r, p, ex, m64, m32, fit = fitted(name)
    n, d = x.shape
    L = r + p
    xd = dev(x)
    mu, comps, lam = host(fit.mean), host(fit.components), host(fit.explained_variance)
    for whiten in (False, True):
        y = fit.transform(xd, whiten)
        assert tuple(y.shape) == (n, r) and y.dtype == torch.float32
        scale, shift = fit.affine(whiten)
        xp = engine._pad_features(xd)
        cp = engine._pad_features(fit.components)
        want = torch.empty_like(y)
        engine.gemm(xp, cp, want, n, r, xp.shape[1], scale=scale, shift=shift, math=engine.MATH_F32)
        assert np.array_equal(bits(y), bits(want))
        # against the float64 transform by the device's own mean, components and variances; the float32 model of the same
        s64 = 1.0 / np.sqrt(lam.astype(D)) if whiten else np.ones(r)
        y64 = R.transform(x, mu, comps, lam if whiten else None)
        with np.errstate(all='ignore'):
            s32 = (F(1) / np.sqrt(lam)) if whiten else np.ones(r, F)
            y32 = (x @ comps.T) * s32 + (-((mu @ comps.T) * s32))
        ymax = np.abs(y64).max()
        check('%s transform whiten=%d' % (name, whiten), host(y), y64, bound(y32, y64, d + L, ymax))
        check('%s scale whiten=%d' % (name, whiten), host(scale), s64, bound(s32, s64, d + L, s64.max()))
        if whiten:
            cov = np.cov(host(y).astype(D), rowvar=False)
            c32, mu32, l32 = m32['components'], m32['mean'], m32['explained_variance']
            with np.errstate(all='ignore'):
                w32 = F(1) / np.sqrt(l32)
                cov32 = np.cov(((x @ c32.T) * w32 + (-((mu32 @ c32.T) * w32))).astype(D), rowvar=False)
            check(name + ' covariance of the whitened transform', cov, np.eye(r), bound(cov32, np.eye(r), n + L, 1.0))
    # rows that were not in the fit, fewer than a tile and none at all
    g = np.random.Generator(np.random.PCG64(4))
    other = g.standard_normal((37, d)).astype(F)
    y = fit.transform(dev(other))
    y64 = R.transform(other, mu, comps)
    check(name + ' transform of other rows', host(y), y64, bound((other @ comps.T) + (-(mu @ comps.T)), y64, d + L, np.abs(y64).max()))
    assert tuple(fit.transform(dev(other[:0])).shape) == (0, r)


def test_inverse_transform_reconstructs():
    x, r, p, ex, m64, m32, fit = fitted('A1')
    n, d = x.shape
    xd = dev(x)
    for whiten in (False, True):
        back = host(fit.inverse_transform(fit.transform(xd, whiten), whiten))
        assert back.shape == (n, d)
        rec64 = R.transform(x, m64['mean'], m64['components']) @ m64['components'] + m64['mean']
        c32, mu32 = m32['components'], m32['mean']
        rec32 = ((x @ c32.T) + (-(mu32 @ c32.T))) @ c32 + mu32
        check('A1 reconstruction whiten=%d' % whiten, back, rec64, bound(rec32, rec64, d + r + p, np.abs(x).max()))
        # the reconstruction error itself is the model's: the variance outside the r kept components
        err, err64 = np.abs(back.astype(D) - x).max(), np.abs(rec64 - x).max()
        assert err <= err64 + bound(rec32, rec64, d + r + p, np.abs(x).max())


def test_tsne_init_scaling_and_use():
    from grl_amd import engine
    x, r, p, ex, m64, m32, fit = fitted('A2')
    n, d = x.shape
    xd = dev(x)
    y0 = fit.tsne_init(xd)
    assert tuple(y0.shape) == (n, 2) and y0.dtype == torch.float32 and y0.is_cuda
    y = host(y0).astype(D)
    sd = np.std(y[:, 0])
    print('tsne_init: std of the first column %.9e' % sd)
    assert abs(sd - 1e-4) <= 4 * EPS * 1e-4 * 2                # 4 ulp of 1e-4 (an ulp is at most 2^-23 of the value)
    want = R.tsne_init(host(fit.transform(xd)).astype(D))
    check('tsne_init against the formula', y, want, (n + 2) * EPS * np.abs(want).max())     # two fp32 sums over n rows, worst case
    ts = engine.tsne(xd, 10.0, 'cosine', 3, init=y0)
    assert ts.n_iter == 3 and ts.seed is None and np.all(np.isfinite(host(ts.embedding)))
    with pytest.raises(ValueError, match='n_components >= 2'):
        engine.pca(xd, 1).tsne_init(xd)


ATTRS = ('mean', 'components', 'explained_variance', 'explained_variance_ratio')


def same_fit(a, b):
    return all(np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))) for k in ATTRS) and \
        (a.total_variance, a.sweeps, a.min_pivot, a.off) == (b.total_variance, b.sweeps, b.min_pivot, b.off)


@pytest.mark.parametrize('name', ['A1', 'B1'])
def test_two_fits_and_the_bf16s_mode_give_identical_bits(name):
    from grl_amd import engine
    x, r, p, ex, m64, m32, fit = fitted(name)
    xd = dev(x)
    assert same_fit(engine.pca(xd, r, p), fit)
    with engine.math_mode('bf16s'):
        other = engine.pca(xd, r, p)
        y = other.transform(xd, True)
    assert same_fit(other, fit) and np.array_equal(bits(y), bits(fit.transform(xd, True)))
    assert not same_fit(engine.pca(xd, r, p, seed=1), fit)


def test_failures_name_their_cure_and_leave_the_device_usable():
    from grl_amd import engine
    from grl_amd._lib import GrlHipError
    x, r, p, ex, m64, m32, fit = fitted('A1')
    bad = x.copy()
    bad[17, 5] = np.nan
    with pytest.raises(GrlHipError, match='remove the non-finite rows'):
        engine.pca(dev(bad), r, p)
    assert same_fit(engine.pca(dev(x), r, p), fit)
    # L above the rank: A1's six directions without noise, L = min(n - 1, d) = 33
    n, d, k, decay = R.CASES['A1'][:4]
    flat = R.planted(n, d, k, decay, noise=0.0)
    rec = R.model(flat, r, 33 - r, dtype=F)['record']
    assert rec['status'] == R.PIVOT_SMALL
    with pytest.raises(GrlHipError, match='lower n_components / oversample'):
        engine.pca(dev(flat), r, 33 - r)
    assert same_fit(engine.pca(dev(x), r, p), fit)
    ok = engine.pca(dev(flat), 6, 0)                           # at the rank it is fine
    check('rank-6 data at L = 6', host(ok.explained_variance), R.exact(flat)['explained_variance'][:6],
          bound(R.model(flat, 6, 0, dtype=F)['explained_variance'], R.exact(flat)['explained_variance'][:6], d + 6,
                R.exact(flat)['explained_variance'][0]))


def test_argument_errors():
    from grl_amd import engine
    x = dev(R.case('A1')[0])
    n, d = x.shape
    for kw in (dict(n_components=0), dict(n_components=True), dict(n_components=2.0), dict(n_components=6, oversample=-1),
               dict(n_components=6, oversample=1.5), dict(n_components=6, n_iter=-1), dict(n_components=6, n_iter=False),
               dict(n_components=6, seed=-1), dict(n_components=6, seed=0.5), dict(n_components=24, oversample=10),
               dict(n_components=34, oversample=0)):
        with pytest.raises(ValueError, match='pca: '):
            engine.pca(x, **kw)
    wide = torch.zeros((600, 600), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match='at most'):
        engine.pca(wide, 510, 3)
    for bad in (x.cpu(), x.double(), x[0], x[:, :, None], x[:1], 'x'):
        with pytest.raises(ValueError, match='pca: '):
            engine.pca(bad, 1, 0)
    fit = fitted('A1')[6]
    for call in (lambda: fit.transform(x[:, :5]), lambda: fit.transform(x.cpu()), lambda: fit.transform(x.double()),
                 lambda: fit.inverse_transform(x), lambda: fit.tsne_init(x[:, :5]), lambda: engine.pca_eigh(x),
                 lambda: engine.pca_eigh(x.cpu()), lambda: engine.pca_orthonormalize(x),
                 lambda: engine.pca_orthonormalize(x[0])):
        with pytest.raises(ValueError):
            call()
    # whiten needs positive kept variances: all-zero rows give a Rayleigh-Ritz matrix of exact zeros
    z = torch.zeros((40, 8), dtype=torch.float32, device=DEV)
    none = engine.pca(z, 2, 0, n_iter=0)
    assert host(none.explained_variance).tolist() == [0.0, 0.0] and none.sweeps == 0 and none.total_variance == 0.0
    assert not bool(none.transform(z).any())
    with pytest.raises(ValueError, match='whiten'):
        none.transform(z, True)


# ----------------------------------------------------------------------------
# 4. ATTEvaluator.evaluate with GRL_EVAL_PCA
# ----------------------------------------------------------------------------
KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_CLUSTER', 'GRL_EVAL_CLUSTER_JACCARD', 'GRL_EVAL_KMEANS', 'GRL_EVAL_SILHOUETTE', 'GRL_EVAL_HDBSCAN',
         'GRL_EVAL_TSNE', 'GRL_EVAL_PCA')


def test_attevaluator_projects_the_features_on_all_three_routes(synth_models, monkeypatch, tmp_path):
    from grl_amd import engine
    from grl_amd.reid.data import get_data
    from grl_amd.reid.evaluator import ATTEvaluator
    cnn, siam, _ = synth_models
    cnn, siam = cnn.to(DEV).eval(), siam.to(DEV).eval()
    _, _, _, q_loader, g_loader = get_data('synthetic', 0, None, 4, 2, 0, 0)
    ev = ATTEvaluator(cnn, siam, only_eval=False)
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    with contextlib.redirect_stdout(io.StringIO()):
        qf, qp, qc = ev.extract_feature(q_loader)
        gf, gp, gc = ev.extract_feature(g_loader)
    gf = torch.cat((qf, gf), 0)
    pids, cams = np.append(qp, gp), np.append(qc, gc)
    path = str(tmp_path) + os.sep
    made = os.path.join(str(tmp_path), 'pca.json')

    def run(rerank=0):
        if os.path.exists(made):
            os.remove(made)
        with contextlib.redirect_stdout(io.StringIO()) as o:
            r = ev.evaluate(None, None, q_loader, g_loader, path, 0, rerank)
        return r, o.getvalue().splitlines(), open(made).read() if os.path.exists(made) else None

    def refuse(c):
        raise ValueError('not strict JSON: %s' % c)

    r_off, text_off, raw_off = run()
    assert raw_off is None and not any(l.startswith('PCA:') for l in text_off)
    monkeypatch.setenv('GRL_EVAL_PCA', '8,1')
    r_on, text_on, raw = run()
    fit = engine.pca(gf, 8)
    lam = [float(v) for v in host(fit.explained_variance)]
    ratio = float(fit.explained_variance_ratio.double().sum())
    line = 'PCA: r = 8, whiten = 1, explained variance ratio = {:.6g}, lambda_1 = {:.6g}, lambda_r = {:.6g}'.format(
        ratio, lam[0], lam[-1])
    assert text_on.count(line) == 1
    at = text_on.index(line)
    assert text_on[:at] == text_off[:at] and text_on[at + 1] == 'Computing distance matrix'
    js = json.loads(raw, parse_constant=refuse)
    assert js['n_components'] == 8 and js['whiten'] is True and js['explained_variance'] == lam
    assert js['explained_variance_ratio_sum'] == ratio and (js['lambda_1'], js['lambda_r']) == (lam[0], lam[-1])
    assert js['n_samples'] == gf.size(0) and js['sweeps'] == fit.sweeps and js['min_pivot'] == fit.min_pivot
    # CMC / mAP are those of the 8-column features (zero-padded to the distance GEMM's 32), on every route
    q8, g8 = (engine._pad_features(fit.transform(t, True)) for t in (qf, gf))
    assert not bool(q8[:, 8:].any()) and not bool(g8[:, 8:].any())

    def lines(cmc, mAP):
        return ['Mean AP: {:4.1%}'.format(mAP)] + ['Rank-{:<3}: {:.1%}'.format(k, cmc[k - 1]) for k in (1, 5, 10, 20)] + \
            ['------------------']

    cmc, mAP = engine.rank_metrics_streaming(q8, g8, qp, pids, qc, cams)
    assert text_on[at + 2:] == lines(cmc, mAP) and r_on == cmc[0]
    monkeypatch.setenv('GRL_EVAL_STREAM', '1')
    r_stream, text_stream, raw_stream = run()
    assert r_stream == r_on and text_stream == text_on and json.loads(raw_stream, parse_constant=refuse) == js
    monkeypatch.delenv('GRL_EVAL_STREAM')
    monkeypatch.setenv('GRL_EVAL_RERANK', 'stream')
    r_rr, text_rr, _ = run(rerank=1)
    cmc, mAP = engine.rerank_metrics_streaming(q8, g8, qp, pids, qc, cams)
    assert text_rr[:at + 2] == text_on[:at + 2] and text_rr[at + 2:] == ['Applying person re-ranking ...'] + lines(cmc, mAP)
    assert r_rr == cmc[0]
    monkeypatch.delenv('GRL_EVAL_RERANK')
    # refused with the verification metric, before the features are extracted
    monkeypatch.setenv('GRL_EVAL_METRIC', 'verify')
    with contextlib.redirect_stdout(io.StringIO()) as o:
        with pytest.raises(ValueError, match='GRL_EVAL_PCA cannot be combined'):
            ev.evaluate(None, None, q_loader, g_loader, path, 0, 0)
    assert 'obtained' not in o.getvalue()
    # unset again: the parent's output, byte for byte
    monkeypatch.delenv('GRL_EVAL_METRIC')
    monkeypatch.delenv('GRL_EVAL_PCA')
    r_again, text_again, raw_again = run()
    assert r_again == r_off and text_again == text_off and raw_again is None
