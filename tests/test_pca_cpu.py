"""The numpy model of engine.pca's contract (tests/pca_ref.py) against LAPACK and scikit-learn, the parts of the
interface that need no device, the GRL_EVAL_PCA knob and the library's bindings."""
import os

import numpy as np
import pytest

import pca_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
ENTRY_POINTS = ('grl_pca_cholesky', 'grl_pca_trsm', 'grl_pca_eigh', 'grl_pca_rowsum', 'grl_pca_rank1', 'grl_pca_sign',
                'grl_pca_affine', 'grl_pca_colscale', 'grl_pca_tsne_init')

_cache = {}


def fitted(name):
    if name not in _cache:
        x, r, p = R.case(name)
        _cache[name] = (x, r, p, R.exact(x), R.model(x, r, p, dtype=D))
    return _cache[name]


# ----------------------------------------------------------------------------
# 1. the float64 model against the exact PCA and against scikit-learn
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['A1', 'A2'])
def test_model64_equals_the_exact_pca_on_the_separated_cases(name):
    x, r, p, ex, m = fitted(name)
    lam, l1 = ex['explained_variance'], ex['explained_variance'][0]
    assert m['components'].shape == (r, x.shape[1]) and m['record']['status'] == 0
    assert np.abs(m['explained_variance'] - lam[:r]).max() <= 1e-12 * l1
    for i in range(r):                                         # every component, none left out
        assert np.abs(m['components'][i] - ex['components'][i]).max() <= 1e-7, i
    assert abs(m['total_variance'] - ex['total_variance']) <= 1e-12 * ex['total_variance']
    assert np.abs(m['mean'] - ex['mean']).max() <= 1e-14


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_model64_explained_variance_sum_is_sklearns(name):
    """Two random starts: only the converged quantity is compared, within what the model itself is away from the exact
    value (the truncation of four power iterations) plus the same for scikit-learn."""
    from sklearn.decomposition import PCA
    x, r, p, ex, m = fitted(name)
    sk = PCA(n_components=r, svd_solver='randomized', n_oversamples=p, iterated_power=4,
             power_iteration_normalizer='QR', random_state=0).fit(x.astype(D))
    exact = ex['explained_variance'][:r].sum()
    own, theirs = m['explained_variance'].sum(), sk.explained_variance_.sum()
    slack = abs(own - exact) + abs(theirs - exact) + 1e-12 * exact
    assert abs(own - theirs) <= slack
    assert own <= exact * (1 + 1e-12)                          # Ritz values never exceed the exact ones in sum
    assert abs(m['total_variance'] - (sk.explained_variance_.sum() / sk.explained_variance_ratio_.sum())) \
        <= 1e-10 * m['total_variance']


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_model32_follows_model64(name):
    """The figures of DESIGN.md 4z's table: float32 loses a few 1e-7 of lambda_1, the pivots stay above 3e-4."""
    x, r, p, ex, m = fitted(name)
    m32 = R.model(x, r, p, dtype=F)
    l1 = m['explained_variance'][0]
    assert np.abs(m32['explained_variance'] - m['explained_variance']).max() <= 1e-6 * l1
    c = m32['components'].astype(D)
    assert np.abs(c @ c.T - np.eye(r)).max() <= 1e-6
    assert m32['record']['status'] == 0 and m32['record']['calls'] == 18 and m32['record']['min_pivot'] >= 3e-4
    assert abs(m32['record']['min_pivot'] - m['record']['min_pivot']) <= 1e-6
    res = R.residual(ex['cov'], m32['components'], m32['explained_variance'])
    assert res <= (1e-6 if name.startswith('A') else 1e-4)


# ----------------------------------------------------------------------------
# 2. the pieces
# ----------------------------------------------------------------------------
def test_sign_rule_and_its_tie():
    c = np.array([[0.1, -0.9, 0.3], [0.5, -0.5, 0.2], [-0.5, 0.5, 0.2], [0.0, 0.0, 0.0], [-0.7, 0.1, 0.7]], dtype=F)
    out = R.sign_fix(c)
    assert np.array_equal(out[0], -c[0])                       # the largest entry was negative
    assert np.array_equal(out[1], c[1])                        # a tie of magnitudes: the lowest column (+0.5) decides
    assert np.array_equal(out[2], -c[2])                       # ... and here it is negative
    assert np.array_equal(out[3], c[3]) and np.array_equal(out[4], -c[4])
    assert np.array_equal(R.sign_fix(out), out)


def test_tsne_init_is_sklearns_pca_start():
    from sklearn.decomposition import PCA
    x, r, p, ex, m = fitted('A2')
    sk = PCA(n_components=2, svd_solver='full').fit_transform(x.astype(D))
    want = sk / np.std(sk[:, 0]) * 1e-4                        # sklearn/manifold/_t_sne.py, init='pca'
    got = R.tsne_init(R.transform(x, ex['mean'], ex['components'][:2]))
    sign = np.sign((got * want).sum(axis=0))                   # scikit-learn fixes the signs by another rule
    assert np.abs(got * sign - want).max() <= 1e-12 * 1e-4 * 10
    assert abs(np.std(got[:, 0]) - 1e-4) <= 1e-18


def test_whitened_transform_has_unit_covariance():
    for name in ('A1', 'B2'):
        x, r, p, ex, m = fitted(name)
        y = R.transform(x, m['mean'], m['components'], m['explained_variance'])
        assert np.abs(np.cov(y, rowvar=False) - np.eye(r)).max() <= 1e-9
        y = R.transform(x, m['mean'], m['components'])
        assert np.abs(np.cov(y, rowvar=False) - np.diag(m['explained_variance'])).max() <= 1e-10 * m['explained_variance'][0]


def test_cholesky_and_solve_orders_and_the_pivot_record():
    g = np.random.Generator(np.random.PCG64(2))
    w = g.standard_normal((37, 90))
    for dtype, tol in ((D, 1e-13), (F, 1e-4)):
        rec = R.new_record()
        gram = (w @ w.T).astype(dtype)
        r = R.cholesky(gram, dtype, rec)
        assert np.abs(r @ r.T - gram).max() <= tol * np.abs(gram).max() and np.all(np.triu(r, 1) == 0)
        assert np.abs(r - np.linalg.cholesky(gram.astype(D))).max() <= tol * np.abs(r).max()
        assert rec['status'] == 0 and rec['calls'] == 1 and 0 < rec['min_pivot'] <= 1
        y = R.trsm(r, w.astype(dtype), dtype)
        assert np.abs(y @ y.T - np.eye(37)).max() <= tol * 100
    # rank-deficient: a duplicated row fails at its own pivot, the factor is the identity from there, the solve finite
    w[20] = w[3]
    rec = R.new_record()
    q = R.orthonormalize(w, F, rec)
    assert (rec['status'], rec['index'], rec['call'], rec['calls']) == (R.PIVOT_SMALL, 20, 0, 2)
    assert rec['min_pivot'] <= R.pivot_tol(37) and np.all(np.isfinite(q))
    assert np.abs(q[:20] @ q[:20].T - np.eye(20)).max() <= 1e-5
    # not finite: recorded as such, and sticky -- the first failure stays
    w[5, 7] = np.nan
    rec = R.new_record()
    R.orthonormalize(w, F, rec)
    assert rec['status'] == R.PIVOT_NONFINITE and rec['call'] == 0 and rec['calls'] == 2
    # the model ends a fit with a bad record without an eigensolve
    x, r, p = R.case('A1')
    bad = x.copy()
    bad[17, 5] = np.nan
    out = R.model(bad, r, p, dtype=F)
    assert out['record']['status'] == R.PIVOT_NONFINITE and 'components' not in out
    n, d, k, decay = R.CASES['A1'][:4]
    out = R.model(R.planted(n, d, k, decay, noise=0.0), r, 33 - r, dtype=F)
    assert out['record']['status'] == R.PIVOT_SMALL and 'components' not in out


@pytest.mark.parametrize('L', [1, 2, 3, 16, 65, 130])
def test_jacobi_model_converges_and_is_orthonormal(L):
    """grl_pca_eigh's algorithm in numpy float32: the round-robin order converges well inside 30 sweeps, and the
    rotation in Rutishauser's form keeps |V^T V - I| at a few 2^-24 (c x_p - s x_q loses 2e-5 at L = 130)."""
    g = np.random.Generator(np.random.PCG64(3 + L))
    lam = np.sort(g.uniform(0.1, 1.0, L))[::-1].copy()
    if L >= 3:
        lam[1] = lam[0]
        lam[-1] = 0.0
    v = np.linalg.qr(g.standard_normal((L, L)))[0]
    b = ((v * lam) @ v.T).astype(F)
    got, vec, sweeps, off, fro = R.jacobi(b)
    want = np.linalg.eigvalsh(b.astype(D))[::-1]
    vec = vec.astype(D)
    assert sweeps < 20 and off <= 2.0 ** -26 * fro * 1.001
    assert np.abs(got - want).max() <= 2 * L * 2.0 ** -24 * want[0]
    assert np.abs(vec.T @ vec - np.eye(L)).max() <= max(2 * L, 8) * 2.0 ** -24
    assert np.abs(b.astype(D) @ vec - vec * got).max() <= 2 * L * 2.0 ** -24 * want[0]
    pairs = [pq for rnd in R.round_robin(L) for pq in rnd]
    assert sorted(pairs) == [(i, j) for i in range(L) for j in range(i + 1, L)]      # every pair once a sweep
    assert all(len(set(sum(rnd, ()))) == 2 * len(rnd) for rnd in R.round_robin(L))     # disjoint within a round
    d = np.diag(np.arange(L, 0, -1).astype(F))
    assert R.jacobi(d)[2] == 0


# ----------------------------------------------------------------------------
# 3. the engine's checks that need no device, the knob, the library
# ----------------------------------------------------------------------------
def test_engine_refuses_bad_arguments_before_any_device_work():
    import torch
    from grl_amd import engine
    x = torch.zeros((8, 4))
    for call in (lambda: engine.pca(x, 2), lambda: engine.pca(x.numpy(), 2), lambda: engine.pca_eigh(x),
                 lambda: engine.pca_orthonormalize(x)):
        with pytest.raises(ValueError, match='on a HIP device'):
            call()
    assert engine.PCA_LMAX == 512 and engine.PCA_MAX_SWEEPS == R.MAX_SWEEPS
    assert engine._pca_pivot_tol(138) == R.pivot_tol(138)


def test_pca_knob_parser():
    from grl_amd.reid.evaluator.attevaluator import parse_pca_knob as parse
    assert parse('GRL_EVAL_PCA', None) is None and parse('GRL_EVAL_PCA', '  ') is None
    assert parse('GRL_EVAL_PCA', '128') == (128, False) and parse('GRL_EVAL_PCA', ' 256 , 1 ') == (256, True)
    assert parse('GRL_EVAL_PCA', '1,0') == (1, False) and parse('GRL_EVAL_PCA', '502,1') == (502, True)
    for bad in ('x', '8,', '8,2', '8,-1', '8,1,0', '0', '-3', '503', '8.5', '8,yes', 'nan', ','):
        with pytest.raises(ValueError, match='GRL_EVAL_PCA'):
            parse('GRL_EVAL_PCA', bad)


def test_pca_knob_is_refused_with_the_verification_metric(monkeypatch):
    from grl_amd.reid.evaluator import ATTEvaluator
    monkeypatch.setenv('GRL_EVAL_PCA', '8,1')
    monkeypatch.setenv('GRL_EVAL_METRIC', 'verify')
    with pytest.raises(ValueError, match='GRL_EVAL_PCA cannot be combined with GRL_EVAL_METRIC=verify'):
        ATTEvaluator(None, None, only_eval=True).evaluate(None, None, None, None, '', 0, 0)
    monkeypatch.setenv('GRL_EVAL_PCA', 'many')
    monkeypatch.delenv('GRL_EVAL_METRIC')
    with pytest.raises(ValueError, match='GRL_EVAL_PCA must be'):
        ATTEvaluator(None, None, only_eval=True).evaluate(None, None, None, None, '', 0, 0)


def test_lib_binds_the_pca_entry_points_at_abi_version_10():
    from grl_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 10 and lib.grl_abi_version() == 10
    header = open(os.path.join(ROOT, 'include', 'grl_hip.h')).read()
    assert '#define GRL_ABI_VERSION 10' in header and 'grl_pca_*' in header
    for name in ENTRY_POINTS:
        assert name in _lib.exported_symbols() and getattr(lib, name).restype is not None
        assert 'int %s(' % name in header
    assert ' pca.hip ' in open(os.path.join(ROOT, 'grl_amd', 'csrc', 'Makefile')).read()
    assert '#define GRL_PCA_LMAX 512' in header and '#define GRL_PCA_MAX_SWEEPS 30' in header


def test_entry_points_check_their_arguments_before_any_launch():
    from grl_amd import _lib
    lib = _lib.load()
    p = 16                                                       # any non-null aligned address: nothing is dereferenced
    E = _lib.GRL_EINVAL
    assert lib.grl_pca_cholesky(p, 32, 0, 1e-6, p, None) == E and lib.grl_pca_cholesky(p, 32, 513, 1e-6, p, None) == E
    assert lib.grl_pca_cholesky(p, 8, 16, 1e-6, p, None) == E and lib.grl_pca_cholesky(None, 32, 16, 1e-6, p, None) == E
    assert lib.grl_pca_cholesky(p, 32, 16, 1e-6, None, None) == E and lib.grl_pca_cholesky(p, 32, 16, float('nan'), p, None) == E
    assert lib.grl_pca_trsm(p, 8, p, 64, 16, 64, None) == E and lib.grl_pca_trsm(p, 32, p, 32, 16, 64, None) == E
    assert lib.grl_pca_trsm(None, 32, p, 64, 16, 64, None) == E and lib.grl_pca_trsm(p, 32, p, 64, 16, 0, None) == 0
    assert lib.grl_pca_eigh(p, 32, p + 64, 32, 600, p, p + 128, 32, p, None) == E
    assert lib.grl_pca_eigh(p, 32, p, 32, 16, p, p + 128, 32, p, None) == E          # a and vt_work are one buffer
    assert lib.grl_pca_eigh(p, 32, p + 64, 32, 16, p, p + 128, 32, None, None) == E
    assert lib.grl_pca_eigh(p, 8, p + 64, 32, 16, p, p + 128, 32, p, None) == E
    assert lib.grl_pca_rowsum(p, 4, 2, 8, p, None) == E and lib.grl_pca_rowsum(p, 8, 0, 8, p, None) == 0
    assert lib.grl_pca_rank1(p, 4, 2, 8, p, p, None) == E and lib.grl_pca_rank1(p, 8, 2, 8, None, p, None) == E
    assert lib.grl_pca_sign(p, 8, 2, 0, None) == E and lib.grl_pca_sign(None, 8, 2, 8, None) == E
    assert lib.grl_pca_affine(None, None, 4, p, p, None) == E and lib.grl_pca_affine(p, None, 0, p, p, None) == E
    assert lib.grl_pca_colscale(p, 2, 4, 4, p, p, 4, None) == E and lib.grl_pca_colscale(p, 4, 0, 4, p, p, 4, None) == 0
    assert lib.grl_pca_tsne_init(p, 1, 4, p, None) == E and lib.grl_pca_tsne_init(p, 2, 0, p, None) == E
