"""The t-SNE contract on the host: the numpy model of tests/tsne_ref.py against scikit-learn's exact
gradient and its perplexity search, the float32 model against the float64 model, the update rule, isolated samples, the
evaluator's knob parser and the library's bindings.  No GPU."""
import math
import os

import numpy as np
import pytest

import hdbscan_ref as HR
import silhouette_ref as SR
import tsne_ref as TR

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('grl_tsne_square_block', 'grl_tsne_perplexity', 'grl_tsne_joint', 'grl_tsne_repulsion', 'grl_tsne_z',
                'grl_tsne_update', 'grl_tsne_kl')
_cache = {}


def host_distances(x):
    """the contract's e(i, j) for both metrics from float32 host arithmetic (the bits of the device's GEMM are not
    needed here: the model is compared with itself and with scikit-learn on the same distances)"""
    x = np.asarray(x, dtype=F)
    negdot = (-(x.astype(np.float64) @ x.astype(np.float64).T)).astype(F)
    sq = (x.astype(np.float64) ** 2).sum(1).astype(F)
    d2 = np.maximum(sq[:, None].astype(np.float64) + sq[None, :] + 2.0 * negdot, 0.0)
    np.fill_diagonal(d2, 0.0)
    return {'cosine': HR.cosine_matrix(negdot, sq), 'euclidean': TR.squared(np.sqrt(d2).astype(F))}


def case(n, metric='cosine', perplexity=30.0, d=24):
    key = (n, metric, perplexity, d)
    if key not in _cache:
        x = SR.planted(d=d)[0][:n]
        e = host_distances(x)[metric]
        K = TR.n_neighbours(n, perplexity)
        idx, dist = TR.neighbours(e, K)
        c32, b32, iso, steps = TR.conditional32(dist, perplexity)
        c64, b64, _ = TR.conditional64(dist, perplexity)
        _cache[key] = dict(e=e, K=K, idx=idx, dist=dist, c32=c32, b32=b32, c64=c64, b64=b64, iso=iso, steps=steps)
    return _cache[key]


CASES = [(129, 'cosine', 30.0), (336, 'cosine', 30.0), (336, 'euclidean', 5.0), (336, 'cosine', 100.0)]


# ----------------------------------------------------------------------------
# 1. the float64 model against scikit-learn
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('n', [129, 336])
def test_model64_gradient_and_kl_are_sklearns_exact_ones(n):
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne
    c = case(n)
    p, _ = TR.joint64(c['idx'], c['c64'], c['iso'])
    assert np.array_equal(p, p.T) and abs(p.sum() - 1.0) < 1e-12
    g = np.random.Generator(np.random.PCG64(3))
    for scale in (1e-4, 3.0):
        y = g.standard_normal((n, 2)) * scale
        for alpha in (1.0, 12.0):
            kl_sk, grad_sk = _t_sne._kl_divergence(y.ravel(), squareform(alpha * p, checks=False), 1.0, n, 2)
            grad, z = TR.gradient64(alpha * p, y)
            assert np.abs(grad - grad_sk.reshape(n, 2)).max() <= 1e-12 * max(1.0, np.abs(grad_sk).max())
            if alpha == 1.0:                  # (sklearn's KL of an exaggerated P is not a divergence of distributions)
                assert abs(TR.kl64(p, y) - kl_sk) <= 1e-9 * abs(kl_sk)


@pytest.mark.parametrize('n,metric,perplexity', CASES)
def test_model64_conditionals_are_sklearns_binary_search(n, metric, perplexity):
    """scikit-learn holds beta in single precision (2^-24 relative), which moves p by p |e - <e>| beta 2^-24: with
    |e - <e>| beta <= 17 for every p >= 1e-7 and p <= 1 that is below 1e-6; the stop rule is the same."""
    from sklearn.manifold import _utils
    c = case(n, metric, perplexity)
    want = np.asarray(_utils._binary_search_perplexity(c['dist'], perplexity, 0), dtype=np.float64)
    assert np.abs(c['c64'] - want).max() <= 1e-6
    assert np.allclose(TR.perplexity_of(c['c64']), perplexity, rtol=2e-5)


# ----------------------------------------------------------------------------
# 2. the float32 model against the float64 model
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('n,metric,perplexity', CASES)
def test_model32_conditionals_follow_model64(n, metric, perplexity):
    """Both searches stop at |H - log(perplexity)| <= 1e-5; float32 evaluates H (about 1.6 .. 4.6 here) to a few 1e-6.
    So the two entropies differ by at most 3e-5: the perplexity by 3e-5 relative, and p, through dp = p (e - <e>) beta
    dH / Var(e beta) with p |e - <e>| beta <= 1 / e . 1 and Var(e beta) >= 0.05 on these inputs, by less than 1e-4 --
    a cap; the measured values are about 7e-6."""
    c = case(n, metric, perplexity)
    assert not c['iso'].any() and c['steps'].max() <= 60
    assert np.abs(c['c32'].astype(np.float64).sum(1) - 1.0).max() <= 1e-5
    assert np.abs(TR.perplexity_of(c['c32']) / perplexity - 1.0).max() <= 5e-5
    assert np.abs(c['c32'] - c['c64']).max() <= 1e-4
    r32, c32, v32 = TR.joint32(c['idx'], c['c32'], c['iso'])
    p64, m64 = TR.joint64(c['idx'], c['c64'], c['iso'])
    r64, c64_, v64 = TR.to_csr(p64, m64)
    assert np.array_equal(r32, r64) and np.array_equal(c32, c64_)
    assert np.abs(v32 - v64).max() <= 1e-4 / n + 2.0 ** -23 * v64.max()
    dense = TR.to_dense(r32, c32, v32, F)
    assert np.array_equal(dense.view(np.uint32), dense.T.view(np.uint32))        # symmetric bit for bit


def gradient_envelope(p, y, alpha):
    """4 (sum |att terms| + sum |rep terms| / Z) per coordinate, in float64: what a rounding error is relative to"""
    y = np.asarray(y, dtype=np.float64)
    dx = y[:, None, :] - y[None, :, :]
    q = 1.0 / (1.0 + (dx ** 2).sum(2))
    np.fill_diagonal(q, 0.0)
    z = q.sum()
    return 4.0 * ((alpha * p * q + q * q / z)[..., None] * np.abs(dx)).sum(1)


@pytest.mark.parametrize('n', [129, 336])
def test_model32_gradient_follows_model64(n):
    """On the same float32 affinities and coordinates the two differ by rounding alone.  A term takes 8 roundings (the
    differences, two squares, their sum, 1 + r, the division, q q or alpha P q, the product) and its partial sum
    n / 64 + 6 <= 12 additions; Z adds its own 12 to the repulsive part: 32 x 2^-24 of the sum of the terms'
    magnitudes bounds it."""
    c = case(n)
    row_ptr, col, val = TR.joint32(c['idx'], c['c32'], c['iso'])
    p = TR.to_dense(row_ptr, col, val)
    g = np.random.Generator(np.random.PCG64(4))
    for y in (TR.init_random(n, 0), (g.standard_normal((n, 2)) * 3).astype(F)):
        for alpha in (1.0, 12.0):
            g32, z32 = TR.gradient32(row_ptr, col, val, y, alpha)
            g64, z64 = TR.gradient64(p, y, alpha)
            assert g32.dtype == F and abs(float(z32) / z64 - 1.0) <= 24 * 2.0 ** -24
            assert (np.abs(g32 - g64) <= 32 * 2.0 ** -24 * gradient_envelope(p, y, alpha) + 1e-30).all()
        assert abs(TR.kl32(row_ptr, col, val, y) - TR.kl64(p, y)) <= 1e-5 * abs(TR.kl64(p, y))


def test_wave_sum_is_the_order_of_the_silhouette_model():
    g = np.random.Generator(np.random.PCG64(8))
    for L in (0, 1, 63, 64, 65, 129, 336):
        t = g.standard_normal((3, L)).astype(F)
        want = np.zeros(3, dtype=F)
        for r in range(3):
            part = np.zeros(64, dtype=F)
            for p in range(L):
                part[p % 64] = part[p % 64] + t[r, p]
            want[r] = SR.tree(part)
        assert np.array_equal(TR.wave_sum(t).view(np.uint32), want.view(np.uint32))


# ----------------------------------------------------------------------------
# 3. the update rule and the schedule
# ----------------------------------------------------------------------------
def test_update_rule_on_hand_built_arrays():
    y = np.array([[1.0, -2.0], [0.5, 0.25], [3.0, 3.0]], dtype=F)
    update = np.array([[0.5, 0.5], [-1.0, 0.0], [2.0, -2.0]], dtype=F)
    gains = np.array([[1.0, 1.0], [0.011, 2.0], [1.0, 0.5]], dtype=F)
    grad = np.array([[-1.0, 1.0], [-3.0, 4.0], [0.0, 8.0]], dtype=F)
    ny, nu, ng = TR.step32(y, update, gains, grad, 0.5, 200.0)
    # update * grad < 0 grows the gain by 0.2, otherwise (zero included) it shrinks by 0.8, floored at 0.01
    want_g = np.array([[F(1.0) + F(0.2), F(1.0) * F(0.8)], [F(0.01), F(2.0) * F(0.8)], [F(1.0) * F(0.8), F(0.5) + F(0.2)]], dtype=F)
    assert np.array_equal(ng, want_g)
    want_u = (F(0.5) * update - F(200.0) * (want_g * grad).astype(F)).astype(F)
    assert np.array_equal(nu, want_u) and np.array_equal(ny, (y + want_u).astype(F))
    assert ng[1, 0] == F(0.01) and F(0.011) * F(0.8) < F(0.01)
    # an isolated sample keeps everything
    ny, nu, ng = TR.step32(y, update, gains, grad, 0.5, 200.0, isolated=np.array([False, True, False]))
    assert np.array_equal(ny[1], y[1]) and np.array_equal(nu[1], update[1]) and np.array_equal(ng[1], gains[1])
    assert np.array_equal(ny[[0, 2]], (y + want_u).astype(F)[[0, 2]])


def test_momentum_and_exaggeration_switch_at_exaggeration_iter():
    assert TR.schedule(0) == (12.0, 0.5) and TR.schedule(249) == (12.0, 0.5) and TR.schedule(250) == (1.0, 0.8)
    assert TR.schedule(1, 4.0, 2) == (4.0, 0.5) and TR.schedule(2, 4.0, 2) == (1.0, 0.8)
    assert TR.auto_learning_rate(336) == 50.0 and TR.auto_learning_rate(13290) == 13290 / 12.0 / 4.0
    c = case(129)
    csr = TR.joint32(c['idx'], c['c32'], c['iso'])
    y0 = TR.init_random(129, 0)
    y, u, g = TR.run32(*csr, y0, 4, 50.0, 12.0, 2)
    # by hand: two steps at (12, 0.5), two at (1, 0.8)
    hy, hu, hg = y0, np.zeros_like(y0), np.ones_like(y0)
    for alpha, mom in ((12.0, 0.5), (12.0, 0.5), (1.0, 0.8), (1.0, 0.8)):
        grad, _ = TR.gradient32(*csr, hy, alpha)
        hy, hu, hg = TR.step32(hy, hu, hg, grad, mom, 50.0)
    assert np.array_equal(y, hy) and np.array_equal(u, hu) and np.array_equal(g, hg)
    # a run continued from its state is the same run
    y2, u2, g2 = TR.run32(*csr, y0, 2, 50.0, 12.0, 2)
    y3, u3, g3 = TR.run32(*csr, y2, 2, 50.0, 12.0, 2, first=2, update=u2, gains=g2)
    assert np.array_equal(y3, y) and np.array_equal(u3, u) and np.array_equal(g3, g)
    assert np.array_equal(TR.init_random(5, 7), np.random.Generator(np.random.PCG64(7)).standard_normal((5, 2)).astype(F) * F(1e-4))


# ----------------------------------------------------------------------------
# 4. isolated samples
# ----------------------------------------------------------------------------
def test_a_nan_row_is_isolated_and_exerts_no_force():
    n, bad = 80, 17
    x = SR.planted(d=24)[0][:n].copy()
    x[bad] = np.nan
    e = host_distances(x)['cosine']
    K = TR.n_neighbours(n, 5.0)
    idx, dist = TR.neighbours(e, K)
    assert not (idx[np.arange(n) != bad] == bad).any()          # NaN ranks last: nobody's neighbour
    cond, beta, iso, _ = TR.conditional32(dist, 5.0)
    assert iso.tolist() == [i == bad for i in range(n)] and np.isnan(beta[bad]) and not cond[bad].any()
    row_ptr, col, val = TR.joint32(idx, cond, iso)
    assert row_ptr[bad + 1] == row_ptr[bad] and not (col == bad).any() and np.isfinite(val).all()
    keep = np.arange(n) != bad
    y = (np.random.Generator(np.random.PCG64(1)).standard_normal((n, 2)) * 2).astype(F)
    y[bad] = np.nan                                             # whatever the isolated row holds, nobody reads it
    g32, z32 = TR.gradient32(row_ptr, col, val, y, 12.0, iso)
    assert np.isfinite(g32).all() and not g32[bad].any() and np.isfinite(z32)
    # the same forces as in the problem without the sample (float64: no order to respect)
    p = TR.to_dense(row_ptr, col, val)
    g64, z64 = TR.gradient64(p, np.nan_to_num(y), 12.0, iso)
    gr, zr = TR.gradient64(p[np.ix_(keep, keep)], y[keep], 12.0)
    assert np.allclose(g64[keep], gr, rtol=1e-12, atol=1e-15) and np.isclose(z64, zr, rtol=1e-13) and not g64[bad].any()
    assert (np.abs(g32[keep] - gr) <= 32 * 2.0 ** -24 * gradient_envelope(p[np.ix_(keep, keep)], y[keep], 12.0) + 1e-30).all()
    # the loop: the isolated row never moves, everybody else stays finite; the KL ignores it
    y0 = TR.init_random(n, 0)
    yy, uu, gg = TR.run32(row_ptr, col, val, y0, 3, 50.0, isolated=iso)
    assert np.array_equal(yy[bad], y0[bad]) and np.isfinite(yy).all() and not uu[bad].any() and (gg[bad] == 1).all()
    assert math.isfinite(TR.kl32(row_ptr, col, val, yy, iso))
    assert np.isclose(TR.kl32(row_ptr, col, val, yy, iso), TR.kl64(p, yy, iso), rtol=1e-5)


def test_model_neighbours_delete_the_sample_by_index_or_the_last_entry():
    e = np.array([[0, 1, 2, 3], [1, 0, 0, 0], [2, 0, 0, 5], [3, 0, 5, 0]], dtype=F)
    idx, dist = TR.neighbours(e, 2)
    # row 1: the zeros tie, the index decides: top-3 = (1, 2, 3) -> the sample deleted; row 2: (1, 2, 0) -> (1, 0)
    assert idx.tolist() == [[1, 2], [2, 3], [1, 0], [1, 0]] and dist.tolist() == [[1, 2], [0, 0], [0, 2], [0, 3]]
    e[3, 3] = 9                                                  # row 3: top-3 = (1, 0, 2): the sample is not in it
    assert TR.neighbours(e, 2)[0][3].tolist() == [1, 0]
    assert TR.n_neighbours(336, 30.0) == 91 and TR.n_neighbours(65, 30.0) == 64 and TR.n_neighbours(336, 5.0) == 16
    assert TR.n_neighbours(336, 100.0) == 301 and TR.n_neighbours(10 ** 6, 340.9) == 1023


# ----------------------------------------------------------------------------
# 5. the engine's checks that need no device, the knob, the library
# ----------------------------------------------------------------------------
def test_engine_refuses_host_tensors_before_any_device_work():
    import torch
    from grl_amd import engine
    x = torch.zeros((8, 4))
    for fn in (engine.tsne, engine.tsne_affinities):
        with pytest.raises(ValueError, match='on a HIP device'):
            fn(x)
        with pytest.raises(ValueError, match='on a HIP device'):
            fn(x.numpy())
        vm = engine.VerifyMetric.__new__(engine.VerifyMetric)
        with pytest.raises(ValueError, match='verify_metric'):
            fn(x, metric=vm)
        with pytest.raises(ValueError, match="'cosine' or 'euclidean'"):
            fn(x, metric='jaccard')
    rp = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match='row_ptr must be'):
        engine.tsne_gradient(rp, torch.zeros(0, dtype=torch.int32), torch.zeros(0), torch.zeros((3, 2)))
    with pytest.raises(ValueError, match='row_ptr must be'):
        engine.tsne_from_affinities(rp, torch.zeros(0, dtype=torch.int32), torch.zeros(0), 10)


def test_tsne_knob_parser():
    from grl_amd.reid.evaluator.attevaluator import parse_tsne_knob as parse
    assert parse('GRL_EVAL_TSNE', None) is None and parse('GRL_EVAL_TSNE', '  ') is None
    assert parse('GRL_EVAL_TSNE', '1') == (30.0, 1000, 0)
    assert parse('GRL_EVAL_TSNE', '1,200') == (1.0, 200, 0)
    assert parse('GRL_EVAL_TSNE', ' 12.5 , 300 , 4 ') == (12.5, 300, 4)
    assert parse('GRL_EVAL_TSNE', '340') == (340.0, 1000, 0)
    for bad in ('x', '30,', '30,1.5', '30,10,1,2', '0.5', '341', 'nan', 'inf', '30,0', '30,10,-1', ','):
        with pytest.raises(ValueError, match='GRL_EVAL_TSNE'):
            parse('GRL_EVAL_TSNE', bad)


def test_tsne_knob_is_refused_with_the_verification_metric(monkeypatch):
    from grl_amd.reid.evaluator import ATTEvaluator
    monkeypatch.setenv('GRL_EVAL_TSNE', '1')
    monkeypatch.setenv('GRL_EVAL_METRIC', 'verify')
    with pytest.raises(ValueError, match='GRL_EVAL_TSNE cannot be combined with GRL_EVAL_METRIC=verify'):
        ATTEvaluator(None, None, only_eval=True).evaluate(None, None, None, None, '', 0, 0)
    monkeypatch.setenv('GRL_EVAL_TSNE', 'many')
    monkeypatch.delenv('GRL_EVAL_METRIC')
    with pytest.raises(ValueError, match='GRL_EVAL_TSNE must be'):
        ATTEvaluator(None, None, only_eval=True).evaluate(None, None, None, None, '', 0, 0)


def test_lib_binds_the_tsne_entry_points_at_abi_version_10():
    from grl_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 10 and lib.grl_abi_version() == 10
    header = open(os.path.join(ROOT, 'include', 'grl_hip.h')).read()
    assert '#define GRL_ABI_VERSION 10' in header and 'grl_tsne_*' in header
    for name in ENTRY_POINTS:
        assert name in _lib.exported_symbols() and getattr(lib, name).restype is not None
        assert 'int %s(' % name in header
    assert ' tsne.hip ' in open(os.path.join(ROOT, 'grl_amd', 'csrc', 'Makefile')).read()


def test_entry_points_check_their_arguments_before_any_launch():
    from grl_amd import _lib
    lib = _lib.load()
    p = 16                                                       # any non-null 8-byte aligned address: nothing is dereferenced
    E = _lib.GRL_EINVAL
    assert lib.grl_tsne_square_block(None, 8, 4, 8, None) == E and lib.grl_tsne_square_block(p, 7, 4, 8, None) == E
    assert lib.grl_tsne_square_block(p, 8, 0, 8, None) == 0
    assert lib.grl_tsne_perplexity(p, 4, 0, 1.0, p, p, p, None) == E and lib.grl_tsne_perplexity(p, 4, 1024, 1.0, p, p, p, None) == E
    assert lib.grl_tsne_perplexity(p, 4, 8, float('nan'), p, p, p, None) == E
    assert lib.grl_tsne_perplexity(p, 4, 8, 1.0, p, None, p, None) == E and lib.grl_tsne_perplexity(p, 0, 8, 1.0, p, p, p, None) == 0
    assert lib.grl_tsne_joint(p, p, 8, p, p, p, 4, 0.0, None, p, None, None, None) == E          # den
    assert lib.grl_tsne_joint(p, p, 8, p, p, p, 4, 8.0, None, None, None, None, None) == E       # count without cnt
    assert lib.grl_tsne_joint(p, p, 8, p, p, p, 4, 8.0, p, None, p, None, None) == E             # fill without val
    assert lib.grl_tsne_repulsion(None, None, 4, p, p, None) == E and lib.grl_tsne_repulsion(p + 4, None, 4, p, p, None) == E
    assert lib.grl_tsne_repulsion(p, None, 0, p, p, None) == 0 and lib.grl_tsne_z(p, 4, None, None) == E
    ok = [p, p, p, p, None, 4, 1.0, p, p, None, p, p, p + 8, 0.5, 50.0, None]
    for i, v in ((0, None), (3, None), (7, None), (8, None), (12, p), (12, None), (10, None), (3, p + 4)):
        a = list(ok)
        a[i] = v
        assert lib.grl_tsne_update(*a) == E, i
    a = list(ok)
    a[9] = a[10] = a[11] = a[12] = None                          # neither a gradient nor a step
    assert lib.grl_tsne_update(*a) == E
    assert lib.grl_tsne_kl(p, p, p, p, None, 4, None, p, None) == E and lib.grl_tsne_kl(p, p, p, p, None, 0, p, p, None) == 0
