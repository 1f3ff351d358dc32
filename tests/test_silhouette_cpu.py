"""The host model of the silhouette contract (tests/silhouette_ref.py) against scikit-learn and a float64
evaluation, and the argument checks of engine.silhouette / cluster_select and the GRL_EVAL_SILHOUETTE parser that
need no device.

The bound of the comparison with scikit-learn comes from the arithmetic, with u = 2^-24: a cosine distance of the
model carries at most (d + 6) u of absolute error (a d-term fp32 dot product relative to the product of the norms, two
norms of d terms each through one sqrt and one reciprocal, two multiplies, one add), and a mean over at most m_max
distances adds (m_max + 2) u D_max (m_max - 1 adds in any order, one division).  So every mean is within
Delta = (d + 6) u + (m_max + 2) u D_max of the exact one, and s = (b - a) / max(a, b) moves by at most
2 (Delta_a + Delta_b) / max(a, b)."""
import numpy as np
import pytest

import cluster_ref as CR
import silhouette_ref as SR

U = 2.0 ** -24
F = np.float32


def _matrices(x):
    """(float32 cosine matrix by the model's chain from float32 dot products, float64 reference matrix)"""
    x64 = x.astype(np.float64)
    dot = np.zeros((x.shape[0], x.shape[0]), dtype=F)
    sq = np.zeros(x.shape[0], dtype=F)
    for c in range(x.shape[1]):                                  # sequential fp32 accumulation over the features
        dot = (dot + (x[:, c, None] * x[None, :, c]).astype(F)).astype(F)
        sq = (sq + (x[:, c] * x[:, c]).astype(F)).astype(F)
    xn = x64 / np.linalg.norm(x64, axis=1, keepdims=True)
    ref = np.clip(1.0 - xn @ xn.T, 0.0, None)
    np.fill_diagonal(ref, 0.0)
    return SR.cosine_matrix(-dot, sq), ref


_case = {}


def case():
    if not _case:
        x, ids = SR.planted()
        _case['x'], _case['ids'] = x, ids
        _case['d32'], _case['d64'] = _matrices(x)
    return _case['x'], _case['ids'], _case['d32'], _case['d64']


def bound(ref64, ids, d):
    """per-sample bound on |s_model - s_reference| and the reference's max(a, b)"""
    _, a, b, _ = SR.samples64(ref64, ids)
    m_max = int(np.bincount(ids).max())
    delta = (d + 6) * U + (m_max + 2) * U * float(ref64.max())
    mx = np.maximum(a, b)
    return 2.0 * (delta + delta) / np.maximum(mx, 1e-300), mx


# ----------------------------------------------------------------------------
# the model against scikit-learn
# ----------------------------------------------------------------------------
def test_model_is_within_the_arithmetic_bound_of_sklearn_on_the_float64_matrix():
    skm = pytest.importorskip('sklearn.metrics')
    x, ids, d32, d64 = case()
    assert x.shape == (336, 24) and np.bincount(ids).tolist() == [1, 1, 2, 3, 63, 64, 65, 130, 7]
    norms = np.linalg.norm(x.astype(np.float64), axis=1)
    assert norms.min() >= 0.49 and norms.max() <= 1.81 and norms.max() / norms.min() > 2
    want = skm.silhouette_samples(d64, ids, metric='precomputed')
    s64 = SR.samples64(d64, ids)[0]
    assert np.abs(s64 - want).max() <= 1e-12                     # the float64 evaluator is sklearn's definition
    lim, mx = bound(d64, ids, x.shape[1])
    multi = np.bincount(ids)[ids] > 1
    assert mx[multi].min() >= 0.05, mx[multi].min()
    s, a, b, scored = SR.samples(d32, ids)
    err = np.abs(s.astype(np.float64) - want)
    print('min max(a, b) = %.3g, largest bound = %.3g, largest difference = %.3g'
          % (mx[multi].min(), lim[multi].max(), err.max()))
    assert scored.all() and (err[multi] <= lim[multi]).all(), float((err[multi] / lim[multi]).max())
    assert (s[~multi] == 0).all() and (want[~multi] == 0).all() and (a[~multi] == 0).all()    # sklearn's singleton rule
    assert SR.score(s, scored) == pytest.approx(skm.silhouette_score(d64, ids, metric='precomputed'), abs=lim.max())


def test_noise_as_singletons_equals_sklearn_on_relabelled_labels_and_drop_leaves_them_out():
    skm = pytest.importorskip('sklearn.metrics')
    x, ids, d32, d64 = case()
    lab = ids.copy()
    noise = np.flatnonzero(ids == 7)[::9]                        # 15 samples of the largest cluster become noise
    lab[noise] = -1 - np.arange(noise.size) % 3                  # any negative label is noise
    relab, k = SR.relabel(lab, 'singleton')
    assert k == 9 + noise.size and np.array_equal(relab[noise], 9 + np.arange(noise.size))
    want = skm.silhouette_samples(d64, relab, metric='precomputed')
    s, a, b, scored = SR.samples(d32, lab, 'singleton')
    lim, _ = bound(d64, relab, x.shape[1])
    multi = np.bincount(relab)[relab] > 1
    assert scored.all() and (np.abs(s - want)[multi] <= lim[multi]).all()
    assert (s[noise] == 0).all() and (s[~multi] == 0).all()
    # 'drop': neither rows nor columns
    keep = lab >= 0
    s2, a2, b2, scored2 = SR.samples(d32, lab, 'drop')
    assert np.array_equal(scored2, keep) and (s2[~keep] == 0).all() and (a2[~keep] == 0).all() and (b2[~keep] == 0).all()
    want2 = skm.silhouette_samples(d64[np.ix_(keep, keep)], lab[keep], metric='precomputed')
    lim2, _ = bound(d64[np.ix_(keep, keep)], lab[keep], x.shape[1])
    multi2 = np.bincount(lab[keep])[lab[keep]] > 1
    assert (np.abs(s2[keep] - want2)[multi2] <= lim2[multi2]).all()
    # dropping the rows and columns by hand is the same bits
    s3 = SR.samples(d32[np.ix_(keep, keep)], lab[keep], 'drop')[0]
    assert np.array_equal(s3.view(np.uint32), s2[keep].view(np.uint32))


# ----------------------------------------------------------------------------
# the order of the sum, empty ids, NaN
# ----------------------------------------------------------------------------
def test_model_sum_follows_the_64_lane_order_and_not_a_sequential_one():
    """2^24 absorbs a lone 1.0 but not the 2.0 that two of them make.  Cluster 1 has 130 members at positions 2..131;
    row 0 (in cluster 0) sees 2^24 at position 2 and 1.0 elsewhere: lane 2 holds 2^24 + 1 + 1 -> 2^24 (both absorbed),
    lane 3 holds 3 (positions 3, 67, 131) and every other lane 2, which the tree then adds without loss of more than
    the odd 1: 127 of the 129 ones survive, up to the last rounding."""
    n = 132
    lab = np.array([0, 0] + [1] * 130)
    d = np.ones((n, n), dtype=F)
    d[0, 2] = F(2.0 ** 24)
    sums, mem, mptr, counts = SR.cluster_sums(d, lab, 2)
    assert mem.tolist() == list(range(n)) and mptr.tolist() == [0, 2, 132]
    part = np.zeros(64, dtype=F)
    for p in range(2, 132):
        part[p % 64] = F(part[p % 64] + d[0, p])
    assert part[2] == F(2.0 ** 24) and part[3] == 3 and part[0] == 2 and part[4] == 2 and part[63] == 2
    assert sums[0, 1] == SR.tree(part) and abs(float(sums[0, 1]) - (2.0 ** 24 + 127)) <= 1
    seq = F(0)
    for p in range(2, 132):
        seq = F(seq + d[0, p])
    assert seq == F(2.0 ** 24)                                   # the sequential sum loses every 1.0
    # the own position is left out by index: a NaN on the diagonal never enters
    d2 = np.ones((n, n), dtype=F)
    np.fill_diagonal(d2, np.nan)
    s, a, b, _ = SR.samples(d2, lab)
    assert not np.isnan(s).any() and (a == 1).all() and (b == 1).all() and (s == 0).all()


def test_empty_cluster_ids_are_skipped_and_nan_propagates():
    g = np.random.Generator(np.random.PCG64(2))
    n = 40
    d = g.uniform(0.1, 2.0, (n, n)).astype(F)
    lab = g.integers(0, 3, n)
    lab[:3] = (0, 1, 2)
    gap = lab * 3 + 1                                            # ids 1, 4, 7: 0, 2, 3, 5, 6 are empty
    s0 = SR.samples(d, lab)
    s1 = SR.samples(d, gap)
    for u, v in zip(s0[:3], s1[:3]):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    assert np.isfinite(s1[2]).all()                              # an empty cluster is no candidate for b
    # a NaN distance: NaN for the sample whose a or b it enters, nobody else
    d2 = d.copy()
    i, j = 5, int(np.flatnonzero(lab != lab[5])[0])
    d2[i, j] = np.nan
    s2 = SR.samples(d2, lab)[0]
    assert np.isnan(s2[i]) and np.array_equal(np.delete(s2, i).view(np.uint32), np.delete(s0[0], i).view(np.uint32))
    assert np.isnan(SR.score(s2, np.ones(n, bool))) and np.isnan(SR.samples64(d2, lab)[0][i])
    # a cluster of one scores 0 even next to a NaN
    lab3 = lab.copy()
    lab3[i] = 9
    assert SR.samples(d2, lab3)[0][i] == 0
    with pytest.raises(ValueError):
        SR.relabel(lab, 'ignore')


def test_selection_input_has_its_strictly_best_reference_score_at_the_middle_eps():
    """The input of the GPU test of engine.cluster_select, checked here with the float64 evaluator: too tight an eps
    shatters the clusters into singletons (which score 0), too loose merges two of them."""
    x, ids = SR.select_case()
    x64 = x.astype(np.float64)
    negdot = (-(x64 @ x64.T)).astype(F)
    xn = x64 / np.linalg.norm(x64, axis=1, keepdims=True)
    dist = np.clip(1.0 - xn @ xn.T, 0.0, None)
    scores, counts = [], []
    for eps in SR.SELECT_EPS:
        lab = CR.dbscan(x.shape[0], 1, CR.edges(negdot, eps))[0]
        s, _, _, scored = SR.samples64(dist, lab)
        scores.append(SR.score(s, scored))
        counts.append(int(lab.max()) + 1)
    assert counts[0] > 40 and counts[1] == 4 and counts[2] == 3, counts
    assert scores[1] > scores[0] + 0.05 and scores[1] > scores[2] + 0.05, scores
    # the margins of the three thresholds: no pair of samples within 0.02 of an eps, so fp32 dot products decide alike
    off = negdot[~np.eye(x.shape[0], dtype=bool)]
    for eps in SR.SELECT_EPS[1:]:
        assert np.abs(off - eps).min() > 0.02


# ----------------------------------------------------------------------------
# argument checks and the knob
# ----------------------------------------------------------------------------
def test_engine_argument_checks_that_come_before_any_device_work():
    import torch
    from grl_amd import engine
    from grl_amd._lib import GrlHipError
    x = torch.zeros((8, 4))
    lab = torch.zeros(8, dtype=torch.int64)
    vm = engine.VerifyMetric.__new__(engine.VerifyMetric)
    with pytest.raises(ValueError, match='verify_metric'):
        engine.silhouette(x, lab, vm)
    with pytest.raises(ValueError, match="'cosine' or 'euclidean'"):
        engine.silhouette(x, lab, 'manhattan')
    with pytest.raises(ValueError, match="'singleton' or 'drop'"):
        engine.silhouette(x, lab, 'cosine', 'ignore')
    with pytest.raises(ValueError, match="'singleton' or 'drop'"):
        engine.silhouette_matrix(torch.zeros((8, 8)), lab, 'ignore')
    for bad in (lab[:7], lab.float(), lab.bool(), lab.view(2, 4), [0] * 8, None):
        with pytest.raises(ValueError, match='labels must be an integer device tensor'):
            engine.silhouette(x, bad)
        with pytest.raises(ValueError, match='labels must be an integer device tensor'):
            engine.silhouette_matrix(torch.zeros((8, 8)), bad)
    with pytest.raises(ValueError, match=r'xf must be a tensor \[n, d\]'):
        engine.silhouette(torch.zeros(8), lab)
    for bad in (torch.zeros((8, 7)), torch.zeros(8), torch.zeros((2, 2, 2))):
        with pytest.raises(ValueError, match='must be square'):
            engine.silhouette_matrix(bad, lab)
    with pytest.raises(GrlHipError):                              # no CPU path
        engine.silhouette(x, lab)
    with pytest.raises(GrlHipError):
        engine.silhouette_matrix(torch.zeros((8, 8)), lab)
    with pytest.raises(ValueError, match='verify_metric'):
        engine.cluster_select(x, [-0.5], metric=vm)
    with pytest.raises(ValueError, match="'cosine' or 'euclidean'"):
        engine.cluster_select(x, [-0.5], score_metric='manhattan')
    with pytest.raises(ValueError, match='eps_list is empty'):
        engine.cluster_select(x, [])
    with pytest.raises(ValueError, match='eps must be a number'):
        engine.cluster_select(x, [-0.5, float('nan')])
    assert callable(engine.Clustering.silhouette) and callable(engine.KMeans.silhouette)


def test_silhouette_knob_parser():
    from grl_amd.reid.evaluator.attevaluator import parse_silhouette_knob as parse
    for off in (None, '', '   '):
        assert parse('GRL_EVAL_SILHOUETTE', off) is None
    assert parse('X', '1') == ('cosine', 'singleton')
    assert parse('X', 'cosine') == ('cosine', 'singleton')
    assert parse('X', ' euclidean ') == ('euclidean', 'singleton')
    assert parse('X', '1,drop') == ('cosine', 'drop')
    assert parse('X', 'cosine , singleton') == ('cosine', 'singleton')
    assert parse('X', 'euclidean,drop') == ('euclidean', 'drop')
    for bad in ('0', '2', 'on', 'Cosine', 'jaccard', 'cosine,', ',drop', 'cosine,noise', 'cosine,drop,1', 'drop',
                '1,1', 'euclidean;drop'):
        with pytest.raises(ValueError, match='GRL_EVAL_SILHOUETTE'):
            parse('GRL_EVAL_SILHOUETTE', bad)


def test_silhouette_knob_needs_a_clustering_knob(monkeypatch):
    """Setting GRL_EVAL_SILHOUETTE alone is refused before any feature is extracted: the error names all four knobs."""
    from grl_amd.reid.evaluator import ATTEvaluator
    for name in ('GRL_EVAL_CLUSTER', 'GRL_EVAL_CLUSTER_JACCARD', 'GRL_EVAL_KMEANS', 'GRL_EVAL_METRIC', 'GRL_EVAL_STREAM',
                 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_ROC'):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv('GRL_EVAL_SILHOUETTE', 'cosine')
    ev = ATTEvaluator(None, None, only_eval=True)
    with pytest.raises(ValueError) as e:
        ev.evaluate(None, None, None, None, None, 0, 0)
    for name in ('GRL_EVAL_SILHOUETTE', 'GRL_EVAL_CLUSTER', 'GRL_EVAL_CLUSTER_JACCARD', 'GRL_EVAL_KMEANS'):
        assert name in str(e.value)
    monkeypatch.setenv('GRL_EVAL_SILHOUETTE', 'maybe')
    with pytest.raises(ValueError, match='GRL_EVAL_SILHOUETTE'):
        ev.evaluate(None, None, None, None, None, 0, 0)


# ----------------------------------------------------------------------------
# the library's entry points
# ----------------------------------------------------------------------------
ENTRY_POINTS = ('grl_silhouette_block', 'grl_silhouette_finish', 'grl_silhouette_rinv')


def test_lib_binds_the_silhouette_entry_points_at_abi_version_10():
    import os
    from grl_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 10 and lib.grl_abi_version() == 10
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'grl_hip.h')).read()
    assert '#define GRL_ABI_VERSION 10' in header and 'grl_silhouette_*' in header
    for name in ENTRY_POINTS:
        assert name in _lib.exported_symbols() and getattr(lib, name).restype is not None
        assert 'int %s(' % name in header


def test_entry_points_check_their_arguments_before_any_launch():
    from grl_amd import _lib
    lib = _lib.load()
    p = 16                                                       # any non-null address: nothing is dereferenced
    ok = [p, 8, 4, 0, 0, 8, p, p, 2, p, None, None, p, p, p, None]

    def block(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.grl_silhouette_block(*a)
    for i in (0, 6, 7, 9, 12, 13, 14):
        assert block(**{'a%d' % i: None}) == _lib.GRL_EINVAL and b'null' in lib.grl_last_error(), i
    for kw in (dict(a2=-1), dict(a3=-1), dict(a4=-1), dict(a8=0), dict(a8=-2)):
        assert block(**kw) == _lib.GRL_EINVAL and b'>= 0' in lib.grl_last_error(), kw
    for kw in (dict(a5=0), dict(a5=-3), dict(a1=7)):
        assert block(**kw) == _lib.GRL_EINVAL and b'ld >= ncols' in lib.grl_last_error(), kw
    assert block(a3=2 ** 31 - 2) == _lib.GRL_EINVAL and b'int32' in lib.grl_last_error()
    for kw in (dict(a10=p), dict(a11=p)):                        # one factor array without the other
        assert block(**kw) == _lib.GRL_EINVAL and b'go together' in lib.grl_last_error()
    assert block(a2=0) == 0                                      # no rows: nothing to launch
    for i in (0, 1, 2, 3, 6):
        a = [p, p, p, p, 4, 2, p, None]
        a[i] = None
        assert lib.grl_silhouette_finish(*a) == _lib.GRL_EINVAL and b'null' in lib.grl_last_error()
    assert lib.grl_silhouette_finish(p, p, p, p, -1, 2, p, None) == _lib.GRL_EINVAL
    assert lib.grl_silhouette_finish(p, p, p, p, 4, 0, p, None) == _lib.GRL_EINVAL
    assert lib.grl_silhouette_finish(None, None, None, None, 0, 1, None, None) == 0
    assert lib.grl_silhouette_rinv(None, 4, p, None) == _lib.GRL_EINVAL and b'null' in lib.grl_last_error()
    assert lib.grl_silhouette_rinv(p, 4, None, None) == _lib.GRL_EINVAL
    assert lib.grl_silhouette_rinv(p, -1, p, None) == _lib.GRL_EINVAL
    assert lib.grl_silhouette_rinv(None, 0, None, None) == 0
