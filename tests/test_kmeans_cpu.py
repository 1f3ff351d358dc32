"""The host model of the k-means contract (tests/kmeans_ref.py) against float64 sums and scikit-learn,
and the argument checks of engine.kmeans / cluster_centroids and the GRL_EVAL_KMEANS parser that need no device."""
import numpy as np
import pytest

import kmeans_ref as KR


def _data(n=257, d=19, seed=3):
    g = np.random.Generator(np.random.PCG64(seed))
    return (g.standard_normal((n, d)) * g.uniform(0.01, 100.0, (n, 1))).astype(np.float32), g


# ----------------------------------------------------------------------------
# the sum
# ----------------------------------------------------------------------------
def test_model_sum_is_within_the_fp32_summation_bound_of_a_float64_sum():
    """Any order of count - 1 fp32 adds is within (count - 1) u sum|x| (1 + O(u)) of the exact sum, u = 2^-24; the
    contract's bound count * 2^-24 * sum|x| leaves the second-order term room."""
    x, g = _data()
    k = 9
    labels = g.integers(-1, k - 1, x.shape[0])                   # cluster k - 1 stays empty, some samples are nobody's
    labels[:3] = (0, 0, 1)
    s, counts = KR.segment_sum(x, labels, k)
    assert s.dtype == np.float32 and counts[k - 1] == 0 and (labels < 0).any()
    for j in range(k):
        m = np.flatnonzero(labels == j)
        assert counts[j] == m.size
        exact = x[m].astype(np.float64).sum(0)
        bound = m.size * 2.0 ** -24 * np.abs(x[m].astype(np.float64)).sum(0)
        assert (np.abs(s[j].astype(np.float64) - exact) <= bound).all(), j
    assert counts.sum() == (labels >= 0).sum()


def test_model_sum_follows_the_four_way_order_and_not_a_plain_sequential_one():
    """Values chosen so that the order shows: 2^24 absorbs a lone 1.0 but not the 2.0 that two of them make."""
    big, one = np.float32(2.0 ** 24), np.float32(1.0)
    x = np.array([[big], [one], [one], [one], [one], [one]], dtype=np.float32)
    labels = np.zeros(6, dtype=np.int64)
    # partials: p0 = (big + x4) = big, p1 = x1 + x5 = 2, p2 = 1, p3 = 1 -> (big + 2) + 2 = big + 4
    s, _ = KR.segment_sum(x, labels, 1)
    assert s[0, 0] == np.float32(2.0 ** 24 + 4)
    seq = np.float32(0)
    for v in x[:, 0]:
        seq = np.float32(seq + v)
    assert seq == big                                            # the sequential sum loses every 1.0
    # members are taken in ascending sample index whatever the labels' neighbours are
    x2 = np.concatenate((x, x), 0)
    lab2 = np.array([0, 1, 0, 1, 0, 1, 1, 0, 1, 0, 1, 0])
    s2, c2 = KR.segment_sum(x2, lab2, 2)
    for j in (0, 1):
        assert s2[j, 0] == KR.segment_sum(x2[lab2 == j], np.zeros(6, dtype=np.int64), 1)[0][0, 0] and c2[j] == 6


# ----------------------------------------------------------------------------
# empty and NaN rules
# ----------------------------------------------------------------------------
def test_assign_tie_nan_and_signed_zero_rules():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    D = np.array([[3, 1, 1, 2],              # tie -> the smaller index
                  [nan, 5, nan, 5],          # NaN sorts after everything
                  [nan, nan, nan, nan],      # nothing but NaN: unassigned
                  [inf, nan, inf, inf],      # +inf before NaN, tie to the smaller index
                  [0.0, -0.0, 1, 1],         # -0 == +0: the smaller index
                  [-inf, -3, -inf, 0]], dtype=np.float32)
    lab, best = KR.assign(D)
    assert lab.tolist() == [1, 1, -1, 0, 0, 0]
    assert best[:2].tolist() == [1.0, 5.0] and np.isnan(best[2]) and best[3] == inf and best[5] == -inf


def test_reduce_rules_for_empty_clusters_and_unusable_norms():
    x = np.array([[3, 4], [1, 0], [-1, 0], [np.nan, 1], [1e30, 1e30], [1e30, 1e30], [2, 0], [5, 5]], dtype=np.float32)
    labels = np.array([0, 1, 1, 2, 3, 3, 5, -1])                 # 1: sums to zero; 2: NaN; 3: norm overflows; 4: empty
    prev = np.arange(12, dtype=np.float32).reshape(6, 2) + 100
    for p in (None, prev):
        fill = (lambda j: np.zeros(2, np.float32)) if p is None else (lambda j: prev[j])
        s, counts, ne = KR.centroids(x, labels, 6, 'sum', p)
        assert counts.tolist() == [1, 2, 1, 2, 0, 1] and ne == 1
        assert s[0].tolist() == [3, 4] and s[1].tolist() == [0, 0] and np.isnan(s[2, 0]) and s[2, 1] == 1
        assert np.array_equal(s[4], fill(4)) and s[5].tolist() == [2, 0]
        m, _, ne = KR.centroids(x, labels, 6, 'mean', p)
        assert ne == 1 and m[3].tolist() == [np.float32(1e30), np.float32(1e30)] and m[1].tolist() == [0, 0]
        assert np.array_equal(m[4], fill(4)) and np.isnan(m[2, 0])
        u, _, ne = KR.centroids(x, labels, 6, 'unit', p)
        assert ne == 4                                           # zero norm, NaN norm, +inf norm, no members
        assert np.allclose(u[0], [0.6, 0.8], rtol=1e-6, atol=0) and u[5].tolist() == [1, 0]
        for j in (1, 2, 3, 4):
            assert np.array_equal(u[j], fill(j)), (j, p is None)
    with pytest.raises(ValueError):
        KR.centroids(x, labels, 6, 'median')


def test_loop_counts_unassigned_samples_and_keeps_an_empty_centroid():
    x = np.array([[1, 0], [0.9, 0.1], [0, 1], [0.1, 0.9], [np.nan, 0]], dtype=np.float32)
    x[:4] /= np.linalg.norm(x[:4], axis=1, keepdims=True)
    c0 = np.array([[1, 0], [0, 1], [-1, 0]], dtype=np.float32)   # the third attracts nothing
    r = KR.kmeans(x, 3, 'cosine', init=c0, max_iter=10)
    assert r['labels'].tolist() == [0, 0, 1, 1, -1] and r['n_unassigned'] == 1 and r['n_empty'] == 1
    assert r['converged'] and r['n_iter'] == 2 and r['n_changed'] == [5, 0]
    assert np.array_equal(r['centroids'][2], c0[2]) and r['counts'].tolist() == [2, 2, 0]
    assert r['inertia'] == pytest.approx(float(np.float64(KR.assign(KR.cosine_matrix(x, KR.centroids(
        x, r['labels'], 3, 'unit', c0)[0]))[1][:4]).sum()), rel=1e-6)
    one = KR.kmeans(x, 3, 'cosine', init=c0, max_iter=1)
    assert not one['converged'] and one['n_iter'] == 1 and one['n_changed'] == [5]


# ----------------------------------------------------------------------------
# validation
# ----------------------------------------------------------------------------
def test_model_validation():
    x, _ = _data(20, 4)
    for k in (0, -1, 21, 2.0, True, '3'):
        with pytest.raises(ValueError):
            KR.kmeans(x, k, 'euclidean', init='random')
    for it in (0, -5, 1.5, False):
        with pytest.raises(ValueError):
            KR.kmeans(x, 3, 'euclidean', max_iter=it)
    for init in ('kmeans++', [0, 1], [0, 1, 1], [0, 1, 20], [0, -1, 2], [0.0, 1.0, 2.0], np.zeros((3, 5), np.float32)):
        with pytest.raises(ValueError):
            KR.kmeans(x, 3, 'euclidean', init=init)
    with pytest.raises(ValueError):
        KR.kmeans(x, 3, 'manhattan')
    want = np.random.Generator(np.random.PCG64(7)).choice(20, 3, replace=False)
    assert np.array_equal(KR.init_rows(x, 3, 'random', 7), x[want])
    assert np.array_equal(KR.init_rows(x, 3, range(3)), x[:3])


def test_engine_argument_checks_that_come_before_any_device_work():
    """The engine refuses these before it touches a tensor's device, so a host tensor is enough to provoke them."""
    import torch
    from grl_amd import engine
    from grl_amd._lib import GrlHipError
    vm = engine.VerifyMetric.__new__(engine.VerifyMetric)
    x = torch.zeros((8, 4))
    for fn, args in ((engine.kmeans, (x, 2, vm)), (engine.kmeans_assign, (x, x[:2], vm))):
        with pytest.raises(ValueError, match='verify_metric'):
            fn(*args)
    with pytest.raises(ValueError, match="'cosine' or 'euclidean'"):
        engine.kmeans(x, 2, 'manhattan')
    with pytest.raises(GrlHipError):                              # no CPU path
        engine.kmeans(x, 2)
    for bad in (0, -1, True, 2.0, '3', 2 ** 31):
        with pytest.raises(ValueError, match='k must be an integer >= 1'):
            engine._kmeans_int(bad, 1, 'kmeans', 'k')
    for bad in (0, False, 1.0, None):
        with pytest.raises(ValueError, match='max_iter must be an integer >= 1'):
            engine._kmeans_int(bad, 1, 'kmeans', 'max_iter')
    assert engine._kmeans_int(np.int64(5), 1, 'kmeans', 'k') == 5
    assert engine.KMEANS_REDUCE == {'sum': 0, 'mean': 1, 'unit': 2}


def test_kmeans_knob_parser():
    from grl_amd.reid.evaluator.attevaluator import parse_kmeans_knob as parse
    for off in (None, '', '   '):
        assert parse('GRL_EVAL_KMEANS', off) is None
    assert parse('X', '625') == (625, 50, 0)
    assert parse('X', ' 625 , 20 ') == (625, 20, 0)
    assert parse('X', '10,3,7') == (10, 3, 7)
    assert parse('X', 'ids') == ('ids', 50, 0)
    assert parse('X', 'ids,20') == ('ids', 20, 0)
    assert parse('X', 'ids,20,5') == ('ids', 20, 5)
    assert parse('X', '1,1,0') == (1, 1, 0)
    for bad in ('0', '-3', 'abc', '1.5', '10,0', '10,-1', '10,2.5', '10,5,-1', '10,5,x', '1,2,3,4', 'IDs', ',5', 'ids,',
                '10,,3', 'nan', '%d' % 2 ** 31):
        with pytest.raises(ValueError, match='GRL_EVAL_KMEANS'):
            parse('GRL_EVAL_KMEANS', bad)


# ----------------------------------------------------------------------------
# pair_scores through the shared helper
# ----------------------------------------------------------------------------
def test_pair_scores_helper_equals_clustering_pair_scores_on_random_labels():
    import torch
    from grl_amd import engine
    g = np.random.Generator(np.random.PCG64(11))
    for n, k, npid in ((0, 0, 1), (1, 1, 1), (50, 6, 9), (200, 30, 17)):
        lab = g.integers(-1, max(k, 1), n)
        pids = g.integers(0, npid, n)
        t = torch.from_numpy(lab.astype(np.int64))
        cl = engine.Clustering(t, None, None, k, int((lab < 0).sum()), 0, 0, 0.0, 1)
        km = engine.KMeans(t, None, None, 1, False, [n], 0, int((lab < 0).sum()), k, 'cosine', 0.0)
        want = cl.pair_scores(pids)
        assert km.pair_scores(pids) == want == engine._pair_scores(t, k, pids)
        # ... and the pair counts are those of a brute-force count over all pairs
        l2 = lab.copy()
        l2[lab < 0] = k + np.arange((lab < 0).sum())
        iu = np.triu_indices(n, 1)
        same_l, same_p = (l2[:, None] == l2[None, :])[iu], (pids[:, None] == pids[None, :])[iu]
        assert (want['tp'], want['pred_pairs'], want['true_pairs'], want['total_pairs']) == (
            int((same_l & same_p).sum()), int(same_l.sum()), int(same_p.sum()), n * (n - 1) // 2)
    with pytest.raises(ValueError, match='expected 3 pids'):
        engine.KMeans(torch.zeros(3, dtype=torch.int64), None, None, 1, False, [3], 0, 0, 1, 'cosine', 0.0).pair_scores([1])


# ----------------------------------------------------------------------------
# scikit-learn
# ----------------------------------------------------------------------------
def test_model_partition_equals_sklearn_lloyd_on_planted_euclidean_data():
    skc = pytest.importorskip('sklearn.cluster')
    g = np.random.Generator(np.random.PCG64(5))
    kc, d = 10, 8
    centres = g.standard_normal((kc, d)) * 10.0
    planted = np.repeat(np.arange(kc), 30)
    x = (centres[planted] + 0.3 * g.standard_normal((planted.size, d))).astype(np.float32)
    perm = g.permutation(planted.size)
    x, planted = x[perm], planted[perm]
    first = np.array([np.flatnonzero(planted == j)[0] for j in range(kc)])      # one initial row per planted cluster
    r = KR.kmeans(x, kc, 'euclidean', init=first, max_iter=50)
    assert r['converged'] and r['n_empty'] == 0 and r['n_unassigned'] == 0
    sk = skc.KMeans(n_clusters=kc, init=x[first].astype(np.float64), n_init=1, algorithm='lloyd', max_iter=50,
                    tol=0.0).fit(x.astype(np.float64))
    assert KR.same_partition(r['labels'], sk.labels_)
    assert KR.same_partition(r['labels'], planted)
    assert not KR.same_partition(r['labels'], np.where(np.arange(planted.size) == 0, (planted[0] + 1) % kc, planted))
    assert r['inertia'] == pytest.approx(sk.inertia_, rel=1e-4)
