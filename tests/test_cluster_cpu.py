"""The clustering contract on the host: the numpy model of tests/cluster_ref.py against scikit-learn's
DBSCAN, the either-direction rule on asymmetric matrices, Clustering.pair_scores against sklearn's pair counts, the
GRL_EVAL_CLUSTER parser, the bindings and PairRoc.eer_threshold.  No GPU is needed."""
import numpy as np
import pytest
import torch

import cluster_ref as CR
import roc_ref as R


def _symmetric(n, seed):
    """A symmetric float32 matrix with four tight groups, a few points half-way between two of them and scattered points:
    values up to 0.5 are edges.  The points in between are non-core points next to one or to two clusters."""
    g = np.random.Generator(np.random.PCG64(seed))
    centres = 0.96 * np.array([(0, 0), (1, 0), (0, 1), (1, 1)]) + 0.05 * g.standard_normal((4, 2))
    mids = 0.5 * (centres[[0, 0, 1, 2]] + centres[[1, 2, 3, 3]])     # between two groups: within 0.5 of both, or of neither
    k = n // 6
    pts = np.concatenate((centres[g.integers(0, 4, n - 2 * k)] + 0.08 * g.standard_normal((n - 2 * k, 2)),
                          mids[g.integers(0, 4, k)] + 0.06 * g.standard_normal((k, 2)),
                          1.5 * g.standard_normal((k, 2))))
    pts = pts[g.permutation(n)]
    D = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1)).astype(np.float32)
    return np.minimum(D, D.T)


def test_model_equals_sklearn_dbscan_on_symmetric_matrices():
    from sklearn.cluster import DBSCAN
    ambiguous = borders = noise = 0
    for seed in range(120):
        n = 30 + seed % 25
        D = _symmetric(n, seed)
        for min_samples in (1, 2, 4, 7):
            A = CR.edges(D, 0.5)
            labels, core = CR.dbscan(n, min_samples, A=A)
            X = np.where(D <= np.float32(0.5), 0.0, 1.0)         # sklearn refuses negative distances; ties stay put
            np.fill_diagonal(X, 0.0)                             # a point counts itself
            sk = DBSCAN(eps=0.5, min_samples=min_samples, metric='precomputed').fit(X)
            assert np.array_equal(labels, sk.labels_), (seed, min_samples)
            assert np.array_equal(np.flatnonzero(core), sk.core_sample_indices_), (seed, min_samples)
            # the same from the CSR form
            l2, c2 = CR.dbscan(n, min_samples, *(None,) + CR.csr(A))
            assert np.array_equal(l2, labels) and np.array_equal(c2, core)
            for j in np.flatnonzero(~core & (labels >= 0)):
                borders += 1
                ambiguous += len(set(labels[A[j] & core])) > 1
            noise += int((labels < 0).sum())
    print('border points %d, of them next to two clusters %d, noise %d' % (borders, ambiguous, noise))
    assert ambiguous > 10 and borders > 200 and noise > 200      # the cases exercise the border rule


def test_model_follows_the_either_direction_rule_on_asymmetric_matrices():
    inf = np.float32(np.inf)
    # three points, one edge stored in one direction only: 0 -> 1.  min_samples 1: {0, 1} and {2}.
    D = np.full((3, 3), inf, dtype=np.float32)
    D[0, 1] = 0.0
    labels, core = CR.dbscan(3, 1, A=CR.edges(D, 0.5))
    assert labels.tolist() == [0, 0, 1] and core.all()
    # min_samples 2: only 0 has an out-edge, so only 0 is core; 1 is its border point through 0's row
    labels, core = CR.dbscan(3, 2, A=CR.edges(D, 0.5))
    assert labels.tolist() == [0, 0, -1] and core.tolist() == [True, False, False]
    # a border point reachable only through the cores' rows, next to two clusters: it takes the smaller id.
    # cores 1 <-> 2 (cluster 0, root 1) and 3 <-> 4 (cluster 1); 4 -> 0 and 2 -> 0 are stored, row 0 is empty
    D = np.full((5, 5), inf, dtype=np.float32)
    for i, j in ((1, 2), (2, 1), (3, 4), (4, 3), (4, 0), (2, 0)):
        D[i, j] = 0.25
    D[0, 0] = -1.0                                               # the diagonal is never an edge
    labels, core = CR.dbscan(5, 2, A=CR.edges(D, 0.25))          # the edge is inclusive
    assert core.tolist() == [False, True, True, True, True] and labels.tolist() == [0, 0, 0, 1, 1]
    assert CR.dbscan(5, 2, A=CR.edges(D, np.nextafter(np.float32(0.25), np.float32(0))))[0].tolist() == [-1] * 5
    # NaN is never an edge, +inf as eps means FLT_MAX: an infinite entry stays outside
    D = np.array([[0, np.nan, inf], [1, 0, -inf], [3e38, 2, 0]], dtype=np.float32)
    assert CR.edges(D, np.inf).tolist() == [[False, False, False], [True, False, True], [True, True, False]]
    assert CR.edges(D, -np.inf).tolist() == [[False, False, False], [False, False, True], [False, False, False]]


def _clustering(labels):
    from grl_amd import engine
    labels = torch.as_tensor(np.asarray(labels, dtype=np.int64))
    k = int(labels.max()) + 1 if labels.numel() and int(labels.max()) >= 0 else 0
    return engine.Clustering(labels, None, None, k, int((labels < 0).sum()), 0, 0, None, 1)


def test_pair_scores_equal_sklearn_pair_counts_and_adjusted_rand():
    from sklearn.metrics import adjusted_rand_score
    from sklearn.metrics.cluster import pair_confusion_matrix
    g = np.random.Generator(np.random.PCG64(5))
    for case in range(60):
        n = int(g.integers(2, 400))
        pids = g.integers(0, max(1, n // int(g.integers(1, 9))), n) * 7 - 3
        labels = g.integers(-1, max(1, n // int(g.integers(1, 9))), n)
        if case % 5 == 0:                                        # no noise, ids without gaps
            labels = np.unique(labels, return_inverse=True)[1].reshape(-1)
        s = _clustering(labels).pair_scores(pids)
        single = labels.astype(np.int64).copy()                  # noise points are singletons
        single[labels < 0] = labels.max() + 1 + np.arange((labels < 0).sum())
        (tn, fp), (fn, tp) = pair_confusion_matrix(pids, single) // 2
        assert (s['tp'], s['pred_pairs'], s['true_pairs'], s['total_pairs']) == (tp, tp + fp, tp + fn, n * (n - 1) // 2)
        assert s['n'] == n and all(isinstance(s[k], int) for k in ('tp', 'pred_pairs', 'true_pairs', 'total_pairs'))
        assert s['ari'] == pytest.approx(adjusted_rand_score(pids, single), abs=1e-12)
        p = tp / (tp + fp) if tp + fp else 1.0
        r = tp / (tp + fn) if tp + fn else 1.0
        assert s['precision'] == pytest.approx(p, abs=1e-12) and s['recall'] == pytest.approx(r, abs=1e-12)
        assert s['f1'] == pytest.approx(2 * p * r / (p + r) if p + r else 0.0, abs=1e-12)
        assert all(isinstance(s[k], float) for k in ('precision', 'recall', 'f1', 'ari'))
    # the 0 / 0 cases
    s = _clustering([-1, -1, -1]).pair_scores([4, 4, 5])         # nothing predicted together
    assert (s['precision'], s['recall'], s['f1'], s['pred_pairs'], s['true_pairs']) == (1.0, 0.0, 0.0, 0, 1)
    s = _clustering([0, 0, 1]).pair_scores([1, 2, 3])            # no two samples share a pid
    assert (s['precision'], s['recall'], s['true_pairs'], s['pred_pairs']) == (0.0, 1.0, 0, 1)
    s = _clustering([0, 1, -1]).pair_scores([1, 2, 3])           # neither: a perfect answer
    assert (s['precision'], s['recall'], s['f1'], s['ari']) == (1.0, 1.0, 1.0, 1.0)
    for labels in ([], [0]):                                     # n = 0 and n = 1
        s = _clustering(labels).pair_scores(labels)
        assert (s['precision'], s['recall'], s['ari'], s['total_pairs'], s['n']) == (1.0, 1.0, 1.0, 0, len(labels))
    with pytest.raises(ValueError, match='pids'):
        _clustering([0, 0]).pair_scores([1])


def test_parse_cluster_knob():
    from grl_amd.reid.evaluator.attevaluator import parse_cluster_knob as parse
    for off in (None, '', '   '):
        assert parse('GRL_EVAL_CLUSTER', off) is None
    assert parse('GRL_EVAL_CLUSTER', '-0.7') == (-0.7, 1)
    assert parse('GRL_EVAL_CLUSTER', ' -0.55 , 4 ') == (-0.55, 4)
    assert parse('GRL_EVAL_CLUSTER', 'eer') == ('eer', 1) and parse('GRL_EVAL_CLUSTER', 'eer,2') == ('eer', 2)
    assert parse('GRL_EVAL_CLUSTER', '1e-3,1') == (1e-3, 1) and parse('GRL_EVAL_CLUSTER', 'inf') == (float('inf'), 1)
    for bad in ('x', 'EER', 'eer,', ',2', '-0.7,0', '-0.7,-1', '-0.7,1.5', '-0.7,two', 'nan', 'nan,2', '-0.7,2,3',
                '-0.7;2'):
        with pytest.raises(ValueError, match='GRL_EVAL_CLUSTER'):
            parse('GRL_EVAL_CLUSTER', bad)


class _Never(object):
    def __getattr__(self, name):
        raise AssertionError('touched %s' % name)


KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_CLUSTER')


def test_bad_knob_and_the_verify_metric_are_refused_before_any_feature_is_extracted(monkeypatch):
    from grl_amd.reid.evaluator import ATTEvaluator
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv('GRL_EVAL_CLUSTER', '-0.7,0')
    with pytest.raises(ValueError, match='GRL_EVAL_CLUSTER'):
        ATTEvaluator(_Never(), _Never(), False).evaluate(None, None, _Never(), _Never(), '', 0, 0)
    monkeypatch.setenv('GRL_EVAL_CLUSTER', 'eer,2')
    for metric in ('verify', 'verify,0.5'):
        monkeypatch.setenv('GRL_EVAL_METRIC', metric)
        with pytest.raises(ValueError, match='GRL_EVAL_CLUSTER.*signed logit'):
            ATTEvaluator(_Never(), _Never(), False).evaluate(None, None, _Never(), _Never(), '', 0, 0)


ENTRY_POINTS = ('grl_cluster_edges_block', 'grl_cluster_init', 'grl_cluster_round', 'grl_cluster_border',
                'grl_cluster_roots', 'grl_cluster_labels')


def test_lib_binds_the_clustering_entry_points_at_abi_version_10():
    import os
    from grl_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 10 and lib.grl_abi_version() == 10
    for name in ENTRY_POINTS:
        assert name in _lib.exported_symbols() and getattr(lib, name).restype is not None
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'grl_hip.h')).read()
    assert '#define GRL_ABI_VERSION 10' in header
    for name in ENTRY_POINTS:
        assert 'int %s(' % name in header


def test_entry_points_check_their_arguments_before_any_launch():
    from grl_amd import _lib
    lib = _lib.load()
    p = 16                                                       # any non-null address: nothing is dereferenced
    ok = [p, 8, 4, 0, 0, 8, -0.5, p, None, None, None]           # the count pass

    def edges(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.grl_cluster_edges_block(*a)
    for kw in (dict(a0=None), dict(a7=None)):
        assert edges(**kw) == _lib.GRL_EINVAL and b'null' in lib.grl_last_error()
    for kw in (dict(a2=-1), dict(a5=0), dict(a5=-3), dict(a3=-1), dict(a4=-1), dict(a1=7)):
        assert edges(**kw) == _lib.GRL_EINVAL and b'bad shape' in lib.grl_last_error()
    assert edges(a6=float('nan')) == _lib.GRL_EINVAL and b'NaN' in lib.grl_last_error()
    for kw in (dict(a8=p), dict(a9=p)):                          # row_ptr without col, col without row_ptr
        assert edges(**kw) == _lib.GRL_EINVAL and b'fill pass' in lib.grl_last_error()
    assert edges(a2=0) == 0                                      # no rows: nothing to launch
    for m in (0, -1):
        assert lib.grl_cluster_init(p, 4, m, p, p, p, None) == _lib.GRL_EINVAL and b'min_samples' in lib.grl_last_error()
    assert lib.grl_cluster_init(p, -1, 1, p, p, p, None) == _lib.GRL_EINVAL
    for i in (0, 3, 4, 5):
        a = [p, 4, 1, p, p, p, None]
        a[i] = None
        assert lib.grl_cluster_init(*a) == _lib.GRL_EINVAL and b'null' in lib.grl_last_error()
    assert lib.grl_cluster_init(None, 0, 1, None, None, None, None) == 0
    assert lib.grl_cluster_round(p, p, p, p, 4, None, None) == _lib.GRL_EINVAL
    assert lib.grl_cluster_round(None, p, p, p, 4, p, None) == _lib.GRL_EINVAL
    assert lib.grl_cluster_round(p, p, p, p, -1, p, None) == _lib.GRL_EINVAL
    assert lib.grl_cluster_border(p, p, p, p, 4, None, None) == _lib.GRL_EINVAL
    assert lib.grl_cluster_roots(p, None, 4, p, None) == _lib.GRL_EINVAL
    assert lib.grl_cluster_labels(p, p, p, None, 4, p, None) == _lib.GRL_EINVAL
    assert lib.grl_cluster_labels(p, p, p, p, -2, p, None) == _lib.GRL_EINVAL


def test_engine_refuses_bad_arguments_before_touching_the_device():
    from grl_amd import engine
    x = torch.zeros((4, 8))                                      # a host tensor: reaching the device path would raise GrlHipError
    for eps in (float('nan'), np.float32('nan'), None, 'eer', True):
        with pytest.raises(ValueError, match='eps'):
            engine.cluster(x, eps)
        with pytest.raises(ValueError, match='eps'):
            engine.eps_graph(x, eps)
        with pytest.raises(ValueError, match='eps'):
            engine.cluster_matrix(x, eps)
    for m in (0, -2, 1.0, 2.5, True, None, '2'):
        with pytest.raises(ValueError, match='min_samples'):
            engine.cluster(x, -0.5, min_samples=m)
        with pytest.raises(ValueError, match='min_samples'):
            engine.cluster_matrix(x, -0.5, min_samples=m)
        with pytest.raises(ValueError, match='min_samples'):
            engine.cluster_from_graph(None, None, 4, min_samples=m)
    with pytest.raises(ValueError, match='metric'):
        engine.cluster(x, -0.5, metric='manhattan')
    vm = engine.VerifyMetric.__new__(engine.VerifyMetric)       # (no device state is needed to be refused)
    with pytest.raises(ValueError, match='signed logit'):
        engine.eps_graph(x, -0.5, metric=vm)
    with pytest.raises(ValueError, match='signed logit'):
        engine.cluster(x, -0.5, metric=vm)
    assert engine.CLUSTER_MAX_EDGES == 1 << 28 or 'GRL_CLUSTER_MAX_EDGES' in __import__('os').environ


def test_eer_threshold_is_the_curve_threshold_of_the_boundary_eer_selects():
    from grl_amd import engine
    pos, neg = np.zeros(256, dtype=np.int64), np.zeros(256, dtype=np.int64)
    pos[[10, 20, 30, 40]] = (6, 2, 1, 1)                         # TPR after each bin: 0.6, 0.8, 0.9, 1.0
    neg[[10, 20, 30, 40]] = (1, 2, 3, 4)                         # FPR:                0.1, 0.3, 0.6, 1.0
    roc = engine.PairRoc(torch.from_numpy(pos), torch.from_numpy(neg), 8)
    t = roc.eer_threshold                                        # FPR >= 1 - TPR first holds after bin 20
    assert isinstance(t, np.float32) and t == roc.curve()[2][1]
    # bin 20 of 8 bits: keys 0x14000000 .. 0x14ffffff; a key with the top bit clear is the complement of a negative float
    assert t == np.array([0xffffffff ^ 0x14ffffff], dtype=np.uint32).view(np.float32)[0]
    assert R.bins(np.array([t]), 8).tolist() == [20]
    assert R.bins(np.nextafter(np.array([t]), np.float32(np.inf)), 8).tolist() == [21]
    assert 0.1 < roc.eer < 0.3 and roc.eer == pytest.approx(R.eer(pos, neg), abs=1e-14)      # (unchanged)
    # the first boundary already qualifies: everything in one bin
    pos[:], neg[:] = 0, 0
    pos[77], neg[77] = 3, 5
    roc = engine.PairRoc(torch.from_numpy(pos), torch.from_numpy(neg), 8)
    assert roc.eer_threshold == roc.curve()[2][0] and R.bins(np.array([roc.eer_threshold]), 8).tolist() == [77]
