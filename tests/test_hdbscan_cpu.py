"""The host model of the HDBSCAN contract (tests/hdbscan_ref.py) against scipy's minimum spanning tree and
scikit-learn's HDBSCAN, the host cut of engine.hdbscan_from_mst against the model on hand-built forests, and the
argument checks and the GRL_EVAL_HDBSCAN parser that need no device.

The comparison with scikit-learn is one of partitions on the cases where a throw-away model of the contract agreed with
scikit-learn 1.7.2: mutual-reachability weights tie structurally (many edges share a core distance), and scikit-learn's
dendrogram breaks such ties by its own sort, so other (min_cluster_size, min_samples) differ by a sample or two; there
the model alone is the yardstick."""
import os

import numpy as np
import pytest

import hdbscan_ref as HR
import silhouette_ref as SR

F = np.float32
SK_CASES = [(2, 1), (5, 2), (10, 3)]

_case = {}


def matrices(x):
    """(cosine, euclidean) float32 distance matrices of the rows x by the model's chains from sequential fp32 dot
    products; both are bitwise symmetric (x_i * x_j commutes, and every later step takes the pair lo first)."""
    n = x.shape[0]
    dot = np.zeros((n, n), dtype=F)
    sq = np.zeros(n, dtype=F)
    for c in range(x.shape[1]):
        dot = (dot + (x[:, c, None] * x[None, :, c]).astype(F)).astype(F)
        sq = (sq + (x[:, c] * x[:, c]).astype(F)).astype(F)
    i, j = np.arange(n)[:, None], np.arange(n)[None, :]
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    t = ((sq[lo] + sq[hi]).astype(F) - (F(2.0) * dot).astype(F)).astype(F)
    return HR.cosine_matrix(-dot, sq), np.sqrt(np.maximum(t, F(1e-12))).astype(F)


def case():
    if not _case:
        x, ids = SR.planted(d=24)
        _case['x'], _case['ids'] = x, ids
        _case['cosine'], _case['euclidean'] = matrices(x)
        _case['forest'] = {}
    return _case


def forest(metric, ms):
    c = case()
    if (metric, ms) not in c['forest']:
        c['forest'][metric, ms] = HR.forest(c[metric], ms)
    return c['forest'][metric, ms]


# ----------------------------------------------------------------------------
# the model's forest
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_model_forest_has_the_weights_of_scipys_minimum_spanning_tree(metric):
    from scipy.sparse import csgraph
    c = case()
    d = c[metric]
    n = d.shape[0]
    assert n == 336 and np.array_equal(d.view(np.uint32), d.T.view(np.uint32))
    assert (d[~np.eye(n, dtype=bool)] > 0).all()                 # scipy reads 0 as "no edge"
    for ms in (1, 2, 5):
        lo, hi, w, core = forest(metric, ms)
        m = HR.reachability_matrix(d, core).astype(np.float64)
        assert np.isfinite(m[~np.eye(n, dtype=bool)]).all()
        np.fill_diagonal(m, 0.0)
        want = np.sort(csgraph.minimum_spanning_tree(m).data)
        assert w.size == n - 1 and np.array_equal(np.sort(w.astype(np.float64)), want)
        assert (lo < hi).all() and np.array_equal(np.lexsort((hi, lo, w)), np.arange(n - 1))
        # the core distance is the distance to the (ms - 1)-th nearest other sample
        off = np.where(np.eye(n, dtype=bool), np.inf, d)
        want_core = np.sort(off, axis=1)[:, ms - 2] if ms > 1 else np.zeros(n, dtype=F)
        assert np.array_equal(core, want_core)


def test_model_core_distance_deletes_the_sample_by_index_or_the_last_entry():
    d = np.array([[5, 1, 2, 3],                                  # the diagonal is not the smallest entry of row 0
                  [1, 0, 4, 6],
                  [2, 4, 0, 0],                                  # a tie at 0 with a larger index: the sample comes first
                  [3, 6, 0, 0]], dtype=F)
    assert HR.core_distances(d, 1).tolist() == [0, 0, 0, 0]
    assert HR.core_distances(d, 2).tolist() == [1, 1, 0, 0]      # row 0: {1, 2} minus the last; row 3: {2, 3} minus 3
    assert HR.core_distances(d, 3).tolist() == [2, 4, 2, 3]
    assert HR.core_distances(d, 4).tolist() == [3, 6, 4, 6]
    lo, hi, w = HR.weights(d, np.array([0, np.nan, 0, np.inf], dtype=F))
    assert (lo.tolist(), hi.tolist(), w.tolist()) == ([0], [2], [2.0])      # no core distance, no edges


# ----------------------------------------------------------------------------
# the cut on hand-built forests: the model, and the engine's host cut against it
# ----------------------------------------------------------------------------
def both_cuts(edges, n, mcs, method):
    from grl_amd import engine
    edges = sorted(edges, key=lambda e: (e[2], e[0], e[1]))
    lo, hi, w = [e[0] for e in edges], [e[1] for e in edges], np.array([e[2] for e in edges], dtype=F)
    labels, stab = HR.cut(lo, hi, w, n, mcs, method)
    got, k, gstab = engine._hdbscan_cut(lo, hi, w.astype(np.float64), n, mcs, method)
    assert np.array_equal(got, labels) and k == stab.size and np.array_equal(gstab, stab)
    return labels.tolist(), stab.tolist()


@pytest.mark.parametrize('method', ['eom', 'leaf'])
def test_cut_of_a_chain(method):
    chain = [(0, 1, 1.0), (1, 2, 1.0), (2, 3, 10.0), (3, 4, 1.0), (4, 5, 1.0)]
    for mcs in (2, 3):
        labels, stab = both_cuts(chain, 6, mcs, method)
        assert labels == [0, 0, 0, 1, 1, 1]
        assert stab == pytest.approx([2.7, 2.7], rel=1e-15)      # 3 points leave at lambda = 1, born at 0.1
    # no split with both sides >= 4: the one component is the root, which is never selected
    assert both_cuts(chain, 6, 4, method)[0] == [-1] * 6
    # a rising chain never splits
    assert both_cuts([(i, i + 1, 1.0 + i) for i in range(5)], 6, 2, method)[0] == [-1] * 6
    # nested: {0,1,2} and {3,4,5} at 1 join at 4, {6,7,8} and {9,10,11} at 1 join at 2, the halves join at 10
    nested = ([(i, i + 1, 1.0) for i in (0, 1, 3, 4, 6, 7, 9, 10)] + [(2, 3, 4.0), (8, 9, 2.0), (5, 6, 10.0)])
    labels, stab = both_cuts(nested, 12, 3, method)
    # left half: S = 6 (1/4 - 1/10) = 0.9 against 2 * 3 (1 - 1/4) = 4.5: the children; right: 6 (1/2 - 1/10) = 2.4
    # against 2 * 3 (1 - 1/2) = 3: the children too
    assert labels == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3
    assert stab == pytest.approx([2.25, 2.25, 1.5, 1.5], rel=1e-15)
    # pulled apart less (joins at 1.25 and 1.5), the halves win under eom and the leaves under leaf
    close = ([(i, i + 1, 1.0) for i in (0, 1, 3, 4, 6, 7, 9, 10)] + [(2, 3, 1.25), (8, 9, 1.5), (5, 6, 10.0)])
    labels, stab = both_cuts(close, 12, 3, method)
    if method == 'eom':                                          # 6 (0.8 - 0.1) = 4.2 > 6 * 0.2; 6 (2/3 - 0.1) = 3.4 > 6 / 3
        assert labels == [0] * 6 + [1] * 6 and stab == pytest.approx([4.2, 3.4], rel=1e-15)
    else:
        assert labels == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3


@pytest.mark.parametrize('method', ['eom', 'leaf'])
def test_cut_of_a_forest_of_several_trees_follows_the_virtual_root_rule(method):
    a = [(0, 1, 1.0), (1, 2, 1.0)]
    b = [(3, 4, 2.0), (4, 5, 2.0), (5, 6, 2.0)]
    # two components of at least 3 samples and a loner: both are selectable clusters born at lambda = 0
    labels, stab = both_cuts(a + b, 8, 3, method)
    assert labels == [0, 0, 0, 1, 1, 1, 1, -1] and stab == [3.0, 2.0]
    # only one of them reaches 4 samples: it is the root, never selected, and the smaller one is noise
    assert both_cuts(a + b, 8, 4, method)[0] == [-1] * 8
    assert both_cuts(b, 8, 3, method)[0] == [-1] * 8
    # none reaches 5; no edges at all
    assert both_cuts(a + b, 8, 5, method)[0] == [-1] * 8
    assert both_cuts([], 3, 2, method) == ([-1] * 3, [])
    assert both_cuts([], 0, 2, method) == ([], [])
    # numbering: by the clusters' smallest sample index, whatever their weights
    labels, stab = both_cuts([(0, 5, 2.0), (5, 6, 2.0), (1, 2, 1.0), (2, 3, 1.0)], 7, 3, method)
    assert labels == [0, 1, 1, 1, -1, 0, 0] and stab == [1.5, 3.0]


@pytest.mark.parametrize('method', ['eom', 'leaf'])
def test_cut_with_all_equal_weights_and_with_zero_weights(method):
    # every weight equal: the dendrogram follows the order (w, lo, hi), a comb that never splits
    assert both_cuts([(i, i + 1, 1.0) for i in range(7)], 8, 2, method)[0] == [-1] * 8
    labels, stab = both_cuts([(i, i + 1, 1.0) for i in (0, 1, 2, 4, 5, 6)], 8, 2, method)
    assert labels == [0] * 4 + [1] * 4 and stab == [4.0, 4.0]
    # duplicates: w = 0 has lambda = 2^126, finite in float64
    dup = [(0, 1, 0.0), (1, 2, 0.0), (3, 4, 0.0), (4, 5, 0.0), (2, 3, 1.0)]
    for mcs in (2, 3):
        labels, stab = both_cuts(dup, 6, mcs, method)
        assert labels == [0, 0, 0, 1, 1, 1] and np.isfinite(stab).all()
        assert stab == pytest.approx([3 * 2.0 ** 126] * 2, rel=1e-15)
    # -0 and a negative weight take the floor too
    assert both_cuts([(0, 1, -0.0), (1, 2, -3.0), (3, 4, 0.0), (4, 5, 0.0), (2, 3, 1.0)], 6, 3, method)[0] == [0] * 3 + [1] * 3


# ----------------------------------------------------------------------------
# the model's partition against scikit-learn
# ----------------------------------------------------------------------------
def sklearn_labels(d, mcs, ms, method):
    import sklearn.cluster as skc
    d64 = np.minimum(d, d.T).astype(np.float64)
    np.fill_diagonal(d64, 0.0)
    return skc.HDBSCAN(min_cluster_size=mcs, min_samples=ms, metric='precomputed', allow_single_cluster=False,
                       cluster_selection_method=method).fit(d64).labels_


@pytest.mark.parametrize('method', ['eom', 'leaf'])
@pytest.mark.parametrize('mcs,ms', SK_CASES)
@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_model_partition_is_sklearns(metric, mcs, ms, method):
    c = case()
    lo, hi, w, _ = forest(metric, ms)
    labels, stab = HR.cut(lo, hi, w, 336, mcs, method)
    want = sklearn_labels(c[metric], mcs, ms, method)
    assert labels.max() + 1 == stab.size >= 2 and (stab > 0).all()
    assert HR.same_partition(labels, want), (int((labels != -1).sum()), int((want != -1).sum()))
    # the numbering: ascending in each cluster's smallest sample index
    first = [int(np.flatnonzero(labels == k)[0]) for k in range(stab.size)]
    assert first == sorted(first)


def test_engine_cut_equals_the_model_on_the_planted_forest():
    from grl_amd import engine
    for metric, ms in (('cosine', 2), ('euclidean', 5)):
        lo, hi, w, _ = forest(metric, ms)
        for mcs in (2, 5, 10, 60):
            for method in ('eom', 'leaf'):
                labels, stab = HR.cut(lo, hi, w, 336, mcs, method)
                got, k, gstab = engine._hdbscan_cut(lo.tolist(), hi.tolist(), w.astype(np.float64), 336, mcs, method)
                assert np.array_equal(got, labels) and k == stab.size and np.array_equal(gstab, stab)


# ----------------------------------------------------------------------------
# argument checks and the knob
# ----------------------------------------------------------------------------
def test_engine_argument_checks_that_come_before_any_device_work():
    import torch
    from grl_amd import engine
    from grl_amd._lib import GrlHipError
    x = torch.zeros((8, 4))
    m = torch.zeros((8, 8))
    vm = engine.VerifyMetric.__new__(engine.VerifyMetric)
    with pytest.raises(ValueError, match='verify_metric'):
        engine.hdbscan(x, metric=vm)
    with pytest.raises(ValueError, match='verify_metric'):
        engine.mutual_reachability_mst(x, 2, vm)
    with pytest.raises(ValueError, match="'cosine' or 'euclidean'"):
        engine.hdbscan(x, metric='manhattan')
    for bad in (1, 0, -3, True, 2.0, '5', None):
        with pytest.raises(ValueError, match='min_cluster_size'):
            engine.hdbscan(x, bad)
        with pytest.raises(ValueError, match='min_cluster_size'):
            engine.hdbscan_matrix(m, bad)
    for bad in (0, -1, 1025, 9, True, 2.0, '2'):                 # 9 > n = 8
        with pytest.raises(ValueError, match='min_samples'):
            engine.hdbscan(x, 5, bad)
        with pytest.raises(ValueError, match='min_samples'):
            engine.hdbscan_matrix(m, 5, bad)
        with pytest.raises(ValueError, match='min_samples'):
            engine.mutual_reachability_mst(x, bad)
    with pytest.raises(ValueError, match='min_samples'):          # the default min_samples = min_cluster_size > n
        engine.hdbscan(x, 9)
    for bad in ('EOM', 'tree', None, 1):
        with pytest.raises(ValueError, match="'eom' or 'leaf'"):
            engine.hdbscan(x, method=bad)
        with pytest.raises(ValueError, match="'eom' or 'leaf'"):
            engine.hdbscan_matrix(m, method=bad)
    for bad in (torch.zeros((8, 7)), torch.zeros(8), torch.zeros((2, 2, 2)), None):
        with pytest.raises(ValueError, match='must be square'):
            engine.hdbscan_matrix(bad)
    with pytest.raises(ValueError, match='float32'):
        engine.hdbscan_matrix(m.double())
    with pytest.raises(ValueError, match=r'xf must be a tensor \[n, d\]'):
        engine.hdbscan(torch.zeros(8))
    with pytest.raises(GrlHipError):                              # no CPU path
        engine.hdbscan(x, 2)
    with pytest.raises(GrlHipError):
        engine.hdbscan_matrix(m, 2)
    e = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match='min_cluster_size'):
        engine.hdbscan_from_mst(e, e, torch.zeros(3), 8, 1)
    with pytest.raises(ValueError, match="'eom' or 'leaf'"):
        engine.hdbscan_from_mst(e, e, torch.zeros(3), 8, 2, 'best')
    with pytest.raises(ValueError, match='one entry per edge'):
        engine.hdbscan_from_mst(e, e[:2], torch.zeros(3), 8, 2)
    with pytest.raises(ValueError, match='one entry per edge'):
        engine.hdbscan_from_mst(e.long(), e, torch.zeros(3), 8, 2)
    with pytest.raises(GrlHipError):
        engine.hdbscan_from_mst(e, e, torch.zeros(3), 8, 2)
    for name in ('pair_scores', 'centroids', 'silhouette'):
        assert callable(getattr(engine.Hdbscan, name))


def test_hdbscan_knob_parser():
    from grl_amd.reid.evaluator.attevaluator import parse_hdbscan_knob as parse
    for off in (None, '', '   '):
        assert parse('GRL_EVAL_HDBSCAN', off) is None
    assert parse('X', '5') == (5, None, 'eom')
    assert parse('X', ' 2 , 1 ') == (2, 1, 'eom')
    assert parse('X', '10,3,leaf') == (10, 3, 'leaf')
    assert parse('X', '10,1024,eom') == (10, 1024, 'eom')
    for bad in ('1', '0', '-5', 'five', '5,', '5,0', '5,1025', '5,2,', '5,2,best', '5,leaf', '5,2,eom,1', '5;2', '2.5'):
        with pytest.raises(ValueError, match='GRL_EVAL_HDBSCAN'):
            parse('GRL_EVAL_HDBSCAN', bad)


def test_hdbscan_knob_is_refused_with_the_verification_metric(monkeypatch):
    """As GRL_EVAL_KMEANS is: before any feature is extracted."""
    from grl_amd.reid.evaluator import ATTEvaluator
    for name in ('GRL_EVAL_CLUSTER', 'GRL_EVAL_CLUSTER_JACCARD', 'GRL_EVAL_KMEANS', 'GRL_EVAL_SILHOUETTE', 'GRL_EVAL_STREAM',
                 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_ROC'):
        monkeypatch.delenv(name, raising=False)
    ev = ATTEvaluator(None, None, only_eval=True)
    monkeypatch.setenv('GRL_EVAL_METRIC', 'verify')
    monkeypatch.setenv('GRL_EVAL_HDBSCAN', '5')
    with pytest.raises(ValueError, match='GRL_EVAL_HDBSCAN cannot be combined with GRL_EVAL_METRIC=verify'):
        ev.evaluate(None, None, None, None, None, 0, 0)
    monkeypatch.delenv('GRL_EVAL_METRIC')
    monkeypatch.setenv('GRL_EVAL_HDBSCAN', '1')
    with pytest.raises(ValueError, match='GRL_EVAL_HDBSCAN'):
        ev.evaluate(None, None, None, None, None, 0, 0)


# ----------------------------------------------------------------------------
# the library's entry points
# ----------------------------------------------------------------------------
ENTRY_POINTS = ('grl_hdbscan_minedge_block', 'grl_hdbscan_cosine_block')


def test_lib_binds_the_hdbscan_entry_points_at_abi_version_10():
    from grl_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 10 and lib.grl_abi_version() == 10
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'grl_hip.h')).read()
    assert '#define GRL_ABI_VERSION 10' in header and 'grl_hdbscan_*' in header
    for name in ENTRY_POINTS:
        assert name in _lib.exported_symbols() and getattr(lib, name).restype is not None
        assert 'int %s(' % name in header


def test_entry_points_check_their_arguments_before_any_launch():
    from grl_amd import _lib
    lib = _lib.load()
    p = 16                                                       # any non-null address: nothing is dereferenced
    ok = [p, 8, 8, 4, 0, 0, 8, p, p, None, p, p, None]           # d, ld, n, nrows, row0, c0, ncols, core, comp, rinv, ..

    def block(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.grl_hdbscan_minedge_block(*a)
    for i in (0, 7, 8, 10, 11):
        assert block(**{'a%d' % i: None}) == _lib.GRL_EINVAL and b'null' in lib.grl_last_error(), i
    for kw in (dict(a2=-1), dict(a3=-1), dict(a4=-1), dict(a5=-1)):
        assert block(**kw) == _lib.GRL_EINVAL and b'>= 0' in lib.grl_last_error(), kw
    for kw in (dict(a6=0), dict(a6=-3), dict(a1=7)):
        assert block(**kw) == _lib.GRL_EINVAL and b'ld >= ncols' in lib.grl_last_error(), kw
    for kw in (dict(a3=9), dict(a4=5), dict(a5=1), dict(a2=7), dict(a4=2 ** 31 - 2), dict(a5=2 ** 31 - 2)):
        assert block(**kw) == _lib.GRL_EINVAL and b'beyond n' in lib.grl_last_error(), kw
    assert block(a3=0) == 0                                      # no rows: nothing to launch
    ok2 = [p, 8, 8, 4, 0, 0, 8, p, None]

    def cosine(**kw):
        a = list(ok2)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.grl_hdbscan_cosine_block(*a)
    for i in (0, 7):
        assert cosine(**{'a%d' % i: None}) == _lib.GRL_EINVAL and b'null' in lib.grl_last_error(), i
    for kw in (dict(a2=-1), dict(a6=0), dict(a1=7), dict(a3=9), dict(a5=1)):
        assert cosine(**kw) == _lib.GRL_EINVAL, kw
    assert cosine(a3=0) == 0
