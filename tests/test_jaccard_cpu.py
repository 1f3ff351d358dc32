"""The Jaccard eps-graph contract on the host: the streaming model of tests/jaccard_ref.py against its
own dense transcription, against the reference's re-ranking output, and, through cluster_ref, against scikit-learn's
DBSCAN; the GRL_EVAL_CLUSTER_JACCARD parser, the argument checks of engine.jaccard_graph / cluster_jaccard and of
grl_jaccard_edges.  No GPU is needed."""
import os

import numpy as np
import pytest
import torch

import cluster_ref as CR
import jaccard_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_features = J.features


def _same(a, b, what):
    for u, v, name in zip(a, b, ('row_ptr', 'col', 'val')):
        assert u.dtype == v.dtype and u.shape == v.shape, (what, name)
        assert np.array_equal(u.view(np.int32) if u.dtype == np.float32 else u,
                              v.view(np.int32) if v.dtype == np.float32 else v), (what, name)


@pytest.mark.parametrize('k1,k2', [(1, 1), (4, 2), (20, 6), (20, 8)])
@pytest.mark.parametrize('d', [5, 16])
@pytest.mark.parametrize('n', [2, 3, 33, 70, 257])
def test_streaming_model_equals_its_dense_transcription(n, d, k1, k2):
    if not (k1 < n and k2 <= n):
        with pytest.raises(ValueError):
            J.graph(J.euclid(_features(n, d, 1)), 0.5, k1, k2)
        return
    S = J.euclid(_features(n, d, n + d))
    Jm = J.dense_matrices(S, k1, k2)[3]                          # once per case; dense_graph thresholds it
    v2 = {w: J.sparse_rows(S, k1, k2, w)[4] for w in (7, n)}
    _same(J.graph(S, 0.5, k1, k2, width=64, window=64), J.dense_graph(S, 0.5, k1, k2), (n, d, k1, k2, 'whole'))
    edges = 0
    for eps, width, window in ((0.5, 7, 16), (0.8, n, 64), (0.999, n, 256), (0.0, 7, 5), (-0.25, n, 300)):
        want = J.threshold(Jm, eps)
        A = J.adjacency(want[0], want[1], n)
        got = J.graph_from_v2(v2[width], n, eps, window)
        _same(got, want, (n, d, k1, k2, eps))
        assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float32
        assert not A.diagonal().any() and np.array_equal(A, A.T)         # t is symmetric bit for bit
        if eps < 0:
            assert got[1].size == 0
        edges += got[1].size
    assert edges > 0


def test_ties_zero_row_and_the_shape_of_v2():
    """The special rows do what they are there for: exact ties in D, a row of the all-zero sample, V2 rows that sum to
    one and stay within the 2048 entries grl_rrs_expand can make."""
    x = _features(70, 16, 3)
    S = J.euclid(x)
    D, V, V2, Jm = J.dense_matrices(S, 20, 6)
    assert D[0, 35] == D[0, 3] == D[0, 0] and (D >= 0).all() and np.isfinite(Jm).all()
    assert np.allclose(V.sum(1), 1, atol=1e-5) and np.allclose(V2.sum(1), 1, atol=1e-5)
    assert ((V2 != 0).sum(1) <= 2048).all() and (Jm.diagonal() < 1e-6).all()
    assert (Jm >= -1e-6).all() and (Jm <= 1).all() and (Jm == 1).any()
    with pytest.raises(ValueError):
        J.graph(S, 1.0)
    with pytest.raises(ValueError):
        J.graph(S, np.inf)
    with pytest.raises(ValueError):
        J.graph(S, np.nan)


def test_expand_equals_rerank_stream_refs_and_takes_empty_lists():
    import rerank_stream_ref as R
    S = J.euclid(_features(70, 16, 3))
    for k1, k2 in ((20, 6), (4, 1), (7, 8)):
        _, rank, lists, vals, v2 = J.sparse_rows(S, k1, k2)
        for (c, v), (c2, v2_) in zip(R.expand(rank, lists, vals, k2), v2):
            assert np.array_equal(c, c2) and np.array_equal(v.view(np.int32), v2_.view(np.int32))
    # 40 exact copies: most of them are not among their own first 21 neighbours and have no k-reciprocal neighbour
    S = J.euclid(J.blob(5, 40, 20, 30, 8))
    _, rank, lists, vals, v2 = J.sparse_rows(S, 20, 6, 16)
    assert sum(l.size == 0 for l in lists) >= 15
    for eps in (0.3, 0.999):
        _same(J.graph(S, eps, 20, 6, width=16, window=32), J.dense_graph(S, eps, 20, 6), eps)
    assert J.graph(S, 0.3, 20, 6)[1].size > 0


def test_dense_model_on_the_stacked_golden_matrices_gives_the_reference_re_ranking():
    """The link to the reference: on S = [[qq, qg], [qg^T, gg]] of the stored re-ranking case, D and J of the dense
    model blend to the stored ``re_ranking`` output, within the bound that pins rerank_stream_ref to it (2e-6)."""
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'rerank_q16_g120.npz'))
    qg, qq, gg = (np.asarray(g[k], np.float32) for k in ('dist', 'qq', 'gg'))
    nq = qg.shape[0]
    S = np.concatenate((np.concatenate((qq, qg), 1), np.concatenate((qg.T, gg), 1)), 0)
    D, _, _, Jm = J.dense_matrices(S, 20, 6)
    lam = np.float32(0.3)
    F = Jm[:nq, nq:] * np.float32(1 - 0.3) + D[:nq, nq:] * lam
    assert F.shape == g['final'].shape and np.abs(F - g['final']).max() < 2e-6


def test_dbscan_on_the_models_graph_equals_sklearn_on_the_dense_jaccard_matrix():
    from sklearn.cluster import DBSCAN
    cases = noise = multi = 0
    for seed in range(40):
        n = 24 + seed % 30
        S = J.euclid(_features(n, 8, 100 + seed, special=seed % 4 == 0))
        k1, k2 = (6, 2) if seed % 2 else (4, 1)
        Jm = J.dense_matrices(S, k1, k2)[3]
        for eps in (0.4, 0.7):
            row_ptr, col, val = J.graph(S, eps, k1, k2, width=16, window=32)
            assert np.array_equal(J.adjacency(row_ptr, col, n), CR.edges(Jm, eps))
            X = np.where(Jm <= np.float32(eps), 0.0, 1.0)
            np.fill_diagonal(X, 0.0)
            for m in (1, 2, 4):
                labels, core = CR.dbscan(n, m, row_ptr=row_ptr, col=col)
                sk = DBSCAN(eps=0.5, min_samples=m, metric='precomputed').fit(X)
                assert np.array_equal(labels, sk.labels_), (seed, eps, m)
                assert np.array_equal(np.flatnonzero(core), sk.core_sample_indices_), (seed, eps, m)
                cases += 1
                noise += int((labels < 0).sum())
                multi += labels.max() >= 1
    assert cases >= 100 and noise > 50 and multi > 50


def test_parse_cluster_jaccard_knob():
    from grl_amd.reid.evaluator.attevaluator import parse_cluster_jaccard_knob as parse
    name = 'GRL_EVAL_CLUSTER_JACCARD'
    for off in (None, '', '   '):
        assert parse(name, off) is None
    assert parse(name, '0.5') == (0.5, 1, 20, 6)
    assert parse(name, ' 0.6 , 4 ') == (0.6, 4, 20, 6)
    assert parse(name, '0.5,2,10') == (0.5, 2, 10, 6)
    assert parse(name, '0.5,2,20,8') == (0.5, 2, 20, 8) and parse(name, '0,1,1,1') == (0.0, 1, 1, 1)
    assert parse(name, '-0.1') == (-0.1, 1, 20, 6) and parse(name, '9.99e-1,3') == (0.999, 3, 20, 6)
    for bad in ('x', 'eer', '0.5,', ',2', '0.5,0', '0.5,-1', '0.5,1.5', '0.5,two', 'nan', 'inf', '-inf', '1', '1.0', '2.5',
                '0.99999999', '0.5,1,0', '0.5,1,21', '0.5,1,20,0', '0.5,1,20,9', '0.5,1,20,6,1', '0.5;2', '0.5,1,,6'):
        with pytest.raises(ValueError, match=name):
            parse(name, bad)


class _Never(object):
    def __getattr__(self, name):
        raise AssertionError('touched %s' % name)


KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_CLUSTER', 'GRL_EVAL_KMEANS', 'GRL_EVAL_CLUSTER_JACCARD')


def test_bad_knob_and_the_verify_metric_are_refused_before_any_feature_is_extracted(monkeypatch):
    from grl_amd.reid.evaluator import ATTEvaluator
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for bad in ('1.0', '0.5,0', '0.5,1,21'):
        monkeypatch.setenv('GRL_EVAL_CLUSTER_JACCARD', bad)
        with pytest.raises(ValueError, match='GRL_EVAL_CLUSTER_JACCARD'):
            ATTEvaluator(_Never(), _Never(), False).evaluate(None, None, _Never(), _Never(), '', 0, 0)
    monkeypatch.setenv('GRL_EVAL_CLUSTER_JACCARD', '0.5,2')
    for metric in ('verify', 'verify,0.5'):
        monkeypatch.setenv('GRL_EVAL_METRIC', metric)
        with pytest.raises(ValueError, match='GRL_EVAL_CLUSTER_JACCARD.*signed logit'):
            ATTEvaluator(_Never(), _Never(), False).evaluate(None, None, _Never(), _Never(), '', 0, 0)


def test_engine_refuses_bad_arguments_before_touching_the_device():
    import inspect
    from grl_amd import engine
    x = torch.zeros((30, 8))                                     # a host tensor: the device path would raise GrlHipError
    for fn in (engine.jaccard_graph, engine.cluster_jaccard):
        with pytest.raises(ValueError, match='HIP device'):
            fn(x, 0.5)
        with pytest.raises(ValueError, match='xf'):
            fn(x.numpy(), 0.5)
        assert 'verify_metric' not in inspect.signature(fn).parameters and 'metric' not in inspect.signature(fn).parameters
        with pytest.raises(TypeError):
            fn(x, 0.5, verify_metric=None)
    with pytest.raises(ValueError, match='min_samples'):
        engine.cluster_jaccard(x, 0.5, min_samples=0)
    with pytest.raises(ValueError, match='min_samples'):
        engine.cluster_jaccard(x, 0.5, min_samples=1.5)
    # everything after the placement check is reached with a stand-in that claims to be on the device
    real = engine._jaccard_args

    class OnDevice(object):
        def __init__(self, shape):
            self.shape, self.dtype, self.is_cuda, self.device = shape, torch.float32, True, 'stand-in'

        def dim(self):
            return len(self.shape)

    def args(shape, eps=0.5, k1=20, k2=6):
        is_tensor = torch.is_tensor
        torch.is_tensor = lambda t: isinstance(t, OnDevice) or is_tensor(t)
        try:
            return real(OnDevice(shape), eps, k1, k2, 'jaccard_graph')
        finally:
            torch.is_tensor = is_tensor
    assert args((30, 8)) == (30, 0.5, 20, 6) and args((2, 1), 0.0, 1, 2) == (2, 0.0, 1, 2)
    assert args((30, 8), -3)[1] == -3.0 and args((30, 8), np.float32(0.3))[1] == float(np.float32(0.3))
    for shape in ((30,), (30, 8, 2), (1, 8), (0, 8), (30, 0)):
        with pytest.raises(ValueError, match='xf|n >= 2'):
            args(shape)
    for eps in (1.0, 1.5, 0.99999999, float('inf'), float('-inf'), float('nan'), None, '0.5', True):
        with pytest.raises(ValueError, match='eps'):
            args((30, 8), eps)
    for k1 in (0, 21, -1, 2.0, True, None):
        with pytest.raises(ValueError, match='k1'):
            args((30, 8), k1=k1)
    with pytest.raises(ValueError, match='k1'):
        args((20, 8), k1=20)                                     # k1 < n
    for k2 in (0, 9, 1.0, None):
        with pytest.raises(ValueError, match='k2'):
            args((30, 8), k2=k2)
    with pytest.raises(ValueError, match='k2'):
        args((3, 8), k1=1, k2=4)                                 # k2 <= n


def test_grl_jaccard_edges_is_bound_and_checks_its_arguments_before_any_launch():
    import ctypes as C
    from grl_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 10 and lib.grl_abi_version() == 10
    assert 'grl_jaccard_edges' in _lib.exported_symbols()
    header = open(os.path.join(ROOT, 'include', 'grl_hip.h')).read()
    assert 'int grl_jaccard_edges(' in header and '#define GRL_ABI_VERSION 10' in header
    assert 'jaccard.hip' in open(os.path.join(ROOT, 'grl_amd', 'csrc', 'Makefile')).read()
    p = 16                                                       # any non-null address: nothing is dereferenced
    count = [p, p, p, p, p, p, 8, C.c_float(0.5), 0, p, None, None, None, None]
    fill = [p, p, p, p, p, p, 8, C.c_float(0.5), 256, None, p, p, None, None]

    def call(base, **kw):
        a = list(base)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.grl_jaccard_edges(*a)
    for i in range(6):
        for base in (count, fill):
            assert call(base, **{'a%d' % i: None}) == _lib.GRL_EINVAL and b'null' in lib.grl_last_error()
    assert call(count, a9=None) == _lib.GRL_EINVAL and b'count pass' in lib.grl_last_error()
    assert call(count, a11=p) == _lib.GRL_EINVAL and call(count, a12=p) == _lib.GRL_EINVAL
    assert call(fill, a11=None) == _lib.GRL_EINVAL and b'fill pass' in lib.grl_last_error()
    for n in (1, 0, -5):
        assert call(count, a6=n) == _lib.GRL_EINVAL and b'n >= 2' in lib.grl_last_error()
    for window in (1, 100, 255, 257, 384 + 1, -256, 8192 + 256, 1 << 20):
        assert call(count, a8=window) == _lib.GRL_EINVAL and b'window' in lib.grl_last_error(), window
        assert call(fill, a8=window) == _lib.GRL_EINVAL
    for eps in (1.0, 2.0, float('inf'), float('-inf'), float('nan')):
        assert call(count, a7=C.c_float(eps)) == _lib.GRL_EINVAL and b'eps' in lib.grl_last_error()
