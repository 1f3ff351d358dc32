"""Tracklet set distances without a GPU: the float32 model of the kernel's contract (tests/setdist_ref.py)
against the float64 definition, the identities that tie the feature to dense mode's mean rows, the GRL_EVAL_SET knob and
the argument checks that come before any device work."""
import os

import numpy as np
import pytest
import torch

import setdist_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# counts on both sides of every path of the mapping: one clip, fewer than a wave's 64 columns (W = 1, 2, 4, 16, 32 with
# 64, 32, 16, 4, 2 rows per load), exactly 32 / 33 / 64 / 65 columns, more rows than one unrolled step, several pieces
Q_COUNTS = [1, 2, 15, 33, 65, 70]
G_COUNTS = [1, 3, 64, 65, 17, 32, 33, 2, 130]


def _sets(q_counts, g_counts, d=24, seed=0, noise=0.35):
    """clip rows = tracklet centre + noise, unit norm; (qc, gc, qptr, gptr) float32 / int64"""
    rng = np.random.Generator(np.random.PCG64(seed))

    def make(counts):
        rows = []
        for c in counts:
            centre = rng.standard_normal(d)
            x = centre[None, :] + noise * np.sqrt(d) * rng.standard_normal((c, d))
            rows.append(x / np.linalg.norm(x, axis=1, keepdims=True))
        return np.concatenate(rows).astype(np.float32), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    qc, qptr = make(q_counts)
    gc, gptr = make(g_counts)
    return qc, gc, qptr, gptr


@pytest.fixture(scope='module')
def sets():
    return _sets(Q_COUNTS, G_COUNTS)


@pytest.fixture(scope='module')
def matrices(sets):
    qc, gc, _, _ = sets
    return {m: R.clip_matrix64(qc, gc, m).astype(np.float32) for m in ('cosine', 'euclidean')}


@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_float32_model_agrees_with_the_float64_definition(sets, matrices, metric):
    qc, gc, qptr, gptr = sets
    E = matrices[metric]
    for reduce in ('chamfer', 'mean'):
        # fp32 rounding of O(1) values summed over <= 1024 terms, and the fp32 clip matrix against the fp64 one
        got = R.set_dist_from_matrix(E, qptr, gptr, reduce)
        assert np.abs(got.astype(np.float64) - R.brute(qc, gc, qptr, gptr, reduce, metric)).max() <= 1e-4, reduce
    for reduce in ('min', 'hausdorff'):                        # selections: exact on the same float32 matrix
        got = R.set_dist_from_matrix(E, qptr, gptr, reduce)
        assert np.array_equal(got.astype(np.float64), R.brute(qc, gc, qptr, gptr, reduce, metric, E=E)), reduce


def test_float64_mean_with_cosine_is_the_distance_of_the_mean_rows(sets):
    qc, gc, qptr, gptr = sets
    q64, g64 = qc.astype(np.float64), gc.astype(np.float64)
    qm = np.stack([q64[qptr[a]:qptr[a + 1]].mean(0) for a in range(len(qptr) - 1)])
    gm = np.stack([g64[gptr[b]:gptr[b + 1]].mean(0) for b in range(len(gptr) - 1)])
    assert np.abs(R.brute(qc, gc, qptr, gptr, 'mean', 'cosine') - (-(qm @ gm.T))).max() <= 1e-12


@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_hausdorff_is_at_least_chamfer_is_at_least_min_on_every_cell(sets, matrices, metric):
    qc, gc, qptr, gptr = sets
    b = {r: R.brute(qc, gc, qptr, gptr, r, metric) for r in ('min', 'chamfer', 'hausdorff')}
    assert (b['hausdorff'] >= b['chamfer']).all() and (b['chamfer'] >= b['min']).all()
    f = {r: R.set_dist_from_matrix(matrices[metric], qptr, gptr, r) for r in ('min', 'chamfer', 'hausdorff')}
    # float32: the chamfer value is a rounded mean of values between min and hausdorff -- a few ulp of slack at most
    assert (f['hausdorff'] >= f['min']).all()
    assert (f['chamfer'] >= f['min'] - 1e-6).all() and (f['hausdorff'] >= f['chamfer'] - 1e-6).all()


def test_model_orders_zeros_propagates_nan_and_keeps_its_summation_order():
    nz, pz = np.float32(-0.0), np.float32(0.0)
    e = np.array([[pz, nz], [pz, pz]], np.float32)
    assert np.signbit(R.cell(e, 'min')) and not np.signbit(R.cell(e, 'hausdorff'))      # -0 below +0
    assert np.signbit(R.cell(np.array([[nz]], np.float32), 'hausdorff'))
    for reduce in R.REDUCES:
        for shape in ((1, 1), (3, 70), (70, 3)):
            e = np.ones(shape, np.float32)
            e[-1, -1] = np.nan
            assert R.cell(e, reduce).view(np.uint32) == 0x7fc00000, (reduce, shape)
            e[-1, -1] = -np.nan
            assert R.cell(e, reduce).view(np.uint32) == 0x7fc00000, (reduce, shape)
    assert R.cell(np.array([[np.inf, -np.inf]], np.float32), 'mean').view(np.uint32) == 0x7fc00000   # a sum that is NaN
    # mean: lane = (i % R) * W + j % 64.  3 x 3 -> W = 4, R = 16: every element its own lane, then the tree
    big, one = np.float32(2.0 ** 24), np.float32(1.0)
    e = np.array([[big, one, one], [one, one, one], [one, one, -big]], np.float32)
    part = np.zeros(64, np.float32)
    for i in range(3):
        for j in range(3):
            part[i * 4 + j] = e[i, j]
    s = 32
    while s:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    assert R.cell(e, 'mean') == np.float32(part[0] / np.float32(9)) and part[0] == 5      # (7 in exact arithmetic)
    # 2 x 130 -> W = 64, one row per load: lane l sums rows 0, 1 of column l, then of column l + 64, then l + 128
    e = np.arange(260, dtype=np.float32).reshape(2, 130) * np.float32(1.1)
    part = np.zeros(64, np.float32)
    for cb in (0, 64, 128):
        for i in range(2):
            for l in range(min(64, 130 - cb)):
                part[l] = part[l] + e[i, cb + l]
    s = 32
    while s:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    assert R.cell(e, 'mean') == np.float32(part[0] / np.float32(260))
    # chamfer: sequential sums in ascending index
    e = np.array([[big, big], [one, big], [one, big], [-big, -big]], np.float32)        # rowmin = big, 1, 1, -big
    rows = np.float32(np.float32(np.float32(big + one) + one) - big)                    # = 0: the ones are absorbed
    cols = np.float32(-big + -big)
    want = np.float32(0.5) * (np.float32(rows / np.float32(4)) + np.float32(cols / np.float32(2)))
    assert rows == 0 and R.cell(e, 'chamfer') == want


def test_the_evaluator_knob_parses():
    from grl_amd.reid.evaluator.attevaluator import parse_set_knob as parse
    name = 'GRL_EVAL_SET'
    assert parse(name, None) is None and parse(name, '') is None and parse(name, '  ') is None
    for reduce in ('min', 'mean', 'chamfer', 'hausdorff'):
        assert parse(name, reduce) == (reduce, 'cosine')
        assert parse(name, reduce + ',cosine') == (reduce, 'cosine')
        assert parse(name, ' %s , euclidean ' % reduce) == (reduce, 'euclidean')
    for bad in ('1', 'x', 'Chamfer', 'chamfer,', ',cosine', 'chamfer,l2', 'chamfer,cosine,1', 'chamfer;cosine', 'max',
                'cosine', 'cosine,chamfer'):
        with pytest.raises(ValueError, match=name) as err:
            parse(name, bad)
        assert repr(bad) in str(err.value)


class _Never(object):
    def __getattr__(self, name):
        raise AssertionError('touched %s' % name)


KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_CLUSTER', 'GRL_EVAL_CLUSTER_JACCARD', 'GRL_EVAL_KMEANS', 'GRL_EVAL_HDBSCAN', 'GRL_EVAL_TSNE',
         'GRL_EVAL_SILHOUETTE', 'GRL_EVAL_PCA', 'GRL_EVAL_DIFFUSION', 'GRL_EVAL_SET')


def test_the_knob_and_its_refused_combinations_raise_before_the_loaders_are_touched(monkeypatch):
    from grl_amd.reid.evaluator import ATTEvaluator
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)

    def run(only_eval=True, rerank=0):
        ATTEvaluator(_Never(), _Never(), only_eval).evaluate(None, None, _Never(), _Never(), '', 0, rerank)
    monkeypatch.setenv('GRL_EVAL_SET', 'chamfer,l2')
    with pytest.raises(ValueError, match="GRL_EVAL_SET.*'chamfer,l2'"):
        run()
    monkeypatch.setenv('GRL_EVAL_SET', 'chamfer')
    with pytest.raises(ValueError, match='GRL_EVAL_SET=chamfer needs the dense mode.*one clip per tracklet'):
        run(only_eval=False)
    with pytest.raises(ValueError, match='GRL_EVAL_SET=chamfer cannot re-rank'):
        run(rerank=1)
    monkeypatch.setenv('GRL_EVAL_RERANK', 'stream')
    with pytest.raises(ValueError, match='GRL_EVAL_SET=chamfer cannot re-rank'):
        run(rerank=1)
    monkeypatch.delenv('GRL_EVAL_RERANK')
    for name, value in (('GRL_EVAL_METRIC', 'verify'), ('GRL_EVAL_METRIC', 'verify,0.5'), ('GRL_EVAL_QE', '3'),
                        ('GRL_EVAL_DBA', '3,2'), ('GRL_EVAL_PCA', '64'), ('GRL_EVAL_DIFFUSION', '50')):
        monkeypatch.setenv(name, value)
        with pytest.raises(ValueError, match='GRL_EVAL_SET=chamfer cannot be combined with .*%s' % name):
            run()
        monkeypatch.delenv(name)
    # accepted: it gets as far as the models and loaders
    for name, value in ((None, None), ('GRL_EVAL_ROC', '1'), ('GRL_EVAL_STREAM', '1'), ('GRL_EVAL_CLUSTER', '-0.7')):
        if name:
            monkeypatch.setenv(name, value)
        with pytest.raises(AssertionError, match='touched'):
            run()
        if name:
            monkeypatch.delenv(name)
    with pytest.raises(ValueError, match='only_eval=True'):
        ATTEvaluator(_Never(), _Never(), False).extract_clip_features(_Never())


def test_tracklet_set_and_the_public_functions_validate_before_the_device(monkeypatch):
    from grl_amd import engine
    from grl_amd._lib import GrlHipError

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    monkeypatch.setattr(engine, '_call', no_device)
    monkeypatch.setattr(engine, 'gemm', no_device)
    host = torch.zeros(6, 32)
    for counts, what in (([3, 0, 3], 'at least one clip'), ([7, -1], 'at least one clip'), ([1025], 'at most 1024'),
                         ([3, 2], 'add up to 5'), ([3, 4], 'add up to 7'), ([], 'add up to 0'), ([2.5, 3.5], 'integers'),
                         ([[3, 3]], 'integers'), (['3', '3'], 'integers')):
        with pytest.raises(ValueError, match=what):
            engine.TrackletSet(torch.zeros(1025, 32) if counts == [1025] else host, counts)
    with pytest.raises(ValueError, match='2-d tensor'):
        engine.TrackletSet(torch.zeros(6), [6])
    with pytest.raises(ValueError, match='2-d tensor'):
        engine.TrackletSet(np.zeros((6, 32), np.float32), [6])
    with pytest.raises(GrlHipError, match='HIP device'):               # valid counts: the device is looked at last
        engine.TrackletSet(host, [1, 2, 3])
    assert engine.SET_MAX_CLIPS == 1024 and sorted(engine.SET_REDUCE) == ['chamfer', 'hausdorff', 'mean', 'min']
    ts = engine.TrackletSet.__new__(engine.TrackletSet)
    ids = ([0], [0], [0], [0])
    for fn, args in ((engine.set_dist, ()), (engine.set_search, (5,)), (engine.set_metrics_streaming, ids),
                     (engine.set_pair_roc, ids)):
        with pytest.raises(ValueError, match="reduce must be 'min', 'mean', 'chamfer' or 'hausdorff'"):
            fn(ts, ts, *args, reduce='max')
        with pytest.raises(ValueError, match="metric must be 'cosine' or 'euclidean'"):
            fn(ts, ts, *args, metric='l1')
        with pytest.raises(ValueError, match='TrackletSet'):
            fn(host, ts, *args)
    for k in (0, 1025, -1):
        with pytest.raises(ValueError, match='k must be in 1..1024'):
            engine.set_search(ts, ts, k)


def test_set_ranges_never_cut_a_tracklet_and_respect_the_cap():
    from grl_amd import engine
    ptr = np.concatenate([[0], np.cumsum([1, 2, 15, 63, 64, 65, 130, 1, 1])]).astype(np.int64)
    n = len(ptr) - 1
    for cap in (1, 2, 16, 64, 100, 200, 10 ** 6):
        for t0, t1 in ((0, n), (2, 6), (n - 1, n)):
            r = engine._set_ranges(ptr, t0, t1, cap)
            assert r[0][0] == t0 and r[-1][1] == t1 and all(a[1] == b[0] for a, b in zip(r, r[1:]))
            for a, b in r:
                assert b > a and (ptr[b] - ptr[a] <= cap or b == a + 1), (cap, a, b)
                if b < t1:                                          # greedy: the next tracklet did not fit
                    assert ptr[b + 1] - ptr[a] > cap
    assert engine._set_ranges(ptr, 3, 3, 5) == []


def test_library_exports_and_header_declare_the_entry_point():
    import ctypes
    from grl_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'grl_hip.h')).read()
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    name = 'grl_setdist_block'
    assert name in _lib.exported_symbols() and getattr(lib, name).restype is not None
    assert hasattr(raw, name) and name + '(' in header
    assert lib.grl_abi_version() == 10 and _lib.ABI_VERSION == 10             # additive only
    assert ' setdist.hip ' in open(os.path.join(ROOT, 'grl_amd', 'csrc', 'Makefile')).read()
    for word, value in (('GRL_SET_MIN', 0), ('GRL_SET_MEAN', 1), ('GRL_SET_CHAMFER', 2), ('GRL_SET_HAUSDORFF', 3),
                        ('GRL_SET_MAX_CLIPS', 1024)):
        assert '#define %s' % word in header and int(header.split('#define %s' % word)[1].split()[0]) == value
    # the argument checks come before any HIP call: fake device pointers (never dereferenced), real host ptr arrays
    E, U = _lib.GRL_EINVAL, _lib.GRL_EUNSUPPORTED

    def call(qcounts, gcounts, ld=None, a0=0, na=None, b0=0, nb=None, reduce=2, ldo=None, e=0x1000, out=0x4000,
             qdev=0x2000, gdev=0x3000, qhost=True, ghost=True):
        qp = np.concatenate([[0], np.cumsum(qcounts)]).astype(np.int64)
        gp = np.concatenate([[0], np.cumsum(gcounts)]).astype(np.int64)
        na = len(qcounts) - a0 if na is None else na
        nb = len(gcounts) - b0 if nb is None else nb
        ld = int(gp[min(b0 + max(nb, 0), len(gcounts))] - gp[b0]) if ld is None else ld
        return lib.grl_setdist_block(e, ld, qp.ctypes.data if qhost else None, qdev, a0, na,
                                     gp.ctypes.data if ghost else None, gdev, b0, nb, reduce, out,
                                     max(nb, 0) if ldo is None else ldo, None)
    q, g = [1, 2, 15], [3, 64, 65, 17]
    assert call(q, g, na=0) == 0 and call(q, g, nb=0) == 0                  # nothing to do, nothing launched
    for kw in (dict(e=None), dict(out=None), dict(qdev=None), dict(gdev=None), dict(qhost=False), dict(ghost=False)):
        assert call(q, g, **kw) == E, kw                                       # a null pointer
    for kw in (dict(na=-1), dict(nb=-1), dict(a0=-1), dict(b0=-1), dict(ld=-1)):
        assert call(q, g, **kw) == E, kw                                       # a negative size
    assert call([1, 0, 15], g) == E and call(q, [3, 0, 1]) == E               # an empty tracklet
    assert call([5, -2, 15], g) == E and call(q, [3, 7, -7, 1]) == E          # a ptr that is not ascending
    assert call(q, g, ld=148) == E                                            # ld below the 149 clip columns
    assert call(q, g, b0=1, ld=145) == E                                      # ... below the 146 of tracklets 1..3
    assert call(q, g, ldo=3) == E                                             # ldo < nb
    for reduce in (-1, 4, 99):
        assert call(q, g, reduce=reduce) == E                                 # an unknown reduce
    assert call([1, 1025], g) == U and call(q, [1025, 2]) == U                # more than 1024 clips
    assert b'1025 clips' in lib.grl_last_error()
    assert call([1, 0, 1025], g) == E                                         # GRL_EINVAL comes first
