"""Product-quantised gallery index without a GPU: the float32 model of the ADC contract
(tests/pq_ref.py) against float64, the encode / decode round trip, topk_recall, the GRL_EVAL_PQ knob, the binding, the
host-side argument checks of pq.hip, and the planted quality case that tests/test_gpu_pq.py repeats on the device."""
import os

import numpy as np
import pytest
import torch

import pq_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
MS = (1, 2, 3, 4, 5, 8, 13, 96)
PQ_NAMES = ('grl_pq_scan', 'grl_pq_lut_finish', 'grl_pq_pack', 'grl_pq_decode')


def _tables(M, ksub=16, nq=5, n=37, seed=0):
    g = np.random.Generator(np.random.PCG64(seed + M))
    lut = (g.standard_normal((nq, M, ksub)) * np.exp(g.uniform(-3, 3, (nq, M, 1)))).astype(np.float32)
    codes = g.integers(0, ksub, (n, M)).astype(np.uint8)
    return lut, codes


def _picked(lut, codes):
    """[nq, n, M]: the entries every pair selects"""
    return np.stack([lut[:, m, :][:, codes[:, m].astype(np.int64)] for m in range(lut.shape[1])], axis=2)


@pytest.mark.parametrize('M', MS)
def test_adc_sum_agrees_with_the_float64_sum_of_the_same_entries(M):
    lut, codes = _tables(M)
    e = _picked(lut, codes).astype(np.float64)
    got = R.adc_sum(lut, codes)
    assert got.dtype == np.float32 and got.shape == (lut.shape[0], codes.shape[0])
    # the longest add chain: M / 4 sequential adds of a partial, then two adds of the join; each rounds by at most 2^-24
    # of a partial sum, which the sum of the absolute entries bounds
    bound = (M / 4 + 2) * U * np.abs(e).sum(2)
    assert (np.abs(got.astype(np.float64) - e.sum(2)) <= bound).all()


def test_adc_sum_follows_the_four_partial_order():
    big, one = np.float32(2.0 ** 24), np.float32(1.0)
    # M = 9, one centroid per subspace: p0 = (big + 1) + 1 = big (m = 0, 4, 8: the ones are absorbed), p1 = p2 = 1, p3 = -big
    vals = [big, one, one, -big, one, 0, 0, 0, one]
    lut = np.zeros((1, 9, 16), np.float32)
    lut[0, :, 3] = vals
    codes = np.full((1, 9), 3, np.uint8)
    p0 = np.float32(np.float32(big + one) + one)
    want = np.float32(np.float32(p0 + one) + np.float32(one + -big))
    assert p0 == big and R.adc_sum(lut, codes)[0, 0] == want == 1                          # 4 in exact arithmetic
    assert np.float32(np.float32(np.float32(big + one) + one) + one) + -big == 0           # (one sequential chain: 0)
    # M <= w: the empty partials are +0, so an all-(+0) table gives +0 and an all-(-0) table of M < 4 gives +0 too
    for M in MS:
        z = R.adc_sum(np.zeros((2, M, 16), np.float32), np.zeros((3, M), np.uint8))
        assert (z == 0).all() and not np.signbit(z).any()
    z = R.adc_sum(np.full((1, 2, 16), -0.0, np.float32), np.zeros((1, 2), np.uint8))
    assert z[0, 0] == 0 and not np.signbit(z[0, 0])


def test_nan_and_infinities_follow_ieee_through_the_adds():
    for M in (1, 5, 8):
        lut, codes = _tables(M, nq=2, n=4)
        lut[0, M - 1, codes[1, M - 1]] = np.nan
        got = R.adc_sum(lut, codes)
        assert np.isnan(got[0, 1]) and not np.isnan(got[1]).any()
        assert not np.isnan(got[0, codes[:, M - 1] != codes[1, M - 1]]).any()
    lut, codes = _tables(8, nq=1, n=3)
    codes[0] = 2
    lut[0, 1, 2], lut[0, 6, 2] = np.inf, -np.inf                  # inf - inf across two partials
    assert np.isnan(R.adc_sum(lut, codes)[0, 0])
    lut[0, 6, 2] = np.inf
    assert R.adc_sum(lut, codes)[0, 0] == np.inf
    # euclidean: a NaN argument of the clamp gives 1e-12 (pairwise_distance_tensor's rule), -inf too
    rn = np.ones(1, np.float32)
    lut[0, 6, 2] = -np.inf
    assert R.adc_dist(lut, codes, 'euclidean', rn)[0, 0] == np.sqrt(np.float32(1e-12))
    lut[0, 1, 2] = -np.inf
    assert R.adc_dist(lut, codes, 'euclidean', rn)[0, 0] == np.sqrt(np.float32(1e-12))
    lut[0, 1, 2] = lut[0, 6, 2] = np.inf
    assert R.adc_dist(lut, codes, 'euclidean', rn)[0, 0] == np.inf


@pytest.mark.parametrize('M', MS)
def test_cosine_adc_is_the_negated_dot_product_with_the_decoded_row(M):
    g = np.random.Generator(np.random.PCG64(100 + M))
    dsub, ksub, nq, n = 32, 16, 4, 29
    C = g.standard_normal((M, ksub, dsub)).astype(np.float32)
    q = g.standard_normal((nq, M * dsub)).astype(np.float32)
    codes = g.integers(0, ksub, (n, M)).astype(np.uint8)
    # the table entries: exact float64 sub-dots rounded once
    lut64 = np.stack([-(q[:, R.sub(m, dsub)].astype(np.float64) @ C[m].astype(np.float64).T) for m in range(M)], axis=1)
    lut = lut64.astype(np.float32)
    want = -(q.astype(np.float64) @ R.decode(codes, C).astype(np.float64).T)
    # one rounding per entry (2^-24 |entry|) and the add chains of the test above
    bound = (M / 4 + 3) * U * np.abs(_picked(lut64, codes)).sum(2) + 1e-300
    assert (np.abs(R.adc_sum(lut, codes).astype(np.float64) - want) <= bound).all()


def test_euclidean_adc_is_the_distance_to_the_decoded_row():
    g = np.random.Generator(np.random.PCG64(7))
    M, dsub, ksub = 5, 32, 16
    C = g.standard_normal((M, ksub, dsub)).astype(np.float32)
    q = g.standard_normal((6, M * dsub)).astype(np.float32)
    codes = g.integers(0, ksub, (40, M)).astype(np.uint8)
    rn = (q.astype(np.float64) ** 2).sum(1).astype(np.float32)
    got = R.adc_dist(R.lut_host(q, C, 'euclidean'), codes, 'euclidean', rn)
    want = np.linalg.norm(q.astype(np.float64)[:, None] - R.decode(codes, C).astype(np.float64)[None], axis=2)
    assert np.abs(got - want).max() <= 1e-4                       # |q|^2 ~ 160: fp32 cancellation, then the sqrt


def test_encode_and_decode_round_trip():
    g = np.random.Generator(np.random.PCG64(3))
    M, ksub, dsub = 5, 16, 32
    C = g.standard_normal((M, ksub, dsub)).astype(np.float32)            # distinct rows
    codes = g.integers(0, ksub, (50, M)).astype(np.uint8)
    x = R.decode(codes, C)
    assert x.shape == (50, M * dsub) and x.dtype == np.float32
    for m in range(M):
        assert np.array_equal(x[:, R.sub(m, dsub)], C[m][codes[:, m]])
    assert np.array_equal(R.encode(x, C, R.euclid), codes)
    with pytest.raises(ValueError):
        R.decode(np.full((1, M), ksub, np.uint8), C)
    # ties go to the smaller centroid index: two equal codebook rows, and a NaN row under the clamp
    C[2, 9] = C[2, 4]
    x = R.decode(codes, C)
    back = R.encode(x, C, R.euclid)
    assert (codes[:, 2] == 9).any() and (back[codes[:, 2] == 9, 2] == 4).all()
    assert np.array_equal(back[codes[:, 2] != 9], codes[codes[:, 2] != 9])
    x[7, 33] = np.nan
    nan_row = R.encode(x, C, R.euclid)[7]
    assert nan_row[1] == 0 and np.array_equal(nan_row[[0, 2, 3, 4]], back[7, [0, 2, 3, 4]])
    x[7] = np.nan
    assert (R.encode(x, C, R.euclid)[7] == 0).all()


def test_search_model_orders_ties_by_the_gallery_index_and_pads():
    D = np.array([[0.5, -1.0, 0.5, -1.0, np.nan, -0.0, 0.0]], np.float32)
    dist, idx = R.search(D, 9)
    assert idx.tolist() == [[1, 3, 5, 6, 0, 2, 4, -1, -1]]
    assert dist[0, :4].tolist() == [-1.0, -1.0, 0.0, 0.0] and np.isnan(dist[0, 6]) and np.isinf(dist[0, 7:]).all()
    junk = np.zeros((1, 7), bool)
    junk[0, [1, 5]] = True
    assert R.search(D, 3, junk)[1].tolist() == [[3, 6, 0]]


def test_topk_recall_on_hand_made_lists():
    from grl_amd import engine
    approx = np.array([[0, 1, 2, 3], [5, 4, 9, 8], [7, -1, -1, -1], [1, 2, 3, 4]])
    exact = np.array([[0, 2, 1, 9], [4, 5, 6, 7], [7, 8, -1, -1], [-1, -1, -1, -1]])
    # k = 1: 1, 0, 1 (the all-padding query is left out); k = 2: 1/2, 2/2, 1/2; k = 4: 3/4, 2/4, 1/2
    want = [2 / 3.0, 2 / 3.0, (0.75 + 0.5 + 0.5) / 3.0]
    for fn in (engine.topk_recall, R.recall):
        got = fn(approx, exact, (1, 2, 4))
        assert np.allclose(got, want, rtol=0, atol=1e-15), got
        assert fn(approx, approx[:, ::-1].copy(), (4,)) == [1.0]              # a set comparison: order inside k is free
        assert np.isnan(fn(approx[3:], exact[3:], (1,))[0])
    assert engine.topk_recall(torch.from_numpy(approx), torch.from_numpy(exact), [2]) == [want[1]]
    with pytest.raises(ValueError, match='topk_recall'):
        engine.topk_recall(approx, exact[:2], (1,))
    with pytest.raises(ValueError, match='k must be'):
        engine.topk_recall(approx, exact, (0,))


def test_the_evaluator_knob_parses():
    from grl_amd.reid.evaluator.attevaluator import parse_pq_knob as parse
    name = 'GRL_EVAL_PQ'
    assert parse(name, None) is None and parse(name, '') is None and parse(name, '  ') is None
    assert parse(name, '96') == (96, 8, 25, 0)
    assert parse(name, ' 8 , 4 ') == (8, 4, 25, 0)
    assert parse(name, '8,4,3') == (8, 4, 3, 0)
    assert parse(name, '8,4,3,7') == (8, 4, 3, 7)
    for bad in ('x', '8,', ',4', '8,4,3,7,1', '8.5', '8;4', '0', '-1', '4097', '8,3', '8,9', '8,4,0', '8,4,1,-1'):
        with pytest.raises(ValueError, match=name) as err:
            parse(name, bad)
        assert repr(bad) in str(err.value)


class _Never(object):
    def __getattr__(self, name):
        raise AssertionError('touched %s' % name)


KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_CLUSTER', 'GRL_EVAL_CLUSTER_JACCARD', 'GRL_EVAL_KMEANS', 'GRL_EVAL_HDBSCAN', 'GRL_EVAL_TSNE',
         'GRL_EVAL_SILHOUETTE', 'GRL_EVAL_PCA', 'GRL_EVAL_DIFFUSION', 'GRL_EVAL_SET', 'GRL_EVAL_PQ')


def test_the_knob_and_its_refused_combinations_raise_before_the_loaders_are_touched(monkeypatch):
    from grl_amd.reid.evaluator import ATTEvaluator
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)

    def run(only_eval=True, rerank=0):
        ATTEvaluator(_Never(), _Never(), only_eval).evaluate(None, None, _Never(), _Never(), '', 0, rerank)
    monkeypatch.setenv('GRL_EVAL_PQ', '8,3')
    with pytest.raises(ValueError, match="GRL_EVAL_PQ.*'8,3'"):
        run()
    monkeypatch.setenv('GRL_EVAL_PQ', '8,4')
    with pytest.raises(ValueError, match='GRL_EVAL_PQ=8,4 cannot re-rank'):
        run(rerank=1)
    for name, value in (('GRL_EVAL_METRIC', 'verify'), ('GRL_EVAL_SET', 'chamfer'), ('GRL_EVAL_DIFFUSION', '50')):
        monkeypatch.setenv(name, value)
        with pytest.raises(ValueError, match='GRL_EVAL_PQ=8,4 cannot be combined with %s' % name):
            run()
        monkeypatch.delenv(name)
    # accepted: it gets as far as the models and loaders
    for name, value in ((None, None), ('GRL_EVAL_STREAM', '1'), ('GRL_EVAL_QE', '3'), ('GRL_EVAL_PCA', '64')):
        if name:
            monkeypatch.setenv(name, value)
        with pytest.raises(AssertionError, match='touched'):
            run(only_eval=False)
        if name:
            monkeypatch.delenv(name)


def test_the_public_functions_validate_before_the_device(monkeypatch):
    from grl_amd import engine
    from grl_amd._lib import GrlHipError

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    monkeypatch.setattr(engine, '_call', no_device)
    monkeypatch.setattr(engine, 'gemm', no_device)
    assert engine.PQ_M_MAX == 4096 and engine.PQ_METRICS == {'cosine': 0, 'euclidean': 1}
    assert engine.PQ_LUT_BYTES == int(os.environ.get('GRL_PQ_LUT_BYTES', str(1 << 30)))
    with pytest.raises(GrlHipError, match='HIP device'):
        engine.PqCodebook(torch.zeros(2, 16, 32))
    with pytest.raises(ValueError, match="metric must be 'cosine' or 'euclidean'"):
        engine.PqCodebook(torch.zeros(2, 16, 32), 'l1')
    host = torch.zeros(300, 256)
    with pytest.raises(GrlHipError, match='HIP device'):
        engine.pq_train(host, 8)
    with pytest.raises(ValueError, match="metric must be 'cosine' or 'euclidean'"):
        engine.pq_train(host, 8, metric='l1')
    index = engine.PqIndex.__new__(engine.PqIndex)
    for fn, args in ((engine.pq_dist, ()), (engine.pq_search, (5,)), (engine.pq_metrics_streaming, ([0], [0], [0], [0]))):
        with pytest.raises(ValueError, match='index must be a PqIndex'):
            fn(host, host, *args)
    for k in (0, 1025, -1):
        with pytest.raises(ValueError, match='k must be in 1..1024'):
            engine.pq_search(host, index, k)
    with pytest.raises(ValueError, match='codebook must be a PqCodebook'):
        engine.PqIndex(host, host)
    with pytest.raises(ValueError, match='codebook must be a PqCodebook'):
        engine.pq_index(host, host)
    for d, M, word in ((256, 3, 'M must divide'), (256, 16, 'dsub'), (80, 1, 'dsub'), (256, 0, 'M must be an integer'),
                       (256, 2.0, 'M must be an integer'), (256, True, 'M must be an integer')):
        with pytest.raises(ValueError, match=word):
            engine._pq_split(d, M, 'pq_train')


def test_library_exports_and_header_declare_the_entry_points():
    import ctypes
    from grl_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'grl_hip.h')).read()
    assert sorted(n for n in _lib._SIGNATURES if n.startswith('grl_pq_')) == sorted(PQ_NAMES)
    for name in PQ_NAMES:
        assert 'int %s(' % name in header, name
    assert ' pq.hip ' in open(os.path.join(ROOT, 'grl_amd', 'csrc', 'Makefile')).read().split('SRCS =')[1].split('\n')[0]
    assert _lib.ABI_VERSION == 10 and int(header.split('#define GRL_ABI_VERSION')[1].split()[0]) == 10     # additive only
    for word, value in (('GRL_PQ_COSINE', 0), ('GRL_PQ_EUCLIDEAN', 1), ('GRL_PQ_M_MAX', 4096)):
        assert '#define %s' % word in header and int(header.split('#define %s' % word)[1].split()[0]) == value
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert lib.grl_abi_version() == 10
    for name in PQ_NAMES:
        assert name in _lib.exported_symbols() and getattr(lib, name).restype is not None and hasattr(raw, name), name


def test_host_argument_checks_return_einval_through_the_c_abi():
    from grl_amd import _lib
    try:
        lib = _lib.load()
    except Exception as e:                                        # noqa: BLE001
        pytest.skip('libgrl_hip.so does not load here: %s' % e)
    E = _lib.GRL_EINVAL
    # fake device pointers (never dereferenced: every call below is refused, or has nothing to launch)

    def scan(lut=0x1000, codes=0x2000, out=0x3000, nq=3, n=100, M=8, ksub=256, ldo=None, metric=0, rn=None):
        return lib.grl_pq_scan(lut, codes, out, nq, n, M, ksub, n if ldo is None else ldo, metric, rn, None)
    assert scan(nq=0) == 0 and scan(n=0) == 0                                  # nothing to do, nothing launched
    for kw in (dict(lut=None), dict(codes=None), dict(out=None), dict(nq=-1), dict(n=-1), dict(M=0), dict(M=4097),
               dict(ksub=0), dict(ksub=8), dict(ksub=100), dict(ksub=512), dict(ldo=99), dict(metric=2), dict(metric=-1),
               dict(metric=1), dict(lut=0x1002), dict(codes=0x2001), dict(out=0x3002), dict(nq=262141)):
        assert scan(**kw) == E, kw
    assert b'pq_scan' in lib.grl_last_error()
    assert scan(metric=1, rn=0x4000, nq=0) == 0

    def finish(lut=0x1000, cn=0x2000, nq=3, M=8, ksub=16):
        return lib.grl_pq_lut_finish(lut, cn, nq, M, ksub, None)
    assert finish(nq=0) == 0
    for kw in (dict(lut=None), dict(cn=None), dict(nq=-1), dict(M=0), dict(ksub=17)):
        assert finish(**kw) == E, kw

    def pack(labels=0x1000, codes=0x2000, codes4=0x3000, n=10, M=8, ksub=16, flag=0x4000):
        return lib.grl_pq_pack(labels, codes, codes4, n, M, ksub, flag, None)
    assert pack(n=0) == 0 and pack(labels=None, n=0) == 0                      # labels may be NULL
    for kw in (dict(codes=None), dict(codes4=None), dict(flag=None), dict(n=-1), dict(M=0), dict(ksub=24),
               dict(codes4=0x3002)):
        assert pack(**kw) == E, kw

    def decode(cb=0x1000, codes=0x2000, out=0x3000, n=10, M=8, ksub=16, dsub=32, ldo=256):
        return lib.grl_pq_decode(cb, codes, out, n, M, ksub, dsub, ldo, None)
    assert decode(n=0) == 0
    for kw in (dict(cb=None), dict(codes=None), dict(out=None), dict(n=-1), dict(M=0), dict(ksub=3), dict(dsub=0),
               dict(dsub=30), dict(ldo=252), dict(ldo=258), dict(cb=0x1004), dict(out=0x3008)):
        assert decode(**kw) == E, kw


# ----------------------------------------------------------------------------
# the planted quality case, decided here: tests/test_gpu_pq.py reuses exactly these inputs on the device
# ----------------------------------------------------------------------------
def test_planted_identities_keep_their_rank_1_under_adc():
    """60 queries, 300 gallery rows of 10 identities, d = 256, M = 8, nbits = 4 (pq_ref.PLANTED).  Measured with the
    numpy model: all 60 rank-1 pids equal the exact ones; the smallest gap between a query's best other-pid and best
    same-pid ADC distance is 0.406 (cosine distances of unit rows: same-pid pairs sit near -0.61, others near 0)."""
    c = R.PLANTED
    qf, gf, q_pids, g_pids = R.planted_case()
    assert qf.shape == (60, 256) and gf.shape == (300, 256)
    C = R.train(gf, c['M'], c['nbits'], c['train_seed'], c['max_iter'])
    codes = R.encode(gf, C, R.euclid)
    D = R.adc_dist(R.lut_host(qf, C, 'cosine'), codes, 'cosine')
    exact = R.negdot(qf, gf)
    exact_pid = g_pids[R.search(exact, 1)[1][:, 0]]
    assert np.array_equal(exact_pid, q_pids)                     # the planted identities are what exact search finds
    adc_pid = g_pids[R.search(D, 1)[1][:, 0]]
    assert np.array_equal(adc_pid, exact_pid)                    # all 60, none left out
    same = g_pids[None, :] == q_pids[:, None]
    margin = (np.where(same, np.inf, D).min(1) - np.where(same, D, np.inf).min(1)).min()
    print('\n[planted PQ case] smallest other-pid minus same-pid ADC gap: %.4f' % margin)
    assert margin > 0
