"""Exact refinement of PQ / IVF-PQ shortlists without a GPU: the float32 model of the contract
(tests/refine_ref.py) against float64, the bf16 pack model on hand-picked bit patterns, ordering / padding / duplicates,
the planted case that tests/test_gpu_refine.py repeats on the device, the GRL_EVAL_REFINE knob, the binding and the
host-side argument checks of refine.hip."""
import os

import numpy as np
import pytest
import torch

import pq_ref as R
import refine_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
NAMES = ('grl_refine_scan', 'grl_refine_pack_bf16')
DS = (4, 252, 256, 260, 1028)


def _pairs(d, n=40, seed=0):
    g = np.random.Generator(np.random.PCG64(seed + d))
    return g.standard_normal((n, d)).astype(np.float32), g.standard_normal((n, d)).astype(np.float32)


@pytest.mark.parametrize('d', DS)
def test_the_model_agrees_with_float64_cosine(d):
    """|dist - exact| <= (ceil(d / 256) + 10) u sum_c |q_c| |x_c|: one rounding per product, ceil(d / 256) adds per partial,
    2 for the join, 6 for the butterfly, one unit for the second-order terms."""
    q, x = _pairs(d)
    got = F.pair_dist(q, x, 'cosine').astype(np.float64)
    q64, x64 = q.astype(np.float64), x.astype(np.float64)
    want = -(q64 * x64).sum(1)
    bound = (-(-d // 256) + 10) * U * (np.abs(q64) * np.abs(x64)).sum(1)
    assert (np.abs(got - want) <= bound).all()


@pytest.mark.parametrize('d', DS)
def test_the_model_agrees_with_float64_euclidean(d):
    """S against S* = sum_c (q_c - x_c)^2 in float64: e_c carries one rounding, so e_c^2 two, the product a third, where
    the cosine term had one -- (ceil(d / 256) + 12) u S* =: ES; then |sqrt(S) - sqrt(S*)| <= ES / sqrt(S*), plus the
    root's own rounding u sqrt(S*) (2 u taken, as tests/test_ivf_cpu.py does)."""
    q, x = _pairs(d, seed=7)
    got = F.pair_dist(q, x, 'euclidean').astype(np.float64)
    s = ((q.astype(np.float64) - x.astype(np.float64)) ** 2).sum(1)
    assert s.min() > 1e-2                                         # (the case keeps clear of the clamp)
    want = np.sqrt(s)
    ES = (-(-d // 256) + 12) * U * s
    assert (np.abs(got - want) <= ES / want + 2 * U * want).all()


def test_bf16_pack_model_rounds_to_nearest_even_on_hand_picked_patterns():
    cases = {0x3f800000: 0x3f80,                                  # 1.0
             0x3f808000: 0x3f80,                                  # an exact half above an even mantissa: down
             0x3f818000: 0x3f82,                                  # an exact half above an odd mantissa: up
             0x3f808001: 0x3f81, 0x3f807fff: 0x3f80,              # just above / below the half
             0x7f7fffff: 0x7f80, 0xff7fffff: 0xff80,              # FLT_MAX overflows to +-inf
             0x7f7f7fff: 0x7f7f,                                  # the largest value that stays finite
             0x7f800000: 0x7f80, 0xff800000: 0xff80,              # infinities
             0x7f800001: 0x7fc0, 0xffc00000: 0x7fc0, 0x7fffffff: 0x7fc0, 0xff80ffff: 0x7fc0,      # every NaN -> 0x7fc0
             0x00000000: 0x0000, 0x80000000: 0x8000,              # +-0
             0x00008000: 0x0000, 0x00018000: 0x0002, 0x80008001: 0x8001}      # denormals round the same way
    u = np.array(sorted(cases), np.uint32)
    got = F.pack_bf16(u.view(np.float32))
    assert got.dtype == np.uint16 and got.tolist() == [cases[int(v)] for v in u]
    w = F.widen(got)
    assert w.dtype == np.float32 and np.array_equal(w.view(np.uint32), got.astype(np.uint32) << 16)
    g = np.random.Generator(np.random.PCG64(3))
    x = g.standard_normal(4000).astype(np.float32)
    back = F.widen(F.pack_bf16(x)).astype(np.float64)
    assert (np.abs(back - x) <= 2.0 ** -8 * np.abs(x)).all()      # half an ulp of 8 significant bits: ulp <= 2^-7 |x|
    assert np.array_equal(F.store_rows(x.reshape(40, 100), 'bf16'), F.widen(F.pack_bf16(x)).reshape(40, 100))
    assert F.store_rows(x.reshape(40, 100), 'f32') is not None and np.array_equal(F.store_rows(x.reshape(40, 100)), x.reshape(40, 100))


def test_ordering_ties_padding_and_duplicates():
    rows = np.zeros((6, 4), np.float32)
    rows[:, 0] = [1.0, 3.0, 3.0, 2.0, 3.0, 0.5]
    q = np.array([[1, 0, 0, 0], [-1, 0, 0, 0]], np.float32)
    cand = np.array([[4, -1, 2, 6, 1, 3, 2, 10 ** 12, 0],
                     [-1, -5, 5, 0, 5, 6, 7, 3, -1]], np.int64)
    D, cidx = F.dist(q, rows, cand)
    assert cidx[0].tolist() == [4, -1, 2, -1, 1, 3, 2, -1, 0] and np.isposinf(D[0, [1, 3, 7]]).all()
    assert D[0, [0, 2, 4, 5, 6, 8]].tolist() == [-3.0, -3.0, -3.0, -2.0, -3.0, -1.0]
    dist, idx = F.rank(D, cidx, 9)
    assert idx[0].tolist() == [1, 2, 2, 4, 3, 0, -1, -1, -1]      # ties to the smaller gallery index; the duplicate twice
    assert dist[0].tolist()[:6] == [-3.0, -3.0, -3.0, -3.0, -2.0, -1.0] and np.isposinf(dist[0, 6:]).all()
    assert idx[1].tolist() == [5, 5, 0, 3, -1, -1, -1, -1, -1] and dist[1].tolist()[:4] == [0.5, 0.5, 1.0, 2.0]
    dist, idx = F.refine_lists(q, rows, cand, 2)
    assert idx.tolist() == [[1, 2], [5, 5]]
    # -0 == +0 and the canonical NaN sort as grl_row_argsort does: NaN last among the live, zeros tie by index
    rows2 = np.zeros((4, 4), np.float32)
    rows2[1, 0], rows2[2, 0], rows2[3, 0] = np.nan, -0.0, 1.0
    D, cidx = F.dist(np.array([[1, 0, 0, 0]], np.float32), rows2, np.array([[1, 2, 0, 3]], np.int64))
    assert D.view(np.uint32)[0, 0] == 0x7fc00000
    assert F.rank(D, cidx, 4)[1].tolist() == [[3, 0, 2, 1]]
    # the Euclidean clamp: a NaN argument and a zero give sqrt(1e-12)
    E = F.dist(np.zeros((1, 4), np.float32), rows2, np.array([[0, 1, 3]], np.int64), 'euclidean')[0]
    floor = np.sqrt(np.float32(1e-12))
    assert E[0, 0] == floor and E[0, 1] == floor and E[0, 2] == 1.0
    with pytest.raises(ValueError):
        F.pair_dist(np.zeros((1, 6), np.float32), np.zeros((1, 6), np.float32))
    with pytest.raises(ValueError):
        F.pair_dist(np.zeros((1, 16388), np.float32), np.zeros((1, 16388), np.float32))


# ----------------------------------------------------------------------------
# the planted case, decided here: tests/test_gpu_refine.py reuses exactly these inputs on the device
# ----------------------------------------------------------------------------
PLANTED_R, PLANTED_K = 40, 10
_planted = {}


def planted():
    """pq_ref's planted case with its codes and the ADC shortlist of R = 40: built once, never modified"""
    if not _planted:
        c = R.PLANTED
        qf, gf, q_pids, g_pids = R.planted_case()
        C = R.train(gf, c['M'], c['nbits'], c['train_seed'], c['max_iter'])
        codes = R.encode(gf, C, R.euclid)
        D = R.adc_dist(R.lut_host(qf, C, 'cosine'), codes)
        _planted.update(qf=qf, gf=gf, short=R.search(D, PLANTED_R)[1], adc=R.search(D, PLANTED_K)[1])
    return _planted


def _exact64(qf, rows, k):
    D = -(qf.astype(np.float64) @ rows.astype(np.float64).T)
    return np.argsort(D, axis=1, kind='stable')[:, :k], np.sort(D, axis=1)


def test_planted_case_refined_recall_is_one_where_adc_is_below_half():
    """Measured with the numpy model: ADC recall@1 / @10 against the float64 ranking 0.017 / 0.385; refined at R = 40
    1.000 / 1.000.  The smallest gap among the first 11 places of any query is 4.27e-6 in float64 against a model error of
    8.7e-8, so the order is decided."""
    p = planted()
    exact, sorted64 = _exact64(p['qf'], p['gf'], PLANTED_K)
    gap = np.diff(sorted64[:, :PLANTED_K + 1], axis=1).min()
    adc = R.recall(p['adc'], exact, (1, PLANTED_K))
    dist, idx = F.refine_lists(p['qf'], p['gf'], p['short'], PLANTED_K)
    err = np.abs(dist.astype(np.float64) - np.take_along_axis(-(p['qf'].astype(np.float64) @ p['gf'].astype(np.float64).T), idx, 1)).max()
    got = R.recall(idx, exact, (1, PLANTED_K))
    print('\n[planted refine case] ADC recall@1 / @10 %.3f / %.3f, refined at R = %d %.3f / %.3f; smallest gap %.3g, model '
          'error %.3g' % (adc[0], adc[1], PLANTED_R, got[0], got[1], gap, err))
    assert gap > 10 * err
    assert adc[1] < 0.5
    assert got == [1.0, 1.0]


def test_planted_case_with_a_bf16_store():
    """the same against the float64 ranking of the WIDENED rows (what the store holds is what is ranked); the figure
    against the fp32 rows' ranking is printed (measured: 1.000)"""
    p = planted()
    rows = F.store_rows(p['gf'], 'bf16')
    assert not np.array_equal(rows, p['gf'])
    exact = _exact64(p['qf'], rows, PLANTED_K)[0]
    idx = F.refine_lists(p['qf'], rows, p['short'], PLANTED_K)[1]
    got = R.recall(idx, exact, (1, PLANTED_K))
    vs32 = R.recall(idx, _exact64(p['qf'], p['gf'], PLANTED_K)[0], (1, PLANTED_K))
    print('\n[planted refine case, bf16 store] refined recall@1 / @10 against the widened rows %.3f / %.3f, against the fp32 '
          'rows %.3f / %.3f' % (got[0], got[1], vs32[0], vs32[1]))
    assert got == [1.0, 1.0]


# ----------------------------------------------------------------------------
# the knob, the binding, the host-side checks
# ----------------------------------------------------------------------------
def test_the_evaluator_knob_parses():
    from grl_amd.reid.evaluator.attevaluator import parse_refine_knob as parse
    name = 'GRL_EVAL_REFINE'
    assert parse(name, None) is None and parse(name, '') is None and parse(name, '  ') is None
    good, bad = F.parse_knob_cases()
    for text, want in good.items():
        assert parse(name, text) == want, text
    for text in bad:
        with pytest.raises(ValueError, match=name) as err:
            parse(name, text)
        assert repr(text) in str(err.value)


class _Never(object):
    def __getattr__(self, name):
        raise AssertionError('touched %s' % name)


KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_CLUSTER', 'GRL_EVAL_CLUSTER_JACCARD', 'GRL_EVAL_KMEANS', 'GRL_EVAL_HDBSCAN', 'GRL_EVAL_TSNE',
         'GRL_EVAL_SILHOUETTE', 'GRL_EVAL_PCA', 'GRL_EVAL_DIFFUSION', 'GRL_EVAL_SET', 'GRL_EVAL_PQ', 'GRL_EVAL_IVF',
         'GRL_EVAL_REFINE')


def test_the_knob_needs_the_pq_knob_and_inherits_its_refusals(monkeypatch):
    from grl_amd.reid.evaluator import ATTEvaluator
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)

    def run(only_eval=True, rerank=0):
        ATTEvaluator(_Never(), _Never(), only_eval).evaluate(None, None, _Never(), _Never(), '', 0, rerank)
    monkeypatch.setenv('GRL_EVAL_REFINE', '40,fp16')
    with pytest.raises(ValueError, match="GRL_EVAL_REFINE.*'40,fp16'"):
        run()
    monkeypatch.setenv('GRL_EVAL_REFINE', '40,bf16')
    with pytest.raises(ValueError, match='GRL_EVAL_REFINE=40,bf16 needs GRL_EVAL_PQ'):
        run()
    monkeypatch.setenv('GRL_EVAL_PQ', '8,4')
    with pytest.raises(ValueError, match='GRL_EVAL_PQ=8,4 cannot re-rank'):
        run(rerank=1)
    monkeypatch.setenv('GRL_EVAL_SET', 'min')
    with pytest.raises(ValueError, match='GRL_EVAL_PQ=8,4 cannot be combined with GRL_EVAL_SET'):
        run()
    monkeypatch.delenv('GRL_EVAL_SET')
    monkeypatch.setenv('GRL_EVAL_IVF', '4,2')
    for only_eval in (True, False):                               # accepted: it gets as far as the models and loaders
        with pytest.raises(AssertionError, match='touched'):
            run(only_eval=only_eval)


def test_the_public_functions_validate_before_the_device(monkeypatch):
    from grl_amd import engine
    from grl_amd._lib import GrlHipError

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    monkeypatch.setattr(engine, '_call', no_device)
    assert engine.REFINE_D_MAX == F.D_MAX == 16384 and engine.REFINE_TYPES == {'f32': 0, 'bf16': 1}
    host = torch.zeros(30, 256)
    with pytest.raises(ValueError, match="dtype must be 'f32' or 'bf16'"):
        engine.RefineStore(host, 'f16')
    with pytest.raises(ValueError, match=r'xf must be a \[n, d\] tensor'):
        engine.RefineStore(host[0])
    for d in (6, 16388, 0):
        with pytest.raises(ValueError, match='xf must have d columns with d a multiple of 4 in 1..16384'):
            engine.RefineStore(torch.zeros(3, d))
    with pytest.raises(GrlHipError, match='HIP device'):
        engine.RefineStore(host)
    store = engine.RefineStore.__new__(engine.RefineStore)
    store.n, store.d, store.dtype = 30, 256, 'f32'
    cand = torch.zeros((30, 5), dtype=torch.int64)
    for fn, args in ((engine.refine_dist, ()), (engine.refine_lists, (3,))):
        with pytest.raises(ValueError, match="metric must be 'cosine' or 'euclidean'"):
            fn(host, store, cand, *args, metric='l1')
        with pytest.raises(ValueError, match='store must be a RefineStore'):
            fn(host, host, cand, *args)
        with pytest.raises(ValueError, match=r'qf must be \[rows, d\] = \[rows, 256\]'):
            fn(host[:, :128], store, cand, *args)
        for bad in (cand.to(torch.int32), cand[:7], cand[0]):
            with pytest.raises(ValueError, match='cand must be an int64 device tensor'):
                fn(host, store, bad, *args)
        with pytest.raises(GrlHipError, match='HIP device'):
            fn(host, store, cand, *args)
    vm = engine.VerifyMetric.__new__(engine.VerifyMetric)
    with pytest.raises(ValueError, match='verify_metric'):
        engine.refine_lists(host, store, cand, 3, metric=vm)
    with pytest.raises(ValueError, match='index must be a PqIndex or an IvfPqIndex'):
        engine.refine_search(host, host, store, 3, 10)
    flat = engine.PqIndex.__new__(engine.PqIndex)
    flat.codebook = engine.PqCodebook.__new__(engine.PqCodebook)
    flat.codebook.metric, flat.codebook.d, flat.n = 'cosine', 256, 30
    ivf = engine.IvfPqIndex.__new__(engine.IvfPqIndex)
    ivf.book = engine.IvfPqCodebook.__new__(engine.IvfPqCodebook)
    ivf.book.metric, ivf.book.d, ivf.book.nlist, ivf.n = 'cosine', 256, 4, 30
    with pytest.raises(ValueError, match='nprobe is for an IvfPqIndex'):
        engine.refine_search(host, flat, store, 3, 10, nprobe=2)
    with pytest.raises(ValueError, match='nprobe is required for an IvfPqIndex'):
        engine.refine_search(host, ivf, store, 3, 10)
    with pytest.raises(ValueError, match='store must be a RefineStore'):
        engine.refine_search(host, flat, host, 3, 10)
    for n, d in ((31, 256), (30, 128)):
        store.n, store.d = n, d
        for index, kw in ((flat, {}), (ivf, dict(nprobe=2))):
            with pytest.raises(ValueError, match='store must hold the rows of the index'):
                engine.refine_search(host, index, store, 3, 10, **kw)
    store.n, store.d = 30, 256
    for k in (0, 1025, 2.0):
        with pytest.raises(ValueError, match=r'k must be an integer in 1\.\.1024'):
            engine.refine_search(host, flat, store, k, 10)
    for k, R_ in ((5, 4), (5, 1025), (1, 0)):
        with pytest.raises(ValueError, match=r'R \(k <= R <= 1024\) must be an integer in %d\.\.1024' % k):
            engine.refine_search(host, flat, store, k, R_)
    with pytest.raises(ValueError, match=r'k must be an integer in 1\.\.1024'):
        engine.refine_lists(host, store, cand, 0)


def test_library_exports_and_header_declare_the_entry_points():
    import ctypes
    from grl_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'grl_hip.h')).read()
    assert sorted(n for n in _lib._SIGNATURES if n.startswith('grl_refine_')) == sorted(NAMES)
    for name in NAMES:
        assert 'int %s(' % name in header, name
    srcs = open(os.path.join(ROOT, 'grl_amd', 'csrc', 'Makefile')).read().split('SRCS =')[1].split('\n')[0]
    assert ' refine.hip ' in srcs
    assert _lib.ABI_VERSION == 10 and int(header.split('#define GRL_ABI_VERSION')[1].split()[0]) == 10     # additive only
    for word, value in (('GRL_REFINE_D_MAX', 16384), ('GRL_REFINE_F32', 0), ('GRL_REFINE_BF16', 1)):
        assert '#define %s' % word in header and int(header.split('#define %s' % word)[1].split()[0]) == value
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.exported_symbols() and getattr(lib, name).restype is not None and hasattr(raw, name), name


def test_host_argument_checks_return_einval_through_the_c_abi():
    from grl_amd import _lib
    lib = _lib.load()
    E = _lib.GRL_EINVAL
    # fake device pointers (never dereferenced: every call below is refused, or has nothing to launch)

    def scan(q=0x1000, ldq=None, store=0x20000, lds=None, typ=0, cand=0x3000, ldc=None, out=0x4000, cidx=0x5000, ldo=None,
             nq=3, L=7, n=100, d=256, metric=0):
        return lib.grl_refine_scan(q, d if ldq is None else ldq, store, d if lds is None else lds, typ, cand,
                                   L if ldc is None else ldc, out, cidx, L if ldo is None else ldo, nq, L, n, d, metric, None)
    assert scan(nq=0) == 0 and scan(L=0) == 0 and scan(nq=0, typ=1, metric=1) == 0      # nothing to do, nothing launched
    for kw in (dict(q=None), dict(store=None), dict(cand=None), dict(out=None), dict(cidx=None), dict(nq=-1), dict(L=-1),
               dict(n=-1), dict(n=2 ** 31), dict(d=0), dict(d=-4), dict(d=6), dict(d=254), dict(d=16388), dict(typ=2),
               dict(typ=-1), dict(metric=2), dict(metric=-1), dict(ldq=252), dict(lds=252), dict(ldq=258), dict(lds=258),
               dict(ldc=6), dict(ldo=6), dict(nq=65536), dict(q=0x1008), dict(store=0x20008), dict(store=0x20004, typ=1),
               dict(cand=0x3004), dict(out=0x4002), dict(cidx=0x5001)):
        assert scan(nq=0, **kw) == E if 'nq' not in kw else scan(**kw) == E, kw
    assert b'refine_scan' in lib.grl_last_error()
    assert scan(nq=0, store=0x20008, typ=1) == 0 and scan(nq=0, d=16384) == 0 and scan(nq=0, d=4) == 0

    def pack(x=0x1000, out=0x2000, count=10):
        return lib.grl_refine_pack_bf16(x, out, count, None)
    assert pack(count=0) == 0
    for kw in (dict(x=None), dict(out=None), dict(count=-1), dict(x=0x1002), dict(out=0x2001)):
        assert pack(count=0, **kw) == E if 'count' not in kw else pack(**kw) == E, kw
    assert b'refine_pack_bf16' in lib.grl_last_error()
