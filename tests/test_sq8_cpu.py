"""The int8 scalar quantiser on the host: the numpy model of tests/sq8_ref.py against float64, its derived
error bound and ranking floor, the evaluator knob's grammar and refusals, the binding and the host-side checks.  No device."""
import os

import numpy as np
import pytest
import torch

import sq8_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('grl_sq8_absmax', 'grl_sq8_steps', 'grl_sq8_encode', 'grl_sq8_decode', 'grl_sq8_query', 'grl_sq8_scan',
         'grl_sq8_scan_i32')


def _case(seed, n=200, d=128, nq=20):
    gal, qry = S.recipe(seed, n=n, d=d, nq=nq)
    mean, delta, inv = S.train(gal)
    codes = S.encode(gal, mean, inv)
    qcodes, scale = S.query(qry, delta)
    return gal, qry, mean, delta, inv, codes, qcodes, scale


# ----------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('d', (1, 60, 64, 68, 128))
def test_the_integer_sum_is_the_int64_product_and_the_layout_is_padded_with_zeros(d):
    gal, qry, mean, delta, inv, codes, qcodes, scale = _case(3, n=70, d=d, nq=9)
    dp = S.dpad(d)
    assert dp % 64 == 0 and 0 <= dp - d < 64
    assert codes.shape == (70, dp) and qcodes.shape == (9, dp) and codes.dtype == np.int8 and qcodes.dtype == np.int8
    assert not codes[:, d:].any() and not qcodes[:, d:].any()
    assert np.abs(codes.astype(np.int64)).max() <= 127 and np.abs(qcodes.astype(np.int64)).max() <= 127
    want = np.einsum('qj,gj->qg', qcodes[:, :d].astype(np.int64), codes[:, :d].astype(np.int64))
    assert np.array_equal(S.isum(qcodes, codes), want)
    # the extreme row of every non-constant column reaches +-127, and the query's largest column too
    assert (np.abs(codes[:, :d].astype(np.int64)).max(0)[delta > 0] == 127).all()
    assert (np.abs(qcodes.astype(np.int64)).max(1) == 127).all()
    D = S.dist(qcodes, scale, S.bias_host(qry, mean), codes)
    assert D.dtype == np.float32 and D.shape == (9, 70)


def test_special_values_follow_the_stated_rules():
    mean = np.array([0.5, 0.0, 0.0, 1.0], dtype=np.float32)
    amax = np.array([2.0, 0.0, 1.0, 4.0], dtype=np.float32)
    delta, inv = S.steps_from_amax(amax)
    assert inv[1] == 0 and delta[1] == 0 and np.array_equal(S.inv_from_delta(delta)[[1]], [0])
    x = np.array([[np.nan, 3.0, np.inf, -100.0], [2.5, np.nan, -np.inf, 5.0], [0.5, -0.0, 1e-45, 1.0]], dtype=np.float32)
    c = S.encode(x, mean, inv)[:, :4]
    assert c.tolist() == [[0, 0, 127, -127], [127, 0, -127, 127], [0, 0, 0, 0]]
    assert S.absmax(x, mean).tolist() == [2.0, 3.0, np.inf, 101.0]                         # NaN ignored, inf kept
    # rint is half to even: (x - mean) * inv = 0.5, 1.5, 2.5 -> 0, 2, 2
    one = np.ones(1, dtype=np.float32)
    assert S.encode(np.array([[0.5], [1.5], [2.5], [-0.5], [-1.5]], dtype=np.float32), 0 * one, one)[:, 0].tolist() == [0, 2, 2, 0, -2]
    # queries: a NaN or infinite w codes as 0 and is left out of the maximum; an all-zero query has scale 0
    d1 = np.array([1.0, 1.0, 1.0, 0.0], dtype=np.float32)
    q = np.array([[np.nan, 2.0, -1.0, 9.0], [np.inf, -0.5, 0.25, 1.0], [0.0, -0.0, 0.0, 7.0], [1.0, np.inf, np.inf, 0.0]], dtype=np.float32)
    qc, sc = S.query(q, d1)
    assert qc[:, :4].tolist() == [[0, 127, -64, 0], [0, -127, 64, 0], [0, 0, 0, 0], [127, 0, 0, 0]]
    assert np.array_equal(sc, (np.array([2.0, 0.5, 0.0, 1.0], dtype=np.float32) / np.float32(127)).astype(np.float32))
    # decode: one multiply, one add
    got = S.decode(np.array([[127, -128, 3, 0]], dtype=np.int8), mean, delta)
    want = [np.float32(m) + np.float32(np.float32(dl) * np.float32(cc)) for m, dl, cc in zip(mean, delta, (127, -128, 3, 0))]
    assert got[0].tolist() == [float(w) for w in want]
    # the float conversion of a sum above 2^24 rounds to nearest even
    big = np.array([[2 ** 24 + 1, 2 ** 24 + 3]], dtype=np.int64)
    assert big.astype(np.float32).tolist() == [[2.0 ** 24, 2.0 ** 24 + 4]]


@pytest.mark.parametrize('seed', S.RECIPE['seeds'])
def test_the_cosine_distance_is_within_the_derived_bound_of_the_true_dot_product(seed):
    """|model - (-q.g)| <= (s_q / 2) sum_j |c[j]| + sum_j |q[j]| delta[j] / 2 + slack, per pair, in float64.

    With w = q delta and s_q = scale: q.g^ = sum_j q[j] mean[j] + sum_j w[j] c[j]; the query's code is cq[j] = w[j] / s_q
    up to half a step, which moves the sum by at most (s_q / 2) sum |c[j]|; g^ differs from g by at most delta[j] / 2 per
    column (no trained row is clamped), which moves q.g by at most sum |q[j]| delta[j] / 2.  The slack is fp32 rounding,
    derived from d: the model's r = 127 / s and w r are rounded (2 ulp of up to 127 per column before rint can cross a
    half: covered by widening the half step by 127 * 2^-22 per column), the row's (x - mean) * inv likewise, and the three
    float32 operations of dot plus the float32 bias stand-in round at 2^-24 relative to |dot| + |bias| <= 2 (unit rows):
    slack = 2^-22 * (127 * (s_q sum|c| + sum|q| delta) + 4)."""
    gal, qry, mean, delta, inv, codes, qcodes, scale = _case(seed, n=S.RECIPE['n'], d=S.RECIPE['d'], nq=S.RECIPE['nq'])
    D = S.dist(qcodes, scale, S.bias_host(qry, mean), codes).astype(np.float64)
    true = -(qry.astype(np.float64) @ gal.astype(np.float64).T)
    sq = scale.astype(np.float64)
    abs_c = np.abs(codes.astype(np.float64)).sum(1)
    t1 = 0.5 * sq[:, None] * abs_c[None, :]
    t2 = 0.5 * (np.abs(qry.astype(np.float64)) @ delta.astype(np.float64))[:, None]
    slack = 2.0 ** -22 * (127.0 * 2.0 * (t1 + t2) + 4.0)
    err = np.abs(D - true)
    print('seed %d: max err %.3e, min bound %.3e, max err / bound %.3f' % (seed, err.max(), (t1 + t2).min(), (err / (t1 + t2 + slack)).max()))
    assert (err <= t1 + t2 + slack).all()


@pytest.mark.parametrize('seed', S.RECIPE['seeds'])
def test_the_ranking_floor_of_the_recipe(seed):
    """recall@10 of the model's cosine ranking against the float64 ranking is >= 0.95 on the recipe (n = 1000, d = 128, 50
    queries).  Measured with this model: seed 0: 0.990, seed 1: 0.984, seed 2: 0.986."""
    r = S.RECIPE
    gal, qry, mean, delta, inv, codes, qcodes, scale = _case(seed, n=r['n'], d=r['d'], nq=r['nq'])
    D = S.dist(qcodes, scale, S.bias_host(qry, mean), codes)
    rec = S.recall_at(S.ranked(D, 10), S.exact_lists(qry, gal, 10), 10)
    print('seed %d: recall@10 %.4f' % (seed, rec))
    assert rec >= r['floor']
    # and by 'euclidean' the same lists up to ties of unit rows: the floor holds there too
    gg = S.sqnorm_host(S.decode(codes, mean, delta))
    De = S.dist(qcodes, scale, S.bias_host(qry, mean), codes, 'euclidean', S.sqnorm_host(qry), gg)
    assert S.recall_at(S.ranked(De, 10), S.exact_lists(qry, gal, 10), 10) >= r['floor']


# ----------------------------------------------------------------------------
# the knob, the binding, the host-side checks
# ----------------------------------------------------------------------------
def test_the_evaluator_knob_parses():
    from grl_amd.reid.evaluator.attevaluator import parse_sq8_knob as parse
    name = 'GRL_EVAL_SQ8'
    assert parse(name, None) is None and parse(name, '') is None and parse(name, '  ') is None
    good, bad = S.parse_knob_cases()
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
         'GRL_EVAL_REFINE', 'GRL_EVAL_NNG', 'GRL_EVAL_BIN', 'GRL_EVAL_SQ8')


def test_the_knob_is_refused_with_what_the_bin_knob_is_refused_with(monkeypatch):
    from grl_amd.reid.evaluator import ATTEvaluator
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)

    def run(only_eval=True, rerank=0):
        ATTEvaluator(_Never(), _Never(), only_eval).evaluate(None, None, _Never(), _Never(), '', 0, rerank)
    monkeypatch.setenv('GRL_EVAL_SQ8', '2')
    with pytest.raises(ValueError, match="GRL_EVAL_SQ8.*'2'"):
        run()
    monkeypatch.setenv('GRL_EVAL_SQ8', '1,16,bf16')
    with pytest.raises(ValueError, match='GRL_EVAL_SQ8=1,16,bf16 cannot re-rank'):
        run(rerank=1)
    for other, value in (('GRL_EVAL_SET', 'min'), ('GRL_EVAL_DIFFUSION', '10'), ('GRL_EVAL_METRIC', 'verify')):
        monkeypatch.setenv(other, value)
        with pytest.raises(ValueError, match='GRL_EVAL_SQ8=1,16,bf16 cannot be combined with %s' % other):
            run()
        monkeypatch.delenv(other)
    for only_eval in (True, False):                               # accepted: it gets as far as the models and loaders
        with pytest.raises(AssertionError, match='touched'):
            run(only_eval=only_eval)


def test_library_exports_and_header_declare_the_entry_points():
    import ctypes
    from grl_amd import _lib, engine
    header = open(os.path.join(ROOT, 'include', 'grl_hip.h')).read()
    assert sorted(n for n in _lib._SIGNATURES if n.startswith('grl_sq8_')) == sorted(NAMES)
    for name in NAMES:
        assert '%s(' % name in header, name
    srcs = open(os.path.join(ROOT, 'grl_amd', 'csrc', 'Makefile')).read().split('SRCS =')[1].split('\n')[0]
    assert ' sq8.hip ' in srcs
    assert _lib.ABI_VERSION == 10 and int(header.split('#define GRL_ABI_VERSION')[1].split()[0]) == 10     # additive only
    for word, value in (('GRL_SQ8_D_MAX', S.D_MAX), ('GRL_SQ8_TILE', S.TILE), ('GRL_SQ8_NQ_MAX', S.NQ_MAX)):
        assert int(header.split('#define %s' % word)[1].split()[0]) == value
    assert (engine.SQ8_D_MAX, engine.SQ8_TILE, engine.SQ8_NQ_MAX) == (S.D_MAX, S.TILE, S.NQ_MAX)
    assert S.D_MAX * 128 * 128 < 2 ** 31                          # the int32 accumulator holds every sum
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.exported_symbols() and getattr(lib, name).restype is not None and hasattr(raw, name), name


def test_host_argument_checks_return_einval_through_the_c_abi():
    from grl_amd import _lib
    lib = _lib.load()
    E = _lib.GRL_EINVAL
    # fake device pointers (never dereferenced: every call below is refused, or has nothing to launch)

    def scan(q=0x1000, ldqc=64, c=0x2000, ldc=64, scale=0x3000, bias=0x4000, qq=None, gg=None, out=0x5000, ldo=0, nq=0, n=0,
             dpad=64, metric=0):
        return lib.grl_sq8_scan(q, ldqc, c, ldc, scale, bias, qq, gg, out, ldo, nq, n, dpad, metric, None)
    assert scan() == 0 and scan(nq=5) == 0 and scan(n=7, ldo=9, dpad=16384, ldqc=16384, ldc=16400) == 0
    assert scan(metric=1, qq=0x6000, gg=0x7000) == 0
    for kw in (dict(q=None), dict(c=None), dict(out=None), dict(scale=None), dict(bias=None), dict(nq=-1), dict(n=-1),
               dict(dpad=0), dict(dpad=32), dict(dpad=96), dict(dpad=16448, ldqc=16448, ldc=16448), dict(ldqc=48), dict(ldc=48),
               dict(ldqc=72), dict(ldc=100), dict(n=7, ldo=6), dict(q=0x1008), dict(c=0x2004), dict(out=0x5002),
               dict(scale=0x3001), dict(bias=0x4002), dict(metric=2), dict(metric=-1), dict(metric=1), dict(metric=1, qq=0x6000),
               dict(metric=1, qq=0x6002, gg=0x7000), dict(nq=S.NQ_MAX + 1)):
        assert scan(**kw) == E, kw
    assert b'sq8_scan' in lib.grl_last_error()

    def raw(q=0x1000, ldqc=64, c=0x2000, ldc=64, out=0x5000, ldo=0, nq=0, n=0, dpad=64):
        return lib.grl_sq8_scan_i32(q, ldqc, c, ldc, out, ldo, nq, n, dpad, None)
    assert raw() == 0
    for kw in (dict(q=None), dict(c=None), dict(out=None), dict(nq=-1), dict(n=-1), dict(dpad=100), dict(ldqc=32), dict(ldc=88),
               dict(n=3, ldo=2), dict(q=0x1001), dict(c=0x2008), dict(out=0x5001), dict(nq=S.NQ_MAX + 1)):
        assert raw(**kw) == E, kw
    assert b'sq8_scan_i32' in lib.grl_last_error()

    def absmax(x=0x1000, ldx=8, mean=0x2000, amax=0x3000, n=-1, d=8):
        return lib.grl_sq8_absmax(x, ldx, mean, amax, n, d, None)
    for kw in (dict(), dict(n=0, x=None), dict(n=0, mean=None), dict(n=0, amax=None), dict(n=0, d=0), dict(n=0, d=16385),
               dict(n=0, ldx=7), dict(n=0, x=0x1002), dict(n=0, mean=0x2001), dict(n=0, amax=0x3002)):
        assert absmax(**kw) == E, kw
    assert b'sq8_absmax' in lib.grl_last_error()

    def steps(amax=None, delta=0x1000, inv=0x2000, d=0):
        return lib.grl_sq8_steps(amax, delta, inv, d, None)
    for kw in (dict(), dict(d=8, delta=None), dict(d=8, inv=None), dict(d=16385), dict(d=8, amax=0x3001), dict(d=8, delta=0x1002),
               dict(d=8, inv=0x2002)):
        assert steps(**kw) == E, kw
    assert b'sq8_steps' in lib.grl_last_error()

    def encode(x=0x1000, ldx=70, mean=0x2000, inv=0x3000, codes=0x4000, ldc=128, n=0, d=70):
        return lib.grl_sq8_encode(x, ldx, mean, inv, codes, ldc, n, d, None)
    assert encode() == 0 and encode(ldc=144) == 0
    for kw in (dict(x=None), dict(mean=None), dict(inv=None), dict(codes=None), dict(n=-1), dict(d=0), dict(d=16385), dict(ldx=69),
               dict(ldc=64), dict(ldc=136), dict(x=0x1001), dict(mean=0x2002), dict(inv=0x3002), dict(codes=0x4008)):
        assert encode(**kw) == E, kw
    assert b'sq8_encode' in lib.grl_last_error()

    def decode(codes=0x1000, ldc=128, mean=0x2000, delta=0x3000, out=0x4000, ldo=70, n=0, d=70):
        return lib.grl_sq8_decode(codes, ldc, mean, delta, out, ldo, n, d, None)
    assert decode() == 0 and decode(ldc=70, codes=0x1001) == 0
    for kw in (dict(codes=None), dict(mean=None), dict(delta=None), dict(out=None), dict(n=-1), dict(d=0), dict(ldc=69),
               dict(ldo=69), dict(mean=0x2001), dict(delta=0x3002), dict(out=0x4002)):
        assert decode(**kw) == E, kw
    assert b'sq8_decode' in lib.grl_last_error()

    def query(q=0x1000, ldq=70, delta=0x2000, qcodes=0x3000, ldc=128, scale=0x4000, nq=0, d=70):
        return lib.grl_sq8_query(q, ldq, delta, qcodes, ldc, scale, nq, d, None)
    assert query() == 0
    for kw in (dict(q=None), dict(delta=None), dict(qcodes=None), dict(scale=None), dict(nq=-1), dict(d=0), dict(d=16385),
               dict(ldq=69), dict(ldc=64), dict(ldc=132), dict(q=0x1002), dict(delta=0x2001), dict(qcodes=0x3004),
               dict(scale=0x4002), dict(nq=S.NQ_MAX + 1)):
        assert query(**kw) == E, kw
    assert b'sq8_query' in lib.grl_last_error()


def test_the_public_functions_validate_before_the_device(monkeypatch):
    from grl_amd import engine

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    monkeypatch.setattr(engine, '_call', no_device)
    monkeypatch.setattr(engine, 'gemm', no_device)
    host = torch.zeros((40, 64))
    for bad in (host, host.to(torch.float64), host.view(-1), [[1.0]]):
        with pytest.raises(ValueError, match='sq8_train: xf must be a 2-d float32 tensor on a HIP device'):
            engine.sq8_train(bad)
    for bad in (torch.zeros(64), torch.zeros((1, 64)), 3.0):
        with pytest.raises(ValueError, match=r'Sq8Codebook: mean must be a float32 device tensor \[d\]'):
            engine.Sq8Codebook(bad, torch.zeros(64))
    with pytest.raises(ValueError, match="Sq8Codebook: metric must be 'cosine' or 'euclidean'"):
        engine.Sq8Codebook(torch.zeros(64), torch.zeros(64), 'l1')
    with pytest.raises(ValueError, match="sq8_train: metric must be 'cosine' or 'euclidean'"):
        monkeypatch.setattr(engine, '_pca_matrix', lambda t, what, name: t)
        engine.sq8_train(host, 'l1')
    with pytest.raises(ValueError, match='sq8_train: xf needs at least one row and 1..16384 columns'):
        engine.sq8_train(host[:0])
    with pytest.raises(ValueError, match='sq8_train: xf needs at least one row and 1..16384 columns'):
        engine.sq8_train(torch.zeros((2, 16385)))
    for fn, name in ((engine.Sq8Index, 'Sq8Index'), (engine.sq8_index, 'sq8_index')):
        with pytest.raises(ValueError, match='%s: codebook must be a Sq8Codebook' % name):
            fn(host, host)
    # a stand-in codebook and index: the argument checks that follow need no device
    book = engine.Sq8Codebook.__new__(engine.Sq8Codebook)
    book.d, book.dpad, book.metric = 70, 128, 'cosine'
    for fn, name in ((book.encode, 'xf'), (book.query, 'qf')):
        with pytest.raises(ValueError, match=r'%s must be \[rows, d\] = \[rows, 70\]' % name):
            fn(torch.zeros((3, 64)))
    for wrong in (torch.zeros((5, 70), dtype=torch.uint8), torch.zeros((5, 70)), 7, torch.zeros((5, 64), dtype=torch.int8)):
        monkeypatch.undo()
        monkeypatch.setattr(engine, '_call', no_device)
        with pytest.raises(ValueError, match=r'Sq8Index: codes must be an int8 device tensor \[rows, dpad\] = \[rows, 128\] or '
                                             r'\[rows, d\] = \[rows, 70\]'):
            engine.Sq8Index(book, wrong)
        with pytest.raises(ValueError, match='Sq8Codebook.decode: codes must be an int8 device tensor'):
            book.decode(wrong)
    monkeypatch.setattr(engine, '_pca_matrix', lambda t, what, name: t)
    index = engine.Sq8Index.__new__(engine.Sq8Index)
    index.codebook, index.d, index.n = book, 70, 40
    q = torch.zeros((3, 70))
    for fn in (engine.sq8_dist, engine.sq8_search, engine.sq8_metrics_streaming, engine.sq8_refine_search, engine._Sq8Blocks):
        with pytest.raises(ValueError, match='index must be a Sq8Index'):
            fn(q, book, *((None,) * (4 if fn is engine.sq8_metrics_streaming else 3 if fn is engine.sq8_refine_search
                                    else 1 if fn is engine.sq8_search else 0)))
    for k in (0, 1025, True, -1):
        with pytest.raises(ValueError, match=r'sq8_search: k must be in 1..1024'):
            engine.sq8_search(q, index, k)
    with pytest.raises(ValueError, match=r'sq8_search: qf must be \[rows, d\] = \[rows, 70\]'):
        engine.sq8_search(torch.zeros((3, 64)), index, 5)
    with pytest.raises(ValueError, match=r'sq8_metrics_streaming: qf must be \[rows, d\] = \[rows, 70\]'):
        engine.sq8_metrics_streaming(torch.zeros((3, 64)), index, None, None, None, None)
    with pytest.raises(ValueError, match='sq8_refine_search: store must be a RefineStore'):
        engine.sq8_refine_search(q, index, host, 5, 10)
    store = engine.RefineStore.__new__(engine.RefineStore)
    store.n, store.d = 41, 70
    with pytest.raises(ValueError, match=r'sq8_refine_search: store must hold the rows of the index: store is \[41, 70\], the '
                                         r'index \[40, 70\]'):
        engine.sq8_refine_search(q, index, store, 5, 10)
    store.n = 40
    for k, R in ((0, 10), (11, 10), (5, 1025), (5.0, 10), (5, True)):
        with pytest.raises(ValueError, match='sq8_refine_search: (k|R)'):
            engine.sq8_refine_search(q, index, store, k, R)
    with pytest.raises(ValueError, match='Sq8Index.reconstruct: rows must be a 1-d integer device tensor'):
        index.reconstruct(torch.zeros(3, dtype=torch.int64))
