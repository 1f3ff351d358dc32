"""Ranking by the Siamese verification head without a GPU: the fold of tests/verify_ref.py against the head taken
literally, the exported entry points and their argument checks, engine.verify_metric's refusals (all of which come
before any device call) and the evaluator's GRL_EVAL_METRIC knob."""
import numpy as np
import pytest
import torch

import verify_ref as V


@pytest.mark.parametrize('beta', [1.0, 0.35])
@pytest.mark.parametrize('d,D,col0', [(96, 32, 32), (192, 64, 64), (160, 64, 0), (160, 64, 96)])
def test_the_fold_reproduces_the_literal_head(beta, d, D, col0):
    """float64 against float64: the two differ by rounding alone.  1e-12 is relative to the entry itself."""
    head = V.make_head(D, seed=d + D)
    assert (head['gamma'] < 0).any() and (head['gamma'] == 0).any() and (head['gamma'] > 0).any()
    dw = head['W'][1] - head['W'][0]
    assert (dw < 0).any() and (dw > 0).any()
    q, g = V.features(7, 33, d, col0, D, seed=3)
    w, c = V.fold(head)
    want = V.literal_F(q, g, col0, head, beta)
    got = V.folded_F(q, g, col0, w, c, beta)
    qv, rq, rg = V.row_terms(q, g, col0, w, c, beta)
    scale = np.abs(qv) @ np.abs(g.astype(np.float64)).T + np.abs(rq)[:, None] + np.abs(rg)[None, :]
    rel = np.abs(got - want) / np.abs(want)
    print('beta %g d %d: worst relative difference %.3e' % (beta, d, rel.max()))
    assert rel.max() <= 1e-12
    # sigmoid(s) is the pair probability, and the pure-head distance is -s
    if beta == 1.0:
        lg = V.literal_logits(q[:, col0:col0 + D], g[:, col0:col0 + D], head)
        assert np.allclose(-got, lg[..., 1] - lg[..., 0], rtol=0, atol=1e-12 * scale.max())


def test_the_error_bound_is_the_documented_formula():
    head = V.make_head(32, seed=1)
    q, g = V.features(3, 5, 96, 32, 32, seed=2)
    w, c = V.fold(head)
    qv, rq, rg = V.row_terms(q, g, 32, w, c, 0.35)
    b = V.error_bound(q, g, 32, w, c, 0.35)
    want = 2 * (96 + 8) * 2.0 ** -24 * (np.abs(qv[1]) @ np.abs(g[4].astype(np.float64)) + abs(rq[1]) + abs(rg[4]))
    assert b.shape == (3, 5) and abs(b[1, 4] - want) <= 1e-15 * want
    b1 = V.error_bound(q, g, 32, w, c, 1.0)                      # beta = 1: the GEMM runs over the slice, K = 32
    qv1, rq1, rg1 = V.row_terms(q, g, 32, w, c, 1.0)
    assert not qv1[:, :32].any() and not qv1[:, 64:].any()
    want1 = 2 * (32 + 8) * 2.0 ** -24 * (np.abs(qv1[0]) @ np.abs(g[0].astype(np.float64)) + abs(rq1[0]) + abs(rg1[0]))
    assert abs(b1[0, 0] - want1) <= 1e-15 * want1


def test_library_exports_the_verify_entry_points():
    import ctypes
    from grl_amd import _lib
    names = ('grl_verify_fold', 'grl_verify_rows', 'grl_verify_finish')
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert n in _lib.exported_symbols() and hasattr(raw, n)
    lib = _lib.load()
    E = _lib.GRL_EINVAL
    # the argument checks come before any HIP call: null pointers, then ranges on fake (never dereferenced) pointers
    import ctypes as C
    eps = C.byref(C.c_double(1e-5))
    assert lib.grl_verify_fold(None, None, None, None, eps, None, None, 64, None, None, None, None) == E
    p = [0x1000 * i for i in range(1, 10)]
    assert lib.grl_verify_fold(p[0], p[1], p[2], p[3], eps, p[4], p[5], 62, p[6], p[7], p[8], None) == E
    assert b'D = 62' in lib.grl_last_error()
    order = ('x', 'ldx', 'n', 'd', 'col0', 'Dv', 'w', 'beta', 'c64', 'r', 'qout', 'ldq', 'full', 'stream')
    good = dict(x=0x10000, ldx=192, n=4, d=192, col0=64, Dv=64, w=0x1000, beta=0.5, c64=None, r=0x2000, qout=None, ldq=0,
                full=0, stream=None)

    def rows(**k):
        a = dict(good, **k)
        a['beta'] = C.byref(C.c_double(a['beta']))
        return lib.grl_verify_rows(*[a[n] for n in order])
    for bad in (dict(x=None), dict(col0=160), dict(col0=-4), dict(col0=62), dict(Dv=62), dict(ldx=188), dict(d=190),
                dict(x=0x10004), dict(beta=0.0), dict(beta=1.5), dict(beta=float('nan')), dict(n=0),
                dict(qout=0x40000, ldq=60), dict(qout=0x40000, ldq=64, full=1), dict(qout=0x40004, ldq=64),
                dict(qout=0x10000 + 64, ldq=192, full=1)):
        assert rows(**bad) == E, bad
    assert b'overlaps' in lib.grl_last_error()
    fin = lib.grl_verify_finish
    assert fin(None, 8, 2, 8, 0x1000, 0x2000, 0, None) == E
    for args in ((0x4000, 7, 2, 8, 0x1000, 0x2000, 0), (0x4000, 8, 0, 8, 0x1000, 0x2000, 0),
                 (0x4000, 8, 2, 8, 0x1000, 0x2000, -1), (0x4002, 8, 2, 8, 0x1000, 0x2000, 0)):
        assert fin(*args, None) == E, args


def _siam(input_num=64, class_num=2):
    from grl_amd.reid.models.Siamese import Siamese
    return Siamese(input_num, 16, class_num).eval()


def test_verify_metric_refuses_what_it_cannot_rank(monkeypatch):
    from grl_amd import engine

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    monkeypatch.setattr(engine, '_call', no_device)
    siam = _siam()
    vm = engine.verify_metric(siam, 64, 0.35)
    assert (vm.col0, vm.Dv, vm.beta, vm.full) == (64, 64, 0.35, True) and not engine.verify_metric(siam, 0).full
    with pytest.raises(ValueError, match='class_num = 3'):
        engine.verify_metric(_siam(class_num=3), 0)
    for beta in (0.0, -0.1, 1.0001, float('nan'), '0.5', None, True):
        with pytest.raises(ValueError, match='beta'):
            engine.verify_metric(siam, 0, beta)
    for col0 in (-4, 2, 1.0, None):
        with pytest.raises(ValueError, match='col0'):
            engine.verify_metric(siam, col0)
    with pytest.raises(ValueError, match='width 48'):
        engine.verify_metric(_siam(input_num=48), 0)
    with pytest.raises(RuntimeError, match='eval'):
        engine.verify_metric(_siam().train(), 0)
    # shapes that only the rows decide: the slice must fit, the GEMM must take K
    qf, gf = torch.zeros(3, 96), torch.zeros(5, 96)
    with pytest.raises(ValueError, match=r'\[64, 128\) does not fit rows of 96'):
        engine.verify_dist(qf, gf, vm)
    with pytest.raises(ValueError, match='rows of 80 columns'):
        engine.search(torch.zeros(3, 80), torch.zeros(5, 80), 2, metric=engine.verify_metric(siam, 0, 0.5))
    with pytest.raises(ValueError, match='rows of 66 columns'):
        engine.verify_dist(torch.zeros(3, 66), torch.zeros(5, 66), engine.verify_metric(siam, 0))
    with pytest.raises(ValueError, match='verify_metric'):
        engine.verify_dist(qf, gf, 'cosine')
    # re-ranking and the feature expansion keep to their own metrics
    with pytest.raises(ValueError, match='metric must be'):
        engine.expand_features(qf, gf, 2, metric=vm)
    import inspect
    for fn in (engine.rerank_search, engine.rerank_metrics_streaming):
        assert 'metric' not in inspect.signature(fn).parameters


def test_verify_has_no_host_path():
    from grl_amd import engine
    from grl_amd._lib import GrlHipError
    vm = engine.verify_metric(_siam(), 64)
    with pytest.raises(GrlHipError):
        engine.verify_dist(torch.zeros(3, 192), torch.zeros(5, 192), vm)


def test_verify_prob_is_the_sigmoid_of_the_logit():
    from grl_amd import engine
    d = np.array([[-3.0, 0.0, 2.5, np.inf]])
    want = 1.0 / (1.0 + np.exp(np.array([[-3.0, 0.0, 2.5]])))
    got = engine.verify_prob(d)
    assert np.allclose(got[:, :3], want, rtol=1e-15, atol=0) and got[0, 3] == 0.0 and got[0, 1] == 0.5
    t = engine.verify_prob(torch.tensor(d, dtype=torch.float32))
    assert torch.is_tensor(t) and np.allclose(t.numpy()[:, :3], want, rtol=1e-6) and t[0, 3] == 0
    assert np.allclose(engine.verify_prob([[0.0, -1.0]]), [[0.5, 1 / (1 + np.exp(-1.0))]])


def test_the_metric_knob_parses():
    from grl_amd.reid.evaluator.attevaluator import parse_metric_knob as parse
    name = 'GRL_EVAL_METRIC'
    for off in (None, '', '  ', 'cosine', ' cosine '):
        assert parse(name, off) is None
    assert parse(name, 'verify') == ('verify', 1.0)
    assert parse(name, 'verify,0.35') == ('verify', 0.35)
    assert parse(name, ' verify , 1 ') == ('verify', 1.0)
    assert parse(name, 'verify,1e-3') == ('verify', 1e-3)
    for bad in ('euclidean', 'Verify', 'verify,', 'verify,x', 'verify,0', 'verify,-0.5', 'verify,1.5', 'verify,nan',
                'verify,inf', 'verify,0.5,1', 'cosine,0.5', '0.5', 'verify;0.5'):
        with pytest.raises(ValueError, match=name):
            parse(name, bad)


def test_the_metric_knob_stops_evaluate_before_any_extraction(monkeypatch):
    from grl_amd.reid.evaluator import ATTEvaluator
    ev = ATTEvaluator(None, None, only_eval=False)

    class NoLoader(object):
        def __iter__(self):
            raise AssertionError('a loader was touched')
        __len__ = __iter__

    def no_extract(loader):
        raise AssertionError('features were extracted')
    monkeypatch.setattr(ev, 'extract_feature', no_extract)
    for name in ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC'):
        monkeypatch.delenv(name, raising=False)
    for value in ('verify', 'verify,0.35'):
        monkeypatch.setenv('GRL_EVAL_METRIC', value)
        with pytest.raises(ValueError, match='GRL_EVAL_METRIC=%s cannot re-rank' % value):
            ev.evaluate(None, None, NoLoader(), NoLoader(), '', 0, 1)
        monkeypatch.setenv('GRL_EVAL_RERANK', 'stream')
        with pytest.raises(ValueError, match='cannot re-rank'):
            ev.evaluate(None, None, NoLoader(), NoLoader(), '', 0, 1)
        monkeypatch.delenv('GRL_EVAL_RERANK')
    monkeypatch.setenv('GRL_EVAL_METRIC', 'verify,2')
    with pytest.raises(ValueError, match='GRL_EVAL_METRIC'):
        ev.evaluate(None, None, NoLoader(), NoLoader(), '', 0, 0)
    # 'cosine' and rerank=0 with the knob set get as far as the extraction
    monkeypatch.setenv('GRL_EVAL_METRIC', 'cosine')
    with pytest.raises(AssertionError, match='extracted'):
        ev.evaluate(None, None, NoLoader(), NoLoader(), '', 0, 1)
    monkeypatch.setenv('GRL_EVAL_METRIC', 'verify')
    with pytest.raises(AssertionError, match='extracted'):
        ev.evaluate(None, None, NoLoader(), NoLoader(), '', 0, 0)
