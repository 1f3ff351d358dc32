"""Query expansion / database-side augmentation without a GPU: the host model of grl_expand_rows
(tests/expand_ref.py) against an independent float64 weighted mean and on hand-made lists, the exported symbol, the
argument checks of engine.expand_features that come before any device call, and the evaluator's two knobs.

The device results are held to the model bit for bit (tests/test_gpu_expand.py), so these tests pin the model itself;
only the float64 comparison carries a bound, derived below."""
import numpy as np
import pytest
import torch

import expand_ref as E

F32 = np.float32


def _case(seed, n, nb, d, L, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    x = (g.standard_normal((n, d)) * scale).astype(F32)
    bank = (g.standard_normal((nb, d)) * scale).astype(F32)
    idx = np.stack([g.permutation(nb)[:L] for _ in range(n)]).astype(np.int64)
    dist = -g.random((n, L)).astype(F32)                       # similarities in (0, 1]
    return x, bank, idx, dist


@pytest.mark.parametrize('m', [1, 5, 10, 64])
@pytest.mark.parametrize('alpha', [0, 1, 3, 8])
def test_model_is_the_float64_weighted_mean_within_the_derived_bound(m, alpha):
    """Error budget of the float32 chain with exact inputs, M = the largest |operand| (x, bank): the partial sums are
    at most M * wsum, so the m rounded additions of acc and the one of every product contribute at most
    (m + 1) * 2^-24 * M * wsum, which the division by wsum brings to (m + 1) * 2^-24 * M; the m rounded additions of
    wsum move the quotient (|quotient| <= M) by at most m * 2^-24 * M, and the division rounds once more: together
    below (2 m + 4) * 2^-24 * M <= (m + 4) * 2^-23 * M."""
    x, bank, idx, dist = _case(10 + m + alpha, 12, 300, 257, 70, scale=3.0)
    got = E.expand_rows(x, bank, idx, dist, m, alpha)
    want = E.expand_rows_f64(x, bank, idx, dist, m, alpha)
    assert got.dtype == F32
    bound = (m + 4) * 2.0 ** -23 * max(np.abs(x).max(), np.abs(bank).max())
    err = np.abs(got.astype(np.float64) - want).max()
    print('m = %d alpha = %d: max error %.3e, bound %.3e' % (m, alpha, err, bound))
    assert err <= bound
    assert err > 0 or m == 1                                   # (it is a float32 chain, not float64 in disguise)


def test_the_float64_weights_are_the_powers_they_stand_for():
    """expand_rows_f64 takes the model's float32 weights as the mean's inputs; against float64 powers they are off by
    the alpha - 1 roundings only."""
    g = np.random.Generator(np.random.PCG64(3))
    for alpha in (1, 2, 3, 8):
        for dv in -g.random(200).astype(F32):
            w = float(E.weight(dv, alpha))
            assert abs(w - float(-dv) ** alpha) <= max(alpha - 1, 0) * 2.0 ** -23 * float(-dv) ** alpha
    assert E.weight(F32(-0.5), 1) == F32(0.5) and E.weight(F32(-0.5), 3) == F32(0.125)


def test_alpha_zero_weights_are_exactly_one_and_the_result_is_the_plain_mean():
    for dv in (-0.3, 0.7, 0.0, np.nan, np.inf, -np.inf):
        w = E.weight(F32(dv), 0)
        assert w.dtype == F32 and w.view(np.uint32) == 0x3f800000
    x = np.array([[1.0, 2.0]], F32)
    bank = np.array([[3.0, 6.0], [5.0, 10.0], [100.0, 100.0]], F32)
    idx = np.array([[1, 0, 2]], np.int64)
    dist = np.array([[0.9, np.nan, -1.0]], F32)                # ignored by alpha = 0
    out = E.expand_rows(x, bank, idx, dist, 2, 0)
    assert np.array_equal(out, np.array([[3.0, 6.0]], F32))    # (1 + 5 + 3) / 3, (2 + 10 + 6) / 3


def test_weights_clamp_negative_similarity_and_nan_to_zero():
    assert E.weight(F32(0.25), 1) == 0 and E.weight(F32(0.25), 3) == 0      # positive distance = negative similarity
    assert E.weight(F32(np.nan), 2) == 0 and E.weight(F32(np.inf), 1) == 0
    assert np.isinf(E.weight(F32(-np.inf), 2))
    x = np.array([[1.0, -1.0]], F32)
    bank = np.array([[8.0, 8.0], [4.0, 2.0]], F32)
    idx = np.array([[0, 1]], np.int64)
    out = E.expand_rows(x, bank, idx, np.array([[0.5, -0.5]], F32), 2, 1)
    assert np.array_equal(out, np.array([[3.0 / 1.5, 0.0]], F32))           # bank[0] has weight 0, bank[1] 0.5
    out = E.expand_rows(x, bank, idx, np.array([[-np.inf, -0.5]], F32), 2, 1)
    assert (out.view(np.uint32) == 0x7fc00000).all()                         # inf / inf: the canonical NaN


def test_skip_self_padding_and_short_lists_keep_the_right_entries():
    idx = np.array([5, -1, 2, 9, -1, 2, 7, 0], np.int64)
    assert E.kept(idx, 2, 3, 10) == [0, 2, 3]
    assert E.kept(idx, 2, 3, 10, skip_self=True) == [0, 3, 6]                 # both copies of 2 are the row itself
    assert E.kept(idx, 5, 3, 10, skip_self=True) == [2, 3, 5]                 # self first
    assert E.kept(idx, 0, 8, 10, skip_self=True) == [0, 2, 3, 5, 6]           # self last, short list
    assert E.kept(idx, 4, 8, 10, skip_self=True) == [0, 2, 3, 5, 6, 7]        # self absent
    assert E.kept(idx, 4, 8, 8) == [0, 2, 5, 6, 7]                            # 9 is outside a bank of 8 rows
    assert E.kept(np.array([-1, -1], np.int64), 0, 2, 4) == []
    # values: 4 rows, identity-like bank, so the kept set is readable from the result
    bank = (np.eye(4, dtype=F32) * 4.0)
    lists = np.array([[0, 1, 2, 3], [1, -1, 0, 2], [-1, -1, -1, -1], [3, 3, 3, 0]], np.int64)
    dist = np.full((4, 4), -1.0, F32)
    out = E.expand_rows(bank, bank, lists, dist, 2, 1, skip_self=True)
    want = np.array([[4, 4, 4, 0], [4, 4, 4, 0], [0, 0, 4, 0], [4, 0, 0, 4]], F32)
    want[[0, 1]] /= 3.0
    want[3] /= 2.0
    assert np.array_equal(out, (want).astype(F32))
    assert np.array_equal(E.expand_rows(bank, bank, lists, dist, 2, 1)[0], np.array([8, 4, 0, 0], F32) / F32(3.0))


def test_the_sum_runs_in_list_order():
    """1 + 2^24 - 2^24 in float32 depends on the order: the model adds in list order, product first."""
    x = np.array([[1.0]], F32)
    bank = np.array([[2.0 ** 24], [-2.0 ** 24]], F32)
    dist = np.full((1, 2), -1.0, F32)
    a = E.expand_rows(x, bank, np.array([[0, 1]], np.int64), dist, 2, 0)
    b = E.expand_rows(np.array([[1.5]], F32), bank, np.array([[0, 1]], np.int64), dist, 2, 0)
    assert a[0, 0] == 0.0                                      # (1 + 2^24) rounds to 2^24 (ties to even)
    assert b[0, 0] == F32(2.0) / F32(3.0)                      # (1.5 + 2^24) rounds up to 2^24 + 2


def test_library_exports_grl_expand_rows():
    import ctypes
    from grl_amd import _lib
    assert 'grl_expand_rows' in _lib.exported_symbols()
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, 'grl_expand_rows')
    # the argument checks come before any HIP call: null pointers, then ranges on fake (never dereferenced) pointers
    assert lib.grl_expand_rows(None, 8, None, 8, None, None, 4, 2, 2, 8, 4, 1, 0, 0, None, 8, None) == _lib.GRL_EINVAL
    a = (0x1000, 8, 0x2000, 8, 0x3000, 0x4000, 4, 2, 2, 8, 4)
    for m, alpha, out in ((0, 0, 0x5000), (5, 0, 0x5000), (1, 9, 0x5000), (1, -1, 0x5000)):
        assert lib.grl_expand_rows(*a, m, alpha, 0, out, 8, None) == _lib.GRL_EINVAL, (m, alpha)
    for out in (0x1000, 0x1000 + 15 * 4, 0x2000 + 4, 0x2000 - 4):            # out inside / straddling x or bank
        assert lib.grl_expand_rows(*a, 1, 0, 0, out, 8, None) == _lib.GRL_EINVAL
        assert b'overlaps' in lib.grl_last_error()


def test_expand_features_rejects_bad_arguments_before_the_device(monkeypatch):
    from grl_amd import engine

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    monkeypatch.setattr(engine, '_call', no_device)
    monkeypatch.setattr(engine, 'search', no_device)
    x, bank = torch.zeros(4, 16), torch.zeros(9, 16)           # host tensors: a device call would be refused later
    for m in (0, -1, engine.SEARCH_K_MAX, 2.0, '3', None, True):
        with pytest.raises(ValueError, match='m must be'):
            engine.expand_features(x, bank, m)
    for alpha in (-1, 9, 1.5, '2', None):
        with pytest.raises(ValueError, match='alpha must be'):
            engine.expand_features(x, bank, 3, alpha)
    with pytest.raises(ValueError, match="metric='cosine'"):
        engine.expand_features(x, bank, 3, 1, metric='euclidean')
    with pytest.raises(ValueError, match='metric must be'):
        engine.expand_features(x, bank, 3, 0, metric='l1')
    with pytest.raises(ValueError, match='skip_self'):
        engine.expand_features(x, bank, 3, skip_self=True)
    for fn in (lambda: engine.expand_from_lists(x, bank, torch.zeros(4, 5), torch.zeros(4, 5, dtype=torch.int64), 6),
               lambda: engine.expand_from_lists(x, bank, torch.zeros(4, 5), torch.zeros(4, 5, dtype=torch.int64), 2, 9),
               lambda: engine.expand_from_lists(x, bank, torch.zeros(4, 5), torch.zeros(4, 6, dtype=torch.int64), 2),
               lambda: engine.expand_from_lists(x, bank, torch.zeros(4, 5), torch.zeros(4, 5, dtype=torch.int64), 2,
                                                skip_self=True)):
        with pytest.raises(ValueError):
            fn()
    assert engine.EXPAND_ALPHA_MAX == 8 and engine.SEARCH_K_MAX == 1024
    # accepted arguments get as far as the search
    with pytest.raises(AssertionError, match='device call'):
        engine.expand_features(x, bank, engine.SEARCH_K_MAX - 1, 8)
    with pytest.raises(AssertionError, match='device call'):
        engine.expand_features(x, bank, 1, 0, metric='euclidean')


def test_expand_features_has_no_host_path():
    from grl_amd import engine
    from grl_amd._lib import GrlHipError
    with pytest.raises(GrlHipError):
        engine.expand_features(torch.zeros(4, 16), torch.zeros(9, 16), 3)
    with pytest.raises(GrlHipError):
        engine.expand_from_lists(torch.zeros(4, 16), torch.zeros(9, 16), torch.zeros(4, 5),
                                 torch.zeros(4, 5, dtype=torch.int64), 2)


def test_the_evaluator_knobs_parse():
    from grl_amd.reid.evaluator.attevaluator import parse_expand_knob as parse
    assert parse('GRL_EVAL_QE', None) is None and parse('GRL_EVAL_QE', '') is None and parse('GRL_EVAL_DBA', ' ') is None
    assert parse('GRL_EVAL_QE', '10') == (10, 0)
    assert parse('GRL_EVAL_DBA', '10,3') == (10, 3)
    assert parse('GRL_EVAL_DBA', ' 5 , 8 ') == (5, 8)
    assert parse('GRL_EVAL_QE', '1023,0') == (1023, 0)
    for bad in ('x', '10,', ',3', '10,3,1', '3.5', '10;3', '0', '1024', '-2', '10,9', '10,-1', '1e1'):
        with pytest.raises(ValueError, match='GRL_EVAL_QE'):
            parse('GRL_EVAL_QE', bad)
    with pytest.raises(ValueError, match='GRL_EVAL_DBA'):
        parse('GRL_EVAL_DBA', 'ten')


def test_a_malformed_knob_stops_evaluate_before_any_extraction(monkeypatch):
    from grl_amd.reid.evaluator import ATTEvaluator
    ev = ATTEvaluator(None, None, only_eval=False)

    def no_extract(loader):
        raise AssertionError('features were extracted')
    monkeypatch.setattr(ev, 'extract_feature', no_extract)
    for name in ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA'):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv('GRL_EVAL_DBA', '10,x')
    with pytest.raises(ValueError, match='GRL_EVAL_DBA'):
        ev.evaluate(None, None, [], [], '', 0, 0)
    monkeypatch.delenv('GRL_EVAL_DBA')
    monkeypatch.setenv('GRL_EVAL_QE', '0')
    with pytest.raises(ValueError, match='GRL_EVAL_QE'):
        ev.evaluate(None, None, [], [], '', 0, 0)
