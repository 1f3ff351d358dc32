"""The streaming re-ranking algorithm (tests/rerank_stream_ref.py, the model of grl_amd/csrc/rerank_stream.hip)
against the whole-matrix host re_ranking, and the new C ABI."""
import os
import re

import numpy as np
import pytest

import rerank_stream_ref as R
from grl_amd.reid.evaluator.rerank import re_ranking
from grl_amd.synthetic import synth_eval_features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('grl_rrs_segment_rows', 'grl_rrs_lists', 'grl_rrs_weights', 'grl_rrs_expand', 'grl_rrs_final')


def _dists(qf, gf):
    qf, gf = np.asarray(qf, np.float32), np.asarray(gf, np.float32)

    def euclid(x, y):
        d = (x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2 * x @ y.T
        return np.sqrt(np.maximum(d, 1e-12)).astype(np.float32)
    return (-(qf @ gf.T)).astype(np.float32), euclid(qf, qf), euclid(gf, gf)


def _check(qg, qq, gg, k1, k2, lam, width, block_cols):
    ref = re_ranking(qg, qq, gg, k1=k1, k2=k2, lambda_value=lam)
    got = R.rerank_stream(qg, qq, gg, k1, k2, lam, width=width, block_cols=block_cols)
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert np.abs(got - ref).max() < 2e-6, (k1, k2, lam, np.abs(got - ref).max())
    assert np.array_equal(np.argsort(got, 1, kind='stable'), np.argsort(ref, 1, kind='stable'))


def test_golden_matches_the_reference_output():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'rerank_q16_g120.npz'))
    got = R.rerank_stream(g['dist'], g['qq'], g['gg'], width=9, block_cols=25)
    assert np.abs(got - g['final']).max() < 2e-6
    _check(g['dist'], g['qq'], g['gg'], 20, 6, 0.3, 9, 25)


@pytest.mark.parametrize('k1,k2,lam', [(20, 6, 0.3), (7, 1, 0.5), (5, 3, 0.1), (3, 6, 0.3), (12, 8, 0.2)])
def test_synthetic_matches_the_host_re_ranking(k1, k2, lam):
    """k2 = 1, odd k1 (round-half-even half: 7 -> 4, 5 -> 2), k1 + 1 < k2, several block widths."""
    qf, gf, *_ = synth_eval_features(20, 150, seed=k1, dim=96, n_ids=25, noise=4.0)
    qg, qq, gg = _dists(qf.numpy(), gf.numpy())
    _check(qg, qq, gg, k1, k2, lam, width=13, block_cols=40)


def test_exact_ties(monkeypatch):
    """Duplicated gallery rows: exact ties in D, in the rank lists and in the final distances.  Ties are broken
    by the smaller index (grl_row_argsort's order), so the host restatement runs with a stable argsort here."""
    stable = np.argsort
    monkeypatch.setattr(np, 'argsort', lambda a, axis=-1, kind=None: stable(a, axis=axis, kind='stable'))
    qf, gf, *_ = synth_eval_features(12, 90, seed=8, dim=96, n_ids=15, noise=3.0)
    gf = np.concatenate([gf.numpy(), gf.numpy()[::3]], 0)
    qg, qq, gg = _dists(qf.numpy(), gf)
    _check(qg, qq, gg, 20, 6, 0.3, width=32, block_cols=17)
    _check(qg, qq, gg, 9, 2, 0.4, width=5, block_cols=200)


def test_half_is_round_half_to_even():
    assert [R.half_of(k) for k in range(1, 21)] == [int(np.around(k / 2.)) for k in range(1, 21)]


def test_entry_points_are_declared_and_bound():
    from grl_amd import _lib, engine
    hdr = open(os.path.join(ROOT, 'include', 'grl_hip.h')).read()
    for name in ENTRY_POINTS:
        assert re.search(r'\bint\s+%s\(' % name, hdr), name
        assert name in _lib._SIGNATURES and name in _lib.exported_symbols(), name
    assert int(re.search(r'#define\s+GRL_ABI_VERSION\s+(\d+)', hdr).group(1)) == 10
    assert _lib.ABI_VERSION == 10
    assert callable(engine.rerank_search) and callable(engine.rerank_metrics_streaming)
    src = open(os.path.join(ROOT, 'grl_amd', 'csrc', 'Makefile')).read()
    assert 'rerank_stream.hip' in src
