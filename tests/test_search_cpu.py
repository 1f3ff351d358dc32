"""The column-block search / ranking algorithm (tests/search_ref.py, the model of grl_amd/csrc/search.hip)
against the whole-matrix definitions: np.argsort(kind='stable') and eva_functions.evaluate.  Distances are
the fma-chain model of the device GEMM (oracle.ref_c.chain_gemm)."""
import contextlib
import io

import numpy as np
import pytest

import search_ref as S
from grl_amd.reid.evaluator.eva_functions import evaluate
from grl_amd.synthetic import synth_eval_features


def _negdot(qf, gf):
    from oracle.ref_c import chain_gemm
    return chain_gemm(np.asarray(qf), np.asarray(gf), mode=1)


@pytest.fixture(scope='module')
def case():
    qf, gf, qp, qc, gp, gc = synth_eval_features(40, 400, seed=1, n_ids=24, noise=7.0)
    return _negdot(qf, gf), qp, qc, gp, gc


def _tied_case():
    """Duplicated gallery rows (exact ties that straddle block boundaries), zero rows (-0 / +0 distances), a
    query whose pid is absent and one whose same-pid entries are all junk."""
    qf, gf, qp, qc, gp, gc = synth_eval_features(12, 150, seed=4, dim=96, n_ids=8, noise=3.0)
    gf, qf = gf.numpy(), qf.numpy()
    rep = np.arange(0, 150, 3)
    gf = np.concatenate([gf, gf[rep]], 0)
    gp, gc = np.append(gp, gp[rep]), np.append(gc, gc[rep])
    gf[20:25] = 0.0
    qf = np.concatenate([qf, np.zeros((1, 96), np.float32), -qf[:1]], 0)
    qp = np.append(qp, [gp[20], 1000]); qc = np.append(qc, [gc[20], 0])
    junk = gp == gp[20]
    gc[junk] = qc[-2]                                     # the zero query's pid: junk only
    return _negdot(qf, gf), qp, qc, gp, gc


def _ref_per_query(D, qp, qc, gp, gc):
    order = np.argsort(D, axis=1, kind='stable')
    first, nhit, ap = [], [], []
    for q in range(D.shape[0]):
        o = order[q]
        same = gp[o] == qp[q]
        keep = ~(same & (gc[o] == qc[q]))
        hits = same[keep]
        pos = np.flatnonzero(hits)
        nhit.append(pos.size)
        first.append(pos[0] if pos.size else -1)
        ap.append(np.mean((np.arange(pos.size) + 1) / (pos + 1.0)) if pos.size else 0.0)
    return np.array(first), np.array(nhit), np.array(ap), order


def _check(D, qp, qc, gp, gc, width, k=100):
    first, nhit, ap = S.rank_blocks(D, qp, gp, qc, gc, width)
    f_ref, n_ref, ap_ref, order = _ref_per_query(D, qp, qc, gp, gc)
    assert np.array_equal(first, f_ref) and np.array_equal(nhit, n_ref), width
    assert np.all(np.abs(ap - ap_ref) <= 1e-12 * np.abs(ap_ref)), width
    cmc, mAP = S.metrics(first, nhit, ap, D.shape[1])
    with contextlib.redirect_stdout(io.StringIO()):
        cmc_ref, map_ref = evaluate(D, qp, gp, qc, gc, indices=order)
    assert np.array_equal(cmc, cmc_ref) and abs(mAP - map_ref) <= 1e-12
    dist, idx = S.topk_blocks(D, k, width)
    kk = min(k, D.shape[1])
    assert np.array_equal(idx[:, :kk], order[:, :kk])
    assert np.array_equal(dist[:, :kk].view(np.uint32), np.take_along_axis(D, order[:, :kk], 1).view(np.uint32))
    assert (idx[:, kk:] == -1).all() and np.isinf(dist[:, kk:]).all()


@pytest.mark.parametrize('width', [1, 7, 64, 400, 4096])
def test_blocks_match_the_whole_matrix(case, width):
    _check(*case, width=width)


@pytest.mark.parametrize('width', [1, 7, 64, 200])
def test_ties_signed_zero_and_unmatched_queries(width):
    D, qp, qc, gp, gc = _tied_case()
    assert (D.view(np.uint32) == 0x80000000).any() or (D == 0).any()      # zero rows give signed zeros
    _check(D, qp, qc, gp, gc, width, k=30)
    first, nhit, _ = S.rank_blocks(D, qp, gp, qc, gc, width)
    assert nhit[-1] == 0 and nhit[-2] == 0 and first[-1] == -1          # absent pid, junk-only pid: skipped


def test_gallery_smaller_than_k(case):
    D, qp, qc, gp, gc = case
    _check(D[:, :37], qp, qc, gp[:37], gc[:37], 7, k=64)


def test_nan_and_signed_zero_keys_follow_the_argsort_order():
    D = np.array([[0.0, -0.0, np.nan, 1.0, -np.inf, np.inf, -0.0, np.float32('nan')]], np.float32)
    D[0, 7] = np.frombuffer(np.uint32(0xffc00001).tobytes(), np.float32)[0]     # another NaN payload
    order = np.argsort(D, axis=1, kind='stable')
    for w in (1, 3, 8):
        dist, idx = S.topk_blocks(D, 8, w)
        assert np.array_equal(idx, order)
        assert np.array_equal(dist.view(np.uint32), np.take_along_axis(D, order, 1).view(np.uint32))
