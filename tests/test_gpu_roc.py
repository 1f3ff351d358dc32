"""Pair-level (verification) metrics on the device (engine.pair_roc / rerank_pair_roc / pair_roc_matrix, roc.hip,
DESIGN.md 4r) against the numpy reference of tests/roc_ref.py.  The histograms are integer counts of the bits the
materialised distance matrix holds, so every comparison of histograms is exact."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import roc_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda:0')
NQ, NG, DIM = 37, 301, 64
BITS = (8, 16, 20)
WIDTHS = (None, 64, 301, 7, 300)     # 64: 16-byte rows, ragged last block (45); 301 / None: one unaligned block;
                                     # 7: below one vector load, every col0 unaligned; 300: aligned rows + a block of one


def _ids(nq, ng, seed):
    """9 pids, 3 cameras.  Query 0's pid (8) is not in the gallery; pid 7 is junk-only for its one query (query 1:
    every gallery entry of pid 7 sits on that query's camera)."""
    g = np.random.Generator(np.random.PCG64(seed))
    qp, gp = g.integers(0, 7, nq), g.integers(0, 8, ng)
    qc, gc = g.integers(0, 3, nq), g.integers(0, 3, ng)
    qp[0], qp[1], qc[1] = 8, 7, 2
    gc[gp == 7] = 2
    assert (gp == 7).sum() > 3 and not (gp == 8).any() and (qp == 7).sum() == 1
    return qp, gp, qc, gc


_shape_case = {}


def shape_case():
    """(qf, gf on the device, ids): one NaN gallery row, one all-zero gallery row (zero distances), two gallery
    rows and one query row scaled so that their products overflow to -inf and +inf.  Built once, never modified."""
    if not _shape_case:
        g = np.random.Generator(np.random.PCG64(21))
        q = g.standard_normal((NQ, DIM)).astype(np.float32)
        x = g.standard_normal((NG, DIM)).astype(np.float32)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        x[5, 3] = np.nan
        x[11] = 0.0
        x[17] *= np.float32(3e38)
        x[18] = -x[17]                                           # query 4 against 17 / 18: -inf and +inf, both negatives
        q[4] *= np.float32(2e38)
        _shape_case['v'] = (torch.from_numpy(q).to(DEV), torch.from_numpy(x).to(DEV), _ids(NQ, NG, 22))
    return _shape_case['v']


_matrices = {}


def matrix(metric):
    """The materialised matrix of the shape case (host float32), computed once."""
    from grl_amd import engine
    if metric not in _matrices:
        qf, gf, _ = shape_case()
        fn = engine.cosin_dist if metric == 'cosine' else engine.pairwise_distance_tensor
        _matrices[metric] = fn(qf, gf).cpu().numpy()
    return _matrices[metric]


def _equal(roc, ref, what):
    assert roc.pos.dtype == torch.int64 and roc.neg.dtype == torch.int64 and roc.pos.is_cuda
    assert np.array_equal(roc.pos.cpu().numpy(), ref[0]), what
    assert np.array_equal(roc.neg.cpu().numpy(), ref[1]), what


# ----------------------------------------------------------------------------
# 1. pair_roc = the reference histograms of the materialised matrix, for every bits and block width
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_histograms_equal_the_reference_of_the_materialised_matrix(metric):
    from grl_amd import engine
    qf, gf, (qp, gp, qc, gc) = shape_case()
    D = matrix(metric)
    assert np.isinf(D).any()
    if metric == 'cosine':                                       # (the Euclidean epilogue clamps a NaN to sqrt(1e-12))
        assert np.isnan(D[:, 5]).all() and np.isneginf(D[4]).any() and np.isposinf(D[4]).any()
        assert (D[:, 11] == 0).all() and np.signbit(D[:, 11]).any()      # the zero row: -(+0) = -0, counted as +0
    P, N = R.classes(qp, gp, qc, gc)
    junk = NQ * NG - int(P.sum()) - int(N.sum())
    assert junk > 0 and not P[0].any() and not P[1].any() and P.sum() > 50
    for bits in BITS:
        ref = R.histograms(D, qp, gp, qc, gc, bits)
        for width in WIDTHS:
            roc = engine.pair_roc(qf, gf, qp, gp, qc, gc, metric=metric, bits=bits, block_cols=width)
            _equal(roc, ref, (metric, bits, width))
            assert roc.bits == bits and roc.n_pos + roc.n_neg + junk == NQ * NG
        assert roc.auc == pytest.approx(R.auc(*ref), abs=1e-14) and roc.eer == pytest.approx(R.eer(*ref), abs=1e-14)
        assert roc.auc_slack == pytest.approx(R.auc_slack(*ref), rel=1e-12)
        for f in R.FPR_TARGETS:
            assert roc.tpr_at_fpr(f) == R.tpr_at_fpr(ref[0], ref[1], f)
    fpr, tpr, thr = roc.curve()                                  # (bits = 20)
    assert np.all(np.diff(fpr) >= 0) and np.all(np.diff(tpr) >= 0) and fpr[-1] == 1.0 and tpr[-1] == 1.0
    assert R.bins(thr, 20).tolist() == np.flatnonzero(ref[0] + ref[1]).tolist()
    if metric == 'cosine':                                       # the NaN column sits in the last bin: accepted last
        assert ref[1][-1] > 0 and np.isnan(thr[-1]) and thr[-2] == np.inf
        assert np.all(np.diff(thr[:-1].astype(np.float64)) > 0) and thr[0] == -np.inf    # -inf is its bin's upper edge
    # default bits, default blocks
    _equal(engine.pair_roc(qf, gf, qp, gp, qc, gc, metric=metric), R.histograms(D, qp, gp, qc, gc, 16), metric)


# ----------------------------------------------------------------------------
# 2. contention: nearly every negative in a handful of bins; then the same with half the gallery negated
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('negate_half', [False, True])
def test_histograms_are_exact_when_the_negatives_pile_into_a_few_bins(negate_half):
    from grl_amd import engine
    nq, ng = 256, 2048
    g = np.random.Generator(np.random.PCG64(31))
    base = g.standard_normal(DIM).astype(np.float32)
    q = base + np.float32(1e-3) * g.standard_normal((nq, DIM)).astype(np.float32)
    x = base + np.float32(1e-3) * g.standard_normal((ng, DIM)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    if negate_half:
        x[::2] *= -1
    qp, gp, qc, gc = _ids(nq, ng, 32)
    qf, gf = torch.from_numpy(q).to(DEV), torch.from_numpy(x).to(DEV)
    D = engine.cosin_dist(qf, gf).cpu().numpy()
    for bits in (16, 8, 20):
        ref = R.histograms(D, qp, gp, qc, gc, bits)
        if bits == 16:
            top = np.sort(ref[1])[::-1]
            share = top[:7 * (2 if negate_half else 1)].sum() / ref[1].sum()
            print('negatives in the %d fullest bins: %.4f of %d' % (7 * (2 if negate_half else 1), share, ref[1].sum()))
            assert share > 0.99
        for width in (None, 1000):                               # one block of two column chunks; three blocks
            _equal(engine.pair_roc(qf, gf, qp, gp, qc, gc, bits=bits, block_cols=width), ref, (bits, width))


# ----------------------------------------------------------------------------
# 3. pair_roc_matrix on strided views
# ----------------------------------------------------------------------------
def test_pair_roc_matrix_reads_a_column_slice_of_a_wider_matrix_in_place():
    from grl_amd import engine
    _, _, (qp, gp, qc, gc) = shape_case()
    D = matrix('cosine')
    wide = torch.full((NQ, 320), float('nan'), device=DEV)
    calls = []
    real = engine._call

    def spy(name, *args):
        if name == 'grl_pair_hist_block':
            calls.append(args[:5])
        return real(name, *args)
    engine._call = spy
    try:
        for off in (4, 3, 0):                                    # 16-byte rows with a ragged end; unaligned rows
            wide.fill_(float('nan'))
            wide[:, off:off + NG] = torch.from_numpy(D).to(DEV)
            view = wide[:, off:off + NG]
            assert not view.is_contiguous()
            for bits in (16, 8):
                _equal(engine.pair_roc_matrix(view, qp, gp, qc, gc, bits=bits), R.histograms(D, qp, gp, qc, gc, bits),
                       (off, bits))
            assert calls[-1] == (view.data_ptr(), 320, NQ, 0, NG)        # read in place: no copy was made
        _equal(engine.pair_roc_matrix(torch.from_numpy(D).to(DEV), qp, gp, qc, gc),
               R.histograms(D, qp, gp, qc, gc, 16), 'contiguous')
        t = torch.from_numpy(np.ascontiguousarray(D.T)).to(DEV).t()              # column-major: copied, still right
        _equal(engine.pair_roc_matrix(t, qp, gp, qc, gc), R.histograms(D, qp, gp, qc, gc, 16), 'transposed')
    finally:
        engine._call = real


def test_histograms_are_exact_when_the_bins_are_spread_over_the_whole_key_range():
    """Random bit patterns (NaNs, infinities and denormals among them): nearly every entry of a workgroup asks for a
    table slot that another bin holds, so the counts take the global path."""
    from grl_amd import engine
    nq, ng = 48, 4100
    g = np.random.Generator(np.random.PCG64(51))
    D = g.integers(0, 2 ** 32, (nq, ng), dtype=np.uint32).view(np.float32)
    D[0, :9], D[1, :9] = 0.0, -0.0                               # both zeros share a bin
    qp, gp, qc, gc = _ids(nq, ng, 52)
    dev = torch.from_numpy(D).to(DEV)
    for bits in (20, 16, 8):
        _equal(engine.pair_roc_matrix(dev, qp, gp, qc, gc, bits=bits), R.histograms(D, qp, gp, qc, gc, bits), bits)


# ----------------------------------------------------------------------------
# 4. the verification head's distance
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('beta', [1.0, 0.35])
def test_verify_metric_histograms_equal_the_reference_on_verify_dist(beta):
    from sklearn.metrics import roc_auc_score
    from grl_amd import engine
    import verify_ref as V
    from test_gpu_verify import make_siam
    d, Dv, col0 = 192, 64, 64
    nq, ng = 12, 301
    siam, _ = make_siam(Dv, seed=Dv)
    q, g = V.features(nq, ng, d, col0, Dv, seed=9)
    qf, gf = torch.from_numpy(q).to(DEV), torch.from_numpy(g).to(DEV)
    qp, gp, qc, gc = _ids(nq, ng, 41)
    vm = engine.verify_metric(siam, col0, beta)
    D = engine.verify_dist(qf, gf, vm).cpu().numpy()
    for bits in (16, 12):
        ref = R.histograms(D, qp, gp, qc, gc, bits)
        for width in (None, 37, 128):
            roc = engine.pair_roc(qf, gf, qp, gp, qc, gc, metric=vm, bits=bits, block_cols=width)
            _equal(roc, ref, (beta, bits, width))
    if beta == 1.0:
        roc = engine.pair_roc(qf, gf, qp, gp, qc, gc, metric=vm)
        P, N = R.classes(qp, gp, qc, gc)
        keep = P | N
        exact = roc_auc_score(P[keep], -D[keep].astype(np.float64))
        print('verify beta 1: binned AUC %.9f exact %.9f slack %.3e' % (roc.auc, exact, roc.auc_slack))
        assert roc.auc_slack < 1e-2 and abs(roc.auc - exact) <= roc.auc_slack
        # a threshold of the curve reads as the head's P(same): descending in the distance, inside (0, 1)
        thr = roc.curve()[2][:-1]
        prob = engine.verify_prob(thr)
        assert np.all(np.diff(prob) <= 0) and prob.max() <= 1.0 and prob.min() >= 0.0


# ----------------------------------------------------------------------------
# 5. re-ranked distances
# ----------------------------------------------------------------------------
def test_rerank_pair_roc_equals_pair_roc_matrix_of_the_device_re_ranking():
    from grl_amd import engine
    from grl_amd.reid.evaluator.rerank import re_ranking
    from grl_amd.synthetic import synth_eval_features
    qf, gf, qp, qc, gp, gc = synth_eval_features(16, 120, seed=5, n_ids=10, noise=3.0)
    qf, gf = qf.to(DEV), gf.to(DEV)
    F = re_ranking(engine.cosin_dist(qf, gf), engine.pairwise_distance_tensor(qf, qf),
                   engine.pairwise_distance_tensor(gf, gf))
    for bits in (16, 10):
        want = engine.pair_roc_matrix(F, qp, gp, qc, gc, bits=bits)
        _equal(want, R.histograms(F.cpu().numpy(), qp, gp, qc, gc, bits), bits)
        for width in (None, 32):
            got = engine.rerank_pair_roc(qf, gf, qp, gp, qc, gc, bits=bits, block_cols=width)
            assert torch.equal(got.pos, want.pos) and torch.equal(got.neg, want.neg), (bits, width)
    assert got.auc == want.auc and got.eer == want.eer


# ----------------------------------------------------------------------------
# 6. two gloo ranks on one device shard the gallery rows
# ----------------------------------------------------------------------------
def _shard_case():
    from grl_amd import engine
    qf, gf, (qp, gp, qc, gc) = shape_case()
    out = {}
    for metric in ('cosine', 'euclidean'):
        roc = engine.pair_roc(qf, gf, qp, gp, qc, gc, metric=metric, bits=16, block_cols=37)
        out[metric] = (roc.pos.cpu(), roc.neg.cpu(), roc.auc, roc.eer)
    return out


def _worker(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.save(_shard_case(), os.path.join(outdir, 'rank%d.pt' % rank))
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_return_the_single_process_histograms(tmp_path_factory):
    single = _shard_case()
    outdir = str(tmp_path_factory.mktemp('roc_w2'))
    world, port = 2, 43700 + os.getpid() % 1500
    ctx = mp.get_context('spawn')
    procs = [ctx.Process(target=_worker, args=(r, world, port, outdir)) for r in range(world)]
    for p in procs:
        p.start()
    failed = None
    for r, p in enumerate(procs):                   # every child has its own time limit; the first failure ends the rest
        if failed is None:
            p.join(120)
            if p.is_alive() or p.exitcode != 0:
                failed = 'rank %d: %s' % (r, 'timed out' if p.is_alive() else 'exit code %r' % p.exitcode)
        if failed is not None and p.is_alive():
            p.terminate()
            p.join(10)
    assert failed is None, failed
    for r in range(world):
        res = torch.load(os.path.join(outdir, 'rank%d.pt' % r), weights_only=False)
        for metric, (pos, neg, auc, eer) in single.items():
            assert torch.equal(res[metric][0], pos) and torch.equal(res[metric][1], neg), (metric, r)
            assert res[metric][2:] == (auc, eer), (metric, r)


# ----------------------------------------------------------------------------
# 7. ATTEvaluator.evaluate with GRL_EVAL_ROC
# ----------------------------------------------------------------------------
KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC')
ROC_LINES = ('ROC AUC', 'EER', 'TPR@FPR=1e-3', 'TPR@FPR=1e-2')


def test_attevaluator_reports_the_pair_metrics_on_every_route(synth_models, monkeypatch, tmp_path):
    from grl_amd import engine
    from grl_amd.reid.data import get_data
    from grl_amd.reid.evaluator import ATTEvaluator
    from grl_amd.reid.evaluator.rerank import re_ranking
    cnn, siam, _ = synth_models
    cnn, siam = cnn.to(DEV).eval(), siam.to(DEV).eval()
    _, _, _, q_loader, g_loader = get_data('synthetic', 0, None, 4, 2, 0, 0)
    ev = ATTEvaluator(cnn, siam, only_eval=False)
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    with contextlib.redirect_stdout(io.StringIO()):
        qf, qp, qc = ev.extract_feature(q_loader)
        gf, gp, gc = ev.extract_feature(g_loader)
    gf, gp, gc = torch.cat((qf, gf), 0), np.append(qp, gp), np.append(qc, gc)
    path = str(tmp_path) + os.sep
    roc_file = os.path.join(str(tmp_path), 'roc.json')

    def run(rerank=0):
        if os.path.exists(roc_file):
            os.remove(roc_file)
        with contextlib.redirect_stdout(io.StringIO()) as o:
            r = ev.evaluate(None, None, q_loader, g_loader, path, 0, rerank)
        return r, o.getvalue(), (json.load(open(roc_file)) if os.path.exists(roc_file) else None)

    def without_roc(text):
        return ''.join(l for l in text.splitlines(True) if not l.startswith(ROC_LINES))

    def check(route, want, rerank=0, bits=16, name='cosine'):
        """knob unset: no file, no ROC line; knob set: the same Rank-1, the same other bytes, the figures of ``want``"""
        monkeypatch.delenv('GRL_EVAL_ROC', raising=False)
        r_off, text_off, file_off = run(rerank)
        assert file_off is None and without_roc(text_off) == text_off and 'ROC' not in text_off, route
        monkeypatch.setenv('GRL_EVAL_ROC', '1' if bits == 16 else str(bits))
        r_on, text_on, js = run(rerank)
        assert r_on == r_off and without_roc(text_on) == text_off, route
        lines = [l for l in text_on.splitlines() if l.startswith(ROC_LINES)]
        assert [l.split(':')[0] for l in lines] == list(ROC_LINES), (route, lines)
        at = text_on.splitlines()
        assert at.index(lines[0]) == max(i for i, l in enumerate(at) if l.startswith('Rank-')) + 1      # after the CMC
        assert 'n_pos = %d' % want.n_pos in lines[0] and 'n_neg = %d' % want.n_neg in lines[0]
        assert lines[0].startswith('ROC AUC: {:.2%}'.format(want.auc)) and lines[1] == 'EER: {:.2%}'.format(want.eer)
        assert js['bits'] == bits and js['metric'] == name and (js['n_pos'], js['n_neg']) == (want.n_pos, want.n_neg)
        assert js['auc'] == pytest.approx(want.auc, abs=1e-12) and js['eer'] == pytest.approx(want.eer, abs=1e-12)
        assert js['auc_slack'] == pytest.approx(want.auc_slack, rel=1e-9)
        assert js['tpr_at_fpr'] == {'%g' % f: want.tpr_at_fpr(f) for f in R.FPR_TARGETS}
        fpr, tpr, thr = want.curve()
        assert js['curve']['fpr'] == fpr.tolist() and js['curve']['tpr'] == tpr.tolist()
        assert len(js['curve']['threshold']) == len(thr)
        return text_off

    ids = (qp, gp, qc, gc)
    cos = engine.pair_roc(qf, gf, *ids)
    # the figures are those of the reference on the materialised matrix of the extracted features
    ref = R.histograms(engine.cosin_dist(qf, gf).cpu().numpy(), qp, gp, qc, gc, 16)
    _equal(cos, ref, 'evaluator features')
    def cmc(text):
        return [l for l in text.splitlines() if l.startswith(('Mean AP', 'Rank-'))]
    dense = check('dense', cos)
    monkeypatch.setenv('GRL_EVAL_STREAM', '1')
    assert cmc(check('stream', cos)) == cmc(dense)
    check('stream, 12 bits', engine.pair_roc(qf, gf, *ids, bits=12), bits=12)
    monkeypatch.delenv('GRL_EVAL_STREAM')
    F = re_ranking(engine.cosin_dist(qf, gf), engine.pairwise_distance_tensor(qf, qf),
                   engine.pairwise_distance_tensor(gf, gf))
    rr = engine.pair_roc_matrix(F, *ids)
    in_memory = check('rerank', rr, rerank=1, name='rerank(cosine)')
    monkeypatch.setenv('GRL_EVAL_RERANK', 'stream')
    assert cmc(check('rerank stream', rr, rerank=1, name='rerank(cosine)')) == cmc(in_memory)
    monkeypatch.delenv('GRL_EVAL_RERANK')
    for beta in ('verify', 'verify,0.35'):
        monkeypatch.setenv('GRL_EVAL_METRIC', beta)
        vm = engine.verify_metric(siam, 2048, 1.0 if beta == 'verify' else 0.35)
        want = engine.pair_roc(qf, gf, *ids, metric=vm)
        text = check(beta, want, name=repr(vm))
        monkeypatch.setenv('GRL_EVAL_STREAM', '1')
        assert cmc(check(beta + ' stream', want, name=repr(vm))) == cmc(text)
        monkeypatch.delenv('GRL_EVAL_STREAM')


# ----------------------------------------------------------------------------
# 8. argument errors
# ----------------------------------------------------------------------------
def test_argument_errors():
    from grl_amd import engine
    qf, gf, (qp, gp, qc, gc) = shape_case()
    for bits in (7, 21, 16.0, None):
        with pytest.raises(ValueError, match='bits'):
            engine.pair_roc(qf, gf, qp, gp, qc, gc, bits=bits)
        with pytest.raises(ValueError, match='bits'):
            engine.pair_roc_matrix(torch.zeros((NQ, NG), device=DEV), qp, gp, qc, gc, bits=bits)
        with pytest.raises(ValueError, match='bits'):
            engine.rerank_pair_roc(qf, gf, qp, gp, qc, gc, bits=bits)
    with pytest.raises(ValueError, match='g_pids'):
        engine.pair_roc(qf, gf, qp, gp[:-1], qc, gc)
    with pytest.raises(ValueError, match='q_camids'):
        engine.pair_roc(qf, gf, qp, gp, qc[:-1], gc)
    with pytest.raises(ValueError, match='g_camids'):
        engine.pair_roc_matrix(torch.zeros((NQ, NG), device=DEV), qp, gp, qc, np.append(gc, 0))
    with pytest.raises(ValueError, match='metric'):
        engine.pair_roc(qf, gf, qp, gp, qc, gc, metric='manhattan')
    with pytest.raises(ValueError, match='no positive'):        # every same-pid pair shares its camera: all junk
        engine.pair_roc(qf, gf, qp, gp, np.zeros(NQ), np.zeros(NG))
    with pytest.raises(ValueError, match='no positive'):
        engine.pair_roc(qf, gf, qp + 100, gp, qc, gc)
    with pytest.raises(ValueError, match='no negative'):
        engine.pair_roc(qf, gf, np.zeros(NQ), np.zeros(NG), qc, gc)
    with pytest.raises(ValueError, match='no positive'):
        engine.pair_roc_matrix(torch.zeros((0, NG), device=DEV), qp[:0], gp, qc[:0], gc)     # no rows: nothing counted
