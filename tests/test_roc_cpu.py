"""Host side of the pair-level (verification) metrics: the key / bin function and the derived figures of
tests/roc_ref.py against known answers and scikit-learn, engine.PairRoc's host arithmetic on the same histograms, the
GRL_EVAL_ROC parser, the entry point's argument checks, and the sharded histogram pass under gloo with the kernel and
the block source replaced by the reference on a host matrix."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import roc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------
# 1. the key
# ----------------------------------------------------------------------------
def test_key_is_monotone_over_a_sorted_sweep_with_zeros_denormals_infinities_and_nans():
    tiny = np.float32(1e-45)                                     # the smallest denormal
    mags = np.array([tiny, 3 * tiny, 1e-39, 1.17549435e-38, 1e-20, 1e-3, 0.5, 1.0, 1.0000001, 7.0, 3e38], np.float32)
    assert np.all(np.diff(mags) > 0)
    sweep = np.concatenate(([-np.inf], -mags[::-1], [-0.0, 0.0], mags, [np.inf])).astype(np.float32)
    k = R.key(sweep).astype(np.int64)
    zero = len(mags) + 1
    assert k[zero] == k[zero + 1] == 0x80000000                  # -0 and +0 share a key
    d = np.diff(k)
    assert np.all(np.delete(d, zero) > 0) and d[zero] == 0       # strictly ascending everywhere else
    nan_pos = np.array([0x7fc00000, 0x7f800001, 0x7fffffff], np.uint32).view(np.float32)
    nan_neg = np.array([0xffc00000, 0xff800001, 0xffffffff], np.uint32).view(np.float32)
    assert np.all(R.key(nan_pos) == 0xffffffff) and np.all(R.key(nan_neg) == 0xffffffff)
    assert k[-1] == 0xff800000 and k[-1] < 0xffffffff            # +inf is below NaN, -inf is the smallest
    assert k[0] == 0x007fffff
    for bits in (8, 16, 20):                                     # the bins inherit the order
        b = R.bins(sweep, bits)
        assert np.all(np.diff(b) >= 0) and b.max() < (1 << bits) and R.bins(nan_neg, bits).min() == (1 << bits) - 1


# ----------------------------------------------------------------------------
# 2. the figures: known answers, scikit-learn
# ----------------------------------------------------------------------------
def _four_bins(pos4, neg4, bits=8):
    pos, neg = np.zeros(1 << bits, np.int64), np.zeros(1 << bits, np.int64)
    for b, p, n in zip((10, 20, 30, 40), pos4, neg4):
        pos[b], neg[b] = p, n
    return pos, neg


# (pos, neg per bin) -> auc, slack, eer, {target: tpr}
#   A: TPR .5 .8 .9 1 / FPR .1 .3 .6 1: crossing between boundaries 1 and 2, FPR + TPR - 1 = -.4 -> .1, t = .8
#   B: TPR .2 .7 .9 1 / FPR 0 .1 .5 1: a bin of positives alone (FPR stays 0: the LAST boundary with FPR <= f counts)
HAND = {
    'A': ((5, 3, 1, 1), (1, 2, 3, 4), 0.79, 0.09, 0.26, {1e-4: 0.0, 1e-3: 0.0, 1e-2: 0.0, 1e-1: 0.5, 0.3: 0.8, 0.59: 0.8}),
    'B': ((2, 5, 2, 1), (0, 1, 4, 5), (2 * 10 + 5 * 9.5 + 2 * 7 + 2.5) / 100, 0.5 * (5 + 8 + 5) / 100,
          0.1 + 0.4 / 3, {1e-4: 0.2, 1e-3: 0.2, 1e-2: 0.2, 1e-1: 0.7, 0.5: 0.9, 1.0: 1.0}),
}


@pytest.mark.parametrize('name', sorted(HAND))
def test_reference_and_engine_figures_on_a_hand_built_four_bin_case(name):
    from grl_amd import engine
    pos4, neg4, auc, slack, eer, tprs = HAND[name]
    pos, neg = _four_bins(pos4, neg4)
    roc = engine.PairRoc(torch.from_numpy(pos), torch.from_numpy(neg), 8)
    assert (roc.n_pos, roc.n_neg) == (10, 10)
    for got in ((R.auc(pos, neg), R.auc_slack(pos, neg), R.eer(pos, neg)), (roc.auc, roc.auc_slack, roc.eer)):
        assert got == pytest.approx((auc, slack, eer), abs=1e-12)
    for f, want in tprs.items():
        assert R.tpr_at_fpr(pos, neg, f) == want and roc.tpr_at_fpr(f) == want, (f, want)
    fpr, tpr, thr = roc.curve()
    assert len(fpr) == 4 and tpr[-1] == 1.0 and fpr[-1] == 1.0 and thr.dtype == np.float32
    # a threshold is its bin's upper edge: the largest float32 of the bin, the next float32 belongs to the next bin
    assert R.bins(thr, 8).tolist() == [10, 20, 30, 40]
    assert R.bins(np.nextafter(thr, np.float32(np.inf)), 8).tolist() == [11, 21, 31, 41]


def test_one_class_missing_is_a_value_error_that_says_which():
    from grl_amd import engine
    pos, neg = _four_bins((1, 1, 1, 1), (0, 0, 0, 0))
    with pytest.raises(ValueError, match='no negative'):
        engine.PairRoc(torch.from_numpy(pos), torch.from_numpy(neg), 8)
    with pytest.raises(ValueError, match='no positive'):
        engine.PairRoc(torch.from_numpy(neg), torch.from_numpy(pos), 8)
    with pytest.raises(ValueError, match='no negative'):
        R.auc(pos, neg)
    with pytest.raises(ValueError, match='no positive'):
        R.eer(neg, pos)


def _scores(nq=60, ng=500, seed=3):
    """Cosine-like distances with overlapping classes, ids with junk, as float32."""
    g = np.random.Generator(np.random.PCG64(seed))
    qp, gp = g.integers(0, 12, nq), g.integers(0, 12, ng)
    qc, gc = g.integers(0, 3, nq), g.integers(0, 3, ng)
    same = qp[:, None] == gp[None, :]
    D = (g.normal(0.0, 0.12, (nq, ng)) - np.where(same, 0.25, 0.0)).astype(np.float32)
    return D, qp, gp, qc, gc


def test_reference_auc_is_within_its_own_slack_of_sklearn_on_the_unquantised_scores():
    from sklearn.metrics import roc_auc_score
    from grl_amd import engine
    D, qp, gp, qc, gc = _scores()
    P, N = R.classes(qp, gp, qc, gc)
    keep = P | N
    assert 0 < (~keep).sum() and P.sum() > 100
    exact = roc_auc_score(P[keep], -D[keep].astype(np.float64))
    assert 0.6 < exact < 0.99                                    # the classes overlap: the order matters
    for bits, cap in ((16, 1e-2), (20, 1e-3), (8, 1.0)):
        pos, neg = R.histograms(D, qp, gp, qc, gc, bits)
        assert pos.sum() == P.sum() and neg.sum() == N.sum()
        slack = R.auc_slack(pos, neg)
        print('bits %d: binned AUC %.9f, exact %.9f, difference %.3e, slack %.3e'
              % (bits, R.auc(pos, neg), exact, abs(R.auc(pos, neg) - exact), slack))
        assert slack < cap                                       # the bound below is not vacuous
        assert abs(R.auc(pos, neg) - exact) <= slack
        roc = engine.PairRoc(torch.from_numpy(pos), torch.from_numpy(neg), bits)
        assert roc.auc == pytest.approx(R.auc(pos, neg), abs=1e-14) and roc.eer == pytest.approx(R.eer(pos, neg), abs=1e-14)
        assert roc.auc_slack == pytest.approx(slack, rel=1e-12)
        for f in R.FPR_TARGETS:
            assert roc.tpr_at_fpr(f) == R.tpr_at_fpr(pos, neg, f)


# ----------------------------------------------------------------------------
# 3. the knob and the entry point's argument checks
# ----------------------------------------------------------------------------
def test_parse_roc_knob():
    from grl_amd.reid.evaluator.attevaluator import parse_roc_knob
    for off in (None, '', '   '):
        assert parse_roc_knob('GRL_EVAL_ROC', off) is None
    assert parse_roc_knob('GRL_EVAL_ROC', '1') == 16
    assert [parse_roc_knob('GRL_EVAL_ROC', v) for v in ('8', ' 12 ', '16', '20')] == [8, 12, 16, 20]
    for bad in ('0', '2', '7', '21', '-16', 'yes', '16,2', '1.0', '16.5', 'nan'):
        with pytest.raises(ValueError, match='GRL_EVAL_ROC'):
            parse_roc_knob('GRL_EVAL_ROC', bad)


def test_bad_knob_is_refused_before_any_feature_is_extracted(monkeypatch):
    from grl_amd.reid.evaluator import ATTEvaluator

    class Never(object):
        def __getattr__(self, name):
            raise AssertionError('touched %s' % name)
    monkeypatch.setenv('GRL_EVAL_ROC', '32')
    for name in ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC'):
        monkeypatch.delenv(name, raising=False)
    with pytest.raises(ValueError, match='GRL_EVAL_ROC'):
        ATTEvaluator(Never(), Never(), False).evaluate(None, None, Never(), Never(), '', 0, 0)


def test_entry_point_checks_its_arguments_before_any_launch():
    from grl_amd import _lib
    lib = _lib.load()
    p = 16                                                       # any non-null address: nothing is dereferenced
    ok = [p, 8, 4, 0, 8, p, p, p, p, 16, p, p, None]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.grl_pair_hist_block(*a)
    for bits in (7, 21, 0, -1):
        assert call(a9=bits) == _lib.GRL_EINVAL and b'bits' in lib.grl_last_error()
    for i in (0, 5, 6, 7, 8, 10, 11):
        assert call(**{'a%d' % i: None}) == _lib.GRL_EINVAL and b'null' in lib.grl_last_error()
    for kw in (dict(a2=-1), dict(a4=0), dict(a4=-3), dict(a3=-1), dict(a1=7)):          # nq, ncols, col0, ld < ncols
        assert call(**kw) == _lib.GRL_EINVAL and b'bad shape' in lib.grl_last_error()
    assert call(a2=0) == 0                                       # no rows: nothing to launch
    assert 'grl_pair_hist_block' in _lib.exported_symbols()


def test_engine_refuses_bad_bits_and_id_lists():
    from grl_amd import engine

    class Blocks(object):
        spans, qf = [], torch.zeros(3, 4)
    ids = (np.zeros(3), np.zeros(5), np.zeros(3), np.zeros(5))
    for bits in (7, 21, 16.0, True, None, '16'):
        with pytest.raises(ValueError, match='bits'):
            engine._roc_blocks(Blocks, 3, 5, *ids, bits=bits, sharded=False)
    with pytest.raises(ValueError, match='g_camids'):
        engine._roc_blocks(Blocks, 3, 5, ids[0], ids[1], ids[2], np.zeros(4), bits=16, sharded=False)
    with pytest.raises(ValueError, match='q_pids'):
        engine._roc_blocks(Blocks, 3, 5, np.zeros(2), ids[1], ids[2], ids[3], bits=16, sharded=False)


# ----------------------------------------------------------------------------
# 4. two gloo ranks: the sharded histograms sum to the single-process ones
# ----------------------------------------------------------------------------
BITS, WIDTH = 12, 37


class _HostBlocks(object):
    """engine's block-source protocol over a host matrix: column blocks of WIDTH inside [lo, hi)."""

    def __init__(self, D, lo, hi):
        self.D, self.qf = D, D
        self.spans = [(c, min(c + WIDTH, hi)) for c in range(lo, hi, WIDTH)]

    def block(self, c0, c1):
        return self.D[:, c0:c1]


def _ref_hist_block(d, c0, ids, bits, pos, neg):
    """grl_pair_hist_block's contract on host tensors, by the reference."""
    qp, qc, gp, gc = (t.numpy() for t in ids)
    n = d.shape[1]
    p, m = R.histograms(d.numpy(), qp, gp[c0:c0 + n], qc, gc[c0:c0 + n], bits)
    pos += torch.from_numpy(p)
    neg += torch.from_numpy(m)


def _worker(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    from grl_amd import engine
    dist.init_process_group('gloo', rank=rank, world_size=world)
    engine._pair_hist_block = _ref_hist_block
    D, qp, gp, qc, gc = _scores(nq=9, ng=301, seed=8)
    lo, hi, sharded = engine._shard(D.shape[1])
    blocks = _HostBlocks(torch.from_numpy(D), lo, hi)
    roc = engine._roc_blocks(blocks, 9, 301, qp, gp, qc, gc, BITS, sharded)
    torch.save(dict(pos=roc.pos, neg=roc.neg, span=(lo, hi), sharded=sharded, blocks=len(blocks.spans), auc=roc.auc),
               os.path.join(outdir, 'rank%d.pt' % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_sum_to_the_single_process_histograms(tmp_path):
    world, port = 2, 41300 + os.getpid() % 1500
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    D, qp, gp, qc, gc = _scores(nq=9, ng=301, seed=8)
    pos, neg = R.histograms(D, qp, gp, qc, gc, BITS)
    spans = []
    for r in range(world):
        out = torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r), weights_only=False)
        assert out['sharded'] and out['blocks'] >= 4
        assert np.array_equal(out['pos'].numpy(), pos) and np.array_equal(out['neg'].numpy(), neg), r
        assert out['auc'] == R.auc(pos, neg) or abs(out['auc'] - R.auc(pos, neg)) < 1e-14
        spans.append(out['span'])
    assert spans == [(0, 151), (151, 301)]                       # each rank counted its own columns only
