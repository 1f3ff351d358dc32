"""The float64 model of the hybrid-memory cross entropy (tests/hybrid_ref.py) is right and the host side of self-paced hybrid
training keeps its books -- all shown without a GPU:

* the model's own identities: its dlogits is torch float64 autograd of its own loss; with identity singletons it is the plain
  cross entropy; the planted ties; the fp32 restatement in the kernel's order sits inside the derived bounds;
* the ARG-MAX GAP CONDITION of every case the GPU file compares `correct` on, on the float64 reference alone;
* HybridLabels numbering and tables on hand-made labels, relabel keeps every tracklet;
* the self-paced filter against a brute-force model that builds the n x n set matrices, tau fixed on the state's second use;
* RawVideoDataset(index=True) item layout, jpeg_collate and the batch stages hand the index on;
* every refusal of HybridMemoryLoss.reset, HybridSEQTrainer._parse_data and train_unsupervised(hybrid=True) fires before a
  device call; HybridSEQTrainer hands the criteria the indices in the targets' row order."""
import os
import re

import numpy as np
import pytest
import torch

import hybrid_ref as R
import loss_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------------------------------------
# the model
@pytest.mark.parametrize('name', R.CE_LAYOUTS)
def test_model_dlogits_is_autograd_of_its_own_loss(name):
    n, N = 9, 70
    d = R.in_ce(n, N, name, wide=False)
    ref = R.hybrid_ce(d['logits'], d['ld'], d['targets'], d['cp'], d['cm'], d['ic'], n, N, d['C'])
    x = torch.from_numpy(d['logits'].reshape(n, N).astype(np.float64)).requires_grad_(True)
    size = torch.from_numpy(np.diff(d['cp']).astype(np.float64))
    z = torch.zeros((n, d['C']), dtype=torch.float64).index_add(1, torch.from_numpy(d['ic'].astype(np.int64)), x) / size
    y = torch.from_numpy(d['targets'])
    valid = (y >= 0) & (y < d['C'])
    loss = torch.nn.functional.cross_entropy(z[valid], y[valid], reduction='sum') / int(valid.sum())
    loss.backward()
    assert abs(loss.item() - ref['loss']) < 1e-12 * (1 + abs(ref['loss']))
    assert np.abs(x.grad.numpy() - ref['dz']).max() < 1e-14
    assert not ref['dz'][~ref['valid']].any() and ref['nv'] == n - 2


@pytest.mark.parametrize('N', (1, 3, 70))
def test_identity_singletons_are_the_plain_cross_entropy(N):
    n = 9
    d = R.in_ce(n, N, 'identity', wide=False)
    d['targets'][3] = -100
    ref = R.hybrid_ce(d['logits'], N, d['targets'], d['cp'], d['cm'], d['ic'], n, N, N)
    plain = LR.softmax_ce(d['logits'], N, d['targets'], None, n, N)
    assert abs(ref['loss'] - plain['loss']) < 1e-12 * (1 + abs(plain['loss'])) and ref['correct'] == plain['correct']
    assert np.abs(ref['dz'] - plain['dz_val']).max() < 1e-15


def test_planted_ties_go_to_the_lowest_class():
    d = R.in_ties()
    ref = R.hybrid_ce(d['logits'], d['ld'], d['targets'], d['cp'], d['cm'], d['ic'], 2, R.TIE_COLS, d['C'])
    assert ref['arg'].tolist() == d['want_arg'] and ref['correct'] == d['want_correct']
    assert (ref['z'][0] == 6.0).sum() == 3 and (ref['z'][1] == 9.0).sum() == 3
    got = R.hybrid_ce_f32(d['logits'], d['ld'], d['targets'], d['cp'], d['cm'], d['ic'], 2, R.TIE_COLS, d['C'])
    assert got['correct'] == d['want_correct'] and (got['z'][0] == 6.0).sum() == 3           # exact in fp32 too


def test_layouts_reach_what_the_sweep_is_for():
    for N in R.CE_COLS:
        for name in R.CE_LAYOUTS:
            d = R.in_ce(33, N, name)
            from grl_amd.reid.loss.hybrid_memory import check_partition
            check_partition(d['cp'], d['cm'], d['ic'])
            sizes = np.diff(d['cp'])
            assert d['targets'][1] == -1 and d['targets'][3] == d['C']
            if name == 'identity':
                assert d['C'] == N and np.array_equal(d['cm'], np.arange(N))
            if name == 'one':
                assert d['C'] == 1
            if name == 'random' and N >= 70:
                assert sizes.max() > 1 and (np.diff(d['cm'])[np.diff(d['ic'][d['cm']]) != 0] < 0).any()     # interleaved members
                first = np.array([d['cm'][p] for p in d['cp'][:-1]])
                assert (np.diff(first) < 0).any()                                                         # permuted numbering
            if name == 'big' and N == 1025:
                assert sizes.max() == R.BIG > 256 and (sizes == 1).sum() == N - R.BIG
    assert R.MAX_CLASSES >= 8298


@pytest.mark.parametrize('n,N', R.CE_CASES)
def test_gap_condition_and_the_fp32_restatement_inside_the_bounds(n, N):
    """every sweep case: with the seed `ce_seed` picks, every valid row's gap between its largest class logit and every other
    exceeds GAP_FACTOR x the larger of the two bounds -- no row excluded; and the fp32 restatement is inside b_hybrid_ce"""
    for name in R.CE_LAYOUTS:
        d = R.in_ce(n, N, name, R.ce_seed(n, N, name))
        a = (d['logits'], d['ld'], d['targets'], d['cp'], d['cm'], d['ic'], n, N, d['C'])
        ref = R.hybrid_ce(*a)
        assert R.gap_ok(ref), (n, N, name)
        got = R.hybrid_ce_f32(*a)
        bd = R.b_hybrid_ce(ref, n, N, d['C'])
        what = ('cpu', n, N, name)
        R.check('cpu hybrid_ce z', got['z'], ref['z'], bd['z'], what)
        R.check('cpu hybrid_ce loss', got['loss'], ref['loss'], bd['loss'], what)
        R.check('cpu hybrid_ce dz', got['dz'], ref['dz'], bd['dz'], what)
        assert got['correct'] == ref['correct']
        if name == 'identity':                              # a singleton's class logit is its logit, bit for bit
            assert np.array_equal(got['z'].view(np.uint32), d['logits'].reshape(n, d['ld'])[:, :N].view(np.uint32))


@pytest.mark.parametrize('D', R.LOSS_D)
def test_gap_condition_of_the_loss_cases(D):
    for tag in ('loss', 'second'):
        d = R.in_loss(D, R.loss_seed(D, tag), tag)
        ref = R.loss(d, D)
        assert R.gap_ok(ref['ce'], e_in=R.e_logits(ref, D)), (D, tag)
        assert d['targets'][4] == -1 and d['index'][7] == -1 and ref['ce']['nv'] == R.LOSS_N - 1
        ok = d['index'] >= 0
        assert np.array_equal(d['ic'][d['index'][ok]][d['targets'][ok] >= 0], d['targets'][ok][d['targets'][ok] >= 0])
        assert np.diff(d['cp']).max() > 1 and (np.diff(d['cp']) == 1).any()                     # mixed classes


# ----------------------------------------------------------------------------------------------------------------------
# HybridLabels
HAND = {'all noise': [-1, -1, -1, -1], 'no noise': [1, 0, 1, 2, 0, 2], 'interleaved': [-1, 1, 1, -1, 0, 0, -1, 5, 1]}


@pytest.mark.parametrize('case', sorted(HAND))
def test_hybrid_labels_numbering_tables_and_relabel(case):
    from grl_amd.reid.train.pseudo import PseudoLabels, HybridLabels
    from grl_amd.reid.loss.hybrid_memory import check_partition
    labels = np.array(HAND[case])
    pl = PseudoLabels(labels)
    h = pl.hybrid()
    assert isinstance(h, HybridLabels) and len(h) == labels.size
    want, nc = R.hybrid_numbering(labels)
    assert h.sample_class.tolist() == want.tolist() and h.n_classes == nc == pl.n_clusters + pl.n_noise
    cp, cm, ic = R.tables(want)
    assert h.class_ptr.tolist() == cp.tolist() and h.class_members.tolist() == cm.tolist() and h.inst_class.tolist() == ic.tolist()
    assert h.class_ptr.dtype == h.class_members.dtype == h.inst_class.dtype == np.int32 and h.sample_class.dtype == np.int64
    assert h.class_ptr_dev.dtype == h.class_members_dev.dtype == h.inst_class_dev.dtype == torch.int32
    assert h.sample_class_dev.dtype == torch.int64 and h.sample_class_dev.tolist() == want.tolist()
    assert h.class_members_dev.tolist() == cm.tolist() and h.class_ptr_dev.tolist() == cp.tolist()
    check_partition(h.class_ptr, h.class_members, h.inst_class)
    if case == 'interleaved':
        assert want.tolist() == [3, 1, 1, 4, 0, 0, 5, 2, 1]                                     # clusters 0 .. 2, then the noise in order
    tracklets = [(('p%d' % i,), 900 + i, i % 3) for i in range(labels.size)]
    out = h.relabel(tracklets)
    assert len(out) == labels.size and [t[1] for t in out] == want.tolist()
    assert all(o[0] == t[0] and o[2] == t[2] for o, t in zip(out, tracklets))
    assert len(pl.relabel(tracklets)) == labels.size - pl.n_noise                              # PseudoLabels' own drops the noise
    with pytest.raises(ValueError, match='HybridLabels.relabel: 2 tracklets for %d labels' % labels.size):
        h.relabel(tracklets[:2])


# ----------------------------------------------------------------------------------------------------------------------
# the self-paced filter
def _triples():
    """planted (eps, tight, loose) label triples, n <= 40"""
    base = np.repeat(np.arange(5), 6)                                                   # five clusters of six
    base = np.concatenate((base, [-1, -1, -1]))                                          # and three noise samples
    tight, loose = base.copy(), base.copy()
    tight[[0, 1]] = -1                                                                   # cluster 0 loses two members under tight
    tight[6:9], tight[9:12] = 7, 8                                                       # cluster 1 splits in two
    loose[loose == 3] = 2                                                                # clusters 2 and 3 merge under loose
    loose[30] = 4                                                                        # cluster 4 swallows a noise sample
    yield 'planted', base, tight, loose
    yield 'stable', base, base.copy(), base.copy()
    yield 'all noise', np.full(7, -1), np.full(7, -1), np.zeros(7, np.int64)
    r = R.rng_for('self-paced')
    for k in range(6):
        n = 40
        e = r.randint(-1, 6, n)
        t = np.where(r.uniform(size=n) < 0.25, -1, e + 10 * r.randint(0, 2, n) * (e >= 0))
        l = np.where(e >= 0, e // 2, np.where(r.uniform(size=n) < 0.5, 0, -1))
        yield 'random %d' % k, e, t, l


def test_self_paced_filter_against_the_brute_force_model():
    from grl_amd.reid.train.pseudo import self_paced_filter, SelfPacedState
    seen = set()
    for name, e, t, l in _triples():
        assert e.size <= 40
        st = SelfPacedState()
        assert st.tau is None
        got = self_paced_filter(e, t, l, st)
        want, tau = R.self_paced_brute(e, t, l)
        assert got.dtype == np.int64 and got.tolist() == want.tolist(), name
        assert (st.tau is None and tau is None) or st.tau == tau, name
        assert ((got == e) | (got == -1)).all()                                          # a sample keeps its cluster or becomes noise
        seen.add((bool((got != np.where(e >= 0, e, -1)).any()), name.split()[0]))
    assert (True, 'planted') in seen and (False, 'stable') in seen
    # the planted triple by hand: cluster 1 splits under tight (comp = 3/6: all six tie at the maximum and stay), the clusters 2
    # and 3 merge under loose (indep = 6/12), cluster 4 grows by one (6/7), cluster 0 keeps its four compact members
    _, e, t, l = next(_triples())
    st = SelfPacedState()
    got = self_paced_filter(e, t, l, st)
    assert st.tau == 0.5 and got[:6].tolist() == [-1, -1, 0, 0, 0, 0] and got[6:12].tolist() == [1] * 6
    assert got[12:30].tolist() == [2] * 6 + [3] * 6 + [4] * 6 and got[30:].tolist() == [-1, -1, -1]


def test_tau_stays_fixed_on_the_second_use():
    from grl_amd.reid.train.pseudo import self_paced_filter, SelfPacedState
    triples = list(_triples())
    _, e, t, l = triples[0]
    st = SelfPacedState()
    self_paced_filter(e, t, l, st)
    tau = st.tau
    for name, e2, t2, l2 in triples[3:]:
        got = self_paced_filter(e2, t2, l2, st)
        assert st.tau == tau, name
        assert got.tolist() == R.self_paced_brute(e2, t2, l2, tau=tau)[0].tolist(), name
    assert any(R.self_paced_brute(e2, t2, l2)[1] != tau for _, e2, t2, l2 in triples[3:])   # (a fresh state would have moved it)
    with pytest.raises(ValueError, match='three label vectors of one length'):
        self_paced_filter(e, t[:3], l, st)


def test_self_paced_labels_refuses_before_any_device_call(monkeypatch):
    from grl_amd import engine
    from grl_amd.reid.train import pseudo

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    for name in ('cluster', 'cluster_jaccard'):
        monkeypatch.setattr(engine, name, no_device)
    with pytest.raises(ValueError, match="method must be 'jaccard' or 'cosine' .got 'kmeans'"):
        pseudo.self_paced_labels(None, pseudo.SelfPacedState(), method='kmeans')
    with pytest.raises(ValueError, match='delta must be > 0'):
        pseudo.self_paced_labels(None, pseudo.SelfPacedState(), delta=0.0)


# ----------------------------------------------------------------------------------------------------------------------
# the index's way from the dataset to the criterion
def _frames(tmp_path, n=3):
    from PIL import Image
    paths = []
    for i in range(n):
        p = str(tmp_path / ('f%d.jpg' % i))
        Image.fromarray(np.full((256, 128, 3), 40 * i, np.uint8)).save(p, quality=90)
        paths.append(p)
    return paths


@pytest.mark.parametrize('decode', ('host', 'device'))
def test_raw_video_dataset_index_layout(tmp_path, decode):
    from grl_amd.reid.data import RawVideoDataset
    paths = _frames(tmp_path)
    tracklets = [(paths, 5, 1), (paths[::-1], 6, 2)]
    for augment in (False, True):
        plain = RawVideoDataset(tracklets, seq_len=2, sample='rrs_test', augment=augment, decode=decode)
        withi = RawVideoDataset(tracklets, seq_len=2, sample='rrs_test', augment=augment, decode=decode, index=True)
        for k in range(2):
            a, b = plain[k], withi[k]
            assert len(a) == (4 if augment else 3) and len(b) == len(a) + 1                   # index=False: today's item
            assert torch.is_tensor(b[-1]) and b[-1].dtype == torch.int64 and b[-1].dim() == 0 and int(b[-1]) == k
            assert a[1:3] == b[1:3] == tracklets[k][1:]
            if decode == 'host':
                assert torch.equal(a[0], b[0])
            else:
                assert [bytes(s) for s in a[0]] == [bytes(s) for s in b[0]]
            if augment:
                assert b[3].dtype == torch.int32 and b[3].shape == a[3].shape                 # the block stays where it was
    assert RawVideoDataset(tracklets).index is False


def test_collates_hand_the_index_on(tmp_path):
    from grl_amd.reid.data import RawVideoDataset
    from grl_amd.reid.data.jpeg import jpeg_collate, JpegBatch
    from torch.utils.data import default_collate
    paths = _frames(tmp_path)
    tracklets = [(paths, 5, 1), (paths[::-1], 6, 2), (paths, 7, 0)]
    for augment in (False, True):
        ds = RawVideoDataset(tracklets, seq_len=2, sample='rrs_test', augment=augment, decode='device', index=True)
        batch = jpeg_collate([ds[2], ds[0]])
        assert isinstance(batch[0], JpegBatch) and len(batch) == (5 if augment else 4)
        assert batch[-1].dtype == torch.int64 and batch[-1].tolist() == [2, 0] and batch[1].tolist() == [7, 5]
        ds = RawVideoDataset(tracklets, seq_len=2, sample='rrs_test', augment=augment, index=True)
        batch = default_collate([ds[1], ds[2]])
        assert len(batch) == (5 if augment else 4) and batch[-1].dtype == torch.int64 and batch[-1].tolist() == [1, 2]


def test_pair_sharded_batches_slice_the_index_with_the_batch():
    from grl_amd import dist
    batch = (torch.zeros((4, 2, 1)), torch.tensor([7, 7, 9, 9]), torch.tensor([0, 5, 2, 3]), torch.tensor([11, 12, 13, 14]))
    out = [b for b in dist.PairShardedBatches([batch], rank=1, world=2)]
    assert out[0][3].tolist() == [13, 14] and out[0][1].tolist() == [9, 9]


class _Crit(object):
    def __init__(self, name, log):
        self.name, self.log = name, log

    def __call__(self, feats, targets, index=None):
        self.log.append((self.name, tuple(feats.shape), targets.tolist(), None if index is None else index.tolist()))
        return feats.sum() * 0.0, torch.zeros((feats.size(0), 4))


def _stub_trainer(cls, log, monkeypatch):
    from grl_amd.reid.train import trainer as T
    t = cls.__new__(cls)
    t.device = torch.device('cpu')
    t.model = lambda imgs: (torch.ones((imgs.size(0), imgs.size(1), 8)), torch.ones((imgs.size(0), imgs.size(1), 8)))
    head = lambda x: (torch.zeros((x.size(0) // 2, x.size(0) // 2, 2)), x.mean(1))          # noqa: E731
    t.siamese_model = t.siamese_model_uncorr = head
    t.criterion_corr, t.criterion_uncorr = _Crit('corr', log), _Crit('uncorr', log)
    t.criterion_ver = lambda prob, tp, tg: (torch.zeros(()), None)
    monkeypatch.setattr(T, 'criterion_triplet', lambda f, y: torch.zeros(f.size(0)))
    monkeypatch.setattr(T.SEQTrainer, '_pair_prob', staticmethod(lambda s: s[..., 1]))
    monkeypatch.setattr(T.SEQTrainer, '_top1', staticmethod(lambda o, y: torch.zeros(())))
    return t


BATCH = (torch.zeros((4, 3, 1)), torch.tensor([7, 7, 9, 9]), torch.tensor([0, 5, 2, 3]), torch.tensor([31, 4, 18, 6]))  # B = 4, T = 3


def test_hybrid_seqtrainer_hands_over_the_indices_in_the_targets_row_order(monkeypatch):
    from grl_amd.reid.train import HybridSEQTrainer, SEQTrainer
    log, seen = [], []
    t = _stub_trainer(HybridSEQTrainer, log, monkeypatch)
    base = SEQTrainer._parse_data
    monkeypatch.setattr(SEQTrainer, '_parse_data', lambda self, inputs: seen.append(len(inputs)) or base(self, inputs))
    inputs, targets = t._parse_data(BATCH)
    assert seen == [3] and targets.tolist() == [7, 7, 9, 9]                                  # the base never sees the index
    t._forward(inputs, targets, 0, 0)
    by = {(e[0], e[1][0]): e for e in log}
    assert by[('corr', 12)][3] == [31, 31, 31, 4, 4, 4, 18, 18, 18, 6, 6, 6]                 # expanded over T, as targetX
    assert by[('corr', 4)][3] == by[('uncorr', 4)][3] == [31, 18, 4, 6]                      # probe-then-gallery, as target
    assert by[('corr', 4)][2] == [7, 9, 7, 9]


def test_hybrid_seqtrainer_refuses_a_batch_without_its_index(monkeypatch):
    from grl_amd.reid.train import HybridSEQTrainer, SEQTrainer
    t = _stub_trainer(HybridSEQTrainer, [], monkeypatch)
    monkeypatch.setattr(SEQTrainer, '_parse_data', lambda self, inputs: pytest.fail('the base was reached'))
    for bad in (BATCH[:3], BATCH[:3] + (BATCH[3].int(),), BATCH[:3] + (BATCH[3][:3],), BATCH[:3] + (BATCH[3].view(2, 2),),
                BATCH[:3] + ([31, 4, 18, 6],), BATCH[:3] + (torch.zeros((4, 6), dtype=torch.int32),)):
        with pytest.raises(ValueError, match=r'RawVideoDataset\(index=True\)'):
            t._parse_data(bad)


def test_refusals_fire_before_any_device_call(monkeypatch):
    from grl_amd import engine
    from grl_amd.reid.loss import HybridMemoryLoss, ClusterMemoryLoss
    from grl_amd.reid.loss import memory
    from grl_amd.reid.train import pseudo, SEQTrainer, HybridSEQTrainer

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    for name in ('_call', 'gemm', 'cluster_centroids', 'cluster_jaccard', 'cluster'):
        monkeypatch.setattr(engine, name, no_device)
    monkeypatch.setattr(memory, '_call', no_device)
    with pytest.raises(ValueError, match='temp must be > 0'):
        HybridMemoryLoss(16, temp=0.0)
    crit = HybridMemoryLoss(16)
    assert (crit.temp, crit.momentum, crit.num_instances, crit.num_classes) == (0.05, 0.2, 1, 1)
    assert {'memory', 'class_ptr', 'class_members', 'inst_class'} <= set(crit.state_dict())
    i32 = lambda *a: torch.tensor(a, dtype=torch.int32)                                      # noqa: E731
    f = torch.zeros((3, 16))
    cp, cm, ic = i32(0, 1, 3), i32(1, 0, 2), i32(1, 0, 1)                                    # classes {1}, {0, 2}
    for args, pattern in (((f.double(), cp, cm, ic), 'memory must be a float32 tensor .got torch.float64'),
                          ((np.zeros((3, 16), np.float32), cp, cm, ic), 'memory must be a float32 tensor .got ndarray'),
                          ((torch.zeros((3, 20)), cp, cm, ic), r'memory must be \[N >= 1, num_features = 16\] .got \(3, 20\)'),
                          ((torch.zeros((0, 16)), cp, cm[:0], ic[:0]), r'memory must be \[N >= 1, num_features = 16\]'),
                          ((f, cp.long(), cm, ic), 'class_ptr must be an int32 tensor .got torch.int64'),
                          ((f, cp, [1, 0, 2], ic), 'class_members must be an int32 tensor .got list'),
                          ((f, cp, cm, ic.view(3, 1)), r'inst_class must be 1-d .got \(3, 1\)'),
                          ((f, cp, cm[:2], ic), 'for 3 memory rows class_members and inst_class must be .3. and class_ptr'),
                          ((f, cp, cm, ic[:2]), 'for 3 memory rows class_members and inst_class must be .3. and class_ptr'),
                          ((f, i32(0, 1, 2, 3, 3), cm, ic), 'for 3 memory rows class_members and inst_class must be .3. and class_ptr'),
                          ((f, i32(0), cm, ic), 'for 3 memory rows class_members and inst_class must be .3. and class_ptr'),
                          ((f, i32(0, 0, 3), cm, ic), 'class_ptr must rise from 0 to N = 3 in steps >= 1'),
                          ((f, i32(1, 2, 3), cm, ic), 'class_ptr must rise from 0 to N = 3'),
                          ((f, i32(0, 1, 2), cm, ic), 'class_ptr must rise from 0 to N = 3'),
                          ((f, cp, i32(1, 0, 0), ic), 'class_members must hold every index 0 .. 2 exactly once'),
                          ((f, cp, i32(1, 0, 3), ic), 'class_members must hold every index 0 .. 2 exactly once'),
                          ((f, cp, i32(1, 2, 0), ic), "a class's members must be listed in ascending index"),
                          ((f, cp, cm, i32(1, 0, 0)), 'inst_class is not the inverse'),
                          ((f, cp, cm, i32(1, 0, 2)), 'inst_class is not the inverse'),
                          ((f, cp, cm, ic), 'memory must be on a HIP device .got cpu')):
        with pytest.raises(ValueError, match='HybridMemoryLoss.reset: (hybrid class tables: )?' + pattern):
            crit.reset(*args)
    big = R.MAX_CLASSES + 1
    with pytest.raises(ValueError, match='%d classes exceed GRL_HYBRID_MAX_CLASSES = %d' % (big, R.MAX_CLASSES)):
        crit.reset(torch.zeros((big, 16)), torch.arange(big + 1, dtype=torch.int32), torch.arange(big, dtype=torch.int32),
                   torch.arange(big, dtype=torch.int32))
    assert crit.num_instances == 1                                                           # a refused reset changes nothing
    # train_unsupervised(hybrid=True): before the evaluator is asked for anything

    class Ev(object):
        def extract_feature(self, loader):
            raise AssertionError('features were extracted')

    def trainer(cls, a, b):
        t = cls.__new__(cls)
        t.criterion_corr, t.criterion_uncorr = a, b
        return t
    tracklets = [((i,), i, i % 2) for i in range(4)]
    run = lambda t, **kw: pseudo.train_unsupervised(t, Ev(), None, tracklets, None, None, 1, **dict(dict(hybrid=True), **kw))  # noqa: E731
    with pytest.raises(ValueError, match='hybrid=True needs a HybridSEQTrainer .got SEQTrainer'):
        run(trainer(SEQTrainer, crit, crit))
    with pytest.raises(ValueError, match='hybrid=True needs criterion_corr to be a HybridMemoryLoss .got ClusterMemoryLoss'):
        run(trainer(HybridSEQTrainer, ClusterMemoryLoss(16, 4), crit))
    with pytest.raises(ValueError, match='hybrid=True needs criterion_uncorr to be a HybridMemoryLoss .got ClusterMemoryLoss'):
        run(trainer(HybridSEQTrainer, crit, ClusterMemoryLoss(16, 4)))
    with pytest.raises(ValueError, match='hybrid=True with cameras=True is not built'):
        run(trainer(HybridSEQTrainer, crit, crit), cameras=True)
    with pytest.raises(ValueError, match='self_paced needs hybrid=True'):
        run(trainer(HybridSEQTrainer, crit, crit), hybrid=False, self_paced=dict(delta=0.02))
    with pytest.raises(ValueError, match="self_paced must be a dict with 'delta'"):
        run(trainer(HybridSEQTrainer, crit, crit), self_paced=dict(eps=0.5))


# ----------------------------------------------------------------------------------------------------------------------
# the C ABI
def test_header_binding_and_library_carry_the_entry_point():
    from grl_amd import _lib
    from grl_amd.reid.loss import hybrid_memory
    src = open(os.path.join(ROOT, 'include', 'grl_hip.h')).read()
    assert re.search(r'int\s+grl_hybrid_ce\(const float\* logits, int64_t ld, const int64_t\* targets, const int32_t\* class_ptr,\s+'
                     r'const int32_t\* class_members, const int32_t\* inst_class, int n, int N, int C, float\* loss,\s+'
                     r'float\* correct, float\* dlogits, int64_t ldd, float\* ws, void\* stream\);', src)
    assert int(re.search(r'#define\s+GRL_HYBRID_MAX_CLASSES\s+(\d+)', src).group(1)) == R.MAX_CLASSES == hybrid_memory.MAX_CLASSES
    assert 4 * R.MAX_CLASSES + 4 * (16 + 4) <= 64 * 1024                                     # z next to the reduction scratch
    assert int(re.search(r'#define\s+GRL_ABI_VERSION\s+(\d+)', src).group(1)) == 10 == _lib.ABI_VERSION
    assert 'grl_hybrid_ce' in _lib.exported_symbols()
    assert 'hybrid.hip' in open(os.path.join(ROOT, 'grl_amd', 'csrc', 'Makefile')).read()


def test_host_argument_checks_return_einval_through_the_c_abi():
    from grl_amd import _lib
    lib = _lib.load()
    # fake device pointers (never dereferenced: every call below is refused before the launch)

    def ce(logits=0x1000, ld=8, targets=0x2000, cp=0x3000, cm=0x4000, ic=0x5000, n=2, N=8, C=3, loss=0x6000, dz=0x7000, ldd=8,
           ws=0x8000):
        return lib.grl_hybrid_ce(logits, ld, targets, cp, cm, ic, n, N, C, loss, None, dz, ldd, ws, None)
    big = R.MAX_CLASSES + 1
    for kw in (dict(logits=None), dict(targets=None), dict(cp=None), dict(cm=None), dict(ic=None), dict(loss=None), dict(ws=None),
               dict(n=0), dict(n=-1), dict(N=0), dict(C=0), dict(C=9), dict(ld=7), dict(ldd=7),
               dict(C=big, N=big, ld=big, ldd=big)):
        assert ce(**kw) == _lib.GRL_EINVAL, kw
