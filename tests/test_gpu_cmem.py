"""Unsupervised training on pseudo-labels and a cluster memory, on a real MI355X: the update kernel grl_cmem_update
(grl_amd/csrc/cmem.hip) through the C ABI and ClusterMemoryLoss against the float64 restatement of tests/cmem_ref.py, the
labelling (grl_amd/reid/train/pseudo.py) on planted identities, one SEQTrainer step and one train_unsupervised epoch.

Every comparison with float64 is per element against that element's derived bound (cmem_ref.py) -- never a norm over the
tensor.  Discrete outputs (sel, the top-1 count, the bits of untouched memory rows, 'instance' against OIMLoss) are compared
exactly; the hard selection is compared with the float64 one under the gap condition that test_cmem_cpu.py asserts for every
such case.  The buffers, helpers and conventions are those of test_gpu_head_float64.py / test_gpu_loss_float64.py."""
import contextlib
import copy
import io

import numpy as np
import pytest
import torch

import cmem_ref as R
import loss_ref as LR
from test_gpu_head_float64 import GUARD, _call, _n, _f, _out, _got, _Inputs, _err
from test_gpu_loss_float64 import ISENT, _Ints, _untouched

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    yield
    R.dump_ratios('MI355X cluster memory')


def _sel(n):
    return torch.full((n + GUARD,), ISENT, dtype=torch.int32, device='cuda')


def _got_sel(sel, n):
    torch.cuda.synchronize()
    a = _n(sel)
    assert (a[n:] == ISENT).all(), 'written past the end of sel'
    return a[:n]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


NAME = ('hard', 'mean')


# ----------------------------------------------------------------------------------------------------------------------
# the kernel
@pytest.mark.parametrize('n,D', R.UPD_CASES)
def test_cmem_update(n, D):
    """grl_cmem_update, both modes x K x label pattern x momentum: sel EQUAL to the reference's selection, the written rows
    inside b_cmem_update, every other row bit-unchanged, and a second launch from the same state gives the same bits."""
    for K in R.UPD_K:
        for pattern in R.UPD_PATTERNS:
            d = R.in_update(n, D, K, pattern)
            t, lab = _Inputs(x=d['x']), _Ints(d['labels'])
            for momentum in R.UPD_MOMENTA:
                for mode in R.MODES:
                    what = (n, D, K, pattern, momentum, NAME[mode])
                    ref = R.cmem_update(d['cent'], d['x'], d['labels'], n, D, K, momentum, mode)
                    if mode == R.HARD:
                        assert R.gap_ok(ref, D), what                       # (test_cmem_cpu asserts it too)
                    runs = []
                    for _ in range(2):
                        cent, sel = _out(K * D, d['cent']), _sel(n)
                        _call('grl_cmem_update', cent, t['x'], lab.t, n, D, K, _f(momentum), mode, sel)
                        runs.append((_got(cent, K * D).reshape(K, D).copy(), _got_sel(sel, n).copy()))
                    (got, gsel), (got2, gsel2) = runs
                    assert np.array_equal(_bits(got), _bits(got2)) and np.array_equal(gsel, gsel2), what
                    assert np.array_equal(gsel, ref['sel']), what
                    bd = R.b_cmem_update(ref, D, momentum, mode)
                    for k in range(K):
                        if k in bd:
                            R.check('cmem_update %s' % NAME[mode], got[k], ref['cent'][k], bd[k], what + (k,))
                        else:
                            assert np.array_equal(_bits(got[k]), _bits(d['cent'][k])), 'row %d was written %r' % (k, what)
            t.unchanged(); lab.unchanged()


@pytest.mark.parametrize('D', R.TIE_D)
def test_cmem_update_first_index_wins_ties_and_sel_may_be_null(D):
    """duplicated rows: the least similar member occurs twice with the same bits, the first is selected; with sel = NULL the
    memory comes out the same bits and nothing else is written"""
    d = R.in_tie(D)
    t, lab = _Inputs(x=d['x']), _Ints(d['labels'])
    ref = R.cmem_update(d['cent'], d['x'], d['labels'], 7, D, 3, 0.2, R.HARD)
    assert ref['sel'].tolist() == [0, 0, 1, 1, 0, 0, 0]
    cent, sel = _out(3 * D, d['cent']), _sel(7)
    _call('grl_cmem_update', cent, t['x'], lab.t, 7, D, 3, _f(0.2), R.HARD, sel)
    assert _got_sel(sel, 7).tolist() == ref['sel'].tolist()
    got = _got(cent, 3 * D).reshape(3, D).copy()
    bd = R.b_cmem_update(ref, D, 0.2, R.HARD)
    for k in (0, 1):
        R.check('cmem_update hard', got[k], ref['cent'][k], bd[k], ('tie', D, k))
    assert np.array_equal(_bits(got[2]), _bits(d['cent'][2]))
    for mode in R.MODES:
        a, b, sel = _out(3 * D, d['cent']), _out(3 * D, d['cent']), _sel(7)
        _call('grl_cmem_update', a, t['x'], lab.t, 7, D, 3, _f(0.2), mode, sel)
        _call('grl_cmem_update', b, t['x'], lab.t, 7, D, 3, _f(0.2), mode, None)
        assert np.array_equal(_bits(_got(a, 3 * D)), _bits(_got(b, 3 * D)))
        if mode == R.MEAN:
            assert _got_sel(sel, 7).tolist() == [1] * 7
    t.unchanged(); lab.unchanged()


def test_cmem_update_rejected_arguments_launch_nothing():
    Err = _err()
    x, lab = torch.ones(64, device='cuda'), torch.zeros(8, dtype=torch.int64, device='cuda')
    cent, sel = _out(64), _sel(8)
    for args in ((cent, x, lab, 0, 8, 3, _f(0.2), 0, sel), (cent, x, lab, 2, 6, 3, _f(0.2), 0, sel),
                 (cent, x, lab, 2, 8, 0, _f(0.2), 0, sel), (cent, x, lab, 2, 8, 3, _f(0.2), 2, sel),
                 (None, x, lab, 2, 8, 3, _f(0.2), 0, sel), (cent, None, lab, 2, 8, 3, _f(0.2), 0, sel),
                 (cent, x, None, 2, 8, 3, _f(0.2), 0, sel)):
        with pytest.raises(Err):
            _call('grl_cmem_update', *args)
    _untouched(cent)
    assert (_got_sel(sel, 8) == ISENT).all()


# ----------------------------------------------------------------------------------------------------------------------
# ClusterMemoryLoss
G = 0.75        # the gradient handed to the loss: (G * loss).backward()


def _crit(K, mode, cent):
    from grl_amd.reid.loss import ClusterMemoryLoss
    crit = ClusterMemoryLoss(R.LOSS_D, K, temp=R.LOSS_TEMP, momentum=R.LOSS_MOMENTUM, mode=mode).cuda()
    assert crit.reset(torch.from_numpy(cent).cuda()) is crit and crit.num_clusters == K
    return crit


def _dev(d):
    return torch.from_numpy(d['x']).cuda().requires_grad_(True), torch.from_numpy(d['labels']).cuda()


@pytest.mark.parametrize('K', R.LOSS_K)
def test_instance_mode_is_oim_loss_bit_for_bit(K):
    from grl_amd.reid.loss import OIMLoss
    d = R.in_loss(K)
    crit = _crit(K, 'instance', d['cent'])
    oim = OIMLoss(R.LOSS_D, K, scalar=1 / R.LOSS_TEMP, momentum=R.LOSS_MOMENTUM).cuda()
    oim.lut.copy_(torch.from_numpy(d['cent']))
    out = []
    for c in (crit, oim):
        x, y = _dev(d)
        loss, logits = c(x, y)
        (loss * G).backward()
        out.append((loss.detach(), logits.detach(), x.grad, logits.grl_top1[0], logits.grl_top1[1]))
    torch.cuda.synchronize()
    for a, b in zip(out[0][:4], out[1][:4]):
        assert torch.equal(a, b)
    assert out[0][4] == out[1][4] == R.LOSS_N
    assert torch.equal(crit.centroids, oim.lut)
    assert not torch.equal(crit.centroids.cpu(), torch.from_numpy(d['cent']))


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('K', R.LOSS_K)
def test_loss_and_gradient_against_float64_and_the_memory_after_backward(K, mode):
    """n = 9, D = 256, one row with the noise label -1: logits, loss and dx end to end from the inputs inside b_loss / b_dx; the
    top-1 count EQUAL to the first-arg-max count on the logits the loss returned; the memory after the backward inside
    b_cmem_update of the model, rows of absent labels bit-unchanged."""
    n, D = R.LOSS_N, R.LOSS_D
    d = R.in_loss(K)
    crit = _crit(K, NAME[mode], d['cent'])
    x, y = _dev(d)
    loss, logits = crit(x, y)
    assert not logits.requires_grad and torch.equal(crit.centroids.cpu(), torch.from_numpy(d['cent']))   # forward updates nothing
    (loss * G).backward()
    torch.cuda.synchronize()
    ref = R.loss(d['x'], d['cent'], d['labels'], n, D, K, R.LOSS_TEMP, g=G)
    bd = R.b_loss(ref, n, D, K)
    what = (K, NAME[mode])
    z = _n(logits)
    R.check('loss logits', z, ref['logits'], bd['logits'], what)
    R.check('loss', loss.item(), ref['loss'], bd['loss'], what)
    own = LR.softmax_ce(z.reshape(-1), K, d['labels'], None, n, K)
    assert float(logits.grl_top1[0]) == own['correct'] and logits.grl_top1[1] == n
    dx = _n(x.grad)
    assert not dx[4].any()                                                  # the noise row: weight 0
    R.check('loss dx', dx, ref['dx'], R.b_dx(ref['og'], K, bd['dz'], d['cent']), what)
    upd = R.cmem_update(d['cent'], d['x'], d['labels'], n, D, K, R.LOSS_MOMENTUM, mode)
    if mode == R.HARD:
        assert R.gap_ok(upd, D), what
    bu = R.b_cmem_update(upd, D, R.LOSS_MOMENTUM, mode)
    got = _n(crit.centroids)
    for k in range(K):
        if k in bu:
            R.check('loss memory %s' % NAME[mode], got[k], upd['cent'][k], bu[k], what + (k,))
        else:
            assert np.array_equal(_bits(got[k]), _bits(d['cent'][k])), k


@pytest.mark.parametrize('K', R.LOSS_K)
def test_used_twice_in_one_graph_the_later_update_is_visible_to_the_earlier_backward(K):
    """As the trainer uses one criterion on frame-level and on clip-level features: autograd runs the LATER node first, so
    the earlier node's gradient reads a memory the later node's update has already changed, and stacks its own update on top
    (pinned for OIM by tests/golden/oim.npz).  The memory equals, bit for bit, two grl_cmem_update launches in that order; the
    earlier node's dx is the float64 gradient on the memory after the first of them -- and not the one on the initial memory."""
    n, D = R.LOSS_N, R.LOSS_D
    d1, d2 = R.in_loss(K), R.in_loss(K, tag='second')
    cent0 = d1['cent']
    crit = _crit(K, 'hard', cent0)
    (x1, y1), (x2, y2) = _dev(d1), _dev(d2)
    l1, _ = crit(x1, y1)
    l2, _ = crit(x2, y2)
    (l1 + l2).backward()
    torch.cuda.synchronize()
    c = torch.from_numpy(cent0).cuda()
    _call('grl_cmem_update', c, x2.detach(), y2, n, D, K, _f(R.LOSS_MOMENTUM), R.HARD, None)
    cent1 = _n(c).copy()
    _call('grl_cmem_update', c, x1.detach(), y1, n, D, K, _f(R.LOSS_MOMENTUM), R.HARD, None)
    assert torch.equal(crit.centroids, c)
    assert not np.array_equal(cent1, cent0)
    # the later node: the initial memory, end to end
    r2 = R.loss(d2['x'], cent0, d2['labels'], n, D, K, R.LOSS_TEMP)
    b2 = R.b_loss(r2, n, D, K)
    R.check('twice dx later node', _n(x2.grad), r2['dx'], R.b_dx(r2['og'], K, b2['dz'], cent0), K)
    # the earlier node: dlogits of its forward (on the initial memory), the gradient on the memory after the later update
    r1 = R.loss(d1['x'], cent0, d1['labels'], n, D, K, R.LOSS_TEMP)
    b1 = R.b_loss(r1, n, D, K)
    og = LR.oim_grad(r1['dz'].reshape(-1), K, cent1, [1.0], r1['scalar'], n, K, D)
    R.check('twice dx earlier node', _n(x1.grad), og['dx'], R.b_dx(og, K, b1['dz'], cent1), K)
    stale = np.abs(_n(x1.grad) - r1['dx']) > R.b_dx(r1['og'], K, b1['dz'], cent0)
    assert stale.any(), 'the earlier backward read the memory as it was before the later update'


# ----------------------------------------------------------------------------------------------------------------------
# labelling
@pytest.mark.parametrize('method,kw', [('cosine', R.PLANT_COSINE), ('jaccard', R.PLANT_JACCARD)])
def test_pseudo_labels_recover_the_planted_partition(method, kw):
    from grl_amd import engine
    from grl_amd.reid.train.pseudo import pseudo_labels, PseudoLabels
    x, pids = R.planted()
    xd = torch.from_numpy(x).cuda()
    pl = pseudo_labels(xd, method, **kw)
    assert pl.n_clusters == R.PLANT_IDS and pl.n_noise == R.PLANT_OUTLIERS and pl.method == method
    assert pl.labels.is_cuda and pl.labels.dtype == torch.int64 and np.array_equal(_n(pl.labels), pl.host)
    assert (pl.host[pids >= 100] == -1).all() and np.array_equal(pl.keep, np.flatnonzero(pids < 100))
    assert pl.pair_scores(pids)['ari'] == 1.0
    kept = PseudoLabels(pl.host[pl.keep]).pair_scores(pids[pl.keep])
    assert kept['ari'] == 1.0 and kept['precision'] == 1.0 and kept['recall'] == 1.0 and kept['n'] == 60
    # centroids: engine.cluster_centroids bit for bit, on a column slice too
    want = engine.cluster_centroids(xd, pl.labels, pl.n_clusters, 'unit')[0]
    got = pl.centroids(xd)
    assert tuple(got.shape) == (6, 64) and torch.equal(got, want)
    part = pl.centroids(xd, cols=(16, 48))
    assert tuple(part.shape) == (6, 32)
    assert torch.equal(part, engine.cluster_centroids(xd[:, 16:48].contiguous(), pl.labels, pl.n_clusters, 'unit')[0])
    assert float((part.double().pow(2).sum(1) - 1).abs().max()) < 1e-5
    with pytest.raises(ValueError, match="%s.* found [01] cluster" % method):
        pseudo_labels(xd, method, **dict(kw, min_samples=40))


def test_pseudo_labels_by_hdbscan_and_kmeans():
    from grl_amd.reid.train.pseudo import pseudo_labels
    x, pids = R.planted()
    xd = torch.from_numpy(x).cuda()
    km = pseudo_labels(xd, 'kmeans', k=6)
    assert 2 <= km.n_clusters <= 6 and km.n_noise == 0 and len(km.relabel([((i,), 0, 0) for i in range(63)])) == 63
    assert sorted(set(km.host.tolist())) == list(range(km.n_clusters))
    hd = pseudo_labels(xd, 'hdbscan', min_cluster_size=5)
    assert hd.n_clusters >= 2 and hd.n_noise + hd.keep.size == 63
    print('\nplanted rows: kmeans k=6 ARI %.3f (%d clusters); hdbscan ARI %.3f (%d clusters, %d noise)' % (
        km.pair_scores(pids)['ari'], km.n_clusters, hd.pair_scores(pids)['ari'], hd.n_clusters, hd.n_noise))


# ----------------------------------------------------------------------------------------------------------------------
# the trainer
class _Clips(torch.utils.data.Dataset):
    """tracklets [((seed,), label, cam)] -> (structured synthetic clip [T,3,256,128], label, cam)"""

    def __init__(self, tracklets, T=2):
        self.tracklets, self.T = list(tracklets), T

    def __len__(self):
        return len(self.tracklets)

    def __getitem__(self, i):
        from grl_amd.synthetic import synth_clips_structured
        paths, label, cam = self.tracklets[i]
        return synth_clips_structured(1, self.T, seed=int(paths[0]))[0], label, cam


def _loader(tracklets, batch):
    return torch.utils.data.DataLoader(_Clips(tracklets), batch_size=batch, shuffle=False, drop_last=True)


def _trainer(synth_models, K, mode='hard'):
    from grl_amd.reid.loss import ClusterMemoryLoss, PairLoss
    from grl_amd.reid.train import SEQTrainer
    dev = torch.device('cuda:0')
    cnn, siam, siamv = (copy.deepcopy(m).to(dev) for m in synth_models)
    crit_c, crit_u = ClusterMemoryLoss(2048, K, mode=mode).to(dev), ClusterMemoryLoss(2048, K, mode=mode).to(dev)
    tr = SEQTrainer(cnn, siam, siamv, PairLoss().to(dev), crit_c, crit_u, None)
    params = [p for m in (cnn, siam, siamv) for p in m.parameters()]
    opt = torch.optim.SGD(params, lr=1e-3, momentum=0.9, weight_decay=5e-4, nesterov=True)
    return tr, opt


def test_one_trainer_step_with_cluster_memories(synth_models):
    """B = 4, T = 2, K = 3 with ClusterMemoryLoss as both id criteria: a finite loss, the memory rows of the batch labels
    changed and unit within b_unit_norm2, the row of the absent label bit-identical, and the same bits from a restored state."""
    K = 3
    g = torch.Generator().manual_seed(5)
    seeds = [torch.nn.functional.normalize(torch.randn((K, 2048), generator=g), dim=1) for _ in range(2)]
    tracklets = [((40 + i,), (0, 0, 2, 2)[i], i % 2) for i in range(4)]
    runs = []
    for _ in range(2):
        tr, opt = _trainer(synth_models, K)
        tr.criterion_corr.reset(seeds[0].clone().cuda())
        tr.criterion_uncorr.reset(seeds[1].clone().cuda())
        with contextlib.redirect_stdout(io.StringIO()):
            tr.train(0, _loader(tracklets, 4), opt)
        torch.cuda.synchronize()
        runs.append((tr.meters['loss'].avg, _n(tr.criterion_corr.centroids).copy(), _n(tr.criterion_uncorr.centroids).copy()))
        for k, m in tr.meters.items():
            assert np.isfinite(float(m.avg)), k
    for (mem, seed) in ((runs[0][1], seeds[0]), (runs[0][2], seeds[1])):
        before = seed.numpy()
        assert np.isfinite(mem).all()
        for k in (0, 2):
            assert not np.array_equal(_bits(mem[k]), _bits(before[k])), k
            assert abs((mem[k].astype(np.float64) ** 2).sum() - 1.0) <= R.b_unit_norm2(2048), k
        assert np.array_equal(_bits(mem[1]), _bits(before[1]))
    assert runs[0][0] == runs[1][0]
    assert np.array_equal(_bits(runs[0][1]), _bits(runs[1][1])) and np.array_equal(_bits(runs[0][2]), _bits(runs[1][2]))


def test_train_unsupervised_one_epoch(synth_models, monkeypatch):
    """8 synthetic tracklets whose pids the flow never uses, one epoch, the clustering replaced by a stub with two noise
    rows: the features come from the evaluator in the tracklets' order, both memories are reseeded with the stub's K from
    their column slices (cluster_centroids' bits), and the train loader is built from the kept tracklets alone."""
    from grl_amd import engine
    from grl_amd.reid.evaluator import ATTEvaluator
    from grl_amd.reid.loss import ClusterMemoryLoss
    from grl_amd.reid.train import pseudo
    fixed = [0, 0, 1, 1, -1, 2, 2, -1]
    tracklets = [((60 + i,), 9000 + i, i % 2) for i in range(8)]
    tr, opt = _trainer(synth_models, 5)
    ev = ATTEvaluator(tr.model, tr.siamese_model, only_eval=False)
    seen = {}

    def stub(xf, **kw):
        seen['xf'], seen['kw'] = xf, kw
        clips = torch.stack([_Clips(tracklets)[i][0] for i in range(8)]).cuda()
        assert not tr.model.training and not tr.siamese_model.training     # the evaluator's eval mode, before the epoch trains
        seen['want'] = torch.cat([engine.extract_features(tr.model, tr.siamese_model, clips[i:i + 4]) for i in (0, 4)])
        return pseudo.PseudoLabels(torch.tensor(fixed, device=xf.device), 'stub')
    monkeypatch.setattr(pseudo, 'pseudo_labels', stub)

    def make_eval_loader(t):
        seen['eval'] = list(t)
        return torch.utils.data.DataLoader(_Clips(t), batch_size=4, shuffle=False)

    def make_train_loader(t):
        seen['train'] = list(t)
        seen['mem'] = (tr.criterion_uncorr.centroids.clone(), tr.criterion_corr.centroids.clone())
        return _loader(t, 4)
    epochs = []
    with contextlib.redirect_stdout(io.StringIO()):
        hist = pseudo.train_unsupervised(tr, ev, opt, tracklets, make_eval_loader, make_train_loader, 1,
                                         label_kwargs=dict(method='jaccard', eps=0.4), on_epoch=lambda e, l: epochs.append((e, l)))
    torch.cuda.synchronize()
    assert seen['eval'] == tracklets and seen['kw'] == dict(method='jaccard', eps=0.4)
    xf = seen['xf']
    assert tuple(xf.shape) == (8, 6144)
    assert torch.equal(xf, seen['want'])                                    # eval mode, the tracklets' order
    assert [t[0] for t in seen['train']] == [tracklets[i][0] for i in (0, 1, 2, 3, 5, 6)]
    assert [t[1] for t in seen['train']] == [0, 0, 1, 1, 2, 2] and [t[2] for t in seen['train']] == [0, 1, 0, 1, 1, 0]
    labels = torch.tensor(fixed, device='cuda')
    for crit, mem, cols in ((tr.criterion_uncorr, seen['mem'][0], (0, 2048)), (tr.criterion_corr, seen['mem'][1], (2048, 4096))):
        assert isinstance(crit, ClusterMemoryLoss) and crit.num_clusters == 3 and tuple(crit.centroids.shape) == (3, 2048)
        assert torch.equal(mem, engine.cluster_centroids(xf[:, cols[0]:cols[1]].contiguous(), labels, 3, 'unit')[0])
        assert bool(torch.isfinite(crit.centroids).all())
        changed = (crit.centroids != mem).any(1).tolist()
        assert changed == [True, True, False]                               # one batch of four: the clusters 0 and 1
    assert len(hist) == 1 and epochs == [(0, hist[0])] and hist[0].n_clusters == 3 and hist[0].n_noise == 2
    for k, m in tr.meters.items():
        assert np.isfinite(float(m.avg)), k
