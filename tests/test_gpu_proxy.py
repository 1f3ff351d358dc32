"""Camera-aware proxy memory on a real MI355X: the kernel grl_proxy_ce (grl_amd/csrc/proxy.hip) through the C ABI and
ProxyMemoryLoss against the float64 restatement of tests/proxy_ref.py, PseudoLabels.proxies on planted identities, one
CameraSEQTrainer step and two train_unsupervised(cameras=True) epochs.

Every comparison with float64 is per element against that element's derived bound (proxy_ref.py) -- never a norm over the
tensor.  Discrete outputs (own, negsel, correct, the bits of zero rows and of untouched memory rows, 'instance' against
ClusterMemoryLoss) are compared exactly.  On the kernel sweep the model selects on the very fp32 logits the kernel is given:
no gap condition.  Behind the GEMM of ProxyMemoryLoss the selection is compared under the gap condition that test_proxy_cpu.py
asserts for every such case.  The buffers, helpers and conventions are those of test_gpu_head_float64.py / test_gpu_cmem.py."""
import contextlib
import io

import numpy as np
import pytest
import torch

import proxy_ref as R
import cmem_ref as CM
import loss_ref as LR
import loss_bounds as LB
from test_gpu_head_float64 import GUARD, SENT, _call, _n, _f, _out, _got, _Inputs, _err, _window
from test_gpu_loss_float64 import ISENT, _Ints, _untouched
from test_gpu_cmem import _bits, _Clips, _loader

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    yield
    R.dump_ratios('MI355X proxy memory')


def _iout(n, dtype):
    return torch.full((n + GUARD,), ISENT, dtype=dtype, device='cuda')


def _igot(t, n):
    torch.cuda.synchronize()
    a = _n(t)
    assert (a[n:] == ISENT).all(), 'written past the end of an integer output'
    return a[:n]


class _Case(object):
    """the device copies of one input set"""

    def __init__(self, d):
        self.d = d
        self.f = _Inputs(logits=d['logits'])
        self.ints = [_Ints(d['labels']), _Ints(d['cams']), _Ints(d['pcl'], torch.int32), _Ints(d['pcm'], torch.int32)]

    def launch(self, n, P, k, w, dz=True, own=True, negsel=True, correct=True, ws=None):
        d = self.d
        o = dict(loss=_out(1), correct=_out(1), dz=_out(n * d['ldd']), own=_iout(n, torch.int64),
                 negsel=_iout(n * max(k, 1), torch.int32), ws=_out(3 * n) if ws is None else ws)
        _call('grl_proxy_ce', self.f['logits'], d['ld'], self.ints[0].t, self.ints[1].t, self.ints[2].t, self.ints[3].t, n, P, k,
              _f(w[0]), _f(w[1]), o['loss'], o['correct'] if correct else None, o['dz'] if dz else None, d['ldd'],
              o['own'] if own else None, o['negsel'] if negsel else None, o['ws'])
        return o

    def unchanged(self):
        self.f.unchanged()
        for i in self.ints:
            i.unchanged()


def _read(o, n, P, k, ldd):
    dz0 = np.full(n * ldd, SENT, np.float32)
    return dict(loss=_got(o['loss'], 1)[0].copy(), correct=_got(o['correct'], 1)[0].copy(), own=_igot(o['own'], n).copy(),
                dz=_window(_got(o['dz'], n * ldd), n, P, ldd, dz0).copy(),
                negsel=_igot(o['negsel'], n * max(k, 1)).copy(), rows=_got(o['ws'], 3 * n).copy())


def _same(a, b, keys=('loss', 'correct', 'own', 'dz', 'negsel', 'rows')):
    return all(np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                              b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]) for k in keys)


def _check(got, ref, n, P, k, what):
    assert np.array_equal(got['own'], ref['own']), what
    if k > 0:
        assert np.array_equal(got['negsel'].reshape(n, k), ref['negsel']), what
    else:
        assert (got['negsel'] == ISENT).all(), what                         # k_neg = 0: negsel is ignored
    assert got['correct'] == ref['correct'], what
    bd = R.b_proxy_ce(ref, n, P)
    assert not got['dz'][~ref['valid']].view(np.uint32).any(), what         # zero rows: exactly +0
    assert np.array_equal(got['rows'][2 * n:], ref['valid'].astype(np.float32)), what
    R.check('proxy_ce loss', got['loss'], ref['loss'], bd['loss'], what)
    R.check('proxy_ce dz', got['dz'], ref['dz'], bd['dz'], what)
    if ref['nv'] == 0:
        assert got['loss'] == 0.0 and got['correct'] == 0.0 and not got['dz'].any(), what


# ----------------------------------------------------------------------------------------------------------------------
# the kernel
@pytest.mark.parametrize('n,P', R.CE_CASES)
def test_proxy_ce(n, P):
    """grl_proxy_ce over cameras x table pattern x k_neg x weights: own, negsel and correct EQUAL to the model's, loss and every
    dlogits element inside b_proxy_ce, invalid rows exactly zero, nothing written outside the windows, and a second launch gives
    the same bits.  One more launch per table with every label -1: no valid row."""
    for C in R.CE_CAMS:
        for pattern in R.CE_TABLES:
            d = R.in_ce(n, P, C, pattern)
            case = _Case(d)
            for k0 in R.CE_K:
                k = min(k0, P)
                for w in R.CE_WEIGHTS:
                    what = (n, P, C, pattern, k, w)
                    ref = R.proxy_ce(d['logits'], d['ld'], d['labels'], d['cams'], d['pcl'], d['pcm'], n, P, k, *w)
                    a = _read(case.launch(n, P, k, w), n, P, k, d['ldd'])
                    b = _read(case.launch(n, P, k, w), n, P, k, d['ldd'])
                    assert _same(a, b), what
                    _check(a, ref, n, P, k, what)
            case.unchanged()
            none = dict(d, labels=np.full(n, -1, np.int64))
            k = min(3, P)
            got = _read(_Case(none).launch(n, P, k, (1.0, 0.5)), n, P, k, d['ldd'])
            ref = R.proxy_ce(none['logits'], d['ld'], none['labels'], d['cams'], d['pcl'], d['pcm'], n, P, k, 1.0, 0.5)
            assert ref['nv'] == 0 and (got['negsel'] == -1).all()
            _check(got, ref, n, P, k, (n, P, C, pattern, 'no valid row'))


def test_proxy_ce_ties_go_to_the_lowest_indices():
    """duplicated values straddle the cut: five copies for three places, the lowest indices win; a pair wholly inside and one
    wholly outside; +0.0 against -0.0 compare equal"""
    d = R.in_ties()
    case = _Case(d)
    ref = R.proxy_ce(d['logits'], d['ld'], d['labels'], d['cams'], d['pcl'], d['pcm'], 2, R.TIE_P, R.TIE_K, 1.0, 0.5)
    got = _read(case.launch(2, R.TIE_P, R.TIE_K, (1.0, 0.5)), 2, R.TIE_P, R.TIE_K, d['ldd'])
    assert got['negsel'].reshape(2, -1).tolist() == [d['want'], d['want']]
    _check(got, ref, 2, R.TIE_P, R.TIE_K, 'ties')
    case.unchanged()


def test_proxy_ce_optional_outputs_may_be_null():
    """dlogits, own, negsel and correct each NULL in turn: the other outputs come out the same bits, nothing behind a NULL
    pointer's buffer is written"""
    n, P, k, w = 9, 257, 3, (1.0, 0.5)
    d = R.in_ce(n, P, 6, 'mixed')
    case = _Case(d)
    full = _read(case.launch(n, P, k, w), n, P, k, d['ldd'])
    for name in ('dz', 'own', 'negsel', 'correct'):
        o = case.launch(n, P, k, w, **{name: False})
        torch.cuda.synchronize()
        if name in ('dz', 'correct'):
            _untouched(o[name])
        else:
            assert (_n(o[name]) == ISENT).all(), name
        o[name] = case.launch(n, P, k, w)[name]                                  # (so that _read finds a written buffer)
        got = _read(o, n, P, k, d['ldd'])
        assert _same(full, got, [key for key in ('loss', 'correct', 'own', 'dz', 'negsel', 'rows') if key != name]), name
    case.unchanged()


def test_proxy_ce_rejected_arguments_launch_nothing():
    Err = _err()
    n, P, big = 2, 8, R.MAX_P + 1
    z = torch.ones(n * big, device='cuda')
    lab, pc = torch.zeros(n, dtype=torch.int64, device='cuda'), torch.zeros(big, dtype=torch.int32, device='cuda')
    loss, cor, dz, ws = _out(1), _out(1), _out(n * big), _out(3 * n)
    own, neg = _iout(n, torch.int64), _iout(n * P, torch.int32)

    def args(**kw):
        a = dict(z=z, ld=P, lab=lab, cam=lab, pcl=pc, pcm=pc, n=n, P=P, k=3, loss=loss, dz=dz, ldd=P, ws=ws)
        a.update(kw)
        return (a['z'], a['ld'], a['lab'], a['cam'], a['pcl'], a['pcm'], a['n'], a['P'], a['k'], _f(1.0), _f(0.5), a['loss'], cor,
                a['dz'], a['ldd'], own, neg, a['ws'])
    for kw in (dict(n=0), dict(P=0), dict(k=-1), dict(k=P + 1), dict(ld=P - 1), dict(ldd=P - 1), dict(z=None), dict(lab=None),
               dict(cam=None), dict(pcl=None), dict(pcm=None), dict(loss=None), dict(ws=None), dict(P=big, ld=big, ldd=big)):
        with pytest.raises(Err):
            _call('grl_proxy_ce', *args(**kw))
    for t in (loss, cor, dz, ws):
        _untouched(t)
    assert (_igot(own, n) == ISENT).all() and (_igot(neg, n * P) == ISENT).all()
    _call('grl_proxy_ce', *args(P=R.MAX_P, ld=R.MAX_P, ldd=R.MAX_P, k=P))       # the limit itself is served
    torch.cuda.synchronize()
    # equal logits, every proxy the rows' own cluster and camera: both terms are log P
    assert abs(float(_got(loss, 1)[0]) - 1.5 * np.log(R.MAX_P)) < 1e-4


# ----------------------------------------------------------------------------------------------------------------------
# ProxyMemoryLoss
G = 0.75        # the gradient handed to the loss: (G * loss).backward()


def _crit(d, k, mode, w=R.LOSS_W):
    from grl_amd.reid.loss import ProxyMemoryLoss
    crit = ProxyMemoryLoss(R.LOSS_D, temp=R.LOSS_TEMP, momentum=R.LOSS_MOMENTUM, mode=mode, k_neg=k, w_intra=w[0],
                           w_inter=w[1]).cuda()
    assert crit.reset(torch.from_numpy(d['mem']).cuda(), torch.from_numpy(d['pcl']).cuda(), torch.from_numpy(d['pcm']).cuda()) is crit
    assert crit.num_proxies == d['mem'].shape[0]
    return crit


def _dev(d):
    return (torch.from_numpy(d['x']).cuda().requires_grad_(True), torch.from_numpy(d['labels']).cuda(),
            torch.from_numpy(d['cams']).cuda())


def _memory_model(mem, x, own, P, mode):
    """the float64 update of the backward with the proxy id as the label -> (memory, {row: bound})"""
    n, D = R.LOSS_N, R.LOSS_D
    if mode == 'instance':
        upd = LR.oim_update(mem, x, own, n, D, P, CM.m32(R.LOSS_MOMENTUM))
        return upd['lut'], LB.b_oim_update(upd, D, CM.m32(R.LOSS_MOMENTUM))
    m = CM.MODES[('hard', 'mean').index(mode)]
    upd = CM.cmem_update(mem, x, own, n, D, P, R.LOSS_MOMENTUM, m)
    if m == CM.HARD:
        assert CM.gap_ok(upd, D)
    return upd['cent'], CM.b_cmem_update(upd, D, R.LOSS_MOMENTUM, m)


@pytest.mark.parametrize('P,k,mode', R.LOSS_CASES)
def test_loss_gradient_and_memory_against_float64(P, k, mode):
    """n = 9, D = 256, one noise row and one row without a proxy: logits, loss and dx end to end from the inputs inside b_loss /
    b_dx, the selection being the float64 one (gap condition); the top-1 count EQUAL to the count on the logits the loss
    returned; the memory after the backward inside its bound, rows of absent proxies bit-unchanged."""
    n, D = R.LOSS_N, R.LOSS_D
    d = R.in_loss(P, k, R.loss_seed(P, k))
    crit = _crit(d, k, mode)
    x, y, cam = _dev(d)
    loss, logits = crit(x, y, cam)
    assert not logits.requires_grad and torch.equal(crit.centroids.cpu(), torch.from_numpy(d['mem']))     # forward updates nothing
    (loss * G).backward()
    torch.cuda.synchronize()
    ref = R.loss(d, P, k, R.LOSS_W, g=G)
    assert R.gap_ok(ref, D)                                                  # (test_proxy_cpu asserts it too)
    bd = R.b_loss(ref, n, D, P)
    what = (P, k, mode)
    z = _n(logits)
    R.check('loss logits', z, ref['logits'], bd['logits'], what)
    R.check('loss', loss.item(), ref['loss'], bd['loss'], what)
    on_device = R.proxy_ce(z.reshape(-1), P, d['labels'], d['cams'], d['pcl'], d['pcm'], n, P, min(k, P), *R.LOSS_W)
    assert float(logits.grl_top1[0]) == on_device['correct'] and logits.grl_top1[1] == n
    assert np.array_equal(on_device['negsel'], ref['ce']['negsel']), what    # the fp32 selection is the float64 one
    dx = _n(x.grad)
    assert not dx[4].any() and not dx[7].any()                               # the noise row and the row without a proxy
    R.check('loss dx', dx, ref['dx'], R.b_dx(ref['og'], P, bd['dz'], d['mem']), what)
    want, bu = _memory_model(d['mem'], d['x'], ref['ce']['own'], P, mode)
    got = _n(crit.centroids)
    assert set(bu) == set(ref['ce']['own'][ref['ce']['valid']].tolist())     # the rows of the batch's proxies, and no other
    for j in range(P):
        if j in bu:
            R.check('loss memory %s' % mode, got[j], want[j], bu[j], what + (j,))
        else:
            assert np.array_equal(_bits(got[j]), _bits(d['mem'][j])), j


@pytest.mark.parametrize('K', CM.LOSS_K)
def test_instance_mode_with_one_camera_and_no_inter_term_is_cluster_memory_loss_bit_for_bit(K):
    from grl_amd.reid.loss import ClusterMemoryLoss
    d = CM.in_loss(K)
    pd = dict(mem=d['cent'], pcl=np.arange(K).astype(np.int32), pcm=np.zeros(K, np.int32))
    for inter_on, w_inter in ((True, 0.0), (False, 0.5)):
        crit = _crit(pd, 50, 'instance', w=(1.0, w_inter))
        crit.inter_on = inter_on
        cm = ClusterMemoryLoss(R.LOSS_D, K, temp=R.LOSS_TEMP, momentum=R.LOSS_MOMENTUM, mode='instance').cuda()
        cm.reset(torch.from_numpy(d['cent']).cuda())
        out = []
        for c in (crit, cm):
            x, y = torch.from_numpy(d['x']).cuda().requires_grad_(True), torch.from_numpy(d['labels']).cuda()
            loss, logits = c(x, y, torch.zeros_like(y)) if c is crit else c(x, y)
            (loss * G).backward()
            out.append((loss.detach(), logits.detach(), x.grad, logits.grl_top1[0], logits.grl_top1[1]))
        torch.cuda.synchronize()
        for a, b in zip(out[0][:4], out[1][:4]):
            assert torch.equal(a, b)
        assert out[0][4] == out[1][4] == R.LOSS_N
        assert torch.equal(crit.centroids, cm.centroids)
        assert not torch.equal(crit.centroids.cpu(), torch.from_numpy(d['cent']))


def test_used_twice_in_one_graph_the_later_update_is_visible_to_the_earlier_backward():
    """As the trainer uses one criterion on frame-level and on clip-level features (pinned for OIM by tests/golden/oim.npz):
    the memory equals, bit for bit, two grl_cmem_update launches in autograd's order with the proxy ids as labels; the earlier
    node's dx is the float64 gradient on the memory after the later node's update -- and not the one on the initial memory."""
    n, D, P, k = R.LOSS_N, R.LOSS_D, 70, 3
    d1, d2 = R.in_loss(P, k, R.loss_seed(P, k)), R.in_loss(P, k, R.loss_seed(P, k, 'second'), 'second')
    d2 = dict(d2, mem=d1['mem'])
    crit = _crit(d1, k, 'hard')
    (x1, y1, c1), (x2, y2, c2) = _dev(d1), _dev(d2)
    l1, _ = crit(x1, y1, c1)
    l2, _ = crit(x2, y2, c2)
    (l1 + l2).backward()
    torch.cuda.synchronize()
    r1, r2 = R.loss(d1, P, k, R.LOSS_W), R.loss(d2, P, k, R.LOSS_W)
    assert R.gap_ok(r1, D) and R.gap_ok(r2, D)
    c = torch.from_numpy(d1['mem']).cuda()
    own1, own2 = (torch.from_numpy(r['ce']['own']).cuda() for r in (r1, r2))
    _call('grl_cmem_update', c, x2.detach(), own2, n, D, P, _f(R.LOSS_MOMENTUM), CM.HARD, None)
    mem1 = _n(c).copy()
    _call('grl_cmem_update', c, x1.detach(), own1, n, D, P, _f(R.LOSS_MOMENTUM), CM.HARD, None)
    assert torch.equal(crit.centroids, c) and not np.array_equal(mem1, d1['mem'])
    b2 = R.b_loss(r2, n, D, P)
    R.check('twice dx later node', _n(x2.grad), r2['dx'], R.b_dx(r2['og'], P, b2['dz'], d1['mem']), P)
    b1 = R.b_loss(r1, n, D, P)
    og = LR.oim_grad(r1['dz'].reshape(-1), P, mem1, [1.0], r1['scalar'], n, P, D)
    R.check('twice dx earlier node', _n(x1.grad), og['dx'], R.b_dx(og, P, b1['dz'], mem1), P)
    stale = np.abs(_n(x1.grad) - r1['dx']) > R.b_dx(r1['og'], P, b1['dz'], d1['mem'])
    assert stale.any(), 'the earlier backward read the memory as it was before the later update'


# ----------------------------------------------------------------------------------------------------------------------
# the flow
def test_proxies_of_the_planted_identities_over_three_cameras():
    from grl_amd import engine
    from grl_amd.reid.train.pseudo import pseudo_labels
    x, pids = CM.planted()
    cams = (np.arange(pids.size) * 7 // 3) % 3
    xd = torch.from_numpy(x).cuda()
    pl = pseudo_labels(xd, 'cosine', **CM.PLANT_COSINE)
    px = pl.proxies(cams)
    pc, pm, sp = R.proxy_numbering(pl.host, cams)
    assert px.n_proxies == pc.size == 18 and np.array_equal(px.proxy_cluster, pc) and np.array_equal(px.proxy_cam, pm)
    assert np.array_equal(px.sample_proxy, sp) and (sp[pids >= 100] == -1).all()
    assert px.proxy_cluster_dev.is_cuda and px.proxy_cluster_dev.dtype == torch.int32 and np.array_equal(_n(px.proxy_cam_dev), pm)
    want = engine.cluster_centroids(xd[:, 16:48].contiguous(), torch.from_numpy(sp).cuda(), 18, 'unit')[0]
    got = px.centroids(xd, cols=(16, 48))
    assert tuple(got.shape) == (18, 32) and torch.equal(got, want)
    with pytest.raises(ValueError, match=r"cols = \(8, 80\) is no column range of 64"):
        px.centroids(xd, cols=(8, 80))


def _trainer(synth_models, mode='instance'):
    import copy
    from grl_amd.reid.loss import ProxyMemoryLoss, PairLoss
    from grl_amd.reid.train import CameraSEQTrainer
    dev = torch.device('cuda:0')
    cnn, siam, siamv = (copy.deepcopy(m).to(dev) for m in synth_models)
    crit_c, crit_u = ProxyMemoryLoss(2048, mode=mode, k_neg=2).to(dev), ProxyMemoryLoss(2048, mode=mode, k_neg=2).to(dev)
    tr = CameraSEQTrainer(cnn, siam, siamv, PairLoss().to(dev), crit_c, crit_u, None)
    params = [p for m in (cnn, siam, siamv) for p in m.parameters()]
    return tr, torch.optim.SGD(params, lr=1e-3, momentum=0.9, weight_decay=5e-4, nesterov=True)


def test_one_camera_trainer_step(synth_models):
    """B = 4, T = 2, five proxies over two cameras: finite loss, precisions and gradients; exactly the memory rows of the batch's
    (cluster, camera) pairs changed, all others bit-unchanged"""
    g = torch.Generator().manual_seed(5)
    seeds = [torch.nn.functional.normalize(torch.randn((5, 2048), generator=g), dim=1) for _ in range(2)]
    pcl, pcm = torch.tensor([0, 0, 1, 2, 2], dtype=torch.int32), torch.tensor([0, 1, 0, 0, 1], dtype=torch.int32)
    tracklets = [((40 + i,), (0, 0, 2, 2)[i], (0, 1, 1, 1)[i]) for i in range(4)]         # proxies 0, 1, 4
    tr, opt = _trainer(synth_models)
    tr.criterion_corr.reset(seeds[0].clone().cuda(), pcl.cuda(), pcm.cuda())
    tr.criterion_uncorr.reset(seeds[1].clone().cuda(), pcl.cuda(), pcm.cuda())
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(0, _loader(tracklets, 4), opt)
    torch.cuda.synchronize()
    for name, m in tr.meters.items():
        assert np.isfinite(float(m.avg)), name
    assert all(bool(torch.isfinite(p.grad).all()) for p in tr._all_params() if p.grad is not None)
    assert any(p.grad is not None and bool(p.grad.abs().sum() > 0) for p in tr._all_params())
    for crit, seed in ((tr.criterion_corr, seeds[0]), (tr.criterion_uncorr, seeds[1])):
        mem = _n(crit.centroids)
        assert np.isfinite(mem).all()
        changed = [not np.array_equal(_bits(mem[j]), _bits(seed.numpy()[j])) for j in range(5)]
        assert changed == [True, True, False, False, True]


def test_train_unsupervised_with_cameras_two_epochs(synth_models, monkeypatch):
    """8 synthetic tracklets over 2 cameras, the clustering replaced by a stub: both memories are reseeded from the proxies'
    centroids over their column slices with the proxies' tables, and inter_on is off in epoch 0 and on in epoch 1"""
    from grl_amd.reid.evaluator import ATTEvaluator
    from grl_amd.reid.train import pseudo
    fixed = [0, 0, 1, 1, -1, 2, 2, -1]
    tracklets = [((60 + i,), 9000 + i, (0, 1, 0, 0, 1, 1, 0, 1)[i]) for i in range(8)]    # pairs (0,0) (0,1) (1,0) (2,0) (2,1)
    tr, opt = _trainer(synth_models)
    ev = ATTEvaluator(tr.model, tr.siamese_model, only_eval=False)
    seen = dict(inter=[], tables=[], mem=[])
    monkeypatch.setattr(pseudo, 'pseudo_labels', lambda xf, **kw: seen.update(xf=xf) or pseudo.PseudoLabels(
        torch.tensor(fixed, device=xf.device), 'stub'))

    def make_train_loader(t):
        seen['inter'].append((tr.criterion_corr.inter_on, tr.criterion_uncorr.inter_on))
        seen['tables'].append((tr.criterion_corr.proxy_cluster.tolist(), tr.criterion_uncorr.proxy_cam.tolist()))
        px = pseudo.PseudoLabels(torch.tensor(fixed, device='cuda')).proxies([x[2] for x in tracklets])
        for crit, cols in ((tr.criterion_uncorr, pseudo.UNCORR_COLS), (tr.criterion_corr, pseudo.CORR_COLS)):
            assert torch.equal(crit.centroids, px.centroids(seen['xf'], cols=cols)) and crit.num_proxies == 5
        return _loader(t, 4)
    with contextlib.redirect_stdout(io.StringIO()):
        hist = pseudo.train_unsupervised(tr, ev, opt, tracklets, lambda t: torch.utils.data.DataLoader(_Clips(t), batch_size=4),
                                         make_train_loader, 2, cameras=True, inter_from_epoch=1)
    torch.cuda.synchronize()
    assert seen['inter'] == [(False, False), (True, True)]
    assert seen['tables'] == [([0, 0, 1, 2, 2], [0, 1, 0, 0, 1])] * 2
    assert len(hist) == 2 and hist[0].n_clusters == 3 and hist[0].n_noise == 2
    for crit in (tr.criterion_corr, tr.criterion_uncorr):
        assert bool(torch.isfinite(crit.centroids).all())
    for name, m in tr.meters.items():
        assert np.isfinite(float(m.avg)), name
