"""Self-paced hybrid memory on a real MI355X: the kernel grl_hybrid_ce (grl_amd/csrc/hybrid.hip) through the C ABI and
HybridMemoryLoss against the float64 restatement of tests/hybrid_ref.py, PseudoLabels.hybrid on planted identities, one
HybridSEQTrainer step and two train_unsupervised(hybrid=True) epochs with and without the self-paced filter.

Every comparison with float64 is per element against that element's derived bound (hybrid_ref.py) -- never a norm over the
tensor.  Discrete outputs (correct, the bits of zero rows and of untouched memory rows, identity singletons against
grl_softmax_ce and ClusterMemoryLoss) are compared exactly; `correct` under the gap condition that test_hybrid_cpu.py asserts
for every case.  The buffers, helpers and conventions are those of test_gpu_head_float64.py / test_gpu_cmem.py."""
import contextlib
import copy
import io

import numpy as np
import pytest
import torch

import hybrid_ref as R
import cmem_ref as CM
import loss_ref as LR
import loss_bounds as LB
from test_gpu_head_float64 import SENT, _call, _n, _f, _out, _got, _Inputs, _err, _window
from test_gpu_loss_float64 import _Ints, _untouched
from test_gpu_cmem import _bits, _Clips

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    yield
    R.dump_ratios('MI355X hybrid memory')
    if GAPS:
        print('  smallest arg-max gap / bound      %.3g' % min(GAPS))


GAPS = []


class _Case(object):
    """the device copies of one input set"""

    def __init__(self, d):
        self.d = d
        self.f = _Inputs(logits=d['logits'])
        self.ints = [_Ints(d['targets']), _Ints(d['cp'], torch.int32), _Ints(d['cm'], torch.int32), _Ints(d['ic'], torch.int32)]

    def launch(self, n, N, dz=True, correct=True):
        d = self.d
        o = dict(loss=_out(1), correct=_out(1), dz=_out(n * d['ldd']), ws=_out(3 * n))
        _call('grl_hybrid_ce', self.f['logits'], d['ld'], self.ints[0].t, self.ints[1].t, self.ints[2].t, self.ints[3].t, n, N,
              d['C'], o['loss'], o['correct'] if correct else None, o['dz'] if dz else None, d['ldd'], o['ws'])
        return o

    def unchanged(self):
        self.f.unchanged()
        for i in self.ints:
            i.unchanged()


def _read(o, n, N, ldd):
    dz0 = np.full(n * ldd, SENT, np.float32)
    return dict(loss=_got(o['loss'], 1)[0].copy(), correct=_got(o['correct'], 1)[0].copy(),
                dz=_window(_got(o['dz'], n * ldd), n, N, ldd, dz0).copy(), rows=_got(o['ws'], 3 * n).copy())


def _same(a, b, keys=('loss', 'correct', 'dz', 'rows')):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in keys)


def _check(got, ref, n, N, C, what):
    bd = R.b_hybrid_ce(ref, n, N, C)
    assert not got['dz'][~ref['valid']].view(np.uint32).any(), what         # zero rows: exactly +0
    assert np.array_equal(got['rows'][2 * n:], ref['valid'].astype(np.float32)), what
    R.check('hybrid_ce loss', got['loss'], ref['loss'], bd['loss'], what)
    R.check('hybrid_ce dz', got['dz'], ref['dz'], bd['dz'], what)
    assert got['correct'] == ref['correct'], what
    if ref['nv'] == 0:
        assert got['loss'] == 0.0 and got['correct'] == 0.0 and not got['dz'].any(), what


# ----------------------------------------------------------------------------------------------------------------------
# the kernel
@pytest.mark.parametrize('n,N', R.CE_CASES)
def test_hybrid_ce(n, N):
    """grl_hybrid_ce over the class layouts, targets -1 and C among the rows: loss and every dlogits element inside
    b_hybrid_ce, correct EQUAL (gap condition: test_hybrid_cpu.py), invalid rows exactly zero, nothing written outside the
    windows, and a second launch gives the same bits.  One more launch per layout with every target -1: no valid row."""
    for name in R.CE_LAYOUTS:
        d = R.in_ce(n, N, name, R.ce_seed(n, N, name))
        case = _Case(d)
        what = (n, N, name)
        ref = R.hybrid_ce(d['logits'], d['ld'], d['targets'], d['cp'], d['cm'], d['ic'], n, N, d['C'])
        GAPS.extend(R.gap_ratios(ref).tolist())
        a = _read(case.launch(n, N), n, N, d['ldd'])
        b = _read(case.launch(n, N), n, N, d['ldd'])
        assert _same(a, b), what
        _check(a, ref, n, N, d['C'], what)
        case.unchanged()
        none = dict(d, targets=np.full(n, -1, np.int64))
        got = _read(_Case(none).launch(n, N), n, N, d['ldd'])
        ref = R.hybrid_ce(none['logits'], d['ld'], none['targets'], d['cp'], d['cm'], d['ic'], n, N, d['C'])
        assert ref['nv'] == 0
        _check(got, ref, n, N, d['C'], what + ('no valid row',))


@pytest.mark.parametrize('n,N', R.CE_CASES)
def test_identity_singletons_are_grl_softmax_ce_bit_for_bit(n, N):
    d = R.in_ce(n, N, 'identity')
    case = _Case(d)
    got = _read(case.launch(n, N), n, N, d['ldd'])
    o = dict(loss=_out(1), correct=_out(1), dz=_out(n * d['ldd']), ws=_out(2 * n))
    _call('grl_softmax_ce', case.f['logits'], d['ld'], case.ints[0].t, None, n, N, o['loss'], o['correct'], o['dz'], d['ldd'], o['ws'])
    want = dict(loss=_got(o['loss'], 1)[0].copy(), correct=_got(o['correct'], 1)[0].copy(),
                dz=_window(_got(o['dz'], n * d['ldd']), n, N, d['ldd'], np.full(n * d['ldd'], SENT, np.float32)).copy())
    assert _same(got, want, ('loss', 'correct', 'dz')), (n, N)
    if n > 1 and N > 1:
        assert (d['targets'] < 0).any() and got['loss'] > 0.0


def test_hybrid_ce_ties_go_to_the_lowest_class():
    d = R.in_ties()
    case = _Case(d)
    ref = R.hybrid_ce(d['logits'], d['ld'], d['targets'], d['cp'], d['cm'], d['ic'], 2, R.TIE_COLS, d['C'])
    got = _read(case.launch(2, R.TIE_COLS), 2, R.TIE_COLS, d['ldd'])
    assert got['correct'] == d['want_correct'] == ref['correct'] and got['rows'][2:4].tolist() == [1.0, 0.0]      # the rows' hits
    _check(got, ref, 2, R.TIE_COLS, d['C'], 'ties')
    for target, hit in ((3, 0.0), (200, 0.0), (1, 1.0)):                       # row 0 again: only the first of the three tied classes hits
        one = dict(d, targets=np.array([target, 70], np.int64))
        assert _read(_Case(one).launch(2, R.TIE_COLS), 2, R.TIE_COLS, d['ldd'])['correct'] == hit, target
    case.unchanged()


def test_hybrid_ce_optional_outputs_may_be_null():
    """dlogits and correct each NULL in turn: the other outputs come out the same bits, nothing behind a NULL pointer's buffer
    is written"""
    n, N = 9, 257
    d = R.in_ce(n, N, 'random')
    case = _Case(d)
    full = _read(case.launch(n, N), n, N, d['ldd'])
    for name in ('dz', 'correct'):
        o = case.launch(n, N, **{name: False})
        _untouched(o[name])
        o[name] = case.launch(n, N)[name]                                  # (so that _read finds a written buffer)
        got = _read(o, n, N, d['ldd'])
        assert _same(full, got, [key for key in ('loss', 'correct', 'dz', 'rows') if key != name]), name
    case.unchanged()


def test_hybrid_ce_rejected_arguments_launch_nothing_and_the_limit_is_served():
    Err = _err()
    n, N, C, big = 2, 8, 3, R.MAX_CLASSES + 1
    z = torch.ones(n * big, device='cuda')
    y = torch.zeros(n, dtype=torch.int64, device='cuda')
    ident = torch.arange(big + 1, dtype=torch.int32, device='cuda')            # class_ptr, class_members and inst_class of singletons
    cp = torch.tensor([0, 1, 3, 8], dtype=torch.int32, device='cuda')
    ic = torch.tensor([0, 1, 1, 2, 2, 2, 2, 2], dtype=torch.int32, device='cuda')
    loss, cor, dz, ws = _out(1), _out(1), _out(n * big), _out(3 * n)

    def args(**kw):
        a = dict(z=z, ld=N, y=y, cp=cp, cm=ident, ic=ic, n=n, N=N, C=C, loss=loss, dz=dz, ldd=N, ws=ws)
        a.update(kw)
        return (a['z'], a['ld'], a['y'], a['cp'], a['cm'], a['ic'], a['n'], a['N'], a['C'], a['loss'], cor, a['dz'], a['ldd'], a['ws'])
    for kw in (dict(n=0), dict(N=0), dict(C=0), dict(C=N + 1), dict(ld=N - 1), dict(ldd=N - 1), dict(z=None), dict(y=None),
               dict(cp=None), dict(cm=None), dict(ic=None), dict(loss=None), dict(ws=None),
               dict(n=1, N=big, C=big, ld=big, ldd=big, cp=ident, ic=ident)):
        with pytest.raises(Err):
            _call('grl_hybrid_ce', *args(**kw))
    for t in (loss, cor, dz, ws):
        _untouched(t)
    top = R.MAX_CLASSES
    _call('grl_hybrid_ce', *args(n=1, N=top, C=top, ld=top, ldd=top, cp=ident, ic=ident))      # the limit itself is served
    torch.cuda.synchronize()
    assert abs(float(_got(loss, 1)[0]) - np.log(top)) < 1e-4 and float(_got(cor, 1)[0]) == 1.0     # equal logits, target 0
    g = _got(dz, n * big)[:top]
    assert abs(g[0] - (1.0 / top - 1.0)) < 1e-6 and np.abs(g[1:] - 1.0 / top).max() < 1e-9


# ----------------------------------------------------------------------------------------------------------------------
# HybridMemoryLoss
G = 0.75        # the gradient handed to the loss: (G * loss).backward()


def _crit(d, D):
    from grl_amd.reid.loss import HybridMemoryLoss
    crit = HybridMemoryLoss(D, temp=R.LOSS_TEMP, momentum=R.LOSS_MOMENTUM).cuda()
    assert crit.reset(torch.from_numpy(d['mem']).cuda(), *(torch.from_numpy(d[k]).cuda() for k in ('cp', 'cm', 'ic'))) is crit
    assert crit.num_instances == d['mem'].shape[0] and crit.num_classes == d['C']
    return crit


def _dev(d):
    return (torch.from_numpy(d['x']).cuda().requires_grad_(True), torch.from_numpy(d['targets']).cuda(),
            torch.from_numpy(d['index']).cuda())


@pytest.mark.parametrize('D', R.LOSS_D)
def test_loss_gradient_and_memory_against_float64(D):
    """n = 9, N = 70 in mixed classes, one row with the target -1 and one with the index -1: logits, loss and dx end to end from
    the inputs inside b_loss / b_dx; the top-1 count EQUAL to the model's on the logits the loss returned; the memory after the
    backward inside its bound at the batch's indices -- the row with the invalid target included --, all other rows
    bit-unchanged.

    D = 1028 is no multiple of 32, the K the logits GEMM takes: the forward hands it zero-padded copies of both operands
    (engine._pad_features); the zero columns add +0 to every dot product, so the bound of D products stands."""
    n, N = R.LOSS_N, R.LOSS_COLS
    d = R.in_loss(D, R.loss_seed(D))
    crit = _crit(d, D)
    x, y, idx = _dev(d)
    loss, logits = crit(x, y, idx)
    assert not logits.requires_grad and torch.equal(crit.memory.cpu(), torch.from_numpy(d['mem']))       # forward updates nothing
    (loss * G).backward()
    torch.cuda.synchronize()
    ref = R.loss(d, D, g=G)
    bd = R.b_loss(ref, n, D, N, d['C'])
    z = _n(logits)
    R.check('loss logits', z, ref['logits'], bd['logits'], D)
    R.check('loss', loss.item(), ref['loss'], bd['loss'], D)
    on_device = R.hybrid_ce(z.reshape(-1), N, d['targets'], d['cp'], d['cm'], d['ic'], n, N, d['C'])
    assert float(logits.grl_top1[0]) == on_device['correct'] == ref['ce']['correct'] and logits.grl_top1[1] == n
    dx = _n(x.grad)
    assert not dx[4].any() and dx[7].any()                                   # the invalid target; the invalid index still learns
    R.check('loss dx', dx, ref['dx'], R.b_dx(ref['og'], N, bd['dz'], d['mem']), D)
    m = CM.m32(R.LOSS_MOMENTUM)
    upd = LR.oim_update(d['mem'], d['x'], d['index'], n, D, N, m)
    bu = LB.b_oim_update(upd, D, m)
    got = _n(crit.memory)
    assert set(bu) == set(d['index'][d['index'] >= 0].tolist()) and int(d['index'][4]) in bu
    for j in range(N):
        if j in bu:
            R.check('loss memory', got[j], upd['lut'][j], bu[j], (D, j))
        else:
            assert np.array_equal(_bits(got[j]), _bits(d['mem'][j])), j


@pytest.mark.parametrize('D', R.LOSS_D)
def test_all_singletons_with_index_equal_targets_is_cluster_memory_loss_bit_for_bit(D):
    """loss, logits, dx, the top-1 count and the memory after the backward: the same bits from both criteria.

    D = 1028 is no multiple of 32, the K the logits GEMM takes: the forward hands it zero-padded copies of both operands
    (engine._pad_features); the zero columns add +0 to every dot product, so the bound of D products stands.  OIM.forward, which
    ClusterMemoryLoss runs, pads in the same way."""
    from grl_amd.reid.loss import ClusterMemoryLoss
    N = R.LOSS_COLS
    d = R.in_loss(D, singletons=True)
    d['index'] = d['targets'].copy()                                         # (row 4: both -1)
    crit = _crit(d, D)
    cm = ClusterMemoryLoss(D, N, temp=R.LOSS_TEMP, momentum=R.LOSS_MOMENTUM, mode='instance').cuda()
    cm.reset(torch.from_numpy(d['mem']).cuda())
    out = []
    for c in (crit, cm):
        x, y, idx = _dev(d)
        loss, logits = c(x, y, idx) if c is crit else c(x, y)
        (loss * G).backward()
        out.append((loss.detach(), logits.detach(), x.grad, logits.grl_top1[0], logits.grl_top1[1]))
    torch.cuda.synchronize()
    for a, b in zip(out[0][:4], out[1][:4]):
        assert torch.equal(a, b)
    assert out[0][4] == out[1][4] == R.LOSS_N
    assert torch.equal(crit.memory, cm.centroids) and not torch.equal(crit.memory.cpu(), torch.from_numpy(d['mem']))


def test_loss_and_gradient_with_more_memory_rows_than_one_gradient_launch_takes():
    """N = 5200 > 5120, the columns grl_oim_grad takes: the backward goes through it in two column blocks added by grl_axpby.
    Loss and dx inside the bounds of the one-launch case (the blocked chain is shorter), the memory changed at the batch's
    indices only, and a second run gives the same bits."""
    D, n, N = 256, R.LOSS_N, R.LOSS_WIDE
    d = R.in_loss(D, N=N)
    outs = []
    for _ in range(2):
        crit = _crit(d, D)
        x, y, idx = _dev(d)
        loss, _ = crit(x, y, idx)
        (loss * G).backward()
        torch.cuda.synchronize()
        outs.append((loss.detach().clone(), x.grad.clone(), crit.memory.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    ref = R.loss(d, D, g=G)
    bd = R.b_loss(ref, n, D, N, d['C'])
    R.check('wide loss', outs[0][0].item(), ref['loss'], bd['loss'], N)
    R.check('wide dx', _n(outs[0][1]), ref['dx'], R.b_dx(ref['og'], N, bd['dz'], d['mem']), N)
    # the second block matters: without it dx is off by far more than the bound
    lo = LR.oim_grad(ref['dz'][:, :5120].copy().reshape(-1), 5120, d['mem'][:5120], [G], ref['scalar'], n, 5120, D)
    assert (np.abs(lo['dx'] - ref['dx']) > R.b_dx(ref['og'], N, bd['dz'], d['mem'])).any()
    changed = np.flatnonzero((_bits(_n(outs[0][2])) != _bits(d['mem'])).any(1))
    assert changed.tolist() == sorted(set(d['index'][d['index'] >= 0].tolist()))


def test_used_twice_in_one_graph_the_later_update_is_visible_to_the_earlier_backward():
    """As the trainer uses one criterion on frame-level and on clip-level features (pinned for OIM by tests/golden/oim.npz):
    the memory equals, bit for bit, two grl_oim_update launches in autograd's order with the indices as labels; the earlier
    node's dx is the float64 gradient on the memory after the later node's update -- and not the one on the initial memory."""
    D, n, N = 256, R.LOSS_N, R.LOSS_COLS
    d1, d2 = R.in_loss(D, R.loss_seed(D)), R.in_loss(D, R.loss_seed(D, 'second'), 'second')
    d2 = dict(d2, mem=d1['mem'], cp=d1['cp'], cm=d1['cm'], ic=d1['ic'], C=d1['C'], targets=np.where(d2['targets'] >= 0,
              d1['ic'][np.maximum(d2['index'], 0)].astype(np.int64), -1))
    crit = _crit(d1, D)
    (x1, y1, i1), (x2, y2, i2) = _dev(d1), _dev(d2)
    l1, _ = crit(x1, y1, i1)
    l2, _ = crit(x2, y2, i2)
    (l1 + l2).backward()
    torch.cuda.synchronize()
    r1, r2 = R.loss(d1, D), R.loss(d2, D)
    c = torch.from_numpy(d1['mem']).cuda()
    _call('grl_oim_update', c, x2.detach(), i2, n, D, N, _f(R.LOSS_MOMENTUM))
    mem1 = _n(c).copy()
    _call('grl_oim_update', c, x1.detach(), i1, n, D, N, _f(R.LOSS_MOMENTUM))
    assert torch.equal(crit.memory, c) and not np.array_equal(mem1, d1['mem'])
    b2 = R.b_loss(r2, n, D, N, d1['C'])
    R.check('twice dx later node', _n(x2.grad), r2['dx'], R.b_dx(r2['og'], N, b2['dz'], d1['mem']), D)
    b1 = R.b_loss(r1, n, D, N, d1['C'])
    og = LR.oim_grad(r1['dz'].reshape(-1), N, mem1, [1.0], r1['scalar'], n, N, D)
    R.check('twice dx earlier node', _n(x1.grad), og['dx'], R.b_dx(og, N, b1['dz'], mem1), D)
    stale = np.abs(_n(x1.grad) - r1['dx']) > R.b_dx(r1['og'], N, b1['dz'], d1['mem'])
    assert stale.any(), 'the earlier backward read the memory as it was before the later update'


def test_out_of_range_indices_leave_the_memory_bits_unchanged():
    D, N = 256, R.LOSS_COLS
    d = R.in_loss(D, R.loss_seed(D))
    d['index'] = np.array([-1, N, N + 5, -100, 2 ** 40, -1, N, -7, N + 1], np.int64)
    crit = _crit(d, D)
    x, y, idx = _dev(d)
    loss, _ = crit(x, y, idx)
    loss.backward()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(_n(crit.memory)), _bits(d['mem'])) and bool(x.grad.abs().sum() > 0)


# ----------------------------------------------------------------------------------------------------------------------
# the flow
def test_hybrid_labels_keep_the_planted_outliers_as_singleton_classes():
    from grl_amd import engine
    from grl_amd.reid.train.pseudo import pseudo_labels
    x, pids = CM.planted()
    xd = torch.from_numpy(x).cuda()
    pl = pseudo_labels(xd, 'cosine', **CM.PLANT_COSINE)
    h = pl.hybrid()
    want, nc = R.hybrid_numbering(pl.host)
    assert pl.n_clusters == CM.PLANT_IDS and pl.n_noise == CM.PLANT_OUTLIERS and h.n_classes == nc == 9
    assert np.array_equal(h.sample_class, want) and sorted(want[pids >= 100].tolist()) == [6, 7, 8]
    sizes = np.diff(h.class_ptr)
    assert sizes.tolist() == [CM.PLANT_PER] * 6 + [1] * 3
    assert h.class_ptr_dev.is_cuda and h.inst_class_dev.dtype == torch.int32 and np.array_equal(_n(h.class_members_dev), h.class_members)
    n = pids.size
    got = h.memory(xd, cols=(16, 48))
    want_mem = engine.cluster_centroids(xd[:, 16:48].contiguous(), torch.arange(n, device='cuda'), n, 'unit')[0]
    assert tuple(got.shape) == (n, 32) and torch.equal(got, want_mem)
    unit = torch.nn.functional.normalize(xd[:, 16:48].double(), dim=1)
    assert float((got.double() - unit).abs().max()) < 1e-6
    with pytest.raises(ValueError, match=r"cols = \(8, 80\) is no column range of 64"):
        h.memory(xd, cols=(8, 80))


class _IndexedClips(_Clips):
    """_Clips whose items end with their dataset index, as RawVideoDataset(index=True)"""

    def __getitem__(self, i):
        return _Clips.__getitem__(self, i) + (torch.tensor(i, dtype=torch.int64),)


def _loader(tracklets, batch, order=None):
    ds = _IndexedClips(tracklets)
    return torch.utils.data.DataLoader(ds if order is None else torch.utils.data.Subset(ds, order), batch_size=batch, shuffle=False,
                                       drop_last=True)


def _trainer(synth_models):
    from grl_amd.reid.loss import HybridMemoryLoss, PairLoss
    from grl_amd.reid.train import HybridSEQTrainer
    dev = torch.device('cuda:0')
    cnn, siam, siamv = (copy.deepcopy(m).to(dev) for m in synth_models)
    crit_c, crit_u = HybridMemoryLoss(2048).to(dev), HybridMemoryLoss(2048).to(dev)
    tr = HybridSEQTrainer(cnn, siam, siamv, PairLoss().to(dev), crit_c, crit_u, None)
    params = [p for m in (cnn, siam, siamv) for p in m.parameters()]
    return tr, torch.optim.SGD(params, lr=1e-3, momentum=0.9, weight_decay=5e-4, nesterov=True)


def test_one_hybrid_trainer_step(synth_models):
    """B = 4, T = 2 out of six instances in the classes {0, 3}, {1}, {2, 4}, {5}: finite loss, precisions and gradients; exactly
    the memory rows at the batch's indices changed, all others bit-unchanged"""
    from grl_amd.reid.train.pseudo import PseudoLabels
    g = torch.Generator().manual_seed(5)
    seeds = [torch.nn.functional.normalize(torch.randn((6, 2048), generator=g), dim=1) for _ in range(2)]
    h = PseudoLabels(torch.tensor([0, -1, 1, 0, 1, -1], device='cuda')).hybrid()
    assert h.sample_class.tolist() == [0, 2, 1, 0, 1, 3]
    tracklets = h.relabel([((40 + i,), 900 + i, 0) for i in range(6)])
    tr, opt = _trainer(synth_models)
    for crit, seed in ((tr.criterion_corr, seeds[0]), (tr.criterion_uncorr, seeds[1])):
        crit.reset(seed.clone().cuda(), h.class_ptr_dev, h.class_members_dev, h.inst_class_dev)
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(0, _loader(tracklets, 4, order=[0, 3, 5, 5]), opt)            # a pair of class 0 and the singleton 5 with itself
    torch.cuda.synchronize()
    for name, m in tr.meters.items():
        assert np.isfinite(float(m.avg)), name
    assert all(bool(torch.isfinite(p.grad).all()) for p in tr._all_params() if p.grad is not None)
    assert any(p.grad is not None and bool(p.grad.abs().sum() > 0) for p in tr._all_params())
    for crit, seed in ((tr.criterion_corr, seeds[0]), (tr.criterion_uncorr, seeds[1])):
        mem = _n(crit.memory)
        assert np.isfinite(mem).all()
        changed = [not np.array_equal(_bits(mem[j]), _bits(seed.numpy()[j])) for j in range(6)]
        assert changed == [True, False, False, True, False, True]


@pytest.mark.parametrize('self_paced', (None, dict(delta=0.02, method='cosine', eps=-0.7, min_samples=2)))
def test_train_unsupervised_hybrid_two_epochs(synth_models, monkeypatch, self_paced):
    """8 synthetic tracklets, the clusterings replaced by stubs: every tracklet is in each epoch's training list, the noise
    samples under class ids of their own; both memories are reseeded from the instances' unit rows over their column slices
    with the labels' tables.  With ``self_paced`` the three clusterings go through the filter and one state serves the run."""
    from grl_amd.reid.evaluator import ATTEvaluator
    from grl_amd.reid.train import pseudo
    from grl_amd import engine
    fixed = [0, 0, 1, 1, 1, 2, 2, -1]
    tight = [0, 0, 1, 1, -1, 2, 2, -1]               # cluster 1 loses sample 4 under the tighter eps
    loose = [0, 0, 1, 1, 1, 2, 2, 2]                 # cluster 2 swallows the noise sample under the looser one
    tracklets = [((60 + i,), 9000 + i, i % 2) for i in range(8)]
    tr, opt = _trainer(synth_models)
    ev = ATTEvaluator(tr.model, tr.siamese_model, only_eval=False)
    seen = dict(lists=[], eps=[], states=[])

    class Res(object):
        def __init__(self, labels, dev):
            self.labels = torch.tensor(labels, device=dev)
    monkeypatch.setattr(pseudo, 'pseudo_labels', lambda xf, **kw: seen.update(xf=xf, kw=kw) or pseudo.PseudoLabels(
        torch.tensor(fixed, device=xf.device), 'stub'))

    def cluster(xf, eps, min_samples, metric):
        seen['eps'].append(round(float(eps), 4))
        seen['xf'] = xf
        return Res({-0.72: tight, -0.7: fixed, -0.68: loose}[round(float(eps), 4)], xf.device)
    monkeypatch.setattr(engine, 'cluster', cluster)
    real_filter = pseudo.self_paced_filter
    monkeypatch.setattr(pseudo, 'self_paced_filter', lambda a, b, c, st: seen['states'].append(st) or real_filter(a, b, c, st))
    # self-paced: tau = 2/3 (indep = 1, 1, 2/3 -> entry min(2, round(2.7))): every cluster passes; sample 4 leaves cluster 1:
    # R_comp = 1/3 against comp = 2/3
    want_host = [0, 0, 1, 1, -1, 2, 2, -1] if self_paced else fixed
    want_class = [0, 0, 1, 1, 3, 2, 2, 4] if self_paced else [0, 0, 1, 1, 1, 2, 2, 3]

    def make_train_loader(t):
        seen['lists'].append(t)
        h = pseudo.PseudoLabels(torch.tensor(want_host, device='cuda')).hybrid()
        for crit, cols in ((tr.criterion_uncorr, pseudo.UNCORR_COLS), (tr.criterion_corr, pseudo.CORR_COLS)):
            assert torch.equal(crit.memory, h.memory(seen['xf'], cols=cols)) and crit.num_instances == 8
            assert crit.class_ptr.tolist() == h.class_ptr.tolist() and crit.class_members.tolist() == h.class_members.tolist()
            assert crit.inst_class.tolist() == want_class
        return _loader(t, 4)
    with contextlib.redirect_stdout(io.StringIO()):
        hist = pseudo.train_unsupervised(tr, ev, opt, tracklets, lambda t: torch.utils.data.DataLoader(_Clips(t), batch_size=4),
                                         make_train_loader, 2, hybrid=True, self_paced=self_paced)
    torch.cuda.synchronize()
    assert len(seen['lists']) == 2
    for t in seen['lists']:
        assert len(t) == 8 and [x[0] for x in t] == [x[0] for x in tracklets] and [x[1] for x in t] == want_class
    assert len(hist) == 2 and hist[0].host.tolist() == want_host and hist[0].n_noise == want_host.count(-1)
    if self_paced:
        assert seen['eps'] == [-0.7, -0.72, -0.68] * 2 and len(seen['states']) == 2 and seen['states'][0] is seen['states'][1]
        assert seen['states'][0].tau == 2 / 3
    else:
        assert seen['kw'] == dict(min_clusters=0)
    for crit in (tr.criterion_corr, tr.criterion_uncorr):
        assert bool(torch.isfinite(crit.memory).all())
    for name, m in tr.meters.items():
        assert np.isfinite(float(m.avg)), name
