"""Mean-teacher soft targets for the hybrid and the proxy memory on a real MI355X: the kernels
grl_soft_hybrid_ce (grl_amd/csrc/soft_hybrid.hip) and grl_soft_proxy_ce (grl_amd/csrc/soft_proxy.hip) through the C ABI,
SoftHybridMemoryLoss / SoftProxyMemoryLoss, one step of MeanTeacherHybridSEQTrainer / MeanTeacherCameraSEQTrainer and two
train_unsupervised epochs of each, against the float64 models of tests/soft_memory_ref.py.

Every comparison with float64 is per element against that element's derived bound -- never a norm over the tensor.  Discrete
outputs (correct, own, negsel, the bits of zero rows) and everything the contract promises bit for bit (w = 0 against the hard
kernels, identity singletons against grl_soft_ce, a second run, a zero-weight trainer step) are compared exactly.  The buffers,
helpers and conventions are those of test_gpu_hybrid.py / test_gpu_proxy.py / test_gpu_teacher.py."""
import contextlib
import copy
import io

import numpy as np
import pytest
import torch

import soft_memory_ref as R
import hybrid_ref as HR
import proxy_ref as PR
from test_gpu_head_float64 import GUARD, SENT, _call, _n, _f, _out, _got, _Inputs, _err, _window
from test_gpu_loss_float64 import ISENT, _Ints, _untouched
from test_gpu_cmem import _bits, _Clips, _loader

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    yield
    R.dump_ratios('MI355X soft hybrid / proxy memory')


def _k(k, P):
    return P if k == 'P' else min(k, P)


def _iout(n, dtype):
    return torch.full((n + GUARD,), ISENT, dtype=dtype, device='cuda')


def _igot(t, n):
    torch.cuda.synchronize()
    a = _n(t)
    assert (a[n:] == ISENT).all(), 'written past the end of an integer output'
    return a[:n]


def _same(a, b, keys):
    return all(np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                              b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]) for k in keys)


# ----------------------------------------------------------------------------------------------------------------------
# grl_soft_hybrid_ce
class _Hybrid(object):
    """the device copies of one input set"""

    def __init__(self, d):
        self.d = d
        self.f = _Inputs(logits=d['logits'], tlogits=d['tlogits'])
        self.ints = [_Ints(d['targets']), _Ints(d['cp'], torch.int32), _Ints(d['cm'], torch.int32), _Ints(d['ic'], torch.int32)]

    def soft(self, n, N, w, teacher=True):
        """one launch into fresh sentinel buffers; w = 0: the workspace is the 3 n floats of grl_hybrid_ce (the guard behind it
        shows that the teacher's scratch was not touched)"""
        d = self.d
        o = dict(loss=_out(1), correct=_out(1), dz=_out(n * d['ldd']), ws=_out(3 * n + (n * d['C'] if w != 0.0 else 0)))
        _call('grl_soft_hybrid_ce', self.f['logits'], d['ld'], self.f['tlogits'] if teacher else None, d['ldt'], self.ints[0].t,
              self.ints[1].t, self.ints[2].t, self.ints[3].t, _f(w), n, N, d['C'], o['loss'], o['correct'], o['dz'], d['ldd'], o['ws'])
        return self.read(o, n, N, w)

    def hard(self, n, N):
        d = self.d
        o = dict(loss=_out(1), correct=_out(1), dz=_out(n * d['ldd']), ws=_out(3 * n))
        _call('grl_hybrid_ce', self.f['logits'], d['ld'], self.ints[0].t, self.ints[1].t, self.ints[2].t, self.ints[3].t, n, N,
              d['C'], o['loss'], o['correct'], o['dz'], d['ldd'], o['ws'])
        return self.read(o, n, N, 0.0)

    def read(self, o, n, N, w):
        ldd = self.d['ldd']
        full = _got(o['ws'], 3 * n + (n * self.d['C'] if w != 0.0 else 0))
        return dict(loss=_got(o['loss'], 1)[0].copy(), correct=_got(o['correct'], 1)[0].copy(), rows=full[:3 * n].copy(),
                    dz=_window(_got(o['dz'], n * ldd), n, N, ldd, np.full(n * ldd, SENT, np.float32)).copy())

    def unchanged(self):
        self.f.unchanged()
        for i in self.ints:
            i.unchanged()


KEYS_H = ('loss', 'correct', 'dz', 'rows')


def _check_hybrid(got, ref, n, N, C, what):
    bd = R.b_soft_hybrid_ce(ref, n, N, C)
    assert not got['dz'][~ref['valid']].view(np.uint32).any(), what         # zero rows: exactly +0
    assert np.array_equal(got['rows'][2 * n:], ref['valid'].astype(np.float32)), what
    print('soft_hybrid %r: loss %.9g (float64 %.9g, bound %.3g)' % (what, got['loss'], ref['loss'], bd['loss']))
    R.check('soft_hybrid_ce loss', got['loss'], ref['loss'], bd['loss'], what)
    R.check('soft_hybrid_ce dz', got['dz'], ref['dz'], bd['dz'], what)
    assert got['correct'] == ref['correct'], what
    if ref['nv'] == 0:
        assert got['loss'] == 0.0 and got['correct'] == 0.0 and not got['dz'].any(), what


@pytest.mark.parametrize('n,N', R.HY_CASES)
def test_soft_hybrid_ce(n, N):
    """n x N over the partitions (all singletons, one class of more than a wave of members beside singletons, interleaved
    members), ld, ldt, ldd wider than N and all different, the targets -1 and C among the rows, w = 0, 0.5, 1: loss and every
    dlogits element inside the derived bound, correct EQUAL (the student's arg-max; gap condition: test_soft_memory_cpu.py),
    invalid rows exactly +0, nothing written outside the windows, the same bits from a second launch; w = 0 with tlogits NULL is
    grl_hybrid_ce bit for bit.  One more launch per partition with every target -1: no valid row."""
    for name in R.HY_LAYOUTS:
        d = R.in_hybrid(n, N, name, R.hy_seed(n, N, name))
        case = _Hybrid(d)
        for w in R.W_SWEEP:
            what = (n, N, name, w)
            ref = R.soft_hybrid_ce(d['logits'], d['ld'], d['tlogits'], d['ldt'], d['targets'], d['cp'], d['cm'], d['ic'], w, n, N,
                                   d['C'])
            a, b = case.soft(n, N, w), case.soft(n, N, w)
            assert _same(a, b, KEYS_H), what
            _check_hybrid(a, ref, n, N, d['C'], what)
        assert _same(case.soft(n, N, 0.0, teacher=False), case.hard(n, N), KEYS_H), (n, N, name, 'w = 0 is grl_hybrid_ce')
        case.unchanged()
        none = dict(d, targets=np.where(np.arange(n) % 2 == 0, -1, d['C']).astype(np.int64))
        ref = R.soft_hybrid_ce(d['logits'], d['ld'], d['tlogits'], d['ldt'], none['targets'], d['cp'], d['cm'], d['ic'], 0.5, n, N,
                               d['C'])
        assert ref['nv'] == 0
        _check_hybrid(_Hybrid(none).soft(n, N, 0.5), ref, n, N, d['C'], (n, N, name, 'no valid row'))


@pytest.mark.parametrize('n,N', R.HY_CASES)
def test_soft_hybrid_ce_on_identity_singletons_is_grl_soft_ce_bit_for_bit(n, N):
    d = R.in_hybrid(n, N, 'identity')
    case = _Hybrid(d)
    ldd = d['ldd']
    for w in R.W_SWEEP:
        got = case.soft(n, N, w)
        o = dict(loss=_out(1), correct=_out(1), dz=_out(n * ldd), ws=_out(3 * n))
        _call('grl_soft_ce', case.f['logits'], d['ld'], case.f['tlogits'], d['ldt'], case.ints[0].t, _f(w), n, N, o['loss'],
              o['correct'], o['dz'], ldd, o['ws'])
        want = dict(loss=_got(o['loss'], 1)[0].copy(), correct=_got(o['correct'], 1)[0].copy(), rows=_got(o['ws'], 3 * n).copy(),
                    dz=_window(_got(o['dz'], n * ldd), n, N, ldd, np.full(n * ldd, SENT, np.float32)).copy())
        assert _same(got, want, KEYS_H), (n, N, w)
    if n > 1 and N > 1:
        assert (d['targets'] < 0).any() and got['loss'] > 0.0
    case.unchanged()


def test_soft_hybrid_ce_rejected_arguments_launch_nothing():
    """everything grl_hybrid_ce refuses, w outside [0, 1] (NaN included), w != 0 without tlogits or with ldt < N: GRL_EINVAL,
    every sentinel output intact; the same arguments with w = 0 and no teacher are served"""
    Err = _err()
    n, N, C, big = 2, 8, 3, HR.MAX_CLASSES + 1
    z = torch.ones(n * big, device='cuda')
    y = torch.zeros(n, dtype=torch.int64, device='cuda')
    ident = torch.arange(big + 1, dtype=torch.int32, device='cuda')
    cp = torch.tensor([0, 1, 3, 8], dtype=torch.int32, device='cuda')
    ic = torch.tensor([0, 1, 1, 2, 2, 2, 2, 2], dtype=torch.int32, device='cuda')
    loss, cor, dz, ws = _out(1), _out(1), _out(n * big), _out(3 * n + n * C)

    def args(**kw):
        a = dict(z=z, ld=N, t=z, ldt=N, y=y, cp=cp, cm=ident, ic=ic, w=0.5, n=n, N=N, C=C, loss=loss, dz=dz, ldd=N, ws=ws)
        a.update(kw)
        return (a['z'], a['ld'], a['t'], a['ldt'], a['y'], a['cp'], a['cm'], a['ic'], _f(a['w']), a['n'], a['N'], a['C'], a['loss'],
                cor, a['dz'], a['ldd'], a['ws'])
    for kw in (dict(n=0), dict(N=0), dict(C=0), dict(C=N + 1), dict(ld=N - 1), dict(ldd=N - 1), dict(z=None), dict(y=None),
               dict(cp=None), dict(cm=None), dict(ic=None), dict(loss=None), dict(ws=None),
               dict(n=1, N=big, C=big, ld=big, ldt=big, ldd=big, cp=ident, ic=ident),
               dict(w=-0.5), dict(w=1.5), dict(w=float('nan')), dict(t=None), dict(ldt=N - 1)):
        with pytest.raises(Err, match='soft_hybrid_ce'):
            _call('grl_soft_hybrid_ce', *args(**kw))
    for t in (loss, cor, dz, ws):
        _untouched(t)
    _call('grl_soft_hybrid_ce', *args(w=0.0, t=None, ldt=0))
    torch.cuda.synchronize()
    assert np.isfinite(_got(loss, 1)[0]) and float(_got(cor, 1)[0]) in (0.0, 1.0, 2.0)
    assert (_n(ws)[3 * n:] == SENT).all()                                       # w = 0: the teacher's scratch is not touched


# ----------------------------------------------------------------------------------------------------------------------
# grl_soft_proxy_ce
class _Proxy(object):
    def __init__(self, d):
        self.d = d
        self.f = _Inputs(logits=d['logits'], tlogits=d['tlogits'])
        self.ints = [_Ints(d['labels']), _Ints(d['cams']), _Ints(d['pcl'], torch.int32), _Ints(d['pcm'], torch.int32)]

    def _outs(self, n, k):
        return dict(loss=_out(1), correct=_out(1), dz=_out(n * self.d['ldd']), own=_iout(n, torch.int64),
                    negsel=_iout(n * max(k, 1), torch.int32), ws=_out(3 * n))

    def soft(self, n, P, k, wts, w, teacher=True):
        d, o = self.d, self._outs(n, k)
        _call('grl_soft_proxy_ce', self.f['logits'], d['ld'], self.f['tlogits'] if teacher else None, d['ldt'], self.ints[0].t,
              self.ints[1].t, self.ints[2].t, self.ints[3].t, _f(w), n, P, k, _f(wts[0]), _f(wts[1]), o['loss'], o['correct'],
              o['dz'], d['ldd'], o['own'], o['negsel'], o['ws'])
        return self.read(o, n, P, k)

    def hard(self, n, P, k, wts):
        d, o = self.d, self._outs(n, k)
        _call('grl_proxy_ce', self.f['logits'], d['ld'], self.ints[0].t, self.ints[1].t, self.ints[2].t, self.ints[3].t, n, P, k,
              _f(wts[0]), _f(wts[1]), o['loss'], o['correct'], o['dz'], d['ldd'], o['own'], o['negsel'], o['ws'])
        return self.read(o, n, P, k)

    def read(self, o, n, P, k):
        ldd = self.d['ldd']
        return dict(loss=_got(o['loss'], 1)[0].copy(), correct=_got(o['correct'], 1)[0].copy(), own=_igot(o['own'], n).copy(),
                    dz=_window(_got(o['dz'], n * ldd), n, P, ldd, np.full(n * ldd, SENT, np.float32)).copy(),
                    negsel=_igot(o['negsel'], n * max(k, 1)).copy(), rows=_got(o['ws'], 3 * n).copy())

    def unchanged(self):
        self.f.unchanged()
        for i in self.ints:
            i.unchanged()


KEYS_P = ('loss', 'correct', 'own', 'dz', 'negsel', 'rows')


def _check_proxy(got, ref, n, P, k, what):
    assert np.array_equal(got['own'], ref['own']), what
    if k > 0:
        assert np.array_equal(got['negsel'].reshape(n, k), ref['negsel']), what
    else:
        assert (got['negsel'] == ISENT).all(), what                         # k_neg = 0: negsel is ignored
    assert got['correct'] == ref['correct'], what
    bd = R.b_soft_proxy_ce(ref, n, P)
    assert not got['dz'][~ref['valid']].view(np.uint32).any(), what         # zero rows: exactly +0
    assert np.array_equal(got['rows'][2 * n:], ref['valid'].astype(np.float32)), what
    R.check('soft_proxy_ce loss', got['loss'], ref['loss'], bd['loss'], what)
    R.check('soft_proxy_ce dz', got['dz'], ref['dz'], bd['dz'], what)
    if ref['nv'] == 0:
        assert got['loss'] == 0.0 and got['correct'] == 0.0 and not got['dz'].any(), what


@pytest.mark.parametrize('n,P', R.PX_CASES)
def test_soft_proxy_ce(n, P):
    """n x P over the tables (spread, mixed, mixed with logits tied across every selection threshold), k_neg = 0, 1, 50, P,
    w_intra or w_inter = 0, w = 0, 0.5, 1, the noise label and a pair without a proxy among the rows: own, negsel and correct
    EQUAL to the model's AND to grl_proxy_ce's on the same logits, loss and every dlogits element inside the derived bound,
    invalid rows exactly +0, nothing written outside the windows, the same bits from a second launch; w = 0 with tlogits NULL is
    grl_proxy_ce bit for bit.  One more launch per table with every label -1: no valid row."""
    for pattern, ties in (('spread', False), ('mixed', False), ('mixed', True)):
        d = R.in_proxy(n, P, 3, pattern, ties=ties)
        case = _Proxy(d)
        for k0 in R.PX_K:
            k = _k(k0, P)
            for wts in R.PX_WEIGHTS:
                hard = case.hard(n, P, k, wts)
                for w in R.W_SWEEP:
                    what = (n, P, pattern, ties, k, wts, w)
                    ref = R.soft_proxy_ce(d['logits'], d['ld'], d['tlogits'], d['ldt'], d['labels'], d['cams'], d['pcl'], d['pcm'],
                                          w, n, P, k, *wts)
                    a, b = case.soft(n, P, k, wts, w), case.soft(n, P, k, wts, w)
                    assert _same(a, b, KEYS_P), what
                    _check_proxy(a, ref, n, P, k, what)
                    assert _same(a, hard, ('own', 'negsel', 'correct')), what
                assert _same(case.soft(n, P, k, wts, 0.0, teacher=False), hard, KEYS_P), (n, P, pattern, k, wts, 'w = 0')
        case.unchanged()
        none = dict(d, labels=np.full(n, -1, np.int64))
        k = min(3, P)
        ref = R.soft_proxy_ce(d['logits'], d['ld'], d['tlogits'], d['ldt'], none['labels'], d['cams'], d['pcl'], d['pcm'], 0.5, n, P,
                              k, 1.0, 0.5)
        got = _Proxy(none).soft(n, P, k, (1.0, 0.5), 0.5)
        assert ref['nv'] == 0 and (got['negsel'] == -1).all()
        _check_proxy(got, ref, n, P, k, (n, P, pattern, 'no valid row'))


def test_soft_proxy_ce_rejected_arguments_launch_nothing():
    Err = _err()
    n, P, big = 2, 8, PR.MAX_P + 1
    z = torch.ones(n * big, device='cuda')
    lab, pc = torch.zeros(n, dtype=torch.int64, device='cuda'), torch.zeros(big, dtype=torch.int32, device='cuda')
    loss, cor, dz, ws = _out(1), _out(1), _out(n * big), _out(3 * n)
    own, neg = _iout(n, torch.int64), _iout(n * P, torch.int32)

    def args(**kw):
        a = dict(z=z, ld=P, t=z, ldt=P, lab=lab, cam=lab, pcl=pc, pcm=pc, w=0.5, n=n, P=P, k=3, loss=loss, dz=dz, ldd=P, ws=ws)
        a.update(kw)
        return (a['z'], a['ld'], a['t'], a['ldt'], a['lab'], a['cam'], a['pcl'], a['pcm'], _f(a['w']), a['n'], a['P'], a['k'],
                _f(1.0), _f(0.5), a['loss'], cor, a['dz'], a['ldd'], own, neg, a['ws'])
    for kw in (dict(n=0), dict(P=0), dict(k=-1), dict(k=P + 1), dict(ld=P - 1), dict(ldd=P - 1), dict(z=None), dict(lab=None),
               dict(cam=None), dict(pcl=None), dict(pcm=None), dict(loss=None), dict(ws=None),
               dict(P=big, ld=big, ldt=big, ldd=big),
               dict(w=-0.5), dict(w=1.5), dict(w=float('nan')), dict(t=None), dict(ldt=P - 1)):
        with pytest.raises(Err, match='soft_proxy_ce'):
            _call('grl_soft_proxy_ce', *args(**kw))
    for t in (loss, cor, dz, ws):
        _untouched(t)
    assert (_igot(own, n) == ISENT).all() and (_igot(neg, n * P) == ISENT).all()
    _call('grl_soft_proxy_ce', *args(w=0.0, t=None, ldt=0))                     # served without a teacher
    torch.cuda.synchronize()
    assert abs(float(_got(loss, 1)[0]) - 1.5 * np.log(P)) < 1e-5                # equal logits, every proxy the rows' own pair


# ----------------------------------------------------------------------------------------------------------------------
# the loss modules
G = 0.75        # the gradient handed to the loss: (G * loss).backward()


def _run(crit, reset, x_host, args, **kw):
    reset(crit)
    x = torch.from_numpy(x_host).cuda().requires_grad_(True)
    loss, logits = crit(x, *args, **kw)
    (loss * G).backward()
    torch.cuda.synchronize()
    return loss.detach(), logits.detach(), x.grad, logits.grl_top1


@pytest.mark.parametrize('D', HR.LOSS_D)
def test_soft_hybrid_memory_loss_against_float64_and_its_backward_is_the_base_class(D):
    """hybrid_ref.in_loss (n = 9, N = 70 in interleaved classes, one target -1, one index -1) with teacher rows near the
    student's, w = 0.5: logits, loss and dx inside the end-to-end bounds, the top-1 count the student's; the teacher gets no
    gradient and is not written; the memory after the backward is HybridMemoryLoss's from the same state, bit for bit.  Without a
    teacher or with weight 0 the call is the base class's: every output the same bits."""
    from grl_amd.reid.loss import HybridMemoryLoss, SoftHybridMemoryLoss
    n, N, w = HR.LOSS_N, HR.LOSS_COLS, R.LOSS_W
    d = HR.in_loss(D, HR.loss_seed(D))
    teach = R.teacher_rows(d['x'], 'hybrid')
    tt = torch.from_numpy(teach).cuda()
    y, idx = torch.from_numpy(d['targets']).cuda(), torch.from_numpy(d['index']).cuda()

    def reset(c):
        c.reset(torch.from_numpy(d['mem']).cuda(), *(torch.from_numpy(d[k]).cuda() for k in ('cp', 'cm', 'ic')))
    soft = SoftHybridMemoryLoss(D, temp=HR.LOSS_TEMP, momentum=HR.LOSS_MOMENTUM).cuda()
    plain = HybridMemoryLoss(D, temp=HR.LOSS_TEMP, momentum=HR.LOSS_MOMENTUM).cuda()
    loss, logits, dx, top1 = _run(soft, reset, d['x'], (y, idx), teacher=tt, soft_weight=w)
    ref = R.hybrid_loss(d, teach, D, w, g=G)
    assert tuple(logits.shape) == (n, N) and not logits.requires_grad and top1[1] == n
    R.check('soft hybrid loss logits', _n(logits), ref['logits'], ref['b_logits'], D)
    R.check('soft hybrid loss', loss.item(), ref['loss'], ref['b_loss'], D)
    assert float(top1[0]) == ref['ce']['correct']
    assert not _n(dx)[4].any() and _n(dx)[7].any()
    R.check('soft hybrid loss dx', _n(dx), ref['dx'], HR.b_dx(ref['og'], N, ref['b_dz'], d['mem']), D)
    assert tt.grad is None and np.array_equal(_n(tt), teach)
    base = _run(plain, reset, d['x'], (y, idx))
    assert torch.equal(soft.memory, plain.memory) and not np.array_equal(_n(soft.memory), d['mem'])
    assert not torch.equal(dx, base[2])                                     # the soft target moved the gradient
    for kw in (dict(teacher=tt, soft_weight=0.0), dict(teacher=None, soft_weight=0.5), dict()):
        got = _run(soft, reset, d['x'], (y, idx), **kw)
        assert all(torch.equal(a, b) for a, b in zip(got[:3], base[:3])) and torch.equal(got[3][0], base[3][0]), kw
        assert torch.equal(soft.memory, plain.memory)
    with pytest.raises(ValueError, match='SoftHybridMemoryLoss: teacher must be on the device of the inputs'):
        soft(torch.from_numpy(d['x']).cuda(), y, idx, teacher=tt.cpu(), soft_weight=0.5)


@pytest.mark.parametrize('P,k,mode', ((3, 3, 'instance'), (70, 3, 'hard'), (70, 50, 'mean')))
def test_soft_proxy_memory_loss_against_float64_and_its_backward_is_the_base_class(P, k, mode):
    """proxy_ref.in_loss (n = 9, three cameras, one noise row, one pair without a proxy) under the selection-gap condition, with
    teacher rows near the student's, w = 0.5: as the hybrid test above, the memory update ``mode`` equal to ProxyMemoryLoss's"""
    from grl_amd.reid.loss import ProxyMemoryLoss, SoftProxyMemoryLoss
    n, D, w = PR.LOSS_N, PR.LOSS_D, R.LOSS_W
    d = PR.in_loss(P, k, R.proxy_loss_seed(P, k), 'soft')
    teach = R.teacher_rows(d['x'], 'proxy')
    tt = torch.from_numpy(teach).cuda()
    y, cam = torch.from_numpy(d['labels']).cuda(), torch.from_numpy(d['cams']).cuda()

    def reset(c):
        c.reset(torch.from_numpy(d['mem']).cuda(), torch.from_numpy(d['pcl']).cuda(), torch.from_numpy(d['pcm']).cuda())
    kw_crit = dict(temp=PR.LOSS_TEMP, momentum=PR.LOSS_MOMENTUM, mode=mode, k_neg=k, w_intra=PR.LOSS_W[0], w_inter=PR.LOSS_W[1])
    soft, plain = SoftProxyMemoryLoss(D, **kw_crit).cuda(), ProxyMemoryLoss(D, **kw_crit).cuda()
    loss, logits, dx, top1 = _run(soft, reset, d['x'], (y, cam), teacher=tt, soft_weight=w)
    ref = R.proxy_loss(d, teach, P, k, PR.LOSS_W, w, g=G)
    assert tuple(logits.shape) == (n, P) and not logits.requires_grad and top1[1] == n
    R.check('soft proxy loss logits', _n(logits), ref['logits'], ref['b_logits'], (P, k))
    R.check('soft proxy loss', loss.item(), ref['loss'], ref['b_loss'], (P, k))
    assert float(top1[0]) == ref['ce']['correct']
    assert not _n(dx)[4].any() and not _n(dx)[7].any()
    R.check('soft proxy loss dx', _n(dx), ref['dx'], PR.b_dx(ref['og'], P, ref['b_dz'], d['mem']), (P, k))
    assert tt.grad is None and np.array_equal(_n(tt), teach)
    base = _run(plain, reset, d['x'], (y, cam))
    assert torch.equal(soft.centroids, plain.centroids) and not np.array_equal(_n(soft.centroids), d['mem'])
    assert not torch.equal(dx, base[2])
    for kw in (dict(teacher=tt, soft_weight=0.0), dict(teacher=None, soft_weight=0.5), dict()):
        got = _run(soft, reset, d['x'], (y, cam), **kw)
        assert all(torch.equal(a, b) for a, b in zip(got[:3], base[:3])) and torch.equal(got[3][0], base[3][0]), kw
        assert torch.equal(soft.centroids, plain.centroids)


# ----------------------------------------------------------------------------------------------------------------------
# the trainers
class _IndexedClips(_Clips):
    """_Clips whose items end with their dataset index, as RawVideoDataset(index=True)"""

    def __getitem__(self, i):
        return _Clips.__getitem__(self, i) + (torch.tensor(i, dtype=torch.int64),)


def _iloader(tracklets, batch, order=None):
    ds = _IndexedClips(tracklets)
    return torch.utils.data.DataLoader(ds if order is None else torch.utils.data.Subset(ds, order), batch_size=batch, shuffle=False,
                                       drop_last=True)


def _make(synth_models, kind, soft_weight, tri_soft_weight=0.0, plain=False, k_neg=2):
    from grl_amd.reid.loss import HybridMemoryLoss, ProxyMemoryLoss, SoftHybridMemoryLoss, SoftProxyMemoryLoss, PairLoss
    from grl_amd.reid.train import (HybridSEQTrainer, CameraSEQTrainer, MeanTeacher, MeanTeacherHybridSEQTrainer,
                                    MeanTeacherCameraSEQTrainer)
    dev = torch.device('cuda:0')
    cnn, siam, siamv = (copy.deepcopy(m).to(dev) for m in synth_models)
    if kind == 'hybrid':
        cls = HybridMemoryLoss if plain else SoftHybridMemoryLoss
        crits = [cls(2048).to(dev) for _ in range(2)]
        base, mt = HybridSEQTrainer, MeanTeacherHybridSEQTrainer
    else:
        cls = ProxyMemoryLoss if plain else SoftProxyMemoryLoss
        crits = [cls(2048, k_neg=k_neg).to(dev) for _ in range(2)]
        base, mt = CameraSEQTrainer, MeanTeacherCameraSEQTrainer
    if plain:
        tr = base(cnn, siam, siamv, PairLoss().to(dev), crits[0], crits[1], None)
    else:
        tr = mt(cnn, siam, siamv, PairLoss().to(dev), crits[0], crits[1], None, teacher=MeanTeacher(cnn, siam, alpha=0.999),
                soft_weight=soft_weight, tri_soft_weight=tri_soft_weight)
    params = [p for m in (cnn, siam, siamv) for p in m.parameters()]
    return tr, torch.optim.SGD(params, lr=1e-3, momentum=0.9, weight_decay=5e-4, nesterov=True)


def _seeds(rows):
    g = torch.Generator().manual_seed(5)
    return [torch.nn.functional.normalize(torch.randn((rows, 2048), generator=g), dim=1) for _ in range(2)]


PCL, PCM = [0, 0, 1, 2, 2], [0, 1, 0, 0, 1]
CAM_TRACKLETS = [((40 + i,), (0, 0, 2, 2)[i], (0, 1, 1, 1)[i]) for i in range(4)]          # proxies 0, 1, 4


def _one_step(tr, opt, kind):
    """one B = 4, T = 2 step from a fixed state: test_gpu_hybrid.py's six instances in the classes {0, 3}, {1}, {2, 4}, {5} /
    test_gpu_proxy.py's five proxies over two cameras"""
    from grl_amd.reid.train.pseudo import PseudoLabels
    if kind == 'hybrid':
        seeds = _seeds(6)
        h = PseudoLabels(torch.tensor([0, -1, 1, 0, 1, -1], device='cuda')).hybrid()
        for crit, seed in ((tr.criterion_corr, seeds[0]), (tr.criterion_uncorr, seeds[1])):
            crit.reset(seed.clone().cuda(), h.class_ptr_dev, h.class_members_dev, h.inst_class_dev)
        loader = _iloader(h.relabel([((40 + i,), 900 + i, 0) for i in range(6)]), 4, order=[0, 3, 5, 5])
    else:
        seeds = _seeds(5)
        pcl, pcm = torch.tensor(PCL, dtype=torch.int32).cuda(), torch.tensor(PCM, dtype=torch.int32).cuda()
        tr.criterion_corr.reset(seeds[0].clone().cuda(), pcl, pcm)
        tr.criterion_uncorr.reset(seeds[1].clone().cuda(), pcl, pcm)
        loader = _loader(CAM_TRACKLETS, 4)
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(0, loader, opt)
    torch.cuda.synchronize()


def _memory(crit):
    return crit.memory if hasattr(crit, 'memory') else crit.centroids


@pytest.mark.parametrize('kind', ('hybrid', 'camera'))
def test_trainer_step_with_both_weights_zero_is_the_base_trainers_step_bit_for_bit(synth_models, kind):
    """soft_weight = 0 and tri_soft_weight = 0: no teacher pass; the loss, every parameter gradient, every parameter and both
    memories equal HybridSEQTrainer's / CameraSEQTrainer's with the hard criteria from the same state, bit for bit; the teacher
    is still updated behind the optimizer step"""
    outs = []
    for plain in (False, True):
        tr, opt = _make(synth_models, kind, 0.0, plain=plain)
        _one_step(tr, opt, kind)
        mods = (tr.model, tr.siamese_model, tr.siamese_model_uncorr)
        outs.append((tr.meters['loss'].avg, [(n, p.grad, p.detach()) for m in mods for n, p in m.named_parameters()],
                     _memory(tr.criterion_corr), _memory(tr.criterion_uncorr)))
        if not plain:
            assert tr.teacher.step == 1 and not opt._optimizer_step_post_hooks and tr._teacher_rows is None
    (la, pa, ca, ua), (lb, pb, cb, ub) = outs
    assert la == lb and np.isfinite(la) and len(pa) == len(pb) > 200
    with_grad = 0
    for (n1, g1, p1), (n2, g2, p2) in zip(pa, pb):
        assert n1 == n2 and (g1 is None) == (g2 is None) and torch.equal(p1, p2), n1
        if g1 is not None:
            assert torch.equal(g1, g2), n1
            with_grad += 1
    assert with_grad > 200 and torch.equal(ca, cb) and torch.equal(ua, ub)


@pytest.mark.parametrize('kind', ('hybrid', 'camera'))
def test_trainer_step_with_soft_targets_against_float64(synth_models, kind):
    """one step with soft_weight = 0.5 and tri_soft_weight = 0.5: the three identity losses and their logits inside the
    end-to-end bounds of the float64 model on the student rows, teacher rows, index / cams and memories the criteria were handed
    (k_neg admits every negative: the selection has no cut that float64 could place elsewhere); the teacher's rows carry no
    gradient; the teacher is updated once, in eval(), without a gradient"""
    tr, opt = _make(synth_models, kind, 0.5, tri_soft_weight=0.5, k_neg=50)
    seen = []

    def hook(mod, args, kwargs, out):
        s = dict(x=_n(args[0]).copy(), y=_n(args[1]).copy(), teacher=_n(kwargs['teacher']).copy(), w=kwargs['soft_weight'],
                 mem=_n(_memory(mod)).copy(), loss=out[0].detach(), top1=out[1].grl_top1[0], logits=out[1].detach(),
                 who='uncorr' if mod is tr.criterion_uncorr else 'corr', grad=kwargs['teacher'].requires_grad)
        s['extra'] = _n(kwargs['index' if kind == 'hybrid' else 'cams']).copy()
        if kind == 'hybrid':
            s.update(cp=_n(mod.class_ptr), cm=_n(mod.class_members), ic=_n(mod.inst_class))
        seen.append(s)
    handles = [c.register_forward_hook(hook, with_kwargs=True) for c in (tr.criterion_corr, tr.criterion_uncorr)]
    _one_step(tr, opt, kind)
    for h in handles:
        h.remove()
    assert sorted((s['who'], s['x'].shape[0]) for s in seen) == [('corr', 4), ('corr', 8), ('uncorr', 4)]
    for s in seen:
        n = s['x'].shape[0]
        assert s['w'] == 0.5 and not s['grad'] and s['teacher'].shape == s['x'].shape and not np.array_equal(s['teacher'], s['x'])
        if kind == 'hybrid':
            d = dict(x=s['x'], mem=s['mem'], targets=s['y'], cp=s['cp'], cm=s['cm'], ic=s['ic'], C=s['cp'].size - 1)
            assert s['extra'].tolist() == ([0, 5, 3, 5] if n == 4 else [0, 0, 3, 3, 5, 5, 5, 5])
            ref = R.hybrid_loss(d, s['teacher'], 2048, 0.5, temp=0.05)
        else:
            d = dict(x=s['x'], mem=s['mem'], labels=s['y'], cams=s['extra'], pcl=np.array(PCL, np.int32), pcm=np.array(PCM, np.int32))
            assert s['extra'].tolist() == ([0, 1, 1, 1] if n == 4 else [0, 0, 1, 1, 1, 1, 1, 1])
            ref = R.proxy_loss(d, s['teacher'], 5, 50, (1.0, 0.5), 0.5, temp=0.07)
        print('%s %s %d rows: loss %.9g (float64 %.9g, bound %.3g)' % (kind, s['who'], n, s['loss'].item(), ref['loss'], ref['b_loss']))
        R.check('trainer id logits', _n(s['logits']), ref['logits'], ref['b_logits'], (kind, s['who'], n))
        R.check('trainer id loss', s['loss'].item(), ref['loss'], ref['b_loss'], (kind, s['who'], n))
        assert ref['ce']['nv'] == n
    assert np.isfinite(tr.meters['loss'].avg)
    assert tr.teacher.step == 1 and not opt._optimizer_step_post_hooks
    assert all(not m.training for m in tr.teacher.models)
    assert all(p.grad is None and not p.requires_grad for m in tr.teacher.models for p in m.parameters())
    assert all(bool(torch.isfinite(p.grad).all()) for p in tr._all_params() if p.grad is not None)


@pytest.mark.parametrize('kind', ('hybrid', 'camera'))
def test_graphed_step_refuses_the_new_trainers(synth_models, kind):
    from grl_amd.train_graph import GraphedTrainStep
    tr, opt = _make(synth_models, kind, 0.5)
    with pytest.raises(ValueError, match='does not capture a MeanTeacher%sSEQTrainer' % ('Hybrid' if kind == 'hybrid' else 'Camera')):
        GraphedTrainStep(tr, opt, torch.zeros((4, 2, 3, 256, 128), device='cuda'), torch.zeros(4, dtype=torch.int64, device='cuda'))


@pytest.mark.parametrize('kind', ('hybrid', 'camera'))
def test_train_unsupervised_two_epochs_with_a_mean_teacher(synth_models, monkeypatch, kind):
    """8 synthetic tracklets over 2 cameras, a stub clustering with two noise rows, two epochs, clustering on the TEACHER's
    features: finite losses, teacher.step = the optimizer's steps, the hook gone from the optimizer, the memories seeded with the
    labels' tables"""
    from grl_amd.reid.evaluator import ATTEvaluator
    from grl_amd.reid.train import pseudo
    fixed = [0, 0, 1, 1, -1, 2, 2, -1]
    tracklets = [((60 + i,), 9000 + i, (0, 1, 0, 0, 1, 1, 0, 1)[i]) for i in range(8)]
    tr, opt = _make(synth_models, kind, 0.5, tri_soft_weight=0.5)
    ev = ATTEvaluator(*tr.teacher.models, only_eval=False)
    steps, feats, losses = [], [], []
    mine = opt.register_step_post_hook(lambda *_: steps.append(1))

    def stub(xf, **kw):
        feats.append(xf.clone())
        return pseudo.PseudoLabels(torch.tensor(fixed, device=xf.device), 'stub')
    monkeypatch.setattr(pseudo, 'pseudo_labels', stub)
    flags = dict(hybrid=True) if kind == 'hybrid' else dict(cameras=True, inter_from_epoch=1)
    with contextlib.redirect_stdout(io.StringIO()):
        hist = pseudo.train_unsupervised(tr, ev, opt, tracklets,
                                         lambda t: torch.utils.data.DataLoader(_Clips(t), batch_size=4, shuffle=False),
                                         (lambda t: _iloader(t, 4)) if kind == 'hybrid' else (lambda t: _loader(t, 4)), 2,
                                         on_epoch=lambda e, l: losses.append(tr.meters['loss'].avg), **flags)
    torch.cuda.synchronize()
    assert len(hist) == 2 and len(losses) == 2 and all(np.isfinite(v) for v in losses)
    want_steps = 4 if kind == 'hybrid' else 2                                 # hybrid: all 8 tracklets; cameras: the 6 clustered
    assert len(steps) == want_steps and tr.teacher.step == want_steps
    assert list(opt._optimizer_step_post_hooks) == [mine.id]                  # the trainer's hook is gone, the test's is left
    assert all(not m.training for m in tr.teacher.models)
    assert tuple(feats[0].shape) == (8, 6144) and not torch.equal(feats[0], feats[1])      # epoch 1 clustered the moved teacher
    for crit in (tr.criterion_corr, tr.criterion_uncorr):
        assert bool(torch.isfinite(_memory(crit)).all())
        if kind == 'hybrid':
            assert crit.num_instances == 8 and crit.inst_class.tolist() == [0, 0, 1, 1, 3, 2, 2, 4]
        else:
            assert crit.num_proxies == 5 and crit.inter_on
    for name, m in tr.meters.items():
        assert np.isfinite(float(m.avg)), name
