"""The soft softmax-triplet loss on a real MI355X: grl_soft_triplet_fwd / grl_soft_triplet_bwd
(grl_amd/csrc/soft_triplet.hip) through the C ABI, SoftTripletLoss, MeanTeacherSEQTrainer(tri_soft_weight=) steps and two
train_unsupervised epochs.

The student part (dist, sel, z) is compared BIT FOR BIT with grl_triplet_fwd; q, the loss and dfeat per element with the
float64 model of tests/soft_triplet_ref.py inside that element's derived bound -- never a norm over the tensor -- stage by
stage on the fp32 values the stage read, and for class (a) end to end with sel equal to the float64 selection under the gap
condition test_soft_triplet_cpu.py asserts.  With w_soft = 0 loss and dfeat are grl_triplet_fwd's / grl_triplet_bwd's bits.
Buffers, helpers and conventions are test_gpu_head_float64.py's and test_gpu_loss_float64.py's."""
import contextlib
import copy
import io

import numpy as np
import pytest
import torch

import soft_triplet_ref as S
from test_gpu_head_float64 import SENT, GUARD, _call, _n, _f, _out, _got, _Inputs, _err
from test_gpu_loss_float64 import ISENT, _Ints, _untouched
from test_gpu_cmem import _Clips, _loader

pytestmark = pytest.mark.gpu

ZERO = np.float32(0.0)


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    yield
    S.dump_ratios('MI355X soft triplet')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _isel(n):
    return torch.full((2 * n + GUARD,), ISENT, dtype=torch.int32, device='cuda')


def _sel_of(sel, n):
    torch.cuda.synchronize()
    a = _n(sel)
    assert (a[2 * n:] == ISENT).all(), 'written past the end of sel'
    return a[:2 * n].copy()


def _hard(f, ids, dloss, n, D):
    """grl_triplet_fwd + grl_triplet_bwd (soft = 1) into fresh sentinel buffers"""
    loss, dist, z, df, sel = _out(n), _out(n * n), _out(n), _out(n * D), _isel(n)
    _call('grl_triplet_fwd', f, ids, n, D, 1, _f(0.0), loss, dist, sel, z)
    _call('grl_triplet_bwd', f, dist, sel, z, dloss, 1, _f(0.0), df, n, D)
    return dict(loss=_got(loss, n).copy(), dist=_got(dist, n * n).reshape(n, n).copy(), z=_got(z, n).copy(), sel=_sel_of(sel, n),
                df=_got(df, n * D).reshape(n, D).copy())


def _soft(f, tf, ids, dloss, w, n, D, q=None):
    """grl_soft_triplet_fwd + grl_soft_triplet_bwd into fresh sentinel buffers; q: the buffer handed over as q (None: NULL)"""
    loss, dist, z, df, sel = _out(n), _out(n * n), _out(n), _out(n * D), _isel(n)
    _call('grl_soft_triplet_fwd', f, tf, ids, n, D, _f(w), loss, dist, sel, z, q)
    _call('grl_soft_triplet_bwd', f, dist, sel, z, q, dloss, _f(w), df, n, D)
    return dict(loss=_got(loss, n).copy(), dist=_got(dist, n * n).reshape(n, n).copy(), z=_got(z, n).copy(), sel=_sel_of(sel, n),
                df=_got(df, n * D).reshape(n, D).copy(), q=None if q is None or S.w_of(w) == 0 else _got(q, n).copy())


# ----------------------------------------------------------------------------------------------------------------------
# the kernels through the C ABI
@pytest.mark.parametrize('pattern', S.TRI_IDS)
@pytest.mark.parametrize('n,D', S.TRI_CASES)
def test_soft_triplet_fwd_and_bwd(n, D, pattern):
    """every class and w = 0.8, 1: dist, sel, z EQUAL grl_triplet_fwd's; q inside its bound of the float64 model at the
    kernel's own sel; the loss on the kernel's z and q; dfeat on the kernel's dist, sel, z, q; class (a): sel equals the float64
    selection, loss and dfeat end to end; the inputs unchanged, the same bits from a second run"""
    for cls in S.TRI_CLASSES:
        d = S.in_soft_triplet(n, D, cls, pattern)
        t, ids = _Inputs(f=d['f'], tf=d['tf'], dloss=d['dloss']), _Ints(d['ids'])
        hard = _hard(t['f'], ids.t, t['dloss'], n, D)
        for w in S.W_SOFT[1:]:
            what = (n, D, pattern, cls, w)
            got = _soft(t['f'], t['tf'], ids.t, t['dloss'], w, n, D, q=_out(n))
            for k in ('dist', 'sel', 'z'):
                assert np.array_equal(got[k].view(np.uint32) if got[k].dtype == np.float32 else got[k],
                                      hard[k].view(np.uint32) if hard[k].dtype == np.float32 else hard[k]), (k, what)
            assert ((got['q'] >= 0) & (got['q'] <= 1)).all(), what
            assert got['z'].max() < 80                # expf(z) in the backward stays finite
            m = S.check_stagewise(got, d, w, n, D, what)
            print('soft triplet %r: q %s loss %s' % (what, np.array2string(got['q'], precision=4), np.array2string(got['loss'], precision=6)))
            if cls == 'a':
                assert S.check_end_to_end(got, d, w, n, D, what)
            if m['same_n'].any():                     # no different-id negative: the mirrored mask gives q = 0 exactly
                assert not _bits(got['q'][m['same_n']]).any(), what
            again = _soft(t['f'], t['tf'], ids.t, t['dloss'], w, n, D, q=_out(n))
            for k in ('loss', 'q', 'df'):
                assert np.array_equal(_bits(got[k]), _bits(again[k])), (k, what)
        t.unchanged(); ids.unchanged()


@pytest.mark.parametrize('pattern', S.TRI_IDS)
@pytest.mark.parametrize('n,D', S.TRI_CASES)
def test_weight_zero_is_the_hard_triplet_bit_for_bit(n, D, pattern):
    """w_soft = 0 with tfeat and q NULL, and with a NaN tfeat and a sentinel q buffer: loss and dfeat are grl_triplet_fwd's and
    grl_triplet_bwd's bits, the q buffer is untouched"""
    for cls in S.TRI_CLASSES:
        d = S.in_soft_triplet(n, D, cls, pattern)
        t, ids = _Inputs(f=d['f'], dloss=d['dloss']), _Ints(d['ids'])
        hard = _hard(t['f'], ids.t, t['dloss'], n, D)
        garbage = torch.full((n * D,), float('nan'), device='cuda')
        for tf, q in ((None, None), (garbage, _out(n))):
            got = _soft(t['f'], tf, ids.t, t['dloss'], 0.0, n, D, q=q)
            for k in ('loss', 'dist', 'z', 'df'):
                assert np.array_equal(_bits(got[k]), _bits(hard[k])), (k, n, D, pattern, cls, tf is None)
            assert np.array_equal(got['sel'], hard['sel'])
            if q is not None:
                _untouched(q)
        t.unchanged(); ids.unchanged()


def test_rejected_arguments_launch_nothing():
    Err = _err()
    n, D = 2, 8
    a = torch.ones(64, device='cuda')
    li = torch.zeros(8, dtype=torch.int64, device='cuda')
    si = torch.full((64,), ISENT, dtype=torch.int32, device='cuda')
    o = [_out(64) for _ in range(5)]
    good = dict(feat=a, tfeat=a, ids=li, n=n, D=D, w=0.8, loss=o[0], dist=o[1], sel=si, z=o[2], q=o[3])
    for kw in (dict(D=6), dict(n=0), dict(n=16385), dict(w=-0.5), dict(w=1.5), dict(w=float('nan')), dict(tfeat=None), dict(q=None),
               dict(tfeat=None, w=1.0), dict(feat=None), dict(ids=None), dict(loss=None), dict(dist=None), dict(sel=None), dict(z=None)):
        g = dict(good, **kw)
        with pytest.raises(Err, match='soft_triplet_fwd'):
            _call('grl_soft_triplet_fwd', g['feat'], g['tfeat'], g['ids'], g['n'], g['D'], _f(g['w']), g['loss'], g['dist'], g['sel'],
                  g['z'], g['q'])
    goodb = dict(feat=a, dist=a, sel=si, z=a, q=a, dloss=a, w=0.8, dfeat=o[4], n=n, D=D)
    for kw in (dict(D=6), dict(n=0), dict(w=-0.5), dict(w=1.5), dict(w=float('nan')), dict(q=None), dict(feat=None), dict(dfeat=None)):
        g = dict(goodb, **kw)
        with pytest.raises(Err, match='soft_triplet_bwd'):
            _call('grl_soft_triplet_bwd', g['feat'], g['dist'], g['sel'], g['z'], g['q'], g['dloss'], _f(g['w']), g['dfeat'], g['n'], g['D'])
    for buf in o:
        _untouched(buf)
    torch.cuda.synchronize()
    assert (_n(a) == 1.0).all() and (_n(si) == ISENT).all() and (_n(li) == 0).all()
    # ... and the neighbouring good arguments are accepted: n = 2 equal rows of one id, D = 4
    _call('grl_soft_triplet_fwd', a, a, li, 2, 4, _f(1.0), o[0], o[1], si, o[2], o[3])
    torch.cuda.synchronize()
    assert (_n(o[0])[:2] != SENT).all() and (_n(o[0])[2:] == SENT).all() and (_n(o[3])[:2] == 0).all() and (_n(o[3])[2:] == SENT).all()
    assert (_n(si)[:4] != ISENT).all() and (_n(si)[4:] == ISENT).all()


# ----------------------------------------------------------------------------------------------------------------------
# SoftTripletLoss
def test_soft_triplet_loss_autograd_against_float64():
    """n = 4, D = 2048, w = 0.8: the module's loss and gradient are the C calls' bits and lie inside the end-to-end bounds of
    the float64 model; the gradient reaches feat only; teacher = None and soft_weight = 0 are TripletLoss('soft', True)"""
    from grl_amd.reid.loss import SoftTripletLoss, TripletLoss
    n, D, w = 4, 2048, 0.8
    d = S.in_soft_triplet(n, D, 'a', 'pairs')
    crit = SoftTripletLoss()
    x = torch.from_numpy(d['f']).cuda().requires_grad_(True)
    y, tt, dl = torch.from_numpy(d['ids']).cuda(), torch.from_numpy(d['tf']).cuda(), torch.from_numpy(d['dloss']).cuda()
    loss = crit(x, y, teacher=tt, soft_weight=w)
    assert tuple(loss.shape) == (n,)
    (loss * dl).sum().backward()
    torch.cuda.synchronize()
    assert tt.grad is None and not tt.requires_grad and np.array_equal(_n(tt), d['tf'])
    direct = _soft(x.detach(), tt, y, dl, w, n, D, q=_out(n))
    assert np.array_equal(_bits(_n(loss)), _bits(direct['loss'])) and np.array_equal(_bits(_n(x.grad)), _bits(direct['df']))
    got = dict(direct, loss=_n(loss), df=_n(x.grad))
    S.check_stagewise(got, d, w, n, D, 'module')
    assert S.check_end_to_end(got, d, w, n, D, 'module')
    hard_crit = TripletLoss('soft', True)
    x0 = torch.from_numpy(d['f']).cuda().requires_grad_(True)
    l0 = hard_crit(x0, y)
    (l0 * dl).sum().backward()
    assert not torch.equal(l0, loss.detach()) and not torch.equal(x0.grad, x.grad)        # the soft target moved both
    for kw in (dict(teacher=None, soft_weight=0.8), dict(teacher=tt, soft_weight=0.0), dict()):
        xi = torch.from_numpy(d['f']).cuda().requires_grad_(True)
        li = crit(xi, y, **kw)
        (li * dl).sum().backward()
        torch.cuda.synchronize()
        assert torch.equal(li, l0) and torch.equal(xi.grad, x0.grad), kw
    with pytest.raises(ValueError, match='SoftTripletLoss: teacher must be on the device of the inputs'):
        crit(x, y, teacher=tt.cpu(), soft_weight=0.5)


# ----------------------------------------------------------------------------------------------------------------------
# the trainer (the fixtures of test_gpu_teacher.py, with the new argument)
K3 = 3
TRACKLETS4 = [((40 + i,), (0, 0, 2, 2)[i], i % 2) for i in range(4)]


def _mt_trainer(synth_models, K, soft_weight, **extra):
    from grl_amd.reid.loss import SoftClusterMemoryLoss, PairLoss
    from grl_amd.reid.train import MeanTeacher, MeanTeacherSEQTrainer
    dev = torch.device('cuda:0')
    cnn, siam, siamv = (copy.deepcopy(m).to(dev) for m in synth_models)
    crit_c, crit_u = SoftClusterMemoryLoss(2048, K).to(dev), SoftClusterMemoryLoss(2048, K).to(dev)
    tr = MeanTeacherSEQTrainer(cnn, siam, siamv, PairLoss().to(dev), crit_c, crit_u, None,
                               teacher=MeanTeacher(cnn, siam, alpha=0.999), soft_weight=soft_weight, **extra)
    params = [p for m in (cnn, siam, siamv) for p in m.parameters()]
    opt = torch.optim.SGD(params, lr=1e-3, momentum=0.9, weight_decay=5e-4, nesterov=True)
    return tr, opt


def _one_step(tr, opt):
    g = torch.Generator().manual_seed(5)
    seeds = [torch.nn.functional.normalize(torch.randn((K3, 2048), generator=g), dim=1) for _ in range(2)]
    tr.criterion_corr.reset(seeds[0].clone().cuda())
    tr.criterion_uncorr.reset(seeds[1].clone().cuda())
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(0, _loader(TRACKLETS4, 4), opt)
    torch.cuda.synchronize()


def test_trainer_step_with_tri_soft_weight_zero_is_the_step_without_the_argument(synth_models):
    """B = 4, T = 2, K = 3, soft_weight = 0.5: tri_soft_weight = 0 against the trainer constructed without the argument -- the
    loss, every gradient, every parameter and both memories, bit for bit"""
    outs = []
    for extra in (dict(tri_soft_weight=0.0), dict()):
        tr, opt = _mt_trainer(synth_models, K3, 0.5, **extra)
        assert tr.tri_soft_weight == 0.0
        _one_step(tr, opt)
        mods = (tr.model, tr.siamese_model, tr.siamese_model_uncorr)
        outs.append((tr.meters['loss'].avg, [(n, p.grad, p.detach()) for m in mods for n, p in m.named_parameters()],
                     tr.criterion_corr.centroids, tr.criterion_uncorr.centroids))
        assert tr.teacher.step == 1
    (la, pa, ca, ua), (lb, pb, cb, ub) = outs
    assert la == lb and np.isfinite(la)
    assert len(pa) == len(pb) > 200
    with_grad = 0
    for (n1, g1, p1), (n2, g2, p2) in zip(pa, pb):
        assert n1 == n2 and (g1 is None) == (g2 is None) and torch.equal(p1, p2), n1
        if g1 is not None:
            assert torch.equal(g1, g2), n1
            with_grad += 1
    assert with_grad > 200
    assert torch.equal(ca, cb) and torch.equal(ua, ub)


def test_trainer_step_with_a_soft_triplet(synth_models, monkeypatch):
    """one step with tri_soft_weight = 0.8 and the module-level hard criterion replaced by a stub that raises: the owned
    SoftTripletLoss is called once with the 4 clip rows and the teacher's ('corr', 'clip') rows (no gradient, not the student's),
    its output is the C call's bits on the captured rows and lies inside the bounds of the float64 model; the loss is finite and
    the teacher advanced"""
    from grl_amd.reid.train import trainer as T

    def hard(*a, **k):
        raise AssertionError('the hard triplet criterion was called')
    monkeypatch.setattr(T, 'criterion_triplet', hard)
    tr, opt = _mt_trainer(synth_models, K3, 0.5, tri_soft_weight=0.8)
    seen = []

    def hook(mod, args, kwargs, out):
        seen.append(dict(x=_n(args[0]).copy(), y=_n(args[1]).copy(), teacher=_n(kwargs['teacher']).copy(), w=kwargs['soft_weight'],
                         grad=kwargs['teacher'].requires_grad, loss=_n(out).copy()))
    h = tr.criterion_soft_triplet.register_forward_hook(hook, with_kwargs=True)
    _one_step(tr, opt)
    h.remove()
    assert len(seen) == 1
    s = seen[0]
    n, D = s['x'].shape
    assert (n, D) == (4, 2048) and s['w'] == 0.8 and not s['grad'] and s['teacher'].shape == s['x'].shape
    assert not np.array_equal(s['teacher'], s['x'])
    d = dict(f=s['x'], tf=s['teacher'], ids=s['y'], dloss=np.full(n, 1.0 / n, np.float32))
    t, ids = _Inputs(f=d['f'], tf=d['tf'], dloss=d['dloss']), _Ints(d['ids'])
    direct = _soft(t['f'], t['tf'], ids.t, t['dloss'], 0.8, n, D, q=_out(n))
    assert np.array_equal(_bits(s['loss']), _bits(direct['loss']))
    print('trainer soft triplet: ids %s q %s loss %s' % (s['y'], direct['q'], direct['loss']))
    if not S.check_end_to_end(direct, d, 0.8, n, D, 'trainer', require_gap=False):        # at the float64 selection, or ...
        S.check_stagewise(direct, d, 0.8, n, D, 'trainer')                                 # ... at the kernel's own
    assert np.isfinite(tr.meters['loss'].avg)
    assert tr.teacher.step == 1 and not opt._optimizer_step_post_hooks


def test_train_unsupervised_two_epochs_with_both_soft_weights(synth_models, monkeypatch):
    """8 planted tracklets, a stub clustering with two noise rows, two epochs with soft_weight = 0.5 and tri_soft_weight = 0.8:
    finite losses, teacher.step = the optimizer's steps"""
    from grl_amd.reid.evaluator import ATTEvaluator
    from grl_amd.reid.train import pseudo
    fixed = [0, 0, 1, 1, -1, 2, 2, -1]
    tracklets = [((60 + i,), 9000 + i, i % 2) for i in range(8)]
    tr, opt = _mt_trainer(synth_models, 5, 0.5, tri_soft_weight=0.8)
    ev = ATTEvaluator(*tr.teacher.models, only_eval=False)
    steps, calls = [], []
    opt.register_step_post_hook(lambda *_: steps.append(1))
    h = tr.criterion_soft_triplet.register_forward_hook(lambda mod, args, out: calls.append(bool(torch.isfinite(out).all())))
    monkeypatch.setattr(pseudo, 'pseudo_labels', lambda xf, **kw: pseudo.PseudoLabels(torch.tensor(fixed, device=xf.device), 'stub'))
    losses = []
    with contextlib.redirect_stdout(io.StringIO()):
        hist = pseudo.train_unsupervised(tr, ev, opt, tracklets,
                                         lambda t: torch.utils.data.DataLoader(_Clips(t), batch_size=4, shuffle=False),
                                         lambda t: _loader(t, 4), 2, on_epoch=lambda e, l: losses.append(tr.meters['loss'].avg))
    torch.cuda.synchronize()
    h.remove()
    assert len(hist) == 2 and len(losses) == 2 and all(np.isfinite(v) for v in losses)
    assert len(steps) == 2 and tr.teacher.step == len(steps)
    assert len(calls) == len(steps) and all(calls)
