"""The instance-contrast terms on a real MI355X: grl_ins_contrast_fwd / grl_ins_contrast_bwd
(grl_amd/csrc/ins_contrast.hip) through the C ABI, InstanceContrastLoss, the three mean-teacher trainers with
ins_hard_weight / ins_soft_weight, and two train_unsupervised epochs.

cos is compared per element with the float64 cosines inside that element's derived bound (tests/ins_contrast_ref.py) -- never
a norm over the tensor; sel must EQUAL the fp32 restatement of the selection applied to the kernel's own cos; loss, coef and
dfeat are compared with the float64 model evaluated at the kernel's sel and cos (stage by stage), and for class (a), whose
inputs meet the gap condition test_ins_contrast_cpu.py asserts, end to end from the rows alone with sel equal to the float64
selection.  Buffers, helpers and conventions are test_gpu_head_float64.py's and test_gpu_loss_float64.py's."""
import contextlib
import copy
import io

import numpy as np
import pytest
import torch

import ins_contrast_ref as S
from test_gpu_head_float64 import SENT, GUARD, _call, _n, _f, _out, _got, _Inputs, _err
from test_gpu_loss_float64 import ISENT, _Ints, _untouched
from test_gpu_cmem import _Clips, _loader
import test_gpu_soft_memory as SM
import test_gpu_soft_triplet as ST

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    yield
    S.dump_ratios('MI355X instance contrast')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _isel(n):
    return torch.full((n * n + GUARD,), ISENT, dtype=torch.int32, device='cuda')


def _sel_of(sel, n):
    torch.cuda.synchronize()
    a = _n(sel)
    assert (a[n * n:] == ISENT).all(), 'written past the end of sel'
    return a[:n * n].reshape(n, n).copy()


def _run(f, m, ids, dloss, tau, tau_t, wh, ws, n, D):
    """grl_ins_contrast_fwd + grl_ins_contrast_bwd into fresh sentinel buffers"""
    loss, cos, coef, df, sel = _out(n), _out(n * n), _out(n * n), _out(n * D), _isel(n)
    _call('grl_ins_contrast_fwd', f, m, ids, n, D, _f(tau), _f(tau_t), _f(wh), _f(ws), loss, cos, sel, coef)
    _call('grl_ins_contrast_bwd', f, m, coef, dloss, _f(tau), df, n, D)
    return dict(loss=_got(loss, n).copy(), cos=_got(cos, n * n).reshape(n, n).copy(), coef=_got(coef, n * n).reshape(n, n).copy(),
                sel=_sel_of(sel, n), df=_got(df, n * D).reshape(n, D).copy())


# ----------------------------------------------------------------------------------------------------------------------
# the kernels through the C ABI
@pytest.mark.parametrize('wide', S.WIDE)
@pytest.mark.parametrize('n,D,pattern', S.CASES)
def test_ins_contrast_fwd_and_bwd(n, D, pattern, wide):
    """every class, weight pair and temperature pair: cos, sel, loss, coef, sum coef and dfeat stage by stage; class (a) end to
    end; the one-id batch exactly 0; the zero student row finite with a zero gradient; inputs unchanged, nothing written past a
    buffer, the same bits from a second run"""
    for cls in S.CLASSES:
        d = S.in_ins(n, D, cls, pattern, wide)
        t, ids = _Inputs(f=d['f'], m=d['m'], dloss=d['dloss']), _Ints(d['ids'])
        for tau, tau_t in S.TAUS:
            for wh, ws in S.WEIGHTS:
                what = (n, D, pattern, wide, cls, tau, tau_t, wh, ws)
                got = _run(t['f'], t['m'], ids.t, t['dloss'], tau, tau_t, wh, ws, n, D)
                assert set(np.unique(got['sel']).tolist()) <= {0, 1, 2} and ((got['sel'] == 2).sum(1) == 1).all(), what
                assert ((got['sel'] > 0).sum(1) == len(set(d['ids'].tolist()))).all(), what
                S.check_stagewise(got, d, tau, tau_t, wh, ws, n, D, what)
                if cls == 'a':
                    S.check_end_to_end(got, d, tau, tau_t, wh, ws, n, D, what)
                if cls == 'z':
                    assert not _bits(got['cos'][0]).any() and not got['df'][0].any() and np.isfinite(got['loss'][0]), what
                    assert got['sel'][0].tolist() == S.select(np.zeros((n, n)), d['ids'])[0].tolist(), what
                if pattern == 'one':
                    assert not got['loss'].any() and not got['coef'].any() and not got['df'].any(), what
                if pattern == 'two':
                    assert np.array_equal(got['sel'] == 2, np.eye(n, dtype=bool)), what
                again = _run(t['f'], t['m'], ids.t, t['dloss'], tau, tau_t, wh, ws, n, D)
                for k in ('loss', 'cos', 'coef', 'df'):
                    assert np.array_equal(_bits(got[k]), _bits(again[k])), (k, what)
                assert np.array_equal(got['sel'], again['sel']), what
        t.unchanged(); ids.unchanged()
    print('ins contrast %r: loss %s' % ((n, D, pattern, wide), np.array2string(got['loss'][:6], precision=6)))


def test_tied_columns_go_to_the_lower_index():
    """class (t), pairs: student rows 0 and 1 are bit-identical (their cos rows are), teacher rows 2 and 3 are (columns 2 and 3
    are, inside one id): column 3 is never selected, and rows 0 and 1 of sel differ only where the anchor's own id differs"""
    n, D = 130, 4
    d = S.in_ins(n, D, 't', 'pairs')
    t, ids = _Inputs(f=d['f'], m=d['m'], dloss=d['dloss']), _Ints(d['ids'])
    got = _run(t['f'], t['m'], ids.t, t['dloss'], 0.1, 0.1, 1.0, 0.4, n, D)
    assert np.array_equal(_bits(got['cos'][0]), _bits(got['cos'][1])) and np.array_equal(_bits(got['cos'][:, 2]), _bits(got['cos'][:, 3]))
    assert (got['sel'][:, 3] == 0).all() and (got['sel'][:, 2] > 0).all()
    assert np.array_equal(got['sel'][0], got['sel'][1])                    # rows 0 and 1 share their id as well
    assert np.array_equal(_bits(got['cos'][:, 0]), _bits(got['cos'][:, n - 1]))         # equal columns of two ids: no tie to rule


def test_the_cap_is_accepted_and_selection_at_1024_finishes():
    """n = 1024 (4 column trips per lane, 512 ids) and n = 2048, the cap, at D = 4: sel equals the restatement on the kernel's
    cos, loss and coef stage-wise"""
    for n in (1024, S.MAX_N):
        D = 4
        d = S.in_ins(n, D, 'a', 'pairs')
        t, ids = _Inputs(f=d['f'], m=d['m'], dloss=d['dloss']), _Ints(d['ids'])
        got = _run(t['f'], t['m'], ids.t, t['dloss'], 0.1, 0.1, 1.0, 0.4, n, D)
        S.check_stagewise(got, d, 0.1, 0.1, 1.0, 0.4, n, D, ('cap', n))
        t.unchanged(); ids.unchanged()


def test_rejected_arguments_launch_nothing():
    Err = _err()
    n, D = 2, 8
    a = torch.ones(64, device='cuda')
    li = torch.zeros(8, dtype=torch.int64, device='cuda')
    si = torch.full((64,), ISENT, dtype=torch.int32, device='cuda')
    o = [_out(64) for _ in range(4)]
    inf, nan = float('inf'), float('nan')
    good = dict(feat=a, tfeat=a, ids=li, n=n, D=D, tau=0.1, tau_t=0.1, wh=1.0, ws=0.4, loss=o[0], cos=o[1], sel=si, coef=o[2])
    for kw in (dict(D=6), dict(D=0), dict(D=2), dict(n=0), dict(n=-3), dict(n=S.MAX_N + 1), dict(tau=0.0), dict(tau=-1.0), dict(tau=inf),
               dict(tau=nan), dict(tau_t=0.0), dict(tau_t=nan), dict(tau_t=inf), dict(wh=-1.0), dict(ws=-0.4), dict(wh=nan),
               dict(wh=0.0, ws=0.0), dict(feat=None), dict(tfeat=None), dict(ids=None), dict(loss=None), dict(cos=None), dict(sel=None),
               dict(coef=None)):
        g = dict(good, **kw)
        with pytest.raises(Err, match='ins_contrast_fwd'):
            _call('grl_ins_contrast_fwd', g['feat'], g['tfeat'], g['ids'], g['n'], g['D'], _f(g['tau']), _f(g['tau_t']), _f(g['wh']),
                  _f(g['ws']), g['loss'], g['cos'], g['sel'], g['coef'])
    goodb = dict(feat=a, tfeat=a, coef=a, dloss=a, tau=0.1, dfeat=o[3], n=n, D=D)
    for kw in (dict(D=6), dict(D=0), dict(n=0), dict(n=S.MAX_N + 1), dict(tau=0.0), dict(tau=nan), dict(tau=inf), dict(feat=None),
               dict(tfeat=None), dict(coef=None), dict(dloss=None), dict(dfeat=None)):
        g = dict(goodb, **kw)
        with pytest.raises(Err, match='ins_contrast_bwd'):
            _call('grl_ins_contrast_bwd', g['feat'], g['tfeat'], g['coef'], g['dloss'], _f(g['tau']), g['dfeat'], g['n'], g['D'])
    for buf in o:
        _untouched(buf)
    torch.cuda.synchronize()
    assert (_n(a) == 1.0).all() and (_n(si) == ISENT).all() and (_n(li) == 0).all()
    # ... and the neighbouring good arguments are accepted: n = 2 equal rows of one id, D = 4: loss and coef exactly 0
    _call('grl_ins_contrast_fwd', a, a, li, 2, 4, _f(0.1), _f(0.1), _f(1.0), _f(0.4), o[0], o[1], si, o[2])
    torch.cuda.synchronize()
    assert (_n(o[0])[:2] == 0).all() and (_n(o[0])[2:] == SENT).all() and (_n(o[2])[:4] == 0).all() and (_n(o[2])[4:] == SENT).all()
    assert _n(si)[:4].tolist() == [2, 0, 2, 0] and (_n(si)[4:] == ISENT).all() and (_n(o[1])[4:] == SENT).all()


# ----------------------------------------------------------------------------------------------------------------------
# InstanceContrastLoss
def test_instance_contrast_loss_autograd_is_the_c_calls():
    """n = 8, D = 2048, weights (1, 0.4), tau 0.05 / teacher_tau 0.1: the module's loss and gradient are the C calls' bits and
    lie inside the end-to-end bounds of the float64 model; the gradient reaches feat only"""
    from grl_amd.reid.loss import InstanceContrastLoss
    n, D, tau, tau_t, wh, ws = 8, 2048, 0.05, 0.1, 1.0, 0.4
    d = S.in_ins(n, D, 'a', 'x4')
    crit = InstanceContrastLoss(tau=tau, teacher_tau=tau_t)
    x = torch.from_numpy(d['f']).cuda().requires_grad_(True)
    y, tt, dl = torch.from_numpy(d['ids']).cuda(), torch.from_numpy(d['m']).cuda(), torch.from_numpy(d['dloss']).cuda()
    loss = crit(x, y, teacher=tt, hard_weight=wh, soft_weight=ws)
    assert tuple(loss.shape) == (n,)
    (loss * dl).sum().backward()
    torch.cuda.synchronize()
    assert tt.grad is None and not tt.requires_grad and np.array_equal(_n(tt), d['m'])
    direct = _run(x.detach(), tt, y, dl, tau, tau_t, wh, ws, n, D)
    assert np.array_equal(_bits(_n(loss)), _bits(direct['loss'])) and np.array_equal(_bits(_n(x.grad)), _bits(direct['df']))
    S.check_end_to_end(direct, d, tau, tau_t, wh, ws, n, D, 'module')
    l2 = InstanceContrastLoss(tau=tau)(x.detach(), y, teacher=tt)          # the defaults: the hard term alone, teacher_tau = tau
    hard = _run(x.detach(), tt, y, dl, tau, tau, 1.0, 0.0, n, D)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(_n(l2)), _bits(hard['loss'])) and not np.array_equal(_bits(_n(l2)), _bits(_n(loss)))
    with pytest.raises(ValueError, match='InstanceContrastLoss: teacher must be on the device of the inputs'):
        crit(x, y, teacher=tt.cpu())


# ----------------------------------------------------------------------------------------------------------------------
# the trainers (the fixtures of test_gpu_soft_triplet.py and test_gpu_soft_memory.py, with the new arguments)
KINDS = ('cluster', 'hybrid', 'camera')


def _make(synth_models, kind, **extra):
    from grl_amd.reid.loss import SoftHybridMemoryLoss, SoftProxyMemoryLoss, PairLoss
    from grl_amd.reid.train import MeanTeacher, MeanTeacherHybridSEQTrainer, MeanTeacherCameraSEQTrainer
    if kind == 'cluster':
        return ST._mt_trainer(synth_models, ST.K3, 0.5, **extra)
    dev = torch.device('cuda:0')
    cnn, siam, siamv = (copy.deepcopy(m).to(dev) for m in synth_models)
    if kind == 'hybrid':
        crits, cls = [SoftHybridMemoryLoss(2048).to(dev) for _ in range(2)], MeanTeacherHybridSEQTrainer
    else:
        crits, cls = [SoftProxyMemoryLoss(2048, k_neg=2).to(dev) for _ in range(2)], MeanTeacherCameraSEQTrainer
    tr = cls(cnn, siam, siamv, PairLoss().to(dev), crits[0], crits[1], None, teacher=MeanTeacher(cnn, siam, alpha=0.999),
             soft_weight=0.5, **extra)
    params = [p for m in (cnn, siam, siamv) for p in m.parameters()]
    return tr, torch.optim.SGD(params, lr=1e-3, momentum=0.9, weight_decay=5e-4, nesterov=True)


def _step(tr, opt, kind):
    if kind == 'cluster':
        ST._one_step(tr, opt)
    else:
        SM._one_step(tr, opt, kind)


def _count_calls(monkeypatch):
    """a wrapper around the module's _call that counts the entry points by name"""
    from grl_amd.reid.loss import ins_contrast
    seen, real = [], ins_contrast._call

    def counting(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(ins_contrast, '_call', counting)
    return seen


def _state(tr):
    mods = (tr.model, tr.siamese_model, tr.siamese_model_uncorr)
    return (tr.meters['loss'].avg, [(n, p.grad, p.detach().clone()) for m in mods for n, p in m.named_parameters()],
            SM._memory(tr.criterion_corr).clone(), SM._memory(tr.criterion_uncorr).clone())


@pytest.mark.parametrize('kind', KINDS)
def test_trainer_step_with_instance_weights_zero_is_the_step_without_the_arguments(synth_models, monkeypatch, kind):
    """ins_hard_weight = ins_soft_weight = 0 against the trainer constructed without the arguments: the loss, every gradient,
    every parameter and both memories bit for bit, and no grl_ins_contrast_* call"""
    seen = _count_calls(monkeypatch)
    outs = []
    for extra in (dict(ins_hard_weight=0.0, ins_soft_weight=0.0, ins_tau=0.05, ins_teacher_tau=0.2), dict()):
        tr, opt = _make(synth_models, kind, **extra)
        assert tr.ins_hard_weight == 0.0 and tr.ins_soft_weight == 0.0
        _step(tr, opt, kind)
        outs.append(_state(tr))
        assert tr.teacher.step == 1
    assert not seen
    (la, pa, ca, ua), (lb, pb, cb, ub) = outs
    assert la == lb and np.isfinite(la) and len(pa) == len(pb) > 200
    with_grad = 0
    for (n1, g1, p1), (n2, g2, p2) in zip(pa, pb):
        assert n1 == n2 and (g1 is None) == (g2 is None) and torch.equal(p1, p2), n1
        if g1 is not None:
            assert torch.equal(g1, g2), n1
            with_grad += 1
    assert with_grad > 200 and torch.equal(ca, cb) and torch.equal(ua, ub)


@pytest.mark.parametrize('kind', KINDS)
def test_two_trainer_steps_with_the_instance_terms(synth_models, monkeypatch, kind):
    """two steps with weights (1, 0.4): the owned InstanceContrastLoss is called once per step with the 4 clip rows and the
    teacher's ('corr', 'clip') rows (no gradient, not the student's), its output is the C calls' bits on the captured rows; the
    losses are finite, the parameters move, the term changes the step"""
    seen = _count_calls(monkeypatch)
    tr, opt = _make(synth_models, kind, ins_hard_weight=1.0, ins_soft_weight=0.4, ins_tau=0.05, ins_teacher_tau=0.1)
    before = [p.detach().clone() for p in tr._all_params()]
    caught = []

    def hook(mod, args, kwargs, out):
        caught.append(dict(x=_n(args[0]).copy(), y=_n(args[1]).copy(), teacher=_n(kwargs['teacher']).copy(), grad=kwargs['teacher'].requires_grad,
                           w=(kwargs['hard_weight'], kwargs['soft_weight']), loss=_n(out).copy()))
    h = tr.criterion_ins.register_forward_hook(hook, with_kwargs=True)
    losses = []
    for _ in range(2):
        _step(tr, opt, kind)
        losses.append(tr.meters['loss'].avg)
    h.remove()
    assert seen == ['grl_ins_contrast_fwd', 'grl_ins_contrast_bwd'] * 2 and len(caught) == 2
    assert all(np.isfinite(v) for v in losses) and tr.teacher.step == 2
    moved = sum(int(not torch.equal(a, p.detach())) for a, p in zip(before, tr._all_params()))
    assert moved > 200
    assert all(bool(torch.isfinite(p.grad).all()) for p in tr._all_params() if p.grad is not None)
    for s in caught:
        n, D = s['x'].shape
        assert (n, D) == (4, 2048) and s['w'] == (1.0, 0.4) and not s['grad'] and not np.array_equal(s['teacher'], s['x'])
        d = dict(f=s['x'], m=s['teacher'], ids=s['y'], dloss=np.full(n, 1.0 / n, np.float32))
        t, ids = _Inputs(f=d['f'], m=d['m'], dloss=d['dloss']), _Ints(d['ids'])
        direct = _run(t['f'], t['m'], ids.t, t['dloss'], 0.05, 0.1, 1.0, 0.4, n, D)
        assert np.array_equal(_bits(s['loss']), _bits(direct['loss']))
        S.check_stagewise(direct, d, 0.05, 0.1, 1.0, 0.4, n, D, ('trainer', kind))
    print('%s trainer: instance loss per step %s' % (kind, [c['loss'].mean() for c in caught]))


def test_train_unsupervised_two_epochs_with_the_instance_terms(synth_models, monkeypatch):
    """8 planted tracklets, a stub clustering with two noise rows, two epochs with the instance weights (1, 0.4): finite meters,
    teacher.step = the optimizer's steps, one finite instance loss per step"""
    from grl_amd.reid.evaluator import ATTEvaluator
    from grl_amd.reid.train import pseudo
    fixed = [0, 0, 1, 1, -1, 2, 2, -1]
    tracklets = [((60 + i,), 9000 + i, i % 2) for i in range(8)]
    tr, opt = ST._mt_trainer(synth_models, 5, 0.5, ins_hard_weight=1.0, ins_soft_weight=0.4)
    ev = ATTEvaluator(*tr.teacher.models, only_eval=False)
    steps, calls = [], []
    opt.register_step_post_hook(lambda *_: steps.append(1))
    h = tr.criterion_ins.register_forward_hook(lambda mod, args, out: calls.append(bool(torch.isfinite(out).all())))
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
    for name, m in tr.meters.items():
        assert np.isfinite(float(m.avg)), name
