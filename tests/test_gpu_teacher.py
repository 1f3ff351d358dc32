"""Mean-teacher soft pseudo-labels on a real MI355X: the kernels grl_ema_update (grl_amd/csrc/ema.hip) and
grl_soft_ce (grl_amd/csrc/softce.hip) through the C ABI, SoftClusterMemoryLoss, the stale-plan guard of MeanTeacher.update,
MeanTeacherSEQTrainer steps and two train_unsupervised epochs.

grl_ema_update is compared BIT FOR BIT with the numpy float32 restatement of tests/teacher_ref.py (where the restatement is
NaN the kernel's result must be NaN: IEEE 754 leaves a NaN's sign and payload to the implementation, and the host's 0 x inf
differs from the device's in the sign bit).  grl_soft_ce is compared per element with the float64 model inside that
element's derived bound (teacher_ref.b_soft_ce) -- never a norm over the tensor; the top-1 count, the zero rows and the
w = 0 form against grl_softmax_ce are compared exactly.  Buffers, helpers and conventions are test_gpu_head_float64.py's."""
import contextlib
import copy
import io

import numpy as np
import pytest
import torch

import teacher_ref as R
from test_gpu_head_float64 import SENT, _call, _n, _f, _out, _got, _window, _Inputs, _err
from test_gpu_loss_float64 import _Ints, _untouched
from test_gpu_cmem import _Clips, _loader

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    yield
    R.dump_ratios('MI355X mean teacher')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------------------------------------
# grl_ema_update
def _ema_table(d, dst, src):
    from grl_amd._lib import GrlEmaEntry
    lay = d['layout']
    arr = (GrlEmaEntry * len(lay))()
    for i, (numel, d0, s0) in enumerate(lay):
        arr[i].dst, arr[i].src, arr[i].numel = dst.data_ptr() + 4 * d0, src.data_ptr() + 4 * s0, numel
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    first = torch.from_numpy(R.chunk_first([m for m, _, _ in lay])).cuda()
    return table, first


@pytest.mark.parametrize('count', R.EMA_COUNTS)
def test_ema_update_is_the_float32_restatement_bit_for_bit(count):
    """1 and 37 entries, numel through 1 .. three chunks + 3, dst or src 4 bytes off a 16-byte boundary, sentinels between the
    tensors, one NaN and one inf in src, alpha 0 / 0.5 / 0.999 / 1: every element the restatement's bits, the sentinels and src
    untouched, and the same bits from a second launch on the same start."""
    d = R.in_ema(count)
    src = torch.from_numpy(d['src']).cuda()
    assert src.data_ptr() % 16 == 0
    inside = np.zeros(d['dst'].size, bool)
    for numel, d0, _ in d['layout']:
        inside[d0:d0 + numel] = True
    for alpha in R.EMA_ALPHAS:
        a, b = F(alpha), F(1.0 - alpha)
        want = R.ema_expected(d, a, b)
        runs = []
        for _ in range(2):
            dst = torch.from_numpy(d['dst']).cuda()
            assert dst.data_ptr() % 16 == 0
            table, first = _ema_table(d, dst, src)
            _call('grl_ema_update', table, first, count, _f(float(a)), _f(float(b)))
            torch.cuda.synchronize()
            runs.append(_n(dst).copy())
        got = runs[0]
        assert np.array_equal(_bits(got), _bits(runs[1])), (count, alpha)
        nan = np.isnan(want)
        assert np.isnan(got[nan]).all(), (count, alpha)
        assert nan.sum() == (2 if alpha == 1.0 else 1)                     # the NaN of src; at alpha = 1 also 0 x inf
        assert np.array_equal(_bits(got[~nan]), _bits(want[~nan])), (count, alpha, int((_bits(got) != _bits(want)).sum()))
        assert (got[~inside] == R.EMA_SENTINEL).all(), 'a sentinel between the tensors was written'
        if alpha == 0.0:
            for numel, d0, s0 in d['layout']:
                fin = np.isfinite(d['src'][s0:s0 + numel])
                assert np.array_equal(_bits(got[d0:d0 + numel][fin]), _bits(d['src'][s0:s0 + numel][fin]))      # a copy
    assert np.array_equal(_bits(_n(src)), _bits(d['src'])), 'src was written'


def test_ema_update_rejected_arguments_launch_nothing():
    Err = _err()
    d = R.in_ema(1)
    dst, src = torch.from_numpy(d['dst']).cuda(), torch.from_numpy(d['src']).cuda()
    table, first = _ema_table(d, dst, src)
    for args in ((None, first, 1), (table, None, 1), (table, first, 0), (table, first, -3)):
        with pytest.raises(Err, match='ema_update'):
            _call('grl_ema_update', *(args + (_f(0.5), _f(0.5))))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(_n(dst)), _bits(d['dst']))


# ----------------------------------------------------------------------------------------------------------------------
# grl_soft_ce
def _soft_ce(d, t, lab, w, n, c, with_teacher=True, tl=None):
    """one launch into fresh sentinel buffers -> (loss, correct, dz window [n][c])"""
    ldd = d['ldd']
    loss, correct, dz = _out(1), _out(1), _out(n * ldd)
    ws = torch.empty(3 * n, device='cuda')
    tl = t['tlogits'] if tl is None and with_teacher else tl
    _call('grl_soft_ce', t['logits'], d['ld'], tl, d['ldt'], lab.t, _f(w), n, c, loss, correct, dz, ldd, ws)
    flat = _got(dz, n * ldd).copy()
    win = _window(flat, n, c, ldd, np.full(n * ldd, SENT, np.float32))
    return float(_got(loss, 1)[0]), float(_got(correct, 1)[0]), win, _got(loss, 1).copy()


@pytest.mark.parametrize('n,c,pattern', R.CE_CASES)
def test_soft_ce_against_float64(n, c, pattern):
    """n x c with ld, ldt, ldd wider than c and all different, 1e30 / sentinels in the gaps, the labels -1 and c among the rows
    (and the cases without a valid row), w = 0.5 and 1, |logits| up to 20: loss and every dlogits element inside the derived
    bound, invalid rows exactly +0, correct EQUAL to the model's (the planted tie goes to the lowest index), the inputs
    unchanged, the same bits from a second launch."""
    d = R.in_soft_ce(n, c, pattern)
    t, lab = _Inputs(logits=d['logits'], tlogits=d['tlogits']), _Ints(d['labels'])
    for w in R.CE_W:
        what = (n, c, pattern, w)
        ref = R.soft_ce(d['logits'], d['ld'], d['tlogits'], d['ldt'], d['labels'], w, n, c)
        bd = R.b_soft_ce(ref, n, c)
        loss, correct, dz, lbits = _soft_ce(d, t, lab, w, n, c)
        loss2, correct2, dz2, lbits2 = _soft_ce(d, t, lab, w, n, c)
        assert np.array_equal(_bits(dz), _bits(dz2)) and np.array_equal(_bits(lbits), _bits(lbits2)) and correct == correct2, what
        print('soft_ce %r: loss %.9g (float64 %.9g, bound %.3g), worst dz ratio %.3f' % (
            what, loss, ref['loss'], bd['loss'], float((np.abs(dz - ref['dz_val']) / np.maximum(bd['dz'], 1e-300))[ref['ok']].max())
            if ref['nv'] else 0.0))
        R.check('soft_ce loss', loss, ref['loss'], bd['loss'], what)
        R.check('soft_ce dz', dz, ref['dz_val'], bd['dz'], what)
        assert correct == ref['correct'], what
        assert not _bits(dz[~ref['ok']]).any(), 'an invalid row is not +0 %r' % (what,)
        if ref['nv'] == 0:
            assert _bits(lbits)[0] == 0 and correct == 0.0
    if pattern == 'mixed' and c >= 2:                                    # the tie: row 0 (label on the first) is a hit ...
        z = d['logits'].reshape(n, d['ld'])[:, :c]
        assert (z[0] == z[0].max()).sum() == 2 and d['labels'][0] == R.ce_tie(c)[0]
        only0 = R.soft_ce(d['logits'][:d['ld']], d['ld'], d['tlogits'][:d['ldt']], d['ldt'], d['labels'][:1], 0.5, 1, c)
        assert only0['correct'] == 1.0
        one = _Ints(d['labels'][:1])
        assert _soft_ce(d, t, one, 0.5, 1, c)[1] == 1.0
        if n >= 9:                                                       # ... row 2 (label on the second) is not
            two = _Ints(np.array([-1, -1, d['labels'][2]], np.int64))
            assert _soft_ce(d, t, two, 0.5, 3, c)[1] == 0.0
    t.unchanged(); lab.unchanged()


@pytest.mark.parametrize('n,c,pattern', R.CE_CASES)
def test_soft_ce_with_weight_zero_is_softmax_ce_bit_for_bit(n, c, pattern):
    """w = 0 with tlogits NULL and with garbage (NaN) tlogits: loss, dlogits and correct are grl_softmax_ce's bits"""
    d = R.in_soft_ce(n, c, pattern)
    t, lab = _Inputs(logits=d['logits']), _Ints(d['labels'])
    ldd = d['ldd']
    loss, correct, dz = _out(1), _out(1), _out(n * ldd)
    ws = torch.empty(2 * n, device='cuda')
    _call('grl_softmax_ce', t['logits'], d['ld'], lab.t, None, n, c, loss, correct, dz, ldd, ws)
    want = (_got(loss, 1).copy(), _got(correct, 1).copy(), _got(dz, n * ldd).copy())
    garbage = torch.full((n * d['ldt'],), float('nan'), device='cuda')
    for tl in (None, garbage):
        loss, correct, dz = _out(1), _out(1), _out(n * ldd)
        ws = torch.empty(3 * n, device='cuda')
        _call('grl_soft_ce', t['logits'], d['ld'], tl, d['ldt'], lab.t, _f(0.0), n, c, loss, correct, dz, ldd, ws)
        got = (_got(loss, 1).copy(), _got(correct, 1).copy(), _got(dz, n * ldd).copy())
        for g, wnt, name in zip(got, want, ('loss', 'correct', 'dlogits')):
            assert np.array_equal(_bits(g), _bits(wnt)), (name, n, c, pattern, tl is None)
    t.unchanged(); lab.unchanged()


def test_soft_ce_null_outputs_and_rejected_arguments():
    Err = _err()
    n, c = 9, 257
    d = R.in_soft_ce(n, c, 'mixed')
    t, lab = _Inputs(logits=d['logits'], tlogits=d['tlogits']), _Ints(d['labels'])
    full = _soft_ce(d, t, lab, 0.5, n, c)
    loss, ws = _out(1), torch.empty(3 * n, device='cuda')
    _call('grl_soft_ce', t['logits'], d['ld'], t['tlogits'], d['ldt'], lab.t, _f(0.5), n, c, loss, None, None, 0, ws)
    assert np.array_equal(_bits(_got(loss, 1)), _bits(full[3]))           # correct and dlogits may be NULL
    loss, correct, dz = _out(1), _out(1), _out(n * d['ldd'])
    good = dict(logits=t['logits'], ld=d['ld'], tl=t['tlogits'], ldt=d['ldt'], lab=lab.t, w=0.5, n=n, c=c, loss=loss,
                correct=correct, dz=dz, ldd=d['ldd'], ws=ws)
    for kw in (dict(logits=None), dict(lab=None), dict(loss=None), dict(ws=None), dict(n=0), dict(c=0), dict(ld=c - 1),
               dict(ldd=c - 1), dict(w=-0.5), dict(w=1.5), dict(w=float('nan')), dict(tl=None), dict(ldt=c - 1)):
        a = dict(good, **kw)
        with pytest.raises(Err, match='soft_ce'):
            _call('grl_soft_ce', a['logits'], a['ld'], a['tl'], a['ldt'], a['lab'], _f(a['w']), a['n'], a['c'], a['loss'],
                  a['correct'], a['dz'], a['ldd'], a['ws'])
    for buf in (loss, correct, dz):
        _untouched(buf)
    t.unchanged(); lab.unchanged()


# ----------------------------------------------------------------------------------------------------------------------
# SoftClusterMemoryLoss
def test_soft_cluster_memory_loss_against_float64_and_its_backward_is_the_base_class():
    """n = 9, D = 256, K = 70 with one noise row: the loss inside the end-to-end bound of the float64 model; the teacher gets
    no gradient; the input gradient is grl_oim_grad of the kernel's dlogits and the memory after the backward is
    ClusterMemoryLoss's from the same state, bit for bit (the update reads the STUDENT rows only)."""
    import cmem_ref as CR
    from grl_amd.reid.loss import ClusterMemoryLoss, SoftClusterMemoryLoss
    n, D, K, w = CR.LOSS_N, CR.LOSS_D, 70, 0.5
    d = CR.in_loss(K)
    teach = CR.in_loss(K, tag='second')['x']
    crit = SoftClusterMemoryLoss(D, K, temp=CR.LOSS_TEMP, momentum=CR.LOSS_MOMENTUM, mode='hard').cuda()
    crit.reset(torch.from_numpy(d['cent']).cuda())
    x, y = torch.from_numpy(d['x']).cuda().requires_grad_(True), torch.from_numpy(d['labels']).cuda()
    tt = torch.from_numpy(teach).cuda()
    loss, logits = crit(x, y, teacher=tt, soft_weight=w)
    assert not logits.requires_grad and tuple(logits.shape) == (n, K) and logits.grl_top1[1] == n
    loss.backward()
    torch.cuda.synchronize()
    ref = R.memory_loss(d['x'], teach, d['cent'], d['labels'], w, n, D, K, CR.LOSS_TEMP)
    bd = R.b_memory_loss(ref, n, D, K)
    R.check('memory loss logits', _n(logits), ref['logits'], bd['logits'], K)
    R.check('memory loss', loss.item(), ref['loss'], bd['loss'], K)
    assert float(logits.grl_top1[0]) == R.soft_ce(_n(logits).reshape(-1), K, None, 0, d['labels'], 0.0, n, K)['correct']
    assert tt.grad is None and not x.grad[4].any() and bool(torch.isfinite(x.grad).all())
    assert np.array_equal(_n(tt), teach)
    plain = ClusterMemoryLoss(D, K, temp=CR.LOSS_TEMP, momentum=CR.LOSS_MOMENTUM, mode='hard').cuda()
    plain.reset(torch.from_numpy(d['cent']).cuda())
    x2 = torch.from_numpy(d['x']).cuda().requires_grad_(True)
    plain(x2, y)[0].backward()
    torch.cuda.synchronize()
    assert torch.equal(crit.centroids, plain.centroids) and not np.array_equal(_n(crit.centroids), d['cent'])
    assert not torch.equal(x.grad, x2.grad)                               # the soft target moved the gradient
    # soft_weight = 0 and teacher = None: the base class's call, bit for bit
    for kw in (dict(teacher=tt, soft_weight=0.0), dict(teacher=None, soft_weight=0.5), dict()):
        a, b = (cls(D, K, temp=CR.LOSS_TEMP, momentum=CR.LOSS_MOMENTUM).cuda() for cls in (SoftClusterMemoryLoss, ClusterMemoryLoss))
        outs = []
        for c_, k_ in ((a, kw), (b, {})):
            c_.reset(torch.from_numpy(d['cent']).cuda())
            xi = torch.from_numpy(d['x']).cuda().requires_grad_(True)
            li, lg = c_(xi, y, **k_)
            li.backward()
            outs.append((li.detach(), lg.detach(), xi.grad, c_.centroids, lg.grl_top1[0]))
        torch.cuda.synchronize()
        assert all(torch.equal(p, q) for p, q in zip(*outs)), kw
    with pytest.raises(ValueError, match='teacher must be on the device of the inputs'):
        crit(x, y, teacher=tt.cpu(), soft_weight=0.5)


# ----------------------------------------------------------------------------------------------------------------------
# the teacher
def _students(synth_models):
    dev = torch.device('cuda:0')
    return tuple(copy.deepcopy(m).to(dev) for m in synth_models)


def _teacher_state(teacher):
    return {name: _n(t).copy() for name, t, _ in teacher.pairs}


def test_update_rebuilds_the_teachers_packed_eval_plan(synth_models):
    """a teacher eval forward, one SGD step on the student, update() at step 0 (a copy), the teacher forward again: the
    second output is the student's own eval() forward bit for bit and differs from the first -- a missing touch_state would
    serve the plan folded from the old weights."""
    from grl_amd import engine
    from grl_amd.reid.train import MeanTeacher
    from grl_amd.synthetic import synth_clips_structured
    cnn, siam, _ = _students(synth_models)
    teacher = MeanTeacher(cnn, siam, alpha=0.999)
    assert teacher.step == 0 and teacher.count > 300 and teacher.numel > 50_000_000
    assert all(not m.training for m in teacher.models) and all(not p.requires_grad for m in teacher.models for p in m.parameters())
    clips = synth_clips_structured(2, 2, seed=3).cuda()
    first = engine.extract_features(*teacher.models, clips).clone()
    opt = torch.optim.SGD(list(cnn.parameters()) + list(siam.parameters()), lr=1e-3)
    cnn.train(); siam.train()
    x_uncorr, x_corr = cnn(clips)
    (x_uncorr.pow(2).sum() + siam(x_corr)[1].pow(2).sum()).backward()
    opt.step()
    teacher.update()
    assert teacher.step == 1
    second = engine.extract_features(*teacher.models, clips)
    cnn.eval(); siam.eval()
    want = engine.extract_features(cnn, siam, clips)
    torch.cuda.synchronize()
    assert torch.equal(second, want)
    assert not torch.equal(second, first)
    for name, t, s in teacher.pairs:
        assert torch.equal(t, s), name
    # the state dict carries both modules under their checkpoint key, the step and alpha
    sd = teacher.state_dict()
    assert set(sd) == {'cnn', 'siamese', 'step', 'alpha'} and sd['step'] == 1 and sd['alpha'] == 0.999
    assert set(sd['cnn']['state_dict']) == set(cnn.state_dict()) and set(sd['siamese']['state_dict']) == set(siam.state_dict())
    other = MeanTeacher(*_students(synth_models)[:2], alpha=0.5)
    before = engine.extract_features(*other.models, clips).clone()
    other.load_state_dict(sd)
    assert other.step == 1 and other.alpha == 0.999
    after = engine.extract_features(*other.models, clips)
    assert torch.equal(after, second) and not torch.equal(after, before)


def _mt_trainer(synth_models, K, soft_weight, plain=False):
    from grl_amd.reid.loss import ClusterMemoryLoss, SoftClusterMemoryLoss, PairLoss
    from grl_amd.reid.train import SEQTrainer, MeanTeacher, MeanTeacherSEQTrainer
    dev = torch.device('cuda:0')
    cnn, siam, siamv = _students(synth_models)
    cls = ClusterMemoryLoss if plain else SoftClusterMemoryLoss
    crit_c, crit_u = cls(2048, K).to(dev), cls(2048, K).to(dev)
    if plain:
        tr = SEQTrainer(cnn, siam, siamv, PairLoss().to(dev), crit_c, crit_u, None)
    else:
        tr = MeanTeacherSEQTrainer(cnn, siam, siamv, PairLoss().to(dev), crit_c, crit_u, None,
                                   teacher=MeanTeacher(cnn, siam, alpha=0.999), soft_weight=soft_weight)
    params = [p for m in (cnn, siam, siamv) for p in m.parameters()]
    opt = torch.optim.SGD(params, lr=1e-3, momentum=0.9, weight_decay=5e-4, nesterov=True)
    return tr, opt


K3 = 3
TRACKLETS4 = [((40 + i,), (0, 0, 2, 2)[i], i % 2) for i in range(4)]


def _seeds():
    g = torch.Generator().manual_seed(5)
    return [torch.nn.functional.normalize(torch.randn((K3, 2048), generator=g), dim=1) for _ in range(2)]


def _one_step(tr, opt):
    seeds = _seeds()
    tr.criterion_corr.reset(seeds[0].clone().cuda())
    tr.criterion_uncorr.reset(seeds[1].clone().cuda())
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(0, _loader(TRACKLETS4, 4), opt)
    torch.cuda.synchronize()


def test_trainer_step_with_soft_weight_zero_is_the_plain_step_bit_for_bit(synth_models):
    """B = 4, T = 2, K = 3: one MeanTeacherSEQTrainer step with soft_weight = 0 against one SEQTrainer + ClusterMemoryLoss step
    from the same state -- the loss, every parameter gradient, every parameter and both memories, bit for bit"""
    outs = []
    for plain in (False, True):
        tr, opt = _mt_trainer(synth_models, K3, 0.0, plain=plain)
        _one_step(tr, opt)
        mods = (tr.model, tr.siamese_model, tr.siamese_model_uncorr)
        outs.append((tr.meters['loss'].avg, [(n, p.grad, p.detach()) for m in mods for n, p in m.named_parameters()],
                     tr.criterion_corr.centroids, tr.criterion_uncorr.centroids))
        if not plain:
            assert tr.teacher.step == 1 and not opt._optimizer_step_post_hooks
    (la, pa, ca, ua), (lb, pb, cb, ub) = outs
    assert la == lb and np.isfinite(la)
    assert len(pa) == len(pb) > 200
    with_grad = 0
    for (n1, g1, p1), (n2, g2, p2) in zip(pa, pb):
        assert n1 == n2 and (g1 is None) == (g2 is None) and torch.equal(p1, p2), n1      # (None: a parameter the step does not use)
        if g1 is not None:
            assert torch.equal(g1, g2), n1
            with_grad += 1
    assert with_grad > 200
    assert torch.equal(ca, cb) and torch.equal(ua, ub)


def test_trainer_step_with_a_soft_target(synth_models):
    """one step with soft_weight = 0.5 from teacher.step = 5 (a = 5 / 6, a real blend): the three identity losses inside the
    end-to-end bound of the float64 model on the fetched student rows, teacher rows and memories; no teacher tensor has a
    gradient; the teacher's weights after the step are the restatement's bits; the teacher's modules are in eval()."""
    tr, opt = _mt_trainer(synth_models, K3, 0.5)
    teacher = tr.teacher
    teacher.step = 5
    before = _teacher_state(teacher)
    seen = []

    def hook(mod, args, kwargs, out):
        seen.append(dict(x=_n(args[0]).copy(), y=_n(args[1]).copy(), teacher=_n(kwargs['teacher']).copy(), w=kwargs['soft_weight'],
                         cent=_n(mod.centroids).copy(), loss=out[0].detach(), top1=out[1].grl_top1[0], logits=out[1].detach(),
                         who='uncorr' if mod is tr.criterion_uncorr else 'corr', grad=kwargs['teacher'].requires_grad))
    handles = [c.register_forward_hook(hook, with_kwargs=True) for c in (tr.criterion_corr, tr.criterion_uncorr)]
    _one_step(tr, opt)
    for h in handles:
        h.remove()
    assert sorted((s['who'], s['x'].shape[0]) for s in seen) == [('corr', 4), ('corr', 8), ('uncorr', 4)]
    for s in seen:
        n = s['x'].shape[0]
        assert s['w'] == 0.5 and not s['grad'] and s['teacher'].shape == s['x'].shape and not np.array_equal(s['teacher'], s['x'])
        ref = R.memory_loss(s['x'], s['teacher'], s['cent'], s['y'], 0.5, n, 2048, K3, 0.05)
        bd = R.b_memory_loss(ref, n, 2048, K3)
        print('%s %d rows: loss %.9g (float64 %.9g, bound %.3g)' % (s['who'], n, s['loss'].item(), ref['loss'], bd['loss']))
        R.check('trainer id loss', s['loss'].item(), ref['loss'], bd['loss'], (s['who'], n))
        R.check('trainer id logits', _n(s['logits']), ref['logits'], bd['logits'], (s['who'], n))
        assert float(s['top1']) == R.soft_ce(_n(s['logits']).reshape(-1), K3, None, 0, s['y'], 0.0, n, K3)['correct']
    assert np.isfinite(tr.meters['loss'].avg)
    assert teacher.step == 6 and not opt._optimizer_step_post_hooks
    assert all(not m.training for m in teacher.models)
    assert all(p.grad is None and not p.requires_grad for m in teacher.models for p in m.parameters())
    a, b = R.ema_alpha(5, 0.999)
    assert abs(float(a) - 5.0 / 6.0) < 1e-7
    moved = 0
    for name, t, s in teacher.pairs:
        want = R.ema_f32(before[name], _n(s), a, b)
        got = _n(t)
        assert np.array_equal(_bits(got), _bits(want)), name
        moved += int(not np.array_equal(got, before[name]))
    assert moved > 200                                                      # the step changed the student, the update the teacher


def test_graphed_step_refuses_the_mean_teacher_trainer(synth_models):
    from grl_amd.train_graph import GraphedTrainStep
    tr, opt = _mt_trainer(synth_models, K3, 0.5)
    with pytest.raises(ValueError, match='does not capture a MeanTeacherSEQTrainer'):
        GraphedTrainStep(tr, opt, torch.zeros((4, 2, 3, 256, 128), device='cuda'), torch.zeros(4, dtype=torch.int64, device='cuda'))


def test_train_unsupervised_two_epochs_with_a_mean_teacher(synth_models, monkeypatch):
    """8 planted tracklets, a stub clustering with two noise rows, two epochs, clustering on the TEACHER's features: finite
    losses, teacher.step = the optimizer's steps, the hook gone from the optimizer, and an ATTEvaluator on teacher.models
    extracts features."""
    from grl_amd.reid.evaluator import ATTEvaluator
    from grl_amd.reid.train import pseudo
    fixed = [0, 0, 1, 1, -1, 2, 2, -1]
    tracklets = [((60 + i,), 9000 + i, i % 2) for i in range(8)]
    tr, opt = _mt_trainer(synth_models, 5, 0.5)
    ev = ATTEvaluator(*tr.teacher.models, only_eval=False)
    steps, feats = [], []
    mine = opt.register_step_post_hook(lambda *_: steps.append(1))

    def stub(xf, **kw):
        feats.append(xf.clone())
        return pseudo.PseudoLabels(torch.tensor(fixed, device=xf.device), 'stub')
    monkeypatch.setattr(pseudo, 'pseudo_labels', stub)
    losses = []
    with contextlib.redirect_stdout(io.StringIO()):
        hist = pseudo.train_unsupervised(tr, ev, opt, tracklets,
                                         lambda t: torch.utils.data.DataLoader(_Clips(t), batch_size=4, shuffle=False),
                                         lambda t: _loader(t, 4), 2, on_epoch=lambda e, l: losses.append(tr.meters['loss'].avg))
    torch.cuda.synchronize()
    assert len(hist) == 2 and len(losses) == 2 and all(np.isfinite(v) for v in losses)
    assert len(steps) == 2 and tr.teacher.step == len(steps)
    assert list(opt._optimizer_step_post_hooks) == [mine.id]                # the trainer's hook is gone, the test's is left
    assert all(not m.training for m in tr.teacher.models)
    assert tuple(feats[0].shape) == (8, 6144) and not torch.equal(feats[0], feats[1])     # epoch 1 clustered the moved teacher
    xf = ev.extract_feature(torch.utils.data.DataLoader(_Clips(tracklets), batch_size=4, shuffle=False))[0]
    assert tuple(xf.shape) == (8, 6144) and bool(torch.isfinite(xf).all())
    for crit in (tr.criterion_corr, tr.criterion_uncorr):
        assert crit.num_clusters == 3 and bool(torch.isfinite(crit.centroids).all())
