"""The soft hybrid / proxy memory without a GPU: the float64 models of tests/soft_memory_ref.py against torch float64 autograd of
the formulas written out with log_softmax (1e-10, the figure DESIGN.md 4am holds its closed form to), the fp32 restatements in
the kernels' term order inside the derived bounds, every ValueError of the two loss modules and the two trainers raised before
any device call, and train_unsupervised's type checks accepting the new classes."""
import os

import numpy as np
import pytest
import torch

import soft_memory_ref as R
import hybrid_ref as HR
import proxy_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _k(k, P):
    return P if k == 'P' else min(k, P)


# ----------------------------------------------------------------------------------------------------------------------
# the float64 models are the formulas
@pytest.mark.parametrize('n,N', ((5, 7), (5, 300)))
@pytest.mark.parametrize('w', R.W_SWEEP)
def test_hybrid_model_is_torch_autograd_of_the_formula(n, N, w):
    for name in R.HY_LAYOUTS:
        d = R.in_hybrid(n, N, name)
        ref = R.soft_hybrid_ce(d['logits'], d['ld'], d['tlogits'], d['ldt'], d['targets'], d['cp'], d['cm'], d['ic'], w, n, N, d['C'])
        z = torch.from_numpy(d['logits'].reshape(n, d['ld'])[:, :N].astype(np.float64)).requires_grad_(True)
        tz = torch.from_numpy(d['tlogits'].reshape(n, d['ldt'])[:, :N].astype(np.float64)).requires_grad_(True)
        loss = R.torch_soft_hybrid(z, tz, torch.from_numpy(d['targets']), d['cp'], d['cm'], w)
        loss.backward()
        assert ref['nv'] >= 1 and (n < 2 or not ref['valid'][1])
        assert abs(loss.item() - ref['loss']) < 1e-10 * max(1.0, abs(ref['loss'])), (name, w)
        assert np.abs(z.grad.numpy() - ref['dz']).max() < 1e-10, (name, w)
        if w == 0.0:
            hard = ref['hard']
            assert abs(ref['loss'] - hard['loss']) < 1e-12 and np.abs(ref['dz'] - hard['dz']).max() < 1e-15
            assert tz.grad is None or not tz.grad.any()


@pytest.mark.parametrize('n,P', ((5, 5), (5, 257)))
@pytest.mark.parametrize('w', R.W_SWEEP)
def test_proxy_model_is_torch_autograd_of_the_formula(n, P, w):
    for pattern in ('spread', 'mixed'):
        for k0 in (0, 1, 50):
            for wts in R.PX_WEIGHTS:
                d = R.in_proxy(n, P, 3, pattern)
                k = _k(k0, P)
                ref = R.soft_proxy_ce(d['logits'], d['ld'], d['tlogits'], d['ldt'], d['labels'], d['cams'], d['pcl'], d['pcm'], w, n,
                                      P, k, *wts)
                z = torch.from_numpy(d['logits'].reshape(n, d['ld'])[:, :P].astype(np.float64)).requires_grad_(True)
                tz = torch.from_numpy(d['tlogits'].reshape(n, d['ldt'])[:, :P].astype(np.float64))
                loss = R.torch_soft_proxy(z, tz, ref, w)
                loss.backward()
                what = (pattern, k, wts, w)
                assert ref['nv'] >= 1 and not ref['valid'][1], what
                assert abs(loss.item() - ref['loss']) < 1e-10 * max(1.0, abs(ref['loss'])), what
                assert np.abs(z.grad.numpy() - ref['dz']).max() < 1e-10, what
                if w == 0.0:
                    hard = ref['hard']
                    assert abs(ref['loss'] - hard['loss']) < 1e-12 and np.abs(ref['dz'] - hard['dz']).max() < 1e-15, what


# ----------------------------------------------------------------------------------------------------------------------
# the bounds are satisfiable: the fp32 restatements in the kernels' order
@pytest.mark.parametrize('n,N', R.HY_CASES)
def test_hybrid_fp32_restatement_is_inside_the_bounds(n, N):
    for name in R.HY_LAYOUTS:
        d = R.in_hybrid(n, N, name, R.hy_seed(n, N, name))
        for w in R.W_SWEEP:
            ref = R.soft_hybrid_ce(d['logits'], d['ld'], d['tlogits'], d['ldt'], d['targets'], d['cp'], d['cm'], d['ic'], w, n, N,
                                   d['C'])
            bd = R.b_soft_hybrid_ce(ref, n, N, d['C'])
            got = R.soft_hybrid_ce_f32(d['logits'], d['ld'], d['tlogits'], d['ldt'], d['targets'], d['cp'], d['cm'], d['ic'], w, n, N,
                                       d['C'])
            R.check('cpu soft_hybrid loss', got['loss'], ref['loss'], bd['loss'], (n, N, name, w))
            R.check('cpu soft_hybrid dz', got['dz'], ref['dz'], bd['dz'], (n, N, name, w))
            assert got['correct'] == ref['correct']
            assert not bd['dz'][~ref['valid']].any() and (bd['dz'][ref['valid']] < 1e-4).all()      # a bound that says something
            if w == 0.0:                                      # the restatement with w = 0 is hybrid_ref's, bit for bit
                hard = HR.hybrid_ce_f32(d['logits'], d['ld'], d['targets'], d['cp'], d['cm'], d['ic'], n, N, d['C'])
                assert np.array_equal(got['dz'].view(np.uint32), hard['dz'].view(np.uint32)) and got['loss'] == hard['loss']


@pytest.mark.parametrize('n,P', R.PX_CASES)
def test_proxy_fp32_restatement_is_inside_the_bounds(n, P):
    for pattern, ties in (('spread', False), ('mixed', False), ('mixed', True)):
        d = R.in_proxy(n, P, 3, pattern, ties=ties)
        for k0 in R.PX_K:
            k = _k(k0, P)
            for wts in R.PX_WEIGHTS:
                for w in R.W_SWEEP:
                    what = (n, P, pattern, ties, k, wts, w)
                    ref = R.soft_proxy_ce(d['logits'], d['ld'], d['tlogits'], d['ldt'], d['labels'], d['cams'], d['pcl'], d['pcm'],
                                          w, n, P, k, *wts)
                    bd = R.b_soft_proxy_ce(ref, n, P)
                    got = R.soft_proxy_ce_f32(d['logits'], d['ld'], d['tlogits'], d['ldt'], ref, w, n, P)
                    R.check('cpu soft_proxy loss', got['loss'], ref['loss'], bd['loss'], what)
                    R.check('cpu soft_proxy dz', got['dz'], ref['dz'], bd['dz'], what)
                    assert not bd['dz'][~ref['valid']].any() and (bd['dz'][ref['valid']] < 1e-4).all(), what


def test_the_sweeps_hold_what_the_kernels_can_get_wrong():
    """out-of-range targets on both sides, a batch without a valid row, a class of more than a wave of members, a row without a
    proxy of its own, and ties across the selection threshold"""
    d = R.in_hybrid(5, 300, 'big')
    assert d['targets'][1] == -1 and d['targets'][3] == d['C'] and np.diff(d['cp']).max() > 64
    assert d['ld'] > 300 and d['ldt'] != d['ld'] and d['ldd'] > 300
    d = R.in_hybrid(5, 1030, 'random')
    cm, cp = d['cm'], d['cp']
    assert any(np.diff(cm[cp[c]:cp[c + 1]]).max(initial=0) > 1 for c in range(d['C']))          # interleaved members
    d = R.in_proxy(5, 257, 3, 'mixed', ties=True)
    ref = PR.proxy_ce(d['logits'], d['ld'], d['labels'], d['cams'], d['pcl'], d['pcm'], 5, 257, 50, 1.0, 0.5)
    assert ref['own'][1] == -1 and ref['own'][3] == -1 and ref['nv'] == 3
    z = d['logits'].reshape(5, d['ld'])[:, :257]
    tied = 0
    for i, rec in ref['r'].items():
        neg = ref['negsel'][i]
        out = np.setdiff1d(rec['N'], neg)
        tied += int(np.isin(z[i, out], z[i, neg]).any())                                         # an equal value refused
    assert tied == 3


# ----------------------------------------------------------------------------------------------------------------------
# refusals, before any device call
def _no_device(monkeypatch):
    from grl_amd import engine
    from grl_amd.reid.loss import memory

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    # (the hard and soft memory criteria launch through memory._call and engine.gemm alone: they hold no _call of their own)
    for mod, name in ((engine, '_call'), (engine, 'gemm'), (memory, '_call')):
        monkeypatch.setattr(mod, name, no_device)


BAD_TEACHERS = ((lambda: torch.zeros((5, 16)), r'teacher must be \[n, D\] = \(6, 16\), the shape of the inputs .got \(5, 16\)'),
                (lambda: torch.zeros((6, 16, 1)), r'teacher must be \[n, D\]'),
                (lambda: torch.zeros((6, 16), dtype=torch.float64), 'teacher must be float32 .got torch.float64'),
                (lambda: torch.zeros((6, 16), device='meta'), 'teacher must be on the device of the inputs, cpu .got meta'),
                (lambda: torch.zeros((6, 16), requires_grad=True), 'teacher must carry no gradient'),
                (lambda: np.zeros((6, 16), np.float32), 'teacher must be a tensor .got ndarray'))


def test_loss_modules_refuse_before_any_device_call(monkeypatch):
    from grl_amd.reid.loss import (HybridMemoryLoss, ProxyMemoryLoss, SoftHybridMemoryLoss, SoftProxyMemoryLoss, SoftHybridMemory,
                                   SoftProxyMemory)
    from grl_amd import _lib
    _no_device(monkeypatch)
    assert issubclass(SoftHybridMemoryLoss, HybridMemoryLoss) and issubclass(SoftProxyMemoryLoss, ProxyMemoryLoss)
    assert SoftHybridMemory.backward is not None and SoftProxyMemory.backward is not None
    assert 'grl_soft_hybrid_ce' in _lib.exported_symbols() and 'grl_soft_proxy_ce' in _lib.exported_symbols()
    assert _lib.ABI_VERSION == 10
    x, y = torch.zeros((6, 16)), torch.zeros(6, dtype=torch.int64)
    hy = SoftHybridMemoryLoss(16, temp=0.05, momentum=0.2)
    px = SoftProxyMemoryLoss(16, temp=0.07, momentum=0.2, mode='hard', k_neg=3, w_intra=1.0, w_inter=0.5)
    assert px.mode == 'hard' and px.k_neg == 3 and hy.num_instances == 1
    for crit, who, extra in ((hy, 'SoftHybridMemoryLoss', dict(index=y)), (px, 'SoftProxyMemoryLoss', dict(cams=y))):
        for make, pattern in BAD_TEACHERS:
            with pytest.raises(ValueError, match=who + ': ' + pattern):
                crit(x, y, teacher=make(), soft_weight=0.5, **extra)
        for w in (-0.1, 1.5, float('nan')):
            with pytest.raises(ValueError, match=who + r': soft_weight must be in \[0, 1\]'):
                crit(x, y, teacher=torch.zeros((6, 16)), soft_weight=w, **extra)
    with pytest.raises(ValueError, match="mode must be 'hard', 'mean' or 'instance'"):       # the base's own checks stand
        SoftProxyMemoryLoss(16, mode='soft')
    with pytest.raises(ValueError, match='temp must be > 0'):
        SoftHybridMemoryLoss(16, temp=0.0)


def test_trainers_refuse_before_any_device_call(monkeypatch):
    from grl_amd import train_graph
    from grl_amd.reid.loss import (HybridMemoryLoss, ProxyMemoryLoss, SoftHybridMemoryLoss, SoftProxyMemoryLoss,
                                   SoftClusterMemoryLoss)
    from grl_amd.reid.train import (MeanTeacher, MeanTeacherMixin, MeanTeacherSEQTrainer, MeanTeacherHybridSEQTrainer,
                                    MeanTeacherCameraSEQTrainer, HybridSEQTrainer, CameraSEQTrainer)
    _no_device(monkeypatch)
    t = object.__new__(MeanTeacher)
    for cls, base, soft, plain in ((MeanTeacherHybridSEQTrainer, HybridSEQTrainer, SoftHybridMemoryLoss, HybridMemoryLoss),
                                   (MeanTeacherCameraSEQTrainer, CameraSEQTrainer, SoftProxyMemoryLoss, ProxyMemoryLoss)):
        who, want = cls.__name__, soft.__name__
        assert issubclass(cls, base) and issubclass(cls, MeanTeacherMixin) and cls.__mro__.index(MeanTeacherMixin) < cls.__mro__.index(base)
        a, b, hard, other = soft(16), soft(16), plain(16), SoftClusterMemoryLoss(16, 4)
        with pytest.raises(ValueError, match='%s: criterion_corr must be a %s .got %s' % (who, want, plain.__name__)):
            cls(None, None, None, None, hard, a, None, teacher=t)
        with pytest.raises(ValueError, match='%s: criterion_uncorr must be a %s .got %s' % (who, want, plain.__name__)):
            cls(None, None, None, None, a, hard, None, teacher=t)
        with pytest.raises(ValueError, match='%s: criterion_corr must be a %s .got SoftClusterMemoryLoss' % (who, want)):
            cls(None, None, None, None, other, a, None, teacher=t)
        with pytest.raises(ValueError, match='%s: criterion_corr and criterion_uncorr must be two objects' % who):
            cls(None, None, None, None, a, a, None, teacher=t)
        with pytest.raises(ValueError, match='%s: teacher must be a MeanTeacher .got NoneType' % who):
            cls(None, None, None, None, a, b, None, teacher=None)
        for bad in (2, -0.5, float('nan')):
            with pytest.raises(ValueError, match=r'%s: soft_weight must be in \[0, 1\]' % who):
                cls(None, None, None, None, a, b, None, teacher=t, soft_weight=bad)
            with pytest.raises(ValueError, match=r'%s: tri_soft_weight must be in \[0, 1\]' % who):
                cls(None, None, None, None, a, b, None, teacher=t, tri_soft_weight=bad)
        # a captured step has no place for the teacher, whichever base carries it
        with pytest.raises(ValueError, match='GraphedTrainStep does not capture a %s' % who):
            train_graph.GraphedTrainStep(object.__new__(cls), None, None, None)
    assert issubclass(MeanTeacherSEQTrainer, MeanTeacherMixin)
    with pytest.raises(ValueError, match='GraphedTrainStep does not capture a MeanTeacherSEQTrainer'):
        train_graph.GraphedTrainStep(object.__new__(MeanTeacherSEQTrainer), None, None, None)


def test_the_mixin_hands_the_criteria_what_their_base_trainer_does():
    """_id_loss without a device: index= / cams= next to teacher= and soft_weight=, the teacher's rows picked by branch, and
    teacher=None with weight 0 when no teacher pass was made"""
    from grl_amd.reid.train import MeanTeacherHybridSEQTrainer, MeanTeacherCameraSEQTrainer, MeanTeacherSEQTrainer
    calls = []

    class Crit(object):
        def __call__(self, feats, targets, **kw):
            calls.append(kw)
            return 'out'
    for cls, key, attr in ((MeanTeacherHybridSEQTrainer, 'index', '_index_rows'), (MeanTeacherCameraSEQTrainer, 'cams', '_cam_rows'),
                           (MeanTeacherSEQTrainer, None, None)):
        tr = object.__new__(cls)
        tr.criterion_corr, tr.criterion_uncorr, tr.soft_weight = Crit(), Crit(), 0.25
        if attr:
            setattr(tr, attr, {'clip': 'c-rows', 'frame': 'f-rows'})
        tr._teacher_rows = {('corr', 'clip'): 'cc', ('corr', 'frame'): 'cf', ('uncorr', 'clip'): 'uc'}
        del calls[:]
        assert tr._id_loss(tr.criterion_uncorr, None, None, 'clip') == 'out'
        tr._id_loss(tr.criterion_corr, None, None, 'frame')
        tr._teacher_rows = None
        tr._id_loss(tr.criterion_corr, None, None, 'clip')
        want = [dict(teacher='uc', soft_weight=0.25), dict(teacher='cf', soft_weight=0.25), dict(teacher=None, soft_weight=0.0)]
        if key:
            for kw, rows in zip(want, ('c-rows', 'f-rows', 'c-rows')):
                kw[key] = rows
        assert calls == want, cls.__name__


def test_train_unsupervised_accepts_the_new_classes(monkeypatch):
    """the isinstance checks of train_unsupervised take the subclasses (zero epochs: the checks alone run), and still refuse a
    trainer or a criterion of the other family"""
    from grl_amd.reid.loss import SoftHybridMemoryLoss, SoftProxyMemoryLoss
    from grl_amd.reid.train import MeanTeacherHybridSEQTrainer, MeanTeacherCameraSEQTrainer, pseudo
    _no_device(monkeypatch)
    hy, cam = object.__new__(MeanTeacherHybridSEQTrainer), object.__new__(MeanTeacherCameraSEQTrainer)
    hy.criterion_corr, hy.criterion_uncorr = SoftHybridMemoryLoss(16), SoftHybridMemoryLoss(16)
    cam.criterion_corr, cam.criterion_uncorr = SoftProxyMemoryLoss(16), SoftProxyMemoryLoss(16)
    assert pseudo.train_unsupervised(hy, None, None, [], None, None, 0, hybrid=True) == []
    assert pseudo.train_unsupervised(hy, None, None, [], None, None, 0, hybrid=True, self_paced=dict(delta=0.02)) == []
    assert pseudo.train_unsupervised(cam, None, None, [], None, None, 0, cameras=True) == []
    with pytest.raises(ValueError, match='hybrid=True needs a HybridSEQTrainer .got MeanTeacherCameraSEQTrainer'):
        pseudo.train_unsupervised(cam, None, None, [], None, None, 0, hybrid=True)
    with pytest.raises(ValueError, match='cameras=True needs a CameraSEQTrainer .got MeanTeacherHybridSEQTrainer'):
        pseudo.train_unsupervised(hy, None, None, [], None, None, 0, cameras=True)
    hy.criterion_uncorr = SoftProxyMemoryLoss(16)
    with pytest.raises(ValueError, match='hybrid=True needs criterion_uncorr to be a HybridMemoryLoss .got SoftProxyMemoryLoss'):
        pseudo.train_unsupervised(hy, None, None, [], None, None, 0, hybrid=True)


def test_the_header_declares_what_the_binding_registers():
    src = open(os.path.join(ROOT, 'include', 'grl_hip.h')).read()
    assert '#define GRL_ABI_VERSION 10' in src
    for name, nargs in (('grl_soft_hybrid_ce', 18), ('grl_soft_proxy_ce', 22)):
        decl = src[src.index('int %s(' % name):]
        decl = decl[:decl.index(';')]
        assert decl.count(',') + 1 == nargs, name
        from grl_amd import _lib
        assert len(_lib._SIGNATURES[name][0]) == nargs, name
