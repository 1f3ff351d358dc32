"""The float64 model of the instance-contrast terms (tests/ins_contrast_ref.py) is torch float64 autograd of the
formula, its closed-form coefficients and gradient are autograd's, the selection rule holds on hand-made ties, the bounds are
satisfiable by an fp32 restatement in the kernels' order, the end-to-end inputs meet the gap condition, and every refusal of
InstanceContrastLoss / the mean-teacher trainers / the example fires without a device.  No GPU."""
import argparse
import ctypes as C
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ins_contrast_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    yield
    S.dump_ratios('instance contrast, fp32 restatement on the CPU')


# ----------------------------------------------------------------------------------------------------------------------
# the model is the formula
def _torch_formula(f, m, ids, tau, tau_t, wh, ws, c_leaf=None):
    """The issue's definition written with torch ops, the selection found independently of S.select.  c_leaf: a leaf that
    replaces the cosines (its gradient is dL / dc)."""
    u = torch.nn.functional.normalize(f, dim=1, eps=1e-12)
    v = torch.nn.functional.normalize(m, dim=1, eps=1e-12).detach()       # the teacher carries no gradient
    c = u @ v.t() if c_leaf is None else c_leaf
    t = v @ v.t()
    out = []
    for i in range(f.shape[0]):
        cols, p = [], None
        for y in torch.unique(ids).tolist():
            mem = torch.nonzero(ids == y)[:, 0]
            vals = c[i, mem].detach()
            if y == int(ids[i]):
                best = vals.min()
                p = len(cols)
            else:
                best = vals.max()
            cols.append(int(mem[torch.nonzero(vals == best)[0, 0]]))        # the lowest index among equals
        cols = torch.tensor(cols)
        logp = torch.log_softmax(c[i, cols] / tau, 0)
        q = torch.softmax(t[i, cols] / tau_t, 0)
        out.append(-wh * logp[p] - ws * (q * logp).sum())
    return torch.stack(out)


@pytest.mark.parametrize('wh,ws', S.WEIGHTS)
@pytest.mark.parametrize('n,D,pattern', S.CASES)
def test_model_and_closed_forms_against_torch_float64_autograd(n, D, pattern, wh, ws):
    """the loss, the closed-form g (autograd in the cosines) and the closed-form df (autograd in f), <= 1e-10; no gradient in m"""
    for tau, tau_t in S.TAUS:
        d = S.in_ins(n, D, 'a', pattern)
        cs, sel, fw, bw = S.ins_full(d['f'], d['m'], d['ids'], tau, tau_t, wh, ws, d['dloss'])
        assert (sel > 0).sum(1).tolist() == [len(set(d['ids'].tolist()))] * n and ((sel == 2).sum(1) == 1).all()
        args = (torch.from_numpy(d['ids']), S.scal(tau), S.scal(tau_t), S.scal(wh), S.scal(ws))
        f = torch.from_numpy(d['f'].astype(np.float64)).requires_grad_(True)
        m = torch.from_numpy(d['m'].astype(np.float64)).requires_grad_(True)
        dl = torch.from_numpy(d['dloss'].astype(np.float64))
        loss = _torch_formula(f, m, *args)
        (loss * dl).sum().backward()
        assert np.abs(loss.detach().numpy() - fw['loss']).max() <= 1e-10
        assert np.abs(f.grad.numpy() - bw['df']).max() <= 1e-10, np.abs(f.grad.numpy() - bw['df']).max()
        assert m.grad is None or not m.grad.any()
        c = torch.from_numpy(cs['c']).requires_grad_(True)
        _torch_formula(f.detach(), m.detach(), *args, c_leaf=c).sum().backward()
        assert np.abs(c.grad.numpy() * S.scal(tau) - fw['g']).max() <= 1e-10
        assert np.abs(fw['g'].sum(1)).max() <= 1e-12
        if pattern == 'one':
            assert not fw['loss'].any() and not fw['g'].any() and not bw['df'].any()
        if pattern == 'two':
            assert np.array_equal(sel == 2, np.eye(n, dtype=bool))         # every positive is the anchor itself


def test_selection_rule_on_hand_made_ties():
    ids = np.array([7, 7, 7, -3, -3, 2 ** 40, 7], np.int64)
    c = np.array([[.5, .2, .2, .9, .9, .1, .2],       # own id 7: the smallest, 0.2, first at column 1; id -3: 0.9 first at 3
                  [.1, .1, .1, .3, .4, .0, .1],       # own: all equal -> column 0; -3: the largest at 4
                  [.9, .8, .7, .4, .4, .2, .6],       # own: column 6 holds 0.6 < 0.7
                  [.5, .6, .6, .2, .2, .3, .1],       # own id -3: equal -> 3; id 7: the largest 0.6 first at 1
                  [.5, .5, .5, .3, .1, .3, .5],       # own -3: column 4; id 7: all equal -> 0
                  [.1, .2, .3, .4, .5, .6, .3],       # own id 2^40: its only member; 7: column 2 (0.3 first at 2); -3: column 4
                  [.0, .0, .0, .0, .0, .0, .0]])      # everything equal: the first member of every id
    want = np.zeros((7, 7), np.int32)
    for i, (p, negs) in enumerate(((1, (3, 5)), (0, (4, 5)), (6, (3, 5)), (3, (1, 5)), (4, (0, 5)), (5, (2, 4)), (0, (3, 5)))):
        want[i, p] = 2
        want[i, list(negs)] = 1
    assert np.array_equal(S.select(c, ids), want)
    assert np.array_equal(S.select(S.F(c), ids), want)                      # the fp32 restatement: the same rule on fp32 values
    g = S.gaps(c, ids)
    assert g[0] == 0 and g[2] == 0 and abs(g[5] - 0.0) < 1e-15             # ties have no gap
    # ids that differ in the high word only are different ids
    y = np.array([5, 5 + (1 << 32), 5], np.int64)
    s = S.select(np.array([[.3, .9, .1]] * 3), y)
    assert s.tolist() == [[0, 1, 2], [1, 2, 0], [0, 1, 2]]
    for n, _, pattern in S.CASES:                                           # the wide ids keep the partition
        a, b = S.ins_ids(n, pattern), S.ins_ids(n, pattern, 'wide')
        assert np.array_equal(a[:, None] == a[None, :], b[:, None] == b[None, :])
    b = S.ins_ids(130, 'pairs', 'wide')
    assert b.min() < 0 and b.max() > 2 ** 31 and len({int(v) & 0xffffffff for v in b}) < len(set(b.tolist()))


# ----------------------------------------------------------------------------------------------------------------------
# the bounds are satisfiable, the end-to-end class meets the gap condition
@pytest.mark.parametrize('n,D,pattern', S.CASES)
def test_fp32_restatement_is_inside_the_bounds(n, D, pattern):
    for cls in S.CLASSES:
        d = S.in_ins(n, D, cls, pattern)
        for (tau, tau_t), (wh, ws) in zip(S.TAUS * 2, S.WEIGHTS + S.WEIGHTS[::-1]):
            what = (n, D, pattern, cls, tau, tau_t, wh, ws)
            got = S.ins_f32(d['f'], d['m'], d['ids'], tau, tau_t, wh, ws, d['dloss'])
            assert np.isfinite(got['loss']).all() and np.isfinite(got['df']).all(), what
            S.check_stagewise(got, d, tau, tau_t, wh, ws, n, D, what)
            if cls == 'a':
                S.check_end_to_end(got, d, tau, tau_t, wh, ws, n, D, what)
            if cls == 'z':
                assert not got['cos'][0].any() and not got['df'][0].any(), what
            if pattern == 'one':
                assert not got['loss'].any() and not got['coef'].any() and not got['df'].any(), what


def test_the_end_to_end_inputs_meet_the_gap_condition():
    """class (a), every case, plain and wide ids, every anchor: each winner beats the runner-up of its id by more than twice
    the derived bound on cos"""
    worst = np.inf
    for n, D, pattern in S.CASES:
        d = S.in_ins(n, D, 'a', pattern)
        cs = S.cosines(d['f'], d['m'])
        g, b = S.gaps(cs['c'], d['ids']), 2 * S.SAFETY * S.e_cos(cs, D).max(1)
        assert (g > b).all(), (n, D, pattern, float(g.min()), float(b.max()))
        worst = min(worst, float((g / b).min()))
        # the tie classes do have ties / a zero row
        t = S.in_ins(n, D, 't', pattern)
        assert np.array_equal(t['f'][1], t['f'][0]) and not np.array_equal(t['m'][1], t['m'][0])
        assert not S.in_ins(n, D, 'z', pattern)['f'][0].any()
    print('smallest gap / (2 x bound): %.3g' % worst)
    t = S.in_ins(130, 4, 't', 'pairs')                                      # columns 2 and 3: one id, equal teacher rows
    assert np.array_equal(t['m'][3], t['m'][2]) and np.array_equal(t['m'][129], t['m'][0]) and t['ids'][2] == t['ids'][3]
    assert (S.gaps(S.cosines(t['f'], t['m'])['c'], t['ids']) <= 1e-15).all()
    c32 = S.cos_f32(t['f'], t['m'])
    assert np.array_equal(c32[:, 2], c32[:, 3]) and (S.select(c32, t['ids'])[:, 3] == 0).all()     # the lower index wins


# ----------------------------------------------------------------------------------------------------------------------
# the Python surface
def _no_device(*a, **k):
    raise AssertionError('a device call was made')


def test_module_refusals_fire_before_any_device_call(monkeypatch):
    from grl_amd.reid.loss import InstanceContrastLoss, ins_contrast, memory
    monkeypatch.setattr(ins_contrast, '_call', _no_device)
    monkeypatch.setattr(memory, '_call', _no_device)
    crit = InstanceContrastLoss()
    assert crit.tau == 0.1 and crit.teacher_tau == 0.1
    assert InstanceContrastLoss(tau=0.05).teacher_tau == 0.05 and InstanceContrastLoss(0.05, 0.2).teacher_tau == 0.2
    x, y, t = torch.zeros((6, 16)), torch.zeros(6, dtype=torch.int64), torch.zeros((6, 16))
    with pytest.raises(ValueError, match='InstanceContrastLoss: teacher is missing'):
        crit(x, y)
    with pytest.raises(ValueError, match='InstanceContrastLoss: teacher is missing'):
        crit(x, y, teacher=None, hard_weight=1.0, soft_weight=0.4)
    for kw, pattern in ((dict(hard_weight=-1.0), 'hard_weight must be a finite number >= 0'),
                        (dict(soft_weight=-0.1), 'soft_weight must be a finite number >= 0'),
                        (dict(soft_weight=float('nan')), 'soft_weight must be a finite number >= 0'),
                        (dict(hard_weight=0.0), 'hard_weight and soft_weight must not both be 0'),
                        (dict(hard_weight=0.0, soft_weight=0.0), 'hard_weight and soft_weight must not both be 0')):
        with pytest.raises(ValueError, match='InstanceContrastLoss: ' + pattern):
            crit(x, y, teacher=t, **kw)
    for kw, pattern in ((dict(tau=0.0), 'tau must be a finite number > 0'), (dict(tau=-0.1), 'tau must be'),
                        (dict(tau=float('inf')), 'tau must be'), (dict(teacher_tau=0.0), 'teacher_tau must be'),
                        (dict(tau=float('nan')), 'tau must be')):
        with pytest.raises(ValueError, match='InstanceContrastLoss: ' + pattern):
            InstanceContrastLoss(**kw)
    for bad, pattern in ((torch.zeros((5, 16)), r'teacher must be \[n, D\] = \(6, 16\)'),
                         (torch.zeros((6, 16), dtype=torch.float64), 'teacher must be float32'),
                         (torch.zeros((6, 16), requires_grad=True), 'teacher must carry no gradient')):
        with pytest.raises(ValueError, match='InstanceContrastLoss: ' + pattern):
            crit(x, y, teacher=bad)
    from grl_amd._lib import GrlHipError
    with pytest.raises(GrlHipError, match='InstanceContrastLoss feat must live on a HIP device'):     # no CPU path, no device call
        crit(x, y, teacher=t)


def _trainers():
    from grl_amd.reid.loss import SoftClusterMemoryLoss, SoftHybridMemoryLoss, SoftProxyMemoryLoss
    from grl_amd.reid.train import MeanTeacherSEQTrainer, MeanTeacherHybridSEQTrainer, MeanTeacherCameraSEQTrainer
    return ((MeanTeacherSEQTrainer, lambda: SoftClusterMemoryLoss(16, 4)), (MeanTeacherHybridSEQTrainer, lambda: SoftHybridMemoryLoss(16)),
            (MeanTeacherCameraSEQTrainer, lambda: SoftProxyMemoryLoss(16)))


def test_trainer_refusals_name_the_argument():
    from grl_amd.reid.train import MeanTeacher
    t = object.__new__(MeanTeacher)
    for cls, crit in _trainers():
        for kw, pattern in ((dict(ins_hard_weight=-1.0), 'ins_hard_weight must be a finite number >= 0'),
                            (dict(ins_soft_weight=-0.5), 'ins_soft_weight must be a finite number >= 0'),
                            (dict(ins_soft_weight=float('nan')), 'ins_soft_weight must be'),
                            (dict(ins_hard_weight=1.0, ins_tau=0.0), 'ins_tau must be a finite number > 0'),
                            (dict(ins_tau=-1.0), 'ins_tau must be'),                       # checked with the weights at 0 too
                            (dict(ins_teacher_tau=0.0), 'ins_teacher_tau must be a finite number > 0')):
            with pytest.raises(ValueError, match='%s: %s' % (cls.__name__, pattern)):
                cls(None, None, None, None, crit(), crit(), None, teacher=t, soft_weight=0.5, **kw)


def test_signatures_and_exports():
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'dropin'))
    import reid
    import grl_amd.reid.loss as L
    assert reid.loss.InstanceContrastLoss is L.InstanceContrastLoss and 'InstanceContrastLoss' in L.__all__
    p = inspect.signature(L.InstanceContrastLoss.__init__).parameters
    assert p['tau'].default == 0.1 and p['teacher_tau'].default is None
    p = inspect.signature(L.InstanceContrastLoss.forward).parameters
    assert list(p)[1:] == ['feat', 'id', 'teacher', 'hard_weight', 'soft_weight']
    assert p['hard_weight'].default == 1.0 and p['soft_weight'].default == 0.0
    for cls, _ in _trainers():
        names = list(inspect.signature(cls.__init__).parameters)
        at = names.index('tri_soft_weight')
        assert names[at + 1:at + 5] == ['ins_hard_weight', 'ins_soft_weight', 'ins_tau', 'ins_teacher_tau'], cls.__name__
        p = inspect.signature(cls.__init__).parameters
        assert p['ins_hard_weight'].default == 0.0 and p['ins_soft_weight'].default == 0.0
        assert p['ins_tau'].default == 0.1 and p['ins_teacher_tau'].default is None


def test_tri_loss_adds_the_instance_term_only_with_a_weight(monkeypatch):
    from grl_amd.reid.train import trainer as T
    from grl_amd.reid.train import MeanTeacherSEQTrainer
    monkeypatch.setattr(T, 'criterion_triplet', lambda f, y: torch.arange(f.size(0), dtype=torch.float32))
    f, y = torch.zeros((4, 8)), torch.zeros(4, dtype=torch.int64)
    mt = object.__new__(MeanTeacherSEQTrainer)
    mt.tri_soft_weight = 0.0
    seen = []
    mt.criterion_ins = lambda feats, target, teacher=None, hard_weight=1.0, soft_weight=0.0: (
        seen.append((feats, target, teacher, hard_weight, soft_weight)) or torch.full((4,), 2.0))
    mt.ins_hard_weight, mt.ins_soft_weight = 0.0, 0.0
    assert float(mt._tri_loss(f, y)) == 1.5 and not seen                  # the parent's term, nothing called
    mt._teacher_rows = {('corr', 'clip'): 'rows'}
    mt.ins_hard_weight, mt.ins_soft_weight = 1.0, 0.4
    assert float(mt._tri_loss(f, y)) == 3.5 and seen == [(f, y, 'rows', 1.0, 0.4)]
    mt.ins_hard_weight = 0.0                                                # the soft term alone
    assert float(mt._tri_loss(f, y)) == 3.5 and seen[1][3:] == (0.0, 0.4)


def test_example_refuses_the_instance_flags_without_a_mean_teacher():
    spec = importlib.util.spec_from_file_location('train_unsupervised_synthetic',
                                                  os.path.join(ROOT, 'examples', 'train_unsupervised_synthetic.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    base = dict(camera_proxies=False, hybrid_memory=False, self_paced=None, mean_teacher=None, soft_weight=None, eval_teacher=False)
    ex.refuse_conflicts(argparse.Namespace(**base))                         # a Namespace without the attributes
    ex.refuse_conflicts(argparse.Namespace(**dict(base, ins_hard_weight=None, ins_soft_weight=None, ins_tau=None)))
    ex.refuse_conflicts(argparse.Namespace(**dict(base, mean_teacher=0.999, soft_weight=0.5, ins_hard_weight=1.0, ins_soft_weight=0.4,
                                                  ins_tau=0.05)))
    for flag, opt in (('ins_hard_weight', '--ins-hard-weight'), ('ins_soft_weight', '--ins-soft-weight'), ('ins_tau', '--ins-tau')):
        with pytest.raises(SystemExit, match=opt + ' needs --mean-teacher'):
            ex.refuse_conflicts(argparse.Namespace(**dict(base, **{flag: 0.5})))
    assert '--ins-hard-weight 1 --ins-soft-weight 0.4' in ex.__doc__


# ----------------------------------------------------------------------------------------------------------------------
# the C ABI
def test_header_binding_and_library_carry_the_entry_points():
    from grl_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'grl_hip.h')).read()
    assert re.search(r'int\s+grl_ins_contrast_fwd\(const float\* feat, const float\* tfeat, const int64_t\* ids, int n, int D, float tau, '
                     r'float tau_t,\s+float w_hard, float w_soft, float\* loss, float\* cos, int32_t\* sel, float\* coef, void\* stream\);', src)
    assert re.search(r'int\s+grl_ins_contrast_bwd\(const float\* feat, const float\* tfeat, const float\* coef, const float\* dloss, float tau, '
                     r'float\* dfeat,\s+int n, int D, void\* stream\);', src)
    assert int(re.search(r'#define\s+GRL_ABI_VERSION\s+(\d+)', src).group(1)) == _lib.ABI_VERSION
    assert {'grl_ins_contrast_fwd', 'grl_ins_contrast_bwd'} <= set(_lib.exported_symbols())
    mk = open(os.path.join(ROOT, 'grl_amd', 'csrc', 'Makefile')).read()
    assert 'ins_contrast.hip' in mk and '-ffp-contract=off' in mk
    body = open(os.path.join(ROOT, 'grl_amd', 'csrc', 'ins_contrast.hip')).read()
    assert 'atomic' not in body.replace('no atomics', '') and 'asm' not in body
    assert 'INS_MAX_N = %d' % S.MAX_N in body and S.MAX_N >= 1024


def test_host_argument_checks_return_einval_through_the_c_abi():
    from grl_amd import _lib
    lib = _lib.load()
    E = _lib.GRL_EINVAL
    # fake device pointers (never dereferenced: every call below is refused before the launch)

    def fwd(feat=0x1000, tfeat=0x2000, ids=0x3000, n=2, D=8, tau=0.1, tau_t=0.1, wh=1.0, ws=0.4, loss=0x4000, cos=0x5000, sel=0x6000,
            coef=0x7000):
        return lib.grl_ins_contrast_fwd(feat, tfeat, ids, n, D, C.c_float(tau), C.c_float(tau_t), C.c_float(wh), C.c_float(ws), loss,
                                        cos, sel, coef, None)
    inf, nan = float('inf'), float('nan')
    for kw in (dict(feat=None), dict(tfeat=None), dict(ids=None), dict(loss=None), dict(cos=None), dict(sel=None), dict(coef=None),
               dict(n=0), dict(n=-1), dict(n=S.MAX_N + 1), dict(D=0), dict(D=2), dict(D=6), dict(D=-4), dict(tau=0.0), dict(tau=-0.1),
               dict(tau=inf), dict(tau=nan), dict(tau_t=0.0), dict(tau_t=inf), dict(tau_t=nan), dict(wh=-1.0), dict(ws=-0.1),
               dict(wh=nan), dict(ws=inf), dict(wh=0.0, ws=0.0), dict(tau_t=0.0, ws=0.0)):
        assert fwd(**kw) == E, kw
        assert b'ins_contrast_fwd' in lib.grl_last_error()

    def bwd(feat=0x1000, tfeat=0x2000, coef=0x3000, dloss=0x4000, tau=0.1, dfeat=0x5000, n=2, D=8):
        return lib.grl_ins_contrast_bwd(feat, tfeat, coef, dloss, C.c_float(tau), dfeat, n, D, None)
    for kw in (dict(feat=None), dict(tfeat=None), dict(coef=None), dict(dloss=None), dict(dfeat=None), dict(n=0), dict(n=S.MAX_N + 1),
               dict(D=0), dict(D=6), dict(tau=0.0), dict(tau=nan), dict(tau=inf)):
        assert bwd(**kw) == E, kw
        assert b'ins_contrast_bwd' in lib.grl_last_error()
