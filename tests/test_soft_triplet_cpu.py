"""The float64 model of the soft softmax-triplet loss (tests/soft_triplet_ref.py) is MMT's SoftTripletLoss, its
bounds are satisfiable by an fp32 restatement in the kernels' order, the sweep's teacher rows exercise the soft term, and
every refusal of SoftTripletLoss / MeanTeacherSEQTrainer(tri_soft_weight=) / the example fires without a device.  No GPU."""
import argparse
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import soft_triplet_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    yield
    S.dump_ratios('soft triplet, fp32 restatement on the CPU')


# ----------------------------------------------------------------------------------------------------------------------
# the model is MMT's loss
def _mmt_soft_triplet(f, tf, ids, w):
    """MMT's SoftTripletLoss written out (Ge et al. 2020, mmt/loss/triplet.py): batch-hard indices from the student's
    distance matrix, log-softmax over (d_ap, d_an), against the hard order (margin 0: -log p_an) and against the softmax of
    the teacher's distances gathered at the same indices; blended (1 - w) hard + w soft.  Per anchor, not averaged."""
    def euclid(x):
        d = x[:, None, :] - x[None, :, :]
        return (d * d).sum(2).add(1e-12).sqrt()
    sim = (ids[:, None] == ids[None, :]).to(f.dtype)
    dist = euclid(f)
    d_ap, ap_idx = (dist + (-9999999.0) * (1 - sim)).max(1)
    d_an, an_idx = (dist + 9999999.0 * sim).min(1)
    logp = torch.log_softmax(torch.stack((d_ap, d_an), 1), 1)
    hard = -logp[:, 1]
    dist_t = euclid(tf)
    ref = torch.softmax(torch.stack((dist_t.gather(1, ap_idx[:, None])[:, 0], dist_t.gather(1, an_idx[:, None])[:, 0]), 1), 1).detach()
    soft = -(ref * logp).sum(1)
    return (1 - w) * hard + w * soft


def _both_sides(ids):
    same = ids[:, None] == ids[None, :]
    return bool(((same.sum(1) > 1) & ((~same).sum(1) > 0)).all())


EXTRA_IDS = {5: np.array([0, 0, 1, 1, 1], np.int64), 9: np.array([0, 0, 0, 1, 1, 1, 2, 2, 2], np.int64)}
MODEL_CASES = [(n, D, cls, pattern) for n, D in S.TRI_CASES for pattern in S.TRI_IDS for cls in ('a', 'b')
               if _both_sides(S.B.tri_ids(n, pattern))] + [(n, D, cls, 'extra') for n in EXTRA_IDS for D in (4, 260) for cls in ('a', 'b')]


def test_model_cases_are_there():
    assert len(MODEL_CASES) >= 18 and any(p != 'extra' for _, _, _, p in MODEL_CASES)


@pytest.mark.parametrize('n,D,cls,pattern', MODEL_CASES)
def test_model_against_torch_float64_autograd_of_mmt(n, D, cls, pattern):
    d = S.in_soft_triplet(n, D, cls, 'pairs' if pattern == 'extra' else pattern)
    if pattern == 'extra':
        d['ids'] = EXTRA_IDS[n]
    for w in S.W_SOFT:
        full, m, bw = S.soft_triplet_full(d['f'], d['tf'], d['ids'], w, n, D, d['dloss'])
        assert full['sel'].reshape(n, 2).min() >= 0 and not m['same_n'].any()
        f = torch.from_numpy(d['f'].astype(np.float64)).requires_grad_(True)
        tf = torch.from_numpy(d['tf'].astype(np.float64)).requires_grad_(True)
        loss = _mmt_soft_triplet(f, tf, torch.from_numpy(d['ids']), S.w_of(w))
        (loss * torch.from_numpy(d['dloss'].astype(np.float64))).sum().backward()
        assert np.abs(loss.detach().numpy() - m['loss']).max() < 1e-10, (w, np.abs(loss.detach().numpy() - m['loss']).max())
        assert np.abs(f.grad.numpy() - bw['df']).max() < 1e-10, (w, np.abs(f.grad.numpy() - bw['df']).max())
        assert tf.grad is None or not tf.grad.any()                           # the teacher gets no gradient
        if S.w_of(w) == 0:                                                    # today's loss
            assert np.array_equal(m['loss'], full['loss'])


# ----------------------------------------------------------------------------------------------------------------------
# the fp32 restatement lies inside the bounds
@pytest.mark.parametrize('pattern', S.TRI_IDS)
@pytest.mark.parametrize('n,D', S.TRI_CASES)
def test_fp32_restatement_is_inside_the_bounds(n, D, pattern):
    for cls in S.TRI_CLASSES:
        d = S.in_soft_triplet(n, D, cls, pattern)
        hard = S.soft_triplet_f32(d['f'], d['tf'], d['ids'], d['dloss'], 0.0, n, D)
        for w in S.W_SOFT:
            what = (n, D, pattern, cls, w)
            got = S.soft_triplet_f32(d['f'], d['tf'], d['ids'], d['dloss'], w, n, D)
            assert np.isfinite(got['loss']).all() and np.isfinite(got['df']).all(), what
            for k in ('dist', 'sel', 'z'):                                    # the student part does not depend on w
                assert np.array_equal(got[k], hard[k]), (k, what)
            if S.w_of(w) != 0:
                assert ((got['q'] >= 0) & (got['q'] <= 1)).all(), what
                S.check('teacher dist', got['td'], S.triplet_dist(d['tf'], n, D)['dist'],
                        S.b_tri_dist(S.triplet_dist(d['tf'], n, D), D), what)
            S.check_stagewise(got, d, w, n, D, what)
            if cls == 'a':
                assert S.check_end_to_end(got, d, w, n, D, what), what


def test_the_teacher_rows_exercise_the_soft_term():
    """class (a), float64 selection: anchors with a positive and a different-id negative exist on both sides of q = 0.5 by a
    margin, and every case meets the gap condition (the GPU test compares sel with the float64 selection there)"""
    both = lo = hi = cases = 0
    for n, D in S.TRI_CASES:
        for pattern in S.TRI_IDS:
            d = S.in_soft_triplet(n, D, 'a', pattern)
            full, m, _ = S.soft_triplet_full(d['f'], d['tf'], d['ids'], 0.8, n, D, d['dloss'])
            assert S.tri_gap_ok(full, S.e_tri_dist(full, D)), (n, D, pattern)
            live = m['has_pos'] & ~m['same_n']
            both += int(live.sum()); lo += int((m['q'][live] < 0.3).sum()); hi += int((m['q'][live] > 0.7).sum())
            cases += 1
            # an anchor without a different-id negative: the mirrored mask drives q to 0
            assert (m['q'][m['same_n']] == 0).all()
            # class (t): the duplicated student rows have different teacher rows
            t = S.in_soft_triplet(n, D, 't', pattern)
            if n >= 2:
                assert np.array_equal(t['f'][1], t['f'][0]) and not np.array_equal(t['tf'][1], t['tf'][0])
    assert cases == 120 and both > 0 and lo > 0 and hi > 0, (cases, both, lo, hi)
    print('anchors with both sides %d, q < 0.3: %d, q > 0.7: %d' % (both, lo, hi))


# ----------------------------------------------------------------------------------------------------------------------
# the Python surface
def _no_device(*a, **k):
    raise AssertionError('a device call was made')


def test_refusals_fire_before_any_device_call(monkeypatch):
    from grl_amd import engine
    from grl_amd.reid.loss import SoftTripletLoss, SoftClusterMemoryLoss, soft_triplet, triplet
    from grl_amd.reid.train import MeanTeacher, MeanTeacherSEQTrainer
    for mod, name in ((engine, '_call'), (soft_triplet, '_call'), (triplet, '_call')):
        monkeypatch.setattr(mod, name, _no_device)
    crit = SoftTripletLoss()
    x, y = torch.zeros((6, 16)), torch.zeros(6, dtype=torch.int64)
    for bad, pattern in ((torch.zeros((5, 16)), r'teacher must be \[n, D\] = \(6, 16\), the shape of the inputs .got \(5, 16\)'),
                         (torch.zeros((6, 16, 1)), r'teacher must be \[n, D\]'),
                         (torch.zeros((6, 16), dtype=torch.float64), 'teacher must be float32 .got torch.float64'),
                         (torch.zeros((6, 16), device='meta'), 'teacher must be on the device of the inputs, cpu .got meta'),
                         (torch.zeros((6, 16), requires_grad=True), 'teacher must carry no gradient'),
                         (np.zeros((6, 16), np.float32), 'teacher must be a tensor .got ndarray')):
        with pytest.raises(ValueError, match='SoftTripletLoss: ' + pattern):
            crit(x, y, teacher=bad, soft_weight=0.8)
    for w in (-0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match=r'SoftTripletLoss: soft_weight must be in \[0, 1\]'):
            crit(x, y, teacher=torch.zeros((6, 16)), soft_weight=w)
    soft, soft2 = SoftClusterMemoryLoss(16, 4), SoftClusterMemoryLoss(16, 4)
    t = object.__new__(MeanTeacher)
    for w in (2, -0.5, float('nan')):
        with pytest.raises(ValueError, match=r'MeanTeacherSEQTrainer: tri_soft_weight must be in \[0, 1\] .got'):
            MeanTeacherSEQTrainer(None, None, None, None, soft, soft2, None, teacher=t, soft_weight=0.5, tri_soft_weight=w)


def test_seqtrainer_tri_loss_reads_the_module_global_when_called(monkeypatch):
    from grl_amd.reid.train import trainer as T
    from grl_amd.reid.train import MeanTeacherSEQTrainer
    calls = []

    def stub(f, y):
        calls.append((f, y))
        return torch.arange(f.size(0), dtype=torch.float32)
    monkeypatch.setattr(T, 'criterion_triplet', stub)
    tr = object.__new__(T.SEQTrainer)
    f, y = torch.zeros((4, 8)), torch.zeros(4, dtype=torch.int64)
    assert float(tr._tri_loss(f, y)) == 1.5 and len(calls) == 1 and calls[0][0] is f and calls[0][1] is y
    # the mean-teacher trainer with the default weight goes the same way; with a weight it calls the loss it owns
    mt = object.__new__(MeanTeacherSEQTrainer)
    mt.tri_soft_weight = 0.0
    assert float(mt._tri_loss(f, y)) == 1.5 and len(calls) == 2
    seen = []
    mt.tri_soft_weight = 0.8
    mt._teacher_rows = {('corr', 'clip'): 'rows'}
    mt.criterion_soft_triplet = lambda feats, target, teacher=None, soft_weight=0.0: (
        seen.append((feats, target, teacher, soft_weight)) or torch.full((4,), 2.0))
    assert float(mt._tri_loss(f, y)) == 2.0 and len(calls) == 2
    assert seen == [(f, y, 'rows', 0.8)]


def test_the_packages_export_the_new_class():
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'dropin'))
    import reid
    import grl_amd.reid.loss as L
    assert reid.loss.SoftTripletLoss is L.SoftTripletLoss and 'SoftTripletLoss' in L.__all__
    import inspect
    from grl_amd.reid.train import MeanTeacherSEQTrainer
    assert inspect.signature(MeanTeacherSEQTrainer.__init__).parameters['tri_soft_weight'].default == 0.0


def test_example_refuses_soft_tri_weight_without_a_mean_teacher():
    spec = importlib.util.spec_from_file_location('train_unsupervised_synthetic',
                                                  os.path.join(ROOT, 'examples', 'train_unsupervised_synthetic.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    base = dict(camera_proxies=False, hybrid_memory=False, self_paced=None, mean_teacher=None, soft_weight=None, eval_teacher=False)
    ex.refuse_conflicts(argparse.Namespace(**base))                           # a Namespace without the attribute
    ex.refuse_conflicts(argparse.Namespace(**dict(base, soft_tri_weight=None)))
    ex.refuse_conflicts(argparse.Namespace(**dict(base, mean_teacher=0.999, soft_weight=0.5, soft_tri_weight=0.8)))
    with pytest.raises(SystemExit, match='--soft-tri-weight needs --mean-teacher'):
        ex.refuse_conflicts(argparse.Namespace(**dict(base, soft_tri_weight=0.8)))
    assert '--soft-tri-weight 0.8' in ex.__doc__


# ----------------------------------------------------------------------------------------------------------------------
# the C ABI
def test_header_binding_and_library_carry_the_entry_points():
    from grl_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'grl_hip.h')).read()
    assert re.search(r'int\s+grl_soft_triplet_fwd\(const float\* feat, const float\* tfeat, const int64_t\* ids, int n, int D, '
                     r'float w_soft,\s+float\* loss, float\* dist, int32_t\* sel, float\* z, float\* q, void\* stream\);', src)
    assert re.search(r'int\s+grl_soft_triplet_bwd\(const float\* feat, const float\* dist, const int32_t\* sel, const float\* z, '
                     r'const float\* q,\s+const float\* dloss, float w_soft, float\* dfeat, int n, int D, void\* stream\);', src)
    assert int(re.search(r'#define\s+GRL_ABI_VERSION\s+(\d+)', src).group(1)) == 10 == _lib.ABI_VERSION
    assert {'grl_soft_triplet_fwd', 'grl_soft_triplet_bwd'} <= set(_lib.exported_symbols())
    mk = open(os.path.join(ROOT, 'grl_amd', 'csrc', 'Makefile')).read()
    assert 'soft_triplet.hip' in mk and re.search(r'loss\.o soft_triplet\.o[^\n]*: triplet_common\.h', mk)
    # one copy of the distance-row loop and of the selection
    for name in ('loss.hip', 'soft_triplet.hip'):
        body = open(os.path.join(ROOT, 'grl_amd', 'csrc', name)).read()
        assert '#include "triplet_common.h"' in body and '1e5f * (same' not in body and 'd[0] * d[0]' not in body, name


def test_host_argument_checks_return_einval_through_the_c_abi():
    from grl_amd import _lib
    lib = _lib.load()
    E = _lib.GRL_EINVAL
    # fake device pointers (never dereferenced: every call below is refused before the launch)

    def fwd(feat=0x1000, tfeat=0x2000, ids=0x3000, n=2, D=8, w=0.8, loss=0x4000, dist=0x5000, sel=0x6000, z=0x7000, q=0x8000):
        return lib.grl_soft_triplet_fwd(feat, tfeat, ids, n, D, C.c_float(w), loss, dist, sel, z, q, None)
    for kw in (dict(feat=None), dict(ids=None), dict(loss=None), dict(dist=None), dict(sel=None), dict(z=None), dict(n=0), dict(n=-1),
               dict(n=16385), dict(D=6), dict(D=0), dict(w=-0.01), dict(w=1.01), dict(w=float('nan')), dict(tfeat=None),
               dict(q=None), dict(tfeat=None, w=1.0)):
        assert fwd(**kw) == E, kw
        assert b'soft_triplet_fwd' in lib.grl_last_error()

    def bwd(feat=0x1000, dist=0x2000, sel=0x3000, z=0x4000, q=0x5000, dloss=0x6000, w=0.8, dfeat=0x7000, n=2, D=8):
        return lib.grl_soft_triplet_bwd(feat, dist, sel, z, q, dloss, C.c_float(w), dfeat, n, D, None)
    for kw in (dict(feat=None), dict(dist=None), dict(sel=None), dict(z=None), dict(dloss=None), dict(dfeat=None), dict(n=0),
               dict(D=6), dict(w=-0.01), dict(w=1.01), dict(w=float('nan')), dict(q=None)):
        assert bwd(**kw) == E, kw
        assert b'soft_triplet_bwd' in lib.grl_last_error()
