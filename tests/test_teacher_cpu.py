"""The float64 model of the soft cross entropy (tests/teacher_ref.py) is right, its bounds are satisfiable and the host side
of the mean teacher keeps its books -- all shown without a GPU:

* the model against torch float64 autograd: the loss, its gradient in the student's logits, no gradient in the teacher's;
* the fp32 numpy restatement of the kernel's order inside the very bounds the GPU test holds the kernel to, and with w = 0
  equal to the restatement of grl_softmax_ce bit for bit;
* the alpha ramp, the table's chunk counts, and every refusal that fires before a device call (CPU tensors, and fake pointers
  through the C ABI as test_cmem_cpu.py)."""
import argparse
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import loss_bounds as LB
import loss_ref as LR
import teacher_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    yield
    R.dump_ratios('fp32 numpy restatement of the soft cross entropy (CPU)')


# ----------------------------------------------------------------------------------------------------------------------
# the sweep and the model
def test_sweep_reaches_every_branch():
    assert {n for n, _, _ in R.CE_CASES} == {1, 2, 9, 33} and {c for _, c, _ in R.CE_CASES} == {1, 2, 255, 256, 257, 1030}
    assert any(p == 'none' for _, _, p in R.CE_CASES)
    assert len({R.CE_LD[0], R.CE_LD[1], R.CE_LD[2]}) == 3 and min(R.CE_LD) > 0
    d = R.in_soft_ce(33, 1030, 'mixed')
    assert d['labels'][1] == -1 and d['labels'][-1] == 1030 and np.abs(d['logits'].reshape(33, -1)[:, :1030]).max() <= 21.0
    z = d['logits'].reshape(33, d['ld'])
    assert z[0, 3] == z[0, 259] == z[0, :1030].max() and d['labels'][0] == 3 and d['labels'][2] == 259
    assert not ((R.in_soft_ce(9, 257, 'none')['labels'] >= 0) & (R.in_soft_ce(9, 257, 'none')['labels'] < 257)).any()
    for count in R.EMA_COUNTS:
        lay, nd, ns = R.ema_layout(count)
        assert len(lay) == count
        assert any(d0 % 4 for _, d0, _ in lay) == (count > 1) and any(s0 % 4 for _, _, s0 in lay) == (count > 1)
        ends_d = sorted((d0, d0 + m) for m, d0, _ in lay)
        assert all(b[0] - a[1] >= R.EMA_SENT for a, b in zip(ends_d, ends_d[1:])) and ends_d[-1][1] + R.EMA_SENT <= nd
    assert set(R.EMA_NUMEL) <= {m for m, _, _ in R.ema_layout(37)[0]}
    assert any(m >= R.EMA_CHUNK and d0 % 4 == 0 and s0 % 4 == 0 for m, d0, s0 in R.ema_layout(37)[0])      # the 16-byte path
    assert R.chunk_first([1, 4096, 4097, 12291]).tolist() == [0, 1, 2, 4, 8]


@pytest.mark.parametrize('w', (0.0,) + R.CE_W)
@pytest.mark.parametrize('n,c,pattern', [(9, 257, 'mixed'), (2, 2, 'mixed'), (33, 255, 'mixed'), (9, 257, 'none'), (1, 1, 'mixed')])
def test_model_against_torch_float64_autograd(n, c, pattern, w):
    d = R.in_soft_ce(n, c, pattern)
    ref = R.soft_ce(d['logits'], d['ld'], d['tlogits'], d['ldt'], d['labels'], w, n, c)
    z = torch.from_numpy(d['logits'].astype(np.float64).reshape(n, d['ld'])[:, :c].copy()).requires_grad_(True)
    tz = torch.from_numpy(d['tlogits'].astype(np.float64).reshape(n, d['ldt'])[:, :c].copy()).requires_grad_(True)
    y = torch.from_numpy(d['labels'])
    loss = R.torch_soft_ce(z, tz.detach(), y, w)                   # the teacher carries no gradient
    assert abs(ref['loss'] - loss.item()) < 1e-12 * (1 + abs(loss.item()))
    gz, gt = torch.autograd.grad(loss, (z, tz), allow_unused=True)
    assert gt is None
    assert np.abs(ref['dz_val'] - gz.numpy()).max() < 1e-13
    invalid = ~ref['ok']
    assert not ref['dz_val'][invalid].any() and not ref['rows'][invalid].any()
    if pattern == 'none':
        assert ref['loss'] == 0.0 and ref['correct'] == 0.0 and ref['nv'] == 0
    # the cross-entropy form and the KL form differ by the teacher's entropy alone
    if w > 0 and ref['nv']:
        ent = -(ref['q'] * np.log(ref['q'])).sum(1)
        kl = (ref['q'] * (np.log(ref['q']) - np.log(ref['p']))).sum(1)
        hard = ref['lse'] - ref['ty']
        assert np.abs(ref['L'] - ((1 - w) * hard + w * (kl + ent)))[ref['ok']].max() < 1e-9


@pytest.mark.parametrize('n,c,pattern', R.CE_CASES)
def test_first_arg_max_wins_the_planted_tie(n, c, pattern):
    d = R.in_soft_ce(n, c, pattern)
    ref = R.soft_ce(d['logits'], d['ld'], d['tlogits'], d['ldt'], d['labels'], 0.5, n, c)
    z = d['logits'].reshape(n, d['ld'])[:, :c]
    want = sum(1 for i in range(n) if 0 <= d['labels'][i] < c and int(np.flatnonzero(z[i] == z[i].max())[0]) == d['labels'][i])
    assert ref['correct'] == want
    if pattern == 'mixed' and c >= 2:
        assert d['labels'][0] == R.ce_tie(c)[0] and want >= 1                  # the tie on the label's side: a hit
        if n >= 9:                                                           # the label on the second of the two: no hit
            assert d['labels'][2] == R.ce_tie(c)[1] and (z[2] == z[2].max()).sum() == 2


@pytest.mark.parametrize('n,c,pattern', R.CE_CASES)
def test_fp32_restatement_is_inside_the_bounds(n, c, pattern):
    d = R.in_soft_ce(n, c, pattern)
    for w in R.CE_W:
        ref = R.soft_ce(d['logits'], d['ld'], d['tlogits'], d['ldt'], d['labels'], w, n, c)
        got = R.soft_ce_f32(d['logits'], d['ld'], d['tlogits'], d['ldt'], d['labels'], w, n, c)
        bd = R.b_soft_ce(ref, n, c)
        what = (n, c, pattern, w)
        R.check('soft_ce loss', got['loss'], ref['loss'], bd['loss'], what)
        R.check('soft_ce dz', got['dz'], ref['dz_val'], bd['dz'], what)
        assert got['correct'] == ref['correct'], what
        assert not got['dz'][~ref['ok']].any() and not np.signbit(got['dz'][~ref['ok']]).any()
        assert np.isfinite(bd['dz']).all() and bd['dz'].max() < 1e-4 and bd['loss'] < 1e-3       # the bounds bound something


@pytest.mark.parametrize('n,c,pattern', R.CE_CASES)
def test_weight_zero_is_the_plain_cross_entropy(n, c, pattern):
    d = R.in_soft_ce(n, c, pattern)
    ref = R.soft_ce(d['logits'], d['ld'], None, 0, d['labels'], 0.0, n, c)
    plain = LR.softmax_ce(d['logits'], d['ld'], d['labels'], None, n, c)
    assert abs(ref['loss'] - plain['loss']) < 1e-12 and np.abs(ref['dz_val'] - plain['dz_val']).max() < 1e-15
    assert ref['correct'] == plain['correct']
    got = R.soft_ce_f32(d['logits'], d['ld'], None, 0, d['labels'], 0.0, n, c)
    p32 = LB.softmax_ce_f32(d['logits'], d['ld'], d['labels'], None, n, c)
    assert np.array_equal(np.float32(got['loss']).view(np.uint32), np.float32(p32['loss']).view(np.uint32))
    assert np.array_equal(got['dz'].view(np.uint32), p32['dz'].view(np.uint32))


# ----------------------------------------------------------------------------------------------------------------------
# the moving average on the host
def test_alpha_ramp_and_the_restatement():
    from grl_amd.reid.train.teacher import ema_alpha
    assert ema_alpha(0, 0.999) == 0.0 and ema_alpha(1, 0.999) == 0.5
    assert abs(ema_alpha(2, 0.999) - 2.0 / 3.0) < 1e-15
    assert ema_alpha(998, 0.999) < 0.999 and ema_alpha(999, 0.999) == 0.999 and ema_alpha(10 ** 6, 0.999) == 0.999
    assert ema_alpha(5, 0.0) == 0.0 and ema_alpha(1, 0.3) == 0.3
    for step in (0, 1, 2, 7, 5000):
        a, b = R.ema_alpha(step, 0.999)
        assert a == np.float32(ema_alpha(step, 0.999)) and b == np.float32(1.0 - ema_alpha(step, 0.999))
    d = R.in_ema(37)
    inside = np.zeros(d['dst'].size, bool)
    src_at = np.zeros(d['dst'].size, np.float32)                 # the src element that meets every dst element
    for numel, d0, s0 in d['layout']:
        inside[d0:d0 + numel] = True
        src_at[d0:d0 + numel] = d['src'][s0:s0 + numel]
    finite = inside & np.isfinite(src_at)
    copy, keep, half = R.ema_expected(d, 0.0, 1.0), R.ema_expected(d, 1.0, 0.0), R.ema_expected(d, 0.5, 0.5)
    assert np.array_equal(copy[finite], src_at[finite])                               # alpha = 0 copies
    assert np.array_equal(keep[finite], d['dst'][finite])                             # alpha = 1 keeps (src finite)
    assert np.isnan(keep[inside & ~finite]).all() and (inside & ~finite).sum() == 2   # 0 inf and 0 NaN are NaN
    assert np.isnan(half[np.isnan(src_at)]).all() and np.isinf(half[np.isinf(src_at)]).all()
    for out in (copy, keep, half):
        assert (out[~inside] == R.EMA_SENTINEL).all()
    assert np.isnan(d['src']).sum() == 1 and np.isinf(d['src']).sum() == 1


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(6, 4)
        self.bn = torch.nn.BatchNorm1d(4)


def test_ema_tensors_take_float_parameters_and_buffers_and_leave_integer_buffers():
    from grl_amd.reid.train import teacher as T
    s, t = _Net(), _Net()
    names = [n for n, _, _ in T.ema_tensors(s, t)]
    assert names == ['fc.weight', 'fc.bias', 'bn.weight', 'bn.bias', 'bn.running_mean', 'bn.running_var']
    arr, first, count = T.ema_table([('a', torch.zeros(5000), torch.zeros(5000)), ('e', torch.zeros(0), torch.zeros(0)),
                                     ('b', torch.zeros(3), torch.zeros(3))])
    assert count == 2 and first == [0, 2, 3] and arr[0].numel == 5000 and arr[1].numel == 3
    assert C.sizeof(T.GrlEmaEntry) == 24


def test_mean_teacher_refusals_fire_before_any_device_call(monkeypatch):
    from grl_amd import engine
    from grl_amd.reid.train import teacher as T

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    monkeypatch.setattr(engine, '_call', no_device)
    monkeypatch.setattr(T, '_call', no_device)
    for alpha in (1.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match=r'alpha must be in \[0, 1\)'):
            T.MeanTeacher(_Net(), _Net(), alpha=alpha)
    with pytest.raises(ValueError, match="teacher tensor 'fc.weight' must be on a HIP device .got cpu"):
        T.MeanTeacher(_Net(), _Net())
    a, b = torch.zeros((4, 6)), torch.zeros((4, 6))
    with pytest.raises(ValueError, match="teacher tensor 'w' must be float32 .got torch.float64"):
        T.check_ema_pairs([('w', a.double(), b)])
    with pytest.raises(ValueError, match="student tensor 'w' must be float32 .got torch.float16"):
        T.check_ema_pairs([('w', a, b.half())])
    with pytest.raises(ValueError, match="student tensor 'w' must be contiguous"):
        T.check_ema_pairs([('w', torch.zeros((6, 4)), torch.zeros((4, 6)).t())])
    with pytest.raises(ValueError, match=r"tensor 'w' is \(4, 6\) in the teacher and \(6, 4\) in the student"):
        T.check_ema_pairs([('w', a, torch.zeros((6, 4)))])
    with pytest.raises(ValueError, match="teacher tensor 'w' shares its storage with the student tensor 'w'"):
        T.check_ema_pairs([('w', a, a)])
    big = torch.zeros(48)
    with pytest.raises(ValueError, match="teacher tensor 'v' shares its storage with the student tensor 'w'"):
        T.check_ema_pairs([('w', a, big[:24].view(4, 6)), ('v', big[24:].view(4, 6), b)])
    with pytest.raises(ValueError, match="teacher tensors 'w' and 'v' overlap in memory"):
        T.check_ema_pairs([('w', big[:24], a.view(-1)), ('v', big[12:36], b.view(-1))])
    with pytest.raises(ValueError, match="teacher tensor 'w' must be on a HIP device .got cpu"):
        T.check_ema_pairs([('w', a, b)])                                      # everything else in order: the device is last


def test_criterion_and_trainer_refusals_fire_before_any_device_call(monkeypatch):
    from grl_amd import engine, train_graph
    from grl_amd.reid.loss import ClusterMemoryLoss, SoftClusterMemoryLoss, memory
    from grl_amd.reid.train import MeanTeacher, MeanTeacherSEQTrainer

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    for mod, name in ((engine, '_call'), (engine, 'gemm'), (memory, '_call')):
        monkeypatch.setattr(mod, name, no_device)
    assert issubclass(SoftClusterMemoryLoss, ClusterMemoryLoss)
    crit = SoftClusterMemoryLoss(16, 4, temp=0.05, momentum=0.2, mode='mean')
    assert crit.mode == 'mean' and tuple(crit.centroids.shape) == (4, 16)
    x, y = torch.zeros((6, 16)), torch.zeros(6, dtype=torch.int64)
    for bad, pattern in ((torch.zeros((5, 16)), r'teacher must be \[n, D\] = \(6, 16\), the shape of the inputs .got \(5, 16\)'),
                         (torch.zeros((6, 16, 1)), r'teacher must be \[n, D\]'),
                         (torch.zeros((6, 16), dtype=torch.float64), 'teacher must be float32 .got torch.float64'),
                         (torch.zeros((6, 16), device='meta'), 'teacher must be on the device of the inputs, cpu .got meta'),
                         (torch.zeros((6, 16), requires_grad=True), 'teacher must carry no gradient'),
                         (np.zeros((6, 16), np.float32), 'teacher must be a tensor .got ndarray')):
        with pytest.raises(ValueError, match='SoftClusterMemoryLoss: ' + pattern):
            crit(x, y, teacher=bad, soft_weight=0.5)
    for w in (-0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match=r'soft_weight must be in \[0, 1\]'):
            crit(x, y, teacher=torch.zeros((6, 16)), soft_weight=w)
    # the trainer: both identity criteria, named; the teacher; the weight
    plain, soft, soft2 = ClusterMemoryLoss(16, 4), SoftClusterMemoryLoss(16, 4), SoftClusterMemoryLoss(16, 4)
    with pytest.raises(ValueError, match='criterion_corr must be a SoftClusterMemoryLoss .got ClusterMemoryLoss'):
        MeanTeacherSEQTrainer(None, None, None, None, plain, soft, None, teacher=None)
    with pytest.raises(ValueError, match='criterion_uncorr must be a SoftClusterMemoryLoss .got ClusterMemoryLoss'):
        MeanTeacherSEQTrainer(None, None, None, None, soft, plain, None, teacher=None)
    with pytest.raises(ValueError, match='must be two objects'):
        MeanTeacherSEQTrainer(None, None, None, None, soft, soft, None, teacher=None)
    with pytest.raises(ValueError, match='teacher must be a MeanTeacher .got NoneType'):
        MeanTeacherSEQTrainer(None, None, None, None, soft, soft2, None, teacher=None)
    t = object.__new__(MeanTeacher)
    with pytest.raises(ValueError, match=r'soft_weight must be in \[0, 1\] .got 2'):
        MeanTeacherSEQTrainer(None, None, None, None, soft, soft2, None, teacher=t, soft_weight=2)
    # a captured step has no place for the teacher
    tr = object.__new__(MeanTeacherSEQTrainer)
    with pytest.raises(ValueError, match='GraphedTrainStep does not capture a MeanTeacherSEQTrainer'):
        train_graph.GraphedTrainStep(tr, None, None, None)


def test_the_packages_export_the_new_classes():
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'dropin'))
    import reid
    import grl_amd.reid.loss as L
    import grl_amd.reid.train as T
    assert reid.loss.SoftClusterMemoryLoss is L.SoftClusterMemoryLoss and 'SoftClusterMemoryLoss' in L.__all__
    assert reid.train.MeanTeacher is T.MeanTeacher and reid.train.MeanTeacherSEQTrainer is T.MeanTeacherSEQTrainer
    assert 'MeanTeacherSEQTrainer' in (T.train_unsupervised.__doc__ or '')


def test_example_refuses_flag_combinations_with_a_message():
    spec = importlib.util.spec_from_file_location('train_unsupervised_synthetic',
                                                  os.path.join(ROOT, 'examples', 'train_unsupervised_synthetic.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    base = dict(camera_proxies=False, hybrid_memory=False, self_paced=None, mean_teacher=None, soft_weight=None, eval_teacher=False)
    ex.refuse_conflicts(argparse.Namespace(**base))
    ex.refuse_conflicts(argparse.Namespace(**dict(base, mean_teacher=0.999, soft_weight=0.5, eval_teacher=True)))
    for kw, pattern in ((dict(mean_teacher=0.999, camera_proxies=True), 'excludes --camera-proxies'),
                        (dict(mean_teacher=0.999, hybrid_memory=True), 'excludes --camera-proxies and --hybrid-memory'),
                        (dict(soft_weight=0.5), 'need --mean-teacher'), (dict(eval_teacher=True), 'need --mean-teacher')):
        with pytest.raises(SystemExit, match=pattern):
            ex.refuse_conflicts(argparse.Namespace(**dict(base, **kw)))


# ----------------------------------------------------------------------------------------------------------------------
# the C ABI
def test_header_binding_and_library_carry_the_entry_points():
    from grl_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'grl_hip.h')).read()
    assert re.search(r'int\s+grl_ema_update\(const GrlEmaEntry\* table_dev, const int64_t\* chunk_first_dev, int count,\s+'
                     r'float alpha, float one_minus_alpha, void\* stream\);', src)
    assert re.search(r'int\s+grl_soft_ce\(const float\* logits, int64_t ld, const float\* tlogits, int64_t ldt, const int64_t\* '
                     r'labels,\s+float w_soft, int n, int c, float\* loss, float\* correct, float\* dlogits, int64_t ldd,\s+'
                     r'float\* ws, void\* stream\);', src)
    assert int(re.search(r'#define\s+GRL_EMA_CHUNK\s+(\d+)', src).group(1)) == R.EMA_CHUNK == _lib.EMA_CHUNK
    assert int(re.search(r'#define\s+GRL_ABI_VERSION\s+(\d+)', src).group(1)) == 10 == _lib.ABI_VERSION
    assert {'grl_ema_update', 'grl_soft_ce'} <= set(_lib.exported_symbols())
    mk = open(os.path.join(ROOT, 'grl_amd', 'csrc', 'Makefile')).read()
    assert 'ema.hip' in mk and 'softce.hip' in mk and re.search(r'softce\.o[^\n]*: ce_finish\.h', mk)


def test_host_argument_checks_return_einval_through_the_c_abi():
    from grl_amd import _lib
    lib = _lib.load()
    E = _lib.GRL_EINVAL
    # fake device pointers (never dereferenced: every call below is refused before the launch)

    def ema(table=0x1000, first=0x2000, count=3, a=0.5, b=0.5):
        return lib.grl_ema_update(table, first, count, C.c_float(a), C.c_float(b), None)
    for kw in (dict(table=None), dict(first=None), dict(count=0), dict(count=-1)):
        assert ema(**kw) == E, kw
        assert b'ema_update' in lib.grl_last_error()

    def ce(logits=0x1000, ld=8, tlogits=0x2000, ldt=8, labels=0x3000, w=0.5, n=2, c=8, loss=0x4000, correct=0x5000, dl=0x6000,
           ldd=8, ws=0x7000):
        return lib.grl_soft_ce(logits, ld, tlogits, ldt, labels, C.c_float(w), n, c, loss, correct, dl, ldd, ws, None)
    for kw in (dict(logits=None), dict(labels=None), dict(loss=None), dict(ws=None), dict(n=0), dict(n=-1), dict(c=0), dict(ld=7),
               dict(ldd=7), dict(w=-0.01), dict(w=1.01), dict(w=float('nan')), dict(tlogits=None), dict(ldt=7),
               dict(tlogits=None, w=1.0)):
        assert ce(**kw) == E, kw
        assert b'soft_ce' in lib.grl_last_error()
