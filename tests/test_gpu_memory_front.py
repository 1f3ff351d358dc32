"""The memory front end (grl_amd/reid/loss/memory.py) on a real MI355X: what every memory criterion launches, in order, and
the column-blocked input gradient under the criteria that reach it.

The launch sequences below are written out from the criteria as they stood before the front end existed (each its own copy
of OIM.forward / OIM.backward); they are not derived from the code under test.  Everything is compared exactly: names,
counts and bits.  n = 9 rows throughout (hybrid_ref.in_loss)."""
import numpy as np
import pytest
import torch

import hybrid_ref as R

pytestmark = pytest.mark.gpu

G = 0.75        # the gradient handed to the loss: (G * loss).backward()
D = 256
TEMP, MOMENTUM = R.LOSS_TEMP, R.LOSS_MOMENTUM
MODES = ('instance', 'hard', 'mean')

UPDATE = {'instance': 'grl_oim_update', 'hard': 'grl_cmem_update', 'mean': 'grl_cmem_update'}
# criterion -> (its cross-entropy entry point, its soft one, the backward's update)
LAUNCHES = dict([('oim', ('grl_softmax_ce', None, 'grl_oim_update')),
                 ('hybrid', ('grl_hybrid_ce', 'grl_soft_hybrid_ce', 'grl_oim_update'))] +
                [('cluster-' + m, ('grl_softmax_ce', 'grl_soft_ce', UPDATE[m])) for m in MODES] +
                [('proxy-' + m, ('grl_proxy_ce', 'grl_soft_proxy_ce', UPDATE[m])) for m in MODES])
BLOCKED = ['grl_oim_grad', 'grl_oim_grad', 'grl_axpby', 'grl_oim_update']      # 5120 < N <= 10240, 'instance'


def _inputs(N):
    """hybrid_ref.in_loss with every memory row a class of its own and index = targets (row 4: both -1): inputs every
    criterion takes, the cluster id, the proxy id and the instance index being one number"""
    d = R.in_loss(D, singletons=True, N=N)
    d['index'] = d['targets'].copy()
    d['teacher'] = R.unit_rows(R.rng_for('memory front', 'teacher', N).standard_normal(d['x'].shape))
    return d


@pytest.fixture(scope='module')
def small():
    return _inputs(R.LOSS_COLS)


@pytest.fixture(scope='module')
def wide():
    return _inputs(R.LOSS_WIDE)


def _criterion(name, d, soft=False):
    """(criterion on the device with d's memory installed, its memory tensor, the extra arguments of its call)"""
    from grl_amd.reid import loss as L
    N = d['mem'].shape[0]
    mem = torch.from_numpy(d['mem']).cuda()
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()                 # noqa: E731
    kind, _, mode = name.partition('-')
    if kind == 'oim':
        crit = L.OIMLoss(D, N, scalar=1.0 / TEMP, momentum=MOMENTUM).cuda()
        crit.lut = mem
        return crit, crit.lut, ()
    if kind == 'cluster':
        crit = (L.SoftClusterMemoryLoss if soft else L.ClusterMemoryLoss)(D, N, temp=TEMP, momentum=MOMENTUM, mode=mode).cuda()
        return crit.reset(mem), crit.centroids, ()
    if kind == 'proxy':
        crit = (L.SoftProxyMemoryLoss if soft else L.ProxyMemoryLoss)(D, temp=TEMP, momentum=MOMENTUM, mode=mode, w_inter=0.0).cuda()
        crit.reset(mem, i32(np.arange(N)), i32(np.zeros(N)))
        return crit, crit.centroids, (torch.zeros(d['x'].shape[0], dtype=torch.int64, device='cuda'),)
    crit = (L.SoftHybridMemoryLoss if soft else L.HybridMemoryLoss)(D, temp=TEMP, momentum=MOMENTUM).cuda()
    crit.reset(mem, i32(d['cp']), i32(d['cm']), i32(d['ic']))
    return crit, crit.memory, (torch.from_numpy(d['index']).cuda(),)


@pytest.fixture
def trace(monkeypatch):
    """the name of every memory._call and ('gemm', M) of every engine.gemm, recorded while the calls go through"""
    from grl_amd import engine
    from grl_amd.reid.loss import memory
    seen, call, gemm = [], memory._call, engine.gemm
    monkeypatch.setattr(memory, '_call', lambda name, *a: (seen.append(name), call(name, *a))[1])
    monkeypatch.setattr(engine, 'gemm', lambda *a, **k: (seen.append(('gemm', a[3])), gemm(*a, **k))[1])
    return seen


def _run(crit, extra, d, seen, grad=True, **soft):
    """forward and (G * loss).backward() -> (loss, logits, x, the launches of the forward, those of the backward)"""
    x = torch.from_numpy(d['x']).cuda().requires_grad_(grad)
    del seen[:]
    loss, logits = crit(x, torch.from_numpy(d['targets']).cuda(), *extra, **soft)
    fwd = list(seen)
    del seen[:]
    (loss * G).backward()
    torch.cuda.synchronize()
    return loss, logits, x, fwd, list(seen)


@pytest.mark.parametrize('name', sorted(LAUNCHES))
def test_hard_criteria_launch_one_gemm_their_cross_entropy_the_gradient_and_the_update(name, small, trace):
    ce, _, update = LAUNCHES[name]
    crit, mem, extra = _criterion(name, small)
    _, logits, x, fwd, bwd = _run(crit, extra, small, trace)
    assert fwd == [('gemm', 9), ce] and bwd == ['grl_oim_grad', update]
    assert tuple(logits.shape) == (9, 70) and bool(x.grad.abs().sum() > 0)
    assert not torch.equal(mem.cpu(), torch.from_numpy(small['mem']))


@pytest.mark.parametrize('name', sorted(n for n in LAUNCHES if n != 'oim'))
def test_soft_criteria_stack_the_teacher_into_the_one_gemm_and_fall_back_to_the_hard_launches(name, small, trace):
    ce, soft_ce, update = LAUNCHES[name]
    teacher = torch.from_numpy(small['teacher']).cuda()
    crit, _, extra = _criterion(name, small, soft=True)
    _, logits, _, fwd, bwd = _run(crit, extra, small, trace, teacher=teacher, soft_weight=0.5)
    assert fwd == [('gemm', 18), soft_ce] and bwd == ['grl_oim_grad', update]
    assert tuple(logits.shape) == (9, 70) and logits.grl_top1[1] == 9                        # the student's rows alone
    for soft in (dict(teacher=None, soft_weight=0.5), dict(teacher=teacher, soft_weight=0.0), dict()):
        crit, _, extra = _criterion(name, small, soft=True)
        fwd, bwd = _run(crit, extra, small, trace, **soft)[3:]
        assert fwd == [('gemm', 9), ce] and bwd == ['grl_oim_grad', update], soft


@pytest.mark.parametrize('name', sorted(LAUNCHES))
def test_inputs_without_a_gradient_skip_the_gradient_launch_and_still_update_the_memory(name, small, trace):
    """the backward runs because the memory tensor asks for a gradient (it gets none: the Functions return None for it)"""
    ce, _, update = LAUNCHES[name]
    crit, mem, extra = _criterion(name, small)
    mem.requires_grad_(True)
    _, _, x, fwd, bwd = _run(crit, extra, small, trace, grad=False)
    assert fwd == [('gemm', 9), ce] and bwd == [update]
    assert x.grad is None and mem.grad is None
    assert not torch.equal(mem.detach().cpu(), torch.from_numpy(small['mem']))


def test_memories_wider_than_one_gradient_launch_give_the_same_bits_from_all_four_criteria(wide, trace):
    """N = hybrid_ref.LOSS_WIDE = 5200 > 5120, the columns one grl_oim_grad launch takes, every memory row a class of its own,
    one camera, no inter-camera term: HybridMemoryLoss, ClusterMemoryLoss('instance'), ProxyMemoryLoss('instance') and OIMLoss
    give the same bits in loss, logits, dx, the top-1 count and the memory after the backward, each through two column blocks
    added by grl_axpby (test_gpu_hybrid.py anchors the hybrid one to float64; test_gpu_hybrid.py and test_gpu_proxy.py hold
    the same equalities at N <= 5120).

    Before the criteria shared one input gradient only HybridMemoryLoss walked the memory in blocks: the other three failed
    here in their backward with "oim_grad: more than 5120 classes"."""
    out = []
    for name in ('hybrid', 'cluster-instance', 'proxy-instance', 'oim'):
        crit, mem, extra = _criterion(name, wide)
        loss, logits, x, fwd, bwd = _run(crit, extra, wide, trace)
        assert fwd == [('gemm', 9), LAUNCHES[name][0]] and bwd == BLOCKED, name
        assert logits.grl_top1[1] == 9
        out.append((name, loss.detach(), logits.detach(), x.grad, logits.grl_top1[0], mem.detach()))
    for other in out[1:]:
        for a, b in zip(out[0][1:], other[1:]):
            assert torch.equal(a, b), other[0]
    assert bool(out[0][3].abs().sum() > 0) and not torch.equal(out[0][5].cpu(), torch.from_numpy(wide['mem']))
