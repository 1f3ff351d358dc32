"""Hybrid-memory loss of self-paced unsupervised training on MI355X (Ge et al., "Self-paced Contrastive
Learning with Hybrid Memory", NeurIPS 2020): one memory row per training INSTANCE (tracklet), and a cross entropy whose
classes are the clusters plus every unclustered instance as a class of its own -- the samples DBSCAN calls noise stay in
the epoch.  A class's logit is the mean of its members' scaled similarities.

The memory and its three tables are what ``PseudoLabels.hybrid()`` gives each epoch (``HybridLabels.memory``,
``class_ptr_dev``, ``class_members_dev``, ``inst_class_dev``); the targets are the class ids, ``index`` the rows' memory rows.

The logits GEMM, the input gradient and the update are the memory front end's (``grl_amd.reid.loss.memory``); between them
stands ONE `grl_hybrid_ce` call -- loss, dlogits and the top-1 count over the classes -- or, against a mean teacher's rows,
`grl_soft_hybrid_ce` (``SoftHybridMemoryLoss``).  The update is the 'instance' rule with the INSTANCE index as the label.

No torch op computes here and nothing syncs with the host; there is no CPU path.  (A ``num_features`` that is no multiple
of 32, the K the logits GEMM takes, costs zero-padded copies of the inputs and the memory per forward: keep it a multiple.)"""
import ctypes as C

import numpy as np
import torch
from torch import nn, autograd

from grl_amd._lib import ptr, require_device
from grl_amd.reid.loss import memory
from grl_amd.reid.loss.memory import _labels, check_memory, check_table, check_devices

MAX_CLASSES = 15360             # GRL_HYBRID_MAX_CLASSES of include/grl_hip.h: the class logits of a row live in LDS


def check_partition(class_ptr, class_members, inst_class):
    """ValueError unless the three host arrays describe a partition of 0 .. N - 1 (N = len(inst_class)) into C =
    len(class_ptr) - 1 non-empty classes whose members ascend, ``inst_class`` being the inverse of the other two."""
    cp, cm, ic = (np.asarray(a).astype(np.int64) for a in (class_ptr, class_members, inst_class))
    N, nc = ic.size, cp.size - 1
    if nc < 1 or cm.size != N or N < 1:
        raise ValueError('hybrid class tables: class_ptr [C + 1 >= 2] and class_members / inst_class [N >= 1] are needed '
                         '(got %d, %d and %d entries)' % (cp.size, cm.size, N))
    if cp[0] != 0 or cp[-1] != N or np.any(np.diff(cp) < 1):
        raise ValueError('hybrid class tables: class_ptr must rise from 0 to N = %d in steps >= 1 (no empty class)' % N)
    if cm.min() < 0 or cm.max() >= N or np.unique(cm).size != N:
        raise ValueError('hybrid class tables: class_members must hold every index 0 .. %d exactly once' % (N - 1))
    inner = np.ones(N, bool)
    inner[cp[:-1]] = False                                 # positions that continue a class
    if np.any(np.diff(cm)[inner[1:]] <= 0):
        raise ValueError("hybrid class tables: a class's members must be listed in ascending index")
    owner = np.repeat(np.arange(nc, dtype=np.int64), np.diff(cp))
    if ic.min() < 0 or ic.max() >= nc or not np.array_equal(ic[cm], owner):
        raise ValueError('hybrid class tables: inst_class is not the inverse of class_ptr / class_members')


def hybrid_ce(ctx, inputs, targets, index, mem, class_ptr, class_members, inst_class, momentum, scalar, teacher=None, w=0.0):
    """A Function's forward: (loss, scaled logits, correct) = grl_hybrid_ce(x . mem^T * scalar, targets, the class tables); with
    ``teacher`` rows, grl_soft_hybrid_ce against (1 - w) the target + w the softmax of the teacher's class logits."""
    require_device(inputs, 'HybridMemory inputs')
    require_device(mem, 'HybridMemory memory')
    x = inputs.contiguous()
    y, idx = _labels(targets, x.device), _labels(index, x.device)
    n = x.size(0)
    if y.numel() != n or idx.numel() != n:
        raise ValueError('%sHybridMemoryLoss: %d targets and %d indices for %d rows' % (
            '' if teacher is None else 'Soft', y.numel(), idx.numel(), n))
    N, nc = mem.size(0), class_ptr.size(0) - 1
    both, logits = memory.scaled_logits(x, mem, scalar, teacher)
    # (ws: rows [3][n]; with a teacher, then its class logits [n][C])
    loss, correct, dlogits, ws = memory.ce_outputs(logits, 3 * n + (0 if teacher is None else n * nc))
    if teacher is None:
        memory._call('grl_hybrid_ce', ptr(logits), N, ptr(y), ptr(class_ptr), ptr(class_members), ptr(inst_class), n, N, nc,
                     ptr(loss), ptr(correct), ptr(dlogits), N, ptr(ws))
    else:
        memory._call('grl_soft_hybrid_ce', ptr(both), N, both.data_ptr() + 4 * n * N, N, ptr(y), ptr(class_ptr),
                     ptr(class_members), ptr(inst_class), C.c_float(w), n, N, nc, ptr(loss), ptr(correct), ptr(dlogits), N,
                     ptr(ws))
    memory.save(ctx, x, idx, dlogits, mem, momentum, scalar, 'instance')
    ctx.mark_non_differentiable(logits, correct)
    return loss, logits, correct


class HybridMemory(autograd.Function):
    """(loss, scaled logits, correct) = ``hybrid_ce``; the backward updates the memory rows ``index``."""

    @staticmethod
    def forward(ctx, inputs, targets, index, mem, class_ptr, class_members, inst_class, momentum, scalar):
        return hybrid_ce(ctx, inputs, targets, index, mem, class_ptr, class_members, inst_class, momentum, scalar)

    @staticmethod
    def backward(ctx, gloss, _glogits, _gcorrect):
        return (memory.backward(ctx, gloss),) + (None,) * 8


class HybridMemoryLoss(nn.Module):
    """``forward(inputs [n, D], targets [n], index [n]) -> (loss, logits)``; ``logits.grl_top1`` carries the count of rows
    whose arg-max class is the target, for ``SEQTrainer._top1``.  ``reset(memory, class_ptr, class_members, inst_class)``
    installs the instance memory [N, D] (float32, unit rows) and the class tables (int32) -- N and the classes may change
    between epochs."""

    def __init__(self, num_features, temp=0.05, momentum=0.2):
        super(HybridMemoryLoss, self).__init__()
        if not temp > 0:
            raise ValueError('HybridMemoryLoss: temp must be > 0 (got %r)' % (temp,))
        self.num_features = num_features
        self.temp = temp
        self.momentum = momentum
        self.register_buffer('memory', torch.zeros(1, num_features))
        self.register_buffer('class_ptr', torch.tensor([0, 1], dtype=torch.int32))
        self.register_buffer('class_members', torch.zeros(1, dtype=torch.int32))
        self.register_buffer('inst_class', torch.zeros(1, dtype=torch.int32))

    @property
    def num_instances(self):
        return self.memory.size(0)

    @property
    def num_classes(self):
        return self.class_ptr.size(0) - 1

    def reset(self, memory, class_ptr, class_members, inst_class):
        """Install ``memory`` [N, num_features] (float32, on the device, unit rows -- ``HybridLabels.memory``) and the
        tables ``class_ptr`` [C + 1], ``class_members`` [N], ``inst_class`` [N] (int32, on the same device).  The tables are
        checked once, on a host copy: a partition of 0 .. N - 1 into C <= GRL_HYBRID_MAX_CLASSES non-empty classes with
        ascending members.  The memory tensor itself becomes the buffer: the backward updates it in place."""
        check_memory('HybridMemoryLoss.reset', 'memory', 'N', memory, self.num_features)
        tables = (('class_ptr', class_ptr), ('class_members', class_members), ('inst_class', inst_class))
        for name, t in tables:
            check_table('HybridMemoryLoss.reset', name, t)
            if t.dim() != 1:
                raise ValueError('HybridMemoryLoss.reset: %s must be 1-d (got %s)' % (name, tuple(t.shape)))
        N = memory.size(0)
        if class_members.size(0) != N or inst_class.size(0) != N or not 2 <= class_ptr.size(0) <= N + 1:
            raise ValueError('HybridMemoryLoss.reset: for %d memory rows class_members and inst_class must be [%d] and '
                             'class_ptr [C + 1], 1 <= C <= %d (got %d, %d and %d entries)' % (
                                 N, N, N, class_members.size(0), inst_class.size(0), class_ptr.size(0)))
        if class_ptr.size(0) - 1 > MAX_CLASSES:
            raise ValueError('HybridMemoryLoss.reset: %d classes exceed GRL_HYBRID_MAX_CLASSES = %d' % (
                class_ptr.size(0) - 1, MAX_CLASSES))
        try:
            check_partition(class_ptr.cpu().numpy(), class_members.cpu().numpy(), inst_class.cpu().numpy())
        except ValueError as e:
            raise ValueError('HybridMemoryLoss.reset: %s' % e)
        check_devices('HybridMemoryLoss.reset', 'memory', memory, tables)
        self.memory = memory.detach().contiguous()
        self.class_ptr = class_ptr.detach().contiguous()
        self.class_members = class_members.detach().contiguous()
        self.inst_class = inst_class.detach().contiguous()
        return self

    def forward(self, inputs, targets, index):
        return memory.top1(HybridMemory.apply(inputs, targets, index, self.memory, self.class_ptr, self.class_members,
                                              self.inst_class, self.momentum, 1.0 / self.temp))
