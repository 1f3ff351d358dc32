"""Hybrid-memory loss with a mean teacher's soft pseudo-labels on MI355X (SpCL, Ge et al. 2020 with the soft
target of MMT, Ge et al. 2020): ``HybridMemoryLoss`` whose cross entropy over the classes -- the clusters, and every
unclustered instance as a class of its own -- is taken against the hard class blended with the softmax of a TEACHER's class
logits from the same instance memory,

    L_i = lse_C(z_i) - (1 - w) z_i[y] - w sum_c softmax_C(t_i)_c z_i[c],      z_c, t_c = the class means of x . mem^T / temp
                                                                               and of teacher . mem^T / temp.

forward : the student's and the teacher's rows are stacked into one [2n, D] operand, so that ONE K-blocked fp32 GEMM (scale
          in the epilogue, as OIMLoss) gives both logits; then ONE `grl_soft_hybrid_ce` call: loss, dlogits and the top-1
          count of the student's rows.
backward: ``HybridMemory``'s own, unchanged -- `grl_oim_grad` on the saved dlogits against the memory AS IT IS WHEN THE BACKWARD
          RUNS (in column blocks of 5120 where N > 5120), then the memory update from the STUDENT's rows.  The teacher carries
          no gradient.

Without a teacher, or with ``soft_weight == 0``, the call is ``HybridMemoryLoss``'s: the same launches, the same bits.
No torch op computes here (the stacking is a copy) and nothing syncs with the host; there is no CPU path."""
import ctypes as C

import torch
from torch import autograd

from grl_amd._lib import ptr, require_device, MATH_F32
from grl_amd.reid.loss.hybrid_memory import HybridMemory, HybridMemoryLoss
from grl_amd.reid.loss.oim import _call, _labels
from grl_amd.reid.loss.soft_memory import check_teacher


class SoftHybridMemory(autograd.Function):
    """(loss, scaled student logits, correct) = grl_soft_hybrid_ce(x . mem^T * scalar, teacher . mem^T * scalar, targets, the
    class tables, w); the backward is ``HybridMemory.backward``."""

    @staticmethod
    def forward(ctx, inputs, targets, index, teacher, mem, class_ptr, class_members, inst_class, momentum, scalar, w):
        from grl_amd import engine
        require_device(inputs, 'SoftHybridMemory inputs')
        require_device(mem, 'SoftHybridMemory memory')
        x = inputs.contiguous()
        y, idx = _labels(targets, x.device), _labels(index, x.device)
        n, D = x.shape
        if y.numel() != n or idx.numel() != n:
            raise ValueError('SoftHybridMemoryLoss: %d targets and %d indices for %d rows' % (y.numel(), idx.numel(), n))
        N, nc = mem.size(0), class_ptr.size(0) - 1
        both = torch.cat((x, teacher))                      # [2n, D]: one GEMM serves the student and the teacher
        scale = torch.full((N,), float(scalar), dtype=torch.float32, device=x.device)
        logits2 = torch.empty((2 * n, N), dtype=torch.float32, device=x.device)
        bk, mk = engine._pad_features(both), engine._pad_features(mem)
        engine.gemm(bk, mk, logits2, 2 * n, N, bk.size(1), scale=scale, math=MATH_F32, kblock=True)
        logits = logits2[:n]
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        correct = torch.empty((), dtype=torch.float32, device=x.device)
        dlogits = torch.empty((n, N), dtype=torch.float32, device=x.device)
        ws = torch.empty(3 * n + n * nc, dtype=torch.float32, device=x.device)     # rows [3][n], then the teacher's classes [n][C]
        _call('grl_soft_hybrid_ce', ptr(logits2), N, logits2.data_ptr() + 4 * n * N, N, ptr(y), ptr(class_ptr),
              ptr(class_members), ptr(inst_class), C.c_float(w), n, N, nc, ptr(loss), ptr(correct), ptr(dlogits), N, ptr(ws))
        ctx.save_for_backward(x, idx, dlogits)
        ctx.mem, ctx.momentum, ctx.scalar = mem, momentum, float(scalar)
        ctx.mark_non_differentiable(logits, correct)
        return loss, logits, correct

    @staticmethod
    def backward(ctx, gloss, _glogits, _gcorrect):
        return HybridMemory.backward(ctx, gloss, _glogits, _gcorrect) + (None, None)


class SoftHybridMemoryLoss(HybridMemoryLoss):
    """``forward(inputs [n, D], targets [n], index [n], teacher=None, soft_weight=0.0) -> (loss, logits)``:
    ``HybridMemoryLoss`` with the teacher's rows ``teacher`` [n, D] (float32, on the device, no gradient) as a soft target of
    weight ``soft_weight`` in [0, 1].  ``logits`` are the student's and carry ``grl_top1``."""

    def forward(self, inputs, targets, index, teacher=None, soft_weight=0.0):
        w = float(soft_weight)
        if not 0.0 <= w <= 1.0:
            raise ValueError('SoftHybridMemoryLoss: soft_weight must be in [0, 1] (got %r)' % (soft_weight,))
        if teacher is None or w == 0.0:
            return super(SoftHybridMemoryLoss, self).forward(inputs, targets, index)
        check_teacher(teacher, inputs, who='SoftHybridMemoryLoss')
        loss, logits, correct = SoftHybridMemory.apply(inputs, targets, index, teacher.contiguous(), self.memory,
                                                       self.class_ptr, self.class_members, self.inst_class, self.momentum,
                                                       1.0 / self.temp, w)
        logits.grl_top1 = (correct, logits.size(0))
        return loss, logits
