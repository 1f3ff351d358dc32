"""Cluster-memory loss with a mean teacher's soft pseudo-labels on MI355X (Mean Teacher, Tarvainen & Valpola
2017; MMT, Ge et al. 2020): ``ClusterMemoryLoss`` whose cross entropy is taken against the hard cluster id blended with the
softmax of a TEACHER's similarities to the same memory,

    L_i = lse(z_i) - (1 - w) z_i[y] - w sum_j softmax(t_i)_j z_i[j],      z = x . cent^T / temp,  t = teacher . cent^T / temp.

forward : the student's and the teacher's rows are stacked into one [2n, D] operand, so that ONE K-blocked fp32 GEMM (scale
          in the epilogue, as OIMLoss) gives both logits; then ONE `grl_soft_ce` call: loss, dlogits and the top-1 count of the
          student's rows.
backward: ``ClusterMemory``'s own -- `grl_oim_grad` on the saved dlogits against the memory AS IT IS WHEN THE BACKWARD RUNS, then
          the memory update from the STUDENT's rows (``mode``, over ``dist.gather_rank_order``).  The teacher carries no gradient.

Without a teacher, or with ``soft_weight == 0``, the call is ``ClusterMemoryLoss``'s: the same launches, the same bits.
No torch op computes here (the stacking is a copy) and nothing syncs with the host; there is no CPU path."""
import ctypes as C

import torch
from torch import autograd

from grl_amd._lib import ptr, require_device, MATH_F32
from grl_amd.reid.loss.cluster_memory import ClusterMemory, ClusterMemoryLoss
from grl_amd.reid.loss.oim import _call, _labels


class SoftClusterMemory(autograd.Function):
    """(loss, scaled student logits, correct) = grl_soft_ce(x . cent^T * scalar, teacher . cent^T * scalar, targets, w); the
    backward is ``ClusterMemory.backward``."""

    @staticmethod
    def forward(ctx, inputs, targets, teacher, cent, momentum, scalar, mode, w):
        from grl_amd import engine
        require_device(inputs, 'SoftClusterMemory inputs')
        require_device(cent, 'SoftClusterMemory centroids')
        ctx.mode = mode
        x = inputs.contiguous()
        y = _labels(targets, x.device)
        n, D = x.shape
        c = cent.size(0)
        both = torch.cat((x, teacher))                      # [2n, D]: one GEMM serves the student and the teacher
        scale = torch.full((c,), float(scalar), dtype=torch.float32, device=x.device)
        logits2 = torch.empty((2 * n, c), dtype=torch.float32, device=x.device)
        bk, ck = engine._pad_features(both), engine._pad_features(cent)
        engine.gemm(bk, ck, logits2, 2 * n, c, bk.size(1), scale=scale, math=MATH_F32, kblock=True)
        logits = logits2[:n]
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        correct = torch.empty((), dtype=torch.float32, device=x.device)
        dlogits = torch.empty((n, c), dtype=torch.float32, device=x.device)
        ws = torch.empty(3 * n, dtype=torch.float32, device=x.device)
        _call('grl_soft_ce', ptr(logits2), c, logits2.data_ptr() + 4 * n * c, c, ptr(y), C.c_float(w), n, c, ptr(loss),
              ptr(correct), ptr(dlogits), c, ptr(ws))
        ctx.save_for_backward(x, y, dlogits)
        ctx.lut, ctx.momentum, ctx.scalar = cent, momentum, float(scalar)
        ctx.mark_non_differentiable(logits, correct)
        return loss, logits, correct

    @staticmethod
    def backward(ctx, gloss, _glogits, _gcorrect):
        return ClusterMemory.backward(ctx, gloss, _glogits, _gcorrect) + (None, None)


def check_teacher(teacher, inputs, who='SoftClusterMemoryLoss'):
    """ValueError unless ``teacher`` is a float32 tensor of ``inputs``' shape on ``inputs``' device that carries no gradient."""
    if not torch.is_tensor(teacher):
        raise ValueError('%s: teacher must be a tensor (got %s)' % (who, type(teacher).__name__))
    if tuple(teacher.shape) != tuple(inputs.shape) or teacher.dim() != 2:
        raise ValueError('%s: teacher must be [n, D] = %s, the shape of the inputs (got %s)' % (
            who, tuple(inputs.shape), tuple(teacher.shape)))
    if teacher.dtype != torch.float32:
        raise ValueError('%s: teacher must be float32 (got %s)' % (who, teacher.dtype))
    if teacher.device != inputs.device:
        raise ValueError('%s: teacher must be on the device of the inputs, %s (got %s)' % (who, inputs.device, teacher.device))
    if teacher.requires_grad:
        raise ValueError('%s: teacher must carry no gradient (compute it under torch.no_grad() or detach it)' % who)


class SoftClusterMemoryLoss(ClusterMemoryLoss):
    """``forward(inputs [n, D], targets [n], teacher=None, soft_weight=0.0) -> (loss, logits)``: ``ClusterMemoryLoss`` with
    the teacher's rows ``teacher`` [n, D] (float32, on the device, no gradient) as a soft target of weight ``soft_weight`` in
    [0, 1].  ``logits`` are the student's and carry ``grl_top1``."""

    def forward(self, inputs, targets, teacher=None, soft_weight=0.0):
        w = float(soft_weight)
        if not 0.0 <= w <= 1.0:
            raise ValueError('SoftClusterMemoryLoss: soft_weight must be in [0, 1] (got %r)' % (soft_weight,))
        if teacher is None or w == 0.0:
            return super(SoftClusterMemoryLoss, self).forward(inputs, targets)
        check_teacher(teacher, inputs)
        loss, logits, correct = SoftClusterMemory.apply(inputs, targets, teacher.contiguous(), self.centroids, self.momentum,
                                                        1.0 / self.temp, self.mode, w)
        logits.grl_top1 = (correct, logits.size(0))
        return loss, logits
