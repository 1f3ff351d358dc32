"""Hybrid-memory loss with a mean teacher's soft pseudo-labels on MI355X (SpCL, Ge et al. 2020 with the soft
target of MMT, Ge et al. 2020): ``HybridMemoryLoss`` whose cross entropy over the classes -- the clusters, and every
unclustered instance as a class of its own -- is taken against the hard class blended with the softmax of a TEACHER's class
logits from the same instance memory,

    L_i = lse_C(z_i) - (1 - w) z_i[y] - w sum_c softmax_C(t_i)_c z_i[c],      z_c, t_c = the class means of x . mem^T / temp
                                                                               and of teacher . mem^T / temp.

The student's and the teacher's logits come out of ONE GEMM of the memory front end (``grl_amd.reid.loss.memory``), then ONE
`grl_soft_hybrid_ce` call (``hybrid_memory.hybrid_ce``); the backward is ``HybridMemory``'s, from the STUDENT's rows.  The
teacher carries no gradient.

Without a teacher, or with ``soft_weight == 0``, the call is ``HybridMemoryLoss``'s: the same launches, the same bits."""
from torch import autograd

from grl_amd.reid.loss import memory
from grl_amd.reid.loss.hybrid_memory import HybridMemory, HybridMemoryLoss, hybrid_ce


class SoftHybridMemory(autograd.Function):
    """(loss, scaled student logits, correct) = grl_soft_hybrid_ce(x . mem^T * scalar, teacher . mem^T * scalar, targets, the
    class tables, w); the backward is ``HybridMemory.backward``."""

    @staticmethod
    def forward(ctx, inputs, targets, index, teacher, mem, class_ptr, class_members, inst_class, momentum, scalar, w):
        return hybrid_ce(ctx, inputs, targets, index, mem, class_ptr, class_members, inst_class, momentum, scalar, teacher, w)

    @staticmethod
    def backward(ctx, gloss, _glogits, _gcorrect):
        return HybridMemory.backward(ctx, gloss, _glogits, _gcorrect) + (None, None)


class SoftHybridMemoryLoss(HybridMemoryLoss):
    """``forward(inputs [n, D], targets [n], index [n], teacher=None, soft_weight=0.0) -> (loss, logits)``:
    ``HybridMemoryLoss`` with the teacher's rows ``teacher`` [n, D] (float32, on the device, no gradient) as a soft target of
    weight ``soft_weight`` in [0, 1].  ``logits`` are the student's and carry ``grl_top1``."""

    def forward(self, inputs, targets, index, teacher=None, soft_weight=0.0):
        teacher, w = memory.soft_target('SoftHybridMemoryLoss', inputs, teacher, soft_weight)
        if teacher is None:
            return super(SoftHybridMemoryLoss, self).forward(inputs, targets, index)
        return memory.top1(SoftHybridMemory.apply(inputs, targets, index, teacher, self.memory, self.class_ptr,
                                                  self.class_members, self.inst_class, self.momentum, 1.0 / self.temp, w))
