"""Cluster-memory loss with a mean teacher's soft pseudo-labels on MI355X (Mean Teacher, Tarvainen & Valpola
2017; MMT, Ge et al. 2020): ``ClusterMemoryLoss`` whose cross entropy is taken against the hard cluster id blended with the
softmax of a TEACHER's similarities to the same memory,

    L_i = lse(z_i) - (1 - w) z_i[y] - w sum_j softmax(t_i)_j z_i[j],      z = x . cent^T / temp,  t = teacher . cent^T / temp.

The student's and the teacher's logits come out of ONE GEMM of the memory front end (``grl_amd.reid.loss.memory``), then ONE
`grl_soft_ce` call (``oim.softmax_ce``); the backward is ``ClusterMemory``'s, from the STUDENT's rows.  The teacher carries no
gradient.

Without a teacher, or with ``soft_weight == 0``, the call is ``ClusterMemoryLoss``'s: the same launches, the same bits."""
from torch import autograd

from grl_amd.reid.loss import memory
from grl_amd.reid.loss.cluster_memory import ClusterMemory, ClusterMemoryLoss
from grl_amd.reid.loss.memory import check_teacher        # noqa: F401  (its callers take it from here)
from grl_amd.reid.loss.oim import softmax_ce


class SoftClusterMemory(autograd.Function):
    """(loss, scaled student logits, correct) = grl_soft_ce(x . cent^T * scalar, teacher . cent^T * scalar, targets, w); the
    backward is ``ClusterMemory.backward``."""

    @staticmethod
    def forward(ctx, inputs, targets, teacher, cent, momentum, scalar, mode, w):
        return softmax_ce(ctx, inputs, targets, cent, momentum, scalar, mode, None, teacher, w)

    @staticmethod
    def backward(ctx, gloss, _glogits, _gcorrect):
        return ClusterMemory.backward(ctx, gloss, _glogits, _gcorrect) + (None, None)


class SoftClusterMemoryLoss(ClusterMemoryLoss):
    """``forward(inputs [n, D], targets [n], teacher=None, soft_weight=0.0) -> (loss, logits)``: ``ClusterMemoryLoss`` with
    the teacher's rows ``teacher`` [n, D] (float32, on the device, no gradient) as a soft target of weight ``soft_weight`` in
    [0, 1].  ``logits`` are the student's and carry ``grl_top1``."""

    def forward(self, inputs, targets, teacher=None, soft_weight=0.0):
        teacher, w = memory.soft_target('SoftClusterMemoryLoss', inputs, teacher, soft_weight)
        if teacher is None:
            return super(SoftClusterMemoryLoss, self).forward(inputs, targets)
        return memory.top1(SoftClusterMemory.apply(inputs, targets, teacher, self.centroids, self.momentum, 1.0 / self.temp,
                                                   self.mode, w))
