"""Camera-aware proxy memory loss with a mean teacher's soft pseudo-labels on MI355X (CAP, Wang et al. 2021
with the soft target of MMT, Ge et al. 2020): ``ProxyMemoryLoss`` whose two cross entropies -- over the proxies of the
sample's camera, and over its cluster's proxies plus the ``k_neg`` hardest proxies of other clusters -- are each taken
against (1 - w) the hard target + w the softmax of a TEACHER's similarities over the SAME set of proxies.  The sets, the own
proxy and the hard negatives are selected from the STUDENT's logits; the teacher is read at the student's selection, the
rule ``SoftTripletLoss`` uses.

The student's and the teacher's logits come out of ONE GEMM of the memory front end (``grl_amd.reid.loss.memory``), then ONE
`grl_soft_proxy_ce` call (``proxy_memory.proxy_ce``); the backward is ``ProxyMemory``'s, from the STUDENT's rows.  The teacher
carries no gradient.

Without a teacher, or with ``soft_weight == 0``, the call is ``ProxyMemoryLoss``'s: the same launches, the same bits."""
from torch import autograd

from grl_amd.reid.loss import memory
from grl_amd.reid.loss.proxy_memory import ProxyMemory, ProxyMemoryLoss, proxy_ce


class SoftProxyMemory(autograd.Function):
    """(loss, scaled student logits, correct) = grl_soft_proxy_ce(x . mem^T * scalar, teacher . mem^T * scalar, targets,
    cams, w); the backward is ``ProxyMemory.backward``."""

    @staticmethod
    def forward(ctx, inputs, targets, cams, teacher, mem, proxy_cluster, proxy_cam, momentum, scalar, mode, k_neg, w_intra,
                w_inter, w):
        return proxy_ce(ctx, inputs, targets, cams, mem, proxy_cluster, proxy_cam, momentum, scalar, mode, k_neg, w_intra,
                        w_inter, teacher, w)

    @staticmethod
    def backward(ctx, gloss, _glogits, _gcorrect):
        return ProxyMemory.backward(ctx, gloss, _glogits, _gcorrect) + (None, None)


class SoftProxyMemoryLoss(ProxyMemoryLoss):
    """``forward(inputs [n, D], targets [n], cams [n], teacher=None, soft_weight=0.0) -> (loss, logits)``:
    ``ProxyMemoryLoss`` with the teacher's rows ``teacher`` [n, D] (float32, on the device, no gradient) as a soft target of
    weight ``soft_weight`` in [0, 1] in both of its cross entropies.  ``logits`` are the student's and carry ``grl_top1``."""

    def forward(self, inputs, targets, cams, teacher=None, soft_weight=0.0):
        teacher, w = memory.soft_target('SoftProxyMemoryLoss', inputs, teacher, soft_weight)
        if teacher is None:
            return super(SoftProxyMemoryLoss, self).forward(inputs, targets, cams)
        return memory.top1(SoftProxyMemory.apply(inputs, targets, cams, teacher, self.centroids, self.proxy_cluster,
                                                 self.proxy_cam, self.momentum, 1.0 / self.temp, self.mode, self.k_neg,
                                                 self.w_intra, self.w_inter if self.inter_on else 0.0, w))
