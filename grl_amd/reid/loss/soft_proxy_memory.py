"""Camera-aware proxy memory loss with a mean teacher's soft pseudo-labels on MI355X (CAP, Wang et al. 2021
with the soft target of MMT, Ge et al. 2020): ``ProxyMemoryLoss`` whose two cross entropies -- over the proxies of the
sample's camera, and over its cluster's proxies plus the ``k_neg`` hardest proxies of other clusters -- are each taken
against (1 - w) the hard target + w the softmax of a TEACHER's similarities over the SAME set of proxies.  The sets, the own
proxy and the hard negatives are selected from the STUDENT's logits; the teacher is read at the student's selection, the
rule ``SoftTripletLoss`` uses.

forward : the student's and the teacher's rows are stacked into one [2n, D] operand, so that ONE K-blocked fp32 GEMM (scale
          in the epilogue, as OIMLoss) gives both logits; then ONE `grl_soft_proxy_ce` call: loss, dlogits, the top-1 count
          and every row's own proxy.
backward: ``ProxyMemory``'s own, unchanged -- `grl_oim_grad` on the saved dlogits against the memory AS IT IS WHEN THE BACKWARD
          RUNS, then the update (``mode``) from the STUDENT's rows.  The teacher carries no gradient.

Without a teacher, or with ``soft_weight == 0``, the call is ``ProxyMemoryLoss``'s: the same launches, the same bits.
No torch op computes here (the stacking is a copy) and nothing syncs with the host; there is no CPU path."""
import ctypes as C

import torch
from torch import autograd

from grl_amd._lib import ptr, require_device, MATH_F32
from grl_amd.reid.loss.oim import _call, _labels
from grl_amd.reid.loss.proxy_memory import ProxyMemory, ProxyMemoryLoss
from grl_amd.reid.loss.soft_memory import check_teacher


class SoftProxyMemory(autograd.Function):
    """(loss, scaled student logits, correct) = grl_soft_proxy_ce(x . mem^T * scalar, teacher . mem^T * scalar, targets,
    cams, w); the backward is ``ProxyMemory.backward``."""

    @staticmethod
    def forward(ctx, inputs, targets, cams, teacher, mem, proxy_cluster, proxy_cam, momentum, scalar, mode, k_neg, w_intra,
                w_inter, w):
        from grl_amd import engine
        require_device(inputs, 'SoftProxyMemory inputs')
        require_device(mem, 'SoftProxyMemory memory')
        x = inputs.contiguous()
        y, cam = _labels(targets, x.device), _labels(cams, x.device)
        n, D = x.shape
        if y.numel() != n or cam.numel() != n:
            raise ValueError('SoftProxyMemoryLoss: %d targets and %d cams for %d rows' % (y.numel(), cam.numel(), n))
        P = mem.size(0)
        both = torch.cat((x, teacher))                      # [2n, D]: one GEMM serves the student and the teacher
        scale = torch.full((P,), float(scalar), dtype=torch.float32, device=x.device)
        logits2 = torch.empty((2 * n, P), dtype=torch.float32, device=x.device)
        bk, mk = engine._pad_features(both), engine._pad_features(mem)
        engine.gemm(bk, mk, logits2, 2 * n, P, bk.size(1), scale=scale, math=MATH_F32, kblock=True)
        logits = logits2[:n]
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        correct = torch.empty((), dtype=torch.float32, device=x.device)
        dlogits = torch.empty((n, P), dtype=torch.float32, device=x.device)
        own = torch.empty(n, dtype=torch.int64, device=x.device)
        ws = torch.empty(3 * n, dtype=torch.float32, device=x.device)
        _call('grl_soft_proxy_ce', ptr(logits2), P, logits2.data_ptr() + 4 * n * P, P, ptr(y), ptr(cam), ptr(proxy_cluster),
              ptr(proxy_cam), C.c_float(w), n, P, min(int(k_neg), P), C.c_float(w_intra), C.c_float(w_inter), ptr(loss),
              ptr(correct), ptr(dlogits), P, ptr(own), None, ptr(ws))
        ctx.save_for_backward(x, own, dlogits)
        ctx.mem, ctx.momentum, ctx.scalar, ctx.mode = mem, momentum, float(scalar), mode
        ctx.mark_non_differentiable(logits, correct)
        return loss, logits, correct

    @staticmethod
    def backward(ctx, gloss, _glogits, _gcorrect):
        return ProxyMemory.backward(ctx, gloss, _glogits, _gcorrect) + (None, None)


class SoftProxyMemoryLoss(ProxyMemoryLoss):
    """``forward(inputs [n, D], targets [n], cams [n], teacher=None, soft_weight=0.0) -> (loss, logits)``:
    ``ProxyMemoryLoss`` with the teacher's rows ``teacher`` [n, D] (float32, on the device, no gradient) as a soft target of
    weight ``soft_weight`` in [0, 1] in both of its cross entropies.  ``logits`` are the student's and carry ``grl_top1``."""

    def forward(self, inputs, targets, cams, teacher=None, soft_weight=0.0):
        w = float(soft_weight)
        if not 0.0 <= w <= 1.0:
            raise ValueError('SoftProxyMemoryLoss: soft_weight must be in [0, 1] (got %r)' % (soft_weight,))
        if teacher is None or w == 0.0:
            return super(SoftProxyMemoryLoss, self).forward(inputs, targets, cams)
        check_teacher(teacher, inputs, who='SoftProxyMemoryLoss')
        loss, logits, correct = SoftProxyMemory.apply(inputs, targets, cams, teacher.contiguous(), self.centroids,
                                                      self.proxy_cluster, self.proxy_cam, self.momentum, 1.0 / self.temp,
                                                      self.mode, self.k_neg, self.w_intra,
                                                      self.w_inter if self.inter_on else 0.0, w)
        logits.grl_top1 = (correct, logits.size(0))
        return loss, logits
