"""Batch-hard soft-margin triplet loss with a mean teacher's soft target on MI355X (MMT's SoftTripletLoss,
Ge et al. 2020): ``TripletLoss('soft', True)`` whose two-way softmax over (d_ap, d_an) is taken against the hard order
blended with the softmax of the TEACHER's distances at the student's batch-hard indices,

    L_i = log(1 + exp(z_i)) - w sigmoid(t_i) z_i,      z_i = d(i, p_i) - d(i, n_i),  t_i = td(i, p_i) - td(i, n_i).

forward : ONE `grl_soft_triplet_fwd` launch -- the student's distance rows, the selection, the teacher's two distances per
          anchor and the per-anchor loss.
backward: ONE `grl_soft_triplet_bwd` launch (the gather form of `grl_triplet_bwd`).  The teacher carries no gradient.

Without a teacher, or with ``soft_weight == 0``, the call is ``TripletLoss('soft', True)``'s: the same launches, the same
bits.  No torch op computes here and nothing syncs with the host; there is no CPU path."""
import ctypes as C

import torch
import torch.nn as nn
from torch import autograd

from grl_amd._lib import ptr, require_device
from grl_amd.reid.loss.oim import _call, _labels
from grl_amd.reid.loss.memory import check_teacher
from grl_amd.reid.loss.triplet import _BatchHard


class _SoftBatchHard(autograd.Function):
    @staticmethod
    def forward(ctx, feat, ids, teacher, w):
        require_device(feat, 'SoftTripletLoss feat')
        f = feat.contiguous()
        y = _labels(ids, f.device)
        n, D = f.shape
        loss = torch.empty(n, dtype=torch.float32, device=f.device)
        dist = torch.empty((n, n), dtype=torch.float32, device=f.device)
        z = torch.empty(n, dtype=torch.float32, device=f.device)
        q = torch.empty(n, dtype=torch.float32, device=f.device)
        sel = torch.empty((n, 2), dtype=torch.int32, device=f.device)
        _call('grl_soft_triplet_fwd', ptr(f), ptr(teacher), ptr(y), n, D, C.c_float(w), ptr(loss), ptr(dist), ptr(sel), ptr(z),
              ptr(q))
        ctx.save_for_backward(f, dist, sel, z, q)
        ctx.w = w
        return loss

    @staticmethod
    def backward(ctx, dloss):
        f, dist, sel, z, q = ctx.saved_tensors
        n, D = f.shape
        df = torch.empty_like(f)
        _call('grl_soft_triplet_bwd', ptr(f), ptr(dist), ptr(sel), ptr(z), ptr(q), ptr(dloss.contiguous().float()),
              C.c_float(ctx.w), ptr(df), n, D)
        return df, None, None, None


class SoftTripletLoss(nn.Module):
    """``forward(feat [n, D], id [n], teacher=None, soft_weight=0.0) -> loss [n]``, per anchor as ``TripletLoss``: the
    batch-hard soft-margin triplet loss with the teacher's rows ``teacher`` [n, D] (float32, on the device, no gradient) as
    a soft target of weight ``soft_weight`` in [0, 1]."""

    def forward(self, feat, id, teacher=None, soft_weight=0.0):
        w = float(soft_weight)
        if not 0.0 <= w <= 1.0:
            raise ValueError('SoftTripletLoss: soft_weight must be in [0, 1] (got %r)' % (soft_weight,))
        if teacher is None or w == 0.0:
            return _BatchHard.apply(feat, id, 1, 0.0)
        check_teacher(teacher, feat, who='SoftTripletLoss')
        return _SoftBatchHard.apply(feat, id, teacher.contiguous(), w)
