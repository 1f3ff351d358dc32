"""Hard instance contrast and soft instance consistency against a mean teacher on MI355X (the two instance
terms of ICE, Chen, Lagadec and Bremond 2021).  With u the L2-normalised student rows, v the L2-normalised teacher rows,
c_ij = <u_i, v_j> and t_ij = <v_i, v_j>, every anchor selects one column per id of the batch -- of its own id the member with
the smallest c_ij (the hard positive p_i, the anchor itself counts), of every other id the member with the largest, the lowest
index among equals -- and over that set K_i

    P = softmax(c_ik / tau),  Q = softmax(t_ik / teacher_tau),  L_i = - hard_weight log P_p - soft_weight sum_k Q_k log P_k.

forward : ONE `grl_ins_contrast_fwd` launch -- the similarity row, the selection, both softmaxes, the per-anchor loss and the
          coefficients g_ik = dL_i / d(c_ik / tau) of the backward.
backward: ONE `grl_ins_contrast_bwd` launch through the normalisation.  The teacher carries no gradient.

The default temperature 0.1 is this project's, not the paper's.  No torch op computes here and nothing syncs with the host;
there is no CPU path."""
import ctypes as C
import math

import torch
import torch.nn as nn
from torch import autograd

from grl_amd._lib import ptr, require_device
from grl_amd.reid.loss.oim import _call, _labels
from grl_amd.reid.loss.memory import check_teacher


class _InsContrast(autograd.Function):
    @staticmethod
    def forward(ctx, feat, ids, teacher, tau, tau_t, wh, ws):
        require_device(feat, 'InstanceContrastLoss feat')
        f = feat.contiguous()
        y = _labels(ids, f.device)
        n, D = f.shape
        loss = torch.empty(n, dtype=torch.float32, device=f.device)
        cos = torch.empty((n, n), dtype=torch.float32, device=f.device)
        coef = torch.empty((n, n), dtype=torch.float32, device=f.device)
        sel = torch.empty((n, n), dtype=torch.int32, device=f.device)
        _call('grl_ins_contrast_fwd', ptr(f), ptr(teacher), ptr(y), n, D, C.c_float(tau), C.c_float(tau_t), C.c_float(wh),
              C.c_float(ws), ptr(loss), ptr(cos), ptr(sel), ptr(coef))
        ctx.save_for_backward(f, teacher, coef)
        ctx.tau = tau
        return loss

    @staticmethod
    def backward(ctx, dloss):
        f, teacher, coef = ctx.saved_tensors
        n, D = f.shape
        df = torch.empty_like(f)
        _call('grl_ins_contrast_bwd', ptr(f), ptr(teacher), ptr(coef), ptr(dloss.contiguous().float()), C.c_float(ctx.tau),
              ptr(df), n, D)
        return df, None, None, None, None, None, None


def check_temperature(name, v, who='InstanceContrastLoss'):
    t = float(v)
    if not (t > 0.0 and math.isfinite(t)):
        raise ValueError('%s: %s must be a finite number > 0 (got %r)' % (who, name, v))
    return t


def check_ins_weights(hard_weight, soft_weight, who='InstanceContrastLoss', names=('hard_weight', 'soft_weight'),
                      allow_both_zero=False):
    """(hard, soft) as floats; ValueError naming the argument for a negative or non-finite weight, and for both 0."""
    out = []
    for name, w in zip(names, (hard_weight, soft_weight)):
        v = float(w)
        if not (v >= 0.0 and math.isfinite(v)):
            raise ValueError('%s: %s must be a finite number >= 0 (got %r)' % (who, name, w))
        out.append(v)
    if not allow_both_zero and out[0] == 0.0 and out[1] == 0.0:
        raise ValueError('%s: %s and %s must not both be 0' % (who, names[0], names[1]))
    return tuple(out)


class InstanceContrastLoss(nn.Module):
    """``InstanceContrastLoss(tau=0.1, teacher_tau=None)``; ``forward(feat [n, D], id [n], teacher [n, D], hard_weight=1.0,
    soft_weight=0.0) -> loss [n]``, per anchor: ``teacher`` holds the teacher's rows of the same samples (float32, on the
    device, no gradient).  ``teacher_tau=None`` means ``tau``."""

    def __init__(self, tau=0.1, teacher_tau=None):
        super(InstanceContrastLoss, self).__init__()
        self.tau = check_temperature('tau', tau)
        self.teacher_tau = self.tau if teacher_tau is None else check_temperature('teacher_tau', teacher_tau)

    def forward(self, feat, id, teacher=None, hard_weight=1.0, soft_weight=0.0):
        wh, ws = check_ins_weights(hard_weight, soft_weight)
        if teacher is None:
            raise ValueError('InstanceContrastLoss: teacher is missing (both terms are taken against the teacher\'s rows)')
        check_teacher(teacher, feat, who='InstanceContrastLoss')
        return _InsContrast.apply(feat, id, teacher.contiguous(), self.tau, self.teacher_tau, wh, ws)
