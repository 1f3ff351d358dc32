"""Online Instance Matching loss (reference: reid/loss/oim.py:8-53) on MI355X.

The scaled-logits GEMM, the input gradient and the look-up table's update inside the backward are the memory front end's
(``grl_amd.reid.loss.memory``); this module's own is `grl_softmax_ce` = F.cross_entropy(mean) AND its
gradient in one launch -- or, against a mean teacher's rows, `grl_soft_ce` (``SoftClusterMemoryLoss``).  The update is the
'instance' rule: the LUT rows of the batch labels are momentum-updated one sample at a time and re-normalised.

SEQTrainer uses one criterion twice per step (trainer.py:126,138): autograd runs the later (clip-level) node first, so the
frame-level backward reads a LUT the clip-level update has already changed and stacks its own update on top.
tests/golden/oim.npz pins exactly that against the reference.

The reference's legacy non-static autograd Function cannot be applied on torch >= 1.5; this is
a static Function with the same maths, pinned to the reference's forward/backward bodies
(tests/golden/make_golden.py:oim_golden).
No torch op computes here and nothing syncs with the host; there is no CPU path."""
import ctypes as C

import torch
from torch import nn, autograd

from grl_amd._lib import ptr, require_device
from grl_amd.reid.loss import memory
from grl_amd.reid.loss.memory import _call, _labels        # noqa: F401  (pairloss, triplet and the teacher take them from here)


def softmax_ce(ctx, inputs, targets, mem, momentum, scalar, mode, weight=None, teacher=None, w=0.0):
    """A Function's forward: (loss, scaled logits, correct) = CE(scalar * x . mem^T, targets), the class ``weight`` in it; with
    ``teacher`` rows, against (1 - w) the target + w softmax(scalar * teacher . mem^T) and without a class weight.  ``mode`` is
    the backward's update."""
    require_device(inputs, 'OIM inputs')
    require_device(mem, 'OIM lut')
    x = inputs.contiguous()
    y = _labels(targets, x.device)
    n, c = x.size(0), mem.size(0)
    both, logits = memory.scaled_logits(x, mem, scalar, teacher)
    loss, correct, dlogits, ws = memory.ce_outputs(logits, (2 if teacher is None else 3) * n)
    if teacher is None:
        if weight is not None:
            require_device(weight, 'OIM class weight')
            weight = weight.contiguous()
        memory._call('grl_softmax_ce', ptr(logits), c, ptr(y), ptr(weight), n, c, ptr(loss), ptr(correct), ptr(dlogits), c,
                     ptr(ws))
    else:
        memory._call('grl_soft_ce', ptr(both), c, both.data_ptr() + 4 * n * c, c, ptr(y), C.c_float(w), n, c, ptr(loss),
                     ptr(correct), ptr(dlogits), c, ptr(ws))
    memory.save(ctx, x, y, dlogits, mem, momentum, scalar, mode)
    ctx.mark_non_differentiable(logits, correct)
    return loss, logits, correct


class OIM(autograd.Function):
    """(loss, scaled logits) = CE(scalar * x . LUT^T, targets); the logits are returned for
    the precision read-out only (trainer.py:127) and carry no gradient."""

    @staticmethod
    def forward(ctx, inputs, targets, lut, momentum, scalar, weight):
        return softmax_ce(ctx, inputs, targets, lut, momentum, scalar, 'instance', weight)

    @staticmethod
    def backward(ctx, gloss, _glogits, _gcorrect):
        return (memory.backward(ctx, gloss),) + (None,) * 5


def oim(inputs, targets, lut, momentum=0.5, scalar=1.0, weight=None):
    """(loss, scaled logits) as the reference's OIMLoss.forward; the logits carry ``grl_top1 = (correct rows, rows)``
    (device scalar) for the trainer's precision read-out."""
    return memory.top1(OIM.apply(inputs, targets, lut, momentum, scalar, weight))


class OIMLoss(nn.Module):
    def __init__(self, num_features, num_classes, scalar=1.0, momentum=0.5,
                 weight=None, size_average=True):
        super(OIMLoss, self).__init__()
        self.num_features = num_features
        self.num_classes = num_classes
        self.momentum = momentum
        self.scalar = scalar
        self.weight = weight
        self.register_buffer('lut', torch.zeros(num_classes, num_features))
        self.size_average = size_average

    def forward(self, inputs, targets):
        return oim(inputs, targets, self.lut, self.momentum, self.scalar, self.weight)
