"""Cluster-memory loss of unsupervised (cluster-contrast) training on MI355X: a temperature-scaled cross entropy against a
memory of unit cluster centroids that is updated inside the backward.

The memory is what ``grl_amd.reid.train.pseudo`` seeds each epoch from the pseudo-labels (``PseudoLabels.centroids``); the
targets are the cluster ids.  Forward and the gradient are OIMLoss's own, with scalar = 1 / temp: the K-blocked GEMM with the
scale in the epilogue and one `grl_softmax_ce` launch for loss, dlogits and the top-1 count (``OIM.forward``); `grl_oim_grad`
reads the memory AS IT IS WHEN THE BACKWARD RUNS.  The update that follows, over ``dist.gather_rank_order(x, y)`` so that
every rank applies the same global update, is one of three rules:

  'instance'  every sample, in batch order: c[y] = m c[y] + (1 - m) x, renormalised (`grl_oim_update` -- OIMLoss bit for bit)
  'hard'      per cluster present in the batch, one blend with its LEAST similar sample (`grl_cmem_update`, mode 0)
  'mean'      per cluster present in the batch, one blend with the mean of its samples (`grl_cmem_update`, mode 1)

A target outside [0, K) -- the noise label -1 -- carries weight 0 in the loss and updates nothing.
No torch op computes here and nothing syncs with the host; there is no CPU path."""
import ctypes as C

import torch
from torch import nn, autograd

from grl_amd._lib import ptr
from grl_amd.reid.loss.oim import OIM, _call

MODES = ('hard', 'mean', 'instance')


class ClusterMemory(autograd.Function):
    """(loss, scaled logits, correct) = CE(x . cent^T / temp, targets), as ``OIM``; ``mode`` picks the backward's update."""

    @staticmethod
    def forward(ctx, inputs, targets, cent, momentum, scalar, mode):
        ctx.mode = mode
        return OIM.forward(ctx, inputs, targets, cent, momentum, scalar, None)

    @staticmethod
    def backward(ctx, gloss, _glogits, _gcorrect):
        x, y, dlogits = ctx.saved_tensors
        cent, m = ctx.lut, ctx.momentum
        n, D = x.shape
        grad_inputs = None
        if ctx.needs_input_grad[0]:
            g = gloss.contiguous().float()
            grad_inputs = torch.empty_like(x)
            _call('grl_oim_grad', ptr(dlogits), cent.size(0), ptr(cent), ptr(g), C.c_float(ctx.scalar),
                  ptr(grad_inputs), n, cent.size(0), D)
        from grl_amd import dist as grl_dist
        xs, ys = grl_dist.gather_rank_order(x, y)
        if ctx.mode == 'instance':
            _call('grl_oim_update', ptr(cent), ptr(xs), ptr(ys), xs.size(0), D, cent.size(0), C.c_float(m))
        else:
            _call('grl_cmem_update', ptr(cent), ptr(xs), ptr(ys), xs.size(0), D, cent.size(0), C.c_float(m),
                  MODES.index(ctx.mode), None)
        return grad_inputs, None, None, None, None, None


class ClusterMemoryLoss(nn.Module):
    """``forward(inputs [n, D], targets [n]) -> (loss, logits)`` with OIMLoss's call surface; ``logits.grl_top1`` carries
    the top-1 count of the cross-entropy launch for ``SEQTrainer._top1``.  ``centroids`` [K, D] float32 is the memory
    (unit rows); ``reset(centroids)`` installs a new one -- K may change between epochs."""

    def __init__(self, num_features, num_clusters, temp=0.05, momentum=0.2, mode='hard'):
        super(ClusterMemoryLoss, self).__init__()
        if mode not in MODES:
            raise ValueError("ClusterMemoryLoss: mode must be 'hard', 'mean' or 'instance' (got %r)" % (mode,))
        if not temp > 0:
            raise ValueError('ClusterMemoryLoss: temp must be > 0 (got %r)' % (temp,))
        self.num_features = num_features
        self.num_clusters = num_clusters
        self.temp = temp
        self.momentum = momentum
        self.mode = mode
        self.register_buffer('centroids', torch.zeros(num_clusters, num_features))

    def reset(self, centroids):
        """Install ``centroids`` [K, num_features] (float32, on the device, unit rows -- ``PseudoLabels.centroids``) as the
        memory.  The tensor itself becomes the buffer: the backward updates it in place."""
        if not (torch.is_tensor(centroids) and centroids.dtype == torch.float32):
            raise ValueError('ClusterMemoryLoss.reset: centroids must be a float32 tensor (got %s)' % (
                centroids.dtype if torch.is_tensor(centroids) else type(centroids).__name__))
        if centroids.dim() != 2 or centroids.size(0) < 1 or centroids.size(1) != self.num_features:
            raise ValueError('ClusterMemoryLoss.reset: centroids must be [K >= 1, num_features = %d] (got %s)' % (
                self.num_features, tuple(centroids.shape)))
        if not centroids.is_cuda:
            raise ValueError('ClusterMemoryLoss.reset: centroids must be on a HIP device (got %s)' % centroids.device)
        self.centroids = centroids.detach().contiguous()
        self.num_clusters = self.centroids.size(0)
        return self

    def forward(self, inputs, targets):
        loss, logits, correct = ClusterMemory.apply(inputs, targets, self.centroids, self.momentum, 1.0 / self.temp,
                                                    self.mode)
        logits.grl_top1 = (correct, logits.size(0))
        return loss, logits
