"""Cluster-memory loss of unsupervised (cluster-contrast) training on MI355X: a temperature-scaled cross entropy against a
memory of unit cluster centroids that is updated inside the backward.

The memory is what ``grl_amd.reid.train.pseudo`` seeds each epoch from the pseudo-labels (``PseudoLabels.centroids``); the
targets are the cluster ids.  Forward and the gradient are OIMLoss's own, with scalar = 1 / temp (``oim.softmax_ce`` on the
memory front end, ``grl_amd.reid.loss.memory``); the update that follows is one of the front end's three rules, ``mode``:
'instance' is OIMLoss bit for bit.

A target outside [0, K) -- the noise label -1 -- carries weight 0 in the loss and updates nothing.
No torch op computes here and nothing syncs with the host; there is no CPU path."""
import torch
from torch import nn, autograd

from grl_amd.reid.loss import memory
from grl_amd.reid.loss.memory import MODES
from grl_amd.reid.loss.oim import softmax_ce


class ClusterMemory(autograd.Function):
    """(loss, scaled logits, correct) = CE(x . cent^T / temp, targets), as ``OIM``; ``mode`` picks the backward's update."""

    @staticmethod
    def forward(ctx, inputs, targets, cent, momentum, scalar, mode):
        return softmax_ce(ctx, inputs, targets, cent, momentum, scalar, mode)

    @staticmethod
    def backward(ctx, gloss, _glogits, _gcorrect):
        return (memory.backward(ctx, gloss),) + (None,) * 5


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
        memory.check_memory('ClusterMemoryLoss.reset', 'centroids', 'K', centroids, self.num_features)
        memory.check_devices('ClusterMemoryLoss.reset', 'centroids', centroids)
        self.centroids = centroids.detach().contiguous()
        self.num_clusters = self.centroids.size(0)
        return self

    def forward(self, inputs, targets):
        return memory.top1(ClusterMemory.apply(inputs, targets, self.centroids, self.momentum, 1.0 / self.temp, self.mode))
