"""Camera-aware proxy memory loss of unsupervised training on MI355X (Wang et al., "Camera-aware Proxies for
Unsupervised Person Re-Identification", AAAI 2021): one memory row per (cluster, camera) pair that occurs, an intra-camera
cross entropy over the proxies of the sample's own camera and an inter-camera term that pulls the sample to all proxies of
its cluster and pushes it from the ``k_neg`` hardest proxies of other clusters.

The memory and its two tables are what ``PseudoLabels.proxies(cams)`` gives each epoch (``ProxyLabels.centroids``,
``proxy_cluster``, ``proxy_cam``); the targets are the cluster ids and ``cams`` the rows' camera ids.

The logits GEMM, the input gradient and the update are the memory front end's (``grl_amd.reid.loss.memory``); between them
stands ONE `grl_proxy_ce` call: loss, dlogits, the top-1 count and every row's own proxy (-1: the noise label, or a pair that
has no proxy; such a row carries no loss, no gradient and updates nothing) -- or, against a mean teacher's rows,
`grl_soft_proxy_ce` (``SoftProxyMemoryLoss``).  The update (``mode``; 'instance' is CAP's rule) takes the PROXY id as the label.

The normaliser of the loss is the batch's valid rows; CAP sums per-camera means ("Not built").
No torch op computes here and nothing syncs with the host; there is no CPU path."""
import ctypes as C

import torch
from torch import nn, autograd

from grl_amd._lib import ptr, require_device
from grl_amd.reid.loss import memory
from grl_amd.reid.loss.memory import MODES, _labels


def proxy_ce(ctx, inputs, targets, cams, mem, proxy_cluster, proxy_cam, momentum, scalar, mode, k_neg, w_intra, w_inter,
             teacher=None, w=0.0):
    """A Function's forward: (loss, scaled logits, correct) = grl_proxy_ce(x . mem^T * scalar, targets, cams); with ``teacher``
    rows, grl_soft_proxy_ce against (1 - w) the hard targets + w the teacher's softmax over the same proxies."""
    require_device(inputs, 'ProxyMemory inputs')
    require_device(mem, 'ProxyMemory memory')
    x = inputs.contiguous()
    y, cam = _labels(targets, x.device), _labels(cams, x.device)
    n = x.size(0)
    if y.numel() != n or cam.numel() != n:
        raise ValueError('%sProxyMemoryLoss: %d targets and %d cams for %d rows' % (
            '' if teacher is None else 'Soft', y.numel(), cam.numel(), n))
    P = mem.size(0)
    both, logits = memory.scaled_logits(x, mem, scalar, teacher)
    loss, correct, dlogits, ws = memory.ce_outputs(logits, 3 * n)
    own = torch.empty(n, dtype=torch.int64, device=x.device)
    if teacher is None:
        memory._call('grl_proxy_ce', ptr(logits), P, ptr(y), ptr(cam), ptr(proxy_cluster), ptr(proxy_cam), n, P,
                     min(int(k_neg), P), C.c_float(w_intra), C.c_float(w_inter), ptr(loss), ptr(correct), ptr(dlogits), P,
                     ptr(own), None, ptr(ws))
    else:
        memory._call('grl_soft_proxy_ce', ptr(both), P, both.data_ptr() + 4 * n * P, P, ptr(y), ptr(cam), ptr(proxy_cluster),
                     ptr(proxy_cam), C.c_float(w), n, P, min(int(k_neg), P), C.c_float(w_intra), C.c_float(w_inter), ptr(loss),
                     ptr(correct), ptr(dlogits), P, ptr(own), None, ptr(ws))
    memory.save(ctx, x, own, dlogits, mem, momentum, scalar, mode)
    ctx.mark_non_differentiable(logits, correct)
    return loss, logits, correct


class ProxyMemory(autograd.Function):
    """(loss, scaled logits, correct) = ``proxy_ce``; ``mode`` picks the backward's update."""

    @staticmethod
    def forward(ctx, inputs, targets, cams, mem, proxy_cluster, proxy_cam, momentum, scalar, mode, k_neg, w_intra, w_inter):
        return proxy_ce(ctx, inputs, targets, cams, mem, proxy_cluster, proxy_cam, momentum, scalar, mode, k_neg, w_intra,
                        w_inter)

    @staticmethod
    def backward(ctx, gloss, _glogits, _gcorrect):
        return (memory.backward(ctx, gloss),) + (None,) * 11


class ProxyMemoryLoss(nn.Module):
    """``forward(inputs [n, D], targets [n], cams [n]) -> (loss, logits)``; ``logits.grl_top1`` carries the count of rows whose
    arg-max proxy belongs to the row's own cluster, for ``SEQTrainer._top1``.  ``reset(centroids, proxy_cluster, proxy_cam)``
    installs the memory [P, D] (float32, unit rows) and its tables (int32 [P]) -- P may change between epochs.  ``inter_on``:
    when false the kernel gets ``w_inter = 0`` (CAP turns the inter-camera term on after a few epochs)."""

    def __init__(self, num_features, temp=0.07, momentum=0.2, mode='instance', k_neg=50, w_intra=1.0, w_inter=0.5):
        super(ProxyMemoryLoss, self).__init__()
        if mode not in MODES:
            raise ValueError("ProxyMemoryLoss: mode must be 'hard', 'mean' or 'instance' (got %r)" % (mode,))
        if not temp > 0:
            raise ValueError('ProxyMemoryLoss: temp must be > 0 (got %r)' % (temp,))
        if int(k_neg) != k_neg or k_neg < 0:
            raise ValueError('ProxyMemoryLoss: k_neg must be an integer >= 0 (got %r)' % (k_neg,))
        self.num_features = num_features
        self.temp = temp
        self.momentum = momentum
        self.mode = mode
        self.k_neg = int(k_neg)
        self.w_intra = float(w_intra)
        self.w_inter = float(w_inter)
        self.inter_on = True
        self.register_buffer('centroids', torch.zeros(1, num_features))
        self.register_buffer('proxy_cluster', torch.zeros(1, dtype=torch.int32))
        self.register_buffer('proxy_cam', torch.zeros(1, dtype=torch.int32))

    @property
    def num_proxies(self):
        return self.centroids.size(0)

    def reset(self, centroids, proxy_cluster, proxy_cam):
        """Install ``centroids`` [P, num_features] (float32, on the device, unit rows -- ``ProxyLabels.centroids``) and the
        tables ``proxy_cluster`` / ``proxy_cam`` (int32 [P], on the same device).  The centroid tensor itself becomes the
        buffer: the backward updates it in place."""
        memory.check_memory('ProxyMemoryLoss.reset', 'centroids', 'P', centroids, self.num_features)
        tables = (('proxy_cluster', proxy_cluster), ('proxy_cam', proxy_cam))
        for name, t in tables:
            memory.check_table('ProxyMemoryLoss.reset', name, t)
            if t.dim() != 1 or t.size(0) != centroids.size(0):
                raise ValueError('ProxyMemoryLoss.reset: %s must hold one entry per proxy, [%d] (got %s)' % (
                    name, centroids.size(0), tuple(t.shape)))
        memory.check_devices('ProxyMemoryLoss.reset', 'centroids', centroids, tables)
        self.centroids = centroids.detach().contiguous()
        self.proxy_cluster = proxy_cluster.detach().contiguous()
        self.proxy_cam = proxy_cam.detach().contiguous()
        return self

    def forward(self, inputs, targets, cams):
        return memory.top1(ProxyMemory.apply(inputs, targets, cams, self.centroids, self.proxy_cluster, self.proxy_cam,
                                             self.momentum, 1.0 / self.temp, self.mode, self.k_neg, self.w_intra,
                                             self.w_inter if self.inter_on else 0.0))
