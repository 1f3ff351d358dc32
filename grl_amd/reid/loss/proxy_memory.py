"""Camera-aware proxy memory loss of unsupervised training on MI355X (Wang et al., "Camera-aware Proxies for
Unsupervised Person Re-Identification", AAAI 2021): one memory row per (cluster, camera) pair that occurs, an intra-camera
cross entropy over the proxies of the sample's own camera and an inter-camera term that pulls the sample to all proxies of
its cluster and pushes it from the ``k_neg`` hardest proxies of other clusters.

The memory and its two tables are what ``PseudoLabels.proxies(cams)`` gives each epoch (``ProxyLabels.centroids``,
``proxy_cluster``, ``proxy_cam``); the targets are the cluster ids and ``cams`` the rows' camera ids.

forward : logits = x . memory^T / temp -- the K-blocked fp32 GEMM with the scale in its epilogue, as OIMLoss -- then ONE
          `grl_proxy_ce` call: loss, dlogits, the top-1 count and every row's own proxy (-1: the noise label, or a pair
          that has no proxy; such a row carries no loss, no gradient and updates nothing).
backward: `grl_oim_grad` on the saved dlogits against the memory AS IT IS WHEN THE BACKWARD RUNS, then the update over
          ``dist.gather_rank_order(x, own)`` with the PROXY id as the label:
  'instance'  every sample, in batch order: c[own] = m c[own] + (1 - m) x, renormalised (`grl_oim_update`; CAP's rule)
  'hard'      per proxy present in the batch, one blend with its least similar sample (`grl_cmem_update`, mode 0)
  'mean'      per proxy present in the batch, one blend with the mean of its samples (`grl_cmem_update`, mode 1)

The normaliser of the loss is the batch's valid rows; CAP sums per-camera means ("Not built").
No torch op computes here and nothing syncs with the host; there is no CPU path."""
import ctypes as C

import torch
from torch import nn, autograd

from grl_amd._lib import ptr, require_device, MATH_F32
from grl_amd.reid.loss.oim import _call, _labels
from grl_amd.reid.loss.cluster_memory import MODES


class ProxyMemory(autograd.Function):
    """(loss, scaled logits, correct) = grl_proxy_ce(x . mem^T * scalar, targets, cams); ``mode`` picks the backward's update."""

    @staticmethod
    def forward(ctx, inputs, targets, cams, mem, proxy_cluster, proxy_cam, momentum, scalar, mode, k_neg, w_intra, w_inter):
        from grl_amd import engine
        require_device(inputs, 'ProxyMemory inputs')
        require_device(mem, 'ProxyMemory memory')
        x = inputs.contiguous()
        y, cam = _labels(targets, x.device), _labels(cams, x.device)
        n, D = x.shape
        if y.numel() != n or cam.numel() != n:
            raise ValueError('ProxyMemoryLoss: %d targets and %d cams for %d rows' % (y.numel(), cam.numel(), n))
        P = mem.size(0)
        scale = torch.full((P,), float(scalar), dtype=torch.float32, device=x.device)
        logits = torch.empty((n, P), dtype=torch.float32, device=x.device)
        xk, mk = engine._pad_features(x), engine._pad_features(mem)        # (D % 32 != 0: zero columns for the GEMM, as OIM.forward)
        engine.gemm(xk, mk, logits, n, P, xk.size(1), scale=scale, math=MATH_F32, kblock=True)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        correct = torch.empty((), dtype=torch.float32, device=x.device)
        dlogits = torch.empty_like(logits)
        own = torch.empty(n, dtype=torch.int64, device=x.device)
        ws = torch.empty(3 * n, dtype=torch.float32, device=x.device)
        _call('grl_proxy_ce', ptr(logits), P, ptr(y), ptr(cam), ptr(proxy_cluster), ptr(proxy_cam), n, P, min(int(k_neg), P),
              C.c_float(w_intra), C.c_float(w_inter), ptr(loss), ptr(correct), ptr(dlogits), P, ptr(own), None, ptr(ws))
        ctx.save_for_backward(x, own, dlogits)
        ctx.mem, ctx.momentum, ctx.scalar, ctx.mode = mem, momentum, float(scalar), mode
        ctx.mark_non_differentiable(logits, correct)
        return loss, logits, correct

    @staticmethod
    def backward(ctx, gloss, _glogits, _gcorrect):
        x, own, dlogits = ctx.saved_tensors
        mem, m = ctx.mem, ctx.momentum
        n, D = x.shape
        P = mem.size(0)
        grad_inputs = None
        if ctx.needs_input_grad[0]:
            g = gloss.contiguous().float()
            grad_inputs = torch.empty_like(x)
            _call('grl_oim_grad', ptr(dlogits), P, ptr(mem), ptr(g), C.c_float(ctx.scalar), ptr(grad_inputs), n, P, D)
        from grl_amd import dist as grl_dist
        xs, ys = grl_dist.gather_rank_order(x, own)
        if ctx.mode == 'instance':
            _call('grl_oim_update', ptr(mem), ptr(xs), ptr(ys), xs.size(0), D, P, C.c_float(m))
        else:
            _call('grl_cmem_update', ptr(mem), ptr(xs), ptr(ys), xs.size(0), D, P, C.c_float(m), MODES.index(ctx.mode), None)
        return (grad_inputs,) + (None,) * 11


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
        if not (torch.is_tensor(centroids) and centroids.dtype == torch.float32):
            raise ValueError('ProxyMemoryLoss.reset: centroids must be a float32 tensor (got %s)' % (
                centroids.dtype if torch.is_tensor(centroids) else type(centroids).__name__))
        if centroids.dim() != 2 or centroids.size(0) < 1 or centroids.size(1) != self.num_features:
            raise ValueError('ProxyMemoryLoss.reset: centroids must be [P >= 1, num_features = %d] (got %s)' % (
                self.num_features, tuple(centroids.shape)))
        for name, t in (('proxy_cluster', proxy_cluster), ('proxy_cam', proxy_cam)):
            if not (torch.is_tensor(t) and t.dtype == torch.int32):
                raise ValueError('ProxyMemoryLoss.reset: %s must be an int32 tensor (got %s)' % (
                    name, t.dtype if torch.is_tensor(t) else type(t).__name__))
            if t.dim() != 1 or t.size(0) != centroids.size(0):
                raise ValueError('ProxyMemoryLoss.reset: %s must hold one entry per proxy, [%d] (got %s)' % (
                    name, centroids.size(0), tuple(t.shape)))
        if not centroids.is_cuda:
            raise ValueError('ProxyMemoryLoss.reset: centroids must be on a HIP device (got %s)' % centroids.device)
        for name, t in (('proxy_cluster', proxy_cluster), ('proxy_cam', proxy_cam)):
            if t.device != centroids.device:
                raise ValueError('ProxyMemoryLoss.reset: %s must be on the device of the centroids, %s (got %s)' % (
                    name, centroids.device, t.device))
        self.centroids = centroids.detach().contiguous()
        self.proxy_cluster = proxy_cluster.detach().contiguous()
        self.proxy_cam = proxy_cam.detach().contiguous()
        return self

    def forward(self, inputs, targets, cams):
        loss, logits, correct = ProxyMemory.apply(inputs, targets, cams, self.centroids, self.proxy_cluster, self.proxy_cam,
                                                  self.momentum, 1.0 / self.temp, self.mode, self.k_neg, self.w_intra,
                                                  self.w_inter if self.inter_on else 0.0)
        logits.grl_top1 = (correct, logits.size(0))
        return loss, logits
