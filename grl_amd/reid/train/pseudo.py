"""Unsupervised training on pseudo-labels (cluster-contrast): the epoch flow that turns the evaluator's
clusterings into a relabelled training set and seeded cluster memories.

  pseudo_labels(xf, method, ..)   one of engine.cluster_jaccard / cluster / hdbscan / kmeans  ->  PseudoLabels
  PseudoLabels                    the labels on the device and on the host, the kept (non-noise) tracklets, unit centroids
  ProxyLabels                     ``PseudoLabels.proxies(cams)``: one proxy per (cluster, camera) pair
  train_unsupervised(..)          per epoch: extract, cluster, seed ``ClusterMemoryLoss.reset``, ``SEQTrainer.train``
                                  (``cameras=True``: ``ProxyMemoryLoss.reset`` from the proxies, ``CameraSEQTrainer``)

SEQTrainer itself is unchanged: it takes any criterion pair, and ``RandomPairSamplerForMars`` / ``RawVideoDataset`` take the
relabelled ``[(paths, label, cam)]`` list as they take a dataset's own."""
import numpy as np
import torch

METHODS = ('jaccard', 'cosine', 'hdbscan', 'kmeans')
UNCORR_COLS = (0, 2048)         # x_uncorr's slice of engine.extract_features' 6144-wide row: what criterion_uncorr sees
CORR_COLS = (2048, 4096)        # the attention-pooled x_corr slice: what criterion_corr sees


class PseudoLabels(object):
    """Cluster ids as training labels.

      labels       int64 [n] (on the device the clustering ran on; a host tensor when built from a host array): the
                   cluster of every sample, compact ids 0 .. n_clusters - 1 in ascending order of the ids given, -1 = noise
      host         the same as an int64 numpy array
      n_clusters, n_noise
      keep         int64 numpy: the indices with a label >= 0, ascending

    Any negative id given is noise.  Ids that are not compact already (an empty k-means cluster) are renumbered, so that a
    memory seeded from them has no empty row."""

    def __init__(self, labels, method=None):
        if torch.is_tensor(labels):
            host = labels.detach().cpu().numpy()            # the one read-back of the n labels
        else:
            host = np.asarray(labels)
        if host.ndim != 1 or host.dtype.kind not in 'iu':
            raise ValueError('PseudoLabels: labels must be n integers (got %s %s)' % (host.dtype, host.shape))
        host = host.astype(np.int64)
        ids = np.unique(host[host >= 0])
        compact = np.where(host >= 0, np.searchsorted(ids, host), -1).astype(np.int64)
        if torch.is_tensor(labels) and labels.dtype == torch.int64 and np.array_equal(compact, host):
            self.labels = labels
        else:
            self.labels = torch.from_numpy(compact)
            if torch.is_tensor(labels):
                self.labels = self.labels.to(labels.device)
        self.host = compact
        self.n_clusters = int(ids.size)
        self.keep = np.flatnonzero(compact >= 0).astype(np.int64)
        self.n_noise = int(compact.size - self.keep.size)
        self.method = method

    def __len__(self):
        return int(self.host.size)

    def relabel(self, tracklets):
        """``[(paths, label, cam)]`` of the kept tracklets, in their original order: the pid of every ``(paths, pid,
        cam)`` replaced by its cluster id, noise dropped."""
        if len(tracklets) != self.host.size:
            raise ValueError('PseudoLabels.relabel: %d tracklets for %d labels' % (len(tracklets), self.host.size))
        return [(tracklets[i][0], int(self.host[i]), tracklets[i][2]) for i in self.keep.tolist()]

    def centroids(self, xf, cols=None):
        """Unit centroids [n_clusters, d'] of the columns ``cols = (c0, c1)`` (default: all) of the rows the labels were
        computed from: ``engine.cluster_centroids(xf[:, c0:c1], labels, n_clusters, reduce='unit')``, noise ignored."""
        from grl_amd import engine
        if cols is not None:
            c0, c1 = cols
            if not 0 <= c0 < c1 <= xf.shape[1]:
                raise ValueError('PseudoLabels.centroids: cols = %r is no column range of %d columns' % (cols, xf.shape[1]))
            xf = xf[:, c0:c1]
        return engine.cluster_centroids(xf, self.labels.to(xf.device), self.n_clusters, reduce='unit')[0]

    def proxies(self, cams):
        """Camera-aware proxy labels: ``cams`` holds one non-negative integer per sample; the distinct
        (cluster, cam) pairs of the kept samples are numbered in ascending (cluster, cam) order -> ``ProxyLabels``.  Runs
        on the host copy of the labels: no further read-back."""
        return ProxyLabels(self, cams)

    def pair_scores(self, pids):
        """``Clustering.pair_scores`` of the labels against true identities (for data whose truth is known): pairwise
        precision / recall / F1 / ARI on the host, a noise sample being a cluster of its own."""
        from grl_amd import engine
        return engine._pair_scores(torch.from_numpy(self.host), self.n_clusters, pids)


class ProxyLabels(object):
    """One proxy per (cluster, camera) pair that occurs among the kept samples of ``labels`` (a PseudoLabels).

      proxy_cluster, proxy_cam   int32 numpy [n_proxies]: the pair of every proxy, ascending in (cluster, cam)
      proxy_cluster_dev, proxy_cam_dev   the same as int32 tensors on the labels' device (``ProxyMemoryLoss.reset`` takes them)
      sample_proxy               int64 numpy [n]: the proxy of every sample, -1 for noise
      sample_proxy_dev           the same on the labels' device
      n_proxies"""

    def __init__(self, labels, cams):
        if torch.is_tensor(cams):
            cams = cams.detach().cpu().numpy()
        cams = np.asarray(cams)
        if cams.ndim != 1 or cams.size != labels.host.size or cams.dtype.kind not in 'iu':
            raise ValueError('PseudoLabels.proxies: cams must be %d integers, one per sample (got %s %s)' % (
                labels.host.size, cams.dtype, cams.shape))
        cams = cams.astype(np.int64)
        if cams.size and cams.min() < 0:
            raise ValueError('PseudoLabels.proxies: a camera id is negative (%d)' % cams.min())
        if cams.size and cams.max() >= 2 ** 31:
            raise ValueError('PseudoLabels.proxies: a camera id does not fit int32 (%d)' % cams.max())
        keep = labels.keep
        span = int(cams.max()) + 1 if cams.size else 1
        pair = labels.host[keep] * span + cams[keep]        # ascending in (cluster, cam)
        ids = np.unique(pair)
        self.labels = labels
        self.n_proxies = int(ids.size)
        self.proxy_cluster = (ids // span).astype(np.int32)
        self.proxy_cam = (ids % span).astype(np.int32)
        self.sample_proxy = np.full(labels.host.size, -1, np.int64)
        self.sample_proxy[keep] = np.searchsorted(ids, pair)
        dev = labels.labels.device
        self.proxy_cluster_dev = torch.from_numpy(self.proxy_cluster).to(dev)
        self.proxy_cam_dev = torch.from_numpy(self.proxy_cam).to(dev)
        self.sample_proxy_dev = torch.from_numpy(self.sample_proxy).to(dev)

    def centroids(self, xf, cols=None):
        """Unit proxy centroids [n_proxies, d'] of the columns ``cols = (c0, c1)`` (default: all) of the rows the labels were
        computed from: ``engine.cluster_centroids(xf[:, c0:c1], sample_proxy, n_proxies, reduce='unit')``, noise ignored."""
        from grl_amd import engine
        if cols is not None:
            c0, c1 = cols
            if not 0 <= c0 < c1 <= xf.shape[1]:
                raise ValueError('ProxyLabels.centroids: cols = %r is no column range of %d columns' % (cols, xf.shape[1]))
            xf = xf[:, c0:c1]
        return engine.cluster_centroids(xf, self.sample_proxy_dev.to(xf.device), self.n_proxies, reduce='unit')[0]


def pseudo_labels(xf, method='jaccard', eps=0.5, min_samples=4, k1=20, k2=6, k=None, min_cluster_size=5, metric='cosine'):
    """Cluster the rows of ``xf`` [n, d] (device) into pseudo-identities:

      'jaccard'  engine.cluster_jaccard(xf, eps, min_samples, k1, k2)      eps: a k-reciprocal Jaccard distance in [0, 1]
      'cosine'   engine.cluster(xf, eps, min_samples, metric)              eps: that metric's distance (cosine: a negated dot)
      'hdbscan'  engine.hdbscan(xf, min_cluster_size, metric=metric)
      'kmeans'   engine.kmeans(xf, k, metric)                              no noise; ``k`` is required

    One read-back of the n labels.  ValueError: an unknown method, 'kmeans' without ``k`` (both before any device call), and
    fewer than 2 clusters -- a cross entropy over one class teaches nothing -- naming the method and its threshold."""
    if method not in METHODS:
        raise ValueError("pseudo_labels: method must be one of %s (got %r)" % (', '.join(repr(m) for m in METHODS), method))
    if method == 'kmeans' and k is None:
        raise ValueError("pseudo_labels: method 'kmeans' needs k, the number of clusters")
    from grl_amd import engine
    if method == 'jaccard':
        res, knob = engine.cluster_jaccard(xf, eps, min_samples, k1, k2), 'eps = %r, min_samples = %r' % (eps, min_samples)
    elif method == 'cosine':
        res, knob = engine.cluster(xf, eps, min_samples, metric), 'eps = %r, min_samples = %r' % (eps, min_samples)
    elif method == 'hdbscan':
        res, knob = engine.hdbscan(xf, min_cluster_size, metric=metric), 'min_cluster_size = %r' % (min_cluster_size,)
    else:
        res, knob = engine.kmeans(xf, k, metric), 'k = %r' % (k,)
    out = PseudoLabels(res.labels, method)
    if out.n_clusters < 2:
        raise ValueError("pseudo_labels: method %r with %s found %d cluster(s) among %d samples (%d noise); training needs "
                         'at least 2: change the threshold' % (method, knob, out.n_clusters, len(out), out.n_noise))
    return out


def train_unsupervised(trainer, evaluator, optimizer, tracklets, make_eval_loader, make_train_loader, epochs,
                       label_kwargs=None, on_epoch=None, cameras=False, inter_from_epoch=0):
    """Cluster-contrast training of ``trainer`` (a SEQTrainer whose ``criterion_corr`` / ``criterion_uncorr`` are
    ``ClusterMemoryLoss``) on ``tracklets`` = [(paths, pid, cam)] whose pids are never used.  Every epoch:

      xf = evaluator.extract_feature(make_eval_loader(tracklets))[0]     eval mode, no augmentation; one row per tracklet,
                                                                          in the list's order (the loader's pids are ignored)
      labels = pseudo_labels(xf, **label_kwargs)                          on the 6144-wide rows
      trainer.criterion_uncorr.reset(labels.centroids(xf, cols=(0, 2048)))
      trainer.criterion_corr.reset(labels.centroids(xf, cols=(2048, 4096)))
      trainer.train(epoch, make_train_loader(labels.relabel(tracklets)), optimizer)
      on_epoch(epoch, labels)                                             if given

    ``cameras=True`` (camera-aware proxies): ``trainer`` is a ``CameraSEQTrainer`` whose two criteria are
    ``ProxyMemoryLoss`` (checked before any device call); both memories are seeded from
    ``proxies = labels.proxies([t[2] for t in tracklets])`` -- ``reset(proxies.centroids(xf, cols), proxies.proxy_cluster_dev,
    proxies.proxy_cam_dev)`` over the same column ranges -- and their ``inter_on`` is ``epoch >= inter_from_epoch``.

    Returns the epochs' ``PseudoLabels``.  Under torch.distributed ``extract_feature`` gathers every row on every rank, so
    all ranks compute the same labels and seed the same memories."""
    tracklets = list(tracklets)
    if cameras:
        from grl_amd.reid.loss import ProxyMemoryLoss
        from grl_amd.reid.train.camera import CameraSEQTrainer
        if not isinstance(trainer, CameraSEQTrainer):
            raise ValueError('train_unsupervised: cameras=True needs a CameraSEQTrainer (got %s): SEQTrainer drops the '
                             "batch's camera ids" % type(trainer).__name__)
        for name in ('criterion_corr', 'criterion_uncorr'):
            if not isinstance(getattr(trainer, name), ProxyMemoryLoss):
                raise ValueError('train_unsupervised: cameras=True needs %s to be a ProxyMemoryLoss (got %s)' % (
                    name, type(getattr(trainer, name)).__name__))
    history = []
    for epoch in range(epochs):
        xf = evaluator.extract_feature(make_eval_loader(tracklets))[0]
        if xf.dim() != 2 or xf.shape[0] != len(tracklets) or xf.shape[1] < CORR_COLS[1]:
            raise ValueError('train_unsupervised: the eval loader gave features %s for %d tracklets (one row of at least '
                             '%d columns per tracklet is needed)' % (tuple(xf.shape), len(tracklets), CORR_COLS[1]))
        labels = pseudo_labels(xf, **(label_kwargs or {}))
        if cameras:
            proxies = labels.proxies([t[2] for t in tracklets])
            for crit, cols in ((trainer.criterion_uncorr, UNCORR_COLS), (trainer.criterion_corr, CORR_COLS)):
                crit.reset(proxies.centroids(xf, cols=cols), proxies.proxy_cluster_dev, proxies.proxy_cam_dev)
                crit.inter_on = epoch >= inter_from_epoch
        else:
            trainer.criterion_uncorr.reset(labels.centroids(xf, cols=UNCORR_COLS))
            trainer.criterion_corr.reset(labels.centroids(xf, cols=CORR_COLS))
        trainer.train(epoch, make_train_loader(labels.relabel(tracklets)), optimizer)
        history.append(labels)
        if on_epoch is not None:
            on_epoch(epoch, labels)
    return history
