"""Unsupervised training on pseudo-labels (cluster-contrast): the epoch flow that turns the evaluator's
clusterings into a relabelled training set and seeded cluster memories.

  pseudo_labels(xf, method, ..)   one of engine.cluster_jaccard / cluster / hdbscan / kmeans  ->  PseudoLabels
  PseudoLabels                    the labels on the device and on the host, the kept (non-noise) tracklets, unit centroids
  train_unsupervised(..)          per epoch: extract, cluster, seed ``ClusterMemoryLoss.reset``, ``SEQTrainer.train``

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

    def pair_scores(self, pids):
        """``Clustering.pair_scores`` of the labels against true identities (for data whose truth is known): pairwise
        precision / recall / F1 / ARI on the host, a noise sample being a cluster of its own."""
        from grl_amd import engine
        return engine._pair_scores(torch.from_numpy(self.host), self.n_clusters, pids)


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
                       label_kwargs=None, on_epoch=None):
    """Cluster-contrast training of ``trainer`` (a SEQTrainer whose ``criterion_corr`` / ``criterion_uncorr`` are
    ``ClusterMemoryLoss``) on ``tracklets`` = [(paths, pid, cam)] whose pids are never used.  Every epoch:

      xf = evaluator.extract_feature(make_eval_loader(tracklets))[0]     eval mode, no augmentation; one row per tracklet,
                                                                          in the list's order (the loader's pids are ignored)
      labels = pseudo_labels(xf, **label_kwargs)                          on the 6144-wide rows
      trainer.criterion_uncorr.reset(labels.centroids(xf, cols=(0, 2048)))
      trainer.criterion_corr.reset(labels.centroids(xf, cols=(2048, 4096)))
      trainer.train(epoch, make_train_loader(labels.relabel(tracklets)), optimizer)
      on_epoch(epoch, labels)                                             if given

    Returns the epochs' ``PseudoLabels``.  Under torch.distributed ``extract_feature`` gathers every row on every rank, so
    all ranks compute the same labels and seed the same memories."""
    tracklets = list(tracklets)
    history = []
    for epoch in range(epochs):
        xf = evaluator.extract_feature(make_eval_loader(tracklets))[0]
        if xf.dim() != 2 or xf.shape[0] != len(tracklets) or xf.shape[1] < CORR_COLS[1]:
            raise ValueError('train_unsupervised: the eval loader gave features %s for %d tracklets (one row of at least '
                             '%d columns per tracklet is needed)' % (tuple(xf.shape), len(tracklets), CORR_COLS[1]))
        labels = pseudo_labels(xf, **(label_kwargs or {}))
        trainer.criterion_uncorr.reset(labels.centroids(xf, cols=UNCORR_COLS))
        trainer.criterion_corr.reset(labels.centroids(xf, cols=CORR_COLS))
        trainer.train(epoch, make_train_loader(labels.relabel(tracklets)), optimizer)
        history.append(labels)
        if on_epoch is not None:
            on_epoch(epoch, labels)
    return history
