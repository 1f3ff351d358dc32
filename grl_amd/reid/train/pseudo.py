"""Unsupervised training on pseudo-labels (cluster-contrast): the epoch flow that turns the evaluator's
clusterings into a relabelled training set and seeded cluster memories.

  pseudo_labels(xf, method, ..)   one of engine.cluster_jaccard / cluster / hdbscan / kmeans  ->  PseudoLabels
  PseudoLabels                    the labels on the device and on the host, the kept (non-noise) tracklets, unit centroids
  ProxyLabels                     ``PseudoLabels.proxies(cams)``: one proxy per (cluster, camera) pair
  HybridLabels                    ``PseudoLabels.hybrid()``: the clusters plus every noise sample as a class of its own, the
                                  class tables and the instance memory of ``HybridMemoryLoss``
  self_paced_labels(xf, state, ..)  DBSCAN at eps - delta, eps, eps + delta; only the clusters that are stable keep their samples
  train_unsupervised(..)          per epoch: extract, cluster, seed ``ClusterMemoryLoss.reset``, ``SEQTrainer.train``
                                  (``cameras=True``: ``ProxyMemoryLoss.reset`` from the proxies, ``CameraSEQTrainer``;
                                  ``hybrid=True``: ``HybridMemoryLoss.reset`` from the instances, ``HybridSEQTrainer``)

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

    def hybrid(self):
        """Hybrid-memory labels: the clusters keep their ids, every noise sample becomes a class of its own
        -> ``HybridLabels``.  Runs on the host copy of the labels: no further read-back."""
        return HybridLabels(self)

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


class HybridLabels(object):
    """Every sample of ``labels`` (a PseudoLabels) in a class: the clusters keep their ids 0 .. K - 1, the noise samples
    become the classes K, K + 1, .. in ascending sample index.

      sample_class               int64 numpy [n]: the class of every sample (``sample_class_dev``: on the labels' device)
      n_classes                  K + n_noise
      class_ptr, class_members   int32 numpy [n_classes + 1] / [n]: the members of class c, in ascending sample index, are
                                 class_members[class_ptr[c] : class_ptr[c + 1]]
      inst_class                 int32 numpy [n]: ``sample_class`` as the kernel's table
      class_ptr_dev, class_members_dev, inst_class_dev   the same on the labels' device (``HybridMemoryLoss.reset`` takes them)"""

    def __init__(self, labels):
        host = labels.host
        noise = np.flatnonzero(host < 0)
        self.labels = labels
        self.sample_class = host.copy()
        self.sample_class[noise] = labels.n_clusters + np.arange(noise.size, dtype=np.int64)
        self.n_classes = labels.n_clusters + int(noise.size)
        self.class_members = np.argsort(self.sample_class, kind='stable').astype(np.int32)
        self.class_ptr = np.concatenate(([0], np.cumsum(np.bincount(self.sample_class, minlength=self.n_classes)))).astype(np.int32)
        self.inst_class = self.sample_class.astype(np.int32)
        dev = labels.labels.device
        self.sample_class_dev = torch.from_numpy(self.sample_class).to(dev)
        self.class_ptr_dev = torch.from_numpy(self.class_ptr).to(dev)
        self.class_members_dev = torch.from_numpy(self.class_members).to(dev)
        self.inst_class_dev = torch.from_numpy(self.inst_class).to(dev)

    def __len__(self):
        return int(self.sample_class.size)

    def relabel(self, tracklets):
        """``[(paths, class, cam)]`` of ALL tracklets, in their order: the pid of every ``(paths, pid, cam)`` replaced by its
        class id.  Tracklet i is row i of the memory: the loader's dataset index is the instance index."""
        if len(tracklets) != self.sample_class.size:
            raise ValueError('HybridLabels.relabel: %d tracklets for %d labels' % (len(tracklets), self.sample_class.size))
        return [(t[0], int(c), t[2]) for t, c in zip(tracklets, self.sample_class.tolist())]

    def memory(self, xf, cols=None):
        """Unit instance rows [n, d'] of the columns ``cols = (c0, c1)`` (default: all) of the rows the labels were computed
        from: ``engine.cluster_centroids(xf[:, c0:c1], arange(n), n, reduce='unit')``."""
        from grl_amd import engine
        if cols is not None:
            c0, c1 = cols
            if not 0 <= c0 < c1 <= xf.shape[1]:
                raise ValueError('HybridLabels.memory: cols = %r is no column range of %d columns' % (cols, xf.shape[1]))
            xf = xf[:, c0:c1]
        n = self.sample_class.size
        return engine.cluster_centroids(xf, torch.arange(n, dtype=torch.int64, device=xf.device), n, reduce='unit')[0]


def _own_sets(labels):
    """int64 [n]: the labels with every noise sample (< 0) in a set of its own, numbered after the clusters."""
    labels = np.asarray(labels).astype(np.int64)
    noise = np.flatnonzero(labels < 0)
    out = labels.copy()
    out[noise] = (max(int(labels.max()) + 1, 0) if labels.size else 0) + np.arange(noise.size, dtype=np.int64)
    return out


def _set_iou(a, b):
    """float64 [n]: |A(i) & B(i)| / |A(i) | B(i)| for the sets A(i), B(i) that hold sample i in the partitions ``a`` and
    ``b`` (int64 [n], every entry >= 0).  From the counts of the (a, b) pairs: O(n log n), no n x n matrix."""
    size_a = np.bincount(a)[a]
    size_b = np.bincount(b)[b]
    _, inv, cnt = np.unique(a * (int(b.max()) + 1) + b, return_inverse=True, return_counts=True)
    inter = cnt[inv.reshape(-1)]
    return inter / (size_a + size_b - inter).astype(np.float64)


class SelfPacedState(object):
    """What ``self_paced_labels`` keeps across the epochs of one run: ``tau``, the independence threshold, fixed at the
    first use that sees a cluster (None until then)."""

    def __init__(self):
        self.tau = None


def self_paced_filter(labels, tight, loose, state):
    """The cluster reliability filter of SpCL on three label vectors of the same n samples (integers, < 0 = noise): the
    clustering at eps, at eps - delta (``tight``) and at eps + delta (``loose``).  In each a noise sample is a set of its own.
    With I(i), T(i), L(i) the sets that hold sample i:

      R_indep(i) = |I(i) & L(i)| / |I(i) | L(i)|        R_comp(i) = |I(i) & T(i)| / |I(i) | T(i)|
      indep(c) = max of R_indep over the members of the eps cluster c,  comp(c) = max of R_comp over them
      state.tau (fixed at the first use): the indep(c) of the m clusters sorted descending, entry min(m - 1, round(0.9 m))
      sample i keeps its cluster iff indep(c) >= tau and R_comp(i) >= comp(c); otherwise it becomes noise

    (``round`` is Python's: halves go to the even integer.)  Returns int64 numpy [n], -1 = noise, the surviving clusters'
    ids unchanged.  Host only."""
    lab = np.asarray(labels)
    tight, loose = np.asarray(tight), np.asarray(loose)
    if lab.ndim != 1 or tight.shape != lab.shape or loose.shape != lab.shape:
        raise ValueError('self_paced_filter: three label vectors of one length are needed (got %s, %s, %s)' % (
            lab.shape, tight.shape, loose.shape))
    lab = lab.astype(np.int64)
    out = np.where(lab >= 0, lab, -1)
    kept = np.flatnonzero(lab >= 0)
    if kept.size == 0:
        return out
    si = _own_sets(lab)
    r_indep, r_comp = _set_iou(si, _own_sets(loose)), _set_iou(si, _own_sets(tight))
    ids, cl = np.unique(lab[kept], return_inverse=True)           # cl: the cluster (0 .. m - 1) of every kept sample
    cl = cl.reshape(-1)
    indep, comp = np.zeros(ids.size), np.zeros(ids.size)
    np.maximum.at(indep, cl, r_indep[kept])
    np.maximum.at(comp, cl, r_comp[kept])
    if state.tau is None:
        m = ids.size
        state.tau = float(np.sort(indep)[::-1][min(m - 1, int(round(0.9 * m)))])
    ok = (indep[cl] >= state.tau) & (r_comp[kept] >= comp[cl])
    out[kept[~ok]] = -1
    return out


def self_paced_labels(xf, state, method='jaccard', eps=0.5, delta=0.02, min_samples=4, k1=20, k2=6, metric='cosine'):
    """Self-paced pseudo-labels (SpCL's reliability criterion): DBSCAN of the rows of ``xf`` at eps - delta,
    eps and eps + delta with ``method`` 'jaccard' (engine.cluster_jaccard) or 'cosine' (engine.cluster), then
    ``self_paced_filter`` -- a cluster keeps the samples for which it is independent (it does not grow much under the
    looser eps) and compact (they stay together under the tighter one); the rest become noise, which
    ``PseudoLabels.hybrid()`` keeps as classes of their own.  ``state``: a ``SelfPacedState`` the caller keeps across the
    epochs.  Three read-backs of n labels.  ValueError before any device call: another method, delta <= 0."""
    if method not in ('jaccard', 'cosine'):
        raise ValueError("self_paced_labels: method must be 'jaccard' or 'cosine' (got %r)" % (method,))
    if not delta > 0:
        raise ValueError('self_paced_labels: delta must be > 0 (got %r)' % (delta,))
    from grl_amd import engine
    runs = []
    for e in (eps, eps - delta, eps + delta):
        res = engine.cluster_jaccard(xf, e, min_samples, k1, k2) if method == 'jaccard' else engine.cluster(xf, e, min_samples, metric)
        runs.append(PseudoLabels(res.labels, method).host)
    out = PseudoLabels(self_paced_filter(runs[0], runs[1], runs[2], state), method)
    out.labels = out.labels.to(xf.device)
    return out


def pseudo_labels(xf, method='jaccard', eps=0.5, min_samples=4, k1=20, k2=6, k=None, min_cluster_size=5, metric='cosine',
                  min_clusters=2):
    """Cluster the rows of ``xf`` [n, d] (device) into pseudo-identities:

      'jaccard'  engine.cluster_jaccard(xf, eps, min_samples, k1, k2)      eps: a k-reciprocal Jaccard distance in [0, 1]
      'cosine'   engine.cluster(xf, eps, min_samples, metric)              eps: that metric's distance (cosine: a negated dot)
      'hdbscan'  engine.hdbscan(xf, min_cluster_size, metric=metric)
      'kmeans'   engine.kmeans(xf, k, metric)                              no noise; ``k`` is required

    One read-back of the n labels.  ValueError: an unknown method, 'kmeans' without ``k`` (both before any device call), and
    fewer than ``min_clusters`` = 2 clusters -- a cross entropy over one class teaches nothing -- naming the method and its
    threshold (hybrid training, where every noise sample is a class too, passes 0)."""
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
    if out.n_clusters < min_clusters:
        raise ValueError("pseudo_labels: method %r with %s found %d cluster(s) among %d samples (%d noise); training needs "
                         'at least %d: change the threshold' % (method, knob, out.n_clusters, len(out), out.n_noise,
                                                                min_clusters))
    return out


def train_unsupervised(trainer, evaluator, optimizer, tracklets, make_eval_loader, make_train_loader, epochs,
                       label_kwargs=None, on_epoch=None, cameras=False, inter_from_epoch=0, hybrid=False, self_paced=None):
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

    ``hybrid=True`` (self-paced hybrid memory): ``trainer`` is a ``HybridSEQTrainer`` whose two criteria are
    ``HybridMemoryLoss`` and ``cameras`` is false (checked before any device call); the train loader must be built on
    ``RawVideoDataset(.., index=True)``.  Both memories are seeded from ``h = labels.hybrid()`` --
    ``reset(h.memory(xf, cols), h.class_ptr_dev, h.class_members_dev, h.inst_class_dev)`` -- and the epoch trains on
    ``h.relabel(tracklets)``: ALL tracklets, the noise samples as classes of their own (``pseudo_labels`` is then called
    with ``min_clusters=0`` unless ``label_kwargs`` says otherwise).  ``self_paced``: a dict with ``delta`` and the
    method's knobs (``method``, ``eps``, ``min_samples``, ``k1``, ``k2``, ``metric``); the labels then come from
    ``self_paced_labels(xf, state, **self_paced)`` with one ``SelfPacedState`` for the run, and ``label_kwargs`` is unused.

    A mean teacher needs nothing here: a ``MeanTeacherSEQTrainer`` with two ``SoftClusterMemoryLoss`` goes
    through the plain branch -- ``reset(centroids)`` is ``ClusterMemoryLoss``'s -- and the caller chooses the model that is
    clustered by the evaluator it passes: ``ATTEvaluator(*teacher.models)`` clusters with the teacher.  The same holds with
    ``hybrid=True`` and ``cameras=True``: ``MeanTeacherHybridSEQTrainer`` / ``MeanTeacherCameraSEQTrainer`` and
    their ``SoftHybridMemoryLoss`` / ``SoftProxyMemoryLoss`` are subclasses of what the checks above ask for.

    Returns the epochs' ``PseudoLabels``.  Under torch.distributed ``extract_feature`` gathers every row on every rank, so
    all ranks compute the same labels and seed the same memories."""
    tracklets = list(tracklets)
    if hybrid:
        from grl_amd.reid.loss import HybridMemoryLoss
        from grl_amd.reid.train.hybrid import HybridSEQTrainer
        if cameras:
            raise ValueError('train_unsupervised: hybrid=True with cameras=True is not built (one of the two)')
        if not isinstance(trainer, HybridSEQTrainer):
            raise ValueError('train_unsupervised: hybrid=True needs a HybridSEQTrainer (got %s): SEQTrainer has no place '
                             "for the batch's instance indices" % type(trainer).__name__)
        for name in ('criterion_corr', 'criterion_uncorr'):
            if not isinstance(getattr(trainer, name), HybridMemoryLoss):
                raise ValueError('train_unsupervised: hybrid=True needs %s to be a HybridMemoryLoss (got %s)' % (
                    name, type(getattr(trainer, name)).__name__))
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
    if self_paced is not None:
        if not hybrid:
            raise ValueError('train_unsupervised: self_paced needs hybrid=True (the samples it turns into noise would be '
                             'dropped from the epoch)')
        if not isinstance(self_paced, dict) or 'delta' not in self_paced:
            raise ValueError("train_unsupervised: self_paced must be a dict with 'delta' and the method's knobs (got %r)" % (
                self_paced,))
        state = SelfPacedState()
    history = []
    for epoch in range(epochs):
        xf = evaluator.extract_feature(make_eval_loader(tracklets))[0]
        if xf.dim() != 2 or xf.shape[0] != len(tracklets) or xf.shape[1] < CORR_COLS[1]:
            raise ValueError('train_unsupervised: the eval loader gave features %s for %d tracklets (one row of at least '
                             '%d columns per tracklet is needed)' % (tuple(xf.shape), len(tracklets), CORR_COLS[1]))
        if self_paced is not None:
            labels = self_paced_labels(xf, state, **self_paced)
        elif hybrid:
            labels = pseudo_labels(xf, **dict(dict(min_clusters=0), **(label_kwargs or {})))
        else:
            labels = pseudo_labels(xf, **(label_kwargs or {}))
        train_list = None
        if hybrid:
            h = labels.hybrid()
            for crit, cols in ((trainer.criterion_uncorr, UNCORR_COLS), (trainer.criterion_corr, CORR_COLS)):
                crit.reset(h.memory(xf, cols=cols), h.class_ptr_dev, h.class_members_dev, h.inst_class_dev)
            train_list = h.relabel(tracklets)
        elif cameras:
            proxies = labels.proxies([t[2] for t in tracklets])
            for crit, cols in ((trainer.criterion_uncorr, UNCORR_COLS), (trainer.criterion_corr, CORR_COLS)):
                crit.reset(proxies.centroids(xf, cols=cols), proxies.proxy_cluster_dev, proxies.proxy_cam_dev)
                crit.inter_on = epoch >= inter_from_epoch
        else:
            trainer.criterion_uncorr.reset(labels.centroids(xf, cols=UNCORR_COLS))
            trainer.criterion_corr.reset(labels.centroids(xf, cols=CORR_COLS))
        trainer.train(epoch, make_train_loader(labels.relabel(tracklets) if train_list is None else train_list), optimizer)
        history.append(labels)
        if on_epoch is not None:
            on_epoch(epoch, labels)
    return history
