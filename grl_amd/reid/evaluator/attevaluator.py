"""ATTEvaluator with the reference's constructor and methods
(/root/reference/reid/evaluator/attevaluator.py:49-163).  Feature extraction and
the query x gallery distance matrix run on the GPU through grl_amd.engine; the
ranking metrics stay on the host."""
import math
import os

import numpy as np
import torch

from grl_amd import engine
from grl_amd import dist as grl_dist
from .eva_functions import evaluate
from .rerank import re_ranking
from .visualize import visualize_ranked_results

__all__ = ['ATTEvaluator', 'evaluate_seq', 'cosin_dist', 'pairwise_distance_tensor', 'visualize_ranked_results']


def evaluate_seq(distmat, query_pids, query_camids, gallery_pids, gallery_camids, path,
                 cmc_topk=(1, 5, 10, 20), indices=None, roc_lines=()):
    """Prints mAP / Rank-k in the reference's format and returns Rank-1
    (attevaluator.py:15-30)."""
    cmc_scores, mAP = evaluate(distmat, np.array(query_pids), np.array(gallery_pids),
                               np.array(query_camids), np.array(gallery_camids), indices=indices)
    return _report(cmc_scores, mAP, cmc_topk, roc_lines)


def _report(cmc_scores, mAP, cmc_topk=(1, 5, 10, 20), roc_lines=()):
    print('Mean AP: {:4.1%}'.format(mAP))
    for r in cmc_topk:
        print("Rank-{:<3}: {:.1%}".format(r, cmc_scores[r - 1]))
    for line in roc_lines:                    # GRL_EVAL_ROC / GRL_EVAL_CLUSTER: the extra figures; none by default
        print(line)
    print("------------------")
    return cmc_scores[0]


def _roc_report(roc, metric_name, path):
    """GRL_EVAL_ROC: the lines ``_report`` prints after the CMC for a ``engine.PairRoc``, and ``path + 'roc.json'``
    (rank 0 alone writes): the scalar figures, ``bits``, the metric's name and the curve over the non-empty bins.
    Strict JSON: a threshold that is not finite (the +inf bin, the NaN bin) is null."""
    import json
    s = roc.summary()
    lines = ['ROC AUC: {:.2%} (+/- {:.1e} from binning; n_pos = {}, n_neg = {})'.format(s['auc'], s['auc_slack'],
                                                                                     s['n_pos'], s['n_neg']),
             'EER: {:.2%}'.format(s['eer']),
             'TPR@FPR=1e-3: {:.2%}'.format(s['tpr_at_fpr']['0.001']),
             'TPR@FPR=1e-2: {:.2%}'.format(s['tpr_at_fpr']['0.01'])]
    if grl_dist._rank_world(None, None)[0] == 0:
        fpr, tpr, thr = roc.curve()
        s['metric'] = metric_name
        s['curve'] = {'fpr': fpr.tolist(), 'tpr': tpr.tolist(),
                      'threshold': [float(t) if np.isfinite(t) else None for t in thr]}
        with open((path or '') + 'roc.json', 'w') as fh:
            json.dump(s, fh, allow_nan=False)
    return lines


def _silhouette_report(sil, gf, labels, js):
    """GRL_EVAL_SILHOUETTE: the label-free score of a report's ``labels`` on the features ``gf`` (engine.silhouette) --
    the report's third line, and its JSON's "silhouette" entry (a score that is not finite is null; labels with fewer
    than 2 clusters have no silhouette: the line says so and the entry's score is null).  ``sil`` = (metric, noise) or
    None, which adds nothing."""
    if sil is None:
        return []
    metric, noise = sil
    lab = labels.cpu().numpy()
    if np.unique(lab[lab >= 0]).size + (int((lab < 0).sum()) if noise == 'singleton' else 0) < 2:
        js['silhouette'] = {'metric': metric, 'noise': noise, 'score': None, 'n_scored': 0, 'n_clusters': 0}
        return ['Silhouette ({}): undefined, fewer than 2 clusters'.format(metric)]
    r = engine.silhouette(gf, labels, metric, noise)
    js['silhouette'] = {'metric': metric, 'noise': noise, 'score': r.score if math.isfinite(r.score) else None,
                        'n_scored': r.n_scored, 'n_clusters': r.n_clusters}
    return ['Silhouette ({}): {:.4f} over {} of {} samples, {} clusters'.format(
        metric, r.score, r.n_scored, int(gf.size(0)), r.n_clusters)]


def _cluster_report(knob, qf, gf, ids, path, roc=None, sil=None):
    """GRL_EVAL_CLUSTER: DBSCAN of the query-prepended gallery ``gf`` by cosine (engine.cluster) -- the two lines
    ``_report`` prints after any ROC lines, and ``path + 'clusters.json'`` (rank 0 alone writes; strict JSON).
    ``knob`` = (eps or 'eer', min_samples); 'eer' is the ``eer_threshold`` of the cosine ``engine.pair_roc`` of
    (qf, gf), taken from ``roc`` when the route has already computed that one.  ``sil`` (GRL_EVAL_SILHOUETTE): a third
    line and the JSON's "silhouette" entry (``_silhouette_report``)."""
    import json
    eps, min_samples = knob
    if eps == 'eer':
        if roc is None:
            roc = engine.pair_roc(qf, gf, *ids)
        eps = float(roc.eer_threshold)
        if not math.isfinite(eps):
            raise ValueError('GRL_EVAL_CLUSTER=eer: the threshold at the equal error rate is %r, not a finite distance '
                             '(the pairs are not separable by a finite cosine threshold); give eps as a number' % eps)
    cl = engine.cluster(gf, eps, min_samples)
    n = int(gf.size(0))
    scores = cl.pair_scores(ids[1])
    lines = ['Clusters: {} ({} noise of {}) at cosine eps = {:g}, min_samples = {}'.format(
                 cl.n_clusters, cl.n_noise, n, cl.eps, cl.min_samples),
             'Pairwise precision: {:.2%}  recall: {:.2%}  F1: {:.2%}  ARI: {:.4f}'.format(
                 scores['precision'], scores['recall'], scores['f1'], scores['ari'])]
    js = {'eps': cl.eps, 'min_samples': cl.min_samples, 'metric': 'cosine', 'n': n, 'n_clusters': cl.n_clusters,
          'n_noise': cl.n_noise, 'n_edges': cl.n_edges, 'pair_scores': scores, 'labels': cl.labels.cpu().tolist()}
    lines += _silhouette_report(sil, gf, cl.labels, js)
    if grl_dist._rank_world(None, None)[0] == 0:
        with open((path or '') + 'clusters.json', 'w') as fh:
            json.dump(js, fh, allow_nan=False)
    return lines


def _cluster_jaccard_report(knob, gf, ids, path, sil=None):
    """GRL_EVAL_CLUSTER_JACCARD: DBSCAN of the query-prepended gallery ``gf`` on the k-reciprocal Jaccard distance
    (engine.cluster_jaccard) -- the two lines ``_report`` prints after GRL_EVAL_CLUSTER's, and
    ``path + 'cluster_jaccard.json'`` (rank 0 alone writes; strict JSON): the fields of clusters.json plus k1 and k2.
    ``knob`` = (eps, min_samples, k1, k2).  ``sil`` (GRL_EVAL_SILHOUETTE): a third line and the JSON's "silhouette"
    entry -- the score of the Jaccard LABELS under the feature metric (cosine or Euclidean distance of the rows of
    ``gf``), not under the Jaccard distance itself, which is sparse and has no silhouette kernel."""
    import json
    eps, min_samples, k1, k2 = knob
    cl = engine.cluster_jaccard(gf, eps, min_samples, k1, k2)
    n = int(gf.size(0))
    scores = cl.pair_scores(ids[1])
    lines = ['Jaccard clusters: {} ({} noise of {}) at eps = {:g}, min_samples = {}, k1 = {}, k2 = {}'.format(
                 cl.n_clusters, cl.n_noise, n, cl.eps, cl.min_samples, k1, k2),
             'Pairwise precision: {:.2%}  recall: {:.2%}  F1: {:.2%}  ARI: {:.4f}'.format(
                 scores['precision'], scores['recall'], scores['f1'], scores['ari'])]
    js = {'eps': cl.eps, 'min_samples': cl.min_samples, 'metric': 'jaccard', 'k1': k1, 'k2': k2, 'n': n,
          'n_clusters': cl.n_clusters, 'n_noise': cl.n_noise, 'n_edges': cl.n_edges, 'pair_scores': scores,
          'labels': cl.labels.cpu().tolist()}
    lines += _silhouette_report(sil, gf, cl.labels, js)
    if grl_dist._rank_world(None, None)[0] == 0:
        with open((path or '') + 'cluster_jaccard.json', 'w') as fh:
            json.dump(js, fh, allow_nan=False)
    return lines


def _kmeans_report(knob, gf, ids, path, sil=None):
    """GRL_EVAL_KMEANS: spherical k-means of the query-prepended gallery ``gf`` (engine.kmeans, 'cosine', random
    initial rows) -- the two lines ``_report`` prints last, and ``path + 'kmeans.json'`` (rank 0 alone writes; strict
    JSON, no centroids).  ``knob`` = (k or 'ids', max_iter, seed); 'ids' is the number of distinct pids in ``gf``.
    ``sil`` (GRL_EVAL_SILHOUETTE): a third line and the JSON's "silhouette" entry (``_silhouette_report``)."""
    import json
    k, max_iter, seed = knob
    if k == 'ids':
        k = int(np.unique(np.asarray(ids[1])).size)
    km = engine.kmeans(gf, k, 'cosine', 'random', seed, max_iter)
    n = int(gf.size(0))
    scores = km.pair_scores(ids[1])
    lines = ['K-means: {} clusters of {} ({} iterations, {}, {} empty), inertia = {:.6g}'.format(
                 km.k, n, km.n_iter, 'converged' if km.converged else 'not converged', km.n_empty, km.inertia),
             'Pairwise precision: {:.2%}  recall: {:.2%}  F1: {:.2%}  ARI: {:.4f}'.format(
                 scores['precision'], scores['recall'], scores['f1'], scores['ari'])]
    js = {'k': km.k, 'max_iter': max_iter, 'seed': seed, 'init': 'random', 'metric': 'cosine', 'n': n,
          'n_iter': km.n_iter, 'converged': km.converged, 'n_changed': km.n_changed, 'n_empty': km.n_empty,
          'n_unassigned': km.n_unassigned, 'inertia': km.inertia if math.isfinite(km.inertia) else None,
          'counts': km.counts.cpu().tolist(), 'pair_scores': scores, 'labels': km.labels.cpu().tolist()}
    lines += _silhouette_report(sil, gf, km.labels, js)
    if grl_dist._rank_world(None, None)[0] == 0:
        with open((path or '') + 'kmeans.json', 'w') as fh:
            json.dump(js, fh, allow_nan=False)
    return lines


def _hdbscan_report(knob, gf, ids, path, sil=None):
    """GRL_EVAL_HDBSCAN: HDBSCAN of the query-prepended gallery ``gf`` by cosine (engine.hdbscan) -- the two lines
    ``_report`` prints after GRL_EVAL_KMEANS's, and ``path + 'hdbscan.json'`` (rank 0 alone writes; strict JSON, no
    edges).  ``knob`` = (min_cluster_size, min_samples or None, method).  ``sil`` (GRL_EVAL_SILHOUETTE): a third line and
    the JSON's "silhouette" entry (``_silhouette_report``)."""
    import json
    mcs, ms, method = knob
    n = int(gf.size(0))
    hd = engine.hdbscan(gf, mcs, ms, 'cosine', method)
    scores = hd.pair_scores(ids[1])
    lines = ['HDBSCAN: {} clusters ({} noise of {}) at min_cluster_size = {}, min_samples = {}, {} ({} rounds)'.format(
                 hd.n_clusters, hd.n_noise, n, hd.min_cluster_size, hd.min_samples, hd.method, hd.rounds),
             'Pairwise precision: {:.2%}  recall: {:.2%}  F1: {:.2%}  ARI: {:.4f}'.format(
                 scores['precision'], scores['recall'], scores['f1'], scores['ari'])]
    js = {'min_cluster_size': hd.min_cluster_size, 'min_samples': hd.min_samples, 'method': hd.method,
          'metric': 'cosine', 'n': n, 'n_clusters': hd.n_clusters, 'n_noise': hd.n_noise, 'n_edges': int(hd.mst[0].numel()),
          'rounds': hd.rounds, 'n_dropped': hd.n_dropped, 'stabilities': hd.stabilities.tolist(),
          'pair_scores': scores, 'labels': hd.labels.cpu().tolist()}
    lines += _silhouette_report(sil, gf, hd.labels, js)
    if grl_dist._rank_world(None, None)[0] == 0:
        with open((path or '') + 'hdbscan.json', 'w') as fh:
            json.dump(js, fh, allow_nan=False)
    return lines


def _tsne_report(knob, gf, ids, path):
    """GRL_EVAL_TSNE: the 2-d t-SNE map of the query-prepended gallery ``gf`` by cosine (engine.tsne) -- the line
    ``_report`` prints after GRL_EVAL_HDBSCAN's, ``path + 'tsne.json'`` (rank 0 alone writes; strict JSON, the NaN
    coordinates of an isolated sample become null; the rows are in the order of the ``labels`` of clusters.json /
    hdbscan.json, so a clustering colours the map without a join) and, when matplotlib imports, ``path + 'tsne.png'``: a
    scatter coloured by pid, the queries ringed.  ``knob`` = (perplexity, n_iter, seed)."""
    import json
    perplexity, n_iter, seed = knob
    n = int(gf.size(0))
    nq = n - (len(ids[1]) - len(ids[0]))
    ts = engine.tsne(gf, perplexity, 'cosine', n_iter, seed)
    lines = ['t-SNE: KL = {:.6g}, perplexity = {:g}, {} iterations, {} isolated of {}'.format(
                 ts.kl, ts.perplexity, ts.n_iter, ts.n_isolated, n)]
    if grl_dist._rank_world(None, None)[0] != 0:
        return lines
    emb = ts.embedding.cpu().numpy()
    js = {'perplexity': ts.perplexity, 'n_iter': ts.n_iter, 'seed': ts.seed, 'metric': 'cosine', 'n': n, 'n_queries': nq,
          'kl': ts.kl if math.isfinite(ts.kl) else None, 'n_isolated': ts.n_isolated,
          'embedding': [[float(v) if np.isfinite(v) else None for v in row] for row in emb],
          'pids': [int(p) for p in ids[1]], 'camids': [int(c) for c in ids[3]]}
    with open((path or '') + 'tsne.json', 'w') as fh:
        json.dump(js, fh, allow_nan=False)
    try:
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
    except ImportError:
        lines.append('t-SNE: matplotlib does not import, no tsne.png (the map is in tsne.json)')
        return lines
    pids = np.asarray(ids[1])
    colour = np.unique(pids, return_inverse=True)[1]
    fig, ax = plt.subplots(figsize=(8, 8))
    ax.scatter(emb[:, 0], emb[:, 1], c=colour, cmap='nipy_spectral', s=6, linewidths=0)
    ax.scatter(emb[:nq, 0], emb[:nq, 1], s=30, facecolors='none', edgecolors='k', linewidths=0.6)
    ax.set_title('t-SNE of {} samples ({} queries ringed), perplexity {:g}, KL {:.4g}'.format(n, nq, ts.perplexity, ts.kl))
    ax.set_xticks([])
    ax.set_yticks([])
    fig.savefig((path or '') + 'tsne.png', dpi=150, bbox_inches='tight')
    plt.close(fig)
    return lines


def cosin_dist(qf, gf):
    return engine.cosin_dist(qf, gf)


def pairwise_distance_tensor(query_x, gallery_x):
    return engine.pairwise_distance_tensor(query_x, gallery_x)


def parse_expand_knob(name, value):
    """``GRL_EVAL_QE`` / ``GRL_EVAL_DBA``: "m" or "m,alpha" -> (m, alpha); unset or empty -> None.  Anything else is a
    ValueError that names the variable (the ranges are engine.expand_features')."""
    if value is None or not value.strip():
        return None
    parts = [p.strip() for p in value.split(',')]
    try:
        if len(parts) > 2:
            raise ValueError
        m, alpha = int(parts[0]), (int(parts[1]) if len(parts) == 2 else 0)
    except ValueError:
        raise ValueError('%s must be "m" or "m,alpha" with integer m and alpha (got %r)' % (name, value))
    if not 1 <= m <= engine.SEARCH_K_MAX - 1 or not 0 <= alpha <= engine.EXPAND_ALPHA_MAX:
        raise ValueError('%s: m must be in 1..%d and alpha in 0..%d (got %r)'
                         % (name, engine.SEARCH_K_MAX - 1, engine.EXPAND_ALPHA_MAX, value))
    return m, alpha


def parse_metric_knob(name, value):
    """``GRL_EVAL_METRIC``: unset, empty or "cosine" -> None (the cosine ranking); "verify" or "verify,beta" ->
    ('verify', beta) with a float beta in (0, 1] (default 1: the verification head alone; engine.verify_metric).
    Anything else is a ValueError that names the variable."""
    if value is None or not value.strip() or value.strip() == 'cosine':
        return None
    parts = [p.strip() for p in value.split(',')]
    try:
        if parts[0] != 'verify' or len(parts) > 2:
            raise ValueError
        beta = float(parts[1]) if len(parts) == 2 else 1.0
    except ValueError:
        raise ValueError('%s must be "cosine", "verify" or "verify,beta" with a float beta (got %r)' % (name, value))
    if not 0.0 < beta <= 1.0:              # (NaN fails both comparisons)
        raise ValueError('%s: beta must be in (0, 1] (got %r)' % (name, value))
    return 'verify', beta


def parse_roc_knob(name, value):
    """``GRL_EVAL_ROC``: unset or empty -> None (off); "1" -> engine.ROC_BITS_DEFAULT (16); an integer in 8..20 -> that
    many histogram bits (engine.pair_roc).  Anything else is a ValueError that names the variable."""
    if value is None or not value.strip():
        return None
    try:
        bits = int(value.strip())
    except ValueError:
        raise ValueError('%s must be "1" or an integer number of histogram bits (got %r)' % (name, value))
    if bits == 1:
        return engine.ROC_BITS_DEFAULT
    if not engine.ROC_BITS_MIN <= bits <= engine.ROC_BITS_MAX:
        raise ValueError('%s: bits must be 1 (the default, %d) or in %d..%d (got %r)'
                         % (name, engine.ROC_BITS_DEFAULT, engine.ROC_BITS_MIN, engine.ROC_BITS_MAX, value))
    return bits


def parse_cluster_knob(name, value):
    """``GRL_EVAL_CLUSTER``: unset or empty -> None (off); "eps" or "eps,min_samples" -> (eps, min_samples) with eps a
    float (a cosine distance: a negated dot product) or the word "eer", and an integer min_samples >= 1 (default 1;
    engine.cluster).  Anything else is a ValueError that names the variable."""
    if value is None or not value.strip():
        return None
    parts = [p.strip() for p in value.split(',')]
    try:
        if len(parts) > 2:
            raise ValueError
        eps = 'eer' if parts[0] == 'eer' else float(parts[0])
        min_samples = int(parts[1]) if len(parts) == 2 else 1
    except ValueError:
        raise ValueError('%s must be "eps" or "eps,min_samples" with eps a float or "eer" and an integer min_samples '
                         '(got %r)' % (name, value))
    if eps != eps or not 1 <= min_samples <= 2 ** 31 - 1:
        raise ValueError('%s: eps must not be NaN and min_samples must be >= 1 (got %r)' % (name, value))
    return eps, min_samples


def parse_cluster_jaccard_knob(name, value):
    """``GRL_EVAL_CLUSTER_JACCARD``: unset or empty -> None (off); "eps", "eps,min_samples", "eps,min_samples,k1" or
    "eps,min_samples,k1,k2" -> (eps, min_samples, k1, k2) with eps a finite float below 1 (a Jaccard distance), an
    integer min_samples >= 1 (default 1), k1 in 1..20 (default 20) and k2 in 1..8 (default 6; engine.cluster_jaccard).
    Anything else is a ValueError that names the variable."""
    if value is None or not value.strip():
        return None
    parts = [p.strip() for p in value.split(',')]
    try:
        if len(parts) > 4:
            raise ValueError
        eps = float(parts[0])
        min_samples, k1, k2 = [int(p) for p in parts[1:]] + [1, 20, 6][len(parts) - 1:]
    except ValueError:
        raise ValueError('%s must be "eps[,min_samples[,k1[,k2]]]" with a float eps and integer min_samples, k1 and k2 '
                         '(got %r)' % (name, value))
    if not (math.isfinite(eps) and float(np.float32(eps)) < 1.0):
        raise ValueError('%s: eps is a Jaccard distance threshold, finite and below 1 (got %r)' % (name, value))
    if not (1 <= min_samples <= 2 ** 31 - 1 and 1 <= k1 <= engine.RERANK_K1_MAX and 1 <= k2 <= engine.RERANK_K2_MAX):
        raise ValueError('%s: min_samples must be >= 1, k1 in 1..%d and k2 in 1..%d (got %r)'
                         % (name, engine.RERANK_K1_MAX, engine.RERANK_K2_MAX, value))
    return eps, min_samples, k1, k2


def parse_kmeans_knob(name, value):
    """``GRL_EVAL_KMEANS``: unset or empty -> None (off); "k", "k,max_iter" or "k,max_iter,seed" -> (k, max_iter,
    seed) with k an integer >= 1 or the word "ids" (the number of distinct pids in the query-prepended gallery), an
    integer max_iter >= 1 (default 50) and an integer seed >= 0 (default 0; engine.kmeans).  Anything else is a
    ValueError that names the variable."""
    if value is None or not value.strip():
        return None
    parts = [p.strip() for p in value.split(',')]
    try:
        if len(parts) > 3:
            raise ValueError
        k = 'ids' if parts[0] == 'ids' else int(parts[0])
        max_iter = int(parts[1]) if len(parts) >= 2 else 50
        seed = int(parts[2]) if len(parts) == 3 else 0
    except ValueError:
        raise ValueError('%s must be "k", "k,max_iter" or "k,max_iter,seed" with k an integer or "ids" and integer '
                         'max_iter and seed (got %r)' % (name, value))
    if (k != 'ids' and not 1 <= k <= 2 ** 31 - 1) or not 1 <= max_iter <= 2 ** 31 - 1 or seed < 0:
        raise ValueError('%s: k and max_iter must be >= 1 and seed >= 0 (got %r)' % (name, value))
    return k, max_iter, seed


def parse_hdbscan_knob(name, value):
    """``GRL_EVAL_HDBSCAN``: unset or empty -> None (off); "min_cluster_size", "min_cluster_size,min_samples" or
    "min_cluster_size,min_samples,method" -> (min_cluster_size, min_samples or None, method) with an integer
    min_cluster_size >= 2, an integer min_samples in 1..1024 (default None: min_cluster_size) and method "eom" (the
    default) or "leaf" (engine.hdbscan).  Anything else is a ValueError that names the variable."""
    if value is None or not value.strip():
        return None
    parts = [p.strip() for p in value.split(',')]
    try:
        if len(parts) > 3:
            raise ValueError
        mcs = int(parts[0])
        ms = int(parts[1]) if len(parts) >= 2 else None
        method = parts[2] if len(parts) == 3 else 'eom'
    except ValueError:
        raise ValueError('%s must be "min_cluster_size", "min_cluster_size,min_samples" or '
                         '"min_cluster_size,min_samples,method" with integers and method "eom" or "leaf" (got %r)'
                         % (name, value))
    if not 2 <= mcs <= 2 ** 31 - 1 or (ms is not None and not 1 <= ms <= engine.SEARCH_K_MAX) \
            or method not in engine.HDBSCAN_METHODS:
        raise ValueError('%s: min_cluster_size must be >= 2, min_samples in 1..%d and method "eom" or "leaf" (got %r)'
                         % (name, engine.SEARCH_K_MAX, value))
    return mcs, ms, method


def parse_tsne_knob(name, value):
    """``GRL_EVAL_TSNE``: unset or empty -> None (off); "perplexity", "perplexity,n_iter" or "perplexity,n_iter,seed" ->
    (perplexity, n_iter, seed) with a perplexity in [1, 341) ("1" alone means 30), an integer n_iter >= 1 (default
    1000) and an integer seed >= 0 (default 0; engine.tsne).  Anything else is a ValueError that names the variable."""
    if value is None or not value.strip():
        return None
    parts = [p.strip() for p in value.split(',')]
    try:
        if len(parts) > 3:
            raise ValueError
        perplexity = 30.0 if parts == ['1'] else float(parts[0])
        n_iter = int(parts[1]) if len(parts) >= 2 else 1000
        seed = int(parts[2]) if len(parts) == 3 else 0
    except ValueError:
        raise ValueError('%s must be "perplexity", "perplexity,n_iter" or "perplexity,n_iter,seed" with a number and '
                         'integers ("1" alone: perplexity 30, 1000 iterations, seed 0) (got %r)' % (name, value))
    if not 1.0 <= perplexity < (engine.SEARCH_K_MAX - 1) // 3 or not 1 <= n_iter <= 2 ** 31 - 1 or seed < 0:
        raise ValueError('%s: perplexity must be in [1, %d), n_iter >= 1 and seed >= 0 (got %r)'
                         % (name, (engine.SEARCH_K_MAX - 1) // 3, value))
    return perplexity, n_iter, seed


def parse_pca_knob(name, value):
    """``GRL_EVAL_PCA``: unset or empty -> None (off); "r" or "r,whiten" -> (r, whiten) with an integer r in 1..502 (the
    components kept; engine.pca adds 10 of oversampling and holds 512 directions) and whiten 0 or 1 (default 0).
    Anything else is a ValueError that names the variable."""
    if value is None or not value.strip():
        return None
    parts = [p.strip() for p in value.split(',')]
    try:
        if len(parts) > 2:
            raise ValueError
        r = int(parts[0])
        whiten = int(parts[1]) if len(parts) == 2 else 0
    except ValueError:
        raise ValueError('%s must be "r" or "r,whiten" with an integer r and whiten 0 or 1 (got %r)' % (name, value))
    if not 1 <= r <= engine.PCA_LMAX - 10 or whiten not in (0, 1):
        raise ValueError('%s: r must be in 1..%d and whiten 0 or 1 (got %r)' % (name, engine.PCA_LMAX - 10, value))
    return r, bool(whiten)


def _pca_report(knob, qf, gf, path):
    """GRL_EVAL_PCA: fit engine.pca on the query-prepended gallery ``gf`` and return the transforms of ``qf`` and ``gf``
    (r columns, whitened or not; zero columns are appended up to a multiple of 32, the width the distance GEMMs take --
    they add +0 to every dot product and norm) -- one printed line and ``path + 'pca.json'`` (rank 0 alone writes;
    strict JSON)."""
    import json
    r, whiten = knob
    fit = engine.pca(gf, r)
    lam = [float(v) for v in fit.explained_variance.cpu()]
    ratio = float(fit.explained_variance_ratio.double().sum())
    print('PCA: r = {}, whiten = {}, explained variance ratio = {:.6g}, lambda_1 = {:.6g}, lambda_r = {:.6g}'.format(
        r, int(whiten), ratio, lam[0], lam[-1]))
    if grl_dist._rank_world(None, None)[0] == 0:
        js = {'n_components': r, 'whiten': bool(whiten), 'explained_variance_ratio_sum': ratio, 'lambda_1': lam[0],
              'lambda_r': lam[-1], 'explained_variance': lam, 'total_variance': fit.total_variance,
              'n_samples': fit.n_samples, 'oversample': fit.oversample, 'n_iter': fit.n_iter, 'seed': fit.seed,
              'sweeps': fit.sweeps, 'min_pivot': fit.min_pivot}
        with open((path or '') + 'pca.json', 'w') as fh:
            json.dump(js, fh, allow_nan=False)
    return engine._pad_features(fit.transform(qf, whiten)), engine._pad_features(fit.transform(gf, whiten))


def parse_diffusion_knob(name, value):
    """``GRL_EVAL_DIFFUSION``: unset or empty -> None (off); "k", "k,kq", "k,kq,alpha" or "k,kq,alpha,n_iter" -> (k, kq,
    alpha, n_iter) with integers k in 1..128 (graph neighbours) and kq in 1..k (query seeds; default 10, or k when k is
    smaller), a float alpha in [0, 1) (default 0.99) and an integer n_iter >= 0 (default 20; engine.diffusion_search).
    Anything else is a ValueError that names the variable."""
    if value is None or not value.strip():
        return None
    parts = [p.strip() for p in value.split(',')]
    try:
        if len(parts) > 4:
            raise ValueError
        k = int(parts[0])
        kq = int(parts[1]) if len(parts) >= 2 else min(10, k)
        alpha = float(parts[2]) if len(parts) >= 3 else 0.99
        n_iter = int(parts[3]) if len(parts) == 4 else 20
    except ValueError:
        raise ValueError('%s must be "k[,kq[,alpha[,n_iter]]]" with integers k, kq and n_iter and a float alpha (got %r)'
                         % (name, value))
    if not 1 <= k <= engine.DIFFUSION_K_MAX or not 1 <= kq <= k or not 0.0 <= alpha < 1.0 \
            or not 0 <= n_iter <= 2 ** 31 - 1:              # (a NaN alpha fails both comparisons)
        raise ValueError('%s: k must be in 1..%d, kq in 1..k, alpha in [0, 1) and n_iter >= 0 (got %r)'
                         % (name, engine.DIFFUSION_K_MAX, value))
    return k, kq, alpha, n_iter


def _diffusion_report(knob, gf, path):
    """GRL_EVAL_DIFFUSION: the mutual-kNN graph of the query-prepended gallery ``gf`` (engine.diffusion_graph, gamma = 3)
    -- one printed line with its edges and isolated rows, and ``path + 'diffusion.json'`` (rank 0 alone writes; strict
    JSON).  Returns the graph, which the ranking and ``--visual`` reuse."""
    import json
    k, kq, alpha, n_iter = knob
    graph = engine.diffusion_graph(gf, k)
    print('Diffusion: k = {}, kq = {}, alpha = {:g}, n_iter = {}, gamma = {}: {} edges, {} isolated of {}'.format(
        k, kq, alpha, n_iter, graph.gamma, graph.n_edges, graph.n_isolated, graph.n))
    if grl_dist._rank_world(None, None)[0] == 0:
        js = {'k': k, 'kq': kq, 'alpha': alpha, 'n_iter': n_iter, 'gamma': graph.gamma, 'metric': 'cosine', 'n': graph.n,
              'n_edges': graph.n_edges, 'n_isolated': graph.n_isolated}
        with open((path or '') + 'diffusion.json', 'w') as fh:
            json.dump(js, fh, allow_nan=False)
    return graph


def parse_silhouette_knob(name, value):
    """``GRL_EVAL_SILHOUETTE``: unset or empty -> None (off); "1" or "cosine", or "euclidean", optionally followed by
    ",drop" or ",singleton" -> (metric, noise) for engine.silhouette (default noise: 'singleton', the convention of
    ``pair_scores``).  Anything else is a ValueError that names the variable."""
    if value is None or not value.strip():
        return None
    parts = [p.strip() for p in value.split(',')]
    metric = {'1': 'cosine', 'cosine': 'cosine', 'euclidean': 'euclidean'}.get(parts[0])
    if metric is None or len(parts) > 2 or (len(parts) == 2 and parts[1] not in ('drop', 'singleton')):
        raise ValueError('%s must be "1", "cosine" or "euclidean", optionally followed by ",drop" or ",singleton" '
                         '(got %r)' % (name, value))
    return metric, parts[1] if len(parts) == 2 else 'singleton'


def parse_set_knob(name, value):
    """``GRL_EVAL_SET``: unset or empty -> None (off); "min", "mean", "chamfer" or "hausdorff", optionally followed by
    ",cosine" or ",euclidean" -> (reduce, metric) for engine.set_metrics_streaming (default metric: 'cosine').  Anything
    else is a ValueError that names the variable."""
    if value is None or not value.strip():
        return None
    parts = [p.strip() for p in value.split(',')]
    if parts[0] not in engine.SET_REDUCE or len(parts) > 2 or (len(parts) == 2 and parts[1] not in engine.SET_METRICS):
        raise ValueError('%s must be "min", "mean", "chamfer" or "hausdorff", optionally followed by ",cosine" or '
                         '",euclidean" (got %r)' % (name, value))
    return parts[0], parts[1] if len(parts) == 2 else 'cosine'


def parse_pq_knob(name, value):
    """``GRL_EVAL_PQ``: unset or empty -> None (off); "M", "M,nbits", "M,nbits,max_iter" or "M,nbits,max_iter,seed" -> (M,
    nbits, max_iter, seed) with an integer M >= 1 (the subspaces; it must divide the feature size into parts of a multiple
    of 32 columns, which engine.pq_train checks against the features), nbits in 4..8 (default 8), max_iter >= 1 (default
    25) and seed >= 0 (default 0).  Anything else is a ValueError that names the variable."""
    if value is None or not value.strip():
        return None
    parts = [p.strip() for p in value.split(',')]
    try:
        if len(parts) > 4:
            raise ValueError
        M = int(parts[0])
        nbits = int(parts[1]) if len(parts) >= 2 else 8
        max_iter = int(parts[2]) if len(parts) >= 3 else 25
        seed = int(parts[3]) if len(parts) == 4 else 0
    except ValueError:
        raise ValueError('%s must be "M", "M,nbits", "M,nbits,max_iter" or "M,nbits,max_iter,seed" with integers (got %r)'
                         % (name, value))
    if not 1 <= M <= engine.PQ_M_MAX or not 4 <= nbits <= 8 or not 1 <= max_iter <= 2 ** 31 - 1 \
            or not 0 <= seed <= 2 ** 31 - 1:
        raise ValueError('%s: M must be in 1..%d, nbits in 4..8, max_iter >= 1 and seed >= 0 (got %r)'
                         % (name, engine.PQ_M_MAX, value))
    return M, nbits, max_iter, seed


def _pq_report(knob, qf, gf, ids, path, keep=None):
    """GRL_EVAL_PQ: a product-quantised index of the query-prepended gallery ``gf`` (engine.pq_train + engine.pq_index, by
    cosine) -- the lines ``_report`` prints last: CMC / mAP under ADC next to the exact ones, recall@1 / 10 / 100 of
    engine.pq_search against engine.search under the same junk rule, the index bytes against the feature bytes -- and
    ``path + 'pq.json'`` (rank 0 alone writes; strict JSON).  A report only: the route's ranking is not touched."""
    import json
    M, nbits, max_iter, seed = knob
    q_pids, g_pids, q_camids, g_camids = ids
    book = engine.pq_train(gf, M, nbits, 'cosine', max_iter, seed)
    index = engine.pq_index(gf, book)
    cmc, mAP = engine.pq_metrics_streaming(qf, index, q_pids, g_pids, q_camids, g_camids)
    cmc_x, mAP_x = engine.rank_metrics_streaming(qf, gf, q_pids, g_pids, q_camids, g_camids)
    k = min(100, engine.SEARCH_K_MAX, int(gf.size(0)))
    approx = engine.pq_search(qf, index, k, exclude=ids)[1]
    exact = engine.search(qf, gf, k, exclude=ids)[1]
    ks = (1, 10, 100)
    recall = engine.topk_recall(approx, exact, ks)
    if keep is not None:                                   # (GRL_EVAL_IVF reports next to these)
        keep.update(k=k, exact=exact, recall=recall, index=index)
    feature_bytes = 4 * int(gf.size(0)) * int(gf.size(1))
    ranks = [r for r in (1, 5, 10, 20) if r <= len(cmc)]
    lines = ['PQ: M = {}, nbits = {} ({} bytes per row of {}), {} rows'.format(M, nbits, M, 4 * int(gf.size(1)), index.n),
             'ADC Mean AP: {:4.1%} (exact {:4.1%})'.format(mAP, mAP_x)]
    lines += ['ADC Rank-{:<3}: {:.1%} (exact {:.1%})'.format(r, cmc[r - 1], cmc_x[r - 1]) for r in ranks]
    lines += ['ADC recall@1: {:.2%}  @10: {:.2%}  @100: {:.2%}'.format(*recall),
              'Index: {} bytes against {} bytes of features ({:.1f}x smaller)'.format(
                  index.nbytes, feature_bytes, feature_bytes / float(index.nbytes))]
    if grl_dist._rank_world(None, None)[0] == 0:
        js = {'M': M, 'nbits': nbits, 'ksub': book.ksub, 'dsub': book.dsub, 'max_iter': max_iter, 'seed': seed,
              'metric': 'cosine', 'n': index.n, 'n_queries': int(qf.size(0)), 'n_iter': book.n_iter,
              'converged': book.converged, 'adc': {'mAP': float(mAP), 'cmc': [float(v) for v in cmc]},
              'exact': {'mAP': float(mAP_x), 'cmc': [float(v) for v in cmc_x]},
              'recall': {str(kk): (r if math.isfinite(r) else None) for kk, r in zip(ks, recall)},
              'index_bytes': int(index.nbytes), 'code_bytes': int(index.codes.numel()), 'feature_bytes': feature_bytes}
        with open((path or '') + 'pq.json', 'w') as fh:
            json.dump(js, fh, allow_nan=False)
    return lines


def parse_ivf_knob(name, value):
    """``GRL_EVAL_IVF``: unset or empty -> None (off); "nlist" or "nlist,nprobe" -> (nlist, nprobe) with integers nlist in
    1..65536 (the inverted lists; at most the gallery rows, which engine.ivf_train checks) and nprobe in 1..min(nlist, 1024)
    (default max(1, nlist // 8), capped at 1024).  Anything else is a ValueError that names the variable."""
    if value is None or not value.strip():
        return None
    parts = [p.strip() for p in value.split(',')]
    try:
        if len(parts) > 2:
            raise ValueError
        nlist = int(parts[0])
        nprobe = int(parts[1]) if len(parts) == 2 else min(max(1, nlist // 8), engine.IVF_NPROBE_MAX)
    except ValueError:
        raise ValueError('%s must be "nlist" or "nlist,nprobe" with integers (got %r)' % (name, value))
    if not 1 <= nlist <= engine.IVF_NLIST_MAX or not 1 <= nprobe <= min(nlist, engine.IVF_NPROBE_MAX):
        raise ValueError('%s: nlist must be in 1..%d and nprobe in 1..min(nlist, %d) (got %r)'
                         % (name, engine.IVF_NLIST_MAX, engine.IVF_NPROBE_MAX, value))
    return nlist, nprobe


def _ivf_report(knob, pq_knob, pq_kept, qf, gf, ids, path):
    """GRL_EVAL_IVF: an IVF-PQ index of the query-prepended gallery ``gf`` (engine.ivf_train + engine.ivf_index, by cosine,
    with GRL_EVAL_PQ's M, nbits, max_iter and seed) -- the lines printed after GRL_EVAL_PQ's: the lists, the mean scanned
    fraction, recall@1 / 10 / 100 of engine.ivf_search against engine.search under the same junk rule next to
    engine.pq_search's, the index bytes -- and ``path + 'ivf.json'`` (rank 0 alone writes; strict JSON).  A report only."""
    import json
    nlist, nprobe = knob
    M, nbits, max_iter, seed = pq_knob
    book = engine.ivf_train(gf, nlist, M, nbits, 'cosine', max_iter, seed)
    index = engine.ivf_index(gf, book)
    k, ks = pq_kept['k'], (1, 10, 100)
    approx = engine.ivf_search(qf, index, k, nprobe, exclude=ids)[1]
    recall = engine.topk_recall(approx, pq_kept['exact'], ks)
    pq_kept.update(ivf_index=index, ivf_nprobe=nprobe, ivf_recall=recall)      # (GRL_EVAL_REFINE reports next to these)
    nq = int(qf.size(0))
    scanned = float(engine.ivf_probe_stats(qf, index, nprobe).sum()) / max(nq * index.n, 1)
    mean_len = index.n / float(nlist)
    feature_bytes = 4 * int(gf.size(0)) * int(gf.size(1))
    lines = ['IVF: nlist = {}, nprobe = {}, list length min / mean / max = {} / {:.1f} / {}'.format(
                 nlist, nprobe, index.list_len_min, mean_len, index.list_len_max),
             'IVF scanned fraction: {:.2%}'.format(scanned),
             'IVF recall@1: {:.2%}  @10: {:.2%}  @100: {:.2%}  (PQ {:.2%}  {:.2%}  {:.2%})'.format(
                 *(tuple(recall) + tuple(pq_kept['recall']))),
             'IVF index: {} bytes against {} bytes of features ({:.1f}x smaller)'.format(
                 index.nbytes, feature_bytes, feature_bytes / float(index.nbytes))]
    if grl_dist._rank_world(None, None)[0] == 0:
        def fin(v):
            return v if math.isfinite(v) else None
        js = {'nlist': nlist, 'nprobe': nprobe, 'M': M, 'nbits': nbits, 'max_iter': max_iter, 'seed': seed, 'metric': 'cosine',
              'n': index.n, 'n_queries': nq, 'list_len': {'min': index.list_len_min, 'mean': mean_len, 'max': index.list_len_max},
              'scanned_fraction': scanned, 'coarse_n_iter': book.coarse_n_iter, 'coarse_converged': book.coarse_converged,
              'recall': {str(kk): fin(r) for kk, r in zip(ks, recall)},
              'pq_recall': {str(kk): fin(r) for kk, r in zip(ks, pq_kept['recall'])},
              'index_bytes': int(index.nbytes), 'feature_bytes': feature_bytes}
        with open((path or '') + 'ivf.json', 'w') as fh:
            json.dump(js, fh, allow_nan=False)
    return lines


def parse_refine_knob(name, value):
    """``GRL_EVAL_REFINE``: unset or empty -> None (off); "R", "R,bf16" or "R,f32" -> (R, dtype) with an integer R in
    1..1024 (the shortlist taken from the codes and re-sorted by exact distances, engine.refine_search) and the type of
    the feature store (default 'f32').  Anything else is a ValueError that names the variable."""
    if value is None or not value.strip():
        return None
    parts = [p.strip() for p in value.split(',')]
    try:
        if len(parts) > 2:
            raise ValueError
        R = int(parts[0])
        dtype = parts[1] if len(parts) == 2 else 'f32'
        if dtype not in ('f32', 'bf16'):
            raise ValueError
    except ValueError:
        raise ValueError('%s must be "R", "R,bf16" or "R,f32" with an integer R (got %r)' % (name, value))
    if not 1 <= R <= engine.SEARCH_K_MAX:
        raise ValueError('%s: R must be in 1..%d (got %r)' % (name, engine.SEARCH_K_MAX, value))
    return R, dtype


def _refine_report(knob, kept, qf, gf, ids, path):
    """GRL_EVAL_REFINE: a feature store of the query-prepended gallery ``gf`` (engine.RefineStore) and the two-stage search
    engine.refine_search over GRL_EVAL_PQ's index and, when GRL_EVAL_IVF is set, over its index -- the lines printed after
    theirs: the store bytes, recall@1 / 10 / 100 of the refined lists against engine.search under the same junk rule next
    to the unrefined figures -- and ``path + 'refine.json'`` (rank 0 alone writes; strict JSON).  A report only."""
    import json
    R, dtype = knob
    store = engine.RefineStore(gf.contiguous(), dtype)
    ks = (1, 10, 100)
    k = min(kept['k'], R)
    feature_bytes = 4 * int(gf.size(0)) * int(gf.size(1))
    lines = ['Refine: R = {}, k = {}, {} store of {} bytes against {} bytes of features'.format(
        R, k, dtype, store.nbytes, feature_bytes)]

    def fin(v):
        return v if math.isfinite(v) else None
    js = {'R': R, 'k': k, 'store': dtype, 'store_bytes': int(store.nbytes), 'feature_bytes': feature_bytes, 'metric': 'cosine',
          'n': store.n, 'n_queries': int(qf.size(0))}
    pq_recall = engine.topk_recall(engine.refine_search(qf, kept['index'], store, k, R, exclude=ids)[1], kept['exact'], ks)
    lines.append('Refined PQ recall@1: {:.2%}  @10: {:.2%}  @100: {:.2%}  (ADC {:.2%}  {:.2%}  {:.2%})'.format(
        *(tuple(pq_recall) + tuple(kept['recall']))))
    js['pq'] = {'refined_recall': {str(kk): fin(r) for kk, r in zip(ks, pq_recall)},
                'recall': {str(kk): fin(r) for kk, r in zip(ks, kept['recall'])}}
    if 'ivf_index' in kept:
        recall = engine.topk_recall(engine.refine_search(qf, kept['ivf_index'], store, k, R, nprobe=kept['ivf_nprobe'],
                                                         exclude=ids)[1], kept['exact'], ks)
        lines.append('Refined IVF recall@1: {:.2%}  @10: {:.2%}  @100: {:.2%}  (IVF {:.2%}  {:.2%}  {:.2%})'.format(
            *(tuple(recall) + tuple(kept['ivf_recall']))))
        js['ivf'] = {'nprobe': kept['ivf_nprobe'], 'refined_recall': {str(kk): fin(r) for kk, r in zip(ks, recall)},
                     'recall': {str(kk): fin(r) for kk, r in zip(ks, kept['ivf_recall'])}}
    if grl_dist._rank_world(None, None)[0] == 0:
        with open((path or '') + 'refine.json', 'w') as fh:
            json.dump(js, fh, allow_nan=False)
    return lines


def parse_nng_knob(name, value):
    """``GRL_EVAL_NNG``: unset or empty -> None (off); "K,D", "K,D,L", "K,D,L,w", "K,D,L,w,T" or "K,D,L,w,T,bf16" (or
    ",f32") -> (K, D, L, w, T, dtype): the exact candidate lists per row (K in 2..128), the degree of the optimised graph (D
    even in 2..min(K, 64)), the itopk size (L a power of two in 8..512, default 64), the parents per iteration (w in 1..8
    with w * D <= 256, default 1), the iteration cap (T >= 1, default 64) and the type of the feature store (default
    'f32') of engine.nng_build / engine.nng_search.  Anything else is a ValueError that names the variable."""
    if value is None or not value.strip():
        return None
    parts = [p.strip() for p in value.split(',')]
    try:
        if not 2 <= len(parts) <= 6:
            raise ValueError
        K, D = int(parts[0]), int(parts[1])
        L = int(parts[2]) if len(parts) >= 3 else 64
        w = int(parts[3]) if len(parts) >= 4 else 1
        T = int(parts[4]) if len(parts) >= 5 else 64
        dtype = parts[5] if len(parts) == 6 else 'f32'
        if dtype not in ('f32', 'bf16'):
            raise ValueError
    except ValueError:
        raise ValueError('%s must be "K,D", "K,D,L", "K,D,L,w", "K,D,L,w,T" or "K,D,L,w,T,bf16" with integers (got %r)'
                         % (name, value))
    if not 2 <= K <= engine.NNG_K_MAX or D % 2 or not 2 <= D <= min(K, engine.NNG_D_MAX) \
            or not engine.NNG_L_MIN <= L <= engine.NNG_L_MAX or L & (L - 1) or not 1 <= w <= engine.NNG_W_MAX \
            or w * D > engine.NNG_WD_MAX or not 1 <= T <= 2 ** 31 - 1:
        raise ValueError('%s: K must be in 2..%d, D even in 2..min(K, %d), L a power of two in %d..%d, w in 1..%d with '
                         'w * D <= %d and T >= 1 (got %r)' % (name, engine.NNG_K_MAX, engine.NNG_D_MAX, engine.NNG_L_MIN,
                                                              engine.NNG_L_MAX, engine.NNG_W_MAX, engine.NNG_WD_MAX, value))
    return K, D, L, w, T, dtype


def _nng_report(knob, qf, gf, ids, path):
    """GRL_EVAL_NNG: a kNN-graph index of the query-prepended gallery ``gf`` (engine.nng_build on the exact lists, by
    cosine) -- the lines printed last: the graph, recall@1 / 10 / 100 of engine.nng_search against engine.search under the
    same junk rule, the mean rows visited per query, the index bytes -- and ``path + 'nng.json'`` (rank 0 alone writes;
    strict JSON).  A report only: the route's ranking is not touched."""
    import json
    K, D, L, w, T, dtype = knob
    n = int(gf.size(0))
    index = engine.nng_build(gf.contiguous(), K, D, 'cosine', dtype)
    k = min(100, L, n)
    approx, stats = engine.nng_search(qf, index, k, L, w, T, exclude=ids, return_stats=True)[1:]
    exact = engine.search(qf, gf, k, exclude=ids)[1]
    ks = (1, 10, 100)
    recall = engine.topk_recall(approx, exact, ks)
    nq = int(qf.size(0))
    visited = float(stats[:, 0].sum()) / max(nq, 1)
    iters = float(stats[:, 1].sum()) / max(nq, 1)
    feature_bytes = 4 * n * int(gf.size(1))
    lines = ['NNG: K = {}, D = {}, L = {}, w = {}, T = {}, {} store, {} rows'.format(K, index.D, L, w, T, dtype, index.n),
             'NNG recall@1: {:.2%}  @10: {:.2%}  @100: {:.2%}  (k = {})'.format(*(tuple(recall) + (k,))),
             'NNG visited rows per query: {:.1f} of {} ({:.2%}), {:.1f} iterations'.format(
                 visited, n, visited / max(n, 1), iters),
             'NNG index: {} bytes against {} bytes of features'.format(index.nbytes, feature_bytes)]
    if grl_dist._rank_world(None, None)[0] == 0:
        js = {'K': K, 'D': index.D, 'L': L, 'w': w, 'T': T, 'store': dtype, 'metric': 'cosine', 'n': index.n, 'n_queries': nq,
              'k': k, 'recall': {str(kk): (r if math.isfinite(r) else None) for kk, r in zip(ks, recall)},
              'visited_mean': visited, 'iterations_mean': iters, 'index_bytes': int(index.nbytes),
              'feature_bytes': feature_bytes}
        with open((path or '') + 'nng.json', 'w') as fh:
            json.dump(js, fh, allow_nan=False)
    return lines


def parse_bin_knob(name, value):
    """``GRL_EVAL_BIN``: unset or empty -> None (off); "nbits", "nbits,method", "nbits,method,n_iter" or
    "nbits,method,n_iter,seed" -> (nbits, method, n_iter, seed) with nbits a multiple of 32 in 32..1024 (the bits of a code
    row), method 'itq' or 'lsh' (default 'itq'), n_iter >= 1 (the ITQ rounds, default 50) and seed >= 0 (default 0) of
    engine.bin_train.  Anything else is a ValueError that names the variable."""
    if value is None or not value.strip():
        return None
    parts = [p.strip() for p in value.split(',')]
    try:
        if len(parts) > 4:
            raise ValueError
        nbits = int(parts[0])
        method = parts[1] if len(parts) >= 2 else 'itq'
        n_iter = int(parts[2]) if len(parts) >= 3 else 50
        seed = int(parts[3]) if len(parts) == 4 else 0
        if method not in engine.BIN_METHODS:
            raise ValueError
    except ValueError:
        raise ValueError('%s must be "nbits", "nbits,itq", "nbits,lsh", "nbits,method,n_iter" or "nbits,method,n_iter,seed" '
                         'with integers (got %r)' % (name, value))
    if nbits % 32 or not 32 <= nbits <= engine.BIN_NBITS_MAX or not 1 <= n_iter <= 2 ** 31 - 1 \
            or not 0 <= seed <= 2 ** 31 - 1:
        raise ValueError('%s: nbits must be a multiple of 32 in 32..%d, n_iter >= 1 and seed >= 0 (got %r)'
                         % (name, engine.BIN_NBITS_MAX, value))
    return nbits, method, n_iter, seed


def _bin_report(knob, qf, gf, ids, path):
    """GRL_EVAL_BIN: a binary-code index of the query-prepended gallery ``gf`` (engine.bin_train + engine.bin_index) -- the
    lines printed last: CMC / mAP by the Hamming and by the asymmetric distance next to the exact ones, recall@1 / 10 / 100
    of engine.bin_search in both modes against engine.search under the same junk rule, the index bytes against the feature
    bytes -- and ``path + 'bin.json'`` (rank 0 alone writes; strict JSON).  A report only: the route's ranking is not
    touched."""
    import json
    nbits, method, n_iter, seed = knob
    q_pids, g_pids, q_camids, g_camids = ids
    book = engine.bin_train(gf, nbits, method, n_iter, seed)
    index = engine.bin_index(gf, book)
    cmc_x, mAP_x = engine.rank_metrics_streaming(qf, gf, q_pids, g_pids, q_camids, g_camids)
    k = min(100, engine.SEARCH_K_MAX, int(gf.size(0)))
    exact = engine.search(qf, gf, k, exclude=ids)[1]
    ks = (1, 10, 100)
    feature_bytes = 4 * int(gf.size(0)) * int(gf.size(1))
    ranks = [r for r in (1, 5, 10, 20) if r <= len(cmc_x)]
    lines = ['BIN: {} bits by {} ({} bytes per row of {}), {} rows'.format(nbits, method, nbits // 8, 4 * int(gf.size(1)),
                                                                          index.n)]
    fin = lambda r: r if math.isfinite(r) else None
    js = {'nbits': nbits, 'method': method, 'n_iter': n_iter, 'seed': seed, 'n': index.n, 'n_queries': int(qf.size(0)), 'k': k,
          'objective': book.objective, 'exact': {'mAP': float(mAP_x), 'cmc': [float(v) for v in cmc_x]},
          'index_bytes': int(index.nbytes), 'code_bytes': int(index.codes.numel()), 'feature_bytes': feature_bytes}
    for mode, tag in (('hamming', 'Hamming'), ('asymmetric', 'Asymmetric')):
        cmc, mAP = engine.bin_metrics_streaming(qf, index, q_pids, g_pids, q_camids, g_camids, mode=mode)
        recall = engine.topk_recall(engine.bin_search(qf, index, k, mode, exclude=ids)[1], exact, ks)
        lines += ['{} Mean AP: {:4.1%} (exact {:4.1%})'.format(tag, mAP, mAP_x)]
        lines += ['{} Rank-{:<3}: {:.1%} (exact {:.1%})'.format(tag, r, cmc[r - 1], cmc_x[r - 1]) for r in ranks]
        lines += ['{} recall@1: {:.2%}  @10: {:.2%}  @100: {:.2%}'.format(tag, *recall)]
        js[mode] = {'mAP': float(mAP), 'cmc': [float(v) for v in cmc], 'recall': {str(kk): fin(r) for kk, r in zip(ks, recall)}}
    lines += ['BIN index: {} bytes against {} bytes of features ({:.1f}x smaller)'.format(
        index.nbytes, feature_bytes, feature_bytes / float(index.nbytes))]
    if grl_dist._rank_world(None, None)[0] == 0:
        with open((path or '') + 'bin.json', 'w') as fh:
            json.dump(js, fh, allow_nan=False)
    return lines


def parse_sq8_knob(name, value):
    """``GRL_EVAL_SQ8``: unset or empty -> None (off); "1" -> (None, None): the int8 scalar-quantised index of
    engine.sq8_train / sq8_search; "1,R", "1,R,f32" or "1,R,bf16" -> (R, dtype): also the two-stage search
    engine.sq8_refine_search with a shortlist of R in 1..1024 rows from an engine.RefineStore of that type (default 'f32').
    Anything else is a ValueError that names the variable."""
    if value is None or not value.strip():
        return None
    parts = [p.strip() for p in value.split(',')]
    try:
        if len(parts) > 3 or parts[0] != '1':
            raise ValueError
        R = int(parts[1]) if len(parts) >= 2 else None
        dtype = parts[2] if len(parts) == 3 else ('f32' if R is not None else None)
        if dtype not in (None, 'f32', 'bf16'):
            raise ValueError
    except ValueError:
        raise ValueError('%s must be "1", "1,R", "1,R,f32" or "1,R,bf16" with an integer R (got %r)' % (name, value))
    if R is not None and not 1 <= R <= engine.SEARCH_K_MAX:
        raise ValueError('%s: R must be in 1..%d (got %r)' % (name, engine.SEARCH_K_MAX, value))
    return R, dtype


def _sq8_report(knob, qf, gf, ids, path):
    """GRL_EVAL_SQ8: an int8 scalar-quantised index of the query-prepended gallery ``gf`` by cosine (engine.sq8_train +
    engine.sq8_index) -- the lines printed last: CMC / mAP of the sq8 ranking next to the exact ones, recall@1 / 10 / 100 of
    engine.sq8_search against engine.search under the same junk rule, with R the same for engine.sq8_refine_search, the
    index bytes against the feature bytes -- and ``path + 'sq8.json'`` (rank 0 alone writes; strict JSON).  A report only:
    the route's ranking is not touched."""
    import json
    R, dtype = knob
    q_pids, g_pids, q_camids, g_camids = ids
    gf = gf.contiguous()
    index = engine.sq8_index(gf, engine.sq8_train(gf, 'cosine'))
    cmc_x, mAP_x = engine.rank_metrics_streaming(qf, gf, q_pids, g_pids, q_camids, g_camids)
    k = min(100, engine.SEARCH_K_MAX, int(gf.size(0)))
    exact = engine.search(qf, gf, k, exclude=ids)[1]
    ks = (1, 10, 100)
    feature_bytes = 4 * int(gf.size(0)) * int(gf.size(1))
    ranks = [r for r in (1, 5, 10, 20) if r <= len(cmc_x)]
    fin = lambda r: r if math.isfinite(r) else None
    cmc, mAP = engine.sq8_metrics_streaming(qf, index, q_pids, g_pids, q_camids, g_camids)
    recall = engine.topk_recall(engine.sq8_search(qf, index, k, exclude=ids)[1], exact, ks)
    lines = ['SQ8: {} bytes per row of {}, {} rows'.format(index.codebook.dpad, 4 * int(gf.size(1)), index.n)]
    lines += ['SQ8 Mean AP: {:4.1%} (exact {:4.1%})'.format(mAP, mAP_x)]
    lines += ['SQ8 Rank-{:<3}: {:.1%} (exact {:.1%})'.format(r, cmc[r - 1], cmc_x[r - 1]) for r in ranks]
    lines += ['SQ8 recall@1: {:.2%}  @10: {:.2%}  @100: {:.2%}'.format(*recall)]
    js = {'n': index.n, 'd': index.d, 'dpad': index.codebook.dpad, 'n_queries': int(qf.size(0)), 'k': k, 'metric': 'cosine',
          'exact': {'mAP': float(mAP_x), 'cmc': [float(v) for v in cmc_x]},
          'sq8': {'mAP': float(mAP), 'cmc': [float(v) for v in cmc], 'recall': {str(kk): fin(r) for kk, r in zip(ks, recall)}},
          'index_bytes': int(index.nbytes), 'code_bytes': int(index.codes.numel()), 'feature_bytes': feature_bytes}
    if R is not None:
        store = engine.RefineStore(gf, dtype)
        kr = min(k, R)
        refined = engine.topk_recall(engine.sq8_refine_search(qf, index, store, kr, R, exclude=ids)[1], exact, ks)
        lines += ['SQ8 refined recall@1: {:.2%}  @10: {:.2%}  @100: {:.2%}  (R = {}, k = {}, {} store of {} bytes)'.format(
            *(tuple(refined) + (R, kr, dtype, store.nbytes)))]
        js['refine'] = {'R': R, 'k': kr, 'store': dtype, 'store_bytes': int(store.nbytes),
                        'recall': {str(kk): fin(r) for kk, r in zip(ks, refined)}}
    lines += ['SQ8 index: {} bytes against {} bytes of features ({:.1f}x smaller)'.format(
        index.nbytes, feature_bytes, feature_bytes / float(index.nbytes))]
    if grl_dist._rank_world(None, None)[0] == 0:
        with open((path or '') + 'sq8.json', 'w') as fh:
            json.dump(js, fh, allow_nan=False)
    return lines


class ATTEvaluator(object):
    def __init__(self, cnn_model, Siamese_model, only_eval):
        self.cnn_model = cnn_model
        self.siamese_model = Siamese_model
        self.only_eval = only_eval
        # clips per forward in dense mode.  The reference uses 8 (attevaluator.py:72-76) to fit
        # its GPU; clip features are independent (eval BN is folded), so any chunking gives the
        # same rows -- 32 keeps the MI355X busy (1900 vs 1400 clip-features/s at 8).
        self.chunk = 32
        # dense mode: tracklets are collected until this many clips are pending, then extracted together in
        # `chunk`-sized forwards -- a MARS tracklet has ~15 clips, one forward per tracklet would leave every
        # forward half empty.  Rows do not depend on what else is in the batch (tested), so the per-tracklet means
        # are the ones a tracklet-by-tracklet run gives, bit for bit.
        self.group = 128

    def _device(self):
        return next(self.cnn_model.parameters()).device

    def extract_feature(self, data_loader):
        return self._extract(data_loader, False)[:3]

    def extract_clip_features(self, data_loader):
        """Dense mode (only_eval=True) without the clip average: ``(engine.TrackletSet, pids, camids)`` -- the clip rows
        ``extract_feature`` averages, one tracklet per item of the loader in its order, and the ids that method returns.
        Under torch.distributed the clip rows travel as the mean rows do (grl_dist.gather_feature_batches), the clip
        counts in the place of the pids of that call."""
        if not self.only_eval:
            raise ValueError('extract_clip_features needs only_eval=True: rrs mode has one clip per tracklet')
        _, pids, camids, tset = self._extract(data_loader, True)
        return tset, pids, camids

    @torch.no_grad()
    def _extract(self, data_loader, want_clips):
        """(mean-row features, pids, camids, TrackletSet or None) -- the first three are ``extract_feature``'s, made by
        the same calls whether the clip rows are kept (``want_clips``, dense mode) or not."""
        self.cnn_model.eval()
        self.siamese_model.eval()
        dev = self._device()
        rank, world = grl_dist._rank_world(None, None)
        # data parallel (one process per GPU): batch i is extracted by rank i % world -- clips are
        # independent, there is no collective on the data path -- and the rows are all-gathered once
        # (sharded at the batch SAMPLER: a rank's loader workers decode only its own clips)
        own = [i for i in range(len(data_loader)) if i % world == rank]
        batches = grl_dist.shard_loader_batches(data_loader, rank, world)
        mine = []
        mine_clips = []                     # want_clips: (batch index, clip rows [n, D], [n], [])
        pending, n_pending = [], 0          # dense mode: (batch index, clips [n,s,c,h,w], pids, camids)

        def flush():
            clips = torch.cat([p[1] for p in pending], 0) if len(pending) > 1 else pending[0][1]
            rows = torch.cat([engine.extract_features(self.cnn_model, self.siamese_model, clips[y:y + self.chunk])
                              for y in range(0, clips.size(0), self.chunk)], 0)
            off = 0
            for i, c, pids, camids in pending:
                mine.append((i, engine.rows_mean(rows[off:off + c.size(0)]), pids, camids))
                if want_clips:
                    mine_clips.append((i, rows[off:off + c.size(0)], [int(c.size(0))], []))
                off += c.size(0)
            del pending[:]
        # the next batch's host->device copy overlaps this batch's kernels (side HIP stream)
        for i, (imgs, pids, camids) in zip(own, engine.DevicePrefetcher(batches, dev)):
            pids, camids = [int(x) for x in pids], [int(x) for x in camids]
            if self.only_eval:
                # dense mode: one tracklet per item, all its clips; features are averaged
                # over clips (attevaluator.py:68-98)
                b, n, s, c, h, w = imgs.size()
                pending.append((i, imgs.view(b * n, s, c, h, w), pids, camids))
                n_pending += b * n
                if n_pending >= self.group:
                    flush()
                    n_pending = 0
            else:
                mine.append((i, engine.extract_features(self.cnn_model, self.siamese_model, imgs), pids, camids))
        if pending:
            flush()
        feat, pids_all, cams_all = grl_dist.gather_feature_batches(mine, len(data_loader))
        pids_all, cams_all = np.asarray(pids_all), np.asarray(cams_all)
        tset = None
        if want_clips:
            rows, counts, _ = grl_dist.gather_feature_batches(mine_clips, len(data_loader))
            tset = engine.TrackletSet(rows, counts)
        return feat, pids_all, cams_all, tset

    def _visualize(self, query, gallery, qf, gf, q_pids, q_camids, g_pids, g_camids, path, rerank, topk=10,
                   metric='cosine', diffusion=None, setdist=None):
        """``visual=1``: the ranked-results folders of visualize_ranked_results in ``path + 'visual'`` for the query
        positions of GRL_VISUAL_QUERIES (comma list; default 4, the reference's visual_id), and ``ranked.json`` in
        the same folder: {query position: [[gallery position, pid, camid, distance], ...]} (a non-finite distance is
        null; a position the query list does not have is skipped with a printed note).  ``gf`` / ``g_pids`` /
        ``g_camids`` carry the prepended queries, so gallery positions below nq are queries.  The lists are the
        junk-filtered top-k of engine.search / engine.rerank_search (``exclude=``): no matrix, no argsort.  Those
        calls are collective under torch.distributed; rank 0 alone writes.  ``metric``: engine.search's (the
        distances of ranked.json are that metric's).  ``diffusion`` = (graph, kq, alpha, n_iter): the lists are
        engine.diffusion_search's and the distances of ranked.json its scores -f.  ``setdist`` = (qset, gset, reduce,
        metric): the lists are engine.set_search's over the tracklets' clip sets and the distances of ranked.json the set
        distances."""
        import json
        if query is None or gallery is None:
            raise ValueError('visual=1 needs the query and gallery tuple lists (img_path(s), pid, camid)')
        nq = qf.size(0)
        if len(query) != nq or len(query) + len(gallery) != gf.size(0):
            raise ValueError('visual=1: %d query / %d gallery tuples for %d / %d feature rows'
                             % (len(query), len(gallery), nq, gf.size(0) - nq))
        spec = os.environ.get('GRL_VISUAL_QUERIES', '4')
        try:
            asked = sorted(set(int(v) for v in spec.split(',') if v.strip()))
        except ValueError:
            raise ValueError('GRL_VISUAL_QUERIES must be a comma list of query positions (got %r)' % spec)
        wanted = [q for q in asked if 0 <= q < nq]
        ids = (q_pids, g_pids, q_camids, g_camids)
        if setdist is not None:
            dist, idx = engine.set_search(setdist[0], setdist[1], topk, reduce=setdist[2], metric=setdist[3], exclude=ids)
        elif diffusion is not None:
            graph, kq, alpha, n_iter = diffusion
            dist, idx = engine.diffusion_search(qf, gf, topk, graph=graph, kq=kq, alpha=alpha, n_iter=n_iter, exclude=ids)
        elif rerank:
            dist, idx = engine.rerank_search(qf, gf, topk, exclude=ids)
        else:
            dist, idx = engine.search(qf, gf, topk, metric=metric, exclude=ids)
        if grl_dist._rank_world(None, None)[0] != 0:
            return
        dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
        if len(wanted) < len(asked):
            print('GRL_VISUAL_QUERIES: no query at position(s) %s (there are %d queries), skipped'
                  % (', '.join(str(q) for q in asked if q not in wanted), nq))
        save_dir = path + 'visual'
        visualize_ranked_results(None, list(query), list(query) + list(gallery), save_dir, visual_id=wanted,
                                 topk=topk, indices=idx)
        ranked = {}
        for q in wanted:                      # strict JSON: a distance that is not finite (NaN feature) becomes null
            ranked[str(q)] = [[int(g), int(g_pids[g]), int(g_camids[g]), float(d) if np.isfinite(d) else None]
                              for g, d in zip(idx[q], dist[q]) if g >= 0]
        with open(os.path.join(save_dir, 'ranked.json'), 'w') as fh:
            json.dump(ranked, fh, indent=1, allow_nan=False)

    def evaluate(self, query, gallery, query_loader, gallery_loader, path, visual, rerank):
        stream = os.environ.get('GRL_EVAL_STREAM') == '1'
        rerank_stream = rerank and os.environ.get('GRL_EVAL_RERANK') == 'stream'
        if stream and rerank and not rerank_stream:
            raise ValueError('GRL_EVAL_STREAM=1 cannot re-rank: k-reciprocal re-ranking needs the full query/gallery '
                             'distance matrices, which the streaming evaluator never builds (unset GRL_EVAL_STREAM)')
        knob = parse_metric_knob('GRL_EVAL_METRIC', os.environ.get('GRL_EVAL_METRIC'))
        if knob is not None and rerank:
            raise ValueError('GRL_EVAL_METRIC=%s cannot re-rank: k-reciprocal re-ranking is defined on Euclidean and '
                             'cosine distance matrices, and the verification head\'s distance is a signed logit '
                             '(unset GRL_EVAL_METRIC or evaluate with rerank=0)' % os.environ['GRL_EVAL_METRIC'].strip())
        dba = parse_expand_knob('GRL_EVAL_DBA', os.environ.get('GRL_EVAL_DBA'))
        qe = parse_expand_knob('GRL_EVAL_QE', os.environ.get('GRL_EVAL_QE'))
        # pair-level metrics, off by default: ROC AUC / EER / TPR@FPR of the distances the route ranks by
        # (engine.pair_roc and its forms), printed after the CMC and stored in path + 'roc.json'
        roc_bits = parse_roc_knob('GRL_EVAL_ROC', os.environ.get('GRL_EVAL_ROC'))
        # identity discovery, off by default: DBSCAN of the query-prepended gallery by cosine (engine.cluster), printed
        # after any ROC lines and stored in path + 'clusters.json'
        cluster_knob = parse_cluster_knob('GRL_EVAL_CLUSTER', os.environ.get('GRL_EVAL_CLUSTER'))
        if cluster_knob is not None and knob is not None:
            raise ValueError('GRL_EVAL_CLUSTER cannot be combined with GRL_EVAL_METRIC=%s: the verification head\'s '
                             'distance is a signed logit of modified query rows against gallery rows, not a distance '
                             'between two samples of one set (unset one of them)'
                             % os.environ['GRL_EVAL_METRIC'].strip())
        # the same on the k-reciprocal Jaccard distance, off by default (engine.cluster_jaccard), printed after
        # GRL_EVAL_CLUSTER's lines and stored in path + 'cluster_jaccard.json'
        jaccard_knob = parse_cluster_jaccard_knob('GRL_EVAL_CLUSTER_JACCARD', os.environ.get('GRL_EVAL_CLUSTER_JACCARD'))
        if jaccard_knob is not None and knob is not None:
            raise ValueError('GRL_EVAL_CLUSTER_JACCARD cannot be combined with GRL_EVAL_METRIC=%s: the verification '
                             'head\'s distance is a signed logit of modified query rows against gallery rows, not a '
                             'distance between two samples of one set (unset one of them)'
                             % os.environ['GRL_EVAL_METRIC'].strip())
        # k-means with a known or budgeted number of identities, off by default: spherical k-means of the query-prepended
        # gallery (engine.kmeans), printed last and stored in path + 'kmeans.json'
        kmeans_knob = parse_kmeans_knob('GRL_EVAL_KMEANS', os.environ.get('GRL_EVAL_KMEANS'))
        if kmeans_knob is not None and knob is not None:
            raise ValueError('GRL_EVAL_KMEANS cannot be combined with GRL_EVAL_METRIC=%s: k-means runs by cosine on '
                             'the routes that rank by cosine (unset one of them)'
                             % os.environ['GRL_EVAL_METRIC'].strip())
        # density clustering without an eps, off by default: HDBSCAN of the query-prepended gallery by cosine
        # (engine.hdbscan), printed after the k-means lines and stored in path + 'hdbscan.json'
        hdbscan_knob = parse_hdbscan_knob('GRL_EVAL_HDBSCAN', os.environ.get('GRL_EVAL_HDBSCAN'))
        if hdbscan_knob is not None and knob is not None:
            raise ValueError('GRL_EVAL_HDBSCAN cannot be combined with GRL_EVAL_METRIC=%s: HDBSCAN runs by cosine on '
                             'the routes that rank by cosine (unset one of them)'
                             % os.environ['GRL_EVAL_METRIC'].strip())
        # the 2-d map of the feature space, off by default: t-SNE of the query-prepended gallery by cosine (engine.tsne),
        # printed after the HDBSCAN lines and stored in path + 'tsne.json' (and 'tsne.png' when matplotlib imports)
        tsne_knob = parse_tsne_knob('GRL_EVAL_TSNE', os.environ.get('GRL_EVAL_TSNE'))
        if tsne_knob is not None and knob is not None:
            raise ValueError('GRL_EVAL_TSNE cannot be combined with GRL_EVAL_METRIC=%s: t-SNE runs by cosine on '
                             'the routes that rank by cosine (unset one of them)'
                             % os.environ['GRL_EVAL_METRIC'].strip())
        # the label-free score of those clusterings, off by default (engine.silhouette): a third line of each report and
        # a "silhouette" entry of its JSON file
        sil_knob = parse_silhouette_knob('GRL_EVAL_SILHOUETTE', os.environ.get('GRL_EVAL_SILHOUETTE'))
        if sil_knob is not None and cluster_knob is None and jaccard_knob is None and kmeans_knob is None \
                and hdbscan_knob is None:
            raise ValueError('GRL_EVAL_SILHOUETTE scores the labels of GRL_EVAL_CLUSTER, GRL_EVAL_CLUSTER_JACCARD, '
                             'GRL_EVAL_KMEANS or GRL_EVAL_HDBSCAN: set one of them too (or unset GRL_EVAL_SILHOUETTE)')
        # PCA / PCA-whitening of the features, off by default (engine.pca): fitted on the query-prepended gallery and
        # applied to both before DBA and QE; everything below runs on the r-column tensors unchanged
        pca_knob = parse_pca_knob('GRL_EVAL_PCA', os.environ.get('GRL_EVAL_PCA'))
        if pca_knob is not None and knob is not None:
            raise ValueError('GRL_EVAL_PCA cannot be combined with GRL_EVAL_METRIC=%s: the verification head reads '
                             'fixed slices of the raw feature rows, which a change of basis does not keep (unset one '
                             'of them)' % os.environ['GRL_EVAL_METRIC'].strip())
        # diffusion re-ranking on the gallery's mutual-kNN graph, off by default (engine.diffusion_search): replaces the
        # plain cosine ranking after PCA / DBA / QE, with GRL_EVAL_STREAM set or not (it never builds the matrix)
        diffusion_knob = parse_diffusion_knob('GRL_EVAL_DIFFUSION', os.environ.get('GRL_EVAL_DIFFUSION'))
        if diffusion_knob is not None and rerank:
            raise ValueError('GRL_EVAL_DIFFUSION cannot re-rank: k-reciprocal re-ranking works on distance matrices, and '
                             'the diffusion scores are the solution of a linear system on the gallery graph, not a '
                             'distance (unset GRL_EVAL_DIFFUSION or evaluate with rerank=0)')
        if diffusion_knob is not None and knob is not None:
            raise ValueError('GRL_EVAL_DIFFUSION cannot be combined with GRL_EVAL_METRIC=%s: the graph\'s edge weights are '
                             'powers of the cosine similarity between two samples of one set, and the verification '
                             'head\'s distance is a signed logit of modified query rows against gallery rows (unset one '
                             'of them)' % os.environ['GRL_EVAL_METRIC'].strip())
        if diffusion_knob is not None and roc_bits:
            raise ValueError('GRL_EVAL_DIFFUSION cannot be combined with GRL_EVAL_ROC: the pair-level figures are taken '
                             'from distance blocks, and the diffusion scores exist per block of queries only (unset one '
                             'of them)')
        # tracklet set distances over the clips of dense mode, off by default (engine.set_metrics_streaming): the ranking,
        # --visual and GRL_EVAL_ROC work on a set-to-set distance between the tracklets' clip sets instead of the
        # distance of their mean rows; the clustering knobs keep running on the mean rows
        set_knob = parse_set_knob('GRL_EVAL_SET', os.environ.get('GRL_EVAL_SET'))
        # a product-quantised index of the gallery, off by default (engine.pq_train / pq_search): a report next to the
        # exact figures of the routes that rank by cosine, after PCA / DBA / QE; the route's ranking is not replaced
        pq_knob = parse_pq_knob('GRL_EVAL_PQ', os.environ.get('GRL_EVAL_PQ'))
        # inverted lists over residual codes on top of it, off by default (engine.ivf_train / ivf_search): one more report
        ivf_knob = parse_ivf_knob('GRL_EVAL_IVF', os.environ.get('GRL_EVAL_IVF'))
        if ivf_knob is not None and pq_knob is None:
            raise ValueError('GRL_EVAL_IVF=%s needs GRL_EVAL_PQ: the index encodes its residuals with GRL_EVAL_PQ\'s M, nbits, '
                             'max_iter and seed (set GRL_EVAL_PQ too)' % os.environ['GRL_EVAL_IVF'].strip())
        # exact refinement of the indexes' shortlists from a feature store, off by default (engine.refine_search): one more report
        refine_knob = parse_refine_knob('GRL_EVAL_REFINE', os.environ.get('GRL_EVAL_REFINE'))
        if refine_knob is not None and pq_knob is None:
            raise ValueError('GRL_EVAL_REFINE=%s needs GRL_EVAL_PQ: the shortlists come from GRL_EVAL_PQ\'s index (and '
                             'GRL_EVAL_IVF\'s, when set); set GRL_EVAL_PQ too' % os.environ['GRL_EVAL_REFINE'].strip())
        # a kNN-graph index of the gallery walked by a beam search, off by default (engine.nng_build / nng_search): a report
        nng_knob = parse_nng_knob('GRL_EVAL_NNG', os.environ.get('GRL_EVAL_NNG'))
        if nng_knob is not None:
            why = None
            if rerank:
                why = 'cannot re-rank: the walk scores a query against gallery rows by cosine, and k-reciprocal ' \
                      're-ranking ranks by a Jaccard blend of whole neighbourhoods (evaluate with rerank=0)'
            elif knob is not None:
                why = 'cannot be combined with GRL_EVAL_METRIC=%s: the walk scores rows by the cosine pair distance, not ' \
                      'by the verification head (unset one of them)' % os.environ['GRL_EVAL_METRIC'].strip()
            elif set_knob is not None:
                why = 'cannot be combined with GRL_EVAL_SET: the set distances are taken between clip rows, and the ' \
                      'graph holds one node per tracklet (unset one of them)'
            elif diffusion_knob is not None:
                why = 'cannot be combined with GRL_EVAL_DIFFUSION: the diffusion scores replace the cosine ranking the ' \
                      'walk approximates (unset one of them)'
            if why is not None:
                raise ValueError('GRL_EVAL_NNG=%s %s' % (os.environ['GRL_EVAL_NNG'].strip(), why))
        # binary hash codes of the gallery and Hamming search, off by default (engine.bin_train / bin_search): a report
        bin_knob = parse_bin_knob('GRL_EVAL_BIN', os.environ.get('GRL_EVAL_BIN'))
        if bin_knob is not None:
            why = None
            if rerank:
                why = 'cannot re-rank: the codes approximate the cosine distance of a query to a gallery row, and ' \
                      'k-reciprocal re-ranking ranks by a Jaccard blend of whole neighbourhoods (evaluate with rerank=0)'
            elif knob is not None:
                why = 'cannot be combined with GRL_EVAL_METRIC=%s: the verification head\'s distance is not a count of ' \
                      'hyperplanes between the rows (unset one of them)' % os.environ['GRL_EVAL_METRIC'].strip()
            elif set_knob is not None:
                why = 'cannot be combined with GRL_EVAL_SET: the set distances are taken between clip rows, and the ' \
                      'index holds one code row per tracklet (unset one of them)'
            elif diffusion_knob is not None:
                why = 'cannot be combined with GRL_EVAL_DIFFUSION: the diffusion scores replace the cosine ranking the ' \
                      'index approximates (unset one of them)'
            if why is not None:
                raise ValueError('GRL_EVAL_BIN=%s %s' % (os.environ['GRL_EVAL_BIN'].strip(), why))
        # an int8 scalar-quantised index of the gallery searched on the integer MFMA, off by default (engine.sq8_train /
        # sq8_search): a report
        sq8_knob = parse_sq8_knob('GRL_EVAL_SQ8', os.environ.get('GRL_EVAL_SQ8'))
        if sq8_knob is not None:
            why = None
            if rerank:
                why = 'cannot re-rank: the codes approximate the cosine distance of a query to a gallery row, and ' \
                      'k-reciprocal re-ranking ranks by a Jaccard blend of whole neighbourhoods (evaluate with rerank=0)'
            elif knob is not None:
                why = 'cannot be combined with GRL_EVAL_METRIC=%s: the verification head\'s distance is not a dot product ' \
                      'of the rows (unset one of them)' % os.environ['GRL_EVAL_METRIC'].strip()
            elif set_knob is not None:
                why = 'cannot be combined with GRL_EVAL_SET: the set distances are taken between clip rows, and the ' \
                      'index holds one code row per tracklet (unset one of them)'
            elif diffusion_knob is not None:
                why = 'cannot be combined with GRL_EVAL_DIFFUSION: the diffusion scores replace the cosine ranking the ' \
                      'index approximates (unset one of them)'
            if why is not None:
                raise ValueError('GRL_EVAL_SQ8=%s %s' % (os.environ['GRL_EVAL_SQ8'].strip(), why))
        if pq_knob is not None:
            why = None
            if rerank:
                why = 'cannot re-rank: the tables approximate the cosine distance of a query to a gallery row, and ' \
                      'k-reciprocal re-ranking ranks by a Jaccard blend of whole neighbourhoods (evaluate with rerank=0)'
            elif knob is not None:
                why = 'cannot be combined with GRL_EVAL_METRIC=%s: the verification head\'s distance is not a sum over ' \
                      'column groups of the rows (unset one of them)' % os.environ['GRL_EVAL_METRIC'].strip()
            elif set_knob is not None:
                why = 'cannot be combined with GRL_EVAL_SET: the set distances are taken between clip rows, and the ' \
                      'index holds one code row per tracklet (unset one of them)'
            elif diffusion_knob is not None:
                why = 'cannot be combined with GRL_EVAL_DIFFUSION: the diffusion scores replace the cosine ranking the ' \
                      'index approximates (unset one of them)'
            if why is not None:
                raise ValueError('GRL_EVAL_PQ=%s %s' % (os.environ['GRL_EVAL_PQ'].strip(), why))
        if set_knob is not None:
            why = None
            if not self.only_eval:
                why = 'needs the dense mode (only_eval=True): rrs mode extracts one clip per tracklet, and a set of one ' \
                      'clip has nothing to choose from'
            elif rerank:
                why = 'cannot re-rank: k-reciprocal re-ranking needs set distances of the gallery against itself, which ' \
                      'this route does not compute (evaluate with rerank=0)'
            elif knob is not None:
                why = 'cannot be combined with GRL_EVAL_METRIC=%s: the verification head scores one row per tracklet, ' \
                      'not a clip pair (unset one of them)' % os.environ['GRL_EVAL_METRIC'].strip()
            elif qe is not None or dba is not None or pca_knob is not None:
                why = 'cannot be combined with GRL_EVAL_QE, GRL_EVAL_DBA or GRL_EVAL_PCA: they rewrite one row per ' \
                      'tracklet, and the set distances are taken between the clip rows (unset one of them)'
            elif diffusion_knob is not None:
                why = 'cannot be combined with GRL_EVAL_DIFFUSION: the graph is built on one row per tracklet and its ' \
                      'scores replace the ranking the set distances would give (unset one of them)'
            if why is not None:
                raise ValueError('GRL_EVAL_SET=%s %s' % (os.environ['GRL_EVAL_SET'].strip(), why))
            qf, q_pids, q_camids, qset = self._extract(query_loader, True)
        else:
            qf, q_pids, q_camids = self.extract_feature(query_loader)
        print('Done, obtained {}-by-{} matrix'.format(qf.size(0), qf.size(1)))
        if set_knob is not None:
            gf, g_pids, g_camids, gset = self._extract(gallery_loader, True)
            # the query clips are prepended to the gallery clips, as the query rows are below
            gset = engine.TrackletSet(torch.cat((qset.clips, gset.clips), 0), np.append(qset.counts, gset.counts))
        else:
            gf, g_pids, g_camids = self.extract_feature(gallery_loader)
        gf = torch.cat((qf, gf), 0)               # query is prepended (attevaluator.py:143-145)
        g_pids = np.append(q_pids, g_pids)
        g_camids = np.append(q_camids, g_camids)
        print('Done, obtained {}-by-{} matrix'.format(gf.size(0), gf.size(1)))
        # feature-side post-processing, off by default (engine.expand_features): database-side augmentation replaces every
        # gallery row by the weighted mean of itself and its m nearest other rows, query expansion then does the same
        # for the queries against the (augmented) gallery, under the junk rule CMC / mAP apply.  Everything below runs
        # on the new tensors unchanged.
        if pca_knob is not None:
            qf, gf = _pca_report(pca_knob, qf, gf, path)
        if dba is not None:
            print('Database-side augmentation: m = {}, alpha = {}'.format(*dba))
            gf = engine.expand_features(gf, gf, dba[0], dba[1], skip_self=True)
        if qe is not None:
            print('Query expansion: m = {}, alpha = {}'.format(*qe))
            qf = engine.expand_features(qf, gf, qe[0], qe[1], exclude=(q_pids, g_pids, q_camids, g_camids))
        print("Computing distance matrix")
        if knob is not None:
            # rank by the trained pair-verification head, blended with the cosine distance (engine.verify_metric); the
            # head reads the out_frame slice of the rows [x_uncorr | out_frame | mean].  QE / DBA above ran by cosine.
            return self._evaluate_verify(knob[1], query, gallery, qf, gf, q_pids, q_camids, g_pids, g_camids, path,
                                         visual, stream, roc_bits)
        ids = (q_pids, g_pids, q_camids, g_camids)
        roc_lines = ()

        def extra(lines, cosine_roc=None):
            """the route's ROC lines, then GRL_EVAL_CLUSTER's, GRL_EVAL_CLUSTER_JACCARD's, GRL_EVAL_KMEANS's,
            GRL_EVAL_HDBSCAN's and GRL_EVAL_TSNE's (by cosine or by the Jaccard distance of the features, whatever the
            route ranks by)"""
            if cluster_knob is not None:
                lines = tuple(lines) + tuple(_cluster_report(cluster_knob, qf, gf, ids, path, cosine_roc, sil_knob))
            if jaccard_knob is not None:
                lines = tuple(lines) + tuple(_cluster_jaccard_report(jaccard_knob, gf, ids, path, sil_knob))
            if kmeans_knob is not None:
                lines = tuple(lines) + tuple(_kmeans_report(kmeans_knob, gf, ids, path, sil_knob))
            if hdbscan_knob is not None:
                lines = tuple(lines) + tuple(_hdbscan_report(hdbscan_knob, gf, ids, path, sil_knob))
            if tsne_knob is not None:
                lines = tuple(lines) + tuple(_tsne_report(tsne_knob, gf, ids, path))
            if pq_knob is not None:
                kept = {} if ivf_knob is not None or refine_knob is not None else None
                lines = tuple(lines) + tuple(_pq_report(pq_knob, qf, gf, ids, path, kept))
                if ivf_knob is not None:
                    lines = tuple(lines) + tuple(_ivf_report(ivf_knob, pq_knob, kept, qf, gf, ids, path))
                if refine_knob is not None:
                    lines = tuple(lines) + tuple(_refine_report(refine_knob, kept, qf, gf, ids, path))
            if nng_knob is not None:
                lines = tuple(lines) + tuple(_nng_report(nng_knob, qf, gf, ids, path))
            if bin_knob is not None:
                lines = tuple(lines) + tuple(_bin_report(bin_knob, qf, gf, ids, path))
            if sq8_knob is not None:
                lines = tuple(lines) + tuple(_sq8_report(sq8_knob, qf, gf, ids, path))
            return lines
        if set_knob is not None:
            reduce, metric = set_knob
            print('Tracklet set distance: {} ({}), {} clips in {} tracklets'.format(
                reduce, metric, int(gset.clips.size(0)), gset.n))
            if visual:
                self._visualize(query, gallery, qf, gf, q_pids, q_camids, g_pids, g_camids, path, 0,
                                setdist=(qset, gset, reduce, metric))
            if roc_bits:
                roc_lines = _roc_report(engine.set_pair_roc(qset, gset, *ids, reduce=reduce, metric=metric, bits=roc_bits),
                                        'set({},{})'.format(reduce, metric), path)
            return _report(*engine.set_metrics_streaming(qset, gset, q_pids, g_pids, q_camids, g_camids, reduce=reduce,
                                                         metric=metric), roc_lines=extra(roc_lines))
        if diffusion_knob is not None:
            graph = _diffusion_report(diffusion_knob, gf, path)
            k, kq, alpha, n_iter = diffusion_knob
            if visual:
                self._visualize(query, gallery, qf, gf, q_pids, q_camids, g_pids, g_camids, path, 0,
                                diffusion=(graph, kq, alpha, n_iter))
            return _report(*engine.diffusion_metrics_streaming(qf, gf, q_pids, g_pids, q_camids, g_camids, graph=graph,
                                                               kq=kq, alpha=alpha, n_iter=n_iter),
                           roc_lines=extra(roc_lines))
        if visual:
            self._visualize(query, gallery, qf, gf, q_pids, q_camids, g_pids, g_camids, path, rerank)
        if rerank_stream:
            # k-reciprocal re-ranking over column blocks (engine.rerank_metrics_streaming): the values of the device
            # re_ranking below without its (q+g)^2 matrices, for any q + g.  Under torch.distributed the sample passes
            # are sharded by sample range and the final pass by gallery column; every rank gets the full result.
            print('Applying person re-ranking ...')
            if roc_bits:                          # (a second pass over the re-ranking state: the knob's cost here)
                roc_lines = _roc_report(engine.rerank_pair_roc(qf, gf, *ids, bits=roc_bits), 'rerank(cosine)', path)
            return _report(*engine.rerank_metrics_streaming(qf, gf, q_pids, g_pids, q_camids, g_camids),
                           roc_lines=extra(roc_lines))
        if stream:
            # column blocks of the distance GEMM and exact CMC / mAP without a sort (engine.rank_metrics_streaming); under
            # torch.distributed the gallery columns are sharded and only match keys and rank histograms travel
            roc = None
            if roc_bits:
                roc = engine.pair_roc(qf, gf, *ids, bits=roc_bits)
                roc_lines = _roc_report(roc, 'cosine', path)
            return _report(*engine.rank_metrics_streaming(qf, gf, q_pids, g_pids, q_camids, g_camids),
                           roc_lines=extra(roc_lines, roc))
        if roc_bits and rerank and qf.size(0) + gf.size(0) > 16384:
            raise ValueError('GRL_EVAL_ROC: %d samples re-rank on the host (more than 16384), where no device matrix '
                             'exists to measure; set GRL_EVAL_RERANK=stream' % (qf.size(0) + gf.size(0)))
        dist_dev = grl_dist.sharded_distmat(qf, gf, cosin_dist)     # gallery rows sharded over the ranks
        # ranking AND the per-query CMC / AP work on the device (one LDS sort network per row up to
        # 16384 gallery entries -- MARS: 11310 -- the chunked network beyond): neither the distance nor
        # the index matrix leaves HBM
        if not rerank:
            roc = None
            if roc_bits:
                roc = engine.pair_roc_matrix(dist_dev, *ids, bits=roc_bits)
                roc_lines = _roc_report(roc, 'cosine', path)
            return evaluate_seq(None, q_pids, q_camids, g_pids, g_camids, path,
                                indices=engine.rank_rows(dist_dev), roc_lines=extra(roc_lines, roc))
        if rerank and qf.size(0) + gf.size(0) <= 16384:
            print('Applying person re-ranking ...')            # entirely on the device
            dist_dev = re_ranking(dist_dev, pairwise_distance_tensor(qf, qf), pairwise_distance_tensor(gf, gf))
            if roc_bits:
                roc_lines = _roc_report(engine.pair_roc_matrix(dist_dev, *ids, bits=roc_bits), 'rerank(cosine)', path)
            return evaluate_seq(None, q_pids, q_camids, g_pids, g_camids, path,
                                indices=engine.rank_rows(dist_dev), roc_lines=extra(roc_lines))
        distmat = dist_dev.cpu().numpy()
        if rerank:                                             # beyond one LDS sort network: host numpy
            print('Applying person re-ranking ...')
            distmat_qq = pairwise_distance_tensor(qf, qf).cpu().numpy()
            distmat_gg = pairwise_distance_tensor(gf, gf).cpu().numpy()
            distmat = re_ranking(distmat, distmat_qq, distmat_gg)
        return evaluate_seq(distmat, q_pids, q_camids, g_pids, g_camids, path, roc_lines=extra(roc_lines))

    def _evaluate_verify(self, beta, query, gallery, qf, gf, q_pids, q_camids, g_pids, g_camids, path, visual, stream,
                         roc_bits=None):
        """The three routes of ``evaluate`` (no re-ranking) under GRL_EVAL_METRIC=verify[,beta].  ``roc_bits``
        (GRL_EVAL_ROC): the pair-level figures of the same distances; for beta = 1 ``engine.verify_prob`` maps a
        threshold of roc.json's curve to the head's P(same)."""
        siam = self.siamese_model
        vm = engine.verify_metric(siam, qf.size(1) - 2 * siam.input_num, beta)
        print('Ranking metric: verification head, beta = {:g}'.format(beta))
        if visual:
            self._visualize(query, gallery, qf, gf, q_pids, q_camids, g_pids, g_camids, path, 0, metric=vm)
        ids, roc_lines = (q_pids, g_pids, q_camids, g_camids), ()
        if stream:
            if roc_bits:
                roc_lines = _roc_report(engine.pair_roc(qf, gf, *ids, metric=vm, bits=roc_bits), repr(vm), path)
            return _report(*engine.rank_metrics_streaming(qf, gf, q_pids, g_pids, q_camids, g_camids, metric=vm),
                           roc_lines=roc_lines)
        dist_dev = grl_dist.sharded_distmat(qf, gf, lambda q, g: engine.verify_dist(q, g, vm))
        if roc_bits:
            roc_lines = _roc_report(engine.pair_roc_matrix(dist_dev, *ids, bits=roc_bits), repr(vm), path)
        return evaluate_seq(None, q_pids, q_camids, g_pids, g_camids, path, indices=engine.rank_rows(dist_dev),
                            roc_lines=roc_lines)
