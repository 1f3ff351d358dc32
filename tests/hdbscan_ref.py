"""Host model of the HDBSCAN contract in numpy, for the tests of engine.mutual_reachability_mst /
hdbscan / hdbscan_matrix / hdbscan_from_mst.  float32 operation by operation up to the forest, float64 for the cut.

Distance of a pair {lo < hi}: a matrix entry as it is, or ``cosine_matrix``: v = fl(fl(d * rinv[lo]) * rinv[hi]) of
d = -dot, the smaller index first, dist = fl(1 + v), negative -> 0.  core[i]: row i of search's top-min_samples list
(order: value with -0 == +0 and NaN last, then index) with the entry of index i deleted, or the last entry if it is not
there; the last remaining value, +0 for min_samples = 1.  w = dist; if core[lo] > w: w = core[lo]; if core[hi] > w:
w = core[hi].  No edge: a core distance that is not finite, a w that is NaN or +inf.  Edges are ordered by (w by float <,
lo, hi); under that strict order the minimum spanning forest is unique, and the model builds it by Kruskal's algorithm
-- not by the Boruvka rounds of the device code -- so the comparison is one of results, not of steps.

The cut is written from the same contract as engine._hdbscan_cut but keeps every node's member list and recurses on the
splits, where the engine keeps one "cluster a point left" per point."""
import numpy as np

import search_ref
import silhouette_ref as SR

F = np.float32
FLOOR = 2.0 ** -126


def cosine_matrix(negdot, sq):
    """The symmetric cosine form of D = -dot [n, n] (bitwise symmetric) and the rows' squared norms [n]."""
    r = SR.rinv(sq)
    n = r.size
    i, j = np.arange(n)[:, None], np.arange(n)[None, :]
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    with np.errstate(invalid='ignore', over='ignore'):
        v = ((np.asarray(negdot, dtype=F) * r[lo]).astype(F) * r[hi]).astype(F)
        dist = (F(1.0) + v).astype(F)
        return np.where(dist < 0, F(0.0), dist).astype(F)


def core_distances(dist, min_samples):
    dist = np.asarray(dist, dtype=F)
    n = dist.shape[0]
    core = np.zeros(n, dtype=F)
    if min_samples == 1:
        return core
    for i in range(n):
        comp = search_ref.composite(search_ref.sort_key(dist[i]), np.arange(n))
        top = np.argsort(comp, kind='stable')[:min_samples].tolist()
        if i in top:
            top.remove(i)
        else:
            top.pop()
        core[i] = dist[i, top[-1]]
    return core


def weights(dist, core):
    """(lo, hi, w) of every edge of the mutual-reachability graph, in the total order (w, lo, hi)."""
    dist = np.asarray(dist, dtype=F)
    n = dist.shape[0]
    lo, hi = np.triu_indices(n, 1)
    w = dist[lo, hi].copy()
    with np.errstate(invalid='ignore'):
        a = core[lo] > w
        w[a] = core[lo][a]
        b = core[hi] > w
        w[b] = core[hi][b]
        keep = np.isfinite(core[lo]) & np.isfinite(core[hi]) & (w < np.inf)
    lo, hi, w = lo[keep], hi[keep], w[keep]
    order = np.lexsort((hi, lo, w))
    return lo[order].astype(np.int32), hi[order].astype(np.int32), w[order]


def reachability_matrix(dist, core):
    """The dense symmetric matrix of the weights, +inf where there is no edge and on the diagonal."""
    n = np.asarray(dist).shape[0]
    lo, hi, w = weights(dist, core)
    m = np.full((n, n), np.inf, dtype=F)
    m[lo, hi] = w
    m[hi, lo] = w
    return m


def _find(parent, a):
    while parent[a] != a:
        parent[a] = parent[parent[a]]
        a = parent[a]
    return a


def forest(dist, min_samples):
    """(lo int32, hi int32, w float32, core float32): the minimum spanning forest in the edges' order, by Kruskal."""
    core = core_distances(dist, min_samples)
    lo, hi, w = weights(dist, core)
    parent = list(range(np.asarray(dist).shape[0]))
    keep = []
    for k, (a, b) in enumerate(zip(lo.tolist(), hi.tolist())):
        ra, rb = _find(parent, a), _find(parent, b)
        if ra != rb:
            parent[ra] = rb
            keep.append(k)
    keep = np.asarray(keep, dtype=np.int64)
    return lo[keep], hi[keep], w[keep], core


def cut(lo, hi, w, n, mcs, method='eom'):
    """(labels int64 [n], stabilities float64 [n_clusters]) of a forest given in the edges' order."""
    if method not in ('eom', 'leaf'):
        raise ValueError("method must be 'eom' or 'leaf' (got %r)" % (method,))
    lo, hi = np.asarray(lo).tolist(), np.asarray(hi).tolist()
    w = np.asarray(w, dtype=np.float64)
    parent = list(range(n))
    tree = {i: (0.0, None, None, [i]) for i in range(n)}     # union-find root -> (lambda, left, right, members)
    for k in range(len(lo)):
        a, b = _find(parent, lo[k]), _find(parent, hi[k])
        assert a != b, 'edge %d closes a cycle' % k
        ta, tb = tree.pop(a), tree.pop(b)
        parent[a] = b
        tree[b] = (1.0 / max(float(w[k]), FLOOR), ta, tb, ta[3] + tb[3])
    tops = [t for t in tree.values() if len(t[3]) >= mcs]

    def condense(t, birth):
        """the cluster born at lambda = birth with the members of t: (stability, members, child clusters)"""
        members, s = t[3], 0.0
        while t[1] is not None:
            lam, a, b, _ = t
            na, nb = len(a[3]), len(b[3])
            if na >= mcs and nb >= mcs:
                s += (na + nb) * (lam - birth)
                return s, members, [condense(a, lam), condense(b, lam)]
            if na >= mcs or nb >= mcs:
                small, t = (b, a) if na >= mcs else (a, b)
                s += len(small[3]) * (lam - birth)
                continue
            s += (na + nb) * (lam - birth)
            break
        return s, members, []

    def eom(c, selectable):
        s, _, kids = c
        if not kids:
            return s, ([c] if selectable else [])
        got = [eom(k, True) for k in kids]
        tot = got[0][0] + got[1][0]
        if not selectable or tot > s:
            return tot, got[0][1] + got[1][1]
        return s, [c]

    def leaves(c, selectable):
        if not c[2]:
            return [c] if selectable else []
        return leaves(c[2][0], True) + leaves(c[2][1], True)
    chosen = []
    for t in tops:
        c = condense(t, 0.0)
        chosen += eom(c, len(tops) >= 2)[1] if method == 'eom' else leaves(c, len(tops) >= 2)
    chosen.sort(key=lambda c: min(c[1]))
    labels = np.full(n, -1, dtype=np.int64)
    for k, c in enumerate(chosen):
        labels[c[1]] = k
    return labels, np.asarray([c[0] for c in chosen], dtype=np.float64)


def same_partition(a, b):
    """the same noise set and the same grouping of the rest, whatever the numbering"""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a < 0, b < 0):
        return False
    keep = a >= 0
    pairs = np.unique(np.stack((a[keep], b[keep]), 1), axis=0)
    return pairs.shape[0] == np.unique(a[keep]).size == np.unique(b[keep]).size
