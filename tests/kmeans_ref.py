"""Host model (numpy) of the k-means contract of DESIGN.md 4t: engine.kmeans_assign / cluster_centroids / kmeans.

Assign works on a float32 distance matrix somebody else computed (the device's own materialised matrix in the GPU
tests, a numpy one in the CPU tests), so labels are integers derived from given bits.  The sum reproduces the
kernel's fixed order in float32: members in ascending sample index dealt to four partial sums, each a sequential
sum from +0.0f, joined as (p0 + p1) + (p2 + p3)."""
import numpy as np

F32 = np.float32


def order_keys(D):
    """csrc/sort_order.h order_key: canonical NaN after +inf, -0 == +0, ascending as unsigned integers."""
    D = np.ascontiguousarray(D, dtype=F32)
    u = D.view(np.uint32).copy()
    u[np.isnan(D)] = 0x7fc00000
    u[D == 0] = 0
    neg = (u & 0x80000000) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def assign(D):
    """(labels int64 [n], best float32 [n]) of a distance matrix D [n, k]: the smallest key, ties to the smaller
    centroid index; a NaN best distance (every entry of the row is NaN) gives label -1."""
    D = np.asarray(D, dtype=F32)
    n = D.shape[0]
    lab = np.argmin(order_keys(D), axis=1).astype(np.int64)      # (argmin: the first of equal keys)
    best = D[np.arange(n), lab]
    lab[np.isnan(best)] = -1
    return lab, best


def members(labels, k):
    """Per cluster, the sample indices with that label in ascending order; labels < 0 belong to nobody."""
    labels = np.asarray(labels)
    return [np.flatnonzero(labels == j) for j in range(k)]


def segment_sum(x, labels, k):
    """(sum float32 [k, d], counts int64 [k]) in the normative order."""
    x = np.asarray(x, dtype=F32)
    out = np.zeros((k, x.shape[1]), dtype=F32)
    counts = np.zeros(k, dtype=np.int64)
    for j, m in enumerate(members(labels, k)):
        counts[j] = m.size
        p = np.zeros((4, x.shape[1]), dtype=F32)
        for pos, i in enumerate(m):
            p[pos & 3] = p[pos & 3] + x[i]
        out[j] = (p[0] + p[1]) + (p[2] + p[3])
    return out, counts


def centroids(x, labels, k, reduce='mean', prev=None):
    """(centroids float32 [k, d], counts, n_empty): 'sum', 'mean' = sum / float32(count), 'unit' = sum * (1 /
    sqrt(sum of squares)) with the squares summed in float32 (the order of that sum is the kernel's own business:
    compare 'unit' within a bound).  Empty (no member; 'unit': norm zero or not finite) -> prev's row or zeros."""
    if reduce not in ('sum', 'mean', 'unit'):
        raise ValueError(reduce)
    s, counts = segment_sum(x, labels, k)
    out = np.zeros_like(s)
    n_empty = 0
    with np.errstate(all='ignore'):
        for j in range(k):
            empty = counts[j] == 0
            if not empty and reduce == 'unit':
                sq = F32(0)
                for v in s[j]:
                    sq = F32(sq + F32(v * v))
                if not (sq > 0) or not np.isfinite(sq):
                    empty = True
                else:
                    out[j] = s[j] * (F32(1) / np.sqrt(sq, dtype=F32))
            elif not empty:
                out[j] = s[j] if reduce == 'sum' else s[j] / F32(counts[j])
            if empty:
                n_empty += 1
                out[j] = prev[j] if prev is not None else 0
    return out, counts, n_empty


def validate(n, k, max_iter):
    for name, v, lo in (('k', k, 1), ('max_iter', max_iter, 1)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < lo:
            raise ValueError('%s must be an integer >= %d (got %r)' % (name, lo, v))
    if k > n:
        raise ValueError('k must be in 1..n')


def init_rows(x, k, init, seed=0):
    """C0 of the loop: a [k, d] array as it is, k distinct sample indices, or 'random' with ``seed``."""
    n = x.shape[0]
    if isinstance(init, np.ndarray) and init.ndim == 2:
        if init.shape != (k, x.shape[1]):
            raise ValueError('init centroids must be [k, d]')
        return init.astype(F32).copy()
    if isinstance(init, str):
        if init != 'random':
            raise ValueError('unknown init %r' % init)
        idx = np.random.Generator(np.random.PCG64(seed)).choice(n, k, replace=False)
    else:
        idx = np.asarray(list(init))
        if idx.ndim != 1 or idx.dtype.kind not in 'iu' or idx.size != k or idx.min() < 0 or idx.max() >= n \
                or np.unique(idx).size != k:
            raise ValueError('init must hold k distinct sample indices')
    return np.asarray(x, dtype=F32)[idx].copy()


def cosine_matrix(x, c):
    return (-(np.asarray(x, dtype=F32) @ np.asarray(c, dtype=F32).T)).astype(F32)


def euclidean_matrix(x, c):
    x, c = np.asarray(x, dtype=F32), np.asarray(c, dtype=F32)
    d2 = (x * x).sum(1)[:, None] + (c * c).sum(1)[None, :] - F32(2) * (x @ c.T)
    return np.sqrt(np.maximum(d2, F32(1e-12))).astype(F32)


def kmeans(x, k, metric='cosine', init='random', seed=0, max_iter=50, dist=None):
    """The loop.  ``dist(C) -> D [n, k] float32`` is the distance of every sample to the centroids C (default: the
    numpy forms above).  Returns a dict with the fields of engine.KMeans."""
    x = np.asarray(x, dtype=F32)
    n = x.shape[0]
    validate(n, k, max_iter)
    if metric not in ('cosine', 'euclidean'):
        raise ValueError(metric)
    if dist is None:
        fn = cosine_matrix if metric == 'cosine' else euclidean_matrix
        dist = lambda c: fn(x, c)                                                     # noqa: E731
    reduce = 'unit' if metric == 'cosine' else 'mean'
    cent = init_rows(x, k, init, seed)
    labels, n_changed, converged = None, [], False
    while len(n_changed) < max_iter and not converged:
        new, best = assign(dist(cent))
        n_changed.append(n if labels is None else int((new != labels).sum()))
        labels = new
        cent, counts, n_empty = centroids(x, labels, k, reduce, cent)
        converged = n_changed[-1] == 0
    ok = labels >= 0
    b = best[ok].astype(np.float64)
    return {'labels': labels, 'centroids': cent, 'counts': counts, 'n_iter': len(n_changed), 'converged': converged,
            'n_changed': n_changed, 'n_empty': n_empty, 'n_unassigned': int(n - ok.sum()), 'k': k, 'metric': metric,
            'inertia': float((b if metric == 'cosine' else b * b).sum())}


def same_partition(a, b):
    """Do two label vectors describe the same partition (label names aside; negatives are singletons)?"""
    a, b = np.asarray(a).copy(), np.asarray(b).copy()
    if a.shape != b.shape:
        return False
    for v in (a, b):
        neg = v < 0
        v[neg] = v.max() + 1 + np.arange(int(neg.sum())) if v.size else 0
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))
