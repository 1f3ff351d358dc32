"""Host model of the silhouette contract in numpy, for the tests of engine.silhouette and its forms.

Member order: mem holds cluster 0's samples in ascending sample index, then cluster 1's, ..; mptr[c] = the first position
of cluster c; a sample with a label outside 0..k-1 is nobody's and is not in mem.  Sum of row i towards cluster c: 64
partial sums, partial l = the sequential float32 sum from +0.0, in ascending position, of the distances at the
cluster's positions p with p % 64 == l, the position with mem[p] == i left out by index; then part[l] += part[l + s],
l < s, for s = 32, 16, 8, 4, 2, 1.  mean = sum / float32(count), count = n_c - 1 for the own cluster and n_c otherwise.
a = the own cluster's mean (0 for a cluster of one); b = the minimum over the other non-empty clusters (-0 below +0,
from +inf), NaN as soon as one mean is NaN.  s = 0 for nobody's samples and
clusters of one, NaN when a or b is NaN, 0 when max(a, b) == 0, otherwise float32(float32(b - a) / max(a, b)).

``samples`` is that in float32, operation by operation; ``samples64`` evaluates the same definitions in float64."""
import numpy as np

F = np.float32


def relabel(labels, noise='singleton'):
    """(labels int64 with -1 = nobody's, k): 'singleton' turns every label < 0 into a cluster of its own, numbered from
    max(label) + 1 in ascending sample index; 'drop' leaves them nobody's."""
    if noise not in ('singleton', 'drop'):
        raise ValueError("noise must be 'singleton' or 'drop' (got %r)" % (noise,))
    lab = np.asarray(labels).astype(np.int64).copy()
    neg = lab < 0
    lab[neg] = -1
    k = int(lab.max()) + 1 if lab.size else 0
    if noise == 'singleton':
        lab[neg] = k + np.arange(int(neg.sum()))
        k += int(neg.sum())
    return lab, k


def member_order(lab, k):
    """(mem int64 [m], mptr int64 [k+1], counts int64 [k]) of labels with -1 = nobody's."""
    counts = np.bincount(lab[lab >= 0], minlength=k).astype(np.int64)
    mptr = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    mem = np.flatnonzero(lab >= 0)
    mem = mem[np.argsort(lab[mem], kind='stable')]               # ascending sample index inside a cluster
    return mem.astype(np.int64), mptr, counts


def tree(part):
    """part [.., 64] float32 -> [..]: part[l] += part[l + s], l < s, for s = 32 .. 1."""
    part = np.array(part, dtype=F)
    s = 32
    while s:
        part[..., :s] = part[..., :s] + part[..., s:2 * s]
        s //= 2
    return part[..., 0]


def rinv(sq):
    """1.0f / sqrtf(sq), both correctly rounded."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return (F(1.0) / np.sqrt(np.asarray(sq, dtype=F))).astype(F)


def cosine_matrix(negdot, sq):
    """The cosine form of D = -dot [n, n] and the rows' squared norms [n]: v = (D * rinv_i) * rinv_j, dist = 1 + v,
    dist < 0 ? 0 : dist (a NaN stays), every operation rounded to float32."""
    r = rinv(sq)
    with np.errstate(invalid='ignore', over='ignore'):
        v = ((np.asarray(negdot, dtype=F) * r[:, None]).astype(F) * r[None, :]).astype(F)
        dist = (F(1.0) + v).astype(F)
        return np.where(dist < 0, F(0.0), dist).astype(F)


def cluster_sums(dist, lab, k):
    """(sums float32 [n, k], mem, mptr, counts): the sum of every row towards every cluster in the contract's order;
    rows of nobody's samples are computed too (nothing is left out of them) and are ignored by ``samples``."""
    dist = np.asarray(dist, dtype=F)
    n = dist.shape[0]
    mem, mptr, counts = member_order(lab, k)
    sums = np.zeros((n, k), dtype=F)
    rows = np.arange(n)
    with np.errstate(invalid='ignore', over='ignore'):
        for c in range(k):
            part = np.zeros((n, 64), dtype=F)
            for p in range(mptr[c], mptr[c + 1]):
                take = rows != mem[p]
                part[take, p % 64] = part[take, p % 64] + dist[take, mem[p]]
            sums[:, c] = tree(part)
    return sums, mem, mptr, counts


def samples(dist, labels, noise='singleton'):
    """(s, a, b float32 [n], scored bool [n]) of a float32 [n, n] matrix of distances, used as given."""
    lab, k = relabel(labels, noise)
    n = lab.size
    sums, mem, mptr, counts = cluster_sums(dist, lab, k)
    a = np.zeros(n, dtype=F)
    b = np.full(n, np.inf, dtype=F)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for c in range(k):
            if counts[c] == 0:
                continue
            own = lab == c
            if counts[c] > 1:
                a[own] = sums[own, c] / F(counts[c] - 1)
            mean = (sums[:, c] / F(counts[c])).astype(F)
            less = (mean < b) | ((mean == b) & np.signbit(mean) & ~np.signbit(b))        # -0 below +0
            nb = np.where(np.isnan(b) | np.isnan(mean), F(np.nan), np.where(less, mean, b)).astype(F)
            b[~own] = nb[~own]
        s = np.zeros(n, dtype=F)
        for i in range(n):
            if lab[i] < 0:
                a[i] = b[i] = 0
            elif counts[lab[i]] <= 1:
                a[i] = 0
            elif np.isnan(a[i]) or np.isnan(b[i]):
                s[i] = np.nan
            else:
                mx = a[i] if a[i] > b[i] else b[i]
                s[i] = F(0) if mx == 0 else F(F(b[i] - a[i]) / mx)
    return s, a, b, lab >= 0


def score(s, scored):
    """float64 mean of the scored samples (NaN if one of them is NaN)."""
    return float(np.asarray(s, dtype=np.float64)[scored].mean())


def samples64(dist, labels, noise='singleton'):
    """The same definitions in float64, without any prescribed order: (s, a, b float64 [n], scored)."""
    dist = np.asarray(dist, dtype=np.float64)
    lab, k = relabel(labels, noise)
    n = lab.size
    counts = np.bincount(lab[lab >= 0], minlength=k)
    a, b, s = np.zeros(n), np.zeros(n), np.zeros(n)
    members = [np.flatnonzero(lab == c) for c in range(k)]
    with np.errstate(invalid='ignore'):
        for i in range(n):
            if lab[i] < 0:
                continue
            cand = [dist[i, members[c]].mean() for c in range(k) if counts[c] and c != lab[i]]
            b[i] = np.nan if np.isnan(cand).any() else min(cand)
            if counts[lab[i]] <= 1:
                continue
            own = members[lab[i]]
            a[i] = dist[i, own[own != i]].sum() / (counts[lab[i]] - 1)
            mx = max(a[i], b[i])
            s[i] = np.nan if np.isnan(a[i]) or np.isnan(b[i]) else (0.0 if mx == 0 else (b[i] - a[i]) / mx)
    return s, a, b, lab >= 0


def planted(sizes=(1, 1, 2, 3, 63, 64, 65, 130, 7), d=24, seed=5, spread=0.25):
    """(x float32 [n, d], planted ids int64 [n]): clusters of the given sizes around random unit directions, every row
    scaled to a norm drawn from 0.5 .. 1.8, the order shuffled.  Built from the seed alone."""
    g = np.random.Generator(np.random.PCG64(seed))
    ids = np.repeat(np.arange(len(sizes)), sizes)
    centres = g.standard_normal((len(sizes), d))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    x = centres[ids] + spread / np.sqrt(d) * g.standard_normal((ids.size, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x *= g.uniform(0.5, 1.8, (ids.size, 1))
    perm = g.permutation(ids.size)
    return x[perm].astype(F), ids[perm]


def select_case(seed=9, d=32, per=20, sigma=0.04):
    """(x float32 [4 * per, d] unit rows, ids): four clusters A, B, C, D around unit directions with cos(A, B) = 0.5 and
    every other pair orthogonal, shuffled -- the input of the cluster_select tests.  At a cosine eps of -0.97 every
    sample stands alone, at -0.75 the four clusters come out, at -0.27 A and B merge."""
    g = np.random.Generator(np.random.PCG64(seed))
    centres = np.zeros((4, d))
    centres[0, 0] = 1.0
    centres[1, 0], centres[1, 1] = 0.5, np.sqrt(0.75)
    centres[2, 2] = 1.0
    centres[3, 3] = 1.0
    ids = np.repeat(np.arange(4), per)
    x = centres[ids] + sigma * g.standard_normal((ids.size, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    perm = g.permutation(ids.size)
    return x[perm].astype(F), ids[perm]


SELECT_EPS = (-0.97, -0.75, -0.27)
