"""numpy model of the Jaccard eps-graph of one sample set (engine.jaccard_graph / cluster_jaccard,
grl_amd/csrc/jaccard.hip), the normative statement of its contract.

Input: S = pairwise_distance_tensor(xf, xf) [n][n] float32 (unsquared).  colmax[i] = max_r S[r][i]^2,
D[i][j] = S[j][i]^2 / colmax[i]; the first K = max(k1+1, k2) entries of every D row (ties to the smaller index), the
expansion lists, the weights V = exp(-D) / sum and V2 are the sample passes of tests/rerank_stream_ref.py applied to the
one-set matrix: nothing is stacked, no sample is counted twice.  Then, for every row i on its own,

    t[i][j] = float32 sum, from +0, over the k with V2[i][k] != 0 in ascending k, of min(V2[i][k], V2[j][k])
    J[i][j] = 1 - t / (2 - t);   edge i -> j  iff  j != i and J[i][j] <= float32(eps)   (eps finite and < 1)

``graph`` is the streaming form (column blocks of S, sparse rows, an inverted index of ALL rows, accumulator windows);
``dense_graph`` is the plain transcription with full D, V and V2 and a loop over k.  Both return the CSR
(row_ptr int64 [n+1], col int32 [E] ascending within a row, val float32 [E] = J of each edge)."""
import numpy as np

import rerank_stream_ref as R

ONE, TWO = np.float32(1), np.float32(2)


def euclid(x):
    """pairwise_distance_tensor(x, x) on the host (float32; not the device GEMM's bits)."""
    x = np.asarray(x, np.float32)
    sq = (x * x).sum(1)
    d = sq[:, None] + sq[None, :] - 2 * (x @ x.T)
    return np.sqrt(np.maximum(d, 1e-12)).astype(np.float32)


class OneSet(object):
    """Columns of S^2 for the sample passes of rerank_stream_ref (its ``Stack`` for one set)."""

    def __init__(self, S):
        self.S = np.asarray(S, np.float32)
        self.N = self.S.shape[0]
        assert self.S.shape == (self.N, self.N) and self.N >= 2

    def columns(self, i0, i1):
        s = self.S[:, i0:i1]
        return s * s


def check_args(n, eps, k1, k2):
    if not (n >= 2 and 1 <= k1 <= 20 and k1 < n and 1 <= k2 <= 8 and k2 <= n):
        raise ValueError('n = %d, k1 = %d, k2 = %d' % (n, k1, k2))
    eps = np.float32(eps)
    if not np.isfinite(eps) or eps >= 1:
        raise ValueError('eps must be finite and < 1')
    return eps


def sparse_rows(S, k1=20, k2=6, width=64, weights=None):
    """(colmax, rank [n][K], lists, vals, v2) of the one-set matrix; ``weights`` replaces the computed ``vals`` (a list
    of float32 arrays, one per sample, aligned with ``lists``)."""
    st = OneSet(S)
    colmax, rank = R.rank_lists(st, max(k1 + 1, k2), width)
    lists = R.expansion_lists(rank, k1)
    vals = R.weights(st, colmax, lists, width) if weights is None else [np.asarray(v, np.float32) for v in weights]
    assert all(v.shape == l.shape for v, l in zip(vals, lists))
    return colmax, rank, lists, vals, expand(rank, lists, vals, k2)


def expand(rank, lists, vals, k2):
    """rerank_stream_ref.expand, also for samples whose expansion list is EMPTY: a sample that ties with more than k1
    others at distance 0 is not among its own first k1 + 1 neighbours, so it has no k-reciprocal neighbour at all.
    Such a list adds nothing to a union and +0 to every sum."""
    out = []
    for i in range(rank.shape[0]):
        rows = [i] if k2 == 1 else list(rank[i, :k2])
        cols = np.unique(np.concatenate([lists[r] for r in rows])).astype(np.int32)
        s = np.zeros(cols.size, np.float32)
        for u, r in enumerate(rows):
            term = np.zeros(cols.size, np.float32)
            if lists[r].size:
                pos = np.minimum(np.searchsorted(lists[r], cols), lists[r].size - 1)
                hit = lists[r][pos] == cols
                term[hit] = vals[r][pos[hit]]
            s = term if u == 0 else (s + term).astype(np.float32)
        v = s if k2 == 1 else (s / np.float32(k2)).astype(np.float32)
        nz = v != 0
        out.append((cols[nz], v[nz]))
    return out


def jaccard_of(t):
    return (ONE - t / (TWO - t)).astype(np.float32)


def jaccard_rows(v2, n, window=64):
    """J [n][n] from the sparse V2 rows by the streaming product: an inverted index of all rows (ascending j in every
    column), and for every row the accumulator windows in ascending order, inside a window the row's non-zero k in
    ascending order.  (The model may hold n x n; the device never does.)"""
    csc = [[] for _ in range(n)]
    for j in range(n):
        for k, v in zip(*v2[j]):
            csc[k].append((j, v))
    csc = [(np.array([j for j, _ in c], np.int64), np.array([v for _, v in c], np.float32)) for c in csc]
    Jm = np.empty((n, n), np.float32)
    for i in range(n):
        for w0, w1 in R.spans(n, window):
            acc = np.zeros(w1 - w0, np.float32)
            for k, vk in zip(*v2[i]):
                rows, cv = csc[k]
                if window < n:
                    sel = (rows >= w0) & (rows < w1)
                    rows, cv = rows[sel], cv[sel]
                idx = rows - w0
                acc[idx] = acc[idx] + np.minimum(vk, cv)
            Jm[i, w0:w1] = jaccard_of(acc)
    return Jm


def threshold(Jm, eps):
    """The CSR (row_ptr, col, val) of the edges of a dense J: j != i and J <= float32(eps), a NaN never."""
    with np.errstate(invalid='ignore'):
        A = np.asarray(Jm, np.float32) <= np.float32(eps)
    np.fill_diagonal(A, False)
    r, c = np.nonzero(A)
    return np.concatenate(([0], np.cumsum(A.sum(1)))).astype(np.int64), c.astype(np.int32), Jm[r, c]


def graph_from_v2(v2, n, eps, window=64):
    return threshold(jaccard_rows(v2, n, window), eps)


def graph(S, eps, k1=20, k2=6, width=64, window=64, weights=None):
    """The model: (row_ptr, col, val)."""
    n = np.asarray(S).shape[0]
    eps = check_args(n, eps, k1, k2)
    v2 = sparse_rows(S, k1, k2, width, weights)[4]
    return graph_from_v2(v2, n, eps, window)


def dense_matrices(S, k1=20, k2=6):
    """(D, V, V2, J) [n][n] float32 by the plain formulas."""
    S = np.asarray(S, np.float32)
    n = S.shape[0]
    sq = S * S
    colmax = sq.max(axis=0)
    D = (sq / colmax[None, :]).T.copy()                      # D[i][j] = S[j][i]^2 / colmax[i]
    K = max(k1 + 1, k2)
    rank = np.argsort(D, axis=1, kind='stable')[:, :K].astype(np.int32)
    lists = R.expansion_lists(rank, k1)
    V = np.zeros((n, n), np.float32)
    for i, e in enumerate(lists):
        w = np.exp(-D[i, e])
        V[i, e] = (w / np.sum(w)).astype(np.float32)
    if k2 == 1:
        V2 = V
    else:
        V2 = np.zeros((n, n), np.float32)
        for i in range(n):
            s = V[rank[i, 0]].copy()
            for u in range(1, k2):
                s = (s + V[rank[i, u]]).astype(np.float32)
            V2[i] = s / np.float32(k2)
    T = np.zeros((n, n), np.float32)
    for i in range(n):
        for k in np.flatnonzero(V2[i]):                      # ascending k; a zero V2[j][k] adds +0
            T[i] = T[i] + np.minimum(V2[i, k], V2[:, k])
    return D, V, V2, jaccard_of(T)


def dense_graph(S, eps, k1=20, k2=6):
    eps = check_args(np.asarray(S).shape[0], eps, k1, k2)
    return threshold(dense_matrices(S, k1, k2)[3], eps)


def adjacency(row_ptr, col, n):
    A = np.zeros((n, n), dtype=bool)
    A[np.repeat(np.arange(n), np.diff(row_ptr)), col] = True
    return A


# ---- inputs shared by the tests ------------------------------------------------------------------------------------
def features(n, d, seed, special=True):
    """n rows around a few centres with different spreads; with ``special`` (n >= 8) three rows are exact copies of
    others (exact ties in D and in the rank lists) and one row is all zero."""
    g = np.random.Generator(np.random.PCG64(seed))
    c = max(1, n // 8)
    centres = g.standard_normal((c, d))
    own = g.integers(0, c, n)
    x = (centres[own] + (0.05 + 0.1 * (own % 3))[:, None] * g.standard_normal((n, d))).astype(np.float32)
    if special and n >= 8:
        x[n // 2], x[n - 1], x[3] = x[0], x[1], x[0]
        x[5] = 0.0
    return x


def blob(seed=77, copies=150, near=150, far=150, d=16):
    """``copies`` exact copies of one sample, ``near`` more within 1e-4 of it and ``far`` scattered samples, shuffled:
    among the copies every distance ties, their rank lists fall on the smallest indices and a handful of columns of V2
    is non-zero in every row of the blob."""
    g = np.random.Generator(np.random.PCG64(seed))
    centre = g.standard_normal(d)
    x = np.concatenate((np.tile(centre, (copies, 1)), centre + 1e-4 * g.standard_normal((near, d)),
                        3.0 * g.standard_normal((far, d)))).astype(np.float32)
    return x[g.permutation(copies + near + far)]


def planted(ids=40, per=8, d=64, seed=0):
    """(unit rows [ids * per, d], pids): every identity a direction on the sphere with its own spread (0.15 .. 0.6 of
    the unit noise), so that no single cosine threshold suits all of them; shuffled."""
    g = np.random.Generator(np.random.PCG64(seed))
    centres = g.standard_normal((ids, d))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    pids = np.repeat(np.arange(ids), per)
    spread = (0.15 + 0.45 * g.random(ids))[pids]
    x = centres[pids] + spread[:, None] * g.standard_normal((ids * per, d)) / np.sqrt(d)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    order = g.permutation(ids * per)
    return x[order].astype(np.float32), pids[order]
