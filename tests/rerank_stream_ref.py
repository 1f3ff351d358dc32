"""numpy model of the streaming k-reciprocal re-ranking of grl_amd/csrc/rerank_stream.hip (engine.rerank_search /
engine.rerank_metrics_streaming).  It never forms D or V: D rows come from column blocks of the stacked
distance matrix S = [[qq, qg], [qg^T, gg]], each row keeps its first K = max(k1+1, k2) neighbours, the weights
are gathered D values of each sample's expanded list, V2 is a sparse row per sample and the Jaccard sums run
over the query's non-zero k in ascending order against an inverted index of the gallery rows."""
import numpy as np

LMAX = 256


def half_of(k1):
    """int(np.around(k1 / 2.)): round half to even."""
    h = k1 // 2
    if k1 % 2 == 1 and h % 2 == 1:
        h += 1
    return h


def spans(n, width):
    return [(i, min(i + width, n)) for i in range(0, n, width)]


class Stack(object):
    """Columns of S^2 (float32) from the three blocks, as the segments of the device path read them."""

    def __init__(self, q_g, q_q, g_g):
        self.qg, self.qq, self.gg = (np.asarray(a, np.float32) for a in (q_g, q_q, g_g))
        self.nq, self.ng = self.qg.shape
        self.N = self.nq + self.ng

    def columns(self, i0, i1):
        """S[:, i0:i1] squared, [N][i1-i0]."""
        nq = self.nq
        cols = []
        for i in range(i0, i1):
            if i < nq:
                c = np.concatenate([self.qq[:, i], self.qg[i, :]])
            else:
                c = np.concatenate([self.qg[:, i - nq], self.gg[:, i - nq]])
            cols.append(c)
        s = np.stack(cols, 1).astype(np.float32)
        return s * s


def rank_lists(st, K, width):
    """colmax [N] and the first K entries of every D row (stable ascending order), one sample block at a time."""
    colmax = np.empty(st.N, np.float32)
    rank = np.empty((st.N, K), np.int32)
    for i0, i1 in spans(st.N, width):
        s = st.columns(i0, i1)
        cm = s.max(axis=0)
        colmax[i0:i1] = cm
        drows = (s / cm[None, :]).T                          # D[i][j] = S[j][i]^2 / colmax[i]
        rank[i0:i1] = np.argsort(drows, axis=1, kind='stable')[:, :K]
    return colmax, rank


def _k_reciprocal(rank, i, k):
    fwd = rank[i, :k + 1]
    back = rank[fwd, :k + 1]
    return fwd[np.where(back == i)[0]]


def expansion_lists(rank, k1):
    half = half_of(k1)
    lists = []
    for i in range(rank.shape[0]):
        base = _k_reciprocal(rank, i, k1)
        expanded = base
        for cand in base:
            cand_set = _k_reciprocal(rank, cand, half)
            if len(np.intersect1d(cand_set, base)) > 2. / 3 * len(cand_set):
                expanded = np.append(expanded, cand_set)
        lists.append(np.unique(expanded).astype(np.int32))
        assert lists[-1].size <= LMAX
    return lists


def weights(st, colmax, lists, width):
    """V[i][lists[i]] from D values gathered out of the recomputed sample blocks."""
    vals = [None] * st.N
    for i0, i1 in spans(st.N, width):
        s = st.columns(i0, i1)
        for i in range(i0, i1):
            e = lists[i]
            d = s[e, i - i0] / colmax[i]
            w = np.exp(-d)
            vals[i] = (w / np.sum(w)).astype(np.float32)
    return vals


def expand(rank, lists, vals, k2):
    """V2 rows as (sorted columns, float32 values): the union of the k2 nearest samples' lists."""
    N = rank.shape[0]
    out = []
    for i in range(N):
        rows = [i] if k2 == 1 else list(rank[i, :k2])
        cols = np.unique(np.concatenate([lists[r] for r in rows]))
        s = np.zeros(cols.size, np.float32)
        for u, r in enumerate(rows):
            pos = np.searchsorted(lists[r], cols)
            hit = (pos < lists[r].size) & (lists[r][np.minimum(pos, lists[r].size - 1)] == cols)
            term = np.where(hit, vals[r][np.minimum(pos, lists[r].size - 1)], np.float32(0)).astype(np.float32)
            s = term if u == 0 else (s + term).astype(np.float32)
        v = s if k2 == 1 else (s / np.float32(k2)).astype(np.float32)
        nz = v != 0
        out.append((cols[nz].astype(np.int32), v[nz]))
    return out


def final(st, colmax, v2, lam, block_cols):
    """F [nq][ng] block by block: Jaccard over the query's non-zero k (ascending) against the CSC of the gallery
    rows, then (1 - lambda) * jaccard + lambda * D."""
    nq, ng, N = st.nq, st.ng, st.N
    csc = [[] for _ in range(N)]
    for j in range(nq, N):                                   # ascending j within every column
        for k, v in zip(*v2[j]):
            csc[k].append((j, v))
    csc = [(np.array([j for j, _ in c], np.int64), np.array([v for _, v in c], np.float32)) for c in csc]
    one_minus = np.float32(1 - lam)
    lam32 = np.float32(lam)
    F = np.empty((nq, ng), np.float32)
    for c0, c1 in spans(ng, block_cols):
        for q in range(nq):
            acc = np.zeros(c1 - c0, np.float32)
            for k, vk in zip(*v2[q]):
                rows, vals = csc[k]
                sel = (rows >= nq + c0) & (rows < nq + c1)
                idx = rows[sel] - (nq + c0)
                acc[idx] = acc[idx] + np.minimum(vk, vals[sel])
            x = st.qg[q, c0:c1]
            d = (x * x) / colmax[q]
            jac = np.float32(1) - acc / (np.float32(2) - acc)
            F[q, c0:c1] = jac * one_minus + d * lam32
    return F


def rerank_stream(q_g, q_q, g_g, k1=20, k2=6, lambda_value=0.3, width=64, block_cols=64):
    st = Stack(q_g, q_q, g_g)
    K = max(k1 + 1, k2)
    colmax, rank = rank_lists(st, K, width)
    lists = expansion_lists(rank, k1)
    vals = weights(st, colmax, lists, width)
    v2 = expand(rank, lists, vals, k2)
    return final(st, colmax, v2, lambda_value, block_cols)
