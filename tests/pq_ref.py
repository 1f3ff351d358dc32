"""Host model (numpy) of the product-quantisation contract of DESIGN.md 4ac / include/grl_hip.h: engine.PqCodebook,
pq_dist, pq_search, topk_recall.

The ADC sum works on float32 tables somebody else computed (the device's own downloaded tables in the GPU tests, numpy
ones in the CPU tests), so every distance is derived from given bits: four partials, p_w the sequential float32 sum from
+0 of lut[q, m, c_m] over m = w, w + 4, .. ascending, joined as (p0 + p1) + (p2 + p3); adds only."""
import numpy as np

from search_ref import sort_key, composite

F32 = np.float32


def sub(m, dsub):
    return slice(m * dsub, (m + 1) * dsub)


def adc_sum(lut, codes):
    """S [nq, n] float32 of tables lut [nq, M, ksub] float32 and codes [n, M] (any integer type)."""
    lut = np.asarray(lut, dtype=F32)
    codes = np.asarray(codes).astype(np.int64)
    nq, M = lut.shape[0], lut.shape[1]
    n = codes.shape[0]
    p = np.zeros((4, nq, n), dtype=F32)
    with np.errstate(all='ignore'):
        for m in range(M):
            p[m & 3] = p[m & 3] + lut[:, m, :][:, codes[:, m]]
        return ((p[0] + p[1]) + (p[2] + p[3])).astype(F32)


def adc_dist(lut, codes, metric='cosine', rn=None):
    """'cosine': S.  'euclidean': sqrt(max(rn[q] + S, 1e-12)) in float32, a NaN argument giving 1e-12."""
    s = adc_sum(lut, codes)
    if metric == 'cosine':
        return s
    if metric != 'euclidean':
        raise ValueError(metric)
    with np.errstate(all='ignore'):
        t = (np.asarray(rn, dtype=F32)[:, None] + s).astype(F32)
        t = np.where(t > F32(1e-12), t, F32(1e-12)).astype(F32)           # (a NaN fails the comparison)
        return np.sqrt(t, dtype=F32)


def encode(x, codebooks, dist):
    """codes uint8 [n, M]: per subspace the smallest key of dist(x[:, sub(m)], C[m]) -> D [n, ksub] float32, ties to the
    smaller centroid index (kmeans_ref.assign's rule)."""
    import kmeans_ref
    x = np.asarray(x, dtype=F32)
    M, ksub, dsub = codebooks.shape
    codes = np.zeros((x.shape[0], M), dtype=np.uint8)
    for m in range(M):
        lab, _ = kmeans_ref.assign(dist(np.ascontiguousarray(x[:, sub(m, dsub)]), codebooks[m]))
        assert (lab >= 0).all()
        codes[:, m] = lab
    return codes


def decode(codes, codebooks):
    """x [n, d] float32: x[i, sub(m)] = C[m, codes[i, m]]."""
    codes = np.asarray(codes).astype(np.int64)
    M, ksub, dsub = codebooks.shape
    if codes.size and codes.max() >= ksub:
        raise ValueError('a code >= ksub')
    return np.concatenate([np.asarray(codebooks, dtype=F32)[m][codes[:, m]] for m in range(M)], axis=1)


def search(D, k, junk=None):
    """(dist [nq, k] float32, idx [nq, k] int64): ascending composite (sort key, gallery index) of every row of D, the
    entries of ``junk`` [nq, ng] bool deleted, truncated to k, padded with index -1 / distance +inf."""
    D = np.asarray(D, dtype=F32)
    nq, ng = D.shape
    idx = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), np.inf, F32)
    for q in range(nq):
        o = np.argsort(composite(sort_key(D[q]), np.arange(ng)), kind='stable')
        if junk is not None:
            o = o[~np.asarray(junk[q], bool)[o]]
        o = o[:k]
        idx[q, :o.size] = o
        dist[q, :o.size] = D[q, o]
    return dist, idx


def recall(approx_idx, exact_idx, ks):
    """Per k: the mean over the queries of |approx[:k] & exact[:k]| / #valid(exact[:k]); -1 is padding; a query without a
    valid exact entry is left out."""
    a, e = np.asarray(approx_idx), np.asarray(exact_idx)
    out = []
    for k in ks:
        part = []
        for ra, re_ in zip(a[:, :k], e[:, :k]):
            valid = set(int(v) for v in re_ if v >= 0)
            if valid:
                part.append(len(valid & set(int(v) for v in ra if v >= 0)) / float(len(valid)))
        out.append(float(np.mean(part)) if part else float('nan'))
    return out


# ---- the planted quality case shared by tests/test_pq_cpu.py (decided there) and tests/test_gpu_pq.py ----
PLANTED = dict(n_ids=10, nq=60, ng=300, d=256, M=8, nbits=4, noise=0.05, seed=0, train_seed=0, max_iter=25)


def planted_case():
    """(qf [60, 256], gf [300, 256], q_pids, g_pids): unit rows around 10 random dense unit directions plus
    0.05 * N(0, 1) per column, renormalised; identity i owns every row with index % 10 == i."""
    c = PLANTED
    rng = np.random.Generator(np.random.PCG64(c['seed']))
    dirs = rng.standard_normal((c['n_ids'], c['d']))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)

    def rows(n):
        pids = np.arange(n) % c['n_ids']
        x = dirs[pids] + c['noise'] * rng.standard_normal((n, c['d']))
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32), pids.astype(np.int64)
    qf, q_pids = rows(c['nq'])
    gf, g_pids = rows(c['ng'])
    return qf, gf, q_pids, g_pids


def train(x, M, nbits, seed=0, max_iter=25):
    """pq_train's rule on the host: subspace m = kmeans_ref.kmeans(x[:, sub(m)], 2**nbits, 'euclidean', 'random',
    seed + m, max_iter)['centroids'] with numpy distance matrices."""
    import kmeans_ref
    x = np.asarray(x, dtype=F32)
    dsub = x.shape[1] // M
    return np.stack([kmeans_ref.kmeans(np.ascontiguousarray(x[:, sub(m, dsub)]), 1 << nbits, 'euclidean', 'random',
                                       seed + m, max_iter)['centroids'] for m in range(M)]).astype(F32)


def lut_host(q, codebooks, metric='cosine'):
    """numpy tables [nq, M, ksub] float32 (their own bits, not the device GEMM's): -q_m . C[m]^T, or cn + 2 * that."""
    q = np.asarray(q, dtype=F32)
    M, ksub, dsub = codebooks.shape
    g = np.stack([negdot(q[:, sub(m, dsub)], codebooks[m]) for m in range(M)], axis=1)
    if metric == 'cosine':
        return g
    cn = (codebooks.astype(F32) ** 2).sum(2, dtype=F32)
    return (cn[None] + F32(2) * g).astype(F32)


def negdot(a, b):
    return (-(np.asarray(a, dtype=F32) @ np.asarray(b, dtype=F32).T)).astype(F32)


def euclid(x, c):
    """pairwise_distance_tensor's form in numpy float32, with the device's clamp: a NaN argument gives 1e-12 (numpy's
    maximum would keep the NaN)."""
    x, c = np.asarray(x, dtype=F32), np.asarray(c, dtype=F32)
    with np.errstate(all='ignore'):
        d2 = (x * x).sum(1)[:, None] + (c * c).sum(1)[None, :] - F32(2) * (x @ c.T)
        return np.sqrt(np.where(d2 > F32(1e-12), d2, F32(1e-12)).astype(F32), dtype=F32)
