"""Host model (numpy) of the IVF-PQ contract of DESIGN.md 4ad / include/grl_hip.h: engine.IvfPqCodebook, IvfPqIndex,
ivf_dist, ivf_search, ivf_probe_stats.  Built on tests/pq_ref.py, whose notation it keeps.

Like pq_ref it works on float32 numbers somebody else computed (the device's own downloaded G0, tables, xn and rn in the
GPU tests, numpy ones in the CPU tests), so every distance is derived from given bits.  A candidate of query q is a gallery
row i whose list lab_i is one of q's probes; g0[q, j] = G0[q, probe[q, j]] is then simply G0[q, lab_i]:

  t = G0[q, lab_i] + S[q, i]                     S = pq_ref.adc_sum over the residual codes (four partials, adds only)
  'cosine':    dist = t
  'euclidean': u = xn[i] + 2 * t (exact multiply), w = rn[q] + u, dist = sqrt(w > 1e-12 ? w : 1e-12)

All arrays here are in GALLERY order; ``lists`` gives the list order the index stores."""
import numpy as np

import pq_ref as R

F32 = np.float32


def lists(labels, nlist):
    """(list_ptr int64 [nlist + 1], ids int32 [n]): the rows grouped by list, ascending gallery index inside a list."""
    labels = np.asarray(labels).astype(np.int64)
    if labels.size and (labels.min() < 0 or labels.max() >= nlist):
        raise ValueError('a label outside 0..nlist-1')
    ids = np.argsort(labels, kind='stable').astype(np.int32)
    ptr = np.zeros(nlist + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(labels, minlength=nlist))
    return ptr, ids


def residual(x, coarse, labels):
    """r[i][c] = x[i][c] - coarse[lab_i][c], one rounded float32 subtraction."""
    with np.errstate(all='ignore'):
        return (np.asarray(x, dtype=F32) - np.asarray(coarse, dtype=F32)[np.asarray(labels).astype(np.int64)]).astype(F32)


def reconstruct(coarse, labels, codes, codebooks):
    """x^[i][sub(m)] = coarse[lab_i][sub(m)] + R[m][code[i, m]], one rounded float32 add."""
    with np.errstate(all='ignore'):
        return (np.asarray(coarse, dtype=F32)[np.asarray(labels).astype(np.int64)] + R.decode(codes, codebooks)).astype(F32)


def sqnorm(x):
    """a float32 row norm of the host's own (the GPU tests download the device's grl_row_sqnorm instead)"""
    x = np.asarray(x, dtype=F32)
    return (x * x).sum(1, dtype=F32)


def probes(Dc, nprobe):
    """probe int64 [nq, nprobe]: the index list of search over Dc [nq, nlist], the metric's distances of the queries to
    the coarse centroids; ties to the smaller list, NaN last."""
    return R.search(Dc, nprobe)[1]


def candidates(labels, probe):
    """cand bool [nq, n]: row i is in one of q's probed lists"""
    labels = np.asarray(labels).astype(np.int64)
    return np.stack([np.isin(labels, p) for p in np.asarray(probe)]) if len(probe) else np.zeros((0, labels.size), bool)


def dist(lut, codes, labels, G0, metric='cosine', xn=None, rn=None):
    """D [nq, n] float32 in gallery order for EVERY pair (the caller masks it by ``candidates``)."""
    labels = np.asarray(labels).astype(np.int64)
    s = R.adc_sum(lut, codes)
    with np.errstate(all='ignore'):
        t = (np.asarray(G0, dtype=F32)[:, labels] + s).astype(F32)
        if metric == 'cosine':
            return t
        if metric != 'euclidean':
            raise ValueError(metric)
        u = (np.asarray(xn, dtype=F32)[None, :] + F32(2) * t).astype(F32)
        w = (np.asarray(rn, dtype=F32)[:, None] + u).astype(F32)
        w = np.where(w > F32(1e-12), w, F32(1e-12)).astype(F32)                # (a NaN fails the comparison)
        return np.sqrt(w, dtype=F32)


def search(D, cand, k, junk=None):
    """pq_ref.search over the candidates only: everything outside ``cand`` is deleted like junk."""
    drop = ~np.asarray(cand, bool)
    if junk is not None:
        drop = drop | np.asarray(junk, bool)
    return R.search(D, k, drop)


def probe_stats(list_ptr, probe):
    lens = np.diff(np.asarray(list_ptr, dtype=np.int64))
    return lens[np.asarray(probe).astype(np.int64)].sum(1)


def train(x, nlist, M, nbits, seed=0, max_iter=25):
    """ivf_train's rule on the host with numpy distance matrices: (coarse, labels, codebooks)."""
    import kmeans_ref
    x = np.asarray(x, dtype=F32)
    coarse = kmeans_ref.kmeans(x, nlist, 'euclidean', 'random', seed, max_iter)['centroids'].astype(F32)
    lab = assign(x, coarse)
    return coarse, lab, R.train(residual(x, coarse, lab), M, nbits, seed + 1, max_iter)


def assign(x, coarse):
    import kmeans_ref
    lab, _ = kmeans_ref.assign(R.euclid(x, coarse))
    return lab.astype(np.int64)


def host_case(q, x, coarse, codebooks, metric):
    """Everything ``dist`` needs, computed by numpy alone: (labels, codes, lut, G0, Dc, xn, rn)."""
    lab = assign(x, coarse)
    codes = R.encode(residual(x, coarse, lab), codebooks, R.euclid)
    G0 = R.negdot(q, coarse)
    Dc = G0 if metric == 'cosine' else R.euclid(q, coarse)
    xn = sqnorm(reconstruct(coarse, lab, codes, codebooks))
    return lab, codes, R.lut_host(q, codebooks, 'cosine'), G0, Dc, xn, sqnorm(q)
