"""numpy models of the tracklet set distances (include/grl_hip.h, "tracklet set distances").  Not collected.

``cell`` / ``set_dist_from_matrix`` are the header's contract in float32, in the kernel's summation order: what
grl_setdist_block must give bit for bit from the same clip distances.  ``brute`` is the table of the definition in
float64, written as plain loops, with no thought for order or speed."""
import numpy as np

REDUCES = ('min', 'mean', 'chamfer', 'hausdorff')
CANONICAL_NAN = np.array([0x7fc00000], dtype=np.uint32).view(np.float32)[0]


def _key(x):
    """order-preserving uint32 image of float32 values that are not NaN: -0 below +0"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def _unkey(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def _seq_sum(x):
    """sequential float32 sum from +0.0f in ascending index"""
    return np.cumsum(np.concatenate([np.zeros(1, np.float32), np.asarray(x, np.float32)]), dtype=np.float32)[-1]


def _mean_sum(e):
    """the 64 lane partials and the halving tree of GRL_SET_MEAN"""
    m, p = e.shape
    W = 64
    if p <= 32:
        W = 1
        while W < p:
            W *= 2
    R = 64 // W
    steps = -(-m // R)
    pieces = []
    for cb in range(0, p, 64):
        w = min(64, p - cb)
        a = np.zeros((steps * R, W), np.float32)          # (adding +0.0f never changes a partial: none can be -0)
        a[:m, :w] = e[:, cb:cb + w]
        pieces.append(a.reshape(steps, R * W))             # lane = (i % R) * W + j % 64, step = i // R
    part = np.cumsum(np.concatenate([np.zeros((1, 64), np.float32)] + pieces, 0), axis=0, dtype=np.float32)[-1].copy()
    s = 32
    while s:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return part[0]


def cell(e, reduce):
    """One m x p cell of float32 clip distances -> the float32 set distance."""
    e = np.ascontiguousarray(e, dtype=np.float32)
    m, p = e.shape
    assert m >= 1 and p >= 1 and reduce in REDUCES
    with np.errstate(invalid='ignore', over='ignore'):
        if reduce == 'mean':
            r = np.float32(_mean_sum(e) / np.float32(m * p))
            return CANONICAL_NAN if r != r else r
        if np.isnan(e).any():
            return CANONICAL_NAN
        k = _key(e)
        rowmin, colmin = k.min(axis=1), k.min(axis=0)
        if reduce == 'min':
            return _unkey(rowmin.min())[()]
        if reduce == 'hausdorff':
            return _unkey(max(rowmin.max(), colmin.max()))[()]
        sr, sc = _seq_sum(_unkey(rowmin)), _seq_sum(_unkey(colmin))
        r = np.float32(0.5) * (np.float32(sr / np.float32(m)) + np.float32(sc / np.float32(p)))
        r = np.float32(r)
        return CANONICAL_NAN if r != r else r


def set_dist_from_matrix(E, qptr, gptr, reduce):
    """[nq, ng] float32 set distances from the clip matrix E [qptr[-1], gptr[-1]] (float32)."""
    E = np.asarray(E, dtype=np.float32)
    nq, ng = len(qptr) - 1, len(gptr) - 1
    out = np.empty((nq, ng), np.float32)
    for a in range(nq):
        for b in range(ng):
            out[a, b] = cell(E[qptr[a]:qptr[a + 1], gptr[b]:gptr[b + 1]], reduce)
    return out


def clip_matrix64(qc, gc, metric):
    """the float64 clip distances of the evaluator's two metrics (attevaluator.py:33-46)"""
    qc, gc = np.asarray(qc, np.float64), np.asarray(gc, np.float64)
    if metric == 'cosine':
        return -(qc @ gc.T)
    assert metric == 'euclidean'
    d2 = (qc * qc).sum(1)[:, None] + (gc * gc).sum(1)[None, :] - 2.0 * (qc @ gc.T)
    return np.sqrt(np.maximum(d2, 1e-12))


def brute(qc, gc, qptr, gptr, reduce, metric, E=None):
    """The definition in float64, plain loops.  ``E``: take these clip distances (any dtype, used as float64) instead
    of computing them from the clip rows."""
    E = clip_matrix64(qc, gc, metric) if E is None else np.asarray(E, np.float64)
    nq, ng = len(qptr) - 1, len(gptr) - 1
    out = np.empty((nq, ng), np.float64)
    for a in range(nq):
        for b in range(ng):
            rows, cols = range(qptr[a], qptr[a + 1]), range(gptr[b], gptr[b + 1])
            m, p = len(rows), len(cols)
            rowmin = [min(float(E[i, j]) for j in cols) for i in rows]
            colmin = [min(float(E[i, j]) for i in rows) for j in cols]
            if reduce == 'min':
                v = min(rowmin)
            elif reduce == 'hausdorff':
                v = max(max(rowmin), max(colmin))
            elif reduce == 'chamfer':
                v = 0.5 * (sum(rowmin) / m + sum(colmin) / p)
            else:
                assert reduce == 'mean'
                v = sum(float(E[i, j]) for i in rows for j in cols) / (m * p)
            out[a, b] = v
    return out
