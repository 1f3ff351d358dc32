"""Host models of diffusion re-ranking (grl_amd/csrc/diffusion.hip, include/grl_hip.h).

(a) ``mutual`` / ``apply`` / ``solve`` with dtype float32: the kernels' arithmetic in numpy with the kernels' operation
    order.  The device results are held to it bit for bit.
(b) the same functions with dtype float64 and ``dense_solve`` (np.linalg.solve of I - alpha S): what (a) approximates.

  lists    : slot t of row i is position t + (t >= selfpos) of the row's k + 1 search entries, selfpos = the first
             position holding i (k when there is none); an index outside [0, n) or a further entry equal to i is
             padding (-1);
  weight   : s = -dist if dist < 0 else 0 (NaN -> 0); w = s, gamma - 1 times w = w * s (always float32: the weights are
             the graph's inputs);
  mutual   : a[i][t] = min(w_ij, w_ji) if i occurs in row j's list at a position p that row j keeps (the first
             occurrence; kept: j occurs in its own list, or p < k), else 0;
  degree   : deg[i] = a[i][0] + a[i][1] + ... from +0, in slot order;
  S        : a / (sqrt(deg_i) * sqrt(deg_j)), 0 where a is 0;
  product  : acc = +0; per slot with S != 0 in slot order acc = acc + (S * p[j]); Ap = p - (alpha * acc);
  dot      : a wave sums WAVE_ROWS consecutive rows in row order from +0, the WAVES wave sums of a block of PART_ROWS rows
             are added in wave order, the partials are added in row order from +0;
  CG       : x0 = 0, r0 = p0 = y; a = rr / pAp, x = x + (a * p), r = r - (a * Ap), b = rr' / rr, p = r + (b * p); a column
             whose rr is not a positive finite number, or whose pAp is <= 0 or not finite, freezes.
"""
import numpy as np

F32 = np.float32
WAVE_ROWS, WAVES = 16, 4
PART_ROWS = WAVE_ROWS * WAVES

# Largest relative error of model (a) against the dense float64 solve (b), max_i |f32_i - f64_i| / max_i |f64_i| per
# column, measured by ``measure_model_error`` on the host: feature_case(seed, 7, 150) for seeds 0..5, k = 8, kq = 3,
# gamma = 3, n_iter = 150 (the float64 CG of the same code agrees with the dense solve to below 1e-12 there, so the
# iteration has converged and what is left is float32 rounding).  The condition number is at most (1 + alpha) /
# (1 - alpha): 19 and 199, so errors far above 19 * 2^-24 = 1.1e-6 and 199 * 2^-24 = 1.2e-5 would mean a bug.
REL_ERR_ALPHA_090 = 7.6e-07
REL_ERR_ALPHA_099 = 4.0e-06
# The tolerance wherever a float32 result meets float64: 4 x the measured value (inputs beyond the seeds tried).
TOL_ALPHA_090 = 4 * REL_ERR_ALPHA_090
TOL_ALPHA_099 = 4 * REL_ERR_ALPHA_099


def tolerance(alpha):
    """4 x the measured error at the next recorded alpha at or above ``alpha`` (the error grows with alpha)."""
    assert 0.0 <= alpha <= 0.99
    return TOL_ALPHA_090 if alpha <= 0.9 else TOL_ALPHA_099


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def feature_case(seed, nq, ng, d=32, n_ids=12, n_cams=3, noise=0.35):
    """Unit-norm float32 rows of ``n_ids`` planted identities; the first nq gallery rows are the queries (the evaluator
    prepends them).  Returns qf, gf, q_pids, q_cams, g_pids, g_cams."""
    g = np.random.Generator(np.random.PCG64(seed))
    centres = g.standard_normal((n_ids, d))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    pids = g.integers(0, n_ids, ng)
    cams = g.integers(0, n_cams, ng)
    x = centres[pids] + noise * g.standard_normal((ng, d)) / np.sqrt(d) * 3.0
    gf = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)
    gf = (gf / np.linalg.norm(gf, axis=1, keepdims=True).astype(F32)).astype(F32)
    return gf[:nq].copy(), gf, pids[:nq].copy(), cams[:nq].copy(), pids, cams


def manifold_case(d=32):
    """The case diffusion exists for.  Gallery = [the query, a chain c_1 .. c_8 on a great circle that turns away from the
    query by 0.25 rad per step, 12 distractors at cosine 0.3 to the query, each in a dimension of its own].  c_1 .. c_5
    are the query's near tracklets (its pid, its camera: junk for the metric), c_6 .. c_8 its true matches under another
    camera, at cosine 0.07, -0.18 and -0.42 to the query: plain cosine ranks every distractor above them.  With k = 4 the
    chain is connected by mutual edges and no distractor has one.
    Returns qf [1, d], gf [21, d], q_pids, q_cams, g_pids, g_cams, matches (gallery indices), distractors."""
    theta, chain, n_dis = 0.25, 8, 12
    assert d >= 2 + n_dis
    rows = [np.eye(d)[0]]
    for m in range(1, chain + 1):
        v = np.zeros(d)
        v[0], v[1] = np.cos(m * theta), np.sin(m * theta)
        rows.append(v)
    for j in range(n_dis):
        v = np.zeros(d)
        v[0], v[2 + j] = 0.3, np.sqrt(1.0 - 0.09)
        rows.append(v)
    gf = np.asarray(rows).astype(F32)
    g_pids = np.array([1] * (1 + chain) + [2 + j for j in range(n_dis)])
    g_cams = np.array([0] * 6 + [1] * 3 + [1] * n_dis)
    matches = np.arange(6, 9)
    distractors = np.arange(9, 9 + n_dis)
    return gf[:1].copy(), gf, g_pids[:1].copy(), g_cams[:1].copy(), g_pids, g_cams, matches, distractors


def host_search(qf, gf, k):
    """engine.search by cosine on the host, for the tests that have no device: float32 -q.g, ascending, ties to the
    smaller index, padded with (-1, +inf); the dot products are rounded from float64, so the lists do not depend on a
    BLAS's summation order.  (Its bits need not be the GEMM's: the models take the lists as inputs.)"""
    qf, gf = np.asarray(qf, F32), np.asarray(gf, F32)
    dist = -(qf.astype(np.float64) @ gf.astype(np.float64).T).astype(F32)
    dist = dist + F32(0.0)                                       # -0 -> +0
    order = np.argsort(dist, axis=1, kind='stable')[:, :k]
    idx = np.full((qf.shape[0], k), -1, np.int64)
    val = np.full((qf.shape[0], k), np.inf, F32)
    idx[:, :order.shape[1]] = order
    val[:, :order.shape[1]] = np.take_along_axis(dist, order, 1)
    return val, idx


# ---------------------------------------------------------------------------------------------------------------------
# the graph
# ---------------------------------------------------------------------------------------------------------------------
def weight(dist, gamma):
    dist = F32(dist)
    s = F32(-dist) if dist < 0 else F32(0.0)                    # NaN < 0 is False
    w = s
    with np.errstate(all='ignore'):
        for _ in range(gamma - 1):
            w = F32(w * s)
    return w


def _selfpos(row, i, k):
    for p in range(k + 1):
        if int(row[p]) == i:
            return p
    return k


def mutual(sidx, sdist, k, gamma, dtype=F32):
    """idx int32 [n, k], a, deg, S from the k + 1 search entries per row (sidx int64 / sdist float32 [n, >= k + 1]).
    ``a`` is float32 in both models (min of two float32 weights); deg and S are computed in ``dtype``."""
    sidx, sdist = np.asarray(sidx), np.asarray(sdist, F32)
    n = sidx.shape[0]
    assert sidx.shape[1] >= k + 1 and 1 <= k <= 128 and 1 <= gamma <= 8
    idx = np.full((n, k), -1, np.int32)
    w = np.zeros((n, k), F32)
    for i in range(n):
        sp = _selfpos(sidx[i], i, k)
        for t in range(k):
            p = t + (1 if t >= sp else 0)
            j = int(sidx[i, p])
            if 0 <= j < n and j != i:
                idx[i, t] = j
                w[i, t] = weight(sdist[i, p], gamma)
    a = np.zeros((n, k), F32)
    for i in range(n):
        for t in range(k):
            j = int(idx[i, t])
            if j < 0:
                continue
            lj = [int(v) for v in sidx[j, :k + 1]]
            if i not in lj:
                continue
            p = lj.index(i)
            if j in lj or p < k:
                a[i, t] = min(w[i, t], weight(sdist[j, p], gamma))
    deg = np.zeros(n, dtype)
    for t in range(k):
        deg = (deg + a[:, t].astype(dtype)).astype(dtype)
    S = np.zeros((n, k), dtype)
    with np.errstate(all='ignore'):
        for i in range(n):
            for t in range(k):
                if a[i, t] != 0:
                    den = dtype(np.sqrt(deg[i]) * np.sqrt(deg[idx[i, t]]))
                    S[i, t] = dtype(dtype(a[i, t]) / den)
    return idx, a, deg, S


def dense(idx, S):
    """The n x n matrix of an ELL graph (float64)."""
    n, k = idx.shape
    M = np.zeros((n, n))
    for i in range(n):
        for t in range(k):
            if S[i, t] != 0:
                M[i, idx[i, t]] += float(S[i, t])
    return M


def seed_vector(seed_idx, seed_val, n, gamma, dtype=F32):
    """y [n][B]: column q holds seed_val[q][t] (gamma 0) or weight(seed_val[q][t], gamma) at node seed_idx[q][t]."""
    seed_idx = np.asarray(seed_idx)
    B, kq = seed_idx.shape
    y = np.zeros((n, B), dtype)
    for q in range(B):
        for t in range(kq):
            j = int(seed_idx[q, t])
            if 0 <= j < n:
                y[j, q] = F32(seed_val[q][t]) if gamma == 0 else weight(seed_val[q][t], gamma)
    return y


# ---------------------------------------------------------------------------------------------------------------------
# the solver
# ---------------------------------------------------------------------------------------------------------------------
def dot_partials(u, v):
    """[ceil(n / PART_ROWS)][B]: the per-workgroup partial sums of sum_i u[i][b] * v[i][b]."""
    dtype = u.dtype.type
    n, B = u.shape
    nblk = -(-n // PART_ROWS)
    prod = np.zeros((nblk * PART_ROWS, B), dtype)
    with np.errstate(all='ignore'):
        prod[:n] = u * v
        prod = prod.reshape(nblk, WAVES, WAVE_ROWS, B)
        wave = np.zeros((nblk, WAVES, B), dtype)
        for r in range(WAVE_ROWS):
            wave = wave + prod[:, :, r]                          # (a padding row adds +0: no change)
        part = wave[:, 0]
        for w in range(1, WAVES):
            part = part + wave[:, w]
    return part


def finish(part):
    total = np.zeros(part.shape[1], part.dtype)
    with np.errstate(all='ignore'):
        for g in range(part.shape[0]):
            total = total + part[g]
    return total


def apply(idx, S, p, alpha):
    """(Ap [n][B], the partials of p . Ap) in p's dtype."""
    dtype = p.dtype.type
    n, k = idx.shape
    S = S.astype(dtype)
    acc = np.zeros_like(p)
    with np.errstate(all='ignore'):
        for t in range(k):
            m = (S[:, t] != 0) & (idx[:, t] >= 0) & (idx[:, t] < n)
            if m.any():
                acc[m] = acc[m] + S[m, t][:, None] * p[idx[m, t]]
        Ap = p - dtype(alpha) * acc
    return Ap, dot_partials(p, Ap)


def solve(idx, S, y, alpha, n_iter):
    """x [n][B] after exactly n_iter iterations of the kernels' conjugate gradients, in y's dtype."""
    dtype = y.dtype.type
    x = np.zeros_like(y)
    if n_iter == 0:
        return x
    r, p = y.copy(), y.copy()
    rr = finish(dot_partials(r, r))
    frozen = np.zeros(y.shape[1], bool)
    with np.errstate(all='ignore'):
        for it in range(n_iter):
            Ap, part = apply(idx, S, p, alpha)
            pAp = finish(part)
            frozen |= ~(rr > 0) | ~(rr < np.inf) | ~(pAp > 0) | ~(pAp < np.inf)
            live = ~frozen
            a = np.where(live, rr / np.where(live, pAp, dtype(1)), dtype(0)).astype(dtype)
            x[:, live] = x[:, live] + a[live] * p[:, live]
            r[:, live] = r[:, live] - a[live] * Ap[:, live]
            if it + 1 == n_iter:
                break
            new = finish(dot_partials(r, r))
            b = np.where(live, new / np.where(live, rr, dtype(1)), dtype(0)).astype(dtype)
            rr = new
            p[:, live] = r[:, live] + b[live] * p[:, live]
    return x


def dense_solve(idx, S, y, alpha):
    """Yardstick (b): f = (I - alpha S)^-1 y in float64 by LAPACK."""
    M = dense(idx, S)
    return np.linalg.solve(np.eye(idx.shape[0]) - float(alpha) * M, np.asarray(y, np.float64))


def rank(f):
    """Gallery order per query for scores f [nq][n]: -f ascending, ties to the smaller index."""
    return np.argsort(-np.asarray(f) + 0.0, axis=1, kind='stable')


def diffuse(qf, gf, k, kq, gamma, alpha, n_iter, dtype=F32, dense_yardstick=False):
    """f [nq][n] of the whole definition on the host lists of ``host_search``."""
    sdist, sidx = host_search(gf, gf, k + 1)
    idx, a, deg, S = mutual(sidx, sdist, k, gamma, dtype)
    qdist, qidx = host_search(qf, gf, kq)
    y = seed_vector(qidx, qdist, gf.shape[0], gamma, dtype)
    if dense_yardstick:
        return dense_solve(idx, S, y, alpha).T
    return solve(idx, S, y, alpha, n_iter).T


def relative_error(f32, f64):
    """Largest over the columns (queries) of max_i |f32_i - f64_i| / max_i |f64_i|."""
    f32, f64 = np.asarray(f32, np.float64), np.asarray(f64, np.float64)
    scale = np.abs(f64).max(axis=1)
    err = np.abs(f32 - f64).max(axis=1)
    return float((err[scale > 0] / scale[scale > 0]).max())


def measure_model_error(alpha, seeds=range(6), nq=7, ng=150, k=8, kq=3, gamma=3, n_iter=150):
    """How REL_ERR_ALPHA_* were obtained: (largest error of (a), largest disagreement of the float64 CG with the dense
    solve) over the seeds."""
    worst, cg = 0.0, 0.0
    for seed in seeds:
        qf, gf = feature_case(seed, nq, ng)[:2]
        ref = diffuse(qf, gf, k, kq, gamma, alpha, n_iter, np.float64, dense_yardstick=True)
        worst = max(worst, relative_error(diffuse(qf, gf, k, kq, gamma, alpha, n_iter, F32), ref))
        cg = max(cg, relative_error(diffuse(qf, gf, k, kq, gamma, alpha, n_iter, np.float64), ref))
    return worst, cg


def ranking_differences(ours, ref_order, ref_f, tol):
    """tests/ranking_check.py's rule for two rankings of scores: (positions that differ, the largest gap in the
    yardstick's scores between the entry we put at a position and the entry the yardstick put there, relative to the
    row's largest score).  A difference is admissible when that gap is below ``tol``."""
    ours, ref_order = np.asarray(ours).astype(np.int64), np.asarray(ref_order).astype(np.int64)
    nq, n = ref_order.shape
    assert ours.shape == (nq, n)
    assert np.array_equal(np.sort(ours, axis=1), np.broadcast_to(np.arange(n), (nq, n))), 'not a permutation'
    diff = ours != ref_order
    scale = np.abs(ref_f).max(axis=1, keepdims=True)
    scale[scale == 0] = 1.0
    gap = np.abs(np.take_along_axis(ref_f, ours, 1) - np.take_along_axis(ref_f, ref_order, 1)) / scale
    return int(diff.sum()), float(gap[diff].max()) if diff.any() else 0.0
