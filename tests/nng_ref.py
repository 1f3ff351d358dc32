"""Host model (numpy, plain loops) of the kNN-graph index contract of DESIGN.md 4af / include/grl_hip.h: the graph
optimisation of engine.nng_optimize (integers, exact) and the beam search of engine.nng_search.  The pair distance is
refine_ref.pair_dist on the store VALUES, the order search_ref's sort_key / composite; neither is copied here."""
import numpy as np

import refine_ref as F
from search_ref import sort_key, composite

K_MAX, D_MAX, L_MIN, L_MAX, W_MAX, WD_MAX = 128, 64, 8, 512, 8, 256
LDS_MAX = 65536


# ----------------------------------------------------------------------------
# graph optimisation
# ----------------------------------------------------------------------------
def live_positions(knn, i):
    """the live positions of row i: not i itself, 0 <= id < n, the first position of every id"""
    n = knn.shape[0]
    seen, out = set(), []
    for b, v in enumerate(knn[i]):
        v = int(v)
        if v == i or not 0 <= v < n or v in seen:
            continue
        seen.add(v)
        out.append(b)
    return out


def detours(knn):
    """det int64 [n, K]: the rank-based 2-hop counts; -1 at a padding position"""
    knn = np.asarray(knn).astype(np.int64)
    n, K = knn.shape
    live = [live_positions(knn, i) for i in range(n)]
    det = np.full((n, K), -1, np.int64)
    for i in range(n):
        for b in live[i]:
            tb, c = knn[i, b], 0
            for a in live[i]:
                if a >= b:
                    break
                ta = knn[i, a]
                for r in live[ta]:
                    if r >= b:
                        break
                    if knn[ta, r] == tb:
                        c += 1
                        break
            det[i, b] = c
    return det


def detours_fast(knn):
    """``detours`` with the membership test answered from a table of first live positions (an n x n array: the model may,
    the product may not); the CPU test holds it to the loops above"""
    knn = np.asarray(knn).astype(np.int64)
    n, K = knn.shape
    live = [live_positions(knn, i) for i in range(n)]
    first = np.full((n, n), K, np.int64)                    # first[t, v]: the live position of id v in row t, K if absent
    for t in range(n):
        lp = np.array(live[t], np.int64)
        first[t, knn[t, lp]] = lp
    det = np.full((n, K), -1, np.int64)
    for i in range(n):
        lp = np.array(live[i], np.int64)
        if lp.size == 0:
            continue
        t = knn[i, lp]
        hit = first[t[:, None], t[None, :]] < lp[None, :]     # [a, b]: t_b stands in row t_a before position b
        det[i, lp] = np.triu(hit, 1).sum(0)
    return det


def forward(knn, det, D):
    """F int64 [n, D]: the ids at the first D live positions of every row in the order (det, b), padded with -1"""
    knn = np.asarray(knn).astype(np.int64)
    n = knn.shape[0]
    out = np.full((n, D), -1, np.int64)
    for i in range(n):
        pos = sorted((int(det[i, b]), b) for b in live_positions(knn, i))[:D]
        for c, (_, b) in enumerate(pos):
            out[i, c] = knn[i, b]
    return out


def reverse(fwd):
    """rev: list of n lists; rev[j] = every i with j in F[i], ordered by (position of j in F[i], i)"""
    n, D = fwd.shape
    rev = [[] for _ in range(n)]
    for p in range(D):
        for i in range(n):
            j = int(fwd[i, p])
            if j >= 0:
                rev[j].append(i)
    return rev


def merge(fwd, rev):
    n, D = fwd.shape
    out = np.full((n, D), -1, np.int64)
    for i in range(n):
        got = []

        def push(v):
            if v >= 0 and v not in got and len(got) < D:
                got.append(v)
                return True
            return False
        for v in fwd[i, :D // 2]:
            push(int(v))
        r, taken = 0, 0
        while r < len(rev[i]) and taken < D // 2:
            taken += push(rev[i][r])
            r += 1
        for v in fwd[i, D // 2:]:
            push(int(v))
        for v in rev[i][r:]:
            push(v)
        out[i, :len(got)] = got
    return out


def optimize(knn, D, fast=False):
    """N int64 [n, D] of the candidate lists knn [n, K]"""
    knn = np.asarray(knn).astype(np.int64)
    K = knn.shape[1]
    if not 2 <= K <= K_MAX or D % 2 or not 2 <= D <= min(K, D_MAX):
        raise ValueError('K, D')
    fwd = forward(knn, (detours_fast if fast else detours)(knn), D)
    return merge(fwd, reverse(fwd))


# ----------------------------------------------------------------------------
# beam search
# ----------------------------------------------------------------------------
def default_seeds(n, L):
    """the seeds of seeds=None: S = min(L, n) ids floor(j * n / S)"""
    S = min(L, n)
    return np.array([(j * n) // S for j in range(S)], np.int64)


def table_slots(n, D, w, T, S):
    ids = min(S + T * w * D, n)
    h = 64
    while h < 2 * ids:
        h *= 2
    return h


def lds_bytes(n, d, D, L, w, T, S):
    P = 8
    while P < L + w * D:
        P *= 2
    W = (max(S, w * D) + 3) // 4 * 4
    return 4 * d + 8 * P + 4 * table_slots(n, D, w, T, S) + 4 * W + 64


def _ckey(dist, ids):
    return composite(sort_key(np.asarray(dist, np.float32)), np.asarray(ids, np.int64))


def search_one(q, rows, nbr, seeds, L, w, T, metric='cosine'):
    """(dist [L] float32, idx [L] int64, visited, iterations) of one query row q [d]"""
    n, D = nbr.shape
    visited = set()
    C = []                                                  # (composite, dist, id, expanded)

    def score(ids):
        if not ids:
            return []
        ids = np.asarray(ids, np.int64)
        dd = F.pair_dist(np.broadcast_to(q, (ids.size, q.size)), rows[ids], metric)
        ck = _ckey(dd, ids)
        return [[int(ck[j]), dd[j], int(ids[j]), False] for j in range(ids.size)]
    first = []
    for s in seeds:
        s = int(s)
        if 0 <= s < n and s not in visited:
            visited.add(s)
            first.append(s)
    C = sorted(score(first), key=lambda e: e[0])[:L]
    iters = 0
    for _ in range(T):
        P = [e for e in C if not e[3]][:w]
        if not P:
            break
        iters += 1
        new = []
        for e in P:
            e[3] = True
        for e in P:
            for v in nbr[e[2]]:
                v = int(v)
                if 0 <= v < n and v not in visited:
                    visited.add(v)
                    new.append(v)
        C = sorted(C + score(new), key=lambda e: e[0])[:L]
    dist = np.full(L, np.inf, np.float32)
    idx = np.full(L, -1, np.int64)
    for j, e in enumerate(C):
        dist[j], idx[j] = e[1], e[2]
    return dist, idx, len(visited), iters


def search(qf, rows, nbr, seeds, L, w=1, T=64, metric='cosine'):
    """(dist [nq, L], idx [nq, L] int64, stats [nq, 2]); seeds [S] (shared) or [nq, S]"""
    qf, rows = np.asarray(qf, np.float32), np.asarray(rows, np.float32)
    nbr, seeds = np.asarray(nbr).astype(np.int64), np.asarray(seeds).astype(np.int64)
    nq = qf.shape[0]
    dist = np.full((nq, L), np.inf, np.float32)
    idx = np.full((nq, L), -1, np.int64)
    stats = np.zeros((nq, 2), np.int64)
    for r in range(nq):
        s = seeds if seeds.ndim == 1 else seeds[r]
        dist[r], idx[r], stats[r, 0], stats[r, 1] = search_one(qf[r], rows, nbr, s, L, w, T, metric)
    return dist, idx, stats


def finish(dist, idx, k, junk=None):
    """the first k entries of the L-lists that are live and not junk (junk [nq, L] bool or None), padded with +inf / -1"""
    nq = dist.shape[0]
    od = np.full((nq, k), np.inf, np.float32)
    oi = np.full((nq, k), -1, np.int64)
    for r in range(nq):
        keep = idx[r] >= 0
        if junk is not None:
            keep &= ~junk[r]
        j = np.flatnonzero(keep)[:k]
        od[r, :j.size], oi[r, :j.size] = dist[r, j], idx[r, j]
    return od, oi


def junk_mask(idx, exclude):
    """[nq, L] bool: the entries that share the query's pid and camera"""
    q_pids, g_pids, q_cams, g_cams = (np.asarray(a) for a in exclude)
    safe = np.where(idx >= 0, idx, 0)
    return (idx >= 0) & (g_pids[safe] == q_pids[:, None]) & (g_cams[safe] == q_cams[:, None])


# ----------------------------------------------------------------------------
# GRL_EVAL_NNG
# ----------------------------------------------------------------------------
def parse_knob_cases():
    """(good, bad) values of GRL_EVAL_NNG shared by the CPU test: (K, D, L, w, T, dtype)"""
    good = {'64,32': (64, 32, 64, 1, 64, 'f32'), ' 16 , 8 , 32 ': (16, 8, 32, 1, 64, 'f32'), '8,8,8,2': (8, 8, 8, 2, 64, 'f32'),
            '128,64,512,4,7': (128, 64, 512, 4, 7, 'f32'), '32,16,64,1,64,bf16': (32, 16, 64, 1, 64, 'bf16'),
            '2,2,8,8,1,f32': (2, 2, 8, 8, 1, 'f32')}
    bad = ('x', '64', '64,', '1,2', '129,32', '64,33', '64,66', '8,16', '64,32,48', '64,32,4', '64,32,1024', '64,32,64,0',
           '64,32,64,9', '64,64,64,8', '64,32,64,1,0', '64,32,64,1,64,fp16', '64,32,64,1,64,bf16,1', '64;32', '6.5,2',
           '64,32,,1', '64,32,bf16')
    return good, bad
