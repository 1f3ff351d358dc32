"""Host model (numpy) of the refinement contract of DESIGN.md 4ae / include/grl_hip.h: engine.RefineStore, refine_dist,
refine_lists, refine_search.

Pair distance of query row q and store row x (the fp32 widening of what the store holds), per column c: 'cosine'
p_c = fl(q_c * x_c); 'euclidean' e_c = fl(q_c - x_c), p_c = fl(e_c * e_c).  Lane l (0..63) owns the columns
256 t + 4 l + e, e = 0..3: its four partials are the sequential float32 sums from +0 of p_c over t ascending (columns
>= d are skipped -- the model pads with zeros, which adds +0 to a partial that is never -0); v_l = (a0 + a1) + (a2 + a3);
then v_l = v_l + v_{l xor o} for o = 32, 16, 8, 4, 2, 1; S = any lane.  'cosine': -S; 'euclidean': sqrt(S > 1e-12 ? S :
1e-12), a NaN argument giving 1e-12.  A NaN result is 0x7fc00000."""
import numpy as np

from search_ref import sort_key, composite

F32 = np.float32
D_MAX = 16384
LANES = np.arange(64)


def pack_bf16(x):
    """uint16 of float32: round to nearest even on the upper 16 bits, every NaN -> 0x7fc0, +-inf and +-0 kept, a finite
    value beyond the bf16 range -> inf."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7fff) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    r[(u & np.uint64(0x7fffffff)) > np.uint64(0x7f800000)] = 0x7fc0
    return r


def widen(b):
    """float32 of bf16 bit patterns (exact)."""
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(F32)


def store_rows(x, dtype='f32'):
    """the VALUES a RefineStore of ``x`` holds: x itself, or widen(pack_bf16(x))"""
    x = np.ascontiguousarray(x, dtype=F32)
    if dtype == 'f32':
        return x
    if dtype != 'bf16':
        raise ValueError(dtype)
    return widen(pack_bf16(x))


def _canonical(v):
    v = np.asarray(v, dtype=F32).copy()
    v.view(np.uint32)[np.isnan(v)] = 0x7fc00000
    return v


def pair_dist(q, x, metric='cosine'):
    """dist [..] float32 of q [.., d] against x [.., d] (equal shapes, rows paired), the normative order."""
    if metric not in ('cosine', 'euclidean'):
        raise ValueError(metric)
    q, x = np.asarray(q, dtype=F32), np.asarray(x, dtype=F32)
    d = q.shape[-1]
    if d % 4 or not 1 <= d <= D_MAX:
        raise ValueError('d')
    T = (d + 255) // 256
    lead = q.shape[:-1]
    qp, xp = np.zeros(lead + (T * 256,), F32), np.zeros(lead + (T * 256,), F32)
    qp[..., :d], xp[..., :d] = q, x
    qp, xp = qp.reshape(lead + (T, 64, 4)), xp.reshape(lead + (T, 64, 4))
    a = np.zeros(lead + (64, 4), F32)
    with np.errstate(all='ignore'):
        for t in range(T):
            if metric == 'cosine':
                p = (qp[..., t, :, :] * xp[..., t, :, :]).astype(F32)
            else:
                e = (qp[..., t, :, :] - xp[..., t, :, :]).astype(F32)
                p = (e * e).astype(F32)
            a = (a + p).astype(F32)
        v = ((a[..., 0] + a[..., 1]).astype(F32) + (a[..., 2] + a[..., 3]).astype(F32)).astype(F32)
        for o in (32, 16, 8, 4, 2, 1):
            v = (v + v[..., LANES ^ o]).astype(F32)
        S = v[..., 0]
        if metric == 'cosine':
            return _canonical(-S)
        return _canonical(np.sqrt(np.where(S > F32(1e-12), S, F32(1e-12)).astype(F32), dtype=F32))


def dist(q, rows, cand, metric='cosine'):
    """(D [nq, L] float32, cidx [nq, L] int64): the distance block of the lists ``cand`` [nq, L] against the store VALUES
    ``rows`` [n, d]; an entry < 0 or >= n is padding: +inf, -1."""
    q, rows = np.asarray(q, dtype=F32), np.asarray(rows, dtype=F32)
    cand = np.asarray(cand).astype(np.int64)
    n = rows.shape[0]
    live = (cand >= 0) & (cand < n)
    D = np.full(cand.shape, np.inf, F32)
    cidx = np.where(live, cand, -1)
    qi, ji = np.nonzero(live)
    if qi.size:
        D[qi, ji] = pair_dist(q[qi], rows[cand[qi, ji]], metric)
    return D, cidx


def rank(D, cidx, k):
    """(dist [nq, k], idx [nq, k] int64): the first k live candidates of every row by the composite (grl_row_argsort's
    key, gallery index) -- a repeated id appears as often as it is listed -- padded with +inf / -1."""
    D, cidx = np.asarray(D, dtype=F32), np.asarray(cidx).astype(np.int64)
    nq = D.shape[0]
    idx = np.full((nq, k), -1, np.int64)
    out = np.full((nq, k), np.inf, F32)
    for r in range(nq):
        live = np.flatnonzero(cidx[r] >= 0)
        o = live[np.argsort(composite(sort_key(D[r, live]), cidx[r, live]), kind='stable')][:k]
        idx[r, :o.size] = cidx[r, o]
        out[r, :o.size] = D[r, o]
    return out, idx


def refine_lists(q, rows, cand, k, metric='cosine'):
    return rank(*dist(q, rows, cand, metric), k)


def parse_knob_cases():
    """(good, bad) values of GRL_EVAL_REFINE shared by the CPU test"""
    good = {'40': (40, 'f32'), ' 200 , bf16 ': (200, 'bf16'), '1': (1, 'f32'), '1024,bf16': (1024, 'bf16'), '7,f32': (7, 'f32')}
    bad = ('x', '0', '-3', '1025', '40,', ',bf16', '40,fp16', '40,bf16,1', '4.5', '40;bf16')
    return good, bad
