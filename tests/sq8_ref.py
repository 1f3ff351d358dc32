"""Host model (numpy) of the int8 scalar quantiser of DESIGN.md 4ah / include/grl_hip.h: engine.Sq8Codebook, sq8_train,
sq8_dist.

Every operation is one float32 operation (numpy rounds each), rint rounds half to even, the integer sum is exact and has
no order, so the model gives the device's bits from the same inputs.  Two inputs come from reductions whose order is the
device's own (``bias`` = q . mean by the fp32 GEMM, the norms by grl_row_sqnorm): the GPU tests hand the model the
downloaded values; the CPU tests use the float32 stand-ins below."""
import numpy as np

F32 = np.float32
D_MAX, TILE, NQ_MAX = 16384, 128, 1048576
C127 = F32(127.0)


def dpad(d):
    return -(-d // 64) * 64


def absmax(x, mean):
    """float32 [d]: max_i |x[i][j] - mean[j]|, NaN ignored (0 for a column of NaN or no rows)"""
    x = np.asarray(x, dtype=F32)
    with np.errstate(all='ignore'):
        a = np.abs((x - np.asarray(mean, dtype=F32)[None, :]).astype(F32))
    a = np.where(np.isnan(a), F32(0), a)
    return a.max(0).astype(F32) if x.shape[0] else np.zeros(x.shape[1], dtype=F32)


def steps_from_amax(amax):
    """(delta, inv) as sq8_train stores them: amax / 127 and 127 / amax, inv 0 where amax is 0"""
    amax = np.asarray(amax, dtype=F32)
    with np.errstate(all='ignore'):
        return (amax / C127).astype(F32), np.where(amax == 0, F32(0), (C127 / amax).astype(F32)).astype(F32)


def inv_from_delta(delta):
    """inv of a caller's delta: 127 / (127 * delta), 0 where delta is 0"""
    delta = np.asarray(delta, dtype=F32)
    with np.errstate(all='ignore'):
        return np.where(delta == 0, F32(0), (C127 / (C127 * delta).astype(F32)).astype(F32)).astype(F32)


def _round(v):
    """int8: 0 for NaN, else rint clamped to -127 .. 127"""
    with np.errstate(all='ignore'):
        r = np.clip(np.rint(np.where(np.isnan(v), F32(0), v)), -127, 127)
    return r.astype(np.int8)


def encode(x, mean, inv):
    """int8 [n, dpad]: clamp(rint((x - mean) * inv), -127, 127), NaN products 0, the columns d .. dpad 0"""
    x = np.asarray(x, dtype=F32)
    n, d = x.shape
    out = np.zeros((n, dpad(d)), dtype=np.int8)
    with np.errstate(all='ignore'):
        v = ((x - np.asarray(mean, dtype=F32)[None, :]).astype(F32) * np.asarray(inv, dtype=F32)[None, :]).astype(F32)
    out[:, :d] = _round(v)
    return out


def decode(codes, mean, delta):
    """float32 [n, d]: mean + delta * float(code), one multiply then one add"""
    d = len(mean)
    c = np.asarray(codes)[:, :d].astype(F32)
    with np.errstate(all='ignore'):
        t = (np.asarray(delta, dtype=F32)[None, :] * c).astype(F32)
        return (np.asarray(mean, dtype=F32)[None, :] + t).astype(F32)


def query(q, delta):
    """(qcodes int8 [nq, dpad], scale float32 [nq]): w = q * delta, s = the largest finite |w| (0 without one),
    r = 127 / s, code = clamp(rint(w * r)) and 0 for a NaN or infinite w (or a NaN product); scale = s / 127; s == 0: all 0"""
    q = np.asarray(q, dtype=F32)
    nq, d = q.shape
    with np.errstate(all='ignore'):
        w = (q * np.asarray(delta, dtype=F32)[None, :]).astype(F32)
        fin = np.isfinite(w)
        s = np.where(fin, np.abs(w), F32(0)).max(1).astype(F32) if d else np.zeros(nq, dtype=F32)
        r = (C127 / s).astype(F32)
        v = (w * r[:, None]).astype(F32)
        scale = (s / C127).astype(F32)
    codes = np.zeros((nq, dpad(d)), dtype=np.int8)
    codes[:, :d] = np.where(fin & (s[:, None] != 0), _round(v), np.int8(0))
    return codes, scale


def isum(qcodes, codes):
    """int64 [nq, n]: the exact integer sums"""
    return np.asarray(qcodes).astype(np.int64) @ np.asarray(codes).astype(np.int64).T


def dist(qcodes, scale, bias, codes, metric='cosine', qq=None, gg=None):
    """float32 [nq, n]: dot = scale * float32(isum) + bias; 'cosine': -dot; 'euclidean': t = (qq + gg) - 2 dot,
    sqrt(t > 1e-12 ? t : 1e-12) (a NaN t gives 1e-12)"""
    s = isum(qcodes, codes)
    assert np.abs(s).max(initial=0) < 2 ** 31
    with np.errstate(all='ignore'):
        dot = ((np.asarray(scale, dtype=F32)[:, None] * s.astype(F32)).astype(F32) + np.asarray(bias, dtype=F32)[:, None]).astype(F32)
        if metric == 'cosine':
            return np.negative(dot)
        t = ((np.asarray(qq, dtype=F32)[:, None] + np.asarray(gg, dtype=F32)[None, :]).astype(F32) - (F32(2.0) * dot).astype(F32)).astype(F32)
        return np.sqrt(np.where(t > F32(1e-12), t, F32(1e-12)).astype(F32)).astype(F32)


# ---- float32 stand-ins for the device's ordered reductions (CPU tests only) ----
def bias_host(q, mean):
    return (np.asarray(q, dtype=np.float64) @ np.asarray(mean, dtype=np.float64)).astype(F32)


def sqnorm_host(x):
    return (np.asarray(x, dtype=np.float64) ** 2).sum(1).astype(F32)


def train(x):
    """(mean, delta, inv) with a float64 column mean rounded once (the device's mean has its own order)"""
    x = np.asarray(x, dtype=F32)
    mean = x.astype(np.float64).mean(0).astype(F32)
    delta, inv = steps_from_amax(absmax(x, mean))
    return mean, delta, inv


# ---- the ranking recipe shared by tests/test_sq8_cpu.py and tests/test_gpu_sq8.py ----
RECIPE = dict(n=1000, d=128, nq=50, seeds=(0, 1, 2), floor=0.95)


def recipe(seed, n=None, d=None, nq=None):
    """(gallery [n, d], queries [50, d]) float32 unit rows: standard_normal + 0.1 as float32, L2-normalised; the gallery
    from PCG64(seed), the queries from PCG64(100 + seed)."""
    r = RECIPE
    n, d, nq = n or r['n'], d or r['d'], nq or r['nq']

    def rows(s, m):
        x = np.random.Generator(np.random.PCG64(s)).standard_normal((m, d)).astype(F32) + F32(0.1)
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)
    return rows(seed, n), rows(100 + seed, nq)


def exact_lists(q, g, k):
    """the k nearest gallery rows of every query by descending dot product (float64), ties to the smaller index"""
    s = np.asarray(q, dtype=np.float64) @ np.asarray(g, dtype=np.float64).T
    return np.argsort(-s, axis=1, kind='stable')[:, :k]


def ranked(D, k):
    return np.argsort(np.asarray(D), axis=1, kind='stable')[:, :k]


def recall_at(approx, exact, k):
    return float(np.mean([len(set(a[:k]) & set(e[:k])) / float(k) for a, e in zip(approx, exact)]))


def parse_knob_cases():
    good = {'1': (None, None), ' 1 ': (None, None), '1,16': (16, 'f32'), '1,100,bf16': (100, 'bf16'),
            ' 1 , 1024 , f32 ': (1024, 'f32'), '1,1': (1, 'f32')}
    bad = ('0', '2', 'on', '1,', '1,0', '1,1025', '1,-4', '1,x', '1,16,fp16', '1,16,bf16,3', '1.0', ',16', '1,16,', 'true')
    return good, bad
