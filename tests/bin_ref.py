"""Host model (numpy) of the binary-code contract of DESIGN.md 4ag / include/grl_hip.h: engine.BinaryCodebook, bin_train,
bin_dist.

Bit b of a row is z[b] > 0 (NaN, -0 and +0 give 0).  Public layout: numpy.packbits(bits, axis=1, bitorder='little'); scan
layout: uint32 [W, n], word w of row g = the public bytes 4w .. 4w + 3, little endian.  The Hamming distance is an integer;
the asymmetric tables are float32 sums in a fixed order, so both are derived from given bits.  The ITQ and LSH trainers
are float64 models of the algorithm (the device's fp32 GEMMs give other low bits, so only properties are compared)."""
import numpy as np

F32 = np.float32
NBITS_MAX, SLAB, NQ_MAX = 1024, 1024, 524280


def bits_of(z):
    """bool [n, nbits]: z > 0 (a NaN compares false)"""
    with np.errstate(invalid='ignore'):
        return np.asarray(z) > 0


def pack(bits):
    """public layout uint8 [n, nbits / 8]: bit j of byte m = column 8m + j"""
    bits = np.asarray(bits, dtype=bool)
    assert bits.ndim == 2 and bits.shape[1] % 32 == 0
    return np.packbits(bits, axis=1, bitorder='little')


def unpack(codes):
    return np.unpackbits(np.asarray(codes, dtype=np.uint8), axis=1, bitorder='little').astype(bool)


def words(codes):
    """scan layout uint32 [W, n] of public codes [n, 4W]"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    n, nb = codes.shape
    assert nb % 4 == 0
    return np.ascontiguousarray(codes.view('<u4').reshape(n, nb // 4).T)


def unwords(w):
    """public codes [n, 4W] of the scan layout [W, n]"""
    w = np.ascontiguousarray(np.asarray(w).astype('<u4').T)
    return w.view(np.uint8).reshape(w.shape[0], -1)


def popcount32(v):
    v = np.asarray(v, dtype=np.uint32)
    v = v - ((v >> 1) & np.uint32(0x55555555))
    v = (v & np.uint32(0x33333333)) + ((v >> 2) & np.uint32(0x33333333))
    v = (v + (v >> 4)) & np.uint32(0x0f0f0f0f)
    return ((v * np.uint32(0x01010101)) >> 24).astype(np.int64)


def hamming(qcodes, gcodes):
    """float32 [nq, n] by unpacked bits: the number of differing bits"""
    q, g = unpack(qcodes), unpack(gcodes)
    return (q[:, None, :] != g[None, :, :]).sum(2).astype(F32)


def hamming_words(qcodes, gcodes):
    """the same by XOR and a word-wise population count on the scan layout, as the kernel counts"""
    qw, gw = words(qcodes).T, words(gcodes)                         # [nq, W], [W, n]
    out = np.zeros((qw.shape[0], gw.shape[1]), dtype=np.int64)
    for w in range(gw.shape[0]):
        out += popcount32(qw[:, w][:, None] ^ gw[w][None, :])
    return out.astype(F32)


def lut(z):
    """float32 [nq, nbits / 8, 256]: entry [q, m, c] = the sequential float32 sum from +0 over j = 0..7 of -z[q, 8m + j]
    where bit j of c is set, +z[q, 8m + j] elsewhere (adds and exact negations only)"""
    z = np.asarray(z, dtype=F32)
    nq, nbits = z.shape
    zz = z.reshape(nq, nbits // 8, 1, 8)
    c = np.arange(256)
    out = np.zeros((nq, nbits // 8, 256), dtype=F32)
    with np.errstate(all='ignore'):
        for j in range(8):
            v = np.broadcast_to(zz[..., j], out.shape)
            out = (out + np.where(((c >> j) & 1).astype(bool), np.negative(v), v)).astype(F32)
    return out


def lut64(z):
    """the same tables in float64 from the float32 projections"""
    z = np.asarray(z, dtype=np.float64)
    nq, nbits = z.shape
    sign = 1.0 - 2.0 * ((np.arange(256)[:, None] >> np.arange(8)[None, :]) & 1)          # [256, 8]
    return np.einsum('qmj,cj->qmc', z.reshape(nq, nbits // 8, 8), sign)


def asym64(zq, gbits):
    """float64 [nq, n]: -sum_b z_q[b] s_g[b], s = +1 where the bit is set, -1 elsewhere"""
    s = 2.0 * np.asarray(gbits, dtype=np.float64) - 1.0
    return -(np.asarray(zq, dtype=np.float64) @ s.T)


# ---- trainers, float64 ----
def lsh(x, nbits, seed=0):
    """(proj [nbits, d] float32 as drawn, shift float64 = -proj mean)"""
    x = np.asarray(x, dtype=np.float64)
    proj = np.random.Generator(np.random.PCG64(seed)).standard_normal((nbits, x.shape[1])).astype(F32)
    return proj, -(proj.astype(np.float64) @ x.mean(0))


def itq(x, nbits, n_iter=50, seed=0):
    """(proj [nbits, d], shift [nbits], objective [n_iter]) in float64: PCA to nbits columns by the eigenvectors of the
    covariance, R_0 = QR of Generator(PCG64(seed)).standard_normal((nbits, nbits)), then n_iter rounds of B = sign(V R)
    (+1 where > 0, else -1), SVD of B^T V = U S W^T, R = W U^T; objective = sum of the singular values per round."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(0)
    xc = x - mean
    lam, vec = np.linalg.eigh(xc.T @ xc)
    comp = vec[:, np.argsort(-lam)[:nbits]].T                        # [nbits, d], orthonormal rows
    v = xc @ comp.T
    r = np.linalg.qr(np.random.Generator(np.random.PCG64(seed)).standard_normal((nbits, nbits)))[0]
    objective = []
    for _ in range(n_iter):
        b = np.where(v @ r > 0, 1.0, -1.0)
        u, s, wt = np.linalg.svd(b.T @ v)
        objective.append(float(s.sum()))
        r = (u @ wt).T
    proj = r.T @ comp
    return proj, -(proj @ mean), objective


# ---- the training recipe shared by tests/test_bin_cpu.py and tests/test_gpu_bin.py ----
RECIPE = dict(n=1000, d=128, ids=50, nbits=32, nq=64, noise=0.6, offset=0.5, n_iter=30)


def recipe(seed, n=None, d=None, ids=None):
    """(gallery [n, d], queries [64, d]) float32 unit rows: c = N(0, 1) [ids, d] and x = c[i mod ids] + 0.6 N(0, 1) + 0.5,
    normalised; the gallery drawn from PCG64(seed), the queries (centres and noise) from PCG64(seed + 100)."""
    r = RECIPE
    n, d, ids = n or r['n'], d or r['d'], ids or r['ids']

    def rows(s, m):
        gen = np.random.Generator(np.random.PCG64(s))
        c = gen.standard_normal((ids, d))
        x = c[np.arange(m) % ids] + r['noise'] * gen.standard_normal((m, d)) + r['offset']
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)
    return rows(seed, n), rows(seed + 100, r['nq'])


def exact_lists(q, g, k):
    """the k nearest gallery rows of every query by descending dot product (float64), ties to the smaller index"""
    s = np.asarray(q, dtype=np.float64) @ np.asarray(g, dtype=np.float64).T
    return np.argsort(-s, axis=1, kind='stable')[:, :k]


def ranked(D, k):
    """the first k columns of every row of D ascending, ties to the smaller index"""
    return np.argsort(np.asarray(D), axis=1, kind='stable')[:, :k]


def recall_at(approx, exact, k):
    return float(np.mean([len(set(a[:k]) & set(e[:k])) / float(k) for a, e in zip(approx, exact)]))


def parse_knob_cases():
    good = {'32': (32, 'itq', 50, 0), '256,lsh': (256, 'lsh', 50, 0), ' 64 , itq , 30 ': (64, 'itq', 30, 0),
            '1024,lsh,1,7': (1024, 'lsh', 1, 7), '96,itq,5,0': (96, 'itq', 5, 0)}
    bad = ('0', '31', '33', '1056', '-32', '32,foo', '32,ITQ', '32,itq,0', '32,itq,5,-1', '32,itq,5,1,2', 'x', '32,,', '32.0',
           '32,itq,x', ',itq')
    return good, bad
