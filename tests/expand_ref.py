"""Host model of grl_expand_rows (grl_amd/csrc/expand.hip, include/grl_hip.h): query expansion / database-side
augmentation from neighbour lists, in numpy float32 with the kernel's operation order.  The device results are held to
it bit for bit, so nothing compared against it has a tolerance.

  kept neighbours of row i : walk the list left to right, skip idx < 0 (and idx >= nb), with skip_self skip idx == i,
                             keep the first m that remain (fewer may);
  weight                   : s = -dist if dist < 0 else 0 (NaN -> 0); alpha == 0: w = 1; else w = s, alpha - 1 times
                             w = w * s;
  accumulation             : acc = x[i]; wsum = 1; per kept neighbour in list order acc = acc + (w * bank[j]) -- the
                             product is rounded, then the sum -- and wsum = wsum + w;
  result                   : acc / wsum (IEEE float32 division); a NaN is stored as 0x7fc00000.
"""
import numpy as np

F32 = np.float32
CANONICAL_NAN = np.frombuffer(np.uint32(0x7fc00000).tobytes(), np.float32)[0]


def kept(idx_row, i, m, nb, skip_self=False):
    """Positions (into the list) of the first m kept entries of row i."""
    out = []
    for t, j in enumerate(idx_row):
        j = int(j)
        if j < 0 or j >= nb or (skip_self and j == i):
            continue
        out.append(t)
        if len(out) == m:
            break
    return out


def weight(dist, alpha):
    """float32 weight of one kept neighbour; alpha - 1 rounded multiplications, left to right."""
    dist = F32(dist)
    s = F32(-dist) if dist < 0 else F32(0.0)              # NaN < 0 is False
    if alpha == 0:
        return F32(1.0)
    w = s
    for _ in range(alpha - 1):
        w = F32(w * s)
    return w


def expand_rows(x, bank, idx, dist, m, alpha=0, skip_self=False):
    """float32 [n, d]: the model of grl_expand_rows on host arrays (x [n, d], bank [nb, d], idx / dist [n, L])."""
    x, bank = np.asarray(x, F32), np.asarray(bank, F32)
    idx, dist = np.asarray(idx), np.asarray(dist, F32)
    n, nb = x.shape[0], bank.shape[0]
    assert idx.shape == dist.shape and idx.shape[0] == n and 1 <= m <= idx.shape[1] and 0 <= alpha <= 8
    assert not skip_self or n == nb
    out = np.empty_like(x)
    with np.errstate(all='ignore'):
        for i in range(n):
            acc = x[i].copy()
            wsum = F32(1.0)
            for t in kept(idx[i], i, m, nb, skip_self):
                w = weight(dist[i, t], alpha)
                prod = (w * bank[int(idx[i, t])]).astype(F32)       # rounded product ...
                acc = (acc + prod).astype(F32)                      # ... then the rounded sum
                wsum = F32(wsum + w)
            out[i] = (acc / wsum).astype(F32)
    out[np.isnan(out)] = CANONICAL_NAN
    return out


def expand_rows_f64(x, bank, idx, dist, m, alpha=0, skip_self=False):
    """The same weighted mean computed independently in float64 (np.dot over the kept rows): what the float32 model
    approximates.  The weights are the float32 values of ``weight`` -- they are the mean's inputs, and their own
    rounding (alpha - 1 products) is not the accumulation's error.  Finite inputs only."""
    x, bank = np.asarray(x, np.float64), np.asarray(bank, np.float64)
    idx, dist = np.asarray(idx), np.asarray(dist, F32)
    n, nb = x.shape[0], bank.shape[0]
    out = np.empty_like(x)
    for i in range(n):
        ts = kept(idx[i], i, m, nb, skip_self)
        js = idx[i, ts].astype(np.int64)
        w = np.array([weight(dist[i, t], alpha) for t in ts], np.float64)
        out[i] = (x[i] + w.dot(bank[js])) / (1.0 + w.sum()) if len(ts) else x[i]
    return out
