"""Numpy reference of the pair-level (verification) metrics, written from the definition in DESIGN.md 4r and sharing
no code with grl_amd.engine: the order-preserving key of a float32, the bin, the two histograms of a full distance
matrix with its id lists, and the figures the host derives from them.  Everything after the histograms is float64 over
ALL 2^bits + 1 bin boundaries (the engine walks the non-empty bins only)."""
import numpy as np

FPR_TARGETS = (1e-4, 1e-3, 1e-2, 1e-1)


def key(d):
    """uint32 keys of float32 values: -0 -> +0; sign clear: bits ^ 0x80000000, sign set: ~bits; NaN: 0xffffffff."""
    d = np.ascontiguousarray(d, dtype=np.float32)
    u = d.view(np.uint32).copy()
    u[d == 0] = 0
    neg = (u >> np.uint32(31)) == 1
    k = np.where(neg, ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(d)] = np.uint32(0xFFFFFFFF)
    return k


def bins(d, bits):
    return (key(d) >> np.uint32(32 - bits)).astype(np.int64)


def classes(q_pids, g_pids, q_cams, g_cams):
    """(positive, negative) boolean [nq, ng] masks; same pid AND same camera is in neither."""
    qp, gp = np.asarray(q_pids).reshape(-1, 1), np.asarray(g_pids).reshape(1, -1)
    qc, gc = np.asarray(q_cams).reshape(-1, 1), np.asarray(g_cams).reshape(1, -1)
    same = qp == gp
    return same & (qc != gc), ~same


def histograms(D, q_pids, g_pids, q_cams, g_cams, bits):
    """(pos, neg) int64 [2^bits] of the matrix D [nq, ng]."""
    D = np.asarray(D, dtype=np.float32)
    b = bins(D, bits).reshape(D.shape)
    P, N = classes(q_pids, g_pids, q_cams, g_cams)
    n = 1 << bits
    return (np.bincount(b[P], minlength=n).astype(np.int64), np.bincount(b[N], minlength=n).astype(np.int64))


def boundaries(pos, neg):
    """(tpr, fpr) float64 [2^bits + 1]: boundary k = the first k bins accepted (boundary 0: nothing)."""
    n_pos, n_neg = int(pos.sum()), int(neg.sum())
    if n_pos == 0:
        raise ValueError('no positive pairs')
    if n_neg == 0:
        raise ValueError('no negative pairs')
    tpr = np.concatenate(([0], np.cumsum(pos))) / float(n_pos)
    fpr = np.concatenate(([0], np.cumsum(neg))) / float(n_neg)
    return tpr, fpr


def auc(pos, neg):
    """Mann-Whitney over the bins: a (positive, negative) pair counts 1 when the positive's bin is lower, 1/2 when the
    two share a bin."""
    n_pos, n_neg = int(pos.sum()), int(neg.sum())
    boundaries(pos, neg)
    total = 0.0
    below = 0                                  # negatives in lower bins
    for p, n in zip(pos.tolist(), neg.tolist()):
        if p:
            total += p * ((n_neg - below - n) + 0.5 * n)
        below += n
    return total / (float(n_pos) * float(n_neg))


def auc_slack(pos, neg):
    return 0.5 * float((pos.astype(np.float64) * neg.astype(np.float64)).sum()) / (float(pos.sum()) * float(neg.sum()))


def eer(pos, neg):
    tpr, fpr = boundaries(pos, neg)
    for k in range(len(tpr)):
        if fpr[k] >= 1.0 - tpr[k]:
            break
    # k >= 1: at boundary 0 FPR = 0 < 1 = 1 - TPR
    g0, g1 = fpr[k - 1] - (1.0 - tpr[k - 1]), fpr[k] - (1.0 - tpr[k])
    t = -g0 / (g1 - g0)
    return float(fpr[k - 1] + t * (fpr[k] - fpr[k - 1]))


def tpr_at_fpr(pos, neg, target):
    tpr, fpr = boundaries(pos, neg)
    return float(tpr[np.flatnonzero(fpr <= target)[-1]])
