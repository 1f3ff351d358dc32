"""Host model of the clustering contract in numpy, for the tests of engine.cluster and its forms.

Edge i -> j (j != i) iff D[i][j] <= float32(eps) (NaN: never; eps = +inf: FLT_MAX); deg = a row's stored edges; core
iff deg + 1 >= min_samples; i ~ j iff i -> j or j -> i; clusters = connected components of the core points under ~,
numbered in ascending order of their smallest core index; a non-core point takes the smallest id among its adjacent
cores; everything else is -1."""
import numpy as np


def edges(D, eps):
    """Boolean [n, n] out-edge matrix of a dense distance matrix (float32)."""
    eps = np.float32(min(float(eps), float(np.finfo(np.float32).max)))
    with np.errstate(invalid='ignore'):
        A = np.asarray(D, dtype=np.float32) <= eps
    np.fill_diagonal(A, False)
    return A


def csr(A):
    """(row_ptr int64 [n+1], col int32 [E]) of a boolean out-edge matrix, columns ascending in every row."""
    r, c = np.nonzero(A)
    return np.concatenate(([0], np.cumsum(A.sum(1)))).astype(np.int64), c.astype(np.int32)


def dbscan(n, min_samples, A=None, row_ptr=None, col=None):
    """(labels int64 [n], core bool [n]) from the out-edge matrix ``A`` or from a CSR (deg = the row's stored entries,
    duplicates and self-loops counted as they are stored)."""
    if A is not None:
        deg = A.sum(1)
    else:
        deg = np.diff(row_ptr)
        A = np.zeros((n, n), dtype=bool)
        A[np.repeat(np.arange(n), deg), col] = True
    U = A | A.T
    np.fill_diagonal(U, False)
    core = deg + 1 >= min_samples
    labels = np.full(n, -1, dtype=np.int64)
    next_id = 0
    for i in range(n):                                   # ascending: a new cluster starts at its smallest core index
        if not core[i] or labels[i] >= 0:
            continue
        labels[i], todo = next_id, [i]
        while todo:
            for j in np.flatnonzero(U[todo.pop()] & core & (labels < 0)):
                labels[j] = next_id
                todo.append(j)
        next_id += 1
    for j in np.flatnonzero(~core):
        near = labels[U[j] & core]
        if near.size:
            labels[j] = near.min()
    return labels, core
