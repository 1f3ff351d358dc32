"""Float64 host model of ranking by the Siamese verification head (engine.verify_metric).

``literal_F`` is the head as the model defines it -- (p - g)^2 for every pair, BatchNorm1d in eval mode, Linear, the
class-1 minus class-0 logit -- blended with the cosine distance.  ``fold`` / ``folded_F`` are the algebra the device
uses, written separately so that the CPU tests can hold one against the other.  Everything is numpy float64."""
import numpy as np


def make_head(D, seed=0):
    """A verification head with every sign case: gamma with negative and exactly-zero entries, running statistics away
    from (0, 1), W[1] - W[0] of mixed sign, a bias.  float32 values (what a module holds), as a dict of arrays."""
    g = np.random.Generator(np.random.PCG64(seed))
    gamma = g.uniform(-1.5, 1.5, D).astype(np.float32)
    gamma[::17] = 0.0
    return dict(gamma=gamma,
                beta=g.uniform(-0.3, 0.3, D).astype(np.float32),
                mean=g.normal(0.0, 0.01, D).astype(np.float32),
                var=g.uniform(1e-4, 2e-3, D).astype(np.float32),
                eps=1e-5,
                W=g.normal(0.0, 0.05, (2, D)).astype(np.float32),
                b=np.array([0.03, -0.02], np.float32))


def _f64(head):
    return {k: np.asarray(v, np.float64) for k, v in head.items()}


def literal_logits(p, g, head):
    """[np, ng, 2]: Linear(BatchNorm1d_eval((p - g)^2)) for every pair, as the model computes it."""
    h = _f64(head)
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    diff = (p[:, None, :] - g[None, :, :]) ** 2
    bn = (diff - h['mean']) / np.sqrt(h['var'] + h['eps']) * h['gamma'] + h['beta']
    return bn @ h['W'].T + h['b']


def literal_F(q, g, col0, head, beta):
    """F = (1 - beta) (-q . g^T) - beta s, s = l1 - l0 of the head on the slice [col0, col0 + D) of the rows."""
    q, g = np.asarray(q, np.float64), np.asarray(g, np.float64)
    D = head['gamma'].shape[0]
    lg = literal_logits(q[:, col0:col0 + D], g[:, col0:col0 + D], head)
    s = lg[..., 1] - lg[..., 0]
    return (1.0 - beta) * (-(q @ g.T)) - beta * s


def fold(head):
    """(w [D], c): s(p, g) = sum_d w_d (p_d - g_d)^2 + c.  The operation order is the one grl_verify_fold documents."""
    h = _f64(head)
    dw = h['W'][1] - h['W'][0]
    sd = np.sqrt(h['var'] + h['eps'])
    w = dw * h['gamma'] / sd
    c = np.sum(dw * (h['beta'] - h['gamma'] * h['mean'] / sd)) + h['b'][1] - h['b'][0]
    return w, float(c)


def row_terms(q, g, col0, w, c, beta):
    """(q' [nq, d], rq [nq], rg [ng]) of the folded form F = -q' . g - (rq + rg)."""
    q, g = np.asarray(q, np.float64), np.asarray(g, np.float64)
    D = w.shape[0]
    qv = (1.0 - beta) * q
    qv[:, col0:col0 + D] = ((1.0 - beta) - 2.0 * beta * w) * q[:, col0:col0 + D]
    rq = beta * ((q[:, col0:col0 + D] ** 2) @ w + c)
    rg = beta * ((g[:, col0:col0 + D] ** 2) @ w)
    return qv, rq, rg


def folded_F(q, g, col0, w, c, beta):
    qv, rq, rg = row_terms(q, g, col0, w, c, beta)
    return -(qv @ np.asarray(g, np.float64).T) - (rq[:, None] + rg[None, :])


def error_bound(q, g, col0, w, c, beta):
    """Per-entry worst case of the device's fp32 evaluation of the folded form: a K-term fp32 fma chain (the NEGDOT
    GEMM; K = the row width, or the head's width D when beta = 1 and the GEMM runs over the slice alone) plus the
    three scalar operations around it:  2 (K + 8) 2^-24 (sum_d |q'_d g_d| + |rq| + |rg|)."""
    qv, rq, rg = row_terms(q, g, col0, w, c, beta)
    K = w.shape[0] if beta == 1.0 else qv.shape[1]
    mag = np.abs(qv) @ np.abs(np.asarray(g, np.float64)).T + np.abs(rq)[:, None] + np.abs(rg)[None, :]
    return 2.0 * (K + 8) * 2.0 ** -24 * mag


def features(nq, ng, d, col0, D, seed):
    """Standard-normal float32 rows [nq, d] / [ng, d] whose head slice [col0, col0 + D) is L2-normalised."""
    g = np.random.Generator(np.random.PCG64(seed))
    out = []
    for n in (nq, ng):
        x = g.standard_normal((n, d)).astype(np.float32)
        s = x[:, col0:col0 + D]
        x[:, col0:col0 + D] = s / np.linalg.norm(s.astype(np.float64), axis=1, keepdims=True).astype(np.float32)
        out.append(x)
    return out[0], out[1]
