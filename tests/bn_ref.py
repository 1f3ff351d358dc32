"""Train-mode BatchNorm restated in float64 (numpy only): the independent reference of the statistics, finalize,
centred-apply and backward kernels (grl_amd/csrc/train.hip, train_bnfuse.hip, train_bf16.hip).

Every function works on float64 arrays laid out as the kernels see them -- rows = pixels (or samples), columns = channels --
and returns, next to its results, the sums of absolute terms that the rounding-error bounds of tests/bn_bounds.py are
built from.  ``apply_centered`` and ``backward`` take mean / invstd / scale as ARGUMENTS: a test hands them the fp32
vectors the kernel under test read, upcast exactly, so that a stage is charged only with its own roundings."""
import numpy as np


def f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def stats(x, pivot=None):
    """Column statistics of x[M][C].  d = x - pivot (pivot: a [C] vector, None = 0).
    Returns dict: sum_d, sum_d2 (what the kernels' slabs hold), mean, var (biased; taken in two passes around the float64
    mean, so that it does not depend on the pivot and keeps its accuracy when |mean| >> spread), and the bound
    ingredients abs_d = sum |d| and sq_d = sum d^2 (= sum |d*d|)."""
    x = f64(x)
    p = np.zeros(x.shape[1]) if pivot is None else f64(pivot)
    d = x - p[None, :]
    m0 = x.mean(0)
    dev = x - m0[None, :]
    corr = dev.mean(0)                                # float64 rounding residue of m0
    mean = m0 + corr
    var = (dev * dev).mean(0) - corr * corr
    return dict(sum_d=d.sum(0), sum_d2=(d * d).sum(0), mean=mean, var=np.maximum(var, 0.0),
                abs_d=np.abs(d).sum(0), sq_d=(d * d).sum(0))


def finalize(mean, var, count, gamma, beta, rm, rv, momentum, eps):
    """invstd, folded scale / shift and the running-statistics update, by torch's rule: the running variance takes the
    UNBIASED batch variance (var * count / (count - 1)); with count == 1 there is no unbiased estimate and the biased
    one (0) is kept.  gamma / beta None = 1 / 0; rm / rv None = no running statistics (returned as None).
    Returns dict: invstd, scale, shift, running_mean, running_var, unbiased."""
    mean, var = f64(mean), f64(var)
    g = np.ones_like(mean) if gamma is None else f64(gamma)
    b = np.zeros_like(mean) if beta is None else f64(beta)
    invstd = 1.0 / np.sqrt(var + float(eps))
    scale = g * invstd
    shift = b - mean * scale
    unbiased = var * (float(count) / (float(count) - 1.0)) if count > 1 else var.copy()
    out = dict(invstd=invstd, scale=scale, shift=shift, unbiased=unbiased, running_mean=None, running_var=None)
    if rm is not None:
        m = float(momentum)
        out['running_mean'] = (1.0 - m) * f64(rm) + m * mean
        out['running_var'] = (1.0 - m) * f64(rv) + m * unbiased
    return out


def apply_centered(z, mean, scale, beta=None, res=None, relu=False):
    """y = relu?((z - mean) * scale + beta + res).  Returns dict: y, pre (y before the ReLU), mask = (y > 0), and
    abs_terms = |z - mean| |scale| + |beta| + |res| per element."""
    z = f64(z)
    t = (z - f64(mean)[None, :]) * f64(scale)[None, :]
    a = np.abs(t)
    if beta is not None:
        t = t + f64(beta)[None, :]
        a = a + np.abs(f64(beta))[None, :]
    if res is not None:
        t = t + f64(res)
        a = a + np.abs(f64(res))
    y = np.maximum(t, 0.0) if relu else t
    return dict(y=y, pre=t, mask=y > 0, abs_terms=a)


def backward(dy, z, mask, mean, invstd, gamma=None):
    """Backward of y = relu?(bn(z) (+ res)) with respect to z, gamma, beta.  ``mask`` (bool [M][C], None = no ReLU) is the
    forward's (y > 0).  g = dy * mask; xhat = (z - mean) * invstd; dbeta = sum g; dgamma = sum g * xhat;
    dz = gamma * invstd * (g - dbeta / M - xhat * dgamma / M).
    Returns dict: g, sum_g, sum_gx, dz, dgamma, dbeta, xhat, and the bound ingredients abs_g = sum |g|,
    abs_gx = sum |g * xhat| per channel, abs_terms = |gamma invstd| (|g| + |sum_g / M| + |xhat| |sum_gx / M|) per element."""
    dy, z = f64(dy), f64(z)
    M = z.shape[0]
    g = dy if mask is None else np.where(np.asarray(mask, dtype=bool), dy, 0.0)
    is_ = f64(invstd)
    xhat = (z - f64(mean)[None, :]) * is_[None, :]
    gx = g * xhat
    sum_g, sum_gx = g.sum(0), gx.sum(0)
    gm = is_ if gamma is None else is_ * f64(gamma)
    k0, k1 = sum_g / M, sum_gx / M
    dz = gm[None, :] * (g - k0[None, :] - xhat * k1[None, :])
    abs_terms = np.abs(gm)[None, :] * (np.abs(g) + np.abs(k0)[None, :] + np.abs(xhat) * np.abs(k1)[None, :])
    return dict(g=g, sum_g=sum_g, sum_gx=sum_gx, dz=dz, dgamma=sum_gx, dbeta=sum_g, xhat=xhat, gm=gm,
                abs_g=np.abs(g).sum(0), abs_gx=np.abs(gx).sum(0), abs_terms=abs_terms)
