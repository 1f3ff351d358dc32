"""The network's first layer restated in float64 (numpy only): the independent reference of the stem convolution, the
3x3 / stride 2 max-pool, its two backwards and the stem im2col (grl_amd/csrc/pointwise.hip, pointwise_bf16.hip, train.hip,
train_bf16.hip).

Images are NCHW [n][3][H][W] as the stem kernels read them; every activation is channels-last, [n][H][W][C] (the stem
output flattened to [n * Ho * Wo][64]), as the kernels write it.  Next to its results a function returns the sums of
absolute terms that the rounding-error bounds of tests/stem_bounds.py are built from."""
import numpy as np


def f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def normalize(u8, mean_std):
    """raw pixels [n][3][H][W] -> (u / 255 - mean[c]) / std[c]; mean_std = mean[0..2], std[0..2]"""
    ms = f64(mean_std)
    return (f64(u8) / 255.0 - ms[:3][None, :, None, None]) / ms[3:6][None, :, None, None]


def stem(x, w, scale, shift, relu, ex=None):
    """7x7 / stride 2 / pad 3 convolution of x [n][3][H][W] (H, W even) with w [64][3][7][7] as an explicit sum over
    (c, ky, kx), then * scale + shift, then the optional ReLU.  Returns dict: y [n * Ho * Wo][64], acc (the convolution),
    A = sum |x| |w| per output element and, if ex (an absolute error of every input pixel) is given, E = sum ex |w|."""
    x, w = f64(x), f64(w).reshape(64, 3, 7, 7)
    n, _, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    xp = np.zeros((n, 3, H + 6, W + 6))
    xp[:, :, 3:H + 3, 3:W + 3] = x
    ep = None
    if ex is not None:
        ep = np.zeros_like(xp)
        ep[:, :, 3:H + 3, 3:W + 3] = f64(ex)
    acc = np.zeros((n, Ho, Wo, 64))
    A = np.zeros_like(acc)
    E = np.zeros_like(acc) if ep is not None else None
    for c in range(3):
        for ky in range(7):
            for kx in range(7):
                p = xp[:, c, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2][..., None]
                wk = w[:, c, ky, kx]
                acc += p * wk
                A += np.abs(p) * np.abs(wk)
                if ep is not None:
                    E += ep[:, c, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2][..., None] * np.abs(wk)
    pre = acc * f64(scale) + f64(shift)
    y = np.maximum(pre, 0.0) if relu else pre
    flat = lambda a: None if a is None else a.reshape(n * Ho * Wo, 64)      # noqa: E731
    return dict(y=flat(y), acc=flat(acc), A=flat(A), E=flat(E), Ho=Ho, Wo=Wo)


def pooled_size(H, W):
    return (H + 1) // 2, (W + 1) // 2


def maxpool(a):
    """3x3 / stride 2 / pad 1 max-pool of a [n][H][W][C] over the valid elements of every window only (no pad value takes
    part).  Returns (y [n][Ho][Wo][C], pos): pos = ky * 3 + kx of the FIRST maximum in (ky, kx) scan order (a later element
    replaces the maximum only if it is strictly larger), uint8."""
    a = np.asarray(a)
    a = a if a.dtype == np.float64 else a.astype(np.float64)
    n, H, W, C = a.shape
    Ho, Wo = pooled_size(H, W)
    y = np.full((n, Ho, Wo, C), -np.inf)
    pos = np.zeros((n, Ho, Wo, C), np.uint8)
    seen = np.zeros((Ho, Wo), bool)
    for ky in range(3):
        for kx in range(3):
            # window o covers inputs 2 o - 1 + k: the outputs for which that input exists
            oy0, ox0 = (1 if ky == 0 else 0), (1 if kx == 0 else 0)
            oy1, ox1 = min(Ho, (H - ky) // 2 + 1), min(Wo, (W - kx) // 2 + 1)
            if oy1 <= oy0 or ox1 <= ox0:
                continue
            v = a[:, 2 * oy0 - 1 + ky:2 * (oy1 - 1) + ky:2, 2 * ox0 - 1 + kx:2 * (ox1 - 1) + kx:2, :]
            ysub, psub = y[:, oy0:oy1, ox0:ox1, :], pos[:, oy0:oy1, ox0:ox1, :]
            take = v > ysub
            ysub[take] = v[take]
            psub[take] = ky * 3 + kx
            seen[oy0:oy1, ox0:ox1] = True
    assert seen.all()
    return y, pos


def maxpool_bwd(pos_or_a, dy, shape=None):
    """gather through the first-maximum positions: dx[n][2 oy - 1 + ky][2 ox - 1 + kx][c] += dy[n][oy][ox][c].
    pos_or_a: the uint8 positions (then shape = (H, W) of the input) or the float input a itself.
    Returns (dx [n][H][W][C], S = the same gather of |dy|: what the rounding bound is built from)."""
    p = np.asarray(pos_or_a)
    if p.dtype != np.uint8:
        shape = p.shape[1:3]
        p = maxpool(p)[1]
    H, W = shape
    dy = f64(dy).reshape(p.shape)
    n, Ho, Wo, C = p.shape
    ni, ci = np.arange(n)[:, None, None, None], np.arange(C)[None, None, None, :]
    iy = 2 * np.arange(Ho)[None, :, None, None] - 1 + (p // 3).astype(np.int64)
    ix = 2 * np.arange(Wo)[None, None, :, None] - 1 + (p % 3).astype(np.int64)
    assert iy.min() >= 0 and iy.max() < H and ix.min() >= 0 and ix.max() < W, 'a position outside the image'
    lin = (((ni * H + iy) * W + ix) * C + ci).ravel()
    dx = np.bincount(lin, weights=dy.ravel(), minlength=n * H * W * C).reshape(n, H, W, C)
    S = np.bincount(lin, weights=np.abs(dy).ravel(), minlength=n * H * W * C).reshape(n, H, W, C)
    return dx, S


def im2col(x, Kp):
    """col[(img, oy, ox)][k] = x[img][c][2 oy - 3 + ky][2 ox - 3 + kx], k = (c * 7 + ky) * 7 + kx; 0 outside the image and for
    147 <= k < Kp"""
    x = f64(x)
    n, _, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    xp = np.zeros((n, 3, H + 6, W + 6))
    xp[:, :, 3:H + 3, 3:W + 3] = x
    col = np.zeros((n, Ho, Wo, Kp))
    for c in range(3):
        for ky in range(7):
            for kx in range(7):
                col[..., (c * 7 + ky) * 7 + kx] = xp[:, c, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2]
    return col.reshape(n * Ho * Wo, Kp)
