"""float64 restatement of the weight gradient grl_conv_wgrad_f32 and grl_stem_wgrad compute: the dense product, the
implicit-GEMM convolution (dgrad_ref.wgrad states it; here it also counts terms) and the 7x7/s2/p3 stem straight from the
NCHW clip.  numpy only; nothing here is written the way the kernels compute it.

Every restatement returns (result, abs_terms, terms): ``abs_terms`` is the same sum over the absolute values of its terms --
what the rounding-error bounds of wgrad_bounds.py are relative to --, ``terms`` the number of non-zero terms of each element.

Layouts: dz[m][ldz] and x[m][ldx] are rows over the reduction index (output pixels); a conv's x is channels-last,
x[n H W][C]; the conv result is torch's dw[N][C][kh][kw]; the stem reads x[n][3][H][W] and returns dw[64][3][7][7]."""
import numpy as np

import dgrad_ref as R

f64 = R.f64


def dense(dz, x, N, K, k_out=None):
    """dw[n][k] = sum_m dz[m][n] x[m][k] for n < N, k < k_out <= K; dz is [M][ldz >= N], x is [M][ldx >= K]."""
    k_out = K if not k_out else k_out
    a, b = f64(dz)[:, :N], f64(x)[:, :k_out]
    return a.T @ b, np.abs(a).T @ np.abs(b), (a != 0).astype(np.float64).T @ (b != 0).astype(np.float64)


def conv(dz, x, n, H, W, Ho, Wo, k, stride, pad):
    """dw[o][c][ky][kx] = sum over (img, oy, ox) of dz[img, oy, ox, o] x[img, stride oy - pad + ky, stride ox - pad + kx, c]
    inside the map: dgrad_ref.wgrad, for any (k, stride, pad) -- 3x3/s1/p1, 3x3/s2/p1 and 1x1/s2/p0 are the model's.
    The term count is the same sum over the operands' non-zero indicators."""
    dw, ab = R.wgrad(dz, x, n, H, W, Ho, Wo, k, stride, pad)
    cnt, _ = R.wgrad(f64(dz) != 0, f64(x) != 0, n, H, W, Ho, Wo, k, stride, pad)
    return dw, ab, cnt


def stem(dz, x, n, H, W):
    """dw[o][c][ky][kx] = sum over (img, oy, ox) of dz[(img Ho + oy) Wo + ox][o] x[img][c][2 oy - 3 + ky][2 ox - 3 + kx]
    inside the image, Ho = H / 2, Wo = W / 2: the 7x7 / stride 2 / pad 3 stem from the NCHW clip."""
    g = f64(dz).reshape(-1, 64)
    cols = stem_columns(f64(x), n, H, W)                # [n Ho Wo][147], column (c 7 + ky) 7 + kx; 0 outside the image
    return tuple((fa.T @ fb).reshape(64, 3, 7, 7) for fa, fb in (
        (g, cols), (np.abs(g), np.abs(cols)), ((g != 0).astype(np.float64), (cols != 0).astype(np.float64))))


def to_torch_layout(slab, N, C, taps):
    """the kernels' slab column kk = t C + c  ->  torch's [N][C][taps]"""
    return np.ascontiguousarray(np.asarray(slab).reshape(N, taps, C).transpose(0, 2, 1))


def stem_columns(x, n, H, W, pixels=None):
    """[pixels][147] float array of the stem's gathered operand, column k = (c 7 + ky) 7 + kx, zero outside the image, for
    the output pixels ``pixels`` (linear indices over [n][Ho][Wo]; all of them when None).  Keeps x's dtype."""
    Ho, Wo = H // 2, W // 2
    xs = np.asarray(x).reshape(n, 3, H, W)
    xp = np.zeros((n, 3, H + 6, W + 6), xs.dtype)
    xp[:, :, 3:H + 3, 3:W + 3] = xs
    pix = np.arange(n * Ho * Wo) if pixels is None else np.asarray(pixels)
    img, oy, ox = pix // (Ho * Wo), (pix // Wo) % Ho, pix % Wo
    k = np.arange(147)
    c, ky, kx = k // 49, (k // 7) % 7, k % 7
    return xp[img[:, None], c[None, :], 2 * oy[:, None] + ky[None, :], 2 * ox[:, None] + kx[None, :]]
