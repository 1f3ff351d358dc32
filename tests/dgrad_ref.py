"""float64 restatement of the convolution backward of train_engine.conv_param_and_input_grads: the data gradient (the
transposed convolution, from its definition, and again by the two decompositions the engine uses for stride 2), the weight
gradient, the packed weight layouts as index formulas, grl_dilate2's three modes and the fused BatchNorm-backward epilogue of
the data-gradient GEMM.  numpy only; nothing here is written the way the kernels compute it unless its name says so.

Layouts: activations and their gradients are channels-last rows, dz[n Ho Wo][cout], x / dx[n H W][cin]; the weight is
torch's w[cout][cin][k][k].  Every sum is returned next to ``abs_terms``, the same sum over the absolute values of its
terms -- what the rounding-error bounds of dgrad_bounds.py are relative to."""
import numpy as np


def f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def out_hw(H, W, k, stride):
    pad = k // 2
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def _taps(Hin, Hout, k, stride, pad):
    """per ky: the output rows oy whose input row iy = stride * oy - pad + ky lies inside the map, as (oy slice, iy slice)"""
    out = []
    for ky in range(k):
        oys = [oy for oy in range(Hout) if 0 <= stride * oy - pad + ky < Hin]
        if not oys:
            out.append(None)
            continue
        lo, hi = oys[0], oys[-1] + 1
        out.append((slice(lo, hi), slice(stride * lo - pad + ky, stride * (hi - 1) - pad + ky + 1, stride)))
    return out


def dgrad(dz, w, n, H, W, Ho, Wo, k, stride, pad):
    """dx[img, iy, ix, c] = sum over (o, ky, kx, oy, ox) with iy = stride * oy - pad + ky, ix = stride * ox - pad + kx of
    dz[img, oy, ox, o] * w[o, c, ky, kx].  Returns (dx, abs_terms), both [n H W][cin]."""
    w = f64(w)
    cout, cin = w.shape[0], w.shape[1]
    g = f64(dz).reshape(n, Ho, Wo, cout)
    dx = np.zeros((n, H, W, cin))
    ab = np.zeros((n, H, W, cin))
    ty, tx = _taps(H, Ho, k, stride, pad), _taps(W, Wo, k, stride, pad)
    for ky in range(k):
        for kx in range(k):
            if ty[ky] is None or tx[kx] is None:
                continue
            (oy, iy), (ox, ix) = ty[ky], tx[kx]
            dx[:, iy, ix, :] += g[:, oy, ox, :] @ w[:, :, ky, kx]
            ab[:, iy, ix, :] += np.abs(g[:, oy, ox, :]) @ np.abs(w[:, :, ky, kx])
    return dx.reshape(n * H * W, cin), ab.reshape(n * H * W, cin)


def parity_taps(p):
    """the taps of a 3x3 stride-2 pad-1 convolution that reach an input row of parity p, in the order of the output rows
    a, a + 1 they belong to (input row 2 a + p): ky = 1 for p = 0; ky = 2 then 0 for p = 1"""
    return [1] if p == 0 else [2, 0]


def dgrad_by_parity(dz, w, n, H, W, Ho, Wo):
    """The data gradient of a 3x3 stride-2 pad-1 convolution on an even map (H = 2 Ho, W = 2 Wo), class by class: input
    pixel (2 a + py, 2 b + px) receives dz[a + i][b + j] . w[:, :, parity_taps(py)[i], parity_taps(px)[j]], and nothing
    from an output row a + 1 == Ho or column b + 1 == Wo.  Returns (dx, abs_terms, terms): terms[row] = taps of that
    pixel's class, (1 + py) (1 + px)."""
    assert H == 2 * Ho and W == 2 * Wo
    w = f64(w)
    cout, cin = w.shape[0], w.shape[1]
    g = f64(dz).reshape(n, Ho, Wo, cout)
    gp = np.zeros((n, Ho + 1, Wo + 1, cout))
    gp[:, :Ho, :Wo] = g
    dx = np.zeros((n, H, W, cin))
    ab = np.zeros((n, H, W, cin))
    terms = np.zeros((n, H, W, 1))
    for py in (0, 1):
        for px in (0, 1):
            for i, ky in enumerate(parity_taps(py)):
                for j, kx in enumerate(parity_taps(px)):
                    s = gp[:, i:i + Ho, j:j + Wo, :]
                    dx[:, py::2, px::2, :] += s @ w[:, :, ky, kx]
                    ab[:, py::2, px::2, :] += np.abs(s) @ np.abs(w[:, :, ky, kx])
            terms[:, py::2, px::2, :] = (1 + py) * (1 + px)
    return dx.reshape(-1, cin), ab.reshape(-1, cin), terms.reshape(-1, 1)


def dgrad_by_zero_stuffing(dz, w, n, H, W, Ho, Wo):
    """The same data gradient for any map: dz zero-stuffed to the input's resolution (up[2 oy][2 ox] = dz[oy][ox]) and
    correlated, stride 1 and pad 1, with the flipped taps: dx[iy][ix] = sum_t up[iy - 1 + ty][ix - 1 + tx] . w[:, :, 2 - ty,
    2 - tx].  Returns (dx, abs_terms)."""
    w = f64(w)
    cout, cin = w.shape[0], w.shape[1]
    up = dilate2(dz, None, n, Ho, Wo, H, W, cout, 0, 0, 0).reshape(n, H, W, cout)
    pad = np.zeros((n, H + 2, W + 2, cout))
    pad[:, 1:H + 1, 1:W + 1] = up
    dx = np.zeros((n, H, W, cin))
    ab = np.zeros((n, H, W, cin))
    for ty in range(3):
        for tx in range(3):
            s = pad[:, ty:ty + H, tx:tx + W, :]
            dx += s @ w[:, :, 2 - ty, 2 - tx]
            ab += np.abs(s) @ np.abs(w[:, :, 2 - ty, 2 - tx])
    return dx.reshape(-1, cin), ab.reshape(-1, cin)


def wgrad(dz, x, n, H, W, Ho, Wo, k, stride, pad):
    """dw[o, c, ky, kx] = sum over (img, oy, ox) of dz[img, oy, ox, o] * x[img, stride * oy - pad + ky, stride * ox - pad +
    kx, c] (inside the map).  Returns (dw, abs_terms), both [cout][cin][k][k]."""
    g = f64(dz).reshape(n, Ho, Wo, -1)
    xs = f64(x).reshape(n, H, W, -1)
    cout, cin = g.shape[3], xs.shape[3]
    dw = np.zeros((cout, cin, k, k))
    ab = np.zeros((cout, cin, k, k))
    ty, tx = _taps(H, Ho, k, stride, pad), _taps(W, Wo, k, stride, pad)
    for ky in range(k):
        for kx in range(k):
            if ty[ky] is None or tx[kx] is None:
                continue
            (oy, iy), (ox, ix) = ty[ky], tx[kx]
            a, b = g[:, oy, ox, :].reshape(-1, cout), xs[:, iy, ix, :].reshape(-1, cin)
            dw[:, :, ky, kx] = a.T @ b
            ab[:, :, ky, kx] = np.abs(a).T @ np.abs(b)
    return dw, ab


# ----------------------------------------------------------------------------------------------------------------------
# packed layouts, as index formulas
def pack_dgrad(w):
    """grl_pack_dgrad_weight: out[c][taps - 1 - t][n] = w[n][c][t]  ->  [cin][taps * cout]"""
    w = np.asarray(w)
    n, c = w.shape[0], w.shape[1]
    taps = w.shape[2] * w.shape[3]
    out = np.empty((c, taps, n), w.dtype)
    for t in range(taps):
        out[:, taps - 1 - t, :] = w.reshape(n, c, taps)[:, :, t].T
    return out.reshape(c, taps * n)


def w_dgrad_s2(w, py, px):
    """Tape.w_dgrad_s2: out[c][i][j][n] = w[n][c][parity_taps(py)[i]][parity_taps(px)[j]]  ->  [cin][(1 + py)(1 + px) cout]"""
    w = np.asarray(w)
    n, c = w.shape[0], w.shape[1]
    kys, kxs = parity_taps(py), parity_taps(px)
    out = np.empty((c, len(kys), len(kxs), n), w.dtype)
    for i, ky in enumerate(kys):
        for j, kx in enumerate(kxs):
            out[:, i, j, :] = w[:, :, ky, kx].T
    return out.reshape(c, -1)


def transpose(x, R, C, ld):
    """grl_transpose: y[c][r] = x.flat[r * ld + c] for r < R, c < C"""
    flat = np.asarray(x).reshape(-1)
    out = np.empty((C, R), flat.dtype)
    for r in range(R):
        out[:, r] = flat[r * ld:r * ld + C]
    return out


def dilate2_hit(n, Ho, Wo, H, W, oy_off, ox_off):
    """[n H W] bool: the pixels (y, x) of the class, y % 2 == oy_off, x % 2 == ox_off, whose source (y // 2, x // 2) exists"""
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    hit = (y % 2 == oy_off) & (x % 2 == ox_off) & (y // 2 < Ho) & (x // 2 < Wo)
    return np.broadcast_to(hit[None], (n, H, W)).reshape(-1)


def dilate2(dz, up0, n, Ho, Wo, H, W, C, accumulate, oy_off, ox_off):
    """grl_dilate2 on rows: at the class pixels up[img][y][x] = dz[img][y // 2][x // 2] (modes 0 and 2) or up0 + dz
    (mode 1); every other pixel is 0 (mode 0) or left as it was (modes 1 and 2).  Keeps dz's dtype (mode 1 adds in it)."""
    dz = np.asarray(dz).reshape(n, Ho, Wo, C)
    hit = dilate2_hit(n, Ho, Wo, H, W, oy_off, ox_off).reshape(n, H, W)
    yy = np.minimum(np.arange(H) // 2, Ho - 1)
    xx = np.minimum(np.arange(W) // 2, Wo - 1)
    src = dz[:, yy][:, :, xx]                                   # [n][H][W][C]: the source pixel of every (y, x)
    if accumulate == 0:
        up = np.where(hit[..., None], src, np.zeros((), dz.dtype))
    else:
        up0 = np.asarray(up0).reshape(n, H, W, C)
        up = np.where(hit[..., None], src + up0 if accumulate == 1 else src, up0)
    return up.reshape(n * H * W, C)


# ----------------------------------------------------------------------------------------------------------------------
def unpack_bits(bits, count):
    """the ReLU mask bytes of grl_bn_apply_centered (fp32 storage: four outputs per byte, bit e of byte i = output 4 i + e)"""
    b = np.asarray(bits, np.uint8)[:count // 4]
    return ((b[:, None] >> np.arange(4, dtype=np.uint8)[None, :]) & 1).astype(bool).reshape(-1)


def fused_epilogue(acc, res, z, mean, invstd, mscale=None, mbeta=None, bits=None):
    """The data-gradient GEMM's BatchNorm-backward epilogue (GrlGemm.bn_z): g = (acc + res) * mask, where the mask is
    ``bits`` (bool [M][N]) if given and (z - mean) * mscale + mbeta > 0 otherwise; and the column sums of g and of
    g * xhat, xhat = (z - mean) * invstd.  Returns dict: g, mask, pre (the pre-activation the mask was taken from, None
    with bits), xhat, sum_g, sum_gx."""
    acc, z = f64(acc), f64(z)
    v = acc if res is None else acc + f64(res)
    zc = z - f64(mean)[None, :]
    pre = None
    if bits is not None:
        mask = np.asarray(bits, bool).reshape(z.shape)
    else:
        pre = zc * f64(mscale)[None, :] + (0.0 if mbeta is None else f64(mbeta)[None, :])
        mask = pre > 0
    g = np.where(mask, v, 0.0)
    xhat = zc * f64(invstd)[None, :]
    return dict(g=g, mask=mask, pre=pre, xhat=xhat, sum_g=g.sum(0), sum_gx=(g * xhat).sum(0), v=v)
