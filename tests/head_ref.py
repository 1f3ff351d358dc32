"""The gate, TRL and Siamese head kernels restated in float64 (numpy only): the independent reference of the fp32 kernels of
grl_amd/csrc/train_head.hip and of the eval-side forward kernels of pointwise.hip that they differentiate.

One function per kernel, with the arguments of its C ABI wrapper (include/grl_hip.h): device buffers are 1-D float64 arrays
that start where the pointer points, leading dimensions / strides and accumulate flags are taken as the wrapper takes them.
A destination that the kernel writes THROUGH a leading dimension, or accumulates into, is handed over with its contents
before the call (``*0`` arguments) and comes back whole: what the kernel may not touch is in it unchanged.  Next to its
results every function returns the sums of absolute terms that the bounds of tests/head_bounds.py are built from.

Written from the formulas -- autograd of reid/models/basebranch.py:58-66 (the gate), grl_model.py:137-178, 222-226 (TRL
reductions, channel attention, the L2-normalised tail) and Siamese.py:85-140 (attention pooling, pair head) -- not from
the kernel bodies.  The norms divide with no epsilon where the model does: an all-zero row is outside the contract."""
import numpy as np


def f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def flat(a):
    return None if a is None else np.ascontiguousarray(f64(a)).reshape(-1)


def view(buf, rows, cols, ld, start=0):
    """rows x cols window of the flat buffer ``buf``: element (r, c) at start + r * ld + c.  Writable."""
    assert buf.ndim == 1 and rows >= 1 and cols >= 0 and (ld >= cols or rows == 1)
    assert start >= 0 and start + (rows - 1) * ld + cols <= buf.size, (start, rows, cols, ld, buf.size)
    return np.lib.stride_tricks.as_strided(buf[start:], (rows, cols), (ld * buf.itemsize, buf.itemsize))


def sigmoid(z):
    z = f64(z)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


# ----------------------------------------------------------------------------------------------------------------------
# the GCE gate
def gce_gate(h, w3, bn_scale, bn_shift, x, M, Ch, C):
    """logit[m] = (h[m] . w3) * bn_scale + bn_shift; map = sigmoid(logit); xc = x map; xu = x (1 - map)."""
    h, x = view(flat(h), M, Ch, Ch), view(flat(x), M, C, C)
    w3 = flat(w3)[:Ch]
    sc, sh = float(flat(bn_scale)[0]), float(flat(bn_shift)[0])
    s = h @ w3
    z = s * sc + sh
    g = sigmoid(z)
    return dict(s=s, abs_s=np.abs(h) @ np.abs(w3), logit=z, abs_logit=np.abs(s * sc) + abs(sh), cmap=g,
                xc=x * g[:, None], xu=x * (1.0 - g)[:, None])


def gate_apply(y, ldy, x, M, C):
    """map[m] = sigmoid(y[m * ldy]); xc = x map; xu = x (1 - map)."""
    z = view(flat(y), M, 1, ldy)[:, 0]
    x = view(flat(x), M, C, C)
    g = sigmoid(z)
    return dict(logit=z, cmap=g, xc=x * g[:, None], xu=x * (1.0 - g)[:, None])


def gate_bwd(dxc, dxu, x, cmap, dx0, accumulate, dy0, ldy, M, C):
    """dx (+)= dxc map + dxu (1 - map);  dy[m * ldy] = map (1 - map) sum_c (dxc - dxu) x  (the other columns of dy stay)."""
    a, b, x = (view(flat(t), M, C, C) for t in (dxc, dxu, x))
    g = flat(cmap)[:M, None]
    dx = a * g + b * (1.0 - g)
    abs_dx = np.abs(a * g) + np.abs(b * (1.0 - g))
    if accumulate:
        d0 = view(flat(dx0), M, C, C)
        dx, abs_dx = dx + d0, abs_dx + np.abs(d0)
    s = ((a - b) * x).sum(1)
    dy = flat(dy0).copy()
    view(dy, M, 1, ldy)[:, 0] = s * g[:, 0] * (1.0 - g[:, 0])
    return dict(dx=dx, abs_dx=abs_dx, s=s, abs_s=np.abs((a - b) * x).sum(1), dy=dy, dy_col=view(dy, M, 1, ldy)[:, 0].copy(),
                g=g[:, 0].copy(), gg=g[:, 0] * (1.0 - g[:, 0]))


# ----------------------------------------------------------------------------------------------------------------------
# TRL reductions
def group_mean(x, y0, groups, rows, C, ldy, out_scale, accumulate):
    """y[g * ldy + c] (+)= out_scale / rows * sum_r x[g][r][c]."""
    x = flat(x)[:groups * rows * C].reshape(groups, rows, C)
    m = x.sum(1) * (float(out_scale) / rows)
    abs_m = np.abs(x).sum(1) * abs(float(out_scale) / rows)
    y = flat(y0).copy()
    yv = view(y, groups, C, ldy)
    yv[:] = m + (yv if accumulate else 0.0)
    return dict(y=y, val=yv.copy(), mean=m, abs_mean=abs_m)


def temporal_mean(x, b, T, inner):
    """y[b][r] = mean_t x[b][t][r]."""
    x = flat(x)[:b * T * inner].reshape(b, T, inner)
    return dict(y=x.mean(1), abs_y=np.abs(x).mean(1))


def sqdiff_mean(f1, f2, b, rows, C, f2_clip_stride):
    """d[b][c] = mean_r (f1[b][r][c] - f2[b * f2_clip_stride + r * C + c])^2."""
    f1 = flat(f1)[:b * rows * C].reshape(b, rows, C)
    f2 = np.stack([view(flat(f2), rows, C, C, i * f2_clip_stride) for i in range(b)])
    t = f1 - f2
    return dict(d=(t * t).mean(1))


def sqdiff_bwd(f1, f2, dd, df2_0, b, rows, C, f2_clip_stride, accumulate_df2):
    """df1[b][r][c] = 2 (f1 - f2) dd[b][c] / rows;   df2[b * stride + r * C + c] (+)= -df1."""
    f1 = flat(f1)[:b * rows * C].reshape(b, rows, C)
    f2 = np.stack([view(flat(f2), rows, C, C, i * f2_clip_stride) for i in range(b)])
    dd = flat(dd)[:b * C].reshape(b, 1, C)
    g = 2.0 * (f1 - f2) * dd / rows
    df2 = flat(df2_0).copy()
    vals = np.empty_like(g)
    for i in range(b):
        v = view(df2, rows, C, C, i * f2_clip_stride)
        v[:] = -g[i] + (v if accumulate_df2 else 0.0)
        vals[i] = v
    return dict(df1=g, df2=df2, df2_val=vals)


def add_strided(a, bsrc, nb, inner, b_clip_stride):
    """y[b][r] = a[b][r] + bsrc[b * b_clip_stride + r]."""
    a = flat(a)[:nb * inner].reshape(nb, inner)
    return dict(y=a + view(flat(bsrc), nb, inner, b_clip_stride))


def mean_T(x, y0, b, T, C, ldy):
    """y[b * ldy + c] = mean_t x[b][t][c]."""
    x = flat(x)[:b * T * C].reshape(b, T, C)
    y = flat(y0).copy()
    view(y, b, C, ldy)[:] = x.mean(1)
    return dict(y=y, val=x.mean(1), abs_val=np.abs(x).mean(1))


def add_rowbcast(dst0, v, M, C, rows_per_group, scale, accumulate):
    """dst[m][c] (+)= v[m // rows_per_group][c] * scale   (the backward of a mean over rows_per_group rows)."""
    groups = (M + rows_per_group - 1) // rows_per_group
    v = flat(v)[:groups * C].reshape(groups, C)
    t = v[np.arange(M) // rows_per_group] * float(scale)
    d0 = flat(dst0)[:M * C].reshape(M, C)
    return dict(dst=t + (d0 if accumulate else 0.0), term=t)


# ----------------------------------------------------------------------------------------------------------------------
# channel attention of one TRL step
def channel_atte(d, w1, w2t, gap, gap_stride, want_catte, fstep0, fstep_stride, accumulate, b, C, Hd):
    """hid = relu(W1 d);  c = sigmoid(W2 hid)  (w2t = W2 transposed, [Hd][C]);  fstep (+)= gap c + gap.
    gap / fstep: row i at i * stride.  ``want_catte`` False = the NULL catte of the wrapper."""
    d = flat(d)[:b * C].reshape(b, C)
    w1, w2t = flat(w1)[:Hd * C].reshape(Hd, C), flat(w2t)[:Hd * C].reshape(Hd, C)
    pre = d @ w1.T
    hid = np.maximum(pre, 0.0)
    z = hid @ w2t
    a = sigmoid(z)
    g = view(flat(gap), b, C, gap_stride)
    o = g * a + g
    fs = flat(fstep0).copy()
    fv = view(fs, b, C, fstep_stride)
    fv[:] = o + (fv if accumulate else 0.0)
    return dict(hid=hid, abs_hid=np.abs(d) @ np.abs(w1).T, logit=z, catte=a if want_catte else None, a=a, gap=g.copy(),
                term=o, fstep=fs, fstep_val=fv.copy(), w2t=w2t)


def catte_bwd(dfs, dfs_stride, gap, gap_stride, catte, dgap0, dgap_stride, accumulate, b, C):
    """fstep = gap c + gap:  ds = dfs gap c (1 - c)  (the gradient of the sigmoid's argument);  dgap (+)= dfs (1 + c)."""
    d, g = view(flat(dfs), b, C, dfs_stride), view(flat(gap), b, C, gap_stride)
    a = flat(catte)[:b * C].reshape(b, C)
    t = d * (1.0 + a)
    dg = flat(dgap0).copy()
    gv = view(dg, b, C, dgap_stride)
    gv[:] = t + (gv if accumulate else 0.0)
    return dict(ds=d * g * a * (1.0 - a), dgap=dg, dgap_val=gv.copy(), term=t, dfs=d.copy(), gap=g.copy())


# ----------------------------------------------------------------------------------------------------------------------
# the L2-normalised tail
def affine_l2norm(x, scale, shift, y0, rows, C, ldy):
    """v = x scale + shift (scale / shift None: v = x);  y[row * ldy + c] = v / |v|."""
    x = view(flat(x), rows, C, C)
    v, abs_v = x, np.abs(x)
    if scale is not None:
        sc, sh = flat(scale)[:C], flat(shift)[:C]
        v, abs_v = x * sc + sh, np.abs(x * sc) + np.abs(sh)
    ss = (v * v).sum(1)
    y = flat(y0).copy()
    view(y, rows, C, ldy)[:] = v / np.sqrt(ss)[:, None]
    return dict(y=y, val=v / np.sqrt(ss)[:, None], v=v, abs_v=abs_v, ss=ss)


def l2norm_bwd(dy, lddy, y, ldy, v, rows, C):
    """y = v / |v|:  dv = (dy - y (y . dy)) / |v|, with the forward's y as an argument."""
    a, b = view(flat(dy), rows, C, lddy), view(flat(y), rows, C, ldy)
    v = view(flat(v), rows, C, C)
    dot = (a * b).sum(1)
    ss = (v * v).sum(1)
    return dict(dv=(a - b * dot[:, None]) / np.sqrt(ss)[:, None], dot=dot, abs_dot=np.abs(a * b).sum(1), ss=ss,
                dy=a.copy(), y=b.copy())


def row_sqnorm(x, rows, K, ld):
    """out[row] = sum_k x[row * ld + k]^2."""
    x = view(flat(x), rows, K, ld)
    return dict(out=(x * x).sum(1))


# ----------------------------------------------------------------------------------------------------------------------
# Siamese temporal attention
def siamese_attn(qk, x, pooled0, b, T, D, C, ldy):
    """qk[b][t] = (Q_t | K_t), 2 D wide.  qh = Q / |Q|, kh = K / |K|; S = qh kh^T; P = softmax_j S; w_j = sum_i P_ij;
    raw = sum_j w_j x_j;  pooled[b * ldy + c] = raw / |raw|.  Returns every intermediate (the backward and the bounds use them)."""
    qk = flat(qk)[:b * T * 2 * D].reshape(b, T, 2, D)
    x = flat(x)[:b * T * C].reshape(b, T, C)
    q, k = qk[:, :, 0], qk[:, :, 1]
    nq, nk = np.sqrt((q * q).sum(2)), np.sqrt((k * k).sum(2))
    qh, kh = q / nq[..., None], k / nk[..., None]
    S = np.einsum('bid,bjd->bij', qh, kh)
    abs_S = np.einsum('bid,bjd->bij', np.abs(qh), np.abs(kh))
    e = np.exp(S - S.max(2, keepdims=True))
    P = e / e.sum(2, keepdims=True)
    w = P.sum(1)
    raw = np.einsum('bj,bjc->bc', w, x)
    nraw = np.sqrt((raw * raw).sum(1))
    out = raw / nraw[:, None]
    pooled = flat(pooled0).copy()
    view(pooled, b, C, ldy)[:] = out
    return dict(pooled=pooled, out=out, q=q, k=k, nq=nq, nk=nk, qh=qh, kh=kh, S=S, abs_S=abs_S, P=P, w=w, raw=raw, nraw=nraw, x=x)


def siamese_attn_bwd(qk, x, out, ldo, dout, lddo, dx0, dx_accumulate, b, T, D, C):
    """Backward of siamese_attn with the forward's ``out`` as an argument:
    draw = (dout - out (out . dout)) / |raw|;  dx_j (+)= w_j draw;  dw_j = draw . x_j;  dP_ij = dw_j;
    dS_ij = P_ij (dP_ij - sum_k P_ik dP_ik);  dqh_i = sum_j dS_ij kh_j;  dkh_j = sum_i dS_ij qh_i;
    dQ = (dqh - qh (qh . dqh)) / |Q|, dK likewise.  Returns dqk[b][T][2 D], dx[b][T][C] and the intermediates."""
    fw = siamese_attn(qk, x, np.zeros(b * C), b, T, D, C, C)
    o, do = view(flat(out), b, C, ldo), view(flat(dout), b, C, lddo)
    od = (o * do).sum(1)
    draw = (do - o * od[:, None]) / fw['nraw'][:, None]
    dxt = fw['w'][:, :, None] * draw[:, None, :]
    dx = dxt + (flat(dx0)[:b * T * C].reshape(b, T, C) if dx_accumulate else 0.0)
    dw = np.einsum('bc,bjc->bj', draw, fw['x'])
    P = fw['P']
    sp = np.einsum('bik,bk->bi', P, dw)
    dS = P * (dw[:, None, :] - sp[:, :, None])
    dqh = np.einsum('bij,bjd->bid', dS, fw['kh'])
    dkh = np.einsum('bij,bid->bjd', dS, fw['qh'])
    dq = (dqh - fw['qh'] * (fw['qh'] * dqh).sum(2, keepdims=True)) / fw['nq'][..., None]
    dk = (dkh - fw['kh'] * (fw['kh'] * dkh).sum(2, keepdims=True)) / fw['nk'][..., None]
    return dict(dqk=np.stack([dq, dk], 2), dx=dx, dx_term=dxt, fw=fw, out=o.copy(), dout=do.copy(), od=od, draw=draw, dw=dw,
                sp=sp, dS=dS, dqh=dqh, dkh=dkh)


# ----------------------------------------------------------------------------------------------------------------------
# the pair head
def pair_sqdiff(p, g, np_, ng, K):
    """diff[i * ng + j][k] = (p[i][k] - g[j][k])^2."""
    p, g = flat(p)[:np_ * K].reshape(np_, 1, K), flat(g)[:ng * K].reshape(1, ng, K)
    return dict(diff=((p - g) ** 2).reshape(np_ * ng, K))


def pair_sqdiff_bwd(p, g, ddiff, np_, ng, K):
    """dp[i] = sum_j 2 (p_i - g_j) ddiff_ij;   dg[j] = -sum_i 2 (p_i - g_j) ddiff_ij."""
    p, g = flat(p)[:np_ * K].reshape(np_, 1, K), flat(g)[:ng * K].reshape(1, ng, K)
    t = 2.0 * (p - g) * flat(ddiff)[:np_ * ng * K].reshape(np_, ng, K)
    return dict(dp=t.sum(1), dg=-t.sum(0), abs_dp=np.abs(t).sum(1), abs_dg=np.abs(t).sum(0))


def pair_verify(p, g, scale, shift, w, bias, np_, ng, K, ncls):
    """out[i][j][c] = bias[c] + sum_k W[c][k] (scale[k] (p[i][k] - g[j][k])^2 + shift[k])   (scale / shift, bias: None = absent)."""
    d = pair_sqdiff(p, g, np_, ng, K)['diff']
    e, abs_e = d, d
    if scale is not None:
        sc, sh = flat(scale)[:K], flat(shift)[:K]
        e, abs_e = d * sc + sh, np.abs(d * sc) + np.abs(sh)
    w = flat(w)[:ncls * K].reshape(ncls, K)
    out = e @ w.T
    if bias is not None:
        out = out + flat(bias)[:ncls]
    return dict(out=out.reshape(np_, ng, ncls), abs_out=(abs_e @ np.abs(w).T).reshape(np_, ng, ncls))
