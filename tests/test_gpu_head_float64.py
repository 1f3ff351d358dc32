"""The fp32 gate, TRL and Siamese head kernels (train_head.hip, and the forward kernels of pointwise.hip they differentiate)
against the float64 restatement of tests/head_ref.py, through the C ABI, on a real MI355X.

Every comparison is per element against that element's derived bound (tests/head_bounds.py) -- never a norm over the
tensor.  A backward that reads a forward kernel's fp32 output (cmap, catte, y, out) is compared with the reference evaluated
on those very fp32 values: a stage answers for its own roundings only; the "end to end" stages then take nothing from the
kernels and carry the forward's own error through the derivative.

Every output lives in a buffer filled with a sentinel that is longer (and, with ld > C, wider) than the kernel may write;
the overwrite forms start from the sentinel and must not depend on it, the accumulate forms start from random values.
Every pointer is 16-byte aligned (sub-views start at a multiple of 4 floats): the kernels load float4."""
import ctypes as C_

import numpy as np
import pytest
import torch

import head_bounds as B
import head_ref as R

pytestmark = pytest.mark.gpu

SENT = 12345.0
GUARD = 64                      # sentinel floats behind every output


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    yield
    B.dump_ratios('MI355X head kernels')


def _te():
    from grl_amd import train_engine as TE
    return TE


def _err():
    from grl_amd._lib import GrlHipError
    return GrlHipError


def _call(name, *args):
    TE = _te()
    TE._call(name, *[TE.ptr(a) if torch.is_tensor(a) else a for a in args])


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _n(t):
    return t.detach().cpu().numpy()


def _f(v):
    return C_.c_float(v)


def _at(t, floats):
    """device address `floats` floats into t (a multiple of 4: 16-byte aligned)"""
    assert floats % 4 == 0 and t.data_ptr() % 16 == 0
    return t.data_ptr() + 4 * floats


def _out(n, init=None):
    """n output floats (the sentinel, or `init`) with GUARD sentinel floats behind them"""
    t = torch.full((n + GUARD,), SENT, device='cuda')
    if init is not None:
        t[:n] = _d(init).reshape(-1)
    return t


def _got(t, n):
    """the n output floats on the host; nothing behind them was written"""
    torch.cuda.synchronize()
    a = _n(t)
    assert (a[n:] == SENT).all(), 'written past the end of the output'
    return a[:n]


def _window(flat_, rows, cols, ld, before, start=0):
    """the rows x cols window (leading dimension ld) of a flat output; everything outside it equals `before`"""
    keep = np.ones(flat_.size, bool)
    idx = start + (np.arange(rows) * ld)[:, None] + np.arange(cols)[None, :]
    keep[idx.reshape(-1)] = False
    assert np.array_equal(flat_[keep], np.asarray(before, np.float32).reshape(-1)[keep]), 'written outside the destination window'
    return flat_[idx]


class _Inputs(object):
    """device copies of the inputs of a case; `unchanged()` after the launches: no kernel wrote to one"""

    def __init__(self, **arrays):
        self.h = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in arrays.items()}
        self.t = {k: _d(v) for k, v in self.h.items()}

    def __getitem__(self, k):
        return self.t[k]

    def unchanged(self):
        torch.cuda.synchronize()
        for k, v in self.h.items():
            assert np.array_equal(_n(self.t[k]).reshape(-1), v.reshape(-1)), 'input %s was written' % k


# ----------------------------------------------------------------------------------------------------------------------
# the gate
@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('M,C,ldy', B.GATE_CASES)
def test_gate_apply_and_bwd(M, C, ldy, cls):
    """grl_gate_apply: bounds b_gate_apply.  grl_gate_bwd on the kernel's own cmap, overwrite and accumulate (b_gate_bwd);
    only column 0 of dy's rows is written.  Then end to end: the float64 chain on the float64 map."""
    d = B.in_gate(M, C, ldy, cls)
    t = _Inputs(y=d['y'], x=d['x'], dxc=d['dxc'], dxu=d['dxu'])
    cmap, xc, xu = _out(M), _out(M * C), _out(M * C)
    _call('grl_gate_apply', t['y'], ldy, t['x'], cmap, xc, xu, M, C)
    ref = R.gate_apply(d['y'], ldy, d['x'], M, C)
    bd = B.b_gate_apply(ref, d['x'])
    what = (M, C, ldy, cls)
    cm = _got(cmap, M)
    B.check('gate_apply cmap', cm, ref['cmap'], bd['cmap'], what)
    B.check('gate_apply xc', _got(xc, M * C).reshape(M, C), ref['xc'], bd['xc'], what)
    B.check('gate_apply xu', _got(xu, M * C).reshape(M, C), ref['xu'], bd['xu'], what)
    col0 = np.arange(M) * ldy
    for acc in (0, 1):
        dy0 = d['dy0'].copy()
        if not acc:
            dy0[col0] = SENT
        dx, dy = _out(M * C, d['dx0'] if acc else None), _out(M * ldy, dy0)
        _call('grl_gate_bwd', t['dxc'], t['dxu'], t['x'], cmap, dx, acc, dy, ldy, M, C)
        bw = R.gate_bwd(d['dxc'], d['dxu'], d['x'], cm, d['dx0'], acc, dy0, ldy, M, C)
        bb = B.b_gate_bwd(bw, C, acc)
        B.check('gate_bwd dx', _got(dx, M * C).reshape(M, C), bw['dx'], bb['dx'], what + (acc,))
        B.check('gate_bwd dy', _window(_got(dy, M * ldy), M, 1, ldy, dy0)[:, 0], bw['dy_col'], bb['dy'], what + (acc,))
        if not acc:
            e2e = R.gate_bwd(d['dxc'], d['dxu'], d['x'], ref['cmap'], d['dx0'], 0, dy0, ldy, M, C)
            be = B.b_gate_bwd(e2e, C, 0, B.e_sigmoid(ref['logit']), d['dxc'], d['dxu'])
            B.check('end to end gate dx', _got(dx, M * C).reshape(M, C), e2e['dx'], be['dx'], what)
            B.check('end to end gate dy', _got(dy, M * ldy)[col0], e2e['dy_col'], be['dy'], what)
    assert np.array_equal(_got(cmap, M), cm)
    t.unchanged()


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('M,Ch,C', B.GCE_CASES)
def test_gce_gate(M, Ch, C, cls):
    """grl_gce_gate with and without a corr_map destination (b_gce_gate: the wave dot, the folded BN, the sigmoid)."""
    d = B.in_gce(M, Ch, C, cls)
    t = _Inputs(**d)
    ref = R.gce_gate(d['h'], d['w3'], d['bsc'], d['bsh'], d['x'], M, Ch, C)
    bd = B.b_gce_gate(ref, d['x'], d['bsc'][0], Ch)
    for with_map in (True, False):
        cmap, xc, xu = _out(M), _out(M * C), _out(M * C)
        _call('grl_gce_gate', t['h'], t['w3'], t['bsc'], t['bsh'], t['x'], cmap if with_map else None, xc, xu, M, Ch, C)
        what = (M, Ch, C, cls, with_map)
        if with_map:
            B.check('gce_gate cmap', _got(cmap, M), ref['cmap'], bd['cmap'], what)
        else:
            assert (_got(cmap, M) == SENT).all()
        B.check('gce_gate xc', _got(xc, M * C).reshape(M, C), ref['xc'], bd['xc'], what)
        B.check('gce_gate xu', _got(xu, M * C).reshape(M, C), ref['xu'], bd['xu'], what)
    t.unchanged()


# ----------------------------------------------------------------------------------------------------------------------
# TRL reductions
@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('groups,rows,C,ld_extra,f2_mult', B.RED_CASES)
def test_group_mean_sqdiff_mean_and_bwd(groups, rows, C, ld_extra, f2_mult, cls):
    """grl_group_mean (scale, accumulate, ldy), grl_sqdiff_mean and grl_sqdiff_bwd (df2 overwritten / accumulated) with f2 and
    df2 as windows that start F2_OFFSET floats inside wider buffers, clip stride rows C or 2 rows C."""
    d = B.in_red(groups, rows, C, f2_mult, cls)
    t = _Inputs(x=d['x'], f1=d['f1'], f2buf=d['f2buf'], dd=d['dd'])
    ldy = C + ld_extra
    what = (groups, rows, C, ld_extra, f2_mult, cls)
    r = B.rng_for('y0', groups, rows, C)
    for scale, acc in ((1.0, 0), (0.5, 1), (2.0, 0)):
        y0 = B.normal(r, groups * ldy, 'a') if acc else np.full(groups * ldy, SENT, np.float32)
        if acc and ld_extra:
            y0.reshape(groups, ldy)[:, C:] = SENT
        y = _out(groups * ldy, y0)
        _call('grl_group_mean', t['x'], y, groups, rows, C, ldy, _f(scale), acc)
        ref = R.group_mean(d['x'], y0, groups, rows, C, ldy, scale, acc)
        B.check('group_mean', _window(_got(y, groups * ldy), groups, C, ldy, y0), ref['val'], B.b_group_mean(ref, rows, acc),
                what + (scale, acc))
    f2v = d['f2buf'][B.F2_OFFSET:]
    dm = _out(groups * C)
    _call('grl_sqdiff_mean', t['f1'], _at(t['f2buf'], B.F2_OFFSET), dm, groups, rows, C, d['stride'])
    ref = R.sqdiff_mean(d['f1'], f2v, groups, rows, C, d['stride'])
    B.check('sqdiff_mean', _got(dm, groups * C).reshape(groups, C), ref['d'], B.b_sqdiff_mean(ref, rows), what)
    _sqdiff_bwd(d, t, groups, rows, C, what)
    t.unchanged()


def _sqdiff_bwd(d, t, groups, rows, C, what):
    n2 = d['f2buf'].size
    for acc in (0, 1):
        df2_0 = d['df2buf'].copy()
        if not acc:
            for g in range(groups):
                o = B.F2_OFFSET + g * d['stride']
                df2_0[o:o + rows * C] = SENT
        df1, df2 = _out(groups * rows * C), _out(n2, df2_0)
        _call('grl_sqdiff_bwd', t['f1'], _at(t['f2buf'], B.F2_OFFSET), t['dd'], df1, _at(df2, B.F2_OFFSET), groups, rows, C,
              d['stride'], acc)
        bw = R.sqdiff_bwd(d['f1'], d['f2buf'][B.F2_OFFSET:], d['dd'], df2_0[B.F2_OFFSET:], groups, rows, C, d['stride'], acc)
        bb = B.b_sqdiff_bwd(bw, acc)
        B.check('sqdiff_bwd df1', _got(df1, groups * rows * C).reshape(groups, rows, C), bw['df1'], bb['df1'], what + (acc,))
        got = _got(df2, n2)
        keep = np.ones(n2, bool)
        vals = np.empty((groups, rows, C))
        for g in range(groups):
            o = B.F2_OFFSET + g * d['stride']
            keep[o:o + rows * C] = False
            vals[g] = got[o:o + rows * C].reshape(rows, C)
        assert np.array_equal(got[keep], df2_0[keep]), 'df2 written outside its windows'
        B.check('sqdiff_bwd df2', vals, bw['df2_val'], bb['df2'], what + (acc,))


def _temporal_mean(b, T, inner):
    r = B.rng_for('tm', b, T, inner)
    x = B.normal(r, (b, T, inner), 'a')
    t = _Inputs(x=x)
    y = _out(b * inner)
    _call('grl_temporal_mean', t['x'], y, b, T, inner)
    ref = R.temporal_mean(x, b, T, inner)
    B.check('temporal_mean', _got(y, b * inner).reshape(b, inner), ref['y'], B.b_mean_over_T(ref['abs_y'], T), (b, T, inner))
    t.unchanged()


def _add_strided(nb, inner, stride):
    r = B.rng_for('as', nb, inner, stride)
    a, bs = B.normal(r, (nb, inner), 'a'), B.normal(r, nb * stride, 'a')
    t = _Inputs(a=a, bs=bs)
    y = _out(nb * inner)
    _call('grl_add_strided', t['a'], t['bs'], y, nb, inner, stride)
    ref = R.add_strided(a, bs, nb, inner, stride)
    B.check('add_strided', _got(y, nb * inner).reshape(nb, inner), ref['y'], B.b_add_strided(ref), (nb, inner, stride))
    t.unchanged()


def _mean_T(b, T, C, ld):
    r = B.rng_for('mt', b, T, C, ld)
    x = B.normal(r, (b, T, C), 'a')
    t = _Inputs(x=x)
    y0 = np.full(b * ld, SENT, np.float32)
    y = _out(b * ld)
    _call('grl_mean_T', t['x'], y, b, T, C, ld)
    ref = R.mean_T(x, y0, b, T, C, ld)
    B.check('mean_T', _window(_got(y, b * ld), b, C, ld, y0), ref['val'], B.b_mean_over_T(ref['abs_val'], T), (b, T, C, ld))
    t.unchanged()


@pytest.mark.parametrize('T', B.EW_T)
@pytest.mark.parametrize('b,rows,C', B.EW_CASES)
def test_temporal_mean_add_strided_mean_T(b, rows, C, T):
    """grl_temporal_mean (T - 1 additions, fl(1 / T), the product), grl_add_strided (one addition; the second operand at a clip
    stride wider than the row), grl_mean_T (into ld = C and C + 8)."""
    _temporal_mean(b, T, rows * C)
    _add_strided(b, rows * C, T * rows * C + 4)
    _mean_T(b * rows, T, C, C + 8 * (T % 2))


def _add_rowbcast(M, Cc, rpg):
    r = B.rng_for('rowbcast', M, Cc, rpg)
    groups = (M + rpg - 1) // rpg
    v, dst0 = B.normal(r, (groups, Cc), 'a'), B.normal(r, (M, Cc), 'a')
    t = _Inputs(v=v)
    for scale, acc in ((1.0, 0), (1.0 / rpg, 1), (0.25, 0)):
        sc = float(np.float32(scale))
        dst = _out(M * Cc, dst0 if acc else None)
        _call('grl_add_rowbcast', dst, t['v'], M, Cc, rpg, _f(sc), acc)
        ref = R.add_rowbcast(dst0, v, M, Cc, rpg, sc, acc)
        B.check('add_rowbcast', _got(dst, M * Cc).reshape(M, Cc), ref['dst'], B.b_add_rowbcast(ref, acc), (M, Cc, rpg, scale, acc))
    t.unchanged()


@pytest.mark.parametrize('M,Cc,rpg', [(b * rows, Cc, rpg) for b, rows, Cc in B.EW_CASES for rpg in B.EW_RPG] + [B.ROWBCAST_SHORT])
def test_add_rowbcast(M, Cc, rpg):
    """grl_add_rowbcast: dst (+)= v[m // rows_per_group] * scale; M = 7 with 5 rows per group: the last group is short."""
    _add_rowbcast(M, Cc, rpg)


def _catte_bwd(b, Cc, cls, catte=None, e_a=None, ref_catte=None, tag='catte_bwd', T=B.CATTE_T):
    d = B.in_catte(b, 3, Cc, cls, T)
    st, off = T * Cc, (Cc if T > 1 else 0)          # the rows at step 1 of [b][T][C] buffers (T = 1: the buffers themselves)
    n = b * st
    if catte is None:
        catte = B.sigmoid_f32(B.normal(B.rng_for('a', b, Cc), (b, Cc), 'a') * np.float32(3))
    t = _Inputs(dfs=d['dfsbuf'], gap=d['gapbuf'], catte=catte)
    for acc in (0, 1):
        dg0 = d['dgapbuf'].copy()
        if not acc:
            for i in range(b):
                dg0[i * st + off:i * st + off + Cc] = SENT
        ds, dgap = _out(b * Cc), _out(n, dg0)
        _call('grl_catte_bwd', _at(t['dfs'], off), st, _at(t['gap'], off), st, t['catte'], ds, _at(dgap, off), st, acc, b, Cc)
        bw = R.catte_bwd(d['dfsbuf'][off:], st, d['gapbuf'][off:], st, catte if ref_catte is None else ref_catte, dg0[off:], st, acc, b, Cc)
        bb = B.b_catte_bwd(bw, catte if ref_catte is None else ref_catte, acc, e_a)
        B.check(tag + ' ds', _got(ds, b * Cc).reshape(b, Cc), bw['ds'], bb['ds'], (b, Cc, cls, acc))
        B.check(tag + ' dgap', _window(_got(dgap, n), b, Cc, st, dg0, off), bw['dgap_val'], bb['dgap'], (b, Cc, cls, acc))
    t.unchanged()


def _pair_sqdiff(n, g, K, cls):
    d = B.in_pair(n, g, K, cls)
    t = _Inputs(p=d['p'], g=d['g'])
    diff = _out(n * g * K)
    _call('grl_pair_sqdiff', t['p'], t['g'], diff, n, g, K)
    ref = R.pair_sqdiff(d['p'], d['g'], n, g, K)
    B.check('pair_sqdiff', _got(diff, n * g * K).reshape(n * g, K), ref['diff'], B.b_pair_sqdiff(ref), (n, g, K, cls))
    t.unchanged()
    return d, t


@pytest.mark.parametrize('name', sorted(B.BIG))
def test_grid_stride_tail(name):
    """One case per grid-stride kernel with just over 8192 * 256 float4 items: the grid is capped and the
    `i += gridDim.x * blockDim.x` tail of the loop runs."""
    case = B.BIG[name]
    assert B.big_items(name, case) > B.GRID_CAP
    if name == 'sqdiff_bwd':
        b, rows, Cc = case
        d = B.in_red(b, rows, Cc, 1, 'b')
        _sqdiff_bwd(d, _Inputs(f1=d['f1'], f2buf=d['f2buf'], dd=d['dd']), b, rows, Cc, case)
    elif name == 'add_rowbcast':
        _add_rowbcast(*case)
    elif name == 'catte_bwd':
        _catte_bwd(case[0], case[1], 'a', T=1)
    elif name == 'temporal_mean':
        _temporal_mean(*case)
    elif name == 'add_strided':
        _add_strided(case[0], case[1], case[1] + 8)
    elif name == 'mean_T':
        _mean_T(case[0], case[1], case[2], case[2])
    else:
        _pair_sqdiff(*case, cls='b')


# ----------------------------------------------------------------------------------------------------------------------
# channel attention
@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('b,Hd,Cc', B.CATTE_CASES)
def test_channel_atte_and_bwd(b, Hd, Cc, cls):
    """grl_channel_atte (both launches; catte present and NULL; fstep overwritten and accumulated; gap and fstep rows of
    [b][3][C] buffers at step 1) with the hidden units read back from the workspace, then grl_catte_bwd on the kernel's own
    catte, and end to end on the float64 one."""
    d = B.in_catte(b, Hd, Cc, cls)
    st, n = B.CATTE_T * Cc, b * B.CATTE_T * Cc
    t = _Inputs(d=d['d'], w1=d['w1'], w2t=d['w2t'], gap=d['gapbuf'])
    catte_k = None
    for acc, with_catte in ((0, True), (1, True), (0, False)):
        f0 = d['fstepbuf'].copy()
        if not acc:
            for i in range(b):
                f0[i * st + Cc:i * st + 2 * Cc] = SENT
        hid, catte, fstep = _out(b * Hd), _out(b * Cc), _out(n, f0)
        _call('grl_channel_atte', t['d'], t['w1'], t['w2t'], _at(t['gap'], Cc), st, catte if with_catte else None,
              _at(fstep, Cc), st, acc, b, Cc, Hd, hid)
        ref = R.channel_atte(d['d'], d['w1'], d['w2t'], d['gapbuf'][Cc:], st, with_catte, f0[Cc:], st, acc, b, Cc, Hd)
        bd = B.channel_atte_bounds(ref, Cc, Hd, acc)
        what = (b, Hd, Cc, cls, acc, with_catte)
        B.check('channel_atte hid', _got(hid, b * Hd).reshape(b, Hd), ref['hid'], bd['hid'], what)
        if with_catte:
            catte_k = _got(catte, b * Cc).reshape(b, Cc).copy()
            B.check('channel_atte catte', catte_k, ref['a'], bd['catte'], what)
        else:
            assert (_got(catte, b * Cc) == SENT).all()
        B.check('channel_atte fstep', _window(_got(fstep, n), b, Cc, st, f0, Cc), ref['fstep_val'], bd['fstep'], what)
    t.unchanged()
    if Hd == 3:                  # (the backward does not depend on Hd)
        _catte_bwd(b, Cc, cls, catte_k)
        _catte_bwd(b, Cc, cls, catte_k, bd['e_catte'], ref['a'], tag='end to end catte_bwd')


# ----------------------------------------------------------------------------------------------------------------------
# the L2-normalised tail
@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('rows,Cc,ld', B.BLOCK_CASES)
def test_l2norm_tail(rows, Cc, ld, cls):
    """grl_affine_l2norm with and without scale / shift into ld = C or C + 8; grl_l2norm_bwd on the kernel's own y (read through
    that ld, dy through another) and end to end on the float64 y; grl_row_sqnorm over rows of that ld."""
    d = B.in_l2(rows, Cc, cls)
    lddy = 2 * ld - Cc
    dyb = np.full(rows * lddy, SENT, np.float32)
    dyb.reshape(rows, lddy)[:, :Cc] = d['dy']
    t = _Inputs(x=d['x'], scale=d['scale'], shift=d['shift'], dyb=dyb)
    y0 = np.full(rows * ld, SENT, np.float32)
    for affine in (True, False):
        y = _out(rows * ld)
        _call('grl_affine_l2norm', t['x'], t['scale'] if affine else None, t['shift'] if affine else None, y, rows, Cc, ld)
        sc, sh = (d['scale'], d['shift']) if affine else (None, None)
        ref = R.affine_l2norm(d['x'], sc, sh, y0, rows, Cc, ld)
        bd = B.affine_l2norm_bounds(ref, Cc, affine)
        what = (rows, Cc, ld, cls, affine)
        yk = _got(y, rows * ld)
        B.check('affine_l2norm', _window(yk, rows, Cc, ld, y0), ref['val'], bd['y'], what)
    # backward of y = v / |v| (no affine: v = x), y as the kernel left it
    dv = _out(rows * Cc)
    _call('grl_l2norm_bwd', t['dyb'], lddy, y, ld, t['x'], dv, rows, Cc)
    got = _got(dv, rows * Cc).reshape(rows, Cc)
    bw = R.l2norm_bwd(dyb, lddy, yk, ld, d['x'], rows, Cc)
    B.check('l2norm_bwd', got, bw['dv'], B.b_l2norm_bwd(bw, Cc), what)
    ybuf = y0.astype(np.float64)
    ybuf.reshape(rows, ld)[:, :Cc] = ref['val']
    e2e = R.l2norm_bwd(dyb, lddy, ybuf, ld, d['x'], rows, Cc)
    B.check('end to end l2norm_bwd', got, e2e['dv'], B.b_l2norm_bwd(e2e, Cc, bd['e_y']), what)
    assert np.array_equal(_got(y, rows * ld), yk)
    xs = B.normal(B.rng_for('sq', rows, Cc), (rows, ld), cls)
    xt, sq = _d(xs), _out(rows)
    _call('grl_row_sqnorm', xt, sq, rows, Cc, ld)
    rs = R.row_sqnorm(xs, rows, Cc, ld)
    B.check('row_sqnorm', _got(sq, rows), rs['out'], B.b_row_sqnorm(rs, Cc), what)
    assert np.array_equal(_n(xt), xs)
    t.unchanged()


# ----------------------------------------------------------------------------------------------------------------------
# Siamese attention
@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('b,T,D,Cc,ex_o,ex_do', B.ATT_CASES)
def test_siamese_attn_and_bwd(b, T, D, Cc, ex_o, ex_do, cls):
    """grl_siamese_attn into ldy = C + ex_o; grl_siamese_attn_bwd on the kernel's own out (ldo = ldy, lddo = C + ex_do), dx
    overwritten and accumulated; end to end on the float64 out (attn_forward_errors' e_out carried through)."""
    d = B.in_att(b, T, D, Cc, cls)
    ldo, lddo = Cc + ex_o, Cc + ex_do
    dob = np.full(b * lddo, SENT, np.float32)
    dob.reshape(b, lddo)[:, :Cc] = d['dout']
    t = _Inputs(qk=d['qk'], x=d['x'], dob=dob)
    p0 = np.full(b * ldo, SENT, np.float32)
    out = _out(b * ldo)
    _call('grl_siamese_attn', t['qk'], t['x'], out, b, T, D, Cc, ldo)
    fw = R.siamese_attn(d['qk'], d['x'], p0, b, T, D, Cc, ldo)
    what = (b, T, D, Cc, ex_o, ex_do, cls)
    ok = _got(out, b * ldo)
    B.check('siamese_attn', _window(ok, b, Cc, ldo, p0), fw['out'], B.b_siamese_attn(fw, T, D, Cc), what)
    obuf = p0.astype(np.float64)
    obuf.reshape(b, ldo)[:, :Cc] = fw['out']
    e_out = B.attn_forward_errors(fw, T, D, Cc)['e_out']
    for acc in (0, 1):
        dqk, dx = _out(b * T * 2 * D), _out(b * T * Cc, d['dx0'] if acc else None)
        _call('grl_siamese_attn_bwd', t['qk'], t['x'], out, ldo, t['dob'], lddo, dqk, dx, acc, b, T, D, Cc)
        gq, gx = _got(dqk, b * T * 2 * D).reshape(b, T, 2, D), _got(dx, b * T * Cc).reshape(b, T, Cc)
        bw = R.siamese_attn_bwd(d['qk'], d['x'], ok, ldo, dob, lddo, d['dx0'], acc, b, T, D, Cc)
        bb = B.b_siamese_attn_bwd(bw, T, D, Cc, acc)
        B.check('siamese_attn_bwd dx', gx, bw['dx'], bb['dx'], what + (acc,))
        B.check('siamese_attn_bwd dqk', gq, bw['dqk'], bb['dqk'], what + (acc,))
        e2e = R.siamese_attn_bwd(d['qk'], d['x'], obuf, ldo, dob, lddo, d['dx0'], acc, b, T, D, Cc)
        be = B.b_siamese_attn_bwd(e2e, T, D, Cc, acc, e_out)
        B.check('end to end siamese dx', gx, e2e['dx'], be['dx'], what + (acc,))
        B.check('end to end siamese dqk', gq, e2e['dqk'], be['dqk'], what + (acc,))
    assert np.array_equal(_got(out, b * ldo), ok)
    t.unchanged()


# ----------------------------------------------------------------------------------------------------------------------
# the pair head
@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('n,g,K', B.PAIR_BWD_CASES)
def test_pair_sqdiff_and_bwd(n, g, K, cls):
    """grl_pair_sqdiff and grl_pair_sqdiff_bwd (one thread per float4 of dp and dg, no stride loop).  The chain is its own end
    to end case: the backward reads p, g and the upstream gradient, nothing the forward wrote."""
    d, t = _pair_sqdiff(n, g, K, cls)
    dd = _d(d['dd'])
    dp, dg = _out(n * K), _out(g * K)
    _call('grl_pair_sqdiff_bwd', t['p'], t['g'], dd, dp, dg, n, g, K)
    bw = R.pair_sqdiff_bwd(d['p'], d['g'], d['dd'], n, g, K)
    bb = B.b_pair_sqdiff_bwd(bw, n, g)
    B.check('pair_sqdiff_bwd dp', _got(dp, n * K).reshape(n, K), bw['dp'], bb['dp'], (n, g, K, cls))
    B.check('pair_sqdiff_bwd dg', _got(dg, g * K).reshape(g, K), bw['dg'], bb['dg'], (n, g, K, cls))
    assert np.array_equal(_n(dd), d['dd'])
    t.unchanged()


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('n,g,K', B.PAIR_VERIFY_CASES)
def test_pair_verify(n, g, K, cls):
    """grl_pair_verify, ncls 1..4, scale / shift and bias each present or NULL."""
    d = B.in_pair(n, g, K, cls)
    t = _Inputs(p=d['p'], g=d['g'], scale=d['scale'], shift=d['shift'], w=d['w'], bias=d['bias'])
    for ncls in (1, 2, 3, 4):
        for affine in (True, False):
            for bias in (True, False):
                out = _out(n * g * ncls)
                _call('grl_pair_verify', t['p'], t['g'], t['scale'] if affine else None, t['shift'] if affine else None, t['w'],
                      t['bias'] if bias else None, out, n, g, K, ncls)
                ref = R.pair_verify(d['p'], d['g'], d['scale'] if affine else None, d['shift'] if affine else None,
                                    d['w'][:ncls], d['bias'][:ncls] if bias else None, n, g, K, ncls)
                B.check('pair_verify', _got(out, n * g * ncls).reshape(n, g, ncls), ref['out'], B.b_pair_verify(ref, K, affine, bias),
                        (n, g, K, cls, ncls, affine, bias))
    t.unchanged()


# ----------------------------------------------------------------------------------------------------------------------
def test_rejected_arguments_launch_nothing():
    """What the wrappers reject -- a width or stride that is no multiple of 4, T = 0 and 17, ncls = 0 and 5, scale without shift
    (and shift without scale), a NULL required pointer, zero rows -- raises GrlHipError and leaves every output untouched."""
    Err = _err()
    a = torch.ones(4096, device='cuda')
    outs = [_out(1024) for _ in range(4)]
    o0, o1, o2, o3 = outs
    f1 = _f(1.0)
    bad = [
        ('grl_gate_apply', (a, 1, a, o0, o1, o2, 4, 6)), ('grl_gate_apply', (a, 1, a, o0, o1, o2, 0, 8)),
        ('grl_gate_apply', (None, 1, a, o0, o1, o2, 4, 8)), ('grl_gate_apply', (a, 0, a, o0, o1, o2, 4, 8)),
        ('grl_gate_apply', (a, 1, a, o0, None, o2, 4, 8)),
        ('grl_gate_bwd', (a, a, a, a, o0, 0, o1, 1, 4, 6)), ('grl_gate_bwd', (a, a, a, a, o0, 0, o1, 1, 0, 8)),
        ('grl_gate_bwd', (a, a, a, None, o0, 0, o1, 1, 4, 8)), ('grl_gate_bwd', (a, a, a, a, o0, 0, None, 1, 4, 8)),
        ('grl_gce_gate', (a, a, a, a, a, o0, o1, o2, 4, 6, 8)), ('grl_gce_gate', (a, a, a, a, a, o0, o1, o2, 4, 8, 6)),
        ('grl_gce_gate', (a, a, a, a, a, o0, o1, o2, 0, 8, 8)), ('grl_gce_gate', (a, None, a, a, a, o0, o1, o2, 4, 8, 8)),
        ('grl_group_mean', (a, o0, 2, 4, 6, 8, f1, 0)), ('grl_group_mean', (a, o0, 2, 4, 8, 10, f1, 0)),
        ('grl_group_mean', (a, o0, 2, 0, 8, 8, f1, 0)), ('grl_group_mean', (a, o0, 0, 4, 8, 8, f1, 0)),
        ('grl_group_mean', (None, o0, 2, 4, 8, 8, f1, 0)),
        ('grl_sqdiff_mean', (a, a, o0, 2, 4, 6, 32)), ('grl_sqdiff_mean', (a, a, o0, 2, 4, 8, 34)),
        ('grl_sqdiff_mean', (a, a, o0, 2, 0, 8, 32)), ('grl_sqdiff_mean', (a, None, o0, 2, 4, 8, 32)),
        ('grl_sqdiff_bwd', (a, a, a, o0, o1, 2, 4, 6, 32, 0)), ('grl_sqdiff_bwd', (a, a, a, o0, o1, 2, 4, 8, 34, 0)),
        ('grl_sqdiff_bwd', (a, a, a, o0, o1, 2, 0, 8, 32, 0)), ('grl_sqdiff_bwd', (a, a, None, o0, o1, 2, 4, 8, 32, 0)),
        ('grl_temporal_mean', (a, o0, 2, 2, 6)), ('grl_temporal_mean', (a, o0, 2, 0, 8)), ('grl_temporal_mean', (a, o0, 0, 2, 8)),
        ('grl_temporal_mean', (None, o0, 2, 2, 8)),
        ('grl_add_strided', (a, a, o0, 2, 6, 8)), ('grl_add_strided', (a, a, o0, 2, 8, 10)), ('grl_add_strided', (a, a, o0, 0, 8, 8)),
        ('grl_add_strided', (a, None, o0, 2, 8, 8)),
        ('grl_mean_T', (a, o0, 2, 2, 6, 8)), ('grl_mean_T', (a, o0, 2, 2, 8, 10)), ('grl_mean_T', (a, o0, 2, 0, 8, 8)),
        ('grl_mean_T', (a, o0, 0, 2, 8, 8)), ('grl_mean_T', (None, o0, 2, 2, 8, 8)),
        ('grl_add_rowbcast', (o0, a, 4, 6, 2, f1, 0)), ('grl_add_rowbcast', (o0, a, 0, 8, 2, f1, 0)),
        ('grl_add_rowbcast', (o0, a, 4, 8, 0, f1, 0)), ('grl_add_rowbcast', (o0, None, 4, 8, 2, f1, 0)),
        ('grl_channel_atte', (a, a, a, a, 8, o0, o1, 8, 0, 2, 6, 3, o2)), ('grl_channel_atte', (a, a, a, a, 10, o0, o1, 8, 0, 2, 8, 3, o2)),
        ('grl_channel_atte', (a, a, a, a, 8, o0, o1, 10, 0, 2, 8, 3, o2)), ('grl_channel_atte', (a, a, a, a, 8, o0, o1, 8, 0, 0, 8, 3, o2)),
        ('grl_channel_atte', (a, a, a, a, 8, o0, o1, 8, 0, 2, 8, 0, o2)), ('grl_channel_atte', (a, a, a, a, 8, o0, o1, 8, 0, 2, 8, 3, None)),
        ('grl_channel_atte', (a, a, None, a, 8, o0, o1, 8, 0, 2, 8, 3, o2)),
        ('grl_catte_bwd', (a, 8, a, 8, a, o0, o1, 8, 0, 2, 6)), ('grl_catte_bwd', (a, 10, a, 8, a, o0, o1, 8, 0, 2, 8)),
        ('grl_catte_bwd', (a, 8, a, 10, a, o0, o1, 8, 0, 2, 8)), ('grl_catte_bwd', (a, 8, a, 8, a, o0, o1, 10, 0, 2, 8)),
        ('grl_catte_bwd', (a, 8, a, 8, a, o0, o1, 8, 0, 0, 8)), ('grl_catte_bwd', (a, 8, a, 8, None, o0, o1, 8, 0, 2, 8)),
        ('grl_affine_l2norm', (a, a, a, o0, 2, 6, 8)), ('grl_affine_l2norm', (a, a, a, o0, 2, 8, 10)),
        ('grl_affine_l2norm', (a, a, a, o0, 0, 8, 8)), ('grl_affine_l2norm', (a, a, None, o0, 2, 8, 8)),
        ('grl_affine_l2norm', (a, None, a, o0, 2, 8, 8)), ('grl_affine_l2norm', (None, a, a, o0, 2, 8, 8)),
        ('grl_l2norm_bwd', (a, 8, a, 8, a, o0, 2, 6)), ('grl_l2norm_bwd', (a, 10, a, 8, a, o0, 2, 8)),
        ('grl_l2norm_bwd', (a, 8, a, 10, a, o0, 2, 8)), ('grl_l2norm_bwd', (a, 8, a, 8, a, o0, 0, 8)),
        ('grl_l2norm_bwd', (a, 8, None, 8, a, o0, 2, 8)),
        ('grl_row_sqnorm', (a, o0, 2, 6, 8)), ('grl_row_sqnorm', (a, o0, 2, 8, 10)), ('grl_row_sqnorm', (a, o0, 0, 8, 8)),
        ('grl_row_sqnorm', (None, o0, 2, 8, 8)),
        ('grl_siamese_attn', (a, a, o0, 2, 0, 8, 8, 8)), ('grl_siamese_attn', (a, a, o0, 2, 17, 8, 8, 8)),
        ('grl_siamese_attn', (a, a, o0, 2, 2, 6, 8, 8)), ('grl_siamese_attn', (a, a, o0, 2, 2, 8, 6, 8)),
        ('grl_siamese_attn', (a, a, o0, 2, 2, 8, 8, 10)), ('grl_siamese_attn', (a, a, o0, 0, 2, 8, 8, 8)),
        ('grl_siamese_attn', (None, a, o0, 2, 2, 8, 8, 8)),
        ('grl_siamese_attn_bwd', (a, a, a, 8, a, 8, o0, o1, 0, 2, 0, 8, 8)), ('grl_siamese_attn_bwd', (a, a, a, 8, a, 8, o0, o1, 0, 2, 17, 8, 8)),
        ('grl_siamese_attn_bwd', (a, a, a, 8, a, 8, o0, o1, 0, 2, 2, 6, 8)), ('grl_siamese_attn_bwd', (a, a, a, 8, a, 8, o0, o1, 0, 2, 2, 8, 6)),
        ('grl_siamese_attn_bwd', (a, a, a, 10, a, 8, o0, o1, 0, 2, 2, 8, 8)), ('grl_siamese_attn_bwd', (a, a, a, 8, a, 10, o0, o1, 0, 2, 2, 8, 8)),
        ('grl_siamese_attn_bwd', (a, a, a, 8, a, 8, o0, o1, 0, 0, 2, 8, 8)), ('grl_siamese_attn_bwd', (a, a, None, 8, a, 8, o0, o1, 0, 2, 2, 8, 8)),
        ('grl_siamese_attn_bwd', (a, a, a, 8, a, 8, None, o1, 0, 2, 2, 8, 8)),
        ('grl_pair_sqdiff', (a, a, o0, 2, 3, 6)), ('grl_pair_sqdiff', (a, a, o0, 0, 3, 8)), ('grl_pair_sqdiff', (a, a, o0, 2, 0, 8)),
        ('grl_pair_sqdiff', (a, None, o0, 2, 3, 8)),
        ('grl_pair_sqdiff_bwd', (a, a, a, o0, o1, 2, 3, 6)), ('grl_pair_sqdiff_bwd', (a, a, a, o0, o1, 0, 3, 8)),
        ('grl_pair_sqdiff_bwd', (a, a, a, o0, o1, 2, 0, 8)), ('grl_pair_sqdiff_bwd', (a, a, None, o0, o1, 2, 3, 8)),
        ('grl_pair_sqdiff_bwd', (a, a, a, o0, None, 2, 3, 8)),
        ('grl_pair_verify', (a, a, a, a, a, a, o0, 2, 3, 6, 2)), ('grl_pair_verify', (a, a, a, a, a, a, o0, 2, 3, 8, 0)),
        ('grl_pair_verify', (a, a, a, a, a, a, o0, 2, 3, 8, 5)), ('grl_pair_verify', (a, a, a, None, a, a, o0, 2, 3, 8, 2)),
        ('grl_pair_verify', (a, a, None, a, a, a, o0, 2, 3, 8, 2)), ('grl_pair_verify', (a, a, a, a, None, a, o0, 2, 3, 8, 2)),
        ('grl_pair_verify', (a, a, a, a, a, a, o0, 0, 3, 8, 2)), ('grl_pair_verify', (a, a, a, a, a, a, o0, 2, 0, 8, 2)),
    ]
    for name, args in bad:
        with pytest.raises(Err):
            _call(name, *args)
    torch.cuda.synchronize()
    for o in outs:
        assert (_n(o) == SENT).all(), 'a rejected call wrote to an output'
    assert (_n(a) == 1.0).all()
    # ... and the same entry points accept the neighbouring good arguments
    _call('grl_pair_verify', a, a, None, None, a, None, o0, 2, 3, 8, 4)
    _call('grl_siamese_attn', a, a, o1, 2, 16, 8, 8, 8)
    torch.cuda.synchronize()
    assert (_n(o0)[:24] != SENT).all() and (_n(o0)[24:] == SENT).all()
    assert (_n(o1)[:16] != SENT).all() and (_n(o1)[16:] == SENT).all()
