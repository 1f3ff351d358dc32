"""The float64 reference of the gate, TRL and Siamese head kernels (tests/head_ref.py) is right, and the bounds of
tests/head_bounds.py are satisfiable -- both shown without a GPU:

* every function of head_ref against torch float64 on the CPU -- forwards against the plain torch expression, backwards
  against torch.autograd.grad of it -- over the sweep of the GPU file (the 8192 * 256 cases by their 2052-float stand-ins);
* fp32 numpy restatements of the reductions in the kernels' own order against head_ref inside the very bounds the GPU tests
  hold the kernels to, on both input classes;
* the sweep takes both sides of every branch it claims to take.

TOL = 1e-12 relative per element is safe: both sides are float64 (2^-53 ~ 1.1e-16), the longest sums have a few thousand
terms and are added pairwise or blocked by numpy and torch alike, so the two differ by some tens of roundings of the
element's absolute terms -- four decades below 1e-12 -- while a wrong formula misses by the size of the element.  "Relative"
is relative to the sum of the absolute values of the terms the element is made of (for a product or a sum without
cancellation that is |element| itself): a difference of two nearly equal operands cannot agree better than that on
either side."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import head_bounds as B
import head_ref as R

TOL = 1e-12
SENT = 12345.0


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    yield
    B.dump_ratios('fp32 numpy restatement (CPU)')


def _t(a, grad=False):
    return torch.from_numpy(np.array(a, dtype=np.float64)).requires_grad_(grad)


def _close(got, ref, what, scale=None):
    ref = ref.detach().numpy() if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64).reshape(ref.shape)
    s = np.abs(ref) if scale is None else np.maximum(np.abs(ref), np.broadcast_to(scale, ref.shape))
    bad = np.abs(got - ref) > TOL * s + 1e-300
    assert not bad.any(), (what, float((np.abs(got - ref) / (s + 1e-300)).max()), int(bad.sum()))


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('M,C,ldy', B.GATE_CASES)
def test_gate_apply_and_bwd(M, C, ldy, cls):
    d = B.in_gate(M, C, ldy, cls)
    fw = R.gate_apply(d['y'], ldy, d['x'], M, C)
    z, x = _t(d['y'][np.arange(M) * ldy], True), _t(d['x'], True)
    g = torch.sigmoid(z)[:, None]
    xc, xu = x * g, x * (1 - g)
    _close(fw['cmap'], g[:, 0], 'cmap'); _close(fw['xc'], xc, 'xc'); _close(fw['xu'], xu, 'xu')
    dx_t, dz_t = torch.autograd.grad([xc, xu], [x, z], [_t(d['dxc']), _t(d['dxu'])])
    for acc in (0, 1):
        bw = R.gate_bwd(d['dxc'], d['dxu'], d['x'], fw['cmap'], d['dx0'], acc, d['dy0'], ldy, M, C)
        _close(bw['dx'], dx_t + (_t(d['dx0']) if acc else 0.0), 'dx', bw['abs_dx'])
        _close(bw['dy_col'], dz_t, 'dy', bw['abs_s'] * bw['gg'])
        keep = np.ones(M * ldy, bool); keep[np.arange(M) * ldy] = False
        assert np.array_equal(bw['dy'][keep], R.f64(d['dy0'])[keep])


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('M,Ch,C', B.GCE_CASES)
def test_gce_gate(M, Ch, C, cls):
    d = B.in_gce(M, Ch, C, cls)
    ref = R.gce_gate(d['h'], d['w3'], d['bsc'], d['bsh'], d['x'], M, Ch, C)
    z = (_t(d['h']) @ _t(d['w3'])) * float(d['bsc'][0]) + float(d['bsh'][0])
    g = torch.sigmoid(z)[:, None]
    # the logit's own float64 noise (relative to |s scale| + |shift|) reaches the map and both products: the 1 + |logit| terms
    _close(ref['logit'], z, 'logit', ref['abs_logit'])
    _close(ref['cmap'], g[:, 0], 'cmap', ref['cmap'] * (1 + ref['abs_logit']))
    _close(ref['xc'], _t(d['x']) * g, 'xc', np.abs(ref['xc']) * (1 + ref['abs_logit'])[:, None])
    _close(ref['xu'], _t(d['x']) * (1 - g), 'xu', np.abs(d['x']) * (1 + ref['abs_logit'])[:, None])
    if cls == 'b':                # the inputs do what they are for: the logits land next to the five values, saturation included
        assert np.abs(ref['logit'][:, None] - B.GATE_LOGITS[None, :]).min(1).max() < 1e-2


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('groups,rows,C,ld_extra,f2_mult', B.RED_CASES + (B.BIG_CPU['sqdiff_bwd'] + (0, 1),))
def test_group_mean_sqdiff_mean_and_bwd(groups, rows, C, ld_extra, f2_mult, cls):
    d = B.in_red(groups, rows, C, f2_mult, cls)
    ldy = C + ld_extra
    y0 = np.full(groups * ldy + 4, SENT)
    x = _t(d['x'])
    for scale, acc in ((1.0, 0), (0.5, 1), (2.0, 1)):
        ref = R.group_mean(d['x'], y0, groups, rows, C, ldy, scale, acc)
        _close(ref['val'], x.mean(1) * scale + (SENT if acc else 0.0), 'group_mean', ref['abs_mean'] + (SENT if acc else 0.0))
        keep = np.ones(y0.size, bool)
        for g in range(groups):
            keep[g * ldy:g * ldy + C] = False
        assert (ref['y'][keep] == SENT).all()
    f2v = d['f2buf'][B.F2_OFFSET:]
    f1 = _t(d['f1'], True)
    f2 = _t(np.stack([f2v[g * d['stride']:g * d['stride'] + rows * C].reshape(rows, C) for g in range(groups)]), True)
    dm = ((f1 - f2) ** 2).mean(1)
    _close(R.sqdiff_mean(d['f1'], f2v, groups, rows, C, d['stride'])['d'], dm, 'sqdiff_mean')
    g1, g2 = torch.autograd.grad(dm, [f1, f2], _t(d['dd']))
    for acc in (0, 1):
        bw = R.sqdiff_bwd(d['f1'], f2v, d['dd'], d['df2buf'][B.F2_OFFSET:], groups, rows, C, d['stride'], acc)
        _close(bw['df1'], g1, 'df1')
        want = g2.numpy().copy()
        buf0 = R.f64(d['df2buf'][B.F2_OFFSET:])
        keep = np.ones(buf0.size, bool)
        for g in range(groups):
            o = g * d['stride']
            keep[o:o + rows * C] = False
            if acc:
                want[g] += buf0[o:o + rows * C].reshape(rows, C)
        _close(bw['df2_val'], want, 'df2', np.abs(g2.numpy()) + (1.0 if acc else 0.0) * np.abs(want))
        assert np.array_equal(bw['df2'][keep], buf0[keep])


def _ew_list():
    return [(b, rows, C, T) for b, rows, C in B.EW_CASES for T in B.EW_T]


@pytest.mark.parametrize('b,rows,C,T', _ew_list() + [(1, 1, 2052, 2)])          # (+ the stand-in of the 8192 * 256 cases)
def test_temporal_mean_add_strided_mean_T(b, rows, C, T):
    r = B.rng_for('ew', b, rows, C, T)
    inner = rows * C
    x = B.normal(r, (b, T, inner), 'a')
    _close(R.temporal_mean(x, b, T, inner)['y'], _t(x).mean(1), 'temporal_mean', np.abs(x).mean(1))
    ld = C + 8
    y0 = np.full(b * rows * ld, SENT)
    xm = B.normal(r, (b * rows, T, C), 'a')
    ref = R.mean_T(xm, y0, b * rows, T, C, ld)
    _close(ref['val'], _t(xm).mean(1), 'mean_T', ref['abs_val'])
    assert (ref['y'].reshape(b * rows, ld)[:, C:] == SENT).all()
    a = B.normal(r, (b, inner), 'a')
    stride = T * inner + 4
    bs = B.normal(r, b * stride, 'a')
    want = _t(a) + _t(np.stack([bs[i * stride:i * stride + inner] for i in range(b)]))
    _close(R.add_strided(a, bs, b, inner, stride)['y'], want, 'add_strided', np.abs(a) + np.abs(want.numpy() - a))


@pytest.mark.parametrize('M,C,rpg', [(b * rows, C, rpg) for b, rows, C in B.EW_CASES for rpg in B.EW_RPG]
                         + [B.ROWBCAST_SHORT, B.BIG_CPU['add_rowbcast']])
def test_add_rowbcast_is_the_backward_of_a_scaled_group_sum(M, C, rpg):
    r = B.rng_for('rowbcast', M, C, rpg)
    groups = (M + rpg - 1) // rpg
    v, dst0 = B.normal(r, (groups, C), 'a'), B.normal(r, (M, C), 'a')
    xs = _t(dst0, True)
    for scale, acc in ((1.0, 0), (1.0 / rpg, 1)):
        sc = float(np.float32(scale))
        y = torch.zeros(groups, C, dtype=torch.float64).index_add(0, torch.arange(M) // rpg, xs) * sc
        (gx,) = torch.autograd.grad(y, xs, _t(v))
        _close(R.add_rowbcast(dst0, v, M, C, rpg, sc, acc)['dst'], gx + (_t(dst0) if acc else 0.0), 'add_rowbcast',
               np.abs(gx.numpy()) + np.abs(dst0))


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('b,Hd,C', B.CATTE_CASES + (B.BIG_CPU['catte_bwd'][:1] + (3,) + B.BIG_CPU['catte_bwd'][1:],))
def test_channel_atte_and_bwd(b, Hd, C, cls):
    d = B.in_catte(b, Hd, C, cls)
    T, st = B.CATTE_T, B.CATTE_T * C
    rows = np.arange(b) * st + C
    gap = _t(np.stack([d['gapbuf'][o:o + C] for o in rows]), True)
    hid = torch.relu(_t(d['d']) @ _t(d['w1']).t())
    z = (hid @ _t(d['w2t'])).detach().requires_grad_(True)
    a = torch.sigmoid(z)
    f = gap * a + gap
    f0 = np.stack([d['fstepbuf'][o:o + C] for o in rows])
    keep = np.ones(b * T * C - C, bool)
    for i in range(b):
        keep[i * st:i * st + C] = False
    for acc in (0, 1):
        ref = R.channel_atte(d['d'], d['w1'], d['w2t'], d['gapbuf'][C:], st, True, d['fstepbuf'][C:], st, acc, b, C, Hd)
        zs = np.abs(ref['hid']) @ np.abs(ref['w2t'])
        _close(ref['hid'], hid, 'hid', ref['abs_hid'])
        _close(ref['logit'], z, 'logit', zs)
        _close(ref['catte'], a, 'catte', ref['a'] * (1 + zs))
        _close(ref['fstep_val'], f + (_t(f0) if acc else 0.0), 'fstep', np.abs(ref['term']) * (1 + zs) + np.abs(f0))
        assert np.array_equal(ref['fstep'][keep], R.f64(d['fstepbuf'][C:])[keep])
    assert R.channel_atte(d['d'], d['w1'], d['w2t'], d['gapbuf'][C:], st, False, d['fstepbuf'][C:], st, 0, b, C, Hd)['catte'] is None
    dfs = np.stack([d['dfsbuf'][o:o + C] for o in rows])
    dz, dg = torch.autograd.grad(f, [z, gap], _t(dfs))
    dg0 = np.stack([d['dgapbuf'][o:o + C] for o in rows])
    for acc in (0, 1):
        bw = R.catte_bwd(d['dfsbuf'][C:], st, d['gapbuf'][C:], st, ref['a'], d['dgapbuf'][C:], st, acc, b, C)
        _close(bw['ds'], dz, 'ds', np.abs(dz.numpy()) * (1 + zs))
        _close(bw['dgap_val'], dg + (_t(dg0) if acc else 0.0), 'dgap', np.abs(bw['term']) * (1 + zs) + np.abs(dg0))
        assert np.array_equal(bw['dgap'][keep], R.f64(d['dgapbuf'][C:])[keep])


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('rows,C,ld', B.BLOCK_CASES)
def test_l2norm_tail(rows, C, ld, cls):
    d = B.in_l2(rows, C, cls)
    y0 = np.full(rows * ld, SENT)
    for affine in (True, False):
        sc, sh = (d['scale'], d['shift']) if affine else (None, None)
        ref = R.affine_l2norm(d['x'], sc, sh, y0, rows, C, ld)
        v = (_t(d['x']) * _t(sc) + _t(sh)) if affine else _t(d['x'])
        v = v.detach().requires_grad_(True)
        y = TF.normalize(v, p=2, dim=1)
        # v = x s + t cancels where the terms do: its float64 noise, relative to |v|'s scale, reaches every y of the row
        cond = (ref['abs_v'] / np.sqrt(ref['ss'])[:, None]).max(1)[:, None] + 1
        _close(ref['val'], y, 'y', np.abs(ref['val']) * cond + cond / np.sqrt(ref['ss'])[:, None] * ref['abs_v'])
        assert (ref['y'].reshape(rows, ld)[:, C:] == SENT).all()
        (dv,) = torch.autograd.grad(y, v, _t(d['dy']))
        ybuf = np.full(rows * ld, SENT); ybuf.reshape(rows, ld)[:, :C] = ref['val']
        dyb = np.full(rows * (2 * ld - C), SENT); dyb.reshape(rows, 2 * ld - C)[:, :C] = d['dy']
        bw = R.l2norm_bwd(dyb, 2 * ld - C, ybuf, ld, ref['v'], rows, C)
        s = (np.abs(bw['dy']) + np.abs(bw['y']) * bw['abs_dot'][:, None]) / np.sqrt(bw['ss'])[:, None]
        _close(bw['dv'], dv, 'dv', s * cond)
    xs = B.normal(B.rng_for('sq', rows, C), (rows, ld), cls)
    _close(R.row_sqnorm(xs, rows, C, ld)['out'], (_t(xs)[:, :C] ** 2).sum(1), 'row_sqnorm')


def _torch_attn(qk, x, b, T, D):
    q, k = qk.view(b, T, 2, D)[:, :, 0], qk.view(b, T, 2, D)[:, :, 1]
    q = q / q.norm(2, 2, keepdim=True)
    k = k / k.norm(2, 2, keepdim=True)
    w = torch.softmax(torch.matmul(q, k.transpose(-1, -2)), dim=-1)
    pooled = torch.matmul(w, x).sum(1)
    return pooled / pooled.norm(2, 1, keepdim=True)


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('b,T,D,C,ex_o,ex_do', B.ATT_CASES)
def test_siamese_attn_and_bwd(b, T, D, C, ex_o, ex_do, cls):
    d = B.in_att(b, T, D, C, cls)
    ldo, lddo = C + ex_o, C + ex_do
    qk, x = _t(d['qk'], True), _t(d['x'], True)
    out = _torch_attn(qk, x, b, T, D)
    fw = R.siamese_attn(d['qk'], d['x'], np.full(b * ldo, SENT), b, T, D, C, ldo)
    # the scores carry 2^-53 sum|qh kh| each; exp turns that into a relative error of P, w and raw: a few thousand terms
    cond = 1 + (np.abs(fw['x']).sum(1) / fw['nraw'][:, None]).max(1)[:, None]
    _close(fw['out'], out, 'out', np.abs(fw['out']) * cond)
    assert (fw['pooled'].reshape(b, ldo)[:, C:] == SENT).all()
    gq, gx = torch.autograd.grad(out, [qk, x], _t(d['dout']))
    obuf = np.full(b * ldo, SENT); obuf.reshape(b, ldo)[:, :C] = fw['out']
    dob = np.full(b * lddo, SENT); dob.reshape(b, lddo)[:, :C] = d['dout']
    for acc in (0, 1):
        bw = R.siamese_attn_bwd(d['qk'], d['x'], obuf, ldo, dob, lddo, d['dx0'], acc, b, T, D, C)
        # absolute terms through the chain (draw -> dw -> dS -> dqh -> dQ), as in the module docstring
        s_draw = (np.abs(bw['dout']) + np.abs(bw['out']) * np.abs(bw['out'] * bw['dout']).sum(1)[:, None]) / fw['nraw'][:, None]
        s_dx = fw['w'][:, :, None] * s_draw[:, None, :]
        _close(bw['dx'], gx + (_t(d['dx0']) if acc else 0.0), 'dx', s_dx * cond[:, :, None] + np.abs(d['dx0']))
        s_dw = np.einsum('bc,bjc->bj', s_draw, np.abs(fw['x'])) * cond
        s_dS = fw['P'] * (s_dw[:, None, :] + np.einsum('bik,bk->bi', fw['P'], s_dw)[:, :, None])
        s_q = np.einsum('bij,bjd->bid', s_dS, np.abs(fw['kh']))
        s_k = np.einsum('bij,bid->bjd', s_dS, np.abs(fw['qh']))
        s_q = (s_q + np.abs(fw['qh']) * (np.abs(fw['qh']) * s_q).sum(2, keepdims=True)) / fw['nq'][..., None]
        s_k = (s_k + np.abs(fw['kh']) * (np.abs(fw['kh']) * s_k).sum(2, keepdims=True)) / fw['nk'][..., None]
        _close(bw['dqk'], gq.view(b, T, 2, D), 'dqk', np.stack([s_q, s_k], 2))


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('n,g,K', B.PAIR_BWD_CASES + B.PAIR_VERIFY_CASES + (B.BIG_CPU['pair_sqdiff'],))
def test_pair_head(n, g, K, cls):
    d = B.in_pair(n, g, K, cls)
    p, q = _t(d['p'], True), _t(d['g'], True)
    diff = ((p[:, None, :] - q[None, :, :]) ** 2).reshape(n * g, K)
    _close(R.pair_sqdiff(d['p'], d['g'], n, g, K)['diff'], diff, 'diff')
    dp, dg = torch.autograd.grad(diff, [p, q], _t(d['dd']))
    bw = R.pair_sqdiff_bwd(d['p'], d['g'], d['dd'], n, g, K)
    _close(bw['dp'], dp, 'dp', bw['abs_dp']); _close(bw['dg'], dg, 'dg', bw['abs_dg'])
    for ncls in (1, 2, 3, 4):
        for affine in (True, False):
            for bias in (True, False):
                e = diff.detach() * _t(d['scale']) + _t(d['shift']) if affine else diff.detach()
                want = e @ _t(d['w'][:ncls]).t() + (_t(d['bias'][:ncls]) if bias else 0.0)
                ref = R.pair_verify(d['p'], d['g'], d['scale'] if affine else None, d['shift'] if affine else None,
                                    d['w'][:ncls], d['bias'][:ncls] if bias else None, n, g, K, ncls)
                _close(ref['out'], want.view(n, g, ncls), 'pair_verify', ref['abs_out'] + (np.abs(d['bias'][:ncls]) if bias else 0.0))


# ----------------------------------------------------------------------------------------------------------------------
def test_sweep_takes_both_sides_of_every_branch():
    # rows past M in the last workgroup of the one-wave-per-row kernels (and a full last workgroup)
    for rows in (B.WAVE_ROWS, [n * g for n, g in B.PAIR_COUNTS], [b * Hd for b in B.CATTE_B for Hd in B.CATTE_HD]):
        idle = [B.last_workgroup_has_idle_waves(r) for r in rows]
        assert any(idle) and not all(idle), rows
    assert set(M for M, _, _ in B.GATE_CASES) == set(B.WAVE_ROWS) and set(C for _, C, _ in B.GATE_CASES) == set(B.WAVE_WIDTH)
    assert set(M for M, _, _ in B.GCE_CASES) == set(B.WAVE_ROWS) and set(c for _, c, _ in B.GCE_CASES) == set(B.WAVE_WIDTH)
    assert set(c for _, _, c in B.GCE_CASES) == set(B.WAVE_WIDTH)
    for M, C, ldy in B.GATE_CASES:
        assert ldy in B.gate_ldys(C)
    assert set(B.gate_ldys(C).index(l) for _, C, l in B.GATE_CASES) == {0, 1, 2}
    # a lane with no trip, with exactly one, and one with two, of the stride-256 and stride-1024 loops
    for widths, stride in ((B.WAVE_WIDTH, 256), (B.CATTE_C, 256), (B.BLOCK_WIDTH, 1024), (B.ATT_C, 1024), (B.ATT_D, 256)):
        lo = [B.lane_trips(w, stride)[0] for w in widths]
        hi = [B.lane_trips(w, stride)[1] for w in widths]
        assert 0 in lo and max(hi) >= 2 and 1 in hi, (widths, stride)
    assert B.lane_trips(256, 256) == (1, 1) and B.lane_trips(260, 256) == (1, 2) and B.lane_trips(252, 256) == (0, 1)
    assert B.lane_trips(1020, 1024) == (0, 1) and B.lane_trips(1028, 1024) == (1, 2) and B.lane_trips(2052, 1024) == (2, 3)
    # fewer rows than waves, as many, more; a wave with two rows
    per = [B.red16_rows_per_wave(r) for r in B.RED_ROWS]
    assert (0, 1) in per and (1, 1) in per and (1, 2) in per and (2, 3) in per
    assert set(r for _, r, _, _, _ in B.RED_CASES) == set(B.RED_ROWS) and set(c for _, _, c, _, _ in B.RED_CASES) == set(B.RED_WIDTH)
    assert set(g for g, _, _, _, _ in B.RED_CASES) == set(B.RED_GROUPS)
    assert set(e for _, _, _, e, _ in B.RED_CASES) == {0, 8} and set(m for _, _, _, _, m in B.RED_CASES) == {1, 2}
    assert any(c > 256 for _, _, c, _, _ in B.RED_CASES)           # a second 256-column slab, and lanes past C in it
    # block-per-row kernels: both leading dimensions at every shape
    assert set(B.BLOCK_CASES) == set((r, C, ld) for r in B.BLOCK_ROWS for C in B.BLOCK_WIDTH for ld in (C, C + 8))
    # T with idle waves (2 T < 4) and with several rows per wave; T * T scores below and above four waves
    per = {T: B.att_rows_per_wave(T) for T in B.ATT_T}
    assert per[1] == (0, 1) and per[2] == (1, 1) and per[16] == (8, 8) and per[5][1] == 3
    assert set(c[1] for c in B.ATT_CASES) == set(B.ATT_T)
    for T in (1, 5):
        assert set((c[2], c[3]) for c in B.ATT_CASES if c[1] == T) >= set((D, C) for D in B.ATT_D for C in B.ATT_C)
    assert (3, 16, max(B.ATT_D), max(B.ATT_C), 8, 0) in B.ATT_CASES
    assert set(c[0] for c in B.ATT_CASES) == set(B.ATT_B) and set(c[4] for c in B.ATT_CASES) == {0, 8} == set(c[5] for c in B.ATT_CASES)
    # the grid-stride tail: exactly the big cases pass 8192 * 256 float4 items, by little; their stand-ins hold 2 * 256 * 4 + 4 floats
    for name, case in B.BIG.items():
        assert B.GRID_CAP < B.big_items(name, case) <= B.GRID_CAP + 2048, name
        assert B.big_items(name, B.BIG_CPU[name]) == 513, name
    assert B.ROWBCAST_SHORT[0] % B.ROWBCAST_SHORT[2] != 0
    assert set(B.CATTE_CASES) == set((b, h, c) for b in B.CATTE_B for h in B.CATTE_HD for c in B.CATTE_C)


# ----------------------------------------------------------------------------------------------------------------------
# the fp32 restatements stay inside the bounds the GPU tests use
@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('M,Ch,C', B.GCE_CASES)
def test_fp32_gate_dots_inside_the_bounds(M, Ch, C, cls):
    d = B.in_gce(M, Ch, C, cls)
    ref = R.gce_gate(d['h'], d['w3'], d['bsc'], d['bsh'], d['x'], M, Ch, C)
    got = B.gce_gate_f32(d['h'], d['w3'], d['bsc'][0], d['bsh'][0], d['x'])
    bd = B.b_gce_gate(ref, d['x'], d['bsc'][0], Ch)
    for k in ('cmap', 'xc', 'xu'):
        B.check('gce_gate ' + k, got[k], ref[k], bd[k], (M, Ch, C, cls))
    g = B.in_gate(M, Ch, 1, cls)
    cmap = B.sigmoid_f32(g['y'])
    bw = R.gate_bwd(g['dxc'], g['dxu'], g['x'], cmap, g['dx0'], 0, g['dy0'], 1, M, Ch)
    B.check('gate_bwd dy', B.gate_bwd_dy_f32(g['dxc'], g['dxu'], g['x'], cmap), bw['dy_col'], B.b_gate_bwd(bw, Ch, 0)['dy'],
            (M, Ch, cls))


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('groups,rows,C,ld_extra,f2_mult', B.RED_CASES)
def test_fp32_red16_sums_inside_the_bounds(groups, rows, C, ld_extra, f2_mult, cls):
    d = B.in_red(groups, rows, C, f2_mult, cls)
    y0 = B.normal(B.rng_for('y0', groups, C), (groups, C), 'a')
    for scale, acc in ((1.0, 0), (0.5, 1)):
        ref = R.group_mean(d['x'], y0, groups, rows, C, C, scale, acc)
        B.check('group_mean', B.group_mean_f32(d['x'], rows, scale, y0 if acc else None), ref['val'],
                B.b_group_mean(ref, rows, acc), (groups, rows, C, cls, acc))
    f2v = d['f2buf'][B.F2_OFFSET:]
    f2 = np.stack([f2v[g * d['stride']:g * d['stride'] + rows * C].reshape(rows, C) for g in range(groups)])
    ref = R.sqdiff_mean(d['f1'], f2v, groups, rows, C, d['stride'])
    B.check('sqdiff_mean', B.sqdiff_mean_f32(d['f1'], f2, rows), ref['d'], B.b_sqdiff_mean(ref, rows), (groups, rows, C, cls))


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('rows,C,ld', [c for c in B.BLOCK_CASES if c[2] == c[1]])
def test_fp32_l2norm_sums_inside_the_bounds(rows, C, ld, cls):
    d = B.in_l2(rows, C, cls)
    for affine in (True, False):
        sc, sh = (d['scale'], d['shift']) if affine else (None, None)
        ref = R.affine_l2norm(d['x'], sc, sh, np.zeros(rows * C), rows, C, C)
        y = B.affine_l2norm_f32(d['x'], sc, sh)
        B.check('affine_l2norm', y, ref['val'], B.affine_l2norm_bounds(ref, C, affine)['y'], (rows, C, cls, affine))
        v32 = B.f32(d['x']) if not affine else B.f32(d['x']) * d['scale'] + d['shift']
        bw = R.l2norm_bwd(d['dy'], C, y, C, v32, rows, C)
        B.check('l2norm_bwd', B.l2norm_bwd_f32(d['dy'], y, v32), bw['dv'], B.b_l2norm_bwd(bw, C), (rows, C, cls, affine))


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('b,T,D,C,ex_o,ex_do', B.ATT_CASES)
def test_fp32_attention_scores_and_pooling_inside_the_bounds(b, T, D, C, ex_o, ex_do, cls):
    d = B.in_att(b, T, D, C, cls)
    fw = R.siamese_attn(d['qk'], d['x'], np.zeros(b * C), b, T, D, C, C)
    B.check('siamese_attn', B.siamese_attn_f32(d['qk'], d['x'], b, T, D, C), fw['out'], B.b_siamese_attn(fw, T, D, C),
            (b, T, D, C, cls))
