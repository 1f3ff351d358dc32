"""The train-mode BatchNorm kernels (train.hip, train_bnfuse.hip, train_bf16.hip) against the float64 restatement of
tests/bn_ref.py, stage by stage through the C ABI, on a real MI355X.

Each stage is handed the fp32 vectors (mean, invstd, scale) the previous kernel produced and is compared with the reference
evaluated on those very vectors: a stage answers for its own roundings only.  Every comparison is per element or per
channel against that element's or channel's bound (tests/bn_bounds.py, where each bound is derived); one end-to-end case
per shape then takes nothing from the kernels and carries the statistics' own error, |mu - fl32(mu)| scale included."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import bn_bounds as B
import bn_ref as R

pytestmark = pytest.mark.gpu

EPS = float(np.float32(1e-5))          # the ABI takes eps and momentum as fp32: the reference gets the value the kernel got
SENT = 12345.0                         # sentinel of memory the kernels must leave alone
B16_SHAPES = tuple(s for s in B.SHAPES if s[1] % 8 == 0) + ((7, 24), (130, 120))      # (+ C / 8 no power of two)
FUSED_SHAPES = tuple(s for s in B.SHAPES if s[1] % 64 == 0)


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    yield
    B.dump_ratios('MI355X kernels')


def _d(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _n(t):
    return t.detach().float().cpu().numpy() if t.dtype == torch.bfloat16 else t.detach().cpu().numpy()


def _te():
    from grl_amd import train_engine as TE
    return TE


def _call(name, *args):
    TE = _te()
    TE._call(name, *[TE.ptr(a) if torch.is_tensor(a) else a for a in args])


def _rows(M):
    return _te()._lib.load().grl_col_stats_rows(M)


def _f(v):
    return C.c_float(v)


def test_the_sweep_takes_both_branches_of_the_apply_kernels():
    """grid_for's rule restated (bn_bounds.grid_for): the register-resident branch runs iff 256 * grid % (C / 4) == 0."""
    fast = {s: B.apply_takes_fast_branch(*s) for s in B.SHAPES}
    assert any(fast.values()) and not all(fast.values())
    assert not fast[(513, 12)] and not fast[(1, 60)] and fast[(513, 256)] and fast[(1, 4)]
    assert all(_rows(M) == B.chunks(M) for M in B.M_LIST)


# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _forward(M, Cc, cls):
    """Inputs of a case on the device and the kernels' own statistics: col_stats (pivot = row 0) -> finalize."""
    d = B.make_inputs(M, Cc, cls)
    t = {k: _d(v) for k, v in d.items()}
    rows = _rows(M)
    slab = torch.empty(rows, 2, Cc, device='cuda')
    _call('grl_col_stats', t['z'], slab, M, Cc, Cc, t['z'])
    vec = torch.empty(4, Cc, device='cuda')
    _call('grl_bn_stats_finalize', slab, rows, Cc, M, t['gamma'], t['beta'], None, None, None, _f(0.1), _f(EPS),
          vec[0], vec[1], vec[2], vec[3], t['z'])
    torch.cuda.synchronize()
    mean, invstd, scale, shift = (_n(vec[i]) for i in range(4))
    return dict(d=d, t=t, slab=_n(slab), vec=vec, mean=mean, invstd=invstd, scale=scale, shift=shift)


def _scenarios(M, Cc, cls):
    """(z, res) of the residual form and z of the form without one; class (c) moves half of the pre-activations to
    within a few ulp of zero (with the kernels' own mean / scale, which the apply and backward stages take as arguments)."""
    f = _forward(M, Cc, cls)
    d = f['d']
    if cls != 'c':
        return d['z'], d['res'], d['z']
    res, _ = B.near_zero_residual(d['z'], f['mean'], f['scale'], d['beta'], d['res'])
    z2, _ = B.near_zero_z(d['z'], f['mean'], f['scale'], d['beta'])
    return d['z'], res, z2


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('M,Cc', B.SHAPES)
def test_col_stats(M, Cc, cls):
    """grl_col_stats with and without a pivot, on a sub-view (ld > C) of a buffer whose other columns hold a sentinel,
    into a slab with sentinel rows behind it: per chunk and channel inside
    sum: (34 + 1) u sum|d| + u |sum|, sum of squares: (34 + 3) u sum d^2 + u |sum| (times 2)."""
    d = B.make_inputs(M, Cc, cls)
    ld = Cc + 8
    host = np.full((M, ld), SENT, np.float32)
    host[:, 4:4 + Cc] = d['z']
    buf = _d(host)
    rows = _rows(M)
    for pivot in (None, d['z'][0]):
        slab = torch.full((rows + 2, 2, Cc), SENT, device='cuda')
        pv = None if pivot is None else _d(pivot)
        _call('grl_col_stats', buf.data_ptr() + 16, slab, M, Cc, ld, pv)
        torch.cuda.synchronize()
        got = _n(slab)
        assert (got[rows:] == SENT).all(), 'slab rows past grl_col_stats_rows(M) were written'
        assert np.array_equal(_n(buf), host), 'the input (columns past C included) was written'
        for ch in range(rows):
            st = R.stats(d['z'][ch * 128:(ch + 1) * 128], pivot)
            what = (M, Cc, cls, 'pivot' if pivot is not None else 'no pivot', ch)
            B.check('col_stats sum', got[ch, 0], st['sum_d'], B.b_col_sum(st['abs_d'], st['sum_d']), what)
            B.check('col_stats sumsq', got[ch, 1], st['sum_d2'], B.b_col_sumsq(st['sq_d'], st['sum_d2']), what)


@pytest.mark.parametrize('rows', [1, 15, 16, 17, 300])
@pytest.mark.parametrize('Cc', [4, 68, 260])
def test_slab_sum(rows, Cc):
    """grl_slab_sum adds in fp64: the result is the float64 sum rounded once to fp32, plus -- with accumulate -- one fp32
    addition: 2 u (|sum| + |result|)."""
    rng = np.random.RandomState(rows * 1000 + Cc)
    stride = 2 * Cc + 4
    host = (rng.standard_normal((rows, stride)) * 10).astype(np.float32)
    init = rng.standard_normal(Cc + 4).astype(np.float32)
    total = R.f64(host[:, :Cc]).sum(0)
    for acc in (0, 1):
        out = _d(init)
        _call('grl_slab_sum', _d(host), rows, stride, Cc, out, acc)
        got = _n(out)
        assert np.array_equal(got[Cc:], init[Cc:])
        ref = total + (R.f64(init[:Cc]) if acc else 0.0)
        B.check('slab_sum', got[:Cc], ref, B.b_slab_sum(total, ref), (rows, Cc, acc))


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('M,Cc', B.SHAPES)
def test_stats_finalize(M, Cc, cls):
    """grl_bn_stats_finalize on the slab grl_col_stats wrote (bounds: bn_bounds.finalize_bounds): mean, invstd, scale,
    shift; running statistics at momentum 0.1 and 0.5, after one call and after three (count == 1 at M = 1: the biased
    variance is kept); the batch counter; NULL gamma / beta; NULL running statistics."""
    f = _forward(M, Cc, cls)
    d, t = f['d'], f['t']
    rows = _rows(M)
    slab = _d(f['slab'])
    S, Q = R.f64(f['slab'][:, 0]).sum(0), R.f64(f['slab'][:, 1]).sum(0)
    for momentum in (0.1, 0.5):
        mom = float(np.float32(momentum))
        for affine in (True, False):
            g, b = (d['gamma'], d['beta']) if affine else (None, None)
            rm, rv = _d(d['rm']), _d(d['rv'])
            nbt = torch.full((1,), 5, dtype=torch.int64, device='cuda')
            vec = torch.full((4, Cc), SENT, device='cuda')
            ref_rm, ref_rv, b_rm, b_rv = d['rm'], d['rv'], 0.0, 0.0
            for call in range(3):
                _call('grl_bn_stats_finalize', slab, rows, Cc, M, t['gamma'] if affine else None,
                      t['beta'] if affine else None, rm, rv, nbt, _f(momentum), _f(EPS), vec[0], vec[1], vec[2], vec[3], t['z'])
                fb = B.finalize_bounds(S, Q, M, d['z'][0], g, b, ref_rm, ref_rv, mom, EPS, b_rm, b_rv)
                ref_rm, ref_rv = fb['ref']['running_mean'], fb['ref']['running_var']
                b_rm, b_rv = fb['running_mean'], fb['running_var']
                what = (M, Cc, cls, momentum, affine, call)
                B.check('finalize running_mean', _n(rm), ref_rm, b_rm, what)
                B.check('finalize running_var', _n(rv), ref_rv, b_rv, what)
            assert int(nbt) == 8
            if M == 1:
                assert (fb['ref']['unbiased'] == 0).all()          # count == 1: running_var decays towards the biased 0
            B.check('finalize mean', _n(vec[0]), fb['mu'], fb['mean'], what)
            for i, k in ((1, 'invstd'), (2, 'scale'), (3, 'shift')):
                B.check('finalize ' + k, _n(vec[i]), fb['ref'][k], fb[k], what)
            if cls == 'b':                   # the constant channel: var = 0 exactly
                assert _n(vec[0])[1] == 1000.0 and _n(vec[1])[1] == np.float32(1.0 / np.sqrt(EPS))
    vec2 = torch.full((4, Cc), SENT, device='cuda')            # no running statistics, no counter
    _call('grl_bn_stats_finalize', slab, rows, Cc, M, t['gamma'], t['beta'], None, None, None, _f(0.1), _f(EPS),
          vec2[0], vec2[1], vec2[2], vec2[3], t['z'])
    assert torch.equal(vec2, f['vec'])


def _apply(z, f, beta, res, relu, bits_on, M, Cc, dtype=torch.float32):
    y = torch.full((M, Cc), SENT, device='cuda').to(dtype)
    per = 8 if dtype == torch.bfloat16 else 4
    bits = torch.full((M * Cc // per + 3,), 0xAB, dtype=torch.uint8, device='cuda') if bits_on else None
    name = 'grl_bn_apply_centered' + ('_bf16' if dtype == torch.bfloat16 else '')
    _call(name, z, f['vec'][0], f['vec'][2], beta, res, y, M, Cc, 1 if relu else 0, bits)
    torch.cuda.synchronize()
    return y, bits


def _bits_of(y, per):
    """the (y > 0) bytes the kernels record: bit e of byte i = (y.flat[per * i + e] > 0)"""
    m = (y.reshape(-1, per) > 0).astype(np.uint8)
    return (m << np.arange(per, dtype=np.uint8)[None, :]).sum(1).astype(np.uint8)


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('M,Cc', B.SHAPES)
def test_apply_centered(M, Cc, cls):
    """grl_bn_apply_centered, {res, none} x {relu, none} x {bits, none}: y inside 4 u (|z - mean| |scale| + |beta| + |res|)
    (times 2) per element; the bits byte for byte (y > 0) of the kernel's own y; nothing written past them."""
    f = _forward(M, Cc, cls)
    d, t = f['d'], f['t']
    z_r, res_c, z_z = _scenarios(M, Cc, cls)
    near = 0
    for res_on in (False, True):
        z = z_r if res_on else z_z
        res = res_c if res_on else None
        zt, rt = _d(z), (None if res is None else _d(res))
        for relu in (False, True):
            fw = R.apply_centered(z, f['mean'], f['scale'], d['beta'], res, relu)
            bound = B.b_apply(fw['abs_terms'])
            near = max(near, int((np.abs(fw['pre']) <= bound).sum()))
            for bits_on in (False, True):
                y, bits = _apply(zt, f, t['beta'], rt, relu, bits_on, M, Cc)
                got = _n(y)
                B.check('apply y', got, fw['y'], bound, (M, Cc, cls, res_on, relu, bits_on))
                if bits_on:
                    bb = _n(bits)
                    assert np.array_equal(bb[:M * Cc // 4], _bits_of(got, 4)) and (bb[M * Cc // 4:] == 0xAB).all()
            if cls == 'b':                   # constant channel: y = beta (+ res), exactly
                want = d['beta'][1] + (res[:, 1] if res_on else np.float32(0))
                assert (got[:, 1] == (np.maximum(want, np.float32(0)) if relu else want)).all()
    # NULL beta
    y = torch.empty(M, Cc, device='cuda')
    _call('grl_bn_apply_centered', _d(z_r), f['vec'][0], f['vec'][2], None, None, y, M, Cc, 0, None)
    fw = R.apply_centered(z_r, f['mean'], f['scale'])
    B.check('apply y', _n(y), fw['y'], B.b_apply(fw['abs_terms']), (M, Cc, cls, 'no beta'))
    print('apply %dx%d (%s): %d pre-activations within their error bound of zero' % (M, Cc, cls, near))
    if cls == 'c' and M * Cc >= 64:
        assert near > 0


def _check_backward(stage, got_dz, got_dg, got_db, bw, M, Cc, dg0, db0, what, k=None, slab_exact=None):
    """dz, dgamma, dbeta of one backward call against bn_ref.backward (bounds: bn_bounds.b_sum_g / b_sum_gx /
    b_accumulate / b_coef / b_dz)."""
    gx = bw['g'] * bw['xhat']
    g_ch, gx_ch = B.chunk_sums(bw['g']), B.chunk_sums(gx)
    if slab_exact is not None:               # the sums were handed over as an fp32 slab: one rounding per chunk
        b_g = B.SAFETY * B.U * np.abs(g_ch).sum(0)
        b_gx = B.SAFETY * B.U * np.abs(gx_ch).sum(0)
    elif k is not None:                      # bf16 twins: their own depth
        b_g = B.SAFETY * (k * B.U * bw['abs_g'] + B.U * np.abs(g_ch).sum(0))
        b_gx = B.SAFETY * ((k + 3) * B.U * bw['abs_gx'] + B.U * np.abs(gx_ch).sum(0))
    else:
        b_g = B.b_sum_g(B.chunk_sums(np.abs(bw['g'])), g_ch, Cc)
        b_gx = B.b_sum_gx(B.chunk_sums(np.abs(gx)), gx_ch, Cc)
    B.check(stage + ' dbeta', got_db, R.f64(db0) + bw['dbeta'], B.b_accumulate(b_g, bw['sum_g'], R.f64(db0)), what)
    B.check(stage + ' dgamma', got_dg, R.f64(dg0) + bw['dgamma'], B.b_accumulate(b_gx, bw['sum_gx'], R.f64(dg0)), what)
    bound = B.b_dz(bw, B.b_coef(b_g, bw['sum_g'], M), B.b_coef(b_gx, bw['sum_gx'], M))
    if got_dz is not None:
        B.check(stage + ' dz', got_dz, bw['dz'], bound, what)
    return bound


def _bwd(name, dy, z, act, f, gamma, M, Cc, dg0, db0, gres=None, acc=0, from_z=False, bits=None, dtype=torch.float32, beta=None):
    dz = torch.full((M, Cc), SENT, device='cuda').to(dtype)
    dg, db = _d(dg0), _d(db0)
    rows = _rows(M)
    slab = torch.empty(rows, 2, Cc, device='cuda')
    coef = torch.empty(2, Cc, device='cuda')
    _call(name, dy, z, act, f['vec'][0], f['vec'][1], gamma, dz, dg, db, slab, coef, M, Cc, gres, acc,
          f['vec'][2] if from_z else None, beta if from_z else None, bits)
    torch.cuda.synchronize()
    return _n(dz), _n(dg), _n(db)


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('M,Cc', B.SHAPES)
def test_bn_bwd(M, Cc, cls):
    """grl_bn_bwd in its five forms -- mask from the activation, from the recorded bits, recomputed from z, no mask, in place
    (gres == dy) -- and gres written / accumulated; dgamma and dbeta accumulate onto non-zero values.  The mask the
    reference uses is (y > 0) of the kernel's own fp32 y: a pre-activation a few ulp from zero may fall on either side."""
    f = _forward(M, Cc, cls)
    d, t = f['d'], f['t']
    z_r, res_c, z_z = _scenarios(M, Cc, cls)
    zr_t, zz_t = _d(z_r), _d(z_z)
    y_r, bits_r = _apply(zr_t, f, t['beta'], _d(res_c), True, True, M, Cc)
    y_z, _ = _apply(zz_t, f, t['beta'], None, True, False, M, Cc)
    mask_r, mask_z = _n(y_r) > 0, _n(y_z) > 0
    dg0, db0 = d['dgamma0'], d['dbeta0']
    bw_r = R.backward(d['dy'], z_r, mask_r, f['mean'], f['invstd'], d['gamma'])
    g32 = np.where(mask_r, d['dy'], np.float32(0))
    for form in ('act', 'bits'):
        for acc in (0, 1):
            gres = _d(d['gres0'])
            out = _bwd('grl_bn_bwd', t['dy'], zr_t, y_r if form == 'act' else None, f, t['gamma'], M, Cc, dg0, db0,
                       gres=gres, acc=acc, bits=bits_r[:M * Cc // 4] if form == 'bits' else None)
            _check_backward('bwd', *out, bw_r, M, Cc, dg0, db0, (M, Cc, cls, form, acc))
            if acc:          # one fp32 addition: u |result| (times 2)
                want = R.f64(g32) + R.f64(d['gres0'])
                B.check('bwd gres', _n(gres), want, B.SAFETY * B.U * np.abs(want), (M, Cc, cls, form))
            else:
                assert np.array_equal(_n(gres), g32)
    dy2 = _d(d['dy'])                                            # in place: dy becomes the masked gradient
    out = _bwd('grl_bn_bwd', dy2, zr_t, y_r, f, t['gamma'], M, Cc, dg0, db0, gres=dy2, acc=0)
    _check_backward('bwd', *out, bw_r, M, Cc, dg0, db0, (M, Cc, cls, 'in place'))
    assert np.array_equal(_n(dy2), g32)
    bw_z = R.backward(d['dy'], z_z, mask_z, f['mean'], f['invstd'], d['gamma'])
    out = _bwd('grl_bn_bwd', t['dy'], zz_t, None, f, t['gamma'], M, Cc, dg0, db0, from_z=True, beta=t['beta'])
    _check_backward('bwd', *out, bw_z, M, Cc, dg0, db0, (M, Cc, cls, 'mask from z'))
    bw_n = R.backward(d['dy'], z_r, None, f['mean'], f['invstd'], d['gamma'])
    out = _bwd('grl_bn_bwd', t['dy'], zr_t, None, f, t['gamma'], M, Cc, dg0, db0)
    _check_backward('bwd', *out, bw_n, M, Cc, dg0, db0, (M, Cc, cls, 'no mask'))
    bw_1 = R.backward(d['dy'], z_r, None, f['mean'], f['invstd'], None)           # NULL gamma, NULL dgamma / dbeta
    dz = torch.empty(M, Cc, device='cuda')
    _call('grl_bn_bwd', t['dy'], zr_t, None, f['vec'][0], f['vec'][1], None, dz, None, None,
          torch.empty(_rows(M), 2, Cc, device='cuda'), torch.empty(2, Cc, device='cuda'), M, Cc, None, 0, None, None, None)
    _check_backward('bwd', _n(dz), bw_1['dgamma'], bw_1['dbeta'], bw_1, M, Cc, 0 * dg0, 0 * db0, (M, Cc, cls, 'no gamma'))


@pytest.mark.parametrize('M,Cc', B.SHAPES)
def test_bn_bwd_finish(M, Cc):
    """grl_bn_bwd_finish on a slab of the reference's own masked gradient (per chunk float64 sums, rounded once to fp32:
    u |chunk sum| is all the sums can be off by): finalize + apply alone."""
    f = _forward(M, Cc, 'a')
    d, t = f['d'], f['t']
    y, _ = _apply(t['z'], f, t['beta'], t['res'], True, False, M, Cc)
    mask = _n(y) > 0
    bw = R.backward(d['dy'], d['z'], mask, f['mean'], f['invstd'], d['gamma'])
    g32 = np.where(mask, d['dy'], np.float32(0))
    rows = _rows(M)
    slab = np.stack([B.chunk_sums(bw['g']), B.chunk_sums(bw['g'] * bw['xhat'])], 1).astype(np.float32)
    for acc in (0, 1):
        dz = torch.full((M, Cc), SENT, device='cuda')
        dg, db, gres = _d(d['dgamma0']), _d(d['dbeta0']), _d(d['gres0'])
        _call('grl_bn_bwd_finish', _d(g32), t['z'], f['vec'][0], f['vec'][1], t['gamma'], dz, dg, db, _d(slab), rows,
              torch.empty(2, Cc, device='cuda'), M, Cc, gres, acc)
        _check_backward('bwd_finish', _n(dz), _n(dg), _n(db), bw, M, Cc, d['dgamma0'], d['dbeta0'], (M, Cc, acc),
                        slab_exact=True)
        want = R.f64(g32) + (R.f64(d['gres0']) if acc else 0.0)
        B.check('bwd_finish gres', _n(gres), want, B.SAFETY * B.U * np.abs(want), (M, Cc, acc))


# ----------------------------------------------------------------------------------------------------------------------
# bf16-storage twins
def _b16_inputs(M, Cc, cls):
    d = dict(B.make_inputs(M, Cc, cls))
    for k in ('z', 'res', 'dy', 'gres0'):
        d[k] = B.bf16_round(d[k]).astype(np.float32)           # bf16-representable
    if cls == 'b':
        d['z'][:, 1] = 1000.0
    return d


def _check_b16(stage, got, ref, fp32_bound, what):
    """a stored bf16 output against the reference rounded to bf16: the fp32 value the kernel rounded is within fp32_bound of
    the reference, so the two roundings differ by at most one bf16 spacing (taken at the larger of the two magnitudes) on
    top of it."""
    rb = B.bf16_round(ref)
    B.check(stage, got, rb, B.bf16_ulp(np.maximum(np.abs(rb), np.abs(got))) + fp32_bound, what)


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('M,Cc', B16_SHAPES)
def test_bf16_twins(M, Cc, cls):
    """grl_col_stats_bf16, grl_bn_apply_centered_bf16, grl_bn_bwd_bf16 on bf16-representable inputs.  Their column sums are
    fp32 with the depth of bn_bounds.k_bf16_reduce; stored tensors are bf16.  (7 x 24 and 130 x 120: C / 8 is no power of
    two -- the lanes-per-row rule once rounded it down to one and left the last channel groups of a row without a lane.)"""
    d = _b16_inputs(M, Cc, cls)
    BF = torch.bfloat16
    t = {k: _d(v) for k, v in d.items()}
    z16, res16, dy16 = t['z'].to(BF), t['res'].to(BF), t['dy'].to(BF)
    rows, k = _rows(M), B.k_bf16_reduce(Cc)
    pivot = d['z'][0]
    ld = Cc + 16                                   # a sub-view: 8 sentinel columns on either side of z
    buf = torch.full((M, ld), SENT, device='cuda').to(BF)
    buf[:, 8:8 + Cc] = z16
    before = buf.clone()
    for pv in (None, pivot):
        slab = torch.full((rows + 2, 2, Cc), SENT, device='cuda')
        _call('grl_col_stats_bf16', buf.data_ptr() + 16, slab, M, Cc, ld, None if pv is None else _d(pv))
        got = _n(slab)
        assert (got[rows:] == SENT).all(), 'slab rows past grl_col_stats_rows(M) were written'
        assert torch.equal(buf, before), 'the input (columns past C included) was written'
        for ch in range(rows):
            st = R.stats(d['z'][ch * 128:(ch + 1) * 128], pv)
            B.check('bf16 col_stats sum', got[ch, 0], st['sum_d'], B.b_col_sum(st['abs_d'], st['sum_d'], k), (M, Cc, cls, ch))
            B.check('bf16 col_stats sumsq', got[ch, 1], st['sum_d2'], B.b_col_sumsq(st['sq_d'], st['sum_d2'], k), (M, Cc, cls, ch))
        slab = slab[:rows].contiguous()
    vec = torch.empty(4, Cc, device='cuda')
    _call('grl_bn_stats_finalize', slab, rows, Cc, M, t['gamma'], t['beta'], None, None, None, _f(0.1), _f(EPS),
          vec[0], vec[1], vec[2], vec[3], _d(pivot))
    f = dict(vec=vec, mean=_n(vec[0]), invstd=_n(vec[1]), scale=_n(vec[2]))
    res = d['res']
    if cls == 'c':           # bf16-representable residuals next to -(pre-activation): the stored y straddles zero
        res, _ = B.near_zero_residual(d['z'], f['mean'], f['scale'], d['beta'], d['res'])
        res = B.bf16_round(res).astype(np.float32)
        res16 = _d(res).to(BF)
    ys = {}
    for res_on in (False, True):
        for relu in (False, True):
            fw = R.apply_centered(d['z'], f['mean'], f['scale'], d['beta'], res if res_on else None, relu)
            y, bits = _apply(z16, f, t['beta'], res16 if res_on else None, relu, True, M, Cc, dtype=BF)
            got = _n(y)
            _check_b16('bf16 apply y', got, fw['y'], B.b_apply(fw['abs_terms']), (M, Cc, cls, res_on, relu))
            bb = _n(bits)
            assert np.array_equal(bb[:M * Cc // 8], _bits_of(got, 8)) and (bb[M * Cc // 8:] == 0xAB).all()
            ys[(res_on, relu)] = (y, bits, got)
    dg0, db0 = d['dgamma0'], d['dbeta0']
    y_r, bits_r, got_r = ys[(True, True)]
    mask_r = got_r > 0
    g32 = np.where(mask_r, d['dy'], np.float32(0))
    bw_r = R.backward(d['dy'], d['z'], mask_r, f['mean'], f['invstd'], d['gamma'])
    bw_z = R.backward(d['dy'], d['z'], ys[(False, True)][2] > 0, f['mean'], f['invstd'], d['gamma'])
    bw_n = R.backward(d['dy'], d['z'], None, f['mean'], f['invstd'], d['gamma'])
    runs = [('act', bw_r, dict(act=y_r)), ('bits', bw_r, dict(bits=bits_r[:M * Cc // 8])),
            ('mask from z', bw_z, dict(from_z=True, beta=t['beta'])), ('no mask', bw_n, dict())]
    for form, bw, kw in runs:
        for acc in ((0, 1) if form in ('act', 'bits') else (None,)):
            gres = None if acc is None else t['gres0'].to(BF)
            act = kw.get('act')
            dz, dg, db = _bwd('grl_bn_bwd_bf16', dy16, z16, act, f, t['gamma'], M, Cc, dg0, db0, gres=gres, acc=acc or 0,
                              dtype=BF, **{a: b for a, b in kw.items() if a != 'act'})
            bound = _check_backward('bf16 bwd', None, dg, db, bw, M, Cc, dg0, db0, (M, Cc, cls, form, acc), k=k)
            _check_b16('bf16 bwd dz', dz, bw['dz'], bound, (M, Cc, cls, form, acc))
            if acc is not None:
                want = R.f64(g32) + (R.f64(d['gres0']) if acc else 0.0)
                if acc:      # one fp32 addition, then the bf16 store
                    _check_b16('bf16 bwd gres', _n(gres), want, B.SAFETY * B.U * np.abs(want), (M, Cc, cls, form, acc))
                else:
                    assert np.array_equal(_n(gres), g32)
    dy2 = dy16.clone()
    dz, dg, db = _bwd('grl_bn_bwd_bf16', dy2, z16, y_r, f, t['gamma'], M, Cc, dg0, db0, gres=dy2, acc=0, dtype=BF)
    bound = _check_backward('bf16 bwd', None, dg, db, bw_r, M, Cc, dg0, db0, (M, Cc, cls, 'in place'), k=k)
    _check_b16('bf16 bwd dz', dz, bw_r['dz'], bound, (M, Cc, cls, 'in place'))
    assert np.array_equal(_n(dy2), g32)


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('M,Cc', FUSED_SHAPES)
def test_finalize_inside_the_apply_pass_against_float64(M, Cc, cls):
    """The fused form (set_bn_finapply(True): grl_bn_finalize_apply forward, the fused finalize + apply inside grl_bn_bwd) at
    its eligible shapes -- C % 64 == 0, at most 64 slab rows -- held to the same float64 bounds as the separate launches."""
    TE = _te()
    f0 = _forward(M, Cc, cls)
    d, t = f0['d'], f0['t']
    rows = _rows(M)
    S, Q = R.f64(f0['slab'][:, 0]).sum(0), R.f64(f0['slab'][:, 1]).sum(0)
    was = TE.set_bn_finapply(True)
    try:
        assert TE._lib.load().grl_bn_finalize_apply_takes(rows, Cc) == 1
        rm, rv = _d(d['rm']), _d(d['rv'])
        nbt = torch.zeros(1, dtype=torch.int64, device='cuda')
        vec = torch.full((4, Cc), SENT, device='cuda')
        y = torch.full((M, Cc), SENT, device='cuda')
        bits = torch.full((M * Cc // 4 + 3,), 0xAB, dtype=torch.uint8, device='cuda')
        _call('grl_bn_finalize_apply', _d(f0['slab']), rows, Cc, M, t['gamma'], t['beta'], rm, rv, nbt, _f(0.1), _f(EPS),
              vec[0], vec[1], vec[2], vec[3], t['z'], t['z'], t['res'], y, M, 1, bits)
        torch.cuda.synchronize()
        fb = B.finalize_bounds(S, Q, M, d['z'][0], d['gamma'], d['beta'], d['rm'], d['rv'], float(np.float32(0.1)), EPS)
        what = (M, Cc, cls)
        B.check('fused finalize mean', _n(vec[0]), fb['mu'], fb['mean'], what)
        for i, k in ((1, 'invstd'), (2, 'scale'), (3, 'shift')):
            B.check('fused finalize ' + k, _n(vec[i]), fb['ref'][k], fb[k], what)
        B.check('fused finalize running_mean', _n(rm), fb['ref']['running_mean'], fb['running_mean'], what)
        B.check('fused finalize running_var', _n(rv), fb['ref']['running_var'], fb['running_var'], what)
        assert int(nbt) == 1
        f = dict(vec=vec, mean=_n(vec[0]), invstd=_n(vec[1]), scale=_n(vec[2]))
        fw = R.apply_centered(d['z'], f['mean'], f['scale'], d['beta'], d['res'], True)
        got = _n(y)
        B.check('fused apply y', got, fw['y'], B.b_apply(fw['abs_terms']), what)
        bb = _n(bits)
        assert np.array_equal(bb[:M * Cc // 4], _bits_of(got, 4)) and (bb[M * Cc // 4:] == 0xAB).all()
        mask = got > 0
        bw = R.backward(d['dy'], d['z'], mask, f['mean'], f['invstd'], d['gamma'])
        g32 = np.where(mask, d['dy'], np.float32(0))
        for form in ('act', 'bits', 'in place'):
            dy = _d(d['dy'])
            gres = dy if form == 'in place' else _d(d['gres0'])
            out = _bwd('grl_bn_bwd', dy, t['z'], None if form == 'bits' else y, f, t['gamma'], M, Cc, d['dgamma0'], d['dbeta0'],
                       gres=gres, acc=0, bits=bits[:M * Cc // 4] if form == 'bits' else None)
            _check_backward('fused bwd', *out, bw, M, Cc, d['dgamma0'], d['dbeta0'], (M, Cc, cls, form))
            assert np.array_equal(_n(gres), g32)
    finally:
        TE.set_bn_finapply(was)


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,Cc', B.SHAPES)
def test_end_to_end_against_float64(M, Cc):
    """col_stats -> finalize -> apply -> backward on class (a) inputs against float64 relu(bn(z) + res) and its gradient,
    with NOTHING taken from the kernels: the statistics' own errors now count.
    mean:   B_mu = (sum bound) / M + 2 u |mu|                       -- the second term is |mu - fl32(mu)|, stated explicitly;
    var:    B_var = (sum-of-squares bound) / M + 2 |md| (sum bound) / M,   md = mean of (z - pivot);
    invstd: B_is = 2 u invstd + invstd^3 B_var / 2;        xhat: B_xh = B_mu invstd + |z - mu| B_is;
    y:      apply bound + B_mu |scale| + |z - mu| (|gamma| B_is + 2 u |scale|)   (scale = fl(gamma invstd_f));
    dgamma: its sum bound + sum_r |g| B_xh;
    dz:     backward bound (with that dgamma bound in k1) + |gamma| B_is |g - k0 - xhat k1| + |gm| B_xh |k1|.
    A pre-activation within its y bound of zero may take either side of the ReLU: the kernel's side is adopted for those
    elements (and only those)."""
    f = _forward(M, Cc, 'a')
    d, t = f['d'], f['t']
    z64 = R.f64(d['z'])
    st = R.stats(z64, z64[0])
    fin = R.finalize(st['mean'], st['var'], M, d['gamma'], d['beta'], None, None, 0.1, EPS)
    gam = np.abs(R.f64(d['gamma']))
    b_s = B.b_col_sum(B.chunk_sums(np.abs(z64 - z64[0])).sum(0), 0.0) + B.SAFETY * B.U * np.abs(B.chunk_sums(z64 - z64[0])).sum(0)
    b_q = B.b_col_sumsq(st['sq_d'], 0.0) + B.SAFETY * B.U * st['sq_d']
    b_mu = b_s / M + B.SAFETY * B.U * np.abs(st['mean'])
    b_var = b_q / M + 2 * np.abs(st['sum_d'] / M) * b_s / M
    is_ = fin['invstd']
    b_is = B.SAFETY * B.U * is_ + 0.5 * is_ ** 3 * b_var
    B.check('end to end mean', f['mean'], st['mean'], b_mu, (M, Cc))
    B.check('end to end invstd', f['invstd'], is_, b_is, (M, Cc))
    y, _ = _apply(t['z'], f, t['beta'], t['res'], True, False, M, Cc)
    got = _n(y)
    fw = R.apply_centered(z64, st['mean'], fin['scale'], d['beta'], d['res'], True)
    zc = np.abs(z64 - st['mean'][None, :])
    b_xh = b_mu[None, :] * is_[None, :] + zc * b_is[None, :]
    b_scale = gam * b_is + B.SAFETY * B.U * np.abs(fin['scale'])             # scale = fl(gamma * invstd_f)
    b_y = B.b_apply(fw['abs_terms']) + (b_mu * np.abs(fin['scale']))[None, :] + zc * b_scale[None, :]
    B.check('end to end y', got, fw['y'], b_y, (M, Cc))
    mask = np.where(np.abs(fw['pre']) <= b_y, got > 0, fw['mask'])
    assert np.array_equal(mask, got > 0)
    dz, dg, db = _bwd('grl_bn_bwd', t['dy'], t['z'], y, f, t['gamma'], M, Cc, 0 * d['dgamma0'], 0 * d['dbeta0'])
    bw = R.backward(d['dy'], z64, mask, st['mean'], is_, d['gamma'])
    gx = bw['g'] * bw['xhat']
    b_g = B.b_sum_g(B.chunk_sums(np.abs(bw['g'])), B.chunk_sums(bw['g']), Cc)
    b_gx = B.b_sum_gx(B.chunk_sums(np.abs(gx)), B.chunk_sums(gx), Cc) + (np.abs(bw['g']) * b_xh).sum(0)
    B.check('end to end dbeta', db, bw['dbeta'], B.b_accumulate(b_g, bw['sum_g'], 0.0), (M, Cc))
    B.check('end to end dgamma', dg, bw['dgamma'], B.b_accumulate(b_gx, bw['sum_gx'], 0.0), (M, Cc))
    inner = np.abs(bw['g'] - (bw['sum_g'] / M)[None, :] - bw['xhat'] * (bw['sum_gx'] / M)[None, :])
    b_dz = (B.b_dz(bw, B.b_coef(b_g, bw['sum_g'], M), B.b_coef(b_gx, bw['sum_gx'], M))
            + (gam * b_is)[None, :] * inner + np.abs(bw['gm'])[None, :] * b_xh * np.abs(bw['sum_gx'] / M)[None, :])
    B.check('end to end dz', dz, bw['dz'], b_dz, (M, Cc))


# ----------------------------------------------------------------------------------------------------------------------
CONV_CASES = [(64, 64, 3, 1, 16, 8, 4), (256, 512, 1, 2, 8, 8, 4)]          # one 3x3 layer, one 1x1 stride-2 layer


@functools.lru_cache(maxsize=None)
def _conv_case(cin, cout, k, stride, H, W, n):
    """One train_engine.conv_bn layer (ReLU, no residual), forward and backward, on NON-NEGATIVE inputs
    (relu(randn) + 0.5, as real layers see them: the conv outputs have non-zero means); everything back on the host."""
    import torch.nn as nn
    TE = _te()
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(cin + cout + k)
    conv = nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=False)
    bn = nn.BatchNorm2d(cout)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (cin * k * k)) ** 0.5)
        bn.weight.copy_(torch.rand(cout, generator=g) + 0.5); bn.bias.copy_(torch.rand(cout, generator=g) * 1.4 - 0.7)
    w, gamma, beta = conv.weight.detach().clone(), bn.weight.detach().numpy().copy(), bn.bias.detach().numpy().copy()
    conv.to(dev); bn.to(dev)
    x = torch.relu(torch.randn(n, cin, H, W, generator=g)) + 0.5
    xd = x.permute(0, 2, 3, 1).contiguous().view(-1, cin).to(dev)
    tp = TE.Tape(dev)
    a, Ho, Wo, z = TE.conv_bn(tp, xd, n, H, W, conv, bn, True)
    M = n * Ho * Wo
    vec = _n(tp.bnrec[id(a)].st.buf)
    gout = torch.randn(M, cout, generator=g)
    out = dict(x=x, w=w, gamma=gamma, beta=beta, M=M, Ho=Ho, Wo=Wo, mean=vec[0], invstd=vec[1], scale=vec[2], z=_n(z), y=_n(a),
               rm=_n(bn.running_mean), rv=_n(bn.running_var), gout=gout.numpy())
    tp.g[id(a)] = gout.to(dev)
    tp.backward()
    out.update(dx=_n(tp.take(xd)), dw=_n(tp.pgrad(conv.weight)), dgamma=_n(tp.pgrad(bn.weight)), dbeta=_n(tp.pgrad(bn.bias)))
    return out


def _epilogue_bounds(z64, M):
    """The GEMM epilogue's sums of z and z^2 (NO pivot), at most K_GEMM_STATS = 34 additions deep per tile of at most 128
    rows, fp64 across tiles:  sum z: 34 u sum|z| + u sum|tile sums|;  sum z^2: (34 + 1) u sum z^2 + u sum z^2 (the square
    rounds once) (times 2).  Returns B_S, B_Q."""
    tiles = np.add.reduceat(z64, np.arange(0, M, 64), axis=0)           # tiles have 64 or 128 rows: the finer split bounds both
    q = (z64 * z64).sum(0)
    return (B.SAFETY * (B.K_GEMM_STATS * B.U * np.abs(z64).sum(0) + B.U * np.abs(tiles).sum(0)),
            B.SAFETY * ((B.K_GEMM_STATS + 1) * B.U * q + B.U * q))


@pytest.mark.parametrize('cin,cout,k,stride,H,W,n', CONV_CASES)
def test_conv_path_statistics_from_the_gemm_epilogue(cin, cout, k, stride, H, W, n):
    """The BatchNorm part of conv_bn in isolation: float64 taken on the kernel's own z.  The statistics come from the GEMM
    epilogue (_epilogue_bounds), so var = Q / M - mean^2 is off by B_var = B_Q / M + 2 |mean| B_S / M -- growing with
    mean^2 / var, which is printed (and recorded in EXPERIMENTS.md) rather than asserted.  Per channel: mean, invstd,
    running_mean, running_var, y, dgamma, dbeta.  (test_conv_path_against_float64_autograd takes nothing from the kernel.)"""
    c = _conv_case(cin, cout, k, stride, H, W, n)
    M, mean_k, invstd_k, scale_k = c['M'], c['mean'], c['invstd'], c['scale']
    zk = R.f64(c['z'])
    ref = R.stats(zk)
    b_S, b_Q = _epilogue_bounds(zk, M)
    b_mu = b_S / M + B.SAFETY * B.U * np.abs(ref['mean'])
    b_var = b_Q / M + 2 * np.abs(ref['mean']) * b_S / M
    fin = R.finalize(ref['mean'], ref['var'], M, c['gamma'], c['beta'], np.zeros(cout), np.ones(cout),
                     float(np.float32(0.1)), EPS)
    is_ = fin['invstd']
    b_is = B.SAFETY * B.U * is_ + 0.5 * is_ ** 3 * b_var
    what = (cin, cout, k, stride)
    B.check('conv mean', mean_k, ref['mean'], b_mu, what)
    B.check('conv invstd', invstd_k, is_, b_is, what)
    B.check('conv running_mean', c['rm'], fin['running_mean'],
            0.1 * b_mu + B.SAFETY * B.U * (2 * 0.1 * np.abs(ref['mean']) + np.abs(fin['running_mean'])), what)
    unb = M / (M - 1.0)
    B.check('conv running_var', c['rv'], fin['running_var'],
            0.1 * unb * b_var + B.SAFETY * B.U * (2 * 0.9 + 2 * 0.1 * fin['unbiased'] + fin['running_var']), what)
    var_k = 1.0 / R.f64(invstd_k) ** 2 - EPS
    print('conv %s: |mean| / std of z: median %.2f, max %.2f; relative error of the batch variance: max %.2e (bound %.2e)' % (
        what, float(np.median(np.abs(ref['mean']) / np.sqrt(ref['var']))), float((np.abs(ref['mean']) / np.sqrt(ref['var'])).max()),
        float((np.abs(var_k - ref['var']) / ref['var']).max()), float((b_var / ref['var']).max())))
    fw = R.apply_centered(zk, mean_k, scale_k, c['beta'], None, True)
    B.check('conv y', c['y'], fw['y'], B.b_apply(fw['abs_terms']), what)
    bw = R.backward(c['gout'], zk, c['y'] > 0, mean_k, invstd_k, c['gamma'])
    gx = bw['g'] * bw['xhat']
    b_g = B.b_sum_g(B.chunk_sums(np.abs(bw['g'])), B.chunk_sums(bw['g']), cout)
    b_gx = B.b_sum_gx(B.chunk_sums(np.abs(gx)), B.chunk_sums(gx), cout)
    B.check('conv dbeta', c['dbeta'], bw['dbeta'], B.b_accumulate(b_g, bw['sum_g'], 0.0), what)
    B.check('conv dgamma', c['dgamma'], bw['dgamma'], B.b_accumulate(b_gx, bw['sum_gx'], 0.0), what)


def _rows_of(t):
    """NCHW tensor -> channels-last rows [n H W][C] (float64 numpy)"""
    return t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1]).double().numpy()


def _nchw(a, n, Ho, Wo):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).view(n, Ho, Wo, -1).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize('cin,cout,k,stride,H,W,n', CONV_CASES)
def test_conv_path_against_float64_autograd(cin, cout, k, stride, H, W, n):
    """conv_bn against torch float64 autograd of relu(BatchNorm2d(Conv2d(x))) on the same non-negative input, NOTHING taken
    from the kernels: mean, running_var, y, dx, dw, dgamma, dbeta, per channel / per element.  First-order bounds, u = 2^-24,
    each term times 2 (SAFETY):
      z:      a dot product of K = k k cin fp32 terms accumulated in fp32 in any order: B_z = K u (|x| * |w|)  (* = the conv);
      mean:   B_mu = mean_r B_z + B_S / M + u |mu|         (B_S, B_Q: the epilogue's sums, _epilogue_bounds);
      var:    B_var = (2 / M) sum_r |z - mu| B_z + B_Q / M + 2 |mu| B_S / M;   running_var: m M / (M - 1) B_var + its roundings;
      invstd: B_is = u is + is^3 B_var / 2;     xhat: B_xh = (B_z + B_mu) is + |z - mu| B_is;
      y:      apply bound + (B_z + B_mu) |scale| + |z - mu| (|gamma| B_is + u |scale|);
      dbeta:  its sum bound;     dgamma: its sum bound + sum_r |g| B_xh;
      dz:     backward bound (those two in k0, k1) + |gamma| B_is |g - k0 - xhat k1| + |gm| B_xh |k1|;
      dx:     (B_dz *^T |w|) + k k cout u (|dz| *^T |w|)      (*^T = the conv's transpose: the data-gradient GEMM);
      dw:     (B_dz x |x|) + M u (|dz| x |x|)                  (x = the weight-gradient correlation, M terms per element).
    A pre-activation within its y bound of zero may take either side of the ReLU; the kernel's side is adopted for those
    elements only (the float64 graph multiplies by that fixed mask)."""
    import torch.nn.functional as F
    from torch.nn.grad import conv2d_input, conv2d_weight
    c = _conv_case(cin, cout, k, stride, H, W, n)
    M, Ho, Wo, pad = c['M'], c['Ho'], c['Wo'], k // 2
    what = (cin, cout, k, stride)
    x64 = c['x'].double().requires_grad_(True)
    w64 = c['w'].double().requires_grad_(True)
    gam_t = torch.from_numpy(R.f64(c['gamma'])).requires_grad_(True)
    bet_t = torch.from_numpy(R.f64(c['beta'])).requires_grad_(True)
    rm, rv = torch.zeros(cout, dtype=torch.float64), torch.ones(cout, dtype=torch.float64)
    mom = float(np.float32(0.1))
    zt = F.conv2d(x64, w64, stride=stride, padding=pad)
    pre = F.batch_norm(zt, rm, rv, gam_t, bet_t, True, mom, EPS)
    z64 = _rows_of(zt)
    # ---- forward bounds
    K = k * k * cin
    b_z = B.SAFETY * K * B.U * _rows_of(F.conv2d(c['x'].double().abs(), c['w'].double().abs(), stride=stride, padding=pad))
    st = R.stats(z64)
    mu, var = st['mean'], st['var']
    zc = np.abs(z64 - mu[None, :])
    b_S, b_Q = _epilogue_bounds(z64, M)
    b_mu = b_z.mean(0) + b_S / M + B.SAFETY * B.U * np.abs(mu)
    b_var = (2.0 / M) * (zc * b_z).sum(0) + b_Q / M + 2 * np.abs(mu) * b_S / M
    is_ = 1.0 / np.sqrt(var + EPS)
    b_is = B.SAFETY * B.U * is_ + 0.5 * is_ ** 3 * b_var
    gam = np.abs(R.f64(c['gamma']))
    scale = gam * is_
    B.check('conv64 mean', c['mean'], mu, b_mu, what)
    unb = M / (M - 1.0)
    B.check('conv64 running_var', c['rv'], rv.numpy(),
            mom * unb * b_var + B.SAFETY * B.U * (2 * (1 - mom) + 2 * mom * var * unb + np.abs(rv.numpy())), what)
    B.check('conv64 running_mean', c['rm'], rm.numpy(),
            mom * b_mu + B.SAFETY * B.U * (2 * mom * np.abs(mu) + np.abs(rm.numpy())), what)
    pre64 = _rows_of(pre)
    abs_terms = zc * scale[None, :] + np.abs(R.f64(c['beta']))[None, :]
    b_xh = (b_z + b_mu[None, :]) * is_[None, :] + zc * b_is[None, :]
    b_y = (B.b_apply(abs_terms) + (b_z + b_mu[None, :]) * scale[None, :]
           + zc * (gam * b_is + B.SAFETY * B.U * scale)[None, :])
    B.check('conv64 y', c['y'], np.maximum(pre64, 0.0), b_y, what)
    mask = np.where(np.abs(pre64) <= b_y, c['y'] > 0, pre64 > 0)
    assert np.array_equal(mask, c['y'] > 0)
    print('conv64 %s: %d of %d pre-activations within their bound of zero' % (what, int((np.abs(pre64) <= b_y).sum()), mask.size))
    # ---- backward through the float64 graph with that mask
    yt = pre * _nchw(mask.astype(np.float64), n, Ho, Wo)
    yt.backward(_nchw(c['gout'], n, Ho, Wo))
    bw = R.backward(c['gout'], z64, mask, mu, is_, c['gamma'])
    assert np.allclose(bw['dgamma'], gam_t.grad.numpy(), rtol=1e-9, atol=1e-12)          # bn_ref and autograd agree (float64)
    gx = bw['g'] * bw['xhat']
    b_g = B.b_sum_g(B.chunk_sums(np.abs(bw['g'])), B.chunk_sums(bw['g']), cout)
    b_gx = B.b_sum_gx(B.chunk_sums(np.abs(gx)), B.chunk_sums(gx), cout) + (np.abs(bw['g']) * b_xh).sum(0)
    B.check('conv64 dbeta', c['dbeta'], bet_t.grad.numpy(), B.b_accumulate(b_g, bw['sum_g'], 0.0), what)
    B.check('conv64 dgamma', c['dgamma'], gam_t.grad.numpy(), B.b_accumulate(b_gx, bw['sum_gx'], 0.0), what)
    k1 = np.abs(bw['sum_gx'] / M)
    inner = np.abs(bw['g'] - (bw['sum_g'] / M)[None, :] - bw['xhat'] * (bw['sum_gx'] / M)[None, :])
    b_dz = (B.b_dz(bw, B.b_coef(b_g, bw['sum_g'], M), B.b_coef(b_gx, bw['sum_gx'], M))
            + (gam * b_is)[None, :] * inner + np.abs(bw['gm'])[None, :] * b_xh * k1[None, :])
    dz_abs, b_dz_t = _nchw(np.abs(bw['dz']), n, Ho, Wo), _nchw(b_dz, n, Ho, Wo)
    wa, xa = c['w'].double().abs(), c['x'].double().abs()
    b_dx = (conv2d_input(xa.shape, wa, b_dz_t, stride=stride, padding=pad)
            + B.SAFETY * k * k * cout * B.U * conv2d_input(xa.shape, wa, dz_abs, stride=stride, padding=pad))
    b_dw = (conv2d_weight(xa, wa.shape, b_dz_t, stride=stride, padding=pad)
            + B.SAFETY * M * B.U * conv2d_weight(xa, wa.shape, dz_abs, stride=stride, padding=pad))
    B.check('conv64 dx', c['dx'], _rows_of(x64.grad), _rows_of(b_dx), what)
    B.check('conv64 dw', c['dw'].reshape(w64.shape), w64.grad.numpy(), b_dw.numpy(), what)
