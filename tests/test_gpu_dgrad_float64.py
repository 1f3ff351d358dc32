"""The convolution backward of train_engine.conv_param_and_input_grads -- the five data-gradient routes, each fresh and
accumulating, the weight gradient, the weight re-layouts, grl_dilate2 and the fused BatchNorm-backward epilogue of the
data-gradient GEMM -- against the float64 restatement of tests/dgrad_ref.py, on a real MI355X.

Every comparison is per element against that element's derived bound (tests/dgrad_bounds.py), never a norm over the tensor;
where the bound is exactly zero (pixels no tap reaches, everything outside a tagged pixel's footprint) the value must be
exactly zero, or bit-equal to the preloaded gradient in the accumulate forms.  The engine function is driven directly: a
fresh Tape, an nn.Conv2d on the device, a dz of the test's own; TE._in_backward is set, as Tape.backward sets it, so that
the GEMMs are the ones the backward runs (one chain past 256 rows).  TE._call and TE.gemm are spied on: the launch
sequence of every sweep entry, in both forms, is the one dgrad_bounds.launches names (one test; the others compare values).

Weight gradients: grl_conv_wgrad_f32 takes a conv-mode product only with cin % 64 == 0 (asserted below); the sweep entries
with cin = 32 or 96 run their data gradient with the weight gradient left to a weight-gradient stack that is not full
(dgrad_bounds.wgrad_accepts).

bf16 storage: the route sweep again with tp.b16 and bf16 dz, x, G0, on the entries with cout % 64 == 0 -- the bf16-storage
GEMM wants K % 64 == 0 and, conv mode, C % 64 == 0 (validate(), gemm_f32.hip), and route D's class (0, 0) has K = C = cout.
Skipped for that reason: every entry with cout = 32, 96 or 160 -- A (32, 32), (64, 96); B (64, 96) twice; C (96, 32) twice;
D (32, 32), (64, 32), (32, 96), (32, 32), (32, 160); E (32, 32) three times.  Every route keeps at least one entry.  The fused
bf16 form needs M % 128 == 0: at the fused test's shapes the wrapper rejects it, which is asserted.

Measured on the MI355X: 119 cases, 2 to 3 s for the whole module, every case under 0.1 s after the first."""
import functools
import time

import numpy as np
import pytest
import torch

import bn_bounds as BB
import bn_ref as BR
import dgrad_bounds as B
import dgrad_ref as R

pytestmark = pytest.mark.gpu

SENT = 12288.0                  # (exact in bf16)
GUARD = 64                      # sentinel elements behind every output
BF16 = torch.bfloat16
T0 = [None]


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    T0[0] = time.time()
    yield
    B.dump_ratios('MI355X convolution backward')
    print('  module run time %.1f s' % (time.time() - T0[0]))


def _te():
    from grl_amd import train_engine as TE
    return TE


def _err():
    from grl_amd._lib import GrlHipError
    return GrlHipError


def _call(name, *args):
    TE = _te()
    TE._call(name, *[TE.ptr(a) if torch.is_tensor(a) else a for a in args])


def _d(a, b16=False):
    t = torch.from_numpy(np.array(a, dtype=np.float32)).cuda()          # (a copy: the cached references are read-only)
    return t.to(BF16) if b16 else t


def _n(t):
    return t.detach().float().cpu().numpy()


def _out(n, init=None, b16=False):
    """n output elements (the sentinel, or `init`) with GUARD sentinel elements behind them"""
    t = torch.full((n + GUARD,), SENT, device='cuda', dtype=BF16 if b16 else torch.float32)
    if init is not None:
        t[:n] = _d(init, b16).reshape(-1)
    return t


def _got(t, n):
    """the n output elements on the host; nothing behind them was written"""
    torch.cuda.synchronize()
    a = _n(t)
    assert (a[n:] == SENT).all(), 'written past the end of the output'
    return a[:n]


def _poison(value, shapes, dtype):
    """fill and free blocks of the sizes the next call allocates: what it does not write shows"""
    blocks = [torch.full(s, value, device='cuda', dtype=dtype) for s in shapes for _ in range(4)]
    torch.cuda.synchronize()
    del blocks


class _StackNotFull(object):
    """conv_param_and_input_grads' `wstack`: a weight-gradient stack with blocks still to come issues no weight gradient"""

    def filled(self):
        return False


# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref(case, cls, b16=False):
    """inputs (rounded to bf16 for the bf16-storage sweep) and the float64 reference, computed once and read-only"""
    cin, cout, k, stride, H, W, n = case
    Ho, Wo, pad = B.geometry(case)
    d = B.make_inputs(case, cls)
    if b16:
        d = {key: B.to_bf16(v) for key, v in d.items()}
    dx, ab = R.dgrad(d['dz'], d['w'], n, H, W, Ho, Wo, k, stride, pad)
    dw, abw = R.wgrad(d['dz'], d['x'], n, H, W, Ho, Wo, k, stride, pad)
    for a in list(d.values()) + [dx, ab, dw, abw]:
        a.setflags(write=False)
    return d, dx, ab, dw, abw


def _conv(case, w):
    import torch.nn as nn
    cin, cout, k, stride, H, W, n = case
    conv = nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(np.array(w)))
    return conv.to('cuda')


def _run_route(case, cls, accumulate, b16=False, poison=None, wgrad=None):
    """one call of conv_param_and_input_grads; returns dict(dx, dw, seq): dx and dw on the host, the spied launch sequence"""
    TE = _te()
    assert TE.get_math() == 'f32'
    cin, cout, k, stride, H, W, n = case
    Ho, Wo, pad = B.geometry(case)
    Min, M = n * H * W, n * Ho * Wo
    d = _ref(case, cls, b16)[0]
    conv = _conv(case, d['w'])
    dz, x = _d(d['dz'], b16), _d(d['x'], b16)
    geom = None if (k == 1 and stride == 1) else (H, W, cin, Ho, Wo, k, k, stride, pad)
    tp = TE.Tape(torch.device('cuda:0'))
    tp.b16 = b16
    buf = None
    if accumulate:
        buf = _out(Min * cin, d['g0'], b16)
        tp.g[id(x)] = buf[:Min * cin].view(Min, cin)
    wgrad = B.wgrad_accepts(case) if wgrad is None else wgrad
    seq = []
    real_call, real_gemm = TE._call, TE.gemm

    def spy_call(name, *args):
        base = name[:-5] if name.endswith('_bf16') else name
        if base == 'grl_dilate2':
            seq.append((base,) + tuple(int(a) for a in args[8:11]))
        elif base != 'grl_cast':
            seq.append((base,))
        return real_call(name, *args)

    def spy_gemm(a, w, *args, **kw):
        seq.append(('gemm', kw.get('conv') is not None, kw.get('res') is not None, bool(kw.get('stats'))))
        return real_gemm(a, w, *args, **kw)

    if poison is not None:
        _poison(poison, [(Min, cin), (M, cin), (Min, cout)], dz.dtype)
    was = TE._in_backward[0]
    TE._call, TE.gemm, TE._in_backward[0] = spy_call, spy_gemm, True
    try:
        TE.conv_param_and_input_grads(tp, dz, x, conv, n, H, W, Ho, Wo, cin, cout, k, stride, geom,
                                      wstack=None if wgrad else (_StackNotFull(), 0))
    finally:
        TE._call, TE.gemm, TE._in_backward[0] = real_call, real_gemm, was
    tp.wgrad_join()
    dx = tp.take(x)
    assert dx is not None and tuple(dx.shape) == (Min, cin) and dx.dtype == dz.dtype
    if accumulate:
        assert dx.data_ptr() == buf.data_ptr(), 'the accumulate form must add into the preloaded gradient'
        got = _got(buf, Min * cin).reshape(Min, cin)
    else:
        torch.cuda.synchronize()
        got = _n(dx)
    dw = _n(tp.pgrad(conv.weight)) if wgrad else None
    assert np.array_equal(_n(dz), d['dz']) and np.array_equal(_n(x), d['x']), 'an input was written'
    assert np.array_equal(_n(conv.weight), d['w']), 'the weight was written'
    return dict(dx=got, dw=dw, seq=seq)


def _check_route(stage, case, cls, accumulate, out, b16=False):
    d, dx, ab, dw, abw = _ref(case, cls, b16)
    want = dx + d['g0'].astype(np.float64) if accumulate else dx
    what = (case, cls, 'accumulate' if accumulate else 'fresh')
    if b16:
        bound = B.b_dx_bf16(case, ab, want, dx, accumulate)
    else:
        bound = B.b_dx(case, ab, want, accumulate)
    B.check(stage + ' dx', out['dx'], want, bound, what)
    exact = bound == 0                      # no term arrives: exactly zero, or G0 bit for bit
    assert np.array_equal(out['dx'][exact], want[exact].astype(np.float32))
    if out['dw'] is not None:
        M = case[6] * B.geometry(case)[0] * B.geometry(case)[1]
        B.check(stage + ' dw', out['dw'], dw, B.b_dw(M, abw, dw), what)
        assert (out['dw'][abw == 0] == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('case', B.CASES)
def test_routes_against_float64(case, cls):
    """dx and dW of every sweep entry, fresh and accumulating.  The fresh form runs twice, after blocks of the sizes it
    allocates were filled with 1e30 and then with NaN and freed: the two results are bit-equal and finite -- every element
    of dx was written (route D's mode 2 writes class by class into an uninitialised buffer)."""
    r = B.route(case[2], case[3], case[4], case[5])
    a = _run_route(case, cls, 0, poison=1e30)
    _check_route('route ' + r, case, cls, 0, a)
    b = _run_route(case, cls, 0, poison=float('nan'))
    assert np.isfinite(b['dx']).all() and np.array_equal(a['dx'].view(np.uint32), b['dx'].view(np.uint32)), \
        'the fresh data gradient depends on what the allocator handed out'
    _check_route('route ' + r + ' accumulate', case, cls, 1, _run_route(case, cls, 1))


def test_tagged_footprint_on_the_device():
    """class (t): the nonzeros of the device's dx are exactly the reference's -- one per tap of the tagged pixel"""
    for i, case in enumerate(B.CASES):
        out = _run_route(case, 't', 0)
        _, dx, _, _, _ = _ref(case, 't')
        assert np.array_equal(out['dx'] != 0, dx != 0), case
        assert int((out['dx'] != 0).any(1).sum()) == B.tagged_footprint(case, i)


def test_every_route_runs_twice_and_in_both_forms():
    """... confirmed on the launches themselves: the spied sequence of every sweep entry, in both forms, is the one
    dgrad_bounds.launches restates from the table of routes (the other tests compare values only)"""
    seen = {}
    for case in B.CASES:
        r = B.route(case[2], case[3], case[4], case[5])
        for acc in (0, 1):
            out = _run_route(case, 'a', acc)
            assert out['seq'] == B.launches(case, acc), (case, acc, out['seq'])
            seen[(r, acc)] = seen.get((r, acc), 0) + 1
            names = [s[0] for s in out['seq']]
            assert names.count('gemm') == (4 if r == 'D' else 1)
            assert names.count('grl_dilate2') == {'A': 0, 'B': 1, 'C': 0, 'D': 4, 'E': 1}[r]
    assert all(seen.get((r, acc), 0) >= 2 for r in 'ABCDE' for acc in (0, 1)), seen


@pytest.mark.parametrize('case', [c for c in B.CASES if B.route(c[2], c[3], c[4], c[5]) == 'A'])
def test_route_A_on_the_first_columns_of_a_wider_weight(case):
    """`kcols` (the GCE split weight): the layer uses the first cin columns of a [cout][2 cin] weight -- the transposed copy
    must be taken with the wide row stride (Tape.w_t's ld), and dW lands in those columns only"""
    import torch.nn as nn
    TE = _te()
    cin, cout, k, stride, H, W, n = case
    Min = n * H * W
    d, dx, ab, dw, abw = _ref(case, 'a')
    other = B.f32(B.rng_for('wide', *case).standard_normal((cout, cin)))
    wide = np.concatenate([d['w'].reshape(cout, cin), other], 1)
    for acc in (0, 1):
        conv = nn.Conv2d(2 * cin, cout, 1, bias=False)
        with torch.no_grad():
            conv.weight.copy_(torch.from_numpy(wide.reshape(cout, 2 * cin, 1, 1)))
        conv.to('cuda')
        dz, x = _d(d['dz']), _d(d['x'])
        tp = TE.Tape(torch.device('cuda:0'))
        buf = _out(Min * cin, d['g0'] if acc else None)
        if acc:
            tp.g[id(x)] = buf[:Min * cin].view(Min, cin)
        was, TE._in_backward[0] = TE._in_backward[0], True
        try:
            TE.conv_param_and_input_grads(tp, dz, x, conv, n, H, W, H, W, cin, cout, 1, 1, None, kcols=cin, ldw=2 * cin)
        finally:
            TE._in_backward[0] = was
        tp.wgrad_join()
        got = tp.take(x)
        assert (got.data_ptr() == buf.data_ptr()) == bool(acc)
        torch.cuda.synchronize()
        want = dx + d['g0'].astype(np.float64) if acc else dx
        B.check('route A kcols dx', _got(buf, Min * cin).reshape(Min, cin) if acc else _n(got), want,
                B.b_dx(case, ab, want, acc), (case, acc))
        gw = _n(tp.pgrad(conv.weight)).reshape(cout, 2 * cin)
        B.check('route A kcols dw', gw[:, :cin], dw.reshape(cout, cin), B.b_dw(Min, abw.reshape(cout, cin), dw.reshape(cout, cin)),
                (case, acc))
        assert (gw[:, cin:] == 0).all() and np.array_equal(_n(conv.weight).reshape(cout, 2 * cin), wide)


@pytest.mark.parametrize('case', B.FORCED_TILE_CASES)
def test_routes_on_the_128_row_conv_gather(case):
    """the conv-mode routes once more with the GEMM forced onto the 128 x 64 tile (grl_gemm_force_tile): the LDS-DMA gather
    with its per-row tap mask, which the tile rule only picks from ~57 000 rows on"""
    lib = _te()._lib.load()
    r = B.route(case[2], case[3], case[4], case[5])
    lib.grl_gemm_force_tile(128, 64)
    try:
        for cls in ('a', 't'):
            for acc in (0, 1):
                _check_route('route %s 128-row tile' % r, case, cls, acc, _run_route(case, cls, acc))
    finally:
        lib.grl_gemm_force_tile(0, 0)


@pytest.mark.parametrize('case', [c for c in B.CASES if B.bf16_accepts(c)])
def test_routes_bf16_storage(case):
    r = B.route(case[2], case[3], case[4], case[5])
    for cls in ('a', 't'):
        for acc in (0, 1):
            out = _run_route(case, cls, acc, b16=True, poison=None if acc else float('nan'))
            _check_route('bf16 route ' + r + (' accumulate' if acc else ''), case, cls, acc, out, b16=True)


def test_the_bf16_subset_keeps_every_route():
    kept = {B.route(c[2], c[3], c[4], c[5]) for c in B.CASES if B.bf16_accepts(c)}
    assert kept == set('ABCDE')
    assert sorted(c[1] for c in B.CASES if not B.bf16_accepts(c)) == sorted([32, 96, 96, 96, 32, 32, 32, 32, 96, 32, 160, 32, 32, 32])


# ----------------------------------------------------------------------------------------------------------------------
# packed weights
def test_packed_weights_equal_the_index_formulas():
    TE = _te()
    dev = torch.device('cuda:0')
    for case in (B.CASES[6], B.CASES[10], B.CASES[14], B.CASES[3]):
        cin, cout, k = case[0], case[1], case[2]
        w = _ref(case, 'a')[0]['w']
        conv = _conv(case, w)
        tp = TE.Tape(dev)
        if k == 3:
            assert np.array_equal(_n(tp.w_dgrad(conv)), R.pack_dgrad(w))
            for py in (0, 1):
                for px in (0, 1):
                    got = tp.w_dgrad_s2(conv, py, px)
                    assert got.is_contiguous() and np.array_equal(_n(got), R.w_dgrad_s2(w, py, px))
        else:
            w2d = conv.weight.detach().view(cout, -1)
            assert np.array_equal(_n(tp.w_t(w2d, conv.weight, ld=w2d.shape[1])), R.transpose(w, cout, cin, cin))
            half = tp.w_t(w2d[:, :cin // 2], conv, ld=w2d.shape[1])          # the first columns of a wider weight (GCE split)
            assert np.array_equal(_n(half), R.transpose(w, cout, cin // 2, cin))
        tp16 = TE.Tape(dev)
        tp16.b16 = True
        if k == 3:
            assert np.array_equal(_n(tp16.w_dgrad(conv)), B.bf16_round(R.pack_dgrad(w)).astype(np.float32))


@pytest.mark.parametrize('Rr', (31, 32, 33, 65))
def test_transpose(Rr):
    rng = B.rng_for('transpose', Rr)
    for Cc in (31, 32, 33, 65):
        for ld in (Cc, Cc + 3):
            x = B.f32(rng.standard_normal(Rr * ld))
            y = _out(Rr * Cc)
            _call('grl_transpose', _d(x), y, Rr, Cc, ld)
            assert np.array_equal(_got(y, Rr * Cc).reshape(Cc, Rr), R.transpose(x, Rr, Cc, ld)), (Rr, Cc, ld)


# ----------------------------------------------------------------------------------------------------------------------
# grl_dilate2 alone
@pytest.mark.parametrize('Cc', (4, 36, 64))
@pytest.mark.parametrize('dH,dW', [(0, 0), (-1, 0), (0, -1), (-1, -1), (1, 0)])
def test_dilate2(dH, dW, Cc):
    """all three modes, all four offset pairs; H in {2 Ho, 2 Ho - 1} and W likewise, and H = 2 Ho + 1, where the
    `(y >> 1) < Ho` guard decides.  Exact; modes 1 and 2 leave every non-class element bit-equal to what it was."""
    n, Ho, Wo = 2, 3, 2
    H, W = 2 * Ho + dH, 2 * Wo + dW
    rng = B.rng_for('dilate2', H, W, Cc)
    dz = B.f32(rng.standard_normal((n * Ho * Wo, Cc)))
    up0 = B.f32(rng.standard_normal((n * H * W, Cc)))
    dz_t = _d(dz)
    for mode in (0, 1, 2):
        for oy in (0, 1):
            for ox in (0, 1):
                up = _out(n * H * W * Cc, None if mode == 0 else up0)
                _call('grl_dilate2', dz_t, up, n, Ho, Wo, H, W, Cc, mode, oy, ox)
                got = _got(up, n * H * W * Cc).reshape(-1, Cc)
                want = R.dilate2(dz, up0, n, Ho, Wo, H, W, Cc, mode, oy, ox)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (H, W, Cc, mode, oy, ox)
                if mode:
                    keep = ~R.dilate2_hit(n, Ho, Wo, H, W, oy, ox)
                    assert np.array_equal(got[keep].view(np.uint32), up0[keep].view(np.uint32))
    assert np.array_equal(_n(dz_t), dz)


def test_dilate2_past_one_pass_of_the_capped_grid():
    """grid_even caps the launch at 8192 workgroups of 256 float4 lanes: 3 x 166 x 264 x 64 floats are 2 103 552 float4 items,
    6 400 more than one pass covers -- the `i += gridDim.x * blockDim.x` trip runs"""
    n, Ho, Wo, Cc = 3, 83, 132, 64
    H, W = 2 * Ho, 2 * Wo
    assert B.GRID_CAP < n * H * W * Cc // 4 < 2 * B.GRID_CAP
    rng = B.rng_for('dilate2 big')
    dz = B.f32(rng.standard_normal((n * Ho * Wo, Cc)))
    up0 = B.f32(rng.standard_normal((n * H * W, Cc)))
    dz_t = _d(dz)
    for mode, oy, ox in ((0, 0, 0), (1, 1, 0), (2, 0, 1)):
        up = _out(n * H * W * Cc, None if mode == 0 else up0)
        _call('grl_dilate2', dz_t, up, n, Ho, Wo, H, W, Cc, mode, oy, ox)
        want = R.dilate2(dz, up0, n, Ho, Wo, H, W, Cc, mode, oy, ox)
        assert np.array_equal(_got(up, n * H * W * Cc).reshape(-1, Cc), want), (mode, oy, ox)


# ----------------------------------------------------------------------------------------------------------------------
# the fused BatchNorm-backward epilogue
FUSED_MAPS = {45: (5, 3, 3), 130: (13, 5, 2), 273: (13, 7, 3)}           # Min -> (H, W, n)
EPS = 1e-5


def _fused_inputs(route, Min, cin):
    """dz, w, res (the gradient already there), and the BatchNorm side: z, statistics vectors, gamma, beta, the forward's
    residual; no pre-activation -- (z - mean) scale + beta for the mask from z, that plus the residual for the mask from
    bits -- within 1e-3 of zero, far outside its rounding bound (asserted by the caller on the reference)"""
    H, W, n = FUSED_MAPS[Min]
    cout, k = (96, 1) if route == 'A' else (64, 3)
    rng = B.rng_for('fused', route, Min, cin)
    dz = B.f32(rng.standard_normal((Min, cout)))
    w = B.f32(rng.standard_normal((cout, cin, k, k)) / np.sqrt(k * k * cin))
    res = B.f32(rng.standard_normal((Min, cin)))
    z = B.f32(rng.uniform(0.5, 2.0, cin)[None, :] * (rng.standard_normal((Min, cin)) + rng.uniform(-1.0, 1.0, cin)[None, :]))
    mean = B.f32(z.astype(np.float64).mean(0))
    invstd = B.f32(1.0 / np.sqrt(z.astype(np.float64).var(0) + EPS))
    gamma = B.f32(rng.uniform(0.5, 1.5, cin))
    beta = B.f32(rng.uniform(-0.7, 0.7, cin))
    scale = B.f32(gamma.astype(np.float64) * invstd)
    fres = B.f32(rng.standard_normal((Min, cin)))
    # ... except every 7th row of channel 0: z == mean and beta == 0 there, the pre-activation is EXACTLY zero in fp32 as in
    # float64 (no rounding: its bound is zero too), and `> 0` masks it -- the one input that tells `>` from `>=`
    beta[0] = 0.0
    pin = np.zeros((Min, cin), bool)
    pin[::7, 0] = True
    z[pin] = mean[0]
    for _ in range(8):
        pre = (z.astype(np.float64) - mean) * scale + beta
        bad = ((np.abs(pre) < 1e-3) & ~pin) | (np.abs(pre + fres) < 1e-3)
        if not bad.any():
            break
        fres = np.where(bad & pin, B.f32(fres + 0.01), fres)
        z = np.where(bad & ~pin, B.f32(z + 0.01 / scale[None, :]), z)
    return dict(H=H, W=W, n=n, cout=cout, k=k, dz=dz, w=w, res=res, z=z, mean=mean, invstd=invstd, gamma=gamma, beta=beta,
                scale=scale, fres=fres)


@pytest.mark.parametrize('cin', (32, 64, 96))
@pytest.mark.parametrize('Min', (45, 130, 273))
@pytest.mark.parametrize('route', ('A', 'C'))
def test_fused_epilogue(route, Min, cin):
    """TE.gemm(..., stats=True, bn=...) as routes A and C issue it: the masked g per element, the slab summed over its rows
    per channel, then grl_bn_bwd_finish on that very slab against bn_ref.backward.  Mask from z and mask from bits (the bits
    grl_bn_apply_centered records), with and without a gradient already there (res)."""
    TE = _te()
    f = _fused_inputs(route, Min, cin)
    H, W, n, cout, k = f['H'], f['W'], f['n'], f['cout'], f['k']
    case = (cin, cout, k, 1, H, W, n)
    conv = _conv(case, f['w'])
    tp = TE.Tape(torch.device('cuda:0'))
    if route == 'A':
        w2d = conv.weight.detach().view(cout, -1)
        wd, K, geom = tp.w_t(w2d, conv.weight, ld=w2d.shape[1]), cout, None
    else:
        wd, K, geom = tp.w_dgrad(conv), 9 * cout, (H, W, cout, H, W, 3, 3, 1, 1)
    acc, ab = R.dgrad(f['dz'], f['w'], n, H, W, H, W, k, 1, k // 2)
    dz_t, z_t = _d(f['dz']), _d(f['z'])
    vec = {key: _d(f[key]) for key in ('mean', 'invstd', 'scale', 'beta', 'gamma')}
    # the forward's bits, as the engine records them: y = relu((z - mean) scale + beta + fres)
    y = torch.empty(Min, cin, device='cuda')
    bits_t = torch.full((Min * cin // 4 + 4,), 0xAB, dtype=torch.uint8, device='cuda')
    _call('grl_bn_apply_centered', z_t, vec['mean'], vec['scale'], vec['beta'], _d(f['fres']), y, Min, cin, 1, bits_t)
    torch.cuda.synchronize()
    fw = BR.apply_centered(f['z'], f['mean'], f['scale'], f['beta'], f['fres'], True)
    assert (np.abs(fw['pre']) > BB.b_apply(fw['abs_terms'])).all()          # no pre-activation within its bound of zero
    bits_ref = fw['pre'] > 0
    assert np.array_equal(R.unpack_bits(bits_t.cpu().numpy(), Min * cin), bits_ref.reshape(-1))
    assert (bits_t.cpu().numpy()[Min * cin // 4:] == 0xAB).all()
    margin = B.b_mask_margin(f['z'], f['mean'], f['scale'], f['beta'])
    was = TE._in_backward[0]
    TE._in_backward[0] = True
    try:
        for form in ('z', 'bits'):
            for has_res in (False, True):
                what = (route, Min, cin, form, has_res)
                dx = _out(Min * cin, f['res'] if has_res else None)
                cur = dx[:Min * cin].view(Min, cin)
                bn = (z_t, vec['mean'], vec['invstd'], vec['scale'] if form == 'z' else None,
                      vec['beta'] if form == 'z' else None, bits_t if form == 'bits' else None)
                _, slab = TE.gemm(dz_t, wd, cur, Min, cin, K, conv=geom, res=cur if has_res else None, stats=True, bn=bn)
                rows = slab.shape[0]
                assert rows in ((Min + 63) // 64, (Min + 127) // 128) and tuple(slab.shape) == (rows, 2, cin)
                g = _got(dx, Min * cin).reshape(Min, cin)
                ep = R.fused_epilogue(acc, f['res'] if has_res else None, f['z'], f['mean'], f['invstd'],
                                      f['scale'] if form == 'z' else None, f['beta'] if form == 'z' else None,
                                      bits_ref if form == 'bits' else None)
                if form == 'z':                     # every pre-activation is outside its rounding bound of zero, or exactly zero with
                    # a zero bound (z == mean, beta == 0: nothing rounds) -- so the mask is the reference's, exactly
                    assert ((np.abs(ep['pre']) > margin) | ((margin == 0) & (ep['pre'] == 0))).all()
                    assert ((ep['pre'] == 0).sum() == (Min + 6) // 7) and not ep['mask'][ep['pre'] == 0].any()
                bd = B.fused_bounds(ep, K, ab, has_res)
                B.check('fused g', g, ep['g'], bd['g'], what)
                assert (g[~ep['mask']] == 0).all() and 0 < ep['mask'].sum() < ep['mask'].size
                s = _n(slab).astype(np.float64).sum(0)
                B.check('fused sum g', s[0], ep['sum_g'], bd['sum_g'], what)
                B.check('fused sum g xhat', s[1], ep['sum_gx'], bd['sum_gx'], what)
                # finalize + apply on that slab (the engine's conv_bn.bwd): dz, dgamma, dbeta against bn_ref.backward
                dzb = torch.full((Min, cin), SENT, device='cuda')
                dg, db = torch.zeros(cin, device='cuda'), torch.zeros(cin, device='cuda')
                _call('grl_bn_bwd_finish', cur, z_t, vec['mean'], vec['invstd'], vec['gamma'], dzb, dg, db, slab, rows,
                      torch.empty(2, cin, device='cuda'), Min, cin, None, 0)
                torch.cuda.synchronize()
                bw = BR.backward(ep['v'], f['z'], ep['mask'], f['mean'], f['invstd'], f['gamma'])
                B.check('fused finish dbeta', _n(db), bw['dbeta'], BB.b_accumulate(bd['sum_g'], bw['sum_g'], 0.0), what)
                B.check('fused finish dgamma', _n(dg), bw['dgamma'], BB.b_accumulate(bd['sum_gx'], bw['sum_gx'], 0.0), what)
                b_dz = (BB.b_dz(bw, BB.b_coef(bd['sum_g'], bw['sum_g'], Min), BB.b_coef(bd['sum_gx'], bw['sum_gx'], Min))
                        + np.abs(bw['gm'])[None, :] * bd['g'])
                B.check('fused finish dz', _n(dzb), bw['dz'], b_dz, what)
    finally:
        TE._in_backward[0] = was
    assert np.array_equal(_n(dz_t), f['dz']) and np.array_equal(_n(z_t), f['z'])


def test_fused_bf16_form_is_rejected_off_the_128_row_grid():
    """bf16 storage carries the reduce only in the interior epilogue of the 128-row tiles: M % 128 != 0 is an error, not a
    different kernel"""
    TE = _te()
    Min, cin, K = 45, 64, 64
    a = torch.zeros(Min, K, device='cuda', dtype=BF16)
    w = torch.zeros(cin, K, device='cuda', dtype=BF16)
    y = torch.zeros(Min, cin, device='cuda', dtype=BF16)
    z = torch.zeros(Min, cin, device='cuda', dtype=BF16)
    v = torch.ones(cin, device='cuda')
    with pytest.raises(_err()):
        TE.gemm(a, w, y, Min, cin, K, stats=True, bn=(z, v, v, v, v, None))
    torch.cuda.synchronize()
    assert (y == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
def test_rejections_before_any_launch():
    TE = _te()
    a = torch.zeros(4 * 4 * 16, device='cuda')
    w = torch.zeros(32 * 32, device='cuda')
    y = _out(16 * 32)
    with pytest.raises(_err()):              # conv-mode GEMM: C = 16 is no multiple of 32 (K = 1 x 2 x 16 is)
        TE.gemm(a, w, y, 16, 32, 32, conv=(4, 4, 16, 4, 4, 1, 2, 1, 0))
    up = _out(2 * 4 * 4 * 8)
    dz = torch.zeros(2 * 2 * 2 * 8, device='cuda')
    for oy, ox in ((2, 0), (0, 2), (-1, 0), (0, -1)):
        with pytest.raises(_err()):
            _call('grl_dilate2', dz, up, 2, 2, 2, 4, 4, 8, 0, oy, ox)
    with pytest.raises(_err()):              # C % 4
        _call('grl_dilate2', dz, up, 2, 2, 2, 4, 4, 6, 0, 0, 0)
    _got(y, 16 * 32), _got(up, 2 * 4 * 4 * 8)
    # a conv-mode weight gradient with cin % 64 != 0 (why those sweep entries run without one)
    case = next(c for c in B.CASES if not B.wgrad_accepts(c))
    with pytest.raises(_err()):
        _run_route(case, 'a', 0, wgrad=True)
