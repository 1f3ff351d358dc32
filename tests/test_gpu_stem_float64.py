"""The stem and max-pool kernels (pointwise.hip, pointwise_bf16.hip, train.hip, train_bf16.hip) against the float64
restatement of tests/stem_ref.py, through the C ABI, on a real MI355X.

Every comparison is per element against that element's derived bound (tests/stem_bounds.py) -- never a norm over the map:
one wrong border pixel fails.  Copies (max-pool forward, im2col) and the fused BatchNorm + ReLU + max-pool (against its
fp32 restatement, positions included) are compared bit for bit; so are the kernels documented bit-identical (the fused bf16
stem + pool against stem + grl_maxpool3x3s2_bf16, the packed weight image against the in-kernel conversion).

Every output lives in a buffer filled with a sentinel and GUARD sentinel elements longer than the kernel may write; a
rejected call must leave the whole buffer as it was."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import stem_bounds as B
import stem_ref as R

pytestmark = pytest.mark.gpu

SENT = 12345.0
IDX_SENT = 0xA5
GUARD = 64                      # sentinel elements behind every output
BF = torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    yield
    B.dump_ratios('MI355X stem and max-pool kernels')


def _L():
    from grl_amd import _lib
    return _lib


def _call(name, *args):
    """through the C ABI; GrlHipError (with the library's message) if the launcher refuses"""
    lib = _L()
    fn = getattr(lib.load(), name)
    lib.check(fn(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], lib.stream()), name)


def _rc(name, *args):
    lib = _L()
    return getattr(lib.load(), name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], lib.stream())


def _d(a, dt=None):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint8:
        return torch.from_numpy(a).cuda()
    t = torch.from_numpy(a.astype(np.float32)).cuda()
    return t.to(dt) if dt is not None else t


def _out(n, dt=torch.float32):
    """n output elements of the sentinel with GUARD more behind them"""
    if dt == torch.uint8:
        return torch.full((n + GUARD,), IDX_SENT, dtype=dt, device='cuda')
    return torch.full((n + GUARD,), SENT, dtype=dt, device='cuda')


def _got(t, n):
    """the n output elements on the host (fp32 / bf16 as float32, positions as uint8); nothing behind them was written"""
    torch.cuda.synchronize()
    if t.dtype == torch.uint8:
        a = t.cpu().numpy()
        assert (a[n:] == IDX_SENT).all(), 'written past the end of the output'
        return a[:n]
    a = t.float().cpu().numpy()
    assert (a[n:] == float(torch.tensor(SENT, dtype=t.dtype).float())).all(), 'written past the end of the output'
    return a[:n]


class _Inputs(object):
    """device copies of a case's inputs; `unchanged()` after the launches: no kernel wrote to one"""

    def __init__(self, dt=None, **arrays):
        self.t = {k: _d(v, None if (np.asarray(v).dtype == np.uint8 or k in dt_f32) else dt) for k, v in arrays.items()}
        torch.cuda.synchronize()
        self.h = {k: v.clone() for k, v in self.t.items()}

    def __getitem__(self, k):
        return self.t[k]

    def unchanged(self):
        torch.cuda.synchronize()
        for k, v in self.h.items():
            assert torch.equal(self.t[k], v), 'input %s was written' % k


dt_f32 = ('mean', 'scale', 'beta', 'shift', 'w', 'ms', 'x32')      # per-channel vectors and fp32 images stay fp32 in the bf16 pipeline


def _pack(w, kind):
    """the packed weight images: 'f32' [64][164] floats, 'pool' [64][2][84] floats, 'bf16' [64][184] bf16"""
    if kind == 'bf16':
        wp = torch.zeros(64 * 184, dtype=BF, device='cuda')
        _call('grl_stem_pack_weight_bf16', w, wp)
    elif kind == 'pool':
        wp = torch.zeros(64 * 168, device='cuda')
        _call('grl_stem_pack_weight_pool', w, wp)
    else:
        wp = torch.zeros(64 * 164, device='cuda')
        _call('grl_stem_pack_weight', w, wp)
    return wp


def _stem_call(t, y, n, H, W, relu, wp, u8, b16):
    name = 'grl_stem_conv7x7' + ('_u8' if u8 else '') + ('_bf16' if b16 else '')
    if u8:
        _call(name, t['x'], t['ms'], t['w'], t['scale'], t['shift'], y, n, H, W, relu, wp)
    else:
        _call(name, t['x'], t['w'], t['scale'], t['shift'], y, n, H, W, relu, wp)


def _stem_inputs(d):
    return _Inputs(x=d['x'], w=d['w'], scale=d['scale'], shift=d['shift'], ms=B.MEAN_STD)


def _relu(ref, relu):
    return np.maximum(ref, 0.0) if relu else ref


# ----------------------------------------------------------------------------------------------------------------------
# the two-launch stems
@pytest.mark.parametrize('b16', (False, True))
@pytest.mark.parametrize('u8', (False, True))
@pytest.mark.parametrize('cls', ('a', 'm'))
@pytest.mark.parametrize('n,H,W', B.STEM_SHAPES)
def test_two_launch_stem(n, H, W, cls, u8, b16):
    """grl_stem_conv7x7(_u8)(_bf16): stem_mfma_kernel / stem_b16_kernel with short tiles in x, in y and in both, Ho or Wo of
    1, relu 0 and 1, with and without the packed weight image (bit-identical), scales of both signs"""
    d = B.stem_case(n, H, W, cls, u8, b16)
    t = _stem_inputs(d)
    wp = _pack(t['w'], 'bf16' if b16 else 'f32')
    m = n * (H // 2) * (W // 2) * 64
    what = (n, H, W, cls, u8, b16)
    for relu in (0, 1):
        ref = _relu(d['ref']['y'], relu)
        bound = (B.b_stem_bf16(d['ref'], d['scale'], d['shift'], ref) if b16 else
                 B.b_stem_f32(d['ref'], d['scale'], d['shift'], B.K_MFMA, 1))
        outs = []
        for packed in (0, 1):
            y = _out(m, BF if b16 else torch.float32)
            _stem_call(t, y, n, H, W, relu, wp if packed else None, u8, b16)
            outs.append(_got(y, m).reshape(-1, 64))
            B.check('stem %s%s' % ('bf16' if b16 else 'fp32', ' u8' if u8 else ''), outs[-1], ref, bound, what + (relu, packed))
        assert np.array_equal(outs[0], outs[1]), 'the packed weight image and the in-kernel conversion differ'
    t.unchanged()


def _valu_child(path):
    """runs in a fresh process with GRL_STEM_VALU set (the launcher reads it once): the fp32 stem over the two-launch sweep"""
    assert os.environ.get('GRL_STEM_VALU')
    out = {}
    for n, H, W in B.STEM_SHAPES:
        for cls in ('a', 'm'):
            d = B.stem_case(n, H, W, cls, False, False)
            t = _stem_inputs(d)
            m = n * (H // 2) * (W // 2) * 64
            for relu in (0, 1):
                y = _out(m)
                _stem_call(t, y, n, H, W, relu, None, False, False)
                out['%d_%d_%d_%s_%d' % (n, H, W, cls, relu)] = _got(y, m)
            t.unchanged()
    np.savez(path, **out)


def test_valu_stem_in_a_child_process():
    """stem_conv7x7_kernel (GRL_STEM_VALU, read once per process): one fresh child runs the two-launch sweep and writes its
    outputs; they are checked here against the same reference at the VALU kernel's depth (147 fused multiply-adds)"""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'valu.npz')
        code = 'import sys; sys.path[:0] = [%r, %r]; import test_gpu_stem_float64 as T; T._valu_child(%r)' % (
            HERE, os.path.dirname(HERE), path)
        env = dict(os.environ, GRL_STEM_VALU='1')
        r = subprocess.run([sys.executable, '-c', code], env=env, timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode('utf-8', 'replace')[-4000:]
        got = dict(np.load(path))
    differs = False
    for n, H, W in B.STEM_SHAPES:
        for cls in ('a', 'm'):
            d = B.stem_case(n, H, W, cls, False, False)
            bound = B.b_stem_f32(d['ref'], d['scale'], d['shift'], B.K_VALU, 0)
            for relu in (0, 1):
                g = got['%d_%d_%d_%s_%d' % (n, H, W, cls, relu)].reshape(-1, 64)
                B.check('stem fp32 VALU', g, _relu(d['ref']['y'], relu), bound, (n, H, W, cls, relu))
            if (n, H, W) == B.STEM_SHAPES[-2] and cls == 'a':
                # the child did run the other kernel: another summation order, other bits somewhere in 38016 sums of 147 terms
                t = _stem_inputs(d)
                y = _out(g.size)
                _stem_call(t, y, n, H, W, 1, None, False, False)
                differs = not np.array_equal(_got(y, g.size).reshape(-1, 64), g)
    assert differs, 'GRL_STEM_VALU did not select stem_conv7x7_kernel in the child'


# ----------------------------------------------------------------------------------------------------------------------
# stem + max-pool in one launch
def _pool_params():
    out = []
    for i, (n, H) in enumerate(B.POOL_CASES):
        for u8 in (False, True):
            out.append((n, H, 'am'[(i + int(u8)) % 2], u8))
    return out


@pytest.mark.parametrize('b16', (False, True))
@pytest.mark.parametrize('n,H,cls,u8', _pool_params())
def test_stem_and_pool_in_one_launch(n, H, cls, u8, b16):
    """grl_stem_pool_f32 / grl_stem_pool_bf16 (both bf16 forms: whichever H selects) at W = 128: one strip and several, a
    short last strip, fewer workgroups than strips, the capped strip count, Hp of 1, 2 and 3.  The bound of a pooled element
    is the largest stem bound in its window.  bf16: also bit-identical to grl_stem_conv7x7(_u8)_bf16 +
    grl_maxpool3x3s2_bf16 (whose stem map is checked per element as well)."""
    W = B.POOL_W
    d = B.stem_case(n, H, W, cls, u8, b16, B.POOL_DISTINCT if n == B.POOL_N_CAP else 0)
    t = _stem_inputs(d)
    Ho, Wo, Hp, Wp = H // 2, W // 2, H // 4, W // 4
    reps = d['reps']
    nd = n // reps                                             # different frames: the reference is built for these
    ref = _relu(d['ref']['y'], 1)
    want = B.tile(R.maxpool(ref.reshape(nd, Ho, Wo, 64))[0].reshape(-1, 64), reps)
    m = n * Hp * Wp * 64
    what = (n, H, cls, u8, b16)
    ms = t['ms'] if u8 else None
    if not b16:
        bs = B.b_stem_f32(d['ref'], d['scale'], d['shift'], B.K_POOL_F32, 1)
        y = _out(m)
        _call('grl_stem_pool_f32', t['x'], int(u8), ms, t['scale'], t['shift'], y, n, H, W, _pack(t['w'], 'pool'))
        B.check('stem + pool fp32%s' % (' u8' if u8 else ''), _got(y, m).reshape(want.shape), want,
                B.tile(B.pool_bound(bs, nd, Ho, Wo).reshape(-1, 64), reps), what)
    else:
        bs = B.b_stem_bf16(d['ref'], d['scale'], d['shift'], ref)
        wp = _pack(t['w'], 'bf16')
        y = _out(m, BF)
        _call('grl_stem_pool_bf16', t['x'], int(u8), ms, t['scale'], t['shift'], y, n, H, W, wp)
        got = _got(y, m).reshape(want.shape)
        B.check('stem + pool bf16 form %d%s' % (B.pool_b16_form(H), ' u8' if u8 else ''), got, want,
                B.tile(B.pool_bound(bs, nd, Ho, Wo).reshape(-1, 64), reps), what)
        ms_, two = n * Ho * Wo * 64, _out(m, BF)
        stem = _out(ms_, BF)
        _stem_call(t, stem, n, H, W, 1, wp, u8, True)
        B.check('stem bf16 (W = 128)%s' % (' u8' if u8 else ''), _got(stem, ms_).reshape((reps,) + ref.shape), B.tile(ref, reps),
                B.tile(bs, reps), what)
        _call('grl_maxpool3x3s2_bf16', stem, two, n, Ho, Wo, 64)
        assert np.array_equal(_got(two, m).reshape(want.shape), got), 'one launch and two launches differ'
    t.unchanged()


# ----------------------------------------------------------------------------------------------------------------------
# the max-pool family
def _mp_run(a, dy, v, b16, what):
    """forward, backward from x, fused BatchNorm + ReLU + max-pool (with and without beta), backward from its positions"""
    n, H, W, C = a.shape
    Ho, Wo = R.pooled_size(H, W)
    dt = BF if b16 else torch.float32
    sfx = '_bf16' if b16 else ''
    t = _Inputs(dt, a=a, dy=dy, mean=v['mean'], scale=v['scale'], beta=v['beta'])
    mo, mi = n * Ho * Wo * C, n * H * W * C
    # forward: a copy, bit for bit
    y = _out(mo, dt)
    _call('grl_maxpool3x3s2' + sfx, t['a'], y, n, H, W, C)
    want, pos = R.maxpool(a)
    assert np.array_equal(_got(y, mo).reshape(want.shape), want), ('max-pool forward', what)
    # backward through the first maximum of x
    dx = _out(mi, dt)
    _call('grl_maxpool3x3s2_bwd' + sfx, t['a'], t['dy'], dx, n, H, W, C)
    rdx, S = R.maxpool_bwd(pos, dy, (H, W))
    B.check('maxpool_bwd' + sfx, _got(dx, mi).reshape(rdx.shape), rdx, B.b_pool_bwd(S, rdx if b16 else None), what)
    # fused BatchNorm + ReLU + max-pool against the fp32 restatement: values and positions bit for bit
    for beta in (t['beta'], None):
        _, y32, p32 = B.bn_relu_maxpool_f32(a, v['mean'], v['scale'], None if beta is None else v['beta'], b16)
        y, idx = _out(mo, dt), _out(mo, torch.uint8)
        _call('grl_bn_relu_maxpool3x3s2' + sfx, t['a'], t['mean'], t['scale'], beta, y, idx, n, H, W, C)
        assert np.array_equal(_got(y, mo).reshape(y32.shape), y32), ('bn_relu_maxpool values', what, beta is None)
        assert np.array_equal(_got(idx, mo).reshape(p32.shape), p32), ('bn_relu_maxpool positions', what, beta is None)
        dx = _out(mi, dt)
        _call('grl_maxpool3x3s2_bwd_idx' + sfx, idx, t['dy'], dx, n, H, W, C)
        rdx, S = R.maxpool_bwd(p32, dy, (H, W))
        B.check('maxpool_bwd_idx' + sfx, _got(dx, mi).reshape(rdx.shape), rdx, B.b_pool_bwd(S, rdx if b16 else None), what)
    t.unchanged()


@pytest.mark.parametrize('b16', (False, True))
@pytest.mark.parametrize('cls', B.MP_CLASSES)
@pytest.mark.parametrize('n,H,W,ci', B.MP_CASES)
def test_maxpool_family(n, H, W, ci, cls, b16):
    """H, W from 1 to 9, C that is and is not a multiple of 64; Gaussian, tied (post-ReLU, constant windows, an all-equal
    map) and all-negative maps"""
    C = (B.MP_C16 if b16 else B.MP_C32)[ci]
    _mp_run(B.mp_map(n, H, W, C, cls, b16), B.mp_dy(n, H, W, C, b16), B.mp_vectors(C), b16, (n, H, W, C, cls, b16))


@pytest.mark.parametrize('b16', (False, True))
def test_maxpool_family_past_one_pass_of_the_capped_grid(b16):
    """the `i += gridDim.x * blockDim.x` tail of the five grid-stride kernels: 8192 x 256 items and a few more"""
    name = 'mp16' if b16 else 'mp32'
    n, H, W, C = B.BIG[name]
    assert B.past_one_pass(B.big_items(name, B.BIG[name]), B.GRID_CAP)
    a = B.big_map(n, H, W, C)
    dy = B.big_map(n, 2, 2, C)[:, :R.pooled_size(H, W)[0], :R.pooled_size(H, W)[1], :]
    v = B.mp_vectors(C)
    Ho, Wo = R.pooled_size(H, W)
    dt = BF if b16 else torch.float32
    sfx = '_bf16' if b16 else ''
    t = _Inputs(dt, a=a, dy=dy, mean=v['mean'], scale=v['scale'], beta=v['beta'])
    mo, mi = n * Ho * Wo * C, n * H * W * C
    y = _out(mo, dt)
    _call('grl_maxpool3x3s2' + sfx, t['a'], y, n, H, W, C)
    want, pos = R.maxpool(a)
    assert np.array_equal(_got(y, mo).reshape(want.shape), want)
    rdx, S = R.maxpool_bwd(pos, dy, (H, W))
    bound = B.b_pool_bwd(S, rdx if b16 else None)
    dx = _out(mi, dt)
    _call('grl_maxpool3x3s2_bwd' + sfx, t['a'], t['dy'], dx, n, H, W, C)
    B.check('maxpool_bwd' + sfx, _got(dx, mi).reshape(rdx.shape), rdx, bound, 'big')
    del want, y, dx
    _, y32, p32 = B.bn_relu_maxpool_f32(a, v['mean'], v['scale'], v['beta'], b16)
    y, idx = _out(mo, dt), _out(mo, torch.uint8)
    _call('grl_bn_relu_maxpool3x3s2' + sfx, t['a'], t['mean'], t['scale'], t['beta'], y, idx, n, H, W, C)
    assert np.array_equal(_got(y, mo).reshape(y32.shape), y32)
    assert np.array_equal(_got(idx, mo).reshape(p32.shape), p32)
    # (the positions of the fused kernel: another routing than `pos`, checked against its own gather)
    rdx, S = R.maxpool_bwd(p32, dy, (H, W))
    dx = _out(mi, dt)
    _call('grl_maxpool3x3s2_bwd_idx' + sfx, idx, t['dy'], dx, n, H, W, C)
    B.check('maxpool_bwd_idx' + sfx, _got(dx, mi).reshape(rdx.shape), rdx, B.b_pool_bwd(S, rdx if b16 else None), 'big')
    t.unchanged()


# ----------------------------------------------------------------------------------------------------------------------
# im2col
def _im2col(n, H, W, Kp, b16, x):
    t = _Inputs(x32=x)
    m = n * (H // 2) * (W // 2) * Kp
    col = _out(m, BF if b16 else torch.float32)
    _call('grl_stem_im2col' + ('_bf16' if b16 else ''), t['x32'], col, n, H, W, Kp)
    want = R.im2col(x, Kp)
    if b16:
        want = B.bf16_round(want)                              # the copy rounds once: the same bits
    assert np.array_equal(_got(col, m).reshape(want.shape), want), (n, H, W, Kp, b16)
    t.unchanged()


@pytest.mark.parametrize('b16', (False, True))
@pytest.mark.parametrize('n,H,W', B.STEM_SHAPES)
def test_stem_im2col(n, H, W, b16):
    for Kp in B.IM2COL_KP:
        _im2col(n, H, W, Kp, b16, B.stem_image(n, H, W, 'a', False, False))


@pytest.mark.parametrize('b16', (False, True))
def test_stem_im2col_past_one_pass_of_the_capped_grid(b16):
    name = 'im2col16' if b16 else 'im2col32'
    n, H, W, Kp = B.BIG[name]
    assert B.past_one_pass(B.big_items(name, B.BIG[name]), B.GRID_CAP)
    _im2col(n, H, W, Kp, b16, B.f32(B.rng_for('bigcol', n, H, W).randint(-64, 65, (n, 3, H, W))))


# ----------------------------------------------------------------------------------------------------------------------
# rejections: GRL_EINVAL, nothing launched, the sentinel-filled outputs untouched
class _Refusals(object):
    def __init__(self, outputs):
        self.outputs = outputs
        torch.cuda.synchronize()
        self.before = [o.clone() for o in outputs]
        self.count = 0

    def refuse(self, name, *args):
        lib = _L()
        assert _rc(name, *args) == lib.GRL_EINVAL, (name, args)
        with pytest.raises(lib.GrlHipError):
            _call(name, *args)
        self.count += 1

    def untouched(self):
        torch.cuda.synchronize()
        for o, b in zip(self.outputs, self.before):
            assert torch.equal(o, b), 'a refused call wrote to its output'


def _vary(base, changes):
    """the argument lists that differ from `base` at one position each"""
    for i, values in changes.items():
        for v in values:
            yield base[:i] + (v,) + base[i + 1:]


@pytest.mark.parametrize('b16', (False, True))
def test_two_launch_stems_refuse_bad_arguments(b16):
    n, H, W = 2, 6, 4
    sfx = '_bf16' if b16 else ''
    for u8 in (False, True):
        d = B.stem_case(n, H, W, 'a', u8, b16)
        t = _stem_inputs(d)
        y = _out(n * 3 * 2 * 64, BF if b16 else torch.float32)
        r = _Refusals([y])
        if u8:
            base, dims = (t['x'], t['ms'], t['w'], t['scale'], t['shift'], y, n, H, W, 1, None), 6
            nulls = (0, 1, 2, 3, 4, 5)
        else:
            base, dims = (t['x'], t['w'], t['scale'], t['shift'], y, n, H, W, 1, None), 5
            nulls = (0, 1, 2, 3, 4)
        changes = {i: (None,) for i in nulls}
        changes.update({dims: (0, -1), dims + 1: (5, 7, 0, -2, -6), dims + 2: (3, 5, 0, -2, -4)})
        for args in _vary(base, changes):
            r.refuse('grl_stem_conv7x7' + ('_u8' if u8 else '') + sfx, *args)
        r.untouched()
        t.unchanged()


@pytest.mark.parametrize('b16', (False, True))
def test_fused_stem_and_pool_refuses_bad_arguments(b16):
    n, H, W = 2, 8, 128
    name = 'grl_stem_pool_bf16' if b16 else 'grl_stem_pool_f32'
    for u8 in (False, True):
        d = B.stem_case(n, H, W, 'a', u8, b16)
        t = _stem_inputs(d)
        wp = _pack(t['w'], 'bf16' if b16 else 'pool')
        y = _out(n * 2 * 32 * 64, BF if b16 else torch.float32)
        r = _Refusals([y])
        base = (t['x'], int(u8), t['ms'] if u8 else None, t['scale'], t['shift'], y, n, H, W, wp)
        changes = {0: (None,), 3: (None,), 4: (None,), 5: (None,), 9: (None,),
                   6: (0, -1, 65536),
                   7: (7, 9, 6, 10, 2, 0, -4, -8),             # odd; H % 4 != 0; H <= 0 (0: a division by zero before the guard)
                   8: (64, 126, 130, 127, 0, -128)}            # W != 128
        if u8:
            changes[2] = (None,)
            changes[0] = (None, t['x'].data_ptr() + 1)          # the kernel loads two pixels as one 2-byte word
        elif not b16:
            changes[0] = (None, t['x'].data_ptr() + 4)          # 8-byte row loads
        for args in _vary(base, changes):
            r.refuse(name, *args)
        r.untouched()
        t.unchanged()


@pytest.mark.parametrize('b16', (False, True))
def test_maxpool_family_refuses_bad_arguments(b16):
    n, H, W, C = 2, 5, 4, 8
    sfx = '_bf16' if b16 else ''
    dt = BF if b16 else torch.float32
    Ho, Wo = R.pooled_size(H, W)
    v = B.mp_vectors(C)
    t = _Inputs(dt, a=B.mp_map(n, H, W, C, 'a', b16), dy=B.mp_dy(n, H, W, C, b16), mean=v['mean'], scale=v['scale'], beta=v['beta'])
    mo, mi = n * Ho * Wo * C, n * H * W * C
    y, dx, idx = _out(mo, dt), _out(mi, dt), _out(mo, torch.uint8)
    good_idx = torch.zeros(mo + GUARD, dtype=torch.uint8, device='cuda')
    r = _Refusals([y, dx, idx])
    bad_c = (12, 4, 2) if b16 else (6, 2, 7)                     # C % 8 (bf16), C % 4 (fp32)
    dims = {0: (0, -1), 1: (0, -1, -5), 2: (0, -1, -4), 3: bad_c}

    def sweep(name, base, first_dim, nulls, extra=None):
        changes = {i: (None,) for i in nulls}
        changes.update({first_dim + k: vals for k, vals in dims.items()})
        changes.update(extra or {})
        for args in _vary(base, changes):
            r.refuse(name, *args)

    sweep('grl_maxpool3x3s2' + sfx, (t['a'], y, n, H, W, C), 2, (0, 1))
    sweep('grl_maxpool3x3s2_bwd' + sfx, (t['a'], t['dy'], dx, n, H, W, C), 3, (0, 1, 2))
    off = (idx.data_ptr() + 1, idx.data_ptr() + 2)              # off 4-byte alignment
    sweep('grl_bn_relu_maxpool3x3s2' + sfx, (t['a'], t['mean'], t['scale'], t['beta'], y, idx, n, H, W, C), 6, (0, 1, 2, 4, 5),
          {5: (None,) + off})
    goff = (good_idx.data_ptr() + 1, good_idx.data_ptr() + 2)
    sweep('grl_maxpool3x3s2_bwd_idx' + sfx, (good_idx, t['dy'], dx, n, H, W, C), 3, (0, 1, 2), {0: (None,) + goff})
    assert r.count > 60
    r.untouched()
    t.unchanged()


@pytest.mark.parametrize('b16', (False, True))
def test_stem_im2col_refuses_bad_arguments(b16):
    n, H, W, Kp = 1, 6, 4, 160
    t = _Inputs(x32=B.stem_image(n, H, W, 'a', False, False))
    col = _out(n * 3 * 2 * Kp, BF if b16 else torch.float32)
    r = _Refusals([col])
    base = (t['x32'], col, n, H, W, Kp)
    for args in _vary(base, {0: (None,), 1: (None,), 2: (0, -1), 3: (0, -2, -6), 4: (0, -2, -4), 5: (128, 146, 150, 0, -160)}):
        r.refuse('grl_stem_im2col' + ('_bf16' if b16 else ''), *args)
    r.untouched()
    t.unchanged()
