"""No GPU: (1) tests/stem_ref.py -- the float64 restatement of the stem convolution, the max-pool, its backward and the stem
im2col that the GPU kernels are compared with -- equals torch in float64 (F.conv2d, F.max_pool2d with its indices, autograd,
F.unfold): the reference is anchored to something that is not this project's code; (2) the fp32 restatements of
tests/stem_bounds.py stay within the derived bounds of the float64 reference, no element excluded: the bounds are
satisfiable; (3) the sweep the GPU file runs takes every side of each restated launch rule."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import stem_bounds as B
import stem_ref as R

REF_SHAPES = ((1, 2, 2), (2, 6, 4), (1, 14, 30), (2, 18, 34), (3, 10, 2))
MP_REF = ((1, 1, 1, 4), (2, 1, 2, 4), (1, 2, 1, 8), (2, 3, 4, 4), (3, 5, 9, 8), (2, 8, 8, 4), (1, 9, 4, 12), (2, 4, 5, 4))


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    yield
    B.dump_ratios('fp32 numpy restatements')


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _nchw(a):
    return _t(a).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


# ----------------------------------------------------------------------------------------------------------------------
# (1) the reference against torch
@pytest.mark.parametrize('n,H,W', REF_SHAPES)
def test_stem_reference_equals_torch(n, H, W):
    p = B.stem_params((H, W, 'ref'), False)
    x = B.stem_image(n, H, W, 'a', False, False)
    for relu in (0, 1):
        ref = R.stem(x, p['w'], p['scale'], p['shift'], relu, ex=np.abs(x))
        y = TF.conv2d(_t(x), _t(p['w']).view(64, 3, 7, 7), stride=2, padding=3)
        assert np.allclose(ref['acc'].reshape(n, H // 2, W // 2, 64), _nhwc(y), rtol=1e-12, atol=1e-13)
        y = y * _t(p['scale']).view(1, 64, 1, 1) + _t(p['shift']).view(1, 64, 1, 1)
        y = torch.relu(y) if relu else y
        assert np.allclose(ref['y'].reshape(n, H // 2, W // 2, 64), _nhwc(y), rtol=1e-12, atol=1e-13)
        A = TF.conv2d(_t(x).abs(), _t(p['w']).abs().view(64, 3, 7, 7), stride=2, padding=3)
        assert np.allclose(ref['A'].reshape(n, H // 2, W // 2, 64), _nhwc(A), rtol=1e-12, atol=1e-13)
        assert np.allclose(ref['E'], ref['A'], rtol=1e-12, atol=1e-13)          # ex = |x|
        assert (ref['A'] >= np.abs(ref['acc']) * (1 - 1e-12)).all()


def test_normalize_reference_equals_torch():
    u = B.stem_image(2, 6, 4, 'a', True, False)
    ms = _t(B.MEAN_STD)
    t = (_t(u) / 255.0 - ms[:3].view(1, 3, 1, 1)) / ms[3:].view(1, 3, 1, 1)
    assert np.array_equal(R.normalize(u, B.MEAN_STD), t.numpy())
    assert u.min() == 0 and u.max() == 255
    e = B.e_normalize(u)
    got = B.normalize_f32(u).astype(np.float64)
    assert (np.abs(got - R.normalize(u, B.MEAN_STD)) <= B.SAFETY * e).all()


def _torch_pool(a):
    """(values, positions ky * 3 + kx) of torch's max_pool2d on a [n][H][W][C] map"""
    n, H, W, C = a.shape
    v, i = TF.max_pool2d(_nchw(a), 3, 2, 1, return_indices=True)
    v, i = _nhwc(v), _nhwc(i)
    Ho, Wo = v.shape[1:3]
    ky = i // W - (2 * np.arange(Ho)[None, :, None, None] - 1)
    kx = i % W - (2 * np.arange(Wo)[None, None, :, None] - 1)
    assert ky.min() >= 0 and ky.max() <= 2 and kx.min() >= 0 and kx.max() <= 2
    return v, (ky * 3 + kx).astype(np.uint8)


@pytest.mark.parametrize('cls', B.MP_CLASSES)
@pytest.mark.parametrize('n,H,W,C', MP_REF)
def test_maxpool_reference_equals_torch_with_positions_and_autograd(n, H, W, C, cls):
    a = B.mp_map(n, H, W, C, cls, False)
    y, pos = R.maxpool(a)
    tv, tp = _torch_pool(a)
    assert y.shape[1:3] == R.pooled_size(H, W)
    assert np.array_equal(y, tv)
    assert np.array_equal(pos, tp)                  # ties included: torch records the first maximum in scan order
    if cls == 'c':
        assert (y < 0).all()                        # nothing but valid elements took part
    dy = B.mp_dy(n, H, W, C, False)
    a4 = _nchw(a).requires_grad_(True)
    TF.max_pool2d(a4, 3, 2, 1).backward(_nchw(dy))
    for first in (pos, a):
        dx, S = R.maxpool_bwd(first, dy, (H, W))
        assert np.allclose(dx, _nhwc(a4.grad), rtol=1e-14, atol=1e-15)
        assert (S >= np.abs(dx) * (1 - 1e-12)).all()


@pytest.mark.parametrize('n,H,W', REF_SHAPES)
def test_im2col_reference_equals_torch_unfold(n, H, W):
    x = B.stem_image(n, H, W, 'a', False, False)
    for Kp in B.IM2COL_KP:
        col = R.im2col(x, Kp)
        u = TF.unfold(_t(x), 7, padding=3, stride=2)            # [n][147][Ho * Wo]
        assert np.array_equal(col[:, :147], u.permute(0, 2, 1).reshape(-1, 147).numpy())
        assert not col[:, 147:].any()


# ----------------------------------------------------------------------------------------------------------------------
# (2) the fp32 restatements within the bounds
@pytest.mark.parametrize('cls', ('a', 'm'))
@pytest.mark.parametrize('u8', (False, True))
@pytest.mark.parametrize('n,H,W', ((2, 6, 4), (1, 14, 30), (1, 18, 34)))
def test_fp32_stem_restatements_within_bounds(n, H, W, u8, cls):
    d = B.stem_case(n, H, W, cls, u8, False)
    x32 = B.normalize_f32(d['x']) if u8 else d['x']
    for order, k, prod in (('mfma', B.K_MFMA, 1), ('pool', B.K_POOL_F32, 1), ('valu', B.K_VALU, 0)):
        bound = B.b_stem_f32(d['ref'], d['scale'], d['shift'], k, prod)
        for relu in (0, 1):
            got = B.stem_f32(x32, d['w'], d['scale'], d['shift'], relu, order)
            ref = np.maximum(d['ref']['y'], 0.0) if relu else d['ref']['y']
            B.check('cpu stem %s' % order, got, ref, bound, (n, H, W, u8, cls, relu))


@pytest.mark.parametrize('cls', ('a', 'm'))
@pytest.mark.parametrize('u8', (False, True))
@pytest.mark.parametrize('n,H,W', ((2, 6, 4), (1, 18, 34)))
def test_bf16_stem_restatement_within_bounds(n, H, W, u8, cls):
    d = B.stem_case(n, H, W, cls, u8, True)
    x16 = B.to_bf16(B.normalize_f32(d['x'])) if u8 else d['x']
    assert np.array_equal(B.to_bf16(d['w']), d['w']) and np.array_equal(B.to_bf16(x16), x16)
    for relu in (0, 1):
        ref = np.maximum(d['ref']['y'], 0.0) if relu else d['ref']['y']
        got = B.bf16_round(B.stem_f32(x16, d['w'], d['scale'], d['shift'], relu, 'pool'))
        B.check('cpu stem bf16', got, ref, B.b_stem_bf16(d['ref'], d['scale'], d['shift'], ref), (n, H, W, u8, cls, relu))


@pytest.mark.parametrize('b16', (False, True))
@pytest.mark.parametrize('n,H', ((1, 4), (2, 12)))
def test_fused_pool_restatement_within_the_window_bound(n, H, b16):
    """max-pooling a restated stem map stays within the largest stem bound of every window"""
    d = B.stem_case(n, H, 8, 'a', False, b16)
    Ho, Wo = H // 2, 4
    ref = np.maximum(d['ref']['y'], 0.0)
    stem = B.stem_f32(d['x'], d['w'], d['scale'], d['shift'], 1, 'pool')
    if b16:
        stem, bs = B.bf16_round(stem), B.b_stem_bf16(d['ref'], d['scale'], d['shift'], ref)
    else:
        bs = B.b_stem_f32(d['ref'], d['scale'], d['shift'], B.K_POOL_F32, 1)
    got = R.maxpool(stem.reshape(n, Ho, Wo, 64))[0]
    want = R.maxpool(ref.reshape(n, Ho, Wo, 64))[0]
    B.check('cpu stem + pool', got, want, B.pool_bound(bs, n, Ho, Wo), (n, H, b16))


@pytest.mark.parametrize('cls', B.MP_CLASSES)
@pytest.mark.parametrize('n,H,W,ci', B.MP_CASES[::3] + (B.BIG_CPU['mp32'][:3] + (0,),))
def test_bn_relu_maxpool_restatement_within_bounds(n, H, W, ci, cls):
    """the fp32 restatement of grl_bn_relu_maxpool3x3s2(_bf16) against float64: the activation within b_apply (plus half a
    bf16 spacing), the pooled value within the largest bound of its window; every element compared"""
    for b16, C in ((False, B.MP_C32[ci]), (True, B.MP_C16[ci])):
        z = B.mp_map(n, H, W, C, cls, b16)
        v = B.mp_vectors(C)
        for beta in (v['beta'], None):
            a32, y32, pos = B.bn_relu_maxpool_f32(z, v['mean'], v['scale'], beta, b16)
            a64 = np.maximum((R.f64(z) - R.f64(v['mean'])) * R.f64(v['scale']) + (0.0 if beta is None else R.f64(beta)), 0.0)
            ba = B.b_bn_relu(z, v['mean'], v['scale'], beta) + (0.5 * B.bf16_ulp(a64) if b16 else 0.0)
            B.check('cpu bn_relu a', a32, a64, ba, (n, H, W, C, cls, b16))
            y64 = R.maxpool(a64)[0]
            B.check('cpu bn_relu_maxpool y', y32, y64, B.pool_bound(ba, n, H, W), (n, H, W, C, cls, b16))
            assert pos.max() <= 8 and y32.shape == pos.shape
            # the recorded position holds the pooled value
            dx, _ = R.maxpool_bwd(pos, np.ones(pos.shape), (H, W))
            assert dx.sum() == pos.size


@pytest.mark.parametrize('n,H,W,ci', B.MP_CASES[1::3])
def test_maxpool_backward_restatement_within_bounds(n, H, W, ci):
    C = B.MP_C32[ci]
    a, dy = B.mp_map(n, H, W, C, 'b', False), B.mp_dy(n, H, W, C, False)
    pos = R.maxpool(a)[1]
    dx, S = R.maxpool_bwd(pos, dy, (H, W))
    got = np.zeros(dx.shape, np.float32)
    Ho, Wo = R.pooled_size(H, W)
    for oy in range(Ho):                                        # sequential fp32 additions, window by window
        for ox in range(Wo):
            p = pos[:, oy, ox, :].astype(np.int64)
            iy, ix = 2 * oy - 1 + p // 3, 2 * ox - 1 + p % 3
            ni, ci_ = np.meshgrid(np.arange(n), np.arange(C), indexing='ij')
            got[ni, iy, ix, ci_] += dy[:, oy, ox, :]
    B.check('cpu maxpool_bwd', got, dx, B.b_pool_bwd(S), (n, H, W, C))
    assert (got[S == 0] == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# (3) the sweep takes every side of the launch rules
def test_two_launch_sweep_reaches_every_tile_kind():
    for th, tw in ((8, 16), (16, 16)):
        kinds = set()
        for n, H, W in B.STEM_SHAPES:
            kinds |= B.tile_kinds(H, W, th, tw)
        assert kinds == {'full', 'x', 'y', 'xy'}, (th, tw, kinds)
    assert any(H // 2 == 1 and W // 2 == 1 for _, H, W in B.STEM_SHAPES)
    assert any(W // 2 == 1 and H // 2 > 1 for _, H, W in B.STEM_SHAPES)
    assert any(B.stem_tiles(H, W, 8, 16) == (1, 1) for _, H, W in B.STEM_SHAPES)
    assert any(min(B.stem_tiles(H, W, 8, 16)) > 1 for _, H, W in B.STEM_SHAPES)            # more than one workgroup each way
    walks = {B.b16_walk(H) for _, H, _ in B.STEM_SHAPES}
    assert any(w[0] > 1 for w in walks) and any(w[1] == 1 for w in walks) and any(1 < w[1] < 4 for w in walks)
    assert any(w == (w[0], 1) and w[0] > 1 for w in walks)      # a second workgroup that walks one tile
    assert max(n for n, _, _ in B.STEM_SHAPES) == 3
    assert all(H % 2 == 0 and W % 2 == 0 for _, H, W in B.STEM_SHAPES)


def test_fused_sweep_reaches_every_side_of_the_strip_rules():
    f32 = {(n, H): B.pool_f32_rule(n, H) for n, H in B.POOL_CASES}
    b16 = {(n, H): B.pool_b16_rule(n, H) for n, H in B.POOL_CASES if B.pool_b16_form(H) == 2}
    one = {(n, H): B.pool_b16_rule(n, H) for n, H in B.POOL_CASES if B.pool_b16_form(H) == 1}
    assert b16 and one                                          # both bf16 forms
    assert all(H % 8 == 4 for _, H in one) and all(H % 8 == 0 for _, H in b16)
    # pooled rows of 1, 2, 3
    assert {1, 2, 3} <= {H // 4 for _, H in B.POOL_CASES}
    for rules, total in ((f32, lambda H: H // 4), (b16, lambda H: H // 2)):
        assert any(s == 1 for s, _, _ in rules.values()) and any(s > 1 for s, _, _ in rules.values())
        assert any(g > 1 and B.last_strip_rows(total(H), per, g) < per for (n, H), (s, per, g) in rules.items())     # short last strip
        assert any(g < s for s, _, g in rules.values())         # fewer workgroups than strips asked for
    # the strip count capped by n * strips < 512, at the largest H
    Hm = B.POOL_H[-1]
    assert f32[(B.POOL_N_CAP, Hm)][0] < f32[(1, Hm)][0] and B.pool_f32_rule(B.POOL_N_CAP // 2, Hm)[0] == f32[(1, Hm)][0]
    assert b16[(B.POOL_N_CAP, Hm)][0] < b16[(1, Hm)][0]
    assert B.POOL_N_CAP * f32[(B.POOL_N_CAP, Hm)][0] >= 512
    # the first form: one workgroup and several, and a workgroup with a single pooled row (its strip holds two stem rows)
    assert any(g == 1 for _, _, g in one.values()) and any(g > 1 for _, _, g in one.values())
    assert any(B.last_strip_rows(H // 2, 32, g) == 2 and g == 1 for (n, H), (_, _, g) in one.items())
    assert any(B.last_strip_rows(H // 2, 32, g) == 2 and g > 1 for (n, H), (_, _, g) in one.items())         # ... below a warm-up tile
    assert {n for n, _ in B.POOL_CASES} == {1, 3, B.POOL_N_CAP}
    assert all(H % 4 == 0 for H in B.POOL_H)


def test_maxpool_sweep_pairs_every_size_with_an_odd_and_an_even_partner():
    for v in B.MP_SIZES:
        for axis in (0, 1):
            partners = {hw[1 - axis] for hw in B.MP_PAIRS if hw[axis] == v}
            assert any(p % 2 for p in partners) and any(p % 2 == 0 for p in partners), (v, axis, partners)
    assert {H for H, _ in B.MP_PAIRS} == set(B.MP_SIZES) == {W for _, W in B.MP_PAIRS}
    assert {ci for _, _, _, ci in B.MP_CASES} == {0, 1, 2, 3} and {n for n, _, _, _ in B.MP_CASES} == {1, 2, 3}
    assert all(c % 4 == 0 for c in B.MP_C32) and all(c % 8 == 0 for c in B.MP_C16)
    # C / 4 (C / 8) that divide the launch's thread count and that do not; one workgroup and several
    items = [n * R.pooled_size(H, W)[0] * R.pooled_size(H, W)[1] * (B.MP_C32[ci] // 4) for n, H, W, ci in B.MP_CASES]
    assert min(items) <= 256 < max(items)
    assert not any(B.past_one_pass(i, B.grid_even(i)) for i in items)


def test_big_cases_run_just_past_one_pass_of_the_capped_grid():
    for name, case in B.BIG.items():
        items = B.big_items(name, case)
        for grid in (B.grid_for(items), B.grid_even(items)):
            assert grid == B.GRID_CAP and B.past_one_pass(items, grid), (name, items)
        assert items <= B.GRID_CAP * 256 * 1.02, (name, items)   # just past
        small = B.big_items(name, B.BIG_CPU[name])
        assert 0 < small <= 4096
    assert B.grid_even(257) == 2 and B.grid_even(513) == 4 and B.grid_for(513) == 3 and B.grid_for(0) == 1


@pytest.mark.parametrize('name', ('mp32', 'mp16'))
def test_big_stand_ins_against_torch(name):
    n, H, W, C = B.BIG_CPU[name]
    a = B.big_map(n, H, W, C)
    assert np.array_equal(B.to_bf16(a), a)
    y, pos = R.maxpool(a)
    tv, tp = _torch_pool(a)
    assert np.array_equal(y, tv) and np.array_equal(pos, tp)


# ----------------------------------------------------------------------------------------------------------------------
# (4) the sweep's inputs tell the wrong rules apart (numpy only: what a kernel with that rule would return)
def _pool_variant(a, pad, last):
    """the max-pool with a pad value taking part (None: valid elements only) and, if `last`, the LAST maximum recorded (>=)"""
    a = R.f64(a)
    n, H, W, C = a.shape
    Ho, Wo = R.pooled_size(H, W)
    y = np.full((n, Ho, Wo, C), -np.inf if pad is None else float(pad))
    pos = np.zeros((n, Ho, Wo, C), np.uint8)
    first = np.ones((n, Ho, Wo, C), bool)
    for oy in range(Ho):
        for ox in range(Wo):
            for k in range(9):
                iy, ix = 2 * oy - 1 + k // 3, 2 * ox - 1 + k % 3
                if not (0 <= iy < H and 0 <= ix < W):
                    continue
                v = a[:, iy, ix, :]
                take = (v >= y[:, oy, ox, :]) if last else (v > y[:, oy, ox, :])
                take |= first[:, oy, ox, :] if pad is None else False
                y[:, oy, ox, :][take] = v[take]
                pos[:, oy, ox, :][take] = k
                first[:, oy, ox, :] = False
    return y, pos


@pytest.mark.parametrize('n,H,W,ci', B.MP_CASES)
def test_sweep_inputs_tell_a_zero_pad_and_a_last_maximum_rule_apart(n, H, W, ci):
    C = B.MP_C32[ci]
    for cls in B.MP_CLASSES:
        a = B.mp_map(n, H, W, C, cls, False)
        y, pos = R.maxpool(a)
        y0, p0 = _pool_variant(a, None, False)
        assert np.array_equal(y, y0) and np.array_equal(pos, p0)           # the brute-force loop agrees with the reference
    # (c) all-negative: a pad that behaves like 0 changes every output (every window of these maps touches the border or not,
    # its maximum is negative all the same)
    a = B.mp_map(n, H, W, C, 'c', False)
    assert (_pool_variant(a, 0.0, False)[0] != R.maxpool(a)[0]).all()
    # (b) ties: recording the last maximum moves positions, and the routed gradient with them, wherever a window holds more
    # than one element
    if H * W > 1:
        a, dy = B.mp_map(n, H, W, C, 'b', False), B.mp_dy(n, H, W, C, False)
        pos, plast = R.maxpool(a)[1], _pool_variant(a, None, True)[1]
        assert (pos != plast).any()
        dx, S = R.maxpool_bwd(pos, dy, (H, W))
        bad = np.abs(R.maxpool_bwd(plast, dy, (H, W))[0] - dx) > B.b_pool_bwd(S)
        assert bad.any()


@pytest.mark.parametrize('H,b16', ((36, False), (40, True), (68, True)))
def test_sweep_tells_a_lower_strip_without_its_warm_up_iteration_apart(H, b16):
    """a workgroup of a lower strip that skipped its warm-up iteration would pool its first row against a zero carry row:
    (row 2 py, row 2 py + 1) only.  On the sweep's inputs that misses the bound in that pooled row."""
    n, W = 1, B.POOL_W
    d = B.stem_case(n, H, W, 'a', False, b16)
    Ho, Wo = H // 2, W // 2
    ref = np.maximum(d['ref']['y'], 0.0).reshape(n, Ho, Wo, 64)
    if b16:
        _, rows, grid = B.pool_b16_rule(n, H)
        starts = [g * rows // 2 for g in range(1, grid)]
        bs = B.b_stem_bf16(d['ref'], d['scale'], d['shift'], ref.reshape(-1, 64))
    else:
        _, prows, grid = B.pool_f32_rule(n, H)
        starts = [g * prows for g in range(1, grid)]
        bs = B.b_stem_f32(d['ref'], d['scale'], d['shift'], B.K_POOL_F32, 1)
    assert starts
    want, bound = R.maxpool(ref)[0], B.pool_bound(bs, n, Ho, Wo)
    for py in starts:
        cut = R.maxpool(ref[:, 2 * py:2 * py + 2])[0][:, 0]               # the window without the row above
        assert (np.abs(cut - want[:, py]) > bound[:, py]).any(), (H, b16, py)
