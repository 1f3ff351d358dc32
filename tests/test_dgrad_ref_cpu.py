"""The float64 reference of the convolution backward (tests/dgrad_ref.py) against torch's float64 convolution gradients, its
two restatements against the definition, the layout formulas against plain torch indexing, and the sweep and bounds of
tests/dgrad_bounds.py: the route rule sends every route both forms, the K-block comments are true, the bounds hold for fp32
sums in the orders they claim to cover.  No GPU."""
import functools

import numpy as np
import pytest
import torch

import dgrad_bounds as B
import dgrad_ref as R

TOL = 1e-12                     # of each element's abs_terms: float64 sums of at most 9 * 160 terms, in two orders


@functools.lru_cache(maxsize=None)
def _ref(case, cls):
    cin, cout, k, stride, H, W, n = case
    Ho, Wo, pad = B.geometry(case)
    d = B.make_inputs(case, cls)
    dx, ab = R.dgrad(d['dz'], d['w'], n, H, W, Ho, Wo, k, stride, pad)
    dw, abw = R.wgrad(d['dz'], d['x'], n, H, W, Ho, Wo, k, stride, pad)
    for a in (dx, ab, dw, abw):
        a.setflags(write=False)
    return d, dx, ab, dw, abw


def _nchw(rows, n, H, W):
    return torch.from_numpy(np.ascontiguousarray(rows, np.float64)).view(n, H, W, -1).permute(0, 3, 1, 2).contiguous()


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).numpy()


def _close(got, want, abs_terms):
    assert got.shape == want.shape
    assert (np.abs(got - want) <= TOL * abs_terms + 1e-300 * (abs_terms == 0)).all() and (got[abs_terms == 0] == 0).all()


@pytest.mark.parametrize('cls', ('a', 'b'))
@pytest.mark.parametrize('case', B.CASES)
def test_reference_against_torch_float64(case, cls):
    from torch.nn.grad import conv2d_input, conv2d_weight
    cin, cout, k, stride, H, W, n = case
    Ho, Wo, pad = B.geometry(case)
    d, dx, ab, dw, abw = _ref(case, cls)
    g = _nchw(d['dz'], n, Ho, Wo)
    w = torch.from_numpy(d['w']).double()
    x = _nchw(d['x'], n, H, W)
    _close(dx, _rows(conv2d_input((n, cin, H, W), w, g, stride=stride, padding=pad)), ab)
    _close(ab, _rows(conv2d_input((n, cin, H, W), w.abs(), g.abs(), stride=stride, padding=pad)), ab)
    _close(dw, conv2d_weight(x, w.shape, g, stride=stride, padding=pad).numpy(), abw)
    _close(abw, conv2d_weight(x.abs(), w.shape, g.abs(), stride=stride, padding=pad).numpy(), abw)


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('case', [c for c in B.CASES if c[2] == 3 and c[3] == 2])
def test_stride2_restatements_equal_the_definition(case, cls):
    cin, cout, k, stride, H, W, n = case
    Ho, Wo, pad = B.geometry(case)
    d, dx, ab, _, _ = _ref(case, cls)
    ex, eab = R.dgrad_by_zero_stuffing(d['dz'], d['w'], n, H, W, Ho, Wo)
    _close(ex, dx, ab)
    _close(eab, ab, ab)
    if B.route(k, stride, H, W) == 'D':
        px, pab, terms = R.dgrad_by_parity(d['dz'], d['w'], n, H, W, Ho, Wo)
        _close(px, dx, ab)
        _close(pab, ab, ab)
        assert np.array_equal(terms * cout, B.k_terms(case))
    else:
        with pytest.raises(AssertionError):
            R.dgrad_by_parity(d['dz'], d['w'], n, H, W, Ho, Wo)


def test_layouts_against_torch_indexing():
    r = np.random.RandomState(3)
    w = r.standard_normal((5, 3, 3, 3)).astype(np.float32)
    wt = torch.from_numpy(w)
    assert np.array_equal(R.pack_dgrad(w), wt.flip(2, 3).permute(1, 2, 3, 0).reshape(3, 45).numpy())
    w1 = r.standard_normal((5, 3, 1, 1)).astype(np.float32)
    assert np.array_equal(R.pack_dgrad(w1), w1.reshape(5, 3).T)
    for py in (0, 1):
        for px in (0, 1):
            kys, kxs = ([1], [2, 0])[py], ([1], [2, 0])[px]
            want = wt[:, :, kys][:, :, :, kxs].permute(1, 2, 3, 0).reshape(3, -1).numpy()
            assert np.array_equal(R.w_dgrad_s2(w, py, px), want)
    buf = r.standard_normal(7 * 12).astype(np.float32)
    assert np.array_equal(R.transpose(buf, 7, 9, 12), torch.from_numpy(buf).view(7, 12)[:, :9].t().numpy())
    assert np.array_equal(R.transpose(buf[:63], 7, 9, 9), buf[:63].reshape(7, 9).T)


@pytest.mark.parametrize('H,W', [(6, 4), (5, 4), (6, 3), (5, 3), (7, 4)])
def test_dilate2_against_torch_indexing(H, W):
    """(7, 4): H == 2 Ho + 1, the one geometry in which `(y >> 1) < Ho` decides"""
    n, Ho, Wo, C = 2, 3, 2, 4
    r = np.random.RandomState(H * 10 + W)
    dz = r.standard_normal((n * Ho * Wo, C)).astype(np.float32)
    up0 = r.standard_normal((n * H * W, C)).astype(np.float32)
    for oy in (0, 1):
        for ox in (0, 1):
            ys = [y for y in range(oy, H, 2) if y // 2 < Ho]
            xs = [x for x in range(ox, W, 2) if x // 2 < Wo]
            src = torch.from_numpy(dz).view(n, Ho, Wo, C)[:, :len(ys), :len(xs)]
            for mode in (0, 1, 2):
                want = torch.zeros(n, H, W, C) if mode == 0 else torch.from_numpy(up0.copy()).view(n, H, W, C)
                if ys and xs:
                    view = want[:, ys[0]:ys[-1] + 1:2, xs[0]:xs[-1] + 1:2]
                    view.copy_(view + src if mode == 1 else src)
                got = R.dilate2(dz, None if mode == 0 else up0, n, Ho, Wo, H, W, C, mode, oy, ox)
                assert got.dtype == np.float32 and np.array_equal(got, want.reshape(-1, C).numpy())
                assert R.dilate2_hit(n, Ho, Wo, H, W, oy, ox).sum() == n * len(ys) * len(xs)


def test_fused_epilogue_reference():
    r = np.random.RandomState(5)
    M, N = 9, 8
    acc, res, z = r.standard_normal((3, M, N))
    mean, mbeta = r.standard_normal((2, N))
    invstd, mscale = r.uniform(0.5, 2.0, (2, N))
    ep = R.fused_epilogue(acc, res, z, mean, invstd, mscale, mbeta)
    t = torch.from_numpy(z).requires_grad_(True)
    pre = (t - torch.from_numpy(mean)) * torch.from_numpy(mscale) + torch.from_numpy(mbeta)
    assert np.array_equal(ep['mask'], (pre > 0).numpy()) and np.allclose(ep['pre'], pre.detach().numpy(), rtol=1e-15)
    assert np.allclose(ep['g'], (acc + res) * ep['mask']) and np.allclose(ep['sum_g'], ep['g'].sum(0))
    assert np.allclose(ep['sum_gx'], (ep['g'] * (z - mean) * invstd).sum(0), rtol=1e-13)
    bits = r.random_sample((M, N)) < 0.5
    eb = R.fused_epilogue(acc, None, z, mean, invstd, bits=bits)
    assert eb['pre'] is None and np.array_equal(eb['g'], np.where(bits, acc, 0.0))
    packed = (bits.reshape(-1, 4) << np.arange(4)).sum(1).astype(np.uint8)
    assert np.array_equal(R.unpack_bits(packed, M * N), bits.reshape(-1))


def test_route_rule_and_kblock_sides():
    """every route runs on at least two sweep entries; the entries' comments name their route, and the side of the 256-row
    rule ('seg' / 'chain', '> 256', '<= 256') they claim -- for the GEMM the route really issues"""
    routes = {}
    for entry in B.SWEEP:
        case, why = entry[:7], entry[7]
        r = B.route(case[2], case[3], case[4], case[5])
        routes.setdefault(r, []).append(case)
        assert why.startswith(r + ':'), entry
        calls = B.gemm_calls(case)
        if 'seg' in why:
            assert any(B.takes_segmented_kernel(M, K) for M, _, K in calls), entry
        else:
            assert not any(B.takes_segmented_kernel(M, K) for M, _, K in calls), entry
        if 'chain' in why:
            assert all(M > B.KBLOCK_ROWS for M, _, _ in calls) and any(K > B.KBLOCK_K for _, _, K in calls), entry
        if '> 256' in why:
            assert all(M > B.KBLOCK_ROWS for M, _, _ in calls), entry
        if '<= 256' in why:
            assert all(M <= B.KBLOCK_ROWS for M, _, _ in calls), entry
        assert all(K % 32 == 0 and N % 32 == 0 for _, N, K in calls) and case[1] % 32 == 0
        assert len(B.launches(case, 0)) == len(B.launches(case, 1))
    assert sorted(routes) == list('ABCDE') and all(len(v) >= 2 for v in routes.values())
    for r, cases in routes.items():             # both sides of 256 rows on every route
        ms = [M for c in cases for M, _, _ in B.gemm_calls(c)]
        assert min(ms) <= B.KBLOCK_ROWS < max(ms), (r, ms)
    segs = [r for r, cases in routes.items() for c in cases if any(B.takes_segmented_kernel(M, K) for M, _, K in B.gemm_calls(c))]
    assert set(segs) == set('CDE')              # (A and B: K = cout <= 512 on every layer of the model and of the sweep)
    assert {B.tag_pixel(c, i)[3] for i, c in enumerate(B.CASES)} == set(B.TAG_PIXELS)
    assert {B.route(c[2], c[3], c[4], c[5]) for c in B.FORCED_TILE_CASES} == set('CDE')
    assert any(B.bf16_accepts(c) for c in routes['D']) and all(any(B.bf16_accepts(c) for c in v) for v in routes.values())


@pytest.mark.parametrize('index,case', list(enumerate(B.CASES)))
def test_tagged_class_names_one_tap_per_nonzero(index, case):
    cin = case[0]
    d, dx, ab, _, _ = _ref(case, 't')
    Ho, Wo, _ = B.geometry(case)
    assert int((d['dz'] != 0).any(1).sum()) == 1
    want = B.tagged_footprint(case, index)
    assert 1 <= want <= case[2] ** 2
    assert int((dx != 0).sum()) == want * cin and int((ab != 0).sum()) == want * cin
    assert int((dx != 0).any(1).sum()) == want


def test_fp32_fused_epilogue_stays_inside_the_bounds():
    """the fused epilogue in fp32 (numpy): acc rounded once from float64 (inside any K u abs_terms), + res, the mask from the
    fp32 pre-activation, the two column sums as one sequential chain per 64-row tile -- against fused_bounds"""
    f = np.float32
    r = B.rng_for('fused cpu')
    M, N, K = 150, 8, 96
    a, w = r.standard_normal((M, K)), r.standard_normal((K, N)) / np.sqrt(K)
    acc, ab = a @ w, np.abs(a) @ np.abs(w)
    res, z = B.f32(r.standard_normal((M, N))), B.f32(1.5 * r.standard_normal((M, N)) + 0.3)
    mean, invstd = B.f32(z.mean(0)), B.f32(1.0 / z.std(0))
    mscale, mbeta = B.f32(invstd * r.uniform(0.5, 1.5, N)), B.f32(r.uniform(-0.7, 0.7, N))
    for has_res in (False, True):
        ep = R.fused_epilogue(acc, res if has_res else None, z, mean, invstd, mscale, mbeta)
        assert (np.abs(ep['pre']) > B.b_mask_margin(z, mean, mscale, mbeta)).all()
        v = acc.astype(f) + res if has_res else acc.astype(f)
        zc = z - mean
        mask = zc * mscale + mbeta > 0
        assert np.array_equal(mask, ep['mask'])
        g = np.where(mask, v, f(0))
        s, q = np.zeros(N), np.zeros(N)
        for t0 in range(0, M, 64):              # a tile: two chains of at most 32 rows, added (depth 33 <= K_GEMM_STATS)
            half = []
            for h0 in (t0, t0 + 32):
                ts, tq = np.zeros(N, f), np.zeros(N, f)
                for m in range(h0, min(M, h0 + 32)):
                    ts = ts + g[m]
                    tq = tq + g[m] * (zc[m] * invstd)
                half.append((ts, tq))
            s, q = s + (half[0][0] + half[1][0]), q + (half[0][1] + half[1][1])
        bd = B.fused_bounds(ep, K, ab, has_res)
        B.check('cpu fused g', g, ep['g'], bd['g'], has_res)
        B.check('cpu fused sum g', s, ep['sum_g'], bd['sum_g'], has_res)
        B.check('cpu fused sum g xhat', q, ep['sum_gx'], bd['sum_gx'], has_res)


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    yield
    B.dump_ratios('fp32 restatements (CPU)')


@pytest.mark.parametrize('cls', ('a', 'b'))
@pytest.mark.parametrize('case', [B.CASES[0], B.CASES[3], B.CASES[5], B.CASES[10], B.CASES[14]])
def test_fp32_sums_stay_inside_the_bounds(case, cls):
    """the data gradient as an fp32 GEMM over im2col'd operands in three orders (numpy's, one sequential chain, 32-k blocks)
    against the float64 reference and b_dx; the accumulate form adds G0 in fp32; class (b)'s bound dwarfs |dx|"""
    cin, cout, k, stride, H, W, n = case
    Ho, Wo, pad = B.geometry(case)
    d, dx, ab, dw, abw = _ref(case, cls)
    g = _nchw(d['dz'], n, Ho, Wo)
    # im2col of the zero-stuffed, padded dz against the flipped weight: [n H W][k k cout] . [k k cout][cin]
    up = d['dz'].astype(np.float64) if stride == 1 else R.dilate2(d['dz'].astype(np.float64), None, n, Ho, Wo, H, W, cout, 0, 0, 0)
    padded = np.zeros((n, H + 2 * pad, W + 2 * pad, cout))
    padded[:, pad:pad + H, pad:pad + W] = up.reshape(n, H, W, cout)
    cols = np.concatenate([padded[:, ty:ty + H, tx:tx + W].reshape(n * H * W, cout) for ty in range(k) for tx in range(k)], 1)
    wm = np.concatenate([d['w'].astype(np.float64)[:, :, k - 1 - ty, k - 1 - tx] for ty in range(k) for tx in range(k)], 0)
    assert np.allclose(cols @ wm, dx, rtol=0, atol=1e-11 * max(1.0, ab.max()))
    worst = 0.0
    for fn in (B.dot_numpy_f32, B.dot_sequential_f32, B.dot_blocked_f32):
        got = fn(cols, wm)
        # the im2col K is k k cout for every pixel: at least the route's own K, so the route's bound is the tighter one for D
        bound = B.SAFETY * k * k * cout * B.U * ab
        worst = max(worst, B.check('cpu dx', got, dx, bound, (case, cls, fn.__name__)))
        acc = got + d['g0']
        B.check('cpu dx accumulate', acc, dx + d['g0'].astype(np.float64),
                bound + B.SAFETY * np.where(ab > 0, B.U * np.abs(dx + d['g0']), 0.0), (case, cls, fn.__name__))
    assert (B.b_dx(case, ab, dx, 0) <= B.SAFETY * k * k * cout * B.U * ab).all()
    if cls == 'b':
        assert np.median(B.b_dx(case, ab, dx, 0)[ab > 0] / np.maximum(np.abs(dx[ab > 0]), 1e-300)) > 1e-6
    M = n * Ho * Wo
    x32 = torch.from_numpy(d['x']).view(n, H, W, cin).permute(0, 3, 1, 2)
    got = torch.nn.grad.conv2d_weight(x32, d['w'].shape, g.float(), stride=stride, padding=pad).numpy()
    B.check('cpu dw', got, dw, B.b_dw(M, abw, dw), (case, cls))
