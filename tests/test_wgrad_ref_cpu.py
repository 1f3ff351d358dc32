"""No GPU: the float64 weight-gradient references of wgrad_ref.py against torch's float64 autograd, the bounds of
wgrad_bounds.py against fp32 numpy restatements of the kernels' summation orders (satisfiable), against seven mutations of
those restatements (sharp), and the coverage the sweep must reach, computed from the restated host rules."""
import functools

import numpy as np
import pytest
import torch

import wgrad_bounds as B
import wgrad_ref as R

IDS = ['%d-%s' % (i, B.kernel_body(e).split('<')[0]) for i, e in enumerate(B.SWEEP)]
STEM_CHANNELS = (0, 1, 31, 32, 47, 63)      # the restatement of the 500+-tile stem entries runs on these output channels


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    yield
    for stage in [s for s in B.RATIOS if s.startswith('mutated')]:      # (those are meant to be over 1)
        del B.RATIOS[stage]
    B.dump_ratios('fp32 restatements of the weight gradient (CPU)')


@functools.lru_cache(maxsize=None)
def _ref(index, cls):
    e = B.SWEEP[index]
    d = B.make_inputs(e, cls)
    out = B.reference(e, d)
    for a in list(d.values()) + list(out):
        a.setflags(write=False)
    return d, out


def _channels(e):
    return np.array(STEM_CHANNELS) if (e.kind == 'stem' and B.stem_tiles(e)[2] > 64) else None


def _restate_and_check(index, cls, mutate=None, stage='cpu', forms=(0, 1)):
    """the fresh form and (the same sum added to the preload in fp32) the accumulate form"""
    e = B.SWEEP[index]
    d, (ref, ab, terms) = _ref(index, cls)
    g0 = d['g0']
    if e.kind == 'stem':
        ch = _channels(e)
        fresh = B.restate_stem(e, d, 0, mutate, ch)
        if ch is not None:
            ref, ab, terms, g0 = ref[ch], ab[ch], terms[ch], g0[ch]
    else:
        fresh = B.restate(e, d, 0, mutate)
    for accumulate in forms:
        got = B.accumulated(g0, fresh) if accumulate else fresh
        want = ref + g0.astype(np.float64) if accumulate else ref
        bound = B.bound(e, ab, terms, want, accumulate)
        B.check('%s %s' % (stage, B.datapath(e)), got, want, bound, (index, e.why, cls, accumulate, mutate))
        exact = bound == 0
        assert np.array_equal(got[exact], want[exact].astype(np.float32)), 'a value no term reaches moved'


# ----------------------------------------------------------------------------------------------------------------------
# references against an independent statement
def _autograd_conv(dz, x_nchw, N, C, k, stride, pad):
    w = torch.zeros(N, C, k, k, dtype=torch.float64, requires_grad=True)
    out = torch.nn.functional.conv2d(x_nchw, w, stride=stride, padding=pad)
    return torch.autograd.grad(out, w, dz)[0].numpy()


CONV_GEOMS = sorted({(e.geom, e.N) for e in B.SWEEP if e.kind == 'conv'})


@pytest.mark.parametrize('geom,N', CONV_GEOMS)
def test_conv_reference_is_autograd(geom, N):
    n, H, W, C, k, stride, pad = geom
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    N = min(N, 24)                                      # (the reference has no tiles: a few output channels say it all)
    r = B.rng_for('autograd', *geom)
    dz, x = r.standard_normal((n * Ho * Wo, N)), r.standard_normal((n * H * W, C))
    dw, ab, terms = R.conv(dz, x, n, H, W, Ho, Wo, k, stride, pad)
    want = _autograd_conv(torch.from_numpy(dz).view(n, Ho, Wo, N).permute(0, 3, 1, 2),
                          torch.from_numpy(x).view(n, H, W, C).permute(0, 3, 1, 2), N, C, k, stride, pad)
    assert dw.shape == (N, C, k, k)
    assert np.abs(dw - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # abs_terms is the same sum over absolute values, terms the same sum over ones
    wa = _autograd_conv(torch.from_numpy(np.abs(dz)).view(n, Ho, Wo, N).permute(0, 3, 1, 2),
                        torch.from_numpy(np.abs(x)).view(n, H, W, C).permute(0, 3, 1, 2), N, C, k, stride, pad)
    wt = _autograd_conv(torch.ones(n, N, Ho, Wo, dtype=torch.float64), torch.ones(n, C, H, W, dtype=torch.float64),
                        N, C, k, stride, pad)
    assert np.abs(ab - wa).max() <= 1e-12 * np.abs(wa).max() and np.array_equal(terms, wt)


@pytest.mark.parametrize('n,H,W', sorted({e.geom for e in B.SWEEP if e.kind == 'stem' and e.M <= 4096}) + [(3, 6, 10)])
def test_stem_reference_is_autograd(n, H, W):
    Ho, Wo = H // 2, W // 2
    r = B.rng_for('autograd stem', n, H, W)
    dz, x = r.standard_normal((n * Ho * Wo, 64)), r.standard_normal((n, 3, H, W))
    dw, ab, terms = R.stem(dz, x, n, H, W)
    g = torch.from_numpy(dz).view(n, Ho, Wo, 64).permute(0, 3, 1, 2)
    want = _autograd_conv(g, torch.from_numpy(x), 64, 3, 7, 2, 3)
    assert np.abs(dw - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    wt = _autograd_conv(torch.ones_like(g), torch.ones(n, 3, H, W, dtype=torch.float64), 64, 3, 7, 2, 3)
    assert np.array_equal(terms, wt)
    # the gathered operand of the restatement is the same convolution: dz^T . columns
    cols = R.stem_columns(x, n, H, W)
    assert np.abs((dz.T @ cols).reshape(64, 3, 7, 7) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_dense_reference_is_matmul():
    r = B.rng_for('autograd dense')
    dz, x = r.standard_normal((37, 48)), r.standard_normal((37, 80))
    dw, ab, terms = R.dense(dz, x, 40, 72, 68)
    want = (torch.from_numpy(dz)[:, :40].t() @ torch.from_numpy(x)[:, :68]).numpy()
    assert dw.shape == (40, 68) and np.abs(dw - want).max() <= 1e-12
    assert np.array_equal(terms, np.full((40, 68), 37.0)) and (ab >= np.abs(dw)).all()


def test_slab_to_torch_layout():
    slab = np.arange(2 * 3 * 4).reshape(2, 12)          # [N = 2][taps = 3][C = 4]
    t = R.to_torch_layout(slab, 2, 4, 3)
    assert t.shape == (2, 4, 3) and t[1, 2, 1] == slab[1, 1 * 4 + 2]


# ----------------------------------------------------------------------------------------------------------------------
# the bounds are satisfiable: every sweep entry, every class, both forms
@pytest.mark.parametrize('index', range(len(B.SWEEP)), ids=IDS)
def test_restatement_meets_the_bounds(index):
    e = B.SWEEP[index]
    for cls in B.classes(e):
        _restate_and_check(index, cls)
        d, (ref, ab, terms) = _ref(index, cls)
        if cls in 'tu':                                 # every non-zero is a single product
            assert terms.max() <= 1 and (ab[terms == 0] == 0).all()
        if cls == 'b' and e.M >= 32:
            # (a conv's border taps sum over a part of the pixels only: dz sums to zero over all of them, not over a part)
            assert np.abs(ref).sum() < (0.05 if e.kind == 'dense' else 0.3) * ab.sum(), 'class (b) does not cancel'


def test_math_modes_miss_the_fp32_bound():
    """what the GPU test relies on to tell which datapath ran: on general fp32 operands the math = bf16 restatement misses
    the exact-fp32 bound on a 128 x 128 tile, the fallback entries (64 x 128 tile) meet it.  (bf16x3 is built to be about as
    accurate as fp32: it may meet that bound or not, nothing is asked of it here.)"""
    seen = set()
    for index, e in enumerate(B.SWEEP):
        if e.math == B.MATH_F32 or e.b16 or B.datapath(e) == 'bf16x3':
            continue
        seen.add(B.datapath(e))
        d, (ref, ab, terms) = _ref(index, 'a')
        got = B.restate(e, d, 0)
        b32 = B.bound(e, ab, terms, ref, 0, as_fp32=True)
        over = (np.abs(got - ref) > b32).any()
        assert over == (B.datapath(e) != 'f32'), (index, e.why)
    assert seen == {'bf16', 'f32'}


# ----------------------------------------------------------------------------------------------------------------------
# the bounds are sharp: each mutation of the restatement fails `check` on at least one sweep entry
def _fails(index, cls, accumulate, mutate):
    try:
        _restate_and_check(index, cls, mutate, stage='mutated', forms=(accumulate,))
    except AssertionError:
        return True
    return False


def _applies(e, mutate):
    if mutate == 'stale_patch':
        return e.kind == 'stem' and B.stem_trips(e) > 1
    if e.kind == 'stem':
        return False
    if mutate == 'late_stage':
        return B.real_splits(e) > 1
    if mutate in ('shift_tap', 'wrap_tap'):
        return e.kind == 'conv' and e.geom[4] == 3
    if mutate == 'no_lo_hi':
        return B.datapath(e) == 'bf16x3'
    if mutate == 'xcd_swap':
        return B.wgrad_tile_mode(*B.tiles_nk(e)) != 0
    return True


@pytest.mark.parametrize('mutate', B.MUTATIONS)
def test_mutation_is_caught(mutate):
    entries = [i for i, e in enumerate(B.SWEEP) if _applies(e, mutate)]
    assert entries, 'no sweep entry can show this mutation'
    caught = {}
    for i in entries[:6]:
        caught[i] = [cls for cls in B.classes(B.SWEEP[i]) if _fails(i, cls, 0, mutate)]
    assert any(caught.values()), (mutate, caught)
    # the tagged classes alone (a single product per element) catch a wrong row or tap wherever their pixel meets it
    if mutate in ('no_lo_hi', 'wrap_tap'):
        assert any(set(c) & set('tu') for c in caught.values()), (mutate, caught)


# ----------------------------------------------------------------------------------------------------------------------
# coverage, computed from the restated rules
def _wg(entries):
    return [e for e in entries if e.kind != 'stem']


def test_sweep_reaches_every_kernel_body_and_tile():
    bodies = {B.kernel_body(e) for e in B.SWEEP}
    want = {'stem_wgrad_kernel<true>', 'stem_wgrad_kernel<false>'}
    for cv in ('true', 'false'):
        want |= {'wgrad_b16in_256_kernel<%s>' % cv, 'wgrad_b16in_kernel<%s>' % cv,
                 'wgrad_kernel<128, 128, %s, 1>' % cv, 'wgrad_kernel<128, 128, %s, 3>' % cv}
        want |= {'wgrad_kernel<%d, %d, %s, 0>' % (bm, bn, cv) for bm in (64, 128) for bn in (64, 128)}
    assert want <= bodies, sorted(want - bodies)
    # the silent fallback is in the sweep: a bf16 / bf16x3 request that runs the exact-fp32 kernel
    assert {e.math for e in B.SWEEP if e.math != B.MATH_F32 and B.datapath(e) == 'f32'} == {B.MATH_BF16, B.MATH_BF16X3}


def test_sweep_reaches_every_conv_path_and_tile_map_mode():
    assert {B.conv_path(e) for e in B.SWEEP} >= {'lin', 'generic', 'small_img'}
    modes = {B.wgrad_tile_mode(*B.tiles_nk(e)) for e in _wg(B.SWEEP)}
    assert modes == {0, 1, 2}
    # lin entries with every fp32 tile shape, and one whose split boundary lies inside an image
    lin = [e for e in B.SWEEP if B.conv_path(e) == 'lin']
    assert {B.wgrad_tile(e) for e in lin} == {(64, 64), (64, 128), (128, 64), (128, 128)}
    assert any(B.real_splits(e) > 1 and B.chunk(e) % (B.out_hw(e)[0] * B.out_hw(e)[1]) != 0 for e in lin)
    # small_img with several images per 32-row stage
    assert any(B.conv_path(e) == 'small_img' and B.out_hw(e)[0] * B.out_hw(e)[1] < 16 for e in B.SWEEP)
    # the tile map is a bijection for every entry (which tile a workgroup computes enters no sum)
    for e in _wg(B.SWEEP):
        tn, tk = B.tiles_nk(e)
        mode = B.wgrad_tile_mode(tn, tk)
        assert sorted(B.wgrad_tile_of(b, tn, tk, mode) for b in range(tn * tk)) == [(i, j) for i in range(tn) for j in range(tk)]


def test_sweep_reaches_every_split_count_and_stage_count():
    f32 = [e for e in _wg(B.SWEEP) if B.datapath(e) == 'f32']
    counts = {B.real_splits(e) for e in f32}
    assert {1, 2, 3, 4, 5} <= counts and max(counts) >= 9, counts
    assert any(B.split_rows(e)[-1][1] - B.split_rows(e)[-1][0] < 32 and B.real_splits(e) > 1 for e in f32)
    # the reduce's unrolled-by-4 loop with and without a tail
    assert any(B.real_splits(e) == 4 for e in f32) and any(B.real_splits(e) > 4 and B.real_splits(e) % 4 for e in f32)
    # the 256-wide tile's three-buffer ring: splits of exactly 1, 2, 3 and >= 4 stages; ragged in N and K; straddling taps
    big = [e for e in B.SWEEP if B.datapath(e) == 'b16in_256']
    stages = {s for e in big for s in B.stages_per_split(e)}
    assert {1, 2, 3} <= stages and max(stages) >= 4, stages
    assert any(e.N % 256 and e.K % 256 for e in big)
    assert {e.geom[3] for e in big if e.kind == 'conv'} == {64, 128}
    assert any(B.real_splits(e) > 1 for e in big)
    # M <= 2049 everywhere but the stem
    assert max(e.M for e in _wg(B.SWEEP)) <= 2049
    # the workspace may be larger than what a launch uses, never smaller
    assert all(B.wgrad_splits(e) >= B.real_splits(e) for e in _wg(B.SWEEP))


def test_sweep_reaches_the_stem_trips():
    stems = [e for e in B.SWEEP if e.kind == 'stem']
    for b16 in (0, 1):
        trips = {B.stem_trips(e, wg) for e in stems if e.b16 == b16 for wg in range(B.stem_wgs(e))}
        assert trips == {1, 2, 3}, trips
    e2 = next(e for e in stems if e.geom == (520, 16, 32))
    assert [wg for wg in range(512) if B.stem_trips(e2, wg) == 2] == list(range(8))
    e3 = next(e for e in stems if e.geom == (1030, 6, 10))
    assert [wg for wg in range(512) if B.stem_trips(e3, wg) == 3] == list(range(6))
    # the tagged pixel of a several-trip entry lies in a second-trip tile
    for e in (e2, e3):
        row, which = B.tag_row(e, 't', B.SWEEP.index(e))
        n, H, W = e.geom
        ty, tx, _ = B.stem_tiles(e)
        img, oy, ox = row // ((H // 2) * (W // 2)), (row // (W // 2)) % (H // 2), row % (W // 2)
        tile = (img * ty + oy // B.SW_TH) * tx + ox // B.SW_TW
        assert which == 'second-trip tile' and 512 <= tile < 1024


def test_issue_examples_follow_the_rules():
    """the figures the sweep's comments state, from the restated rules"""
    by = {(e.kind, e.M, e.N, e.K, e.b16, e.math): e for e in B.SWEEP}
    e = by[('dense', 257, 128, 256, 0, 0)]
    assert (B.real_splits(e), B.chunk(e)) == (2, 160)
    assert [B.real_splits(by[('dense', M, 128, 256, 0, 0)]) for M in (513, 1000, 1025, 2049)] == [3, 4, 5, 9]
    assert B.split_rows(by[('dense', 2049, 128, 256, 0, 0)])[-1] == (2048, 2049)
    assert B.wgrad_tile(by[('dense', 260, 264, 520, 1, 0)]) == (128, 128)          # 137 280 < 2^19
    assert B.wgrad_tile(by[('dense', 20, 520, 1032, 1, 0)]) == (256, 256)
    assert [B.stages_per_split(by[('dense', M, 520, 1032, 1, 0)]) for M in (20, 64, 96, 100, 257)] == [[1], [2], [3], [4], [5, 4]]
    assert B.wgrad_tile_mode(*B.tiles_nk(by[('dense', 40, 512, 2048, 0, 0)])) == 1
    assert B.wgrad_tile_mode(*B.tiles_nk(by[('dense', 40, 2048, 512, 0, 0)])) == 2
    # the two shapes test_gpu_train_bf16.py once called "the 256 x 256 LDS-DMA tile" take the 128-wide kernel
    for M, N, K in ((5000, 264, 520), (33, 256, 256)):
        assert B.wgrad_tile(B._dense(M, N, K, '', b16=1)) == (128, 128)
    assert B.wgrad_tile(B._dense(4096, 512, 2048, '', b16=1)) == (256, 256)
