"""The float64 reference of the OIM, triplet and pair loss kernels (tests/loss_ref.py) is right, and the bounds of
tests/loss_bounds.py are satisfiable -- both shown without a GPU:

* every function of loss_ref against torch float64 on the CPU -- forwards against the plain torch expression
  (F.cross_entropy, the batch-hard expression of test_triplet_forward_backward, F.softmax, F.binary_cross_entropy),
  backwards against torch.autograd.grad of it -- over the sweep of the GPU file;
* the sweep takes both sides of every branch it claims to take, and every class-(a) triplet case meets the gap condition
  under which the GPU file may compare the kernel's selection with the float64 one;
* fp32 numpy restatements of the reductions in the kernels' own order against loss_ref inside the very bounds the GPU tests
  hold the kernels to.

TOL = 1e-12 of each element's absolute terms, as in test_head_ref_cpu.py: both sides are float64."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import loss_bounds as B
import loss_ref as R

TOL = 1e-12
IGNORE = -100


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    yield
    B.dump_ratios('fp32 numpy restatement of the loss kernels (CPU)')


def _t(a, grad=False):
    return torch.from_numpy(np.array(a, dtype=np.float64)).requires_grad_(grad)


def _close(got, ref, what, scale=None):
    ref = ref.detach().numpy() if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64).reshape(ref.shape)
    s = np.abs(ref) if scale is None else np.maximum(np.abs(ref), np.broadcast_to(scale, ref.shape))
    bad = np.abs(got - ref) > TOL * s + 1e-300
    assert not bad.any(), (what, float((np.abs(got - ref) / (s + 1e-300)).max()), int(bad.sum()))


# ----------------------------------------------------------------------------------------------------------------------
def test_sweep_takes_both_sides_of_every_branch():
    # softmax_ce_kernel: lanes of the 256 with no trip, one, two, three, five; fewer classes than a wave; ties in one lane's
    # second trip, across waves, and with the later index in the earlier wave
    t = [B.lane_trips(c, 256) for c in B.CE_C]
    assert {(0, 1), (1, 1), (1, 2), (2, 3), (4, 5)} <= set(t)
    assert min(B.CE_C) < 64 and {255, 256, 257} <= set(B.CE_C)
    (a0, b0), (a1, b1), (a2, b2) = B.CE_TIES
    assert a0 % 256 == b0 % 256 and b0 >= 256
    assert a1 // 64 != b1 // 64 and max(a1, b1) < 256
    assert a2 > b2 and a2 // 64 != b2 // 64
    assert any(c > max(max(p) for p in B.CE_TIES) for _, c, cls in B.CE_CASES if cls == 't')
    assert any(n == 9 for n, _, cls in B.CE_CASES if cls == 't')            # 9 rows: every pair with every label position
    assert len(set(B.CE_FLAGS)) == 16
    for n in (3, 9):
        for c in (3, 257):
            y = B.ce_labels(B.rng_for(0), n, c, 'mixed')
            assert (y == -100).sum() == 1 and (y == c).sum() == 1 and ((y >= 0) & (y < c)).any()
            y = B.ce_labels(B.rng_for(0), n, c, 'none')
            assert not ((y >= 0) & (y < c)).any()
    # oim_grad_kernel: c % 4 = 0 .. 3; rows past n in the last workgroup or not; lanes past D or not; more than one workgroup
    # along D and along n; both sides of the LDS opt-in; the wrapper's limit itself
    cs, ns, Ds = {c for _, c, _, _, _ in B.OG_CASES}, {n for n, _, _, _, _ in B.OG_CASES}, {D for _, _, D, _, _ in B.OG_CASES}
    assert cs == set(B.OG_C) and ns == set(B.OG_N) and Ds == set(B.OG_D)
    assert {c % 4 for c in cs} == {0, 1, 3}                 # a full last group of four, one class in it, three
    assert {n % 8 == 0 for n in ns} == {True, False} and max(ns) > 16
    assert {D % 256 == 0 for D in Ds} == {True, False} and max(Ds) > 512 and min(Ds) < 256
    assert B.og_lds_bytes(2048) == B.OG_LDS_OPT_IN and B.og_lds_bytes(2049) > B.OG_LDS_OPT_IN
    assert B.og_lds_bytes(B.OG_MAX_C) == 160 * 1024 and B.og_lds_bytes(B.OG_MAX_C + 1) > 160 * 1024
    assert all(n <= 9 for n, c, _, _, _ in B.OG_CASES if c >= 2048)
    assert {e for _, _, _, e, _ in B.OG_CASES} == {0, 3} and {g for _, _, _, _, g in B.OG_CASES} == {True, False}
    # triplet_fwd_kernel: waves with no column, one, more; lanes of the wave with no trip, one, two; triplet_bwd_kernel: threads
    # past D / 4, a second workgroup along D
    w = [B.tri_wave_columns(n) for n in B.TRI_N]
    assert {(0, 1), (1, 1), (1, 2), (2, 3)} <= set(w)
    t = [B.lane_trips(D, 256) for D in B.TRI_D]
    assert {(0, 1), (1, 1), (1, 2)} <= set(t) and max(hi for _, hi in t) > 4
    # (the side without idle threads, D / 4 a multiple of 256, is the model's D = 2048 of test_gpu_train_kernels.py)
    assert all(D // 4 % 256 != 0 for D in B.TRI_D) and min(B.TRI_D) // 4 < 256 < max(B.TRI_D) // 4 < 512
    for n in (4, 5, 9):
        assert len(set(B.tri_ids(n, 'distinct'))) == n and len(set(B.tri_ids(n, 'equal'))) == 1
        cnt = np.unique(B.tri_ids(n, 'singleton'), return_counts=True)[1]
        assert (cnt == 1).any() and (cnt == 2).any()
        assert (np.unique(B.tri_ids(n, 'pairs'), return_counts=True)[1] == 2).any()
    # elementwise kernels of 256 threads: below, at, above one workgroup, two full ones and one item
    assert {m % 256 == 0 for m in B.SM2_M} == {True, False} and min(B.SM2_M) == 1 and max(B.SM2_M) > 512
    # pair_bce_kernel (one workgroup): idle lanes, one, two, three trips
    t = [B.pair_lane_trips(n) for n in B.PAIR_N]
    assert {(0, 1), (1, 1), (1, 2), (2, 3)} <= set(t) and min(B.PAIR_N) == 1
    # scale_dev_kernel: the capped grid's second pass
    assert max(B.SCALE_N) < B.SCALE_GRID_CAP * 256 < B.SCALE_BIG < 2 * B.SCALE_GRID_CAP * 256
    # oim_update_kernel: lanes (stride 1024 floats) with no trip, one, two, three; a label whose first sample is not sample 0
    # and that occurs three times; labels outside the table; a label of the table that never occurs
    t = [B.lane_trips(D, 1024) for D in B.UPD_D]
    assert {(0, 1), (1, 1), (1, 2), (2, 3)} <= set(t)
    assert any(len(l) == 1 for l in B.UPD_LABELS) and any(len(set(l)) == 1 and len(l) == 3 for l in B.UPD_LABELS)
    assert any(l.count(3) == 3 and l.index(1) == 1 and l.count(1) == 2 for l in B.UPD_LABELS)
    assert any(max(l) >= B.UPD_CLASSES_N and min(l) < 0 for l in B.UPD_LABELS)
    assert all(len(set(range(B.UPD_CLASSES_N)) - set(l)) > 0 for l in B.UPD_LABELS)


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pat', B.CE_LABELS)
@pytest.mark.parametrize('n,c,cls', B.CE_CASES)
def test_softmax_ce(n, c, cls, pat):
    for wide, with_w in sorted({f[:2] for f in B.CE_FLAGS}):
        ld, ldd = (c + 3, c + 5) if wide else (c, c)
        d = B.in_softmax_ce(n, c, ld, cls, pat)
        w = d['weight'] if with_w else None
        dz0 = np.full(n * ldd + 7, 12345.0)
        ref = R.softmax_ce(d['logits'], ld, d['labels'], w, n, c, dz0, ldd)
        z = _t(d['logits'].reshape(n, ld)[:, :c], True)
        y = torch.from_numpy(np.where((d['labels'] >= 0) & (d['labels'] < c), d['labels'], IGNORE))
        keep = np.ones(dz0.size, bool)
        keep[(np.arange(n)[:, None] * ldd + np.arange(c)[None, :]).reshape(-1)] = False
        assert (ref['dz'][keep] == 12345.0).all()
        if pat == 'none':                       # torch: nan (0 / 0); the kernels' documented choice: zeros
            assert ref['loss'] == 0.0 and ref['correct'] == 0.0 and not ref['dz_val'].any()
            continue
        loss = TF.cross_entropy(z, y, weight=None if w is None else _t(w), ignore_index=IGNORE)
        scale = (ref['gscale'] * (np.abs(ref['lse']) + np.abs(ref['ty']))).sum()
        _close(ref['loss'], loss, 'loss', scale)
        _close(ref['dz_val'], torch.autograd.grad(loss, z)[0], 'dz', ref['gscale'][:, None] * (ref['p'] + ref['onehot']))
        hit = (z.detach().max(1)[1] == y) & (y != IGNORE)          # torch.max: the first index at the maximum
        assert ref['correct'] == float(hit.sum())
        if cls == 't':                          # the inputs do what they are for: the maximum is attained exactly twice
            assert ((z.detach().numpy() == z.detach().numpy().max(1, keepdims=True)).sum(1) == 2).all()
        # fp32 restatement of the reduction order inside the GPU file's bounds
        f = B.softmax_ce_f32(d['logits'], ld, d['labels'], w, n, c)
        bd = B.b_softmax_ce(ref, n, c)
        B.check('softmax_ce rows', f['rows'], ref['rows'], bd['rows'], (n, c, cls, pat))
        B.check('softmax_ce loss', f['loss'], ref['loss'], bd['loss'], (n, c, cls, pat))
        B.check('softmax_ce dz', f['dz'], ref['dz_val'], bd['dz'], (n, c, cls, pat))


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('n,c,D,ex,with_g', B.OG_CASES)
def test_oim_grad(n, c, D, ex, with_g, cls):
    d = B.in_oim_grad(n, c, D, c + ex, cls)
    g = d['g'] if with_g else None
    ref = R.oim_grad(d['dl'], c + ex, d['lut'], g, d['alpha'], n, c, D)
    dl = _t(d['dl'].reshape(n, c + ex)[:, :c])
    want = (d['alpha'] * (float(d['g'][0]) if with_g else 1.0)) * (dl @ _t(d['lut']))
    _close(ref['dx'], want, 'dx', ref['abs_dx'])
    if c * n * D <= 2048 * 8 * 257:
        B.check('oim_grad dx', B.oim_grad_f32(d['dl'], c + ex, d['lut'], g, d['alpha'], n, c, D), ref['dx'], B.b_oim_grad(ref, c),
                (n, c, D, cls))


def _torch_triplet(f, ids, soft, margin32):
    """the plain expression of test_triplet_forward_backward"""
    n = f.shape[0]
    diff = f.unsqueeze(1) - f.unsqueeze(0)
    dist = (diff.pow(2).sum(2) + 1e-12).sqrt()
    same = ids.unsqueeze(1).eq(ids.unsqueeze(0))
    pos = same & ~torch.eye(n, dtype=torch.bool)
    z = (dist * pos.double()).max(1)[0] - (dist + 1e5 * same.double()).min(1)[0]
    return dist, (TF.softplus(z) if soft else torch.clamp(z + float(margin32), min=0))


@pytest.mark.parametrize('margin', B.TRI_MARGINS)
@pytest.mark.parametrize('pattern', B.TRI_IDS)
@pytest.mark.parametrize('n,D', B.TRI_CASES)
def test_triplet(n, D, pattern, margin):
    soft, m32 = margin == 'soft', np.float32(0.0 if margin == 'soft' else margin)
    for cls in B.TRI_CLASSES:
        d = B.in_triplet(n, D, cls, pattern)
        full = R.triplet_full(d['f'], d['ids'], n, D, soft, m32, d['dloss'])
        f = _t(d['f'], True)
        dist, loss = _torch_triplet(f, torch.from_numpy(d['ids']), soft, m32)
        _close(full['dist'], dist, 'dist')
        # z = vp - vn is a difference: its float64 noise is relative to |vp| + |vn|
        _close(full['loss'], loss, 'loss', np.abs(full['vp']) + np.abs(full['vn']))
        e_dist = B.e_tri_dist(full, D)
        if cls != 't':                          # with exact ties torch's backward of max / min need not pick the first index
            grad = torch.autograd.grad(loss, f, _t(d['dloss']))[0]
            # the quotient (f_i - f_o) / d loses what the subtraction of nearly equal rows loses: relative to |f| / d
            _close(full['df'], grad, 'df', full['abs_df'])
        d32 = B.triplet_dist_f32(d['f'], n, D)
        B.check('triplet dist', d32, full['dist'], B.b_tri_dist(full, D), (n, D, cls, pattern))
        if cls == 'a':
            # the condition under which the GPU file compares the kernel's selection with the float64 one -- never skipped
            assert B.tri_gap_ok(full, e_dist, None if soft else m32), (n, D, pattern, margin)
            s = R.triplet_select(d32, d['ids'], n, soft, m32)
            assert np.array_equal(s['sel'], full['sel'])
            B.check('end to end triplet loss', s['loss'], full['loss'],
                    B.SAFETY * B.e_tri_loss(full['z'], soft, m32, B.e_tri_z(full, e_dist)), (n, D, pattern))
            bw = R.triplet_bwd(d['f'], d32, s['sel'], s['z'], d['dloss'], soft, m32, n, D)
            _close(bw['df'], R.triplet_bwd(d['f'], d32.astype(np.float64), full['sel'], s['z'], d['dloss'], soft, m32, n, D)['df'], 'bwd')
        if cls == 't' and n >= 3 and pattern in ('equal', 'distinct'):
            s = R.triplet_select(d32, d['ids'], n, soft, m32)
            assert d32[2, 0] == d32[2, 1]       # rows 0 and 1 are duplicates: two candidates of anchor 2 tie bit for bit
            assert s['sel'][4] != 1 and s['sel'][5] != 1        # ... and the later of the two never wins


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('m', B.SM2_M)
def test_softmax2_and_bwd(m, cls):
    d = B.in_softmax2(m, cls)
    ref = R.softmax2(d['scores'], m)
    s = _t(d['scores'], True)
    p = TF.softmax(s, dim=-1)
    _close(ref['p'], p[:, 1], 'p'); _close(ref['p0'], p[:, 0], 'p0')
    g = torch.autograd.grad(p[:, 1], s, _t(d['dp']))[0]
    bw = R.softmax2_bwd(ref['p'], ref['p0'], d['dp'], m)
    _close(bw['ds'], g, 'ds', np.abs(bw['g'] * ref['p'])[:, None])
    ea, eb = np.exp(np.float32(ref['ta'])).astype(np.float32), np.exp(np.float32(ref['tb'])).astype(np.float32)
    B.check('softmax2 prob', eb / (ea + eb), ref['p'], B.b_softmax2(ref)['p'], (m, cls))


@pytest.mark.parametrize('cls', B.PAIR_CLASSES)
@pytest.mark.parametrize('n', B.PAIR_N)
def test_pair_bce(n, cls):
    d = B.in_pair(n, cls)
    ref = R.pair_bce(d['prob'], d['tp'], d['tg'], n)
    s64 = d['prob'].astype(np.float64)
    y = (d['tp'][None, :] == d['tg'][:, None]).astype(np.float64)
    if cls == 'a':
        s = _t(s64, True)
        loss = TF.binary_cross_entropy(s, _t(y))
        _close(ref['loss'], loss, 'loss', np.abs(ref['term']).sum() / (n * n))
        _close(ref['dprob'], torch.autograd.grad(loss, s)[0], 'dprob')
    else:
        # the clamped closed form at the edges, element by element
        vals = set(np.unique(d['prob']).tolist())
        if n >= 15:                             # every edge value under y = 0 and under y = 1
            assert vals == set(np.float32(B.PAIR_EDGE).tolist())
            for v in np.float32(B.PAIR_EDGE):
                assert ((d['prob'] == v) & (y == 0)).any() and ((d['prob'] == v) & (y == 1)).any(), v
        tot = 0.0
        for a in range(n):
            for b in range(n):
                v, t = s64[a, b], y[a, b]
                lg = (np.log(v) if v > 0 else -np.inf) if t else (np.log1p(-v) if v < 1 else -np.inf)
                tot -= max(lg, -100.0)
                want = (v - t) / max((1.0 - v) * v, 1e-12) / (n * n)
                assert abs(ref['dprob'][a, b] - want) <= TOL * abs(want)
        _close(ref['loss'], tot / (n * n), 'loss')
        assert ((d['prob'] == 0.5) & (y == 1)).any() and (n == 1 or ((d['prob'] == 0.5) & (y == 0)).any())
        if n >= 15:
            assert ref['term'].max() == 100.0       # the log clamp is reached ...
            assert ((y == 0) & (d['prob'] == 0.0)).any()        # ... and y * log with y = 0 against log = -100
    dec = (np.float32(d['prob']) > np.float32(1) - np.float32(d['prob']))
    assert ref['hits'] == float((dec == (y > 0)).sum())
    f = B.pair_bce_f32(d['prob'], d['tp'], d['tg'], n)
    bd = B.b_pair_bce(ref, n)
    B.check('pair_bce loss', f['loss'], ref['loss'], bd['loss'], (n, cls))
    B.check('pair_bce dprob', f['dprob'], ref['dprob'], bd['dprob'], (n, cls))


@pytest.mark.parametrize('n', B.SCALE_N + (B.SCALE_BIG_CPU,))
def test_scale_dev(n):
    r = B.rng_for('scale', n)
    x, g = B.normal(r, n, 'a'), B.f32([0.37])
    ref = R.scale_dev(x, g, 20.0, n)
    _close(ref['y'], _t(x) * (20.0 * float(g[0])), 'y')
    B.check('scale_dev', np.float32(20.0) * g[0] * x, ref['y'], B.b_scale_dev(ref), n)


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('momentum', B.UPD_MOMENTA)
@pytest.mark.parametrize('labels', B.UPD_LABELS)
@pytest.mark.parametrize('D', B.UPD_D)
def test_oim_update(D, labels, momentum, cls):
    d = B.in_oim_update(D, labels, momentum, cls)
    ref = R.oim_update(d['lut'], d['x'], d['labels'], len(labels), D, B.UPD_CLASSES_N, momentum)
    lut, x = _t(d['lut']).clone(), _t(d['x'])
    for j, y in enumerate(labels):              # reid/loss/oim.py's loop
        if 0 <= y < B.UPD_CLASSES_N:
            lut[y] = momentum * lut[y] + (1.0 - momentum) * x[j]
            lut[y] = lut[y] / lut[y].norm()
    # the normalised row is a quotient by its norm: an element's absolute terms are the row's largest element (a cancelling
    # blend loses two digits of the sixteen once, in the first replay of its label; later samples do not cancel again)
    _close(ref['lut'], lut, 'lut', np.abs(ref['lut']).max(1, keepdims=True))
    touched = {s['row'] for s in ref['steps']}
    for y in range(B.UPD_CLASSES_N):
        if y not in touched:
            assert np.array_equal(ref['lut'][y], d['lut'][y].astype(np.float64))
    if cls == 'b' and momentum == 0.5:          # the inputs do what they are for: the first blend of a label cancels
        first = ref['steps'][0]
        assert np.sqrt(first['ss']) < 0.05
    f = B.oim_update_f32(d['lut'], d['x'], labels, D, B.UPD_CLASSES_N, momentum)
    bd = B.b_oim_update(ref, D, momentum)
    assert set(bd) == touched
    for y in touched:
        B.check('oim_update', f[y], ref['lut'][y], bd[y], (D, labels, momentum, cls, y))
