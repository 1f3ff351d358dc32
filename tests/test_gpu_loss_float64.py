"""The fp32 loss kernels (loss.hip: OIM cross entropy and its gradients, the batch-hard triplet loss, the pair softmax / BCE,
scale_dev; oim_update_kernel of train_head.hip) against the float64 restatement of tests/loss_ref.py, through the C ABI, on a
real MI355X.

Every comparison is per element against that element's derived bound (tests/loss_bounds.py) -- never a norm over the tensor.
A stage that reads another kernel's fp32 output (the selection reads dist; the triplet backward dist, sel and z; the softmax
backward prob and prob0) is compared with the reference evaluated on those very fp32 values: a stage answers for its own
roundings only; the "end to end" stages then take nothing from the kernels.  Discrete outputs (correct, sel, z, the pair hit
count, zeros on ignored rows, the bits of untouched table rows) are compared exactly, with their fp32 restatement; the one
discrete output compared with a float64 decision -- sel, end to end, class (a) -- is compared under the gap condition that
test_loss_ref_cpu.py asserts for every such case.

Every output lives in a buffer filled with a sentinel that is longer (and, with ldd > c, wider) than the kernel may write;
the buffers, helpers and conventions are those of test_gpu_head_float64.py."""
import numpy as np
import pytest
import torch

import loss_bounds as B
import loss_ref as R
from test_gpu_head_float64 import SENT, GUARD, _call, _n, _f, _out, _got, _window, _Inputs, _err

pytestmark = pytest.mark.gpu

ISENT = -7777


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    yield
    B.dump_ratios('MI355X loss kernels')


class _Ints(object):
    """integer inputs (int64 labels / ids) on the device; `unchanged()` after the launches"""

    def __init__(self, a, dtype=torch.int64):
        self.h = np.ascontiguousarray(a)
        self.t = torch.from_numpy(self.h.copy()).to(dtype).cuda()

    def unchanged(self):
        torch.cuda.synchronize()
        assert np.array_equal(_n(self.t), self.h), 'an integer input was written'


def _untouched(t):
    torch.cuda.synchronize()
    assert (_n(t) == SENT).all(), 'an output behind a NULL pointer / of a rejected call was written'


# ----------------------------------------------------------------------------------------------------------------------
# OIM
@pytest.mark.parametrize('n,c,cls', B.CE_CASES)
def test_softmax_ce(n, c, cls):
    """grl_softmax_ce over the three label patterns x sixteen launches (CE_FLAGS: ld / ldd wider than c, weight, dlogits and
    correct present or NULL): loss, the row losses and hits of the workspace, correct, dz through ldd."""
    for pat in B.CE_LABELS:
        for wide, with_w, with_dz, with_cor in B.CE_FLAGS:
            ld, ldd = (c + 3, c + 5) if wide else (c, c)
            d = B.in_softmax_ce(n, c, ld, cls, pat)
            t, lab = _Inputs(logits=d['logits'], weight=d['weight']), _Ints(d['labels'])
            loss, cor, ws, dz = _out(1), _out(1), _out(2 * n), _out(n * ldd)
            _call('grl_softmax_ce', t['logits'], ld, lab.t, t['weight'] if with_w else None, n, c, loss, cor if with_cor else None,
                  dz if with_dz else None, ldd, ws)
            dz0 = np.full(n * ldd, SENT, np.float32)
            ref = R.softmax_ce(d['logits'], ld, d['labels'], d['weight'] if with_w else None, n, c, dz0, ldd)
            bd = B.b_softmax_ce(ref, n, c)
            what = (n, c, cls, pat, wide, with_w, with_dz, with_cor)
            rows = _got(ws, 2 * n)
            assert np.array_equal(rows[n:], ref['hits']), what
            assert (rows[:n][~ref['ok']] == 0).all(), what
            B.check('softmax_ce rows', rows[:n], ref['rows'], bd['rows'], what)
            got = _got(loss, 1)[0]
            if pat == 'none':
                assert got == 0.0 and ref['loss'] == 0.0, what
            B.check('softmax_ce loss', got, ref['loss'], bd['loss'], what)
            if with_cor:
                assert _got(cor, 1)[0] == ref['correct'], what
            else:
                _untouched(cor)
            if with_dz:
                win = _window(_got(dz, n * ldd), n, c, ldd, dz0)
                assert (win[~ref['ok']] == 0).all(), what
                B.check('softmax_ce dz', win, ref['dz_val'], bd['dz'], what)
            else:
                _untouched(dz)
            t.unchanged(); lab.unchanged()


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('n,c,D,ex,with_g', B.OG_CASES)
def test_oim_grad(n, c, D, ex, with_g, cls):
    """grl_oim_grad: dl read through ldd (the columns past c hold 1e30), c padded to four in LDS, rows past n and lanes past D
    guarded, the opted-in LDS size from c = 2049 to the wrapper's limit 5120."""
    d = B.in_oim_grad(n, c, D, c + ex, cls)
    t = _Inputs(dl=d['dl'], lut=d['lut'], g=d['g'])
    dx = _out(n * D)
    _call('grl_oim_grad', t['dl'], c + ex, t['lut'], t['g'] if with_g else None, _f(d['alpha']), dx, n, c, D)
    ref = R.oim_grad(d['dl'], c + ex, d['lut'], d['g'] if with_g else None, d['alpha'], n, c, D)
    B.check('oim_grad dx', _got(dx, n * D).reshape(n, D), ref['dx'], B.b_oim_grad(ref, c), (n, c, D, ex, with_g, cls))
    t.unchanged()


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('momentum', B.UPD_MOMENTA)
@pytest.mark.parametrize('labels', B.UPD_LABELS)
@pytest.mark.parametrize('D', B.UPD_D)
def test_oim_update(D, labels, momentum, cls):
    """grl_oim_update: the replayed rows inside b_oim_update; every row whose label does not occur, or occurs only out of
    range, keeps its bits."""
    d = B.in_oim_update(D, labels, momentum, cls)
    nc, n = B.UPD_CLASSES_N, len(labels)
    t, lab = _Inputs(x=d['x']), _Ints(d['labels'])
    lut = _out(nc * D, d['lut'])
    _call('grl_oim_update', lut, t['x'], lab.t, n, D, nc, _f(momentum))
    got = _got(lut, nc * D).reshape(nc, D)
    ref = R.oim_update(d['lut'], d['x'], d['labels'], n, D, nc, momentum)
    bd = B.b_oim_update(ref, D, momentum)
    for y in range(nc):
        if y in bd:
            B.check('oim_update', got[y], ref['lut'][y], bd[y], (D, labels, momentum, cls, y))
        else:
            assert np.array_equal(got[y].view(np.uint32), d['lut'][y].view(np.uint32)), 'row %d was written' % y
    t.unchanged(); lab.unchanged()


# ----------------------------------------------------------------------------------------------------------------------
# triplet
def _sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


@pytest.mark.parametrize('pattern', B.TRI_IDS)
@pytest.mark.parametrize('n,D', B.TRI_CASES)
def test_triplet_fwd_and_bwd(n, D, pattern):
    """grl_triplet_fwd: dist inside b_tri_dist; sel and z EQUAL to the fp32 restatement of the selection on the kernel's own
    dist; the loss on the kernel's z.  grl_triplet_bwd on the kernel's own dist / sel / z.  Class (a): the kernel's sel equals
    the float64 selection (gap condition), loss and dfeat end to end."""
    for margin in B.TRI_MARGINS:
        soft, m32 = int(margin == 'soft'), np.float32(0.0 if margin == 'soft' else margin)
        for cls in B.TRI_CLASSES:
            d = B.in_triplet(n, D, cls, pattern)
            t, ids = _Inputs(f=d['f'], dloss=d['dloss']), _Ints(d['ids'])
            loss, dist, z, df = _out(n), _out(n * n), _out(n), _out(n * D)
            sel = torch.full((2 * n + GUARD,), ISENT, dtype=torch.int32, device='cuda')
            _call('grl_triplet_fwd', t['f'], ids.t, n, D, soft, _f(m32), loss, dist, sel, z)
            what = (n, D, pattern, margin, cls)
            dk, zk = _got(dist, n * n).reshape(n, n).copy(), _got(z, n).copy()
            selk = _n(sel)
            assert (selk[2 * n:] == ISENT).all(), 'written past the end of sel'
            selk = selk[:2 * n].copy()
            dref = R.triplet_dist(d['f'], n, D)
            B.check('triplet dist', dk, dref['dist'], B.b_tri_dist(dref, D), what)
            s = R.triplet_select(dk, d['ids'], n, soft, m32)
            assert np.array_equal(selk, s['sel']), what
            assert np.array_equal(zk, s['z']), what
            B.check('triplet loss', _got(loss, n), s['loss'], B.SAFETY * B.e_tri_loss(zk, soft, m32), what)
            assert zk.max() < 80                # expf(z) in the backward stays finite
            _call('grl_triplet_bwd', t['f'], dist, sel, z, t['dloss'], soft, _f(m32), df, n, D)
            dfk = _got(df, n * D).reshape(n, D)
            bw = R.triplet_bwd(d['f'], dk, selk, zk, d['dloss'], soft, m32, n, D)
            B.check('triplet dfeat', dfk, bw['df'], B.b_tri_bwd(bw, soft), what)
            if cls == 'a':
                full = R.triplet_full(d['f'], d['ids'], n, D, soft, m32, d['dloss'])
                e_dist = B.e_tri_dist(full, D)
                assert B.tri_gap_ok(full, e_dist, None if soft else m32), what        # (test_loss_ref_cpu asserts it too)
                assert np.array_equal(selk, full['sel']), what
                e_z = B.e_tri_z(full, e_dist)
                B.check('end to end triplet loss', _got(loss, n), full['loss'], B.SAFETY * B.e_tri_loss(full['z'], soft, m32, e_z), what)
                sg = _sigmoid(full['z'])
                e_gz = np.abs(d['dloss']) * sg * (1.0 - sg) * e_z if soft else np.zeros(n)
                B.check('end to end triplet dfeat', dfk, full['df'],
                        B.b_tri_bwd(full, soft, e_gz, e_dist, full['dist'], full['sel']), what)
            assert np.array_equal(_got(dist, n * n).reshape(n, n), dk) and np.array_equal(_got(z, n), zk)
            assert np.array_equal(_n(sel)[:2 * n], selk) and (_n(sel)[2 * n:] == ISENT).all()
            t.unchanged(); ids.unchanged()


# ----------------------------------------------------------------------------------------------------------------------
# pair verification
@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('m', B.SM2_M)
def test_softmax2_and_bwd(m, cls):
    """grl_softmax2 with and without prob0; grl_softmax2_bwd on the kernel's own prob / prob0, and end to end."""
    d = B.in_softmax2(m, cls)
    t = _Inputs(scores=d['scores'], dp=d['dp'])
    ref = R.softmax2(d['scores'], m)
    bd = B.b_softmax2(ref)
    for with_p0 in (False, True):
        p, p0 = _out(m), _out(m)
        _call('grl_softmax2', t['scores'], p, p0 if with_p0 else None, m)
        B.check('softmax2 prob', _got(p, m), ref['p'], bd['p'], (m, cls, with_p0))
        if with_p0:
            B.check('softmax2 prob0', _got(p0, m), ref['p0'], bd['p0'], (m, cls))
        else:
            _untouched(p0)
    pk, p0k = _got(p, m).copy(), _got(p0, m).copy()
    ds = _out(2 * m)
    _call('grl_softmax2_bwd', p, p0, t['dp'], ds, m)
    bw = R.softmax2_bwd(pk, p0k, d['dp'], m)
    got = _got(ds, 2 * m).reshape(m, 2)
    B.check('softmax2_bwd dscores', got, bw['ds'], B.b_softmax2_bwd(bw), (m, cls))
    e2e = R.softmax2_bwd(ref['p'], ref['p0'], d['dp'], m)
    e = B.e_softmax2(ref)
    B.check('end to end softmax2 dscores', got, e2e['ds'], B.b_softmax2_bwd(e2e, e['p'], e['p0']), (m, cls))
    assert np.array_equal(_got(p, m), pk) and np.array_equal(_got(p0, m), p0k)
    t.unchanged()


@pytest.mark.parametrize('cls', B.PAIR_CLASSES)
@pytest.mark.parametrize('n', B.PAIR_N)
def test_pair_bce(n, cls):
    """grl_pair_bce with prec and dprob each present and NULL: the loss, dprob, prec inside its bound and the hit count it
    encodes EQUAL to the count of the fp32 decisions."""
    d = B.in_pair(n, cls)
    t, tp, tg = _Inputs(prob=d['prob']), _Ints(d['tp']), _Ints(d['tg'])
    ref = R.pair_bce(d['prob'], d['tp'], d['tg'], n)
    bd = B.b_pair_bce(ref, n)
    for with_prec in (True, False):
        for with_dp in (True, False):
            loss, prec, dp = _out(1), _out(1), _out(n * n)
            _call('grl_pair_bce', t['prob'], tp.t, tg.t, n, loss, prec if with_prec else None, dp if with_dp else None)
            what = (n, cls, with_prec, with_dp)
            B.check('pair_bce loss', _got(loss, 1)[0], ref['loss'], bd['loss'], what)
            if with_prec:
                got = float(_got(prec, 1)[0])
                assert round(got * n * n) == ref['hits'], what
                B.check('pair_bce prec', got, ref['prec'], bd['prec'], what)
            else:
                _untouched(prec)
            if with_dp:
                B.check('pair_bce dprob', _got(dp, n * n).reshape(n, n), ref['dprob'], bd['dprob'], what)
            else:
                _untouched(dp)
    t.unchanged(); tp.unchanged(); tg.unchanged()


@pytest.mark.parametrize('n', B.SCALE_N + (B.SCALE_BIG,))
def test_scale_dev(n):
    """grl_scale_dev; the last case is just over 4096 x 256 items: the grid is capped and the stride loop's second pass runs"""
    r = B.rng_for('scale', n)
    x, g = B.normal(r, n, 'a'), B.f32([0.37])
    t = _Inputs(x=x, g=g)
    y = _out(n)
    _call('grl_scale_dev', t['x'], t['g'], _f(20.0), y, n)
    ref = R.scale_dev(x, g, 20.0, n)
    B.check('scale_dev', _got(y, n), ref['y'], B.b_scale_dev(ref), n)
    t.unchanged()


# ----------------------------------------------------------------------------------------------------------------------
def test_rejected_arguments_launch_nothing():
    """What the wrappers reject raises GrlHipError and leaves every sentinel output intact; the neighbouring good arguments
    (5120 classes, D = 4) are then accepted."""
    Err = _err()
    a = torch.ones(5120 * 4, device='cuda')
    li = torch.zeros(64, dtype=torch.int64, device='cuda')
    si = torch.full((64,), ISENT, dtype=torch.int32, device='cuda')
    outs = [_out(1024) for _ in range(4)]
    o0, o1, o2, o3 = outs
    f1 = _f(1.0)
    bad = [
        # softmax_ce(logits, ld, labels, weight, n, c, loss, correct, dlogits, ldd, ws)
        ('grl_softmax_ce', (a, 7, li, None, 2, 8, o0, o1, o2, 8, o3)), ('grl_softmax_ce', (a, 8, li, None, 2, 8, o0, o1, o2, 7, o3)),
        ('grl_softmax_ce', (a, 8, li, None, 0, 8, o0, o1, o2, 8, o3)), ('grl_softmax_ce', (a, 8, li, None, 2, 0, o0, o1, o2, 8, o3)),
        ('grl_softmax_ce', (a, 8, li, None, 2, 8, None, o1, o2, 8, o3)), ('grl_softmax_ce', (a, 8, li, None, 2, 8, o0, o1, o2, 8, None)),
        ('grl_softmax_ce', (a, 8, None, None, 2, 8, o0, o1, o2, 8, o3)),
        # oim_grad(dlogits, ldd, lut, g, alpha, dx, n, c, D)
        ('grl_oim_grad', (a, 5121, a, None, f1, o0, 1, 5121, 4)), ('grl_oim_grad', (a, 7, a, None, f1, o0, 2, 8, 4)),
        ('grl_oim_grad', (a, 8, a, None, f1, o0, 2, 8, 0)),
        # triplet_fwd(feat, ids, n, D, soft, margin, loss, dist, sel, z) / triplet_bwd(feat, dist, sel, z, dloss, soft, margin, dfeat, n, D)
        ('grl_triplet_fwd', (a, li, 2, 6, 1, f1, o0, o1, si, o2)), ('grl_triplet_fwd', (a, li, 0, 8, 1, f1, o0, o1, si, o2)),
        ('grl_triplet_fwd', (a, li, 16385, 8, 1, f1, o0, o1, si, o2)),
        ('grl_triplet_bwd', (a, a, si, a, a, 1, f1, o0, 2, 6)),
        # softmax2(scores, prob, prob0, m) / softmax2_bwd(prob, prob0, dprob, dscores, m)
        ('grl_softmax2', (a, o0, o1, 0)), ('grl_softmax2', (None, o0, o1, 4)), ('grl_softmax2', (a, None, o1, 4)),
        ('grl_softmax2_bwd', (a, a, a, o0, 0)), ('grl_softmax2_bwd', (a, None, a, o0, 4)), ('grl_softmax2_bwd', (a, a, a, None, 4)),
        # pair_bce(prob, tar_probe, tar_gallery, n, loss, prec, dprob)
        ('grl_pair_bce', (a, li, li, 0, o0, o1, o2)), ('grl_pair_bce', (a, li, li, 4097, o0, o1, o2)),
        # scale_dev(x, g, alpha, y, n)
        ('grl_scale_dev', (a, a, f1, o0, 0)), ('grl_scale_dev', (a, None, f1, o0, 4)),
        # oim_update(lut, x, labels, n, D, num_classes, momentum)
        ('grl_oim_update', (o0, a, li, 2, 6, 6, _f(0.5))), ('grl_oim_update', (o0, a, li, 2, 8, 0, _f(0.5))),
    ]
    for name, args in bad:
        with pytest.raises(Err):
            _call(name, *args)
    torch.cuda.synchronize()
    for o in outs:
        assert (_n(o) == SENT).all(), 'a rejected call wrote to an output'
    assert (_n(a) == 1.0).all() and (_n(si) == ISENT).all() and (_n(li) == 0).all()
    # ... and the same entry points accept the neighbouring good arguments
    _call('grl_oim_grad', a, 5120, a, None, f1, o0, 1, 5120, 4)
    _call('grl_triplet_fwd', a, li, 2, 4, 1, f1, o1, o2, si, o3)
    lut = _out(24, np.ones(24, np.float32))
    _call('grl_oim_update', lut, a, li, 1, 4, 6, _f(0.5))
    torch.cuda.synchronize()
    assert (_n(o0)[:4] == 5120.0).all() and (_n(o0)[4:] == SENT).all()
    assert (_n(o1)[:2] != SENT).all() and (_n(o1)[2:] == SENT).all()
    assert (np.abs(_n(o2)[:4] - 1e-6) < 1e-9).all() and (_n(o2)[4:] == SENT).all()
    assert (_n(si)[:4] != ISENT).all() and (_n(si)[4:] == ISENT).all()
    assert np.array_equal(_got(lut, 24), np.r_[np.full(4, 0.5), np.ones(20)].astype(np.float32))
