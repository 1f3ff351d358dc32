"""The float64 BatchNorm reference (tests/bn_ref.py) is right, and the bounds of tests/bn_bounds.py are satisfiable --
both shown without a GPU:

* bn_ref against torch float64 BatchNorm1d / BatchNorm2d autograd at every shape of the GPU sweep;
* an fp32 numpy restatement of the kernels' own summation order (fp32 partials of at most 128 rows, fp64 across them)
  against bn_ref inside the very bounds the GPU tests hold the kernels to, for every input of that sweep."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import bn_bounds as B
import bn_ref as R

EPS = 1e-5


MAX_TOL = {}                    # input class -> largest relative tolerance test_reference_matches_torch_float64 used


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    yield
    B.dump_ratios('fp32 numpy restatement (CPU)')
    print('bn_ref vs torch float64: largest relative tolerance used per input class: %s' % (
        ', '.join('%s %.2e' % kv for kv in sorted(MAX_TOL.items()))))


def _tol_rel(z, mean, var):
    """Both sides are float64.  1e-12 relative, except where the data themselves make z - mean ill conditioned: the operands
    of that subtraction carry 2^-53 relative each, which the difference sees amplified by cond = (max |z| + |mean|) / std;
    8 roundings of that size reach an output (two operands, the mean's own rounding, var and invstd through the squares,
    the products after them).  Classes (a) and (c) have cond < 20 once there are enough rows and stay at 1e-12."""
    cond = (np.abs(z).max(0) + np.abs(mean)) / np.sqrt(var + EPS) + 1.0
    return np.maximum(1e-12, 8 * B.U64 * cond)


def _close(got, ref, tol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bad = np.abs(got - ref) > tol
    assert not bad.any(), (what, float(np.abs(got - ref).max()), int(bad.sum()))


def _torch_bn(C, dims, gamma, beta, rm, rv, momentum):
    bn = (nn.BatchNorm1d if dims == 1 else nn.BatchNorm2d)(C, eps=EPS, momentum=momentum).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(R.f64(gamma))); bn.bias.copy_(torch.from_numpy(R.f64(beta)))
        bn.running_mean.copy_(torch.from_numpy(R.f64(rm))); bn.running_var.copy_(torch.from_numpy(R.f64(rv)))
    return bn


def _torch_forward(bn, z, dims):
    """z[M][C] through the module: BatchNorm1d on [M][C], BatchNorm2d on [1][C][M][1] (rows are pixels)."""
    M, C = z.shape
    x = z if dims == 1 else z.t().reshape(1, C, M, 1)
    if M == 1:
        # the modules refuse one value per channel in training mode; the native op does not
        y = torch.batch_norm(x, bn.weight, bn.bias, None, None, True, bn.momentum, bn.eps, False)
    else:
        y = bn(x)
    return y if dims == 1 else y.reshape(C, M).t()


@pytest.mark.parametrize('dims', [1, 2])
@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('M,C', B.SHAPES)
def test_reference_matches_torch_float64(M, C, cls, dims):
    d = B.make_inputs(M, C, cls)
    z64 = R.f64(d['z'])
    st = R.stats(z64, pivot=z64[0])
    tol = _tol_rel(z64, st['mean'], st['var'])
    MAX_TOL[cls] = max(MAX_TOL.get(cls, 0.0), float(tol.max()))
    if cls != 'b' and M >= 127:                     # (a handful of rows can have a small variance by chance)
        assert (tol == 1e-12).all()
    # the allowance has a ceiling that follows from the inputs: |z| + |mean| <= 2 * 1.5e3 + spread over std >= sqrt(eps)
    # (class (b)'s constant channel) is cond < 1e6, so 8 * 2^-53 * cond < 1e-9; classes (a) / (c) stay below 1e-10
    assert tol.max() < (1e-9 if cls == 'b' else 1e-10)
    # the pivot changes the sums, not the statistics
    st0 = R.stats(z64)
    _close(st0['mean'], st['mean'], 1e-15 * (np.abs(z64).max(0) + 1e-300), 'mean with / without pivot')
    _close(st0['var'], st['var'], tol * (st['var'] + 1e-300), 'var with / without pivot')
    _close(st['sum_d'] / M + z64[0], st['mean'], 1e-13 * np.abs(z64).max(0), 'mean from the pivoted sum')
    for momentum in (0.1, 0.5):
        fin = R.finalize(st['mean'], st['var'], M, d['gamma'], d['beta'], d['rm'], d['rv'], momentum, EPS)
        for res_on in (False, True):
            for relu in (False, True):
                res = d['res'] if res_on else None
                if cls == 'c' and res_on:           # half of the pre-activations a few fp32 ulp from zero
                    res, _ = B.near_zero_residual(d['z'], st['mean'].astype(np.float32), fin['scale'].astype(np.float32),
                                                  d['beta'], d['res'])
                bn = _torch_bn(C, dims, d['gamma'], d['beta'], d['rm'], d['rv'], momentum)
                zt = torch.from_numpy(z64).requires_grad_(True)
                rt = None if res is None else torch.from_numpy(R.f64(res)).requires_grad_(True)
                yt = _torch_forward(bn, zt, dims)
                yt = yt if rt is None else yt + rt
                yt = torch.relu(yt) if relu else yt
                yt.backward(torch.from_numpy(R.f64(d['dy'])))
                fw = R.apply_centered(z64, st['mean'], fin['scale'], d['beta'], res, relu)
                what = (M, C, cls, dims, momentum, res_on, relu)
                # z - mean is off by 2^-53 (|z| + |mean|) ABSOLUTE on either side (dx below: 8 such roundings, times
                # invstd), whatever is left of the difference -- that term does not shrink with |z - mean|
                dx = 8 * B.U64 * (np.abs(z64).max(0) + np.abs(st['mean'])) * fin['invstd']
                _close(fw['y'], yt.detach().numpy(), tol[None, :] * fw['abs_terms'] + (dx * np.abs(R.f64(d['gamma'])))[None, :],
                       ('y',) + what)
                if M > 1:
                    _close(fin['running_mean'], bn.running_mean.numpy(), 1e-12 * (np.abs(d['rm']) + np.abs(z64).max(0)),
                           ('running_mean',) + what)
                    _close(fin['running_var'], bn.running_var.numpy(), tol * np.abs(fin['running_var']),
                           ('running_var',) + what)
                else:
                    # count == 1: no unbiased estimate exists; the reference keeps the biased variance (0)
                    assert (st['var'] == 0).all() and (fin['unbiased'] == 0).all()
                    _close(fin['running_var'], (1 - momentum) * R.f64(d['rv']), 1e-15 * np.abs(d['rv']), 'count == 1')
                # the mask is read off the OTHER side's y, as the GPU tests read it off the kernel's: an element within
                # the y tolerance of zero may legitimately fall on either side
                mask = yt.detach().numpy() > 0
                near = np.abs(fw['pre']) <= tol[None, :] * fw['abs_terms'] + (dx * np.abs(R.f64(d['gamma'])))[None, :]
                assert not relu or ((mask == fw['mask']) | near).all()
                bw = R.backward(d['dy'], z64, mask if relu else None, st['mean'], fin['invstd'], d['gamma'])
                mg = bw['abs_g'] / M
                _close(bw['dz'], zt.grad.numpy(), tol[None, :] * bw['abs_terms'] + np.abs(bw['gm'])[None, :] * dx[None, :] * (
                    np.abs(bw['sum_gx'] / M)[None, :] + (np.abs(bw['xhat']) + 1) * mg[None, :]), ('dz',) + what)
                _close(bw['dgamma'], bn.weight.grad.numpy(), tol * bw['abs_gx'] + dx * bw['abs_g'] + 1e-300, ('dgamma',) + what)
                _close(bw['dbeta'], bn.bias.grad.numpy(), 1e-12 * bw['abs_g'] + 1e-300, ('dbeta',) + what)
                if rt is not None:
                    assert np.array_equal(bw['g'], rt.grad.numpy())


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('M,C', B.SHAPES)
def test_reference_statistics_against_extended_precision(M, C, cls):
    """bn_ref.stats' mean and two-pass variance against the same sums in numpy's long double (extended precision on x86), to 1e-12 relative in EVERY
    class -- ill conditioned (b) included, where the tolerance of the torch comparison has to give: a one-pass
    E[x^2] - E[x]^2 in float64 would miss this by ~1e-6 there."""
    z = R.f64(B.make_inputs(M, C, cls)['z'])
    zl = z.astype(np.longdouble)
    ml = zl.mean(0)
    vl = ((zl - ml[None, :]) ** 2).mean(0)
    for pivot in (None, z[0]):
        st = R.stats(z, pivot)
        _close(st['mean'], ml.astype(np.float64), 1e-15 * np.abs(z).max(0) + 1e-300, ('mean', M, C, cls))
        _close(st['var'], vl.astype(np.float64), 1e-12 * vl.astype(np.float64) + 1e-300, ('var', M, C, cls))


@pytest.mark.parametrize('M,C', [(2, 12), (7, 132), (129, 68), (513, 64)])
def test_reference_running_statistics_after_three_steps(M, C):
    for momentum in (0.1, 0.5):
        d = B.make_inputs(M, C, 'a')
        bn = _torch_bn(C, 1, d['gamma'], d['beta'], d['rm'], d['rv'], momentum)
        rm, rv = R.f64(d['rm']), R.f64(d['rv'])
        for step in range(3):
            z = R.f64(B.make_inputs(M, C, 'a', seed=step)['z'])
            bn(torch.from_numpy(z))
            st = R.stats(z, pivot=z[0])
            fin = R.finalize(st['mean'], st['var'], M, d['gamma'], d['beta'], rm, rv, momentum, EPS)
            rm, rv = fin['running_mean'], fin['running_var']
        _close(rm, bn.running_mean.numpy(), 1e-12 * np.abs(rm) + 1e-14, 'running_mean x3')
        _close(rv, bn.running_var.numpy(), 1e-12 * np.abs(rv), 'running_var x3')
        assert int(bn.num_batches_tracked) == 3


def test_sweep_takes_both_branches_of_the_apply_kernels():
    fast = [B.apply_takes_fast_branch(M, C) for M, C in B.SHAPES]
    assert any(fast) and not all(fast)
    assert set(M for M, _ in B.SHAPES) == set(B.M_LIST) and set(C for _, C in B.SHAPES) == set(B.C_LIST)
    for M in B.M_LIST:
        assert sum(1 for m, _ in B.SHAPES if m == M) >= 3
    for C in B.C_LIST:
        assert sum(1 for _, c in B.SHAPES if c == C) >= 3
    assert (4 * 128 + 1, 260) in B.SHAPES


@pytest.mark.parametrize('cls', B.CLASSES)
@pytest.mark.parametrize('M,C', B.SHAPES)
def test_fp32_restatement_of_the_kernels_stays_inside_the_bounds(M, C, cls):
    """What the GPU tests will ask of the kernels, asked of a numpy fp32 program with the kernels' summation order."""
    d = B.make_inputs(M, C, cls)
    z = d['z']
    for pivot in (None, z[0]):
        slab = B.col_stats_f32(z, pivot)
        for ch in range(B.chunks(M)):
            st = R.stats(z[ch * 128:(ch + 1) * 128], pivot)
            B.check('col_stats sum', slab[ch, 0], st['sum_d'], B.b_col_sum(st['abs_d'], st['sum_d']))
            B.check('col_stats sumsq', slab[ch, 1], st['sum_d2'], B.b_col_sumsq(st['sq_d'], st['sum_d2']))
    S, Q = R.f64(slab[:, 0]).sum(0), R.f64(slab[:, 1]).sum(0)
    for momentum in (0.1, 0.5):
        mom = float(np.float32(momentum))
        fb = B.finalize_bounds(S, Q, M, z[0], d['gamma'], d['beta'], d['rm'], d['rv'], mom, float(np.float32(EPS)))
        got = B.finalize_f32(S, Q, M, z[0], d['gamma'], d['beta'], d['rm'], d['rv'], momentum, EPS)
        B.check('finalize mean', got['mean'], fb['mu'], fb['mean'])
        for k in ('invstd', 'scale', 'shift', 'running_mean', 'running_var'):
            B.check('finalize ' + k, got[k], fb['ref'][k], fb[k])
    mean, invstd, scale = got['mean'], got['invstd'], got['scale']
    if cls == 'b':
        assert got['invstd'][1] == np.float32(1.0 / np.sqrt(float(np.float32(EPS)))) and got['mean'][1] == 1000.0
    for res_on in (False, True):
        for relu in (False, True):
            zz, res = z, (d['res'] if res_on else None)
            if cls == 'c':
                if res_on:
                    res, _ = B.near_zero_residual(z, mean, scale, d['beta'], d['res'])
                else:
                    zz, _ = B.near_zero_z(z, mean, scale, d['beta'])
            fw = R.apply_centered(zz, mean, scale, d['beta'], res, relu)
            y = B.apply_f32(zz, mean, scale, d['beta'], res, relu)
            B.check('apply y', y, fw['y'], B.b_apply(fw['abs_terms']))
            if cls == 'b':
                want = d['beta'][1] + (res[:, 1] if res_on else np.float32(0))       # y = beta (+ res), exactly
                assert (y[:, 1] == (np.maximum(want, np.float32(0)) if relu else want)).all()
            mask = (y > 0) if relu else None          # the mask the backward acts on is the fp32 one
            bw = R.backward(d['dy'], zz, mask, mean, invstd, d['gamma'])
            slab = B.bwd_reduce_f32(d['dy'], zz, mask, mean, invstd)
            g_ch, gx_ch = B.chunk_sums(bw['g']), B.chunk_sums(bw['g'] * bw['xhat'])
            b_g = B.b_sum_g(B.chunk_sums(np.abs(bw['g'])), g_ch, C)
            b_gx = B.b_sum_gx(B.chunk_sums(np.abs(bw['g'] * bw['xhat'])), gx_ch, C)
            sg, sgx = R.f64(slab[:, 0]).sum(0), R.f64(slab[:, 1]).sum(0)
            B.check('bwd sum g', sg, bw['sum_g'], b_g)
            B.check('bwd sum g xhat', sgx, bw['sum_gx'], b_gx)
            k0, k1 = (sg / M).astype(np.float32), (sgx / M).astype(np.float32)
            dz = B.bwd_apply_f32(d['dy'], zz, mask, mean, invstd, d['gamma'], k0, k1)
            B.check('bwd dz', dz, bw['dz'], B.b_dz(bw, B.b_coef(b_g, bw['sum_g'], M), B.b_coef(b_gx, bw['sum_gx'], M)))
