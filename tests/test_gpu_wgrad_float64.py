"""The weight-gradient kernels of grl_amd/csrc/train.hip -- wgrad_kernel<BM, BN, CONV, MATH> (four tile shapes, three math
modes), wgrad_b16in_kernel, wgrad_b16in_256_kernel, stem_wgrad_kernel and the wgrad_reduce_kernel behind them -- against the
float64 restatement of tests/wgrad_ref.py, on a real MI355X.

Every comparison is per element against that element's derived bound (tests/wgrad_bounds.py), never a norm over the tensor;
where the bound is exactly zero (taps outside the image, everything a tagged pixel does not reach) the value must be exactly
zero, or bit-equal to the preloaded gradient in the accumulate form.  grl_conv_wgrad_f32 and grl_stem_wgrad are called
through their own descriptors, with a workspace of exactly the size the library asks for -- asserted equal to the restated
host rules times N K --, and no environment variable of the project's is set: the natural rules reach every edge of the
sweep (test_wgrad_ref_cpu.py asserts that from the restatements).

Memory hygiene, for every entry and class: each operand sits inside a NaN-filled allocation, the workspace is NaN before
every call (a slab element that is read but was never written shows), 64 sentinel elements behind dw and behind the workspace
are intact afterwards, the inputs are bit-unchanged, and the fresh result is bit-equal on a second call.

Which datapath ran: on general fp32 operands a math = bf16 entry on a 128 x 128 tile misses the exact-fp32 bound; the
fallback entries (math = bf16 / bf16x3 on a 64 x 128 tile) are held to the exact-fp32 bound.

Measured on the MI355X: 85 cases (63 sweep entries, each with every class, fresh twice and accumulating), 3.5 s for the
whole module, the slowest case (the 520-tile stem, 17 MB of dz) 0.66 s, every other one under 0.25 s.  Largest
|error| / bound per stage (SAFETY = 2 the only factor; EXPERIMENTS.md, "float64 anchor of the weight-gradient kernels"):
  f32 dense 0.495, f32 lin 0.491, f32 generic 0.495, f32 small_img 0.469      (the accumulate form's one addition: u |result|
  b16in_128 dense 0.497, conv 0.496; b16in_256 dense 0.500, conv 0.499         against 2 u |result| where a single exact
  stem 0.498, stem with bf16 dz 0.500                                          product arrives)
  bf16x3 dense 0.400, conv 0.464
  bf16 dense 0.955, conv 0.950   (a tagged element is ONE product of two operands rounded to bf16: the charged 2 x 2^-9 times
                                  SAFETY is bf16's first-order worst case, so this stage sits near 1 by construction)"""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

import wgrad_bounds as B

pytestmark = pytest.mark.gpu

SENT = 12288.0
GUARD = 64                      # sentinel elements behind every output, NaN elements around every operand
SLACK = 4096                    # (rejection cases only: room behind dw / the workspace for the shape the bad descriptor names)
BF16 = torch.bfloat16
T0 = [None]
IDS = ['%d-%s' % (i, B.kernel_body(e).split('<')[0]) for i, e in enumerate(B.SWEEP)]


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    T0[0] = time.time()
    yield
    B.dump_ratios('MI355X weight gradient')
    print('  module run time %.1f s' % (time.time() - T0[0]))


def _L():
    from grl_amd import _lib
    return _lib


class _Operand(object):
    """an input inside a NaN-filled allocation: [GUARD NaN | skew | values | GUARD NaN]"""

    def __init__(self, a, b16, skew=0):
        self.lo = GUARD + skew
        self.t = torch.full((self.lo + a.size + GUARD,), float('nan'), device='cuda', dtype=BF16 if b16 else torch.float32)
        self.t[self.lo:self.lo + a.size] = torch.from_numpy(np.array(a, dtype=np.float32).reshape(-1)).cuda().to(self.t.dtype)
        self.was = self.bits()

    def ptr(self):
        return self.t.data_ptr() + self.lo * self.t.element_size()

    def bits(self):
        return self.t.view(torch.int16 if self.t.dtype == BF16 else torch.int32).cpu().numpy()

    def unchanged(self):
        return np.array_equal(self.bits(), self.was)


class _Output(object):
    """n fp32 elements (`init`, or `fill`) with GUARD sentinel elements behind them; `skew` elements in front"""

    def __init__(self, n, init=None, fill=SENT, skew=0):
        self.n, self.lo = n, skew
        self.t = torch.full((skew + n + GUARD,), SENT, device='cuda', dtype=torch.float32)
        self.t[skew:skew + n] = fill
        if init is not None:
            self.t[skew:skew + init.size] = torch.from_numpy(np.array(init, dtype=np.float32).reshape(-1)).cuda()

    def ptr(self):
        return self.t.data_ptr() + 4 * self.lo

    def bits(self):
        torch.cuda.synchronize()
        return self.t.view(torch.int32).cpu().numpy()

    def values(self, shape):
        torch.cuda.synchronize()
        a = self.t.cpu().numpy()
        assert (a[self.lo + self.n:] == SENT).all() and (a[:self.lo] == SENT).all(), 'written outside the output'
        return a[self.lo:self.lo + int(np.prod(shape))].reshape(shape)


@functools.lru_cache(maxsize=None)
def _ref(index, cls):
    """inputs and the float64 reference, computed once and read-only"""
    e = B.SWEEP[index]
    d = B.make_inputs(e, cls)
    out = B.reference(e, d)
    for a in list(d.values()) + list(out):
        a.setflags(write=False)
    return d, out


def _descriptor(e, dz, x, dw, ws, accumulate):
    _lib = _L()
    cv = (0,) * 9
    if e.kind == 'conv':
        n, H, W, Cc, k, stride, pad = e.geom
        Ho, Wo = B.out_hw(e)
        cv = (H, W, Cc, Ho, Wo, k, k, stride, pad)
    return _lib.GrlWgrad(dz, x, dw, ws, e.M, e.N, e.K, e.ldz, e.K if e.kind == 'conv' else e.ldx, e.k_out, accumulate,
                         1 if e.kind == 'conv' else 0, *(cv + (e.math, e.b16)))


def _workspace_floats(e, desc=None):
    """what the library asks for -- and that it is what the restated host rules say"""
    lib = _L().load()
    if e.kind == 'stem':
        asked = int(lib.grl_stem_wgrad_workspace_floats(*e.geom))
    else:
        asked = int(lib.grl_wgrad_workspace_floats(C.byref(desc if desc is not None else _descriptor(e, 0, 0, 0, 0, 0))))
    assert asked == B.workspace_floats(e), (e, asked, B.workspace_floats(e))
    if e.kind != 'stem':
        assert asked == B.wgrad_splits(e) * e.N * e.K and B.wgrad_splits(e) >= B.real_splits(e)
    return asked


def _launch(e, dz, x, dw, ws, accumulate):
    _lib = _L()
    lib = _lib.load()
    if e.kind == 'stem':
        n, H, W = e.geom
        _lib.check(lib.grl_stem_wgrad(x.ptr(), dz.ptr(), e.b16, dw.ptr(), ws.ptr(), n, H, W, accumulate, _lib.stream()),
                   'grl_stem_wgrad')
    else:
        d = _descriptor(e, dz.ptr(), x.ptr(), dw.ptr(), ws.ptr(), accumulate)
        _lib.check(lib.grl_conv_wgrad_f32(C.byref(d), _lib.stream()), 'grl_conv_wgrad_f32')


def _stage(e):
    p = B.datapath(e)
    if p == 'stem':
        return 'stem, bf16 dz' if e.b16 else 'stem'
    return '%s %s' % (p, B.conv_path(e) or e.kind)


def _run_class(index, cls):
    """one entry and class: fresh twice, then accumulating; returns the fresh result"""
    e = B.SWEEP[index]
    d, (ref, ab, terms) = _ref(index, cls)
    dz = _Operand(d['dz'], bool(e.b16))
    x = _Operand(d['x'], bool(e.b16) and e.kind != 'stem')
    nws = _workspace_floats(e)
    fresh = []
    for accumulate in (0, 0, 1):
        ws = _Output(nws, fill=float('nan'))
        dw = _Output(ref.size, init=d['g0'] if accumulate else None)
        _launch(e, dz, x, dw, ws, accumulate)
        got = dw.values(ref.shape)
        ws.values((0,))
        want = ref + d['g0'].astype(np.float64) if accumulate else ref
        what = (index, e.why, cls, 'accumulate' if accumulate else 'fresh')
        bound = B.bound(e, ab, terms, want, accumulate)
        B.check(_stage(e), got, want, bound, what)
        exact = bound == 0                      # no term arrives: exactly zero, or the preload bit for bit
        assert np.array_equal(got[exact], want[exact].astype(np.float32)), what
        if not accumulate:
            fresh.append(got.copy())
    assert np.array_equal(fresh[0].view(np.int32), fresh[1].view(np.int32)), 'the second call differs'
    assert dz.unchanged() and x.unchanged(), 'an input was written'
    return fresh[0]


@pytest.mark.parametrize('index', range(len(B.SWEEP)), ids=IDS)
def test_weight_gradient_per_element(index):
    e = B.SWEEP[index]
    for cls in B.classes(e):
        got = _run_class(index, cls)
        if cls == 'a' and e.math == B.MATH_BF16 and not e.b16:
            # which datapath ran: the bf16 MFMA on a 128 x 128 tile cannot meet the exact-fp32 bound on general operands;
            # on any other tile the request falls back to the exact-fp32 kernel (whose bound _run_class has applied)
            d, (ref, ab, terms) = _ref(index, cls)
            over = (np.abs(got - ref) > B.bound(e, ab, terms, ref, 0, as_fp32=True)).any()
            assert over == (B.datapath(e) == 'bf16'), (e.why, B.datapath(e))


# ----------------------------------------------------------------------------------------------------------------------
# rejections: the call raises and has touched neither dw nor the workspace
_BASE_DENSE = B._dense(33, 40, 72, '', ldz=48, ldx=80)
_BASE_CONV = B._conv(2, 4, 16, 64, 40, 3, 1, 1, '')
_BASE_B16 = B._dense(33, 64, 64, '', ldz=72, ldx=72, b16=1)
REJECTIONS = (
    ('conv: C % 64 != 0', _BASE_CONV, dict(C=32, K=9 * 32), {}),
    ('N % 4 != 0', _BASE_DENSE, dict(N=42), {}),
    ('K % 4 != 0', _BASE_DENSE, dict(K=74), {}),
    ('conv: M % (Ho Wo) != 0', _BASE_CONV, dict(M=127), {}),
    ('bf16-in: ldz % 8 != 0', _BASE_B16, dict(ldz=68), {}),
    ('bf16-in: ldx % 8 != 0', _BASE_B16, dict(ldx=68), {}),
    ('bf16-in: dz not 16-byte aligned', _BASE_B16, {}, dict(dz=4)),
    ('bf16-in: x not 16-byte aligned', _BASE_B16, {}, dict(x=4)),
    ('conv: k_out with taps > 1', _BASE_CONV, dict(k_out=9 * 64 - 4), {}),
    ('dense: dw not 16-byte aligned', _BASE_DENSE, {}, dict(dw=1)),
)


@pytest.mark.parametrize('what,e,fields,skew', REJECTIONS, ids=[r[0] for r in REJECTIONS])
@pytest.mark.parametrize('accumulate', (0, 1))
def test_rejected_call_launches_nothing(what, e, fields, skew, accumulate):
    _lib = _L()
    lib = _lib.load()
    r = B.rng_for('reject', e.M, e.N, e.K)
    xrows = e.M if e.kind == 'dense' else e.geom[0] * e.geom[1] * e.geom[2]
    dz = _Operand(B.to_bf16(r.standard_normal((e.M, e.ldz))), bool(e.b16), skew.get('dz', 0))
    x = _Operand(B.to_bf16(r.standard_normal((xrows, e.ldx))), bool(e.b16), skew.get('x', 0))
    nws = int(lib.grl_wgrad_workspace_floats(C.byref(_descriptor(e, 0, 0, 0, 0, 0))))
    ws = _Output(nws + SLACK, fill=float('nan'))
    dw = _Output(e.N * e.K + SLACK, init=B.f32(r.standard_normal(e.N * e.K + SLACK)), skew=skew.get('dw', 0))
    before = dw.bits().copy(), ws.bits().copy()
    d = _descriptor(e, dz.ptr(), x.ptr(), dw.ptr(), ws.ptr(), accumulate)
    for k, v in fields.items():
        setattr(d, k, v)
    with pytest.raises(_lib.GrlHipError):
        _lib.check(lib.grl_conv_wgrad_f32(C.byref(d), _lib.stream()), what)
    assert np.array_equal(dw.bits(), before[0]), 'a rejected call wrote dw'
    assert np.array_equal(ws.bits(), before[1]), 'a rejected call wrote the workspace'
    assert dz.unchanged() and x.unchanged()


def test_rejection_bases_are_accepted():
    """the descriptors the rejection cases start from are valid: each case fails for its one fault alone"""
    for e in (_BASE_DENSE, _BASE_CONV, _BASE_B16):
        r = B.rng_for('accept', e.M, e.N, e.K)
        xrows = e.M if e.kind == 'dense' else e.geom[0] * e.geom[1] * e.geom[2]
        d = dict(dz=B.to_bf16(r.standard_normal((e.M, e.ldz))), x=B.to_bf16(r.standard_normal((xrows, e.ldx))))
        ref, ab, terms = B.reference(e, d)
        dz, x = _Operand(d['dz'], bool(e.b16)), _Operand(d['x'], bool(e.b16))
        ws = _Output(int(_L().load().grl_wgrad_workspace_floats(C.byref(_descriptor(e, 0, 0, 0, 0, 0)))), fill=float('nan'))
        dw = _Output(ref.size)
        _launch(e, dz, x, dw, ws, 0)
        B.check('rejection bases', dw.values(ref.shape), ref, B.bound(e, ab, terms, ref, 0), e)


def test_stem_rejects_bad_arguments():
    """grl_stem_wgrad: odd H or W, a dz that is not 16-byte aligned: raised, nothing written"""
    _lib = _L()
    lib = _lib.load()
    e = B._stem(1, 16, 32, 0, '')
    r = B.rng_for('reject stem')
    dz = _Operand(B.f32(r.standard_normal((e.M, 64))), False, skew=1)
    x = _Operand(B.f32(r.standard_normal((1, 3, 16, 32))), False)
    ws = _Output(int(lib.grl_stem_wgrad_workspace_floats(1, 16, 32)), fill=float('nan'))
    dw = _Output(64 * 147)
    before = dw.bits().copy(), ws.bits().copy()
    for args in ((x.ptr(), dz.ptr(), 0, dw.ptr(), ws.ptr(), 1, 16, 32), (x.ptr(), dz.ptr() - 4, 0, dw.ptr(), ws.ptr(), 1, 15, 32),
                 (x.ptr(), dz.ptr() - 4, 0, dw.ptr(), ws.ptr(), 1, 16, 31)):
        with pytest.raises(_lib.GrlHipError):
            _lib.check(lib.grl_stem_wgrad(*(args + (0, _lib.stream()))), 'grl_stem_wgrad')
    assert np.array_equal(dw.bits(), before[0]) and np.array_equal(ws.bits(), before[1])
