"""MX-FP8 eval datapath ('mxfp8', GRL_MATH_MXFP8) without a GPU: the numpy model of the numerics contract
(tests/mx_ref.py) on hand-computed cases, the host build of the quantiser's element / exponent rules against it,
the math-mode switches and the new C ABI."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mx_ref as R                      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _block(vals):
    x = np.zeros((1, 32), dtype=np.float32)
    x[0, :len(vals)] = vals
    return x


def test_scale_rule():
    # e = floor(log2 amax) - 8: amax 1.0 -> e = -8 (byte 119); 3.0 -> -7; 448 -> 0; 512 -> 1; 0.75 -> -9
    for amax, e in ((1.0, -8), (3.0, -7), (448.0, 0), (512.0, 1), (0.75, -9), (2.0 ** 100, 92), (2.0 ** -120, -127)):
        q, s = R.quantize_rows(_block([amax, -amax / 4]))
        assert int(s[0, 0]) == e + 127, (amax, int(s[0, 0]) - 127, e)
    # the largest element maps to [256, 512): 1.0 * 2^8 = 256 = 0x78 (exponent field 15, mantissa 0)
    q, s = R.quantize_rows(_block([1.0]))
    assert q[0, 0] == 0x78 and R.e4m3_decode(q[0, 0]) == 256.0
    # clamping at the top: +inf counts as 2^128 -> e = 120, and the inf element saturates
    q, s = R.quantize_rows(_block([np.inf, 1.0]))
    assert int(s[0, 0]) == 120 + 127 and q[0, 0] == 0x7E


def test_saturation_at_448():
    # amax in [2^k * 448/256, 2^(k+1)): scaled values in [448, 512) saturate to 0x7E (= 448), never NaN
    q, s = R.quantize_rows(_block([1.9, -1.99, 1.75]))
    assert int(s[0, 0]) - 127 == -8
    assert q[0, 0] == 0x7E and q[0, 1] == 0xFE and q[0, 2] == 0x7E         # 1.9 * 256 = 486.4, 1.75 * 256 = 448
    assert R.e4m3_decode(0x7E) == 448.0 and R.e4m3_decode(0xFE) == -448.0
    assert np.isnan(R.e4m3_decode(0x7F))


def test_round_to_nearest_even_ties():
    # within [256, 512) the e4m3 step is 32: 272 = 256 + 16 is a tie -> 256 (even), 304 = 288 + 16 -> 320 (even)
    e4 = R.e4m3_encode
    assert R.e4m3_decode(e4(272.0)) == 256.0 and R.e4m3_decode(e4(304.0)) == 320.0
    assert R.e4m3_decode(e4(272.01)) == 288.0 and R.e4m3_decode(e4(303.99)) == 288.0
    # step 1/8 in [1, 2): 1.0625 -> 1.0, 1.1875 -> 1.25
    assert R.e4m3_decode(e4(1.0625)) == 1.0 and R.e4m3_decode(e4(1.1875)) == 1.25


def test_subnormals():
    # e4m3 subnormals are multiples of 2^-9 below 2^-6; ties to even; 2^-10 -> 0, 3 * 2^-10 -> 2^-8
    e4 = R.e4m3_encode
    assert e4(2.0 ** -9) == 0x01 and e4(7 * 2.0 ** -9) == 0x07 and e4(2.0 ** -6) == 0x08
    assert e4(2.0 ** -10) == 0x00 and e4(3 * 2.0 ** -10) == 0x02 and e4(-5 * 2.0 ** -10) == 0x82
    assert e4(15 * 2.0 ** -10) == 0x08                       # 7.5 * 2^-9 rounds up into the smallest normal
    assert R.e4m3_decode(0x03) == 3 * 2.0 ** -9
    # in a block: amax 1.0 (e = -8) puts 2^-15 at 2^-7 = subnormal code 4
    q, _ = R.quantize_rows(_block([1.0, 2.0 ** -15, 2.0 ** -18]))
    assert q[0, 1] == 0x04 and q[0, 2] == 0x00


def test_zero_block_and_nan():
    q, s = R.quantize_rows(np.zeros((2, 64), dtype=np.float32))
    assert (s == 0).all() and (q == 0).all()
    x = _block([1.0, np.nan, -2.0])
    q, s = R.quantize_rows(x)
    assert int(s[0, 0]) - 127 == -7                         # NaN ignored by the amax
    assert q[0, 1] & 0x7F == 0x7F
    d = R.dequantize(q, s)
    assert np.isnan(d[0, 1]) and d[0, 0] == 1.0 and d[0, 2] == -2.0
    # an all-NaN block: scale byte 0, NaN elements (the NaN reaches every output it touches)
    q, s = R.quantize_rows(np.full((1, 32), np.nan, dtype=np.float32))
    assert s[0, 0] == 0 and np.isnan(R.dequantize(q, s)).all()


def test_dequantised_error_bound():
    # |x - deq(q(x))| <= 2^-4 |x| for normal-range elements (3 mantissa bits), <= 2^(e-10) absolute in the subnormal
    # range, and |x| - 448 * 2^e where the block maximum saturates
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((64, 256)) * np.exp(rng.uniform(-8, 8, (64, 1)))).astype(np.float32)
    q, s = R.quantize_rows(x)
    d = R.dequantize(q, s)
    e = (s.astype(np.int64) - 127).repeat(32, axis=1)
    bound = np.maximum(np.maximum(np.abs(x) * 2.0 ** -4, np.ldexp(1.0, e - 10)), np.abs(x) - np.ldexp(448.0, e))
    assert (np.abs(d - x) <= bound).all()


def _lib():
    from grl_amd import _lib
    return _lib.load()


def _host_quant(x):
    """tests/mx_ref.quantize_rows through the library's host build of the device rules"""
    lib = _lib()
    x = np.ascontiguousarray(x, dtype=np.float32)
    M, K = x.shape
    bits = x.view(np.int32)
    q = np.zeros((M, K), np.uint8)
    s = np.zeros((M, K // 32), np.uint8)
    for r in range(M):
        for kb in range(K // 32):
            blk = bits[r, 32 * kb:32 * kb + 32]
            ab = blk & 0x7FFFFFFF
            ab = ab[ab <= 0x7F800000]
            e = lib.grl_mx_block_exp_host(int(ab.max()) if ab.size else 0)
            s[r, kb] = e + 127
            for i in range(32):
                q[r, 32 * kb + i] = lib.grl_mx_e4m3_host(int(blk[i]), e)
    return q, s


def test_host_quantiser_matches_the_model():
    """The integer-only device rule (built for the host too) is bit-identical to the float64 model: random blocks over
    the whole bf16 range, zero, tiny (subnormal), huge, inf and NaN blocks, signed zeros, exact ties."""
    rng = np.random.default_rng(1)
    rows = [rng.standard_normal(64) * np.exp(rng.uniform(-80, 80)) for _ in range(24)]
    rows.append(np.zeros(64))
    rows.append(np.full(64, 1e-39) * rng.standard_normal(64))                # fp32 subnormals
    rows.append(np.full(64, 1e-38) * rng.standard_normal(64))                # normal maxima below 2^-118: e clamps at -127
    rows.append(rng.standard_normal(64) * 1e37)
    r = rng.standard_normal(64); r[3] = np.nan; r[40] = np.inf; r[41] = -np.inf
    rows.append(r)
    rows.append(np.full(64, np.nan))
    rows.append(np.array([1.0, 272 / 256.0, 304 / 256.0, -0.0, 2.0 ** -15, 3 * 2.0 ** -18] * 10 + [0.0] * 4))
    x = np.stack(rows).astype(np.float32)
    x = R.bf16_round(x)                                              # (A is bf16 in the pipeline)
    q0, s0 = R.quantize_rows(x)
    q1, s1 = _host_quant(x)
    assert np.array_equal(s0, s1), np.argwhere(s0 != s1)[:5]
    bad = np.argwhere(q0 != q1)
    assert bad.size == 0, [(tuple(i), float(x[tuple(i)]), int(q0[tuple(i)]), int(q1[tuple(i)])) for i in bad[:5]]


def test_host_element_rule_exhaustive_over_bf16():
    """Every bf16 bit pattern at the scale of a few representative exponents: host rule == model."""
    lib = _lib()
    u = (np.arange(65536, dtype=np.uint32) << 16)
    x = u.view(np.float32)
    for e in (-127, -20, -8, 0, 5, 120):
        with np.errstate(over='ignore', invalid='ignore'):
            ref = R.e4m3_encode(x.astype(np.float64) * 2.0 ** -e)
        sel = np.arange(0, 65536, 7)                                 # (a 1-in-7 sample keeps the ctypes loop short)
        got = np.array([lib.grl_mx_e4m3_host(int(np.int32(u[i].astype(np.int64) - (1 << 32) if u[i] >= 2 ** 31 else u[i])), e)
                        for i in sel], dtype=np.uint8)
        bad = np.nonzero(got != ref[sel])[0]
        assert bad.size == 0, (e, [(hex(int(u[sel][i])), int(ref[sel][i]), int(got[i])) for i in bad[:5]])


def test_mxfp8_is_experimental_not_a_user_mode():
    """The MX datapath is slower than 'bf16s' today (EXPERIMENTS.md): set_math / math_mode / GRL_MATH refuse it, the
    experimental switch reaches it and restores the previous mode."""
    from grl_amd import engine
    old = engine.get_math()
    with pytest.raises(KeyError):
        engine.set_math('mxfp8')
    with pytest.raises(KeyError):
        with engine.math_mode('mxfp8'):
            pass
    assert engine.get_math() == old
    with engine.experimental_math('mxfp8'):
        assert engine.get_math() == 'mxfp8' and engine._math[0] == engine.MATH_MXFP8
        with engine.math_mode('bf16s'):
            assert engine.get_math() == 'bf16s'
        assert engine.get_math() == 'mxfp8'
    assert engine.get_math() == old


def test_train_engine_refuses_mxfp8():
    from grl_amd import train_engine
    old = train_engine.get_math()
    with pytest.raises(ValueError, match='eval-only'):
        train_engine.set_math('mxfp8')
    assert train_engine.get_math() == old


def test_mx_prototypes_are_bound():
    import ctypes as C
    from grl_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'grl_hip.h')).read()
    assert re.search(r'#define\s+GRL_MATH_MXFP8\s+4\b', hdr)
    assert _lib.MATH_MXFP8 == 4 and _lib.ABI_VERSION == lib.grl_abi_version() == 10
    for n in ('grl_mx_pack_weights', 'grl_mx_quantize_rows', 'grl_mx_image_bytes'):
        assert n in _lib._SIGNATURES and n in hdr
    assert lib.grl_mx_image_bytes(3, 96) == 3 * 96 + 3 * 4
    assert lib.grl_mx_image_bytes(2, 160) == 2 * 160 + 2 * 8
    assert lib.grl_mx_image_bytes(2, 48) == 0
    # argument checks before any HIP call
    assert lib.grl_mx_pack_weights(16, 8, 48, 48, 16, None) == _lib.GRL_EUNSUPPORTED
    assert lib.grl_mx_quantize_rows(None, 8, 64, 64, 16, None) == _lib.GRL_EINVAL
    # the GEMM entry: unsupported MX descriptors are refused with GRL_EUNSUPPORTED, no device needed
    d = _lib.GrlGemm()
    d.a = d.w = d.y = 16
    d.M, d.N, d.K, d.lda, d.ldw, d.ldy = 64, 64, 64, 64, 64, 64
    d.math = _lib.MATH_MXFP8
    for field, val in (('epilogue', _lib.EPI_EUCLID), ('epilogue', _lib.EPI_NEGDOT), ('stats', 16), ('kblock', 1),
                       ('out_f32', 1), ('K', 48)):
        old = getattr(d, field)
        setattr(d, field, val)
        assert lib.grl_conv_gemm_f32(C.byref(d), None) == _lib.GRL_EUNSUPPORTED, field
        assert b'mxfp8' in lib.grl_last_error()
        setattr(d, field, old)
    # without the activation scratch: GRL_EINVAL, and the workspace query names the size
    assert lib.grl_conv_gemm_f32(C.byref(d), None) == _lib.GRL_EINVAL
    assert lib.grl_conv_gemm_f32_workspace_floats(C.byref(d)) == (64 * 64 + 64 * 4) // 4
