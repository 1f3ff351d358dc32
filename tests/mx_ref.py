"""numpy model of the MX-FP8 numerics contract of GRL_MATH_MXFP8 (include/grl_hip.h).

OCP MX v1.0 with blocks of 32 consecutive elements along K:

  * shared exponent e = floor(log2(amax)) - 8 (8 = emax of e4m3), clamped to [-127, 127]; amax is the largest |x| of
    the block, NaNs ignored, +inf counting as 2^128; the E8M0 scale byte is e + 127;
  * an all-zero block (amax == 0) gets scale byte 0 and zero elements;
  * element = e4m3fn (OCP, not fnuz) of x * 2^-e, rounded to nearest even, saturated to +-448; NaN -> 0x7F (with the
    sign bit of the input), -0 keeps its sign (0x80).

This is the yardstick of the device quantiser (grl_mx_quantize_rows / grl_mx_pack_weights); it is written
independently of it (float64 arithmetic here, integer bit manipulation there).
"""
import numpy as np

BLOCK = 32
E4M3_MAX = 448.0
E4M3_EMAX = 8


def scale_padded(kb):
    """scale bytes per row of an MX image: K/32 rounded up to a multiple of 4"""
    return (kb + 3) // 4 * 4


def block_exponent(amax):
    """e of the contract for an array of block maxima (float64, >= 0, no NaN); zero blocks give -127"""
    amax = np.asarray(amax, dtype=np.float64)
    _, ex = np.frexp(np.where(np.isfinite(amax) & (amax > 0), amax, 1.0))
    fl = ex.astype(np.int64) - 1                          # floor(log2(amax)) for finite amax > 0
    fl = np.where(np.isinf(amax), 128, fl)
    e = np.clip(fl - E4M3_EMAX, -127, 127)
    return np.where(amax == 0, -127, e)


def e4m3_encode(f):
    """float64 array (already scaled) -> e4m3fn codes, round to nearest even, saturating"""
    with np.errstate(invalid='ignore', over='ignore'):
        return _e4m3_encode(np.asarray(f, dtype=np.float64))


def _e4m3_encode(f):
    sign = np.where(np.signbit(f), 0x80, 0).astype(np.int64)
    a = np.abs(f)
    nan = np.isnan(f)
    a = np.where(nan, 0.0, np.minimum(a, 1024.0))          # (inf saturates below; keeps the casts finite)
    sub = a < 2.0 ** -6
    q_sub = np.rint(a * 512.0).astype(np.int64)           # multiples of 2^-9, 8 = the smallest normal (code 0x08)
    m, ex = np.frexp(np.where(sub, 1.0, a))               # a = m * 2^ex, m in [0.5, 1)
    E = ex.astype(np.int64) - 1
    q = np.rint((m * 2.0 - 1.0) * 8.0).astype(np.int64)   # 3 mantissa bits, ties to even (np.rint)
    code_n = ((E + 7) << 3) + q                           # q == 8 carries into the exponent
    code = np.where(sub, q_sub, code_n)
    code = np.where(a >= E4M3_MAX, 0x7E, np.minimum(code, 0x7E))
    code = np.where(nan, 0x7F, code)
    return (code | sign).astype(np.uint8)


def e4m3_decode(codes):
    """e4m3fn codes -> float64"""
    c = np.asarray(codes, dtype=np.int64)
    s = np.where(c & 0x80, -1.0, 1.0)
    ef = (c >> 3) & 15
    mf = c & 7
    v = np.where(ef == 0, mf / 8.0 * 2.0 ** -6, (1.0 + mf / 8.0) * 2.0 ** (ef - 7.0))
    v = np.where((c & 0x7F) == 0x7F, np.nan, v)
    return s * v


def quantize_rows(x):
    """x: [M][K] (K % 32 == 0) -> (elements uint8 [M][K], scale bytes uint8 [M][K/32])"""
    x = np.asarray(x, dtype=np.float64)
    M, K = x.shape
    assert K % BLOCK == 0
    blk = x.reshape(M, K // BLOCK, BLOCK)
    amax = np.nanmax(np.where(np.isnan(blk), 0.0, np.abs(blk)), axis=2)
    e = block_exponent(amax)
    f = blk * np.ldexp(1.0, -e)[:, :, None]
    return e4m3_encode(f).reshape(M, K), (e + 127).astype(np.uint8)


def dequantize(elems, scales):
    """(elements [M][K], scale bytes [M][K/32]) -> float64 [M][K]"""
    M, K = elems.shape
    v = e4m3_decode(elems).reshape(M, K // BLOCK, BLOCK)
    return (v * np.ldexp(1.0, scales.astype(np.int64) - 127)[:, :, None]).reshape(M, K)


def fake_quant(x):
    """x -> dequantize(quantize_rows(x)) (float64)"""
    return dequantize(*quantize_rows(x))


def bf16_round(x):
    """float array -> nearest bf16 (ties to even), returned as float32 (NaN kept)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16).astype(np.uint32)
    r = np.where(np.isnan(x), np.uint32(0x7FC00000), r)
    return r.view(np.float32)
