"""The int8 scalar-quantised gallery on the device (engine.Sq8Codebook / sq8_train / sq8_index / sq8_dist / sq8_search /
sq8_metrics_streaming / sq8_refine_search, sq8.hip, GRL_EVAL_SQ8) against the numpy model of
tests/sq8_ref.py.  The integer sums are exact and every float step is one fp32 operation, so every comparison of codes,
sums and distances is exact; the two ordered reductions the model does not own (bias = q . mean by the fp32 GEMM, the
norms by grl_row_sqnorm) are downloaded and handed to it."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import sq8_ref as S
import pq_ref as R
import search_filter_ref as FR

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257, 1000)
NQS = (1, 2, 15, 16, 17, 33, 65, 129)                             # every remainder of the 128 x 128 tile and of its 32 x 32 parts
DPADS = (64, 128, 192, 6144)
DS = (1, 4, 60, 64, 68, 6144)


def bits(a):
    if torch.is_tensor(a):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def product(q, g):
    """the exact int64 product through float64 (every sum is below 2^53)"""
    return (q.astype(np.float64) @ g.astype(np.float64).T).astype(np.int64)


def scan_i32(q, g, nq, n, dpad, ldqc=None, ldc=None, ldo=None):
    """grl_sq8_scan_i32 over the first nq rows of q and n rows of g (device int8, row strides ldqc / ldc)"""
    from grl_amd import engine
    from grl_amd._lib import ptr
    ldo = n if ldo is None else ldo
    out = torch.full((nq, ldo), -77, dtype=torch.int32, device=DEV)
    engine._call('grl_sq8_scan_i32', ptr(q), ldqc or q.stride(0), ptr(g), ldc or g.stride(0), ptr(out), ldo, nq, n, dpad)
    return out


# ----------------------------------------------------------------------------
# 1. integer exactness of the scan
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('dpad', DPADS)
def test_raw_sums_equal_the_int64_product_for_every_remainder_of_the_tile(dpad):
    gen = np.random.Generator(np.random.PCG64(dpad))
    slack = 16
    # queries uniform over all 256 bytes (-128 and +127 included); the gallery skewed and row-dependent, in a wider array
    # whose slack columns and surrounding rows hold sentinels that must not enter any sum
    q = np.full((max(NQS), dpad + slack), 0x55, dtype=np.int8)
    q[:, :dpad] = gen.integers(-128, 128, (max(NQS), dpad))
    q[0, :4] = (-128, 127, -128, 127)
    off = 3
    g = np.full((off + max(NS) + 2, dpad + slack), 0x33, dtype=np.int8)
    body = np.clip(np.rint(gen.standard_normal((max(NS), dpad)) * 50 + 20), -128, 127)
    body[::7] = gen.integers(-128, 128, body[::7].shape)
    body[1, :4] = (127, -128, -128, 127)
    g[off:off + max(NS), :dpad] = body
    qd, gd = dev(q), dev(g)
    want = product(q[:, :dpad], g[off:off + max(NS), :dpad])
    for n in NS:
        for nq in NQS:
            ldo = n + (5 if (n + nq) % 2 else 0)
            got = scan_i32(qd, gd[off:], nq, n, dpad, ldo=ldo).cpu().numpy()
            assert np.array_equal(got[:, :n], want[:nq, :n]), (n, nq)
            assert (got[:, n:] == -77).all(), (n, nq)
    # contiguous operands give the same
    got = scan_i32(dev(q[:33, :dpad]), dev(g[off:off + 257, :dpad]), 33, 257, dpad).cpu().numpy()
    assert np.array_equal(got, want[:33, :257])


@pytest.mark.parametrize('dpad', (64, 192))
def test_unit_queries_read_back_the_columns_of_an_asymmetric_gallery(dpad):
    """query row i is the unit code e_i: out[i][g] must be gallery[g][i] -- a swapped row / column, a transposed tile or a
    k that is paired wrongly between the operands cannot pass"""
    n = 200
    gi, ji = np.arange(n)[:, None], np.arange(dpad)[None, :]
    g = ((gi * 7 + ji * 13 + (gi * ji) % 5) % 255 - 127).astype(np.int8)
    q = np.zeros((dpad, dpad), dtype=np.int8)
    q[np.arange(dpad), np.arange(dpad)] = 1
    got = scan_i32(dev(q), dev(g), dpad, n, dpad).cpu().numpy()
    assert np.array_equal(got, g.T.astype(np.int64))
    assert not np.array_equal(g[:dpad, :dpad], g[:dpad, :dpad].T)


# ----------------------------------------------------------------------------
# 2. accumulator width
# ----------------------------------------------------------------------------
def test_the_accumulator_holds_the_largest_sums_and_the_conversion_rounds_to_nearest_even():
    from grl_amd import engine
    from grl_amd._lib import ptr
    d, n, nq = 16384, 17, 3
    gen = np.random.Generator(np.random.PCG64(9))
    g = np.full((n, d), 127, dtype=np.int8)
    q = np.full((nq, d), 127, dtype=np.int8)
    q[1] = -127
    q[2, ::2] = -127
    for r in range(1, n):                                          # row r has r planted sign flips, then random ones from row 9 on
        g[r, gen.choice(d, r, replace=False)] = -127
    g[9:] = np.where(gen.random((n - 9, d)) < 0.3, -127, 127)
    want = product(q, g)
    assert want[0, 0] == 16384 * 127 * 127 and np.abs(want).max() > 2.6e8
    qd, gd = dev(q), dev(g)
    assert np.array_equal(scan_i32(qd, gd, nq, n, d).cpu().numpy(), want)
    # through the float epilogue with scale 1, bias 0: -float32(isum), and the sums are not all representable
    assert (want.astype(np.float32).astype(np.int64) != want).any()
    one, zero = torch.ones(nq, device=DEV), torch.zeros(nq, device=DEV)
    out = torch.empty((nq, n), dtype=torch.float32, device=DEV)
    engine._call('grl_sq8_scan', ptr(qd), d, ptr(gd), d, ptr(one), ptr(zero), None, None, ptr(out), n, nq, n, d, 0)
    assert np.array_equal(bits(out), bits(np.negative(want.astype(np.float32))))
    assert np.array_equal(bits(out), bits(S.dist(q, np.ones(nq), np.zeros(nq), g)))


# ----------------------------------------------------------------------------
# 3. encode, query, decode, absmax
# ----------------------------------------------------------------------------
SPECIAL = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-39, 1e30, -1e30, 3e38], dtype=np.float32)


@pytest.mark.parametrize('d', DS)
def test_encode_query_and_decode_equal_the_model_bit_for_bit(d):
    from grl_amd import engine
    dp = S.dpad(d)
    for n in NS:
        gen = np.random.Generator(np.random.PCG64(1000 * d + n))
        x = (gen.standard_normal((n, d)) * gen.random(d)[None, :] + 0.3).astype(np.float32)
        if d > 4:
            x[:, 3] = np.float32(0.25)                             # a constant column: delta 0, inv 0
        xd = dev(x)
        book = engine.sq8_train(xd)
        assert (book.d, book.dpad, book.metric) == (d, dp, 'cosine')
        mean = book.mean.cpu().numpy()
        amax = S.absmax(x, mean)
        delta, inv = S.steps_from_amax(amax)
        assert np.array_equal(bits(book.delta), bits(delta)) and np.array_equal(bits(book.inv), bits(inv)), n
        assert np.abs(mean - x.astype(np.float64).mean(0)).max() <= 1e-5
        if d > 4:
            assert delta[3] == 0 and inv[3] == 0
        codes = book.encode(xd)
        assert codes.dtype == torch.int8 and tuple(codes.shape) == (n, dp)
        want = S.encode(x, mean, inv)
        assert np.array_equal(codes.cpu().numpy(), want), n
        assert not codes[:, d:].any()
        assert np.array_equal(bits(book.decode(codes)), bits(S.decode(want, mean, delta))), n
        assert np.array_equal(bits(book.decode(codes[:, :d].contiguous())), bits(S.decode(want, mean, delta))), n
        # rows outside the training range (clamped) and planted special values, encoded by the same codebook
        y = (x * np.float32(3.0)).astype(np.float32)
        y[gen.integers(0, n, 4 * n), gen.integers(0, d, 4 * n)] = SPECIAL[gen.integers(0, len(SPECIAL), 4 * n)]
        y[0, :min(d, len(SPECIAL))] = SPECIAL[:d]
        got = book.encode(dev(y)).cpu().numpy()
        assert np.array_equal(got, S.encode(y, mean, inv)), n
        assert np.abs(got.astype(np.int64)).max() <= 127
        # absmax ignores NaN and keeps the rest
        am = torch.empty(d, dtype=torch.float32, device=DEV)
        engine._call('grl_sq8_absmax', engine.ptr(dev(y)), d, engine.ptr(book.mean), engine.ptr(am), n, d)
        assert np.array_equal(bits(am), bits(S.absmax(y, mean))), n
        # queries: the same rows, the special ones, an all-zero row
        qrows = np.concatenate((x[:5], y[:7], np.zeros((1, d), dtype=np.float32)))
        qcodes, scale, bias, qq = book.query(dev(qrows))
        wc, ws = S.query(qrows, delta)
        assert qcodes.dtype == torch.int8 and tuple(qcodes.shape) == (len(qrows), dp)
        assert np.array_equal(qcodes.cpu().numpy(), wc) and np.array_equal(bits(scale), bits(ws)), n
        assert not qcodes[-1].any() and float(scale[-1]) == 0.0 and not qcodes[:, d:].any()
        ok = np.isfinite(qrows).all(1)
        # the fp32 GEMM's sum of dp products: at most dp roundings of 2^-24 relative to sum |q mean| (doubled)
        tol = (d + 32) * 2.0 ** -23 * (np.abs(qrows[ok].astype(np.float64)) @ np.abs(mean.astype(np.float64)))
        assert (np.abs(bias.cpu().numpy()[ok] - S.bias_host(qrows[ok], mean)) <= tol).all()
    # a caller's codebook: inv = 127 / (127 delta), 0 where delta is 0
    delta = np.abs(gen.standard_normal(d)).astype(np.float32)
    delta[0] = 0
    book = engine.Sq8Codebook(dev(mean), dev(delta), 'euclidean')
    assert np.array_equal(bits(book.inv), bits(S.inv_from_delta(delta))) and book.metric == 'euclidean'
    assert np.array_equal(book.encode(xd).cpu().numpy(), S.encode(x, mean, S.inv_from_delta(delta)))
    assert tuple(book.encode(xd[:0]).shape) == (0, dp) and engine.sq8_index(xd[:0], book).n == 0


# ----------------------------------------------------------------------------
# 4. distances
# ----------------------------------------------------------------------------
def _rows(n, d, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    x = g.standard_normal((n, d)).astype(np.float32) + np.float32(0.1)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def model_dist(index, blocks_or_query, metric):
    qcodes, scale, bias, qq = blocks_or_query
    return S.dist(qcodes.cpu().numpy(), scale.cpu().numpy(), bias.cpu().numpy(), index.codes.cpu().numpy(), metric,
                  qq.cpu().numpy(), index.gg.cpu().numpy())


@pytest.mark.parametrize('metric', ('cosine', 'euclidean'))
def test_dist_equals_the_model_fed_the_downloaded_bias_and_norms_for_every_blocking(metric):
    from grl_amd import engine
    for d, n, nq in ((60, 257, 5), (128, 1000, 33), (6144, 129, 17)):
        gx = _rows(n, d, 3 + n)
        gx[1::2] = gx[0:-1:2][:gx[1::2].shape[0]]                   # duplicate rows
        gd, qd = dev(gx), dev(_rows(nq, d, 11 + nq))
        index = engine.sq8_index(gd, engine.sq8_train(gd, metric))
        assert (index.n, index.d, tuple(index.gg.shape)) == (n, d, (n,))
        assert index.nbytes == n * S.dpad(d) + 4 * n + 12 * d
        book = index.codebook
        # gg is grl_row_sqnorm of the decoded rows; reconstruct returns them
        rec = index.reconstruct(torch.arange(n, device=DEV))
        assert np.array_equal(bits(rec), bits(S.decode(index.codes.cpu().numpy(), book.mean.cpu().numpy(), book.delta.cpu().numpy())))
        assert np.abs(index.gg.cpu().numpy() - S.sqnorm_host(rec.cpu().numpy())).max() <= 1e-5
        # a stored value is within half a step of its row, the half widened by the rounding of (x - mean) * inv (two
        # roundings of a value of at most 127: 127 * 2^-22 steps) and of the decode (2^-23 relative)
        dl = book.delta.cpu().numpy().astype(np.float64)
        assert (np.abs(rec.cpu().numpy().astype(np.float64) - gx) <= dl[None, :] * (0.5 + 127 * 2.0 ** -22) + 2.0 ** -22).all()
        D = engine.sq8_dist(qd, index)
        assert tuple(D.shape) == (nq, n) and D.dtype == torch.float32
        want = model_dist(index, book.query(qd), metric)
        assert np.array_equal(bits(D), bits(want)), (d, n, nq)
        for bc in (1, 7, 256, n):
            assert np.array_equal(bits(engine.sq8_dist(qd, index, block_cols=bc)), bits(D)), bc
        assert np.array_equal(bits(engine.sq8_dist(qd, index, block_bytes=1)), bits(D))
        # and it means what it says: within the derived bound of tests/test_sq8_cpu.py of the float64 -q.g, plus the fp32
        # GEMM's bias (d roundings of 2^-24 on sum |q mean|, doubled)
        if metric == 'cosine':
            qn = qd.cpu().numpy().astype(np.float64)
            qcodes, scale, bias, qq = book.query(qd)
            t1 = 0.5 * scale.cpu().numpy().astype(np.float64)[:, None] * np.abs(index.codes.cpu().numpy().astype(np.float64)).sum(1)[None, :]
            t2 = 0.5 * (np.abs(qn) @ dl)[:, None]
            slack = 2.0 ** -22 * (127.0 * 2.0 * (t1 + t2) + 4.0) + d * 2.0 ** -23 * (np.abs(qn) @ np.abs(book.mean.cpu().numpy().astype(np.float64)))[:, None]
            assert (np.abs(D.cpu().numpy().astype(np.float64) + qn @ gx.astype(np.float64).T) <= t1 + t2 + slack).all()


# ----------------------------------------------------------------------------
# 5. search and metrics
# ----------------------------------------------------------------------------
_cache = {}


def search_case(metric):
    """33 queries against 300 code rows with duplicates, d = 68; D = the materialised matrix, its ranking and ids.  Built
    once per metric, never modified."""
    from grl_amd import engine
    if metric not in _cache:
        gx = _rows(300, 68, 17)
        gx[1::2] = gx[0:-1:2]
        gd = dev(gx)
        index = engine.sq8_index(gd, engine.sq8_train(gd, metric))
        qf = dev(_rows(33, 68, 19))
        D = engine.sq8_dist(qf, index)
        g = np.random.Generator(np.random.PCG64(77))
        ids = (g.integers(0, 12, 33), g.integers(0, 12, 300), g.integers(0, 3, 33), g.integers(0, 3, 300))
        _cache[metric] = (index, qf, D, engine.rank_rows(D), ids, gd)
    return _cache[metric]


@pytest.mark.parametrize('metric', ('cosine', 'euclidean'))
def test_search_is_the_head_of_the_ranked_matrix_with_ties_to_the_smaller_index(metric):
    from grl_amd import engine
    index, qf, D, order, ids, gd = search_case(metric)
    Dn, n = D.cpu().numpy(), index.n
    assert (np.diff(np.sort(Dn, axis=1), axis=1) == 0).any(axis=1).all()           # ties in every row
    for k in (1, 10, 1024):                                        # 1024 > n = 300: padding
        dv, di = engine.sq8_search(qf, index, k)
        assert tuple(dv.shape) == (33, k) and di.dtype == torch.int64
        kk = min(k, n)
        want_i = order[:, :kk].cpu().numpy().astype(np.int64)
        assert np.array_equal(di[:, :kk].cpu().numpy(), want_i), k
        assert np.array_equal(bits(dv[:, :kk]), bits(np.take_along_axis(Dn, want_i, 1))), k
        assert (di[:, kk:] == -1).all() and torch.isinf(dv[:, kk:]).all() and (dv[:, kk:] > 0).all()
        mv, mi = R.search(Dn, k)
        assert np.array_equal(di.cpu().numpy(), mi) and np.array_equal(bits(dv), bits(mv)), k
        dv, di = engine.sq8_search(qf, index, k, exclude=ids)
        wv, wi = FR.filtered_topk(Dn, k, *ids)
        assert np.array_equal(di.cpu().numpy(), wi) and np.array_equal(bits(dv), bits(wv)), k
    d0, i0 = engine.sq8_search(qf, index, 10)
    for kw in (dict(block_cols=1), dict(block_cols=7), dict(block_cols=256), dict(block_cols=n), dict(block_bytes=1)):
        dv, di = engine.sq8_search(qf, index, 10, **kw)
        assert np.array_equal(bits(dv), bits(d0)) and torch.equal(di, i0), kw


def test_empty_queries_and_an_empty_gallery():
    from grl_amd import engine
    index, qf, D, order, ids, gd = search_case('cosine')
    dv, di = engine.sq8_search(qf[:0], index, 5)
    assert tuple(dv.shape) == (0, 5) and tuple(di.shape) == (0, 5)
    assert tuple(engine.sq8_dist(qf[:0], index).shape) == (0, 300)
    empty = engine.sq8_index(gd[:0], index.codebook)
    dv, di = engine.sq8_search(qf, empty, 5)
    assert (di == -1).all() and torch.isinf(dv).all() and tuple(dv.shape) == (33, 5)
    assert tuple(engine.sq8_dist(qf, empty).shape) == (33, 0)


@pytest.mark.parametrize('metric', ('cosine', 'euclidean'))
def test_streaming_metrics_equal_the_matrix_consumers(metric):
    from grl_amd import engine
    index, qf, D, order, ids, gd = search_case(metric)
    cmc, mAP = engine.rank_metrics(order, *ids, max_rank=50)
    for bc in (None, 64):                                          # one pass, several passes
        c2, m2 = engine.sq8_metrics_streaming(qf, index, *ids, max_rank=50, block_cols=bc)
        assert np.array_equal(c2, cmc), bc
        assert abs(m2 - mAP) <= 1e-6, bc                           # fp64, another summation order


@pytest.mark.parametrize('metric', ('cosine', 'euclidean'))
def test_refine_is_its_stated_composition(metric):
    from grl_amd import engine
    index, qf, D, order, ids, gd = search_case(metric)
    n = index.n
    for dtype in ('f32', 'bf16'):
        store = engine.RefineStore(gd, dtype)
        for k, Rr, ex in ((10, 100, None), (10, 10, None), (5, 64, ids)):
            dv, di = engine.sq8_refine_search(qf, index, store, k, Rr, exclude=ex)
            cand = engine.sq8_search(qf, index, Rr, exclude=ex)[1]
            wv, wi = engine.refine_lists(qf, store, cand, k, metric)
            assert np.array_equal(bits(dv), bits(wv)) and torch.equal(di, wi), (dtype, k, Rr)
        # R = n: the shortlist is every row, so the lists are refine_lists over all rows
        dv, di = engine.sq8_refine_search(qf, index, store, 10, n)
        every = torch.arange(n, dtype=torch.int64, device=DEV).repeat(33, 1)
        wv, wi = engine.refine_lists(qf, store, every, 10, metric)
        assert torch.equal(di, wi) and np.array_equal(bits(dv), bits(wv)), dtype


# ----------------------------------------------------------------------------
# 6. the recipe on the device
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('seed', S.RECIPE['seeds'])
def test_the_recipe_ranks_as_the_model_does_and_meets_the_floor(seed):
    from grl_amd import engine
    gal, qry = S.recipe(seed)
    gd, qd = dev(gal), dev(qry)
    book = engine.sq8_train(gd)
    index = engine.sq8_index(gd, book)
    mean = book.mean.cpu().numpy()
    delta, inv = S.steps_from_amax(S.absmax(gal, mean))
    assert np.array_equal(index.codes.cpu().numpy(), S.encode(gal, mean, inv))
    qcodes, scale, bias, qq = book.query(qd)
    wc, ws = S.query(qry, delta)
    assert np.array_equal(qcodes.cpu().numpy(), wc) and np.array_equal(bits(scale), bits(ws))
    Dm = S.dist(wc, ws, bias.cpu().numpy(), index.codes.cpu().numpy())
    di = engine.sq8_search(qd, index, 10)[1].cpu().numpy()
    assert np.array_equal(di, S.ranked(Dm, 10))
    exact = S.exact_lists(qry, gal, 10)
    rec_dev, rec_model = S.recall_at(di, exact, 10), S.recall_at(S.ranked(Dm, 10), exact, 10)
    print('seed %d: recall@10 device %.4f model %.4f' % (seed, rec_dev, rec_model))
    assert rec_dev == rec_model and rec_dev >= S.RECIPE['floor']
    # the same bits from a second run
    again = engine.sq8_train(gd)
    assert torch.equal(again.mean, book.mean) and torch.equal(again.delta, book.delta) and torch.equal(again.inv, book.inv)


# ----------------------------------------------------------------------------
# 7. arguments
# ----------------------------------------------------------------------------
def test_value_errors_name_the_argument_and_rejected_calls_launch_nothing():
    from grl_amd import engine, _lib
    from grl_amd._lib import ptr
    index, qf, D, order, ids, gd = search_case('cosine')
    book = index.codebook
    host = torch.zeros((4, 68))
    with pytest.raises(ValueError, match='sq8_train: xf must be a 2-d float32 tensor on a HIP device'):
        engine.sq8_train(host)
    with pytest.raises(ValueError, match="sq8_train: metric must be 'cosine' or 'euclidean'"):
        engine.sq8_train(gd, 'l1')
    with pytest.raises(ValueError, match='sq8_train: xf needs at least one row'):
        engine.sq8_train(gd[:0])
    with pytest.raises(ValueError, match=r'Sq8Codebook: mean must be a float32 device tensor \[d\]'):
        engine.Sq8Codebook(host[0], book.delta)
    with pytest.raises(ValueError, match=r'Sq8Codebook: delta must be a float32 device tensor \[d\] = \[68\]'):
        engine.Sq8Codebook(book.mean, book.delta[:60])
    with pytest.raises(ValueError, match='Sq8Codebook: delta must be >= 0'):
        engine.Sq8Codebook(book.mean, -book.delta - 1)
    nan = book.delta.clone()
    nan[3] = float('nan')
    with pytest.raises(ValueError, match='Sq8Codebook: delta must be >= 0'):
        engine.Sq8Codebook(book.mean, nan)
    with pytest.raises(ValueError, match="Sq8Codebook: metric must be 'cosine' or 'euclidean'"):
        engine.Sq8Codebook(book.mean, book.delta, 'dot')
    for fn, what in ((book.encode, 'Sq8Codebook.encode: xf'), (book.query, 'Sq8Codebook.query: qf'),
                     (lambda t: engine.sq8_index(t, book), 'sq8_index: xf'), (lambda t: engine.sq8_dist(t, index), '_Sq8Blocks: qf'),
                     (lambda t: engine.sq8_search(t, index, 3), 'sq8_search: qf'),
                     (lambda t: engine.sq8_metrics_streaming(t, index, *ids), 'sq8_metrics_streaming: qf')):
        with pytest.raises(ValueError, match=r'%s must be \[rows, d\] = \[rows, 68\]' % what):
            fn(gd[:3, :64].contiguous())
        with pytest.raises(ValueError, match='%s must be a 2-d float32 tensor on a HIP device' % what):
            fn(host)
    for wrong in (index.codes.to(torch.uint8), index.codes[:, :64].contiguous(), index.codes.cpu(), 5):
        with pytest.raises(ValueError, match=r'Sq8Index: codes must be an int8 device tensor \[rows, dpad\] = \[rows, 128\] or '
                                             r'\[rows, d\] = \[rows, 68\]'):
            engine.Sq8Index(book, wrong)
    dirty = index.codes.clone()
    dirty[5, 100] = 1
    with pytest.raises(ValueError, match=r'Sq8Index: the columns d .. dpad = 68 .. 128 of codes must be 0'):
        engine.Sq8Index(book, dirty)
    narrow = engine.Sq8Index(book, index.codes[:, :68].contiguous())              # the public view is accepted
    assert torch.equal(narrow.codes, index.codes) and np.array_equal(bits(narrow.gg), bits(index.gg))
    for fn in (lambda: engine.sq8_dist(qf, book), lambda: engine.sq8_search(qf, book, 3), lambda: engine._Sq8Blocks(qf, None),
               lambda: engine.sq8_metrics_streaming(qf, 7, *ids), lambda: engine.sq8_refine_search(qf, book, None, 3, 5)):
        with pytest.raises(ValueError, match='index must be a Sq8Index'):
            fn()
    for k in (0, 1025, True):
        with pytest.raises(ValueError, match='sq8_search: k must be in 1..1024'):
            engine.sq8_search(qf, index, k)
    store = engine.RefineStore(gd)
    with pytest.raises(ValueError, match='sq8_refine_search: store must be a RefineStore'):
        engine.sq8_refine_search(qf, index, gd, 3, 5)
    with pytest.raises(ValueError, match=r'sq8_refine_search: store must hold the rows of the index: store is \[299, 68\]'):
        engine.sq8_refine_search(qf, index, engine.RefineStore(gd[:299].contiguous()), 3, 5)
    for k, Rr, name in ((0, 5, 'k'), (6, 5, 'R'), (3, 1025, 'R'), (3.0, 5, 'k')):
        with pytest.raises(ValueError, match='sq8_refine_search: %s' % name):
            engine.sq8_refine_search(qf, index, store, k, Rr)
    for rows in (torch.zeros(2, device=DEV), torch.zeros((1, 2), dtype=torch.int64, device=DEV), [0, 1]):
        with pytest.raises(ValueError, match='Sq8Index.reconstruct: rows must be a 1-d integer device tensor'):
            index.reconstruct(rows)
    with pytest.raises(ValueError, match=r'Sq8Index.reconstruct: rows must be in 0..n-1 = 0..299'):
        index.reconstruct(torch.tensor([0, 300], device=DEV))
    # rejected C calls leave their output alone (the status comes before any launch)
    lib = _lib.load()
    out = torch.full((33, 300), 5.5, dtype=torch.float32, device=DEV)
    qcodes, scale, bias, qq = book.query(qf)
    args = lambda **kw: [kw.get('q', ptr(qcodes)), kw.get('ldqc', 128), ptr(index.codes), kw.get('ldc', 128), ptr(scale), ptr(bias),
                         kw.get('qq', None), None, ptr(out), kw.get('ldo', 300), 33, 300, kw.get('dpad', 128), kw.get('metric', 0), None]
    for kw in (dict(q=ptr(qcodes) + 8), dict(ldqc=64), dict(ldc=120), dict(ldo=299), dict(dpad=96), dict(metric=1), dict(metric=3),
               dict(metric=1, qq=ptr(qq))):
        assert lib.grl_sq8_scan(*args(**kw)) == _lib.GRL_EINVAL, kw
    torch.cuda.synchronize()
    assert (out == 5.5).all()
    assert lib.grl_sq8_scan(*args()) == 0
    assert np.array_equal(bits(out), bits(D))


# ----------------------------------------------------------------------------
# 8. ATTEvaluator.evaluate with GRL_EVAL_SQ8
# ----------------------------------------------------------------------------
KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_CLUSTER', 'GRL_EVAL_CLUSTER_JACCARD', 'GRL_EVAL_KMEANS', 'GRL_EVAL_HDBSCAN', 'GRL_EVAL_TSNE',
         'GRL_EVAL_SILHOUETTE', 'GRL_EVAL_PCA', 'GRL_EVAL_DIFFUSION', 'GRL_EVAL_SET', 'GRL_EVAL_PQ', 'GRL_EVAL_IVF',
         'GRL_EVAL_REFINE', 'GRL_EVAL_NNG', 'GRL_EVAL_BIN', 'GRL_EVAL_SQ8')


def test_attevaluator_reports_the_index_next_to_the_exact_figures(synth_models, monkeypatch, tmp_path):
    from grl_amd import engine
    from grl_amd.reid.data import get_data
    from grl_amd.reid.evaluator import ATTEvaluator
    cnn, siam, _ = synth_models
    cnn, siam = cnn.to(DEV).eval(), siam.to(DEV).eval()
    _, _, _, q_loader, g_loader = get_data('synthetic', 0, None, 4, 2, 0, 0)
    ev = ATTEvaluator(cnn, siam, only_eval=False)
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    with contextlib.redirect_stdout(io.StringIO()):
        qf, qp, qc = ev.extract_feature(q_loader)
        gf, gp, gc = ev.extract_feature(g_loader)
    gf, gp, gc = torch.cat((qf, gf), 0), np.append(qp, gp), np.append(qc, gc)
    ids = (qp, gp, qc, gc)
    n, d = int(gf.size(0)), int(gf.size(1))
    path = str(tmp_path) + os.sep
    out_file = os.path.join(str(tmp_path), 'sq8.json')

    def run(rerank=0):
        if os.path.exists(out_file):
            os.remove(out_file)
        with contextlib.redirect_stdout(io.StringIO()) as o:
            r = ev.evaluate(None, None, q_loader, g_loader, path, 0, rerank)
        return r, o.getvalue().splitlines(), open(out_file).read() if os.path.exists(out_file) else None

    def refuse(c):
        raise ValueError('not strict JSON: %s' % c)

    index = engine.sq8_index(gf, engine.sq8_train(gf))
    cmc_x, mAP_x = engine.rank_metrics_streaming(qf, gf, *ids)
    k = min(100, n)
    exact = engine.search(qf, gf, k, exclude=ids)[1]
    cmc, mAP = engine.sq8_metrics_streaming(qf, index, *ids)
    recall = engine.topk_recall(engine.sq8_search(qf, index, k, exclude=ids)[1], exact, (1, 10, 100))
    store = engine.RefineStore(gf.contiguous(), 'bf16')
    refined = engine.topk_recall(engine.sq8_refine_search(qf, index, store, 16, 16, exclude=ids)[1], exact, (1, 10, 100))
    for route in ('dense', 'stream'):
        if route == 'stream':
            monkeypatch.setenv('GRL_EVAL_STREAM', '1')
        r_off, text_off, file_off = run()
        assert file_off is None and not any('SQ8' in l for l in text_off), route
        for value, extra_want in (('1', 8), ('1,16,bf16', 9)):
            monkeypatch.setenv('GRL_EVAL_SQ8', value)
            r_on, text_on, raw = run()
            monkeypatch.delenv('GRL_EVAL_SQ8')
            assert r_on == r_off, route
            extra = len(text_on) - len(text_off)
            assert extra == extra_want and text_on[:len(text_off) - 1] == text_off[:-1] and text_on[-1] == text_off[-1], route
            new = text_on[len(text_off) - 1:-1]
            assert new[0] == 'SQ8: {} bytes per row of {}, {} rows'.format(S.dpad(d), 4 * d, n)
            assert new[1] == 'SQ8 Mean AP: {:4.1%} (exact {:4.1%})'.format(mAP, mAP_x)
            assert new[2] == 'SQ8 Rank-{:<3}: {:.1%} (exact {:.1%})'.format(1, cmc[0], cmc_x[0])
            assert new[6] == 'SQ8 recall@1: {:.2%}  @10: {:.2%}  @100: {:.2%}'.format(*recall)
            assert new[-1].startswith('SQ8 index: {} bytes against {} bytes of features'.format(index.nbytes, 4 * n * d))
            js = json.loads(raw, parse_constant=refuse)
            assert js['sq8'] == {'mAP': float(mAP), 'cmc': [float(v) for v in cmc],
                                 'recall': {'1': recall[0], '10': recall[1], '100': recall[2]}}, route
            assert js['exact'] == {'mAP': float(mAP_x), 'cmc': [float(v) for v in cmc_x]}, route
            assert (js['index_bytes'], js['code_bytes'], js['feature_bytes']) == (index.nbytes, n * S.dpad(d), 4 * n * d), route
            assert (js['n'], js['d'], js['dpad'], js['n_queries'], js['k'], js['metric']) == (n, d, S.dpad(d), int(qf.size(0)), k, 'cosine')
            if value == '1':
                assert 'refine' not in js
            else:
                assert new[7] == 'SQ8 refined recall@1: {:.2%}  @10: {:.2%}  @100: {:.2%}  (R = 16, k = 16, bf16 store of {} bytes)'.format(
                    *(tuple(refined) + (store.nbytes,)))
                assert js['refine'] == {'R': 16, 'k': 16, 'store': 'bf16', 'store_bytes': store.nbytes,
                                        'recall': {'1': refined[0], '10': refined[1], '100': refined[2]}}, route
    monkeypatch.delenv('GRL_EVAL_STREAM')
    monkeypatch.setenv('GRL_EVAL_SQ8', '1,16')
    with pytest.raises(ValueError, match='GRL_EVAL_SQ8=1,16 cannot re-rank'):
        run(rerank=1)
    for name, value in (('GRL_EVAL_METRIC', 'verify'), ('GRL_EVAL_SET', 'chamfer'), ('GRL_EVAL_DIFFUSION', '5')):
        monkeypatch.setenv(name, value)
        with pytest.raises(ValueError, match='GRL_EVAL_SQ8=1,16 cannot be combined with %s' % name):
            run()
        with pytest.raises(ValueError, match='GRL_EVAL_SQ8=1,16 cannot be combined with %s' % name):
            ATTEvaluator(cnn, siam, only_eval=True).evaluate(None, None, q_loader, g_loader, path, 0, 0)
        monkeypatch.delenv(name)
