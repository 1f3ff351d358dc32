"""Binary hash codes and Hamming search on the device (engine.BinaryCodebook / bin_train / bin_index / bin_dist /
bin_search / bin_metrics_streaming / bin_refine_search, bin.hip, GRL_EVAL_BIN) against the numpy model of
tests/bin_ref.py.  The codes are the sign bits of the device's own downloaded projections, a Hamming distance is an exact
integer and the asymmetric tables add in a fixed fp32 order, so every comparison of codes and distances is exact."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import bin_ref as B
import pq_ref as R
import search_filter_ref as FR

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NBITS = (32, 64, 96, 256, 1024)
NS = (1, 63, 64, 65, 257, 1000)
NQS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 33)                           # every remainder of grl_bin_scan's tile of 8 queries, and full tiles
MODES = ('hamming', 'asymmetric')


def bits(a):
    if torch.is_tensor(a):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def _rows(n, d, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    x = g.standard_normal((n, d)).astype(np.float32) + np.float32(0.1)
    return torch.from_numpy(x / np.linalg.norm(x, axis=1, keepdims=True)).to(DEV)


def _book(nbits, d=64, seed=0, shift=True):
    from grl_amd import engine
    g = np.random.Generator(np.random.PCG64(1000 + seed + nbits))
    proj = torch.from_numpy(g.standard_normal((nbits, d)).astype(np.float32)).to(DEV)
    sh = torch.from_numpy((0.05 * g.standard_normal(nbits)).astype(np.float32)).to(DEV) if shift else None
    return engine.BinaryCodebook(proj, sh)


def _codes(n, nbits, seed=0, dup=True):
    """random code rows; with ``dup`` about half of the rows repeat an earlier row (ties between gallery entries)"""
    g = np.random.Generator(np.random.PCG64(2000 + seed + nbits))
    c = g.integers(0, 256, (n, nbits // 8)).astype(np.uint8)
    if dup and n > 1:
        src = g.integers(0, n, n)
        take = g.random(n) < 0.5
        c[take] = c[np.minimum(src, np.arange(n))[take]]
    return torch.from_numpy(c).to(DEV)


def _scan(qcodes, index, ldo=None, fill=None):
    """grl_bin_scan of caller-supplied query codes (uint8 [nq, nbits / 8]) over the whole index"""
    from grl_amd import engine
    from grl_amd._lib import ptr
    nq, n = qcodes.shape[0], index.n
    ldo = n if ldo is None else ldo
    out = torch.full((nq, ldo), -7.25 if fill is None else fill, dtype=torch.float32, device=DEV)
    engine._call('grl_bin_scan', ptr(qcodes.contiguous().view(torch.int32)), ptr(index._scan), n, ptr(out), ldo, nq, n,
                 index.nbits)
    return out


# ----------------------------------------------------------------------------
# 1. pack
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('nbits', NBITS)
def test_codes_are_the_sign_bits_of_the_downloaded_projections_in_both_layouts(nbits):
    from grl_amd import engine
    from grl_amd._lib import ptr
    book = _book(nbits, d=40)                                       # d is padded to 64 inside
    for n in NS:
        x = _rows(n, 40, n + nbits)
        z = book.project(x)
        assert tuple(z.shape) == (n, nbits) and z.dtype == torch.float32
        codes, scan = book._pack(z)
        zh = z.cpu().numpy()
        want = B.pack(B.bits_of(zh))
        assert codes.dtype == torch.uint8 and np.array_equal(codes.cpu().numpy(), want), n
        assert tuple(scan.shape) == (nbits // 32, n) and np.array_equal(u32(scan), B.words(want)), n
        assert torch.equal(book.encode(x), codes)
        index = engine.bin_index(x, book)
        assert torch.equal(index.codes, codes) and torch.equal(index._scan, scan) and (index.n, index.nbits) == (n, nbits)
        assert torch.equal(engine.BinaryIndex(book, codes)._scan, scan)               # grl_bin_words agrees
        assert index.nbytes == n * nbits // 8 + 4 * (nbits // 32) * n + 4 * nbits * 40 + 4 * nbits
        # planted special values: NaN, -0, +0 give 0; +inf 1; -inf 0; the smallest subnormals by their sign
        special = np.array([np.nan, -0.0, 0.0, np.inf, -np.inf, 1e-45, -1e-45, -np.nan], dtype=np.float32)
        g = np.random.Generator(np.random.PCG64(n))
        zs = zh.copy()
        for col in sorted(set((0, 7, 31, nbits // 2, nbits - 1))):
            zs[:, col] = special[g.integers(0, 8, n)]
        zs[0, :8] = special
        zd = torch.from_numpy(zs).to(DEV)
        codes, scan = book._pack(zd)
        want = B.pack(B.bits_of(zs))
        assert np.array_equal(codes.cpu().numpy(), want) and np.array_equal(u32(scan), B.words(want)), n
        assert int(codes[0, 0]) == 0b00101000
        # ldz > nbits, ldw > n, and the +-1 signs of the same launch
        ldz, ldw = nbits + 12, n + 5
        wide = torch.full((n, ldz), 3.0, dtype=torch.float32, device=DEV)
        wide[:, :nbits] = zd
        c2 = torch.zeros((n, nbits // 8), dtype=torch.uint8, device=DEV)
        s2 = torch.full((nbits // 32, ldw), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
        sg = torch.full((n, nbits + 4), 9.0, dtype=torch.float32, device=DEV)
        engine._call('grl_bin_pack', ptr(wide), ldz, ptr(c2), ptr(s2), ldw, ptr(sg), nbits + 4, n, nbits)
        assert torch.equal(c2, codes) and torch.equal(s2[:, :n], scan) and (s2[:, n:] == 0x5a5a5a5a).all()
        assert np.array_equal(sg[:, :nbits].cpu().numpy(), np.where(B.bits_of(zs), 1.0, -1.0).astype(np.float32))
        assert (sg[:, nbits:] == 9.0).all()
    assert tuple(book.encode(x[:0]).shape) == (0, nbits // 8) and engine.bin_index(x[:0], book).n == 0


# ----------------------------------------------------------------------------
# 2. Hamming scan
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('nbits', NBITS)
def test_hamming_scan_equals_the_model_on_the_downloaded_codes(nbits):
    from grl_amd import engine
    slab = engine.BIN_SLAB
    book = _book(nbits)
    for i, n in enumerate(NS + (slab - 1, slab, slab + 1)):
        index = engine.BinaryIndex(book, _codes(n, nbits, seed=n))
        gh = index.codes.cpu().numpy()
        for nq in NQS:
            qc = _codes(nq, nbits, seed=31 * nq + n, dup=False)
            qc[0] = index.codes[n // 2]                             # a query that IS a gallery row: distance 0
            got = _scan(qc, index)
            want = B.hamming_words(qc.cpu().numpy(), gh)
            assert np.array_equal(bits(got), bits(want)), (n, nq)
            assert float(got[0, n // 2]) == 0.0
            if (i + nq) % 4 == 0:
                assert np.array_equal(want, B.hamming(qc.cpu().numpy(), gh)), (n, nq)


@pytest.mark.parametrize('nbits', NBITS)
def test_all_zero_and_all_one_codes_give_0_and_nbits(nbits):
    from grl_amd import engine
    book = _book(nbits)
    n = 300
    zero = torch.zeros((n, nbits // 8), dtype=torch.uint8, device=DEV)
    ones = torch.full((n, nbits // 8), 255, dtype=torch.uint8, device=DEV)
    for gal, q, want in ((zero, zero, 0), (ones, ones, 0), (zero, ones, nbits), (ones, zero, nbits)):
        got = _scan(q[:5], engine.BinaryIndex(book, gal))
        assert (got == float(want)).all()


def test_scan_writes_only_its_columns_and_queries_under_a_wider_ldo():
    from grl_amd import engine
    book = _book(96)
    for n, nq, ldo in ((65, 3, 72), (1025, 9, 1031)):
        index = engine.BinaryIndex(book, _codes(n, 96, seed=n))
        qc = _codes(nq + 2, 96, seed=5, dup=False)
        want = B.hamming_words(qc.cpu().numpy()[:nq], index.codes.cpu().numpy())
        out = _scan(qc[:nq], index, ldo=ldo)
        assert np.array_equal(bits(out[:, :n]), bits(want)) and (out[:, n:] == -7.25).all()


@pytest.mark.parametrize('mode', MODES)
def test_dist_of_real_queries_equals_the_models_on_the_downloaded_codes_and_tables(mode):
    from grl_amd import engine
    for nbits, n, nq in ((32, 257, 5), (256, 1000, 33), (1024, 65, 3)):
        book = _book(nbits, d=64)
        gx = _rows(n, 64, 3 + n)
        gx[1::2] = gx[0:-1:2][:gx[1::2].shape[0]]                   # duplicate rows
        index = engine.bin_index(gx, book)
        qf = _rows(nq, 64, 11 + nq)
        D = engine.bin_dist(qf, index, mode)
        assert tuple(D.shape) == (nq, n) and D.dtype == torch.float32
        if mode == 'hamming':
            want = B.hamming_words(book.encode(qf).cpu().numpy(), index.codes.cpu().numpy())
            assert D.min() >= 0 and D.max() <= nbits
        else:
            want = R.adc_dist(book.lut(qf).cpu().numpy(), index.codes.cpu().numpy(), 'cosine')
            # and the tables mean what they say: -sum_b z_q[b] s_g[b], here in float64 from the downloaded z
            ref = B.asym64(book.project(qf).cpu().numpy(), B.unpack(index.codes.cpu().numpy()))
            assert np.abs(D.cpu().numpy() - ref).max() <= nbits * 2.0 ** -22 * np.abs(book.project(qf).cpu().numpy()).max()
        assert np.array_equal(bits(D), bits(want)), (nbits, n, nq)
        for bc in (1, 64, 257, n):
            assert np.array_equal(bits(engine.bin_dist(qf, index, mode, block_cols=bc)), bits(D)), bc
        assert np.array_equal(bits(engine.bin_dist(qf, index, mode, block_bytes=1)), bits(D))


# ----------------------------------------------------------------------------
# 3. asymmetric tables
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('nbits', NBITS)
def test_tables_equal_the_model_on_the_downloaded_projections_bit_for_bit(nbits):
    from grl_amd import engine
    from grl_amd._lib import ptr
    book = _book(nbits)
    for nq in (1, 3, 33):
        qf = _rows(nq, 64, 7 + nq)
        lut = book.lut(qf)
        assert tuple(lut.shape) == (nq, nbits // 8, 256) and lut.dtype == torch.float32
        z = book.project(qf)
        assert np.array_equal(bits(lut), bits(B.lut(z.cpu().numpy()))), nq
        # a NaN query column, infinities and signed zeros, through the kernel's own entry point (ldz > nbits)
        ldz = nbits + 8
        zs = torch.zeros((nq, ldz), dtype=torch.float32, device=DEV)
        zs[:, :nbits] = z
        zs[0, 9], zs[0, 16], zs[0, 17], zs[0, 24], zs[0, 25] = float('nan'), float('inf'), float('inf'), 0.0, -0.0
        zs[nq - 1, nbits - 1] = float('-inf')
        out = torch.empty((nq, nbits // 8, 256), dtype=torch.float32, device=DEV)
        engine._call('grl_bin_lut', ptr(zs), ldz, ptr(out), nq, nbits)
        assert np.array_equal(bits(out), bits(B.lut(zs[:, :nbits].cpu().numpy()))), nq
        assert torch.isnan(out[0, 1]).all() and not torch.isnan(out[0, 0]).any()
        assert torch.isnan(out[0, 2]).sum() == 128                  # inf - inf where the two bits differ
    assert tuple(book.lut(qf[:0]).shape) == (0, nbits // 8, 256)


# ----------------------------------------------------------------------------
# 4. search and metrics
# ----------------------------------------------------------------------------
_cache = {}


def search_case(mode):
    """33 queries against 300 code rows with duplicates, 64 bits; D = the materialised matrix, its ranking and ids.  Built
    once per mode, never modified."""
    from grl_amd import engine
    if mode not in _cache:
        book = _book(64, d=64, seed=3)
        gx = _rows(300, 64, 17)
        gx[1::2] = gx[0:-1:2]
        index = engine.bin_index(gx, book)
        qf = _rows(33, 64, 19)
        D = engine.bin_dist(qf, index, mode)
        g = np.random.Generator(np.random.PCG64(77))
        ids = (g.integers(0, 12, 33), g.integers(0, 12, 300), g.integers(0, 3, 33), g.integers(0, 3, 300))
        _cache[mode] = (index, qf, D, engine.rank_rows(D), ids)
    return _cache[mode]


@pytest.mark.parametrize('mode', MODES)
def test_search_is_the_head_of_the_ranked_matrix_with_ties_to_the_smaller_index(mode):
    from grl_amd import engine
    index, qf, D, order, ids = search_case(mode)
    Dn, n = D.cpu().numpy(), index.n
    assert (np.diff(np.sort(Dn, axis=1), axis=1) == 0).any(axis=1).all()           # ties in every row
    for k in (1, 10, 1024):                                        # 1024 > n = 300: padding
        dv, di = engine.bin_search(qf, index, k, mode)
        assert tuple(dv.shape) == (33, k) and di.dtype == torch.int64
        kk = min(k, n)
        want_i = order[:, :kk].cpu().numpy().astype(np.int64)
        assert np.array_equal(di[:, :kk].cpu().numpy(), want_i), k
        assert np.array_equal(bits(dv[:, :kk]), bits(np.take_along_axis(Dn, want_i, 1))), k
        assert (di[:, kk:] == -1).all() and torch.isinf(dv[:, kk:]).all() and (dv[:, kk:] > 0).all()
        mv, mi = R.search(Dn, k)
        assert np.array_equal(di.cpu().numpy(), mi) and np.array_equal(bits(dv), bits(mv)), k
        dv, di = engine.bin_search(qf, index, k, mode, exclude=ids)
        wv, wi = FR.filtered_topk(Dn, k, *ids)
        assert np.array_equal(di.cpu().numpy(), wi) and np.array_equal(bits(dv), bits(wv)), k


@pytest.mark.parametrize('mode', MODES)
def test_every_blocking_of_columns_and_queries_gives_the_same_bits(mode, monkeypatch):
    from grl_amd import engine
    index, qf, D, order, ids = search_case(mode)
    d0, i0 = engine.bin_search(qf, index, 10, mode)
    for bc in (1, 64, 257, index.n):
        dv, di = engine.bin_search(qf, index, 10, mode, block_cols=bc)
        assert np.array_equal(bits(dv), bits(d0)) and torch.equal(di, i0), bc
    dv, di = engine.bin_search(qf, index, 10, mode, block_bytes=1)
    assert np.array_equal(bits(dv), bits(d0)) and torch.equal(di, i0)
    # forced chunking of the queries: the grid's limit ('hamming'), the table budget ('asymmetric': 8 * 256 * 4 = 8192
    # bytes per query, row blocks of 4 and of 1)
    if mode == 'hamming':
        limits = [('BIN_NQ_MAX', 8), ('BIN_NQ_MAX', 1)]
    else:
        limits = [('PQ_LUT_BYTES', 4 * 8192 + 17), ('PQ_LUT_BYTES', 1)]
    for name, limit in limits:
        for kw in (dict(), dict(exclude=ids), dict(block_cols=64)):
            dw, iw = engine.bin_search(qf, index, 10, mode, **kw)
            monkeypatch.setattr(engine, name, limit)
            dv, di = engine.bin_search(qf, index, 10, mode, **kw)
            Dv = engine.bin_dist(qf, index, mode)
            monkeypatch.undo()
            assert np.array_equal(bits(dv), bits(dw)) and torch.equal(di, iw), (limit, kw)
            assert np.array_equal(bits(Dv), bits(D)), limit
    if mode == 'asymmetric':
        monkeypatch.setattr(engine, 'PQ_LUT_BYTES', 4 * 8192)
        with pytest.raises(ValueError, match=r'bin_metrics_streaming.*270336 bytes.*GRL_PQ_LUT_BYTES'):
            engine.bin_metrics_streaming(qf, index, *ids, mode=mode)


@pytest.mark.parametrize('mode', MODES)
def test_empty_queries_and_an_empty_gallery(mode):
    from grl_amd import engine
    index, qf, D, order, ids = search_case(mode)
    dv, di = engine.bin_search(qf[:0], index, 5, mode)
    assert tuple(dv.shape) == (0, 5) and tuple(di.shape) == (0, 5)
    assert tuple(engine.bin_dist(qf[:0], index, mode).shape) == (0, 300)
    empty = engine.bin_index(qf[:0], index.codebook)
    dv, di = engine.bin_search(qf, empty, 5, mode)
    assert (di == -1).all() and torch.isinf(dv).all() and tuple(dv.shape) == (33, 5)
    assert tuple(engine.bin_dist(qf, empty, mode).shape) == (33, 0)


@pytest.mark.parametrize('mode', MODES)
def test_streaming_metrics_equal_the_matrix_consumers(mode):
    from grl_amd import engine
    index, qf, D, order, ids = search_case(mode)
    cmc, mAP = engine.rank_metrics(order, *ids, max_rank=50)
    for bc in (None, 64):                                          # one pass, two passes
        c2, m2 = engine.bin_metrics_streaming(qf, index, *ids, mode=mode, max_rank=50, block_cols=bc)
        assert np.array_equal(c2, cmc), bc
        assert abs(m2 - mAP) <= 1e-6, bc                           # fp64, another summation order


# ----------------------------------------------------------------------------
# 5. refine, 6. training: the recipe of tests/bin_ref.py
# ----------------------------------------------------------------------------
_trained = {}


def trained(seed):
    """the recipe's gallery and queries on the device, the ITQ and LSH codebooks, their indexes and the exact lists"""
    from grl_amd import engine
    if seed not in _trained:
        r = B.RECIPE
        gal, qry = B.recipe(seed)
        tg, tq = torch.from_numpy(gal).to(DEV), torch.from_numpy(qry).to(DEV)
        itq = engine.bin_train(tg, r['nbits'], 'itq', r['n_iter'], seed)
        lsh = engine.bin_train(tg, r['nbits'], 'lsh', r['n_iter'], seed)
        exact = engine.search(tq, tg, 10)[1]
        _trained[seed] = (tg, tq, itq, lsh, engine.bin_index(tg, itq), engine.bin_index(tg, lsh), exact)
    return _trained[seed]


@pytest.mark.parametrize('seed', (0, 1, 2))
def test_training_on_the_recipe(seed):
    from grl_amd import engine
    r = B.RECIPE
    nbits = r['nbits']
    tg, tq, itq, lsh, i_itq, i_lsh, exact = trained(seed)
    # LSH: the host draw, centred on pca's mean
    host = np.random.Generator(np.random.PCG64(seed)).standard_normal((nbits, r['d'])).astype(np.float32)
    assert np.array_equal(bits(lsh.proj), bits(host)) and (lsh.method, lsh.seed, lsh.objective) == ('lsh', seed, None)
    p = engine.pca(tg, nbits, seed=seed)
    want_shift = -(host.astype(np.float64) @ p.mean.cpu().numpy().astype(np.float64))
    assert np.abs(lsh.shift.cpu().numpy() - want_shift).max() <= 1e-5
    # ITQ: the objective rises, the projection stays orthonormal, centred as well
    assert (itq.method, itq.n_iter, itq.seed, itq.nbits, itq.d) == ('itq', r['n_iter'], seed, nbits, r['d'])
    assert len(itq.objective) == r['n_iter'] and itq.objective[-1] > itq.objective[0]
    eye = np.eye(nbits)
    pj, pc = itq.proj.cpu().numpy().astype(np.float64), p.components.cpu().numpy().astype(np.float64)
    err, err_pca = np.abs(pj @ pj.T - eye).max(), np.abs(pc @ pc.T - eye).max()
    print('seed %d: max|proj proj^T - I| = %.3e, pca components %.3e, objective %.2f -> %.2f'
          % (seed, err, err_pca, itq.objective[0], itq.objective[-1]))
    assert err <= 8 * err_pca
    want_shift = -(pj @ p.mean.cpu().numpy().astype(np.float64))
    assert np.abs(itq.shift.cpu().numpy() - want_shift).max() <= 1e-5
    # quality: the orderings of the issue's table
    rec = {}
    for name, index in (('itq', i_itq), ('lsh', i_lsh)):
        for mode in MODES:
            rec[name, mode] = engine.topk_recall(engine.bin_search(tq, index, 10, mode)[1], exact, (10,))[0]
    print('seed %d: recall@10 %s' % (seed, rec))
    assert rec['itq', 'hamming'] > rec['lsh', 'hamming']
    assert rec['itq', 'asymmetric'] >= rec['itq', 'hamming']
    # the same bits from a second run
    again = engine.bin_train(tg, nbits, 'itq', r['n_iter'], seed)
    assert np.array_equal(bits(again.proj), bits(itq.proj)) and np.array_equal(bits(again.shift), bits(itq.shift))
    assert again.objective == itq.objective and torch.equal(again.encode(tg), i_itq.codes)
    assert torch.equal(engine.bin_train(tg, nbits, 'lsh', 1, seed).encode(tg), i_lsh.codes)


def test_training_refuses_what_pca_refuses():
    from grl_amd import engine
    x = _rows(40, 64, 1)
    with pytest.raises(ValueError, match='pca: L = n_components \\+ oversample = 42 must be at most'):
        engine.bin_train(x, 32)                                     # n - 1 = 39 < 42
    with pytest.raises(ValueError, match='pca: L = n_components'):
        engine.bin_train(_rows(200, 64, 1), 64)                     # d = 64 < 74
    book = engine.bin_train(x, 64, 'lsh')                           # LSH has no such limit
    assert (book.nbits, book.d) == (64, 64)


@pytest.mark.parametrize('mode', MODES)
def test_refine_is_its_stated_composition_and_does_not_lose_recall(mode):
    from grl_amd import engine
    tg, tq, itq, lsh, index, _, exact = trained(0)
    g = np.random.Generator(np.random.PCG64(5))
    ids = (g.integers(0, 50, 64), np.arange(1000) % 50, g.integers(0, 3, 64), g.integers(0, 3, 1000))
    for dtype in ('f32', 'bf16'):
        store = engine.RefineStore(tg, dtype)
        for k, Rr, ex in ((10, 100, None), (10, 10, None), (5, 64, ids)):
            dv, di = engine.bin_refine_search(tq, index, store, k, Rr, mode, exclude=ex)
            cand = engine.bin_search(tq, index, Rr, mode, exclude=ex)[1]
            wv, wi = engine.refine_lists(tq, store, cand, k, 'cosine')
            assert np.array_equal(bits(dv), bits(wv)) and torch.equal(di, wi), (dtype, k, Rr)
    store = engine.RefineStore(tg)
    plain = engine.topk_recall(engine.bin_search(tq, index, 10, mode)[1], exact, (10,))[0]
    for Rr in (10, 100):
        refined = engine.topk_recall(engine.bin_refine_search(tq, index, store, 10, Rr, mode)[1], exact, (10,))[0]
        assert refined >= plain, (Rr, refined, plain)


# ----------------------------------------------------------------------------
# 7. ATTEvaluator.evaluate with GRL_EVAL_BIN
# ----------------------------------------------------------------------------
KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_CLUSTER', 'GRL_EVAL_CLUSTER_JACCARD', 'GRL_EVAL_KMEANS', 'GRL_EVAL_HDBSCAN', 'GRL_EVAL_TSNE',
         'GRL_EVAL_SILHOUETTE', 'GRL_EVAL_PCA', 'GRL_EVAL_DIFFUSION', 'GRL_EVAL_SET', 'GRL_EVAL_PQ', 'GRL_EVAL_IVF',
         'GRL_EVAL_REFINE', 'GRL_EVAL_NNG', 'GRL_EVAL_BIN')


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
    out_file = os.path.join(str(tmp_path), 'bin.json')

    def run(rerank=0):
        if os.path.exists(out_file):
            os.remove(out_file)
        with contextlib.redirect_stdout(io.StringIO()) as o:
            r = ev.evaluate(None, None, q_loader, g_loader, path, 0, rerank)
        return r, o.getvalue().splitlines(), open(out_file).read() if os.path.exists(out_file) else None

    def refuse(c):
        raise ValueError('not strict JSON: %s' % c)

    book = engine.bin_train(gf, 32, 'itq', 5, 1)
    index = engine.bin_index(gf, book)
    cmc_x, mAP_x = engine.rank_metrics_streaming(qf, gf, *ids)
    k = min(100, n)
    exact = engine.search(qf, gf, k, exclude=ids)[1]
    want = {}
    for mode in MODES:
        cmc, mAP = engine.bin_metrics_streaming(qf, index, *ids, mode=mode)
        want[mode] = (cmc, mAP, engine.topk_recall(engine.bin_search(qf, index, k, mode, exclude=ids)[1], exact, (1, 10, 100)))
    for route in ('dense', 'stream'):
        if route == 'stream':
            monkeypatch.setenv('GRL_EVAL_STREAM', '1')
        r_off, text_off, file_off = run()
        assert file_off is None and not any('BIN' in l or 'Hamming' in l or 'Asymmetric' in l for l in text_off), route
        monkeypatch.setenv('GRL_EVAL_BIN', '32,itq,5,1')
        r_on, text_on, raw = run()
        monkeypatch.delenv('GRL_EVAL_BIN')
        assert r_on == r_off, route
        extra = len(text_on) - len(text_off)
        assert extra == 14 and text_on[:len(text_off) - 1] == text_off[:-1] and text_on[-1] == text_off[-1], route
        new = text_on[len(text_off) - 1:-1]
        assert new[0] == 'BIN: 32 bits by itq (4 bytes per row of {}), {} rows'.format(4 * d, n)
        for j, (mode, tag) in enumerate((('hamming', 'Hamming'), ('asymmetric', 'Asymmetric'))):
            cmc, mAP, recall = want[mode]
            part = new[1 + 6 * j:7 + 6 * j]
            assert part[0] == '{} Mean AP: {:4.1%} (exact {:4.1%})'.format(tag, mAP, mAP_x)
            assert part[1] == '{} Rank-{:<3}: {:.1%} (exact {:.1%})'.format(tag, 1, cmc[0], cmc_x[0])
            assert part[5] == '{} recall@1: {:.2%}  @10: {:.2%}  @100: {:.2%}'.format(tag, *recall)
        assert new[13].startswith('BIN index: {} bytes against {} bytes of features'.format(index.nbytes, 4 * n * d))
        js = json.loads(raw, parse_constant=refuse)
        for mode in MODES:
            cmc, mAP, recall = want[mode]
            assert js[mode] == {'mAP': float(mAP), 'cmc': [float(v) for v in cmc],
                                'recall': {'1': recall[0], '10': recall[1], '100': recall[2]}}, (route, mode)
        assert js['exact'] == {'mAP': float(mAP_x), 'cmc': [float(v) for v in cmc_x]}, route
        assert (js['index_bytes'], js['code_bytes'], js['feature_bytes']) == (index.nbytes, 4 * n, 4 * n * d), route
        assert (js['nbits'], js['method'], js['n_iter'], js['seed'], js['n'], js['n_queries']) == (32, 'itq', 5, 1, n, int(qf.size(0)))
        assert js['objective'] == book.objective and len(js['objective']) == 5
    monkeypatch.delenv('GRL_EVAL_STREAM')
    monkeypatch.setenv('GRL_EVAL_BIN', '32,lsh')
    with pytest.raises(ValueError, match='GRL_EVAL_BIN=32,lsh cannot re-rank'):
        run(rerank=1)
    for name, value in (('GRL_EVAL_METRIC', 'verify'), ('GRL_EVAL_SET', 'chamfer'), ('GRL_EVAL_DIFFUSION', '5')):
        monkeypatch.setenv(name, value)
        with pytest.raises(ValueError, match='GRL_EVAL_BIN=32,lsh cannot be combined with %s' % name):
            run()
        with pytest.raises(ValueError, match='GRL_EVAL_BIN=32,lsh cannot be combined with %s' % name):
            ATTEvaluator(cnn, siam, only_eval=True).evaluate(None, None, q_loader, g_loader, path, 0, 0)
        monkeypatch.delenv(name)
    monkeypatch.setenv('GRL_EVAL_BIN', '256')                      # 256 + 10 components from 75 rows: pca's own error
    with pytest.raises(ValueError, match='pca: L = n_components'):
        run()
