"""Product-quantised gallery index and ADC search on the device (engine.PqCodebook / pq_train / pq_index / pq_dist /
pq_search / pq_metrics_streaming, pq.hip, GRL_EVAL_PQ) against the numpy model of tests/pq_ref.py.  The
tables are the NEGDOT GEMM's bits and the scan adds the selected entries in a fixed fp32 order, so every comparison of
distances is exact (bit patterns); the codes are integers derived from the bits of the device's own distance blocks."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import pq_ref as R
import search_filter_ref as FR

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
METRICS = ('cosine', 'euclidean')


def bits(a):
    if torch.is_tensor(a):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rows(n, d, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    x = g.standard_normal((n, d)).astype(np.float32)
    return torch.from_numpy(x / np.linalg.norm(x, axis=1, keepdims=True)).to(DEV)


def _book(M, ksub, dsub, metric='cosine', seed=0):
    from grl_amd import engine
    g = np.random.Generator(np.random.PCG64(1000 + seed + M))
    return engine.PqCodebook(torch.from_numpy(g.standard_normal((M, ksub, dsub)).astype(np.float32) * 0.2).to(DEV), metric)


def _codes(n, M, ksub, seed=0, dup=True):
    """random codes; with ``dup`` about half of the rows repeat an earlier row (ties between gallery entries)"""
    g = np.random.Generator(np.random.PCG64(2000 + seed + M))
    c = g.integers(0, ksub, (n, M)).astype(np.uint8)
    if dup and n > 1:
        src = g.integers(0, n, n)
        take = g.random(n) < 0.5
        c[take] = c[np.minimum(src, np.arange(n))[take]]
    return torch.from_numpy(c).to(DEV)


def _sqnorm(x):
    from grl_amd import engine
    from grl_amd._lib import ptr
    x = x.contiguous()
    out = torch.empty(x.shape[0], dtype=torch.float32, device=DEV)
    engine._call('grl_row_sqnorm', ptr(x), ptr(out), x.shape[0], x.shape[1], x.shape[1])
    return out


def _model(blocks, index):
    """the numpy model on the DOWNLOADED tables (and query norms) of a block source"""
    book = index.codebook
    rn = blocks.rn.cpu().numpy() if blocks.rn is not None else None
    return R.adc_dist(blocks.lut.cpu().numpy(), index.codes.cpu().numpy(), book.metric, rn)


# ----------------------------------------------------------------------------
# 1. tables
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('d,M', [(256, 1), (256, 2), (256, 4), (256, 8), (160, 5)])
def test_tables_are_the_negdot_gemm_bits_and_the_euclidean_form(d, M):
    from grl_amd import engine
    dsub = d // M
    for ksub in (16, 256):
        book, book_e = _book(M, ksub, dsub), _book(M, ksub, dsub, 'euclidean')
        assert (book.M, book.ksub, book.dsub, book.d, book.metric) == (M, ksub, dsub, d, 'cosine')
        for nq in (1, 3, 33):
            qf = _rows(nq, d, 7 + nq)
            lut, lut_e = book.lut(qf), book_e.lut(qf)
            assert tuple(lut.shape) == (nq, M, ksub) and lut.dtype == torch.float32
            for m in range(M):
                g = engine.cosin_dist(qf[:, m * dsub:(m + 1) * dsub].contiguous(), book.codebooks[m]).cpu().numpy()
                assert np.array_equal(bits(lut[:, m]), bits(g)), (ksub, nq, m)
                cn = _sqnorm(book.codebooks[m]).cpu().numpy()
                want = (cn[None, :] + (np.float32(2) * g).astype(np.float32)).astype(np.float32)
                assert np.array_equal(bits(lut_e[:, m]), bits(want)), (ksub, nq, m)
    assert tuple(book.lut(qf[:0]).shape) == (0, M, 256)


# ----------------------------------------------------------------------------
# 2. scan
# ----------------------------------------------------------------------------
NS = (1, 63, 64, 65, 257, 1000)
NQS = (1, 2, 3, 5, 33)


def _scan_case(M, ksub, n, nq, metric, seed=0):
    from grl_amd import engine
    book = _book(M, ksub, 32, metric, seed)
    index = engine.PqIndex(book, _codes(n, M, ksub, seed + n))
    return index, _rows(nq, 32 * M, seed + 31 * nq + n)


@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('M', [1, 2, 3, 4, 5, 7, 8, 13])
def test_scan_equals_the_model_on_the_downloaded_tables(M, metric):
    from grl_amd import engine
    for i, n in enumerate(NS):
        for j, nq in enumerate(NQS):
            index, qf = _scan_case(M, (16, 256, 64)[(i + j) % 3], n, nq, metric)
            blocks = engine._PqBlocks(qf, index, block_cols=n)
            got = blocks.block(0, n)
            assert tuple(got.shape) == (nq, n)
            assert np.array_equal(bits(got), bits(_model(blocks, index))), (n, nq)
            assert np.array_equal(bits(engine.pq_dist(qf, index)), bits(got)), (n, nq)


@pytest.mark.parametrize('metric', METRICS)
def test_scan_over_several_slabs_and_with_forced_chunking(metric):
    from grl_amd import engine
    # 4100 columns: three workgroups along the gallery, the last one ragged
    index, qf = _scan_case(5, 256, 4100, 5, metric)
    blocks = engine._PqBlocks(qf, index, block_cols=4100)
    assert np.array_equal(bits(blocks.block(0, 4100)), bits(_model(blocks, index)))
    # M = 192 at d = 6144: one query's table is 192 KiB, more than a CU's LDS
    index, qf = _scan_case(192, 256, 257, 5, metric)
    assert index.codebook.d == 6144
    blocks = engine._PqBlocks(qf, index, block_cols=257)
    assert np.array_equal(bits(blocks.block(0, 257)), bits(_model(blocks, index)))


@pytest.mark.parametrize('metric', METRICS)
def test_scan_follows_ieee_on_nan_and_infinite_table_entries(metric):
    from grl_amd import engine
    M, ksub, n, nq = 7, 16, 257, 5
    index, qf = _scan_case(M, ksub, n, nq, metric)
    blocks = engine._PqBlocks(qf, index, block_cols=n)
    clean = blocks.block(0, n).clone()
    lut = blocks.lut
    lut[0, 2, 3] = float('nan')
    lut[1, 0, 5], lut[1, 4, 5] = float('inf'), float('inf')            # same partial: +inf
    lut[2, 1, 7], lut[2, 6, 7] = float('inf'), float('-inf')           # partials 1 and 2: inf - inf where both are picked
    lut[3, 3, 1] = float('-inf')
    got = blocks.block(0, n)
    want = _model(blocks, index)
    assert np.array_equal(bits(got), bits(want))
    codes = index.codes.cpu().numpy()
    hit = codes[:, 2] == 3
    assert hit.any() and (~hit).any()
    if metric == 'cosine':
        assert np.isnan(got[0].cpu().numpy()[hit]).all()
    else:
        assert (got[0].cpu().numpy()[hit] == np.sqrt(np.float32(1e-12))).all()       # the clamp's rule for a NaN
    assert np.array_equal(bits(got[0].cpu().numpy()[~hit]), bits(clean[0].cpu().numpy()[~hit]))
    assert np.array_equal(bits(got[4]), bits(clean[4]))                # the untouched query


@pytest.mark.parametrize('metric', METRICS)
def test_scan_writes_only_its_columns_under_a_wider_ldo(metric):
    from grl_amd import engine
    from grl_amd._lib import ptr
    M, ksub, n, nq, ldo = 5, 64, 65, 3, 72
    index, qf = _scan_case(M, ksub, n, nq, metric)
    blocks = engine._PqBlocks(qf, index, block_cols=n)
    want = blocks.block(0, n).clone()
    out = torch.full((nq, ldo), -7.25, dtype=torch.float32, device=DEV)
    engine._call('grl_pq_scan', ptr(blocks.lut), ptr(index._scan), ptr(out), nq, n, M, ksub, ldo,
                 engine.PQ_METRICS[metric], ptr(blocks.rn))
    assert np.array_equal(bits(out[:, :n]), bits(want))
    assert (out[:, n:] == -7.25).all()


# ----------------------------------------------------------------------------
# 3. block invariance, 4. search order
# ----------------------------------------------------------------------------
_cache = {}


def search_case(metric):
    """33 queries against 300 code rows with duplicates, M = 5, ksub = 16; D = the materialised ADC matrix, its ranking
    and ids.  Built once per metric, never modified."""
    from grl_amd import engine
    if metric not in _cache:
        index, qf = _scan_case(5, 16, 300, 33, metric, seed=3)
        D = engine.pq_dist(qf, index)
        g = np.random.Generator(np.random.PCG64(77))
        ids = (g.integers(0, 12, 33), g.integers(0, 12, 300), g.integers(0, 3, 33), g.integers(0, 3, 300))
        _cache[metric] = (index, qf, D, engine.rank_rows(D), ids)
    return _cache[metric]


@pytest.mark.parametrize('metric', METRICS)
def test_every_blocking_gives_the_same_bits(metric, monkeypatch):
    from grl_amd import engine
    index, qf, D, order, ids = search_case(metric)
    n = index.n
    d0, i0 = engine.pq_search(qf, index, 10)
    for bc in (1, 64, 257, n):
        assert np.array_equal(bits(engine.pq_dist(qf, index, block_cols=bc)), bits(D)), bc
        dv, di = engine.pq_search(qf, index, 10, block_cols=bc)
        assert np.array_equal(bits(dv), bits(d0)) and torch.equal(di, i0), bc
    assert np.array_equal(bits(engine.pq_dist(qf, index, block_bytes=1)), bits(D))
    # tables of 5 * 16 * 4 = 320 bytes per query: 33 queries in row blocks of 4 (and of 1)
    for limit in (4 * 320 + 17, 1):
        monkeypatch.setattr(engine, 'PQ_LUT_BYTES', limit)
        for kw in (dict(), dict(exclude=ids), dict(block_cols=64)):
            dv, di = engine.pq_search(qf, index, 10, **kw)
            monkeypatch.setattr(engine, 'PQ_LUT_BYTES', 1 << 30)
            dw, iw = engine.pq_search(qf, index, 10, **kw)
            monkeypatch.setattr(engine, 'PQ_LUT_BYTES', limit)
            assert np.array_equal(bits(dv), bits(dw)) and torch.equal(di, iw), (limit, kw)
        with pytest.raises(ValueError, match=r'pq_metrics_streaming.*10560 bytes.*GRL_PQ_LUT_BYTES'):
            engine.pq_metrics_streaming(qf, index, *ids)


@pytest.mark.parametrize('metric', METRICS)
def test_search_is_the_head_of_the_ranked_matrix_with_ties_to_the_smaller_index(metric):
    from grl_amd import engine
    index, qf, D, order, ids = search_case(metric)
    Dn, n = D.cpu().numpy(), index.n
    codes = index.codes.cpu().numpy()
    assert np.unique(codes, axis=0).shape[0] < n                   # duplicate code rows: equal distances
    assert (np.diff(np.sort(Dn, axis=1), axis=1) == 0).any(axis=1).all()
    for k in (1, 10, 1024):                                        # 1024 > n = 300: padding
        dv, di = engine.pq_search(qf, index, k)
        assert tuple(dv.shape) == (33, k) and di.dtype == torch.int64
        kk = min(k, n)
        want_i = order[:, :kk].cpu().numpy().astype(np.int64)
        assert np.array_equal(di[:, :kk].cpu().numpy(), want_i), k
        assert np.array_equal(bits(dv[:, :kk]), bits(np.take_along_axis(Dn, want_i, 1))), k
        assert (di[:, kk:] == -1).all() and torch.isinf(dv[:, kk:]).all() and (dv[:, kk:] > 0).all()
        mv, mi = R.search(Dn, k)
        assert np.array_equal(di.cpu().numpy(), mi) and np.array_equal(bits(dv), bits(mv)), k
    for k in (1, 10, 1024):
        dv, di = engine.pq_search(qf, index, k, exclude=ids)
        wv, wi = FR.filtered_topk(Dn, k, *ids)
        assert np.array_equal(di.cpu().numpy(), wi) and np.array_equal(bits(dv), bits(wv)), k


def test_search_with_k_1024_below_the_gallery_size():
    from grl_amd import engine
    index, qf = _scan_case(4, 16, 1500, 3, 'cosine', seed=5)
    D = engine.pq_dist(qf, index)
    order = engine.rank_rows(D)[:, :1024].cpu().numpy().astype(np.int64)
    dv, di = engine.pq_search(qf, index, 1024, block_cols=257)
    assert np.array_equal(di.cpu().numpy(), order)
    assert np.array_equal(bits(dv), bits(np.take_along_axis(D.cpu().numpy(), order, 1)))


# ----------------------------------------------------------------------------
# 5. metrics
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('metric', METRICS)
def test_streaming_metrics_equal_the_matrix_consumers(metric):
    from grl_amd import engine
    index, qf, D, order, ids = search_case(metric)
    cmc, mAP = engine.rank_metrics(order, *ids, max_rank=50)
    for bc in (None, 64):                                          # one pass, two passes
        c2, m2 = engine.pq_metrics_streaming(qf, index, *ids, max_rank=50, block_cols=bc)
        assert np.array_equal(c2, cmc), bc
        assert abs(m2 - mAP) <= 1e-6, bc                           # fp64, another summation order


# ----------------------------------------------------------------------------
# 6. encode / decode
# ----------------------------------------------------------------------------
def test_encode_is_kmeans_assign_per_subspace_and_decode_is_a_gather():
    from grl_amd import engine
    M, ksub, dsub, n = 5, 16, 32, 301
    book = _book(M, ksub, dsub)
    book.codebooks[2, 9] = book.codebooks[2, 4]                    # a tie inside a codebook
    g = np.random.Generator(np.random.PCG64(11))
    x = book.decode(_codes(n, M, ksub, dup=False)) + torch.from_numpy(
        (0.05 * g.standard_normal((n, M * dsub))).astype(np.float32)).to(DEV)
    x[:40] = book.decode(_codes(40, M, ksub, seed=9, dup=False))   # rows that ARE centroids: exact ties at (4, 9)
    x[7, 33] = float('nan')                                        # one NaN entry: subspace 1 of row 7
    x[8] = float('nan')
    codes = book.encode(x)
    assert codes.dtype == torch.uint8 and tuple(codes.shape) == (n, M)
    for m in range(M):
        lab = engine.kmeans_assign(x[:, m * dsub:(m + 1) * dsub].contiguous(), book.codebooks[m], 'euclidean')[0]
        assert torch.equal(codes[:, m].to(torch.int64), lab), m
    assert not (codes[:, 2] == 9).any() and (codes[:40, 2] == 4).any()
    assert int(codes[7, 1]) == 0 and (codes[8] == 0).all()         # the clamp turns a NaN row into a tie at 1e-12
    index = engine.pq_index(x, book)
    assert torch.equal(index.codes, codes) and index.n == n
    assert torch.equal(index._scan, engine.PqIndex(book, codes)._scan)
    assert index.nbytes == n * M + 4 * 2 * n + 4 * M * ksub * dsub
    dec = book.decode(codes)
    want = R.decode(codes.cpu().numpy(), book.codebooks.cpu().numpy())
    assert np.array_equal(bits(dec), bits(want))
    assert tuple(book.encode(x[:0]).shape) == (0, M) and tuple(book.decode(codes[:0]).shape) == (0, M * dsub)
    bad = codes.clone()
    bad[300, 4] = ksub
    with pytest.raises(ValueError, match=r'PqIndex: codes must be in 0..ksub-1 = 0..15'):
        engine.PqIndex(book, bad)
    with pytest.raises(ValueError, match=r'decode: codes must be in 0..ksub-1'):
        book.decode(bad)
    for wrong in (codes.to(torch.int32), codes[:, :4], codes.cpu(), codes.view(-1)):
        with pytest.raises(ValueError, match='codes must be a uint8 device tensor'):
            engine.PqIndex(book, wrong)
    with pytest.raises(ValueError, match=r'xf must be \[rows, d\]'):
        book.encode(x[:, :128])


# ----------------------------------------------------------------------------
# 7. train
# ----------------------------------------------------------------------------
def test_train_is_one_euclidean_kmeans_per_subspace():
    from grl_amd import engine
    n, d, M, nbits = 301, 128, 4, 4
    g = np.random.Generator(np.random.PCG64(13))
    x = torch.from_numpy(g.standard_normal((n, d)).astype(np.float32)).to(DEV)
    for metric in METRICS:
        book = engine.pq_train(x, M=M, nbits=nbits, metric=metric, seed=3)
        assert (book.M, book.ksub, book.dsub, book.d, book.metric) == (4, 16, 32, 128, metric)
        for m in range(M):
            km = engine.kmeans(x[:, 32 * m:32 * (m + 1)].contiguous(), 16, 'euclidean', 'random', 3 + m, 25)
            assert np.array_equal(bits(book.codebooks[m]), bits(km.centroids)), m
            assert (book.n_iter[m], book.converged[m], book.inertia[m]) == (km.n_iter, km.converged, km.inertia)
    with pytest.raises(ValueError, match='pq_train: xf needs at least ksub = 2\\*\\*nbits = 16 rows'):
        engine.pq_train(x[:15], 4, 4)
    with pytest.raises(ValueError, match='pq_train: M must divide'):
        engine.pq_train(x, 3, 4)
    with pytest.raises(ValueError, match='pq_train: M must be an integer'):
        engine.pq_train(x, 0, 4)
    with pytest.raises(ValueError, match='pq_train: dsub = d / M must be a multiple of 32'):
        engine.pq_train(x, 8, 4)
    for nb in (3, 9, 4.0, True):
        with pytest.raises(ValueError, match='pq_train: nbits must be an integer in 4..8'):
            engine.pq_train(x, 4, nb)
    with pytest.raises(ValueError, match='pq_train: max_iter'):
        engine.pq_train(x, 4, 4, max_iter=0)
    with pytest.raises(ValueError, match='pq_train: seed'):
        engine.pq_train(x, 4, 4, seed=-1)
    with pytest.raises(ValueError, match='ksub must be 2\\*\\*nbits'):
        engine.PqCodebook(torch.zeros((4, 24, 32), device=DEV))
    with pytest.raises(ValueError, match='dsub'):
        engine.PqCodebook(torch.zeros((4, 16, 16), device=DEV))
    with pytest.raises(ValueError, match=r'codebooks must be \[M, ksub, dsub\]'):
        engine.PqCodebook(torch.zeros((16, 32), device=DEV))


# ----------------------------------------------------------------------------
# 8. quality
# ----------------------------------------------------------------------------
def test_planted_identities_keep_their_rank_1_on_the_device():
    """The case tests/test_pq_cpu.py decides with the numpy model, on exactly its inputs: all 60 queries."""
    from grl_amd import engine
    c = R.PLANTED
    qf, gf, q_pids, g_pids = R.planted_case()
    tq, tg = torch.from_numpy(qf).to(DEV), torch.from_numpy(gf).to(DEV)
    book = engine.pq_train(tg, c['M'], c['nbits'], 'cosine', c['max_iter'], c['train_seed'])
    index = engine.pq_index(tg, book)
    adc = engine.pq_search(tq, index, 1)[1][:, 0].cpu().numpy()
    exact = engine.search(tq, tg, 1)[1][:, 0].cpu().numpy()
    assert np.array_equal(g_pids[exact], q_pids)
    assert np.array_equal(g_pids[adc], g_pids[exact])
    assert engine.topk_recall(engine.pq_search(tq, index, 30)[1], engine.search(tq, tg, 30)[1], (30,))[0] > 0.9
    assert index.nbytes < 4 * gf.size // 8


# ----------------------------------------------------------------------------
# 9. repeatability
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('metric', METRICS)
def test_two_streams_give_identical_bits(metric):
    from grl_amd import engine
    index, qf, D, order, ids = search_case(metric)
    big, qbig = _scan_case(13, 256, 1000, 33, metric)
    runs = []
    for _ in range(2):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            runs.append((engine.pq_dist(qbig, big), engine.pq_dist(qf, index, block_cols=64),
                         engine.pq_search(qf, index, 10), engine.pq_search(qf, index, 1024, exclude=ids)))
        s.synchronize()
    a, b = runs
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    assert np.array_equal(bits(a[1]), bits(D))
    for u, v in ((a[2], b[2]), (a[3], b[3])):
        assert np.array_equal(bits(u[0]), bits(v[0])) and torch.equal(u[1], v[1])


# ----------------------------------------------------------------------------
# 10. ATTEvaluator.evaluate with GRL_EVAL_PQ
# ----------------------------------------------------------------------------
KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_CLUSTER', 'GRL_EVAL_CLUSTER_JACCARD', 'GRL_EVAL_KMEANS', 'GRL_EVAL_HDBSCAN', 'GRL_EVAL_TSNE',
         'GRL_EVAL_SILHOUETTE', 'GRL_EVAL_PCA', 'GRL_EVAL_DIFFUSION', 'GRL_EVAL_SET', 'GRL_EVAL_PQ')


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
    out_file = os.path.join(str(tmp_path), 'pq.json')

    def run(rerank=0):
        if os.path.exists(out_file):
            os.remove(out_file)
        with contextlib.redirect_stdout(io.StringIO()) as o:
            r = ev.evaluate(None, None, q_loader, g_loader, path, 0, rerank)
        return r, o.getvalue().splitlines(), open(out_file).read() if os.path.exists(out_file) else None

    def refuse(c):
        raise ValueError('not strict JSON: %s' % c)

    book = engine.pq_train(gf, 8, 4, 'cosine', 25, 0)
    index = engine.pq_index(gf, book)
    cmc, mAP = engine.pq_metrics_streaming(qf, index, *ids)
    cmc_x, mAP_x = engine.rank_metrics_streaming(qf, gf, *ids)
    recall = engine.topk_recall(engine.pq_search(qf, index, 100, exclude=ids)[1],
                                engine.search(qf, gf, 100, exclude=ids)[1], (1, 10, 100))
    for route in ('dense', 'stream'):
        if route == 'stream':
            monkeypatch.setenv('GRL_EVAL_STREAM', '1')
        r_off, text_off, file_off = run()
        assert file_off is None and not any('ADC' in l or l.startswith('PQ') for l in text_off), route
        monkeypatch.setenv('GRL_EVAL_PQ', '8,4')
        r_on, text_on, raw = run()
        monkeypatch.delenv('GRL_EVAL_PQ')
        assert r_on == r_off, route
        extra = len(text_on) - len(text_off)
        assert extra == 8 and text_on[:len(text_off) - 1] == text_off[:-1] and text_on[-1] == text_off[-1], route
        new = text_on[len(text_off) - 1:-1]
        assert new[0] == 'PQ: M = 8, nbits = 4 (8 bytes per row of {}), {} rows'.format(4 * d, n)
        assert new[1] == 'ADC Mean AP: {:4.1%} (exact {:4.1%})'.format(mAP, mAP_x)
        assert new[2] == 'ADC Rank-{:<3}: {:.1%} (exact {:.1%})'.format(1, cmc[0], cmc_x[0])
        assert new[6] == 'ADC recall@1: {:.2%}  @10: {:.2%}  @100: {:.2%}'.format(*recall)
        assert new[7].startswith('Index: {} bytes against {} bytes of features'.format(index.nbytes, 4 * n * d))
        js = json.loads(raw, parse_constant=refuse)
        assert js['adc'] == {'mAP': float(mAP), 'cmc': [float(v) for v in cmc]}, route
        assert js['exact'] == {'mAP': float(mAP_x), 'cmc': [float(v) for v in cmc_x]}, route
        assert js['recall'] == {'1': recall[0], '10': recall[1], '100': recall[2]}, route
        assert (js['index_bytes'], js['code_bytes'], js['feature_bytes']) == (index.nbytes, 8 * n, 4 * n * d), route
        assert (js['M'], js['nbits'], js['ksub'], js['dsub'], js['n'], js['n_queries']) == (8, 4, 16, d // 8, n, int(qf.size(0)))
    monkeypatch.delenv('GRL_EVAL_STREAM')
    monkeypatch.setenv('GRL_EVAL_PQ', '8,4')
    with pytest.raises(ValueError, match='GRL_EVAL_PQ=8,4 cannot re-rank'):
        run(rerank=1)
    for name, value in (('GRL_EVAL_METRIC', 'verify'), ('GRL_EVAL_SET', 'chamfer'), ('GRL_EVAL_DIFFUSION', '5')):
        monkeypatch.setenv(name, value)
        with pytest.raises(ValueError, match='GRL_EVAL_PQ=8,4 cannot be combined with %s' % name):
            run()
        with pytest.raises(ValueError, match='GRL_EVAL_PQ=8,4 cannot be combined with %s' % name):
            ATTEvaluator(cnn, siam, only_eval=True).evaluate(None, None, q_loader, g_loader, path, 0, 0)
        monkeypatch.delenv(name)
    monkeypatch.setenv('GRL_EVAL_PQ', '7')                         # M does not divide the feature size
    with pytest.raises(ValueError, match='M must divide'):
        run()
