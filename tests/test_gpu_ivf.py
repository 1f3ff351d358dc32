"""IVF-PQ index on the device (engine.IvfPqCodebook / ivf_train / ivf_index / IvfPqIndex / ivf_dist / ivf_search /
ivf_probe_stats, ivf.hip, GRL_EVAL_IVF) against the numpy model of tests/ivf_ref.py.  The model is fed with
the DOWNLOADED device G0, tables, xn, rn, ids and list_ptr, so only the scan is under test and every comparison of
distances is exact (bit patterns)."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import ivf_ref as V
import pq_ref as R
import search_filter_ref as FR

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
METRICS = ('cosine', 'euclidean')
IVF_MC = 16                                # the subspaces ivf.hip stages at once: M = 20 walks two chunks at ksub = 256
# empty lists first, in the middle and last; a virtual row crosses a 2048-column slab inside a list (2049, 2500)
LENS = (0, 1, 7, 2049, 300, 0, 2500, 0)
NLIST, N = len(LENS), sum(LENS)


def bits(a):
    if torch.is_tensor(a):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rows(n, d, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    x = g.standard_normal((n, d)).astype(np.float32)
    return torch.from_numpy(x / np.linalg.norm(x, axis=1, keepdims=True)).to(DEV)


def _book(M, ksub, metric, nlist=NLIST, seed=0, zero=False, dsub=32):
    from grl_amd import engine
    g = np.random.Generator(np.random.PCG64(1000 + seed + M))
    pq = engine.PqCodebook(torch.from_numpy(g.standard_normal((M, ksub, dsub)).astype(np.float32) * 0.2).to(DEV), 'cosine')
    # rows of unequal norm (2 .. 0.5): -q . c and |q - c| then order the lists differently, so the probe metric shows
    coarse = _rows(nlist, M * dsub, 500 + seed + M) * torch.linspace(2.0, 0.5, nlist, device=DEV).view(-1, 1)
    return engine.IvfPqCodebook(torch.zeros_like(coarse) if zero else coarse, pq, metric)


def _labels(seed=0, lens=LENS):
    g = np.random.Generator(np.random.PCG64(3000 + seed))
    lab = np.repeat(np.arange(len(lens)), lens)
    g.shuffle(lab)
    return torch.from_numpy(lab.astype(np.int64)).to(DEV)


def _codes(n, M, ksub, seed=0):
    """random codes; about half of the rows repeat an earlier row (ties between gallery entries, whatever their lists)"""
    g = np.random.Generator(np.random.PCG64(2000 + seed + M))
    c = g.integers(0, ksub, (n, M)).astype(np.uint8)
    src = g.integers(0, n, n)
    take = g.random(n) < 0.5
    c[take] = c[np.minimum(src, np.arange(n))[take]]
    return torch.from_numpy(c).to(DEV)


_indexes = {}


def _index(M, ksub, metric, seed=0):
    """the index of the LENS lists over random duplicated codes; built once per key, never modified"""
    from grl_amd import engine
    key = (M, ksub, metric, seed)
    if key not in _indexes:
        _indexes[key] = engine.IvfPqIndex(_book(M, ksub, metric, seed=seed), _labels(seed), _codes(N, M, ksub, seed))
    return _indexes[key]


def _model(qf, qs, index, nprobe):
    """(D [nq, n], cand [nq, n]) of the numpy model on downloaded device data: G0 = cosin_dist(qf, coarse), the metric's
    distances to the centroids, the tables, xn, rn, ids and list_ptr.  The probes are the MODEL's (ivf_ref.probes on the
    downloaded distances); the engine's probes and g0 are checked against them, not taken over."""
    from grl_amd import engine
    book, n = index.book, index.n
    G0 = engine.cosin_dist(qf, book.coarse).cpu().numpy()
    Dc = G0 if book.metric == 'cosine' else engine.pairwise_distance_tensor(qf, book.coarse).cpu().numpy()
    probe = V.probes(Dc, nprobe)
    assert np.array_equal(qs.probe.cpu().numpy(), probe) and qs.probe.dtype == torch.int32
    assert np.array_equal(engine.search(qf, book.coarse, nprobe, book.metric)[1].cpu().numpy(), probe)
    assert np.array_equal(bits(qs.g0), bits(np.take_along_axis(G0, probe, 1)))
    ids, ptr_ = index.ids.cpu().numpy(), index.list_ptr.cpu().numpy()
    lab = np.empty(n, np.int64)
    for l in range(book.nlist):
        lab[ids[ptr_[l]:ptr_[l + 1]]] = l
    xn = rn = None
    if book.metric == 'euclidean':
        xn = np.empty(n, np.float32)
        xn[ids] = index.xn.cpu().numpy()
        rn = qs.rn.cpu().numpy()
    D = V.dist(qs.lut.cpu().numpy(), index.codes.cpu().numpy(), lab, G0, book.metric, xn, rn)
    return D, V.candidates(lab, probe)


def _scatter(qs, index, d, cidx):
    """a chunk (dist, cidx) as (D [nq, n], cand [nq, n]) in gallery order; every gallery index at most once per row"""
    d, cidx = d.cpu().numpy(), cidx.cpu().numpy()
    D = np.zeros((qs.nq, index.n), np.float32)
    cand = np.zeros((qs.nq, index.n), bool)
    for q in range(qs.nq):
        live = cidx[q] >= 0
        assert np.unique(cidx[q][live]).size == live.sum()
        assert not live[int(live.sum()):].any() and np.isposinf(d[q][~live]).all()      # the padding is the row's tail
        D[q, cidx[q][live]] = d[q][live]
        cand[q, cidx[q][live]] = True
    return D, cand


def _same(D, cand, Dm, candm):
    assert np.array_equal(cand, candm)
    assert np.array_equal(bits(np.where(cand, D, 0)), bits(np.where(cand, Dm, 0)))


# ----------------------------------------------------------------------------
# 1. the scan against the model
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('M', [1, 3, 4, 5, 8, 13, IVF_MC + 4])
def test_scan_equals_the_model_on_the_downloaded_device_data(M, metric):
    from grl_amd import engine
    for i, nq in enumerate((1, 3, 33)):
        ksub = 256 if M > IVF_MC else (16, 256)[(i + M) % 2]
        index = _index(M, ksub, metric)
        assert np.diff(index.list_ptr.cpu().numpy()).tolist() == list(LENS)
        qf = _rows(nq, 32 * M, 40 + nq + M)
        for nprobe in (1, 2, NLIST):
            qs = engine._IvfQueries(qf, index, nprobe)
            Dm, candm = _model(qf, qs, index, nprobe)
            D, cand = engine.ivf_dist(qf, index, nprobe)
            _same(D.cpu().numpy(), cand.cpu().numpy(), Dm, candm)
            stats = engine.ivf_probe_stats(qf, index, nprobe)
            assert stats.dtype == torch.int64 and np.array_equal(stats.cpu().numpy(), candm.sum(1))
        assert candm.all() and nprobe == NLIST
    # the fixture can tell the probe metrics apart: cosine and Euclidean order the lists differently
    G0 = engine.cosin_dist(qf, index.book.coarse).cpu().numpy()
    E = engine.pairwise_distance_tensor(qf, index.book.coarse).cpu().numpy()
    assert not np.array_equal(V.probes(G0, 2), V.probes(E, 2))


@pytest.mark.parametrize('metric', METRICS)
def test_scan_follows_ieee_on_nan_and_infinite_table_entries_and_a_nan_query(metric):
    from grl_amd import engine
    M, ksub, nq = 7, 16, 6
    index = _index(M, ksub, metric)
    qf = _rows(nq, 32 * M, 9).clone()
    qf[5] = float('nan')
    qs = engine._IvfQueries(qf, index, NLIST)
    assert qs.probe[5].tolist() == list(range(NLIST))             # every distance of the NaN row ties: ascending lists
    clean = _scatter(qs, index, *qs.chunk(0, NLIST, N))[0]
    lut = qs.lut
    lut[0, 2, 3] = float('nan')
    lut[1, 0, 5], lut[1, 4, 5] = float('inf'), float('inf')            # same partial: +inf
    lut[3, 3, 1] = float('-inf')
    D, cand = _scatter(qs, index, *qs.chunk(0, NLIST, N))
    Dm, candm = _model(qf, qs, index, NLIST)
    _same(D, cand, Dm, candm)
    codes = index.codes.cpu().numpy()
    hit = codes[:, 2] == 3
    assert hit.any() and (~hit).any() and cand.all()
    floor = np.sqrt(np.float32(1e-12))
    if metric == 'cosine':
        assert np.isnan(D[0][hit]).all() and np.isnan(D[5]).all()
        assert np.isposinf(D[1][(codes[:, 0] == 5) | (codes[:, 4] == 5)]).all() and np.isneginf(D[3][codes[:, 3] == 1]).all()
    else:
        assert (D[0][hit] == floor).all() and (D[5] == floor).all()     # the clamp's rule for a NaN
        assert np.isposinf(D[1][(codes[:, 0] == 5) | (codes[:, 4] == 5)]).all() and (D[3][codes[:, 3] == 1] == floor).all()
    assert np.array_equal(bits(D[0][~hit]), bits(clean[0][~hit]))
    assert np.array_equal(bits(D[4]), bits(clean[4]))                  # the untouched query


# ----------------------------------------------------------------------------
# 2. search: order, ties, padding, the junk rule, every chunking
# ----------------------------------------------------------------------------
_cache = {}


def search_case(metric):
    """33 queries, M = 5, ksub = 16 on the LENS lists; the materialised distances per nprobe and the ids of the junk rule.
    Built once per metric, never modified."""
    from grl_amd import engine
    if metric not in _cache:
        index = _index(5, 16, metric, seed=3)
        qf = _rows(33, 160, 77)
        g = np.random.Generator(np.random.PCG64(77))
        ids = (g.integers(0, 12, 33), g.integers(0, 12, N), g.integers(0, 3, 33), g.integers(0, 3, N))
        mats = {p: tuple(t.cpu().numpy() for t in engine.ivf_dist(qf, index, p)) for p in (1, 2, NLIST)}
        _cache[metric] = (index, qf, mats, ids)
    return _cache[metric]


@pytest.mark.parametrize('metric', METRICS)
def test_search_is_the_head_of_the_ranked_candidates_with_ties_to_the_smaller_gallery_index(metric):
    from grl_amd import engine
    index, qf, mats, ids = search_case(metric)
    codes, lab = index.codes.cpu().numpy(), index.labels().cpu().numpy()
    assert lab.dtype == np.int64 and np.array_equal(lab, _labels(3).cpu().numpy())
    # duplicate code rows in different lists: equal distances under an equal coarse term only, so look at the result
    _, first = np.unique(codes, axis=0, return_index=True)
    assert first.size < N
    junk = FR.junk_mask(*ids)
    tied = 0
    for nprobe in (1, 2, NLIST):
        D, cand = mats[nprobe]
        for k in (1, 10, 1024):
            dv, di = engine.ivf_search(qf, index, k, nprobe)
            assert tuple(dv.shape) == (33, k) and di.dtype == torch.int64 and dv.dtype == torch.float32
            mv, mi = V.search(D, cand, k)
            assert np.array_equal(di.cpu().numpy(), mi) and np.array_equal(bits(dv), bits(mv)), (nprobe, k)
            dv, di = engine.ivf_search(qf, index, k, nprobe, exclude=ids)
            mv, mi = V.search(D, cand, k, junk)
            assert np.array_equal(di.cpu().numpy(), mi) and np.array_equal(bits(dv), bits(mv)), (nprobe, k)
        with np.errstate(invalid='ignore'):                        # (inf - inf in the padding)
            tied += int((np.diff(mv, axis=1) == 0).sum())
        # k = 1024 above the candidate count of a query that probes short lists: padding
        short = cand.sum(1) < 1024
        if nprobe == 1:
            assert short.any()
        assert (mi[short, -1] == -1).all() and np.isposinf(dv.cpu().numpy()[short, -1]).all()
    assert tied > 0


@pytest.mark.parametrize('metric', METRICS)
def test_every_chunking_gives_the_same_bits(metric, monkeypatch):
    from grl_amd import engine
    index, qf, mats, ids = search_case(metric)
    nprobe = NLIST
    d0, i0 = engine.ivf_search(qf, index, 50, nprobe)
    e0, j0 = engine.ivf_search(qf, index, 50, nprobe, exclude=ids)
    assert engine._ivf_plan(index, 33, nprobe, None) == (33, nprobe)
    one_probe = 8 * 33 * 2500                                      # the longest list, all queries: one probe per chunk
    assert engine._ivf_plan(index, 33, nprobe, one_probe) == (33, 1)
    assert engine._ivf_plan(index, 33, nprobe, 8 * 33 * 4549) == (33, 2)
    assert engine._ivf_plan(index, 33, nprobe, 8 * 5 * 2500 + 9) == (5, 1)      # one probe exceeds it: query row blocks
    assert engine._ivf_plan(index, 33, nprobe, 1) == (1, 1)
    for bb in (one_probe, 8 * 33 * 4549, 8 * 5 * 2500 + 9, 1):
        dv, di = engine.ivf_search(qf, index, 50, nprobe, block_bytes=bb)
        assert np.array_equal(bits(dv), bits(d0)) and torch.equal(di, i0), bb
        dv, di = engine.ivf_search(qf, index, 50, nprobe, exclude=ids, block_bytes=bb)
        assert np.array_equal(bits(dv), bits(e0)) and torch.equal(di, j0), bb
    # tables of 5 * 16 * 4 = 320 bytes per query: 33 queries in row blocks of 4
    monkeypatch.setattr(engine, 'PQ_LUT_BYTES', 4 * 320 + 17)
    assert engine._ivf_plan(index, 33, nprobe, None) == (4, nprobe)
    dv, di = engine.ivf_search(qf, index, 50, nprobe, exclude=ids)
    assert np.array_equal(bits(dv), bits(e0)) and torch.equal(di, j0)


@pytest.mark.parametrize('metric', METRICS)
def test_a_second_stream_and_a_repeated_run_give_identical_bits(metric):
    from grl_amd import engine
    index, qf, mats, ids = search_case(metric)
    big, qbig = _index(IVF_MC + 4, 256, metric), _rows(33, 32 * (IVF_MC + 4), 5)
    runs = []
    for _ in range(2):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            runs.append((engine.ivf_dist(qbig, big, NLIST)[0], engine.ivf_dist(qf, index, 2)[0],
                         engine.ivf_search(qf, index, 10, 2), engine.ivf_search(qf, index, 1024, NLIST, exclude=ids)))
        s.synchronize()
    a, b = runs
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    assert np.array_equal(bits(a[1]), bits(mats[2][0]))
    for u, v in ((a[2], b[2]), (a[3], b[3])):
        assert np.array_equal(bits(u[0]), bits(v[0])) and torch.equal(u[1], v[1])


@pytest.mark.parametrize('M,ksub', [(5, 16), (IVF_MC + 4, 256)])
def test_a_zero_coarse_quantiser_reduces_the_search_to_pq_search(M, ksub):
    """nprobe = nlist, 'cosine', coarse = 0: g0 = -q . 0 is a zero of either sign and t = g0 + S has S's bits (S is never
    -0: its partials start from +0), so the new scan must give the old scan's bits on the same codes."""
    from grl_amd import engine
    book = _book(M, ksub, 'cosine', zero=True)
    codes = _codes(N, M, ksub, 11)
    index = engine.IvfPqIndex(book, _labels(11), codes)
    flat = engine.PqIndex(book.pq, codes)
    # the cross-list tie order is under test only if equal code rows sit in different lists
    _, inv = np.unique(codes.cpu().numpy(), axis=0, return_inverse=True)
    labn, inv = index.labels().cpu().numpy(), np.asarray(inv).reshape(-1)
    lo, hi = np.full(inv.max() + 1, NLIST), np.full(inv.max() + 1, -1)
    np.minimum.at(lo, inv, labn)
    np.maximum.at(hi, inv, labn)
    assert (hi > lo).any()
    qf = _rows(33, 32 * M, 12)
    ids = search_case('cosine')[3]
    for kw in (dict(), dict(exclude=ids)):
        dv, di = engine.ivf_search(qf, index, 100, NLIST, **kw)
        pv, pi = engine.pq_search(qf, flat, 100, **kw)
        assert np.array_equal(bits(dv), bits(pv)) and torch.equal(di, pi), kw
    D, cand = engine.ivf_dist(qf, index, NLIST)
    assert cand.all() and np.array_equal(bits(D), bits(engine.pq_dist(qf, flat)))


# ----------------------------------------------------------------------------
# 3. building: labels, list order, residual, reconstruct, xn, the range checks, training
# ----------------------------------------------------------------------------
def _sqnorm(x):
    from grl_amd import engine
    from grl_amd._lib import ptr
    x = x.contiguous()
    out = torch.empty(x.shape[0], dtype=torch.float32, device=DEV)
    engine._call('grl_row_sqnorm', ptr(x), ptr(out), x.shape[0], x.shape[1], x.shape[1])
    return out


@pytest.mark.parametrize('metric', METRICS)
def test_index_is_kmeans_assign_ascending_lists_and_the_residual_codes(metric, monkeypatch):
    from grl_amd import engine
    M, ksub, nlist, n = 5, 16, 6, 777
    book = _book(M, ksub, metric, nlist=nlist, seed=2)
    xf = (book.coarse[torch.from_numpy(np.arange(n) % (nlist - 1)).to(DEV)] + 0.3 * _rows(n, 160, 21)).contiguous()
    xf[5] = float('nan')                                           # list 0, code 0 everywhere
    index = engine.ivf_index(xf, book)
    lab = engine.kmeans_assign(xf, book.coarse, 'euclidean')[0]
    assert torch.equal(index.labels(), lab) and int(lab[5]) == 0 and (index.codes[5] == 0).all()
    labn = lab.cpu().numpy()
    ptr_, ids = V.lists(labn, nlist)
    assert np.array_equal(index.list_ptr.cpu().numpy(), ptr_) and index.list_ptr.dtype == torch.int64
    assert np.array_equal(index.ids.cpu().numpy(), ids) and index.ids.dtype == torch.int32
    assert ptr_[-1] == n and ptr_[-2] == n                         # the last list is empty
    for l in range(nlist):
        assert (np.diff(ids[ptr_[l]:ptr_[l + 1]]) > 0).all()
    # the residual kernel, the codes and the reconstruction against the model, bit for bit
    res = engine._ivf_residual(xf, lab.to(torch.int32), book.coarse, torch.empty_like(xf))
    xn_, cn_ = xf.cpu().numpy(), book.coarse.cpu().numpy()
    want = V.residual(xn_, cn_, labn)
    keep = np.arange(n) != 5
    assert np.array_equal(bits(res)[keep], bits(want)[keep]) and np.isnan(res[5].cpu().numpy()).all()
    assert torch.equal(index.codes, book.pq.encode(res))
    rows = torch.from_numpy(np.array([0, 776, 5, 5, 100, 3], np.int64)).to(DEV)
    xh = index.reconstruct(rows)
    C = book.pq.codebooks.cpu().numpy()
    codes = index.codes.cpu().numpy()
    assert np.array_equal(bits(xh), bits(V.reconstruct(cn_, labn[rows.cpu().numpy()], codes[rows.cpu().numpy()], C)))
    full = index.reconstruct(torch.arange(n, device=DEV))
    assert np.array_equal(bits(full), bits(V.reconstruct(cn_, labn, codes, C)))
    if metric == 'euclidean':
        assert np.array_equal(bits(index.xn), bits(_sqnorm(full[index.ids.to(torch.int64)])))
    else:
        assert index.xn is None
    # the residuals are encoded in row blocks: a budget of 100 rows gives the same index
    monkeypatch.setattr(engine, 'SEARCH_BLOCK_BYTES', 100 * 4 * 160)
    again = engine.ivf_index(xf, book)
    assert torch.equal(again.codes, index.codes) and torch.equal(again._scan, index._scan) and torch.equal(again.ids, index.ids)
    if metric == 'euclidean':
        assert np.array_equal(bits(again.xn), bits(index.xn))
    assert index.nbytes == (8 * (nlist + 1) + 4 * n + n * M + 4 * 2 * n + 4 * n + (4 * n if metric == 'euclidean' else 0)
                            + 4 * nlist * 160 + 4 * M * ksub * 32)
    with pytest.raises(ValueError, match='rows must be in 0..n-1'):
        index.reconstruct(torch.tensor([n], device=DEV))


def test_constructors_check_their_arguments_on_the_device():
    from grl_amd import engine
    book = _book(5, 16, 'cosine')
    lab, codes = _labels(), _codes(N, 5, 16)
    for bad in (NLIST, -1, 2 ** 40):
        wrong = lab.clone()
        wrong[17] = bad
        with pytest.raises(ValueError, match=r'labels must be in 0\.\.nlist-1 = 0\.\.7'):
            engine.IvfPqIndex(book, wrong, codes)
    wrong = codes.clone()
    wrong[3, 4] = 16
    with pytest.raises(ValueError, match='codes must be in 0..ksub-1'):
        engine.IvfPqIndex(book, lab, wrong)
    with pytest.raises(ValueError, match='labels must be an integer device tensor'):
        engine.IvfPqIndex(book, lab[:-1], codes)
    with pytest.raises(ValueError, match='labels must be an integer device tensor'):
        engine.IvfPqIndex(book, lab.to(torch.float32), codes)
    with pytest.raises(ValueError, match='codes must be a uint8 device tensor'):
        engine.IvfPqIndex(book, lab, codes[:, :4])
    pq = book.pq
    with pytest.raises(ValueError, match='nlist in 1..65536'):
        engine.IvfPqCodebook(torch.zeros((0, 160), device=DEV), pq)
    with pytest.raises(ValueError, match=r'coarse must be \[nlist, d\]'):
        engine.IvfPqCodebook(torch.zeros(160, device=DEV), pq)
    with pytest.raises(ValueError, match='pq.d must equal'):
        engine.IvfPqCodebook(torch.zeros((4, 192), device=DEV), pq)
    with pytest.raises(ValueError, match='pq must be a PqCodebook'):
        engine.IvfPqCodebook(book.coarse, pq.codebooks)
    with pytest.raises(ValueError, match="whose metric is 'cosine'"):
        engine.IvfPqCodebook(book.coarse, engine.PqCodebook(pq.codebooks, 'euclidean'))
    with pytest.raises(ValueError, match='at least max'):
        engine.ivf_train(_rows(20, 160, 1), 30, 5, 4)
    with pytest.raises(ValueError, match='nlist must be an integer in 1..65536'):
        engine.ivf_train(_rows(20, 160, 1), 0, 5, 4)
    # an empty gallery and an index whose rows all sit in one list
    empty = engine.ivf_index(torch.zeros((0, 160), device=DEV), book)
    dv, di = engine.ivf_search(_rows(3, 160, 2), empty, 4, 2)
    assert (di == -1).all() and torch.isinf(dv).all() and empty.n == 0


def test_train_is_the_three_calls_it_is_defined_by():
    from grl_amd import engine
    xf = _rows(400, 128, 8)
    book = engine.ivf_train(xf, 5, 4, 4, 'euclidean', 6, 3)
    run = engine.kmeans(xf, 5, 'euclidean', 'random', 3, 6)
    assert np.array_equal(bits(book.coarse), bits(run.centroids))
    assert (book.coarse_n_iter, book.coarse_converged, book.coarse_inertia) == (run.n_iter, run.converged, run.inertia)
    lab = engine.kmeans_assign(xf, run.centroids, 'euclidean')[0]
    res = torch.from_numpy(V.residual(xf.cpu().numpy(), run.centroids.cpu().numpy(), lab.cpu().numpy())).to(DEV)
    pq = engine.pq_train(res, 4, 4, 'cosine', 6, 4)
    assert np.array_equal(bits(book.pq.codebooks), bits(pq.codebooks))
    assert book.pq.metric == 'cosine' and book.metric == 'euclidean' and book.pq.n_iter == pq.n_iter
    assert book.pq.inertia == pq.inertia and (book.nlist, book.d) == (5, 128)


# ----------------------------------------------------------------------------
# 4. the planted case of tests/test_ivf_cpu.py on the device
# ----------------------------------------------------------------------------
def test_planted_case_equals_the_model_at_every_nprobe():
    from grl_amd import engine
    c = R.PLANTED
    qf, gf, q_pids, g_pids = R.planted_case()
    tq, tg = torch.from_numpy(qf).to(DEV), torch.from_numpy(gf).to(DEV)
    book = engine.ivf_train(tg, 4, c['M'], c['nbits'], 'cosine', c['max_iter'], c['train_seed'])
    index = engine.ivf_index(tg, book)
    exact = engine.search(tq, tg, 10)[1].cpu().numpy()
    share = []
    for nprobe in (1, 2, 4):
        qs = engine._IvfQueries(tq, index, nprobe)
        Dm, candm = _model(tq, qs, index, nprobe)
        D, cand = engine.ivf_dist(tq, index, nprobe)
        _same(D.cpu().numpy(), cand.cpu().numpy(), Dm, candm)             # the device lists are the model's
        dv, di = engine.ivf_search(tq, index, 30, nprobe)
        mv, mi = V.search(Dm, candm, 30)
        assert np.array_equal(di.cpu().numpy(), mi) and np.array_equal(bits(dv), bits(mv)), nprobe
        share.append(float(np.mean([candm[i, exact[i]].mean() for i in range(len(qf))])))
    assert all(b >= a for a, b in zip(share, share[1:])) and share[-1] == 1.0 and candm.all()


# ----------------------------------------------------------------------------
# 5. ATTEvaluator.evaluate with GRL_EVAL_IVF
# ----------------------------------------------------------------------------
KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_CLUSTER', 'GRL_EVAL_CLUSTER_JACCARD', 'GRL_EVAL_KMEANS', 'GRL_EVAL_HDBSCAN', 'GRL_EVAL_TSNE',
         'GRL_EVAL_SILHOUETTE', 'GRL_EVAL_PCA', 'GRL_EVAL_DIFFUSION', 'GRL_EVAL_SET', 'GRL_EVAL_PQ', 'GRL_EVAL_IVF')


def test_attevaluator_reports_the_inverted_lists_after_the_pq_lines(synth_models, monkeypatch, tmp_path):
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
    files = [os.path.join(str(tmp_path), f) for f in ('pq.json', 'ivf.json')]

    def run():
        for f in files:
            if os.path.exists(f):
                os.remove(f)
        with contextlib.redirect_stdout(io.StringIO()) as o:
            r = ev.evaluate(None, None, q_loader, g_loader, path, 0, 0)
        return (r, o.getvalue().splitlines()) + tuple(open(f).read() if os.path.exists(f) else None for f in files)

    def refuse(c):
        raise ValueError('not strict JSON: %s' % c)

    book = engine.ivf_train(gf, 3, 8, 4, 'cosine', 25, 0)
    index = engine.ivf_index(gf, book)
    k = min(100, n)
    exact = engine.search(qf, gf, k, exclude=ids)[1]
    recall = engine.topk_recall(engine.ivf_search(qf, index, k, 2, exclude=ids)[1], exact, (1, 10, 100))
    flat = engine.pq_index(gf, engine.pq_train(gf, 8, 4, 'cosine', 25, 0))
    pq_recall = engine.topk_recall(engine.pq_search(qf, flat, k, exclude=ids)[1], exact, (1, 10, 100))
    scanned = float(engine.ivf_probe_stats(qf, index, 2).sum()) / (int(qf.size(0)) * n)
    lens = np.diff(index.list_ptr.cpu().numpy())
    for route in ('dense', 'stream'):
        if route == 'stream':
            monkeypatch.setenv('GRL_EVAL_STREAM', '1')
        monkeypatch.setenv('GRL_EVAL_PQ', '8,4')
        r_pq, text_pq, raw_pq, none = run()
        assert none is None and not any(l.startswith('IVF') for l in text_pq), route
        monkeypatch.setenv('GRL_EVAL_IVF', '3,2')
        r_on, text_on, raw_pq_on, raw = run()
        monkeypatch.delenv('GRL_EVAL_IVF')
        monkeypatch.delenv('GRL_EVAL_PQ')
        assert r_on == r_pq and raw_pq_on == raw_pq, route                  # pq.json byte for byte
        assert len(text_on) == len(text_pq) + 4 and text_on[:len(text_pq) - 1] == text_pq[:-1], route
        assert text_on[-1] == text_pq[-1], route
        new = text_on[len(text_pq) - 1:-1]
        assert new[0] == 'IVF: nlist = 3, nprobe = 2, list length min / mean / max = {} / {:.1f} / {}'.format(
            lens.min(), n / 3.0, lens.max())
        assert new[1] == 'IVF scanned fraction: {:.2%}'.format(scanned)
        assert new[2] == 'IVF recall@1: {:.2%}  @10: {:.2%}  @100: {:.2%}  (PQ {:.2%}  {:.2%}  {:.2%})'.format(
            *(tuple(recall) + tuple(pq_recall)))
        assert new[3].startswith('IVF index: {} bytes against {} bytes of features'.format(index.nbytes, 4 * n * d))
        js = json.loads(raw, parse_constant=refuse)
        assert (js['nlist'], js['nprobe'], js['M'], js['nbits'], js['n'], js['n_queries']) == (3, 2, 8, 4, n, int(qf.size(0)))
        assert js['recall'] == {'1': recall[0], '10': recall[1], '100': recall[2]}, route
        assert js['pq_recall'] == {'1': pq_recall[0], '10': pq_recall[1], '100': pq_recall[2]}, route
        assert js['scanned_fraction'] == scanned and js['index_bytes'] == index.nbytes
        assert js['list_len'] == {'min': int(lens.min()), 'mean': n / 3.0, 'max': int(lens.max())}
    monkeypatch.setenv('GRL_EVAL_IVF', '3,2')
    with pytest.raises(ValueError, match='GRL_EVAL_IVF=3,2 needs GRL_EVAL_PQ'):
        run()
