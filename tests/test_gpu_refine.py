"""Exact refinement of shortlists on the device (engine.RefineStore / refine_dist / refine_lists / refine_search,
refine.hip, GRL_EVAL_REFINE) against the numpy model of tests/refine_ref.py.  The model is fed with the
DOWNLOADED store values, queries and lists, and every comparison of distances is exact (bit patterns)."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import pq_ref as R
import refine_ref as F
import search_filter_ref as FR

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
METRICS = ('cosine', 'euclidean')
TYPES = ('f32', 'bf16')
DS = (4, 252, 256, 260, 1028)              # one lane group idle, exactly one chunk, a ragged second chunk, five chunks
LS = (1, 3, 4, 5, 33)                      # fewer candidates than waves .. one more than a slab of 32
N = 37
HAND = (0x3f800000, 0x3f808000, 0x3f818000, 0x3f808001, 0x3f807fff, 0x7f7fffff, 0xff7fffff, 0x7f7f7fff, 0x7f800000,
        0xff800000, 0x7f800001, 0xffc00000, 0x7fffffff, 0xff80ffff, 0x00000000, 0x80000000, 0x00008000, 0x00018000,
        0x80008001)


def bits(a):
    if torch.is_tensor(a):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rand(n, d, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(g.standard_normal((n, d)).astype(np.float32)).to(DEV)


def _values(store):
    """the downloaded VALUES of a store: its fp32 rows, or the widened bf16 bit patterns"""
    if store.dtype == 'f32':
        return store.data.cpu().numpy()
    return F.widen(store.data.view(torch.int16).cpu().numpy().view(np.uint16))


def _lists(nq, L, n, seed):
    """random lists with padding first, in the middle and last, an id == n, one far above, and a repeated id, wherever
    the shape has room for them (flattened positions, so that L = 1 gets them in different rows)"""
    g = np.random.Generator(np.random.PCG64(seed))
    c = g.integers(0, n, (nq, L)).astype(np.int64)
    flat = c.reshape(-1)
    t = flat.size
    flat[0] = -1
    if t > 1:
        flat[t - 1] = -1
    if t > 2:
        flat[t // 2] = -7
    if t > 3:
        flat[1] = n
    if t > 4:
        flat[3] = 2 ** 40
    if L > 5:
        c[:, 5] = c[:, 2]                                         # a repeated id in every row
        c[nq - 1, 4] = n - 1
    return c


_stores = {}


def _store(d, dtype):
    """N rows of d columns; built once per key, never modified"""
    from grl_amd import engine
    if (d, dtype) not in _stores:
        _stores[d, dtype] = engine.RefineStore(_rand(N, d, 100 + d), dtype)
    return _stores[d, dtype]


# ----------------------------------------------------------------------------
# 1. the scan against the model
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', TYPES)
@pytest.mark.parametrize('metric', METRICS)
def test_refine_dist_equals_the_model_on_the_downloaded_inputs(metric, dtype):
    from grl_amd import engine
    for d in DS:
        store = _store(d, dtype)
        assert (store.n, store.d, store.dtype, store.nbytes) == (N, d, dtype, N * d * (4 if dtype == 'f32' else 2))
        rows = _values(store)
        ids = torch.arange(N - 1, -1, -1, device=DEV)
        assert np.array_equal(bits(store.rows(ids)), bits(rows[::-1]))
        for nq in (1, 5):
            qf = _rand(nq, d, 7 * d + nq)
            for L in LS:
                cand = _lists(nq, L, N, d + L + nq)
                got = engine.refine_dist(qf, store, torch.from_numpy(cand).to(DEV), metric)
                want, cidx = F.dist(qf.cpu().numpy(), rows, cand, metric)
                assert got.dtype == torch.float32 and tuple(got.shape) == (nq, L)
                assert np.array_equal(bits(got), bits(want)), (d, nq, L)
                assert np.isposinf(got.cpu().numpy()[cidx < 0]).all() and (cidx < 0).any()


@pytest.mark.parametrize('dtype', TYPES)
def test_special_values_follow_ieee_and_every_nan_is_canonical(dtype):
    from grl_amd import engine
    d = 260
    x = _rand(6, d, 5).clone()
    x[0, 3], x[1, 7], x[2, 258], x[3, 0], x[3, 1] = float('nan'), float('inf'), float('-inf'), float('inf'), float('-inf')
    x[4] = 0.0
    x[4, 5] = -0.0
    store = engine.RefineStore(x, dtype)
    rows = _values(store)
    qf = _rand(3, d, 6).clone()
    qf[1] = 0.0                                                    # a query of zeros
    qf[2, 10] = float('nan')
    cand = torch.arange(6, device=DEV).view(1, 6).repeat(3, 1)
    floor = np.sqrt(np.float32(1e-12))
    for metric in METRICS:
        got = engine.refine_dist(qf, store, cand, metric)
        want = F.dist(qf.cpu().numpy(), rows, cand.cpu().numpy(), metric)[0]
        assert np.array_equal(bits(got), bits(want)), metric
        g = got.cpu().numpy()
        nan = np.isnan(g)
        assert (bits(g)[nan] == 0x7fc00000).all()
        if metric == 'cosine':
            assert nan[0, 0] and nan[2].all() and nan[1, :4].all()  # a NaN column, a NaN query, 0 * inf
            assert np.isinf(g[0, 1]) and np.isinf(g[0, 2])
            assert g[1, 4] == 0 and g[1, 5] == 0 and bits(g)[1, 5] == bits(want)[1, 5]      # -0 or +0 as the model has it
        else:
            assert g[0, 0] == floor and (g[2] == floor).all()     # a NaN argument of the clamp gives 1e-12
            assert np.isposinf(g[0, 1:4]).all() and np.isposinf(g[1, 1:4]).all()
            assert g[1, 4] == floor                                # |0 - 0|: the clamp


@pytest.mark.parametrize('d', (4, 1028))
def test_pack_bf16_equals_the_model(d):
    from grl_amd import engine
    from grl_amd._lib import ptr
    n = 9 if d == 4 else 3                                         # 36 / 3084 elements: a ragged end of 4 behind the groups of 8
    x = _rand(n, d, 40 + d).cpu().numpy() * np.float32(50)
    x.reshape(-1)[:len(HAND)] = np.array(HAND, np.uint32).view(np.float32)
    t = torch.from_numpy(x).to(DEV)
    store = engine.RefineStore(t, 'bf16')
    assert store.data.dtype == torch.bfloat16 and tuple(store.data.shape) == (n, d)
    got = store.data.view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, F.pack_bf16(x))
    assert got.reshape(-1)[:len(HAND)].tolist() == F.pack_bf16(np.array(HAND, np.uint32).view(np.float32)).tolist()
    assert np.array_equal(bits(store.rows(torch.arange(n, device=DEV))), bits(F.widen(got)))
    # pointers that are not 16-byte aligned: the element-by-element kernel
    flat = t.reshape(-1)
    out = torch.zeros(flat.numel(), dtype=torch.int16, device=DEV)
    engine._call('grl_refine_pack_bf16', ptr(flat[1:]), ptr(out[1:]), flat.numel() - 1)
    assert np.array_equal(out.cpu().numpy().view(np.uint16)[1:], F.pack_bf16(x).reshape(-1)[1:]) and int(out[0]) == 0
    # an fp32 store is the caller's tensor, not a copy
    assert engine.RefineStore(t, 'f32').data.data_ptr() == t.data_ptr()


# ----------------------------------------------------------------------------
# 2. refine_lists: order, ties, padding, duplicates, every blocking
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', TYPES)
@pytest.mark.parametrize('metric', METRICS)
def test_refine_lists_is_the_models_ranking_for_every_blocking(metric, dtype):
    from grl_amd import engine
    d, nq, L = 260, 5, 33
    store = _store(d, dtype)
    rows = _values(store)
    qf = _rand(nq, d, 11)
    cand = _lists(nq, L, N, 12)
    cand[1, :8] = cand[1, 8]                                       # one id eight times
    tc = torch.from_numpy(cand).to(DEV)
    for k in (1, L, L + 3):
        dv, di = engine.refine_lists(qf, store, tc, k, metric)
        mv, mi = F.refine_lists(qf.cpu().numpy(), rows, cand, k, metric)
        assert tuple(dv.shape) == (nq, k) and di.dtype == torch.int64 and dv.dtype == torch.float32
        assert np.array_equal(di.cpu().numpy(), mi) and np.array_equal(bits(dv), bits(mv)), k
        for bb in (8 * L, 8 * L * 2 + 1, 1):                       # one query row per block, two, and a budget below one row
            bv, bi = engine.refine_lists(qf, store, tc, k, metric, block_bytes=bb)
            assert np.array_equal(bits(bv), bits(dv)) and torch.equal(bi, di), (k, bb)
        av, ai = engine.refine_lists(qf, store, tc, k, metric)
        assert np.array_equal(bits(av), bits(dv)) and torch.equal(ai, di)
    assert (mi[:, -3:] == -1).all() and np.isposinf(mv[:, -3:]).all()          # k = L + 3: padding
    assert (mi[1] == cand[1, 8]).sum() >= 9                        # the duplicates all appear
    # no candidates at all, and an empty store
    ev, ei = engine.refine_lists(qf, store, tc[:, :0], 4, metric)
    assert (ei == -1).all() and torch.isinf(ev).all()
    empty = engine.RefineStore(torch.zeros((0, d), device=DEV), dtype)
    ev, ei = engine.refine_lists(qf, empty, tc, 4, metric)
    assert (ei == -1).all() and torch.isinf(ev).all() and empty.nbytes == 0
    assert torch.isinf(engine.refine_dist(qf, empty, tc, metric)).all()


# ----------------------------------------------------------------------------
# 3. refine_search over a flat index: the planted case of tests/test_refine_cpu.py on the device
# ----------------------------------------------------------------------------
def _junk_ids(nq, n, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    return (g.integers(0, 12, nq), g.integers(0, 12, n), g.integers(0, 3, nq), g.integers(0, 3, n))


def _check_two_stage(qf, index, store, first, k, R_, ids, **kw):
    """refine_search == refine_lists over the first stage's own lists == the model on them; no junk entry with exclude"""
    from grl_amd import engine
    metric = index.codebook.metric if isinstance(index, engine.PqIndex) else index.book.metric
    rows = _values(store)
    junk = FR.junk_mask(*ids)
    plain = None
    for ex in (None, ids):
        cand = first(qf, index, R_, exclude=ex, **kw)[1]
        if ex is None:                                            # does the unfiltered shortlist hold junk at all?
            c = cand.cpu().numpy()
            saw_junk = any(junk[q, c[q][c[q] >= 0]].any() for q in range(c.shape[0]))
            plain = cand
        else:
            assert torch.equal(cand, plain) != saw_junk           # then the junk rule changes the shortlists
        dv, di = engine.refine_search(qf, index, store, k, R_, exclude=ex, **kw)
        lv, li = engine.refine_lists(qf, store, cand, k, metric)
        assert np.array_equal(bits(dv), bits(lv)) and torch.equal(di, li)
        mv, mi = F.refine_lists(qf.cpu().numpy(), rows, cand.cpu().numpy(), k, metric)
        assert np.array_equal(di.cpu().numpy(), mi) and np.array_equal(bits(dv), bits(mv))
        got = di.cpu().numpy()
        hit = np.array([junk[q, got[q][got[q] >= 0]].any() for q in range(got.shape[0])])
        assert ex is None or not hit.any()                        # the junk rule of the first stage is all it takes
    return got, saw_junk


def test_refine_search_over_a_flat_index_and_the_planted_recall():
    from grl_amd import engine
    c = R.PLANTED
    qf, gf, q_pids, g_pids = R.planted_case()
    tq, tg = torch.from_numpy(qf).to(DEV), torch.from_numpy(gf).to(DEV)
    index = engine.pq_index(tg, engine.pq_train(tg, c['M'], c['nbits'], 'cosine', c['max_iter'], c['train_seed']))
    exact = np.argsort(-(qf.astype(np.float64) @ gf.astype(np.float64).T), axis=1, kind='stable')[:, :10]
    for dtype in TYPES:
        store = engine.RefineStore(tg, dtype)
        assert _check_two_stage(tq, index, store, engine.pq_search, 10, 40, _junk_ids(len(qf), len(gf), 3))[1]
        idx = engine.refine_search(tq, index, store, 10, 40)[1].cpu().numpy()
        if dtype == 'bf16':                                        # ranked is what the store holds: the widened rows
            w = _values(store).astype(np.float64)
            exact = np.argsort(-(qf.astype(np.float64) @ w.T), axis=1, kind='stable')[:, :10]
        adc = R.recall(engine.pq_search(tq, index, 10)[1].cpu().numpy(), exact, (1, 10))
        got = R.recall(idx, exact, (1, 10))
        print('\n[planted refine case, %s store, on the device] ADC recall@1 / @10 %.3f / %.3f, refined at R = 40 %.3f / %.3f'
              % (dtype, adc[0], adc[1], got[0], got[1]))
        assert got == [1.0, 1.0] and adc[1] < 0.5


# ----------------------------------------------------------------------------
# 4. refine_search over an IVF-PQ index built from supplied labels and codes
# ----------------------------------------------------------------------------
LENS = (0, 1, 7, 2049, 300, 0, 2500, 0)
NLIST, NIVF = len(LENS), sum(LENS)


def _unit(n, d, seed):
    x = _rand(n, d, seed)
    return x / x.norm(dim=1, keepdim=True)


def _ivf_index(metric, M=5, ksub=16, dsub=32):
    from grl_amd import engine
    g = np.random.Generator(np.random.PCG64(1000 + M))
    pq = engine.PqCodebook(torch.from_numpy(g.standard_normal((M, ksub, dsub)).astype(np.float32) * 0.2).to(DEV), 'cosine')
    coarse = _unit(NLIST, M * dsub, 500 + M) * torch.linspace(2.0, 0.5, NLIST, device=DEV).view(-1, 1)
    lab = np.repeat(np.arange(NLIST), LENS)
    g.shuffle(lab)
    codes = torch.from_numpy(g.integers(0, ksub, (NIVF, M)).astype(np.uint8)).to(DEV)
    return engine.IvfPqIndex(engine.IvfPqCodebook(coarse, pq, metric), torch.from_numpy(lab.astype(np.int64)).to(DEV), codes)


@pytest.mark.parametrize('metric', METRICS)
def test_refine_search_over_an_ivf_index(metric):
    from grl_amd import engine
    index = _ivf_index(metric)
    qf = _unit(9, 160, 77)
    ids = _junk_ids(9, NIVF, 5)
    for dtype in TYPES:
        store = engine.RefineStore(_unit(NIVF, 160, 78), dtype)
        for nprobe, R_ in ((1, 50), (NLIST, 200)):
            got, saw_junk = _check_two_stage(qf, index, store, engine.ivf_search, 20, R_, ids, nprobe=nprobe)
        assert (got >= 0).all() and saw_junk                      # (all lists probed: 1800 candidates, the ids can tell)
    # a query that probes the one-row list alone: R candidates are not there, the tail is padding
    short = engine.ivf_search(qf, index, 50, 1)[1]
    dv, di = engine.refine_search(qf, index, store, 20, 50, nprobe=1)
    few = (short >= 0).sum(1) < 20
    assert ((di[few] >= 0).sum(1) == (short[few] >= 0).sum(1)).all()


# ----------------------------------------------------------------------------
# 5. refusals
# ----------------------------------------------------------------------------
def test_refusals_name_the_argument():
    from grl_amd import engine
    index = _ivf_index('cosine')
    flat = engine.PqIndex(index.book.pq, index.codes)
    store = engine.RefineStore(_unit(NIVF, 160, 78))
    qf = _unit(3, 160, 1)
    with pytest.raises(ValueError, match='xf must have d columns with d a multiple of 4'):
        engine.RefineStore(torch.zeros((3, 6), device=DEV))
    with pytest.raises(ValueError, match='xf must have d columns with d a multiple of 4 in 1..16384'):
        engine.RefineStore(torch.zeros((2, 16388), device=DEV))
    with pytest.raises(ValueError, match='xf must be contiguous'):
        engine.RefineStore(torch.zeros((8, 8), device=DEV).t())
    with pytest.raises(ValueError, match='ids must be in 0..n-1'):
        store.rows(torch.tensor([NIVF], device=DEV))
    for bad in (engine.RefineStore(_unit(NIVF - 1, 160, 2)), engine.RefineStore(_unit(NIVF, 128, 2))):
        for ix, kw in ((flat, {}), (index, dict(nprobe=2))):
            with pytest.raises(ValueError, match='store must hold the rows of the index'):
                engine.refine_search(qf, ix, bad, 5, 10, **kw)
    with pytest.raises(ValueError, match=r'R \(k <= R <= 1024\) must be an integer in 5\.\.1024'):
        engine.refine_search(qf, flat, store, 5, 4)
    with pytest.raises(ValueError, match=r'R \(k <= R <= 1024\) must be an integer in 5\.\.1024'):
        engine.refine_search(qf, index, store, 5, 1025, nprobe=2)
    with pytest.raises(ValueError, match='nprobe is for an IvfPqIndex'):
        engine.refine_search(qf, flat, store, 5, 10, nprobe=2)
    with pytest.raises(ValueError, match='nprobe is required'):
        engine.refine_search(qf, index, store, 5, 10)
    with pytest.raises(ValueError, match=r'nprobe must be an integer in 1\.\.8'):
        engine.refine_search(qf, index, store, 5, 10, nprobe=9)
    cand = torch.zeros((3, 4), dtype=torch.int64, device=DEV)
    vm = engine.VerifyMetric.__new__(engine.VerifyMetric)
    for fn, args in ((engine.refine_dist, ()), (engine.refine_lists, (2,))):
        with pytest.raises(ValueError, match='verify_metric'):
            fn(qf, store, cand, *args, metric=vm)
        with pytest.raises(ValueError, match='cand must be an int64 device tensor'):
            fn(qf, store, cand.cpu(), *args)
    with pytest.raises(ValueError, match=r'k must be an integer in 1\.\.1024'):
        engine.refine_lists(qf, store, cand, 1025)
    dv, di = engine.refine_lists(qf, store, cand, 1024)            # k far above L: padding
    assert (di[:, 4:] == -1).all() and (di[:, :4] == 0).all()


# ----------------------------------------------------------------------------
# 6. ATTEvaluator.evaluate with GRL_EVAL_REFINE
# ----------------------------------------------------------------------------
KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_CLUSTER', 'GRL_EVAL_CLUSTER_JACCARD', 'GRL_EVAL_KMEANS', 'GRL_EVAL_HDBSCAN', 'GRL_EVAL_TSNE',
         'GRL_EVAL_SILHOUETTE', 'GRL_EVAL_PCA', 'GRL_EVAL_DIFFUSION', 'GRL_EVAL_SET', 'GRL_EVAL_PQ', 'GRL_EVAL_IVF',
         'GRL_EVAL_REFINE')


def test_attevaluator_reports_the_refined_recall_after_the_index_lines(synth_models, monkeypatch, tmp_path):
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
    n, d, nq = int(gf.size(0)), int(gf.size(1)), int(qf.size(0))
    path = str(tmp_path) + os.sep
    files = [os.path.join(str(tmp_path), f) for f in ('pq.json', 'ivf.json', 'refine.json')]

    def run():
        for f in files:
            if os.path.exists(f):
                os.remove(f)
        with contextlib.redirect_stdout(io.StringIO()) as o:
            r = ev.evaluate(None, None, q_loader, g_loader, path, 0, 0)
        return (r, o.getvalue().splitlines()) + tuple(open(f).read() if os.path.exists(f) else None for f in files)

    def refuse(c):
        raise ValueError('not strict JSON: %s' % c)

    R_ = 16
    k = min(100, n, R_)
    exact = engine.search(qf, gf, min(100, n), exclude=ids)[1]
    flat = engine.pq_index(gf, engine.pq_train(gf, 8, 4, 'cosine', 25, 0))
    ivf = engine.ivf_index(gf, engine.ivf_train(gf, 3, 8, 4, 'cosine', 25, 0))
    ks = (1, 10, 100)
    adc = engine.topk_recall(engine.pq_search(qf, flat, min(100, n), exclude=ids)[1], exact, ks)
    coarse = engine.topk_recall(engine.ivf_search(qf, ivf, min(100, n), 2, exclude=ids)[1], exact, ks)
    monkeypatch.setenv('GRL_EVAL_PQ', '8,4')
    r_pq, text_pq, raw_pq, none, none2 = run()
    assert none is None and none2 is None and not any(l.startswith('Refine') for l in text_pq)      # unset: no trace of it
    for dtype in TYPES:
        store = engine.RefineStore(gf.contiguous(), dtype)
        want = engine.topk_recall(engine.refine_search(qf, flat, store, k, R_, exclude=ids)[1], exact, ks)
        monkeypatch.setenv('GRL_EVAL_REFINE', '%d,%s' % (R_, dtype) if dtype == 'bf16' else str(R_))
        r_on, text_on, raw_pq_on, none, raw = run()
        assert r_on == r_pq and raw_pq_on == raw_pq and none is None                  # pq.json byte for byte
        assert len(text_on) == len(text_pq) + 2 and text_on[:len(text_pq) - 1] == text_pq[:-1] and text_on[-1] == text_pq[-1]
        new = text_on[len(text_pq) - 1:-1]
        assert new[0] == 'Refine: R = {}, k = {}, {} store of {} bytes against {} bytes of features'.format(
            R_, k, dtype, store.nbytes, 4 * n * d)
        assert new[1] == 'Refined PQ recall@1: {:.2%}  @10: {:.2%}  @100: {:.2%}  (ADC {:.2%}  {:.2%}  {:.2%})'.format(
            *(tuple(want) + tuple(adc)))
        js = json.loads(raw, parse_constant=refuse)
        assert (js['R'], js['k'], js['store'], js['store_bytes'], js['n'], js['n_queries']) == (R_, k, dtype, store.nbytes, n, nq)
        assert js['feature_bytes'] == 4 * n * d and 'ivf' not in js
        assert js['pq'] == {'refined_recall': dict(zip(('1', '10', '100'), want)), 'recall': dict(zip(('1', '10', '100'), adc))}
    # with the inverted lists too: their lines first, then the refined figures of both indexes
    monkeypatch.setenv('GRL_EVAL_IVF', '3,2')
    monkeypatch.delenv('GRL_EVAL_REFINE')
    r_ivf, text_ivf, raw_pq_ivf, raw_ivf, none = run()
    monkeypatch.setenv('GRL_EVAL_REFINE', '%d,bf16' % R_)
    r_on, text_on, raw_pq_on, raw_ivf_on, raw = run()
    assert r_on == r_ivf and raw_pq_on == raw_pq and raw_ivf_on == raw_ivf and none is None      # ivf.json byte for byte
    assert len(text_on) == len(text_ivf) + 3 and text_on[:len(text_ivf) - 1] == text_ivf[:-1] and text_on[-1] == text_ivf[-1]
    want_ivf = engine.topk_recall(engine.refine_search(qf, ivf, store, k, R_, nprobe=2, exclude=ids)[1], exact, ks)
    assert text_on[-2] == 'Refined IVF recall@1: {:.2%}  @10: {:.2%}  @100: {:.2%}  (IVF {:.2%}  {:.2%}  {:.2%})'.format(
        *(tuple(want_ivf) + tuple(coarse)))
    js = json.loads(raw, parse_constant=refuse)
    assert js['ivf'] == {'nprobe': 2, 'refined_recall': dict(zip(('1', '10', '100'), want_ivf)),
                         'recall': dict(zip(('1', '10', '100'), coarse))}
    assert js['pq']['refined_recall'] == dict(zip(('1', '10', '100'), want))
    monkeypatch.delenv('GRL_EVAL_PQ')
    monkeypatch.delenv('GRL_EVAL_IVF')
    with pytest.raises(ValueError, match='GRL_EVAL_REFINE=16,bf16 needs GRL_EVAL_PQ'):
        run()
