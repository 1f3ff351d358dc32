"""The kNN-graph index on the device (engine.nng_knn / nng_optimize / NnGraphIndex / nng_build / nng_search, nng.hip,
GRL_EVAL_NNG) against the numpy model of tests/nng_ref.py.  The model is fed with the DOWNLOADED store
values, tables, seeds and queries; every comparison of distances is on bit patterns, every id and stat is exact.  Recall
is asserted nowhere: the lists are the model's, so the model's recall is the kernel's."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import nng_ref as G
import refine_ref as F
from search_ref import sort_key, composite
from test_gpu_refine import HAND

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
METRICS = ('cosine', 'euclidean')
TYPES = ('f32', 'bf16')


def bits(a):
    if torch.is_tensor(a):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rand(n, d, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(g.standard_normal((n, d)).astype(np.float32)).to(DEV)


def _values(store):
    if store.dtype == 'f32':
        return store.data.cpu().numpy()
    return F.widen(store.data.view(torch.int16).cpu().numpy().view(np.uint16))


_stores = {}


def _store(n, d, dtype):
    """n rows of d columns; built once per key, never modified"""
    from grl_amd import engine
    if (n, d, dtype) not in _stores:
        _stores[n, d, dtype] = engine.RefineStore(_rand(n, d, 100 + d + n), dtype)
    return _stores[n, d, dtype]


def _table(n, D, seed):
    """a random table: mostly live ids, a few -1 / n / n + 5 entries, repeats as they fall"""
    g = np.random.Generator(np.random.PCG64(seed))
    t = g.integers(0, n, (n, D)).astype(np.int32)
    t[g.random((n, D)) < 0.08] = -1
    t[g.random((n, D)) < 0.04] = n
    t[g.random((n, D)) < 0.02] = n + 5
    return torch.from_numpy(t).to(DEV)


def _check(qf, index, L, w, T, seeds, note=None):
    """engine.nng_search at k = L against the model: distances by bits, ids and stats exactly"""
    from grl_amd import engine
    dv, di, st = engine.nng_search(qf, index, L, L, w, T, seeds=seeds, return_stats=True)
    assert dv.dtype == torch.float32 and di.dtype == torch.int64 and st.dtype == torch.int32
    assert tuple(dv.shape) == tuple(di.shape) == (qf.shape[0], L) and tuple(st.shape) == (qf.shape[0], 2)
    s = np.array(engine.nng_default_seeds(index.n, L)) if seeds is None else seeds.cpu().numpy()
    wd, wi, ws = G.search(qf.cpu().numpy(), _values(index.store), index.neighbors.cpu().numpy(), s, L, w, T, index.metric)
    assert np.array_equal(di.cpu().numpy(), wi), note
    assert np.array_equal(bits(dv), bits(wd)), note
    assert np.array_equal(st.cpu().numpy(), ws), note
    return dv, di, st


# ----------------------------------------------------------------------------
# 1. the walk against the model: a pruned sweep of the shapes
# ----------------------------------------------------------------------------
#        d     n   D   L  w   T   S  nq
SWEEP = ((4, 37, 2, 8, 1, 1, 1, 1),
         (252, 37, 4, 16, 2, 3, 5, 3),
         (260, 300, 16, 64, 8, 50, 64, 9),
         (1028, 300, 16, 16, 1, 50, 16, 3),
         (260, 300, 4, 8, 8, 3, 8, 9),
         (4, 300, 2, 64, 2, 50, 1, 1),
         (1028, 37, 16, 64, 1, 3, 5, 1),
         (252, 300, 4, 64, 2, 50, 5, 3),
         (2308, 37, 4, 16, 2, 6, 5, 3))             # nine full column chunks and a ragged one: the unrolled loop, its rest, the tail


@pytest.mark.parametrize('dtype', TYPES)
@pytest.mark.parametrize('metric', METRICS)
def test_the_walk_equals_the_model_on_the_downloaded_inputs(metric, dtype):
    from grl_amd import engine
    for d, n, D, L, w, T, S, nq in SWEEP:
        index = engine.NnGraphIndex(_store(n, d, dtype), _table(n, D, 7 * n + D), metric)
        assert (index.n, index.d, index.D, index.metric, index.nbytes) == (n, d, D, metric, 4 * n * D)
        qf = _rand(nq, d, 3 * d + nq)
        g = np.random.Generator(np.random.PCG64(S + L))
        seeds = torch.from_numpy(g.integers(0, n, (S,))).to(DEV)
        _, _, st = _check(qf, index, L, w, T, seeds, (d, n, D, L, w, T, S, nq))
        assert (st[:, 1] >= 1).all() and (st[:, 0] <= S + T * w * D).all()
    # the default seeds: S = min(L, n) evenly spaced rows
    for d, n, D, L in ((252, 37, 4, 64), (260, 300, 16, 16)):
        _check(_rand(2, d, 11), engine.NnGraphIndex(_store(n, d, dtype), _table(n, D, 7 * n + D), metric), L, 1, 5, None)


# ----------------------------------------------------------------------------
# 2. hand-made tables, seeds and stores
# ----------------------------------------------------------------------------
HAND_N, HAND_D = 12, 8
HAND_TABLE = ((1, 1, 2, -1),        # the same neighbour twice
              (3, -1, 12, 4),       # padding -1 and >= n in the middle; shares 3 with row 2 (two parents of one iteration)
              (3, 2, 5, 5),         # a self-loop and a repeat
              (-1, -1, -1, 40),     # no live neighbour
              (0, 6, 7, 8), (9, 4, 3, 2), (10, 11, 0, 1), (7, 7, 7, 7), (9, 10, 11, 3), (5, 8, 2, 1), (4, 6, 0, 12), (3, 3, -5, 10))


def _hand_store(dtype):
    from grl_amd import engine
    pat = np.array(HAND, np.uint32)
    x = pat[(np.arange(HAND_N * HAND_D) * 7) % pat.size].reshape(HAND_N, HAND_D).view(np.float32).copy()
    x[2] = 0.0                                                     # zeros, and a row of -0
    x[6] = -0.0
    x[4] = np.float32(0.5)
    x[9] = x[5] = np.linspace(-1, 1, HAND_D, dtype=np.float32)     # whole identical rows: the tie goes to the smaller id
    x[7] = np.float32(1.0)
    x[10, :] = 2.0
    x[10, 3] = np.inf
    x[11, :] = -1.0
    x[11, 1] = -np.inf
    return engine.RefineStore(torch.from_numpy(x).to(DEV), dtype)


@pytest.mark.parametrize('dtype', TYPES)
def test_hand_made_tables_seeds_and_special_values(dtype):
    from grl_amd import engine
    store = _hand_store(dtype)
    table = torch.tensor(HAND_TABLE, dtype=torch.int32, device=DEV)
    qf = _rand(4, HAND_D, 5).clone()
    qf[1] = 1.0
    qf[2] = 0.0
    qf[3, 2] = float('nan')
    shared = torch.tensor([0, 0, -1, 12, 2, 0], device=DEV)                      # repeats and padding
    per_query = torch.tensor([[0, 1], [3, 3], [-1, 7], [11, 12]], device=DEV)    # a seed without neighbours, one live seed
    saw = set()
    for metric in METRICS:
        index = engine.NnGraphIndex(store, table, metric)
        for w, T, L in ((1, 1, 8), (2, 2, 8), (2, 12, 16), (1, 12, 16), (8, 3, 8)):
            for seeds in (shared, per_query):
                dv, di, st = _check(qf, index, L, w, T, seeds, (metric, w, T, L))
                b, i = bits(dv), di.cpu().numpy()
                saw |= set(b[i >= 0].tolist())
                for r in range(4):                                 # rows 5 and 9 are the same row: the same bits, 5 first
                    p5, p9 = np.flatnonzero(i[r] == 5), np.flatnonzero(i[r] == 9)
                    if p5.size and p9.size:
                        assert p5[0] < p9[0] and b[r, p5[0]] == b[r, p9[0]]
        # a seed with no live neighbour: one iteration expands it, then nothing is left to expand
        _, di, st = _check(qf[:1], index, 8, 1, 12, torch.tensor([3], device=DEV))
        assert st.cpu().numpy().tolist() == [[1, 1]] and di.cpu().numpy()[0].tolist() == [3] + [-1] * 7
    assert 0x7fc00000 in saw and 0x7f800000 in saw and 0xff800000 in saw and 0x80000000 in saw     # NaN, +-inf, -0 (= -(+0))


# ----------------------------------------------------------------------------
# 3. the exhaustive property: a ring walked to the end is the exact search
# ----------------------------------------------------------------------------
def _ring(ids, n, D=2):
    nbr = np.full((n, D), -1, np.int32)
    for a, b in zip(ids, list(ids[1:]) + [ids[0]]):
        nbr[a, D - 1] = b
    return nbr


@pytest.mark.parametrize('dtype', TYPES)
@pytest.mark.parametrize('metric', METRICS)
def test_a_ring_walked_to_the_end_equals_refine_lists(metric, dtype):
    from grl_amd import engine
    n, d, k, nq = 37, 260, 10, 3
    store = _store(n, d, dtype)
    qf = _rand(nq, d, 21)
    everything = torch.arange(n, device=DEV).view(1, n).repeat(nq, 1)
    index = engine.NnGraphIndex(store, torch.from_numpy(_ring(list(range(n)), n)).to(DEV), metric)
    dv, di, st = engine.nng_search(qf, index, k, L=64, w=1, T=n, seeds=torch.tensor([5], device=DEV), return_stats=True)
    wv, wi = engine.refine_lists(qf, store, everything, k, metric)
    assert np.array_equal(bits(dv), bits(wv)) and torch.equal(di, wi)
    assert st.cpu().numpy().tolist() == [[n, n]] * nq
    # two disjoint rings, seeded in one: the exact search over that ring alone; the walk stops when all of it is expanded
    a, b = list(range(0, n, 3)), [i for i in range(n) if i % 3]
    nbr = _ring(a, n)
    nbr[b] = _ring(b, n)[b]
    index = engine.NnGraphIndex(store, torch.from_numpy(nbr).to(DEV), metric)
    for ids, T in ((a, n), (b, 1000)):                             # (T far above n: the table is sized by n)
        dv, di, st = engine.nng_search(qf, index, k, L=64, w=1, T=T, seeds=torch.tensor([ids[1]], device=DEV), return_stats=True)
        wv, wi = engine.refine_lists(qf, store, torch.tensor(ids, device=DEV).view(1, -1).repeat(nq, 1), k, metric)
        assert np.array_equal(bits(dv), bits(wv)) and torch.equal(di, wi)
        assert st.cpu().numpy().tolist() == [[len(ids), len(ids)]] * nq          # early stop: the iteration count


# ----------------------------------------------------------------------------
# 4. results, the junk rule, blocking, determinism
# ----------------------------------------------------------------------------
def test_k_below_L_padding_the_junk_rule_blocking_and_two_runs(monkeypatch):
    from grl_amd import engine
    n, d, D, L, nq = 300, 252, 16, 64, 9
    store = _store(n, d, 'f32')
    index = engine.NnGraphIndex(store, _table(n, D, 9), 'cosine')
    qf = _rand(nq, d, 31)
    full_v, full_i, full_s = _check(qf, index, L, 2, 20, None)
    for k in (1, 10, L):
        dv, di = engine.nng_search(qf, index, k, L, 2, 20)
        assert np.array_equal(bits(dv), bits(full_v[:, :k])) and torch.equal(di, full_i[:, :k])
    # the junk rule on the finished list of L
    g = np.random.Generator(np.random.PCG64(3))
    ids = (g.integers(0, 4, nq), g.integers(0, 4, n), g.integers(0, 2, nq), g.integers(0, 2, n))
    junk = G.junk_mask(full_i.cpu().numpy(), ids)
    assert junk.any() and (junk.sum(1) < L).all()
    for k in (10, L):
        dv, di = engine.nng_search(qf, index, k, L, 2, 20, exclude=ids)
        wv, wi = G.finish(full_v.cpu().numpy(), full_i.cpu().numpy(), k, junk)
        assert np.array_equal(bits(dv), bits(wv)) and np.array_equal(di.cpu().numpy(), wi)
    assert (wi[:, -1] == -1).all() and np.isposinf(wv[:, -1]).all()               # k = L with junk removed: padded
    # fewer than k live results: a ring of three
    nbr = np.full((n, 2), -1, np.int32)
    nbr[[4, 5, 6], 0] = [5, 6, 4]
    small = engine.NnGraphIndex(store, torch.from_numpy(nbr).to(DEV), 'cosine')
    dv, di = engine.nng_search(qf, small, 8, 8, 1, 10, seeds=torch.tensor([4], device=DEV))
    assert (np.sort(di.cpu().numpy()[:, :3], axis=1) == [4, 5, 6]).all() and (di[:, 3:] == -1).all()
    assert np.isposinf(dv.cpu().numpy()[:, 3:]).all()
    # query blocks forced small, and a second run: the same bits
    per_query = torch.from_numpy(g.integers(0, n, (nq, 5))).to(DEV)
    one = engine.nng_search(qf, index, L, L, 2, 20, seeds=per_query, return_stats=True)
    monkeypatch.setattr(engine, 'NNG_QUERY_BLOCK', 2)
    for seeds, want in ((None, (full_v, full_i, full_s)), (per_query, one)):
        for _ in range(2):
            got = engine.nng_search(qf, index, L, L, 2, 20, seeds=seeds, return_stats=True)
            assert np.array_equal(bits(got[0]), bits(want[0])) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    empty = engine.nng_search(qf[:0], index, 5)
    assert tuple(empty[0].shape) == tuple(empty[1].shape) == (0, 5)


# ----------------------------------------------------------------------------
# 5. the build: exact lists, the optimisation, the index
# ----------------------------------------------------------------------------
def _messy(n, K, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    knn = g.integers(0, n, (n, K)).astype(np.int64)
    for i in range(n):
        knn[i, g.integers(0, K)] = i
        if K > 2:
            knn[i, g.integers(0, K)] = (-1, n, 2 ** 40, -7)[i % 4]
        if K > 3:
            a, b = g.choice(K, 2, replace=False)
            knn[i, max(a, b)] = knn[i, min(a, b)]
    knn[n // 2] = -1                                               # a node without candidates
    return knn


@pytest.mark.parametrize('n,K,D', ((37, 4, 2), (37, 8, 8), (300, 16, 8), (300, 128, 64)))
def test_nng_optimize_equals_the_model(n, K, D):
    from grl_amd import engine
    exact = engine.nng_knn(_store(n, 256, 'f32'), K)          # (the exact lists go through the GEMM: d % 32 == 0)
    for knn in (exact, torch.from_numpy(_messy(n, K, n + K)).to(DEV), exact.to(torch.int32)):
        got = engine.nng_optimize(knn, D)
        assert got.dtype == torch.int32 and tuple(got.shape) == (n, D) and got.is_contiguous()
        assert np.array_equal(got.cpu().numpy(), G.optimize(knn.cpu().numpy(), D, fast=True))
        if knn.dtype == torch.int32:
            break


@pytest.mark.parametrize('metric', METRICS)
def test_nng_knn_is_the_exact_search_with_self_removed(metric):
    from grl_amd import engine
    n, d = 37, 256
    store = _store(n, d, 'f32')
    D = (engine.cosin_dist if metric == 'cosine' else engine.pairwise_distance_tensor)(store.data, store.data).cpu().numpy()
    for K in (2, 36, 40):                                          # 40 > n - 1: the tail is padding
        got = engine.nng_knn(store, K, metric).cpu().numpy()
        assert got.dtype == np.int64 and got.shape == (n, K)
        for i in range(n):
            others = np.array([j for j in range(n) if j != i])
            want = others[np.argsort(composite(sort_key(D[i, others]), others), kind='stable')][:K]
            assert np.array_equal(got[i, :want.size], want) and (got[i, want.size:] == -1).all()
    assert torch.equal(engine.nng_knn(store.data, 5, metric), engine.nng_knn(store, 5, metric))        # rows or a store
    assert torch.equal(engine.nng_knn(store, 5, metric, block_bytes=4096), engine.nng_knn(store, 5, metric))


def test_nng_build_is_the_index_over_the_optimised_exact_lists():
    from grl_amd import engine
    n, d = 300, 256
    xf = _store(n, d, 'f32').data
    for dtype in TYPES:
        index = engine.nng_build(xf, K=16, D=8, metric='euclidean', dtype=dtype)
        want = engine.NnGraphIndex(engine.RefineStore(xf, dtype), engine.nng_optimize(engine.nng_knn(xf, 16, 'euclidean'), 8),
                                   'euclidean')
        assert torch.equal(index.neighbors, want.neighbors) and torch.equal(index.store.data, want.store.data)
        assert (index.n, index.d, index.D, index.metric, index.store.dtype) == (n, d, 8, 'euclidean', dtype)
        assert index.nbytes == 4 * n * 8 + (2 * n * d if dtype == 'bf16' else 0)      # a bf16 copy is the index's own
        _check(_rand(3, d, 2), index, 16, 1, 20, None)
    store = engine.RefineStore(xf, 'bf16')
    knn = engine.nng_knn(xf, 16)
    mine = engine.nng_build(store, D=8, dtype='bf16', knn=knn)     # a caller's store and lists
    assert mine.store is store and mine.nbytes == 4 * n * 8 and torch.equal(mine.neighbors, engine.nng_optimize(knn, 8))


# ----------------------------------------------------------------------------
# 6. refusals
# ----------------------------------------------------------------------------
def test_refusals_name_the_argument():
    from grl_amd import engine
    n, d = 37, 252
    store = _store(n, d, 'f32')
    table = _table(n, 4, 1)
    index = engine.NnGraphIndex(store, table, 'cosine')
    qf = _rand(3, d, 1)
    for bad, word in ((table.to(torch.int64), 'neighbors must be an int32 device tensor'), (table.cpu(), 'on the device of the store'),
                      (table[:30].contiguous(), 'one row per store row'), (table[:, :3].contiguous(), 'D even in 2..64'),
                      (_table(n, 8, 1)[:, ::2], 'neighbors must be contiguous'), (_table(n, 66, 1), 'D even in 2..64')):
        with pytest.raises(ValueError, match=word):
            engine.NnGraphIndex(store, bad, 'cosine')
    with pytest.raises(ValueError, match='store must be a RefineStore'):
        engine.NnGraphIndex(store.data, table)
    with pytest.raises(ValueError, match="metric must be 'cosine' or 'euclidean'"):
        engine.NnGraphIndex(store, table, 'l1')
    vm = engine.VerifyMetric.__new__(engine.VerifyMetric)
    with pytest.raises(ValueError, match='verify_metric'):
        engine.NnGraphIndex(store, table, vm)
    with pytest.raises(ValueError, match='verify_metric'):
        engine.nng_search(qf, vm, 3)
    with pytest.raises(ValueError, match='verify_metric'):
        engine.nng_build(store, metric=vm)
    for kw, word in ((dict(k=0), r'k \(k <= L = 64\) must be an integer in 1\.\.64'), (dict(k=65), r'k \(k <= L = 64\)'),
                     (dict(k=9, L=8), r'k \(k <= L = 8\)'), (dict(L=48), 'L must be a power of two in 8..512'),
                     (dict(L=4), r'L \(a power of two\) must be an integer in 8\.\.512'), (dict(L=1024), r'in 8\.\.512'),
                     (dict(w=0), r'w must be an integer in 1\.\.8'), (dict(w=9), r'w must be an integer in 1\.\.8'),
                     (dict(T=0), 'T must be an integer in 1'), (dict(T=2.5), 'T must be an integer'),
                     (dict(seeds=[1, 2]), 'seeds must be an integer device tensor'),
                     (dict(seeds=torch.tensor([1, 2])), 'seeds must be an integer device tensor'),
                     (dict(seeds=torch.zeros(3, device=DEV)), 'seeds must be an integer device tensor'),
                     (dict(seeds=torch.zeros((2, 4), dtype=torch.int64, device=DEV)), 'one row per query: 3'),
                     (dict(seeds=torch.zeros((0,), dtype=torch.int64, device=DEV)), '1 <= S <= L = 64'),
                     (dict(seeds=torch.zeros((9,), dtype=torch.int64, device=DEV), L=8), '1 <= S <= L = 8'),
                     (dict(exclude=(1, 2, 3)), 'exclude must be')):
        a = dict(k=3)
        a.update(kw)
        with pytest.raises(ValueError, match=word):
            engine.nng_search(qf, index, **a)
    with pytest.raises(ValueError, match=r'w must keep w \* D <= 256 \(got w = 5 with D = 64\)'):
        engine.nng_search(qf, engine.NnGraphIndex(store, _table(n, 64, 1)), 3, w=5)
    with pytest.raises(ValueError, match=r'qf must be \[rows, d\] = \[rows, 252\]'):
        engine.nng_search(qf[:, :248], index, 3)
    with pytest.raises(ValueError, match='index must be an NnGraphIndex'):
        engine.nng_search(qf, store, 3)
    # the LDS limit: both numbers
    big = engine.RefineStore(torch.zeros((2200, 12288), device=DEV))
    wide = engine.NnGraphIndex(big, torch.full((2200, 32), -1, dtype=torch.int32, device=DEV))
    need = G.lds_bytes(2200, 12288, 32, 64, 1, 64, 64)
    assert need > G.LDS_MAX
    with pytest.raises(ValueError, match='need %d bytes of LDS, the limit is 65536' % need):
        engine.nng_search(torch.zeros((1, 12288), device=DEV), wide, 3)
    engine.nng_search(torch.zeros((1, 12288), device=DEV), wide, 3, T=8)          # a shorter walk fits
    for bad, word in ((torch.zeros((5, 1), dtype=torch.int64, device=DEV), 'K in 2..128'),
                      (torch.zeros((5, 129), dtype=torch.int64, device=DEV), 'K in 2..128'),
                      (torch.zeros((5, 4), device=DEV), 'knn must be an integer device tensor'),
                      (torch.zeros((5, 4), dtype=torch.int64), 'knn must be an integer device tensor')):
        with pytest.raises(ValueError, match=word):
            engine.nng_optimize(bad, 2)
    knn = torch.zeros((5, 4), dtype=torch.int64, device=DEV)
    for D in (0, 6, 2.0):
        with pytest.raises(ValueError, match='nng_optimize: D '):
            engine.nng_optimize(knn, D)
    with pytest.raises(ValueError, match='D must be even'):
        engine.nng_optimize(knn, 3)
    with pytest.raises(ValueError, match=r'K must be an integer in 2\.\.128'):
        engine.nng_knn(store, 1)
    with pytest.raises(ValueError, match="must be an 'f32' RefineStore"):
        engine.nng_knn(_store(n, d, 'bf16'), 4)
    with pytest.raises(ValueError, match="dtype must be the store's own"):
        engine.nng_build(store, dtype='bf16')
    with pytest.raises(ValueError, match="knn is required with a 'bf16' RefineStore"):
        engine.nng_build(_store(n, d, 'bf16'), dtype='bf16')
    with pytest.raises(ValueError, match='knn must have one row per store row'):
        engine.nng_build(store, knn=knn)


# ----------------------------------------------------------------------------
# 7. ATTEvaluator.evaluate with GRL_EVAL_NNG
# ----------------------------------------------------------------------------
KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_CLUSTER', 'GRL_EVAL_CLUSTER_JACCARD', 'GRL_EVAL_KMEANS', 'GRL_EVAL_HDBSCAN', 'GRL_EVAL_TSNE',
         'GRL_EVAL_SILHOUETTE', 'GRL_EVAL_PCA', 'GRL_EVAL_DIFFUSION', 'GRL_EVAL_SET', 'GRL_EVAL_PQ', 'GRL_EVAL_IVF',
         'GRL_EVAL_REFINE', 'GRL_EVAL_NNG')


def test_attevaluator_reports_the_graph_recall_last_and_nothing_else_changes(synth_models, monkeypatch, tmp_path):
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
    files = [os.path.join(str(tmp_path), f) for f in ('pq.json', 'nng.json')]

    def run():
        for f in files:
            if os.path.exists(f):
                os.remove(f)
        with contextlib.redirect_stdout(io.StringIO()) as o:
            r = ev.evaluate(None, None, q_loader, g_loader, path, 0, 0)
        return (r, o.getvalue().splitlines()) + tuple(open(f).read() if os.path.exists(f) else None for f in files)

    def refuse(c):
        raise ValueError('not strict JSON: %s' % c)

    for pq in (None, '8,4'):
        if pq:
            monkeypatch.setenv('GRL_EVAL_PQ', pq)
        r_off, text_off, raw_pq, none = run()
        assert none is None and not any(l.startswith('NNG') for l in text_off)        # unset: no trace of it
        for value, (K, D, L, w, T, dtype) in (('8,4,8,2,5', (8, 4, 8, 2, 5, 'f32')), ('8,4,16,1,6,bf16', (8, 4, 16, 1, 6, 'bf16'))):
            monkeypatch.setenv('GRL_EVAL_NNG', value)
            r_on, text_on, raw_pq_on, raw = run()
            monkeypatch.delenv('GRL_EVAL_NNG')
            assert r_on == r_off and raw_pq_on == raw_pq                              # the figures and pq.json byte for byte
            assert len(text_on) == len(text_off) + 4 and text_on[:len(text_off) - 1] == text_off[:-1] and text_on[-1] == text_off[-1]
            new = text_on[len(text_off) - 1:-1]
            index = engine.nng_build(gf.contiguous(), K, D, 'cosine', dtype)
            k = min(100, L, n)
            _, approx, stats = engine.nng_search(qf, index, k, L, w, T, exclude=ids, return_stats=True)
            recall = engine.topk_recall(approx, engine.search(qf, gf, k, exclude=ids)[1], (1, 10, 100))
            visited = float(stats[:, 0].sum()) / nq
            assert new[0] == 'NNG: K = {}, D = {}, L = {}, w = {}, T = {}, {} store, {} rows'.format(K, D, L, w, T, dtype, n)
            assert new[1] == 'NNG recall@1: {:.2%}  @10: {:.2%}  @100: {:.2%}  (k = {})'.format(*(tuple(recall) + (k,)))
            assert new[2].startswith('NNG visited rows per query: {:.1f} of {} '.format(visited, n))
            assert new[3] == 'NNG index: {} bytes against {} bytes of features'.format(index.nbytes, 4 * n * d)
            js = json.loads(raw, parse_constant=refuse)
            assert js['recall'] == dict(zip(('1', '10', '100'), recall)) and js['visited_mean'] == visited
            assert (js['K'], js['D'], js['L'], js['w'], js['T'], js['store'], js['n'], js['n_queries'], js['k'], js['index_bytes']) == \
                (K, D, L, w, T, dtype, n, nq, k, index.nbytes)
    monkeypatch.setenv('GRL_EVAL_NNG', '8,4')
    with pytest.raises(ValueError, match='GRL_EVAL_NNG=8,4 cannot re-rank'):
        ev.evaluate(None, None, q_loader, g_loader, path, 0, 1)
