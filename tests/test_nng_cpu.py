"""The kNN-graph index contract of DESIGN.md 4af on the host: the numpy model tests/nng_ref.py against a brute-force set
formulation of the graph optimisation, the exhaustive property of the beam search in the model, the GRL_EVAL_NNG parser,
the default seeds, the binding and the host-side checks.  No device."""
import os

import numpy as np
import pytest
import torch

import nng_ref as G
import refine_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('grl_nng_search_lds_bytes', 'grl_nng_search', 'grl_nng_detours', 'grl_nng_merge')


def messy_lists(n, K, seed):
    """random candidate lists with padding (-1, n, far above), self entries and repeats in every row that has room"""
    g = np.random.Generator(np.random.PCG64(seed))
    knn = g.integers(0, n, (n, K)).astype(np.int64)
    for i in range(n):
        knn[i, g.integers(0, K)] = i
        if K > 2:
            knn[i, g.integers(0, K)] = (-1, n, 2 ** 40, -7)[i % 4]
        if K > 3:
            a, b = g.choice(K, 2, replace=False)
            knn[i, max(a, b)] = knn[i, min(a, b)]
    return knn


# ----------------------------------------------------------------------------
# graph optimisation: the model against sets
# ----------------------------------------------------------------------------
def brute_optimize(knn, D):
    """the contract written with sets and comprehensions instead of the model's loops"""
    n, K = knn.shape
    clean = []                                                     # per row: {position: id} of the live positions
    for i in range(n):
        row, seen = {}, set()
        for b in range(K):
            v = int(knn[i, b])
            if v != i and 0 <= v < n and v not in seen:
                row[b] = v
                seen.add(v)
        clean.append(row)
    fwd = []
    for i in range(n):
        det = {b: sum(1 for a in clean[i] if a < b and tb in {v for r, v in clean[clean[i][a]].items() if r < b})
               for b, tb in clean[i].items()}
        fwd.append([clean[i][b] for b in sorted(clean[i], key=lambda b: (det[b], b))[:D]])
    rev = [sorted((f.index(j), i) for i, f in enumerate(fwd) if j in f) for j in range(n)]
    rev = [[i for _, i in r] for r in rev]
    out = np.full((n, D), -1, np.int64)
    for i in range(n):
        got = list(fwd[i][:D // 2])
        fresh = [v for v in rev[i] if v not in got]
        got += fresh[:D // 2]
        got += [v for v in fwd[i][D // 2:] if v not in got]
        got += [v for v in rev[i] if v not in got]
        got = got[:D]
        out[i, :len(got)] = got
    return out


@pytest.mark.parametrize('n,K,D', ((9, 2, 2), (23, 4, 2), (23, 6, 6), (40, 12, 8), (31, 16, 4)))
def test_the_models_optimisation_equals_the_set_formulation(n, K, D):
    g = np.random.Generator(np.random.PCG64(n + K))
    exact = np.argsort(g.random((n, n)) + 4.0 * np.eye(n), axis=1)[:, :K]          # proper lists: unique, no self
    for knn in (exact, messy_lists(n, K, 3 * n + K)):
        N = G.optimize(knn, D)
        assert np.array_equal(N, brute_optimize(knn, D))
        assert np.array_equal(G.detours_fast(knn), G.detours(knn)) and np.array_equal(G.optimize(knn, D, fast=True), N)
        for i in range(n):
            row = N[i][N[i] >= 0]
            assert len(set(row)) == len(row) and i not in row and (row < n).all()
            assert (N[i][len(row):] == -1).all()                                   # padding last


def test_detours_count_two_hop_paths_by_rank():
    # 0 -> 1, 2, 3 and 1 -> 2 (rank 0), 2 -> 3 (rank 1): position 1 (id 2) has a detour through 1; position 2 (id 3) has
    # one through 2, whose row reaches 3 at rank 1 < 2, and none through 1
    knn = np.array([[1, 2, 3], [2, 0, 3], [0, 3, 1], [0, 1, 2]])
    det = G.detours(knn)
    assert det[0].tolist() == [0, 1, 1]
    assert G.forward(knn, det, 2)[0].tolist() == [1, 2]
    knn[0, 1] = 0                                                   # a self entry is padding: det -1, never chosen
    assert G.detours(knn)[0].tolist() == [0, -1, 0]


def test_the_optimiser_refuses_sizes_outside_the_domain():
    knn = np.zeros((5, 4), np.int64)
    for D in (0, 3, 6):
        with pytest.raises(ValueError):
            G.optimize(knn, D)
    with pytest.raises(ValueError):
        G.optimize(np.zeros((5, 1), np.int64), 2)


# ----------------------------------------------------------------------------
# beam search: the exhaustive property in the model
# ----------------------------------------------------------------------------
def ring(ids, n, D=2):
    """a table whose row i holds the next id of the ring `ids` first and padding behind it"""
    nbr = np.full((n, D), -1, np.int64)
    for a, b in zip(ids, list(ids[1:]) + [ids[0]]):
        nbr[a, 0] = b
    return nbr


@pytest.mark.parametrize('metric', ('cosine', 'euclidean'))
def test_a_ring_walked_to_the_end_is_the_exact_search(metric):
    g = np.random.Generator(np.random.PCG64(5))
    n, d, k = 21, 8, 6
    rows = g.standard_normal((n, d)).astype(np.float32)
    rows[7] = rows[3]                                              # a tie of whole rows: the smaller id first
    q = g.standard_normal((3, d)).astype(np.float32)
    dist, idx, stats = G.search(q, rows, ring(list(range(n)), n), [4], 32, 1, n, metric)
    want = F.refine_lists(q, rows, np.tile(np.arange(n), (3, 1)), k, metric)
    got = G.finish(dist, idx, k)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
    assert (stats[:, 0] == n).all() and (stats[:, 1] == n).all() and (idx[:, n:] == -1).all()
    # two disjoint rings seeded in one: the exact search over that ring alone
    a, b = list(range(0, n, 2)), list(range(1, n, 2))
    nbr = ring(a, n)
    nbr[b, 0] = ring(b, n)[b, 0]
    dist, idx, stats = G.search(q, rows, nbr, [b[2]], 32, 1, n, metric)
    want = F.refine_lists(q, rows, np.tile(np.array(b), (3, 1)), k, metric)
    got = G.finish(dist, idx, k)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
    assert (stats[:, 0] == len(b)).all() and (stats[:, 1] == len(b)).all()          # early stop: everything expanded


def test_the_model_keeps_visited_ids_out_and_caps_the_iterations():
    g = np.random.Generator(np.random.PCG64(6))
    n, d = 30, 4
    rows = g.standard_normal((n, d)).astype(np.float32)
    q = g.standard_normal((2, d)).astype(np.float32)
    nbr = g.integers(-1, n + 1, (n, 4))
    dist, idx, stats = G.search(q, rows, nbr, [0, 0, -1, n, 5], 8, 2, 3, 'cosine')
    assert (stats[:, 1] <= 3).all() and (stats[:, 0] <= 2 + 3 * 2 * 4).all()
    for r in range(2):
        live = idx[r][idx[r] >= 0]
        assert len(set(live)) == len(live)
        key = F.composite(F.sort_key(dist[r, :live.size]), live)
        assert (np.diff(key.astype(object)) > 0).all()
    junk = G.junk_mask(idx, (np.array([1, 2]), np.arange(n) % 3, np.array([0, 0]), np.zeros(n, int)))
    fd, fi = G.finish(dist, idx, 8, junk)
    for r in range(2):
        keep = idx[r][(idx[r] >= 0) & ~junk[r]]
        assert np.array_equal(fi[r, :keep.size], keep) and (fi[r, keep.size:] == -1).all() and np.isposinf(fd[r, keep.size:]).all()


# ----------------------------------------------------------------------------
# the knob, the seeds, the binding, the host-side checks
# ----------------------------------------------------------------------------
def test_the_evaluator_knob_parses():
    from grl_amd.reid.evaluator.attevaluator import parse_nng_knob as parse
    name = 'GRL_EVAL_NNG'
    assert parse(name, None) is None and parse(name, '') is None and parse(name, '  ') is None
    good, bad = G.parse_knob_cases()
    for text, want in good.items():
        assert parse(name, text) == want, text
    for text in bad:
        with pytest.raises(ValueError, match=name) as err:
            parse(name, text)
        assert repr(text) in str(err.value)


class _Never(object):
    def __getattr__(self, name):
        raise AssertionError('touched %s' % name)


KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_CLUSTER', 'GRL_EVAL_CLUSTER_JACCARD', 'GRL_EVAL_KMEANS', 'GRL_EVAL_HDBSCAN', 'GRL_EVAL_TSNE',
         'GRL_EVAL_SILHOUETTE', 'GRL_EVAL_PCA', 'GRL_EVAL_DIFFUSION', 'GRL_EVAL_SET', 'GRL_EVAL_PQ', 'GRL_EVAL_IVF',
         'GRL_EVAL_REFINE', 'GRL_EVAL_NNG')


def test_the_knob_is_refused_with_what_the_pq_knob_is_refused_with(monkeypatch):
    from grl_amd.reid.evaluator import ATTEvaluator
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)

    def run(only_eval=True, rerank=0):
        ATTEvaluator(_Never(), _Never(), only_eval).evaluate(None, None, _Never(), _Never(), '', 0, rerank)
    monkeypatch.setenv('GRL_EVAL_NNG', '16,8,48')
    with pytest.raises(ValueError, match="GRL_EVAL_NNG.*'16,8,48'"):
        run()
    monkeypatch.setenv('GRL_EVAL_NNG', '16,8')
    with pytest.raises(ValueError, match='GRL_EVAL_NNG=16,8 cannot re-rank'):
        run(rerank=1)
    for other, value in (('GRL_EVAL_SET', 'min'), ('GRL_EVAL_DIFFUSION', '10'), ('GRL_EVAL_METRIC', 'verify')):
        monkeypatch.setenv(other, value)
        with pytest.raises(ValueError, match='GRL_EVAL_NNG=16,8 cannot be combined with %s' % other):
            run()
        monkeypatch.delenv(other)
    for only_eval in (True, False):                               # accepted: it gets as far as the models and loaders
        with pytest.raises(AssertionError, match='touched'):
            run(only_eval=only_eval)


def test_the_default_seeds_are_evenly_spaced_and_deterministic():
    from grl_amd import engine
    for n, L in ((1, 8), (5, 8), (8, 8), (37, 16), (300, 64), (11310, 64), (2 ** 18, 512), (2 ** 31 - 1, 512)):
        s = engine.nng_default_seeds(n, L)
        assert s == engine.nng_default_seeds(n, L) == G.default_seeds(n, L).tolist()
        assert len(s) == min(L, n) and s[0] == 0 and all(0 <= v < n for v in s) and all(b > a for a, b in zip(s, s[1:]))
        assert s == [j * n // len(s) for j in range(len(s))]
        if len(s) > 1:
            gaps = {b - a for a, b in zip(s, s[1:])}
            assert max(gaps) - min(gaps) <= 1                      # evenly spaced


def test_library_exports_and_header_declare_the_entry_points():
    import ctypes
    from grl_amd import _lib, engine
    header = open(os.path.join(ROOT, 'include', 'grl_hip.h')).read()
    assert sorted(n for n in _lib._SIGNATURES if n.startswith('grl_nng_')) == sorted(NAMES)
    for name in NAMES:
        assert '%s(' % name in header, name
    srcs = open(os.path.join(ROOT, 'grl_amd', 'csrc', 'Makefile')).read().split('SRCS =')[1].split('\n')[0]
    assert ' nng.hip ' in srcs
    assert _lib.ABI_VERSION == 10 and int(header.split('#define GRL_ABI_VERSION')[1].split()[0]) == 10     # additive only
    for word, value in (('GRL_NNG_K_MAX', G.K_MAX), ('GRL_NNG_D_MAX', G.D_MAX), ('GRL_NNG_L_MIN', G.L_MIN),
                        ('GRL_NNG_L_MAX', G.L_MAX), ('GRL_NNG_W_MAX', G.W_MAX), ('GRL_NNG_WD_MAX', G.WD_MAX),
                        ('GRL_NNG_LDS_MAX', G.LDS_MAX)):
        assert int(header.split('#define %s' % word)[1].split()[0]) == value
    assert (engine.NNG_K_MAX, engine.NNG_D_MAX, engine.NNG_L_MIN, engine.NNG_L_MAX, engine.NNG_W_MAX, engine.NNG_WD_MAX,
            engine.NNG_LDS_MAX) == (G.K_MAX, G.D_MAX, G.L_MIN, G.L_MAX, G.W_MAX, G.WD_MAX, G.LDS_MAX)
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.exported_symbols() and getattr(lib, name).restype is not None and hasattr(raw, name), name


def test_the_lds_bytes_follow_the_header_and_the_defaults_fit():
    from grl_amd import _lib
    lib = _lib.load()
    for n, d, D, L, w, T, S in ((2 ** 18, 6144, 32, 64, 1, 64, 64), (37, 4, 2, 8, 1, 1, 1), (300, 1028, 16, 64, 8, 50, 5),
                                (100, 256, 64, 512, 4, 10 ** 6, 512), (2 ** 20, 16384, 32, 64, 1, 64, 64)):
        assert lib.grl_nng_search_lds_bytes(n, d, D, L, w, T, S) == G.lds_bytes(n, d, D, L, w, T, S)
    assert G.lds_bytes(2 ** 18, 6144, 32, 64, 1, 64, 64) == 58688 <= G.LDS_MAX       # the defaults at d = 6144
    assert G.table_slots(2 ** 18, 32, 1, 64, 64) == 8192 >= 2 * (64 + 64 * 32)
    assert G.table_slots(20, 32, 8, 10 ** 6, 8) == 64                               # never more than n ids
    for kw in (dict(L=48), dict(L=4), dict(L=1024), dict(D=3), dict(D=66), dict(w=0), dict(w=9), dict(w=8, D=64), dict(T=0),
               dict(S=0), dict(S=65), dict(d=6), dict(d=16388), dict(n=2 ** 31), dict(n=-1)):
        a = dict(n=100, d=256, D=32, L=64, w=1, T=64, S=64)
        a.update(kw)
        assert lib.grl_nng_search_lds_bytes(a['n'], a['d'], a['D'], a['L'], a['w'], a['T'], a['S']) == -1, kw


def test_host_argument_checks_return_einval_through_the_c_abi():
    from grl_amd import _lib
    lib = _lib.load()
    E = _lib.GRL_EINVAL
    # fake device pointers (never dereferenced: every call below is refused, or has nothing to launch)

    def go(q=0x1000, ldq=None, store=0x20000, lds=None, typ=0, nbr=0x3000, seeds=0x4000, stride=0, out=0x5000, oidx=0x6000,
           stats=0x7000, nq=0, n=100, d=256, D=32, L=64, w=1, T=64, S=64, metric=0):
        return lib.grl_nng_search(q, d if ldq is None else ldq, store, d if lds is None else lds, typ, nbr, seeds, stride, out,
                                  oidx, stats, nq, n, d, D, L, w, T, S, metric, None)
    assert go() == 0 and go(typ=1, metric=1, stride=64, store=0x20008) == 0          # nothing to do, nothing launched
    for kw in (dict(q=None), dict(store=None), dict(nbr=None), dict(seeds=None), dict(out=None), dict(oidx=None),
               dict(stats=None), dict(nq=-1), dict(nq=65536), dict(n=-1), dict(n=2 ** 31), dict(d=0), dict(d=6), dict(d=16388),
               dict(D=0), dict(D=3), dict(D=66), dict(L=4), dict(L=48), dict(L=1024), dict(w=0), dict(w=9), dict(w=8, D=64),
               dict(T=0), dict(S=0), dict(S=65), dict(typ=2), dict(metric=2), dict(ldq=252), dict(lds=258), dict(stride=5),
               dict(q=0x1008), dict(store=0x20008), dict(store=0x20004, typ=1), dict(nbr=0x3002), dict(seeds=0x4001),
               dict(out=0x5002), dict(oidx=0x6001), dict(stats=0x7002)):
        assert go(**kw) == E, kw
    assert b'nng_search' in lib.grl_last_error()
    assert go(n=2 ** 20, d=16384, T=1000) == E                                       # the LDS limit, before any launch
    msg = lib.grl_last_error().decode()
    assert str(G.lds_bytes(2 ** 20, 16384, 32, 64, 1, 1000, 64)) in msg and '65536' in msg

    def det(knn=0x1000, out=0x2000, n=0, K=8):
        return lib.grl_nng_detours(knn, out, n, K, None)
    assert det() == 0
    for kw in (dict(knn=None), dict(out=None), dict(n=-1), dict(n=2 ** 31), dict(K=1), dict(K=129), dict(knn=0x1002)):
        assert det(**kw) == E, kw
    assert b'nng_detours' in lib.grl_last_error()

    def mrg(fwd=0x1000, off=0x2000, rev=0x3000, out=0x4000, n=0, D=8):
        return lib.grl_nng_merge(fwd, off, rev, out, n, D, None)
    assert mrg() == 0
    for kw in (dict(fwd=None), dict(off=None), dict(rev=None), dict(out=None), dict(n=-1), dict(D=0), dict(D=3), dict(D=66),
               dict(off=0x2004), dict(rev=0x3001)):
        assert mrg(**kw) == E, kw
    assert b'nng_merge' in lib.grl_last_error()


def test_the_public_functions_validate_before_the_device(monkeypatch):
    from grl_amd import engine
    from grl_amd._lib import GrlHipError

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    monkeypatch.setattr(engine, '_call', no_device)
    host = torch.zeros(30, 256)
    store = engine.RefineStore.__new__(engine.RefineStore)
    store.n, store.d, store.dtype, store.data = 30, 256, 'f32', host
    with pytest.raises(ValueError, match='store must be a RefineStore'):
        engine.NnGraphIndex(host, torch.zeros((30, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match='neighbors must be an int32 device tensor'):
        engine.NnGraphIndex(store, torch.zeros((30, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match='neighbors must be on the device of the store'):
        engine.NnGraphIndex(store, torch.zeros((30, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="metric must be 'cosine' or 'euclidean'"):
        engine.NnGraphIndex(store, torch.zeros((30, 4), dtype=torch.int32), 'l1')
    vm = engine.VerifyMetric.__new__(engine.VerifyMetric)
    for fn, args in ((engine.NnGraphIndex, (store, torch.zeros((30, 4), dtype=torch.int32))), (engine.nng_knn, (store, 4)),
                     (engine.nng_build, (store,))):
        with pytest.raises(ValueError, match='verify_metric'):
            fn(*args, metric=vm)
    for K in (1, 129, 2.0):
        with pytest.raises(ValueError, match=r'nng_knn: K must be an integer in 2\.\.128'):
            engine.nng_knn(store, K)
    store.dtype = 'bf16'
    with pytest.raises(ValueError, match="store_or_xf must be an 'f32' RefineStore"):
        engine.nng_knn(store, 4)
    with pytest.raises(ValueError, match="knn is required with a 'bf16' RefineStore"):
        engine.nng_build(store, dtype='bf16')
    with pytest.raises(ValueError, match="dtype must be the store's own"):
        engine.nng_build(store)
    with pytest.raises(ValueError, match="dtype must be 'f32' or 'bf16'"):
        engine.nng_build(store, dtype='f16')
    store.dtype = 'f32'
    with pytest.raises(ValueError, match='knn must be an integer device tensor'):
        engine.nng_optimize(torch.zeros((30, 4), dtype=torch.int64), 2)
    with pytest.raises(ValueError, match='index must be an NnGraphIndex'):
        engine.nng_search(host, store, 3)
    with pytest.raises(ValueError, match='verify_metric'):
        engine.nng_search(host, vm, 3)
    index = engine.NnGraphIndex.__new__(engine.NnGraphIndex)
    index.store, index.n, index.d, index.D, index.metric = store, 30, 256, 32, 'cosine'
    with pytest.raises(ValueError, match=r'qf must be \[rows, d\] = \[rows, 256\]'):
        engine.nng_search(host[:, :128], index, 3)
    with pytest.raises(GrlHipError, match='HIP device'):
        engine.nng_search(host, index, 3)
