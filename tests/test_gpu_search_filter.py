"""Junk-filtered gallery search on the device: grl_topk_block_filtered through the C ABI, engine.search(exclude=)
and engine.rerank_search(exclude=), one process and sharded over gloo ranks, and ATTEvaluator.evaluate(visual=1).

The yardstick is tests/search_filter_ref.py applied to the MATERIALISED ranking: rank_rows(D) with the junk entries
of each query (its pid AND camera) deleted, truncated to k, and D at those indices.  Indices must be equal and
distances bit-equal; nothing here has a tolerance."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import search_filter_ref as F
from grl_amd.synthetic import synth_eval_features

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda:0')


def _bits(t):
    return t.contiguous().view(torch.int32)


def _full(metric, qf, gf):
    from grl_amd import engine
    return engine.cosin_dist(qf, gf) if metric == 'cosine' else engine.pairwise_distance_tensor(qf, gf)


def _expect(D, k, ids, drop=None):
    """Host model on the materialised device ranking of D; (dist bits int32 [nq, k], idx int64 [nq, k]) numpy."""
    from grl_amd import engine
    order = engine.rank_rows(D).cpu().numpy()
    dist, idx = F.filter_ranked(order, D.cpu().numpy(), k, *ids, drop=drop)
    return dist.view(np.int32), idx


def _assert_result(got, D, k, ids, what, drop=None):
    dist, idx = got
    assert dist.dtype == torch.float32 and idx.dtype == torch.int64 and tuple(idx.shape) == (D.shape[0], k)
    want_d, want_i = _expect(D, k, ids, drop)
    assert np.array_equal(idx.cpu().numpy(), want_i), what
    assert np.array_equal(_bits(dist).cpu().numpy(), want_d), what
    return want_i


# ----------------------------------------------------------------------------
# 1. the kernel through the C ABI, on distance matrices given as a whole
# ----------------------------------------------------------------------------
def _dev_ids(ids):
    qp, gp, qc, gc = ids
    return [torch.from_numpy(np.asarray(a).astype(np.int32)).to(DEV) for a in (qp, qc, gp, gc)]


def _kernel_topk(D, k, ids, width, cidx=None, filtered=True):
    """Running top-k over column blocks of D [nq, ng] (device) with grl_topk_block(_filtered); with ``cidx`` [nq, ng]
    column j of row q is gallery entry cidx[q, j] (< 0: skipped) and D holds the distances in that column order."""
    from grl_amd import engine
    from grl_amd._lib import ptr
    nq, ng = D.shape
    t = _dev_ids(ids)
    run_key = torch.full((nq, k), -1, dtype=torch.int64, device=DEV)
    run_val = torch.full((nq, k), float('inf'), dtype=torch.float32, device=DEV)
    for c0 in range(0, ng, width):
        c1 = min(c0 + width, ng)
        d = D[:, c0:c1].contiguous()
        ci = None if cidx is None else cidx[:, c0:c1].contiguous()
        head = (ptr(d), c1 - c0, ptr(ci), c1 - c0 if ci is not None else 0, nq, c1 - c0, c0, k, ptr(run_key),
                ptr(run_val))
        if filtered:
            engine._call('grl_topk_block_filtered', *head, ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]))
        else:
            engine._call('grl_topk_block', *head)
    idx = run_key & 0xffffffff
    idx[idx == 0xffffffff] = -1
    return run_val, idx


def _special_case(seed=3, nq=24, ng=1500):
    """Distances from a handful of values (NaN, both zeros, infinities, exact ties) and heavy junk: 4 pids x 2
    cameras.  Query 0: its whole pid is junk.  Query 1: 40 junk entries at the very front (distance -2).  Query 2:
    a pid the gallery does not have."""
    g = np.random.Generator(np.random.PCG64(seed))
    pool = np.array([np.nan, -0.0, 0.0, -1.0, 0.5, 0.5, np.inf, -np.inf, 1e-30, -1e-30, 2.0, -2.5], np.float32)
    D = pool[g.integers(0, pool.size, (nq, ng))]
    rnd = g.random((nq, ng)) < 0.3
    D[rnd] = g.standard_normal(int(rnd.sum())).astype(np.float32)
    gp, gc = g.integers(0, 4, ng), g.integers(0, 2, ng)
    qp, qc = g.integers(0, 4, nq), g.integers(0, 2, nq)
    qp[0], qc[0] = 9, 1
    gp[g.choice(ng, 60, replace=False)] = 9
    gc[gp == 9] = 1                                           # query 0: every entry of its pid shares its camera
    qp[1], qc[1] = 0, 0
    junk1 = np.flatnonzero((gp == 0) & (gc == 0))
    assert junk1.size > 40
    D[1, junk1[:40]] = -2.0
    D[1, D[1] < -2.0] = 0.25                                  # nothing else before them but the other junk
    qp[2], qc[2] = 11, 3
    return D, (qp, gp, qc, gc)


@pytest.mark.parametrize('k', [1, 10, 100, 1024])
def test_kernel_equals_the_host_model_on_special_values(k):
    D, ids = _special_case()
    Dd = torch.from_numpy(D).to(DEV)
    junk = F.junk_mask(*ids)
    assert junk[0].sum() == 60 and (np.asarray(ids[1]) == 9).sum() == 60          # a whole pid is junk
    order1 = np.argsort(F.sort_key(D[1]), kind='stable')
    assert junk[1][order1[:40]].all()                          # 40 junk entries before the first kept one
    for width in (1500, 256, 100, 7):
        if width == 7 and k > 10:
            continue                                                               # (launch count, not coverage)
        want = _assert_result(_kernel_topk(Dd, k, ids, width), Dd, k, ids, (k, width))
        assert not junk[np.arange(D.shape[0])[:, None], np.maximum(want, 0)][want >= 0].any()
    # the host model from D alone agrees with the one on rank_rows(D)
    d2, i2 = F.filtered_topk(D, k, *ids)
    d1, i1 = _expect(Dd, k, ids)
    assert np.array_equal(i1, i2) and np.array_equal(d1, d2.view(np.int32))


def test_kernel_pads_when_fewer_than_k_entries_are_kept():
    g = np.random.Generator(np.random.PCG64(8))
    nq, ng = 5, 300
    D = g.standard_normal((nq, ng)).astype(np.float32)
    gp, gc = np.ones(ng, np.int64), np.zeros(ng, np.int64)
    gp[[7, 150, 299]] = 2                                     # three entries survive for the queries of pid 1 / camera 0
    qp, qc = np.array([1, 1, 1, 2, 1]), np.array([0, 0, 0, 0, 1])
    gc[[7, 150, 299]] = 0                                     # query 3 (pid 2, camera 0): exactly those three are junk
    ids = (qp, gp, qc, gc)
    Dd = torch.from_numpy(D).to(DEV)
    for k, width in ((10, 300), (10, 64), (1, 300), (1024, 128), (3, 300), (4, 299)):
        want = _assert_result(_kernel_topk(Dd, k, ids, width), Dd, k, ids, (k, width))
        assert set(want[0][want[0] >= 0].tolist()) <= {7, 150, 299}
        assert (want[0] >= 0).sum() == min(k, 3) and (want[3] >= 0).sum() == min(k, ng - 3)
        assert (want[4] >= 0).sum() == min(k, ng)             # another camera: nothing is junk
    # a query for which EVERYTHING is junk: the list stays empty
    ids = (np.array([1]), np.ones(ng, np.int64), np.array([0]), np.zeros(ng, np.int64))
    dist, idx = _kernel_topk(Dd[:1].contiguous(), 10, ids, 128)
    assert bool((idx == -1).all()) and bool(torch.isinf(dist).all()) and bool((dist > 0).all())


def test_kernel_with_explicit_column_indices():
    """cidx: the columns of every row are a permutation of the gallery of their own, some skipped (-1); the pid and
    camera of a column are those of its GALLERY INDEX."""
    D, ids = _special_case(seed=4, nq=12, ng=700)
    g = np.random.Generator(np.random.PCG64(6))
    nq, ng = D.shape
    perm = np.stack([g.permutation(ng) for _ in range(nq)])
    Dp = np.take_along_axis(D, perm, 1)
    skipped = g.random((nq, ng)) < 0.1                        # by column position
    cidx = np.where(skipped, -1, perm).astype(np.int32)
    drop = np.zeros((nq, ng), bool)
    np.put_along_axis(drop, perm, skipped, 1)                 # by gallery index
    Dd, Dpd, cd = torch.from_numpy(D).to(DEV), torch.from_numpy(Dp).to(DEV), torch.from_numpy(cidx).to(DEV)
    for k, width in ((10, 700), (100, 256), (1, 33), (1024, 700)):
        _assert_result(_kernel_topk(Dpd, k, ids, width, cidx=cd), Dd, k, ids, (k, width), drop=drop)


def test_a_filter_that_matches_nothing_is_the_unfiltered_kernel():
    D, ids = _special_case(seed=5)
    Dd = torch.from_numpy(D).to(DEV)
    nothing = (np.full(D.shape[0], -7), ids[1], ids[2], ids[3])
    for k, width in ((1, 1500), (10, 256), (100, 100), (1024, 512)):
        a = _kernel_topk(Dd, k, nothing, width)
        b = _kernel_topk(Dd, k, ids, width, filtered=False)
        assert torch.equal(a[1], b[1]) and torch.equal(_bits(a[0]), _bits(b[0])), (k, width)


def test_bad_arguments_are_refused():
    from grl_amd import _lib, engine
    from grl_amd._lib import ptr
    d = torch.zeros((2, 8), device=DEV)
    key = torch.full((2, 4), -1, dtype=torch.int64, device=DEV)
    val = torch.full((2, 4), float('inf'), device=DEV)
    i = torch.zeros(8, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.GrlHipError):
        engine._call('grl_topk_block_filtered', ptr(d), 8, None, 0, 2, 8, 0, 4, ptr(key), ptr(val), ptr(i), ptr(i),
                     None, ptr(i))
    with pytest.raises(_lib.GrlHipError):
        engine._call('grl_topk_block_filtered', ptr(d), 8, None, 0, 2, 8, 0, 1025, ptr(key), ptr(val), ptr(i), ptr(i),
                     ptr(i), ptr(i))
    qf = torch.zeros((2, 16), device=DEV)
    with pytest.raises(ValueError, match='g_pids'):
        engine.search(qf, qf, 1, exclude=([0, 1], [0], [0, 1], [0, 1]))
    with pytest.raises(ValueError, match='exclude'):
        engine.search(qf, qf, 1, exclude=([0, 1], [0, 1]))


# ----------------------------------------------------------------------------
# 2. engine.search(exclude=)
# ----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small():
    return synth_eval_features(40, 400, seed=1, n_ids=24, noise=7.0)


@pytest.fixture(scope='module')
def mars():
    return synth_eval_features(1980, 13290, seed=1)


def _check_search(case, k, metric, what=None, **kw):
    from grl_amd import engine
    qf, gf, qp, qc, gp, gc = case
    qf, gf = qf.to(DEV), gf.to(DEV)
    ids = (qp, gp, qc, gc)
    D = _full(metric, qf, gf)
    got = engine.search(qf, gf, k, metric=metric, exclude=ids, **kw)
    assert got[0].is_cuda and got[1].is_cuda
    return _assert_result(got, D, k, ids, (metric, k, kw, what)), D


@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_search_with_exclude_equals_the_filtered_sorted_matrix(metric, small, mars):
    # the evaluator's layout: the query rows lead the gallery, so every query has itself as junk at distance ~ -1 / 0
    qp, qc, gp, gc = small[2:]
    assert np.array_equal(gp[:40], qp) and np.array_equal(gc[:40], qc)
    for k, kw in ((1, {}), (10, dict(block_cols=7)), (100, dict(block_cols=64)), (256, dict(block_cols=1)),
                  (10, dict(block_cols=256)), (10, dict(block_cols=400)), (1024, {}), (1024, dict(block_cols=100)),
                  (50, dict(block_bytes=40 * 4 * 256))):          # width rule: 256-column blocks, ragged last one
        want, D = _check_search(small, k, metric, **kw)
        assert (want[:, 0] != np.arange(40)).all()                # never the query itself
    from grl_amd import engine
    blocks = engine._ColumnBlocks(small[0].to(DEV), small[1].to(DEV), metric, block_bytes=40 * 4 * 256)
    assert blocks.width == 256 and blocks.spans[-1] == (256, 400)
    _check_search(mars, 100, metric, block_cols=2048)
    _check_search(mars, 100, metric)
    blocks = engine._ColumnBlocks(mars[0].to(DEV), mars[1].to(DEV), metric, block_bytes=1980 * 4 * 3072)
    assert blocks.width == 3072 and blocks.spans[-1] == (12288, 13290)
    _check_search((mars[0][:300], mars[1], mars[2][:300], mars[3][:300], mars[4], mars[5]), 1000, metric,
                  block_bytes=300 * 4 * 3072)


def test_search_with_exclude_on_ties_signed_zeros_and_nan():
    """Zero rows give -0 / +0 distances, duplicated rows tie exactly, a NaN feature gives NaN distances."""
    g = np.random.Generator(np.random.PCG64(5))
    gf = g.standard_normal((300, 64)).astype(np.float32)
    gf[10:20] = 0.0
    gf[200:210] = gf[0]
    gf[250, 3] = np.nan
    qf = np.concatenate([gf[:5], np.zeros((3, 64), np.float32), -gf[5:8]], 0)
    gp, gc = g.integers(0, 6, 300), g.integers(0, 2, 300)
    gp[200:210], gc[200:205] = gp[0], gc[0]                       # half of query 0's exact ties are junk
    gp[250] = 99                                                  # the NaN column is junk for nobody
    qp, qc = np.append(gp[:5], g.integers(0, 6, 6)), np.append(gc[:5], g.integers(0, 2, 6))
    case = (torch.from_numpy(qf), torch.from_numpy(gf), qp, qc, gp, gc)
    for metric, w in (('cosine', 7), ('euclidean', 64), ('cosine', None)):
        want, D = _check_search(case, 40, metric, block_cols=w)
        assert metric != 'cosine' or bool(torch.isnan(D[:, 250]).all())
    want, _ = _check_search(case, 300, 'cosine', block_cols=33)       # the whole kept gallery: NaN entries last
    kept0 = want[0][want[0] >= 0]
    assert kept0[-1] == 250 and kept0.size == 300 - int(F.junk_mask(qp, gp, qc, gc)[0].sum())


def test_exclude_none_makes_the_same_calls_and_a_void_filter_changes_nothing(small, monkeypatch):
    from grl_amd import engine
    qf, gf, qp, qc, gp, gc = small
    qf, gf = qf.to(DEV), gf.to(DEV)
    seen = []
    real = engine._call

    def recording(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(engine, '_call', recording)
    for metric in ('cosine', 'euclidean'):
        D = _full(metric, qf, gf)
        ref = engine.rank_rows(D).long()
        del seen[:]
        d0, i0 = engine.search(qf, gf, 50, metric=metric, block_cols=64)
        plain = [n for n in seen if n.startswith('grl_topk')]
        assert plain == ['grl_topk_block'] * 7
        d1, i1 = engine.search(qf, gf, 50, metric=metric, exclude=None, block_cols=64)
        assert torch.equal(i1, i0) and torch.equal(_bits(d1), _bits(d0))
        assert torch.equal(i0, ref[:, :50]) and torch.equal(_bits(d0), _bits(torch.gather(D, 1, ref[:, :50])))
        del seen[:]
        void = (np.full(40, -3), gp, qc, gc)
        d2, i2 = engine.search(qf, gf, 50, metric=metric, exclude=void, block_cols=64)
        assert [n for n in seen if n.startswith('grl_topk')] == ['grl_topk_block_filtered'] * 7
        assert torch.equal(i2, i0) and torch.equal(_bits(d2), _bits(d0))


# ----------------------------------------------------------------------------
# 3. engine.rerank_search(exclude=)
# ----------------------------------------------------------------------------
RERANK_CASES = {
    'fixture': (40, 400, 1, dict(n_ids=24, noise=7.0), 64, (20, 6)),
    'k1k2_small': (33, 257, 4, dict(n_ids=20, noise=5.0), 32, (7, 1)),
    'n3000': (300, 2701, 7, dict(n_ids=200, noise=7.0), 512, (20, 6)),
}


def _rerank_inputs(name):
    nq, ng, seed, kw, width, ks = RERANK_CASES[name]
    qf, gf, qp, qc, gp, gc = synth_eval_features(nq, ng, seed=seed, **kw)
    return qf.to(DEV), gf.to(DEV), (qp, gp, qc, gc), width, ks


@pytest.mark.parametrize('name', sorted(RERANK_CASES))
def test_rerank_search_with_exclude_equals_the_filtered_materialised_re_ranking(name, monkeypatch):
    from grl_amd import engine
    from grl_amd.reid.evaluator.rerank import re_ranking
    qf, gf, ids, width, (k1, k2) = _rerank_inputs(name)
    Fm = re_ranking(engine.cosin_dist(qf, gf), engine.pairwise_distance_tensor(qf, qf),
                    engine.pairwise_distance_tensor(gf, gf), k1=k1, k2=k2, lambda_value=0.3)
    seen = []
    real = engine._call

    def recording(fn, *args):
        if fn.startswith('grl_topk'):
            seen.append((fn, int(args[5])))                      # ncols
        return real(fn, *args)
    monkeypatch.setattr(engine, '_call', recording)
    N = qf.shape[0] + gf.shape[0]
    for k in (1, 10, 1024):
        del seen[:]
        got = engine.rerank_search(qf, gf, k, k1=k1, k2=k2, exclude=ids, block_cols=width)
        _assert_result(got, Fm, k, ids, (name, k))
        # the K-nearest lists of the k-reciprocal sets (rows of length N) stay unfiltered; the final pass is filtered
        assert {n for f, n in seen if f == 'grl_topk_block'} == {N}
        final = [n for f, n in seen if f == 'grl_topk_block_filtered']
        assert final and sum(final) == gf.shape[0] and N not in final
    plain = engine.rerank_search(qf, gf, 10, k1=k1, k2=k2, block_cols=width)
    order = engine.rank_rows(Fm).long()
    assert torch.equal(plain[1], order[:, :10]) and torch.equal(_bits(plain[0]), _bits(torch.gather(Fm, 1, order[:, :10])))


# ----------------------------------------------------------------------------
# 4. worlds of two and three ranks on one device over gloo: equal to one process, bit for bit
# ----------------------------------------------------------------------------
SHARD_CASES = {
    # name -> (nq, ng, seed, synth keywords, block_cols, (k1, k2), evaluator layout)
    'fixture': (40, 400, 1, dict(n_ids=24, noise=7.0), 64, (20, 6), True),
    'disjoint': (100, 199, 12, dict(n_ids=30, noise=5.0), 32, (20, 6), False),
    'tiny_gallery': (40, 2, 14, dict(n_ids=3, noise=1.0), None, (20, 6), False),      # fewer columns than ranks
    'n3000': (300, 2701, 7, dict(n_ids=200, noise=7.0), 512, (20, 6), True),
}
SHARD_SMALL = ('fixture', 'disjoint', 'tiny_gallery')


def _shard_inputs(name):
    nq, ng, seed, kw, width, ks, layout = SHARD_CASES[name]
    if layout:
        qf, gf, qp, qc, gp, gc = synth_eval_features(nq, ng, seed=seed, **kw)
    else:
        _, x, _, _, pids, cams = synth_eval_features(1, nq + ng, seed=seed, **kw)
        qf, gf, qp, qc, gp, gc = x[:nq], x[nq:], pids[:nq], cams[:nq], pids[nq:], cams[nq:]
    if name == 'tiny_gallery':                      # one entry is junk for query 0, the other for nobody
        gp, gc = np.array([qp[0], qp[1]]), np.array([qc[0], qc[1] + 1])
    return qf.to(DEV), gf.to(DEV), (qp, gp, qc, gc), width, ks


def _run_shard_case(name):
    from grl_amd import engine
    qf, gf, ids, width, (k1, k2) = _shard_inputs(name)
    out = {}
    for metric in ('cosine', 'euclidean'):
        for k in (1, 50, 1024):
            d, i = engine.search(qf, gf, k, metric=metric, exclude=ids, block_cols=width)
            out['%s_%d' % (metric, k)] = (_bits(d).cpu(), i.cpu())
    for k in (10, 1024):
        d, i = engine.rerank_search(qf, gf, k, k1=k1, k2=k2, exclude=ids, block_cols=width)
        out['rerank_%d' % k] = (_bits(d).cpu(), i.cpu())
    return out


def _worker(rank, world, port, outdir, names):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    res = {name: _run_shard_case(name) for name in names}
    torch.save(res, os.path.join(outdir, 'rank%d.pt' % rank))
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


def _spawn(world, names, tmp_path_factory, port0):
    outdir = str(tmp_path_factory.mktemp('filter_w%d' % world))
    mp.spawn(_worker, args=(world, port0 + os.getpid() % 1500, outdir, names), nprocs=world, join=True)
    return [torch.load(os.path.join(outdir, 'rank%d.pt' % r), weights_only=False) for r in range(world)]


@pytest.fixture(scope='module')
def single():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run_shard_case(name)
        return cache[name]
    return get


@pytest.fixture(scope='module')
def world2(tmp_path_factory):
    return _spawn(2, SHARD_SMALL + ('n3000',), tmp_path_factory, 40100)


@pytest.fixture(scope='module')
def world3(tmp_path_factory):
    return _spawn(3, SHARD_SMALL, tmp_path_factory, 41700)


def _assert_ranks_equal(ranks, ref, name):
    for r, res in enumerate(ranks):
        assert sorted(res[name]) == sorted(ref)
        for key in ref:
            assert torch.equal(res[name][key][1], ref[key][1]), (name, key, 'rank', r)
            assert torch.equal(res[name][key][0], ref[key][0]), (name, key, 'rank', r)


@pytest.mark.parametrize('name', SHARD_SMALL)
def test_one_process_of_the_sharded_cases_equals_the_host_model(name, single):
    """What the ranks are compared with is itself the contract."""
    from grl_amd import engine
    qf, gf, ids, width, _ = _shard_inputs(name)
    got = single(name)
    for metric in ('cosine', 'euclidean'):
        D = _full(metric, qf, gf)
        for k in (1, 50, 1024):
            want_d, want_i = _expect(D, k, ids)
            assert np.array_equal(got['%s_%d' % (metric, k)][1].numpy(), want_i)
            assert np.array_equal(got['%s_%d' % (metric, k)][0].numpy(), want_d)


@pytest.mark.parametrize('name', SHARD_SMALL + ('n3000',))
def test_two_ranks_equal_one_process(name, world2, single):
    _assert_ranks_equal(world2, single(name), name)


@pytest.mark.parametrize('name', SHARD_SMALL)
def test_three_ranks_equal_one_process(name, world3, single):
    _assert_ranks_equal(world3, single(name), name)


# ----------------------------------------------------------------------------
# 5. ATTEvaluator.evaluate(visual=1) on the device
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('rerank', [0, 1])
def test_attevaluator_visual_writes_the_filtered_lists(rerank, synth_models, tmp_path, monkeypatch):
    import visual_tree as V
    from grl_amd import engine
    from grl_amd.reid.evaluator import ATTEvaluator
    from grl_amd.reid.evaluator.rerank import re_ranking
    from grl_amd.synthetic import synth_clips
    monkeypatch.chdir(tmp_path)
    for name in ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK'):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv('GRL_VISUAL_QUERIES', '1,4')
    query, gallery = V.make_tree('frames')['video']
    nq, ng = len(query), len(gallery)
    cnn, siam, _ = synth_models
    cnn, siam = cnn.to(DEV).eval(), siam.to(DEV).eval()

    def loader(items, seed):
        return [(synth_clips(len(items), 2, seed=seed), torch.tensor([i[1] for i in items]),
                 torch.tensor([i[2] for i in items]))]
    q, g = loader(query, 31), loader(gallery, 32)
    ev = ATTEvaluator(cnn, siam, only_eval=False)
    with contextlib.redirect_stdout(io.StringIO()) as o0:
        r0 = ev.evaluate(query, gallery, q, g, 'plain_', 0, rerank)
    with contextlib.redirect_stdout(io.StringIO()) as o1:
        r1 = ev.evaluate(query, gallery, q, g, 'run_', 1, rerank)
    assert r1 == r0 and not os.path.exists('plain_visual')
    keep = ('Mean AP', 'Rank-')
    assert [l for l in o1.getvalue().splitlines() if l.startswith(keep)] == \
        [l for l in o0.getvalue().splitlines() if l.startswith(keep)]
    # the lists against the materialised distances of the same features
    with contextlib.redirect_stdout(io.StringIO()):
        qf, qp, qc = ev.extract_feature(q)
        gf, gp, gc = ev.extract_feature(g)
    gf, gp, gc = torch.cat((qf, gf), 0), np.append(qp, gp), np.append(qc, gc)
    D = engine.cosin_dist(qf, gf)
    if rerank:
        D = re_ranking(D, engine.pairwise_distance_tensor(qf, qf), engine.pairwise_distance_tensor(gf, gf))
    want_d, want_i = _expect(D, 10, (qp, gp, qc, gc))
    ranked = json.load(open('run_visual/ranked.json'))
    assert sorted(ranked) == ['1', '4']
    everything = list(query) + list(gallery)
    got = V.listing('run_visual')
    for qi in (1, 4):
        rows = ranked[str(qi)]
        assert [r[0] for r in rows] == [int(x) for x in want_i[qi]]
        assert [np.float32(r[3]).view(np.int32) for r in rows] == list(want_d[qi])
        assert all(r[1] == gp[r[0]] and r[2] == gc[r[0]] for r in rows)
        qdir = os.path.basename(query[qi][0][0])
        for rank, gi in enumerate(want_i[qi], 1):
            names = sorted(p.rsplit('/', 1)[1] for p in got if p.startswith('%s/gallery_top%03d/' % (qdir, rank)))
            assert names == sorted(os.path.basename(p) for p in everything[gi][0]), (qi, rank)
        assert qi not in want_i[qi]                               # the prepended query itself is junk
