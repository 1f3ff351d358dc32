"""Gallery search and streaming ranking metrics on the device (engine.search / engine.rank_metrics_streaming,
search.hip) against the materialised path: cosin_dist / pairwise_distance_tensor + rank_rows + rank_metrics."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from grl_amd.synthetic import synth_eval_features

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def small():
    return synth_eval_features(40, 400, seed=1, n_ids=24, noise=7.0)


@pytest.fixture(scope='module')
def mars():
    return synth_eval_features(1980, 13290, seed=1)


@pytest.fixture(scope='module')
def wide():
    """A gallery beyond one LDS sort network (rank_rows' chunked regime)."""
    return synth_eval_features(48, 20000, seed=2, dim=768, n_ids=300)


def _full(metric, qf, gf):
    from grl_amd import engine
    return engine.cosin_dist(qf, gf) if metric == 'cosine' else engine.pairwise_distance_tensor(qf, gf)


def _dup(case):
    """Gallery with exact ties across block boundaries: rows 0..63 repeated at the end, pids/cams with them."""
    qf, gf, qp, qc, gp, gc = case
    rep = np.arange(64)
    return qf, torch.cat((gf, gf[rep]), 0), qp, qc, np.append(gp, gp[rep]), np.append(gc, gc[rep])


@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_column_blocks_are_bit_identical_to_the_full_matrix(metric, small, mars, wide):
    from grl_amd import engine
    for case, widths in ((small, [1, 7, 64, 256, 400, None]), (mars, [2048, None]), (wide, [4096, None])):
        qf, gf = case[0].to(DEV), case[1].to(DEV)
        full = _full(metric, qf, gf)
        for w in widths:
            blocks = engine._ColumnBlocks(qf, gf, metric, block_cols=w)
            assert blocks.spans[0][0] == 0 and blocks.spans[-1][1] == gf.shape[0]
            for c0, c1 in blocks.spans:
                assert torch.equal(blocks.block(c0, c1).view(torch.int32), full[:, c0:c1].view(torch.int32)), \
                    (metric, tuple(full.shape), w, c0, c1)
        # the default picks one block here; a small budget picks ragged 256-multiples
        blocks = engine._ColumnBlocks(qf, gf, metric, block_bytes=qf.shape[0] * 4 * 768)
        assert blocks.width == min(768, gf.shape[0]) and blocks.spans[-1][1] == gf.shape[0]
        for c0, c1 in blocks.spans:
            assert torch.equal(blocks.block(c0, c1).view(torch.int32), full[:, c0:c1].view(torch.int32))


def _check_search(qf, gf, k, metric, block_cols):
    from grl_amd import engine
    qf, gf = qf.to(DEV), gf.to(DEV)
    full = _full(metric, qf, gf)
    ref = engine.rank_rows(full).long()
    dist, idx = engine.search(qf, gf, k, metric=metric, block_cols=block_cols)
    assert dist.dtype == torch.float32 and idx.dtype == torch.int64 and dist.is_cuda and idx.is_cuda
    kk = min(k, gf.shape[0])
    assert torch.equal(idx[:, :kk], ref[:, :kk]), (metric, k, block_cols)
    assert torch.equal(dist[:, :kk].view(torch.int32), torch.gather(full, 1, ref[:, :kk]).view(torch.int32))
    if kk < k:
        assert bool((idx[:, kk:] == -1).all()) and bool(torch.isinf(dist[:, kk:]).all())


@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_search_equals_the_sorted_matrix(metric, small, mars, wide):
    qf, gf = small[0], small[1]
    for k, w in ((1, None), (10, 7), (100, 64), (256, 1), (1024, None), (1024, 100)):
        _check_search(qf, gf, k, metric, w)             # k = 1024 > 400 gallery entries: padded
    qf, gf = _dup(small)[:2]
    _check_search(qf, gf, 100, metric, 64)
    _check_search(qf, gf, 464, metric, 200)
    _check_search(mars[0], mars[1], 100, metric, 2048)
    _check_search(mars[0], mars[1], 100, metric, None)
    _check_search(mars[0][:300], mars[1], 1000, metric, 3000)
    _check_search(wide[0], wide[1], 100, metric, None)
    _check_search(wide[0], wide[1], 50, metric, 4096)


def test_search_ties_and_signed_zero():
    """Zero rows give -0 / +0 distances (NEGDOT of zero vectors); duplicated rows tie exactly."""
    from grl_amd import engine
    g = np.random.Generator(np.random.PCG64(5))
    gf = g.standard_normal((300, 64)).astype(np.float32)
    gf[10:20] = 0.0
    gf[200:210] = gf[0]
    qf = np.concatenate([gf[:5], np.zeros((3, 64), np.float32), -gf[5:8]], 0)
    _check_search(torch.from_numpy(qf), torch.from_numpy(gf), 40, 'cosine', 7)
    _check_search(torch.from_numpy(qf), torch.from_numpy(gf), 40, 'euclidean', 64)
    with pytest.raises(ValueError):
        engine.search(torch.from_numpy(qf).to(DEV), torch.from_numpy(gf).to(DEV), 1025)


def _order_key(bits):
    """order_key of grl_amd/csrc/sort_order.h on the uint32 bit patterns of float32 values (integer arithmetic, so
    that no host float operation meets a signalling NaN): canonical NaN, -0 -> +0, order-preserving uint32."""
    u = bits.copy()
    mag = u & np.uint32(0x7fffffff)
    u[mag > 0x7f800000] = 0x7fc00000                            # v != v
    u[mag == 0] = 0                                             # v == 0.f
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def test_argsort_topk_and_pair_hist_share_one_order():
    """grl_row_argsort, grl_topk_block and grl_pair_hist_block on one hand-made block of special values (no GEMM):
    both zeros, both infinities, NaN of either sign with and without payload, the smallest and largest denormal of
    either sign, +-FLT_MAX, each repeated on both sides of column 256 (topk_block_kernel's chunk), between normals.
    run_val carries the block's own bits (include/grl_hip.h), so a NaN comes back with the sign and payload it went
    in with; the canonical NaN 0x7fc00000 it is ranked as is read from the key half of run_key."""
    from grl_amd import engine
    from grl_amd._lib import ptr
    nq, n = 4, 320
    special = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7fa00001, 0xffc12345,
                        0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x7f7fffff, 0xff7fffff], np.uint32)
    g = np.random.Generator(np.random.PCG64(11))
    bits = g.standard_normal((nq, n)).astype(np.float32).view(np.uint32)
    for r in range(nq):                                         # 3 copies left of column 256, 2 right, shuffled per row
        left, right = g.permutation(256)[:3 * special.size], 256 + g.permutation(64)[:2 * special.size]
        bits[r, left] = np.tile(special, 3)
        bits[r, right] = np.tile(special, 2)
    key = _order_key(bits)
    nan = (bits & np.uint32(0x7fffffff)) > 0x7f800000
    assert nan.sum() == nq * 20 and (key[nan] == 0xffc00000).all()
    assert (key[(bits & np.uint32(0x7fffffff)) == 0] == 0x80000000).all()
    d = torch.from_numpy(bits.view(np.int32)).to(DEV).view(torch.float32)
    assert torch.equal(d.view(torch.int32).cpu(), torch.from_numpy(bits.view(np.int32)))        # every payload arrived

    order = engine.rank_rows(d).long()
    assert np.array_equal(order.cpu().numpy(), np.argsort(key, axis=1, kind='stable'))
    run_key = torch.full((nq, n), -1, dtype=torch.int64, device=DEV)
    run_val = torch.full((nq, n), float('inf'), dtype=torch.float32, device=DEV)
    engine._call('grl_topk_block', ptr(d), n, None, 0, nq, n, 0, n, ptr(run_key), ptr(run_val))
    assert torch.equal(run_key & 0xffffffff, order)
    assert torch.equal(run_val.view(torch.int32), torch.gather(d, 1, order).view(torch.int32))
    ranked_as = (run_key >> 32) & 0xffffffff                    # the key every entry was ranked by: NaN as 0x7fc00000
    assert np.array_equal(ranked_as.cpu().numpy(), np.take_along_axis(key, order.cpu().numpy(), 1).astype(np.int64))

    def hist(block, nrows):
        """neg histogram at bits = 8 of a contiguous block: every pair is a negative, nothing is junk"""
        ids = [torch.full((m,), v, dtype=torch.int32, device=DEV) for m, v in
               ((nrows, 0), (nrows, 0), (block.shape[1], 1), (block.shape[1], 0))]
        pos = torch.zeros(256, dtype=torch.int64, device=DEV)
        neg = torch.zeros(256, dtype=torch.int64, device=DEV)
        engine._pair_hist_block(block, 0, ids, 8, pos, neg)
        assert int(pos.sum()) == 0
        return neg.cpu().numpy()
    neg = hist(d, nq)
    assert neg.sum() == nq * n and np.array_equal(neg, np.bincount((key >> 24).ravel(), minlength=256))
    nans = d[0][torch.from_numpy(nan[0]).to(DEV)].contiguous().view(1, -1)       # 20 NaN of every kind: the last bin
    assert np.array_equal(np.flatnonzero(hist(nans, 1)), [255]) and nans.shape[1] == 20
    zeros = torch.tensor([[0x00000000, -0x80000000]], dtype=torch.int32, device=DEV).view(torch.float32)
    assert hist(zeros, 1)[128] == 2                                              # +0 and -0: one bin


def _per_query_ref(full, qp, gp, qc, gc):
    from grl_amd import engine, _lib
    from grl_amd._lib import ptr
    idx = engine.rank_rows(full)
    nq, ng = full.shape
    t = [torch.from_numpy(np.asarray(a).astype(np.int32)).to(DEV) for a in (qp, qc, gp, gc)]
    first = torch.empty(nq, dtype=torch.int32, device=DEV)
    nhit = torch.empty(nq, dtype=torch.int32, device=DEV)
    ap = torch.empty(nq, dtype=torch.float64, device=DEV)
    engine._call('grl_rank_metrics', ptr(idx), ng, ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), nq, ng, ptr(first),
                 ptr(nhit), ptr(ap))
    return idx, first.cpu().numpy(), nhit.cpu().numpy(), ap.cpu().numpy()


def _check_metrics(case, metric, block_cols, golden=None):
    from grl_amd import engine
    qf, gf, qp, qc, gp, gc = case
    qf, gf = qf.to(DEV), gf.to(DEV)
    full = _full(metric, qf, gf)
    idx, f_ref, n_ref, ap_ref = _per_query_ref(full, qp, gp, qc, gc)
    first, nhit, ap = (t.cpu().numpy() for t in
                       engine._rank_streaming(qf, gf, qp, gp, qc, gc, metric=metric, block_cols=block_cols))
    assert np.array_equal(first, f_ref) and np.array_equal(nhit, n_ref), (metric, block_cols)
    assert np.all(np.abs(ap - ap_ref) <= 1e-12 * np.abs(ap_ref)), np.abs(ap - ap_ref).max()
    with contextlib.redirect_stdout(io.StringIO()) as o1:
        cmc, mAP = engine.rank_metrics_streaming(qf, gf, qp, gp, qc, gc, metric=metric, block_cols=block_cols)
    with contextlib.redirect_stdout(io.StringIO()) as o2:
        cmc_r, map_r = engine.rank_metrics(idx, qp, gp, qc, gc)
    assert o1.getvalue() == o2.getvalue()
    assert cmc.dtype == cmc_r.dtype and np.array_equal(cmc, cmc_r) and isinstance(mAP, float)
    assert abs(mAP - map_r) <= 1e-12
    if golden is not None:
        assert np.allclose(cmc[:20], golden['cmc'], atol=1e-6) and abs(mAP - float(golden['mAP'])) < 1e-6


@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_streaming_metrics_match_the_materialised_path(metric, small, mars, wide, golden):
    for w in (1, 7, 64, 400, None):
        _check_metrics(small, metric, w, golden('evaluator_q40_g400.npz') if metric == 'cosine' else None)
    _check_metrics(_dup(small), metric, 64)
    _check_metrics(mars, metric, 2048)
    _check_metrics(mars, metric, None)
    _check_metrics(wide, metric, 4096)
    _check_metrics(wide, metric, None)


def test_streaming_metrics_small_gallery_and_unmatched_queries():
    """ng < max_rank keeps the note; queries whose pid is absent or whose only same-pid entries are junk are
    skipped exactly as rank_metrics skips them."""
    g = np.random.Generator(np.random.PCG64(9))
    gf = g.standard_normal((30, 32)).astype(np.float32)
    qf = gf[:6].copy()
    gp = g.integers(0, 5, 30); gc = g.integers(0, 3, 30)
    qp = np.array([gp[0], gp[1], 77, gp[3], 99, gp[5]]); qc = gc[:6].copy()
    gp[gp == qp[3]] = qp[3]; gc[gp == qp[3]] = qc[3]            # query 3: every same-pid entry is junk
    case = (torch.from_numpy(qf), torch.from_numpy(gf), qp, qc, gp, gc)
    _check_metrics(case, 'cosine', 7)
    _check_metrics(case, 'euclidean', None)


def test_streaming_memory_stays_below_a_quarter_of_the_matrix(mars):
    from grl_amd import engine
    qf, gf, qp, qc, gp, gc = mars
    qf, gf = qf.to(DEV), gf.to(DEV)
    engine.rank_metrics_streaming(qf[:8], gf[:512], qp[:8], gp[:512], qc[:8], gc[:512])   # warm the allocator path
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    engine.rank_metrics_streaming(qf, gf, qp, gp, qc, gc, block_cols=2048)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    assert grown < qf.shape[0] * gf.shape[0] * 4 / 4, grown


def test_attevaluator_streaming_prints_and_returns_the_same(synth_models, monkeypatch, capsys):
    from grl_amd.reid.evaluator import ATTEvaluator
    from grl_amd.synthetic import synth_clips
    cnn, siam, _ = synth_models
    cnn, siam = cnn.to(DEV).eval(), siam.to(DEV).eval()
    rng = np.random.Generator(np.random.PCG64(3))

    def items(n, seed):
        return (synth_clips(n, 2, seed=seed), torch.from_numpy(rng.integers(0, 3, n)),
                torch.from_numpy(rng.integers(0, 2, n)))
    q, g = items(4, 21), items(26, 22)
    ev = ATTEvaluator(cnn, siam, only_eval=False)
    monkeypatch.delenv('GRL_EVAL_STREAM', raising=False)
    capsys.readouterr()
    r_def = ev.evaluate(None, None, [q], [g], None, False, False)
    out_def = capsys.readouterr().out
    monkeypatch.setenv('GRL_EVAL_STREAM', '1')
    r_str = ev.evaluate(None, None, [q], [g], None, False, False)
    out_str = capsys.readouterr().out
    assert 'Mean AP:' in out_def and out_str == out_def and r_str == r_def
    with pytest.raises(ValueError, match='re-rank'):
        ev.evaluate(None, None, [q], [g], None, False, True)


# ----------------------------------------------------------------------------
# two ranks on one device (gloo): shards of the gallery columns
# ----------------------------------------------------------------------------
def _dist_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from grl_amd import engine
    sent = []
    real = {n: getattr(dist, n) for n in ('all_gather', 'all_reduce', 'all_gather_object', 'broadcast')}

    def counting(name):
        def f(*a, **kw):
            ts = [t for t in list(a) + list(kw.values()) if torch.is_tensor(t)]
            ts += [t for x in a if isinstance(x, (list, tuple)) for t in x if torch.is_tensor(t)]
            sent.append((name, max([t.numel() * t.element_size() for t in ts] or [0])))
            return real[name](*a, **kw)
        return f
    for n in real:
        setattr(dist, n, counting(n))
    res = {}
    for name, (nq, ng, w) in (('small', (40, 400, 64)), ('mid', (300, 3000, 512))):
        qf, gf, qp, qc, gp, gc = synth_eval_features(nq, ng, seed=1, n_ids=24 if nq == 40 else 200, noise=7.0)
        qf, gf = qf.to(DEV), gf.to(DEV)
        for metric in ('cosine', 'euclidean'):
            del sent[:]
            with contextlib.redirect_stdout(io.StringIO()):
                cmc, mAP = engine.rank_metrics_streaming(qf, gf, qp, gp, qc, gc, metric=metric, block_cols=w)
            d, i = engine.search(qf, gf, 50, metric=metric, block_cols=w)
            res[(name, metric)] = (cmc, mAP, d.cpu(), i.cpu(), list(sent), nq * ng * 4)
    for n in real:
        setattr(dist, n, real[n])
    out[rank] = res
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_shard_the_gallery_and_exchange_no_matrix():
    from grl_amd import engine
    world, port = 2, 29700 + (os.getpid() + 777) % 1500
    ctx = mp.get_context('spawn')
    out = ctx.Manager().dict()
    mp.spawn(_dist_worker, args=(world, port, out), nprocs=world, join=True)
    for name, (nq, ng, w) in (('small', (40, 400, 64)), ('mid', (300, 3000, 512))):
        qf, gf, qp, qc, gp, gc = synth_eval_features(nq, ng, seed=1, n_ids=24 if nq == 40 else 200, noise=7.0)
        qf, gf = qf.to(DEV), gf.to(DEV)
        for metric in ('cosine', 'euclidean'):
            with contextlib.redirect_stdout(io.StringIO()):
                cmc, mAP = engine.rank_metrics_streaming(qf, gf, qp, gp, qc, gc, metric=metric, block_cols=w)
            d, i = engine.search(qf, gf, 50, metric=metric, block_cols=w)
            for r in range(world):
                cmc_r, map_r, d_r, i_r, sent, matrix_bytes = out[r][(name, metric)]
                assert np.array_equal(cmc_r, cmc) and abs(map_r - mAP) <= 1e-12, (name, metric, r)
                assert torch.equal(i_r, i.cpu()) and torch.equal(d_r.view(torch.int32), d.cpu().view(torch.int32))
                assert sent and all(nbytes < matrix_bytes / 2 for _, nbytes in sent), sent      # a column shard is half
