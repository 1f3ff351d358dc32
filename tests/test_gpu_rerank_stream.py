"""Streaming k-reciprocal re-ranking (engine.rerank_search / engine.rerank_metrics_streaming, rerank_stream.hip)
against the materialised device re-ranking (rerank.hip: grl_rerank_build / rank_rows / grl_rerank_krecip /
grl_rerank_expand / grl_rerank_jaccard) as the yardstick: every intermediate and the result bit for bit."""
import contextlib
import io

import numpy as np
import pytest
import torch

from grl_amd.synthetic import synth_eval_features

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
# (nq, ng, k1, k2, lambda, seed) of test_device_re_ranking_matches_reference_golden_and_numpy
CASES = ((48, 600, 20, 6, 0.3, 3), (33, 257, 7, 1, 0.5, 4), (20, 300, 12, 3, 0.1, 5))


def _feats(nq, ng, seed, **kw):
    qf, gf, qp, qc, gp, gc = synth_eval_features(nq, ng, seed=seed, **kw)
    return qf.to(DEV), gf.to(DEV), qp, qc, gp, gc


def _bits(t):
    return t.contiguous().view(torch.int32)


def _materialised(qf, gf, k1, k2, lam):
    """The five launches of rerank.py's _re_ranking_device, keeping every intermediate (no N limit)."""
    from grl_amd import _lib, engine
    from grl_amd._lib import ptr
    import ctypes as C

    def call(name, *args):
        _lib.check(getattr(_lib.load(), name)(*args, _lib.stream()), name)
    qg, qq, gg = engine.cosin_dist(qf, gf), engine.pairwise_distance_tensor(qf, qf), \
        engine.pairwise_distance_tensor(gf, gf)
    nq, ng = qg.shape
    N = nq + ng
    D = torch.empty((N, N), dtype=torch.float32, device=DEV)
    colmax = torch.empty(N, dtype=torch.float32, device=DEV)
    call('grl_rerank_build', ptr(qg), ptr(qq), ptr(gg), nq, ng, ptr(D), ptr(colmax))
    rank = engine.rank_rows(D)
    V = torch.zeros((N, N), dtype=torch.float32, device=DEV)
    lcnt = torch.empty(N, dtype=torch.int32, device=DEV)
    lidx = torch.empty((N, 256), dtype=torch.int32, device=DEV)
    call('grl_rerank_krecip', ptr(D), ptr(rank), N, k1, ptr(V), ptr(lcnt), ptr(lidx))
    V2T = torch.zeros((N, N), dtype=torch.float32, device=DEV)
    V2q = torch.zeros((nq, N), dtype=torch.float32, device=DEV)
    call('grl_rerank_expand', ptr(V), ptr(rank), ptr(lcnt), ptr(lidx), N, nq, k2, ptr(V2T), ptr(V2q))
    F = None
    if N <= 16384:
        F = torch.empty((nq, ng), dtype=torch.float32, device=DEV)
        call('grl_rerank_jaccard', ptr(V2q), ptr(V2T), ptr(D), N, nq, C.c_float(lam), C.c_float(1 - lam), ptr(F))
    return dict(D=D, colmax=colmax, rank=rank, V=V, lcnt=lcnt, lidx=lidx, V2T=V2T, V2q=V2q, F=F)


def _check_sparse(rr, m):
    """rr (engine._Rerank) against the materialised intermediates m."""
    N, K = rr.N, rr.K
    assert torch.equal(_bits(rr.colmax), _bits(m['colmax']))
    assert torch.equal(rr.rank, m['rank'][:, :K])
    assert torch.equal(rr.lcnt, m['lcnt'])
    valid = torch.arange(256, device=DEV)[None, :] < rr.lcnt[:, None].long()
    assert torch.equal(rr.lidx[valid], m['lidx'][valid])
    rows = torch.arange(N, device=DEV)[:, None].expand(N, 256)[valid]
    assert torch.equal(_bits(rr.lval[valid]), _bits(m['V'][rows, rr.lidx[valid].long()]))
    assert int((m['V'] != 0).sum()) == int(valid.sum())
    # V2: CSR rows = the non-zeros of V2T's columns, in ascending order, bit for bit
    nnz = int(rr.row_ptr[-1])
    V2 = m['V2T'].t()
    nz = V2 != 0
    assert nnz == int(nz.sum())
    cnt = rr.row_ptr[1:] - rr.row_ptr[:-1]
    assert torch.equal(cnt, nz.sum(1))
    r_idx, c_idx = nz.nonzero(as_tuple=True)                    # row-major: ascending column within a row
    assert torch.equal(rr.col[:nnz].long(), c_idx)
    assert torch.equal(_bits(rr.val[:nnz]), _bits(V2[r_idx, c_idx]))
    assert torch.equal(_bits(m['V2q']), _bits(m['V2T'][:, :rr.nq].t()))


def test_d_rows_and_rank_lists_equal_rerank_build():
    """D rows of the sample blocks (several widths, ragged last blocks, blocks straddling the query/gallery
    boundary) are grl_rerank_build's bits; the query-side row blocks of q x g are the full matrix's bits."""
    from grl_amd import engine
    qf, gf, *_ = _feats(48, 600, 3, n_ids=40, noise=4.0)
    m = _materialised(qf, gf, 20, 6, 0.3)
    full_qg = engine.cosin_dist(qf, gf)
    for w in (1, 7, 32, 100, 256, None):
        sb = engine._SampleBlocks(qf, gf, block_cols=w)
        assert sb.spans[-1][1] == 648
        colmax = torch.full((648,), float('nan'), device=DEV)
        straddle = 0
        for i0, i1 in sb.spans:
            straddle += i0 < 48 < i1
            dr = sb.d_rows(i0, i1, colmax)
            assert torch.equal(_bits(dr), _bits(m['D'][i0:i1])), (w, i0, i1)
            for s0, s1, up, ldu, lo, lrs, lcs in sb.segments(i0, i1):
                if s0 < 48:
                    assert torch.equal(_bits(lo), _bits(full_qg[s0:s1])), (w, s0, s1)
        assert torch.equal(_bits(colmax), _bits(m['colmax']))
        if w in (7, 100):
            assert straddle == 1
    for w in (7, None):
        rr = engine._Rerank(qf, gf, 20, 6, 0.3, block_cols=w)
        assert torch.equal(rr.rank, m['rank'][:, :21])


@pytest.mark.parametrize('case', CASES + ((1980, 13290, 20, 6, 0.3, 1),), ids=['c0', 'c1', 'c2', 'mars'])
def test_sparse_weights_and_expansion_equal_the_dense_ones(case):
    from grl_amd import engine
    nq, ng, k1, k2, lam, seed = case
    kw = dict(n_ids=40, noise=4.0) if nq < 100 else {}
    qf, gf, *_ = _feats(nq, ng, seed, **kw)
    m = _materialised(qf, gf, k1, k2, lam)
    rr = engine._Rerank(qf, gf, k1, k2, lam)
    _check_sparse(rr, m)


def _check_search_and_metrics(qf, gf, qp, qc, gp, gc, k1, k2, lam, widths, F=None):
    from grl_amd import engine
    from grl_amd.reid.evaluator.rerank import re_ranking
    if F is None:
        F = re_ranking(engine.cosin_dist(qf, gf), engine.pairwise_distance_tensor(qf, qf),
                       engine.pairwise_distance_tensor(gf, gf), k1=k1, k2=k2, lambda_value=lam)
    order = engine.rank_rows(F)
    with contextlib.redirect_stdout(io.StringIO()):
        cmc_ref, map_ref = engine.rank_metrics(order, qp, gp, qc, gc)
    ref = order.long()
    for w in widths:
        for k in (1, 10, 100):
            dist, idx = engine.rerank_search(qf, gf, k, k1=k1, k2=k2, lambda_value=lam, block_cols=w)
            kk = min(k, gf.shape[0])
            assert torch.equal(idx[:, :kk], ref[:, :kk]), (w, k)
            assert torch.equal(_bits(dist[:, :kk]), _bits(torch.gather(F, 1, ref[:, :kk]))), (w, k)
        with contextlib.redirect_stdout(io.StringIO()):
            cmc, mAP = engine.rerank_metrics_streaming(qf, gf, qp, gp, qc, gc, k1=k1, k2=k2, lambda_value=lam,
                                                       block_cols=w)
        assert np.array_equal(cmc, cmc_ref) and abs(mAP - map_ref) <= 1e-12, (w, mAP, map_ref)


@pytest.mark.parametrize('case', CASES, ids=['c0', 'c1', 'c2'])
def test_search_and_metrics_equal_the_materialised_re_ranking(case):
    nq, ng, k1, k2, lam, seed = case
    qf, gf, qp, qc, gp, gc = _feats(nq, ng, seed, n_ids=40, noise=4.0)
    _check_search_and_metrics(qf, gf, qp, qc, gp, gc, k1, k2, lam, (64, None))
    # duplicated gallery rows: exact ties across block boundaries
    rep = np.arange(40)
    gf2 = torch.cat((gf, gf[rep]), 0)
    _check_search_and_metrics(qf, gf2, qp, qc, np.append(gp, gp[rep]), np.append(gc, gc[rep]), k1, k2, lam, (100,))


def test_search_and_metrics_at_mars_shape():
    qf, gf, qp, qc, gp, gc = _feats(1980, 13290, 1)
    _check_search_and_metrics(qf, gf, qp, qc, gp, gc, 20, 6, 0.3, (2048, None))


def test_beyond_one_lds_sort_network():
    """q + g = 20048 > 16384, where grl_rerank_jaccard refuses: the intermediates equal the dense kernels', and
    F equals an ordered accumulation over V2q and V2T in ascending k."""
    from grl_amd import engine
    qf, gf, qp, qc, gp, gc = _feats(48, 20000, 2, dim=768, n_ids=300)
    k1, k2, lam = 20, 6, 0.3
    m = _materialised(qf, gf, k1, k2, lam)
    rr = engine._Rerank(qf, gf, k1, k2, lam)
    _check_sparse(rr, m)
    nq, N = 48, 20048
    V2q, V2T = m['V2q'], m['V2T']
    del m['V']
    nzc = (V2q != 0).sum(1)
    L = int(nzc.max())
    kidx = torch.full((nq, L), N, dtype=torch.int64, device=DEV)        # padding: a zero row (adds +0 = no change)
    for i in range(nq):
        ks = (V2q[i] != 0).nonzero().flatten()                         # ascending k
        kidx[i, :ks.numel()] = ks
    V2Tz = torch.cat((V2T, torch.zeros((1, N), device=DEV)), 0)
    vq = torch.cat((V2q, torch.zeros((nq, 1), device=DEV)), 1)
    acc = torch.zeros((nq, N), dtype=torch.float32, device=DEV)
    for t in range(L):
        kt = kidx[:, t]
        acc = acc + torch.minimum(vq.gather(1, kt[:, None]), V2Tz[kt])
    jac = 1.0 - acc / (2.0 - acc)
    one_minus = float(np.float32(1 - lam))
    F = (jac * one_minus + m['D'][:nq] * lam)[:, nq:].contiguous()
    del acc, jac, V2Tz, vq
    blocks = engine._RerankBlocks(qf, gf, rr, block_cols=4096)
    for c0, c1 in blocks.spans:
        assert torch.equal(_bits(blocks.block(c0, c1)), _bits(F[:, c0:c1])), (c0, c1)
    del m
    _check_search_and_metrics(qf, gf, qp, qc, gp, gc, k1, k2, lam, (4096,), F=F)


def test_memory_stays_below_a_quarter_of_the_materialised_path():
    from grl_amd import engine
    from grl_amd.reid.evaluator.rerank import re_ranking
    qf, gf, qp, qc, gp, gc = _feats(1980, 13290, 1)
    with contextlib.redirect_stdout(io.StringIO()):
        engine.rerank_metrics_streaming(qf[:8], gf[:512], qp[:8], gp[:512], qc[:8], gc[:512])   # warm the allocator
    torch.cuda.synchronize()

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with contextlib.redirect_stdout(io.StringIO()):
            fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    def materialised():
        F = re_ranking(engine.cosin_dist(qf, gf), engine.pairwise_distance_tensor(qf, qf),
                       engine.pairwise_distance_tensor(gf, gf))
        engine.rank_metrics(engine.rank_rows(F), qp, gp, qc, gc)
    p_mat = peak(materialised)
    p_str = peak(lambda: engine.rerank_metrics_streaming(qf, gf, qp, gp, qc, gc))
    assert p_str < p_mat / 4, (p_str, p_mat)
    # no single allocation of nq x ng elements, let alone N x N, at the default budget and a small one
    for fn in (lambda: engine.rerank_metrics_streaming(qf, gf, qp, gp, qc, gc),
               lambda: engine.rerank_metrics_streaming(qf, gf, qp, gp, qc, gc, block_bytes=16 << 20),
               lambda: engine.rerank_search(qf, gf, 100)):
        assert _largest_allocation(fn) < 1980 * 13290 * 4


def _largest_allocation(fn):
    """Bytes of the largest device allocation fn makes (the caching allocator's trace)."""
    torch.cuda.synchronize()
    torch.cuda.memory._record_memory_history(max_entries=1000000)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            fn()
        torch.cuda.synchronize()
        snap = torch.cuda.memory._snapshot()
    finally:
        torch.cuda.memory._record_memory_history(enabled=None)
    sizes = [e['size'] for trace in snap['device_traces'] for e in trace if e['action'] == 'alloc']
    assert sizes
    return max(sizes)


def test_two_runs_are_bit_identical():
    from grl_amd import engine
    qf, gf, qp, qc, gp, gc = _feats(300, 3000, 7, n_ids=200, noise=7.0)
    a = engine.rerank_search(qf, gf, 50, block_cols=512)
    b = engine.rerank_search(qf, gf, 50, block_cols=512)
    assert torch.equal(a[1], b[1]) and torch.equal(_bits(a[0]), _bits(b[0]))
    with contextlib.redirect_stdout(io.StringIO()):
        m1 = engine.rerank_metrics_streaming(qf, gf, qp, gp, qc, gc, block_cols=512)
        m2 = engine.rerank_metrics_streaming(qf, gf, qp, gp, qc, gc, block_cols=512)
    assert np.array_equal(m1[0], m2[0]) and m1[1] == m2[1]


def test_out_of_range_arguments_raise():
    from grl_amd import engine
    qf, gf, qp, qc, gp, gc = _feats(8, 40, 1, n_ids=5)
    for kw in (dict(k1=0), dict(k1=21), dict(k2=0), dict(k2=9), dict(k1=48)):
        with pytest.raises(ValueError):
            engine.rerank_search(qf, gf, 5, **kw)
        with pytest.raises(ValueError):
            engine.rerank_metrics_streaming(qf, gf, qp, gp, qc, gc, **kw)
    for k in (0, 1025):
        with pytest.raises(ValueError):
            engine.rerank_search(qf, gf, k)
    with pytest.raises(ValueError):
        engine.rerank_metrics_streaming(qf, gf, qp[:3], gp, qc, gc)


def test_attevaluator_streaming_re_ranking_prints_and_returns_the_same(synth_models, monkeypatch, capsys):
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
    monkeypatch.delenv('GRL_EVAL_RERANK', raising=False)
    capsys.readouterr()
    r_def = ev.evaluate(None, None, [q], [g], None, False, True)
    out_def = capsys.readouterr().out
    assert 'Applying person re-ranking ...' in out_def and 'Mean AP:' in out_def
    monkeypatch.setenv('GRL_EVAL_RERANK', 'stream')
    for stream in (None, '1'):
        if stream is None:
            monkeypatch.delenv('GRL_EVAL_STREAM', raising=False)
        else:
            monkeypatch.setenv('GRL_EVAL_STREAM', stream)
        r_str = ev.evaluate(None, None, [q], [g], None, False, True)
        out_str = capsys.readouterr().out
        assert out_str == out_def and r_str == r_def, stream
    monkeypatch.delenv('GRL_EVAL_RERANK')
    with pytest.raises(ValueError, match='re-rank'):
        ev.evaluate(None, None, [q], [g], None, False, True)
