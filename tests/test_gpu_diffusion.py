"""Diffusion re-ranking on the device (engine.diffusion_graph / diffusion_solve / diffusion_search /
diffusion_metrics_streaming, diffusion.hip) and the GRL_EVAL_DIFFUSION knob of ATTEvaluator.evaluate.

The yardstick is tests/diffusion_ref.py: model (a), the kernels' arithmetic in numpy float32 with the same operation
order, to which every kernel result is held bit for bit (``.view(torch.int32)``), and (b), the dense float64 solve, which
the ranking meets under tests/ranking_check.py's rule with the tolerance recorded in diffusion_ref (4 x the model's own
measured error, never derived from the device code).  d = 32 throughout."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import diffusion_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
F32 = np.float32
RANK_SEED = 1                     # tests/test_diffusion_cpu.py checks model (a) against (b) on this fixture


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got, want, what=None):
    """got: device float32 tensor; want: host float32 array."""
    g = _bits(got).cpu().numpy()
    w = np.ascontiguousarray(want, F32).view(np.int32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError('%s: %d of %d elements differ, first at %s: got %#x, want %#x'
                             % (what, len(bad), g.size, tuple(bad[0]), int(g[tuple(bad[0])]) & 0xffffffff,
                                int(w[tuple(bad[0])]) & 0xffffffff))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _lists(gf, k):
    """engine.search(gf, gf, k + 1) as host arrays (dist, idx)."""
    from grl_amd import engine
    d, i = engine.search(gf, gf, k + 1)
    return d.cpu().numpy(), i.cpu().numpy()


# ----------------------------------------------------------------------------
# 1. grl_diffusion_mutual through the C ABI against model (a)
# ----------------------------------------------------------------------------
def _mutual_kernel(sidx, sdist, k, gamma, ldl_pad=0, ldo_pad=0):
    """The kernel on host lists with leading dimensions k + 1 + ldl_pad and k + ldo_pad; returns (idx, S, deg) after
    checking that the columns of the outputs beyond k were left alone."""
    from grl_amd import engine
    from grl_amd._lib import ptr
    n = sidx.shape[0]
    it = torch.full((n, k + 1 + ldl_pad), 0, dtype=torch.int64, device=DEV)        # (padding columns name row 0)
    dt = torch.full((n, k + 1 + ldl_pad), -1.0, dtype=torch.float32, device=DEV)
    it[:, :k + 1] = _dev(sidx[:, :k + 1])
    dt[:, :k + 1] = _dev(sdist[:, :k + 1])
    idx = torch.full((n, k + ldo_pad), 77, dtype=torch.int32, device=DEV)
    w = torch.full((n, k + ldo_pad), 1234.5, dtype=torch.float32, device=DEV)
    deg = torch.full((n + 3,), -9.0, dtype=torch.float32, device=DEV)
    engine._call('grl_diffusion_mutual', ptr(it), ptr(dt), k + 1 + ldl_pad, n, k, gamma, ptr(idx), ptr(w), k + ldo_pad,
                 ptr(deg))
    torch.cuda.synchronize()
    assert bool((idx[:, k:] == 77).all()) and bool((w[:, k:] == 1234.5).all()) and bool((deg[n:] == -9.0).all())
    return idx[:, :k], w[:, :k], deg[:n]


def _check_mutual(sidx, sdist, k, gamma, what, **pads):
    idx, S, deg = _mutual_kernel(sidx, sdist, k, gamma, **pads)
    want_idx, a, want_deg, want_S = R.mutual(sidx, sdist, k, gamma)
    assert np.array_equal(idx.cpu().numpy(), want_idx), what
    _same_bits(deg, want_deg, (what, 'deg'))
    _same_bits(S, want_S, (what, 'S'))
    return want_idx, want_S, want_deg


@pytest.mark.parametrize('n,k,gamma,pads', [(1, 1, 3, {}), (2, 1, 1, {}), (2, 3, 3, dict(ldl_pad=2, ldo_pad=1)),
                                            (5, 8, 3, dict(ldl_pad=1, ldo_pad=3)), (67, 5, 3, dict(ldo_pad=2)),
                                            (130, 64, 2, dict(ldl_pad=3)), (130, 128, 8, {})])
def test_mutual_kernel_equals_the_host_model(n, k, gamma, pads):
    gf = _dev(R.feature_case(20 + n, 1, n)[1])
    sdist, sidx = _lists(gf, k)
    assert (sidx[:, min(n, k + 1):] == -1).all()                  # n <= k: padding slots
    idx, S, deg = _check_mutual(sidx, sdist, k, gamma, (n, k), **pads)
    assert n < 3 or (S != 0).any()


def test_mutual_kernel_with_duplicate_rows_and_an_isolated_row():
    """Rows 10 .. 13 are one vector: they tie, and with k = 2 row 13 falls outside its own list (the last entry is
    dropped instead) while row 12 is its own last entry.  Row 5 has no positive similarity: it is isolated."""
    g = np.random.Generator(np.random.PCG64(3))
    x = np.abs(g.standard_normal((40, 32)))
    x[11:14] = x[10]
    x[5] = -np.abs(g.standard_normal(32))
    gf = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)
    for k in (2, 6):
        sdist, sidx = _lists(_dev(gf), k)
        if k == 2:
            assert 13 not in sidx[13] and sidx[12].tolist() == [10, 11, 12]
        assert (sdist[5, 1:] > 0).all()
        idx, S, deg = _check_mutual(sidx, sdist, k, 3, ('duplicates', k), ldl_pad=1, ldo_pad=1)
        assert deg[5] == 0 and not S[5].any() and not S[idx == 5].any()
        assert (idx[13] != 13).all()


# ----------------------------------------------------------------------------
# 2. grl_diffusion_apply and diffusion_solve against model (a)
# ----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def graphs():
    """{n: (engine graph, host idx, host S)} for n = 67 and 257 (not a multiple of the 64 rows of a partial), k = 8."""
    from grl_amd import engine
    out = {}
    for n in (67, 257):
        gf = _dev(R.feature_case(n, 1, n)[1])
        graph = engine.diffusion_graph(gf, 8, 3)
        sdist, sidx = _lists(gf, 8)
        idx, a, deg, S = R.mutual(sidx, sdist, 8, 3)
        assert np.array_equal(graph.idx.cpu().numpy(), idx)
        _same_bits(graph.weight, S, 'graph')
        _same_bits(graph.deg, deg, 'deg')
        assert graph.n_edges == int((S != 0).sum()) and graph.n_isolated == int((deg == 0).sum())
        assert (graph.n, graph.k, graph.gamma) == (n, 8, 3) and 0 < graph.n_edges < n * 8
        out[n] = (graph, gf, idx, S)
    return out


@pytest.mark.parametrize('B', [1, 3, 64, 65, 256, 260])           # 256, 260: the 16-byte path, one tile and a ragged second
@pytest.mark.parametrize('n', [67, 257])
def test_apply_kernel_and_its_fused_partials_equal_the_host_model(n, B, graphs):
    from grl_amd import _lib, engine
    from grl_amd._lib import ptr
    graph, gf, idx, S = graphs[n]
    g = np.random.Generator(np.random.PCG64(n + B))
    p = g.standard_normal((n, B)).astype(F32)
    want, want_part = R.apply(idx, S, p, F32(0.99))
    nblk = -(-n // _lib.load().grl_diffusion_part_rows())
    pd = _dev(p)
    out = torch.full((n * B + 5,), 4321.0, dtype=torch.float32, device=DEV)
    part = torch.full((nblk * B + 5,), 4321.0, dtype=torch.float32, device=DEV)
    engine._call('grl_diffusion_apply', ptr(graph.idx), ptr(graph.weight), 8, n, 8, ptr(pd), B, 0.99, ptr(out), ptr(part))
    torch.cuda.synchronize()
    assert bool((out[n * B:] == 4321.0).all()) and bool((part[nblk * B:] == 4321.0).all())
    _same_bits(out[:n * B].view(n, B), want, 'Ap')
    _same_bits(part[:nblk * B].view(nblk, B), want_part, 'partials of p . Ap')
    _same_bits(pd, p, 'p is only read')


def _seeds(graph, gf, nq, kq, gamma=3):
    """search's seed lists of the first nq rows, and their weights by the host model."""
    from grl_amd import engine
    sdist, sidx = engine.search(gf[:nq].contiguous(), gf, kq)
    val = np.array([[R.weight(v, gamma) for v in row] for row in sdist.cpu().numpy()], F32)
    return sidx, _dev(val), sidx.cpu().numpy(), val


@pytest.mark.parametrize('n,nq,n_iter', [(257, 7, 1), (257, 7, 2), (257, 7, 20), (67, 260, 3)])
def test_solve_equals_the_host_model_and_repeats_its_bits(n, nq, n_iter, graphs):
    from grl_amd import engine
    graph, gf, idx, S = graphs[n]
    qsrc = gf if nq <= n else torch.cat([gf] * 4)[:nq].contiguous()
    sdist, sidx = engine.search(qsrc[:nq].contiguous(), gf, 3)
    val = np.array([[R.weight(v, 3) for v in row] for row in sdist.cpu().numpy()], F32)
    val[3] = 0                                                     # a zero seed column: frozen from the start
    y = R.seed_vector(sidx.cpu().numpy(), val, n, 0)
    want = R.solve(idx, S, y, F32(0.99), n_iter).T
    got = engine.diffusion_solve(graph, sidx, _dev(val), 0.99, n_iter)
    assert tuple(got.shape) == (nq, n)
    _same_bits(got, want, ('solve', n_iter))
    assert not got[3].any() and bool(torch.isfinite(got).all())
    again = engine.diffusion_solve(graph, sidx, _dev(val), 0.99, n_iter)
    assert torch.equal(_bits(again), _bits(got))
    if n_iter == 20:
        _same_bits(engine.diffusion_solve(graph, sidx, _dev(val), 0.0, 5), y.T, 'alpha = 0: f = y')
        assert not engine.diffusion_solve(graph, sidx, _dev(val), 0.99, 0).any()


# ----------------------------------------------------------------------------
# 3. diffusion_search / diffusion_metrics_streaming
# ----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def case():
    qf, gf, qp, qc, gp, gc = R.feature_case(RANK_SEED, 7, 150)
    return _dev(qf), _dev(gf), (qp, gp, qc, gc)


KW = dict(k=8, kq=3, gamma=3)


def test_query_blocks_give_identical_bits_and_equal_the_ranked_full_matrix(case):
    from grl_amd import engine
    qf, gf, ids = case
    n = gf.shape[0]
    graph = engine.diffusion_graph(gf, 8, 3)
    sidx, val_dev, _, _ = _seeds(graph, gf, 7, 3)
    f = engine.diffusion_solve(graph, sidx, val_dev, 0.99, 20)
    order = engine.rank_rows(-f)
    want_metrics = engine.rank_metrics(order, *ids)
    want_idx = order[:, :40].long()
    want_score = torch.gather(-f, 1, want_idx)
    for kw in (dict(query_block=1), dict(query_block=3), dict(query_block=7), {}, dict(graph=graph),
               dict(block_bytes=20 * n * 2)):                      # the last: a default block of 2 queries
        score, idx = engine.diffusion_search(qf, gf, 40, **dict(KW, **kw))
        assert idx.dtype == torch.int64 and tuple(idx.shape) == (7, 40)
        assert torch.equal(idx, want_idx), kw
        assert torch.equal(_bits(score), _bits(want_score)), kw
        cmc, mAP = engine.diffusion_metrics_streaming(qf, gf, *ids, **dict(KW, **kw))
        assert np.array_equal(cmc, want_metrics[0]) and mAP == want_metrics[1], kw
    # padding as search pads, and the empty shapes
    score, idx = engine.diffusion_search(qf, gf[:20].contiguous(), 30, k=4, kq=2)
    assert bool((idx[:, 20:] == -1).all()) and bool(torch.isinf(score[:, 20:]).all()) and bool((idx[:, :20] >= 0).all())
    score, idx = engine.diffusion_search(qf[:0], gf, 5, **KW)
    assert tuple(score.shape) == (0, 5) and tuple(idx.shape) == (0, 5)
    score, idx = engine.diffusion_search(qf, gf[:0], 5, **KW)
    assert tuple(idx.shape) == (7, 5) and bool((idx == -1).all())
    g0 = engine.diffusion_graph(gf[:0], 8)
    assert (g0.n, g0.n_edges, g0.n_isolated) == (0, 0, 0) and tuple(g0.idx.shape) == (0, 8)


def test_exclude_equals_deleting_the_junk_from_the_unfiltered_ranking(case):
    from grl_amd import engine
    qf, gf, ids = case
    qp, gp, qc, gc = ids
    n = gf.shape[0]
    _, full = engine.diffusion_search(qf, gf, n, **KW)
    score, idx = engine.diffusion_search(qf, gf, 25, exclude=ids, query_block=3, **KW)
    full, idx = full.cpu().numpy(), idx.cpu().numpy()
    dropped = 0
    for q in range(7):
        keep = [g for g in full[q] if not (gp[g] == qp[q] and gc[g] == qc[q])]
        dropped += n - len(keep)
        assert idx[q].tolist() == keep[:25], q
    assert dropped >= 7                                            # every query is its own junk entry at least


def test_ranking_meets_the_float64_yardstick(case):
    """tests/ranking_check.py's rule against the dense float64 solve (b) on the device's own lists: positions may differ
    only between entries whose (b) scores are closer than the recorded tolerance, and in at most 1 % of the positions."""
    from grl_amd import engine
    qf, gf, ids = case
    n = gf.shape[0]
    sdist, sidx = _lists(gf, 8)
    qd, qi = engine.search(qf, gf, 3)
    for alpha, n_iter in ((0.99, 150), (0.9, 60)):
        idx64, a, deg, S64 = R.mutual(sidx, sdist, 8, 3, np.float64)
        y = R.seed_vector(qi.cpu().numpy(), qd.cpu().numpy(), n, 3, np.float64)
        ref = R.dense_solve(idx64, S64, y, alpha).T
        score, idx = engine.diffusion_search(qf, gf, n, alpha=alpha, n_iter=n_iter, **KW)
        err = R.relative_error(-score.cpu().numpy(), np.take_along_axis(ref, idx.cpu().numpy(), 1))
        n_diff, gap = R.ranking_differences(idx.cpu().numpy(), R.rank(ref), ref, R.tolerance(alpha))
        print('alpha = %g: error of f %.3e (tolerance %.3e); %d of %d positions differ, largest gap %.3e'
              % (alpha, err, R.tolerance(alpha), n_diff, ref.size, gap))
        assert err <= R.tolerance(alpha)
        assert gap <= R.tolerance(alpha) and n_diff <= 0.01 * ref.size


def test_manifold_case_ranks_every_match_above_every_distractor():
    from grl_amd import engine
    qf, gf, qp, qc, gp, gc, matches, distractors = R.manifold_case()
    qd, gd = _dev(qf), _dev(gf)
    n = gf.shape[0]
    plain = engine.search(qd, gd, n)[1][0].cpu().tolist()
    assert max(plain.index(d) for d in distractors) < min(plain.index(m) for m in matches)     # cosine fails
    score, idx = engine.diffusion_search(qd, gd, n, k=4, kq=3)
    order = idx[0].cpu().tolist()
    assert max(order.index(m) for m in matches) < min(order.index(d) for d in distractors)
    _, idx = engine.diffusion_search(qd, gd, 3, k=4, kq=3, exclude=(qp, gp, qc, gc))
    assert sorted(idx[0].cpu().tolist()) == sorted(int(m) for m in matches)
    cmc, mAP = engine.diffusion_metrics_streaming(qd, gd, qp, gp, qc, gc, k=4, kq=3)
    assert cmc[0] == 1.0 and mAP == 1.0
    assert engine.rank_metrics_streaming(qd, gd, qp, gp, qc, gc)[1] < 0.5


def test_alpha_zero_ranks_the_seeds_first_in_their_order(case):
    from grl_amd import engine
    qf, gf, ids = case
    sdist, sidx = engine.search(qf, gf, 3)
    score, idx = engine.diffusion_search(qf, gf, 5, alpha=0.0, **KW)
    w = np.array([[R.weight(v, 3) for v in row] for row in sdist.cpu().numpy()], F32)
    si = sidx.cpu().numpy()
    for q in range(7):
        want = [int(si[q, t]) for t in np.lexsort((si[q], -w[q]))]        # by weight, ties to the smaller index
        assert idx[q, :3].cpu().tolist() == want
        assert want == si[q].tolist() or len(set(w[q].tolist())) < 3       # search's order, unless two weights tie
    _same_bits(-score[:, :3], np.sort(w, axis=1)[:, ::-1], 'f = y at the seeds')
    assert not score[:, 3:].any()
    # n_iter = 0: f = 0, the ranking is the index order
    assert engine.diffusion_search(qf, gf, 5, n_iter=0, **KW)[1].cpu().tolist() == [list(range(5))] * 7


def test_refused_arguments(case):
    from grl_amd import engine
    qf, gf, ids = case
    graph = engine.diffusion_graph(gf, 8)
    vm = engine.VerifyMetric.__new__(engine.VerifyMetric)
    for bad in (dict(k=0), dict(k=129), dict(k=2.0), dict(kq=0), dict(kq=9, k=8), dict(kq=9, graph=graph), dict(gamma=0),
                dict(gamma=9), dict(alpha=1.0), dict(alpha=-0.5), dict(alpha=float('nan')), dict(n_iter=-1),
                dict(n_iter=1.5), dict(query_block=0), dict(graph='graph'),
                dict(graph=engine.diffusion_graph(gf[:50].contiguous(), 8))):
        with pytest.raises(ValueError):
            engine.diffusion_search(qf, gf, 5, **bad)
        with pytest.raises(ValueError):
            engine.diffusion_metrics_streaming(qf, gf, *ids, **bad)
    for k_out in (0, 1025):
        with pytest.raises(ValueError):
            engine.diffusion_search(qf, gf, k_out)
    for bad in (dict(metric=vm), dict(metric='euclidean'), dict(k=0), dict(gamma=9)):
        with pytest.raises(ValueError):
            engine.diffusion_graph(gf, **dict(dict(k=8), **bad))
    with pytest.raises(ValueError, match='HIP device'):
        engine.diffusion_search(qf.cpu(), gf, 5)
    with pytest.raises(ValueError, match='HIP device'):
        engine.diffusion_graph(gf.cpu())
    sidx, val, _, _ = _seeds(graph, gf, 4, 3)
    for fn in (lambda: engine.diffusion_solve(graph, sidx.int(), val), lambda: engine.diffusion_solve(graph, sidx, val[:, :2]),
               lambda: engine.diffusion_solve(graph, sidx.cpu(), val.cpu()), lambda: engine.diffusion_solve(graph, sidx, val, 1.0),
               lambda: engine.diffusion_solve(graph, sidx, val, 0.5, -1)):
        with pytest.raises(ValueError):
            fn()


def test_memory_stays_below_the_query_x_gallery_matrix_plus_the_graph():
    from grl_amd import engine
    n, nq, d, k = 2048, 512, 32, 50
    g = torch.Generator(device=DEV).manual_seed(5)
    gf = torch.randn((n, d), device=DEV, generator=g)
    gf /= gf.norm(dim=1, keepdim=True)
    qf = gf[:nq].clone()
    engine.diffusion_search(qf[:8], gf[:256].contiguous(), 10, query_block=4)          # warm the allocator
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    score, idx = engine.diffusion_search(qf, gf, 10, query_block=64, block_bytes=1 << 20)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    matrix, graph = nq * n * 4, n * k * 8 + n * 4
    print('peak above the inputs: %d bytes; the %d x %d matrix: %d bytes, the graph: %d bytes' % (peak, nq, n, matrix, graph))
    assert peak < matrix + graph, (peak, matrix, graph)
    assert bool((idx[:, 0] >= 0).all())


# ----------------------------------------------------------------------------
# 4. ATTEvaluator.evaluate with GRL_EVAL_DIFFUSION
# ----------------------------------------------------------------------------
KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_DIFFUSION')
KEEP = ('Mean AP', 'Rank-')


@pytest.fixture(scope='module')
def eval_case(synth_models):
    from grl_amd.reid.evaluator import ATTEvaluator
    from grl_amd.synthetic import synth_clips
    cnn, siam, _ = synth_models
    cnn, siam = cnn.to(DEV).eval(), siam.to(DEV).eval()
    g = np.random.Generator(np.random.PCG64(21))
    nq, ng = 6, 23
    gp, gc = g.integers(0, 5, ng), g.integers(0, 3, ng)
    qp, qc = gp[:nq].copy(), (gc[:nq] + 1) % 3                       # every query has its pid in the gallery
    q = [(synth_clips(nq, 2, seed=31), torch.from_numpy(qp), torch.from_numpy(qc))]
    gl = [(synth_clips(ng, 2, seed=32), torch.from_numpy(gp), torch.from_numpy(gc))]
    ev = ATTEvaluator(cnn, siam, only_eval=False)
    with contextlib.redirect_stdout(io.StringIO()):
        qf, qp2, qc2 = ev.extract_feature(q)
        gf, gp2, gc2 = ev.extract_feature(gl)
    gf, gp2, gc2 = torch.cat((qf, gf), 0), np.append(qp2, gp2), np.append(qc2, gc2)
    return ev, q, gl, qf, gf, (qp2, gp2, qc2, gc2)


def _lines(text):
    return [l for l in text.splitlines() if l.startswith(KEEP)]


@pytest.mark.parametrize('stream', [None, '1'])
def test_attevaluator_knob_ranks_by_diffusion(stream, eval_case, monkeypatch, tmp_path):
    from grl_amd import engine
    from grl_amd.reid.evaluator.attevaluator import _report, evaluate_seq
    ev, q, gl, qf, gf, ids = eval_case
    path = str(tmp_path) + os.sep
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    if stream:
        monkeypatch.setenv('GRL_EVAL_STREAM', stream)
    # unset: the default route, unchanged
    with contextlib.redirect_stdout(io.StringIO()) as o0:
        r0 = ev.evaluate(None, None, q, gl, path, 0, 0)
    with contextlib.redirect_stdout(io.StringIO()) as ob:
        if stream:
            rb = _report(*engine.rank_metrics_streaming(qf, gf, *ids))
        else:
            rb = evaluate_seq(None, ids[0], ids[2], ids[1], ids[3], '', indices=engine.rank_rows(engine.cosin_dist(qf, gf)))
    assert r0 == rb and _lines(o0.getvalue()) == _lines(ob.getvalue())
    assert 'Diffusion' not in o0.getvalue() and not os.path.exists(path + 'diffusion.json')
    # set
    monkeypatch.setenv('GRL_EVAL_DIFFUSION', '5,3,0.9,10')
    with contextlib.redirect_stdout(io.StringIO()) as o1:
        r1 = ev.evaluate(None, None, q, gl, path, 0, 0)
    graph = engine.diffusion_graph(gf, 5)
    with contextlib.redirect_stdout(io.StringIO()) as ow:
        rw = _report(*engine.diffusion_metrics_streaming(qf, gf, *ids, k=5, kq=3, alpha=0.9, n_iter=10))
    text = o1.getvalue()
    assert r1 == rw and _lines(text) == _lines(ow.getvalue()) and len(_lines(text)) == 5
    line = 'Diffusion: k = 5, kq = 3, alpha = 0.9, n_iter = 10, gamma = 3: %d edges, %d isolated of %d' % (
        graph.n_edges, graph.n_isolated, graph.n)
    assert line in text and text.index(line) < text.index('Mean AP')
    js = json.load(open(path + 'diffusion.json'))
    assert js == {'k': 5, 'kq': 3, 'alpha': 0.9, 'n_iter': 10, 'gamma': 3, 'metric': 'cosine', 'n': graph.n,
                  'n_edges': graph.n_edges, 'n_isolated': graph.n_isolated}
    # refused combinations
    # (under GRL_EVAL_STREAM=1 the evaluator's older refusal of rerank=1 comes first)
    with pytest.raises(ValueError, match='GRL_EVAL_STREAM=1 cannot re-rank' if stream else 'GRL_EVAL_DIFFUSION cannot re-rank'):
        ev.evaluate(None, None, q, gl, path, 0, 1)
    monkeypatch.setenv('GRL_EVAL_METRIC', 'verify')
    with pytest.raises(ValueError, match='GRL_EVAL_DIFFUSION cannot be combined with GRL_EVAL_METRIC'):
        ev.evaluate(None, None, q, gl, path, 0, 0)


def test_attevaluator_visual_takes_its_lists_from_diffusion_search(synth_models, tmp_path, monkeypatch):
    import visual_tree as V
    from grl_amd import engine
    from grl_amd.reid.evaluator import ATTEvaluator
    from grl_amd.synthetic import synth_clips
    monkeypatch.chdir(tmp_path)
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv('GRL_VISUAL_QUERIES', '1,4')
    monkeypatch.setenv('GRL_EVAL_DIFFUSION', '5,3,0.9,10')
    query, gallery = V.make_tree('frames')['video']
    cnn, siam, _ = synth_models
    cnn, siam = cnn.to(DEV).eval(), siam.to(DEV).eval()

    def loader(items, seed):
        return [(synth_clips(len(items), 2, seed=seed), torch.tensor([i[1] for i in items]),
                 torch.tensor([i[2] for i in items]))]
    q, g = loader(query, 31), loader(gallery, 32)
    ev = ATTEvaluator(cnn, siam, only_eval=False)
    with contextlib.redirect_stdout(io.StringIO()) as o0:
        r0 = ev.evaluate(query, gallery, q, g, 'plain_', 0, 0)
    with contextlib.redirect_stdout(io.StringIO()) as o1:
        r1 = ev.evaluate(query, gallery, q, g, 'run_', 1, 0)
    assert r1 == r0 and not os.path.exists('plain_visual') and _lines(o1.getvalue()) == _lines(o0.getvalue())
    with contextlib.redirect_stdout(io.StringIO()):
        qf, qp, qc = ev.extract_feature(q)
        gf, gp, gc = ev.extract_feature(g)
    gf, gp, gc = torch.cat((qf, gf), 0), np.append(qp, gp), np.append(qc, gc)
    score, idx = engine.diffusion_search(qf, gf, 10, k=5, kq=3, alpha=0.9, n_iter=10, exclude=(qp, gp, qc, gc))
    score, idx = score.cpu().numpy(), idx.cpu().numpy()
    ranked = json.load(open('run_visual/ranked.json'))
    assert sorted(ranked) == ['1', '4']
    for qi in (1, 4):
        rows = ranked[str(qi)]
        keep = idx[qi] >= 0
        assert [r[0] for r in rows] == [int(x) for x in idx[qi][keep]]
        assert [np.float32(r[3]).view(np.int32) for r in rows] == list(score[qi][keep].view(np.int32))
        assert all(r[1] == gp[r[0]] and r[2] == gc[r[0]] for r in rows) and qi not in idx[qi]
