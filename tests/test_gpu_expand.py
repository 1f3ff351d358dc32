"""Query expansion / database-side augmentation on the device: grl_expand_rows through the C ABI,
engine.expand_from_lists / engine.expand_features in one process and over gloo ranks, and the GRL_EVAL_QE /
GRL_EVAL_DBA knobs of ATTEvaluator.evaluate.

The yardstick is tests/expand_ref.py, the kernel's arithmetic in numpy float32 with the same operation order.  Every
comparison is bit-equal (``.view(torch.int32)``); nothing here has a tolerance."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import expand_ref as E
from grl_amd.synthetic import synth_eval_features

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda:0')
F32 = np.float32


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got, want, what=None):
    """got: device float32 tensor; want: host float32 array."""
    g = _bits(got).cpu().numpy()
    w = np.ascontiguousarray(want).view(np.int32)
    assert g.shape == w.shape, what
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError('%s: %d of %d elements differ, first at %s: got %#x, want %#x'
                             % (what, len(bad), g.size, tuple(bad[0]), g[tuple(bad[0])] & 0xffffffff,
                                w[tuple(bad[0])] & 0xffffffff))


# ----------------------------------------------------------------------------
# 1. the kernel through the C ABI against the host model
# ----------------------------------------------------------------------------
def _padded(a, ld, fill):
    """Device buffer [rows][ld] holding a [rows][d] host array in its first d columns."""
    t = torch.full((a.shape[0], ld), fill, dtype=torch.float32, device=DEV)
    t[:, :a.shape[1]] = torch.from_numpy(a).to(DEV)
    return t


def _kernel(x, bank, idx, dist, m, alpha, skip_self, pads=(0, 0, 0), ldl_pad=0):
    """grl_expand_rows on host arrays with leading dimensions d + pads (x, bank, out) and L + ldl_pad; returns the
    [n, d] result after checking that the columns of out beyond d were left alone."""
    from grl_amd import engine
    from grl_amd._lib import ptr
    n, d = x.shape
    L = idx.shape[1]
    xd, bd = _padded(x, d + pads[0], 7.5), _padded(bank, d + pads[1], -3.25)
    out = torch.full((n, d + pads[2]), 1234.5, dtype=torch.float32, device=DEV)
    it = torch.full((n, L + ldl_pad), 0, dtype=torch.int64, device=DEV)
    dt = torch.full((n, L + ldl_pad), -1.0, dtype=torch.float32, device=DEV)
    it[:, :L] = torch.from_numpy(idx).to(DEV)
    dt[:, :L] = torch.from_numpy(dist).to(DEV)
    engine._call('grl_expand_rows', ptr(xd), d + pads[0], ptr(bd), d + pads[1], ptr(it), ptr(dt), L + ldl_pad, n,
                 bank.shape[0], d, L, m, alpha, 1 if skip_self else 0, ptr(out), d + pads[2])
    torch.cuda.synchronize()
    assert bool((out[:, d:] == 1234.5).all())
    return out[:, :d]


def _lists(seed, n, nb, d, L):
    """Rows of nb == n features and lists that hold: repeated neighbours, padding anywhere, the self entry first
    (row % 4 == 0), in the middle (1), absent (2) and last (3), positive distances (negative similarity: weight 0),
    a NaN, a +inf and a -inf distance, lists of padding only and short lists, a NaN in x and a NaN in the bank."""
    g = np.random.Generator(np.random.PCG64(seed))
    x = g.standard_normal((n, d)).astype(F32)
    bank = x.copy() if n == nb else g.standard_normal((nb, d)).astype(F32)
    idx = g.integers(0, nb, (n, L)).astype(np.int64)
    rows = np.arange(n)[:, None]
    idx[idx == rows] = (idx[idx == rows] + 1) % nb                 # no accidental self entry
    idx[g.random((n, L)) < 0.1] = -1
    dist = -g.random((n, L)).astype(F32)
    pos = g.random((n, L)) < 0.15
    dist[pos] = g.random(int(pos.sum())).astype(F32)
    for i in range(n):
        where = {0: 0, 1: L // 2, 3: L - 1}.get(i % 4)
        if where is not None:
            idx[i, where] = i
    idx[6 % n, :] = -1                                             # nothing to expand with
    idx[9 % n, 2:] = -1                                            # a short list
    dist[3 % n, 0] = np.nan
    dist[4 % n, 0] = np.inf
    dist[7 % n, L // 3] = -np.inf
    idx[7 % n, L // 3] = (7 % n + 1) % nb                          # (kept: the row becomes inf / inf)
    x[5 % n, 0] = np.nan
    bank[2, d - 1] = np.nan
    if n == nb:
        x[2, d - 1] = np.nan
    idx[1 % n, 1 % L] = 2                                          # the NaN bank row is a neighbour of row 1
    return x, bank, idx, dist


PADS = {0: (0, 0, 0), 1: (4, 8, 12), 3: (1, 3, 5), 8: (8, 0, 4)}     # by alpha: aligned, aligned, unaligned, aligned


@pytest.mark.parametrize('m', [1, 5, 10, 64, 1023])
@pytest.mark.parametrize('d', [6144, 2048, 257, 5])
def test_kernel_equals_the_host_model(d, m):
    n = nb = 40
    L = m + 5
    x, bank, idx, dist = _lists(100 + d + m, n, nb, d, L)
    saw_nan = False
    for alpha in (0, 1, 3, 8):
        for skip_self in (False, True):
            want = E.expand_rows(x, bank, idx, dist, m, alpha, skip_self)
            got = _kernel(x, bank, idx, dist, m, alpha, skip_self, PADS[alpha], ldl_pad=alpha % 3)
            _same_bits(got, want, (d, m, alpha, skip_self))
            saw_nan = saw_nan or bool(np.isnan(want[5]).any())
    assert saw_nan                                                  # the NaN feature reached the output
    # m == L: the whole list
    want = E.expand_rows(x, bank, idx, dist, L, 1, True)
    _same_bits(_kernel(x, bank, idx, dist, L, 1, True), want, (d, 'm == L'))


def test_kernel_with_a_bank_of_its_own_and_special_rows():
    """n != nb (query expansion): no self entry; the special rows behave as the contract says."""
    n, nb, d, L = 23, 300, 1030, 16
    x, bank, idx, dist = _lists(5, n, nb, d, L)
    for alpha in (0, 2, 3):
        want = E.expand_rows(x, bank, idx, dist, 10, alpha)
        _same_bits(_kernel(x, bank, idx, dist, 10, alpha, False, (0, 0, 0)), want, alpha)
        _same_bits(_kernel(x, bank, idx, dist, 10, alpha, False, (2, 2, 2)), want, alpha)
        assert np.array_equal(want[6].view(np.int32), x[6].view(np.int32))          # padding only: the row itself
        assert np.isnan(want[5, 0]) and not np.isnan(want[5, 1:]).any()             # a NaN of x stays in its column
        assert np.isnan(want[1, d - 1])                                             # a NaN of the bank reaches row 1
        if alpha:
            assert (want[7].view(np.uint32) == 0x7fc00000).all()                     # -inf distance: inf / inf
    # positive distances only, alpha > 0: every weight is 0 and x comes back (x + 0 * bank, / 1)
    ok = ~np.isnan(bank).any(1)
    idx2 = np.where(ok[np.maximum(idx, 0)] & (idx >= 0), idx, -1)
    got = _kernel(x, bank, idx2, np.abs(dist) + F32(0.5), 10, 3, False)
    _same_bits(got, E.expand_rows(x, bank, idx2, np.abs(dist) + F32(0.5), 10, 3), 'weights 0')
    keep = ~np.isnan(x).any(1)
    assert np.array_equal(got.cpu().numpy()[keep], x[keep] + F32(0.0))


# ----------------------------------------------------------------------------
# 2. engine.expand_features against the model applied to engine.search's own lists
# ----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small():
    return synth_eval_features(40, 400, seed=1, n_ids=24, noise=7.0)


def _check_features(xf, bank, m, alpha=0, metric='cosine', exclude=None, skip_self=False, **kw):
    from grl_amd import engine
    got = engine.expand_features(xf, bank, m, alpha, metric=metric, exclude=exclude, skip_self=skip_self, **kw)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == tuple(xf.shape)
    assert got.data_ptr() not in (xf.data_ptr(), bank.data_ptr())
    dist, idx = engine.search(xf, bank, m + (1 if skip_self else 0), metric=metric, exclude=exclude, **kw)
    want = E.expand_rows(xf.cpu().numpy(), bank.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy(), m, alpha,
                         skip_self)
    _same_bits(got, want, (m, alpha, metric, skip_self, kw))
    again = engine.expand_from_lists(xf, bank, dist, idx, m, alpha, skip_self)
    assert torch.equal(_bits(again), _bits(got))
    return want, idx.cpu().numpy()


def test_expand_features_equals_the_model_on_the_search_lists(small):
    qf, gf, qp, qc, gp, gc = small
    qf, gf = qf.to(DEV), gf.to(DEV)
    ids = (qp, gp, qc, gc)
    base_q, base_g = qf.clone(), gf.clone()
    for kw in ({}, dict(block_cols=7), dict(block_cols=64), dict(block_cols=256), dict(block_cols=150),
               dict(block_bytes=40 * 4 * 256)):                            # ragged last blocks: 400 = 57 * 7 + 1, ...
        for m, alpha in ((1, 0), (10, 0), (10, 3), (5, 8)):
            _check_features(qf, gf, m, alpha, **kw)
            want, idx = _check_features(qf, gf, m, alpha, exclude=ids, **kw)
            assert (idx[:, 0] != np.arange(40)).all()                      # junk rule: never the prepended query itself
        _check_features(qf, gf, 10, 0, metric='euclidean', **kw)
        _check_features(qf, gf, 10, 0, metric='euclidean', exclude=ids, **kw)
        for m, alpha in ((1, 1), (10, 3)):
            want, idx = _check_features(gf, gf, m, alpha, skip_self=True, **kw)     # DBA: xf IS bank
            assert idx.shape[1] == m + 1 and (idx[:, 0] == np.arange(400)).mean() > 0.9
    _check_features(gf, gf, 3, 0, metric='euclidean', skip_self=True)
    _check_features(qf, gf, 1023, 1)                                         # the longest list: padding past 400
    _check_features(gf, gf, 1023, 1, skip_self=True)
    assert torch.equal(_bits(qf), _bits(base_q)) and torch.equal(_bits(gf), _bits(base_g))   # inputs only read
    # without exclude the prepended query is its own first neighbour, and with alpha = 0, m = 1 the mean of two copies
    got = _check_features(qf, gf, 1, 0)[0]
    assert np.array_equal(got, ((qf.cpu().numpy() * 2) / F32(2.0)))


def test_expand_features_at_other_feature_sizes():
    """(the search GEMM takes feature sizes that are multiples of 32; any d is the kernel's own contract, above)"""
    for dim, nq, ng in ((96, 12, 150), (1056, 9, 64)):
        qf, gf, qp, qc, gp, gc = synth_eval_features(nq, ng, seed=4, dim=dim, n_ids=8, noise=3.0)
        qf, gf = qf.to(DEV), gf.to(DEV)
        _check_features(qf, gf, 7, 2, exclude=(qp, gp, qc, gc), block_cols=33)
        _check_features(gf, gf, 7, 2, skip_self=True, block_cols=33)


# ----------------------------------------------------------------------------
# 3. refusals
# ----------------------------------------------------------------------------
def test_overlapping_out_and_bad_ranges_are_refused():
    from grl_amd import _lib, engine
    from grl_amd._lib import ptr
    lib = _lib.load()
    n, d, L = 8, 64, 6
    buf = torch.zeros((3 * n, d), device=DEV)
    x, bank, out = buf[:n], buf[n:2 * n], buf[2 * n:]
    idx = torch.zeros((n, L), dtype=torch.int64, device=DEV)
    dist = torch.zeros((n, L), device=DEV)

    def rc(o, m=2, alpha=0, skip=0, ldo=d):
        return lib.grl_expand_rows(ptr(x), d, ptr(bank), d, ptr(idx), ptr(dist), L, n, n, d, L, m, alpha, skip,
                                   o, ldo, _lib.stream())
    assert rc(ptr(out)) == 0
    for o in (ptr(x), ptr(bank), ptr(x) + 4 * (n * d - 1), ptr(bank) + 4 * d * 3, ptr(x) - 4 * (n * d - 1)):
        assert rc(o) == _lib.GRL_EINVAL
        assert b'overlaps' in lib.grl_last_error()
    assert rc(ptr(out), m=0) == _lib.GRL_EINVAL and rc(ptr(out), m=L + 1) == _lib.GRL_EINVAL
    assert rc(ptr(out), alpha=-1) == _lib.GRL_EINVAL and rc(ptr(out), alpha=9) == _lib.GRL_EINVAL
    assert rc(ptr(out), ldo=d - 1) == _lib.GRL_EINVAL
    torch.cuda.synchronize()
    with pytest.raises(_lib.GrlHipError, match='overlaps'):
        engine._call('grl_expand_rows', ptr(x), d, ptr(bank), d, ptr(idx), ptr(dist), L, n, n, d, L, 2, 0, 0, ptr(bank), d)
    qf = torch.zeros((4, 32), device=DEV)                     # (the search GEMM takes feature sizes that are multiples of 32)
    gf = torch.zeros((9, 32), device=DEV)
    for bad in (dict(m=0), dict(m=1024), dict(m=3, alpha=9), dict(m=3, alpha=-1), dict(m=3, alpha=1, metric='euclidean'),
                dict(m=3, skip_self=True), dict(m=3, metric='l2')):
        with pytest.raises(ValueError):
            engine.expand_features(qf, gf, **bad)
    d5, i5 = engine.search(qf, gf, 5)
    for bad in (dict(m=6), dict(m=0), dict(m=2, alpha=9), dict(m=2, skip_self=True)):
        with pytest.raises(ValueError):
            engine.expand_from_lists(qf, gf, d5, i5, **bad)
    with pytest.raises(_lib.GrlHipError):
        engine.expand_from_lists(qf, gf, d5, i5.int(), 2)
    with pytest.raises(ValueError):
        engine.expand_from_lists(qf, gf, d5[:, :4], i5, 2)


# ----------------------------------------------------------------------------
# 4. reproducibility, and a world of two gloo ranks on one device
# ----------------------------------------------------------------------------
DIST_CASES = ('qe', 'qe_alpha', 'qe_euclid', 'dba', 'dba_then_qe')


def _run_dist_cases():
    from grl_amd import engine
    qf, gf, qp, qc, gp, gc = synth_eval_features(40, 400, seed=1, n_ids=24, noise=7.0)
    qf, gf = qf.to(DEV), gf.to(DEV)
    ids = (qp, gp, qc, gc)
    out = {}
    out['qe'] = engine.expand_features(qf, gf, 10, 0, exclude=ids, block_cols=64)
    out['qe_alpha'] = engine.expand_features(qf, gf, 10, 3, exclude=ids)
    out['qe_euclid'] = engine.expand_features(qf, gf, 5, 0, metric='euclidean', block_cols=33)
    out['dba'] = engine.expand_features(gf, gf, 10, 3, skip_self=True, block_cols=64)
    out['dba_then_qe'] = engine.expand_features(qf, out['dba'], 10, 3, exclude=ids)
    return {k: _bits(v).cpu() for k, v in out.items()}


def _worker(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.save(_run_dist_cases(), os.path.join(outdir, 'rank%d.pt' % rank))
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


def test_two_runs_are_bit_identical_and_two_ranks_return_the_single_process_tensor(tmp_path_factory):
    a, b = _run_dist_cases(), _run_dist_cases()
    assert sorted(a) == sorted(DIST_CASES)
    for k in DIST_CASES:
        assert torch.equal(a[k], b[k]), k
    outdir = str(tmp_path_factory.mktemp('expand_w2'))
    mp.spawn(_worker, args=(2, 43300 + os.getpid() % 1500, outdir), nprocs=2, join=True)
    for r in range(2):
        res = torch.load(os.path.join(outdir, 'rank%d.pt' % r), weights_only=False)
        assert sorted(res) == sorted(DIST_CASES)
        for k in DIST_CASES:
            assert torch.equal(res[k], a[k]), (k, 'rank', r)


# ----------------------------------------------------------------------------
# 5. memory
# ----------------------------------------------------------------------------
def test_memory_stays_below_a_quarter_of_the_matrix_the_path_avoids():
    from grl_amd import engine
    n, nb, d, m = 4096, 262144, 64, 10
    g = torch.Generator(device=DEV).manual_seed(11)
    bank = torch.randn((nb, d), device=DEV, generator=g)
    bank /= bank.norm(dim=1, keepdim=True)
    xf = bank[:n].clone()
    engine.expand_features(xf[:8], bank[:512], m)                          # warm the allocator
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = engine.expand_features(xf, bank, m, 3)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    matrix = n * nb * 4
    print('peak above the inputs: %d bytes; the %d x %d matrix: %d bytes' % (peak, n, nb, matrix))
    assert matrix > 4.29e9 and peak < matrix / 4, (peak, matrix)
    # and the result is the model's on a sample of rows (each row depends on its own list only)
    dist, idx = engine.search(xf, bank, m)
    rows = np.arange(0, n, 97)
    want = E.expand_rows(xf.cpu().numpy()[rows], bank.cpu().numpy(), idx.cpu().numpy()[rows], dist.cpu().numpy()[rows],
                         m, 3)
    _same_bits(out[torch.from_numpy(rows).to(DEV)], want, 'large bank')


# ----------------------------------------------------------------------------
# 6. ATTEvaluator.evaluate with GRL_EVAL_QE / GRL_EVAL_DBA
# ----------------------------------------------------------------------------
KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA')
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


def _downstream(qf, gf, ids, rerank):
    """What the evaluator does with a pair of feature tensors when no knob is set (materialised path): returns
    (Rank-1, the printed Mean AP / Rank-k lines)."""
    from grl_amd import engine
    from grl_amd.reid.evaluator.attevaluator import evaluate_seq
    from grl_amd.reid.evaluator.rerank import re_ranking
    qp, gp, qc, gc = ids
    D = engine.cosin_dist(qf, gf)
    with contextlib.redirect_stdout(io.StringIO()) as o:
        if rerank:
            D = re_ranking(D, engine.pairwise_distance_tensor(qf, qf), engine.pairwise_distance_tensor(gf, gf))
        r1 = evaluate_seq(None, qp, qc, gp, gc, '', indices=engine.rank_rows(D))
    return r1, [l for l in o.getvalue().splitlines() if l.startswith(KEEP)]


def _model_expand(xf, bank, m, alpha, exclude=None, skip_self=False):
    from grl_amd import engine
    dist, idx = engine.search(xf, bank, m + (1 if skip_self else 0), exclude=exclude)
    out = E.expand_rows(xf.cpu().numpy(), bank.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy(), m, alpha, skip_self)
    return torch.from_numpy(out).to(DEV)


@pytest.mark.parametrize('rerank', [0, 1])
@pytest.mark.parametrize('qe,dba', [('3,2', None), (None, '2,1'), ('3,2', '2,1'), ('4', '3')])
def test_attevaluator_knobs_give_the_metrics_of_the_model_expanded_features(qe, dba, rerank, eval_case, monkeypatch):
    from grl_amd.reid.evaluator.attevaluator import parse_expand_knob
    ev, q, gl, qf, gf, ids = eval_case
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    with contextlib.redirect_stdout(io.StringIO()) as o0:
        r0 = ev.evaluate(None, None, q, gl, '', 0, rerank)
    base = _downstream(qf, gf, ids, rerank)                          # the helper IS the evaluator without knobs
    assert r0 == base[0] and [l for l in o0.getvalue().splitlines() if l.startswith(KEEP)] == base[1]
    assert 'expansion' not in o0.getvalue() and 'augmentation' not in o0.getvalue()
    qf2, gf2 = qf, gf
    if dba:
        monkeypatch.setenv('GRL_EVAL_DBA', dba)
        gf2 = _model_expand(gf, gf, *parse_expand_knob('GRL_EVAL_DBA', dba), skip_self=True)
    if qe:
        monkeypatch.setenv('GRL_EVAL_QE', qe)
        qf2 = _model_expand(qf, gf2, *parse_expand_knob('GRL_EVAL_QE', qe), exclude=ids)
    want = _downstream(qf2, gf2, ids, rerank)
    with contextlib.redirect_stdout(io.StringIO()) as o1:
        r1 = ev.evaluate(None, None, q, gl, '', 0, rerank)
    text = o1.getvalue()
    assert r1 == want[0] and [l for l in text.splitlines() if l.startswith(KEEP)] == want[1]
    if dba:
        m, a = parse_expand_knob('GRL_EVAL_DBA', dba)
        assert 'Database-side augmentation: m = %d, alpha = %d' % (m, a) in text
    if qe:
        m, a = parse_expand_knob('GRL_EVAL_QE', qe)
        assert 'Query expansion: m = %d, alpha = %d' % (m, a) in text
    assert ('augmentation' in text) == bool(dba) and ('expansion' in text) == bool(qe)


def test_attevaluator_knobs_reach_the_streaming_paths(eval_case, monkeypatch):
    ev, q, gl, qf, gf, ids = eval_case
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv('GRL_EVAL_DBA', '2,1')
    monkeypatch.setenv('GRL_EVAL_QE', '3,2')
    gf2 = _model_expand(gf, gf, 2, 1, skip_self=True)
    qf2 = _model_expand(qf, gf2, 3, 2, exclude=ids)
    want = _downstream(qf2, gf2, ids, 0)
    monkeypatch.setenv('GRL_EVAL_STREAM', '1')
    with contextlib.redirect_stdout(io.StringIO()) as o:
        r = ev.evaluate(None, None, q, gl, '', 0, 0)
    assert r == want[0] and [l for l in o.getvalue().splitlines() if l.startswith(KEEP)] == want[1]


def test_unset_knobs_make_no_expansion_call_and_set_knobs_only_insert_theirs(eval_case, monkeypatch):
    """Through engine._call: with both knobs unset the evaluator never reaches grl_expand_rows (nor a search), twice
    the same sequence; with them set the sequence is that one with a block of search + expansion calls inserted."""
    from grl_amd import engine
    ev, q, gl, qf, gf, ids = eval_case
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    seen = []
    real = engine._call

    def recording(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(engine, '_call', recording)

    def run(rerank):
        del seen[:]
        with contextlib.redirect_stdout(io.StringIO()):
            ev.evaluate(None, None, q, gl, '', 0, rerank)
        return list(seen)
    for rerank in (0, 1):
        monkeypatch.delenv('GRL_EVAL_QE', raising=False)
        monkeypatch.delenv('GRL_EVAL_DBA', raising=False)
        plain = run(rerank)
        assert plain == run(rerank) and plain
        assert 'grl_expand_rows' not in plain and not [n for n in plain if n.startswith('grl_topk')]
        monkeypatch.setenv('GRL_EVAL_QE', '3,2')
        monkeypatch.setenv('GRL_EVAL_DBA', '2,1')
        both = run(rerank)
        added = ['grl_topk_block', 'grl_expand_rows', 'grl_topk_block_filtered', 'grl_expand_rows']
        at = both.index('grl_topk_block')
        assert both[at:at + 4] == added and both[:at] + both[at + 4:] == plain
