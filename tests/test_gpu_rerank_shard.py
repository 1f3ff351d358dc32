"""Streaming k-reciprocal re-ranking sharded over the ranks of a process group: the sample passes by
contiguous sample range, the final pass by gallery column, CSR / CSC assembly by rerank_stream.hip's own kernels.

The ranks are started as in test_gpu_dist.py: spawned processes that share cuda:0 and talk over gloo (device tensors
staged through the host by grl_amd.dist), results written to a temporary directory and compared in the parent with
the single-process run.  The contract is equality: every value is produced by the same fp32 operations, only by
another rank, so nothing here has a tolerance except the mAP (fp64 sum in another order, 1e-12 as in DESIGN 4n)."""
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

# name -> (nq, ng, seed, synth_eval_features keywords, block_cols, (k1, k2)).  N = nq + ng is odd and not a multiple
# of 3 except where noted; shard_rows(299, ., 2) = [0, 150, 299] and shard_rows(299, ., 3) = [0, 100, 200, 299], so
# `edge2` has the query/gallery boundary on a range edge in a world of 2 and inside a range in a world of 3, `edge3`
# the other way round.  block_cols = 32 gives every rank several sample blocks and several column blocks.
CASES = {
    'edge2': (150, 149, 11, dict(n_ids=30, noise=5.0), 32, (20, 6)),
    'edge3': (100, 199, 12, dict(n_ids=30, noise=5.0), 32, (20, 6)),
    'k1k2_one': (100, 199, 13, dict(n_ids=30, noise=5.0), 32, (1, 1)),
    'fixture': (40, 400, 1, dict(n_ids=24, noise=7.0), 64, (20, 6)),       # tests/golden/evaluator_q40_g400.npz's inputs
    'tiny_gallery': (40, 2, 14, dict(n_ids=3, noise=1.0), None, (20, 6)),  # fewer gallery columns than ranks (world 3)
    'n3000': (300, 2701, 7, dict(n_ids=200, noise=7.0), 512, (20, 6)),
}
SMALL = ('edge2', 'edge3', 'k1k2_one', 'fixture', 'tiny_gallery')
COUNTED = 'edge3'                 # the case whose library calls are recorded


def _bits(t):
    return t.contiguous().view(torch.int32)


def _inputs(name):
    nq, ng, seed, kw, width, ks = CASES[name]
    if name in ('fixture', 'n3000'):                    # the evaluator's layout: the query rows lead the gallery
        qf, gf, qp, qc, gp, gc = synth_eval_features(nq, ng, seed=seed, **kw)
    else:                                               # disjoint query and gallery rows (nq may exceed ng)
        _, x, _, _, pids, cams = synth_eval_features(1, nq + ng, seed=seed, **kw)
        qf, gf, qp, qc, gp, gc = x[:nq], x[nq:], pids[:nq], cams[:nq], pids[nq:], cams[nq:]
    if name == 'tiny_gallery':                          # both gallery entries match some query from another camera
        gp, gc = np.array([qp[0], qp[1]]), np.array([qc[0] + 1, qc[1] + 1])
    return qf.to(DEV), gf.to(DEV), qp, qc, gp, gc, width, ks


def _ks(ng):
    return sorted(set((1, 10, min(1024, ng), 1024)))


def _run_case(name, record=None):
    """rerank_search for every k and rerank_metrics_streaming with the per-query arrays behind it; CPU tensors."""
    from grl_amd import engine
    qf, gf, qp, qc, gp, gc, width, (k1, k2) = _inputs(name)
    out = {}
    real_call = engine._call
    if record is not None:
        def counting(fn_name, *args):
            if fn_name == 'grl_rrs_segment_rows':       # (up, ldu, lo, lrs, lcs, nq, ng, w, colmax + s0, drows, ldd)
                record.append(('A1', int(args[8]), int(args[7])))
            elif fn_name == 'grl_rrs_weights':          # (up, ldu, lo, lrs, lcs, nq, ng, w, s0, colmax, ...)
                record.append(('A2', int(args[9]), int(args[8]), int(args[7])))
            return real_call(fn_name, *args)
        engine._call = counting
    try:
        for k in _ks(gf.shape[0]):
            dist, idx = engine.rerank_search(qf, gf, k, k1=k1, k2=k2, block_cols=width)
            out['dist%d' % k], out['idx%d' % k] = _bits(dist).cpu(), idx.cpu()
            if record is not None:
                engine._call = real_call                # one call's worth of records is what the parent checks
    finally:
        engine._call = real_call
    kept = []
    real_cmc = engine._cmc_map

    def keep(first, nhit, ap, ng, max_rank):
        kept.append((first.cpu(), nhit.cpu(), ap.cpu()))
        return real_cmc(first, nhit, ap, ng, max_rank)
    engine._cmc_map = keep
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            cmc, mAP = engine.rerank_metrics_streaming(qf, gf, qp, gp, qc, gc, k1=k1, k2=k2, block_cols=width)
    finally:
        engine._cmc_map = real_cmc
    out['first'], out['nhit'], out['ap'] = kept[0]
    out['cmc'], out['mAP'] = torch.from_numpy(np.asarray(cmc)), float(mAP)
    return out


def _worker(rank, world, port, outdir, names):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    res = {}
    for name in names:
        record = [] if name == COUNTED else None
        res[name] = _run_case(name, record)
        if record is not None:
            base = [r[1] for r in record if r[0] == 'A2'][0]          # colmax's address: pass A2 hands it over whole
            res['calls'] = dict(A1=[((p - base) // 4, (p - base) // 4 + w) for tag, p, w in
                                    (r for r in record if r[0] == 'A1')],
                                A2=[(r[2], r[2] + r[3]) for r in record if r[0] == 'A2'])
    torch.save(res, os.path.join(outdir, 'rank%d.pt' % rank))
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


def _spawn(world, names, tmp_path_factory, port0):
    outdir = str(tmp_path_factory.mktemp('shard_w%d' % world))
    mp.spawn(_worker, args=(world, port0 + os.getpid() % 1500, outdir, names), nprocs=world, join=True)
    return [torch.load(os.path.join(outdir, 'rank%d.pt' % r), weights_only=False) for r in range(world)]


@pytest.fixture(scope='module')
def single():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run_case(name)
        return cache[name]
    return get


@pytest.fixture(scope='module')
def world2(tmp_path_factory):
    return _spawn(2, SMALL + ('n3000',), tmp_path_factory, 35100)


@pytest.fixture(scope='module')
def world3(tmp_path_factory):
    return _spawn(3, SMALL, tmp_path_factory, 36700)


def _assert_equal_results(got, ref, what):
    for key in ref:
        if key == 'mAP':
            assert abs(got[key] - ref[key]) <= 1e-12, (what, key, got[key], ref[key])
        elif key == 'ap':
            assert float((got[key] - ref[key]).abs().max()) <= 1e-12, (what, key)
        else:
            assert torch.equal(got[key], ref[key]), (what, key)


# ----------------------------------------------------------------------------
# 1. CSR / CSC assembly kernels against the torch construction they replace
# ----------------------------------------------------------------------------
def _torch_construction(cnt, col, val, nq, N):
    """row_ptr and the gallery rows' CSC as engine._Rerank built them before grl_rrs_scan / grl_rrs_transpose."""
    dev = cnt.device
    row_ptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    torch.cumsum(cnt, 0, out=row_ptr[1:])
    nnz = int(row_ptr[-1].item())
    g0 = int(row_ptr[nq].item())
    kcol = col[g0:nnz].long()
    order = torch.sort(kcol, stable=True).indices
    grow = torch.repeat_interleave(torch.arange(nq, N, dtype=torch.int32, device=dev), cnt[nq:].long(),
                                   output_size=nnz - g0)
    csc_ptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(kcol, minlength=N), 0, out=csc_ptr[1:])
    return row_ptr, csc_ptr, grow[order].contiguous(), val[g0:nnz][order].contiguous()


def _random_csr(N, nq, max_cnt, seed, empty_rows=0.2, even_cols=False, hubs=(), gallery_empty=False):
    g = np.random.Generator(np.random.PCG64(seed))
    pool = np.arange(0, N, 2) if even_cols else np.arange(N)
    rows = []
    for i in range(N):
        n = 0 if (g.random() < empty_rows or (gallery_empty and i >= nq)) else int(g.integers(0, max_cnt + 1))
        c = set(g.choice(pool, size=min(n, pool.size), replace=False).tolist())
        for h, share in hubs:
            if i >= nq and g.random() < share:
                c.add(h)
        rows.append(np.sort(np.fromiter(c, dtype=np.int64, count=len(c))))
    cnt = np.array([r.size for r in rows], dtype=np.int32)
    col = np.concatenate(rows).astype(np.int32) if cnt.sum() else np.zeros(0, np.int32)
    val = g.random(col.size, dtype=np.float32) + np.float32(0.01)
    return torch.from_numpy(cnt).to(DEV), torch.from_numpy(col).to(DEV), torch.from_numpy(val).to(DEV)


CSR_CASES = {
    'one_sample': dict(N=1, nq=0, max_cnt=1, empty_rows=0.0),
    'seven': dict(N=7, nq=3, max_cnt=5),
    'one_gallery_row': dict(N=300, nq=299, max_cnt=40, empty_rows=0.0),
    'no_queries': dict(N=1000, nq=0, max_cnt=30),
    'empty_rows_and_columns': dict(N=2049, nq=517, max_cnt=60, empty_rows=0.3, even_cols=True),
    'long_columns': dict(N=3001, nq=100, max_cnt=20, hubs=((5, 1.0), (7, 0.5), (3000, 0.4))),   # > one LDS chunk of 1024
    'nnz_zero': dict(N=50, nq=10, max_cnt=0),
    'gallery_rows_empty': dict(N=50, nq=10, max_cnt=8, gallery_empty=True),
}


@pytest.mark.parametrize('name', sorted(CSR_CASES))
def test_scan_and_transpose_equal_the_torch_construction(name):
    from grl_amd import engine
    from grl_amd._lib import ptr
    kw = dict(CSR_CASES[name])
    N, nq = kw.pop('N'), kw.pop('nq')
    cnt, col, val = _random_csr(N, nq, seed=len(name), **kw)
    row_ref, ptr_ref, crow_ref, cval_ref = _torch_construction(cnt, col, val, nq, N)
    row_ptr = torch.full((N + 1,), -7, dtype=torch.int64, device=DEV)
    engine._call('grl_rrs_scan', ptr(cnt), N, ptr(row_ptr))
    assert torch.equal(row_ptr, row_ref)
    n_g = crow_ref.numel()
    if name == 'long_columns':
        assert int((ptr_ref[1:] - ptr_ref[:-1]).max()) > 2048
    colp = col if col.numel() else torch.zeros(1, dtype=torch.int32, device=DEV)
    valp = val if val.numel() else torch.zeros(1, dtype=torch.float32, device=DEV)
    runs = []
    for _ in range(2):
        csc_ptr = torch.full((N + 1,), -7, dtype=torch.int64, device=DEV)
        csc_row = torch.full((max(n_g, 1),), -7, dtype=torch.int32, device=DEV)
        csc_val = torch.full((max(n_g, 1),), float('nan'), dtype=torch.float32, device=DEV)
        ccnt = torch.full((N,), 99, dtype=torch.int32, device=DEV)
        tmp_row, tmp_val = torch.empty_like(csc_row), torch.empty_like(csc_val)
        engine._call('grl_rrs_transpose', ptr(row_ptr), ptr(colp), ptr(valp), nq, N, ptr(ccnt), ptr(tmp_row),
                     ptr(tmp_val), ptr(csc_ptr), ptr(csc_row), ptr(csc_val))
        assert torch.equal(csc_ptr, ptr_ref)
        assert torch.equal(csc_row[:n_g], crow_ref)
        assert torch.equal(_bits(csc_val[:n_g]), _bits(cval_ref))
        runs.append((csc_row, csc_val))
    assert torch.equal(runs[0][0][:n_g], runs[1][0][:n_g])
    # rows ascending inside every column
    if n_g > 1:
        same_col = torch.repeat_interleave(torch.arange(N, device=DEV), (ptr_ref[1:] - ptr_ref[:-1]))
        inside = same_col[1:] == same_col[:-1]
        assert bool((crow_ref[1:][inside] > crow_ref[:-1][inside]).all())


def test_place_puts_packed_shards_at_their_row_offsets():
    from grl_amd import engine
    from grl_amd._lib import ptr
    N, nq = 1001, 37
    cnt, col, val = _random_csr(N, nq, 25, seed=5)
    row_ptr = torch.empty(N + 1, dtype=torch.int64, device=DEV)
    engine._call('grl_rrs_scan', ptr(cnt), N, ptr(row_ptr))
    rp = row_ptr.cpu().tolist()
    out_c = torch.full_like(col, -1)
    out_v = torch.full_like(val, float('nan'))
    bounds = [0, 334, 334, 668, 1001]                       # an empty shard among them
    cap = max(rp[b1] - rp[b0] for b0, b1 in zip(bounds, bounds[1:])) + 13
    for b0, b1 in zip(bounds, bounds[1:]):
        n = rp[b1] - rp[b0]
        src_c = torch.full((cap,), -5, dtype=torch.int32, device=DEV)      # padded as an uneven all-gather leaves it
        src_v = torch.full((cap,), -5.0, dtype=torch.float32, device=DEV)
        src_c[:n], src_v[:n] = col[rp[b0]:rp[b1]], val[rp[b0]:rp[b1]]
        engine._call('grl_rrs_place', ptr(src_c), ptr(src_v), cap, ptr(row_ptr), b0, b1, ptr(out_c), ptr(out_v))
    assert torch.equal(out_c, col) and torch.equal(_bits(out_v), _bits(val))


# ----------------------------------------------------------------------------
# 2. one process: still the materialised device path, with the device-built CSR / CSC
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['fixture', 'edge2', 'k1k2_one', 'n3000'])
def test_single_process_equals_the_materialised_re_ranking(name, single):
    from grl_amd import engine
    from grl_amd.reid.evaluator.rerank import re_ranking
    qf, gf, qp, qc, gp, gc, width, (k1, k2) = _inputs(name)
    F = re_ranking(engine.cosin_dist(qf, gf), engine.pairwise_distance_tensor(qf, qf),
                   engine.pairwise_distance_tensor(gf, gf), k1=k1, k2=k2, lambda_value=0.3)
    order = engine.rank_rows(F)
    with contextlib.redirect_stdout(io.StringIO()):
        cmc_ref, map_ref = engine.rank_metrics(order, qp, gp, qc, gc)
    ref, got = order.long(), single(name)
    for k in _ks(gf.shape[0]):
        kk = min(k, gf.shape[0])
        assert torch.equal(got['idx%d' % k][:, :kk], ref[:, :kk].cpu()), k
        assert torch.equal(got['dist%d' % k][:, :kk], _bits(torch.gather(F, 1, ref[:, :kk])).cpu()), k
        assert bool((got['idx%d' % k][:, kk:] == -1).all())
    assert np.array_equal(got['cmc'].numpy(), cmc_ref) and abs(got['mAP'] - map_ref) <= 1e-12
    if name == 'n3000':                                  # other block widths change nothing
        for w in (96, 1000, None):
            dist, idx = engine.rerank_search(qf, gf, 10, k1=k1, k2=k2, block_cols=w)
            assert torch.equal(idx.cpu(), got['idx10']) and torch.equal(_bits(dist).cpu(), got['dist10']), w


# ----------------------------------------------------------------------------
# 3. worlds of two and three ranks: every rank returns the single-process result
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('name', SMALL + ('n3000',))
def test_two_ranks_equal_one_process(name, world2, single):
    for r in range(2):
        _assert_equal_results(world2[r][name], single(name), (name, 'rank', r))


@pytest.mark.parametrize('name', SMALL)
def test_three_ranks_equal_one_process(name, world3, single):
    for r in range(3):
        _assert_equal_results(world3[r][name], single(name), (name, 'rank', r))


# ----------------------------------------------------------------------------
# 4. the work is divided: each rank's GEMM passes touch its own samples only
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('world', [2, 3])
def test_each_rank_runs_the_sample_passes_for_its_own_range_only(world, world2, world3):
    from grl_amd import dist as grl_dist
    ranks = world2 if world == 2 else world3
    nq, ng = CASES[COUNTED][:2]
    N = nq + ng
    for tag in ('A1', 'A2'):
        everything = []
        for r in range(world):
            lo, hi = grl_dist.shard_rows(N, r, world)
            spans = ranks[r]['calls'][tag]
            assert len(spans) >= 3, (tag, r, spans)              # several sample blocks per rank
            assert all(lo <= a < b <= hi for a, b in spans), (tag, r, (lo, hi), spans)
            everything += spans
        everything.sort()
        assert everything[0][0] == 0 and everything[-1][1] == N
        assert all(a[1] == b[0] for a, b in zip(everything, everything[1:])), (tag, everything)   # exactly once


# ----------------------------------------------------------------------------
# 5. ATTEvaluator with GRL_EVAL_RERANK=stream under two ranks
# ----------------------------------------------------------------------------
def _run_eval_rerank():
    from torch.utils.data import DataLoader
    from grl_amd.reid.evaluator import ATTEvaluator
    from grl_amd.reid.data import SyntheticPairs
    from test_gpu_dist import _models, T
    cnn, siam, _ = _models(DEV)
    ev = ATTEvaluator(cnn, siam, only_eval=False)
    q = DataLoader(SyntheticPairs(5, T, seed=11), batch_size=4)           # 10 clips: batches of 4, 4, 2
    g = DataLoader(SyntheticPairs(13, T, seed=12), batch_size=4)          # 26 clips: 7 batches, ragged tail
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        r1 = ev.evaluate(None, None, q, g, None, False, True)
    lines = [l for l in buf.getvalue().splitlines() if l.startswith(('Mean AP', 'Rank-'))]
    return float(r1), lines, 'Applying person re-ranking ...' in buf.getvalue()


def _eval_worker(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), GRL_EVAL_RERANK='stream')
    os.environ.pop('GRL_EVAL_STREAM', None)
    import torch.distributed as dist
    from grl_amd import engine
    dist.init_process_group('gloo', rank=rank, world_size=world)
    seen = []
    real_call = engine._call

    def counting(fn_name, *args):
        if fn_name == 'grl_rrs_segment_rows':
            seen.append(int(args[7]))
        return real_call(fn_name, *args)
    engine._call = counting
    try:
        res = _run_eval_rerank()
    finally:
        engine._call = real_call
    torch.save((res, sum(seen)), os.path.join(outdir, 'rank%d.pt' % rank))
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


def test_attevaluator_streaming_re_ranking_under_two_ranks(tmp_path, monkeypatch):
    world = 2
    mp.spawn(_eval_worker, args=(world, 38300 + os.getpid() % 1500, str(tmp_path)), nprocs=world, join=True)
    monkeypatch.setenv('GRL_EVAL_RERANK', 'stream')
    monkeypatch.delenv('GRL_EVAL_STREAM', raising=False)
    ref = _run_eval_rerank()
    assert ref[2] and len(ref[1]) == 5
    samples = 0
    for r in range(world):
        got, n = torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r), weights_only=False)
        assert got == ref, (r, got, ref)
        samples += n
    assert samples == 10 + (10 + 26)            # q + g samples (the query is prepended to the gallery), each once
