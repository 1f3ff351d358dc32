"""Tracklet set distances over clip features (setdist.hip, engine.TrackletSet / set_dist / set_search /
set_metrics_streaming / set_pair_roc, GRL_EVAL_SET) on the device.

The yardsticks are tests/setdist_ref.py -- the header's contract in numpy float32, fed with the clip matrix the EXISTING
engine.cosin_dist / pairwise_distance_tensor make of the clip tensors -- and the existing matrix consumers (rank_rows,
rank_metrics, pair_roc_matrix) on the materialised set distances.  Everything is an equality of bits except the mAP
(fp64 sum in another order: 1e-12).  Run as a script (``--worker``) this file is one rank of test 6."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import setdist_ref as R                                        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
Q_COUNTS = [1, 2, 15, 63, 64, 65, 130]
G_COUNTS = [[1, 3, 64, 65, 17, 129, 2][i % 7] for i in range(37)]
COMBOS = [(r, m) for r in R.REDUCES for m in ('cosine', 'euclidean')]
RANK_TIMEOUT = 240                                             # seconds for one spawned rank, import of torch included


def _bits(t):
    return t.contiguous().view(torch.int32)


def _rows(counts, d, rng, noise=0.35):
    """clip rows = tracklet centre + noise, unit norm (float32 numpy)"""
    rows = []
    for c in counts:
        x = rng.standard_normal(d)[None, :] + noise * np.sqrt(d) * rng.standard_normal((c, d))
        rows.append(x / np.linalg.norm(x, axis=1, keepdims=True))
    return np.concatenate(rows).astype(np.float32)


def _make_sets(q_counts=Q_COUNTS, g_counts=G_COUNTS, d=96, seed=5):
    from grl_amd import engine
    rng = np.random.Generator(np.random.PCG64(seed))
    qc, gc = _rows(q_counts, d, rng), _rows(g_counts, d, rng)
    return (engine.TrackletSet(torch.from_numpy(qc).to(DEV), q_counts),
            engine.TrackletSet(torch.from_numpy(gc).to(DEV), g_counts))


def _ids(nq, ng, seed=9):
    """tracklet ids: every query has matches from another camera, and junk (its pid AND camera) in the gallery"""
    rng = np.random.Generator(np.random.PCG64(seed))
    qp, qc = np.arange(nq) % 5, rng.integers(0, 2, nq)
    gp, gc = np.arange(ng) % 5, np.arange(ng) // 5 % 2         # every pid is in the gallery under both cameras
    return qp, gp, qc, gc


@pytest.fixture(scope='module')
def sets():
    return _make_sets()


@pytest.fixture(scope='module')
def clip_matrix(sets):
    """the clip x clip matrices of the existing evaluator functions, on the host; computed once"""
    from grl_amd import engine
    qset, gset = sets
    return {'cosine': engine.cosin_dist(qset.clips, gset.clips).cpu().numpy(),
            'euclidean': engine.pairwise_distance_tensor(qset.clips, gset.clips).cpu().numpy()}


@pytest.fixture(scope='module')
def dense(sets):
    """engine.set_dist per (reduce, metric), computed once and left unchanged"""
    from grl_amd import engine
    cache = {}

    def get(reduce, metric):
        if (reduce, metric) not in cache:
            cache[reduce, metric] = engine.set_dist(sets[0], sets[1], reduce, metric)
        return cache[reduce, metric]
    return get


# ----------------------------------------------------------------------------
# 1. the kernel against the model, bit for bit
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('reduce,metric', COMBOS)
def test_set_dist_equals_the_model_on_the_existing_clip_matrix(sets, clip_matrix, dense, reduce, metric):
    qset, gset = sets
    want = R.set_dist_from_matrix(clip_matrix[metric], qset.ptr, gset.ptr, reduce)
    got = dense(reduce, metric).cpu().numpy()
    assert got.shape == (7, 37)
    bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
    assert bad.size == 0, (reduce, metric, len(bad), [(int(a), int(b), got[a, b], want[a, b]) for a, b in bad[:5]])


def test_tracklet_set_mean_rows_are_rows_mean_of_the_clips(sets):
    from grl_amd import engine
    qset = sets[0]
    want = torch.cat([engine.rows_mean(qset.clips[int(a):int(b)]) for a, b in zip(qset.ptr, qset.ptr[1:])], 0)
    got = qset.mean_rows()
    assert got.shape == (7, 96) and torch.equal(_bits(got), _bits(want))
    odd = engine.TrackletSet(qset.clips[:, :40].contiguous(), Q_COUNTS)              # padded to 64 columns inside
    assert odd.d == 40 and odd.clips.shape[1] == 64 and odd.mean_rows().shape == (7, 40)
    assert torch.equal(_bits(odd.mean_rows()), _bits(want[:, :40]))


# ----------------------------------------------------------------------------
# 2. blocking does not change a bit
# ----------------------------------------------------------------------------
ONE_PAIR = 4                                                   # bytes: one scratch cell -> one tracklet pair per GEMM tile
RAGGED = 4 * 68000                                             # query ranges of 210 and 130 clips, gallery ranges <= 323


@pytest.mark.parametrize('reduce,metric', [('min', 'cosine'), ('mean', 'cosine'), ('chamfer', 'cosine'),
                                           ('hausdorff', 'cosine'), ('chamfer', 'euclidean'), ('mean', 'euclidean')])
def test_blocks_and_tiles_give_the_bits_of_set_dist(sets, dense, reduce, metric):
    from grl_amd import engine
    qset, gset = sets
    full = dense(reduce, metric)
    for block_bytes in (None, ONE_PAIR, RAGGED):
        for block_cols in (1, 5, 37, None):
            blocks = engine._SetBlocks(qset, gset, reduce, metric, block_cols, block_bytes)
            assert blocks.nq == 7 and blocks.qf is qset.clips
            assert blocks.spans[0][0] == 0 and blocks.spans[-1][1] == 37
            assert all(a[1] == b[0] for a, b in zip(blocks.spans, blocks.spans[1:]))
            if block_cols is not None:
                assert all(c1 - c0 == block_cols for c0, c1 in blocks.spans[:-1])
            for c0, c1 in blocks.spans:
                first = blocks.block(c0, c1).clone()
                assert torch.equal(_bits(first), _bits(full[:, c0:c1])), (block_bytes, block_cols, c0, c1)
                assert torch.equal(_bits(blocks.block(c0, c1)), _bits(first)), (block_bytes, block_cols, c0, c1)


def test_tiles_are_whole_tracklets_within_the_budget(sets):
    from grl_amd import engine
    qset, gset = sets
    pairs = engine._SetBlocks(qset, gset, block_bytes=ONE_PAIR, block_cols=37).tiles(0, 37)
    assert sorted(pairs) == [(a, a + 1, b, b + 1) for a in range(7) for b in range(37)]
    ragged = engine._SetBlocks(qset, gset, block_bytes=RAGGED, block_cols=37).tiles(3, 37)
    assert sorted(set(t[:2] for t in ragged)) == [(0, 6), (6, 7)]
    cols = sorted(set(t[2:] for t in ragged))
    assert cols[0][0] == 3 and cols[-1][1] == 37 and all(a[1] == b[0] for a, b in zip(cols, cols[1:])) and len(cols) > 2
    assert len(set(b1 - b0 for b0, b1 in cols)) > 1                                   # ragged
    for a0, a1, b0, b1 in ragged:
        m, p = int(qset.ptr[a1] - qset.ptr[a0]), int(gset.ptr[b1] - gset.ptr[b0])
        assert 4 * m * p <= RAGGED
    whole = engine._SetBlocks(qset, gset).tiles(0, 37)                                # 256 MiB: one tile
    assert whole == [(0, 7, 0, 37)]


# ----------------------------------------------------------------------------
# 3. the cap: 1024 clips, and what is refused
# ----------------------------------------------------------------------------
def test_a_tracklet_of_1024_clips_equals_the_model_and_1025_or_none_is_refused():
    from grl_amd import engine
    from grl_amd._lib import GrlHipError, ptr
    big, small = _make_sets([1024], [1, 5, 70], d=32, seed=6)
    E = engine.cosin_dist(big.clips, small.clips).cpu().numpy()
    Et = engine.cosin_dist(small.clips, big.clips).cpu().numpy()
    for reduce in R.REDUCES:
        got = engine.set_dist(big, small, reduce).cpu().numpy()
        assert np.array_equal(got.view(np.int32), R.set_dist_from_matrix(E, big.ptr, small.ptr, reduce).view(np.int32))
        got = engine.set_dist(small, big, reduce).cpu().numpy()                       # 1024 columns: 16 pieces
        want = R.set_dist_from_matrix(Et, small.ptr, big.ptr, reduce)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), reduce
    x = torch.zeros((1025, 32), device=DEV)
    with pytest.raises(ValueError, match='at most 1024'):
        engine.TrackletSet(x, [1025])
    with pytest.raises(ValueError, match='at least one clip'):
        engine.TrackletSet(x, [1000, 0, 25])
    e, out = torch.zeros(1025 * 4, device=DEV), torch.zeros(4, device=DEV)
    gp = np.array([0, 1, 2, 3, 4], np.int64)
    for counts, code in (([1025], '(-3)'), ([3, 0, 2], '(-1)')):
        qp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        qd, gd = torch.from_numpy(qp).to(DEV), torch.from_numpy(gp).to(DEV)
        with pytest.raises(GrlHipError, match=code.replace('(', r'\(').replace(')', r'\)')):
            engine._call('grl_setdist_block', ptr(e), 4, qp.ctypes.data, ptr(qd), 0, len(counts), gp.ctypes.data, ptr(gd),
                         0, 4, engine.SET_REDUCE['chamfer'], ptr(out), 4)
    assert bool((out == 0).all())                                                     # refused before any launch


# ----------------------------------------------------------------------------
# 4. NaN
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_a_nan_clip_makes_its_tracklets_column_nan_and_nothing_else(sets, dense, metric):
    from grl_amd import engine
    qset, gset = sets
    bad_t = 12                                                                         # 129 clips: three pieces
    clips = gset.clips.clone()
    clips[int(gset.ptr[bad_t]) + 77] = float('nan')                                    # one clip row
    gnan = engine.TrackletSet(clips, G_COUNTS)
    keep = [b for b in range(37) if b != bad_t]
    fn = engine.cosin_dist if metric == 'cosine' else engine.pairwise_distance_tensor
    E = fn(qset.clips, gnan.clips).cpu().numpy()
    col = slice(int(gset.ptr[bad_t]) + 77, int(gset.ptr[bad_t]) + 78)
    # cosine: -dot of a NaN row is NaN.  euclidean: whatever the existing epilogue makes of a NaN norm -- the model reads
    # the same matrix either way, and where the matrix has the NaN the cell must be the canonical one
    assert metric != 'cosine' or np.isnan(E[:, col]).all()
    nan_cell = bool(np.isnan(E[:, col]).all())
    for reduce in R.REDUCES:
        got = engine.set_dist(qset, gnan, reduce, metric)
        want = R.set_dist_from_matrix(E, qset.ptr, gnan.ptr, reduce)
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), reduce
        assert torch.equal(_bits(got[:, keep]), _bits(dense(reduce, metric)[:, keep])), reduce
        if nan_cell:
            assert bool((_bits(got[:, bad_t]) == 0x7fc00000).all()), reduce
            dist, idx = engine.set_search(qset, gnan, 37, reduce, metric, block_cols=5)
            assert bool((idx[:, -1] == bad_t).all()) and bool((_bits(dist[:, -1]) == 0x7fc00000).all())
            assert not bool(torch.isnan(dist[:, :-1]).any())


# ----------------------------------------------------------------------------
# 5. the consumers on set-distance blocks against the matrix consumers on set_dist
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('block_cols', [5, None])
@pytest.mark.parametrize('reduce,metric', [('chamfer', 'cosine'), ('hausdorff', 'euclidean'), ('mean', 'cosine'),
                                           ('min', 'euclidean')])
def test_search_metrics_and_roc_equal_the_matrix_consumers(sets, dense, reduce, metric, block_cols):
    from grl_amd import engine
    qset, gset = sets
    nq, ng = 7, 37
    D = dense(reduce, metric)
    order = engine.rank_rows(D).long()
    qp, gp, qc, gc = _ids(nq, ng)
    kw = dict(reduce=reduce, metric=metric, block_cols=block_cols, block_bytes=None if block_cols else 4 * 7 * 11)
    junk = (qp[:, None] == gp[None, :]) & (qc[:, None] == gc[None, :])
    assert junk.any(axis=1).all()
    for k in (1, 10, 64):
        kk = min(k, ng)
        dist, idx = engine.set_search(qset, gset, k, **kw)
        assert torch.equal(idx[:, :kk], order[:, :kk])
        assert torch.equal(_bits(dist[:, :kk]), _bits(torch.gather(D, 1, order[:, :kk])))
        assert bool((idx[:, kk:] == -1).all()) and bool(torch.isinf(dist[:, kk:]).all())
        dist, idx = engine.set_search(qset, gset, k, exclude=(qp, gp, qc, gc), **kw)
        for q in range(nq):
            kept = [int(g) for g in order[q].tolist() if not junk[q, g]]
            n = min(k, len(kept))
            assert idx[q, :n].tolist() == kept[:n], (k, q)
            assert torch.equal(_bits(dist[q, :n]), _bits(D[q, kept[:n]])), (k, q)
            assert bool((idx[q, n:] == -1).all()) and bool(torch.isinf(dist[q, n:]).all()) and bool((dist[q, n:] > 0).all())
    with contextlib.redirect_stdout(io.StringIO()):
        cmc_ref, map_ref = engine.rank_metrics(order.int(), qp, gp, qc, gc)
        cmc, mAP = engine.set_metrics_streaming(qset, gset, qp, gp, qc, gc, **kw)
    assert np.array_equal(cmc, cmc_ref) and abs(mAP - map_ref) <= 1e-12
    ref = engine.pair_roc_matrix(D, qp, gp, qc, gc)
    roc = engine.set_pair_roc(qset, gset, qp, gp, qc, gc, **kw)
    assert torch.equal(roc.pos, ref.pos) and torch.equal(roc.neg, ref.neg) and roc.bits == ref.bits
    assert (roc.n_pos, roc.n_neg, roc.auc, roc.eer) == (ref.n_pos, ref.n_neg, ref.auc, ref.eer)


# ----------------------------------------------------------------------------
# 6. a world of two ranks on one GPU: bit-equal to the single process
# ----------------------------------------------------------------------------
def _run_consumers():
    """set_search and set_metrics_streaming with the per-query arrays behind the CMC; CPU tensors"""
    from grl_amd import engine
    qset, gset = _make_sets()
    qp, gp, qc, gc = _ids(qset.n, gset.n)
    out = {}
    for reduce, metric in (('chamfer', 'cosine'), ('hausdorff', 'euclidean')):
        tag = reduce + '/' + metric
        for exclude in (None, (qp, gp, qc, gc)):
            dist, idx = engine.set_search(qset, gset, 10, reduce, metric, exclude=exclude, block_cols=5)
            key = tag + ('/junk' if exclude else '')
            out[key + '/dist'], out[key + '/idx'] = _bits(dist).cpu(), idx.cpu()
        kept = []
        real = engine._cmc_map

        def keep(first, nhit, ap, ng, max_rank):
            kept.append((first.cpu(), nhit.cpu(), ap.cpu()))
            return real(first, nhit, ap, ng, max_rank)
        engine._cmc_map = keep
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                cmc, mAP = engine.set_metrics_streaming(qset, gset, qp, gp, qc, gc, reduce, metric, block_cols=5)
        finally:
            engine._cmc_map = real
        out[tag + '/first'], out[tag + '/nhit'], out[tag + '/ap'] = kept[0]
        out[tag + '/cmc'], out[tag + '/mAP'] = torch.from_numpy(np.asarray(cmc)), float(mAP)
    return out


def _worker(rank, world, port, outdir):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    res = _run_consumers()
    torch.save(res, os.path.join(outdir, 'rank%d.pt' % rank))
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_equal_the_single_process(tmp_path):
    world, port = 2, 39900 + os.getpid() % 1500
    import time
    logs = [open(os.path.join(str(tmp_path), 'rank%d.log' % r), 'wb') for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), '--worker', str(r), str(world), str(port),
                               str(tmp_path)], cwd=ROOT, stdout=logs[r], stderr=subprocess.STDOUT)
             for r in range(world)]
    codes = [None] * world
    deadline = time.monotonic() + RANK_TIMEOUT                 # every rank under its limit, every status looked at
    try:
        while None in codes and all(c in (None, 0) for c in codes) and time.monotonic() < deadline:
            for r, p in enumerate(procs):
                if codes[r] is None:
                    try:
                        codes[r] = p.wait(timeout=0.2)
                    except subprocess.TimeoutExpired:
                        pass
    finally:
        for p in procs:                                        # a rank that failed leaves its peer in a collective
            if p.poll() is None:
                p.kill()
                p.wait()
        for f in logs:
            f.close()
    tails = [open(f.name, 'rb').read().decode('utf-8', 'replace')[-2000:] for f in logs]
    assert codes == [0] * world, (codes, tails)
    ref = _run_consumers()
    for r in range(world):
        got = torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r), weights_only=False)
        assert sorted(got) == sorted(ref)
        for key in ref:
            if key.endswith('/mAP'):
                assert abs(got[key] - ref[key]) <= 1e-12, (r, key)
            elif key.endswith('/ap'):
                assert float((got[key] - ref[key]).abs().max()) <= 1e-12, (r, key)
            else:
                assert torch.equal(got[key], ref[key]), (r, key)


# ----------------------------------------------------------------------------
# 7. the evaluator end to end
# ----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gpu_models(synth_models):
    assert torch.cuda.is_available()
    cnn, siam, siamv = synth_models
    return cnn.to(DEV).eval(), siam.to(DEV).eval(), siamv.to(DEV).eval()


EVAL_KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
              'GRL_EVAL_CLUSTER', 'GRL_EVAL_CLUSTER_JACCARD', 'GRL_EVAL_KMEANS', 'GRL_EVAL_HDBSCAN', 'GRL_EVAL_TSNE',
              'GRL_EVAL_SILHOUETTE', 'GRL_EVAL_PCA', 'GRL_EVAL_DIFFUSION', 'GRL_EVAL_SET')


def _first_ranks(order, qp, gp, qc, gc):
    """per query: the position of its first match among the kept (non-junk) gallery entries of ``order``"""
    out = []
    for q in range(len(qp)):
        kept = [g for g in order[q] if not (gp[g] == qp[q] and gc[g] == qc[q])]
        hits = [r for r, g in enumerate(kept) if gp[g] == qp[q]]
        out.append(hits[0] if hits else -1)
    return out


Q_N = [1, 9, 4, 2, 7]
Q_PIDS, Q_CAMS = [0, 1, 2, 3, 4], [0, 0, 1, 1, 0]
G_PIDS, G_CAMS = [i % 6 for i in range(26)], [(i // 6) % 2 for i in range(26)]
G_N = [(5 * i) % 9 + 1 for i in range(26)]
for _i in range(26):                                           # a match has a whole number of copies of its query's clips
    _p = G_PIDS[_i]
    if _p < 5 and G_CAMS[_i] != Q_CAMS[_p]:
        G_N[_i] = max(1, min(9 // Q_N[_p], round(G_N[_i] / Q_N[_p]))) * Q_N[_p]


@pytest.fixture(scope='module')
def eval_case(gpu_models):
    """five query and twenty-six gallery tracklets of 1-9 clips at T = 2 as dense-mode loaders, and their features:
    extracted once, left unchanged.

    An identity is something the features can see.  Under the synthetic weights any two clips have nearly the same
    features: measured on 40 clips, a clip's dot product with itself is 2.9982 - 2.9984 and with another clip 2.9980 -
    2.9983 for white-noise clips (``synth_clips``), 2.99967 - 2.99985 against 2.9936 - 2.9993 for
    ``synth_clips_structured``, while the fp32 distance GEMM rounds at about 1e-5 at that magnitude.  Pids dealt out over
    unrelated white-noise clips therefore leave every first-match rank to rounding.  Here the clips are the structured
    ones, and a gallery tracklet that is a match of a query (its pid, another camera) is filmed from that query's clips:
    all n of them, once or a whole number of times, so its mean row is the query's and its distance -|mean|^2, below the
    distance to any other mean row m' by |mean - m'|^2 / 2 up to the difference of the two norms -- about 1.4e-3 / n for
    unrelated structured clips (1.6e-4 for the nine-clip query), ten times the rounding or more.  Every other gallery
    tracklet (another pid, the junk of the query's own camera, pid 5 which nobody asks for) has clips of its own."""
    from grl_amd import engine
    from grl_amd.reid.evaluator import ATTEvaluator
    from grl_amd.synthetic import synth_clips_structured as synth_clips
    cnn, siam, _ = gpu_models
    q_clips = [synth_clips(n, 2, seed=300 + i) for i, n in enumerate(Q_N)]

    def gallery_clips(i):
        pid = G_PIDS[i]
        if pid < len(Q_N) and G_CAMS[i] != Q_CAMS[pid]:          # a match of query `pid`
            return q_clips[pid][[j % Q_N[pid] for j in range(G_N[i])]]
        return synth_clips(G_N[i], 2, seed=400 + i)

    def loader(clips, pids, cams):
        return [(x.unsqueeze(0), torch.tensor([pids[i]]), torch.tensor([cams[i]])) for i, x in enumerate(clips)]
    c = {'ql': loader(q_clips, Q_PIDS, Q_CAMS), 'gl': loader([gallery_clips(i) for i in range(26)], G_PIDS, G_CAMS)}
    ev = c['ev'] = ATTEvaluator(cnn, siam, only_eval=True)
    ev.group, ev.chunk = 12, 8                                  # clips are batched across tracklets
    c['plain_q'], c['plain_g'] = ev.extract_feature(c['ql']), ev.extract_feature(c['gl'])
    c['qset'], c['qp'], c['qc'] = ev.extract_clip_features(c['ql'])
    gset, gp, gc = ev.extract_clip_features(c['gl'])
    c['gset'], c['gp'], c['gc'] = gset, gp, gc
    c['gall'] = engine.TrackletSet(torch.cat((c['qset'].clips, gset.clips), 0), Q_N + G_N)     # the query is prepended
    c['gp_all'], c['gc_all'] = np.append(c['qp'], gp), np.append(c['qc'], gc)
    return c


def _keep_first_ranks(monkeypatch):
    """every _cmc_map call (the streamed routes end in one) leaves its per-query first-match ranks in the list"""
    from grl_amd import engine
    firsts, real = [], engine._cmc_map

    def keep(first, nhit, ap, ng, max_rank):
        firsts.append(first.cpu().tolist())
        return real(first, nhit, ap, ng, max_rank)
    monkeypatch.setattr(engine, '_cmc_map', keep)
    return firsts


def test_evaluator_end_to_end_on_set_distances(eval_case, capsys, monkeypatch, tmp_path):
    from grl_amd import engine
    c = eval_case
    ev, ql, gl, qset, gall = c['ev'], c['ql'], c['gl'], c['qset'], c['gall']
    for name in EVAL_KNOBS:
        monkeypatch.delenv(name, raising=False)
    # extract_clip_features returns the rows extract_feature averages, and the same ids
    assert list(qset.counts) == Q_N and list(c['gset'].counts) == G_N and qset.clips.shape == (sum(Q_N), 6144)
    assert list(c['qp']) == Q_PIDS and list(c['qc']) == Q_CAMS and list(c['gp']) == G_PIDS and list(c['gc']) == G_CAMS
    assert np.array_equal(c['plain_q'][1], c['qp']) and np.array_equal(c['plain_g'][2], c['gc'])
    assert c['plain_q'][0].shape == (5, 6144) and torch.equal(_bits(qset.mean_rows()), _bits(c['plain_q'][0]))
    assert torch.equal(_bits(c['gset'].mean_rows()), _bits(c['plain_g'][0]))
    # extract_feature does not see the knob
    monkeypatch.setenv('GRL_EVAL_SET', 'chamfer')
    again = ev.extract_feature(ql)
    assert torch.equal(_bits(c['plain_q'][0]), _bits(again[0]))
    assert np.array_equal(c['plain_q'][1], again[1]) and np.array_equal(c['plain_q'][2], again[2])

    firsts = _keep_first_ranks(monkeypatch)
    capsys.readouterr()
    r1 = ev.evaluate(None, None, ql, gl, None, False, False)
    out = capsys.readouterr().out
    assert 'Tracklet set distance: chamfer (cosine), %d clips in 31 tracklets' % (sum(Q_N) + sum(G_N)) in out
    assert 'Mean AP:' in out and 'Rank-1' in out
    assert out.index('Tracklet set distance') < out.index('Mean AP:')
    D = engine.set_dist(qset, gall, 'chamfer')
    order = engine.rank_rows(D)
    with contextlib.redirect_stdout(io.StringIO()):
        cmc, _ = engine.rank_metrics(order, c['qp'], c['gp_all'], c['qc'], c['gc_all'])
    assert r1 == cmc[0]
    assert firsts[-1] == _first_ranks(order.cpu().tolist(), c['qp'], c['gp_all'], c['qc'], c['gc_all'])
    # GRL_EVAL_ROC on the same route: the lines carry the route's label
    monkeypatch.setenv('GRL_EVAL_SET', 'hausdorff,euclidean')
    monkeypatch.setenv('GRL_EVAL_ROC', '1')
    ev.evaluate(None, None, ql, gl, str(tmp_path) + os.sep, False, False)
    out = capsys.readouterr().out
    assert 'Tracklet set distance: hausdorff (euclidean)' in out and 'ROC AUC:' in out and 'EER:' in out
    with open(os.path.join(str(tmp_path), 'roc.json')) as fh:
        assert '"metric": "set(hausdorff,euclidean)"' in fh.read()


def test_set_mean_keeps_the_first_match_ranks_of_the_plain_dense_run(eval_case, capsys, monkeypatch):
    """GRL_EVAL_SET=mean against the plain dense run (GRL_EVAL_STREAM=1, so both routes report their per-query
    first-match ranks): equal, except where the plain run separates the two neighbours that changed places by less than
    1e-6 -- the allowance the feature's specification sets.

    The tracklets of ``eval_case`` give every query matches that the features tell apart from the rest by far more than
    fp32 rounding, so the ranks are decided by the tracklets and not by the last bits.  (On pids dealt out over unrelated
    white-noise clips both routes are within 1e-5 of the float64 value and a row's neighbours 1.7e-6 apart: EXPERIMENTS.md.)
    Measured: first-match ranks [0, 6, 0, 0, 0] on both routes -- single-clip rows have the larger norm and pass the
    nine-clip query's matches on both -- and no entries change places around a match."""
    from grl_amd import engine
    c = eval_case
    ev, ql, gl, qset, gall, qp, gp_all = c['ev'], c['ql'], c['gl'], c['qset'], c['gall'], c['qp'], c['gp_all']
    for name in EVAL_KNOBS:
        monkeypatch.delenv(name, raising=False)
    firsts = _keep_first_ranks(monkeypatch)
    monkeypatch.setenv('GRL_EVAL_SET', 'mean')
    ev.evaluate(None, None, ql, gl, None, False, False)
    first_set = firsts[-1]
    monkeypatch.delenv('GRL_EVAL_SET')
    monkeypatch.setenv('GRL_EVAL_STREAM', '1')
    ev.evaluate(None, None, ql, gl, None, False, False)
    first_plain = firsts[-1]
    capsys.readouterr()
    dm = engine.cosin_dist(c['plain_q'][0], torch.cat((c['plain_q'][0], c['plain_g'][0]), 0))
    Dm, order_m = dm.double().cpu().numpy(), engine.rank_rows(dm).cpu().numpy()
    order_s = engine.rank_rows(engine.set_dist(qset, gall, 'mean')).cpu().numpy()
    swaps, worst = 0, []
    for q in range(5):
        if first_set[q] == first_plain[q]:
            continue
        swaps += 1                                  # allowed only between neighbours the plain run barely separates
        pos_m, pos_s = np.argsort(order_m[q]), np.argsort(order_s[q])
        for g1 in range(31):
            for g2 in range(g1 + 1, 31):
                match = gp_all[g1] == qp[q] or gp_all[g2] == qp[q]
                if match and (pos_m[g1] < pos_m[g2]) != (pos_s[g1] < pos_s[g2]):
                    worst.append((abs(Dm[q, g1] - Dm[q, g2]), q, g1, g2))
    with capsys.disabled():
        print('\n[GRL_EVAL_SET=mean vs plain dense] first-match ranks %s / %s: %d of 5 differ; largest plain-run gap '
              'between two entries that changed places around a match: %.3e'
              % (first_set, first_plain, swaps, max(worst)[0] if worst else 0.0))
    assert all(w[0] < 1e-6 for w in worst), sorted(worst, reverse=True)[:5]


if __name__ == '__main__':
    if len(sys.argv) == 6 and sys.argv[1] == '--worker':
        _worker(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
    else:
        sys.exit('usage: test_gpu_setdist.py --worker RANK WORLD PORT OUTDIR')
