"""HDBSCAN on the device (engine.mutual_reachability_mst / hdbscan / hdbscan_matrix / hdbscan_from_mst, hdbscan.hip,
DESIGN.md 4x) against the numpy model of tests/hdbscan_ref.py.  Under the strict edge order (w, lo, hi) the minimum
spanning forest is unique, so the device's core distances and edges are compared bit for bit and edge for edge with the
model (Kruskal) run on the read-back device distances; the labels with the model's cut, numbering included, and on the
cases of tests/test_hdbscan_cpu.py with scikit-learn's partition."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import hdbscan_ref as HR
import silhouette_ref as SR

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
WIDTHS = (1, 7, 64, 100, 336)
SK_CASES = [(2, 1), (5, 2), (10, 3)]

_cache = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    """bit patterns equal, any NaN equal to any NaN"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def symmetric(m):
    return np.array_equal(bits(m), bits(m.T))


def device_distances(x):
    """(cosine distances by the contract's symmetric chain, euclidean distances) as float32 host matrices from what the
    device computes for the rows ``x`` (zero-padded as the engine pads them) -- after asserting the precondition: the
    device's cosin_dist and pairwise_distance_tensor of a set against itself are symmetric bit for bit."""
    from grl_amd import engine
    xp = engine._pad_features(x)
    n, d = xp.shape
    sq = torch.empty(n, dtype=torch.float32, device=DEV)
    engine._call('grl_row_sqnorm', engine.ptr(xp), engine.ptr(sq), n, d, d)
    negdot = engine.cosin_dist(xp, xp).cpu().numpy()
    euc = engine.pairwise_distance_tensor(xp, xp).cpu().numpy()
    assert symmetric(negdot) and symmetric(euc)
    return HR.cosine_matrix(negdot, sq.cpu().numpy()), euc


def case(d=24, n=336):
    """The first ``n`` rows of the planted input of the CPU test (336 samples in clusters of 1 .. 130, norms 0.5 .. 1.8,
    shuffled) in d = 24 or d = 5 features and their device distances.  Built once."""
    if (d, n) not in _cache:
        x, ids = SR.planted(d=d)
        x, ids = x[:n], ids[:n]
        xd = dev(x)
        cos, euc = device_distances(xd)
        _cache[d, n] = {'x': xd, 'host': x, 'ids': ids, 'cosine': cos, 'euclidean': euc, 'forest': {}}
    return _cache[d, n]


def model_forest(c, metric, ms):
    if (metric, ms) not in c['forest']:
        c['forest'][metric, ms] = HR.forest(c[metric], ms)
    return c['forest'][metric, ms]


def rounds_bound(n):
    return int(np.ceil(np.log2(n))) + 1


def check_forest(got, want, n):
    lo, hi, w, core, info = got
    wlo, whi, ww, wcore = want
    assert (lo.dtype, hi.dtype, w.dtype, core.dtype) == (torch.int32, torch.int32, torch.float32, torch.float32)
    assert same(core.cpu().numpy(), wcore)
    assert np.array_equal(lo.cpu().numpy(), wlo) and np.array_equal(hi.cpu().numpy(), whi)
    assert same(w.cpu().numpy(), ww)
    assert info['n_dropped'] == 0 and 0 <= info['rounds'] <= rounds_bound(n)


def mst_equal(a, b):
    return all(torch.equal(s, t) for s, t in zip(a[:2], b[:2])) and same(a[2].cpu().numpy(), b[2].cpu().numpy())


# ----------------------------------------------------------------------------
# 1. the forest and the core distances, bit for bit against the model on the device's own distances
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('d', [24, 5])
@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_forest_equals_the_model_for_every_block_width(metric, d):
    from grl_amd import engine
    c = case(d)
    n = 336
    assert symmetric(c[metric])                                  # (the feature forms' precondition, see device_distances)
    for ms in (1, 2, 5):
        want = model_forest(c, metric, ms)
        assert want[0].size == n - 1
        for width in (None,) + WIDTHS:
            got = engine.mutual_reachability_mst(c['x'], ms, metric, block_cols=width)
            check_forest(got, want, n)
        check_forest(engine.mutual_reachability_mst(c['x'], ms, metric, block_bytes=1), want, n)   # the floor of 256 columns
        assert got[4]['rounds'] >= 2


@pytest.mark.parametrize('n', [65, 129])
@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_forest_at_the_lane_chunk_edges(metric, n):
    """One wave reads a row in chunks of 64 columns: n = 65 and 129 leave a chunk of one column, widths 63 .. 65 cut
    just before, on and just after the chunk edge."""
    from grl_amd import engine
    c = case(24, n)
    want = model_forest(c, metric, 2)
    for width in (63, 64, 65, None):
        check_forest(engine.mutual_reachability_mst(c['x'], 2, metric, block_cols=width), want, n)


# ----------------------------------------------------------------------------
# 2. the matrix form: heavy ties, NaN rows, +inf blocks, strided rows, asymmetry
# ----------------------------------------------------------------------------
def test_heavy_ties_give_the_models_forest_exactly():
    """Weights drawn from {1, 2, 3}: nearly every comparison is a tie, and only the order (w, lo, hi) -- the same from
    both ends of an edge, in every lane and across the block cuts -- keeps the rounds from closing cycles or losing
    edges."""
    from grl_amd import engine
    g = np.random.Generator(np.random.PCG64(3))
    n = 130
    a = g.integers(1, 4, (n, n)).astype(np.float32)
    a = np.minimum(a, a.T)
    np.fill_diagonal(a, 0.0)
    ad = dev(a)
    for ms in (1, 2, 3):
        want = HR.forest(a, ms)
        assert want[0].size == n - 1
        for width in (None, 7, 64, 65):
            r = engine.hdbscan_matrix(ad, 5, ms, block_cols=width)
            check_forest(r.mst + (r.core_dist, {'rounds': r.rounds, 'n_dropped': r.n_dropped}), want, n)
            assert r.mst[0].numel() == n - 1 and r.metric == 'precomputed'
            assert np.array_equal(r.labels.cpu().numpy(), HR.cut(*want[:3], n, 5)[0])


def test_nan_rows_inf_blocks_and_strided_matrices():
    from grl_amd import engine
    c = case()
    n = 80
    a = c['euclidean'][:n, :n].copy()
    a[:40, 40:] = np.inf                                         # two groups without a finite distance between them
    a[40:, :40] = np.inf
    a[7, :] = np.nan                                             # a sample whose distances are all NaN
    a[:, 7] = np.nan
    assert symmetric(a)
    wide = torch.full((n, n + 13), float('nan'), dtype=torch.float32, device=DEV)
    wide[:, 5:5 + n] = dev(a)
    strided = wide[:, 5:5 + n]
    assert strided.stride(0) == n + 13 and not strided.is_contiguous()
    for ms in (1, 2, 4):
        want = HR.forest(a, ms)
        assert want[0].size == n - 3                             # a forest: two trees and the loner
        for m, width in ((dev(a), None), (dev(a), 7), (strided, None), (strided, 64)):
            r = engine.hdbscan_matrix(m, 30, ms, block_cols=width)
            check_forest(r.mst + (r.core_dist, {'rounds': r.rounds, 'n_dropped': r.n_dropped}), want, n)
            lab = r.labels.cpu().numpy()
            # the virtual-root rule: neither tree splits into two parts of 30, so each is one selectable cluster
            assert lab[7] == -1 and r.n_clusters == 2 and r.n_noise == 1
            assert (np.delete(lab[:40], 7) == 0).all() and (lab[40:] == 1).all()
            assert np.array_equal(lab, HR.cut(*want[:3], n, 30)[0])
        assert np.isnan(r.core_dist.cpu().numpy()[7]) == (ms > 1)
        # a finer cut of the same forest: the model's labels, numbering included
        for method in ('eom', 'leaf'):
            r5 = engine.hdbscan_matrix(strided, 5, ms, method)
            labels, stab = HR.cut(*want[:3], n, 5, method)
            assert np.array_equal(r5.labels.cpu().numpy(), labels) and np.array_equal(r5.stabilities, stab)
            assert r5.labels[7] == -1 and r5.n_clusters == stab.size >= 2


def test_asymmetric_matrix_is_refused():
    from grl_amd import engine
    c = case()
    a = c['euclidean'][:40, :40].copy()
    engine.hdbscan_matrix(dev(a), 5)
    b = a.copy()
    b[3, 9] = np.nextafter(b[3, 9], np.float32(np.inf))          # one bit
    with pytest.raises(ValueError, match='symmetric bit for bit'):
        engine.hdbscan_matrix(dev(b), 5)
    z = a.copy()
    z[3, 9] = z[9, 3] = 0.0
    engine.hdbscan_matrix(dev(z), 5)
    z[9, 3] = -0.0                                               # equal as numbers, not as bits
    with pytest.raises(ValueError, match='symmetric bit for bit'):
        engine.hdbscan_matrix(dev(z), 5)
    with pytest.raises(ValueError, match='square'):
        engine.hdbscan_matrix(dev(a)[:, :39], 5)
    with pytest.raises(ValueError, match='float32'):
        engine.hdbscan_matrix(dev(a).double(), 5)


# ----------------------------------------------------------------------------
# 3. the labels
# ----------------------------------------------------------------------------
def sklearn_labels(d, mcs, ms, method):
    from sklearn.cluster import HDBSCAN
    d64 = np.minimum(d, d.T).astype(np.float64)
    np.fill_diagonal(d64, 0.0)
    return HDBSCAN(min_cluster_size=mcs, min_samples=ms, metric='precomputed', allow_single_cluster=False,
                   cluster_selection_method=method).fit(d64).labels_


@pytest.mark.parametrize('method', ['eom', 'leaf'])
@pytest.mark.parametrize('mcs,ms', SK_CASES)
@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_labels_equal_the_models_cut_and_sklearns_partition(metric, mcs, ms, method):
    from grl_amd import engine
    c = case()
    n = 336
    r = engine.hdbscan(c['x'], mcs, ms, metric, method)
    lo, hi, w, core = model_forest(c, metric, ms)
    labels, stab = HR.cut(lo, hi, w, n, mcs, method)
    assert r.labels.dtype == torch.int64 and r.labels.device.type == 'cuda' and tuple(r.labels.shape) == (n,)
    assert np.array_equal(r.labels.cpu().numpy(), labels)
    assert r.stabilities.dtype == np.float64 and np.array_equal(r.stabilities, stab)
    assert r.n_clusters == stab.size and r.n_noise == int((labels < 0).sum())
    assert (r.min_cluster_size, r.min_samples, r.metric, r.method) == (mcs, ms, metric, method)
    assert r.n_dropped == 0 and 1 <= r.rounds <= rounds_bound(n) and same(r.core_dist.cpu().numpy(), core)
    assert HR.same_partition(labels, sklearn_labels(c[metric], mcs, ms, method))


def test_result_methods_recut_and_repeatability():
    from grl_amd import engine
    c = case()
    n, ids = 336, c['ids']
    r = engine.hdbscan(c['x'], 2, 1)
    # the planted clusters of 2 .. 130 samples come out, the two planted singletons are noise
    s = r.pair_scores(ids)
    assert (r.n_clusters, r.n_noise) == (7, 2) and s['ari'] == 1.0 and s['precision'] == 1.0 and s['recall'] == 1.0
    assert s == engine._pair_scores(r.labels, r.n_clusters, ids)
    cen, counts = r.centroids(c['x'])
    want_cen, want_counts = engine.cluster_centroids(c['x'], r.labels, r.n_clusters, 'unit')
    assert torch.equal(cen, want_cen) and torch.equal(counts, want_counts) and int(counts.sum()) == n - 2
    sil = r.silhouette(c['x'])
    want_sil = engine.silhouette(c['x'], r.labels, 'cosine', 'singleton')
    assert sil.metric == 'cosine' and sil.score == want_sil.score and torch.equal(sil.samples, want_sil.samples)
    assert engine.hdbscan(c['x'], 5, 2, 'euclidean').silhouette(c['x']).metric == 'euclidean'
    assert r.silhouette(c['x'], 'euclidean', 'drop').noise == 'drop'
    # min_samples = None means min_cluster_size
    a, b = engine.hdbscan(c['x'], 4), engine.hdbscan(c['x'], 4, 4)
    assert a.min_samples == 4 and torch.equal(a.labels, b.labels) and mst_equal(a.mst, b.mst)
    # the forest depends on min_samples only: another min_cluster_size or method is a cut of the same edges
    full = engine.hdbscan(c['x'], 10, 3, 'euclidean', 'leaf')
    base = engine.hdbscan(c['x'], 5, 3, 'euclidean')
    assert mst_equal(full.mst, base.mst)
    re = engine.hdbscan_from_mst(*base.mst, n, 10, 'leaf')
    assert torch.equal(re.labels, full.labels) and np.array_equal(re.stabilities, full.stabilities)
    assert (re.n_clusters, re.n_noise, re.core_dist, re.rounds) == (full.n_clusters, full.n_noise, None, None)
    perm = torch.randperm(base.mst[0].numel(), generator=torch.Generator().manual_seed(1)).to(DEV)
    re2 = engine.hdbscan_from_mst(*(t[perm] for t in base.mst), n, 10, 'leaf')       # any edge order: it is sorted first
    assert torch.equal(re2.labels, full.labels) and mst_equal(re2.mst, base.mst)
    lo, hi, w = base.mst
    with pytest.raises(ValueError, match='closes a cycle'):
        engine.hdbscan_from_mst(torch.cat((lo, lo[:1])), torch.cat((hi, hi[:1])), torch.cat((w, w[:1])), n, 5)
    with pytest.raises(ValueError, match='lo < hi < n'):
        engine.hdbscan_from_mst(hi, lo, w, n, 5)
    with pytest.raises(ValueError, match='lo < hi < n'):
        engine.hdbscan_from_mst(lo, hi, w, n - 1, 5)
    # two runs and every block width: the same bits
    for metric in ('cosine', 'euclidean'):
        ref = engine.hdbscan(c['x'], 5, 2, metric)
        for kw in ({},) + tuple({'block_cols': w} for w in WIDTHS) + ({'block_bytes': 1},):
            q = engine.hdbscan(c['x'], 5, 2, metric, **kw)
            assert torch.equal(q.labels, ref.labels) and mst_equal(q.mst, ref.mst), kw
            assert same(q.core_dist.cpu().numpy(), ref.core_dist.cpu().numpy()) and np.array_equal(q.stabilities, ref.stabilities)


def test_tiny_inputs_and_argument_errors_on_the_device():
    from grl_amd import engine
    c = case()
    x = c['x']
    for n in (0, 1):
        for r in (engine.hdbscan(x[:n]), engine.hdbscan(x[:n], 2, 1, 'euclidean', 'leaf'),
                  engine.hdbscan_matrix(torch.zeros((n, n), device=DEV))):
            assert r.labels.tolist() == [-1] * n and r.labels.dtype == torch.int64 and r.labels.device.type == 'cuda'
            assert (r.n_clusters, r.n_noise, r.rounds, r.n_dropped) == (0, n, 0, 0) and r.stabilities.size == 0
            assert r.mst[0].numel() == 0 and r.core_dist.tolist() == [0.0] * n
    r = engine.hdbscan(x[:2], 2, 1)                              # one edge; the one component is the root: all noise
    assert r.labels.tolist() == [-1, -1] and r.mst[0].tolist() == [0] and r.mst[1].tolist() == [1] and r.rounds == 1
    assert same(r.mst[2].cpu().numpy(), c['cosine'][:1, 1])
    r = engine.hdbscan(x[:2], 2, 2)
    assert same(r.core_dist.cpu().numpy(), c['cosine'][[0, 1], [1, 0]]) and r.mst[0].numel() == 1
    vm = engine.VerifyMetric.__new__(engine.VerifyMetric)
    with pytest.raises(ValueError, match='verify_metric'):
        engine.hdbscan(x, metric=vm)
    for bad in (1, True, 2.5):
        with pytest.raises(ValueError, match='min_cluster_size'):
            engine.hdbscan(x, bad)
    for bad in (0, 337, 1025, True, 1.0):
        with pytest.raises(ValueError, match='min_samples'):
            engine.hdbscan(x, 5, bad)
        with pytest.raises(ValueError, match='min_samples'):
            engine.mutual_reachability_mst(x, bad)
    with pytest.raises(ValueError, match='min_samples'):
        engine.hdbscan_matrix(dev(c['cosine'][:40, :40]), 5, 41)
    with pytest.raises(ValueError, match="'eom' or 'leaf'"):
        engine.hdbscan(x, method='best')
    with pytest.raises(ValueError, match="'cosine' or 'euclidean'"):
        engine.hdbscan(x, metric='jaccard')
    with pytest.raises(ValueError, match='no feature columns'):
        engine.hdbscan(torch.empty((4, 0), device=DEV), 2, 1)
    assert engine.hdbscan(x[:40], 5, 40).min_samples == 40      # min_samples = n is the limit


# ----------------------------------------------------------------------------
# 4. ATTEvaluator.evaluate with GRL_EVAL_HDBSCAN
# ----------------------------------------------------------------------------
KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_CLUSTER', 'GRL_EVAL_CLUSTER_JACCARD', 'GRL_EVAL_KMEANS', 'GRL_EVAL_SILHOUETTE', 'GRL_EVAL_HDBSCAN')


def test_attevaluator_adds_the_hdbscan_lines_and_json(synth_models, monkeypatch, tmp_path):
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
    gf = torch.cat((qf, gf), 0)
    pids = np.append(qp, gp)
    n = gf.size(0)
    path = str(tmp_path) + os.sep
    made = os.path.join(str(tmp_path), 'hdbscan.json')

    def run():
        if os.path.exists(made):
            os.remove(made)
        with contextlib.redirect_stdout(io.StringIO()) as o:
            r = ev.evaluate(None, None, q_loader, g_loader, path, 0, 0)
        return r, o.getvalue().splitlines(), open(made).read() if os.path.exists(made) else None

    def refuse(c):
        raise ValueError('not strict JSON: %s' % c)

    # unset: the lines of today, no file
    monkeypatch.setenv('GRL_EVAL_KMEANS', '3,5,1')
    r_off, text_off, raw_off = run()
    assert raw_off is None and not any('HDBSCAN' in l for l in text_off)
    # set: two lines after the k-means lines, everything else unchanged
    monkeypatch.setenv('GRL_EVAL_HDBSCAN', '2,1')
    r_on, text_on, raw = run()
    assert r_on == r_off and text_on[:-3] + text_on[-1:] == text_off
    hd = engine.hdbscan(gf, 2, 1)
    s = hd.pair_scores(pids)
    assert text_on[-3] == 'HDBSCAN: {} clusters ({} noise of {}) at min_cluster_size = 2, min_samples = 1, eom ({} rounds)'.format(
        hd.n_clusters, hd.n_noise, n, hd.rounds)
    assert text_on[-2] == 'Pairwise precision: {:.2%}  recall: {:.2%}  F1: {:.2%}  ARI: {:.4f}'.format(
        s['precision'], s['recall'], s['f1'], s['ari'])
    assert text_on[-5].startswith('K-means:')
    js = json.loads(raw, parse_constant=refuse)
    assert js == {'min_cluster_size': 2, 'min_samples': 1, 'method': 'eom', 'metric': 'cosine', 'n': n,
                  'n_clusters': hd.n_clusters, 'n_noise': hd.n_noise, 'n_edges': int(hd.mst[0].numel()),
                  'rounds': hd.rounds, 'n_dropped': 0, 'stabilities': hd.stabilities.tolist(), 'pair_scores': s,
                  'labels': hd.labels.cpu().tolist()}
    # alone, on the streaming route, with the silhouette line as the third
    monkeypatch.delenv('GRL_EVAL_KMEANS')
    monkeypatch.setenv('GRL_EVAL_STREAM', '1')
    monkeypatch.setenv('GRL_EVAL_HDBSCAN', '2,2,leaf')
    monkeypatch.setenv('GRL_EVAL_SILHOUETTE', 'euclidean')
    _, text, raw = run()
    hd = engine.hdbscan(gf, 2, 2, 'cosine', 'leaf')
    assert text[-4].startswith('HDBSCAN: {} clusters ({} noise of {}) at min_cluster_size = 2, min_samples = 2, leaf'.format(
        hd.n_clusters, hd.n_noise, n))
    assert text[-3].startswith('Pairwise precision') and text[-2].startswith('Silhouette (euclidean): ')
    js = json.loads(raw, parse_constant=refuse)
    assert js['labels'] == hd.labels.cpu().tolist() and js['method'] == 'leaf'
    assert js['silhouette']['metric'] == 'euclidean' and js['silhouette']['noise'] == 'singleton'
    if hd.n_clusters + hd.n_noise >= 2:
        assert js['silhouette']['score'] == hd.silhouette(gf, 'euclidean').score
    # refused with the verification metric
    monkeypatch.setenv('GRL_EVAL_METRIC', 'verify')
    with pytest.raises(ValueError, match='GRL_EVAL_HDBSCAN cannot be combined'):
        ev.evaluate(None, None, q_loader, g_loader, path, 0, 0)
