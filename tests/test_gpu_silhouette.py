"""Silhouette coefficients on the device (engine.silhouette / silhouette_matrix / cluster_select, silhouette.hip,
DESIGN.md 4w) against the numpy model of tests/silhouette_ref.py.  Every sum has a prescribed fp32 order, so the device's
samples, a and b are compared bit for bit with the model run on the read-back device distances (the outputs of
cosin_dist / grl_row_sqnorm and pairwise_distance_tensor); only the comparisons with scikit-learn and with a float64
evaluation carry a bound, the one derived in tests/test_silhouette_cpu.py."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import silhouette_ref as SR

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
U = 2.0 ** -24
WIDTHS = (1, 7, 64, 100, 336)

_cache = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    """bit patterns equal, any NaN equal to any NaN"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_distances(x):
    """(cosine distances by the contract's chain, euclidean distances) as float32 host matrices, both from what the
    device computes for the rows ``x`` (zero-padded to the GEMM's multiple of 32 features, as the engine pads them)."""
    from grl_amd import engine
    xp = engine._pad_features(x)
    n, d = xp.shape
    sq = torch.empty(n, dtype=torch.float32, device=DEV)
    engine._call('grl_row_sqnorm', engine.ptr(xp), engine.ptr(sq), n, d, d)
    negdot = engine.cosin_dist(xp, xp).cpu().numpy()
    return SR.cosine_matrix(negdot, sq.cpu().numpy()), engine.pairwise_distance_tensor(xp, xp).cpu().numpy()


def case(d=24):
    """The planted input of the CPU test (336 samples in clusters of 1, 1, 2, 3, 63, 64, 65, 130, 7, norms 0.5 .. 1.8,
    shuffled) in d = 24 or d = 5 features, its device distances, labels with 15 noise samples, and 'mixed' labels: ids
    with gaps, the cluster of 63 broken into 63 clusters of one in the middle of the member order (a run that crosses
    a 64-position chunk edge), and every fifth sample of the cluster of 130 noise.  Built once."""
    if d not in _cache:
        x, ids = SR.planted(d=d)
        lab = ids.copy()
        noise = np.flatnonzero(ids == 7)[::9]
        lab[noise] = -1 - np.arange(noise.size) % 3
        mixed = ids * 100
        four = np.flatnonzero(ids == 4)
        mixed[four] = 400 + np.arange(four.size)
        mixed[np.flatnonzero(ids == 7)[::5]] = -1
        xd = dev(x)
        cos, euc = device_distances(xd)
        _cache[d] = {'x': xd, 'host': x, 'ids': ids, 'noisy': lab, 'mixed': mixed, 'cosine': cos, 'euclidean': euc}
    return _cache[d]


def check(r, model, n, metric, noise):
    s, a, b, scored = model
    assert r.samples.dtype == r.a.dtype == r.b.dtype == torch.float32 and r.scored.dtype == torch.bool
    assert tuple(r.samples.shape) == tuple(r.a.shape) == tuple(r.b.shape) == tuple(r.scored.shape) == (n,)
    assert same(r.samples.cpu().numpy(), s) and same(r.a.cpu().numpy(), a) and same(r.b.cpu().numpy(), b)
    assert np.array_equal(r.scored.cpu().numpy(), scored) and r.n_scored == int(scored.sum())
    want = SR.score(s, scored)
    assert (np.isnan(r.score) and np.isnan(want)) or r.score == want
    assert isinstance(r.score, float) and r.metric == metric and r.noise == noise


def equal(r, q):
    return (same(r.samples.cpu().numpy(), q.samples.cpu().numpy()) and same(r.a.cpu().numpy(), q.a.cpu().numpy())
            and same(r.b.cpu().numpy(), q.b.cpu().numpy()) and torch.equal(r.scored, q.scored)
            and (r.score == q.score or (np.isnan(r.score) and np.isnan(q.score)))
            and (r.n_scored, r.n_clusters) == (q.n_scored, q.n_clusters))


# ----------------------------------------------------------------------------
# 1. bit for bit against the model on the device's own distances
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('d', [24, 5])
@pytest.mark.parametrize('noise', ['singleton', 'drop'])
@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_samples_equal_the_model_on_the_device_distances(metric, noise, d):
    from grl_amd import engine
    c = case(d)
    n = c['host'].shape[0]
    for lab in (c['ids'], c['mixed'], c['noisy']):
        r = engine.silhouette(c['x'], dev(lab), metric, noise)
        check(r, SR.samples(c[metric], lab, noise), n, metric, noise)
        k = np.unique(lab[lab >= 0]).size + (int((lab < 0).sum()) if noise == 'singleton' else 0)
        assert r.n_clusters == k
    assert r.n_scored == (n if noise == 'singleton' else n - 15)
    s = r.samples.cpu().numpy()
    assert (s[c['noisy'] < 0] == 0).all() and np.isfinite(s).all() and np.abs(s).max() <= 1
    # int32 labels and labels with unused ids between them give the same bits
    assert equal(r, engine.silhouette(c['x'], dev(c['noisy'].astype(np.int32)), metric, noise))
    gap = np.where(c['noisy'] >= 0, 3 * c['noisy'] + 2, c['noisy'])
    q = engine.silhouette(c['x'], dev(gap), metric, noise)
    assert same(q.samples.cpu().numpy(), s) and q.n_clusters == r.n_clusters


@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_same_bits_for_every_block_width_and_on_a_second_run(metric):
    """Widths 1 and 7 cut inside every 64-position chunk, 64 on the chunk edges, 100 leaves the clusters of 63 .. 130
    members straddling a block edge at positions that are no multiple of 64, 336 is one block."""
    from grl_amd import engine
    c = case()
    for noise, lab in (('singleton', c['noisy']), ('drop', c['noisy']), ('singleton', c['ids']),
                       ('singleton', c['mixed']), ('drop', c['mixed'])):
        labd = dev(lab)
        ref = engine.silhouette(c['x'], labd, metric, noise)
        assert equal(ref, engine.silhouette(c['x'], labd, metric, noise))
        for w in WIDTHS:
            assert equal(ref, engine.silhouette(c['x'], labd, metric, noise, block_cols=w)), (noise, w)
        assert equal(ref, engine.silhouette(c['x'], labd, metric, noise, block_bytes=1))      # the floor of 256 columns


# ----------------------------------------------------------------------------
# 2. the matrix form
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_silhouette_equals_silhouette_matrix_of_the_corresponding_matrix(metric):
    from grl_amd import engine
    c = case()
    n = c['host'].shape[0]
    m = dev(c[metric])                          # 'cosine': the stated chain on cosin_dist and grl_row_sqnorm
    wide = torch.full((n, n + 13), float('nan'), dtype=torch.float32, device=DEV)
    wide[:, 5:5 + n] = m
    for noise in ('singleton', 'drop'):
        labd = dev(c['noisy'])
        ref = engine.silhouette(c['x'], labd, metric, noise)
        got = engine.silhouette_matrix(m, labd, noise)
        assert got.metric == 'precomputed' and got.noise == noise
        assert same(got.samples.cpu().numpy(), ref.samples.cpu().numpy()) and got.score == ref.score
        assert same(got.a.cpu().numpy(), ref.a.cpu().numpy()) and same(got.b.cpu().numpy(), ref.b.cpu().numpy())
        strided = wide[:, 5:5 + n]
        assert strided.stride(0) == n + 13 and not strided.is_contiguous()
        for w in (None, 7, 100):
            assert equal(got, engine.silhouette_matrix(strided, labd, noise, block_cols=w)), w
    # used as given: an asymmetric matrix, the diagonal never read
    g = np.random.Generator(np.random.PCG64(4))
    a = g.uniform(0.0, 3.0, (n, n)).astype(np.float32)
    np.fill_diagonal(a, np.nan)
    r = engine.silhouette_matrix(dev(a), dev(c['ids']))
    check(r, SR.samples(a, c['ids']), n, 'precomputed', 'singleton')
    assert np.isfinite(r.score)
    with pytest.raises(ValueError, match='square'):
        engine.silhouette_matrix(dev(a)[:, :n - 1], dev(c['ids']))
    with pytest.raises(ValueError, match='float32'):
        engine.silhouette_matrix(dev(a).double(), dev(c['ids']))


# ----------------------------------------------------------------------------
# 3. against scikit-learn and a float64 evaluation
# ----------------------------------------------------------------------------
def test_cosine_is_within_the_arithmetic_bound_of_sklearn_end_to_end():
    skm = pytest.importorskip('sklearn.metrics')
    from grl_amd import engine
    c = case()
    x64 = c['host'].astype(np.float64)
    xn = x64 / np.linalg.norm(x64, axis=1, keepdims=True)
    ref = np.clip(1.0 - xn @ xn.T, 0.0, None)
    np.fill_diagonal(ref, 0.0)
    ids = c['ids']
    want = skm.silhouette_samples(ref, ids, metric='precomputed')
    _, a, b, _ = SR.samples64(ref, ids)
    mx = np.maximum(a, b)
    multi = np.bincount(ids)[ids] > 1
    assert mx[multi].min() >= 0.05
    delta = (c['host'].shape[1] + 6) * U + (int(np.bincount(ids).max()) + 2) * U * float(ref.max())
    lim = 2.0 * (delta + delta) / np.maximum(mx, 1e-300)
    r = engine.silhouette(c['x'], dev(ids), 'cosine')
    err = np.abs(r.samples.cpu().numpy().astype(np.float64) - want)
    print('largest bound = %.3g, largest difference = %.3g' % (lim[multi].max(), err.max()))
    assert (err[multi] <= lim[multi]).all() and (err[~multi] == 0).all()
    assert abs(r.score - skm.silhouette_score(ref, ids, metric='precomputed')) <= lim[multi].max()


def test_euclidean_is_within_the_summation_bound_of_a_float64_evaluation_of_the_device_matrix():
    """The reference is the float64 evaluation of the device's own fp32 matrix, so the cancellation inside the distance
    stays out: a mean of m distances is within (m + 2) u D_max (m - 1 adds, one division)."""
    from grl_amd import engine
    c = case()
    ids = c['ids']
    want, a, b, _ = SR.samples64(c['euclidean'], ids)
    mx = np.maximum(a, b)
    multi = np.bincount(ids)[ids] > 1
    assert mx[multi].min() >= 0.05
    delta = (int(np.bincount(ids).max()) + 2) * U * float(c['euclidean'].max())
    lim = 2.0 * (delta + delta) / np.maximum(mx, 1e-300)
    r = engine.silhouette(c['x'], dev(ids), 'euclidean')
    err = np.abs(r.samples.cpu().numpy().astype(np.float64) - want)
    print('largest bound = %.3g, largest difference = %.3g' % (lim[multi].max(), err.max()))
    assert (err[multi] <= lim[multi]).all() and (err[~multi] == 0).all()


# ----------------------------------------------------------------------------
# 4. NaN, single clusters
# ----------------------------------------------------------------------------
def test_nan_rows_and_too_few_clusters():
    from grl_amd import engine
    c = case()
    n = c['host'].shape[0]
    ids = c['ids']
    bad = int(np.flatnonzero(ids == 6)[3])                       # a member of the cluster of 65
    x = c['host'].copy()
    x[bad, 2] = np.nan
    xd = dev(x)
    cos, _ = device_distances(xd)
    assert np.isnan(cos[bad]).all() and np.isnan(cos[:, bad]).all() and np.isnan(cos).sum() == 2 * n - 1
    multi = np.bincount(ids)[ids] > 1
    # inside a cluster: its members get a NaN a, everybody else a NaN candidate for b; clusters of one still score 0
    r = engine.silhouette(xd, dev(ids), 'cosine')
    check(r, SR.samples(cos, ids), n, 'cosine', 'singleton')
    s = r.samples.cpu().numpy()
    assert np.isnan(s[multi]).all() and (s[~multi] == 0).all() and np.isnan(r.score) and r.n_scored == n
    # dropped as noise: neither a row nor a column, and nobody else is affected
    lab = ids.copy()
    lab[bad] = -1
    r = engine.silhouette(xd, dev(lab), 'cosine', 'drop')
    check(r, SR.samples(cos, lab, 'drop'), n, 'cosine', 'drop')
    s = r.samples.cpu().numpy()
    keep = np.arange(n) != bad
    clean = engine.silhouette(dev(c['host'][keep]), dev(ids[keep]), 'cosine')
    assert same(s[keep], clean.samples.cpu().numpy()) and s[bad] == 0 and not bool(r.scored[bad])
    assert np.isfinite(r.score) and r.score == clean.score and r.n_scored == n - 1
    # as a singleton it scores 0 itself and is a NaN candidate for everybody else's b
    r = engine.silhouette(xd, dev(lab), 'cosine', 'singleton')
    check(r, SR.samples(cos, lab, 'singleton'), n, 'cosine', 'singleton')
    s = r.samples.cpu().numpy()
    assert s[bad] == 0 and np.isnan(s[multi & keep]).all() and np.isnan(r.score)
    # fewer than two clusters among the scored samples
    one = torch.zeros(n, dtype=torch.int64, device=DEV)
    for args in ((one,), (one, 'euclidean'), (one - 1, 'cosine', 'drop'), (torch.where(dev(ids) == 7, 0, -1), 'cosine', 'drop')):
        with pytest.raises(ValueError, match='fewer than 2 clusters'):
            engine.silhouette(c['x'], *args)
    with pytest.raises(ValueError, match='fewer than 2 clusters'):
        engine.silhouette_matrix(dev(c['cosine']), one)
    r = engine.silhouette(c['x'], one - 1)                       # all noise as singletons: n clusters, every score 0
    check(r, SR.samples(c['cosine'], np.full(n, -1)), n, 'cosine', 'singleton')
    assert r.n_clusters == n and r.score == 0.0 and float(r.b.min()) > 0
    with pytest.raises(ValueError, match='no feature columns'):
        engine.silhouette(torch.empty((n, 0), device=DEV), dev(ids))


# ----------------------------------------------------------------------------
# 5. the result methods and the selection of eps
# ----------------------------------------------------------------------------
def select_input():
    if 'sel' not in _cache:
        x, ids = SR.select_case()
        _cache['sel'] = (dev(x), ids)
    return _cache['sel']


def test_result_methods_score_the_labels_of_cluster_and_kmeans():
    from grl_amd import engine
    x, ids = select_input()
    cl = engine.cluster(x, SR.SELECT_EPS[1], 2)
    assert cl.n_clusters == 4
    for args in ((), ('euclidean',), ('cosine', 'drop')):
        assert equal(cl.silhouette(x, *args), engine.silhouette(x, cl.labels, *args))
    assert cl.silhouette(x).noise == 'singleton' and cl.silhouette(x).metric == 'cosine'
    first = [int(np.flatnonzero(ids == j)[0]) for j in range(4)]
    for metric in ('cosine', 'euclidean'):
        km = engine.kmeans(x, 4, metric, init=first, max_iter=20)
        r = km.silhouette(x)
        assert r.metric == metric and equal(r, engine.silhouette(x, km.labels, metric))
        other = 'euclidean' if metric == 'cosine' else 'cosine'
        assert km.silhouette(x, other).metric == other
        assert r.score > 0.5 and r.n_clusters == 4 and r.n_scored == ids.size


def test_cluster_select_picks_the_middle_eps_of_too_tight_right_too_loose():
    from grl_amd import engine
    x, ids = select_input()
    best, rows = engine.cluster_select(x, SR.SELECT_EPS)
    assert [r['eps'] for r in rows] == [float(np.float32(e)) for e in SR.SELECT_EPS]
    assert best.eps == rows[1]['eps'] and best.n_clusters == 4 and best.pair_scores(ids)['ari'] == 1.0
    assert rows[0]['n_clusters'] > 40 and rows[1]['n_clusters'] == 4 and rows[2]['n_clusters'] == 3
    assert rows[1]['score'] > rows[0]['score'] and rows[1]['score'] > rows[2]['score']
    for r in rows:
        cl = engine.cluster(x, r['eps'])
        assert (r['n_clusters'], r['n_noise']) == (cl.n_clusters, cl.n_noise) and r['score'] == cl.silhouette(x).score
    # min_samples = 2 sheds the tight eps' loners as noise; scored as singletons they still count for 0
    best2, rows2 = engine.cluster_select(x, SR.SELECT_EPS, min_samples=2, score_metric='euclidean')
    loners = int((torch.bincount(engine.cluster(x, SR.SELECT_EPS[0]).labels) == 1).sum())
    assert best2.eps == rows2[1]['eps'] and rows2[0]['n_noise'] == loners > 20
    assert rows2[0]['score'] == engine.silhouette(x, engine.cluster(x, SR.SELECT_EPS[0], 2).labels, 'euclidean').score
    # one cluster has no score; ties go to the smaller eps
    best3, rows3 = engine.cluster_select(x, (0.9, -0.7, SR.SELECT_EPS[1]))
    assert rows3[0]['score'] is None and rows3[0]['n_clusters'] == 1
    assert rows3[1]['score'] == rows3[2]['score'] and best3.eps == rows3[2]['eps']
    with pytest.raises(ValueError, match='no eps'):
        engine.cluster_select(x, (0.9,))


# ----------------------------------------------------------------------------
# 6. ATTEvaluator.evaluate with GRL_EVAL_SILHOUETTE
# ----------------------------------------------------------------------------
KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_CLUSTER', 'GRL_EVAL_CLUSTER_JACCARD', 'GRL_EVAL_KMEANS', 'GRL_EVAL_SILHOUETTE')


def test_attevaluator_adds_the_silhouette_line_and_json_entry(synth_models, monkeypatch, tmp_path):
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
    n = gf.size(0)
    path = str(tmp_path) + os.sep

    def run(files):
        for f in files:
            if os.path.exists(os.path.join(str(tmp_path), f)):
                os.remove(os.path.join(str(tmp_path), f))
        with contextlib.redirect_stdout(io.StringIO()) as o:
            r = ev.evaluate(None, None, q_loader, g_loader, path, 0, 0)
        return r, o.getvalue().splitlines(), [open(os.path.join(str(tmp_path), f)).read() for f in files]

    def refuse(c):
        raise ValueError('not strict JSON: %s' % c)

    def line(r, metric):
        return 'Silhouette ({}): {:.4f} over {} of {} samples, {} clusters'.format(metric, r.score, r.n_scored, n,
                                                                                   r.n_clusters)

    # k-means: the third line comes last, the JSON gains one key, everything else is what it is without the knob
    monkeypatch.setenv('GRL_EVAL_KMEANS', '3,5,1')
    r_off, text_off, (raw_off,) = run(['kmeans.json'])
    assert not any('Silhouette' in l for l in text_off) and 'silhouette' not in json.loads(raw_off)
    monkeypatch.setenv('GRL_EVAL_SILHOUETTE', '1')
    r_on, text_on, (raw_on,) = run(['kmeans.json'])
    assert r_on == r_off
    km = engine.kmeans(gf, 3, 'cosine', 'random', 1, 5)
    want = km.silhouette(gf, 'cosine')
    assert text_on[-2] == line(want, 'cosine') and text_on[:-2] + text_on[-1:] == text_off
    js = json.loads(raw_on, parse_constant=refuse)
    assert js.pop('silhouette') == {'metric': 'cosine', 'noise': 'singleton', 'score': want.score,
                                    'n_scored': want.n_scored, 'n_clusters': want.n_clusters}
    assert js == json.loads(raw_off) and list(js) == list(json.loads(raw_off))
    # DBSCAN and k-means together, streaming route, euclidean and 'drop': one line after each report
    monkeypatch.setenv('GRL_EVAL_STREAM', '1')
    monkeypatch.setenv('GRL_EVAL_CLUSTER', '-0.9,2')
    monkeypatch.setenv('GRL_EVAL_SILHOUETTE', 'euclidean,drop')
    _, text, (raw_c, raw_k) = run(['clusters.json', 'kmeans.json'])
    assert [l.split(':')[0].split(' (')[0] for l in text[-7:-1]] == ['Clusters', 'Pairwise precision', 'Silhouette',
                                                                       'K-means', 'Pairwise precision', 'Silhouette']
    cl = engine.cluster(gf, -0.9, 2)
    jc = json.loads(raw_c, parse_constant=refuse)['silhouette']
    if cl.n_clusters >= 2:
        want = cl.silhouette(gf, 'euclidean', 'drop')
        assert text[-5] == line(want, 'euclidean') and want.n_scored == n - cl.n_noise
        assert jc == {'metric': 'euclidean', 'noise': 'drop', 'score': want.score, 'n_scored': want.n_scored,
                      'n_clusters': want.n_clusters}
    else:
        assert text[-5] == 'Silhouette (euclidean): undefined, fewer than 2 clusters' and jc['score'] is None
    assert text[-2] == line(km.silhouette(gf, 'euclidean'), 'euclidean')
    assert json.loads(raw_k, parse_constant=refuse)['silhouette']['noise'] == 'drop'
    # alone it is refused
    monkeypatch.delenv('GRL_EVAL_CLUSTER')
    monkeypatch.delenv('GRL_EVAL_KMEANS')
    with pytest.raises(ValueError, match='GRL_EVAL_CLUSTER_JACCARD'):
        ev.evaluate(None, None, q_loader, g_loader, path, 0, 0)
