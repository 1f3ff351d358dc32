"""k-means and cluster centroids on the device (engine.kmeans / kmeans_assign / cluster_centroids, kmeans.hip, DESIGN.md
4t) against the numpy model of tests/kmeans_ref.py.  Labels and counts are integers derived from the bits of the
materialised distance matrix, and the 'sum' / 'mean' centroids follow a fixed fp32 order, so those comparisons are
exact (bit patterns); 'unit' goes through grl_row_sqnorm's own summation order and is compared within
(d + 4) * 2^-24 relative per element of the float64 normalisation of the exact sums (fp32 norm accumulation over d
terms, one sqrt, one reciprocal, one multiply)."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import kmeans_ref as KR

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
N, DIM = 301, 64
SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 64, 65, 257)         # straddle the four-way split and the wave width
U = 2.0 ** -24

_cache = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def feature_case():
    """301 unit rows: 10 centres in a 3-d latent, 241 points at centre + 0.12 N(0, 1), 60 background points; the latent
    sits in feature columns 0, 21, 42 of 64.  Built once, never modified."""
    if 'x' not in _cache:
        g = np.random.Generator(np.random.PCG64(31))
        centres = g.standard_normal((10, 3))
        lat = np.concatenate((centres[g.integers(0, 10, 241)] + 0.12 * g.standard_normal((241, 3)),
                              g.standard_normal((60, 3))))
        x = np.zeros((N, DIM), dtype=np.float32)
        x[:, [0, 21, 42]] = lat.astype(np.float32)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        _cache['x'] = torch.from_numpy(x[g.permutation(N)]).to(DEV)
    return _cache['x']


def special_case():
    """Unit rows with one NaN row (5), one all-zero row (11) and three rows (17, 18 = -2 x 17, 19 = 2 x 17) whose
    products with each other overflow."""
    if 's' not in _cache:
        g = np.random.Generator(np.random.PCG64(21))
        x = g.standard_normal((N, DIM)).astype(np.float32)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        x[5, 3] = np.nan
        x[11] = 0.0
        x[17] *= np.float32(1.5e19)
        x[18] = -x[17] * np.float32(2.0)
        x[19] = x[17] * np.float32(2.0)
        _cache['s'] = torch.from_numpy(x).to(DEV)
    return _cache['s']


def planted_case():
    """300 unit rows around 10 well-separated directions (orthogonal axes of 64), shuffled; (x, planted ids)."""
    if 'p' not in _cache:
        g = np.random.Generator(np.random.PCG64(77))
        ids = np.repeat(np.arange(10), 30)
        x = 0.05 * g.standard_normal((300, DIM))
        x[np.arange(300), 5 * ids + 2] += 1.0
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        perm = g.permutation(300)
        _cache['p'] = (torch.from_numpy(x[perm].astype(np.float32)).to(DEV), ids[perm])
    return _cache['p']


def dev_matrix(x, metric):
    from grl_amd import engine
    fn = engine.cosin_dist if metric == 'cosine' else engine.pairwise_distance_tensor
    return lambda c: fn(x, c if torch.is_tensor(c) else torch.from_numpy(np.ascontiguousarray(c)).to(DEV)).cpu().numpy()


def unit_close(got, sums, d, what):
    """got [d] against the float64 normalisation of the exact sums, (d + 4) * 2^-24 relative per element"""
    s = sums.astype(np.float64)
    want = s / np.sqrt((s * s).sum())
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= (d + 4) * U * np.abs(want)).all(), (what, float((err / np.maximum(np.abs(want), 1e-300)).max() / U))


# ----------------------------------------------------------------------------
# 1. the segmented row sum at its edges
# ----------------------------------------------------------------------------
def rowsum_case(d, unaligned):
    """(x device [n, d], host copy, labels): clusters of SIZES[j] members, 20 samples nobody's, shuffled so that the
    members interleave.  ``unaligned``: x is a view one float into a buffer, so its pointer is 4 mod 16."""
    key = ('rs', d, unaligned)
    if key not in _cache:
        g = np.random.Generator(np.random.PCG64(100 + d))
        labels = np.concatenate([np.full(s, j) for j, s in enumerate(SIZES)] + [np.full(20, -1)])
        labels = labels[g.permutation(labels.size)]
        n = labels.size
        x = (g.standard_normal((n, d)) * g.uniform(1e-3, 1e3, (n, 1))).astype(np.float32)
        x[3, 1] = -0.0
        if unaligned:
            flat = torch.zeros(n * d + 5, dtype=torch.float32, device=DEV)
            xd = flat[1:1 + n * d].view(n, d)
            xd.copy_(torch.from_numpy(x))
            assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
        else:
            xd = torch.from_numpy(x).to(DEV)
            assert xd.data_ptr() % 16 == 0
        _cache[key] = (xd, x, labels)
    return _cache[key]


@pytest.mark.parametrize('d,unaligned', [(64, False), (70, False), (260, False), (64, True), (260, True)])
def test_segment_rowsum_equals_the_model_bit_for_bit(d, unaligned):
    from grl_amd import engine
    xd, x, labels = rowsum_case(d, unaligned)
    k = len(SIZES)
    lab = torch.from_numpy(labels).to(DEV)
    assert (labels < 0).sum() == 20 and not (np.diff(np.flatnonzero(labels == 11)) == 1).all()   # interleaved
    g = np.random.Generator(np.random.PCG64(9))
    prev = g.standard_normal((k, d)).astype(np.float32)
    prev_d = torch.from_numpy(prev).to(DEV)
    want_sum, want_counts = KR.segment_sum(x, labels, k)
    assert want_counts.tolist() == list(SIZES)
    for reduce in ('sum', 'mean', 'unit'):
        for p, pd in ((None, None), (prev, prev_d)):
            got, counts = engine.cluster_centroids(xd, lab, k, reduce, pd)
            again, counts2 = engine.cluster_centroids(xd, lab, k, reduce, pd)
            assert got.dtype == torch.float32 and tuple(got.shape) == (k, d) and counts.dtype == torch.int64
            assert counts.cpu().tolist() == list(SIZES) == counts2.cpu().tolist()
            got, again = got.cpu().numpy(), again.cpu().numpy()
            assert np.array_equal(bits(got), bits(again)), (reduce, 'two calls')
            want, _, n_empty = KR.centroids(x, labels, k, reduce, p)
            assert n_empty == 1
            assert np.array_equal(bits(got[0]), bits(prev[0] if p is not None else np.zeros(d))), (reduce, 'empty row')
            if reduce == 'unit':
                for j in range(1, k):
                    unit_close(got[j], want_sum[j], d, (d, unaligned, j))
            else:
                assert np.array_equal(bits(got), bits(want)), (reduce, d, unaligned)
    # k defaults to max(label) + 1; int32 labels give the same bits
    got, counts = engine.cluster_centroids(xd, lab.to(torch.int32), reduce='sum')
    assert tuple(got.shape) == (k, d) and np.array_equal(bits(got.cpu().numpy()), bits(want_sum))
    assert counts.cpu().tolist() == list(SIZES)


def test_cluster_centroids_argument_checks_and_unusable_norms():
    from grl_amd import engine
    xd, x, labels = rowsum_case(64, False)
    lab = torch.from_numpy(labels).to(DEV)
    with pytest.raises(ValueError, match='label 11 is outside 0..k-1 = 0..10'):
        engine.cluster_centroids(xd, lab, 11)
    with pytest.raises(ValueError, match="reduce must be 'sum', 'mean' or 'unit'"):
        engine.cluster_centroids(xd, lab, 12, 'median')
    with pytest.raises(ValueError, match='integer device tensor'):
        engine.cluster_centroids(xd, lab.float(), 12)
    with pytest.raises(ValueError, match='integer device tensor'):
        engine.cluster_centroids(xd, lab[:-1], 12)
    with pytest.raises(ValueError, match='prev must be'):
        engine.cluster_centroids(xd, lab, 12, prev=xd[:11])
    # more clusters than labels name: the tail is empty; all labels negative: k = 0
    got, counts = engine.cluster_centroids(xd, lab, 15, 'mean')
    assert counts.cpu().tolist() == list(SIZES) + [0, 0, 0] and not got[12:].any()
    got, counts = engine.cluster_centroids(xd, torch.full_like(lab, -3))
    assert tuple(got.shape) == (0, 64) and counts.numel() == 0
    # 'unit': a sum that is zero, NaN or overflows is empty and keeps prev (the model's rules, tests/test_kmeans_cpu.py)
    h = np.zeros((8, 4), dtype=np.float32)
    h[:, :2] = [[3, 4], [1, 0], [-1, 0], [np.nan, 1], [1e30, 1e30], [1e30, 1e30], [2, 0], [5, 5]]
    hl = np.array([0, 1, 1, 2, 3, 3, 5, -1])
    prev = np.arange(24, dtype=np.float32).reshape(6, 4) + 100
    got, counts = engine.cluster_centroids(torch.from_numpy(h).to(DEV), torch.from_numpy(hl).to(DEV), 6, 'unit',
                                           torch.from_numpy(prev).to(DEV))
    got = got.cpu().numpy()
    assert counts.cpu().tolist() == [1, 2, 1, 2, 0, 1]
    for j in (1, 2, 3, 4):
        assert np.array_equal(got[j], prev[j]), j
    assert got[5].tolist() == [1, 0, 0, 0]
    unit_close(got[0, :2], h[0, :2], 4, 'unit 3-4-5')


# ----------------------------------------------------------------------------
# 2. assign
# ----------------------------------------------------------------------------
def assign_centroids(x):
    """37 centroids from the rows of x: 20 duplicates 5 (ties), 9 carries a NaN, 12 is the all-zero row"""
    c = x[torch.arange(0, 37 * 8, 8, device=DEV)].clone()
    c[20] = c[5]
    c[9, 7] = float('nan')
    c[12] = x[11]
    return c.contiguous()


@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
@pytest.mark.parametrize('which', ['feature', 'special'])
def test_kmeans_assign_equals_search_and_the_model_on_the_materialised_matrix(metric, which):
    from grl_amd import engine
    x = feature_case() if which == 'feature' else special_case()
    c = assign_centroids(x)
    k = c.shape[0]
    D = dev_matrix(x, metric)(c)
    want_lab, want_best = KR.assign(D)
    assert (want_lab != 20).all() and (metric != 'cosine' or (want_lab == 5).any())      # the duplicate loses every tie
    # a NaN distance is never the best of a row that holds a number, and a row of nothing but NaN is unassigned
    nan = np.isnan(D)
    rows = np.flatnonzero(~nan.all(1))
    assert not nan[rows, want_lab[rows]].any() and np.array_equal(want_lab < 0, nan.all(1))
    if metric == 'cosine':                                       # -dot keeps a NaN: the NaN centroid attracts nobody,
        assert nan[:, 9].all() and (want_lab != 9).all()         # the NaN sample belongs to nobody
        assert which != 'special' or (nan[5].all() and want_lab[5] == -1 and want_lab[11] >= 0)
    else:       # pairwise_distance_tensor clamps d^2 at 1e-12 and the clamp drops a NaN: such an entry is the number
        assert not nan[:, 9].any() and (D[:, 9] < 1e-5).all()    # sqrt(1e-12), which search ranks as it stands
    for width in (None, 7, 64, k):
        lab, dist = engine.kmeans_assign(x, c, metric, block_cols=width)
        assert lab.dtype == torch.int64 and dist.dtype == torch.float32 and lab.is_cuda and tuple(lab.shape) == (N,)
        sd, si = engine.search(x, c, 1, metric, block_cols=width)
        lab, dist, sd, si = lab.cpu().numpy(), dist.cpu().numpy(), sd.cpu().numpy()[:, 0], si.cpu().numpy()[:, 0]
        assert np.array_equal(bits(dist), bits(sd)), (metric, width)
        assert np.array_equal(lab, np.where(np.isnan(sd), -1, si)), (metric, width)
        assert np.array_equal(lab, want_lab), (metric, width)
        assert np.array_equal(bits(dist)[want_lab >= 0], bits(want_best)[want_lab >= 0]), (metric, width)
        assert np.isnan(dist[want_lab < 0]).all()
    lab2, _ = engine.kmeans_assign(x, c, metric, block_bytes=4 * N * 16)
    assert np.array_equal(lab2.cpu().numpy(), want_lab)


def test_kmeans_refuses_what_cluster_refuses_and_bad_arguments():
    from grl_amd import engine
    x = feature_case()
    vm = engine.VerifyMetric.__new__(engine.VerifyMetric)
    with pytest.raises(ValueError, match='verify_metric'):
        engine.kmeans(x, 3, vm)
    for k in (0, N + 1, 2.0, True):
        with pytest.raises(ValueError, match='kmeans: k must be'):
            engine.kmeans(x, k)
    for it in (0, -1, 1.5):
        with pytest.raises(ValueError, match='max_iter must be an integer >= 1'):
            engine.kmeans(x, 3, max_iter=it)
    for init in ('kmeans++', [0, 1], [0, 1, 1], [0, 1, N], [0, -1, 2], [0.0, 1.0, 2.0], x[:4], x[:3, :5]):
        with pytest.raises(ValueError, match='kmeans: init'):
            engine.kmeans(x, 3, init=init)
    with pytest.raises(ValueError, match='seed'):
        engine.kmeans(x, 3, seed=-1)
    with pytest.raises(ValueError, match='at least one centroid'):
        engine.kmeans_assign(x, x[:0])
    # 'random' is numpy's PCG64 choice, then rows
    want = np.random.Generator(np.random.PCG64(7)).choice(N, 3, replace=False)
    a = engine.kmeans(x, 3, init='random', seed=7, max_iter=1)
    b = engine.kmeans(x, 3, init=want.tolist(), max_iter=1)
    c = engine.kmeans(x, 3, init=x[torch.from_numpy(want).to(DEV)], max_iter=1)
    for r in (b, c):
        assert torch.equal(a.labels, r.labels) and torch.equal(a.centroids, r.centroids)


# ----------------------------------------------------------------------------
# 3. one step
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_one_step_equals_model_assign_and_update(metric):
    from grl_amd import engine
    x = feature_case()
    xh = x.cpu().numpy()
    k = 12
    c0 = x[torch.arange(0, 12 * 25, 25, device=DEV)].clone()
    c0[7] = c0[2]                                                # loses every tie to 2: attracts nothing
    c0h = c0.cpu().numpy()
    got = engine.kmeans(x, k, metric, init=c0, max_iter=1)
    assert np.array_equal(bits(c0.cpu().numpy()), bits(c0h))     # the caller's tensor is not written
    lab, best = KR.assign(dev_matrix(x, metric)(c0))
    reduce = 'unit' if metric == 'cosine' else 'mean'
    want, counts, n_empty = KR.centroids(xh, lab, k, reduce, c0h)
    assert counts[7] == 0 and n_empty == 1 and (counts[np.arange(k) != 7] > 0).all()
    assert np.array_equal(got.labels.cpu().numpy(), lab) and got.labels.dtype == torch.int64
    assert got.counts.cpu().tolist() == counts.tolist() and got.counts.dtype == torch.int64
    assert (got.n_iter, got.converged, got.n_changed, got.n_empty, got.n_unassigned) == (1, False, [N], 1, 0)
    assert (got.k, got.metric) == (k, metric)
    cent = got.centroids.cpu().numpy()
    assert np.array_equal(bits(cent[7]), bits(c0h[7]))           # empty: keeps its row
    if metric == 'euclidean':
        assert np.array_equal(bits(cent), bits(want))
        assert got.inertia == float((best.astype(np.float64) ** 2).sum())
    else:
        sums = KR.segment_sum(xh, lab, k)[0]
        for j in range(k):
            if j != 7:
                unit_close(cent[j], sums[j], DIM, j)
        assert got.inertia == float(best.astype(np.float64).sum())


# ----------------------------------------------------------------------------
# 4. loop invariants
# ----------------------------------------------------------------------------
def same_result(a, b):
    return (torch.equal(a.labels, b.labels) and np.array_equal(bits(a.centroids.cpu().numpy()), bits(b.centroids.cpu().numpy()))
            and torch.equal(a.counts, b.counts) and a.n_changed == b.n_changed and a.inertia == b.inertia
            and (a.n_iter, a.converged, a.n_empty, a.n_unassigned) == (b.n_iter, b.converged, b.n_empty, b.n_unassigned))


@pytest.mark.parametrize('k,metric,max_iter', [(1, 'cosine', 30), (3, 'cosine', 30), (10, 'cosine', 30),
                                               (37, 'cosine', 30), (301, 'cosine', 30), (10, 'euclidean', 30),
                                               (37, 'euclidean', 2)])
def test_loop_invariants(k, metric, max_iter):
    from grl_amd import engine
    x = feature_case()
    reduce = 'unit' if metric == 'cosine' else 'mean'
    r = engine.kmeans(x, k, metric, init='random', seed=4, max_iter=max_iter)
    print('k %d %s: %d iterations, converged %s, changed %s, empty %d, inertia %.6g'
          % (k, metric, r.n_iter, r.converged, r.n_changed, r.n_empty, r.inertia))
    assert 1 <= r.n_iter <= max_iter and len(r.n_changed) == r.n_iter and r.n_changed[0] == N
    assert (r.n_changed[-1] == 0) == r.converged
    assert all(c > 0 for c in r.n_changed[:-1])
    assert int(r.counts.sum()) + r.n_unassigned == N and r.n_unassigned == 0
    assert torch.equal(r.counts, torch.bincount(r.labels, minlength=k))
    if not r.converged:
        assert r.n_iter == max_iter
    if k == 1:                                                   # one cluster: nothing can change in the second round
        assert r.converged and r.n_changed == [N, 0]
    # centroids = the update of the returned labels from the centroids they were assigned against: recover those
    # by running one iteration less
    if r.n_iter > 1:
        before = engine.kmeans(x, k, metric, init='random', seed=4, max_iter=r.n_iter - 1).centroids
    else:
        before = x[torch.from_numpy(np.random.Generator(np.random.PCG64(4)).choice(N, k, replace=False)).to(DEV)]
    again, counts = engine.cluster_centroids(x, r.labels, k, reduce, before)
    assert np.array_equal(bits(again.cpu().numpy()), bits(r.centroids.cpu().numpy())) and torch.equal(counts, r.counts)
    lab_before, dist_before = engine.kmeans_assign(x, before, metric)
    assert torch.equal(lab_before, r.labels)
    d64 = dist_before.cpu().numpy().astype(np.float64)
    assert r.inertia == float((d64 if metric == 'cosine' else d64 ** 2).sum())
    if r.converged:
        assert torch.equal(engine.kmeans_assign(x, r.centroids, metric)[0], r.labels)
    for width in (7, 64, k):
        assert same_result(r, engine.kmeans(x, k, metric, init='random', seed=4, max_iter=max_iter, block_cols=width)), width
    assert same_result(r, engine.kmeans(x, k, metric, init='random', seed=4, max_iter=max_iter))


def test_k_equal_n_from_every_sample_converges_with_every_count_one():
    from grl_amd import engine
    x = feature_case()
    for metric in ('cosine', 'euclidean'):
        r = engine.kmeans(x, N, metric, init=range(N), max_iter=5)
        assert r.converged and r.n_iter == 2 and r.n_changed == [N, 0] and r.n_empty == 0
        assert r.labels.cpu().tolist() == list(range(N)) and r.counts.cpu().tolist() == [1] * N


# ----------------------------------------------------------------------------
# 5. planted data
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_planted_partition_is_recovered_and_equals_the_model(metric):
    from grl_amd import engine
    x, ids = planted_case()
    first = [int(np.flatnonzero(ids == j)[0]) for j in range(10)]
    r = engine.kmeans(x, 10, metric, init=first, max_iter=20)
    assert r.converged and r.n_empty == 0 and r.counts.cpu().tolist() == [30] * 10
    s = r.pair_scores(ids)
    assert s['ari'] == 1.0 and s['precision'] == 1.0 and s['recall'] == 1.0
    m = KR.kmeans(x.cpu().numpy(), 10, metric, init=first, max_iter=20, dist=dev_matrix(x, metric))
    assert m['converged'] and KR.same_partition(m['labels'], r.labels.cpu().numpy())
    assert np.array_equal(m['labels'], r.labels.cpu().numpy()) and m['n_changed'] == r.n_changed
    assert r.pair_scores(np.zeros(300))['recall'] < 1.0          # (the scores do look at the pids)


# ----------------------------------------------------------------------------
# 6. the DBSCAN result's centres
# ----------------------------------------------------------------------------
def test_clustering_centroids_equal_cluster_centroids_on_the_dbscan_labels():
    from grl_amd import engine
    x = feature_case()
    cl = engine.cluster(x, -0.99, 2)
    assert cl.n_clusters >= 3 and cl.n_noise >= 1
    for reduce in ('unit', 'mean', 'sum'):
        got, counts = cl.centroids(x, reduce)
        want, wc = engine.cluster_centroids(x, cl.labels, cl.n_clusters, reduce)
        assert tuple(got.shape) == (cl.n_clusters, DIM) and torch.equal(got, want) and torch.equal(counts, wc)
    got, counts = cl.centroids(x)                                # 'unit' is the default
    assert torch.equal(got, engine.cluster_centroids(x, cl.labels, cl.n_clusters, 'unit')[0])
    assert np.allclose(got.norm(dim=1).cpu().numpy(), 1.0, atol=1e-5)
    lab = cl.labels.cpu().numpy()
    sums, mc = KR.segment_sum(x.cpu().numpy(), lab, cl.n_clusters)
    assert np.array_equal(bits(cl.centroids(x, 'sum')[0].cpu().numpy()), bits(sums))
    assert counts.cpu().tolist() == mc.tolist() and int(counts.sum()) == N - cl.n_noise


# ----------------------------------------------------------------------------
# 7. ATTEvaluator.evaluate with GRL_EVAL_KMEANS
# ----------------------------------------------------------------------------
KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_CLUSTER', 'GRL_EVAL_KMEANS')


def test_attevaluator_runs_kmeans_on_the_gallery(synth_models, monkeypatch, tmp_path):
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
    gf, gp = torch.cat((qf, gf), 0), np.append(qp, gp)
    n = gf.size(0)
    path = str(tmp_path) + os.sep
    out_file = os.path.join(str(tmp_path), 'kmeans.json')

    def run():
        if os.path.exists(out_file):
            os.remove(out_file)
        with contextlib.redirect_stdout(io.StringIO()) as o:
            r = ev.evaluate(None, None, q_loader, g_loader, path, 0, 0)
        text = open(out_file).read() if os.path.exists(out_file) else None
        return r, o.getvalue(), text

    def refuse(c):
        raise ValueError('not strict JSON: %s' % c)

    def check(route, value, k, max_iter, seed):
        monkeypatch.delenv('GRL_EVAL_KMEANS', raising=False)
        r_off, text_off, file_off = run()
        assert file_off is None and 'K-means' not in text_off and 'Pairwise' not in text_off, route
        monkeypatch.setenv('GRL_EVAL_KMEANS', value)
        r_on, text_on, raw = run()
        monkeypatch.delenv('GRL_EVAL_KMEANS')
        assert r_on == r_off, route
        want = engine.kmeans(gf, k, 'cosine', 'random', seed, max_iter)
        s = want.pair_scores(gp)
        lines = ['K-means: {} clusters of {} ({} iterations, {}, {} empty), inertia = {:.6g}'.format(
                     k, n, want.n_iter, 'converged' if want.converged else 'not converged', want.n_empty, want.inertia),
                 'Pairwise precision: {:.2%}  recall: {:.2%}  F1: {:.2%}  ARI: {:.4f}'.format(
                     s['precision'], s['recall'], s['f1'], s['ari'])]
        at = text_on.splitlines()
        assert at[-3:] == lines + ['------------------'], (route, at[-3:])         # the k-means lines come last
        assert ''.join(at[:-3]) + '------------------' == ''.join(text_off.splitlines()), route
        js = json.loads(raw, parse_constant=refuse)
        assert js == {'k': k, 'max_iter': max_iter, 'seed': seed, 'init': 'random', 'metric': 'cosine', 'n': n,
                      'n_iter': want.n_iter, 'converged': want.converged, 'n_changed': want.n_changed,
                      'n_empty': want.n_empty, 'n_unassigned': 0, 'inertia': want.inertia,
                      'counts': want.counts.cpu().tolist(), 'pair_scores': s, 'labels': want.labels.cpu().tolist()}, route
        return text_off

    n_ids = int(np.unique(gp).size)
    assert 1 < n_ids < n
    check('dense', 'ids,20', n_ids, 20, 0)
    monkeypatch.setenv('GRL_EVAL_STREAM', '1')
    check('stream', '3,2,5', 3, 2, 5)
    monkeypatch.setenv('GRL_EVAL_CLUSTER', 'eer')                # combined: DBSCAN's lines first, k-means last
    monkeypatch.setenv('GRL_EVAL_KMEANS', '2')
    at = run()[1].splitlines()
    assert [l.split(':')[0] for l in at[-5:-1]] == ['Clusters', 'Pairwise precision', 'K-means', 'Pairwise precision']
    monkeypatch.delenv('GRL_EVAL_CLUSTER')
    monkeypatch.delenv('GRL_EVAL_STREAM')
    monkeypatch.setenv('GRL_EVAL_METRIC', 'verify')
    with pytest.raises(ValueError, match='GRL_EVAL_KMEANS cannot be combined with GRL_EVAL_METRIC'):
        run()
    monkeypatch.delenv('GRL_EVAL_METRIC')
    monkeypatch.setenv('GRL_EVAL_KMEANS', '0')
    with pytest.raises(ValueError, match='GRL_EVAL_KMEANS'):
        run()
