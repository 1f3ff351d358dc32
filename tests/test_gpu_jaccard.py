"""DBSCAN on the k-reciprocal Jaccard distance on the device (engine.jaccard_graph / cluster_jaccard, jaccard.hip,
DESIGN.md 4v) against the numpy model of tests/jaccard_ref.py, tests/cluster_ref.py and scikit-learn.

What is compared bit for bit, and the one place where it is not.  The model reads S = pairwise_distance_tensor(xf, xf)
as the device computed it, so colmax, the rank lists and the expansion lists are integers and IEEE operations on equal
bits: equal.  The weights are V = expf(-D) / sum, and no host restates the device's expf bit for bit (its last step is
the hardware's exp2, good to 1 ulp; numpy's exp is good to 1 ulp as well).  Measured on MI355X with the inputs below: 40 %
of the weights differ from numpy's, by at most 4 ulp, and with numpy's weights the graphs' row_ptr and col were still
equal while 100 % of the cases with edges had some val off in the last bits.  So the weights are checked against numpy
within 8 ulp (2 from the two exps in the numerator, 2 in every term of the sum, at most 3 from the roundings of a
pairwise sum of <= 256 terms whose inputs differ, 1 from the quotient), and the model is then run on the device's
weights (``weights=``): from there on everything is sums, quotients and minima of equal bits in a stated order, and
row_ptr, col and val are equal bit for bit."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import cluster_ref as CR
import jaccard_ref as J

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
KS = ((1, 1), (4, 2), (20, 6), (20, 8))
EPS = (0.0, 0.3, 0.6, 0.999, -0.5)
ULP = 2.0 ** -23

_cache = {}


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _rows(n, d, seed=None):
    """The case's rows on the device; d = 260 is a column slice of a wider matrix (rows 264 floats apart)."""
    x = torch.from_numpy(J.features(n, d, n + d if seed is None else seed)).to(DEV)
    if d == 260:
        wide = torch.zeros((n, 264), device=DEV)
        wide[:, :d] = x
        x = wide[:, :d]
        assert not x.is_contiguous()
    return x


def _model(x, k1, k2, key=None):
    """(state, S, J of the model on the device's weights) of the rows ``x``; cached by ``key``.  Checks every stage of
    the state that the model restates: colmax, rank lists and expansion lists exactly, the weights within 8 ulp, V2
    bit for bit from the device's weights."""
    from grl_amd import engine
    if key is not None and key in _cache:
        return _cache[key]
    n = x.shape[0]
    st = engine._JaccardSet(x, k1, k2)
    xp = engine._pad_features(x)
    S = engine.pairwise_distance_tensor(xp, xp).cpu().numpy()
    colmax, rank, lists, vals, _ = J.sparse_rows(S, k1, k2, 64)
    assert np.array_equal(_bits(st.colmax.cpu().numpy()), _bits(colmax))
    assert np.array_equal(st.rank.cpu().numpy(), rank)
    lcnt, lidx, lval = (t.cpu().numpy() for t in (st.lcnt, st.lidx, st.lval))
    assert np.array_equal(lcnt, [l.size for l in lists])
    dev_w = []
    for i in range(n):
        assert np.array_equal(lidx[i, :lcnt[i]], lists[i]), i
        w = lval[i, :lcnt[i]].copy()
        assert (np.abs(w.astype(np.float64) - vals[i]) <= 8 * ULP * vals[i]).all(), i
        dev_w.append(w)
    v2 = J.sparse_rows(S, k1, k2, 64, weights=dev_w)[4]
    rp, col, val = (t.cpu().numpy() for t in (st.row_ptr, st.col, st.val))
    assert rp[n] == st.nnz == sum(c.size for c, _ in v2)
    assert np.array_equal(col[:st.nnz], np.concatenate([c for c, _ in v2]))
    assert np.array_equal(_bits(val[:st.nnz]), _bits(np.concatenate([v for _, v in v2])))
    # the CSC is the transpose over ALL rows, ascending samples in every column
    cp, crow, cval = (t.cpu().numpy() for t in (st.csc_ptr, st.csc_row, st.csc_val))
    order = np.lexsort((np.repeat(np.arange(n), np.diff(rp)), col[:st.nnz]))
    assert cp[n] == st.nnz and np.array_equal(crow[:st.nnz], np.repeat(np.arange(n), np.diff(rp))[order])
    assert np.array_equal(_bits(cval[:st.nnz]), _bits(val[:st.nnz][order]))
    out = (st, S, J.jaccard_rows(v2, n, 1024))
    if key is not None:
        _cache[key] = out
    return out


def _equal(got, want, what):
    got = [t.cpu().numpy() for t in got]
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32, what
    for g, w, name in zip(got, want, ('row_ptr', 'col', 'val')):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), (what, name)


# ----------------------------------------------------------------------------
# 1. the graph against the model
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('k1,k2', KS)
@pytest.mark.parametrize('d', [5, 16, 260])
@pytest.mark.parametrize('n', [2, 3, 33, 65, 257, 700])
def test_jaccard_graph_equals_the_model(n, d, k1, k2):
    from grl_amd import engine
    x = _rows(n, d)
    if not (k1 < n and k2 <= n):
        with pytest.raises(ValueError, match='k1|k2'):
            engine.jaccard_graph(x, 0.5, k1, k2)
        return
    _, _, Jm = _model(x, k1, k2)
    edges = []
    for eps in EPS:
        want = J.threshold(Jm, eps)
        got = engine.jaccard_graph(x, eps, k1, k2, return_dist=True)
        assert all(t.is_cuda for t in got) and got[2].dtype == torch.float32
        _equal(got, want, (n, d, k1, k2, eps))
        edges.append(want[1].size)
    pair = engine.jaccard_graph(x, 0.6, k1, k2)
    assert len(pair) == 2
    _equal(pair, J.threshold(Jm, 0.6)[:2], 'without the distances')
    assert edges[4] == 0 and edges[3] > 0 and edges[0] <= edges[1] <= edges[2] <= edges[3]
    if n >= 257:                                                 # 32 groups, lists of at most 256: most pairs share no
        assert edges[3] < n * (n - 1)                            # neighbour, and J = 1 is never an edge


# ----------------------------------------------------------------------------
# 2. invariance: accumulator window, block width, run
# ----------------------------------------------------------------------------
def test_result_does_not_depend_on_the_window_the_block_width_or_the_run():
    from grl_amd import engine
    n, k1, k2 = 700, 20, 6
    x = _rows(n, 16)
    st, _, Jm = _model(x, k1, k2, key='n700')
    for eps in (0.6, 0.999):
        want = J.threshold(Jm, eps)
        assert want[1].size > n
        for window in (256, 512, 0, 0):                          # 700 columns: three windows, two, one; twice in a row
            _equal(st.graph(eps, return_dist=True, window=window), want, (eps, window))
    ref = [st.row_ptr, st.col, st.val, st.csc_ptr, st.csc_row, st.csc_val, st.rank, st.lcnt]
    for width in (32, 96, None, None):
        other = engine._JaccardSet(x, k1, k2, block_cols=width)
        assert other.width == (width or 352)                     # _SampleBlocks' rule: 32 * ceil(n / 64)
        for a, b in zip(ref, (other.row_ptr, other.col, other.val, other.csc_ptr, other.csc_row, other.csc_val,
                              other.rank, other.lcnt)):
            assert torch.equal(a, b), width
        _equal(engine.jaccard_graph(x, 0.6, k1, k2, block_cols=width, return_dist=True), J.threshold(Jm, 0.6), width)
    _equal(engine.jaccard_graph(x, 0.6, k1, k2, block_bytes=12 * n * 64, return_dist=True), J.threshold(Jm, 0.6),
           'block_bytes')


# ----------------------------------------------------------------------------
# 3. dense rows and long columns
# ----------------------------------------------------------------------------
def test_worst_case_rows_a_tight_blob_of_300_samples():
    """150 exact copies of one sample, 150 more within 1e-4 of it and 150 scattered samples.  Among the copies every
    distance ties, the rank lists fall on the smallest indices and a handful of columns of V2 is non-zero in every row
    of the blob: CSC lists of hundreds of entries, rows with hundreds of candidates, more than one round of the 256-wide
    compaction, several windows at window = 256."""
    from grl_amd import engine
    from grl_amd._lib import ptr
    x = torch.from_numpy(J.blob()).to(DEV)
    n, k1, k2 = 450, 20, 8
    st, _, Jm = _model(x, k1, k2)
    longest = int((st.csc_ptr[1:] - st.csc_ptr[:-1]).max())
    widest = int((st.row_ptr[1:] - st.row_ptr[:-1]).max())
    for eps in (0.3, 0.9, 0.999):
        want = J.threshold(Jm, eps)
        for window in (256, 0):
            got = st.graph(eps, return_dist=True, window=window)
            _equal(got, want, (eps, window))
            cnt = torch.full((n,), -7, dtype=torch.int32, device=DEV)
            st._edges(eps, window, cnt, None, None, None)        # the count pass alone
            assert torch.equal(cnt.long(), got[0][1:] - got[0][:-1])
        row_ptr, col = got[0].cpu().numpy(), got[1].cpu().numpy()
        rows = np.repeat(np.arange(n), np.diff(row_ptr))
        assert (col != rows).all() and (0 <= col).all() and (col < n).all()
        assert ((np.diff(col) > 0) | (np.diff(rows) > 0)).all()             # ascending within every row
    deg = np.diff(J.threshold(Jm, 0.999)[0])
    print('longest CSC column %d, widest V2 row %d, largest degree at eps 0.999: %d' % (longest, widest, deg.max()))
    # the 150 copies share their D rows, so their rank lists tie onto the same (smallest) indices: those columns are
    # non-zero in every copy's row, and two copies have equal V2 rows (J = 0 up to rounding: an edge at every eps here)
    assert longest >= 150 and np.diff(J.threshold(Jm, 0.3)[0]).max() >= 149


# ----------------------------------------------------------------------------
# 4. labels
# ----------------------------------------------------------------------------
def _same_labels(cl, labels, core, what):
    assert cl.labels.dtype == torch.int64 and cl.core.dtype == torch.bool and cl.labels.is_cuda, what
    assert np.array_equal(cl.core.cpu().numpy(), core), what
    assert np.array_equal(cl.labels.cpu().numpy(), labels), what
    assert cl.n_clusters == labels.max() + 1 and cl.n_noise == int((labels < 0).sum()), what


@pytest.mark.parametrize('min_samples', [1, 2, 4])
def test_cluster_jaccard_equals_the_model_and_sklearn(min_samples):
    from sklearn.cluster import DBSCAN
    from grl_amd import engine
    n, k1, k2 = 257, 10, 4
    x = _rows(n, 16, seed=5)
    _, _, Jm = _model(x, k1, k2, key='labels')
    for eps in (0.4, 0.7):
        row_ptr, col, _ = J.threshold(Jm, eps)
        labels, core = CR.dbscan(n, min_samples, row_ptr=row_ptr, col=col)
        cl = engine.cluster_jaccard(x, eps, min_samples, k1, k2)
        _same_labels(cl, labels, core, (eps, min_samples))
        assert cl.n_edges == col.size and cl.eps == float(np.float32(eps)) and cl.min_samples == min_samples
        assert isinstance(cl, engine.Clustering) and 1 <= cl.rounds <= n + 1
        X = np.where(Jm <= np.float32(eps), 0.0, 1.0)
        np.fill_diagonal(X, 0.0)
        sk = DBSCAN(eps=0.5, min_samples=min_samples, metric='precomputed').fit(X)
        assert np.array_equal(cl.labels.cpu().numpy(), sk.labels_), (eps, min_samples)
        assert np.array_equal(np.flatnonzero(cl.core.cpu().numpy()), sk.core_sample_indices_), (eps, min_samples)
        assert labels.max() >= 2 and (min_samples == 1 or (labels < 0).any())


def test_planted_identities_pair_scores_centroids_and_the_edge_limit():
    from grl_amd import engine
    x, pids = J.planted(40, 8, 64, seed=2)
    xd = torch.from_numpy(x).to(DEV)
    n = 320
    _, _, Jm = _model(xd, 20, 6)
    row_ptr, col, _ = J.threshold(Jm, 0.5)
    labels, core = CR.dbscan(n, 2, row_ptr=row_ptr, col=col)
    cl = engine.cluster_jaccard(xd, 0.5, min_samples=2)
    _same_labels(cl, labels, core, 'planted')
    host = engine.Clustering(torch.from_numpy(labels), None, None, int(labels.max()) + 1, 0, 0, 0, 0.5, 2)
    s = cl.pair_scores(pids)
    assert s == host.pair_scores(pids)
    print('planted identities: %d clusters, %d noise, precision %.3f recall %.3f ARI %.3f'
          % (cl.n_clusters, cl.n_noise, s['precision'], s['recall'], s['ari']))
    assert cl.n_clusters >= 2
    # the centres of the clusters it found
    cent, counts = cl.centroids(xd)
    assert tuple(cent.shape) == (cl.n_clusters, 64) and int(counts.sum()) == n - cl.n_noise
    c2, n2 = engine.cluster_centroids(xd, torch.from_numpy(labels).to(DEV), int(labels.max()) + 1, 'unit')
    assert torch.equal(cent, c2) and torch.equal(counts, n2)
    assert np.array_equal(counts.cpu().numpy(), np.bincount(labels[labels >= 0]))
    # the edge limit is checked after the count pass, before col exists
    E = col.size
    assert cl.n_edges == E > 0
    real, seen = engine._call, []

    def spy(name, *args):
        if name == 'grl_jaccard_edges':
            seen.append(args[10])                                # out_row_ptr: None in the count pass
        return real(name, *args)
    engine._call = spy
    try:
        with pytest.raises(ValueError, match=r'E = %d.*limit of %d' % (E, E - 1)):
            engine.jaccard_graph(xd, 0.5, max_edges=E - 1)
        assert seen == [None]                                    # the fill pass never ran
        with pytest.raises(ValueError, match='limit'):
            engine.cluster_jaccard(xd, 0.5, max_edges=10)
        assert engine.jaccard_graph(xd, 0.5, max_edges=E)[1].numel() == E
    finally:
        engine._call = real
    for bad in (1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='eps'):
            engine.cluster_jaccard(xd, bad)
    with pytest.raises(ValueError, match='xf'):
        engine.jaccard_graph(xd[0], 0.5)
    with pytest.raises(ValueError, match='n >= 2'):
        engine.jaccard_graph(xd[:1], 0.5, 1, 1)


# ----------------------------------------------------------------------------
# 5. ATTEvaluator.evaluate with GRL_EVAL_CLUSTER_JACCARD
# ----------------------------------------------------------------------------
KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_CLUSTER', 'GRL_EVAL_KMEANS', 'GRL_EVAL_CLUSTER_JACCARD')


def test_attevaluator_clusters_the_gallery_by_the_jaccard_distance(synth_models, monkeypatch, tmp_path):
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
    k1, k2 = min(20, n - 1), min(6, n)
    path = str(tmp_path) + os.sep
    out_file = os.path.join(str(tmp_path), 'cluster_jaccard.json')

    def run(rerank=0):
        if os.path.exists(out_file):
            os.remove(out_file)
        with contextlib.redirect_stdout(io.StringIO()) as o:
            r = ev.evaluate(None, None, q_loader, g_loader, path, 0, rerank)
        return r, o.getvalue().splitlines(), (json.load(open(out_file)) if os.path.exists(out_file) else None)
    r_off, text_off, file_off = run()
    assert file_off is None and not any(l.startswith(('Jaccard', 'Pairwise')) for l in text_off)
    eps, m = 0.6, 2
    want = engine.cluster_jaccard(gf, eps, m, k1, k2)
    s = want.pair_scores(gp)
    lines = ['Jaccard clusters: {} ({} noise of {}) at eps = {:g}, min_samples = {}, k1 = {}, k2 = {}'.format(
                 want.n_clusters, want.n_noise, n, want.eps, m, k1, k2),
             'Pairwise precision: {:.2%}  recall: {:.2%}  F1: {:.2%}  ARI: {:.4f}'.format(
                 s['precision'], s['recall'], s['f1'], s['ari'])]
    report = {'eps': want.eps, 'min_samples': m, 'metric': 'jaccard', 'k1': k1, 'k2': k2, 'n': n,
              'n_clusters': want.n_clusters, 'n_noise': want.n_noise, 'n_edges': want.n_edges, 'pair_scores': s,
              'labels': want.labels.cpu().tolist()}
    monkeypatch.setenv('GRL_EVAL_CLUSTER_JACCARD', '%r,%d,%d,%d' % (eps, m, k1, k2))
    r_on, text_on, js = run()
    assert r_on == r_off and js == report
    assert text_on[-3:] == lines + ['------------------'] and text_on[:-3] == text_off[:-1]
    # with the other reports: after GRL_EVAL_CLUSTER's lines, before GRL_EVAL_KMEANS's
    monkeypatch.setenv('GRL_EVAL_CLUSTER', '-0.5')
    monkeypatch.setenv('GRL_EVAL_KMEANS', '3')
    _, text, js = run()
    heads = [l.split(':')[0] for l in text if l.startswith(('Clusters', 'Jaccard clusters', 'K-means', 'Pairwise'))]
    assert heads == ['Clusters', 'Pairwise precision', 'Jaccard clusters', 'Pairwise precision', 'K-means',
                     'Pairwise precision'] and js == report
    at = text.index(lines[0])
    assert text[at + 1] == lines[1] and text[at - 2].startswith('Clusters: ')
    monkeypatch.delenv('GRL_EVAL_CLUSTER')
    monkeypatch.delenv('GRL_EVAL_KMEANS')
    # every route
    monkeypatch.setenv('GRL_EVAL_STREAM', '1')
    _, text, js = run()
    assert text[-3:-1] == lines and js == report
    monkeypatch.delenv('GRL_EVAL_STREAM')
    _, text, js = run(rerank=1)
    assert text[-3:-1] == lines and js == report
    monkeypatch.setenv('GRL_EVAL_RERANK', 'stream')
    _, text, js = run(rerank=1)
    assert text[-3:-1] == lines and js == report
    monkeypatch.delenv('GRL_EVAL_RERANK')
    monkeypatch.setenv('GRL_EVAL_METRIC', 'verify')
    with pytest.raises(ValueError, match='GRL_EVAL_CLUSTER_JACCARD.*signed logit'):
        run()
