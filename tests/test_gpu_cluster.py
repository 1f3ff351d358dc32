"""DBSCAN on the device (engine.eps_graph / cluster / cluster_matrix / cluster_from_graph, cluster.hip)
against the numpy model of tests/cluster_ref.py and scikit-learn.  Graphs, core flags and labels are integers derived
from the bits the materialised distance matrix holds, so every comparison is exact."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import cluster_ref as CR

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
N, DIM = 301, 64
WIDTHS = (None, 64, 301, 7, 300)     # 64: 16-byte rows, ragged last block (45); 301 / None: one unaligned block;
                                     # 7: below one vector load, every col0 unaligned; 300: aligned rows + a block of one
EPS = (-0.995, -0.99, -0.98)
MIN_SAMPLES = (1, 2, 6)

_cache = {}


def feature_case():
    """301 unit rows on the device: 10 centres in a 3-d latent, 241 points at centre + 0.12 N(0, 1), 60 background
    points N(0, 1); the latent sits in feature columns 0, 21, 42 of 64.  Built once, never modified."""
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
    """Unit rows with one NaN row (5), one all-zero row (11) and three rows (17, 18 = -2 x 17, 19 = 2 x 17) scaled so
    that their products with each other overflow: D[17][19] = -inf, D[17][18] = D[18][19] = +inf."""
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


def matrix(which, metric):
    """The materialised matrix (host float32) of a case, computed once."""
    from grl_amd import engine
    key = (which, metric)
    if key not in _cache:
        x = feature_case() if which == 'feature' else special_case()
        fn = engine.cosin_dist if metric == 'cosine' else engine.pairwise_distance_tensor
        _cache[key] = fn(x, x).cpu().numpy()
    return _cache[key]


def _graph_equal(got, A, what):
    row_ptr, col = got
    assert row_ptr.dtype == torch.int64 and col.dtype == torch.int32 and row_ptr.is_cuda and col.is_cuda, what
    want_ptr, want_col = CR.csr(A)
    assert np.array_equal(row_ptr.cpu().numpy(), want_ptr), what
    assert np.array_equal(col.cpu().numpy(), want_col), what     # (CR.csr: ascending in every row)


def _same(cl, labels, core, what):
    assert cl.labels.dtype == torch.int64 and cl.core.dtype == torch.bool and cl.labels.is_cuda, what
    assert np.array_equal(cl.core.cpu().numpy(), core), what
    assert np.array_equal(cl.labels.cpu().numpy(), labels), what
    assert cl.n_clusters == (labels.max() + 1 if labels.size else 0) and cl.n_noise == int((labels < 0).sum()), what


# ----------------------------------------------------------------------------
# 1. the feature case: graph, labels, sklearn
# ----------------------------------------------------------------------------
def test_feature_case_has_clusters_noise_borders_and_ambiguous_borders_on_the_device_matrix():
    """What the feature case must offer at min_samples = 6, on the matrix the device computed: at every eps at least 3
    clusters, noise and rows without any edge; at one eps of the set at least (-0.995 on the host: two of them) a border
    point adjacent to cores of two different clusters, the case the smallest-id rule decides."""
    D = matrix('feature', 'cosine')
    found = False
    for eps in EPS:
        A = CR.edges(D, eps)
        labels, core = CR.dbscan(N, 6, A=A)
        U = A | A.T
        border = np.flatnonzero(~core & (labels >= 0))
        ambiguous = sum(len(set(labels[U[j] & core])) > 1 for j in border)
        print('eps %g: %d clusters, %d noise, %d border (%d next to two clusters), %d rows without an edge, E = %d'
              % (eps, labels.max() + 1, (labels < 0).sum(), border.size, ambiguous, (A.sum(1) == 0).sum(), A.sum()))
        assert labels.max() + 1 >= 3 and (labels < 0).sum() >= 1 and (A.sum(1) == 0).any(), eps
        found = found or ambiguous >= 1
    assert found                                                 # a border point next to cores of two clusters


@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_eps_graph_equals_the_csr_of_the_materialised_matrix(metric):
    from grl_amd import engine
    x = feature_case()
    D = matrix('feature', metric)
    for eps in (EPS if metric == 'cosine' else (0.1, 0.2, float(D[3, 7]))):
        A = CR.edges(D, eps)
        assert 0 < A.sum() < N * (N - 1)
        for width in WIDTHS:
            _graph_equal(engine.eps_graph(x, eps, metric=metric, block_cols=width), A, (metric, eps, width))
    _graph_equal(engine.eps_graph(x, eps, metric=metric, block_bytes=4 * N * 256), A, 'block_bytes')


@pytest.mark.parametrize('min_samples', MIN_SAMPLES)
def test_cluster_equals_the_model_and_cluster_matrix_equals_sklearn(min_samples):
    from sklearn.cluster import DBSCAN
    from grl_amd import engine
    x = feature_case()
    D = matrix('feature', 'cosine')
    S = np.minimum(D, D.T)                                       # symmetrised: what sklearn can be asked about
    for eps in EPS:
        labels, core = CR.dbscan(N, min_samples, A=CR.edges(D, eps))
        for width in (None, 64, 7):
            cl = engine.cluster(x, eps, min_samples, block_cols=width)
            _same(cl, labels, core, (eps, min_samples, width))
            assert cl.n_edges == CR.edges(D, eps).sum() and cl.min_samples == min_samples
            assert cl.eps == float(np.float32(eps)) and 1 <= cl.rounds <= N + 1
        X = np.where(S <= np.float32(eps), 0.0, 1.0)
        np.fill_diagonal(X, 0.0)
        sk = DBSCAN(eps=0.5, min_samples=min_samples, metric='precomputed').fit(X)
        cm = engine.cluster_matrix(torch.from_numpy(S).to(DEV), eps, min_samples)
        assert np.array_equal(cm.labels.cpu().numpy(), sk.labels_), (eps, min_samples)
        assert np.array_equal(np.flatnonzero(cm.core.cpu().numpy()), sk.core_sample_indices_), (eps, min_samples)
    # euclidean, through the same entry
    E = matrix('feature', 'euclidean')
    labels, core = CR.dbscan(N, min_samples, A=CR.edges(E, 0.15))
    _same(engine.cluster(x, 0.15, min_samples, metric='euclidean', block_cols=64), labels, core, 'euclidean')


# ----------------------------------------------------------------------------
# 2. special values
# ----------------------------------------------------------------------------
def test_special_values_nan_zero_row_infinities_and_infinite_eps():
    from grl_amd import engine
    x = special_case()
    D = matrix('special', 'cosine')
    assert np.isnan(D[5]).all() and np.isnan(D[:, 5]).all()
    assert (D[11, [0, 1, 2]] == 0).all()                         # the zero row: distances of (signed) zero
    assert np.isneginf(D[17, 19]) and np.isposinf(D[17, 18]) and np.isposinf(D[19, 18]) and np.isfinite(D[17, 17])
    exact = float(D[40, 41])                                     # an entry's exact value: the edge is inclusive
    below = float(np.nextafter(np.float32(exact), np.float32(-np.inf)))
    for eps in (np.inf, -np.inf, 0.0, -0.0, exact, below, -0.3, 3.0e38):
        A = CR.edges(D, eps)
        for width in (None, 64, 7):
            _graph_equal(engine.eps_graph(x, eps, block_cols=width), A, (eps, width))
        for m in (1, 2):
            _same(engine.cluster(x, eps, m), *CR.dbscan(N, m, A=A), what=(eps, m))
    A = CR.edges(D, exact)
    assert A[40, 41] and not CR.edges(D, below)[40, 41]
    # eps = +inf: the complete graph on everything that is neither NaN nor +inf; every such row's neighbours (more
    # than 256) cross the fill kernel's chunk boundary
    A = CR.edges(D, np.inf)
    finite = ~np.isnan(D) & ~np.isposinf(D)
    np.fill_diagonal(finite, False)
    assert np.array_equal(A, finite) and A.sum(1).max() == N - 2 and A.sum() >= (N - 1) * (N - 2) - 4
    assert A[5].sum() == 0 and A[:, 5].sum() == 0                # the NaN row is alone
    cl = engine.cluster(x, np.inf, 2)
    assert cl.n_clusters == 1 and cl.n_noise == 1 and int(cl.labels[5]) == -1 and cl.n_edges == A.sum()
    # eps = -inf: only the -inf entries are edges
    A = CR.edges(D, -np.inf)
    assert A.sum() == np.isneginf(D).sum() - np.isneginf(np.diag(D)).sum() and A.sum() >= 1


def test_cluster_matrix_follows_the_either_direction_rule_on_an_asymmetric_matrix():
    """A matrix that is not symmetric anywhere (cosine distances plus independent noise per entry), with a NaN row, a
    +inf and a -inf entry and one pair whose edge exists in one direction only by a wide margin."""
    from grl_amd import engine
    g = np.random.Generator(np.random.PCG64(13))
    x = g.standard_normal((N, 16))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    M = (-(x @ x.T) + 0.05 * g.standard_normal((N, N))).astype(np.float32)
    M[5], M[6, 8], M[8, 6] = np.nan, np.inf, -np.inf
    M[7, 9], M[9, 7] = -1.0, 1.0
    A = CR.edges(M, -0.55)
    one_way = int((A & ~A.T).sum())
    print('edges %d, stored in one direction only %d' % (A.sum(), one_way))
    assert one_way > 50 and A[7, 9] and not A[9, 7] and A[8, 6] and not A[6, 8]
    dev = torch.from_numpy(M).to(DEV)
    for m in (1, 2, 4, 6):
        labels, core = CR.dbscan(N, m, A=A)
        _same(engine.cluster_matrix(dev, -0.55, m), labels, core, m)
        assert labels[7] == labels[9] or m > 1 + A[7].sum()
    assert ((CR.dbscan(N, 4, A=A)[0] >= 0) & ~CR.dbscan(N, 4, A=A)[1]).sum() > 5          # border points exist


def test_eps_graph_across_the_vector_paths_chunk_boundary():
    """1100 columns in 16-byte rows: the four-columns-a-lane path has a second, ragged chunk."""
    from grl_amd import engine
    g = np.random.Generator(np.random.PCG64(7))
    x = g.standard_normal((1100, 32)).astype(np.float32)       # (the GEMM takes K in multiples of 32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    xd = torch.from_numpy(x).to(DEV)
    D = engine.cosin_dist(xd, xd).cpu().numpy()
    for eps in (np.inf, -0.2):
        A = CR.edges(D, eps)
        for width in (None, 1028):
            _graph_equal(engine.eps_graph(xd, eps, block_cols=width), A, (eps, width))
    assert CR.edges(D, np.inf).sum() == 1100 * 1099


# ----------------------------------------------------------------------------
# 3. cluster_from_graph on host-built CSRs
# ----------------------------------------------------------------------------
def _csr(n, edges):
    """CSR in the order given (rows grouped, no sorting inside a row, duplicates kept)."""
    rows = [[] for _ in range(n)]
    for i, j in edges:
        rows[i].append(j)
    row_ptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int64)
    col = np.array([j for r in rows for j in r], dtype=np.int32)
    return row_ptr, col


def _from_graph(n, edges, m):
    from grl_amd import engine
    row_ptr, col = _csr(n, edges)
    cl = engine.cluster_from_graph(torch.from_numpy(row_ptr).to(DEV), torch.from_numpy(col).to(DEV), n, m)
    _same(cl, *CR.dbscan(n, m, row_ptr=row_ptr, col=col), what=(n, m, len(edges)))
    return cl


def test_components_of_long_paths_stars_and_duplicate_edges():
    g = np.random.Generator(np.random.PCG64(3))
    # a path over 301 nodes in descending index order, each edge stored once
    desc = [(i, i - 1) for i in range(N - 1, 0, -1)]
    cl = _from_graph(N, desc, 1)
    assert cl.n_clusters == 1 and (cl.parent == 0).all() and (cl.labels == 0).all()
    # a path through a random permutation, stored in the direction of the walk
    perm = g.permutation(N)
    walk = list(zip(perm[:-1].tolist(), perm[1:].tolist()))
    cl = _from_graph(N, walk, 1)
    assert cl.n_clusters == 1 and (cl.parent == 0).all()
    print('rounds: descending path %d, permuted path %d' % (_from_graph(N, desc, 1).rounds, cl.rounds))
    # with min_samples 2 the walk's last node has no out-edge: it is a border point of the one cluster
    cl = _from_graph(N, walk, 2)
    assert cl.n_clusters == 1 and cl.n_noise == 0 and not bool(cl.core[perm[-1]])
    # two paths (150 and 151 nodes), then joined by one edge stored in one direction only
    a, b = perm[:150], perm[150:]
    two = list(zip(a[:-1].tolist(), a[1:].tolist())) + list(zip(b[:-1].tolist(), b[1:].tolist()))
    cl = _from_graph(N, two, 1)
    assert cl.n_clusters == 2 and sorted(set(cl.parent.tolist())) == sorted((int(a.min()), int(b.min())))
    cl = _from_graph(N, two + [(int(b[70]), int(a[20]))], 1)
    assert cl.n_clusters == 1 and (cl.parent == 0).all()
    # a star whose centre is the only core: borders, no core-core edge; stored from the centre / from the leaves
    for edges in ([(200, j) for j in range(N) if j != 200 and j % 3], [(j, 200) for j in range(N) if j != 200 and j % 3]):
        m, leaves = (3 if edges[0][0] == 200 else 2), len(edges)
        cl = _from_graph(N, edges, m)
        assert cl.n_noise == N - 1 - leaves and int(cl.labels[200]) == 0
        if edges[0][0] == 200:
            assert cl.core.sum() == 1 and cl.n_clusters == 1
        else:                                                    # every leaf is core (one out-edge), the centre is a border point
            assert not bool(cl.core[200]) and cl.n_clusters == leaves
    # no edges at all
    cl = _from_graph(N, [], 1)
    assert cl.n_clusters == N and cl.labels.tolist() == list(range(N)) and cl.n_edges == 0
    cl = _from_graph(N, [], 2)
    assert cl.n_clusters == 0 and cl.n_noise == N
    # duplicate edges in both directions, a self-loop, unsorted rows
    dup = [(5, 9), (9, 5), (5, 9), (9, 5), (9, 5), (9, 9), (30, 2), (2, 30), (30, 9), (30, 9), (300, 0)]
    for m in (1, 2, 3, 4):
        _from_graph(N, dup, m)


def test_malformed_graphs_and_limits_are_value_errors():
    from grl_amd import engine
    x = feature_case()
    row_ptr, col = _csr(4, [(0, 1), (1, 0), (2, 3)])
    rp, c = torch.from_numpy(row_ptr).to(DEV), torch.from_numpy(col).to(DEV)
    assert engine.cluster_from_graph(rp, c, 4).n_clusters == 2
    for bad_rp, bad_c, what in ((rp, torch.tensor([1, 0, 4], dtype=torch.int32, device=DEV), 'outside'),
                                (rp, torch.tensor([1, -1, 3], dtype=torch.int32, device=DEV), 'outside'),
                                (rp, c[:2], 'len'), (rp + 1, c, r'row_ptr\[0\]'),
                                (torch.tensor([0, 2, 1, 3, 3], device=DEV), c, 'descends'),
                                (rp[:-1], c, 'n \\+ 1'), (rp.int(), c, 'row_ptr'), (rp, c.long(), 'col'),
                                (rp.cpu(), c, 'row_ptr')):
        with pytest.raises(ValueError, match=what):
            engine.cluster_from_graph(bad_rp, bad_c, 4)
    D = matrix('feature', 'cosine')
    n_edges = int(CR.edges(D, -0.98).sum())
    with pytest.raises(ValueError, match=r'eps = -0\.98.*E = %d.*limit of %d' % (n_edges, n_edges - 1)):
        engine.eps_graph(x, -0.98, max_edges=n_edges - 1)
    with pytest.raises(ValueError, match='limit'):
        engine.cluster(x, -0.98, max_edges=10)
    with pytest.raises(ValueError, match='limit'):
        engine.cluster_matrix(torch.from_numpy(D).to(DEV), -0.98, max_edges=10)
    assert engine.eps_graph(x, -0.98, max_edges=n_edges)[1].numel() == n_edges
    with pytest.raises(ValueError, match='square'):
        engine.cluster_matrix(torch.zeros((4, 5), device=DEV), 0.5)
    with pytest.raises(ValueError, match='square'):
        engine.cluster_matrix(torch.zeros((4,), device=DEV), 0.5)


# ----------------------------------------------------------------------------
# 4. strided input, tiny n, determinism
# ----------------------------------------------------------------------------
def test_cluster_matrix_reads_a_column_slice_of_a_wider_matrix_in_place():
    from grl_amd import engine
    D = matrix('feature', 'cosine')
    labels, core = CR.dbscan(N, 6, A=CR.edges(D, -0.99))
    wide = torch.full((N, 320), float('-inf'), device=DEV)
    calls = []
    real = engine._call

    def spy(name, *args):
        if name == 'grl_cluster_edges_block':
            calls.append(args[:6])
        return real(name, *args)
    engine._call = spy
    try:
        for off in (4, 3, 0):                                    # 16-byte rows with a ragged end; unaligned rows
            wide.fill_(float('-inf'))
            wide[:, off:off + N] = torch.from_numpy(D).to(DEV)
            view = wide[:, off:off + N]
            assert not view.is_contiguous()
            _same(engine.cluster_matrix(view, -0.99, 6), labels, core, off)
            assert calls[-1] == (view.data_ptr(), 320, N, 0, 0, N)       # read in place: no copy was made
        t = torch.from_numpy(np.ascontiguousarray(D.T)).to(DEV).t()      # column-major: copied, still right
        _same(engine.cluster_matrix(t, -0.99, 6), labels, core, 'transposed')
    finally:
        engine._call = real


def test_zero_and_one_sample():
    from grl_amd import engine
    for n in (0, 1):
        x = torch.ones((n, DIM), device=DEV)
        row_ptr, col = engine.eps_graph(x, 0.0)
        assert row_ptr.tolist() == [0] * (n + 1) and col.numel() == 0 and col.dtype == torch.int32
        for m, want in ((1, list(range(n))), (2, [-1] * n)):
            for cl in (engine.cluster(x, 0.0, m), engine.cluster(x, 5.0, m, metric='euclidean'),
                       engine.cluster_matrix(torch.zeros((n, n), device=DEV), 0.0, m),
                       engine.cluster_from_graph(row_ptr, col, n, m)):
                assert cl.labels.tolist() == want and cl.labels.dtype == torch.int64 and cl.core.dtype == torch.bool
                assert cl.core.tolist() == [m == 1] * n and cl.n_edges == 0
                assert (cl.n_clusters, cl.n_noise) == ((n, 0) if m == 1 else (0, n))
                assert cl.pair_scores(np.zeros(n))['ari'] == 1.0


def test_two_runs_give_identical_graphs_parents_and_labels():
    from grl_amd import engine
    x = feature_case()
    runs = []
    for _ in range(2):
        row_ptr, col = engine.eps_graph(x, -0.98, block_cols=64)
        cl = engine.cluster_from_graph(row_ptr, col, N, 6)
        runs.append((row_ptr, col, cl.parent, cl.labels, cl.core))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # a root is its component's smallest core index
    labels, parent, core = (t.cpu().numpy() for t in (runs[0][3], runs[0][2], runs[0][4]))
    for k in range(labels.max() + 1):
        members = np.flatnonzero((labels == k) & core)
        assert (parent[members] == members.min()).all()
    assert (parent[~core] == np.flatnonzero(~core)).all()


# ----------------------------------------------------------------------------
# 5. ATTEvaluator.evaluate with GRL_EVAL_CLUSTER
# ----------------------------------------------------------------------------
KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_CLUSTER')
LINES = ('Clusters: ', 'Pairwise precision: ')


def test_attevaluator_clusters_the_gallery_on_every_route(synth_models, monkeypatch, tmp_path):
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
    gf, gp, gc = torch.cat((qf, gf), 0), np.append(qp, gp), np.append(qc, gc)
    n = gf.size(0)
    path = str(tmp_path) + os.sep
    out_file = os.path.join(str(tmp_path), 'clusters.json')

    def run(rerank=0):
        if os.path.exists(out_file):
            os.remove(out_file)
        with contextlib.redirect_stdout(io.StringIO()) as o:
            r = ev.evaluate(None, None, q_loader, g_loader, path, 0, rerank)
        return r, o.getvalue(), (json.load(open(out_file)) if os.path.exists(out_file) else None)

    def check(route, value, eps, m, rerank=0):
        """knob unset: no file, no line; knob set: the same Rank-1, the same other bytes, the two lines and the file"""
        monkeypatch.delenv('GRL_EVAL_CLUSTER', raising=False)
        r_off, text_off, file_off = run(rerank)
        assert file_off is None and 'Clusters' not in text_off and 'Pairwise' not in text_off, route
        monkeypatch.setenv('GRL_EVAL_CLUSTER', value)
        r_on, text_on, js = run(rerank)
        monkeypatch.delenv('GRL_EVAL_CLUSTER')
        assert r_on == r_off, route
        assert ''.join(l for l in text_on.splitlines(True) if not l.startswith(LINES)) == text_off, route
        want = engine.cluster(gf, eps, m)
        s = want.pair_scores(gp)
        at = text_on.splitlines()
        lines = [l for l in at if l.startswith(LINES)]
        assert lines == ['Clusters: {} ({} noise of {}) at cosine eps = {:g}, min_samples = {}'.format(
                             want.n_clusters, want.n_noise, n, want.eps, m),
                         'Pairwise precision: {:.2%}  recall: {:.2%}  F1: {:.2%}  ARI: {:.4f}'.format(
                             s['precision'], s['recall'], s['f1'], s['ari'])], (route, lines)
        assert at.index(lines[1]) == at.index(lines[0]) + 1 and at[at.index(lines[1]) + 1] == '------------------'
        last = max(i for i, l in enumerate(at) if l.startswith(('Rank-', 'ROC', 'EER', 'TPR@FPR')))
        assert at.index(lines[0]) == last + 1, route             # after the CMC and after any ROC lines
        assert js == {'eps': want.eps, 'min_samples': m, 'metric': 'cosine', 'n': n, 'n_clusters': want.n_clusters,
                      'n_noise': want.n_noise, 'n_edges': want.n_edges, 'pair_scores': s,
                      'labels': want.labels.cpu().tolist()}, route
        return text_off

    # the labels are those of the model on the materialised matrix of the extracted features
    D = engine.cosin_dist(gf, gf).cpu().numpy()
    eer = float(engine.pair_roc(qf, gf, qp, gp, qc, gc).eer_threshold)
    assert np.isfinite(eer)
    for eps, m in ((eer, 1), (eer, 2)):
        _same(engine.cluster(gf, eps, m), *CR.dbscan(n, m, A=CR.edges(D, eps)), what=('evaluator features', m))
    fixed = float(np.float32(np.median(D)))
    check('dense', '%r,2' % fixed, fixed, 2)
    check('dense eer', 'eer', eer, 1)
    eer12 = float(engine.pair_roc(qf, gf, qp, gp, qc, gc, bits=12).eer_threshold)
    monkeypatch.setenv('GRL_EVAL_ROC', '12')
    check('dense eer with a 12-bit ROC', 'eer,2', eer12, 2)      # the route's cosine PairRoc is reused
    monkeypatch.setenv('GRL_EVAL_STREAM', '1')
    check('stream eer with a 12-bit ROC', 'eer', eer12, 1)
    monkeypatch.delenv('GRL_EVAL_STREAM')
    monkeypatch.setenv('GRL_EVAL_ROC', '1')                      # still by cosine; the route's ROC is not a cosine one
    check('rerank with its own ROC', 'eer', eer, 1, rerank=1)
    monkeypatch.delenv('GRL_EVAL_ROC')
    monkeypatch.setenv('GRL_EVAL_RERANK', 'stream')
    check('rerank stream', '%r' % fixed, fixed, 1, rerank=1)
    monkeypatch.delenv('GRL_EVAL_RERANK')
    monkeypatch.setenv('GRL_EVAL_DBA', '3')
    monkeypatch.setenv('GRL_EVAL_CLUSTER', '%r' % fixed)
    _, text, js = run()
    dba = engine.expand_features(gf, gf, 3, 0, skip_self=True)   # clustered after DBA
    assert js['labels'] == engine.cluster(dba, fixed, 1).labels.cpu().tolist()
    monkeypatch.delenv('GRL_EVAL_DBA')
    monkeypatch.setenv('GRL_EVAL_METRIC', 'verify')
    with pytest.raises(ValueError, match='GRL_EVAL_CLUSTER.*signed logit'):
        run()
