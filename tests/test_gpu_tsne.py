"""t-SNE on the device (engine.tsne / tsne_affinities / tsne_gradient / tsne_from_affinities, tsne.hip)
against the numpy model of tests/tsne_ref.py.  The neighbour lists, the joint affinities, the gradient and the loop are
compared bit for bit -- the lists with the model run on the read-back device distances, the joint affinities with the
model run on the device's own conditional affinities (the hardware's expf is not pinned), the gradient and the loop on
the device's own CSR; the conditional affinities and the KL within bounds computed from the two host models."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import hdbscan_ref as HR
import silhouette_ref as SR
import tsne_ref as TR

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
F = np.float32
WIDTHS = (1, 7, 64, 100, 336)
PERPLEXITIES = (5.0, 30.0, 100.0)

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


def host(t):
    return t.cpu().numpy()


def symmetric(m):
    return np.array_equal(bits(m), bits(m.T))


def device_distances(x):
    """e(i, j) of the contract for both metrics as float32 host matrices from what the device computes for the rows
    ``x`` (zero-padded as the engine pads them) -- after asserting the precondition: the device's cosin_dist and
    pairwise_distance_tensor of a set against itself are symmetric bit for bit."""
    from grl_amd import engine
    xp = engine._pad_features(x)
    n, d = xp.shape
    sq = torch.empty(n, dtype=torch.float32, device=DEV)
    engine._call('grl_row_sqnorm', engine.ptr(xp), engine.ptr(sq), n, d, d)
    negdot = host(engine.cosin_dist(xp, xp))
    euc = host(engine.pairwise_distance_tensor(xp, xp))
    assert symmetric(negdot) and symmetric(euc)
    return {'cosine': HR.cosine_matrix(negdot, host(sq)), 'euclidean': TR.squared(euc)}


def case(d=24, n=336):
    """The first ``n`` rows of the planted input (clusters of 1 .. 130, norms 0.5 .. 1.8, shuffled) in d features and
    their device distances.  Built once."""
    if (d, n) not in _cache:
        x, ids = SR.planted(d=d)
        xd = dev(x[:n])
        _cache[d, n] = dict(x=xd, ids=ids[:n], e=device_distances(xd), lists={}, aff={})
    return _cache[d, n]


def model_lists(c, metric, perplexity):
    key = (metric, perplexity)
    if key not in c['lists']:
        n = c['x'].shape[0]
        c['lists'][key] = TR.neighbours(c['e'][metric], TR.n_neighbours(n, perplexity))
    return c['lists'][key]


def affinities(c, metric='cosine', perplexity=30.0):
    """the device's affinities of a case at the default block width, read back once"""
    from grl_amd import engine
    key = (metric, perplexity)
    if key not in c['aff']:
        row_ptr, col, val, info = engine.tsne_affinities(c['x'], perplexity, metric)
        c['aff'][key] = dict(dev=(row_ptr, col, val), csr=(host(row_ptr), host(col), host(val)), info=info,
                             idx=host(info['idx']), e=host(info['e']), cond=host(info['cond']),
                             iso=host(info['isolated']))
    return c['aff'][key]


def hub_case():
    """300 samples in d = 64: 299 around one direction c at an angle of 45 degrees, mutually at about 60 degrees, and
    their mean direction, which is everybody's nearest neighbour: its row of P holds all the others."""
    if 'hub' not in _cache:
        g = np.random.Generator(np.random.PCG64(11))
        c = g.standard_normal(64)
        c /= np.linalg.norm(c)
        u = g.standard_normal((299, 64))
        u -= (u @ c)[:, None] * c
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        x = c + u
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        m = x.mean(0)
        x = np.concatenate((x[:150], (m / np.linalg.norm(m))[None], x[150:])).astype(F)
        xd = dev(x)
        _cache['hub'] = dict(x=xd, hub=150, e=device_distances(xd), lists={}, aff={})
    return _cache['hub']


def check_lists(info, want, K):
    widx, we = want
    assert info['K'] == K and info['idx'].dtype == torch.int32 and info['e'].dtype == torch.float32
    assert np.array_equal(host(info['idx']), widx) and same(host(info['e']), we)


# ----------------------------------------------------------------------------
# 1. the neighbour lists, bit for bit against the model on the device's own distances
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('d', [24, 5])
@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_neighbours_equal_the_model_for_every_block_width(metric, d):
    from grl_amd import engine
    c = case(d)
    for perplexity, K in zip(PERPLEXITIES, (16, 91, 301)):
        want = model_lists(c, metric, perplexity)
        ref = affinities(c, metric, perplexity)
        check_lists(ref['info'], want, K)
        for width in WIDTHS:
            row_ptr, col, val, info = engine.tsne_affinities(c['x'], perplexity, metric, block_cols=width)
            check_lists(info, want, K)
            # the same bits for every block width, all the way to the joint affinities
            assert same(host(info['cond']), ref['cond']) and same(host(info['beta']), host(ref['info']['beta']))
            assert np.array_equal(host(row_ptr), ref['csr'][0]) and np.array_equal(host(col), ref['csr'][1])
            assert same(host(val), ref['csr'][2])
    info = engine.tsne_affinities(c['x'], 30.0, metric, block_bytes=1)[3]      # the floor of 256 columns
    check_lists(info, model_lists(c, metric, 30.0), 91)


@pytest.mark.parametrize('n', [65, 129])
@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_neighbours_at_the_lane_chunk_edges(metric, n):
    """One wave reads a row in chunks of 64: n = 65 and 129 leave a chunk of one, widths 63 .. 65 cut just before, on
    and just after the chunk edge.  At n = 65 and perplexity 30 every other sample is a neighbour: K = n - 1."""
    from grl_amd import engine
    c = case(24, n)
    K = TR.n_neighbours(n, 30.0)
    assert K == (64 if n == 65 else 91)
    want = model_lists(c, metric, 30.0)
    for width in (63, 64, 65, None):
        check_lists(engine.tsne_affinities(c['x'], 30.0, metric, block_cols=width)[3], want, K)


# ----------------------------------------------------------------------------
# 2. the conditional affinities: within the two host models' distance of the float64 model
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('perplexity', PERPLEXITIES)
@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_conditional_affinities_follow_the_float64_model(metric, perplexity):
    c = case(24)
    a = affinities(c, metric, perplexity)
    cond, e = a['cond'], a['e']
    assert not a['iso'].any()
    K = cond.shape[1]
    # a row is K float32 quotients by one sum: each within 2^-24 relative, the float64 total within K 2^-24 of the
    # exact quotients' total, which is 1 up to the rounding of the sum itself ((K / 64 + 6) 2^-24)
    assert np.abs(cond.astype(np.float64).sum(1) - 1.0).max() <= (2 * K / 64 + 8) * 2.0 ** -24
    assert np.abs(TR.perplexity_of(cond) / perplexity - 1.0).max() <= 1e-3
    m32 = TR.conditional32(e, perplexity)[0]
    m64, b64, _ = TR.conditional64(e, perplexity)
    bound = 4 * np.abs(m32 - m64).max()
    assert 0 < bound < 1e-4
    assert np.abs(cond - m64).max() <= bound
    beta = host(a['info']['beta'])
    assert np.abs(beta / b64 - 1.0).max() <= 1e-3


# ----------------------------------------------------------------------------
# 3. the joint affinities: the model on the device's conditional affinities, bit for bit
# ----------------------------------------------------------------------------
def check_joint(a, n):
    row_ptr, col, val = a['csr']
    wr, wc, wv = TR.joint32(a['idx'], a['cond'], a['iso'])
    assert a['dev'][0].dtype == torch.int64 and a['dev'][1].dtype == torch.int32 and a['dev'][2].dtype == torch.float32
    assert row_ptr.shape == (n + 1,) and np.array_equal(row_ptr, wr) and np.array_equal(col, wc) and same(val, wv)
    assert symmetric(TR.to_dense(row_ptr, col, val, F))


@pytest.mark.parametrize('d', [24, 5])
@pytest.mark.parametrize('metric', ['cosine', 'euclidean'])
def test_joint_affinities_equal_the_model_on_the_device_conditionals(metric, d):
    c = case(d)
    for perplexity in PERPLEXITIES:
        check_joint(affinities(c, metric, perplexity), 336)
    for n in (65, 129):
        check_joint(affinities(case(24, n), metric, 30.0), n)


def test_joint_affinities_of_a_hub_and_of_a_nan_row():
    from grl_amd import engine
    c = hub_case()
    a = affinities(c, 'cosine', 5.0)
    check_lists(a['info'], model_lists(c, 'cosine', 5.0), 16)
    check_joint(a, 300)
    lens = np.diff(a['csr'][0])
    assert lens[c['hub']] == 299 and np.sort(lens)[-2] < 64      # one row of n - 1 entries, past any 256-entry step
    # a NaN row: isolated, in nobody's list, no entry of the CSR; everything else as the model has it
    x = case(24, 129)['x'].clone()
    x[40] = float('nan')
    e = device_distances(x)['cosine']
    row_ptr, col, val, info = engine.tsne_affinities(x, 5.0, 'cosine', block_cols=50)
    check_lists(info, TR.neighbours(e, 16), 16)
    iso = host(info['isolated'])
    assert iso.tolist() == [i == 40 for i in range(129)] and iso.dtype == np.bool_
    assert np.isnan(host(info['beta'])[40]) and not host(info['cond'])[40].any()
    a = dict(dev=(row_ptr, col, val), csr=(host(row_ptr), host(col), host(val)), idx=host(info['idx']),
             cond=host(info['cond']), iso=iso)
    check_joint(a, 129)
    assert a['csr'][0][41] == a['csr'][0][40] and not (a['csr'][1] == 40).any() and np.isfinite(a['csr'][2]).all()
    # K = n - 1: the NaN sample is in everybody's list, so everybody is isolated and there is nothing to embed
    x = case(24, 65)['x'].clone()
    x[3] = float('nan')
    row_ptr, col, val, info = engine.tsne_affinities(x, 30.0)
    assert host(info['isolated']).all() and col.numel() == 0 and not host(row_ptr).any()
    r = engine.tsne(x, 30.0, n_iter=2)
    assert r.n_isolated == 65 and np.isnan(host(r.embedding)).all() and r.kl == 0.0


# ----------------------------------------------------------------------------
# 4. the gradient, bit for bit
# ----------------------------------------------------------------------------
def check_gradient(a, y, alpha, iso=None):
    from grl_amd import engine
    grad, z = engine.tsne_gradient(*a['dev'], dev(y), alpha, None if iso is None else dev(iso))
    wg, wz = TR.gradient32(*a['csr'], y, alpha, iso)
    assert grad.dtype == torch.float32 and tuple(grad.shape) == y.shape and tuple(z.shape) == (1,)
    assert same(host(z), np.asarray([wz])) and same(host(grad), wg)
    return host(grad)


def coordinates(n):
    g = np.random.Generator(np.random.PCG64(21))
    y3 = (g.standard_normal((n, 2)) * 3).astype(F)
    twin = y3.copy()
    twin[n // 2] = twin[3]                                       # two coincident points: dx = 0, q = 1
    return TR.init_random(n, 0), y3, twin


@pytest.mark.parametrize('n', [65, 129, 336])
def test_gradient_equals_the_model(n):
    a = affinities(case(24, n), 'cosine', 30.0)
    for y in coordinates(n):
        for alpha in (12.0, 1.0):
            g = check_gradient(a, y, alpha)
            assert np.isfinite(g).all() and np.abs(g).max() > 0
    # an isolated sample on a caller's request: it feels no force and exerts none, whatever its row of y holds
    iso = np.zeros(n, dtype=bool)
    iso[[5, n - 1]] = True
    y = coordinates(n)[1].copy()
    g = check_gradient(a, y, 12.0, iso)
    y[5] = np.nan
    g2 = check_gradient(a, y, 12.0, iso)
    assert same(g, g2) and not g[5].any() and not g[n - 1].any()


def test_gradient_of_the_hub_and_of_a_nan_row():
    from grl_amd import engine
    c = hub_case()
    a = affinities(c, 'cosine', 5.0)
    for y in coordinates(300)[:2]:
        check_gradient(a, y, 12.0)
    x = case(24, 129)['x'].clone()
    x[40] = float('nan')
    row_ptr, col, val, info = engine.tsne_affinities(x, 5.0)
    a = dict(dev=(row_ptr, col, val), csr=(host(row_ptr), host(col), host(val)))
    y = coordinates(129)[1]
    g = check_gradient(a, y, 1.0, host(info['isolated']))
    assert np.isfinite(g).all() and not g[40].any()


# ----------------------------------------------------------------------------
# 5. the loop, bit for bit; repeatability
# ----------------------------------------------------------------------------
def check_state(r, want):
    y, update, gains = want
    assert same(host(r.embedding), y) and same(host(r.update), update) and same(host(r.gains), gains)


def test_three_iterations_and_the_momentum_switch_equal_the_model():
    from grl_amd import engine
    c = case(24)
    a = affinities(c)
    y0 = TR.init_random(336, 0)
    lr = F(TR.auto_learning_rate(336))
    r = engine.tsne(c['x'], 30.0, n_iter=3)
    assert r.learning_rate == 50.0 and r.seed == 0 and r.n_iter == 3 and r.n_isolated == 0 and r.metric == 'cosine'
    assert all(torch.equal(s, t) for s, t in zip(r.affinities[:2], a['dev'][:2])) and same(host(r.affinities[2]), a['csr'][2])
    check_state(r, TR.run32(*a['csr'], y0, 3, lr))
    r = engine.tsne_from_affinities(*a['dev'], 3, seed=0)
    check_state(r, TR.run32(*a['csr'], y0, 3, lr))
    # across the switch: iterations 0 and 1 at (12, 0.5), iteration 2 at (1, 0.8)
    r2 = engine.tsne_from_affinities(*a['dev'], 3, exaggeration_iter=2)
    check_state(r2, TR.run32(*a['csr'], y0, 3, lr, 12.0, 2))
    assert not same(host(r2.embedding), host(r.embedding))
    # and the iterations 249, 250, 251 of the default schedule from a state that is handed in
    g = np.random.Generator(np.random.PCG64(5))
    y = (g.standard_normal((336, 2)) * 2).astype(F)
    u = (g.standard_normal((336, 2)) * 0.1).astype(F)
    gn = g.uniform(0.01, 3.0, (336, 2)).astype(F)
    r3 = engine.tsne_from_affinities(*a['dev'], 3, init=dev(y), first_iter=249, gains=dev(gn), update=dev(u),
                                     learning_rate=80.0, early_exaggeration=4.0)
    assert r3.seed is None and r3.learning_rate == 80.0
    check_state(r3, TR.run32(*a['csr'], y, 3, 80.0, 4.0, 250, first=249, update=u, gains=gn))
    # euclidean, another seed
    ae = affinities(c, 'euclidean', 30.0)
    r = engine.tsne(c['x'], 30.0, 'euclidean', n_iter=2, seed=3)
    check_state(r, TR.run32(*ae['csr'], TR.init_random(336, 3), 2, lr))


def test_two_runs_and_two_block_widths_give_identical_bits():
    from grl_amd import engine
    c = case(24)
    runs = [engine.tsne(c['x'], 30.0, n_iter=60, block_cols=w) for w in (None, None, 7, 336)]
    for r in runs[1:]:
        assert torch.equal(r.embedding.view(torch.int32), runs[0].embedding.view(torch.int32)) and r.kl == runs[0].kl
        assert torch.equal(r.gains.view(torch.int32), runs[0].gains.view(torch.int32))
    # a run continued from its state is the same run
    a = runs[0].affinities
    half = engine.tsne_from_affinities(*a, 25)
    rest = engine.tsne_from_affinities(*a, 35, init=half.embedding, first_iter=25, gains=half.gains, update=half.update)
    assert torch.equal(rest.embedding.view(torch.int32), runs[0].embedding.view(torch.int32)) and rest.kl == runs[0].kl


# ----------------------------------------------------------------------------
# 6. end to end: 500 iterations on the planted input
# ----------------------------------------------------------------------------
def test_end_to_end_kl_and_trustworthiness():
    """Planted 336, d = 24, perplexity 30, 500 iterations, seed 0.  Measured on an MI355X: the device's KL 0.628242451,
    the host's float32 evaluation at the read-back P and y 0.628242451, its float64 evaluation 0.628242444; the float64
    model from the same init ends at 0.626141 (ratio 1.0034); 5-neighbour trustworthiness 0.9615 against 0.9602 for
    scikit-learn's exact TSNE and 0.9607 for the float64 model."""
    from sklearn.manifold import TSNE, trustworthiness
    from grl_amd import engine
    c = case(24)
    r = engine.tsne(c['x'], 30.0, n_iter=500)
    y = host(r.embedding)
    row_ptr, col, val = (host(t) for t in r.affinities)
    assert np.isfinite(y).all() and r.n_isolated == 0
    p = TR.to_dense(row_ptr, col, val)
    kl32, kl64 = TR.kl32(row_ptr, col, val, y), TR.kl64(p, y)
    print('kl: device %.9g, host float32 %.9g, host float64 %.9g' % (r.kl, kl32, kl64))
    assert abs(r.kl - kl64) <= 4 * abs(kl32 - kl64)
    # the float64 model from the same init, on the float64 model's own affinities of the device's distances
    a = affinities(c)
    c64, _, iso = TR.conditional64(a['e'], 30.0)
    p64, _ = TR.joint64(a['idx'], c64, iso)
    y64 = TR.run64(p64, TR.init_random(336, 0), 500, TR.auto_learning_rate(336))
    kl_model = TR.kl64(p64, y64)
    print('kl: device %.6g, float64 model %.6g (ratio %.4f)' % (r.kl, kl_model, r.kl / kl_model))
    assert r.kl <= 1.05 * kl_model
    e = c['e']['cosine'].astype(np.float64)
    np.fill_diagonal(e, 0.0)
    sk = TSNE(method='exact', init='random', metric='precomputed', perplexity=30.0, random_state=0).fit_transform(np.sqrt(e))
    t_dev, t_sk = trustworthiness(e, y, n_neighbors=5, metric='precomputed'), trustworthiness(e, sk, n_neighbors=5, metric='precomputed')
    print('trustworthiness(5): device %.4f, scikit-learn exact %.4f, float64 model %.4f'
          % (t_dev, t_sk, trustworthiness(e, y64, n_neighbors=5, metric='precomputed')))
    assert t_dev >= t_sk - 0.01


# ----------------------------------------------------------------------------
# 7. ATTEvaluator.evaluate with GRL_EVAL_TSNE
# ----------------------------------------------------------------------------
KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_CLUSTER', 'GRL_EVAL_CLUSTER_JACCARD', 'GRL_EVAL_KMEANS', 'GRL_EVAL_SILHOUETTE', 'GRL_EVAL_HDBSCAN',
         'GRL_EVAL_TSNE')


def test_attevaluator_adds_the_tsne_line_json_and_png(synth_models, monkeypatch, tmp_path):
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
    pids, cams = np.append(qp, gp), np.append(qc, gc)
    n, nq = gf.size(0), qf.size(0)
    path = str(tmp_path) + os.sep
    made, png, hdb = (os.path.join(str(tmp_path), f) for f in ('tsne.json', 'tsne.png', 'hdbscan.json'))

    def run():
        for f in (made, png):
            if os.path.exists(f):
                os.remove(f)
        with contextlib.redirect_stdout(io.StringIO()) as o:
            r = ev.evaluate(None, None, q_loader, g_loader, path, 0, 0)
        return r, o.getvalue().splitlines(), open(made).read() if os.path.exists(made) else None

    def refuse(c):
        raise ValueError('not strict JSON: %s' % c)

    # unset: the lines of today, no file
    monkeypatch.setenv('GRL_EVAL_HDBSCAN', '2,1')
    r_off, text_off, raw_off = run()
    assert raw_off is None and not os.path.exists(png) and not any('t-SNE' in l for l in text_off)
    # set: one line after the HDBSCAN lines, everything else unchanged
    monkeypatch.setenv('GRL_EVAL_TSNE', '2,20,1')
    r_on, text_on, raw = run()
    ts = engine.tsne(gf, 2.0, 'cosine', 20, 1)
    try:
        import matplotlib                                        # noqa: F401
        note = []
    except ImportError:
        note = ['t-SNE: matplotlib does not import, no tsne.png (the map is in tsne.json)']
    k = 1 + len(note)
    assert r_on == r_off and text_on[:-1 - k] + text_on[-1:] == text_off
    assert text_on[-1 - k] == 't-SNE: KL = {:.6g}, perplexity = 2, 20 iterations, {} isolated of {}'.format(
        ts.kl, ts.n_isolated, n)
    assert text_on[-k:-1] == note and text_on[-2 - k].startswith('Pairwise precision') and text_on[-3 - k].startswith('HDBSCAN:')
    js = json.loads(raw, parse_constant=refuse)
    emb = host(ts.embedding)
    assert js == {'perplexity': 2.0, 'n_iter': 20, 'seed': 1, 'metric': 'cosine', 'n': n, 'n_queries': nq, 'kl': ts.kl,
                  'n_isolated': ts.n_isolated,
                  'embedding': [[None if np.isnan(v) else float(v) for v in row] for row in emb],
                  'pids': [int(p) for p in pids], 'camids': [int(c) for c in cams]}
    # the rows are those of hdbscan.json's labels: a clustering colours the map without a join
    assert len(json.load(open(hdb))['labels']) == len(js['embedding']) == n
    assert os.path.exists(png) == (not note) and (note or open(png, 'rb').read(8) == b'\x89PNG\r\n\x1a\n')
    # alone, on the streaming route
    monkeypatch.delenv('GRL_EVAL_HDBSCAN')
    monkeypatch.setenv('GRL_EVAL_STREAM', '1')
    _, text, raw = run()
    assert text[-1 - k] == text_on[-1 - k] and json.loads(raw, parse_constant=refuse) == js
    # refused with the verification metric
    monkeypatch.setenv('GRL_EVAL_METRIC', 'verify')
    with pytest.raises(ValueError, match='GRL_EVAL_TSNE cannot be combined'):
        ev.evaluate(None, None, q_loader, g_loader, path, 0, 0)


# ----------------------------------------------------------------------------
# 8. the argument errors
# ----------------------------------------------------------------------------
def test_argument_errors():
    from grl_amd import engine
    c = case(24, 65)
    x = c['x']
    a = affinities(c)
    row_ptr, col, val = a['dev']
    for fn in (engine.tsne, engine.tsne_affinities):
        with pytest.raises(ValueError, match='2-d float32'):
            fn(x.view(65, 4, 6))
        with pytest.raises(ValueError, match='2-d float32'):
            fn(x.double())
        with pytest.raises(ValueError, match='n >= 3'):
            fn(x[:2])
        for bad in (True, 0.5, 64.0, 100.0, float('nan'), '30', None):
            with pytest.raises(ValueError, match='perplexity'):
                fn(x, bad)
        with pytest.raises(ValueError, match="'cosine' or 'euclidean'"):
            fn(x, metric='jaccard')
        with pytest.raises(ValueError, match='verify_metric'):
            fn(x, metric=engine.VerifyMetric.__new__(engine.VerifyMetric))
    with pytest.raises(ValueError, match='perplexity'):
        engine.tsne(torch.zeros((2000, 8), device=DEV), 341.0)
    for bad in (0, -1, True, 2.5):
        with pytest.raises(ValueError, match='n_iter'):
            engine.tsne(x, n_iter=bad)
        with pytest.raises(ValueError, match='n_iter'):
            engine.tsne_from_affinities(row_ptr, col, val, bad)
    for bad in (torch.zeros((65, 3), device=DEV), torch.zeros((64, 2), device=DEV), torch.zeros((65, 2)),
                torch.zeros((65, 2), device=DEV, dtype=torch.float64), 'pca', None):
        with pytest.raises(ValueError, match='init'):
            engine.tsne(x, init=bad)
    for kw in (dict(seed=-1), dict(seed=True), dict(learning_rate=0.0), dict(learning_rate='fast'),
               dict(early_exaggeration=0.0), dict(exaggeration_iter=-1)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            engine.tsne(x, **kw)
    # a caller's CSR: not square, not sorted, the wrong types
    y = dev(TR.init_random(65, 0))
    with pytest.raises(ValueError, match='not square'):
        engine.tsne_gradient(row_ptr[:-1], col, val, y[:64])
    with pytest.raises(ValueError, match='not square'):
        engine.tsne_gradient(row_ptr, torch.full_like(col, 65), val, y)
    swapped = col.clone()
    swapped[[0, 1]] = swapped[[1, 0]]
    with pytest.raises(ValueError, match='not sorted'):
        engine.tsne_gradient(row_ptr, swapped, val, y)
    with pytest.raises(ValueError, match='not sorted'):
        engine.tsne_from_affinities(row_ptr, swapped, val, 5)
    with pytest.raises(ValueError, match='col must be'):
        engine.tsne_gradient(row_ptr, col.long(), val, y)
    with pytest.raises(ValueError, match='y must be'):
        engine.tsne_gradient(row_ptr, col, val, y[:64])
    with pytest.raises(ValueError, match='isolated must be'):
        engine.tsne_gradient(row_ptr, col, val, y, isolated=torch.zeros(64, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError, match='first_iter'):
        engine.tsne_from_affinities(row_ptr, col, val, 5, first_iter=-1)
    with pytest.raises(ValueError, match='gains must be'):
        engine.tsne_from_affinities(row_ptr, col, val, 5, gains=torch.ones((64, 2), device=DEV))
