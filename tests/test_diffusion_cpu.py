"""Diffusion re-ranking without a GPU: the float32 host model of the kernels (tests/diffusion_ref.py, (a))
against the dense float64 solve (b), the exact identities of the definition, the manifold fixture, the bindings, the
argument checks that come before any device call and the GRL_EVAL_DIFFUSION knob.

The device results are held to model (a) bit for bit (tests/test_gpu_diffusion.py), so these tests pin the model itself.
The one tolerance, wherever float32 meets float64, is 4 x the model's own measured error (diffusion_ref.REL_ERR_*)."""
import os

import numpy as np
import pytest
import torch

import diffusion_ref as R

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANK_SEED = 1                     # the ranking fixture shared with the GPU test: feature_case(RANK_SEED, 7, 150)


def _graph(seed, ng=150, k=8, gamma=3, dtype=F32):
    qf, gf = R.feature_case(seed, 7, ng)[:2]
    sdist, sidx = R.host_search(gf, gf, k + 1)
    return qf, gf, R.mutual(sidx, sdist, k, gamma, dtype)


@pytest.mark.parametrize('alpha,recorded', [(0.9, R.REL_ERR_ALPHA_090), (0.99, R.REL_ERR_ALPHA_099)])
def test_model_against_the_dense_float64_solve(alpha, recorded):
    """The measurement behind the recorded constants, repeated: the converged float64 CG equals the dense solve, the
    float32 model's error is the recorded one (to the digits recorded: the constant is a measurement), and it is inside
    the sanity bound cond * 2^-24."""
    worst, cg = R.measure_model_error(alpha)
    cond = (1 + alpha) / (1 - alpha)
    print('alpha = %g: model (a) vs dense float64 %.3e (recorded %.3e, cond * 2^-24 = %.3e); float64 CG vs dense %.3e'
          % (alpha, worst, recorded, cond * 2.0 ** -24, cg))
    assert cg < 1e-12
    assert 0.9 * recorded < worst <= recorded
    assert recorded <= cond * 2.0 ** -24
    assert R.tolerance(alpha) == 4 * recorded
    # inputs beyond the seeds measured stay inside the 4 x tolerance
    assert R.measure_model_error(alpha, seeds=(11, 12))[0] <= R.tolerance(alpha)


def test_symmetry_of_s_is_bit_for_bit():
    for seed, k, gamma in ((0, 8, 3), (1, 5, 1), (2, 16, 8)):
        _, gf, (idx, a, deg, S) = _graph(seed, k=k, gamma=gamma)
        assert S.dtype == F32 and idx.dtype == np.int32
        edges = {}
        for i in range(idx.shape[0]):
            for t in range(k):
                if S[i, t] != 0:
                    edges[(i, int(idx[i, t]))] = S[i, t].view(np.uint32)
        assert edges
        for (i, j), bits in edges.items():
            assert edges.get((j, i)) == bits, (i, j)
        assert (S >= 0).all() and (a[S == 0] == 0).all()
        M = R.dense(idx, S)
        assert np.abs(np.linalg.eigvalsh(M)).max() <= 1 + 1e-6            # the spectrum of D^-1/2 A D^-1/2


def test_lists_drop_self_or_the_last_entry_and_keep_padding():
    # row 0: self first; row 1: self in the middle; row 2: self absent (duplicates tie before it): last entry dropped;
    # row 3: padding inside the list
    sidx = np.array([[0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 3, -1], [3, 0, -1, -1]], np.int64)
    sdist = -np.array([[1, .9, .8, .7], [.9, 1, .6, .5], [.8, .6, .4, 0], [1, .7, 0, 0]], F32)
    idx, a, deg, S = R.mutual(sidx, sdist, 3, 1)
    assert idx.tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, -1, -1]]
    # 0-3: row 3 keeps 0, row 0 keeps 3 -> min(.7, .7); 2-3: row 3 does not list 2 -> 0; 1-3: row 3 does not list 1
    assert a.tolist() == [[F32(.9), F32(.8), F32(.7)], [F32(.9), F32(.6), 0], [F32(.8), F32(.6), 0], [F32(.7), 0, 0]]
    assert deg[3] == F32(.7) and deg[0] == F32(F32(F32(.9) + F32(.8)) + F32(.7))
    # the last entry of a list without self is not kept, so it is no mutual edge either
    sidx = np.array([[1, 2, 3], [0, 1, 2], [0, 2, 1], [0, 3, 1]], np.int64)        # row 0: [1, 2, 3], no self
    sdist = -np.full((4, 3), 0.5, F32)
    idx, a, deg, S = R.mutual(sidx, sdist, 2, 2)
    assert idx[0].tolist() == [1, 2] and idx[3].tolist() == [0, 1]
    assert a[3, 0] == 0                                   # row 0 dropped 3 (its last entry), so 3-0 is not mutual
    assert a[0, 0] == F32(0.25) and a[1, 0] == F32(0.25)


def test_exact_identities():
    qf, gf, (idx, a, deg, S) = _graph(2)
    n = gf.shape[0]
    qdist, qidx = R.host_search(qf, gf, 3)
    y = R.seed_vector(qidx, qdist, n, 3)
    # alpha = 0: f = y exactly, whatever the number of iterations
    for n_iter in (1, 2, 20):
        assert np.array_equal(R.solve(idx, S, y, 0.0, n_iter).view(np.uint32), y.view(np.uint32))
    # n_iter = 0: f = 0, and the ranking is the index order
    f0 = R.solve(idx, S, y, 0.99, 0)
    assert not f0.any() and np.array_equal(R.rank(f0.T), np.broadcast_to(np.arange(n), (7, n)))
    # a zero column freezes at once and stays zero, without NaN
    y2 = y.copy()
    y2[:, 3] = 0
    f = R.solve(idx, S, y2, 0.99, 20)
    assert not f[:, 3].any() and np.isfinite(f).all()
    assert np.array_equal(f[:, :3].view(np.uint32), R.solve(idx, S, y, 0.99, 20)[:, :3].view(np.uint32))   # independent


def test_isolated_nodes_keep_f_equal_y():
    """A row whose similarities are all <= 0 has no edge: its row and column of S are zero.  In the dense solve its f is
    its y exactly; in the CG model an isolated node that is no seed stays exactly 0, and an isolated seed converges to
    its y within the recorded tolerance (CG reaches it through the column's shared step sizes)."""
    qf, gf = R.feature_case(3, 7, 80)[:2]
    gf = gf.copy()
    gf[5] = -gf[:40].sum(0)
    gf[5] /= np.linalg.norm(gf[5])
    sdist, sidx = R.host_search(gf, gf, 7)
    sdist[5, 1:] = np.abs(sdist[5, 1:])                   # (make every similarity of row 5 to another row <= 0)
    for dtype in (F32, np.float64):
        idx, a, deg, S = R.mutual(sidx, sdist, 6, 3, dtype)
        assert deg[5] == 0 and not S[5].any() and not S[idx == 5].any()
        y = np.zeros((80, 2), dtype)
        y[[1, 2, 3], 0] = (1.0, 0.5, 0.25)                # column 0: node 5 is no seed
        y[[5, 2], 1] = (0.75, 0.5)                        # column 1: node 5 is a seed
        ref = R.dense_solve(idx, S, y, 0.99)
        assert abs(ref[5, 0]) < 1e-15 and abs(ref[5, 1] - 0.75) < 1e-15
        f = R.solve(idx, S, y, 0.99, 120)
        assert f[5, 0] == 0
        assert abs(float(f[5, 1]) - 0.75) <= R.tolerance(0.99) * np.abs(ref[:, 1]).max()


def test_dot_products_have_the_kernels_partial_sum_ranges():
    g = np.random.Generator(np.random.PCG64(5))
    for n in (1, 16, 17, 64, 65, 257):
        u, v = g.standard_normal((n, 3)).astype(F32), g.standard_normal((n, 3)).astype(F32)
        part = R.dot_partials(u, v)
        assert part.shape == (-(-n // 64), 3) and part.dtype == F32
        want = np.zeros_like(part)
        for blk in range(part.shape[0]):
            waves = []
            for w in range(4):
                acc = np.zeros(3, F32)
                for i in range(blk * 64 + w * 16, min(blk * 64 + w * 16 + 16, n)):
                    acc = acc + u[i] * v[i]
                waves.append(acc)
            want[blk] = ((waves[0] + waves[1]) + waves[2]) + waves[3]
        assert np.array_equal(part.view(np.uint32), want.view(np.uint32))
    # the order matters: 2^24 + 1 - 2^24 across two waves' rows
    u = np.zeros((64, 1), F32)
    u[0], u[1], u[16] = 2.0 ** 24, 1.0, -2.0 ** 24
    assert R.finish(R.dot_partials(u, np.ones_like(u)))[0] == 0.0          # wave 0: 2^24 + 1 -> 2^24; + wave 1 -> 0


def test_ranking_fixture_stays_under_the_cap_against_the_float64_yardstick():
    """The GPU test compares diffusion_search with (b) under tests/ranking_check.py's rule; the model itself must pass
    it on the same fixture: positions differ only where (b)'s scores are closer than the tolerance, and in at most 1 % of
    the positions."""
    qf, gf = R.feature_case(RANK_SEED, 7, 150)[:2]
    for alpha, n_iter in ((0.99, 150), (0.9, 60)):
        ref = R.diffuse(qf, gf, 8, 3, 3, alpha, n_iter, np.float64, dense_yardstick=True)
        f = R.diffuse(qf, gf, 8, 3, 3, alpha, n_iter)
        assert R.relative_error(f, ref) <= R.tolerance(alpha)
        n_diff, gap = R.ranking_differences(R.rank(f), R.rank(ref), ref, R.tolerance(alpha))
        print('alpha = %g: %d of %d positions differ, largest gap %.3e' % (alpha, n_diff, ref.size, gap))
        assert gap <= R.tolerance(alpha) and n_diff <= 0.01 * ref.size
        assert (ref > 0).mean() > 0.5                          # the scores reach most of the gallery: not a ranking of ties


def test_manifold_case_ranks_every_match_above_every_distractor_where_cosine_does_not():
    qf, gf, qp, qc, gp, gc, matches, distractors = R.manifold_case()
    cos = (qf @ gf.T)[0]
    assert cos[distractors].min() > cos[matches].max()          # plain cosine: every distractor before every match
    assert np.allclose(np.linalg.norm(gf, axis=1), 1.0, atol=1e-6)
    ref = R.diffuse(qf, gf, 4, 3, 3, 0.99, 0, np.float64, dense_yardstick=True)[0]
    assert ref[matches].min() > ref[distractors].max() and ref[matches].min() > 0
    f = R.diffuse(qf, gf, 4, 3, 3, 0.99, 20)[0]                 # the model at the defaults' iteration count
    assert f[matches].min() > f[distractors].max()
    order = R.rank(f[None])[0]
    pos = {int(g): p for p, g in enumerate(order)}
    assert max(pos[int(m)] for m in matches) < min(pos[int(d)] for d in distractors)
    # the junk rule leaves the matches at the top: the query and its near tracklets share pid and camera
    kept = [int(g) for g in order if not (gp[g] == qp[0] and gc[g] == qc[0])]
    assert sorted(kept[:3]) == sorted(int(m) for m in matches)


def test_library_exports_and_header_declare_the_entry_points():
    import ctypes
    from grl_amd import _lib
    names = ('grl_diffusion_mutual', 'grl_diffusion_part_rows', 'grl_diffusion_apply', 'grl_diffusion_seed',
             'grl_diffusion_workspace_floats', 'grl_diffusion_solve', 'grl_diffusion_transpose')
    header = open(os.path.join(ROOT, 'include', 'grl_hip.h')).read()
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        assert name in _lib.exported_symbols() and getattr(lib, name).restype is not None
        assert hasattr(raw, name) and name + '(' in header
    assert lib.grl_abi_version() == 10
    assert lib.grl_diffusion_part_rows() == R.PART_ROWS
    assert 'diffusion.hip' in open(os.path.join(ROOT, 'grl_amd', 'csrc', 'Makefile')).read()
    # workspace: p, Ap, the partials and three per-column arrays, each rounded up to 4 floats
    assert lib.grl_diffusion_workspace_floats(67, 3) == 2 * 204 + 8 + 3 * 4
    assert lib.grl_diffusion_workspace_floats(0, 3) == 0
    # the argument checks come before any HIP call: fake (never dereferenced) pointers
    E = _lib.GRL_EINVAL
    assert lib.grl_diffusion_mutual(None, None, 9, 4, 8, 3, None, None, 8, None, None) == E
    a = (0x1000, 0x2000)
    for ldl, n, k, gamma, ldo in ((9, 4, 0, 3, 8), (9, 4, 129, 3, 200), (9, 4, 8, 0, 8), (9, 4, 8, 9, 8), (8, 4, 8, 3, 8),
                                  (9, 0, 8, 3, 8), (9, 4, 8, 3, 7)):
        assert lib.grl_diffusion_mutual(*a, ldl, n, k, gamma, 0x3000, 0x4000, ldo, 0x5000, None) == E, (ldl, n, k, gamma)
    g = (0x1000, 0x2000, 8, 4, 8)
    assert lib.grl_diffusion_apply(*g, 0x3000, 0, 0.5, 0x4000, 0x5000, None) == E               # B = 0
    assert lib.grl_diffusion_apply(*g, 0x3000, 2, 0.5, 0x3000, 0x5000, None) == E               # Ap is p
    assert lib.grl_diffusion_apply(0x1000, 0x2000, 7, 4, 8, 0x3000, 2, 0.5, 0x4000, 0x5000, None) == E    # ldg < k
    for alpha, n_iter in ((1.0, 3), (-0.1, 3), (float('nan'), 3), (0.5, -1)):
        assert lib.grl_diffusion_solve(*g, 0x3000, 2, alpha, n_iter, 0x4000, 0x5000, None) == E, (alpha, n_iter)
    assert lib.grl_diffusion_seed(0x1000, 0x2000, 2, 3, 3, 4, 0, 0x3000, None) == E             # lds < kq
    assert lib.grl_diffusion_seed(0x1000, 0x2000, 3, 3, 3, 4, 9, 0x3000, None) == E             # gamma
    assert lib.grl_diffusion_transpose(0x1000, 4, 3, 1, 0x2000, 3, None) == E                   # ldo < n


def test_arguments_are_refused_before_the_device(monkeypatch):
    from grl_amd import engine

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    monkeypatch.setattr(engine, '_call', no_device)
    monkeypatch.setattr(engine, 'search', no_device)
    host = torch.zeros(6, 32)
    # non-device tensors
    with pytest.raises(ValueError, match='HIP device'):
        engine.diffusion_graph(host)
    with pytest.raises(ValueError, match='HIP device'):
        engine.diffusion_search(host, host, 5)
    with pytest.raises(ValueError, match='HIP device'):
        engine.diffusion_metrics_streaming(host, host, [0] * 6, [0] * 6, [0] * 6, [0] * 6)
    # ranges come first, so host tensors reach them
    for k in (0, 129, -1, 2.0, '5', None, True):
        with pytest.raises(ValueError, match='k must be'):
            engine.diffusion_graph(host, k)
        with pytest.raises(ValueError, match='k must be'):
            engine.diffusion_search(host, host, 5, k=k)
    for gamma in (0, 9, 1.5, None):
        with pytest.raises(ValueError, match='gamma must be'):
            engine.diffusion_graph(host, 5, gamma)
    with pytest.raises(ValueError, match="metric must be 'cosine'"):
        engine.diffusion_graph(host, 5, metric='euclidean')
    vm = engine.VerifyMetric.__new__(engine.VerifyMetric)
    with pytest.raises(ValueError, match='not a distance between two samples of one set'):
        engine.diffusion_graph(host, 5, metric=vm)
    assert engine.DIFFUSION_K_MAX == 128 and engine.DIFFUSION_GAMMA_MAX == 8
    g = engine.DiffusionGraph(torch.zeros((0, 5), dtype=torch.int32), torch.zeros((0, 5)), torch.zeros(0), 0, 5, 3)
    assert (g.n_edges, g.n_isolated) == (0, 0)
    si, sv = torch.zeros((2, 3), dtype=torch.int64), torch.zeros((2, 3))
    for alpha in (1.0, -0.01, float('nan'), 1.5, None, '0.5', 1 - 1e-9):          # (1 - 1e-9 is 1 in float32)
        with pytest.raises(ValueError, match='alpha must'):
            engine.diffusion_solve(g, si, sv, alpha)
    for n_iter in (-1, 2.5, None, '3'):
        with pytest.raises(ValueError, match='n_iter must be'):
            engine.diffusion_solve(g, si, sv, 0.5, n_iter)
    with pytest.raises(ValueError, match='seed_idx'):
        engine.diffusion_solve(g, si, sv)                                          # host seed lists
    with pytest.raises(ValueError, match='DiffusionGraph'):
        engine.diffusion_solve(None, si, sv)


def test_the_evaluator_knob_parses():
    from grl_amd.reid.evaluator.attevaluator import parse_diffusion_knob as parse
    name = 'GRL_EVAL_DIFFUSION'
    assert parse(name, None) is None and parse(name, '') is None and parse(name, ' ') is None
    assert parse(name, '50') == (50, 10, 0.99, 20)
    assert parse(name, '5') == (5, 5, 0.99, 20)                      # the default kq never exceeds k
    assert parse(name, '50,7') == (50, 7, 0.99, 20)
    assert parse(name, ' 50 , 7 , 0.9 ') == (50, 7, 0.9, 20)
    assert parse(name, '128,128,0,0') == (128, 128, 0.0, 0)
    for bad in ('x', '50,', ',3', '50,10,0.9,20,1', '3.5', '50;3', '0', '129', '-2', '50,51', '50,0', '50,10,1',
                '50,10,1.0', '50,10,-0.1', '50,10,nan', '50,10,0.9,-1', '50,10,0.9,2.5'):
        with pytest.raises(ValueError, match=name):
            parse(name, bad)


def test_the_knob_is_refused_with_rerank_or_another_metric_before_any_extraction(monkeypatch):
    from grl_amd.reid.evaluator import ATTEvaluator
    ev = ATTEvaluator(None, None, only_eval=False)

    def no_extract(loader):
        raise AssertionError('features were extracted')
    monkeypatch.setattr(ev, 'extract_feature', no_extract)
    for name in ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
                 'GRL_EVAL_DIFFUSION'):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv('GRL_EVAL_DIFFUSION', '50,x')
    with pytest.raises(ValueError, match='GRL_EVAL_DIFFUSION'):
        ev.evaluate(None, None, [], [], '', 0, 0)
    monkeypatch.setenv('GRL_EVAL_DIFFUSION', '50')
    with pytest.raises(ValueError, match='GRL_EVAL_DIFFUSION cannot re-rank'):
        ev.evaluate(None, None, [], [], '', 0, 1)
    monkeypatch.setenv('GRL_EVAL_METRIC', 'verify')
    with pytest.raises(ValueError, match='GRL_EVAL_DIFFUSION cannot be combined with GRL_EVAL_METRIC=verify'):
        ev.evaluate(None, None, [], [], '', 0, 0)
    monkeypatch.delenv('GRL_EVAL_METRIC')
    monkeypatch.setenv('GRL_EVAL_ROC', '1')
    with pytest.raises(ValueError, match='GRL_EVAL_DIFFUSION cannot be combined with GRL_EVAL_ROC'):
        ev.evaluate(None, None, [], [], '', 0, 0)
    monkeypatch.delenv('GRL_EVAL_ROC')
    with pytest.raises(AssertionError, match='features were extracted'):       # accepted: it gets as far as extraction
        ev.evaluate(None, None, [], [], '', 0, 0)
