"""The float64 model of the cluster-memory update and loss (tests/cmem_ref.py) is right, its bounds are satisfiable and the
host side of unsupervised training keeps its books -- all shown without a GPU:

* the properties of the update model (only present labels change, -1 and K ignored, the first-index tie rule, momentum 1 and
  0, hard = mean for single-member clusters), and the loss model against torch float64 autograd;
* the SELECTION-GAP CONDITION, on the float64 reference alone: for every hard-mode case the GPU file compares with a float64
  selection, the gap between the smallest and the second smallest similarity of every cluster exceeds 4 x the first-order
  fp32 bound of one similarity.  No case is excluded;
* the fp32 numpy restatement of the kernel's summation order inside the very bounds the GPU test holds the kernel to;
* PseudoLabels from host labels, the relabelled list under RandomPairSamplerForMars, and every refusal that fires before a
  device call (fake pointers through the C ABI, as test_sq8_cpu.py)."""
import os
import re

import numpy as np
import pytest
import torch

import cmem_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


@pytest.fixture(scope='module', autouse=True)
def _ratios():
    yield
    R.dump_ratios('fp32 numpy restatement of the cluster-memory update (CPU)')


def _unit(a):
    return a / np.sqrt((a * a).sum(-1, keepdims=True))


# ----------------------------------------------------------------------------------------------------------------------
# the sweep
def test_sweep_takes_both_sides_of_every_branch():
    from head_bounds import lane_trips
    t = [lane_trips(D, 1024) for D in R.UPD_D]
    assert {(0, 1), (1, 1), (1, 2), (2, 3)} <= set(t)                      # lanes with no trip, one, two, three
    assert any(D // 4 % 64 for D in R.UPD_D) and min(R.UPD_D) == 4
    assert min(R.UPD_N) == 1 and max(R.UPD_N) > 32 and min(R.UPD_K) == 1
    rng = R.rng_for(1)
    for n in (9, 33):
        y = R.labels_for(n, 70, 'mixed', rng)
        assert y[0] == -1 and y[-1] == 70 and ((y >= 0) & (y < 70)).sum() == n - 2
        assert len(set(R.labels_for(n, 70, 'distinct'))) == n and len(set(R.labels_for(n, 3, 'equal'))) == 1
        assert (R.labels_for(n, 3, 'distinct') >= 3).sum() == n - 3        # distinct labels past K fall outside the memory
        y = R.labels_for(n, 3, 'pairs')                                     # members that are not adjacent, a leader that is not row 0
        assert (np.diff(np.flatnonzero(y == 0)) > 1).any() and np.flatnonzero(y == 1)[0] == 2
    assert not ((R.labels_for(1, 3, 'mixed', rng) >= 0).any())             # a batch with no valid label at all
    assert len(list(R.hard_cases())) == len(R.UPD_CASES) * len(R.UPD_K) * len(R.UPD_PATTERNS) + 2 * len(R.LOSS_K)


# ----------------------------------------------------------------------------------------------------------------------
# the model's properties
@pytest.mark.parametrize('mode', R.MODES)
def test_only_rows_of_present_labels_change_and_out_of_range_labels_are_ignored(mode):
    d = R.in_update(9, 260, 70, 'mixed')
    ref = R.cmem_update(d['cent'], d['x'], d['labels'], 9, 260, 70, 0.2, mode)
    present = set(int(v) for v in d['labels'] if 0 <= v < 70)
    assert d['labels'][0] == -1 and d['labels'][-1] == 70 and present
    for k in range(70):
        same = np.array_equal(ref['cent'][k], d['cent'][k].astype(np.float64))
        assert same == (k not in present), k
    assert ref['sel'][0] == 0 and ref['sel'][-1] == 0
    assert {st['row'] for st in ref['steps']} == present
    assert np.allclose((ref['cent'] ** 2).sum(1), 1.0, atol=1e-6)
    # the result of a row does not depend on the batch's other labels
    keep = d['labels'] == ref['steps'][0]['row']
    alone = R.cmem_update(d['cent'], d['x'][keep], d['labels'][keep], int(keep.sum()), 260, 70, 0.2, mode)
    assert np.array_equal(alone['cent'][ref['steps'][0]['row']], ref['cent'][ref['steps'][0]['row']])
    assert np.array_equal(alone['sel'], ref['sel'][keep])


def test_selection_is_the_least_similar_member_and_the_first_index_wins_ties():
    d = R.in_tie(256)
    ref = R.cmem_update(d['cent'], d['x'], d['labels'], 7, 256, 3, 0.2, R.HARD)
    assert ref['sel'].tolist() == [0, 0, 1, 1, 0, 0, 0]                    # sample 2, not its copy 5; cluster 0 has one member
    st = [s for s in ref['steps'] if s['row'] == 1][0]
    assert st['pick'] == d['first'] and st['s'][2] == st['s'][4] == st['s'].min() and st['gap'] == 0.0
    assert st['s'][0] == st['s'][3]                                         # samples 0 and 4: a tie that is not the minimum
    # every other member is further from the minimum than 4 x the bound of a similarity: the device must see the same two
    for D in R.TIE_D:
        d = R.in_tie(D)
        st = [s for s in R.cmem_update(d['cent'], d['x'], d['labels'], 7, D, 3, 0.2, R.HARD)['steps'] if s['row'] == 1][0]
        others = np.delete(st['s'], [2, 4])
        assert st['pick'] == 2 and others.min() - st['s'].min() > R.GAP_FACTOR * float(R.e_similarity(st, D).max())
    d = R.in_tie(256)
    assert R.pick_least(np.array([np.nan, -1.0, -2.0])) == 0               # a NaN running best is never replaced ...
    assert R.pick_least(np.array([0.5, np.nan, 0.25, np.nan])) == 2        # ... and a NaN never replaces
    mean = R.cmem_update(d['cent'], d['x'], d['labels'], 7, 256, 3, 0.2, R.MEAN)
    assert mean['sel'].tolist() == [1] * 7


@pytest.mark.parametrize('mode', R.MODES)
def test_momentum_one_keeps_the_direction_and_momentum_zero_gives_the_normalised_v(mode):
    d = R.in_update(9, 252, 3, 'pairs')
    c0 = d['cent'].astype(np.float64)
    one = R.cmem_update(d['cent'], d['x'], d['labels'], 9, 252, 3, 1.0, mode)
    assert np.abs(one['cent'] - _unit(c0)).max() < TOL
    zero = R.cmem_update(d['cent'], d['x'], d['labels'], 9, 252, 3, 0.0, mode)
    for st in zero['steps']:
        assert np.abs(zero['cent'][st['row']] - _unit(st['v'])).max() < TOL
        X = d['x'].astype(np.float64)[st['members']]
        if mode == R.HARD:
            assert np.array_equal(st['v'], X[np.argmin(X @ c0[st['row']])])
        else:
            assert np.abs(st['v'] - X.mean(0)).max() < TOL


def test_hard_equals_mean_when_every_cluster_has_one_member():
    d = R.in_update(33, 260, 70, 'distinct')
    a = R.cmem_update(d['cent'], d['x'], d['labels'], 33, 260, 70, 0.2, R.HARD)
    b = R.cmem_update(d['cent'], d['x'], d['labels'], 33, 260, 70, 0.2, R.MEAN)
    assert np.array_equal(a['cent'], b['cent']) and np.array_equal(a['sel'], b['sel']) and a['sel'].all()


@pytest.mark.parametrize('K', R.LOSS_K)
def test_loss_model_against_torch_float64(K):
    import torch.nn.functional as TF
    d = R.in_loss(K)
    n, D = R.LOSS_N, R.LOSS_D
    ref = R.loss(d['x'], d['cent'], d['labels'], n, D, K, R.LOSS_TEMP, g=0.75)
    x = torch.from_numpy(d['x'].astype(np.float64)).requires_grad_(True)
    z = x @ torch.from_numpy(d['cent'].astype(np.float64)).t() * float(np.float32(1.0 / R.LOSS_TEMP))
    y = torch.from_numpy(np.where((d['labels'] >= 0) & (d['labels'] < K), d['labels'], -100))
    loss = TF.cross_entropy(z, y, ignore_index=-100)
    assert abs(ref['loss'] - loss.item()) < 1e-12 * (1 + abs(loss.item()))
    assert np.abs(ref['logits'] - z.detach().numpy()).max() < 1e-12 * 20
    dx = torch.autograd.grad(loss, x, torch.tensor(0.75, dtype=torch.float64))[0].numpy()
    assert np.abs(ref['dx'] - dx).max() < 1e-12 * (1 + np.abs(dx).max())
    assert (d['labels'] == -1).sum() == 1 and not ref['dx'][4].any()      # the noise row: weight 0, no gradient


# ----------------------------------------------------------------------------------------------------------------------
# the selection-gap condition (a condition, not a tolerance) and the bounds' satisfiability
def test_selection_gap_condition_holds_for_every_hard_case():
    worst, seen = np.inf, 0
    for what, d, n, D, K in R.hard_cases():
        ref = R.cmem_update(d['cent'], d['x'], d['labels'], n, D, K, 0.2, R.HARD)
        for st in ref['steps']:
            if st['count'] > 1:
                seen += 1
                bound = float(R.e_similarity(st, D).max())
                assert st['gap'] > R.GAP_FACTOR * bound, (what, st['row'], st['gap'], bound)
                worst = min(worst, st['gap'] / bound)
        assert R.gap_ok(ref, D), what
    print('\nselection gap / bound of one similarity: smallest %.1f over %d clusters with two or more members' % (worst, seen))
    assert seen > 300


@pytest.mark.parametrize('n,D', R.UPD_CASES)
def test_fp32_restatement_is_inside_the_bounds(n, D):
    for K in R.UPD_K:
        for pattern in R.UPD_PATTERNS:
            d = R.in_update(n, D, K, pattern)
            for momentum in R.UPD_MOMENTA:
                for mode in R.MODES:
                    what = (n, D, K, pattern, momentum, mode)
                    ref = R.cmem_update(d['cent'], d['x'], d['labels'], n, D, K, momentum, mode)
                    got = R.cmem_update_f32(d['cent'], d['x'], d['labels'], n, D, K, momentum, mode)
                    assert np.array_equal(got['sel'], ref['sel']), what
                    bd = R.b_cmem_update(ref, D, momentum, mode)
                    for k in range(K):
                        if k in bd:
                            R.check('cmem_update %s' % ('hard', 'mean')[mode], got['cent'][k], ref['cent'][k], bd[k], what + (k,))
                        else:
                            assert np.array_equal(got['cent'][k].view(np.uint32), d['cent'][k].view(np.uint32)), what + (k,)


def test_planted_rows_are_separable_by_the_host_models():
    """the labelling case of the GPU file: the host models of DBSCAN on the cosine and on the Jaccard distance recover the
    planted partition with the outliers as noise, with room to spare on both thresholds"""
    import cluster_ref as CR
    import jaccard_ref as J
    x, pids = R.planted()
    n = pids.size
    assert n == 63 and (pids >= 100).sum() == 3
    dots = x.astype(np.float64) @ x.astype(np.float64).T
    same = (pids[:, None] == pids[None, :]) & ~np.eye(n, dtype=bool)
    assert dots[same].min() > 0.85 and dots[pids[:, None] != pids[None, :]].max() < 0.38
    Jm = J.dense_matrices(J.euclid(x), R.PLANT_JACCARD['k1'], R.PLANT_JACCARD['k2'])[3]
    assert Jm[same].max() < 0.1 and Jm[pids[:, None] != pids[None, :]].min() > 0.9
    rp, col, _ = J.threshold(Jm, R.PLANT_JACCARD['eps'])
    for labels in (CR.dbscan(n, 4, A=CR.edges(-dots.astype(np.float32), R.PLANT_COSINE['eps']))[0],
                   CR.dbscan(n, 4, row_ptr=rp, col=col)[0]):
        assert (labels[pids >= 100] == -1).all() and (labels[pids < 100] >= 0).all() and labels.max() == 5
        assert all(len(set(labels[pids == p])) == 1 for p in range(6))


# ----------------------------------------------------------------------------------------------------------------------
# PseudoLabels from host labels (no device)
TRACKLETS = [(('t%d_a.jpg' % i, 't%d_b.jpg' % i), 1000 + i, i % 3) for i in range(12)]
HOST = np.array([5, 5, -1, 9, 2, 9, 5, -1, 2, 2, 9, 5], np.int64)          # ids 2, 5, 9 -> 0, 1, 2


def test_pseudo_labels_bookkeeping_from_host_labels():
    from grl_amd.reid.train.pseudo import PseudoLabels
    from grl_amd.reid.data.sampler import RandomPairSamplerForMars
    pl = PseudoLabels(HOST)
    assert pl.n_clusters == 3 and pl.n_noise == 2 and len(pl) == 12
    assert pl.host.tolist() == [1, 1, -1, 2, 0, 2, 1, -1, 0, 0, 2, 1]      # compact ids, ascending in the ids given
    assert pl.host.dtype == np.int64 and pl.labels.dtype == torch.int64 and pl.labels.tolist() == pl.host.tolist()
    assert pl.keep.tolist() == [0, 1, 3, 4, 5, 6, 8, 9, 10, 11]
    out = pl.relabel(TRACKLETS)
    assert [t[0] for t in out] == [TRACKLETS[i][0] for i in pl.keep]       # noise dropped, order kept
    assert [t[1] for t in out] == [1, 1, 2, 0, 2, 1, 0, 0, 2, 1] and [t[2] for t in out] == [TRACKLETS[i][2] for i in pl.keep]
    assert all(isinstance(t[1], int) for t in out)
    # already compact labels are kept as they are (the device tensor of a clustering is not copied)
    t = torch.tensor([0, 1, -1, 1, 0])
    assert PseudoLabels(t).labels is t and PseudoLabels(t).n_clusters == 2
    assert PseudoLabels(np.array([-1, -7, -1])).n_clusters == 0 and PseudoLabels(np.array([-3, 4])).host.tolist() == [-1, 0]
    # the sampler takes the list unchanged: every (anchor, positive) pair shares the pseudo-label
    torch.manual_seed(0); np.random.seed(0)
    idx = list(RandomPairSamplerForMars(out))
    assert len(idx) == 2 * len(out) and sorted(idx[0::2]) == list(range(len(out)))
    assert all(out[a][1] == out[b][1] for a, b in zip(idx[0::2], idx[1::2]))
    assert any(a != b for a, b in zip(idx[0::2], idx[1::2]))
    # pair_scores against hidden identities: the host's own count
    pids = np.array([0, 0, 7, 1, 2, 1, 0, 8, 2, 2, 1, 0])
    s = pl.pair_scores(pids)
    assert s['ari'] == 1.0 and s['precision'] == 1.0 and s['recall'] == 1.0 and s['n'] == 12
    assert pl.pair_scores(np.arange(12) % 2)['ari'] < 0.5
    with pytest.raises(ValueError, match='12 labels'):
        pl.relabel(TRACKLETS[:5])
    with pytest.raises(ValueError, match='labels must be n integers'):
        PseudoLabels(np.zeros(4))
    with pytest.raises(ValueError, match='labels must be n integers'):
        PseudoLabels(np.zeros((2, 2), np.int64))


class _Stub(object):
    def __init__(self, labels):
        self.labels = torch.as_tensor(labels, dtype=torch.int64)


def test_refusals_fire_before_any_device_call(monkeypatch):
    from grl_amd import engine
    from grl_amd.reid.loss import ClusterMemoryLoss, memory
    from grl_amd.reid.train import pseudo

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    for name in ('_call', 'gemm', 'cluster', 'cluster_jaccard', 'hdbscan', 'kmeans', 'cluster_centroids'):
        monkeypatch.setattr(engine, name, no_device)
    monkeypatch.setattr(memory, '_call', no_device)
    xf = torch.zeros((8, 16))
    with pytest.raises(ValueError, match="method must be one of 'jaccard', 'cosine', 'hdbscan', 'kmeans' .got 'dbscan'"):
        pseudo.pseudo_labels(xf, method='dbscan')
    with pytest.raises(ValueError, match="'kmeans' needs k"):
        pseudo.pseudo_labels(xf, method='kmeans')
    # fewer than two clusters: the message names the method and its threshold
    calls = []
    for method, fn, labels, pattern in (
            ('cosine', 'cluster', [-1] * 8, r"'cosine' with eps = -0\.7, min_samples = 4 found 0 cluster.*8 noise"),
            ('jaccard', 'cluster_jaccard', [0, 0, 0, 0, 0, -1, -1, 0], r"'jaccard' with eps = 0\.5, min_samples = 4 found 1 cluster"),
            ('hdbscan', 'hdbscan', [-1] * 8, r"'hdbscan' with min_cluster_size = 5 found 0"),
            ('kmeans', 'kmeans', [2] * 8, r"'kmeans' with k = 3 found 1 cluster")):
        monkeypatch.setattr(engine, fn, lambda *a, _l=labels, **k: calls.append(a[1:]) or _Stub(_l))
        with pytest.raises(ValueError, match=pattern):
            pseudo.pseudo_labels(xf, method=method, k=3, **({'eps': -0.7} if method == 'cosine' else {}))
    assert calls == [(-0.7, 4, 'cosine'), (0.5, 4, 20, 6), (5,), (3, 'cosine')]      # the arguments each engine call received
    monkeypatch.setattr(engine, 'cluster', lambda *a, **k: _Stub([0, 0, 1, 1, -1, 1, 0, 1]))
    ok = pseudo.pseudo_labels(xf, method='cosine', eps=-0.7)
    assert ok.n_clusters == 2 and ok.n_noise == 1 and ok.method == 'cosine'
    with pytest.raises(ValueError, match=r"cols = \(8, 40\) is no column range of 16"):
        ok.centroids(xf, cols=(8, 40))
    # ClusterMemoryLoss: the constructor and reset name what is wrong
    with pytest.raises(ValueError, match="mode must be 'hard', 'mean' or 'instance' .got 'soft'"):
        ClusterMemoryLoss(16, 4, mode='soft')
    with pytest.raises(ValueError, match='temp must be > 0'):
        ClusterMemoryLoss(16, 4, temp=0.0)
    crit = ClusterMemoryLoss(16, 4)
    assert tuple(crit.centroids.shape) == (4, 16) and crit.centroids.dtype == torch.float32 and 'centroids' in crit.state_dict()
    for bad, pattern in ((torch.zeros((3, 16), dtype=torch.float64), 'centroids must be a float32 tensor .got torch.float64'),
                         (np.zeros((3, 16), np.float32), 'centroids must be a float32 tensor .got ndarray'),
                         (torch.zeros((3, 20)), r'centroids must be \[K >= 1, num_features = 16\] .got \(3, 20\)'),
                         (torch.zeros(16), r'centroids must be \[K >= 1, num_features = 16\]'),
                         (torch.zeros((0, 16)), r'centroids must be \[K >= 1, num_features = 16\]'),
                         (torch.zeros((3, 16)), 'centroids must be on a HIP device .got cpu')):
        with pytest.raises(ValueError, match='ClusterMemoryLoss.reset: ' + pattern):
            crit.reset(bad)
    assert crit.num_clusters == 4 and tuple(crit.centroids.shape) == (4, 16)           # a refused reset changes nothing


def test_train_unsupervised_refuses_a_loader_that_does_not_give_one_row_per_tracklet():
    from grl_amd.reid.train.pseudo import train_unsupervised

    class Ev(object):
        def extract_feature(self, loader):
            return torch.zeros((3, 6144)), None, None
    with pytest.raises(ValueError, match=r'features \(3, 6144\) for 12 tracklets'):
        train_unsupervised(None, Ev(), None, TRACKLETS, lambda t: t, lambda t: t, 1)


# ----------------------------------------------------------------------------------------------------------------------
# the C ABI
def test_header_binding_and_library_carry_the_entry_point():
    from grl_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'grl_hip.h')).read()
    assert re.search(r'int\s+grl_cmem_update\(float\* cent, const float\* x, const int64_t\* labels, int n, int D, int K, '
                     r'float momentum, int mode,\s+int32_t\* sel, void\* stream\);', src)
    assert int(re.search(r'#define\s+GRL_ABI_VERSION\s+(\d+)', src).group(1)) == 10 == _lib.ABI_VERSION
    assert 'grl_cmem_update' in _lib.exported_symbols()
    assert 'cmem.hip' in open(os.path.join(ROOT, 'grl_amd', 'csrc', 'Makefile')).read()


def test_host_argument_checks_return_einval_through_the_c_abi():
    import ctypes as C
    from grl_amd import _lib
    lib = _lib.load()
    E = _lib.GRL_EINVAL
    # fake device pointers (never dereferenced: every call below is refused before the launch)

    def upd(cent=0x1000, x=0x2000, labels=0x3000, n=2, D=8, K=3, m=0.2, mode=0, sel=0x4000):
        return lib.grl_cmem_update(cent, x, labels, n, D, K, C.c_float(m), mode, sel, None)
    for kw in (dict(cent=None), dict(x=None), dict(labels=None), dict(n=0), dict(n=-1), dict(D=0), dict(D=6), dict(D=-4),
               dict(K=0), dict(mode=2), dict(mode=-1), dict(cent=0x1004), dict(x=0x2008)):
        assert upd(**kw) == E, kw
        assert b'cmem_update' in lib.grl_last_error()
