"""The float64 model of the camera-aware proxy cross entropy (tests/proxy_ref.py) is right and the host side of camera-aware
training keeps its books -- all shown without a GPU:

* the model's own identities: with one camera, one proxy per cluster and k_neg >= P both terms are the plain cross entropy
  over all P columns; the gradient's rows sum to 0 over each set; finite differences of the loss against the gradient; the
  planted ties;
* the sweep reaches every label pattern the GPU file has to cover;
* the SELECTION-GAP CONDITION of the ProxyMemoryLoss cases, on the float64 reference alone: with the seed `loss_seed` picks,
  every row's gap between the last admitted and the first refused negative exceeds 4 x the bound of one logit.  No row is
  excluded -- and a fixed seed would not do (printed);
* ProxyLabels numbering and noise handling, and every refusal that fires before a device call;
* SEQTrainer._forward calls its three identity criteria through _id_loss; CameraSEQTrainer hands them the cameras in the
  targets' row order."""
import os
import re

import numpy as np
import pytest
import torch

import proxy_ref as R
import loss_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------------------------------------
# the model
@pytest.mark.parametrize('P', (1, 3, 70))
def test_one_camera_one_proxy_per_cluster_and_all_negatives_is_the_plain_cross_entropy(P):
    n = 9
    r = R.rng_for('plain', P)
    z = R.f32(5.0 * r.standard_normal((n, P)))
    y = r.randint(0, P, n).astype(np.int64)
    y[2] = -1
    pcl, pcm = np.arange(P).astype(np.int32), np.zeros(P, np.int32)
    plain = LR.softmax_ce(z.reshape(-1), P, y, None, n, P)
    for w in ((1.0, 0.0), (0.0, 1.0)):
        ref = R.proxy_ce(z.reshape(-1), P, y, np.zeros(n, np.int64), pcl, pcm, n, P, P, *w)
        assert abs(ref['loss'] - plain['loss']) < 1e-12 * (1 + abs(plain['loss']))
        assert np.abs(ref['dz'] - plain['dz_val']).max() < 1e-14
        assert ref['correct'] == plain['correct'] and ref['nv'] == n - 1
        assert np.array_equal(ref['own'], np.where(y >= 0, y, -1)) and not ref['dz'][2].any()
    both = R.proxy_ce(z.reshape(-1), P, y, np.zeros(n, np.int64), pcl, pcm, n, P, P, 1.0, 0.5)
    assert abs(both['loss'] - 1.5 * plain['loss']) < 1e-12 * (1 + abs(plain['loss']))


def test_gradient_rows_sum_to_zero_over_each_set_and_match_finite_differences():
    n, P, C, k = 9, 70, 6, 3
    d = R.in_ce(n, P, C, 'mixed', wide=False)
    z64 = d['logits'].astype(np.float64).reshape(n, P)
    for w in R.CE_WEIGHTS:
        ref = R.proxy_ce(z64.reshape(-1), P, d['labels'], d['cams'], d['pcl'], d['pcm'], n, P, k, *w)
        assert 2 <= ref['nv'] < n
        for i, rec in ref['r'].items():
            assert abs((rec['ga'] * rec['A']).sum()) < 1e-14 and abs((rec['gu'] * rec['U']).sum()) < 1e-14
            assert not rec['ga'][~rec['A']].any() and not rec['gu'][~rec['U']].any()
            assert rec['U'].sum() == rec['npos'] + min(k, P - rec['npos'])
        rng = np.random.RandomState(3)
        for _ in range(12):                                     # central differences; the selection does not move (gap >> h)
            i, j = int(rng.choice(list(ref['r']))), rng.randint(P)
            h = 1e-6
            zp, zm = z64.copy(), z64.copy()
            zp[i, j] += h
            zm[i, j] -= h
            lp = R.proxy_ce(zp.reshape(-1), P, d['labels'], d['cams'], d['pcl'], d['pcm'], n, P, k, *w)
            lm = R.proxy_ce(zm.reshape(-1), P, d['labels'], d['cams'], d['pcl'], d['pcm'], n, P, k, *w)
            assert np.array_equal(lp['negsel'], ref['negsel']) and np.array_equal(lm['negsel'], ref['negsel'])
            assert abs((lp['loss'] - lm['loss']) / (2 * h) - ref['dz'][i, j]) < 1e-7, (w, i, j)


def test_invalid_rows_ties_and_the_selection_order():
    d = R.in_ties()
    ref = R.proxy_ce(d['logits'], d['ld'], d['labels'], d['cams'], d['pcl'], d['pcm'], 2, R.TIE_P, R.TIE_K, 1.0, 0.5)
    assert ref['negsel'].tolist() == [d['want'], d['want']] and ref['own'].tolist() == [0, 0]
    z = d['logits'].reshape(2, -1)
    assert np.signbit(z[1, 40]) and not np.signbit(z[1, 41]) and z[1, 40] == z[1, 41]      # -0.0 against +0.0
    assert ref['r'][0]['gap'] == 0.0                                                        # the cut runs through the copies
    # k_neg = 0: no negatives, U = Pos; a camera whose only proxy is the row's own: lse_A of one term, intra = 0
    d = R.in_ce(9, 70, 6, 'mixed')
    ref = R.proxy_ce(d['logits'], d['ld'], d['labels'], d['cams'], d['pcl'], d['pcm'], 9, 70, 0, 1.0, 0.5)
    assert ref['negsel'].shape == (9, 0) and all(rec['U'].sum() == rec['npos'] for rec in ref['r'].values())
    assert ref['own'][1] == -1 and ref['own'][3] == -1 and d['labels'][3] >= 0              # noise; a pair without a proxy
    assert ref['r'][2]['A'].sum() == 1 and ref['r'][2]['intra'] == 0.0
    assert ref['r'][4]['npos'] == 1 and ref['r'][4]['inter'] == 0.0                         # the one-camera cluster, no negatives
    assert not ref['dz'][1].any() and not ref['dz'][3].any() and ref['nv'] == 7


def test_sweep_reaches_every_pattern():
    seen = set()
    for n, P in R.CE_CASES:
        for C in R.CE_CAMS:
            for pattern in R.CE_TABLES:
                d = R.in_ce(n, P, C, pattern)
                assert d['pcl'].shape == d['pcm'].shape == (P,) and d['pcm'].max() < C and d['pcm'].min() >= 0
                for k in R.CE_K:
                    ref = R.proxy_ce(d['logits'], d['ld'], d['labels'], d['cams'], d['pcl'], d['pcm'], n, P, min(k, P), 1.0, 0.5)
                    if (d['labels'] == -1).any():
                        seen.add('noise')
                    if ((d['labels'] >= 0) & (ref['own'] < 0)).any():
                        seen.add('no proxy')
                    for rec in ref['r'].values():
                        nN = P - rec['npos']
                        seen.add('no negatives' if nN == 0 else 'k > |N|' if k > nN else 'k == |N|' if k == nN else 'cut')
                        if rec['A'].sum() == 1:
                            seen.add('lone camera')
                        if rec['npos'] == 1 and C > 1:
                            seen.add('one-camera cluster')
                        if rec['npos'] > 1:
                            seen.add('several positives')
    assert seen == {'noise', 'no proxy', 'no negatives', 'k > |N|', 'k == |N|', 'cut', 'lone camera',
                    'one-camera cluster', 'several positives'}, seen
    assert max(R.CE_P) > 1024 and 257 in R.CE_P and R.trips(1025, 256) == 5


def test_selection_gap_condition_holds_for_every_loss_case():
    worst, fixed = np.inf, []
    for P, k, mode in R.LOSS_CASES:
        for tag in ('loss', 'second'):
            seed = R.loss_seed(P, k, tag)
            ref = R.loss(R.in_loss(P, k, seed, tag), P, k, R.LOSS_W)
            for gap, bound in R.gaps(ref, R.LOSS_D):
                assert gap > R.GAP_FACTOR * bound, (P, k, tag, gap, bound)
                worst = min(worst, gap / bound)
            assert R.gap_ok(ref, R.LOSS_D)
            fixed.append((P, k, tag, seed))
    print('\nselection gap / bound of one logit: smallest %.1f; seeds %r' % (worst, fixed))
    # a fixed seed is not enough: at P = 257, k = 50 the first seeds hold rows whose cut is closer than the bound allows
    ratios = []
    for seed in range(4):
        r = R.rng_for('proxy', 'loss', 257, R.LOSS_CAMS, seed)
        pcl, pcm = R.table(257, R.LOSS_CAMS, 'spread', None)
        j = r.randint(0, 257, R.LOSS_N)
        d = dict(mem=R.unit_rows(r.standard_normal((257, R.LOSS_D))), x=R.unit_rows(r.standard_normal((R.LOSS_N, R.LOSS_D))),
                 labels=pcl[j].astype(np.int64), cams=pcm[j].astype(np.int64), pcl=pcl, pcm=pcm)
        ratios.append(min(g / b for g, b in R.gaps(R.loss(d, 257, 50, R.LOSS_W), R.LOSS_D)))
    print('P = 257, k = 50, seeds 0 .. 3: smallest gap / bound %s' % ', '.join('%.2f' % v for v in ratios))


# ----------------------------------------------------------------------------------------------------------------------
# ProxyLabels
HOST = np.array([5, 5, -1, 9, 2, 9, 5, -1, 2, 2, 9, 5], np.int64)          # ids 2, 5, 9 -> clusters 0, 1, 2
CAMS = np.array([3, 0, 1, 0, 0, 0, 3, 2, 7, 0, 7, 0], np.int64)


def test_proxy_labels_numbering_and_noise():
    from grl_amd.reid.train.pseudo import PseudoLabels, ProxyLabels
    pl = PseudoLabels(HOST)
    px = pl.proxies(CAMS)
    assert isinstance(px, ProxyLabels)
    pc, pm, sp = R.proxy_numbering(pl.host, CAMS)
    assert px.n_proxies == 6 == pc.size
    assert px.proxy_cluster.tolist() == pc.tolist() == [0, 0, 1, 1, 2, 2]
    assert px.proxy_cam.tolist() == pm.tolist() == [0, 7, 0, 3, 0, 7]                       # ascending (cluster, cam)
    assert px.sample_proxy.tolist() == sp.tolist() == [3, 2, -1, 4, 0, 4, 3, -1, 1, 0, 5, 2]
    assert px.proxy_cluster.dtype == px.proxy_cam.dtype == np.int32 and px.sample_proxy.dtype == np.int64
    assert px.proxy_cluster_dev.dtype == px.proxy_cam_dev.dtype == torch.int32 and px.sample_proxy_dev.dtype == torch.int64
    assert px.proxy_cluster_dev.tolist() == pc.tolist() and px.sample_proxy_dev.tolist() == sp.tolist()
    assert pl.proxies(CAMS.tolist()).sample_proxy.tolist() == sp.tolist() and pl.proxies(torch.from_numpy(CAMS)).n_proxies == 6
    assert PseudoLabels(np.array([-1, -1])).proxies([0, 1]).n_proxies == 0                  # noise alone: no proxy
    for bad, pattern in ((CAMS[:5], 'cams must be 12 integers'), (CAMS.astype(np.float64), 'cams must be 12 integers'),
                         (np.where(CAMS == 7, -1, CAMS), 'a camera id is negative'), (CAMS + 2 ** 31, 'a camera id does not fit int32')):
        with pytest.raises(ValueError, match='PseudoLabels.proxies: ' + pattern):
            pl.proxies(bad)


def test_refusals_fire_before_any_device_call(monkeypatch):
    from grl_amd import engine
    from grl_amd.reid.loss import ProxyMemoryLoss, ClusterMemoryLoss, memory
    from grl_amd.reid.train import pseudo, SEQTrainer, CameraSEQTrainer

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    for name in ('_call', 'gemm', 'cluster_centroids', 'cluster_jaccard'):
        monkeypatch.setattr(engine, name, no_device)
    monkeypatch.setattr(memory, '_call', no_device)
    with pytest.raises(ValueError, match="mode must be 'hard', 'mean' or 'instance' .got 'soft'"):
        ProxyMemoryLoss(16, mode='soft')
    with pytest.raises(ValueError, match='temp must be > 0'):
        ProxyMemoryLoss(16, temp=0.0)
    with pytest.raises(ValueError, match='k_neg must be an integer >= 0'):
        ProxyMemoryLoss(16, k_neg=-1)
    crit = ProxyMemoryLoss(16)
    assert (crit.temp, crit.momentum, crit.mode, crit.k_neg, crit.w_intra, crit.w_inter, crit.inter_on) == \
        (0.07, 0.2, 'instance', 50, 1.0, 0.5, True)
    assert {'centroids', 'proxy_cluster', 'proxy_cam'} <= set(crit.state_dict())
    i32, f = torch.zeros(3, dtype=torch.int32), torch.zeros((3, 16))
    for args, pattern in (((f.double(), i32, i32), 'centroids must be a float32 tensor .got torch.float64'),
                          ((np.zeros((3, 16), np.float32), i32, i32), 'centroids must be a float32 tensor .got ndarray'),
                          ((torch.zeros((3, 20)), i32, i32), r'centroids must be \[P >= 1, num_features = 16\] .got \(3, 20\)'),
                          ((torch.zeros((0, 16)), i32[:0], i32[:0]), r'centroids must be \[P >= 1, num_features = 16\]'),
                          ((f, i32, i32), 'centroids must be on a HIP device .got cpu')):
        with pytest.raises(ValueError, match='ProxyMemoryLoss.reset: ' + pattern):
            crit.reset(*args)
    assert crit.num_proxies == 1                                                            # a refused reset changes nothing
    for args, pattern in (((f, i32.long(), i32), 'proxy_cluster must be an int32 tensor .got torch.int64'),
                          ((f, i32, [0, 0, 0]), 'proxy_cam must be an int32 tensor .got list'),
                          ((f, i32, i32[:2]), r'proxy_cam must hold one entry per proxy, \[3\] .got \(2,\)')):
        with pytest.raises(ValueError, match='ProxyMemoryLoss.reset: ' + pattern):
            crit.reset(*args)
    # train_unsupervised(cameras=True): the wrong trainer, the wrong criterion -- before the evaluator is asked for anything

    class Ev(object):
        def extract_feature(self, loader):
            raise AssertionError('features were extracted')

    def trainer(cls, a, b):
        t = cls.__new__(cls)
        t.criterion_corr, t.criterion_uncorr = a, b
        return t
    tracklets = [((i,), i, i % 2) for i in range(4)]
    run = lambda t: pseudo.train_unsupervised(t, Ev(), None, tracklets, None, None, 1, cameras=True)     # noqa: E731
    with pytest.raises(ValueError, match='cameras=True needs a CameraSEQTrainer .got SEQTrainer'):
        run(trainer(SEQTrainer, crit, crit))
    with pytest.raises(ValueError, match='cameras=True needs criterion_corr to be a ProxyMemoryLoss .got ClusterMemoryLoss'):
        run(trainer(CameraSEQTrainer, ClusterMemoryLoss(16, 4), crit))
    with pytest.raises(ValueError, match='cameras=True needs criterion_uncorr to be a ProxyMemoryLoss .got ClusterMemoryLoss'):
        run(trainer(CameraSEQTrainer, crit, ClusterMemoryLoss(16, 4)))


# ----------------------------------------------------------------------------------------------------------------------
# the camera's way to the criterion
class _Crit(object):
    def __init__(self, name, log):
        self.name, self.log = name, log

    def __call__(self, feats, targets, cams=None):
        self.log.append((self.name, tuple(feats.shape), targets.tolist(), None if cams is None else cams.tolist()))
        return feats.sum() * 0.0, torch.zeros((feats.size(0), 4))


def _stub_trainer(cls, log, monkeypatch):
    from grl_amd.reid.train import trainer as T
    t = cls.__new__(cls)
    t.device = torch.device('cpu')
    t.model = lambda imgs: (torch.ones((imgs.size(0), imgs.size(1), 8)), torch.ones((imgs.size(0), imgs.size(1), 8)))
    head = lambda x: (torch.zeros((x.size(0) // 2, x.size(0) // 2, 2)), x.mean(1))          # noqa: E731
    t.siamese_model = t.siamese_model_uncorr = head
    t.criterion_corr, t.criterion_uncorr = _Crit('corr', log), _Crit('uncorr', log)
    t.criterion_ver = lambda prob, tp, tg: (torch.zeros(()), None)
    monkeypatch.setattr(T, 'criterion_triplet', lambda f, y: torch.zeros(f.size(0)))
    monkeypatch.setattr(T.SEQTrainer, '_pair_prob', staticmethod(lambda s: s[..., 1]))
    monkeypatch.setattr(T.SEQTrainer, '_top1', staticmethod(lambda o, y: torch.zeros(())))
    return t


BATCH = (torch.zeros((4, 3, 1)), torch.tensor([7, 7, 9, 9]), torch.tensor([0, 5, 2, 3]))      # B = 4 (two pairs), T = 3


def test_seqtrainer_calls_its_three_identity_criteria_through_id_loss(monkeypatch):
    from grl_amd.reid.train import SEQTrainer
    log, hook = [], []
    t = _stub_trainer(SEQTrainer, log, monkeypatch)
    base = SEQTrainer._id_loss
    monkeypatch.setattr(SEQTrainer, '_id_loss', lambda self, c, f, y, rows: hook.append((c.name, rows)) or base(self, c, f, y, rows))
    inputs, targets = t._parse_data(BATCH)
    t._forward(inputs, targets, 0, 0)
    assert sorted(hook) == [('corr', 'clip'), ('corr', 'frame'), ('uncorr', 'clip')]
    assert [h[1] for h in hook if h[0] == 'corr'] == ['frame', 'clip']                       # the frame-level call comes first
    assert all(entry[3] is None for entry in log) and len(log) == 3                          # the base hands over no camera
    by = {(e[0], e[1][0]): e for e in log}
    assert by[('corr', 12)][2] == [7, 7, 7, 7, 7, 7, 9, 9, 9, 9, 9, 9] and by[('corr', 4)][2] == [7, 9, 7, 9]


def test_camera_seqtrainer_hands_over_the_cameras_in_the_targets_row_order(monkeypatch):
    from grl_amd.reid.train import CameraSEQTrainer
    log = []
    t = _stub_trainer(CameraSEQTrainer, log, monkeypatch)
    inputs, targets = t._parse_data(BATCH)
    assert targets.tolist() == [7, 7, 9, 9]
    t._forward(inputs, targets, 0, 0)
    by = {(e[0], e[1][0]): e for e in log}
    assert by[('corr', 12)][3] == [0, 0, 0, 5, 5, 5, 2, 2, 2, 3, 3, 3]                       # expanded over T, as targetX
    assert by[('corr', 4)][3] == by[('uncorr', 4)][3] == [0, 2, 5, 3]                        # probe-then-gallery, as target
    assert by[('corr', 4)][2] == [7, 9, 7, 9]


# ----------------------------------------------------------------------------------------------------------------------
# the C ABI
def test_header_binding_and_library_carry_the_entry_point():
    from grl_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'grl_hip.h')).read()
    assert re.search(r'int\s+grl_proxy_ce\(const float\* logits, int64_t ld, const int64_t\* labels, const int64_t\* cams,\s+'
                     r'const int32_t\* proxy_cluster, const int32_t\* proxy_cam, int n, int P, int k_neg, float w_intra,\s+'
                     r'float w_inter, float\* loss, float\* correct, float\* dlogits, int64_t ldd, int64_t\* own,\s+'
                     r'int32_t\* negsel, float\* ws, void\* stream\);', src)
    assert int(re.search(r'#define\s+GRL_PROXY_MAX_P\s+(\d+)', src).group(1)) == 8192 == R.MAX_P
    assert int(re.search(r'#define\s+GRL_ABI_VERSION\s+(\d+)', src).group(1)) == 10 == _lib.ABI_VERSION
    assert 'grl_proxy_ce' in _lib.exported_symbols()
    assert 'proxy.hip' in open(os.path.join(ROOT, 'grl_amd', 'csrc', 'Makefile')).read()


def test_host_argument_checks_return_einval_through_the_c_abi():
    import ctypes as C
    from grl_amd import _lib
    lib = _lib.load()
    # fake device pointers (never dereferenced: every call below is refused before the launch)

    def ce(logits=0x1000, ld=8, labels=0x2000, cams=0x3000, pcl=0x4000, pcm=0x5000, n=2, P=8, k=3, loss=0x6000, dz=0x7000,
           ldd=8, ws=0x8000):
        return lib.grl_proxy_ce(logits, ld, labels, cams, pcl, pcm, n, P, k, C.c_float(1.0), C.c_float(0.5), loss, None, dz, ldd,
                                None, None, ws, None)
    for kw in (dict(logits=None), dict(labels=None), dict(cams=None), dict(pcl=None), dict(pcm=None), dict(loss=None),
               dict(ws=None), dict(n=0), dict(n=-1), dict(P=0), dict(k=-1), dict(k=9), dict(ld=7), dict(ldd=7),
               dict(P=R.MAX_P + 1, ld=R.MAX_P + 1, ldd=R.MAX_P + 1)):
        assert ce(**kw) == _lib.GRL_EINVAL, kw
        assert b'proxy_ce' in lib.grl_last_error()
