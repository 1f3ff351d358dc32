"""IVF-PQ index without a GPU: the float32 model of the contract (tests/ivf_ref.py) against float64, the
nesting of the probes, its reduction to tests/pq_ref.py under an all-zero coarse quantiser, padding / ties / the junk
rule, the GRL_EVAL_IVF knob, the binding, the host-side argument checks of ivf.hip, and the planted case that
tests/test_gpu_ivf.py repeats on the device."""
import os

import numpy as np
import pytest
import torch

import ivf_ref as V
import pq_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
IVF_NAMES = ('grl_ivf_scan', 'grl_ivf_residual', 'grl_ivf_reconstruct', 'grl_ivf_check_labels')
METRICS = ('cosine', 'euclidean')


def _case(M, nlist=5, ksub=16, dsub=32, nq=6, n=90, seed=0, zero_coarse=False):
    g = np.random.Generator(np.random.PCG64(seed + 31 * M))
    d = M * dsub
    coarse = g.standard_normal((nlist, d)).astype(np.float32)
    if zero_coarse:
        coarse[:] = 0
    C = (0.3 * g.standard_normal((M, ksub, dsub))).astype(np.float32)
    x = (coarse[g.integers(0, nlist, n)] + 0.3 * g.standard_normal((n, d))).astype(np.float32)
    q = (coarse[g.integers(0, nlist, nq)] + 0.3 * g.standard_normal((nq, d))).astype(np.float32)
    return q, x, coarse, C


@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('M', (1, 3, 4, 5, 8, 13))
def test_the_model_agrees_with_a_float64_brute_force_on_the_reconstructed_rows(M, metric):
    """The float32 numbers x^ = fl(coarse[lab] + R[code]) are taken as given and -q . x^ / |q - x^| computed in float64.

    Tolerance, with u = 2^-24 and A[q, i] = sum_c |q_c| (|coarse_c| + |R_c|) over the d = M * dsub columns of the pair:
      * x^ differs from coarse + R by one rounding per column: at most u * sum |q_c| |x^_c| <= u A in the dot product;
      * G0 is a float32 dot product of d terms and the M table entries are dot products of dsub terms each: any summation
        order is within (terms) * u * sum |products|, together at most d u A (to first order);
      * the ADC chain adds at most M / 4 + 2 times per partial and the join, and t = g0 + S once more: (M / 4 + 3) u A.
      So |t - (-q . x^)| <= (d + M / 4 + 5) u A =: Et (one more u A for the second-order terms).
    Euclidean: w = rn + (xn + 2 t) against w* = |q|^2 + |x^|^2 - 2 q . x^.  rn and xn are d-term sums of squares (d u
    each, relative), the doubling is exact, two more adds round by u (|rn| + |xn| + 2 |t|) at most:
      Ew = d u (rn + xn) + 2 Et + 2 u (rn + xn + 2 |t|),
    and |sqrt(w) - sqrt(w*)| <= Ew / sqrt(w*), plus the root's own rounding u sqrt(w*) (2 u taken)."""
    q, x, coarse, C = _case(M)
    d = q.shape[1]
    lab, codes, lut, G0, Dc, xn, rn = V.host_case(q, x, coarse, C, metric)
    got = V.dist(lut, codes, lab, G0, metric, xn, rn).astype(np.float64)
    xh = V.reconstruct(coarse, lab, codes, C).astype(np.float64)
    q64 = q.astype(np.float64)
    A = np.abs(q64) @ (np.abs(coarse[lab].astype(np.float64)) + np.abs(R.decode(codes, C).astype(np.float64))).T
    Et = (d + M / 4.0 + 5) * U * A
    dot = -(q64 @ xh.T)
    if metric == 'cosine':
        assert (np.abs(got - dot) <= Et).all()
        return
    rn64, xn64 = (q64 ** 2).sum(1)[:, None], (xh ** 2).sum(1)[None, :]
    w = rn64 + xn64 + 2 * dot
    want = np.sqrt(w)
    assert w.min() > 1.0                                          # (the case keeps clear of the clamp)
    Ew = d * U * (rn64 + xn64) + 2 * Et + 2 * U * (rn64 + xn64 + 2 * np.abs(dot))
    assert (np.abs(got - want) <= Ew / want + 2 * U * want).all()


@pytest.mark.parametrize('metric', METRICS)
def test_probes_are_nested_and_the_candidate_recall_is_monotone(metric):
    q, x, coarse, C = _case(4, nlist=7, n=150, nq=9, seed=3)
    lab, codes, lut, G0, Dc, xn, rn = V.host_case(q, x, coarse, C, metric)
    exact = R.search(R.negdot(q, x) if metric == 'cosine' else R.euclid(q, x), 10)[1]
    share, last = [], None
    for nprobe in range(1, 8):
        probe = V.probes(Dc, nprobe)
        assert probe.shape == (9, nprobe) and (np.sort(probe, 1)[:, 1:] != np.sort(probe, 1)[:, :-1]).all()
        if last is not None:
            assert np.array_equal(probe[:, :-1], last)            # rank j does not depend on nprobe
        last = probe
        cand = V.candidates(lab, probe)
        assert np.array_equal(V.probe_stats(V.lists(lab, 7)[0], probe), cand.sum(1))
        share.append(np.mean([cand[i, exact[i]].mean() for i in range(9)]))
    assert all(b >= a for a, b in zip(share, share[1:])) and share[-1] == 1.0
    assert cand.all()


def test_an_all_zero_coarse_quantiser_reduces_the_model_to_pq_ref():
    q, x, coarse, C = _case(5, nlist=3, zero_coarse=True)
    lab, codes, lut, G0, Dc, xn, rn = V.host_case(q, x, coarse, C, 'cosine')
    assert (lab == 0).all()                                       # every centroid ties: the smaller list
    ptr, ids = V.lists(lab, 3)
    assert ptr.tolist() == [0, 90, 90, 90] and np.array_equal(ids, np.arange(90))
    assert np.array_equal(codes, R.encode(x, C, R.euclid))        # the residual of a zero centroid is the row
    probe = V.probes(Dc, 3)
    assert np.array_equal(probe, np.tile(np.arange(3), (6, 1)))
    D = V.dist(lut, codes, lab, G0, 'cosine')
    want = R.adc_dist(lut, codes, 'cosine')
    assert np.array_equal(D.view(np.uint32), want.view(np.uint32))
    a, b = V.search(D, V.candidates(lab, probe), 20), R.search(want, 20)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def test_lists_residual_and_reconstruct():
    lab = np.array([2, 0, 2, 5, 0, 2])
    ptr, ids = V.lists(lab, 7)
    assert ptr.tolist() == [0, 2, 2, 5, 5, 5, 6, 6] and ids.tolist() == [1, 4, 0, 2, 5, 3] and ids.dtype == np.int32
    with pytest.raises(ValueError):
        V.lists(np.array([0, 7]), 7)
    with pytest.raises(ValueError):
        V.lists(np.array([-1]), 7)
    g = np.random.Generator(np.random.PCG64(5))
    coarse = g.standard_normal((7, 64)).astype(np.float32)
    C = g.standard_normal((2, 16, 32)).astype(np.float32)
    x = g.standard_normal((6, 64)).astype(np.float32)
    r = V.residual(x, coarse, lab)
    assert r.dtype == np.float32 and np.array_equal(r[3], x[3] - coarse[5])
    codes = g.integers(0, 16, (6, 2)).astype(np.uint8)
    xh = V.reconstruct(coarse, lab, codes, C)
    assert np.array_equal(xh[3, 32:], coarse[5, 32:] + C[1, codes[3, 1]])
    # a NaN row: every coarse distance is clamped to 1e-12, list 0; its residual is NaN, code 0 everywhere
    x[4] = np.nan
    lab2 = V.assign(x, coarse)
    assert lab2[4] == 0 and (R.encode(V.residual(x, coarse, lab2), C, R.euclid)[4] == 0).all()


def test_search_pads_breaks_ties_by_the_gallery_index_and_applies_the_junk_rule():
    # two lists; rows 1 and 4 carry the same codes in DIFFERENT lists with equal coarse terms: a tie between lists
    lab = np.array([0, 1, 0, 1, 0, 1])
    codes = np.array([[1], [2], [3], [1], [2], [3]], np.uint8)
    lut = np.zeros((2, 1, 16), np.float32)
    lut[:, 0, :4] = [9.0, 0.5, -1.0, 0.5]
    G0 = np.zeros((2, 2), np.float32)
    D = V.dist(lut, codes, lab, G0)
    assert D[0].tolist() == [0.5, -1.0, 0.5, 0.5, -1.0, 0.5]
    both = V.candidates(lab, np.array([[1, 0], [1, 0]]))
    dist, idx = V.search(D, both, 8)
    assert idx[0].tolist() == [1, 4, 0, 2, 3, 5, -1, -1] and np.isinf(dist[0, 6:]).all() and dist[0, 5] == 0.5
    one = V.candidates(lab, np.array([[1], [0]]))                # query 0 probes list 1 only, query 1 list 0 only
    dist, idx = V.search(D, one, 4)
    assert idx.tolist() == [[1, 3, 5, -1], [4, 0, 2, -1]] and dist[0, 3] == np.inf
    junk = np.zeros((2, 6), bool)
    junk[0, 1] = junk[1, 0] = True
    assert V.search(D, one, 2, junk)[1].tolist() == [[3, 5], [4, 2]]
    # the euclidean form: a NaN argument of the clamp gives 1e-12
    xn, rn = np.ones(6, np.float32), np.array([np.nan, 1.0], np.float32)
    E = V.dist(lut, codes, lab, G0, 'euclidean', xn, rn)
    assert (E[0] == np.sqrt(np.float32(1e-12))).all() and E[1, 1] == np.sqrt(np.float32(1e-12)) and E[1, 0] == np.sqrt(np.float32(3))


def test_the_evaluator_knob_parses():
    from grl_amd.reid.evaluator.attevaluator import parse_ivf_knob as parse
    name = 'GRL_EVAL_IVF'
    assert parse(name, None) is None and parse(name, '') is None and parse(name, '  ') is None
    assert parse(name, '64') == (64, 8) and parse(name, '4') == (4, 1) and parse(name, '1') == (1, 1)
    assert parse(name, ' 64 , 3 ') == (64, 3) and parse(name, '64,64') == (64, 64)
    assert parse(name, '65536') == (65536, 1024) and parse(name, '65536,1024') == (65536, 1024)
    for bad in ('x', '8,', ',4', '8,4,3', '8.5', '8;4', '0', '-1', '65537', '8,0', '8,9', '4096,1025', '8,-1'):
        with pytest.raises(ValueError, match=name) as err:
            parse(name, bad)
        assert repr(bad) in str(err.value)


class _Never(object):
    def __getattr__(self, name):
        raise AssertionError('touched %s' % name)


KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_CLUSTER', 'GRL_EVAL_CLUSTER_JACCARD', 'GRL_EVAL_KMEANS', 'GRL_EVAL_HDBSCAN', 'GRL_EVAL_TSNE',
         'GRL_EVAL_SILHOUETTE', 'GRL_EVAL_PCA', 'GRL_EVAL_DIFFUSION', 'GRL_EVAL_SET', 'GRL_EVAL_PQ', 'GRL_EVAL_IVF')


def test_the_knob_needs_the_pq_knob_and_raises_before_the_loaders_are_touched(monkeypatch):
    from grl_amd.reid.evaluator import ATTEvaluator
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)

    def run(only_eval=True, rerank=0):
        ATTEvaluator(_Never(), _Never(), only_eval).evaluate(None, None, _Never(), _Never(), '', 0, rerank)
    monkeypatch.setenv('GRL_EVAL_IVF', '8,9')
    with pytest.raises(ValueError, match="GRL_EVAL_IVF.*'8,9'"):
        run()
    monkeypatch.setenv('GRL_EVAL_IVF', '8,2')
    with pytest.raises(ValueError, match='GRL_EVAL_IVF=8,2 needs GRL_EVAL_PQ'):
        run()
    monkeypatch.setenv('GRL_EVAL_PQ', '8,4')
    with pytest.raises(ValueError, match='GRL_EVAL_PQ=8,4 cannot re-rank'):          # the PQ knob's refusals are inherited
        run(rerank=1)
    monkeypatch.setenv('GRL_EVAL_DIFFUSION', '50')
    with pytest.raises(ValueError, match='GRL_EVAL_PQ=8,4 cannot be combined with GRL_EVAL_DIFFUSION'):
        run()
    monkeypatch.delenv('GRL_EVAL_DIFFUSION')
    for only_eval in (True, False):                               # accepted: it gets as far as the models and loaders
        with pytest.raises(AssertionError, match='touched'):
            run(only_eval=only_eval)


def test_the_public_functions_validate_before_the_device(monkeypatch):
    from grl_amd import engine
    from grl_amd._lib import GrlHipError

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    monkeypatch.setattr(engine, '_call', no_device)
    monkeypatch.setattr(engine, 'gemm', no_device)
    assert (engine.IVF_NLIST_MAX, engine.IVF_NPROBE_MAX) == (65536, 1024)
    host = torch.zeros(300, 256)
    with pytest.raises(ValueError, match="metric must be 'cosine' or 'euclidean'"):
        engine.IvfPqCodebook(host[:4], None, 'l1')
    with pytest.raises(GrlHipError, match='HIP device'):
        engine.IvfPqCodebook(host[:4], None)
    with pytest.raises(ValueError, match="metric must be 'cosine' or 'euclidean'"):
        engine.ivf_train(host, 4, 8, metric='l1')
    with pytest.raises(GrlHipError, match='HIP device'):
        engine.ivf_train(host, 4, 8)
    for fn in (engine.ivf_index, engine.IvfPqIndex):
        with pytest.raises(ValueError, match='book must be an IvfPqCodebook'):
            fn(host, host, host) if fn is engine.IvfPqIndex else fn(host, host)
    for fn, args in ((engine.ivf_search, (5, 1)), (engine.ivf_dist, (1,)), (engine.ivf_probe_stats, (1,))):
        with pytest.raises(ValueError, match='index must be an IvfPqIndex'):
            fn(host, host, *args)
    book = engine.IvfPqCodebook.__new__(engine.IvfPqCodebook)
    book.nlist, book.d = 4, 256
    index = engine.IvfPqIndex.__new__(engine.IvfPqIndex)
    index.book = book
    for k in (0, 1025, -1):
        with pytest.raises(ValueError, match='k must be in 1..1024'):
            engine.ivf_search(host, index, k, 1)
    for nprobe in (0, 5, -1, 1.0, True):
        for fn, args in ((engine.ivf_search, (5, nprobe)), (engine.ivf_dist, (nprobe,)), (engine.ivf_probe_stats, (nprobe,))):
            with pytest.raises(ValueError, match=r'nprobe must be an integer in 1\.\.4'):
                fn(host, index, *args)
    book.nlist = 5000
    with pytest.raises(ValueError, match=r'nprobe must be an integer in 1\.\.1024'):
        engine.ivf_search(host, index, 5, 1025)
    with pytest.raises(GrlHipError, match='HIP device'):
        engine.ivf_search(host, index, 5, 4)


def test_library_exports_and_header_declare_the_entry_points():
    import ctypes
    from grl_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'grl_hip.h')).read()
    assert sorted(n for n in _lib._SIGNATURES if n.startswith('grl_ivf_')) == sorted(IVF_NAMES)
    for name in IVF_NAMES:
        assert 'int %s(' % name in header, name
    srcs = open(os.path.join(ROOT, 'grl_amd', 'csrc', 'Makefile')).read().split('SRCS =')[1].split('\n')[0]
    assert ' ivf.hip ' in srcs and ' pq.hip ' in srcs
    assert _lib.ABI_VERSION == 10 and int(header.split('#define GRL_ABI_VERSION')[1].split()[0]) == 10     # additive only
    for word, value in (('GRL_IVF_NLIST_MAX', 65536), ('GRL_IVF_NPROBE_MAX', 1024)):
        assert '#define %s' % word in header and int(header.split('#define %s' % word)[1].split()[0]) == value
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert lib.grl_abi_version() == 10
    for name in IVF_NAMES:
        assert name in _lib.exported_symbols() and getattr(lib, name).restype is not None and hasattr(raw, name), name


def test_host_argument_checks_return_einval_through_the_c_abi():
    from grl_amd import _lib
    lib = _lib.load()
    E = _lib.GRL_EINVAL
    # fake device pointers (never dereferenced: every call below is refused, or has nothing to launch)

    def scan(lut=0x1000, codes=0x2000, ids=0x3000, lp=0x4000, probe=0x5000, g0=0x6000, ldp=None, np_=2, off=0x7000,
             xn=None, rn=None, out=0x8000, cidx=0x9000, ldo=None, width=50, nq=3, n=100, nlist=4, M=8, ksub=256, metric=0):
        return lib.grl_ivf_scan(lut, codes, ids, lp, probe, g0, np_ if ldp is None else ldp, np_, off, xn, rn, out, cidx,
                                width if ldo is None else ldo, width, nq, n, nlist, M, ksub, metric, None)
    assert scan(nq=0) == 0 and scan(n=0) == 0 and scan(width=0) == 0          # nothing to do, nothing launched
    for kw in (dict(lut=None), dict(codes=None), dict(ids=None), dict(lp=None), dict(probe=None), dict(g0=None),
               dict(off=None), dict(out=None), dict(cidx=None), dict(nq=-1), dict(n=-1), dict(n=2 ** 31), dict(width=-1),
               dict(nlist=0), dict(nlist=65537), dict(np_=0), dict(np_=5), dict(np_=1025, nlist=4096), dict(M=0),
               dict(M=4097), dict(ksub=8), dict(ksub=100), dict(ksub=512), dict(metric=2), dict(metric=-1), dict(metric=1),
               dict(metric=1, xn=0xa000), dict(metric=1, rn=0xb000), dict(ldp=1), dict(ldo=49), dict(nq=65536),
               dict(lut=0x1002), dict(codes=0x2001), dict(out=0x8002), dict(cidx=0x9002), dict(lp=0x4004),
               dict(ids=0x3002), dict(probe=0x5001), dict(g0=0x6002), dict(off=0x7003),
               dict(metric=1, xn=0xa002, rn=0xb000), dict(metric=1, xn=0xa000, rn=0xb001)):
        assert scan(**kw) == E, kw
    assert b'ivf_scan' in lib.grl_last_error()
    assert scan(metric=1, xn=0xa000, rn=0xb000, nq=0) == 0

    def residual(x=0x1000, ldx=64, labels=0x2000, coarse=0x3000, nlist=4, out=0x4000, ldo=64, rows=10, d=64):
        return lib.grl_ivf_residual(x, ldx, labels, coarse, nlist, out, ldo, rows, d, None)
    assert residual(rows=0) == 0
    for kw in (dict(x=None), dict(labels=None), dict(coarse=None), dict(out=None), dict(rows=-1), dict(d=0), dict(nlist=0),
               dict(nlist=65537), dict(ldx=63), dict(ldo=63)):
        assert residual(**kw) == E, kw

    def reconstruct(coarse=0x1000, cb=0x2000, labels=0x3000, codes=0x4000, out=0x5000, rows=10, nlist=4, M=8, ksub=16,
                    dsub=32, ldo=256):
        return lib.grl_ivf_reconstruct(coarse, cb, labels, codes, out, rows, nlist, M, ksub, dsub, ldo, None)
    assert reconstruct(rows=0) == 0
    for kw in (dict(coarse=None), dict(cb=None), dict(labels=None), dict(codes=None), dict(out=None), dict(rows=-1),
               dict(nlist=0), dict(M=0), dict(M=4097), dict(ksub=3), dict(dsub=0), dict(ldo=255)):
        assert reconstruct(**kw) == E, kw

    def check(labels=0x1000, n=10, nlist=4, flag=0x2000):
        return lib.grl_ivf_check_labels(labels, n, nlist, flag, None)
    assert check(n=0) == 0
    for kw in (dict(labels=None), dict(flag=None), dict(n=-1), dict(nlist=0), dict(nlist=65537)):
        assert check(**kw) == E, kw


# ----------------------------------------------------------------------------
# the planted case, decided here: tests/test_gpu_ivf.py reuses exactly these inputs on the device
# ----------------------------------------------------------------------------
PLANTED_NLIST = 4


def test_planted_identities_under_ivf_adc():
    """pq_ref's planted case (60 queries, 300 rows, 10 identities, d = 256, M = 8, nbits = 4) with nlist = 4.  Measured
    with the numpy model: the lists hold 90 / 60 / 90 / 60 rows (whole identities), the candidate recall of the exact
    top-10 is 1.000 at nprobe = 1, 2, 3 and 4 (a query's ten nearest rows share its identity and so its list), and at
    nprobe = 4 all 60 rank-1 identities equal the exact ones (EXPERIMENTS.md).  The assertions are the structural ones; the
    figures are printed."""
    c = R.PLANTED
    qf, gf, q_pids, g_pids = R.planted_case()
    coarse, lab, C = V.train(gf, PLANTED_NLIST, c['M'], c['nbits'], c['train_seed'], c['max_iter'])
    lab, codes, lut, G0, Dc, xn, rn = V.host_case(qf, gf, coarse, C, 'cosine')
    D = V.dist(lut, codes, lab, G0)
    exact = R.search(R.negdot(qf, gf), 10)[1]
    share = []
    for nprobe in (1, 2, 3, 4):
        cand = V.candidates(lab, V.probes(Dc, nprobe))
        share.append(float(np.mean([cand[i, exact[i]].mean() for i in range(len(qf))])))
    assert all(b >= a for a, b in zip(share, share[1:])) and share[-1] == 1.0
    top = V.search(D, cand, 1)[1][:, 0]
    agree = int((g_pids[top] == g_pids[exact[:, 0]]).sum())
    print('\n[planted IVF case] list lengths %s, candidate recall@10 %s, rank-1 identity agreement at nprobe = 4: %d / %d'
          % (np.diff(V.lists(lab, PLANTED_NLIST)[0]).tolist(), ['%.3f' % s for s in share], agree, len(qf)))
    assert (top >= 0).all()
