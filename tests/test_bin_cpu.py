"""The binary-code contract of DESIGN.md 4ag on the host: the numpy model tests/bin_ref.py against numpy.packbits, a
word-wise population count and float64, the float64 ITQ model's properties on the training recipe, the GRL_EVAL_BIN parser
and refusals, the binding and the host-side checks.  No device."""
import os

import numpy as np
import pytest
import torch

import bin_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('grl_bin_scan', 'grl_bin_pack', 'grl_bin_words', 'grl_bin_lut')
NBITS = (32, 64, 96, 256, 1024)


# ----------------------------------------------------------------------------
# layouts and distances
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('nbits', NBITS)
def test_pack_is_packbits_little_and_the_scan_layout_is_its_little_endian_words(nbits):
    g = np.random.Generator(np.random.PCG64(nbits))
    for n in (1, 5, 65):
        bits = g.random((n, nbits)) < 0.5
        codes = B.pack(bits)
        assert codes.dtype == np.uint8 and codes.shape == (n, nbits // 8)
        assert np.array_equal(codes, np.packbits(bits, axis=1, bitorder='little'))
        for i, b in ((0, 0), (n - 1, nbits - 1), (n // 2, 9 % nbits)):
            assert bool((codes[i, b // 8] >> (b % 8)) & 1) == bool(bits[i, b])
        assert np.array_equal(B.unpack(codes), bits)
        w = B.words(codes)
        assert w.dtype == np.uint32 and w.shape == (nbits // 32, n)
        for i, b in ((0, 0), (n - 1, nbits - 1), (n // 2, 41 % nbits)):
            assert bool((int(w[b // 32, i]) >> (b % 32)) & 1) == bool(bits[i, b])
        assert np.array_equal(B.unwords(w), codes)


def test_the_bit_rule_sends_nan_and_both_zeros_to_zero():
    z = np.array([[np.nan, -0.0, 0.0, np.inf, -np.inf, 1e-45, -1e-45, 3.0] * 4], dtype=np.float32)
    assert B.bits_of(z)[0, :8].tolist() == [False, False, False, True, False, True, False, True]
    assert B.pack(B.bits_of(z))[0].tolist() == [0b10101000] * 4


@pytest.mark.parametrize('nbits', NBITS)
def test_hamming_by_unpacked_bits_equals_the_word_wise_popcount(nbits):
    g = np.random.Generator(np.random.PCG64(7 + nbits))
    gc = B.pack(g.random((67, nbits)) < 0.5)
    gc[1::2] = gc[0:-1:2][:gc[1::2].shape[0]]                       # duplicate rows: distance 0 between them
    qc = np.concatenate([B.pack(g.random((4, nbits)) < 0.3), gc[:3], np.zeros((1, nbits // 8), np.uint8),
                         np.full((1, nbits // 8), 255, np.uint8)])
    d = B.hamming(qc, gc)
    assert d.dtype == np.float32 and np.array_equal(d, B.hamming_words(qc, gc))
    assert d[4, 0] == 0 and d[4, 1] == 0 and d.min() >= 0 and d.max() <= nbits
    assert np.array_equal(d[-2] + d[-1], np.full(67, nbits, np.float32))          # all-zero and all-one queries
    assert np.array_equal(B.popcount32(np.array([0, 1, 0xffffffff, 0x80000001, 0x0f0f0f0f], np.uint32)), [0, 1, 32, 2, 16])


def test_the_float32_tables_follow_float64_and_give_the_asymmetric_distance():
    g = np.random.Generator(np.random.PCG64(3))
    z = (g.standard_normal((5, 64)) * 3).astype(np.float32)
    t32, t64 = B.lut(z), B.lut64(z)
    assert t32.dtype == np.float32 and t32.shape == (5, 8, 256)
    # 8 sequential adds: at most 7 roundings of partial sums bounded by sum |z_j|
    bound = 7 * 2.0 ** -24 * np.abs(z.astype(np.float64)).reshape(5, 8, 8).sum(2)[:, :, None]
    assert (np.abs(t32 - t64) <= bound).all()
    assert np.array_equal(t32[:, :, 0], -t32[:, :, 255])             # exact negations
    gbits = g.random((33, 64)) < 0.5
    codes = B.pack(gbits)
    picked = t64[:, np.arange(8)[None, :], codes.astype(np.int64)]   # [5, 33, 8]
    assert np.allclose(picked.sum(2), B.asym64(z, gbits), rtol=0, atol=1e-9)
    # a NaN column poisons exactly the entries of its byte; -0 + +0 stays +0
    z[0, 9] = np.nan
    t = B.lut(z)
    assert np.isnan(t[0, 1]).all() and not np.isnan(t[0, 0]).any() and not np.isnan(t[1:]).any()
    assert np.array_equal(B.lut(np.zeros((1, 32), np.float32)).view(np.uint32), np.zeros((1, 4, 256), np.uint32))


# ----------------------------------------------------------------------------
# the float64 ITQ model on the training recipe
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('seed', (0, 1, 2))
def test_itq_model_objective_orthogonality_and_mirror_codes(seed):
    r = B.RECIPE
    gal, qry = B.recipe(seed)
    assert gal.shape == (r['n'], r['d']) and qry.shape == (r['nq'], r['d'])
    proj, shift, obj = B.itq(gal, r['nbits'], r['n_iter'], seed)
    assert len(obj) == r['n_iter']
    assert all(b >= a * (1 - 1e-12) for a, b in zip(obj, obj[1:])) and obj[-1] > obj[0]
    assert np.abs(proj @ proj.T - np.eye(r['nbits'])).max() <= 1e-10
    x = gal.astype(np.float64)
    mean = x.mean(0)
    z = x @ proj.T + shift
    zm = (2 * mean - x) @ proj.T + shift
    assert np.abs(z + zm).max() <= 1e-10                            # the mirror image's projection is -z
    far = np.abs(z) > 1e-9
    assert far.mean() > 0.99 and (B.bits_of(z)[far] != B.bits_of(zm)[far]).all()
    # the orderings the GPU test asserts, in the model
    exact = B.exact_lists(qry, gal, 10)
    lp, ls = B.lsh(gal, r['nbits'], seed)

    def recalls(p, s):
        zq, zg = qry.astype(np.float64) @ p.T + s, x @ p.T + s
        gb = B.bits_of(zg)
        ham = B.hamming(B.pack(B.bits_of(zq)), B.pack(gb))
        return B.recall_at(B.ranked(ham, 10), exact, 10), B.recall_at(B.ranked(B.asym64(zq, gb), 10), exact, 10)
    itq_h, itq_a = recalls(proj, shift)
    lsh_h, _ = recalls(lp.astype(np.float64), ls)
    assert itq_h > lsh_h and itq_a >= itq_h


# ----------------------------------------------------------------------------
# the knob, the binding, the host-side checks
# ----------------------------------------------------------------------------
def test_the_evaluator_knob_parses():
    from grl_amd.reid.evaluator.attevaluator import parse_bin_knob as parse
    name = 'GRL_EVAL_BIN'
    assert parse(name, None) is None and parse(name, '') is None and parse(name, '  ') is None
    good, bad = B.parse_knob_cases()
    for text, want in good.items():
        assert parse(name, text) == want, text
    for text in bad:
        with pytest.raises(ValueError, match=name) as err:
            parse(name, text)
        assert repr(text) in str(err.value)


class _Never(object):
    def __getattr__(self, name):
        raise AssertionError('touched %s' % name)


KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC', 'GRL_EVAL_ROC',
         'GRL_EVAL_CLUSTER', 'GRL_EVAL_CLUSTER_JACCARD', 'GRL_EVAL_KMEANS', 'GRL_EVAL_HDBSCAN', 'GRL_EVAL_TSNE',
         'GRL_EVAL_SILHOUETTE', 'GRL_EVAL_PCA', 'GRL_EVAL_DIFFUSION', 'GRL_EVAL_SET', 'GRL_EVAL_PQ', 'GRL_EVAL_IVF',
         'GRL_EVAL_REFINE', 'GRL_EVAL_NNG', 'GRL_EVAL_BIN')


def test_the_knob_is_refused_with_what_the_pq_knob_is_refused_with(monkeypatch):
    from grl_amd.reid.evaluator import ATTEvaluator
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)

    def run(only_eval=True, rerank=0):
        ATTEvaluator(_Never(), _Never(), only_eval).evaluate(None, None, _Never(), _Never(), '', 0, rerank)
    monkeypatch.setenv('GRL_EVAL_BIN', '48,itq')
    with pytest.raises(ValueError, match="GRL_EVAL_BIN.*'48,itq'"):
        run()
    monkeypatch.setenv('GRL_EVAL_BIN', '64,lsh')
    with pytest.raises(ValueError, match='GRL_EVAL_BIN=64,lsh cannot re-rank'):
        run(rerank=1)
    for other, value in (('GRL_EVAL_SET', 'min'), ('GRL_EVAL_DIFFUSION', '10'), ('GRL_EVAL_METRIC', 'verify')):
        monkeypatch.setenv(other, value)
        with pytest.raises(ValueError, match='GRL_EVAL_BIN=64,lsh cannot be combined with %s' % other):
            run()
        monkeypatch.delenv(other)
    for only_eval in (True, False):                               # accepted: it gets as far as the models and loaders
        with pytest.raises(AssertionError, match='touched'):
            run(only_eval=only_eval)


def test_library_exports_and_header_declare_the_entry_points():
    import ctypes
    from grl_amd import _lib, engine
    header = open(os.path.join(ROOT, 'include', 'grl_hip.h')).read()
    assert sorted(n for n in _lib._SIGNATURES if n.startswith('grl_bin_')) == sorted(NAMES)
    for name in NAMES:
        assert '%s(' % name in header, name
    srcs = open(os.path.join(ROOT, 'grl_amd', 'csrc', 'Makefile')).read().split('SRCS =')[1].split('\n')[0]
    assert ' bin.hip ' in srcs
    assert _lib.ABI_VERSION == 10 and int(header.split('#define GRL_ABI_VERSION')[1].split()[0]) == 10     # additive only
    for word, value in (('GRL_BIN_NBITS_MAX', B.NBITS_MAX), ('GRL_BIN_SLAB', B.SLAB), ('GRL_BIN_NQ_MAX', B.NQ_MAX)):
        assert int(header.split('#define %s' % word)[1].split()[0]) == value
    assert (engine.BIN_NBITS_MAX, engine.BIN_SLAB, engine.BIN_NQ_MAX) == (B.NBITS_MAX, B.SLAB, B.NQ_MAX)
    para = header.split('binary hash codes')[1].split('#define GRL_BIN_NBITS_MAX')[0]
    for phrase in ('PUBLIC LAYOUT', 'SCAN LAYOUT', "bitorder='little'", 'z[i][b] > 0', 'NaN, -0 and +0 give 0', 'little endian',
                   'grl_pq_pack', 'ksub = 256', 'popcount', 'GRL_PQ_COSINE', 'sequential fp32 sum from +0.0f', 'GRL_EINVAL'):
        assert phrase in para, phrase
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.exported_symbols() and getattr(lib, name).restype is not None and hasattr(raw, name), name


def test_host_argument_checks_return_einval_through_the_c_abi():
    from grl_amd import _lib
    lib = _lib.load()
    E = _lib.GRL_EINVAL
    # fake device pointers (never dereferenced: every call below is refused, or has nothing to launch)

    def scan(q=0x1000, words=0x2000, ldw=0, out=0x3000, ldo=0, nq=0, n=0, nbits=64):
        return lib.grl_bin_scan(q, words, ldw, out, ldo, nq, n, nbits, None)
    assert scan() == 0 and scan(nq=5, n=0) == 0 and scan(nq=0, n=7, ldw=7, ldo=9, nbits=1024) == 0
    for kw in (dict(q=None), dict(words=None), dict(out=None), dict(nq=-1), dict(n=-1), dict(nbits=0), dict(nbits=48),
               dict(nbits=-32), dict(nbits=1056), dict(n=7, ldw=6, ldo=7), dict(n=7, ldw=7, ldo=6), dict(q=0x1002),
               dict(words=0x2001), dict(out=0x3002), dict(nq=B.NQ_MAX + 1)):
        assert scan(**kw) == E, kw
    assert b'bin_scan' in lib.grl_last_error()

    def pack(z=0x1000, ldz=64, codes=0x2000, words=0x3000, ldw=0, signs=None, lds=0, n=0, nbits=64):
        return lib.grl_bin_pack(z, ldz, codes, words, ldw, signs, lds, n, nbits, None)
    assert pack() == 0 and pack(codes=None, words=None, signs=0x4000, lds=64) == 0 and pack(ldz=100) == 0
    for kw in (dict(z=None), dict(codes=None, words=None), dict(n=-1), dict(nbits=40), dict(nbits=2048), dict(ldz=63),
               dict(n=3, ldw=2), dict(signs=0x4000, lds=60), dict(z=0x1001), dict(codes=0x2002), dict(words=0x3001),
               dict(signs=0x4002, lds=64)):
        assert pack(**kw) == E, kw
    assert b'bin_pack' in lib.grl_last_error()

    def words(codes=0x1000, out=0x2000, ldw=0, n=0, nbits=32):
        return lib.grl_bin_words(codes, out, ldw, n, nbits, None)
    assert words() == 0
    for kw in (dict(codes=None), dict(out=None), dict(n=-1), dict(nbits=16), dict(n=4, ldw=3), dict(codes=0x1001),
               dict(out=0x2002)):
        assert words(**kw) == E, kw
    assert b'bin_words' in lib.grl_last_error()

    def lut(z=0x1000, ldz=32, out=0x2000, nq=0, nbits=32):
        return lib.grl_bin_lut(z, ldz, out, nq, nbits, None)
    assert lut() == 0
    for kw in (dict(z=None), dict(out=None), dict(nq=-1), dict(nbits=8), dict(ldz=31), dict(z=0x1002), dict(out=0x2001)):
        assert lut(**kw) == E, kw
    assert b'bin_lut' in lib.grl_last_error()


def test_the_public_functions_validate_before_the_device(monkeypatch):
    from grl_amd import engine

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    monkeypatch.setattr(engine, '_call', no_device)
    monkeypatch.setattr(engine, 'gemm', no_device)
    host = torch.zeros((40, 64))
    for bad in (host, host.to(torch.float64), host.view(-1), [[1.0]]):
        with pytest.raises(ValueError, match='bin_train: xf must be a 2-d float32 tensor on a HIP device'):
            engine.bin_train(bad, 32)
    with pytest.raises(ValueError, match='BinaryCodebook: proj must be a 2-d float32 tensor on a HIP device'):
        engine.BinaryCodebook(host)
    # a stand-in for device rows: the argument checks that follow need no device
    monkeypatch.setattr(engine, '_pca_matrix', lambda t, what, name: t)
    with pytest.raises(ValueError, match="bin_train: method must be 'itq' or 'lsh'"):
        engine.bin_train(host, 32, 'pca')
    for nbits in (0, 16, 48, 1056, 32.0, True, '32'):
        with pytest.raises(ValueError, match='bin_train: nbits must be an integer multiple of 32 in 32..1024'):
            engine.bin_train(host, nbits)
    for n_iter in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match='bin_train: n_iter must be an integer >= 1'):
            engine.bin_train(host, 32, 'lsh', n_iter)
    for seed in (-1, 0.5):
        with pytest.raises(ValueError, match='bin_train: seed must be an integer >= 0'):
            engine.bin_train(host, 32, 'lsh', 5, seed)
    with pytest.raises(ValueError, match='BinaryCodebook: nbits must be an integer multiple of 32'):
        engine.BinaryCodebook(torch.zeros((40, 64)))
    with pytest.raises(ValueError, match="metric must be 'cosine' or 'euclidean'"):
        engine.BinaryCodebook(torch.zeros((32, 64)), None, 'l1')
    with pytest.raises(ValueError, match=r'shift must be None or a float32 device tensor \[nbits\] = \[32\]'):
        engine.BinaryCodebook(torch.zeros((32, 64)), torch.zeros(32))
    book = engine.BinaryCodebook(torch.zeros((32, 64)))
    assert (book.nbits, book.d, book.metric, book.shift, book.objective) == (32, 64, 'cosine', None, None)
    for fn in (book.project, book.encode, book.lut):
        with pytest.raises(ValueError, match=r'must be \[rows, d\] = \[rows, 64\]'):
            fn(torch.zeros((3, 32)))
    with pytest.raises(ValueError, match='BinaryIndex: codebook must be a BinaryCodebook'):
        engine.BinaryIndex(host, host)
    with pytest.raises(ValueError, match='bin_index: codebook must be a BinaryCodebook'):
        engine.bin_index(host, host)
    for wrong in (torch.zeros((5, 4), dtype=torch.uint8), torch.zeros((5, 4)), 7):
        with pytest.raises(ValueError, match=r'BinaryIndex: codes must be a uint8 device tensor \[n, nbits / 8\] = \[n, 4\]'):
            engine.BinaryIndex(book, wrong)
    index = engine.BinaryIndex.__new__(engine.BinaryIndex)
    index.codebook, index.nbits, index.n = book, 32, 40
    for fn, args in ((engine.bin_dist, (host, host)), (engine.bin_search, (host, host, 3)),
                     (engine.bin_metrics_streaming, (host, host, 0, 0, 0, 0)), (engine.bin_refine_search, (host, host, host, 1, 2))):
        with pytest.raises(ValueError, match='index must be a BinaryIndex'):
            fn(*args)
    for fn, args in ((engine.bin_dist, (host, index)), (engine.bin_search, (host, index, 3)),
                     (engine.bin_metrics_streaming, (host, index, 0, 0, 0, 0)), (engine.bin_refine_search, (host, index, host, 1, 2))):
        with pytest.raises(ValueError, match="mode must be 'hamming' or 'asymmetric'"):
            fn(*args, mode='jaccard')
    for k in (0, 1025, True):
        with pytest.raises(ValueError, match=r'bin_search: k must be in 1\.\.1024'):
            engine.bin_search(host, index, k)
    with pytest.raises(ValueError, match=r'bin_search: qf must be \[rows, d\] = \[rows, 64\]'):
        engine.bin_search(host[:, :32], index, 3)
    many = torch.empty((engine.PQ_NQ_MAX + 1, 64))                 # grl_pq_scan's grid limit has its own message
    with pytest.raises(ValueError, match=r"at most 262140 queries per call in mode 'asymmetric'.*got 262141"):
        engine.bin_metrics_streaming(many, index, 0, 0, 0, 0, mode='asymmetric')
    with pytest.raises(ValueError, match='bin_refine_search: store must be a RefineStore'):
        engine.bin_refine_search(host, index, host, 1, 2)
    store = engine.RefineStore.__new__(engine.RefineStore)
    store.n, store.d, store.dtype, store.data = 41, 64, 'f32', host
    with pytest.raises(ValueError, match=r'store is \[41, 64\], the index \[40, 64\]'):
        engine.bin_refine_search(host, index, store, 1, 2)
    store.n = 40
    with pytest.raises(ValueError, match='bin_refine_search: k must be an integer'):
        engine.bin_refine_search(host, index, store, 0, 2)
    with pytest.raises(ValueError, match=r'bin_refine_search: R \(k <= R <= 1024\)'):
        engine.bin_refine_search(host, index, store, 5, 4)
