"""The shared pieces of the streamed retrieval layer that need no device (engine._block_spans, the width rule of every
``_BlockSource``; engine._int_arg and engine._search_k, the argument checks): literal expectations, written down from the
rule each block source and each validator carried on its own before they were folded into one."""
import re

import numpy as np
import pytest

from grl_amd import engine

# (nq, lo, hi, block_cols, block_bytes) -> (width, spans) of the matrix sources (granule 256)
MATRIX_RULE = [
    ((40, 0, 300, 64, None), (64, [(0, 64), (64, 128), (128, 192), (192, 256), (256, 300)])),
    ((40, 0, 300, None, 1), (256, [(0, 256), (256, 300)])),                  # the floor of 256 columns
    ((3, 0, 1000, None, 8400), (512, [(0, 512), (512, 1000)])),              # 700 fit: rounded down to 512
    ((0, 0, 300, None, 4096), (300, [(0, 300)])),                            # no query counts as one
    ((40, 100, 100, 64, None), (1, [])),                                     # an empty range: width 1, no span
    ((40, 10, 75, 1000, None), (65, [(10, 75)])),
]


@pytest.mark.parametrize('args,want', MATRIX_RULE)
def test_matrix_width_rule(args, want):
    nq, lo, hi, block_cols, block_bytes = args
    assert engine._block_spans(nq, lo, hi, block_cols, block_bytes) == want
    assert engine._block_spans(nq, lo, hi, block_cols, block_bytes, granule=256) == want


class _Probe(engine._BlockSource):
    """a source without a device: nq = 0 (or no span) allocates nothing"""

    def __init__(self, nq, lo, hi, block_cols, block_bytes, granule=256):
        self.nq, self.qf = nq, None
        self._cut(lo, hi, block_cols, block_bytes, granule)


def test_no_queries_or_no_columns_take_no_buffer():
    p = _Probe(0, 0, 300, None, 4096)
    assert (p.width, p.spans, p.buf) == (300, [(0, 300)], None)
    p = _Probe(40, 100, 100, 64, None)
    assert (p.width, p.spans, p.buf) == (1, [], None)
    p = _Probe(0, 0, 10, None, 100, granule=None)
    assert (p.width, p.spans, p.buf) == (10, [(0, 10)], None)


def test_default_budget_is_read_at_call_time(monkeypatch):
    monkeypatch.setattr(engine, 'SEARCH_BLOCK_BYTES', 4 * 10 * 768)
    assert engine._block_budget(None) == 4 * 10 * 768 and engine._block_budget(12.0) == 12
    assert engine._block_spans(10, 0, 2000)[0] == 768
    assert engine._block_spans(10, 0, 2000, None, None, None)[0] == 768
    monkeypatch.setattr(engine, 'SEARCH_BLOCK_BYTES', 4 * 10 * 767)
    assert engine._block_spans(10, 0, 2000)[0] == 512
    assert engine._block_spans(10, 0, 2000, None, None, None)[0] == 767


# the rule of _SetBlocks: budget // (4 * max(nq, 1)) tracklet columns, no rounding and no floor
SET_RULE = [
    ((40, 0, 300, 64, None), (64, [(0, 64), (64, 128), (128, 192), (192, 256), (256, 300)])),
    ((40, 0, 300, None, 1), (1, [(c, c + 1) for c in range(300)])),           # a budget below 4 * nq: width 1
    ((40, 0, 300, None, 159), (1, [(c, c + 1) for c in range(300)])),
    ((40, 0, 300, None, 160 * 7 + 159), (7, [(c, min(c + 7, 300)) for c in range(0, 300, 7)])),
    ((3, 0, 1000, None, 8400), (700, [(0, 700), (700, 1000)])),               # no rounding to 256
    ((0, 0, 300, None, 4096), (300, [(0, 300)])),
    ((40, 100, 100, 64, None), (1, [])),
    ((40, 10, 75, 1000, None), (65, [(10, 75)])),
    ((5, 3, 40, None, 20 * 10), (10, [(3, 13), (13, 23), (23, 33), (33, 40)])),
]


@pytest.mark.parametrize('args,want', SET_RULE)
def test_set_width_rule(args, want):
    nq, lo, hi, block_cols, block_bytes = args
    assert engine._block_spans(nq, lo, hi, block_cols, block_bytes, granule=None) == want


def test_sample_and_rerank_rules_keep_their_results():
    # _SampleBlocks / _JaccardSet: multiples of 32 whose three buffers fit, never the whole matrix
    assert engine._sample_block_cols(1000, 1) == 32
    assert engine._sample_block_cols(1000, 12 * 1000 * 100) == 96
    assert engine._sample_block_cols(1000, 1 << 40) == 512                    # ceil(1000 / 64) * 32
    assert engine._sample_block_cols(10, 1 << 40) == 32
    assert engine._silhouette_width(40, 300, None, 1) == 256
    assert engine._silhouette_width(3, 1000, None, 8400) == 512
    assert engine._silhouette_width(40, 0, 64, None) == 1
    assert engine._silhouette_width(40, 65, 1000, None) == 65


def _refused(call, message):
    with pytest.raises(ValueError, match='^' + re.escape(message) + '$'):
        call()


def test_int_arg_messages_of_the_former_validators():
    ia = engine._int_arg
    # _pq_int and _hdbscan_int: 'in lo..hi'
    _refused(lambda: ia(9, 4, 8, 'pq_train', 'nbits'), 'pq_train: nbits must be an integer in 4..8 (got 9)')
    _refused(lambda: ia(1, 2, 2 ** 31 - 1, 'hdbscan', 'min_cluster_size'),
             'hdbscan: min_cluster_size must be an integer in 2..2147483647 (got 1)')
    # _roc_bits
    _refused(lambda: engine._roc_bits(21, 'pair_roc'), 'pair_roc: bits must be an integer in 8..20 (got 21)')
    # _diffusion_int: closed, and open-ended where the limit is the C int's
    _refused(lambda: engine._diffusion_int(0, 1, 128, 'diffusion_graph', 'k'),
             'diffusion_graph: k must be an integer in 1..128 (got 0)')
    _refused(lambda: engine._diffusion_int(-1, 0, 2 ** 31 - 1, 'diffusion_solve', 'n_iter'),
             'diffusion_solve: n_iter must be an integer in 0.. (got -1)')
    _refused(lambda: engine._diffusion_int(2 ** 31, 0, 2 ** 31 - 1, 'diffusion_solve', 'n_iter'),
             'diffusion_solve: n_iter must be an integer in 0.. (got 2147483648)')
    # _kmeans_int and _cluster_min_samples: '>= lo', the limit of 2**31 - 1 enforced and not printed
    _refused(lambda: engine._kmeans_int(0, 1, 'kmeans', 'k'), 'kmeans: k must be an integer >= 1 (got 0)')
    _refused(lambda: engine._kmeans_int(2 ** 31, 1, 'kmeans', 'k'), 'kmeans: k must be an integer >= 1 (got 2147483648)')
    assert engine._kmeans_int(2 ** 31 - 1, 1, 'kmeans', 'k') == 2 ** 31 - 1
    _refused(lambda: engine._cluster_min_samples(0, 'cluster'), 'cluster: min_samples must be an integer >= 1 (got 0)')
    _refused(lambda: engine._cluster_min_samples(2 ** 31, 'cluster'),
             'cluster: min_samples must be an integer >= 1 (got 2147483648)')
    # _pca_int: '>= lo' with no limit at all
    _refused(lambda: ia(-1, 0, None, 'pca', 'seed'), 'pca: seed must be an integer >= 0 (got -1)')
    assert ia(2 ** 40, 0, None, 'pca', 'seed') == 2 ** 40


@pytest.mark.parametrize('lo,hi', [(1, 8), (0, 0), (-3, 5), (2, 2 ** 31 - 1)])
def test_int_arg_accepts_and_refuses(lo, hi):
    ia = engine._int_arg
    for good in (lo, hi, np.int64(lo), np.int32(lo)):
        got = ia(good, lo, hi, 'f', 'v')
        assert got == good and type(got) is int
    assert ia(np.int64(5), 1, 8, 'f', 'v') == 5
    for bad in (True, False, 2.0, float(lo), np.float32(lo), None, str(lo), lo - 1, hi + 1, np.int64(lo - 1), np.int64(hi + 1)):
        with pytest.raises(ValueError, match=r'^f: v must be an integer in %d\.\.%d \(got ' % (lo, hi)):
            ia(bad, lo, hi, 'f', 'v')
    with pytest.raises(ValueError, match=r'^f: v must be an integer >= %d \(got ' % lo):
        ia(lo - 1, lo, None, 'f', 'v')
    assert ia(hi + 1, lo, None, 'f', 'v') == hi + 1


def test_search_k():
    assert engine.SEARCH_K_MAX == 1024
    for bad in (0, 1025, True, -1, False):
        _refused(lambda: engine._search_k(bad, 'search'), 'search: k must be in 1..1024 (got %r)' % (bad,))
    _refused(lambda: engine._search_k(1025, 'pq_search'), 'pq_search: k must be in 1..1024 (got 1025)')
    for good, want in ((1, 1), (1024, 1024), (np.int32(7), 7)):
        got = engine._search_k(good, 'search')
        assert got == want and type(got) is int


def test_check_index_words_the_article():
    class Other(object):
        pass
    for cls, text in ((engine.PqIndex, 'a PqIndex'), (engine.IvfPqIndex, 'an IvfPqIndex'),
                      (engine.BinaryIndex, 'a BinaryIndex'), (engine.Sq8Index, 'a Sq8Index')):
        _refused(lambda: engine._check_index(Other(), cls, 'f'), 'f: index must be %s (got Other)' % text)


def test_every_search_refuses_a_bool_k_before_any_device_call(monkeypatch):
    def fail(*a, **kw):
        raise AssertionError('a device call before the argument check')
    monkeypatch.setattr(engine, '_call', fail)
    monkeypatch.setattr(engine, 'gemm', fail)

    def bare(cls):                                       # an instance for the type checks that come before k
        return cls.__new__(cls)
    calls = {'search': lambda k: engine.search(None, None, k),
             'rerank_search': lambda k: engine.rerank_search(None, None, k),
             'set_search': lambda k: engine.set_search(bare(engine.TrackletSet), bare(engine.TrackletSet), k),
             'pq_search': lambda k: engine.pq_search(None, bare(engine.PqIndex), k),
             'ivf_search': lambda k: engine.ivf_search(None, bare(engine.IvfPqIndex), k, 1),
             'bin_search': lambda k: engine.bin_search(None, bare(engine.BinaryIndex), k),
             'sq8_search': lambda k: engine.sq8_search(None, bare(engine.Sq8Index), k)}
    for what, call in calls.items():
        for bad in (True, False, 0, 1025):
            _refused(lambda: call(bad), '%s: k must be in 1..1024 (got %r)' % (what, bad))
