"""The block-source contract (engine._BlockSource) for each of the five sources, and the running top-k list
(engine._TopK) they are ranked into: the blocks hold the materialised matrix's bits for every width, a block comes back
with the same bits when it is asked for again, ``_search_blocks`` over a source is ``rank_rows`` of that matrix, padding
included, and an empty side gives the empty result without a launch."""
import numpy as np
import pytest
import torch

from test_gpu_bin import _book as bin_book, _codes as bin_codes
from test_gpu_pq import _book as pq_book, _codes as pq_codes, _rows
from test_gpu_setdist import _make_sets

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NQ, N, D = 5, 37, 64
WIDTHS = (1, 7, N, None)
Q_COUNTS = [2, 1, 3, 1, 2]
G_COUNTS = [1 + i % 3 for i in range(N)]
NAMES = ('cosine', 'euclidean', 'pq', 'pq-euclidean', 'hamming', 'asymmetric', 'sq8', 'set')


def _bits(t):
    return t.contiguous().view(torch.int32)


class Case(object):
    """one source: ``make(block_cols, nq=NQ, n=N)`` builds it over the first nq queries and n columns; ``dist`` is the
    materialised [NQ, N] matrix, computed once and never written"""

    def __init__(self, name):
        from grl_amd import engine as E
        self.name = name
        qf, gf = _rows(NQ, D, 11), _rows(N, D, 12)
        if name in ('cosine', 'euclidean'):
            self.dist = E.cosin_dist(qf, gf) if name == 'cosine' else E.pairwise_distance_tensor(qf, gf)
            self.make = lambda bc, nq=NQ, n=N: E._ColumnBlocks(qf[:nq], gf[:n], name, bc)
        elif name in ('pq', 'pq-euclidean'):
            book = pq_book(2, 16, 32, 'euclidean' if name == 'pq-euclidean' else 'cosine')
            codes = pq_codes(N, 2, 16)
            index = {n: E.PqIndex(book, codes[:n]) for n in (N, 0)}       # (built here: a constructor may launch)
            self.dist = E.pq_dist(qf, index[N])
            self.make = lambda bc, nq=NQ, n=N: E._PqBlocks(qf[:nq], index[n], bc)
        elif name in ('hamming', 'asymmetric'):
            book, codes = bin_book(64, D), bin_codes(N, 64)
            index = {n: E.BinaryIndex(book, codes[:n]) for n in (N, 0)}
            self.dist = E.bin_dist(qf, index[N], name)
            self.make = lambda bc, nq=NQ, n=N: E._BinBlocks(qf[:nq], index[n], name, bc)
        elif name == 'sq8':
            book = E.sq8_train(gf)
            codes = book.encode(gf)
            index = {n: E.Sq8Index(book, codes[:n]) for n in (N, 0)}
            self.dist = E.sq8_dist(qf, index[N])
            self.make = lambda bc, nq=NQ, n=N: E._Sq8Blocks(qf[:nq], index[n], bc)
        else:
            qset, gset = _make_sets(Q_COUNTS, G_COUNTS, D, seed=13)
            self.dist = E.set_dist(qset, gset, 'chamfer', 'cosine')

            def make(bc, nq=NQ, n=N):
                qs = E.TrackletSet(qset.clips[:sum(Q_COUNTS[:nq])], Q_COUNTS[:nq])
                gs = E.TrackletSet(gset.clips[:sum(G_COUNTS[:n])], G_COUNTS[:n])
                return E._SetBlocks(qs, gs, 'chamfer', 'cosine', bc)
            self.make = make
        assert tuple(self.dist.shape) == (NQ, N) and self.dist.dtype == torch.float32
        self.order = E.rank_rows(self.dist).long()


_CASES = {}


@pytest.fixture(params=NAMES)
def case(request):
    if request.param not in _CASES:
        _CASES[request.param] = Case(request.param)
    return _CASES[request.param]


@pytest.fixture
def record(monkeypatch):
    """the names of every engine._call and 'gemm' for every engine.gemm, recorded while the calls go through"""
    from grl_amd import engine
    names, call, gemm = [], engine._call, engine.gemm
    monkeypatch.setattr(engine, '_call', lambda name, *a: (names.append(name), call(name, *a))[1])
    monkeypatch.setattr(engine, 'gemm', lambda *a, **kw: (names.append('gemm'), gemm(*a, **kw))[1])
    return names


def test_blocks_are_the_matrix_bits_for_every_width_and_again(case):
    from grl_amd import engine
    for bc in WIDTHS:
        blocks = case.make(bc)
        assert isinstance(blocks, engine._BlockSource) and blocks.nq == NQ and blocks.qf.device == case.dist.device
        want = N if bc is None else bc
        assert blocks.width == want and blocks.spans == [(c, min(c + want, N)) for c in range(0, N, want)]
        assert blocks.buf.numel() == NQ * want
        parts = []
        for c0, c1 in blocks.spans:
            first = blocks.block(c0, c1)
            assert tuple(first.shape) == (NQ, c1 - c0) and first.data_ptr() == blocks.buf.data_ptr()
            parts.append(first.clone())
            assert torch.equal(_bits(blocks.block(c0, c1)), _bits(parts[-1])), (case.name, bc, c0)
        assert torch.equal(_bits(torch.cat(parts, 1)), _bits(case.dist)), (case.name, bc)
        for c0, c1 in reversed(blocks.spans):                          # and in another order, after the others
            assert torch.equal(_bits(blocks.block(c0, c1)), _bits(case.dist[:, c0:c1])), (case.name, bc, c0)


def _expect(case, k, keep=None):
    """rank_rows of the matrix cut to k, -1 / +inf where a row has fewer entries (``keep`` [NQ, N] bool: the entries left)"""
    idx = torch.full((NQ, k), -1, dtype=torch.int64, device=DEV)
    val = torch.full((NQ, k), float('inf'), dtype=torch.float32, device=DEV)
    for q in range(NQ):
        row = case.order[q] if keep is None else case.order[q][keep[q][case.order[q]]]
        m = min(k, row.numel())
        idx[q, :m] = row[:m]
        val[q, :m] = case.dist[q][row[:m]]
    return val, idx


@pytest.mark.parametrize('k', (1, N, N + 3))
def test_search_blocks_is_rank_rows_of_the_matrix(case, k):
    from grl_amd import engine
    want_val, want_idx = _expect(case, k)
    for bc in WIDTHS:
        val, idx = engine._search_blocks(case.make(bc), NQ, k, False)
        assert idx.dtype == torch.int64 and val.dtype == torch.float32 and tuple(idx.shape) == tuple(val.shape) == (NQ, k)
        assert torch.equal(idx, want_idx), (case.name, bc)
        assert torch.equal(_bits(val), _bits(want_val)), (case.name, bc)


def test_an_empty_side_gives_the_empty_lists_without_a_launch(case, record):
    from grl_amd import engine
    inf = torch.tensor(float('inf'), device=DEV)
    for bc in WIDTHS:
        n_spans = len(case.make(bc).spans)
        del record[:]
        blocks = case.make(bc, nq=0)
        assert blocks.nq == 0 and blocks.buf is None and len(blocks.spans) == n_spans
        val, idx = engine._search_blocks(blocks, 0, 4, False)
        assert tuple(val.shape) == tuple(idx.shape) == (0, 4) and idx.dtype == torch.int64 and val.dtype == torch.float32
        blocks = case.make(bc, n=0)
        assert blocks.spans == [] and blocks.buf is None and blocks.width == 1
        val, idx = engine._search_blocks(blocks, NQ, 4, False)
        assert tuple(val.shape) == tuple(idx.shape) == (NQ, 4) and idx.dtype == torch.int64
        assert bool((idx == -1).all()) and bool((val == inf).all())
        assert record == [], (case.name, bc, record)


def test_topk_pushed_in_halves_is_the_whole(case, record):
    from grl_amd import engine
    k, h, r = 9, 16, 2
    dist = case.dist.clone()
    del record[:]
    whole = engine._TopK(NQ, k, DEV)
    assert bool((whole.key == -1).all()) and bool(torch.isinf(whole.val).all()) and whole.key.dtype == torch.int64
    whole.push(dist, N, N, 0)
    cols = engine._TopK(NQ, k, DEV)
    cols.push(dist, N, h, 0)
    cols.push(dist[:, h:], N, N - h, h)
    rows = engine._TopK(NQ, k, DEV)
    rows.push(dist[r:], N, N, 0, rows=(r, NQ))
    rows.push(dist, N, N, 0, rows=(0, r))
    assert record == ['grl_topk_block'] * 5
    for other in (cols, rows):
        assert torch.equal(other.key, whole.key) and torch.equal(_bits(other.val), _bits(whole.val)), case.name
    want_val, want_idx = _expect(case, k)
    val, idx = whole.result()
    assert torch.equal(idx, want_idx) and torch.equal(_bits(val), _bits(want_val))
    cidx = torch.arange(N, dtype=torch.int32, device=DEV).flip(0).repeat(NQ, 1).contiguous()    # entry ids of their own
    named = engine._TopK(NQ, k, DEV)
    named.push(dist.flip(1).contiguous(), N, N, 0, cidx, N)
    assert torch.equal(named.key, whole.key) and torch.equal(_bits(named.val), _bits(whole.val))


def test_the_junk_path_makes_filtered_calls_only(case, record):
    from grl_amd import engine
    g = np.random.Generator(np.random.PCG64(17))
    qp, gp, qc, gc = g.integers(0, 4, NQ), g.integers(0, 4, N), g.integers(0, 2, NQ), g.integers(0, 2, N)
    junk = engine._junk_ids((qp, gp, qc, gc), NQ, N, DEV)
    keep = torch.from_numpy(~((qp[:, None] == gp[None, :]) & (qc[:, None] == gc[None, :]))).to(DEV)
    assert 0 < int((~keep).sum()) < NQ * N
    for k in (3, N + 3):
        want_val, want_idx = _expect(case, k, keep)
        for bc in WIDTHS:
            blocks = case.make(bc)
            del record[:]
            val, idx = engine._search_blocks(blocks, NQ, k, False, junk)
            ranked = [name for name in record if name.startswith('grl_topk_block')]
            assert ranked == ['grl_topk_block_filtered'] * len(blocks.spans), (case.name, bc, ranked)
            assert torch.equal(idx, want_idx) and torch.equal(_bits(val), _bits(want_val)), (case.name, bc, k)
    rows = engine._TopK(NQ, 3, DEV)                                  # and by query rows: the junk arrays move with them
    del record[:]
    rows.push(case.dist[2:].contiguous(), N, N, 0, junk=junk, rows=(2, NQ))
    rows.push(case.dist, N, N, 0, junk=junk, rows=(0, 2))
    assert record == ['grl_topk_block_filtered'] * 2
    want_val, want_idx = _expect(case, 3, keep)
    assert torch.equal(rows.result()[1], want_idx) and torch.equal(_bits(rows.result()[0]), _bits(want_val))
