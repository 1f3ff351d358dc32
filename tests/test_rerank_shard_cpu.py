"""Index logic of the sharded streaming re-ranking (grl_amd.dist: the sample-range split, the shard offsets and the
uneven all-gather), under gloo with CPU tensors in worlds of two and three ranks.  The kernels have no CPU form;
what runs here is the plumbing between them."""
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shard_bounds_are_a_contiguous_split_with_sizes_at_most_one_apart():
    from grl_amd import dist as grl_dist
    for n in (0, 1, 2, 3, 7, 299, 441, 15270):
        for world in (1, 2, 3, 8):
            b = grl_dist.shard_bounds(n, world)
            assert len(b) == world + 1 and b[0] == 0 and b[-1] == n
            sizes = [b[r + 1] - b[r] for r in range(world)]
            assert min(sizes) >= 0 and max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)
            for r in range(world):
                assert grl_dist.shard_rows(n, r, world) == (b[r], b[r + 1])
    assert grl_dist.shard_bounds(299, 2) == [0, 150, 299]
    assert grl_dist.shard_bounds(299, 3) == [0, 100, 200, 299]


def _csr(n_rows, seed):
    """Row counts (some zero) and entries whose value names their position: entry e of the whole CSR is e."""
    g = torch.Generator().manual_seed(seed)
    cnt = torch.randint(0, 6, (n_rows,), generator=g, dtype=torch.int32)
    cnt[::5] = 0
    cnt[1:8] += 3                      # front-loaded, so that equal row ranges hold unequal numbers of entries
    return cnt, torch.arange(int(cnt.sum()), dtype=torch.int32)


def _worker(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    from grl_amd import dist as grl_dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    out = {}
    # rows of a [n, 4] table and of a vector, each rank holding its own range only
    for n in (11, 3, 2, 1):                                   # fewer rows than ranks: some shares are empty
        bounds = grl_dist.shard_bounds(n, world)
        lo, hi = bounds[rank], bounds[rank + 1]
        table = torch.full((n, 4), -1.0)
        table[lo:hi] = torch.arange(n * 4, dtype=torch.float32).view(n, 4)[lo:hi]
        vec = torch.full((n,), -1, dtype=torch.int32)
        vec[lo:hi] = torch.arange(n, dtype=torch.int32)[lo:hi]
        out['table%d' % n] = grl_dist.gather_row_ranges(table, bounds)
        out['vec%d' % n] = grl_dist.gather_row_ranges(vec, bounds)
    # the V2 exchange: row counts first, then every rank's packed entries placed at the prefix sum of its first row
    n = 23
    cnt_all, ent_all = _csr(n, 5)
    bounds = grl_dist.shard_bounds(n, world)
    lo, hi = bounds[rank], bounds[rank + 1]
    cnt = torch.zeros(n, dtype=torch.int32)
    cnt[lo:hi] = cnt_all[lo:hi]
    grl_dist.gather_row_ranges(cnt, bounds)
    row_ptr = torch.zeros(n + 1, dtype=torch.int64)
    torch.cumsum(cnt, 0, out=row_ptr[1:])
    at = [int(row_ptr[b]) for b in bounds]
    sizes = [at[r + 1] - at[r] for r in range(world)]
    parts = grl_dist.all_gather_uneven(ent_all[at[rank]:at[rank + 1]], sizes)
    assert [p.numel() for p in parts] == sizes
    ent = torch.full((int(row_ptr[-1]),), -1, dtype=torch.int32)
    for r, p in enumerate(parts):
        ent[at[r]:at[r + 1]] = p
    out['cnt'], out['ent'], out['sizes'] = cnt, ent, sizes
    out['nothing'] = [p.numel() for p in grl_dist.all_gather_uneven(torch.zeros(0, dtype=torch.int32), [0] * world)]
    try:
        grl_dist.all_gather_uneven(torch.zeros(2), [3] * world)
        out['mismatch'] = 'accepted'
    except ValueError:
        out['mismatch'] = 'refused'
    torch.save(out, os.path.join(outdir, 'rank%d.pt' % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('world', [2, 3])
def test_uneven_gathers_give_every_rank_the_whole(world, tmp_path):
    port = 39900 + 7 * world + os.getpid() % 1500
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    cnt_all, ent_all = _csr(23, 5)
    for r in range(world):
        out = torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r), weights_only=False)
        for n in (11, 3, 2, 1):
            assert torch.equal(out['table%d' % n], torch.arange(n * 4, dtype=torch.float32).view(n, 4)), (r, n)
            assert torch.equal(out['vec%d' % n], torch.arange(n, dtype=torch.int32)), (r, n)
        assert torch.equal(out['cnt'], cnt_all) and torch.equal(out['ent'], ent_all)
        assert sum(out['sizes']) == ent_all.numel() and len(set(out['sizes'])) > 1       # the shards ARE uneven
        assert out['nothing'] == [0] * world and out['mismatch'] == 'refused'
