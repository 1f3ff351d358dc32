"""Time and peak device memory (over the inputs) of k-reciprocal re-ranking, materialised against streaming.

  mars: 1980 x 13290 at 6144-d (N = 15270): re_ranking + rank_rows + rank_metrics (rerank.hip) against
        engine.rerank_metrics_streaming and engine.rerank_search(k=100) (rerank_stream.hip)
  big:  10^4 queries x 10^5 gallery rows at 256-d, streaming only (the materialised path would need
        (q+g)^2 matrices of 48 GB each and refuses q + g > 16384)

One JSON line per measurement.  Usage: python tools/rerank_rate.py [--case mars|big|all] [--reps R] [--world W]

--world W > 1 starts W ranks that share cuda:0 and talk over gloo (as `bench.py --gpus 2` under GRL_SINGLE_DEVICE=1)
and times the sharded streaming paths only; every rank prints its own lines (`rank`, `world`).  On one device the
ranks share the compute units: the wall time there says what the exchange costs, not what W devices would gain."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from grl_amd import engine  # noqa: E402
from grl_amd.reid.evaluator.rerank import re_ranking  # noqa: E402
from grl_amd.synthetic import synth_eval_features  # noqa: E402


def measure(fn, reps):
    """(best seconds, peak bytes over what was allocated before) of fn()."""
    best, peak = float('inf'), 0
    for _ in range(reps):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
        peak = max(peak, torch.cuda.max_memory_allocated() - base)
    return best, peak


_WHO = {}                         # rank / world of a --world run, added to every line


def report(case, path, shape, sec, peak):
    print(json.dumps(dict({'case': case, 'path': path, 'nq': shape[0], 'ng': shape[1], 'dim': shape[2],
                           'seconds': round(sec, 4), 'peak_gib': round(peak / 2 ** 30, 3)}, **_WHO)), flush=True)


def run(case, nq, ng, dim, reps, materialised):
    # synth_eval_features builds three equal blocks: 255 = 3 x 85 plus a zero column gives 256-d with the same distances
    qf, gf, qp, qc, gp, gc = synth_eval_features(nq, ng, seed=1, dim=dim - dim % 3)
    pad = dim % 3
    qf, gf = (torch.nn.functional.pad(t, (0, pad)).cuda() for t in (qf, gf))
    with contextlib.redirect_stdout(io.StringIO()):            # kernels loaded, allocator warm
        engine.rerank_metrics_streaming(qf[:8], gf[:512], qp[:8], gp[:512], qc[:8], gc[:512])
    shape = (nq, ng, dim)
    if materialised:
        def mat():
            F = re_ranking(engine.cosin_dist(qf, gf), engine.pairwise_distance_tensor(qf, qf),
                           engine.pairwise_distance_tensor(gf, gf))
            engine.rank_metrics(engine.rank_rows(F), qp, gp, qc, gc)
        report(case, 'materialised re_ranking + rank_rows + rank_metrics', shape, *measure(mat, reps))
    report(case, 'rerank_metrics_streaming', shape,
           *measure(lambda: engine.rerank_metrics_streaming(qf, gf, qp, gp, qc, gc), reps))
    report(case, 'rerank_search k=100', shape, *measure(lambda: engine.rerank_search(qf, gf, 100), reps))


def cases(a, materialised=True):
    if a.case in ('mars', 'all'):
        run('mars', 1980, 13290, 6144, a.reps, materialised)
    if a.case in ('big', 'all'):
        run('big', 10000, 100000, 256, 1, False)


def rank_main(rank, a, port):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=a.world)
    _WHO.update(rank=rank, world=a.world)
    cases(a, materialised=False)
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', choices=['mars', 'big', 'all'], default='all')
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--world', type=int, default=1)
    a = ap.parse_args()
    if a.world > 1:
        import torch.multiprocessing as mp
        mp.spawn(rank_main, args=(a, 41000 + os.getpid() % 1500), nprocs=a.world, join=True)
    else:
        cases(a)


if __name__ == '__main__':
    main()
