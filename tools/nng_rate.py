#!/usr/bin/env python
"""Times the kNN-graph index (engine.nng_build / nng_search, nng.hip) on tools/pq_rate.py's data recipe:
synthetic unit rows with planted identities at the MARS shape (1980 queries x 11310 gallery rows x 6144) and at a large
gallery (1980 x 2^18 x 6144), k = 100; the queries are the first rows of the gallery.  The graph has K = 64 candidates
per row -- the exact lists (engine.nng_knn) at the MARS shape, the lists of refine_search over a flat PQ index (M = 96,
nbits = 8, R = 200, the row itself among them and dropped by the optimiser) at the large one -- and degree D = 32.

Per shape, one process; per store type (f32, bf16) and per (L, w, T) of the sweep, 15 warm-ups then 20 timed calls in
turn (HIP events; the discipline of tools/verify_rate.py), median / min / max in ms:
  nng_search        engine.nng_search at k = min(100, L) from the default seeds
  scan              grl_refine_scan over random id lists of R = mean visited rows per query from the same store: the same
                    gather without the dependent chain -- the yardstick of the walk's rate
and once per shape engine.search and both refine_search routes (flat PQ, IVF-PQ with nlist = 64 at nprobe = 4; R = 200)
on the f32 store.  Derived: visited rows per query (mean), gathered bytes per second = visited * d * (4 | 2) / time for
the walk and for the scan, their ratio, recall@1 / 10 / 100 against exact search, the build times.

  python tools/nng_rate.py [--shape mars|large|both] [--sweep 128:1:64,256:1:64] [--K 64] [--D 32] [--warm 15] [--reps 20]
                           [--M 96] [--nbits 8] [--nlist 64] [--nprobe 4] [--R 200] [--max-iter 25] [--train-rows 65536]
                           [--noise 1.0] [--json PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pq_rate import SHAPES, planted_rows, wall  # noqa: E402
from verify_rate import in_turn  # noqa: E402

KS = (1, 10, 100)


def approx_lists(gf, flat, store, K, R, rows=8192):
    """int64 [n, K + 1]: refine_search of the rows against their own index, in query blocks"""
    from grl_amd import engine
    out = []
    for r0 in range(0, gf.shape[0], rows):
        out.append(engine.refine_search(gf[r0:r0 + rows], flat, store, K + 1, R)[1])
    return torch.cat(out, 0)


def measure(name, a, dev):
    from grl_amd import engine
    nq, n = SHAPES[name]
    d, k = 6144, 100
    gf, _ = planted_rows(n, d, max(2, n // 18), a.noise, 1, dev)
    qf = gf[:nq].contiguous()
    res = {'shape': name, 'nq': nq, 'n': n, 'd': d, 'k': k, 'K': a.K, 'D': a.D, 'noise': a.noise, 'runs': []}
    exact = engine.search(qf, gf, k)[1]
    t_rows = min(n, a.train_rows)
    flat = engine.pq_index(gf, engine.pq_train(gf[:t_rows], a.M, a.nbits, 'cosine', a.max_iter, 0))
    ivf = engine.ivf_index(gf, engine.ivf_train(gf[:t_rows], a.nlist, a.M, a.nbits, 'cosine', a.max_iter, 0))
    f32 = engine.RefineStore(gf, 'f32')

    def recall(idx, upto):
        r = engine.topk_recall(idx, exact, [kk for kk in KS if kk <= upto])
        return dict(zip(('1', '10', '100'), r))
    if name == 'mars':
        knn, res['knn_s'] = wall(lambda: engine.nng_knn(f32, a.K))
        res['knn'] = 'exact (nng_knn)'
    else:
        knn, res['knn_s'] = wall(lambda: approx_lists(gf, flat, f32, a.K, a.R))
        res['knn'] = 'refine_search over the flat PQ index, R = %d' % a.R
    table, res['optimize_s'] = wall(lambda: engine.nng_optimize(knn, a.D))
    res['table_bytes'], res['feature_bytes'] = int(table.numel()) * 4, 4 * n * d
    res['live_degree_mean'] = float((table >= 0).sum()) / n
    res['ms'] = in_turn({'search': lambda: engine.search(qf, gf, k),
                         'refine_pq': lambda: engine.refine_search(qf, flat, f32, k, a.R),
                         'refine_ivf': lambda: engine.refine_search(qf, ivf, f32, k, a.R, nprobe=a.nprobe)}, a.warm, a.reps)
    res['refine_pq_recall'] = recall(engine.refine_search(qf, flat, f32, k, a.R)[1], k)
    res['refine_ivf_recall'] = recall(engine.refine_search(qf, ivf, f32, k, a.R, nprobe=a.nprobe)[1], k)
    print(json.dumps({key: v for key, v in res.items() if key != 'runs'}), flush=True)
    del flat, ivf
    for dtype in ('f32', 'bf16'):
        store = f32 if dtype == 'f32' else engine.RefineStore(gf, 'bf16')
        index = engine.NnGraphIndex(store, table, 'cosine')
        for L, w, T in a.sweep:
            kk = min(k, L)
            _, idx, stats = engine.nng_search(qf, index, kk, L, w, T, return_stats=True)
            visited = float(stats[:, 0].sum()) / nq
            R = max(1, int(round(visited)))
            cand = torch.randint(0, n, (nq, R), device=dev)
            out = torch.empty((nq, R), dtype=torch.float32, device=dev)
            cidx = torch.empty((nq, R), dtype=torch.int32, device=dev)
            ms = in_turn({'nng_search': lambda: engine.nng_search(qf, index, kk, L, w, T),
                          'scan': lambda: engine._refine_scan(qf, store, cand, 'cosine', out, cidx)}, a.warm, a.reps)
            width = 4 if dtype == 'f32' else 2
            run = {'store': dtype, 'L': L, 'w': w, 'T': T, 'k': kk, 'visited_mean': visited,
                   'iterations_mean': float(stats[:, 1].sum()) / nq, 'ms': ms,
                   'walk_TBps': visited * nq * d * width / (ms['nng_search'][0] * 1e-3) / 1e12,
                   'scan_TBps': R * nq * d * width / (ms['scan'][0] * 1e-3) / 1e12,
                   'recall': recall(idx, kk), 'over_search': ms['nng_search'][0] / res['ms']['search'][0]}
            run['walk_over_scan_rate'] = run['walk_TBps'] / run['scan_TBps']
            res['runs'].append(run)
            print(json.dumps(run), flush=True)
        del index, store
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='both', choices=('mars', 'large', 'both'))
    ap.add_argument('--sweep', default='64:1:64,128:1:64,128:1:96,128:2:48,256:1:64,256:2:32',
                    type=lambda s: [tuple(int(v) for v in t.split(':')) for t in s.split(',')])
    ap.add_argument('--K', type=int, default=64)
    ap.add_argument('--D', type=int, default=32)
    ap.add_argument('--warm', type=int, default=15)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--M', type=int, default=96)
    ap.add_argument('--nbits', type=int, default=8)
    ap.add_argument('--nlist', type=int, default=64)
    ap.add_argument('--nprobe', type=int, default=4)
    ap.add_argument('--R', type=int, default=200)
    ap.add_argument('--max-iter', type=int, default=25)
    ap.add_argument('--train-rows', type=int, default=65536)
    ap.add_argument('--noise', type=float, default=1.0)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {'device': torch.cuda.get_device_name(0), 'warm': a.warm, 'reps': a.reps, 'shapes': []}
    for name in (('mars', 'large') if a.shape == 'both' else (a.shape,)):
        out['shapes'].append(measure(name, a, dev))
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
