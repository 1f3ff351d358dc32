#!/usr/bin/env python
"""Times the exact refinement of shortlists (engine.RefineStore / refine_lists / refine_search, refine.hip)
on tools/pq_rate.py's data recipe: synthetic unit rows with planted identities at the MARS shape (1980 queries x 11310
gallery rows x 6144) and at a large gallery (1980 x 2^18 x 6144), M = 96, nbits = 8, k = 100; the queries are the first
rows of the gallery.  The IVF index has nlist = 64 and is searched at nprobe = 4.

Per shape, one process; per (R, store type), R in {100, 200, 1000}, store in {f32, bf16}, the functions in turn, 15
warm-ups then 20 timed launches each (HIP events; the discipline of tools/verify_rate.py), median / min / max in ms:
  scan              grl_refine_scan alone over pq_search's lists of R candidates (one launch, buffers already there)
  refine_lists      engine.refine_lists on the same lists: the scan and grl_topk_block
  refine_pq         engine.refine_search over the PqIndex: pq_search at R, then refine_lists
  refine_ivf        engine.refine_search over the IvfPqIndex: ivf_search at R, then refine_lists
and once per shape engine.search, pq_search and ivf_search at k.  Derived: the scan's gathered bytes per second,
nq * R * d * (4 | 2) / time (padding entries are not counted), and recall@1 / 10 / 100 against exact search before and
after refinement.

  python tools/refine_rate.py [--shape mars|large|both] [--R 100,200,1000] [--warm 15] [--reps 20] [--M 96] [--nbits 8]
                              [--nlist 64] [--nprobe 4] [--max-iter 25] [--train-rows 65536] [--noise 1.0] [--json PATH]
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


def measure(name, a, dev):
    from grl_amd import engine
    nq, n = SHAPES[name]
    d, k = 6144, 100
    gf, _ = planted_rows(n, d, max(2, n // 18), a.noise, 1, dev)
    qf = gf[:nq].contiguous()
    res = {'shape': name, 'nq': nq, 'n': n, 'd': d, 'M': a.M, 'nbits': a.nbits, 'k': k, 'noise': a.noise, 'nlist': a.nlist,
           'nprobe': a.nprobe, 'runs': []}
    t_rows = min(n, a.train_rows)
    exact = engine.search(qf, gf, k)[1]
    flat = engine.pq_index(gf, engine.pq_train(gf[:t_rows], a.M, a.nbits, 'cosine', a.max_iter, 0))
    ivf = engine.ivf_index(gf, engine.ivf_train(gf[:t_rows], a.nlist, a.M, a.nbits, 'cosine', a.max_iter, 0))

    def recall(idx):
        return dict(zip(('1', '10', '100'), engine.topk_recall(idx, exact, KS)))
    res['pq_recall'] = recall(engine.pq_search(qf, flat, k)[1])
    res['ivf_recall'] = recall(engine.ivf_search(qf, ivf, k, a.nprobe)[1])
    res['ms'] = in_turn({'search': lambda: engine.search(qf, gf, k),
                         'pq_search': lambda: engine.pq_search(qf, flat, k),
                         'ivf_search': lambda: engine.ivf_search(qf, ivf, k, a.nprobe)}, a.warm, a.reps)
    res['feature_bytes'], res['pq_index_bytes'], res['ivf_index_bytes'] = 4 * n * d, int(flat.nbytes), int(ivf.nbytes)
    print(json.dumps({key: v for key, v in res.items() if key != 'runs'}), flush=True)
    for dtype in ('f32', 'bf16'):
        store, pack_s = wall(lambda: engine.RefineStore(gf, dtype))
        for R in a.R:
            cand = engine.pq_search(qf, flat, R)[1]
            live = int((cand >= 0).sum())
            out = torch.empty((nq, R), dtype=torch.float32, device=dev)
            cidx = torch.empty((nq, R), dtype=torch.int32, device=dev)
            fns = {'scan': lambda: engine._refine_scan(qf, store, cand, 'cosine', out, cidx),
                   'refine_lists': lambda: engine.refine_lists(qf, store, cand, k),
                   'refine_pq': lambda: engine.refine_search(qf, flat, store, k, R),
                   'refine_ivf': lambda: engine.refine_search(qf, ivf, store, k, R, nprobe=a.nprobe)}
            run = {'store': dtype, 'R': R, 'store_bytes': int(store.nbytes), 'pack_s': pack_s, 'live_candidates': live,
                   'distinct_rows': int(torch.unique(cand[cand >= 0]).numel()), 'ms': in_turn(fns, a.warm, a.reps)}
            gathered = live * d * (4 if dtype == 'f32' else 2)
            run['gathered_bytes'] = gathered
            run['scan_TBps'] = [gathered / (t * 1e-3) / 1e12 for t in run['ms']['scan']]
            run['refine_pq_over_search'] = run['ms']['refine_pq'][0] / res['ms']['search'][0]
            run['refine_ivf_over_search'] = run['ms']['refine_ivf'][0] / res['ms']['search'][0]
            run['refined_pq_recall'] = recall(engine.refine_search(qf, flat, store, k, R)[1])
            run['refined_ivf_recall'] = recall(engine.refine_search(qf, ivf, store, k, R, nprobe=a.nprobe)[1])
            res['runs'].append(run)
            print(json.dumps(run), flush=True)
        del store
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='both', choices=('mars', 'large', 'both'))
    ap.add_argument('--R', default='100,200,1000', type=lambda s: [int(v) for v in s.split(',')])
    ap.add_argument('--warm', type=int, default=15)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--M', type=int, default=96)
    ap.add_argument('--nbits', type=int, default=8)
    ap.add_argument('--nlist', type=int, default=64)
    ap.add_argument('--nprobe', type=int, default=4)
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
