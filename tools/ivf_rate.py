#!/usr/bin/env python
"""Times the IVF-PQ index (engine.ivf_train / ivf_index / ivf_search, ivf.hip) against engine.pq_search,
whose code it leaves alone and which is the yardstick, on tools/pq_rate.py's data recipe: synthetic unit rows with planted
identities at the MARS shape (1980 queries x 11310 gallery rows x 6144) and at a large gallery (1980 x 2^18 x 6144), M = 96,
nbits = 8, k = 100; the queries are the first rows of the gallery.

Per shape, one process; per (nlist, nprobe), nlist in {64, 1024}, nprobe in {1, nlist / 16, nlist}, the functions in turn,
15 warm-ups then 20 timed launches each (HIP events; the discipline of tools/verify_rate.py), median / min / max in ms:
  coarse        the probes (search over the coarse centroids) and G0 gathered at them
  tables        book.pq.lut(qf): M NEGDOT GEMMs into the [nq, M, ksub] residual tables
  scan          grl_ivf_scan over all probe chunks (probes, tables and offsets' inputs already there)
  scan_topk     the same chunks through grl_topk_block with the scan's cidx
  ivf_search    engine.ivf_search(qf, index, 100, nprobe): all of the above
and pq_search once per shape.  Once each: the train and encode wall times, the scanned fraction, recall@1 / 10 / 100 of
ivf_search and of pq_search against exact search, the index bytes.

  python tools/ivf_rate.py [--shape mars|large|both] [--nlist 64,1024] [--warm 15] [--reps 20] [--M 96] [--nbits 8]
                           [--max-iter 25] [--train-rows 65536] [--noise 1.0] [--json PATH]
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


def chunks(index, nq, nprobe):
    """(rows, spans): the query rows per block and the (j0, j1, width) probe chunks ivf_search serves"""
    from grl_amd import engine
    rows, per = engine._ivf_plan(index, nq, nprobe, None)
    return rows, [(j0, min(j0 + per, nprobe), min(index._longest[min(j0 + per, nprobe) - j0], index.n))
                  for j0 in range(0, nprobe, per)]


def measure(name, a, dev):
    from grl_amd import engine
    from grl_amd._lib import ptr
    nq, n = SHAPES[name]
    d, k = 6144, 100
    gf, _ = planted_rows(n, d, max(2, n // 18), a.noise, 1, dev)
    qf = gf[:nq].contiguous()
    res = {'shape': name, 'nq': nq, 'n': n, 'd': d, 'M': a.M, 'nbits': a.nbits, 'k': k, 'noise': a.noise, 'runs': []}
    t_rows = min(n, a.train_rows)
    exact = engine.search(qf, gf, k)[1]
    flat_book, res['pq_train_s'] = wall(lambda: engine.pq_train(gf[:t_rows], a.M, a.nbits, 'cosine', a.max_iter, 0))
    flat, res['pq_encode_s'] = wall(lambda: engine.pq_index(gf, flat_book))
    res['pq_index_bytes'], res['feature_bytes'] = int(flat.nbytes), 4 * n * d
    res['pq_recall'] = dict(zip(('1', '10', '100'), engine.topk_recall(engine.pq_search(qf, flat, k)[1], exact, (1, 10, 100))))
    res['pq_search_ms'] = in_turn({'pq_search': lambda: engine.pq_search(qf, flat, k)}, a.warm, a.reps)['pq_search']
    print(json.dumps({key: v for key, v in res.items() if key != 'runs'}), flush=True)
    del flat, flat_book
    for nlist in a.nlist:
        book, train_s = wall(lambda: engine.ivf_train(gf[:t_rows], nlist, a.M, a.nbits, 'cosine', a.max_iter, 0))
        index, encode_s = wall(lambda: engine.ivf_index(gf, book))
        for nprobe in sorted(set((1, max(1, nlist // 16), min(nlist, engine.IVF_NPROBE_MAX)))):
            run = {'nlist': nlist, 'nprobe': nprobe, 'train_s': train_s, 'encode_s': encode_s, 'train_rows': t_rows,
                   'coarse_iters': book.coarse_n_iter, 'index_bytes': int(index.nbytes),
                   'list_len': [index.list_len_min, n / float(nlist), index.list_len_max]}
            run['scanned_fraction'] = float(engine.ivf_probe_stats(qf, index, nprobe).sum()) / (nq * float(n))
            rows, spans = chunks(index, nq, nprobe)
            blocks = [(q0, engine._IvfQueries(qf[q0:q0 + rows], index, nprobe)) for q0 in range(0, nq, rows)]
            run['query_blocks'], run['chunks'], run['chunk_width'] = len(blocks), len(spans), spans[0][2]
            run_key = torch.empty((nq, k), dtype=torch.int64, device=dev)
            run_val = torch.empty((nq, k), dtype=torch.float32, device=dev)

            def scan():
                for q0, qs in blocks:
                    for j0, j1, width in spans:
                        qs.chunk(j0, j1, width)

            def scan_topk():
                run_key.fill_(-1)
                run_val.fill_(float('inf'))
                for q0, qs in blocks:
                    for j0, j1, width in spans:
                        dd, cidx = qs.chunk(j0, j1, width)
                        engine._call('grl_topk_block', ptr(dd), width, ptr(cidx), width, qs.nq, width, 0, k, ptr(run_key[q0:]),
                                     ptr(run_val[q0:]))
            fns = {'coarse': lambda: engine._ivf_probe(qf, book, nprobe),
                   'tables': lambda: book.pq.lut(qf),
                   'scan': scan,
                   'scan_topk': scan_topk,
                   'ivf_search': lambda: engine.ivf_search(qf, index, k, nprobe)}
            run['ms'] = in_turn(fns, a.warm, a.reps)
            run['ivf_search_over_pq_search'] = run['ms']['ivf_search'][0] / res['pq_search_ms'][0]
            run['recall'] = dict(zip(('1', '10', '100'),
                                     engine.topk_recall(engine.ivf_search(qf, index, k, nprobe)[1], exact, (1, 10, 100))))
            res['runs'].append(run)
            print(json.dumps(run), flush=True)
            del blocks
        del index, book
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='both', choices=('mars', 'large', 'both'))
    ap.add_argument('--nlist', default='64,1024', type=lambda s: [int(v) for v in s.split(',')])
    ap.add_argument('--warm', type=int, default=15)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--M', type=int, default=96)
    ap.add_argument('--nbits', type=int, default=8)
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
