#!/usr/bin/env python
"""Times the binary-code index (engine.bin_train / bin_index / bin_search, bin.hip) next to the product
quantiser at the same bytes per row (M = nbits / 8, ksub = 256) and to exact search, on tools/pq_rate.py's data recipe:
synthetic unit rows with planted identities made on the device, the queries the first rows of the gallery, at the MARS
shape (1980 x 11310 x 6144) and a large gallery (1980 x 2^18 x 6144).

Per shape, one process, the functions in turn, 15 warm-ups then 20 timed launches each (HIP events; the discipline of
tools/verify_rate.py), medians:
  bin_scan        grl_bin_scan over all column blocks (the query codes already there)
  asym_scan       grl_pq_scan over the asymmetric tables of the binary index (the tables already there)
  pq_scan         grl_pq_scan over the product quantiser's codes (M = nbits / 8, ksub = 256; the tables already there)
  bin_search      engine.bin_search(qf, index, 100, 'hamming'): projection + pack + scan + top-k
  asym_search     engine.bin_search(qf, index, 100, 'asymmetric'): projection + tables + scan + top-k
  pq_search       engine.pq_search(qf, pq_index, 100)
  exact_search    engine.search(qf, gf, 100) on the raw features
and, once each: the train and encode wall times, recall@10 of each search against exact search, the index bytes.  The
figure the issue asks for is bin_scan / pq_scan: both read the same words, one does a population count per dword where the
other does four LDS gathers.

  python tools/bin_rate.py [--shape mars|large|both] [--warm 15] [--reps 20] [--nbits 256] [--method itq] [--n-iter 50]
                           [--pq-max-iter 25] [--train-rows 65536] [--noise 1.0] [--json PATH]
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


def measure(name, a, dev):
    from grl_amd import engine
    nq, n = SHAPES[name]
    d, k, M = 6144, 100, a.nbits // 8
    gf, _ = planted_rows(n, d, max(2, n // 18), a.noise, 1, dev)
    qf = gf[:nq].contiguous()
    res = {'shape': name, 'nq': nq, 'n': n, 'd': d, 'nbits': a.nbits, 'method': a.method, 'M': M, 'k': k, 'noise': a.noise}
    t_rows = min(n, a.train_rows)
    res['train_rows'] = t_rows
    book, res['bin_train_s'] = wall(lambda: engine.bin_train(gf[:t_rows], a.nbits, a.method, a.n_iter, 0))
    res['objective'] = None if book.objective is None else [book.objective[0], book.objective[-1]]
    index, res['bin_encode_s'] = wall(lambda: engine.bin_index(gf, book))
    pq_book, res['pq_train_s'] = wall(lambda: engine.pq_train(gf[:t_rows], M, 8, 'cosine', a.pq_max_iter, 0))
    pq_index, res['pq_encode_s'] = wall(lambda: engine.pq_index(gf, pq_book))
    res['bin_index_bytes'], res['pq_index_bytes'], res['feature_bytes'] = int(index.nbytes), int(pq_index.nbytes), 4 * n * d
    ham = engine._BinBlocks(qf, index, 'hamming')
    asym = engine._BinBlocks(qf, index, 'asymmetric')
    pq = engine._PqBlocks(qf, pq_index)
    res['blocks'], res['block_cols'] = len(ham.spans), ham.width

    def scan(blocks):
        def run():
            for c0, c1 in blocks.spans:
                blocks.block(c0, c1)
        return run
    fns = {'bin_scan': scan(ham), 'asym_scan': scan(asym), 'pq_scan': scan(pq),
           'bin_search': lambda: engine.bin_search(qf, index, k, 'hamming'),
           'asym_search': lambda: engine.bin_search(qf, index, k, 'asymmetric'),
           'pq_search': lambda: engine.pq_search(qf, pq_index, k),
           'exact_search': lambda: engine.search(qf, gf, k)}
    res['ms'] = in_turn(fns, a.warm, a.reps)
    ms = {key: v[0] for key, v in res['ms'].items()}
    res['bin_scan_over_pq_scan'] = ms['bin_scan'] / ms['pq_scan']
    res['bin_search_over_pq_search'] = ms['bin_search'] / ms['pq_search']
    res['bin_search_over_exact_search'] = ms['bin_search'] / ms['exact_search']
    t = ms['bin_scan'] * 1e-3
    res['bin_scan_pairs_per_s'] = nq * float(n) / t
    res['bin_scan_out_gb_per_s'] = 4.0 * nq * n / t / 1e9            # the distance block it writes
    exact = engine.search(qf, gf, k)[1]
    res['recall_at_10'] = {
        'bin_search': engine.topk_recall(engine.bin_search(qf, index, k, 'hamming')[1], exact, (10,))[0],
        'asym_search': engine.topk_recall(engine.bin_search(qf, index, k, 'asymmetric')[1], exact, (10,))[0],
        'pq_search': engine.topk_recall(engine.pq_search(qf, pq_index, k)[1], exact, (10,))[0],
        'exact_search': 1.0}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='both', choices=('mars', 'large', 'both'))
    ap.add_argument('--warm', type=int, default=15)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--nbits', type=int, default=256)
    ap.add_argument('--method', default='itq', choices=('itq', 'lsh'))
    ap.add_argument('--n-iter', type=int, default=50)
    ap.add_argument('--pq-max-iter', type=int, default=25)
    ap.add_argument('--train-rows', type=int, default=65536)
    ap.add_argument('--noise', type=float, default=1.0)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {'device': torch.cuda.get_device_name(0), 'warm': a.warm, 'reps': a.reps, 'shapes': []}
    for name in (('mars', 'large') if a.shape == 'both' else (a.shape,)):
        out['shapes'].append(measure(name, a, dev))
        print(json.dumps(out['shapes'][-1]), flush=True)
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
