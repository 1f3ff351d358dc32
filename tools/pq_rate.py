#!/usr/bin/env python
"""Times the product-quantised index (engine.pq_train / pq_index / pq_search, pq.hip) against exact
search on synthetic unit rows with planted identities, at two shapes: the MARS shape (1980 queries x 11310 gallery rows
x 6144) and a large gallery (1980 x 2^18 x 6144: 6.4 GB of features), M = 96, nbits = 8.  The rows are made on the device
(a 2^18 x 6144 host array would take longer to make than everything measured here): identity centres plus noise,
normalised; the queries are the first rows of the gallery, as the evaluator prepends them.

Per shape, one process, the functions in turn, 15 warm-ups then 20 timed launches each (HIP events; the discipline of
tools/verify_rate.py), medians:
  tables        codebook.lut(qf): M NEGDOT GEMMs into the [nq, M, ksub] tables
  scan          grl_pq_scan over all column blocks of the index (the tables already there)
  scan_topk     the same blocks through search's running top-k (k = 100)
  pq_search     engine.pq_search(qf, index, 100): tables + scan + top-k
  exact_search  engine.search(qf, gf, 100) on the raw features
and, once each: the train and encode wall times, recall@1 / 10 / 100 of pq_search against exact search, the index bytes
against the feature bytes.  The scan's lookups per second (nq n M / t) are put next to the LDS rate of the read it uses
(one ds_read_b128 serves four queries: 256 B / clk / CU = 64 lookups / clk / CU, 256 CUs, the clock the device reports).

  python tools/pq_rate.py [--shape mars|large|both] [--warm 15] [--reps 20] [--M 96] [--nbits 8] [--max-iter 25]
                          [--train-rows 65536] [--noise 1.0] [--json PATH]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from verify_rate import in_turn  # noqa: E402

SHAPES = {'mars': (1980, 11310), 'large': (1980, 1 << 18)}


def planted_rows(n, d, n_ids, noise, seed, dev, chunk=16384):
    """[n, d] unit rows on the device, made in chunks: row i = unit(centre[pid_i] + e), the centres unit vectors and e ~
    N(0, noise^2 / d) per column (|e| ~ noise).  Returns (rows, pids)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    centres = torch.randn((n_ids, d), generator=g, device=dev)
    centres /= centres.norm(dim=1, keepdim=True)
    pids = torch.randint(0, n_ids, (n,), generator=g, device=dev)
    x = torch.empty((n, d), dtype=torch.float32, device=dev)
    for r0 in range(0, n, chunk):
        r1 = min(r0 + chunk, n)
        rows = centres[pids[r0:r1]] + (noise / float(np.sqrt(d))) * torch.randn((r1 - r0, d), generator=g, device=dev)
        x[r0:r1] = rows / rows.norm(dim=1, keepdim=True)
    return x, pids.cpu().numpy()


def device_clock_hz():
    """(Hz, where it came from): the device properties' clock, else the management library's current clock, else the
    part's nominal 2.4 GHz (said so in the result)."""
    rate = getattr(torch.cuda.get_device_properties(0), 'clock_rate', None)
    if rate:
        return rate * 1e3, 'device properties'
    try:
        return float(torch.cuda.clock_rate()) * 1e6, 'management library'
    except Exception:                                             # noqa: BLE001
        return 2.4e9, 'nominal'


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def measure(name, a, dev):
    from grl_amd import engine
    nq, n = SHAPES[name]
    d, k = 6144, 100
    gf, pids = planted_rows(n, d, max(2, n // 18), a.noise, 1, dev)
    qf = gf[:nq].contiguous()
    res = {'shape': name, 'nq': nq, 'n': n, 'd': d, 'M': a.M, 'nbits': a.nbits, 'k': k, 'noise': a.noise}
    t_rows = min(n, a.train_rows)
    book, res['train_s'] = wall(lambda: engine.pq_train(gf[:t_rows], a.M, a.nbits, 'cosine', a.max_iter, 0))
    res['train_rows'], res['train_iters'] = t_rows, [int(min(book.n_iter)), int(max(book.n_iter))]
    index, res['encode_s'] = wall(lambda: engine.pq_index(gf, book))
    res['index_bytes'], res['feature_bytes'] = int(index.nbytes), 4 * n * d
    res['memory_ratio'] = res['feature_bytes'] / float(index.nbytes)
    blocks = engine._PqBlocks(qf, index)
    res['blocks'], res['block_cols'] = len(blocks.spans), blocks.width
    res['lut_bytes'] = 4 * blocks.lut.numel()

    def scan():
        for c0, c1 in blocks.spans:
            blocks.block(c0, c1)
    fns = {'tables': lambda: book.lut(qf),
           'scan': scan,
           'scan_topk': lambda: engine._search_blocks(blocks, nq, k, False),
           'pq_search': lambda: engine.pq_search(qf, index, k),
           'exact_search': lambda: engine.search(qf, gf, k)}
    res['ms'] = in_turn(fns, a.warm, a.reps)
    t_scan = res['ms']['scan'][0] * 1e-3
    clock_hz, res['clock_source'] = device_clock_hz()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res['clock_mhz'], res['cus'] = clock_hz / 1e6, cus
    res['lookups_per_s'] = nq * float(n) * a.M / t_scan
    res['lds_b128_lookups_per_s'] = 64.0 * cus * clock_hz            # 256 B / clk / CU, 4 bytes per lookup
    res['scan_fraction_of_lds_rate'] = res['lookups_per_s'] / res['lds_b128_lookups_per_s']
    res['pq_search_over_exact_search'] = res['ms']['pq_search'][0] / res['ms']['exact_search'][0]
    approx = engine.pq_search(qf, index, k)[1]
    exact = engine.search(qf, gf, k)[1]
    res['recall'] = dict(zip(('1', '10', '100'), engine.topk_recall(approx, exact, (1, 10, 100))))
    res['rank1_pid_agreement'] = float(np.mean(pids[approx[:, 0].cpu().numpy()] == pids[exact[:, 0].cpu().numpy()]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='both', choices=('mars', 'large', 'both'))
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
        print(json.dumps(out['shapes'][-1]), flush=True)
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
