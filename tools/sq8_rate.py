#!/usr/bin/env python
"""Times the int8 scalar-quantised index (engine.sq8_train / sq8_index / sq8_search, sq8.hip) next to exact
search and to the binary-code index, on tools/pq_rate.py's data recipe: synthetic unit rows with planted identities made
on the device, the queries the first rows of the gallery, at the MARS shape (1980 x 11310 x 6144) and a large gallery
(1980 x 2^18 x 6144).

Per shape, one process (run the tool once per --shape), the functions in turn, 15 warm-ups then 20 timed launches each
(HIP events; the discipline of tools/verify_rate.py), medians:
  sq8_scan        grl_sq8_scan over all column blocks (the query codes already there)
  sq8_scan_i32    grl_sq8_scan_i32 over the same blocks: the raw sums, no float epilogue
  sq8_query       the query side: quantise + bias GEMM + norms (Sq8Codebook.query)
  sq8_search      engine.sq8_search(qf, index, 100): query + scan + top-k
  sq8_refine      engine.sq8_refine_search(qf, index, store, 100, 100) with a bf16 store
  bin_search      engine.bin_search(qf, bin_index, 100, 'hamming') (256 bits; LSH by default: the time does not depend on
                  how the hyperplanes were trained)
  exact_search    engine.search(qf, gf, 100) on the raw features
and, once each: the train and encode wall times, recall@10 of each search against exact search, the index bytes, and the
integer rate of sq8_scan (2 * nq * n * dpad operations over its time) as a fraction of --peak-tops.

  python tools/sq8_rate.py --shape mars|large [--warm 15] [--reps 20] [--nbits 256] [--bin-method lsh] [--train-rows 65536]
                           [--noise 1.0] [--peak-tops 5000] [--json PATH]
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
    from grl_amd._lib import ptr
    nq, n = SHAPES[name]
    d, k = 6144, 100
    gf, _ = planted_rows(n, d, max(2, n // 18), a.noise, 1, dev)
    qf = gf[:nq].contiguous()
    res = {'shape': name, 'nq': nq, 'n': n, 'd': d, 'k': k, 'noise': a.noise, 'nbits': a.nbits, 'bin_method': a.bin_method}
    t_rows = min(n, a.train_rows)
    res['train_rows'] = t_rows
    book, res['sq8_train_s'] = wall(lambda: engine.sq8_train(gf[:t_rows]))
    index, res['sq8_encode_s'] = wall(lambda: engine.sq8_index(gf, book))
    store = engine.RefineStore(gf, 'bf16')
    bin_book = engine.bin_train(gf[:t_rows], a.nbits, a.bin_method, 50, 0)
    bin_index = engine.bin_index(gf, bin_book)
    res['sq8_index_bytes'], res['bin_index_bytes'], res['feature_bytes'] = int(index.nbytes), int(bin_index.nbytes), 4 * n * d
    res['store_bytes'] = int(store.nbytes)
    blocks = engine._Sq8Blocks(qf, index)
    res['blocks'], res['block_cols'] = len(blocks.spans), blocks.width
    dpad = book.dpad
    raw = torch.empty((nq, blocks.width), dtype=torch.int32, device=dev)

    def scan():
        for c0, c1 in blocks.spans:
            blocks.block(c0, c1)

    def scan_i32():
        for c0, c1 in blocks.spans:
            engine._call('grl_sq8_scan_i32', ptr(blocks.qcodes), dpad, ptr(index.codes[c0:c1]), dpad, ptr(raw), c1 - c0, nq,
                         c1 - c0, dpad)
    fns = {'sq8_scan': scan, 'sq8_scan_i32': scan_i32, 'sq8_query': lambda: book.query(qf),
           'sq8_search': lambda: engine.sq8_search(qf, index, k),
           'sq8_refine': lambda: engine.sq8_refine_search(qf, index, store, k, k),
           'bin_search': lambda: engine.bin_search(qf, bin_index, k, 'hamming'),
           'exact_search': lambda: engine.search(qf, gf, k)}
    res['ms'] = in_turn(fns, a.warm, a.reps)
    ms = {key: v[0] for key, v in res['ms'].items()}
    res['sq8_search_over_exact_search'] = ms['sq8_search'] / ms['exact_search']
    res['sq8_search_over_bin_search'] = ms['sq8_search'] / ms['bin_search']
    t = ms['sq8_scan'] * 1e-3
    res['sq8_scan_tops'] = 2.0 * nq * n * dpad / t / 1e12
    res['sq8_scan_i32_tops'] = 2.0 * nq * n * dpad / (ms['sq8_scan_i32'] * 1e-3) / 1e12
    res['peak_tops'] = a.peak_tops
    res['sq8_scan_fraction_of_peak'] = res['sq8_scan_tops'] / a.peak_tops
    res['sq8_scan_out_gb_per_s'] = 4.0 * nq * n / t / 1e9
    exact = engine.search(qf, gf, k)[1]
    res['recall_at_10'] = {
        'sq8_search': engine.topk_recall(engine.sq8_search(qf, index, k)[1], exact, (10,))[0],
        'sq8_refine': engine.topk_recall(engine.sq8_refine_search(qf, index, store, k, k)[1], exact, (10,))[0],
        'bin_search': engine.topk_recall(engine.bin_search(qf, bin_index, k, 'hamming')[1], exact, (10,))[0],
        'exact_search': 1.0}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', required=True, choices=('mars', 'large'))
    ap.add_argument('--warm', type=int, default=15)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--nbits', type=int, default=256)
    ap.add_argument('--bin-method', default='lsh', choices=('itq', 'lsh'))
    ap.add_argument('--train-rows', type=int, default=65536)
    ap.add_argument('--noise', type=float, default=1.0)
    ap.add_argument('--peak-tops', type=float, default=5000.0, help='dense int8 MFMA peak of the device in TOP/s')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {'device': torch.cuda.get_device_name(0), 'warm': a.warm, 'reps': a.reps}
    out.update(measure(a.shape, a, dev))
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
