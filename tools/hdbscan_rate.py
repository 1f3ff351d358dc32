#!/usr/bin/env python
"""Times engine.hdbscan at the MARS shape (13290 samples x 6144: the query-prepended gallery) on unit-norm synthetic rows
with planted identities (the input of tools/silhouette_rate.py).  Split into its parts: one bare pass over the
``_ColumnBlocks`` of cosin_dist(x, x) (the GEMM floor: code that existed before), the core-distance pass, the forest
(its rounds and the time per round), grl_hdbscan_minedge_block alone on the materialised matrix (every distance read
once: the achieved GB/s over n^2 x 4 bytes is reported) for the first round -- every sample a component of its own, no
column skipped -- and for the last round's components, and the host cut.  One process, the functions in turn: 15
warm-ups, then 20 timed runs each (HIP events; the discipline of tools/verify_rate.py), medians.  ``--host 1`` adds the
off-the-shelf route for comparison: download the float32 matrix, scikit-learn's HDBSCAN(metric='precomputed') on its
float64 copy (one run, wall clock).

  python tools/hdbscan_rate.py [--warm 15] [--reps 20] [--n 13290] [--mcs 5] [--ms 5] [--host 0] [--json PATH]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warm', type=int, default=15)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--n', type=int, default=13290)
    ap.add_argument('--mcs', type=int, default=5)
    ap.add_argument('--ms', type=int, default=5)
    ap.add_argument('--host', type=int, default=0)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    from grl_amd import engine
    from grl_amd._lib import ptr
    from grl_amd.synthetic import synth_eval_features
    dev = torch.device('cuda:0')
    n, nq = a.n, min(1980, a.n)
    qf, gf, qp, qc, gp, gc = synth_eval_features(nq, n, seed=1)
    gf = (gf * (1.0 / float(np.sqrt(3.0)))).to(dev)        # three unit blocks per row -> unit rows
    hd = engine.hdbscan(gf, a.mcs, a.ms)
    res = {'n': n, 'd': gf.shape[1], 'warm': a.warm, 'reps': a.reps, 'device': torch.cuda.get_device_name(0),
           'min_cluster_size': a.mcs, 'min_samples': a.ms, 'rounds': hd.rounds, 'n_dropped': hd.n_dropped,
           'n_edges': int(hd.mst[0].numel()), 'n_clusters': hd.n_clusters, 'n_noise': hd.n_noise,
           'pair_scores': hd.pair_scores(gp)}
    blocks = engine._ColumnBlocks(gf, gf, 'cosine')
    res['blocks'] = len(blocks.spans)
    sq, rinv = torch.empty(n, device=dev), torch.empty(n, device=dev)
    engine._call('grl_row_sqnorm', ptr(gf), ptr(sq), n, gf.shape[1], gf.shape[1])
    engine._call('grl_silhouette_rinv', ptr(sq), n, ptr(rinv))

    def block_pass():
        for c0, c1 in blocks.spans:
            blocks.block(c0, c1)
    fns = {'block_pass': block_pass,
           'hdbscan': lambda: engine.hdbscan(gf, a.mcs, a.ms),
           'forest': lambda: engine.mutual_reachability_mst(gf, a.ms),
           'core_pass': lambda: engine._hdbscan_core_dist(blocks, n, a.ms, rinv)}
    res['ms'] = in_turn(fns, a.warm, a.reps)
    floor = res['ms']['block_pass'][0]
    res['round_ms'] = (res['ms']['forest'][0] - res['ms']['core_pass'][0]) / max(hd.rounds, 1)
    res['round_over_floor'] = res['round_ms'] / floor
    res['total_over_floor_passes'] = res['ms']['hdbscan'][0] / ((1 + hd.rounds) * floor)
    # the block kernel on its own, on the materialised matrix (one block: every entry read once)
    D = engine.cosin_dist(gf, gf)
    core = hd.core_dist
    best_w = torch.empty(n, dtype=torch.float32, device=dev)
    best_j = torch.empty(n, dtype=torch.int32, device=dev)
    first = torch.arange(n, dtype=torch.int32, device=dev)
    last = torch.where(hd.labels >= 0, hd.labels, hd.labels.max() + 1 + torch.arange(n, device=dev)).to(torch.int32)
    kern = {}
    for name, comp in (('first_round', first), ('last_round', last)):
        kern['minedge/' + name] = (lambda comp=comp: engine._call(
            'grl_hdbscan_minedge_block', ptr(D), n, n, n, 0, 0, n, ptr(core), ptr(comp), ptr(rinv), ptr(best_w),
            ptr(best_j)))
    res['kernel_ms'] = in_turn(kern, a.warm, a.reps)
    res['minedge_gbps'] = {k: n * n * 4 / (v[0] * 1e-3) / 1e9 for k, v in res['kernel_ms'].items()}
    res['minedge_over_floor'] = {k: v[0] / floor for k, v in res['kernel_ms'].items()}
    # the host cut, wall clock
    lo, hi, w = (t.cpu().numpy() for t in hd.mst)
    cut = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        engine._hdbscan_cut(lo.tolist(), hi.tolist(), w.astype(np.float64), n, a.mcs, 'eom')
        cut.append((time.perf_counter() - t0) * 1e3)
    res['cut_ms'] = (float(np.median(cut)), float(min(cut)), float(max(cut)))
    if a.host:
        from sklearn.cluster import HDBSCAN
        t0 = time.perf_counter()
        engine._call('grl_hdbscan_cosine_block', ptr(D), n, n, n, 0, 0, n, ptr(rinv))
        d64 = D.cpu().numpy().astype(np.float64)
        t1 = time.perf_counter()
        np.fill_diagonal(d64, 0.0)
        sk = HDBSCAN(min_cluster_size=a.mcs, min_samples=a.ms, metric='precomputed', allow_single_cluster=False).fit(d64)
        t2 = time.perf_counter()
        lab = hd.labels.cpu().numpy()
        res['host'] = {'download_ms': (t1 - t0) * 1e3, 'sklearn_ms': (t2 - t1) * 1e3,
                       'n_clusters': int(sk.labels_.max()) + 1, 'n_noise': int((sk.labels_ < 0).sum()),
                       'labels_differ': int(((lab < 0) != (sk.labels_ < 0)).sum())}
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
