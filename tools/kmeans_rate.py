#!/usr/bin/env python
"""Times one iteration of engine.kmeans at the MARS shape (13290 samples x 6144: the query-prepended gallery, k = 625)
on unit-norm synthetic rows with planted identities, split into its parts: the bare pass over the ``_ColumnBlocks`` of
cosin_dist(x, C) (the GEMM floor: code that existed before k-means), top-1 + relabel on the finished blocks' lists,
the member lists, grl_segment_rowsum alone and the whole update; then the full run (spherical k-means from random
rows).  For the row-sum kernel the achieved GB/s over (n d + k d) 4 bytes is reported: each assigned row is read once,
k x d is written.  One process, the functions in turn: 15 warm-ups, then 20 timed launches each (HIP events; the
discipline of tools/verify_rate.py).

With ``--host 1`` the host route is timed once for comparison: download of the features plus scikit-learn's
KMeans(init=the same rows, n_init=1, algorithm='lloyd') on the unit rows (Euclidean Lloyd: on unit rows its assignment
is the cosine one, its centroids are not re-normalised), with the pair scores of both.

  python tools/kmeans_rate.py [--warm 15] [--reps 20] [--host 0] [--n 13290] [--k 625] [--max-iter 50] [--json PATH]
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
    ap.add_argument('--host', type=int, default=0)
    ap.add_argument('--n', type=int, default=13290)
    ap.add_argument('--k', type=int, default=625)
    ap.add_argument('--max-iter', type=int, default=50)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    from grl_amd import engine
    from grl_amd._lib import ptr
    from grl_amd.synthetic import synth_eval_features
    dev = torch.device('cuda:0')
    n, k = a.n, a.k
    _, gf, _, _, gp, _ = synth_eval_features(min(1980, n), n, seed=1)
    gf = (gf * (1.0 / float(np.sqrt(3.0)))).to(dev)        # three unit blocks per row -> unit rows
    d = gf.shape[1]
    res = {'n': n, 'd': d, 'k': k, 'warm': a.warm, 'reps': a.reps, 'device': torch.cuda.get_device_name(0),
           'n_ids': int(np.unique(gp).size)}
    seed_rows = np.random.Generator(np.random.PCG64(0)).choice(n, k, replace=False)
    cent = gf[torch.from_numpy(seed_rows).to(dev)].contiguous()
    blocks = engine._ColumnBlocks(gf, cent, 'cosine')
    res['blocks'] = len(blocks.spans)

    def block_pass():
        for c0, c1 in blocks.spans:
            blocks.block(c0, c1)
    run_key, run_val = engine._kmeans_top1(gf, cent, 'cosine', None, None)
    labels, counts, _ = engine._kmeans_relabel(run_key, run_val, k)
    mptr = torch.empty(k + 1, dtype=torch.int64, device=dev)
    cursor = torch.zeros(k, dtype=torch.int32, device=dev)
    tmp = torch.empty(n, dtype=torch.int32, device=dev)
    mem = torch.empty(n, dtype=torch.int32, device=dev)
    total = torch.zeros((k, d), dtype=torch.float32, device=dev)

    def member_lists():
        engine._call('grl_rrs_scan', ptr(counts), k, ptr(mptr))
        cursor.zero_()
        engine._call('grl_kmeans_members', ptr(labels), n, k, ptr(mptr), ptr(cursor), ptr(tmp), ptr(mem))

    def rowsum():
        engine._call('grl_segment_rowsum', ptr(gf), d, n, ptr(mptr), ptr(mem), n, k, d, ptr(total), d)
    member_lists()
    fns = {'block_pass': block_pass,
           'assign': lambda: engine._kmeans_top1(gf, cent, 'cosine', None, None),
           'relabel': lambda: engine._kmeans_relabel(run_key, run_val, k),
           'member_lists': member_lists,
           'segment_rowsum': rowsum,
           'update': lambda: engine._kmeans_update(gf, labels, counts, k, 'unit', cent),
           'kmeans/1_iteration': lambda: engine.kmeans(gf, k, init=cent, max_iter=1),
           'kmeans/full': lambda: engine.kmeans(gf, k, init=cent, max_iter=a.max_iter)}
    res['ms'] = in_turn(fns, a.warm, a.reps)
    res['rowsum_gbps'] = (n * d + k * d) * 4 / (res['ms']['segment_rowsum'][0] * 1e-3) / 1e9
    res['top1_ms'] = res['ms']['assign'][0] - res['ms']['block_pass'][0]
    # the kernel's sum against an index_add_ in float64 (the order differs; the values agree to fp32 rounding)
    ref = torch.zeros((k, d), dtype=torch.float64, device=dev).index_add_(0, labels.to(torch.int64), gf.double())
    res['rowsum_max_abs_err'] = float((total.double() - ref).abs().max())
    counts_h = counts.cpu().numpy()
    res['cluster_sizes'] = {'min': int(counts_h.min()), 'median': float(np.median(counts_h)), 'max': int(counts_h.max())}
    km = engine.kmeans(gf, k, init=cent, max_iter=a.max_iter)
    res['result'] = {'n_iter': km.n_iter, 'converged': km.converged, 'n_changed': km.n_changed, 'n_empty': km.n_empty,
                     'inertia': km.inertia, 'pair_scores': km.pair_scores(gp)}
    if a.host:
        from sklearn.cluster import KMeans
        host = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        H = gf.cpu().numpy()
        host['download_s'] = time.perf_counter() - t0
        t0 = time.perf_counter()
        sk = KMeans(n_clusters=k, init=H[seed_rows], n_init=1, algorithm='lloyd', max_iter=a.max_iter, tol=0.0).fit(H)
        host['kmeans_s'] = time.perf_counter() - t0
        host['n_iter'] = int(sk.n_iter_)
        host['pair_scores'] = engine._pair_scores(torch.from_numpy(sk.labels_.astype(np.int64)), k, gp)
        res['host'] = host
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
