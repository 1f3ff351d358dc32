#!/usr/bin/env python
"""Times engine.cluster at the MARS shape (13290 samples x 6144: the query-prepended gallery) on unit-norm synthetic
rows with planted identities, eps at that input's ``PairRoc.eer_threshold``, min_samples 1 and 4, against the GEMM
floor: the two bare passes over the ``_ColumnBlocks`` of cosin_dist(x, x) that eps_graph cannot avoid (code that
existed before the clustering).  Also eps_graph alone, cluster_from_graph alone on the finished graph, the edge kernel
alone (count and fill) on the materialised matrix, the component rounds, E and the pair scores.  One process, the
functions in turn: 15 warm-ups, then 20 timed launches each (HIP events; the discipline of tools/verify_rate.py).

With ``--host 1`` the host route is timed once for comparison: download of cosin_dist(x, x) (n^2 floats) plus
sklearn's DBSCAN(metric='precomputed') on it (shifted by +1: sklearn refuses negative distances), and its labels are
compared with the device's.

  python tools/cluster_rate.py [--warm 15] [--reps 20] [--host 0] [--n 13290] [--json PATH]
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
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    from grl_amd import engine
    from grl_amd._lib import ptr
    from grl_amd.synthetic import synth_eval_features
    dev = torch.device('cuda:0')
    n, nq = a.n, min(1980, a.n)
    qf, gf, qp, qc, gp, gc = synth_eval_features(nq, n, seed=1)
    scale = 1.0 / float(np.sqrt(3.0))                      # three unit blocks per row -> unit rows
    qf, gf = (qf * scale).to(dev), (gf * scale).to(dev)
    roc = engine.pair_roc(qf, gf, qp, gp, qc, gc)
    eps = float(roc.eer_threshold)
    res = {'n': n, 'd': gf.shape[1], 'warm': a.warm, 'reps': a.reps, 'device': torch.cuda.get_device_name(0),
           'eps': eps, 'eer': roc.eer}
    blocks = engine._ColumnBlocks(gf, gf, 'cosine')
    res['blocks'] = len(blocks.spans)

    def two_passes():
        for _ in range(2):
            for c0, c1 in blocks.spans:
                blocks.block(c0, c1)
    row_ptr, col = engine.eps_graph(gf, eps)
    fns = {'two_block_passes': two_passes, 'eps_graph': lambda: engine.eps_graph(gf, eps)}
    for m in (1, 4):
        fns['cluster/m%d' % m] = lambda m=m: engine.cluster(gf, eps, m)
        fns['cluster_from_graph/m%d' % m] = lambda m=m: engine.cluster_from_graph(row_ptr, col, n, m, _checked=True)
    res['ms'] = in_turn(fns, a.warm, a.reps)
    res['non_gemm_ms'] = {k: res['ms'][k][0] - res['ms']['two_block_passes'][0] for k in ('cluster/m1', 'cluster/m4')}
    # the edge kernel on its own, on the materialised matrix (every entry read once per pass)
    D = engine.cosin_dist(gf, gf)
    cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    col2 = torch.empty_like(col)

    def count():
        engine._call('grl_cluster_edges_block', ptr(D), n, n, 0, 0, n, eps, ptr(cnt), None, None)

    def fill():
        cnt.zero_()
        engine._call('grl_cluster_edges_block', ptr(D), n, n, 0, 0, n, eps, ptr(cnt), ptr(row_ptr), ptr(col2))
    res['kernel_ms'] = in_turn({'count': count, 'fill': fill}, a.warm, a.reps)
    res['kernel_gbps'] = {k: n * n * 4 / (v[0] * 1e-3) / 1e9 for k, v in res['kernel_ms'].items()}
    assert torch.equal(col2, col)
    for m in (1, 4):
        cl = engine.cluster(gf, eps, m)
        res['result/m%d' % m] = {'n_clusters': cl.n_clusters, 'n_noise': cl.n_noise, 'n_edges': cl.n_edges,
                                 'rounds': cl.rounds, 'pair_scores': cl.pair_scores(gp)}
    if a.host:
        from sklearn.cluster import DBSCAN
        host = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        H = engine.cosin_dist(gf, gf).cpu().numpy()
        host['download_s'] = time.perf_counter() - t0
        H += 1.0
        np.maximum(H, 0.0, out=H)
        for m in (1, 4):
            t0 = time.perf_counter()
            sk = DBSCAN(eps=eps + 1.0, min_samples=m, metric='precomputed').fit(H)
            host['dbscan_s/m%d' % m] = time.perf_counter() - t0
            host['labels_equal/m%d' % m] = bool(np.array_equal(sk.labels_, engine.cluster(gf, eps, m).labels.cpu().numpy()))
        res['host'] = host
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
