#!/usr/bin/env python
"""Times engine.silhouette at the MARS shape (13290 samples x 6144: the query-prepended gallery) on unit-norm synthetic
rows with planted identities, next to engine.cluster on the same input (eps at that input's ``PairRoc.eer_threshold``):
the labels scored are that clustering's.  Split into its parts: one bare pass over the ``_ColumnBlocks`` of
cosin_dist(x, x) (the GEMM floor: code that existed before), the member lists, the block kernel alone on the
materialised matrix (every distance read once: the achieved GB/s over n^2 x 4 bytes is reported) for the clustering's
labels and for the two extremes of the cluster loop -- two clusters, and every sample a cluster of its own --, the
matrix form, and the score.  One process, the functions in turn: 15 warm-ups, then 20 timed launches each (HIP events;
the discipline of tools/verify_rate.py).

  python tools/silhouette_rate.py [--warm 15] [--reps 20] [--n 13290] [--json PATH]
"""
import argparse
import json
import os
import sys

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
    eps = float(engine.pair_roc(qf, gf, qp, gp, qc, gc).eer_threshold)
    cl = engine.cluster(gf, eps)
    res = {'n': n, 'd': gf.shape[1], 'warm': a.warm, 'reps': a.reps, 'device': torch.cuda.get_device_name(0),
           'eps': eps, 'n_clusters': cl.n_clusters, 'n_noise': cl.n_noise}
    blocks = engine._ColumnBlocks(gf, gf, 'cosine')
    res['blocks'] = len(blocks.spans)

    def block_pass():
        for c0, c1 in blocks.spans:
            blocks.block(c0, c1)
    fns = {'block_pass': block_pass,
           'cluster': lambda: engine.cluster(gf, eps),
           'silhouette/cosine': lambda: engine.silhouette(gf, cl.labels, 'cosine'),
           'silhouette/euclidean': lambda: engine.silhouette(gf, cl.labels, 'euclidean'),
           'member_lists': lambda: engine._silhouette_labels(cl.labels, n, 'singleton', 'silhouette_rate')}
    res['ms'] = in_turn(fns, a.warm, a.reps)
    res['non_gemm_ms'] = res['ms']['silhouette/cosine'][0] - res['ms']['block_pass'][0]
    r = engine.silhouette(gf, cl.labels, 'cosine')
    res['score'] = {'cosine': r.score, 'euclidean': engine.silhouette(gf, cl.labels, 'euclidean').score,
                    'n_scored': r.n_scored, 'pair_scores': cl.pair_scores(gp)}
    # the block kernel on its own, on the materialised matrix in member order (one block: every entry read once)
    D = engine.cosin_dist(gf, gf)
    part = torch.empty((n, 64), dtype=torch.float32, device=dev)
    av = torch.empty(n, dtype=torch.float32, device=dev)
    bv = torch.empty(n, dtype=torch.float32, device=dev)
    kern = {}
    for name, labels in (('clusters', cl.labels), ('two', (torch.arange(n, device=dev) % 2)),
                         ('singletons', torch.arange(n, device=dev))):
        lab32, counts, mptr, mem, k, m, _ = engine._silhouette_labels(labels, n, 'singleton', 'silhouette_rate')
        Dm = D[:, mem.to(torch.int64)].contiguous()
        kern['block/' + name] = (lambda Dm=Dm, lab32=lab32, mptr=mptr, mem=mem, k=k: engine._call(
            'grl_silhouette_block', ptr(Dm), n, n, 0, 0, n, ptr(mem), ptr(mptr), k, ptr(lab32), None, None, ptr(part),
            ptr(av), ptr(bv)))
    kern['matrix_form'] = lambda: engine.silhouette_matrix(D, cl.labels)
    res['kernel_ms'] = in_turn(kern, a.warm, a.reps)
    res['block_gbps'] = {k: n * n * 4 / (v[0] * 1e-3) / 1e9 for k, v in res['kernel_ms'].items() if k.startswith('block/')}
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
