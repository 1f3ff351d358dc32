#!/usr/bin/env python
"""Times the cluster-memory update and one labelling pass of unsupervised training.

* grl_cmem_update (hard and mean) against grl_oim_update, the per-sample rule, on the same inputs: D = 2048, K = 625 unit
  rows, n = 128 (clip level: 64 clusters x 2 rows) and n = 512 (frame level: 64 clusters x 8 rows).  A launch is a few
  microseconds, so a timed window is ``--batch`` launches between two HIP events; reported per launch.
* pseudo_labels (method 'jaccard', the default arguments) on 8298 x 6144 unit rows with planted identities -- the MARS
  training set's tracklet count -- and the seeding of the two memories from its labels (PseudoLabels.centroids on the two
  2048-column slices).

One process, the functions in turn: warm-ups, then the median of the timed windows (the discipline of tools/verify_rate.py).
Nothing here is a threshold.

  python tools/cmem_rate.py [--warm 15] [--reps 20] [--batch 50] [--n-label 8298] [--json PATH]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from verify_rate import in_turn  # noqa: E402

D, K, IDS = 2048, 625, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warm', type=int, default=15)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=50)
    ap.add_argument('--n-label', type=int, default=8298)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    from grl_amd import engine
    from grl_amd._lib import ptr
    from grl_amd.reid.train.pseudo import pseudo_labels
    from grl_amd.synthetic import synth_eval_features
    dev = torch.device('cuda:0')
    res = {'D': D, 'K': K, 'warm': a.warm, 'reps': a.reps, 'batch': a.batch, 'device': torch.cuda.get_device_name(0)}
    g = torch.Generator().manual_seed(0)
    unit = torch.nn.functional.normalize
    fns = {}
    keep = []
    for n in (128, 512):
        x = unit(torch.randn((n, D), generator=g), dim=1).to(dev)
        y = torch.randperm(K, generator=g)[:IDS].repeat_interleave(n // IDS).to(dev)
        for name, mode in (('oim_update', None), ('cmem_update/hard', 0), ('cmem_update/mean', 1)):
            cent = unit(torch.randn((K, D), generator=torch.Generator().manual_seed(1)), dim=1).to(dev)
            keep.append((x, y, cent))

            def launch(x=x, y=y, cent=cent, n=n, mode=mode):
                for _ in range(a.batch):
                    if mode is None:
                        engine._call('grl_oim_update', ptr(cent), ptr(x), ptr(y), n, D, K, C.c_float(0.2))
                    else:
                        engine._call('grl_cmem_update', ptr(cent), ptr(x), ptr(y), n, D, K, C.c_float(0.2), mode, None)
            fns['%s/n%d' % (name, n)] = launch
    ms = in_turn(fns, a.warm, a.reps)
    res['us_per_launch'] = {k: tuple(1e3 * v / a.batch for v in t) for k, t in ms.items()}
    for x, y, cent in keep:
        assert bool(torch.isfinite(cent).all())

    n = a.n_label
    _, gf, _, _, gp, _ = synth_eval_features(0, n, seed=1)
    gf = (gf * (1.0 / float(np.sqrt(3.0)))).to(dev)                      # three unit blocks per row -> unit rows
    labels = pseudo_labels(gf)
    res['labelling'] = {'n': n, 'd': gf.shape[1], 'method': 'jaccard', 'n_clusters': labels.n_clusters, 'n_noise': labels.n_noise,
                        'pair_scores': labels.pair_scores(gp)}
    res['labelling']['ms'] = in_turn({
        'pseudo_labels': lambda: pseudo_labels(gf),
        'seed_two_memories': lambda: (labels.centroids(gf, cols=(0, 2048)), labels.centroids(gf, cols=(2048, 4096))),
    }, max(1, a.warm // 5), max(3, a.reps // 4))
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
