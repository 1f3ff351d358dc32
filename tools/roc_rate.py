#!/usr/bin/env python
"""Times engine.pair_roc against engine.rank_metrics_streaming (the unchanged streaming CMC / mAP path, the yardstick)
at the MARS shape (1980 queries x 11310 gallery rows x 6144), under metric='cosine' and under the verification-head
metric with beta = 1, in one process, the functions in turn: 15 warm-ups, then 20 timed launches each (HIP events;
the discipline of tools/verify_rate.py).  Also the distance pass alone (cosin_dist / verify_dist) and the histogram
kernel alone on the materialised matrix, with its bytes (nq * ng * 4: every entry read once) over its time, for
bits = 16 and 20.

  python tools/roc_rate.py [--warm 15] [--reps 20] [--json PATH]

Under ``rocprofv3 --kernel-trace --stats -- python tools/roc_rate.py --warm 2 --reps 3`` the per-kernel table gives
pair_hist_kernel's own duration, which is the bandwidth DESIGN.md 4r / EXPERIMENTS.md quote.
"""
import argparse
import contextlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from verify_rate import in_turn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warm', type=int, default=15)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    from grl_amd import engine
    from grl_amd.reid import models
    from grl_amd.synthetic import synth_eval_features, synth_state_dict
    dev = torch.device('cuda:0')
    nq, ng = 1980, 11310
    qf, gf, qp, qc, gp, gc = synth_eval_features(nq, ng, seed=1)
    qf, gf = qf.to(dev), gf.to(dev)
    siam = models.create('siamese', input_num=2048, output_num=512, class_num=2)
    siam.load_state_dict(synth_state_dict(siam, seed=0, prefix='siamese.'))
    siam.to(dev).eval()
    metrics = {'cosine': 'cosine', 'verify_b1': engine.verify_metric(siam, 2048, 1.0)}
    ids = (qp, gp, qc, gc)
    res = {'nq': nq, 'ng': ng, 'd': qf.shape[1], 'warm': a.warm, 'reps': a.reps,
           'device': torch.cuda.get_device_name(0)}

    def quiet(fn):
        def f():
            with contextlib.redirect_stdout(io.StringIO()):
                return fn()
        return f
    fns = {}
    for n, m in metrics.items():
        fns['pair_roc/' + n] = lambda m=m: engine.pair_roc(qf, gf, *ids, metric=m)
        fns['rank_metrics_streaming/' + n] = quiet(lambda m=m: engine.rank_metrics_streaming(qf, gf, *ids, metric=m))
    fns['distmat/cosine'] = lambda: engine.cosin_dist(qf, gf)
    fns['distmat/verify_b1'] = lambda: engine.verify_dist(qf, gf, metrics['verify_b1'])
    res['ms'] = in_turn(fns, a.warm, a.reps)
    res['pair_roc_over_rank_metrics_streaming'] = {
        n: res['ms']['pair_roc/' + n][0] / res['ms']['rank_metrics_streaming/' + n][0] for n in metrics}
    # the histogram kernel on its own, on the materialised matrices
    mats = {'cosine': engine.cosin_dist(qf, gf), 'verify_b1': engine.verify_dist(qf, gf, metrics['verify_b1']).clone()}
    dids = tuple(engine._ids(x, n, 'ids', dev) for x, n in ((qp, nq), (qc, nq), (gp, ng), (gc, ng)))
    kern = {}
    for n, D in mats.items():
        for bits in (16, 20):
            hist = torch.zeros((2, 1 << bits), dtype=torch.int64, device=dev)
            kern['%s/bits%d' % (n, bits)] = lambda D=D, bits=bits, hist=hist: engine._pair_hist_block(
                D, 0, dids, bits, hist[0], hist[1])
    res['kernel_ms'] = in_turn(kern, a.warm, a.reps)
    res['kernel_bytes'] = nq * ng * 4
    res['kernel_gbps'] = {k: nq * ng * 4 / (v[0] * 1e-3) / 1e9 for k, v in res['kernel_ms'].items()}
    for n, m in metrics.items():
        roc = engine.pair_roc(qf, gf, *ids, metric=m)
        s = roc.summary()
        s['nonempty_bins'] = int(((roc.pos != 0) | (roc.neg != 0)).sum().item())
        res['figures/' + n] = s
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
