#!/usr/bin/env python
"""Times engine.search and engine.rank_metrics_streaming at the MARS shape (1980 queries x 11310 gallery rows x 6144)
under metric='cosine' and under the verification-head metric (engine.verify_metric) with beta = 1 and beta = 0.35, in
one process, the three metrics in turn: 15 warm-ups, then 20 timed launches each (HIP events; the discipline of
tools/distmat_gap.py).  Also the three small kernels of verify.hip on their own: the fold, the row terms of the queries
and of the gallery, and the finish pass over the whole 1980 x 11310 matrix with its bytes (nq * ng * 8: one read and
one write of every entry) over its time.

  python tools/verify_rate.py [--warm 15] [--reps 20] [--k 100] [--json PATH]

Under ``rocprofv3 --kernel-trace --stats -- python tools/verify_rate.py --warm 2 --reps 3`` the per-kernel table gives
the finish kernel's own duration (verify_finish_kernel), which is the bandwidth DESIGN.md 4q / EXPERIMENTS.md quote.
"""
import argparse
import contextlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def in_turn(fns, warm, reps):
    """{name: (median, min, max) ms}: warm every function, then time them in turn, reps rounds."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(event_ms(fn))
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warm', type=int, default=15)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--k', type=int, default=100)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    from grl_amd import engine
    from grl_amd._lib import ptr
    from grl_amd.reid import models
    from grl_amd.synthetic import synth_eval_features, synth_state_dict
    dev = torch.device('cuda:0')
    nq, ng = 1980, 11310
    qf, gf, qp, qc, gp, gc = synth_eval_features(nq, ng, seed=1)
    qf, gf = qf.to(dev), gf.to(dev)
    siam = models.create('siamese', input_num=2048, output_num=512, class_num=2)
    siam.load_state_dict(synth_state_dict(siam, seed=0, prefix='siamese.'))
    siam.to(dev).eval()
    metrics = {'cosine': 'cosine', 'verify_b1': engine.verify_metric(siam, 2048, 1.0),
               'verify_b035': engine.verify_metric(siam, 2048, 0.35)}
    res = {'nq': nq, 'ng': ng, 'd': qf.shape[1], 'k': a.k, 'warm': a.warm, 'reps': a.reps,
           'device': torch.cuda.get_device_name(0)}

    def quiet(fn):
        def f():
            with contextlib.redirect_stdout(io.StringIO()):
                return fn()
        return f
    res['search_ms'] = in_turn({n: (lambda m=m: engine.search(qf, gf, a.k, metric=m)) for n, m in metrics.items()},
                               a.warm, a.reps)
    res['rank_metrics_streaming_ms'] = in_turn(
        {n: quiet(lambda m=m: engine.rank_metrics_streaming(qf, gf, qp, gp, qc, gc, metric=m))
         for n, m in metrics.items()}, a.warm, a.reps)
    res['distmat_ms'] = in_turn({'cosine': lambda: engine.cosin_dist(qf, gf),
                                 'verify_b1': lambda: engine.verify_dist(qf, gf, metrics['verify_b1']),
                                 'verify_b035': lambda: engine.verify_dist(qf, gf, metrics['verify_b035'])},
                                a.warm, a.reps)
    # the kernels of verify.hip on their own
    vm = metrics['verify_b035']
    w, c64, _ = vm.folded()
    D = engine.cosin_dist(qf, gf)
    rq = torch.zeros(nq, device=dev)
    rg = torch.zeros(ng, device=dev)
    qv = torch.empty_like(qf)
    qs = torch.empty((nq, 2048), device=dev)
    import ctypes as C
    b035, b1 = C.byref(C.c_double(0.35)), C.byref(C.c_double(1.0))
    parts = in_turn({
        'fold': lambda: engine.VerifyFoldPlan(siam),
        'rows_query_full': lambda: engine._call('grl_verify_rows', ptr(qf), 6144, nq, 6144, 2048, 2048, ptr(w), b035,
                                                ptr(c64), ptr(rq), ptr(qv), 6144, 1),
        'rows_query_slice': lambda: engine._call('grl_verify_rows', ptr(qf), 6144, nq, 6144, 2048, 2048, ptr(w), b1,
                                                 ptr(c64), ptr(rq), ptr(qs), 2048, 0),
        'rows_gallery': lambda: engine._call('grl_verify_rows', ptr(gf), 6144, ng, 6144, 2048, 2048, ptr(w), b035, None,
                                             ptr(rg), None, 0, 0),
        'finish': lambda: engine._call('grl_verify_finish', ptr(D), ng, nq, ng, ptr(rq), ptr(rg), 0),
    }, a.warm, a.reps)
    res['kernels_ms'] = parts
    res['finish_bytes'] = nq * ng * 8
    res['finish_gbps'] = nq * ng * 8 / (parts['finish'][0] * 1e-3) / 1e9
    for key in ('search_ms', 'rank_metrics_streaming_ms', 'distmat_ms'):
        cos = res[key]['cosine'][0]
        res[key + '_over_cosine'] = {n: res[key][n][0] / cos for n in res[key]}
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
