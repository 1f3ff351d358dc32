#!/usr/bin/env python
"""Times grl_expand_rows (engine.expand_from_lists) against the torch formulation of the same arithmetic
(``bank[idx]`` gather, multiply by the weights, sum over m, divide), in one process, alternating the two, with
warm-ups and HIP events; also the peak device memory of each above the inputs, and the whole expand_features call
(search + expansion).  Shapes: database-side augmentation and query expansion at the MARS size.

  python tools/expand_rate.py [--reps N] [--m M] [--alpha A] [--json PATH]

Bytes the kernel has to move per call (the algorithm's, from the shapes): n * (m + 1) * d * 4 read (x and m bank
rows per row), n * d * 4 written, n * L * 12 of lists.  GB/s = those bytes over the median time.
"""
import argparse
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


def alternate(fns, reps, warm=3):
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


def peak_over_inputs(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def torch_expand(xf, bank, dist, idx, alpha):
    """The same mean in torch ops (lists without padding or self entries): materialises the n x m x d gather."""
    w = torch.ones_like(dist) if alpha == 0 else (-dist).clamp_min(0) ** alpha
    acc = xf + (bank[idx] * w.unsqueeze(2)).sum(1)
    return acc / (1.0 + w.sum(1, keepdim=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--m', type=int, default=10)
    ap.add_argument('--alpha', type=int, default=3)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    from grl_amd import engine
    from grl_amd.synthetic import synth_eval_features
    dev = torch.device('cuda:0')
    qf, gf, qp, qc, gp, gc = synth_eval_features(1980, 13290, seed=1)
    qf, gf = qf.to(dev), gf.to(dev)
    ids = (qp, gp, qc, gc)
    m, alpha = a.m, a.alpha
    res = {'m': m, 'alpha': alpha, 'reps': a.reps, 'device': torch.cuda.get_device_name(0)}
    cases = {
        'dba_13290': (gf, gf, dict(skip_self=True)),
        'qe_1980': (qf, gf, dict(exclude=ids)),
    }
    for name, (xf, bank, kw) in cases.items():
        n, d = xf.shape
        skip = bool(kw.get('skip_self'))
        dist, idx = engine.search(xf, bank, m + (1 if skip else 0), exclude=kw.get('exclude'))
        if skip:                      # the torch formulation gets the lists with the self entry already removed
            keep = idx != torch.arange(n, device=dev).unsqueeze(1)
            assert bool((keep.sum(1) == m).all())
            t_idx, t_dist = idx[keep].view(n, m), dist[keep].view(n, m)
        else:
            t_idx, t_dist = idx, dist
        assert bool((t_idx >= 0).all())
        ours = engine.expand_from_lists(xf, bank, dist, idx, m, alpha, skip)
        theirs = torch_expand(xf, bank, t_dist, t_idx, alpha)
        r = {'n': n, 'd': d, 'max_abs_diff_vs_torch': float((ours - theirs).abs().max())}
        del ours, theirs
        t = alternate({'kernel': lambda: engine.expand_from_lists(xf, bank, dist, idx, m, alpha, skip),
                       'torch': lambda: torch_expand(xf, bank, t_dist, t_idx, alpha)}, a.reps)
        moved = n * (m + 1) * d * 4 + n * d * 4 + n * idx.shape[1] * 12
        r['kernel_ms'], r['torch_ms'] = t['kernel'], t['torch']
        r['kernel_bytes'] = moved
        r['kernel_gbps'] = moved / (t['kernel'][0] * 1e-3) / 1e9
        r['torch_over_kernel'] = t['torch'][0] / t['kernel'][0]
        r['kernel_peak_bytes'] = peak_over_inputs(lambda: engine.expand_from_lists(xf, bank, dist, idx, m, alpha, skip))
        r['torch_peak_bytes'] = peak_over_inputs(lambda: torch_expand(xf, bank, t_dist, t_idx, alpha))
        r['gather_bytes'] = n * m * d * 4
        full = alternate({'expand_features': lambda: engine.expand_features(xf, bank, m, alpha, **kw)}, a.reps, warm=2)
        r['expand_features_ms'] = full['expand_features']
        r['expand_features_peak_bytes'] = peak_over_inputs(lambda: engine.expand_features(xf, bank, m, alpha, **kw))
        res[name] = r
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
