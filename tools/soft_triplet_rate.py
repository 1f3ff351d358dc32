#!/usr/bin/env python
"""Times the soft softmax-triplet kernels and the trainer step that carries them.

* grl_soft_triplet_fwd + grl_soft_triplet_bwd at w_soft = 0.8 against grl_triplet_fwd + grl_triplet_bwd (soft margin) on the
  same n x 2048 rows: n = 32, 64, 128, ids in pairs.  A pair of calls is a few microseconds, so a timed window is ``--batch``
  pairs between two HIP events; reported per pair, with the ratio soft / hard and the spread (max - min) of the windows.
* one 32 x 4 trainer step (forward + 5-term loss + backward + SGD + the teacher's update, bench.py's shapes), fp32 and bf16
  storage, under MeanTeacherSEQTrainer + SoftClusterMemoryLoss with (soft_weight, tri_soft_weight) = (0.5, 0) and (0.5, 0.8):
  the second swaps the hard triplet's two launches for the soft one's two and reads two more rows per anchor.

The yardsticks are the hard pair and the (0.5, 0) step, timed in the same run.  No threshold: the expectation that the soft
step stays within the spread of the windows is reported as ``within_spread``, not enforced.

One process, the variants alternating: warm-ups, then the median of the timed windows (the discipline of tools/verify_rate.py).

  python tools/soft_triplet_rate.py [--warm 15] [--reps 20] [--batch 50] [--steps 20] [--no-step] [--json PATH]
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
from teacher_rate import models_on, IDS  # noqa: E402

D = 2048
W = 0.8


def pair_times(a, dev):
    from grl_amd import engine
    from grl_amd._lib import ptr
    g = torch.Generator().manual_seed(0)
    fns, keep = {}, []
    for n in (32, 64, 128):
        f = torch.nn.functional.normalize(torch.randn((n, D), generator=g), dim=1).to(dev)
        tf = torch.nn.functional.normalize(torch.randn((n, D), generator=g), dim=1).to(dev)
        y = (torch.arange(n) // 2).to(dev)
        loss, z, q = (torch.empty(n, device=dev) for _ in range(3))
        dist, sel = torch.empty((n, n), device=dev), torch.empty((n, 2), dtype=torch.int32, device=dev)
        dl, df = torch.full((n,), 1.0 / n, device=dev), torch.empty_like(f)
        keep.append((f, tf, y, loss, z, q, dist, sel, dl, df))

        def soft(f=f, tf=tf, y=y, loss=loss, z=z, q=q, dist=dist, sel=sel, dl=dl, df=df, n=n):
            for _ in range(a.batch):
                engine._call('grl_soft_triplet_fwd', ptr(f), ptr(tf), ptr(y), n, D, C.c_float(W), ptr(loss), ptr(dist), ptr(sel),
                             ptr(z), ptr(q))
                engine._call('grl_soft_triplet_bwd', ptr(f), ptr(dist), ptr(sel), ptr(z), ptr(q), ptr(dl), C.c_float(W), ptr(df),
                             n, D)

        def hard(f=f, y=y, loss=loss, z=z, dist=dist, sel=sel, dl=dl, df=df, n=n):
            for _ in range(a.batch):
                engine._call('grl_triplet_fwd', ptr(f), ptr(y), n, D, 1, C.c_float(0.0), ptr(loss), ptr(dist), ptr(sel), ptr(z))
                engine._call('grl_triplet_bwd', ptr(f), ptr(dist), ptr(sel), ptr(z), ptr(dl), 1, C.c_float(0.0), ptr(df), n, D)
        fns['soft/n%d' % n] = soft
        fns['hard/n%d' % n] = hard
    ms = in_turn(fns, a.warm, a.reps)
    us = {k: tuple(1e3 * v / a.batch for v in t) for k, t in ms.items()}
    out = {'us_per_pair': us, 'soft_over_hard': {}, 'soft_minus_hard_us': {}, 'spread_us': {}}
    for k in us:
        if k.startswith('soft/'):
            n = k[len('soft/'):]
            h = us['hard/' + n]
            out['soft_over_hard'][n] = us[k][0] / h[0]
            out['soft_minus_hard_us'][n] = us[k][0] - h[0]
            out['spread_us'][n] = max(us[k][2] - us[k][1], h[2] - h[1])
    return out


def step_times(a, dev, math, b=32, t=4):
    from grl_amd import engine, train_engine
    from grl_amd.reid.loss import SoftClusterMemoryLoss, PairLoss
    from grl_amd.reid.train import MeanTeacher, MeanTeacherSEQTrainer
    from grl_amd.synthetic import synth_clips
    unit = torch.nn.functional.normalize
    clips = synth_clips(b, t, seed=0).to(dev)
    batch = (clips, (torch.arange(b, device=dev) // 2 * 7) % IDS, torch.arange(b, device=dev) % 6)
    fns = {}
    for name, tri_w in (('hard_triplet', 0.0), ('soft_triplet', W)):
        cnn, siam, siamv = models_on(dev)
        crits = []
        for s in (1, 2):
            mem = unit(torch.randn((IDS, 2048), generator=torch.Generator().manual_seed(s)), dim=1).to(dev)
            crits.append(SoftClusterMemoryLoss(2048, IDS, mode='instance').to(dev).reset(mem))
        tr = MeanTeacherSEQTrainer(cnn, siam, siamv, PairLoss().to(dev), crits[0], crits[1], None,
                                   teacher=MeanTeacher(cnn, siam, alpha=0.999), soft_weight=0.5, tri_soft_weight=tri_w)
        opt = torch.optim.SGD(tr._all_params(), lr=1e-3, momentum=0.9, weight_decay=5e-4, nesterov=True)

        def step(tr=tr, opt=opt):
            inputs, targets = tr._parse_data(batch)
            loss = tr._forward(inputs, targets, 0, 0)[0]
            opt.zero_grad()
            loss.backward()
            opt.step()
            tr.teacher.update()                            # (what MeanTeacherSEQTrainer.train hooks behind the step)
        fns[name] = step
    old, old_eval = train_engine.set_math(math), engine.get_math()
    engine.set_math(math)                                  # the teacher's eval forward on the same datapath
    try:
        ms = in_turn(fns, max(3, a.warm // 3), a.steps)
    finally:
        train_engine.set_math(old)
        engine.set_math(old_eval)
    diff = ms['soft_triplet'][0] - ms['hard_triplet'][0]
    spread = max(v[2] - v[1] for v in ms.values())
    return {'b': b, 't': t, 'math': math, 'ms_per_step': ms, 'soft_minus_hard_ms': diff, 'spread_ms': spread,
            'within_spread': bool(diff <= spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warm', type=int, default=15)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=50)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = {'warm': a.warm, 'reps': a.reps, 'batch': a.batch, 'w_soft': W, 'D': D, 'device': torch.cuda.get_device_name(0)}
    res['pair'] = pair_times(a, dev)
    if not a.no_step:
        res['step'] = [step_times(a, dev, 'f32'), step_times(a, dev, 'bf16s')]
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
    assert np.isfinite(list(res['pair']['soft_over_hard'].values())).all()


if __name__ == '__main__':
    main()
