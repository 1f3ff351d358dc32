#!/usr/bin/env python
"""Times the instance-contrast kernels and the trainer step that carries them.

* grl_ins_contrast_fwd + grl_ins_contrast_bwd at weights (1, 0.4), tau 0.1, against grl_soft_triplet_fwd + grl_soft_triplet_bwd
  (w_soft = 0.8) on the same n x 2048 student and teacher rows: n = 32 and 128, ids in pairs.  A pair of calls is a few
  microseconds, so a timed window is ``--batch`` pairs between two HIP events; reported per pair, with the ratio and the spread
  (max - min) of the windows.
* one 32 x 4 fp32 trainer step (forward + 5-term loss + backward + SGD + the teacher's update, bench.py's shapes) under
  MeanTeacherSEQTrainer + SoftClusterMemoryLoss with soft_weight = 0.5 and instance weights (0, 0) against (1, 0.4), and a third
  trainer built WITHOUT the instance arguments: it runs the launches of the (0, 0) one, so the difference of those two is what
  two identical steps differ by in this run.

No threshold: the expectation that the step with the terms stays within the spread of the windows is reported as
``within_spread``, not enforced.  One process, the variants alternating: warm-ups, then the median of the timed windows (the
discipline of tools/verify_rate.py).

  python tools/ins_contrast_rate.py [--warm 5] [--reps 20] [--batch 50] [--steps 20] [--no-step] [--json PATH]
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
W_TRI = 0.8
W_INS = (1.0, 0.4)
TAU = 0.1


def pair_times(a, dev):
    from grl_amd import engine
    from grl_amd._lib import ptr
    g = torch.Generator().manual_seed(0)
    fns, keep = {}, []
    for n in (32, 128):
        f = torch.nn.functional.normalize(torch.randn((n, D), generator=g), dim=1).to(dev)
        tf = torch.nn.functional.normalize(torch.randn((n, D), generator=g), dim=1).to(dev)
        y = (torch.arange(n) // 2).to(dev)
        loss, z, q = (torch.empty(n, device=dev) for _ in range(3))
        dist, cos, coef = (torch.empty((n, n), device=dev) for _ in range(3))
        sel2, seln = torch.empty((n, 2), dtype=torch.int32, device=dev), torch.empty((n, n), dtype=torch.int32, device=dev)
        dl, df = torch.full((n,), 1.0 / n, device=dev), torch.empty_like(f)
        keep.append((f, tf, y, loss, z, q, dist, cos, coef, sel2, seln, dl, df))

        def ins(f=f, tf=tf, y=y, loss=loss, cos=cos, coef=coef, sel=seln, dl=dl, df=df, n=n):
            for _ in range(a.batch):
                engine._call('grl_ins_contrast_fwd', ptr(f), ptr(tf), ptr(y), n, D, C.c_float(TAU), C.c_float(TAU), C.c_float(W_INS[0]),
                             C.c_float(W_INS[1]), ptr(loss), ptr(cos), ptr(sel), ptr(coef))
                engine._call('grl_ins_contrast_bwd', ptr(f), ptr(tf), ptr(coef), ptr(dl), C.c_float(TAU), ptr(df), n, D)

        def tri(f=f, tf=tf, y=y, loss=loss, z=z, q=q, dist=dist, sel=sel2, dl=dl, df=df, n=n):
            for _ in range(a.batch):
                engine._call('grl_soft_triplet_fwd', ptr(f), ptr(tf), ptr(y), n, D, C.c_float(W_TRI), ptr(loss), ptr(dist), ptr(sel),
                             ptr(z), ptr(q))
                engine._call('grl_soft_triplet_bwd', ptr(f), ptr(dist), ptr(sel), ptr(z), ptr(q), ptr(dl), C.c_float(W_TRI), ptr(df),
                             n, D)
        fns['ins/n%d' % n] = ins
        fns['tri/n%d' % n] = tri
    ms = in_turn(fns, a.warm, a.reps)
    us = {k: tuple(1e3 * v / a.batch for v in t) for k, t in ms.items()}
    out = {'us_per_pair': us, 'ins_over_tri': {}, 'ins_minus_tri_us': {}, 'spread_us': {}}
    for k in us:
        if k.startswith('ins/'):
            n = k[len('ins/'):]
            h = us['tri/' + n]
            out['ins_over_tri'][n] = us[k][0] / h[0]
            out['ins_minus_tri_us'][n] = us[k][0] - h[0]
            out['spread_us'][n] = max(us[k][2] - us[k][1], h[2] - h[1])
    return out


def step_times(a, dev, math='f32', b=32, t=4):
    from grl_amd import engine, train_engine
    from grl_amd.reid.loss import SoftClusterMemoryLoss, PairLoss
    from grl_amd.reid.train import MeanTeacher, MeanTeacherSEQTrainer
    from grl_amd.synthetic import synth_clips
    unit = torch.nn.functional.normalize
    clips = synth_clips(b, t, seed=0).to(dev)
    batch = (clips, (torch.arange(b, device=dev) // 2 * 7) % IDS, torch.arange(b, device=dev) % 6)
    fns = {}
    for name, extra in (('ins_0_0', dict(ins_hard_weight=0.0, ins_soft_weight=0.0)), ('no_ins_arguments', dict()),
                        ('ins_1_0.4', dict(ins_hard_weight=W_INS[0], ins_soft_weight=W_INS[1], ins_tau=TAU))):
        cnn, siam, siamv = models_on(dev)
        crits = []
        for s in (1, 2):
            mem = unit(torch.randn((IDS, 2048), generator=torch.Generator().manual_seed(s)), dim=1).to(dev)
            crits.append(SoftClusterMemoryLoss(2048, IDS, mode='instance').to(dev).reset(mem))
        tr = MeanTeacherSEQTrainer(cnn, siam, siamv, PairLoss().to(dev), crits[0], crits[1], None,
                                   teacher=MeanTeacher(cnn, siam, alpha=0.999), soft_weight=0.5, **extra)
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
        ms = in_turn(fns, a.warm, a.steps)
    finally:
        train_engine.set_math(old)
        engine.set_math(old_eval)
    diff = ms['ins_1_0.4'][0] - ms['ins_0_0'][0]
    same = ms['ins_0_0'][0] - ms['no_ins_arguments'][0]
    spread = max(v[2] - v[1] for v in ms.values())
    return {'b': b, 't': t, 'math': math, 'ms_per_step': ms, 'ins_minus_zero_ms': diff, 'zero_minus_no_arguments_ms': same,
            'spread_ms': spread, 'within_spread': bool(diff <= spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warm', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=50)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = {'warm': a.warm, 'reps': a.reps, 'batch': a.batch, 'w_ins': W_INS, 'tau': TAU, 'w_tri': W_TRI, 'D': D,
           'device': torch.cuda.get_device_name(0)}
    res['pair'] = pair_times(a, dev)
    if not a.no_step:
        res['step'] = [step_times(a, dev)]
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
    assert np.isfinite(list(res['pair']['ins_over_tri'].values())).all()


if __name__ == '__main__':
    main()
