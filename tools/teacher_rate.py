#!/usr/bin/env python
"""Times the mean teacher's two kernels and the trainer step that carries them.

* grl_ema_update over the REAL model's table (ResNet50-GRL + Siamese head: every float32 parameter and buffer, one launch)
  against the stock forms on the same tensors: torch._foreach_mul_ + torch._foreach_add_, and torch._foreach_lerp_.  Reported
  per call and as bytes moved per second (12 bytes per element: dst read, src read, dst written) against the 8 TB/s HBM peak
  the README uses.  THE ONE THRESHOLD of this tool: the HIP launch must not be slower than the mul + add form by more than
  the spread (max - min) of the repeated windows of this run; the tool exits non-zero if it is.
* grl_soft_ce against grl_softmax_ce on the same n x c logits: n = 64 and 128 rows, c = 625 and 2196 columns.  A call is a
  few microseconds, so a timed window is ``--batch`` calls between two HIP events; reported per call.
* one 32 x 4 trainer step (forward + 5-term loss + backward + SGD, bench.py's), fp32 and bf16 storage, under SEQTrainer +
  ClusterMemoryLoss and under MeanTeacherSEQTrainer + SoftClusterMemoryLoss (soft_weight 0.5, the teacher's update behind the
  optimizer step): the difference is the teacher's eval forward plus the two kernels.

One process, the functions in turn: warm-ups, then the median of the timed windows (the discipline of tools/verify_rate.py).

  python tools/teacher_rate.py [--warm 15] [--reps 20] [--batch 50] [--ema-batch 5] [--steps 20] [--no-step] [--json PATH]
"""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from verify_rate import in_turn  # noqa: E402

IDS = 625
HBM_PEAK = 8.0e12


def models_on(dev):
    from grl_amd.reid import models
    from grl_amd.synthetic import synth_state_dict
    with contextlib.redirect_stdout(io.StringIO()):
        cnn = models.create('resnet50_grl', num_features=2048, dropout=0, numclasses=IDS, pretrained=False)
    siam = models.create('siamese', input_num=2048, output_num=512, class_num=2)
    siamv = models.create('siamese_video', input_num=2048, output_num=512, class_num=2)
    cnn.load_state_dict(synth_state_dict(cnn, seed=0))
    siam.load_state_dict(synth_state_dict(siam, seed=0, prefix='siamese.'))
    siamv.load_state_dict(synth_state_dict(siamv, seed=0, prefix='siamese_video.'))
    return cnn.to(dev).train(), siam.to(dev).train(), siamv.to(dev).train()


def ema_times(a, dev):
    from grl_amd import engine
    from grl_amd._lib import ptr
    from grl_amd.reid.train import MeanTeacher
    cnn, siam, _ = models_on(dev)
    teacher = MeanTeacher(cnn, siam, alpha=0.999)
    dsts, srcs = [d for _, d, _ in teacher.pairs], [s.detach() for _, _, s in teacher.pairs]
    alpha, oma = 0.999, 1.0 - 0.999

    def hip():
        for _ in range(a.ema_batch):
            engine._call('grl_ema_update', ptr(teacher.table), ptr(teacher.chunk_first), teacher.count, C.c_float(alpha),
                         C.c_float(oma))

    def foreach_mul_add():
        for _ in range(a.ema_batch):
            torch._foreach_mul_(dsts, alpha)
            torch._foreach_add_(dsts, srcs, alpha=oma)

    def foreach_lerp():
        for _ in range(a.ema_batch):
            torch._foreach_lerp_(dsts, srcs, oma)
    ms = in_turn({'grl_ema_update': hip, 'foreach_mul_add': foreach_mul_add, 'foreach_lerp': foreach_lerp}, a.warm, a.reps)
    per = {k: tuple(v / a.ema_batch for v in t) for k, t in ms.items()}
    nbytes = 12 * teacher.numel
    rate = {k: nbytes / (t[0] * 1e-3) for k, t in per.items()}
    spread = max(per[k][2] - per[k][1] for k in ('grl_ema_update', 'foreach_mul_add'))
    return {'tensors': teacher.count, 'floats': teacher.numel, 'bytes_per_call': nbytes, 'ms_per_call': per,
            'bytes_per_s': rate, 'fraction_of_8TBps': {k: v / HBM_PEAK for k, v in rate.items()},
            'hip_minus_foreach_ms': per['grl_ema_update'][0] - per['foreach_mul_add'][0], 'spread_ms': spread,
            'within_threshold': bool(per['grl_ema_update'][0] - per['foreach_mul_add'][0] <= spread)}


def ce_times(a, dev):
    from grl_amd import engine
    from grl_amd._lib import ptr
    g = torch.Generator().manual_seed(0)
    fns, keep = {}, []
    for n in (64, 128):
        for c in (625, 2196):
            z = (20.0 * torch.cos(6.2831853 * torch.rand((n, c), generator=g))).to(dev)
            tz = (z + 4.0 * torch.randn((n, c), generator=g).to(dev)).clamp_(-20.0, 20.0)
            y = torch.randint(0, c, (n,), generator=g).to(dev)
            loss, cor = torch.empty((), device=dev), torch.empty((), device=dev)
            dz, ws = torch.empty_like(z), torch.empty(3 * n, device=dev)
            keep.append((z, tz, y, loss, cor, dz, ws))

            def soft(z=z, tz=tz, y=y, loss=loss, cor=cor, dz=dz, ws=ws, n=n, c=c):
                for _ in range(a.batch):
                    engine._call('grl_soft_ce', ptr(z), c, ptr(tz), c, ptr(y), C.c_float(0.5), n, c, ptr(loss), ptr(cor), ptr(dz),
                                 c, ptr(ws))

            def softmax(z=z, y=y, loss=loss, cor=cor, dz=dz, ws=ws, n=n, c=c):
                for _ in range(a.batch):
                    engine._call('grl_softmax_ce', ptr(z), c, ptr(y), None, n, c, ptr(loss), ptr(cor), ptr(dz), c, ptr(ws))
            fns['soft_ce/n%d/c%d' % (n, c)] = soft
            fns['softmax_ce/n%d/c%d' % (n, c)] = softmax
    ms = in_turn(fns, a.warm, a.reps)
    us = {k: tuple(1e3 * v / a.batch for v in t) for k, t in ms.items()}
    ratio = {k[len('soft_ce/'):]: us[k][0] / us['softmax_ce/' + k[len('soft_ce/'):]][0] for k in us if k.startswith('soft_ce/')}
    return {'us_per_call': us, 'soft_over_softmax': ratio}


def step_times(a, dev, math, b=32, t=4):
    from grl_amd import engine, train_engine
    from grl_amd.reid.loss import ClusterMemoryLoss, SoftClusterMemoryLoss, PairLoss
    from grl_amd.reid.train import SEQTrainer, MeanTeacher, MeanTeacherSEQTrainer
    from grl_amd.synthetic import synth_clips
    unit = torch.nn.functional.normalize
    clips = synth_clips(b, t, seed=0).to(dev)
    batch = (clips, (torch.arange(b, device=dev) // 2 * 7) % IDS, torch.arange(b, device=dev) % 6)
    fns = {}
    for name in ('seq_trainer/cluster_memory', 'mean_teacher/soft_cluster_memory'):
        cnn, siam, siamv = models_on(dev)
        mt = name.startswith('mean_teacher')
        crits = []
        for s in (1, 2):
            mem = unit(torch.randn((IDS, 2048), generator=torch.Generator().manual_seed(s)), dim=1).to(dev)
            crits.append((SoftClusterMemoryLoss if mt else ClusterMemoryLoss)(2048, IDS, mode='instance').to(dev).reset(mem))
        if mt:
            tr = MeanTeacherSEQTrainer(cnn, siam, siamv, PairLoss().to(dev), crits[0], crits[1], None,
                                       teacher=MeanTeacher(cnn, siam, alpha=0.999), soft_weight=0.5)
        else:
            tr = SEQTrainer(cnn, siam, siamv, PairLoss().to(dev), crits[0], crits[1], None)
        opt = torch.optim.SGD(tr._all_params(), lr=1e-3, momentum=0.9, weight_decay=5e-4, nesterov=True)

        def step(tr=tr, opt=opt, mt=mt):
            inputs, targets = tr._parse_data(batch)
            loss = tr._forward(inputs, targets, 0, 0)[0]
            opt.zero_grad()
            loss.backward()
            opt.step()
            if mt:
                tr.teacher.update()                        # (what MeanTeacherSEQTrainer.train hooks behind the step)
        fns[name] = step
    old, old_eval = train_engine.set_math(math), engine.get_math()
    engine.set_math(math)                                  # the teacher's eval forward on the same datapath
    try:
        ms = in_turn(fns, max(3, a.warm // 3), a.steps)
    finally:
        train_engine.set_math(old)
        engine.set_math(old_eval)
    return {'b': b, 't': t, 'math': math, 'ms_per_step': ms,
            'teacher_ms': ms['mean_teacher/soft_cluster_memory'][0] - ms['seq_trainer/cluster_memory'][0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warm', type=int, default=15)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=50)
    ap.add_argument('--ema-batch', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = {'warm': a.warm, 'reps': a.reps, 'batch': a.batch, 'ema_batch': a.ema_batch, 'device': torch.cuda.get_device_name(0)}
    res['ema'] = ema_times(a, dev)
    res['kernel'] = ce_times(a, dev)
    if not a.no_step:
        res['step'] = [step_times(a, dev, 'f32'), step_times(a, dev, 'bf16s')]
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
    assert np.isfinite(list(res['kernel']['soft_over_softmax'].values())).all()
    if not res['ema']['within_threshold']:
        sys.exit('grl_ema_update is slower than _foreach_mul_ + _foreach_add_ by %.4f ms per call, more than the spread of the '
                 'windows (%.4f ms): find out why' % (res['ema']['hip_minus_foreach_ms'], res['ema']['spread_ms']))


if __name__ == '__main__':
    main()
