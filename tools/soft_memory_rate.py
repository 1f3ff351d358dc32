#!/usr/bin/env python
"""Times the two soft memory kernels against their hard twins and the trainer steps that carry them.

* grl_soft_hybrid_ce (w = 0.5) against grl_hybrid_ce on the same n x N logits: n = 128 rows, (N, C) = (625, 625) -- every
  instance a class of its own, an early epoch -- and (8298, ~2000): MARS's tracklets in clusters of random sizes.
* grl_soft_proxy_ce (w = 0.5) against grl_proxy_ce: n = 128, P = 625 and 2196 proxies over 6 cameras, k_neg = 50.
  A call is tens of microseconds, so a timed window is ``--batch`` calls between two HIP events; reported per call.
* one 32 x 4 trainer step (forward + 5-term loss + backward + SGD, bench.py's) in fp32: HybridSEQTrainer + HybridMemoryLoss
  against MeanTeacherHybridSEQTrainer + SoftHybridMemoryLoss, CameraSEQTrainer + ProxyMemoryLoss against
  MeanTeacherCameraSEQTrainer + SoftProxyMemoryLoss (soft_weight 0.5, the teacher's update behind the optimizer step): the
  difference is the teacher's eval forward plus the soft kernels.

One process, the variants in turn: warm-ups, then the median of the timed windows with their minimum and maximum (the
discipline of tools/verify_rate.py / tools/teacher_rate.py).  No threshold: the figures go to EXPERIMENTS.md.

  python tools/soft_memory_rate.py [--warm 15] [--reps 20] [--batch 50] [--steps 20] [--no-step] [--json PATH]
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

N_ROWS = 128
HYBRID_SHAPES = ((625, 625), (8298, 2000))
PROXY_SHAPES = (625, 2196)
CAMS, K_NEG = 6, 50


def partition(N, C, seed):
    """(class_ptr, class_members, inst_class) int32 of N instances in C non-empty classes of random sizes (C = N: singletons)"""
    r = np.random.RandomState(seed)
    ic = np.concatenate((np.arange(C), r.randint(0, C, N - C)))
    r.shuffle(ic)
    order = np.argsort(ic, kind='stable')
    ptr = np.concatenate(([0], np.cumsum(np.bincount(ic, minlength=C))))
    return ptr.astype(np.int32), order.astype(np.int32), ic.astype(np.int32)


def hybrid_times(a, dev):
    from grl_amd import engine
    from grl_amd._lib import ptr
    g = torch.Generator().manual_seed(0)
    n, fns, keep, classes = N_ROWS, {}, [], {}
    for N, C0 in HYBRID_SHAPES:
        cp, cm, ic = (torch.from_numpy(t).to(dev) for t in partition(N, C0, N))
        nc = cp.numel() - 1
        z = (20.0 * torch.cos(6.2831853 * torch.rand((n, N), generator=g))).to(dev)
        tz = (z + 4.0 * torch.randn((n, N), generator=g).to(dev)).clamp_(-20.0, 20.0)
        y = ic[torch.randint(0, N, (n,), generator=g).to(dev)].to(torch.int64)
        loss, cor = torch.empty((), device=dev), torch.empty((), device=dev)
        dz, ws = torch.empty_like(z), torch.empty(3 * n + n * nc, device=dev)
        keep.append((z, tz, y, cp, cm, ic, loss, cor, dz, ws))
        classes['N%d' % N] = nc

        def soft(z=z, tz=tz, y=y, cp=cp, cm=cm, ic=ic, loss=loss, cor=cor, dz=dz, ws=ws, N=N, nc=nc):
            for _ in range(a.batch):
                engine._call('grl_soft_hybrid_ce', ptr(z), N, ptr(tz), N, ptr(y), ptr(cp), ptr(cm), ptr(ic), C.c_float(0.5), n, N,
                             nc, ptr(loss), ptr(cor), ptr(dz), N, ptr(ws))

        def hard(z=z, y=y, cp=cp, cm=cm, ic=ic, loss=loss, cor=cor, dz=dz, ws=ws, N=N, nc=nc):
            for _ in range(a.batch):
                engine._call('grl_hybrid_ce', ptr(z), N, ptr(y), ptr(cp), ptr(cm), ptr(ic), n, N, nc, ptr(loss), ptr(cor), ptr(dz),
                             N, ptr(ws))
        fns['soft_hybrid_ce/N%d' % N] = soft
        fns['hybrid_ce/N%d' % N] = hard
    ms = in_turn(fns, a.warm, a.reps)
    us = {k: tuple(1e3 * v / a.batch for v in t) for k, t in ms.items()}
    ratio = {k[len('soft_hybrid_ce/'):]: us[k][0] / us['hybrid_ce/' + k[len('soft_hybrid_ce/'):]][0]
             for k in us if k.startswith('soft_hybrid_ce/')}
    return {'n': n, 'classes': classes, 'us_per_call': us, 'soft_over_hard': ratio}


def proxy_times(a, dev):
    from grl_amd import engine
    from grl_amd._lib import ptr
    g = torch.Generator().manual_seed(1)
    n, fns, keep = N_ROWS, {}, []
    for P in PROXY_SHAPES:
        j = torch.arange(P)
        pcl, pcm = (j // CAMS).to(torch.int32).to(dev), (j % CAMS).to(torch.int32).to(dev)
        z = (14.0 * torch.cos(6.2831853 * torch.rand((n, P), generator=g))).to(dev)
        tz = (z + 3.0 * torch.randn((n, P), generator=g).to(dev)).clamp_(-14.0, 14.0)
        pick = torch.randint(0, P, (n,), generator=g).to(dev)
        y, cam = pcl[pick].to(torch.int64), pcm[pick].to(torch.int64)
        loss, cor = torch.empty((), device=dev), torch.empty((), device=dev)
        dz, ws, own = torch.empty_like(z), torch.empty(3 * n, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
        keep.append((z, tz, y, cam, pcl, pcm, loss, cor, dz, ws, own))

        def soft(z=z, tz=tz, y=y, cam=cam, pcl=pcl, pcm=pcm, loss=loss, cor=cor, dz=dz, ws=ws, own=own, P=P):
            for _ in range(a.batch):
                engine._call('grl_soft_proxy_ce', ptr(z), P, ptr(tz), P, ptr(y), ptr(cam), ptr(pcl), ptr(pcm), C.c_float(0.5), n, P,
                             K_NEG, C.c_float(1.0), C.c_float(0.5), ptr(loss), ptr(cor), ptr(dz), P, ptr(own), None, ptr(ws))

        def hard(z=z, y=y, cam=cam, pcl=pcl, pcm=pcm, loss=loss, cor=cor, dz=dz, ws=ws, own=own, P=P):
            for _ in range(a.batch):
                engine._call('grl_proxy_ce', ptr(z), P, ptr(y), ptr(cam), ptr(pcl), ptr(pcm), n, P, K_NEG, C.c_float(1.0),
                             C.c_float(0.5), ptr(loss), ptr(cor), ptr(dz), P, ptr(own), None, ptr(ws))
        fns['soft_proxy_ce/P%d' % P] = soft
        fns['proxy_ce/P%d' % P] = hard
    ms = in_turn(fns, a.warm, a.reps)
    us = {k: tuple(1e3 * v / a.batch for v in t) for k, t in ms.items()}
    ratio = {k[len('soft_proxy_ce/'):]: us[k][0] / us['proxy_ce/' + k[len('soft_proxy_ce/'):]][0]
             for k in us if k.startswith('soft_proxy_ce/')}
    return {'n': n, 'k_neg': K_NEG, 'cams': CAMS, 'us_per_call': us, 'soft_over_hard': ratio}


def step_times(a, dev, kind, b=32, t=4):
    """``kind``: 'hybrid' (625 instances, every pair of clips one cluster of two) or 'camera' (625 clusters x 6 cameras)"""
    from grl_amd import engine, train_engine
    from grl_amd.reid.loss import HybridMemoryLoss, ProxyMemoryLoss, SoftHybridMemoryLoss, SoftProxyMemoryLoss, PairLoss
    from grl_amd.reid.train import (HybridSEQTrainer, CameraSEQTrainer, MeanTeacher, MeanTeacherHybridSEQTrainer,
                                    MeanTeacherCameraSEQTrainer)
    from grl_amd.synthetic import synth_clips
    unit = torch.nn.functional.normalize
    clips = synth_clips(b, t, seed=0).to(dev)
    ar = torch.arange(b, device=dev)
    if kind == 'hybrid':
        rows = IDS
        cp, cm, ic = (torch.from_numpy(x).to(dev) for x in partition(rows, rows // 2, 3))
        index = (ar * 7) % rows
        index[1::2] = index[0::2]                           # a pair of clips shares its instance (and so its class)
        batch = (clips, ic[index].to(torch.int64), ar % CAMS, index)
        names = ('hybrid_trainer/hybrid_memory', 'mean_teacher/soft_hybrid_memory')
    else:
        rows = IDS * CAMS
        j = torch.arange(rows)
        pcl, pcm = (j // CAMS).to(torch.int32).to(dev), (j % CAMS).to(torch.int32).to(dev)
        batch = (clips, (ar // 2 * 7) % IDS, ar % CAMS)
        names = ('camera_trainer/proxy_memory', 'mean_teacher/soft_proxy_memory')
    fns = {}
    for name in names:
        cnn, siam, siamv = models_on(dev)
        mt = name.startswith('mean_teacher')
        crits = []
        for s in (1, 2):
            mem = unit(torch.randn((rows, 2048), generator=torch.Generator().manual_seed(s)), dim=1).to(dev)
            if kind == 'hybrid':
                crits.append((SoftHybridMemoryLoss if mt else HybridMemoryLoss)(2048).to(dev).reset(mem, cp, cm, ic))
            else:
                crits.append((SoftProxyMemoryLoss if mt else ProxyMemoryLoss)(2048, k_neg=K_NEG).to(dev).reset(mem, pcl, pcm))
        base, soft = ((HybridSEQTrainer, MeanTeacherHybridSEQTrainer) if kind == 'hybrid'
                      else (CameraSEQTrainer, MeanTeacherCameraSEQTrainer))
        if mt:
            tr = soft(cnn, siam, siamv, PairLoss().to(dev), crits[0], crits[1], None, teacher=MeanTeacher(cnn, siam, alpha=0.999),
                      soft_weight=0.5)
        else:
            tr = base(cnn, siam, siamv, PairLoss().to(dev), crits[0], crits[1], None)
        opt = torch.optim.SGD(tr._all_params(), lr=1e-3, momentum=0.9, weight_decay=5e-4, nesterov=True)

        def step(tr=tr, opt=opt, mt=mt):
            inputs, targets = tr._parse_data(batch)
            loss = tr._forward(inputs, targets, 0, 0)[0]
            opt.zero_grad()
            loss.backward()
            opt.step()
            if mt:
                tr.teacher.update()                        # (what the trainers' train() hooks behind the step)
        fns[name] = step
    old, old_eval = train_engine.set_math('f32'), engine.get_math()
    engine.set_math('f32')                                 # the teacher's eval forward on the same datapath
    try:
        ms = in_turn(fns, max(3, a.warm // 3), a.steps)
    finally:
        train_engine.set_math(old)
        engine.set_math(old_eval)
    return {'kind': kind, 'b': b, 't': t, 'math': 'f32', 'memory_rows': rows, 'ms_per_step': ms,
            'teacher_ms': ms[names[1]][0] - ms[names[0]][0]}


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
    res = {'warm': a.warm, 'reps': a.reps, 'batch': a.batch, 'device': torch.cuda.get_device_name(0)}
    res['hybrid'] = hybrid_times(a, dev)
    res['proxy'] = proxy_times(a, dev)
    if not a.no_step:
        res['step'] = [step_times(a, dev, 'hybrid'), step_times(a, dev, 'camera')]
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
    assert np.isfinite(list(res['hybrid']['soft_over_hard'].values()) + list(res['proxy']['soft_over_hard'].values())).all()


if __name__ == '__main__':
    main()
