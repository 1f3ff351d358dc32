#!/usr/bin/env python
"""Times the camera-aware proxy cross entropy and the trainer step that carries it.

* grl_proxy_ce (k_neg = 50, both terms, all outputs the loss asks for) against grl_softmax_ce, the call it replaces, on the
  same n x P logits in the same process: n = 32 and 128 rows, P = 2048 and 4096 proxies spread over 6 cameras.  A call is a
  few microseconds, so a timed window is ``--batch`` calls between two HIP events; reported per call.
* one 32 x 4 trainer step on bf16 storage (forward + 5-term loss + backward + SGD, bench.py's) with ClusterMemoryLoss (625
  centroids, SEQTrainer) and with ProxyMemoryLoss (625 and 625 x 6 proxies, CameraSEQTrainer), in turn.

One process, the functions in turn: warm-ups, then the median of the timed windows (the discipline of tools/verify_rate.py).
Nothing here is a threshold.

  python tools/proxy_rate.py [--warm 15] [--reps 20] [--batch 50] [--steps 20] [--no-step] [--json PATH]
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

CAMS, K_NEG, IDS = 6, 50, 625


def kernel_times(a, dev):
    from grl_amd import engine
    from grl_amd._lib import ptr
    g = torch.Generator().manual_seed(0)
    fns, keep = {}, []
    for n in (32, 128):
        for P in (2048, 4096):
            z = (14.0 * torch.cos(6.2831853 * torch.rand((n, P), generator=g))).to(dev)
            pcl = (torch.arange(P) // CAMS).to(torch.int32).to(dev)
            pcm = (torch.arange(P) % CAMS).to(torch.int32).to(dev)
            j = torch.randint(0, P, (n,), generator=g)
            y, cam = (j // CAMS).to(dev), (j % CAMS).to(dev)
            loss, cor = torch.empty((), device=dev), torch.empty((), device=dev)
            dz, own, ws = torch.empty_like(z), torch.empty(n, dtype=torch.int64, device=dev), torch.empty(3 * n, device=dev)
            keep.append((z, pcl, pcm, y, cam, loss, cor, dz, own, ws))

            def proxy(z=z, pcl=pcl, pcm=pcm, y=y, cam=cam, loss=loss, cor=cor, dz=dz, own=own, ws=ws, n=n, P=P):
                for _ in range(a.batch):
                    engine._call('grl_proxy_ce', ptr(z), P, ptr(y), ptr(cam), ptr(pcl), ptr(pcm), n, P, K_NEG, C.c_float(1.0),
                                 C.c_float(0.5), ptr(loss), ptr(cor), ptr(dz), P, ptr(own), None, ptr(ws))

            def softmax(z=z, y=y, loss=loss, cor=cor, dz=dz, ws=ws, n=n, P=P):
                for _ in range(a.batch):
                    engine._call('grl_softmax_ce', ptr(z), P, ptr(y), None, n, P, ptr(loss), ptr(cor), ptr(dz), P, ptr(ws))
            fns['proxy_ce/n%d/P%d' % (n, P)] = proxy
            fns['softmax_ce/n%d/P%d' % (n, P)] = softmax
    ms = in_turn(fns, a.warm, a.reps)
    us = {k: tuple(1e3 * v / a.batch for v in t) for k, t in ms.items()}
    ratio = {k[len('proxy_ce/'):]: us[k][0] / us['softmax_ce/' + k[len('proxy_ce/'):]][0] for k in us if k.startswith('proxy_ce/')}
    return {'us_per_call': us, 'proxy_over_softmax': ratio}


def step_times(a, dev, b=32, t=4):
    from grl_amd import train_engine
    from grl_amd.reid import models
    from grl_amd.reid.loss import ClusterMemoryLoss, ProxyMemoryLoss, PairLoss
    from grl_amd.reid.train import SEQTrainer, CameraSEQTrainer
    from grl_amd.synthetic import synth_clips, synth_state_dict
    unit = torch.nn.functional.normalize
    clips = synth_clips(b, t, seed=0).to(dev)
    pids = (torch.arange(b, device=dev) // 2 * 7) % IDS
    cams = torch.arange(b, device=dev) % CAMS
    fns = {}
    for name, P in (('cluster_memory/K625', IDS), ('proxy_memory/P625', IDS), ('proxy_memory/P3750', IDS * CAMS)):
        with contextlib.redirect_stdout(io.StringIO()):
            cnn = models.create('resnet50_grl', num_features=2048, dropout=0, numclasses=IDS, pretrained=False)
        siam = models.create('siamese', input_num=2048, output_num=512, class_num=2)
        siamv = models.create('siamese_video', input_num=2048, output_num=512, class_num=2)
        cnn.load_state_dict(synth_state_dict(cnn, seed=0))
        siam.load_state_dict(synth_state_dict(siam, seed=0, prefix='siamese.'))
        siamv.load_state_dict(synth_state_dict(siamv, seed=0, prefix='siamese_video.'))
        cnn, siam, siamv = cnn.to(dev).train(), siam.to(dev).train(), siamv.to(dev).train()
        crits = []
        for s in (1, 2):
            mem = unit(torch.randn((P, 2048), generator=torch.Generator().manual_seed(s)), dim=1).to(dev)
            if name.startswith('cluster'):
                crits.append(ClusterMemoryLoss(2048, P, mode='instance').to(dev).reset(mem))
            else:
                per = P // IDS                                   # proxies per cluster: cameras 0 .. per - 1
                pcl, pcm = (torch.arange(P) // per).to(torch.int32).to(dev), (torch.arange(P) % per).to(torch.int32).to(dev)
                crits.append(ProxyMemoryLoss(2048, mode='instance').to(dev).reset(mem, pcl, pcm))
        cls = SEQTrainer if name.startswith('cluster') else CameraSEQTrainer
        tr = cls(cnn, siam, siamv, PairLoss().to(dev), crits[0], crits[1], None)
        opt = torch.optim.SGD(tr._all_params(), lr=1e-3, momentum=0.9, weight_decay=5e-4, nesterov=True)
        batch = (clips, pids, cams % (P // IDS))

        def step(tr=tr, opt=opt, batch=batch):
            inputs, targets = tr._parse_data(batch)
            loss = tr._forward(inputs, targets, 0, 0)[0]
            opt.zero_grad()
            loss.backward()
            opt.step()
        fns[name] = step
    old = train_engine.set_math('bf16s')
    try:
        ms = in_turn(fns, max(3, a.warm // 3), a.steps)
    finally:
        train_engine.set_math(old)
    return {'b': b, 't': t, 'math': 'bf16s', 'ms_per_step': ms}


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
    res = {'cams': CAMS, 'k_neg': K_NEG, 'warm': a.warm, 'reps': a.reps, 'batch': a.batch, 'device': torch.cuda.get_device_name(0)}
    res['kernel'] = kernel_times(a, dev)
    if not a.no_step:
        res['step'] = step_times(a, dev)
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
    assert np.isfinite(list(res['kernel']['proxy_over_softmax'].values())).all()


if __name__ == '__main__':
    main()
