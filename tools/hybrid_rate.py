#!/usr/bin/env python
"""Times the hybrid-memory cross entropy and the trainer step that carries it.

* grl_hybrid_ce against grl_softmax_ce on the same n x N logits in the same process: n = 64 and 128 rows, N = 2196 and 8298
  memory rows (the MARS training tracklets of one camera pair / of all), about a third of the rows outliers -- singleton
  classes -- and the rest in clusters of 2 .. 14 interleaved members.  grl_softmax_ce sees the N columns as N classes: the
  same bytes read and written.  A call is a few microseconds, so a timed window is ``--batch`` calls between two HIP
  events; reported per call.
* one 32 x 4 trainer step on bf16 storage (forward + 5-term loss + backward + SGD, bench.py's) with ClusterMemoryLoss (625
  centroids, SEQTrainer) and with HybridMemoryLoss (2196 and 8298 instances, HybridSEQTrainer), in turn.

One process, the functions in turn: warm-ups, then the median of the timed windows (the discipline of tools/verify_rate.py).
Nothing here is a threshold.

  python tools/hybrid_rate.py [--warm 15] [--reps 20] [--batch 50] [--steps 20] [--no-step] [--json PATH]
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

from verify_rate import in_turn  # noqa: E402

IDS = 625


def classes(N, seed=0):
    """int64 numpy [N], -1 = outlier: about a third outliers, the rest in clusters of 2 .. 14 members, shuffled"""
    g = np.random.Generator(np.random.PCG64(seed))
    labels, k, left = [], 0, N - N // 3
    while left > 0:
        size = min(left, int(g.integers(2, 15)))
        labels += [k] * size
        k, left = k + 1, left - size
    labels = np.array(labels + [-1] * (N // 3), np.int64)
    return labels[g.permutation(N)]


def kernel_times(a, dev):
    from grl_amd import engine
    from grl_amd._lib import ptr
    from grl_amd.reid.train.pseudo import PseudoLabels
    g = torch.Generator().manual_seed(0)
    fns, keep, shape = {}, [], {}
    for n in (64, 128):
        for N in (2196, 8298):
            z = (14.0 * torch.cos(6.2831853 * torch.rand((n, N), generator=g))).to(dev)
            h = PseudoLabels(torch.from_numpy(classes(N)).to(dev)).hybrid()
            y = h.sample_class_dev[torch.randint(0, N, (n,), generator=g).to(dev)].contiguous()
            cp, cm, ic, nc = h.class_ptr_dev, h.class_members_dev, h.inst_class_dev, h.n_classes
            loss, cor = torch.empty((), device=dev), torch.empty((), device=dev)
            dz, ws = torch.empty_like(z), torch.empty(3 * n, device=dev)
            keep.append((z, h, y, loss, cor, dz, ws))
            shape['n%d/N%d' % (n, N)] = {'classes': nc, 'outliers': int(h.labels.n_noise)}

            def hybrid(z=z, y=y, cp=cp, cm=cm, ic=ic, loss=loss, cor=cor, dz=dz, ws=ws, n=n, N=N, nc=nc):
                for _ in range(a.batch):
                    engine._call('grl_hybrid_ce', ptr(z), N, ptr(y), ptr(cp), ptr(cm), ptr(ic), n, N, nc, ptr(loss), ptr(cor),
                                 ptr(dz), N, ptr(ws))

            def softmax(z=z, y=y, loss=loss, cor=cor, dz=dz, ws=ws, n=n, N=N):
                for _ in range(a.batch):
                    engine._call('grl_softmax_ce', ptr(z), N, ptr(y), None, n, N, ptr(loss), ptr(cor), ptr(dz), N, ptr(ws))
            fns['hybrid_ce/n%d/N%d' % (n, N)] = hybrid
            fns['softmax_ce/n%d/N%d' % (n, N)] = softmax
    ms = in_turn(fns, a.warm, a.reps)
    us = {k: tuple(1e3 * v / a.batch for v in t) for k, t in ms.items()}
    ratio = {k[len('hybrid_ce/'):]: us[k][0] / us['softmax_ce/' + k[len('hybrid_ce/'):]][0] for k in us if k.startswith('hybrid_ce/')}
    return {'us_per_call': us, 'hybrid_over_softmax': ratio, 'shape': shape}


def step_times(a, dev, b=32, t=4):
    from grl_amd import train_engine
    from grl_amd.reid import models
    from grl_amd.reid.loss import ClusterMemoryLoss, HybridMemoryLoss, PairLoss
    from grl_amd.reid.train import SEQTrainer, HybridSEQTrainer
    from grl_amd.reid.train.pseudo import PseudoLabels
    from grl_amd.synthetic import synth_clips, synth_state_dict
    unit = torch.nn.functional.normalize
    clips = synth_clips(b, t, seed=0).to(dev)
    cams = torch.arange(b, device=dev) % 6
    fns = {}
    for name, N in (('cluster_memory/K625', IDS), ('hybrid_memory/N2196', 2196), ('hybrid_memory/N8298', 8298)):
        with contextlib.redirect_stdout(io.StringIO()):
            cnn = models.create('resnet50_grl', num_features=2048, dropout=0, numclasses=IDS, pretrained=False)
        siam = models.create('siamese', input_num=2048, output_num=512, class_num=2)
        siamv = models.create('siamese_video', input_num=2048, output_num=512, class_num=2)
        cnn.load_state_dict(synth_state_dict(cnn, seed=0))
        siam.load_state_dict(synth_state_dict(siam, seed=0, prefix='siamese.'))
        siamv.load_state_dict(synth_state_dict(siamv, seed=0, prefix='siamese_video.'))
        cnn, siam, siamv = cnn.to(dev).train(), siam.to(dev).train(), siamv.to(dev).train()
        hybrid = name.startswith('hybrid')
        if hybrid:
            h = PseudoLabels(torch.from_numpy(classes(N)).to(dev)).hybrid()
            idx = []                                                     # pairs as the pair sampler's: two instances of one class,
            for k in range(b // 2):                                      # an outlier with itself
                i = (k * 37) % N
                mem = h.class_members[h.class_ptr[h.inst_class[i]]:h.class_ptr[h.inst_class[i] + 1]]
                idx += [i, int(mem[-1] if mem[-1] != i else mem[0])]
            index = torch.tensor(idx, dtype=torch.int64, device=dev)
            batch = (clips, h.sample_class_dev[index], cams, index)
        else:
            batch = (clips, (torch.arange(b, device=dev) // 2 * 7) % IDS, cams)
        crits = []
        for s in (1, 2):
            mem = unit(torch.randn((N, 2048), generator=torch.Generator().manual_seed(s)), dim=1).to(dev)
            if hybrid:
                crits.append(HybridMemoryLoss(2048).to(dev).reset(mem, h.class_ptr_dev, h.class_members_dev, h.inst_class_dev))
            else:
                crits.append(ClusterMemoryLoss(2048, N, mode='instance').to(dev).reset(mem))
        tr = (HybridSEQTrainer if hybrid else SEQTrainer)(cnn, siam, siamv, PairLoss().to(dev), crits[0], crits[1], None)
        opt = torch.optim.SGD(tr._all_params(), lr=1e-3, momentum=0.9, weight_decay=5e-4, nesterov=True)

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
    res = {'warm': a.warm, 'reps': a.reps, 'batch': a.batch, 'device': torch.cuda.get_device_name(0)}
    res['kernel'] = kernel_times(a, dev)
    if not a.no_step:
        res['step'] = step_times(a, dev)
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
    assert np.isfinite(list(res['kernel']['hybrid_over_softmax'].values())).all()


if __name__ == '__main__':
    main()
