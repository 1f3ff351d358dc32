#!/usr/bin/env python
"""Times one pass over the set-distance blocks (engine._SetBlocks) at the MARS dense shape: 1980 query
and 13290 gallery tracklets of 15 clips each, d = 6144, 'chamfer' over 'cosine' clip distances, on unit-norm synthetic
clip rows (tracklet centre + noise).  A pass is what set_search / set_pair_roc run once and set_metrics_streaming twice:
every block of the tracklet x tracklet distances, each from its clip tiles -- one fp32 NEGDOT GEMM into the scratch and
one grl_setdist_block on it.  HIP events around every GEMM, every grl_setdist_block and the whole pass; ``--warm`` passes
first (code objects, the allocator, clocks), then ``--reps`` timed ones, the median reported.

Prints one JSON line: the shape, the tiles, ms per pass for the GEMMs, for grl_setdist_block and in total, the achieved
GEMM TFLOP/s and the scratch bytes per second the reduction reads, and the reduction's share of the GEMM time.

  python tools/setdist_rate.py [--warm 2] [--reps 3] [--nq 1980] [--ng 13290] [--clips 15] [--d 6144]
                               [--reduce chamfer] [--metric cosine] [--json PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _clips(n, clips, d, seed, dev, noise=0.35):
    """[n * clips, d] unit rows on the device: tracklet centre + noise, generated in slabs (the gallery is 4.9 GB)"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    out = torch.empty((n * clips, d), dtype=torch.float32, device=dev)
    step = 1024
    for t0 in range(0, n, step):
        t1 = min(t0 + step, n)
        centre = torch.randn((t1 - t0, 1, d), generator=g, device=dev)
        x = centre + noise * float(np.sqrt(d)) * torch.randn((t1 - t0, clips, d), generator=g, device=dev)
        x = x / x.norm(dim=2, keepdim=True)
        out[t0 * clips:t1 * clips] = x.view(-1, d)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warm', type=int, default=2)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--nq', type=int, default=1980)
    ap.add_argument('--ng', type=int, default=13290)
    ap.add_argument('--clips', type=int, default=15)
    ap.add_argument('--d', type=int, default=6144)
    ap.add_argument('--reduce', default='chamfer')
    ap.add_argument('--metric', default='cosine')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('setdist_rate.py measures on the GPU and found none')
    from grl_amd import engine
    dev = torch.device('cuda:0')
    qset = engine.TrackletSet(_clips(a.nq, a.clips, a.d, 1, dev), [a.clips] * a.nq)
    gset = engine.TrackletSet(_clips(a.ng, a.clips, a.d, 2, dev), [a.clips] * a.ng)
    blocks = engine._SetBlocks(qset, gset, a.reduce, a.metric)
    tiles = [t for c0, c1 in blocks.spans for t in blocks.tiles(c0, c1)]

    events = {'gemm': [], 'setdist': []}
    real_gemm, real_call = engine.gemm, engine._call

    def timed(kind, fn, *args, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn(*args, **kw)
        e1.record()
        events[kind].append((e0, e1))
        return r

    def gemm(*args, **kw):
        return timed('gemm', real_gemm, *args, **kw)

    def call(name, *args):
        if name == 'grl_setdist_block':
            return timed('setdist', real_call, name, *args)
        return real_call(name, *args)

    def one_pass():
        for c0, c1 in blocks.spans:
            blocks.block(c0, c1)
    runs = []
    engine.gemm, engine._call = gemm, call
    try:
        for it in range(a.warm + a.reps):
            del events['gemm'][:], events['setdist'][:]
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            one_pass()
            t1.record()
            torch.cuda.synchronize()
            if it >= a.warm:
                runs.append({'total': t0.elapsed_time(t1),
                             'gemm': sum(e0.elapsed_time(e1) for e0, e1 in events['gemm']),
                             'setdist': sum(e0.elapsed_time(e1) for e0, e1 in events['setdist'])})
    finally:
        engine.gemm, engine._call = real_gemm, real_call
    ms = {k: float(np.median([r[k] for r in runs])) for k in ('total', 'gemm', 'setdist')}
    nqc, ngc = a.nq * a.clips, a.ng * a.clips
    flop = 2.0 * nqc * ngc * qset.clips.shape[1]
    res = {'nq': a.nq, 'ng': a.ng, 'clips': a.clips, 'd': a.d, 'reduce': a.reduce, 'metric': a.metric,
           'device': torch.cuda.get_device_name(0), 'warm': a.warm, 'reps': a.reps,
           'block_bytes': blocks.budget, 'blocks': len(blocks.spans), 'tiles': len(tiles),
           'largest_tile_clips': [int(max(qset.ptr[t[1]] - qset.ptr[t[0]] for t in tiles)),
                                  int(max(gset.ptr[t[3]] - gset.ptr[t[2]] for t in tiles))],
           'ms': ms, 'ms_runs': runs,
           'gemm_tflops': flop / (ms['gemm'] * 1e-3) / 1e12,
           'setdist_scratch_gbps': 4.0 * nqc * ngc / (ms['setdist'] * 1e-3) / 1e9,
           'setdist_over_gemm': ms['setdist'] / ms['gemm']}
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
