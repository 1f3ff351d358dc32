#!/usr/bin/env python
"""The 'mxfp8' eval datapath against 'bf16s' and 'f32' in ONE process on the same clips (synthetic weights):

  * configs[2] (64 x 8): bf16s / mxfp8 alternated three times; configs[1] (32 x 4): f32 / mxfp8 once;
    each series 15 warm-up + 20 timed steps of engine.extract_features;
  * clip-features/s, ms per step and the feature deviation against 'f32' (min per-clip cosine, relative L2);
  * the MX GEMM's TFLOP/s on the pipeline's dominant shapes next to the bf16s kernel on the same shape (layer-3 3x3
    conv, layer-3 / 4 1x1 convs, the TRL memo GEMM b*128 x 2048 x 2048), as a fraction of the MX-fp8 and bf16 dense
    peaks; the MX time includes its activation-quantisation pass (reported separately too).

  python tools/mxfp8_rate.py [--steps 20] [--warmup 15] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BF16_TF = 2500.0           # MI355X_MICROARCH.md: dense bf16 MFMA
PEAK_MXFP8_TF = 5000.0          # dense e4m3 on the block-scaled MFMA (2x bf16 per clock)


def _mode(engine, mode):
    return engine.experimental_math(mode) if mode == 'mxfp8' else engine.math_mode(mode)


def series(engine, cnn, siam, clips, mode, steps, warmup):
    with _mode(engine, mode), torch.no_grad():
        for _ in range(warmup):
            engine.extract_features(cnn, siam, clips)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            engine.extract_features(cnn, siam, clips)
        e1.record()
        torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    return dict(mode=mode, ms_per_step=round(ms, 3), clips_per_s=round(clips.shape[0] / ms * 1e3, 1))


def deviation(engine, cnn, clips):
    out = {}
    with torch.no_grad():
        with engine.math_mode('f32'):
            ref = engine._grl_eval(cnn, clips)
            ref = (ref[0].clone(), ref[1].clone())
        for mode in ('bf16s', 'mxfp8'):
            with _mode(engine, mode):
                got = engine._grl_eval(cnn, clips)
            for name, r, g in (('x_uncorr', ref[0], got[0]), ('x_corr', ref[1], got[1])):
                r2, g2 = r.reshape(-1, 2048).double(), g.reshape(-1, 2048).double()
                cos = torch.nn.functional.cosine_similarity(r2, g2, dim=1).min().item()
                rl = ((g2 - r2).norm() / r2.norm()).item()
                out['%s.%s' % (mode, name)] = dict(min_cos=round(cos, 6), rel_l2=float('%.4e' % rl))
    return out


def gemm_rates(engine, lib_mod, dev, iters=20):
    from grl_amd import _lib
    res = []
    shapes = [   # (name, M, N, K, conv)    configs[2]: 512 frames, layer 3 = 16 x 8, layer 4 = 16 x 8 (stride 1 in GRL)
        ('layer3 3x3 256->256', 512 * 128, 256, 9 * 256, (16, 8, 256, 16, 8, 3, 3, 1, 1)),
        ('layer3 1x1 1024->256', 512 * 128, 256, 1024, None),
        ('layer4 1x1 2048->512', 512 * 128, 512, 2048, None),
        ('layer4 1x1 512->2048', 512 * 128, 2048, 512, None),
        ('TRL memo 2048x2048', 64 * 128, 2048, 2048, None),
    ]
    for name, M, N, K, conv in shapes:
        rows = M if conv is None else M // (conv[3] * conv[4]) * conv[0] * conv[1]
        ka = K if conv is None else conv[2]
        a = (torch.randn(rows, ka, device=dev) * 0.5).to(torch.bfloat16)
        w32 = torch.randn(N, K, device=dev) / K ** 0.5
        wb = w32.to(torch.bfloat16)
        lib = _lib.load()
        wmx = torch.empty(lib.grl_mx_image_bytes(N, K), dtype=torch.uint8, device=dev)
        _lib.check(lib.grl_mx_pack_weights(_lib.ptr(w32), N, K, K, _lib.ptr(wmx), _lib.stream()), 'pack')
        y = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        sc, sh = torch.ones(N, device=dev), torch.zeros(N, device=dev)
        qimg = torch.empty(lib.grl_mx_image_bytes(rows, ka), dtype=torch.uint8, device=dev)
        row = dict(shape=name, M=M, N=N, K=K)
        for tag, w, m in (('bf16s', wb, engine.MATH_BF16S), ('mxfp8', wmx, engine.MATH_MXFP8)):
            def run():
                engine.gemm(a, w, y, M, N, K, scale=sc, shift=sh, relu=True, conv=conv, math=m)
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                run()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / iters * 1e3
            tf = 2.0 * M * N * K / (us * 1e-6) / 1e12
            peak = PEAK_MXFP8_TF if tag == 'mxfp8' else PEAK_BF16_TF
            row[tag] = dict(us=round(us, 1), tflops=round(tf, 1), of_peak=round(tf / peak, 3))
        # the activation-quantisation pass alone
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            _lib.check(lib.grl_mx_quantize_rows(_lib.ptr(a), rows, ka, ka, _lib.ptr(qimg), _lib.stream()), 'quant')
        e1.record()
        torch.cuda.synchronize()
        row['mxfp8']['quant_us'] = round(e0.elapsed_time(e1) / iters * 1e3, 1)
        res.append(row)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=15)
    ap.add_argument('--json', default=None)
    ap.add_argument('--no-pipeline', action='store_true', help='GEMM shapes only')
    args = ap.parse_args()
    from bench import build_models
    from grl_amd import engine, _lib
    from grl_amd.synthetic import synth_clips
    dev = torch.device('cuda:0')
    _lib.load()
    cnn, siam, _, _ = build_models(dev)
    out = dict(steps=args.steps, warmup=args.warmup)
    if not args.no_pipeline:
        c2 = synth_clips(64, 8, seed=1).to(dev)
        runs = []
        for _ in range(3):
            for mode in ('bf16s', 'mxfp8'):
                r = series(engine, cnn, siam, c2, mode, args.steps, args.warmup)
                runs.append(r)
                print('configs[2] 64x8 %-6s %8.3f ms/step %9.1f clips/s' % (mode, r['ms_per_step'], r['clips_per_s']), flush=True)
        out['configs2'] = runs
        b = [r['ms_per_step'] for r in runs if r['mode'] == 'bf16s']
        m = [r['ms_per_step'] for r in runs if r['mode'] == 'mxfp8']
        out['configs2_speedup_mxfp8_over_bf16s'] = round(sorted(b)[1] / sorted(m)[1], 3)
        print('configs[2] median speedup mxfp8 / bf16s: %.3f' % out['configs2_speedup_mxfp8_over_bf16s'])
        out['configs2_deviation_vs_f32'] = deviation(engine, cnn, synth_clips(16, 8, seed=3).to(dev))
        del c2
        c1 = synth_clips(32, 4, seed=1).to(dev)
        runs = [series(engine, cnn, siam, c1, mode, args.steps, args.warmup) for mode in ('f32', 'mxfp8')]
        for r in runs:
            print('configs[1] 32x4 %-6s %8.3f ms/step %9.1f clips/s' % (r['mode'], r['ms_per_step'], r['clips_per_s']))
        out['configs1'] = runs
        out['configs1_deviation_vs_f32'] = deviation(engine, cnn, c1)
        print(json.dumps(out['configs2_deviation_vs_f32']))
        print(json.dumps(out['configs1_deviation_vs_f32']))
    out['gemm'] = gemm_rates(engine, _lib, dev)
    for r in out['gemm']:
        print('%-22s M %6d N %5d K %5d | bf16s %7.1f us %6.1f TF (%.3f) | mxfp8 %7.1f us %6.1f TF (%.3f), quant %6.1f us' % (
            r['shape'], r['M'], r['N'], r['K'], r['bf16s']['us'], r['bf16s']['tflops'], r['bf16s']['of_peak'],
            r['mxfp8']['us'], r['mxfp8']['tflops'], r['mxfp8']['of_peak'], r['mxfp8']['quant_us']))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)
    print(json.dumps(dict(configs2_speedup=out.get('configs2_speedup_mxfp8_over_bf16s'))))


if __name__ == '__main__':
    main()
