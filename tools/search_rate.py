#!/usr/bin/env python
"""Times the streaming evaluator (engine.rank_metrics_streaming) and gallery search (engine.search) against the
materialised path (cosin_dist + rank_rows + rank_metrics), in one process, with warm-ups:

  1. MARS size (1980 x 13290 x 6144): materialised vs streaming (default block = one pass; block_cols=2048);
  2. search(k=100) alone at MARS size, without and with the junk filter (exclude=);
  3. a large synthetic case (default 10^4 x 10^6 x 256, random unit rows on the device), run only where the
     materialised path would need more than the block budget: streaming metrics and search(k=100), with the
     peak torch.cuda.max_memory_allocated over the inputs.

  python tools/search_rate.py [--reps N] [--large NQ NG DIM] [--no-large] [--json PATH]
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


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def peak_over_inputs(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--large', type=int, nargs=3, default=[10000, 1000000, 256], metavar=('NQ', 'NG', 'DIM'))
    ap.add_argument('--no-large', action='store_true')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    from grl_amd import engine
    from grl_amd.synthetic import synth_eval_features
    dev = torch.device('cuda:0')

    def quiet():
        return contextlib.redirect_stdout(io.StringIO())
    res = {'block_bytes': engine.SEARCH_BLOCK_BYTES}

    qf, gf, qp, qc, gp, gc = synth_eval_features(1980, 13290, seed=1)
    qf, gf = qf.to(dev), gf.to(dev)

    def materialised():
        return engine.rank_metrics(engine.rank_rows(engine.cosin_dist(qf, gf)), qp, gp, qc, gc)

    def streaming(w=None):
        return lambda: engine.rank_metrics_streaming(qf, gf, qp, gp, qc, gc, block_cols=w)
    with quiet():
        r_mat, r_str = materialised(), streaming()()
    assert np.array_equal(r_mat[0], r_str[0]) and abs(r_mat[1] - r_str[1]) <= 1e-12
    with quiet():
        res['mars_materialised_ms'] = timed(materialised, a.reps)
        res['mars_streaming_ms'] = timed(streaming(), a.reps)
        res['mars_streaming_2048_ms'] = timed(streaming(2048), a.reps)
        res['mars_cosin_dist_ms'] = timed(lambda: engine.cosin_dist(qf, gf), a.reps)
        res['mars_search_k100_ms'] = timed(lambda: engine.search(qf, gf, 100), a.reps)
        res['mars_search_k100_2048_ms'] = timed(lambda: engine.search(qf, gf, 100, block_cols=2048), a.reps)
        ex = (qp, gp, qc, gc)                 # junk-filtered lists (same pid AND camera dropped), same process
        res['mars_search_k100_exclude_ms'] = timed(lambda: engine.search(qf, gf, 100, exclude=ex), a.reps)
        res['mars_search_k100_2048_exclude_ms'] = timed(
            lambda: engine.search(qf, gf, 100, exclude=ex, block_cols=2048), a.reps)
        res['mars_peak_materialised_bytes'] = peak_over_inputs(materialised)
        res['mars_peak_streaming_bytes'] = peak_over_inputs(streaming())
        res['mars_peak_streaming_2048_bytes'] = peak_over_inputs(streaming(2048))
    res['mars_ratio_streaming_over_materialised'] = res['mars_streaming_ms'][0] / res['mars_materialised_ms'][0]
    del qf, gf

    nq, ng, dim = a.large
    need = nq * ng * 8                                    # distance matrix + int32 argsort of the materialised path
    if not a.no_large and need > engine.SEARCH_BLOCK_BYTES:
        g = torch.Generator(device=dev).manual_seed(7)
        gf = torch.randn((ng, dim), device=dev, generator=g)
        gf /= gf.norm(dim=1, keepdim=True)
        qf = gf[:nq].clone()
        rng = np.random.Generator(np.random.PCG64(7))
        gp = rng.integers(0, max(1, ng // 500), ng); gc = rng.integers(0, 6, ng)
        qp, qc = gp[:nq].copy(), gc[:nq].copy()
        torch.cuda.synchronize()
        with quiet():
            res['large_shape'] = [nq, ng, dim]
            res['large_materialised_would_need_bytes'] = need
            res['large_streaming_ms'] = timed(lambda: engine.rank_metrics_streaming(qf, gf, qp, gp, qc, gc),
                                              max(1, a.reps // 5), warm=1)
            res['large_search_k100_ms'] = timed(lambda: engine.search(qf, gf, 100), max(1, a.reps // 5), warm=1)
            res['large_peak_streaming_bytes'] = peak_over_inputs(
                lambda: engine.rank_metrics_streaming(qf, gf, qp, gp, qc, gc))
            res['large_peak_search_bytes'] = peak_over_inputs(lambda: engine.search(qf, gf, 100))
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
