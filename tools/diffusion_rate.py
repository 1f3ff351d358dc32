#!/usr/bin/env python
"""Times engine.diffusion_search at the MARS shape (13290 x 6144 query-prepended gallery, 1980 queries) on unit-norm
synthetic rows with planted identities, at the defaults (k = 50, kq = 10, gamma = 3, alpha = 0.99, n_iter = 20), split
into its parts: the two bare ``search`` passes (gallery x gallery for the lists, queries x gallery for the seeds: the
floor, code that existed before diffusion), grl_diffusion_mutual alone, the whole graph build, one grl_diffusion_apply,
the whole solve of one query block (seed scatter, 20 CG iterations, transpose), and the total with and without a
prebuilt graph.  For the product the achieved GB/s is reported against its algorithmic bytes twice: the compulsory
traffic (p read once, Ap written once, idx and S read once) and the gathered bytes (one neighbour row per non-zero slot,
which the caches serve).  One process, the functions in turn: 15 warm-ups, then 20 timed launches each (HIP events; the
discipline of tools/verify_rate.py); medians.

With ``--host N`` scipy's sparse conjugate gradients solve N of the columns on the host for comparison (same matrix, 20
iterations, float64), when scipy imports.

  python tools/diffusion_rate.py [--warm 15] [--reps 20] [--host 0] [--n 13290] [--nq 1980] [--json PATH]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from verify_rate import in_turn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warm', type=int, default=15)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host', type=int, default=0)
    ap.add_argument('--n', type=int, default=13290)
    ap.add_argument('--nq', type=int, default=1980)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    from grl_amd import _lib, engine
    from grl_amd._lib import ptr
    from grl_amd.synthetic import synth_eval_features
    dev = torch.device('cuda:0')
    n, nq, k, kq, gamma, alpha, n_iter = a.n, min(a.nq, a.n), 50, 10, 3, 0.99, 20
    qf, gf, qp, qc, gp, gc = synth_eval_features(nq, n, seed=1)
    scale = 1.0 / float(np.sqrt(3.0))                        # three unit blocks per row -> unit rows
    qf, gf = (qf * scale).to(dev), (gf * scale).to(dev)
    d = gf.shape[1]
    B = engine._diffusion_query_block(None, None, n, nq, 5, 'diffusion_rate')
    res = {'n': n, 'nq': nq, 'd': d, 'k': k, 'kq': kq, 'gamma': gamma, 'alpha': alpha, 'n_iter': n_iter, 'query_block': B,
           'warm': a.warm, 'reps': a.reps, 'device': torch.cuda.get_device_name(0)}
    graph = engine.diffusion_graph(gf, k, gamma)
    res['graph'] = {'n_edges': graph.n_edges, 'n_isolated': graph.n_isolated, 'slots': n * k}
    sdist, sidx = engine.search(gf, gf, k + 1)
    qdist, qidx = engine.search(qf, gf, kq)
    bi, bd = qidx[:B].contiguous(), qdist[:B].contiguous()
    idx = torch.empty((n, k), dtype=torch.int32, device=dev)
    w = torch.empty((n, k), dtype=torch.float32, device=dev)
    deg = torch.empty((n,), dtype=torch.float32, device=dev)
    p = torch.randn((n, B), device=dev)
    Ap = torch.empty_like(p)
    part = torch.empty((-(-n // _lib.load().grl_diffusion_part_rows()), B), dtype=torch.float32, device=dev)
    fns = {'search/gallery_x_gallery': lambda: engine.search(gf, gf, k + 1),
           'search/queries_x_gallery': lambda: engine.search(qf, gf, kq),
           'mutual': lambda: engine._call('grl_diffusion_mutual', ptr(sidx), ptr(sdist), k + 1, n, k, gamma, ptr(idx), ptr(w),
                                          k, ptr(deg)),
           'graph': lambda: engine.diffusion_graph(gf, k, gamma),
           'apply': lambda: engine._call('grl_diffusion_apply', ptr(graph.idx), ptr(graph.weight), k, n, k, ptr(p), B, alpha,
                                         ptr(Ap), ptr(part)),
           'solve_block': lambda: engine._diffusion_block(graph, bi, bd, gamma, alpha, n_iter, True),
           'total/prebuilt_graph': lambda: engine.diffusion_search(qf, gf, 100, graph=graph),
           'total': lambda: engine.diffusion_search(qf, gf, 100),
           'metrics/prebuilt_graph': lambda: engine.diffusion_metrics_streaming(qf, gf, qp, gp, qc, gc, graph=graph)}
    res['ms'] = in_turn(fns, a.warm, a.reps)
    t_apply = res['ms']['apply'][0] * 1e-3
    res['apply_compulsory_gbps'] = (2 * n * B * 4 + n * k * 8) / t_apply / 1e9
    res['apply_gathered_gbps'] = (graph.n_edges + 2 * n) * B * 4 / t_apply / 1e9
    res['floor_ms'] = res['ms']['search/gallery_x_gallery'][0] + res['ms']['search/queries_x_gallery'][0]
    res['blocks'] = -(-nq // B)
    res['map'] = {'diffusion': engine.diffusion_metrics_streaming(qf, gf, qp, gp, qc, gc, graph=graph)[1],
                  'cosine': engine.rank_metrics_streaming(qf, gf, qp, gp, qc, gc)[1]}
    if a.host:
        try:
            import scipy.sparse as sp
            import scipy.sparse.linalg as spl
        except ImportError:
            res['host'] = 'scipy does not import'
        else:
            cols = min(a.host, B)
            gi, gw = graph.idx.cpu().numpy(), graph.weight.cpu().numpy().astype(np.float64)
            rows = np.repeat(np.arange(n), k)
            keep = gw.reshape(-1) != 0
            S = sp.csr_matrix((gw.reshape(-1)[keep], (rows[keep], gi.reshape(-1)[keep])), shape=(n, n))
            A = sp.identity(n, format='csr') - alpha * S
            y = np.zeros((n, cols))
            hi, hd = bi.cpu().numpy(), bd.cpu().numpy()
            for q in range(cols):
                y[hi[q], q] = np.maximum(-hd[q].astype(np.float64), 0) ** gamma
            t0 = time.perf_counter()
            for q in range(cols):
                spl.cg(A, y[:, q], maxiter=n_iter)
            dt = time.perf_counter() - t0
            res['host'] = {'columns': cols, 'cg_s': dt, 'ms_per_column': dt / cols * 1e3}
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
