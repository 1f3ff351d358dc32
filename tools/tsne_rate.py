#!/usr/bin/env python
"""Times engine.tsne at the MARS shape (13290 samples x 6144: the query-prepended gallery) on unit-norm synthetic rows
with planted identities (the input of tools/hdbscan_rate.py).  Split into its parts: one bare pass over the
``_ColumnBlocks`` of cosin_dist(x, x) (the GEMM floor: code that existed before) against the affinity stage
(engine.tsne_affinities: that pass with the top-k lists, the perplexity search, the transpose and the CSR); one
iteration of the loop and each of its three kernels alone (grl_tsne_repulsion: the n (n - 1) pair terms per second are
reported; grl_tsne_z; grl_tsne_update) at the coordinates a run ends with; the loop of ``--iters`` iterations on given
affinities; and the whole call.  One process, the functions in turn: 15 warm-ups, then 20 timed runs each (HIP events;
the discipline of tools/verify_rate.py), medians.  ``--host 1`` adds the off-the-shelf route for comparison: download
the features, scikit-learn's Barnes-Hut TSNE(metric='cosine', init='random') with the same perplexity and iterations
(one run, wall clock), and the 5-neighbour trustworthiness of both maps on a sample of the rows.

  python tools/tsne_rate.py [--warm 15] [--reps 20] [--n 13290] [--perplexity 30] [--iters 1000] [--host 0] [--json PATH]
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
    ap.add_argument('--n', type=int, default=13290)
    ap.add_argument('--perplexity', type=float, default=30.0)
    ap.add_argument('--iters', type=int, default=1000)
    ap.add_argument('--host', type=int, default=0)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    from grl_amd import engine
    from grl_amd._lib import ptr
    from grl_amd.synthetic import synth_eval_features
    dev = torch.device('cuda:0')
    n, nq = a.n, min(1980, a.n)
    qf, gf, qp, qc, gp, gc = synth_eval_features(nq, n, seed=1)
    gf = (gf * (1.0 / float(np.sqrt(3.0)))).to(dev)        # three unit blocks per row -> unit rows
    ts = engine.tsne(gf, a.perplexity, n_iter=a.iters)
    row_ptr, col, val = ts.affinities
    res = {'n': n, 'd': gf.shape[1], 'warm': a.warm, 'reps': a.reps, 'device': torch.cuda.get_device_name(0),
           'perplexity': a.perplexity, 'iters': a.iters, 'K': min(n - 1, int(3 * a.perplexity) + 1),
           'entries': int(col.numel()), 'longest_row': int((row_ptr[1:] - row_ptr[:-1]).max()), 'kl': ts.kl,
           'n_isolated': ts.n_isolated, 'learning_rate': ts.learning_rate}
    blocks = engine._ColumnBlocks(gf, gf, 'cosine')
    res['blocks'] = len(blocks.spans)

    def block_pass():
        for c0, c1 in blocks.spans:
            blocks.block(c0, c1)
    y = ts.embedding.contiguous()
    y2, rep, grad = torch.empty_like(y), torch.empty_like(y), torch.empty_like(y)
    gains, update = torch.ones_like(y), torch.zeros_like(y)
    rowz = torch.empty(n, dtype=torch.float32, device=dev)
    z = torch.empty(1, dtype=torch.float32, device=dev)
    csr = (ptr(row_ptr), ptr(col), ptr(val))

    def repulsion():
        engine._call('grl_tsne_repulsion', ptr(y), None, n, ptr(rep), ptr(rowz))

    def fold_z():
        engine._call('grl_tsne_z', ptr(rowz), n, ptr(z))

    def step():                                             # (learning rate 0: the state it reads stays what it is)
        engine._call('grl_tsne_update', *csr, ptr(y), None, n, 1.0, ptr(rep), ptr(z), None, ptr(gains), ptr(update),
                     ptr(y2), 0.8, 0.0)

    def iteration():
        repulsion()
        fold_z()
        step()
    fns = {'block_pass': block_pass,
           'affinities': lambda: engine.tsne_affinities(gf, a.perplexity),
           'repulsion': repulsion, 'z': fold_z, 'update': step, 'iteration': iteration,
           'gradient': lambda: engine.tsne_gradient(row_ptr, col, val, y),
           'loop': lambda: engine.tsne_from_affinities(row_ptr, col, val, a.iters),
           'tsne': lambda: engine.tsne(gf, a.perplexity, n_iter=a.iters)}
    res['ms'] = in_turn(fns, a.warm, a.reps)
    ms = {k: v[0] for k, v in res['ms'].items()}
    res['affinities_over_floor'] = ms['affinities'] / ms['block_pass']
    res['pair_terms_per_s'] = n * (n - 1) / (ms['repulsion'] * 1e-3)
    res['loop_ms_per_iteration'] = ms['loop'] / a.iters
    res['kernels_sum_ms'] = ms['repulsion'] + ms['z'] + ms['update']
    if a.host:
        from sklearn.manifold import TSNE, trustworthiness
        t0 = time.perf_counter()
        x = gf.cpu().numpy()
        t1 = time.perf_counter()
        sk = TSNE(method='barnes_hut', metric='cosine', init='random', perplexity=a.perplexity, max_iter=a.iters,
                  random_state=0).fit(x)
        t2 = time.perf_counter()
        rows = np.random.Generator(np.random.PCG64(0)).choice(n, min(n, 3000), replace=False)
        emb = ts.embedding.cpu().numpy()
        res['host'] = {'download_ms': (t1 - t0) * 1e3, 'sklearn_ms': (t2 - t1) * 1e3, 'kl': float(sk.kl_divergence_),
                       'trustworthiness_rows': int(rows.size),
                       'trustworthiness_sklearn': float(trustworthiness(x[rows], sk.embedding_[rows], n_neighbors=5, metric='cosine')),
                       'trustworthiness_device': float(trustworthiness(x[rows], emb[rows], n_neighbors=5, metric='cosine'))}
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
