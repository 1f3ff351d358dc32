#!/usr/bin/env python
"""Times engine.cluster_jaccard at the MARS shape (13290 samples x 6144: the query-prepended gallery) on unit-norm
synthetic rows with planted identities, k1 = 20, k2 = 6, eps 0.5 and 0.6, min_samples 1 and 4.  Reported:
the total; the front half (passes A1 and A2 over the distance GEMM, the lists, the expansion, the transpose:
``engine._JaccardSet``); grl_jaccard_edges' count and fill launches alone on the finished state; cluster_from_graph
alone with its component rounds; E, nnz(V2), the longest and the median CSC column; the pair scores against the planted
ids next to engine.cluster's on the same input at its ``PairRoc.eer_threshold``.  The floor of the front half is the
two bare passes over the 'euclidean' ``_ColumnBlocks`` (code that existed before); engine.cluster on the same input is
the neighbouring feature.  One process, the functions in turn: warm-ups, then the median of the timed launches (HIP
events; the discipline of tools/verify_rate.py).

  python tools/jaccard_rate.py [--warm 15] [--reps 20] [--n 13290] [--json PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from verify_rate import in_turn  # noqa: E402

K1, K2 = 20, 6
EPS = (0.5, 0.6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warm', type=int, default=15)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--n', type=int, default=13290)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    from grl_amd import engine
    from grl_amd.synthetic import synth_eval_features
    dev = torch.device('cuda:0')
    n, nq = a.n, min(1980, a.n)
    qf, gf, qp, qc, gp, gc = synth_eval_features(nq, n, seed=1)
    scale = 1.0 / float(np.sqrt(3.0))                      # three unit blocks per row -> unit rows
    qf, gf = (qf * scale).to(dev), (gf * scale).to(dev)
    res = {'n': n, 'd': gf.shape[1], 'k1': K1, 'k2': K2, 'warm': a.warm, 'reps': a.reps,
           'device': torch.cuda.get_device_name(0)}
    st = engine._JaccardSet(gf, K1, K2)
    blocks = engine._ColumnBlocks(gf, gf, 'euclidean', block_cols=st.width)
    csc_len = (st.csc_ptr[1:] - st.csc_ptr[:-1])
    row_len = (st.row_ptr[1:] - st.row_ptr[:-1])
    res.update({'sample_block': st.width, 'blocks': len(blocks.spans), 'nnz_v2': st.nnz,
                'v2_row_max': int(row_len.max()), 'v2_row_mean': float(row_len.float().mean()),
                'csc_col_max': int(csc_len.max()), 'csc_col_median': float(csc_len.float().median())})

    def two_passes():
        for _ in range(2):
            for c0, c1 in blocks.spans:
                blocks.block(c0, c1)
    graphs = {eps: st.graph(eps) for eps in EPS}
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    cols = {eps: torch.empty_like(graphs[eps][1]) for eps in EPS}
    fns = {'two_block_passes': two_passes, 'front_half': lambda: engine._JaccardSet(gf, K1, K2)}
    for eps in EPS:
        fns['jaccard_graph/eps%g' % eps] = lambda eps=eps: engine.jaccard_graph(gf, eps, K1, K2)
        fns['edges_count/eps%g' % eps] = lambda eps=eps: st._edges(eps, 0, cnt, None, None, None)
        fns['edges_fill/eps%g' % eps] = lambda eps=eps: st._edges(eps, 0, None, graphs[eps][0], cols[eps], None)
        for m in (1, 4):
            fns['cluster_jaccard/eps%g/m%d' % (eps, m)] = lambda eps=eps, m=m: engine.cluster_jaccard(gf, eps, m, K1, K2)
            fns['cluster_from_graph/eps%g/m%d' % (eps, m)] = lambda eps=eps, m=m: engine.cluster_from_graph(
                graphs[eps][0], graphs[eps][1], n, m, _checked=True)
    res['ms'] = ms = in_turn(fns, a.warm, a.reps)
    for eps in EPS:
        assert torch.equal(cols[eps], graphs[eps][1])
        edges = ms['edges_count/eps%g' % eps][0] + ms['edges_fill/eps%g' % eps][0]
        res['edges_share/eps%g' % eps] = edges / ms['jaccard_graph/eps%g' % eps][0]
        res['edges_over_front_half/eps%g' % eps] = edges / ms['front_half'][0]
        for m in (1, 4):
            cl = engine.cluster_jaccard(gf, eps, m, K1, K2)
            res['result/eps%g/m%d' % (eps, m)] = {'n_clusters': cl.n_clusters, 'n_noise': cl.n_noise,
                                                 'n_edges': cl.n_edges, 'rounds': cl.rounds,
                                                 'pair_scores': cl.pair_scores(gp)}
    # the neighbouring feature on the same input: DBSCAN on the cosine eps-graph at the equal-error threshold
    roc = engine.pair_roc(qf, gf, qp, gp, qc, gc)
    ceps = float(roc.eer_threshold)
    res['cosine'] = {'eps': ceps, 'eer': roc.eer,
                     'ms': in_turn({'cluster/m%d' % m: (lambda m=m: engine.cluster(gf, ceps, m)) for m in (1, 4)},
                                   a.warm, a.reps)}
    for m in (1, 4):
        cl = engine.cluster(gf, ceps, m)
        res['cosine']['result/m%d' % m] = {'n_clusters': cl.n_clusters, 'n_noise': cl.n_noise, 'n_edges': cl.n_edges,
                                           'rounds': cl.rounds, 'pair_scores': cl.pair_scores(gp)}
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
