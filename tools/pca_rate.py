#!/usr/bin/env python
"""Times engine.pca at the MARS shape (13290 samples x 6144: the query-prepended gallery) on the unit-norm synthetic
rows with planted identities of DESIGN.md 4w (the input of tools/tsne_rate.py), for r = 128 and 256 components (L = r +
10).  Split into its parts, each a stage of the fit on the buffers a fit ends with: the GEMM passes (``project`` = X Q^T
with its shift and transpose, ``back`` = the weight-gradient GEMM with its rank-one term), the orthonormalisations
(CholeskyQR2 of the [L, d] and of the [L, n] matrix: Gram GEMM, grl_pca_cholesky, grl_pca_trsm, twice), the Rayleigh-Ritz
matrix, the Jacobi eigensolve, the components GEMM; then the whole fit and one transform of all rows.  The floor is the
bare GEMM of the fit's shape measured in the same process: ``engine.gemm`` [n, L] = X Q^T without epilogue, times the
2 q + 1 tall products a fit with q power iterations makes (code that existed before).  One process, the functions in
turn: 15 warm-ups, then 20 timed runs each (HIP events; the discipline of tools/verify_rate.py), medians.  ``--host 1``
adds the off-the-shelf route: download the features, scikit-learn's PCA(svd_solver='randomized') with the same
oversampling and iterations on 16 threads (one run, wall clock).

  python tools/pca_rate.py [--warm 15] [--reps 20] [--n 13290] [--r 128,256] [--iters 4] [--host 0] [--json PATH]
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
    ap.add_argument('--r', default='128,256')
    ap.add_argument('--iters', type=int, default=4)
    ap.add_argument('--host', type=int, default=0)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    from grl_amd import engine
    from grl_amd.synthetic import synth_eval_features
    dev = torch.device('cuda:0')
    n, nq = a.n, min(1980, a.n)
    qf, gf, qp, qc, gp, gc = synth_eval_features(nq, n, seed=1)
    gf = (gf * (1.0 / float(np.sqrt(3.0)))).to(dev)        # three unit blocks per row -> unit rows
    d = gf.shape[1]
    res = {'n': n, 'd': d, 'warm': a.warm, 'reps': a.reps, 'device': torch.cuda.get_device_name(0), 'iters': a.iters,
           'fits': []}
    for r in [int(v) for v in a.r.split(',')]:
        L = r + 10
        fit = engine.pca(gf, r, n_iter=a.iters)
        one = {'r': r, 'L': L, 'sweeps': fit.sweeps, 'min_pivot': fit.min_pivot, 'off': fit.off,
               'explained_variance_ratio_sum': float(fit.explained_variance_ratio.double().sum()),
               'lambda_1': float(fit.explained_variance[0]), 'lambda_r': float(fit.explained_variance[-1])}
        st = engine._PcaFit(engine._pad_features(gf), n, d, L, dev)     # a fit's buffers, left in the state a fit ends with
        st.mean()
        q0 = np.random.Generator(np.random.PCG64(0)).standard_normal((L, d)).astype(np.float32)
        st.q[:L, :d] = torch.from_numpy(q0).to(dev)
        st.orth_q()
        st.project()
        b = st.ritz_matrix()
        bare = torch.empty((n, st.L4), dtype=torch.float32, device=dev)

        def eigh():
            return st.eigh(b.clone())
        vt = eigh()[1]
        fns = {'gemm_floor': lambda: engine.gemm(st.xp, st.q, bare, n, st.L4, st.dp, math=engine.MATH_F32),
               'mean': st.mean, 'project': st.project, 'back': st.back, 'orth_q': st.orth_q, 'orth_z': st.orth_z,
               'ritz_matrix': st.ritz_matrix, 'clone': lambda: b.clone(), 'eigh': eigh,
               'components': lambda: st.components(vt, r), 'sums': st.sums,
               'fit': lambda: engine.pca(gf, r, n_iter=a.iters),
               'transform': lambda: fit.transform(gf), 'transform_whiten': lambda: fit.transform(gf, True)}
        one['ms'] = in_turn(fns, a.warm, a.reps)
        ms = {k: v[0] for k, v in one['ms'].items()}
        q = a.iters
        one['gemm_passes_ms'] = (q + 1) * ms['project'] + q * ms['back']
        one['orthonormalisations_ms'] = (q + 1) * ms['orth_q'] + q * ms['orth_z']
        one['eigensolve_ms'] = ms['eigh'] - ms['clone']
        one['floor_ms'] = (2 * q + 1) * ms['gemm_floor']
        one['fit_over_floor'] = ms['fit'] / one['floor_ms']
        if a.host:
            from sklearn.decomposition import PCA
            from threadpoolctl import threadpool_limits
            t0 = time.perf_counter()
            xh = gf.cpu().numpy()
            t1 = time.perf_counter()
            with threadpool_limits(limits=16):
                sk = PCA(n_components=r, svd_solver='randomized', n_oversamples=10, iterated_power=a.iters,
                         power_iteration_normalizer='QR', random_state=0).fit(xh)
            t2 = time.perf_counter()
            lam = fit.explained_variance.cpu().numpy().astype(np.float64)
            one['host'] = {'download_ms': (t1 - t0) * 1e3, 'sklearn_ms': (t2 - t1) * 1e3,
                           'max_rel_eigenvalue_difference': float(np.abs(lam - sk.explained_variance_).max() / lam[0])}
        res['fits'].append(one)
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
