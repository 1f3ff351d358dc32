"""Ranking by the Siamese verification head on the device (engine.verify_metric / verify_dist, verify.hip) against the
float64 host model of tests/verify_ref.py, the existing per-pair head kernel, and the materialised ranking path."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import verify_ref as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda:0')
NQ, NG = 5, 300
REAL = (6144, 2048, 2048)                   # d, head width, col0: rows [x_uncorr | out_frame | mean]
SMALL = (192, 64, 64)                       # Siamese(input_num=64): the GEMM takes K = 192 and K = 64
BETAS = (1.0, 0.35)
WIDTHS = (128, 37, None)                    # 128: 3 blocks, ragged last (44); 37: 9 blocks whose rows are unaligned


def make_siam(D, seed, out=16):
    """A Siamese whose verification head holds verify_ref.make_head(D, seed); the rest keeps its initialisation."""
    from grl_amd.reid.models.Siamese import Siamese
    torch.manual_seed(seed)
    siam = Siamese(D, out, 2)
    head = V.make_head(D, seed)
    with torch.no_grad():
        siam.classifierBN.weight.copy_(torch.from_numpy(head['gamma']))
        siam.classifierBN.bias.copy_(torch.from_numpy(head['beta']))
        siam.classifierBN.running_mean.copy_(torch.from_numpy(head['mean']))
        siam.classifierBN.running_var.copy_(torch.from_numpy(head['var']))
        siam.classifierlinear.weight.copy_(torch.from_numpy(head['W']))
        siam.classifierlinear.bias.copy_(torch.from_numpy(head['b']))
    assert siam.classifierBN.eps == head['eps']
    return siam.to(DEV).eval(), head


_cases = {}


def case(shape):
    """(siam, head, qf, gf as numpy, qf, gf on the device, w, c) for a (d, D, col0); built once, never modified."""
    if shape not in _cases:
        d, D, col0 = shape
        siam, head = make_siam(D, seed=D)
        q, g = V.features(NQ, NG, d, col0, D, seed=7)
        w, c = V.fold(head)
        _cases[shape] = (siam, head, q, g, torch.from_numpy(q).to(DEV), torch.from_numpy(g).to(DEV), w, c)
    return _cases[shape]


_dists = {}


def dist_of(shape, beta):
    """verify_dist of a case, computed once (the tests below compare everything else with it)."""
    from grl_amd import engine
    if (shape, beta) not in _dists:
        siam, head, q, g, qf, gf, w, c = case(shape)
        vm = engine.verify_metric(siam, shape[2], beta)
        _dists[(shape, beta)] = (vm, engine.verify_dist(qf, gf, vm).clone())
    return _dists[(shape, beta)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ids():
    """pids / cameras with junk entries (same pid and camera as the query) and one query without any match."""
    g = np.random.Generator(np.random.PCG64(11))
    gp, gc = g.integers(0, 4, NG), g.integers(0, 3, NG)
    qp, qc = np.array([0, 1, 2, 3, 99]), np.array([0, 1, 2, 0, 1])
    assert all(((gp == p) & (gc == c)).any() and ((gp == p) & (gc != c)).any() for p, c in zip(qp[:4], qc[:4]))
    return qp, gp, qc, gc


# ----------------------------------------------------------------------------
# 1. the fold
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [REAL, SMALL])
def test_fold_kernel_equals_the_float64_fold(shape):
    from grl_amd import engine
    siam, head, w, c = case(shape)[0], case(shape)[1], case(shape)[6], case(shape)[7]
    plan = engine._plan(siam, engine.VerifyFoldPlan)
    assert plan.w.dtype == torch.float32 and plan.c64.dtype == torch.float64 and plan.c32.dtype == torch.float32
    assert np.array_equal(plan.w.cpu().numpy().view(np.int32), w.astype(np.float32).view(np.int32))
    c_dev = float(plan.c64.item())
    print('c: device %.17g host %.17g relative difference %.3e' % (c_dev, c, abs(c_dev - c) / abs(c)))
    assert abs(c_dev - c) <= 1e-12 * abs(c)
    assert plan.c32.item() == np.float32(c_dev)
    assert engine._plan(siam, engine.VerifyFoldPlan) is plan                    # cached ...


def test_a_weight_update_refolds():
    from grl_amd import engine
    siam, head = make_siam(64, seed=5)
    vm = engine.verify_metric(siam, 0)
    w0 = vm.folded()[0].clone()
    with torch.no_grad():
        siam.classifierlinear.weight.mul_(2.0)
    assert torch.equal(vm.folded()[0], w0 * 2.0)                                # (a power of two: exact)
    with torch.no_grad():
        siam.classifierBN.running_var.mul_(1.5)                                 # a buffer, as a train-mode forward moves it
    head['W'] = head['W'] * 2.0
    head['var'] = siam.classifierBN.running_var.cpu().numpy()
    assert np.array_equal(vm.folded()[0].cpu().numpy(), V.fold(head)[0].astype(np.float32))


# ----------------------------------------------------------------------------
# 2. verify_dist against the head taken literally, in float64
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('beta', BETAS)
@pytest.mark.parametrize('shape', [REAL, SMALL])
def test_verify_dist_is_the_literal_head_within_the_fp32_bound(shape, beta):
    """Tolerance per entry: verify_ref.error_bound, the worst case of a K-term fp32 fma chain plus the three scalar
    operations, 2 (K + 8) 2^-24 (sum_d |q'_d g_d| + |rq| + |rg|), evaluated in float64 for that entry."""
    siam, head, q, g, qf, gf, w, c = case(shape)
    vm, D = dist_of(shape, beta)
    assert tuple(D.shape) == (NQ, NG) and D.dtype == torch.float32
    want = V.literal_F(q, g, shape[2], head, beta)
    bound = V.error_bound(q, g, shape[2], w, c, beta)
    ratio = np.abs(D.cpu().numpy().astype(np.float64) - want) / bound
    print('d %d beta %g: worst error / bound = %.3e (worst error %.3e)'
          % (shape[0], beta, ratio.max(), np.abs(D.cpu().numpy() - want).max()))
    assert ratio.max() <= 1.0
    if beta == 1.0:                                                             # sigmoid(-F) = the pair probability
        from grl_amd import engine
        lg = V.literal_logits(q[:, shape[2]:shape[2] + shape[1]], g[:, shape[2]:shape[2] + shape[1]], head)
        prob = np.exp(lg[..., 1]) / (np.exp(lg[..., 0]) + np.exp(lg[..., 1]))
        assert np.abs(engine.verify_prob(D).cpu().numpy() - prob).max() <= 0.25 * bound.max() + 2.0 ** -23


# ----------------------------------------------------------------------------
# 3. agreement with the per-pair head kernel of the training batch
# ----------------------------------------------------------------------------
def test_verify_dist_agrees_with_grl_pair_verify():
    from grl_amd import engine
    D_in = 2048
    siam, head = make_siam(D_in, seed=3, out=128)
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(4)).standard_normal((8, 4, D_in)).astype(np.float32)).to(DEV)
    cls, out = engine.siamese_forward(siam, x)
    half = 4
    assert tuple(cls.shape) == (half, half, 2)
    got = engine.verify_dist(out[:half], out[half:], engine.verify_metric(siam, 0, 1.0))
    w, c = V.fold(head)
    o = out.cpu().numpy()
    bound = V.error_bound(o[:half], o[half:], 0, w, c, 1.0)
    diff = np.abs((cls[..., 0] - cls[..., 1]).cpu().numpy().astype(np.float64) - got.cpu().numpy())
    print('pair kernel against verify_dist: worst difference / bound = %.3e' % (diff / bound).max())
    assert (diff <= bound).all()


# ----------------------------------------------------------------------------
# 4. a block holds the matrix's bits; search = the sorted matrix
# ----------------------------------------------------------------------------
def _filtered_ref(D, order, k, ids):
    qp, gp, qc, gc = ids
    idx = np.full((NQ, k), -1, np.int64)
    val = np.full((NQ, k), np.inf, np.float32)
    for q in range(NQ):
        o = order[q]
        if ids is not None:
            o = o[~((gp[o] == qp[q]) & (gc[o] == qc[q]))]
        o = o[:k]
        idx[q, :o.size] = o
        val[q, :o.size] = D[q, o]
    return val, idx


@pytest.mark.parametrize('beta', BETAS)
@pytest.mark.parametrize('shape', [REAL, SMALL])
def test_blocks_and_search_equal_the_matrix_bit_for_bit(shape, beta):
    from grl_amd import engine
    qf, gf = case(shape)[4], case(shape)[5]
    vm, D = dist_of(shape, beta)
    order = engine.rank_rows(D).long().cpu().numpy()
    Dh = D.cpu().numpy()
    ids = _ids()
    for width in WIDTHS:
        blocks = engine._ColumnBlocks(qf, gf, vm, block_cols=width)
        if width is not None:
            assert len(blocks.spans) >= 3 and (blocks.spans[-1][1] - blocks.spans[-1][0]) < width
        for c0, c1 in blocks.spans:
            assert torch.equal(_bits(blocks.block(c0, c1)), _bits(D[:, c0:c1])), (width, c0, c1)
        for k in (10, NG + 100):                                                # k > ng: the tail is padding
            for exclude in (None, ids):
                dist, idx = engine.search(qf, gf, k, metric=vm, exclude=exclude, block_cols=width)
                val_ref, idx_ref = _filtered_ref(Dh, order, k, exclude if exclude is not None else
                                                 (np.full(NQ, -1), np.zeros(NG), np.zeros(NQ), np.zeros(NG)))
                assert np.array_equal(idx.cpu().numpy(), idx_ref), (width, k, exclude is not None)
                assert np.array_equal(dist.cpu().numpy().view(np.int32), val_ref.view(np.int32))
                if k > NG:
                    assert (idx_ref[:, -1] == -1).all() and np.isinf(val_ref[:, -1]).all()
    # a shard of the gallery rows prepares its own row terms and still holds the matrix's bits
    blocks = engine._ColumnBlocks(qf, gf, vm, block_cols=50, lo=101, hi=NG)
    assert blocks.rg.numel() == NG - 101
    for c0, c1 in blocks.spans:
        assert torch.equal(_bits(blocks.block(c0, c1)), _bits(D[:, c0:c1])), (c0, c1)


# ----------------------------------------------------------------------------
# 5. streaming CMC / mAP
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('beta', BETAS)
def test_streaming_metrics_equal_the_materialised_ones(beta):
    from grl_amd import engine
    qf, gf = case(REAL)[4], case(REAL)[5]
    vm, D = dist_of(REAL, beta)
    qp, gp, qc, gc = _ids()
    with contextlib.redirect_stdout(io.StringIO()):
        cmc_ref, map_ref = engine.rank_metrics(engine.rank_rows(D), qp, gp, qc, gc)
    for width in WIDTHS:
        with contextlib.redirect_stdout(io.StringIO()):
            cmc, mAP = engine.rank_metrics_streaming(qf, gf, qp, gp, qc, gc, metric=vm, block_cols=width)
        assert np.array_equal(cmc, cmc_ref) and abs(mAP - map_ref) <= 1e-12, (width, mAP, map_ref)


# ----------------------------------------------------------------------------
# 6. ATTEvaluator.evaluate with GRL_EVAL_METRIC
# ----------------------------------------------------------------------------
KNOBS = ('GRL_EVAL_STREAM', 'GRL_EVAL_RERANK', 'GRL_EVAL_QE', 'GRL_EVAL_DBA', 'GRL_EVAL_METRIC')
KEEP = ('Mean AP', 'Rank-')


def test_attevaluator_ranks_by_the_head_on_every_route(synth_models, monkeypatch, tmp_path):
    from grl_amd import engine
    from grl_amd.reid.data import get_data
    from grl_amd.reid.evaluator import ATTEvaluator
    from grl_amd.reid.evaluator.attevaluator import evaluate_seq
    from grl_amd.reid.evaluator.eva_functions import evaluate
    cnn, siam, _ = synth_models
    cnn, siam = cnn.to(DEV).eval(), siam.to(DEV).eval()
    _, _, _, q_loader, g_loader = get_data('synthetic', 0, None, 4, 2, 0, 0)
    ev = ATTEvaluator(cnn, siam, only_eval=False)
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    with contextlib.redirect_stdout(io.StringIO()):
        qf, qp, qc = ev.extract_feature(q_loader)
        gf, gp, gc = ev.extract_feature(g_loader)
    gf, gp, gc = torch.cat((qf, gf), 0), np.append(qp, gp), np.append(qc, gc)

    def run(rerank=0, visual=0, query=None, gallery=None):
        with contextlib.redirect_stdout(io.StringIO()) as o:
            r = ev.evaluate(query, gallery, q_loader, g_loader, str(tmp_path) + os.sep, visual, rerank)
        return r, o.getvalue()

    def lines(text):
        return [l for l in text.splitlines() if l.startswith(KEEP)]
    # the knob unset: the cosine metrics of the same features, and no word of the head
    with contextlib.redirect_stdout(io.StringIO()) as o:
        r_cos = evaluate_seq(None, qp, qc, gp, gc, '', indices=engine.rank_rows(engine.cosin_dist(qf, gf)))
    r0, text0 = run()
    assert r0 == r_cos and lines(text0) == lines(o.getvalue()) and 'Ranking metric' not in text0
    monkeypatch.setenv('GRL_EVAL_METRIC', 'cosine')
    assert run() == (r0, text0)
    # verify,0.35: default and streaming routes, and the host ranking of verify_dist
    monkeypatch.setenv('GRL_EVAL_METRIC', 'verify,0.35')
    r_def, text_def = run()
    monkeypatch.setenv('GRL_EVAL_STREAM', '1')
    r_str, text_str = run()
    monkeypatch.delenv('GRL_EVAL_STREAM')
    assert 'Ranking metric: verification head, beta = 0.35' in text_def
    assert r_str == r_def and lines(text_str) == lines(text_def)
    vm = engine.verify_metric(siam, 2048, 0.35)
    D = engine.verify_dist(qf, gf, vm)
    cmc, mAP = evaluate(D.cpu().numpy(), qp, gp, qc, gc)
    assert r_def == cmc[0]
    assert lines(text_def)[0] == 'Mean AP: {:4.1%}'.format(mAP)
    # visual=1: ranked.json carries F of the junk-filtered top-k
    import json
    monkeypatch.setenv('GRL_VISUAL_QUERIES', '0,3')
    query = [(('q%d.jpg' % i,), int(p), int(c)) for i, (p, c) in enumerate(zip(qp, qc))]
    gallery = [(('g%d.jpg' % i,), int(p), int(c)) for i, (p, c) in enumerate(zip(gp[len(qp):], gc[len(qp):]))]
    monkeypatch.setattr('grl_amd.reid.evaluator.attevaluator.visualize_ranked_results', lambda *a, **k: None)
    os.makedirs(str(tmp_path / 'visual'), exist_ok=True)
    r_vis, _ = run(visual=1, query=query, gallery=gallery)
    assert r_vis == r_def
    dist, idx = engine.search(qf, gf, 10, metric=vm, exclude=(qp, gp, qc, gc))
    ranked = json.load(open(str(tmp_path / 'visual' / 'ranked.json')))
    for qi in (0, 3):
        assert [e[0] for e in ranked[str(qi)]] == idx[qi].tolist()
        assert [np.float32(e[3]) for e in ranked[str(qi)]] == dist[qi].cpu().numpy().tolist()
    # rerank=1 is refused before anything runs
    with pytest.raises(ValueError, match='cannot re-rank'):
        run(rerank=1)


# ----------------------------------------------------------------------------
# 7. two gloo ranks on one device shard the gallery rows
# ----------------------------------------------------------------------------
def _shard_case():
    from grl_amd import engine
    siam, head, q, g, qf, gf, w, c = case(SMALL)
    qp, gp, qc, gc = _ids()
    out = {}
    for beta in BETAS:
        vm = engine.verify_metric(siam, SMALL[2], beta)
        d, i = engine.search(qf, gf, 20, metric=vm, exclude=(qp, gp, qc, gc), block_cols=37)
        with contextlib.redirect_stdout(io.StringIO()):
            cmc, mAP = engine.rank_metrics_streaming(qf, gf, qp, gp, qc, gc, metric=vm, block_cols=37)
        out[beta] = (_bits(d).cpu(), i.cpu(), cmc, mAP)
    return out


def _worker(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.save(_shard_case(), os.path.join(outdir, 'rank%d.pt' % rank))
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_return_the_single_process_lists_and_metrics(tmp_path_factory):
    single = _shard_case()
    outdir = str(tmp_path_factory.mktemp('verify_w2'))
    world, port = 2, 45100 + os.getpid() % 1500
    ctx = mp.get_context('spawn')
    procs = [ctx.Process(target=_worker, args=(r, world, port, outdir)) for r in range(world)]
    for p in procs:
        p.start()
    failed = None
    for r, p in enumerate(procs):                   # every child has its own time limit; the first failure ends the rest
        if failed is None:
            p.join(120)
            if p.is_alive() or p.exitcode != 0:
                failed = 'rank %d: %s' % (r, 'timed out' if p.is_alive() else 'exit code %r' % p.exitcode)
        if failed is not None and p.is_alive():
            p.terminate()
            p.join(10)
    assert failed is None, failed
    for r in range(world):
        res = torch.load(os.path.join(outdir, 'rank%d.pt' % r), weights_only=False)
        for beta in BETAS:
            d, i, cmc, mAP = res[beta]
            assert torch.equal(d, single[beta][0]) and torch.equal(i, single[beta][1]), (beta, r)
            assert np.array_equal(cmc, single[beta][2]) and abs(mAP - single[beta][3]) <= 1e-12, (beta, r)
