"""MX-FP8 eval datapath ('mxfp8', GRL_MATH_MXFP8, gemm_mxfp8.hip) on the device, against the numpy model of its
numerics contract (tests/mx_ref.py)."""
import os
import sys

import numpy as np
import pytest
import torch

from grl_amd.synthetic import synth_clips, synth_state_dict

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mx_ref as R                      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _lib():
    from grl_amd import _lib
    return _lib, _lib.load()


def _quant_dev(x_bf16):
    """grl_mx_quantize_rows of a bf16 [M][K] device tensor -> (elements, scales) numpy"""
    _l, lib = _lib()
    M, K = x_bf16.shape
    img = torch.empty(lib.grl_mx_image_bytes(M, K), dtype=torch.uint8, device=DEV)
    _l.check(lib.grl_mx_quantize_rows(_l.ptr(x_bf16), M, K, x_bf16.stride(0), _l.ptr(img), _l.stream()), 'quantize')
    return _split(img.cpu().numpy(), M, K)


def _split(img, M, K):
    sk = R.scale_padded(K // 32)
    return img[:M * K].reshape(M, K), img[M * K:].reshape(M, sk)[:, :K // 32]


def _pack_dev(w_f32, K=None):
    _l, lib = _lib()
    N, ldw = w_f32.shape
    K = K or ldw
    img = torch.empty(lib.grl_mx_image_bytes(N, K), dtype=torch.uint8, device=DEV)
    _l.check(lib.grl_mx_pack_weights(_l.ptr(w_f32), N, K, ldw, _l.ptr(img), _l.stream()), 'pack')
    return img


def _special_rows(rng, K):
    rows = [rng.standard_normal(K) * np.exp(rng.uniform(-30, 30)) for _ in range(40)]
    rows.append(np.zeros(K))
    rows.append(rng.standard_normal(K) * 1e-38)              # tiny (fp32 subnormals after the bf16 cast in places)
    rows.append(rng.standard_normal(K) * 1e36)               # huge
    r = rng.standard_normal(K); r[5] = np.nan; r[K // 2] = np.nan; rows.append(r)
    rows.append(np.full(K, np.nan))
    r = rng.standard_normal(K); r[:32] = 0; r[40] = np.inf; rows.append(r)
    return np.stack(rows)


def test_quantizers_bit_identical_to_the_model():
    rng = np.random.default_rng(3)
    K = 160                                                  # (5 blocks: a padded scale row)
    x = R.bf16_round(_special_rows(rng, K).astype(np.float32))
    xt = torch.from_numpy(x).to(DEV).to(torch.bfloat16)
    assert np.array_equal(xt.float().cpu().numpy(), x, equal_nan=True)
    q, s = _quant_dev(xt)
    q0, s0 = R.quantize_rows(x)
    assert np.array_equal(s, s0), np.argwhere(s != s0)[:5]
    assert np.array_equal(q, q0), np.argwhere(q != q0)[:5]
    # weights: fp32 source with a leading dimension wider than K
    w = _special_rows(rng, 256).astype(np.float32)
    wt = torch.from_numpy(w).to(DEV)
    img = _pack_dev(wt, K=192).cpu().numpy()
    q1, s1 = _split(img, w.shape[0], 192)
    q0, s0 = R.quantize_rows(w[:, :192])
    assert np.array_equal(s1, s0) and np.array_equal(q1, q0)
    pad = img[w.shape[0] * 192:].reshape(w.shape[0], 8)[:, 6:]
    assert (pad == 0).all()


def _mx_gemm(a16, wimg, M, N, K, conv=None, scale=None, shift=None, res=None, gbias=None, rpg=0, relu=False, ldy=None,
             rowscale=None):
    from grl_amd import engine
    y = torch.full((M, ldy or N), float('nan'), dtype=torch.bfloat16, device=DEV)
    engine.gemm(a16, wimg, y, M, N, K, scale=scale, shift=shift, res=res, gbias=gbias, rows_per_group=rpg, relu=relu,
                conv=conv, math=engine.MATH_MXFP8, ldy=ldy, rowscale=rowscale)
    return y


def _im2col(img, n, H, W, C, k, stride, pad):
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    x = img.reshape(n, H, W, C)
    xp = np.zeros((n, H + 2 * pad, W + 2 * pad, C), dtype=img.dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    cols = []
    for ty in range(k):
        for tx in range(k):
            cols.append(xp[:, ty:ty + stride * Ho:stride, tx:tx + stride * Wo:stride, :])
    return np.concatenate(cols, axis=3).reshape(n * Ho * Wo, k * k * C), Ho, Wo


def _exact_operand(rng, rows, K, lo, hi):
    """integers of <= 3 significant bits times a power of two per 32-block in [2^lo, 2^hi]: quantisation is exact"""
    v = rng.choice([0, 1, 2, 3, 4, 5, 6, 7, -1, -2, -3, -4, -5, -6, -7], size=(rows, K)).astype(np.float64)
    p = rng.integers(lo, hi + 1, size=(rows, K // 32)).repeat(32, axis=1)
    return (v * np.ldexp(1.0, p)).astype(np.float32)


@pytest.mark.parametrize('form', ['dense', 'conv_s1', 'conv_s2'])
def test_exact_data_gemm_matches_fp64_exactly(form):
    """Operand lane maps and scale maps: with exactly quantisable data (every product and partial sum exact in fp32)
    the MX GEMM equals the fp64 product bit for bit after the bf16 store.  A and W are different (asymmetric)."""
    rng = np.random.default_rng(11)
    if form == 'dense':
        M, N, K = 256 + 37, 192, 2048
        a = _exact_operand(rng, M, K, -4, 0)
        A = a
        conv = None
    else:
        stride = 1 if form == 'conv_s1' else 2
        n, H, W, Cc = 3, 13, 11, 96
        a = _exact_operand(rng, n * H * W, Cc, -4, 0)
        A, Ho, Wo = _im2col(a.astype(np.float64), n, H, W, Cc, 3, stride, 1)
        M, N, K = A.shape[0], 192, A.shape[1]
        conv = (H, W, Cc, Ho, Wo, 3, 3, stride, 1)
    w = _exact_operand(rng, N, K, 0, 4)
    a16 = torch.from_numpy(a).to(DEV).to(torch.bfloat16)
    assert np.array_equal(a16.float().cpu().numpy(), a)
    y = _mx_gemm(a16, _pack_dev(torch.from_numpy(w).to(DEV)), M, N, K, conv=conv)
    ref = R.bf16_round((A.astype(np.float64) @ w.astype(np.float64).T).astype(np.float32))
    got = y.float().cpu().numpy()
    bad = np.argwhere(got != ref)
    assert bad.size == 0, '%d of %d differ, first %s' % (len(bad), got.size, [(tuple(i), got[tuple(i)], ref[tuple(i)]) for i in bad[:4]])


def _ref_gemm(A, w, scale=None, shift=None, res=None, gbias=None, rpg=0, relu=False, rowscale=None):
    """fp64 of the model-dequantised operands + the epilogue; (value, tolerance scale sum |a.b|)"""
    qa = R.fake_quant(A)
    qw = R.fake_quant(w)
    acc = qa @ qw.T
    mag = np.abs(qa) @ np.abs(qw).T
    v = acc
    if rowscale is not None:
        v = v * rowscale[:, None]
        mag = mag * np.abs(rowscale)[:, None]
    if gbias is not None:
        v = v + gbias[np.arange(A.shape[0]) // rpg]
    if scale is not None:
        v = v * scale[None, :]
    if shift is not None:
        v = v + shift[None, :]
    if res is not None:
        v = v + res
    if relu:
        v = np.maximum(v, 0)
    return v, mag * (np.abs(scale)[None, :] if scale is not None else 1.0)


CASES = {
    '1x1': dict(M=1000, N=256, K=512),
    '1x1_n64': dict(M=517, N=64, K=256),
    'res_relu': dict(M=640, N=384, K=1024, res=True, relu=True),
    'gbias': dict(M=768, N=1024, K=2048, gbias=True),
    'rowscale_gbias': dict(M=300, N=128, K=256, gbias=True, rowscale=True),
    '3x3_s1': dict(conv=(2, 16, 8, 128, 3, 1), N=128),
    '3x3_s2': dict(conv=(3, 15, 9, 128, 3, 2), N=256),
    'down_s2': dict(conv=(2, 16, 8, 256, 1, 2), N=512),
    'c576': dict(conv=(2, 12, 6, 64, 3, 1), N=64),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_random_data_routes(case):
    cfg = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    N = cfg['N']
    conv = None
    if 'conv' in cfg:
        n, H, W, Cc, k, stride = cfg['conv']
        pad = k // 2
        img = R.bf16_round(rng.standard_normal((n * H * W, Cc)).astype(np.float32))
        A, Ho, Wo = _im2col(img.astype(np.float64), n, H, W, Cc, k, stride, pad)
        a_dev = img
        M, K = A.shape
        conv = (H, W, Cc, Ho, Wo, k, k, stride, pad)
    else:
        M, K = cfg['M'], cfg['K']
        A = R.bf16_round(rng.standard_normal((M, K)).astype(np.float32))
        a_dev = A
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    scale = rng.uniform(0.5, 2.0, N).astype(np.float32)
    shift = rng.standard_normal(N).astype(np.float32)
    res = R.bf16_round(rng.standard_normal((M, N)).astype(np.float32)) if cfg.get('res') else None
    rpg = 128
    gb = rng.standard_normal(((M + rpg - 1) // rpg, N)).astype(np.float32) if cfg.get('gbias') else None
    rs = rng.uniform(-2.0, 2.0, M).astype(np.float32) if cfg.get('rowscale') else None
    t = lambda x: None if x is None else torch.from_numpy(x).to(DEV)      # noqa: E731
    y = _mx_gemm(t(a_dev).to(torch.bfloat16), _pack_dev(t(w)), M, N, K, conv=conv, scale=t(scale), shift=t(shift),
                 res=None if res is None else t(res).to(torch.bfloat16), gbias=t(gb), rpg=rpg if gb is not None else 0,
                 relu=bool(cfg.get('relu')), rowscale=t(rs))
    ref, mag = _ref_gemm(A.astype(np.float64), w.astype(np.float64), scale, shift, res, gb, rpg, bool(cfg.get('relu')), rs)
    got = y.float().cpu().numpy().astype(np.float64)
    err = np.abs(got - ref)
    tol = np.abs(ref) * 2.0 ** -8 + 1e-5 * mag        # one bf16 half-ulp + 1e-5 sum |a.b|
    print('%s: max |err| %.3e, max err / tol %.3f' % (case, err.max(), (err / tol).max()))
    assert (err <= tol).all()


def test_nan_reaches_its_row_and_column():
    rng = np.random.default_rng(5)
    M, N, K = 256, 128, 256
    a = rng.standard_normal((M, K)).astype(np.float32)
    a[7, 100] = np.nan
    w = rng.standard_normal((N, K)).astype(np.float32)
    w[9, 3] = np.nan
    y = _mx_gemm(torch.from_numpy(a).to(DEV).to(torch.bfloat16), _pack_dev(torch.from_numpy(w).to(DEV)), M, N, K,
                 relu=True).float().cpu().numpy()
    nan = np.isnan(y)
    assert nan[7].all() and nan[:, 9].all() and nan.sum() == N + M - 1


def test_unsupported_descriptors_do_not_launch():
    from grl_amd import engine
    _l, lib = _lib()
    a = torch.randn(256, 64, device=DEV).to(torch.bfloat16)
    w = _pack_dev(torch.randn(128, 64, device=DEV))
    y = torch.full((256, 128), 7.0, dtype=torch.bfloat16, device=DEV)
    for kw in (dict(epilogue=_l.EPI_EUCLID, rnorm=torch.ones(256, device=DEV), cnorm=torch.ones(128, device=DEV)),
               dict(stats=True), dict(kblock=True)):
        with pytest.raises(_l.GrlHipError, match='mxfp8') as ei:
            engine.gemm(a, w, y, 256, 128, 64, math=engine.MATH_MXFP8, **kw)
        assert '(-3)' in str(ei.value)
    with pytest.raises(_l.GrlHipError, match=r'\(-3\)'):
        engine.gemm(a, w, y, 256, 128, 48, math=engine.MATH_MXFP8)
    torch.cuda.synchronize()
    assert (y.float() == 7.0).all()


# ----------------------------------------------------------------------------------------------------------------
# the pipeline
# ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cnn(synth_models):
    return synth_models[0].to(DEV).eval()


def _mode(mode):
    from grl_amd import engine
    return engine.experimental_math(mode) if mode == 'mxfp8' else engine.math_mode(mode)


def _feats(cnn, clips, mode):
    from grl_amd import engine
    with _mode(mode), torch.no_grad():
        xu, xc = engine._grl_eval(cnn, clips)
    torch.cuda.synchronize()
    return xu.clone(), xc.clone()


def _extract(cnn, siam, clips, mode):
    from grl_amd import engine
    with _mode(mode), torch.no_grad():
        f = engine.extract_features(cnn, siam, clips)
    torch.cuda.synchronize()
    return f.clone()


def _cos(a, b):
    a = a.reshape(a.shape[0] * (a.shape[1] if a.dim() == 3 else 1), -1).double()
    b = b.reshape(a.shape).double()
    return torch.nn.functional.cosine_similarity(a, b, dim=1)


def _rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


REL_L2_BOUND = 0.15      # ~2x the measured maximum, 0.080 (EXPERIMENTS.md, 'MX-FP8 eval datapath')


@pytest.mark.parametrize('bt', [(8, 4), (32, 4), (64, 8)])
@pytest.mark.parametrize('raw', [False, True])
def test_features_close_to_f32(synth_models, bt, raw):
    """x_uncorr / x_corr of the forward and the 6144-d extract_features output (the public entry point, float or raw
    uint8 clips) under the MX datapath against 'f32': per-clip cosine >= 0.98, relative L2 within REL_L2_BOUND."""
    cnn, siam = synth_models[0].to(DEV).eval(), synth_models[1].to(DEV).eval()
    b, t = bt
    clips = synth_clips(b, t, seed=2, raw=raw).to(DEV)
    ref = _feats(cnn, clips, 'f32') + (_extract(cnn, siam, clips, 'f32'),)
    mx = _feats(cnn, clips, 'mxfp8') + (_extract(cnn, siam, clips, 'mxfp8'),)
    for name, r, m in zip(('x_uncorr', 'x_corr', 'extract_features'), ref, mx):
        assert torch.isfinite(m).all()
        cos = _cos(m, r)
        rl = _rel_l2(m, r)
        print('mxfp8 %dx%d raw=%s %s: min per-clip cosine %.5f, rel L2 %.4e' % (b, t, raw, name, cos.min().item(), rl))
        assert cos.min().item() >= 0.98
        assert rl <= REL_L2_BOUND


def test_features_deterministic_and_do_not_disturb_other_modes(cnn):
    clips = synth_clips(8, 4, seed=4).to(DEV)
    f0, b0 = _feats(cnn, clips, 'f32'), _feats(cnn, clips, 'bf16s')
    m1 = _feats(cnn, clips, 'mxfp8')
    m2 = _feats(cnn, clips, 'mxfp8')
    f1, b1 = _feats(cnn, clips, 'f32'), _feats(cnn, clips, 'bf16s')
    for x, y in zip(m1 + f0 + b0, m2 + f1 + b1):
        assert torch.equal(x, y)


def test_load_state_dict_repacks(synth_models):
    import copy
    cnn = copy.deepcopy(synth_models[0]).to(DEV).eval()
    clips = synth_clips(8, 4, seed=6).to(DEV)
    before = _feats(cnn, clips, 'mxfp8')
    sd2 = synth_state_dict(cnn, seed=5)
    cnn.load_state_dict({k: v.to(DEV) for k, v in sd2.items()})
    after = _feats(cnn, clips, 'mxfp8')
    ref = _feats(cnn, clips, 'f32')
    assert not torch.equal(before[0], after[0])
    assert _cos(after[0], ref[0]).min().item() >= 0.98 and _cos(after[1], ref[1]).min().item() >= 0.98


def _launches(cnn, b, t, mode):
    """(math, M, N, K, conv?) -> count of the gemm() launches of one forward in ``mode``"""
    from grl_amd import engine
    seen = {}
    orig = engine.gemm

    def spy(a, w, y, M, N, K, *args, **kw):
        key = (kw.get('math'), M, N, K, kw.get('conv') is not None)
        seen[key] = seen.get(key, 0) + 1
        return orig(a, w, y, M, N, K, *args, **kw)
    engine.gemm = spy
    try:
        _feats(cnn, synth_clips(b, t, seed=1).to(DEV), mode)
    finally:
        engine.gemm = orig
    return seen


@pytest.mark.parametrize('bt', [(32, 4), (64, 8)])
def test_mx_launch_set(cnn, bt):
    """Every GEMM the bf16s forward issues through gemm() on the bf16-storage datapath runs MX under 'mxfp8' (the
    fused TRL f1 + squared-difference GEMM becomes the plain f1 GEMM of the same shape), and nothing else does:
    the fp32 per-clip linears stay fp32 ('MX-FP8 eval datapath')."""
    from grl_amd import engine
    b, t = bt
    ref = _launches(cnn, b, t, 'bf16s')
    seen = _launches(cnn, b, t, 'mxfp8')
    mx = {k[1:]: v for k, v in seen.items() if k[0] == engine.MATH_MXFP8}
    want = {k[1:]: v for k, v in ref.items() if k[0] == engine.MATH_BF16S}
    print('%dx%d: %d MX launches over %d shapes: %s' % (b, t, sum(mx.values()), len(mx), sorted(mx.items())))
    assert mx and mx == want
    assert {k: v for k, v in seen.items() if k[0] != engine.MATH_MXFP8} == \
        {k: v for k, v in ref.items() if k[0] != engine.MATH_BF16S}
    n = b * t
    assert mx[(n * 128, 1024, 2048, False)] == 1 and mx[(n * 128, 256, 1024, False)] >= 1      # GCE corr0, corr2 (+ layer-3 conv1s)
    assert mx[(n * 128, 2048, 2048, False)] == 2                                                # TRL f2, both directions
    assert mx[(b * 128, 2048, 2048, False)] == 2 * t                                             # TRL f1
    assert mx[(b * 128, 512, 2048, False)] == 2 * t and mx[(b * 128, 512, 512, False)] == 2 * t  # TRL c1, c2
    assert mx[(b * 128, 2048, 512, False)] == 2 * t                                              # TRL c3


def test_ranking_of_trained_model_matches_f32():
    """A user-level check: the synthetic re-id problem of tools/convergence_check.py (fixed colour layouts per identity +
    per-clip / per-frame deviation + noise), trained from random initialisation for 150 bf16s iterations with the
    reference's loss and SGD settings; fresh clips of the same identities are then ranked (cosine distance on the 6144-d
    evaluator features).  Rank-1 and mAP with MX-FP8 features are within 1 point of those with f32 features of the
    same weights."""
    import contextlib
    import io
    import torch.nn.functional as F
    from grl_amd import engine, train_engine as TE
    from grl_amd.reid import models
    from grl_amd.reid.train import SEQTrainer
    from grl_amd.reid.loss import OIMLoss, PairLoss
    from grl_amd.reid.evaluator.eva_functions import evaluate
    from grl_amd.synthetic import IMAGENET_MEAN, IMAGENET_STD
    n_id, t, p, iters = 64, 4, 16, 150
    base = torch.from_numpy(np.random.Generator(np.random.PCG64(1234)).uniform(0.0, 1.0, (n_id, 3, 8, 4)).astype(np.float32))

    def clips_of(ids, seed):
        g = np.random.Generator(np.random.PCG64([seed, 5]))
        n = len(ids)
        dc = torch.from_numpy(g.uniform(-0.10, 0.10, (n, 1, 3, 8, 4)).astype(np.float32))
        df = torch.from_numpy(g.uniform(-0.05, 0.05, (n, t, 3, 8, 4)).astype(np.float32))
        low = F.interpolate((base[ids].unsqueeze(1) + dc + df).view(n * t, 3, 8, 4), size=(256, 128), mode='bilinear',
                            align_corners=False)
        noise = torch.from_numpy(g.uniform(-0.1, 0.1, (n * t, 3, 256, 128)).astype(np.float32))
        x = (low + noise).clamp_(0, 1).view(n, t, 3, 256, 128)
        mean = torch.tensor(IMAGENET_MEAN).view(1, 1, 3, 1, 1)
        std = torch.tensor(IMAGENET_STD).view(1, 1, 3, 1, 1)
        return ((x - mean) / std).to(DEV)

    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        cnn = models.create('resnet50_grl', num_features=2048, dropout=0, numclasses=625, pretrained=False)
    siam = models.create('siamese', input_num=2048, output_num=512, class_num=2)
    siamv = models.create('siamese_video', input_num=2048, output_num=512, class_num=2)
    cnn, siam, siamv = cnn.to(DEV), siam.to(DEV), siamv.to(DEV)
    tr = SEQTrainer(cnn, siam, siamv, PairLoss().to(DEV), OIMLoss(2048, 625, scalar=30, momentum=0.5).to(DEV),
                    OIMLoss(2048, 625, scalar=30, momentum=0.5).to(DEV), None)
    base_ids = set(map(id, cnn.backbone.parameters()))
    groups = [{'params': list(cnn.backbone.parameters()), 'lr': 1e-3},
              {'params': [q for q in cnn.parameters() if id(q) not in base_ids] + list(siam.parameters()) +
               list(siamv.parameters()), 'lr': 2e-3}]
    opt = torch.optim.SGD(groups, lr=1e-3, momentum=0.9, weight_decay=5e-4, nesterov=True)
    old = TE.set_math('bf16s')
    try:
        sched = np.random.Generator(np.random.PCG64(77))
        for it in range(iters):
            cnn.train(); siam.train(); siamv.train()
            ids = np.repeat(sched.choice(n_id, p, replace=False), 2)
            loss = tr._forward([clips_of(ids, 1000 + it)], torch.from_numpy(ids).to(DEV), it, 0)[0]
            opt.zero_grad(); loss.backward(); opt.step()
    finally:
        TE.set_math(old)
    cnn.eval(); siam.eval()
    q_ids, g_ids = np.arange(n_id), np.repeat(np.arange(n_id), 3)
    q_clips = [clips_of(q_ids[i:i + 32], 9000 + i) for i in range(0, n_id, 32)]
    g_clips = [clips_of(g_ids[i:i + 32], 9500 + i) for i in range(0, len(g_ids), 32)]
    res = {}
    for mode in ('f32', 'mxfp8'):
        with _mode(mode), torch.no_grad():
            qf = torch.cat([engine.extract_features(cnn, siam, c) for c in q_clips])
            gf = torch.cat([engine.extract_features(cnn, siam, c) for c in g_clips])
        dist = (-(F.normalize(qf, dim=1) @ F.normalize(gf, dim=1).t())).cpu().numpy()
        with contextlib.redirect_stdout(io.StringIO()):
            cmc, mAP = evaluate(dist, q_ids, g_ids, np.zeros(n_id, int), np.ones(len(g_ids), int), max_rank=10)
        res[mode] = (100.0 * float(cmc[0]), 100.0 * float(mAP))
    print('ranking after %d bf16s iterations: f32 Rank-1 %.1f mAP %.1f | mxfp8 Rank-1 %.1f mAP %.1f' % (
        (iters,) + res['f32'] + res['mxfp8']))
    assert res['f32'][0] > 3 * 100.0 / n_id                         # the model learned something (chance = 1.6 %)
    assert abs(res['mxfp8'][0] - res['f32'][0]) <= 1.0 and abs(res['mxfp8'][1] - res['f32'][1]) <= 1.0
