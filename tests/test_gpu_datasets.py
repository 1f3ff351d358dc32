"""get_data('mars' | 'duke') on the device input path: frames decoded on the GPU (the default) against Pillow in the
loader (GRL_DECODE=host), through the trainer's augmentation, a training epoch, the evaluator in both modes and the
reference's two entry points through dropin/, on the miniature trees of tests/dataset_tree.py."""
import contextlib
import io
import os
import os.path as osp
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import dataset_tree as T

pytestmark = pytest.mark.gpu

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))


@pytest.fixture(scope='module')
def trees(tmp_path_factory):
    base = tmp_path_factory.mktemp('datasets')
    T.make_mars_tree(str(base / 'MARS'))
    T.make_duke_tree(str(base / 'DukeMTMC-VideoReID'))
    return str(base)


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _get_data(name, trees, decode, only_eval=False, workers=0, batch=8):
    from grl_amd.reid.data import get_data
    old = os.environ.get('GRL_DECODE')
    os.environ['GRL_DECODE'] = decode
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            return get_data(name, 0, trees, batch, 4, 4, workers, only_eval=only_eval)
    finally:
        if old is None:
            os.environ.pop('GRL_DECODE', None)
        else:
            os.environ['GRL_DECODE'] = old


@pytest.mark.parametrize('name', ['mars', 'duke'])
def test_first_train_batch_device_equals_host(trees, name):
    """the first train batch, same seeds: device decode (+ per-size RectScale for Duke) and host decode give the same
    clips after the trainer's device augmentation, bit for bit"""
    from grl_amd import engine
    dev = torch.device('cuda:0')
    out = {}
    for decode in ('device', 'host'):
        _seed(11)
        loader = _get_data(name, trees, decode)[2]
        imgs, pids, cams, params = next(engine.DevicePrefetcher(iter(loader), dev))
        assert imgs.dtype == torch.uint8
        out[decode] = (engine.augment_normalize_u8(engine.rect_scale_u8(imgs), params), pids, cams, params)
    d, h = out['device'], out['host']
    assert tuple(d[0].shape) == (8, 4, 3, 256, 128)
    for a, b in zip(d[1:], h[1:]):
        assert torch.equal(a, b)
    assert torch.equal(d[0], h[0])
    assert bool(torch.isfinite(d[0]).all())


def test_train_epoch_from_device_decode(trees, synth_models):
    """one SEQTrainer.train epoch fed by get_data('mars') (device decode, 2 workers): finite loss, parameters move"""
    from grl_amd.reid.loss import OIMLoss, PairLoss
    from grl_amd.reid.train import SEQTrainer
    import copy
    dev = torch.device('cuda:0')
    cnn, siam, siamv = (copy.deepcopy(m).to(dev) for m in synth_models)
    _seed(5)
    _, num_classes, train, _, _ = _get_data('mars', trees, 'device', workers=2)
    crit_c = OIMLoss(2048, 625, scalar=30, momentum=0.5).to(dev)
    crit_u = OIMLoss(2048, 625, scalar=30, momentum=0.5).to(dev)
    tr = SEQTrainer(cnn, siam, siamv, PairLoss().to(dev), crit_c, crit_u, None)
    params = [p for m in (cnn, siam, siamv) for p in m.parameters()]
    opt = torch.optim.SGD(params, lr=1e-3, momentum=0.9, weight_decay=5e-4, nesterov=True)
    w0 = cnn.backbone.base[0].weight.detach().clone()
    q0 = siam.featQ.weight.detach().clone()
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(0, train, opt)
    torch.cuda.synchronize()
    assert len(train) == 4
    for k, m in tr.meters.items():
        assert np.isfinite(float(m.avg)), k
    for p, p0 in ((cnn.backbone.base[0].weight, w0), (siam.featQ.weight, q0)):
        assert bool(torch.isfinite(p).all())
        assert float((p - p0).abs().max()) > 0


@pytest.mark.parametrize('only_eval', [False, True], ids=['rrs_test', 'dense'])
def test_evaluate_device_equals_host(trees, synth_models, only_eval):
    """ATTEvaluator on get_data('mars') loaders: features from device decode are bit-identical to those from host
    decode, and evaluate()'s Rank-1 is the host metric on those features"""
    from grl_amd.reid.evaluator import ATTEvaluator
    from grl_amd.reid.evaluator.eva_functions import evaluate as host_evaluate
    dev = torch.device('cuda:0')
    cnn, siam, _ = synth_models
    cnn, siam = cnn.to(dev).eval(), siam.to(dev).eval()
    feats = {}
    for decode in ('device', 'host'):
        _, _, _, q, g = _get_data('mars', trees, decode, only_eval=only_eval, workers=2)
        ev = ATTEvaluator(cnn, siam, only_eval=only_eval)
        feats[decode] = (ev.extract_feature(q), ev.extract_feature(g))
        if decode == 'device':
            with contextlib.redirect_stdout(io.StringIO()):
                top1 = ev.evaluate(None, None, q, g, None, 0, 0)
    (qf, qp, qc), (gf, gp, gc) = feats['device']
    (qf_h, qp_h, _), (gf_h, gp_h, _) = feats['host']
    assert torch.equal(qf, qf_h) and torch.equal(gf, gf_h)
    assert list(qp) == list(qp_h) and list(gp) == list(gp_h)
    assert qf.size(0) == 6 and gf.size(0) == 15
    qf, gf = qf.double().cpu().numpy(), torch.cat((feats['device'][0][0], gf), 0).double().cpu().numpy()
    with contextlib.redirect_stdout(io.StringIO()):
        cmc, _ = host_evaluate(-(qf @ gf.T), qp, np.append(qp, gp), qc, np.append(qc, gc))
    assert abs(float(top1) - float(cmc[0])) < 1e-6


def test_dropin_mars_flow(trees, tmp_path):
    """mars_train.py's main and test_all.py's evaluation through dropin/, -d mars --data-dir <tree>, one epoch"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, osp.join(ROOT, 'dropin')]))
    env.pop('GRL_DECODE', None)
    r = subprocess.run([sys.executable, osp.join(ROOT, 'tests', 'dropin_mars_flow.py'), '-d', 'mars', '--data-dir',
                        trees, '--epochs', '1', '--logs-dir', str(tmp_path / 'logs')],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'dropin flow ok' in r.stdout
