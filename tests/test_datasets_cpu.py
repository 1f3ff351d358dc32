"""MARS / DukeMTMC-VideoReID indexes, the pair sampler and get_data's loaders (no GPU): pinned to what the reference's
own classes compute on the miniature trees of tests/dataset_tree.py (tests/golden/datasets.json, written by
tests/golden/make_dataset_golden.py)."""
import collections
import io
import json
import os
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest
import torch

import dataset_tree as T

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
GOLDEN = osp.join(ROOT, 'tests', 'golden', 'datasets.json')


@pytest.fixture(scope='module')
def gold():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.fixture(scope='module')
def trees(tmp_path_factory):
    base = tmp_path_factory.mktemp('datasets')
    T.make_mars_tree(str(base / 'MARS'))
    T.make_duke_tree(str(base / 'DukeMTMC-VideoReID'))
    return str(base)


def _quiet(fn, *a, **k):
    import contextlib
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _rel(tracklets, root):
    return [[[osp.relpath(p, root) for p in paths], pid, camid] for paths, pid, camid in tracklets]


def _mars(trees, **kw):
    from grl_amd.reid.dataset import get_sequence
    return _quiet(get_sequence, 'mars', data_dir=trees, **kw)


def _duke(trees, **kw):
    from grl_amd.reid.dataset import get_sequence
    return _quiet(get_sequence, 'duke', data_dir=trees, **kw)


@pytest.mark.parametrize('key', ['mars', 'mars_min_seq_len'])
def test_mars_matches_reference(trees, gold, key):
    g = gold[key]
    m = _mars(trees, min_seq_len=g.get('min_seq_len', 0))
    root = osp.join(trees, 'MARS')
    assert m.root == root
    for split in ('train', 'query', 'gallery'):
        assert _rel(getattr(m, split), root) == g[split], split
        assert all(isinstance(p, tuple) for p, _, _ in getattr(m, split))
    for k in ('num_train_pids', 'num_query_pids', 'num_gallery_pids'):
        assert getattr(m, k) == g[k], k
    for info in ('queryinfo', 'galleryinfo'):
        for f in ('pid', 'camid', 'tranum'):
            assert list(getattr(getattr(m, info), f)) == g[info][f], (info, f)


def test_mars_min_seq_len_keeps_info_of_dropped_tracks(gold):
    """the reference's quirk: galleryinfo still lists a track that min_seq_len dropped"""
    g = gold['mars_min_seq_len']
    assert len(g['galleryinfo']['pid']) > len(g['gallery'])
    assert len(gold['mars']['galleryinfo']['pid']) == len(gold['mars']['gallery'])


def test_duke_matches_reference(trees, gold):
    g = gold['duke']
    d = _duke(trees)
    root = osp.join(trees, 'DukeMTMC-VideoReID')

    def bag(ts):
        return collections.Counter((tuple(p), pid, cam) for p, pid, cam in ts)
    for split in ('train', 'train_dense', 'query', 'gallery'):
        assert bag(_rel(getattr(d, split), root)) == bag(g[split]), split
    for k in ('num_train_pids', 'num_query_pids', 'num_gallery_pids'):
        assert getattr(d, k) == g[k], k
    label = {osp.relpath(p[0], root).split(os.sep)[1]: pid for p, pid, _ in d.train}
    assert label == g['label_map']
    # walked in sorted order: the same on every filesystem
    assert _rel(d.train, root) == sorted(_rel(d.train, root), key=lambda t: t[0][0])


def test_duke_missing_frame_index_is_skipped(trees):
    d = _duke(trees)
    t = [p for p, _, _ in d.train if '/0023/0001/' in p[0].replace(os.sep, '/')][0]
    names = [osp.basename(p) for p in t]
    assert len(names) == 6 and not any('F0003' in n for n in names) and not any('F0008' in n for n in names)


def _check_pairs(seq, train):
    pid_cams = collections.defaultdict(set)
    for _, pid, cam in train:
        pid_cams[pid].add(cam)
    assert len(seq) == 2 * len(train)
    assert sorted(seq[0::2]) == list(range(len(train)))
    for a, p in zip(seq[0::2], seq[1::2]):
        assert train[a][1] == train[p][1]
        if len(pid_cams[train[a][1]]) > 1:
            assert train[a][2] != train[p][2]


def test_sampler_matches_reference(trees, gold):
    from grl_amd.reid.data import RandomPairSamplerForMars
    m = _mars(trees)
    for seed, want in gold['mars']['sampler'].items():
        torch.manual_seed(int(seed))
        np.random.seed(int(seed))
        got = list(RandomPairSamplerForMars(m.train))
        assert got == want, seed
        _check_pairs(got, m.train)


def test_sampler_single_tracklet_and_single_camera():
    from grl_amd.reid.data import RandomPairSamplerForMars
    train = [((), 0, 0), ((), 1, 2), ((), 1, 2), ((), 1, 2)]
    torch.manual_seed(3)
    np.random.seed(3)
    seq = list(RandomPairSamplerForMars(train))
    for a, p in zip(seq[0::2], seq[1::2]):
        assert (p == a) if a == 0 else (p != a and p in (1, 2, 3))


def _seed(s):
    import random
    random.seed(s)                  # the augmentation draws (augment.draw_clip_params)
    np.random.seed(s)               # the frame draws and the positives
    torch.manual_seed(s)            # the sampler's permutation


def _loaders(name, trees, only_eval, batch=8, **env):
    from grl_amd.reid.data import get_data
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return _quiet(get_data, name, 0, trees, batch, 4, 4, 0, only_eval=only_eval)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize('name', ['mars', 'duke'])
@pytest.mark.parametrize('only_eval', [False, True])
def test_get_data_shapes(trees, gold, name, only_eval):
    g = gold[name]
    dataset, num_classes, train, query, gallery = _loaders(name, trees, only_eval)
    assert num_classes == g['num_train_pids'] == dataset.num_train_pids
    assert len(train) == 2 * len(g['train']) // 8
    per = 1 if only_eval else 30
    assert len(query) == -(-len(g['query']) // per) and len(gallery) == -(-len(g['gallery']) // per)
    assert train.dataset.sample == 'rrs_train' and train.dataset.augment and train.drop_last
    assert query.dataset.sample == gallery.dataset.sample == ('dense' if only_eval else 'rrs_test')
    assert train.dataset.decode == 'device'


def test_get_data_train_batch_device_and_host(trees):
    """device decode: the batch carries compressed frames that know their files; GRL_DECODE=host: Pillow in the worker
    (Duke: RectScale'd to 256 x 128 there).  Same sampler, same frame draws, same augmentation block."""
    from grl_amd.reid.data.jpeg import JpegBatch
    for name in ('mars', 'duke'):
        _seed(1)
        dev = next(iter(_loaders(name, trees, False)[2]))
        _seed(1)
        host = next(iter(_loaders(name, trees, False, GRL_DECODE='host')[2]))
        assert isinstance(dev[0], JpegBatch) and dev[0].shape == (8, 4)
        assert all(osp.isfile(s.path) for s in dev[0].streams)
        assert host[0].dtype == torch.uint8 and tuple(host[0].shape) == (8, 4, 3, 256, 128)
        for a, b in zip(dev[1:], host[1:]):
            assert torch.equal(a, b)
        assert tuple(dev[3].shape) == tuple(host[3].shape) and dev[3].dtype == torch.int32
        assert (dev[1][0::2] == dev[1][1::2]).all()


def test_get_data_rejects_other_datasets(trees):
    from grl_amd.reid.data import get_data
    for name in ('ilidsvidsequence', 'prid2011sequence'):
        with pytest.raises(NotImplementedError, match='optical flow'):
            get_data(name, 0, trees, 8, 4, 4, 0)
    with pytest.raises(ValueError, match='GRL_DECODE'):
        _loaders('mars', trees, False, GRL_DECODE='gpu')
    ds, n, train, q, g = get_data('synthetic', 0, trees, 8, 4, 4, 0)
    assert n == 625 and len(train) == 16 and len(q) == 1 and len(g) == 4


def test_missing_info_file_names_it(trees, tmp_path):
    import shutil
    root = str(tmp_path / 'MARS')
    shutil.copytree(osp.join(trees, 'MARS', 'info'), osp.join(root, 'info'))
    os.remove(osp.join(root, 'info', 'query_IDX.mat'))
    from grl_amd.reid.dataset import Mars, DukeMTMCVidReID
    with pytest.raises(RuntimeError, match='query_IDX.mat'):
        _quiet(Mars, root=root)
    with pytest.raises(RuntimeError, match=str(tmp_path / 'nowhere' / 'MARS')):
        _quiet(Mars, data_dir=str(tmp_path / 'nowhere'))
    os.makedirs(str(tmp_path / 'duke' / 'train'))
    with pytest.raises(RuntimeError, match='query'):
        _quiet(DukeMTMCVidReID, root=str(tmp_path / 'duke'))


def test_root_resolution(trees, monkeypatch):
    from grl_amd.reid.dataset import Mars
    mars = osp.join(trees, 'MARS')
    assert _quiet(Mars, data_dir=mars).root == mars                       # data_dir with the layout
    assert _quiet(Mars, data_dir=trees).root == mars                      # data_dir/MARS
    monkeypatch.setenv('GRL_MARS_ROOT', mars)
    assert _quiet(Mars, data_dir='/nonexistent').root == mars             # the environment before data_dir
    assert _quiet(Mars, root=mars, data_dir='/nonexistent').root == mars


def test_parsing_writes_nothing_into_the_root(trees):
    before = T.snapshot(trees)
    _mars(trees)
    _duke(trees)
    for name in ('mars', 'duke'):
        loaders = _loaders(name, trees, False)
        next(iter(loaders[2]))
        next(iter(loaders[3]))
    assert T.snapshot(trees) == before


def test_unsupported_frame_names_its_file(tmp_path):
    from PIL import Image
    from grl_amd.reid.data import RawVideoDataset
    from grl_amd.reid.data.jpeg import JpegUnsupported, jpeg_collate
    paths = []
    for i, prog in enumerate((False, True, False, False)):
        p = str(tmp_path / ('f%d.jpg' % i))
        Image.fromarray(T.frame_image(i)).save(p, 'JPEG', quality=90, progressive=prog)
        paths.append(p)
    ds = RawVideoDataset([(tuple(paths), 0, 0)], seq_len=4, sample='rrs_test', decode='device')
    batch = jpeg_collate([ds[0]])[0]
    with pytest.raises(JpegUnsupported, match=r"f1\.jpg.*GRL_DECODE=host"):
        batch.pack()
    with pytest.raises(JpegUnsupported, match=r"f1\.jpg"):          # the clip slice a rank takes keeps the paths
        batch[0:1].pack()


def test_dropin_maps_reid_dataset():
    code = ('import reid.dataset, reid.data, grl_amd.reid.dataset as d, grl_amd.reid.data.sampler as s;'
            'assert reid.dataset is d and reid.data.RandomPairSamplerForMars is s.RandomPairSamplerForMars;'
            'assert reid.dataset.get_sequence is d.get_sequence')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, osp.join(ROOT, 'dropin')]))
    subprocess.check_call([sys.executable, '-c', code], env=env, cwd=ROOT)


def _gloo_rank(rank, world, trees, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.manual_seed(5)
        np.random.seed(5)
        ds, _, train, _, _ = _loaders('mars', trees, False)
        assert train.batch_size == 4 and train.grl_rank_sharded
        out[rank] = list(train.sampler)
    finally:
        dist.destroy_process_group()


def test_sharded_sampler_world2_interleaves(trees):
    import socket
    import torch.multiprocessing as mp
    from grl_amd.reid.data import RandomPairSamplerForMars
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    with mp.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_gloo_rank, args=(2, trees, port, out), nprocs=2, join=True)
        shards = [out[0], out[1]]
    torch.manual_seed(5)
    np.random.seed(5)
    train = _mars(trees).train
    whole = list(RandomPairSamplerForMars(train))
    merged = []
    for k in range(len(whole) // 8):
        merged += shards[0][4 * k:4 * k + 4] + shards[1][4 * k:4 * k + 4]
    assert merged == whole[:len(merged)] and len(merged) == len(whole) // 8 * 8
    for sh in shards:
        for a, p in zip(sh[0::2], sh[1::2]):
            assert train[a][1] == train[p][1]
