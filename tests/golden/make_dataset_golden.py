#!/usr/bin/env python
"""Generate tests/golden/datasets.json by running the REFERENCE's dataset classes and pair sampler (imported from
/root/reference, as make_golden.py does) on the miniature trees of tests/dataset_tree.py.  Runs only in the build
container; the output is plain data (root-relative tracklet lists, pids, camids, counts, sampler index sequences)
consumed by tests/test_datasets_cpu.py.

The reference hard-codes its dataset roots as class attributes (MARS derives its file paths from the root when the
class is created), so they are pointed at a fresh temporary tree here; the split_*.json caches the reference writes
land in that tree and are thrown away with it.

    python tests/golden/make_dataset_golden.py
"""
import contextlib
import io
import json
import os
import os.path as osp
import sys
import tempfile

import numpy as np
import torch

HERE = osp.dirname(osp.abspath(__file__))
sys.path.insert(0, osp.dirname(HERE))           # tests/: dataset_tree
sys.path.insert(0, HERE)                        # make_golden: the reference's import-time stubs

import dataset_tree as T                        # noqa: E402
from make_golden import import_reference       # noqa: E402

SEEDS = (0, 7)
MIN_SEQ_LEN = 4


def rel(tracklets, root):
    return [[[osp.relpath(p, root) for p in paths], int(pid), int(camid)] for paths, pid, camid in tracklets]


def run_mars(Mars, root, min_seq_len):
    info = osp.join(root, 'info')
    for attr, path in (('root', root), ('train_name_path', osp.join(info, 'train_name.txt')),
                       ('test_name_path', osp.join(info, 'test_name.txt')),
                       ('track_train_info_path', osp.join(info, 'tracks_train_info.mat')),
                       ('track_test_info_path', osp.join(info, 'tracks_test_info.mat')),
                       ('query_IDX_path', osp.join(info, 'query_IDX.mat')),
                       ('split_train_json_path', osp.join(root, 'split_train.json')),
                       ('split_query_json_path', osp.join(root, 'split_query.json')),
                       ('split_gallery_json_path', osp.join(root, 'split_gallery.json'))):
        setattr(Mars, attr, path)
    for n in ('split_train.json', 'split_query.json', 'split_gallery.json'):
        if osp.exists(osp.join(root, n)):
            os.remove(osp.join(root, n))
    with contextlib.redirect_stdout(io.StringIO()):
        m = Mars(min_seq_len=min_seq_len)
    return m, dict(
        train=rel(m.train, root), query=rel(m.query, root), gallery=rel(m.gallery, root),
        num_train_pids=m.num_train_pids, num_query_pids=m.num_query_pids, num_gallery_pids=m.num_gallery_pids,
        queryinfo=dict(pid=list(m.queryinfo.pid), camid=list(m.queryinfo.camid), tranum=list(m.queryinfo.tranum)),
        galleryinfo=dict(pid=list(m.galleryinfo.pid), camid=list(m.galleryinfo.camid),
                         tranum=list(m.galleryinfo.tranum)))


def sampler_runs(Sampler, train):
    out = {}
    for seed in SEEDS:
        torch.manual_seed(seed)
        np.random.seed(seed)
        out[str(seed)] = [int(i) for i in Sampler(train)]
    return out


def main():
    import_reference()
    from reid.data.sampler import RandomPairSamplerForMars
    from reid.dataset.duke import DukeMTMCVidReID
    from reid.dataset.mars import Mars

    golden = {}
    with tempfile.TemporaryDirectory() as tmp:
        root = T.make_mars_tree(osp.join(tmp, 'MARS'))
        m, golden['mars'] = run_mars(Mars, root, 0)
        golden['mars']['sampler'] = sampler_runs(RandomPairSamplerForMars, m.train)
        _, golden['mars_min_seq_len'] = run_mars(Mars, root, MIN_SEQ_LEN)
        golden['mars_min_seq_len']['min_seq_len'] = MIN_SEQ_LEN

        root = T.make_duke_tree(osp.join(tmp, 'DukeMTMC-VideoReID'))
        DukeMTMCVidReID.root = root
        with contextlib.redirect_stdout(io.StringIO()):
            d = DukeMTMCVidReID()
        label = {}
        for paths, pid, _ in d.train:
            label[osp.relpath(paths[0], root).split(os.sep)[1]] = pid
        golden['duke'] = dict(
            train=rel(d.train, root), train_dense=rel(d.train_dense, root), query=rel(d.query, root),
            gallery=rel(d.gallery, root), num_train_pids=d.num_train_pids, num_query_pids=d.num_query_pids,
            num_gallery_pids=d.num_gallery_pids, label_map=label)

    out = osp.join(HERE, 'datasets.json')
    with open(out, 'w') as fh:
        json.dump(golden, fh, separators=(',', ':'), sort_keys=True)
    print('wrote %s (%d bytes)' % (out, osp.getsize(out)))


if __name__ == '__main__':
    main()
