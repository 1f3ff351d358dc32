"""DukeMTMC-VideoReID (Wu et al., CVPR 2018): the tracklet index of the reference's ``reid/dataset/duke.py``, restated.

Layout under the root: ``{train,query,gallery}/<pid>/<tracklet>/*.jpg``.

Behaviour kept from the reference: train pids are relabelled by enumerating ``set(pids)`` of the split's person
directories (query and gallery keep the directory's pid); a tracklet of ``n`` files is looked up frame by frame as
``*F0001*.jpg`` .. ``*F{n:04d}*.jpg``, an index without a file is skipped (so a tracklet that starts at F0002 loses
its last frame, as upstream); tracklets of fewer than ``min_seq_len`` files are dropped; the camera is the digit after
'C' -- name position 5 in the old naming (``0001C6F0099X30823.jpg``), 6 in the new (``0001_C6_F0099_X30823.jpg``) --
made 0-based; ``train_dense`` cuts every train tracklet into pieces of 32 frames (the last piece takes the remainder).

Difference: directories and frame matches are walked in SORTED order.  The reference uses raw ``glob`` order, which
depends on the filesystem, so its tracklet order (and with it a seeded sampler's draws) differs from machine to
machine.  The tracklets themselves are the same, and so is the label map unless two pids share a slot of the set's
hash table (its iteration order then follows insertion order).  Nothing is cached in the root."""
import os
import os.path as osp
import re

import numpy as np

from ._root import check_paths, resolve_root

DENSE_STEP = 32
_FRAME_KEY = re.compile(r'(?=(F\d{4}))')


def _listdir(path):
    """Sorted visible entries of ``path`` (glob's '*' skips names that start with a dot)."""
    return sorted(n for n in os.listdir(path) if not n.startswith('.'))


class DukeMTMCVidReID(object):

    def __init__(self, min_seq_len=0, verbose=True, root=None, data_dir=None, **kwargs):
        self.root = self.dataset_dir = resolve_root(root, data_dir, 'GRL_DUKE_ROOT', 'DukeMTMC-VideoReID', 'train')
        self.train_dir = osp.join(self.root, 'train')
        self.query_dir = osp.join(self.root, 'query')
        self.gallery_dir = osp.join(self.root, 'gallery')
        self.min_seq_len = min_seq_len
        check_paths([self.root, self.train_dir, self.query_dir, self.gallery_dir])

        train, num_train_pids, train_imgs = self._process_dir(self.train_dir, relabel=True)
        query, num_query_pids, query_imgs = self._process_dir(self.query_dir, relabel=False)
        gallery, num_gallery_pids, gallery_imgs = self._process_dir(self.gallery_dir, relabel=False)
        train_dense = []
        for paths, pid, camid in train:
            n = len(paths) // DENSE_STEP
            if n == 0:
                train_dense.append((paths, pid, camid))
            for i in range(n):
                end = len(paths) if i == n - 1 else (i + 1) * DENSE_STEP
                train_dense.append((paths[i * DENSE_STEP:end], pid, camid))

        self.train, self.train_dense, self.query, self.gallery = train, train_dense, query, gallery
        self.num_train_pids, self.num_query_pids, self.num_gallery_pids = num_train_pids, num_query_pids, num_gallery_pids

        if verbose:
            n_imgs = train_imgs + query_imgs + gallery_imgs
            print("=> DukeMTMC-VideoReID loaded from %s" % self.root)
            print("  subset         | # ids | # tracklets")
            print("  train          | {:5d} | {:8d}".format(num_train_pids, len(train)))
            print("  train_dense    | {:5d} | {:8d}".format(num_train_pids, len(train_dense)))
            print("  query          | {:5d} | {:8d}".format(num_query_pids, len(query)))
            print("  gallery        | {:5d} | {:8d}".format(num_gallery_pids, len(gallery)))
            if n_imgs:
                print("  images per tracklet: {} ~ {}, average {:.1f}".format(min(n_imgs), max(n_imgs), np.mean(n_imgs)))

    def _process_dir(self, dir_path, relabel):
        """-> (tracklets, num_pids, file count per kept tracklet)."""
        pdirs = _listdir(dir_path)
        pids = set(int(p) for p in pdirs)
        label = {pid: i for i, pid in enumerate(pids)}
        tracklets, num_imgs = [], []
        for pdir in pdirs:
            pid = label[int(pdir)] if relabel else int(pdir)
            for tdir in _listdir(osp.join(dir_path, pdir)):
                tpath = osp.join(dir_path, pdir, tdir)
                files = [f for f in _listdir(tpath) if f.endswith('.jpg')]
                if len(files) < self.min_seq_len:
                    continue
                num_imgs.append(len(files))
                first = {}                      # 'F0001' -> the first file (sorted) whose name holds it
                for f in files:
                    for m in _FRAME_KEY.finditer(f[:-4]):
                        first.setdefault(m.group(1), f)
                keys = ('F%04d' % k for k in range(1, len(files) + 1))
                paths = [osp.join(tpath, first[k]) for k in keys if k in first]
                if not paths:
                    raise ValueError("DukeMTMC-VideoReID: no frame F0001..F%04d in '%s'" % (len(files), tpath))
                name = osp.basename(paths[0])
                camid = int(name[5] if name.find('_') == -1 else name[6]) - 1
                tracklets.append((tuple(paths), pid, camid))
        return tracklets, len(pids), num_imgs
