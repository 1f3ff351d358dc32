"""MARS (Zheng et al., ECCV 2016): the tracklet index of the reference's ``reid/dataset/mars.py``, restated.

Layout under the root::

    info/train_name.txt  info/test_name.txt            one frame file name per line
    info/tracks_train_info.mat  info/tracks_test_info.mat   rows [first, last, pid, camid], 1-based line numbers
    info/query_IDX.mat                                  1-based rows of tracks_test_info that form the query
    bbox_train/<pid4>/<name>  bbox_test/<pid4>/<name>   the frames

Behaviour kept from the reference: junk tracks (pid -1) are skipped; camids are 1..6 in the files and 0-based here;
train pids are relabelled by enumerating ``set(pids)`` of the whole train table (junk included, so that the count
``num_train_pids`` is the reference's); query and gallery pids are not relabelled; the gallery is every test track
that is not a query track, in file order; ``min_seq_len`` drops short tracklets, but ``queryinfo`` / ``galleryinfo``
still list the pid and camid of every non-junk track, dropped ones included (the reference appends them before its
length test).  Differences: a tracklet whose frames name different persons or cameras raises ValueError naming it
(the reference asserts), and nothing is cached in the root."""
import os.path as osp

import numpy as np

from ._root import check_paths, resolve_root


class infostruct(object):
    pass


def _read_names(path):
    with open(path, 'r') as f:
        return [line.rstrip() for line in f]


def _load_table(path, key):
    from scipy.io import loadmat
    return np.asarray(loadmat(path)[key]).astype(np.int64)


class Mars(object):

    def __init__(self, min_seq_len=0, root=None, data_dir=None, verbose=True):
        self.root = resolve_root(root, data_dir, 'GRL_MARS_ROOT', 'MARS', 'info')
        info = osp.join(self.root, 'info')
        self.train_name_path = osp.join(info, 'train_name.txt')
        self.test_name_path = osp.join(info, 'test_name.txt')
        self.track_train_info_path = osp.join(info, 'tracks_train_info.mat')
        self.track_test_info_path = osp.join(info, 'tracks_test_info.mat')
        self.query_IDX_path = osp.join(info, 'query_IDX.mat')
        check_paths([self.root, self.train_name_path, self.test_name_path, self.track_train_info_path,
                     self.track_test_info_path, self.query_IDX_path])

        train_names = _read_names(self.train_name_path)
        test_names = _read_names(self.test_name_path)
        track_train = _load_table(self.track_train_info_path, 'track_train_info')
        track_test = _load_table(self.track_test_info_path, 'track_test_info')
        query_idx = _load_table(self.query_IDX_path, 'query_IDX').reshape(-1) - 1
        in_query = np.zeros(len(track_test), bool)
        in_query[query_idx] = True
        track_query = track_test[query_idx]
        track_gallery = track_test[~in_query]

        train, num_train_pids, train_imgs, _, _ = self._tracklets(
            train_names, track_train, 'bbox_train', True, min_seq_len)
        query, num_query_pids, query_imgs, query_pid, query_camid = self._tracklets(
            test_names, track_query, 'bbox_test', False, min_seq_len)
        gallery, num_gallery_pids, gallery_imgs, gallery_pid, gallery_camid = self._tracklets(
            test_names, track_gallery, 'bbox_test', False, min_seq_len)

        self.train, self.query, self.gallery = train, query, gallery
        self.num_train_pids, self.num_query_pids, self.num_gallery_pids = num_train_pids, num_query_pids, num_gallery_pids
        self.queryinfo = infostruct()
        self.queryinfo.pid, self.queryinfo.camid, self.queryinfo.tranum = query_pid, query_camid, query_imgs
        self.galleryinfo = infostruct()
        self.galleryinfo.pid, self.galleryinfo.camid, self.galleryinfo.tranum = gallery_pid, gallery_camid, gallery_imgs

        if verbose:
            n_imgs = train_imgs + query_imgs + gallery_imgs
            print("=> MARS loaded from %s" % self.root)
            print("  subset   | # ids | # tracklets")
            print("  train    | {:5d} | {:8d}".format(num_train_pids, len(train)))
            print("  query    | {:5d} | {:8d}".format(num_query_pids, len(query)))
            print("  gallery  | {:5d} | {:8d}".format(num_gallery_pids, len(gallery)))
            if n_imgs:
                print("  images per tracklet: {} ~ {}, average {:.1f}".format(min(n_imgs), max(n_imgs), np.mean(n_imgs)))

    def _tracklets(self, names, table, home_dir, relabel, min_seq_len):
        """-> (tracklets, num_pids, images per kept tracklet, pid per non-junk track, camid per non-junk track)."""
        pids = set(table[:, 2].tolist())
        label = {pid: i for i, pid in enumerate(pids)} if relabel else None
        tracklets, num_imgs, info_pid, info_camid = [], [], [], []
        for first, last, pid, camid in table.tolist():
            if pid == -1:
                continue
            if not 1 <= camid <= 6:
                raise ValueError("MARS %s: track [%d, %d] has camid %d outside 1..6" % (home_dir, first, last, camid))
            if relabel:
                pid = label[pid]
            camid -= 1
            frames = names[first - 1:last]
            if len({n[:4] for n in frames}) != 1:
                raise ValueError("MARS %s: track [%d, %d] (%s) does not hold the frames of one person"
                                 % (home_dir, first, last, frames[0] if frames else 'empty'))
            if len({n[5] for n in frames}) != 1:
                raise ValueError("MARS %s: track [%d, %d] (%s) holds frames of different cameras"
                                 % (home_dir, first, last, frames[0]))
            if len(frames) >= min_seq_len:
                tracklets.append((tuple(osp.join(self.root, home_dir, n[:4], n) for n in frames), pid, camid))
                num_imgs.append(len(frames))
            info_pid.append(pid)
            info_camid.append(camid)
        return tracklets, len(pids), num_imgs, info_pid, info_camid
