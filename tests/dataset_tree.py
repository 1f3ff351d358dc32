"""Miniature MARS and DukeMTMC-VideoReID trees on disk, in the datasets' own layouts: real baseline JPEG frames
(Pillow, quality 90), MARS's ``info/*.txt`` name lists and ``*.mat`` track tables (scipy.io.savemat), Duke's
``<split>/<pid>/<tracklet>/*.jpg`` directories.  Used by the CPU tests, the GPU tests and tools/loop_rate.py.

The MARS tree covers a pid with one camera and one tracklet, a pid with one camera and several tracklets, pids seen
by several cameras, junk (-1) and distractor (0) test tracks, and tracklets shorter than the clip length.  The Duke
tree has frames of several sizes, both naming schemes and a tracklet with a missing frame index."""
import os

import numpy as np

# MARS train tracks: (pid, camera, frames)
MARS_TRAIN = [
    (1, 1, 6),                                   # one camera, one tracklet
    (3, 2, 5), (3, 2, 7), (3, 2, 3),             # one camera, several tracklets (one shorter than seq_len 4)
    (5, 1, 6), (5, 2, 4), (5, 3, 8), (5, 3, 5),  # three cameras
    (7, 2, 9), (7, 4, 2), (7, 4, 6),             # two cameras, a two-frame tracklet
    (9, 6, 5), (9, 1, 7),
    (11, 5, 4), (11, 3, 6), (11, 5, 5),
]
# MARS test tracks (file order); QUERY: 1-based rows of them
MARS_TEST = [
    (-1, 1, 3),                                  # junk
    (2, 1, 5), (2, 2, 6), (2, 3, 2),
    (0, 4, 4),                                   # distractor
    (4, 2, 6), (4, 5, 7), (4, 5, 3),
    (6, 6, 5), (6, 1, 4),
    (-1, 3, 2),
    (8, 3, 6), (8, 4, 5), (8, 1, 1),
    (0, 2, 3),
    (10, 1, 5), (10, 3, 4), (12, 2, 6), (12, 6, 3), (14, 4, 5), (14, 5, 4), (16, 1, 3), (16, 2, 5),
]
MARS_QUERY = [2, 6, 9, 12, 17, 19]     # (query + gallery: at least 20 entries, the evaluator prints Rank-20)

# Duke tracklets: split -> [(pid, tracklet, camera, frames, (width, height), naming, missing frame index or None)]
DUKE = {
    'train': [
        (17, 1, 1, 6, (128, 256), 'new', None), (17, 2, 2, 5, (96, 220), 'new', None),
        (23, 1, 3, 7, (110, 240), 'new', 3),                       # F0003 missing
        (23, 2, 3, 4, (128, 256), 'new', None),
        (42, 1, 5, 5, (80, 180), 'old', None), (42, 2, 6, 6, (128, 256), 'old', None),
        (42, 3, 5, 70, (90, 200), 'new', None),                    # more than 64 frames: two dense pieces
        (58, 1, 8, 3, (128, 256), 'new', None),
    ],
    'query': [
        (5, 1, 2, 5, (100, 230), 'new', None), (31, 1, 4, 6, (128, 256), 'new', None),
    ],
    'gallery': [
        (5, 1, 1, 4, (128, 256), 'new', None), (5, 2, 3, 6, (90, 200), 'new', None),
        (31, 1, 7, 5, (120, 250), 'new', None), (64, 1, 2, 3, (128, 256), 'new', None),
    ],
}


def frame_image(seed, size=(128, 256)):
    """A smooth, person-sized RGB frame (width, height) that differs per seed."""
    w, h = size
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = rng.uniform(40, 215, 3).astype(np.float32)
    slope = rng.uniform(-0.4, 0.4, (3, 2)).astype(np.float32)
    img = base[:, None, None] + slope[:, 0, None, None] * (y - h / 2) + slope[:, 1, None, None] * (x - w / 2)
    img += 18 * np.sin(x[None] / rng.uniform(4, 12) + y[None] / rng.uniform(6, 20))
    img += rng.normal(0, 4, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8).transpose(1, 2, 0)


def _write_jpeg(path, seed, size=(128, 256), pool=None):
    """Write one frame; with ``pool`` (a dict) frames repeat with period ``pool['n']`` and are hard-linked."""
    from PIL import Image
    if pool is not None:
        key = (seed % pool['n'], size)
        src = pool.get(key)
        if src is not None:
            try:
                os.link(src, path)
            except OSError:
                with open(src, 'rb') as a, open(path, 'wb') as b:
                    b.write(a.read())
            return
        pool[key] = path
    Image.fromarray(frame_image(seed, size)).save(path, 'JPEG', quality=90)


def _mars_name(pid, cam, track, frame):
    return ('00-1' if pid == -1 else '%04d' % pid) + 'C%dT%04dF%03d.jpg' % (cam, track, frame)


def make_mars_tree(root, train=MARS_TRAIN, test=MARS_TEST, query=MARS_QUERY, pool=None):
    """Write a MARS tree under ``root`` (created); returns ``root``.  ``pool``: number of distinct frames to hard-link
    around (large trees for rate measurements); None writes every frame."""
    from scipy.io import savemat
    os.makedirs(os.path.join(root, 'info'), exist_ok=True)
    links = {'n': pool} if pool else None
    seed = 0
    for split, tracks, key in (('train', train, 'track_train_info'), ('test', test, 'track_test_info')):
        names, table, count = [], [], {}
        for pid, cam, n in tracks:
            t = count[(pid, cam)] = count.get((pid, cam), 0) + 1
            first = len(names) + 1
            d = os.path.join(root, 'bbox_' + split, _mars_name(pid, cam, t, 1)[:4])
            os.makedirs(d, exist_ok=True)
            for f in range(1, n + 1):
                name = _mars_name(pid, cam, t, f)
                names.append(name)
                _write_jpeg(os.path.join(d, name), seed, pool=links)
                seed += 1
            table.append([first, len(names), pid, cam])
        with open(os.path.join(root, 'info', '%s_name.txt' % split), 'w') as fh:
            fh.write(''.join(n + '\n' for n in names))
        savemat(os.path.join(root, 'info', 'tracks_%s_info.mat' % split), {key: np.array(table, dtype=np.int32)})
    savemat(os.path.join(root, 'info', 'query_IDX.mat'), {'query_IDX': np.array(query, dtype=np.int32)[None]})
    return root


def make_duke_tree(root, spec=DUKE):
    """Write a DukeMTMC-VideoReID tree under ``root`` (created); returns ``root``."""
    seed = 100000
    for split, tracks in spec.items():
        for pid, tr, cam, n, size, naming, missing in tracks:
            d = os.path.join(root, split, '%04d' % pid, '%04d' % tr)
            os.makedirs(d, exist_ok=True)
            frames = [f for f in range(1, n + 2) if f != missing][:n] if missing else range(1, n + 1)
            for f in frames:
                if naming == 'new':
                    name = '%04d_C%d_F%04d_X%05d.jpg' % (pid, cam, f, 10000 + seed % 90000)
                else:
                    name = '%04dC%dF%04dX%05d.jpg' % (pid, cam, f, 10000 + seed % 90000)
                _write_jpeg(os.path.join(d, name), seed, size)
                seed += 1
    return root


def synthetic_mars_spec(n_pids, tracks_per_pid, frames_per_track, seed=0):
    """Train tracks for a larger MARS tree (rate measurements): every pid on two to four cameras."""
    rng = np.random.RandomState(seed)
    train = []
    for p in range(1, n_pids + 1):
        cams = rng.choice(np.arange(1, 7), rng.randint(2, 5), replace=False)
        for k in range(tracks_per_pid):
            train.append((p, int(cams[k % len(cams)]), int(rng.randint(frames_per_track // 2, frames_per_track * 3 // 2))))
    return train


def snapshot(root):
    """{relative path: (size, mtime_ns)} of every entry under ``root`` -- to show that parsing writes nothing."""
    out = {}
    for d, dirs, files in os.walk(root):
        for n in dirs + files:
            p = os.path.join(d, n)
            st = os.lstat(p)
            out[os.path.relpath(p, root)] = (st.st_size, st.st_mtime_ns)
    return out
