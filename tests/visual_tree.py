"""A small frame tree for the ranked-results visualisation (grl_amd.reid.evaluator.visualize), with the MARS test
tracks and file names of tests/dataset_tree.py.  The frames are a few bytes each: visualisation only copies them.
Shared by tests/golden/make_visual_golden.py (the reference's run) and tests/test_visualize_cpu.py."""
import os

import numpy as np

import dataset_tree as T

TOPK = 10
QUERY_ROWS = [2, 7, 9, 12, 17, 19]        # 1-based rows of MARS_TEST; row 7 (pid 4, camera 5) has a second tracklet there
# (scenario, visual_id, topk) of every recorded run; topk = 30 exceeds the 23 gallery entries
RUNS = [('video', 0, TOPK), ('video', 3, TOPK), ('video', 5, TOPK), ('video', 1, 30), ('video', 4, 1),
        ('image', 2, TOPK), ('image', 5, 3)]


def make_tree(root):
    """Writes the frames under ``root`` (relative paths stay relative) and returns {scenario: (query, gallery)}:
    'video' has tuples of frame paths per entry, 'image' the first frame alone.  The gallery is every test track
    (junk and distractor pids included), the queries are QUERY_ROWS of it, so each query meets itself and, for one,
    another tracklet of its pid and camera in the gallery."""
    tracks, count = [], {}
    for pid, cam, n in T.MARS_TEST:
        t = count[(pid, cam)] = count.get((pid, cam), 0) + 1
        d = os.path.join(root, 'bbox_test', T._mars_name(pid, cam, t, 1)[:4])
        os.makedirs(d, exist_ok=True)
        paths = []
        for f in range(1, n + 1):
            p = os.path.join(d, T._mars_name(pid, cam, t, f))
            with open(p, 'wb') as fh:
                fh.write(('frame %d %d %d %d\n' % (pid, cam, t, f)).encode())
            paths.append(p)
        tracks.append((tuple(paths), pid, cam))
    rows = [r - 1 for r in QUERY_ROWS]
    video = ([tracks[r] for r in rows], tracks)
    image = ([(tracks[r][0][0], tracks[r][1], tracks[r][2]) for r in rows], [(p[0], pid, cam) for p, pid, cam in tracks])
    return {'video': video, 'image': image}


def distance_matrix():
    """[6, 23] float32, all values distinct multiples of 1/256 (no ties: the reference's argsort is not stable).
    Each query's own track is nearest (-1, as the cosine distance of a prepended query) and two more tracks of its
    pid follow, so junk and matches lead every row."""
    rng = np.random.RandomState(20)
    nq, ng = len(QUERY_ROWS), len(T.MARS_TEST)
    d = np.stack([rng.permutation(ng) + 1 for _ in range(nq)]).astype(np.float32) / 256
    pids = np.array([t[0] for t in T.MARS_TEST])
    for q, r in enumerate(r - 1 for r in QUERY_ROWS):
        same = np.flatnonzero(pids == pids[r])
        d[q, same] = -(np.arange(same.size, dtype=np.float32) + 1) / 512
        d[q, r] = -1.0
    return d


def listing(root):
    """Sorted relative paths of every directory and file under ``root`` ('/' separators)."""
    out = []
    for d, dirs, files in os.walk(root):
        for n in dirs + files:
            out.append(os.path.relpath(os.path.join(d, n), root).replace(os.sep, '/'))
    return sorted(out)
