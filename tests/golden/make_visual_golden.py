#!/usr/bin/env python
"""Generate tests/golden/visual_ranked.json by running the REFERENCE's visualize_ranked_results (imported from
/root/reference, as make_golden.py does) on the frame tree and distance matrix of tests/visual_tree.py.  Runs only
in the build container; the output is plain data -- the distance matrix, and per run the relative path names of the
folder it wrote and the lines it printed -- consumed by tests/test_visualize_cpu.py.

    python tests/golden/make_visual_golden.py
"""
import contextlib
import io
import json
import os
import os.path as osp
import sys
import tempfile

HERE = osp.dirname(osp.abspath(__file__))
sys.path.insert(0, osp.dirname(HERE))           # tests/: visual_tree, dataset_tree
sys.path.insert(0, HERE)                        # make_golden: the reference's import-time stubs

import visual_tree as V                         # noqa: E402
from make_golden import import_reference       # noqa: E402


def main():
    import_reference()
    from reid.evaluator.visualize import visualize_ranked_results
    dist = V.distance_matrix()
    golden = {'distmat': [[float(x) for x in row] for row in dist], 'runs': []}
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)                           # relative paths: the printed save_dir does not name this machine
        sets = V.make_tree('frames')
        for n, (scenario, visual_id, topk) in enumerate(V.RUNS):
            query, gallery = sets[scenario]
            save_dir = osp.join('out%d' % n, 'visual')
            os.makedirs('out%d' % n)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                visualize_ranked_results(dist, query, gallery, save_dir, visual_id=visual_id, topk=topk)
            golden['runs'].append(dict(scenario=scenario, visual_id=visual_id, topk=topk, save_dir=save_dir,
                                       listing=V.listing(save_dir), printed=buf.getvalue().splitlines()))
        os.chdir(HERE)
    out = osp.join(HERE, 'visual_ranked.json')
    with open(out, 'w') as fh:
        json.dump(golden, fh, separators=(',', ':'), sort_keys=True)
    print('wrote %s (%d bytes)' % (out, osp.getsize(out)))


if __name__ == '__main__':
    main()
