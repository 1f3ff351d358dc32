"""Ranked-results folders with the layout of the reference's visualize_ranked_results (its
reid/evaluator/visualize.py:17-81): per query, a folder with the query's frames and the frames of its top-k
gallery tracklets, gallery entries with the query's pid AND camera left out.  The ranked lists may come from the
device (engine.search / engine.rerank_search with ``exclude=``), so no distance matrix has to exist.

visualize_in_pic (matplotlib, commented out in the reference) is not provided."""
import os
import shutil

import numpy as np

from grl_amd.utils.osutils import mkdir_if_missing

__all__ = ['visualize_ranked_results']


def _frames(entry):
    """(paths, is_sequence) of one (img_path(s), pid, camid) entry."""
    paths = entry[0]
    if isinstance(paths, (tuple, list)):
        return list(paths), True
    return [paths], False


def _place(entry, folder, label):
    """Copy an entry into ``folder``: a tracklet becomes the sub-folder ``label`` holding every frame, a single image
    the file ``<label>_name_<its basename>``."""
    paths, sequence = _frames(entry)
    if sequence:
        target = os.path.join(folder, label)
        mkdir_if_missing(target)
        for p in paths:
            shutil.copy(p, target)
    else:
        shutil.copy(paths[0], os.path.join(folder, '%s_name_%s' % (label, os.path.basename(paths[0]))))


def _ranked_row(q, entry, gallery, distmat, indices, topk):
    """Gallery positions to show for query position q, best first, at most topk."""
    if indices is not None:                                   # filtered upstream; negative = padding
        row = [int(g) for g in indices[q] if g >= 0]
        return row[:topk]
    pid, cam = entry[1], entry[2]
    row = []
    for g in np.argsort(distmat[q], kind='stable'):
        if len(row) == topk:
            break
        if gallery[g][1] == pid and gallery[g][2] == cam:
            continue
        row.append(int(g))
    return row


def visualize_ranked_results(distmat, query, gallery, save_dir='', visual_id=2, topk=10, indices=None):
    """For the query at position ``visual_id`` (an int, or a sequence of positions) write
    ``<save_dir>/<basename of its first frame>/`` with ``query_top000`` and ``gallery_top001`` .. ``gallery_topNNN``
    (N <= topk): folders of frames for tracklets, files ``..._name_<basename>`` for single images.  Gallery entries
    with the query's pid and camera are left out.  Prints the reference's lines.

    distmat: (num_query, num_gallery) distances, host or device; rows are ranked ascending, ties to the smaller
        index.  Not touched when ``indices`` is given (may then be None).
    query, gallery: sequences of (img_path(s), pid, camid).
    indices: optional [num_query, k] ranked gallery positions per query, host or device, ALREADY filtered (what
        engine.search(..., exclude=...) returns); negative entries are padding.  No filtering is done on them."""
    def host(a):
        return a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)
    if indices is None:
        distmat = host(distmat)
        shape = tuple(distmat.shape)
    else:
        indices = host(indices)
        shape = (len(query), len(gallery))
        if indices.ndim != 2 or indices.shape[0] != shape[0]:
            raise ValueError('indices must be [num_query, k] (got shape %s for %d queries)'
                             % (tuple(indices.shape), shape[0]))
    if shape != (len(query), len(gallery)):
        raise ValueError('distmat is %s for %d queries and %d gallery entries' % (shape, len(query), len(gallery)))
    print('Visualizing top-%d ranks' % topk)
    print('# query: %d\n# gallery %d' % shape)
    print('Saving images to "%s"' % save_dir)
    mkdir_if_missing(save_dir)
    wanted = sorted(set(int(v) for v in np.asarray(visual_id).reshape(-1)))
    for q in wanted:
        if not 0 <= q < shape[0]:                             # the reference passes over a position it does not have
            continue
        folder = os.path.join(save_dir, os.path.basename(_frames(query[q])[0][0]))
        mkdir_if_missing(folder)
        _place(query[q], folder, 'query_top000')
        for n, g in enumerate(_ranked_row(q, query[q], gallery, distmat, indices, topk), 1):
            _place(gallery[g], folder, 'gallery_top%03d' % n)
    print('Done')
