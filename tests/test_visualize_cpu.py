"""Ranked-results visualisation on the host (grl_amd.reid.evaluator.visualize, ATTEvaluator.evaluate(visual=1)).

visualize_ranked_results is pinned against tests/golden/visual_ranked.json: the folder the REFERENCE's function wrote
and the lines it printed for the frame tree and distance matrix of tests/visual_tree.py (recorded by
tests/golden/make_visual_golden.py).  The evaluator test replaces feature extraction and the two engine entry points
it needs by host models, so it runs without a device; tests/test_gpu_search_filter.py runs the real ones."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import search_filter_ref as F
import visual_tree as V
from grl_amd.reid.evaluator import visualize_ranked_results

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'visual_ranked.json')


@pytest.fixture(scope='module')
def recorded():
    with open(GOLDEN) as fh:
        g = json.load(fh)
    g['distmat'] = np.array(g['distmat'], dtype=np.float32)
    assert np.array_equal(g['distmat'], V.distance_matrix())            # the fixture belongs to this tree
    return g


@pytest.fixture()
def tree(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                                          # relative paths, as when recording
    return V.make_tree('frames')


def _run(run, tree, n, **kw):
    query, gallery = tree[run['scenario']]
    save_dir = os.path.join('%s%d' % (kw.pop('tag', 'out'), n), 'visual')
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        visualize_ranked_results(kw.pop('distmat', None), query, gallery, save_dir, visual_id=run['visual_id'],
                                 topk=run['topk'], **kw)
    return save_dir, buf.getvalue().splitlines()


def test_folders_and_printed_lines_equal_the_reference(recorded, tree):
    assert [(r['scenario'], r['visual_id'], r['topk']) for r in recorded['runs']] == V.RUNS
    for n, run in enumerate(recorded['runs']):
        save_dir, printed = _run(run, tree, n, distmat=recorded['distmat'])
        assert save_dir == run['save_dir']
        assert printed == run['printed'], (n, printed)
        assert V.listing(save_dir) == run['listing'], n
        # every frame is a copy of the one it is named after
        query, gallery = tree[run['scenario']]
        src = {os.path.basename(p): p for item in gallery for p in
               (item[0] if isinstance(item[0], tuple) else (item[0],))}
        for rel in run['listing']:
            p = os.path.join(save_dir, rel)
            if os.path.isfile(p):
                name = os.path.basename(p).split('_name_')[-1]
                assert open(p, 'rb').read() == open(src[name], 'rb').read()


def test_the_recorded_runs_cover_junk_padding_and_both_entry_kinds(recorded, tree):
    """What the fixture has to show: junk in front of the first kept entry, a run that asks for more than is left,
    single-image entries."""
    d = recorded['distmat']
    query, gallery = tree['video']
    qp, qc = [q[1] for q in query], [q[2] for q in query]
    gp, gc = [g[1] for g in gallery], [g[2] for g in gallery]
    junk = F.junk_mask(qp, gp, qc, gc)
    assert junk.sum(1).min() >= 1 and junk.sum(1).max() >= 2
    assert all(junk[q, int(np.argmin(d[q]))] for q in range(len(query)))          # the nearest entry is junk
    wide = [r for r in recorded['runs'] if r['topk'] > d.shape[1]]
    assert wide and any('_name_' in p for r in recorded['runs'] for p in r['listing'])
    for r in wide:
        tops = [p for p in r['listing'] if p.count('/') == 1 and 'gallery_top' in p]
        assert len(tops) == d.shape[1] - int(junk[r['visual_id']].sum())


def test_indices_give_the_same_folder_as_the_distance_matrix(recorded, tree):
    d = recorded['distmat']
    for n, run in enumerate(recorded['runs']):
        query, gallery = tree[run['scenario']]
        ids = ([q[1] for q in query], [g[1] for g in gallery], [q[2] for q in query], [g[2] for g in gallery])
        k = min(run['topk'], 16)
        _, idx = F.filtered_topk(d, k, *ids)                                     # host model of engine.search(exclude=)
        if run['topk'] > k:                                                      # a list shorter than topk: all of it
            run = dict(run, listing=[p for p in run['listing'] if 'gallery_top' not in p
                                     or int(p.split('gallery_top')[1][:3]) <= k])
        for form in (idx, torch.from_numpy(idx), idx.tolist()):
            save_dir, printed = _run(run, tree, n, indices=form, tag='idx%s' % type(form).__name__)
            assert printed[:3] == run['printed'][:3] and printed[-1] == 'Done'
            assert V.listing(save_dir) == run['listing'], n
    # padded rows (-1) end the list
    run = recorded['runs'][3]
    _, idx = F.filtered_topk(d, 30, *ids_of(tree['video']))
    assert (idx[:, -1] == -1).all()
    save_dir, _ = _run(run, tree, 99, indices=idx, tag='pad')
    assert V.listing(save_dir) == run['listing']


def ids_of(sets):
    query, gallery = sets
    return [q[1] for q in query], [g[1] for g in gallery], [q[2] for q in query], [g[2] for g in gallery]


def test_visual_id_may_be_a_sequence(recorded, tree):
    d = recorded['distmat']
    query, gallery = tree['video']
    with contextlib.redirect_stdout(io.StringIO()):
        visualize_ranked_results(d, query, gallery, 'seq/visual', visual_id=[5, 0, 3], topk=V.TOPK)
        visualize_ranked_results(d, query, gallery, 'none/visual', visual_id=[], topk=V.TOPK)
    want = sorted(p for r in recorded['runs'][:3] for p in r['listing'])
    assert V.listing('seq/visual') == want
    assert V.listing('none/visual') == []


# ----------------------------------------------------------------------------
# ATTEvaluator.evaluate(visual=1) with host stand-ins for the device work
# ----------------------------------------------------------------------------
class _Holder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def _host_engine(monkeypatch, calls):
    """engine.search and engine.rank_metrics_streaming as numpy on the host, same signatures."""
    from grl_amd import engine
    from grl_amd.reid.evaluator.eva_functions import evaluate

    def dmat(qf, gf):
        return -(qf.numpy().astype(np.float32) @ gf.numpy().astype(np.float32).T)

    def search(qf, gf, k, metric='cosine', exclude=None, block_cols=None, block_bytes=None):
        calls.append(('search', k, exclude is not None))
        dist, idx = F.filtered_topk(dmat(qf, gf), k, *exclude)
        return torch.from_numpy(dist), torch.from_numpy(idx)

    def rank_metrics_streaming(qf, gf, q_pids, g_pids, q_camids, g_camids, **kw):
        return evaluate(dmat(qf, gf), q_pids, g_pids, q_camids, g_camids)
    monkeypatch.setattr(engine, 'search', search)
    monkeypatch.setattr(engine, 'rank_metrics_streaming', rank_metrics_streaming)


def test_evaluate_with_visual_writes_the_folder_and_returns_the_same_rank1(tree, monkeypatch, tmp_path):
    from grl_amd.reid.evaluator import ATTEvaluator
    query, gallery = tree['video']
    nq, ng = len(query), len(gallery)
    rng = np.random.RandomState(4)
    centres = rng.standard_normal((20, 32)).astype(np.float32)

    def feats(items):
        x = np.stack([centres[pid + 1] for _, pid, _ in items]) + 0.8 * rng.standard_normal((len(items), 32))
        x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
        return torch.from_numpy(x), np.array([i[1] for i in items]), np.array([i[2] for i in items])
    table = {'q': feats(query), 'g': feats(gallery)}
    ev = ATTEvaluator(_Holder(), _Holder(), only_eval=False)
    monkeypatch.setattr(ev, 'extract_feature', lambda loader: table[loader])
    calls = []
    _host_engine(monkeypatch, calls)
    monkeypatch.setenv('GRL_EVAL_STREAM', '1')
    monkeypatch.delenv('GRL_EVAL_RERANK', raising=False)
    monkeypatch.delenv('GRL_VISUAL_QUERIES', raising=False)

    def run(visual, path):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            r1 = ev.evaluate(query, gallery, 'q', 'g', path, visual, 0)
        return r1, buf.getvalue()
    r_plain, out_plain = run(0, 'log/a_')
    assert not calls and not os.path.exists('log')
    os.makedirs('log')
    r_vis, out_vis = run(1, 'log/a_')
    assert r_vis == r_plain and calls == [('search', 10, True)]
    metric_lines = [l for l in out_plain.splitlines() if l.startswith(('Mean AP', 'Rank-'))]
    assert len(metric_lines) == 5 and metric_lines == [l for l in out_vis.splitlines()
                                                       if l.startswith(('Mean AP', 'Rank-'))]
    assert 'Visualizing top-10 ranks' in out_vis and 'Saving images to "log/a_visual"' in out_vis

    # the lists: filtered top-10 of the query-prepended gallery; positions below nq are the queries themselves
    qf, qp, qc = table['q']
    gf = torch.cat((qf, table['g'][0]), 0)
    gp, gc = np.append(qp, table['g'][1]), np.append(qc, table['g'][2])
    dist, idx = F.filtered_topk(-(qf.numpy() @ gf.numpy().T), 10, qp, gp, qc, gc)
    ranked = json.load(open('log/a_visual/ranked.json'))
    assert list(ranked) == ['4']                                                 # the reference's visual_id
    assert ranked['4'] == [[int(g), int(gp[g]), int(gc[g]), float(d)] for g, d in zip(idx[4], dist[4])]
    everything = list(query) + list(gallery)
    qdir = os.path.basename(query[4][0][0])
    got = V.listing('log/a_visual')
    assert 'ranked.json' in got and qdir in got and qdir + '/query_top000' in got
    for rank, g in enumerate(idx[4], 1):
        assert not (gp[g] == qp[4] and gc[g] == qc[4])
        names = sorted(p.rsplit('/', 1)[1] for p in got if p.startswith('%s/gallery_top%03d/' % (qdir, rank)))
        assert names == sorted(os.path.basename(p) for p in everything[g][0]), rank
    assert not any('gallery_top011' in p for p in got)

    # GRL_VISUAL_QUERIES: a comma list of query positions
    monkeypatch.setenv('GRL_VISUAL_QUERIES', '0, 5')
    r_two, _ = run(1, 'log/b_')
    assert r_two == r_plain
    assert sorted(json.load(open('log/b_visual/ranked.json'))) == ['0', '5']
    tops = [p for p in V.listing('log/b_visual') if p.count('/') == 0 and p != 'ranked.json']
    assert sorted(tops) == sorted(os.path.basename(query[q][0][0]) for q in (0, 5))

    # a position the query list does not have is skipped with a note; a non-integer names the variable
    monkeypatch.setenv('GRL_VISUAL_QUERIES', '2,17,-1')
    r_note, out_note = run(1, 'log/d_')
    assert r_note == r_plain and 'GRL_VISUAL_QUERIES: no query at position(s) -1, 17' in out_note
    assert sorted(json.load(open('log/d_visual/ranked.json'))) == ['2']
    monkeypatch.setenv('GRL_VISUAL_QUERIES', '2,x')
    with pytest.raises(ValueError, match='GRL_VISUAL_QUERIES'):
        run(1, 'log/e_')
    monkeypatch.setenv('GRL_VISUAL_QUERIES', '4')

    with pytest.raises(ValueError, match='tuple lists'):
        ev.evaluate(None, None, 'q', 'g', 'log/c_', 1, 0)
