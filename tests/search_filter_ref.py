"""numpy model of the junk-filtered search contract (engine.search / engine.rerank_search with ``exclude=``,
grl_topk_block_filtered): row q of the result is the stable argsort of D[q] under grl_row_argsort's order with the
gallery entries of query q's pid AND camera deleted, truncated to k; index -1 / distance +inf pad a short row."""
import numpy as np

from search_ref import sort_key


def junk_mask(q_pids, g_pids, q_cams, g_cams):
    """[nq, ng] bool: gallery entry g is junk for query q (eva_functions.py:151-155)."""
    q_pids, g_pids = np.asarray(q_pids), np.asarray(g_pids)
    q_cams, g_cams = np.asarray(q_cams), np.asarray(g_cams)
    return (g_pids[None, :] == q_pids[:, None]) & (g_cams[None, :] == q_cams[:, None])


def filter_ranked(order, D, k, q_pids, g_pids, q_cams, g_cams, drop=None):
    """(dist [nq, k] float32, idx [nq, k] int64) from a full ranking ``order`` [nq, ng] (e.g. rank_rows(D)):
    delete junk, truncate, pad.  ``D`` [nq, ng] gives the distances at the kept indices (their own bits).
    ``drop`` [nq, ng] bool: entries that never reached the kernel (cidx < 0), deleted as well."""
    order, D = np.asarray(order).astype(np.int64), np.asarray(D, np.float32)
    nq = order.shape[0]
    junk = junk_mask(q_pids, g_pids, q_cams, g_cams)
    if drop is not None:
        junk = junk | np.asarray(drop, bool)
    idx = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), np.inf, np.float32)
    for q in range(nq):
        kept = order[q][~junk[q][order[q]]][:k]
        idx[q, :kept.size] = kept
        dist[q, :kept.size] = D[q, kept]
    return dist, idx


def filtered_topk(D, k, q_pids, g_pids, q_cams, g_cams):
    """The contract from D alone: stable argsort of the sort keys, delete junk, truncate."""
    D = np.asarray(D, np.float32)
    order = np.argsort(sort_key(D), axis=1, kind='stable')
    return filter_ranked(order, D, k, q_pids, g_pids, q_cams, g_cams)
