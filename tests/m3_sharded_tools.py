"""Numpy references of the row-sharded bge-m3 search (tests/test_m3_sharded_*.py): the three steps that run between the two
all-gathers, as include/rag_hip.h states them.

  merge        every rank's [Q, pool] list (ids int64, -1 padded anywhere; float64 scores) -> the [Q, k] best by (score descending,
               id ascending), -1 / 0.0 behind; nothing is normalised
  candidates   mode 0 the merged dense list; mode 1 RRF(rrf_k) of the merged dense and sparse lists, top-pool; mode 2 the same RRF
               at top_k = 2 * pool, -1 padded
  combine      each slot takes the components of the LOWEST rank whose owned flag is set; no owner or cand < 0: an empty slot;
               score = ((wc * c + ws * s) + wd * d) / ((wd + ws) + wc); stable top-k (score descending, slot ascending)

Nothing here touches the GPU or the package under test."""
import numpy as np

import m3_fused_tools as F


def merge(ids, scores, k):
    """ids int64 [L, Q, n], scores float64 [L, Q, n] -> (ids [Q, k], scores [Q, k])"""
    ids, scores = np.asarray(ids, np.int64), np.asarray(scores, np.float64)
    Q = ids.shape[1]
    out_i, out_s = np.full((Q, k), -1, np.int64), np.zeros((Q, k), np.float64)
    for q in range(Q):
        i, s = ids[:, q].reshape(-1), scores[:, q].reshape(-1)
        keep = i >= 0
        i, s = i[keep], s[keep]
        order = np.lexsort((i, -s))[:k]
        out_i[q, :order.shape[0]], out_s[q, :order.shape[0]] = i[order], s[order]
    return out_i, out_s


def rrf(lists, rrf_k, top_k):
    """lists: 1-d id arrays (-1 = padding: it holds its position, as in the library's lists) -> keys int64 [top_k], -1 padded.
    score = sum of 1 / (rrf_k + rank) in list order, ranks from 1; ties keep first-seen order."""
    score, first = {}, []
    for lst in lists:
        for rank, key in enumerate(lst, start=1):
            key = int(key)
            if key < 0:
                continue
            v = 1.0 / (rrf_k + rank)
            if key in score:
                score[key] = score[key] + v
            else:
                score[key] = v
                first.append(key)
    order = sorted(range(len(first)), key=lambda i: score[first[i]], reverse=True)[:top_k]
    out = np.full(top_k, -1, np.int64)
    out[:len(order)] = [first[i] for i in order]
    return out


def candidates(dense_ids, sparse_ids, mode, rrf_k=60):
    """merged lists [Q, pool] -> candidate ids [Q, slots]"""
    dense_ids = np.asarray(dense_ids, np.int64)
    if mode == 0:
        return dense_ids.copy()
    pool = dense_ids.shape[1]
    top_k = 2 * pool if mode == 2 else pool
    return np.stack([rrf([dense_ids[q], sparse_ids[q]], rrf_k, top_k) for q in range(dense_ids.shape[0])])


def partial(cand, lo, hi, dense=None, sparse=None, colbert=None):
    """what the rank that holds rows [lo, hi) sends: (owned bool [Q, S], components float64 [3, Q, S]); dense / sparse / colbert
    map (q, global row) -> that component, None = weight 0"""
    cand = np.asarray(cand, np.int64)
    owned = (cand >= lo) & (cand < hi)
    comp = np.zeros((3,) + cand.shape, np.float64)
    for c, fn in enumerate((dense, sparse, colbert)):
        if fn is None:
            continue
        for q, j in zip(*np.nonzero(owned)):
            comp[c, q, j] = fn(int(q), int(cand[q, j]))
    return owned, comp


def combine_topk(cand, owned, comp, weights, k):
    """cand [Q, S], owned bool [world, Q, S], comp float64 [world, 3, Q, S] -> (ids [Q, k], scores [Q, k], components [Q, k, 3])"""
    cand, owned, comp = np.asarray(cand, np.int64), np.asarray(owned, bool), np.asarray(comp, np.float64)
    Q, S = cand.shape
    has = owned.any(axis=0)
    owner = np.argmax(owned, axis=0)                                     # the first (lowest) rank that owns the slot
    qq, jj = np.meshgrid(np.arange(Q), np.arange(S), indexing="ij")
    c = comp[owner, :, qq, jj]                                           # [Q, S, 3]
    valid = has & (cand >= 0)
    score = F.combine(c[..., 0], c[..., 1], c[..., 2], weights)
    ids, sc, out = np.full((Q, k), -1, np.int64), np.zeros((Q, k), np.float64), np.zeros((Q, k, 3), np.float64)
    for q in range(Q):
        live = np.nonzero(valid[q])[0]
        order = live[np.argsort(-score[q, live], kind="stable")][:k]
        n = order.shape[0]
        ids[q, :n], sc[q, :n], out[q, :n] = cand[q, order], score[q, order], c[q, order]
    return ids, sc, out
