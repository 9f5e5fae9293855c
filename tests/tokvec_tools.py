"""Float64 reference of the resident token-vector store's rerank (rag_tokvec_*; tests/test_tokvec_*.py).

The reference IS the contract of include/rag_hip.h: a slot's score is m3_tools.maxsim of the query's rows against the candidate
document's rows; a slot with cand < 0, a row at or past the store's documents, a document without rows or a query without rows
scores 0.0 and is EMPTY; the top-k is a stable order (score descending, candidate position ascending) over the slots that are not
empty, padded with -1 / 0.0. Nothing here touches the GPU or the package under test."""
import numpy as np

import m3_tools as M


def fp16_round(x):
    """what the store keeps of float32 vectors: round to nearest even to fp16, read back as float32"""
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def unit_rows(rng, n, dim):
    v = rng.standard_normal((n, dim))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def slot_empty(q_off, d_off, cand):
    """bool [Q, pool]: the slots the rules above leave out"""
    q_off, d_off, cand = np.asarray(q_off, np.int64), np.asarray(d_off, np.int64), np.asarray(cand, np.int64)
    n_docs = d_off.shape[0] - 1
    nq = np.diff(q_off)[:, None]
    ok = (cand >= 0) & (cand < n_docs)
    nd = np.where(ok, np.diff(d_off)[np.clip(cand, 0, max(n_docs - 1, 0))] if n_docs else 0, 0)
    return ~ok | (nd <= 0) | (nq <= 0)


def pair_scores(q_vecs, q_off, d_vecs, d_off, cand):
    """float64 [Q, pool]: MaxSim of every slot over the GIVEN vectors (stored or original), 0.0 for an empty slot"""
    cand = np.asarray(cand, np.int64)
    empty = slot_empty(q_off, d_off, cand)
    out = np.zeros(cand.shape, dtype=np.float64)
    for q in range(cand.shape[0]):
        vq = q_vecs[int(q_off[q]):int(q_off[q + 1])]
        for j in range(cand.shape[1]):
            if not empty[q, j]:
                d = int(cand[q, j])
                out[q, j] = M.maxsim(vq, d_vecs[int(d_off[d]):int(d_off[d + 1])])
    return out


def stable_topk(scores, cand, empty, k, idmap=None, id_base=0, n_index=None):
    """(ids int64 [Q, k], rows int32 [Q, k], scores float64 [Q, k]) of a [Q, pool] score table: score descending, equal scores in
    candidate order, empty slots skipped, -1 / -1 / 0.0 behind. ids = idmap[row] or id_base + row; with an index of n_index rows a
    scored row it does not have gets id -1 (its row is still returned)."""
    scores, cand = np.asarray(scores, np.float64), np.asarray(cand, np.int64)
    Q = cand.shape[0]
    ids, rows, sc = np.full((Q, k), -1, np.int64), np.full((Q, k), -1, np.int32), np.zeros((Q, k), np.float64)
    for q in range(Q):
        live = np.nonzero(~empty[q])[0]
        order = live[np.argsort(-scores[q, live], kind="stable")][:k]
        n = order.shape[0]
        rows[q, :n] = cand[q, order]
        sc[q, :n] = scores[q, order]
        ids[q, :n] = [-1 if n_index is not None and r >= n_index else int(idmap[r]) if idmap is not None else id_base + int(r)
                      for r in cand[q, order]]
    return ids, rows, sc


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
