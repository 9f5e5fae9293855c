"""The world and the truth of the exhaustive MaxSim search (mode 2 of rag_retrieve_maxsim_dev; tests/test_tokvec_search_*.py).

The contract (include/rag_hip.h): for each query the top-`pool` of score[q][d] over every document d the query may see - not
deleted, of the query's tenant when one is given - score descending, the lower row first on equal scores; a document without rows
and a query without rows are never listed; ids / scores [Q][k] are the first k of that list, cand [Q][pool] all of it, padding
-1 / 0.0. The truth is built from a [Q][N] float32 matrix of pair scores - the tests fill it with rag_tokvec_rerank's own
pair_scores_out over ALL rows, in slices of at most 256 candidates - the visibility mask, and a numpy stable sort. numpy only:
nothing here touches the GPU or the package under test."""
import numpy as np

import tokvec_tools as V

N_DOCS, INDEX_DIM = 700, 64
DIMS = (96, 128)                                        # 96: an odd number of K-steps for the 8-bit form's two-step loop
EDGE_ROWS = (0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255)      # the tile edges and the 8-tile switch between the instantiations
Q_ROWS = (0, 1, 16, 17, 32, 33, 40, 64, 5)
SRC, COPIES = 20, (300, 699)                            # exact ties: two copies of document 20, one of them the store's last
Q_NEAR = (4, 5)                                         # queries cut from document 20's own rows: the three tie at the top
PER_QUERY = np.array([(-1, 0, 1, 2)[i % 4] for i in range(len(Q_ROWS))], dtype=np.int32)
LAST_PLAIN = 698                                        # the last row that is not a copy
_WORLDS = {}


def doc_rows(rng):
    """row counts: three passes over EDGE_ROWS, each shifted by one so that every count lands in every tenant (row % 3), then
    1 - 60 at random; the copies take their source's count"""
    n_edge = 3 * len(EDGE_ROWS)
    counts = [EDGE_ROWS[(i + i // len(EDGE_ROWS)) % len(EDGE_ROWS)] for i in range(n_edge)]
    counts += [int(c) for c in rng.integers(1, 61, N_DOCS - n_edge)]
    for c in COPIES:
        counts[c] = counts[SRC]
    return counts


def world(dim):
    """dict(vecs [rows, dim] float32 unit rows, off int64 [N + 1], qv, qo, emb [N, INDEX_DIM], q_emb, tenants int32 [N])"""
    if dim not in _WORLDS:
        rng = np.random.default_rng(1000 + dim)
        counts = doc_rows(rng)
        assert counts[SRC] == 128 and len(counts) == N_DOCS
        docs = [V.unit_rows(rng, c, dim) for c in counts]
        for c in COPIES:
            docs[c] = docs[SRC].copy()
        off = np.zeros(N_DOCS + 1, dtype=np.int64)
        off[1:] = np.cumsum(counts)
        queries = [V.unit_rows(rng, c, dim) for c in Q_ROWS]
        queries[Q_NEAR[0]] = docs[SRC][:Q_ROWS[Q_NEAR[0]]].copy()
        queries[Q_NEAR[1]] = docs[SRC][10:10 + Q_ROWS[Q_NEAR[1]]].copy()
        qo = np.zeros(len(Q_ROWS) + 1, dtype=np.int64)
        qo[1:] = np.cumsum(Q_ROWS)
        _WORLDS[dim] = dict(vecs=np.ascontiguousarray(np.concatenate(docs)), off=off, qv=np.ascontiguousarray(np.concatenate(queries)), qo=qo,
                            emb=rng.standard_normal((N_DOCS, INDEX_DIM)).astype(np.float32),
                            q_emb=rng.standard_normal((len(Q_ROWS), INDEX_DIM)).astype(np.float32),
                            tenants=(np.arange(N_DOCS) % 3).astype(np.int32))
    return _WORLDS[dim]


def slices(n_docs, width=256):
    """every row of the store as candidate lists of at most `width`: [(first row, count), ...]"""
    return [(a, min(width, n_docs - a)) for a in range(0, n_docs, width)]


def ranked(q_off, d_off, tenants, deleted, q_tenants):
    """bool [Q, N]: the pairs the search ranks. q_tenants: an int for every query, or one number per query (< 0: no filter)."""
    q_off, d_off = np.asarray(q_off, np.int64), np.asarray(d_off, np.int64)
    Q, N = q_off.shape[0] - 1, d_off.shape[0] - 1
    qt = np.broadcast_to(np.asarray(q_tenants, dtype=np.int64).reshape(-1), (Q,)) if np.ndim(q_tenants) else np.full(Q, int(q_tenants))
    alive = np.ones(N, dtype=bool)
    alive[np.asarray(list(deleted), dtype=np.int64)] = False
    see = alive[None, :] & ((qt[:, None] < 0) | (np.asarray(tenants)[None, :] == qt[:, None]))
    return see & (np.diff(d_off) > 0)[None, :] & (np.diff(q_off) > 0)[:, None]


def truth(scores, mask, pool, k, ids=None):
    """(ids int64 [Q, k], scores float64 [Q, k], cand int64 [Q, pool]) of a [Q, N] float32 score matrix and the ranked mask:
    score descending, lower row first on equal scores (a stable sort over the rows in order), -1 / 0.0 behind"""
    scores = np.asarray(scores, dtype=np.float32)
    Q = scores.shape[0]
    out_ids, out_sc, cand = np.full((Q, k), -1, np.int64), np.zeros((Q, k), np.float64), np.full((Q, pool), -1, np.int64)
    for q in range(Q):
        rows = np.nonzero(mask[q])[0]
        order = rows[np.argsort(-scores[q, rows].astype(np.float64), kind="stable")][:pool]
        named = order if ids is None else np.asarray(ids, np.int64)[order]
        cand[q, :order.shape[0]] = named
        n = min(k, order.shape[0])
        out_ids[q, :n] = named[:n]
        out_sc[q, :n] = scores[q, order[:n]].astype(np.float64)
    return out_ids, out_sc, cand


def truth_loops(scores, mask, pool, k):
    """the same by a plain double loop: pick the best remaining pair `pool` times (for the CPU check of truth())"""
    Q, N = mask.shape
    out_ids, out_sc, cand = np.full((Q, k), -1, np.int64), np.zeros((Q, k), np.float64), np.full((Q, pool), -1, np.int64)
    for q in range(Q):
        taken = set()
        for slot in range(pool):
            best = -1
            for d in range(N):
                if mask[q, d] and d not in taken and (best < 0 or float(scores[q, d]) > float(scores[q, best])):
                    best = d
            if best < 0:
                break
            taken.add(best)
            cand[q, slot] = best
            if slot < k:
                out_ids[q, slot], out_sc[q, slot] = best, float(scores[q, best])
    return out_ids, out_sc, cand
