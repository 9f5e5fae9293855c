"""References and seeded worlds of the three-way bge-m3 score tests (tests/test_m3_fused_*.py): the point lookup in the
learned-sparse postings (rag_sparse_score_rows_*) and the fused dense + sparse + MaxSim score (rag_m3_score_rows_dev,
rag_retrieve_m3_dev).

The references ARE the contract of include/rag_hip.h. point_scores: for each slot, search every query token's posting list for
the row and add float64(qw) * float64(w) in token order. combine: ((w_colbert * colbert + w_sparse * sparse) + w_dense * dense) /
((w_dense + w_sparse) + w_colbert) in float64, the association Python gives m3_tools.combine. Nothing here touches the GPU or the
package under test."""
import numpy as np

import m3_tools as M
import sparse_tools as S
import tokvec_tools as V

N_A, V_A = 10_300, 3000                          # corpus A: five full 2048-document ranges and a short one
FIXED_ROWS = [0, 1, 2047, 2048, 4095, 4096, 8191, 8192, 10239, 10240, 10299]
DIM, TOK_DIM, POOL = 64, 64, 50
WEIGHT_SETS = ((0.4, 0.2, 0.4), (0.4, 0.2, 0.0), (1.0, 0.0, 1.0))
_A, _W = {}, {}


def corpus_a():
    """dict(indptr, doc, w, queries, packed, all = float64 [32, N_A] scores of every document), built once and read-only"""
    if not _A:
        indptr, doc, w = S.make_corpus(n_docs=N_A, n_terms=V_A, seed=5)
        queries = S.make_queries(indptr, seed=6)
        _A.update(indptr=indptr, doc=doc, w=w, queries=queries, packed=S.pack_queries(queries), all=S.all_scores(indptr, doc, w, N_A, queries))
        for a in (indptr, doc, w, _A["all"]):
            a.setflags(write=False)
    return _A


def point_scores(indptr, doc, w, n_docs, queries, cand):
    """float64 [Q, pool]: the score of the row in every slot, 0.0 for a slot < 0 or >= n_docs. One binary search per (slot, token)."""
    cand = np.asarray(cand, dtype=np.int64)
    out = np.zeros(cand.shape, dtype=np.float64)
    n_terms = indptr.shape[0] - 1
    for q, (terms, weights) in enumerate(queries):
        for j, row in enumerate(cand[q]):
            if row < 0 or row >= n_docs:
                continue
            s = np.float64(0.0)
            for t, qw in zip(terms, weights):
                if t < 0 or t >= n_terms or not (qw > 0):
                    continue
                a, e = int(indptr[t]), int(indptr[t + 1])
                p = a + int(np.searchsorted(doc[a:e], row))
                if p < e and doc[p] == row:
                    s = s + np.float64(qw) * np.float64(w[p])
            out[q, j] = s
    return out


def combine(dense, sparse, colbert, weights):
    wd, ws, wc = (np.float64(x) for x in weights)
    d, s, c = (np.asarray(a, dtype=np.float64) for a in (dense, sparse, colbert))
    return ((wc * c + ws * s) + wd * d) / ((wd + ws) + wc)


def slots_a(seed=21):
    """int32 [32, 19]: per query the fixed rows, the query's own top three sparse rows (-1 where it has fewer), three seeded random
    rows, one -1 and one N_A"""
    a = corpus_a()
    rng = np.random.default_rng(seed)
    out = []
    for q in range(len(a["queries"])):
        top, _ = S.topk(a["all"][q], 3)
        out.append(FIXED_ROWS + [int(r) for r in top] + [int(r) for r in rng.integers(0, N_A, 3)] + [-1, N_A])
    return np.asarray(out, dtype=np.int32)


def long_query():
    """300 tokens that repeat query 0's 70 terms with fresh weights: crosses the 256-token LDS chunk"""
    a = corpus_a()
    rng = np.random.default_rng(22)
    terms = np.resize(np.asarray(a["queries"][0][0]), 300)
    return terms, (rng.random(300) * 2.0).astype(np.float32) + np.float32(1e-3)


def world():
    """the world of tests/test_tokvec_gpu.py on corpus A: a 64-d index with explicit ids and tenants, 0-39 token vectors of 64 d per
    document, query 3 without token vectors; dense query i = the embedding of query i's sparse top-1 row + 0.7 x Gaussian noise"""
    if not _W:
        a = corpus_a()
        rng = np.random.default_rng(8)
        Q = len(a["queries"])
        emb = rng.standard_normal((N_A, DIM)).astype(np.float32)
        top1 = np.array([max(int(S.topk(a["all"][q], 1)[0][0]), 0) for q in range(Q)])
        q_emb = (emb[top1] + 0.7 * rng.standard_normal((Q, DIM))).astype(np.float32)
        counts = rng.integers(0, 40, N_A)
        flat = V.unit_rows(rng, int(counts.sum()), TOK_DIM)
        d_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        q_counts = [int(c) for c in rng.integers(1, 34, Q)]
        q_counts[3] = 0
        qv, qo = M.pack([V.unit_rows(rng, c, TOK_DIM) for c in q_counts], TOK_DIM)
        _W.update(emb=emb, q_emb=q_emb, d_vecs=flat, d_off=d_off, qv=qv, qo=qo, ids=(5000 + 3 * np.arange(N_A)).astype(np.int64),
                  tenants=(np.arange(N_A) % 3).astype(np.int32))
        for v in _W.values():
            v.setflags(write=False)
    return _W


def csr_of_rows(keep):
    """corpus A's postings of the documents `keep` (ascending), renumbered 0 .. len(keep) - 1"""
    a = corpus_a()
    remap = np.full(N_A, -1, dtype=np.int64)
    remap[keep] = np.arange(len(keep))
    term_of = np.repeat(np.arange(V_A, dtype=np.int64), np.diff(a["indptr"]))
    sel = remap[a["doc"]] >= 0
    indptr = np.zeros(V_A + 1, dtype=np.int64)
    np.cumsum(np.bincount(term_of[sel], minlength=V_A), out=indptr[1:])
    return indptr, remap[a["doc"][sel]].astype(np.int32), np.ascontiguousarray(a["w"][sel])


def vecs_of_rows(keep):
    w = world()
    return M.pack([w["d_vecs"][w["d_off"][i]:w["d_off"][i + 1]] for i in keep], TOK_DIM)


def cosine64(q, rows_emb):
    """numpy's float64 cosine of one float32 query against float32 rows"""
    q, r = np.asarray(q, dtype=np.float64), np.asarray(rows_emb, dtype=np.float64)
    return (r @ q) / (np.linalg.norm(q) * np.linalg.norm(r, axis=1))
