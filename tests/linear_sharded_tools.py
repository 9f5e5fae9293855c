"""TEST INFRASTRUCTURE of tests/test_linear_sharded_*.py: ONE small world (numpy only, built once per process) for the linear
fusion over row shards, and the numpy statement of what the library must compute.

The world: 4,600 rows x dim 64 (three 2048-document BM25 ranges unsharded), cut into three unequal contiguous shards, the last
with fewer rows than k. A vocabulary of 300 terms: 5 long posting lists (1,000 - 2,600 documents), 55 medium ones (40 - 400) and
240 short ones (1 - 11 postings). 28 queries, k = 10. Built in on purpose:
  query 0   every term out of vocabulary (-1): no raw score anywhere, divisor 1.0 on every rank
  query 1   one term whose postings all lie in shard 1
  query 2   aims at rows 100 (shard 0) and 3000 (shard 1), which are duplicates in every plane: an exact hybrid tie across shards
  tenants   row % 3, except that tenant 2 owns no row of the last shard (and the duplicate rows share tenant 1)
  deleted   a handful of rows on every shard, the best BM25 document of query 3 among them
The fusion itself is CPython's operation order, rag/retrieval.py:302: (alpha * sem + beta * raw / max) + gamma * temporal."""
import numpy as np

from oracle import rag_oracle as O

N, D, Q, K = 4600, 64, 28, 10
BOUNDS = ((0, 2100), (2100, 4594), (4594, N))
N_TERMS = 300
TIE = (100, 3000)
ONE_SHARD_TERM = 299
WEIGHTS = (0.55, 0.35, 0.10)
_W = {}


def postings():
    from optimized_rag_amd.bm25 import Bm25Postings
    w = world()
    return Bm25Postings(w["indptr"], w["doc"], w["tf"], w["doc_len"], w["idf"], w["avgdl"])


def world():
    if _W:
        return _W
    from optimized_rag_amd.bm25 import Bm25Postings
    rng = np.random.default_rng(20261)
    emb = rng.standard_normal((N, D)).astype(np.float32)
    temporal = np.where(rng.uniform(size=N) < 0.4, 0.15 * 0.5 ** (rng.uniform(0, 90, N) / 30.0), 0.0)
    doc_len = rng.integers(5, 40, N).astype(np.int32)
    # document-major first, so that a duplicate document is one copy; then inverted to the term-major CSR
    sizes = np.concatenate([rng.integers(1000, 2600, 5), rng.integers(40, 400, 55), rng.integers(1, 12, 240)])
    has = np.zeros((N_TERMS, N), np.int32)                              # term frequency of (term, document), 0 = absent
    for t in range(N_TERMS):
        d = rng.choice(N, int(sizes[t]), replace=False)
        has[t, d] = rng.integers(1, 4, d.shape[0])
    lo1, hi1 = BOUNDS[1]
    has[ONE_SHARD_TERM] = 0
    has[ONE_SHARD_TERM, [lo1 + 400, lo1 + 500, hi1 - 7]] = (2, 1, 3)
    a, b = TIE
    emb[b], temporal[b], doc_len[b], has[:, b] = emb[a], temporal[a], doc_len[a], has[:, a]
    has[[7, 80], a] = has[[7, 80], b] = (2, 1)                           # both carry the terms query 2 asks for
    indptr = np.zeros(N_TERMS + 1, np.int64)
    np.cumsum((has > 0).sum(axis=1), out=indptr[1:])
    t_idx, d_idx = np.nonzero(has)                                      # term-major, documents ascending
    doc, tf = d_idx.astype(np.int32), has[t_idx, d_idx].astype(np.int32)
    idf = Bm25Postings.idf_table(np.diff(indptr), N)
    avgdl = float(doc_len.sum()) / N
    tenants = (np.arange(N) % 3).astype(np.int32)
    tenants[BOUNDS[2][0]:] = np.arange(N - BOUNDS[2][0]) % 2            # tenant 2 owns nothing on the last shard
    tenants[b] = tenants[a]
    # queries: 1 - 4 terms over the three list classes, repeats and an unknown term among them
    terms_of = [[-1, -1], [ONE_SHARD_TERM], [7, 80]]
    while len(terms_of) < Q:
        n = int(rng.integers(1, 5))
        t = [int(rng.choice([rng.integers(0, 5), rng.integers(5, 60), rng.integers(60, N_TERMS)])) for _ in range(n)]
        if len(terms_of) % 9 == 0:
            t.append(-1)
        if len(terms_of) % 7 == 0:
            t.append(t[0])
        terms_of.append(t)
    ptr = np.cumsum([0] + [len(t) for t in terms_of]).astype(np.int32)
    terms = np.asarray([x for t in terms_of for x in t], np.int32)
    q_emb = (emb[rng.integers(0, N, Q)] + 0.6 * rng.standard_normal((Q, D))).astype(np.float32)
    q_emb[2] = emb[a]
    raw = np.stack([O.bm25_scores_csr(indptr, doc, tf, doc_len, idf, avgdl, t) for t in terms_of])
    deleted = np.array(sorted({5, 2047, 2048, lo1 + 1, hi1 - 1, N - 3, int(np.argmax(raw[3]))}), np.int64)
    assert not set(deleted.tolist()) & set(TIE)
    visible = np.ones(N, bool)
    visible[deleted] = False
    tenant_q = np.array([(-1, 0, 1, 2)[i % 4] for i in range(Q)], np.int32)      # the per-query tenant array of the tests
    tenant_q[2] = 1
    _W.update(emb=emb, temporal=temporal, doc_len=doc_len, indptr=indptr, doc=doc, tf=tf, idf=idf, avgdl=avgdl, tenants=tenants,
              terms_of=terms_of, ptr=ptr, terms=terms, q_emb=q_emb, raw=raw, deleted=deleted, visible=visible, tenant_q=tenant_q)
    return _W


def cosines(q_emb, emb):
    """float64 cosine of every (query, row): each row's sums are formed from that row alone, so a slice of rows gives the bits of
    the whole."""
    e, q = emb.astype(np.float64), q_emb.astype(np.float64)
    dots = np.stack([np.add.reduce(e * q[i], axis=1) for i in range(q.shape[0])])
    ne, nq = np.sqrt(np.add.reduce(e * e, axis=1)), np.sqrt(np.add.reduce(q * q, axis=1))
    return dots / (nq[:, None] * ne[None, :])


def seen(tenant, lo=0, hi=N, deleted=True):
    """[Q, hi - lo] bool: the rows query q may see. tenant: an int or one number per query, < 0 = not filtered."""
    w = world()
    t = np.broadcast_to(np.asarray(tenant, np.int32), (Q,))
    m = (t[:, None] < 0) | (w["tenants"][None, lo:hi] == t[:, None])
    return m & w["visible"][None, lo:hi] if deleted else m


def local_max(raw, mask):
    """[Q] largest raw score over the rows a query sees, -inf without one"""
    return np.where(mask, raw, -np.inf).max(axis=1) if raw.shape[1] else np.full(raw.shape[0], -np.inf)


def divisor(mx):
    """rag/retrieval.py:343-344: the maximum when it is > 0, else 1.0 (-inf = no document included)"""
    return np.where(mx > 0, mx, 1.0)


def fuse_topk(sem, raw, temporal, mask, div, weights, k, id_base=0):
    """The fusion over the given rows with the given per-query divisor -> (ids, hybrid, semantic, keyword, temporal), each [Q, k],
    (hybrid desc, row asc), -1 / 0.0 padded."""
    a, b, g = weights
    kw = raw / div[:, None]
    hyb = (a * sem + b * kw) + g * temporal[None, :]
    ids = np.full((sem.shape[0], k), -1, np.int64)
    out = np.zeros((4, sem.shape[0], k))
    for q in range(sem.shape[0]):
        rows = np.nonzero(mask[q])[0]
        top = rows[np.lexsort((rows, -hyb[q, rows]))[:k]]
        ids[q, :len(top)] = id_base + top
        out[0, q, :len(top)], out[1, q, :len(top)], out[2, q, :len(top)] = hyb[q, top], sem[q, top], kw[q, top]
        out[3, q, :len(top)] = temporal[top]
    return (ids,) + tuple(out)


def merge(parts, k):
    """parts: per shard (ids, hybrid, semantic, keyword, temporal) -> the same five arrays of the global top-k: hybrid desc, id
    asc, -1 skipped wherever it stands, the components carried with their row."""
    ids = np.concatenate([p[0] for p in parts], axis=1)
    planes = [np.concatenate([p[i] for p in parts], axis=1) for i in range(1, 5)]
    o_ids = np.full((ids.shape[0], k), -1, np.int64)
    out = np.zeros((4, ids.shape[0], k))
    for q in range(ids.shape[0]):
        live = np.nonzero(ids[q] >= 0)[0]
        top = live[np.lexsort((ids[q, live], -planes[0][q, live]))[:k]]
        o_ids[q, :len(top)] = ids[q, top]
        for i in range(4):
            out[i, q, :len(top)] = planes[i][q, top]
    return (o_ids,) + tuple(out)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def assert_same(got, exp, what=""):
    """got / exp: (ids, hybrid, semantic, keyword, temporal); ids equal, the four float64 planes equal as bits"""
    np.testing.assert_array_equal(got[0], exp[0], err_msg=f"{what} ids")
    for i, name in enumerate(("hybrid", "semantic", "keyword", "temporal"), 1):
        np.testing.assert_array_equal(bits(got[i]), bits(exp[i]), err_msg=f"{what} {name}")


NAMES = ("ids", "hybrid", "semantic", "keyword", "temporal")


# ---- GPU side (imported lazily: the CPU test uses only what is above) -------------------------------------------------------------
def load_handle(eng, lo, hi, temporal=True, tenants=True, deleted=True, sharded=None):
    """Rows [lo, hi) of the world on one handle under id_base = lo: through ShardedHybridIndex.load_shard when `sharded` (the
    index object) is given, else the plain engine calls of the unsharded truth."""
    w = world()
    post = postings().shard(lo, hi)
    t = np.ascontiguousarray(w["temporal"][lo:hi]) if temporal else None
    if sharded is not None:
        sharded.load_shard(np.ascontiguousarray(w["emb"][lo:hi]), lo, post, temporal=t)
    else:
        eng.index_load(np.ascontiguousarray(w["emb"][lo:hi]), id_base=lo)
        post.load(eng)
        eng.set_temporal(t)
    if tenants:
        eng.set_tenants(np.ascontiguousarray(w["tenants"][lo:hi]))
    if deleted:
        mine = w["deleted"][(w["deleted"] >= lo) & (w["deleted"] < hi)]
        assert eng.index_delete(mine) == len(mine)
    return eng


def query_tensors(device="cuda"):
    import torch
    w = world()
    return tuple(torch.from_numpy(np.ascontiguousarray(w[n])).to(device) for n in ("q_emb", "ptr", "terms"))


def as_np(out):
    """dict of tensors (hybrid_linear_dev / search_linear) -> the five arrays, copied to the host"""
    return tuple(out[n].cpu().numpy().copy() for n in NAMES)
