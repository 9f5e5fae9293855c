"""GPU: live writes to the resident index (rag_index_insert_host / rag_index_delete_host / rag_index_compact).

After any sequence of writes a search must equal the exact scan over the LIVE rows (the oracle models a deleted row as a row of
no tenant) and, bit for bit, the same call on a fresh handle loaded with only the live rows in row order."""
import ctypes

import numpy as np
import pytest

from oracle import rag_oracle as O

pytestmark = pytest.mark.gpu

D = 256
NO = -7                    # oracle tenant of a deleted row


@pytest.fixture(scope="module")
def make():
    from optimized_rag_amd import RagEngine
    made = []

    def mk():
        e = RagEngine(dim=D, device=0)
        made.append(e)
        return e

    yield mk
    for e in made:
        e.close()


class Model:
    """What the SQL table holds: every row the engine stores, in row order, with its id / tenant / live flag."""

    def __init__(self, emb, ids, ten):
        self.emb, self.ids, self.ten = emb.copy(), ids.copy(), ten.copy()
        self.live = np.ones(len(ids), dtype=bool)

    def insert(self, emb, ids, ten):
        self.emb = np.concatenate([self.emb, emb])
        self.ids = np.concatenate([self.ids, ids])
        self.ten = np.concatenate([self.ten, ten])
        self.live = np.concatenate([self.live, np.ones(len(ids), dtype=bool)])

    def delete(self, ids, tenant=-1):
        hit = np.isin(self.ids, ids) & self.live & ((self.ten == tenant) if tenant >= 0 else True)
        self.live &= ~hit
        return int(hit.sum())

    def oracle(self, q, k, tenant=-1):
        tor = np.where(self.live, self.ten if tenant >= 0 else 0, NO)
        rows, sc = O.dense_topk(self.emb, q, k, tor, tenant if tenant >= 0 else 0)
        return np.where(rows >= 0, self.ids[np.maximum(rows, 0)], -1), rows, sc


def fresh_of(make, m, tenants=True):
    f = make()
    lv = np.nonzero(m.live)[0]
    f.index_load(m.emb[lv], ids=m.ids[lv])
    if tenants and len(lv):
        f.set_tenants(m.ten[lv])
    return f, lv


def check(eng, m, q, k, tenant=-1, fresh=None):
    ids, rows, sc = eng.dense_topk(q, k, tenant=tenant)
    oid, orow, osc = m.oracle(q, k, tenant)
    np.testing.assert_array_equal(ids, oid)
    np.testing.assert_array_equal(rows, orow.astype(np.int32))
    assert np.abs(sc - osc).max() < 1e-9
    if fresh is not None:
        f, lv = fresh
        fid, frow, fsc = f.dense_topk(q, k, tenant=tenant)
        np.testing.assert_array_equal(fid, ids)
        np.testing.assert_array_equal(fsc.view(np.int64), sc.view(np.int64))          # score bits
        np.testing.assert_array_equal(np.where(frow >= 0, lv[np.maximum(frow, 0)], -1), rows)


def queries(rng, m, Q):
    src = m.emb[rng.integers(0, len(m.ids), Q)]
    return (src + 0.4 * rng.standard_normal((Q, D))).astype(np.float32)


OPTIONS = [{}, {"force_level": 1}, {"force_level": 2}, {"no_second_pass": 1}, {"no_smallq": 1}, {"dense_persist": 1}]


@pytest.mark.parametrize("opts", OPTIONS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) or "default")
def test_mixed_writes_vs_oracle_and_fresh_handle(make, opts):
    rng = np.random.default_rng(7)
    n0, T = 3000, 5
    emb = rng.standard_normal((n0, D)).astype(np.float32)
    ids = rng.permutation(10 * n0)[:n0].astype(np.int64) + 1000
    ten = rng.integers(0, T, n0).astype(np.int32)
    eng = make()
    for k_, v in opts.items():
        eng.set_option(k_, v)
    eng.index_load(emb, ids=ids)
    eng.set_tenants(ten)
    m = Model(emb, ids, ten)
    next_id = 10 * n0 + 5000
    for rnd in range(24):
        op = rnd % 3
        if op == 0:                                        # insert: fresh vectors, duplicates of live rows, zero rows, new tenants
            n = int(rng.choice([1, 7, 300, 1500]))
            e = rng.standard_normal((n, D)).astype(np.float32)
            dup = rng.random(n) < 0.2
            e[dup] = m.emb[rng.integers(0, len(m.ids), int(dup.sum()))]
            e[rng.random(n) < 0.02] = 0.0
            new_ids = np.arange(next_id, next_id + n, dtype=np.int64)[rng.permutation(n)]
            next_id += n
            t = rng.integers(0, T + rnd // 3, n).astype(np.int32)
            first = eng.index_insert(e, ids=new_ids, tenants=t)
            assert first == len(m.ids)
            m.insert(e, new_ids, t)
        elif op == 1:                                      # delete: live, already deleted, unknown ids; sometimes a tenant predicate
            pick = m.ids[rng.integers(0, len(m.ids), int(rng.choice([1, 50, 600])))]
            pick = np.concatenate([pick, [-5, 10 ** 12]])
            tenant = int(rng.integers(0, T)) if rng.random() < 0.3 else -1
            assert eng.index_delete(pick, tenant=tenant) == m.delete(pick, tenant)
        Q = int(rng.choice([1, 64, 300]))
        k = int(rng.choice([1, 20, 100, 256]))
        tenant = int(rng.integers(0, T + 2)) if rng.random() < 0.4 else -1
        check(eng, m, queries(rng, m, Q), k, tenant)
    assert eng.index_deleted_rows() == int((~m.live).sum())
    fr = fresh_of(make, m)
    for Q, k, tenant in ((1, 20, -1), (64, 100, -1), (300, 256, 2), (64, 20, 0)):
        check(eng, m, queries(rng, m, Q), k, tenant, fresh=fr)


def test_overflowing_duplicate_cluster_after_deletes(make):
    """5000 copies of one vector: every candidate buffer overflows (second pass / float64 scan) - deleted copies must stay out."""
    rng = np.random.default_rng(3)
    base = rng.standard_normal((4000, D)).astype(np.float32)
    v = rng.standard_normal(D).astype(np.float32)
    emb = np.concatenate([base, np.repeat(v[None], 5000, 0)])
    ids = np.arange(len(emb), dtype=np.int64) * 3 + 11
    eng = make()
    eng.index_load(emb, ids=ids)
    m = Model(emb, ids, np.zeros(len(ids), dtype=np.int32))
    dele = ids[4000:][rng.permutation(5000)[:3000]]
    assert eng.index_delete(dele) == m.delete(dele) == 3000
    q = np.concatenate([v[None], v[None] + 0.01 * rng.standard_normal((3, D))]).astype(np.float32)
    for k in (20, 256):
        check(eng, m, q, k, fresh=fresh_of(make, m, tenants=False))


def test_zero_query_after_deleting_first_rows(make):
    eng = make()
    rng = np.random.default_rng(1)
    eng.index_load(rng.standard_normal((30, D)).astype(np.float32))
    assert eng.index_delete(np.arange(10)) == 10
    ids, rows, sc = eng.dense_topk(np.zeros((1, D), np.float32), 20)
    np.testing.assert_array_equal(rows[0], np.arange(10, 30))
    np.testing.assert_array_equal(ids[0], np.arange(10, 30))
    assert (sc == 0.0).all()


def test_compaction_keeps_results_ids_and_maps_rows(make):
    rng = np.random.default_rng(11)
    n0 = 9000
    emb = rng.standard_normal((n0, D)).astype(np.float32)
    ten = rng.integers(0, 4, n0).astype(np.int32)
    eng = make()
    eng.index_load(emb, id_base=500)                         # implicit ids 500 + row
    eng.set_tenants(ten)
    eng.set_temporal(rng.random(n0))
    eng.index_insert(rng.standard_normal((100, D)).astype(np.float32), tenants=np.full(100, 9, np.int32),
                     temporal=rng.random(100))              # implicit ids kept: 500 + 9000 ...
    m = Model(np.concatenate([emb, eng.fetch_rows(np.arange(n0, n0 + 100))]), np.arange(n0 + 100, dtype=np.int64) + 500,
              np.concatenate([ten, np.full(100, 9, np.int32)]))
    dele = m.ids[rng.random(len(m.ids)) < 0.3]
    assert eng.index_delete(dele) == m.delete(dele)
    q = queries(rng, m, 64)
    before = [eng.dense_topk(q, k, tenant=t) for k, t in ((20, -1), (100, 9), (256, 1))]
    row_map = eng.index_compact()
    lv = np.nonzero(m.live)[0]
    exp_map = np.full(len(m.ids), -1, np.int64)
    exp_map[lv] = np.arange(len(lv))
    np.testing.assert_array_equal(row_map, exp_map)
    assert eng.index_deleted_rows() == 0 and eng.n_rows == len(lv)
    for (k, t), (bi, br, bs) in zip(((20, -1), (100, 9), (256, 1)), before):
        ai, ar, as_ = eng.dense_topk(q, k, tenant=t)
        np.testing.assert_array_equal(ai, bi)                                      # ids never change
        np.testing.assert_array_equal(as_.view(np.int64), bs.view(np.int64))
        np.testing.assert_array_equal(ar, np.where(br >= 0, row_map[np.maximum(br, 0)], -1))
    np.testing.assert_array_equal(eng.fetch_rows(np.arange(len(lv))), m.emb[lv])
    # the explicit-id column survives further writes: delete by the implicit ids, insert with new ones
    assert eng.index_delete(m.ids[lv[:5]]) == 5
    m2 = Model(m.emb[lv], m.ids[lv], m.ten[lv])
    m2.delete(m.ids[lv[:5]])
    check(eng, m2, q, 50)


def test_failed_insert_leaves_the_index_unchanged(make):
    from optimized_rag_amd import RagError
    rng = np.random.default_rng(5)
    emb = rng.standard_normal((2000, D)).astype(np.float32)
    eng = make()
    eng.index_load(emb, ids=np.arange(2000, dtype=np.int64) + 1)
    eng.set_tenants(np.zeros(2000, np.int32))
    q = emb[:8] + 0.1
    before = eng.dense_topk(q, 30)
    e = rng.standard_normal((3, D)).astype(np.float32)
    with pytest.raises(RagError):                            # id 7 is live
        eng.index_insert(e, ids=np.array([5000, 7, 5001]), tenants=np.zeros(3, np.int32))
    with pytest.raises(RagError):                            # repeated inside the block
        eng.index_insert(e, ids=np.array([5000, 5000, 5001]), tenants=np.zeros(3, np.int32))
    with pytest.raises(RagError):                            # the tenant plane is missing
        eng.index_insert(e, ids=np.array([5000, 5002, 5001]))
    n = ctypes.c_int64()
    eng.lib.rag_index_rows(eng.h, ctypes.byref(n))
    assert n.value == 2000
    after = eng.dense_topk(q, 30)
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    # a deleted id may come back
    assert eng.index_delete([7]) == 1
    eng.index_insert(e[:1], ids=np.array([7]), tenants=np.zeros(1, np.int32))


def test_insert_on_a_handle_without_index_and_into_reserved_capacity(make):
    rng = np.random.default_rng(9)
    eng = make()
    e = rng.standard_normal((50, D)).astype(np.float32)
    assert eng.index_insert(e) == 0                            # creates an implicit-id index (ids 0..49)
    m = Model(e, np.arange(50, dtype=np.int64), np.zeros(50, np.int32))
    check(eng, m, e[:4], 10)
    eng2 = make()
    eng2.index_reserve(5000, id_base=100)
    eng2.index_append(e)
    eng2.index_insert(e[:10] * 2)                            # fills the reservation, implicit ids 150..159
    ids, _, _ = eng2.dense_topk(e[:1] * 2, 2)
    assert ids[0, 0] in (100, 150)


def _postings(rng, n):
    from optimized_rag_amd.bm25 import Bm25Postings
    vocab = 400
    docs = []
    for L in rng.poisson(12, n):
        docs.append([int(x) % vocab for x in rng.zipf(1.1, int(L)) - 1])
    corpus = [" ".join(f"t{t}" for t in d) for d in docs]
    return docs, corpus, Bm25Postings.from_corpus(corpus)


@pytest.mark.parametrize("opt", [None, "bm25_packed", "bm25_no_staging", "bm25_sort_merge", "bm25_linear_grid"])
def test_bm25_and_hybrid_after_deletes(make, opt):
    import torch
    rng = np.random.default_rng(23)
    N, Q, k = 9000, 12, 50
    docs, corpus, post = _postings(rng, N)
    emb = rng.standard_normal((N, D)).astype(np.float32)
    ids = (np.arange(N)[::-1] + 70_000).astype(np.int64)
    ten = rng.integers(0, 3, N).astype(np.int32)
    eng = make()
    if opt:
        eng.set_option(opt, 1)
    eng.index_load(emb, ids=ids)
    eng.set_tenants(ten)
    post.load(eng)
    qs = [" ".join(f"t{t}" for t in rng.choice(docs[int(rng.integers(0, N))] or [1], size=4)) for _ in range(Q)]
    ptr, terms = post.encode_queries(qs)
    dead = rng.random(N) < 0.25
    # the best BM25 hits of the first queries are among the deleted rows
    obm = O.BM25Okapi([O.tokenize(c) for c in corpus])
    raws = [obm.get_scores(O.tokenize(q)) for q in qs]
    for r in raws[:4]:
        dead[O.stable_topk_desc(r, 5)] = True
    assert eng.index_delete(ids[dead]) == int(dead.sum())
    for tenant in (-1, 1):
        bid, brow, bsc, bmx = eng.bm25_topk(ptr, terms, k, tenant=tenant)
        for qi in range(Q):
            keep = ~dead & ((ten == tenant) if tenant >= 0 else True)
            raw = np.where(keep, raws[qi], -np.inf)
            mx = raw.max() if raw.max() > 0 else 1.0
            top = O.stable_topk_desc(raw, k)
            top = top[np.isfinite(raw[top])]
            np.testing.assert_array_equal(brow[qi, :len(top)], top.astype(np.int32))
            np.testing.assert_array_equal(bid[qi, :len(top)], ids[top])
            np.testing.assert_array_equal(bsc[qi, :len(top)], raws[qi][top] / mx)
            assert bmx[qi] == mx
    dense = eng.bm25_scores(ptr, terms)
    for qi in range(Q):
        np.testing.assert_array_equal(dense[qi], np.where(dead, 0.0, raws[qi]))
    # hybrid RRF: oracle dense top-pool over the live rows + oracle BM25 top-pool over the live documents + oracle RRF
    lv = np.nonzero(~dead)[0]
    qd = torch.from_numpy((emb[rng.integers(0, N, Q)] + 0.5 * rng.standard_normal((Q, D))).astype(np.float32)).cuda()
    pd, td = torch.from_numpy(ptr).cuda(), torch.from_numpy(terms).cuda()
    keys, rrf, ranks = eng.hybrid_rrf_dev(qd, pd, td, 40, 20, tenant=-1)
    torch.cuda.synchronize()
    d_rows, _ = O.dense_topk(emb[lv], qd.cpu().numpy(), 40)
    for qi in range(Q):
        raw = np.where(dead, -np.inf, raws[qi])
        b_rows = O.stable_topk_desc(raw, 40)
        b_rows = b_rows[np.isfinite(raw[b_rows])]
        okeys, oscores, oranks = O.rrf_fuse([[int(ids[lv[r]]) for r in d_rows[qi]], [int(ids[r]) for r in b_rows]], k=60, top_k=20)
        assert keys[qi].cpu().tolist()[:len(okeys)] == okeys
        assert rrf[qi].cpu().tolist()[:len(oscores)] == oscores
    hy = eng.hybrid_linear_dev(qd, pd, td, 20, 0.55, 0.35, 0.10)
    torch.cuda.synchronize()
    rows_l = hy["rows"].cpu().numpy()
    assert not np.isin(rows_l[rows_l >= 0], np.nonzero(dead)[0]).any()


def test_bm25_stale_after_insert_and_compaction(make):
    from optimized_rag_amd import RagError
    rng = np.random.default_rng(29)
    N = 3000
    docs, corpus, post = _postings(rng, N)
    eng = make()
    emb = rng.standard_normal((N, D)).astype(np.float32)
    eng.index_load(emb)
    post.load(eng)
    ptr, terms = post.encode_queries(["t1 t2 t3"])
    eng.bm25_topk(ptr, terms, 10)
    eng.index_delete([0, 1])                                 # deletes keep the postings valid
    eng.bm25_topk(ptr, terms, 10)
    eng.index_insert(rng.standard_normal((2, D)).astype(np.float32))
    with pytest.raises(RagError, match="stale"):
        eng.bm25_topk(ptr, terms, 10)
    eng.index_compact()                                      # N rows again: the count matches, the alignment does not
    with pytest.raises(RagError, match="stale"):
        eng.bm25_topk(ptr, terms, 10)
    corpus2 = corpus[2:] + ["t1 t2 t3 t3", "t9"]
    from optimized_rag_amd.bm25 import Bm25Postings
    post2 = Bm25Postings.from_corpus(corpus2).load(eng)
    ptr2, terms2 = post2.encode_queries(["t1 t2 t3"])
    _, rows, sc, _ = eng.bm25_topk(ptr2, terms2, 10)
    raw = O.BM25Okapi([O.tokenize(c) for c in corpus2]).get_scores(O.tokenize("t1 t2 t3"))
    np.testing.assert_array_equal(rows[0], O.stable_topk_desc(raw, 10).astype(np.int32))


def test_dev_search_queued_before_a_delete_returns_the_old_result(make):
    import torch
    rng = np.random.default_rng(31)
    N, Q, k = 200_000, 256, 100
    emb = rng.standard_normal((N, D)).astype(np.float32)
    eng = make()
    eng.index_load(emb)
    q = (emb[:Q] + 0.3 * rng.standard_normal((Q, D))).astype(np.float32)
    assert eng.index_delete([N - 1]) == 1                    # the deleted-row path (vis) is live when the search is queued
    ref_ids, _, _ = eng.dense_topk(q, k)
    s = torch.cuda.Stream()
    qd = torch.from_numpy(q).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        ids_out = torch.empty((Q, k), dtype=torch.int64, device="cuda")
        sc_out = torch.empty((Q, k), dtype=torch.float64, device="cuda")
        eng.dense_topk_dev(qd, k, ids_out, None, sc_out, stream=s)
    assert eng.index_delete(ref_ids[:, 0]) > 0               # host delete of every query's best hit
    s.synchronize()
    np.testing.assert_array_equal(ids_out.cpu().numpy(), ref_ids)
    new_ids, _, _ = eng.dense_topk(q, k)
    assert not np.isin(new_ids, ref_ids[:, 0]).any()


def live_postings(post, lv):
    """The loaded postings restricted to the live documents lv (renumbered), with the loaded idf and avgdl: what a fresh
    handle of the live rows must hold to score BM25 as the index with deletions does."""
    from optimized_rag_amd.bm25 import Bm25Postings
    remap = np.full(post.n_docs, -1, np.int64)
    remap[lv] = np.arange(len(lv))
    keep = remap[post.doc] >= 0
    term = np.repeat(np.arange(len(post.indptr) - 1), np.diff(post.indptr))
    counts = np.bincount(term[keep], minlength=len(post.indptr) - 1)
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(post.indptr.dtype)
    return Bm25Postings(indptr, remap[post.doc[keep]].astype(post.doc.dtype), post.tf[keep], post.doc_len[lv], post.idf, post.avgdl,
                        post.vocab, post.k1, post.b)


def test_hybrid_linear_after_writes_equals_fresh_handle(make):
    import torch
    rng = np.random.default_rng(41)
    N, Q, k = 6000, 16, 30
    docs, corpus, post = _postings(rng, N)
    emb = rng.standard_normal((N, D)).astype(np.float32)
    tmp = rng.random(N) * 0.1
    eng = make()
    eng.index_load(emb, ids=np.arange(N, dtype=np.int64) + 9)
    eng.set_temporal(tmp)
    eng.index_insert(rng.standard_normal((40, D)).astype(np.float32), ids=np.arange(40, dtype=np.int64) + 90_000,
                     temporal=np.full(40, 3.0))             # larger than every loaded score: temporal_absmax must grow
    emb = np.concatenate([emb, eng.fetch_rows(np.arange(N, N + 40))])
    tmp = np.concatenate([tmp, np.full(40, 3.0)])
    ids = np.concatenate([np.arange(N) + 9, np.arange(40) + 90_000]).astype(np.int64)
    corpus = corpus + [" ".join(f"t{t}" for t in rng.integers(0, 50, 8)) for _ in range(40)]
    from optimized_rag_amd.bm25 import Bm25Postings
    post = Bm25Postings.from_corpus(corpus)
    post.load(eng)                                           # postings of the current rows after the insert
    dead = rng.random(N + 40) < 0.2
    assert eng.index_delete(ids[dead]) == int(dead.sum())
    lv = np.nonzero(~dead)[0]
    f = make()
    f.index_load(emb[lv], ids=ids[lv])
    f.set_temporal(tmp[lv])
    live_postings(post, lv).load(f)
    qs = [" ".join(corpus[int(i)].split()[:3]) or "t1" for i in rng.integers(0, N + 40, Q)]
    ptr, terms = post.encode_queries(qs)
    qd = torch.from_numpy((emb[rng.integers(0, N + 40, Q)] + 0.5 * rng.standard_normal((Q, D))).astype(np.float32)).cuda()
    pd, td = torch.from_numpy(ptr).cuda(), torch.from_numpy(terms).cuda()
    for a_, b_, g_ in ((0.55, 0.35, 0.10), (0.3, 0.2, 0.5)):
        got = {n: v.cpu().numpy() for n, v in eng.hybrid_linear_dev(qd, pd, td, k, a_, b_, g_).items()}
        exp = {n: v.cpu().numpy() for n, v in f.hybrid_linear_dev(qd, pd, td, k, a_, b_, g_).items()}
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got["ids"], exp["ids"])
        for n in ("hybrid", "semantic", "keyword", "temporal"):
            np.testing.assert_array_equal(got[n].view(np.int64), exp[n].view(np.int64))


def test_token_store_inserts_deletes_compaction_and_rerank(make):
    """retrieve_rerank_dev modes 0 / 1 after deletes, mode 0 after inserts with tokens and after compaction (odd passage length:
    the u16 rows are moved two bytes at a time): candidates and logit bits equal to a fresh handle of the live rows."""
    import torch
    from oracle import bert_oracle as B
    from optimized_rag_amd.bm25 import Bm25Postings
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    rng = np.random.default_rng(43)
    N, Q, pool, k, Ld, Lq, L = 700, 4, 8, 4, 19, 10, 32
    cfg = dict(vocab_size=2000, hidden=384, layers=2, heads=12, ffn=1536, max_pos=64, type_vocab=2, eps=1e-12)
    wts = flatten_state_dict(B.seeded_weights(cfg, 5), cfg["layers"])
    emb = rng.standard_normal((N, D)).astype(np.float32)
    tok = rng.integers(200, 2000, (N, Ld)).astype(np.int32)
    tl = rng.integers(3, Ld + 1, N).astype(np.int32)
    ids = np.arange(N, dtype=np.int64) * 2 + 1
    corpus = [" ".join(f"t{t % 40}" for t in tok[i, :tl[i]]) for i in range(N)]
    eng = make()
    eng.index_load(emb, ids=ids)
    eng.tokens_load(tok, tl)
    eng.ce_load(cfg, wts)
    post = Bm25Postings.from_corpus(corpus)
    post.load(eng)
    q_emb = torch.from_numpy((emb[rng.integers(0, N, Q)] + 0.3 * rng.standard_normal((Q, D))).astype(np.float32)).cuda()
    q_tok = torch.from_numpy(rng.integers(200, 2000, (Q, Lq)).astype(np.int32)).cuda()
    q_len = torch.from_numpy(np.array([Lq, 3, 5, 7], np.int32)).cuda()
    ptr, terms = post.encode_queries([" ".join(corpus[int(i)].split()[:4]) for i in rng.integers(0, N, Q)])
    hy = dict(term_ptr=torch.from_numpy(ptr).cuda(), terms=torch.from_numpy(terms).cuda())

    def run(e, **kw):
        out = [x.cpu().numpy().copy() for x in e.retrieve_rerank_dev(q_emb, q_tok, q_len, pool, k, L_pair=L, **kw)]
        torch.cuda.synchronize()
        return out

    def same(a, b):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8))

    def fresh(m_emb, m_ids, m_tok, m_tl, postings=None):
        f = make()
        f.index_load(m_emb, ids=m_ids)
        f.tokens_load(m_tok, m_tl)
        f.ce_load(cfg, wts)
        if postings is not None:
            postings.load(f)
        return f

    base = run(eng)
    dead = np.zeros(N, bool)
    dead[np.unique(np.searchsorted(ids, base[3][:, :3].ravel()))] = True             # the best candidates go
    dead |= rng.random(N) < 0.1
    assert eng.index_delete(ids[dead]) == int(dead.sum())
    lv = np.nonzero(~dead)[0]
    f = fresh(emb[lv], ids[lv], tok[lv], tl[lv], live_postings(post, lv))
    same(run(eng), run(f))
    same(run(eng, **hy), run(f, **hy))
    # inserts with tokens (some rows the best match of a query), then mode 0
    n_new = 30
    e_new = np.concatenate([q_emb.cpu().numpy()[:2], rng.standard_normal((n_new - 2, D)).astype(np.float32)])
    t_new = rng.integers(200, 2000, (n_new, Ld)).astype(np.int32)
    l_new = rng.integers(1, Ld + 1, n_new).astype(np.int32)
    i_new = np.arange(n_new, dtype=np.int64) * 2 + 100_000
    with pytest.raises(Exception):
        eng.index_insert(e_new, ids=i_new, tokens=t_new[:, :Ld - 1], token_lens=l_new)          # wrong passage length
    eng.index_insert(e_new, ids=i_new, tokens=t_new, token_lens=l_new)
    a_emb, a_ids = np.concatenate([emb, e_new]), np.concatenate([ids, i_new])
    a_tok, a_tl = np.concatenate([tok, t_new]), np.concatenate([tl, l_new])
    live = np.concatenate([~dead, np.ones(n_new, bool)])
    lv = np.nonzero(live)[0]
    f = fresh(a_emb[lv], a_ids[lv], a_tok[lv], a_tl[lv])
    same(run(eng), run(f))
    # compaction moves every plane, the token store included
    row_map = eng.index_compact()
    np.testing.assert_array_equal(row_map[lv], np.arange(len(lv)))
    same(run(eng), run(f))
