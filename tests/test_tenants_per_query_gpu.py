"""GPU: search batches with a tenant PER QUERY (rag_*_tenants_*; RagEngine methods with `tenant=` an array).

Every result is held against BOTH
  * the scalar-tenant entry, called once per distinct tenant over that tenant's queries: np.array_equal, floats by their bits;
  * the oracle, per query: O.dense_topk under the tenant, the CSR BM25 oracle masked to the tenant, O.rrf_fuse, the linear
    fusion in the reference's operation order, the float64 BERT - ids exact, cosines within 1e-9, BM25 and RRF bit-exact,
    logits within 4e-3 (the bars of test_dense_gpu.py, test_hybrid_gpu.py, test_pipeline_gpu.py).
Tenant layouts (TENANT numbers of the queries in brackets): two interleaved tenants [0, 1], two stored contiguously with
ranges that start and end inside tiles [2, 3], one of 3 rows - fewer than k - [4], a number that owns no row [5], and
unfiltered queries [-1]. Shapes are the smallest that reach each path."""
import numpy as np
import pytest

import stream_tools as T
from oracle import bert_oracle as B
from oracle import rag_oracle as O
from test_pipeline_gpu import CLS, SEP, build_pairs

pytestmark = pytest.mark.gpu

D = 64
QUERY_TENANTS = np.array([0, 2, -1, 1, 4, 3, 5], dtype=np.int32)
DEAD = -99                                  # marks a deleted row in the oracle's tenant column


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else (a.view(np.int32) if a.dtype == np.float32 else a)


def assert_same(got, ref, what=""):
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape and g.dtype == r.dtype, (what, i)
        assert np.array_equal(bits(g), bits(r)), f"{what}: output {i} differs from the scalar-tenant entry"


def by_tenant(call, tenants):
    """call(sel, tenant) -> tuple of arrays for the queries `sel` under one scalar tenant; assembled into whole-batch arrays."""
    whole = None
    for t in np.unique(tenants):
        sel = np.nonzero(tenants == t)[0]
        part = call(sel, int(t))
        if whole is None:
            whole = [np.empty((len(tenants),) + p.shape[1:], dtype=p.dtype) for p in part]
        for w, p in zip(whole, part):
            w[sel] = p
    return whole


def layout(N):
    """tenant of every row: see the module docstring"""
    a, b = (700, 1500) if N < 3000 else (1400, 3000)
    ten = np.empty(N, dtype=np.int32)
    ten[:a] = np.arange(a) % 2
    ten[a:b] = 2
    ten[b:] = 3
    ten[[5, a + 10, N - 1]] = 4
    return ten


def query_tenants(Q, rng=None):
    t = np.resize(QUERY_TENANTS, Q).copy()
    if rng is not None:
        rng.shuffle(t)
    return t


def planted(rng, corpus, Q, noise=0.4):
    return (corpus[rng.integers(0, corpus.shape[0], Q)] + noise * rng.standard_normal((Q, corpus.shape[1]))).astype(np.float32)


def oracle_dense(corpus, queries, k, ten_rows, tenants):
    """rows [Q, k] (-1 padded) and cosines of every query under ITS tenant (ten_rows: DEAD for deleted rows)"""
    rows = np.full((len(queries), k), -1, dtype=np.int64)
    sc = np.zeros((len(queries), k))
    for t in np.unique(tenants):
        sel = np.nonzero(tenants == t)[0]
        col, want = (ten_rows, int(t)) if t >= 0 else ((ten_rows != DEAD).astype(np.int32), 1)
        if (col == want).any():
            rows[sel], sc[sel] = O.dense_topk(corpus, queries[sel], k, col, want)
    return rows, sc


def check_dense(eng, corpus, queries, k, ten_rows, tenants, ids=None, oracle=None):
    assert hasattr(eng.lib, "rag_dense_topk_tenants_host")          # (a one-query array must not pass for a scalar by conversion)
    got = eng.dense_topk(queries, k, tenant=tenants)
    stats = eng.dense_stats()                                    # of the per-query call
    ref = by_tenant(lambda sel, t: eng.dense_topk(queries[sel], k, tenant=t), tenants)
    assert_same(got, ref, "dense")
    orow, osc = oracle if oracle is not None else oracle_dense(corpus, queries, k, ten_rows, tenants)
    orow, osc = orow[:, :k], osc[:, :k]
    np.testing.assert_array_equal(got[1], orow.astype(np.int32))
    np.testing.assert_array_equal(got[0], orow if ids is None else np.where(orow >= 0, ids[np.maximum(orow, 0)], -1))
    np.testing.assert_allclose(got[2], osc, rtol=0, atol=1e-9)
    return got, stats


@pytest.fixture(scope="module")
def engines():
    from optimized_rag_amd import RagEngine
    made = []

    def make(dim=D):
        e = RagEngine(dim=dim, device=0)
        made.append(e)
        return e

    yield make
    for e in made:
        e.close()


_DENSE = {}


def dense_world(engines, N):
    """one corpus, one engine and ONE oracle result (300 queries, k = 20) per N: smaller batches and k are its prefixes"""
    if N not in _DENSE:
        rng = np.random.default_rng(N)
        corpus = rng.standard_normal((N, D)).astype(np.float32)
        ten = layout(N)
        queries = planted(rng, corpus, 300)
        tq = query_tenants(300, rng)
        tq[:7] = QUERY_TENANTS                                   # every kind of tenant inside the smallest mixed batch
        eng = engines()
        eng.index_load(corpus)
        eng.set_tenants(ten)
        _DENSE[N] = dict(corpus=corpus, ten=ten, q=queries, tq=tq, eng=eng, oracle=oracle_dense(corpus, queries, 20, ten, tq))
    return _DENSE[N]


# ------------------------------------------------------------------------------------------------------------ 1. dense
@pytest.mark.parametrize("k", [5, 20])
@pytest.mark.parametrize("Q", [1, 64, 65, 130, 300])
@pytest.mark.parametrize("N", [2309, 4613])
def test_dense_mixed_tenants(engines, N, Q, k):
    w = dense_world(engines, N)
    orow, osc = w["oracle"]
    got, st = check_dense(w["eng"], w["corpus"], w["q"][:Q], k, w["ten"], w["tq"][:Q], oracle=(orow[:Q], osc[:Q]))
    assert st["proven_fast"] + st["proven_wide"] + st["exact_scan"] == Q and st["exact_scan"] == 0, st
    for qi in np.nonzero(w["tq"][:Q] == 4)[0]:                   # 3 rows: padded
        assert (got[1][qi, 3:] == -1).all() and (got[1][qi, :3] >= 0).all() and (got[2][qi, 3:] == 0).all()
    for qi in np.nonzero(w["tq"][:Q] == 5)[0]:                   # owns no row: all padding
        assert (got[0][qi] == -1).all() and (got[1][qi] == -1).all() and (got[2][qi] == 0).all()


@pytest.mark.parametrize("n_union", [8, 9, 10])
def test_dense_union_of_tile_lists_at_the_stage0_boundary(engines, n_union):
    """Every query filtered, two contiguous tenants whose tile lists (4 + 4, 5 + 4, 5 + 5 tiles, none shared, ranges starting and
    ending inside tiles) are together shorter than the table's 19 tiles: the union is searched - ONE dense stage of 8 or of 9
    tiles (the select-after-stage-0 boundary test_dense_gpu.py pins for a single tenant), two stages at 10."""
    w = dense_world(engines, 4613)
    eng, corpus, N = w["eng"], w["corpus"], 4613
    na, nb = {8: (4, 4), 9: (5, 4), 10: (5, 5)}[n_union]
    ten = np.full(N, 9, dtype=np.int32)
    a0, a1 = 256 * 2 + 17, 256 * (2 + na) - 40
    b0, b1 = 256 * 8 + 5, 256 * (8 + nb) - 7
    ten[a0:a1], ten[b0:b1] = 0, 1
    rng = np.random.default_rng(n_union)
    queries = np.concatenate([planted(rng, corpus[a0:a1], 6, 0.2), planted(rng, corpus[b0:b1], 6, 0.2)])
    tq = np.array([0] * 6 + [1] * 6, dtype=np.int32)
    perm = rng.permutation(12)
    queries, tq = queries[perm], tq[perm]
    eng.set_tenants(ten)
    try:
        check_dense(eng, corpus, queries, 5, ten, tq)
        _, st = check_dense(eng, corpus, queries, 5, ten, tq)    # ... (the scalar calls in between chose other universes)
        assert st["stages"] == (2 if n_union == 10 else 1) and st["exact_scan"] == 0, st
    finally:
        eng.set_tenants(w["ten"])


# -------------------------------------------------------------------------------------------------- 2. dense fallbacks
@pytest.mark.parametrize("option,value,ran", [
    ("force_level", 1, "proven_wide"),             # the wide ranking of every query
    ("force_level", 2, "exact_scan"),              # the float64 scan: a LIST of flagged queries, in rounds
    ("stage_growth", 100000, "second_pass"),       # forced overflow: re-emission through ws_ovf, dead slots mapped to query 0
    ("stage_growth+no_second_pass", 100000, "exact_scan"),
])
def test_dense_fallback_paths_follow_the_query_indirections(engines, option, value, ran):
    """Q = 300 mixed tenants (two query tiles) through every path that reaches a query by an indirection. The forced overflow is
    test_second_pass_replaces_the_exact_scan's: one threshold stage over the whole table with a threshold drawn from 2048 rows.
    The small corpus cannot overflow a 4096-entry buffer, so those two cases run on the smallest one that does: the stage emits about
    rows x k / 2048 keys per query, 5,900 at 60k rows and k = 200 - for the unfiltered and the interleaved queries; the contiguous
    tenant of 4,000 rows cannot overflow, so the second pass runs with dead slots."""
    if option.startswith("stage_growth"):
        N, k = 60_000, 200
        if N not in _DENSE:
            rng = np.random.default_rng(N)
            corpus = rng.standard_normal((N, D)).astype(np.float32)
            ten = (np.arange(N) % 3).astype(np.int32)
            ten[20_000:24_000] = 3
            tq = np.resize(np.array([0, 1, -1, 2, 3, -1], dtype=np.int32), 300)
            queries = planted(rng, corpus, 300)
            eng = engines()
            eng.index_load(corpus)
            eng.set_tenants(ten)
            _DENSE[N] = dict(corpus=corpus, ten=ten, q=queries, tq=tq, eng=eng, oracle=oracle_dense(corpus, queries, k, ten, tq))
        w = _DENSE[N]
    else:
        w, k = dense_world(engines, 4613), 20
    eng = w["eng"]
    names = option.split("+")
    eng.set_option(names[0], value)
    for n in names[1:]:
        eng.set_option(n, 1)
    try:
        got = eng.dense_topk(w["q"], k, tenant=w["tq"])
        st = eng.dense_stats()
    finally:
        for n in names:
            eng.set_option(n, 0)
    assert st[ran] > 0, (option, st)                                   # the path under test really ran
    ref = by_tenant(lambda sel, t: eng.dense_topk(w["q"][sel], k, tenant=t), w["tq"])
    assert_same(got, ref, option)
    np.testing.assert_array_equal(got[1], w["oracle"][0][:, :k].astype(np.int32))
    np.testing.assert_allclose(got[2], w["oracle"][1][:, :k], rtol=0, atol=1e-9)


# -------------------------------------------------------------------------------------------------------- 3. live index
def test_live_index_delete_insert_compact(engines):
    rng = np.random.default_rng(31)
    N = 2309
    corpus = rng.standard_normal((N, D)).astype(np.float32)
    ten = layout(N)
    ids = np.arange(N, dtype=np.int64) + 10_000
    eng = engines()
    eng.index_load(corpus, ids=ids)
    eng.set_tenants(ten)
    mine = np.nonzero(ten == 2)[0]
    gone = mine[::3]                                                    # a third of tenant 2's rows
    assert eng.index_delete(ids[gone]) == len(gone)
    new = rng.standard_normal((300, D)).astype(np.float32)
    new_ids = np.arange(300, dtype=np.int64) + 90_000
    eng.index_insert(new, ids=new_ids, tenants=np.full(300, 7, dtype=np.int32))    # a tenant the table did not know
    corpus = np.concatenate([corpus, new])
    ids = np.concatenate([ids, new_ids])
    ten = np.concatenate([ten, np.full(300, 7, dtype=np.int32)])
    ten_live = ten.copy()
    ten_live[gone] = DEAD
    Q, k = 70, 20
    queries = np.concatenate([planted(rng, corpus[mine], 20), planted(rng, corpus, 30), planted(rng, new, 20)])
    tq = np.concatenate([np.full(20, 2), query_tenants(30, rng), np.resize([7, -1], 20)]).astype(np.int32)
    before, _ = check_dense(eng, corpus, queries, k, ten_live, tq, ids=ids)
    assert not np.isin(before[0], ids[gone]).any()
    row_map = eng.index_compact()
    keep = row_map >= 0
    assert keep.sum() == len(corpus) - len(gone)
    after, _ = check_dense(eng, corpus[keep], queries, k, ten[keep], tq, ids=ids[keep])
    np.testing.assert_array_equal(after[0], before[0])                  # the same documents, by id, with the same score bits
    np.testing.assert_array_equal(bits(after[2]), bits(before[2]))


def test_negative_scalar_tenants_stay_unfiltered_after_a_per_query_call(engines):
    """Every scalar tenant < 0 means "no filter" (include/rag_hip.h), -2 included - the value the per-query mark of the emit
    kernels has inside the library. On an index with deleted rows (the visibility table is consulted even without a filter),
    after a per-query batch left its column tenants behind the thresholds: the scalar entries with tenant = -2 and -7 return
    what tenant = -1 returns, bit for bit, and the oracle's result over the live rows - host and device entry, small and full batch."""
    import torch
    rng = np.random.default_rng(41)
    N, k = 4613, 20
    corpus = rng.standard_normal((N, D)).astype(np.float32)
    ten = layout(N)
    eng = engines()
    eng.index_load(corpus)
    eng.set_tenants(ten)
    gone = np.arange(0, N, 5)
    assert eng.index_delete(gone) == len(gone)
    ten_live = ten.copy()
    ten_live[gone] = DEAD
    for Q in (40, 300):
        queries = planted(rng, corpus, Q)
        tq = np.resize(np.array([0, 1, 2, 3], dtype=np.int32), Q)            # every column tenant >= 0: a stale word would filter
        check_dense(eng, corpus, queries, k, ten_live, tq)
        eng.dense_topk(queries, k, tenant=tq)                                # the per-query call is the LAST one before the scalar ones
        unfiltered = np.full(Q, -1, dtype=np.int32)
        orow, osc = oracle_dense(corpus, queries, k, ten_live, unfiltered)
        ref = eng.dense_topk(queries, k, tenant=-1)
        for t in (-2, -7):
            eng.dense_topk(queries, k, tenant=tq)
            got = eng.dense_topk(queries, k, tenant=t)
            assert_same(got, ref, f"tenant={t}")
            np.testing.assert_array_equal(got[1], orow.astype(np.int32))
            np.testing.assert_allclose(got[2], osc, rtol=0, atol=1e-9)
            eng.dense_topk(queries, k, tenant=tq)
            qd = torch.from_numpy(queries).cuda()
            o = (torch.empty((Q, k), dtype=torch.int64, device="cuda"), torch.empty((Q, k), dtype=torch.int32, device="cuda"),
                 torch.empty((Q, k), dtype=torch.float64, device="cuda"))
            eng.dense_topk_dev(qd, k, *o, tenant=t)
            torch.cuda.synchronize()
            assert_same([x.cpu().numpy() for x in o], ref, f"dev, tenant={t}")


# -------------------------------------------------------------------------------------------------------------- 4. BM25
NB = 2 * 2048 + 5


class Bm25World:
    """N = 2 x 2048 + 5 documents over a small Zipf vocabulary, dim-64 embeddings, the tenant layouts; 130 queries."""

    def __init__(self, engines, opts=(), tail=0, seed=77):
        from optimized_rag_amd.bm25 import Bm25Postings
        rng = np.random.default_rng(seed)
        self.N, self.id_base = NB, 1000
        lens = rng.poisson(8, NB)
        toks = (rng.zipf(1.2, int(lens.sum())) - 1) % 300
        ptr = np.concatenate([[0], np.cumsum(lens)])
        self.texts = [" ".join(f"t{t}" for t in toks[ptr[i]:ptr[i + 1]]) for i in range(NB)]
        self.emb = rng.standard_normal((NB, D)).astype(np.float32)
        self.ten = layout(NB)
        n0 = NB - tail
        self.eng = engines()
        for name, v in opts:
            self.eng.set_option(name, v)
        self.eng.index_load(self.emb[:n0], id_base=self.id_base)
        self.eng.set_tenants(self.ten[:n0])
        self.post = Bm25Postings.from_corpus(self.texts[:n0]).load(self.eng)
        if tail:                                                        # the last rows arrive as an insert + an appended segment
            self.eng.index_insert(self.emb[n0:], tenants=self.ten[n0:])
            self.post.append_to(self.eng, self.post.extend(self.texts[n0:]))
        self.queries = [" ".join(f"t{t}" for t in (rng.zipf(1.2, int(rng.integers(1, 7))) - 1) % 300) for _ in range(130)]
        self.queries[9] = "nosuchtoken"
        self.ptr, self.terms = self.post.encode_queries(self.queries)
        self.q = planted(rng, self.emb, 130)
        self.tq = query_tenants(130, rng)
        self.tq[:3] = [0, 2, -1]
        p = self.post
        self.raw = [O.bm25_scores_csr(p.indptr, p.doc, p.tf, p.doc_len, p.idf, p.avgdl, self.terms[self.ptr[i]:self.ptr[i + 1]])
                    for i in range(130)]

    def sub(self, sel):
        """(term_ptr, terms) of the queries sel"""
        parts = [self.terms[self.ptr[i]:self.ptr[i + 1]] for i in sel]
        ptr = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)
        return ptr, (np.concatenate(parts) if parts else np.zeros(0)).astype(np.int32)

    def oracle_bm25(self, qi, k):
        """rows (padded), normalised scores, divisor of query qi under its tenant - None for a tenant without rows"""
        t = int(self.tq[qi])
        mine = np.nonzero(self.ten == t)[0] if t >= 0 else np.arange(self.N)
        if len(mine) == 0:
            return None
        raw = self.raw[qi][mine]
        m = raw.max() if raw.max() > 0 else 1.0
        top = O.stable_topk_desc(raw, k)
        rows = np.full(k, -1, dtype=np.int32)
        sc = np.zeros(k)
        rows[:len(top)], sc[:len(top)] = mine[top], raw[top] / m
        return rows, sc, m


_BM = {}


def bm_world(engines, key, **kw):
    if key not in _BM:
        _BM[key] = Bm25World(engines, **kw)
    return _BM[key]


def check_bm25(w, Q, k, dev):
    import torch
    eng = w.eng
    ptr, terms = w.sub(range(Q))
    tq = w.tq[:Q]

    def run(ptr_, terms_, tenant):
        n = len(ptr_) - 1
        if not dev:
            return eng.bm25_topk(ptr_, terms_, k, tenant=tenant)
        o = (torch.empty((n, k), dtype=torch.int64, device="cuda"), torch.empty((n, k), dtype=torch.int32, device="cuda"),
             torch.empty((n, k), dtype=torch.float64, device="cuda"), torch.empty((n,), dtype=torch.float64, device="cuda"))
        eng.bm25_topk_dev(torch.from_numpy(ptr_).cuda(), torch.from_numpy(terms_).cuda(), k, o[0], o[1], o[2], raw_max_out=o[3], tenant=tenant)
        torch.cuda.synchronize()
        return tuple(x.cpu().numpy() for x in o)

    got = run(ptr, terms, tq)
    ref = by_tenant(lambda sel, t: run(*w.sub(sel), t), tq)
    assert_same(got, ref, "bm25")                                       # ids, rows, scores and raw_max_out
    for qi in range(Q):
        o = w.oracle_bm25(qi, k)
        if o is None:
            assert (got[1][qi] == -1).all() and (got[2][qi] == 0).all()
            continue
        np.testing.assert_array_equal(got[1][qi], o[0])
        np.testing.assert_array_equal(bits(got[2][qi]), bits(o[1]))     # bit-exact
        assert got[3][qi] == o[2]
        np.testing.assert_array_equal(got[0][qi], np.where(o[0] >= 0, o[0].astype(np.int64) + w.id_base, -1))
    return got


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("Q", [3, 130])                                  # the XCD-aware plan starts at 128 queries
@pytest.mark.parametrize("packed", [0, 1])
def test_bm25_mixed_tenants(engines, packed, Q, dev):
    w = bm_world(engines, ("packed", packed), opts=(("bm25_packed", packed),))
    check_bm25(w, Q, 10, dev)


def test_bm25_behind_an_appended_tail_segment(engines):
    w = bm_world(engines, "tail", opts=(("bm25_tail_fold", -1),), tail=300)
    s = w.eng.bm25_segment_stats()
    assert s["tail_docs"] == 300 and s["folds"] == 0 and s["base_docs"] == NB - 300
    check_bm25(w, 130, 10, True)
    check_bm25(w, 3, 10, False)


def test_bm25_sub_batches_carry_their_tenants(engines):
    """bm25_ws_mb = 1 and k = 1000: a query's partial lists take 3 ranges x (12 k + 36) + 12 k bytes, so 1 MiB holds 21 queries
    and the 130 run in 7 sub-batches (bm25_topk_dev's rule, from the handle's segment facts); bm25_plan_slots = 8 besides."""
    w = bm_world(engines, ("packed", 0), opts=(("bm25_packed", 0),))
    k = 1000
    s = w.eng.bm25_segment_stats()
    ranges = -(-s["base_docs"] // 2048) + -(-s["tail_docs"] // 2048)
    per_query = ranges * (k * 12 + 4 + 8 * 4) + k * 12
    assert ranges == 3 and (1 << 20) // per_query < 130 / 6                # several sub-batches
    plain = check_bm25(w, 130, k, True)
    for opt, val in (("bm25_ws_mb", 1), ("bm25_plan_slots", 8)):
        w.eng.set_option(opt, val)
    try:
        got = check_bm25(w, 130, k, True)
    finally:
        for opt in ("bm25_ws_mb", "bm25_plan_slots"):
            w.eng.set_option(opt, 0)
    assert_same(got, plain, "sub-batched")


# -------------------------------------------------------------------------------------------------------- 5. hybrid RRF
@pytest.mark.parametrize("Q", [5, 130])                                  # 5: the BM25 leg on the side stream
def test_hybrid_rrf_mixed_tenants(engines, Q):
    import torch
    w = bm_world(engines, ("packed", 0), opts=(("bm25_packed", 0),))
    eng, pool, k = w.eng, 20, 10
    tq = w.tq[:Q].copy()
    if Q == 5:
        tq[:] = [0, 2, -1, 4, 5]

    def run(sel, tenant):
        ptr, terms = w.sub(sel)
        out = eng.hybrid_rrf_dev(torch.from_numpy(w.q[sel]).cuda(), torch.from_numpy(ptr).cuda(), torch.from_numpy(terms).cuda(), pool, k,
                                 tenant=tenant)
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy().copy() for t in out)

    got = run(np.arange(Q), tq)
    ref = by_tenant(run, tq)
    assert_same(got, ref, "hybrid_rrf")
    drows, _ = oracle_dense(w.emb, w.q[:Q], pool, w.ten, tq)
    for qi in range(Q):
        t = int(tq[qi])
        mine = np.nonzero(w.ten == t)[0] if t >= 0 else np.arange(w.N)
        brows = mine[O.stable_topk_desc(w.raw[qi][mine], pool)] if len(mine) else []
        okeys, oscores, oranks = O.rrf_fuse([[int(r) + w.id_base for r in drows[qi] if r >= 0], [int(r) + w.id_base for r in brows]],
                                            k=60, top_k=k)
        n = len(okeys)
        assert got[0][qi, :n].tolist() == okeys and (got[0][qi, n:] == -1).all()
        assert got[1][qi, :n].tolist() == oscores and got[2][qi, :n].tolist() == oranks
        if t >= 0:
            assert all(w.ten[key - w.id_base] == t for key in okeys)


# ------------------------------------------------------------------------------------------ 6. index-level linear fusion
def test_hybrid_linear_uses_each_querys_own_tenant_maximum(engines):
    import torch
    from test_hybrid_gpu import _sparse_postings
    rng = np.random.default_rng(78)
    N, k = 4096, 25
    emb = rng.standard_normal((N, D)).astype(np.float32)
    ten = layout(N)
    temporal = np.where(rng.uniform(size=N) < 0.4, 0.15 * 0.5 ** (rng.uniform(0, 90, N) / 30.0), 0.0)
    post = _sparse_postings(rng, N, 12, 600)
    eng = engines()
    eng.index_load(emb)
    eng.set_tenants(ten)
    eng.set_temporal(temporal)
    post.load(eng)
    terms_of = [[0, 1], [2, 3, 4], [5], [11, 0, 7], [6, 1], [8], [9, 10, 2]]
    tq = QUERY_TENANTS.copy()                                            # Q = 7: every kind of tenant
    ptr = np.cumsum([0] + [len(t) for t in terms_of]).astype(np.int32)
    terms = np.asarray([x for t in terms_of for x in t], dtype=np.int32)
    q = planted(rng, emb, 7)
    a, b, g = O.weights_for_intent("search")

    def run(sel, tenant):
        p = np.cumsum([0] + [len(terms_of[i]) for i in sel]).astype(np.int32)
        tm = np.asarray([x for i in sel for x in terms_of[i]], dtype=np.int32)
        out = eng.hybrid_linear_dev(torch.from_numpy(q[sel]).cuda(), torch.from_numpy(p).cuda(), torch.from_numpy(tm).cuda(), k, a, b, g,
                                    tenant=tenant)
        torch.cuda.synchronize()
        return tuple(out[key].cpu().numpy().copy() for key in ("ids", "rows", "hybrid", "semantic", "keyword", "temporal"))

    got = run(np.arange(7), tq)
    assert_same(got, by_tenant(run, tq), "hybrid_linear")
    differs = 0
    for qi, t in enumerate(terms_of):
        tenant = int(tq[qi])
        mine = np.nonzero(ten == tenant)[0] if tenant >= 0 else np.arange(N)
        if len(mine) == 0:
            assert (got[1][qi] == -1).all()
            continue
        raw = O.bm25_scores_csr(post.indptr, post.doc, post.tf, post.doc_len, post.idf, post.avgdl, t)
        m = raw[mine].max() if raw[mine].max() > 0 else 1.0
        differs += m != (raw.max() if raw.max() > 0 else 1.0)
        kw = raw[mine] / m                                               # the query's OWN tenant's maximum
        hyb = (a * O.cosine_matrix(q[qi:qi + 1], emb[mine])[0] + b * kw) + g * temporal[mine]
        order = O.stable_topk_desc(hyb, k)
        n = len(order)
        assert got[1][qi, :n].tolist() == mine[order].tolist() and (got[1][qi, n:] == -1).all()
        assert got[4][qi, :n].tolist() == kw[order].tolist()
        np.testing.assert_allclose(got[2][qi, :n], hyb[order], atol=1e-12)
    assert differs > 0                                                   # some tenant's maximum was not the corpus maximum


def test_hybrid_linear_second_pass_with_mixed_tenants(engines):
    """The fused re-emission under per-query tenants (it runs through the one-workgroup-per-tile kernel there, and reads each
    column's bias row through the query map and its tenant from the gathered plane): the forced overflow of the dense fallback
    test, 60k rows and k = 200, on the linear fusion. The contiguous tenant cannot overflow: dead slots."""
    import torch
    from test_hybrid_gpu import _sparse_postings
    rng = np.random.default_rng(79)
    N, k, Q = 60_000, 200, 12
    emb = rng.standard_normal((N, D)).astype(np.float32)
    ten = (np.arange(N) % 3).astype(np.int32)
    ten[20_000:24_000] = 3
    temporal = np.where(rng.uniform(size=N) < 0.3, 0.15 * 0.5 ** (rng.uniform(0, 90, N) / 30.0), 0.0)
    post = _sparse_postings(rng, N, 12, 2000)
    eng = engines()
    eng.index_load(emb)
    eng.set_tenants(ten)
    eng.set_temporal(temporal)
    post.load(eng)
    tq = np.resize(np.array([0, 3, -1, 1, 2, -1], dtype=np.int32), Q)
    terms_of = [[int(x) for x in rng.integers(0, 12, int(rng.integers(1, 4)))] for _ in range(Q)]
    q = planted(rng, emb, Q)
    a, b, g = 0.55, 0.35, 0.10
    seen = []

    def run(sel, tenant):
        p = np.cumsum([0] + [len(terms_of[i]) for i in sel]).astype(np.int32)
        tm = np.asarray([x for i in sel for x in terms_of[i]], dtype=np.int32)
        out = eng.hybrid_linear_dev(torch.from_numpy(q[sel]).cuda(), torch.from_numpy(p).cuda(), torch.from_numpy(tm).cuda(), k, a, b, g,
                                    tenant=tenant)
        torch.cuda.synchronize()
        seen.append(eng.dense_stats())
        return tuple(out[key].cpu().numpy().copy() for key in ("ids", "rows", "hybrid", "semantic", "keyword", "temporal"))

    eng.set_option("stage_growth", 100000)
    try:
        got = run(np.arange(Q), tq)
        st = seen[0]
        assert st["overflowed"] > 0 and st["second_pass"] > 0 and st["exact_scan"] == 0, st
        assert_same(got, by_tenant(run, tq), "hybrid_linear, second pass")
    finally:
        eng.set_option("stage_growth", 0)
    for qi in (0, 1, 2):                                                 # interleaved, contiguous, unfiltered
        mine = np.nonzero(ten == tq[qi])[0] if tq[qi] >= 0 else np.arange(N)
        raw = O.bm25_scores_csr(post.indptr, post.doc, post.tf, post.doc_len, post.idf, post.avgdl, terms_of[qi])
        kw = raw[mine] / (raw[mine].max() if raw[mine].max() > 0 else 1.0)
        hyb = (a * O.cosine_matrix(q[qi:qi + 1], emb[mine])[0] + b * kw) + g * temporal[mine]
        order = O.stable_topk_desc(hyb, k)
        assert got[1][qi].tolist() == mine[order].tolist()
        np.testing.assert_allclose(got[2][qi], hyb[order], atol=1e-12)


# -------------------------------------------------------------------------------------------------------------- 7. pipeline
@pytest.mark.parametrize("mode", [0, 1])
def test_retrieve_rerank_mixed_tenants(mode):
    import torch
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.bm25 import Bm25Postings
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    rng = np.random.default_rng(200 + mode)
    N, Dm, Q, pool, k, Ld, Lq, L = 300, 1536, 4, 8, 3, 20, 14, 24
    cfg = dict(vocab_size=2000, hidden=384, layers=2, heads=12, ffn=1536, max_pos=64, type_vocab=2, eps=1e-12)
    wts = B.seeded_weights(cfg, 17)
    emb = rng.standard_normal((N, Dm)).astype(np.float32)
    ten = (np.arange(N) % 2).astype(np.int32)
    ten[100:180] = 2
    ten[[3, 150, 299]] = 4
    tq = np.array([1, 2, -1, 4], dtype=np.int32)
    q_emb = planted(rng, emb, Q)
    tok = rng.integers(200, cfg["vocab_size"], (N, Ld)).astype(np.int32)
    tok_len = rng.integers(3, Ld + 1, N).astype(np.int32)
    q_tok = rng.integers(200, cfg["vocab_size"], (Q, Lq)).astype(np.int32)
    q_len = np.array([Lq, 3, 5, 9], dtype=np.int32)
    corpus = [" ".join(f"t{t}" for t in tok[i, :tok_len[i]] % 40) for i in range(N)]
    queries = [" ".join(f"t{t}" for t in q_tok[i, :q_len[i]] % 40) for i in range(Q)]
    eng = RagEngine(dim=Dm, device=0)
    try:
        eng.index_load(emb, id_base=1000)
        eng.set_tenants(ten)
        eng.tokens_load(tok, tok_len)
        eng.ce_load(cfg, flatten_state_dict(wts, cfg["layers"]))
        post = Bm25Postings.from_corpus(corpus).load(eng)
        ptr, terms = post.encode_queries(queries)

        def run(sel, tenant):
            parts = [terms[ptr[i]:ptr[i + 1]] for i in sel]
            p = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int32)
            args = dict(term_ptr=torch.from_numpy(p).cuda(), terms=torch.from_numpy(np.concatenate(parts).astype(np.int32)).cuda()) if mode else {}
            out = eng.retrieve_rerank_dev(torch.from_numpy(q_emb[sel]).cuda(), torch.from_numpy(q_tok[sel]).cuda(),
                                          torch.from_numpy(q_len[sel]).cuda(), pool, k, L_pair=L, cls_id=CLS, sep_id=SEP, tenant=tenant, **args)
            torch.cuda.synchronize()
            return tuple(t.cpu().numpy().copy() for t in out)

        ids, sc, lg, cand = got = run(np.arange(Q), tq)
        assert_same(got, by_tenant(run, tq), "retrieve_rerank")          # ids, scores, logits and cand_out, bit for bit
    finally:
        eng.close()
    d_rows, _ = oracle_dense(emb, q_emb, pool, ten, tq)
    ocand = np.full((Q, pool), -1, dtype=np.int64)
    obm = O.BM25Okapi([O.tokenize(c) for c in corpus])
    for qi in range(Q):
        if mode == 0:
            ocand[qi] = d_rows[qi]
            continue
        mine = np.nonzero(ten == tq[qi])[0] if tq[qi] >= 0 else np.arange(N)
        b_rows = mine[O.stable_topk_desc(obm.get_scores(O.tokenize(queries[qi]))[mine], pool)]
        keys, _, _ = O.rrf_fuse([[int(r) for r in d_rows[qi] if r >= 0], [int(r) for r in b_rows]], k=60, top_k=pool)
        ocand[qi, :len(keys)] = keys
    np.testing.assert_array_equal(cand, np.where(ocand >= 0, ocand + 1000, -1))
    assert (cand[3] >= 0).sum() == 3                                     # the 3-row tenant: 3 candidates, padded
    pid, ptt, plen = build_pairs(q_tok, q_len, ocand, tok, tok_len, L)
    ologit = B.forward_logits(wts, cfg, pid, ptt, plen).reshape(Q, pool)
    for qi in range(Q):
        for j in range(k):
            if ids[qi, j] < 0:
                continue
            src = int(np.nonzero(ocand[qi] == ids[qi, j] - 1000)[0][0])
            assert abs(float(lg[qi, j]) - float(ologit[qi, src])) < 4e-3
            assert abs(float(sc[qi, j]) - O.sigmoid(float(ologit[qi, src]))) < 1e-3


# ------------------------------------------------------------------------------------- 8. host array lifetime and ordering
def test_tenants_array_is_consumed_before_the_call_returns(engines):
    """A *_dev call queued on a non-default stream behind 200 ms of pending work; the tenants array is overwritten the moment the
    call returns; after the synchronise the results are those of the ORIGINAL array - and the call did not wait for the stream."""
    import torch
    w = bm_world(engines, ("packed", 0), opts=(("bm25_packed", 0),))
    eng, Q, pool, k = w.eng, 24, 20, 10
    ptr, terms = w.sub(range(Q))
    qd, pd, td = torch.from_numpy(w.q[:Q]).cuda(), torch.from_numpy(ptr).cuda(), torch.from_numpy(terms).cuda()
    tq = np.ascontiguousarray(w.tq[:Q], dtype=np.int32)                  # int32, contiguous: the library reads THIS memory
    other = np.roll(tq, 3).copy()
    assert (other != tq).any()

    def dense(tenants, s):
        o = (torch.empty((Q, k), dtype=torch.int64, device="cuda"), torch.empty((Q, k), dtype=torch.int32, device="cuda"),
             torch.empty((Q, k), dtype=torch.float64, device="cuda"))
        eng.dense_topk_dev(qd, k, o[0], o[1], o[2], tenant=tenants, stream=s)
        return o

    def hybrid(tenants, s):
        return eng.hybrid_rrf_dev(qd, pd, td, pool, k, tenant=tenants, stream=s)

    for call in (dense, hybrid):
        ref = [t.cpu().numpy().copy() for t in call(tq.copy(), None)]
        torch.cuda.synchronize()
        wrong = [t.cpu().numpy().copy() for t in call(other.copy(), None)]
        torch.cuda.synchronize()
        assert any((a != b).any() for a, b in zip(ref, wrong))          # the two arrays do give different results
        s = torch.cuda.Stream()
        live = tq.copy()
        with torch.cuda.stream(s):
            T.busy(s)
            out = call(live, s)
            live[:] = other                                              # overwritten at once
            clones = [o.clone() for o in out]
        pending = not s.query()
        s.synchronize()
        T.assert_same(T.to_np(clones), ref, call.__name__)
        assert pending, f"{call.__name__} waited for the work queued before it on its stream"


# ------------------------------------------------------------------------------------------------------ 9. argument errors
def test_argument_errors_leave_the_outputs_untouched(engines):
    import torch
    from optimized_rag_amd import RagError
    from optimized_rag_amd.bm25 import Bm25Postings
    rng = np.random.default_rng(9)
    N, Q, k = 600, 4, 5
    emb = rng.standard_normal((N, D)).astype(np.float32)
    texts = [" ".join(f"t{t}" for t in rng.integers(0, 50, 6)) for _ in range(N)]
    tq = np.array([0, 1, -1, 0], dtype=np.int32)
    qd = torch.from_numpy(planted(rng, emb, Q)).cuda()

    def outputs():
        return (torch.full((Q, k), 77, dtype=torch.int64, device="cuda"), torch.full((Q, k), 77, dtype=torch.int32, device="cuda"),
                torch.full((Q, k), 77.0, dtype=torch.float64, device="cuda"))

    def untouched(o):
        torch.cuda.synchronize()
        assert all(bool((t == 77).all()) for t in o)

    # a tenant >= 0 without a tenant table
    eng = engines()
    eng.index_load(emb)
    post = Bm25Postings.from_corpus(texts)
    post.load(eng)
    ptr, terms = post.encode_queries(["t1 t2", "t3", "t4 t5", "t6"])
    pd, td = torch.from_numpy(ptr).cuda(), torch.from_numpy(terms).cuda()
    o = outputs()
    with pytest.raises(RagError, match=r"\(-1\).*no tenants loaded"):
        eng.dense_topk_dev(qd, k, *o, tenant=tq)
    with pytest.raises(RagError, match=r"\(-1\)"):
        eng.bm25_topk_dev(pd, td, k, *o, tenant=tq)
    with pytest.raises(RagError, match=r"\(-1\)"):
        eng.dense_topk(qd.cpu().numpy(), k, tenant=tq)
    untouched(o)
    eng.dense_topk_dev(qd, k, *o, tenant=np.full(Q, -1, dtype=np.int32))          # nobody filtered: no table needed
    torch.cuda.synchronize()
    assert bool((o[1] >= 0).all())
    # a stale tenant table: rows appended after it was set
    eng = engines()
    eng.index_reserve(N)
    eng.index_append(emb[:400])
    eng.set_tenants((np.arange(400) % 2).astype(np.int32))
    eng.index_append(emb[400:])
    o = outputs()
    with pytest.raises(RagError, match=r"\(-1\).*stale"):
        eng.dense_topk_dev(qd, k, *o, tenant=tq)
    with pytest.raises(RagError, match=r"\(-1\).*stale"):
        eng.dense_topk_dev(qd, k, *o, tenant=0)                                    # (as the scalar entry answers)
    untouched(o)
    # stale postings: a row inserted behind them
    eng = engines()
    eng.index_load(emb)
    eng.set_tenants((np.arange(N) % 2).astype(np.int32))
    post.load(eng)
    eng.index_insert(emb[:1], tenants=np.array([1], dtype=np.int32))
    o = outputs()
    with pytest.raises(RagError, match=r"\(-3\).*stale"):
        eng.bm25_topk_dev(pd, td, k, *o, tenant=tq)
    with pytest.raises(RagError, match=r"\(-3\).*stale"):
        eng.hybrid_rrf_dev(qd, pd, td, 8, k, tenant=tq)
    with pytest.raises(RagError, match=r"\(-3\).*stale"):
        eng.hybrid_linear_dev(qd, pd, td, k, 0.5, 0.4, 0.1, tenant=tq)
    untouched(o)
    eng.dense_topk_dev(qd, k, *o, tenant=tq)                                       # the dense entry does not need the postings
    torch.cuda.synchronize()
    assert bool((o[1][0] >= 0).all())
