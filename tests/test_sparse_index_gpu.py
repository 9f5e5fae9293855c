"""GPU: the learned-sparse inverted index (rag_sparse_load_host / rag_sparse_topk_* / rag_sparse_scores_host /
rag_hybrid_sparse_rrf_dev) against the float64 reference of tests/sparse_tools.py. Every comparison is bit for bit: the score is
a float64 sum of exact float32 x float32 products in the query's token order (tests/test_sparse_cpu.py shows that the order
matters on this corpus), the top-k a stable order with ties to the lower row, the padding exactly -1 / -1 / 0.0."""
import numpy as np
import pytest

import sparse_tools as S
import stream_tools as T

pytestmark = pytest.mark.gpu

KS = [1, 7, 100, 256, 1024]
N_MID, DIM = 20_000, 64                  # the corpus cut that sits beside a dense index: 10 ranges, so the thresholded stages run
_W = {}


def world():
    """The seeded corpus, its 32 queries and the reference scores, computed once and never written to."""
    if not _W:
        ip, doc, w = S.make_corpus()
        qs = S.make_queries(ip)
        _W.update(full=(ip, doc, w), qs=qs, packed=S.pack_queries(qs), ref=S.all_scores(ip, doc, w, S.N_FULL, qs))
        mid = S.cut(ip, doc, w, N_MID)
        qm = S.make_queries(mid[0], seed=13)
        _W.update(mid=mid, qs_mid=qm, packed_mid=S.pack_queries(qm), ref_mid=S.all_scores(*mid, N_MID, qm))
        rng = np.random.default_rng(5)
        emb = rng.standard_normal((N_MID, DIM)).astype(np.float32)
        _W.update(emb=emb, q=(emb[rng.integers(0, N_MID, 32)] + 0.3 * rng.standard_normal((32, DIM))).astype(np.float32))
        for v in _W.values():
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
    return _W


def engine(postings=None, n_docs=None, dim=DIM, **index):
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=dim, device=0)
    if index:
        e.index_load(index.pop("emb"), **index)
    if postings is not None:
        e.sparse_load(*postings, n_docs)
    return e


@pytest.fixture(scope="module")
def full():
    e = engine(world()["full"], S.N_FULL)
    yield e
    e.close()


@pytest.fixture(scope="module")
def mid():
    """The 20,000-document cut beside a dense index of the same rows with explicit ids and three tenants."""
    w = world()
    e = engine(w["mid"], N_MID, emb=w["emb"], ids=pk())
    e.set_tenants(tenants())
    yield e
    e.close()


def pk():
    return (np.random.default_rng(21).permutation(N_MID) + 1_000_000).astype(np.int64)


def tenants():
    return np.random.default_rng(22).integers(0, 3, N_MID).astype(np.int32)


def topk_dev(e, packed, k, tenant=-1, stream=None, rows=True):
    import torch
    ptr, terms, wts = (torch.from_numpy(np.array(a)).cuda() for a in packed)          # (a copy: the shared arrays are read-only)
    if terms.numel() == 0:
        terms, wts = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.float32, device="cuda")
    Q = ptr.shape[0] - 1
    ids = torch.full((Q, k), -7, dtype=torch.int64, device="cuda")
    rw = torch.full((Q, k), -7, dtype=torch.int32, device="cuda") if rows else None
    sc = torch.full((Q, k), -7.0, dtype=torch.float64, device="cuda")
    e.sparse_topk_dev(ptr, terms, wts, k, ids, rw, sc, stream=stream, tenant=tenant)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), rw.cpu().numpy() if rows else None, sc.cpu().numpy()


def check_lists(got, ref_rows, ref_sc, idmap=None, what=""):
    ids, rows, sc = got
    np.testing.assert_array_equal(rows, ref_rows, err_msg=what + " rows")
    np.testing.assert_array_equal(S.bits(sc), S.bits(ref_sc), err_msg=what + " score bits")
    want = ref_rows.astype(np.int64) if idmap is None else np.where(ref_rows >= 0, idmap[np.maximum(ref_rows, 0)], -1)
    np.testing.assert_array_equal(ids, want, err_msg=what + " ids")
    pad = ref_rows < 0
    assert (ids[pad] == -1).all() and (rows[pad] == -1).all() and (S.bits(sc[pad]) == 0).all(), what + " padding"


def test_info_reports_the_resident_form(full):
    ip, doc, _ = world()["full"]
    info = full.sparse_info()
    assert (info["n_docs"], info["n_terms"], info["nnz"]) == (S.N_FULL, S.V_FULL, doc.shape[0])
    # 8 B per posting (+ 8 postings of padding), 32 B per term, tables of at most a quarter of the postings x 4 B
    assert 8 * (doc.shape[0] + 8) + 32 * S.V_FULL <= info["hbm_bytes"] <= 9 * (doc.shape[0] + 8) + 32 * S.V_FULL
    e = engine()
    try:
        assert e.sparse_info() == dict(n_docs=0, n_terms=0, nnz=0, hbm_bytes=0)
    finally:
        e.close()


def test_every_score_of_every_query_is_bit_equal():
    w = world()
    n = 6000
    post = S.cut(*w["full"], n)
    e = engine(post, n)
    try:
        got = e.sparse_scores(*w["packed"])
        np.testing.assert_array_equal(S.bits(got), S.bits(S.all_scores(*post, n, w["qs"])))
        assert got.shape == (32, n) and (got[25:28] == 0).all()
        # the plan holds 8 token slots: the tokens past it are searched, and weighted, inside the scoring kernel
        e.set_option("bm25_plan_slots", 8)
        np.testing.assert_array_equal(S.bits(e.sparse_scores(*w["packed"])), S.bits(got))
    finally:
        e.close()


@pytest.mark.parametrize("k", KS)
def test_topk_host_and_device_equal_the_reference(full, k):
    w = world()
    ref_rows, ref_sc = S.topk_all(w["ref"], k)
    host = full.sparse_topk(*w["packed"], k)
    check_lists(host, ref_rows, ref_sc, what=f"host k={k}")
    dev = topk_dev(full, w["packed"], k)
    check_lists(dev, ref_rows, ref_sc, what=f"dev k={k}")
    assert (ref_rows[24] >= 0).sum() in range(1, 100) and (ref_rows[25:28] == -1).all()


def test_a_query_does_not_depend_on_its_batch(full):
    w = world()
    k = 100
    ref_rows, ref_sc = S.topk_all(w["ref"], k)
    tiled = S.pack_queries((w["qs"] * 7)[:200])                     # 200 queries: past the 128 of the XCD-column grid
    for got in (full.sparse_topk(*tiled, k), topk_dev(full, tiled, k)):
        for b in range(0, 200, 32):
            n = min(32, 200 - b)
            check_lists(tuple(a[b:b + n] for a in got), ref_rows[:n], ref_sc[:n], what=f"tiled batch at {b}")
    for i in (0, 3, 24, 25, 28, 29):
        one = S.pack_queries([w["qs"][i]])
        check_lists(full.sparse_topk(*one, k), ref_rows[i:i + 1], ref_sc[i:i + 1], what=f"query {i} alone")
    # without rows_out
    ids, _, sc = topk_dev(full, w["packed"], k, rows=False)
    np.testing.assert_array_equal(ids, ref_rows.astype(np.int64))
    # sort-merge and exact-select paths give the same lists
    for opt in ("bm25_sort_merge", "bm25_no_staging", "bm25_linear_grid"):
        full.set_option(opt, 1)
        try:
            check_lists(full.sparse_topk(*tiled, k), *S.topk_all(np.concatenate([w["ref"]] * 7)[:200], k), what=opt)
        finally:
            full.set_option(opt, 0)


def test_a_tie_plateau_is_cut_by_the_lowest_rows():
    vals = [0.25, 0.5, 1.0]
    ip, doc, wt = S.make_corpus(weight_values=vals)
    by_df = np.argsort(-np.diff(ip), kind="stable")
    qs = [(by_df[[6, 7, 8]], np.array([1.0, 0.5, 0.25], dtype=np.float32))] + S.make_queries(ip, weight_values=[1.0, 0.5, 0.25])[:12]
    ref = S.all_scores(ip, doc, wt, S.N_FULL, qs)
    e = engine((ip, doc, wt), S.N_FULL)
    try:
        for k in (100, 256):
            rr, rs = S.topk_all(ref, k)
            assert (ref[0] == rs[0, k - 1]).sum() > 100 and (ref[0] > rs[0, k - 1]).sum() < k          # the plateau crosses k
            check_lists(e.sparse_topk(*S.pack_queries(qs), k), rr, rs, what=f"ties host k={k}")
            check_lists(topk_dev(e, S.pack_queries(qs), k), rr, rs, what=f"ties dev k={k}")
    finally:
        e.close()


@pytest.mark.parametrize("n", [1, 5, 2048, 2049])
def test_small_corpora_with_k_above_the_matches(n):
    w = world()
    post = S.cut(*w["full"], n)
    ref = S.all_scores(*post, n, w["qs"])
    e = engine(post, n)
    try:
        for k in (1, 10, 1024):
            rr, rs = S.topk_all(ref, k)
            check_lists(e.sparse_topk(*w["packed"], k), rr, rs, what=f"n={n} k={k}")
        check_lists(topk_dev(e, w["packed"], 64), *S.topk_all(ref, 64), what=f"n={n} dev")
        np.testing.assert_array_equal(S.bits(e.sparse_scores(*w["packed"])), S.bits(ref))
    finally:
        e.close()


def test_ids_tenants_and_deleted_rows_follow_the_dense_index():
    from optimized_rag_amd._lib import RagError
    w = world()
    ids, ten = pk(), tenants()
    e = engine(w["mid"], N_MID, emb=w["emb"], ids=ids)
    try:
        k = 100
        with pytest.raises(RagError, match=r"\(-1\)"):               # a dense index without a tenant table
            e.sparse_topk(*w["packed_mid"], k, tenant=1)
        e.set_tenants(ten)
        check_lists(e.sparse_topk(*w["packed_mid"], k), *S.topk_all(w["ref_mid"], k), idmap=ids, what="explicit ids")
        for t in (0, 2):
            rr, rs = S.topk_all(w["ref_mid"], k, hidden=ten != t)
            assert (ten[rr[rr >= 0]] == t).all()
            check_lists(e.sparse_topk(*w["packed_mid"], k, tenant=t), rr, rs, idmap=ids, what=f"tenant {t} host")
            check_lists(topk_dev(e, w["packed_mid"], k, tenant=t), rr, rs, idmap=ids, what=f"tenant {t} dev")
        # delete the top documents of some queries: they vanish, the lists are the reference's with those rows masked
        top = np.unique(S.topk_all(w["ref_mid"], 5)[0][[0, 1, 5, 12, 24]])
        top = top[top >= 0]
        assert e.index_delete(ids[top]) == top.shape[0]
        hidden = np.zeros(N_MID, dtype=bool)
        hidden[top] = True
        rr, rs = S.topk_all(w["ref_mid"], k, hidden=hidden)
        assert not np.isin(rr, top).any()
        check_lists(e.sparse_topk(*w["packed_mid"], k), rr, rs, idmap=ids, what="after deletes host")
        check_lists(topk_dev(e, w["packed_mid"], k), rr, rs, idmap=ids, what="after deletes dev")
        check_lists(e.sparse_topk(*w["packed_mid"], k, tenant=1), *S.topk_all(w["ref_mid"], k, hidden=hidden | (ten != 1)), idmap=ids,
                    what="after deletes, tenant 1")
        sc = e.sparse_scores(*w["packed_mid"])
        np.testing.assert_array_equal(S.bits(sc), S.bits(np.where(hidden[None, :], 0.0, w["ref_mid"])))
        # an insert leaves the postings stale: the sparse entries refuse, the handle and the dense search go on
        n_new = 40
        rng = np.random.default_rng(8)
        new_emb = rng.standard_normal((n_new, DIM)).astype(np.float32)
        new_ids = np.arange(n_new, dtype=np.int64) + 5_000_000
        e.index_insert(new_emb, ids=new_ids, tenants=np.full(n_new, 1, dtype=np.int32))
        for call in (lambda: e.sparse_topk(*w["packed_mid"], k), lambda: e.sparse_scores(*w["packed_mid"]),
                     lambda: topk_dev(e, w["packed_mid"], k), lambda: hybrid(e, w["q"], w["packed_mid"], 100, 20)):
            with pytest.raises(RagError, match=r"\(-3\)"):
                call()
        d_ids, _, _ = e.dense_topk(new_emb[:4], 1)
        np.testing.assert_array_equal(d_ids[:, 0], new_ids[:4])
        # a reload of the extended postings makes them current
        ext = S.cut(*w["full"], N_MID + n_new)
        e.sparse_load(*ext, N_MID + n_new)
        ref_ext = S.all_scores(*ext, N_MID + n_new, w["qs_mid"])
        hid_ext = np.concatenate([hidden, np.zeros(n_new, dtype=bool)])
        check_lists(e.sparse_topk(*w["packed_mid"], k), *S.topk_all(ref_ext, k, hidden=hid_ext), idmap=np.concatenate([ids, new_ids]),
                    what="after the reload")
        # compaction leaves them stale again
        e.index_compact()
        with pytest.raises(RagError, match=r"\(-3\)"):
            e.sparse_topk(*w["packed_mid"], k)
    finally:
        e.close()


def test_a_tenant_filter_without_a_dense_index_is_an_argument_error(full):
    from optimized_rag_amd._lib import RagError
    w = world()
    with pytest.raises(RagError, match=r"\(-1\)"):
        full.sparse_topk(*w["packed"], 10, tenant=0)
    with pytest.raises(RagError, match=r"\(-1\)"):
        topk_dev(full, w["packed"], 10, tenant=0)
    check_lists(full.sparse_topk(*w["packed"], 10), *S.topk_all(w["ref"], 10), what="after the refused calls")


def test_a_rejected_load_leaves_the_index_as_it_was():
    from optimized_rag_amd._lib import RagError
    w = world()
    n = 3000
    post = S.cut(*w["full"], n)
    ref = S.topk_all(S.all_scores(*post, n, w["qs"]), 50)
    e = engine(post, n)
    try:
        ip, doc, wt = (a.copy() for a in post)
        t = int(np.argmax(np.diff(ip)))
        a = int(ip[t])

        def broken(**kw):
            d, x, p, nd, nt = doc.copy(), wt.copy(), ip.copy(), n, ip.shape[0] - 1
            if "swap" in kw:
                d[a], d[a + 1] = d[a + 1], d[a]
            if "dup" in kw:
                d[a + 1] = d[a]
            if "big" in kw:
                d[int(ip[t + 1]) - 1] = n
            if "neg" in kw:
                d[a] = -1
            if "weight" in kw:
                x[a + 2] = kw["weight"]
            if "indptr" in kw:
                p[t + 1] -= 1
                p[t + 2] = p[t + 1] - 1
            return p, d, x, kw.get("n_docs", nd)

        for kw in (dict(swap=1), dict(dup=1), dict(big=1), dict(neg=1), dict(weight=0.0), dict(weight=-1.0), dict(weight=np.nan),
                   dict(weight=np.inf), dict(indptr=1), dict(n_docs=0)):
            with pytest.raises(RagError, match=r"\(-1\)"):
                e.sparse_load(*broken(**kw))
            assert e.sparse_info()["n_docs"] == n
            check_lists(e.sparse_topk(*w["packed"], 50), *ref, what=f"after the rejected load {kw}")
        # a second load replaces the first
        post2 = S.cut(*w["full"], 1000)
        e.sparse_load(*post2, 1000)
        check_lists(e.sparse_topk(*w["packed"], 50), *S.topk_all(S.all_scores(*post2, 1000, w["qs"]), 50), what="second load")
    finally:
        e.close()


def test_bm25_and_sparse_postings_are_resident_side_by_side():
    from optimized_rag_amd.bm25 import Bm25Postings
    w = world()
    rng = np.random.default_rng(4)
    words = [f"w{i}" for i in range(300)]
    corpus = [" ".join(rng.choice(words, int(rng.integers(5, 40)))) for _ in range(5000)]
    bm = Bm25Postings.from_corpus(corpus)
    bq = bm.encode_queries([" ".join(rng.choice(words, 5)) for _ in range(16)])
    n = 6000
    post = S.cut(*w["full"], n)
    ref = S.topk_all(S.all_scores(*post, n, w["qs"]), 100)
    e = engine()
    try:
        bm.load(e)
        before = e.bm25_topk(*bq, 100)
        e.sparse_load(*post, n)
        after = e.bm25_topk(*bq, 100)
        for x, y in zip(before, after):
            np.testing.assert_array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y)
        check_lists(e.sparse_topk(*w["packed"], 100), *ref, what="beside BM25")
        bm.load(e)                                                   # ... and the other way round
        check_lists(e.sparse_topk(*w["packed"], 100), *ref, what="after a BM25 reload")
        assert (e.bm25_topk(*bq, 100)[2] == before[2]).all()
    finally:
        e.close()


def test_two_half_shards_merge_into_the_unsharded_list():
    import torch
    from optimized_rag_amd.sparse import LexicalPostings
    w = world()
    k, half = 100, 9_000
    p = LexicalPostings(*w["mid"], N_MID)
    ref_rows, ref_sc = S.topk_all(w["ref_mid"], k)
    lists = []
    for a, b in ((0, half), (half, N_MID)):
        e = engine(dim=DIM, emb=w["emb"][a:b], id_base=a)
        try:
            p.shard(a, b).load(e)
            ids, _, sc = topk_dev(e, w["packed_mid"], k)
            lists.append((ids, sc))
        finally:
            e.close()
    e = engine()
    try:
        ids = torch.from_numpy(np.stack([x[0] for x in lists])).cuda()
        sc = torch.from_numpy(np.stack([x[1] for x in lists])).cuda()
        out_ids, out_sc = torch.empty((32, k), dtype=torch.int64, device="cuda"), torch.empty((32, k), dtype=torch.float64, device="cuda")
        e.merge_topk_dev(ids, sc, out_ids, out_sc)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out_ids.cpu().numpy(), ref_rows.astype(np.int64))
        np.testing.assert_array_equal(S.bits(out_sc.cpu().numpy()), S.bits(ref_sc))
    finally:
        e.close()


def hybrid(e, q, packed, pool, k, tenant=-1, stream=None):
    import torch
    ptr, terms, wts = (torch.from_numpy(np.array(a)).cuda() for a in packed)          # (a copy: the shared arrays are read-only)
    keys, rrf, ranks = e.hybrid_sparse_rrf_dev(torch.from_numpy(np.array(q)).cuda(), ptr, terms, wts, pool, k, tenant=tenant,
                                               stream=stream)
    torch.cuda.synchronize()
    return keys.cpu().numpy(), rrf.cpu().numpy(), ranks.cpu().numpy()


def test_hybrid_equals_the_three_call_composition_and_the_oracle(mid):
    import torch
    from oracle import rag_oracle as O
    w = world()
    Q, pool, k = 32, 100, 20
    ids = pk()
    for tenant in (-1, 1):
        keys, rrf, ranks = hybrid(mid, w["q"], w["packed_mid"], pool, k, tenant=tenant)
        # the composition: dense top-pool, sparse top-pool, RRF - one call after another
        q = torch.from_numpy(np.array(w["q"])).cuda()
        lists = torch.empty((Q, 2, pool), dtype=torch.int64, device="cuda")
        d_ids, d_rows, d_sc = (torch.empty((Q, pool), dtype=t, device="cuda") for t in (torch.int64, torch.int32, torch.float64))
        mid.dense_topk_dev(q, pool, d_ids, d_rows, d_sc, tenant=tenant)
        s_ids, _, _ = topk_dev(mid, w["packed_mid"], pool, tenant=tenant)
        lists[:, 0], lists[:, 1] = d_ids, torch.from_numpy(s_ids).cuda()
        c_keys, c_rrf, c_ranks = (torch.empty((Q, k), dtype=torch.int64, device="cuda"), torch.empty((Q, k), dtype=torch.float64, device="cuda"),
                                  torch.empty((Q, k, 2), dtype=torch.int32, device="cuda"))
        mid.rrf_fuse_dev(lists, c_keys, c_rrf, c_ranks)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(keys, c_keys.cpu().numpy())
        np.testing.assert_array_equal(S.bits(rrf), S.bits(c_rrf.cpu().numpy()))
        np.testing.assert_array_equal(ranks, c_ranks.cpu().numpy())
        # the oracle's RRF over the reference lists
        hidden = None if tenant < 0 else tenants() != tenant
        ref_rows, _ = S.topk_all(w["ref_mid"], pool, hidden=hidden)
        dense = d_ids.cpu().numpy()
        n_sparse = (ref_rows >= 0).sum(axis=1)
        assert (n_sparse == 0).any() and ((n_sparse > 0) & (n_sparse < pool)).any() and (n_sparse == pool).any()
        for i in range(Q):
            sparse = [int(ids[r]) for r in ref_rows[i] if r >= 0]
            o_keys, o_sc, o_ranks = O.rrf_fuse([[int(x) for x in dense[i] if x >= 0], sparse], k=60, top_k=k)
            n = len(o_keys)
            assert n == k
            np.testing.assert_array_equal(keys[i], o_keys)
            np.testing.assert_array_equal(S.bits(rrf[i]), S.bits(np.asarray(o_sc)))
            np.testing.assert_array_equal(ranks[i], np.asarray(o_ranks, dtype=np.int32))
            if not sparse:                                           # an empty sparse list: the dense list's order
                np.testing.assert_array_equal(keys[i], dense[i, :k])


def test_device_calls_are_ordered_on_their_stream(mid):
    import torch
    w = world()
    k = 50
    ptr, terms, wts = w["packed_mid"]
    ref_rows, ref_sc = S.topk_all(w["ref_mid"], k)
    ids = pk()

    def call(d, s):
        o_ids = torch.empty((32, k), dtype=torch.int64, device="cuda")
        o_rows = torch.empty((32, k), dtype=torch.int32, device="cuda")
        o_sc = torch.empty((32, k), dtype=torch.float64, device="cuda")
        mid.sparse_topk_dev(d["ptr"], d["terms"], d["w"], k, o_ids, o_rows, o_sc, stream=s)
        return [o_ids, o_rows, o_sc]

    wrong = dict(ptr=np.zeros_like(ptr), terms=np.zeros_like(terms), w=np.zeros_like(wts))       # legal: 32 empty queries
    real = dict(ptr=ptr, terms=terms, w=wts)
    s = torch.cuda.Stream()
    got, pending = T.late_producer(call, wrong, real, s)
    assert pending, "rag_sparse_topk_dev waited for the work queued before it on its stream"
    check_lists(tuple(got), ref_rows, ref_sc, idmap=ids, what="behind a late producer")


def test_a_load_behind_a_queued_search_waits_for_it():
    import torch
    w = world()
    k = 50
    old, new = S.cut(*w["full"], 8000), S.cut(*w["full"], 5000)
    ref_old = S.topk_all(S.all_scores(*old, 8000, w["qs"]), k)
    ref_new = S.topk_all(S.all_scores(*new, 5000, w["qs"]), k)
    e = engine(old, 8000)
    try:
        dev = T.to_dev(dict(zip(("ptr", "terms", "w"), w["packed"])))
        s = torch.cuda.Stream()

        def call():
            out = [torch.empty((32, k), dtype=t, device="cuda") for t in (torch.int64, torch.int32, torch.float64)]
            e.sparse_topk_dev(dev["ptr"], dev["terms"], dev["w"], k, *out, stream=s)
            return out
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            call()                                                   # first-use workspace growth out of the way
            s.synchronize()
            T.busy(s)
            queued = [o.clone() for o in call()]
        assert not s.query()
        e.sparse_load(*new, 5000)                                    # a host write: returns after the queued search
        assert s.query(), "rag_sparse_load_host returned while the queued search was still pending"
        with torch.cuda.stream(s):
            later = [o.clone() for o in call()]
        s.synchronize()
        check_lists(tuple(T.to_np(queued)), *ref_old, what="queued before the load")
        check_lists(tuple(T.to_np(later)), *ref_new, what="after the load")
    finally:
        e.close()
