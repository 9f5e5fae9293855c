"""GPU: a tenant PER QUERY for the learned-sparse index and the bge-m3 composites (rag_sparse_topk_tenants_*,
rag_hybrid_sparse_rrf_tenants_dev, rag_retrieve_maxsim_tenants_dev, rag_retrieve_m3_tenants_dev; the RagEngine methods with
`tenant=` an array).

Every result is held against BOTH
  * the scalar-tenant entry, called once per distinct tenant over that tenant's queries: np.array_equal, floats by their bits;
  * the numpy reference, per query: sparse_tools.topk over the all-document scores with hidden = (another tenant's row | a deleted
    row) - rows, ids and score bits exact; the oracle's dense top-k under the tenant (ids exact) and its RRF (keys, scores and
    ranks exact); m3_fused_tools.combine over the float64 cosine, the all-document sparse score and MaxSim of the STORED fp16
    vectors. Bars (those of test_sparse_index_gpu.py, test_tokvec_gpu.py and test_m3_fused_gpu.py): sparse bit-exact, a dense
    component within 1e-9, a MaxSim score within 1e-4, a three-way score within (w_colbert / sum) * 1e-4 + 1e-9.
The world is the smallest that reaches each path: 4,613 documents = three 2048-document ranges, the last one partial, 300 live
terms, dim 64, token vectors of 32 d; 14 queries whose tenants cycle through test_tenants_per_query_gpu's layouts - two interleaved
tenants [0, 1], one stored contiguously across the 2048 boundary [2], the rest [3], one of 3 rows, fewer than k [4], a number that
owns no row [5], unfiltered [-1]."""
import ctypes as C

import numpy as np
import pytest

import m3_fused_tools as F
import m3_tools as M
import sparse_tools as S
import tokvec_tools as V
from oracle import rag_oracle as O
from test_tenants_per_query_gpu import DEAD, QUERY_TENANTS, assert_same, by_tenant, layout, oracle_dense

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = r"\(-1\)", r"\(-3\)"
N, N_TERMS, D, TOK_DIM = 4613, 300 + S.N_EMPTY, 64, 32
NQ_ALL, NQ = 50, 14
POOL, K = 20, 10
TAIL = 600
_W = {}


def world():
    """the seeded data, built once and read-only: embeddings, explicit ids, the tenant of every row, the sparse CSR, 1-11 token
    vectors per document, 50 queries (1-6 frequent and Zipf-drawn terms each, 1-8 token vectors, a planted dense vector) and the
    float64 sparse score of every (query, document)"""
    if not _W:
        rng = np.random.default_rng(19)
        indptr, doc, w = S.make_corpus(n_docs=N, n_terms=N_TERMS, seed=3)
        by_df = np.argsort(-np.diff(indptr), kind="stable")
        queries = []
        for i in range(NQ_ALL):
            n = int(rng.integers(1, 7))
            terms = np.concatenate([by_df[rng.integers(0, 8, 1)], rng.integers(0, 300, n - 1)]).astype(np.int32)
            queries.append((terms, (rng.random(n) * 2.0).astype(np.float32) + np.float32(1e-3)))
        emb = rng.standard_normal((N, D)).astype(np.float32)
        q_emb = (emb[rng.integers(0, N, NQ_ALL)] + 0.4 * rng.standard_normal((NQ_ALL, D))).astype(np.float32)
        counts = rng.integers(1, 12, N)
        d_vecs = V.unit_rows(rng, int(counts.sum()), TOK_DIM)
        d_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        qvecs = [V.unit_rows(rng, int(c), TOK_DIM) for c in rng.integers(1, 9, NQ_ALL)]
        ten = layout(N)
        _W.update(indptr=indptr, doc=doc, w=w, queries=queries, all=S.all_scores(indptr, doc, w, N, queries), emb=emb, q_emb=q_emb,
                  d_vecs=d_vecs, d_off=d_off, stored=V.fp16_round(d_vecs), qvecs=qvecs, ten=ten,
                  ids=(7000 + 2 * np.arange(N)).astype(np.int64), tq=np.resize(QUERY_TENANTS, NQ_ALL).astype(np.int32))
        for t in range(5):                                               # every tenant that owns rows matches something
            for q in np.nonzero(_W["tq"][:NQ] == t)[0]:
                assert (_W["all"][q][ten == t] > 0).any()
        assert ((ten == 2).nonzero()[0].min() < 2048 < (ten == 2).nonzero()[0].max()) and (ten == 4).sum() == 3 and not (ten == 5).any()
    return _W


def block_csr(lo, hi):
    """the postings of the documents [lo, hi), renumbered from 0"""
    w = world()
    sel = (w["doc"] >= lo) & (w["doc"] < hi)
    term_of = np.repeat(np.arange(N_TERMS, dtype=np.int64), np.diff(w["indptr"]))
    indptr = np.zeros(N_TERMS + 1, dtype=np.int64)
    np.cumsum(np.bincount(term_of[sel], minlength=N_TERMS), out=indptr[1:])
    return indptr, (w["doc"][sel] - lo).astype(np.int32), np.ascontiguousarray(w["w"][sel])


def block_vecs(lo, hi):
    w = world()
    return M.pack([w["d_vecs"][w["d_off"][i]:w["d_off"][i + 1]] for i in range(lo, hi)], TOK_DIM)


def make_engine(n0=N, sparse=True, tokvec=True, tenants=True, headroom=0, opts=()):
    from optimized_rag_amd import RagEngine
    w = world()
    e = RagEngine(dim=D, device=0)
    for name, v in opts:
        e.set_option(name, v)
    e.index_load(np.array(w["emb"][:n0]), ids=np.array(w["ids"][:n0]))
    if tenants:
        e.set_tenants(np.array(w["ten"][:n0]))
    if sparse:
        e.sparse_load(*block_csr(0, n0), n0)
    if tokvec:
        v, off = block_vecs(0, n0)
        e.tokvec_reserve(n0 + headroom, int(off[-1]) + 16 * headroom, TOK_DIM)
        e.tokvec_append(v, off)
    return e


@pytest.fixture(scope="module")
def full():
    e = make_engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def live():
    """the last 600 documents arrive as live writes - rows inserted with their tenants, postings appended as a tail segment that is
    not folded, token vectors appended - after 60 rows of the base were deleted"""
    w = world()
    n0 = N - TAIL
    e = make_engine(n0=n0, headroom=TAIL, opts=(("sparse_tail_fold", -1),))
    dead = np.concatenate([np.arange(3, n0, 67), [5]])                   # tenant 4's row 5 among them
    assert e.index_delete(w["ids"][dead]) == dead.shape[0]
    e.index_insert(np.array(w["emb"][n0:]), ids=np.array(w["ids"][n0:]), tenants=np.array(w["ten"][n0:]))
    e.sparse_append(*block_csr(n0, N), TAIL)
    e.tokvec_append(*block_vecs(n0, N))
    s = e.sparse_segment_stats()
    assert s["tail_docs"] == TAIL and s["folds"] == 0 and s["base_docs"] == n0
    yield e, dead
    e.close()


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def inputs(sel):
    """the queries `sel` as device tensors: packed terms and weights, dense vectors, packed token vectors"""
    w = world()
    ptr, terms, wts = S.pack_queries([w["queries"][i] for i in sel])
    qv, qo = M.pack([w["qvecs"][i] for i in sel], TOK_DIM)
    return dict(host=(ptr, terms, wts), ptr=_t(ptr), terms=_t(terms), w=_t(wts), q_emb=_t(w["q_emb"][np.asarray(sel)]), qv=_t(qv), qo=_t(qo))


def run_sparse(e, sel, tenant, k, dev):
    import torch
    d = inputs(sel)
    if not dev:
        return e.sparse_topk(*d["host"], k, tenant=tenant)
    n = len(sel)
    o = (torch.empty((n, k), dtype=torch.int64, device="cuda"), torch.empty((n, k), dtype=torch.int32, device="cuda"),
         torch.empty((n, k), dtype=torch.float64, device="cuda"))
    e.sparse_topk_dev(d["ptr"], d["terms"], d["w"], k, *o, tenant=tenant)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in o)


def run_hybrid(e, sel, tenant, pool=POOL, k=K):
    import torch
    d = inputs(sel)
    out = e.hybrid_sparse_rrf_dev(d["q_emb"], d["ptr"], d["terms"], d["w"], pool, k, tenant=tenant)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy().copy() for x in out)


def run_maxsim(e, sel, tenant, mode, pool=POOL, k=K):
    import torch
    d = inputs(sel)
    kw = dict(term_ptr=d["ptr"], terms=d["terms"], weights=d["w"]) if mode else {}
    out = e.retrieve_maxsim_dev(d["q_emb"], d["qv"], d["qo"], pool, k, tenant=tenant, **kw)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy().copy() for x in out)


def run_m3(e, sel, tenant, mode, weights=(0.4, 0.2, 0.4), pool=POOL, k=K):
    import torch
    d = inputs(sel)
    kw = {}
    if mode != 0 or weights[1] > 0:
        kw.update(term_ptr=d["ptr"], terms=d["terms"], weights=d["w"])
    if weights[2] > 0:
        kw.update(q_vecs=d["qv"], q_off=d["qo"])
    out = e.retrieve_m3_dev(d["q_emb"], pool, k, mode=mode, w=weights, tenant=tenant, **kw)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy().copy() for x in out)


def both(run, sel, tq, what):
    """the per-query call, held against the scalar entry once per distinct tenant"""
    sel = np.asarray(sel)
    got = run(sel, tq)
    assert_same(got, by_tenant(lambda s, t: run(sel[s], t), tq), what)
    return got


# ---- the numpy references ------------------------------------------------------------------------------------------------------------
def hidden_of(t, dead=None):
    w = world()
    h = (w["ten"] != t) if t >= 0 else np.zeros(N, dtype=bool)
    if dead is not None:
        h = h.copy()
        h[dead] = True
    return h


def ids_of(rows):
    w = world()
    rows = np.asarray(rows, dtype=np.int64)
    return np.where(rows >= 0, w["ids"][np.maximum(rows, 0)], -1)


def ref_sparse(sel, tq, k, dead=None):
    w = world()
    r = [S.topk(w["all"][q], k, hidden_of(int(t), dead)) for q, t in zip(sel, tq)]
    return np.stack([x[0] for x in r]), np.stack([x[1] for x in r])


def ref_dense(sel, tq, pool, dead=None):
    w = world()
    ten = w["ten"].copy()
    if dead is not None:
        ten[dead] = DEAD
    return oracle_dense(w["emb"], w["q_emb"][np.asarray(sel)], pool, ten, np.asarray(tq))


def ref_candidates(sel, tq, mode, pool, dead=None):
    """candidate ROWS [Q, slots], -1 padded: the dense top-pool, its RRF with the sparse top-pool, or the union of the two"""
    d_rows, _ = ref_dense(sel, tq, pool, dead)
    if mode == 0:
        return d_rows
    s_rows, _ = ref_sparse(sel, tq, pool, dead)
    slots = 2 * pool if mode == 2 else pool
    out = np.full((len(sel), slots), -1, dtype=np.int64)
    for i in range(len(sel)):
        keys, _, _ = O.rrf_fuse([[int(r) for r in d_rows[i] if r >= 0], [int(r) for r in s_rows[i] if r >= 0]], k=60, top_k=slots)
        out[i, :len(keys)] = keys
    return out


def check_sparse(got, sel, tq, k, dead=None):
    rows, sc = ref_sparse(sel, tq, k, dead)
    np.testing.assert_array_equal(got[1], rows)
    np.testing.assert_array_equal(got[0], ids_of(rows))
    np.testing.assert_array_equal(S.bits(got[2]), S.bits(sc))
    w = world()
    for i, t in enumerate(tq):
        live = got[1][i][got[1][i] >= 0]
        assert t < 0 or (w["ten"][live] == t).all()
        if t == 5:
            assert live.shape[0] == 0 and (got[2][i] == 0).all()


def check_hybrid(got, sel, tq, pool, k, dead=None):
    d_rows, _ = ref_dense(sel, tq, pool, dead)
    s_rows, _ = ref_sparse(sel, tq, pool, dead)
    for i in range(len(sel)):
        keys, scores, ranks = O.rrf_fuse([[int(ids_of(r)) for r in d_rows[i] if r >= 0], [int(ids_of(r)) for r in s_rows[i] if r >= 0]],
                                         k=60, top_k=k)
        n = len(keys)
        assert got[0][i, :n].tolist() == keys and (got[0][i, n:] == -1).all()
        assert got[1][i, :n].tolist() == scores and got[2][i, :n].tolist() == ranks


def check_ranked(ids, sc, cand_ids, ref_of_row, bar, what):
    """a returned list against reference scores of the candidate rows: every id is a candidate, scores fall, each is within `bar`
    of its reference, and no candidate left out beats the last one returned by more than the two bars allow"""
    w = world()
    for i in range(ids.shape[0]):
        have = cand_ids[i][cand_ids[i] >= 0]
        n = min(ids.shape[1], have.shape[0])
        assert (ids[i, :n] >= 0).all() and (ids[i, n:] == -1).all() and (sc[i, n:] == 0).all(), what
        rows = (ids[i, :n] - 7000) // 2
        assert set(ids[i, :n].tolist()) <= set(have.tolist()) and len(set(ids[i, :n].tolist())) == n, what
        assert (np.diff(sc[i, :n]) <= 0).all(), what
        ref = np.array([ref_of_row(i, int(r)) for r in rows])
        assert n == 0 or np.abs(sc[i, :n] - ref).max() <= bar, (what, i, np.abs(sc[i, :n] - ref).max())
        for r in (have - 7000) // 2:
            if r not in rows:
                assert ref_of_row(i, int(r)) <= sc[i, n - 1] + 2 * bar, what
        assert (w["ids"][rows] == ids[i, :n]).all()


def maxsim_ref(sel):
    w = world()
    return lambda i, r: M.maxsim(w["qvecs"][sel[i]], w["stored"][w["d_off"][r]:w["d_off"][r + 1]])


def check_maxsim(got, sel, tq, mode, pool, dead=None):
    ids, sc, cand = got
    np.testing.assert_array_equal(cand, ids_of(ref_candidates(sel, tq, mode, pool, dead)))
    check_ranked(ids, sc, cand, maxsim_ref(sel), 1e-4, f"maxsim mode {mode}")


def check_m3(got, sel, tq, mode, weights, pool, dead=None):
    w = world()
    ids, sc, comp, cand = got
    wd, ws, wc = weights
    np.testing.assert_array_equal(cand, ids_of(ref_candidates(sel, tq, mode, pool, dead)))
    ms = maxsim_ref(sel)

    def parts(i, r):
        cos = F.cosine64(w["q_emb"][sel[i]], w["emb"][r:r + 1])[0] if wd > 0 else 0.0
        return cos, (w["all"][sel[i]][r] if ws > 0 else 0.0), (ms(i, r) if wc > 0 else 0.0)

    bar = (wc / (wd + ws + wc)) * 1e-4 + 1e-9
    check_ranked(ids, sc, cand, lambda i, r: F.combine(*parts(i, r), weights), bar, f"m3 mode {mode} weights {weights}")
    live = ids >= 0
    np.testing.assert_array_equal(S.bits(sc[live]), S.bits(F.combine(comp[..., 0], comp[..., 1], comp[..., 2], weights)[live]))
    assert (comp[~live] == 0).all()
    for i, j in zip(*np.nonzero(live)):
        cos, sp, cb = parts(i, int((ids[i, j] - 7000) // 2))
        assert abs(comp[i, j, 0] - cos) < 1e-9 and S.bits(comp[i, j, 1]) == S.bits(sp) and abs(comp[i, j, 2] - cb) <= 1e-4


SEL, TQ = np.arange(NQ), np.resize(QUERY_TENANTS, NQ).astype(np.int32)


# ---- 1. the sparse top-k --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("k", [10, 1000])                                # 1000: above every tenant's matches but the unfiltered ones'
def test_sparse_topk_mixed_tenants(full, k, dev):
    assert hasattr(full.lib, "rag_sparse_topk_tenants_host") and hasattr(full.lib, "rag_sparse_topk_tenants_dev")
    got = both(lambda s, t: run_sparse(full, s, t, k, dev), SEL, TQ, "sparse_topk")
    check_sparse(got, SEL, TQ, k)
    short = [(got[1][i] >= 0).sum() for i in range(NQ) if TQ[i] == 4]
    assert all(0 < n <= 3 for n in short)


@pytest.mark.parametrize("option,value,sel", [("bm25_first_ranges", 1, SEL),         # the thresholded stage runs (3 ranges > 2 x 1)
                                              ("bm25_plan_slots", 2, None)])         # tokens past the planned slots: weights read in the kernel
def test_sparse_topk_paths_under_mixed_tenants(option, value, sel):
    w = world()
    if sel is None:
        sel = np.array([i for i in range(NQ_ALL) if len(w["queries"][i][0]) == 5][:7])
        assert sel.shape[0] >= 4
    tq = np.resize(QUERY_TENANTS, len(sel)).astype(np.int32)
    e = make_engine(tokvec=False, opts=((option, value),))
    try:
        for dev in (False, True):
            got = both(lambda s, t: run_sparse(e, s, t, 10, dev), sel, tq, option)
            check_sparse(got, sel, tq, 10)
    finally:
        e.close()


def test_sparse_sub_batches_carry_their_tenants(full):
    """k = 1000 and bm25_ws_mb = 1: a query's partial lists take 3 ranges x (12 k + 36) + 12 k bytes, so 1 MiB holds 21 queries and
    the 50 run in 3 sub-batches"""
    k, sel, tq = 1000, np.arange(NQ_ALL), world()["tq"]
    assert (1 << 20) // (3 * (k * 12 + 4 + 8 * 4) + k * 12) == 21
    plain = run_sparse(full, sel, tq, k, True)
    full.set_option("bm25_ws_mb", 1)
    try:
        got = both(lambda s, t: run_sparse(full, s, t, k, True), sel, tq, "sub-batched")
    finally:
        full.set_option("bm25_ws_mb", 0)
    assert_same(got, plain, "sub-batched against one piece")
    check_sparse(got, sel, tq, k)


# ---- 2. the composites ----------------------------------------------------------------------------------------------------------------
def test_hybrid_sparse_rrf_mixed_tenants(full):
    got = both(lambda s, t: run_hybrid(full, s, t), SEL, TQ, "hybrid_sparse_rrf")
    check_hybrid(got, SEL, TQ, POOL, K)


@pytest.mark.parametrize("mode", [0, 1])
def test_retrieve_maxsim_mixed_tenants(full, mode):
    got = both(lambda s, t: run_maxsim(full, s, t, mode), SEL, TQ, f"retrieve_maxsim mode {mode}")
    check_maxsim(got, SEL, TQ, mode, POOL)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_retrieve_m3_mixed_tenants(full, mode):
    got = both(lambda s, t: run_m3(full, s, t, mode), SEL, TQ, f"retrieve_m3 mode {mode}")
    check_m3(got, SEL, TQ, mode, (0.4, 0.2, 0.4), POOL)


@pytest.mark.parametrize("weights,sparse,tokvec", [((0.4, 0.2, 0.0), True, False), ((1.0, 0.0, 1.0), False, True)])
def test_retrieve_m3_without_a_leg(weights, sparse, tokvec):
    e = make_engine(sparse=sparse, tokvec=tokvec)
    try:
        for mode in ((0, 1, 2) if sparse else (0,)):
            got = both(lambda s, t: run_m3(e, s, t, mode, weights), SEL, TQ, f"retrieve_m3 {weights} mode {mode}")
            check_m3(got, SEL, TQ, mode, weights, POOL)
    finally:
        e.close()


# ---- 3. live writes -------------------------------------------------------------------------------------------------------------------
def test_after_live_writes_and_after_the_fold(live):
    e, dead = live

    def everything():
        out = {}
        for dev in (False, True):
            out["sparse", dev] = both(lambda s, t: run_sparse(e, s, t, 10, dev), SEL, TQ, "sparse_topk, live")
            check_sparse(out["sparse", dev], SEL, TQ, 10, dead)
        out["hybrid"] = both(lambda s, t: run_hybrid(e, s, t), SEL, TQ, "hybrid_sparse_rrf, live")
        check_hybrid(out["hybrid"], SEL, TQ, POOL, K, dead)
        out["maxsim"] = both(lambda s, t: run_maxsim(e, s, t, 1), SEL, TQ, "retrieve_maxsim, live")
        check_maxsim(out["maxsim"], SEL, TQ, 1, POOL, dead)
        out["m3"] = both(lambda s, t: run_m3(e, s, t, 2), SEL, TQ, "retrieve_m3, live")
        check_m3(out["m3"], SEL, TQ, 2, (0.4, 0.2, 0.4), POOL, dead)
        return out

    before = everything()
    tail_rows = before["sparse", True][1]
    assert (tail_rows >= N - TAIL).any() and ((tail_rows >= 0) & (tail_rows < N - TAIL)).any()      # both segments contribute
    assert not np.isin(tail_rows, dead).any()
    e.sparse_fold()
    s = e.sparse_segment_stats()
    assert s["tail_docs"] == 0 and s["folds"] == 1
    after = everything()
    for key in before:
        assert_same(after[key], before[key], f"{key} after rag_sparse_fold")


# ---- 4. routing and independence --------------------------------------------------------------------------------------------------------
def all_entries(e, sel, tenant):
    return [run_sparse(e, sel, tenant, 10, False), run_sparse(e, sel, tenant, 10, True), run_hybrid(e, sel, tenant),
            run_maxsim(e, sel, tenant, 1), run_m3(e, sel, tenant, 2)]


def test_uniform_arrays_return_the_scalar_entrys_bits(full):
    for t in (2, -1):
        got, ref = all_entries(full, SEL, np.full(NQ, t, dtype=np.int32)), all_entries(full, SEL, t)
        for g, r in zip(got, ref):
            assert_same(g, r, f"uniform array of {t}")
    got, ref = all_entries(full, SEL, np.array([-1, -5] * 7, dtype=np.int32)), all_entries(full, SEL, -1)      # every value < 0 is "unfiltered"
    for g, r in zip(got, ref):
        assert_same(g, r, "all unfiltered")


def test_negative_scalar_tenants_stay_unfiltered_after_a_per_query_call(live):
    e, dead = live
    ref = all_entries(e, SEL, -1)
    check_sparse(ref[0], SEL, np.full(NQ, -1), 10, dead)
    for t in (-2, -7):
        all_entries(e, SEL, TQ)                                          # the per-query call is the last one before the scalar ones
        for g, r in zip(all_entries(e, SEL, t), ref):
            assert_same(g, r, f"tenant={t}")


def test_a_querys_result_does_not_depend_on_its_batch(full):
    rng = np.random.default_rng(5)
    order = rng.permutation(NQ)
    batch = all_entries(full, SEL[order], TQ[order])
    for pos in range(NQ):
        alone = all_entries(full, SEL[order][pos:pos + 1], TQ[order][pos:pos + 1])
        for b, a in zip(batch, alone):
            assert_same([x[pos:pos + 1] for x in b], a, f"query {order[pos]} alone")


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------------
def test_a_null_tenants_array_is_an_argument_error(full):
    import torch
    d = inputs(SEL)
    p = lambda t: C.c_void_p(t.data_ptr())
    ptr, terms, wts = d["host"]
    h = lambda a: C.c_void_p(a.ctypes.data)
    ids, rows, sc = np.full((NQ, K), -7, np.int64), np.full((NQ, K), -7, np.int32), np.full((NQ, K), np.nan)
    i64 = lambda *s: torch.full(s, -7, dtype=torch.int64, device="cuda")
    f64 = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device="cuda")
    o_ids, o_rows, o_sc, o_cand = i64(NQ, K), torch.full((NQ, K), -7, dtype=torch.int32, device="cuda"), f64(NQ, K), i64(NQ, 2 * POOL)
    lists, ws, ranks, comp = i64(2, NQ, POOL), f64(NQ, POOL), torch.full((NQ, K, 2), -7, dtype=torch.int32, device="cuda"), f64(NQ, K, 3)
    L, H = full.lib, full.h
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    calls = [
        lambda: L.rag_sparse_topk_tenants_host(H, h(ptr), h(terms), h(wts), NQ, K, None, h(ids), h(rows), h(sc)),
        lambda: L.rag_sparse_topk_tenants_dev(H, p(d["ptr"]), p(d["terms"]), p(d["w"]), NQ, K, None, p(o_ids), p(o_rows), p(o_sc), st),
        lambda: L.rag_hybrid_sparse_rrf_tenants_dev(H, p(d["q_emb"]), p(d["ptr"]), p(d["terms"]), p(d["w"]), NQ, POOL, K, 60, None, p(lists), p(ws),
                                                    p(o_ids), p(o_sc), p(ranks), st),
        lambda: L.rag_retrieve_maxsim_tenants_dev(H, p(d["q_emb"]), p(d["ptr"]), p(d["terms"]), p(d["w"]), p(d["qv"]), p(d["qo"]), NQ, POOL, K, 60,
                                                  None, 1, p(o_ids), p(o_sc), p(o_cand), st),
        lambda: L.rag_retrieve_m3_tenants_dev(H, p(d["q_emb"]), p(d["ptr"]), p(d["terms"]), p(d["w"]), p(d["qv"]), p(d["qo"]), NQ, POOL, K, 60,
                                              None, 2, 0.4, 0.2, 0.4, p(o_ids), p(o_sc), p(comp), p(o_cand), st),
    ]
    for call in calls:
        assert call() == -1
    torch.cuda.synchronize()
    assert (ids == -7).all() and (rows == -7).all() and np.isnan(sc).all()
    for t in (o_ids, o_rows, o_sc, o_cand, comp):
        assert (t.cpu().numpy() == -7).all()


def test_a_tenants_array_fails_where_the_scalar_filter_fails():
    from optimized_rag_amd import RagError
    w = world()
    mixed = TQ
    e = make_engine(tenants=False)                                       # no tenant table
    try:
        for tenant in (1, mixed):
            for call in (lambda: run_sparse(e, SEL, tenant, 10, False), lambda: run_sparse(e, SEL, tenant, 10, True),
                         lambda: run_hybrid(e, SEL, tenant), lambda: run_maxsim(e, SEL, tenant, 1), lambda: run_m3(e, SEL, tenant, 2)):
                with pytest.raises(RagError, match=ERR_ARG):
                    call()
        assert (run_sparse(e, SEL, np.full(NQ, -1, dtype=np.int32), 10, True)[1][:, 0] >= 0).all()      # nothing filtered: served
    finally:
        e.close()
    e = make_engine(sparse=False)                                        # postings of fewer documents than the index has rows
    try:
        e.sparse_load(*block_csr(0, N - 100), N - 100)
        for tenant in (1, mixed):
            for call in (lambda: run_sparse(e, SEL, tenant, 10, False), lambda: run_sparse(e, SEL, tenant, 10, True),
                         lambda: run_hybrid(e, SEL, tenant), lambda: run_maxsim(e, SEL, tenant, 1)):
                with pytest.raises(RagError, match=ERR_ARG):
                    call()
        e.sparse_load(*block_csr(0, N), N)
        both(lambda s, t: run_sparse(e, s, t, 10, True), SEL, TQ, "after the reload")
        e.index_insert(np.array(w["q_emb"][:1]), ids=np.array([1], dtype=np.int64), tenants=np.array([0], dtype=np.int32))
        for tenant in (1, mixed):                                        # stale postings
            for call in (lambda: run_sparse(e, SEL, tenant, 10, False), lambda: run_sparse(e, SEL, tenant, 10, True),
                         lambda: run_hybrid(e, SEL, tenant), lambda: run_m3(e, SEL, tenant, 2, (0.4, 0.2, 0.0))):
                with pytest.raises(RagError, match=ERR_STATE):
                    call()
    finally:
        e.close()
