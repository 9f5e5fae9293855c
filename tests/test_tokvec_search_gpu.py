"""GPU: the exhaustive MaxSim search - mode 2 of rag_retrieve_maxsim_dev / rag_retrieve_maxsim_tenants_dev, tokvec_scan_kernel and
its select (csrc/tokvec.hip), RagEngine.tokvec_search_dev, GpuDocumentIndex.search_late_interaction(mode="maxsim").

Truth comes from code that existed before the search did: rag_tokvec_rerank_host with pair_scores_out over ALL 700 rows of the
world of tests/tokvec_search_tools.py, in three candidate slices of at most 256, gives a [9][700] float32 matrix once per rig
(form x dim); the visibility mask and a numpy stable sort give the lists. Mode 2 must return exactly those ids, those score BITS
(the bit-identity contract of include/rag_hip.h) and those candidates, for every (query, visible document) pair of the world - and
every listed score lies within 1e-4 (the header's bound for the rerank kernel) of float64 MaxSim over the fetched stored rows."""
import ctypes as C

import numpy as np
import pytest

import m3_tools as M
import sparse_tools as S
import tokvec_search_tools as W
import tokvec_tools as V

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = r"\(-1\)", r"\(-3\)"
IDS = (5000 + 3 * np.arange(W.N_DOCS)).astype(np.int64)
Q = len(W.Q_ROWS)
_SPARSE = {}


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sparse_world():
    if not _SPARSE:
        indptr, doc, w = S.make_corpus(n_docs=W.N_DOCS, n_terms=3000, seed=5)
        _SPARSE.update(indptr=indptr, doc=doc, w=w, packed=S.pack_queries(S.make_queries(indptr, seed=6)[:Q]))
    return _SPARSE


def all_pair_scores(e, qv, qo, n_docs):
    """float32 [Q, n_docs]: the rerank entry's own pair score of every (query, row), whatever the row's visibility"""
    parts = []
    for first, n in W.slices(n_docs):
        cand = np.tile(np.arange(first, first + n, dtype=np.int32), (qo.shape[0] - 1, 1))
        parts.append(e.tokvec_rerank(qv, qo, cand, 1)[3])
    return np.concatenate(parts, axis=1)


def float64_scores(e, qv, qo, n_docs):
    """float64 [Q, n_docs]: MaxSim over the rows the store holds (tokvec_fetch), 0.0 where either side has no rows"""
    out = np.zeros((qo.shape[0] - 1, n_docs))
    for d in range(n_docs):
        rows = e.tokvec_fetch(d)
        for q in range(out.shape[0]):
            vq = qv[int(qo[q]):int(qo[q + 1])]
            if rows.shape[0] and vq.shape[0]:
                out[q, d] = M.maxsim(vq, rows)
    return out


@pytest.fixture(scope="module", params=[(f, d) for f in ("fp16", "mxfp8") for d in W.DIMS], ids=lambda p: f"{p[0]}-{p[1]}")
def rig(request):
    from optimized_rag_amd import RagEngine
    form, dim = request.param
    w, sp = W.world(dim), sparse_world()
    e = RagEngine(dim=W.INDEX_DIM, device=0)
    e.index_load(w["emb"], ids=IDS)
    e.set_tenants(w["tenants"])
    e.sparse_load(sp["indptr"], sp["doc"], sp["w"], W.N_DOCS)
    e.tokvec_load(w["vecs"], w["off"], form=form)
    scores = all_pair_scores(e, w["qv"], w["qo"], W.N_DOCS)
    assert scores.shape == (Q, W.N_DOCS)
    best3 = int(np.argmax(np.where(np.diff(w["off"]) > 0, scores[3], -np.inf)))
    deleted = (0, W.LAST_PLAIN, best3)
    assert len({*deleted, W.SRC, *W.COPIES}) == 6
    assert e.index_delete(IDS[list(deleted)]) == 3
    ptr, terms, wts = sp["packed"]
    dev = dict(qv=_t(w["qv"]), qo=_t(w["qo"]), q_emb=_t(w["q_emb"]), ptr=_t(ptr), terms=_t(terms), w=_t(wts))
    yield dict(e=e, w=w, scores=scores, exact=float64_scores(e, w["qv"], w["qo"], W.N_DOCS), deleted=deleted, dev=dev, form=form, dim=dim)
    e.close()


def search(rig, pool, k, tenant=-1):
    import torch
    out = rig["e"].tokvec_search_dev(rig["dev"]["qv"], rig["dev"]["qo"], k, pool=pool, tenant=tenant)
    torch.cuda.synchronize()
    return [t.cpu().numpy().copy() for t in out]


def expected(rig, pool, k, tenant=-1):
    w = rig["w"]
    return W.truth(rig["scores"], W.ranked(w["qo"], w["off"], w["tenants"], rig["deleted"], tenant), pool, k, ids=IDS)


def same(got, exp, what):
    np.testing.assert_array_equal(got[0], exp[0], err_msg=what + ": ids")
    np.testing.assert_array_equal(V.bits(got[1]), V.bits(exp[1]), err_msg=what + ": score bits")
    np.testing.assert_array_equal(got[2], exp[2], err_msg=what + ": candidates")


def test_the_world_holds_the_cases(rig):
    """the preconditions: the three copies tie exactly at the top of the queries cut from document 20, every edge row count is a
    document of every tenant, and the deleted best document of query 3 would otherwise head its list"""
    w, sc = rig["w"], rig["scores"]
    counts = np.diff(w["off"])
    for t in range(3):
        assert set(W.EDGE_ROWS) <= set(counts[w["tenants"] == t].tolist())
    for q in W.Q_NEAR:
        assert sc[q, W.SRC] == sc[q, W.COPIES[0]] == sc[q, W.COPIES[1]] == sc[q].max() > 0.99
    assert (sc[0] == 0).all() and (sc[:, counts == 0] == 0).all()
    ids, _, _ = expected(rig, 5, 5)
    assert IDS[rig["deleted"][2]] not in ids[3] and ids[4, :3].tolist() == IDS[[W.SRC, *W.COPIES]].tolist()


@pytest.mark.parametrize("pool,k", [(37, 10), (256, 256), (1, 1)])
@pytest.mark.parametrize("tenant", [-1, 1, "per_query"])
def test_mode_2_is_the_truth(rig, tenant, pool, k):
    ten = W.PER_QUERY if tenant == "per_query" else tenant
    got, exp = search(rig, pool, k, ten), expected(rig, pool, k, ten)
    same(got, exp, f"{rig['form']} dim {rig['dim']} tenant {tenant} pool {pool} k {k}")
    assert (got[0][0] == -1).all() and (got[1][0] == 0.0).all(), "a query without rows lists nothing"
    if pool == 256 and tenant != -1:
        assert (got[0][1:] == -1).any() and (got[0][1:, 0] >= 0).all(), "more slots than a tenant's documents: padding"
    rows = (got[0] - 5000) // 3
    listed = got[0] >= 0
    qi = np.broadcast_to(np.arange(Q)[:, None], rows.shape)
    err = np.abs(got[1][listed] - rig["exact"][qi[listed], rows[listed]])
    print(f"{rig['form']} dim {rig['dim']} tenant {tenant} pool {pool}: max |score - float64 MaxSim over the stored rows| = {err.max():.3e}")
    assert err.max() < 1e-4


def test_sub_batches_give_the_bits_of_the_default(rig):
    """tokvec_scan_queries = 4 (sub-batches 4 + 4 + 1) and = 1; the two option names exist, an unknown one does not"""
    from optimized_rag_amd import RagError
    e = rig["e"]
    base = search(rig, 37, 10, W.PER_QUERY)
    try:
        for qb in (4, 1):
            e.set_option("tokvec_scan_queries", qb)
            same(search(rig, 37, 10, W.PER_QUERY), base, f"tokvec_scan_queries = {qb}")
        e.set_option("tokvec_scan_queries", 0)
        e.set_option("tokvec_scan_ws_mb", 1)
        same(search(rig, 37, 10, W.PER_QUERY), base, "tokvec_scan_ws_mb = 1")
    finally:
        e.set_option("tokvec_scan_queries", 0)
        e.set_option("tokvec_scan_ws_mb", 0)
    with pytest.raises(RagError, match=ERR_ARG):
        e.set_option("tokvec_scan_rows", 1)


def raw_call(rig, mode, q_emb=True, qv=None, pool=8, k=4):
    """the C entry as it is: its return code"""
    import torch
    e, d = rig["e"], rig["dev"]
    ids = torch.empty((Q, k), dtype=torch.int64, device="cuda")
    sc = torch.empty((Q, k), dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = e.lib.rag_retrieve_maxsim_dev(e.h, p(d["q_emb"]) if q_emb else None, p(d["ptr"]), p(d["terms"]), p(d["w"]),
                                       p(d["qv"] if qv is None else qv), p(d["qo"]), Q, pool, k, 60, -1, mode, p(ids), p(sc), None,
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, ids.cpu().numpy(), sc.cpu().numpy()


def test_arguments(rig):
    """a NULL q_emb is accepted in mode 2 alone; a misaligned q_vecs is refused; mode 3 does not exist; with cand_out NULL the lists
    are the same"""
    import torch
    exp = expected(rig, 8, 4)
    rc, ids, sc = raw_call(rig, 2, q_emb=False)
    assert rc == 0
    np.testing.assert_array_equal(ids, exp[0])
    np.testing.assert_array_equal(V.bits(sc), V.bits(exp[1]))
    assert raw_call(rig, 2)[0] == 0
    for mode in (0, 1):
        assert raw_call(rig, mode)[0] == 0 and raw_call(rig, mode, q_emb=False)[0] == -1
    assert raw_call(rig, 3)[0] == -1
    shifted = torch.empty((rig["dev"]["qv"].numel() + 4,), dtype=torch.float32, device="cuda")
    for by in (1, 2, 3):                                                # 4, 8, 12 bytes past a 16-byte boundary
        qv = shifted[by:by + rig["dev"]["qv"].numel()].view(rig["dev"]["qv"].shape)
        qv.copy_(rig["dev"]["qv"])
        assert qv.data_ptr() % 16 == 4 * by
        assert raw_call(rig, 2, qv=qv)[0] == -1
        assert b"16-byte aligned" in rig["e"].lib.rag_last_error(rig["e"].h)
    for pool, k in ((0, 0), (8, 9), (257, 10)):
        assert raw_call(rig, 2, pool=pool, k=max(k, 1) if pool else 1)[0] == -1


def test_modes_0_and_1_are_unchanged_around_mode_2(rig):
    import torch
    e, d = rig["e"], rig["dev"]

    def composite(mode):
        kw = dict(term_ptr=d["ptr"], terms=d["terms"], weights=d["w"]) if mode else {}
        out = e.retrieve_maxsim_dev(d["q_emb"], d["qv"], d["qo"], 37, 10, tenant=W.PER_QUERY, **kw)
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in out]

    before = [composite(0), composite(1)]
    assert (before[0][0][1:, 0] >= 0).all() and (before[1][0][1:, 0] >= 0).all()
    exp = expected(rig, 256, 256, W.PER_QUERY)
    same(search(rig, 256, 256, W.PER_QUERY), exp, "mode 2 between the composites")
    for mode in (0, 1):
        same(composite(mode), before[mode], f"mode {mode} after mode 2")
    same(search(rig, 256, 256, W.PER_QUERY), exp, "mode 2 after the composites")


def test_a_store_that_does_not_fit_the_index_is_refused():
    """a store of another document count, and a stale one (a plain compaction renumbered the rows): RAG_ERR_STATE"""
    import torch
    from optimized_rag_amd import RagEngine, RagError
    rng = np.random.default_rng(3)
    counts = [3, 0, 17, 5, 40, 1, 16, 2, 9, 33, 4, 8]
    vecs = V.unit_rows(rng, sum(counts), 64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    qv, qo = _t(V.unit_rows(rng, 7, 64)), _t(np.array([0, 3, 7], dtype=np.int64))
    e = RagEngine(dim=32, device=0)
    try:
        e.index_load(rng.standard_normal((12, 32)).astype(np.float32))
        with pytest.raises(RagError, match=ERR_STATE):                  # no store at all
            e.tokvec_search_dev(qv, qo, 3)
        e.tokvec_load(vecs[:off[11]], off[:12])
        with pytest.raises(RagError, match=ERR_STATE):                  # 11 documents for 12 rows
            e.tokvec_search_dev(qv, qo, 3)
        e.tokvec_load(vecs, off)
        ids, sc, cand = e.tokvec_search_dev(qv, qo, 3, pool=12)
        torch.cuda.synchronize()
        assert sorted(cand[0].tolist()) == [-1] + [i for i in range(12) if i != 1]      # the document without rows is never listed
        assert e.index_delete(np.array([4], np.int64)) == 1
        e.index_compact()
        with pytest.raises(RagError, match=ERR_STATE):                  # stale
            e.tokvec_search_dev(qv, qo, 3)
    finally:
        e.close()


# ---- the planted case: a passage only MaxSim finds ----------------------------------------------------------------------------
def planted():
    rng = np.random.default_rng(77)
    n, dim, x = 200, 64, 150
    q_emb = rng.standard_normal(W.INDEX_DIM).astype(np.float32)
    qv = V.unit_rows(rng, 24, dim)
    emb = rng.standard_normal((n, W.INDEX_DIM)).astype(np.float32)
    emb[x] = -q_emb
    docs = [V.unit_rows(rng, int(c), dim) for c in rng.integers(1, 50, n)]
    docs[x] = qv.copy()
    vecs, off = M.pack(docs, dim)
    return dict(n=n, x=x, q_emb=q_emb, qv=qv, emb=emb, vecs=vecs, off=off)


def test_a_passage_only_maxsim_finds():
    """document X: index embedding = the negated query embedding, token vectors = the query's own. The dense pool never holds it;
    the exhaustive search returns it first with a score of 1.0 (within 1e-3: the fp16 store's bound against the original rows)"""
    import torch
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.document_store import GpuDocumentIndex
    p = planted()
    qv, qo, q_emb = _t(p["qv"]), _t(np.array([0, p["qv"].shape[0]], dtype=np.int64)), _t(p["q_emb"][None])
    e = RagEngine(dim=W.INDEX_DIM, device=0)
    try:
        e.index_load(p["emb"])
        e.tokvec_load(p["vecs"], p["off"])
        _, _, cand0 = e.retrieve_maxsim_dev(q_emb, qv, qo, 10, 10)
        torch.cuda.synchronize()
        assert p["x"] not in cand0.cpu().numpy() and (cand0.cpu().numpy() >= 0).all()
        ids, sc, cand = e.tokvec_search_dev(qv, qo, 5, pool=10)
        torch.cuda.synchronize()
        assert int(ids[0, 0]) == p["x"] == int(cand[0, 0]) and abs(float(sc[0, 0]) - 1.0) < 1e-3
    finally:
        e.close()

    class Service:
        """what GpuDocumentIndex asks of its embedding service, answered with the planted query"""
        def generate_embedding(self, text):
            return p["q_emb"].tolist()

        def encode_multi(self, texts, return_dense=True, return_sparse=True, return_colbert_vecs=True):
            return dict(dense_vecs=p["q_emb"][None] if return_dense else None, lexical_weights=None,
                        colbert_vecs=[p["qv"]] if return_colbert_vecs else None)

    e = RagEngine(dim=W.INDEX_DIM, device=0)
    try:
        index = GpuDocumentIndex(Service(), dim=W.INDEX_DIM, engine=e)
        index.bulk_load([dict(content=f"text {i}", agent_id="a" if i % 2 == 0 else "b", filename=f"f{i}") for i in range(p["n"])], p["emb"])
        index.load_token_vectors(p["vecs"], p["off"])
        late = index.search_late_interaction("a", "the query", top_k=5, pool=10, mode="maxsim")
        assert len(late) == 5 and late[0]["filename"] == f"f{p['x']}" and abs(late[0]["colbert_score"] - 1.0) < 1e-3
        assert all(r["score"] == r["colbert_score"] for r in late) and all(int(r["filename"][1:]) % 2 == 0 for r in late)
        assert [r["colbert_score"] for r in late] == sorted((r["colbert_score"] for r in late), reverse=True)
        dense = index.search_late_interaction("a", "the query", top_k=5, pool=10, mode="dense")
        assert len(dense) == 5 and f"f{p['x']}" not in [r["filename"] for r in dense]
        assert index.search_late_interaction("b", "the query", top_k=5, mode="maxsim")[0]["filename"] != f"f{p['x']}"
        assert index.search_late_interaction("nobody", "the query", top_k=5, mode="maxsim") == []
    finally:
        e.close()
