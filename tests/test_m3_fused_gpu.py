"""GPU: the point lookup in the learned-sparse postings (rag_sparse_score_rows_*) and the three-way bge-m3 score over resident data
(rag_m3_score_rows_dev, rag_retrieve_m3_dev, GpuDocumentIndex.search_m3) against the references of tests/m3_fused_tools.py.

Bit-exact: the point scores (against the all-document numpy reference, on the base, across a tail and after a fold), every
component against the entry that owns it (rag_dense_topk_*, the point lookup, rag_tokvec_rerank_dev's pair scores), the combine
against numpy's float64 expression, the selection, the composite against the separate entries, live writes against a fresh handle,
stream order. Bars: a dense component within 1e-9 of numpy's float64 cosine (the bar of the dense search's scores); a score within
(w_colbert / sum) * 1e-4 + 1e-9 of the float64 reference over the STORED fp16 token vectors (the store's bar, scaled by the weight
MaxSim enters with); search_m3 within 1e-3 of m3_tools.score_pairs (the bar search_late_interaction holds)."""
import json

import numpy as np
import pytest

import m3_fused_tools as F
import m3_tools as M
import sparse_tools as S
import stream_tools as T
import tokvec_tools as V
import xlmr_tools as X

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = r"\(-1\)", r"\(-3\)"
N_A, POOL = F.N_A, F.POOL


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _point_dev(e, packed, cand):
    import torch
    ptr, terms, wts = packed
    out = torch.full(cand.shape, float("nan"), dtype=torch.float64, device="cuda")
    e.sparse_score_rows_dev(_t(ptr), _t(terms), _t(wts), _t(cand.astype(np.int32)), out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _expected(all_scores, cand):
    n = all_scores.shape[1]
    ok = (cand >= 0) & (cand < n)
    return np.where(ok, np.take_along_axis(all_scores, np.clip(cand, 0, n - 1).astype(np.int64), axis=1), 0.0)


def _check_points(e, a_all, packed, cand, what):
    exp = _expected(a_all, cand)
    dev = _point_dev(e, packed, cand)
    np.testing.assert_array_equal(S.bits(dev), S.bits(exp), err_msg=what + ": device entry")
    host = e.sparse_score_rows(*packed, cand)
    np.testing.assert_array_equal(S.bits(host), S.bits(dev), err_msg=what + ": host entry")
    return dev


# ---- 1. the point lookup on the base ------------------------------------------------------------------------------------------------
def test_point_lookup_on_the_base():
    from optimized_rag_amd import RagEngine, RagError
    a = F.corpus_a()
    cand = F.slots_a()
    e = RagEngine(dim=64, device=0)
    try:
        with pytest.raises(RagError, match=ERR_STATE):                   # nothing loaded
            e.sparse_score_rows(*a["packed"], cand)
        e.sparse_load(a["indptr"], a["doc"], a["w"], N_A)
        dev = _check_points(e, a["all"], a["packed"], cand, "corpus A")
        assert (dev[:, -2:] == 0).all() and (dev[:, 11] > 0).sum() >= 28 and (dev[0] > 0).sum() >= 10
        # a 300-token query crosses the 256-token chunk
        lq = [F.long_query()]
        _check_points(e, S.all_scores(a["indptr"], a["doc"], a["w"], N_A, lq), S.pack_queries(lq), cand[:1], "300 tokens")
        # a score is a function of its query and row: the same bits at pool 1, at pool 256 among other rows, and in a second run
        for col in (3, 11, 16):
            alone = _point_dev(e, a["packed"], cand[:, col:col + 1])
            np.testing.assert_array_equal(S.bits(alone[:, 0]), S.bits(dev[:, col]))
        rng = np.random.default_rng(23)
        wide = rng.integers(-1, N_A + 2, (32, 256)).astype(np.int32)
        wide[:, 200] = cand[:, 11]
        got = _check_points(e, a["all"], a["packed"], wide, "pool 256")
        np.testing.assert_array_equal(S.bits(got[:, 200]), S.bits(dev[:, 11]))
        np.testing.assert_array_equal(S.bits(_point_dev(e, a["packed"], cand)), S.bits(dev))
        for bad in (np.zeros((32, 257), np.int32), np.zeros((32, 0), np.int32)):
            with pytest.raises(RagError, match=ERR_ARG):
                _point_dev(e, a["packed"], bad)
    finally:
        e.close()


# ---- 2. across a tail ---------------------------------------------------------------------------------------------------------------
def test_point_lookup_across_a_tail_and_after_the_fold():
    from optimized_rag_amd import RagEngine
    a = F.corpus_a()
    V1 = F.V_A + 1                                                       # one more term, known to the appended rows only
    term = np.concatenate([np.repeat(np.arange(F.V_A, dtype=np.int64), np.diff(a["indptr"])), np.full(3, F.V_A, dtype=np.int64)])
    doc = np.concatenate([a["doc"].astype(np.int64), [9005, 9999, 10299]])
    wt = np.concatenate([a["w"], np.array([0.5, 1.25, 2.0], dtype=np.float32)])

    def csr(lo, hi, n_terms):
        sel = (doc >= lo) & (doc < hi) & (term < n_terms)
        order = np.argsort(term[sel] * N_A + doc[sel], kind="stable")
        indptr = np.zeros(n_terms + 1, dtype=np.int64)
        np.cumsum(np.bincount(term[sel], minlength=n_terms), out=indptr[1:])
        return indptr, (doc[sel][order] - lo).astype(np.int32), np.ascontiguousarray(wt[sel][order])

    merged = csr(0, N_A, V1)
    by_df = np.argsort(-np.diff(a["indptr"]), kind="stable")
    queries = list(a["queries"]) + [(np.array([F.V_A]), np.array([1.5], np.float32)),
                                    (np.array([int(by_df[2]), F.V_A, int(by_df[700]), F.V_A]), np.array([0.5, 1.0, 2.0, 0.25], np.float32))]
    packed = S.pack_queries(queries)
    full = S.all_scores(*merged, N_A, queries)
    assert full[32, 9005] == 0.75 and full[33, 10299] >= 2.5 and (full[32, :9000] == 0).all()
    extra = np.tile(np.array([8999, 9000, 9005, 9999, 10000], dtype=np.int32), (len(queries), 1))
    cand = np.concatenate([np.concatenate([F.slots_a(), F.slots_a()[:2]]), extra], axis=1)
    e = RagEngine(dim=64, device=0)
    try:
        e.set_option("sparse_tail_fold", -1)
        e.sparse_load(*csr(0, 9000, F.V_A), 9000)
        e.sparse_append(*csr(9000, 10000, V1), 1000, V1)
        e.sparse_append(*csr(10000, N_A, V1), 300, V1)                  # the second append rebuilds the tail
        st = e.sparse_segment_stats()
        assert st["base_docs"] == 9000 and st["tail_docs"] == 1300
        before = _check_points(e, full, packed, cand, "base 9000 + tail 1300")
        e.sparse_fold()
        assert e.sparse_segment_stats()["tail_docs"] == 0 and e.sparse_segment_stats()["base_docs"] == N_A
        after = _check_points(e, full, packed, cand, "after the fold")
        np.testing.assert_array_equal(S.bits(after), S.bits(before))
    finally:
        e.close()


# ---- 3. combine and selection -------------------------------------------------------------------------------------------------------
def _load(e, keep=None, sparse=True, tokvec=True, tenants=True, headroom=0):
    w = F.world()
    keep = np.arange(N_A) if keep is None else np.asarray(keep)
    e.index_load(np.array(w["emb"][keep]), ids=np.array(w["ids"][keep]))
    if tenants:
        e.set_tenants(np.array(w["tenants"][keep]))
    if sparse:
        e.sparse_load(*F.csr_of_rows(keep), keep.shape[0])
    if tokvec:
        v, off = F.vecs_of_rows(keep)
        e.tokvec_reserve(keep.shape[0] + headroom, off[-1] + 64 * headroom, F.TOK_DIM)
        e.tokvec_append(v, off)


@pytest.fixture(scope="module")
def full():
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=F.DIM, device=0)
    _load(e)
    yield e
    e.close()


def _dev_inputs():
    w, a = F.world(), F.corpus_a()
    ptr, terms, wts = a["packed"]
    return dict(q_emb=w["q_emb"], qv=w["qv"], qo=w["qo"], ptr=ptr, terms=terms, w=wts)


def _score_rows(e, cand, k, weights, dev=None, stream=None):
    """rag_m3_score_rows_dev over candidate rows [Q, pool] -> (ids, rows, scores, components) as numpy"""
    import torch
    d = dev or T.to_dev(_dev_inputs())
    Q = cand.shape[0]
    ids = torch.full((Q, k), -7, dtype=torch.int64, device="cuda")
    rows = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((Q, k), float("nan"), dtype=torch.float64, device="cuda")
    comp = torch.full((Q, k, 3), float("nan"), dtype=torch.float64, device="cuda")
    kw = {}
    if weights[1] > 0:
        kw.update(term_ptr=d["ptr"], terms=d["terms"], weights=d["w"])
    if weights[2] > 0:
        kw.update(q_vecs=d["qv"], q_off=d["qo"])
    cand_dev = cand if hasattr(cand, "is_cuda") else _t(cand.astype(np.int32))
    e.m3_score_rows_dev(cand_dev, k, ids, sc, q_emb=d["q_emb"], w=weights, rows_out=rows, components_out=comp, stream=stream, **kw)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (ids, rows, sc, comp)]


_CAND = {}


def candidates(e):
    """per query the dense top-POOL rows then the sparse top-POOL rows (-1 padded), as the engine's own searches report them,
    with the dense search's score of every row of its list"""
    if not _CAND:
        w, a = F.world(), F.corpus_a()
        _, d_rows, d_sc = e.dense_topk(np.array(w["q_emb"]), POOL)
        _, s_rows, _ = e.sparse_topk(*a["packed"], POOL)
        cand = np.concatenate([d_rows, s_rows], axis=1).astype(np.int32)
        cand[0, 5] = N_A                                                 # a row the index does not have: an empty slot
        _CAND.update(cand=cand, d_rows=d_rows, d_sc=d_sc, s_rows=s_rows)
    return _CAND


def test_candidates_come_from_either_list_and_from_both(full):
    c = candidates(full)
    n = 0
    for q in range(32):
        d, s = set(c["d_rows"][q][c["d_rows"][q] >= 0].tolist()), set(c["s_rows"][q][c["s_rows"][q] >= 0].tolist())
        n += bool(d - s) and bool(s - d) and bool(d & s)
    assert n >= 20, n


@pytest.mark.parametrize("weights", F.WEIGHT_SETS)
def test_components_combine_and_selection(full, weights):
    import torch
    from optimized_rag_amd import RagEngine
    w, a = F.world(), F.corpus_a()
    c = candidates(full)
    cand, pool = c["cand"], 2 * POOL
    wd, ws, wc = weights
    e = full
    if wc == 0 or ws == 0:                                               # a weight of 0: its resident structure is not required
        e = RagEngine(dim=F.DIM, device=0)
        _load(e, sparse=ws > 0, tokvec=wc > 0)
    try:
        ids, rows, sc, comp = _score_rows(e, cand, pool, weights)
    finally:
        if e is not full:
            e.close()
    # the owners of the components, on the full handle
    sparse_pt = _point_dev(full, a["packed"], cand)
    d = T.to_dev(_dev_inputs())
    ps = torch.full((32, pool), float("nan"), dtype=torch.float32, device="cuda")
    full.tokvec_rerank_dev(d["qv"], d["qo"], _t(cand), 1, torch.empty((32, 1), dtype=torch.int64, device="cuda"), None,
                           torch.empty((32, 1), dtype=torch.float64, device="cuda"), ps)
    torch.cuda.synchronize()
    ps = ps.cpu().numpy()
    np.testing.assert_array_equal(S.bits(sparse_pt), S.bits(_expected(a["all"], cand)))
    empty = (cand < 0) | (cand >= N_A)
    stored = V.fp16_round(w["d_vecs"])
    worst_dense = worst_score = 0.0
    slot_scores = np.zeros(cand.shape, dtype=np.float64)
    for q in range(32):
        n = int((~empty[q]).sum())
        assert (rows[q, :n] >= 0).all() and (rows[q, n:] == -1).all() and (ids[q, n:] == -1).all() and (sc[q, n:] == 0).all() and \
            (comp[q, n:] == 0).all(), "every slot that holds a row of the index is ranked, whatever its score; the rest is padding"
        np.testing.assert_array_equal(ids[q, :n], w["ids"][rows[q, :n]])
        of_row = {int(r): comp[q, i] for i, r in enumerate(rows[q, :n])}
        dense_of = {int(r): s for r, s in zip(c["d_rows"][q], c["d_sc"][q]) if r >= 0}
        slot_of = {}
        for j, r in enumerate(cand[q]):
            slot_of.setdefault(int(r), j)
        cos = F.cosine64(w["q_emb"][q], w["emb"][rows[q, :n]])
        vq = w["qv"][w["qo"][q]:w["qo"][q + 1]]
        for i, r in enumerate(rows[q, :n]):
            r = int(r)
            dn, sp, cb = comp[q, i]
            if wd > 0:
                if r in dense_of:
                    assert S.bits(dn) == S.bits(dense_of[r]), "the dense component has the bits the dense search reports"
                worst_dense = max(worst_dense, abs(dn - cos[i]))
            else:
                assert dn == 0
            j = slot_of[r]
            assert S.bits(sp) == (S.bits(sparse_pt[q, j]) if ws > 0 else S.bits(0.0))
            assert S.bits(cb) == (S.bits(np.float64(ps[q, j])) if wc > 0 else S.bits(0.0))
            ref_c = M.maxsim(vq, stored[w["d_off"][r]:w["d_off"][r + 1]]) if wc > 0 else 0.0
            ref = F.combine(cos[i] if wd > 0 else 0.0, a["all"][q][r] if ws > 0 else 0.0, ref_c, weights)
            worst_score = max(worst_score, abs(sc[q, i] - ref))
        np.testing.assert_array_equal(S.bits(sc[q, :n]), S.bits(F.combine(comp[q, :n, 0], comp[q, :n, 1], comp[q, :n, 2], weights)))
        for j, r in enumerate(cand[q]):
            if not empty[q, j]:
                slot_scores[q, j] = F.combine(*of_row[int(r)], weights)
    print(f"m3 score rows, weights {weights}: max |dense - float64 cosine| = {worst_dense:.3e}, max |score - float64 reference| = {worst_score:.3e}")
    assert worst_dense < 1e-9
    assert worst_score < (wc / (wd + ws + wc)) * 1e-4 + 1e-9
    e_ids, e_rows, e_sc = V.stable_topk(slot_scores, cand, empty, pool, idmap=w["ids"])
    np.testing.assert_array_equal(rows, e_rows)
    np.testing.assert_array_equal(ids, e_ids)
    np.testing.assert_array_equal(S.bits(sc), S.bits(e_sc))
    if wc > 0:
        assert (comp[3, :, 2] == 0).all() and (rows[3] >= 0).sum() >= POOL      # query 3 has no token vectors and is ranked all the same
    # a smaller k is the head of the same list; the optional outputs may be left out
    i5, r5, s5, c5 = _score_rows(full, cand, 7, (0.4, 0.2, 0.4)) if weights == F.WEIGHT_SETS[0] else (ids[:, :7], rows[:, :7], sc[:, :7], comp[:, :7])
    np.testing.assert_array_equal(r5, rows[:, :7])
    np.testing.assert_array_equal(S.bits(s5), S.bits(sc[:, :7]))


# ---- 4. the composite ---------------------------------------------------------------------------------------------------------------
def _composite(e, mode, weights=(0.4, 0.2, 0.4), tenant=-1, stream=None, dev=None, pool=POOL, k=10):
    import torch
    d = dev or T.to_dev(_dev_inputs())
    kw = {}
    if mode != 0 or weights[1] > 0:
        kw.update(term_ptr=d["ptr"], terms=d["terms"], weights=d["w"])
    if weights[2] > 0:
        kw.update(q_vecs=d["qv"], q_off=d["qo"])
    out = e.retrieve_m3_dev(d["q_emb"], pool, k, mode=mode, w=weights, tenant=tenant, stream=stream, **kw)
    if stream is None:
        torch.cuda.synchronize()
    return [x.clone() for x in out]


def _separate(e, mode, weights=(0.4, 0.2, 0.4), tenant=-1, pool=POOL, k=10):
    """the search entries, then rag_m3_score_rows_dev on their rows -> (ids, scores, components, candidate ids) as numpy"""
    import torch
    d = T.to_dev(_dev_inputs())
    Q = 32
    i64 = lambda *s: torch.empty(s, dtype=torch.int64, device="cuda")
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")
    if mode == 1:
        keys, _, _ = e.hybrid_sparse_rrf_dev(d["q_emb"], d["ptr"], d["terms"], d["w"], pool, pool, tenant=tenant)
        c_ids = keys.clone()
    else:
        lists = i64(Q, 2, pool)
        d_ids, s_ids = i64(Q, pool), i64(Q, pool)
        e.dense_topk_dev(d["q_emb"], pool, d_ids, None, f64(Q, pool), tenant=tenant)
        c_ids = d_ids
        if mode == 2:
            e.sparse_topk_dev(d["ptr"], d["terms"], d["w"], pool, s_ids, None, f64(Q, pool), tenant=tenant)
            lists[:, 0], lists[:, 1] = d_ids, s_ids
            c_ids = i64(Q, 2 * pool)
            e.rrf_fuse_dev(lists, c_ids, f64(Q, 2 * pool), torch.empty((Q, 2 * pool, 2), dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    c_rows = torch.where(c_ids >= 0, (c_ids - 5000) // 3, c_ids).to(torch.int32).contiguous()      # the world's ids back to rows
    ids, _, sc, comp = _score_rows(e, c_rows, k, weights)
    return [ids, sc, comp, c_ids.cpu().numpy()]


def _same(got, exp, what):
    g = [x.cpu().numpy() if hasattr(x, "cpu") else x for x in got]
    np.testing.assert_array_equal(g[0], exp[0], err_msg=what + ": ids")
    np.testing.assert_array_equal(S.bits(g[1]), S.bits(exp[1]), err_msg=what + ": score bits")
    np.testing.assert_array_equal(S.bits(g[2]), S.bits(exp[2]), err_msg=what + ": component bits")
    np.testing.assert_array_equal(g[3], exp[3], err_msg=what + ": candidates")


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_composite_is_the_search_entries_followed_by_the_score(full, mode):
    got = _composite(full, mode)
    _same(got, _separate(full, mode), f"mode {mode}")
    ids, sc, comp, cand = T.to_np(got)
    assert cand.shape == (32, 2 * POOL if mode == 2 else POOL) and (ids[:, 0] >= 0).sum() >= 30
    for q in range(32):
        live = sc[q][ids[q] >= 0]
        assert (np.diff(live) <= 0).all() and set(ids[q][ids[q] >= 0].tolist()) <= set(cand[q].tolist())
    if mode == 2:
        c = candidates(full)
        w = F.world()
        for q in range(32):
            have = cand[q][cand[q] >= 0]
            assert len(set(have.tolist())) == have.shape[0], "a duplicate in the union"
            both = np.concatenate([c["d_rows"][q], c["s_rows"][q]])
            assert set(w["ids"][both[both >= 0]].tolist()) == set(have.tolist()), "the union holds every row of both lists"
        _same(_composite(full, 2, weights=(0.4, 0.2, 0.0)), _separate(full, 2, weights=(0.4, 0.2, 0.0)), "mode 2 without MaxSim")
    # a tenant filter: only that tenant's rows, and still the separate entries' bits
    got = _composite(full, mode, tenant=1)
    _same(got, _separate(full, mode, tenant=1), f"mode {mode}, tenant 1")
    ids, _, _, cand = T.to_np(got)
    for x in (ids, cand):
        assert (((x[x >= 0] - 5000) // 3) % 3 == 1).all()


def test_deleted_rows_never_appear():
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=F.DIM, device=0)
    try:
        _load(e)
        best = T.to_np(_composite(e, 2))[0][:, :3]
        deleted = np.unique(best[best >= 0])
        assert e.index_delete(deleted) == deleted.shape[0] > 20
        for mode in (0, 1, 2):
            for tenant in (-1, 1):
                got = _composite(e, mode, tenant=tenant)
                ids, _, _, cand = T.to_np(got)
                assert not np.isin(ids, deleted).any() and not np.isin(cand, deleted).any() and (ids[:, 0] >= 0).sum() >= 28
                _same(got, _separate(e, mode, tenant=tenant), f"after deletes, mode {mode}, tenant {tenant}")
    finally:
        e.close()


def test_limits_and_missing_pieces(full):
    from optimized_rag_amd import RagEngine, RagError
    w = F.world()
    for mode, pool, k in ((0, POOL, 0), (0, 8, 9), (2, 129, 10), (0, 257, 10)):
        with pytest.raises(RagError, match=ERR_ARG):
            _composite(full, mode, pool=pool, k=k)
    assert T.to_np(_composite(full, 2, pool=128, k=128))[0].shape == (32, 128)
    for bad in ((-0.1, 0.2, 0.4), (0.0, 0.0, 0.0), (0.4, float("nan"), 0.4), (float("inf"), 0.2, 0.4)):
        with pytest.raises(RagError, match=ERR_ARG):
            _composite(full, 0, weights=bad)
        with pytest.raises(RagError, match=ERR_ARG):
            _score_rows(full, candidates(full)["cand"], 5, bad)
    with pytest.raises(RagError, match=ERR_ARG):
        _composite(full, 3)
    e = RagEngine(dim=F.DIM, device=0)
    try:
        _load(e, tokvec=False)
        with pytest.raises(RagError, match=ERR_STATE):                   # no token-vector store
            _composite(e, 0)
        e.tokvec_load(*F.vecs_of_rows(np.arange(10)))
        with pytest.raises(RagError, match=ERR_STATE):                   # a store of 10 documents beside the index's rows
            _composite(e, 0)
        with pytest.raises(RagError, match=ERR_STATE):
            _score_rows(e, candidates(full)["cand"], 5, (0.4, 0.2, 0.4))
        assert T.to_np(_composite(e, 2, weights=(0.4, 0.2, 0.0)))[0].shape == (32, 10)
        e.index_insert(np.array(w["q_emb"][:1]), ids=np.array([1], dtype=np.int64), tenants=np.array([0], dtype=np.int32))
        for mode in (0, 2):                                              # stale postings, with and without a sparse weight
            with pytest.raises(RagError, match=ERR_STATE):
                _composite(e, mode, weights=(0.4, 0.2 if mode == 0 else 0.0, 0.0))
        with pytest.raises(RagError, match=ERR_STATE):
            _point_dev(e, F.corpus_a()["packed"], F.slots_a())
    finally:
        e.close()


def test_a_refused_composite_leaves_the_handles_id_mapping_alone():
    """64 rows with explicit ids: each of the three resident composites is refused by a state or an argument check, and the dense
    search that follows on the same handle still reports the explicit ids (the composites run their candidate stage in row space)"""
    import torch
    from optimized_rag_amd import RagEngine, RagError
    w = F.world()
    d = T.to_dev(_dev_inputs())
    q_tok = torch.ones((32, 8), dtype=torch.int32, device="cuda")
    q_len = torch.full((32,), 8, dtype=torch.int32, device="cuda")
    e = RagEngine(dim=F.DIM, device=0)
    try:
        _load(e, np.arange(64), sparse=False, tokvec=False, tenants=False)

        def refused(code, call):
            with pytest.raises(RagError, match=code):
                call()
            ids, rows, _ = e.dense_topk(np.array(w["q_emb"]), 4)
            assert (rows >= 0).all() and (rows < 64).all()
            np.testing.assert_array_equal(ids, w["ids"][rows])

        refused(ERR_ARG, lambda: e.retrieve_rerank_dev(d["q_emb"], q_tok, q_len, 8, 4))              # no cross-encoder
        refused(ERR_STATE, lambda: e.retrieve_maxsim_dev(d["q_emb"], d["qv"], d["qo"], 8, 4))         # no token-vector store
        refused(ERR_STATE, lambda: _composite(e, 1, pool=8, k=4))                                     # no sparse index
        e.tokvec_load(*F.vecs_of_rows(np.arange(10)))                                                 # 10 documents beside 64 rows
        refused(ERR_STATE, lambda: e.retrieve_maxsim_dev(d["q_emb"], d["qv"], d["qo"], 8, 4))
        refused(ERR_STATE, lambda: _composite(e, 0, weights=(0.4, 0.0, 0.4), pool=8, k=4))
        refused(ERR_ARG, lambda: e.retrieve_maxsim_dev(d["q_emb"], d["qv"], d["qo"], 257, 4))
        refused(ERR_ARG, lambda: _composite(e, 2, weights=(1.0, 0.0, 0.0), pool=129, k=4))
    finally:
        e.close()


# ---- 5. live writes -----------------------------------------------------------------------------------------------------------------
def test_live_writes_keep_the_three_way_score_current():
    from optimized_rag_amd import RagEngine
    w, a = F.world(), F.corpus_a()
    n0 = N_A - 40
    a_, b = RagEngine(dim=F.DIM, device=0), RagEngine(dim=F.DIM, device=0)
    try:
        a_.set_option("sparse_tail_fold", -1)
        _load(a_, np.arange(n0), headroom=40)
        new = np.arange(n0, N_A)
        a_.index_insert(np.array(w["emb"][new]), ids=np.array(w["ids"][new]), tenants=np.array(w["tenants"][new]))
        term_of = np.repeat(np.arange(F.V_A, dtype=np.int64), np.diff(a["indptr"]))
        sel = a["doc"] >= n0
        indptr = np.zeros(F.V_A + 1, dtype=np.int64)
        np.cumsum(np.bincount(term_of[sel], minlength=F.V_A), out=indptr[1:])
        a_.sparse_append(indptr, (a["doc"][sel] - n0).astype(np.int32), np.ascontiguousarray(a["w"][sel]), 40)
        a_.tokvec_append(*F.vecs_of_rows(new))

        def check(keep, what):
            _load(b, keep)
            for tenant in (-1, 2):
                got, exp = _composite(a_, 2, tenant=tenant), T.to_np(_composite(b, 2, tenant=tenant))
                _same(got, exp, f"{what}, tenant {tenant}")
            return T.to_np(got)[0]

        check(np.arange(N_A), "after the inserts and the appends")
        best = T.to_np(_composite(a_, 2))[0][:, :2]
        dead_ids = np.unique(best[best >= 0])[:25]
        assert dead_ids.shape[0] == 25 and a_.index_delete(dead_ids) == 25
        live = np.setdiff1d(np.arange(N_A), (dead_ids - 5000) // 3)
        ids = check(live, "after the deletes")
        assert not np.isin(ids, dead_ids).any()
        rm = a_.index_compact(keep_resident=True)
        assert (rm >= 0).sum() == live.shape[0] and a_.tokvec_info()["n_docs"] == live.shape[0]
        check(live, "after rag_index_compact_live")
    finally:
        a_.close()
        b.close()


# ---- 6. stream order ----------------------------------------------------------------------------------------------------------------
def test_retrieve_m3_dev_is_ordered_on_its_stream(full):
    import torch
    call = lambda d, s: _composite(full, 2, stream=s, dev=d)
    real = _dev_inputs()
    wrong = {k: np.zeros_like(v) for k, v in real.items()}               # legal: queries without terms or token vectors
    wrong["q_emb"] = np.ones_like(real["q_emb"])
    ref = T.serial(call, wrong, real)
    assert (ref[0][:, 0] >= 0).sum() >= 30
    got, pending = T.late_producer(call, wrong, real, torch.cuda.Stream())
    assert pending, "rag_retrieve_m3_dev waited for the work queued before it on its stream"
    T.assert_same(got, ref, "three-way composite behind a late producer")


# ---- 7. the service -----------------------------------------------------------------------------------------------------------------
def test_search_m3_on_a_seeded_checkpoint(tmp_path):
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.document_store import GpuDocumentIndex
    from optimized_rag_amd.embeddings import LocalEmbeddingService
    from optimized_rag_amd.sparse import LexicalPostings
    words = [f"w{i}" for i in range(60)]
    hf = X.xlmr_hf_config(vocab_size=64, hidden=128, layers=2, heads=4, ffn=256)
    sd = X.seeded_xlmr(hf, 9, head=False)
    heads = M.seeded_heads(128, 96, 4)
    d = tmp_path / "m3"
    X.write_checkpoint(d, hf, sd, words=words)
    (d / "1_Pooling").mkdir()
    (d / "1_Pooling" / "config.json").write_text(json.dumps(dict(pooling_mode_cls_token=True, pooling_mode_mean_tokens=False)))
    M.write_head_files(d, heads)
    cfg = dict(vocab_size=64, hidden=128, layers=2, heads=4, ffn=256, max_pos=64, type_vocab=1, eps=1e-5)
    w = X.xlmr_to_bert_names(sd, head=False)
    rng = np.random.default_rng(12)
    query = " ".join(rng.choice(words[:20], 6))
    texts = [" ".join(rng.choice(words[:30], int(rng.integers(2, 40)))) for _ in range(40)]
    agents = ["a" if i % 4 else "b" for i in range(40)]
    enc = X.roberta_tokenizer(words).encode_batch([query] + texts)
    pl = np.array([len(x.ids) for x in enc], dtype=np.int32)
    pi = np.zeros((len(enc), int(pl.max())), dtype=np.int32)
    for i, x in enumerate(enc):
        pi[i, :pl[i]] = x.ids
    ref = M.heads_reference(w, cfg, pi, np.zeros_like(pi), pl, heads)
    e = RagEngine(dim=128, device=0)
    try:
        svc = LocalEmbeddingService.from_dir(str(d), engine=e, max_length=64)
        exp = M.score_pairs(ref, pi, pl, [0] * 40, list(range(1, 41)), svc.special_ids())
        index = GpuDocumentIndex(svc, dim=128, engine=e)
        rows = [dict(content=t, agent_id=a, filename=f"f{i}", metadata=dict(i=i)) for i, (t, a) in enumerate(zip(texts, agents))]
        index.bulk_load(rows, np.asarray(svc.generate_embeddings_batch(texts), dtype=np.float32))
        plain = index.search("a", query, top_k=5, with_embeddings=False)
        assert len(plain) == 5 and index.search_m3("a", query, top_k=5) == plain        # no resident legs yet: answered with `search`
        index.load_lexical(LexicalPostings.from_texts(svc, texts))
        assert index.search_m3("a", query, top_k=5) == plain                            # no token vectors yet
        index.build_token_vectors(texts, batch=16)
        row_of = {t["filename"]: i for i, t in enumerate(rows)}
        keys = {"content", "filename", "file_type", "score", "dense_score", "sparse_score", "colbert_score", "metadata"}
        for agent, top_k, cands in (("a", 5, "union"), ("b", 3, "dense"), ("a", 4, "dense+sparse")):
            res = index.search_m3(agent, query, top_k=top_k, pool=40, candidates=cands)
            assert len(res) == top_k and all(set(r) == keys for r in res)
            got = [row_of[r["filename"]] for r in res]
            assert all(agents[i] == agent for i in got)
            sc = np.array([r["score"] for r in res])
            for key, name in (("dense_score", "dense"), ("sparse_score", "sparse"), ("colbert_score", "colbert"), ("score", "colbert+sparse+dense")):
                err = float(np.abs(np.array([r[key] for r in res]) - exp[name][got]).max())
                print(f"search_m3 {cands}: max |{key} - reference| = {err:.3e}")
            assert err < 1e-3, err                                       # the score; the components are printed
            assert (np.diff(sc) <= 0).all()
            # every row of the agent is a candidate at this pool: nothing better was left out
            rest = [i for i in range(40) if agents[i] == agent and i not in got]
            assert exp["colbert+sparse+dense"][rest].max() <= sc.min() + 1e-3
        two = index.search_m3("a", query, top_k=5, pool=40, weights=(0.4, 0.2, 0.0))
        got = [row_of[r["filename"]] for r in two]
        assert all(r["colbert_score"] == 0.0 for r in two)
        assert np.abs(np.array([r["score"] for r in two]) - exp["sparse+dense"][got]).max() < 1e-3
        assert index.search_m3("nobody", query, top_k=5) == []
        assert index.search_m3("a", query, top_k=5, candidates="bm25") == plain
        assert index.search_m3("a", query, top_k=5, weights=(0.0, 0.0, 0.0)) == plain
        e.tokvec_reserve(1, 0, 96)                                       # the store dropped: what `search` answers
        assert index.search_m3("a", query, top_k=5, pool=40) == plain
    finally:
        e.close()
