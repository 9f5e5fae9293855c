"""GPU: the learned-sparse postings through live writes - rag_sparse_append_host / rag_sparse_fold / rag_sparse_segment_stats and
rag_index_compact_live. Every comparison is bit for bit against a FRESH handle that holds the same rows and was loaded by
rag_sparse_load_host with the merged (or compacted) CSR, and, after a compaction, against what the handle itself returned
immediately before the call with its rows mapped through the row map. The all-document scores are also held to the float64
numpy reference of tests/sparse_tools.py. No tolerance anywhere."""
import numpy as np
import pytest

import sparse_tools as S

pytestmark = pytest.mark.gpu

N0, BLOCKS, DIM = 3000, (1, 700, 2100), 32       # a base that ends inside a 2048-document range; the tail starts inside that
N_ALL = N0 + sum(BLOCKS)                         # range, grows past a range boundary and ends on a partial range
V0, V = 3500, 4000                               # the base's vocabulary and the vocabulary after the second block
T_TAIL, T_NEW = 3200, 3600                       # a known term that occurs only in appended rows / a term past the base's vocabulary
NO_FOLD = (("sparse_tail_fold", -1),)
_W = {}


def coo_of(indptr, doc, w):
    return np.repeat(np.arange(indptr.shape[0] - 1, dtype=np.int64), np.diff(indptr)), doc.astype(np.int64), w


def csr_of(term, doc, w, n_terms, n_docs):
    """term-major CSR of COO postings (any order in, documents ascending per term out)"""
    order = np.argsort(term * max(n_docs, 1) + doc, kind="stable")
    indptr = np.zeros(n_terms + 1, dtype=np.int64)
    np.cumsum(np.bincount(term, minlength=n_terms), out=indptr[1:])
    return indptr, doc[order].astype(np.int32), np.ascontiguousarray(w[order], dtype=np.float32)


def make_world(weight_values=None):
    rng = np.random.default_rng(3)
    ip, doc, w = S.make_corpus(N_ALL, V, seed=7, weight_values=weight_values)
    term, doc, w = coo_of(ip, doc, w)
    # two terms without a posting in the base: one inside its vocabulary, one past it (both only in rows >= N0 + 1)
    xt = np.array([T_TAIL] * 4 + [T_NEW] * 3, dtype=np.int64)
    xd = np.array([N0 + 5, N0 + 300, N0 + 900, N_ALL - 1, N0 + 5, N0 + 2000, N_ALL - 2], dtype=np.int64)
    xw = (np.array([0.5, 1.25, 0.75, 2.0, 1.5, 0.25, 1.0], dtype=np.float32) if weight_values is None
          else rng.choice(np.asarray(weight_values, dtype=np.float32), 7))
    term, doc, w = np.concatenate([term, xt]), np.concatenate([doc, xd]), np.concatenate([w, xw]).astype(np.float32)
    full = csr_of(term, doc, w, V, N_ALL)
    qs = S.make_queries(full[0], weight_values=weight_values)
    by_df = np.argsort(-np.diff(full[0]), kind="stable")
    one = np.float32(1.0)
    qs += [(np.array([T_TAIL]), np.array([one])), (np.array([T_NEW]), np.array([0.5], np.float32)),
           (np.array([T_TAIL, int(by_df[3]), T_TAIL, T_NEW]), np.array([1.0, 0.5, 0.25, 1.0], np.float32)),
           (by_df[[0]], np.array([one])), (by_df[[40]], np.array([one])), (by_df[[200]], np.array([one]))]
    emb = rng.standard_normal((N_ALL, DIM)).astype(np.float32)
    out = dict(coo=(term, doc, w), full=full, qs=qs, packed=S.pack_queries(qs), emb=emb,
               q=(emb[rng.integers(0, N_ALL, len(qs))] + 0.3 * rng.standard_normal((len(qs), DIM))).astype(np.float32),
               ids=(rng.permutation(N_ALL) + 1_000_000).astype(np.int64), ten=rng.integers(0, 3, N_ALL).astype(np.int32))
    for v in out.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


def world():
    if not _W:
        _W.update(make_world())
    return _W


def postings_of(w, orig, n_terms):
    """CSR of the original documents `orig` (ascending), renumbered 0 .. len(orig) - 1, over n_terms terms"""
    term, doc, wt = w["coo"]
    inv = np.full(N_ALL, -1, dtype=np.int64)
    inv[orig] = np.arange(len(orig))
    keep = (inv[doc] >= 0) & (term < n_terms)
    return csr_of(term[keep], inv[doc[keep]], wt[keep], n_terms, len(orig))


class Live:
    """A handle with a dense index (explicit ids, tenants) and sparse postings over the first rows of the world; `orig` = the
    world's document behind each current row, `covered` = rows the postings cover."""

    def __init__(self, w, n0=N0, n_terms=V0, opts=NO_FOLD, bm25=False):
        from optimized_rag_amd import RagEngine
        self.w, self.e = w, RagEngine(dim=DIM, device=0)
        for name, v in opts:
            self.e.set_option(name, v)
        self.orig = np.arange(n0)
        self.e.index_load(np.array(w["emb"][:n0]), ids=np.array(w["ids"][:n0]))
        self.e.set_tenants(np.array(w["ten"][:n0]))
        self.e.sparse_load(*postings_of(w, self.orig, n_terms), n0)
        self.covered, self.n_terms, self.next = n0, n_terms, n0
        if bm25:
            self.e.bm25_load(*bm25_of(postings_of(w, self.orig, n_terms), self.orig))

    def close(self):
        self.e.close()

    def insert(self, n):
        d = np.arange(self.next, self.next + n)
        self.e.index_insert(np.array(self.w["emb"][d]), ids=np.array(self.w["ids"][d]), tenants=np.array(self.w["ten"][d]))
        self.orig = np.concatenate([self.orig, d])
        self.next += n

    def block(self, n, n_terms):
        return postings_of(self.w, self.orig[self.covered:self.covered + n], n_terms)

    def append(self, n, n_terms=None):
        self.n_terms = max(self.n_terms, n_terms or 0)
        self.e.sparse_append(*self.block(n, self.n_terms), n)
        self.covered += n

    def delete(self, rows):
        assert self.e.index_delete(np.array(self.w["ids"][self.orig[np.asarray(rows)]])) == len(rows)

    def compact(self, **kw):
        rm = self.e.index_compact(**(kw or dict(keep_resident=True)))
        live = rm >= 0
        self.covered = int(live[:self.covered].sum())
        self.orig = self.orig[live]
        return rm

    def fresh(self):
        """a fresh handle with the same rows and the CSR of the covered (= all) rows"""
        from optimized_rag_amd import RagEngine
        assert self.covered == len(self.orig)
        e = RagEngine(dim=DIM, device=0)
        e.index_load(np.array(self.w["emb"][self.orig]), ids=np.array(self.w["ids"][self.orig]))
        e.set_tenants(np.array(self.w["ten"][self.orig]))
        e.sparse_load(*postings_of(self.w, self.orig, self.n_terms), len(self.orig))
        return e


def bm25_of(post, orig):
    """BM25 arrays over the same postings: seeded term frequencies, lengths and idf values"""
    rng = np.random.default_rng(17)
    ip, doc, _ = post
    idf = rng.random(ip.shape[0] - 1) * 4.0 + 0.1
    dl = rng.integers(20, 200, len(orig)).astype(np.int32)
    return ip, doc, rng.integers(1, 6, doc.shape[0]).astype(np.int32), dl, idf, float(dl.mean())


def results(e, w, hybrid=True, ks=(1, 20, 100)):
    """everything the contract names, as host arrays"""
    import torch
    out = {}
    for k in ks:
        for tenant in (-1, 1):
            out[f"topk k={k} tenant={tenant}"] = e.sparse_topk(*w["packed"], k, tenant=tenant)
    out["scores"] = (e.sparse_scores(*w["packed"]),)
    e.set_option("bm25_plan_slots", 8)               # the 70-term query's tokens past the plan: weighted inside the scoring kernel
    out["topk slots=8"] = e.sparse_topk(*w["packed"], 20)
    out["scores slots=8"] = (e.sparse_scores(*w["packed"]),)
    e.set_option("bm25_plan_slots", 0)
    if hybrid:
        ptr, terms, wts = (torch.from_numpy(np.array(a)).cuda() for a in w["packed"])
        q = torch.from_numpy(np.array(w["q"])).cuda()
        keys, rrf, ranks = e.hybrid_sparse_rrf_dev(q, ptr, terms, wts, 100, 20)
        torch.cuda.synchronize()
        out["hybrid"] = (keys.cpu().numpy(), rrf.cpu().numpy(), ranks.cpu().numpy())
        ids = torch.full((len(w["qs"]), 20), -7, dtype=torch.int64, device="cuda")
        rows = torch.full((len(w["qs"]), 20), -7, dtype=torch.int32, device="cuda")
        sc = torch.full((len(w["qs"]), 20), -7.0, dtype=torch.float64, device="cuda")
        e.sparse_topk_dev(ptr, terms, wts, 20, ids, rows, sc, tenant=2)
        torch.cuda.synchronize()
        out["topk dev tenant=2"] = (ids.cpu().numpy(), rows.cpu().numpy(), sc.cpu().numpy())
    return out


def same(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        for x, y in zip(a[name], b[name]):
            x, y = np.asarray(x), np.asarray(y)
            assert x.shape == y.shape and x.dtype == y.dtype, f"{what}: {name}"
            np.testing.assert_array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y,
                                          err_msg=f"{what}: {name}")


def check_fresh(st, what, numpy_ref=True):
    f = st.fresh()
    try:
        got = results(st.e, st.w)
        same(got, results(f, st.w), what)
    finally:
        f.close()
    if numpy_ref:
        ip, doc, wt = postings_of(st.w, st.orig, st.n_terms)
        np.testing.assert_array_equal(S.bits(got["scores"][0]), S.bits(S.all_scores(ip, doc, wt, len(st.orig), st.w["qs"])), err_msg=what)
    return got


def mapped(before, rm):
    """results from before a compaction with their rows sent through the row map (scores, ids and hybrid keys do not move)"""
    out = {}
    live = rm >= 0
    for name, v in before.items():
        if name.startswith("topk"):
            ids, rows, sc = v
            assert (rm[rows[rows >= 0]] >= 0).all(), "a deleted row was returned before the compaction"
            out[name] = (ids, np.where(rows >= 0, rm[np.maximum(rows, 0)], -1).astype(np.int32), sc)
        elif name.startswith("scores"):
            out[name] = (np.ascontiguousarray(v[0][:, live]),)
        else:
            out[name] = v
    return out


# ---- appends ----------------------------------------------------------------------------------------------------------
def test_appends_of_1_700_and_2100_rows_equal_a_fresh_load():
    w = world()
    st = Live(w)
    try:
        for n, vt in zip(BLOCKS, (V0, V, V)):
            st.insert(n)
            st.append(n, vt)
            got = check_fresh(st, f"after the block of {n}")
            s = st.e.sparse_segment_stats()
            assert (s["base_docs"], s["tail_docs"], s["n_terms"], s["folds"]) == (N0, st.covered - N0, vt, 0)
            info = st.e.sparse_info()
            assert (info["n_docs"], info["n_terms"], info["nnz"]) == (st.covered, vt, s["base_nnz"] + s["tail_nnz"])
        assert s["appends"] == 3 and s["tail_bytes"] > 8 * s["tail_nnz"]
        qi = len(w["qs"]) - 6                            # the term that exists only in the tail, the new term, both with a repeat
        sc = got["scores"][0]
        assert (sc[qi] > 0).sum() == 4 and (sc[qi, :N0] == 0).all() and (sc[qi + 1] > 0).sum() == 3
        assert N0 + 5 in got["topk k=20 tenant=-1"][1][qi + 2]         # the document that holds both terms (the repeated one adds twice)
    finally:
        st.close()


def test_ties_across_the_boundary_go_to_the_lower_row():
    w = make_world(weight_values=[0.25, 0.5, 1.0])
    st = Live(w, n_terms=V)
    try:
        st.insert(N_ALL - N0)
        st.append(N_ALL - N0, V)
        got = check_fresh(st, "tie corpus")
        ref = S.all_scores(*w["full"], N_ALL, w["qs"])
        crossed = 0
        for k in (20, 100):
            rr, rs = S.topk_all(ref, k)
            np.testing.assert_array_equal(got[f"topk k={k} tenant=-1"][1], rr)
            np.testing.assert_array_equal(S.bits(got[f"topk k={k} tenant=-1"][2]), S.bits(rs))
            for q in range(len(w["qs"])):
                tie = np.nonzero((ref[q] == rs[q, k - 1]) & (rs[q, k - 1] > 0))[0]
                crossed += bool(tie.size and tie[0] < N0 <= tie[-1] and (ref[q] >= rs[q, k - 1]).sum() > k)
        assert crossed >= 4                              # plateaus that the k-th place cuts and that lie on both sides of the boundary
    finally:
        st.close()


# ---- staleness and rejected blocks ----------------------------------------------------------------------------------------
def test_postings_stay_stale_until_every_inserted_row_is_covered():
    from optimized_rag_amd._lib import RagError
    w = world()
    st = Live(w)
    try:
        st.insert(5)
        with pytest.raises(RagError, match=r"\(-3\).*stale"):
            st.e.sparse_topk(*w["packed"], 5)
        st.append(3)
        with pytest.raises(RagError, match=r"\(-3\).*stale"):
            st.e.sparse_topk(*w["packed"], 5)
        with pytest.raises(RagError, match=r"\(-3\).*stale"):
            results(st.e, w, ks=())
        ip, doc, wt = st.block(2, V0)
        assert doc.shape[0] > 8
        s0, info0 = st.e.sparse_segment_stats(), st.e.sparse_info()
        top = int(np.argmax(np.diff(ip)))
        a = int(ip[top])
        bad_doc, bad_zero, bad_nan = doc.copy(), wt.copy(), wt.copy()
        if ip[top + 1] - a >= 2:
            bad_doc[a], bad_doc[a + 1] = doc[a + 1], doc[a]          # descending documents inside a term
        else:
            bad_doc[a] = 2                                           # a document past the block
        bad_zero[3], bad_nan[5] = 0.0, np.nan
        for args, n in (((ip, bad_doc, wt), 2), ((ip, doc, bad_zero), 2), ((ip, doc, bad_nan), 2),
                        ((st.block(2, V0)[0], doc, wt), 3),          # one row more than the index has
                        ((ip[:-1], doc[:int(ip[-2])], wt[:int(ip[-2])]), 2)):      # a vocabulary that shrinks
            with pytest.raises(RagError, match=r"\(-1\)"):
                st.e.sparse_append(*args, n)
            assert st.e.sparse_segment_stats() == s0 and st.e.sparse_info() == info0
            with pytest.raises(RagError, match=r"\(-3\).*stale"):
                st.e.sparse_topk(*w["packed"], 5)
        st.append(2)                                                 # the corrected block
        check_fresh(st, "5 inserted, 3 + 2 appended")
    finally:
        st.close()


def test_append_without_postings_is_a_state_error():
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd._lib import RagError
    e = RagEngine(dim=DIM, device=0)
    try:
        for call in (lambda: e.sparse_append(np.zeros(2, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), 1),
                     e.sparse_fold, e.sparse_segment_stats):
            with pytest.raises(RagError, match=r"\(-3\)"):
                call()
    finally:
        e.close()


# ---- fold -----------------------------------------------------------------------------------------------------------------
def test_fold_and_the_automatic_fold_change_no_bit():
    w = world()
    st = Live(w)
    try:
        st.insert(701)
        st.append(1)
        st.append(700, V)
        before = results(st.e, w)
        s0 = st.e.sparse_segment_stats()
        st.e.sparse_fold()
        s1 = st.e.sparse_segment_stats()
        assert (s1["base_docs"], s1["tail_docs"], s1["tail_nnz"], s1["tail_bytes"], s1["folds"]) == (N0 + 701, 0, 0, 0, 1)
        assert s1["base_nnz"] == s0["base_nnz"] + s0["tail_nnz"] and s1["appends"] == 2 and s1["n_terms"] == V
        same(before, results(st.e, w), "fold")
        st.e.sparse_fold()                                           # nothing to fold
        assert st.e.sparse_segment_stats() == s1
        st.e.set_option("sparse_tail_fold", 50)                      # an append folds once the tail holds more than 50 documents
        st.insert(2100)
        st.append(40)
        assert st.e.sparse_segment_stats()["tail_docs"] == 40
        st.append(2060)
        s2 = st.e.sparse_segment_stats()
        assert (s2["base_docs"], s2["tail_docs"], s2["folds"]) == (N_ALL, 0, 2)
        check_fresh(st, "automatic fold")
    finally:
        st.close()


# ---- rag_index_compact_live -------------------------------------------------------------------------------------------------
def grown(w, **kw):
    """base of 3,000 rows + a tail of 801"""
    st = Live(w, **kw)
    st.insert(801)
    st.append(1)
    st.append(800, V)
    return st


def rows_of_term(st, t):
    ip, doc, _ = postings_of(st.w, st.orig, st.n_terms)
    return doc[ip[t]:ip[t + 1]].astype(np.int64)


SCENARIOS = {
    "base only": lambda st: np.r_[0, 7, 100:140, 2047, 2048, 2999],
    "tail only": lambda st: np.r_[3000, 3001, 3100:3200, 3800],
    "both": lambda st: np.r_[0:3:2, 500:1500:7, 2990:3010, 3500:3700:3, 3800],
    "the whole tail": lambda st: np.arange(3000, 3801),
    "the whole base": lambda st: np.arange(0, 3000),
    "a term loses every posting": lambda st: np.union1d(rows_of_term(st, T_TAIL), rows_of_term(st, T_NEW)),
}


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_compact_live_keeps_the_sparse_postings(name):
    w = world()
    st = grown(w)
    try:
        rows = SCENARIOS[name](st)
        st.delete(rows)
        before = results(st.e, w)
        appends = st.e.sparse_segment_stats()["appends"]
        rm = st.compact()
        assert (rm < 0).sum() == len(rows) and st.e.n_rows == 3801 - len(rows)
        got = check_fresh(st, name)
        same(mapped(before, rm), got, name + ": before the call, through the row map")
        s = st.e.sparse_segment_stats()
        base_live, tail_live = int((rm[:3000] >= 0).sum()), int((rm[3000:] >= 0).sum())
        want = (base_live, tail_live) if base_live and tail_live else (base_live + tail_live, 0)
        assert (s["base_docs"], s["tail_docs"]) == want and s["appends"] == appends and s["folds"] == 0
        assert s["base_nnz"] + s["tail_nnz"] == postings_of(w, st.orig, st.n_terms)[1].shape[0]
        if name == "a term loses every posting":
            assert (got["scores"][0][len(w["qs"]) - 6] == 0).all() and st.e.sparse_info()["n_terms"] == V
        st.e.sparse_fold()
        same(got, results(st.e, w), name + ": folded afterwards")
    finally:
        st.close()


def test_compact_live_beside_bm25_postings_equals_compact_bm25():
    w = world()
    a, b = Live(w, bm25=True), Live(w, bm25=True)
    try:
        rows = np.r_[3:900:5, 2040:2060]
        for st in (a, b):
            st.delete(rows)
        ra, rb = a.compact(keep_resident=True), b.compact(keep_postings=True)
        np.testing.assert_array_equal(ra, rb)
        ptr, terms, _ = w["packed"]
        for k in (1, 20, 100):
            for x, y in zip(a.e.bm25_topk(ptr, terms, k), b.e.bm25_topk(ptr, terms, k)):
                np.testing.assert_array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y)
        assert a.e.bm25_segment_stats() == b.e.bm25_segment_stats()
        check_fresh(a, "beside BM25 postings")
        from optimized_rag_amd._lib import RagError
        with pytest.raises(RagError, match=r"\(-3\).*stale"):        # rag_index_compact_bm25 leaves the sparse postings stale, as before
            b.e.sparse_topk(*w["packed"], 5)
    finally:
        a.close()
        b.close()


def test_every_covered_row_deleted_ends_as_a_plain_compaction():
    from optimized_rag_amd._lib import RagError
    w = world()
    st = Live(w, n0=300)
    try:
        st.insert(4)                                                 # four rows the postings do not cover survive
        st.delete(np.arange(300))
        rm = st.compact()
        assert (rm[:300] == -1).all() and st.e.n_rows == 4
        with pytest.raises(RagError, match=r"\(-3\).*stale"):
            st.e.sparse_topk(*w["packed"], 5)
        st.covered = 0
        with pytest.raises(RagError):                                # nothing an append could align: only a reload helps
            st.append(4)
            st.e.sparse_topk(*w["packed"], 5)
        st.e.sparse_load(*postings_of(w, st.orig, V0), 4)
        st.covered = 4
        check_fresh(st, "reloaded")
    finally:
        st.close()


def test_nothing_deleted_moves_and_marks_nothing():
    w = world()
    st = grown(w)
    try:
        before, s0, i0 = results(st.e, w), st.e.sparse_segment_stats(), st.e.sparse_info()
        rm = st.compact()
        np.testing.assert_array_equal(rm, np.arange(3801))
        assert st.e.sparse_segment_stats() == s0 and st.e.sparse_info() == i0
        same(before, results(st.e, w), "nothing deleted")
    finally:
        st.close()


def test_rows_inserted_but_not_appended_are_appended_in_their_new_order():
    from optimized_rag_amd._lib import RagError
    w = world()
    st = grown(w)
    try:
        st.insert(200)                                               # rows 3801 .. 4000: not covered
        st.delete(np.r_[10:20, 3000:3050, 3900:3950])
        rm = st.compact()
        assert st.covered == 3801 - 60 and len(st.orig) == 4001 - 110
        with pytest.raises(RagError, match=r"\(-3\).*stale"):
            st.e.sparse_topk(*w["packed"], 5)
        st.append(100)
        with pytest.raises(RagError, match=r"\(-3\).*stale"):
            st.e.sparse_topk(*w["packed"], 5)
        st.append(50)
        check_fresh(st, "the remaining rows appended after the compaction")
    finally:
        st.close()


def test_after_a_plain_compaction_only_a_reload_helps():
    from optimized_rag_amd._lib import RagError
    w = world()
    st = grown(w)
    try:
        st.delete(np.r_[5:9])
        st.compact(keep_resident=False)
        s0 = st.e.sparse_segment_stats()
        st.delete(np.r_[100:110])
        st.compact()                                                 # behaves as rag_index_compact for the postings
        assert st.e.sparse_segment_stats() == s0
        with pytest.raises(RagError, match=r"\(-3\).*stale"):
            st.e.sparse_topk(*w["packed"], 5)
        st.e.sparse_load(*postings_of(w, st.orig, V), len(st.orig))
        st.covered = len(st.orig)
        check_fresh(st, "reloaded after a plain compaction")
    finally:
        st.close()
