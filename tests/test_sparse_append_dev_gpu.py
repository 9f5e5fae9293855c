"""GPU: learned-sparse postings appended from DOC-MAJOR blocks - rag_sparse_append_dev, rag_sparse_append_docs_host,
rag_sparse_clear and rag_sparse_export_host. Every comparison is bit for bit: against a second handle fed the same blocks,
transposed by the numpy mirror of tests/sparse_docs_tools.py, through rag_sparse_append_host; against a fresh handle loaded with
the merged CSR; and, for a rejected block, against the handle's own state before the call. No tolerance anywhere."""
import numpy as np
import pytest

import sparse_docs_tools as D
import sparse_tools as S

pytestmark = pytest.mark.gpu

NO_FOLD = (("sparse_tail_fold", -1),)
ROUTES = ("dev", "docs_host", "host")


def bits(a):
    a = np.asarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b, what):
    assert a.keys() == b.keys(), what
    for name in a:
        assert len(a[name]) == len(b[name])
        for x, y in zip(a[name], b[name]):
            x, y = np.asarray(x), np.asarray(y)
            assert x.shape == y.shape and x.dtype == y.dtype, f"{what}: {name}"
            np.testing.assert_array_equal(bits(x), bits(y), err_msg=f"{what}: {name}")


def append_block(e, route, block, n_terms):
    """one doc-major block (ptr, terms, weights) through the route under test; "host": its mirror transpose through _append_host"""
    import torch
    ptr, terms, w = block
    n = ptr.shape[0] - 1
    if route == "dev":
        cap = terms.shape[0] + 5                                     # a capacity past the block's postings, as the compaction leaves it
        t = torch.full((cap,), -9, dtype=torch.int32, device="cuda")
        x = torch.full((cap,), float("nan"), dtype=torch.float32, device="cuda")
        t[:terms.shape[0]] = torch.from_numpy(np.array(terms))
        x[:terms.shape[0]] = torch.from_numpy(np.array(w))
        e.sparse_append_dev(torch.from_numpy(np.array(ptr)).cuda(), t, x, n_terms)
    elif route == "docs_host":
        e.sparse_append_docs(ptr, terms, w, n_terms)
    else:
        e.sparse_append(*D.transpose(ptr, terms, w, n_terms), n, n_terms)


def results(e, w, hybrid=True, ks=(1, 20, 100)):
    """everything the contract names, as host arrays"""
    import torch
    out = {}
    for k in ks:
        for tenant in ((-1, 1) if hybrid else (-1,)):
            out[f"topk k={k} tenant={tenant}"] = e.sparse_topk(*w["packed"], k, tenant=tenant)
    out["scores"] = (e.sparse_scores(*w["packed"]),)
    out["score rows"] = (e.sparse_score_rows(*w["packed"], np.array(w["cand"])),)
    x = e.sparse_export()
    out["export"] = (x["indptr"], x["doc"], x["weight"], np.int64(x["n_docs"]))
    s = e.sparse_segment_stats()
    out["stats"] = (np.array([s[k] for k in sorted(s)], dtype=np.int64),)
    if hybrid:
        ptr, terms, wts = (torch.from_numpy(np.array(a)).cuda() for a in w["packed"])
        keys, rrf, ranks = e.hybrid_sparse_rrf_dev(torch.from_numpy(np.array(w["q"])).cuda(), ptr, terms, wts, 100, 20)
        torch.cuda.synchronize()
        out["hybrid"] = (keys.cpu().numpy(), rrf.cpu().numpy(), ranks.cpu().numpy())
    return out


class Live:
    """A handle with a dense index (explicit ids, tenants) and sparse postings over the first rows of the world, written through
    one route; `orig` = the world's document behind each current row, `covered` = rows the postings cover."""

    def __init__(self, w, route, n0=D.N0, n_terms=D.V0, opts=NO_FOLD, index=True):
        from optimized_rag_amd import RagEngine
        self.w, self.route, self.e, self.index = w, route, RagEngine(dim=D.DIM, device=0), index
        for name, v in opts:
            self.e.set_option(name, v)
        self.orig = np.arange(n0)
        if index:
            self.e.index_load(np.array(w["emb"][:n0]), ids=np.array(w["ids"][:n0]))
            self.e.set_tenants(np.array(w["ten"][:n0]))
        self.e.sparse_load(*D.postings_of(w, self.orig, n_terms), n0)
        self.covered, self.n_terms, self.next = n0, n_terms, n0

    def close(self):
        self.e.close()

    def insert(self, n):
        d = np.arange(self.next, self.next + n)
        if self.index:
            self.e.index_insert(np.array(self.w["emb"][d]), ids=np.array(self.w["ids"][d]), tenants=np.array(self.w["ten"][d]))
        self.orig = np.concatenate([self.orig, d])
        self.next += n

    def block(self, n, n_terms):
        return D.doc_major_of_csr(*D.postings_of(self.w, self.orig[self.covered:self.covered + n], n_terms), n)

    def append(self, n, n_terms=None):
        self.n_terms = max(self.n_terms, n_terms or 0)
        append_block(self.e, self.route, self.block(n, self.n_terms), self.n_terms)
        self.covered += n

    def fresh(self):
        from optimized_rag_amd import RagEngine
        assert self.covered == len(self.orig)
        e = RagEngine(dim=D.DIM, device=0)
        if self.index:
            e.index_load(np.array(self.w["emb"][self.orig]), ids=np.array(self.w["ids"][self.orig]))
            e.set_tenants(np.array(self.w["ten"][self.orig]))
        e.sparse_load(*D.postings_of(self.w, self.orig, self.n_terms), len(self.orig))
        return e


def without_stats(r):
    return {k: v for k, v in r.items() if k != "stats"}


def check_fresh(st, got, what):
    """a fresh handle with the merged CSR gives the same bits (its segments differ: one base, no tail), and the export IS that CSR"""
    f = st.fresh()
    try:
        same(without_stats(got), without_stats(results(f, st.w, hybrid=st.index)), what + ": against a fresh load")
    finally:
        f.close()
    ip, doc, wt = D.postings_of(st.w, st.orig, st.n_terms)
    same({"export": got["export"]}, {"export": (ip, doc, wt, np.int64(len(st.orig)))}, what + ": the export against numpy")


# ---- appends --------------------------------------------------------------------------------------------------------------------
def test_appends_of_1_700_and_2100_rows_equal_the_host_append_and_a_fresh_load():
    w = D.world()
    sts = [Live(w, r) for r in ROUTES]
    try:
        for n, vt in zip(D.BLOCKS, (D.V0, D.V, D.V)):
            got = []
            for st in sts:
                st.insert(n)
                st.append(n, vt)
                got.append(results(st.e, w))
            for r, g in zip(ROUTES[:2], got[:2]):
                same(g, got[2], f"after the block of {n}: {r} against rag_sparse_append_host")
            check_fresh(sts[0], got[0], f"after the block of {n}")
            s = sts[0].e.sparse_segment_stats()
            assert (s["base_docs"], s["tail_docs"], s["n_terms"], s["folds"]) == (D.N0, sts[0].covered - D.N0, vt, 0)
        assert s["appends"] == 3
        sc = got[0]["scores"][0]
        qi = len(w["qs"]) - 3                            # the term only the tail holds, the new term, the digit-boundary terms
        assert (sc[qi] > 0).sum() == 4 and (sc[qi, :D.N0] == 0).all() and (sc[qi + 1] > 0).sum() == 3 and (sc[qi + 2, D.N0 + 701:] > 0).any()
        # ... the same again after a fold, and after a compaction that keeps the postings with a seeded 10 % deleted
        dead = np.nonzero(np.random.default_rng(41).random(D.N_ALL) < 0.10)[0]
        folded = []
        for st in sts:
            st.e.sparse_fold()
            folded.append(results(st.e, w))
        for r, g in zip(ROUTES[:2], folded[:2]):
            same(g, folded[2], f"folded: {r}")
        same(without_stats(folded[0]), without_stats(got[0]), "the fold changes no bit")
        compacted = []
        for st in sts:
            assert st.e.index_delete(np.array(w["ids"][dead])) == len(dead)
            rm = st.e.index_compact(keep_resident=True)
            st.orig = st.orig[rm >= 0]
            st.covered = len(st.orig)
            compacted.append(results(st.e, w))
        for r, g in zip(ROUTES[:2], compacted[:2]):
            same(g, compacted[2], f"compacted: {r}")
        check_fresh(sts[0], compacted[0], "compacted")
    finally:
        for st in sts:
            st.close()


def test_compaction_of_base_and_tail_after_device_appends():
    """the tail built on the device goes through rag_index_compact_live unfolded, as a host-built one does"""
    w = D.world()
    sts = [Live(w, r) for r in ("dev", "host")]
    try:
        dead = np.nonzero(np.random.default_rng(43).random(D.N0 + 701) < 0.10)[0]
        got = []
        for st in sts:
            st.insert(701)
            st.append(1)
            st.append(700, D.V)
            assert st.e.index_delete(np.array(w["ids"][dead])) == len(dead)
            rm = st.e.index_compact(keep_resident=True)
            st.orig = st.orig[rm >= 0]
            st.covered = len(st.orig)
            got.append(results(st.e, w))
        same(got[0], got[1], "compacted with a tail")
        assert got[0]["stats"][0].tolist() == got[1]["stats"][0].tolist() and sts[0].e.sparse_segment_stats()["tail_docs"] > 0
        check_fresh(sts[0], got[0], "compacted with a tail")
    finally:
        for st in sts:
            st.close()


# ---- edge blocks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(D.edge_blocks()))
def test_edge_blocks(name):
    from optimized_rag_amd import RagEngine
    w = D.world()
    ptr, terms, wt, vt = D.edge_blocks()[name]
    n = ptr.shape[0] - 1
    base = D.postings_of(w, np.arange(300), D.V_EDGE)                 # a small base: the block's rows follow it
    qs = [(np.array(D.DIGIT_TERMS + [77, 17]), np.ones(8, np.float32)), (np.array([vt - 1, 5, D.V_EDGE]), np.array([1.0, 0.5, 2.0], np.float32))]
    if terms.shape[0]:
        pick = np.unique(terms)[:: max(1, np.unique(terms).shape[0] // 40)]
        qs.append((pick, np.full(pick.shape[0], 0.75, np.float32)))
    world = dict(packed=S.pack_queries(qs), cand=np.array([[0, 299, 300, 300 + n - 1, 300 + n, -1]] * len(qs), dtype=np.int32))
    got = []
    for route in ROUTES:
        e = RagEngine(dim=D.DIM, device=0)
        try:
            e.set_option("sparse_tail_fold", -1)
            e.sparse_load(*base, 300)
            append_block(e, route, (ptr, terms, wt), vt)
            got.append(results(e, world, hybrid=False, ks=(1, 20)))
        finally:
            e.close()
    same(got[0], got[2], name + ": dev")
    same(got[1], got[2], name + ": docs_host")
    ip, doc, x, n_docs = got[0]["export"]
    assert n_docs == 300 + n and ip.shape[0] == vt + 1 and ip[-1] == base[0][-1] + terms.shape[0]
    if name == "one term in every document":
        np.testing.assert_array_equal(doc[ip[78] - n:ip[78]], np.arange(300, 300 + n))       # the long list, in document order
    if name == "a vocabulary of 250,002":
        assert got[0]["scores"][0][1, 300] > 0                        # the last term of the grown vocabulary is searchable


# ---- from nothing ---------------------------------------------------------------------------------------------------------------
def test_a_block_on_a_handle_without_postings_becomes_the_base():
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd._lib import RagError
    w = D.world()
    rows = np.arange(D.N0)
    block = D.doc_major_of_csr(*D.postings_of(w, rows, D.V0), D.N0)
    world = dict(w, cand=np.minimum(w["cand"], D.N0 - 1))
    ref = RagEngine(dim=D.DIM, device=0)
    e = RagEngine(dim=D.DIM, device=0)
    try:
        for h in (ref, e):
            h.index_load(np.array(w["emb"][:D.N0]), ids=np.array(w["ids"][:D.N0]))
            h.set_tenants(np.array(w["ten"][:D.N0]))
        ref.sparse_load(*D.postings_of(w, rows, D.V0), D.N0)
        want = results(ref, world)
        e.sparse_clear()                                              # nothing resident: OK
        with pytest.raises(RagError, match=r"\(-3\)"):
            e.sparse_export()
        for route in ("dev", "docs_host", "dev"):
            append_block(e, route, block, D.V0)
            same(results(e, world), want, f"the block as the base ({route})")
            assert e.sparse_segment_stats()["appends"] == 0
            e.sparse_clear()
            assert e.sparse_info()["n_docs"] == 0
            with pytest.raises(RagError, match=r"\(-3\)"):
                e.sparse_segment_stats()
        # a base from the device, then appends through the host route and the device route: one index either way
        append_block(e, "dev", D.doc_major_of_csr(*D.postings_of(w, rows[:1000], D.V0), 1000), D.V0)
        append_block(e, "host", D.doc_major_of_csr(*D.postings_of(w, rows[1000:2500], D.V0), 1500), D.V0)
        append_block(e, "dev", D.doc_major_of_csr(*D.postings_of(w, rows[2500:], D.V0), 500), D.V0)
        same(without_stats(results(e, world)), without_stats(want), "base and appends from the device")
    finally:
        ref.close()
        e.close()


# ---- rejections -----------------------------------------------------------------------------------------------------------------
def bad_blocks(block, V):
    """name -> (doc_ptr, terms, weights, n_terms_total, nnz_cap or None, message): each malformed in one way"""
    ptr, terms, w = block
    assert ptr.shape[0] == 3 and ptr[1] >= 3 and ptr[2] - ptr[1] >= 3
    a = int(ptr[1])
    out = {}
    p = ptr.copy(); p[0] = 1
    out["doc_ptr[0] != 0"] = (p, terms, w, V, None, "start at 0")
    p = ptr.copy(); p[1] = ptr[2] + 1
    out["a decreasing offset"] = (p, terms, w, V, None, "never decrease")
    # negative offsets: posting 0's owner then starts below 0, and the look-back at the previous term may not follow it there
    p = ptr.copy(); p[0] = -1
    out["doc_ptr[0] = -1"] = (p, terms, w, V, None, r"start at 0.*document 0\b")
    p = ptr.copy(); p[1] = -2
    out["a negative middle offset"] = (p, terms, w, V, None, r"never decrease.*document 0\b")
    p = ptr.copy(); p[0], p[1] = -5, -3
    out["two negative offsets"] = (p, terms, w, V, None, r"start at 0.*document 0\b")
    out["doc_ptr[n] > nnz_cap"] = (ptr, terms, w, V, int(ptr[2]) - 1, "nnz_cap")
    t = terms.copy(); t[a + 1] = V
    out["a term at n_terms_total"] = (ptr, t, w, V, None, r"term outside.*posting %d\b" % (a + 1))
    t = terms.copy(); t[0] = -1
    out["a negative term"] = (ptr, t, w, V, None, "term outside")
    t = terms.copy(); t[a + 1], t[a + 2] = terms[a + 2], terms[a + 1]
    out["descending terms"] = (ptr, t, w, V, None, "strictly ascending")
    t = terms.copy(); t[1] = terms[0]
    out["a repeated term"] = (ptr, t, w, V, None, r"strictly ascending.*posting 1\b")
    for name, v in (("a zero weight", 0.0), ("a negative weight", -1.0), ("a NaN weight", np.nan), ("an infinite weight", np.inf)):
        x = w.copy(); x[2] = v
        out[name] = (ptr, terms, x, V, None, r"finite and > 0.*posting 2\b")
    out["a shrinking vocabulary"] = (ptr, np.minimum(terms, V - 2), w, V - 1, None, "shrink")
    return out


def call_raw(e, route, ptr, terms, w, V, cap):
    import torch
    if route == "docs_host":
        from optimized_rag_amd._lib import _ptr
        ptr, terms, w = np.ascontiguousarray(ptr, np.int32), np.ascontiguousarray(terms, np.int32), np.ascontiguousarray(w, np.float32)
        e._check(e.lib.rag_sparse_append_docs_host(e.h, _ptr(ptr), _ptr(terms), _ptr(w), ptr.shape[0] - 1, terms.shape[0] if cap is None else cap,
                                                   V), "rag_sparse_append_docs_host")
    else:
        t, x = torch.from_numpy(np.array(terms)).cuda(), torch.from_numpy(np.array(w)).cuda()
        if cap is not None:
            t, x = t[:cap].contiguous(), x[:cap].contiguous()
        e.sparse_append_dev(torch.from_numpy(np.array(ptr)).cuda(), t, x, V)


def state(e):
    """what a rejected call may not change, readable on a stale handle too: the postings, the segments, the totals"""
    x, s, i = e.sparse_export(), e.sparse_segment_stats(), e.sparse_info()
    return dict(export=(x["indptr"], x["doc"], x["weight"], np.int64(x["n_docs"])), stats=(np.array([s[k] for k in sorted(s)], dtype=np.int64),),
                info=(np.array([i[k] for k in sorted(i)], dtype=np.int64),))


@pytest.mark.parametrize("route", ROUTES[:2])
def test_rejected_blocks_change_nothing(route):
    from optimized_rag_amd._lib import RagError
    w = D.world()
    st = Live(w, route)                                               # a dense index: 5 rows inserted, 3 appended - stale
    free = Live(w, route, index=False)                                # postings alone: searchable throughout
    try:
        st.insert(5)
        st.append(3)
        free.insert(3)
        free.append(3)
        stale = lambda: pytest.raises(RagError, match=r"\(-3\).*stale")
        with stale():
            st.e.sparse_topk(*w["packed"], 5)
        s0, f0, r0 = state(st.e), state(free.e), results(free.e, w, hybrid=False)
        block = st.block(2, D.V0)
        for name, (ptr, terms, wt, V, cap, msg) in bad_blocks(block, D.V0).items():
            for h in (st, free):
                with pytest.raises(RagError, match=r"\(-1\).*" + msg):
                    call_raw(h.e, route, ptr, terms, wt, V, cap)
            same(state(st.e), s0, name)
            same(state(free.e), f0, name)
            with stale():
                st.e.sparse_topk(*w["packed"], 5)
        three = D.doc_major_of_csr(*D.postings_of(w, st.orig[st.covered - 1:st.covered + 2], D.V0), 3)
        with pytest.raises(RagError, match=r"\(-1\).*more rows than the index has"):
            call_raw(st.e, route, *three, D.V0, None)
        with pytest.raises(RagError, match=r"\(-1\).*n_docs_new must be >= 1"):
            st.e._check(st.e.lib.rag_sparse_append_docs_host(st.e.h, None, None, None, 0, 0, D.V0), "rag_sparse_append_docs_host")
        with pytest.raises(RagError, match=r"\(-1\).*null"):
            st.e._check(st.e.lib.rag_sparse_append_dev(st.e.h, None, None, None, 2, 0, D.V0, None), "rag_sparse_append_dev")
        same(state(st.e), s0, "after every rejection")
        same(results(free.e, w, hybrid=False), r0, "scores after every rejection")
        st.append(2)                                                  # the same handle takes the good block
        check_fresh(st, results(st.e, w), "5 inserted, 3 + 2 appended")
    finally:
        st.close()
        free.close()


# ---- stream order ---------------------------------------------------------------------------------------------------------------
def test_a_search_queued_before_the_append_sees_the_old_postings():
    import torch
    import stream_tools as T
    from optimized_rag_amd import RagEngine
    w = D.world()
    K = 20
    e = RagEngine(dim=D.DIM, device=0)                                # postings alone: appends are always allowed
    try:
        e.set_option("sparse_tail_fold", -1)
        base, more = np.arange(D.N0), np.arange(D.N0, D.N0 + 701)
        e.sparse_load(*D.postings_of(w, base, D.V), D.N0)
        ref_old = e.sparse_topk(*w["packed"], K)
        ptr, terms, wts = (torch.from_numpy(np.array(a)).cuda() for a in w["packed"])
        Q = ptr.shape[0] - 1
        ids = torch.full((Q, K), -7, dtype=torch.int64, device="cuda")
        rows = torch.full((Q, K), -7, dtype=torch.int32, device="cuda")
        sc = torch.full((Q, K), -7.0, dtype=torch.float64, device="cuda")
        bp, bt, bw = (torch.from_numpy(np.array(a)).cuda() for a in D.doc_major_of_csr(*D.postings_of(w, more, D.V), len(more)))
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        T.busy(s, 100.0)
        e.sparse_topk_dev(ptr, terms, wts, K, ids, rows, sc, stream=s)
        pending = not s.query()
        e.sparse_append_dev(bp, bt, bw, D.V)                          # on the default stream: waits for the queued search all the same
        s.synchronize()
        assert pending, "the stream had drained before the append was called: the test showed nothing"
        T.assert_same(T.to_np((ids, rows, sc)), list(ref_old), "queued before the append")
        ref_new = e.sparse_topk(*w["packed"], K)
        assert (ref_new[1] >= D.N0).any() and e.sparse_info()["n_docs"] == D.N0 + 701
    finally:
        e.close()
