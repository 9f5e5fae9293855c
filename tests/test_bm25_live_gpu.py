"""GPU: appendable BM25 postings (rag_bm25_append_host / rag_bm25_fold / rag_bm25_segment_stats).

The contract: statistics are frozen at the last load, and after any sequence of appends every BM25 and hybrid result is
BIT-IDENTICAL to a fresh handle that holds the same rows and was loaded with the merged CSR, the concatenated idf table and the
same avgdl / k1 / b. That fresh load is itself pinned by oracle.rag_oracle.bm25_scores_csr (explicit idf and avgdl) +
stable_topk_desc + rrf_fuse, as tests/test_live_index_gpu.py does for deletes.

The base has 3000 rows - not a multiple of the 2048-document scoring range - so the boundary range exists in both segments;
tenant 2 only owns rows from 2500 on, so a query that matches fewer than k of its documents fills its list with zero-score rows
of that boundary range: a base row emitted by both segments would show up twice."""
import copy

import numpy as np
import pytest

from oracle import rag_oracle as O

pytestmark = pytest.mark.gpu

D = 256
N0 = 3000
BLOCKS = (1, 7, 2048, 3000)
WEIGHTS = (1, -0.5, 0.1)             # tests/test_dense_exactness_gpu.py WEIGHTS[0]: a negative beta


@pytest.fixture(scope="module")
def make():
    from optimized_rag_amd import RagEngine
    made = []

    def mk(dim=D):
        e = RagEngine(dim=dim, device=0)
        made.append(e)
        return e

    yield mk
    for e in made:
        e.close()


def _texts(rng, n, new_terms):
    """Zipf-distributed `t<i>` tokens (tests/test_live_index_gpu.py _postings); with new_terms also `n<j>` tokens that no base
    document holds, and empty documents."""
    out = []
    for L in rng.poisson(12, n):
        w = [f"t{int(x) % 400}" for x in rng.zipf(1.1, int(L)) - 1]
        if new_terms:
            if rng.random() < 0.05:
                w = []
            elif rng.random() < 0.4:
                w += [f"n{int(j)}" for j in rng.integers(0, 40, 3)]
                if rng.random() < 0.03:
                    w += ["rare"]
        out.append(" ".join(w))
    return out


class Live:
    """An engine that takes inserts + appends, and everything a fresh handle / the oracle need to replay it."""
    N0 = N0                                                      # rows of the base (SmallShape: 2048 + 5)

    def make_texts(self, n, new_terms):
        return _texts(self.rng, n, new_terms)

    def base_postings(self):
        from optimized_rag_amd.bm25 import Bm25Postings
        return Bm25Postings.from_corpus(self.texts)

    def __init__(self, make, seed, opts=(), dense=True):
        self.make, self.rng, self.dense = make, np.random.default_rng(seed), dense
        rng, N0 = self.rng, self.N0
        self.texts = self.make_texts(N0, False)
        self.emb = rng.standard_normal((N0, D)).astype(np.float32)
        self.ids = np.arange(N0, dtype=np.int64)[::-1].copy() + 70_000
        self.ten = np.where(np.arange(N0) < 2500, rng.integers(0, 2, N0), rng.integers(0, 3, N0)).astype(np.int32)
        self.dead = np.zeros(N0, dtype=bool)
        self.post = self.base_postings()
        self.V0 = len(self.post.vocab)
        self.eng = make()
        for k_, v in opts:
            self.eng.set_option(k_, v)
        if dense:
            self.eng.index_load(self.emb, ids=self.ids)
            self.eng.set_tenants(self.ten)
        self.post.load(self.eng)

    def new_rows(self, nb):
        rng = self.rng
        n = len(self.ids)
        return (self.make_texts(nb, True), rng.standard_normal((nb, D)).astype(np.float32),
                np.arange(n, n + nb, dtype=np.int64) + 500_000, rng.integers(0, 3, nb).astype(np.int32))

    def insert(self, texts, e, ids, ten):
        if self.dense:
            assert self.eng.index_insert(e, ids=ids, tenants=ten) == len(self.ids)
        self.texts += texts
        self.emb = np.concatenate([self.emb, e])
        self.ids = np.concatenate([self.ids, ids])
        self.ten = np.concatenate([self.ten, ten])
        self.dead = np.concatenate([self.dead, np.zeros(len(ids), dtype=bool)])

    def grow(self, nb):
        texts, e, ids, ten = self.new_rows(nb)
        self.insert(texts, e, ids, ten)
        self.post.append_to(self.eng, self.post.extend(texts))

    def grow_with(self, texts):
        _, e, ids, ten = self.new_rows(len(texts))
        self.insert(texts, e, ids, ten)
        self.post.append_to(self.eng, self.post.extend(texts))

    def delete(self, rows):
        self.dead[rows] = True
        assert self.eng.index_delete(self.ids[rows]) == len(rows)

    def fresh(self, opts=()):
        """A new handle with the same rows, loaded with the MERGED CSR and the frozen statistics."""
        p = self.post
        f = self.make()
        for k_, v in opts:
            f.set_option(k_, v)
        if self.dense:
            f.index_load(self.emb, ids=self.ids)
            f.set_tenants(self.ten)
        f.bm25_load(p.indptr, p.doc, p.tf, p.doc_len, p.idf, p.avgdl, p.k1, p.b)
        if self.dead.any():
            f.index_delete(self.ids[self.dead])
        return f

    def queries(self):
        rng, p = self.rng, self.post
        n = len(self.texts)
        qs = []
        for _ in range(4):                                       # tokens of random documents, base and tail
            toks = (self.texts[int(rng.integers(0, n))] or "t1").split()
            qs.append(" ".join(rng.choice(toks, size=4)))
        toks = (self.texts[n - 1] or self.texts[n - 2] or "t5 t6").split()
        qs.append(" ".join(rng.choice(toks, size=3)))            # the newest document
        qs.append("n3 n7 n3")                                    # terms that occur only in appended documents
        qs.append("rare")                                        # matches fewer than k documents
        df = np.diff(p.indptr)
        few = np.nonzero((df >= 1) & (df <= 4))[0]
        words = list(p.vocab)
        qs.append(" ".join(words[int(t)] for t in few[:2]) if len(few) else "t399")
        qs.append(" ".join(f"t{int(x) % 400}" for x in rng.zipf(1.1, 20) - 1) + " n5")     # longer than 8 plan slots
        qs.append("zzz-unknown")
        return qs

    def raw(self, terms_of_query):
        p = self.post
        return O.bm25_scores_csr(p.indptr, p.doc, p.tf, p.doc_len, p.idf, p.avgdl, terms_of_query, p.k1, p.b)


class SmallShape:
    """Mixin in front of Live (or a subclass): the smallest base whose boundary range exists in both segments - 2048 + 5 rows -
    over at most 64 terms: `s<i>` (s0 .. s35 Zipf, with a bracket table; s36 .. s39 with a handful of postings and none) anywhere,
    `g<j>` only in appended ones. At most 8 queries. empty_terms: the loaded CSR also holds two terms without postings in front
    of every other term and one behind them (equal offsets; each with an idf of its own, so an impact computed with a
    neighbour's idf shows)."""
    N0 = 2048 + 5
    empty_terms = False

    def make_texts(self, n, new_terms):
        rng, out = self.rng, []
        for L in rng.poisson(8, n):
            w = [f"s{min(int(x), 36) - 1}" for x in rng.zipf(1.3, int(L))]
            if rng.random() < 0.01:
                w += [f"s{36 + int(rng.integers(0, 4))}"]
            if new_terms and rng.random() < 0.5:
                w += [f"g{int(j)}" for j in rng.integers(0, 20, 2)]
            out.append(" ".join(w))
        return out

    def base_postings(self):
        p = super().base_postings()
        if self.empty_terms:
            V, nnz = len(p.vocab), int(p.indptr[-1])
            p.indptr = np.concatenate([[0, 0], p.indptr, [nnz]]).astype(np.int64)
            p.idf = np.concatenate([[0.75, 1.25], p.idf, [0.625]])
            p.vocab = {"e0": 0, "e1": 1, **{w: t + 2 for w, t in p.vocab.items()}, "elast": V + 2}
        assert len(p.vocab) <= 44
        return p

    def queries(self):
        rng, n = self.rng, len(self.texts)
        pick = lambda i, m: " ".join(rng.choice((self.texts[i] or "s1").split(), size=m))
        w0 = next(w for w, t in self.post.vocab.items() if t == (2 if self.empty_terms else 0))     # the first term with postings
        return [pick(int(rng.integers(0, n)), 4), pick(int(rng.integers(0, n)), 3), pick(n - 1, 3), "g3 g7 g3", f"{w0} s1 e0 elast",
                "s39 s38 s37 e1", " ".join(f"s{int(x)}" for x in rng.integers(0, 40, 11)) + " g5", "zzz-unknown"]


class Small(SmallShape, Live):
    pass


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def outputs(eng, st, ptr, terms, qd, tenant=-1, dense=True):
    """Every BM25 / hybrid entry point on one handle -> {name: numpy array}."""
    import torch
    out = {}
    Q = len(ptr) - 1
    pd, td = _t(ptr), _t(terms)
    for k in (10, 100):
        ids, rows, sc, mx = eng.bm25_topk(ptr, terms, k, tenant=tenant)
        out.update({f"topk{k}_ids": ids, f"topk{k}_rows": rows, f"topk{k}_sc": sc, f"topk{k}_max": mx})
        di = torch.empty((Q, k), dtype=torch.int64, device="cuda")
        dr = torch.empty((Q, k), dtype=torch.int32, device="cuda")
        ds = torch.empty((Q, k), dtype=torch.float64, device="cuda")
        dm = torch.empty((Q,), dtype=torch.float64, device="cuda")
        eng.bm25_topk_dev(pd, td, k, di, dr, ds, dm, tenant=tenant)
        torch.cuda.synchronize()
        out.update({f"dev{k}_ids": di.cpu().numpy(), f"dev{k}_rows": dr.cpu().numpy(), f"dev{k}_sc": ds.cpu().numpy(),
                    f"dev{k}_max": dm.cpu().numpy()})
    out["scores"] = eng.bm25_scores(ptr, terms)
    if dense:
        keys, rrf, ranks = eng.hybrid_rrf_dev(qd, pd, td, 40, 20, tenant=tenant)
        torch.cuda.synchronize()
        out.update({"rrf_keys": keys.cpu().numpy().copy(), "rrf_sc": rrf.cpu().numpy().copy(), "rrf_ranks": ranks.cpu().numpy().copy()})
        hy = eng.hybrid_linear_dev(qd, pd, td, 20, *WEIGHTS, tenant=tenant)
        torch.cuda.synchronize()
        out.update({f"lin_{k_}": v.cpu().numpy().copy() for k_, v in hy.items()})
    return out


def same_bits(a, b):
    assert a.keys() == b.keys()
    for name in a:
        x, y = a[name], b[name]
        assert x.shape == y.shape and x.dtype == y.dtype, name
        if x.dtype.kind == "f":
            x, y = x.view(np.int64 if x.dtype == np.float64 else np.int32), y.view(np.int64 if y.dtype == np.float64 else np.int32)
        np.testing.assert_array_equal(x, y, err_msg=name)


def check_oracle(st, got, ptr, terms, qd, tenant=-1, normalize=True, dense=True):
    Q = len(ptr) - 1
    keep = ~st.dead & ((st.ten == tenant) if tenant >= 0 else True)
    raws = [st.raw(terms[ptr[qi]:ptr[qi + 1]]) for qi in range(Q)]
    for qi in range(Q):
        raw = np.where(keep, raws[qi], -np.inf)
        mx = raw.max() if raw.max() > 0 else 1.0
        for k in (10, 100):
            top = O.stable_topk_desc(raw, k)
            top = top[np.isfinite(raw[top])]
            for pre in ("topk", "dev"):
                rows, ids, sc = got[f"{pre}{k}_rows"][qi], got[f"{pre}{k}_ids"][qi], got[f"{pre}{k}_sc"][qi]
                np.testing.assert_array_equal(rows[:len(top)], top.astype(np.int32), err_msg=f"{pre}{k} q{qi}")
                assert (rows[len(top):] == -1).all() and (ids[len(top):] == -1).all()
                assert len(set(rows[:len(top)].tolist())) == len(top)                       # no row twice
                np.testing.assert_array_equal(ids[:len(top)], st.ids[top] if dense else top)
                np.testing.assert_array_equal(sc[:len(top)], raws[qi][top] / mx if normalize else raws[qi][top])
                assert got[f"{pre}{k}_max"][qi] == mx
        np.testing.assert_array_equal(got["scores"][qi], np.where(st.dead, 0.0, raws[qi]))
    if not dense:
        return
    if tenant < 0:
        lv = np.nonzero(~st.dead)[0]
        d_rows, _ = O.dense_topk(st.emb[lv], qd.cpu().numpy(), 40)
        for qi in range(Q):
            raw = np.where(keep, raws[qi], -np.inf)
            b_rows = O.stable_topk_desc(raw, 40)
            b_rows = b_rows[np.isfinite(raw[b_rows])]
            okeys, oscores, oranks = O.rrf_fuse([[int(st.ids[lv[r]]) for r in d_rows[qi] if r >= 0], [int(st.ids[r]) for r in b_rows]],
                                                k=60, top_k=20)
            assert got["rrf_keys"][qi].tolist()[:len(okeys)] == okeys
            assert got["rrf_sc"][qi].tolist()[:len(oscores)] == oscores
            assert got["rrf_ranks"][qi].tolist()[:len(oranks)] == [list(r) for r in oranks]
    # linear fusion: the keyword component of every returned row is its raw score over the best live (tenant) document
    for qi in range(Q):
        raw = np.where(keep, raws[qi], -np.inf)
        mx = raw.max() if raw.max() > 0 else 1.0
        rows = got["lin_rows"][qi]
        ok = rows >= 0
        assert keep[rows[ok]].all()
        np.testing.assert_array_equal(got["lin_keyword"][qi][ok], raws[qi][rows[ok]] / mx)
        np.testing.assert_array_equal(got["lin_ids"][qi][ok], st.ids[rows[ok]])


def full_check(st, tenant=-1, fresh_opts=(), normalize=True, fresh=None):
    qs = st.queries()
    ptr, terms = st.post.encode_queries(qs)
    n = len(st.ids)
    qd = _t((st.emb[st.rng.integers(0, n, len(qs))] + 0.5 * st.rng.standard_normal((len(qs), D))).astype(np.float32)) if st.dense else None
    got = outputs(st.eng, st, ptr, terms, qd, tenant, st.dense)
    f = fresh or st.fresh(fresh_opts)
    if not normalize:
        f.bm25_set_normalize(False)
    same_bits(got, outputs(f, st, ptr, terms, qd, tenant, st.dense))
    check_oracle(st, got, ptr, terms, qd, tenant, normalize, st.dense)
    if fresh is None:
        f.close()
    return got


def test_appends_equal_a_load_of_the_merged_csr(make):
    st = Live(make, 101)
    for nb in BLOCKS:
        st.grow(nb)
        s = st.eng.bm25_segment_stats()
        assert s["base_docs"] == N0 and s["tail_docs"] == len(st.ids) - N0 and s["n_terms"] == len(st.post.vocab)
        assert s["base_nnz"] + s["tail_nnz"] == int(st.post.indptr[-1]) and s["tail_bytes"] > 0
        full_check(st)
    s = st.eng.bm25_segment_stats()
    assert s["appends"] == len(BLOCKS) and s["folds"] == 0 and s["n_terms"] > st.V0
    assert sum(1 for t in st.texts[N0:] if not t) > 0            # empty documents went through
    full_check(st, tenant=2)                                     # tenant 2: rows >= 2500 only (the boundary range and the tail)
    full_check(st, tenant=0)


def test_long_queries_deletes_in_both_segments_and_raw_mode(make):
    opts = (("bm25_plan_slots", 8),)
    st = Live(make, 103, opts)
    for nb in (7, 2048, 300):
        st.grow(nb)
    full_check(st, fresh_opts=opts)
    n = len(st.ids)
    rows = np.unique(np.concatenate([st.rng.integers(0, N0, 400), st.rng.integers(N0, n, 300), np.arange(2040, 2060),
                                     np.arange(N0 - 5, N0 + 5)]))
    # the best hits of "rare" and of the new-term query go too
    ptr, terms = st.post.encode_queries(["rare", "n3 n7 n3"])
    for qi in range(2):
        rows = np.union1d(rows, O.stable_topk_desc(st.raw(terms[ptr[qi]:ptr[qi + 1]]), 3))
    st.delete(rows)
    full_check(st, fresh_opts=opts)
    full_check(st, tenant=2, fresh_opts=opts)
    st.eng.bm25_set_normalize(False)
    full_check(st, fresh_opts=opts, normalize=False)
    st.eng.bm25_set_normalize(True)
    for o in ("bm25_no_staging", "bm25_sort_merge", "bm25_linear_grid"):
        st.eng.set_option(o, 1)
        full_check(st, fresh_opts=opts)
        st.eng.set_option(o, 0)


def test_appends_behind_a_packed_base(make):
    st = Live(make, 107, (("bm25_packed", 1),))
    for nb in (7, 2048):
        st.grow(nb)
    full_check(st)                                               # against an UNPACKED load of the merged CSR
    full_check(st, tenant=2, fresh_opts=(("bm25_packed", 1),))
    from optimized_rag_amd import RagError
    with pytest.raises(RagError, match="packed"):
        st.eng.bm25_fold()
    st.eng.set_option("bm25_tail_fold", 5)                       # the automatic fold leaves a packed base alone
    st.grow(9)
    s = st.eng.bm25_segment_stats()
    assert s["folds"] == 0 and s["tail_docs"] == 7 + 2048 + 9
    full_check(st)


def test_standalone_postings_without_a_dense_index(make):
    st = Live(make, 109, dense=False)
    for nb in (1, 2500):
        st.grow(nb)
        full_check(st)


def test_fold(make):
    st = Live(make, 113, (("bm25_tail_fold", -1),))
    for nb in (7, 2048, 3000):
        st.grow(nb)
    f = st.fresh()
    qs = st.queries()
    ptr, terms = st.post.encode_queries(qs)
    qd = _t((st.emb[:len(qs)] + 0.25).astype(np.float32))
    before = outputs(st.eng, st, ptr, terms, qd)
    s0 = st.eng.bm25_segment_stats()
    assert s0["tail_docs"] == 5055 and s0["folds"] == 0
    st.eng.bm25_fold()
    s1 = st.eng.bm25_segment_stats()
    assert s1["tail_docs"] == 0 and s1["tail_nnz"] == 0 and s1["tail_bytes"] == 0 and s1["folds"] == 1
    assert s1["base_docs"] == N0 + 5055 and s1["base_nnz"] == s0["base_nnz"] + s0["tail_nnz"] and s1["n_terms"] == s0["n_terms"]
    same_bits(before, outputs(st.eng, st, ptr, terms, qd))
    same_bits(before, outputs(f, st, ptr, terms, qd))
    f.close()
    st.eng.bm25_fold()                                           # nothing to fold: a no-op
    assert st.eng.bm25_segment_stats()["folds"] == 1
    st.grow(11)                                                  # appends go on behind the folded base (8055 rows: not a range multiple)
    full_check(st)
    full_check(st, tenant=2)


def test_fold_by_itself(make):
    st = Live(make, 127, (("bm25_tail_fold", 5),))
    st.grow(3)
    assert st.eng.bm25_segment_stats()["tail_docs"] == 3
    st.grow(2)
    s = st.eng.bm25_segment_stats()
    assert s["tail_docs"] == 5 and s["folds"] == 0               # folds once the tail holds MORE than 5 documents
    st.grow(1)
    s = st.eng.bm25_segment_stats()
    assert s["tail_docs"] == 0 and s["folds"] == 1 and s["base_docs"] == N0 + 6 and s["appends"] == 3
    full_check(st)
    st.eng.set_option("bm25_tail_fold", -1)
    st.grow(2500)
    assert st.eng.bm25_segment_stats()["tail_docs"] == 2500
    full_check(st)


def test_first_append_is_an_empty_block(make):
    """the tail's vocabulary is the base's while it holds no posting at all; then postings arrive, then the fold"""
    st = Small(make, 151, (("bm25_tail_fold", -1),))
    st.grow_with([""] * 5)
    s = st.eng.bm25_segment_stats()
    assert s["tail_docs"] == 5 and s["tail_nnz"] == 0 and s["n_terms"] == st.V0 > 0
    full_check(st)
    full_check(st, tenant=2)
    st.grow(300)
    assert st.eng.bm25_segment_stats()["tail_nnz"] > 0
    full_check(st)
    st.eng.bm25_fold()
    s = st.eng.bm25_segment_stats()
    assert s["tail_docs"] == 0 and s["base_docs"] == st.N0 + 305 and s["folds"] == 1
    full_check(st)
    full_check(st, tenant=2)


def test_vocabulary_grows_behind_a_smaller_tail(make):
    """old tail: the base's terms only; the next block brings the `g` terms, so old tail ++ block merges V_old < V lists, and the
    fold merges the base's V_base < V with the tail's"""
    st = Small(make, 157, (("bm25_tail_fold", -1),))
    st.grow_with(st.make_texts(200, False))
    assert st.eng.bm25_segment_stats()["n_terms"] == st.V0
    full_check(st)
    st.grow(300)
    V = st.eng.bm25_segment_stats()["n_terms"]
    assert st.V0 < V == len(st.post.vocab) <= 64
    assert all(int(st.post.doc[st.post.indptr[t]]) >= st.N0 + 200 for t in range(st.V0, V))      # new terms: only in the block
    full_check(st)
    full_check(st, tenant=2)
    st.eng.bm25_fold()
    assert st.eng.bm25_segment_stats()["tail_docs"] == 0
    full_check(st)
    st.grow(7)                                                   # and a tail behind the grown base
    full_check(st, tenant=2)


def test_partial_coverage_stays_stale(make):
    from optimized_rag_amd import RagError
    st = Live(make, 131)
    texts, e, ids, ten = st.new_rows(5)
    st.insert(texts, e, ids, ten)
    ptr, terms = st.post.encode_queries(["t1 t2 t3"])
    qd = _t(st.emb[:1])
    with pytest.raises(RagError, match="stale"):
        st.eng.bm25_topk(ptr, terms, 10)
    st.post.append_to(st.eng, st.post.extend(texts[:3]))
    assert st.eng.bm25_segment_stats()["tail_docs"] == 3
    with pytest.raises(RagError, match="stale"):
        st.eng.bm25_topk(ptr, terms, 10)
    with pytest.raises(RagError, match="stale"):
        st.eng.bm25_scores(ptr, terms)
    with pytest.raises(RagError, match="stale"):
        st.eng.hybrid_rrf_dev(qd, _t(ptr), _t(terms), 40, 20)
    with pytest.raises(RagError, match="stale"):
        st.eng.hybrid_linear_dev(qd, _t(ptr), _t(terms), 20, *WEIGHTS)
    st.post.append_to(st.eng, st.post.extend(texts[3:]))
    full_check(st)


def test_failed_appends_change_nothing(make):
    from optimized_rag_amd import RagEngine, RagError
    st = Live(make, 137)
    st.grow(40)
    ptr, terms = st.post.encode_queries(st.queries())
    qd = _t(st.emb[:len(ptr) - 1])
    before = outputs(st.eng, st, ptr, terms, qd)
    s0 = st.eng.bm25_segment_stats()
    blk = copy.deepcopy(st.post).extend(["t1 t2 brandnew", "t3"])
    with pytest.raises(RagError, match="more rows"):             # the index has no such rows
        st.eng.bm25_append(blk["indptr"], blk["doc"], blk["tf"], blk["doc_len"], blk["idf_new"], blk["n_terms_total"])
    assert st.eng.bm25_segment_stats() == s0
    same_bits(before, outputs(st.eng, st, ptr, terms, qd))       # the next search: the previous result bit for bit
    # malformed blocks for rows that DO exist: refused, and the postings stay as stale as the insert left them
    texts, e, ids, ten = st.new_rows(2)
    st.insert(texts, e, ids, ten)
    blk = copy.deepcopy(st.post).extend(texts)
    V = blk["n_terms_total"]
    for bad in (dict(blk, doc=blk["doc"] + 2),                                            # a document number past the block
                dict(blk, doc=blk["doc"][::-1].copy()),                                   # not ascending inside a term
                dict(blk, indptr=np.concatenate([blk["indptr"][:-1], blk["indptr"][-1:] + 5])),   # more postings than documents
                dict(blk, doc_len=blk["doc_len"][:0])):                                   # n_docs_new < 1
        arrs = [np.ascontiguousarray(bad[k_]) for k_ in ("indptr", "doc", "tf", "doc_len", "idf_new")]
        with pytest.raises(RagError):       # through the C entry itself: the Python wrapper's own shape checks are not the point
            st.eng._check(st.eng.lib.rag_bm25_append_host(st.eng.h, *[a.ctypes.data for a in arrs], len(arrs[3]), V), "rag_bm25_append_host")
    with pytest.raises(RagError):                                # the vocabulary may not shrink
        st.eng.bm25_append(np.zeros(st.V0, np.int64), blk["doc"][:0], blk["tf"][:0], blk["doc_len"], blk["idf_new"][:0], st.V0 - 1)
    assert st.eng.bm25_segment_stats() == s0
    with pytest.raises(RagError, match="stale"):
        st.eng.bm25_topk(ptr, terms, 10)
    st.post.append_to(st.eng, st.post.extend(texts))
    full_check(st)
    # no postings loaded
    e = RagEngine(dim=D, device=0)
    try:
        with pytest.raises(RagError, match="no postings"):
            e.bm25_append(blk["indptr"], blk["doc"], blk["tf"], blk["doc_len"], blk["idf_new"], blk["n_terms_total"])
        with pytest.raises(RagError):
            e.bm25_segment_stats()
    finally:
        e.close()


def test_compaction_needs_a_reload(make):
    from optimized_rag_amd import RagError
    from optimized_rag_amd.bm25 import Bm25Postings
    st = Live(make, 139)
    st.grow(30)
    st.delete(np.array([3, 2050, N0 + 4]))
    full_check(st)
    st.eng.index_compact()
    ptr, terms = st.post.encode_queries(["t1 t2 t3"])
    with pytest.raises(RagError, match="stale"):
        st.eng.bm25_topk(ptr, terms, 10)
    # rows inserted and appended after the compaction do not align the postings again
    # (6 rows, a block of 3: after the compaction took 3 rows away the covered rows then EQUAL the index rows - and still
    # describe other rows)
    e = st.rng.standard_normal((6, D)).astype(np.float32)
    st.eng.index_insert(e, ids=np.arange(6, dtype=np.int64) + 9_000_001, tenants=np.zeros(6, np.int32))
    blk = copy.deepcopy(st.post).extend(["t1", "t2", "t3 t3"])
    st.eng.bm25_append(blk["indptr"], blk["doc"], blk["tf"], blk["doc_len"], blk["idf_new"], blk["n_terms_total"])
    with pytest.raises(RagError, match="stale"):
        st.eng.bm25_topk(ptr, terms, 10)
    assert st.eng.bm25_segment_stats()["base_docs"] + st.eng.bm25_segment_stats()["tail_docs"] == len(st.ids) - 3 + 6
    live = [t for t, d in zip(st.texts, st.dead) if not d] + ["t1", "t2", "t3 t3", "t4", "", "t1 t9"]
    post2 = Bm25Postings.from_corpus(live).load(st.eng)
    assert st.eng.bm25_segment_stats()["tail_docs"] == 0 and st.eng.bm25_segment_stats()["appends"] == 0
    ptr2, terms2 = post2.encode_queries(["t1 t2 t3"])
    _, rows, _, _ = st.eng.bm25_topk(ptr2, terms2, 10)
    raw = O.bm25_scores_csr(post2.indptr, post2.doc, post2.tf, post2.doc_len, post2.idf, post2.avgdl, terms2)
    np.testing.assert_array_equal(rows[0], O.stable_topk_desc(raw, 10).astype(np.int32))


def test_retrieve_rerank_candidates_after_appends():
    """rag_retrieve_rerank_dev mode 1 (dense + BM25 + RRF candidates -> cross-encoder), the headline path an insert used to
    take down: candidate lists and reranked outputs equal the fresh handle's, the candidates the oracle's RRF top-pool."""
    import torch
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.bm25 import Bm25Postings
    from optimized_rag_amd.cross_encoder import random_init_tensors
    rng = np.random.default_rng(149)
    Dm, Q, pool, k, Ld, Lq, L = 1536, 4, 10, 5, 24, 6, 32
    n_new = (1, 2100)
    N = N0 + sum(n_new)
    cfg = dict(vocab_size=3000, hidden=384, layers=2, heads=12, ffn=1536, max_pos=64, type_vocab=2, eps=1e-12)
    emb = rng.standard_normal((N, Dm)).astype(np.float32)
    tok = rng.integers(200, cfg["vocab_size"], (N, Ld)).astype(np.int32)
    tok_len = rng.integers(3, Ld + 1, N).astype(np.int32)
    pick = rng.integers(N0 - 50, N, Q)                           # queries near the boundary range and in the tail
    q_emb = (emb[pick] + 0.5 * rng.standard_normal((Q, Dm))).astype(np.float32)
    q_tok, q_len = tok[pick, :Lq].copy(), np.minimum(tok_len[pick], Lq).astype(np.int32)
    corpus = [" ".join(f"t{t}" for t in tok[i, :tok_len[i]] % (50 if i < N0 else 70)) for i in range(N)]
    queries = [" ".join(f"t{t}" for t in q_tok[i, :q_len[i]] % 70) for i in range(Q)]
    t = lambda a: torch.from_numpy(a).cuda()
    eng, fresh = RagEngine(dim=Dm, device=0), RagEngine(dim=Dm, device=0)
    try:
        post = Bm25Postings.from_corpus(corpus[:N0])
        eng.index_load(emb[:N0])
        eng.tokens_load(tok[:N0], tok_len[:N0])
        eng.ce_load(cfg, random_init_tensors(cfg, 3))
        post.load(eng)
        a = N0
        for nb in n_new:
            eng.index_insert(emb[a:a + nb], tokens=tok[a:a + nb], token_lens=tok_len[a:a + nb])
            post.append_to(eng, post.extend(corpus[a:a + nb]))
            a += nb
        assert len(post.vocab) > 50 and eng.bm25_segment_stats()["tail_docs"] == sum(n_new)
        fresh.index_load(emb)
        fresh.tokens_load(tok, tok_len)
        fresh.ce_load(cfg, random_init_tensors(cfg, 3))
        fresh.bm25_load(post.indptr, post.doc, post.tf, post.doc_len, post.idf, post.avgdl)
        ptr, terms = post.encode_queries(queries)
        args = (t(q_emb), t(q_tok), t(q_len), pool, k)
        got = [x.cpu().numpy().copy() for x in eng.retrieve_rerank_dev(*args, term_ptr=t(ptr), terms=t(terms), L_pair=L)]
        ref = [x.cpu().numpy().copy() for x in fresh.retrieve_rerank_dev(*args, term_ptr=t(ptr), terms=t(terms), L_pair=L)]
        torch.cuda.synchronize()
    finally:
        eng.close()
        fresh.close()
    for x, y in zip(got, ref):
        np.testing.assert_array_equal(x.view(np.int64 if x.dtype == np.float64 else x.dtype), y.view(np.int64 if y.dtype == np.float64 else y.dtype))
    d_rows, _ = O.dense_topk(emb, q_emb, pool)
    for qi in range(Q):
        raw = O.bm25_scores_csr(post.indptr, post.doc, post.tf, post.doc_len, post.idf, post.avgdl, terms[ptr[qi]:ptr[qi + 1]])
        okeys, _, _ = O.rrf_fuse([[int(r) for r in d_rows[qi]], [int(r) for r in O.stable_topk_desc(raw, pool)]], k=60, top_k=pool)
        assert got[3][qi].tolist()[:len(okeys)] == okeys
