"""GPU: BM25 statistics refreshed on the device (rag_bm25_live_counts_host / rag_bm25_set_statistics_host / rag_bm25_refresh,
option bm25_keep_tf).

The contract, checked by every scenario: after a refresh every BM25 / hybrid output is BIT-IDENTICAL to a fresh handle (loaded
WITHOUT the option) that holds the same rows with the same deletes and was loaded with the merged CSR, the refreshed idf table
and avgdl; that fresh load is what the oracle computes from those numbers (check_oracle); and the idf table the device
returns is the host mirror's (Bm25Postings.refresh) bit for bit. Helpers and the 3000-row base come from
tests/test_bm25_live_gpu.py and tests/test_bm25_compact_gpu.py."""
import copy
import math

import numpy as np
import pytest

import stream_tools as T
from oracle import rag_oracle as O
from test_bm25_compact_gpu import CLive, NO_FOLD, PACKED, TENANTS, _delete_in_both
from test_bm25_live_gpu import D, N0, SmallShape, check_oracle, full_check, outputs, same_bits

pytestmark = pytest.mark.gpu

KEEP = (("bm25_keep_tf", 1),)
BOTH = pytest.mark.parametrize("opts", [NO_FOLD, PACKED], ids=["plain", "packed"])


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


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def _shift_texts(rng, n):
    """Long documents over t0 and the terms t30 .. t59 only: appended to the Zipf base they turn rare terms into common ones, keep
    t0 in more than half of the corpus (a negative raw idf) and raise avgdl - a change of scale alone would leave idf as it is."""
    return [" ".join(["t0"] + [f"t{int(x)}" for x in rng.integers(30, 60, int(L))]) for L in rng.poisson(30, n)]


SHIFT_QUERIES = ["t31 t200 t7", "t45 t45 t120", "t3 t58", "t33 t150 t151 t12", "t59 t2 t2 t90", "t40 t300", "t0 t35 t210"]


class RLive(CLive):
    """CLive with option bm25_keep_tf on the engine (never on the fresh handles), and the refresh with its host mirror."""

    def __init__(self, make, seed, opts=(), dense=True, rare_rows=(), keep=True):
        super().__init__(make, seed, tuple(opts) + (KEEP if keep else ()), dense, rare_rows)
        self.extra_queries = []

    def queries(self):
        return super().queries() + self.extra_queries

    def live(self):
        return ~self.dead[:self.post.n_docs]

    def counts(self):
        """numpy on the mirror: live postings per term, live documents, the sum of their lengths"""
        p, live = self.post, self.live()
        V = p.indptr.shape[0] - 1
        term_of = np.repeat(np.arange(V), np.diff(p.indptr))
        return np.bincount(term_of[live[p.doc]], minlength=V), int(live.sum()), int(p.doc_len[live].sum())

    def refresh(self):
        df, n, s = self.counts()
        avgdl_before = self.post.avgdl
        idf, info = self.eng.bm25_refresh(self.post.epsilon)
        old = self.post.idf.copy()
        self.post.refresh(self.live())
        np.testing.assert_array_equal(_bits(idf), _bits(self.post.idf))
        assert info["n_docs_live"] == n and info["nnz_live"] == int(df.sum()) and info["n_terms"] == len(df)
        assert info["avgdl_after"] == self.post.avgdl == s / n and info["avgdl_before"] == avgdl_before
        assert info["terms_without_postings"] == int((df == 0).sum())
        assert info["negative_idf_terms"] == int(((df > 0) & (2 * df > n)).sum())        # ln(N - df + .5) < ln(df + .5)
        assert info["idf_max_abs_change"] == np.abs(self.post.idf - old).max()
        return idf, info


def _fresh_opts(opts):
    return PACKED if opts is PACKED else ()


def _batch(st, queries):
    ptr, terms = st.post.encode_queries(queries)
    qd = _t((st.emb[:len(queries)] + 0.25).astype(np.float32))
    return ptr, terms, qd


def _tops(st, ptr, terms, k=10):
    keep = ~st.dead
    return [O.stable_topk_desc(np.where(keep, st.raw(terms[ptr[q]:ptr[q + 1]]), -np.inf), k).tolist() for q in range(len(ptr) - 1)]


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@BOTH
def test_grown_index_without_deletes(make, opts):
    st = RLive(make, 501, opts)
    st.grow_with(_shift_texts(st.rng, 3000))
    if opts is NO_FOLD:
        st.eng.bm25_fold()                                            # a base alone (a packed base cannot absorb its tail)
        assert st.eng.bm25_segment_stats()["tail_docs"] == 0
    st.extra_queries = SHIFT_QUERIES
    ptr, terms, qd = _batch(st, SHIFT_QUERIES)
    before = outputs(st.eng, st, ptr, terms, qd)
    tops_frozen = _tops(st, ptr, terms)
    np.testing.assert_array_equal(before["topk10_rows"], np.array(tops_frozen, dtype=np.int32))
    s0 = st.eng.bm25_segment_stats()
    idf, info = st.refresh()
    assert st.eng.bm25_segment_stats() == s0                          # offsets and segments are not touched
    assert info["n_docs_live"] == N0 + 3000 and info["terms_without_postings"] == 0 and info["negative_idf_terms"] > 0
    assert info["idf_max_abs_change"] > 1.0 and info["avgdl_after"] > info["avgdl_before"] + 5
    tops_fresh = _tops(st, ptr, terms)
    assert tops_fresh != tops_frozen                                  # the oracle alone: fresh statistics rank differently
    after = outputs(st.eng, st, ptr, terms, qd)
    np.testing.assert_array_equal(after["topk10_rows"], np.array(tops_fresh, dtype=np.int32))
    assert (after["topk10_rows"] != before["topk10_rows"]).any()
    for t in TENANTS:
        full_check(st, tenant=t, fresh_opts=_fresh_opts(opts))
    if opts is PACKED:
        full_check(st)                                                # and against an UNPACKED load


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@BOTH
def test_base_and_tail_with_deletes(make, opts):
    st = RLive(make, 503, opts)
    for nb in (7, 2048):
        st.grow(nb)
    st.grow_with(_shift_texts(st.rng, 600))
    assert st.eng.bm25_segment_stats()["tail_docs"] == 2655
    rows = _delete_in_both(st)
    df, n, s = st.counts()
    assert (df < np.diff(st.post.indptr)).any() and n == len(st.ids) - len(rows)
    got_df, got_n, got_s = st.eng.bm25_live_counts()
    np.testing.assert_array_equal(got_df, df.astype(np.int32))        # live postings only, base and tail together
    assert (got_n, got_s) == (n, s)
    st.refresh()
    np.testing.assert_array_equal(st.eng.bm25_live_counts()[0], df.astype(np.int32))      # counting changes nothing
    st.extra_queries = SHIFT_QUERIES
    for t in TENANTS:
        full_check(st, tenant=t, fresh_opts=_fresh_opts(opts))
    st.eng.bm25_set_normalize(False)
    full_check(st, fresh_opts=_fresh_opts(opts), normalize=False)
    full_check(st, tenant=2, fresh_opts=_fresh_opts(opts), normalize=False)
    st.eng.bm25_set_normalize(True)


def test_live_counts_without_deletes_and_standalone(make):
    """nothing deleted: df is the difference of the offsets (no posting is read); a handle without a dense index has no deletes"""
    st = RLive(make, 505, NO_FOLD, dense=False)
    st.grow(2500)
    df, n, s = st.eng.bm25_live_counts()
    np.testing.assert_array_equal(df, np.diff(st.post.indptr).astype(np.int32))
    assert (n, s) == (st.post.n_docs, int(st.post.doc_len.sum()))
    st.post.refresh_on(st.eng)                                        # asserts the two idf tables agree
    full_check(st)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def _step_check(st, rng, opts):
    qs, ptr, terms, qd = st.query_batch()
    tenant = TENANTS[int(rng.integers(0, 3))]
    got = outputs(st.eng, st, ptr, terms, qd, tenant)
    f = st.fresh(_fresh_opts(opts))
    same_bits(got, outputs(f, st, ptr, terms, qd, tenant))
    f.close()
    return got, ptr, terms, qd, tenant


def _delete_some(st, rng):
    lv = np.nonzero(~st.dead)[0]
    st.delete(rng.choice(lv, int(rng.integers(1, max(2, len(lv) // 4))), replace=False))


@pytest.mark.parametrize("order", ["refresh grow fold delete compact refresh grow refresh",
                                   "grow delete compact refresh shift fold refresh delete refresh compact",
                                   "shift refresh delete refresh compact grow grow fold compact refresh"])
def test_refresh_between_appends_folds_and_compactions(make, order):
    rng = np.random.default_rng(len(order))
    st = RLive(make, 507 + len(order), NO_FOLD)
    st.extra_queries = SHIFT_QUERIES[:3]
    for op in order.split():
        _apply(st, rng, op, NO_FOLD)
        got, ptr, terms, qd, tenant = _step_check(st, rng, NO_FOLD)
    check_oracle(st, got, ptr, terms, qd, tenant)
    s = st.eng.bm25_segment_stats()
    assert s["base_nnz"] + s["tail_nnz"] == int(st.post.indptr[-1])


def _apply(st, rng, op, opts):
    if op == "grow":
        st.grow(int(rng.choice([1, 5, 40, 300])))
    elif op == "shift":
        st.grow_with(_shift_texts(rng, int(rng.choice([30, 900]))))
    elif op == "delete":
        _delete_some(st, rng)
    elif op == "fold":
        if opts is not PACKED:
            st.eng.bm25_fold()
    elif op == "compact":
        st.compact()
        st.check_stats()
    else:
        st.refresh()


@pytest.mark.parametrize("seq", range(8))
def test_seeded_random_sequences(make, seq):
    rng = np.random.default_rng(7000 + seq)
    opts = (NO_FOLD, PACKED, (("bm25_tail_fold", 64),), ())[seq % 4]
    st = RLive(make, 600 + seq, opts)
    try:
        ops = list(rng.permutation(["grow", "shift", "delete", "fold", "compact", "refresh"])) + \
            list(rng.choice(["grow", "delete", "fold", "compact", "refresh"], 2)) + ["refresh"]
        for op in ops:
            _apply(st, rng, str(op), opts)
            got, ptr, terms, qd, tenant = _step_check(st, rng, opts)
        check_oracle(st, got, ptr, terms, qd, tenant)
    finally:
        st.eng.close()


class SmallR(SmallShape, RLive):
    pass


@BOTH
def test_small_life_cycle_keeps_tf_and_lengths(make, opts):
    """append -> compaction that keeps the postings -> append -> fold (a packed base refuses it) -> refresh on the 2048 + 5 row
    base: every step moves the kept tf plane / value tables and the document lengths along"""
    from optimized_rag_amd import RagError
    st = SmallR(make, 521, opts)
    st.grow(300)
    st.delete(np.unique(np.concatenate([st.rng.integers(0, len(st.ids), 150), np.arange(2040, 2060)])))
    st.compact()
    s = st.check_stats()
    assert s["tail_docs"] > 0 and s["base_docs"] < st.N0
    full_check(st, fresh_opts=_fresh_opts(opts))
    st.grow(200)
    if opts is PACKED:
        with pytest.raises(RagError, match=r"\(-3\).*bm25_fold: the base postings are packed \(option bm25_packed\)"):
            st.eng.bm25_fold()
    else:
        st.eng.bm25_fold()
        assert st.check_stats()["tail_docs"] == 0
    full_check(st, fresh_opts=_fresh_opts(opts))
    st.delete(st.rng.choice(len(st.ids), 40, replace=False))
    _, info = st.refresh()
    assert info["n_docs_live"] == len(st.ids) - 40 and info["idf_max_abs_change"] > 0
    for t in TENANTS:
        full_check(st, tenant=t, fresh_opts=_fresh_opts(opts))
    if opts is PACKED:
        full_check(st)                                                # and against an UNPACKED load


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def test_a_term_that_loses_every_posting(make):
    st = RLive(make, 509, NO_FOLD, rare_rows=(17, 2047, 2999))
    st.grow(300)
    t_rare = st.post.vocab["rare"]
    rows = np.array([i for i, t in enumerate(st.texts) if "rare" in t.split()])
    assert len(rows) >= 3
    st.delete(rows)
    idf, info = st.refresh()
    n = len(st.ids) - len(rows)
    assert info["terms_without_postings"] >= 1 and info["n_docs_live"] == n
    assert idf[t_rare] == math.log(n + 0.5) - math.log(0.5) and st.post.vocab["rare"] == t_rare
    full_check(st)
    ptr, terms = st.post.encode_queries(["rare"])
    assert not st.eng.bm25_topk(ptr, terms, 10)[2].any()
    st.compact()                                                      # the term has an empty list now and keeps its idf
    st.refresh()
    full_check(st, tenant=2)


@BOTH
@pytest.mark.parametrize("segment", ["base", "tail"])
def test_every_row_of_one_segment_deleted(make, opts, segment):
    st = RLive(make, 511, opts)
    for nb in (7, 300):
        st.grow(nb)
    st.delete(np.arange(N0) if segment == "base" else np.arange(N0, N0 + 307))
    _, info = st.refresh()
    assert info["n_docs_live"] == (307 if segment == "base" else N0) and info["terms_without_postings"] > 0
    for t in TENANTS:
        full_check(st, tenant=t, fresh_opts=_fresh_opts(opts))
    st.compact()                                                      # a tail replaces the emptied base / the tail is dropped
    st.grow(5)
    st.refresh()
    full_check(st, fresh_opts=_fresh_opts(opts) if segment == "tail" else ())


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
@BOTH
def test_set_statistics_with_the_callers_own_table(make, opts):
    st = RLive(make, 513, opts)
    st.grow(2048)
    _delete_in_both(st)
    p = st.post
    p.idf = np.ones_like(p.idf)
    p.avgdl = 2.0 * p.avgdl
    st.eng.bm25_set_statistics(p.idf, p.avgdl)
    full_check(st, fresh_opts=_fresh_opts(opts))
    # negative values of the caller's own, and idf 0.0 for a third of the terms: the scoring kernels skip such a term's postings
    # by the idf in the term metadata, base and tail
    t = np.arange(len(p.idf))
    p.idf = np.where(t % 3 == 0, -0.5, np.where(t % 3 == 1, 0.0, 0.25 + t / 64.0))
    p.avgdl = 3.5
    st.eng.bm25_set_statistics(p.idf, p.avgdl)
    st.extra_queries = SHIFT_QUERIES
    full_check(st, tenant=2, fresh_opts=_fresh_opts(opts))
    st.grow(9)                                                        # later appends use the installed statistics
    full_check(st, fresh_opts=_fresh_opts(opts))
    st.refresh()                                                      # ... and the terms that had idf 0.0 count again, in both segments
    assert (st.post.idf != 0.0).all()
    for tn in TENANTS:
        full_check(st, tenant=tn, fresh_opts=_fresh_opts(opts))


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def test_errors_change_nothing(make):
    from optimized_rag_amd import RagEngine, RagError
    st = RLive(make, 517, NO_FOLD, keep=False)                        # the option is off
    st.grow(40)
    ptr, terms, qd = _batch(st, SHIFT_QUERIES)
    before = outputs(st.eng, st, ptr, terms, qd)
    V = len(st.post.vocab)
    for call in (lambda: st.eng.bm25_refresh(), lambda: st.eng.bm25_live_counts(),
                 lambda: st.eng.bm25_set_statistics(np.ones(V), 3.0)):
        with pytest.raises(RagError, match=r"\(-3\).*bm25_keep_tf"):
            call()
    same_bits(before, outputs(st.eng, st, ptr, terms, qd))

    st = RLive(make, 519, NO_FOLD)
    st.grow(40)
    ptr, terms, qd = _batch(st, SHIFT_QUERIES)
    before = outputs(st.eng, st, ptr, terms, qd)
    s0 = st.eng.bm25_segment_stats()
    V = len(st.post.vocab)
    bad_idf = np.ones(V)
    bad_idf[V // 2] = np.nan
    for call in (lambda: st.eng.bm25_refresh(float("nan")), lambda: st.eng.bm25_refresh(float("inf")),
                 lambda: st.eng.bm25_set_statistics(np.ones(V), 0.0), lambda: st.eng.bm25_set_statistics(np.ones(V), -1.0),
                 lambda: st.eng.bm25_set_statistics(np.ones(V), float("nan")), lambda: st.eng.bm25_set_statistics(bad_idf, 3.0)):
        with pytest.raises(RagError, match=r"\(-1\)"):
            call()
    # a term frequency the uint16 plane cannot hold, at append and at load: refused, nothing changed
    sa = RLive(make, 520, NO_FOLD, dense=False)                       # (a standalone handle takes appends at any time)
    sa.grow(40)
    before_sa = outputs(sa.eng, sa, ptr, terms, None, dense=False)
    sa0 = sa.eng.bm25_segment_stats()
    blk = copy.deepcopy(sa.post).extend(["t1 t2 t2", "t3"])
    big = blk["tf"].copy()
    big[0] = 65536
    with pytest.raises(RagError, match=r"\(-1\).*65535"):
        sa.eng.bm25_append(blk["indptr"], blk["doc"], big, blk["doc_len"], blk["idf_new"], blk["n_terms_total"])
    assert sa.eng.bm25_segment_stats() == sa0
    same_bits(before_sa, outputs(sa.eng, sa, ptr, terms, None, dense=False))
    texts, e, ids, ten = st.new_rows(2)
    p = st.post
    big = p.tf.copy()
    big[len(big) // 2] = 65536
    with pytest.raises(RagError, match=r"\(-1\).*65535"):
        st.eng.bm25_load(p.indptr, p.doc, big, p.doc_len, p.idf, p.avgdl)
    assert st.eng.bm25_segment_stats() == s0
    same_bits(before, outputs(st.eng, st, ptr, terms, qd))
    # the postings are stale (rows without postings)
    st.insert(texts, e, ids, ten)
    for call in (lambda: st.eng.bm25_refresh(), lambda: st.eng.bm25_live_counts(), lambda: st.eng.bm25_set_statistics(np.ones(V), 3.0)):
        with pytest.raises(RagError, match=r"\(-3\).*stale"):
            call()
    st.post.append_to(st.eng, st.post.extend(texts))
    # nothing is live
    st.delete(np.arange(len(st.ids)))
    bm_only = lambda: {"scores": st.eng.bm25_scores(ptr, terms), **dict(zip("irsm", st.eng.bm25_topk(ptr, terms, 10)))}
    dead_out = bm_only()
    assert not dead_out["scores"].any() and (dead_out["r"] == -1).all()
    with pytest.raises(RagError, match=r"\(-3\).*no live"):
        st.eng.bm25_refresh()
    df, n, s = st.eng.bm25_live_counts()                              # the counts themselves are not an error: all zero
    assert not df.any() and (n, s) == (0, 0)
    same_bits(dead_out, bm_only())
    st.eng.close()
    # no postings at all
    e = RagEngine(dim=D, device=0)
    try:
        e.set_option("bm25_keep_tf", 1)
        with pytest.raises(RagError, match=r"\(-3\).*no postings"):
            e._check(e.lib.rag_bm25_refresh(e.h, 0.25, None, None), "rag_bm25_refresh")
    finally:
        e.close()


def test_tf_65535_fits(make):
    from optimized_rag_amd.bm25 import Bm25Postings
    e = make()
    e.set_option("bm25_keep_tf", 1)
    post = Bm25Postings.from_corpus(["a b", "a a c", "b c c d"])
    post.tf = post.tf.copy()
    post.tf[0] = 65535
    post.idf = np.ones_like(post.idf)
    post.load(e)
    idf, info = e.bm25_refresh()
    post.refresh()
    np.testing.assert_array_equal(_bits(idf), _bits(post.idf))
    ptr, terms = post.encode_queries(["a b c d"])
    np.testing.assert_array_equal(e.bm25_scores(ptr, terms)[0], O.bm25_scores_csr(post.indptr, post.doc, post.tf, post.doc_len, post.idf,
                                                                                 post.avgdl, terms))


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
def test_device_memory(make):
    import torch
    from optimized_rag_amd import RagEngine

    def run(keep):
        st = RLive(lambda dim=D: RagEngine(dim=dim, device=0), 521, NO_FOLD, keep=keep)
        try:
            st.grow(2048)
            st.delete(st.rng.choice(len(st.ids), 500, replace=False))
            qs, ptr, terms, qd = st.query_batch()
            outputs(st.eng, st, ptr, terms, qd)
            torch.cuda.synchronize()
            if keep:
                free0 = torch.cuda.mem_get_info()[0]
                st.eng.bm25_refresh()
                st.eng.bm25_live_counts()
                st.eng.bm25_set_statistics(st.post.idf, st.post.avgdl)
                assert torch.cuda.mem_get_info()[0] == free0          # the scratch is gone, nothing else was allocated
                outputs(st.eng, st, ptr, terms, qd)
        finally:
            st.eng.close()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    run(False)                                                        # torch's own caches reach their steady size
    assert run(True) == run(False)


# ---- 8 ---------------------------------------------------------------------------------------------------------------------
@BOTH
def test_option_on_without_a_refresh_changes_no_bit(make, opts):
    rng = np.random.default_rng(523)
    on, off = RLive(make, 523, opts), RLive(make, 523, opts, keep=False)
    for op in ("grow", "shift", "delete", "fold", "grow", "compact", "grow"):
        seed_ = int(rng.integers(1 << 30))
        for st in (on, off):
            _apply(st, np.random.default_rng(seed_), op, opts)
        qs, ptr, terms, qd = on.query_batch()
        off.query_batch()                                             # (keeps the two generators in step)
        for t in (-1, 2):
            same_bits(outputs(on.eng, on, ptr, terms, qd, t), outputs(off.eng, off, ptr, terms, qd, t))
    s_on, s_off = on.eng.bm25_segment_stats(), off.eng.bm25_segment_stats()
    assert s_on["tail_bytes"] > s_off["tail_bytes"] > 0               # the tail's tf plane is counted
    assert {k: v for k, v in s_on.items() if k != "tail_bytes"} == {k: v for k, v in s_off.items() if k != "tail_bytes"}


# ---- 9 ---------------------------------------------------------------------------------------------------------------------
def test_a_queued_device_search_sees_the_statistics_from_before(make):
    import torch
    st = RLive(make, 527, NO_FOLD)
    st.grow_with(_shift_texts(st.rng, 2500))
    ptr, terms, _ = _batch(st, SHIFT_QUERIES)
    Q, k = len(SHIFT_QUERIES), 10
    pd, td = _t(ptr), _t(terms)

    def call(s):
        outs = (torch.empty((Q, k), dtype=torch.int64, device="cuda"), torch.empty((Q, k), dtype=torch.int32, device="cuda"),
                torch.empty((Q, k), dtype=torch.float64, device="cuda"), torch.empty((Q,), dtype=torch.float64, device="cuda"))
        st.eng.bm25_topk_dev(pd, td, k, *outs, stream=s)
        return outs

    old = list(st.eng.bm25_topk(ptr, terms, k))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call(s)                                                       # first use of every workspace
        s.synchronize()
        T.busy(s)
        queued = [o.clone() for o in call(s)]
    assert not s.query()                                              # the search has not run yet
    st.refresh()
    with torch.cuda.stream(s):
        again = [o.clone() for o in call(s)]
    s.synchronize()
    new = list(st.eng.bm25_topk(ptr, terms, k))
    order = (0, 1, 2, 3)
    T.assert_same([x for x in T.to_np(queued)], [old[i] for i in order], "queued before the refresh")
    T.assert_same([x for x in T.to_np(again)], [new[i] for i in order], "after the refresh")
    assert (old[1] != new[1]).any()
    full_check(st)


# ---- 10 --------------------------------------------------------------------------------------------------------------------
def test_negative_mean(make):
    """Every term in every document: every raw idf is negative, so is their mean, so is every floored idf - all scores are
    negative and the linear fusion's emission bound rests on the recomputed negative-idf bound. 5000 rows: the thresholded
    stages of the fused dense search run. The oracle rebuilds BM25Okapi over the corpus (hybrid_search, bm25_scores)."""
    import torch
    from optimized_rag_amd.bm25 import Bm25Postings
    rng = np.random.default_rng(531)
    N, k = 5000, 25
    words = ["a", "b", "c", "d", "e"]
    corpus = [" ".join(rng.permutation(np.repeat(words, rng.integers(1, 5, 5)))) for _ in range(N)]
    emb = rng.standard_normal((N, D)).astype(np.float32)
    queries = ["a b", "c c e", "d", "e a b c d zzz"]
    q_emb = (emb[[7, 2500, 4100, 4999]] + 0.4 * rng.standard_normal((4, D))).astype(np.float32)
    post = Bm25Postings.from_corpus(corpus)
    ref_idf, ref_avgdl = post.idf.copy(), post.avgdl
    assert (ref_idf < 0).all() and post._frozen_mean < 0
    eng = make()
    eng.set_option("bm25_keep_tf", 1)
    eng.index_load(emb)
    eng.bm25_load(post.indptr, post.doc, post.tf, post.doc_len, np.full(5, 0.75), 2.0 * ref_avgdl)      # no negative idf at the load
    idf, info = eng.bm25_refresh()
    np.testing.assert_array_equal(_bits(idf), _bits(ref_idf))
    assert info["avgdl_after"] == ref_avgdl and info["negative_idf_terms"] == 5
    ptr, terms = post.encode_queries(queries)
    raw = eng.bm25_scores(ptr, terms)
    out = eng.hybrid_linear_dev(_t(q_emb), _t(ptr), _t(terms), k, 0.55, 0.35, 0.10)
    torch.cuda.synchronize()
    got = {key: v.cpu().numpy() for key, v in out.items()}
    for qi, query in enumerate(queries):
        kw = O.bm25_scores(query, corpus)
        assert max(kw) < 0
        assert raw[qi].tolist() == kw                                 # the maximum is not > 0: the divisor is 1.0
        idx, rows = O.hybrid_search(query, corpus, emb, q_emb[qi], top_k=k, bm25_available=True)
        assert got["rows"][qi].tolist() == idx, query
        assert got["keyword"][qi].tolist() == [r["keyword_score"] for r in rows]
        np.testing.assert_allclose(got["hybrid"][qi], [r["hybrid_score"] for r in rows], atol=1e-12)


def test_negative_idf_bound_follows_the_refresh(make):
    """The corpus and the queries of tests/test_dense_exactness_gpu.py::test_fused_bound_negative_bm25_scores_that_compete (raw
    scores ~1e-4 apart around -1250 competing with 0.01 * cosine), but loaded with POSITIVE statistics: the negative idf values
    arrive with the refresh, and the fused dense search keeps every row of the exact top-k only if the bound on a negative raw
    score (neg_idf_absmax) was recomputed from the new table."""
    from test_dense_exactness_gpu import _check_linear, _hybrid, _negative_idf_postings
    rng = np.random.default_rng(17)
    N, Dm, k, Q = 6000, 64, 25, 200
    a, b, g = 0.01, 1.0, 0.0
    emb = rng.standard_normal((N, Dm)).astype(np.float32)
    post = _negative_idf_postings(N, filler_words=1_000_000 + np.arange(N) // 40)
    terms = [0, 5] * 200
    q = rng.standard_normal((Q, Dm)).astype(np.float32)
    eng = make(Dm)
    eng.set_option("bm25_keep_tf", 1)
    eng.index_load(emb)
    eng.bm25_load(post.indptr, post.doc, post.tf, post.doc_len, np.ones(6), 1.0)
    idf, info = eng.bm25_refresh()
    np.testing.assert_array_equal(_bits(idf), _bits(post.idf))
    assert (idf < 0).all() and info["avgdl_after"] == post.avgdl and info["negative_idf_terms"] == 6
    raw = O.bm25_scores_csr(post.indptr, post.doc, post.tf, post.doc_len, post.idf, post.avgdl, terms)
    assert (raw <= 0).all() and np.abs(raw).max() > 1000
    sem = O.cosine_matrix(q, emb)
    hyb = (a * sem + b * (raw / 1.0)[None, :]) + g * 0.0
    got = _hybrid(eng, q, [terms] * Q, k, a, b, g)
    st = eng.dense_stats()
    assert st["proven_fast"] + st["proven_wide"] + st["exact_scan"] == Q and st["exact_scan"] == 0, st
    _check_linear(got, [(raw, raw / 1.0, hyb[qi], O.stable_topk_desc(hyb[qi], k + 1)) for qi in range(Q)], k)


def test_retrieve_rerank_candidates_after_a_refresh():
    """rag_retrieve_rerank_dev mode 1 (dense + BM25 + RRF candidates -> cross-encoder) after appends of another term
    distribution, deletes and a refresh: every output equals the fresh handle's, the candidates the oracle's RRF top-pool.
    Modelled on tests/test_bm25_live_gpu.py::test_retrieve_rerank_candidates_after_appends."""
    import torch
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.bm25 import Bm25Postings
    from optimized_rag_amd.cross_encoder import random_init_tensors
    rng = np.random.default_rng(541)
    Dm, Q, pool, k, Ld, Lq, L = 1536, 4, 10, 5, 24, 6, 32
    n_new = (1, 2100)
    N = N0 + sum(n_new)
    cfg = dict(vocab_size=3000, hidden=384, layers=2, heads=12, ffn=1536, max_pos=64, type_vocab=2, eps=1e-12)
    emb = rng.standard_normal((N, Dm)).astype(np.float32)
    tok = rng.integers(200, cfg["vocab_size"], (N, Ld)).astype(np.int32)
    tok_len = rng.integers(3, Ld + 1, N).astype(np.int32)
    dead = np.zeros(N, dtype=bool)
    dead[rng.integers(0, N, 700)] = True
    dead[N0 - 5:N0 + 5] = True
    live = np.nonzero(~dead)[0]
    pick = rng.choice(live[live >= N0 - 50], Q)
    q_emb = (emb[pick] + 0.5 * rng.standard_normal((Q, Dm))).astype(np.float32)
    q_tok, q_len = tok[pick, :Lq].copy(), np.minimum(tok_len[pick], Lq).astype(np.int32)
    corpus = [" ".join(f"t{t}" for t in tok[i, :tok_len[i]] % (50 if i < N0 else 12)) for i in range(N)]     # the tail: 12 terms only
    queries = [" ".join(f"t{t}" for t in q_tok[i, :q_len[i]] % 50) for i in range(Q)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    eng, fresh = RagEngine(dim=Dm, device=0), RagEngine(dim=Dm, device=0)
    try:
        eng.set_option("bm25_keep_tf", 1)
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
        assert eng.index_delete(np.nonzero(dead)[0].astype(np.int64)) == int(dead.sum())
        frozen = post.idf.copy()
        post.refresh_on(eng, live=~dead)
        assert np.abs(post.idf - frozen).max() > 0.5
        fresh.index_load(emb)
        fresh.tokens_load(tok, tok_len)
        fresh.ce_load(cfg, random_init_tensors(cfg, 3))
        fresh.bm25_load(post.indptr, post.doc, post.tf, post.doc_len, post.idf, post.avgdl)
        fresh.index_delete(np.nonzero(dead)[0].astype(np.int64))
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
    d_rows, _ = O.dense_topk(emb[live], q_emb, pool)
    for qi in range(Q):
        raw = O.bm25_scores_csr(post.indptr, post.doc, post.tf, post.doc_len, post.idf, post.avgdl, terms[ptr[qi]:ptr[qi + 1]])
        raw = np.where(dead, -np.inf, raw)
        b_rows = O.stable_topk_desc(raw, pool)
        okeys, _, _ = O.rrf_fuse([[int(live[r]) for r in d_rows[qi]], [int(r) for r in b_rows if np.isfinite(raw[r])]], k=60, top_k=pool)
        assert got[3][qi].tolist()[:len(okeys)] == okeys
