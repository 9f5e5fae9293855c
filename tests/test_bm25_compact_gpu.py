"""GPU: compaction that keeps the BM25 postings live (rag_index_compact_bm25, RagEngine.index_compact(keep_postings=True)).

The contract, checked by every scenario:
  1. after the call every BM25 / hybrid output is BIT-IDENTICAL to a fresh handle that holds the live rows in row order and was
     loaded with the compacted CSR (the host mirror, Bm25Postings.compacted) and the frozen statistics;
  2. that fresh load is what the oracle computes (check_oracle);
  3. the same handle returned the same doc ids and the same score bits immediately BEFORE the call, rows mapped through the
     returned row map (deletes already hid the rows).
Helpers and the 3000-row base (not a multiple of the 2048-document scoring range) come from tests/test_bm25_live_gpu.py."""
import numpy as np
import pytest

from oracle import rag_oracle as O
from test_bm25_live_gpu import D, N0, Live, check_oracle, full_check, outputs, same_bits

pytestmark = pytest.mark.gpu

TENANTS = (-1, 0, 2)
PACKED = (("bm25_packed", 1),)
NO_FOLD = (("bm25_tail_fold", -1),)


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


class CLive(Live):
    """Live whose compaction also filters texts / emb / ids / ten / dead through the row map and compacts the mirror.
    rare_rows: base rows that get the word `rare` (Live.queries asks for it), so that a base term can lose every posting."""

    def __init__(self, make, seed, opts=(), dense=True, rare_rows=()):
        super().__init__(make, seed, opts, dense)
        if len(rare_rows):                                          # the postings again, from the patched texts
            from optimized_rag_amd.bm25 import Bm25Postings
            for r in rare_rows:
                self.texts[r] = (self.texts[r] + " rare").strip()
            self.post = Bm25Postings.from_corpus(self.texts)
            self.V0 = len(self.post.vocab)
            self.post.load(self.eng)
        self.next_id = 500_000

    def new_rows(self, nb):
        """Live.new_rows numbers the new ids after the row count, which a compaction lowers: ids from a counter, never reused."""
        texts, e, _, ten = super().new_rows(nb)
        ids = np.arange(self.next_id, self.next_id + nb, dtype=np.int64)
        self.next_id += nb
        return texts, e, ids, ten

    def compact(self, keep=True):
        row_map = self.eng.index_compact(keep_postings=keep)
        live = row_map >= 0
        np.testing.assert_array_equal(live, ~self.dead)
        np.testing.assert_array_equal(row_map[live], np.arange(int(live.sum())))
        self.post.compacted(row_map[:self.post.n_docs])             # the mirror covers the rows whose postings were appended
        self.texts = [t for t, l in zip(self.texts, live) if l]
        self.emb, self.ids, self.ten = self.emb[live], self.ids[live], self.ten[live]
        self.dead = np.zeros(len(self.ids), dtype=bool)
        assert self.eng.n_rows == len(self.ids)
        return row_map

    def query_batch(self):
        qs = self.queries()
        ptr, terms = self.post.encode_queries(qs)
        n = len(self.ids)
        qd = _t((self.emb[self.rng.integers(0, n, len(qs))] + 0.5 * self.rng.standard_normal((len(qs), D))).astype(np.float32))
        return qs, ptr, terms, qd

    def check_stats(self):
        s = self.eng.bm25_segment_stats()
        assert s["base_docs"] + s["tail_docs"] == self.post.n_docs
        assert s["base_nnz"] + s["tail_nnz"] == int(self.post.indptr[-1])
        assert s["n_terms"] == len(self.post.vocab)
        return s


def _bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else (a.view(np.int32) if a.dtype == np.float32 else a)


def same_through_map(before, after, row_map):
    """check 3: ids and score bits as before the call, rows through the row map, all-document scores at the live rows."""
    live = row_map >= 0
    for k in (10, 100):
        for pre in ("topk", "dev"):
            for what in ("ids", "sc", "max"):
                name = f"{pre}{k}_{what}"
                np.testing.assert_array_equal(_bits(after[name]), _bits(before[name]), err_msg=name)
            rows = before[f"{pre}{k}_rows"]
            mapped = np.where(rows >= 0, row_map[np.maximum(rows, 0)], -1).astype(np.int32)
            np.testing.assert_array_equal(after[f"{pre}{k}_rows"], mapped, err_msg=f"{pre}{k}_rows")
    assert after["scores"].shape == (before["scores"].shape[0], int(live.sum()))
    np.testing.assert_array_equal(_bits(after["scores"]), _bits(np.ascontiguousarray(before["scores"][:, live])))
    for name in ("rrf_keys", "rrf_sc"):
        np.testing.assert_array_equal(_bits(after[name]), _bits(before[name]), err_msg=name)


def compact_and_check(st, fresh_opts=(), normalize=True):
    """The three checks around one compaction with keep_postings, for every tenant."""
    qs, ptr, terms, qd = st.query_batch()
    before = {t: outputs(st.eng, st, ptr, terms, qd, t) for t in TENANTS}
    appends = st.eng.bm25_segment_stats()["appends"]
    row_map = st.compact()
    s = st.check_stats()
    assert s["appends"] == appends                                # the counter survives
    for t in TENANTS:
        same_through_map(before[t], outputs(st.eng, st, ptr, terms, qd, t), row_map)
        full_check(st, tenant=t, fresh_opts=fresh_opts, normalize=normalize)
    return row_map


def test_base_only(make):
    rare = (17, 2047, 2999)
    st = CLive(make, 301, rare_rows=rare)
    t_rare = st.post.vocab["rare"]
    assert st.post.indptr[t_rare + 1] - st.post.indptr[t_rare] == 3
    # scattered rows, rows of the boundary range (2048 .. 2999), the only documents of a rare term
    rows = np.unique(np.concatenate([st.rng.integers(0, N0, 350), np.arange(2040, 2060), np.arange(2990, N0), np.array(rare)]))
    st.delete(rows)
    full_check(st)
    s0 = st.eng.bm25_segment_stats()
    compact_and_check(st)
    s1 = st.eng.bm25_segment_stats()
    assert s1["base_docs"] == N0 - len(rows) and s1["tail_docs"] == 0 and s1["folds"] == 0 and s1["base_nnz"] < s0["base_nnz"]
    # the rare term kept its number and its idf and has an empty list: a query for it scores like an unknown word
    assert st.post.vocab["rare"] == t_rare and st.post.indptr[t_rare + 1] == st.post.indptr[t_rare]
    ptr, terms = st.post.encode_queries(["rare", "zzz-unknown"])
    assert terms.tolist() == [t_rare, -1]
    ids, rws, sc, mx = st.eng.bm25_topk(ptr, terms, 10)
    assert not sc.any() and (mx == 1.0).all()
    np.testing.assert_array_equal(rws[0], rws[1])
    np.testing.assert_array_equal(ids[0], ids[1])
    assert not st.eng.bm25_scores(ptr, terms).any()
    # one whole 2048-document range goes: what was the boundary range becomes range 0
    st.delete(np.arange(0, 2048))
    compact_and_check(st)
    assert st.eng.bm25_segment_stats()["base_docs"] == N0 - len(rows) - 2048
    st.grow(9)                                                    # and the postings take appends again
    full_check(st)


def _delete_in_both(st):
    n = len(st.ids)
    base = st.eng.bm25_segment_stats()["base_docs"]
    rows = np.unique(np.concatenate([st.rng.integers(0, base, 400), st.rng.integers(base, n, 300), np.arange(2040, 2060),
                                     np.arange(base - 5, base + 5)]))
    ptr, terms = st.post.encode_queries(["rare", "n3 n7 n3"])    # the best hits of the tail-only queries go too
    for qi in range(2):
        rows = np.union1d(rows, O.stable_topk_desc(st.raw(terms[ptr[qi]:ptr[qi + 1]]), 3))
    rows = rows[~st.dead[rows]]
    st.delete(rows)
    return rows


def test_base_and_tail(make):
    st = CLive(make, 307, NO_FOLD)
    for nb in (7, 2048):
        st.grow(nb)
    _delete_in_both(st)
    compact_and_check(st)
    s = st.eng.bm25_segment_stats()
    assert s["tail_docs"] > 0 and s["base_docs"] < N0 and s["folds"] == 0 and s["appends"] == 2      # remapped separately, no fold
    assert s["tail_bytes"] > 0
    st.grow(7)                                                    # appends go on behind the remapped tail
    st.grow(2048)
    assert st.eng.bm25_segment_stats()["appends"] == 4
    full_check(st)
    full_check(st, tenant=2)
    _delete_in_both(st)
    compact_and_check(st)                                         # a second compaction, on remapped postings
    qs, ptr, terms, qd = st.query_batch()
    before = outputs(st.eng, st, ptr, terms, qd)
    s0 = st.eng.bm25_segment_stats()
    st.eng.bm25_fold()
    s1 = st.check_stats()
    assert s1["tail_docs"] == 0 and s1["folds"] == 1 and s1["base_nnz"] == s0["base_nnz"] + s0["tail_nnz"]
    same_bits(before, outputs(st.eng, st, ptr, terms, qd))
    full_check(st, tenant=0)


def test_packed_base_with_a_tail(make):
    from optimized_rag_amd import RagError
    st = CLive(make, 311, PACKED)
    for nb in (7, 2048):
        st.grow(nb)
    _delete_in_both(st)
    compact_and_check(st, fresh_opts=PACKED)
    full_check(st)                                                # and against an UNPACKED load of the compacted CSR
    s = st.eng.bm25_segment_stats()
    assert s["tail_docs"] > 0 and s["folds"] == 0
    with pytest.raises(RagError, match="packed"):                 # the base is still the packed one
        st.eng.bm25_fold()
    st.grow(30)
    _delete_in_both(st)
    compact_and_check(st, fresh_opts=PACKED)


@pytest.mark.parametrize("opts", [NO_FOLD, PACKED], ids=["plain", "packed"])
def test_every_base_row_deleted(make, opts):
    st = CLive(make, 313, opts)
    for nb in (7, 300):
        st.grow(nb)
    rows = np.concatenate([np.arange(N0), N0 + st.rng.choice(307, 40, replace=False)])
    st.delete(rows)
    compact_and_check(st)
    s = st.eng.bm25_segment_stats()
    assert s["base_docs"] + s["tail_docs"] == 267 and s["appends"] == 2
    st.grow(5)
    full_check(st)
    full_check(st, tenant=2)


def test_every_tail_row_deleted(make):
    """The tail has no survivor and is dropped: a base alone, whose own term count stays below the vocabulary the tail brought."""
    st = CLive(make, 359, NO_FOLD)
    for nb in (7, 300):
        st.grow(nb)
    assert len(st.post.vocab) > st.V0                             # the tail brought terms of its own
    rows = np.concatenate([np.arange(N0, N0 + 307), st.rng.choice(N0, 200, replace=False), np.arange(2040, 2060)])
    st.delete(np.unique(rows))
    compact_and_check(st)
    s = st.eng.bm25_segment_stats()
    assert s["tail_docs"] == 0 and s["tail_nnz"] == 0 and s["tail_bytes"] == 0 and s["base_docs"] == len(st.ids)
    assert s["appends"] == 2 and s["folds"] == 0
    ptr, terms = st.post.encode_queries(["n3 n7 n3"])            # tail-only terms: known, with empty lists
    assert (terms >= st.V0).all()
    assert not st.eng.bm25_topk(ptr, terms, 10)[2].any()
    st.grow(40)                                                   # a new tail behind the base
    for t in TENANTS:
        full_check(st, tenant=t)


def test_every_covered_row_deleted(make):
    """No covered row survives: there is nothing to keep, the call ends like the plain compaction and only a reload helps."""
    from optimized_rag_amd import RagError
    st = CLive(make, 367, NO_FOLD)
    st.grow(40)
    texts, e, ids, ten = st.new_rows(300)
    st.insert(texts, e, ids, ten)                                 # 300 rows without postings: the only rows that stay
    st.delete(np.arange(N0 + 40))
    s0 = st.eng.bm25_segment_stats()
    row_map = st.compact()
    np.testing.assert_array_equal(row_map[N0 + 40:], np.arange(300))
    assert st.post.n_docs == 0 and st.eng.n_rows == 300
    assert st.eng.bm25_segment_stats() == s0                      # the old postings, left alone and unusable
    ptr, terms = st.post.encode_queries(["t1 t2 t3"])
    with pytest.raises(RagError, match="stale"):
        st.eng.bm25_topk(ptr, terms, 10)
    st.post.extend(st.texts)
    st.post.load(st.eng)                                          # frozen statistics, the 300 rows' postings
    st.check_stats()
    for t in TENANTS:
        full_check(st, tenant=t)
    st.grow(3)
    st.delete(np.array([1]))
    compact_and_check(st)                                         # and from there on the new call keeps them live


def test_uncovered_rows_stay_stale_until_appended(make):
    from optimized_rag_amd import RagError
    st = CLive(make, 317)
    st.grow(40)
    texts, e, ids, ten = st.new_rows(5)
    st.insert(texts, e, ids, ten)                                 # 5 rows without postings
    n = len(st.ids)
    st.delete(np.unique(np.concatenate([st.rng.integers(0, N0 + 40, 200), np.array([N0 + 3, n - 4])])))     # one of the 5 too
    st.compact()
    s = st.check_stats()
    assert s["base_docs"] + s["tail_docs"] == len(st.ids) - 4
    ptr, terms = st.post.encode_queries(["t1 t2 t3"])
    with pytest.raises(RagError, match="stale"):
        st.eng.bm25_topk(ptr, terms, 10)
    with pytest.raises(RagError, match="stale"):
        st.eng.hybrid_rrf_dev(_t(st.emb[:1]), _t(ptr), _t(terms), 40, 20)
    rest = st.texts[st.post.n_docs:]
    assert len(rest) == 4
    st.post.append_to(st.eng, st.post.extend(rest[:1]))
    with pytest.raises(RagError, match="stale"):
        st.eng.bm25_topk(ptr, terms, 10)
    st.post.append_to(st.eng, st.post.extend(rest[1:]))
    st.check_stats()
    for t in TENANTS:
        full_check(st, tenant=t)


def test_after_a_plain_compaction_only_a_reload_helps(make):
    from optimized_rag_amd import RagError
    st = CLive(make, 331)
    st.grow(30)
    st.delete(np.array([3, 2050, N0 + 4]))
    st.compact(keep=False)                                        # the old symbol: stale and compacted
    ptr, terms = st.post.encode_queries(["t1 t2 t3"])
    with pytest.raises(RagError, match="stale"):
        st.eng.bm25_topk(ptr, terms, 10)
    s0 = st.eng.bm25_segment_stats()
    st.delete(np.array([5, 2051]))
    st.compact(keep=True)
    with pytest.raises(RagError, match="stale"):
        st.eng.bm25_topk(ptr, terms, 10)
    assert st.eng.bm25_segment_stats() == s0                      # postings that describe other rows are left alone
    st.post.load(st.eng)                                          # the compacted mirror, frozen statistics
    for t in TENANTS:
        full_check(st, tenant=t)
    st.delete(np.array([7]))                                      # and from there on the new call keeps them live
    compact_and_check(st)


def test_nothing_deleted_is_the_identity(make):
    st = CLive(make, 337)
    st.grow(7)
    qs, ptr, terms, qd = st.query_batch()
    before = outputs(st.eng, st, ptr, terms, qd)
    s0 = st.eng.bm25_segment_stats()
    assert st.eng.index_delete(np.array([-5, 123_456_789])) == 0
    row_map = st.eng.index_compact(keep_postings=True)
    np.testing.assert_array_equal(row_map, np.arange(N0 + 7))
    assert st.eng.bm25_segment_stats() == s0
    same_bits(before, outputs(st.eng, st, ptr, terms, qd))
    texts, e, ids, ten = st.new_rows(2)                           # stale postings stay stale through the identity
    st.insert(texts, e, ids, ten)
    from optimized_rag_amd import RagError
    st.eng.index_compact(keep_postings=True)
    with pytest.raises(RagError, match="stale"):
        st.eng.bm25_topk(ptr, terms, 10)
    st.post.append_to(st.eng, st.post.extend(texts))
    full_check(st)


def test_raw_mode(make):
    st = CLive(make, 347, NO_FOLD)
    st.eng.bm25_set_normalize(False)
    st.grow(300)
    rows = _delete_in_both(st)
    n_before = len(st.ids)
    compact_and_check(st, normalize=False)
    ptr, terms = st.post.encode_queries(["t1 t2", "n3"])
    sc = st.eng.bm25_scores(ptr, terms)
    assert sc.shape == (2, n_before - len(rows)) and len(st.ids) == n_before - len(rows)
    _, _, top, mx = st.eng.bm25_topk(ptr, terms, 10)
    assert top[0, 0] == mx[0]                                     # still raw after the call: the best score IS the maximum
    st.eng.bm25_set_normalize(True)
    full_check(st)


def test_device_memory_is_released(make):
    import torch
    st = CLive(make, 349, NO_FOLD)
    st.grow(2048)
    qs, ptr, terms, qd = st.query_batch()
    outputs(st.eng, st, ptr, terms, qd)                           # the search workspaces exist
    n = len(st.ids)
    st.delete(st.rng.choice(n, n // 3, replace=False))
    outputs(st.eng, st, ptr, terms, qd)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    st.compact()
    free1 = torch.cuda.mem_get_info()[0]
    assert free1 >= free0, (free0, free1)                         # staging, masks and the old postings are gone
    full_check(st)


def test_retrieve_rerank_candidates_after_a_compaction():
    """rag_retrieve_rerank_dev mode 1 (dense + BM25 + RRF candidates -> cross-encoder) with a token store, modelled on
    tests/test_bm25_live_gpu.py::test_retrieve_rerank_candidates_after_appends: the token plane moves in the same call."""
    import torch
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.bm25 import Bm25Postings
    from optimized_rag_amd.cross_encoder import random_init_tensors
    rng = np.random.default_rng(353)
    Dm, Q, pool, k, Ld, Lq, L = 1536, 4, 10, 5, 24, 6, 32
    n_new = (1, 2100)
    N = N0 + sum(n_new)
    cfg = dict(vocab_size=3000, hidden=384, layers=2, heads=12, ffn=1536, max_pos=64, type_vocab=2, eps=1e-12)
    emb = rng.standard_normal((N, Dm)).astype(np.float32)
    tok = rng.integers(200, cfg["vocab_size"], (N, Ld)).astype(np.int32)
    tok_len = rng.integers(3, Ld + 1, N).astype(np.int32)
    dead = np.zeros(N, dtype=bool)
    dead[rng.integers(0, N, 900)] = True
    dead[2040:2060] = True
    dead[N0 - 5:N0 + 5] = True
    live = np.nonzero(~dead)[0]
    pick = rng.choice(live[live >= N0 - 50], Q)                  # queries near the boundary range and in the tail
    q_emb = (emb[pick] + 0.5 * rng.standard_normal((Q, Dm))).astype(np.float32)
    q_tok, q_len = tok[pick, :Lq].copy(), np.minimum(tok_len[pick], Lq).astype(np.int32)
    corpus = [" ".join(f"t{t}" for t in tok[i, :tok_len[i]] % (50 if i < N0 else 70)) for i in range(N)]
    queries = [" ".join(f"t{t}" for t in q_tok[i, :q_len[i]] % 70) for i in range(Q)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    eng, fresh = RagEngine(dim=Dm, device=0), RagEngine(dim=Dm, device=0)
    try:
        post = Bm25Postings.from_corpus(corpus[:N0])
        eng.index_load(emb[:N0])                                  # implicit ids: id = row, stored by the compaction
        eng.tokens_load(tok[:N0], tok_len[:N0])
        eng.ce_load(cfg, random_init_tensors(cfg, 3))
        post.load(eng)
        a = N0
        for nb in n_new:
            eng.index_insert(emb[a:a + nb], tokens=tok[a:a + nb], token_lens=tok_len[a:a + nb])
            post.append_to(eng, post.extend(corpus[a:a + nb]))
            a += nb
        assert eng.index_delete(np.nonzero(dead)[0].astype(np.int64)) == int(dead.sum())
        row_map = eng.index_compact(keep_postings=True)
        np.testing.assert_array_equal(row_map >= 0, ~dead)
        post.compacted(row_map)
        s = eng.bm25_segment_stats()
        assert s["base_docs"] + s["tail_docs"] == len(live) and s["base_nnz"] + s["tail_nnz"] == int(post.indptr[-1])
        fresh.index_load(emb[live], ids=live.astype(np.int64))
        fresh.tokens_load(tok[live], tok_len[live])
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
        np.testing.assert_array_equal(_bits(x), _bits(y))
    d_rows, _ = O.dense_topk(emb[live], q_emb, pool)
    for qi in range(Q):
        raw = O.bm25_scores_csr(post.indptr, post.doc, post.tf, post.doc_len, post.idf, post.avgdl, terms[ptr[qi]:ptr[qi + 1]])
        okeys, _, _ = O.rrf_fuse([[int(live[r]) for r in d_rows[qi]], [int(live[r]) for r in O.stable_topk_desc(raw, pool)]], k=60, top_k=pool)
        assert got[3][qi].tolist()[:len(okeys)] == okeys


@pytest.mark.parametrize("seq", range(20))
def test_seeded_random_sequences(make, seq):
    rng = np.random.default_rng(9000 + seq)
    opts = (NO_FOLD, PACKED, (("bm25_tail_fold", 64),), ())[seq % 4]
    st = CLive(make, 400 + seq, opts)
    try:
        for step in range(6):
            op = ("grow", "delete", "compact")[step % 3] if step < 3 else rng.choice(["grow", "delete", "compact"])
            if op == "grow":
                st.grow(int(rng.choice([1, 5, 40, 300])))
            elif op == "delete":
                lv = np.nonzero(~st.dead)[0]
                st.delete(rng.choice(lv, int(rng.integers(1, max(2, len(lv) // 4))), replace=False))
            else:
                st.compact()
                st.check_stats()
            qs, ptr, terms, qd = st.query_batch()
            tenant = TENANTS[int(rng.integers(0, 3))]
            got = outputs(st.eng, st, ptr, terms, qd, tenant)
            f = st.fresh(PACKED if opts is PACKED else ())
            same_bits(got, outputs(f, st, ptr, terms, qd, tenant))
            f.close()
        check_oracle(st, got, ptr, terms, qd, tenant)
    finally:
        st.eng.close()
