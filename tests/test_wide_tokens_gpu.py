"""GPU: the 24-bit passage token store (rag_tokens_load_wide_host, rag_tokens_reserve_wide, rag_tokens_info) through every place
rows live: the one-shot load, the device appends, live inserts past the reservation, deletes and both compactions, the pair
builder and the one-call pipeline. The store is only observable through the pair assembly, so every check reads it back with
rag_ce_build_pairs_dev and compares the int32 arrays exactly with the numpy builder of tests/xlmr_tools.py. Passage length 7
makes the byte plane's rows unaligned (7 B) and the uint16 plane's 14 B."""
import ctypes as C

import numpy as np
import pytest

import xlmr_tools as X
from oracle import bert_oracle as B

pytestmark = pytest.mark.gpu

RAG_ERR_ARG = -1
CLS, SEP = 101, 102
DIM = 64
ID_MAX = (1 << 24) - 1
EDGE_IDS = [65535, 65536, 70000, 250001, ID_MAX]


def _engine():
    from optimized_rag_amd import RagEngine
    return RagEngine(dim=DIM, device=0)


@pytest.fixture()
def eng():
    e = _engine()
    yield e
    e.close()


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _store(rng, n, L, hi):
    tok = rng.integers(0, hi, (n, L)).astype(np.int32)
    tok_len = rng.integers(0, L + 1, n).astype(np.int32)
    tok_len[:2] = [L, 0]
    tok_len[-1] = L
    return tok, tok_len


def _read_store(eng, n_rows, L):
    """the pair arrays of every row (and of -1 and two rows past the end) under an empty query, max_length L + 3: the whole passage"""
    cand = np.concatenate([np.arange(n_rows), [-1, n_rows, n_rows + 9]]).astype(np.int64).reshape(1, -1)
    return X.device_pairs(eng, np.zeros((1, 1), dtype=np.int32), np.zeros(1, dtype=np.int32), cand, max(8, L + 3), CLS, SEP)


def _expect_store(tok, tok_len):
    n, L = tok.shape
    cand = np.concatenate([np.arange(n), [-1, n, n + 9]]).astype(np.int64).reshape(1, -1)
    return X.build_pairs(np.zeros((1, 1), dtype=np.int32), np.zeros(1, dtype=np.int32), cand, tok, tok_len, max(8, L + 3), CLS, SEP)


def _assert_store(eng, tok, tok_len):
    for got, want in zip(_read_store(eng, tok.shape[0], tok.shape[1]), _expect_store(tok, tok_len)):
        np.testing.assert_array_equal(got, want)


def _append(eng, tok, tok_len, a, b):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(tok[a:b])).cuda()
    ln = torch.from_numpy(np.ascontiguousarray(tok_len[a:b])).cuda()
    rc = eng.lib.rag_tokens_append_dev(eng.h, C.c_void_p(t.data_ptr()), C.c_void_p(ln.data_ptr()), b - a, None)
    torch.cuda.synchronize()
    return rc


def test_wide_store_equals_narrow_store_on_ids_that_fit_16_bits():
    """The same tokens (all < 65536, L = 7) in a 16-bit and a 24-bit handle: equal pair arrays, and rag_retrieve_rerank_dev (modes 0
    and 1) returns the same ids, float64 score bits, float32 logit bits and candidate lists."""
    import torch
    from optimized_rag_amd.bm25 import Bm25Postings
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    rng = np.random.default_rng(41)
    N, L, Q, pool, k, Lq, Lp = 300, 7, 5, 8, 4, 6, 12
    cfg = dict(vocab_size=65536, hidden=128, layers=2, heads=4, ffn=512, max_pos=64, type_vocab=2, eps=1e-12)
    w = flatten_state_dict(B.seeded_weights(cfg, 3), cfg["layers"])
    emb = rng.standard_normal((N, DIM)).astype(np.float32)
    q_emb = (emb[rng.integers(0, N, Q)] + 0.5 * rng.standard_normal((Q, DIM))).astype(np.float32)
    tok, tok_len = _store(rng, N, L, 65536)
    tok[0, 0], tok[N - 1, L - 1] = 65535, 65535
    q_tok = rng.integers(200, 65536, (Q, Lq)).astype(np.int32)
    q_len = np.array([Lq, 0, 1, 3, Lq], dtype=np.int32)
    corpus = [" ".join(f"t{t % 40}" for t in tok[i, :tok_len[i]]) or "t0" for i in range(N)]
    queries = [" ".join(f"t{t % 40}" for t in q_tok[i, :max(1, q_len[i])]) for i in range(Q)]
    post = Bm25Postings.from_corpus(corpus)
    ptr, terms = post.encode_queries(queries)
    t = lambda a: torch.from_numpy(a).cuda()
    cand = np.concatenate([rng.integers(0, N, (Q, pool - 2)), np.full((Q, 1), -1), np.full((Q, 1), N - 1)], axis=1).astype(np.int64)
    out = {}
    for bits in (16, 24):
        e = _engine()
        try:
            e.index_load(emb)
            e.tokens_load(tok, tok_len, id_bits=bits)
            assert e.tokens_info() == {"rows": N, "L": L, "id_bits": bits}
            e.ce_load(cfg, w)
            post.load(e)
            res = [X.device_pairs(e, q_tok, q_len, cand, Lp, CLS, SEP)]
            for kw in ({}, dict(term_ptr=t(ptr), terms=t(terms))):
                r = e.retrieve_rerank_dev(t(q_emb), t(q_tok), t(q_len), pool, k, L_pair=Lp, cls_id=CLS, sep_id=SEP, **kw)
                torch.cuda.synchronize()
                res.append([x.cpu().numpy().copy() for x in r])
            out[bits] = res
        finally:
            e.close()
    for a, b in zip(out[16][0], X.build_pairs(q_tok, q_len, cand, tok, tok_len, Lp, CLS, SEP)):
        np.testing.assert_array_equal(a, b)
    for mode in (0, 1, 2):
        for a, b in zip(out[16][mode], out[24][mode]):
            assert a.dtype == b.dtype
            np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))                # bits, not values
    assert (out[24][1][0] >= 0).all() and (out[24][2][0] >= 0).all()


def test_the_range_of_a_wide_store_and_what_it_rejects(eng):
    """65535, 65536, 70000, 250001 and 16777215 in the first and last slot of the first and last row come back exactly; 16777216 and
    -1 are RAG_ERR_ARG at load, append and insert; a rejected append moves nothing and the next block is accepted; rag_tokens_info
    says 24, and 16 again after rag_tokens_load_host."""
    rng = np.random.default_rng(42)
    n, L = 6, 7
    emb = rng.standard_normal((n, DIM)).astype(np.float32)
    assert eng.tokens_info() == {"rows": 0, "L": 0, "id_bits": 0}
    for v in EDGE_IDS:
        tok, tok_len = _store(rng, n, L, ID_MAX + 1)
        tok[0, 0] = tok[0, L - 1] = tok[n - 1, 0] = tok[n - 1, L - 1] = v
        eng.tokens_load(tok, tok_len, id_bits=24)
        assert eng.tokens_info() == {"rows": n, "L": L, "id_bits": 24}
        _assert_store(eng, tok, tok_len)
    tok, tok_len = _store(rng, n, L, ID_MAX + 1)
    eng.tokens_load(tok, tok_len, id_bits=24)
    for bits in (8, 32, 0):
        assert eng.lib.rag_tokens_load_wide_host(eng.h, _p(tok), _p(tok_len), n, L, bits) == RAG_ERR_ARG
        assert eng.lib.rag_tokens_reserve_wide(eng.h, n, L, bits) == RAG_ERR_ARG
    _assert_store(eng, tok, tok_len)                                       # an unknown width is refused before anything is dropped
    for bad in (ID_MAX + 1, -1):
        for slot in ((0, 0), (n - 1, L - 1)):
            t2 = tok.copy()
            t2[slot] = bad
            # load
            assert eng.lib.rag_tokens_load_wide_host(eng.h, _p(t2), _p(tok_len), n, L, 24) == RAG_ERR_ARG
            assert b"[0, 16777215]" in eng.lib.rag_last_error(eng.h)
            # append: block 1 stays, the bad block 2 is rejected whole, the good block 2 is then taken
            eng.tokens_reserve(n, L, id_bits=24)
            assert eng.tokens_info() == {"rows": 0, "L": L, "id_bits": 24}
            assert _append(eng, tok, tok_len, 0, 2) == 0
            t3 = tok.copy()
            t3[2 + (slot[0] > 0) * (n - 3), slot[1]] = bad
            assert _append(eng, t3, tok_len, 2, n) == RAG_ERR_ARG
            assert b"[0, 16777215]" in eng.lib.rag_last_error(eng.h)
            assert eng.tokens_info()["rows"] == 2
            vis = tok_len.copy()
            vis[2:] = 0                                                    # rows not appended read as empty passages
            _assert_store(eng, tok, vis)
            assert _append(eng, tok, tok_len, 2, n) == 0
            assert eng.tokens_info()["rows"] == n
            _assert_store(eng, tok, tok_len)
            # insert: the index holds n rows with their store; a bad block changes nothing
            eng.index_load(emb)
            eng.tokens_load(tok, tok_len, id_bits=24)
            with pytest.raises(Exception, match=r"\[0, 16777215\]"):
                eng.index_insert(emb[:2], tokens=t2[[slot[0], 1]], token_lens=tok_len[:2])
            assert eng.tokens_info() == {"rows": n, "L": L, "id_bits": 24} and eng.n_rows == n
            _assert_store(eng, tok, tok_len)
    # the 16-bit calls stay 16 bits wide and replace the store
    narrow = np.minimum(tok, 65535)
    eng.tokens_load(narrow, tok_len)
    assert eng.tokens_info() == {"rows": n, "L": L, "id_bits": 16}
    _assert_store(eng, narrow, tok_len)
    assert eng.lib.rag_tokens_load_host(eng.h, _p(tok), _p(tok_len), n, L) == RAG_ERR_ARG                 # 65536 and above: still refused
    eng.tokens_reserve(n, L)
    assert eng.tokens_info() == {"rows": 0, "L": L, "id_bits": 16}
    eng.tokens_reserve(n, L, id_bits=24)
    assert eng.tokens_info()["id_bits"] == 24
    rows, bits = C.c_int64(-1), C.c_int(-1)
    assert eng.lib.rag_tokens_info(eng.h, C.byref(rows), None, C.byref(bits)) == 0 and (rows.value, bits.value) == (0, 24)
    assert eng.lib.rag_tokens_info(eng.h, None, None, None) == 0


def test_three_ways_in_give_one_store():
    """tokens_load(id_bits=24), reserve + two uneven device appends, and an empty reserved index filled by index_insert: identical
    pair arrays (ids past 65535 everywhere, L = 7)."""
    rng = np.random.default_rng(43)
    n, L = 211, 7
    emb = rng.standard_normal((n, DIM)).astype(np.float32)
    tok, tok_len = _store(rng, n, L, ID_MAX + 1)
    tok[5] = EDGE_IDS + [0, 1]
    want = _expect_store(tok, tok_len)
    got = []
    for way in range(3):
        e = _engine()
        try:
            if way == 0:
                e.tokens_load(tok, tok_len, id_bits=24)
            elif way == 1:
                e.tokens_reserve(n, L, id_bits=24)
                assert _append(e, tok, tok_len, 0, 3) == 0 and _append(e, tok, tok_len, 3, n) == 0
            else:
                e.index_reserve(n)
                e.tokens_reserve(n, L, id_bits=24)
                e.index_insert(emb[:130], tokens=tok[:130], token_lens=tok_len[:130])
                e.index_insert(emb[130:], tokens=tok[130:], token_lens=tok_len[130:])
            assert e.tokens_info() == {"rows": n, "L": L, "id_bits": 24}
            got.append(_read_store(e, n, L))
        finally:
            e.close()
    for g in got:
        for a, b in zip(g, want):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("keep_postings", [False, True], ids=["compact", "compact_bm25"])
@pytest.mark.parametrize("L", [7, 12])
def test_live_writes_move_both_planes(keep_postings, L):
    """Inserts past the reservation grow both planes; a scattered third of the rows (row 0 and the last among them) is deleted;
    rag_index_compact / rag_index_compact_bm25 move the byte plane (a row of 7 B goes through the byte gather, 12 B through the
    word one) with the rest: every surviving id's passage is what it was. A duplicate id changes nothing."""
    from optimized_rag_amd.bm25 import Bm25Postings
    rng = np.random.default_rng(44 + L)
    N0, NB, n = 260, 90, 350
    emb = rng.standard_normal((n, DIM)).astype(np.float32)
    tok, tok_len = _store(rng, n, L, ID_MAX + 1)
    tok[:, 0] = np.where(np.arange(n) % 3 == 0, ID_MAX - np.arange(n), tok[:, 0])         # a value per row that only both planes give
    ids = (5000 + rng.permutation(n)).astype(np.int64)
    e = _engine()
    try:
        e.index_load(emb[:N0], ids=ids[:N0])
        e.tokens_load(tok[:N0], tok_len[:N0], id_bits=24)                  # capacity = N0: the first insert grows both planes
        e.index_insert(emb[N0:N0 + NB - 1], ids=ids[N0:N0 + NB - 1], tokens=tok[N0:N0 + NB - 1], token_lens=tok_len[N0:N0 + NB - 1])
        e.index_insert(emb[n - 1:], ids=ids[n - 1:], tokens=tok[n - 1:], token_lens=tok_len[n - 1:])
        assert e.tokens_info() == {"rows": n, "L": L, "id_bits": 24}
        _assert_store(e, tok, tok_len)
        with pytest.raises(Exception, match="already live"):
            e.index_insert(emb[:2], ids=np.array([9, ids[17]], dtype=np.int64), tokens=tok[:2], token_lens=tok_len[:2])
        assert e.tokens_info() == {"rows": n, "L": L, "id_bits": 24} and e.n_rows == n
        _assert_store(e, tok, tok_len)
        if keep_postings:
            corpus = [" ".join(f"t{t % 30}" for t in tok[i]) for i in range(n)]
            Bm25Postings.from_corpus(corpus).load(e)
        dead = np.zeros(n, dtype=bool)
        dead[[0, n - 1]] = True
        dead[rng.choice(np.arange(1, n - 1), n // 3 - 2, replace=False)] = True
        assert e.index_delete(ids[dead]) == dead.sum()
        _assert_store(e, tok, tok_len)                                     # deleted rows stay in place until the compaction
        row_map = e.index_compact(keep_postings=keep_postings)
        live = np.flatnonzero(~dead)
        np.testing.assert_array_equal(row_map[live], np.arange(len(live)))
        assert (row_map[dead] == -1).all()
        assert e.tokens_info() == {"rows": len(live), "L": L, "id_bits": 24}
        _assert_store(e, tok[live], tok_len[live])
        # and the store still takes rows afterwards
        e.index_insert(emb[:1], ids=np.array([1], dtype=np.int64), tokens=tok[:1], token_lens=tok_len[:1])
        _assert_store(e, np.concatenate([tok[live], tok[:1]]), np.concatenate([tok_len[live], tok_len[:1]]))
    finally:
        e.close()


@pytest.mark.parametrize("hi,bits", [(250002, 24), (65536, 16)], ids=["wide", "narrow"])
def test_a_shard_loads_its_tokens_at_the_width_its_ids_need(tmp_path, hi, bits):
    """shard_format.load_shard_into(with_tokens=True): the store is reserved with the headroom at the width meta.json's token_id_max
    asks for, filled chunk by chunk (three appends here), and stays row-aligned with the index through a live insert."""
    from optimized_rag_amd import shard_format as SF
    rng = np.random.default_rng(45)
    n, L = 150, 7
    emb = rng.standard_normal((n + 1, DIM)).astype(np.float32)
    tok, tok_len = _store(rng, n + 1, L, hi)
    tok[n - 1, L - 1] = hi - 1
    w = SF.ShardWriter(str(tmp_path / "shard"), DIM)
    for i in range(n):
        w.add(100 + i, f"agent{i % 2}", f"text {i}", emb[i])
    w.close(build_bm25=False, tokens=tok[:n], token_lens=tok_len[:n])
    sh = SF.open_shard(str(tmp_path / "shard"))
    e = _engine()
    try:
        SF.load_shard_into(e, sh, chunk_rows=64, with_bm25=False, headroom_rows=4, with_tokens=True)
        assert e.tokens_info() == {"rows": n, "L": L, "id_bits": bits}
        _assert_store(e, tok[:n], tok_len[:n])
        e.index_insert(emb[n:], ids=np.array([7], dtype=np.int64), tenants=np.array([0], dtype=np.int32), tokens=tok[n:], token_lens=tok_len[n:])
        _assert_store(e, tok, tok_len)
    finally:
        e.close()
        sh.close()
