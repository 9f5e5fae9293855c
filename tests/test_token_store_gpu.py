"""GPU: the resident passage-token store (rag_tokens_load_host, rag_tokens_reserve, rag_tokens_append_dev) at its limits. The store
is only observable through the pair assembly, so every check reads it back with rag_ce_build_pairs_dev and compares the int32
pairs exactly with the oracle's assembly, as tests/test_property_gpu.py::test_pair_assembly_is_the_tokenizers_longest_first does.
Dropping `+ o` from `h->tok + o` in tokens_load_host (every staging piece then lands at the start of the store) fails
test_one_load_spanning_two_staging_pieces; before the counter of out-of-range ids was cleared on rejection,
test_a_rejected_append_does_not_poison_the_handle failed."""
import ctypes as C

import numpy as np
import pytest

from oracle import rag_oracle as O

pytestmark = pytest.mark.gpu

RAG_ERR_ARG = -1
CLS, SEP = 101, 102
DIM = 64


@pytest.fixture()
def eng():
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=DIM, device=0)
    yield e
    e.close()


def _tp(t):
    return C.c_void_p(t.data_ptr())


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _read_rows(eng, rows, L, n_visible):
    """What the store holds for `rows`, read through the pair assembly with an EMPTY query and max_length L + 3 (at most 512, which
    shows the first 509 tokens of a longer passage): [CLS] [SEP] passage [SEP]. Rows at or past n_visible (not appended yet) must
    read as empty passages. Returns the passages, one list per row."""
    import torch
    rows = np.asarray(rows, dtype=np.int64)
    P, Lp = len(rows), min(512, max(8, L + 3))
    ids = torch.full((P, Lp), -3, dtype=torch.int32, device="cuda")
    tt = torch.full((P, Lp), -3, dtype=torch.int32, device="cuda")
    lens = torch.full((P,), -3, dtype=torch.int32, device="cuda")
    q_tok = torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    q_len = torch.zeros((1,), dtype=torch.int32, device="cuda")
    eng.ce_build_pairs_dev(q_tok, q_len, torch.from_numpy(rows.reshape(1, P)).cuda(), ids, tt, lens)
    torch.cuda.synchronize()
    ids, tt, lens = ids.cpu().numpy(), tt.cpu().numpy(), lens.cpu().numpy()
    out = []
    for p in range(P):
        n = int(lens[p])
        assert ids[p, 0] == CLS and ids[p, 1] == SEP and ids[p, n - 1] == SEP and (ids[p, n:] == 0).all()
        assert tt[p].tolist() == [0, 0] + [1] * (n - 2) + [0] * (Lp - n)
        out.append(ids[p, 2:n - 1].tolist())
        if rows[p] >= n_visible or rows[p] < 0:
            assert n == 3
    return out


def _assert_store_equals(eng, tok, tok_len, n_visible=None):
    n, L = tok.shape
    n_visible = n if n_visible is None else n_visible
    got = _read_rows(eng, list(range(n)) + [-1, n, n + 5], L, n_visible)
    for r in range(n):
        assert got[r] == (tok[r, :min(tok_len[r], 509)].tolist() if r < n_visible else []), r
    assert got[n:] == [[], [], []]


def _assert_pairs_equal_oracle(eng, tok, tok_len, q_tok, q_len, cand, l_pair):
    """the full longest-first assembly against O.longest_first_lengths, as the existing pair-assembly property does"""
    import torch
    Q, pool = cand.shape
    ids = torch.zeros((Q * pool, l_pair), dtype=torch.int32, device="cuda")
    tt = torch.zeros_like(ids)
    lens = torch.zeros((Q * pool,), dtype=torch.int32, device="cuda")
    eng.ce_build_pairs_dev(torch.from_numpy(q_tok).cuda(), torch.from_numpy(q_len).cuda(), torch.from_numpy(cand).cuda(), ids, tt, lens)
    torch.cuda.synchronize()
    for qi in range(Q):
        for j in range(pool):
            r = int(cand[qi, j])
            ql, dl = O.longest_first_lengths(int(q_len[qi]), 0 if r < 0 else int(tok_len[r]), l_pair - 3)
            row = [CLS] + list(q_tok[qi, :ql]) + [SEP] + ([] if r < 0 else list(tok[r, :dl])) + [SEP]
            p = qi * pool + j
            assert int(lens[p]) == len(row)
            assert ids[p].tolist() == row + [0] * (l_pair - len(row))
            assert tt[p].tolist() == [0] * (ql + 2) + [1] * (len(row) - ql - 2) + [0] * (l_pair - len(row))


def _store(rng, n, L, hi=65536):
    tok = rng.integers(0, hi, (n, L)).astype(np.int32)
    tok_len = rng.integers(0, L + 1, n).astype(np.int32)
    tok_len[: min(n, 2)] = [L, 0][: min(n, 2)]
    return tok, tok_len


def _append(eng, tok, tok_len, a, b):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(tok[a:b])).cuda()
    ln = torch.from_numpy(np.ascontiguousarray(tok_len[a:b])).cuda()
    rc = eng.lib.rag_tokens_append_dev(eng.h, _tp(t) if b > a else None, _tp(ln) if b > a else None, b - a, None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("L", [1, 37, 512])
def test_appended_blocks_equal_the_one_shot_load(eng, L):
    """rag_tokens_reserve + uneven rag_tokens_append_dev blocks (one of zero rows, one of a single row) == one rag_tokens_load_host
    of the same rows; between two appends exactly the rows appended so far are visible."""
    rng = np.random.default_rng(L)
    n = 211
    tok, tok_len = _store(rng, n, L)
    q_tok = rng.integers(200, 5000, (3, 9)).astype(np.int32)
    q_len = np.array([9, 1, 4], dtype=np.int32)
    cand = rng.integers(-1, n, (3, 17)).astype(np.int64)
    eng.tokens_load(tok, tok_len)
    _assert_store_equals(eng, tok, tok_len)
    l_pair = min(512, max(8, L // 2 + 9))
    _assert_pairs_equal_oracle(eng, tok, tok_len, q_tok, q_len, cand, l_pair)
    eng.tokens_reserve(n, L)
    _assert_store_equals(eng, tok, tok_len, n_visible=0)
    cuts = [0, 1, 1, 64, 65, 200, 211]
    for a, b in zip(cuts, cuts[1:]):
        assert _append(eng, tok, tok_len, a, b) == 0
        _assert_store_equals(eng, tok, tok_len, n_visible=b)
    _assert_pairs_equal_oracle(eng, tok, tok_len, q_tok, q_len, cand, l_pair)


def test_search_between_appends_is_refused_until_the_store_is_as_long_as_the_index(eng):
    """rag_retrieve_rerank_dev refuses (RAG_ERR_ARG) while the store holds fewer rows than the index and runs once the last block is
    in; its result is the one the same handle gives after a one-shot load of the same rows."""
    import torch
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    from oracle import bert_oracle as B
    rng = np.random.default_rng(5)
    n, L = 90, 24
    cfg = dict(vocab_size=2000, hidden=384, layers=1, heads=12, ffn=1536, max_pos=64, type_vocab=2, eps=1e-12)
    eng.ce_load(cfg, flatten_state_dict(B.seeded_weights(cfg, 3), cfg["layers"]))
    corpus = rng.standard_normal((n, DIM)).astype(np.float32)
    eng.index_load(corpus)
    tok, tok_len = _store(rng, n, L, hi=2000)
    q_emb = torch.from_numpy(corpus[[3, 50]] + 0.1).cuda()
    q_tok = torch.from_numpy(rng.integers(5, 2000, (2, 6)).astype(np.int32)).cuda()
    q_len = torch.tensor([6, 2], dtype=torch.int32, device="cuda")

    def search():
        out = eng.retrieve_rerank_dev(q_emb, q_tok, q_len, 8, 4, L_pair=40)
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in out]

    eng.tokens_reserve(n, L)
    for a, b in [(0, 40), (40, 89)]:
        with pytest.raises(Exception, match=r"\(-1\)"):
            search()
        assert _append(eng, tok, tok_len, a, b) == 0
    with pytest.raises(Exception, match=r"\(-1\)"):
        search()                                                   # 89 of 90 rows
    assert _append(eng, tok, tok_len, 89, 90) == 0
    ids_a, sc_a, lg_a, cand_a = search()
    eng.tokens_load(tok, tok_len)
    ids_b, sc_b, lg_b, cand_b = search()
    assert (cand_a == cand_b).all() and (ids_a == ids_b).all() and (ids_a >= 0).all()
    assert np.allclose(lg_a, lg_b, rtol=0, atol=1e-5) and np.allclose(sc_a, sc_b, rtol=0, atol=1e-5)


def test_appends_outside_the_reservation_are_refused_and_change_nothing(eng):
    import torch
    rng = np.random.default_rng(9)
    n, L = 40, 16
    tok, tok_len = _store(rng, n, L)
    # before any reservation
    assert _append(eng, tok, tok_len, 0, 4) == RAG_ERR_ARG
    assert _append(eng, tok, tok_len, 0, 0) == RAG_ERR_ARG
    # L = 513: refused by both load paths, an existing store stays as it was
    eng.tokens_load(tok, tok_len)
    assert eng.lib.rag_tokens_reserve(eng.h, 10, 513) == RAG_ERR_ARG
    assert eng.lib.rag_tokens_reserve(eng.h, 0, 16) == RAG_ERR_ARG
    wide = np.zeros((2, 513), dtype=np.int32)
    assert eng.lib.rag_tokens_load_host(eng.h, _p(wide), _p(np.zeros(2, dtype=np.int32)), 2, 513) == RAG_ERR_ARG
    _assert_store_equals(eng, tok, tok_len)
    assert _append(eng, tok, tok_len, 0, 1) == RAG_ERR_ARG           # a loaded store is full: nothing can be appended to it
    _assert_store_equals(eng, tok, tok_len)
    # past the reservation: refused whole, the rows appended before stay, the remaining room can still be filled
    eng.tokens_reserve(n, L)
    assert _append(eng, tok, tok_len, 0, 30) == 0
    assert _append(eng, tok, tok_len, 29, 40) == RAG_ERR_ARG           # 11 rows into room for 10
    t = torch.zeros((1, L), dtype=torch.int32, device="cuda")
    assert eng.lib.rag_tokens_append_dev(eng.h, _tp(t), _tp(t), -1, None) == RAG_ERR_ARG
    _assert_store_equals(eng, tok, tok_len, n_visible=30)
    assert _append(eng, tok, tok_len, 30, 40) == 0
    assert _append(eng, tok, tok_len, 0, 1) == RAG_ERR_ARG
    _assert_store_equals(eng, tok, tok_len)


def test_token_ids_up_to_65535_and_the_rejection_of_wider_ones(eng):
    """The store is 16 bits wide: 65535 is accepted and comes back as 65535 (not -1, not 0); 65536 and -1 are rejected by
    rag_tokens_load_host and by rag_tokens_append_dev."""
    n, L = 6, 8
    tok = np.arange(n * L, dtype=np.int32).reshape(n, L) * 7
    tok[2, 3] = 65535
    tok[5, 7] = 65535
    tok[0, 0] = 65534
    tok_len = np.full(n, L, dtype=np.int32)
    eng.tokens_load(tok, tok_len)
    _assert_store_equals(eng, tok, tok_len)
    eng.tokens_reserve(n, L)
    assert _append(eng, tok, tok_len, 0, n) == 0
    _assert_store_equals(eng, tok, tok_len)
    for bad in (65536, -1, 2**31 - 1, -2**31, 65536 + 17):
        t2 = tok.copy()
        t2[4, 1] = bad
        assert eng.lib.rag_tokens_load_host(eng.h, _p(t2), _p(tok_len), n, L) == RAG_ERR_ARG, bad
        eng.tokens_reserve(n, L)
        assert _append(eng, t2, tok_len, 0, n) == RAG_ERR_ARG, bad
        _assert_store_equals(eng, tok, tok_len, n_visible=0)


def test_a_rejected_append_does_not_poison_the_handle(eng):
    """After an append that was rejected for an out-of-range id, a valid append of the same row range succeeds and the store
    equals the one built without the failed attempt; a second failure is still caught."""
    rng = np.random.default_rng(13)
    n, L = 50, 12
    tok, tok_len = _store(rng, n, L)
    bad = tok.copy()
    bad[25, 3] = 70000
    bad[31, 0] = -5
    eng.tokens_reserve(n, L)
    assert _append(eng, tok, tok_len, 0, 20) == 0
    assert _append(eng, bad, tok_len, 20, 35) == RAG_ERR_ARG
    _assert_store_equals(eng, tok, tok_len, n_visible=20)
    assert _append(eng, tok, tok_len, 20, 35) == 0                    # the same rows, now valid
    _assert_store_equals(eng, tok, tok_len, n_visible=35)
    assert _append(eng, bad, tok_len, 20, 35) == RAG_ERR_ARG           # (also past nothing: 35 + 15 = 50 fits, the ids are what is wrong)
    assert _append(eng, tok, tok_len, 35, 50) == 0
    _assert_store_equals(eng, tok, tok_len)


def test_one_load_spanning_two_staging_pieces(eng):
    """rag_tokens_load_host streams the int32 ids through a 64 Mi-token staging piece. 140,000 rows x 500 tokens = 70 M tokens is
    two pieces, the boundary falling inside row 134,217; row contents are a cheap function of (row, position). Checked: rows at the
    start, on both sides of and across the boundary, and the last rows. A rejected id in the SECOND piece is still caught."""
    n, L = 140_000, 500
    piece = 64 << 20
    assert n * L > piece and (piece // L) * L != piece
    r = np.arange(n, dtype=np.int32)[:, None]
    tok = r * 7919 + (r >> 9)                                         # < 2**31 for 140,000 rows
    tok = tok + np.arange(L, dtype=np.int32)[None, :] * 31
    tok &= 0xFFFF
    assert tok.dtype == np.int32 and tok.shape == (n, L) and tok.max() == 65535
    tok_len = ((r[:, 0] * 13) % (L + 1)).astype(np.int32)
    b = piece // L
    rows = [0, 1, 2, b - 2, b - 1, b, b + 1, b + 2, n - 2, n - 1]
    tok_len[rows] = L
    eng.tokens_load(tok, tok_len)
    got = _read_rows(eng, rows + [n, -1], L, n)
    for i, row in enumerate(rows):
        assert got[i] == tok[row].tolist(), row
    sample = list(range(5, n, 9973))
    got = _read_rows(eng, sample, L, n)
    for i, row in enumerate(sample):
        assert got[i] == tok[row, :tok_len[row]].tolist(), row
    tok[n - 1, L - 1] = 65536
    assert eng.lib.rag_tokens_load_host(eng.h, _p(tok), _p(tok_len), n, L) == RAG_ERR_ARG
