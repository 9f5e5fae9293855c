"""GPU: the resident token-vector store (rag_tokvec_*) and the late-interaction rerank over it (tokvec_maxsim_kernel, the raw top-k,
rag_retrieve_maxsim_dev) against the float64 reference of tests/tokvec_tools.py.

Bars (include/rag_hip.h): (a) |score - float64 MaxSim over the STORED fp16 rows| < 1e-4 (query split 2^-22 relative + fp32
accumulation over <= 1024 terms, 1024 * 2^-24 = 6.1e-5: the bar of rag_maxsim_*); (b) |score - float64 MaxSim over the ORIGINAL
float32 unit rows| < 1e-3 (fp16 rounding moves a dot of unit vectors by <= 2^-11 = 4.9e-4, subnormals 2^-25 * sqrt(dim), a mean
of maxima is 1-Lipschitz: <= 5.9e-4 with (a)). Everything else - the stored bits, the slot rules, the selection, determinism, the
composite against the separate calls, stream order - is bit-exact.
Measured on an MI355X, (a) / (b) at dim 32, 96, 128, 1024: 5.0e-8 / 8.6e-5, 3.1e-8 / 3.6e-5, 3.7e-8 / 4.5e-5, 4.3e-8 / 1.2e-5."""
import numpy as np
import pytest

import m3_tools as M
import sparse_tools as S
import stream_tools as T
import tokvec_tools as V

pytestmark = pytest.mark.gpu

D_ROWS = [0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257]          # 8 tiles = the 2-tile groups, 9 and 17 = the 4-tile groups
Q_ROWS = [0, 1, 16, 17, 32, 33, 65]
ERR_ARG, ERR_STATE = r"\(-1\)", r"\(-3\)"


@pytest.fixture(scope="module")
def eng():
    """a handle WITHOUT a dense index: ids are row numbers"""
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=64, device=0)
    yield e
    e.close()


def _pack_unit(rng, counts, dim):
    return M.pack([V.unit_rows(rng, n, dim) for n in counts], dim)


def _fetch_all(e):
    info = e.tokvec_info()
    docs = [e.tokvec_fetch(i) for i in range(info["n_docs"])]
    return M.pack(docs, info["dim"])


def _rerank_dev(e, q, qo, cand, k, stream=None, rows=True, pairs=True):
    import torch
    Q, pool = cand.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ids = torch.full((Q, k), -7, dtype=torch.int64, device="cuda")
    rw = torch.full((Q, k), -7, dtype=torch.int32, device="cuda") if rows else None
    sc = torch.full((Q, k), float("nan"), dtype=torch.float64, device="cuda")
    ps = torch.full((Q, pool), float("nan"), dtype=torch.float32, device="cuda") if pairs else None
    qd = t(q) if q.shape[0] else torch.zeros((1, q.shape[1]), device="cuda")
    e.tokvec_rerank_dev(qd, t(qo), t(cand.astype(np.int32)), k, ids, rw, sc, ps, stream=stream)
    torch.cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in (ids, rw, sc, ps))


# ---- the store -------------------------------------------------------------------------------------------------------------------
def test_fetch_is_numpy_fp16_rounding_and_info():
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=64, device=0)
    try:
        assert e.tokvec_info() == {"n_docs": 0, "rows": 0, "dim": 0, "hbm_bytes": 0}
        rng = np.random.default_rng(0)
        dim, counts = 96, [3, 0, 0, 17, 1, 0, 40, 0]
        n = sum(counts)
        v = rng.standard_normal((n, dim)).astype(np.float32)
        v[0] *= 1e-6                                                     # fp16 subnormals and underflow to zero
        v[1] *= 1e-4
        v[2] = np.float32(1.0) + np.float32(2.0 ** -11) * rng.integers(0, 4, dim).astype(np.float32)      # exact halfway cases: ties to even
        v[3] = 60000.0 * rng.choice([-1.0, 1.0], dim)                   # near the top of the range, still finite
        v[4, :8] = [0.0, -0.0, 65504.0, -65504.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 65519.0]
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        e.tokvec_load(v, off)
        info = e.tokvec_info()
        assert info == {"n_docs": len(counts), "rows": n, "dim": dim, "hbm_bytes": n * dim * 2 + (len(counts) + 1) * 8}
        exp = V.fp16_round(v)
        for i, c in enumerate(counts):
            got = e.tokvec_fetch(i)
            assert got.shape == (c, dim) and got.dtype == np.float32
            np.testing.assert_array_equal(got.view(np.uint32), exp[off[i]:off[i + 1]].view(np.uint32))
        # a store that holds nothing but empty documents, and a second load replacing the first
        e.tokvec_load(np.zeros((0, 32), dtype=np.float32), np.zeros(4, dtype=np.int64))
        assert e.tokvec_info()["n_docs"] == 3 and e.tokvec_info()["rows"] == 0 and e.tokvec_info()["dim"] == 32
        assert e.tokvec_fetch(2).shape == (0, 32)
        ids, rows, sc, ps = e.tokvec_rerank(np.ones((2, 32), np.float32), [0, 2], [[0, 1, 2, 3]], 4)
        assert (ids == -1).all() and (rows == -1).all() and (sc == 0).all() and (ps == 0).all()
    finally:
        e.close()


def test_load_and_chunked_appends_give_the_same_store(eng):
    import torch
    from optimized_rag_amd import RagEngine
    rng = np.random.default_rng(1)
    dim, counts = 64, [5, 0, 33, 1, 0, 64, 7, 2, 0, 19]
    v, off = M.pack([rng.standard_normal((c, dim)).astype(np.float32) for c in counts], dim)
    eng.tokvec_load(v, off)
    ref_v, ref_off = _fetch_all(eng)
    np.testing.assert_array_equal(ref_off, off)
    np.testing.assert_array_equal(ref_v, V.fp16_round(v))
    other = RagEngine(dim=64, device=0)
    try:
        other.tokvec_reserve(len(counts) + 3, off[-1] + 10, dim)
        other.tokvec_append(v, off[0:4])                                 # host block: documents 0-2
        vd, od = torch.from_numpy(v).cuda(), torch.from_numpy(off).cuda()
        other.tokvec_append_dev(vd, od[3:8].contiguous())               # device block with offsets that do not start at 0: documents 3-6
        other.tokvec_append(v, off[7:9])                                 # one document
        other.tokvec_append_dev(vd, od[8:].contiguous())
        other.tokvec_append(v, off[5:6])                                 # a block of no documents is legal and changes nothing
        assert other.tokvec_info()["n_docs"] == len(counts) and other.tokvec_info()["rows"] == off[-1]
        got_v, got_off = _fetch_all(other)
        np.testing.assert_array_equal(got_off, off)
        np.testing.assert_array_equal(got_v.view(np.uint32), ref_v.view(np.uint32))
    finally:
        other.close()


def test_append_of_embed_multi_dev_outputs_as_they_are():
    import torch
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    from oracle import bert_oracle as B
    cfg = dict(vocab_size=500, hidden=128, layers=2, heads=2, ffn=256, max_pos=128, type_vocab=2, eps=1e-12)
    e = RagEngine(dim=128, device=0)
    try:
        e.embed_load(cfg, flatten_state_dict(B.seeded_weights(cfg, 51), cfg["layers"], head=False), normalize=True, pooling="cls")
        e.embed_heads_load(**M.seeded_heads(128, 32, 9))
        rng = np.random.default_rng(2)
        lens = np.array([1, 2, 17, 64, 33, 5], dtype=np.int32)
        ids = rng.integers(5, 500, (6, 64)).astype(np.int32)
        tok = torch.full((int((lens - 1).sum()), 32), float("nan"), device="cuda")
        off = torch.full((7,), -7, dtype=torch.int64, device="cuda")
        e.embed_multi_dev(torch.from_numpy(ids).cuda(), torch.zeros((6, 64), dtype=torch.int32, device="cuda"), torch.from_numpy(lens).cuda(),
                          tok=tok, row_off=off)
        e.tokvec_reserve(12, 2 * tok.shape[0], 32)
        e.tokvec_append_dev(tok, off)
        e.tokvec_append_dev(tok, off)                                    # the same forward's outputs behind themselves
        h_tok, h_off = tok.cpu().numpy(), off.cpu().numpy()
        np.testing.assert_array_equal(h_off, np.concatenate([[0], np.cumsum(lens - 1)]))
        got_v, got_off = _fetch_all(e)
        np.testing.assert_array_equal(got_off, np.concatenate([h_off, h_off[-1] + h_off[1:]]))
        np.testing.assert_array_equal(got_v, np.concatenate([V.fp16_round(h_tok)] * 2))
        e.tokvec_load(h_tok, h_off)
        got2, _ = _fetch_all(e)
        np.testing.assert_array_equal(got2, got_v[:h_tok.shape[0]])
    finally:
        e.close()


def test_every_rejection_leaves_the_counts_and_the_block_can_be_retried():
    import torch
    from optimized_rag_amd import RagEngine, RagError
    e = RagEngine(dim=64, device=0)
    try:
        rng = np.random.default_rng(3)
        dim = 32
        good = rng.standard_normal((10, dim)).astype(np.float32)
        off = np.array([0, 4, 4, 10], dtype=np.int64)
        with pytest.raises(RagError, match=ERR_ARG):
            e.tokvec_append(good, off)                                   # before a reserve
        for bad_dim in (0, 16, 48, 1056):
            with pytest.raises(RagError, match=ERR_ARG):
                e.tokvec_reserve(4, 10, bad_dim)
        e.tokvec_reserve(4, 16, dim)
        e.tokvec_append(good[:4], [0, 4])
        state = e.tokvec_info()
        assert state["n_docs"] == 1 and state["rows"] == 4

        def dev(v, o):
            e.tokvec_append_dev(torch.from_numpy(np.ascontiguousarray(v)).cuda(), torch.from_numpy(np.asarray(o, dtype=np.int64)).cuda())

        def host(v, o):
            e.tokvec_append(v, o)

        nan, inf, big = good.copy(), good.copy(), good.copy()
        nan[9, 31] = np.nan
        inf[0, 0] = -np.inf
        big[5, 7] = 1.0e5                                                # finite as float32, not as fp16
        for put in (host, dev):
            for v, o in ((good, [0, 1, 2, 3, 10]),                       # past the reserved documents
                         (np.concatenate([good, good]), [0, 13]),        # past the reserved rows
                         (good, [0, 6, 5, 10]),                          # a decreasing offset inside the block
                         (good, [4, 2]),                                 # ... and at its ends
                         (nan, off), (inf, off), (big, off)):
                with pytest.raises(RagError, match=ERR_ARG):
                    put(v, o)
                assert e.tokvec_info() == state
                np.testing.assert_array_equal(e.tokvec_fetch(0), V.fp16_round(good[:4]))
            # the block that was rejected for its values goes in once they are finite
            put(good, off)
            assert e.tokvec_info()["n_docs"] == 4 and e.tokvec_info()["rows"] == 14
            got_v, got_off = _fetch_all(e)
            np.testing.assert_array_equal(got_off, [0, 4, 8, 8, 14])
            np.testing.assert_array_equal(got_v, V.fp16_round(np.concatenate([good[:4], good])))
            e.tokvec_reserve(4, 16, dim)                                 # a reserve replaces the store
            assert e.tokvec_info()["n_docs"] == 0
            e.tokvec_append(good[:4], [0, 4])
    finally:
        e.close()


# ---- scores ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [32, 96, 128, 1024])
def test_scores_against_float64_over_stored_and_original_vectors(eng, dim):
    rng = np.random.default_rng(dim)
    d, d_off = _pack_unit(rng, D_ROWS, dim)
    q, q_off = _pack_unit(rng, Q_ROWS, dim)
    eng.tokvec_load(d, d_off)
    stored, _ = _fetch_all(eng)
    np.testing.assert_array_equal(stored, V.fp16_round(d))
    cand = np.tile(np.arange(len(D_ROWS), dtype=np.int32), (len(Q_ROWS), 1))
    k = len(D_ROWS)
    ids, rows, sc, ps = _rerank_dev(eng, q, q_off, cand, k)
    empty = V.slot_empty(q_off, d_off, cand)
    assert ps.dtype == np.float32 and (ps[empty] == 0).all() and empty[0].all() and empty[:, 0].all() and not empty[1:, 1:].any()
    exp_a = V.pair_scores(q, q_off, stored, d_off, cand)
    exp_b = V.pair_scores(q, q_off, d, d_off, cand)
    err_a, err_b = float(np.abs(ps - exp_a).max()), float(np.abs(ps - exp_b).max())
    print(f"tokvec rerank dim {dim}: max |score - float64 over the stored rows| = {err_a:.3e}, over the original rows = {err_b:.3e}")
    assert err_a < 1e-4
    assert err_b < 1e-3
    # the lists: the stable top-k of the device's own scores; no index on this handle: ids are the rows
    e_ids, e_rows, e_sc = V.stable_topk(ps, cand, empty, k)
    np.testing.assert_array_equal(rows, e_rows)
    np.testing.assert_array_equal(ids, e_rows.astype(np.int64))
    np.testing.assert_array_equal(V.bits(sc), V.bits(e_sc))
    # the host form gives the device form's bits
    h_ids, h_rows, h_sc, h_ps = eng.tokvec_rerank(q, q_off, cand, k)
    for a, b in ((h_ids, ids), (h_rows, rows), (V.bits(h_sc), V.bits(sc)), (h_ps.view(np.uint32), ps.view(np.uint32))):
        np.testing.assert_array_equal(a, b)


def test_negative_maxima_and_exact_powers_of_two(eng):
    rng = np.random.default_rng(4)
    # every similarity negative: a zero-filled tile tail or an unmasked pad row would give a maximum >= 0 or too high
    dim = 96
    u = M.normalize(rng.standard_normal((1, dim)))
    qs = [M.normalize(u + 0.05 * rng.standard_normal((n, dim))).astype(np.float32) for n in (17, 5, 33)]
    ds = [M.normalize(-u + 0.05 * rng.standard_normal((n, dim))).astype(np.float32) for n in (1, 17, 33, 129, 145)]
    q, qo = M.pack(qs, dim)
    d, do = M.pack(ds, dim)
    eng.tokvec_load(d, do)
    cand = np.tile(np.arange(5, dtype=np.int32), (3, 1))
    _, _, _, ps = _rerank_dev(eng, q, qo, cand, 5)
    exp = V.pair_scores(q, qo, V.fp16_round(d), do, cand)
    assert (exp < -0.5).all() and (ps < 0).all() and np.abs(ps - exp).max() < 1e-4
    # entries in {0, +-2^-k}: exact as fp16, every product and sum exact in float32 and float64 alike, so a score is the float32
    # rounding of the exact value - a wrong row, a wrong k slice or a pad row in a maximum changes it
    dim = 64

    def sparse_rows(n):
        a = np.zeros((n, dim), dtype=np.float32)
        for r in range(n):
            cols = rng.choice(dim, 4, replace=False)
            a[r, cols] = rng.choice([-1.0, 1.0], 4) * 2.0 ** -rng.integers(1, 6, 4)
        return a

    counts_q, counts_d = [1, 16, 17, 33, 40], [1, 15, 17, 32, 70, 130, 257]
    q, qo = M.pack([sparse_rows(n) for n in counts_q], dim)
    d, do = M.pack([sparse_rows(n) for n in counts_d], dim)
    eng.tokvec_load(d, do)
    np.testing.assert_array_equal(_fetch_all(eng)[0], d)
    cand = np.tile(np.arange(len(counts_d), dtype=np.int32), (len(counts_q), 1))
    _, _, _, ps = _rerank_dev(eng, q, qo, cand, 1)
    exp = V.pair_scores(q, qo, d, do, cand).astype(np.float32)
    np.testing.assert_array_equal(ps.view(np.uint32), exp.view(np.uint32))


def test_a_pairs_bits_do_not_depend_on_pool_slot_neighbours_or_run(eng):
    rng = np.random.default_rng(6)
    dim = 128
    counts = (D_ROWS * 3)[:30]
    d, do = _pack_unit(rng, counts, dim)
    eng.tokvec_load(d, do)
    q, qo = _pack_unit(rng, [9, 33, 17], dim)
    target = 11                                                          # a 257-row document; query 1 (33 rows)
    one_q, one_off = q[qo[1]:qo[2]], np.array([0, 33], dtype=np.int64)
    alone = _rerank_dev(eng, one_q, one_off, np.array([[target]], dtype=np.int32), 1)
    assert alone[3][0, 0] != 0 and alone[1][0, 0] == target
    cand = rng.integers(-1, len(counts) + 2, (3, 256)).astype(np.int32)
    cand[1, 77] = target
    cand[1, 200] = target
    cand[2, 0] = 8                                                       # a 127-row document for the 2-tile groups
    big = _rerank_dev(eng, q, qo, cand, 256)
    again = _rerank_dev(eng, q, qo, cand, 256)
    for a, b in zip(big, again):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    bits = alone[3].view(np.uint32)[0, 0]
    assert big[3].view(np.uint32)[1, 77] == bits and big[3].view(np.uint32)[1, 200] == bits
    short = _rerank_dev(eng, q[qo[2]:qo[3]], np.array([0, 17], dtype=np.int64), np.array([[3, 8]], dtype=np.int32), 2)
    assert short[3].view(np.uint32)[0, 1] == big[3].view(np.uint32)[2, 0]
    for qi in range(3):                                                  # every slot of the big call, against the reference
        same = cand[qi] == target
        assert len(set(big[3].view(np.uint32)[qi][same].tolist())) <= 1


# ---- selection -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def idx():
    """a handle WITH a dense index of 40 rows (dim 64)"""
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=64, device=0)
    yield e
    e.close()


def test_selection_is_the_stable_topk_of_the_devices_own_scores(idx):
    rng = np.random.default_rng(7)
    dim, n_idx = 32, 40
    counts = [int(c) for c in rng.integers(1, 20, 36)]                   # the store holds 36 of the index's 40 rows
    counts[5] = 0
    d, do = _pack_unit(rng, counts, dim)
    emb = rng.standard_normal((n_idx, 64)).astype(np.float32)
    explicit = (9000 - 7 * np.arange(n_idx)).astype(np.int64)
    q, qo = _pack_unit(rng, [4, 0, 9, 2], dim)
    pool = 24
    cand = rng.integers(0, 36, (4, pool)).astype(np.int32)
    cand[0, [3, 10, 11]] = -1                                            # empty slots in the middle
    cand[0, 5] = 36                                                      # rows past the store: inside the index, and beyond everything
    cand[0, 6] = 2 ** 30
    cand[0, 7] = 5                                                       # a document without rows
    cand[0, 15] = cand[0, 14] = cand[0, 2] = 9                           # duplicated candidates: equal scores keep candidate order
    cand[2] = -1                                                         # an all-empty query by its candidates; query 1 by its rows
    cand[3, :] = 12
    for ids_arg, id_base in ((explicit, 0), (None, 1000)):
        idx.index_load(emb, ids=ids_arg, id_base=id_base)
        idx.tokvec_load(d, do)
        for k in (1, 5, pool):
            ids, rows, sc, ps = _rerank_dev(idx, q, qo, cand, k)
            empty = V.slot_empty(qo, do, cand)
            assert empty[1].all() and empty[2].all() and empty[0, [3, 5, 6, 7, 10, 11]].all() and (ps[empty] == 0).all()
            assert np.abs(ps - V.pair_scores(q, qo, V.fp16_round(d), do, cand)).max() < 1e-4
            e_ids, e_rows, e_sc = V.stable_topk(ps, cand, empty, k, idmap=ids_arg, id_base=id_base)
            np.testing.assert_array_equal(rows, e_rows)
            np.testing.assert_array_equal(ids, e_ids)
            np.testing.assert_array_equal(V.bits(sc), V.bits(e_sc))
            assert (rows[1] == -1).all() and (ids[2] == -1).all() and (sc[1] == 0).all()
            if k == pool:
                assert (rows[3] == 12).all() and 0 < (rows[0] >= 0).sum() == (~empty[0]).sum() <= pool - 6
                dup = np.nonzero(rows[0] == 9)[0]
                assert dup.shape[0] >= 3 and (np.diff(dup) == 1).all() and len(set(V.bits(sc[0][dup]).tolist())) == 1
            # outputs that may be NULL
            ids2, none_rows, sc2, none_ps = _rerank_dev(idx, q, qo, cand, k, rows=False, pairs=False)
            assert none_rows is None and none_ps is None
            np.testing.assert_array_equal(ids2, ids)
            np.testing.assert_array_equal(V.bits(sc2), V.bits(sc))
    # a store ahead of the index (rows 30 - 35 are not in it yet): those rows are scored and returned, their ids are -1
    cand[0, 1], cand[3, 2] = 33, 35
    for ids_arg, id_base in ((explicit[:30], 0), (None, 1000)):
        idx.index_load(emb[:30], ids=ids_arg, id_base=id_base)
        ids, rows, sc, ps = _rerank_dev(idx, q, qo, cand, pool)
        empty = V.slot_empty(qo, do, cand)
        e_ids, e_rows, e_sc = V.stable_topk(ps, cand, empty, pool, idmap=ids_arg, id_base=id_base, n_index=30)
        np.testing.assert_array_equal(rows, e_rows)
        np.testing.assert_array_equal(ids, e_ids)
        assert ((rows >= 30) == ((ids == -1) & (rows >= 0))).all() and (rows >= 30).any() and (ids[rows >= 0][rows[rows >= 0] < 30] >= 0).all()
    from optimized_rag_amd import RagError
    with pytest.raises(RagError, match="dim"):                           # query vectors narrower than the store: refused before any read
        idx.tokvec_rerank(np.ones((4, 16), np.float32), [0, 1, 2, 3, 4], cand, 2)
    with pytest.raises(RagError, match="past"):                          # offsets that end past the query rows
        idx.tokvec_rerank(q, qo + 1, cand, 2)
    for bad_k, bad_pool in ((0, 8), (9, 8), (1, 257)):
        with pytest.raises(RagError, match=ERR_ARG):
            _rerank_dev(idx, q, qo, np.zeros((4, bad_pool), dtype=np.int32), bad_k)


# ---- the composite ---------------------------------------------------------------------------------------------------------------
N_DOCS, DIM, TOK_DIM, POOL, K = 600, 64, 64, 50, 10
_WORLD = {}


def world():
    if not _WORLD:
        rng = np.random.default_rng(8)
        indptr, doc, w = S.make_corpus(n_docs=N_DOCS, n_terms=3000, seed=5)
        queries = S.make_queries(indptr, seed=6)
        emb = rng.standard_normal((N_DOCS, DIM)).astype(np.float32)
        q_emb = (emb[rng.integers(0, N_DOCS, len(queries))] + 0.7 * rng.standard_normal((len(queries), DIM))).astype(np.float32)
        counts = [int(c) for c in rng.integers(0, 40, N_DOCS)]
        vecs = [V.unit_rows(rng, c, TOK_DIM) for c in counts]
        q_counts = [int(c) for c in rng.integers(1, 34, len(queries))]
        q_counts[3] = 0
        qv, qo = _pack_unit(rng, q_counts, TOK_DIM)
        _WORLD.update(indptr=indptr, doc=doc, w=w, packed=S.pack_queries(queries), emb=emb, q_emb=q_emb, vecs=vecs, qv=qv, qo=qo,
                      ids=(5000 + 3 * np.arange(N_DOCS)).astype(np.int64), tenants=(np.arange(N_DOCS) % 3).astype(np.int32))
    return _WORLD


def _load_world(e, keep=None, tenants=True, headroom=0):
    """the world's rows `keep` (all: None) on handle e, in row order: index with explicit ids, tenants, sparse postings, token vectors"""
    w = world()
    keep = np.arange(N_DOCS) if keep is None else np.asarray(keep)
    e.index_load(w["emb"][keep], ids=w["ids"][keep])
    if tenants:
        e.set_tenants(w["tenants"][keep])
    remap = np.full(N_DOCS, -1, dtype=np.int64)
    remap[keep] = np.arange(keep.shape[0])
    term_of = np.repeat(np.arange(w["indptr"].shape[0] - 1, dtype=np.int64), np.diff(w["indptr"]))
    sel = remap[w["doc"]] >= 0
    indptr = np.zeros_like(w["indptr"])
    np.cumsum(np.bincount(term_of[sel], minlength=indptr.shape[0] - 1), out=indptr[1:])
    e.sparse_load(indptr, remap[w["doc"][sel]].astype(np.int32), w["w"][sel], keep.shape[0])
    v, off = M.pack([w["vecs"][i] for i in keep], TOK_DIM)
    e.tokvec_reserve(keep.shape[0] + headroom, off[-1] + 64 * headroom, TOK_DIM)
    e.tokvec_append(v, off)


def _composite(e, mode, tenant=-1, stream=None, dev=None, pool=POOL, k=K):
    import torch
    w = world()
    if dev is None:
        ptr, terms, wts = w["packed"]
        dev = T.to_dev(dict(q_emb=w["q_emb"], qv=w["qv"], qo=w["qo"], ptr=ptr, terms=terms, w=wts))
    sparse = dict(term_ptr=dev["ptr"], terms=dev["terms"], weights=dev["w"]) if mode == 1 else {}
    ids, sc, cand = e.retrieve_maxsim_dev(dev["q_emb"], dev["qv"], dev["qo"], pool, k, tenant=tenant, stream=stream, **sparse)
    if stream is None:
        torch.cuda.synchronize()
    return [ids.clone(), sc.clone(), cand.clone()]


def _separate(e, mode, tenant=-1, pool=POOL, k=K):
    """the existing search entry followed by rag_tokvec_rerank_dev on its rows -> (ids, scores, candidate ids)"""
    import torch
    w = world()
    ptr, terms, wts = w["packed"]
    d = T.to_dev(dict(q_emb=w["q_emb"], qv=w["qv"], qo=w["qo"], ptr=ptr, terms=terms, w=wts))
    Q = w["q_emb"].shape[0]
    if mode == 0:
        c_ids = torch.empty((Q, pool), dtype=torch.int64, device="cuda")
        c_rows = torch.empty((Q, pool), dtype=torch.int32, device="cuda")
        e.dense_topk_dev(d["q_emb"], pool, c_ids, c_rows, torch.empty((Q, pool), dtype=torch.float64, device="cuda"), tenant=tenant)
    else:
        keys, _, _ = e.hybrid_sparse_rrf_dev(d["q_emb"], d["ptr"], d["terms"], d["w"], pool, pool, tenant=tenant)
        c_ids = keys.clone()
        c_rows = torch.where(c_ids >= 0, (c_ids - 5000) // 3, c_ids).to(torch.int32)      # the world's ids back to rows of the FULL load
    ids = torch.empty((Q, k), dtype=torch.int64, device="cuda")
    sc = torch.empty((Q, k), dtype=torch.float64, device="cuda")
    e.tokvec_rerank_dev(d["qv"], d["qo"], c_rows.contiguous(), k, ids, None, sc)
    torch.cuda.synchronize()
    return [ids, sc, c_ids]


def _same(got, exp, what):
    g, x = T.to_np(got), T.to_np(exp)
    np.testing.assert_array_equal(g[0], x[0], err_msg=what + ": ids")
    np.testing.assert_array_equal(V.bits(g[1]), V.bits(x[1]), err_msg=what + ": score bits")
    np.testing.assert_array_equal(g[2], x[2], err_msg=what + ": candidates")


@pytest.fixture(scope="module")
def full():
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=DIM, device=0)
    _load_world(e)
    yield e
    e.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_composite_is_the_search_entry_followed_by_the_rerank(full, mode):
    w = world()
    got = _composite(full, mode)
    _same(got, _separate(full, mode), f"mode {mode}")
    ids, sc, cand = T.to_np(got)
    assert (ids[:, 0] >= 0).sum() >= 30 and (ids[3] == -1).all() and (sc[3] == 0).all()         # query 3 has no token vectors
    # against the float64 reference: scores of the returned ids over the stored rows
    row_of = lambda i: (int(i) - 5000) // 3
    for qi in (0, 7, 31):
        vq = w["qv"][w["qo"][qi]:w["qo"][qi + 1]]
        for i, s in zip(ids[qi], sc[qi]):
            if i >= 0:
                assert abs(s - M.maxsim(vq, V.fp16_round(w["vecs"][row_of(i)]))) < 1e-4
        live = [s for i, s in zip(ids[qi], sc[qi]) if i >= 0]
        assert live == sorted(live, reverse=True) and set(ids[qi][ids[qi] >= 0]) <= set(cand[qi])


def test_composite_limits_and_missing_pieces(full):
    from optimized_rag_amd import RagEngine, RagError
    for pool, k in ((POOL, 0), (8, 9), (257, 10)):
        with pytest.raises(RagError, match=ERR_ARG):
            _composite(full, 0, pool=pool, k=k)
    full.set_tenants(None)
    with pytest.raises(RagError, match=ERR_ARG):                         # a tenant filter without a tenant table
        _composite(full, 0, tenant=1)
    full.set_tenants(world()["tenants"])
    e = RagEngine(dim=DIM, device=0)
    try:
        e.index_load(world()["emb"])
        with pytest.raises(RagError, match=ERR_STATE):                   # no store
            _composite(e, 0)
        e.tokvec_load(*M.pack(world()["vecs"][:10], TOK_DIM))
        with pytest.raises(RagError, match=ERR_STATE):                   # a store of 10 documents beside 600 rows
            _composite(e, 0)
    finally:
        e.close()


def test_tenant_filter_deletes_compaction_and_inserts():
    from optimized_rag_amd import RagEngine, RagError
    w = world()
    a, b = RagEngine(dim=DIM, device=0), RagEngine(dim=DIM, device=0)
    try:
        _load_world(a)
        base0 = _composite(a, 0)
        deleted = np.unique(T.to_np(base0)[0][:, :3].reshape(-1))       # the best hits of every query
        deleted = deleted[deleted >= 0]
        assert a.index_delete(deleted) == deleted.shape[0] > 20
        dead_rows = (deleted - 5000) // 3
        live = np.setdiff1d(np.arange(N_DOCS), dead_rows)
        # deletes need nothing: against a fresh handle holding only the live rows (of the tenant, for the filtered call)
        for tenant in (-1, 1):
            keep = live if tenant < 0 else live[w["tenants"][live] == tenant]
            _load_world(b, keep, tenants=False)
            for mode in (0, 1):
                got, exp = _composite(a, mode, tenant=tenant), _composite(b, mode)
                _same(got, exp, f"tenant {tenant} mode {mode} against the live rows")
                assert not np.isin(T.to_np(got)[0], deleted).any()
        # a compaction moves rows: stale until a reload; the handle stays usable
        row_map = a.index_compact()
        assert (row_map >= 0).sum() == live.shape[0] and a.tokvec_info()["n_docs"] == N_DOCS
        with pytest.raises(RagError, match=ERR_STATE):
            _composite(a, 0)
        with pytest.raises(RagError, match=ERR_STATE):
            _rerank_dev(a, w["qv"], w["qo"], np.zeros((len(w["qo"]) - 1, 4), dtype=np.int32), 2)
        with pytest.raises(RagError, match=ERR_STATE):
            a.tokvec_rerank(w["qv"], w["qo"], np.zeros((len(w["qo"]) - 1, 4), dtype=np.int32), 2)
        assert a.dense_topk(w["q_emb"], 5)[0].shape == (len(w["qo"]) - 1, 5)
        v, off = M.pack([w["vecs"][i] for i in live], TOK_DIM)
        a.tokvec_reserve(live.shape[0] + 2, off[-1] + 80, TOK_DIM)      # headroom for the two rows inserted below
        a.tokvec_append(v, off)
        _load_world(b, live[w["tenants"][live] == 1], tenants=False)
        _same(_composite(a, 0, tenant=1), _composite(b, 0), "after the compaction and the reload")
        a.index_compact()                                                # nothing deleted: nothing moves, nothing is marked
        _same(_composite(a, 0, tenant=1), _composite(b, 0), "after a compaction without deleted rows")
        # an insert leaves the store alone: the composite waits for the new rows' vectors, the explicit-row entry does not
        rng = np.random.default_rng(9)
        new_emb = w["q_emb"][:2] * 1.0
        a.index_insert(new_emb, ids=np.array([1, 2], dtype=np.int64), tenants=np.array([1, 1], dtype=np.int32))
        with pytest.raises(RagError, match=ERR_STATE):
            _composite(a, 0)
        assert _rerank_dev(a, w["qv"], w["qo"], np.zeros((len(w["qo"]) - 1, 4), dtype=np.int32), 2)[0].shape[1] == 2
        new_vecs = [V.unit_rows(rng, 40, TOK_DIM), w["qv"][w["qo"][1]:w["qo"][2]]]
        a.tokvec_append(new_vecs[0], [0, 40])
        with pytest.raises(RagError, match=ERR_STATE):                   # one of the two rows covered
            _composite(a, 0)
        a.tokvec_append(new_vecs[1], [0, new_vecs[1].shape[0]])
        ids, sc, cand = T.to_np(_composite(a, 0, tenant=1))
        # query 1 finds its own token vectors in the inserted row 2 (dense cosine 1, MaxSim 1 up to fp16 storage)
        assert ids[1, 0] == 2 and abs(sc[1, 0] - 1.0) < 1e-3 and 1 in cand[0]
    finally:
        a.close()
        b.close()


# ---- stream order ----------------------------------------------------------------------------------------------------------------
def test_rerank_dev_is_ordered_on_its_stream(full):
    import torch
    w = world()
    rng = np.random.default_rng(10)
    Q = len(w["qo"]) - 1
    cand = rng.integers(-1, N_DOCS, (Q, 64)).astype(np.int32)

    def call(d, s):
        ids = torch.empty((Q, 8), dtype=torch.int64, device="cuda")
        rows = torch.empty((Q, 8), dtype=torch.int32, device="cuda")
        sc = torch.empty((Q, 8), dtype=torch.float64, device="cuda")
        ps = torch.empty((Q, 64), dtype=torch.float32, device="cuda")
        full.tokvec_rerank_dev(d["qv"], d["qo"], d["cand"], 8, ids, rows, sc, ps, stream=s)
        return [ids, rows, sc, ps]

    wrong = dict(qv=np.zeros_like(w["qv"]), qo=np.zeros_like(w["qo"]), cand=np.full_like(cand, -1))      # legal: nothing to score
    real = dict(qv=w["qv"], qo=w["qo"], cand=cand)
    ref = T.serial(call, wrong, real)
    assert (ref[1][0] >= 0).all() and np.abs(ref[3]).max() > 0.1
    got, pending = T.late_producer(call, wrong, real, torch.cuda.Stream())
    assert pending, "rag_tokvec_rerank_dev waited for the work queued before it on its stream"
    T.assert_same(got, ref, "rerank behind a late producer")


@pytest.mark.parametrize("mode", [0, 1])
def test_retrieve_maxsim_dev_is_ordered_on_its_stream(full, mode):
    import torch
    w = world()
    ptr, terms, wts = w["packed"]
    call = lambda d, s: _composite(full, mode, stream=s, dev=d)
    real = dict(q_emb=w["q_emb"], qv=w["qv"], qo=w["qo"], ptr=ptr, terms=terms, w=wts)
    wrong = {k: np.zeros_like(v) for k, v in real.items()}               # legal: queries without terms or token vectors
    wrong["q_emb"] = np.ones_like(w["q_emb"])
    ref = T.serial(call, wrong, real)
    assert (ref[0][:, 0] >= 0).sum() >= 30
    got, pending = T.late_producer(call, wrong, real, torch.cuda.Stream())
    assert pending, "rag_retrieve_maxsim_dev waited for the work queued before it on its stream"
    T.assert_same(got, ref, f"composite mode {mode} behind a late producer")
