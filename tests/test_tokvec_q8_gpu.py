"""GPU: the 8-bit form of the resident token-vector store (RAG_TOKVEC_MXFP8: E4M3 codes with one power-of-two scale per 32
components) against the numpy quantiser of tests/tokvec_q8_tools.py and against the fp16 form.

Bit for bit: rag_tokvec_fetch_host against the numpy quantiser (seeded rows and the edge blocks); one load against chunked host and
device appends; the rerank and the four composites against an fp16-form handle loaded with the FETCHED rows (every stored value is
an fp16 value, the kernel expands it to the same MFMA operand: the same bits); a pair's score whatever surrounds it; the store
through rag_index_compact_live against a fresh 8-bit handle loaded with the survivors' original float32 rows.
Bars: (a) |score - float64 MaxSim over the fetched rows| < 1e-4, the fp16 form's derivation; (b) |score - float64 MaxSim over the
ORIGINAL float32 unit rows| < 2^-4 + 2^-13 + 1e-4: derived (an E4M3 component at or above the block's smallest normal moves by <=
2^-4 |x|, a smaller one by <= 2^-18 amax, a mean of maxima is 1-Lipschitz), not measured.
Measured on an MI355X, (a) / (b) at dim 32, 96, 128, 1024 (seeded unit rows without a planted component: the maxima are small
dots of random rows): 5.8e-8 / 9.3e-3, 4.6e-8 / 5.8e-3, 2.5e-8 / 4.3e-3, 3.0e-8 / 1.8e-3; through search_late_interaction 1.2e-3.
On the CPU (tests/test_tokvec_q8_cpu.py, float64 MaxSim over stored against original rows with a planted query component): 2.7e-3,
2.1e-3, 1.6e-3, 6.6e-4. Ranking quality on a real checkpoint's vectors is unmeasured: none exists offline."""
import json

import numpy as np
import pytest

import m3_tools as M
import sparse_tools as S
import stream_tools as T
import tokvec_q8_tools as Q8
import tokvec_tools as V

pytestmark = pytest.mark.gpu

DIMS = [32, 96, 128, 1024]
D_ROWS = [0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257]
Q_ROWS = [0, 1, 16, 17, 32, 33, 65]
ERR_ARG, ERR_STATE = r"\(-1\)", r"\(-3\)"
u32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _engine(dim=64):
    from optimized_rag_amd import RagEngine
    return RagEngine(dim=dim, device=0)


@pytest.fixture(scope="module")
def eng():
    """the 8-bit handle, WITHOUT a dense index: ids are row numbers"""
    e = _engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def twin():
    """the fp16-form handle that is loaded with what the 8-bit one returns from fetch"""
    e = _engine()
    yield e
    e.close()


def _pack_unit(rng, counts, dim):
    return M.pack([V.unit_rows(rng, n, dim) for n in counts], dim)


def _fetch_all(e):
    info = e.tokvec_info()
    return M.pack([e.tokvec_fetch(i) for i in range(info["n_docs"])], info["dim"])


def _load_twin(e8, e16):
    """e16 <- the fetched rows of e8 in the fp16 form; they are fp16 values, so e16 stores exactly them"""
    v, off = _fetch_all(e8)
    e16.tokvec_load(v, off)
    assert e16.tokvec_form() == "fp16"
    np.testing.assert_array_equal(u32(_fetch_all(e16)[0]), u32(v))
    return v, off


def _rerank_dev(e, q, qo, cand, k):
    import torch
    Q, pool = cand.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ids = torch.full((Q, k), -7, dtype=torch.int64, device="cuda")
    rw = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((Q, k), float("nan"), dtype=torch.float64, device="cuda")
    ps = torch.full((Q, pool), float("nan"), dtype=torch.float32, device="cuda")
    qd = t(q) if q.shape[0] else torch.zeros((1, q.shape[1]), device="cuda")
    e.tokvec_rerank_dev(qd, t(qo), t(cand.astype(np.int32)), k, ids, rw, sc, ps)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in (ids, rw, sc, ps))


def _same_rerank(a, b, what):
    for name, x, y in zip(("ids", "rows", "scores", "pair scores"), a, b):
        assert x.dtype == y.dtype and x.shape == y.shape, f"{what}: {name}"
        np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=f"{what}: {name}")


def _hbm_interval(rows, docs, dim):
    lo = rows * dim * 33 // 32 + (docs + 1) * 8
    return lo, lo + 16 * rows + 64


def _mixed_rows(dim):
    """seeded unit rows, rows of every block exponent, the edge blocks -> (vectors, offsets) with empty documents between"""
    rng = np.random.default_rng(dim)
    unit = V.unit_rows(rng, 21, dim)
    wide = (rng.standard_normal((30, dim)) * np.exp(rng.uniform(-12, 9, (30, 1)))).astype(np.float32)
    v = np.concatenate([unit, wide, Q8.edge_rows(dim)])
    counts = [3, 0, 0, 17, 1, 0, 30, 0, v.shape[0] - 51]
    return v, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


# ---- the store -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_fetch_is_the_numpy_quantiser_bit_for_bit_and_info(dim):
    e = _engine()
    try:
        assert e.tokvec_form() is None
        v, off = _mixed_rows(dim)
        n, docs = v.shape[0], off.shape[0] - 1
        e.tokvec_load(v, off, form="mxfp8")
        assert e.tokvec_form() == "mxfp8"
        info = e.tokvec_info()
        assert set(info) == {"n_docs", "rows", "dim", "hbm_bytes"} and (info["n_docs"], info["rows"], info["dim"]) == (docs, n, dim)
        lo, hi = _hbm_interval(n, docs, dim)
        assert lo <= info["hbm_bytes"] <= hi, (lo, info["hbm_bytes"], hi)
        exp = Q8.stored(v)
        for i in range(docs):
            got = e.tokvec_fetch(i)
            assert got.shape == (off[i + 1] - off[i], dim) and got.dtype == np.float32
            np.testing.assert_array_equal(u32(got), u32(exp[off[i]:off[i + 1]]), err_msg=f"document {i}")
        # a reservation alone reports its bytes; the fp16 form's figure is the one it always was
        e.tokvec_reserve(7, 1000, dim, form="mxfp8")
        lo, hi = _hbm_interval(1000, 7, dim)
        assert lo <= e.tokvec_info()["hbm_bytes"] <= hi and e.tokvec_form() == "mxfp8" and e.tokvec_info()["rows"] == 0
        e.tokvec_reserve(7, 1000, dim)
        assert e.tokvec_info()["hbm_bytes"] == 1000 * dim * 2 + 8 * 8 and e.tokvec_form() == "fp16"
    finally:
        e.close()


def test_a_second_load_replaces_the_first_in_either_form_and_an_unknown_form_is_refused():
    from optimized_rag_amd import RagError
    e = _engine()
    try:
        rng = np.random.default_rng(1)
        a, a_off = _pack_unit(rng, [4, 0, 9], 96)
        b, b_off = _pack_unit(rng, [2, 33], 32)
        e.tokvec_load(a, a_off, form="mxfp8")
        e.tokvec_load(b, b_off, form="mxfp8")                            # the same form
        assert e.tokvec_form() == "mxfp8" and e.tokvec_info()["n_docs"] == 2 and e.tokvec_info()["dim"] == 32
        np.testing.assert_array_equal(u32(_fetch_all(e)[0]), u32(Q8.stored(b)))
        e.tokvec_load(a, a_off)                                          # the other form
        assert e.tokvec_form() == "fp16" and e.tokvec_info()["hbm_bytes"] == 13 * 96 * 2 + 4 * 8
        np.testing.assert_array_equal(u32(_fetch_all(e)[0]), u32(V.fp16_round(a)))
        e.tokvec_load(a, a_off, form="mxfp8")                            # and back
        assert e.tokvec_form() == "mxfp8"
        np.testing.assert_array_equal(u32(_fetch_all(e)[0]), u32(Q8.stored(a)))
        # an unknown form: RAG_ERR_ARG from the library, the store stays as it is
        for bad in (2, -1, 7):
            with pytest.raises(RagError, match=ERR_ARG):
                e.tokvec_reserve(4, 16, 32, form=bad)
            with pytest.raises(RagError, match=ERR_ARG):
                e.tokvec_load(b, b_off, form=bad)
        with pytest.raises(RagError, match="form"):
            e.tokvec_reserve(4, 16, 32, form="int4")
        assert e.tokvec_form() == "mxfp8" and e.tokvec_info()["n_docs"] == 3
        np.testing.assert_array_equal(u32(_fetch_all(e)[0]), u32(Q8.stored(a)))
    finally:
        e.close()


def test_every_rejection_leaves_the_counts_and_the_block_can_be_retried():
    import torch
    from optimized_rag_amd import RagError
    e = _engine()
    try:
        rng = np.random.default_rng(3)
        dim = 96
        good = rng.standard_normal((10, dim)).astype(np.float32)
        good[7, 40] = 65519.0                                            # the largest magnitude the fp16 form accepts: saturates
        off = np.array([0, 4, 4, 10], dtype=np.int64)
        e.tokvec_reserve(4, 16, dim, form="mxfp8")
        e.tokvec_append(good[:4], [0, 4])
        state = e.tokvec_info()
        assert state["n_docs"] == 1 and state["rows"] == 4

        def dev(v, o):
            e.tokvec_append_dev(torch.from_numpy(np.ascontiguousarray(v)).cuda(), torch.from_numpy(np.asarray(o, dtype=np.int64)).cuda())

        def host(v, o):
            e.tokvec_append(v, o)

        nan, inf, big = good.copy(), good.copy(), good.copy()
        nan[9, 95] = np.nan
        inf[0, 0] = -np.inf
        big[5, 33] = 65520.0                                             # rounds to inf as fp16: what the fp16 form rejects
        for put in (host, dev):
            for v, o in ((good, [0, 1, 2, 3, 10]),                       # past the reserved documents
                         (np.concatenate([good, good]), [0, 13]),        # past the reserved rows
                         (good, [0, 6, 5, 10]),                          # a decreasing offset inside the block
                         (nan, off), (inf, off), (big, off)):
                with pytest.raises(RagError, match=ERR_ARG):
                    put(v, o)
                assert e.tokvec_info() == state and e.tokvec_form() == "mxfp8"
                np.testing.assert_array_equal(u32(e.tokvec_fetch(0)), u32(Q8.stored(good[:4])))
            put(good, off)                                               # the corrected block appends
            assert e.tokvec_info()["n_docs"] == 4 and e.tokvec_info()["rows"] == 14
            got_v, got_off = _fetch_all(e)
            np.testing.assert_array_equal(got_off, [0, 4, 8, 8, 14])
            np.testing.assert_array_equal(u32(got_v), u32(Q8.stored(np.concatenate([good[:4], good]))))
            assert got_v[4 + 7, 40] == 57344.0
            e.tokvec_reserve(4, 16, dim, form="mxfp8")
            e.tokvec_append(good[:4], [0, 4])
    finally:
        e.close()


@pytest.mark.parametrize("dim", [32, 96])
def test_load_and_chunked_appends_give_the_same_bits(eng, dim):
    import torch
    rng = np.random.default_rng(11)
    counts = [5, 0, 33, 1, 0, 64, 7, 2, 0, 19]
    v, off = M.pack([(rng.standard_normal((c, dim)) * np.exp(rng.uniform(-6, 6, (c, 1)))).astype(np.float32) for c in counts], dim)
    eng.tokvec_load(v, off, form="mxfp8")
    ref_v, ref_off = _fetch_all(eng)
    np.testing.assert_array_equal(ref_off, off)
    np.testing.assert_array_equal(u32(ref_v), u32(Q8.stored(v)))
    other = _engine()
    try:
        other.tokvec_reserve(len(counts) + 3, off[-1] + 10, dim, form="mxfp8")
        other.tokvec_append(v, off[0:4])                                 # host block: documents 0-2
        vd, od = torch.from_numpy(v).cuda(), torch.from_numpy(off).cuda()
        other.tokvec_append_dev(vd, od[3:8].contiguous())               # device block whose offsets do not start at 0
        other.tokvec_append(v, off[7:9])
        other.tokvec_append_dev(vd, od[8:].contiguous())
        assert other.tokvec_info()["n_docs"] == len(counts) and other.tokvec_info()["rows"] == off[-1]
        got_v, got_off = _fetch_all(other)
        np.testing.assert_array_equal(got_off, off)
        np.testing.assert_array_equal(u32(got_v), u32(ref_v))
    finally:
        other.close()


# ---- scores ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_rerank_has_the_fp16_forms_bits_over_the_fetched_rows_and_meets_both_bars(eng, twin, dim):
    rng = np.random.default_rng(dim)
    d, d_off = _pack_unit(rng, D_ROWS, dim)
    q, q_off = _pack_unit(rng, Q_ROWS, dim)
    eng.tokvec_load(d, d_off, form="mxfp8")
    stored, _ = _load_twin(eng, twin)
    np.testing.assert_array_equal(u32(stored), u32(Q8.stored(d)))
    n = len(D_ROWS)
    cand = np.tile(np.arange(n, dtype=np.int32), (len(Q_ROWS), 1))
    cand = np.concatenate([cand, np.full((len(Q_ROWS), 1), -1, np.int32), np.full((len(Q_ROWS), 1), n, np.int32)], axis=1)   # cand < 0, past the store
    k = cand.shape[1]
    got = _rerank_dev(eng, q, q_off, cand, k)
    _same_rerank(got, _rerank_dev(twin, q, q_off, cand, k), f"dim {dim}: 8-bit against the fp16 form over the fetched rows")
    ids, rows, sc, ps = got
    empty = V.slot_empty(q_off, d_off, cand)
    # the slot rules: an empty query (row 0), an empty document (column 0), cand < 0 and a row past the store score 0.0 and are skipped
    assert empty[0].all() and empty[:, 0].all() and empty[:, n].all() and empty[:, n + 1].all() and not empty[1:, 1:n].any()
    assert (ps[empty] == 0).all()
    err_a = float(np.abs(ps - V.pair_scores(q, q_off, stored, d_off, cand)).max())
    err_b = float(np.abs(ps - V.pair_scores(q, q_off, d, d_off, cand)).max())
    print(f"tokvec 8-bit rerank dim {dim}: max |score - float64 over the fetched rows| = {err_a:.3e}, over the original rows = {err_b:.3e}")
    assert err_a < 1e-4
    assert err_b < Q8.BAR_B
    e_ids, e_rows, e_sc = V.stable_topk(ps, cand, empty, k)
    np.testing.assert_array_equal(rows, e_rows)
    np.testing.assert_array_equal(ids, e_rows.astype(np.int64))
    np.testing.assert_array_equal(V.bits(sc), V.bits(e_sc))
    _same_rerank(eng.tokvec_rerank(q, q_off, cand, k), got, f"dim {dim}: _host against _dev")


@pytest.mark.parametrize("dim", [32, 96])
def test_edge_blocks_and_wide_rows_score_as_the_fp16_form_does(eng, twin, dim):
    """stored values down to 2^-24 and up to 57344, both signs of zero, every block exponent: the expansion to the fp16 operand is
    exact for all of them (queries scaled so that no sum overflows float32)"""
    v, off = _mixed_rows(dim)
    eng.tokvec_load(v, off, form="mxfp8")
    _load_twin(eng, twin)
    rng = np.random.default_rng(5)
    q, qo = _pack_unit(rng, [3, 17], dim)
    q[:3] *= np.float32(2.0 ** 10)                                       # subnormal stored values reach the float32 score
    cand = np.tile(np.arange(off.shape[0] - 1, dtype=np.int32), (2, 1))
    got = _rerank_dev(eng, q, qo, cand, cand.shape[1])
    assert np.isfinite(got[3]).all() and (got[3] != 0).any()
    _same_rerank(got, _rerank_dev(twin, q, qo, cand, cand.shape[1]), f"dim {dim}: edge blocks")


def test_a_pairs_bits_do_not_depend_on_pool_slot_neighbours_or_run(eng):
    rng = np.random.default_rng(6)
    dim = 128
    counts = (D_ROWS * 3)[:30]
    d, do = _pack_unit(rng, counts, dim)
    eng.tokvec_load(d, do, form="mxfp8")
    q, qo = _pack_unit(rng, [9, 33, 17], dim)
    target = 11                                                          # a 257-row document; query 1 (33 rows)
    one_q, one_off = q[qo[1]:qo[2]], np.array([0, 33], dtype=np.int64)
    alone = _rerank_dev(eng, one_q, one_off, np.array([[target]], dtype=np.int32), 1)         # pool 1, query position 0
    assert alone[3][0, 0] != 0 and alone[1][0, 0] == target
    cand = rng.integers(-1, len(counts) + 2, (3, 256)).astype(np.int32)
    cand[1, 77] = target
    cand[1, 200] = target
    cand[2, 0] = 8                                                       # a 127-row document: the 2-tile groups
    big = _rerank_dev(eng, q, qo, cand, 256)                             # pool 256, query position 1, two slots
    _same_rerank(_rerank_dev(eng, q, qo, cand, 256), big, "a second run")
    bits = alone[3].view(np.uint32)[0, 0]
    assert big[3].view(np.uint32)[1, 77] == bits and big[3].view(np.uint32)[1, 200] == bits
    short = _rerank_dev(eng, q[qo[2]:qo[3]], np.array([0, 17], dtype=np.int64), np.array([[3, 8]], dtype=np.int32), 2)
    assert short[3].view(np.uint32)[0, 1] == big[3].view(np.uint32)[2, 0]


# ---- the composites and live writes -------------------------------------------------------------------------------------------------
N_DOCS, DIM, TOK_DIM, POOL, K, WEIGHTS = 300, 64, 96, 40, 10, (0.4, 0.2, 0.4)
_WORLD = {}


def world():
    if not _WORLD:
        rng = np.random.default_rng(8)
        indptr, doc, w = S.make_corpus(n_docs=N_DOCS, n_terms=1500, seed=5)
        queries = S.make_queries(indptr, seed=6)
        emb = rng.standard_normal((N_DOCS, DIM)).astype(np.float32)
        q_emb = (emb[rng.integers(0, N_DOCS, len(queries))] + 0.7 * rng.standard_normal((len(queries), DIM))).astype(np.float32)
        counts = [int(c) for c in rng.integers(0, 40, N_DOCS)]
        counts[0], counts[1], counts[150], counts[N_DOCS - 1] = 7, 0, 0, 21
        vecs = [V.unit_rows(rng, c, TOK_DIM) for c in counts]
        q_counts = [int(c) for c in rng.integers(1, 34, len(queries))]
        q_counts[3] = 0
        qv, qo = _pack_unit(rng, q_counts, TOK_DIM)
        _WORLD.update(indptr=indptr, doc=doc, w=w, packed=S.pack_queries(queries), emb=emb, q_emb=q_emb, vecs=vecs, qv=qv, qo=qo,
                      ids=(5000 + 3 * np.arange(N_DOCS)).astype(np.int64))
    return _WORLD


def _load_world(e, form, keep=None, headroom=0, vecs=None):
    """the world's rows `keep` (all: None) on handle e: index with explicit ids, sparse postings, token vectors (`vecs`: per world row,
    default the original float32 rows) in `form`"""
    w = world()
    keep = np.arange(N_DOCS) if keep is None else np.asarray(keep)
    e.index_load(w["emb"][keep], ids=w["ids"][keep])
    remap = np.full(N_DOCS, -1, dtype=np.int64)
    remap[keep] = np.arange(keep.shape[0])
    term_of = np.repeat(np.arange(w["indptr"].shape[0] - 1, dtype=np.int64), np.diff(w["indptr"]))
    sel = remap[w["doc"]] >= 0
    indptr = np.zeros_like(w["indptr"])
    np.cumsum(np.bincount(term_of[sel], minlength=indptr.shape[0] - 1), out=indptr[1:])
    e.sparse_load(indptr, remap[w["doc"][sel]].astype(np.int32), w["w"][sel], keep.shape[0])
    v, off = M.pack([(vecs or w["vecs"])[i] for i in keep], TOK_DIM)
    e.tokvec_reserve(keep.shape[0] + headroom, off[-1] + 64 * headroom, TOK_DIM, form=form)
    e.tokvec_append(v, off)


def _composites(e, sparse=True):
    """every composite entry on the world's queries -> {name: tuple of numpy outputs}"""
    import torch
    w = world()
    ptr, terms, wts = w["packed"]
    d = T.to_dev(dict(q_emb=w["q_emb"], qv=w["qv"], qo=w["qo"], ptr=ptr, terms=terms, w=wts))
    sp = dict(term_ptr=d["ptr"], terms=d["terms"], weights=d["w"])
    Q = w["q_emb"].shape[0]
    out = {}

    def keep(name, tensors):
        torch.cuda.synchronize()
        out[name] = tuple(t.cpu().numpy() for t in tensors)

    keep("retrieve_maxsim mode 0", e.retrieve_maxsim_dev(d["q_emb"], d["qv"], d["qo"], POOL, K))
    if not sparse:
        return out
    keep("retrieve_maxsim mode 1", e.retrieve_maxsim_dev(d["q_emb"], d["qv"], d["qo"], POOL, K, **sp))
    rows = torch.from_numpy(np.random.default_rng(9).integers(-1, e.n_rows + 1, (Q, POOL)).astype(np.int32)).cuda()
    ids = torch.full((Q, K), -7, dtype=torch.int64, device="cuda")
    sc = torch.full((Q, K), float("nan"), dtype=torch.float64, device="cuda")
    rw = torch.full((Q, K), -7, dtype=torch.int32, device="cuda")
    comp = torch.full((Q, K, 3), float("nan"), dtype=torch.float64, device="cuda")
    e.m3_score_rows_dev(rows, K, ids, sc, q_emb=d["q_emb"], q_vecs=d["qv"], q_off=d["qo"], w=WEIGHTS, rows_out=rw, components_out=comp, **sp)
    keep("m3_score_rows", (ids, sc, rw, comp))
    for mode in (1, 2):
        keep(f"retrieve_m3 mode {mode}", e.retrieve_m3_dev(d["q_emb"], POOL, K, q_vecs=d["qv"], q_off=d["qo"], mode=mode, w=WEIGHTS, **sp))
    return out


def _same_composites(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        for i, (x, y) in enumerate(zip(a[name], b[name])):
            assert x.shape == y.shape and x.dtype == y.dtype, f"{what}: {name} output {i}"
            np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=f"{what}: {name} output {i}")


def test_composites_have_the_fp16_forms_bits_over_the_fetched_rows():
    w = world()
    a, b = _engine(DIM), _engine(DIM)
    try:
        _load_world(a, "mxfp8")
        fetched = [a.tokvec_fetch(i) for i in range(N_DOCS)]
        for i in (0, 2, N_DOCS - 1):
            np.testing.assert_array_equal(u32(fetched[i]), u32(Q8.stored(w["vecs"][i])))
        _load_world(b, "fp16", vecs=fetched)
        got = _composites(a)
        _same_composites(got, _composites(b), "8-bit against the fp16 form over the fetched rows")
        ids, sc, cand = got["retrieve_maxsim mode 1"]
        assert (ids[:, 0] >= 0).sum() >= 20 and (ids[3] == -1).all()             # query 3 has no token vectors
        for qi in (0, 7):                                                        # and the scores are MaxSim of the stored rows
            vq = w["qv"][w["qo"][qi]:w["qo"][qi + 1]]
            for i, s in zip(ids[qi], sc[qi]):
                if i >= 0:
                    assert abs(s - M.maxsim(vq, fetched[(int(i) - 5000) // 3])) < 1e-4
        comp = got["retrieve_m3 mode 2"][2]
        assert np.abs(comp[..., 2]).max() > 0.05                                 # the colbert component took part
    finally:
        a.close()
        b.close()


def test_live_writes_insert_compact_live_and_a_plain_compaction():
    from optimized_rag_amd import RagError
    w = world()
    a, f = _engine(DIM), _engine(DIM)
    try:
        a.set_option("tokvec_compact_rows", 64)                          # ~5,800 rows move in chunks of 64: every chunk border is crossed
        _load_world(a, "mxfp8", headroom=4)
        hbm = a.tokvec_info()["hbm_bytes"]
        # first, middle, last, a run, and documents without rows (1 and 150)
        dead = np.array([0, 1, 2, 77, 78, 79, 150, 151, 222, N_DOCS - 1])
        live = np.setdiff1d(np.arange(N_DOCS), dead)
        assert a.index_delete(w["ids"][dead]) == dead.shape[0]
        rm = a.index_compact(keep_resident=True)
        np.testing.assert_array_equal(np.nonzero(rm < 0)[0], dead)
        info = a.tokvec_info()
        assert (info["n_docs"], info["rows"], info["hbm_bytes"]) == (live.shape[0], sum(w["vecs"][i].shape[0] for i in live), hbm)
        assert a.tokvec_form() == "mxfp8"
        # equals a fresh 8-bit handle loaded with the survivors' ORIGINAL float32 rows: quantisation is per row and block
        _load_world(f, "mxfp8", keep=live)
        got_v, got_off = _fetch_all(a)
        exp_v, exp_off = _fetch_all(f)
        np.testing.assert_array_equal(got_off, exp_off)
        np.testing.assert_array_equal(u32(got_v), u32(exp_v))
        np.testing.assert_array_equal(u32(got_v), u32(Q8.stored(M.pack([w["vecs"][i] for i in live], TOK_DIM)[0])))
        cand = np.random.default_rng(3).integers(-1, live.shape[0] + 1, (len(w["qo"]) - 1, 64)).astype(np.int32)
        _same_rerank(_rerank_dev(a, w["qv"], w["qo"], cand, 16), _rerank_dev(f, w["qv"], w["qo"], cand, 16), "rerank after compact_live")
        _same_composites(_composites(a), _composites(f), "composites after compact_live")
        # an insert leaves the store alone: the composite waits for the new rows' vectors
        rng = np.random.default_rng(9)
        new_vecs = [V.unit_rows(rng, 40, TOK_DIM), w["qv"][w["qo"][1]:w["qo"][2]]]
        a.index_insert(w["q_emb"][:2] * 1.0, ids=np.array([1, 2], dtype=np.int64))
        with pytest.raises(RagError, match=ERR_STATE):
            _composites(a, sparse=False)
        a.tokvec_append(new_vecs[0], [0, 40])
        with pytest.raises(RagError, match=ERR_STATE):                   # one of the two rows covered
            _composites(a, sparse=False)
        a.tokvec_append(new_vecs[1], [0, new_vecs[1].shape[0]])
        np.testing.assert_array_equal(u32(a.tokvec_fetch(live.shape[0] + 1)), u32(Q8.stored(new_vecs[1])))
        ids, sc, _ = _composites(a, sparse=False)["retrieve_maxsim mode 0"]
        # query 1 finds its own token vectors in the inserted row (dense cosine 1; MaxSim 1 up to the storage error of bar (b))
        assert ids[1, 0] == 2 and abs(sc[1, 0] - 1.0) < Q8.BAR_B
        # a plain compaction that removes rows marks the store stale, as for the fp16 form; the handle stays usable
        assert a.index_delete(np.array([1], dtype=np.int64)) == 1
        a.index_compact()
        with pytest.raises(RagError, match=ERR_STATE):
            _composites(a, sparse=False)
        with pytest.raises(RagError, match=ERR_STATE):
            a.tokvec_rerank(w["qv"], w["qo"], cand, 2)
        assert a.dense_topk(w["q_emb"], 5)[0].shape == (len(w["qo"]) - 1, 5)
        a.tokvec_load(*M.pack(new_vecs, TOK_DIM), form="mxfp8")          # a reload clears it
        assert a.tokvec_rerank(w["qv"], w["qo"], cand[:, :4], 2)[0].shape[1] == 2
    finally:
        a.close()
        f.close()


# ---- the Python surface ------------------------------------------------------------------------------------------------------------
def test_document_index_loads_and_searches_the_8_bit_form(tmp_path):
    import xlmr_tools as X
    from optimized_rag_amd.document_store import GpuDocumentIndex
    from optimized_rag_amd.embeddings import LocalEmbeddingService
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
    rng = np.random.default_rng(12)
    query = " ".join(rng.choice(words[:20], 6))
    texts = [" ".join(rng.choice(words[:30], int(rng.integers(2, 40)))) for _ in range(40)]
    enc = X.roberta_tokenizer(words).encode_batch([query] + texts)
    pl = np.array([len(x.ids) for x in enc], dtype=np.int32)
    pi = np.zeros((len(enc), int(pl.max())), dtype=np.int32)
    for i, x in enumerate(enc):
        pi[i, :pl[i]] = x.ids
    ref = M.heads_reference(X.xlmr_to_bert_names(sd, head=False), cfg, pi, np.zeros_like(pi), pl, heads)
    exp = np.array([M.maxsim(ref["vecs"][0], ref["vecs"][1 + i]) for i in range(40)])
    e = _engine(128)
    try:
        svc = LocalEmbeddingService.from_dir(str(d), engine=e, max_length=64)
        index = GpuDocumentIndex(svc, dim=128, engine=e)
        rows = [dict(content=t, agent_id="a", filename=f"f{i}", metadata=dict(i=i)) for i, t in enumerate(texts)]
        index.bulk_load(rows, np.asarray(svc.generate_embeddings_batch(texts), dtype=np.float32))
        vecs = svc.encode_multi(texts, return_dense=False, return_sparse=False)["colbert_vecs"]
        index.load_token_vectors(*M.pack(vecs, 96))                      # form="fp16" is the default: results as before
        assert e.tokvec_form() == "fp16"
        res16 = index.search_late_interaction("a", query, top_k=5, pool=20)
        index.load_token_vectors(*M.pack(vecs, 96), form="fp16")
        assert index.search_late_interaction("a", query, top_k=5, pool=20) == res16
        assert max(abs(r["colbert_score"] - exp[int(r["filename"][1:])]) for r in res16) < 1e-3
        index.load_token_vectors(*M.pack(vecs, 96), form="mxfp8")
        assert e.tokvec_form() == "mxfp8"
        res8 = index.search_late_interaction("a", query, top_k=5, pool=20)
        assert len(res8) == 5 and all(r["score"] == r["colbert_score"] for r in res8)
        err = max(abs(r["colbert_score"] - exp[int(r["filename"][1:])]) for r in res8)
        print(f"search_late_interaction over the 8-bit form: max |colbert_score - float64 MaxSim| = {err:.3e}")
        assert err < Q8.BAR_B
        assert (np.diff([r["colbert_score"] for r in res8]) <= 0).all()
        index.build_token_vectors(texts, batch=16, form="mxfp8")         # the forward's output quantised on the device: the same store
        assert e.tokvec_form() == "mxfp8" and index.search_late_interaction("a", query, top_k=5, pool=20) == res8
    finally:
        e.close()
