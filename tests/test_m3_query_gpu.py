"""GPU: rag_search_m3_tokens_dev / _tenants_dev - query token ids in, the three-way bge-m3 ranking out - against the three calls it
composes, made one after another by the caller: rag_embed_multi_dev -> rag_lexical_compact_dev -> rag_retrieve_m3_dev. Every
comparison is exact: ids, candidate lists, and the bits of the float64 scores and components.

The world is small: a seeded 2-layer, hidden-128 encoder with 64-wide attention heads and both heads of the embedder (token vectors of
96 d), 300 rows with explicit ids and three tenants, sparse postings and a token-vector store over them, 12 queries of 1-40 tokens,
among them one that is only [CLS] [SEP] (no terms, one token row), one of a single token (no token row) and one at seq_len."""
import numpy as np
import pytest

import m3_tools as M
import sparse_tools as S
import stream_tools as ST
import tokvec_tools as V
from oracle import bert_oracle as B

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = r"\(-1\)", r"\(-3\)"
CFG = dict(vocab_size=500, hidden=128, layers=2, heads=2, ffn=256, max_pos=128, type_vocab=2, eps=1e-12)
N, D, TOK_DIM, L = 300, 128, 96, 40
CLS, SEP = 1, 2
SKIP = (0, CLS, SEP, 3)
POOL, K = 20, 7
WEIGHTS = [(0.4, 0.2, 0.4), (0.4, 0.2, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)]
QUERY_TENANTS = [0, 1, 2, -1, 5, 0, 1, 2, -1, 0, 5, 1]                   # 5 owns no row, -1 is not filtered
_W = {}


def world():
    if not _W:
        rng = np.random.default_rng(77)
        lens = np.array([2, 1, L, 7, 12, 40, 3, 25, 33, 5, 18, 9], dtype=np.int32)
        ids = rng.integers(4, 200, (len(lens), L)).astype(np.int32)      # the frequent end of the corpus vocabulary: terms match
        ids[:, 0] = CLS
        for i, n in enumerate(lens):
            ids[i, n - 1] = SEP if n > 1 else CLS
            ids[i, n:] = 0
        indptr, doc, w = S.make_corpus(n_docs=N, n_terms=CFG["vocab_size"] + S.N_EMPTY, seed=5)
        counts = rng.integers(1, 9, N)
        d_vecs = V.unit_rows(rng, int(counts.sum()), TOK_DIM)
        _W.update(ids=ids, tt=np.zeros_like(ids), lens=lens, emb=rng.standard_normal((N, D)).astype(np.float32),
                  row_ids=(9000 + 3 * np.arange(N)).astype(np.int64), ten=(np.arange(N) % 3).astype(np.int32), csr=(indptr, doc, w),
                  d_vecs=d_vecs, d_off=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                  weights=B.seeded_weights(CFG, 21), heads=M.seeded_heads(D, TOK_DIM, 6))
    return _W


def make_engine(tok_head=True, lex_head=True, sparse=True, tokvec=True, dim=D, embedder=True):
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    w = world()
    e = RagEngine(dim=dim, device=0)
    e.index_load(np.ascontiguousarray(w["emb"][:, :dim]), ids=np.array(w["row_ids"]))
    e.set_tenants(np.array(w["ten"]))
    if embedder:
        e.embed_load(CFG, flatten_state_dict(w["weights"], CFG["layers"], head=False), normalize=True, pooling="cls")
        h = w["heads"]
        if tok_head or lex_head:
            e.embed_heads_load(tok_w=h["tok_w"] if tok_head else None, tok_b=h["tok_b"] if tok_head else None,
                               lex_w=h["lex_w"] if lex_head else None, lex_b=h["lex_b"])
    if sparse:
        e.sparse_load(*w["csr"], N)
    if tokvec:
        e.tokvec_reserve(N, int(w["d_off"][-1]), TOK_DIM)
        e.tokvec_append(w["d_vecs"], w["d_off"])
    return e


@pytest.fixture(scope="module")
def engine():
    e = make_engine()
    yield e
    e.close()


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(tensors):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy().copy() for t in tensors]


def queries(sel=None):
    w = world()
    sel = np.arange(len(w["lens"])) if sel is None else np.asarray(sel)
    return _t(w["ids"][sel]), _t(w["tt"][sel]), _t(w["lens"][sel])


def one_call(e, q, mode, wts, tenant=-1, pool=POOL, k=K, stream=None):
    return _np(e.search_m3_tokens_dev(*q, pool, k, skip_ids=SKIP, mode=mode, w=wts, tenant=tenant, stream=stream))


def three_calls(e, q, mode, wts, tenant=-1, pool=POOL, k=K):
    """the caller's composition, at the capacities the one call documents: Q * (L - 1) token rows, Q * L terms"""
    import torch
    ids, tt, lens = q
    Q, Ls = ids.shape
    need_lex, need_tok = wts[1] > 0 or mode != 0, wts[2] > 0
    f32 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    dense = f32(Q, D)
    lex = f32(Q, Ls) if need_lex else None
    tok = f32(max(Q * (Ls - 1), 1), TOK_DIM) if need_tok else None
    off = torch.full((Q + 1,), -1, dtype=torch.int64, device="cuda") if need_tok else None
    e.embed_multi_dev(ids, tt, lens, dense=dense, lex=lex, tok=tok[:Q * (Ls - 1)] if need_tok else None, row_off=off)
    kw = {}
    if need_lex:
        ptr = torch.zeros((Q + 1,), dtype=torch.int32, device="cuda")
        terms = torch.zeros((Q * Ls,), dtype=torch.int32, device="cuda")
        qw = torch.zeros((Q * Ls,), dtype=torch.float32, device="cuda")
        e.lexical_compact_dev(ids, lex, lens, ptr, terms, qw, skip_ids=SKIP)
        kw.update(term_ptr=ptr, terms=terms, weights=qw)
    if need_tok:
        kw.update(q_vecs=tok, q_off=off)
    return _np(e.retrieve_m3_dev(dense, pool, k, mode=mode, w=wts, tenant=tenant, **kw))


def assert_same(got, ref, what):
    for g, r, name in zip(got, ref, ("ids", "scores", "components", "candidates")):
        if g.dtype == np.float64:
            g, r = g.view(np.int64), r.view(np.int64)
        np.testing.assert_array_equal(g, r, err_msg=f"{what}: {name}")


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_one_call_equals_the_three_calls(engine, mode):
    q = queries()
    for wts in WEIGHTS:
        ref = three_calls(engine, q, mode, wts)
        got = one_call(engine, q, mode, wts)
        assert_same(got, ref, f"mode {mode}, weights {wts}")
        ids, sc, comp, cand = got
        assert (ids[:, 0] >= 9000).all() and np.isfinite(sc).all()
        if wts[2] > 0:
            assert (comp[1, :, 2] == 0).all() and (comp[[0, 2, 3], 0, 2] != 0).all()     # a one-token query has no token row
        if wts[1] > 0:
            assert (comp[0, :, 1] == 0).all() and (comp[:, :, 1] > 0).any()              # [CLS] [SEP] alone has no terms
        for t in (0, 2):                                                                 # a scalar tenant
            assert_same(one_call(engine, q, mode, wts, tenant=t), three_calls(engine, q, mode, wts, tenant=t), f"mode {mode}, tenant {t}")


@pytest.mark.parametrize("mode", [0, 2])
def test_tenants_form_equals_the_scalar_form_query_by_query(engine, mode):
    w = world()
    ten = np.array(QUERY_TENANTS, dtype=np.int32)
    row_tenant = dict(zip(w["row_ids"].tolist(), w["ten"].tolist()))
    for wts in WEIGHTS[:2]:
        got = one_call(engine, queries(), mode, wts, tenant=ten)
        assert_same(got, three_calls(engine, queries(), mode, wts, tenant=ten), f"mode {mode}, per-query tenants, three calls")
        for i, t in enumerate(ten):
            single = one_call(engine, queries([i]), mode, wts, tenant=int(t))
            assert_same([g[i:i + 1] for g in got], single, f"mode {mode}, query {i}, tenant {t}")
            hit = got[0][i][got[0][i] >= 0]
            if t == 5:
                assert hit.size == 0 and (got[1][i] == 0).all()                          # a tenant that owns no row: all padding
            elif t >= 0:
                assert hit.size == K and all(row_tenant[int(x)] == t for x in hit)
            else:
                assert hit.size == K and len({row_tenant[int(x)] for x in hit}) > 1


def test_a_small_call_after_a_larger_one(engine):
    wts = WEIGHTS[0]
    small = queries([3, 0, 6])
    first = one_call(engine, small, 2, wts, pool=8, k=4)
    one_call(engine, queries(), 2, wts, pool=64, k=30)                                   # the workspace grows ...
    again = one_call(engine, small, 2, wts, pool=8, k=4)                                 # ... and is carved smaller again
    assert_same(again, first, "after a larger call")
    assert_same(again, three_calls(engine, small, 2, wts, pool=8, k=4), "after a larger call, three calls")


def test_what_a_zero_weight_leaves_out_is_not_required(engine):
    from optimized_rag_amd import RagError
    q = queries()
    no_colbert = make_engine(tok_head=False, tokvec=False)               # w_colbert = 0: no token head, no store
    try:
        for mode in (0, 1, 2):
            assert_same(one_call(no_colbert, q, mode, (0.4, 0.2, 0.0)), one_call(engine, q, mode, (0.4, 0.2, 0.0)), f"no token head, mode {mode}")
        with pytest.raises(RagError, match=ERR_STATE):
            one_call(no_colbert, q, 0, (0.4, 0.2, 0.4))
        assert_same(one_call(no_colbert, q, 0, (1.0, 0.0, 0.0)), one_call(engine, q, 0, (1.0, 0.0, 0.0)), "usable after the error")
    finally:
        no_colbert.close()
    no_sparse = make_engine(lex_head=False, sparse=False)                # mode 0 with w_sparse = 0: no lexical head, no postings
    try:
        for wts in ((1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.5, 0.0, 0.5)):
            assert_same(one_call(no_sparse, q, 0, wts), one_call(engine, q, 0, wts), f"no lexical head, weights {wts}")
        for mode, wts in ((0, (0.4, 0.2, 0.4)), (1, (1.0, 0.0, 0.0)), (2, (0.0, 0.0, 1.0))):
            with pytest.raises(RagError, match=ERR_STATE):
                one_call(no_sparse, q, mode, wts)
        assert_same(one_call(no_sparse, q, 0, (1.0, 0.0, 0.0)), one_call(engine, q, 0, (1.0, 0.0, 0.0)), "usable after the errors")
    finally:
        no_sparse.close()


def test_errors_leave_the_handle_usable(engine):
    from optimized_rag_amd import RagError
    q = queries()
    bare = make_engine(embedder=False)                                   # no embedder at all
    try:
        with pytest.raises(RagError, match=ERR_STATE):
            one_call(bare, q, 0, (1.0, 0.0, 0.0))
    finally:
        bare.close()
    narrow = make_engine(dim=64, sparse=False, tokvec=False)             # an index of another dimension than the embedder's output
    try:
        with pytest.raises(RagError, match=ERR_ARG):
            one_call(narrow, q, 0, (1.0, 0.0, 0.0))
        assert narrow.dense_topk(world()["emb"][:2, :64], 3)[0].shape == (2, 3)
    finally:
        narrow.close()
    ref = one_call(engine, q, 2, WEIGHTS[0])
    for bad in (dict(mode=3), dict(pool=300), dict(k=POOL + 1), dict(wts=(0.0, 0.0, 0.0)), dict(wts=(-1.0, 0.5, 0.5))):
        kw = dict(mode=2, wts=WEIGHTS[0])
        kw.update(bad)
        with pytest.raises(RagError, match=ERR_ARG):
            one_call(engine, q, kw.pop("mode"), kw.pop("wts"), **kw)
    with pytest.raises(RagError, match=ERR_ARG):
        engine.search_m3_tokens_dev(*q, POOL, K, skip_ids=range(9))
    assert_same(one_call(engine, q, 2, WEIGHTS[0]), ref, "after the errors")


@pytest.mark.parametrize("per_query", [False, True])
def test_ordered_on_the_callers_stream(engine, per_query):
    """inputs produced on a non-default stream immediately before the call, outputs consumed on it immediately after, nothing
    synchronised in between: the bits of the call made alone"""
    import torch
    w = world()
    real = dict(ids=w["ids"], tt=w["tt"], lens=w["lens"])
    wrong = dict(ids=np.roll(w["ids"], 3, axis=0), tt=w["tt"], lens=np.roll(w["lens"], 3))
    tenant = np.array(QUERY_TENANTS, dtype=np.int32) if per_query else 1
    call = lambda dev, st: list(engine.search_m3_tokens_dev(dev["ids"], dev["tt"], dev["lens"], POOL, K, skip_ids=SKIP, mode=2, w=WEIGHTS[0],
                                                            tenant=tenant, stream=st))
    ref = ST.serial(call, wrong, real)
    got, pending = ST.late_producer(call, wrong, real, torch.cuda.Stream())
    ST.assert_same(got, ref, "search_m3_tokens_dev on a side stream")
    assert_same(ref, one_call(engine, queries(), 2, WEIGHTS[0], tenant=tenant), "serial")
    assert pending, "search_m3_tokens_dev waited for the work queued before it on its stream"
