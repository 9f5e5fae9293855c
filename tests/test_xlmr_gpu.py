"""GPU: XLM-RoBERTa rerankers and embedders end to end - the RoBERTa pair layout of the device pair builder
(rag_ce_set_pair_format), models with one token type, the checkpoint loaders (cross_encoder.map_checkpoint, tokenizer.json), and the
one-call pipeline over a 24-bit token store against the oracle composition of tests/test_pipeline_gpu.py, at that file's bars:
candidates bit-exact, sigmoid scores within 1e-3, logits within 4e-3. Unlike there, the order of the ids is asserted for every
query: WORLD_SEED is chosen so that the ORACLE's top k + 1 scores of every query are more than 2e-3 apart
(test_the_oracle_scores_of_the_end_to_end_world_are_well_separated checks that on the CPU)."""
import json

import numpy as np
import pytest

import xlmr_tools as X
from oracle import bert_oracle as B
from oracle import rag_oracle as O

gpu = pytest.mark.gpu

RAG_ERR_ARG = -1
SCORE_TOL = 1e-3
DIM = 64
WORLD_SEED = 32          # oracle gap 4.2e-3 (seeds 0 .. 39 were tried on the CPU, oracle alone; most have a near-tie)


def _engine(dim=DIM):
    from optimized_rag_amd import RagEngine
    return RagEngine(dim=dim, device=0)


# ---- 5. the RoBERTa layout ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("id_bits", [16, 24])
def test_roberta_pair_layout_equals_the_numpy_builder(id_bits):
    """ql = 0, dl = 0, a -1 candidate, a row past the store, both sides over their share, L_pair = 8 and 9 (M = 4 and 5), 24, and 512
    with a 512-token query and passage; all types 0; back on format 0 the output is what it was before; format 2 is refused."""
    rng = np.random.default_rng(51)
    hi = 65536 if id_bits == 16 else 250002
    n, Ld, Lq = 9, 512, 512
    tok = rng.integers(3, hi, (n, Ld)).astype(np.int32)
    tok_len = np.array([0, 3, 512, 100, 1, 2, 509, 510, 600], dtype=np.int32)          # (600: clamped to the store's 512)
    q_tok = rng.integers(3, hi, (5, Lq)).astype(np.int32)
    q_len = np.array([0, 2, 512, 7, 254], dtype=np.int32)
    cand = np.tile(np.array([0, 1, 2, 3, -1, 4, 5, 6, 7, 8, n, n + 3], dtype=np.int64), (5, 1))
    e = _engine()
    try:
        e.tokens_load(tok, tok_len, id_bits=id_bits)
        for Lp in (8, 9, 24, 512):
            before = X.device_pairs(e, q_tok, q_len, cand, Lp, 101, 102)
            for a, b in zip(before, X.build_pairs(q_tok, q_len, cand, tok, tok_len, Lp, 101, 102, fmt=X.PAIR_BERT)):
                np.testing.assert_array_equal(a, b)
            e.ce_set_pair_format(X.PAIR_ROBERTA)
            got = X.device_pairs(e, q_tok, q_len, cand, Lp, X.XLMR_CLS, X.XLMR_SEP)
            want = X.build_pairs(q_tok, q_len, cand, tok, tok_len, Lp, X.XLMR_CLS, X.XLMR_SEP, fmt=X.PAIR_ROBERTA)
            for a, b in zip(got, want):
                np.testing.assert_array_equal(a, b)
            assert not got[1].any() and got[2].max() <= Lp and got[2].min() == 4
            assert e.lib.rag_ce_set_pair_format(e.h, 2) == RAG_ERR_ARG and e.lib.rag_ce_set_pair_format(e.h, -1) == RAG_ERR_ARG
            again = X.device_pairs(e, q_tok, q_len, cand, Lp, X.XLMR_CLS, X.XLMR_SEP)              # a refused format changes nothing
            for a, b in zip(again, got):
                np.testing.assert_array_equal(a, b)
            e.ce_set_pair_format(X.PAIR_BERT)
            after = X.device_pairs(e, q_tok, q_len, cand, Lp, 101, 102)
            for a, b in zip(after, before):
                np.testing.assert_array_equal(a, b)
    finally:
        e.close()


# ---- 6. the loader adds no arithmetic ---------------------------------------------------------------------------------------
def _score_rows(rng, P, L, vocab):
    lens = rng.integers(1, L + 1, P).astype(np.int32)
    lens[:4] = [1, 2, L - 1, L]
    ids = rng.integers(5, vocab, (P, L)).astype(np.int32)
    ids[:, 0] = X.XLMR_CLS
    ids[0, 0], ids[1, 1] = vocab - 1, 65536
    ids[np.arange(L)[None, :] >= lens[:, None]] = X.XLMR_PAD
    return ids, lens


@gpu
@pytest.mark.parametrize("hidden,heads,ffn", [(384, 12, 768), (128, 4, 512)], ids=["mx-384", "split16-128"])
def test_the_xlmr_loader_adds_no_arithmetic(tmp_path, hidden, heads, ffn):
    """An XLM-R checkpoint directory (vocab 70000, one token type) through LocalCrossEncoder.from_dir, and the same tensors
    relabelled by hand as a BERT with two identical type rows through flatten_state_dict + ce_load: bit-identical logits for the same
    id arrays (hidden 384 runs the MX forward and its load-time probe, which feeds token type 1; hidden 128 the split-fp16 one). With
    one token type, token_type_ids all 1 scores as all 0. The logits are the float64 BERT's at the project's 4e-3."""
    from optimized_rag_amd.cross_encoder import LocalCrossEncoder, flatten_state_dict
    hf = X.xlmr_hf_config(hidden=hidden, heads=heads, ffn=ffn)
    sd = X.seeded_xlmr(hf, 61)
    words = [f"w{i}" for i in range(40)]
    word_ids = np.linspace(4, 69999, len(words)).astype(int)
    path = X.write_checkpoint(tmp_path / "xlmr-ce", hf, sd, words, word_ids)
    rng = np.random.default_rng(62)
    P, L = 24, 64
    ids, lens = _score_rows(rng, P, L, 70000)
    zeros, ones = np.zeros_like(ids), np.ones_like(ids)
    e = _engine()
    try:
        ce = LocalCrossEncoder.from_dir(path, engine=e)
        assert (ce.pair_format, ce.cls_id, ce.sep_id, ce.vocab_size, ce.max_length) == (1, 0, 2, 70000, 64)
        assert ce.cfg["type_vocab"] == 1 and ce.cfg["max_pos"] == 64 and ce.cfg["eps"] == 1e-5
        got0 = e.ce_score(ids, zeros, lens)
        got1 = e.ce_score(ids, ones, lens)
        # the handle now assembles RoBERTa pairs, and predict() tokenises with the directory's tokenizer.json
        pairs = [(" ".join(rng.choice(words, int(a))), " ".join(rng.choice(words, int(b)))) for a, b in ((1, 1), (3, 9), (30, 40), (5, 70), (61, 2))]
        pid, ptt, plen = ce.tokenize_pairs(pairs)
        assert not ptt.any() and plen.max() == 64 and pid.max() > 65535 and (pid[:, 0] == 0).all()
        assert pid[0, :plen[0]].tolist()[2:4] == [2, 2]
        pred = ce.predict(pairs)
        np.testing.assert_array_equal(pred, e.ce_score(pid, ptt, plen))
    finally:
        e.close()
    bert = X.xlmr_to_bert_names(sd, type_rows=2)
    cfg = dict(vocab_size=70000, hidden=hidden, layers=2, heads=heads, ffn=ffn, max_pos=64, type_vocab=2, eps=1e-5)
    e = _engine()
    try:
        e.ce_load(cfg, flatten_state_dict(bert, 2))
        ref0 = e.ce_score(ids, zeros, lens)
        ref1 = e.ce_score(ids, ones, lens)
    finally:
        e.close()
    assert np.isfinite(got0).all()
    np.testing.assert_array_equal(got0, ref0)
    np.testing.assert_array_equal(got1, ref1)
    np.testing.assert_array_equal(got0, got1)
    exp = B.forward_logits(bert, cfg, ids.astype(np.int64), zeros.astype(np.int64), lens, fast_erf=True)
    err = float(np.abs(got0 - exp).max())
    print(f"hidden {hidden}: max |logit - float64 BERT on the relabelled tensors| = {err:.2e}")
    assert err < 4 * SCORE_TOL
    pexp = B.forward_logits(bert, cfg, pid.astype(np.int64), ptt.astype(np.int64), plen, fast_erf=True)
    assert np.abs(pred - pexp).max() < 4 * SCORE_TOL


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------
N, Q, POOL, K, LD, LQ, LP = 300, 5, 8, 4, 20, 14, 24
HF = X.xlmr_hf_config(hidden=384, heads=12, ffn=1536)


class World:
    """corpus, queries, model and the oracle's answers for both modes (numpy only: built once, shared, never changed)"""

    def __init__(self, seed):
        from optimized_rag_amd.cross_encoder import map_checkpoint
        rng = np.random.default_rng(1000 + seed)
        self.sd = X.seeded_xlmr(HF, 70 + seed)
        self.cfg, self.w = map_checkpoint(HF, self.sd)
        self.emb = rng.standard_normal((N, DIM)).astype(np.float32)
        self.q_emb = (self.emb[rng.integers(0, N, Q)] + 0.5 * rng.standard_normal((Q, DIM))).astype(np.float32)
        self.tok = rng.integers(5, 70000, (N, LD)).astype(np.int32)
        self.tok[:, 0] = 69999 - np.arange(N)                                            # every passage opens above 65535
        self.tok_len = rng.integers(3, LD + 1, N).astype(np.int32)
        self.tok_len[:5] = LD
        self.q_tok = rng.integers(5, 70000, (Q, LQ)).astype(np.int32)
        self.q_len = np.array([LQ, 3, 5, 9, 1], dtype=np.int32)
        self.tenants = (np.arange(N) % 3).astype(np.int32)
        self.corpus = [" ".join(f"t{t % 40}" for t in self.tok[i, :self.tok_len[i]]) for i in range(N)]
        self.queries = [" ".join(f"t{t % 40}" for t in self.q_tok[i, :self.q_len[i]]) for i in range(Q)]
        self.oracle = {hybrid: self._oracle(hybrid) for hybrid in (False, True)}

    def _oracle(self, hybrid):
        d_rows, _ = O.dense_topk(self.emb, self.q_emb, POOL)
        ocand = d_rows.astype(np.int64)
        if hybrid:
            obm = O.BM25Okapi([O.tokenize(c) for c in self.corpus])
            ocand = np.full((Q, POOL), -1, dtype=np.int64)
            for qi in range(Q):
                b_rows = O.stable_topk_desc(obm.get_scores(O.tokenize(self.queries[qi])), POOL)
                keys, _, _ = O.rrf_fuse([[int(r) for r in d_rows[qi]], [int(r) for r in b_rows]], k=60, top_k=POOL)
                ocand[qi, :len(keys)] = keys
        pid, ptt, plen = X.build_pairs(self.q_tok, self.q_len, ocand, self.tok, self.tok_len, LP, X.XLMR_CLS, X.XLMR_SEP, fmt=X.PAIR_ROBERTA)
        ologit = B.forward_logits(self.w, self.cfg, pid.astype(np.int64), ptt.astype(np.int64), plen, fast_erf=True).reshape(Q, POOL)
        oscore = np.array([[O.sigmoid(float(x)) for x in row] for row in ologit])
        order = [sorted(range(POOL), key=lambda j: -oscore[qi, j]) for qi in range(Q)]              # Python's stable sort, as the reference
        return dict(cand=ocand, logit=ologit, score=oscore, order=order)

    def min_gap(self):
        return min(float(np.abs(np.diff([o["score"][qi, j] for j in o["order"][qi][:K + 1]])).min()) for o in self.oracle.values() for qi in range(Q))


@pytest.fixture(scope="module")
def world():
    return World(WORLD_SEED)


def test_the_oracle_scores_of_the_end_to_end_world_are_well_separated(world):
    """CPU: in the oracle alone, every query's top k + 1 sigmoid scores are more than 2e-3 apart in both modes, so the device's
    1e-3 cannot reorder them and the GPU test below may demand the ids in order."""
    assert (world.oracle[False]["cand"] >= 0).all() and (world.oracle[True]["cand"] >= 0).all()
    assert world.tok.max() == 69999 and (world.tok[:, 0] > 65535).all()
    gap = world.min_gap()
    print("smallest gap between neighbouring oracle scores among the top k + 1:", gap)
    assert gap > 2 * SCORE_TOL


@pytest.fixture(scope="module")
def loaded(world):
    """one handle for the end-to-end checks: index, tenants, 24-bit store, BM25 postings, the mapped model, RoBERTa pairs"""
    from optimized_rag_amd.bm25 import Bm25Postings
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    e = _engine()
    e.index_load(world.emb)
    e.set_tenants(world.tenants)
    e.tokens_load(world.tok, world.tok_len, id_bits=24)
    e.ce_load(world.cfg, flatten_state_dict(world.w, world.cfg["layers"]))
    e.ce_set_pair_format(world.cfg["pair_format"])
    post = Bm25Postings.from_corpus(world.corpus).load(e)
    yield e, post
    e.close()


def _call(e, world, post, hybrid, rows=slice(None), tenant=-1):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    kw = {}
    if hybrid:
        ptr, terms = post.encode_queries(world.queries[rows])
        kw = dict(term_ptr=t(ptr), terms=t(terms))
    out = e.retrieve_rerank_dev(t(world.q_emb[rows]), t(world.q_tok[rows]), t(world.q_len[rows]), POOL, K, L_pair=LP, cls_id=world.cfg["cls_id"],
                                sep_id=world.cfg["sep_id"], tenant=tenant, **kw)
    torch.cuda.synchronize()
    return [x.cpu().numpy().copy() for x in out]


@gpu
@pytest.mark.parametrize("hybrid", [False, True], ids=["mode0", "mode1"])
def test_end_to_end_matches_the_oracle_composition_in_order(world, loaded, hybrid):
    e, post = loaded
    ids, sc, lg, cand = _call(e, world, post, hybrid)
    o = world.oracle[hybrid]
    assert world.min_gap() > 2 * SCORE_TOL
    np.testing.assert_array_equal(cand, o["cand"])                                       # candidates: bit-exact
    for qi in range(Q):
        top = o["order"][qi][:K]
        print(f"query {qi}: max |score - oracle| = {np.abs(sc[qi] - o['score'][qi, top]).max():.2e}, "
              f"max |logit - oracle| = {np.abs(lg[qi] - o['logit'][qi, top]).max():.2e}")
    for qi in range(Q):
        top = o["order"][qi][:K]
        np.testing.assert_allclose(sc[qi], o["score"][qi, top], atol=SCORE_TOL)
        np.testing.assert_allclose(lg[qi], o["logit"][qi, top], atol=4 * SCORE_TOL)
        assert ids[qi].tolist() == [int(o["cand"][qi, j]) for j in top], qi             # in order, every query


@gpu
def test_per_query_tenants_equal_the_scalar_calls_on_a_wide_store(world, loaded):
    e, post = loaded
    tenants = np.array([0, 1, -1, 2, 0], dtype=np.int32)
    for hybrid in (False, True):
        batch = _call(e, world, post, hybrid, tenant=tenants)
        for qi in range(Q):
            one = _call(e, world, post, hybrid, rows=slice(qi, qi + 1), tenant=int(tenants[qi]))
            for a, b in zip(batch, one):
                np.testing.assert_array_equal(a[qi:qi + 1].view(np.uint8), b.view(np.uint8))
        c = batch[3]
        for qi in range(Q):
            if tenants[qi] >= 0:
                assert (world.tenants[c[qi][c[qi] >= 0]] == tenants[qi]).all()


@gpu
def test_sharded_pipeline_at_world_1_equals_the_one_call_with_roberta_pairs(world, loaded):
    """ShardedPipeline inherits the handle's pair layout and store width without a change of its own."""
    import torch
    from optimized_rag_amd.sharded import ShardedPipeline
    e, post = loaded
    ref = _call(e, world, post, True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ptr, terms = post.encode_queries(world.queries)
    e.bm25_set_normalize(False)
    try:
        pipe = ShardedPipeline(e, rank=0, world=1)
        got = pipe.retrieve_rerank(t(world.q_emb), t(ptr), t(terms), t(world.q_tok), t(world.q_len), POOL, K, L_pair=LP, cls_id=world.cfg["cls_id"],
                                   sep_id=world.cfg["sep_id"])
        torch.cuda.synchronize()
        got = [x.cpu().numpy().copy() for x in got]
    finally:
        e.bm25_set_normalize(True)
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a, b)


# ---- 8. the embedder ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pooling", ["mean", "cls"])
def test_xlmr_embedder_through_the_service_loader(tmp_path, pooling):
    """An XLMRobertaModel-shaped encoder directory (names without a prefix, tokenizer.json, 1_Pooling/config.json) through
    LocalEmbeddingService.from_dir against the float64 oracle on the hand-relabelled tensors, at the bars of
    tests/test_embeddings_gpu.py: 1e-3 per component of the unit vector, cosine above 1 - 1e-6."""
    from optimized_rag_amd.embeddings import LocalEmbeddingService
    hf = X.xlmr_hf_config(hidden=384, heads=12, ffn=1536)
    sd = X.seeded_xlmr(hf, 81, head=False, prefix="")
    words = [f"w{i}" for i in range(60)]
    path = X.write_checkpoint(tmp_path / "xlmr-enc", hf, sd, words, np.linspace(4, 69999, len(words)).astype(int))
    (tmp_path / "xlmr-enc" / "1_Pooling").mkdir()
    (tmp_path / "xlmr-enc" / "1_Pooling" / "config.json").write_text(json.dumps(dict(
        word_embedding_dimension=384, pooling_mode_cls_token=pooling == "cls", pooling_mode_mean_tokens=pooling == "mean")))
    rng = np.random.default_rng(82)
    texts = [" ".join(rng.choice(words, int(n))) for n in (1, 2, 5, 17, 30, 61, 62, 80)]
    e = _engine(dim=384)
    try:
        svc = LocalEmbeddingService.from_dir(path, engine=e, max_length=64)
        assert svc.pooling == pooling and svc.cfg["type_vocab"] == 1 and svc.cfg["max_pos"] == 64 and svc.get_embedding_dimension() == 384
        ids, tt, lens = svc.tokenize(texts)
        assert lens.tolist() == [3, 4, 7, 19, 32, 63, 64, 64] and ids.max() > 65535 and (ids[:, 0] == 0).all() and not tt.any()
        got = np.asarray(svc.generate_embeddings_batch(texts), dtype=np.float64)
    finally:
        e.close()
    bert = X.xlmr_to_bert_names(sd, head=False)
    cfg = dict(vocab_size=70000, hidden=384, layers=2, heads=12, ffn=1536, max_pos=64, type_vocab=1, eps=1e-5)
    if pooling == "mean":
        exp = B.sentence_embeddings(bert, cfg, ids.astype(np.int64), tt.astype(np.int64), lens, fast_erf=True)
    else:
        _, hid = B.forward_hidden(bert, cfg, ids.astype(np.int64), tt.astype(np.int64), lens, fast_erf=True)
        exp = hid[:, 0] / np.linalg.norm(hid[:, 0], axis=1, keepdims=True)
    err, cos = float(np.abs(got - exp).max()), float((got * exp).sum(1).min())
    print(f"{pooling}: max component error {err:.2e}, 1 - min cosine {1 - cos:.2e}")
    assert err < 1e-3 and cos > 1 - 1e-6
