"""GPU: GpuDocumentIndex with device_query=True - the query tokenised on the host, then the forward, the lexical compaction and the
search on the device without a host round trip - returns exactly what the host-assembled path returns: the same dicts in the same
order, every score field compared with ==. On the fixture shape of tests/test_m3_tenants_service_gpu.py, with the embedding service
on the index's engine (rag_search_m3_tokens_tenants_dev) and on an engine of its own (the three-call form). add_texts, whose
per-token Python loop became rag_lexical_compact_dev, leaves the resident postings and the held mirror as that loop left them."""
import json
import logging

import numpy as np
import pytest

import m3_tools as M
import xlmr_tools as X

pytestmark = pytest.mark.gpu

AGENTS = ["a", "c", None, "b", "ghost", "a", "b", None, "c"]
WEIGHTS = [(0.4, 0.2, 0.4), (0.4, 0.2, 0.0), (0.0, 0.0, 1.0)]
WORDS = [f"w{i}" for i in range(60)]


def build(tmp, own_engine):
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.document_store import GpuDocumentIndex
    from optimized_rag_amd.embeddings import LocalEmbeddingService
    from optimized_rag_amd.sparse import LexicalPostings
    hf = X.xlmr_hf_config(vocab_size=64, hidden=128, layers=2, heads=4, ffn=256)
    sd = X.seeded_xlmr(hf, 9, head=False)
    X.write_checkpoint(tmp, hf, sd, words=WORDS)
    (tmp / "1_Pooling").mkdir()
    (tmp / "1_Pooling" / "config.json").write_text(json.dumps(dict(pooling_mode_cls_token=True, pooling_mode_mean_tokens=False)))
    M.write_head_files(tmp, M.seeded_heads(128, 96, 4))
    rng = np.random.default_rng(31)
    texts = [" ".join(rng.choice(WORDS[:30], int(rng.integers(2, 40)))) for _ in range(60)]
    agents = ["tiny" if i in (7, 23) else "abc"[i % 3] for i in range(60)]
    queries = [" ".join(rng.choice(WORDS[:24], int(rng.integers(1, 8)))) for _ in AGENTS]
    e = RagEngine(dim=128, device=0)
    e2 = RagEngine(dim=128, device=0) if own_engine else None
    svc = LocalEmbeddingService.from_dir(str(tmp), engine=e2 or e, max_length=64)
    index = GpuDocumentIndex(svc, dim=128, engine=e)
    rows = [dict(content=t, agent_id=a, filename=f"f{i}", metadata=dict(i=i), id=100 + 3 * i) for i, (t, a) in enumerate(zip(texts, agents))]
    index.bulk_load(rows, np.asarray(svc.generate_embeddings_batch(texts), dtype=np.float32))
    index.load_lexical(LexicalPostings.from_texts(svc, texts))
    index.build_token_vectors(texts, batch=16, headroom_docs=8, headroom_rows=8 * 64)
    return index, queries, [e, e2]


@pytest.fixture(scope="module", params=["one_engine", "two_engines"])
def service(request, tmp_path_factory):
    index, queries, engines = build(tmp_path_factory.mktemp("m3q"), request.param == "two_engines")
    yield index, queries
    for e in engines:
        if e is not None:
            e.close()


@pytest.fixture()
def spy(service, monkeypatch):
    """counts the calls of the one-call entry and of the host forward: which path a search took"""
    index, _ = service
    seen = dict(one_call=0, encode_multi=0)
    one, enc = index.engine.search_m3_tokens_dev, index.embeddings.encode_multi

    def one_call(*a, **kw):
        seen["one_call"] += 1
        return one(*a, **kw)

    def encode_multi(*a, **kw):
        seen["encode_multi"] += 1
        return enc(*a, **kw)

    monkeypatch.setattr(index.engine, "search_m3_tokens_dev", one_call)
    monkeypatch.setattr(index.embeddings, "encode_multi", encode_multi)
    return seen


@pytest.mark.parametrize("candidates", ["dense", "dense+sparse", "union"])
def test_search_m3_device_query_equals_the_host_path(service, spy, candidates):
    index, queries = service
    same_engine = index.embeddings.engine is index.engine
    for w in WEIGHTS:
        kw = dict(top_k=5, pool=20, weights=w, candidates=candidates)
        host = index.search_m3_many(AGENTS, queries, **kw)
        assert spy["one_call"] == 0 and spy["encode_multi"] == 1
        got = index.search_m3_many(AGENTS, queries, device_query=True, **kw)
        assert spy["encode_multi"] == 1 and spy["one_call"] == (1 if same_engine else 0)     # no host forward; the one call where it applies
        assert got == host
        assert got[4] == [] and all(len(m) == 5 for i, m in enumerate(got) if AGENTS[i] != "ghost")
        for a, q in list(zip(AGENTS, queries))[:5]:
            assert index.search_m3(a, q, device_query=True, **kw) == index.search_m3(a, q, **kw)
        spy.update(one_call=0, encode_multi=0)
    assert index.search_m3_many("b", queries, candidates=candidates, device_query=True) == index.search_m3_many("b", queries, candidates=candidates)
    assert index.search_m3_many("ghost", queries[:2], candidates=candidates, device_query=True) == [[], []]
    assert index.search_m3_many(AGENTS, [], device_query=True) == []
    # more than a pool of the union: the per-query form, as without device_query
    if candidates == "union":
        kw = dict(top_k=30, pool=20, candidates="union")
        assert index.search_m3_many(AGENTS, queries, device_query=True, **kw) == index.search_m3_many(AGENTS, queries, **kw)
        assert index.search_m3("a", queries[0], device_query=True, **kw) == index.search_m3("a", queries[0], **kw)


@pytest.mark.parametrize("mode", ["sparse", "dense+sparse"])
def test_search_lexical_many_device_query_equals_the_host_path(service, spy, mode):
    index, queries = service
    for kw in (dict(top_k=5, pool=20), dict(top_k=30, pool=10)):
        host = index.search_lexical_many(AGENTS, queries, mode=mode, **kw)
        n = spy["encode_multi"]
        got = index.search_lexical_many(AGENTS, queries, mode=mode, device_query=True, **kw)
        assert spy["encode_multi"] == n and got == host
        assert got[4] == [] and sum(len(m) for m in got) > 20
    assert index.search_lexical_many(None, queries[:2], mode=mode, device_query=True) == index.search_lexical_many(None, queries[:2], mode=mode)
    assert index.search_lexical_many("ghost", queries[:2], mode=mode, device_query=True) == [[], []]
    assert index.search_lexical_many(AGENTS, queries, mode="bm25", device_query=True) == [[] for _ in queries]


def test_a_service_without_token_ids_falls_back_with_one_logged_line(service, caplog):
    index, queries = service

    class Plain:
        """an embedding service that offers texts -> vectors and maps only"""
        def __init__(self, svc):
            self.encode_multi, self.generate_embedding, self.generate_embeddings_batch = svc.encode_multi, svc.generate_embedding, svc.generate_embeddings_batch

    svc = index.embeddings
    host = index.search_m3_many(AGENTS, queries, top_k=5, pool=20)
    index.embeddings = Plain(svc)
    try:
        with caplog.at_level(logging.INFO):
            assert index.search_m3_many(AGENTS, queries, top_k=5, pool=20, device_query=True) == host
        assert len([r for r in caplog.records if "device_query" in r.getMessage()]) == 1
    finally:
        index.embeddings = svc


def test_add_texts_leaves_the_postings_the_python_loop_left(service):
    """runs last in the module: it adds rows"""
    from optimized_rag_amd.sparse import LexicalPostings
    index, queries = service
    svc = index.embeddings
    new = [" ".join(WORDS[20:26]), " ".join(WORDS[3:9] + WORDS[3:5]), WORDS[11], " ".join(WORDS[10:12] * 9)]
    mirror = index._lexical
    expect = LexicalPostings(mirror.indptr.copy(), mirror.doc.copy(), mirror.weight.copy(), mirror.n_docs)
    info0 = index.engine.sparse_info()
    # the parent's loop: one forward per batch, lexical_map over every text, from_weights / extend
    skip = set(svc.special_ids())
    for part in (new[:3], new[3:]):                                      # add_texts(batch=3) forwards them in these batches
        ids, tt, lens = svc.tokenize(part)
        _, lx, _, _ = svc.engine.embed_multi(ids, tt, lens, dense=False, lexical=True, tokens=False)
        maps = [M.lexical_map(ids[i], lx[i], lens[i], skip) for i in range(len(part))]
        top = max((int(k) for m in maps for k in m), default=-1)
        expect.extend(LexicalPostings.from_weights(maps, max(expect.n_terms, top + 1)))
    got_ids = index.add_texts("fresh", new, batch=3)
    assert len(got_ids) == 4 and len(index.rows) == 64
    for name in ("indptr", "doc", "weight"):
        a, b = getattr(index._lexical, name), getattr(expect, name)
        assert a.dtype == b.dtype
        np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b,
                                      err_msg=name)
    info = index.engine.sparse_info()
    assert info["n_docs"] == expect.n_docs == 64 and info["nnz"] == expect.nnz > info0["nnz"] and info["n_terms"] == expect.n_terms
    # ... and a fresh load of the expected postings scores every document as the appended resident ones do
    ptr, terms, qw = LexicalPostings.encode_queries(svc.encode_multi(new + queries[:3], return_dense=False, return_colbert_vecs=False)["lexical_weights"])
    live = index.engine.sparse_scores(ptr, terms, qw)
    from optimized_rag_amd import RagEngine
    fresh = RagEngine(dim=128, device=0)
    try:
        expect.load(fresh)
        np.testing.assert_array_equal(live.view(np.int64), fresh.sparse_scores(ptr, terms, qw).view(np.int64))
    finally:
        fresh.close()
    assert (live[:4, 60:] > 0).any()
    for kw in (dict(candidates="union"), dict(candidates="dense", weights=(0.4, 0.2, 0.0))):
        agents, qs = ["fresh", None, "a"], [new[0], new[1], queries[0]]
        got = index.search_m3_many(agents, qs, top_k=3, pool=20, device_query=True, **kw)
        assert got == index.search_m3_many(agents, qs, top_k=3, pool=20, **kw) and got[0][0]["content"] == new[0]
