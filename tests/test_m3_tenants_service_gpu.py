"""GPU: GpuDocumentIndex.search_lexical_many / search_m3_many - a batch of queries with ONE AGENT PER QUERY over a seeded
bge-m3-shaped checkpoint directory (built as tests/test_sparse_service_gpu.py and tests/test_m3_fused_gpu.py build theirs).

Element i of a batched result equals the single-query method's answer for (agent_id[i], queries[i]): the same dicts in the same
order, every score field compared with ==. The single-query methods are held against the float64 references by their own tests."""
import json

import numpy as np
import pytest

import m3_tools as M
import xlmr_tools as X

pytestmark = pytest.mark.gpu

AGENTS = ["a", "c", None, "b", "ghost", "a", "b", None, "c"]


@pytest.fixture(scope="module")
def service(tmp_path_factory):
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.document_store import GpuDocumentIndex
    from optimized_rag_amd.embeddings import LocalEmbeddingService
    from optimized_rag_amd.sparse import LexicalPostings
    words = [f"w{i}" for i in range(60)]
    hf = X.xlmr_hf_config(vocab_size=64, hidden=128, layers=2, heads=4, ffn=256)
    sd = X.seeded_xlmr(hf, 9, head=False)
    d = tmp_path_factory.mktemp("m3")
    X.write_checkpoint(d, hf, sd, words=words)
    (d / "1_Pooling").mkdir()
    (d / "1_Pooling" / "config.json").write_text(json.dumps(dict(pooling_mode_cls_token=True, pooling_mode_mean_tokens=False)))
    M.write_head_files(d, M.seeded_heads(128, 96, 4))
    rng = np.random.default_rng(31)
    texts = [" ".join(rng.choice(words[:30], int(rng.integers(2, 40)))) for _ in range(60)]
    agents = ["tiny" if i in (7, 23) else "abc"[i % 3] for i in range(60)]
    queries = [" ".join(rng.choice(words[:24], int(rng.integers(1, 8)))) for _ in AGENTS]
    e = RagEngine(dim=128, device=0)
    svc = LocalEmbeddingService.from_dir(str(d), engine=e, max_length=64)
    index = GpuDocumentIndex(svc, dim=128, engine=e)
    rows = [dict(content=t, agent_id=a, filename=f"f{i}", metadata=dict(i=i), id=100 + 3 * i) for i, (t, a) in enumerate(zip(texts, agents))]
    index.bulk_load(rows, np.asarray(svc.generate_embeddings_batch(texts), dtype=np.float32))
    index.load_lexical(LexicalPostings.from_texts(svc, texts))
    index.build_token_vectors(texts, batch=16, headroom_docs=8, headroom_rows=8 * 64)
    yield index, queries, words
    e.close()


def singles_lexical(index, agents, queries, **kw):
    return [index.search_lexical(a, q, **kw) for a, q in zip(agents, queries)]


def singles_m3(index, agents, queries, **kw):
    return [index.search_m3(a, q, **kw) for a, q in zip(agents, queries)]


@pytest.mark.parametrize("mode", ["sparse", "dense+sparse"])
def test_search_lexical_many_equals_the_single_calls(service, mode):
    index, queries, _ = service
    for kw in (dict(top_k=5, pool=20), dict(top_k=30, pool=10)):
        many = index.search_lexical_many(AGENTS, queries, mode=mode, **kw)
        single = singles_lexical(index, AGENTS, queries, mode=mode, **kw)
        assert many == single
        assert many[4] == [] and sum(len(m) for m in many) > 20
        keys = {"content", "filename", "file_type", "metadata", "score", "sparse_score"} | ({"rrf_score"} if mode != "sparse" else set())
        assert all(set(r) == keys for m in many for r in m)
    if mode != "sparse":
        assert any(r["sparse_score"] == 0.0 for m in many for r in m) and any(r["sparse_score"] > 0.0 for m in many for r in m)
    assert index.search_lexical_many("a", queries, mode=mode) == index.search_lexical_many(["a"] * len(queries), queries, mode=mode) == \
        singles_lexical(index, ["a"] * len(queries), queries, mode=mode)
    assert index.search_lexical_many(None, queries[:2], mode=mode) == singles_lexical(index, [None, None], queries[:2], mode=mode)
    assert index.search_lexical_many("ghost", queries[:2], mode=mode) == [[], []]
    assert index.search_lexical_many(["a"], queries[:2], mode=mode) == [[], []]                     # a list of the wrong length: logged, empty
    assert index.search_lexical_many(AGENTS, queries, mode="bm25") == [[] for _ in queries]
    assert index.search_lexical_many(AGENTS, []) == []


@pytest.mark.parametrize("candidates", ["dense", "dense+sparse", "union"])
def test_search_m3_many_equals_the_single_calls(service, candidates):
    index, queries, _ = service
    for kw in (dict(top_k=5, pool=20), dict(top_k=4, pool=60, weights=(0.4, 0.2, 0.0)), dict(top_k=6, pool=3, weights=(0.0, 0.0, 1.0))):
        many = index.search_m3_many(AGENTS, queries, candidates=candidates, **kw)
        single = singles_m3(index, AGENTS, queries, candidates=candidates, **kw)
        assert many == single
        assert many[4] == [] and all(len(m) == kw["top_k"] for i, m in enumerate(many) if AGENTS[i] in ("a", "b", "c", None))
        keys = {"content", "filename", "file_type", "score", "dense_score", "sparse_score", "colbert_score", "metadata"}
        assert all(set(r) == keys for m in many for r in m)
    assert index.search_m3_many("b", queries, candidates=candidates) == index.search_m3_many(["b"] * len(queries), queries, candidates=candidates) == \
        singles_m3(index, ["b"] * len(queries), queries, candidates=candidates)
    assert index.search_m3_many("ghost", queries[:2], candidates=candidates) == [[], []]


def test_tiny_agents_live_writes_and_failures(service):
    index, queries, words = service
    agents = ["tiny", "a", "tiny"]
    many = index.search_m3_many(agents, queries[:3], top_k=5, pool=20)
    assert many == singles_m3(index, agents, queries[:3], top_k=5, pool=20) and len(many[0]) == 2 and len(many[1]) == 5
    assert index.search_lexical_many(agents, queries[:3], top_k=5, pool=20) == singles_lexical(index, agents, queries[:3], top_k=5, pool=20)
    # rows added live, for a new agent and a known one: the batched forms see them as the single calls do
    new = [" ".join(words[20:26]), " ".join(words[3:9]), " ".join(words[10:12])]
    ids = index.add_texts("fresh", new[:2]) + index.add_texts("a", new[2:])
    assert len(ids) == 3 and len(index.rows) == 63
    agents = ["fresh", "a", None, "fresh"]
    qs = [new[0], new[2], new[1], queries[0]]
    for cands in ("dense", "union"):
        many = index.search_m3_many(agents, qs, top_k=3, pool=20, candidates=cands)
        assert many == singles_m3(index, agents, qs, top_k=3, pool=20, candidates=cands)
        assert many[0][0]["content"] == new[0] and len(many[0]) == 2 and many[2][0]["content"] == new[1]
    for mode in ("sparse", "dense+sparse"):
        many = index.search_lexical_many(agents, qs, top_k=3, pool=20, mode=mode)
        assert many == singles_lexical(index, agents, qs, top_k=3, pool=20, mode=mode) and many[0][0]["content"] == new[0]
    # a failure is answered as the single-query methods answer it: search_many for the three-way form, [] for the lexical one
    plain = index.search_many(agents, qs, top_k=3, with_embeddings=False)
    assert index.search_m3_many(agents, qs, top_k=3, candidates="bm25") == plain
    assert index.search_m3_many(agents, qs, top_k=3, weights=(0.0, 0.0, 0.0)) == plain
    index.engine.tokvec_reserve(1, 0, 96)                                # the store dropped
    assert index.search_m3_many(agents, qs, top_k=3, pool=20) == plain
    assert index.search_m3_many(agents, qs, top_k=3, pool=20, weights=(0.4, 0.2, 0.0)) == \
        singles_m3(index, agents, qs, top_k=3, pool=20, weights=(0.4, 0.2, 0.0))
