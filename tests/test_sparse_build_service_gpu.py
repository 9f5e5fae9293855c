"""GPU: GpuDocumentIndex.build_lexical - the lexical postings built on the device from the forward's output (rag_lexical_compact_dev
into rag_sparse_append_dev), no host mirror - against a TWIN index over the same rows whose postings went the host way
(LexicalPostings.from_texts + load_lexical). Every search returns the same dicts with == on every score field, before and after
add_texts (device route against mirror route), add_rows(lexical_weights=...) and compact(keep_resident=True); the exported
postings equal the twin's mirror arrays. The model is the seeded small m3-shaped checkpoint of tests/m3_tools.py /
tests/xlmr_tools.py that the other service tests use (tests/m3_model.py holds no checkpoint)."""
import json

import numpy as np
import pytest

import m3_tools as M
import xlmr_tools as X

pytestmark = pytest.mark.gpu

WORDS = [f"w{i}" for i in range(60)]
AGENTS = ["a", "c", None, "b", "ghost", "a"]


def twin_indexes(tmp):
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.document_store import GpuDocumentIndex
    from optimized_rag_amd.embeddings import LocalEmbeddingService
    from optimized_rag_amd.sparse import LexicalPostings, ResidentLexical
    hf = X.xlmr_hf_config(vocab_size=64, hidden=128, layers=2, heads=4, ffn=256)
    X.write_checkpoint(tmp, hf, X.seeded_xlmr(hf, 9, head=False), words=WORDS)
    (tmp / "1_Pooling").mkdir()
    (tmp / "1_Pooling" / "config.json").write_text(json.dumps(dict(pooling_mode_cls_token=True, pooling_mode_mean_tokens=False)))
    M.write_head_files(tmp, M.seeded_heads(128, 96, 4))
    rng = np.random.default_rng(31)
    texts = [" ".join(rng.choice(WORDS[:30], int(rng.integers(2, 40)))) for _ in range(60)]
    agents = ["abc"[i % 3] for i in range(60)]
    queries = [" ".join(rng.choice(WORDS[:24], int(rng.integers(1, 8)))) for _ in AGENTS]
    out, engines = [], []
    for device_built in (True, False):
        e = RagEngine(dim=128, device=0)
        engines.append(e)
        svc = LocalEmbeddingService.from_dir(str(tmp), engine=e, max_length=64)
        index = GpuDocumentIndex(svc, dim=128, engine=e)
        rows = [dict(content=t, agent_id=a, document_id=i // 4, filename=f"f{i}", metadata=dict(i=i), id=100 + 3 * i)
                for i, (t, a) in enumerate(zip(texts, agents))]
        index.bulk_load(rows, np.asarray(svc.generate_embeddings_batch(texts), dtype=np.float32))
        if device_built:
            index.build_lexical(texts, batch=16)                     # four blocks: a base and three appends
            assert isinstance(index._lexical, ResidentLexical) and (index._lexical.n_docs, index._lexical.n_terms) == (60, 64)
        else:
            index.load_lexical(LexicalPostings.from_texts(svc, texts))
        index.build_token_vectors(texts, batch=16, headroom_docs=16, headroom_rows=16 * 64)
        out.append(index)
    return out, queries, engines


@pytest.fixture()
def twins(tmp_path):
    """built per test: the second test adds and removes rows"""
    (dev, host), queries, engines = twin_indexes(tmp_path)
    yield dev, host, queries
    for e in engines:
        e.close()


def searches(index, queries):
    out = {}
    for mode in ("sparse", "dense+sparse"):
        out["lexical " + mode] = [index.search_lexical(a, q, top_k=8, mode=mode, pool=30) for a, q in zip(AGENTS, queries)]
        out["lexical many " + mode] = index.search_lexical_many(AGENTS, queries, top_k=8, mode=mode, pool=30)
    for cand in ("dense", "dense+sparse", "union"):
        out["m3 " + cand] = [index.search_m3(a, q, top_k=5, pool=20, candidates=cand) for a, q in zip(AGENTS, queries)]
    assert sum(len(r) for r in out["lexical sparse"]) > 20 and sum(len(r) for r in out["m3 union"]) > 15
    return out


def same_postings(dev, host):
    got = dev._lexical.export(dev.engine)
    for name in ("indptr", "doc", "weight"):
        a, b = getattr(got, name), getattr(host._lexical, name)
        assert a.dtype == b.dtype and a.shape == b.shape, name
        np.testing.assert_array_equal(a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b, err_msg=name)
    assert (got.n_docs, got.n_terms) == (host._lexical.n_docs, host._lexical.n_terms) == (dev._lexical.n_docs, dev._lexical.n_terms)


def test_build_lexical_equals_from_texts_and_load_lexical(twins):
    dev, host, queries = twins
    assert dev.engine.sparse_info()["n_docs"] == host.engine.sparse_info()["n_docs"] == 60
    same_postings(dev, host)
    assert searches(dev, queries) == searches(host, queries)
    with pytest.raises(ValueError):
        dev.build_lexical(["one text"])


def test_live_writes_over_device_built_postings_equal_the_mirror_route(twins):
    from optimized_rag_amd.sparse import ResidentLexical
    dev, host, queries = twins
    new = [" ".join(WORDS[20:26]), " ".join(WORDS[3:9] + WORDS[3:5]), WORDS[11], " ".join(WORDS[10:12] * 9), " ".join(WORDS[25:30])]
    ids = [index.add_texts("a", new[:3], batch=2, document_id=40) + index.add_texts("b", new[3:], document_id=41) for index in (dev, host)]
    assert ids[0] == ids[1] and len(ids[0]) == 5
    assert isinstance(dev._lexical, ResidentLexical) and dev._lexical.n_docs == 65 == dev.engine.sparse_info()["n_docs"]
    same_postings(dev, host)
    assert searches(dev, queries) == searches(host, queries)
    hit = dev.search_lexical("a", new[0], top_k=10, mode="sparse")
    assert any(r["content"] == new[0] for r in hit), "the appended row is not among the lexical hits of its own text"
    # add_rows with host maps: one doc-major block through rag_sparse_append_docs_host / the mirror's term-major block
    svc = dev.embeddings
    more = [" ".join(WORDS[1:7]), WORDS[29]]
    maps = svc.encode_multi(more, return_dense=False, return_sparse=True, return_colbert_vecs=False)["lexical_weights"]
    emb = np.asarray(svc.generate_embeddings_batch(more), dtype=np.float32)
    for index in (dev, host):
        ids, tt, lens = index.embeddings.tokenize(more)
        _, _, tk, off = index.embeddings.engine.embed_multi(ids, tt, lens, dense=False, lexical=False, tokens=True)
        index.add_rows([dict(content=t, agent_id="c", document_id=42, metadata={}) for t in more], emb, lexical_weights=maps, token_vectors=(tk, off))
    with pytest.raises(ValueError):                                  # checked before anything is written, as with the mirror
        dev.add_rows([dict(content="x", agent_id="c")], emb[:1], lexical_weights=[{3: float("nan")}])
    assert len(dev.rows) == 67 and dev._lexical.n_docs == 67
    same_postings(dev, host)
    assert searches(dev, queries) == searches(host, queries)
    # delete two documents (one of them appended), compact with the resident legs kept
    for index in (dev, host):
        assert index.delete_document("a", 40) and index.delete_document("b", 2)
        rm = index.compact(keep_resident=True)
        assert (rm < 0).sum() >= 4
    assert dev._lexical.n_docs == host._lexical.n_docs == len(dev.rows) == dev.engine.sparse_info()["n_docs"]
    same_postings(dev, host)
    assert searches(dev, queries) == searches(host, queries)
    # a plain compaction drops the stand-in as it drops the mirror
    for index in (dev, host):
        assert index.delete_document("c", 42)
        index.compact()
        assert index._lexical is None and index.search_lexical("a", queries[0], top_k=5) == []
