"""GPU: GpuDocumentIndex keeps its lexical and late-interaction legs live through writes, on the seeded checkpoint directory of
tests/m3_tools.py / tests/xlmr_tools.py: add_texts makes the new rows findable by search_lexical and search_late_interaction
without any reload, and delete_document + compact(keep_resident=True) leaves both searches answering exactly what an index
built from scratch over the surviving texts answers."""
import json

import numpy as np
import pytest

import m3_tools as M
import xlmr_tools as X

pytestmark = pytest.mark.gpu


def build(svc, e, texts, agents, docs, headroom=(0, 0)):
    from optimized_rag_amd.document_store import GpuDocumentIndex
    from optimized_rag_amd.sparse import LexicalPostings
    index = GpuDocumentIndex(svc, dim=128, engine=e)
    rows = [dict(content=t, agent_id=a, document_id=d, filename=t, metadata={}) for t, a, d in zip(texts, agents, docs)]
    index.bulk_load(rows, np.asarray(svc.generate_embeddings_batch(texts), dtype=np.float32))
    index.load_lexical(LexicalPostings.from_texts(svc, texts))
    index.build_token_vectors(texts, batch=16, headroom_docs=headroom[0], headroom_rows=headroom[1])
    return index


def hits(index, agent, query):
    out = {}
    for mode in ("sparse", "dense+sparse"):
        out["lexical " + mode] = [(r["content"], r["score"], r["sparse_score"]) for r in index.search_lexical(agent, query, top_k=8, mode=mode, pool=30)]
    for mode in ("dense", "dense+sparse"):
        out["late " + mode] = [(r["content"], r["colbert_score"]) for r in index.search_late_interaction(agent, query, top_k=8, pool=30, mode=mode)]
        assert all("colbert_score" in r for r in index.search_late_interaction(agent, query, top_k=8, pool=30, mode=mode))
    return out


def test_add_texts_delete_document_and_compact_keep_every_leg_live(tmp_path):
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.embeddings import LocalEmbeddingService
    words = [f"w{i}" for i in range(60)]
    hf = X.xlmr_hf_config(vocab_size=64, hidden=128, layers=2, heads=4, ffn=256)
    sd = X.seeded_xlmr(hf, 9, head=False)
    d = tmp_path / "m3"
    X.write_checkpoint(d, hf, sd, words=words)
    (d / "1_Pooling").mkdir()
    (d / "1_Pooling" / "config.json").write_text(json.dumps(dict(pooling_mode_cls_token=True, pooling_mode_mean_tokens=False)))
    M.write_head_files(d, M.seeded_heads(128, 96, 4))
    rng = np.random.default_rng(12)
    texts = list(dict.fromkeys(" ".join(rng.choice(words[:30], int(rng.integers(2, 40)))) for _ in range(60)))[:52]
    assert len(texts) == 52
    agents = ["a" if i % 4 else "b" for i in range(52)]
    docs = [i // 4 for i in range(52)]                               # documents of four chunks
    query = " ".join(rng.choice(words[:20], 6))
    e, e2 = RagEngine(dim=128, device=0), RagEngine(dim=128, device=0)
    try:
        svc = LocalEmbeddingService.from_dir(str(d), engine=e, max_length=64)
        svc2 = LocalEmbeddingService.from_dir(str(d), engine=e2, max_length=64)
        index = build(svc, e, texts[:40], agents[:40], docs[:40], headroom=(16, 16 * 64))
        # 12 more texts, all three heads from one forward per batch: nothing is reloaded
        for at in (40, 47):
            n = 7 if at == 40 else 5
            for doc_id in sorted(set(docs[at:at + n])):
                sel = [i for i in range(at, at + n) if docs[i] == doc_id]
                for agent in ("a", "b"):
                    part = [texts[i] for i in sel if agents[i] == agent]
                    if part:
                        index.add_texts(agent, part, batch=3, document_id=doc_id)
        assert e.tokvec_info()["n_docs"] == 52 and e.sparse_info()["n_docs"] == 52 and len(index.rows) == 52
        # the rows are in another order than texts[] (grouped by agent inside a document): compare by content
        order = [r["content"] for r in index.rows]
        scratch = build(svc2, e2, order, [r["agent_id"] for r in index.rows], [r["document_id"] for r in index.rows])
        for agent in ("a", "b"):
            got = hits(index, agent, query)
            assert got == hits(scratch, agent, query), agent
            assert all(len(v) == 8 for v in got.values())
        new = set(texts[40:])
        wide = index.search_lexical("a", " ".join(texts[45].split()[:6]), top_k=30, mode="sparse")
        assert any(r["content"] in new for r in wide), "no appended row among the lexical hits"
        late = index.search_late_interaction("a", texts[45], top_k=3, pool=30)
        assert late and late[0]["content"] == texts[45] and "colbert_score" in late[0]
        # delete three documents (one of them appended), compact, and compare with an index over the surviving texts
        for doc_id in (0, 5, 11):
            for agent in ("a", "b"):
                assert index.delete_document(agent, doc_id)
        rm = index.compact(keep_resident=True)
        assert (rm < 0).sum() == 12 and len(index.rows) == 40
        assert e.tokvec_info()["n_docs"] == 40 and e.sparse_info()["n_docs"] == 40 and index._lexical.n_docs == 40
        left = [r["content"] for r in index.rows]
        scratch = build(svc2, e2, left, [r["agent_id"] for r in index.rows], [r["document_id"] for r in index.rows])
        for agent in ("a", "b"):
            got = hits(index, agent, query)
            assert got == hits(scratch, agent, query), agent
            assert all(len(v) == 8 for v in got.values())
        # the default compaction still leaves both legs stale
        assert index.delete_document("a", 3)
        index.compact()
        assert index.search_lexical("a", query, top_k=5) == []
    finally:
        e.close()
        e2.close()
