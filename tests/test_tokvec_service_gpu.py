"""GPU: GpuDocumentIndex.build_token_vectors / load_token_vectors / search_late_interaction on a seeded checkpoint directory with
bge-m3's head files (m3_tools.write_head_files), against the float64 reference of tests/m3_tools.py: every returned colbert_score
within 1e-3 of the reference's MaxSim for that row, the list in the order of the device's own scores, nothing better left out of
it, and any failure answered with `search`."""
import json

import numpy as np
import pytest

import m3_tools as M
import xlmr_tools as X

pytestmark = pytest.mark.gpu


def test_build_search_and_fallback(tmp_path):
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.document_store import GpuDocumentIndex
    from optimized_rag_amd.embeddings import LocalEmbeddingService
    from optimized_rag_amd.sparse import LexicalPostings
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
    w = X.xlmr_to_bert_names(sd, head=False)
    rng = np.random.default_rng(12)
    query = " ".join(rng.choice(words[:20], 6))
    texts = [" ".join(rng.choice(words[:30], int(rng.integers(2, 40)))) for _ in range(40)]
    agents = ["a" if i % 4 else "b" for i in range(40)]
    # the float64 reference: MaxSim of the query's token vectors against every text's
    enc = X.roberta_tokenizer(words).encode_batch([query] + texts)
    pl = np.array([len(x.ids) for x in enc], dtype=np.int32)
    pi = np.zeros((len(enc), int(pl.max())), dtype=np.int32)
    for i, x in enumerate(enc):
        pi[i, :pl[i]] = x.ids
    ref = M.heads_reference(w, cfg, pi, np.zeros_like(pi), pl, heads)
    exp = np.array([M.maxsim(ref["vecs"][0], ref["vecs"][1 + i]) for i in range(40)])
    e = RagEngine(dim=128, device=0)
    try:
        svc = LocalEmbeddingService.from_dir(str(d), engine=e, max_length=64)
        index = GpuDocumentIndex(svc, dim=128, engine=e)
        rows = [dict(content=t, agent_id=a, filename=f"f{i}", metadata=dict(i=i)) for i, (t, a) in enumerate(zip(texts, agents))]
        index.bulk_load(rows, np.asarray(svc.generate_embeddings_batch(texts), dtype=np.float32))
        # without token vectors the method answers with `search`
        plain = index.search("a", query, top_k=5, with_embeddings=False)
        assert len(plain) == 5 and index.search_late_interaction("a", query, top_k=5) == plain
        index.build_token_vectors(texts, batch=16)
        info = e.tokvec_info()
        assert info["n_docs"] == 40 and info["dim"] == 96 and info["rows"] == int((pl[1:] - 1).sum())
        row_of = {t["filename"]: i for i, t in enumerate(rows)}

        def check(res, agent, top_k, pool):
            assert len(res) == top_k and all(set(r) == {"content", "filename", "file_type", "score", "colbert_score", "metadata"} for r in res)
            got = [row_of[r["filename"]] for r in res]
            sc = np.array([r["colbert_score"] for r in res])
            assert all(agents[i] == agent for i in got) and all(r["score"] == r["colbert_score"] for r in res)
            err = float(np.abs(sc - exp[got]).max())
            assert err < 1e-3, err
            assert (np.diff(sc) <= 0).all(), "not in the order of the device's scores"
            cands = [row_of[r["filename"]] for r in index.search(agent, query, top_k=pool, with_embeddings=False)]
            assert set(got) <= set(cands)
            rest = [i for i in cands if i not in got]
            assert not rest or exp[rest].max() <= sc.min() + 1e-3, "a better candidate was left out"
            return err

        res = index.search_late_interaction("a", query, top_k=5, pool=20)
        err = check(res, "a", 5, 20)
        print(f"search_late_interaction: max |colbert_score - float64 MaxSim| = {err:.3e}")
        check(index.search_late_interaction("b", query, top_k=3, pool=8), "b", 3, 8)
        assert index.search_late_interaction("nobody", query, top_k=5) == []
        # dense + sparse candidates: every row of the agent is a candidate at this pool, so the list is the agent's best by MaxSim
        index.load_lexical(LexicalPostings.from_texts(svc, texts))
        fused = index.search_late_interaction("a", query, top_k=5, pool=40, mode="dense+sparse")
        assert [r["filename"] for r in fused] == [r["filename"] for r in index.search_late_interaction("a", query, top_k=5, pool=40)]
        # vectors kept from an ingest and loaded from host arrays give the same store, hence the same list
        vecs = svc.encode_multi(texts, return_dense=False, return_sparse=False)["colbert_vecs"]
        index.load_token_vectors(*M.pack(vecs, 96))
        assert index.search_late_interaction("a", query, top_k=5, pool=20) == res
        # an induced failure falls back to `search`, and so does an unknown mode
        def boom(*a, **k):
            raise RuntimeError("induced")
        real, e.tokvec_rerank = e.tokvec_rerank, boom
        try:
            assert index.search_late_interaction("a", query, top_k=5, pool=20) == plain
        finally:
            e.tokvec_rerank = real
        assert index.search_late_interaction("a", query, top_k=5, mode="bm25") == plain
        # token vectors of another width than the embedder's head: refused, not read past their end
        index.load_token_vectors(*M.pack([v[:, :64] for v in vecs], 64))
        assert index.search_late_interaction("a", query, top_k=5, pool=20) == plain
        index.load_token_vectors(*M.pack(vecs, 96))
        with pytest.raises(ValueError):
            GpuDocumentIndex(svc, dim=128, engine=e).build_token_vectors([])
        index.build_token_vectors(texts, batch=0)                        # a batch size below 1 counts as 1
        assert index.search_late_interaction("a", query, top_k=5, pool=20) == res
    finally:
        e.close()
