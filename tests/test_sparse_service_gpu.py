"""GPU, end to end: a checkpoint directory with the lexical head -> LocalEmbeddingService -> LexicalPostings.from_texts ->
GpuDocumentIndex.load_lexical / search_lexical. The sparse list is the float64 reference of tests/sparse_tools.py on the very
maps `encode_multi` returned (documents, order and score bits); each score also agrees with the pairwise rag_lexical_match_* of
the same (query, passage) to relative 2^-22 (that call returns the float32 of a float64 sum taken in another order: one float32
rounding, 2^-24, with room for the sum's own float64 error); the fused list is the oracle's RRF of `search`'s dense list and
the sparse list."""
import json
import logging

import numpy as np
import pytest

import m3_tools as M
import sparse_tools as S
import xlmr_tools as X

pytestmark = pytest.mark.gpu


def as_rows(maps):
    """{token id: weight} maps as the padded (ids, weights, lens) rows rag_lexical_match_* takes."""
    L = max(1, max(len(m) for m in maps))
    ids, w = np.zeros((len(maps), L), dtype=np.int32), np.zeros((len(maps), L), dtype=np.float32)
    for i, m in enumerate(maps):
        ids[i, :len(m)], w[i, :len(m)] = list(m.keys()), list(m.values())
    return ids, w, np.array([len(m) for m in maps], dtype=np.int32)


def test_lexical_index_and_search_from_a_checkpoint_directory(tmp_path, caplog):
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.document_store import GpuDocumentIndex
    from optimized_rag_amd.embeddings import LocalEmbeddingService
    from optimized_rag_amd.sparse import LexicalPostings
    from oracle import rag_oracle as O
    words = [f"w{i}" for i in range(60)]
    hf = X.xlmr_hf_config(vocab_size=64, hidden=128, layers=2, heads=4, ffn=256)
    sd = X.seeded_xlmr(hf, 9, head=False)
    heads = M.seeded_heads(128, 96, 4)
    plain, full = tmp_path / "plain", tmp_path / "m3"
    for d in (plain, full):
        X.write_checkpoint(d, hf, sd, words=words)
        (d / "1_Pooling").mkdir()
        (d / "1_Pooling" / "config.json").write_text(json.dumps(dict(pooling_mode_cls_token=True, pooling_mode_mean_tokens=False)))
    M.write_head_files(full, heads)
    rng = np.random.default_rng(17)
    # passages over word subsets of their own, so that a query shares tokens with some passages and with others none
    texts = []
    for i in range(300):
        lo = int(rng.integers(0, 40))
        texts.append(" ".join(rng.choice(words[lo:lo + 20], int(rng.integers(3, 30)))))
    # (w59 occurs in no passage: that query's sparse list is empty, and its fused list is the dense list's order)
    queries = [" ".join(rng.choice(words[:12], 4)), " ".join(rng.choice(words[30:60], 7)), words[59], " ".join(rng.choice(words, 12))]
    e = RagEngine(dim=128, device=0)
    try:
        svc = LocalEmbeddingService.from_dir(str(full), engine=e, max_length=64)
        assert svc.has_lexical_head
        post = LexicalPostings.from_texts(svc, texts, batch=128)
        assert post.n_docs == 300 and post.n_terms == 64 and post.nnz > 300
        maps = []                                                    # the same forwards, batch by batch: the same bits
        for b in range(0, 300, 128):
            maps += svc.encode_multi(texts[b:b + 128], return_dense=False, return_colbert_vecs=False)["lexical_weights"]
        assert all(maps) and len(set(texts)) == 300
        ref_post = LexicalPostings.from_weights(maps, 64)
        for a, b in ((post.indptr, ref_post.indptr), (post.doc, ref_post.doc), (post.weight, ref_post.weight)):
            np.testing.assert_array_equal(a, b)
        index = GpuDocumentIndex(svc, dim=128, engine=e)
        agents = ["a" if i % 3 else "b" for i in range(300)]
        index.bulk_load([dict(content=t, agent_id=agents[i], filename=f"f{i}") for i, t in enumerate(texts)],
                        np.asarray(svc.generate_embeddings_batch(texts), dtype=np.float32))
        with pytest.raises(ValueError):
            index.load_lexical(post.shard(0, 299))
        index.load_lexical(post)
        d_ids, d_w, d_lens = as_rows(maps)
        for qi, query in enumerate(queries):
            qmap = svc.encode_multi([query], return_dense=False, return_colbert_vecs=False)["lexical_weights"][0]
            ptr, terms, wts = LexicalPostings.encode_queries([qmap])
            s = S.scores(post.indptr, post.doc, post.weight, 300, terms, wts)
            for agent, hidden in (("a", np.array([x != "a" for x in agents])), (None, None)):
                top_k = 25
                rows, sc = S.topk(s, top_k, hidden=hidden)
                n = int((rows >= 0).sum())
                got = index.search_lexical(agent, query, top_k, mode="sparse")
                assert [g["content"] for g in got] == [texts[r] for r in rows[:n]] and [g["filename"] for g in got] == [f"f{r}" for r in rows[:n]]
                np.testing.assert_array_equal(S.bits([g["sparse_score"] for g in got]), S.bits(sc[:n]))
                assert all(g["score"] == g["sparse_score"] and "rrf_score" not in g for g in got)
                if n:
                    q_ids, q_w, q_lens = as_rows([qmap])
                    pair = e.lexical_match(q_ids, q_w, q_lens, d_ids, d_w, d_lens, np.zeros(n, dtype=np.int32), rows[:n].astype(np.int32)).astype(np.float64)
                    rel = np.abs(pair - sc[:n]) / sc[:n]
                    print(f"query {qi} agent {agent}: {n} hits, max relative |lexical_match - sparse score| = {rel.max():.3e}")
                    assert rel.max() <= 2.0 ** -22
                # fused: RRF of search's dense list and the sparse list, dense first
                pool, k = 40, 10
                dense = [d["content"] for d in index.search(agent, query, top_k=pool, with_embeddings=False)]
                srows, _ = S.topk(s, pool, hidden=hidden)
                sparse = [texts[r] for r in srows if r >= 0]
                o_keys, o_sc, _ = O.rrf_fuse([dense, sparse], k=60, top_k=k)
                fused = index.search_lexical(agent, query, k, mode="dense+sparse", pool=pool)
                assert [g["content"] for g in fused] == o_keys
                np.testing.assert_array_equal(S.bits([g["rrf_score"] for g in fused]), S.bits(o_sc))
                smap = {texts[r]: float(v) for r, v in zip(*S.topk(s, pool, hidden=hidden)) if r >= 0}
                assert all(g["score"] == g["rrf_score"] and g["sparse_score"] == smap.get(g["content"], 0.0) for g in fused)
        assert index.search_lexical("nobody", queries[0], 5) == []
        # a bad mode, stale postings and a service without the lexical head: logged, answered with []
        with caplog.at_level(logging.ERROR):
            assert index.search_lexical("a", queries[0], 5, mode="weighted") == []
            index.add_rows([dict(content="w1 w2", agent_id="a")], np.asarray(svc.generate_embeddings_batch(["w1 w2"]), dtype=np.float32))
            assert index.search_lexical("a", queries[0], 5, mode="sparse") == [] and index.search_lexical("a", queries[0], 5) == []
            assert len(index.search("a", queries[0], 5)) == 5
            old = LocalEmbeddingService.from_dir(str(plain), engine=e, max_length=64)
            assert not old.has_lexical_head
            index.embeddings = old
            assert index.search_lexical("a", queries[0], 5) == []
        assert sum("Lexical search failed" in r.getMessage() for r in caplog.records) == 4
    finally:
        e.close()
