"""Pin the CPU oracle (oracle/rag_oracle.py) against golden vectors produced by running the reference's
own Python (tools/make_golden.py). CPU-only; no GPU, no /root/reference access at run time."""
import json
import os
from datetime import datetime

import numpy as np
import pytest

from oracle import rag_oracle as O

TOL = 1e-12      # float64, different summation order only


def load(golden_dir, name):
    with open(os.path.join(golden_dir, name)) as f:
        return json.load(f)


def test_cosine_all_copies(golden_dir):
    g = np.load(os.path.join(golden_dir, "cosine.npz"))
    a, b = g["a"], g["b"]
    mine = np.array([O.cosine(a[i], b[i]) for i in range(len(a))])
    for k in ("retrieval", "openai", "mmr", "consistency", "compressor", "helpers"):
        np.testing.assert_allclose(mine, g["exp_" + k], rtol=0, atol=TOL, err_msg=k)
    assert mine[5] == 0.0 and mine[6] == 0.0                    # zero-norm -> exactly 0.0
    assert abs(mine[3] - 1.0) < 1e-12 and abs(mine[4] + 1.0) < 1e-12
    M = O.cosine_matrix(a, b)
    np.testing.assert_allclose(np.diag(M), g["exp_retrieval"], atol=TOL)
    assert O.cosine([], [1.0, 2.0], empty_is_zero=True) == g["mmr_empty"][0] == 0.0
    assert O.cosine([1.0], [], empty_is_zero=True) == g["mmr_empty"][1] == 0.0
    assert abs(O.cosine([1.0, 2.0, 3.0], [1.0, 2.0]) - float(g["trunc"])) < TOL


def test_hybrid_search(golden_dir):
    g = load(golden_dir, "hybrid_search.json")
    assert {k: tuple(v[x] for x in ("alpha", "beta", "gamma")) for k, v in g["intent_weights"].items()} == O.INTENT_WEIGHTS
    for c in g["cases"]:
        idx, rows = O.hybrid_search(
            c["query"], c["corpus"], np.array(c["embeddings"], dtype=np.float32),
            np.array(c["query_embedding"], dtype=np.float32), top_k=c["top_k"], metadata=c["metadata"],
            intent=c["intent"], default_weights=tuple(c["alpha_beta_gamma_default"]),
            use_adaptive_weights=c["use_adaptive_weights"], bm25_available=False,
            now=datetime.fromisoformat(c["now"]))
        assert idx == c["expected_idx"]
        for r, e in zip(rows, c["expected"]):
            for k in e:
                assert abs(r[k] - e[k]) < TOL, k
    for kcase in g["keyword"]:
        assert O.simple_keyword_scores(kcase["query"], kcase["corpus"]) == kcase["expected"]


def test_rrf(golden_dir):
    g = load(golden_dir, "rrf.json")
    for c in g["cases"]:
        keys, scores, ranks = O.rrf_fuse(c["lists"], k=c["k"], top_k=c["top_k"])
        assert keys == c["expected_ids"]
        assert scores == c["expected_scores"]                   # same fp64 ops in the same order: bit-exact
        for key, rk in zip(keys, ranks):
            for li, lst in enumerate(c["lists"]):
                assert rk[li] == (lst.index(key) + 1 if key in lst else 0)
    d = g["dup"]
    lists = [[x if x is not None else "" for x in l] for l in d["lists"]]
    keys, scores, _ = O.rrf_fuse(lists, k=60, top_k=10)
    assert keys == d["expected_contents"] and scores == d["expected_scores"]


def test_mmr(golden_dir):
    g = load(golden_dir, "mmr.json")
    for c in g["class"]:
        pos, sc = O.mmr_class(c["q"], c["emb"], c["top_k"], c["lambda"])
        assert pos == c["expected_pos"]
        np.testing.assert_allclose(sc, c["expected_mmr"], atol=TOL)
    for c in g["helper"]:
        assert O.mmr_helper(c["q"], c["emb"], c["k"], c["lambda"]) == c["expected_pos"]


def test_consistency(golden_dir):
    g = load(golden_dir, "consistency.json")
    for c in g["cases"]:
        table = c["embeddings"]
        for d, exp in zip(c["docs"], c["expected_claims"]):
            assert O.extract_claims(d["content"]) == exp
        out = O.check_consistency(c["docs"], lambda texts: [table[t] for t in texts], threshold=c["threshold"])
        exp = c["expected"]
        assert out["consistent"] == exp["consistent"]
        assert out["contradiction_count"] == exp["contradiction_count"]
        assert out["total_claims"] == exp["total_claims"]
        assert abs(out["confidence"] - exp["confidence"]) < TOL
        assert out["warning"] == exp["warning"]
        assert out["contradictions"] == exp["contradictions"]
    e = g["edge"]
    assert O.check_consistency([{"content": "x"}], None) == e["one_doc"]
    assert O.check_consistency([{"content": "Tiny."}, {"content": "Also tiny."}], None) == e["few_claims"]

    def boom(t):
        raise RuntimeError("down")

    out = O.check_consistency(e["embed_fail_docs"], boom)
    assert out == e["embed_fail"]
    for p in e["is_contradiction"]:
        assert O.is_contradiction(p["a"], p["b"]) == p["expected"]


def test_compressor_pieces(golden_dir):
    g = load(golden_dir, "compressor.json")
    sh = g["score_hybrid"]
    table = sh["embeddings"]
    mine = O.score_sentences_hybrid(sh["query"], sh["sentences"], table[sh["query"]], [table[s] for s in sh["sentences"]])
    np.testing.assert_allclose(mine, sh["expected"], atol=TOL)
    for c in g["lexical"]:
        assert abs(O.score_sentence_lexical(c["q"], c["s"]) - c["expected"]) < TOL
    for c in g["split"]:
        assert O.split_sentences(c["text"]) == c["expected"]


def test_reranker_postprocessing(golden_dir):
    g = load(golden_dir, "rerankers.json")
    oai = g["openai"]
    emb = np.array(oai["emb"], dtype=np.float32)
    origs = [(r.get("similarity", 0) or r.get("score", 0)) for r in oai["results"]]
    sc = O.openai_rerank_scores(emb[0], emb[1:], origs)
    order = O.stable_topk_desc(sc, oai["top_k"])
    assert [int(i) for i in order] == oai["expected_pos"]
    np.testing.assert_allclose([sc[i] for i in order], oai["expected_rerank"], atol=TOL)
    cr = g["cross"]
    sig = [O.sigmoid(float(np.float32(x))) for x in cr["logits"][:-1]]      # last one (-30) is still finite
    sig.append(O.sigmoid(float(np.float32(cr["logits"][-1]))))
    order = O.stable_topk_desc(sig, cr["top_k"])
    assert [int(i) for i in order] == [e["pos"] for e in cr["expected"]]
    for i, e in zip(order, cr["expected"]):
        assert abs(sig[i] - e["cross_encoder_score"]) < 1e-15


def test_chunk_chain_reproduces_the_reference_chunks(golden_dir):
    """O.chunk_chain, fed the sentences and embeddings the reference's SemanticChunker saw, groups them into the chunks the
    reference recorded (tests/golden/cosine_sites.json["chunker"]): contents, chunk ids, sentence counts and sizes."""
    import re
    g = load(golden_dir, "cosine_sites.json")
    table = g["embeddings_noise09"]
    n_chain = 0
    for c in g["chunker"]:
        text, md = c["text"], c["metadata"]
        sentences = [s.strip() for s in re.split(r'(?<=[.!?])\s+', text) if s.strip()]
        if not sentences:
            got = []
        elif len(text) < c["min_chunk_size"]:                     # the whole text is one chunk before any embedding is made
            got = [{"content": text, "metadata": {**(md or {}), "chunk_id": 0}}]
        else:
            groups = O.chunk_chain([table[s] for s in sentences], [len(s) for s in sentences], c["threshold"],
                                   c["max_chunk_size"], c["min_chunk_size"])
            assert groups[0] == 0 and all(b - a in (0, 1) for a, b in zip(groups, groups[1:]))
            got = []
            for cid in range(groups[-1] + 1):
                content = " ".join(s for s, gi in zip(sentences, groups) if gi == cid)
                got.append({"content": content, "metadata": {"chunk_id": cid, "num_sentences": groups.count(cid),
                                                             "chunk_size": len(content), **(md or {})}})
            n_chain += len(got) > 2
        assert got == c["expected"]
    assert n_chain >= 4                                           # joins and splits both happen in the fixture


def test_mmr_greedy_is_the_two_loops():
    """O.mmr_greedy (running max over precomputed cosines, used for pools of 256 where the O(k^2 n) loops take minutes) returns
    bit-identical picks and scores to O.mmr_class / O.mmr_helper, on Gaussian inputs, on integer inputs full of exact ties, with
    duplicates and a zero row, up to top_k = n."""
    for seed, n, dim, integer in [(0, 1, 8, False), (1, 7, 3, True), (2, 24, 16, False), (3, 33, 5, True), (4, 64, 2, True),
                                  (5, 40, 64, False)]:
        rng = np.random.default_rng(seed)
        embs = rng.integers(-3, 4, (n, dim)).astype(np.float64) if integer else rng.standard_normal((n, dim)).astype(np.float32).astype(np.float64)
        if n > 4:
            embs[3] = embs[1]
            embs[2] = 0.0
        q = embs[0] + 1.0 if integer else rng.standard_normal(dim)
        rel0 = [O.cosine(q, e, empty_is_zero=True) for e in embs]
        sim = [[O.cosine(a, b) for b in embs] for a in embs]
        for lam in (0.0, 0.5, 0.7, 1.0):
            for k in sorted({1, max(1, n // 2), n}):
                assert O.mmr_greedy(rel0, sim, k, lam, 0) == O.mmr_class(q, embs, k, lam)
                if n > k:
                    assert O.mmr_greedy(rel0, sim, k, lam, 1) == O.mmr_helper(q, embs, k, lam, with_scores=True)
                    assert O.mmr_helper(q, embs, k, lam) == O.mmr_greedy(rel0, sim, k, lam, 1)[0]


def test_exact_chain_recipe_is_independent_of_the_summation_order():
    """The input recipe of tests/small_inputs.py for the chunk chain: at every dimension the GPU test uses, the oracle's
    similarities are IDENTICAL under the sequential and a randomly permuted summation order (every sum is exact), each chain
    makes at least three chunks, and a threshold taken from the chain is met exactly on the chain again, where `>=` against `>`
    decides the grouping."""
    import small_inputs as SI
    for dim in SI.CHAIN_DIMS:
        for seed in range(3 if dim > 2000 else 6):
            embs, lens = SI.exact_chain(seed, dim)
            perm = np.random.default_rng(seed).permutation(dim)
            g0, s0 = O.chunk_chain(embs, lens, 0.5, SI.CHAIN_MAX, SI.CHAIN_MIN, with_sims=True)
            g1, s1 = O.chunk_chain(embs, lens, 0.5, SI.CHAIN_MAX, SI.CHAIN_MIN, order=perm, with_sims=True)
            assert s0 == s1 and g0 == g1, (dim, seed)
            assert g0[-1] >= 2, (dim, seed)
            assert max(g0.count(c) for c in set(g0)) <= 9
            t = SI.deciding_threshold(g0, s0, lens, SI.CHAIN_MAX, SI.CHAIN_MIN)
            assert t is not None and t >= 0.5, (dim, seed)
            gt, st_ = O.chunk_chain(embs, lens, t, SI.CHAIN_MAX, SI.CHAIN_MIN, with_sims=True)
            assert gt == g0 and st_ == s0 and t in st_
            assert O.chunk_chain(embs, lens, SI.next_up(t), SI.CHAIN_MAX, SI.CHAIN_MIN) != gt, (dim, seed)


def test_rerank_topk_is_sigmoid_then_the_stable_sort(golden_dir):
    cr = load(golden_dir, "rerankers.json")["cross"]
    lg = [float(np.float32(x)) for x in cr["logits"]]
    ids, sc, out_lg = O.rerank_topk(lg, list(range(100, 100 + len(lg))), cr["top_k"])
    assert ids == [100 + e["pos"] for e in cr["expected"]]
    assert all(abs(s - e["cross_encoder_score"]) < 1e-15 for s, e in zip(sc, cr["expected"]))
    # empty slots are skipped wherever they sit, exact ties keep candidate order, short lists are padded
    assert O.rerank_topk([40.0, 3.0, 50.0, 3.0, -1.0], [7, -1, 8, 9, 10], 4) == ([7, 8, 9, 10], [1.0, 1.0, O.sigmoid(3.0), O.sigmoid(-1.0)], [40.0, 50.0, 3.0, -1.0])
    assert O.rerank_topk([1.0, 2.0], [-1, 5], 2) == ([5, -1], [O.sigmoid(2.0), 0.0], [2.0, 0.0])
