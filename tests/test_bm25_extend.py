"""CPU: Bm25Postings.extend - the host mirror of appendable postings (rag_bm25_append_host).

After `p = from_corpus(A); p.extend(B)` the CSR mirror is exactly `from_corpus(A + B)`, the statistics are the FROZEN ones of
`from_corpus(A)`, and `refreshed()` gives the statistics a rebuild would. Scores over the mirror are pinned by
oracle.rag_oracle.bm25_scores_csr, which takes explicit idf / avgdl."""
import numpy as np
import pytest

from oracle import rag_oracle as O
from tools_textgen import make_doc


def _corpus(rng, n, extra_words=()):
    docs = []
    for i in range(n):
        d = make_doc(rng, int(rng.integers(1, 4)))
        if extra_words and rng.random() < 0.5:
            d += " " + " ".join(extra_words[int(j)] for j in rng.integers(0, len(extra_words), 3))
        docs.append(d)
    return docs


def _splits():
    rng = np.random.default_rng(41)
    A = _corpus(rng, 300)
    new_words = [f"novel{i}" for i in range(12)]
    return {
        "one_doc": (A, _corpus(rng, 1)),
        "many_docs": (A, _corpus(rng, 450) + ["", "   "]),                       # with empty documents
        "new_terms": (A, _corpus(rng, 120, new_words) + ["novel3 novel3 Zurich"]),
    }


SPLITS = _splits()


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("name", sorted(SPLITS))
def test_extend_mirror_equals_from_corpus_and_statistics_stay_frozen(name):
    from optimized_rag_amd.bm25 import Bm25Postings
    A, Bc = SPLITS[name]
    pa = Bm25Postings.from_corpus(A)
    V_A = len(pa.vocab)
    p = Bm25Postings.from_corpus(A)
    block = p.extend(Bc)
    full = Bm25Postings.from_corpus(A + Bc)
    for f in ("indptr", "doc", "tf", "doc_len"):
        np.testing.assert_array_equal(getattr(p, f), getattr(full, f), err_msg=f)
        assert getattr(p, f).dtype == getattr(full, f).dtype, f
    assert list(p.vocab.items()) == list(full.vocab.items())
    # frozen statistics
    np.testing.assert_array_equal(_bits(p.idf[:V_A]), _bits(pa.idf))
    assert _bits(p.avgdl) == _bits(pa.avgdl)
    assert p.idf.shape[0] == len(full.vocab)
    # the block: the CSR of the new documents alone over the grown vocabulary, block-relative document numbers
    alone = Bm25Postings.from_corpus(Bc)
    assert block["n_terms_total"] == len(full.vocab) and block["indptr"].shape[0] == len(full.vocab) + 1
    np.testing.assert_array_equal(block["doc_len"], alone.doc_len)
    assert int(block["indptr"][-1]) == int(alone.indptr[-1])
    for w, t_alone in alone.vocab.items():
        t = full.vocab[w]
        a, e = block["indptr"][t], block["indptr"][t + 1]
        np.testing.assert_array_equal(block["doc"][a:e], alone.doc[alone.indptr[t_alone]:alone.indptr[t_alone + 1]])
        np.testing.assert_array_equal(block["tf"][a:e], alone.tf[alone.indptr[t_alone]:alone.indptr[t_alone + 1]])
    np.testing.assert_array_equal(_bits(block["idf_new"]), _bits(p.idf[V_A:]))
    if name == "new_terms":
        assert len(full.vocab) > V_A


@pytest.mark.parametrize("name", sorted(SPLITS))
def test_refreshed_statistics_equal_a_rebuild(name):
    from optimized_rag_amd.bm25 import Bm25Postings
    A, Bc = SPLITS[name]
    p = Bm25Postings.from_corpus(A)
    p.extend(Bc)
    full = Bm25Postings.from_corpus(A + Bc)
    r = p.refreshed()
    np.testing.assert_array_equal(_bits(r.idf), _bits(full.idf))
    assert _bits(r.avgdl) == _bits(full.avgdl)
    np.testing.assert_array_equal(r.indptr, full.indptr)
    d = p.drift()
    assert d["avgdl_frozen"] == p.avgdl and d["avgdl_true"] == full.avgdl
    assert d["idf_max_abs_change"] == float(np.abs(full.idf - p.idf).max())
    assert r.drift()["idf_max_abs_change"] == 0.0


@pytest.mark.parametrize("name", sorted(SPLITS))
def test_two_extends_equal_one(name):
    from optimized_rag_amd.bm25 import Bm25Postings
    A, Bc = SPLITS[name]
    rng = np.random.default_rng(3)
    C2 = _corpus(rng, 40, ["later0", "later1"])
    one = Bm25Postings.from_corpus(A)
    one.extend(Bc + C2)
    two = Bm25Postings.from_corpus(A)
    two.extend(Bc)
    two.extend(C2)
    for f in ("indptr", "doc", "tf", "doc_len"):
        np.testing.assert_array_equal(getattr(one, f), getattr(two, f), err_msg=f)
    assert list(one.vocab.items()) == list(two.vocab.items())
    V_A = len(Bm25Postings.from_corpus(A).vocab)
    np.testing.assert_array_equal(_bits(one.idf[:V_A]), _bits(two.idf[:V_A]))
    assert _bits(one.avgdl) == _bits(two.avgdl)


@pytest.mark.parametrize("name", sorted(SPLITS))
def test_scores_over_the_mirror_equal_the_per_segment_scores(name):
    """Each document lives in one segment and its score is summed in query-token order from the same impacts: scoring the
    merged CSR equals scoring the old postings and the block separately (frozen idf / avgdl on both sides)."""
    from optimized_rag_amd.bm25 import Bm25Postings
    A, Bc = SPLITS[name]
    p = Bm25Postings.from_corpus(A)
    base = Bm25Postings.from_corpus(A)
    block = p.extend(Bc)
    queries = ["memory vector index", "novel3 zurich system system", "paris unknownword london", "novel1"]
    ptr, terms = p.encode_queries(queries)
    seen = 0.0
    for qi in range(len(queries)):
        qt = terms[ptr[qi]:ptr[qi + 1]]
        merged = O.bm25_scores_csr(p.indptr, p.doc, p.tf, p.doc_len, p.idf, p.avgdl, qt)
        s_base = O.bm25_scores_csr(base.indptr, base.doc, base.tf, base.doc_len, p.idf[:len(base.vocab)], p.avgdl, qt)
        s_tail = O.bm25_scores_csr(block["indptr"], block["doc"], block["tf"], block["doc_len"], p.idf, p.avgdl, qt)
        np.testing.assert_array_equal(_bits(merged), _bits(np.concatenate([s_base, s_tail])))
        seen = max(seen, float(np.abs(merged).max()))
    assert seen > 0


def test_new_term_idf_rule():
    import math
    from optimized_rag_amd.bm25 import Bm25Postings, EPSILON
    A = ["a b c", "a b", "a c d", "b d"]
    p = Bm25Postings.from_corpus(A)
    mean_loaded = float(np.cumsum(p.idf)[-1]) / p.idf.shape[0]
    block = p.extend(["x a", "x y", "x", "x b", "x z"])          # x: df 5 of N 9 -> negative; y, z: df 1
    V = p.vocab
    assert block["idf_new"][V["x"] - 4] == EPSILON * mean_loaded
    assert block["idf_new"][V["y"] - 4] == math.log(9 - 1 + 0.5) - math.log(1 + 0.5)
    frozen = p.idf.copy()
    p.extend(["y y", "q"])
    np.testing.assert_array_equal(_bits(p.idf[:len(frozen)]), _bits(frozen))       # frozen from then on
