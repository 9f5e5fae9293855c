"""CPU: Bm25Postings.refresh - the host mirror of rag_bm25_refresh (statistics recomputed over the live documents, in place).

The reference for every case is `from_corpus` over the texts that are live: rank-bm25's rule. Term numbers never change in the
mirror, so the tables are compared by word. Where the deletes leave the first-appearance order of the terms alone the two
tables are the same array; otherwise only the summation order of the mean differs, which shows in the floored values alone."""
import math

import numpy as np
import pytest

from optimized_rag_amd.bm25 import EPSILON, Bm25Postings


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def _texts(rng, n, vocab=300, extra=()):
    """Zipf-distributed tokens: the most frequent ones sit in more than half of the documents (negative raw idf)."""
    out = []
    for L in rng.poisson(14, n):
        w = [f"t{int(x) % vocab}" for x in rng.zipf(1.1, int(L)) - 1]
        if extra and rng.random() < 0.5:
            w += [extra[int(j)] for j in rng.integers(0, len(extra), 2)]
        out.append(" ".join(w))
    return out


def _by_word(p, words):
    return np.array([p.idf[p.vocab[w]] for w in words], dtype=np.float64)


def _raw_idf(df, n):
    return math.log(n - df + 0.5) - math.log(df + 0.5)


def test_refresh_after_extend_is_a_rebuild():
    rng = np.random.default_rng(7)
    A, B = _texts(rng, 400), _texts(rng, 700, extra=[f"n{i}" for i in range(9)]) + ["", "t1 t1 n3"]
    p = Bm25Postings.from_corpus(A)
    p.extend(B)
    frozen = p.idf.copy()
    assert p.refresh() is p
    ref = Bm25Postings.from_corpus(A + B)
    assert p.vocab == ref.vocab
    np.testing.assert_array_equal(_bits(p.idf), _bits(ref.idf))
    assert p.avgdl == ref.avgdl
    assert (ref.idf != frozen).any()                                 # the frozen table was another one
    assert (np.diff(p.indptr) * 2 > p.n_docs).any()                  # ... and the epsilon floor was exercised
    np.testing.assert_array_equal(_bits(p.idf), _bits(p.refreshed().idf))      # refreshed() agrees and is left as it was


def test_live_mask_that_keeps_the_term_order():
    rng = np.random.default_rng(11)
    texts = _texts(rng, 600)
    p = Bm25Postings.from_corpus(texts)
    # a document may go unless it is the first one a term appears in
    first_doc = {p.doc[p.indptr[t]] for t in range(len(p.vocab))}
    live = np.ones(len(texts), dtype=bool)
    cand = np.array([d for d in range(len(texts)) if d not in first_doc])
    live[rng.choice(cand, len(cand) // 2, replace=False)] = False
    assert (~live).sum() > 100
    ref = Bm25Postings.from_corpus([t for t, l in zip(texts, live) if l])
    assert list(ref.vocab) == list(p.vocab)
    p.refresh(live)
    np.testing.assert_array_equal(_bits(p.idf), _bits(ref.idf))
    assert p.avgdl == ref.avgdl
    assert p.n_docs == len(texts)                                    # the mirror itself keeps every document


def test_arbitrary_deletes_differ_in_the_mean_only():
    rng = np.random.default_rng(13)
    texts = _texts(rng, 800)
    p = Bm25Postings.from_corpus(texts)
    live = rng.random(len(texts)) > 0.4
    ref = Bm25Postings.from_corpus([t for t, l in zip(texts, live) if l])
    assert list(ref.vocab) != [w for w in p.vocab if w in ref.vocab]          # the order did change
    p.refresh(live)
    words = list(ref.vocab)
    got, exp = _by_word(p, words), ref.idf
    n = int(live.sum())
    df = np.diff(ref.indptr)
    floored = np.array([_raw_idf(int(d), n) < 0 for d in df])
    assert floored.any() and (~floored).any()
    np.testing.assert_array_equal(_bits(got[~floored]), _bits(exp[~floored]))
    np.testing.assert_allclose(got[floored], exp[floored], rtol=0, atol=1e-12)
    assert p.avgdl == ref.avgdl


def test_a_term_without_postings_keeps_its_number():
    texts = ["alpha beta", "beta gamma gamma", "beta delta", "gamma delta epsilon", "beta"]
    p = Bm25Postings.from_corpus(texts)
    t_alpha, t_eps = p.vocab["alpha"], p.vocab["epsilon"]
    live = np.array([False, True, True, False, True])                # alpha and epsilon lose every posting
    p.refresh(live)
    n = 3
    assert p.vocab["alpha"] == t_alpha and p.vocab["epsilon"] == t_eps and len(p.idf) == 5
    gone = math.log(n + 0.5) - math.log(0.5)
    assert p.idf[t_alpha] == gone and p.idf[t_eps] == gone
    # the mean runs over beta (df 3), gamma (df 1), delta (df 1) in term-number order - not over the two that are gone
    vals = [_raw_idf(3, n), _raw_idf(1, n), _raw_idf(1, n)]
    mean = ((vals[0] + vals[1]) + vals[2]) / 3
    assert p._frozen_mean == mean
    assert p.idf[p.vocab["beta"]] == EPSILON * mean                  # ln(0.5) - ln(3.5) < 0: floored
    assert p.idf[p.vocab["gamma"]] == vals[1]
    assert p.avgdl == (3 + 2 + 1) / 3
    ref = Bm25Postings.from_corpus([t for t, l in zip(texts, live) if l])
    np.testing.assert_array_equal(_bits(_by_word(p, list(ref.vocab))), _bits(ref.idf))
    with pytest.raises(ValueError):
        p.refresh(np.zeros(5, dtype=bool))
    with pytest.raises(ValueError):
        p.refresh(np.ones(4, dtype=bool))


def test_frozen_mean_follows_the_refresh():
    rng = np.random.default_rng(17)
    A = _texts(rng, 20, vocab=40)
    p = Bm25Postings.from_corpus(A)
    m0 = p._frozen_mean
    p.extend(_texts(rng, 60, vocab=40))
    p.refresh()
    m1 = p._frozen_mean
    assert m1 != m0
    raw = np.array([_raw_idf(int(d), p.n_docs) for d in np.diff(p.indptr)])
    assert m1 == float(np.cumsum(raw)[-1]) / len(raw)
    # a new term in more than half of all documents: its negative idf is floored by the NEW mean
    blk = p.extend(["common " + t for t in _texts(rng, 100, vocab=40)])
    t = p.vocab["common"]
    assert _raw_idf(100, 180) < 0
    assert p.idf[t] == p.epsilon * m1 and blk["idf_new"][0] == p.epsilon * m1


def test_negative_mean_on_a_tiny_corpus():
    texts = ["a b c", "c b a a", "b c a b c"]
    p = Bm25Postings.from_corpus(texts)
    p.idf = np.ones(3)                                               # whatever it was loaded with
    p.refresh()
    raw = math.log(0.5) - math.log(3.5)
    mean = ((raw + raw) + raw) / 3
    assert mean < 0 and p._frozen_mean == mean
    assert (p.idf == EPSILON * mean).all() and (p.idf < 0).all()
    np.testing.assert_array_equal(_bits(p.idf), _bits(Bm25Postings.from_corpus(texts).idf))
    assert p.avgdl == 12 / 3
