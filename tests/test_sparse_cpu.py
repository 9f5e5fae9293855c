"""CPU: the host side of the learned-sparse index (optimized-rag_amd/sparse.py LexicalPostings) and the float64 reference of
tests/sparse_tools.py that the GPU tests compare against bit for bit - including that the reference's bits really depend on the
token order, and that the seeded corpus holds every table form the kernel has a path for."""
import numpy as np
import pytest

import sparse_tools as S
from optimized_rag_amd.sparse import LexicalPostings

MAPS = [{5: 0.5, 2: 1.5, 9: 0.25}, {2: 2.0, 7: 0.125, 3: 0.0}, {9: 4.0, 5: 1.0}]


def test_from_weights_builds_term_major_csr():
    p = LexicalPostings.from_weights(MAPS)
    assert (p.n_docs, p.n_terms, p.nnz) == (3, 10, 7)                   # the zero weight is left out
    np.testing.assert_array_equal(p.indptr, [0, 0, 0, 2, 2, 2, 4, 4, 5, 5, 7])
    np.testing.assert_array_equal(p.doc, [0, 1, 0, 2, 1, 0, 2])
    np.testing.assert_array_equal(p.weight, np.array([1.5, 2.0, 0.5, 1.0, 0.125, 0.25, 4.0], dtype=np.float32))
    assert p.indptr.dtype == np.int64 and p.doc.dtype == np.int32 and p.weight.dtype == np.float32
    for t in range(p.n_terms):
        assert (np.diff(p.doc[p.indptr[t]:p.indptr[t + 1]]) > 0).all()
    wide = LexicalPostings.from_weights(MAPS, n_terms=64)
    assert wide.n_terms == 64 and wide.nnz == 7 and int(wide.indptr[-1]) == 7
    with pytest.raises(ValueError):
        LexicalPostings.from_weights(MAPS, n_terms=9)                   # token 9 does not fit
    with pytest.raises(ValueError):
        LexicalPostings.from_weights([{1: float("inf")}])
    with pytest.raises(ValueError):
        LexicalPostings.from_weights([{1: float("nan")}])
    with pytest.raises(ValueError):
        LexicalPostings.from_weights([])


def test_encode_queries_sorts_each_query_by_token_id():
    ptr, terms, w = LexicalPostings.encode_queries([{9: 1.0, 2: 0.5, 5: 2.0}, {}, {7: 0.25, -1: 1.0, 3: 0.0}])
    np.testing.assert_array_equal(ptr, [0, 3, 3, 6])
    np.testing.assert_array_equal(terms, [2, 5, 9, -1, 3, 7])
    np.testing.assert_array_equal(w, np.array([0.5, 2.0, 1.0, 1.0, 0.0, 0.25], dtype=np.float32))
    assert ptr.dtype == np.int32 and terms.dtype == np.int32 and w.dtype == np.float32


def test_reference_on_a_corpus_worked_out_by_hand():
    p = LexicalPostings.from_weights(MAPS)
    ptr, terms, w = LexicalPostings.encode_queries([{2: 2.0, 9: 0.5, 4: 1.0, 11: 1.0}])
    s = S.scores(p.indptr, p.doc, p.weight, 3, terms, w)
    # doc 0: 2.0 * 1.5 + 0.5 * 0.25; doc 1: 2.0 * 2.0; doc 2: 0.5 * 4.0 (terms 4 and 11 match nothing / lie outside)
    np.testing.assert_array_equal(s, [3.125, 4.0, 2.0])
    rows, sc = S.topk(s, 5)
    np.testing.assert_array_equal(rows, [1, 0, 2, -1, -1])
    np.testing.assert_array_equal(sc, [4.0, 3.125, 2.0, 0.0, 0.0])
    rows, sc = S.topk(s, 2, hidden=np.array([False, True, False]))
    np.testing.assert_array_equal(rows, [0, 2])
    # ties go to the lower row; a zero score is never returned
    rows, _ = S.topk(np.array([1.0, 0.0, 2.0, 1.0, 2.0]), 5)
    np.testing.assert_array_equal(rows, [2, 4, 0, 3, -1])
    # a weight that is not > 0 adds nothing, a repeated term adds twice
    np.testing.assert_array_equal(S.scores(p.indptr, p.doc, p.weight, 3, [2, 2, 5, 9], np.array([1.0, 1.0, np.nan, -1.0], np.float32)),
                                  [3.0, 4.0, 0.0])


def test_shard_scores_equal_the_slice_of_the_full_scores():
    indptr, doc, w = S.make_corpus(n_docs=5000, n_terms=3000, seed=3)
    full = LexicalPostings(indptr, doc, w, 5000)
    qs = S.make_queries(indptr, seed=5)
    A = S.all_scores(indptr, doc, w, 5000, qs)
    for a, b in ((0, 2048), (2048, 5000), (1234, 1235)):
        sh = full.shard(a, b)
        assert sh.n_docs == b - a and sh.n_terms == full.n_terms
        assert all((np.diff(sh.doc[sh.indptr[t]:sh.indptr[t + 1]]) > 0).all() for t in range(0, sh.n_terms, 37))
        np.testing.assert_array_equal(S.bits(S.all_scores(sh.indptr, sh.doc, sh.weight, b - a, qs)), S.bits(A[:, a:b]))


def test_seeded_corpus_has_every_table_form_and_an_order_sensitive_reference():
    indptr, doc, w = S.make_corpus()
    df = np.diff(indptr)
    print("postings", doc.shape[0], "| df >= N/4:", int((df >= S.N_FULL / 4).sum()), "| df < 8:", int((df < 8).sum()),
          "| empty:", int((df == 0).sum()))
    assert 1_000_000 < doc.shape[0] < 1_050_000 and w.min() > 0 and np.isfinite(w).all()
    assert (df >= S.N_FULL / 4).sum() >= 3              # direct per-range bracket rows
    assert ((df >= 32) & (df < 2000)).sum() >= 100       # coarser tables
    assert (df < 8).sum() >= 10_000                      # no table at all
    assert (df == 0).sum() >= S.N_EMPTY                  # empty lists
    qs = S.make_queries(indptr)
    assert len(qs[0][0]) == 70 and len(set(qs[0][0].tolist())) == 70
    A = S.all_scores(indptr, doc, w, S.N_FULL, qs)
    matches = (A > 0).sum(axis=1)
    assert (matches > 20_000).sum() >= 5 and 0 < matches[24] < 100 and not matches[25:28].any()
    # reversing the token order changes the bits of some scores: the bit-exact GPU tests pin an ORDER, not just a sum
    B = S.all_scores(indptr, doc, w, S.N_FULL, [(t[::-1], qw[::-1]) for t, qw in qs])
    changed = int((S.bits(A) != S.bits(B)).sum())
    print("scores whose bits change with the token order:", changed)
    assert changed > 100 and np.abs(A - B).max() < 1e-12


def test_tie_corpus_has_a_plateau_across_k():
    indptr, doc, w = S.make_corpus(weight_values=[0.25, 0.5, 1.0])
    by_df = np.argsort(-np.diff(indptr), kind="stable")
    s = S.scores(indptr, doc, w, S.N_FULL, by_df[[6, 7, 8]], np.array([1.0, 0.5, 0.25], dtype=np.float32))
    rows, sc = S.topk(s, 100)
    above, tied = int((s > sc[99]).sum()), int((s == sc[99]).sum())
    print("k-th score", sc[99], "| above:", above, "| tied:", tied)
    assert above < 100 < above + tied and tied > 200
    cut_rows = np.nonzero(s == sc[99])[0][:100 - above]
    np.testing.assert_array_equal(np.sort(rows[above:]), cut_rows)          # the plateau is cut by the lowest rows
