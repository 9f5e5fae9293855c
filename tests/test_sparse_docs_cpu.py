"""CPU: the doc-major side of the learned-sparse index - the numpy mirror of the device transposition (tests/sparse_docs_tools.py)
against LexicalPostings.from_weights, LexicalPostings.doc_major against from_weights' rules, and the ResidentLexical stand-in
against the mirror's counts."""
import numpy as np
import pytest

import sparse_docs_tools as D
import sparse_tools as S
from optimized_rag_amd.sparse import LexicalPostings, ResidentLexical


def same_postings(got, want):
    for g, x in zip(got, want):
        assert g.dtype == x.dtype and g.shape == x.shape
        np.testing.assert_array_equal(g.view(np.int32) if g.dtype == np.float32 else g, x.view(np.int32) if x.dtype == np.float32 else x)


@pytest.mark.parametrize("n_terms,want", [(1, 0), (64, 1), (65, 2), (4096, 2), (4097, 3), (250_002, 3)])
def test_pass_counts(n_terms, want):
    assert D.passes(n_terms) == want


@pytest.mark.parametrize("seed,n_docs,n_terms", [(1, 1, 40), (2, 300, 64), (3, 700, 65), (4, 2100, 5000), (5, 500, 4097)])
def test_mirror_equals_from_weights_on_seeded_blocks(seed, n_docs, n_terms):
    ptr, terms, w = D.doc_major_of_csr(*S.make_corpus(n_docs, n_terms + S.N_EMPTY, seed=seed)[:3], n_docs)
    terms = (terms % n_terms).astype(np.int32)                       # fold into the vocabulary, then make each document's terms distinct
    docs = []
    for a, e in zip(ptr[:-1], ptr[1:]):
        docs.append(np.unique(terms[a:e]))
    ptr2 = np.zeros(n_docs + 1, dtype=np.int32)
    ptr2[1:] = np.cumsum([len(d) for d in docs])
    terms2 = np.concatenate(docs).astype(np.int32)
    w2 = np.ascontiguousarray(w[:terms2.shape[0]])
    p = LexicalPostings.from_weights(D.maps_of(ptr2, terms2, w2), n_terms)
    same_postings(D.transpose(ptr2, terms2, w2, n_terms), (p.indptr, p.doc, p.weight))
    if n_docs >= 700:
        assert terms2.shape[0] > D.TILE and terms2.shape[0] % D.TILE != 0      # more than one tile, the last one partial


@pytest.mark.parametrize("name", list(D.edge_blocks()))
def test_mirror_equals_from_weights_on_the_edge_blocks(name):
    ptr, terms, w, n_terms = D.edge_blocks()[name]
    p = LexicalPostings.from_weights(D.maps_of(ptr, terms, w), n_terms)
    got = D.transpose(ptr, terms, w, n_terms)
    same_postings(got, (p.indptr, p.doc, p.weight))
    if name == "one term in every document":
        assert got[0][78] - got[0][77] == D.N_LONG > D.TILE
    if name == "a vocabulary of 250,002":
        assert D.passes(n_terms) == 3 and got[0][-1] - got[0][-2] == 3       # the last term: documents 0, 50 and 100


def test_a_stable_pass_alone_keeps_documents_ascending():
    """an atomic cursor would not: the pass must rank a posting behind the EARLIER ones of its digit, across tiles"""
    key = np.tile(np.array([5, 5, 9, 5], dtype=np.int64), 3000)
    dest = D.counting_pass(key, 0)
    assert sorted(dest.tolist()) == list(range(key.shape[0]))
    five = dest[key == 5]
    assert (np.diff(five) > 0).all() and five[0] == 0 and dest[key == 9][0] == five.shape[0]


# ---- LexicalPostings.doc_major ----------------------------------------------------------------------------------------------
def test_doc_major_holds_from_weights_postings():
    rng = np.random.default_rng(8)
    maps = []
    for d in range(400):
        ts = rng.choice(900, int(rng.integers(0, 20)), replace=False)
        maps.append({int(t): float(x) for t, x in zip(ts, rng.random(ts.shape[0]) * 2 - 0.2)})       # some weights <= 0: dropped
    maps[7] = {}
    maps[9] = {3: 0.0, 5: -1.0}
    ptr, terms, w = LexicalPostings.doc_major(maps, 1000)
    assert ptr.dtype == np.int32 and terms.dtype == np.int32 and w.dtype == np.float32 and ptr[0] == 0 and ptr[-1] == terms.shape[0]
    assert ptr[8] == ptr[7] and ptr[10] == ptr[9] and (w > 0).all()
    for a, e in zip(ptr[:-1], ptr[1:]):
        assert (np.diff(terms[a:e]) > 0).all()
    p = LexicalPostings.from_weights(maps, 1000)
    same_postings(D.transpose(ptr, terms, w, 1000), (p.indptr, p.doc, p.weight))
    ptr_d, terms_d, _ = LexicalPostings.doc_major(maps)              # n_terms defaults as in from_weights
    assert LexicalPostings.from_weights(maps).n_terms == int(terms_d.max()) + 1 and np.array_equal(ptr_d, ptr)


@pytest.mark.parametrize("maps,n_terms", [([{1: float("nan")}], 10), ([{1: float("inf")}], 10), ([{1: 1e39}], 10), ([{10: 1.0}], 10),
                                          ([{-1: 1.0}], 10), ([], 10), ([{1: 1.0}], 0)])
def test_doc_major_raises_where_from_weights_raises(maps, n_terms):
    with pytest.raises(ValueError):
        LexicalPostings.from_weights(maps, n_terms)
    with pytest.raises(ValueError):
        LexicalPostings.doc_major(maps, n_terms)


def test_doc_major_of_only_dropped_entries_is_an_empty_block():
    ptr, terms, w = LexicalPostings.doc_major([{4: 0.0}, {}], 10)
    assert ptr.tolist() == [0, 0, 0] and terms.shape == (0,) and w.shape == (0,)
    assert LexicalPostings.from_weights([{4: 0.0}, {}], 10).nnz == 0


# ---- ResidentLexical --------------------------------------------------------------------------------------------------------
def test_resident_lexical_counts_follow_the_mirror():
    ip, doc, w = S.make_corpus(500, 2000, seed=4)
    mirror, stand_in = LexicalPostings(ip, doc, w, 500), ResidentLexical(500, 2000)
    rng = np.random.default_rng(2)
    live = rng.random(500) > 0.1
    row_map = np.where(live, np.cumsum(live) - 1, -1)
    mirror.compacted(row_map)
    stand_in.compacted(row_map)
    assert (stand_in.n_docs, stand_in.n_terms) == (mirror.n_docs, mirror.n_terms) == (int(live.sum()), 2000)
    mirror.extend([{3: 1.0}, {2500: 2.0}], 2600)
    stand_in.appended(2, 2600)
    assert (stand_in.n_docs, stand_in.n_terms) == (mirror.n_docs, mirror.n_terms)
    for bad in (np.zeros(3, np.int64), np.arange(stand_in.n_docs)[::-1].copy()):
        with pytest.raises(ValueError):
            LexicalPostings(*S.make_corpus(stand_in.n_docs, 50, seed=1), stand_in.n_docs).compacted(bad)
        with pytest.raises(ValueError):
            stand_in.compacted(bad)
    with pytest.raises(ValueError):
        stand_in.appended(1, 100)
