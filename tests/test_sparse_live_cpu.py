"""CPU: the host mirror of the learned-sparse postings through live writes - LexicalPostings.extend / compacted against
sparse_tools.cut and a direct rebuild from the surviving {token id: weight} maps, array for array."""
import numpy as np
import pytest

import sparse_tools as S
from optimized_rag_amd.sparse import LexicalPostings

N0, BLOCKS, V0, V = 3000, (1, 700, 2100), 3500, 4000
N_ALL = N0 + sum(BLOCKS)


def maps_of(indptr, doc, w, n_docs):
    maps = [dict() for _ in range(n_docs)]
    term_of = np.repeat(np.arange(indptr.shape[0] - 1), np.diff(indptr))
    for t, d, x in zip(term_of.tolist(), doc.tolist(), w.tolist()):
        maps[d][t] = x
    return maps


@pytest.fixture(scope="module")
def corpus():
    ip, doc, w = S.make_corpus(N_ALL, V, seed=7)
    maps = maps_of(ip, doc, w, N_ALL)
    maps[N0 + 5][3600] = 1.5                     # a term past the base's vocabulary, first seen in the second block
    maps[N0 + 300][3600] = 0.25
    maps[N0 + 5][3200] = 0.5                     # a known term without a posting in the base
    return maps


def equal(p, q):
    assert p.n_docs == q.n_docs and p.n_terms == q.n_terms
    for a, b in ((p.indptr, q.indptr), (p.doc, q.doc), (p.weight, q.weight)):
        assert a.dtype == b.dtype
        np.testing.assert_array_equal(a, b)


def test_extend_equals_a_rebuild_and_the_block_is_relative(corpus):
    post = LexicalPostings.from_weights(corpus[:N0], V0)
    at = N0
    for n, vt in zip(BLOCKS, (V0, V, V)):
        block = post.extend(corpus[at:at + n], vt)
        alone = LexicalPostings.from_weights(corpus[at:at + n], vt)
        np.testing.assert_array_equal(block["indptr"], alone.indptr)
        np.testing.assert_array_equal(block["doc"], alone.doc)
        np.testing.assert_array_equal(block["weight"], alone.weight)
        assert (block["n_docs"], block["n_terms_total"]) == (n, vt)
        assert block["doc"].size == 0 or (0 <= block["doc"].min() and block["doc"].max() < n)
        at += n
        equal(post, LexicalPostings.from_weights(corpus[:at], vt))
    assert post.indptr[3601] - post.indptr[3600] == 2 and post.indptr[3201] - post.indptr[3200] == 1
    # the cut of the merged mirror at the old size is the old mirror
    ip, doc, w = S.cut(post.indptr, post.doc, post.weight, N0)
    base = LexicalPostings.from_weights(corpus[:N0], V)
    np.testing.assert_array_equal(ip, base.indptr)
    np.testing.assert_array_equal(doc, base.doc)
    np.testing.assert_array_equal(w, base.weight)
    # a LexicalPostings block is taken as it is; a vocabulary may not shrink
    again = LexicalPostings.from_weights(corpus[:N0], V0)
    again.extend(LexicalPostings.from_weights(corpus[N0:N0 + 701], V))
    equal(again, LexicalPostings.from_weights(corpus[:N0 + 701], V))
    with pytest.raises(ValueError):
        again.extend(corpus[:1], V0)


@pytest.mark.parametrize("rows", [np.r_[0, 7, 2999], np.r_[3000:3801], np.r_[0:3000], np.r_[3005, 3300], np.r_[0:5801]],
                         ids=["base", "tail", "whole base", "a term loses every posting", "everything"])
def test_compacted_equals_a_rebuild_from_the_surviving_maps(corpus, rows):
    post = LexicalPostings.from_weights(corpus[:N0], V0)
    at = N0
    for n, vt in zip(BLOCKS, (V0, V, V)):
        post.extend(corpus[at:at + n], vt)
        at += n
    live = np.ones(N_ALL, dtype=bool)
    live[rows] = False
    rm = np.where(live, np.cumsum(live) - 1, -1)
    post.compacted(rm)
    left = [corpus[i] for i in np.nonzero(live)[0]]
    if left:
        equal(post, LexicalPostings.from_weights(left, V))
    else:
        assert post.n_docs == 0 and post.nnz == 0 and post.n_terms == V and not post.indptr.any()
    if rows.tolist() == [3005, 3300]:
        assert post.indptr[3601] == post.indptr[3600] and post.indptr[3201] == post.indptr[3200]
    with pytest.raises(ValueError):
        post.compacted(np.zeros(post.n_docs + 1, dtype=np.int64))
    if post.n_docs > 1:
        with pytest.raises(ValueError):
            post.compacted(np.arange(post.n_docs, dtype=np.int64)[::-1])
