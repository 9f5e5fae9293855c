"""CPU: the numpy reference of rag_lexical_compact_* (tests/lexical_compact_tools.py) is what the Python path computes today -
LexicalPostings.encode_queries over the maps of m3_tools.lexical_map (the loop of LocalEmbeddingService.encode_multi) - integer
for integer and float bit for float bit, on every case the GPU test runs; and the case list reaches every class it promises."""
import numpy as np

import lexical_compact_tools as T
import m3_tools as M


def python_path(case):
    """encode_queries over lexical_map's maps. lexical_map has no rule for an id < 0 (a tokenizer never produces one); the
    contract drops such a position, so the negative ids a text holds join its skip set here."""
    from optimized_rag_amd.sparse import LexicalPostings
    ids, w, lens = case["ids"], case["weights"], case["lens"]
    L = ids.shape[1]
    maps = []
    for i in range(ids.shape[0]):
        n = int(np.clip(int(lens[i]), 0, L))
        skip = set(case["skip"]) | {int(x) for x in ids[i, :n] if x < 0}
        maps.append(M.lexical_map(ids[i], w[i], n, skip))
    return LexicalPostings.encode_queries(maps)


def test_reference_equals_the_python_path_on_every_case():
    for case in T.cases():
        ptr, terms, qw = T.compact(case["ids"], case["weights"], case["lens"], case["skip"])
        eptr, eterms, eqw = python_path(case)
        assert ptr.dtype == eptr.dtype == np.int32 and terms.dtype == eterms.dtype == np.int32 and qw.dtype == eqw.dtype == np.float32
        np.testing.assert_array_equal(ptr, eptr, err_msg=case["name"])
        np.testing.assert_array_equal(terms, eterms, err_msg=case["name"])
        np.testing.assert_array_equal(qw.view(np.uint32), eqw.view(np.uint32), err_msg=case["name"])
        assert ptr[0] == 0 and ptr[-1] == terms.shape[0] == qw.shape[0]


def test_cases_reach_every_class():
    cases = T.cases()
    reached = set().union(*(c["classes"] for c in cases))
    assert reached == T.CLASSES
    by = {c["name"]: c for c in cases}
    for L in T.SEQ_LENS:
        c = by[f"seq_len_{L}"]
        assert c["ids"].shape[1] == L and c["lens"].max() == L
        ptr, terms, _ = T.compact(c["ids"], c["weights"], c["lens"], c["skip"])
        if L >= 5:                                                      # the vocabulary repeats: there is something to reduce
            assert 0 < ptr[-1] < np.clip(c["lens"], 0, L).sum()
    for n in T.N_TEXTS:
        assert by[f"n_texts_{n}"]["ids"].shape == (n, 8)
    assert {len(c["skip"]) for c in cases} >= {0, 8}
    # the text shapes are what their names say
    c = by["text_shapes"]
    ptr, terms, qw = T.compact(c["ids"], c["weights"], c["lens"], c["skip"])
    counts = np.diff(ptr)
    assert c["lens"][0] == 0 and counts[0] == 0 and c["lens"][1] > c["ids"].shape[1] and counts[1] > 0
    assert counts[2] == 0 and counts[8] == 0 and c["lens"][2] > 0 and c["lens"][8] > 0        # all special: middle and last
    assert counts[3] == 1 and qw[ptr[3]] == np.float32(0.75)                                  # equal maxima
    for row, at in ((4, 0), (5, 16), (6, 32)):
        assert counts[row] == 1 and terms[ptr[row]] == 30 and qw[ptr[row]] == np.float32(0.875) and c["weights"][row].argmax() == at
    # the weight classes and the id range
    c = by["values_and_id_range"]
    ptr, terms, qw = T.compact(c["ids"], c["weights"], c["lens"], c["skip"])
    first = dict(zip(terms[:ptr[1]].tolist(), qw[:ptr[1]].tolist()))
    assert first == {0: 0.75, 50: float(T.SUBNORMAL), 53: 2.0, 54: float("inf"), 55: float(T.SUBNORMAL), 56: float(np.float32(3e38)),
                     T.INT32_MAX: 0.25}
    assert (c["ids"] < 0).any() and (terms >= 0).all() and terms[:ptr[1]].tolist() == sorted(first)
    assert 0 < float(T.SUBNORMAL) < np.finfo(np.float32).tiny
