"""CPU: the surfaces and the numpy references of the three-way bge-m3 score (tests/m3_fused_tools.py). The four entries are declared
and in the ctypes table; the point-lookup reference has the bits of the all-document reference on corpus A; the reference combine
is m3_tools.combine in both of upstream's weighted modes."""
import os
import re

import numpy as np

import m3_fused_tools as F
import m3_tools as M
import sparse_tools as S

NAMES = ("rag_sparse_score_rows_dev", "rag_sparse_score_rows_host", "rag_m3_score_rows_dev", "rag_retrieve_m3_dev")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_four_entries_are_declared_and_in_the_ctypes_table():
    from optimized_rag_amd import RagEngine, _lib
    header = open(os.path.join(ROOT, "include", "rag_hip.h")).read()
    for name in NAMES:
        assert name in _lib.exported_symbols()
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, name + " is not declared in include/rag_hip.h"
        n_args = len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","))
        assert n_args == len(_lib._SIGS[name][0]), name
    for method in ("sparse_score_rows", "sparse_score_rows_dev", "m3_score_rows_dev", "retrieve_m3_dev"):
        assert callable(getattr(RagEngine, method))
    from optimized_rag_amd.document_store import GpuDocumentIndex
    assert callable(GpuDocumentIndex.search_m3)


def test_corpus_a_is_the_corpus_the_issue_describes():
    a = F.corpus_a()
    df = np.diff(a["indptr"])
    assert a["indptr"][-1] == 131_731 and (df == 0).sum() == 1000 and ((df > 0) & (df < 8)).sum() == 315
    assert len(a["queries"]) == 32 and len(a["queries"][0][0]) == 70


def test_point_reference_has_the_bits_of_the_all_document_reference():
    a = F.corpus_a()
    cand = F.slots_a()
    assert cand.shape == (32, 19) and (cand[:, -2] == -1).all() and (cand[:, -1] == F.N_A).all()
    got = F.point_scores(a["indptr"], a["doc"], a["w"], F.N_A, a["queries"], cand)
    ok = (cand >= 0) & (cand < F.N_A)
    exp = np.where(ok, np.take_along_axis(a["all"], np.clip(cand, 0, F.N_A - 1).astype(np.int64), axis=1), 0.0)
    np.testing.assert_array_equal(S.bits(got), S.bits(exp))
    assert (got[:, 11] > 0).sum() >= 28 and (got[~ok] == 0).all()       # the queries' own best rows score; the empty slots do not
    # the 300-token query: the same bits from the point reference and the range-wise one
    lq = [F.long_query()]
    full = S.all_scores(a["indptr"], a["doc"], a["w"], F.N_A, lq)
    got = F.point_scores(a["indptr"], a["doc"], a["w"], F.N_A, lq, cand[:1])
    exp = np.where(ok[:1], full[0][np.clip(cand[:1], 0, F.N_A - 1)], 0.0)
    np.testing.assert_array_equal(S.bits(got), S.bits(exp))
    assert (got > 0).sum() >= 3


def test_reference_combine_is_m3_tools_combine_in_both_modes():
    rng = np.random.default_rng(0)
    d, s, c = rng.uniform(-1, 1, 500), rng.uniform(0, 30, 500), rng.uniform(-1, 1, 500).astype(np.float32)
    s[:50] = 0.0
    c[40:90] = 0.0
    for w in ((0.4, 0.2, 0.4), (1.0, 0.3, 1.0), (0.15, 1.7, 0.9)):
        exp = M.combine(d, s, c, w)
        np.testing.assert_array_equal(S.bits(F.combine(d, s, c, w)), S.bits(exp["colbert+sparse+dense"]))
        two = (w[0], w[1], 0.0)
        np.testing.assert_array_equal(S.bits(F.combine(d, s, c, two)), S.bits(exp["sparse+dense"]))
        np.testing.assert_array_equal(S.bits(F.combine(d, s, np.zeros_like(c), two)), S.bits(exp["sparse+dense"]))
