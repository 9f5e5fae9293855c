"""CPU: the argument behind the linear fusion over row shards, in numpy on the inputs the GPU tests use
(tests/linear_sharded_tools.py). A shard that fuses with the GLOBAL BM25 maximum and reports its top-k, merged by (hybrid
descending, id ascending), gives the whole-corpus fusion bit for bit - ids, hybrid and the three components - because every
operand but the maximum is per row and the order is total. A shard that fuses with its OWN maximum does not: the inputs are
built so that this shows, and the first tests pin that. The last test pins the new entry points in the header, the ctypes
table and the built library."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as G
import linear_sharded_tools as L
from oracle import rag_oracle as O

NEW_EXPORTS = ("rag_hybrid_linear_batch", "rag_hybrid_linear_begin_dev", "rag_hybrid_linear_begin_tenants_dev",
               "rag_hybrid_linear_finish_dev", "rag_hybrid_linear_finish_tenants_dev", "rag_hybrid_linear_merge_gathered_dev")
_R = {}


def ref():
    """whole-corpus cosines and raw scores, and the same from each shard's OWN rows and postings (not slices of the whole)"""
    if not _R:
        w = L.world()
        post = L.postings()
        sem = L.cosines(w["q_emb"], w["emb"])
        shards = []
        for lo, hi in L.BOUNDS:
            p = post.shard(lo, hi)
            raw = np.stack([O.bm25_scores_csr(p.indptr, p.doc, p.tf, p.doc_len, p.idf, p.avgdl, t) for t in w["terms_of"]])
            shards.append(dict(lo=lo, hi=hi, raw=raw, sem=L.cosines(w["q_emb"], w["emb"][lo:hi]), temporal=w["temporal"][lo:hi]))
        _R.update(sem=sem, shards=shards)
    return _R


def sharded(tenant, weights, temporal=True, local=False):
    """the protocol in numpy: local maxima -> their maximum (or, local=True, each shard's own) -> shard top-k -> merge"""
    r = ref()
    masks = [L.seen(tenant, s["lo"], s["hi"]) for s in r["shards"]]
    maxima = np.stack([L.local_max(s["raw"], m) for s, m in zip(r["shards"], masks)])
    parts = []
    for i, (s, m) in enumerate(zip(r["shards"], masks)):
        div = L.divisor(maxima[i] if local else maxima.max(axis=0))
        t = s["temporal"] if temporal else np.zeros(s["hi"] - s["lo"])
        parts.append(L.fuse_topk(s["sem"], s["raw"], t, m, div, weights, L.K, id_base=s["lo"]))
    return L.merge(parts, L.K), maxima


def whole(tenant, weights, temporal=True):
    w, r = L.world(), ref()
    m = L.seen(tenant)
    t = w["temporal"] if temporal else np.zeros(L.N)
    return L.fuse_topk(r["sem"], w["raw"], t, m, L.divisor(L.local_max(w["raw"], m)), weights, L.K)


def test_the_inputs_test_the_feature():
    w, r = L.world(), ref()
    assert L.N > 2 * 2048 and L.BOUNDS[2][1] - L.BOUNDS[2][0] < L.K, "three BM25 ranges; the last shard is shorter than k"
    counts = np.diff(w["indptr"])
    assert (counts > 1000).sum() >= 3 and ((counts >= 40) & (counts <= 1000)).sum() >= 20 and (counts < 12).sum() >= 100
    for s in r["shards"]:                                                # a shard's own postings give the bits of the whole
        np.testing.assert_array_equal(L.bits(s["raw"]), L.bits(w["raw"][:, s["lo"]:s["hi"]]))
        np.testing.assert_array_equal(L.bits(s["sem"]), L.bits(r["sem"][:, s["lo"]:s["hi"]]))
    masks = [L.seen(-1, s["lo"], s["hi"]) for s in r["shards"]]
    maxima = np.stack([L.local_max(s["raw"], m) for s, m in zip(r["shards"], masks)])
    best = maxima.max(axis=0)
    one_shard = ((maxima == best[None, :]).sum(axis=0) == 1) & (best > 0)
    assert one_shard.sum() * 4 >= L.Q, "the best BM25 document of a quarter of the queries lies on one shard only"
    assert (w["raw"][0] == 0).all() and np.isneginf(maxima[2]).sum() == 0 and (maxima[:, 0] == 0).all()
    assert (w["raw"][1][:L.BOUNDS[1][0]] == 0).all() and (w["raw"][1][L.BOUNDS[1][1]:] == 0).all() and w["raw"][1].max() > 0
    a, b = L.TIE
    assert r["sem"][2, a] == r["sem"][2, b] and w["raw"][2, a] == w["raw"][2, b] > 0 and w["temporal"][a] == w["temporal"][b]
    assert not (w["tenants"][L.BOUNDS[2][0]:] == 2).any() and (w["tenants"][:L.BOUNDS[2][0]] == 2).any()
    assert not w["visible"][int(np.argmax(w["raw"][3]))] and all((~w["visible"][lo:hi]).any() for lo, hi in L.BOUNDS)
    # a tenant without a row on a shard: that shard reports -inf, and the maximum of the finite entries is the tenant's maximum
    m2 = np.stack([L.local_max(s["raw"], L.seen(2, s["lo"], s["hi"])) for s in r["shards"]])
    assert np.isneginf(m2[2]).all() and np.isfinite(m2[:2]).all()


@pytest.mark.parametrize("tenant", (-1, 1, "per query"))
@pytest.mark.parametrize("weights,temporal", [(L.WEIGHTS, True), ((0.7, 0.0, 0.3), True), ((0.6, 0.4, 0.0), False), ((0.5, -0.3, -0.2), True)])
def test_global_maximum_and_merge_are_the_whole_corpus_fusion(tenant, weights, temporal):
    t = L.world()["tenant_q"] if tenant == "per query" else tenant
    got, maxima = sharded(t, weights, temporal)
    exp = whole(t, weights, temporal)
    L.assert_same(got, exp)
    if tenant == -1 and weights == L.WEIGHTS:
        assert got[0][2, :2].tolist() == list(L.TIE), "the tie across two shards: lower id first"
        assert (got[0][:, L.K - 1] >= 0).all()
    if tenant == "per query":
        assert (got[0][:, 0] >= 0).all()


def test_local_maxima_do_not_merge_into_the_whole_corpus_fusion():
    got, maxima = sharded(-1, L.WEIGHTS, local=True)
    exp = whole(-1, L.WEIGHTS)
    assert (np.stack([np.unique(m).size for m in maxima.T]) > 1).sum() * 4 >= L.Q, "the shards' maxima differ"
    differ = [q for q in range(L.Q) if got[0][q].tolist() != exp[0][q].tolist()]
    assert differ, "fusing with local maxima must change the top-k of at least one query"
    assert 0 not in differ, "a query without any match has divisor 1.0 everywhere: local and global agree"


def test_merge_skips_padding_and_carries_components():
    ids = np.array([[[7, -1, 3]], [[-1, 5, 9]], [[-1, -1, -1]]])
    hyb = np.array([[[1.0, 9.0, 0.5]], [[9.0, 1.0, 0.5]], [[9.0, 9.0, 9.0]]])
    comp = [hyb + i for i in (10, 20, 30)]
    got = L.merge([(ids[r], hyb[r]) + tuple(c[r] for c in comp) for r in range(3)], 5)
    np.testing.assert_array_equal(got[0], [[5, 7, 3, 9, -1]])
    np.testing.assert_array_equal(got[1], [[1.0, 1.0, 0.5, 0.5, 0.0]])
    np.testing.assert_array_equal(got[3], [[21.0, 21.0, 20.5, 20.5, 0.0]])


def test_new_entry_points_are_declared_bound_and_exported():
    from optimized_rag_amd import _lib, sharded as S
    G.build()
    hdr = open(os.path.join(G.ROOT, "include", "rag_hip.h")).read()
    declared = set(re.findall(r"\b(rag_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load_library()
    for name in NEW_EXPORTS:
        assert name in declared, name
        assert name in _lib.exported_symbols(), name
        assert hasattr(lib, name), name
    assert lib.rag_hybrid_linear_begin_tenants_dev.argtypes[4] is ctypes.c_void_p
    assert lib.rag_hybrid_linear_finish_tenants_dev.argtypes[9] is ctypes.c_void_p
    for m in ("hybrid_linear_batch", "hybrid_linear_begin_dev", "hybrid_linear_finish_dev", "hybrid_linear_merge_gathered_dev"):
        assert callable(getattr(_lib.RagEngine, m)), m
    assert callable(S.ShardedHybridIndex.search_linear)
    # no handle: an error code, never a crash (nothing here touches a GPU)
    n = ctypes.c_int(0)
    assert lib.rag_hybrid_linear_batch(None, ctypes.byref(n)) != 0
    assert lib.rag_hybrid_linear_begin_dev(None, None, None, 1, -1, None, None) != 0
    assert lib.rag_hybrid_linear_finish_dev(None, None, None, 1, 1, 1, 0.5, 0.3, 0.2, -1, None, None) != 0
    assert lib.rag_hybrid_linear_merge_gathered_dev(None, None, 1, 1, 1, None, None, None, None, None, None) != 0
