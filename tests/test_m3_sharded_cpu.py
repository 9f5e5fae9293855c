"""CPU: the references of the row-sharded bge-m3 search (tests/m3_sharded_tools.py) run over three unequal shards of corpus A
reproduce the UNSHARDED references array for array: sparse_tools.topk for the sparse list, a (score descending, row ascending)
sort for the dense list, the oracle's RRF for the candidates, m3_fused_tools.combine + tokvec_tools.stable_topk for the ranking.
This is the argument the GPU tests then hold the library to: every score is a function of (query, row), the order (score, id) is
total, so merged per-shard lists ARE the global lists, and a slot scored by its owner carries the bits the unsharded call computes."""
import numpy as np
import pytest

import m3_fused_tools as F
import m3_sharded_tools as H
import m3_tools as M
import sparse_tools as S
import tokvec_tools as V
from oracle import rag_oracle as O

N, POOL, K = F.N_A, F.POOL, 10
BOUNDS = ((0, 4096), (4096, 10260), (10260, N))                          # the last shard has fewer rows than POOL
_R = {}


def ref():
    """dense [32, N] and sparse [32, N] float64 scores of every document, the unsharded lists, the per-shard lists"""
    if not _R:
        w, a = F.world(), F.corpus_a()
        dense = np.stack([F.cosine64(w["q_emb"][q], w["emb"]) for q in range(32)])
        sparse = a["all"]
        d_ids = np.stack([np.lexsort((np.arange(N), -dense[q]))[:POOL] for q in range(32)]).astype(np.int64)
        d_sc = np.take_along_axis(dense, d_ids, axis=1)
        s_ids, s_sc = S.topk_all(sparse, POOL)
        shard_lists = []
        for lo, hi in BOUNDS:
            n = min(POOL, hi - lo)
            di = np.full((32, POOL), -1, np.int64)
            ds = np.zeros((32, POOL))
            for q in range(32):
                top = np.lexsort((np.arange(hi - lo), -dense[q, lo:hi]))[:n]
                di[q, :n], ds[q, :n] = lo + top, dense[q, lo + top]
            si, ss = S.topk_all(sparse[:, lo:hi], POOL)
            shard_lists.append((di, ds, np.where(si >= 0, si.astype(np.int64) + lo, -1), ss))
        _R.update(dense=dense, sparse=sparse, d_ids=d_ids, d_sc=d_sc, s_ids=s_ids.astype(np.int64), s_sc=s_sc, shards=shard_lists)
    return _R


def colbert(q, row):
    w = F.world()
    vq, vd = w["qv"][w["qo"][q]:w["qo"][q + 1]], w["d_vecs"][w["d_off"][row]:w["d_off"][row + 1]]
    return float(np.float32(M.maxsim(vq, vd))) if len(vq) and len(vd) else 0.0


def test_merged_shard_lists_are_the_unsharded_lists():
    r = ref()
    assert (r["shards"][2][0][:, N - 10260:] == -1).all(), "the short shard pads its dense list"
    di, ds = H.merge([s[0] for s in r["shards"]], [s[1] for s in r["shards"]], POOL)
    np.testing.assert_array_equal(di, r["d_ids"])
    np.testing.assert_array_equal(S.bits(ds), S.bits(r["d_sc"]))
    si, ss = H.merge([s[2] for s in r["shards"]], [s[3] for s in r["shards"]], POOL)
    np.testing.assert_array_equal(si, r["s_ids"])
    np.testing.assert_array_equal(S.bits(ss), S.bits(r["s_sc"]))
    # interior padding is skipped wherever it stands, and equal scores go by id
    i, s = H.merge(np.array([[[7, -1, 3]], [[-1, 5, 9]]]), np.array([[[1.0, 9.0, 0.5]], [[9.0, 1.0, 0.5]]]), 4)
    np.testing.assert_array_equal(i, [[5, 7, 3, 9]])
    np.testing.assert_array_equal(s, [[1.0, 1.0, 0.5, 0.5]])


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_candidates_equal_the_rrf_of_the_unsharded_lists(mode):
    r = ref()
    got = H.candidates(r["d_ids"], r["s_ids"], mode)
    slots = 2 * POOL if mode == 2 else POOL
    assert got.shape == (32, slots)
    for q in range(32):
        if mode == 0:
            exp = list(r["d_ids"][q])
        else:
            exp, _, _ = O.rrf_fuse([[int(x) for x in r["d_ids"][q] if x >= 0], [int(x) for x in r["s_ids"][q] if x >= 0]], k=60, top_k=slots)
        np.testing.assert_array_equal(got[q, :len(exp)], exp)
        assert (got[q, len(exp):] == -1).all()
    # padding holds its position: an id behind a -1 keeps the rank of its place
    np.testing.assert_array_equal(H.rrf([np.array([-1, 4]), np.array([9, -1])], 60, 3), [9, 4, -1])


@pytest.mark.parametrize("weights", F.WEIGHT_SETS)
@pytest.mark.parametrize("mode", (0, 1, 2))
def test_owner_scoring_and_combine_equal_the_unsharded_ranking(mode, weights):
    r = ref()
    wd, ws, wc = weights
    cand = H.candidates(r["d_ids"], r["s_ids"], mode)
    fns = dict(dense=(lambda q, row: r["dense"][q, row]) if wd > 0 else None, sparse=(lambda q, row: r["sparse"][q, row]) if ws > 0 else None,
               colbert=colbert if wc > 0 else None)
    parts = [H.partial(cand, lo, hi, **fns) for lo, hi in BOUNDS]
    owned = np.stack([p[0] for p in parts])
    assert (owned.sum(axis=0) == (cand >= 0)).all(), "every candidate has exactly one owner"
    assert owned[2].any() and owned[0].any()
    ids, sc, comp = H.combine_topk(cand, owned, np.stack([p[1] for p in parts]), weights, K)
    # the unsharded reference: every slot's components from the whole arrays, combine, stable top-k
    whole = H.partial(cand, 0, N, **fns)[1]
    score = F.combine(whole[0], whole[1], whole[2], weights)
    e_ids, e_rows, e_sc = V.stable_topk(score, cand, cand < 0, K)
    np.testing.assert_array_equal(ids, e_ids)
    np.testing.assert_array_equal(S.bits(sc), S.bits(e_sc))
    for q in range(32):
        slot = {int(c): j for j, c in reversed(list(enumerate(cand[q]))) if c >= 0}
        for i, row in enumerate(e_rows[q]):
            exp = whole[:, q, slot[int(row)]] if row >= 0 else np.zeros(3)
            np.testing.assert_array_equal(S.bits(comp[q, i]), S.bits(exp))


def test_overlapping_owners_resolve_to_the_lowest_rank_and_ownerless_slots_are_empty():
    cand = np.array([[5, 6, -1, 7]])
    owned = np.array([[[0, 1, 0, 0]], [[1, 1, 1, 0]]], bool)             # slot 1: two owners; slot 2: owned but cand < 0; slot 3: none
    comp = np.zeros((2, 3, 1, 4))
    comp[0, 0, 0, 1], comp[1, 0, 0, 1], comp[1, 0, 0, 0] = 0.25, 0.75, 0.5
    ids, sc, out = H.combine_topk(cand, owned, comp, (1.0, 0.0, 0.0), 4)
    np.testing.assert_array_equal(ids, [[5, 6, -1, -1]])
    np.testing.assert_array_equal(sc, [[0.5, 0.25, 0.0, 0.0]])
    assert out[0, 1, 0] == 0.25
