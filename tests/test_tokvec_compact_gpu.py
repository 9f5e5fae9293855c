"""GPU: the resident token-vector store through rag_index_compact_live. Documents of 0, 1, 15, 16, 17, 33, 255 and 257 rows in a
seeded order over a 32-d dense index; the staging chunk forced to 64 rows (a 255-row document spans chunks) and at its default.
Everything is bit for bit: rag_tokvec_fetch_host of every survivor against the bits from before, the reranks and
rag_retrieve_maxsim_dev against a fresh handle with the surviving documents loaded and against the handle's own results from
before the call through the row map."""
import numpy as np
import pytest

import sparse_tools as S
import tokvec_compact_tools as C
import tokvec_tools as TV

pytestmark = pytest.mark.gpu

DIM_INDEX, Q, POOL, K = 32, 4, 16, 8
_W = {}

DELETES = {
    "first, last, a run, a 0-row and the 1-row document in front of the 255-row one": [0, 5, 6, 7, 8, C.ONE, C.ZERO, C.N_DOCS - 1],
    "the 1-row document alone": [C.ONE],
    "every document": list(range(C.N_DOCS)),
}


def world(dim):
    if dim not in _W:
        rng = np.random.default_rng(100 + dim)
        vecs, off = C.make_store(dim)
        n_index = 50                                             # more rows than the store has documents: the tests cut
        emb = rng.standard_normal((n_index, DIM_INDEX)).astype(np.float32)
        q_lens = np.array([5, 32, 33, 1])
        q_off = np.zeros(Q + 1, dtype=np.int64)
        np.cumsum(q_lens, out=q_off[1:])
        ip, doc, wt = S.make_corpus(n_index, 1200, seed=9)       # 200 terms with postings
        by_df = np.argsort(-np.diff(ip), kind="stable")
        sq = [(by_df[[0, 3, 9]], np.array([1.0, 0.5, 2.0], np.float32)), (by_df[[1, 2]], np.array([0.75, 1.5], np.float32)),
              (by_df[[4, 40, 7, 11]], np.array([1.0, 1.0, 0.25, 0.5], np.float32)), (by_df[[5]], np.array([1.0], np.float32))]
        w = dict(vecs=vecs, off=off, emb=emb, ids=(rng.permutation(n_index) + 5000).astype(np.int64),
                 q_emb=(emb[[3, 17, 30, 38]] + 0.2 * rng.standard_normal((Q, DIM_INDEX))).astype(np.float32),
                 q_vecs=TV.unit_rows(rng, int(q_off[-1]), dim), q_off=q_off, sparse=(ip, doc, wt), sq=S.pack_queries(sq),
                 cand=np.stack([rng.permutation(C.N_DOCS)[:POOL] for _ in range(Q)]).astype(np.int32))
        for v in w.values():
            for a in (v if isinstance(v, tuple) else (v,)):
                a.setflags(write=False)
        _W[dim] = w
    return _W[dim]


def sparse_rows(w, rows):
    """the sparse CSR of the world's documents `rows` (ascending), renumbered"""
    ip, doc, wt = w["sparse"]
    inv = np.full(len(w["emb"]), -1, dtype=np.int64)
    inv[rows] = np.arange(len(rows))
    term = np.repeat(np.arange(ip.shape[0] - 1, dtype=np.int64), np.diff(ip))
    keep = inv[doc] >= 0
    out = np.zeros_like(ip)
    np.cumsum(np.bincount(term[keep], minlength=ip.shape[0] - 1), out=out[1:])
    return out, inv[doc[keep]].astype(np.int32), wt[keep].copy()        # the renumbering is monotone: the order inside a term stays


def handle(w, rows, docs, chunk=0, docs_cap=None, sparse=True):
    """index rows `rows` of the world, the store's documents `docs`; the reservation is exactly the rows of `docs`"""
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=DIM_INDEX, device=0)
    e.set_option("tokvec_compact_rows", chunk)
    e.index_load(np.array(w["emb"][rows]), ids=np.array(w["ids"][rows]))
    off = w["off"]
    lens = np.diff(off)[docs]
    e.tokvec_reserve(docs_cap or max(1, len(docs)), int(lens.sum()), w["vecs"].shape[1])
    if len(docs):
        new_off = np.zeros(len(docs) + 1, dtype=np.int64)
        np.cumsum(lens, out=new_off[1:])
        v = np.concatenate([w["vecs"][off[d]:off[d + 1]] for d in docs]) if lens.sum() else np.zeros((0, w["vecs"].shape[1]), np.float32)
        e.tokvec_append(v, new_off)
    if sparse and len(rows):
        e.sparse_load(*sparse_rows(w, rows), len(rows))
    return e


def searches(e, w, cand, retrieve=True):
    import torch
    out = {"rerank": e.tokvec_rerank(np.array(w["q_vecs"]), np.array(w["q_off"]), cand, K)}
    if retrieve:
        t = lambda a: torch.from_numpy(np.array(a)).cuda()
        qe, qv, qo = t(w["q_emb"]), t(w["q_vecs"]), t(w["q_off"])
        ptr, terms, wts = (t(a) for a in w["sq"])
        pool = min(POOL, e.n_rows)
        for mode, kw in (("mode 0", {}), ("mode 1", dict(term_ptr=ptr, terms=terms, weights=wts))):
            r = e.retrieve_maxsim_dev(qe, qv, qo, pool, min(K, pool), **kw)
            torch.cuda.synchronize()
            out[mode] = tuple(x.cpu().numpy() for x in r)
    return out


def same(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        for x, y in zip(a[name], b[name]):
            assert x.shape == y.shape and x.dtype == y.dtype, f"{what}: {name}"
            view = {np.dtype(np.float64): np.int64, np.dtype(np.float32): np.int32}.get(x.dtype)
            np.testing.assert_array_equal(x.view(view) if view else x, y.view(view) if view else y, err_msg=f"{what}: {name}")


@pytest.mark.parametrize("chunk", [64, 0])
@pytest.mark.parametrize("dim", [32, 1024])
@pytest.mark.parametrize("name", list(DELETES))
def test_store_moves_with_its_rows(name, dim, chunk):
    from optimized_rag_amd._lib import RagError
    w = world(dim)
    n = C.N_DOCS
    deleted = np.asarray(DELETES[name])
    live = np.setdiff1d(np.arange(n), deleted)
    e = handle(w, np.arange(n), np.arange(n), chunk, docs_cap=n + 4)
    try:
        stored = [e.tokvec_fetch(d) for d in range(n)]
        for d in range(n):
            np.testing.assert_array_equal(stored[d], w["vecs"][w["off"][d]:w["off"][d + 1]])
        assert e.index_delete(np.array(w["ids"][deleted])) == len(deleted)
        cand_old = np.where(np.isin(w["cand"], deleted), -1, w["cand"]).astype(np.int32)      # explicit rows are not filtered: leave them out
        before = searches(e, w, cand_old, retrieve=len(live) > 0)
        info0 = e.tokvec_info()
        rm = e.index_compact(keep_resident=True)
        np.testing.assert_array_equal(np.nonzero(rm < 0)[0], deleted)
        info = e.tokvec_info()
        rows_left = int(np.diff(w["off"])[live].sum())
        assert (info["n_docs"], info["rows"], info["dim"], info["hbm_bytes"]) == (len(live), rows_left, dim, info0["hbm_bytes"])
        for new, d in enumerate(live):
            np.testing.assert_array_equal(e.tokvec_fetch(new).view(np.int32), stored[d].view(np.int32), err_msg=f"document {d}")
        if len(live):
            cand_new = np.where(cand_old >= 0, rm[np.maximum(cand_old, 0)], -1).astype(np.int32)
            got = searches(e, w, cand_new)
            f = handle(w, live, live)
            try:
                same(got, searches(f, w, cand_new), name + ": fresh handle")
            finally:
                f.close()
            ids, rows, sc, ps = before["rerank"]
            before["rerank"] = (ids, np.where(rows >= 0, rm[np.maximum(rows, 0)], -1).astype(np.int32), sc, ps)
            same(got, before, name + ": before the call, through the row map")
            assert (got["rerank"][1] >= 0).any() and (got["mode 1"][0] >= 0).any()
        # the freed rows are headroom of the same reservation: exactly as many fit again, not one more
        freed = int(w["off"][-1]) - rows_left
        assert freed > 0
        e.tokvec_append(np.array(w["vecs"][:freed]), np.array([0, freed - 1, freed], dtype=np.int64))
        assert e.tokvec_info()["rows"] == int(w["off"][-1]) and e.tokvec_info()["n_docs"] == len(live) + 2
        np.testing.assert_array_equal(e.tokvec_fetch(len(live) + 1), w["vecs"][freed - 1:freed])
        with pytest.raises(RagError, match=r"\(-1\).*reserved rows"):
            e.tokvec_append(np.array(w["vecs"][:1]), np.array([0, 1], dtype=np.int64))
    finally:
        e.close()


@pytest.mark.parametrize("n_index", [30, 50])
def test_a_store_ahead_of_or_behind_the_index(n_index):
    """30 index rows under 40 stored documents: the 10 extra documents follow the survivors. 50 rows over 40 documents: the rows
    past the store do not concern it."""
    w = world(32)
    n = C.N_DOCS
    deleted = np.array([2, C.ONE, 29] + ([45] if n_index > n else []))
    e = handle(w, np.arange(n_index), np.arange(n), 64, sparse=False)
    try:
        stored = [e.tokvec_fetch(d) for d in range(n)]
        assert e.index_delete(np.array(w["ids"][deleted])) == len(deleted)
        rm = e.index_compact(keep_resident=True)
        keep = C.keep_of(n, rm)
        left = np.nonzero(keep)[0]
        assert len(left) == n - 3 and e.tokvec_info()["n_docs"] == n - 3 and e.tokvec_info()["rows"] == int(np.diff(w["off"])[left].sum())
        for new, d in enumerate(left):
            np.testing.assert_array_equal(e.tokvec_fetch(new).view(np.int32), stored[d].view(np.int32), err_msg=f"document {d}")
        cand = np.stack([np.arange(POOL) + 20] * Q).astype(np.int32)         # rows on both sides of the index's end
        got = e.tokvec_rerank(np.array(w["q_vecs"]), np.array(w["q_off"]), cand, K)
        f = handle(w, np.setdiff1d(np.arange(n_index), deleted), left, sparse=False)
        try:
            for x, y in zip(got, f.tokvec_rerank(np.array(w["q_vecs"]), np.array(w["q_off"]), cand, K)):
                np.testing.assert_array_equal(x, y)
        finally:
            f.close()
    finally:
        e.close()


def test_a_plain_compaction_still_marks_the_store_stale_and_nothing_deleted_moves_nothing():
    from optimized_rag_amd._lib import RagError
    w = world(32)
    n = C.N_DOCS
    e = handle(w, np.arange(n), np.arange(n), 64)
    try:
        info = e.tokvec_info()
        np.testing.assert_array_equal(e.index_compact(keep_resident=True), np.arange(n))
        assert e.tokvec_info() == info
        e.index_delete(np.array(w["ids"][[3]]))
        e.index_compact(keep_postings=True)
        with pytest.raises(RagError, match=r"\(-3\).*stale"):
            e.tokvec_rerank(np.array(w["q_vecs"]), np.array(w["q_off"]), np.array(w["cand"]), K)
        e.index_delete(np.array(w["ids"][[4]]))
        e.index_compact(keep_resident=True)                          # a stale store stays stale and is not moved
        assert e.tokvec_info() == info
        with pytest.raises(RagError, match=r"\(-3\).*stale"):
            e.tokvec_rerank(np.array(w["q_vecs"]), np.array(w["q_off"]), np.array(w["cand"]), K)
    finally:
        e.close()
