"""GPU: stream ordering of the live writes to the learned-sparse postings and the token-vector store. A *_dev search queued on a
side stream behind busy work, BEFORE rag_sparse_append_host / rag_sparse_fold / rag_index_compact_live is called, returns the
result from before the write - every live write first waits for the work the handle's *_dev calls queued."""
import numpy as np
import pytest

import stream_tools as T
import test_sparse_live_gpu as L
import test_tokvec_compact_gpu as G
import tokvec_compact_tools as C

pytestmark = pytest.mark.gpu

K = 20


def queued_sparse_topk(e, w, s):
    """busy work, then rag_sparse_topk_dev on stream s; returns the output tensors (not yet waited for)"""
    import torch
    ptr, terms, wts = (torch.from_numpy(np.array(a)).cuda() for a in w["packed"])
    Q = ptr.shape[0] - 1
    ids = torch.full((Q, K), -7, dtype=torch.int64, device="cuda")
    rows = torch.full((Q, K), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((Q, K), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    T.busy(s, 100.0)
    e.sparse_topk_dev(ptr, terms, wts, K, ids, rows, sc, stream=s)
    return (ids, rows, sc), (ptr, terms, wts)


def test_sparse_search_queued_before_an_append_and_a_fold_sees_the_old_postings():
    import torch
    from optimized_rag_amd import RagEngine
    w = L.world()
    e = RagEngine(dim=L.DIM, device=0)                                # postings alone: appends are always allowed
    try:
        e.set_option("sparse_tail_fold", -1)
        base, more = np.arange(L.N0), np.arange(L.N0, L.N0 + 701)
        e.sparse_load(*L.postings_of(w, base, L.V), L.N0)
        ref_old = e.sparse_topk(*w["packed"], K)
        s = torch.cuda.Stream()
        out, keep = queued_sparse_topk(e, w, s)
        pending = not s.query()
        e.sparse_append(*L.postings_of(w, more, L.V), len(more))      # waits for the queued search
        s.synchronize()
        assert pending, "the stream had drained before the append was called: the test showed nothing"
        T.assert_same(T.to_np(out), list(ref_old), "queued before the append")
        ref_new = e.sparse_topk(*w["packed"], K)
        assert (ref_new[1] >= L.N0).any()
        out, keep = queued_sparse_topk(e, w, s)
        pending = not s.query()
        e.sparse_fold()
        s.synchronize()
        assert pending
        T.assert_same(T.to_np(out), list(ref_new), "queued before the fold")
        T.assert_same(list(e.sparse_topk(*w["packed"], K)), list(ref_new), "after the fold")
    finally:
        e.close()


def test_searches_queued_before_a_compaction_see_the_old_rows():
    import torch
    w = G.world(32)
    n = C.N_DOCS
    e = G.handle(w, np.arange(n), np.arange(n), 64)
    try:
        deleted = np.array([0, C.ONE, 30])
        assert e.index_delete(np.array(w["ids"][deleted])) == 3
        ref = G.searches(e, w, np.array(w["cand"]))
        t = lambda a: torch.from_numpy(np.array(a)).cuda()
        qe, qv, qo = t(w["q_emb"]), t(w["q_vecs"]), t(w["q_off"])
        ptr, terms, wts = (t(a) for a in w["sq"])
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        T.busy(s, 100.0)
        r = e.retrieve_maxsim_dev(qe, qv, qo, G.POOL, G.K, term_ptr=ptr, terms=terms, weights=wts, stream=s)
        with torch.cuda.stream(s):
            clones = [x.clone() for x in r]
        pending = not s.query()
        rm = e.index_compact(keep_resident=True)                      # waits for the queued retrieval
        s.synchronize()
        assert pending, "the stream had drained before the compaction was called: the test showed nothing"
        assert (rm < 0).sum() == 3
        T.assert_same(T.to_np(clones), list(ref["mode 1"]), "queued before the compaction")
        after = G.searches(e, w, np.where(rm[w["cand"]] >= 0, rm[w["cand"]], -1).astype(np.int32))
        T.assert_same(list(after["mode 1"]), list(ref["mode 1"]), "after the compaction (ids and scores do not move)")
    finally:
        e.close()
