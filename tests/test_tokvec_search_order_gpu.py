"""GPU: stream order, call history and output bounds of the exhaustive MaxSim search (mode 2 of rag_retrieve_maxsim_dev and of
rag_retrieve_maxsim_tenants_dev), with the tools the existing suites use: tests/stream_tools.py (serial, late_producer) and
tests/guard_tools.py. The world is tests/tokvec_search_tools.py's; what the lists must BE is tests/test_tokvec_search_gpu.py's
business - here a call is compared with the same call made alone on a fresh handle.

  inputs produced late on the stream are honoured, and the call does not wait for the work queued before it;
  Q = 9 -> 2 -> 9 on one handle, with modes 0 / 1 and a rag_retrieve_m3_dev between (they carve the same workspace): the bits of a
  fresh handle's single call - the plane, the row lists and the rerank's slots are written whole by every call;
  guard bytes around ids_out, scores_out and cand_out stay intact at k = pool = 1 and at a pool that divides nothing."""
import numpy as np
import pytest

import guard_tools as G
import sparse_tools as S
import stream_tools as T
import tokvec_search_tools as W

pytestmark = pytest.mark.gpu

Q = len(W.Q_ROWS)
POOL, K = 37, 10
DELETED = (0, W.LAST_PLAIN, 451)
_SPARSE = {}


def sparse_world():
    if not _SPARSE:
        indptr, doc, w = S.make_corpus(n_docs=W.N_DOCS, n_terms=3000, seed=5)
        _SPARSE.update(indptr=indptr, doc=doc, w=w, packed=S.pack_queries(S.make_queries(indptr, seed=6)[:Q]))
    return _SPARSE


def load(form, dim):
    from optimized_rag_amd import RagEngine
    w, sp = W.world(dim), sparse_world()
    e = RagEngine(dim=W.INDEX_DIM, device=0)
    e.index_load(w["emb"], id_base=1000)
    e.set_tenants(w["tenants"])
    e.sparse_load(sp["indptr"], sp["doc"], sp["w"], W.N_DOCS)
    e.tokvec_load(w["vecs"], w["off"], form=form)
    assert e.index_delete(1000 + np.array(DELETED, np.int64)) == 3
    return e


@pytest.fixture(scope="module", params=[("fp16", 128), ("mxfp8", 96)], ids=lambda p: f"{p[0]}-{p[1]}")
def rig(request):
    form, dim = request.param
    e = load(form, dim)
    yield dict(e=e, w=W.world(dim), form=form, dim=dim)
    e.close()


def first_queries(w, n):
    """the token vectors and offsets of the world's first n queries"""
    return dict(qv=w["qv"][:int(w["qo"][n])] if n < Q else w["qv"], qo=w["qo"][:n + 1])


def bind(e, pool, k, tenant):
    def call(d, s):
        return list(e.tokvec_search_dev(d["qv"], d["qo"], k, pool=pool, tenant=tenant, stream=s))
    return call


@pytest.mark.parametrize("tenant", [-1, "per_query"])
def test_late_inputs_are_honoured_and_the_call_does_not_wait(rig, tenant):
    import torch
    real = first_queries(rig["w"], Q)
    wrong = dict(qv=np.zeros_like(real["qv"]), qo=np.zeros_like(real["qo"]))       # legal: nine queries without rows
    call = bind(rig["e"], POOL, K, W.PER_QUERY if tenant == "per_query" else tenant)
    ref = T.serial(call, wrong, real)
    assert (ref[0][1:, 0] >= 0).all() and (ref[2][1:, POOL - 1] >= 0).all()
    got, pending = T.late_producer(call, wrong, real, torch.cuda.Stream())
    assert pending, "mode 2 of rag_retrieve_maxsim_dev waited for the work queued before it on its stream"
    T.assert_same(got, ref, f"mode 2 behind a late producer, tenant {tenant}")


def test_nothing_of_an_earlier_call_shows(rig):
    """9 -> modes 0 and 1 -> 2 -> retrieve_m3_dev -> 9 queries on one handle against single calls on a fresh one"""
    import torch
    w, e = rig["w"], rig["e"]
    ptr, terms, wts = sparse_world()["packed"]
    dev9 = T.to_dev(dict(q_emb=w["q_emb"], ptr=ptr, terms=terms, w=wts, **first_queries(w, Q)))
    dev2 = T.to_dev(first_queries(w, 2 + 2))                                        # queries 0 .. 3: the first has no rows
    dev2 = dict(qv=dev2["qv"][int(w["qo"][2]):], qo=(dev2["qo"][2:] - int(w["qo"][2])).contiguous())      # queries 2 and 3
    assert dev2["qv"].data_ptr() % 16 == 0
    ten2 = W.PER_QUERY[2:4].copy()

    def run(eng, d, pool, k, tenant):
        out = eng.tokvec_search_dev(d["qv"], d["qo"], k, pool=pool, tenant=tenant)
        torch.cuda.synchronize()
        return T.to_np(out)

    fresh = load(rig["form"], rig["dim"])
    try:
        ref9, ref2 = run(fresh, dev9, 256, 20, W.PER_QUERY), None
    finally:
        fresh.close()
    fresh = load(rig["form"], rig["dim"])
    try:
        ref2 = run(fresh, dev2, 5, 5, ten2)
    finally:
        fresh.close()
    T.assert_same(run(e, dev9, 256, 20, W.PER_QUERY), ref9, "the first large call")
    sp = dict(term_ptr=dev9["ptr"], terms=dev9["terms"], weights=dev9["w"])
    e.retrieve_maxsim_dev(dev9["q_emb"], dev9["qv"], dev9["qo"], POOL, K)
    e.retrieve_maxsim_dev(dev9["q_emb"], dev9["qv"], dev9["qo"], POOL, K, **sp)
    T.assert_same(run(e, dev2, 5, 5, ten2), ref2, "the small call after modes 0 and 1")
    e.retrieve_m3_dev(dev9["q_emb"], POOL, K, q_vecs=dev9["qv"], q_off=dev9["qo"], mode=2, **sp)
    T.assert_same(run(e, dev9, 256, 20, W.PER_QUERY), ref9, "the large call after the small one and retrieve_m3_dev")
    np.testing.assert_array_equal(ref9[0][[2, 3]][:, :5], ref2[0], err_msg="a query's list does not depend on its batch")


@pytest.mark.parametrize("pool,k", [(1, 1), (37, 7), (256, 256)])
@pytest.mark.parametrize("per_query", [False, True])
def test_the_outputs_are_written_inside_their_arrays(rig, monkeypatch, pool, k, per_query):
    import torch
    w, e = rig["w"], rig["e"]
    dev = T.to_dev(first_queries(w, Q))
    ref = T.to_np(e.tokvec_search_dev(dev["qv"], dev["qo"], k, pool=pool, tenant=W.PER_QUERY if per_query else 2))
    torch.cuda.synchronize()
    ref = [r.copy() for r in ref]
    guards = G.Guards()
    G.patch_torch(monkeypatch, guards)
    e._ts_key = None                                                     # the method allocates its outputs again: guarded ones
    out = e.tokvec_search_dev(dev["qv"], dev["qo"], k, pool=pool, tenant=W.PER_QUERY if per_query else 2)
    assert guards.check() == 3
    T.assert_same(T.to_np(out), ref, "guarded outputs")
    assert all(o.data_ptr() % 16 == o.element_size() for o in out)
    e._ts_key = None
