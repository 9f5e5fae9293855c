"""GPU: the linear fusion over row shards (rag_hybrid_linear_begin_dev / _finish_dev / _merge_gathered_dev,
ShardedHybridIndex.search_linear) against THE truth: rag_hybrid_linear_dev / _tenants_dev on one unsharded handle holding all rows
(id_base 0, the merged postings, the whole temporal vector). ids, hybrid bits and the three component planes are compared as bits.

Three handles on one GPU hold the unequal contiguous shards of tests/linear_sharded_tools.py (the last has fewer rows than k); the
two gathers are a torch.stack here and real collectives in tests/test_linear_sharded_two_ranks_gpu.py. What the inputs contain, and
why local maxima would not do, is asserted in numpy by tests/test_linear_sharded_cpu.py."""
import numpy as np
import pytest

import linear_sharded_tools as L
import stream_tools as T

pytestmark = pytest.mark.gpu

K = L.K


@pytest.fixture(scope="module")
def handles():
    """(truth, [three shard handles]) with tenants, temporal vectors and the deleted rows"""
    from optimized_rag_amd import RagEngine
    truth = L.load_handle(RagEngine(dim=L.D, device=0), 0, L.N)
    shards = [L.load_handle(RagEngine(dim=L.D, device=0), lo, hi) for lo, hi in L.BOUNDS]
    yield truth, shards
    for e in [truth] + shards:
        e.close()


@pytest.fixture(scope="module")
def small():
    """a handle of its own for the tests that break and reload it: rows [0, 600)"""
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=L.D, device=0)
    yield e
    e.close()


def run_shards(engs, q, ptr, terms, k, weights, tenant=-1, stream=None):
    """the protocol over several handles of one process: the gathers are the stacked buffers"""
    import torch
    n, world = q.shape[0], len(engs)
    mx = torch.empty((world, n), dtype=torch.float64, device="cuda")
    parts = torch.empty((world, 5, n, k), dtype=torch.int64, device="cuda")
    for r, e in enumerate(engs):
        e.hybrid_linear_begin_dev(ptr, terms, mx[r], tenant=tenant, stream=stream)
    for r, e in enumerate(engs):
        e.hybrid_linear_finish_dev(q, mx, k, *weights, parts[r], tenant=tenant, stream=stream)
    o = dict(ids=torch.empty((n, k), dtype=torch.int64, device="cuda"),
             **{name: torch.empty((n, k), dtype=torch.float64, device="cuda") for name in L.NAMES[1:]})
    engs[0].hybrid_linear_merge_gathered_dev(parts, *(o[name] for name in L.NAMES), stream=stream)
    return o, mx, parts


def one_call(eng, q, ptr, terms, k, weights, tenant=-1):
    import torch
    out = L.as_np(eng.hybrid_linear_dev(q, ptr, terms, k, *weights, tenant=tenant))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("tenant", (-1, 1, 2, "per query"))
@pytest.mark.parametrize("weights", [L.WEIGHTS, (0.7, 0.0, 0.3), (0.5, -0.3, -0.2)])
def test_three_shards_equal_the_one_call_entry(handles, weights, tenant):
    import torch
    truth, shards = handles
    q, ptr, terms = L.query_tensors()
    t = L.world()["tenant_q"] if tenant == "per query" else tenant
    exp = one_call(truth, q, ptr, terms, K, weights, t)
    o, mx, _ = run_shards(shards, q, ptr, terms, K, weights, t)
    torch.cuda.synchronize()
    L.assert_same(L.as_np(o), exp, f"{weights} tenant {tenant}")
    mx = mx.cpu().numpy()
    if tenant == 2:
        assert np.isneginf(mx[2]).all() and np.isfinite(mx[:2]).all(), "tenant 2 owns no row of the last shard"
    if tenant == -1:
        assert np.isfinite(mx).all()
        assert exp[0][2, :2].tolist() == list(L.TIE), "the exact tie across two shards: lower id first"
        assert (np.stack([np.unique(c).size for c in mx.T]) > 1).sum() * 4 >= L.Q, "the shards' maxima differ"


def test_gamma_zero_without_a_temporal_vector(handles):
    import torch
    truth, shards = handles
    q, ptr, terms = L.query_tensors()
    w = L.world()
    try:
        for e in [truth] + shards:
            e.set_temporal(None)
        exp = one_call(truth, q, ptr, terms, K, (0.6, 0.4, 0.0))
        o, _, _ = run_shards(shards, q, ptr, terms, K, (0.6, 0.4, 0.0))
        torch.cuda.synchronize()
        L.assert_same(L.as_np(o), exp)
        assert (exp[4] == 0).all()
    finally:
        truth.set_temporal(w["temporal"])
        for e, (lo, hi) in zip(shards, L.BOUNDS):
            e.set_temporal(np.ascontiguousarray(w["temporal"][lo:hi]))


def test_local_maxima_would_not_merge_into_the_truth(handles):
    """the shards' own rag_hybrid_linear_dev results, merged: the feature's absence shows on these inputs"""
    import torch
    truth, shards = handles
    q, ptr, terms = L.query_tensors()
    exp = one_call(truth, q, ptr, terms, K, L.WEIGHTS)
    parts = [one_call(e, q, ptr, terms, K, L.WEIGHTS) for e in shards]
    got = L.merge(parts, K)
    assert any(got[0][i].tolist() != exp[0][i].tolist() for i in range(L.Q))


def test_world_one_through_the_class_equals_the_one_call_entry(handles):
    import torch
    import torch.distributed as dist
    from optimized_rag_amd.sharded import ShardedHybridIndex
    truth, _ = handles
    q, ptr, terms = L.query_tensors()
    assert not dist.is_initialized(), "world 1 needs no process group: there is no collective to make"
    ix = ShardedHybridIndex(truth, rank=0, world=1)
    for tenant in (-1, L.world()["tenant_q"]):
        exp = one_call(truth, q, ptr, terms, K, L.WEIGHTS, tenant)
        got = L.as_np(ix.search_linear(q, ptr, terms, K, *L.WEIGHTS, tenant=tenant))
        torch.cuda.synchronize()
        L.assert_same(got, exp)
    assert ix._lin_batch(q.device) == truth.hybrid_linear_batch() == 256


def test_a_batch_above_the_sub_batch_is_looped(handles):
    """sub-batch forced to 8 through the class: 28 queries in pieces of 8, 8, 8, 4 give the bits of the whole batch"""
    import torch
    from optimized_rag_amd.sharded import ShardedHybridIndex
    truth, _ = handles
    q, ptr, terms = L.query_tensors()
    ix = ShardedHybridIndex(truth, rank=0, world=1)
    ix.linear_sub_batch = 8
    for tenant in (-1, L.world()["tenant_q"]):
        exp = one_call(truth, q, ptr, terms, K, L.WEIGHTS, tenant)
        got = L.as_np(ix.search_linear(q, ptr, terms, K, *L.WEIGHTS, tenant=tenant))
        torch.cuda.synchronize()
        L.assert_same(got, exp)


def test_a_small_call_after_a_larger_one(handles):
    import torch
    truth, shards = handles
    q, ptr, terms = L.query_tensors()
    exp = one_call(truth, q, ptr, terms, K, L.WEIGHTS)
    run_shards(shards, q, ptr, terms, K, L.WEIGHTS)
    n = 5
    o, _, _ = run_shards(shards, q[:n].contiguous(), ptr[:n + 1].contiguous(), terms, 3, L.WEIGHTS)
    torch.cuda.synchronize()
    got = L.as_np(o)
    L.assert_same(got, tuple(x[:n, :3] for x in exp))


def test_merge_entry_alone(handles):
    import torch
    _, shards = handles
    rng = np.random.default_rng(3)
    world, n, k = 3, 4, 6
    ids = np.stack([rng.permutation(1000)[:n * k].reshape(n, k) + 1000 * r for r in range(world)]).astype(np.int64)
    hyb = rng.integers(0, 6, (world, n, k)) / 4.0                        # many equal scores: the id decides
    ids[0, :, 2] = -1                                                    # holes in the middle of a list
    ids[1, 1, 0] = -1
    ids[2] = -1                                                          # a rank with an all-padding block
    comp = [rng.standard_normal((world, n, k)) for _ in range(3)]
    exp = L.merge([(ids[r], hyb[r]) + tuple(c[r] for c in comp) for r in range(world)], k)
    block = np.stack([np.stack([ids[r]] + [L.bits(x[r]) for x in [hyb] + comp]) for r in range(world)])
    g = torch.from_numpy(block).cuda()
    new = lambda dt: torch.full((n, k), -7, dtype=dt, device="cuda")
    o = [new(torch.int64)] + [new(torch.float64) for _ in range(4)]
    shards[2].hybrid_linear_merge_gathered_dev(g, *o)
    torch.cuda.synchronize()
    L.assert_same(tuple(x.cpu().numpy() for x in o), exp)
    # world 1: the list itself with its holes closed; components NULL
    o1 = [new(torch.int64), new(torch.float64)]
    shards[2].hybrid_linear_merge_gathered_dev(g[:1].contiguous(), *o1)
    torch.cuda.synchronize()
    e1 = L.merge([(ids[0], hyb[0]) + tuple(c[0] for c in comp)], k)
    np.testing.assert_array_equal(o1[0].cpu().numpy(), e1[0])
    np.testing.assert_array_equal(L.bits(o1[1].cpu().numpy()), L.bits(e1[1]))
    assert (e1[0][:, k - 1] == -1).all()
    from optimized_rag_amd import RagError
    with pytest.raises(RagError, match=r"\(-1\).*4092"):
        big = torch.zeros((17, 5, 1, 256), dtype=torch.int64, device="cuda")
        shards[2].hybrid_linear_merge_gathered_dev(big, torch.empty((1, 256), dtype=torch.int64, device="cuda"),
                                                   torch.empty((1, 256), dtype=torch.float64, device="cuda"))


def test_state_and_argument_errors_leave_the_handle_usable(small):
    import torch
    from optimized_rag_amd import RagError
    lo, hi, n = 0, 600, 8
    q, ptr, terms = L.query_tensors()
    q, ptr = q[:n].contiguous(), ptr[:n + 1].contiguous()
    tq = L.world()["tenant_q"][:n].copy()
    mx = torch.empty((1, n), dtype=torch.float64, device="cuda")
    part = torch.empty((5, n, K), dtype=torch.int64, device="cuda")
    eng = small

    def pair_is_right(tenant=-1):
        exp = one_call(eng, q, ptr, terms, K, L.WEIGHTS, tenant)
        o, _, _ = run_shards([eng], q, ptr, terms, K, L.WEIGHTS, tenant)
        torch.cuda.synchronize()
        L.assert_same(L.as_np(o), exp)

    def begin(tenant=-1):
        eng.hybrid_linear_begin_dev(ptr, terms, mx[0], tenant=tenant)

    def finish_fails(code, tenant=-1, nq=n, match=""):
        with pytest.raises(RagError, match=rf"\({code}\).*{match}"):
            eng.hybrid_linear_finish_dev(q[:nq], mx[:, :nq].contiguous(), K, *L.WEIGHTS, part[:, :nq].contiguous(), tenant=tenant)

    L.load_handle(eng, lo, hi, deleted=False)
    pair_is_right()
    finish_fails(-3)                                                     # no begin (the pair before consumed its own)
    pair_is_right()
    begin()
    finish_fails(-3, nq=n - 1)                                           # another Q
    finish_fails(-3)                                                     # ... and that finish consumed the state
    pair_is_right()
    begin(tenant=1)
    finish_fails(-3, tenant=2)                                           # another tenant
    begin(tenant=tq)
    finish_fails(-3, tenant=int(tq[0]))                                  # an array begun, a scalar finished
    begin(tenant=tq)
    tq2 = tq.copy()
    tq2[3] = (tq2[3] + 2) % 3
    finish_fails(-3, tenant=tq2)
    pair_is_right(tq)
    begin()
    eng.hybrid_linear_dev(q, ptr, terms, K, *L.WEIGHTS)                  # reuses the workspace
    finish_fails(-3)
    pair_is_right()
    begin()
    eng.set_temporal(np.ascontiguousarray(L.world()["temporal"][lo:hi]))  # a host write
    finish_fails(-3)
    pair_is_right()
    begin()
    eng.index_insert(L.world()["emb"][:2], tenants=np.zeros(2, np.int32), temporal=np.zeros(2))        # a live write: the rows changed, the postings are stale
    finish_fails(-3)
    L.load_handle(eng, lo, hi, deleted=False)
    pair_is_right()
    # Q above the limit: RAG_ERR_ARG, and the message names the limit
    limit = eng.hybrid_linear_batch()
    assert limit == 256
    ptr_big = torch.zeros(limit + 2, dtype=torch.int32, device="cuda")
    with pytest.raises(RagError, match=rf"\(-1\).*{limit} queries"):
        eng.hybrid_linear_begin_dev(ptr_big, terms, torch.empty(limit + 1, dtype=torch.float64, device="cuda"))
    finish_fails(-3)
    # weights are checked as rag_hybrid_linear_dev checks them
    begin()
    with pytest.raises(RagError, match=r"\(-1\).*alpha"):
        eng.hybrid_linear_finish_dev(q, mx, K, 0.0, 0.3, 0.1, part)
    pair_is_right()
    # explicit ids: the order across shards is defined through id_base
    eng.set_ids(np.arange(hi - lo, dtype=np.int64) * 3)
    with pytest.raises(RagError, match=r"\(-3\).*explicit ids"):
        begin()
    L.load_handle(eng, lo, hi, deleted=False)
    pair_is_right()


def test_begin_finish_and_merge_are_ordered_on_the_callers_stream(handles):
    """tests/stream_tools.py on a side stream: busy work, the inputs copied in behind it, the three calls, a clone of the outputs -
    equal to the same calls made alone, and the calls return while the stream is still busy."""
    import torch
    _, shards = handles
    w = L.world()
    real = dict(q=w["q_emb"], ptr=w["ptr"], terms=w["terms"])
    wrong = dict(q=np.zeros((L.Q, L.D), np.float32), ptr=np.zeros(L.Q + 1, np.int32), terms=np.full(len(w["terms"]), -1, np.int32))

    def call(d, s):
        o, mx, parts = run_shards(shards, d["q"], d["ptr"], d["terms"], K, L.WEIGHTS, w["tenant_q"], stream=s)
        return [o[n] for n in L.NAMES] + [mx, parts]

    ref = T.serial(call, wrong, real)
    got, pending = T.late_producer(call, wrong, real, torch.cuda.Stream())
    T.assert_same(got, ref, "linear fusion over shards")
    assert pending, "begin / finish / merge waited for the work queued before them on their stream"
