"""GPU: ShardedHybridIndex.search_linear with the REAL library in TWO processes (the shape of
tests/test_m3_sharded_two_ranks_gpu.py: the development boxes have one GPU, so both ranks open their own handle on cuda:0 and
exchange through gloo; an 8-GPU node runs the same class over RCCL). Every rank must end with exactly what rag_hybrid_linear_dev /
_tenants_dev return on the unsharded index - ids, hybrid bits, the three component planes - and with what rank 0 holds. The
second pass forces a sub-batch of 12, so 28 queries take three begin / finish pairs and six gathers. The parent joins the
children under a deadline and ends them when it passes: a stalled gather fails."""
import os
import socket
import time

import numpy as np
import pytest

import linear_sharded_tools as L

pytestmark = pytest.mark.gpu

DEADLINE_S = 120
CUT = 2100                                                               # rank 0: [0, 2100), rank 1: [2100, 4600)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, ret):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from optimized_rag_amd import RagEngine
        from optimized_rag_amd.sharded import ShardedHybridIndex
        w = L.world()
        q, ptr, terms = L.query_tensors(torch.device("cuda", 0))
        lo, hi = ((0, CUT), (CUT, L.N))[rank]
        eng = RagEngine(dim=L.D, device=0)
        ix = ShardedHybridIndex(eng, rank=rank, world=world)
        L.load_handle(eng, lo, hi, sharded=ix)
        cases = [("scalar", L.WEIGHTS, -1, None), ("tenant", L.WEIGHTS, 1, None), ("per query", (0.5, -0.3, -0.2), w["tenant_q"], None),
                 ("pieces", L.WEIGHTS, w["tenant_q"], 12)]
        got = {}
        for name, weights, tenant, step in cases:
            ix.linear_sub_batch = step
            r = ix.search_linear(q, ptr, terms, L.K, *weights, tenant=tenant)
            torch.cuda.synchronize()
            got[name] = L.as_np(r)
        ok = ix._lin_agreed == 256
        if rank == 0:                                                    # the unsharded truth, same library, the one-call entries
            whole = L.load_handle(RagEngine(dim=L.D, device=0), 0, L.N)
            for name, weights, tenant, _ in cases:
                exp = L.as_np(whole.hybrid_linear_dev(q, ptr, terms, L.K, *weights, tenant=tenant))
                torch.cuda.synchronize()
                ok &= np.array_equal(got[name][0], exp[0]) and all(np.array_equal(L.bits(g), L.bits(e)) for g, e in zip(got[name][1:], exp[1:]))
                ok &= bool((exp[0][:, 0] >= 0).all())
            ok &= got["scalar"][0][2, :2].tolist() == list(L.TIE)            # the tie: lower id first, one row from each rank
            whole.close()
        # every rank holds the same result: compare with rank 0's
        for name in got:
            for i, a in enumerate(got[name]):
                ref = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy())
                dist.broadcast(ref, src=0)
                ok &= np.array_equal(ref.numpy(), np.ascontiguousarray(a).view(np.int64))
        ret[rank] = bool(ok)
        eng.close()
    finally:
        dist.destroy_process_group()


def test_two_processes_on_one_gpu_equal_the_unsharded_entry():
    import torch.multiprocessing as mp
    world = 2
    mgr = mp.Manager()
    ret = mgr.dict()
    ctx = mp.spawn(_rank, args=(world, _free_port(), ret), nprocs=world, join=False)
    end = time.monotonic() + DEADLINE_S
    done = False
    try:
        while not done and time.monotonic() < end:
            done = ctx.join(timeout=max(0.1, min(5.0, end - time.monotonic())))
    finally:
        if not done:
            for p in ctx.processes:
                if p.is_alive():
                    p.terminate()
            for p in ctx.processes:
                p.join(10)
                if p.is_alive():
                    p.kill()
    assert done, f"the ranks did not finish within {DEADLINE_S} s (a stalled gather?)"
    assert dict(ret) == {0: True, 1: True}
