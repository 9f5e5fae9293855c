"""GPU: sharded.ShardedM3Index with the REAL library in TWO processes (the shape of tests/test_sharded_two_ranks_gpu.py: the
development boxes have one GPU, so both ranks open their own handle on cuda:0 and exchange through gloo; an 8-GPU node runs the
same class over RCCL). Every rank must end with exactly what the one-call entries return on the unsharded index - the three-way
search in its three modes (ids, float64 score bits, component bits, candidate lists), the late-interaction rerank, the sparse list -
and with what rank 0 holds. The parent joins the children under a deadline and ends them when it passes: a stalled gather fails."""
import os
import socket
import time

import numpy as np
import pytest

import m3_fused_tools as F

pytestmark = pytest.mark.gpu

N, POOL, K = F.N_A, F.POOL, 10
DEADLINE_S = 120


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
        from optimized_rag_amd.sharded import ShardedM3Index, shard_bounds
        from optimized_rag_amd.sparse import LexicalPostings
        w, a = F.world(), F.corpus_a()
        emb = np.array(w["emb"])
        emb[7] = emb[N - 9]                                              # an exact dense tie across the two shards
        q_emb = np.array(w["q_emb"])
        q_emb[0] = emb[7]
        post = LexicalPostings(np.array(a["indptr"]), np.array(a["doc"]), np.array(a["w"]), N)
        dev = torch.device("cuda", 0)
        cuda = lambda x: torch.from_numpy(np.array(x)).to(dev)
        ptr, terms, wts = (cuda(x) for x in a["packed"])
        q, qv, qo = cuda(q_emb), cuda(w["qv"]), cuda(w["qo"])

        def load(ix, lo, hi):
            off = (w["d_off"][lo:hi + 1] - w["d_off"][lo]).astype(np.int64)
            ix.load_shard(emb[lo:hi], lo, post.shard(lo, hi), np.array(w["d_vecs"][w["d_off"][lo]:w["d_off"][hi]]), off)

        b, e = shard_bounds(N, world)[rank]
        eng = RagEngine(dim=F.DIM, device=0)
        ix = ShardedM3Index(eng, rank=rank, world=world)
        load(ix, b, e)
        got = {}
        for mode in (0, 1, 2):
            r = ix.search_m3(q, ptr, terms, wts, qv, qo, POOL, K, mode=mode)
            torch.cuda.synchronize()
            got[mode] = {n: v.cpu().clone() for n, v in r.items()}
        r = ix.search_late_interaction(q, qv, qo, POOL, K, term_ptr=ptr, terms=terms, weights=wts)
        torch.cuda.synchronize()
        got["late"] = {n: v.cpu().clone() for n, v in r.items()}
        l_ids, l_sc = ix.search_lexical(ptr, terms, wts, K)
        torch.cuda.synchronize()
        got["lex"] = dict(ids=l_ids.cpu().clone(), scores=l_sc.cpu().clone())
        ok = True
        if rank == 0:                                                    # the unsharded truth, same library, one-call entries
            whole = RagEngine(dim=F.DIM, device=0)
            load(ShardedM3Index(whole, rank=0, world=1), 0, N)
            for mode in (0, 1, 2):
                ids, sc, comp, cand = whole.retrieve_m3_dev(q, POOL, K, term_ptr=ptr, terms=terms, weights=wts, q_vecs=qv, q_off=qo, mode=mode)
                torch.cuda.synchronize()
                g = got[mode]
                ok &= torch.equal(g["ids"], ids.cpu()) and torch.equal(g["candidates"], cand.cpu())
                ok &= torch.equal(g["scores"].view(torch.int64), sc.cpu().view(torch.int64))
                ok &= torch.equal(g["components"].view(torch.int64), comp.cpu().view(torch.int64))
                ok &= bool((ids[:, 0] >= 0).all())
            ok &= got[0]["candidates"][0, :2].tolist() == [7, N - 9]         # the tie: lower id first, one from each shard
            ids, sc, cand = whole.retrieve_maxsim_dev(q, qv, qo, POOL, K, term_ptr=ptr, terms=terms, weights=wts)
            torch.cuda.synchronize()
            g = got["late"]
            ok &= torch.equal(g["ids"], ids.cpu()) and torch.equal(g["candidates"], cand.cpu())
            ok &= torch.equal(g["scores"].view(torch.int64), sc.cpu().view(torch.int64))
            si = torch.empty((32, K), dtype=torch.int64, device=dev)
            ss = torch.empty((32, K), dtype=torch.float64, device=dev)
            whole.sparse_topk_dev(ptr, terms, wts, K, si, None, ss)
            torch.cuda.synchronize()
            ok &= torch.equal(got["lex"]["ids"], si.cpu()) and torch.equal(got["lex"]["scores"].view(torch.int64), ss.cpu().view(torch.int64))
            whole.close()
        # every rank holds the same result: compare with rank 0's
        for key in (0, 1, 2, "late", "lex"):
            for name in ("ids", "candidates"):
                if name in got[key]:
                    ref = got[key][name].clone()
                    dist.broadcast(ref, src=0)
                    ok &= torch.equal(ref, got[key][name])
        ret[rank] = bool(ok)
        eng.close()
    finally:
        dist.destroy_process_group()


def test_two_processes_on_one_gpu_equal_the_unsharded_entries():
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
