"""GPU: the writes of sharded.py with the REAL collectives, in TWO processes (the shape of tests/test_m3_sharded_two_ranks_gpu.py:
both ranks open their own handle on cuda:0 and exchange through gloo). The sequence of tests/test_sharded_writes_gpu.py in short
form - explicit ids, two inserts with two owners, deletes on both shards, compact, a third insert onto a compacted shard,
refresh_statistics (BM25 world) - through the
SPMD calls themselves: every rank makes the same call with the same arguments. Both ranks must end with the bits of the one-call
entries on one unsharded handle that received the same writes. The parent joins the children under a deadline."""
import os
import socket
import sys
import time

import numpy as np
import pytest

import linear_sharded_tools as L
import m3_fused_tools as F

pytestmark = pytest.mark.gpu

K, POOL = L.K, 30
DEADLINE_S = 150
BLOCKS = (300, 120, 40)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def gid(rows):
    return 7 + 3 * np.asarray(rows, dtype=np.int64)


def _rank(rank, world, port, ret):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from optimized_rag_amd import RagEngine
        from optimized_rag_amd.bm25 import Bm25Postings
        from optimized_rag_amd.sharded import ShardedHybridIndex, ShardedM3Index, shard_bounds
        from optimized_rag_amd.sparse import LexicalPostings
        dev = torch.device("cuda", 0)
        cuda = lambda x: torch.from_numpy(np.array(x)).to(dev)
        eq = lambda a, b: torch.equal(a.cpu().view(torch.int64) if a.dtype == torch.float64 else a.cpu(),
                                      b.cpu().view(torch.int64) if b.dtype == torch.float64 else b.cpu())
        ok, bad = True, []

        def need(cond, what):
            """the checks that did not hold are reported by name"""
            if not cond:
                bad.append(f"line {sys._getframe(1).f_lineno}: {what}")
            return bool(cond)

        # ---- dense + BM25 + temporal: search, search_hybrid, search_linear ---------------------------------------------------
        w = L.world()
        rng = np.random.default_rng(5)
        mirror = Bm25Postings(w["indptr"].copy(), w["doc"].copy(), w["tf"].copy(), w["doc_len"].copy(), w["idf"].copy(), w["avgdl"],
                              vocab={f"w{t}": t for t in range(L.N_TERMS)})
        n_new = sum(BLOCKS)
        new_emb = (w["emb"][rng.integers(0, L.N, n_new)] + 0.5 * rng.standard_normal((n_new, L.D))).astype(np.float32)
        new_ten = rng.integers(0, 3, n_new).astype(np.int32)
        new_tmp = 0.1 * rng.uniform(size=n_new)
        texts = [" ".join([f"w{int(t)}" for t in rng.integers(0, L.N_TERMS, 4)] + [f"n{int(rng.integers(0, 6))}"]) for _ in range(n_new)]
        texts[0] = "n0 n1 n2 n3 n4 n5 " + texts[0]                                   # terms 300 .. 305, introduced by the first block
        terms_of = list(w["terms_of"]) + [[300, 7], [303], [305, -1]]
        ptr = cuda(np.cumsum([0] + [len(t) for t in terms_of]).astype(np.int32))
        terms = cuda(np.asarray([x for t in terms_of for x in t], np.int32))
        q = cuda(np.concatenate([w["q_emb"], new_emb[[3, BLOCKS[0] + 5, 11]]]).astype(np.float32))
        tenant_q = np.concatenate([w["tenant_q"], [-1, 1, 0]]).astype(np.int32)
        lo, hi = shard_bounds(L.N, world)[rank]
        eng = RagEngine(dim=L.D, device=0)
        eng.set_option("bm25_keep_tf", 1)
        ix = ShardedHybridIndex(eng, rank=rank, world=world)
        ix.load_shard(np.ascontiguousarray(w["emb"][lo:hi]), lo, mirror.shard(lo, hi), temporal=np.ascontiguousarray(w["temporal"][lo:hi]),
                      ids=gid(np.arange(lo, hi)))
        eng.set_tenants(np.ascontiguousarray(w["tenants"][lo:hi]))
        whole = None
        if rank == 0:
            whole = RagEngine(dim=L.D, device=0)
            whole.set_option("bm25_keep_tf", 1)
            whole.index_load(np.ascontiguousarray(w["emb"]), ids=gid(np.arange(L.N)))
            mirror.load(whole)
            whole.set_temporal(w["temporal"])
            whole.set_tenants(w["tenants"])

        def check():
            good = True
            for tenant in (-1, tenant_q):
                ids, sc = ix.search(q, K, tenant=tenant)
                hyb = ix.search_hybrid(q, ptr, terms, POOL, K, tenant=tenant)
                lin = ix.search_linear(q, ptr, terms, K, *L.WEIGHTS, tenant=tenant)
                torch.cuda.synchronize()
                mine = [ids, sc, hyb["keys"], hyb["rrf"], hyb["ranks"]] + [lin[n] for n in L.NAMES]
                if rank == 0:
                    e_ids = torch.empty_like(ids)
                    e_sc = torch.empty_like(sc)
                    whole.dense_topk_dev(q, K, e_ids, None, e_sc, tenant=tenant)
                    keys, rrf, ranks = whole.hybrid_rrf_dev(q, ptr, terms, POOL, K, tenant=tenant)
                    e_lin = whole.hybrid_linear_dev(q, ptr, terms, K, *L.WEIGHTS, tenant=tenant)
                    torch.cuda.synchronize()
                    for g, e in zip(mine, [e_ids, e_sc, keys, rrf, ranks] + [e_lin[n] for n in L.NAMES]):
                        good &= eq(g, e)
                for g in mine:                                                      # both ranks hold rank 0's result
                    ref = g.cpu().clone()
                    dist.broadcast(ref, src=0)
                    good &= torch.equal(ref.view(torch.int64) if ref.dtype == torch.float64 else ref, g.cpu().view(torch.int64) if g.dtype == torch.float64 else g.cpu())
            return good

        ok &= need(check(), "check()")
        at, row, owners = 0, L.N, []
        for b in range(2):
            n = BLOCKS[b]
            block = mirror.extend(texts[at:at + n])
            args = (new_emb[at:at + n], gid(np.arange(row, row + n)))
            kw = dict(tenants=new_ten[at:at + n], temporal=new_tmp[at:at + n])
            owner, first = ix.insert_rows(*args, postings=block, **kw)
            owners.append(owner)
            if rank == 0:
                whole.index_insert(*args, **kw)
                whole.bm25_append(block["indptr"], block["doc"], block["tf"], block["doc_len"], block["idf_new"], block["n_terms_total"])
            at, row = at + n, row + n
            ok &= need(check(), "check()")
        ok &= need(owners == [0, 1], "owners == [0, 1]")  # equal shards: the tie goes to rank 0, then rank 1 is shorter
        victims = np.concatenate([gid([3, 1000, 2299, 2300, 4000, L.N + 7, L.N + 350]), gid(np.arange(500, 700)), [5, -1]])
        n_del = ix.delete_ids(victims)
        ok &= need(n_del == len(victims) - 2, "n_del == len(victims) - 2")
        if rank == 0:
            ok &= need(whole.index_delete(victims) == n_del, "whole.index_delete(victims) == n_del")
        ok &= need(check(), "check()")
        row_map = ix.compact()
        ok &= need(int((row_map < 0).sum()) == (204 if rank == 0 else 3), "int((row_map < 0).sum()) == (204 if rank == 0 else 3)")
        ok &= need(ix.layout()["rows"] == [2300 + BLOCKS[0] - 204, 2300 + BLOCKS[1] - 3], "ix.layout()['rows'] == [2300 + BLOCKS[0] - 204, 2300 + BLOCKS[1] - 3]")
        ok &= need(check(), "check()")
        n = BLOCKS[2]
        block = mirror.extend(texts[at:at + n])
        args = (new_emb[at:at + n], gid(np.arange(row, row + n)))
        kw = dict(tenants=new_ten[at:at + n], temporal=new_tmp[at:at + n])
        owner, _ = ix.insert_rows(*args, postings=block, **kw)
        ok &= need(owner == 0, "owner == 0")  # 2396 rows against 2417
        if rank == 0:
            whole.index_insert(*args, **kw)
            whole.bm25_append(block["indptr"], block["doc"], block["tf"], block["doc_len"], block["idf_new"], block["n_terms_total"])
        ok &= need(check(), "check()")
        idf, avgdl = ix.refresh_statistics()
        if rank == 0:
            e_idf, info = whole.bm25_refresh(0.25)
            ok &= need(np.array_equal(idf.view(np.int64), e_idf.view(np.int64)) and avgdl == info["avgdl_after"], "np.array_equal(idf.view(np.int64), e_idf.view(np.int64)) and avgdl == ")
        ok &= need(check(), "check()")
        try:                                                                        # refused on every rank alike, nothing changed
            ix.insert_rows(new_emb[:1], [7], tenants=[0], temporal=[0.0], postings=None)
            ok = False
        except ValueError:
            pass
        ok &= need(check(), "check()")
        eng.close()
        if whole is not None:
            whole.close()

        # ---- bge-m3: search_m3 (the union mode), search_lexical: two inserts with two owners, deletes, compact, a third insert
        # (a device block) onto a compacted shard
        mw, a = F.world(), F.corpus_a()
        N0 = 6000
        MB = ((N0, N0 + 400), (N0 + 400, N0 + 700), (N0 + 700, N0 + 800))
        N1 = MB[-1][1]
        emb = np.array(mw["emb"])
        mptr, mterms, mwts = (cuda(x) for x in a["packed"])
        mq, qv, qo = cuda(mw["q_emb"]), cuda(mw["qv"]), cuda(mw["qo"])

        def lexical(rows):
            ip, doc, wt = F.csr_of_rows(np.asarray(rows))
            return LexicalPostings(ip, doc, wt, len(rows))

        def vecs(b, e):
            return np.array(mw["d_vecs"][mw["d_off"][b]:mw["d_off"][e]]), (mw["d_off"][b:e + 1] - mw["d_off"][b]).astype(np.int64)

        spare = (N1 - N0, int(mw["d_off"][N1] - mw["d_off"][N0]))
        lo, hi = ((0, 3100), (3100, N0))[rank]
        eng = RagEngine(dim=F.DIM, device=0)
        mx = ShardedM3Index(eng, rank=rank, world=world)
        mx.load_shard(emb[lo:hi], lo, lexical(np.arange(lo, hi)), *vecs(lo, hi), ids=gid(np.arange(lo, hi)), token_reserve=spare)
        whole = None
        if rank == 0:
            whole = RagEngine(dim=F.DIM, device=0)
            ShardedM3Index(whole, rank=0, world=1).load_shard(emb[:N0], 0, lexical(np.arange(N0)), *vecs(0, N0), ids=gid(np.arange(N0)),
                                                             token_reserve=spare)

        def check_m3():
            good = True
            r = mx.search_m3(mq, mptr, mterms, mwts, qv, qo, POOL, K, mode=2)
            l_ids, l_sc = mx.search_lexical(mptr, mterms, mwts, K)
            torch.cuda.synchronize()
            mine = [r["ids"], r["scores"], r["components"], r["candidates"], l_ids, l_sc]
            if rank == 0:
                exp = list(whole.retrieve_m3_dev(mq, POOL, K, term_ptr=mptr, terms=mterms, weights=mwts, q_vecs=qv, q_off=qo, mode=2))
                si = torch.empty_like(l_ids)
                ss = torch.empty_like(l_sc)
                whole.sparse_topk_dev(mptr, mterms, mwts, K, si, None, ss)
                torch.cuda.synchronize()
                for g, e in zip(mine, exp + [si, ss]):
                    good &= eq(g, e)
            for g in mine:                                                          # both ranks hold rank 0's bits, the float64 planes too
                mine_bits = g.cpu().view(torch.int64) if g.dtype == torch.float64 else g.cpu()
                ref = mine_bits.clone()
                dist.broadcast(ref, src=0)
                good &= torch.equal(ref, mine_bits)
            return good

        def insert_m3(b, device=False):
            b0, b1 = MB[b]
            rows = np.arange(b0, b1)
            blk = lexical(rows)
            lex = dict(indptr=blk.indptr, doc=blk.doc, weight=blk.weight, n_docs=b1 - b0, n_terms_total=F.V_A)
            given = lex
            if device:                                                              # doc-major CUDA tensors: rag_sparse_append_dev
                term_of = np.repeat(np.arange(F.V_A, dtype=np.int64), np.diff(blk.indptr))
                order = np.lexsort((term_of, blk.doc))
                dptr = np.zeros(b1 - b0 + 1, dtype=np.int64)
                np.cumsum(np.bincount(blk.doc, minlength=b1 - b0), out=dptr[1:])
                given = (cuda(dptr.astype(np.int32)), cuda(term_of[order].astype(np.int32)), cuda(blk.weight[order]), F.V_A)
            tv, off = vecs(b0, b1)
            got = mx.insert_rows(emb[b0:b1], gid(rows), lexical=given, token_vecs=tv, token_off=off)
            if rank == 0:
                whole.index_insert(emb[b0:b1], ids=gid(rows))
                whole.sparse_append(lex["indptr"], lex["doc"], lex["weight"], b1 - b0, F.V_A)
                whole.tokvec_append(tv, off)
            return got

        ok &= need(check_m3(), "check_m3()")
        ok &= need(insert_m3(0) == (1, 2900), "insert_m3(0) == (1, 2900)")  # 3100 rows against 2900
        ok &= need(check_m3(), "check_m3()")
        ok &= need(insert_m3(1) == (0, 3100), "insert_m3(1) == (0, 3100)")  # 3100 against 3300
        ok &= need(check_m3(), "check_m3()")
        head = int(mx.search_lexical(mptr, mterms, mwts, K)[0][4, 0])
        victims = np.unique(np.concatenate([gid([0, 3099, 3100, N0 + 3, N0 + 450]), gid(np.arange(1000, 1200)), [head]]))
        n_del = mx.delete_ids(victims)
        ok &= need(n_del == len(victims), "n_del == len(victims)")
        if rank == 0:
            ok &= need(whole.index_delete(victims) == n_del, "whole.index_delete(victims) == n_del")
        ok &= need(check_m3(), "check_m3()")
        row_map = mx.compact()
        ok &= need(int((row_map < 0).sum()) >= (203 if rank == 0 else 2), "int((row_map < 0).sum()) >= (203 if rank == 0 else 2)")
        rows_now = list(mx.layout()["rows"])                              # (a copy: the class updates its own)
        ok &= need(sum(rows_now) == N0 + 700 - len(victims) and rows_now[0] < rows_now[1], "sum(rows_now) == N0 + 700 - len(victims) and rows_now[0] < rows_now[1]")
        ok &= need(check_m3(), "check_m3()")
        owner, first = insert_m3(2, device=True)                                    # onto rank 0, which the compaction just renumbered
        ok &= need((owner, first) == (0, rows_now[0]), "(owner, first) == (0, rows_now[0])")
        if rank == 0:
            ok &= need(bool((eng.rows_of_ids(gid(np.arange(*MB[2]))) == first + np.arange(100)).all()), "bool((eng.rows_of_ids(gid(np.arange(*MB[2]))) == first + np.arange(100")
        else:
            ok &= need(bool((eng.rows_of_ids(gid(np.arange(*MB[2]))) < 0).all()), "bool((eng.rows_of_ids(gid(np.arange(*MB[2]))) < 0).all())")
        ok &= need(check_m3(), "check_m3()")
        ret[rank] = list(bad) if not ok else []
        eng.close()
        if whole is not None:
            whole.close()
    finally:
        dist.destroy_process_group()


def test_two_processes_write_and_search_like_one_unsharded_handle():
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
    assert dict(ret) == {0: [], 1: []}
