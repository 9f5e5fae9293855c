#!/usr/bin/env python3
"""Agents mixed in one batch (rag_*_tenants_*) on a 1M x 1536 index with 256 tenants: 256 queries, one per tenant, k = 100.
Per layout - tenants interleaved row by row, tenants stored contiguously - three device-synchronised p50 wall times of
  * the per-query-tenant call (one call, a tenant array);
  * the loop of 256 scalar-tenant calls of one query each: what a multi-agent host had before;
  * the unfiltered call of the same 256 queries (the floor: the same pass without a filter, and the WRONG answer);
for rag_dense_topk_*_dev (k = 100) and rag_hybrid_rrf_*_dev (pool 100, k 20) over synthetic postings (bench_modes.synthetic_csr:
Poisson(60) tokens per document, Zipf(1.1) over 100,000 terms). A third shape on the contiguous layout draws the 256 queries from
16 tenants only: the union of their tile lists is shorter than the table, so the dense pass walks it instead of every tile.
The per-query results are checked against the loop's, bit for bit, before anything is timed.
Writes profiles/multi_tenant_1M.json.  python tools/multi_tenant_probe.py [--rows N] [--out PATH]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_tenant_1M.json"))
    a = ap.parse_args()
    import torch
    import bench_modes as BM
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.bm25 import Bm25Postings
    N, D, Q, K, T, POOL, KH = a.rows, a.dim, 256, 100, 256, 100, 20
    rng = np.random.default_rng(5)
    layouts = {"interleaved": (np.arange(N) % T).astype(np.int32), "contiguous": (np.arange(N) * T // N).astype(np.int32)}
    indptr, doc, tf, dl, tok, doc_ptr = BM.synthetic_csr(N, 100_000, 60)
    idf = Bm25Postings.idf_table(np.diff(indptr), N)
    idf[np.diff(indptr) == 0] = 0.0
    ptr, terms = BM._term_queries(tok, doc_ptr, N, Q)
    pd, td = torch.from_numpy(ptr).cuda(), torch.from_numpy(terms).cuda()
    one = [(torch.from_numpy(np.array([0, ptr[i + 1] - ptr[i]], np.int32)).cuda(), torch.from_numpy(terms[ptr[i]:ptr[i + 1]].copy()).cuda())
           for i in range(Q)]
    eng = RagEngine(dim=D, device=0)
    eng.index_reserve(N)
    gen = torch.Generator(device="cuda").manual_seed(11)
    q_rows = np.sort(rng.integers(0, N, Q))                                # every query is planted next to one row
    q = torch.empty((Q, D), dtype=torch.float32, device="cuda")
    step = 125_000
    for b in range(0, N, step):
        blk = torch.randn((min(step, N - b), D), generator=gen, device="cuda", dtype=torch.float32)
        for i in np.nonzero((q_rows >= b) & (q_rows < b + step))[0]:
            q[i] = blk[q_rows[i] - b] + 0.5 * torch.randn((D,), generator=gen, device="cuda")
        eng.index_append(blk)
    del blk
    eng.bm25_load(indptr, doc, tf, dl, idf, float(dl.sum()) / N)
    ids, sc = torch.empty((Q, K), dtype=torch.int64, device="cuda"), torch.empty((Q, K), dtype=torch.float64, device="cuda")
    ids1, sc1 = torch.empty((1, K), dtype=torch.int64, device="cuda"), torch.empty((1, K), dtype=torch.float64, device="cuda")
    out = {"rows": N, "dim": D, "queries": Q, "tenants": T, "k": K, "hybrid": {"pool": POOL, "k": KH},
           "note": "p50 wall ms, device-synchronised; loop = 256 scalar-tenant calls of one query each", "layouts": {}}

    def measure(tq):
        def dense_loop():
            for i in range(Q):
                eng.dense_topk_dev(q[i:i + 1], K, ids1, None, sc1, tenant=int(tq[i]))

        def hybrid_loop():
            for i in range(Q):
                eng.hybrid_rrf_dev(q[i:i + 1], one[i][0], one[i][1], POOL, KH, tenant=int(tq[i]))
        # the one call equals the loop, bit for bit
        eng.dense_topk_dev(q, K, ids, None, sc, tenant=tq)
        torch.cuda.synchronize()
        got = (ids.cpu().numpy().copy(), sc.cpu().numpy().copy())
        keys = eng.hybrid_rrf_dev(q, pd, td, POOL, KH, tenant=tq)[0].cpu().numpy().copy()
        for i in range(0, Q, 17):
            eng.dense_topk_dev(q[i:i + 1], K, ids1, None, sc1, tenant=int(tq[i]))
            torch.cuda.synchronize()
            assert (ids1.cpu().numpy()[0] == got[0][i]).all() and (sc1.cpu().numpy()[0].view(np.int64) == got[1][i].view(np.int64)).all()
            k1 = eng.hybrid_rrf_dev(q[i:i + 1], one[i][0], one[i][1], POOL, KH, tenant=int(tq[i]))[0].cpu().numpy()
            assert (k1[0] == keys[i]).all()
        r = {"dense": {"per_query_tenants_ms": BM._p50_ms(lambda: eng.dense_topk_dev(q, K, ids, None, sc, tenant=tq), 10, 3),
                       "loop_of_scalar_calls_ms": BM._p50_ms(dense_loop, 3, 1),
                       "unfiltered_ms": BM._p50_ms(lambda: eng.dense_topk_dev(q, K, ids, None, sc), 10, 3)},
             "hybrid_rrf": {"per_query_tenants_ms": BM._p50_ms(lambda: eng.hybrid_rrf_dev(q, pd, td, POOL, KH, tenant=tq), 10, 3),
                            "loop_of_scalar_calls_ms": BM._p50_ms(hybrid_loop, 3, 1),
                            "unfiltered_ms": BM._p50_ms(lambda: eng.hybrid_rrf_dev(q, pd, td, POOL, KH), 10, 3)}}
        for v in r.values():
            v["loop_over_one_call"] = v["loop_of_scalar_calls_ms"] / v["per_query_tenants_ms"]
        return r

    for name, ten in layouts.items():
        eng.set_tenants(ten)
        tq = ten[q_rows].copy()                                            # each query under the tenant of its planted row
        out["layouts"][name] = measure(tq)
        print(name, json.dumps(out["layouts"][name]), flush=True)
        if name == "contiguous":
            few = (ten[q_rows] % 16 * 16).astype(np.int32)                 # 16 tenants, 16 queries each: a union of ~270 tiles
            out["layouts"]["contiguous_16_of_256_tenants"] = measure(few)
            print("contiguous_16_of_256_tenants", json.dumps(out["layouts"]["contiguous_16_of_256_tenants"]), flush=True)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
