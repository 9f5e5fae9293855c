"""Times the three-way bge-m3 score over resident data against the MaxSim composite it extends, on one MI355X; writes
profiles/m3_fused.json.

Shape: 256 queries x pool 100 over 25,600 documents: a 1024-d dense index, learned-sparse postings (30,000 terms, 64 per document,
Zipf-drawn), 255 token vectors per document at token dim 1024 and 128; a query has 32 token vectors and 32 weighted terms. Per
token dim, in ONE process, alternating round by round:
  rag_retrieve_m3_dev mode 1     dense + sparse RRF top-100 -> dense + sparse + MaxSim score -> top-20
  rag_retrieve_m3_dev mode 2     the union of the dense and the sparse top-100 (200 slots) -> the same
  rag_retrieve_maxsim_dev mode 1 the unchanged yardstick: the same candidates as mode 1, MaxSim alone
  rag_sparse_score_rows_dev      the point lookup alone over [256][100] rows
and, for the attribution of the added time, rag_m3_score_rows_dev over the same fixed rows with the dense weight alone, the sparse
weight alone and all three, beside rag_tokvec_rerank_dev on those rows.
Reported: the medians, the added time of mode 1 over the yardstick (same candidates, same MaxSim launch: what the cosines, the point
lookups and the combine cost), and the point kernel's (slot, token) lookups per second.

Method (as tools/tokvec_time.py): device-pointer entries on resident arrays, device events around `reps` back-to-back calls, one
discarded round, then `--rounds` timed ones; per arm the median over rounds with the fastest and slowest beside it. Needs a GPU.

    python tools/m3_fused_time.py [--rounds 5] [--out profiles/m3_fused.json] [--dims 1024,128]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn, reps):
    """fn() `reps` times between two device events -> ms per call"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def summary(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), rounds_ms=v)


def postings(rng, n_docs, n_terms, per_doc):
    """term-major CSR (indptr int64, doc int32, weight float32): per_doc distinct Zipf-drawn terms per document"""
    p = np.arange(1, n_terms + 1, dtype=np.float64) ** -1.1
    p /= p.sum()
    owner = np.repeat(np.arange(n_docs, dtype=np.int64), per_doc)
    term = rng.choice(n_terms, size=owner.shape[0], p=p).astype(np.int64)
    key = np.unique(term * n_docs + owner)
    term, doc = key // n_docs, (key % n_docs).astype(np.int32)
    w = (rng.random(key.shape[0]) * 2.0).astype(np.float32) + np.float32(1e-3)
    indptr = np.zeros(n_terms + 1, dtype=np.int64)
    np.cumsum(np.bincount(term, minlength=n_terms), out=indptr[1:])
    return indptr, doc, w, p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dims", default="1024,128")
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--pool", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "m3_fused.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("m3_fused_time: needs a GPU")
    from optimized_rag_amd import RagEngine
    nq, pool, qr, dr, k, q_terms, dim, n_terms = args.queries, args.pool, 32, 255, 20, 32, 1024, 30_000
    n_docs = nq * pool
    res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds)
    rng = np.random.default_rng(0)
    eng = RagEngine(dim=dim, device=0)
    unit = lambda t: torch.nn.functional.normalize(t, dim=-1)
    torch.manual_seed(0)
    emb = torch.randn((n_docs, dim))
    eng.index_load(emb.numpy())
    q_emb = (emb[torch.randint(0, n_docs, (nq,))] + 0.7 * torch.randn((nq, dim))).cuda().contiguous()
    indptr, doc, w, p = postings(rng, n_docs, n_terms, 64)
    eng.sparse_load(indptr, doc, w, n_docs)
    ptr = torch.arange(nq + 1, dtype=torch.int32, device="cuda") * q_terms
    terms = torch.from_numpy(np.concatenate([rng.choice(n_terms, q_terms, replace=False, p=p) for _ in range(nq)]).astype(np.int32)).cuda()
    qw = torch.from_numpy((rng.random(nq * q_terms) * 2.0).astype(np.float32) + np.float32(1e-3)).cuda()
    sparse = dict(term_ptr=ptr, terms=terms, weights=qw)
    rows = torch.from_numpy(rng.integers(0, n_docs, (nq, pool)).astype(np.int32)).cuda()
    pt = torch.empty((nq, pool), dtype=torch.float64, device="cuda")
    point = lambda: eng.sparse_score_rows_dev(ptr, terms, qw, rows, pt)
    ids_o, sc_o = torch.empty((nq, k), dtype=torch.int64, device="cuda"), torch.empty((nq, k), dtype=torch.float64, device="cuda")
    for tdim in [int(x) for x in args.dims.split(",")]:
        torch.manual_seed(tdim)
        qv = unit(torch.randn((nq * qr, tdim), device="cuda"))
        qo = torch.arange(nq + 1, dtype=torch.int64, device="cuda") * qr
        eng.tokvec_reserve(n_docs, n_docs * dr, tdim)
        block = 256
        off = torch.arange(block + 1, dtype=torch.int64, device="cuda") * dr
        for b in range(0, n_docs, block):
            m = min(block, n_docs - b)
            eng.tokvec_append_dev(unit(torch.randn((m * dr, tdim), device="cuda")), off[:m + 1].contiguous())
        arms = {"retrieve_m3_dev_mode1": lambda: eng.retrieve_m3_dev(q_emb, pool, k, q_vecs=qv, q_off=qo, mode=1, **sparse),
                "retrieve_m3_dev_mode2": lambda: eng.retrieve_m3_dev(q_emb, pool, k, q_vecs=qv, q_off=qo, mode=2, **sparse),
                "retrieve_maxsim_dev_mode1": lambda: eng.retrieve_maxsim_dev(q_emb, qv, qo, pool, k, **sparse),
                "sparse_score_rows_dev": point,
                # attribution of the added time, on the fixed [256][100] rows: one component each (with the combine + select), then
                # all three beside the MaxSim rerank of the same rows
                "m3_score_rows_dev_dense_only": lambda: eng.m3_score_rows_dev(rows, k, ids_o, sc_o, q_emb=q_emb, w=(1.0, 0.0, 0.0)),
                "m3_score_rows_dev_sparse_only": lambda: eng.m3_score_rows_dev(rows, k, ids_o, sc_o, w=(0.0, 1.0, 0.0), **sparse),
                "m3_score_rows_dev": lambda: eng.m3_score_rows_dev(rows, k, ids_o, sc_o, q_emb=q_emb, q_vecs=qv, q_off=qo, **sparse),
                "tokvec_rerank_dev": lambda: eng.tokvec_rerank_dev(qv, qo, rows, k, ids_o, None, sc_o)}
        for fn in arms.values():
            fn()
        torch.cuda.synchronize()
        ids1, sc1, comp1, cand1 = [t.clone() for t in eng.retrieve_m3_dev(q_emb, pool, k, q_vecs=qv, q_off=qo, mode=1, **sparse)]
        _, _, cand_y = eng.retrieve_maxsim_dev(q_emb, qv, qo, pool, k, **sparse)
        torch.cuda.synchronize()
        assert torch.equal(cand1, cand_y) and (ids1[:, 0] >= 0).all() and torch.isfinite(sc1).all(), "the arms do not see the same candidates"
        reps = max(10, 5 * 1024 // tdim)
        ms = {name: [] for name in arms}
        quick = ("sparse_score_rows_dev", "m3_score_rows_dev_dense_only", "m3_score_rows_dev_sparse_only")
        for rnd in range(args.rounds + 1):                               # the arms alternate round by round
            for name, fn in arms.items():
                t = window(fn, 200 if name in quick else reps)
                if rnd > 0:                                              # round 0 settles the clocks after the allocations
                    ms[name].append(t)
        r = {name: summary(v) for name, v in ms.items()}
        r["added_ms_mode1_over_maxsim_composite"] = r["retrieve_m3_dev_mode1"]["median_ms"] - r["retrieve_maxsim_dev_mode1"]["median_ms"]
        lookups = nq * pool * q_terms
        r["sparse_score_rows_dev"].update(lookups=lookups, lookups_per_s=lookups / (r["sparse_score_rows_dev"]["median_ms"] * 1e-3))
        r["added_ms_score_rows_over_tokvec_rerank"] = r["m3_score_rows_dev"]["median_ms"] - r["tokvec_rerank_dev"]["median_ms"]
        r["added_cosine_bytes"] = nq * pool * dim * 4
        r["store_hbm_bytes"] = eng.tokvec_info()["hbm_bytes"]
        r["what"] = (f"{nq} queries x pool {pool}, {qr} query rows, {dr} passage rows, token dim {tdim}, {q_terms} query terms, index dim {dim}, "
                     f"{n_docs} documents, {int(indptr[-1])} postings; top-{k}")
        res[f"dim{tdim}"] = r
        print(f"token dim {tdim}", json.dumps({a: round(r[a]["median_ms"], 4) for a in arms}), "added ms", round(r["added_ms_mode1_over_maxsim_composite"], 4),
              "lookups/s", f"{r['sparse_score_rows_dev']['lookups_per_s']:.3e}", flush=True)
        del qv
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    eng.close()


if __name__ == "__main__":
    main()
