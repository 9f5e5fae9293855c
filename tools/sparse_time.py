"""Times the learned-sparse index against the BM25 leg on one MI355X; writes profiles/sparse_index.json.

Workload: 1M documents; the postings are the CSR of the bench's BM25 text generator (bench_modes.zipf_postings_gpu: document
length ~ Poisson(120), tokens truncated-Zipf(1.1) over 100,000 terms) - loaded once as BM25 postings (tf as generated) and once
as learned-sparse postings (the SAME offsets and documents, tf replaced by seeded float32 weights U(0, 2) + 1e-3); 1024 queries
of 4-12 terms drawn from sampled documents (bench_modes.term_queries_from_docs) with seeded float32 weights; top-100.

(a) rag_sparse_topk_dev against rag_bm25_topk_dev on that CSR and those queries, the two alternating in one process.
(b) rag_hybrid_sparse_rrf_dev against rag_hybrid_rrf_dev over a 1M x 1536 dense index, pool 100, k 20, the same way.
Bytes per query: sum of df x 8 B (sparse) / x 12 B (BM25) over the query's tokens.

Method: device-pointer entries on resident arrays, device events around `--reps` back-to-back calls, one discarded round, then
`--rounds` timed ones, the arms alternating round by round; per arm the median over rounds with the fastest and slowest beside it.
The file is stamped with the commit it was measured on (`git rev-parse HEAD`, or --rev where the tree travels without its
history). Needs a GPU: no fallback.

    python tools/sparse_time.py [--rounds 5] [--reps 5] [--rows 1000000] [--out profiles/sparse_index.json] [--rev COMMIT]"""
import argparse
import json
import os
import statistics
import subprocess
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


def alternating(arms, reps, rounds):
    """{name: fn} -> {name: [ms per call of every timed round]}; round 0 is discarded, the arms alternate round by round"""
    ms = {k: [] for k in arms}
    for rnd in range(rounds + 1):
        for name, fn in arms.items():
            t = window(fn, reps)
            if rnd > 0:
                ms[name].append(t)
    return ms


def summary(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), rounds_ms=v)


def commit(rev):
    if rev:
        return rev
    try:
        return subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--rev", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_index.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("sparse_time: needs a GPU")
    import bench_modes as BM
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.bm25 import Bm25Postings
    N, Q, V, DIM, pool, k = args.rows, args.queries, 100_000, 1536, 100, 20
    device = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0), commit=commit(args.rev), rounds=args.rounds, reps_per_round=args.reps,
               what=f"{N} documents, {V} terms, Poisson(120) lengths, Zipf(1.1) tokens; {Q} queries of 4-12 terms, top-{pool}")
    qdocs = np.random.default_rng(7).integers(0, N, Q)
    indptr, doc, tf, dl, sampled = BM.zipf_postings_gpu(N, V, 120, device, sample_docs=qdocs)
    ptr, terms = BM.term_queries_from_docs(sampled, qdocs)
    rng = np.random.default_rng(11)
    weight = (rng.random(doc.shape[0], dtype=np.float32) * np.float32(2.0)) + np.float32(1e-3)
    qw = (rng.random(terms.shape[0], dtype=np.float32) * np.float32(2.0)) + np.float32(1e-3)
    df = np.diff(indptr)
    touched = float(df[terms[terms >= 0]].sum())
    res["postings"] = dict(nnz=int(indptr[-1]), postings_touched_per_batch=touched, sparse_bytes_per_query=touched * 8 / Q,
                           bm25_bytes_per_query=touched * 12 / Q)
    eng = RagEngine(dim=DIM, device=0)
    post = Bm25Postings(indptr, doc, tf, dl, Bm25Postings.idf_table(df.clip(min=0), N), float(dl.sum()) / N)
    post.idf[df == 0] = 0.0
    post.load(eng)
    eng.sparse_load(indptr, doc, weight, N)
    res["sparse_info"] = eng.sparse_info()
    del weight, tf, doc
    ptr_d, terms_d, qw_d = (torch.from_numpy(a).to(device) for a in (ptr, terms, qw))
    ids = torch.empty((Q, pool), dtype=torch.int64, device=device)
    sc = torch.empty((Q, pool), dtype=torch.float64, device=device)
    arms = {"bm25_topk_dev": lambda: eng.bm25_topk_dev(ptr_d, terms_d, pool, ids, None, sc),
            "sparse_topk_dev": lambda: eng.sparse_topk_dev(ptr_d, terms_d, qw_d, pool, ids, None, sc)}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    a = {n: summary(v) for n, v in alternating(arms, args.reps, args.rounds).items()}
    a["sparse_over_bm25"] = a["sparse_topk_dev"]["median_ms"] / a["bm25_topk_dev"]["median_ms"]
    a["bm25_spread"] = a["bm25_topk_dev"]["max_ms"] / a["bm25_topk_dev"]["min_ms"]
    a["sparse_algorithmic_GBs"] = touched * 8 / (a["sparse_topk_dev"]["median_ms"] * 1e-3) / 1e9
    a["bm25_algorithmic_GBs"] = touched * 12 / (a["bm25_topk_dev"]["median_ms"] * 1e-3) / 1e9
    res["topk"] = a
    print("topk", json.dumps({n: round(a[n]["median_ms"], 3) for n in arms}), "sparse / bm25 =", round(a["sparse_over_bm25"], 3),
          "| bm25 max / min =", round(a["bm25_spread"], 3), flush=True)

    g = torch.Generator(device=device)
    g.manual_seed(1234)
    corpus = torch.randn((N, DIM), generator=g, device=device)
    corpus /= corpus.norm(dim=1, keepdim=True)
    rows = torch.randint(0, N, (Q,), generator=torch.Generator().manual_seed(4321))
    q = corpus[rows.to(device)] + torch.randn((Q, DIM), generator=g, device=device) * (0.5 / DIM ** 0.5)
    q = (q / q.norm(dim=1, keepdim=True)).contiguous()
    eng.index_load(corpus)
    del corpus
    arms = {"hybrid_rrf_dev": lambda: eng.hybrid_rrf_dev(q, ptr_d, terms_d, pool, k),
            "hybrid_sparse_rrf_dev": lambda: eng.hybrid_sparse_rrf_dev(q, ptr_d, terms_d, qw_d, pool, k)}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    b = {n: summary(v) for n, v in alternating(arms, args.reps, args.rounds).items()}
    b["sparse_over_bm25"] = b["hybrid_sparse_rrf_dev"]["median_ms"] / b["hybrid_rrf_dev"]["median_ms"]
    b["bm25_spread"] = b["hybrid_rrf_dev"]["max_ms"] / b["hybrid_rrf_dev"]["min_ms"]
    b["what"] = f"dense index {N} x {DIM}, pool {pool}, k {k}; both hybrids fork their keyword leg onto the side stream"
    res["hybrid"] = b
    print("hybrid", json.dumps({n: round(b[n]["median_ms"], 3) for n in arms}), "sparse / bm25 =", round(b["sparse_over_bm25"], 3),
          "| bm25 max / min =", round(b["bm25_spread"], 3), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    eng.close()


if __name__ == "__main__":
    main()
