"""Times what the SPLIT form of the linear fusion costs on one MI355X: world-1 sharded.ShardedHybridIndex.search_linear
(rag_hybrid_linear_begin_dev, rag_hybrid_linear_finish_dev, rag_hybrid_linear_merge_gathered_dev; no gather at world 1) against the
one-call rag_hybrid_linear_dev on the same handle and index; writes profiles/linear_sharded_world1.json. Multi-GPU scaling cannot
be measured on a one-GPU box: this is the price of the extra launches, of the [5][Q][k] block and of the merge alone. There is no
second BM25 pass in the split form - the seam keeps the score planes.

Shape: 1M rows x 1536, BM25 postings of 20,000 Zipf-drawn terms with 32 per document, a temporal vector on 40 % of the rows, 256
queries of 4 terms, k = 20, weights (0.55, 0.35, 0.10). Method as tools/m3_sharded_time.py: device events around `--reps`
back-to-back calls after one untimed call, one discarded round, then `--rounds` timed ones with the two arms alternating and
their order reversed every other round; per arm the median with the fastest and slowest beside it. Before anything is timed the
split form's ids, hybrid bits and component bits are checked against the one call's. `--one-call-only` times the first arm alone
(the same world on another build of the library, for a before / after of rag_hybrid_linear_dev itself). Needs a GPU.

    python tools/linear_sharded_time.py [--rounds 5] [--reps 10] [--rows 1000000] [--out profiles/linear_sharded_world1.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ, K, Q_TERMS, DIM, N_TERMS, PER_DOC = 256, 20, 4, 1536, 20_000, 32
WEIGHTS = (0.55, 0.35, 0.10)


def window(fn, reps):
    """one untimed call, then fn() `reps` times between two device events -> ms per call"""
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def summary(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), rounds_ms=v)


def bm25_csr(rng, n_docs, n_terms, per_doc):
    """term-major CSR (indptr int64, doc int32 ascending inside a term, tf int32) of per_doc Zipf-drawn terms per document, the
    document lengths, and the draw probabilities"""
    p = np.arange(1, n_terms + 1, dtype=np.float64) ** -1.1
    p /= p.sum()
    owner = np.repeat(np.arange(n_docs, dtype=np.int64), per_doc)
    term = rng.choice(n_terms, size=owner.shape[0], p=p).astype(np.int64)
    key, tf = np.unique(term * n_docs + owner, return_counts=True)
    term, doc = key // n_docs, (key % n_docs).astype(np.int32)
    indptr = np.zeros(n_terms + 1, dtype=np.int64)
    np.cumsum(np.bincount(term, minlength=n_terms), out=indptr[1:])
    doc_len = np.full(n_docs, per_doc, np.int32) + rng.integers(0, 20, n_docs).astype(np.int32)
    return indptr, doc, tf.astype(np.int32), doc_len, p


def load_world(eng, n_rows, load=None):
    """Fills the handle (through `load(emb, postings, temporal)` when given, else the plain engine calls) and returns the
    replicated query tensors (q_emb, term_ptr, terms)."""
    import torch
    from optimized_rag_amd.bm25 import Bm25Postings
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    emb = torch.randn((n_rows, DIM), device="cuda")
    q_emb = (emb[torch.randint(0, n_rows, (NQ,), device="cuda")] + 0.7 * torch.randn((NQ, DIM), device="cuda")).contiguous()
    indptr, doc, tf, doc_len, p = bm25_csr(rng, n_rows, N_TERMS, PER_DOC)
    post = Bm25Postings(indptr, doc, tf, doc_len, Bm25Postings.idf_table(np.diff(indptr), n_rows), float(doc_len.sum()) / n_rows)
    temporal = np.where(rng.uniform(size=n_rows) < 0.4, 0.15 * 0.5 ** (rng.uniform(0, 90, n_rows) / 30.0), 0.0)
    if load is not None:
        load(emb, post, temporal)
    else:
        eng.index_load(emb)
        post.load(eng)
        eng.set_temporal(temporal)
    del emb
    ptr = torch.arange(NQ + 1, dtype=torch.int32, device="cuda") * Q_TERMS
    terms = torch.from_numpy(np.concatenate([rng.choice(N_TERMS, Q_TERMS, replace=False, p=p) for _ in range(NQ)]).astype(np.int32)).cuda()
    return q_emb, ptr, terms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--one-call-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_sharded_world1.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("linear_sharded_time: needs a GPU")
    from optimized_rag_amd import RagEngine
    res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, reps_per_round=args.reps,
               what=f"{NQ} queries of {Q_TERMS} terms, {args.rows} rows x {DIM}, BM25 postings of {N_TERMS} terms ({PER_DOC} draws per "
                    f"document), temporal vector, top-{K}, weights {WEIGHTS}; world 1, no gather")
    eng = RagEngine(dim=DIM, device=0)
    ix = None
    if args.one_call_only:
        q_emb, ptr, terms = load_world(eng, args.rows)
    else:
        from optimized_rag_amd.sharded import ShardedHybridIndex
        ix = ShardedHybridIndex(eng, rank=0, world=1)
        q_emb, ptr, terms = load_world(eng, args.rows, load=lambda emb, post, temporal: ix.load_shard(emb, 0, post, temporal=temporal))

    def one_call():
        return eng.hybrid_linear_dev(q_emb, ptr, terms, K, *WEIGHTS)

    def split():
        return ix.search_linear(q_emb, ptr, terms, K, *WEIGHTS)

    arms = {"hybrid_linear_dev": one_call}
    if ix is not None:
        exp = {n: v.clone() for n, v in one_call().items()}
        got = split()
        torch.cuda.synchronize()
        assert torch.equal(got["ids"], exp["ids"]) and (exp["ids"][:, 0] >= 0).all()
        for name in ("hybrid", "semantic", "keyword", "temporal"):
            assert torch.equal(got[name].view(torch.int64), exp[name].view(torch.int64)), name
        assert (exp["keyword"].max(dim=1).values > 0).all(), "every query matches a document"
        arms["sharded_search_linear_world1"] = split
    ms = {name: [] for name in arms}
    for rnd in range(args.rounds + 1):                                   # round 0 is discarded; the order flips every other round
        for name, fn in (list(arms.items()) if rnd % 2 == 0 else list(arms.items())[::-1]):
            t = window(fn, args.reps)
            if rnd > 0:
                ms[name].append(t)
    r = {name: summary(v) for name, v in ms.items()}
    r["one_call_spread"] = r["hybrid_linear_dev"]["max_ms"] / r["hybrid_linear_dev"]["min_ms"]
    if ix is not None:
        r["split_over_one_call"] = r["sharded_search_linear_world1"]["median_ms"] / r["hybrid_linear_dev"]["median_ms"]
    res["arms"] = r
    print(json.dumps({a: r[a] for a in arms}), flush=True)
    print("split / one call:", round(r.get("split_over_one_call", float("nan")), 4), "| one call max / min:", round(r["one_call_spread"], 4),
          flush=True)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
