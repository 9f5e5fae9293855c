"""Times the live writes to the learned-sparse postings and the token-vector store on one MI355X; writes profiles/live_resident.json.

Shape: 1M documents with the sparse corpus of tools/sparse_time.py (bench_modes.zipf_postings_gpu: Poisson(120) lengths,
Zipf(1.1) tokens over 100,000 terms, seeded float32 weights), a `--dim`-wide dense index of the same rows, and the token-vector
store of tools/tokvec_time.py: 25,600 documents x 255 rows x 1024 (13.4 GB as fp16).

(1) rag_index_compact_live after deleting a seeded 10 % of the rows, against the only way to reach the same state without it:
    rag_index_compact_bm25, then rag_sparse_load_host of the survivors' CSR and the survivors' vectors uploaded from float32
    host memory into a fresh reservation (rag_tokvec_reserve + rag_tokvec_append_host in blocks of 1,600 documents from one host
    block: the transfer and conversion of rag_tokvec_load_host without a 24 GB host array). The survivors' CSR is prepared
    outside the timed window; both arms run on this build (the three calls of the old way are unchanged by it).
(2) rag_sparse_append_host of 1,000 rows onto a tail of 0 and of 50,000 documents, against rag_sparse_load_host of the whole CSR.
(3) rag_sparse_topk_dev over base + tail (51,000 tail documents) against the folded index, with the BM25 arm of
    tools/sparse_time.py beside them as the yardstick of the session's spread.
Also the device-to-device copy rate of this process (a 4 GiB torch copy), for the store's move.

Method: host calls are synchronous: wall time (time.perf_counter) around the call, state rebuilt before every round; searches by
device events around `--reps` calls, arms alternating. One discarded round, then `--rounds`; median with fastest and slowest.

    python tools/live_resident_time.py [--rounds 5] [--rows 1000000] [--out profiles/live_resident.json] [--rev COMMIT]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def summary(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), rounds_ms=v)


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def doc_slice(indptr, doc, w, a, b):
    """term-major CSR of the documents [a, b), renumbered from 0"""
    keep = (doc >= a) & (doc < b)
    term_of = np.repeat(np.arange(indptr.shape[0] - 1, dtype=np.int64), np.diff(indptr))
    out = np.zeros_like(indptr)
    np.cumsum(np.bincount(term_of[keep], minlength=indptr.shape[0] - 1), out=out[1:])
    return out, (doc[keep] - a).astype(np.int32), w[keep].copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--store-docs", type=int, default=25_600)
    ap.add_argument("--doc-rows", type=int, default=255)
    ap.add_argument("--tok-dim", type=int, default=1024)
    ap.add_argument("--rev", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_resident.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("live_resident_time: needs a GPU")
    import bench_modes as BM
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.bm25 import Bm25Postings
    from sparse_time import alternating, commit
    N, V, Q, pool, R = args.rows, 100_000, 1024, 100, args.rounds
    SD, DR, TD, BLK = args.store_docs, args.doc_rows, args.tok_dim, 1_600
    device = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0), commit=commit(args.rev), rounds=R,
               what=f"{N} documents x dim {args.dim}, {V} terms; store {SD} x {DR} x {TD} fp16")
    qdocs = np.random.default_rng(7).integers(0, N, Q)
    indptr, doc, tf, dl, sampled = BM.zipf_postings_gpu(N, V, 120, device, sample_docs=qdocs)
    ptr, terms = BM.term_queries_from_docs(sampled, qdocs)
    rng = np.random.default_rng(11)
    weight = (rng.random(doc.shape[0], dtype=np.float32) * np.float32(2.0)) + np.float32(1e-3)
    qw = (rng.random(terms.shape[0], dtype=np.float32) * np.float32(2.0)) + np.float32(1e-3)
    nnz = int(indptr[-1])
    res["postings"] = dict(nnz=nnz, csr_bytes=nnz * 8 + (V + 1) * 8)

    # ---- (2) appends and (3) search over base + tail, on handles without a dense index --------------------------------------
    NB = N - 51_000
    base = doc_slice(indptr, doc, weight, 0, NB)
    tail50 = doc_slice(indptr, doc, weight, NB, NB + 50_000)
    blk0 = doc_slice(indptr, doc, weight, NB, NB + 1_000)
    blk50 = doc_slice(indptr, doc, weight, NB + 50_000, NB + 51_000)
    eng = RagEngine(dim=args.dim, device=0)
    eng.set_option("sparse_tail_fold", -1)
    t_load, t_app0, t_app50 = [], [], []
    for rnd in range(R + 1):
        a = wall_ms(lambda: eng.sparse_load(indptr, doc, weight, N))
        eng.sparse_load(*base, NB)
        b = wall_ms(lambda: eng.sparse_append(*blk0, 1_000))
        eng.sparse_load(*base, NB)
        eng.sparse_append(*tail50, 50_000)
        c = wall_ms(lambda: eng.sparse_append(*blk50, 1_000))
        if rnd:
            t_load.append(a), t_app0.append(b), t_app50.append(c)
    s = eng.sparse_segment_stats()
    res["append"] = dict(sparse_load_whole_csr=summary(t_load), append_1000_onto_empty_tail=summary(t_app0),
                         append_1000_onto_50000_tail=summary(t_app50), block_nnz=[int(blk0[0][-1]), int(blk50[0][-1])],
                         tail_bytes_rebuilt=s["tail_bytes"], segments=s)
    print("append", json.dumps({k: round(v["median_ms"], 2) for k, v in res["append"].items() if isinstance(v, dict) and "median_ms" in v}), flush=True)
    folded, bm = RagEngine(dim=args.dim, device=0), RagEngine(dim=args.dim, device=0)
    folded.sparse_load(indptr, doc, weight, N)
    df = np.diff(indptr)
    post = Bm25Postings(indptr, doc, tf, dl, Bm25Postings.idf_table(df.clip(min=0), N), float(dl.sum()) / N)
    post.idf[df == 0] = 0.0
    post.load(bm)
    ptr_d, terms_d, qw_d = (torch.from_numpy(a).to(device) for a in (ptr, terms, qw))
    ids = torch.empty((Q, pool), dtype=torch.int64, device=device)
    sc = torch.empty((Q, pool), dtype=torch.float64, device=device)
    arms = {"bm25_topk_dev": lambda: bm.bm25_topk_dev(ptr_d, terms_d, pool, ids, None, sc),
            "sparse_base_plus_tail": lambda: eng.sparse_topk_dev(ptr_d, terms_d, qw_d, pool, ids, None, sc),
            "sparse_folded": lambda: folded.sparse_topk_dev(ptr_d, terms_d, qw_d, pool, ids, None, sc)}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    a = {n: summary(v) for n, v in alternating(arms, args.reps, R).items()}
    a["tail_over_folded"] = a["sparse_base_plus_tail"]["median_ms"] / a["sparse_folded"]["median_ms"]
    a["bm25_spread"] = a["bm25_topk_dev"]["max_ms"] / a["bm25_topk_dev"]["min_ms"]
    res["search"] = a
    print("search", json.dumps({n: round(a[n]["median_ms"], 3) for n in arms}), "tail / folded =", round(a["tail_over_folded"], 3),
          "| bm25 max / min =", round(a["bm25_spread"], 3), flush=True)
    for e in (eng, folded, bm):
        e.close()
    del post, tf

    # ---- the copy rate of this process ---------------------------------------------------------------------------------------
    x = torch.empty(1 << 30, dtype=torch.float32, device=device)
    y = torch.empty_like(x)
    y.copy_(x)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(4):
        y.copy_(x)
    ev[1].record()
    ev[1].synchronize()
    res["d2d_copy_GBs"] = 4 * x.numel() * 4 / (ev[0].elapsed_time(ev[1]) * 1e-3) / 1e9      # bytes copied (read + written: twice that)
    del x, y

    # ---- (1) the compaction ----------------------------------------------------------------------------------------------------
    g = torch.Generator(device=device)
    g.manual_seed(1234)
    corpus = torch.randn((N, args.dim), generator=g, device=device)
    block = torch.randn((BLK * DR, TD), generator=g, device=device)
    block /= block.norm(dim=1, keepdim=True)
    off_d = torch.arange(0, BLK + 1, dtype=torch.int64, device=device) * DR
    block_h, off_h = block.cpu().numpy(), off_d.cpu().numpy()
    dead = np.sort(np.random.default_rng(5).choice(N, N // 10, replace=False)).astype(np.int64)
    live = np.ones(N, dtype=bool)
    live[dead] = False
    new_of = np.where(live, np.cumsum(live) - 1, -1)
    keep = live[doc]
    term_of = np.repeat(np.arange(V, dtype=np.int64), np.diff(indptr))
    s_ptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(term_of[keep], minlength=V), out=s_ptr[1:])
    s_doc, s_w = new_of[doc[keep]].astype(np.int32), weight[keep].copy()
    del term_of, keep
    sd_live = int(live[:SD].sum())
    eng = RagEngine(dim=args.dim, device=0)

    def setup():
        eng.index_load(corpus)
        eng.sparse_load(indptr, doc, weight, N)
        eng.tokvec_reserve(SD, SD * DR, TD)
        for _ in range(SD // BLK):
            eng.tokvec_append_dev(block, off_d)
        assert eng.index_delete(dead) == dead.shape[0]

    def old_way():
        eng.index_compact(keep_postings=True)
        eng.sparse_load(s_ptr, s_doc, s_w, N - dead.shape[0])
        eng.tokvec_reserve(SD, SD * DR, TD)
        left = sd_live
        while left > 0:
            n = min(BLK, left)
            eng.tokvec_append(block_h[:n * DR], off_h[:n + 1])
            left -= n

    t_live, t_old = [], []
    for rnd in range(R + 1):
        setup()
        a = wall_ms(lambda: eng.index_compact(keep_resident=True))
        assert eng.tokvec_info()["n_docs"] == sd_live and eng.sparse_info()["nnz"] == s_doc.shape[0]
        setup()
        b = wall_ms(old_way)
        if rnd:
            t_live.append(a), t_old.append(b)
    store_bytes = sd_live * DR * TD * 2
    res["compact"] = dict(compact_live=summary(t_live), compact_bm25_plus_reloads=summary(t_old), deleted_rows=int(dead.shape[0]),
                          store_documents_left=sd_live, store_bytes_left=store_bytes, postings_left=int(s_doc.shape[0]),
                          floor_bytes=dict(store_read_plus_written=2 * store_bytes, postings_streamed_twice=2 * nnz * 8,
                                           row_planes_read_plus_written=2 * (N - dead.shape[0]) * (args.dim * 4 + args.dim * 2 + 8)))
    res["compact"]["speedup"] = res["compact"]["compact_bm25_plus_reloads"]["median_ms"] / res["compact"]["compact_live"]["median_ms"]
    print("compact", json.dumps({k: round(v["median_ms"], 1) for k, v in res["compact"].items() if isinstance(v, dict) and "median_ms" in v}),
          "old / live =", round(res["compact"]["speedup"], 2), "| d2d copy GB/s =", round(res["d2d_copy_GBs"], 1), flush=True)
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
