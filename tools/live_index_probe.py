#!/usr/bin/env python3
"""Live-write costs on a 1M x 1536 index with tenants (rag_index_insert_host / _delete_host / _compact):
single-row insert and single-id delete latency, dense top-k (Q = 256, k = 100) before and after deleting 10 % of the rows at
random, and compaction at 10 % and 50 % deleted rows (bytes moved = rows after the first moved row x the bytes of every
plane). Writes profiles/live_index_1M.json.  python tools/live_index_probe.py [--rows N] [--out PATH]

--bm25: appendable postings instead (rag_bm25_append_host / rag_bm25_fold) on the same index with the bench's synthetic text
(bench_modes.synthetic_csr: Poisson(120) tokens per document, Zipf(1.1) over 100,000 terms): append time for blocks of 1 and
1,000 rows, rag_bm25_topk_dev (Q = 256, k = 100) and rag_hybrid_rrf_dev (pool 100, k 20) with a tail of 0, 1 % and 5 % of the
base, then the fold. Device-synchronised wall times, shapes warmed up. Writes profiles/live_bm25_1M.json.
Then compaction that keeps the postings (rag_index_compact_bm25), with and without a 5 % tail, at 10 % and at 50 % of the rows
deleted, each run on a fresh PAIR of identical handles: one takes rag_index_compact, the other rag_index_compact_bm25 (the difference is the
cost of the posting remap); the first then takes the path the new call replaces - Bm25Postings.compacted on the host +
rag_bm25_load_host - and both are searched (the same CSR, remapped on the device against freshly loaded). --part append /
compact runs one half and merges it into the file.
--part refresh: statistics refreshed on the device (option bm25_keep_tf, rag_bm25_refresh) with a tail of 0 / 1 % / 5 % and 10 % of
the rows deleted, on a PAIR of identical handles, option off and on: the two searches interleaved A/B (and A/A against a second handle without the option) before
anything is deleted; then rag_bm25_refresh, its two halves on their own (rag_bm25_live_counts_host, rag_bm25_set_statistics_host; the host idf
rule is the rest) and the rewrite's achieved TB/s; and what the call replaces, timed in the same run - Bm25Postings.refreshed on the
host + rag_bm25_load_host of the merged CSR. Writes profiles/live_bm25_refresh_1M.json."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def med_ms(f, n):
    t = []
    for _ in range(n):
        a = time.perf_counter()
        f()
        t.append((time.perf_counter() - a) * 1e3)
    return float(np.median(t))


def compact_probe(a, data):
    """Compaction with the postings kept, against the plain compaction + host rebuild + reload it replaces."""
    import torch
    import bench_modes as BM
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.bm25 import Bm25Postings
    N, D, V = a.rows, a.dim, 100_000
    indptr, doc, tf, dl, tok, doc_ptr = data
    rng = np.random.default_rng(1)
    block = rng.standard_normal((min(125_000, N), D), dtype=np.float32)      # the row values do not matter here: one block, repeated
    term_of = np.repeat(np.arange(V, dtype=np.int32), np.diff(indptr))
    Q = 256
    ptr, terms = BM._term_queries(tok, doc_ptr, N, Q)
    pd, td = torch.from_numpy(ptr).cuda(), torch.from_numpy(terms).cuda()
    q = torch.from_numpy(rng.standard_normal((Q, D), dtype=np.float32)).cuda()
    ids = torch.empty((Q, 100), dtype=torch.int64, device="cuda")
    sc = torch.empty((Q, 100), dtype=torch.float64, device="cuda")

    def csr(lo, hi):
        m = (doc >= lo) & (doc < hi)
        ip = np.zeros(V + 1, dtype=np.int64)
        np.cumsum(np.bincount(term_of[m], minlength=V), out=ip[1:])
        return ip, (doc[m] - lo).astype(np.int32), tf[m]
    ip0, d0, tf0 = csr(0, N)
    idf = Bm25Postings.idf_table(np.diff(ip0), N)
    idf[np.diff(ip0) == 0] = 0.0
    avgdl = float(dl[:N].sum()) / N

    def build(n_tail):
        eng = RagEngine(dim=D, device=0)
        eng.index_reserve(N + n_tail + 4096)
        for b in range(0, N, block.shape[0]):
            eng.index_append(block[:min(block.shape[0], N - b)])
        eng.set_option("bm25_tail_fold", -1)
        eng.bm25_load(ip0, d0, tf0, dl[:N], idf, avgdl)
        if n_tail:
            eng.index_insert(block[:n_tail])
            ipt, dt_, tft = csr(N, N + n_tail)
            eng.bm25_append(ipt, dt_, tft, dl[N:N + n_tail], np.zeros(0, dtype=np.float64), V)
        return eng

    def searches(eng):
        return {"bm25_topk_dev_q256_k100_ms": BM._p50_ms(lambda: eng.bm25_topk_dev(pd, td, 100, ids, None, sc), 20, 5),
                "hybrid_rrf_dev_q256_ms": BM._p50_ms(lambda: eng.hybrid_rrf_dev(q, pd, td, 100, 20), 20, 5)}

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        return r, (time.perf_counter() - t0) * 1e3
    out = {}
    warm = RagEngine(dim=D, device=0)                            # both calls once on a small index: the timed ones start warm
    warm.index_load(block[:8192])
    ipw, dw, tfw = csr(0, 8192)
    warm.bm25_load(ipw, dw, tfw, dl[:8192], idf, avgdl)
    for keep_postings in (True, False):
        warm.index_delete(np.arange(int(keep_postings), 4096, 2, dtype=np.int64))
        warm.index_compact(keep_postings=keep_postings)
    warm.close()
    for tail_name, n_tail in (("no_tail", 0), ("tail_5pct", N // 20)):
        n_all = N + n_tail
        ipm, dm, tfm = csr(0, n_all)
        for tag, frac in (("10pct", 0.1), ("50pct", 0.5)):      # a fresh pair per fraction: each run starts from the full index
            plain, keep = build(n_tail), build(n_tail)
            mirror = Bm25Postings(ipm.copy(), dm.copy(), tfm.copy(), dl[:n_all].copy(), idf, avgdl)
            live_ids = np.arange(n_all, dtype=np.int64)          # implicit ids: id = row
            victims = rng.permutation(live_ids)[: int(len(live_ids) * frac)]
            for e in (plain, keep):
                assert e.index_delete(victims) == len(victims)
            s0 = keep.bm25_segment_stats()
            row_map, plain_ms = timed(lambda: plain.index_compact())
            row_map2, keep_ms = timed(lambda: keep.index_compact(keep_postings=True))
            assert np.array_equal(row_map, row_map2)
            s1 = keep.bm25_segment_stats()
            _, host_ms = timed(lambda: mirror.compacted(row_map))
            _, load_ms = timed(lambda: plain.bm25_load(mirror.indptr, mirror.doc, mirror.tf, mirror.doc_len, idf, avgdl))
            live_ids = live_ids[row_map >= 0]
            nnz0, nnz1 = s0["base_nnz"] + s0["tail_nnz"], s1["base_nnz"] + s1["tail_nnz"]
            assert nnz1 == int(mirror.indptr[-1]) and s1["base_docs"] + s1["tail_docs"] == len(live_ids)
            # keep pass: doc ids read, 1 bit per posting written; scatter pass: doc ids + impacts read, survivors written
            nbytes = nnz0 * 4 + nnz0 // 8 + nnz0 // 8 + nnz0 * 12 + nnz1 * 12
            remap_ms = keep_ms - plain_ms
            out[f"{tail_name}_{tag}"] = {
                "rows_before": int(len(row_map)), "rows_after": int(len(live_ids)), "postings_before": int(nnz0), "postings_after": int(nnz1),
                "segments_after": {k: s1[k] for k in ("base_docs", "tail_docs", "base_nnz", "tail_nnz", "appends", "folds")},
                "index_compact_ms": plain_ms, "index_compact_bm25_ms": keep_ms, "remap_ms": remap_ms,
                "remap_bytes": int(nbytes), "remap_gb_per_s": nbytes / (remap_ms * 1e-3) / 1e9 if remap_ms > 0 else None,
                "host_compacted_ms": host_ms, "bm25_load_host_ms": load_ms, "reload_path_ms": host_ms + load_ms,
                "reload_over_remap": (host_ms + load_ms) / remap_ms if remap_ms > 0 else None,
                "search_after_remap": searches(keep), "search_after_reload": searches(plain)}
            print(tail_name, tag, json.dumps(out[f"{tail_name}_{tag}"]), flush=True)
            plain.close()
            keep.close()
    out["note"] = ("remap_ms = rag_index_compact_bm25 - rag_index_compact on identical handles; remap_bytes = the posting arrays streamed "
                   "by the keep and scatter passes (row-map gathers, offsets and table rebuild not counted); reload_path = "
                   "Bm25Postings.compacted on the host + rag_bm25_load_host, which replaces a tail by one base")
    return out


def refresh_probe(a, data):
    """rag_bm25_refresh against the host rebuild + reload it replaces; search times with option bm25_keep_tf off and on."""
    import torch
    import bench_modes as BM
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.bm25 import Bm25Postings
    N, D, V = a.rows, a.dim, 100_000
    indptr, doc, tf, dl, tok, doc_ptr = data
    rng = np.random.default_rng(2)
    block = rng.standard_normal((min(125_000, N), D), dtype=np.float32)
    term_of = np.repeat(np.arange(V, dtype=np.int32), np.diff(indptr))
    Q = 256
    ptr, terms = BM._term_queries(tok, doc_ptr, N, Q)
    pd, td = torch.from_numpy(ptr).cuda(), torch.from_numpy(terms).cuda()
    q = torch.from_numpy(rng.standard_normal((Q, D), dtype=np.float32)).cuda()
    ids = torch.empty((Q, 100), dtype=torch.int64, device="cuda")
    sc = torch.empty((Q, 100), dtype=torch.float64, device="cuda")

    def csr(lo, hi):
        m = (doc >= lo) & (doc < hi)
        ip = np.zeros(V + 1, dtype=np.int64)
        np.cumsum(np.bincount(term_of[m], minlength=V), out=ip[1:])
        return ip, (doc[m] - lo).astype(np.int32), tf[m]
    ip0, d0, tf0 = csr(0, N)
    idf = Bm25Postings.idf_table(np.diff(ip0), N)
    idf[np.diff(ip0) == 0] = 0.0
    avgdl = float(dl[:N].sum()) / N

    def build(n_tail, keep):
        eng = RagEngine(dim=D, device=0)
        eng.index_reserve(N + n_tail + 4096)
        for b in range(0, N, block.shape[0]):
            eng.index_append(block[:min(block.shape[0], N - b)])
        eng.set_option("bm25_tail_fold", -1)
        eng.set_option("bm25_keep_tf", keep)
        eng.bm25_load(ip0, d0, tf0, dl[:N], idf, avgdl)
        if n_tail:
            eng.index_insert(block[:n_tail])
            ipt, dt_, tft = csr(N, N + n_tail)
            eng.bm25_append(ipt, dt_, tft, dl[N:N + n_tail], np.zeros(0, dtype=np.float64), V)
        return eng

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        return r, (time.perf_counter() - t0) * 1e3
    out = {"rows": N, "dim": D, "vocab": V, "mean_doc_len": 120}
    for tail_name, n_tail in (("tail_0", 0), ("tail_1pct", N // 100), ("tail_5pct", N // 20)):
        n_all = N + n_tail
        off, on, off_b = build(n_tail, 0), build(n_tail, 1), build(n_tail, 0)    # off_b: a second handle without the option (A/A)
        calls = {"bm25_topk_dev_q256_k100_ms": lambda e: e.bm25_topk_dev(pd, td, 100, ids, None, sc),
                 "hybrid_rrf_dev_q256_ms": lambda e: e.hybrid_rrf_dev(q, pd, td, 100, 20)}
        ab = {k: {"off": [], "on": [], "off_b": []} for k in calls}
        for _ in range(5):                                       # interleaved: off, on, off_b, off, on, off_b, ...
            for k, f in calls.items():
                for name, e in (("off", off), ("on", on), ("off_b", off_b)):
                    ab[k][name].append(BM._p50_ms(lambda: f(e), 20, 5))
        off_b.close()
        s_on = on.bm25_segment_stats()
        nnz = s_on["base_nnz"] + s_on["tail_nnz"]
        victims = rng.permutation(n_all)[: n_all // 10].astype(np.int64)
        for e in (off, on):
            assert e.index_delete(victims) == len(victims)
        on.bm25_live_counts()                                    # first use of every kernel
        runs, first_info = [], None
        for _ in range(3):
            (idf_new, info), refresh_ms = timed(lambda: on.bm25_refresh())
            first_info = first_info or info
            _, counts_ms = timed(lambda: on.bm25_live_counts())
            _, rewrite_ms = timed(lambda: on.bm25_set_statistics(idf_new, info["avgdl_after"]))
            runs.append((refresh_ms, counts_ms, rewrite_ms))
        refresh_ms, counts_ms, rewrite_ms = (float(np.median([r[i] for r in runs])) for i in range(3))
        rewrite_bytes = nnz * (4 + 2 + 8)                        # doc id + tf read, impact written (doc_len and metadata: gathers, not counted)
        after = {k: BM._p50_ms(lambda: f(on), 20, 5) for k, f in calls.items()}
        after_off = {k: BM._p50_ms(lambda: f(off), 20, 5) for k, f in calls.items()}      # the same deletes, frozen statistics
        ipm, dm, tfm = csr(0, n_all)
        mirror = Bm25Postings(ipm, dm, tfm, dl[:n_all].copy(), np.concatenate([idf]), avgdl)
        fresh, host_ms = timed(lambda: mirror.refreshed())
        _, load_ms = timed(lambda: off.bm25_load(fresh.indptr, fresh.doc, fresh.tf, fresh.doc_len, fresh.idf, fresh.avgdl))
        out[tail_name] = {
            "documents": n_all, "postings": int(nnz), "tail_docs": s_on["tail_docs"], "deleted_rows": int(len(victims)),
            "search_before_deletes_interleaved_ab": ab,
            "search_on_over_off_median": {k: float(np.median(v["on"]) / np.median(v["off"])) for k, v in ab.items()},
            "search_off_spread": {k: [float(min(v["off"] + v["off_b"])), float(max(v["off"] + v["off_b"]))] for k, v in ab.items()},
            "search_on_spread": {k: [float(min(v["on"])), float(max(v["on"]))] for k, v in ab.items()},
            "refresh_ms": refresh_ms, "live_counts_ms": counts_ms, "set_statistics_ms": rewrite_ms,
            "host_idf_ms": refresh_ms - counts_ms - rewrite_ms, "refresh_runs_ms": runs,
            "rewrite_bytes": int(rewrite_bytes), "rewrite_tb_per_s": rewrite_bytes / (rewrite_ms * 1e-3) / 1e12,
            "info": first_info, "search_after_refresh_10pct_deleted": after, "search_option_off_10pct_deleted": after_off,
            "host_refreshed_ms": host_ms, "bm25_load_host_ms": load_ms, "reload_path_ms": host_ms + load_ms,
            "reload_over_refresh": (host_ms + load_ms) / refresh_ms}
        print(tail_name, json.dumps(out[tail_name]), flush=True)
        off.close()
        on.close()
    out["note"] = ("refresh_ms = one rag_bm25_refresh; live_counts_ms / set_statistics_ms = its two halves called on their own right after "
                   "(set_statistics includes the 0.8 MB idf upload), host_idf_ms = the rest (the idf rule on the host + the df download); "
                   "rewrite_bytes = doc id + tf read and impact written per posting; reload_path = Bm25Postings.refreshed on the host + "
                   "rag_bm25_load_host of the merged CSR (statistics over ALL documents: the host mirror has no live mask there)")
    return out


def write_out(a, part):
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out.update(part)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(part))


def bm25_probe(a):
    import torch
    import bench_modes as BM
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.bm25 import Bm25Postings
    N, D, V = a.rows, a.dim, 100_000
    extra = N // 20 + 8192                                # the 5 % tail and the timed blocks behind it
    indptr, doc, tf, dl, tok, doc_ptr = BM.synthetic_csr(N + extra, V, 120)
    if a.part == "refresh":
        a.out = a.refresh_out
        return write_out(a, refresh_probe(a, (indptr, doc, tf, dl, tok, doc_ptr)))
    if a.part in ("all", "compact"):
        write_out(a, {"compaction": compact_probe(a, (indptr, doc, tf, dl, tok, doc_ptr))})
    if a.part == "compact":
        return
    rng = np.random.default_rng(0)
    eng = RagEngine(dim=D, device=0)
    eng.index_reserve(N + extra + 4096)
    for b in range(0, N, 125_000):
        eng.index_append(rng.standard_normal((min(125_000, N - b), D), dtype=np.float32))
    term_of = np.repeat(np.arange(V, dtype=np.int32), np.diff(indptr))
    is_base = doc < N

    def csr(mask, first):
        ip = np.zeros(V + 1, dtype=np.int64)
        np.cumsum(np.bincount(term_of[mask], minlength=V), out=ip[1:])
        return ip, (doc[mask] - first).astype(np.int32), tf[mask]
    ip0, d0, tf0 = csr(is_base, 0)
    idf = Bm25Postings.idf_table(np.diff(ip0), N)
    idf[np.diff(ip0) == 0] = 0.0
    avgdl = float(dl[:N].sum()) / N
    eng.set_option("bm25_tail_fold", -1)                  # the probe folds when it says so
    eng.bm25_load(ip0, d0, tf0, dl[:N], idf, avgdl)
    e_term, e_doc, e_tf = term_of[~is_base], doc[~is_base], tf[~is_base]
    del term_of, is_base, ip0, d0, tf0
    none = np.zeros(0, dtype=np.float64)

    def grow(n):                                          # insert + append the next n documents; returns the append's seconds
        first = eng.n_rows
        m = (e_doc >= first) & (e_doc < first + n)
        ip = np.zeros(V + 1, dtype=np.int64)
        np.cumsum(np.bincount(e_term[m], minlength=V), out=ip[1:])
        bd, bt, bl = (e_doc[m] - first).astype(np.int32), e_tf[m], dl[first:first + n]
        eng.index_insert(rng.standard_normal((n, D), dtype=np.float32))
        t0 = time.perf_counter()
        eng.bm25_append(ip, bd, bt, bl, none, V)
        return (time.perf_counter() - t0) * 1e3
    Q = 256
    ptr, terms = BM._term_queries(tok, doc_ptr, N, Q)
    pd, td = torch.from_numpy(ptr).cuda(), torch.from_numpy(terms).cuda()
    q = torch.from_numpy(rng.standard_normal((Q, D), dtype=np.float32)).cuda()
    ids = torch.empty((Q, 100), dtype=torch.int64, device="cuda")
    sc = torch.empty((Q, 100), dtype=torch.float64, device="cuda")

    def searches():
        return {"bm25_topk_dev_q256_k100_ms": BM._p50_ms(lambda: eng.bm25_topk_dev(pd, td, 100, ids, None, sc), 20, 5),
                "hybrid_rrf_dev_q256_ms": BM._p50_ms(lambda: eng.hybrid_rrf_dev(q, pd, td, 100, 20), 20, 5)}
    out = {"rows": N, "dim": D, "vocab": V, "mean_doc_len": 120, "base_nnz": int(eng.bm25_segment_stats()["base_nnz"]), "tails": {}}
    for name, target in (("0", 0), ("1pct", N // 100), ("5pct", N // 20)):
        have = eng.bm25_segment_stats()["tail_docs"]
        if target > have:
            grow(target - have)
        st = eng.bm25_segment_stats()
        rec = {"tail_docs": st["tail_docs"], "tail_nnz": st["tail_nnz"], "tail_bytes": st["tail_bytes"]}
        rec.update(searches())
        rec["append_1row_ms"] = float(np.median([grow(1) for _ in range(7)]))
        rec["append_1000rows_ms"] = float(np.median([grow(1000) for _ in range(3)]))
        out["tails"][name] = rec
    st = eng.bm25_segment_stats()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.bm25_fold()
    fold_ms = (time.perf_counter() - t0) * 1e3
    nnz = st["base_nnz"] + st["tail_nnz"]
    out["fold"] = {"tail_docs": st["tail_docs"], "tail_nnz": st["tail_nnz"], "ms": fold_ms,
                   "bytes_moved": int(nnz * 12 * 2), "note": "every posting (doc int32 + impact float64) read once and written once; tables rebuilt"}
    out["fold"]["tb_per_s"] = out["fold"]["bytes_moved"] / (fold_ms * 1e-3) / 1e12
    out["after_fold"] = searches()
    write_out(a, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bm25", action="store_true", help="probe the appendable postings instead (profiles/live_bm25_1M.json)")
    ap.add_argument("--part", choices=("all", "append", "compact", "refresh"), default="all",
                    help="with --bm25: the append / fold runs, the compaction runs, or both (merged into the output file); "
                         "refresh: the statistics refresh, into its own file")
    ap.add_argument("--refresh-out", default=os.path.join(ROOT, "profiles", "live_bm25_refresh_1M.json"))
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "live_bm25_1M.json" if a.bm25 else "live_index_1M.json")
    if a.bm25:
        return bm25_probe(a)
    from optimized_rag_amd import RagEngine
    N, D = a.rows, a.dim
    rng = np.random.default_rng(0)
    eng = RagEngine(dim=D, device=0)
    eng.index_reserve(N + 4096)                           # headroom: the inserts below do not grow the planes
    for b in range(0, N, 125_000):
        eng.index_append(rng.standard_normal((min(125_000, N - b), D), dtype=np.float32))
    ten = rng.integers(0, 100, N).astype(np.int32)
    eng.set_tenants(ten)
    q = rng.standard_normal((256, D), dtype=np.float32)
    out = {"rows": N, "dim": D, "tenants": 100}
    eng.dense_topk(q, 100)
    out["dense_q256_k100_ms_before"] = med_ms(lambda: eng.dense_topk(q, 100), 10)
    row = rng.standard_normal((1, D), dtype=np.float32)
    nxt = [N]

    def ins():
        eng.index_insert(row, tenants=np.array([int(nxt[0] % 100)], np.int32))
        nxt[0] += 1
    out["insert_1row_ms"] = med_ms(ins, 50)
    victims = iter(rng.permutation(N)[:60].tolist())
    out["delete_1id_ms"] = med_ms(lambda: eng.index_delete([next(victims)]), 50)
    n_now = eng.n_rows
    eng.index_delete(rng.permutation(n_now)[: n_now // 10])
    out["deleted_fraction_for_search"] = eng.index_deleted_rows() / n_now
    eng.dense_topk(q, 100)
    out["dense_q256_k100_ms_after_10pct_deleted"] = med_ms(lambda: eng.dense_topk(q, 100), 10)
    out["dense_after_vs_before"] = out["dense_q256_k100_ms_after_10pct_deleted"] / out["dense_q256_k100_ms_before"]
    row_bytes = D * 4 + ((D + 63) // 64 * 64) * 2 + 8 + 4          # emb32 + emb16 + ids + tenants

    def compact(tag):
        n0 = eng.n_rows
        a_ = time.perf_counter()
        m = eng.index_compact()
        dt = time.perf_counter() - a_
        moved = np.nonzero(m != np.arange(n0))[0]
        first = int(moved[0]) if len(moved) else n0
        nbytes = int((m >= 0)[first:].sum()) * row_bytes
        out[f"compact_{tag}"] = {"rows_before": n0, "rows_after": int((m >= 0).sum()), "ms": dt * 1e3, "bytes_moved": nbytes,
                                 "tb_per_s": nbytes / dt / 1e12}
        return m
    m = compact("10pct")
    live_ids = np.nonzero(m >= 0)[0]                  # ids were implicit (id = row) before this first compaction stored them
    eng.index_delete(rng.permutation(live_ids)[: len(live_ids) // 2])
    compact("50pct")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
