#!/usr/bin/env python3
"""Live-write costs on a 1M x 1536 index with tenants (rag_index_insert_host / _delete_host / _compact):
single-row insert and single-id delete latency, dense top-k (Q = 256, k = 100) before and after deleting 10 % of the rows at
random, and compaction at 10 % and 50 % deleted rows (bytes moved = rows after the first moved row x the bytes of every
plane). Writes profiles/live_index_1M.json.  python tools/live_index_probe.py [--rows N] [--out PATH]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_index_1M.json"))
    a = ap.parse_args()
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
