"""Times the device id-to-row map (csrc/idmap.hip) on one MI355X and writes profiles/idmap.json:

  build     rag_index_id_map(h, 1) at 1M and 12.5M serial ids (index dim 4, so only the id plane matters): host wall time of the
            call (allocation, the clear / put / order launches, the read-back of the counters), HBM bytes, longest_probe
  lookup    rag_index_rows_of_ids_dev of 256 x 200 ids (half of them unknown) on the 12.5M table, device events
  search    world-1 sharded.ShardedM3Index.search_m3 with explicit ids (7 + 3 * row, map enabled) against the same rows under
            id_base on the SAME handle - the protocol and shape of tools/m3_sharded_time.py: arms alternating, one discarded
            round, `--rounds` x `--reps` calls, per arm the median with the fastest and slowest beside it. The ids are switched
            between the windows (rag_index_set_ids_host), outside what is timed; before anything is timed the two forms' results
            are checked to be the same rows, scores and components.

    python tools/idmap_time.py [--rounds 5] [--reps 10] [--out profiles/idmap.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from m3_fused_time import postings, summary  # noqa: E402
from m3_tenants_time import window  # noqa: E402


def build_times(n, rounds):
    from optimized_rag_amd import RagEngine
    eng = RagEngine(dim=4, device=0)
    rng = np.random.default_rng(1)
    eng.index_load(rng.standard_normal((n, 4)).astype(np.float32), ids=1000 + np.arange(n, dtype=np.int64))
    ms = []
    for _ in range(rounds + 1):
        eng.index_id_map(False)
        t0 = time.perf_counter()
        eng.index_id_map(True)
        ms.append((time.perf_counter() - t0) * 1e3)
    info = eng.index_id_map_info()
    return eng, dict(ids=n, build=summary(ms[1:]), slots=info["slots"], hbm_bytes=info["hbm_bytes"], longest_probe=info["longest_probe"],
                     ids_ascending=info["ids_ascending"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "idmap.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("idmap_time: needs a GPU")
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.sharded import ShardedM3Index
    res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, reps_per_round=args.reps, builds=[])
    eng, b = build_times(1_000_000, args.rounds)
    eng.close()
    res["builds"].append(b)
    print(json.dumps(b), flush=True)
    eng, b = build_times(12_500_000, args.rounds)
    res["builds"].append(b)
    print(json.dumps(b), flush=True)
    rng = np.random.default_rng(2)
    n_look = 256 * 200
    ask = 1000 + rng.integers(0, 25_000_000, n_look).astype(np.int64)           # half of them past the last id
    ids_dev = torch.from_numpy(ask).cuda()
    rows_dev = torch.empty(n_look, dtype=torch.int32, device="cuda")
    look = lambda: eng.rows_of_ids_dev(ids_dev, rows_dev)
    look()
    torch.cuda.synchronize()
    exp = np.where(ask - 1000 < 12_500_000, ask - 1000, -1).astype(np.int32)
    assert np.array_equal(rows_dev.cpu().numpy(), exp)
    ms = [window(look, args.reps) for _ in range(args.rounds + 1)][1:]
    res["lookup"] = dict(ids=n_look, table_ids=12_500_000, **summary(ms))
    print(json.dumps(res["lookup"]), flush=True)
    eng.close()

    # ---- search_m3 at world 1: explicit ids through the map against id_base, on one handle
    nq, pool, qr, dr, k, q_terms, dim, n_terms, tdim, mode = 256, 100, 32, 255, 20, 32, 1024, 30_000, 128, 2
    n_docs = nq * pool
    res["search_what"] = (f"{nq} queries x pool {pool}, {n_docs} documents; index dim {dim}, {q_terms} query terms, {qr} query rows and {dr} passage "
                          f"rows of token dim {tdim}; mode {mode} ({2 * pool} slots), top-{k}, weights (0.4, 0.2, 0.4); world 1, no gather")
    rng = np.random.default_rng(0)
    eng = RagEngine(dim=dim, device=0)
    ix = ShardedM3Index(eng, rank=0, world=1)
    unit = lambda t: torch.nn.functional.normalize(t, dim=-1)
    torch.manual_seed(0)
    emb = torch.randn((n_docs, dim))
    ix.load_shard(emb.numpy(), 0)
    q_emb = (emb[torch.randint(0, n_docs, (nq,))] + 0.7 * torch.randn((nq, dim))).cuda().contiguous()
    indptr, doc, w, p = postings(rng, n_docs, n_terms, 64)
    eng.sparse_load(indptr, doc, w, n_docs)
    ptr = torch.arange(nq + 1, dtype=torch.int32, device="cuda") * q_terms
    terms = torch.from_numpy(np.concatenate([rng.choice(n_terms, q_terms, replace=False, p=p) for _ in range(nq)]).astype(np.int32)).cuda()
    qw = torch.from_numpy((rng.random(nq * q_terms) * 2.0).astype(np.float32) + np.float32(1e-3)).cuda()
    torch.manual_seed(tdim)
    qv = unit(torch.randn((nq * qr, tdim), device="cuda"))
    qo = torch.arange(nq + 1, dtype=torch.int64, device="cuda") * qr
    eng.tokvec_reserve(n_docs, n_docs * dr, tdim)
    off = torch.arange(257, dtype=torch.int64, device="cuda") * dr
    for b0 in range(0, n_docs, 256):
        m = min(256, n_docs - b0)
        eng.tokvec_append_dev(unit(torch.randn((m * dr, tdim), device="cuda")), off[:m + 1].contiguous())
    explicit = 7 + 3 * np.arange(n_docs, dtype=np.int64)

    def use(form):
        if form == "explicit_ids_map":
            eng.set_ids(explicit)
            eng.index_id_map(True)
        else:
            eng.index_id_map(False)
            eng.lib.rag_index_set_ids_host(eng.h, None, n_docs)

    search = lambda: ix.search_m3(q_emb, ptr, terms, qw, qv, qo, pool, k, mode=mode)
    use("id_base")
    base = {n: v.clone() for n, v in search().items()}
    use("explicit_ids_map")
    got = search()
    torch.cuda.synchronize()
    as_id = lambda t: torch.where(t >= 0, 7 + 3 * t, t)
    assert torch.equal(got["ids"], as_id(base["ids"])) and torch.equal(got["candidates"], as_id(base["candidates"]))
    assert torch.equal(got["scores"].view(torch.int64), base["scores"].view(torch.int64))
    assert torch.equal(got["components"].view(torch.int64), base["components"].view(torch.int64))
    arms = ["id_base", "explicit_ids_map"]
    ms = {a: [] for a in arms}
    for rnd in range(args.rounds + 1):
        for a in (arms if rnd % 2 == 0 else arms[::-1]):
            use(a)
            t = window(search, args.reps)
            if rnd > 0:
                ms[a].append(t)
    r = {a: summary(v) for a, v in ms.items()}
    r["explicit_over_id_base"] = r["explicit_ids_map"]["median_ms"] / r["id_base"]["median_ms"]
    r["id_base_spread"] = r["id_base"]["max_ms"] / r["id_base"]["min_ms"]
    res["search_m3_world1"] = r
    print(json.dumps(r), flush=True)
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
