"""Times the late-interaction rerank over the resident fp16 token-vector store against the float32 pair path on one MI355X; writes
profiles/tokvec_store.json.

Shape: 256 queries x 100 candidates, 32 query rows, 255 passage rows, at dim 1024 and dim 128. Per dim, in ONE process:
  rag_tokvec_rerank_dev   scores + top-20 over the store (25,600 documents x 255 fp16 rows)
  rag_maxsim_dev          the same pairs over float32 copies of the SAME stored (fp16-rounded) vectors
alternating round by round, and a device-to-device copy timed in the same process (read + write bytes over time). Both kernels are
bound by the passage bytes they read (products of sizes: rows x dim x 2 B and x 4 B); reported per arm: the median, the passage
bytes per second and their fraction of the measured copy rate, and the ratio of the two medians. The two arms' scores are compared
first (the same vectors: they agree within the two kernels' 1e-4 bars).

Method (as tools/m3_time.py): device-pointer entries on resident arrays, device events around `reps` back-to-back calls, one
discarded round, then `--rounds` timed ones; per arm the median over rounds with the fastest and slowest beside it. Needs a GPU.

    python tools/tokvec_time.py [--rounds 5] [--out profiles/tokvec_store.json] [--dims 1024,128]"""
import argparse
import json
import os
import statistics
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dims", default="1024,128")
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--candidates", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tokvec_store.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tokvec_time: needs a GPU")
    from optimized_rag_amd import RagEngine
    res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds)
    eng = RagEngine(dim=64, device=0)
    unit = lambda t: torch.nn.functional.normalize(t, dim=-1)

    # ---- the device's copy rate, measured here
    n = 1 << 30
    src, dst = torch.empty(n, dtype=torch.float32, device="cuda").normal_(), torch.empty(n, dtype=torch.float32, device="cuda")
    v = [window(lambda: dst.copy_(src), 5) for _ in range(args.rounds + 1)][1:]
    copy_rate = 2 * 4 * n / (statistics.median(v) * 1e-3)
    res["copy"] = dict(bytes_moved=2 * 4 * n, **summary(v), bytes_per_s=copy_rate)
    print("copy rate GB/s", round(copy_rate / 1e9, 1), flush=True)
    del src, dst

    nq, cand, qr, dr, k = args.queries, args.candidates, 32, 255, 20
    n_docs = nq * cand
    for dim in [int(x) for x in args.dims.split(",")]:
        torch.manual_seed(dim)
        qv = unit(torch.randn((nq * qr, dim), device="cuda"))
        d32 = torch.empty((n_docs * dr, dim), device="cuda")              # float32 copies of the stored vectors
        eng.tokvec_reserve(n_docs, n_docs * dr, dim)
        block = 256                                                        # documents per append
        off = torch.arange(block + 1, dtype=torch.int64, device="cuda") * dr
        for b in range(0, n_docs, block):
            m = min(block, n_docs - b)
            chunk = unit(torch.randn((m * dr, dim), device="cuda"))
            eng.tokvec_append_dev(chunk, off[:m + 1].contiguous())
            d32[b * dr:(b + m) * dr] = chunk.half().float()
        info = eng.tokvec_info()
        assert info["n_docs"] == n_docs and info["rows"] == n_docs * dr
        qo = torch.arange(nq + 1, dtype=torch.int64, device="cuda") * qr
        do = torch.arange(n_docs + 1, dtype=torch.int64, device="cuda") * dr
        pq = torch.arange(n_docs, dtype=torch.int32, device="cuda") // cand
        pd = torch.arange(n_docs, dtype=torch.int32, device="cuda")
        rows = pd.reshape(nq, cand).contiguous()
        out32 = torch.empty((n_docs,), device="cuda")
        ids, sc = torch.empty((nq, k), dtype=torch.int64, device="cuda"), torch.empty((nq, k), dtype=torch.float64, device="cuda")
        ps = torch.empty((nq, cand), device="cuda")
        store = lambda: eng.tokvec_rerank_dev(qv, qo, rows, k, ids, None, sc, ps)
        pairs = lambda: eng.maxsim_dev(qv, qo, d32, do, pq, pd, out32)
        store()
        pairs()
        torch.cuda.synchronize()
        want = (qv[:qr].double() @ d32[:dr].double().T).max(1).values.mean().item()
        diff = (ps.reshape(-1) - out32).abs().max().item()
        assert abs(ps[0, 0].item() - want) < 1e-4 and diff < 2e-4, (ps[0, 0].item(), want, diff)
        assert torch.equal(sc[:, 0], ps.double().max(1).values)
        reps = max(20, 10 * 1024 // dim)                              # at least 0.1 s of work per window
        ms = {"tokvec_rerank_dev": [], "maxsim_dev": []}
        for rnd in range(args.rounds + 1):                               # the arms alternate round by round
            for name, fn in (("tokvec_rerank_dev", store), ("maxsim_dev", pairs)):
                t = window(fn, reps)
                if rnd > 0:                                              # round 0 settles the clocks after the allocations
                    ms[name].append(t)
        r = {name: summary(v) for name, v in ms.items()}
        for name, width in (("tokvec_rerank_dev", 2), ("maxsim_dev", 4)):
            nbytes = n_docs * dr * dim * width
            r[name].update(passage_bytes=nbytes, passage_bytes_per_s=nbytes / (r[name]["median_ms"] * 1e-3),
                           fraction_of_measured_copy_rate=nbytes / (r[name]["median_ms"] * 1e-3) / copy_rate)
        r["speedup_over_maxsim_dev"] = r["maxsim_dev"]["median_ms"] / r["tokvec_rerank_dev"]["median_ms"]
        r["max_abs_score_difference_between_the_arms"] = diff
        r["reps_per_round"] = reps
        r["what"] = f"{nq} queries x {cand} candidates, {qr} query rows, {dr} passage rows, dim {dim}; top-{k} included in the store arm"
        r["store_hbm_bytes"] = info["hbm_bytes"]
        res[f"dim{dim}"] = r
        print(f"dim {dim}", json.dumps({a: {x: r[a][x] for x in ("median_ms", "min_ms", "max_ms", "fraction_of_measured_copy_rate")} for a in ms}),
              "speedup", round(r["speedup_over_maxsim_dev"], 3), flush=True)
        del d32, qv
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    eng.close()


if __name__ == "__main__":
    main()
