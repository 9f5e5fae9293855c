"""Times the exhaustive MaxSim search (mode 2 of rag_retrieve_maxsim_dev: tokvec_scan_kernel, its select and the closing rerank)
on one MI355X against the rerank kernel's own pair rate on the same store; writes profiles/tokvec_search.json.

Shape: 100,000 passages x 128 rows at dim 128 and dim 1024, stored as fp16 and as mxfp8; 256 queries x 32 rows, pool 100, k 20.
Per (dim, form), in ONE process and alternating round by round:
  search          RagEngine.tokvec_search_dev over every passage                          (25,600,000 pairs per batch)
  search_tenant   the same for a tenant that owns every 100th row                         (256,000 pairs per batch)
  rerank          rag_tokvec_rerank_dev over 256 x 100 random rows of the same store      (25,600 pairs per batch): the yardstick -
                  one workgroup per pair, every pair reading its passage from HBM
Reported per arm: ms per batch (median of the rounds, fastest and slowest beside it), pairs per second, algorithmic FLOP/s
(2 * nq * nd * dim per pair) and issued FLOP/s (twice that: the float32 query enters as hi + lo fp16 halves), each as a fraction
of the fp16 MFMA peak bench.py prices against (PEAK_MFMA_TFLOPS), and the search's pair rate over the rerank's. Before timing, the
search's scores are compared bit for bit with a rerank of its own candidate rows.

Method (as tools/tokvec_time.py): device-pointer entries on resident arrays, device events around `reps` back-to-back calls, one
discarded round, then `--rounds` timed ones. Needs a GPU.

    python tools/tokvec_search_time.py [--rounds 5] [--out profiles/tokvec_search.json] [--dims 128,1024] [--passages 100000]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_MFMA_FLOPS = 2500.0e12          # bench.py PEAK_MFMA_TFLOPS


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
    ap.add_argument("--dims", default="128,1024")
    ap.add_argument("--forms", default="fp16,mxfp8")
    ap.add_argument("--passages", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tokvec_search.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("tokvec_search_time: needs a GPU")
    from optimized_rag_amd import RagEngine
    res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, peak_mfma_flops=PEAK_MFMA_FLOPS)
    unit = lambda t: torch.nn.functional.normalize(t, dim=-1)
    n_docs, nq, qr, dr, pool, k, every = args.passages, args.queries, 32, 128, 100, 20, 100
    eng = RagEngine(dim=64, device=0)
    eng.index_load(torch.randn((n_docs, 64), device="cuda"))
    eng.set_tenants((np.arange(n_docs) % every == 0).astype(np.int32))      # tenant 1 owns every 100th row: 1 % of them
    n_tenant = (n_docs + every - 1) // every
    for dim in [int(x) for x in args.dims.split(",")]:
        for form in args.forms.split(","):
            torch.manual_seed(dim)
            qv = unit(torch.randn((nq * qr, dim), device="cuda"))
            qo = torch.arange(nq + 1, dtype=torch.int64, device="cuda") * qr
            eng.tokvec_reserve(n_docs, n_docs * dr, dim, form=form)
            block = max(1, (1 << 28) // (dr * dim))                         # documents per append: 1 GiB of float32
            off = torch.arange(block + 1, dtype=torch.int64, device="cuda") * dr
            for b in range(0, n_docs, block):
                m = min(block, n_docs - b)
                eng.tokvec_append_dev(unit(torch.randn((m * dr, dim), device="cuda")), off[:m + 1].contiguous())
            info = eng.tokvec_info()
            assert info["n_docs"] == n_docs and info["rows"] == n_docs * dr
            cand = torch.randint(0, n_docs, (nq, pool), dtype=torch.int32, device="cuda")
            ids, sc = torch.empty((nq, k), dtype=torch.int64, device="cuda"), torch.empty((nq, k), dtype=torch.float64, device="cuda")
            arms = {"search": lambda: eng.tokvec_search_dev(qv, qo, k, pool=pool),
                    "search_tenant": lambda: eng.tokvec_search_dev(qv, qo, k, pool=pool, tenant=1),
                    "rerank": lambda: eng.tokvec_rerank_dev(qv, qo, cand, k, ids, None, sc)}
            pairs = {"search": nq * n_docs, "search_tenant": nq * n_tenant, "rerank": nq * pool}
            # the search's scores are the rerank's bits for the same rows (ids are rows here: implicit ids from 0)
            s_ids, s_sc, s_cand = [t.clone() for t in arms["search"]()]
            eng.tokvec_rerank_dev(qv, qo, s_cand.to(torch.int32), k, ids, None, sc)
            torch.cuda.synchronize()
            assert torch.equal(ids, s_ids) and torch.equal(sc.view(torch.int64), s_sc.view(torch.int64)) and bool((s_ids >= 0).all())
            t_ids = arms["search_tenant"]()[0]
            torch.cuda.synchronize()
            assert bool((t_ids % every == 0).all())
            one = window(arms["search"], 1)
            reps = {"search": max(1, int(500 / one)), "search_tenant": 10, "rerank": 20}       # about half a second of search per window
            ms = {name: [] for name in arms}
            for rnd in range(args.rounds + 1):                              # the arms alternate round by round
                for name, fn in arms.items():
                    t = window(fn, reps[name])
                    if rnd > 0:                                            # round 0 settles the clocks after the allocations
                        ms[name].append(t)
            r = {}
            for name, v in ms.items():
                s = summary(v)
                per_s = pairs[name] / (s["median_ms"] * 1e-3)
                flops = per_s * 2 * qr * dr * dim
                s.update(pairs_per_batch=pairs[name], pairs_per_s=per_s, algorithmic_flops_per_s=flops, issued_flops_per_s=2 * flops,
                         algorithmic_fraction_of_mfma_peak=flops / PEAK_MFMA_FLOPS, issued_fraction_of_mfma_peak=2 * flops / PEAK_MFMA_FLOPS,
                         reps_per_round=reps[name])
                r[name] = s
            r["search_pair_rate_over_rerank"] = r["search"]["pairs_per_s"] / r["rerank"]["pairs_per_s"]
            r["search_tenant_pair_rate_over_rerank"] = r["search_tenant"]["pairs_per_s"] / r["rerank"]["pairs_per_s"]
            r["what"] = (f"{n_docs} passages x {dr} rows, dim {dim}, {form}; {nq} queries x {qr} rows, pool {pool}, k {k}; the tenant owns "
                         f"{n_tenant} passages; select and closing rerank included in the search arms")
            r["store_hbm_bytes"] = info["hbm_bytes"]
            res[f"dim{dim}_{form}"] = r
            print(f"dim {dim} {form}", json.dumps({a: {x: round(r[a][x], 4) for x in ("median_ms", "min_ms", "max_ms", "issued_fraction_of_mfma_peak")}
                                                   for a in ms}), "pair rate over rerank", round(r["search_pair_rate_over_rerank"], 3),
                  "tenant", round(r["search_tenant_pair_rate_over_rerank"], 3), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:                                 # after every shape: a partial file is still a record
                json.dump(res, f, indent=1)
                f.write("\n")
            del qv
    eng.close()


if __name__ == "__main__":
    main()
