"""Times the late-interaction rerank over the 8-bit form of the resident token-vector store (RAG_TOKVEC_MXFP8) against the fp16
form on one MI355X; writes profiles/tokvec_q8.json.

Shape: 256 queries x 100 candidates, 32 query rows, 255 passage rows, at dim 1024 and dim 128. Per dim, in ONE process, two handles
hold the SAME passages (25,600 documents x 255 rows, appended from the same device blocks), one in each form:
  rag_tokvec_rerank_dev    scores + top-20, on the fp16-form handle and on the 8-bit handle
  rag_retrieve_m3_dev      mode 1 (dense + learned-sparse RRF candidates, three-way score at weights 0.4 / 0.2 / 0.4, top-20) over a
                           64-d index and seeded postings of the same 25,600 rows, on both handles
alternating round by round, and a device-to-device copy timed in the same process (read + write bytes over time). The fp16 arm is
the yardstick: the kernel as it was before the 8-bit form existed. Reported per arm: the median with the fastest and slowest round,
the passage bytes per second (rows x row bytes of the form: 2 dim, or dim + dim / 32 padded to 16) and their fraction of the
measured copy rate; per dim the ratio of the two medians beside the byte floor (33/64 = 0.516 at dim 1024). The 8-bit scores are
compared first with the fp16 arm's (bar (b) of include/rag_hip.h).

Method (as tools/tokvec_time.py): device-pointer entries on resident arrays, device events around `reps` back-to-back calls, one
discarded round, then `--rounds` timed ones. Needs a GPU.

    python tools/tokvec_q8_time.py [--rounds 5] [--out profiles/tokvec_q8.json] [--dims 1024,128]"""
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


def row_bytes(dim, form):
    return 2 * dim if form == "fp16" else (dim + dim // 32 + 15) // 16 * 16


def seeded_postings(rng, n_docs, n_terms, per_doc=16):
    """term-major CSR (indptr int64, doc int32 ascending inside a term, weight float32 > 0): per_doc distinct terms per document"""
    import numpy as np
    term = np.argsort(rng.random((n_docs, n_terms)), axis=1)[:, :per_doc].astype(np.int64).reshape(-1)
    doc = np.repeat(np.arange(n_docs, dtype=np.int32), per_doc)
    order = np.lexsort((doc, term))
    indptr = np.zeros(n_terms + 1, dtype=np.int64)
    np.cumsum(np.bincount(term, minlength=n_terms), out=indptr[1:])
    return indptr, doc[order], (rng.random(order.shape[0]) * 2 + 1e-3).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dims", default="1024,128")
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--candidates", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tokvec_q8.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("tokvec_q8_time: needs a GPU")
    from optimized_rag_amd import RagEngine
    res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds)
    forms = ("fp16", "mxfp8")
    eng = {f: RagEngine(dim=64, device=0) for f in forms}
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
    # the index and the postings of the three-way arm: the same on both handles
    rng = np.random.default_rng(1)
    emb = rng.standard_normal((n_docs, 64)).astype(np.float32)
    indptr, doc, wt = seeded_postings(rng, n_docs, 3000)
    q_terms = np.sort(np.argsort(rng.random((nq, 3000)), axis=1)[:, :8].astype(np.int32), axis=1)     # 8 distinct terms per query, ascending
    ptr = torch.arange(nq + 1, dtype=torch.int32, device="cuda") * 8
    terms, qw = torch.from_numpy(q_terms.reshape(-1)).cuda(), torch.from_numpy((rng.random(nq * 8) * 2 + 1e-3).astype(np.float32)).cuda()
    q_emb = torch.from_numpy((emb[rng.integers(0, n_docs, nq)] + 0.7 * rng.standard_normal((nq, 64))).astype(np.float32)).cuda()
    for f in forms:
        eng[f].index_load(emb)
        eng[f].sparse_load(indptr, doc, wt, n_docs)

    for dim in [int(x) for x in args.dims.split(",")]:
        torch.manual_seed(dim)
        qv = unit(torch.randn((nq * qr, dim), device="cuda"))
        for f in forms:
            eng[f].tokvec_reserve(n_docs, n_docs * dr, dim, form=f)
        block = 256                                                        # documents per append
        off = torch.arange(block + 1, dtype=torch.int64, device="cuda") * dr
        for b in range(0, n_docs, block):
            m = min(block, n_docs - b)
            chunk = unit(torch.randn((m * dr, dim), device="cuda"))
            for f in forms:
                eng[f].tokvec_append_dev(chunk, off[:m + 1].contiguous())
        info = {f: eng[f].tokvec_info() for f in forms}
        for f in forms:
            assert info[f]["n_docs"] == n_docs and info[f]["rows"] == n_docs * dr and eng[f].tokvec_form() == f
        qo = torch.arange(nq + 1, dtype=torch.int64, device="cuda") * qr
        rows = (torch.arange(n_docs, dtype=torch.int32, device="cuda")).reshape(nq, cand).contiguous()
        out = {f: (torch.empty((nq, k), dtype=torch.int64, device="cuda"), torch.empty((nq, k), dtype=torch.float64, device="cuda"),
                   torch.empty((nq, cand), device="cuda")) for f in forms}
        arms = {}
        for f in forms:
            arms[f"tokvec_rerank_dev {f}"] = (lambda f=f: eng[f].tokvec_rerank_dev(qv, qo, rows, k, out[f][0], None, out[f][1], out[f][2]))
            arms[f"retrieve_m3_dev mode 1 {f}"] = (lambda f=f: eng[f].retrieve_m3_dev(q_emb, cand, k, term_ptr=ptr, terms=terms, weights=qw, q_vecs=qv,
                                                                                     q_off=qo, mode=1, w=(0.4, 0.2, 0.4)))
        for fn in arms.values():
            fn()
        torch.cuda.synchronize()
        diff = (out["fp16"][2] - out["mxfp8"][2]).abs().max().item()
        assert diff < 2.0 ** -4 + 2.0 ** -13 + 2e-4, diff
        reps = max(20, 10 * 1024 // dim)                              # at least 0.1 s of work per window
        ms = {name: [] for name in arms}
        for rnd in range(args.rounds + 1):                               # the arms alternate round by round
            for name, fn in arms.items():
                t = window(fn, reps if name.startswith("tokvec") else max(5, reps // 4))
                if rnd > 0:                                              # round 0 settles the clocks after the allocations
                    ms[name].append(t)
        r = {name: summary(v) for name, v in ms.items()}
        for f in forms:
            nbytes = n_docs * dr * row_bytes(dim, f)
            for name in (f"tokvec_rerank_dev {f}", f"retrieve_m3_dev mode 1 {f}"):
                r[name].update(passage_bytes=nbytes, passage_bytes_per_s=nbytes / (r[name]["median_ms"] * 1e-3),
                               fraction_of_measured_copy_rate=nbytes / (r[name]["median_ms"] * 1e-3) / copy_rate)
            r[f"store_hbm_bytes {f}"] = info[f]["hbm_bytes"]
        r["rerank_median_ratio_mxfp8_over_fp16"] = r["tokvec_rerank_dev mxfp8"]["median_ms"] / r["tokvec_rerank_dev fp16"]["median_ms"]
        r["retrieve_m3_median_ratio_mxfp8_over_fp16"] = r["retrieve_m3_dev mode 1 mxfp8"]["median_ms"] / r["retrieve_m3_dev mode 1 fp16"]["median_ms"]
        r["byte_floor_of_the_ratio"] = row_bytes(dim, "mxfp8") / row_bytes(dim, "fp16")
        r["max_abs_score_difference_between_the_forms"] = diff
        r["reps_per_round"] = reps
        r["what"] = f"{nq} queries x {cand} candidates, {qr} query rows, {dr} passage rows, dim {dim}; top-{k} included"
        res[f"dim{dim}"] = r
        print(f"dim {dim}", json.dumps({a: {x: r[a][x] for x in ("median_ms", "min_ms", "max_ms", "fraction_of_measured_copy_rate")} for a in ms}),
              "rerank ratio", round(r["rerank_median_ratio_mxfp8_over_fp16"], 3), "floor", round(r["byte_floor_of_the_ratio"], 3), flush=True)
        del qv
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for e in eng.values():
        e.close()


if __name__ == "__main__":
    main()
