"""Times the ingest of learned-sparse postings from DOC-MAJOR device blocks on one MI355X; writes profiles/sparse_ingest.json.

Corpus: the 1M documents / 80.3 M postings of tools/live_resident_time.py (bench_modes.zipf_postings_gpu: Poisson(120) lengths,
Zipf(1.1) tokens over 100,000 terms, seeded float32 weights), also kept doc-major on the device: a block of it is exactly what
rag_lexical_compact_dev leaves there (int32 offsets from 0, terms ascending per document, float32 weights), so no forward is in
any window.

(1) One block of 64 / 256 / 1,000 rows onto an empty tail and onto a tail of 50,000 documents (base: the first 949,000), three arms:
    dev     rag_sparse_append_dev of the doc-major block
    host    rag_sparse_append_host of the same block transposed BEFORE the window: the device transposition against the upload
    parent  what add_texts did before rag_sparse_append_dev: three device-to-host copies of the block, one dict per text,
            LexicalPostings.from_weights, LexicalPostings.extend of the whole host mirror, rag_sparse_append_host
(2) The whole index from nothing: 1,000-row device appends with the default fold policy, against the dicts of every block +
    LexicalPostings.from_weights + rag_sparse_load_host (`--build-host-rounds`: one round is a Python loop over 80 M entries).

Method (tools/live_resident_time.py): the calls are synchronous - wall time around the call, state rebuilt before every round,
one discarded round, then `--rounds`; median with fastest and slowest.

    python tools/sparse_ingest_time.py [--rounds 5] [--parent-rounds 5] [--rows 1000000] [--skip-build] [--out profiles/sparse_ingest.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-rounds", type=int, default=5)
    ap.add_argument("--build-host-rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--skip-build", action="store_true")
    ap.add_argument("--rev", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_ingest.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("sparse_ingest_time: needs a GPU")
    import bench_modes as BM
    from live_resident_time import doc_slice, summary, wall_ms
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.sparse import LexicalPostings
    from sparse_time import commit
    N, V, R = args.rows, 100_000, args.rounds
    device = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0), commit=commit(args.rev), rounds=R, parent_rounds=args.parent_rounds,
               what=f"{N} documents, {V} terms")
    indptr, doc, _, _, _ = BM.zipf_postings_gpu(N, V, 120, device)
    weight = (np.random.default_rng(11).random(doc.shape[0], dtype=np.float32) * np.float32(2.0)) + np.float32(1e-3)
    nnz = int(indptr[-1])
    res["postings"] = dict(nnz=nnz)
    # the doc-major twin on the device (torch as a data generator: outside every window)
    term_d = torch.repeat_interleave(torch.arange(V, device=device), torch.from_numpy(np.diff(indptr)).to(device))
    doc_d = torch.from_numpy(doc).to(device).long()
    order = torch.argsort(doc_d * V + term_d)
    dm_terms = term_d[order].int().contiguous()
    dm_w = torch.from_numpy(weight).to(device)[order].contiguous()
    dm_ptr = torch.zeros(N + 1, dtype=torch.int64, device=device)
    dm_ptr[1:] = torch.cumsum(torch.bincount(doc_d, minlength=N), 0)
    del term_d, doc_d, order
    ptr_h = dm_ptr.cpu().numpy()

    def dev_block(a, b):
        lo, hi = int(ptr_h[a]), int(ptr_h[b])
        return (dm_ptr[a:b + 1] - lo).int().contiguous(), dm_terms[lo:hi], dm_w[lo:hi]

    NB = N - 51_000
    base = doc_slice(indptr, doc, weight, 0, NB)
    base50 = doc_slice(indptr, doc, weight, 0, NB + 50_000)
    tail50 = doc_slice(indptr, doc, weight, NB, NB + 50_000)
    eng = RagEngine(dim=64, device=0)
    eng.set_option("sparse_tail_fold", -1)

    def state(tail):
        eng.sparse_load(*base, NB)
        if tail:
            eng.sparse_append(*tail50, tail)
        return LexicalPostings(*(base50 if tail else base), NB + tail)       # the host mirror of the parent's route (extend replaces its arrays)

    def parent_route(mirror, blk):
        p, t, q = (x.cpu().numpy() for x in blk)
        maps = [dict(zip(t[a:b].tolist(), q[a:b].tolist())) for a, b in zip(p[:-1], p[1:])]
        mirror.append_to(eng, mirror.extend(LexicalPostings.from_weights(maps, V)))

    res["append"] = {}
    for tail in (0, 50_000):
        for rows in (64, 256, 1_000):
            a = NB + tail
            blk = dev_block(a, a + rows)
            csr = doc_slice(indptr, doc, weight, a, a + rows)
            t = dict(dev=[], host=[], parent=[])
            for rnd in range(max(R, args.parent_rounds) + 1):
                if rnd <= R:
                    state(tail)
                    x = wall_ms(lambda: eng.sparse_append_dev(*blk, V))
                    state(tail)
                    y = wall_ms(lambda: eng.sparse_append(*csr, rows))
                    if rnd:
                        t["dev"].append(x), t["host"].append(y)
                if rnd <= args.parent_rounds:
                    mirror = state(tail)
                    z = wall_ms(lambda: parent_route(mirror, blk))
                    if rnd:
                        t["parent"].append(z)
            nb = int(csr[0][-1])
            common = V * 32 + (V + 1) * 8                              # every arm: the new tail's term metadata and offsets go up
            out = {k: summary(v) for k, v in t.items() if v}
            out.update(block_nnz=nb, bytes_per_call=dict(dev=dict(d2h=(V + 2) * 8, h2d=common),
                                                         host=dict(d2h=0, h2d=common + nb * 8 + (V + 1) * 8),
                                                         parent=dict(d2h=(rows + 1) * 4 + nb * 8, h2d=common + nb * 8 + (V + 1) * 8)))
            res["append"][f"{rows}_rows_onto_{tail}_tail"] = out
            print(rows, tail, json.dumps({k: round(v["median_ms"], 3) for k, v in out.items() if isinstance(v, dict) and "median_ms" in v}), flush=True)
    res["append"]["segments"] = eng.sparse_segment_stats()
    eng.sparse_clear()

    if not args.skip_build:
        B = 1_000
        blocks = [dev_block(a, min(N, a + B)) for a in range(0, N, B)]
        eng.set_option("sparse_tail_fold", 0)                         # the default fold policy

        def build_dev():
            eng.sparse_clear()
            for blk in blocks:
                eng.sparse_append_dev(*blk, V)

        def build_host():
            maps = []
            for blk in blocks:
                p, t, q = (x.cpu().numpy() for x in blk)
                maps.extend(dict(zip(t[a:b].tolist(), q[a:b].tolist())) for a, b in zip(p[:-1], p[1:]))
            LexicalPostings.from_weights(maps, V).load(eng)

        td, th = [], []
        for rnd in range(R + 1):
            x = wall_ms(build_dev)
            if rnd:
                td.append(x)
        s = eng.sparse_segment_stats()
        got = eng.sparse_export()
        same = bool(np.array_equal(got["indptr"], indptr) and np.array_equal(got["doc"], doc) and np.array_equal(got["weight"].view(np.int32), weight.view(np.int32)))
        print("build dev", round(float(np.median(td)), 1), "ms; the export equals the corpus CSR:", same, flush=True)
        for rnd in range(args.build_host_rounds + 1 if args.build_host_rounds else 0):
            x = wall_ms(build_host)
            if rnd:
                th.append(x)
            print("build host", round(x, 1), "ms", flush=True)
        res["build"] = dict(device_appends_of_1000_rows=summary(td), segments_after=s, export_equals_corpus=same,
                            dicts_from_weights_load_host=summary(th) if th else None, host_rounds=args.build_host_rounds,
                            bytes=dict(dev_d2h_per_append=(V + 2) * 8, host_d2h_total=(N + len(blocks)) * 4 + nnz * 8, host_h2d_total=nnz * 8 + (V + 1) * 8))
    eng.close()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
