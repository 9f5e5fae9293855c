"""Times the embedder's token-vector and lexical heads and the MaxSim kernel on one MI355X; writes profiles/m3_heads.json.

(a) The cost of the heads: rag_embed_multi_dev with all three outputs (tok_dim 1024 + the lexical head) against rag_embed_dev on the
    same 65,536 tokens (256 texts of 256) of the 1024-wide, 16-head, 2-layer, ffn 4096 encoder of tools/ce_long_time.py, the two
    alternating in one process.
(b) rag_maxsim_dev: 256 queries x 100 candidates, 32 query rows, 255 passage rows, dim 1024. Its floor is the passage bytes
    (25,600 x 255 x 1024 x 4 B = 26.7 GB, a product of sizes); reported beside it: the device's copy rate measured here (a 4 GiB
    device-to-device copy, read + write bytes over time) and the fraction of that rate the kernel reaches on the passage bytes.

Method: device-pointer entries on resident arrays, device events around `--reps` back-to-back calls, one discarded round, then
`--rounds` timed ones; per arm the median over rounds with the fastest and slowest round beside it. Needs a GPU: no fallback.

    python tools/m3_time.py [--rounds 5] [--reps 10] [--out profiles/m3_heads.json] [--candidates 100]"""
import argparse
import json
import os
import statistics
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


def timed(fn, reps, rounds):
    """rounds + 1 windows, the first discarded -> ms per call of every timed round"""
    return [window(fn, reps) for _ in range(rounds + 1)][1:]


def summary(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), rounds_ms=v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--candidates", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "m3_heads.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("m3_time: needs a GPU")
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.cross_encoder import random_init_tensors
    res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, reps_per_round=args.reps)

    # ---- (a) the heads beside the forward
    cfg = dict(vocab_size=8000, hidden=1024, layers=2, heads=16, ffn=4096, max_pos=512, type_vocab=2, eps=1e-12)
    eng = RagEngine(dim=1024, device=0)
    eng.embed_load(cfg, random_init_tensors(cfg, seed=3)[:-4], normalize=True, pooling="cls")
    rng = np.random.default_rng(0)
    lw = rng.standard_normal(1024)
    eng.embed_heads_load(tok_w=(rng.standard_normal((1024, 1024)) * 0.05).astype(np.float32), tok_b=np.zeros(1024, dtype=np.float32),
                         lex_w=(lw / np.abs(lw).sum()).astype(np.float32), lex_b=0.0)
    texts, L = 256, 256
    ids = torch.from_numpy(rng.integers(1000, cfg["vocab_size"], (texts, L)).astype(np.int32)).cuda()
    tt = torch.zeros_like(ids)
    lens = torch.full((texts,), L, dtype=torch.int32, device="cuda")
    rows = texts * (L - 1)
    dense0 = torch.empty((texts, 1024), device="cuda")
    dense1, lex = torch.empty((texts, 1024), device="cuda"), torch.empty((texts, L), device="cuda")
    tok, off = torch.empty((rows, 1024), device="cuda"), torch.empty((texts + 1,), dtype=torch.int64, device="cuda")
    plain = lambda: eng.embed_dev(ids, tt, lens, dense0)
    multi = lambda: eng.embed_multi_dev(ids, tt, lens, dense=dense1, lex=lex, tok=tok, row_off=off)
    for _ in range(2):
        plain()
        multi()
    torch.cuda.synchronize()
    assert torch.equal(dense0, dense1) and int(off[-1]) == rows and torch.isfinite(tok).all()
    ms = {"embed_dev": [], "embed_multi_dev": []}
    for rnd in range(args.rounds + 1):                           # the arms alternate round by round
        for name, fn in (("embed_dev", plain), ("embed_multi_dev", multi)):
            t = window(fn, args.reps)
            if rnd > 0:                                          # round 0 settles the clocks after the allocations
                ms[name].append(t)
    a = {k: summary(v) for k, v in ms.items()}
    a["heads_ms"] = a["embed_multi_dev"]["median_ms"] - a["embed_dev"]["median_ms"]
    a["heads_share_of_forward"] = a["heads_ms"] / a["embed_dev"]["median_ms"]
    a["what"] = f"{texts} texts of {L} tokens, hidden 1024, 16 heads of 64, 2 layers, ffn 4096; heads: tok_dim 1024 + lexical"
    res["heads"] = a
    print("heads", json.dumps({k: v for k, v in a.items() if k in ("heads_ms", "heads_share_of_forward")}),
          {k: round(a[k]["median_ms"], 3) for k in ms}, flush=True)
    eng.embed_load(cfg, random_init_tensors(cfg, seed=3)[:-4], normalize=True)            # frees the heads' scratch
    del tok, lex, dense0, dense1

    # ---- the device's copy rate, measured here
    n = 1 << 30
    src, dst = torch.empty(n, dtype=torch.float32, device="cuda").normal_(), torch.empty(n, dtype=torch.float32, device="cuda")
    v = timed(lambda: dst.copy_(src), 5, args.rounds)
    copy_rate = 2 * 4 * n / (statistics.median(v) * 1e-3)
    res["copy"] = dict(bytes_moved=2 * 4 * n, **summary(v), bytes_per_s=copy_rate)
    print("copy rate GB/s", round(copy_rate / 1e9, 1), flush=True)
    del src, dst

    # ---- (b) MaxSim
    nq, cand, qr, dr, dim = 256, args.candidates, 32, 255, 1024
    unit = lambda t: torch.nn.functional.normalize(t, dim=-1)
    qv = unit(torch.randn((nq * qr, dim), device="cuda"))
    dv = torch.empty((nq * cand * dr, dim), device="cuda")
    step = 1 << 18
    for s in range(0, dv.shape[0], step):
        dv[s:s + step] = unit(torch.randn((min(step, dv.shape[0] - s), dim), device="cuda"))
    qo = torch.arange(nq + 1, dtype=torch.int64, device="cuda") * qr
    do = torch.arange(nq * cand + 1, dtype=torch.int64, device="cuda") * dr
    pq = torch.arange(nq * cand, dtype=torch.int32, device="cuda") // cand
    pd = torch.arange(nq * cand, dtype=torch.int32, device="cuda")
    out = torch.empty((nq * cand,), device="cuda")
    run = lambda: eng.maxsim_dev(qv, qo, dv, do, pq, pd, out)
    run()
    torch.cuda.synchronize()
    want = (qv[:qr].double() @ dv[:dr].double().T).max(1).values.mean().item()
    assert abs(out[0].item() - want) < 1e-4, (out[0].item(), want)
    v = timed(run, max(1, args.reps // 3), args.rounds)
    d_bytes = dv.numel() * 4
    b = summary(v)
    b.update(what=f"{nq} queries x {cand} candidates, {qr} query rows, {dr} passage rows, dim {dim}", passage_bytes=d_bytes,
             passage_bytes_per_s=d_bytes / (b["median_ms"] * 1e-3),
             fraction_of_measured_copy_rate=d_bytes / (b["median_ms"] * 1e-3) / copy_rate,
             floor_ms_at_8TBps=d_bytes / 8e12 * 1e3, mfma_flop=3 * 2.0 * nq * cand * qr * dr * dim)
    res["maxsim"] = b
    print("maxsim", json.dumps({k: b[k] for k in ("median_ms", "min_ms", "max_ms", "passage_bytes_per_s", "fraction_of_measured_copy_rate")}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    eng.close()


if __name__ == "__main__":
    main()
