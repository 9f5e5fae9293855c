"""Times one embedding forward of 256 texts x 128 tokens on a 768-wide, 2-layer, ffn 3072 encoder: once with 12 heads of 64 (the
EPI_QKV64 epilogue + ce_attention64_kernel) and once with 24 heads of 32 (the d32 kernels: the same GEMM work, the same attention
FLOPs). Writes profiles/ce_head64.json. No bar: a record of what the 64-wide path costs beside its 32-wide twin.

Method: the device-pointer entry (rag_embed_dev) on resident token arrays, every text full length; each model on a handle of its own;
both warmed up; the two models alternate over `--rounds` rounds, each round timing `--reps` back-to-back forwards per model between
two device events. Per model: the median over rounds of (round time / reps), the fastest and slowest round. Needs a GPU: no fallback.

    python tools/ce_head64_time.py [--rounds 9] [--reps 50] [--out profiles/ce_head64.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEXTS, TOKENS = 256, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ce_head64.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ce_head64_time: needs a GPU")
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.cross_encoder import random_init_tensors

    rng = np.random.default_rng(0)
    ids = torch.from_numpy(rng.integers(1000, 30522, (TEXTS, TOKENS)).astype(np.int32)).cuda()
    tt = torch.zeros_like(ids)
    lens = torch.full((TEXTS,), TOKENS, dtype=torch.int32, device="cuda")
    models = {}
    for heads in (12, 24):
        cfg = dict(vocab_size=30522, hidden=768, layers=2, heads=heads, ffn=3072, max_pos=512, type_vocab=2, eps=1e-12)
        eng = RagEngine(dim=768, device=0)
        eng.embed_load(cfg, random_init_tensors(cfg, seed=3)[:-4], normalize=True)      # the encoder's tensors: no pooler / classifier
        out = torch.empty((TEXTS, 768), dtype=torch.float32, device="cuda")
        models[heads] = (eng, out)

    def forwards(heads, n):
        eng, out = models[heads]
        for _ in range(n):
            eng.embed_dev(ids, tt, lens, out)

    for heads in models:                                     # warm-up: workspaces, code objects, LDS attributes
        forwards(heads, 5)
    torch.cuda.synchronize()
    for heads, (_, out) in models.items():
        assert torch.isfinite(out).all(), heads
    ms = {heads: [] for heads in models}
    for _ in range(args.rounds):
        for heads in models:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            forwards(heads, args.reps)
            b.record()
            b.synchronize()
            ms[heads].append(a.elapsed_time(b) / args.reps)
    res = dict(what="one embedding forward (rag_embed_dev), 256 texts x 128 tokens, hidden 768, 2 layers, ffn 3072; ms per forward",
               device=torch.cuda.get_device_name(0), texts=TEXTS, tokens=TOKENS, rounds=args.rounds, reps_per_round=args.reps)
    for heads, v in ms.items():
        res[f"heads_{heads}_d{768 // heads}"] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), rounds_ms=v)
    res["ratio_d64_over_d32"] = res["heads_12_d64"]["median_ms"] / res["heads_24_d32"]["median_ms"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "what"}))
    for eng, _ in models.values():
        eng.close()


if __name__ == "__main__":
    main()
