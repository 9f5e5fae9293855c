"""Times the two attention forms of the length classes above 512 against each other: one embedding forward of a 1024-wide, 16-head
(64-wide heads), 2-layer, ffn 4096 encoder at seq_len 768, 1024, 1536, 2048, 4096 and 8192, every case about 65,536 tokens of
full-length texts (85, 64, 42, 32, 16 and 8 texts), once with the streamed form of ce_attention64_kernel (option ce_attn_stream = 1: streamed at every class above
512) and once with the DIRECT form (-1). Writes profiles/ce_long_seq.json. The GEMMs, LayerNorms and pooling are the same launches
in both arms, so the difference of the two forward times is the difference of the attention kernels.

Method: the device-pointer entry (rag_embed_dev) on resident token arrays, one handle; per case both forms are warmed up (workspace,
code objects, LDS attribute) and checked to return the same bits, then alternate over one discarded and `--rounds` timed rounds, each
round timing `--reps` back-to-back forwards per form between two device events (a quarter of a second or more per window). Per form: the median over rounds of (round time / reps), the fastest and
slowest round. A form wins a class when the medians differ by more than the larger of the two spreads (slowest - fastest round).
Needs a GPU: no fallback.

    python tools/ce_long_time.py [--rounds 7] [--reps 20] [--out profiles/ce_long_seq.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOKENS = 65536
SEQ_LENS = (768, 1024, 1536, 2048, 4096, 8192)
FORMS = {"streamed": 1, "direct": -1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ce_long_seq.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ce_long_time: needs a GPU")
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.cross_encoder import random_init_tensors

    cfg = dict(vocab_size=8000, hidden=1024, layers=2, heads=16, ffn=4096, max_pos=8192, type_vocab=2, eps=1e-12)
    eng = RagEngine(dim=1024, device=0)
    eng.embed_load(cfg, random_init_tensors(cfg, seed=3)[:-4], normalize=True)          # the encoder's tensors: no pooler / classifier
    rng = np.random.default_rng(0)
    res = dict(what="one embedding forward (rag_embed_dev), about 65,536 tokens of full-length texts, hidden 1024, 16 heads of 64, 2 layers, "
                    "ffn 4096; ms per forward with the streamed (ce_attn_stream = 1) and the DIRECT (-1) attention form",
               device=torch.cuda.get_device_name(0), tokens=TOKENS, rounds=args.rounds, reps_per_round=args.reps, cases={})
    try:
        for L in SEQ_LENS:
            texts = TOKENS // L
            ids = torch.from_numpy(rng.integers(1000, cfg["vocab_size"], (texts, L)).astype(np.int32)).cuda()
            tt = torch.zeros_like(ids)
            lens = torch.full((texts,), L, dtype=torch.int32, device="cuda")
            outs = {f: torch.empty((texts, 1024), dtype=torch.float32, device="cuda") for f in FORMS}

            def forwards(form, n):
                eng.set_option("ce_attn_stream", FORMS[form])
                for _ in range(n):
                    eng.embed_dev(ids, tt, lens, outs[form])

            for form in FORMS:
                forwards(form, 2)
            torch.cuda.synchronize()
            assert torch.isfinite(outs["streamed"]).all() and torch.equal(outs["streamed"], outs["direct"]), L
            ms = {form: [] for form in FORMS}
            for rnd in range(args.rounds + 1):
                for form in FORMS:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    forwards(form, args.reps)
                    b.record()
                    b.synchronize()
                    if rnd > 0:                              # round 0 settles the clocks after the case's allocations
                        ms[form].append(a.elapsed_time(b) / args.reps)
            case = dict(texts=texts)
            for form, v in ms.items():
                case[form] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), rounds_ms=v)
            gap = case["direct"]["median_ms"] - case["streamed"]["median_ms"]
            spread = max(case[f]["max_ms"] - case[f]["min_ms"] for f in FORMS)
            case["direct_minus_streamed_ms"], case["spread_ms"] = gap, spread
            case["faster"] = "undecided" if abs(gap) <= spread else ("streamed" if gap > 0 else "direct")
            res["cases"][f"seq_len_{L}"] = case
            print(L, json.dumps({k: v for k, v in case.items() if k in ("direct_minus_streamed_ms", "spread_ms", "faster")}),
                  {f: round(case[f]["median_ms"], 3) for f in FORMS}, flush=True)
    finally:
        eng.set_option("ce_attn_stream", 0)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    eng.close()


if __name__ == "__main__":
    main()
