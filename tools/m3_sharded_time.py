"""Times what the SPLIT form of the three-way bge-m3 search costs on one MI355X: world-1 sharded.ShardedM3Index.search_m3 (local
lists, rag_m3_candidates_gathered_dev, rag_m3_score_ids_dev, rag_m3_combine_gathered_dev; no gather at world 1) against the
one-call rag_retrieve_m3_dev on the same handle and index; writes profiles/m3_sharded_world1.json. Multi-GPU scaling cannot be
measured on a one-GPU box: this is the price of the extra launches and of the [4][Q][slots] planes alone.

Shape and method are tools/m3_tenants_time.py's: 256 queries x pool 100 over 25,600 documents (1024-d dense index, 30,000 sparse
terms with 64 per document, 255 token vectors of dim 128 per document; 32 terms and 32 token vectors per query), mode 2, top-20;
device events around `--reps` back-to-back calls after one untimed call, one discarded round, then `--rounds` timed ones with the two
arms alternating and their order reversed every other round; per arm the median with the fastest and slowest beside it. Before
anything is timed the split form's ids, score bits, component bits and candidates are checked against the one call's. Needs a GPU.

    python tools/m3_sharded_time.py [--rounds 5] [--reps 10] [--out profiles/m3_sharded_world1.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from m3_fused_time import postings, summary  # noqa: E402
from m3_tenants_time import window  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "m3_sharded_world1.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("m3_sharded_time: needs a GPU")
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.sharded import ShardedM3Index
    nq, pool, qr, dr, k, q_terms, dim, n_terms, tdim, mode = 256, 100, 32, 255, 20, 32, 1024, 30_000, 128, 2
    n_docs = nq * pool
    res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, reps_per_round=args.reps,
               what=f"{nq} queries x pool {pool}, {n_docs} documents; index dim {dim}, {q_terms} query terms, {qr} query rows and {dr} passage rows "
                    f"of token dim {tdim}; mode {mode} ({2 * pool} slots), top-{k}, weights (0.4, 0.2, 0.4); world 1, no gather")
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
    for b in range(0, n_docs, 256):
        m = min(256, n_docs - b)
        eng.tokvec_append_dev(unit(torch.randn((m * dr, tdim), device="cuda")), off[:m + 1].contiguous())

    def one_call():
        return eng.retrieve_m3_dev(q_emb, pool, k, term_ptr=ptr, terms=terms, weights=qw, q_vecs=qv, q_off=qo, mode=mode)

    def split():
        return ix.search_m3(q_emb, ptr, terms, qw, qv, qo, pool, k, mode=mode)

    exp = [x.clone() for x in one_call()]
    got = split()
    torch.cuda.synchronize()
    for name, e in zip(("ids", "scores", "components", "candidates"), exp):
        g = got[name]
        assert torch.equal(g if g.dtype == torch.int64 else g.view(torch.int64), e if e.dtype == torch.int64 else e.view(torch.int64)), name
    assert (exp[0][:, 0] >= 0).all()

    arms = {"retrieve_m3_dev": one_call, "sharded_search_m3_world1": split}
    ms = {name: [] for name in arms}
    for rnd in range(args.rounds + 1):                                   # round 0 is discarded; the order flips every other round
        for name, fn in (list(arms.items()) if rnd % 2 == 0 else list(arms.items())[::-1]):
            t = window(fn, args.reps)
            if rnd > 0:
                ms[name].append(t)
    r = {name: summary(v) for name, v in ms.items()}
    r["split_over_one_call"] = r["sharded_search_m3_world1"]["median_ms"] / r["retrieve_m3_dev"]["median_ms"]
    r["one_call_spread"] = r["retrieve_m3_dev"]["max_ms"] / r["retrieve_m3_dev"]["min_ms"]
    res["arms"] = r
    print(json.dumps({a: r[a] for a in arms}), flush=True)
    print("split / one call:", round(r["split_over_one_call"], 4), "| one call max / min:", round(r["one_call_spread"], 4), flush=True)
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
