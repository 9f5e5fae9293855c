"""Times the per-query-tenant forms of the learned-sparse search and of the three-way bge-m3 composite on one MI355X; writes
profiles/m3_tenants.json.

Shape (tools/m3_fused_time.py's): 256 queries x pool 100 over 25,600 documents - a 1024-d dense index, learned-sparse postings
(30,000 terms, 64 per document, Zipf-drawn), 255 token vectors per document at token dim 128; a query has 32 token vectors and 32
weighted terms. The documents belong to 16 tenants, 1,600 consecutive rows each; query i belongs to tenant i % 16. In ONE process,
the arms alternating round by round:
  (a) a MIXED batch through rag_retrieve_m3_tenants_dev (mode 1, top-20) and rag_sparse_topk_tenants_dev (top-100), against the
      only correct form before these entries existed: a loop of scalar-tenant calls, one per distinct tenant over its 16 queries;
  (b) a UNIFORM array (every query tenant 3) against the scalar entry with tenant = 3: the same path by routing.
Before anything is timed the mixed batch's ids are checked against the loop's.

Two comparisons against the parent commit need its build and therefore other processes; their results are merged in by name:
  --sparse-runs parent=FILE change=FILE ...   profiles written by tools/sparse_time.py on either tree, in the order they were run
  --bench-runs parent=FILE change=FILE ...    files holding the JSON line of `bench.py --gpus 1 --steps 20 --warmup 3`

Method (as tools/multi_tenant_probe.py and tools/m3_fused_time.py): device-pointer entries on resident arrays, device events around
`--reps` back-to-back calls after one untimed call, one discarded round, then `--rounds` timed ones in which the arms run in
turn, in reverse order every other round (so that neither arm of a pair always follows the other); per arm the median with the
fastest and slowest beside it. Needs a GPU.

    python tools/m3_tenants_time.py [--rounds 5] [--reps 10] [--out profiles/m3_tenants.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from m3_fused_time import postings, summary  # noqa: E402


def window(fn, reps):
    """one untimed call (the arm before it ran other batch sizes and tenants), then fn() `reps` times between two device
    events -> ms per call"""
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def labelled(items):
    out = []
    for it in items or []:
        label, _, path = it.partition("=")
        out.append((label, path))
    return out


def last_json_line(path):
    with open(path) as f:
        lines = [ln for ln in f.read().splitlines() if ln.lstrip().startswith("{")]
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tenants", type=int, default=16)
    ap.add_argument("--token-dim", type=int, default=128)
    ap.add_argument("--sparse-runs", nargs="*")
    ap.add_argument("--bench-runs", nargs="*")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "m3_tenants.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("m3_tenants_time: needs a GPU")
    from optimized_rag_amd import RagEngine
    nq, pool, qr, dr, k, q_terms, dim, n_terms, T, tdim = 256, 100, 32, 255, 20, 32, 1024, 30_000, args.tenants, args.token_dim
    n_docs = nq * pool
    res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, reps_per_round=args.reps,
               what=f"{nq} queries x pool {pool}, {n_docs} documents in {T} tenants of {n_docs // T} consecutive rows, query i under tenant i % {T}; "
                    f"index dim {dim}, {q_terms} query terms, {qr} query rows and {dr} passage rows of token dim {tdim}; m3 mode 1 top-{k}, sparse top-{pool}")
    rng = np.random.default_rng(0)
    eng = RagEngine(dim=dim, device=0)
    unit = lambda t: torch.nn.functional.normalize(t, dim=-1)
    torch.manual_seed(0)
    emb = torch.randn((n_docs, dim))
    eng.index_load(emb.numpy())
    eng.set_tenants((np.arange(n_docs) // (n_docs // T)).astype(np.int32))
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

    mixed = (np.arange(nq) % T).astype(np.int32)
    uniform = np.full(nq, 3, dtype=np.int32)
    # the scalar loop's inputs: every tenant's queries as a batch of their own, prepared once
    subs = []
    for t in range(T):
        sel = torch.from_numpy(np.nonzero(mixed == t)[0]).cuda()
        n = sel.shape[0]
        tsel = (sel[:, None] * q_terms + torch.arange(q_terms, device="cuda")[None]).reshape(-1)
        vsel = (sel[:, None] * qr + torch.arange(qr, device="cuda")[None]).reshape(-1)
        subs.append(dict(t=t, sel=sel, q=q_emb[sel].contiguous(), ptr=ptr[:n + 1].contiguous(), terms=terms[tsel].contiguous(), qw=qw[tsel].contiguous(),
                         qv=qv[vsel].contiguous(), qo=qo[:n + 1].contiguous(),
                         ids=torch.empty((n, pool), dtype=torch.int64, device="cuda"), sc=torch.empty((n, pool), dtype=torch.float64, device="cuda")))
    s_ids = torch.empty((nq, pool), dtype=torch.int64, device="cuda")
    s_sc = torch.empty((nq, pool), dtype=torch.float64, device="cuda")

    def m3(tenant):
        return eng.retrieve_m3_dev(q_emb, pool, k, term_ptr=ptr, terms=terms, weights=qw, q_vecs=qv, q_off=qo, mode=1, tenant=tenant)

    def m3_loop():
        for s in subs:
            eng.retrieve_m3_dev(s["q"], pool, k, term_ptr=s["ptr"], terms=s["terms"], weights=s["qw"], q_vecs=s["qv"], q_off=s["qo"], mode=1, tenant=s["t"])

    def sparse(tenant):
        eng.sparse_topk_dev(ptr, terms, qw, pool, s_ids, None, s_sc, tenant=tenant)

    def sparse_loop():
        for s in subs:
            eng.sparse_topk_dev(s["ptr"], s["terms"], s["qw"], pool, s["ids"], None, s["sc"], tenant=s["t"])

    # the mixed batch returns what the loop returns
    got = m3(mixed)[0].clone()
    sparse(mixed)
    sparse_loop()
    torch.cuda.synchronize()
    for s in subs:
        part = eng.retrieve_m3_dev(s["q"], pool, k, term_ptr=s["ptr"], terms=s["terms"], weights=s["qw"], q_vecs=s["qv"], q_off=s["qo"], mode=1, tenant=s["t"])[0]
        assert torch.equal(got[s["sel"]], part) and torch.equal(s_ids[s["sel"]], s["ids"]), "the mixed batch and the scalar loop disagree"
    assert (got[:, 0] >= 0).all()

    arms = {"retrieve_m3_tenants_dev_mixed": lambda: m3(mixed), "retrieve_m3_dev_scalar_loop": m3_loop,
            "sparse_topk_tenants_dev_mixed": lambda: sparse(mixed), "sparse_topk_dev_scalar_loop": sparse_loop,
            "retrieve_m3_tenants_dev_uniform": lambda: m3(uniform), "retrieve_m3_dev_scalar": lambda: m3(3),
            "sparse_topk_tenants_dev_uniform": lambda: sparse(uniform), "sparse_topk_dev_scalar": lambda: sparse(3)}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in arms}
    for rnd in range(args.rounds + 1):                                   # the arms alternate round by round, in reverse order every
        for name, fn in (list(arms.items()) if rnd % 2 == 0 else list(arms.items())[::-1]):      # other round; round 0 is discarded
            t = window(fn, args.reps)
            if rnd > 0:
                ms[name].append(t)
    r = {name: summary(v) for name, v in ms.items()}
    ratio = lambda a, b: r[a]["median_ms"] / r[b]["median_ms"]
    r["m3_mixed_over_scalar_loop"] = ratio("retrieve_m3_tenants_dev_mixed", "retrieve_m3_dev_scalar_loop")
    r["sparse_mixed_over_scalar_loop"] = ratio("sparse_topk_tenants_dev_mixed", "sparse_topk_dev_scalar_loop")
    r["m3_uniform_over_scalar"] = ratio("retrieve_m3_tenants_dev_uniform", "retrieve_m3_dev_scalar")
    r["sparse_uniform_over_scalar"] = ratio("sparse_topk_tenants_dev_uniform", "sparse_topk_dev_scalar")
    r["m3_scalar_spread"] = r["retrieve_m3_dev_scalar"]["max_ms"] / r["retrieve_m3_dev_scalar"]["min_ms"]
    r["sparse_scalar_spread"] = r["sparse_topk_dev_scalar"]["max_ms"] / r["sparse_topk_dev_scalar"]["min_ms"]
    res["arms"] = r
    print(json.dumps({a: round(r[a]["median_ms"], 4) for a in arms}), flush=True)
    print("mixed / loop: m3", round(r["m3_mixed_over_scalar_loop"], 3), "sparse", round(r["sparse_mixed_over_scalar_loop"], 3),
          "| uniform / scalar: m3", round(r["m3_uniform_over_scalar"], 4), "sparse", round(r["sparse_uniform_over_scalar"], 4),
          "| scalar max / min: m3", round(r["m3_scalar_spread"], 4), "sparse", round(r["sparse_scalar_spread"], 4), flush=True)
    eng.close()

    runs = labelled(args.sparse_runs)
    if runs:                                                             # the scalar sparse arm of tools/sparse_time.py, parent and change alternating
        rows = [dict(tree=label, commit=d.get("commit"), **{a: d[sec][a] for sec, a in (("topk", "sparse_topk_dev"), ("hybrid", "hybrid_sparse_rrf_dev"))})
                for label, d in ((label, json.load(open(path))) for label, path in runs)]
        res["scalar_sparse_against_parent"] = dict(runs=rows, what="tools/sparse_time.py, one process per run, in this order")
    runs = labelled(args.bench_runs)
    if runs:
        res["bench_headline_against_parent"] = dict(runs=[dict(tree=label, line=last_json_line(path)) for label, path in runs],
                                                    what="python bench.py --gpus 1 --steps 20 --warmup 3, one process per run, in this order")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
