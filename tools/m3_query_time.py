"""Times the bge-m3 query path of GpuDocumentIndex.search_m3_many from query TEXT to result dicts, host-assembled against
device-resident, on one MI355X; writes profiles/m3_query_path.json.

  host    device_query=False, the parent commit's way: encode_multi (forward, synchronise, [Q][L] lexical weights and every token vector
          copied to the host, a Python loop over every token), LexicalPostings.encode_queries, three uploads, rag_retrieve_m3_tenants_dev
  device  device_query=True: tokenise, upload the token ids, ONE call (rag_search_m3_tokens_tenants_dev), copy the results out
Both arms tokenise on the host, end with the same copy of ids, scores and components and build the same result dicts; they are timed
with the wall clock around the whole call (each returns synchronised), at 1 query and at 256 queries.

Shape (tools/m3_tenants_time.py's): 25,600 documents in 16 tenants - a 1024-d dense index, learned-sparse postings (30,000 terms, 64
per document, Zipf-drawn), 255 token vectors per document at token dim 128; pool 100, top-20, candidates "dense+sparse". The embedder
is a seeded XLM-R-large-shaped encoder (hidden 1024, 16 heads of 64, ffn 4096, vocabulary 30,000 = the term space) with a 128-wide
token-vector head and a lexical head, once per entry of `--layers`: 24 layers is bge-m3's depth, 2 layers a forward light enough that
the assembly around it is most of the call. Queries are 8-32 tokens ([CLS] + 6-30 Zipf-drawn words + [SEP]), agent i % 16.

Method: in ONE process, after both arms ran once untimed and their results were compared (the same dicts: rows, order, every score
field ==), `--rounds` + 1 rounds in which the arms run in turn, in reverse order every other round, each arm `reps` calls back to back
per round; round 0 is discarded; per arm the median over rounds of the mean call time, the fastest and slowest round beside it.
Needs a GPU.

    python tools/m3_query_time.py [--rounds 7] [--layers 24,2] [--out profiles/m3_query_path.json]"""
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

CLS, SEP, FIRST_WORD = 0, 2, 4                    # XLM-R's <s>, </s>; words are the ids from 4 on


class WordTokenizer:
    """the part of a `tokenizers.Tokenizer` the embedding service uses, over the words "t<id>": <s> words </s>, truncated"""
    class _Enc:
        def __init__(self, ids):
            self.ids = ids

    def __init__(self):
        self.max_length = 512

    def enable_truncation(self, max_length):
        self.max_length = int(max_length)

    def no_padding(self):
        pass

    def token_to_id(self, t):
        return {"<s>": CLS, "<pad>": 1, "</s>": SEP, "<unk>": 3}.get(t)

    def encode_batch(self, texts):
        return [self._Enc([CLS] + [int(w[1:]) for w in t.split()][:self.max_length - 2] + [SEP]) for t in texts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--layers", default="24,2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "m3_query_path.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("m3_query_time: needs a GPU")
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.cross_encoder import random_init_tensors
    from optimized_rag_amd.document_store import GpuDocumentIndex
    from optimized_rag_amd.embeddings import LocalEmbeddingService
    from optimized_rag_amd.sparse import LexicalPostings
    nq, pool, dr, k, dim, n_terms, T, tdim = 256, 100, 255, 20, 1024, 30_000, 16, 128
    n_docs = nq * pool
    rng = np.random.default_rng(0)
    eng = RagEngine(dim=dim, device=0)

    def service(layers):
        """the embedder with `layers` layers and both heads, loaded on eng (replaces the one before it)"""
        cfg = dict(vocab_size=n_terms, hidden=dim, layers=layers, heads=16, ffn=4096, max_pos=514, type_vocab=2, eps=1e-5, cls_id=CLS, sep_id=SEP)
        svc = LocalEmbeddingService(cfg, random_init_tensors(cfg, seed=3)[:-4], WordTokenizer(), max_length=64, engine=eng, pooling="cls",
                                    model="seeded-xlmr-shape")
        hr = np.random.default_rng(1)
        lw = hr.standard_normal(dim)
        svc.load_heads(dict(tok_w=(hr.standard_normal((tdim, dim)) * 0.05).astype(np.float32), tok_b=np.zeros(tdim, dtype=np.float32),
                            lex_w=(lw / np.abs(lw).sum()).astype(np.float32), lex_b=0.01))
        return svc

    depths = [int(x) for x in args.layers.split(",")]
    svc = service(depths[0])
    index = GpuDocumentIndex(svc, dim=dim, engine=eng)
    torch.manual_seed(0)
    index.bulk_load([dict(content=f"d{i}", agent_id=f"agent{i // (n_docs // T)}") for i in range(n_docs)], torch.randn((n_docs, dim)).numpy())
    indptr, doc, w, p = postings(rng, n_docs, n_terms, 64)
    index.load_lexical(LexicalPostings(indptr, doc, w, n_docs))
    unit = lambda t: torch.nn.functional.normalize(t, dim=-1)
    eng.tokvec_reserve(n_docs, n_docs * dr, tdim)
    off = torch.arange(257, dtype=torch.int64, device="cuda") * dr
    for b in range(0, n_docs, 256):
        m = min(256, n_docs - b)
        eng.tokvec_append_dev(unit(torch.randn((m * dr, tdim), device="cuda")), off[:m + 1].contiguous())
    pw = p[FIRST_WORD:] / p[FIRST_WORD:].sum()
    queries = [" ".join(f"t{t}" for t in FIRST_WORD + rng.choice(n_terms - FIRST_WORD, int(rng.integers(6, 31)), p=pw)) for _ in range(nq)]
    agents = [f"agent{i % T}" for i in range(nq)]
    q_tokens = [len(q.split()) + 2 for q in queries]

    calls = dict(one=0)
    one_call = eng.search_m3_tokens_dev

    def counted(*a, **kw):
        calls["one"] += 1
        return one_call(*a, **kw)

    eng.search_m3_tokens_dev = counted
    kw = dict(top_k=k, pool=pool, candidates="dense+sparse")
    arm = lambda n, device: (lambda: index.search_m3_many(agents[:n], queries[:n], device_query=device, **kw))
    res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds,
               what=f"search_m3_many, text in / dicts out: {n_docs} documents in {T} tenants, index dim {dim}, {n_terms} terms x 64 per document, {dr} "
                    f"passage rows of token dim {tdim}; pool {pool}, top-{k}, candidates dense+sparse; embedder hidden {dim}, 16 heads, ffn 4096; "
                    f"queries of {min(q_tokens)}-{max(q_tokens)} tokens, one agent per query; wall clock around the whole call",
               runs=[])
    for layers in depths:
        if layers != depths[0]:
            index.embeddings = service(layers)
        run = dict(layers=layers, arms={})
        for n, reps in ((1, 60), (nq, 16)):                               # windows of about a third of a second
            host, device = arm(n, False), arm(n, True)
            a, before = host(), calls["one"]
            b = device()
            assert calls["one"] == before + 1, "the device arm did not take the one-call path"
            assert len(a) == n and all(len(x) == k and "colbert_score" in x[0] for x in a), "the host arm fell back to the plain search"
            identical = a == b
            assert identical, "the two arms disagree"
            ms = dict(host=[], device=[])
            for rnd in range(args.rounds + 1):                           # round 0 is discarded; the order flips every other round
                for name, fn in ((("host", host), ("device", device)) if rnd % 2 == 0 else (("device", device), ("host", host))):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        fn()
                    t = (time.perf_counter() - t0) * 1e3 / reps
                    if rnd > 0:
                        ms[name].append(t)
            r = {name: summary(v) for name, v in ms.items()}
            r.update(queries=n, reps_per_round=reps, host_over_device=r["host"]["median_ms"] / r["device"]["median_ms"],
                     identical_ids_and_score_bits=bool(identical))
            run["arms"][f"{n}_queries"] = r
            print(f"{layers} layers, {n} queries: host {r['host']['median_ms']:.3f} ms, device {r['device']['median_ms']:.3f} ms, host / device "
                  f"{r['host_over_device']:.3f}, identical {identical}", flush=True)
        res["runs"].append(run)
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
