"""Stream ordering of the device-pointer (`*_dev`) entries added after tests/test_stream_order_gpu.py was written: the
learned-sparse index, the token-vector store, the three-way bge-m3 score, the per-query-tenant forms, the steps of the row-sharded
searches and the id map. The regimes are that file's (include/rag_hip.h, "Ordering"): every call runs on a non-default stream
behind stream_tools.busy, its inputs arrive late, and every result is compared bit for bit with the same call made alone and
synchronously on a fresh handle. The inputs that are "not there yet" are legal values (zero queries, empty term lists, -1
candidate slots, all-zero q_off, token id 0 with length 1, gathered blocks of -1 ids with owned flags 0): a mis-ordered read
gives unequal arrays, never an out-of-range access. test_three_calls_back_to_back_behind_busy_work also asserts that those
inputs give another answer than the real ones, so that a read of the wrong ones cannot pass unseen.

World (built once per process from the generators of sparse_tools, tokvec_tools and m3_tools; m3_fused_tools.world() is fixed at
10,300 rows of 0-39 token vectors, so the generators it calls are called with the numbers below instead): 5000 rows = three keyword
ranges of 2048 documents and 20 dense tiles; dim 64 (128 on the handles whose embedder writes the query vectors: the embedder of
tests/test_m3_query_gpu.py has hidden 128); 1-12 token vectors of width 64 per document; learned-sparse vocabulary 1600; tenants
0..2; 40 queries, 300 for the dense-backed composites (their query tiling starts at 256); pool 50, k 10.

Every case names the `*_dev` entries it must reach (ENTRIES); the late-producer test records the entries the wrapper really
called and compares. tests/test_stream_order_table_cpu.py holds that table against the declarations of include/rag_hip.h.

Measured on an MI355X, one run (also in DESIGN.md section 4.7). The file: 101 tests in 30 s, none above 2.2 s. Host-side enqueue
cost of the slowest new call (rag_search_m3_tokens_dev, mode 2, 40 queries): 0.30 ms against 209.9 ms of busy work, so the busy
time stays at stream_tools.BUSY_MS for every case; test_enqueue_cost_is_small_against_the_busy_time measures both again and
asserts the 10x ratio. Every test passed on the library as it stood: no ordering bug was found.

Mutants, one line each, a launch, clear or copy moved from the caller's stream to the handle's private stream, built aside and
run once against the narrowest test:
  m3_own_rows_kernel in m3_score_ids_dev     FAILS test_late_producer...[m3_score_ids_dev-implicit_ids] (80 % of the block)
  idmap_lookup_kernel in idmap_rows_of_ids   FAILS test_late_producer...[rows_of_ids_dev] (every row)
  hipMemsetAsync of max_key in linear_scores FAILS test_two_different_batches_back_to_back[hybrid_linear_tenants_dev] (16 % of the
                                             keyword plane). max_key is reduced with atomicMax: a clear that runs early shows only
                                             when the batch before left a larger maximum in a slot, so by that argument the
                                             late-producer and three-call cases cannot catch it (reasoned, not run)
  the upload of the per-query tenants (qten) FAILS the same test (78 %)
None survived. Not run: any mutant against the whole file.
"""
import contextlib
import time

import numpy as np
import pytest

import m3_tools as M
import sparse_tools as S
import stream_tools as T
import test_stream_order_gpu as A
import tokvec_tools as V

pytestmark = pytest.mark.gpu

Case = A.Case                                    # (parts, options, wrong, real, bind)
out = A.out
N, D, DE, TOK, VS = 5000, 64, 128, 64, 1600      # rows, index dim, embedder hidden (the dim of the token-id handles), token-vector dim, sparse vocabulary
Q, QBIG, POOL, K = 40, 300, 50, 10
W3 = (0.4, 0.2, 0.4)
CFG = dict(vocab_size=500, hidden=128, layers=2, heads=2, ffn=256, max_pos=128, type_vocab=2, eps=1e-12)     # tests/test_m3_query_gpu.py
LT, CLS, SEP = 40, 1, 2
SKIP = (0, CLS, SEP, 3)
BOUNDS = ((0, 2100), (2100, 4970), (4970, N))    # three unequal shards; the last holds fewer rows than the pool
ENQUEUE_MS_SLOWEST = T.BUSY_MS / 10
_W = {}


def sparse_queries(indptr, rng):
    """Q weighted queries in the shapes of sparse_tools.make_queries (which needs terms of 1-3 postings: a corpus of 5000
    documents over 600 live terms has none): one of 70 terms (past the 64 planned slots), 33 of 1-12 Zipf-drawn terms, and an
    empty one, one outside the vocabulary, a term with an empty list, a repeated term, zero and NaN weights, the three longest
    lists"""
    live = VS - S.N_EMPTY
    p = np.arange(1, live + 1, dtype=np.float64) ** -1.1
    p /= p.sum()
    by_df = np.argsort(-np.diff(indptr), kind="stable")
    wts = lambda n: (rng.random(n) * 2.0).astype(np.float32) + np.float32(1e-3)
    qs = [(rng.choice(live, 70, replace=False, p=p), wts(70))]
    for _ in range(Q - 7):
        n = int(rng.integers(1, 13))
        qs.append((rng.choice(live, n, replace=False, p=p), wts(n)))
    qs.append((np.zeros(0, np.int32), np.zeros(0, np.float32)))
    qs.append((np.array([-1, VS, VS + 5, -7]), wts(4)))
    qs.append((np.array([VS - 1]), wts(1)))
    qs.append((np.array([int(by_df[50]), int(by_df[300]), int(by_df[50])]), wts(3)))
    qs.append((by_df[[10, 400, 20, 500]], np.array([0.0, 1.25, np.nan, 0.5], dtype=np.float32)))
    qs.append((by_df[[0, 1, 2]], wts(3)))
    assert len(qs) == Q
    return qs


def world():
    if _W:
        return _W
    from optimized_rag_amd.bm25 import Bm25Postings
    rng = np.random.default_rng(4747)
    w = {}
    w["emb"] = rng.standard_normal((N, DE)).astype(np.float32)
    w["q"] = (w["emb"][rng.integers(0, N, QBIG)] + 0.4 * rng.standard_normal((QBIG, DE))).astype(np.float32)
    docs = rng.integers(0, 400, (N, 12))
    w["corpus"] = [" ".join(f"t{t}" for t in d) for d in docs]
    w["post"] = Bm25Postings.from_corpus(w["corpus"])
    w["queries"] = [" ".join([f"t{t}" for t in docs[int(rng.integers(0, N))]][:11] + ["zzz"]) for _ in range(QBIG)]
    w["temporal"] = rng.random(N)
    w["tenants"] = (np.arange(N) % 3).astype(np.int32)
    w["tenant_q"] = np.array([0, 1, 2, -1, 5] * (QBIG // 5), np.int32)           # 5 owns no row, -1 is not filtered
    w["ids"] = (5000 + 3 * np.arange(N)).astype(np.int64)
    w["csr"] = S.make_corpus(n_docs=N, n_terms=VS, seed=5)
    base = sparse_queries(w["csr"][0], rng)
    w["sq"] = [base[i % Q] for i in range(QBIG)]
    counts = rng.integers(1, 13, N)
    w["d_vecs"] = V.unit_rows(rng, int(counts.sum()), TOK)
    w["d_off"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    qc = rng.integers(1, 21, Q)
    qc[3] = 0                                                                    # a query without token vectors
    qlist = [V.unit_rows(rng, int(c), TOK) for c in qc]
    w["qlist"] = [qlist[i % Q] for i in range(QBIG)]
    lens = rng.integers(1, LT + 1, Q).astype(np.int32)
    lens[:3] = (2, 1, LT)                                                        # [CLS] [SEP] alone, a single token, the full length
    tid = rng.integers(4, 200, (Q, LT)).astype(np.int32)
    tid[:, 0] = CLS
    for i, n in enumerate(lens):
        tid[i, n - 1] = SEP if n > 1 else CLS
        tid[i, n:] = 0
    w["tid"], w["tlen"] = tid, lens
    w["tok"] = rng.integers(200, 2000, (N, 20)).astype(np.int32)
    w["tok_len"] = rng.integers(3, 21, N).astype(np.int32)
    _W.update(w)
    return _W


def models():
    """the seeded encoders (built on first use: only the model-backed cases need them)"""
    w = world()
    if "enc_t" not in w:
        from optimized_rag_amd.cross_encoder import flatten_state_dict
        from oracle import bert_oracle as B
        w["enc_t"] = flatten_state_dict(B.seeded_weights(CFG, 21), CFG["layers"], head=False)
        w["heads"], w["heads2"] = M.seeded_heads(DE, TOK, 6), M.seeded_heads(DE, TOK, 7)
        w["ce_t"] = flatten_state_dict(B.seeded_weights(A.CE_CFG, 11), A.CE_CFG["layers"])
    return w


class Spy:
    """the library of one handle, recording the device-pointer entries called through it"""

    def __init__(self, lib, seen):
        self._lib, self._seen = lib, seen

    def __getattr__(self, name):
        if name.startswith("rag_") and name.endswith("_dev"):
            self._seen.add(name)
        return getattr(self._lib, name)


def load(eng, parts, lo=0, hi=N):
    """the named parts of world() over rows [lo, hi) (a shard is loaded under id_base = lo)"""
    from optimized_rag_amd.sparse import LexicalPostings
    w = world()
    dim = eng.dim
    emb = np.ascontiguousarray(w["emb"][lo:hi, :dim])
    if "ids" in parts:
        eng.index_load(emb, ids=np.array(w["ids"][lo:hi]))
        eng.index_id_map()
    elif "index" in parts:
        eng.index_load(emb, id_base=lo)
    if "tenants" in parts:
        eng.set_tenants(np.array(w["tenants"][lo:hi]))
    if "bm25" in parts:
        w["post"].load(eng)
    if "temporal" in parts:
        eng.set_temporal(np.array(w["temporal"][lo:hi]))
    if "sparse" in parts:
        LexicalPostings(*w["csr"], N).shard(lo, hi).load(eng)
    for name, form in (("tokvec", "fp16"), ("tokvec8", "mxfp8")):
        if name in parts:
            off = w["d_off"]
            eng.tokvec_load(np.array(w["d_vecs"][off[lo]:off[hi]]), (off[lo:hi + 1] - off[lo]).astype(np.int64), form=form)
    if "embedder" in parts:
        m = models()
        eng.embed_load(CFG, m["enc_t"], normalize=True, pooling="cls")
        eng.embed_heads_load(**m["heads"])
    if "ce" in parts:
        eng.ce_load(A.CE_CFG, models()["ce_t"])
    if "tokens" in parts:
        eng.tokens_load(w["tok"], w["tok_len"])
    return eng


@pytest.fixture
def make():
    """make(*parts, seen=None, **options): a fresh handle (dim 128 with the embedder, else 64) loaded with the named parts; with
    "shards", three handles over BOUNDS. `seen` collects the *_dev entries called. All are closed at the end."""
    from optimized_rag_amd import RagEngine
    made = []

    def one(parts, options, seen, lo=0, hi=N):
        eng = RagEngine(dim=DE if "embedder" in parts else D, device=0)
        made.append(eng)
        if seen is not None:
            eng.lib = Spy(eng.lib, seen)
        for name, value in options.items():
            eng.set_option(name, value)
        return load(eng, parts, lo, hi)

    def _make(*parts, seen=None, **options):
        if "shards" in parts:
            return [one(parts, options, seen, lo, hi) for lo, hi in BOUNDS]
        return one(parts, options, seen)

    yield _make
    for e in made:
        e.close()


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def lex(n, first=0):
    ptr, terms, wts = S.pack_queries(world()["sq"][first:first + n])
    return dict(ptr=ptr, terms=terms, w=wts)


def vecs(n, first=0):
    qv, qo = M.pack(world()["qlist"][first:first + n], TOK)
    return dict(qv=qv, qo=qo)


def keywords(n, sel=None):
    w = world()
    sel = range(n) if sel is None else sel
    ptr, terms = w["post"].encode_queries([w["queries"][i] for i in sel])
    return dict(ptr=ptr, terms=terms)


def dense(n, dim=D, sel=None):
    sel = np.arange(n) if sel is None else np.asarray(sel)
    return dict(q=np.ascontiguousarray(world()["q"][sel, :dim]))


def blank(real, **fill):
    """the legal-but-wrong twin of `real`: zeros of the same shapes (zero queries, term pointers and offsets that name nothing,
    weights that add nothing), `fill` for the arrays whose empty value is not 0"""
    return {k: np.full_like(v, fill[k]) if k in fill else np.zeros_like(v) for k, v in real.items()}


def tenants_of(per_query, n, first=0, sel=None):
    """the tenant argument of n queries: one number each (those of the queries `sel`, where given), or -1 for the batch"""
    if not per_query:
        return -1
    t = world()["tenant_q"]
    return np.array(t[first:first + n]) if sel is None else np.ascontiguousarray(t[np.asarray(sel)])


def on(s):
    import torch
    return torch.cuda.stream(s) if s is not None else contextlib.nullcontext()


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def case_dense_tenants(n=QBIG):
    import torch
    ten = tenants_of(True, n)
    real = dense(n)

    def bind(eng):
        def call(d, s):
            ids, rows, sc = out((n, K), torch.int64), out((n, K), torch.int32), out((n, K), torch.float64)
            eng.dense_topk_dev(d["q"], K, ids, rows, sc, tenant=ten, stream=s)
            return [ids, rows, sc]
        return call
    return Case(("index", "tenants"), {}, blank(real), real, bind)


def case_sparse_topk(per_query=False, n=Q, first=0):
    import torch
    ten = tenants_of(per_query, n, first)
    real = lex(n, first)

    def bind(eng):
        def call(d, s):
            ids, rows, sc = out((n, K), torch.int64), out((n, K), torch.int32), out((n, K), torch.float64)
            eng.sparse_topk_dev(d["ptr"], d["terms"], d["w"], K, ids, rows, sc, stream=s, tenant=ten)
            return [ids, rows, sc]
        return call
    return Case(("index", "tenants", "sparse"), {}, blank(real, terms=-1), real, bind)


def case_bm25(per_query=True, n=Q, tenant=-1, **options):
    import torch
    ten = tenants_of(True, n) if per_query else tenant
    real = keywords(n)

    def bind(eng):
        def call(d, s):
            ids, rows, sc, mx = out((n, K), torch.int64), out((n, K), torch.int32), out((n, K), torch.float64), out((n,), torch.float64)
            eng.bm25_topk_dev(d["ptr"], d["terms"], K, ids, rows, sc, mx, stream=s, tenant=ten)
            return [ids, rows, sc, mx]
        return call
    return Case(("index", "tenants", "bm25"), dict(bm25_plan_slots=8, **options), blank(real, terms=-1), real, bind)


def case_hybrid_rrf(per_query=True, n=QBIG):
    ten = tenants_of(per_query, n)
    real = dict(**dense(n), **keywords(n))

    def bind(eng):
        def call(d, s):
            return list(eng.hybrid_rrf_dev(d["q"], d["ptr"], d["terms"], POOL, K, tenant=ten, stream=s))
        return call
    return Case(("index", "tenants", "bm25"), dict(bm25_plan_slots=8), blank(real, terms=-1), real, bind)


def case_hybrid_sparse_rrf(per_query=False, n=QBIG, **options):
    ten = tenants_of(per_query, n)
    real = dict(**dense(n), **lex(n))

    def bind(eng):
        def call(d, s):
            return list(eng.hybrid_sparse_rrf_dev(d["q"], d["ptr"], d["terms"], d["w"], POOL, K, tenant=ten, stream=s))
        return call
    return Case(("index", "tenants", "sparse"), options, blank(real, terms=-1), real, bind)


NAMES = ("ids", "rows", "hybrid", "semantic", "keyword", "temporal")


def case_hybrid_linear_tenants(n=QBIG, sel=None):
    ten = tenants_of(True, n, sel=sel)
    real = dict(**dense(n, sel=sel), **keywords(n, sel))

    def bind(eng):
        def call(d, s):
            o = eng.hybrid_linear_dev(d["q"], d["ptr"], d["terms"], K, 0.6, 0.3, 0.1, tenant=ten, stream=s)
            return [o[name] for name in NAMES]
        return call
    return Case(("index", "tenants", "bm25", "temporal"), dict(bm25_plan_slots=8), blank(real, terms=-1), real, bind)


def case_linear_chain(per_query=False, n=Q, sel=None):
    """begin -> the gather of the maxima (a device copy, world 1) -> finish -> the gather of the blocks -> merge"""
    import torch
    ten = tenants_of(per_query, n, sel=sel)
    real = dict(**dense(n, sel=sel), **keywords(n, sel))

    def bind(eng):
        def call(d, s):
            mx, gmx = out((n,), torch.float64), out((1, n), torch.float64)
            part, gpart = out((5, n, K), torch.int64), out((1, 5, n, K), torch.int64)
            o = [out((n, K), torch.int64)] + [out((n, K), torch.float64) for _ in range(4)]
            eng.hybrid_linear_begin_dev(d["ptr"], d["terms"], mx, tenant=ten, stream=s)
            with on(s):
                gmx[0].copy_(mx)
            eng.hybrid_linear_finish_dev(d["q"], gmx, K, 0.6, 0.3, 0.1, part, tenant=ten, stream=s)
            with on(s):
                gpart[0].copy_(part)
            eng.hybrid_linear_merge_gathered_dev(gpart, *o, stream=s)
            return [mx, part] + o
        return call
    return Case(("index", "tenants", "bm25", "temporal"), dict(bm25_plan_slots=8), blank(real, terms=-1), real, bind)


def case_retrieve_rerank_tenants(n=12, pool=16, k=5, L=32):
    rng = np.random.default_rng(9)
    Lq = 6                                                       # 192 pairs x 32 tokens = 6144: two chunks of 4096
    ten = tenants_of(True, n)
    real = dict(**dense(n), **keywords(n), q_tok=rng.integers(200, 2000, (n, Lq)).astype(np.int32),
                q_len=rng.integers(1, Lq + 1, n).astype(np.int32))
    wrong = blank(real, terms=-1, q_len=1)

    def bind(eng):
        def call(d, s):
            return list(eng.retrieve_rerank_dev(d["q"], d["q_tok"], d["q_len"], pool, k, term_ptr=d["ptr"], terms=d["terms"], L_pair=L,
                                                tenant=ten, stream=s))
        return call
    return Case(("index", "tenants", "bm25", "ce", "tokens"), dict(ce_chunk_tokens=4096, bm25_plan_slots=8), wrong, real, bind)


def slots(rng, n, pool):
    """int32 [n, pool] rows: random, with an empty slot and a row past the index in the first query"""
    cand = rng.integers(0, N, (n, pool)).astype(np.int32)
    cand[0, :2] = (-1, N)
    return cand


def case_sparse_score_rows(n=Q):
    import torch
    real = dict(**lex(n), cand=slots(np.random.default_rng(21), n, POOL))

    def bind(eng):
        def call(d, s):
            sc = out((n, POOL), torch.float64)
            eng.sparse_score_rows_dev(d["ptr"], d["terms"], d["w"], d["cand"], sc, stream=s)
            return [sc]
        return call
    return Case(("index", "sparse"), {}, blank(real, terms=-1, cand=-1), real, bind)


def case_m3_score_rows(weights, n=Q):
    import torch
    real = dict(cand=slots(np.random.default_rng(22), n, POOL), **vecs(n))
    if weights[0] > 0:
        real.update(dense(n))
    if weights[1] > 0:
        real.update(lex(n))

    def bind(eng):
        def call(d, s):
            ids, sc = out((n, K), torch.int64), out((n, K), torch.float64)
            rows, comp = out((n, K), torch.int32), out((n, K, 3), torch.float64)
            eng.m3_score_rows_dev(d["cand"], K, ids, sc, q_emb=d.get("q"), term_ptr=d.get("ptr"), terms=d.get("terms"), weights=d.get("w"),
                                  q_vecs=d["qv"], q_off=d["qo"], w=weights, rows_out=rows, components_out=comp, stream=s)
            return [ids, sc, rows, comp]
        return call
    return Case(("index", "sparse", "tokvec"), {}, blank(real, terms=-1, cand=-1), real, bind)


def case_tokvec_rerank(store="tokvec", n=Q, first=0):
    import torch
    real = dict(cand=slots(np.random.default_rng(23), n, POOL), **vecs(n, first))

    def bind(eng):
        def call(d, s):
            ids, rows, sc = out((n, K), torch.int64), out((n, K), torch.int32), out((n, K), torch.float64)
            ps = out((n, POOL), torch.float32)
            eng.tokvec_rerank_dev(d["qv"], d["qo"], d["cand"], K, ids, rows, sc, ps, stream=s)
            return [ids, rows, sc, ps]
        return call
    return Case(("index", store), {}, blank(real, cand=-1), real, bind)


def case_retrieve_maxsim(per_query=False, n=QBIG):
    ten = tenants_of(per_query, n)
    real = dict(**dense(n), **lex(n), **vecs(n))

    def bind(eng):
        def call(d, s):
            return list(eng.retrieve_maxsim_dev(d["q"], d["qv"], d["qo"], POOL, K, term_ptr=d["ptr"], terms=d["terms"], weights=d["w"],
                                                tenant=ten, stream=s))
        return call
    return Case(("index", "tenants", "sparse", "tokvec"), {}, blank(real, terms=-1), real, bind)


def case_retrieve_m3(mode, per_query=False, n=QBIG):
    ten = tenants_of(per_query, n)
    real = dict(**dense(n), **lex(n), **vecs(n))

    def bind(eng):
        def call(d, s):
            return list(eng.retrieve_m3_dev(d["q"], POOL, K, term_ptr=d["ptr"], terms=d["terms"], weights=d["w"], q_vecs=d["qv"], q_off=d["qo"],
                                            mode=mode, w=W3, tenant=ten, stream=s))
        return call
    return Case(("index", "tenants", "sparse", "tokvec"), {}, blank(real, terms=-1), real, bind)


def case_maxsim(n=Q, n_docs=60, n_pairs=200):
    import torch
    w = world()
    rng = np.random.default_rng(24)
    d, do = w["d_vecs"][:w["d_off"][n_docs]], w["d_off"][:n_docs + 1]
    pq, pd = rng.integers(-1, n + 1, n_pairs).astype(np.int32), rng.integers(-1, n_docs + 1, n_pairs).astype(np.int32)
    v = vecs(n)
    real = dict(q=v["qv"], qo=v["qo"], d=np.array(d), do=np.array(do), pq=pq, pd=pd)

    def bind(eng):
        def call(dv, s):
            o = out((n_pairs,), torch.float32)
            eng.maxsim_dev(dv["q"], dv["qo"], dv["d"], dv["do"], dv["pq"], dv["pd"], o, stream=s)
            return [o]
        return call
    return Case((), {}, blank(real), real, bind)


def texts(n=Q):
    """token ids, per-position lexical weights (a third of them 0) and lengths of the first n query texts"""
    w = world()
    rng = np.random.default_rng(25)
    wt = rng.random((n, LT)).astype(np.float32)
    wt[rng.random((n, LT)) < 0.3] = 0.0
    return dict(ids=np.array(w["tid"][:n]), w=wt, lens=np.array(w["tlen"][:n]))


def case_lexical_match(n=Q, n_pairs=120):
    import torch
    rng = np.random.default_rng(26)
    real = dict(**texts(n), pq=rng.integers(-1, n + 1, n_pairs).astype(np.int32), pd=rng.integers(-1, n + 1, n_pairs).astype(np.int32))

    def bind(eng):
        def call(d, s):
            o = out((n_pairs,), torch.float32)
            eng.lexical_match_dev(d["ids"], d["w"], d["lens"], d["ids"], d["w"], d["lens"], d["pq"], d["pd"], o, skip_ids=SKIP, stream=s)
            return [o]
        return call
    return Case((), {}, blank(real, lens=1), real, bind)


def case_lexical_compact(n=Q):
    import torch
    real = texts(n)

    def bind(eng):
        def call(d, s):
            ptr, terms, qw = out((n + 1,), torch.int32), out((n * LT,), torch.int32), out((n * LT,), torch.float32)
            eng.lexical_compact_dev(d["ids"], d["w"], d["lens"], ptr, terms, qw, skip_ids=SKIP, stream=s)
            return [ptr, terms, qw]                              # entries past ptr[n] keep the fill on both sides
        return call
    return Case((), {}, blank(real, lens=1), real, bind)


def token_inputs(n=Q):
    w = world()
    real = dict(ids=np.array(w["tid"][:n]), tt=np.zeros((n, LT), np.int32), lens=np.array(w["tlen"][:n]))
    return real, blank(real, lens=1)                             # token id 0 with length 1


def case_embed_multi(n=Q):
    import torch
    real, wrong = token_inputs(n)

    def bind(eng):
        def call(d, s):
            dn, lx = out((n, DE), torch.float32), out((n, LT), torch.float32)
            tk, off = out((n * (LT - 1), TOK), torch.float32), out((n + 1,), torch.int64)
            eng.embed_multi_dev(d["ids"], d["tt"], d["lens"], dense=dn, lex=lx, tok=tk, row_off=off, stream=s)
            return [dn, lx, tk, off]
        return call
    return Case(("embedder",), {}, wrong, real, bind)


def case_search_m3_tokens(per_query=False, mode=2, n=Q):
    ten = tenants_of(per_query, n)
    real, wrong = token_inputs(n)

    def bind(eng):
        def call(d, s):
            return list(eng.search_m3_tokens_dev(d["ids"], d["tt"], d["lens"], POOL, K, skip_ids=SKIP, mode=mode, w=W3, tenant=ten, stream=s))
        return call
    return Case(("index", "tenants", "sparse", "tokvec", "embedder"), {}, wrong, real, bind)


def asked_ids(rng, shape):
    """ids the explicit-id index holds, their upper neighbours (unknown) and -1"""
    ids = world()["ids"]
    return rng.choice(np.concatenate([ids, ids + 1, [-1]]), shape).astype(np.int64)


def case_rows_of_ids(n=256 * Q):
    import torch
    real = dict(ids=asked_ids(np.random.default_rng(27), n))

    def bind(eng):
        def call(d, s):
            rows = out((n,), torch.int32)
            eng.rows_of_ids_dev(d["ids"], rows, stream=s)
            return [rows]
        return call
    return Case(("ids",), {}, blank(real, ids=-1), real, bind)


def gathered_lists(rng, world_n, n, pool):
    """[world, 4, n, pool] int64: ids | score bits | ids | score bits, every rank's lists over its own id range, scores descending"""
    g = np.empty((world_n, 4, n, pool), np.int64)
    for r in range(world_n):
        for p, scale in ((0, 1.0), (2, 9.0)):
            g[r, p] = rng.permutation(50000)[:n * pool].reshape(n, pool) + r * 50000
            g[r, p + 1] = (-np.sort(-(rng.random((n, pool)) * scale + 0.1), axis=1)).view(np.int64)
    g[1, 2, 0, pool // 2:] = -1                                  # a short sparse list
    return g


def case_m3_candidates_gathered(mode, n=Q):
    import torch
    g = gathered_lists(np.random.default_rng(28), 3, n, POOL)
    wrong = np.zeros_like(g)
    wrong[:, 0] = wrong[:, 2] = -1
    width = 2 * POOL if mode == 2 else POOL

    def bind(eng):
        def call(d, s):
            lists, sc, cand = out((2, n, POOL), torch.int64), out((2, n, POOL), torch.float64), out((n, width), torch.int64)
            eng.m3_candidates_gathered_dev(d["g"], lists, sc, cand, mode=mode, stream=s)
            return [lists, sc, cand]
        return call
    return Case((), {}, dict(g=wrong), dict(g=g), bind)


def case_m3_score_ids(explicit, n=Q, width=2 * POOL):
    import torch
    rng = np.random.default_rng(29)
    cand = asked_ids(rng, (n, width)) if explicit else rng.integers(-1, N + 50, (n, width)).astype(np.int64)
    real = dict(cand=cand, **dense(n), **lex(n), **vecs(n))

    def bind(eng):
        def call(d, s):
            part = out((4, n, width), torch.int64)
            eng.m3_score_ids_dev(d["cand"], part, q_emb=d["q"], term_ptr=d["ptr"], terms=d["terms"], weights=d["w"], q_vecs=d["qv"],
                                 q_off=d["qo"], w=W3, stream=s)
            return [part]
        return call
    return Case(("ids" if explicit else "index", "sparse", "tokvec"), {}, blank(real, terms=-1, cand=-1), real, bind)


def case_m3_combine_gathered(n=Q, width=2 * POOL):
    import torch
    rng = np.random.default_rng(30)
    cand = np.stack([rng.permutation(100000)[:width] for _ in range(n)]).astype(np.int64)
    cand[rng.random((n, width)) < 0.1] = -1
    owner = rng.integers(-1, 3, (n, width))                      # -1: nobody owns the slot
    g = np.zeros((3, 4, n, width), np.int64)
    for r in range(3):
        mine = owner == r
        g[r, 0] = mine
        g[r, 1:] = np.where(mine[None], rng.random((3, n, width)).view(np.int64), 0)
    real = dict(cand=cand, g=g)

    def bind(eng):
        def call(d, s):
            ids, sc, comp = out((n, K), torch.int64), out((n, K), torch.float64), out((n, K, 3), torch.float64)
            eng.m3_combine_gathered_dev(d["cand"], d["g"], ids, sc, comp, w=W3, stream=s)
            return [ids, sc, comp]
        return call
    return Case((), {}, blank(real, cand=-1), real, bind)


def case_shard_chain(mode=2, n=Q):
    """The row-sharded three-way search on three handles of one process (tests/test_m3_sharded_gpu.py arranges its shards so): the
    local lists, then the three entries between the two all-gathers, the gathers done as device copies on the same stream."""
    import torch
    real = dict(**dense(n), **lex(n), **vecs(n))
    width = 2 * POOL if mode == 2 else POOL
    i64, f64 = torch.int64, torch.float64

    def bind(engs):
        def call(d, s):
            recv, recv2 = out((3, 4, n, POOL), i64), out((3, 4, n, width), i64)
            for r, e in enumerate(engs):
                send = out((4, n, POOL), i64)
                e.dense_topk_dev(d["q"], POOL, send[0], None, send[1].view(f64), stream=s)
                e.sparse_topk_dev(d["ptr"], d["terms"], d["w"], POOL, send[2], None, send[3].view(f64), stream=s)
                with on(s):
                    recv[r].copy_(send)
            cands = []
            for r, e in enumerate(engs):
                lists, sc, cand = out((2, n, POOL), i64), out((2, n, POOL), f64), out((n, width), i64)
                e.m3_candidates_gathered_dev(recv, lists, sc, cand, mode=mode, stream=s)
                part = out((4, n, width), i64)
                e.m3_score_ids_dev(cand, part, q_emb=d["q"], term_ptr=d["ptr"], terms=d["terms"], weights=d["w"], q_vecs=d["qv"], q_off=d["qo"],
                                   w=W3, stream=s)
                with on(s):
                    recv2[r].copy_(part)
                cands.append(cand)
            outs = []
            for e, cand in zip(engs, cands):
                ids, sc, comp = out((n, K), i64), out((n, K), f64), out((n, K, 3), f64)
                e.m3_combine_gathered_dev(cand, recv2, ids, sc, comp, w=W3, stream=s)
                outs += [ids, sc, comp, cand]
            return outs + [recv, recv2]
        return call
    return Case(("shards", "index", "sparse", "tokvec"), {}, blank(real, terms=-1), real, bind)


def case_tokvec_append(n=200):
    """reserve, then blocks appended from device memory; each is read back through tokvec_rerank_dev on the same stream"""
    import torch
    w = world()
    rows = int(w["d_off"][n])
    real = dict(vecs=np.array(w["d_vecs"][:rows]), off=np.array(w["d_off"][:n + 1]))
    wrong = dict(vecs=np.zeros_like(real["vecs"]), off=real["off"].copy())
    state = {}

    def bind(eng):
        eng.tokvec_reserve(2 * n, 2 * rows, TOK)
        state[id(eng)] = 0
        qv, qo = (torch.from_numpy(a).cuda() for a in M.pack(w["qlist"][:1], TOK))

        def call(d, s):
            first = state[id(eng)]
            eng.tokvec_append_dev(d["vecs"], d["off"], stream=s)
            state[id(eng)] = first + n
            with on(s):
                cand = torch.arange(first, first + n, dtype=torch.int32, device="cuda").reshape(1, n)
            ids, rws, sc, ps = out((1, K), torch.int64), out((1, K), torch.int32), out((1, K), torch.float64), out((1, n), torch.float32)
            eng.tokvec_rerank_dev(qv, qo, cand, K, ids, rws, sc, ps, stream=s)
            return [ids, rws, sc, ps]
        return call
    return Case(("index",), {}, wrong, real, bind)


def doc_major(n):
    """the learned-sparse postings of documents [0, n) as rag_lexical_compact_dev writes them"""
    indptr, doc, wt = world()["csr"]
    term_of = np.repeat(np.arange(VS, dtype=np.int64), np.diff(indptr))
    keep = doc < n
    order = np.lexsort((term_of[keep], doc[keep]))
    ptr = np.zeros(n + 1, np.int32)
    ptr[1:] = np.cumsum(np.bincount(doc[keep], minlength=n))
    return dict(ptr=ptr, terms=term_of[keep][order].astype(np.int32), w=np.ascontiguousarray(wt[keep][order]))


def case_sparse_append(n=200):
    """a block of empty documents (legal), then the real block, appended from device memory; each block's rows are read back through
    sparse_score_rows_dev on the same stream"""
    import torch
    real = doc_major(n)
    state = {}

    def bind(eng):
        state[id(eng)] = 0
        qd = {k: torch.from_numpy(v).cuda() for k, v in lex(8).items()}

        def call(d, s):
            first = state[id(eng)]
            eng.sparse_append_dev(d["ptr"], d["terms"], d["w"], VS, stream=s)
            state[id(eng)] = first + n
            with on(s):
                cand = torch.arange(first, first + n, dtype=torch.int32, device="cuda").repeat(8, 1)
            sc = out((8, n), torch.float64)
            eng.sparse_score_rows_dev(qd["ptr"], qd["terms"], qd["w"], cand, sc, stream=s)
            return [sc]
        return call
    return Case(("index",), {}, blank(real), real, bind)


def case_build_pairs():
    import torch
    rng = np.random.default_rng(7)
    n, pool, Lq, L = 12, 16, 6, 32
    cand = rng.integers(0, N, (n, pool)).astype(np.int64)
    cand[0, 10:] = -1
    real = dict(q_tok=rng.integers(200, 2000, (n, Lq)).astype(np.int32), q_len=rng.integers(1, Lq + 1, n).astype(np.int32), cand=cand)

    def bind(eng):
        def call(d, s):
            io, to, lo = out((n * pool, L), torch.int32), out((n * pool, L), torch.int32), out((n * pool,), torch.int32)
            eng.ce_build_pairs_dev(d["q_tok"], d["q_len"], d["cand"], io, to, lo, stream=s)
            return [io, to, lo]
        return call
    return Case(("tokens",), {}, blank(real, q_len=1, cand=-1), real, bind)


# name -> (builder, asynchronous). ENTRIES: the *_dev entries the case must reach (checked against what the wrapper called).
CASES = {
    "dense_topk_tenants_dev": (case_dense_tenants, True),
    "sparse_topk_dev": (case_sparse_topk, True),
    "sparse_topk_tenants_dev": (lambda: case_sparse_topk(True), True),
    "bm25_topk_tenants_dev": (case_bm25, True),
    "hybrid_rrf_tenants_dev": (case_hybrid_rrf, True),
    "hybrid_sparse_rrf_dev-forked": (case_hybrid_sparse_rrf, True),
    "hybrid_sparse_rrf_dev-no_fork": (lambda: case_hybrid_sparse_rrf(no_fork=1), True),
    "hybrid_sparse_rrf_tenants_dev": (lambda: case_hybrid_sparse_rrf(True), True),
    "hybrid_linear_tenants_dev": (case_hybrid_linear_tenants, True),
    "retrieve_rerank_tenants_dev": (case_retrieve_rerank_tenants, True),
    "sparse_score_rows_dev": (case_sparse_score_rows, True),
    "m3_score_rows_dev-three_way": (lambda: case_m3_score_rows(W3), True),
    "m3_score_rows_dev-colbert_only": (lambda: case_m3_score_rows((0.0, 0.0, 1.0)), True),
    "tokvec_rerank_dev-fp16": (case_tokvec_rerank, True),
    "tokvec_rerank_dev-mxfp8": (lambda: case_tokvec_rerank("tokvec8"), True),
    "retrieve_maxsim_dev": (case_retrieve_maxsim, True),
    "retrieve_maxsim_tenants_dev": (lambda: case_retrieve_maxsim(True), True),
    "retrieve_m3_dev-0": (lambda: case_retrieve_m3(0), True),
    "retrieve_m3_dev-1": (lambda: case_retrieve_m3(1), True),
    "retrieve_m3_dev-2": (lambda: case_retrieve_m3(2), True),
    "retrieve_m3_tenants_dev": (lambda: case_retrieve_m3(2, True), True),
    "maxsim_dev": (case_maxsim, True),
    "lexical_match_dev": (case_lexical_match, True),
    "lexical_compact_dev": (case_lexical_compact, True),
    "embed_multi_dev": (case_embed_multi, True),
    "search_m3_tokens_dev": (case_search_m3_tokens, True),
    "search_m3_tokens_tenants_dev": (lambda: case_search_m3_tokens(True), True),
    "rows_of_ids_dev": (case_rows_of_ids, True),
    "m3_candidates_gathered_dev-0": (lambda: case_m3_candidates_gathered(0), True),
    "m3_candidates_gathered_dev-1": (lambda: case_m3_candidates_gathered(1), True),
    "m3_candidates_gathered_dev-2": (lambda: case_m3_candidates_gathered(2), True),
    "m3_score_ids_dev-implicit_ids": (lambda: case_m3_score_ids(False), True),
    "m3_score_ids_dev-explicit_ids": (lambda: case_m3_score_ids(True), True),
    "m3_combine_gathered_dev": (case_m3_combine_gathered, True),
    "m3_shard_chain": (case_shard_chain, True),
    "hybrid_linear_chain": (case_linear_chain, True),
    "hybrid_linear_chain-tenants": (lambda: case_linear_chain(True), True),
    # documented as waiting for `stream` (host writes that take device memory): compared, not asked to stay pending
    "tokvec_append_dev": (case_tokvec_append, False),
    "sparse_append_dev": (case_sparse_append, False),
}

_CHAIN = ("rag_hybrid_linear_begin_dev", "rag_hybrid_linear_finish_dev", "rag_hybrid_linear_merge_gathered_dev")
ENTRIES = {name: ("rag_" + name.split("-")[0],) for name in CASES}
ENTRIES.update({
    "rows_of_ids_dev": ("rag_index_rows_of_ids_dev",),
    "m3_shard_chain": ("rag_dense_topk_dev", "rag_sparse_topk_dev", "rag_m3_candidates_gathered_dev", "rag_m3_score_ids_dev",
                       "rag_m3_combine_gathered_dev"),
    "hybrid_linear_chain": _CHAIN,
    "hybrid_linear_chain-tenants": ("rag_hybrid_linear_begin_tenants_dev", "rag_hybrid_linear_finish_tenants_dev", _CHAIN[2]),
    "tokvec_append_dev": ("rag_tokvec_append_dev", "rag_tokvec_rerank_dev"),
    "sparse_append_dev": ("rag_sparse_append_dev", "rag_sparse_score_rows_dev"),
})


def differ(a, b):
    return any(not np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


# ---- 1. late producer, early consumer ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_late_producer_and_early_consumer_on_a_side_stream(make, name):
    """busy -> inputs copied in -> the call -> a clone of its outputs, all on one non-default stream; equal to the call made alone,
    and (every entry but the two documented appends) returned while the stream was still busy. The shard chain is also held
    against rag_retrieve_m3_dev on one handle with all rows."""
    import torch
    builder, asynchronous = CASES[name]
    parts, options, wrong, real, bind = builder()
    ref = T.serial(bind(make(*parts, **options)), wrong, real)
    seen = set()
    eng = make(*parts, seen=seen, **options)
    got, pending = T.late_producer(bind(eng), wrong, real, torch.cuda.Stream())
    T.assert_same(got, ref, name)
    assert seen == set(ENTRIES[name]), f"{name} reached {sorted(seen)}"
    if asynchronous:
        assert pending, f"{name} waited for the work queued before it on its stream: the header calls it asynchronous"
    if name == "m3_shard_chain":
        whole = T.serial(case_retrieve_m3(2, n=Q).bind(make("index", "sparse", "tokvec")), wrong, real)
        for r in range(3):
            T.assert_same(got[4 * r:4 * r + 4], whole, f"rank {r} against the unsharded index")


# ---- 2. three calls back to back -----------------------------------------------------------------------------------------------------
STATELESS = sorted(n for n in CASES if CASES[n][1])


@pytest.mark.parametrize("name", STATELESS)
def test_three_calls_back_to_back_behind_busy_work(make, name):
    """busy -> the call -> the same call on the legal-but-wrong inputs -> the first call again, queued at once on one side stream
    (tests/test_stream_order_gpu.py, the test of this name). Per-call state prepared on another stream than the caller's - the
    pipe_ws carve's planes cleared, qten or union_tiles copied, max_key zeroed, the fork of the legs - is then prepared for all
    three before the first runs."""
    import torch
    parts, options, wrong, real, bind = CASES[name][0]()
    ref_call = bind(make(*parts, **options))
    refs = []
    for ins in (real, wrong, real):
        refs.append(T.to_np(ref_call(T.to_dev(ins), None)))
        torch.cuda.synchronize()
    assert differ(refs[0], refs[1]), f"{name}: the wrong inputs give the answer of the real ones; a read of them would pass unseen"
    call = bind(make(*parts, **options))
    s = torch.cuda.Stream()
    d_real, d_wrong = T.to_dev(real), T.to_dev(wrong)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call(d_wrong, s)
        s.synchronize()
        T.busy(s)
        got = [[o.clone() for o in call(d, s)] for d in (d_real, d_wrong, d_real)]
    assert not s.query()
    s.synchronize()
    for i, (g, r) in enumerate(zip(got, refs)):
        T.assert_same(T.to_np(g), r, f"{name} call {i}")


@pytest.mark.parametrize("name", ["hybrid_linear_tenants_dev", "hybrid_linear_chain"])
def test_two_different_batches_back_to_back(make, name):
    """The same entry on the queries in their order and then in reverse, queued at once behind busy work. The per-query maxima of
    the linear fusion are reduced with atomicMax into `max_key`, which each call zeroes first: zeroed on another stream, a slot
    keeps the larger of the two batches' maxima (with the same batch twice, or an empty one in between, it would not show).
    The per-query tenants are reversed with the queries: copied to `qten` on another stream, the second batch's reach the device
    before the first batch runs."""
    import torch
    builder = case_hybrid_linear_tenants if name == "hybrid_linear_tenants_dev" else (lambda **kw: case_linear_chain(True, **kw))
    n = Q
    cases = [builder(n=n), builder(n=n, sel=list(range(n))[::-1])]
    parts, options = cases[0].parts, cases[0].options
    ref_eng = make(*parts, **options)
    refs = []
    for c in cases:
        refs.append(T.to_np(c.bind(ref_eng)(T.to_dev(c.real), None)))
        torch.cuda.synchronize()
    assert differ(refs[0], refs[1])
    eng = make(*parts, **options)
    s = torch.cuda.Stream()
    devs = [T.to_dev(c.real) for c in cases]
    calls = [c.bind(eng) for c in cases]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        calls[0](devs[0], s)
        s.synchronize()
        T.busy(s)
        got = [[o.clone() for o in call(d, s)] for call, d in zip(calls, devs)]
    assert not s.query()
    s.synchronize()
    for i, (g, r) in enumerate(zip(got, refs)):
        T.assert_same(T.to_np(g), r, f"{name} batch {i}")


# ---- 3. between the halves of the linear fusion --------------------------------------------------------------------------------------
def halves(eng, d, n, s, between=()):
    """begin -> the calls of `between` -> finish on stream s -> (clone of the partial block, their clones)"""
    import torch
    mx, gmx, part = out((n,), torch.float64), out((1, n), torch.float64), out((5, n, K), torch.int64)
    eng.hybrid_linear_begin_dev(d["ptr"], d["terms"], mx, stream=s)
    with on(s):
        gmx[0].copy_(mx)
        mid = [[o.clone() for o in call(dv, s)] for call, dv in between]
    eng.hybrid_linear_finish_dev(d["q"], gmx, K, 0.6, 0.3, 0.1, part, stream=s)
    with on(s):
        return [mx.clone(), part.clone()], mid


def test_other_device_calls_between_begin_and_finish_of_the_linear_fusion(make):
    """rag_hybrid_linear_begin_dev leaves the score planes of its batch in the handle (lin_ws, lin_begun); by common.h only a host
    call, a write or rag_hybrid_linear_dev drops them. Queued at once behind busy work: begin -> dense_topk_tenants_dev ->
    bm25_topk_dev -> hybrid_rrf_dev -> retrieve_m3_dev -> finish. The partial block equals that of begin -> finish alone, and each
    interposed result its own reference: none of the four carves, clears or grows what the begun state keeps."""
    import torch
    parts = ("index", "tenants", "bm25", "temporal", "sparse", "tokvec")
    options = dict(bm25_plan_slots=8)
    lin = dict(**dense(Q), **keywords(Q))
    # per-query tenants; one tenant for the batch (the scalar entry); forked legs, no tenant; the union of the two candidate lists
    mids = [case_dense_tenants(), case_bm25(False, n=QBIG, tenant=1), case_hybrid_rrf(False), case_retrieve_m3(2)]

    def inputs(eng):
        d = T.to_dev(lin)
        between = [(c.bind(eng), T.to_dev(c.real)) for c in mids]
        torch.cuda.synchronize()
        return d, between

    ref_eng = make(*parts, **options)
    d, between = inputs(ref_eng)
    ref_part, _ = halves(ref_eng, d, Q, None)
    ref_part = T.to_np(ref_part)
    ref_mid = []
    for call, dv in between:
        ref_mid.append(T.to_np(call(dv, None)))
        torch.cuda.synchronize()
    seen = set()
    eng = make(*parts, seen=seen, **options)
    d, between = inputs(eng)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        halves(eng, d, Q, s, between)                        # first use of every workspace
        s.synchronize()
        T.busy(s)
        got_part, got_mid = halves(eng, d, Q, s, between)
    assert not s.query()
    s.synchronize()
    assert {"rag_dense_topk_tenants_dev", "rag_bm25_topk_dev", "rag_hybrid_rrf_dev", "rag_retrieve_m3_dev"} <= seen
    T.assert_same(T.to_np(got_part), ref_part, "the partial block with four calls between begin and finish")
    for g, r, what in zip(got_mid, ref_mid, ("dense_topk_tenants_dev", "bm25_topk_dev", "hybrid_rrf_dev", "retrieve_m3_dev")):
        T.assert_same(T.to_np(g), r, what + " between begin and finish")


def test_a_host_call_between_begin_and_finish_is_refused_and_the_handle_goes_on(make):
    import torch
    from optimized_rag_amd import RagError
    parts, options = ("index", "tenants", "bm25", "temporal"), dict(bm25_plan_slots=8)
    lin = dict(**dense(Q), **keywords(Q))
    ref_eng = make(*parts, **options)
    ref, _ = halves(ref_eng, T.to_dev(lin), Q, None)
    ref = T.to_np(ref)
    eng = make(*parts, **options)
    d = T.to_dev(lin)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        mx, gmx, part = out((Q,), torch.float64), out((1, Q), torch.float64), out((5, Q, K), torch.int64)
        eng.hybrid_linear_begin_dev(d["ptr"], d["terms"], mx, stream=s)
        eng.dense_topk(world()["q"][:1, :D], 3)              # a host call: the begun state does not survive it
        gmx[0].copy_(mx)
        with pytest.raises(RagError, match=r"\(-3\)"):
            eng.hybrid_linear_finish_dev(d["q"], gmx, K, 0.6, 0.3, 0.1, part, stream=s)
        got, _ = halves(eng, d, Q, s)
    s.synchronize()
    T.assert_same(T.to_np(got), ref, "begin -> finish after the refusal")


# ---- 4. a host call behind a queued device call --------------------------------------------------------------------------------------
def host_calls():
    """name -> (parts, host call(eng) -> list of arrays), each with other inputs and another batch size than the device call's"""
    w = world()
    rng = np.random.default_rng(77)
    one = S.pack_queries(w["sq"][11:12])
    qv, qo = M.pack(w["qlist"][5:6], TOK)
    cand = rng.integers(0, N, (1, 9)).astype(np.int32)
    dv, do = np.array(w["d_vecs"][:w["d_off"][4]]), np.array(w["d_off"][:5])
    t = texts(3)
    tid, tlen = np.array(w["tid"][7:8]), np.array(w["tlen"][7:8])
    return {
        "sparse_topk": (("index", "sparse"), lambda e: list(e.sparse_topk(*one, 7))),
        "tokvec_rerank": (("index", "tokvec"), lambda e: list(e.tokvec_rerank(qv, qo, cand, 4))),
        "maxsim": ((), lambda e: [e.maxsim(qv, qo, dv, do, np.zeros(4, np.int32), np.arange(4, dtype=np.int32))]),
        "tokvec_fetch": (("tokvec",), lambda e: [e.tokvec_fetch(17)]),
        "embed_multi": (("embedder",), lambda e: list(e.embed_multi(tid, np.zeros_like(tid), tlen))),
        "lexical_compact": ((), lambda e: list(e.lexical_compact(t["ids"], t["w"], t["lens"], skip_ids=SKIP))),
        "sparse_scores": (("sparse",), lambda e: [e.sparse_scores(*one)]),
        "sparse_score_rows": (("sparse",), lambda e: [e.sparse_score_rows(*one, cand)]),
        "rows_of_ids": (("ids",), lambda e: [e.rows_of_ids(w["ids"][[3, 4000, 77]] + np.array([0, 1, 0]))]),
    }


# (the device case, the same entry at one query, the host call)
PAIRS = {
    "retrieve_m3_dev/sparse_topk": (lambda n: case_retrieve_m3(2, n=n), QBIG, "sparse_topk"),
    "retrieve_m3_dev/tokvec_rerank": (lambda n: case_retrieve_m3(2, n=n), QBIG, "tokvec_rerank"),
    "retrieve_m3_dev/maxsim": (lambda n: case_retrieve_m3(2, n=n), QBIG, "maxsim"),
    "retrieve_maxsim_dev/tokvec_fetch": (lambda n: case_retrieve_maxsim(n=n), QBIG, "tokvec_fetch"),
    "search_m3_tokens_dev/embed_multi": (lambda n: case_search_m3_tokens(n=n), Q, "embed_multi"),
    "search_m3_tokens_dev/lexical_compact": (lambda n: case_search_m3_tokens(n=n), Q, "lexical_compact"),
    "sparse_topk_dev/sparse_scores": (lambda n: case_sparse_topk(n=n), Q, "sparse_scores"),
    "m3_score_ids_dev/sparse_score_rows": (lambda n: case_m3_score_ids(False, n=n), Q, "sparse_score_rows"),
    "rows_of_ids_dev/rows_of_ids": (lambda n: case_rows_of_ids(n=256 * n), Q, "rows_of_ids"),
}


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_host_call_behind_a_queued_device_call(make, pair):
    """busy -> a large *_dev call queued on a side stream -> at once a *_host call of the same handle with other inputs -> the *_dev
    call again at one query. All three equal their serial references: the host call behaves as if it ran after the queued work
    (the deterministic form of tests/test_stream_order_gpu.py: behind the busy work the device call has certainly not started
    when the host call is made, so workspaces and host-side sizes the host call changes are what the queued call then finds)."""
    import torch
    builder, n, host_name = PAIRS[pair]
    hparts, hcall = host_calls()[host_name]
    parts, options, wrong, real, bind = builder(n)
    sparts, soptions, swrong, sreal, sbind = builder(1)
    parts = tuple(sorted(set(parts) | set(hparts)))
    ref_eng = make(*parts, **options)
    ref_big = T.serial(bind(ref_eng), wrong, real)
    ref_host = [np.asarray(x) for x in hcall(ref_eng)]
    ref_small = T.serial(sbind(ref_eng), swrong, sreal)
    eng = make(*parts, **options)
    s = torch.cuda.Stream()
    call, scall = bind(eng), sbind(eng)
    dev, sdev = T.to_dev(real), T.to_dev(sreal)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call(dev, s)                                        # first use of every workspace
        s.synchronize()
        T.busy(s)
        big = [o.clone() for o in call(dev, s)]
    assert not s.query()
    got_host = [np.asarray(x) for x in hcall(eng)]
    with torch.cuda.stream(s):
        small = [o.clone() for o in scall(sdev, s)]
    s.synchronize()
    T.assert_same(T.to_np(big), ref_big, pair + ": the queued call")
    T.assert_same(got_host, ref_host, pair + ": the host call")
    T.assert_same(T.to_np(small), ref_small, pair + ": one query after the host call")


# ---- 5. a host writer behind a queued call -------------------------------------------------------------------------------------------
def tolerant(call):
    """call(d, s) with RAG_ERR_STATE as a result of its own: what a lookup returns once the id map is gone"""
    def wrapped(d, s):
        import torch
        from optimized_rag_amd import RagError
        try:
            return call(d, s)
        except RagError as e:
            if "(-3)" not in str(e):
                raise
            return [torch.full((1,), -3, dtype=torch.int32, device="cuda")]
    return wrapped


def queued_then_written(make, case, write):
    """busy -> the *_dev call queued -> the write (a host call: it must return only once the stream is idle) -> the call again.
    The queued result equals that of a handle that never saw the write, the later one that of a handle written to first; returns
    the two references."""
    import torch
    parts, options, wrong, real, bind = case
    before = make(*parts, **options)
    ref_before = T.serial(tolerant(bind(before)), wrong, real)
    after = make(*parts, **options)
    write(after)
    ref_after = T.serial(tolerant(bind(after)), wrong, real)
    eng = make(*parts, **options)
    s = torch.cuda.Stream()
    call, dev = tolerant(bind(eng)), T.to_dev(real)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call(dev, s)
        s.synchronize()
        T.busy(s)
        queued = [o.clone() for o in call(dev, s)]
    assert not s.query()
    write(eng)
    assert s.query(), "the writer returned while work queued before it was still pending"
    with torch.cuda.stream(s):
        later = [o.clone() for o in call(dev, s)]
    s.synchronize()
    T.assert_same(T.to_np(queued), ref_before, "queued before the write")
    T.assert_same(T.to_np(later), ref_after, "after the write")
    return ref_before, ref_after


def other_store(e):
    w = world()
    e.tokvec_load(np.ascontiguousarray(w["d_vecs"][::-1]), w["d_off"])       # every document gets other rows; the offsets stay


def other_tokens(e):
    w = world()
    e.tokens_load(np.roll(w["tok"], 1, axis=0), np.roll(w["tok_len"], 1), id_bits=24)       # rag_tokens_load_wide_host


def other_statistics(e):
    p = world()["post"]
    e.bm25_set_statistics(p.idf * np.linspace(0.5, 1.5, p.idf.shape[0]), p.avgdl * 1.3)


WRITERS = {
    "tokvec_load/tokvec_rerank_dev": (case_tokvec_rerank, other_store),
    "tokvec_load/retrieve_m3_dev": (lambda: case_retrieve_m3(2, n=Q), other_store),
    "embed_heads_load/embed_multi_dev": (case_embed_multi, lambda e: e.embed_heads_load(**models()["heads2"])),
    "tokens_load_wide/ce_build_pairs_dev": (case_build_pairs, other_tokens),
    "bm25_set_statistics/bm25_topk_dev": (lambda: case_bm25(False, bm25_keep_tf=1), other_statistics),      # (the option keeps what the impacts are recomputed from)
    "index_id_map_off/rows_of_ids_dev": (case_rows_of_ids, lambda e: e.index_id_map(False)),
    "set_ids/rows_of_ids_dev": (case_rows_of_ids, lambda e: e.set_ids(world()["ids"] + 1)),
    "index_delete/rows_of_ids_dev": (case_rows_of_ids, lambda e: e.index_delete(world()["ids"][100:700])),
    "index_id_map_off/m3_score_ids_dev": (lambda: case_m3_score_ids(True), lambda e: e.index_id_map(False)),
    "set_ids/m3_score_ids_dev": (lambda: case_m3_score_ids(True), lambda e: e.set_ids(world()["ids"] + 1)),
    "index_delete/m3_score_ids_dev": (lambda: case_m3_score_ids(True), lambda e: e.index_delete(world()["ids"][100:700])),
}


@pytest.mark.parametrize("name", sorted(WRITERS))
def test_host_writer_behind_a_queued_call(make, name):
    """The writers that came with the later entries: each waits for the queued call, which still sees the old state, and the same
    call made afterwards sees the new one (once the id map is disabled, a lookup on explicit ids is RAG_ERR_STATE)."""
    builder, write = WRITERS[name]
    a, b = queued_then_written(make, builder(), write)
    assert differ(a, b), f"{name}: the write changes nothing the call returns"
    if name.startswith("index_id_map_off"):
        assert b[0].tolist() == [-3]


# ---- 6. the enqueue cost of the slowest new call -------------------------------------------------------------------------------------
def test_enqueue_cost_is_small_against_the_busy_time(make):
    """tests/test_stream_order_gpu.py, the test of this name, on rag_search_m3_tokens_dev in mode 2 (the forward of the embedder, the
    compaction and the three-way search queued by one call): 10 x its enqueue time must fit into the busy time, or `s.query()`
    proves nothing."""
    import torch
    parts, options, wrong, real, bind = case_search_m3_tokens()
    call = bind(make(*parts, **options))
    s = torch.cuda.Stream()
    dev = T.to_dev(real)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call(dev, s)
        s.synchronize()
        t0 = time.perf_counter()
        call(dev, s)
        enqueue_ms = (time.perf_counter() - t0) * 1e3
        s.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        T.busy(s)
        b.record(s)
        b.synchronize()
    busy_ms = a.elapsed_time(b)
    print(f"enqueue {enqueue_ms:.2f} ms, busy {busy_ms:.1f} ms")
    assert busy_ms >= T.BUSY_MS
    assert enqueue_ms <= ENQUEUE_MS_SLOWEST and 10 * enqueue_ms <= busy_ms
