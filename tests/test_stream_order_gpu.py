"""Stream ordering of the device-pointer (`*_dev`) entry points and of host calls made around them (include/rag_hip.h,
"Ordering"). Every other GPU test hands the library torch's legacy default stream and synchronises the device before its next
call; under that regime a kernel on the wrong stream, a null-stream clear, an input read at enqueue time or a missing join
all give the right answer. Here every call runs on a non-default stream behind work that keeps the stream busy, its inputs
arrive late, and every result is compared bit for bit with the same call made alone and synchronously on a fresh handle
(and, for the entries named in the tests, with the oracle under the tolerance that entry's own test file uses).

Inputs that are not there yet are legal values the header accepts (zero queries, out-of-vocabulary terms, empty candidate
slots, token id 0 with length 1): a mis-ordered read gives unequal arrays, never an out-of-range access.

Busy time (tests/stream_tools.py): BUSY_MS = 200 ms of torch.cuda._sleep, 210 ms measured with device events on an MI355X.
Host-side enqueue cost of the slowest call of this file there (the one-call pipeline with hybrid candidates): 0.17 to 0.28 ms,
a 700th of the busy time; test_enqueue_cost_is_small_against_the_busy_time measures both again and asserts the 10x ratio.

Against the library of the commit before the host-after-device wait, one run, made before the tests named next existed: every
test passed except test_host_dense_search_while_a_device_search_runs (8 host searches met the running device search; 94 % of
its ids wrong). NEVER RUN without the wait: the 13 cases of test_host_call_while_a_device_call_runs and the oracle tests added
with them. So the wait at the start of rag_ce_score_host and rag_embed_host has no recorded witness: no test is known to
fail without it (the earlier cross-encoder overlap, whose host call had to reallocate the workspace and so waited for the
device by itself, was "not seen to fail"). The other tests pin promises that already held; the one-line mutants they were
checked against are named in their docstrings."""
import collections
import time

import numpy as np
import pytest

from oracle import bert_oracle as B
from oracle import rag_oracle as O
import stream_tools as T

pytestmark = pytest.mark.gpu

ENQUEUE_MS_SLOWEST = 20.0        # bound asserted below: BUSY_MS / 10
D, N, QBIG = 128, 7000, 300      # 7000 rows: 4 BM25 doc ranges of 2048, 28 dense tiles; 300 queries: two query tiles
CE_CFG = dict(vocab_size=2000, hidden=384, layers=2, heads=12, ffn=1536, max_pos=128, type_vocab=2, eps=1e-12)
LOGIT_TOL, DENSE_TOL, EMBED_TOL = 4e-3, 1e-9, 1e-3      # tests/test_cross_encoder_gpu.py, test_dense_gpu.py, test_embeddings_gpu.py
_WORLD = {}


def world():
    """Corpus, postings, queries, model weights and token store shared by the tests (built once; handles are per test)."""
    if _WORLD:
        return _WORLD
    from optimized_rag_amd.bm25 import Bm25Postings
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    rng = np.random.default_rng(2024)
    w = _WORLD
    w["emb"] = rng.standard_normal((N, D)).astype(np.float32)
    w["q"] = (w["emb"][rng.integers(0, N, QBIG)] + 0.4 * rng.standard_normal((QBIG, D))).astype(np.float32)
    docs = rng.integers(0, 400, (N, 12))
    w["corpus"] = [" ".join(f"t{t}" for t in d) for d in docs]
    w["post"] = Bm25Postings.from_corpus(w["corpus"])
    # 12-token queries (longer than the 8 planned slots the tests force), one token out of vocabulary
    w["queries"] = [" ".join([f"t{t}" for t in docs[int(rng.integers(0, N))]][:11] + ["zzz"]) for _ in range(QBIG)]
    w["ptr"], w["terms"] = w["post"].encode_queries(w["queries"])
    w["temporal"] = rng.random(N)
    w["ce_w"] = B.seeded_weights(CE_CFG, 11)
    w["ce_t"] = flatten_state_dict(w["ce_w"], CE_CFG["layers"])
    w["ce_w2"] = B.seeded_weights(CE_CFG, 12)
    w["ce_t2"] = flatten_state_dict(w["ce_w2"], CE_CFG["layers"])
    w["emb_t"] = flatten_state_dict(w["ce_w"], CE_CFG["layers"], head=False)
    w["tok"] = rng.integers(200, CE_CFG["vocab_size"], (N, 20)).astype(np.int32)
    w["tok_len"] = rng.integers(3, 21, N).astype(np.int32)
    return w


NBIG = 100_000
_BIG = {}


def big_world():
    """100,000 rows over a 16-word vocabulary: every query token has ~75,000 postings in 49 doc ranges, so the BM25 leg of a
    hybrid call (float64 scoring of ~900,000 postings per query) outlasts its dense leg (dim 128 on the MFMA path)."""
    if _BIG:
        return _BIG
    from optimized_rag_amd.bm25 import Bm25Postings
    rng = np.random.default_rng(2025)
    b = _BIG
    b["emb"] = rng.standard_normal((NBIG, D)).astype(np.float32)
    b["q"] = (b["emb"][rng.integers(0, NBIG, QBIG)] + 0.4 * rng.standard_normal((QBIG, D))).astype(np.float32)
    words = np.array([f"u{t}" for t in range(16)])
    b["post"] = Bm25Postings.from_corpus([" ".join(r) for r in words[rng.integers(0, 16, (NBIG, 12))]])
    b["ptr"], b["terms"] = b["post"].encode_queries([" ".join(r) for r in words[rng.integers(0, 16, (QBIG, 12))]])
    b["temporal"] = rng.random(NBIG)
    return b


def pairs(rng, P, L):
    lens = rng.integers(3, L + 1, P).astype(np.int32)
    ids = rng.integers(5, CE_CFG["vocab_size"], (P, L)).astype(np.int32)
    ids[np.arange(L)[None, :] >= lens[:, None]] = 0
    tt = ((np.arange(L)[None, :] >= 7) & (np.arange(L)[None, :] < lens[:, None])).astype(np.int32)
    return dict(ids=ids, tt=tt, lens=lens)


def wrong_pairs(P, L):
    return dict(ids=np.zeros((P, L), np.int32), tt=np.zeros((P, L), np.int32), lens=np.ones(P, np.int32))


@pytest.fixture
def make():
    """make(*parts, dim=D, **options): a fresh handle loaded with the named parts of world(); all are closed at the end."""
    from optimized_rag_amd import RagEngine
    made = []

    def _make(*parts, dim=D, **options):
        w = world()
        eng = RagEngine(dim=dim, device=0)
        made.append(eng)
        for name, value in options.items():
            eng.set_option(name, value)
        if "index" in parts:
            eng.index_load(w["emb"])
        if "bm25" in parts:
            w["post"].load(eng)
        if "big" in parts:
            eng.index_load(big_world()["emb"])
            big_world()["post"].load(eng)
        if "temporal" in parts:
            eng.set_temporal(big_world()["temporal"] if "big" in parts else w["temporal"])
        if "ce" in parts:
            eng.ce_load(CE_CFG, w["ce_t"])
        if "embed" in parts:
            eng.embed_load(CE_CFG, w["emb_t"], normalize=True)
        if "tokens" in parts:
            eng.tokens_load(w["tok"], w["tok_len"])
        return eng

    yield _make
    for e in made:
        e.close()


# one entry at one shape: handle parts to load, options to set, the legal-but-wrong and the real inputs, bind(eng) -> call(dev, stream)
Case = collections.namedtuple("Case", "parts options wrong real bind")


def out(shape, dtype, fill=-7):
    import torch
    return torch.full(shape, fill, dtype=dtype, device="cuda")


# ---- the 16 device-pointer entries as (parts, options, wrong inputs, real inputs, call(eng) -> call(dev, stream)) ---------------
def case_dense(Q=QBIG, k=10):
    import torch
    w = world()

    def bind(eng):
        def call(d, s):
            ids, rows, sc = out((Q, k), torch.int64), out((Q, k), torch.int32), out((Q, k), torch.float64)
            eng.dense_topk_dev(d["q"], k, ids, rows, sc, stream=s)
            return [ids, rows, sc]
        return call
    return Case(("index",), {}, dict(q=np.zeros((Q, D), np.float32)), dict(q=w["q"][np.arange(Q) % QBIG]), bind)


def case_merge(L=3, Q=40, k=10):
    import torch
    rng = np.random.default_rng(1)
    ids = np.stack([rng.permutation(100000)[:Q * k].reshape(Q, k) + l * 100000 for l in range(L)]).astype(np.int64)
    sc = -np.sort(-rng.random((L, Q, k)), axis=2)

    def bind(eng):
        def call(d, s):
            io, so = out((Q, k), torch.int64), out((Q, k), torch.float64)
            eng.merge_topk_dev(d["ids"], d["sc"], io, so, stream=s)
            return [io, so]
        return call
    return Case((), {}, dict(ids=np.full_like(ids, -1), sc=np.zeros_like(sc)), dict(ids=ids, sc=sc), bind)


def case_fuse_gathered(W=2, Q=40, pool=20, k=10):
    import torch
    rng = np.random.default_rng(2)
    g = np.empty((W, 4, Q, pool), np.int64)
    for r in range(W):
        g[r, 0] = rng.permutation(50000)[:Q * pool].reshape(Q, pool) + r * 50000
        g[r, 1] = (-np.sort(-rng.random((Q, pool)), axis=1)).view(np.int64)
        g[r, 2] = rng.permutation(50000)[:Q * pool].reshape(Q, pool) + r * 50000
        g[r, 3] = (-np.sort(-(rng.random((Q, pool)) * 9 + 0.1), axis=1)).view(np.int64)
    wrong = np.zeros_like(g)
    wrong[:, 0] = -1
    wrong[:, 2] = -1

    def bind(eng):
        def call(d, s):
            lo, so = out((2, Q, pool), torch.int64), out((2, Q, pool), torch.float64)
            ko, ro, ra = out((Q, k), torch.int64), out((Q, k), torch.float64), out((Q, k, 2), torch.int32)
            eng.hybrid_fuse_gathered_dev(d["g"], k, lo, so, ko, ro, ra, stream=s)
            return [lo, so, ko, ro, ra]
        return call
    return Case((), {}, dict(g=wrong), dict(g=g), bind)


def rrf_lists(rng, Q, n_lists, ln):
    return np.stack([np.stack([rng.permutation(3 * ln)[:ln] for _ in range(n_lists)]) for _ in range(Q)]).astype(np.int64)


def case_rrf(Q=40, n_lists=2, ln=20, k=10):
    import torch
    lists = rrf_lists(np.random.default_rng(3), Q, n_lists, ln)

    def bind(eng):
        def call(d, s):
            ko, so, ra = out((Q, k), torch.int64), out((Q, k), torch.float64), out((Q, k, n_lists), torch.int32)
            eng.rrf_fuse_dev(d["lists"], ko, so, ra, stream=s)
            return [ko, so, ra]
        return call
    return Case((), {}, dict(lists=np.full_like(lists, -1)), dict(lists=lists), bind)


def wrong_terms(Q, n_terms):
    return dict(ptr=np.zeros(Q + 1, np.int32), terms=np.full(max(n_terms, 1), -1, np.int32))


def real_terms(Q, big=False):
    w = big_world() if big else world()
    return dict(ptr=w["ptr"][:Q + 1].copy(), terms=w["terms"][:w["ptr"][Q]].copy())


def case_bm25(Q=QBIG, k=10, big=False, **options):
    import torch
    real = real_terms(Q, big)

    def bind(eng):
        def call(d, s):
            ids, rows, sc, mx = out((Q, k), torch.int64), out((Q, k), torch.int32), out((Q, k), torch.float64), out((Q,), torch.float64)
            eng.bm25_topk_dev(d["ptr"], d["terms"], k, ids, rows, sc, mx, stream=s)
            return [ids, rows, sc, mx]
        return call
    return Case((("big",) if big else ("index", "bm25")), dict(bm25_plan_slots=8, **options), wrong_terms(Q, len(real["terms"])), real, bind)


def case_hybrid_rrf(Q=QBIG, pool=20, k=10, big=False, **options):
    w = big_world() if big else world()
    real = dict(q=w["q"][:Q], **real_terms(Q, big))
    wrong = dict(q=np.zeros((Q, D), np.float32), **wrong_terms(Q, len(real["terms"])))

    def bind(eng):
        def call(d, s):
            return list(eng.hybrid_rrf_dev(d["q"], d["ptr"], d["terms"], pool, k, stream=s))
        return call
    return Case((("big",) if big else ("index", "bm25")), dict(bm25_plan_slots=8, **options), wrong, real, bind)


def case_hybrid_linear(Q=QBIG, k=10, big=False):
    w = big_world() if big else world()
    real = dict(q=w["q"][:Q], **real_terms(Q, big))
    wrong = dict(q=np.zeros((Q, D), np.float32), **wrong_terms(Q, len(real["terms"])))

    def bind(eng):
        def call(d, s):
            o = eng.hybrid_linear_dev(d["q"], d["ptr"], d["terms"], k, 0.6, 0.3, 0.1, stream=s)
            return [o[n] for n in ("ids", "rows", "hybrid", "semantic", "keyword", "temporal")]
        return call
    return Case((("big", "temporal") if big else ("index", "bm25", "temporal")), dict(bm25_plan_slots=8), wrong, real, bind)


def case_mmr(variant=0, Q=24, pool=40, k=8):
    import torch
    w = world()
    rng = np.random.default_rng(4)
    rows = np.stack([rng.choice(N, pool, replace=False) for _ in range(Q)]).astype(np.int32)
    rows[min(1, Q - 1), 3 * pool // 4:] = -1

    def bind(eng):
        def call(d, s):
            sel, sc = out((Q, k), torch.int32), out((Q, k), torch.float64)
            eng.mmr_select_dev(d["q"], d["rows"], k, 0.7, variant, sel, sc, stream=s)
            return [sel, sc]
        return call
    return Case(("index",), {}, dict(q=np.zeros((Q, D), np.float32), rows=np.full_like(rows, -1)), dict(q=w["q"][:Q], rows=rows), bind)


def case_ce(ce_mx, P=100, L=64):
    import torch
    real = pairs(np.random.default_rng(5), P, L)

    def bind(eng):
        def call(d, s):
            lg = out((P,), torch.float32)
            eng.ce_score_dev(d["ids"], d["tt"], d["lens"], lg, stream=s)
            return [lg]
        return call
    return Case(("ce",), dict(ce_chunk_tokens=4096, ce_mx=ce_mx), wrong_pairs(P, L), real, bind)       # 6400 tokens: two chunks


def case_embed(P=100, L=64):
    import torch
    real = pairs(np.random.default_rng(6), P, L)
    real["tt"][:] = 0

    def bind(eng):
        def call(d, s):
            o = out((P, CE_CFG["hidden"]), torch.float32)
            eng.embed_dev(d["ids"], d["tt"], d["lens"], o, stream=s)
            return [o]
        return call
    return Case(("embed",), dict(ce_chunk_tokens=4096), wrong_pairs(P, L), real, bind)


def case_build_pairs(Q=12, pool=16, Lq=6, L=32):
    import torch
    w = world()
    rng = np.random.default_rng(7)
    cand = rng.integers(0, N, (Q, pool)).astype(np.int64)
    cand[0, 5 * pool // 8:] = -1
    real = dict(q_tok=rng.integers(200, 2000, (Q, Lq)).astype(np.int32), q_len=rng.integers(1, Lq + 1, Q).astype(np.int32), cand=cand)
    wrong = dict(q_tok=np.zeros((Q, Lq), np.int32), q_len=np.ones(Q, np.int32), cand=np.full_like(cand, -1))

    def bind(eng):
        def call(d, s):
            io, to, lo = out((Q * pool, L), torch.int32), out((Q * pool, L), torch.int32), out((Q * pool,), torch.int32)
            eng.ce_build_pairs_dev(d["q_tok"], d["q_len"], d["cand"], io, to, lo, stream=s)
            return [io, to, lo]
        return call
    return Case(("tokens",), {}, wrong, real, bind)


def case_rerank_topk(Q=12, pool=16, k=5):
    import torch
    rng = np.random.default_rng(8)
    cand = rng.permutation(1000)[:Q * pool].reshape(Q, pool).astype(np.int64)
    cand[min(2, Q - 1), ::3] = -1
    real = dict(logits=rng.standard_normal(Q * pool).astype(np.float32), cand=cand)
    wrong = dict(logits=np.zeros(Q * pool, np.float32), cand=np.full_like(cand, -1))

    def bind(eng):
        def call(d, s):
            io, so, lo = out((Q, k), torch.int64), out((Q, k), torch.float64), out((Q, k), torch.float32)
            eng.rerank_topk_dev(d["logits"], d["cand"], io, so, lo, stream=s)
            return [io, so, lo]
        return call
    return Case((), {}, wrong, real, bind)


def case_retrieve_rerank(mode, Q=12, pool=16, k=5, L=32):
    w = world()
    rng = np.random.default_rng(9)
    Lq = 6                                                       # 192 pairs x 32 tokens = 6144: two chunks of 4096
    real = dict(q=w["q"][:Q], q_tok=rng.integers(200, 2000, (Q, Lq)).astype(np.int32), q_len=rng.integers(1, Lq + 1, Q).astype(np.int32),
                **real_terms(Q))
    wrong = dict(q=np.zeros((Q, D), np.float32), q_tok=np.zeros((Q, Lq), np.int32), q_len=np.ones(Q, np.int32),
                 **wrong_terms(Q, len(real["terms"])))

    def bind(eng):
        def call(d, s):
            kw = dict(term_ptr=d["ptr"], terms=d["terms"]) if mode else {}
            return list(eng.retrieve_rerank_dev(d["q"], d["q_tok"], d["q_len"], pool, k, L_pair=L, stream=s, **kw))
        return call
    return Case(("index", "bm25", "ce", "tokens"), dict(ce_chunk_tokens=4096, bm25_plan_slots=8), wrong, real, bind)


def case_tokens_append():
    """reserve, then blocks appended from device memory; the store is read back through ce_build_pairs_dev on the same stream"""
    import torch
    w = world()
    n, Lt, L = 300, 20, 32
    state = {}

    def bind(eng):
        eng.tokens_reserve(2 * n, Lt)
        state[id(eng)] = 0

        def call(d, s):
            first = state[id(eng)]
            eng.tokens_append_dev(d["tok"], d["len"], stream=s)
            state[id(eng)] = first + n
            cand = torch.arange(first, first + n, dtype=torch.int64, device="cuda").reshape(1, n)
            q_tok, q_len = torch.zeros((1, 1), dtype=torch.int32, device="cuda"), torch.zeros((1,), dtype=torch.int32, device="cuda")
            io, to, lo = out((n, L), torch.int32), out((n, L), torch.int32), out((n,), torch.int32)
            eng.ce_build_pairs_dev(q_tok, q_len, cand, io, to, lo, stream=s)
            return [io, lo]
        return call
    wrong = dict(tok=np.zeros((n, Lt), np.int32), len=np.ones(n, np.int32))
    return Case((), {}, wrong, dict(tok=w["tok"][:n], len=w["tok_len"][:n]), bind)


def case_index_load(append):
    """the wrappers take no stream=: they use the current stream (the `with` block) and synchronise it themselves"""
    import torch
    w = world()
    Q, k = 16, 10
    qd = {}

    def bind(eng):
        if append:
            eng.index_reserve(2 * N)

        def call(d, s):
            assert s is None
            if append:
                eng.index_append(d["emb"])
            else:
                eng.index_load(d["emb"])
            if "q" not in qd:
                qd["q"] = torch.from_numpy(w["q"][:Q]).cuda()
                torch.cuda.current_stream().synchronize()
            ids, sc = out((Q, k), torch.int64), out((Q, k), torch.float64)
            eng.dense_topk_dev(qd["q"], k, ids, None, sc)
            return [ids, sc]
        return call
    return Case((), {}, dict(emb=np.zeros((N, D), np.float32)), dict(emb=w["emb"]), bind)


CASES = {
    "dense_topk_dev": (case_dense, True),
    "merge_topk_dev": (case_merge, True),
    "hybrid_fuse_gathered_dev": (case_fuse_gathered, True),
    "rrf_fuse_dev": (case_rrf, True),
    "bm25_topk_dev": (case_bm25, True),
    "bm25_topk_dev-sub_batched": (lambda: case_bm25(bm25_ws_mb=1), True),
    "hybrid_rrf_dev-forked": (case_hybrid_rrf, True),
    "hybrid_rrf_dev-no_fork": (lambda: case_hybrid_rrf(no_fork=1), True),
    "hybrid_rrf_dev-above_fork_max_q": (lambda: case_hybrid_rrf(fork_max_q=100), True),
    "hybrid_rrf_dev-below_fork_max_q": (lambda: case_hybrid_rrf(Q=64, fork_max_q=100), True),
    # forked, over big_world: the shape built to make the BM25 leg the long one, so that the fusion has to wait for the join
    "hybrid_rrf_dev-long_bm25_leg": (lambda: case_hybrid_rrf(big=True), True),
    "hybrid_linear_dev": (case_hybrid_linear, True),
    "mmr_select_dev-0": (lambda: case_mmr(0), True),
    "mmr_select_dev-1": (lambda: case_mmr(1), True),
    "ce_score_dev-mx": (lambda: case_ce(1), True),
    "ce_score_dev-split": (lambda: case_ce(-1), True),
    "embed_dev": (case_embed, True),
    "ce_build_pairs_dev": (case_build_pairs, True),
    "rerank_topk_dev": (case_rerank_topk, True),
    "retrieve_rerank_dev-0": (lambda: case_retrieve_rerank(0), True),
    "retrieve_rerank_dev-1": (lambda: case_retrieve_rerank(1), True),
    # documented as returning after its rows are checked / wrappers that synchronise themselves: not asked to stay pending
    "tokens_append_dev": (case_tokens_append, False),
    "index_load_dev": (lambda: case_index_load(False), False),
    "index_append_dev": (lambda: case_index_load(True), False),
}


def run_case(make, name, with_block_only=False):
    import torch
    builder, asynchronous = CASES[name]
    parts, options, wrong, real, bind = builder()
    dim = CE_CFG["hidden"] if "embed" in parts else D
    ref = T.serial(bind(make(*parts, dim=dim, **options)), wrong, real)
    eng = make(*parts, dim=dim, **options)
    s = torch.cuda.Stream()
    got, pending = T.late_producer(bind(eng), wrong, real, s, with_block_only=with_block_only or name.startswith("index_"))
    T.assert_same(got, ref, name)
    if asynchronous:
        assert pending, f"{name} waited for the work queued before it on its stream: the header calls it asynchronous"
    return got, real


# ---- Part 1: late producer, early consumer ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_late_producer_and_early_consumer_on_a_side_stream(make, name):
    """busy -> inputs copied in -> the call -> a clone of its outputs, all on one non-default stream; equal to the call made alone.
    A kernel, copy or clear of the entry issued on another stream than the caller's (the handle's private stream, the null
    stream) runs before the inputs arrive or after the clone, and the arrays differ.
    Mutants: the side stream of hybrid_legs not made to wait for the fork event fails the forked hybrid cases and
    retrieve_rerank_dev-1 here; search_init_kernel launched on the handle's private stream fails hybrid_linear_dev and
    retrieve_rerank_dev-1 here (and the dense cases of the back-to-back test below).
    NOT caught by any test: the caller's stream not made to wait for the join event of hybrid_legs. The BM25 leg is queued
    first and finished before the dense leg at every shape tried (7000 rows; 100,000 rows over a 16-word vocabulary,
    hybrid_rrf_dev-long_bm25_leg), and the internal side stream cannot be held back from outside."""
    run_case(make, name)


STATELESS = sorted(n for n in CASES if CASES[n][1])


@pytest.mark.parametrize("name", STATELESS)
def test_three_calls_back_to_back_behind_busy_work(make, name):
    """busy -> the call -> the same call on other (the legal-but-wrong) inputs -> the first call again, queued at once on one
    side stream. Per-call state the entry prepares on another stream than the caller's (counters and thresholds zeroed, a
    workspace cleared, the side stream's fork) is then prepared for all three before the first runs, and a call finds what
    its predecessor left. Mutant: search_init_kernel launched on the handle's private stream fails every dense-backed case."""
    import torch
    builder, _ = CASES[name]
    parts, options, wrong, real, bind = builder()
    dim = CE_CFG["hidden"] if "embed" in parts else D
    ref_eng = make(*parts, dim=dim, **options)
    ref_call = bind(ref_eng)
    refs = []
    for ins in (real, wrong, real):
        refs.append(T.to_np(ref_call(T.to_dev(ins), None)))
        torch.cuda.synchronize()
    eng = make(*parts, dim=dim, **options)
    call = bind(eng)
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


@pytest.mark.parametrize("name", ["dense_topk_dev", "bm25_topk_dev", "hybrid_rrf_dev-forked", "ce_score_dev-mx", "retrieve_rerank_dev-1"])
def test_the_with_block_alone_is_honoured(make, name):
    """no stream= argument: the wrapper takes torch's current stream, here the side stream of the `with` block"""
    run_case(make, name, with_block_only=True)


def test_an_explicit_stream_wins_inside_a_with_block_of_another_stream(make):
    import torch
    w = world()
    Q, k = QBIG, 10
    ref_eng = make("index")
    ref = ref_eng.dense_topk(w["q"], k)
    eng = make("index")
    s, other = torch.cuda.Stream(), torch.cuda.Stream()
    qd = torch.zeros((Q, D), dtype=torch.float32, device="cuda")
    pin = torch.from_numpy(w["q"]).pin_memory()
    ids, rows, sc = out((Q, k), torch.int64), out((Q, k), torch.int32), out((Q, k), torch.float64)
    eng.dense_topk_dev(qd, k, ids, rows, sc)
    torch.cuda.synchronize()
    T.busy(s)
    with torch.cuda.stream(s):
        qd.copy_(pin, non_blocking=True)
    with torch.cuda.stream(other):
        eng.dense_topk_dev(qd, k, ids, rows, sc, stream=s)
    with torch.cuda.stream(s):
        clones = [ids.clone(), rows.clone(), sc.clone()]
    assert not s.query()
    s.synchronize()
    T.assert_same(T.to_np(clones), list(ref), "explicit stream")


def test_results_on_the_side_stream_match_the_oracle(make):
    """Under the tolerance of each entry's own test file: dense (ids exact, 1e-9), BM25 (bit-exact), RRF (keys and ranks
    exact, 1e-12), rerank top-k (ids exact, 1e-12), cross-encoder logits (4e-3), sentence embeddings (1e-3). The other
    entries follow in the tests below."""
    w = world()
    (ids, rows, sc), real = run_case(make, "dense_topk_dev")
    oid, osc = O.dense_topk(w["emb"], real["q"], ids.shape[1])
    np.testing.assert_array_equal(ids, oid)
    np.testing.assert_allclose(sc, osc, rtol=0, atol=DENSE_TOL)

    (ids, rows, sc, mx), real = run_case(make, "bm25_topk_dev")
    post = w["post"]
    for qi in range(0, QBIG, 37):
        t = real["terms"][real["ptr"][qi]:real["ptr"][qi + 1]].tolist()
        raw = O.bm25_scores_csr(post.indptr, post.doc, post.tf, post.doc_len, post.idf, post.avgdl, t)
        m = raw.max() if raw.max() > 0 else 1.0
        top = O.stable_topk_desc(raw, ids.shape[1])
        np.testing.assert_array_equal(rows[qi], top.astype(np.int32))
        np.testing.assert_array_equal(sc[qi], raw[top] / m)
        assert mx[qi] == m

    (keys, rsc, ranks), real = run_case(make, "rrf_fuse_dev")
    for qi in range(keys.shape[0]):
        ok, osc_, orank = O.rrf_fuse([[int(x) for x in lst] for lst in real["lists"][qi]], k=60, top_k=keys.shape[1])
        assert keys[qi].tolist() == ok and ranks[qi].tolist() == orank
        np.testing.assert_allclose(rsc[qi], osc_, atol=1e-12)

    (rid, rscore, rlogit), real = run_case(make, "rerank_topk_dev")
    pool = real["cand"].shape[1]
    for qi in range(rid.shape[0]):
        oi, os_, ol = O.rerank_topk(real["logits"][qi * pool:(qi + 1) * pool], real["cand"][qi], rid.shape[1])
        assert rid[qi].tolist() == oi
        np.testing.assert_allclose(rscore[qi], os_, atol=1e-12)
        np.testing.assert_array_equal(rlogit[qi], np.asarray(ol, np.float32))

    sel = [0, 1, 50, 99]
    for name in ("ce_score_dev-mx", "ce_score_dev-split"):
        (lg,), real = run_case(make, name)
        exp = B.forward_logits(w["ce_w"], CE_CFG, real["ids"][sel].astype(np.int64), real["tt"][sel].astype(np.int64), real["lens"][sel], fast_erf=True)
        assert np.abs(lg[sel] - exp).max() < LOGIT_TOL
    (vec,), real = run_case(make, "embed_dev")
    exp = B.sentence_embeddings(w["ce_w"], CE_CFG, real["ids"][sel].astype(np.int64), real["tt"][sel].astype(np.int64), real["lens"][sel], fast_erf=True)
    assert np.abs(vec[sel] - exp).max() < EMBED_TOL



def merged(ids, sc, k):
    """k best of the concatenated lists of one query: score descending, id ascending; empty slots (-1) last"""
    ids, sc = np.concatenate(ids), np.concatenate(sc)
    live = ids >= 0
    ids, sc = ids[live], sc[live]
    order = np.lexsort((ids, -sc))[:k]
    return ids[order], sc[order]


def test_merge_and_gathered_fusion_on_the_side_stream_match_the_oracle(make):
    """merge_topk_dev: exact (scores are copied). hybrid_fuse_gathered_dev: merged lists exact, BM25 scores divided by the global
    maximum exact, RRF keys and ranks exact, RRF scores 1e-12 (tests/test_sharded_gloo.py, tests/test_hybrid_gpu.py)."""
    (ids, sc), real = run_case(make, "merge_topk_dev")
    for qi in range(ids.shape[0]):
        oi, os_ = merged(list(real["ids"][:, qi]), list(real["sc"][:, qi]), ids.shape[1])
        np.testing.assert_array_equal(ids[qi], oi)
        np.testing.assert_array_equal(sc[qi], os_)
    (lists, lsc, keys, rrf, ranks), real = run_case(make, "hybrid_fuse_gathered_dev")
    g = real["g"]
    pool, k = g.shape[3], keys.shape[1]
    for qi in range(g.shape[2]):
        di, ds = merged(list(g[:, 0, qi]), list(g[:, 1, qi].view(np.float64)), pool)
        bi, bs = merged(list(g[:, 2, qi]), list(g[:, 3, qi].view(np.float64)), pool)
        np.testing.assert_array_equal(lists[0, qi], di)
        np.testing.assert_array_equal(lists[1, qi], bi)
        np.testing.assert_array_equal(lsc[0, qi], ds)
        np.testing.assert_array_equal(lsc[1, qi], bs / (bs.max() if bs.max() > 0 else 1.0))
        ok, osc, orank = O.rrf_fuse([[int(x) for x in di], [int(x) for x in bi]], k=60, top_k=k)
        assert keys[qi].tolist() == ok and ranks[qi].tolist() == orank
        np.testing.assert_allclose(rrf[qi], osc, atol=1e-12)


def bm25_raw(post, real, qi):
    t = real["terms"][real["ptr"][qi]:real["ptr"][qi + 1]].tolist()
    return O.bm25_scores_csr(post.indptr, post.doc, post.tf, post.doc_len, post.idf, post.avgdl, t)


@pytest.mark.parametrize("name", ["hybrid_rrf_dev-forked", "hybrid_rrf_dev-no_fork"])
def test_hybrid_rrf_on_the_side_stream_matches_the_oracle(make, name):
    """oracle dense top-pool + oracle BM25 top-pool -> oracle RRF: keys and ranks exact, scores 1e-12 (tests/test_hybrid_gpu.py)"""
    w = world()
    (keys, rrf, ranks), real = run_case(make, name)
    pool, k = 20, keys.shape[1]
    d_rows, _ = O.dense_topk(w["emb"], real["q"], pool)
    for qi in range(0, QBIG, 23):
        b_rows = O.stable_topk_desc(bm25_raw(w["post"], real, qi), pool)
        ok, osc, orank = O.rrf_fuse([[int(r) for r in d_rows[qi]], [int(r) for r in b_rows]], k=60, top_k=k)
        assert keys[qi].tolist() == ok and ranks[qi].tolist() == orank
        np.testing.assert_allclose(rrf[qi], osc, atol=1e-12)


def test_hybrid_linear_on_the_side_stream_matches_the_oracle(make):
    """hybrid = (alpha * cosine + beta * BM25 / max) + gamma * temporal in float64 over every row, stable sort: rows exact,
    scores and components 1e-12 (tests/test_hybrid_gpu.py)"""
    w = world()
    (ids, rows, hyb, sem, kw, tmp), real = run_case(make, "hybrid_linear_dev")
    k = ids.shape[1]
    for qi in range(0, QBIG, 23):
        cos = O.cosine_matrix(real["q"][qi:qi + 1], w["emb"])[0]
        raw = bm25_raw(w["post"], real, qi)
        key = raw / (raw.max() if raw.max() > 0 else 1.0)
        fused = (0.6 * cos + 0.3 * key) + 0.1 * w["temporal"]
        top = O.stable_topk_desc(fused, k)
        np.testing.assert_array_equal(rows[qi], top.astype(np.int32))
        np.testing.assert_array_equal(ids[qi], top)
        np.testing.assert_allclose(hyb[qi], fused[top], atol=1e-12)
        np.testing.assert_allclose(sem[qi], cos[top], atol=1e-12)
        np.testing.assert_allclose(kw[qi], key[top], atol=1e-12)
        np.testing.assert_allclose(tmp[qi], w["temporal"][top], atol=1e-12)


@pytest.mark.parametrize("variant", [0, 1])
def test_mmr_on_the_side_stream_matches_the_oracle(make, variant):
    """picks exact, scores 1e-12, as tests/test_hybrid_gpu.py checks the same entry"""
    w = world()
    (sel, sc), real = run_case(make, f"mmr_select_dev-{variant}")
    k = sel.shape[1]
    for qi in (0, 1, 7, 23):
        live = [j for j in range(real["rows"].shape[1]) if real["rows"][qi, j] >= 0]
        cand = [w["emb"][real["rows"][qi, j]].astype(np.float64).tolist() for j in live]
        qv = real["q"][qi].astype(np.float64).tolist()
        if variant == 0:
            pos, osc = O.mmr_class(qv, cand, k, 0.7)
            np.testing.assert_allclose(sc[qi, :len(osc)], osc, atol=1e-12)
        else:
            pos = O.mmr_helper(qv, cand, k, 0.7)
        assert sel[qi].tolist() == [live[p] for p in pos] + [-1] * (k - len(pos))


def build_pairs(q_tok, q_len, cand, tok, tok_len, L, cls=101, sep=102):
    """[CLS] query [SEP] passage [SEP] rows in plain numpy, truncated longest-first (tests/test_pipeline_gpu.py)"""
    Q, pool = cand.shape
    ids, tt, lens = np.zeros((Q * pool, L), np.int32), np.zeros((Q * pool, L), np.int32), np.zeros(Q * pool, np.int32)
    for q in range(Q):
        for j in range(pool):
            r = int(cand[q, j])
            ql, dl = O.longest_first_lengths(int(min(q_len[q], q_tok.shape[1])), 0 if r < 0 else int(min(tok_len[r], tok.shape[1])), L - 3)
            row = [cls] + list(q_tok[q, :ql]) + [sep] + ([] if r < 0 else list(tok[r, :dl])) + [sep]
            p = q * pool + j
            ids[p, :len(row)] = row
            tt[p, ql + 2:len(row)] = 1
            lens[p] = len(row)
    return ids, tt, lens


def test_pair_assembly_and_token_appends_on_the_side_stream_match_numpy(make):
    w = world()
    (ids, tt, lens), real = run_case(make, "ce_build_pairs_dev")
    oi, ot, ol = build_pairs(real["q_tok"], real["q_len"], real["cand"], w["tok"], w["tok_len"], ids.shape[1])
    np.testing.assert_array_equal(ids, oi)
    np.testing.assert_array_equal(tt, ot)
    np.testing.assert_array_equal(lens, ol)
    # the second block of 300 rows (the first one held token 0 with length 1), read back through the pair assembly
    (ids, lens), real = run_case(make, "tokens_append_dev")
    n = real["tok"].shape[0]
    oi, _, ol = build_pairs(np.zeros((1, 1), np.int32), np.zeros(1, np.int32), np.arange(n)[None, :], real["tok"], real["len"], ids.shape[1])
    np.testing.assert_array_equal(ids, oi)
    np.testing.assert_array_equal(lens, ol)


def test_index_loads_from_device_memory_on_the_side_stream_match_the_oracle(make):
    """the search that follows the load on the same stream: ids exact, scores 1e-9 (tests/test_dense_gpu.py)"""
    w = world()
    oid, osc = O.dense_topk(w["emb"], w["q"][:16], 10)
    (ids, sc), _ = run_case(make, "index_load_dev")
    np.testing.assert_array_equal(ids, oid)
    np.testing.assert_allclose(sc, osc, rtol=0, atol=DENSE_TOL)
    (ids, sc), _ = run_case(make, "index_append_dev")              # behind a first block of N zero rows (they score 0.0)
    np.testing.assert_array_equal(ids, oid + N)
    np.testing.assert_allclose(sc, osc, rtol=0, atol=DENSE_TOL)


@pytest.mark.parametrize("mode", [0, 1])
def test_pipeline_on_the_side_stream_matches_the_oracle_composition(make, mode):
    """Candidates bit-exact (oracle dense top-pool, or dense + BM25 + RRF); sigmoid scores 1e-3, logits 4e-3 against the float64
    BERT oracle on numpy-built pairs; the order identical wherever the oracle's scores are further apart than the tolerance
    (tests/test_pipeline_gpu.py)."""
    w = world()
    (ids, sc, lg, cand), real = run_case(make, f"retrieve_rerank_dev-{mode}")
    Q, pool, k, L, tol = cand.shape[0], cand.shape[1], ids.shape[1], 32, 1e-3
    d_rows, _ = O.dense_topk(w["emb"], real["q"], pool)
    ocand = d_rows.astype(np.int64)
    if mode:
        ocand = np.full((Q, pool), -1, np.int64)
        for qi in range(Q):
            b_rows = O.stable_topk_desc(bm25_raw(w["post"], real, qi), pool)
            keys, _, _ = O.rrf_fuse([[int(r) for r in d_rows[qi]], [int(r) for r in b_rows]], k=60, top_k=pool)
            ocand[qi, :len(keys)] = keys
    np.testing.assert_array_equal(cand, ocand)
    pid, ptt, plen = build_pairs(real["q_tok"], real["q_len"], ocand, w["tok"], w["tok_len"], L)
    ologit = B.forward_logits(w["ce_w"], CE_CFG, pid.astype(np.int64), ptt.astype(np.int64), plen.astype(np.int64)).reshape(Q, pool)
    oscore = np.array([[O.sigmoid(float(x)) for x in row] for row in ologit])
    for qi in range(Q):
        order = sorted(range(pool), key=lambda j: -oscore[qi, j])
        np.testing.assert_allclose(sc[qi], [oscore[qi, j] for j in order[:k]], atol=tol)
        np.testing.assert_allclose(lg[qi], [ologit[qi, j] for j in order[:k]], atol=4 * tol)
        if np.abs(np.diff([oscore[qi, j] for j in order[:k + 1]])).min() > 2 * tol:
            assert ids[qi].tolist() == [int(ocand[qi, j]) for j in order[:k]]
        else:
            assert set(ids[qi].tolist()) <= set(ocand[qi].tolist())


def test_enqueue_cost_is_small_against_the_busy_time(make):
    """The busy work must outlast the host-side cost of queueing a call behind it, or `s.query()` proves nothing: the slowest
    call of this file (the one-call pipeline, hybrid candidates) is timed on an idle stream and must take less than a tenth of
    BUSY_MS to enqueue; the busy work itself is timed with device events."""
    import torch
    parts, options, wrong, real, bind = case_retrieve_rerank(1)
    eng = make(*parts, **options)
    call = bind(eng)
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


# ---- Part 2: a host call while a device-pointer call of the same handle is pending --------------------------------------------------
def host_calls(big=False, pair_len=40):
    """name -> (parts, host call(eng) -> list of arrays), each with inputs and a batch size unlike the device call's. big: for
    handles loaded with big_world() (the BM25 queries must use that vocabulary)."""
    w = world()
    rng = np.random.default_rng(77)
    q1 = ((big_world() if big else w)["emb"][4321:4322] + 0.2).astype(np.float32)
    hp = pairs(rng, 1, pair_len)
    ptr1, terms1 = big_world()["post"].encode_queries(["u3 u7 u7 u1"]) if big else w["post"].encode_queries([w["corpus"][99]])
    small = rng.standard_normal((9, D)).astype(np.float32)
    adhoc = ["a b c", "b c d d", "e"]
    from optimized_rag_amd.bm25 import Bm25Postings
    ap = Bm25Postings.from_corpus(adhoc)
    aptr, aterms = ap.encode_queries(["b d", "e a"])
    return {
        "dense_topk": (("index",), lambda e: list(e.dense_topk(q1, 7))),
        "ce_score": (("ce",), lambda e: [e.ce_score(hp["ids"], hp["tt"], hp["lens"])]),
        "embed": (("embed",), lambda e: [e.embed(hp["ids"], np.zeros_like(hp["tt"]), hp["lens"])]),
        "bm25_topk": (("index", "bm25"), lambda e: list(e.bm25_topk(ptr1, terms1, 5))),
        "bm25_scores": (("index", "bm25"), lambda e: [e.bm25_scores(ptr1, terms1)]),
        "bm25_scores_adhoc": (("index", "bm25"), lambda e: [e.bm25_scores_adhoc(ap.indptr, ap.doc, ap.tf, ap.doc_len, ap.idf, ap.avgdl, aptr, aterms)]),
        "pairwise_cosine": (("index",), lambda e: [e.pairwise_cosine(small)]),
        "rrf_fuse": (("index",), lambda e: list(e.rrf_fuse(rrf_lists(np.random.default_rng(5), 3, 2, 9), top_k=5))),
        "mmr_select": (("index",), lambda e: list(e.mmr_select(small[0], small, 4, 0.7, 0))),
        "chunk_chain": (("index",), lambda e: [e.chunk_chain(small, np.full(9, 30, np.int32), 0.1, 200, 20)]),
        "linear_fuse_topk": (("index",), lambda e: list(e.linear_fuse_topk(np.linspace(0, 1, 50), np.linspace(1, 0, 50) ** 2, None, 0.6, 0.3, 0.1, 5))),
        "fetch_rows": (("index",), lambda e: [e.fetch_rows([5, 6999, 17])]),
        # 64 MiB of float64 pairs: far past the staging arena the earlier calls of a handle left, so the arena grows in the middle
        "pairwise_cosine-arena_grows": (("index",), lambda e: [e.pairwise_cosine(np.tile(small, (320, 1)))]),
    }


PAIRS = [("dense_topk_dev", "dense_topk"), ("hybrid_rrf_dev-forked", "dense_topk"), ("hybrid_linear_dev", "dense_topk"),
         ("retrieve_rerank_dev-1", "dense_topk"), ("ce_score_dev-mx", "ce_score"), ("ce_score_dev-split", "ce_score"),
         ("retrieve_rerank_dev-1", "ce_score"), ("embed_dev", "embed"),
         ("bm25_topk_dev", "bm25_topk"), ("bm25_topk_dev", "bm25_scores"), ("bm25_topk_dev", "bm25_scores_adhoc"),
         ("hybrid_rrf_dev-forked", "bm25_topk"), ("hybrid_rrf_dev-forked", "bm25_scores"), ("hybrid_rrf_dev-forked", "bm25_scores_adhoc"),
         ("dense_topk_dev", "pairwise_cosine"), ("dense_topk_dev", "rrf_fuse"), ("dense_topk_dev", "mmr_select"),
         ("dense_topk_dev", "chunk_chain"), ("dense_topk_dev", "linear_fuse_topk"), ("dense_topk_dev", "fetch_rows"),
         ("dense_topk_dev", "pairwise_cosine-arena_grows")]


def small_case(name):
    """the same entry at a small batch (1 query / 2 pairs): what a host drives between its large batches"""
    base = name.split("-")[0]
    if base == "dense_topk_dev":
        return case_dense(Q=1)
    if base == "hybrid_rrf_dev":
        return case_hybrid_rrf(Q=1)
    if base == "hybrid_linear_dev":
        return case_hybrid_linear(Q=1)
    if base == "retrieve_rerank_dev":
        return case_retrieve_rerank(1, Q=1)
    if base == "bm25_topk_dev":
        return case_bm25(Q=1)
    if base == "ce_score_dev":
        return case_ce(1 if name.endswith("mx") else -1, P=2)
    return case_embed(P=2)


@pytest.mark.parametrize("dev_name,host_name", PAIRS)
def test_host_call_behind_a_queued_device_call(make, dev_name, host_name):
    """busy -> a large *_dev call queued on a side stream -> at once a *_host call of the same handle with other inputs and
    batch size 1 -> the *_dev call again at a small batch. All three equal their serial references: the host call behaves as
    if it ran after the queued work. Deterministic: behind the busy work the device call has certainly not started when the
    host call is made, so host-side state the host call changes at enqueue time (q16_dirty, ws_q, ws_pairs) and workspaces
    it rewrites are what the queued call then finds.
    Without the wait (run once on the commit before it): not seen to fail. There the host call runs at once on the handle's
    private stream and is finished before the queued call starts; the race needs both on the device together (the
    overlapping variant below, which did fail)."""
    import torch
    hparts, hcall = host_calls()[host_name]
    parts, options, wrong, real, bind = CASES[dev_name][0]()
    sparts, soptions, swrong, sreal, sbind = small_case(dev_name)
    parts = tuple(sorted(set(parts) | set(hparts)))
    dim = CE_CFG["hidden"] if "embed" in parts else D
    ref_eng = make(*parts, dim=dim, **options)
    ref_big = T.serial(bind(ref_eng), wrong, real)
    ref_host = hcall(ref_eng)
    ref_small = T.serial(sbind(ref_eng), swrong, sreal)
    eng = make(*parts, dim=dim, **options)
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
    got_host = hcall(eng)
    with torch.cuda.stream(s):
        small = [o.clone() for o in scall(sdev, s)]
    s.synchronize()
    T.assert_same(T.to_np(big), ref_big, dev_name)
    T.assert_same([np.asarray(x) for x in got_host], [np.asarray(x) for x in ref_host], host_name)
    T.assert_same(T.to_np(small), ref_small, dev_name + " (small batch after the host call)")


def test_small_device_batch_then_large_host_batch(make):
    """the other way round: 1 query queued on the device side, 300 host queries at once behind it"""
    import torch
    w = world()
    parts, options, wrong, real, bind = case_dense(Q=1)
    ref_eng = make("index")
    ref_dev = T.serial(bind(ref_eng), wrong, real)
    ref_host = ref_eng.dense_topk(w["q"][::-1], 10)
    eng = make("index")
    s = torch.cuda.Stream()
    call, dev = bind(eng), T.to_dev(real)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call(dev, s)
        s.synchronize()
        T.busy(s)
        first = [o.clone() for o in call(dev, s)]
    assert not s.query()
    got_host = eng.dense_topk(w["q"][::-1], 10)
    with torch.cuda.stream(s):
        again = [o.clone() for o in call(dev, s)]
    s.synchronize()
    T.assert_same(T.to_np(first), ref_dev)
    T.assert_same(list(got_host), list(ref_host))
    T.assert_same(T.to_np(again), ref_dev)


def overlapping(make, parts, dim, options, bind, real, hcall, n_host=8):
    import torch
    ref_eng = make(*parts, dim=dim, **options)
    ref_call = bind(ref_eng)
    ref = T.to_np(ref_call(T.to_dev(real), None))
    torch.cuda.synchronize()
    ref_host = [np.asarray(x) for x in hcall(ref_eng)]
    eng = make(*parts, dim=dim, **options)
    s = torch.cuda.Stream()
    call, dev = bind(eng), T.to_dev(real)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call(dev, s)
        s.synchronize()
        outs = call(dev, s)
        clones = [o.clone() for o in outs]
    hosts, overlapped = [], 0
    for _ in range(n_host):                                  # a fixed small count, not a loop until something breaks
        if s.query():
            break
        hosts.append([np.asarray(x) for x in hcall(eng)])
        overlapped += 1
    s.synchronize()
    print(f"host calls issued while the device call was pending: {overlapped}")
    assert overlapped >= 1, "the device call had finished before the first host call was made: nothing was tested"
    T.assert_same(T.to_np(clones), ref, "device call")
    for h in hosts:
        T.assert_same(h, ref_host, "host call")


def test_host_dense_search_while_a_device_search_runs(make):
    """No busy work: 4096 queries over 200,000 rows run for milliseconds on the side stream while up to 8 single-query host
    searches are issued (each is made only while `s.query()` is still false). Both searches use the handle's one dense
    workspace; the host one used to run on the private stream at the same time, zeroing `cnt` / `tau` / `stats` and clearing
    rows of `q16` under the running search. CAN ONLY FAIL WITH SOME PROBABILITY on a library without the wait (the two must
    meet on the device); with it the host call starts after the device work and the test is deterministic.
    Without the wait (run once): FAILED, all 8 host searches were issued while the device search was pending and 94 % of the
    device search's ids were wrong."""
    import torch
    rng = np.random.default_rng(91)
    Q, k, rows = 4096, 50, 200_000
    emb = rng.standard_normal((rows, D)).astype(np.float32)
    q = (emb[rng.integers(0, rows, Q)] + 0.4 * rng.standard_normal((Q, D))).astype(np.float32)
    q1 = (emb[77:78] * 1.5).astype(np.float32)

    def make_big(*parts, **kw):
        e = make(**kw)
        e.index_load(emb)
        return e

    def bind(eng):
        def call(d, s):
            ids, rws, sc = out((Q, k), torch.int64), out((Q, k), torch.int32), out((Q, k), torch.float64)
            eng.dense_topk_dev(d["q"], k, ids, rws, sc, stream=s)
            return [ids, rws, sc]
        return call
    overlapping(make_big, (), D, {}, bind, dict(q=q), lambda e: list(e.dense_topk(q1, 7)))


def overlap_cases():
    """name -> (device case, big world?, host call name). The device batches run for milliseconds to tens of milliseconds. The
    host model calls use one pair of the SAME padded length (128) as the device batch: the host call then needs no new
    workspace (a reallocation frees the old one, which waits for the device and hides the race) and writes its
    activations into the rows the running device chunk is using."""
    ce_opts = dict(P=4096, L=128)
    return {
        "hybrid_rrf_dev/dense_topk": (lambda: case_hybrid_rrf(big=True), True, "dense_topk"),
        "hybrid_linear_dev/dense_topk": (lambda: case_hybrid_linear(big=True), True, "dense_topk"),
        "retrieve_rerank_dev/dense_topk": (lambda: case_retrieve_rerank(1, Q=64, pool=64, L=128), False, "dense_topk"),
        "retrieve_rerank_dev/ce_score": (lambda: case_retrieve_rerank(1, Q=64, pool=64, L=128), False, "ce_score"),
        "ce_score_dev-mx/ce_score": (lambda: case_ce(1, **ce_opts), False, "ce_score"),
        "ce_score_dev-split/ce_score": (lambda: case_ce(-1, **ce_opts), False, "ce_score"),
        "embed_dev/embed": (lambda: case_embed(**ce_opts), False, "embed"),
        "bm25_topk_dev/bm25_topk": (lambda: case_bm25(big=True), True, "bm25_topk"),
        "bm25_topk_dev/bm25_scores": (lambda: case_bm25(big=True), True, "bm25_scores"),
        "bm25_topk_dev/bm25_scores_adhoc": (lambda: case_bm25(big=True), True, "bm25_scores_adhoc"),
        "hybrid_rrf_dev/bm25_topk": (lambda: case_hybrid_rrf(big=True), True, "bm25_topk"),
        "hybrid_rrf_dev/bm25_scores": (lambda: case_hybrid_rrf(big=True), True, "bm25_scores"),
        "hybrid_rrf_dev/bm25_scores_adhoc": (lambda: case_hybrid_rrf(big=True), True, "bm25_scores_adhoc"),
    }


@pytest.mark.parametrize("name", sorted(overlap_cases()))
def test_host_call_while_a_device_call_runs(make, name):
    """The overlapping variant of every remaining pair: no busy work, the device call running on the side stream, up to 8 host
    calls issued while `s.query()` is false; every result equals its serial reference. CAN ONLY FAIL WITH SOME PROBABILITY on
    a library without the wait; deterministic with it. These 13 cases were never run on a library without the wait: which
    of them fail there is not known (see the module docstring)."""
    builder, big, host_name = overlap_cases()[name]
    parts, options, wrong, real, bind = builder()
    hparts, hcall = host_calls(big=big, pair_len=128)[host_name]
    if not big:
        parts = tuple(sorted(set(parts) | set(hparts)))
    dim = CE_CFG["hidden"] if "embed" in parts else D
    if name.startswith(("ce_score_dev", "embed_dev")):
        options = {k: v for k, v in options.items() if k != "ce_chunk_tokens"}       # one chunk: every row of the planes in use
    overlapping(make, parts, dim, options, bind, real, hcall)


def test_dense_stats_after_a_queued_search_are_that_searchs(make):
    import torch
    w = world()
    parts, options, wrong, real, bind = case_dense(Q=QBIG)
    eng = make("index")
    eng.dense_topk(w["q"][:5], 3)
    s = torch.cuda.Stream()
    call, dev = bind(eng), T.to_dev(real)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call(dev, s)
        s.synchronize()
        eng.dense_topk(w["q"][:5], 3)
        T.busy(s)
        call(dev, s)
    st = eng.dense_stats()
    assert st["n_queries"] == QBIG and st["proven_fast"] + st["proven_wide"] + st["exact_scan"] == QBIG, st


# ---- Part 3: writes behind a queued call -----------------------------------------------------------------------------------------------
def queued_then_written(make, parts, options, dev_case, writes, dim=D):
    """busy -> the *_dev call queued -> each write in turn (host calls) -> the call again. Returns (queued result, result
    after the writes, and the two references: a handle that never saw the writes, a handle written to first)."""
    import torch
    wrong, real, bind = dev_case.wrong, dev_case.real, dev_case.bind
    before = make(*parts, dim=dim, **options)
    ref_before = T.serial(bind(before), wrong, real)
    after = make(*parts, dim=dim, **options)
    for wr in writes:
        wr(after)
    ref_after = T.serial(bind(after), wrong, real)
    eng = make(*parts, dim=dim, **options)
    s = torch.cuda.Stream()
    call, dev = bind(eng), T.to_dev(real)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call(dev, s)
        s.synchronize()
        T.busy(s)
        queued = [o.clone() for o in call(dev, s)]
    assert not s.query()
    for wr in writes:
        wr(eng)
    with torch.cuda.stream(s):
        later = [o.clone() for o in call(dev, s)]
    s.synchronize()
    T.assert_same(T.to_np(queued), ref_before, "queued before the write")
    T.assert_same(T.to_np(later), ref_after, "after the write")
    return ref_before, ref_after


def differ(a, b):
    return any(not np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_tenant_table_set_changed_and_cleared_behind_a_queued_search(make):
    import torch
    w = world()
    rng = np.random.default_rng(31)
    t1, t2 = rng.integers(0, 3, N).astype(np.int32), rng.integers(0, 3, N).astype(np.int32)
    Q, k = 64, 10

    unfiltered = set()                                       # handles whose table was cleared: they are searched without a filter

    def clear(e):
        e.set_tenants(None)
        unfiltered.add(id(e))

    def tenant_case(tenant):
        def bind(eng):
            def call(d, s):
                ids, rows, sc = out((Q, k), torch.int64), out((Q, k), torch.int32), out((Q, k), torch.float64)
                eng.dense_topk_dev(d["q"], k, ids, rows, sc, tenant=-1 if id(eng) in unfiltered else tenant, stream=s)
                return [ids, rows, sc]
            return call
        return Case(("index",), {}, dict(q=np.zeros((Q, D), np.float32)), dict(q=w["q"][:Q]), bind)

    eng_parts = ("index",)

    def first(e):
        e.set_tenants(t1)

    def make1(*parts, **kw):                                 # handles that start with the first table
        e = make(*parts, **kw)
        first(e)
        return e
    # set -> change: the queued tenant-1 search sees the first table
    a, b = queued_then_written(make1, eng_parts, {}, tenant_case(1), [lambda e: e.set_tenants(t2)])
    assert differ(a, b)
    # clear: the queued filtered search still filters; the unfiltered search made afterwards sees every row
    a, b = queued_then_written(make1, eng_parts, {}, tenant_case(1), [clear])
    assert (t1[a[1]] == 1).all() and not (t1[b[1]] == 1).all()
    np.testing.assert_array_equal(b[0], O.dense_topk(w["emb"], w["q"][:Q], k)[0])
    # set on a handle without a table, behind an unfiltered search
    queued_then_written(make, eng_parts, {}, tenant_case(-1), [first])


def test_ids_replaced_behind_a_queued_search(make):
    pk = (np.random.default_rng(32).permutation(N) + 10_000).astype(np.int64)
    a, b = queued_then_written(make, ("index",), {}, case_dense(Q=64), [lambda e: e.set_ids(pk)])
    np.testing.assert_array_equal(b[0], pk[a[0]])


def test_temporal_scores_replaced_behind_a_queued_linear_fusion(make):
    t2 = np.random.default_rng(33).random(N) * 3
    a, b = queued_then_written(make, ("index", "bm25", "temporal"), dict(bm25_plan_slots=8), case_hybrid_linear(Q=64), [lambda e: e.set_temporal(t2)])
    assert differ(a, b)


def test_token_store_replaced_behind_a_queued_pipeline_call(make):
    w = world()
    tok2 = np.roll(w["tok"], 1, axis=0)
    len2 = np.roll(w["tok_len"], 1)
    a, b = queued_then_written(make, ("index", "bm25", "ce", "tokens"), dict(ce_chunk_tokens=4096, bm25_plan_slots=8), case_retrieve_rerank(1),
                               [lambda e: e.tokens_load(tok2, len2)])
    assert differ(a, b)


def other_postings():
    """Postings of the corpus in reverse row order under the SAME term numbering as world()["post"] (the term ids of the queued
    queries stay legal and mean the same words; every row holds another document)."""
    from optimized_rag_amd.bm25 import Bm25Postings
    w = world()
    p2 = Bm25Postings.from_corpus(w["corpus"][::-1])
    order = np.asarray([p2.vocab[t] for t in w["post"].vocab])                       # dicts keep first-appearance order
    assert len(order) == len(p2.vocab)
    indptr = np.concatenate([[0], np.cumsum(np.diff(p2.indptr)[order])]).astype(np.int64)
    perm = np.concatenate([np.arange(p2.indptr[t], p2.indptr[t + 1]) for t in order])
    return Bm25Postings(indptr, p2.doc[perm], p2.tf[perm], p2.doc_len, p2.idf[order], p2.avgdl, w["post"].vocab, p2.k1, p2.b)


@pytest.mark.parametrize("dev_name", ["bm25_topk_dev", "hybrid_rrf_dev-forked"])
def test_postings_replaced_and_normalisation_switched_behind_a_queued_call(make, dev_name):
    p2 = other_postings()
    case = CASES[dev_name][0]()
    a, b = queued_then_written(make, ("index", "bm25"), case.options, case, [lambda e: p2.load(e)])
    assert differ(a, b)
    # the switch is host state read while a call enqueues: no wait is needed for the queued call to keep the old value
    a, b = queued_then_written(make, ("index", "bm25"), case.options, case, [lambda e: e.bm25_set_normalize(False)])
    assert differ(a, b) == (dev_name == "bm25_topk_dev")         # the fused ranks of the hybrid call do not depend on it


def test_index_reloaded_behind_a_queued_search(make):
    w = world()
    a, b = queued_then_written(make, ("index",), {}, case_dense(Q=64), [lambda e: e.index_load(w["emb"][::-1].copy())])
    np.testing.assert_array_equal(b[0], N - 1 - a[0])


def test_index_reserved_anew_behind_a_queued_search(make):
    """rag_index_reserve drops the index: the queued search still sees the rows, the one made afterwards an empty index"""
    a, b = queued_then_written(make, ("index",), {}, case_dense(Q=64), [lambda e: e.index_reserve(N)])
    assert (a[0] >= 0).all() and (b[0] == -1).all()


def test_embedding_weights_replaced_behind_a_queued_call(make):
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    t2 = flatten_state_dict(world()["ce_w2"], CE_CFG["layers"], head=False)
    a, b = queued_then_written(make, ("embed",), dict(ce_chunk_tokens=4096), case_embed(), [lambda e: e.embed_load(CE_CFG, t2, normalize=True)],
                               dim=CE_CFG["hidden"])
    assert differ(a, b)


@pytest.mark.parametrize("ce_mx", [1, -1])
def test_weights_replaced_behind_a_queued_scoring(make, ce_mx):
    w = world()
    a, b = queued_then_written(make, ("ce",), dict(ce_chunk_tokens=4096, ce_mx=ce_mx), case_ce(ce_mx), [lambda e: e.ce_load(CE_CFG, w["ce_t2"])])
    assert differ(a, b)


def test_rejected_then_accepted_token_block_behind_busy_work(make):
    """rag_tokens_reserve clears the counter of bad ids; the first append counts into it on the caller's (non-blocking) stream.
    A rejected block (an id above 65535) must leave the counter clear for the accepted one that follows.
    The clear moved back to a null-stream hipMemset is NOT caught (passes here and on the commit before): the runtime finishes
    that 4-byte memset before it returns, so no stream can run ahead of it; the stream-ordered clear states the intent."""
    import torch
    from optimized_rag_amd import RagError
    w = world()
    n, Lt, L = 300, 20, 32
    eng = make()
    eng.tokens_reserve(n, Lt)
    s = torch.cuda.Stream()
    bad = w["tok"][:n].copy()
    bad[17, 3] = 70000
    tok_d, bad_d, len_d = (torch.from_numpy(a).cuda() for a in (w["tok"][:n], bad, w["tok_len"][:n]))
    torch.cuda.synchronize()
    T.busy(s)
    with pytest.raises(RagError):
        eng.tokens_append_dev(bad_d, len_d, stream=s)
    T.busy(s, 50)
    eng.tokens_append_dev(tok_d, len_d, stream=s)
    with torch.cuda.stream(s):
        cand = torch.arange(n, dtype=torch.int64, device="cuda").reshape(1, n)
        io, to, lo = out((n, L), torch.int32), out((n, L), torch.int32), out((n,), torch.int32)
        eng.ce_build_pairs_dev(torch.zeros((1, 1), dtype=torch.int32, device="cuda"), torch.zeros((1,), dtype=torch.int32, device="cuda"),
                               cand, io, to, lo, stream=s)
    s.synchronize()
    io, lo = io.cpu().numpy(), lo.cpu().numpy()
    for r in (0, 17, n - 1):
        ln = int(w["tok_len"][r])
        assert lo[r] == ln + 3 and io[r, 2:2 + ln].tolist() == w["tok"][r, :ln].tolist()


# ---- Part 4: workspace growth with work queued; two handles at once ---------------------------------------------------------------------
def grow_sequence(make, cases):
    """On one side stream, nothing synchronising in between: every case of `cases` in turn (small, large, small). Each equals
    the same call on a handle of its own."""
    import torch
    parts = tuple(sorted(set().union(*[set(c.parts) for c in cases])))
    options = {k: v for c in cases for k, v in c.options.items()}
    dim = CE_CFG["hidden"] if "embed" in parts else D
    refs = []
    for c in cases:
        e = make(*parts, dim=dim, **options)
        refs.append(T.to_np(c.bind(e)(T.to_dev(c.real), None)))
    torch.cuda.synchronize()
    eng = make(*parts, dim=dim, **options)
    s = torch.cuda.Stream()
    devs = [T.to_dev(c.real) for c in cases]
    torch.cuda.synchronize()
    got = []
    with torch.cuda.stream(s):
        T.busy(s, 50)
        for c, d in zip(cases, devs):
            got.append([o.clone() for o in c.bind(eng)(d, s)])
    s.synchronize()
    for i, (g, r) in enumerate(zip(got, refs)):
        T.assert_same(T.to_np(g), r, f"call {i}")


def test_dense_workspace_grows_with_work_queued(make):
    grow_sequence(make, [case_dense(Q=8), case_dense(Q=600), case_dense(Q=8)])


def test_bm25_workspace_grows_with_work_queued(make):
    grow_sequence(make, [case_bm25(Q=4, k=10), case_bm25(Q=200, k=100), case_bm25(Q=4, k=10)])


def test_cross_encoder_workspace_grows_with_work_queued(make):
    grow_sequence(make, [case_ce(1, P=4, L=64), case_ce(1, P=300, L=64), case_ce(1, P=4, L=32), case_ce(1, P=4, L=64)])


def test_pipeline_workspace_grows_with_work_queued(make):
    grow_sequence(make, [case_retrieve_rerank(1, Q=4, pool=16), case_retrieve_rerank(1, Q=4, pool=128), case_retrieve_rerank(1, Q=4, pool=16)])


def test_two_handles_on_two_streams_at_once(make):
    """Two handles of one process on device 0 (dims 128 and 64, 7000 and 3000 rows, different cross-encoder weights), each
    on its own stream, their calls enqueued alternately behind busy work so that they run together. Each returns what it
    returns alone: nothing process-wide (function attributes, side stream, statics) leaks between handles."""
    import torch
    from optimized_rag_amd.bm25 import Bm25Postings
    w = world()
    rng = np.random.default_rng(55)
    D2, N2, Q, k = 64, 3000, 64, 10
    emb2 = rng.standard_normal((N2, D2)).astype(np.float32)
    q2 = (emb2[:Q] + 0.3 * rng.standard_normal((Q, D2))).astype(np.float32)
    post2 = Bm25Postings.from_corpus(w["corpus"][:N2])
    ptr2, terms2 = post2.encode_queries(w["queries"][:Q])
    cp = pairs(rng, 64, 64)

    def second():
        e = make(dim=D2, bm25_plan_slots=8, ce_chunk_tokens=4096)
        e.index_load(emb2)
        post2.load(e)
        e.ce_load(CE_CFG, w["ce_t2"])
        return e

    def run(eng, d, s):
        ids, rows, sc = out((Q, k), torch.int64), out((Q, k), torch.int32), out((Q, k), torch.float64)
        lg = out((64,), torch.float32)
        eng.dense_topk_dev(d["q"], k, ids, rows, sc, stream=s)
        hy = eng.hybrid_rrf_dev(d["q"], d["ptr"], d["terms"], 20, k, stream=s)
        eng.ce_score_dev(d["ids"], d["tt"], d["lens"], lg, stream=s)
        return [ids, rows, sc, lg] + [t.clone() for t in hy]

    in1 = dict(q=w["q"][:Q], **real_terms(Q), **cp)
    in2 = dict(q=q2, ptr=ptr2, terms=terms2, **cp)
    parts1 = ("index", "bm25", "ce")
    opts1 = dict(bm25_plan_slots=8, ce_chunk_tokens=4096)
    ref1 = T.to_np(run(make(*parts1, **opts1), T.to_dev(in1), None))
    ref2 = T.to_np(run(second(), T.to_dev(in2), None))
    torch.cuda.synchronize()
    e1, e2 = make(*parts1, **opts1), second()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    d1, d2 = T.to_dev(in1), T.to_dev(in2)
    torch.cuda.synchronize()
    T.busy(s1)
    T.busy(s2)
    got1, got2 = [], []
    for _ in range(2):
        with torch.cuda.stream(s1):
            got1 = [o.clone() for o in run(e1, d1, s1)]
        with torch.cuda.stream(s2):
            got2 = [o.clone() for o in run(e2, d2, s2)]
    s1.synchronize()
    s2.synchronize()
    T.assert_same(T.to_np(got1), ref1, "handle 1")
    T.assert_same(T.to_np(got2), ref2, "handle 2")
