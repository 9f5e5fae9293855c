"""No call's result depends on the calls its handle served before.

Almost every other GPU test builds a handle, makes one call of one shape and compares. The library keeps grow-only device
buffers per handle (tests/test_workspace_table_cpu.py lists them) that every call carves anew by its own shape, and
`dev_buf::reserve` keeps no contents. Here one handle serves a SEQUENCE of calls of different shapes on one side stream, behind
busy work and with nothing synchronising in between (the `grow_sequence` of tests/test_stream_order_gpu.py), and every result
is compared bit for bit with the same call made alone on a fresh handle. The case builders, the 5000-row world and the
shapes (Q = 40, QBIG = 300) are those of tests/test_stream_order_resident_gpu.py; the builders defined here only add the
arguments those lack (pool, k, a query selection).

A sequence is small -> large -> small: the large call must re-allocate what the small one carved (a pointer carved before the
re-allocation would then be stale), and the second small call runs on a buffer whose bytes the large one wrote. That the large
call really exceeds the small one's carve is not taken on trust: SEQUENCES gives, per sequence, the buffer and its byte counts
for the small and the large shape, computed by the functions below that restate the carve functions of the library
(256-byte planes, common.h stage_size), and test_the_large_call_exceeds_the_small_carve asserts large > small for each.

  pipe_ws, P = Q * pool, PS = Q * S, S = 2 * pool in mode 2 and pool otherwise (pipeline.hip):
    cand_ws_planes      lists 16 P | scores 8 P | cand 8 PS | rrf 8 PS | ranks 8 PS | (narrow) rows 4 PS
    m3_retrieve_planes  cand_ws_planes (narrow) | dense 8 PS | sparse 8 PS
                        Q = 300, pool 50: modes 0 / 1 1,020,672 B, mode 2 1,680,896 B; Q = 8: 28,160 B and 45,056 B
                        Q = 300, mode 2: pool 16 537,600 B, pool 128 4,300,800 B
    retrieve_maxsim     cand_ws_planes (narrow): Q = 8 21,504 B, Q = 300 780,544 B
    retrieve_rerank     cand_ws_planes | ids 4 P L | types 4 P L | lengths 4 P | logits 4 P (Q = 12, pool 16, L = 32: 59,904 B)
    m3_score_rows       dense 8 P | sparse 8 P: Q = 4 3,584 B, Q = 40 32,256 B
    m3_score_ids        rows 4 P | dense 8 P | sparse 8 P at P = Q * 100: Q = 4 8,448 B, Q = 40 80,128 B
    m3_candidates       rrf 8 Q S (modes 1, 2): Q = 4 3,328 B, Q = 40 32,000 B
    search_m3_tokens    m3_retrieve_planes | dense 4 Q H | lex 4 Q L | ptr 4 (Q + 1) | terms 4 Q L | weights 4 Q L | tok 4 Q (L - 1) T |
                        offsets 8 (Q + 1), H = 128, L = 40, T = 64: Q = 4, mode 2 68,352 B; Q = 40: mode 2 664,064 B, mode 0
                        576,768 B, pool 16 511,488 B, pool 128 1,013,248 B
  tv_ws (tokvec.hip tokvec_score_slots): scores 4 P | slots 4 P: Q = 4 2,048 B, Q = 40 16,384 B
  qten (dense.hip stage_query_tenants): 4 B x Q rounded up to 1024 queries: 4,096 B up to 1024 queries, 8,192 B at 1100
  the dense ws / exact / flag set (dense.hip): sized by the query count rounded up to the 256-query tile: 8 -> 256, 300 -> 512
  scan_scores (dense.hip exact_scan_rounds, every query through the float64 scan under force_level = 2): round_q x n_blocks x k x 12 B
                        with window = 2048 - k, rows per block = (n / 1024 rounded up + window - 1) rounded down to the window, n_blocks =
                        n / that rounded up, round_q = min(Q, max(256, min(65535, 512 MB / (n_blocks x k x 12)))). At 5000 rows, k = 10:
                        3 blocks, round_q = Q: Q = 8 2,880 B, Q = 300 108,000 B
  ix->ws of a keyword index (bm25.hip bm25_ws_planes, the device entries): partial keys 8 Q R k | partial rows 4 Q R k | counts 4 Q R |
                        running keys 8 Q k | running rows 4 Q k | tau 8 Q | plan offsets 4 Q t (R + 1) | plan metadata 16 Q 64, R = 3
                        ranges of 2048 documents (no tail segment), t = the planned slots per query (1 to 64, chosen per call; the
                        tests of the keyword search force 8); the all-document scoring of the linear fusion has no partial and no
                        running lists. Top-k, k = 10: Q = 8 at most 21,248 B (t = 64), Q = 300 at least 462,848 B (t = 1).
                        All-document scoring, t = 8: Q = 8 9,728 B, Q = 256 300,032 B
  lin_ws (api.hip linear_carve) is sized by the ROW count and the sub-batch (256 queries at 5000 rows; ld = 6144, the fp16 plane's rows):
                        10,240,000 + 6,291,456 + 2 x 2,048 + 2 x 1,024 + 24,576 + 1,280 + 262,144 = 16,825,600 B whatever Q is. The
                        linear sequences therefore grow the dense set, ix->ws and qten around a lin_ws that stays; lin_ws with another
                        row count is tests/test_state_history_gpu.py.
  No library buffer grows in the sequences marked None in SEQUENCES: maxsim_dev, sparse_score_rows_dev, lexical_match_dev and
  lexical_compact_dev work in the caller's buffers alone, and k changes only the outputs of the two composites (their carve
  depends on Q, pool and mode). These sequences check that a call of another shape in between changes nothing; no size is asserted.

Measured on an MI355X, one run (also in DESIGN.md section 4.7): the 34 tests of this file in 5 s, none above 2.1 s (none among
the 60 slowest of the whole suite). Every test passed on the library as it stood: no result depended on the handle's earlier calls.

Mutants (value-only, built aside, each run once against this file and tests/test_state_history_gpu.py):
  the per-call upload of qten skipped              FAILS [hybrid_rrf_tenants_dev], [hybrid_linear_tenants_dev], [hybrid_linear_chain-tenants],
                                                   [sparse_topk_tenants_dev], [retrieve_m3_tenants_dev], [search_m3_tokens_tenants_dev] and
                                                   test_a_one_call_fusion_between_begin_and_finish_drops_the_pair
  the q16_dirty clear of dense.hip dropped         SURVIVES: the stale query rows are columns >= q_valid, which every epilogue skips
  the zero fill of lin_ws on growth dropped        SURVIVES, with a reservation: the pad rows it zeroes are masked (tests/test_state_history_gpu.py:
                                                   after rag_index_load of a smaller index they hold Inf / NaN and change nothing), but what
                                                   the mutant's fresh allocations held was whatever hipMalloc returned, which no test controls
  lin_begun.on kept across a lin_ws re-allocation  SURVIVES: lin_ws grows only after a host call or a live write, which drop the pair first
"""
import numpy as np
import pytest

import stream_tools as T
import test_stream_order_resident_gpu as R

pytestmark = pytest.mark.gpu

make = R.make
Case = R.Case
out = R.out
Q, QBIG, POOL, K = R.Q, R.QBIG, R.POOL, R.K
SMALL = 4
H, LT, TOK = R.DE, R.LT, R.TOK
QTEN = 1100                                      # past the 1024 queries qten is first reserved for


# ---- the carve functions, restated ----------------------------------------------------------------------------------------------------
def plane(n, elt):
    return -(-(n * elt) // 256) * 256


def cand_bytes(P, PS, narrow):
    return plane(2 * P, 8) + plane(P, 8) + 2 * plane(PS, 8) + plane(2 * PS, 4) + (plane(PS, 4) if narrow else 0)


def m3_bytes(n, pool=POOL, mode=2):
    P, PS = n * pool, n * pool * (2 if mode == 2 else 1)
    return cand_bytes(P, PS, True) + 2 * plane(PS, 8)


def maxsim_bytes(n, pool=POOL):
    return cand_bytes(n * pool, n * pool, True)


def rerank_bytes(n, pool, L):
    P = n * pool
    return cand_bytes(P, P, False) + 2 * plane(P * L, 4) + 2 * plane(P, 4)


def score_rows_bytes(n, pool=POOL):
    return 2 * plane(n * pool, 8)


def score_ids_bytes(n, width=2 * POOL):
    return plane(n * width, 4) + 2 * plane(n * width, 8)


def tokens_bytes(n, pool=POOL, mode=2):
    return (m3_bytes(n, pool, mode) + plane(n * H, 4) + plane(n * LT, 4) + plane(n + 1, 4) + 2 * plane(n * LT, 4) +
            plane(n * (LT - 1) * TOK, 4) + plane(n + 1, 8))


def tv_bytes(n, pool=POOL):
    return 2 * plane(n * pool, 4)


def qten_bytes(n):
    return 4 * (-(-n // 1024) * 1024)


def dense_rows(n):
    return -(-n // 256) * 256


def keyword_bytes(n, k=K, topk=True, plan_t=8, ranges=3):
    """bm25_ws_planes for a device entry: topk (mode 0) or the all-document scoring (mode 1); BM_PLAN_T = 64, bm_plan_meta 16 B"""
    n_cnt = n * ranges
    n_part, n_out = (n_cnt * k, n * k) if topk else (0, 0)
    return (plane(n_part, 8) + plane(n_part, 4) + plane(n_cnt, 4) + plane(n_out, 8) + plane(n_out, 4) + plane(n, 8) +
            plane(n * plan_t * (ranges + 1), 4) + plane(n * 64, 16))


def scan_bytes(n, k=K, n_rows=R.N):
    """the scan_scores reserve of dense.hip exact_scan_rounds (SCAN_CHUNK 2048, SCAN_ROUND 256)"""
    window = 2048 - k
    rows_per_block = max(1, (n_rows + 1023) // 1024 + window - 1) // window * window
    n_blocks = -(-n_rows // rows_per_block)
    round_q = min(n, max(256, min(65535, (512 << 20) // (n_blocks * k * 12))))
    return round_q * n_blocks * k * 12


def embed_tokens(n, L=LT):
    """the token rows of the embedder's workspace (cross_encoder.hip ws_renew: P x L rounded up to 256)"""
    return -(-(n * L) // 256) * 256


def linear_bytes(n_rows, ld, qb=256):
    return (plane(qb * n_rows, 8) + plane(qb * ld, 4) + 2 * plane(qb, 8) + 2 * plane(qb, 4) + plane(ld, 4) + plane(qb + 1, 4) +
            plane(qb * 256, 4))


# ---- builders with the arguments tests/test_stream_order_resident_gpu.py fixes ----------------------------------------------------------
def case_m3(mode, n=QBIG, pool=POOL, k=K, per_query=False):
    """R.case_retrieve_m3 with pool and k"""
    ten = R.tenants_of(per_query, n)
    real = dict(**R.dense(n), **R.lex(n), **R.vecs(n))

    def bind(eng):
        def call(d, s):
            return list(eng.retrieve_m3_dev(d["q"], pool, k, term_ptr=d["ptr"], terms=d["terms"], weights=d["w"], q_vecs=d["qv"], q_off=d["qo"],
                                            mode=mode, w=R.W3, tenant=ten, stream=s))
        return call
    return Case(("index", "tenants", "sparse", "tokvec"), {}, R.blank(real, terms=-1), real, bind)


def case_m3_tokens(mode, n=Q, pool=POOL, k=K, per_query=False):
    """R.case_search_m3_tokens with pool and k"""
    ten = R.tenants_of(per_query, n)
    real, wrong = R.token_inputs(n)

    def bind(eng):
        def call(d, s):
            return list(eng.search_m3_tokens_dev(d["ids"], d["tt"], d["lens"], pool, k, skip_ids=R.SKIP, mode=mode, w=R.W3, tenant=ten, stream=s))
        return call
    return Case(("index", "tenants", "sparse", "tokvec", "embedder"), {}, wrong, real, bind)


def case_rrf_tenants(n, shift=0):
    """R.case_hybrid_rrf with per-query tenants over n queries drawn (with repeats) from the QBIG of the world; the tenants are
    those of the queries `shift` places on, so that two calls give different tenants to the same slot of qten"""
    sel = np.arange(n) % QBIG
    ten = R.tenants_of(True, n, sel=(np.arange(n) + shift) % QBIG)
    real = dict(**R.dense(n, sel=sel), **R.keywords(n, sel))

    def bind(eng):
        def call(d, s):
            return list(eng.hybrid_rrf_dev(d["q"], d["ptr"], d["terms"], POOL, K, tenant=ten, stream=s))
        return call
    return Case(("index", "tenants", "bm25"), dict(bm25_plan_slots=8), R.blank(real, terms=-1), real, bind)


def chain_explicit_ids(n):
    """R.case_shard_chain on three shards loaded with explicit ids and the id map (m3_score_ids_dev looks its candidates up there)"""
    return R.case_shard_chain(2, n)._replace(parts=("shards", "ids", "sparse", "tokvec"))


def sml(build, small=SMALL, large=Q):
    """small -> large -> the same small again"""
    a = build(small)
    return [a, build(large), a]


# name -> (cases(), the buffer whose growth the sequence is about, its size for the small and for the large call; None, None where
# no library buffer grows). The keyword sizes are the most the small call can ask against the least the large one can (t above).
SEQUENCES = {
    "dense_topk_tenants_dev-exact_scan": (lambda: sml(lambda n: R.case_dense_tenants(n)._replace(options=dict(force_level=2)), 8, QBIG),
                                          "scan_scores", scan_bytes(8), scan_bytes(QBIG)),
    "sparse_topk_dev": (lambda: [R.case_sparse_topk(n=8), R.case_sparse_topk(n=QBIG), R.case_sparse_topk(n=8, first=8)],
                        "ix->ws", keyword_bytes(8, plan_t=64), keyword_bytes(QBIG, plan_t=1)),
    "sparse_topk_tenants_dev": (lambda: [R.case_sparse_topk(True, n=8), R.case_sparse_topk(True, n=QBIG), R.case_sparse_topk(True, n=8, first=8)],
                                "ix->ws", keyword_bytes(8, plan_t=64), keyword_bytes(QBIG, plan_t=1)),
    "hybrid_sparse_rrf_dev": (lambda: sml(lambda n: R.case_hybrid_sparse_rrf(n=n), 8, QBIG), "dense rows", dense_rows(8), dense_rows(QBIG)),
    "hybrid_rrf_tenants_dev": (lambda: [case_rrf_tenants(8), case_rrf_tenants(QTEN, 1), case_rrf_tenants(8)],
                               "qten", qten_bytes(8), qten_bytes(QTEN)),
    "hybrid_linear_tenants_dev": (lambda: [R.case_hybrid_linear_tenants(n=8), R.case_hybrid_linear_tenants(n=QBIG),
                                           R.case_hybrid_linear_tenants(n=8, sel=list(range(8))[::-1])],
                                  "dense rows", dense_rows(8), dense_rows(QBIG)),
    "hybrid_linear_chain": (lambda: [R.case_linear_chain(n=8), R.case_linear_chain(n=256, sel=np.arange(256)), R.case_linear_chain(n=8, sel=list(range(8))[::-1])],
                            "ix->ws", keyword_bytes(8, topk=False), keyword_bytes(256, topk=False)),
    "hybrid_linear_chain-tenants": (lambda: [R.case_linear_chain(True, n=8), R.case_linear_chain(True, n=256, sel=np.arange(256)),
                                             R.case_linear_chain(True, n=8, sel=list(range(8))[::-1])],
                                    "ix->ws", keyword_bytes(8, topk=False), keyword_bytes(256, topk=False)),
    "tokvec_rerank_dev-fp16": (lambda: [R.case_tokvec_rerank(n=SMALL), R.case_tokvec_rerank(n=Q), R.case_tokvec_rerank(n=SMALL, first=9)],
                               "tv_ws", tv_bytes(SMALL), tv_bytes(Q)),
    "tokvec_rerank_dev-mxfp8": (lambda: [R.case_tokvec_rerank("tokvec8", n=SMALL), R.case_tokvec_rerank("tokvec8", n=Q),
                                         R.case_tokvec_rerank("tokvec8", n=SMALL, first=9)], "tv_ws", tv_bytes(SMALL), tv_bytes(Q)),
    "retrieve_maxsim_dev": (lambda: sml(lambda n: R.case_retrieve_maxsim(n=n), 8, QBIG), "pipe_ws", maxsim_bytes(8), maxsim_bytes(QBIG)),
    "maxsim_dev": (lambda: sml(R.case_maxsim), None, None, None),
    "retrieve_m3_dev-count": (lambda: sml(lambda n: case_m3(2, n), 8, QBIG), "pipe_ws", m3_bytes(8), m3_bytes(QBIG)),
    "retrieve_m3_dev-mode_0_2_0": (lambda: sml(lambda m: case_m3(m), 0, 2), "pipe_ws", m3_bytes(QBIG, mode=0), m3_bytes(QBIG, mode=2)),
    "retrieve_m3_dev-mode_1_2_1": (lambda: sml(lambda m: case_m3(m), 1, 2), "pipe_ws", m3_bytes(QBIG, mode=1), m3_bytes(QBIG, mode=2)),
    "retrieve_m3_dev-pool": (lambda: sml(lambda p: case_m3(2, pool=p, k=5), 16, 128), "pipe_ws", m3_bytes(QBIG, 16), m3_bytes(QBIG, 128)),
    "retrieve_m3_dev-k": (lambda: sml(lambda k: case_m3(2, pool=128, k=k), 5, 100), None, None, None),
    "retrieve_m3_tenants_dev": (lambda: sml(lambda n: case_m3(2, n, per_query=True), 8, QBIG), "pipe_ws", m3_bytes(8), m3_bytes(QBIG)),
    "search_m3_tokens_dev-count": (lambda: sml(lambda n: case_m3_tokens(2, n)), "pipe_ws", tokens_bytes(SMALL), tokens_bytes(Q)),
    "search_m3_tokens_dev-mode_0_2_0": (lambda: sml(lambda m: case_m3_tokens(m), 0, 2), "pipe_ws", tokens_bytes(Q, mode=0), tokens_bytes(Q, mode=2)),
    "search_m3_tokens_dev-mode_1_2_1": (lambda: sml(lambda m: case_m3_tokens(m), 1, 2), "pipe_ws", tokens_bytes(Q, mode=1), tokens_bytes(Q, mode=2)),
    "search_m3_tokens_dev-pool": (lambda: sml(lambda p: case_m3_tokens(2, pool=p, k=5), 16, 128), "pipe_ws", tokens_bytes(Q, 16), tokens_bytes(Q, 128)),
    "search_m3_tokens_dev-k": (lambda: sml(lambda k: case_m3_tokens(2, pool=128, k=k), 5, 100), None, None, None),
    "search_m3_tokens_tenants_dev": (lambda: sml(lambda n: case_m3_tokens(2, n, per_query=True)), "pipe_ws", tokens_bytes(SMALL), tokens_bytes(Q)),
    "m3_shard_chain-implicit_ids": (lambda: sml(lambda n: R.case_shard_chain(2, n)), "pipe_ws", score_ids_bytes(SMALL), score_ids_bytes(Q)),
    "m3_shard_chain-explicit_ids": (lambda: sml(chain_explicit_ids), "pipe_ws", score_ids_bytes(SMALL), score_ids_bytes(Q)),
    "sparse_score_rows_dev": (lambda: sml(R.case_sparse_score_rows), None, None, None),
    "m3_score_rows_dev": (lambda: sml(lambda n: R.case_m3_score_rows(R.W3, n)), "pipe_ws", score_rows_bytes(SMALL), score_rows_bytes(Q)),
    "lexical_match_dev": (lambda: sml(R.case_lexical_match), None, None, None),
    "lexical_compact_dev": (lambda: sml(R.case_lexical_compact), None, None, None),
    "embed_multi_dev": (lambda: sml(R.case_embed_multi), "the token rows of the embedder's workspace", embed_tokens(SMALL), embed_tokens(Q)),
}


def test_the_large_call_exceeds_the_small_carve():
    """(needs no device, but belongs to the table above) The byte counts of the module docstring, from the functions that restate
    the carves; every sequence's large call is larger than its small one in the buffer it is about."""
    assert (m3_bytes(QBIG, mode=0), m3_bytes(QBIG, mode=1), m3_bytes(QBIG, mode=2)) == (1_020_672, 1_020_672, 1_680_896)
    assert (m3_bytes(8, mode=0), m3_bytes(8)) == (28_160, 45_056)
    assert (m3_bytes(QBIG, 16), m3_bytes(QBIG, 128)) == (537_600, 4_300_800)
    assert (maxsim_bytes(8), maxsim_bytes(QBIG)) == (21_504, 780_544)
    assert rerank_bytes(12, 16, 32) == 59_904
    assert (score_rows_bytes(SMALL), score_rows_bytes(Q)) == (3_584, 32_256)
    assert (score_ids_bytes(SMALL), score_ids_bytes(Q)) == (8_448, 80_128)
    assert (plane(SMALL * 2 * POOL, 8), plane(Q * 2 * POOL, 8)) == (3_328, 32_000)
    assert (tokens_bytes(SMALL), tokens_bytes(Q)) == (68_352, 664_064)
    assert (tv_bytes(SMALL), tv_bytes(Q)) == (2_048, 16_384)
    assert (qten_bytes(8), qten_bytes(1024), qten_bytes(QTEN)) == (4_096, 4_096, 8_192)
    assert linear_bytes(R.N, 6144) == 16_825_600
    assert (scan_bytes(8), scan_bytes(QBIG)) == (2_880, 108_000)
    assert (keyword_bytes(8, plan_t=64), keyword_bytes(QBIG, plan_t=1)) == (21_248, 462_848)
    assert (keyword_bytes(8, topk=False), keyword_bytes(256, topk=False)) == (9_728, 300_032)
    for name, (_, what, small, large) in SEQUENCES.items():
        assert what is None or large > small, f"{name}: the large call asks {large} of {what}, the small one {small}"


def history(make, cases):
    """Every case of `cases` in turn on one handle and one side stream behind busy work, nothing synchronising in between; each
    equals the same call alone on a handle of its own (one reference per distinct case)."""
    import torch
    parts = tuple(sorted(set().union(*[set(c.parts) for c in cases])))
    options = {k: v for c in cases for k, v in c.options.items()}
    refs = {}
    for c in cases:
        if id(c) not in refs:
            refs[id(c)] = T.to_np(c.bind(make(*parts, **options))(T.to_dev(c.real), None))
            torch.cuda.synchronize()
    eng = make(*parts, **options)
    s = torch.cuda.Stream()
    devs = [T.to_dev(c.real) for c in cases]
    calls = [c.bind(eng) for c in cases]
    torch.cuda.synchronize()
    got = []
    with torch.cuda.stream(s):
        T.busy(s, 50)
        for call, d in zip(calls, devs):
            got.append([o.clone() for o in call(d, s)])
    s.synchronize()
    for i, (g, c) in enumerate(zip(got, cases)):
        T.assert_same(T.to_np(g), refs[id(c)], f"call {i}")


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_small_large_small_on_one_handle(make, name):
    history(make, SEQUENCES[name][0]())


def test_one_pipeline_workspace_under_four_composites(make):
    """retrieve_rerank -> retrieve_m3 mode 2 -> retrieve_maxsim -> retrieve_rerank on one handle: the four carve pipe_ws by four
    layouts: rerank at Q = 12, pool 16, L = 32 takes 59,904 B; m3 at Q = 300, pool 50 takes 1,680,896 B, which re-allocates it; maxsim
    at Q = 300 takes 780,544 B of that; rerank again its first 59,904 B."""
    assert rerank_bytes(12, 16, 32) < maxsim_bytes(QBIG) < m3_bytes(QBIG)
    a = R.case_retrieve_rerank_tenants()
    history(make, [a, case_m3(2), R.case_retrieve_maxsim(), a])


def test_a_one_call_fusion_between_begin_and_finish_drops_the_pair(make):
    """begin (8 queries) -> rag_hybrid_linear_dev (300 queries) -> finish: the one-call entry overwrites the score planes, so finish is
    RAG_ERR_STATE (include/rag_hip.h), the one-call result is right, and the next begin -> finish pair is right."""
    import torch
    from optimized_rag_amd import RagError
    parts, options = ("index", "tenants", "bm25", "temporal"), dict(bm25_plan_slots=8)
    lin = dict(**R.dense(8), **R.keywords(8))
    big = R.case_hybrid_linear_tenants(n=QBIG)
    ref_eng = make(*parts, **options)
    ref_pair, _ = R.halves(ref_eng, T.to_dev(lin), 8, None)
    ref_pair = T.to_np(ref_pair)
    ref_big = T.to_np(big.bind(make(*parts, **options))(T.to_dev(big.real), None))
    torch.cuda.synchronize()
    eng = make(*parts, **options)
    d, dbig = T.to_dev(lin), T.to_dev(big.real)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        T.busy(s, 50)
        mx, gmx, part = out((8,), torch.float64), out((1, 8), torch.float64), out((5, 8, K), torch.int64)
        eng.hybrid_linear_begin_dev(d["ptr"], d["terms"], mx, stream=s)
        got_big = [o.clone() for o in big.bind(eng)(dbig, s)]
        gmx[0].copy_(mx)
        with pytest.raises(RagError, match=r"\(-3\)"):
            eng.hybrid_linear_finish_dev(d["q"], gmx, K, 0.6, 0.3, 0.1, part, stream=s)
        got_pair, _ = R.halves(eng, d, 8, s)
    s.synchronize()
    T.assert_same(T.to_np(got_big), ref_big, "the one-call fusion after a begin")
    T.assert_same(T.to_np(got_pair), ref_pair, "begin -> finish after the refusal")
