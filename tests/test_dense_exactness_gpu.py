"""GPU: the dense search's exactness proof under pressure.

The search promises the float64 scan's result because a row is dropped only when its fp16-pass score S~ is below
tau = s~(k) - 2 * eps, with |S~ - S| <= eps (comment above select_kernel, csrc/dense.hip). On Gaussian data |S~ - S| is a
hundredth of eps, so nothing tests that inequality. Here the corpus holds the worst-case rows of tests/fp16_adversary.py:
"minus" rows that belong in the exact top-k and sit ~1.3 to 1.5 analytic bounds below the k-th fp16 score. A threshold one
bound below s~(k), an eps a tenth of its value or a fused bound without its |alpha| factor loses them.
Every case first asserts its CPU preconditions over its whole corpus (fp16_adversary.check_case), then compares the engine
with the float64 oracle: rows and ids equal, scores within 1e-9; and asserts from dense_stats() which path answered.
Further down: the float32 range (rows and queries from denormals to just below overflow) and the side terms of the fused
linear-hybrid bound (negative weights, large temporal scores, negative BM25 scores of any magnitude)."""
import numpy as np
import pytest

import fp16_adversary as A
from oracle import rag_oracle as O

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-9          # float64 on both sides, different summation order (tests/test_dense_gpu.py)


@pytest.fixture(scope="module")
def eng_factory():
    from optimized_rag_amd import RagEngine
    made = []

    def make(dim, **options):
        e = RagEngine(dim=dim, device=0)
        made.append(e)
        for name, value in options.items():
            e.set_option(name, value)
        return e

    yield make
    for e in made:
        e.close()


def visible_case(case, visible):
    """The case as the search sees it under a tenant filter / after deletes: only the visible rows, renumbered."""
    new = np.cumsum(visible) - 1
    assert all(visible[r].all() for r in case.plus_rows + case.minus_rows)
    return A.Case(case.corpus[visible], case.queries, [new[r] for r in case.plus_rows], [new[r] for r in case.minus_rows], case.k)


def compare(eng, corpus, queries, k, visible=None, tenant=-1):
    got_ids, got_rows, got_sc = eng.dense_topk(queries, k, tenant=tenant)
    if visible is None:
        oid, osc = O.dense_topk(corpus, queries, k)
    else:
        oid, osc = O.dense_topk(corpus, queries, k, visible.astype(np.int32), 1)
    np.testing.assert_array_equal(got_rows, oid.astype(np.int32))
    np.testing.assert_array_equal(got_ids, oid)
    np.testing.assert_allclose(got_sc, osc, rtol=0, atol=SCORE_TOL)
    st = eng.dense_stats()
    assert st["proven_fast"] + st["proven_wide"] + st["exact_scan"] == queries.shape[0], st
    return st


def run_case(eng, case, visible=None, tenant=-1, scan_ok=False):
    """CPU preconditions over what the search sees, then the engine against the oracle. Returns (stats, measured figures)."""
    m = A.check_case(case if visible is None else visible_case(case, visible))
    st = compare(eng, case.corpus, case.queries, case.k, visible, tenant)
    assert st["eps"] >= m["E"], (st, m)                    # the code's bound covers the analytic one
    assert m["gap"] < 2.0 * st["eps"], (st, m)             # the proof's own precondition: if this fails the CASE is wrong
    if not scan_ok:
        assert st["exact_scan"] == 0, st                   # answered by the proof, not rescued by the float64 scan
    return st, m


# ----------------------------------------------------------------------------------------------------------- emit threshold
@pytest.mark.parametrize("N,k,minus_at,stages", [
    (40000, 100, 40000 - 1, 3),          # last tile of the table, last stage (stages: tiles 0-7, 8-79, 80-156)
    (40000, 100, 12000, 3),              # the middle of stage 1
    (40000, 100, 30000, 3),              # the middle of stage 2
    (2305, 20, 2304, 2),                 # the trailing stage that stands on its own
])
@pytest.mark.parametrize("linear", [1, 0])
def test_emit_threshold_keeps_the_minus_row(eng_factory, N, k, minus_at, stages, linear):
    """Table order (dense_linear_order): the k plus rows are among the first 2048 rows, so tau = s~(k) - 2 eps is set from them
    after stage 0 and the minus row, scored in a later stage, meets the emission compare itself. The same data in the default
    permuted tile order: whichever stage scores it, the row must come back."""
    case = A.make_case(N + minus_at, 64, k, 1, 0.19, N, plus_at=700, minus_at=minus_at)
    eng = eng_factory(64, dense_linear_order=linear)
    eng.index_load(case.corpus)
    st, _ = run_case(eng, case)
    assert st["stages"] == stages and st["overflowed"] == 0, st


# --------------------------------------------------------------------------------------------------------- select compaction
@pytest.mark.parametrize("N,plus_at,stages", [(2000, 300, 1), (40000, 20000, 2)])
def test_select_compaction_keeps_the_minus_rows(eng_factory, N, plus_at, stages):
    """Plus and minus rows inside ONE stage: the emission sees the previous stage's threshold (none at all in stage 0), and it
    is the compaction at the end of select_wave, with the tau it has just computed, that must keep the minus rows."""
    k, n_minus = 20, 3
    case = A.make_case(N, 64, k, 1, 0.19, N, plus_at=plus_at, minus_at=plus_at + k + 4, n_minus=n_minus)
    eng = eng_factory(64, dense_linear_order=1)
    eng.index_load(case.corpus)
    st, _ = run_case(eng, case)
    assert st["stages"] == stages, st


# -------------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("dim,k,Q,cosine,N", A.SHAPES)
def test_shapes(eng_factory, dim, k, Q, cosine, N):
    """dim (64 and 1536: tile multiples, 100 and 384: padded), k from 1 to the maximum, one query (small-batch kernel), 130 (one
    full query tile) and 300 (two query tiles). Every query is its own family, drawn with its own positions and signs, so one
    query's plus rows are background for the others. Plus rows at the head of the table, minus rows in its last tiles."""
    case = A.make_case(1000 + dim + k + Q, dim, k, Q, cosine, N)
    eng = eng_factory(dim, dense_linear_order=1)
    eng.index_load(case.corpus)
    st, m = run_case(eng, case)
    assert st["stages"] >= 2 and st["overflowed"] == 0, st
    print(f"dim {dim} k {k} Q {Q}: gap {m['gap_ratio']:.3f} E = {m['gap'] / st['eps']:.3f} eps, eps = {st['eps']:.4e}")


# ------------------------------------------------------------------------------------------------ wide path and second pass
def test_more_than_256_tied_plus_rows_take_the_wide_path(eng_factory):
    case = A.make_case(11, 64, 20, 1, 0.19, 6000, n_plus=300, n_minus=2)
    eng = eng_factory(64, dense_linear_order=1)
    eng.index_load(case.corpus)
    st, _ = run_case(eng, case)
    assert st["proven_wide"] >= 1, st


def _overflow_case():
    # stage 0 (rows 0..2047) sees only rows far below everything else, so the one threshold stage that follows emits all
    # ~7,000 remaining rows into the 4096-entry buffer; the family sits at the end of the table
    def offset(rng, n):
        return np.where(np.arange(n) < 2048, rng.uniform(0.3, 0.5, n), rng.uniform(0.05, 0.1, n))
    return A.make_case(12, 64, 20, 1, 0.19, 9000, plus_at=8900, n_minus=2, offset=offset)


def test_second_pass_re_emission_keeps_the_minus_rows(eng_factory):
    """Forced overflow (stage_growth): the select tightens tau from the 4096 keys that were kept, the second MFMA pass re-emits
    at that tau, and its select - now with the plus rows among the keys - must keep the minus rows at the final tau."""
    case = _overflow_case()
    eng = eng_factory(64, dense_linear_order=1, stage_growth=100000)
    eng.index_load(case.corpus)
    st, _ = run_case(eng, case)
    assert st["overflowed"] >= 1 and st["second_pass"] == st["overflowed"], st


@pytest.mark.parametrize("level", [1, 2])
def test_forced_levels_give_the_same_output(eng_factory, level):
    case = _overflow_case()
    eng = eng_factory(64, dense_linear_order=1)
    eng.index_load(case.corpus)
    ref = eng.dense_topk(case.queries, case.k)
    eng.set_option("force_level", level)
    st, _ = run_case(eng, case, scan_ok=True)
    assert st["proven_fast"] == 0 and (level == 1 or st["exact_scan"] == 1), st
    for a, b in zip(ref, eng.dense_topk(case.queries, case.k)):
        np.testing.assert_array_equal(a, b)


# --------------------------------------------------------------------------------------------------------------- fix-up path
def test_tenant_filter_and_deleted_rows(eng_factory):
    """The emission's fix-up loop (tenant filter, deleted rows): the family belongs to tenant 1, the background is spread over
    three tenants, so the minus rows' tile also holds foreign rows. Then 900 background rows are deleted, then the plus rows:
    the minus rows lead and the rest must rank by the oracle of the live rows."""
    N, k = 6000, 20
    case = A.make_case(13, 64, k, 1, 0.19, N, plus_at=500, n_minus=3)
    rng = np.random.default_rng(13)
    tenants = rng.integers(0, 3, N).astype(np.int32)
    tenants[case.plus_rows[0]] = tenants[case.minus_rows[0]] = 1
    eng = eng_factory(64, dense_linear_order=1)
    eng.index_load(case.corpus)
    eng.set_tenants(tenants)
    st, _ = run_case(eng, case, visible=tenants == 1, tenant=1)
    assert st["stages"] >= 2, st
    alive = np.ones(N, dtype=bool)
    family = np.concatenate([case.plus_rows[0], case.minus_rows[0]])
    dead = rng.choice(np.setdiff1d(np.arange(N), family), 900, replace=False)
    alive[dead] = False
    assert eng.index_delete(dead) == 900
    run_case(eng, case, visible=alive)
    run_case(eng, case, visible=alive & (tenants == 1), tenant=1)
    assert eng.index_delete(case.plus_rows[0]) == len(case.plus_rows[0])
    alive[case.plus_rows[0]] = False
    st = compare(eng, case.corpus, case.queries, k, visible=alive)
    assert st["exact_scan"] == 0, st
    got_rows = eng.dense_topk(case.queries, k)[1]
    assert got_rows[0, :3].tolist() == case.minus_rows[0].tolist()


# ------------------------------------------------------------------------------------------------- through the fused kernel
def _no_match_postings(n_docs):
    from optimized_rag_amd.bm25 import Bm25Postings
    indptr = np.asarray([0, 2, 3], dtype=np.int64)
    doc = np.asarray([1, 5, 7], dtype=np.int32)
    tf = np.ones(3, dtype=np.int32)
    doc_len = np.full(n_docs, 4, dtype=np.int32)
    return Bm25Postings(indptr, doc, tf, doc_len, Bm25Postings.idf_table(np.diff(indptr), n_docs), 4.0)


@pytest.mark.parametrize("alpha", [1.0, 0.25, 4.0])
def test_fused_kernel_scales_its_bound_with_alpha(eng_factory, alpha):
    """rag_hybrid_linear_dev with beta = gamma = 0 and queries that match nothing (every term out of vocabulary) is the dense
    search with its scores - and the adversarial gap - multiplied by alpha. Only an eps that carries |alpha| keeps the minus
    rows at alpha = 4. N > 2048, so a threshold stage runs."""
    import torch
    N, k, Q = 6000, 20, 3
    case = A.make_case(14, 384, k, Q, 0.25, N, n_minus=2)
    m = A.check_case(case)
    eng = eng_factory(384, dense_linear_order=1)
    eng.index_load(case.corpus)
    _no_match_postings(N).load(eng)
    ptr = torch.arange(Q + 1, dtype=torch.int32).cuda()
    terms = torch.full((Q,), -1, dtype=torch.int32).cuda()
    out = eng.hybrid_linear_dev(torch.from_numpy(case.queries).cuda(), ptr, terms, k, alpha, 0.0, 0.0)
    torch.cuda.synchronize()
    got = {key: v.cpu().numpy() for key, v in out.items()}
    st = eng.dense_stats()
    assert st["eps"] >= alpha * m["E"] and alpha * m["gap"] < 2.0 * st["eps"], (st, m)
    assert st["exact_scan"] == 0 and st["stages"] >= 2, st
    oid, osc = O.dense_topk(case.corpus, case.queries, k)
    np.testing.assert_array_equal(got["rows"], oid.astype(np.int32))
    np.testing.assert_array_equal(got["ids"], oid)
    np.testing.assert_allclose(got["hybrid"], (alpha * osc + 0.0 * 0.0) + 0.0 * 0.0, rtol=0, atol=SCORE_TOL)
    assert (got["keyword"] == 0.0).all() and (got["temporal"] == 0.0).all()
    if alpha == 1.0:
        for a, b in zip(eng.dense_topk(case.queries, k), (got["ids"], got["rows"])):
            np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------------------------ all cosines negative
def test_all_cosines_negative(eng_factory):
    """The query is the negated centroid of a one-sided corpus: every score is negative, so the ordered keys of negative floats
    decide, and with k above a tenant's live rows the -1 / 0.0 padding must follow them."""
    rng = np.random.default_rng(15)
    N, D = 6000, 64
    centroid = rng.standard_normal(D)
    corpus = (centroid[None, :] + 0.3 * rng.standard_normal((N, D))).astype(np.float32)
    queries = np.stack([-centroid, -centroid + 0.05 * rng.standard_normal(D)]).astype(np.float32)
    assert O.cosine_matrix(queries, corpus).max() < -0.5
    tenants = np.zeros(N, dtype=np.int32)
    few = np.asarray([5, 2050, 2304, 3000, 4444, 5998, 5999])
    tenants[few] = 1
    eng = eng_factory(D)
    eng.index_load(corpus)
    eng.set_tenants(tenants)
    st = compare(eng, corpus, queries, 20)
    assert st["exact_scan"] == 0, st
    compare(eng, corpus, queries, 20, visible=tenants == 1, tenant=1)
    ids, rows, sc = eng.dense_topk(queries, 20, tenant=1)
    assert (rows[:, 7:] == -1).all() and (ids[:, 7:] == -1).all() and (sc[:, 7:] == 0.0).all() and (sc[:, :7] < 0).all()
    compare(eng, corpus, queries, 256, visible=tenants == 0, tenant=0)


# --------------------------------------------------------------------------------------------------------- the float32 range
EXPONENTS = list(range(-140, 121, 20))       # 2^-140 (float32 denormals: 2^-149 is the smallest) ... 2^120 (norm just below overflow)


@pytest.mark.parametrize("dim", [64, 1536])
def test_float32_range_of_rows_and_queries(eng_factory, dim):
    """Rows and queries scaled by 2^-140 ... 2^120: the cosine does not depend on the scale, and the oracle is given the float32
    values that were stored (a denormal row has fewer significant bits, and the oracle sees the same bits). Every query has one
    planted neighbour per exponent, placed in late tiles of the table order, so each must pass a threshold stage's emission
    compare with the fp16 row that normalize_rows_kernel made of it. Searched with unscaled queries and with query j scaled
    by 2^EXPONENTS[j]. A row of denormals used to get an infinite float32 scale, an inf / NaN fp16 row, and was never emitted
    (the float64 scale fixes that). The same vectors through pairwise_cosine, float32 and float64, and one live insert of a
    denormal and a huge row."""
    rng = np.random.default_rng(dim)
    N, k, n_s = 3000, 20, len(EXPONENTS)
    corpus = rng.standard_normal((N, dim))
    base_q = rng.standard_normal((n_s, dim))
    planted = 2100 + np.arange(n_s * n_s) * 4                                # rows 2100 ... 2880: tiles 8 to 11
    for qi in range(n_s):
        for si, s in enumerate(EXPONENTS):
            corpus[planted[qi * n_s + si]] = (base_q[qi] + 0.2 * rng.standard_normal(dim)) * 2.0 ** s
    corpus = corpus.astype(np.float32)                                       # cast after scaling
    assert np.isfinite(corpus).all() and (np.abs(corpus[planted[0]]).max() < 1.2e-38) and (corpus[planted[0]] != 0).any()
    q_plain = base_q.astype(np.float32)
    q_scaled = (base_q * (2.0 ** np.asarray(EXPONENTS, dtype=np.float64))[:, None]).astype(np.float32)
    assert np.isfinite(q_scaled).all()
    eng = eng_factory(dim, dense_linear_order=1)
    eng.index_load(corpus)
    for queries in (q_plain, q_scaled):
        oid, _ = O.dense_topk(corpus, queries, k)
        for qi in range(n_s):                                                # the planted rows are what the oracle finds
            assert set(planted[qi * n_s:(qi + 1) * n_s].tolist()) <= set(oid[qi].tolist())
        st = compare(eng, corpus, queries, k)
        assert st["stages"] >= 2 and st["exact_scan"] == 0, st
    a, b = q_scaled, corpus[planted[:n_s]]
    np.testing.assert_allclose(eng.pairwise_cosine(a, b), O.cosine_matrix(a, b), rtol=0, atol=1e-12)
    np.testing.assert_allclose(eng.pairwise_cosine(a.astype(np.float64), b.astype(np.float64)), O.cosine_matrix(a, b), rtol=0, atol=1e-12)
    a64 = base_q * (2.0 ** np.asarray(EXPONENTS, dtype=np.float64))[:, None] * 2.0 ** -300       # float64 only: below float32's range
    np.testing.assert_allclose(eng.pairwise_cosine(a64, b.astype(np.float64)), O.cosine_matrix(a64, b), rtol=0, atol=1e-12)
    # live insert goes through dense_index_normalize_range: a denormal and a huge near-copy of queries 3 and 4
    new = np.stack([(base_q[3] + 0.1 * rng.standard_normal(dim)) * 2.0 ** -135, (base_q[4] + 0.1 * rng.standard_normal(dim)) * 2.0 ** 118]).astype(np.float32)
    assert eng.index_insert(new) == N
    grown = np.concatenate([corpus, new])
    oid, _ = O.dense_topk(grown, q_plain, k)
    assert oid[3, 0] == N and oid[4, 0] == N + 1
    compare(eng, grown, q_plain, k)


# ------------------------------------------------------------------------------------------- the fused bound's side terms
WEIGHTS = [(1, -0.5, 0.1), (0.5, 0.4, -0.3), (0.01, 1, 0), (4, 0.35, 0.1), (1e-3, 1e-3, 1)]


def _linear_oracle(post, emb, q, terms_of, temporal, a, b, g, k):
    out = []
    for qi, t in enumerate(terms_of):
        raw = O.bm25_scores_csr(post.indptr, post.doc, post.tf, post.doc_len, post.idf, post.avgdl, t)
        kw = raw / (raw.max() if raw.max() > 0 else 1.0)
        sem = O.cosine_matrix(q[qi:qi + 1], emb)[0]
        hyb = (a * sem + b * kw) + g * temporal
        out.append((raw, kw, hyb, O.stable_topk_desc(hyb, k + 1)))
    return out


def _check_linear(got, oracle, k):
    """Rows in the oracle's order, except that pairs closer than the float64 arithmetic can tell apart may swap (the rule of
    tests/test_property_gpu.py: 1e-12 for the cosine's summation order; plus two units in the last place of the hybrid score
    itself, which is 1.8e-12 at a temporal term of 1e4): compared as sets there. Keyword scores bit-identical."""
    for qi, (raw, kw, hyb, order) in enumerate(oracle):
        tol = 1e-12 + 2.0 ** -51 * float(np.abs(hyb[order]).max())
        rows = got["rows"][qi].tolist()
        h = hyb[order]
        gaps_ok = all(abs(h[j] - h[j + 1]) > tol or h[j] == h[j + 1] for j in range(k))
        if gaps_ok:
            assert rows == order[:k].tolist(), (qi, rows, order[:k].tolist())
        else:
            assert sorted(rows) == sorted(order[:k].tolist()), qi
        assert got["keyword"][qi].tolist() == kw[rows].tolist()
        np.testing.assert_allclose(got["hybrid"][qi], hyb[rows], rtol=0, atol=tol)


def _hybrid(eng, q, terms_of, k, a, b, g):
    import torch
    ptr = np.cumsum([0] + [len(t) for t in terms_of]).astype(np.int32)
    terms = np.asarray([x for t in terms_of for x in t], dtype=np.int32)
    out = eng.hybrid_linear_dev(torch.from_numpy(q).cuda(), torch.from_numpy(ptr).cuda(), torch.from_numpy(terms).cuda(), k, a, b, g)
    torch.cuda.synchronize()
    return {key: v.cpu().numpy() for key, v in out.items()}


@pytest.mark.parametrize("mag", [0.15, 50.0, 1e4])
def test_fused_bound_negative_weights_and_large_temporal(eng_factory, mag):
    """Weights of either sign and temporal planes of magnitude 0.15, 50 and 1e4 of both signs whose values are near-ties (they
    differ in bits far below float32, in which the emission forms gamma * temporal), with ordinary, repeated and
    out-of-vocabulary keyword queries (every keyword score 0, divisor 1.0)."""
    from test_hybrid_gpu import _sparse_postings
    rng = np.random.default_rng(int(mag * 100))
    N, D, k = 6000, 64, 25
    emb = rng.standard_normal((N, D)).astype(np.float32)
    post = _sparse_postings(rng, N, 12, 900)
    temporal = mag * rng.choice([-1.0, 1.0], N) * (1.0 + 1e-9 * rng.uniform(0, 1, N))
    temporal[rng.uniform(size=N) < 0.2] = 0.0
    terms_of = [[0, 1], [2, 3, 4, 4, 4], [-1, -1], [11, 0, 7], [5]]
    q = (emb[[5, 100, 2000, 4001, 5999]] + 0.5 * rng.standard_normal((5, D))).astype(np.float32)
    eng = eng_factory(D)
    eng.index_load(emb)
    eng.set_temporal(temporal)
    post.load(eng)
    for a, b, g in WEIGHTS:
        got = _hybrid(eng, q, terms_of, k, a, b, g)
        st = eng.dense_stats()
        assert st["proven_fast"] + st["proven_wide"] + st["exact_scan"] == len(terms_of), st
        _check_linear(got, _linear_oracle(post, emb, q, terms_of, temporal, a, b, g, k), k)
        assert got["temporal"].tolist() == [[temporal[r] for r in rows] for rows in got["rows"].tolist()]
        assert (got["keyword"][2] == 0.0).all()


def _negative_idf_postings(n_rows, filler_words=None):
    """40 documents' worth of 6 common terms (every document holds every term, term frequencies 1 to 24) repeated to n_rows rows:
    every idf is negative, rank-bm25's floor 0.25 * average_idf is negative too, and every raw score is <= 0. filler_words
    (one count per row) lengthens the documents with words no query asks for."""
    from optimized_rag_amd.bm25 import Bm25Postings
    n_terms = 6
    base_tf = 1 + (np.arange(40)[:, None] * 7 + np.arange(n_terms)[None, :] * 5) % 24           # [40, 6]
    tf = base_tf[np.arange(n_rows) % 40]                                                         # [n_rows, 6]
    indptr = (np.arange(n_terms + 1) * n_rows).astype(np.int64)
    doc = np.tile(np.arange(n_rows, dtype=np.int32), n_terms)
    doc_len = (tf.sum(axis=1) + (0 if filler_words is None else filler_words)).astype(np.int32)
    idf = Bm25Postings.idf_table(np.diff(indptr), n_rows)
    return Bm25Postings(indptr, doc, tf.T.reshape(-1).astype(np.int32), doc_len, idf, float(doc_len.sum()) / n_rows)


def test_fused_bound_negative_bm25_scores_of_any_magnitude(eng_factory):
    """Negative-idf corpus, queries of 1, 8 and 40 repeated tokens (and of 200 and 400, to put the magnitude beyond doubt): all
    raw scores are <= 0, so they are divided by 1.0 and the long queries score far below -8, the constant the fused bound
    used to allow for |keyword score|. On THIS corpus the parent commit passes all the same: the 150 copies of a document
    share one raw score, so the float32 rounding of raw32 * qscale is common to every row that competes (documents differ by
    far more than alpha * cosine). The case that fails without the per-query margin is the next test."""
    rng = np.random.default_rng(16)
    N, D, k = 6000, 64, 25
    emb = rng.standard_normal((N, D)).astype(np.float32)
    post = _negative_idf_postings(N)
    assert (post.idf < 0).all()
    terms_of = [[2], [0, 1, 2, 3, 4, 5, 0, 1], [3] * 40, [1] * 200, [0, 5] * 200]
    q = (emb[[5, 100, 2000, 4001, 5999]] + 0.5 * rng.standard_normal((5, D))).astype(np.float32)
    temporal = np.where(rng.uniform(size=N) < 0.4, 0.15 * 0.5 ** (rng.uniform(0, 90, N) / 30.0), 0.0)
    raws = [O.bm25_scores_csr(post.indptr, post.doc, post.tf, post.doc_len, post.idf, post.avgdl, t) for t in terms_of]
    assert all((r <= 0).all() for r in raws) and np.abs(raws[2]).max() > 8.0
    print("largest |raw| per query:", [float(np.abs(r).max()) for r in raws])
    eng = eng_factory(D)
    eng.index_load(emb)
    eng.set_temporal(temporal)
    post.load(eng)
    for a, b, g in WEIGHTS:
        got = _hybrid(eng, q, terms_of, k, a, b, g)
        st = eng.dense_stats()
        assert st["proven_fast"] + st["proven_wide"] + st["exact_scan"] == len(terms_of), st
        _check_linear(got, _linear_oracle(post, emb, q, terms_of, temporal, a, b, g, k), k)


def test_fused_bound_negative_bm25_scores_that_compete(eng_factory):
    """The case that shows the old constant wrong. The 150 copies of each of the 40 documents differ by one filler word out of
    a million, so their raw scores for a 400-token query lie ~1e-4 apart around -1250: close enough to compete with
    0.01 * cosine, and each with its own float32 rounding (one unit in the last place of 1250 is 1.2e-4). With
    (alpha, beta, gamma) = (0.01, 1, 0) a margin that allows |keyword score| <= 8 is 2 eps = 2.8e-5; the test first shows on
    the CPU, from a float32 restatement of the emitted score, that such a margin loses a row of the exact top-k for some of
    the 200 queries, then asks the engine for the oracle's result on all of them."""
    rng = np.random.default_rng(17)
    N, D, k, Q = 6000, 64, 25, 200
    a, b, g = 0.01, 1.0, 0.0
    emb = rng.standard_normal((N, D)).astype(np.float32)
    post = _negative_idf_postings(N, filler_words=1_000_000 + np.arange(N) // 40)
    terms = [0, 5] * 200
    q = rng.standard_normal((Q, D)).astype(np.float32)
    raw = O.bm25_scores_csr(post.indptr, post.doc, post.tf, post.doc_len, post.idf, post.avgdl, terms)
    assert (raw <= 0).all() and np.abs(raw).max() > 1000
    sem = O.cosine_matrix(q, emb)
    hyb = (a * sem + b * (raw / 1.0)[None, :]) + g * 0.0
    # the emitted score: float32(alpha) * S~ + float32(raw) * float32(beta / 1.0), one float32 rounding of the sum
    s32 = (np.float64(np.float32(a)) * sem + (raw.astype(np.float32) * np.float32(b)).astype(np.float64)[None, :]).astype(np.float32).astype(np.float64)
    old_two_eps = 2.0 * (a * (A.emit_bound(D) + 2e-5) + (a + 8.0 * b) * 2.0 ** -21 + 1e-7)
    lost = 0
    for qi in range(Q):
        top = O.stable_topk_desc(hyb[qi], k)
        lost += int((np.sort(s32[qi])[-k] - s32[qi][top] > old_two_eps).sum())
    print(f"max |float32 emitted score - hybrid| = {np.abs(s32 - hyb).max():.3e}, margin for |kw| <= 8: {old_two_eps:.3e}, rows it would lose: {lost}")
    assert lost >= 1
    eng = eng_factory(D)
    eng.index_load(emb)
    post.load(eng)
    got = _hybrid(eng, q, [terms] * Q, k, a, b, g)
    st = eng.dense_stats()
    assert st["proven_fast"] + st["proven_wide"] + st["exact_scan"] == Q and st["exact_scan"] == 0, st
    oracle = [(raw, raw / 1.0, hyb[qi], O.stable_topk_desc(hyb[qi], k + 1)) for qi in range(Q)]
    _check_linear(got, oracle, k)
