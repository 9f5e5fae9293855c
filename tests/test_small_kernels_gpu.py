"""GPU: the small float64 kernels around the search paths, at their documented limits and on inputs where every float64 sum is
exact (tests/small_inputs.py), so that the device must agree with oracle/rag_oracle.py bit for bit - no tolerance and no
"numerical tie" excuse:

  rag_chunk_chain_host                      groups == O.chunk_chain, thresholds sitting exactly on a similarity, dim up to 8192
  rag_mmr_select_host / rag_mmr_select_dev  picks and scores == O.mmr_class / O.mmr_helper, pool up to 256, top_k up to the pool
  rag_rerank_topk_dev                       == O.rerank_topk on its own, saturated sigmoids, empty slots anywhere
  rag_rrf_fuse_host / rag_rrf_fuse_dev      == O.rrf_fuse at the 1024-item limit, 64-bit keys, empty lists
  rag_linear_fuse_topk_host                 == the stable sort at top_k = 1024, n around the 2048 chunk, +-inf
  rag_pairwise_cosine_f64_host              == O.cosine on float64 inputs; differs from the float32 entry where it must

Each of these one-line mutants of the library, built aside and run once on the MI355X, failed the test named: `>=` -> `>` in the
chunk-chain join (test_chunk_chain_equals_the_oracle_on_exact_chains); `i < j` -> `i > j` in rerank_topk_kernel
(test_rerank_topk_on_its_own); `ra < rb` -> `ra > rb` in pair_before_f (test_linear_fusion_at_top_k_1024); `oi < best_i` ->
`oi > best_i` in the wave reduction and `red_i[w] < bi` -> `red_i[w] > bi` in the cross-wave step of the MMR argmax (both MMR
tests). `j < best_i` -> `j > best_i` in the per-thread loop of the MMR argmax changes nothing and cannot be caught: a pool is at
most 256 candidates for 256 threads, a thread never holds two, so that comparison never decides (csrc/mmr.hip says so now).

Plus one hypothesis property per kernel on Gaussian float32 inputs. Deliberately NOT covered: NaN logits and NaN fused scores (the
reference's own sort is unspecified on them)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

import small_inputs as SI
from oracle import rag_oracle as O

pytestmark = pytest.mark.gpu

RAG_ERR_ARG = -1
_ENGINES = {}


def _engine(dim=64):
    from optimized_rag_amd import RagEngine
    if dim not in _ENGINES:
        _ENGINES[dim] = RagEngine(dim=dim, device=0)
    return _ENGINES[dim]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


N_EX = int(os.environ.get("RAG_PROPERTY_EXAMPLES", "300"))
COMMON = dict(deadline=None, max_examples=max(20, N_EX // 6), derandomize="RAG_PROPERTY_EXAMPLES" not in os.environ, database=None,
              suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large])


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _tp(t):
    return C.c_void_p(t.data_ptr())


# =================================================================================================================
# chunk chain
# =================================================================================================================

def _chain_rc(eng, embs, lens, thr, max_chunk, min_chunk):
    embs = np.ascontiguousarray(embs, dtype=np.float32)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    out = np.full((embs.shape[0],), -7, dtype=np.int32)
    rc = eng.lib.rag_chunk_chain_host(eng.h, _p(embs), _p(lens), embs.shape[0], embs.shape[1], float(thr), int(max_chunk), int(min_chunk), _p(out))
    return rc, out


def _assert_order_free(embs, lens, thr, max_chunk, min_chunk):
    """the test's own precondition: the oracle's similarities do not depend on the summation order on this input"""
    dim = embs.shape[1]
    fwd = O.chunk_chain(embs, lens, thr, max_chunk, min_chunk, with_sims=True)
    rev = O.chunk_chain(embs, lens, thr, max_chunk, min_chunk, order=range(dim - 1, -1, -1), with_sims=True)
    per = O.chunk_chain(embs, lens, thr, max_chunk, min_chunk, order=np.random.default_rng(dim).permutation(dim), with_sims=True)
    assert fwd == rev == per, "test input bug: a sum is not exact on this chain"
    return fwd


@pytest.mark.parametrize("dim", SI.CHAIN_DIMS)
def test_chunk_chain_equals_the_oracle_on_exact_chains(dim):
    """rag_chunk_chain_host == O.chunk_chain with `==`, at dims on both sides of the 256-thread stride and at the 8192 limit
    (64 KiB of dynamic LDS beside the static 96 bytes), for: the threshold 0.5; a threshold EQUAL to a similarity of the chain
    (`>=` decides) and the next float above it (the grouping must change); thresholds no similarity meets (2.0: only the
    min_chunk rule joins) and every similarity meets (-2.0: only max_chunk closes chunks)."""
    eng = _engine()
    for seed in range(2 if dim > 2000 else 3):
        embs, lens = SI.exact_chain(seed, dim)
        g0, s0 = _assert_order_free(embs, lens, 0.5, SI.CHAIN_MAX, SI.CHAIN_MIN)
        assert g0[-1] >= 2
        t = SI.deciding_threshold(g0, s0, lens, SI.CHAIN_MAX, SI.CHAIN_MIN)
        assert t is not None and t in s0
        g_at = O.chunk_chain(embs, lens, t, SI.CHAIN_MAX, SI.CHAIN_MIN)
        g_above = O.chunk_chain(embs, lens, SI.next_up(t), SI.CHAIN_MAX, SI.CHAIN_MIN)
        assert g_at == g0 and g_above != g_at                       # precondition: `>=` against `>` decides on this chain
        g_all = O.chunk_chain(embs, lens, -2.0, SI.CHAIN_MAX, SI.CHAIN_MIN)
        assert g_all == [i // 9 for i in range(len(lens))]           # only max_chunk (9 sentences of 10 characters) closes chunks
        expect = {0.5: g0, t: g_at, SI.next_up(t): g_above, -2.0: g_all,
                  2.0: O.chunk_chain(embs, lens, 2.0, SI.CHAIN_MAX, SI.CHAIN_MIN)}
        for thr, exp in expect.items():
            got = eng.chunk_chain(embs, lens, thr, SI.CHAIN_MAX, SI.CHAIN_MIN).tolist()
            assert got == exp, (dim, seed, thr)
        # min_chunk absorbs every dissimilar sentence: nothing meets 2.0, nothing ever reaches min_chunk -> one chunk. (The
        # grouping does not depend on any similarity here, so the 39 halvings in a row do not matter.)
        assert O.chunk_chain(embs, lens, 2.0, SI.CHAIN_MAX, 10_000) == [0] * len(lens)
        assert eng.chunk_chain(embs, lens, 2.0, SI.CHAIN_MAX, 10_000).tolist() == [0] * len(lens)


@pytest.mark.parametrize("dim", [1, 3, 257, 1536])
def test_chunk_chain_zero_sentences_and_threshold_zero(dim):
    """An all-zero sentence has similarity 0.0 by the zero-norm rule, against a running chunk and as the running chunk itself; with
    threshold 0.0 it joins (0.0 >= 0.0), with the smallest positive float as threshold it does not."""
    eng = _engine()
    embs, lens = SI.exact_chain(11, dim)
    embs[3] = 0.0                    # meets a running chunk of three absorbed sentences: the similarity alone decides
    embs[20] = 0.0
    tiny = SI.next_up(0.0)
    g_zero, s_zero = _assert_order_free(embs, lens, 0.0, SI.CHAIN_MAX, SI.CHAIN_MIN)
    g_tiny, _ = _assert_order_free(embs, lens, tiny, SI.CHAIN_MAX, SI.CHAIN_MIN)
    assert s_zero[2] == 0.0 and g_zero[3] == g_zero[2] and g_tiny[3] != g_tiny[2]
    assert eng.chunk_chain(embs, lens, 0.0, SI.CHAIN_MAX, SI.CHAIN_MIN).tolist() == g_zero
    assert eng.chunk_chain(embs, lens, tiny, SI.CHAIN_MAX, SI.CHAIN_MIN).tolist() == g_tiny
    allz = np.zeros((7, dim), dtype=np.float32)
    lens7 = np.full(7, 30, dtype=np.int32)
    for thr in (0.0, tiny):
        assert eng.chunk_chain(allz, lens7, thr, 90, 25).tolist() == O.chunk_chain(allz, lens7, thr, 90, 25)


def test_chunk_chain_single_sentence_and_the_dimension_limit():
    """n = 1 is one chunk; dim 8192 is the documented limit (include/rag_hip.h) and works; 8193 and the other bad sizes are
    RAG_ERR_ARG and leave the output alone."""
    eng = _engine()
    for dim in (1, 64, 8192):
        rc, out = _chain_rc(eng, np.ones((1, dim)), [10], 0.7, 90, 25)
        assert rc == 0 and out.tolist() == [0]
    embs, lens = SI.exact_chain(0, 8192, n=12)
    rc, out = _chain_rc(eng, embs, lens, 0.5, SI.CHAIN_MAX, SI.CHAIN_MIN)
    assert rc == 0 and out.tolist() == O.chunk_chain(embs, lens, 0.5, SI.CHAIN_MAX, SI.CHAIN_MIN)
    rc, out = _chain_rc(eng, np.ones((3, 8193)), [10, 10, 10], 0.5, 90, 25)
    assert rc == RAG_ERR_ARG and out.tolist() == [-7] * 3
    out = np.zeros(1, dtype=np.int32)
    one = np.ones((1, 4), dtype=np.float32)
    ln = np.ones(1, dtype=np.int32)
    assert eng.lib.rag_chunk_chain_host(eng.h, _p(one), _p(ln), 0, 4, 0.5, 90, 25, _p(out)) == RAG_ERR_ARG
    assert eng.lib.rag_chunk_chain_host(eng.h, _p(one), _p(ln), 1, 0, 0.5, 90, 25, _p(out)) == RAG_ERR_ARG


def _gaussian_chain_case(eng, seed, n, dim, thr, max_chunk, min_chunk, tally):
    """One example of the Gaussian chunk-chain property; eng None = oracle side only (used to check the caps on the CPU)."""
    rng = np.random.default_rng(seed)
    embs = SI.clustered_sentences(rng, n, dim, n_centres=int(rng.integers(2, 5)), noise=float(rng.uniform(0.2, 0.7)))
    lens = rng.integers(5, 40, n).astype(np.int32)
    groups, sims = O.chunk_chain(embs, lens, thr, max_chunk, min_chunk, with_sims=True)
    tally["examples"] += 1
    if any(abs(s - thr) < 1e-9 for s in sims):                     # the device may legitimately round to the other side
        tally["skipped"] += 1
        return
    h = SI.chain_hinges(groups, lens, max_chunk, min_chunk)
    joins = any(h[i - 1] and groups[i] == groups[i - 1] for i in range(1, n))
    splits = any(groups[i] != groups[i - 1] for i in range(1, n))
    tally["join_and_split"] += joins and splits
    if eng is not None:
        assert eng.chunk_chain(embs, lens, thr, max_chunk, min_chunk).tolist() == groups


CHAIN_EXAMPLES = max(60, N_EX // 2)          # cheap (one workgroup, a few dozen sentences); enough for the two shares below to be stable
CHAIN_PROPERTY = dict(seed=st.integers(0, 2**31 - 1), n=st.integers(2, 48), dim=st.sampled_from(SI.CHAIN_DIMS),
                      thr=st.floats(0.0, 1.0), max_chunk=st.sampled_from([100, 250, 5000]), min_chunk=st.sampled_from([1, 30, 80]))


def test_chunk_chain_on_gaussian_sentences():
    """Property on Gaussian float32 sentences around a few cluster centres: groups == O.chunk_chain. An example whose threshold lies
    within 1e-9 of one of the oracle's similarities is not compared (a parallel sum may round it to the other side); at most 1 %
    of the examples may go that way, and at least a third must contain both a join decided by the similarity and a split."""
    eng = _engine()
    tally = dict(examples=0, skipped=0, join_and_split=0)

    @settings(**{**COMMON, "max_examples": CHAIN_EXAMPLES})
    @given(**CHAIN_PROPERTY)
    def run(seed, n, dim, thr, max_chunk, min_chunk):
        _gaussian_chain_case(eng, seed, n, dim, thr, max_chunk, min_chunk, tally)

    run()
    print("chunk chain property:", tally)
    assert tally["skipped"] <= 0.01 * tally["examples"], tally
    assert tally["join_and_split"] * 3 >= tally["examples"], tally


# =================================================================================================================
# MMR
# =================================================================================================================
MMR_N = [1, 2, 63, 64, 65, 255, 256]
MMR_LAM = [0.0, 0.5, 1.0]


def _mmr_oracle(q, embs, top_k, lam, variant, rel=None, sim=None):
    """(positions, scores) of the reference loop. The literal O(k^2 n) loops where they take well under a second, else the
    running-max form of the same loops (O.mmr_greedy, pinned to them bit for bit by tests/test_oracle_golden.py)."""
    n = len(embs)
    if n * top_k * top_k <= (80_000 if lam == 0.5 else 5_000):
        e64 = [np.asarray(e, dtype=np.float64) for e in embs]
        q64 = np.asarray(q, dtype=np.float64)
        if variant == 0:
            return O.mmr_class(q64, e64, top_k, lam)
        assert n > top_k
        return O.mmr_helper(q64, e64, top_k, lam, with_scores=True)
    if rel is None:
        rel = O.cosine_matrix(np.asarray(q)[None, :], embs)[0].tolist()
        sim = O.cosine_matrix(embs, embs).tolist()
    return O.mmr_greedy(rel, sim, top_k, lam, variant)


def _assert_integer_sums_exact(q, embs):
    """precondition of the `==` below: integer entries, so every dot product and squared norm is an exact integer < 2**53 in any
    summation order; checked by reversing the order"""
    a = np.asarray(embs, dtype=np.float64)
    assert (a == np.round(a)).all() and np.abs(a).max() <= 3 and 9 * a.shape[1] < 2**53
    qq = np.asarray(q, dtype=np.float64)
    assert (O.cosine_matrix(qq[None, ::-1], a[:, ::-1]) == O.cosine_matrix(qq[None, :], a)).all()
    assert (O.cosine_matrix(a[:, ::-1], a[:, ::-1]) == O.cosine_matrix(a, a)).all()


@pytest.mark.parametrize("dim", [1, 3, 63, 64, 65, 1536])
@pytest.mark.parametrize("n", MMR_N)
def test_mmr_host_entry_is_bit_identical_on_integer_vectors(n, dim):
    """rag_mmr_select_host: picks AND winning scores == the oracle, both variants, top_k in {1, n // 2, n}, lambda in {0, 0.5, 1}.
    Integer vectors in small dims are full of exact duplicates, zero vectors and exact score ties across all 256 threads and 4 waves:
    'first maximal candidate wins' is decided by the reduction's tie rule alone."""
    eng = _engine()
    rng = np.random.default_rng([n, dim])
    embs = SI.int_vectors(rng, n, dim)
    q = SI.int_vectors(rng, 1, dim)[0]
    _assert_integer_sums_exact(q, embs)
    rel = O.cosine_matrix(q[None, :], embs)[0].tolist()
    sim = O.cosine_matrix(embs, embs).tolist()
    for top_k in sorted({1, max(1, n // 2), n}):
        for lam in MMR_LAM:
            for variant in (0, 1):
                if variant == 1 and n <= top_k:
                    continue                                    # apply_mmr returns its input unchanged there (host-side rule)
                pos, sc = _mmr_oracle(q, embs, top_k, lam, variant, rel, sim)
                got, gsc = eng.mmr_select(q, embs, top_k, lam, variant)
                assert got.tolist() == pos, (n, dim, top_k, lam, variant)
                assert gsc.tolist() == sc, (n, dim, top_k, lam, variant)


@pytest.mark.parametrize("dim", [4, 64, 68, 1536])
def test_mmr_device_entry_is_bit_identical_on_integer_rows(dim):
    """rag_mmr_select_dev over rows of the resident index: several queries with different pools, -1 slots scattered through the
    pool, pools of 1 .. 256, top_k up to the pool (-1 / 0.0 padding once the live candidates run out), repeated rows."""
    import torch
    from optimized_rag_amd import RagEngine
    eng = RagEngine(dim=dim, device=0)
    try:
        rng = np.random.default_rng(dim)
        N, Q = 300, 3
        corpus = SI.int_vectors(rng, N, dim)
        queries = SI.int_vectors(rng, Q, dim)
        eng.index_load(corpus)
        q_d = torch.from_numpy(queries).cuda()
        for pool in MMR_N:
            rows = rng.integers(0, N, (Q, pool)).astype(np.int32)
            if pool >= 63:
                rows[0, rng.choice(pool, pool // 5, replace=False)] = -1          # scattered
                rows[1, :3] = -1                                                   # head
                rows[1, -2:] = -1                                                  # tail
            rows_d = torch.from_numpy(rows).cuda()
            per_query = []
            for qi in range(Q):
                live = [j for j in range(pool) if rows[qi, j] >= 0]
                embs = corpus[rows[qi, live]]
                _assert_integer_sums_exact(queries[qi], embs)
                per_query.append((live, embs, O.cosine_matrix(queries[qi][None, :], embs)[0].tolist(), O.cosine_matrix(embs, embs).tolist()))
            for top_k in sorted({1, max(1, pool // 2), pool}):
                for lam in MMR_LAM:
                    for variant in (0, 1):
                        sel = torch.full((Q, top_k), -9, dtype=torch.int32, device="cuda")
                        sc = torch.full((Q, top_k), -9.0, dtype=torch.float64, device="cuda")
                        eng.mmr_select_dev(q_d, rows_d, top_k, lam, variant, sel, sc)
                        torch.cuda.synchronize()
                        for qi, (live, embs, rel, sim) in enumerate(per_query):
                            if variant == 1 and len(live) <= top_k:
                                continue                            # the kernel has no shortcut, the reference has no loop there
                            pos, osc = _mmr_oracle(queries[qi], embs, top_k, lam, variant, rel, sim)
                            pad = top_k - len(pos)
                            assert sel[qi].tolist() == [live[p] for p in pos] + [-1] * pad, (dim, pool, top_k, lam, variant, qi)
                            assert sc[qi].tolist() == list(osc) + [0.0] * pad, (dim, pool, top_k, lam, variant, qi)
        # the argument checks: a pool of 257 and an unknown variant are refused by both entries
        sel = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
        sc = torch.zeros((1, 4), dtype=torch.float64, device="cuda")
        rows257 = torch.zeros((1, 257), dtype=torch.int32, device="cuda")
        with pytest.raises(Exception, match=r"\(-1\)"):
            eng.mmr_select_dev(q_d[:1], rows257, 4, 0.5, 0, sel, sc)
        with pytest.raises(Exception, match=r"\(-1\)"):
            eng.mmr_select_dev(q_d[:1], rows257[:, :256].contiguous(), 4, 0.5, 2, sel, sc)
        e257 = np.ones((257, dim), dtype=np.float32)
        hs, hc = np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.float64)
        qh = np.ascontiguousarray(queries[0])
        assert eng.lib.rag_mmr_select_host(eng.h, _p(qh), _p(e257), 257, dim, 4, 0.5, 0, _p(hs), _p(hc)) == RAG_ERR_ARG
        assert eng.lib.rag_mmr_select_host(eng.h, _p(qh), _p(e257), 256, dim, 4, 0.5, 2, _p(hs), _p(hc)) == RAG_ERR_ARG
        assert eng.lib.rag_mmr_select_host(eng.h, _p(qh), _p(e257), 256, dim, 4, 0.5, 1, _p(hs), _p(hc)) == 0
    finally:
        eng.close()


@settings(**COMMON)
@given(seed=st.integers(0, 2**31 - 1), n=st.sampled_from(MMR_N), dim=st.sampled_from([1, 3, 63, 64, 65, 1536]),
       kk=st.sampled_from(["one", "half", "all"]), lam=st.sampled_from([0.0, 0.3, 0.5, 0.7, 1.0]), variant=st.integers(0, 1), dup=st.integers(0, 3))
def test_mmr_on_gaussian_vectors(seed, n, dim, kk, lam, variant, dup):
    """Property on Gaussian float32 candidates at the boundary pool sizes and dims, with the tie rule of
    tests/test_property_gpu.py::test_mmr_greedy_loop_on_the_device: the picks may part ways only where the device's pick scores
    within 1e-12 of the reference's under the reference's arithmetic."""
    rng = np.random.default_rng(seed)
    top_k = {"one": 1, "half": max(1, n // 2), "all": n}[kk]
    if variant == 1 and n <= top_k:
        top_k = max(1, n // 2)
        if n <= top_k:
            return
    embs = rng.standard_normal((n, dim)).astype(np.float32)
    for _ in range(dup):
        a, b = rng.integers(0, n, 2)
        embs[a] = embs[b]
    q = rng.standard_normal(dim).astype(np.float32)
    rel = O.cosine_matrix(q[None, :], embs)[0].tolist()
    sim = O.cosine_matrix(embs, embs).tolist()
    pos, osc = O.mmr_greedy(rel, sim, top_k, lam, variant)
    got, gsc = _engine().mmr_select(q, embs, top_k, lam, variant)
    got = got.tolist()
    assert len(got) == len(pos)
    if got == pos:
        np.testing.assert_allclose(gsc, osc, rtol=0, atol=1e-12)
        return
    j = next(i for i in range(len(pos)) if got[i] != pos[i])
    chosen = pos[:j]

    def ref_score(i):
        ms = max(sim[i][s] for s in chosen) if chosen else None
        if variant == 0:
            return lam * rel[i] + (1 - lam) * ((1 - ms) if chosen else 1.0)
        return lam * rel[i] - (1 - lam) * (ms if chosen else 0.0)
    assert abs(ref_score(got[j]) - ref_score(pos[j])) < 1e-12, (got, pos, j)


# =================================================================================================================
# rerank top-k
# =================================================================================================================
# Largest |device sigmoid - O.sigmoid| measured on the MI355X, in ulp of the oracle's value: 1.0 over the fixed cases (pools of 255
# and 256; 0.0 at pools 1 and 2), 2.0 over the Gaussian property. One exp and one division, each within an ulp, and the rounding of
# 1 + exp(-x) between them. The bound is twice the largest figure measured, which is also the allowance this test started from.
RERANK_ULP = 4


def _rerank_case(rng, Q, pool):
    """logits: multiples of 0.25 in [-12, 12] (neighbouring sigmoids differ by > 1e-6: no near-ties), many exact duplicates, and a
    block >= 40 whose float64 sigmoid is exactly 1.0 (ties fall to candidate position). Nothing between 12 and 40."""
    lg = (rng.integers(-48, 49, (Q, pool)) * 0.25).astype(np.float32)
    sat = rng.random((Q, pool)) < 0.2
    lg[sat] = rng.choice(np.array([40.0, 40.25, 55.5, 88.0], dtype=np.float32), int(sat.sum()))
    cand = rng.permutation(10 * Q * pool)[:Q * pool].reshape(Q, pool).astype(np.int64) + 2**40
    return lg, cand


def _run_rerank(eng, lg, cand, k):
    import torch
    Q = cand.shape[0]
    ids = torch.full((Q, k), -5, dtype=torch.int64, device="cuda")
    sc = torch.full((Q, k), -5.0, dtype=torch.float64, device="cuda")
    out = torch.full((Q, k), -5.0, dtype=torch.float32, device="cuda")
    eng.rerank_topk_dev(torch.from_numpy(lg).cuda(), torch.from_numpy(cand).cuda(), ids, sc, out)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("pool", [1, 2, 255, 256])
def test_rerank_topk_on_its_own(pool):
    """rag_rerank_topk_dev == O.rerank_topk: ids and raw logits exactly, scores within RERANK_ULP; k in {1, pool}; 4 queries of
    which one has -1 candidates at the head, in the middle and at the tail and one is all -1."""
    eng = _engine()
    rng = np.random.default_rng(pool)
    worst = 0.0
    for rep in range(3):
        lg, cand = _rerank_case(rng, 4, pool)
        cand[3, :] = -1
        if pool >= 255:
            cand[1, :4] = -1
            cand[1, 100:131] = -1
            cand[1, -3:] = -1
            cand[2, rng.choice(pool, 60, replace=False)] = -1
            lg[0, 64:192] = 41.0                                    # a saturated block across the wave boundaries
        elif pool == 2:
            cand[1, rep % 2] = -1
        assert (O.sigmoid(40.0) == 1.0) and not ((lg > 12.0) & (lg < 40.0)).any()
        for k in sorted({1, pool}):
            ids, sc, out = _run_rerank(eng, lg, cand, k)
            for qi in range(4):
                eid, esc, elg = O.rerank_topk(lg[qi], cand[qi], k)
                assert ids[qi].tolist() == eid, (pool, k, qi)
                assert out[qi].tolist() == elg, (pool, k, qi)
                live = [i for i, x in enumerate(eid) if x >= 0]
                assert sc[qi, len(live):].tolist() == [0.0] * (k - len(live))
                if live:
                    u = SI.ulps(sc[qi, :len(live)], esc[:len(live)])
                    worst = max(worst, float(u.max()))
                    assert u.max() <= RERANK_ULP, (pool, k, qi, float(u.max()))
    print(f"rerank_topk pool {pool}: largest score error {worst} ulp")


def test_rerank_topk_argument_checks():
    import torch
    eng = _engine()
    for pool, k in [(4, 5), (257, 1), (257, 257)]:
        lg = torch.zeros((1, pool), dtype=torch.float32, device="cuda")
        cand = torch.zeros((1, pool), dtype=torch.int64, device="cuda")
        ids = torch.full((1, k), -5, dtype=torch.int64, device="cuda")
        sc = torch.zeros((1, k), dtype=torch.float64, device="cuda")
        out = torch.zeros((1, k), dtype=torch.float32, device="cuda")
        rc = eng.lib.rag_rerank_topk_dev(eng.h, _tp(lg), _tp(cand), 1, pool, k, _tp(ids), _tp(sc), _tp(out), None)
        torch.cuda.synchronize()
        assert rc == RAG_ERR_ARG and ids.tolist() == [[-5] * k]


def test_rerank_topk_on_gaussian_logits():
    """Property on Gaussian float32 logits (distinct with probability 1, all well inside |x| < 30): same ids in the same order,
    scores within RERANK_ULP."""
    worst = [0.0]

    @settings(**COMMON)
    @given(seed=st.integers(0, 2**31 - 1), q=st.integers(1, 5), pool=st.sampled_from([1, 2, 3, 63, 64, 65, 255, 256]),
           kk=st.sampled_from(["one", "half", "all"]), holes=st.floats(0.0, 0.5))
    def run(seed, q, pool, kk, holes):
        rng = np.random.default_rng(seed)
        lg = (3.0 * rng.standard_normal((q, pool))).astype(np.float32)
        cand = np.arange(q * pool, dtype=np.int64).reshape(q, pool)
        cand[rng.random((q, pool)) < holes] = -1
        k = {"one": 1, "half": max(1, pool // 2), "all": pool}[kk]
        s64 = np.sort(np.array([O.sigmoid(float(x)) for x in np.unique(lg)]))
        # the oracle's order must not hang on the last bits: distinct logits give sigmoids at least 1e-12 apart
        assert len(s64) < 2 or np.diff(s64).min() > 1e-12, "test input bug: near-tied sigmoids"
        ids, sc, out = _run_rerank(_engine(), lg, cand, k)
        for qi in range(q):
            eid, esc, elg = O.rerank_topk(lg[qi], cand[qi], k)
            assert ids[qi].tolist() == eid and out[qi].tolist() == elg
            u = SI.ulps(sc[qi], esc)[np.array(eid) >= 0]
            if len(u):
                worst[0] = max(worst[0], float(u.max()))
                assert u.max() <= RERANK_ULP

    run()
    print(f"rerank_topk property: largest score error {worst[0]} ulp")


# =================================================================================================================
# reciprocal rank fusion
# =================================================================================================================

def _rrf_both_entries(eng, lists, top_k, rrf_k=60):
    """lists [Q, L, len] int64 through rag_rrf_fuse_host and rag_rrf_fuse_dev -> two (keys, scores, ranks) triples"""
    import torch
    Q, L, ln = lists.shape
    host = eng.rrf_fuse(lists, rrf_k=rrf_k, top_k=top_k)
    keys = torch.full((Q, top_k), -5, dtype=torch.int64, device="cuda")
    sc = torch.full((Q, top_k), -5.0, dtype=torch.float64, device="cuda")
    rk = torch.full((Q, top_k, L), -5, dtype=torch.int32, device="cuda")
    # a zero-length list table still needs a valid pointer: one element that must never be read as a key
    src = torch.from_numpy(lists).cuda() if lists.size else torch.full((1,), 12345, dtype=torch.int64, device="cuda")
    rc = eng.lib.rag_rrf_fuse_dev(eng.h, _tp(src), Q, L, ln, rrf_k, top_k, _tp(keys), _tp(sc), _tp(rk), None)
    torch.cuda.synchronize()
    assert rc == 0
    return host, (keys.cpu().numpy(), sc.cpu().numpy(), rk.cpu().numpy())


def _assert_rrf(eng, lists, top_k, rrf_k=60):
    lists = np.ascontiguousarray(lists, dtype=np.int64)
    Q, L, ln = lists.shape
    for name, (keys, sc, rk) in zip(("host", "dev"), _rrf_both_entries(eng, lists, top_k, rrf_k)):
        for qi in range(Q):
            ek, es, er = O.rrf_fuse([[int(x) for x in l if x >= 0] for l in lists[qi]], k=rrf_k, top_k=top_k)
            pad = top_k - len(ek)
            assert keys[qi].tolist() == ek + [-1] * pad, (name, qi)
            assert sc[qi].tolist() == es + [0.0] * pad, (name, qi)           # same float64 additions in the same order: bit-exact
            assert rk[qi].tolist() == er + [[0] * L] * pad, (name, qi)


@pytest.mark.parametrize("n_lists,list_len", [(1, 1024), (4, 256), (8, 128), (1024, 1)])
def test_rrf_at_the_1024_item_limit(n_lists, list_len):
    """1024 items per query in every split the limit allows: all keys distinct (1024 owners in the 2048-slot table), all lists
    identical (every key n_lists times), ragged -1 tails, 64-bit keys next to small ones; top_k below, at and above the number of
    distinct keys. Three queries per call."""
    eng = _engine()
    rng = np.random.default_rng([n_lists, list_len])
    T = n_lists * list_len
    big = np.array([2**62 - 1, 2**62, 2**62 + 1, 2**63 - 2, 2**63 - 3, 0, 1, 2**32, 2**32 + 1], dtype=np.int64)
    distinct = []
    for _ in range(3):
        small = np.unique(rng.integers(2, 2**31, 2 * T))[:T - len(big)]
        distinct.append(rng.permutation(np.concatenate([big, small])).reshape(n_lists, list_len))
    distinct = np.stack(distinct)
    assert all(len(np.unique(d)) == T for d in distinct)
    for top_k in (1, 1000, 1024, 1030):
        _assert_rrf(eng, distinct, top_k)
    one = rng.permutation(5000)[:list_len].astype(np.int64)
    same = np.broadcast_to(one, (3, n_lists, list_len)).copy()
    same[1] = same[1, :, ::-1]
    _assert_rrf(eng, same, min(list_len + 3, 300))
    ragged = distinct.copy() % 700                                   # a universe of 700: keys recur across lists, rarely inside one
    for qi in range(3):
        for l in range(n_lists):
            keep = int(rng.integers(0, list_len + 1))
            ragged[qi, l, keep:] = -1
    ragged[2, 0, :] = -1                                             # an empty first list
    _assert_rrf(eng, ragged, 64)
    _assert_rrf(eng, ragged, 701)


def test_rrf_repeats_wide_keys_empty_lists_and_the_1025_rejection():
    import torch
    eng = _engine()
    # a key repeated inside one list adds once per occurrence and ranks by its first position
    lists = np.array([[[7, 3, 7, 9, 7, -1], [3, 3, 2**63 - 2, 7, -1, -1], [2**62, 5, 2**62, 5, 2**62, 5]]], dtype=np.int64)
    for top_k in (1, 3, 6, 10):
        _assert_rrf(eng, lists, top_k)
        _assert_rrf(eng, lists, top_k, rrf_k=1)
    # list_len = 0 right after a call that left real keys behind in the handle's staging buffer: nothing to fuse, all padding
    _assert_rrf(eng, lists, 4)
    _assert_rrf(eng, np.zeros((2, 3, 0), dtype=np.int64), 5)
    _assert_rrf(eng, np.full((2, 3, 4), -1, dtype=np.int64), 5)
    # 1025 items: refused by both entries, outputs untouched
    for n_lists, list_len in [(1, 1025), (5, 205), (1025, 1), (41, 25)]:
        bad = np.zeros((1, n_lists, list_len), dtype=np.int64)
        keys, sc = np.full((1, 3), -5, dtype=np.int64), np.zeros((1, 3))
        rk = np.zeros((1, 3, n_lists), dtype=np.int32)
        assert eng.lib.rag_rrf_fuse_host(eng.h, _p(bad), 1, n_lists, list_len, 60, 3, _p(keys), _p(sc), _p(rk)) == RAG_ERR_ARG
        assert keys.tolist() == [[-5] * 3]
        kd = torch.full((1, 3), -5, dtype=torch.int64, device="cuda")
        sd = torch.zeros((1, 3), dtype=torch.float64, device="cuda")
        rd = torch.zeros((1, 3, n_lists), dtype=torch.int32, device="cuda")
        assert eng.lib.rag_rrf_fuse_dev(eng.h, _tp(torch.from_numpy(bad).cuda()), 1, n_lists, list_len, 60, 3, _tp(kd), _tp(sd), _tp(rd), None) == RAG_ERR_ARG
        torch.cuda.synchronize()
        assert kd.tolist() == [[-5] * 3]


@settings(**COMMON)
@given(seed=st.integers(0, 2**31 - 1), shape=st.sampled_from([(1, 1024), (2, 512), (3, 341), (16, 64), (64, 16), (341, 3), (1024, 1), (5, 7)]),
       universe=st.sampled_from([1, 30, 1000, 2**62]), top_k=st.sampled_from([1, 10, 256, 1024]), rrf_k=st.sampled_from([0, 1, 60]), q=st.integers(1, 3))
def test_rrf_property_up_to_the_limit(seed, shape, universe, top_k, rrf_k, q):
    """Property: random keys WITH repeats inside and across lists, ragged tails, shapes up to 1024 items, host and device entry."""
    rng = np.random.default_rng(seed)
    n_lists, list_len = shape
    lists = rng.integers(0, universe, (q, n_lists, list_len), dtype=np.int64)
    for qi in range(q):
        for l in range(n_lists):
            lists[qi, l, int(rng.integers(0, list_len + 1)):] = -1
    _assert_rrf(_engine(), lists, top_k, rrf_k)


# =================================================================================================================
# linear fusion
# =================================================================================================================
LEVELS = np.array([0.0, 0.25, 0.5, 1.0])


def _assert_linear(eng, sem, kw, tmp, a, b, g, top_k):
    t = np.zeros_like(sem) if tmp is None else tmp
    with np.errstate(invalid="ignore"):
        hyb = (a * sem + b * kw) + g * t                           # CPython's association (retrieval.py:302)
    assert not np.isnan(hyb).any(), "test input bug: NaN fused scores are out of scope"
    exp = O.stable_topk_desc(hyb, top_k)
    idx, got = eng.linear_fuse_topk(sem, kw, tmp, a, b, g, top_k)
    assert got.tobytes() == hyb.tobytes()
    assert idx.tolist() == exp.tolist()
    return idx


@pytest.mark.parametrize("n", [1024, 2047, 2048, 2049, 50_000])
def test_linear_fusion_at_top_k_1024(n):
    """top_k = 1024, the limit (the merge kernel then has exactly as much room as carry), at n around the 2048-score chunk and
    at 25 chunks. Scores come from four levels and weights that are powers of two, so the fused scores are exact, take a dozen
    distinct values, and nearly everything ties: only 'lower index first' orders them. Then the same with +inf and -inf among
    the inputs (never on the same row with opposite signs: no NaN), and temporal NULL against zeros."""
    eng = _engine()
    rng = np.random.default_rng(n)
    sem = LEVELS[rng.integers(0, 4, n)]
    kw = LEVELS[rng.integers(0, 4, n)]
    tmp = LEVELS[rng.integers(0, 4, n)]
    top_k = min(1024, n)
    _assert_linear(eng, sem, kw, tmp, 0.5, 0.25, 0.25, top_k)
    i_none = _assert_linear(eng, sem, kw, None, 0.5, 0.25, 0.25, top_k)
    i_zero = _assert_linear(eng, sem, kw, np.zeros(n), 0.5, 0.25, 0.25, top_k)
    assert i_none.tolist() == i_zero.tolist()
    _assert_linear(eng, np.zeros(n), np.zeros(n), None, 0.5, 0.25, 0.25, top_k)          # one value: the answer is 0 .. top_k - 1
    _assert_linear(eng, sem[::-1].copy(), kw, tmp, 0.5, 0.25, 0.0, 1)
    sem2, kw2 = sem.copy(), kw.copy()
    hot = rng.choice(n, 40, replace=False)
    sem2[hot[:10]] = np.inf
    kw2[hot[10:20]] = np.inf
    sem2[hot[20:30]] = -np.inf
    kw2[hot[30:]] = -np.inf
    sem2[[0, n - 1]] = [-np.inf, np.inf]
    kw2[[0, n - 1]] = [0.5, 0.5]
    _assert_linear(eng, sem2, kw2, tmp, 0.5, 0.25, 0.25, top_k)
    # nearly all -inf: the top_k must reach into the -inf rows, in index order
    sem3 = np.full(n, -np.inf)
    sem3[rng.choice(n, 100, replace=False)] = 1.0
    _assert_linear(eng, sem3, kw, None, 0.5, 0.25, 0.25, top_k)


def test_linear_fusion_argument_checks():
    eng = _engine()
    n = 3000
    s = np.zeros(n)
    idx, hyb = np.full(2000, -5, dtype=np.int32), np.zeros(n)
    for nn, top_k in [(n, 1025), (n, 0), (1000, 1001), (1, 2)]:
        assert eng.lib.rag_linear_fuse_topk_host(eng.h, _p(s), _p(s), None, nn, 0.5, 0.25, 0.25, top_k, _p(idx), _p(hyb)) == RAG_ERR_ARG
        assert (idx == -5).all()
    assert eng.lib.rag_linear_fuse_topk_host(eng.h, _p(s), _p(s), None, n, 0.5, 0.25, 0.25, 1024, _p(idx), _p(hyb)) == 0
    assert idx[:1024].tolist() == list(range(1024))


@settings(**COMMON)
@given(seed=st.integers(0, 2**31 - 1), n=st.sampled_from([1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 9000]), kk=st.sampled_from([1, 7, 1024]),
       decimals=st.integers(0, 3), with_temporal=st.booleans())
def test_linear_fusion_on_gaussian_scores(seed, n, kk, decimals, with_temporal):
    """Property on Gaussian scores rounded to a few decimals (ties), top_k up to 1024, n on both sides of the chunk size."""
    rng = np.random.default_rng(seed)
    sem = np.round(rng.standard_normal(n), decimals)
    kw = np.round(rng.random(n), decimals)
    tmp = np.round(0.15 * rng.random(n), decimals + 1) if with_temporal else None
    _assert_linear(_engine(), sem, kw, tmp, 0.55, 0.35, 0.10, min(kk, n))


# =================================================================================================================
# float64 pairwise cosine
# =================================================================================================================
# Largest |device - O.cosine| measured on the MI355X over test_pairwise_cosine_f64_equals_the_oracle, in ulp of the oracle's value:
# 0 (dim 1), 3 (dim 63), 4 (dim 64), 4 (dim 65), 3 (dim 1536): three sums in two different orders, two square roots, a product and
# a division. The allowance this test started from is 4 ulp and the measured maximum reaches it, so it stays at 4.
COSINE_ULP = 4


@pytest.mark.parametrize("dim", [1, 63, 64, 65, 1536])
def test_pairwise_cosine_f64_equals_the_oracle(dim):
    """rag_pairwise_cosine_f64_host on float64 inputs that are NOT float32-representable == O.cosine within COSINE_ULP; zero rows
    give exactly 0.0; m = 0 or n = 0 is a successful no-op."""
    eng = _engine()
    rng = np.random.default_rng(dim)
    # rows around a common direction, so that the cosines sit where the callers' thresholds do (0.3 .. 1) and the dot product
    # does not cancel: an ulp of the RESULT is then a meaningful unit for the error of the three sums behind it
    base = rng.standard_normal(dim)
    a = (base + 0.5 * rng.standard_normal((9, dim))) * np.exp(rng.uniform(-3, 3, (9, 1)))
    b = (base + 0.5 * rng.standard_normal((7, dim))) * np.exp(rng.uniform(-3, 3, (7, 1)))
    a[4] = 0.0
    b[2] = 0.0
    b[5] = a[1]
    b[6] = -3.0 * a[6]
    got = eng.pairwise_cosine(a, b)
    exp = np.array([[O.cosine(x.tolist(), y.tolist()) for y in b] for x in a])
    assert (got[4] == 0.0).all() and (got[:, 2] == 0.0).all()
    nz = exp != 0.0
    u = SI.ulps(got[nz], exp[nz])
    print(f"pairwise_cosine_f64 dim {dim}: largest error {float(u.max())} ulp")
    assert u.max() <= COSINE_ULP, float(u.max())
    out = np.full(3, -5.0)
    assert eng.lib.rag_pairwise_cosine_f64_host(eng.h, _p(a), 0, _p(b), 7, dim, _p(out)) == 0
    assert eng.lib.rag_pairwise_cosine_f64_host(eng.h, _p(a), 9, _p(b), 0, dim, _p(out)) == 0
    assert eng.lib.rag_pairwise_cosine_f64_host(eng.h, _p(a), 1, _p(b), 1, 0, _p(out)) == RAG_ERR_ARG
    assert (out == -5.0).all()


def _threshold_pair(dim=64, thr=0.85):
    """(a, b) float64 whose cosine is just above thr while the cosine of the float32-rounded vectors is below it, both by margins
    (> 1e-10) far above any rounding of the float64 arithmetic itself."""
    for seed in range(200):
        rng = np.random.default_rng(seed)
        a = rng.standard_normal(dim)
        o = rng.standard_normal(dim)
        o -= a * (o @ a) / (a @ a)
        c = thr + 2e-9
        b = c * a / np.linalg.norm(a) + math.sqrt(1 - c * c) * o / np.linalg.norm(o)
        c64 = O.cosine(a.tolist(), b.tolist())
        c32 = O.cosine(a.astype(np.float32).tolist(), b.astype(np.float32).tolist())
        if c64 >= thr + 1e-10 and c32 < thr - 1e-10:
            return a, b, c64, c32
    raise AssertionError("test input bug: no pair found")


def test_pairwise_cosine_f64_stays_on_its_side_of_0_85():
    """Why the float64 entry exists (include/rag_hip.h): a pair at ConsistencyChecker's `>= 0.85` must not flip because its inputs
    were rounded to float32 first. On such a pair the float64 entry says >= 0.85 and the float32 entry, fed the same numbers,
    says < 0.85: the two paths differ where they must."""
    eng = _engine()
    a, b, c64, c32 = _threshold_pair()
    assert c64 >= 0.85 > c32
    got64 = eng.pairwise_cosine(a[None, :], b[None, :])[0, 0]
    got32 = eng.pairwise_cosine(a[None, :].astype(np.float32), b[None, :].astype(np.float32))[0, 0]
    assert got64 >= 0.85 and abs(got64 - c64) < 1e-13
    assert got32 < 0.85 and abs(got32 - c32) < 1e-13
    raw = np.zeros(1)
    assert eng.lib.rag_pairwise_cosine_f64_host(eng.h, _p(a), 1, _p(b), 1, a.shape[0], _p(raw)) == 0
    assert raw[0] == got64


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pairwise_cosine_aliased_equals_copied(dtype):
    """pairwise_cosine(a) (one upload, both operands the same device buffer) == pairwise_cosine(a, a.copy()) bit for bit."""
    eng = _engine()
    for dim in (1, 65, 1536):
        a = np.random.default_rng(dim).standard_normal((33, dim)).astype(dtype)
        a[5] = 0.0
        a[7] = a[3]
        alias = eng.pairwise_cosine(a)
        assert alias.tobytes() == eng.pairwise_cosine(a, a.copy()).tobytes()
        assert alias.tobytes() == eng.pairwise_cosine(a, a).tobytes()
        assert (alias == alias.T).all() and (alias[5] == 0.0).all()


@settings(**COMMON)
@given(seed=st.integers(0, 2**31 - 1), m=st.integers(1, 12), n=st.integers(1, 12), dim=st.sampled_from([1, 63, 64, 65, 1536]), zero_rows=st.booleans())
def test_pairwise_cosine_f64_on_gaussian_vectors(seed, m, n, dim, zero_rows):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((m, dim))
    b = rng.standard_normal((n, dim))
    if zero_rows:
        a[rng.integers(0, m)] = 0.0
    got = _engine().pairwise_cosine(a, b)
    exp = np.array([[O.cosine(x.tolist(), y.tolist()) for y in b] for x in a])
    # a cosine near 0 is a cancelling sum: its error is bounded in absolute terms (dim * 2**-53 * |x||y| / (|x||y|)), not in ulp of the result
    assert np.abs(got - exp).max() <= 1536 * 2.0**-53
    assert (got[exp == 0.0] == 0.0).all()
