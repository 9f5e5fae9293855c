"""CPU: the strategies of tests/m3_model.py run through the model alone, with the settings and the example counts of
tests/test_m3_property_gpu.py (the default run pins the generator's seed: these are the examples the GPU properties see).

(a) the model after any drawn operation list equals the model built fresh from the surviving documents - postings, token
    vectors, ids, tenants - and its results from before a compaction, rows sent through the row map, are the results after it;
(b) every class of inputs the GPU properties are there for occurs in at least 5 % of its property's examples (P3: of the examples
    of both start sizes together). The counts are printed (pytest -s).
This module is what keeps the GPU properties from passing on trivial draws."""
import numpy as np
from hypothesis import given

import m3_model as MM
import sparse_tools as S

FLOOR = 0.05


def _floor(name, seen, classes=None):
    n = len(seen)
    assert n > 0
    classes = classes or list(seen[0])
    counts = {c: sum(bool(s.get(c)) if isinstance(s, dict) else c in s for s in seen) for c in classes}
    print(f"\n{name}: {n} examples")
    for c, v in counts.items():
        print(f"  {v:4d}  {100.0 * v / n:5.1f} %  {c}")
    missing = [c for c, v in counts.items() if v < FLOOR * n or v == 0]
    assert not missing, (name, missing)


def test_p1_maxsim_cases_reach_every_class():
    seen = []

    @MM.prop("p1")
    @given(case=MM.maxsim_cases())
    def run(case):
        b = MM.build_maxsim(case)
        assert b["q"].shape == (b["q_off"][-1], case["dim"]) and b["d"].shape == (b["d_off"][-1], case["dim"])
        assert b["q"].dtype == b["d"].dtype == np.float32
        if case["family"] != "pow2":
            for a in (b["q"], b["d"]):
                assert a.shape[0] == 0 or np.abs(np.linalg.norm(a.astype(np.float64), axis=1) - 1.0).max() < 1e-6
        if case["family"] == "negated" and b["q"].shape[0] and b["d"].shape[0]:
            assert (b["q"].astype(np.float64) @ b["d"].astype(np.float64).T).max() < -0.5
        if case["family"] == "one sign" and b["q"].shape[0] and b["d"].shape[0]:
            assert (np.sign(b["q"][0]) == np.sign(b["d"][-1])).all()
        if case["family"] == "subnormal" and b["d"].shape[0]:
            small = np.abs(b["d"]) < 2.0 ** -14
            assert small.sum(axis=1).min() >= case["dim"] - 4 and (b["d"][small] != 0).any()
        seen.append(MM.maxsim_classes(case))

    run()
    _floor("P1 MaxSim", seen)


def test_p2_sparse_cases_reach_every_class():
    seen = []

    @MM.prop("p2")
    @given(case=MM.sparse_cases())
    def run(case):
        b = MM.build_sparse(case)
        ip, doc, w, n = b["indptr"], b["doc"], b["w"], b["n_docs"]
        assert ip[0] == 0 and ip[-1] == doc.shape[0] == w.shape[0] and np.isfinite(w).all() and (w > 0).all()
        for t in range(b["n_terms"]):
            d = doc[ip[t]:ip[t + 1]]
            assert (np.diff(d) > 0).all() and (d.shape[0] == 0 or (d[0] >= 0 and d[-1] < n))
        assert all(ip[t + 1] - ip[t] == n for t in b["all_terms"]) and all(ip[t + 1] == ip[t] for t in b["none_terms"])
        assert np.bincount(doc, minlength=n).max() <= 30 and np.isfinite(b["ref"]).all()
        # the blocks of the appended form put the corpus together again
        bounds = [0] + b["cuts"] + [n]
        parts = [MM.rows_span(ip, doc, w, lo, hi) for lo, hi in zip(bounds[:-1], bounds[1:])]
        assert sum(p[1].shape[0] for p in parts) == doc.shape[0]
        got = np.concatenate([S.all_scores(*p, hi - lo, b["queries"]) for p, lo, hi in zip(parts, bounds[:-1], bounds[1:])], axis=1)
        np.testing.assert_array_equal(S.bits(got), S.bits(b["ref"]))
        seen.append(MM.sparse_classes(case, b))

    run()
    _floor("P2 sparse", seen)


def _results(m, q):
    """what the model answers with its deleted rows hidden: sparse scores and top-k when the postings are current"""
    out = {}
    hidden = np.asarray(m.dead, dtype=bool)
    if m.consistent()["sparse"]:
        sc = S.all_scores(*m.csr(0, m.n_rows), m.n_rows, q["sparse"])
        sc[:, hidden] = 0.0
        out["scores"] = sc
        out["topk"] = S.topk_all(sc, 7, hidden)
    return out


def _sequence(case, seen):
    w, m, q = MM.build_sequence(case)
    assert m.consistent() == dict(dense=True, sparse=True, tokvec=True)
    for op in case["ops"]:
        before, (fm, fmap) = _results(m, q), m.fresh()
        store_before = [m.store_doc(d) for d in range(m.tv_docs)]
        n_before, tv_before = m.n_rows, m.tv_docs
        kind, payload = MM.apply(m, op)
        assert 0 < m.sp_base <= m.sp_cov <= m.n_rows and 0 <= m.tv_docs <= m.tv_docs_cap and m.tv_rows() <= m.tv_rows_cap
        if kind == "delete":
            assert m.n_rows == n_before and (payload is None or len(set(payload[1].tolist())) == len(payload[0]))
        if kind != "compact":
            continue
        np.testing.assert_array_equal(payload, fmap)
        # the model after the compaction IS the model built fresh from the surviving documents
        assert m.n_rows == fm.n_rows and all(a is b for a, b in zip(m.rows, fm.rows)) and not any(m.dead)
        fm.sp_cov, fm.n_terms = m.sp_cov, m.n_terms
        for x, y in zip(m.csr(0, m.sp_cov), fm.csr(0, m.sp_cov)):
            np.testing.assert_array_equal(x, y)
        for x, y in zip(m.columns(), fm.columns()):
            np.testing.assert_array_equal(x, y)
        keep = [d for i, d in enumerate(store_before) if i >= n_before or fmap[i] >= 0]      # the store: survivors, then the documents ahead
        assert m.tv_docs == len(keep) and all(m.store_doc(i) is d for i, d in enumerate(keep))
        assert (tv_before == n_before) <= (m.tv_docs == m.n_rows), "a current store stays current"
        after = _results(m, q)
        if before and after:                     # results from before the call, rows sent through the row map
            live = fmap >= 0
            np.testing.assert_array_equal(S.bits(before["scores"][:, live]), S.bits(after["scores"]))
            rows, sc = before["topk"]
            np.testing.assert_array_equal(np.where(rows >= 0, fmap[np.maximum(rows, 0)], -1), after["topk"][0])
            np.testing.assert_array_equal(S.bits(sc), S.bits(after["topk"][1]))
    # ... and at the end: the fresh model of the survivors has their postings, vectors, ids and tenants
    fm, fmap = m.fresh()
    live = m.live_rows()
    assert fm.n_rows == live.shape[0] and [fm.rows[i].id for i in range(fm.n_rows)] == [m.rows[r].id for r in live]
    if m.consistent()["sparse"]:
        sc = S.all_scores(*m.csr(0, m.n_rows), m.n_rows, q["sparse"])
        np.testing.assert_array_equal(S.bits(sc[:, live]), S.bits(fm.sparse_scores(q["sparse"])))
    seen.append(set(m.seen))


def test_p3_sequence_cases_reach_every_class():
    seen = []

    @MM.prop("p3_small")
    @given(case=MM.sequence_cases(MM.SMALL_STARTS))
    def small(case):
        _sequence(case, seen)

    @MM.prop("p3_large")
    @given(case=MM.sequence_cases(MM.LARGE_STARTS))
    def large(case):
        _sequence(case, seen)

    small()
    n_small = len(seen)
    large()
    assert n_small > 0 and len(seen) > n_small
    _floor("P3 sequences", seen, MM.SEQUENCE_CLASSES)


def test_a_pinned_seed_gives_two_functions_the_same_examples():
    """what lets this module speak for the GPU module: the examples depend on the strategy, the settings and the seed alone"""
    if MM.EXPLORE:
        return
    a, b = [], []

    @MM.prop("p3_small")
    @given(case=MM.sequence_cases(MM.SMALL_STARTS))
    def one(case):
        a.append(case)

    @MM.prop("p3_small")
    @given(case=MM.sequence_cases(MM.SMALL_STARTS))
    def two(case):
        b.append(repr(case))

    one()
    two()
    assert [repr(c) for c in a] == b and len(b) == MM.COUNTS["p3_small"]
