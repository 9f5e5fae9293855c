"""GPU: property tests (hypothesis) of the bge-m3 paths - MaxSim over caller-held and resident token vectors, the learned-sparse
index, and drawn write sequences over the whole resident stack - on the worlds of tests/m3_model.py. The default run is
derandomized with a pinned generator seed, so tests/test_m3_property_cases_cpu.py counts the input classes over exactly these
examples; RAG_PROPERTY_EXAMPLES explores. Engines are reused across examples where a load replaces everything they hold; every
output buffer is poisoned before the call that fills it. No bar here is new: they are the bars of tests/test_tokvec_gpu.py,
tests/test_sparse_*_gpu.py and tests/test_m3_fused_gpu.py.

P1 adds one relation: rag_maxsim_dev over the FETCHED (fp16-exact) rows gives the bits of the store's pair score for the same
query. Both kernels split the float32 query alike; a fetched row's `lo` half is exactly zero, so m3_maxsim_kernel's extra al * bh
MFMA adds +0.0 to every accumulator and what remains per accumulator - (ah * bl, ah * bh) per K-step - is tokvec_maxsim_kernel's
sequence; the maxima, their float64 sum in query order and the division are the same code. It is asserted bit for bit.

P3 follows the header where the issue text and the header part: rag_tokvec_rerank_* takes explicit rows and answers while the
store is behind or ahead of the index (only a plain compaction stales it); the entries that need the store to hold exactly the
index's rows are rag_m3_score_rows_dev / rag_retrieve_m3_dev with a colbert weight. rag_tokvec_fetch_host is compared for every
document of a store of up to 400, and above that for a drawn sample and the documents around every row a compaction removed.

Default example counts (m3_model.COUNTS at N_EX = 300) and wall times measured on an MI355X are in each test's docstring."""
import numpy as np
import pytest
from hypothesis import given

import m3_fused_tools as F
import m3_model as MM
import m3_tools as M
import sparse_tools as S
import tokvec_tools as V

pytestmark = pytest.mark.gpu

ERR_STATE = r"\(-3\)"
_ENGINES = {}


def _engine(key, dim=32):
    from optimized_rag_amd import RagEngine
    if key not in _ENGINES:
        _ENGINES[key] = RagEngine(dim=dim, device=0)
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def _t(a, pad=False):
    """a CUDA tensor of a host array; pad: one unused element behind it, so that an empty array still has an address"""
    import torch
    a = np.ascontiguousarray(a)
    if pad:
        a = np.concatenate([a.reshape(-1), np.zeros(1, a.dtype)])
    return torch.from_numpy(a).cuda()


def _np_out(*ts):
    import torch
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b, what):
    """two result bundles {name: tuple of arrays}, bit for bit"""
    assert a.keys() == b.keys(), what
    for name in a:
        for x, y in zip(a[name], b[name]):
            x, y = np.asarray(x), np.asarray(y)
            assert x.shape == y.shape and x.dtype == y.dtype, f"{what}: {name}"
            view = {np.dtype(np.float64): np.int64, np.dtype(np.float32): np.int32}.get(x.dtype)
            np.testing.assert_array_equal(x.view(view) if view else x, y.view(view) if view else y, err_msg=f"{what}: {name}")


# ---- P1 -----------------------------------------------------------------------------------------------------------------------------
def _maxsim_dev(e, q, qo, d, do, pq, pd):
    import torch
    dim = q.shape[1]
    out = torch.full((pq.shape[0],), float("nan"), dtype=torch.float32, device="cuda")
    qd = _t(q) if q.shape[0] else torch.zeros((1, dim), device="cuda")
    dd = _t(d) if d.shape[0] else torch.zeros((1, dim), device="cuda")
    e.maxsim_dev(qd, _t(qo), dd, _t(do), _t(pq), _t(pd), out)
    return _np_out(out)[0]


def _rerank_dev(e, q, qo, cand, k):
    import torch
    Q, pool = cand.shape
    ids = torch.full((Q, k), -7, dtype=torch.int64, device="cuda")
    rows = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((Q, k), float("nan"), dtype=torch.float64, device="cuda")
    ps = torch.full((Q, pool), float("nan"), dtype=torch.float32, device="cuda")
    qd = _t(q) if q.shape[0] else torch.zeros((1, q.shape[1]), device="cuda")
    e.tokvec_rerank_dev(qd, _t(qo), _t(cand.astype(np.int32)), k, ids, rows, sc, ps)
    return _np_out(ids, rows, sc, ps)


@MM.prop("p1")
@given(case=MM.maxsim_cases())
def test_p1_maxsim_over_given_and_resident_vectors(case):
    """60 examples, 4.0 s (11.7 s as the first GPU test of a process: device and library start-up). rag_maxsim_dev within 1e-4 of m3_tools.maxsim; rag_tokvec_rerank_dev's pair scores within 1e-4 of float64
    over the fetched rows and within 1e-3 over the originals; both bit-exact on the power-of-two family; the host forms give the
    device forms' bits; a pair's bits do not depend on its slot, its pool or its neighbours; the top-k is the stable top-k of the
    device's own scores; and rag_maxsim_dev over the fetched rows gives the store's bits (module docstring)."""
    b = MM.build_maxsim(case)
    q, qo, d, do, dim, rng = b["q"], b["q_off"], b["d"], b["d_off"], case["dim"], b["rng"]
    Q, D = len(qo) - 1, len(do) - 1
    e = _engine("p1")                                                    # no dense index: ids are row numbers
    e.tokvec_load(d, do)
    assert e.tokvec_info()["n_docs"] == D and e.tokvec_info()["rows"] == d.shape[0] and e.tokvec_info()["dim"] == dim
    stored = M.pack([e.tokvec_fetch(i) for i in range(D)], dim)[0]
    np.testing.assert_array_equal(_f32(stored), _f32(V.fp16_round(d)))
    # every pair, and three that lie outside their side
    pq = np.concatenate([np.repeat(np.arange(Q), D), [-1, 0, Q]]).astype(np.int32)
    pd = np.concatenate([np.tile(np.arange(D), Q), [0, D, 0]]).astype(np.int32)
    inside = (pq >= 0) & (pq < Q) & (pd >= 0) & (pd < D)

    def ref(dv):
        return np.array([M.maxsim(q[qo[a]:qo[a + 1]], dv[do[c]:do[c + 1]]) if ok else 0.0 for a, c, ok in zip(pq, pd, inside)])
    given_ = _maxsim_dev(e, q, qo, d, do, pq, pd)
    fetched = _maxsim_dev(e, q, qo, stored, do, pq, pd)
    ref_orig, ref_stored = ref(d), ref(stored)
    err = float(np.abs(given_ - ref_orig).max())
    assert err < 1e-4, f"rag_maxsim_dev: {err:.3e}"
    assert float(np.abs(fetched - ref_stored).max()) < 1e-4
    np.testing.assert_array_equal(_f32(e.maxsim(q, qo, d, do, pq, pd)), _f32(given_), err_msg="rag_maxsim_host")
    # the store: every document in every query's pool, an empty slot and a row past the store
    cand = np.concatenate([np.tile(np.arange(D), (Q, 1)), np.full((Q, 1), -1), np.full((Q, 1), D)], axis=1).astype(np.int32)
    pool = D + 2
    k = min(case["k"], pool)
    ids, rows, sc, ps = _rerank_dev(e, q, qo, cand, k)
    empty = V.slot_empty(qo, do, cand)
    assert ps.dtype == np.float32 and (ps[empty] == 0).all() and empty[:, -2:].all()
    exp_a, exp_b = V.pair_scores(q, qo, stored, do, cand), V.pair_scores(q, qo, d, do, cand)
    err_a, err_b = float(np.abs(ps - exp_a).max()), float(np.abs(ps - exp_b).max())
    assert err_a < 1e-4, f"store, over the fetched rows: {err_a:.3e}"
    assert err_b < 1e-3, f"store, over the original rows: {err_b:.3e}"
    if case["family"] == "negated":
        assert (ps[~empty] < -0.5 + 1e-3).all() and (given_[inside & (ref_orig != 0)] < 0).all()
    if case["family"] == "pow2":                                         # every product and sum is exact: the float32 rounding of the exact value
        np.testing.assert_array_equal(_f32(ps), _f32(exp_b.astype(np.float32)))
        np.testing.assert_array_equal(_f32(given_), _f32(ref_orig.astype(np.float32)))
    e_ids, e_rows, e_sc = V.stable_topk(ps, cand, empty, k)
    np.testing.assert_array_equal(rows, e_rows)
    np.testing.assert_array_equal(ids, e_rows.astype(np.int64))
    np.testing.assert_array_equal(V.bits(sc), V.bits(e_sc))
    for got, dev in zip(e.tokvec_rerank(q, qo, cand, k), (ids, rows, sc, ps)):
        np.testing.assert_array_equal(got.view(np.uint8), dev.view(np.uint8), err_msg="rag_tokvec_rerank_host")
    # the new relation: the caller-held kernel over the fetched rows has the store kernel's bits
    np.testing.assert_array_equal(_f32(fetched[:Q * D].reshape(Q, D)), _f32(ps[:, :D]), err_msg="rag_maxsim_dev over the fetched rows")
    # a pair's bits are a function of its own rows: another pool, another slot, other neighbours; then alone
    perm = rng.permutation(D)
    cand2 = np.concatenate([np.full((Q, 1), D + 3), np.tile(perm, (Q, 1)), np.full((Q, 2), -1), np.tile(perm[:1], (Q, 1))], axis=1).astype(np.int32)
    ps2 = _rerank_dev(e, q, qo, cand2, 1)[3]
    np.testing.assert_array_equal(_f32(ps2[:, 1:D + 1]), _f32(ps[:, perm]))
    np.testing.assert_array_equal(_f32(ps2[:, -1]), _f32(ps[:, perm[0]]))
    a, c = int(rng.integers(0, Q)), int(rng.integers(0, D))
    alone = _rerank_dev(e, q[qo[a]:qo[a + 1]], np.array([0, qo[a + 1] - qo[a]], dtype=np.int64), np.array([[c]], dtype=np.int32), 1)[3]
    assert _f32(alone)[0, 0] == _f32(ps)[a, c]


# ---- P2 -----------------------------------------------------------------------------------------------------------------------------
def _sparse_bundle(e, b, k, slots, tenants, q_emb, pool, kk):
    """everything the contract names of one loaded corpus, as host arrays; tenants: None without an index"""
    import torch
    ptr, terms, wts = b["packed"]
    dptr, dterms, dwts = _t(ptr), _t(terms, pad=True), _t(wts, pad=True)
    Q = ptr.shape[0] - 1
    out = {"scores": (e.sparse_scores(ptr, terms, wts),), "rows host": (e.sparse_score_rows(ptr, terms, wts, slots),)}
    pts = torch.full(slots.shape, float("nan"), dtype=torch.float64, device="cuda")
    e.sparse_score_rows_dev(dptr, dterms, dwts, _t(slots), pts)
    out["rows dev"] = _np_out(pts)
    for t in ([-1] if tenants is None else [-1, 1]):
        out[f"topk host {t}"] = e.sparse_topk(ptr, terms, wts, k, tenant=t)
        ids = torch.full((Q, k), -7, dtype=torch.int64, device="cuda")
        rows = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
        sc = torch.full((Q, k), float("nan"), dtype=torch.float64, device="cuda")
        e.sparse_topk_dev(dptr, dterms, dwts, k, ids, rows, sc, tenant=t)
        out[f"topk dev {t}"] = _np_out(ids, rows, sc)
    if tenants is not None:
        for t in getattr(e, "_hybs", ()):
            t.fill_(-7)
        keys, rrf, ranks = e.hybrid_sparse_rrf_dev(_t(q_emb), dptr, dterms, dwts, pool, kk, tenant=1)
        out["hybrid"] = _np_out(keys, rrf, ranks)
    return out


def _three_calls(e, b, q_emb, pool, kk, tenant):
    """rag_dense_topk_dev + rag_sparse_topk_dev + rag_rrf_fuse_dev"""
    import torch
    ptr, terms, wts = b["packed"]
    Q = ptr.shape[0] - 1
    lists = torch.full((Q, 2, pool), -7, dtype=torch.int64, device="cuda")
    d_ids, s_ids = (torch.full((Q, pool), -7, dtype=torch.int64, device="cuda") for _ in range(2))
    sc = torch.empty((Q, pool), dtype=torch.float64, device="cuda")
    e.dense_topk_dev(_t(q_emb), pool, d_ids, None, sc, tenant=tenant)
    e.sparse_topk_dev(_t(ptr), _t(terms, pad=True), _t(wts, pad=True), pool, s_ids, None, sc, tenant=tenant)
    lists[:, 0], lists[:, 1] = d_ids, s_ids
    keys = torch.full((Q, kk), -7, dtype=torch.int64, device="cuda")
    rrf = torch.full((Q, kk), float("nan"), dtype=torch.float64, device="cuda")
    ranks = torch.full((Q, kk, 2), -7, dtype=torch.int32, device="cuda")
    e.rrf_fuse_dev(lists, keys, rrf, ranks)
    return _np_out(keys, rrf, ranks)


@MM.prop("p2")
@given(case=MM.sparse_cases())
def test_p2_sparse_index_on_drawn_corpora(case):
    """100 examples, 1.1 s. Bit for bit: rag_sparse_scores_host == the numpy loop; rag_sparse_topk_* (host and device, with and without
    a tenant when an index is attached) == sparse_tools.topk; rag_sparse_score_rows_* at drawn slots (-1 and n_docs among them) ==
    the all-document scores; rag_hybrid_sparse_rrf_dev == the three-call composition; and the corpus loaded as a base + one or two
    appended blocks at the drawn cuts, the same after rag_sparse_fold and with the automatic fold, == the one-shot load."""
    b = MM.build_sparse(case)
    rng, n, k, ref = b["rng"], b["n_docs"], case["k"], b["ref"]
    Q = len(b["queries"])
    ids = tenants = q_emb = None
    engines = [_engine("p2 one shot"), _engine("p2 appended")]
    if case["with_index"]:
        emb = rng.standard_normal((n, 32)).astype(np.float32)
        ids, tenants = (500 + 3 * rng.permutation(n)).astype(np.int64), rng.integers(0, 3, n).astype(np.int32)
        q_emb = (emb[rng.integers(0, n, Q)] + 0.3 * rng.standard_normal((Q, 32))).astype(np.float32)
        for e in engines:
            e.index_load(emb, ids=ids)
            e.set_tenants(tenants)
    else:
        engines = [_engine("p2 one shot, no index"), _engine("p2 appended, no index")]
    one, app = engines
    slots = rng.integers(0, n, (Q, 9)).astype(np.int32)
    slots[:, 0], slots[:, 1], slots[:, 2], slots[:, 3] = -1, n, 0, n - 1
    for q in range(Q):                                                   # the query's own best rows: slots that score
        top = S.topk(ref[q], 3)[0]
        slots[q, 4:4 + int((top >= 0).sum())] = top[top >= 0]
    pool, kk = int(rng.integers(1, 257)), 0
    kk = int(rng.integers(1, pool + 1))
    for e in engines:
        e.set_option("bm25_plan_slots", case["plan_slots"])
        e.set_option("sparse_tail_fold", -1)
    try:
        one.sparse_load(b["indptr"], b["doc"], b["w"], n)
        got = _sparse_bundle(one, b, k, slots, tenants, q_emb, pool, kk)
        # against the references
        np.testing.assert_array_equal(S.bits(got["scores"][0]), S.bits(ref), err_msg="rag_sparse_scores_host")
        ok = (slots >= 0) & (slots < n)
        exp = np.where(ok, np.take_along_axis(ref, np.clip(slots, 0, n - 1).astype(np.int64), axis=1), 0.0)
        for name in ("rows host", "rows dev"):
            np.testing.assert_array_equal(S.bits(got[name][0]), S.bits(exp), err_msg=name)
        for t in ([-1] if tenants is None else [-1, 1]):
            e_rows, e_sc = S.topk_all(ref, k, None if t < 0 else tenants != t)
            e_ids = e_rows.astype(np.int64) if ids is None else np.where(e_rows >= 0, ids[np.maximum(e_rows, 0)], -1)
            for name in (f"topk host {t}", f"topk dev {t}"):
                np.testing.assert_array_equal(got[name][1], e_rows, err_msg=name)
                np.testing.assert_array_equal(got[name][0], e_ids, err_msg=name)
                np.testing.assert_array_equal(S.bits(got[name][2]), S.bits(e_sc), err_msg=name)
        if tenants is not None:
            for x, y in zip(got["hybrid"], _three_calls(one, b, q_emb, pool, kk, 1)):
                np.testing.assert_array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y,
                                              err_msg="rag_hybrid_sparse_rrf_dev against the three calls")
        if not b["cuts"]:
            return
        # the same corpus as base + appended blocks; folded by hand; folded by the append itself
        bounds = [0] + b["cuts"] + [n]
        blocks = [MM.rows_span(b["indptr"], b["doc"], b["w"], lo, hi) + (hi - lo,) for lo, hi in zip(bounds[:-1], bounds[1:])]

        def load_blocks():
            app.sparse_load(*blocks[0])
            for blk in blocks[1:]:
                app.sparse_append(*blk)
        load_blocks()
        st = app.sparse_segment_stats()
        assert (st["base_docs"], st["tail_docs"], st["folds"]) == (bounds[1], n - bounds[1], 0)
        _same(_sparse_bundle(app, b, k, slots, tenants, q_emb, pool, kk), got, "base + appended blocks")
        app.sparse_fold()
        st = app.sparse_segment_stats()
        assert (st["base_docs"], st["tail_docs"], st["folds"]) == (n, 0, 1)
        _same(_sparse_bundle(app, b, k, slots, tenants, q_emb, pool, kk), got, "after rag_sparse_fold")
        app.set_option("sparse_tail_fold", 1)                            # an append folds once the tail holds more than one document
        load_blocks()
        st = app.sparse_segment_stats()
        assert st["base_docs"] + st["tail_docs"] == n and st["tail_docs"] <= 1
        _same(_sparse_bundle(app, b, k, slots, tenants, q_emb, pool, kk), got, "with the automatic fold")
    finally:
        for e in engines:
            e.set_option("bm25_plan_slots", 0)
            e.set_option("sparse_tail_fold", 0)


# ---- P3 -----------------------------------------------------------------------------------------------------------------------------
POOL, K = 8, 5


def _raises_state(call):
    from optimized_rag_amd import RagError
    with pytest.raises(RagError, match=ERR_STATE):
        call()


def _m3_rows(e, q, dev, slots, weights):
    """rag_m3_score_rows_dev over explicit rows -> (ids, rows, scores, components)"""
    import torch
    Q = slots.shape[0]
    k = slots.shape[1]
    ids = torch.full((Q, k), -7, dtype=torch.int64, device="cuda")
    rows = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((Q, k), float("nan"), dtype=torch.float64, device="cuda")
    comp = torch.full((Q, k, 3), float("nan"), dtype=torch.float64, device="cuda")
    kw = {}
    if weights[1] > 0:
        kw.update(term_ptr=dev["ptr"], terms=dev["terms"], weights=dev["w"])
    if weights[2] > 0:
        kw.update(q_vecs=dev["qv"], q_off=dev["qo"])
    e.m3_score_rows_dev(_t(slots), k, ids, sc, q_emb=dev["q_emb"], w=weights, rows_out=rows, components_out=comp, **kw)
    return _np_out(ids, rows, sc, comp)


def _retrieve(e, dev, mode, weights, tenant=-1):
    """rag_retrieve_m3_dev -> (ids, scores, components, candidate ids)"""
    kw = {}
    if mode != 0 or weights[1] > 0:
        kw.update(term_ptr=dev["ptr"], terms=dev["terms"], weights=dev["w"])
    if weights[2] > 0:
        kw.update(q_vecs=dev["qv"], q_off=dev["qo"])
    for t in getattr(e, "_m3", ()):
        t.fill_(-7)
    return _np_out(*e.retrieve_m3_dev(dev["q_emb"], POOL, K, mode=mode, w=weights, tenant=tenant, **kw))


def _dev_queries(q):
    ptr, terms, wts = q["packed"]
    return dict(ptr=_t(ptr), terms=_t(terms, pad=True), w=_t(wts, pad=True), q_emb=_t(q["q_emb"]), qv=_t(q["qv"]), qo=_t(q["qo"]))


def _stack_results(e, q, dev, slots, tenant):
    """everything the contract names of a handle whose three legs are current"""
    ptr, terms, wts = q["packed"]
    out = {"sparse scores": (e.sparse_scores(ptr, terms, wts),), "sparse rows": (e.sparse_score_rows(ptr, terms, wts, slots),),
           "rerank": e.tokvec_rerank(q["qv"], q["qo"], slots, min(K, slots.shape[1]))}
    for t in (-1, tenant):
        out[f"sparse topk {t}"] = e.sparse_topk(ptr, terms, wts, K, tenant=t)
    for w in F.WEIGHT_SETS:
        out[f"m3 rows {w}"] = _m3_rows(e, q, dev, slots, w)
    for mode in (0, 1, 2):
        out[f"retrieve {mode}"] = _retrieve(e, dev, mode, F.WEIGHT_SETS[0])
    out[f"retrieve 2 tenant {tenant}"] = _retrieve(e, dev, 2, F.WEIGHT_SETS[0], tenant)
    return out


def _mapped(res, row_map, n_after):
    """results of a handle with hidden rows, its row numbers sent through `row_map` (scores and ids do not move)"""
    send = lambda rows: np.where(rows >= 0, row_map[np.clip(rows, 0, len(row_map) - 1)], -1).astype(np.int32)
    out = {}
    for name, v in res.items():
        if name == "sparse scores":
            out[name] = (np.ascontiguousarray(v[0][:, row_map >= 0]),)
        elif name.startswith("sparse topk") or name == "rerank" or name.startswith("m3 rows"):
            assert (row_map[v[1][v[1] >= 0]] >= 0).all(), "a hidden row was returned"
            out[name] = (v[0], send(v[1])) + tuple(v[2:])
        else:
            out[name] = v
    return out


def _load_fresh(f, fm):
    emb, ids, ten = fm.columns()
    f.index_load(emb, ids=ids)
    f.set_tenants(ten)
    f.sparse_load(*fm.csr(0, fm.n_rows), fm.n_rows)
    f.tokvec_load(*fm.packed(0, fm.n_rows))


def _check_components(fm, q, ref_sc, rows, sc, comp, weights, what):
    """rows / scores / components [Q, k] of either m3 entry against the references over the fresh model"""
    wd, ws, wc = weights
    bar = (wc / (wd + ws + wc)) * 1e-4 + 1e-9
    assert np.isfinite(sc).all() and np.isfinite(comp).all(), what + ": a NaN or inf score"
    for qi in range(rows.shape[0]):
        live = np.nonzero(rows[qi] >= 0)[0]
        if not live.shape[0]:
            continue
        r = rows[qi, live]
        cos = fm.dense_cos(q["q_emb"][qi], r) if wd > 0 else np.zeros(len(r))
        assert np.abs(comp[qi, live, 0] - cos).max() < 1e-9, what + ": dense component"
        zero = np.array([not fm.rows[i].emb.any() for i in r]) | (not q["q_emb"][qi].any())
        assert (comp[qi, live, 0][zero] == 0.0).all(), what + ": a zero embedding scores 0.0"
        np.testing.assert_array_equal(S.bits(comp[qi, live, 1]), S.bits(ref_sc[qi, r] if ws > 0 else np.zeros(len(r))), err_msg=what + ": sparse component")
        vq = q["qv"][q["qo"][qi]:q["qo"][qi + 1]]
        col = np.array([M.maxsim(vq, fm.rows[i].stored) if wc > 0 else 0.0 for i in r])
        assert np.abs(sc[qi, live] - F.combine(cos, ref_sc[qi, r] if ws > 0 else 0.0, col, weights)).max() < bar, what + ": score"
        np.testing.assert_array_equal(S.bits(sc[qi, live]), S.bits(F.combine(comp[qi, live, 0], comp[qi, live, 1], comp[qi, live, 2], weights)),
                                      err_msg=what + ": combine")
        assert (np.diff(sc[qi, live]) <= 0).all(), what + ": order"


def _check_against_references(fm, q, slots, tenant, res):
    n = fm.n_rows
    _, ids, ten = fm.columns()
    ref_sc = fm.sparse_scores(q["sparse"])
    np.testing.assert_array_equal(S.bits(res["sparse scores"][0]), S.bits(ref_sc))
    ok = (slots >= 0) & (slots < n)
    np.testing.assert_array_equal(S.bits(res["sparse rows"][0]), S.bits(np.where(ok, np.take_along_axis(ref_sc, np.clip(slots, 0, n - 1).astype(np.int64), axis=1), 0.0)))
    for t in (-1, tenant):
        e_rows, e_sc = S.topk_all(ref_sc, K, None if t < 0 else ten != t)
        g_ids, g_rows, g_sc = res[f"sparse topk {t}"]
        np.testing.assert_array_equal(g_rows, e_rows)
        np.testing.assert_array_equal(g_ids, np.where(e_rows >= 0, ids[np.maximum(e_rows, 0)], -1))
        np.testing.assert_array_equal(S.bits(g_sc), S.bits(e_sc))
    stored, off = fm.packed(0, n, stored=True)
    r_ids, r_rows, r_sc, ps = res["rerank"]
    empty = V.slot_empty(q["qo"], off, slots)
    assert (ps[empty] == 0).all() and np.abs(ps - V.pair_scores(q["qv"], q["qo"], stored, off, slots)).max() < 1e-4
    e_ids, e_rows, e_sc = V.stable_topk(ps, slots, empty, min(K, slots.shape[1]), idmap=ids)
    np.testing.assert_array_equal(r_rows, e_rows)
    np.testing.assert_array_equal(r_ids, e_ids)
    np.testing.assert_array_equal(V.bits(r_sc), V.bits(e_sc))
    for w in F.WEIGHT_SETS:
        m_ids, m_rows, m_sc, m_comp = res[f"m3 rows {w}"]
        n_ok = ok.sum(axis=1)
        for qi in range(slots.shape[0]):                                # every slot that holds a row of the index is ranked, whatever its score
            assert (m_rows[qi, :n_ok[qi]] >= 0).all() and (m_rows[qi, n_ok[qi]:] == -1).all() and (m_ids[qi, n_ok[qi]:] == -1).all()
            assert sorted(m_rows[qi, :n_ok[qi]].tolist()) == sorted(slots[qi][ok[qi]].tolist())
            at = {int(r): j for j, r in enumerate(slots[qi])}
            if w[2] > 0:                                                 # the colbert component has the rerank's pair-score bits
                j = [at[int(r)] for r in m_rows[qi, :n_ok[qi]]]
                np.testing.assert_array_equal(S.bits(m_comp[qi, :n_ok[qi], 2]), S.bits(ps[qi, j].astype(np.float64)))
        np.testing.assert_array_equal(m_ids, np.where(m_rows >= 0, ids[np.maximum(m_rows, 0)], -1))
        _check_components(fm, q, ref_sc, m_rows, m_sc, m_comp, w, f"m3_score_rows {w}")
    row_of = {int(i): r for r, i in enumerate(ids)}
    for name in ("retrieve 0", "retrieve 1", "retrieve 2", f"retrieve 2 tenant {tenant}"):
        g_ids, g_sc, g_comp, g_cand = res[name]
        rows = np.array([[row_of[int(i)] if i >= 0 else -1 for i in line] for line in g_ids])
        for qi in range(rows.shape[0]):
            have = g_ids[qi][g_ids[qi] >= 0]
            assert set(have.tolist()) <= set(g_cand[qi].tolist()) and len(set(have.tolist())) == len(have), name
        if "tenant" in name:
            assert (ten[rows[rows >= 0]] == tenant).all(), name
        _check_components(fm, q, ref_sc, rows, g_sc, g_comp, F.WEIGHT_SETS[0], name)


FETCH_ALL = 400          # stores of more documents: a drawn sample and the documents around the rows a compaction removed


def _check_state(e, f, m, q, dev, rng, tenant, focus=()):
    """after one operation: the entries that need a stale leg refuse, the others answer; with every leg current, the live handle
    against a fresh handle and the references"""
    c = m.consistent()
    ptr, terms, wts = q["packed"]
    n = m.n_rows
    probe = np.tile(np.array([0, n - 1, -1, n], dtype=np.int32), (4, 1))
    assert e.dense_topk(q["q_emb"], 3)[0].shape == (4, 3)                # the dense leg never goes stale
    e.tokvec_rerank(q["qv"], q["qo"], probe, 2)                         # explicit rows: the store answers ahead of and behind the index
    if not c["sparse"]:
        _raises_state(lambda: e.sparse_topk(ptr, terms, wts, K))
        _raises_state(lambda: e.sparse_score_rows(ptr, terms, wts, probe))
        _raises_state(lambda: _m3_rows(e, q, dev, probe, (0.4, 0.2, 0.0)))
        for mode, w in ((0, (0.4, 0.2, 0.0)), (1, (1.0, 0.0, 0.0)), (2, (1.0, 0.0, 0.0))):
            _raises_state(lambda: _retrieve(e, dev, mode, w))
    if not c["tokvec"]:
        _raises_state(lambda: _m3_rows(e, q, dev, probe, (0.4, 0.0, 0.4)))
        _raises_state(lambda: _retrieve(e, dev, 0, (1.0, 0.0, 1.0)))
    # what does not need the stale leg still answers
    w_ok = (1.0, 0.2 if c["sparse"] else 0.0, 1.0 if c["tokvec"] else 0.0)
    assert _m3_rows(e, q, dev, probe, w_ok)[0].shape == (4, 4)
    assert _retrieve(e, dev, 0, w_ok)[0].shape == (4, K)
    if c["sparse"]:
        assert e.sparse_topk(ptr, terms, wts, K)[0].shape == (4, K)
    if not (c["sparse"] and c["tokvec"]):
        return None
    fm, fmap = m.fresh()
    _load_fresh(f, fm)
    nf = fm.n_rows
    pick = rng.permutation(nf)[:POOL - 2]
    zero = [i for i in range(nf) if not fm.rows[i].emb.any()]
    if zero and zero[0] not in pick:
        pick[0] = zero[0]                                                # a row with a zero embedding among the slots
    f_slots = np.stack([np.concatenate([rng.permutation(pick), [-1, nf]]) for _ in range(4)]).astype(np.int32)
    back = np.nonzero(fmap >= 0)[0]                                      # fresh row -> live row
    e_slots = np.where(f_slots < 0, -1, np.where(f_slots >= nf, n, back[np.clip(f_slots, 0, nf - 1)])).astype(np.int32)
    exp = _stack_results(f, q, dev, f_slots, tenant)
    got = _stack_results(e, q, dev, e_slots, tenant)
    _same(_mapped(got, fmap, nf), exp, "the live handle against a fresh handle")
    docs = range(nf) if nf <= FETCH_ALL else sorted({0, nf - 1, *[int(d) for d in rng.integers(0, nf, 100)], *[d for d in focus if 0 <= d < nf][:150]})
    for d in docs:
        np.testing.assert_array_equal(_f32(e.tokvec_fetch(int(back[d]))), _f32(fm.rows[d].stored), err_msg=f"tokvec_fetch of document {back[d]}")
    _check_against_references(fm, q, f_slots, tenant, exp)
    return got


def _run_sequence(case):
    from optimized_rag_amd import RagEngine
    w, m, q = MM.build_sequence(case)
    rng = np.random.default_rng([case["seed"], 7])
    f = _engine("p3 fresh")
    e = RagEngine(dim=w.emb_dim, device=0)
    try:
        e.set_option("sparse_tail_fold", -1)
        emb, ids, ten = m.columns()
        e.index_load(emb, ids=ids)
        e.set_tenants(ten)
        e.sparse_load(*m.csr(0, m.sp_base), m.sp_base)
        if m.sp_cov > m.sp_base:
            e.sparse_append(*m.csr(m.sp_base, m.sp_cov), m.sp_cov - m.sp_base)
        e.tokvec_reserve(m.tv_docs_cap, m.tv_rows_cap, w.tok_dim)
        e.tokvec_append(*m.packed(0, m.tv_docs))
        dev = _dev_queries(q)
        tenant = int(rng.integers(0, 3))
        last = _check_state(e, f, m, q, dev, rng, tenant)
        assert last is not None
        for op in case["ops"]:
            if op[0] == "compact":
                kind, row_map = MM.apply(m, op)
                got_map = e.index_compact(keep_resident=True)
                np.testing.assert_array_equal(got_map, row_map)
                assert e.n_rows == m.n_rows and e.tokvec_info()["n_docs"] == m.tv_docs and e.tokvec_info()["rows"] == m.tv_rows()
                st = e.sparse_segment_stats()
                assert (st["base_docs"], st["tail_docs"]) == (m.sp_base, m.sp_cov - m.sp_base)
                gone = np.nonzero(row_map < 0)[0]
                at = gone - np.arange(len(gone))                         # the new number of the first live row behind each removed one
                now = _check_state(e, f, m, q, dev, rng, tenant, focus=sorted({int(a) + j for a in at for j in (-2, -1, 0, 1)}))
                if last is not None and now is not None:
                    # the results from before the call, through the row map (the slots are drawn anew: the entries without slots)
                    before = {k_: v for k_, v in _mapped(last, row_map, m.n_rows).items() if k_.startswith(("sparse scores", "sparse topk", "retrieve"))}
                    _same(before, {k_: now[k_] for k_ in before}, "before the compaction, through the row map")
                last = now
                continue
            kind, payload = MM.apply(m, op)
            if payload is None:
                continue
            if kind == "insert":
                e.index_insert(np.stack([d.emb for d in payload]), ids=np.array([d.id for d in payload], dtype=np.int64),
                               tenants=np.array([d.tenant for d in payload], dtype=np.int32))
            elif kind == "sparse_append":
                lo, hi, n_terms = payload
                e.sparse_append(*m.csr(lo, hi), hi - lo, n_terms)
            elif kind == "tokvec_append":
                e.tokvec_append(*m.packed(*payload))
            elif kind == "delete":
                assert e.index_delete(payload[1]) == len(payload[1])
            elif kind == "fold":
                e.sparse_fold()
                assert e.sparse_segment_stats()["tail_docs"] == 0
            last = _check_state(e, f, m, q, dev, rng, tenant)
    finally:
        e.close()


@MM.prop("p3_small")
@given(case=MM.sequence_cases(MM.SMALL_STARTS))
def test_p3_write_sequences_from_small_starts(case):
    """25 examples, 3.5 s: starts of 1-50 and 2040-2056 rows. After every operation the entries that need a stale leg return
    RAG_ERR_STATE and the others answer; in every state with all legs current the live handle equals a fresh handle loaded from
    the surviving documents, bit for bit, and the references (sparse bit-exact, dense within 1e-9, score within (w_colbert / sum)
    * 1e-4 + 1e-9); after a compaction the results from before the call, through the row map, are the results after it."""
    _run_sequence(case)


@MM.prop("p3_large")
@given(case=MM.sequence_cases(MM.LARGE_STARTS))
def test_p3_write_sequences_from_large_starts(case):
    """7 examples, 1.9 s: the same from starts of 3000-5000 rows (two or three 2048-document ranges, token stores of up to 100,000 rows)."""
    _run_sequence(case)
