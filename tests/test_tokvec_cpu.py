"""CPU-only: the float64 reference of the token-vector rerank (tests/tokvec_tools.py) against a plain double loop, the fp16
storage bound of include/rag_hip.h (rag_tokvec_*) on unit vectors, and the presence of the new entry points in the header, the
ctypes table and the built library. No compute calls (there is no GPU here)."""
import os
import re

import numpy as np

import __graft_entry__ as G
import tokvec_tools as V

SYMBOLS = ("rag_tokvec_reserve", "rag_tokvec_append_dev", "rag_tokvec_append_host", "rag_tokvec_load_host", "rag_tokvec_info",
           "rag_tokvec_fetch_host", "rag_tokvec_rerank_dev", "rag_tokvec_rerank_host", "rag_retrieve_maxsim_dev")


def _loop_maxsim(vq, vd):
    if len(vq) == 0 or len(vd) == 0:
        return 0.0
    total = 0.0
    for a in vq:
        best = -float("inf")
        for b in vd:
            best = max(best, float(sum(float(x) * float(y) for x, y in zip(a, b))))
        total += best
    return total / len(vq)


def test_reference_against_a_plain_loop():
    rng = np.random.default_rng(5)
    dim = 8
    d_rows = [0, 1, 3, 5]
    q_rows = [0, 2, 3]
    dv = -np.abs(rng.standard_normal((sum(d_rows), dim))).astype(np.float32)          # every dot with a positive query is negative
    qv = np.abs(rng.standard_normal((sum(q_rows), dim))).astype(np.float32)
    d_off, q_off = np.concatenate([[0], np.cumsum(d_rows)]), np.concatenate([[0], np.cumsum(q_rows)])
    cand = np.array([[0, 1, 2, 3, -1, 4], [3, -1, 2, 2, 9, 0], [1, 3, 3, -5, 2, 0]], dtype=np.int32)
    got = V.pair_scores(qv, q_off, dv, d_off, cand)
    empty = V.slot_empty(q_off, d_off, cand)
    for q in range(3):
        for j in range(cand.shape[1]):
            d = int(cand[q, j])
            is_empty = d < 0 or d >= len(d_rows) or d_rows[d] == 0 or q_rows[q] == 0
            assert bool(empty[q, j]) == is_empty
            exp = 0.0 if is_empty else _loop_maxsim(qv[q_off[q]:q_off[q + 1]], dv[d_off[d]:d_off[d + 1]])
            assert abs(got[q, j] - exp) < 1e-12
    assert (got[1][~empty[1]] < 0).all() and empty[0].all()
    # stable top-k: empty slots left out wherever they sit, equal scores (the duplicated candidate) in candidate order
    ids, rows, sc = V.stable_topk(got, cand, empty, 4, id_base=100)
    np.testing.assert_array_equal(rows[0], [-1] * 4)
    np.testing.assert_array_equal(sc[0], [0.0] * 4)
    live = [(got[1, j], j) for j in range(cand.shape[1]) if not empty[1, j]]
    order = sorted(live, key=lambda t: (-t[0], t[1]))
    np.testing.assert_array_equal(rows[1][:len(order)], [cand[1, j] for _, j in order])
    assert (rows[1][len(order):] == -1).all() and (ids[1][:len(order)] == rows[1][:len(order)] + 100).all()
    dup = [i for i in range(3) if rows[1][i] == 2]
    assert len(dup) == 2 and dup[1] == dup[0] + 1 and sc[1][dup[0]] == sc[1][dup[1]]
    ids2, _, _ = V.stable_topk(got, cand, empty, 2, idmap=np.array([7, 5, 3, 1]))
    np.testing.assert_array_equal(ids2[1], [[7, 5, 3, 1][r] for r in rows[1][:2]])


def test_fp16_storage_moves_a_maxsim_of_unit_vectors_by_less_than_the_bound():
    """Contract (b): rounding the stored rows to fp16 moves <q, d> of unit vectors by at most 2^-11 * sum |q_i d_i| <= 2^-11 (plus
    fp16 subnormals: 2^-25 * sqrt(dim)), and a mean of maxima is 1-Lipschitz in that error."""
    bound = 2.0 ** -11 + 2.0 ** -20
    rng = np.random.default_rng(11)
    worst = worst_same = 0.0
    for dim in (32, 96, 128, 384, 1024):
        q, d = V.unit_rows(rng, 33, dim), V.unit_rows(rng, 129, dim)
        off_q, off_d = np.array([0, 33]), np.array([0, 129])
        cand = np.zeros((1, 1), dtype=np.int32)
        a = V.pair_scores(q, off_q, d, off_d, cand)[0, 0]
        b = V.pair_scores(q, off_q, V.fp16_round(d), off_d, cand)[0, 0]
        worst = max(worst, abs(a - b))
        assert abs(a - b) <= bound
        # rows whose components all round the same way (down in magnitude) against queries of the same signs: the errors add up.
        # The rows are NOT renormalised after the nudge (dividing by the norm, 1.0003, would take the 0.49 ulp away again and
        # leave randomly rounded rows): their norms lie within 1e-3 of 1, which the derivation of the bound absorbs
        # (2^-11 * |q| * |d|, and the measured figure is under half of it).
        h = V.fp16_round(d)
        step = np.spacing(np.abs(h).astype(np.float16)).astype(np.float32)
        up = ((np.abs(h) + np.float32(0.49) * step) * np.sign(h)).astype(np.float32)      # rounds back to h: every component loses 0.49 ulp
        back = V.fp16_round(up)
        down = float((np.abs(back) < np.abs(up)).mean())
        assert down >= 0.95 and not (np.abs(back) > np.abs(up)).any(), f"dim {dim}: only {down:.2%} of the components round down"
        assert np.abs(np.linalg.norm(up.astype(np.float64), axis=1) - 1.0).max() < 1e-3
        qs = np.concatenate([np.abs(q[i]) * np.sign(up[i * 3]) for i in range(33)]).reshape(33, dim).astype(np.float32)
        a = V.pair_scores(qs, off_q, up, off_d, cand)[0, 0]
        b = V.pair_scores(qs, off_q, back, off_d, cand)[0, 0]
        assert b < a, "rounding every component towards zero must lower a MaxSim of sign-aligned rows"
        worst_same = max(worst_same, abs(a - b))
        assert abs(a - b) <= bound
    print(f"fp16 storage: seeded unit vectors move MaxSim by at most {worst:.2e}, same-direction rounding rows by {worst_same:.2e} "
          f"(bound {bound:.2e})")


def test_new_symbols_in_header_ctypes_table_and_library():
    G.build()
    import optimized_rag_amd
    from optimized_rag_amd import _lib
    lib = optimized_rag_amd.load_library()
    hdr = open(os.path.join(G.ROOT, "include", "rag_hip.h")).read()
    declared = set(re.findall(r"\b(rag_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert name in declared, f"{name} not declared in rag_hip.h"
        assert name in _lib.exported_symbols(), f"{name} missing from the ctypes table"
        assert hasattr(lib, name), f"{name} not exported by librag_hip.so"
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.document_store import GpuDocumentIndex
    for m in ("tokvec_reserve", "tokvec_append", "tokvec_append_dev", "tokvec_load", "tokvec_info", "tokvec_fetch", "tokvec_rerank",
              "tokvec_rerank_dev", "retrieve_maxsim_dev"):
        assert callable(getattr(RagEngine, m, None)), m
    for m in ("load_token_vectors", "build_token_vectors", "search_late_interaction"):
        assert callable(getattr(GpuDocumentIndex, m, None)), m
