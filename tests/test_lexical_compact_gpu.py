"""GPU: rag_lexical_compact_dev / _host against the numpy reference of tests/lexical_compact_tools.py, integer for integer and float
bit for float bit (no tolerance anywhere), on the smallest shapes at which the kernel can go wrong: sequence lengths that are no
power of two, one wave, the 256-thread workgroup, several keys per thread, the LDS limit (8192); empty, over-long, all-special and
one-id texts; the weight classes of the contract; ids 0, 2^31 - 1 and < 0; 0 and 8 skip ids; text counts that take the scan across
a wave, a workgroup and its per-thread loop; capacities at, below and far below the total; invariance; argument errors."""
import ctypes as C

import numpy as np
import pytest

import lexical_compact_tools as T

pytestmark = pytest.mark.gpu

ERR_ARG = r"\(-1\)"
GUARD_I, GUARD_F = np.int32(-77), np.float32(-5.5)


@pytest.fixture(scope="module")
def engine():
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=64, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases():
    """the cases with their reference, computed once"""
    out = T.cases()
    for c in out:
        c["ref"] = T.compact(c["ids"], c["weights"], c["lens"], c["skip"])
    return out


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_dev(e, ids, w, lens, skip, cap, guard=4):
    """(term_ptr, terms [cap + guard], qweights [cap + guard]) of the device form; the arrays start as guard values"""
    import torch
    n = ids.shape[0]
    ptr = torch.full((n + 1,), -9, dtype=torch.int32, device="cuda")
    terms = torch.full((cap + guard,), int(GUARD_I), dtype=torch.int32, device="cuda")
    qw = torch.full((cap + guard,), float(GUARD_F), dtype=torch.float32, device="cuda")
    e.lexical_compact_dev(_t(ids), _t(w), _t(lens), ptr, terms[:cap], qw[:cap], skip_ids=skip)
    torch.cuda.synchronize()
    return ptr.cpu().numpy(), terms.cpu().numpy(), qw.cpu().numpy()


def assert_bits(got, ref, what):
    for g, r, name in zip(got, ref, ("term_ptr", "terms", "qweights")):
        assert g.dtype == r.dtype, (what, name)
        np.testing.assert_array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, r.view(np.uint32) if r.dtype == np.float32 else r,
                                      err_msg=f"{what}: {name}")


def test_dev_and_host_equal_the_reference_on_every_case(engine, cases):
    for c in cases:
        rptr, rterms, rqw = c["ref"]
        total = int(rptr[-1])
        n, L = c["ids"].shape
        ptr, terms, qw = run_dev(engine, c["ids"], c["weights"], c["lens"], c["skip"], n * L)
        assert_bits((ptr, terms[:total], qw[:total]), c["ref"], c["name"] + " _dev")
        assert (terms[total:] == GUARD_I).all() and (qw[total:] == GUARD_F).all(), c["name"]
        assert_bits(engine.lexical_compact(c["ids"], c["weights"], c["lens"], skip_ids=c["skip"]), c["ref"], c["name"] + " _host")
        assert_bits(engine.lexical_compact(c["ids"], c["weights"], c["lens"], skip_ids=c["skip"], terms_cap=total), c["ref"],
                    c["name"] + " _host at the exact capacity")


@pytest.mark.parametrize("name", ["seq_len_300", "text_shapes", "n_texts_65"])
def test_capacity(engine, cases, name):
    c = next(x for x in cases if x["name"] == name)
    rptr, rterms, rqw = c["ref"]
    total = int(rptr[-1])
    assert total > 1
    for cap in (total, total - 1, 0):
        ptr, terms, qw = run_dev(engine, c["ids"], c["weights"], c["lens"], c["skip"], cap)
        np.testing.assert_array_equal(ptr, rptr)                       # term_ptr[n] is the true total whatever fits
        np.testing.assert_array_equal(terms[:cap], rterms[:cap])
        np.testing.assert_array_equal(qw[:cap].view(np.uint32), rqw[:cap].view(np.uint32))
        assert (terms[cap:] == GUARD_I).all() and (qw[cap:] == GUARD_F).all()          # nothing at or past the capacity
    for cap in (total - 1, 0):
        with pytest.raises(Exception, match=ERR_ARG):
            engine.lexical_compact(c["ids"], c["weights"], c["lens"], skip_ids=c["skip"], terms_cap=cap)
    assert_bits(engine.lexical_compact(c["ids"], c["weights"], c["lens"], skip_ids=c["skip"]), c["ref"], "after the refusals")


def test_a_text_is_a_function_of_its_own_row(engine):
    """alone, among neighbours, and at a larger seq_len with padding: the same slice"""
    rng = np.random.default_rng(5)
    ids, w, lens = T.random_texts(rng, 7, 70, vocab=25)
    lens[3] = 70
    refs = [T.compact(ids[i:i + 1], w[i:i + 1], lens[i:i + 1], (2, 3)) for i in range(7)]
    ptr, terms, qw = run_dev(engine, ids, w, lens, (2, 3), 7 * 70)
    wide_ids = np.full((7, 300), 9, dtype=np.int32)
    wide_w = np.full((7, 300), 7.0, dtype=np.float32)
    wide_ids[:, :70], wide_w[:, :70] = ids, w
    wptr, wterms, wqw = run_dev(engine, wide_ids, wide_w, np.minimum(lens, 70), (2, 3), 7 * 300)
    np.testing.assert_array_equal(ptr, wptr)
    for i in range(7):
        a, b = int(ptr[i]), int(ptr[i + 1])
        alone = run_dev(engine, ids[i:i + 1], w[i:i + 1], lens[i:i + 1], (2, 3), 70)
        for got_t, got_w in ((terms[a:b], qw[a:b]), (wterms[a:b], wqw[a:b]), (alone[1][:b - a], alone[2][:b - a])):
            np.testing.assert_array_equal(got_t, refs[i][1])
            np.testing.assert_array_equal(got_w.view(np.uint32), refs[i][2].view(np.uint32))
        assert alone[0].tolist() == [0, b - a]


def test_argument_errors_leave_the_handle_usable(engine, cases):
    import torch
    from optimized_rag_amd import RagError
    c = next(x for x in cases if x["name"] == "seq_len_33")
    ids, w, lens = c["ids"], c["weights"], c["lens"]
    with pytest.raises(RagError, match=ERR_ARG):
        engine.lexical_compact(ids, w, lens, skip_ids=range(9))
    with pytest.raises(RagError, match=ERR_ARG):
        engine.lexical_compact(np.zeros((1, 8193), np.int32), np.zeros((1, 8193), np.float32), [1])
    with pytest.raises(RagError, match=ERR_ARG):
        engine.lexical_compact(np.zeros((0, 4), np.int32), np.zeros((0, 4), np.float32), np.zeros(0, np.int32))
    d_ids, d_w, d_lens = _t(ids), _t(w), _t(lens)
    ptr = torch.zeros((ids.shape[0] + 1,), dtype=torch.int32, device="cuda")
    terms = torch.zeros((ids.size,), dtype=torch.int32, device="cuda")
    qw = torch.zeros((ids.size,), dtype=torch.float32, device="cuda")
    with pytest.raises(RagError, match=ERR_ARG):
        engine.lexical_compact_dev(d_ids, d_w, d_lens, ptr, terms, qw, skip_ids=range(9))
    with pytest.raises(RagError, match=ERR_ARG):
        engine.lexical_compact_dev(d_ids, d_w, d_lens, None, terms, qw)
    p = lambda t: C.c_void_p(t.data_ptr())
    for null in ("terms", "qweights"):                                  # a capacity > 0 with a NULL output array
        rc = engine.lib.rag_lexical_compact_dev(engine.h, p(d_ids), p(d_w), p(d_lens), ids.shape[0], ids.shape[1], None, 0, p(ptr),
                                                None if null == "terms" else p(terms), None if null == "qweights" else p(qw), ids.size, None)
        assert rc == -1
    rc = engine.lib.rag_lexical_compact_host(engine.h, C.c_void_p(ids.ctypes.data), C.c_void_p(w.ctypes.data), C.c_void_p(lens.ctypes.data),
                                             ids.shape[0], ids.shape[1], None, 0, None, None, None, ids.size)
    assert rc == -1
    torch.cuda.synchronize()
    got = run_dev(engine, ids, w, lens, c["skip"], ids.size)
    total = int(c["ref"][0][-1])
    assert_bits((got[0], got[1][:total], got[2][:total]), c["ref"], "after the errors")
