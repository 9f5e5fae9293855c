"""GPU: the row-aligned planes of the resident index (emb32, emb16, ids, tenants, temporal, vis and the token store's three) across
every capacity boundary a live write can cross, each with the smallest index that crosses it.

A written-to handle is compared with a fresh handle loaded with the same final rows: dense_topk ids, rows and score bits,
fetch_rows bits, and the token store read back through the pair builder (as tests/test_wide_tokens_gpu.py reads it). Nothing
here depends on how a capacity is kept, only on what the planes hold afterwards."""
import ctypes as C

import numpy as np
import pytest

import xlmr_tools as X

pytestmark = pytest.mark.gpu

DIM, L, K = 64, 8, 10
CLS, SEP = 101, 102


@pytest.fixture()
def make():
    from optimized_rag_amd import RagEngine
    made = []

    def mk():
        e = RagEngine(dim=DIM, device=0)
        made.append(e)
        return e

    yield mk
    for e in made:
        e.close()


class Rows:
    """Every row the handle stores, in row order, with its planes and live flag."""

    def __init__(self, rng, n, bits=0, id0=5000):
        self.emb = rng.standard_normal((n, DIM)).astype(np.float32)
        self.ids = (id0 + rng.permutation(n)).astype(np.int64)
        self.ten = rng.integers(0, 3, n).astype(np.int32)
        self.tmp = rng.random(n)
        self.tok = rng.integers(0, 1 << (bits or 16), (n, L)).astype(np.int32)
        self.tok[:, 0] = (1 << (bits or 16)) - 1 - np.arange(n) % 200      # a value per row that needs every plane of the store
        self.tok_len = rng.integers(0, L + 1, n).astype(np.int32)
        self.tok_len[[0, -1]] = L
        self.live = np.ones(n, dtype=bool)

    def block(self, a, b, ids=True, tenants=False, temporal=False, tokens=False):
        return dict(emb=self.emb[a:b], ids=self.ids[a:b] if ids else None, tenants=self.ten[a:b] if tenants else None,
                    temporal=self.tmp[a:b] if temporal else None, tokens=self.tok[a:b] if tokens else None,
                    token_lens=self.tok_len[a:b] if tokens else None)


def n_rows_of(e):
    n = C.c_int64()
    assert e.lib.rag_index_rows(e.h, C.byref(n)) == 0
    return int(n.value)


def queries(rng, r, n):
    """near the first, the last and four other stored rows among the first n"""
    src = np.concatenate([[0, n - 1], rng.integers(0, n, 4)])
    return (r.emb[src] + 0.4 * rng.standard_normal((len(src), DIM))).astype(np.float32)


def same_as_fresh(make, e, r, n, q, ids=None, tenants=None):
    """e holds rows [0, n) of r (some deleted): it answers as a fresh handle loaded with the live ones in row order"""
    assert n_rows_of(e) == n
    lv = np.flatnonzero(r.live[:n])
    ids = r.ids[:n] if ids is None else ids
    f = make()
    f.index_load(r.emb[lv], ids=ids[lv])
    if tenants is not None:
        f.set_tenants(r.ten[lv])
    for t in [-1] + ([tenants] if tenants is not None else []):
        gi, gr, gs = e.dense_topk(q, K, tenant=t)
        fi, fr, fs = f.dense_topk(q, K, tenant=t)
        np.testing.assert_array_equal(gi, fi)
        np.testing.assert_array_equal(gr, np.where(fr >= 0, lv[np.maximum(fr, 0)], -1))
        np.testing.assert_array_equal(gs.view(np.int64), fs.view(np.int64))                  # score bits
    np.testing.assert_array_equal(e.fetch_rows(lv).view(np.uint32), f.fetch_rows(np.arange(len(lv))).view(np.uint32))
    f.close()


def same_store(e, r, n, bits):
    """the token store holds rows [0, n) of r (a deleted row stays in place until the compaction)"""
    assert e.tokens_info() == {"rows": n, "L": L, "id_bits": bits}
    cand = np.concatenate([np.arange(n), [-1, n, n + 9]]).astype(np.int64).reshape(1, -1)
    q_tok, q_len = np.zeros((1, 1), dtype=np.int32), np.zeros(1, dtype=np.int32)
    want = X.build_pairs(q_tok, q_len, cand, r.tok[:n], r.tok_len[:n], L + 3, CLS, SEP)
    for got, exp in zip(X.device_pairs(e, q_tok, q_len, cand, L + 3, CLS, SEP), want):
        np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("bits", [16, 24])
def test_every_plane_grows_across_both_boundaries(make, bits):
    """2,040 rows with every plane, then blocks of 1 (every plane but emb16 grows: 2,041 > 2,040, to 2,040 + 255 + 256 = 2,551 rows),
    7 (2,048 rows: exactly emb16's padding, nothing grows), 300 (2,348 rows: emb16 alone grows, past its 2,048-row padding) and 250
    (2,598 rows: past the 2,551 rows of the first growth, every plane but emb16 grows again)."""
    rng = np.random.default_rng(100 + bits)
    r = Rows(rng, 2598, bits)
    e = make()
    n = 2040
    e.index_load(r.emb[:n], ids=r.ids[:n])
    e.set_tenants(r.ten[:n])
    e.set_temporal(r.tmp[:n])
    e.tokens_load(r.tok[:n], r.tok_len[:n], id_bits=bits)
    for b in (1, 7, 300, 250):
        assert e.index_insert(**r.block(n, n + b, tenants=True, temporal=True, tokens=True)) == n
        n += b
        same_as_fresh(make, e, r, n, queries(rng, r, n), tenants=1)
        same_store(e, r, n, bits)


@pytest.mark.parametrize("reserved", [False, True], ids=["exact", "reserved"])
def test_implicit_ids_become_a_stored_column(make, reserved):
    """100 rows that answer to 500 + row, then 300 rows that bring ids (400 rows > 100 + 12 + 256: growth by the need itself where
    the index has no spare capacity; none where rag_index_reserve left 5,000 rows, but for the id column, which starts here)."""
    rng = np.random.default_rng(200)
    r = Rows(rng, 400)
    e = make()
    if reserved:
        e.index_reserve(5000, id_base=500)
        e.index_append(r.emb[:100])
    else:
        e.index_load(r.emb[:100], id_base=500)
    ids = np.concatenate([500 + np.arange(100), r.ids[100:]]).astype(np.int64)
    assert (r.ids >= 5000).all()
    same_as_fresh(make, e, r, 100, queries(rng, r, 100), ids=ids[:100])
    assert e.index_insert(**r.block(100, 400)) == 100
    same_as_fresh(make, e, r, 400, queries(rng, r, 400), ids=ids)
    assert e.index_delete(np.array([500, 599, ids[399]])) == 3                        # old rows by 500 + row, a new one by its id
    r.live[[0, 99, 399]] = False
    same_as_fresh(make, e, r, 400, queries(rng, r, 400), ids=ids)


@pytest.mark.parametrize("bits", [16, 24])
def test_inserts_inside_and_past_a_token_reservation(make, bits):
    """A store reserved for 150 rows and filled to the index's 100: 30 rows fit the reservation, 40 more (170 rows) do not."""
    import torch
    rng = np.random.default_rng(300 + bits)
    r = Rows(rng, 170, bits)
    e = make()
    e.index_load(r.emb[:100], ids=r.ids[:100])
    e.tokens_reserve(150, L, id_bits=bits)
    e.tokens_append_dev(torch.from_numpy(r.tok[:100].copy()).cuda(), torch.from_numpy(r.tok_len[:100].copy()).cuda())
    torch.cuda.synchronize()
    n = 100
    same_store(e, r, n, bits)
    for b in (30, 40):
        assert e.index_insert(**r.block(n, n + b, tokens=True)) == n
        n += b
        same_as_fresh(make, e, r, n, queries(rng, r, n))
        same_store(e, r, n, bits)


def test_vis_is_created_grown_dropped_and_created_again(make):
    """Deletes create vis for the 300 rows there are; 50 inserted rows do not fit it; the compaction drops it and maps the rows; the
    next delete creates it again."""
    rng = np.random.default_rng(400)
    r = Rows(rng, 360)
    e = make()
    e.index_load(r.emb[:300], ids=r.ids[:300])
    dead = np.concatenate([[0, 299], rng.choice(np.arange(1, 299), 18, replace=False)])
    assert e.index_delete(r.ids[dead]) == 20
    r.live[dead] = False
    same_as_fresh(make, e, r, 300, queries(rng, r, 300))
    assert e.index_insert(**r.block(300, 350)) == 300
    same_as_fresh(make, e, r, 350, queries(rng, r, 350))
    row_map = e.index_compact()
    lv = np.flatnonzero(r.live[:350])
    want = np.full(350, -1, dtype=np.int64)
    want[lv] = np.arange(len(lv))
    np.testing.assert_array_equal(row_map, want)
    assert e.index_deleted_rows() == 0
    keep = np.concatenate([lv, np.arange(350, 360)])
    for name in ("emb", "ids", "ten", "tmp", "tok", "tok_len"):
        setattr(r, name, getattr(r, name)[keep])
    r.live = np.ones(len(keep), dtype=bool)
    n = len(lv)
    same_as_fresh(make, e, r, n, queries(rng, r, n))
    assert e.index_insert(**r.block(n, n + 10)) == n
    n += 10
    assert e.index_delete(r.ids[[1, n - 1, n - 4, 77, 200]]) == 5
    r.live[[1, n - 1, n - 4, 77, 200]] = False
    same_as_fresh(make, e, r, n, queries(rng, r, n))


def test_an_insert_starts_the_planes_of_an_empty_handle(make):
    """No index: the first block brings ids, tenants and temporal scores and starts those planes; a block without them is then
    refused and changes nothing; one with them is taken."""
    rng = np.random.default_rng(500)
    r = Rows(rng, 120)
    e = make()
    assert e.index_insert(**r.block(0, 50, tenants=True, temporal=True)) == 0
    q = queries(rng, r, 50)
    same_as_fresh(make, e, r, 50, q, tenants=2)
    before = e.dense_topk(q, K)
    with pytest.raises(Exception, match="tenants are required iff the index has a tenant table"):
        e.index_insert(**r.block(50, 80))
    with pytest.raises(Exception, match="temporal scores are required iff the index has them"):
        e.index_insert(**r.block(50, 80, tenants=True))
    assert n_rows_of(e) == 50
    for a, b in zip(before, e.dense_topk(q, K)):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    assert e.index_insert(**r.block(50, 120, tenants=True, temporal=True)) == 50
    same_as_fresh(make, e, r, 120, queries(rng, r, 120), tenants=2)


def test_temporal_scores_outlive_an_index_reload(make):
    """PINS current behaviour, not an endorsement: the temporal scores are no plane of the index proper, so rag_index_load_host
    does not drop the 300 set before it. The 100-row index that follows counts as one that has them: a block without temporal
    scores is refused, a block with them is taken."""
    rng = np.random.default_rng(600)
    r = Rows(rng, 300)
    e = make()
    e.index_load(r.emb, ids=r.ids)
    e.set_temporal(r.tmp)
    e.index_load(r.emb[:100], ids=r.ids[:100])
    with pytest.raises(Exception, match="temporal scores are required iff the index has them"):
        e.index_insert(**r.block(100, 110))
    assert n_rows_of(e) == 100
    assert e.index_insert(**r.block(100, 110, temporal=True)) == 100
    same_as_fresh(make, e, r, 110, queries(rng, r, 110))
