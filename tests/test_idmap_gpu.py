"""GPU: the device id-to-row map (rag_index_id_map, rag_index_rows_of_ids_*, rag_index_id_map_info) on one handle, against a
dict and the numpy model of tests/idmap_tools.py. Everything is exact."""
import numpy as np
import pytest

from idmap_tools import IdMapModel, colliding_ids, home, slots_for

pytestmark = pytest.mark.gpu

D = 64


@pytest.fixture(scope="module")
def make():
    from optimized_rag_amd import RagEngine
    made = []

    def mk():
        e = RagEngine(dim=D, device=0)
        made.append(e)
        return e

    yield mk
    for e in made:
        e.close()


def rows_emb(rng, n):
    return rng.standard_normal((n, D)).astype(np.float32)


def grow_cap(cap, need):
    """the row capacity after an insert (csrc/live.hip grow_cap)"""
    return cap if need <= cap else max(need, cap + cap // 8 + 256)


def reserved(make, rng, cap, ids):
    """a handle with room for `cap` rows, len(ids) rows appended, explicit ids"""
    e = make()
    e.index_reserve(cap)
    e.index_append(rows_emb(rng, len(ids)))
    e.set_ids(np.asarray(ids, dtype=np.int64))
    return e


def check_lookups(e, d, extra=()):
    """every id of the dict resolves to its row; the extras, -1 and ids beside the known ones to -1"""
    known = np.fromiter(d.keys(), dtype=np.int64, count=len(d))
    ask = np.concatenate([known, np.asarray(list(extra), dtype=np.int64), [-1, -2, -(1 << 63)], known[:50] + (1 << 40)])
    exp = np.array([d.get(int(i), -1) for i in ask], dtype=np.int32)
    np.testing.assert_array_equal(e.rows_of_ids(ask), exp)


def refused(call, code, *words):
    from optimized_rag_amd import RagError
    with pytest.raises(RagError) as ei:
        call()
    msg = str(ei.value)
    assert f"({code})" in msg, msg
    for w in words:
        assert w in msg, msg


def test_chain_wraps_the_table_end_erase_and_reinsert(make):
    rng = np.random.default_rng(0)
    base = 1000 + np.arange(300, dtype=np.int64)
    e = reserved(make, rng, 5000, base)
    e.index_id_map()
    info = e.index_id_map_info()
    slots = info["slots"]
    assert info["enabled"] == 1 and slots == slots_for(5000) and info["entries"] == 300 and info["tombstones"] == 0
    assert info["hbm_bytes"] == 12 * slots and info["ids_ascending"] == 1 and info["rebuilds"] == 0
    assert 1 <= info["longest_probe"] <= 3                                        # serial ids: at most two per home slot
    d = {int(i): r for r, i in enumerate(base)}
    check_lookups(e, d)

    chain = colliding_ids(slots, slots - 3, 70, exclude=base)                    # 70 keys from slot slots - 3: past the table end
    assert (home(chain, slots) == slots - 3).all()
    first = e.index_insert(rows_emb(rng, 70), ids=chain)
    assert first == 300
    d.update({int(i): first + j for j, i in enumerate(chain)})
    info = e.index_id_map_info()
    assert info["slots"] == slots and info["entries"] == 370 and info["rebuilds"] == 0
    assert info["longest_probe"] >= 70
    check_lookups(e, d)

    # erase one id of the chain: whichever slot it had, the ids behind it are still found
    gone = int(chain[35])
    assert e.index_delete([gone]) == 1
    row_gone = d.pop(gone)
    info = e.index_id_map_info()
    assert (info["entries"], info["tombstones"]) == (369, 1)
    check_lookups(e, d, extra=[gone])
    # the same id on a new row takes its slot back
    first = e.index_insert(rows_emb(rng, 1), ids=[gone])
    assert first == 370 and first != row_gone
    d[gone] = first
    info = e.index_id_map_info()
    assert (info["entries"], info["tombstones"], info["rebuilds"]) == (370, 0, 0)
    check_lookups(e, d)

    # id 0 and ids near 2^62 (and the largest int64)
    far = np.array([0, (1 << 62) - 1, 1 << 62, (1 << 62) + 1, (1 << 63) - 1], dtype=np.int64)
    first = e.index_insert(rows_emb(rng, 5), ids=far)
    d.update({int(i): first + j for j, i in enumerate(far)})
    check_lookups(e, d, extra=[(1 << 62) + 2, 1, (1 << 63) - 2])
    assert e.index_id_map_info()["ids_ascending"] == 0                            # the id taken back was below the last live id


def test_tombstones_until_a_rebuild_and_growth_past_the_reservation(make):
    rng = np.random.default_rng(1)
    cap, n = 1000, 600
    ids = 7 + 3 * np.arange(n, dtype=np.int64)
    e = reserved(make, rng, cap, ids)
    e.index_id_map()
    m = IdMapModel(cap)
    m.build([(int(i), r) for r, i in enumerate(ids)], count=False)
    d = {int(i): r for r, i in enumerate(ids)}
    next_id = int(ids[-1]) + 1

    def same_as_model():
        info = e.index_id_map_info()
        assert (info["slots"], info["entries"], info["tombstones"], info["rebuilds"]) == (m.slots, m.entries, m.tombstones, m.rebuilds)
        return info

    same_as_model()
    for rnd in range(4):                                  # 100 deletes + 100 inserts per round, inside the reservation
        victims = rng.choice(np.fromiter(d.keys(), dtype=np.int64), 100, replace=False)
        assert e.index_delete(victims) == 100
        for v in victims:
            assert m.erase(int(v))
            del d[int(v)]
        blk = next_id + np.arange(100, dtype=np.int64)
        next_id += 100
        assert not m.must_rebuild(100, cap)
        first = e.index_insert(rows_emb(rng, 100), ids=blk)
        m.insert(blk, first)
        d.update({int(i): first + j for j, i in enumerate(blk)})
        info = same_as_model()
        assert info["tombstones"] == 100 * (rnd + 1) and info["ids_ascending"] == 1
        check_lookups(e, d, extra=victims)
    # the insert that passes the reservation grows the table and drops the tombstones
    n0 = 1000
    blk = next_id + np.arange(40, dtype=np.int64)
    new_cap = grow_cap(cap, n0 + 40)
    assert m.must_rebuild(40, new_cap)
    first = e.index_insert(rows_emb(rng, 40), ids=blk)
    assert first == n0
    d.update({int(i): first + j for j, i in enumerate(blk)})
    m.build(sorted(d.items(), key=lambda kv: kv[1]), new_cap)
    info = same_as_model()
    assert info["tombstones"] == 0 and info["rebuilds"] == 1 and info["slots"] == slots_for(new_cap) > slots_for(cap)
    check_lookups(e, d)
    # a deleted id inserted again on a new row resolves to the new row
    victim = int(victims[0])                              # deleted in the last round
    assert victim not in d and e.rows_of_ids([victim])[0] == -1
    first = e.index_insert(rows_emb(rng, 1), ids=[victim])
    d[victim] = first
    check_lookups(e, d)
    assert e.index_id_map_info()["ids_ascending"] == 0   # that id is below the last live id


@pytest.mark.parametrize("variant", ["compact", "compact_bm25", "compact_live"])
def test_every_compact_rebuilds_the_map(make, variant):
    rng = np.random.default_rng(2)
    n = 3000
    ids = 7 + 3 * np.arange(n, dtype=np.int64)
    e = make()
    e.index_load(rows_emb(rng, n), ids=ids)
    e.index_id_map()
    assert e.index_id_map_info()["slots"] == slots_for(n)
    victims = rng.choice(ids, 700, replace=False)
    assert e.index_delete(victims) == 700
    assert e.index_id_map_info()["tombstones"] == 700
    row_map = e.index_compact(keep_postings=variant == "compact_bm25", keep_resident=variant == "compact_live")
    d = {int(i): int(row_map[r]) for r, i in enumerate(ids) if row_map[r] >= 0}
    assert len(d) == n - 700 and sorted(d.values()) == list(range(n - 700))
    info = e.index_id_map_info()
    assert (info["entries"], info["tombstones"], info["rebuilds"], info["ids_ascending"]) == (n - 700, 0, 1, 1)
    check_lookups(e, d, extra=victims)
    # with nothing deleted a compaction moves nothing and rebuilds nothing
    e.index_compact(keep_postings=variant == "compact_bm25", keep_resident=variant == "compact_live")
    assert e.index_id_map_info()["rebuilds"] == 1


def test_set_ids_rebuilds_and_decides_the_order_again(make):
    rng = np.random.default_rng(3)
    n = 1500
    e = make()
    e.index_load(rows_emb(rng, n), ids=np.arange(n, dtype=np.int64))
    e.index_id_map()
    perm = rng.permutation(n).astype(np.int64) * 5 + 11
    e.set_ids(perm)
    info = e.index_id_map_info()
    assert (info["enabled"], info["ids_ascending"], info["rebuilds"], info["entries"]) == (1, 0, 1, n)
    check_lookups(e, {int(i): r for r, i in enumerate(perm)}, extra=[0, 1, 2])
    asc = np.sort(perm)
    e.set_ids(asc)
    info = e.index_id_map_info()
    assert (info["ids_ascending"], info["rebuilds"]) == (1, 2)
    check_lookups(e, {int(i): r for r, i in enumerate(asc)})
    # a duplicate given to set_ids: the ids are set, the map is disabled, the handle goes on
    dup = asc.copy()
    dup[700] = dup[3]
    refused(lambda: e.set_ids(dup), -1, "duplicate", str(int(dup[3])))
    assert e.index_id_map_info()["enabled"] == 0
    assert e.dense_topk(rows_emb(rng, 2), 5)[0].shape == (2, 5)


def test_the_order_of_ids_through_inserts_and_deletes(make):
    rng = np.random.default_rng(4)
    e = reserved(make, rng, 2000, 10 * np.arange(300, dtype=np.int64))
    e.index_id_map()
    assert e.index_id_map_info()["ids_ascending"] == 1
    e.index_insert(rows_emb(rng, 3), ids=[3000, 3010, 3020])
    assert e.index_id_map_info()["ids_ascending"] == 1
    # the last live rows go: an id above what is left still ascends, wherever the deleted ids were
    assert e.index_delete([3000, 3010, 3020, 2990]) == 4
    e.index_insert(rows_emb(rng, 2), ids=[2985, 2995])
    assert e.index_id_map_info()["ids_ascending"] == 1
    e.index_insert(rows_emb(rng, 2), ids=[4000, 3999])                          # a block that descends in itself
    assert e.index_id_map_info()["ids_ascending"] == 0
    f = reserved(make, rng, 2000, 10 * np.arange(300, dtype=np.int64))
    f.index_id_map()
    f.index_insert(rows_emb(rng, 1), ids=[2985])                                 # a block of one, below the last live id 2990
    assert f.index_id_map_info()["ids_ascending"] == 0
    refused(lambda: f.index_insert(rows_emb(rng, 1), ids=[2990]), -1, "already live")
    assert f.index_id_map_info()["entries"] == 301 and f.rows_of_ids([2990, 2985]).tolist() == [299, 300]


def test_refusals_at_enable_leave_the_map_disabled_and_the_handle_usable(make):
    rng = np.random.default_rng(5)
    n = 400
    ids = 100 + np.arange(n, dtype=np.int64)
    emb = rows_emb(rng, n)
    e = make()
    e.index_load(emb, ids=ids)
    # explicit ids and no map
    refused(lambda: e.rows_of_ids([100]), -3, "id map")
    dup = ids.copy()
    dup[399] = dup[17]
    e.set_ids(dup)
    refused(lambda: e.index_id_map(), -1, "duplicate", str(int(dup[17])))
    assert e.index_id_map_info() == dict(enabled=0, ids_ascending=0, slots=0, entries=0, tombstones=0, longest_probe=0, hbm_bytes=0, rebuilds=0)
    refused(lambda: e.rows_of_ids([100]), -3, "id map")
    neg = ids.copy()
    neg[5] = -9
    e.set_ids(neg)
    refused(lambda: e.index_id_map(), -1, "negative", "-9")
    assert e.index_id_map_info()["enabled"] == 0
    # a duplicate that is deleted is no duplicate: the map holds the live rows
    e.set_ids(dup)
    assert e.index_delete([int(dup[17])]) == 2
    e.index_id_map()
    d = {int(i): r for r, i in enumerate(dup) if i != dup[17]}
    check_lookups(e, d, extra=[int(dup[17])])
    # a negative id in an insert while the map is enabled: refused before anything changes
    refused(lambda: e.index_insert(rows_emb(rng, 2), ids=[9000, -4]), -1, ">= 0")
    assert e.index_id_map_info()["entries"] == n - 2
    check_lookups(e, d)
    got = e.dense_topk(emb[:3], 1)[1][:, 0]
    np.testing.assert_array_equal(got, [0, 1, 2])
    # disabling frees the table; enabling again builds it again
    e.index_id_map(False)
    assert e.index_id_map_info()["enabled"] == 0
    refused(lambda: e.rows_of_ids([100]), -3, "id map")
    e.index_id_map()
    check_lookups(e, d)
    # a load replaces the index and drops the map
    e.index_load(emb, ids=ids)
    assert e.index_id_map_info()["enabled"] == 0


def test_implicit_ids_answer_by_arithmetic(make):
    rng = np.random.default_rng(6)
    n = 500
    e = make()
    e.index_load(rows_emb(rng, n), id_base=1000)
    ask = np.array([999, 1000, 1001, 1000 + n - 1, 1000 + n, -1, 0, 1 << 62], dtype=np.int64)
    exp = np.array([-1, 0, 1, n - 1, -1, -1, -1, -1], dtype=np.int32)
    np.testing.assert_array_equal(e.rows_of_ids(ask), exp)                       # legal without the map, too
    e.index_id_map()
    info = e.index_id_map_info()
    assert (info["enabled"], info["slots"], info["entries"], info["ids_ascending"], info["hbm_bytes"]) == (1, 0, 0, 1, 0)
    np.testing.assert_array_equal(e.rows_of_ids(ask), exp)
    assert e.index_delete([1001]) == 1
    exp[2] = -1
    np.testing.assert_array_equal(e.rows_of_ids(ask), exp)
    # the first insert with explicit ids stores the id column: the map gets its table then
    first = e.index_insert(rows_emb(rng, 2), ids=[5000, 5001])
    info = e.index_id_map_info()
    assert info["slots"] >= 2 * (n + 2) and info["entries"] == n + 1 and info["ids_ascending"] == 1
    d = {1000 + r: r for r in range(n) if r != 1}
    d.update({5000: first, 5001: first + 1})
    check_lookups(e, d, extra=[1001])
    # ... and a compaction of an implicit-id index does the same
    f = make()
    f.index_load(rows_emb(rng, n), id_base=1000)
    f.index_id_map()
    assert f.index_delete([1000, 1007]) == 2
    row_map = f.index_compact()
    info = f.index_id_map_info()
    assert info["slots"] == slots_for(n) and info["entries"] == n - 2 and info["ids_ascending"] == 1
    check_lookups(f, {1000 + r: int(row_map[r]) for r in range(n) if row_map[r] >= 0}, extra=[1000, 1007])


def test_dev_lookup_is_ordered_on_a_side_stream(make):
    import torch
    import stream_tools as S
    rng = np.random.default_rng(7)
    n = 5000
    ids = 7 + 3 * np.arange(n, dtype=np.int64)
    e = make()
    e.index_load(rows_emb(rng, n), ids=ids)
    e.index_id_map()
    assert e.index_delete(ids[100:110]) == 10
    real = rng.choice(np.concatenate([ids, ids + 1, [-1]]), 256 * 200).astype(np.int64)
    wrong = np.full_like(real, -1)
    exp = np.where((real - 7) % 3 == 0, (real - 7) // 3, -1)
    exp[(real < 7) | (exp >= n) | ((exp >= 100) & (exp < 110))] = -1

    def call(dev, stream):
        out = torch.empty(dev["ids"].numel(), dtype=torch.int32, device="cuda")
        e.rows_of_ids_dev(dev["ids"], out, stream=stream)
        return [out]

    ref = S.serial(call, {"ids": wrong}, {"ids": real})
    np.testing.assert_array_equal(ref[0], exp.astype(np.int32))
    got, pending = S.late_producer(call, {"ids": wrong}, {"ids": real}, torch.cuda.Stream())
    assert pending, "the call waited for its stream"
    S.assert_same(got, ref, "rows_of_ids_dev")
    np.testing.assert_array_equal(e.rows_of_ids(real), exp.astype(np.int32))
