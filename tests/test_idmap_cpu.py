"""CPU-only: the numpy model of the id-to-row map (tests/idmap_tools.py) against a dict, the pinned hash, and the new entries'
declarations, exports and bindings (no GPU call is made)."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as G
from idmap_tools import EMPTY, IdMapModel, colliding_ids, home, slots_for

NEW = ["rag_index_id_map", "rag_index_rows_of_ids_dev", "rag_index_rows_of_ids_host", "rag_index_id_map_info"]


def test_hash_constant_is_pinned():
    """home(id) = ((uint64)id * 0x9E3779B97F4A7C15) >> (64 - log2(slots)), from integer arithmetic done by hand"""
    assert int(home(1, 1 << 7)) == 79                        # the constant's top 7 bits: 0x9E >> 1
    assert int(home(2, 1 << 11)) == 483
    assert int(home(12345678901, 1 << 15)) == 342
    assert int(home((1 << 62) + 5, 1 << 11)) == 696          # the product wraps modulo 2^64
    assert int(home(0, 1 << 15)) == 0
    for i, lg in ((1, 7), (2, 11), (12345678901, 15), ((1 << 62) + 5, 11)):
        assert int(home(i, 1 << lg)) == ((i * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)) >> (64 - lg)


@pytest.mark.parametrize("lg", [7, 11, 15])
def test_serial_keys_land_at_most_two_per_home_slot(lg):
    slots = 1 << lg
    for base in (0, 1, 7, 10 ** 6, 10 ** 12):
        assert np.bincount(home(base + np.arange(slots // 2), slots), minlength=slots).max() <= 2


def test_slots_rule():
    assert slots_for(0) == 128 and slots_for(64) == 128 and slots_for(65) == 256
    assert slots_for(5000) == 16384 and slots_for(8192) == 16384 and slots_for(8193) == 32768


def test_colliding_ids_share_the_slot():
    slots = 4096
    ids = colliding_ids(slots, slots - 3, 70)
    assert len(set(ids.tolist())) == 70 and ids.max() < 1 << 26 and (np.diff(ids) > 0).all()
    assert (home(ids, slots) == slots - 3).all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_model_equals_dict_through_random_writes(seed):
    """random insert / erase / re-insert sequences, collisions forced by a small id range and a chain that wraps the table end"""
    rng = np.random.default_rng(seed)
    cap = 200
    m = IdMapModel(cap)
    assert m.slots == 512
    d, n_rows = {}, 0
    pool = np.concatenate([rng.choice(5000, 300, replace=False), colliding_ids(m.slots, m.slots - 3, 80), [0, (1 << 62) + 3, (1 << 62) + 4]])
    for step in range(400):
        op = rng.integers(0, 3)
        if op == 0 or not d:
            free = [int(i) for i in pool if int(i) not in d]
            blk = [int(x) for x in rng.choice(free, size=min(len(free), int(rng.integers(1, 9))), replace=False)] if free else []
            if not blk:
                continue
            cap = max(cap, n_rows + len(blk))
            if m.must_rebuild(len(blk), cap):
                d.update({i: n_rows + j for j, i in enumerate(blk)})
                m.build(sorted(d.items(), key=lambda kv: kv[1]), cap)
                assert m.tombstones == 0
            else:
                m.insert(blk, n_rows)
                d.update({i: n_rows + j for j, i in enumerate(blk)})
            n_rows += len(blk)
        else:
            i = int(rng.choice(list(d)))
            assert m.erase(i) and not m.erase(i)
            del d[i]
        assert m.entries == len(d) and m.entries + m.tombstones <= m.slots // 2
        assert (m.keys != EMPTY).sum() == m.entries + m.tombstones
        for i in pool:
            assert m.lookup(int(i)) == d.get(int(i), -1), (step, int(i))
        assert m.lookup(-1) == -1 and m.lookup(123456789) == -1
    assert m.rebuilds > 0


def test_erase_keeps_the_chain_and_reinsert_reuses_the_slot():
    m = IdMapModel(300)
    ids = colliding_ids(m.slots, m.slots - 3, 64)
    m.insert(ids, 0)
    assert m.longest_probe == 64                            # one chain, wrapped around the table end
    used = int((m.keys != EMPTY).sum())
    assert m.erase(int(ids[20])) and m.lookup(int(ids[20])) == -1
    assert [m.lookup(int(i)) for i in ids[21:]] == list(range(21, 64))
    assert (m.entries, m.tombstones) == (63, 1)
    m.insert([int(ids[20])], 64)
    assert m.lookup(int(ids[20])) == 64 and (m.entries, m.tombstones) == (64, 0)
    assert int((m.keys != EMPTY).sum()) == used


# ---- the ABI: header == library == ctypes table, for the new entries ----------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    G.build()
    import optimized_rag_amd
    return optimized_rag_amd.load_library()


def test_new_entries_declared_exported_and_bound(lib):
    from optimized_rag_amd import _lib
    hdr = open(os.path.join(G.ROOT, "include", "rag_hip.h")).read()
    declared = set(re.findall(r"\b(rag_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/rag_hip.h"
        assert name in _lib.exported_symbols(), f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert "typedef struct rag_id_map_info" in hdr and "0x9E3779B97F4A7C15" in hdr
    assert ctypes.sizeof(_lib.IdMapInfo) == 2 * 4 + 6 * 8
    for method in ("index_id_map", "index_id_map_info", "rows_of_ids", "rows_of_ids_dev"):
        assert callable(getattr(_lib.RagEngine, method))


def test_new_entries_refuse_a_null_handle(lib):
    from optimized_rag_amd import _lib
    info = _lib.IdMapInfo()
    ids = np.zeros(4, dtype=np.int64)
    rows = np.zeros(4, dtype=np.int32)
    assert lib.rag_index_id_map(None, 1) != 0
    assert lib.rag_index_id_map_info(None, ctypes.byref(info)) != 0
    assert lib.rag_index_rows_of_ids_host(None, ids.ctypes.data, 4, rows.ctypes.data) != 0
    assert lib.rag_index_rows_of_ids_dev(None, None, 0, None, None) != 0
