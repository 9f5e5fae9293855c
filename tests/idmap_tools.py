"""numpy model of the device id-to-row map (include/rag_hip.h, "id-to-row map"; csrc/idmap.hip): the hash, linear probing,
tombstones and the rebuild rule, and a finder for ids that collide at a chosen home slot. Shared by tests/test_idmap_cpu.py and
tests/test_idmap_gpu.py. Which slot a key occupies may differ from the device's (that depends on the order of its atomics);
lookups, entries, tombstones, slots and rebuilds may not."""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
EMPTY = -(1 << 63)
MIN_SLOTS = 128


def home(ids, slots):
    """home(id) = ((uint64)id * 0x9E3779B97F4A7C15) >> (64 - log2(slots)); ids: int or array of ids >= 0."""
    lg = int(slots).bit_length() - 1
    assert slots == 1 << lg and lg >= 1
    with np.errstate(over="ignore"):
        return ((np.asarray(ids, dtype=np.int64).astype(np.uint64) * np.uint64(GOLDEN)) >> np.uint64(64 - lg)).astype(np.int64)


def slots_for(row_capacity):
    s = MIN_SLOTS
    while s < 2 * row_capacity:
        s <<= 1
    return s


def colliding_ids(slots, slot, count, below=1 << 26, exclude=()):
    """`count` distinct ids in [0, below) whose home slot is `slot`, ascending, none of them in `exclude`."""
    ids = np.arange(below, dtype=np.int64)
    hit = ids[home(ids, slots) == slot]
    if len(exclude):
        hit = hit[~np.isin(hit, np.asarray(exclude, dtype=np.int64))]
    assert len(hit) >= count, f"only {len(hit)} ids below {below} share home slot {slot} of {slots}"
    return hit[:count].copy()


class IdMapModel:
    """The table of one index: put / erase / lookup as the device does them, one key at a time."""

    def __init__(self, row_capacity):
        self.rebuilds = 0
        self._alloc(slots_for(row_capacity))

    def _alloc(self, slots):
        self.slots = slots
        self.keys = np.full(slots, EMPTY, dtype=np.int64)
        self.rows = np.full(slots, -1, dtype=np.int32)
        self.entries = self.tombstones = self.longest_probe = 0

    def _find(self, id_):
        s = int(home(id_, self.slots))
        for step in range(self.slots):
            k = int(self.keys[s])
            if k == id_:
                return s, step + 1
            if k == EMPTY:
                return -1 - s, step + 1          # the unused slot that ends the chain
            s = (s + 1) & (self.slots - 1)
        raise AssertionError("a full table: the load bound was broken")

    def lookup(self, id_):
        if id_ < 0:
            return -1
        s, _ = self._find(int(id_))
        return int(self.rows[s]) if s >= 0 else -1

    def _put(self, id_, row):
        assert id_ >= 0
        s, probe = self._find(int(id_))
        if s >= 0:
            assert self.rows[s] < 0, f"duplicate live id {id_}"
            self.tombstones -= 1
        else:
            s = -1 - s
            self.keys[s] = id_
        self.rows[s] = row
        self.entries += 1
        self.longest_probe = max(self.longest_probe, probe)

    def build(self, live_pairs, row_capacity=0, count=True):
        """A rebuild: an empty table (grown to the row capacity) filled with the (id, row) pairs of the live rows."""
        self._alloc(max(self.slots if row_capacity == 0 else slots_for(row_capacity), slots_for(len(live_pairs))))
        for id_, row in live_pairs:
            self._put(int(id_), int(row))
        self.rebuilds += 1 if count else 0

    def must_rebuild(self, n_new, row_capacity_after):
        return self.entries + self.tombstones + n_new > self.slots // 2 or slots_for(row_capacity_after) > self.slots

    def insert(self, ids, first_row):
        self.longest_probe = 0
        for i, id_ in enumerate(ids):
            self._put(int(id_), first_row + i)

    def erase(self, id_):
        s, _ = self._find(int(id_))
        if s >= 0 and self.rows[s] >= 0:
            self.rows[s] = -1
            self.entries -= 1
            self.tombstones += 1
            return True
        return False
