"""CPU: the numpy mirror of the token-vector store's compaction (tests/tokvec_compact_tools.py) - new offsets and the fp16
bits after the chunked in-place move - against the surviving documents concatenated, on the document lengths of the GPU test."""
import numpy as np
import pytest

import tokvec_compact_tools as C

DELETES = {
    "the first document": [0],
    "the last document": [C.N_DOCS - 1],
    "a run of adjacent documents": list(range(5, 10)),
    "a 0-row document": [C.ZERO],
    "a 1-row document in front of a 255-row one": [C.ONE],
    "several": [0, 3, C.ONE, 14, 15, C.ZERO, 31, C.N_DOCS - 1],
    "every document": list(range(C.N_DOCS)),
    "nothing": [],
}


def row_map_of(n, deleted):
    live = np.ones(n, dtype=bool)
    live[deleted] = False
    return np.where(live, np.cumsum(live) - 1, -1)


@pytest.mark.parametrize("chunk", [1, 64, 1 << 20])
@pytest.mark.parametrize("name", list(DELETES))
def test_in_place_move_equals_the_concatenation(name, chunk):
    vecs, off = C.make_store(32)
    assert set(np.diff(off).tolist()) == set(C.LENS) and off[C.LONG + 1] - off[C.LONG] == 255 and off[C.ONE + 1] - off[C.ONE] == 1
    bits = vecs.astype(np.float16).view(np.uint16)
    rm = row_map_of(C.N_DOCS, DELETES[name])
    want_bits, want_off = C.rebuilt(bits.copy(), off, rm)
    work = bits.copy()
    new_off, rows = C.compact_in_place(work, off, rm, chunk)
    np.testing.assert_array_equal(new_off, want_off)
    assert rows == want_bits.shape[0] == int(np.diff(off)[rm >= 0].sum())
    np.testing.assert_array_equal(work[:rows], want_bits)


@pytest.mark.parametrize("n_index", [30, 50])
def test_a_store_ahead_of_or_behind_the_index(n_index):
    """documents the store holds past the index rows follow the survivors; rows past the store's documents do not concern it"""
    vecs, off = C.make_store(32)
    bits = vecs.astype(np.float16).view(np.uint16)
    rm = row_map_of(n_index, [2, C.ONE, 29])
    keep = C.keep_of(C.N_DOCS, rm)
    assert keep.sum() == C.N_DOCS - 3 and keep[min(n_index, C.N_DOCS):].all()
    want_bits, want_off = C.rebuilt(bits.copy(), off, rm)
    work = bits.copy()
    new_off, rows = C.compact_in_place(work, off, rm, 64)
    np.testing.assert_array_equal(new_off, want_off)
    np.testing.assert_array_equal(work[:rows], want_bits)
