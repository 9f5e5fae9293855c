"""Seeded token-vector stores and the numpy mirror of their compaction (rag_index_compact_live; tests/test_tokvec_compact_*.py).

The mirror runs the device's algorithm on host arrays: a per-document map (new offsets, first old row), destination chunks in
ascending order, each gathered into a staging array by a search over the chunk's documents and then copied onto the store IN
PLACE. `rebuilt` is the independent reference: the surviving documents' rows concatenated. Nothing here touches the GPU."""
import numpy as np

LENS = (0, 1, 15, 16, 17, 33, 255, 257)
N_DOCS = 40
ONE, LONG = 11, 12                           # a 1-row document directly in front of a 255-row one: deleting it moves 255 rows down by one
ZERO = 20                                    # a document without rows


def make_store(dim, seed=1, n_docs=N_DOCS):
    """(vecs float32 [rows, dim] of fp16-representable unit-ish rows, offsets int64 [n_docs + 1])"""
    rng = np.random.default_rng(seed)
    lens = rng.choice(np.asarray(LENS), n_docs)
    lens[1:1 + len(LENS)] = rng.permutation(np.asarray(LENS))    # every length occurs
    lens[ONE], lens[LONG], lens[ZERO] = 1, 255, 0
    lens[0], lens[n_docs - 1] = 17, 33                           # the first and the last document have rows
    off = np.zeros(n_docs + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    v = rng.standard_normal((int(off[-1]), dim))
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    return v.astype(np.float16).astype(np.float32), off


def keep_of(n_store_docs, row_map):
    """bool per stored document: documents below the index rows follow the row map, the ones past it stay"""
    n_map = min(n_store_docs, len(row_map))
    keep = np.ones(n_store_docs, dtype=bool)
    keep[:n_map] = np.asarray(row_map[:n_map]) >= 0
    return keep


def rebuilt(bits, off, row_map):
    """(bits, offsets) of the surviving documents, concatenated in order"""
    keep = keep_of(len(off) - 1, row_map)
    parts = [bits[off[d]:off[d + 1]] for d in np.nonzero(keep)[0]]
    new_off = np.zeros(int(keep.sum()) + 1, dtype=np.int64)
    np.cumsum(np.diff(off)[keep], out=new_off[1:])
    return (np.concatenate(parts) if parts else bits[:0]), new_off


def compact_in_place(bits, off, row_map, chunk_rows):
    """The device's move on `bits` (uint16 [rows, dim], MODIFIED in place); returns (new offsets, rows after)."""
    keep = keep_of(len(off) - 1, row_map)
    src_start = off[:-1][keep]
    new_off = np.zeros(int(keep.sum()) + 1, dtype=np.int64)
    np.cumsum(np.diff(off)[keep], out=new_off[1:])
    docs_new, rows_new = len(src_start), int(new_off[-1])
    if keep.all():
        return new_off, rows_new
    first = int(np.argmin(keep))                                  # documents before it do not move
    for r0 in range(int(new_off[first]), rows_new, chunk_rows):
        m = min(chunk_rows, rows_new - r0)
        R = np.arange(r0, r0 + m)
        d = np.searchsorted(new_off[:docs_new + 1], R, side="right") - 1      # the LAST document that starts at or before the row
        stage = bits[src_start[d] + (R - new_off[d])].copy()
        assert (src_start[d] + (R - new_off[d]) >= R).all()       # every source lies at or above its destination
        bits[r0:r0 + m] = stage
    return new_off, rows_new
