"""Tools of the doc-major sparse append tests (tests/test_sparse_docs_cpu.py, tests/test_sparse_append_dev_gpu.py).

`transpose` is a numpy mirror of the device transposition AS IMPLEMENTED in csrc/bm25.hip (rag_sparse_append_dev): the same digit
width, the same tile size, one stable counting pass per digit of the term number - per-tile digit counts, one exclusive scan over
(digit, tile), and a posting's rank among the earlier postings of its tile with the same digit. The CPU tests pin it to
LexicalPostings.from_weights; the GPU tests compare the library with a host append of the block it yields.
Nothing here touches the GPU at import."""
import numpy as np

import sparse_tools as S

BITS, TILE = 6, 2048                    # BM_TR_BITS, BM_TR_TILE


def passes(n_terms):
    """digit passes that order term numbers below n_terms (bm_tr_passes)"""
    n, m = 0, int(n_terms) - 1
    while m > 0:
        n, m = n + 1, m >> BITS
    return n


def counting_pass(key, shift):
    """destination of every posting under one stable pass over digit (key >> shift) & 63"""
    nnz = key.shape[0]
    n_tiles = (nnz + TILE - 1) // TILE
    digit = (key >> shift) & ((1 << BITS) - 1)
    cell = digit * n_tiles + np.arange(nnz, dtype=np.int64) // TILE          # digit-major, as tile_count is stored
    count = np.bincount(cell, minlength=(1 << BITS) * n_tiles)
    off = np.zeros(count.shape[0] + 1, dtype=np.int64)
    np.cumsum(count, out=off[1:])
    by_cell = np.argsort(cell, kind="stable")
    rank = np.empty(nnz, dtype=np.int64)
    rank[by_cell] = np.arange(nnz, dtype=np.int64) - off[cell[by_cell]]      # earlier postings of the same (digit, tile)
    return off[cell] + rank


def transpose(ptr, terms, weights, n_terms):
    """doc-major (ptr [n + 1], terms, weights) -> term-major (indptr int64 [n_terms + 1], doc int32, weight float32)"""
    ptr = np.asarray(ptr, dtype=np.int64)
    nnz = int(ptr[-1])
    key = np.asarray(terms[:nnz], dtype=np.int64)
    doc = np.repeat(np.arange(ptr.shape[0] - 1, dtype=np.int64), np.diff(ptr))
    w = np.asarray(weights[:nnz], dtype=np.float32)
    indptr = np.zeros(n_terms + 1, dtype=np.int64)
    np.cumsum(np.bincount(key, minlength=n_terms), out=indptr[1:])
    for p in range(passes(n_terms) if nnz else 0):
        dest = counting_pass(key, p * BITS)
        nk, nd, nw = np.empty_like(key), np.empty_like(doc), np.empty_like(w)
        nk[dest], nd[dest], nw[dest] = key, doc, w
        key, doc, w = nk, nd, nw
    return indptr, doc.astype(np.int32), np.ascontiguousarray(w)


def maps_of(ptr, terms, weights):
    """the {token id: weight} maps of a doc-major block"""
    return [{int(t): float(x) for t, x in zip(terms[a:e], weights[a:e])} for a, e in zip(ptr[:-1], ptr[1:])]


def doc_major_of_csr(indptr, doc, w, n_docs):
    """term-major CSR -> the doc-major block of the same postings"""
    term = np.repeat(np.arange(indptr.shape[0] - 1, dtype=np.int64), np.diff(indptr))
    order = np.lexsort((term, doc))
    ptr = np.zeros(n_docs + 1, dtype=np.int64)
    np.cumsum(np.bincount(doc, minlength=n_docs), out=ptr[1:])
    return ptr.astype(np.int32), term[order].astype(np.int32), np.ascontiguousarray(w[order], dtype=np.float32)


def block_of(docs, n_docs):
    """doc-major block from a list of (document, terms ascending) with seeded weights: [(d, [t, ...]), ...] -> (ptr, terms, weights)"""
    rng = np.random.default_rng(29)
    per = np.zeros(n_docs, dtype=np.int64)
    terms = []
    for d, ts in docs:
        per[d] = len(ts)
        terms.extend(ts)
    ptr = np.zeros(n_docs + 1, dtype=np.int32)
    ptr[1:] = np.cumsum(per)
    w = (rng.random(len(terms)) * 2.0).astype(np.float32) + np.float32(1e-3)
    return ptr, np.asarray(terms, dtype=np.int32), w


V_EDGE, V_BIG, N_LONG = 5000, 250_002, 2100
DIGIT_TERMS = [0, 63, 64, 4095, 4096, V_EDGE - 1]


def edge_blocks():
    """name -> (ptr, terms, weights, n_terms_total): the blocks the issue lists, each over the vocabulary it names"""
    rng = np.random.default_rng(5)
    some = lambda: sorted(rng.choice(V_EDGE, int(rng.integers(1, 30)), replace=False).tolist())
    out = {}
    out["empty documents first"] = block_of([(d, some()) for d in range(3, 9)], 9) + (V_EDGE,)
    out["empty documents in the middle"] = block_of([(d, some()) for d in (0, 1, 5, 6)], 7) + (V_EDGE,)
    out["empty documents last"] = block_of([(d, some()) for d in range(4)], 8) + (V_EDGE,)
    out["every document empty"] = block_of([], 5) + (V_EDGE,)
    out["one document with one term"] = block_of([(0, [17])], 1) + (V_EDGE,)
    # one term in every document of a 2,100-row block (a list longer than a tile) beside ordinary terms; 2,100 + ... postings
    long_docs = [(d, sorted(set([77] + rng.choice(V_EDGE, 3, replace=False).tolist()))) for d in range(N_LONG)]
    out["one term in every document"] = block_of(long_docs, N_LONG) + (V_EDGE,)
    out["the digit boundaries"] = block_of([(0, DIGIT_TERMS), (1, DIGIT_TERMS[1:4]), (2, []), (3, DIGIT_TERMS[::2])], 4) + (V_EDGE,)
    out["a term past the known vocabulary"] = block_of([(0, [5, V_EDGE]), (1, [V_EDGE + 70])], 2) + (V_EDGE + 71,)
    few = [(d, sorted(rng.choice(V_BIG, 3, replace=False).tolist() + ([V_BIG - 1] if d % 50 == 0 else []))) for d in range(120)]
    out["a vocabulary of 250,002"] = block_of(few, 120) + (V_BIG,)
    out["65,535 documents of one term each"] = block_of([(d, [int(t)]) for d, t in enumerate(rng.integers(0, V_EDGE, 65535))], 65535) + (V_EDGE,)
    assert int(out["one term in every document"][0][-1]) % TILE != 0 and int(out["65,535 documents of one term each"][0][-1]) % TILE != 0
    return out


# ---- the world of the append tests: test_sparse_live_gpu.py's shapes over a vocabulary of 5,000 -------------------------------
N0, BLOCKS, DIM = 3000, (1, 700, 2100), 32       # the base ends inside a 2048-document range; the tail crosses a range boundary
N_ALL = N0 + sum(BLOCKS)                         # and ends on a partial range
V0, V = 4500, 5000                               # the base's vocabulary and the vocabulary after the second block
T_TAIL, T_NEW = 4200, 4600                       # a known term only appended rows hold / a term past the base's vocabulary


def csr_of(term, doc, w, n_terms, n_docs):
    order = np.argsort(term * max(n_docs, 1) + doc, kind="stable")
    indptr = np.zeros(n_terms + 1, dtype=np.int64)
    np.cumsum(np.bincount(term, minlength=n_terms), out=indptr[1:])
    return indptr, doc[order].astype(np.int32), np.ascontiguousarray(w[order], dtype=np.float32)


_W = {}


def world():
    """Seeded postings of N_ALL documents over V terms (sparse_tools.make_corpus: terms below V - 1000) plus, in appended rows
    only, T_TAIL, T_NEW and the terms 4095, 4096 and V - 1; queries, embeddings, ids and tenants. Built once, read-only."""
    if _W:
        return _W
    rng = np.random.default_rng(3)
    ip, doc, w = S.make_corpus(N_ALL, V, seed=7)
    term = np.repeat(np.arange(V, dtype=np.int64), np.diff(ip))
    xt = np.array([T_TAIL] * 4 + [T_NEW] * 3 + [4095, 4096, V - 1, V - 1], dtype=np.int64)
    xd = np.array([N0 + 5, N0 + 300, N0 + 900, N_ALL - 1, N0 + 5, N0 + 2000, N_ALL - 2, N0 + 701, N0 + 701, N0 + 702, N_ALL - 1], dtype=np.int64)
    xw = np.array([0.5, 1.25, 0.75, 2.0, 1.5, 0.25, 1.0, 0.5, 0.75, 1.0, 1.25], dtype=np.float32)
    term, doc, w = np.concatenate([term, xt]), np.concatenate([doc.astype(np.int64), xd]), np.concatenate([w, xw]).astype(np.float32)
    full = csr_of(term, doc, w, V, N_ALL)
    qs = S.make_queries(full[0])
    one = np.float32(1.0)
    qs += [(np.array([T_TAIL]), np.array([one])), (np.array([T_NEW]), np.array([0.5], np.float32)),
           (np.array([4095, 4096, V - 1, 0, 63, 64]), np.array([1.0, 0.5, 0.25, 1.0, 0.5, 2.0], np.float32))]
    emb = rng.standard_normal((N_ALL, DIM)).astype(np.float32)
    _W.update(coo=(term, doc, w), full=full, qs=qs, packed=S.pack_queries(qs), emb=emb,
              q=(emb[rng.integers(0, N_ALL, len(qs))] + 0.3 * rng.standard_normal((len(qs), DIM))).astype(np.float32),
              ids=(rng.permutation(N_ALL) + 1_000_000).astype(np.int64), ten=rng.integers(0, 3, N_ALL).astype(np.int32),
              cand=rng.integers(-1, N_ALL + 3, (len(qs), 16)).astype(np.int32))
    for v in _W.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _W


def postings_of(w, orig, n_terms):
    """term-major CSR of the world's documents `orig` (ascending), renumbered 0 .. len(orig) - 1, over n_terms terms"""
    term, doc, wt = w["coo"]
    inv = np.full(N_ALL, -1, dtype=np.int64)
    inv[orig] = np.arange(len(orig))
    keep = (inv[doc] >= 0) & (term < n_terms)
    return csr_of(term[keep], inv[doc[keep]], wt[keep], n_terms, len(orig))
