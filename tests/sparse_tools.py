"""Float64 reference and seeded corpora of the learned-sparse index tests (tests/test_sparse_*.py).

The reference IS the contract of include/rag_hip.h (rag_sparse_*): token by token, in the query's order,
`score[doc[a:e]] += float64(qw) * w[a:e].astype(float64)`; a term outside [0, V) or a weight that is not > 0 adds nothing;
the top-k is a stable order (score descending, row ascending) over the visible documents with score > 0.
Nothing here touches the GPU or the package under test."""
import numpy as np

N_FULL, V_FULL = 75_001, 30_000          # 36 full 2048-document ranges + a short tail
N_EMPTY = 1_000                          # the last terms of the vocabulary get no posting at all


def make_corpus(n_docs=N_FULL, n_terms=V_FULL, seed=7, weight_values=None):
    """Term-major CSR (indptr int64, doc int32, weight float32). Each document gets 8-24 terms drawn with probability
    proportional to rank^-1.1 from the first n_terms - N_EMPTY terms, deduplicated; weights float32 U(0, 2) + 1e-3, or drawn
    from `weight_values` (the tie corpus)."""
    rng = np.random.default_rng(seed)
    live = max(1, n_terms - N_EMPTY)
    p = np.arange(1, live + 1, dtype=np.float64) ** -1.1
    p /= p.sum()
    per_doc = rng.integers(8, 25, n_docs)
    owner = np.repeat(np.arange(n_docs, dtype=np.int64), per_doc)
    term = rng.choice(live, size=owner.shape[0], p=p).astype(np.int64)
    key = np.unique(term * n_docs + owner)                       # sorted: term-major, documents ascending, duplicates gone
    term, doc = key // n_docs, (key % n_docs).astype(np.int32)
    if weight_values is None:
        w = (rng.random(key.shape[0]) * 2.0).astype(np.float32) + np.float32(1e-3)
    else:
        w = rng.choice(np.asarray(weight_values, dtype=np.float32), size=key.shape[0])
    indptr = np.zeros(n_terms + 1, dtype=np.int64)
    np.cumsum(np.bincount(term, minlength=n_terms), out=indptr[1:])
    return indptr, doc, w.astype(np.float32)


def cut(indptr, doc, w, n_docs):
    """The postings of the documents [0, n_docs) of a corpus."""
    keep = doc < n_docs
    term_of = np.repeat(np.arange(indptr.shape[0] - 1, dtype=np.int64), np.diff(indptr))
    out = np.zeros_like(indptr)
    np.cumsum(np.bincount(term_of[keep], minlength=indptr.shape[0] - 1), out=out[1:])
    return out, doc[keep].copy(), w[keep].copy()


def pack_queries(queries):
    """[(terms, weights), ...] -> (term_ptr int32, terms int32, weights float32), order kept."""
    ptr = np.zeros(len(queries) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(t) for t, _ in queries])
    terms = np.concatenate([np.asarray(t, dtype=np.int32) for t, _ in queries]) if ptr[-1] else np.zeros(0, np.int32)
    wts = np.concatenate([np.asarray(w, dtype=np.float32) for _, w in queries]) if ptr[-1] else np.zeros(0, np.float32)
    return ptr, terms, wts


def make_queries(indptr, seed=11, weight_values=None):
    """32 queries over a make_corpus index: a 70-term query (past the 64 planned slots), 9 over the 200 most frequent terms,
    14 of 1-12 Zipf-drawn terms, and the eight edge cases named in the comments."""
    rng = np.random.default_rng(seed)
    V = indptr.shape[0] - 1
    df = np.diff(indptr)
    by_df = np.argsort(-df, kind="stable")
    live = V - N_EMPTY
    p = np.arange(1, live + 1, dtype=np.float64) ** -1.1
    p /= p.sum()

    def wts(n):
        if weight_values is None:
            return (rng.random(n) * 2.0).astype(np.float32) + np.float32(1e-3)
        return rng.choice(np.asarray(weight_values, dtype=np.float32), size=n)

    qs = [(rng.choice(live, 70, replace=False, p=p), wts(70))]
    for _ in range(9):
        n = int(rng.integers(2, 7))
        qs.append((rng.choice(by_df[:200], n, replace=False), wts(n)))
    for _ in range(14):
        n = int(rng.integers(1, 13))
        qs.append((rng.choice(live, n, replace=False, p=p), wts(n)))
    rare = np.nonzero((df >= 1) & (df <= 3))[0]
    qs.append((rare[:4], wts(4)))                                            # fewer than k matches
    qs.append((np.zeros(0, np.int32), np.zeros(0, np.float32)))              # empty query
    qs.append((np.array([-1, V, V + 5, -7]), wts(4)))                        # only terms outside the vocabulary
    qs.append((np.array([V - 1]), wts(1)))                                   # a term with an empty list
    t = int(by_df[50])
    qs.append((np.array([t, int(by_df[300]), t]), wts(3)))                   # a repeated term adds twice
    qs.append((by_df[[10, 400, 20, 900]], np.array([0.0, 1.25, np.nan, 0.5], dtype=np.float32)))   # zero and NaN weights add nothing
    qs.append((by_df[[0, 1, 2]], wts(3)))                                    # the three longest lists
    qs.append((np.array([int(by_df[5]), -1, int(rare[7]), V + 1, int(by_df[150])]), wts(5)))       # known and unknown mixed
    assert len(qs) == 32
    return qs


def scores(indptr, doc, w, n_docs, terms, weights):
    """One query's float64 score of every document."""
    s = np.zeros(n_docs, dtype=np.float64)
    V = indptr.shape[0] - 1
    for t, qw in zip(terms, weights):
        if t < 0 or t >= V or not (qw > 0):
            continue
        a, e = int(indptr[t]), int(indptr[t + 1])
        s[doc[a:e]] += np.float64(qw) * w[a:e].astype(np.float64)            # documents are unique inside a list
    return s


def all_scores(indptr, doc, w, n_docs, queries):
    return np.stack([scores(indptr, doc, w, n_docs, t, qw) for t, qw in queries])


def topk(s, k, hidden=None):
    """Stable top-k of one score row: (rows int32 [k], scores float64 [k]), -1 / 0.0 behind the matches."""
    ok = s > 0
    if hidden is not None:
        ok &= ~hidden
    cand = np.nonzero(ok)[0]
    order = cand[np.lexsort((cand, -s[cand]))][:k]
    rows = np.full(k, -1, dtype=np.int32)
    sc = np.zeros(k, dtype=np.float64)
    rows[:order.shape[0]] = order
    sc[:order.shape[0]] = s[order]
    return rows, sc


def topk_all(S, k, hidden=None):
    r = [topk(s, k, hidden) for s in S]
    return np.stack([x[0] for x in r]), np.stack([x[1] for x in r])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
