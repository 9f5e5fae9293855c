"""A plain numpy model of one handle's resident bge-m3 state - dense rows, learned-sparse postings, token-vector store - through
live writes, the drawn worlds of the three properties of tests/test_m3_property_gpu.py, and the classes their examples must
reach (counted by tests/test_m3_property_cases_cpu.py). Nothing here touches the GPU or the package under test.

The model keeps, per index row, the document behind it (float32 embedding, id, tenant, {term: float32 weight} as two sorted
arrays, float32 token vectors) and a deleted flag, and three counters: index rows, rows the sparse postings cover (base | tail),
documents the token-vector store holds. The store may run AHEAD of the index (its extra documents are the next documents of
the world, in order) or BEHIND it. The rules are those of include/rag_hip.h:
  insert           new rows; the postings and the store are behind until appends cover them
  sparse_append    the next rows' postings into the tail (never past the index rows)
  tokvec_append    the next documents' vectors (inside the reservation)
  delete           hides rows; stales nothing
  fold             tail -> base
  compact_live     live rows move down in order; the covered rows of the postings and the store's documents below the index rows
                   follow the row map, the store's documents past the index rows stay behind the survivors; base | tail become
                   their live parts, one segment when either is empty
The store is current when it holds exactly the index rows. The postings follow the header's flag: an insert marks them stale, the
append after which they cover every row clears it, a compaction leaves it as it was - so postings whose uncovered rows were
deleted and compacted away cover every row and are stale all the same (nothing is left to append: only a reload helps); the
model reports that state as the handle does. The references are the existing ones: sparse_tools.scores / topk,
m3_fused_tools.point_scores / combine, tokvec_tools.pair_scores / stable_topk."""
import os

import numpy as np
from hypothesis import HealthCheck, seed, settings
from hypothesis import strategies as st

import m3_fused_tools as F
import m3_tools as M
import sparse_tools as S
import tokvec_tools as V

N_EX = int(os.environ.get("RAG_PROPERTY_EXAMPLES", "300"))          # raise for an exploratory run
EXPLORE = "RAG_PROPERTY_EXAMPLES" in os.environ
# the pattern of tests/test_property_gpu.py: the default run is derandomized, RAG_PROPERTY_EXAMPLES explores
COMMON = dict(deadline=None, max_examples=N_EX, derandomize=not EXPLORE, database=None,
              suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large, HealthCheck.filter_too_much])
# default example counts, as fractions of N_EX; P3 runs as two functions by start size
COUNTS = dict(p1=max(20, N_EX // 5), p2=max(16, N_EX // 3), p3_small=max(12, N_EX // 12), p3_large=max(6, N_EX // 40))
_SEEDS = dict(p1=1, p2=5, p3_small=6, p3_large=1)


def prop(name):
    """settings of one property. The default run pins the generator's seed, so that the CPU module counts the classes over exactly
    the examples the GPU module runs; an exploring run draws fresh ones."""
    s = settings(**{**COMMON, "max_examples": COUNTS[name]})
    if EXPLORE:
        return s
    return lambda f: seed(_SEEDS[name])(s(f))


# ---- P1: MaxSim worlds ------------------------------------------------------------------------------------------------------------
FAMILIES = ("gaussian", "one sign", "negated", "subnormal", "pow2")


@st.composite
def maxsim_cases(draw):
    """row counts come from the generator; the family and the class of the dim (32 = one K-step, a power of two, any multiple of
    32) from a numpy generator over the drawn seed, which keeps the five families and three dim classes equally likely"""
    seed_ = draw(st.integers(0, 2**31 - 1))
    q_count = st.one_of(st.integers(0, 1), st.integers(1, 32), st.integers(33, 70))
    d_count = st.one_of(st.just(0), st.integers(1, 16), st.integers(17, 128), st.integers(129, 300))
    q_counts, d_counts = draw(st.lists(q_count, min_size=1, max_size=4)), draw(st.lists(d_count, min_size=1, max_size=6))
    rng = np.random.default_rng([seed_, 1] + q_counts + d_counts)        # (the generator repeats a seed while it varies the rest)
    dim = int([32, rng.choice([64, 128, 256, 512, 1024]), 32 * rng.integers(1, 33)][int(rng.integers(0, 3))])
    return dict(seed=seed_, dim=dim, family=FAMILIES[int(rng.integers(0, len(FAMILIES)))], q_counts=q_counts, d_counts=d_counts,
                k=draw(st.integers(1, 8)))


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def family_rows(rng, family, n_q, n_d, dim):
    """(query rows [n_q, dim], document rows [n_d, dim]) float32 of one family; unit rows but for the power-of-two family"""
    if family == "gaussian":
        return V.unit_rows(rng, n_q, dim), V.unit_rows(rng, n_d, dim)
    if family == "one sign":                     # every product of every dot is positive: the fp32 accumulation never cancels
        s = rng.choice([-1.0, 1.0], dim)
        return _unit(s * (1.0 + 0.1 * rng.random((n_q, dim)))), _unit(s * (1.0 + 0.1 * rng.random((n_d, dim))))
    if family == "negated":                      # every similarity < -0.5: a zero-filled tile tail or a pad row would win the maximum
        u = M.normalize(rng.standard_normal((1, dim)))
        noise = 0.05 / np.sqrt(dim / 32.0)
        return _unit(u + noise * rng.standard_normal((n_q, dim))), _unit(-u + noise * rng.standard_normal((n_d, dim)))
    if family == "subnormal":                    # a few components of normal size, the rest below 2^-14: fp16 subnormals once split or stored

        def rows(n):
            a = rng.uniform(-1.0, 1.0, (n, dim)) * 2.0 ** -16
            for r in range(n):
                cols = rng.choice(dim, 4, replace=False)
                a[r, cols] = rng.standard_normal(4) + np.sign(rng.standard_normal(4))
            return _unit(a) if n else a.astype(np.float32)
        return rows(n_q), rows(n_d)

    def rows(n):                                 # {0, +-2^-k}: exact as fp16; every product and sum exact in float32 and float64 alike
        a = np.zeros((n, dim), dtype=np.float32)
        for r in range(n):
            cols = rng.choice(dim, 4, replace=False)
            a[r, cols] = rng.choice([-1.0, 1.0], 4) * 2.0 ** -rng.integers(1, 6, 4)
        return a
    return rows(n_q), rows(n_d)


def build_maxsim(case):
    rng = np.random.default_rng(case["seed"])
    q_off = np.concatenate([[0], np.cumsum(case["q_counts"])]).astype(np.int64)
    d_off = np.concatenate([[0], np.cumsum(case["d_counts"])]).astype(np.int64)
    q, d = family_rows(rng, case["family"], int(q_off[-1]), int(d_off[-1]), case["dim"])
    return dict(q=np.ascontiguousarray(q), q_off=q_off, d=np.ascontiguousarray(d), d_off=d_off, rng=rng)


def maxsim_classes(case):
    tiles = [(c + 15) // 16 for c in case["d_counts"]]
    dim = case["dim"]
    return {"document tiles: 0": 0 in tiles, "document tiles: 1": 1 in tiles, "document tiles: 2-8": any(2 <= t <= 8 for t in tiles),
            "document tiles: > 8": any(t > 8 for t in tiles), "partial last tile": any(c % 16 for c in case["d_counts"]),
            "query of more than 32 rows": any(c > 32 for c in case["q_counts"]), "dim 32": dim == 32,
            "dim not a power of two": dim & (dim - 1) != 0,
            "all-negative pair": case["family"] == "negated" and any(case["q_counts"]) and any(case["d_counts"])}


# ---- weights shared by P2 and P3 -----------------------------------------------------------------------------------------------
WEIGHT_FAMILIES = ("uniform", "four values", "wide")
FOUR = np.array([0.25, 0.5, 1.0, 1.5], dtype=np.float32)


def draw_weights(rng, n, family):
    """finite float32 weights > 0: U(0, 2) (+ 1e-3, as sparse_tools.make_corpus keeps them off zero); four distinct values; or
    2^U(-120, 120) with a float32 subnormal and a value near FLT_MAX among them (a float64 sum of 300 products stays below 1e80)"""
    if family == "uniform":
        return (rng.random(n) * 2.0).astype(np.float32) + np.float32(1e-3)
    if family == "four values":
        return rng.choice(FOUR, size=n)
    w = (2.0 ** rng.uniform(-120.0, 120.0, n)).astype(np.float32)
    if n >= 4:
        at = rng.choice(n, 2, replace=False)
        w[at[0]], w[at[1]] = np.float32(2.0 ** -140), np.float32(3.0e38)
    return w


def csr_of(term, doc, w, n_terms, n_docs):
    """term-major CSR of COO postings (documents ascending per term)"""
    term, doc = np.asarray(term, dtype=np.int64), np.asarray(doc, dtype=np.int64)
    order = np.argsort(term * max(n_docs, 1) + doc, kind="stable")
    indptr = np.zeros(n_terms + 1, dtype=np.int64)
    np.cumsum(np.bincount(term, minlength=n_terms), out=indptr[1:])
    return indptr, doc[order].astype(np.int32), np.ascontiguousarray(np.asarray(w, dtype=np.float32)[order])


def draw_queries(rng, n_terms, lengths, family, common):
    """weighted queries over [0, n_terms): terms from `common` (frequent terms) and the whole vocabulary, one repeated term, terms
    outside the vocabulary, and a zero, a negative and a NaN weight once the query is long enough"""
    qs = []
    for n in lengths:
        terms = np.where(rng.random(n) < 0.5, rng.choice(common, n), rng.integers(0, n_terms, n)).astype(np.int64) if n else np.zeros(0, np.int64)
        w = draw_weights(rng, n, family)
        if n >= 2:
            terms[n - 1] = terms[0]                                      # a repeated term adds twice
        if n >= 4:
            terms[1] = [-1, n_terms, n_terms + 5][int(rng.integers(0, 3))]
        if n >= 6:
            w[2], w[3], w[4] = 0.0, -1.0, np.nan
        qs.append((terms, w))
    return qs


# ---- P2: sparse corpora ---------------------------------------------------------------------------------------------------------
@st.composite
def sparse_cases(draw):
    """the generator favours small and repeated values, so what the size classes hang on - the number of documents, the cut points
    of the appended form, a small or a wide k - comes from a numpy generator over the drawn values: fifteen equally likely slots, two for each
    of the five sizes where a range, or the corpus, ends exactly, one for each span around them and two for the largest span"""
    seed_ = draw(st.integers(0, 2**31 - 1))
    q_len = st.one_of(st.integers(0, 12), st.integers(65, 120), st.integers(257, 300))
    case = dict(seed=seed_, n_terms=draw(st.integers(3, 400)), n_all=draw(st.integers(0, 3)), n_none=draw(st.integers(0, 3)),
                per_doc=draw(st.integers(0, 27)), family=draw(st.sampled_from(WEIGHT_FAMILIES)), q_family=draw(st.sampled_from(WEIGHT_FAMILIES)),
                q_lens=draw(st.lists(q_len, min_size=2, max_size=4)), plan_slots=draw(st.sampled_from([0, 8])), with_index=draw(st.booleans()))
    # (the generator repeats a seed while it varies the rest: everything drawn goes into the numpy generator's seed)
    rng = np.random.default_rng([seed_, 1, case["n_terms"], case["n_all"], case["n_none"], case["per_doc"], case["plan_slots"]] + case["q_lens"])
    n_docs = int(([1, 2047, 2048, 2049, 4096] * 2 + [rng.integers(1, 301), rng.integers(2040, 2061), rng.integers(4090, 4101),
                                                     rng.integers(6000, 9001), rng.integers(6000, 9001)])[int(rng.integers(0, 15))])
    cuts = [int(c) if c < n_docs and rng.random() < 0.5 else float(rng.random()) for c in (2048, 4096)[:int(rng.integers(1, 3))]]
    k = int(rng.integers(1, 13)) if rng.random() < 0.5 else int(rng.integers(1, 1025))
    return dict(case, n_docs=n_docs, cuts=cuts, k=k)


def build_sparse(case):
    """the corpus (CSR), its queries, the cut points of the appended form and the float64 reference scores"""
    rng = np.random.default_rng(case["seed"])
    n, V_ = case["n_docs"], case["n_terms"]
    n_all = min(case["n_all"], V_ - 1)
    n_none = min(case["n_none"], V_ - 1 - n_all)
    perm = rng.permutation(V_)
    all_terms, none_terms, free = perm[:n_all], perm[n_all:n_all + n_none], perm[n_all + n_none:]
    per = rng.integers(0, min(case["per_doc"], len(free)) + 1, n)          # 0 .. per_doc picks per document, duplicates dropped
    picks = free[rng.integers(0, len(free), (n, max(int(per.max()), 1)))]
    use = np.arange(picks.shape[1])[None, :] < per[:, None]
    doc = np.broadcast_to(np.arange(n)[:, None], picks.shape)[use]
    key = np.unique(picks[use].astype(np.int64) * n + doc)
    term, doc = key // n, key % n
    term = np.concatenate([term, np.repeat(all_terms.astype(np.int64), n)])
    doc = np.concatenate([doc, np.tile(np.arange(n), n_all)])
    indptr, doc, w = csr_of(term, doc, draw_weights(rng, term.shape[0], case["family"]), V_, n)
    common = np.concatenate([all_terms, none_terms, free[:8]])
    q_lens = list(case["q_lens"])
    q_lens[0] = max(q_lens[0], 1)                                         # (a call whose queries hold no token at all has nothing to point at)
    queries = draw_queries(rng, V_, q_lens, case["q_family"], common)
    cuts = sorted({min(max(1, c if isinstance(c, int) else int(c * n)), n - 1) for c in case["cuts"]}) if n >= 2 else []
    ref = S.all_scores(indptr, doc, w, n, queries)
    return dict(indptr=indptr, doc=doc, w=w, n_docs=n, n_terms=V_, all_terms=all_terms, none_terms=none_terms, queries=queries,
                packed=S.pack_queries(queries), cuts=cuts, ref=ref, rng=rng)


def rows_span(indptr, doc, w, lo, hi):
    """the CSR of the documents [lo, hi), renumbered from 0: one block of rag_sparse_append_host"""
    term_of = np.repeat(np.arange(indptr.shape[0] - 1, dtype=np.int64), np.diff(indptr))
    sel = (doc >= lo) & (doc < hi)
    out = np.zeros_like(indptr)
    np.cumsum(np.bincount(term_of[sel], minlength=indptr.shape[0] - 1), out=out[1:])
    return out, (doc[sel] - lo).astype(np.int32), np.ascontiguousarray(w[sel])


def sparse_classes(case, b):
    n, k = b["n_docs"], case["k"]
    toks = [(t, w) for t, w in b["queries"]]
    flat_t = np.concatenate([t for t, _ in toks]) if toks else np.zeros(0, np.int64)
    flat_w = np.concatenate([w for _, w in toks]) if toks else np.zeros(0, np.float32)
    tie = False
    for s in b["ref"]:
        top = np.sort(s[s > 0])[::-1]
        tie |= bool(top.shape[0] > k and top[k - 1] == top[k])
    live = (flat_w > 0) & (flat_t >= 0) & (flat_t < b["n_terms"])
    out = {f"n_docs == {v}": n == v for v in (1, 2047, 2048, 2049, 4096)}
    out.update({"n_docs > 4096": n > 4096, "a queried term held by every document": bool(np.isin(flat_t[live], b["all_terms"]).any()),
                "a queried term held by none": bool(np.isin(flat_t[live], b["none_terms"]).any()),
                "query of more than 64 tokens": any(len(t) > 64 for t, _ in toks), "query of more than 256 tokens": any(len(t) > 256 for t, _ in toks),
                "repeated term": any(len(t) >= 2 for t, _ in toks), "out-of-vocabulary term": bool(((flat_t < 0) | (flat_t >= b["n_terms"])).any()),
                "zero / negative / NaN query weight": bool((flat_w == 0).any() and (flat_w < 0).any() and np.isnan(flat_w).any()),
                "exact tie across k": tie, "cut on a 2048 boundary": any(c % 2048 == 0 for c in b["cuts"]),
                "cut off a 2048 boundary": any(c % 2048 for c in b["cuts"])})
    return out


# ---- P3: the model ------------------------------------------------------------------------------------------------------------------
class Doc:
    __slots__ = ("emb", "id", "tenant", "terms", "w", "vecs", "stored")


class World:
    """the documents a handle may ever see, in insertion order, generated in blocks of 64 from (seed, block)"""

    def __init__(self, seed_, n0, tok_dim, v0, v_max, family, per_doc, rows_max, emb_dim=32):
        self.seed, self.n0, self.tok_dim, self.v0, self.v_max, self.family = seed_, n0, tok_dim, v0, v_max, family
        self.per_doc, self.rows_max, self.emb_dim, self._docs = per_doc, rows_max, emb_dim, []

    def doc(self, i):
        while i >= len(self._docs):
            self._block(len(self._docs) // 64)
        return self._docs[i]

    def _block(self, b):
        rng = np.random.default_rng([self.seed, b])
        counts = np.where(rng.random(64) < 0.25, 0, rng.integers(0, self.rows_max + 1, 64))      # a quarter of the documents without rows
        for j in range(64):
            i, d = b * 64 + j, Doc()
            d.emb = rng.standard_normal(self.emb_dim).astype(np.float32)
            if i % 41 == 3:
                d.emb[:] = 0.0                                           # a zero embedding: cosine 0.0, never NaN
            d.id, d.tenant = 1_000_000 + 7 * i + int(rng.integers(0, 7)), int(rng.integers(0, 3))
            vocab = self.v0 if i < self.n0 else self.v_max               # documents behind the start may hold terms past its vocabulary
            d.terms = np.unique(rng.integers(0, vocab, int(rng.integers(0, self.per_doc + 1)))).astype(np.int64)
            if i % 3 == 0:
                d.terms = np.union1d(d.terms, [0]).astype(np.int64)      # term 0 is frequent: long lists, ties
            d.w = draw_weights(rng, d.terms.shape[0], self.family)
            d.vecs = V.unit_rows(rng, int(counts[j]), self.tok_dim)
            d.stored = V.fp16_round(d.vecs)
            self._docs.append(d)


OPS = ("insert", "sparse_append", "tokvec_append", "delete", "fold", "compact")
PHRASES = (("insert", "sparse_append", "tokvec_append"), ("insert", "tokvec_append", "sparse_append"), ("tokvec_append", "insert", "sparse_append"),
           ("delete:base", "compact"), ("delete:tail", "compact"), ("delete:both", "compact"), ("delete:empty", "compact"), ("delete:last",),
           ("insert", "sparse_append", "delete:tail", "compact", "tokvec_append"), ("insert", "tokvec_append", "delete:both", "compact", "sparse_append"),
           ("tokvec_append", "delete:any", "compact", "insert", "sparse_append"), ("fold",), ("insert", "delete:any", "compact"),
           # the rarer classes once more: a tail-only and an empty-documents-only compaction, a store ahead of the index, a fold
           ("delete:tail", "compact"), ("delete:empty", "compact"), ("delete:empty", "compact", "insert"), ("tokvec_append", "delete:base", "compact"),
           ("fold", "insert", "sparse_append"))
_FREE = ("insert", "sparse_append", "tokvec_append", "delete:any", "delete:last", "fold", "compact")


@st.composite
def sequence_cases(draw, starts):
    """a start state and up to 12 operations: two or three phrases that reach the compaction classes (picked by a numpy generator over
    everything drawn, as in the other strategies) with the freely drawn operations put between them at drawn places"""
    case = dict(seed=draw(st.integers(0, 2**31 - 1)), n0=draw(starts), tok_dim=draw(st.sampled_from([32, 64])), v0=draw(st.integers(3, 60)),
                v_grow=draw(st.integers(0, 8)), family=draw(st.sampled_from(WEIGHT_FAMILIES)), rows_max=draw(st.sampled_from([2, 17, 40])),
                headroom=draw(st.integers(0, 60)), tail0=draw(st.integers(0, 30)), zero_query=draw(st.booleans()))
    free = draw(st.lists(st.tuples(st.sampled_from(_FREE), st.integers(0, 12)), min_size=0, max_size=5))
    params = draw(st.lists(st.tuples(st.integers(1, 40), st.integers(0, 2**16)), min_size=12, max_size=12))
    rng = np.random.default_rng([case["seed"], 2, case["n0"], case["headroom"], case["tail0"], len(free)] + [a for a, _ in params])
    kinds = [k for i in rng.integers(0, len(PHRASES), int(rng.integers(2, 4))) for k in PHRASES[int(i)]]
    for kind, at in free:
        kinds.insert(min(at, len(kinds)), kind)
    return dict(case, ops=[(kind, n, salt) for kind, (n, salt) in zip(kinds[:12], params)])


SMALL_STARTS = st.one_of(st.integers(1, 50), st.integers(2040, 2056))
LARGE_STARTS = st.integers(3000, 5000)


class Model:
    def __init__(self, world, docs=None):
        self.world = world
        self.rows = [world.doc(i) for i in range(world.n0)] if docs is None else list(docs)      # the document behind each index row
        self.dead = [False] * len(self.rows)
        self.next = world.n0                     # the world's next document (meaningless for a model built from given documents)
        self.sp_cov = self.sp_base = self.tv_docs = len(self.rows)
        self.sp_stale = False                    # the header's rule: set by an insert, cleared by the append that covers the last row
        self.n_terms = max([world.v0] + [int(d.terms[-1]) + 1 for d in self.rows if d.terms.shape[0]])
        self.tv_docs_cap = self.tv_rows_cap = None
        self.seen = set()                        # the classes this model's history has reached

    # ---- state -------------------------------------------------------------------------------------------------------------------
    @property
    def n_rows(self):
        return len(self.rows)

    def store_doc(self, d):
        """the document behind the store's document d: its index row, or - ahead of the index - the world's next documents"""
        return self.rows[d] if d < self.n_rows else self.world.doc(self.next + d - self.n_rows)

    def tv_rows(self):
        return sum(self.store_doc(d).vecs.shape[0] for d in range(self.tv_docs))

    def reserve(self, headroom):
        """the reservation the start state makes: `headroom` documents and their rows beyond what the store holds"""
        extra = sum(self.world.doc(self.next + j).vecs.shape[0] for j in range(headroom))
        self.tv_docs_cap, self.tv_rows_cap = max(1, self.tv_docs + headroom), self.tv_rows() + extra
        return self.tv_docs_cap, self.tv_rows_cap

    def consistent(self):
        assert self.sp_stale or self.sp_cov == self.n_rows
        return dict(dense=True, sparse=not self.sp_stale, tokvec=self.tv_docs == self.n_rows)

    def live_rows(self):
        return np.nonzero(~np.asarray(self.dead, dtype=bool))[0]

    def _note_state(self):
        c = self.consistent()
        if not c["sparse"] and c["tokvec"]:
            self.seen.add("sparse stale, the others current")
        if c["sparse"] and not c["tokvec"]:
            self.seen.add("token vectors stale, the others current")
        if c["sparse"] and c["tokvec"]:
            self.seen.add("every leg current again after a write")

    # ---- operations (each returns what the caller hands to the engine) -------------------------------------------------------------
    def insert(self, n):
        docs = [self.world.doc(self.next + j) for j in range(n)]
        self.rows += docs
        self.dead += [False] * n
        self.next += n
        self.sp_stale = True
        self.seen.add("insert")
        self._note_state()
        return docs

    def sparse_append(self, n, grow=0):
        """(rows lo, hi, n_terms) of the block, or None when every row is covered"""
        n = min(n, self.n_rows - self.sp_cov)
        if n <= 0:
            return None
        lo, hi = self.sp_cov, self.sp_cov + n
        need = max([self.n_terms] + [int(d.terms[-1]) + 1 for d in self.rows[lo:hi] if d.terms.shape[0]])
        self.n_terms = min(max(need, self.n_terms + grow), max(need, self.world.v_max))
        self.sp_cov = hi
        self.sp_stale = self.sp_stale and hi < self.n_rows
        self.seen.add("sparse_append")
        self._note_state()
        return lo, hi, self.n_terms

    def tokvec_append(self, n, ahead=6):
        """(store documents lo, hi) of the block, or None when nothing fits: at most `ahead` documents past the index, inside the
        reservation"""
        n = min(n, self.n_rows + ahead - self.tv_docs, (self.tv_docs_cap or 0) - self.tv_docs)
        room = (self.tv_rows_cap or 0) - self.tv_rows()
        lo = hi = self.tv_docs
        while hi - lo < n and self.store_doc(hi).vecs.shape[0] <= room:
            room -= self.store_doc(hi).vecs.shape[0]
            hi += 1
        if hi == lo:
            return None
        self.tv_docs = hi
        self.seen.add("tokvec_append")
        self._note_state()
        return lo, hi

    def pick_deletes(self, target, n, salt):
        """live rows to delete: in the postings' base, their tail, both, documents without token rows, the last row, or anywhere;
        one covered live row always stays (with none left a compaction keeps no postings: only a reload helps)"""
        rng = np.random.default_rng([self.world.seed, salt])
        live = self.live_rows()
        pools = {"base": live[live < self.sp_base], "tail": live[(live >= self.sp_base) & (live < self.sp_cov)],
                 "empty": np.array([r for r in live if self.rows[r].vecs.shape[0] == 0], dtype=np.int64), "last": live[live == self.n_rows - 1], "any": live}
        if target == "both":
            half = max(1, n // 2)
            rows = np.concatenate([rng.permutation(pools["base"])[:half], rng.permutation(pools["tail"])[:half]])
        else:
            rows = rng.permutation(pools[target])[:n]
        keep = live[live < self.sp_cov]
        if keep.shape[0] and np.isin(keep, rows).all():
            rows = rows[rows != keep[0]]
        return np.sort(rows).astype(np.int64)

    def delete(self, rows):
        for r in rows:
            assert not self.dead[r]
            self.dead[r] = True
        if len(rows):
            self.seen.add("delete")
            if self.n_rows - 1 in rows:
                self.seen.add("delete of the last row")
        return np.array([self.rows[r].id for r in rows], dtype=np.int64)

    def fold(self):
        self.sp_base = self.sp_cov
        self.seen.add("fold")

    def compact_live(self):
        """the row map int64 [rows before]: new row, or -1"""
        dead = np.asarray(self.dead, dtype=bool)
        row_map = np.where(dead, -1, np.cumsum(~dead) - 1).astype(np.int64)
        self.seen.add("compact")
        if not dead.any():
            return row_map
        in_base, in_tail = dead[:self.sp_base].any(), dead[self.sp_base:self.sp_cov].any()
        if self.sp_cov > self.sp_base and (in_base or in_tail):
            self.seen.add("compaction: deleted rows in " + ("base and tail" if in_base and in_tail else "the base only" if in_base else "the tail only"))
        gone = [r for r in np.nonzero(dead)[0] if r < self.tv_docs]
        if gone and all(self.rows[r].vecs.shape[0] == 0 for r in gone):
            self.seen.add("compaction: every deleted document has no token rows")
        if self.tv_docs < self.n_rows:
            self.seen.add("compaction: store behind the index")
        if self.tv_docs > self.n_rows:
            self.seen.add("compaction: store ahead of the index")
        below = lambda x: int((~dead[:min(x, self.n_rows)]).sum())
        base, cov = below(self.sp_base), below(self.sp_cov)
        assert cov > 0, "pick_deletes keeps a covered row"
        self.sp_base, self.sp_cov = (base, cov) if base and cov > base else (cov, cov)
        self.tv_docs = below(self.tv_docs) + max(0, self.tv_docs - self.n_rows)
        self.rows = [d for d, x in zip(self.rows, dead) if not x]
        self.dead = [False] * len(self.rows)
        self._note_state()
        return row_map

    # ---- read-outs ---------------------------------------------------------------------------------------------------------------
    def csr(self, lo, hi, n_terms=None):
        """term-major CSR of the rows [lo, hi), documents numbered from lo"""
        n_terms = self.n_terms if n_terms is None else n_terms
        docs = self.rows[lo:hi]
        term = np.concatenate([d.terms for d in docs]) if docs else np.zeros(0, np.int64)
        doc = np.repeat(np.arange(len(docs)), [d.terms.shape[0] for d in docs])
        w = np.concatenate([d.w for d in docs]) if docs else np.zeros(0, np.float32)
        return csr_of(term, doc, w, n_terms, len(docs))

    def packed(self, lo, hi, stored=False):
        """(vectors float32 [rows, dim], offsets int64) of the store's documents [lo, hi): as given, or as the store keeps them"""
        return M.pack([self.store_doc(d).stored if stored else self.store_doc(d).vecs for d in range(lo, hi)], self.world.tok_dim)

    def columns(self):
        return (np.stack([d.emb for d in self.rows]), np.array([d.id for d in self.rows], dtype=np.int64),
                np.array([d.tenant for d in self.rows], dtype=np.int32))

    def fresh(self):
        """(model of the surviving documents alone - what a new handle loads to reach this state - , row map into it)"""
        dead = np.asarray(self.dead, dtype=bool)
        m = Model(self.world, [d for d, x in zip(self.rows, dead) if not x])
        m.n_terms, m.next = self.n_terms, self.next
        return m, np.where(dead, -1, np.cumsum(~dead) - 1).astype(np.int64)

    # ---- references over a model without deleted rows (a fresh one) ------------------------------------------------------------------
    def sparse_scores(self, queries):
        return S.all_scores(*self.csr(0, self.n_rows), self.n_rows, queries)

    def dense_cos(self, q_emb, rows):
        """float64 cosine of one query against rows, 0.0 where either norm is zero"""
        q = np.asarray(q_emb, dtype=np.float64)
        r = np.stack([self.rows[i].emb for i in rows]).astype(np.float64)
        den = np.linalg.norm(q) * np.linalg.norm(r, axis=1)
        return np.where(den > 0, (r @ q) / np.where(den > 0, den, 1.0), 0.0)


def build_sequence(case):
    """(world, model at the start, queries): the start has `tail0` of its rows in the tail when it has more than that"""
    w = World(case["seed"], case["n0"], case["tok_dim"], case["v0"], case["v0"] + case["v_grow"], case["family"], 6, case["rows_max"])
    m = Model(w)
    m.sp_base = m.n_rows - case["tail0"] if m.n_rows > case["tail0"] else m.n_rows
    m.reserve(case["headroom"])
    rng = np.random.default_rng([case["seed"], 99])
    sq = draw_queries(rng, w.v_max, [7, 2, 0, 12], case["family"], np.arange(min(4, w.v0)))
    q_emb = rng.standard_normal((4, w.emb_dim)).astype(np.float32)
    q_emb[1] = m.rows[0].emb + 0.2 * rng.standard_normal(w.emb_dim).astype(np.float32)
    if case["zero_query"]:
        q_emb[2] = 0.0
    qv, qo = M.pack([V.unit_rows(rng, c, w.tok_dim) for c in (5, 0, 33, 1)], w.tok_dim)
    return w, m, dict(sparse=sq, packed=S.pack_queries(sq), q_emb=q_emb, qv=qv, qo=qo)


def apply(m, op):
    """run one drawn operation on the model; returns (kind, payload for the engine or None when the state left nothing to do)"""
    kind, n, salt = op
    full = salt % 4 != 0                         # three times in four an insert or an append closes the whole gap it finds, else n
    if kind == "insert":
        return kind, m.insert(m.tv_docs - m.n_rows if full and m.tv_docs > m.n_rows else n)
    if kind == "sparse_append":
        return kind, m.sparse_append(m.n_rows - m.sp_cov if full else n, grow=salt % 3)
    if kind == "tokvec_append":
        return kind, m.tokvec_append(m.n_rows - m.tv_docs if full and m.tv_docs < m.n_rows else n)
    if kind.startswith("delete"):
        rows = m.pick_deletes(kind.split(":")[1], n, salt)
        return "delete", (rows, m.delete(rows)) if len(rows) else None
    if kind == "fold":
        m.fold()
        return kind, True
    return "compact", m.compact_live()


SEQUENCE_CLASSES = ("insert", "sparse_append", "tokvec_append", "delete", "fold", "compact", "compaction: deleted rows in the base only",
                    "compaction: deleted rows in the tail only", "compaction: deleted rows in base and tail",
                    "compaction: every deleted document has no token rows", "compaction: store behind the index",
                    "compaction: store ahead of the index", "sparse stale, the others current", "token vectors stale, the others current",
                    "every leg current again after a write", "delete of the last row")
