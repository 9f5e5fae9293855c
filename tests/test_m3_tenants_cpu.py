"""CPU: GpuDocumentIndex.search_lexical_many / search_m3_many over a recording numpy engine (the style of
tests/test_tenants_per_query_cpu.py): a batch goes out as ONE search call with an int32 tenant array of length Q (an unknown agent:
the number no row carries; None: -1), the ids it returns are mapped back to the rows' payloads, an unknown agent gets [], the
lexical forms equal the single-query calls, failures are answered as the single-query methods answer them - and a tenant array
of the wrong shape is a RagError before the library is touched."""
import types

import numpy as np
import pytest

from optimized_rag_amd.document_store import GpuDocumentIndex
from oracle import rag_oracle as O

D, V, N = 16, 40, 60
SEARCHES = ("sparse_topk", "dense_topk", "hybrid_sparse_rrf_dev", "retrieve_m3_dev")


class RecordingEngine:
    """numpy stand-in of the engine methods the lexical and three-way searches use; records (method, tenant, arguments) per call.
    ids are explicit (500 + 7 * row) and the device methods return ids, as the library's do."""

    def __init__(self, rng):
        self.calls = []
        self.fail = False
        self.W = np.where(rng.random((N, V)) < 0.2, rng.random((N, V)) + 0.01, 0.0).astype(np.float32)

    def searches(self):
        return [c for c in self.calls if c[0] in SEARCHES]

    def index_load(self, emb):
        self.emb = np.asarray(emb, np.float32)

    def set_tenants(self, t):
        self.ten = np.asarray(t, np.int32)

    def set_ids(self, ids):
        self.ids = np.asarray(ids, np.int64)

    def _tenants(self, tenant, Q):
        if isinstance(tenant, (int, np.integer)):
            return np.full(Q, int(tenant))
        assert isinstance(tenant, np.ndarray) and tenant.dtype == np.int32 and tenant.shape == (Q,)
        return tenant

    def _top(self, s, t, k):
        cand = np.nonzero(self.ten == t)[0] if t >= 0 else np.arange(N)
        return cand[np.argsort(-s[cand], kind="stable")][:k]

    def _dense(self, q):
        q, e = np.asarray(q, np.float64), self.emb.astype(np.float64)
        return np.stack([(e @ q[i]) / (np.linalg.norm(q[i]) * np.linalg.norm(e, axis=1)) for i in range(len(q))])

    def _sparse(self, ptr, terms, weights):
        out = np.zeros((len(ptr) - 1, N))
        for i in range(len(ptr) - 1):
            for t, w in zip(terms[ptr[i]:ptr[i + 1]], weights[ptr[i]:ptr[i + 1]]):
                if 0 <= t < V:
                    out[i] += np.float64(w) * self.W[:, t].astype(np.float64)
        return out

    def _lists(self, s, tenant, k, positive):
        rows, sc = np.full((len(s), k), -1, np.int32), np.zeros((len(s), k))
        for i, t in enumerate(self._tenants(tenant, len(s))):
            top = self._top(s[i], int(t), k)
            top = top[s[i][top] > 0] if positive else top
            rows[i, :len(top)], sc[i, :len(top)] = top, s[i][top]
        return np.where(rows >= 0, self.ids[np.maximum(rows, 0)], -1), rows, sc

    def dense_topk(self, q, k, tenant=-1):
        self.calls.append(("dense_topk", tenant))
        return self._lists(self._dense(q), tenant, k, False)

    def sparse_topk(self, ptr, terms, weights, k, tenant=-1):
        if self.fail:
            raise RuntimeError("no postings")
        self.calls.append(("sparse_topk", tenant))
        return self._lists(self._sparse(ptr, terms, weights), tenant, k, True)

    def sparse_score_rows(self, ptr, terms, weights, rows):
        self.calls.append(("sparse_score_rows", None))
        s = self._sparse(ptr, terms, weights)
        return np.where(rows >= 0, np.take_along_axis(s, np.maximum(rows, 0).astype(np.int64), axis=1), 0.0)

    def rrf_fuse(self, lists, rrf_k=60, top_k=10):
        Q = lists.shape[0]
        keys, sc, ranks = np.full((Q, top_k), -1, np.int64), np.zeros((Q, top_k)), np.zeros((Q, top_k, 2), np.int32)
        for i in range(Q):
            k_, s_, r_ = O.rrf_fuse([[int(x) for x in l if x >= 0] for l in lists[i]], k=rrf_k, top_k=top_k)
            keys[i, :len(k_)], sc[i, :len(k_)] = k_, s_
            ranks[i, :len(k_)] = np.asarray(r_).reshape(-1, 2)
        return keys, sc, ranks

    def _candidates(self, q, ptr, terms, weights, pool, top_k, rrf_k, tenant):
        d_ids, _, _ = self._lists(self._dense(q), tenant, pool, False)
        s_ids, _, _ = self._lists(self._sparse(ptr, terms, weights), tenant, pool, True)
        return self.rrf_fuse(np.stack([d_ids, s_ids], axis=1), rrf_k=rrf_k, top_k=top_k)

    def hybrid_sparse_rrf_dev(self, q, ptr, terms, weights, pool, k, rrf_k=60, tenant=-1, stream=None):
        self.calls.append(("hybrid_sparse_rrf_dev", tenant, dict(pool=pool, k=k)))
        return self._candidates(q, ptr, terms, weights, pool, k, rrf_k, tenant)

    def retrieve_m3_dev(self, q, pool, k, term_ptr=None, terms=None, weights=None, q_vecs=None, q_off=None, mode=2, w=(0.4, 0.2, 0.4),
                        rrf_k=60, tenant=-1, stream=None):
        if self.fail:
            raise RuntimeError("no token vectors")
        self.calls.append(("retrieve_m3_dev", tenant, dict(pool=pool, k=k, mode=mode, w=w, sparse=term_ptr is not None, colbert=q_vecs is not None)))
        Q = len(q)
        if mode == 0:
            cand, _, _ = self._lists(self._dense(q), tenant, pool, False)
        else:
            cand, _, _ = self._candidates(q, term_ptr, terms, weights, pool, 2 * pool if mode == 2 else pool, rrf_k, tenant)
        dn = self._dense(q)
        sp = self._sparse(term_ptr, terms, weights) if w[1] > 0 else np.zeros((Q, N))
        ids, sc, comp = np.full((Q, k), -1, np.int64), np.zeros((Q, k)), np.zeros((Q, k, 3))
        for i in range(Q):
            rows = (cand[i][cand[i] >= 0] - 500) // 7
            c = np.stack([dn[i][rows] if w[0] > 0 else 0 * rows, sp[i][rows], 0.5 * dn[i][rows] if w[2] > 0 else 0 * rows], axis=1).astype(np.float64)
            s = ((w[2] * c[:, 2] + w[1] * c[:, 1]) + w[0] * c[:, 0]) / ((w[0] + w[1]) + w[2])
            top = np.argsort(-s, kind="stable")[:k]
            ids[i, :len(top)], sc[i, :len(top)], comp[i, :len(top)] = self.ids[rows[top]], s[top], c[top]
        return ids, sc, comp, cand


class Embedder:
    """encode_multi over fixed tables; counts the forwards"""

    def __init__(self, rng, queries):
        self.dense = {q: rng.standard_normal(D).astype(np.float32) for q in queries}
        self.lex = {q: {int(t): float(rng.random() + 0.1) for t in rng.choice(V, int(rng.integers(1, 5)), replace=False)} for q in queries}
        self.vecs = {q: rng.standard_normal((3, 8)).astype(np.float32) for q in queries}
        self.forwards = []

    def encode_multi(self, texts, return_dense=True, return_sparse=True, return_colbert_vecs=True):
        self.forwards.append(len(texts))
        return dict(dense_vecs=np.stack([self.dense[t] for t in texts]) if return_dense else None,
                    lexical_weights=[self.lex[t] for t in texts] if return_sparse else None,
                    colbert_vecs=[self.vecs[t] for t in texts] if return_colbert_vecs else None)

    def generate_embedding(self, text):
        return self.dense[text].tolist()


def make_index():
    rng = np.random.default_rng(3)
    eng = RecordingEngine(rng)
    queries = [f"q{i}" for i in range(9)]
    idx = GpuDocumentIndex(Embedder(rng, queries), dim=D, engine=eng)
    idx._to_device = lambda a: a                                         # the stand-in computes on the host arrays
    idx._to_host = lambda *t: list(t)
    agents = ["a0", "a1", "a2"]
    rows = [{"content": f"c{i}", "agent_id": agents[i % 3] if i >= 4 else "tiny", "id": 500 + 7 * i} for i in range(N)]
    idx.bulk_load(rows, rng.standard_normal((N, D)).astype(np.float32))
    return idx, eng, queries


AGENTS = ["a0", "a2", "nobody", "tiny", None, "a0", "ghost", "a2", "a1"]


def check_tenant_array(idx, tenant):
    assert isinstance(tenant, np.ndarray) and tenant.dtype == np.int32 and tenant.shape == (len(AGENTS),)
    known = set(idx._tenant_id.values())
    for a, t in zip(AGENTS, tenant):
        if a is None:
            assert t == -1
        elif a in idx._tenant_id:
            assert t == idx._tenant_id[a]
        else:
            assert t >= 0 and int(t) not in known                         # an unknown agent searches under a tenant no row has


@pytest.mark.parametrize("mode", ["sparse", "dense+sparse"])
def test_search_lexical_many_is_one_search_call_and_equals_the_single_calls(mode):
    idx, eng, qs = make_index()
    single = [idx.search_lexical(a, q, top_k=5, mode=mode, pool=12) for a, q in zip(AGENTS, qs)]
    eng.calls.clear()
    idx.embeddings.forwards.clear()
    many = idx.search_lexical_many(AGENTS, qs, top_k=5, mode=mode, pool=12)
    assert idx.embeddings.forwards == [9]                                # ONE forward for all queries
    assert len(eng.searches()) == 1                                      # ONE search call, with a tenant array
    name, tenant = eng.searches()[0][:2]
    assert name == ("sparse_topk" if mode == "sparse" else "hybrid_sparse_rrf_dev")
    check_tenant_array(idx, tenant)
    assert [c[0] for c in eng.calls if c[0] not in SEARCHES] == ([] if mode == "sparse" else ["sparse_score_rows"])
    assert many == single
    assert many[2] == [] and many[6] == [] and sum(len(m) for m in many) > 15
    assert all(r["content"].startswith("c") for m in many for r in m)
    if mode != "sparse":
        assert eng.searches()[0][2] == dict(pool=12, k=5)
        eng.calls.clear()
        idx.search_lexical_many(AGENTS, qs, top_k=20, mode=mode, pool=12)
        assert eng.searches()[0][2] == dict(pool=20, k=20)               # pool is at least top_k, as in search_lexical
    eng.calls.clear()
    assert idx.search_lexical_many("a1", qs, top_k=4, mode=mode) == idx.search_lexical_many(["a1"] * 9, qs, top_k=4, mode=mode)
    assert [int(t) for t in eng.searches()[0][1]] == [idx._tenant_id["a1"]] * 9
    assert idx.search_lexical_many(["a0"], qs[:2], mode=mode) == [[], []]            # a list of the wrong length: logged, answered empty
    assert idx.search_lexical_many(AGENTS, qs, mode="bm25") == [[] for _ in qs]
    eng.fail = True
    assert idx.search_lexical_many(AGENTS, qs, mode="sparse") == [[] for _ in qs]


@pytest.mark.parametrize("candidates,mode,cap", [("dense", 0, 256), ("dense+sparse", 1, 256), ("union", 2, 128)])
def test_search_m3_many_is_one_device_call(candidates, mode, cap):
    idx, eng, qs = make_index()
    many = idx.search_m3_many(AGENTS, qs, top_k=5, pool=12, candidates=candidates)
    assert idx.embeddings.forwards == [9]
    assert len(eng.calls) == 1 and eng.calls[0][0] == "retrieve_m3_dev"
    check_tenant_array(idx, eng.calls[0][1])
    assert eng.calls[0][2] == dict(pool=12, k=5, mode=mode, w=(0.4, 0.2, 0.4), sparse=True, colbert=True)
    assert many[2] == [] and many[6] == [] and len(many[0]) == 5 and len(many[3]) == 4      # `tiny` owns 4 rows: no padding leaks out
    ten = {a: t for a, t in idx._tenant_id.items()}
    for a, m in zip(AGENTS, many):
        rows = [int(r["content"][1:]) for r in m]
        assert a is None or all(eng.ten[r] == ten[a] for r in rows)      # the ids came back as THIS index's rows
        assert all(set(r) == {"content", "filename", "file_type", "score", "dense_score", "sparse_score", "colbert_score", "metadata"} for r in m)
        sc = [r["score"] for r in m]
        assert sc == sorted(sc, reverse=True)
    # each query's answer does not depend on the batch it came in, and a one-agent string is the list with that agent repeated
    for i in (0, 3, 4, 8):
        assert idx.search_m3_many([AGENTS[i]], [qs[i]], top_k=5, pool=12, candidates=candidates) == [many[i]]
    assert idx.search_m3_many("a2", qs, top_k=3, candidates=candidates) == idx.search_m3_many(["a2"] * 9, qs, top_k=3, candidates=candidates)
    # pool is clamped as search_m3 clamps it; a weight of 0 leaves its inputs out
    eng.calls.clear()
    idx.search_m3_many(AGENTS, qs, top_k=7, pool=500, weights=(1.0, 0.0, 0.0), candidates=candidates)
    assert eng.calls[0][2] == dict(pool=cap, k=7, mode=mode, w=(1.0, 0.0, 0.0), sparse=mode != 0, colbert=False)
    eng.calls.clear()
    idx.search_m3_many(AGENTS, qs, top_k=9, pool=2, candidates=candidates)
    assert eng.calls[0][2]["pool"] == 9 and eng.calls[0][2]["k"] == 9


def test_search_m3_many_failures_are_answered_with_search_many():
    idx, eng, qs = make_index()
    plain = idx.search_many(AGENTS, qs, top_k=5, with_embeddings=False)
    assert sum(len(p) for p in plain) > 20
    assert idx.search_m3_many(AGENTS, qs, top_k=5, candidates="bm25") == plain
    assert idx.search_m3_many(AGENTS, qs, top_k=5, weights=(0.4, 0.2)) == plain
    eng.fail = True
    assert idx.search_m3_many(AGENTS, qs, top_k=5) == plain
    assert idx.search_m3_many(["a0"], qs[:2], top_k=5) == [[], []]       # a list of the wrong length: search_many's answer for it


def test_index_without_any_known_agent():
    """No agent known: a query under an agent finds nothing and is not sent; the unfiltered ones go out as one unfiltered call."""
    idx, eng, qs = make_index()
    idx._tenant_id = {}
    for call, name in ((lambda a, q: idx.search_lexical_many(a, q, top_k=3, mode="sparse"), "sparse_topk"),
                       (lambda a, q: idx.search_m3_many(a, q, top_k=3, pool=10), "retrieve_m3_dev")):
        eng.calls.clear()
        out = call(["a0", None, "a1", None], qs[:4])
        assert len(eng.searches()) == 1 and eng.searches()[0][0] == name and eng.searches()[0][1].tolist() == [-1, -1]
        assert out[0] == [] and out[2] == [] and len(out[1]) == 3 and len(out[3]) == 3
        assert [out[1], out[3]] == call([None, None], [qs[1], qs[3]])
        eng.calls.clear()
        assert call(["a0", "a1"], qs[:2]) == [[], []] and eng.calls == []


def test_tenant_arrays_of_the_wrong_shape_are_refused_before_the_library_is_touched():
    from optimized_rag_amd import RagEngine, RagError
    from optimized_rag_amd._lib import _tenant_arg
    ptr, terms, w = np.array([0, 1, 2, 3], np.int32), np.zeros(3, np.int32), np.ones(3, np.float32)
    nothing = types.SimpleNamespace()                                    # no .lib, no .h: reaching for either is an AttributeError
    for bad in ([1, 2], np.zeros((3, 1), np.int32), np.zeros(4, np.int32)):
        with pytest.raises(RagError, match="tenant"):
            RagEngine.sparse_topk(nothing, ptr, terms, w, 5, tenant=bad)
        with pytest.raises(RagError, match="tenant"):
            _tenant_arg(bad, 3)
    with pytest.raises(AttributeError):                                  # a well-formed array goes on to the per-query entry
        RagEngine.sparse_topk(nothing, ptr, terms, w, 5, tenant=[0, -1, 2])
