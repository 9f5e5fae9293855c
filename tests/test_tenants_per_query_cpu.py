"""CPU: GpuDocumentIndex.search_many / search_batch with ONE AGENT PER QUERY, over a recording numpy engine (the style of
tests/test_live_document_index.py): the batch goes out as one dense call with a tenant array, element i equals the single
call, an unknown agent gives [], and a scalar agent_id still takes the scalar path."""
import numpy as np

from optimized_rag_amd.document_store import GpuDocumentIndex

D = 16


class RecordingEngine:
    """Exact float64 cosine top-k with a scalar tenant or a tenant per query; records the `tenant` argument of every call."""

    def __init__(self):
        self.calls = []

    def index_load(self, emb):
        self.emb = np.asarray(emb, np.float32)

    def set_tenants(self, t):
        self.ten = np.asarray(t, np.int32)

    def set_ids(self, ids):
        pass

    def fetch_rows(self, rows):
        return self.emb[np.asarray(rows, dtype=np.int64)]

    def dense_topk(self, q, k, tenant=-1):
        self.calls.append(tenant)
        per_query = not isinstance(tenant, (int, np.integer))
        if per_query:
            assert isinstance(tenant, np.ndarray) and tenant.dtype == np.int32 and tenant.shape == (len(q),)
        q, e = q.astype(np.float64), self.emb.astype(np.float64)
        # one matrix-vector product per query: the same bits whatever batch the query arrives in
        s = np.stack([(e @ q[i]) / (np.linalg.norm(q[i]) * np.linalg.norm(e, axis=1)) for i in range(len(q))])
        rows = np.full((len(q), k), -1, np.int32)
        sc = np.zeros((len(q), k))
        for i in range(len(q)):
            t = int(tenant[i]) if per_query else int(tenant)
            cand = np.nonzero(self.ten == t)[0] if t >= 0 else np.arange(len(e))
            top = cand[np.argsort(-s[i, cand], kind="stable")][:k]
            rows[i, :len(top)] = top
            sc[i, :len(top)] = s[i, top]
        return None, rows, sc


class Embedder:
    def __init__(self, table):
        self.table = table

    def generate_embedding(self, text):
        return self.table[text]


def make_index():
    rng = np.random.default_rng(3)
    eng = RecordingEngine()
    idx = GpuDocumentIndex(None, dim=D, engine=eng)
    agents = ["a0", "a1", "a2"]
    rows = [{"content": f"c{i}", "agent_id": agents[i % 3] if i >= 4 else "tiny", "id": 500 + i} for i in range(60)]
    emb = rng.standard_normal((60, D)).astype(np.float32)
    idx.bulk_load(rows, emb)
    queries = {f"q{i}": rng.standard_normal(D).astype(np.float32).tolist() for i in range(9)}
    idx.embeddings = Embedder(queries)
    return idx, eng, list(queries)


def test_search_many_with_one_agent_per_query_equals_the_single_calls():
    idx, eng, qs = make_index()
    agents = ["a0", "a2", "nobody", "tiny", "a1", "a0", "ghost", "a2", "tiny"]
    single = [idx.search(a, q, 5) for a, q in zip(agents, qs)]
    eng.calls.clear()
    many = idx.search_many(agents, qs, 5)
    assert len(eng.calls) == 1 and isinstance(eng.calls[0], np.ndarray)            # ONE call, with a tenant array
    assert many == single
    assert many[2] == [] and many[6] == []                                         # unknown agents
    assert len(many[3]) == 4 and len(many[0]) == 5                                 # fewer rows than top_k: no padding leaks out
    known = {idx._tenant_id[a] for a in ("a0", "a1", "a2", "tiny")}
    assert int(eng.calls[0][2]) >= 0 and int(eng.calls[0][2]) not in known         # an unknown agent searches under a tenant no row has


def test_search_batch_with_agent_list_and_unfiltered_queries():
    idx, eng, qs = make_index()
    embs = np.asarray([idx.embeddings.table[q] for q in qs], dtype=np.float32)
    agents = ["a1", None, "nobody", "a0", None, "tiny", "a1", "a2", "a0"]
    rows, scores = idx.search_batch(agents, embs, 6)
    assert rows.shape == (9, 6) and scores.shape == (9, 6)
    for i, a in enumerate(agents):
        r1, s1 = idx.search_batch(a, embs[i:i + 1], 6)
        np.testing.assert_array_equal(rows[i], r1[0])
        np.testing.assert_array_equal(scores[i].view(np.int64), s1[0].view(np.int64))
    assert (rows[2] == -1).all() and (scores[2] == 0).all()


def test_agent_list_beside_the_scalar_agent_on_one_index():
    """the same index serves both forms: a list goes out as an array, a scalar agent_id still takes the scalar path"""
    idx, eng, qs = make_index()
    idx.search_many(["a1", "a0", "a1"], qs[:3], 4)
    assert len(eng.calls) == 1 and isinstance(eng.calls[0], np.ndarray)
    eng.calls.clear()
    out = idx.search_many("a1", qs[:3], 4)
    assert len(out) == 3 and all(len(o) == 4 for o in out)
    assert eng.calls == [idx._tenant_id["a1"]] and isinstance(eng.calls[0], int)    # one call, an int tenant as before
    eng.calls.clear()
    assert idx.search_many("nobody", qs[:3], 4) == [[], [], []] and eng.calls == []  # unknown scalar agent: no engine call
    idx.search_batch(None, np.zeros((2, D), np.float32) + 1, 3)
    assert eng.calls == [-1]
    eng.calls.clear()
    assert idx.search_many(["a0"], qs[:2], 3) == [[], []] and eng.calls == []      # a list of the wrong length: logged, answered empty


def test_index_without_any_known_agent():
    """No agent known (no tenant table on the engine): a query under an agent finds nothing and is not sent; the unfiltered
    queries of the same batch go out as ONE unfiltered call."""
    rng = np.random.default_rng(4)
    eng = RecordingEngine()
    idx = GpuDocumentIndex(None, dim=D, engine=eng)
    emb = rng.standard_normal((20, D)).astype(np.float32)
    eng.index_load(emb)
    eng.set_tenants(np.zeros(20, np.int32))
    q = rng.standard_normal((4, D)).astype(np.float32)
    assert idx._tenant_id == {}
    rows, scores = idx.search_batch(["a0", None, "a1", None], q, 3)
    assert len(eng.calls) == 1 and eng.calls[0] == -1
    assert (rows[[0, 2]] == -1).all() and (scores[[0, 2]] == 0).all()
    _, r1, s1 = eng.dense_topk(q[[1, 3]], 3, tenant=-1)
    np.testing.assert_array_equal(rows[[1, 3]], r1)
    np.testing.assert_array_equal(scores[[1, 3]].view(np.int64), s1.view(np.int64))
    eng.calls.clear()
    rows, _ = idx.search_batch(["a0", "a1"], q[:2], 3)
    assert (rows == -1).all() and eng.calls == []


def test_tenant_argument_forms():
    """an int, a numpy integer, a 0-d array: ONE tenant (the scalar entries, as int(tenant) took them before); a sequence of
    length Q: a tenant per query; any other shape is refused"""
    import pytest
    from optimized_rag_amd import RagError
    from optimized_rag_amd._lib import _tenant_arg
    for one in (3, np.int32(3), np.int64(3), np.array(3), np.array(3, dtype=np.int16)):
        assert _tenant_arg(one, 5) == (False, 3)
    assert _tenant_arg(np.array(-1), 1) == (False, -1)
    per_query, t = _tenant_arg([1, -1, 2], 3)
    assert per_query and t.dtype == np.int32 and t.tolist() == [1, -1, 2] and t.flags["C_CONTIGUOUS"]
    per_query, t = _tenant_arg(np.array([7]), 1)
    assert per_query and t.shape == (1,)
    for bad in ([1, 2], np.zeros((3, 1), np.int32)):
        with pytest.raises(RagError):
            _tenant_arg(bad, 3)
