"""GPU: a handle gives back every byte of device memory it took.

Every device allocation of the library has one owner (csrc/common.h dev_buf): destroying a handle, reloading a component on a
live handle and an argument error inside a load must each leave the device's free memory where it was. Free memory is read
with torch.cuda.mem_get_info() (hipMemGetInfo) and compared for EQUALITY: hipFree returns memory at once. Every torch tensor
the steps need is created once, before the first reading, so torch's own allocator takes nothing new between readings.
One process, the steps in sequence (test order matters only for speed: each test builds what it needs)."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, L_TOK, LQ, Q, POOL, K, L_PAIR = 3000, 256, 24, 8, 4, 16, 5, 32
N_INS = 500                     # inserted rows: more than the growth headroom of 3000 loaded rows, so every plane reallocates
CFG = dict(vocab_size=2000, hidden=384, layers=2, heads=12, ffn=1536, max_pos=64, type_vocab=2, eps=1e-12)   # smoke()'s model


class World:
    """Host data of one handle and the device tensors of its searches, made once per process."""

    def __init__(self):
        import torch
        from optimized_rag_amd.bm25 import Bm25Postings
        from optimized_rag_amd.cross_encoder import flatten_state_dict
        from oracle import bert_oracle as B
        rng = np.random.default_rng(11)
        self.emb = rng.standard_normal((N, D)).astype(np.float32)
        self.ids = (10_000 + 3 * np.arange(N)).astype(np.int64)
        self.tenants = (np.arange(N) // 750).astype(np.int32)                  # four tenants, stored contiguously
        self.temporal = (0.1 * rng.random(N)).astype(np.float64)
        self.tok = rng.integers(200, CFG["vocab_size"], (N, L_TOK)).astype(np.int32)
        self.tok_len = rng.integers(3, L_TOK + 1, N).astype(np.int32)
        corpus = [" ".join(f"t{t}" for t in self.tok[i, :self.tok_len[i]] % 50) for i in range(N)]
        self.post = Bm25Postings.from_corpus(corpus)
        w = B.seeded_weights(CFG, 7)
        self.ce_tensors = flatten_state_dict(w, CFG["layers"])
        self.emb_tensors = flatten_state_dict(w, CFG["layers"], head=False)
        self.ins_emb = rng.standard_normal((N_INS, D)).astype(np.float32)
        self.ins_ids = (900_000 + np.arange(N_INS)).astype(np.int64)
        self.ins_tok = rng.integers(200, CFG["vocab_size"], (N_INS, L_TOK)).astype(np.int32)
        self.ins_tok_len = rng.integers(3, L_TOK + 1, N_INS).astype(np.int32)
        q = (self.emb[rng.integers(0, N, Q)] + 0.5 * rng.standard_normal((Q, D))).astype(np.float32)
        q_tok = rng.integers(200, CFG["vocab_size"], (Q, LQ)).astype(np.int32)
        ptr, terms = self.post.encode_queries([" ".join(f"t{t}" for t in q_tok[i] % 50) for i in range(Q)])
        self.q_host = q
        self.embed_ids = np.ascontiguousarray(self.tok[:6, :16])
        self.embed_tt = np.zeros_like(self.embed_ids)
        self.embed_lens = np.minimum(self.tok_len[:6], 16).astype(np.int32)
        cuda = lambda a: torch.from_numpy(a).cuda()                            # noqa: E731
        self.q, self.q_tok, self.q_len = cuda(q), cuda(q_tok), cuda(np.full(Q, LQ, dtype=np.int32))
        self.ptr, self.terms = cuda(ptr), cuda(terms)
        self.mmr_sel = torch.empty((Q, K), dtype=torch.int32, device="cuda")
        self.mmr_sc = torch.empty((Q, K), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

    def load_index(self, eng):
        eng.index_load(self.emb, ids=self.ids)
        eng.set_tenants(self.tenants)
        eng.set_temporal(self.temporal)

    def load_all(self, eng):
        self.load_index(eng)
        self.post.load(eng)
        eng.tokens_load(self.tok, self.tok_len)
        eng.ce_load(CFG, self.ce_tensors)
        eng.embed_load(CFG, self.emb_tensors)

    def searches(self, eng):
        """Every search path of a fully loaded handle -> host copies of the results."""
        import torch
        out = {}
        out["dense"] = eng.dense_topk(self.q_host, K)
        out["dense_tenant"] = eng.dense_topk(self.q_host, K, tenant=2)
        keys, rrf, ranks = eng.hybrid_rrf_dev(self.q, self.ptr, self.terms, POOL, K)
        torch.cuda.synchronize()
        out["rrf"] = (keys.cpu().numpy(), rrf.cpu().numpy(), ranks.cpu().numpy())
        lin = eng.hybrid_linear_dev(self.q, self.ptr, self.terms, K, 0.6, 0.3, 0.1)
        torch.cuda.synchronize()
        out["linear"] = tuple(lin[n].cpu().numpy() for n in ("ids", "rows", "hybrid", "semantic", "keyword", "temporal"))
        rr = eng.retrieve_rerank_dev(self.q, self.q_tok, self.q_len, POOL, K, term_ptr=self.ptr, terms=self.terms, L_pair=L_PAIR)
        torch.cuda.synchronize()
        out["rerank"] = tuple(t.cpu().numpy() for t in rr)
        eng.mmr_select_dev(self.q, lin["rows"], K, 0.7, 0, self.mmr_sel, self.mmr_sc)
        torch.cuda.synchronize()
        out["mmr"] = (self.mmr_sel.cpu().numpy(), self.mmr_sc.cpu().numpy())
        out["embed"] = (eng.embed(self.embed_ids, self.embed_tt, self.embed_lens),)
        return out


@pytest.fixture(scope="module")
def world():
    return World()


def free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def destroy(eng):
    eng.close()
    del eng
    gc.collect()          # the engine's cached output tensors go back to torch's allocator (which keeps the memory)


def assert_same_bits(a, b):
    assert a.keys() == b.keys()
    for name in a:
        for x, y in zip(a[name], b[name]):
            assert x.dtype == y.dtype and x.shape == y.shape, name
            np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=name)


def full_life(world):
    """Build a handle with everything on it, use every search and every write, destroy it."""
    from optimized_rag_amd import RagEngine
    eng = RagEngine(dim=D, device=0)
    world.load_all(eng)
    world.searches(eng)
    assert eng.index_delete(world.ids[100:400:3]) == 100
    first = eng.index_insert(world.ins_emb, ids=world.ins_ids, tenants=np.full(N_INS, 1, dtype=np.int32),
                             temporal=np.zeros(N_INS), tokens=world.ins_tok, token_lens=world.ins_tok_len)
    assert first == N                                           # 3000 loaded rows had no spare capacity: every plane grew
    row_map = eng.index_compact()
    assert (row_map < 0).sum() == 100 and eng.n_rows == N + N_INS - 100
    ids, _, _ = eng.dense_topk(world.ins_emb[:2], 1)            # the moved rows are searchable
    assert ids[:, 0].tolist() == world.ins_ids[:2].tolist()
    destroy(eng)


def test_destroy_returns_all_device_memory(world):
    """Three full lives of a handle in a row. The first absorbs one-time allocations of the runtime and of torch; after the
    second and the third, free memory equals the value after the first."""
    free = []
    for _ in range(3):
        full_life(world)
        free.append(free_bytes())
    print("free bytes after each destroy:", free)
    assert free[1] == free[0] and free[2] == free[0]


def test_reload_on_a_live_handle_replaces_and_frees(world):
    """index / BM25 / cross-encoder / token store loaded twice in a row on a handle in use: the second load frees what the
    first made (free memory is the same after both), and the searches return the first round's results bit for bit."""
    from optimized_rag_amd import RagEngine
    eng = RagEngine(dim=D, device=0)
    try:
        world.load_all(eng)
        before = world.searches(eng)
        for name, load in (("index_load", lambda: world.load_index(eng)), ("bm25_load", lambda: world.post.load(eng)),
                           ("ce_load", lambda: eng.ce_load(CFG, world.ce_tensors)),
                           ("tokens_load", lambda: eng.tokens_load(world.tok, world.tok_len))):
            load()
            first = free_bytes()
            load()
            second = free_bytes()
            print(f"{name}: free after first / second load: {first} / {second}")
            assert second == first, name
        assert_same_bits(world.searches(eng), before)
    finally:
        destroy(eng)


def test_rejected_load_leaves_memory_and_the_loaded_postings(world):
    """rag_bm25_load_host with a decreasing indptr is an argument error found while the new index is being built. State
    afterwards, as csrc/bm25.hip documents it (bm25_build hands the index over on success only, and bm25_load_host replaces the
    resident postings only then): the postings loaded before stay resident and searchable, and no device memory was taken."""
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd._lib import RagError
    eng = RagEngine(dim=D, device=0)
    try:
        world.load_all(eng)
        before = world.searches(eng)
        free0 = free_bytes()
        p = world.post
        bad = p.indptr.copy()
        bad[len(bad) // 2] = bad[len(bad) // 2 - 1] - 1          # one term with a negative posting count
        with pytest.raises(RagError, match="non-decreasing"):
            eng.bm25_load(bad, p.doc, p.tf, p.doc_len, p.idf, p.avgdl, p.k1, p.b)
        assert free_bytes() == free0
        assert_same_bits(world.searches(eng), before)
    finally:
        destroy(eng)
