"""GPU: live writes on row shards with explicit ids (sharded.py insert_rows / delete_ids / compact / refresh_statistics over the
device id-to-row map). One process: three handles hold unequal shards, a fourth holds the whole corpus in id order with the same
explicit ids and receives the same inserts, the same deletes and rag_bm25_refresh where the shards refreshed. After every step
every sharded search must return the bits of the one-call entry on the whole handle. The gathers are torch.stack here and real
collectives in tests/test_sharded_writes_two_ranks_gpu.py. Everything is exact.

Worlds: tests/linear_sharded_tools.py (BM25, temporal scores, tenants, an exact tie across two shards) for search / search_hybrid /
search_linear, tests/m3_fused_tools.py (learned-sparse postings, token vectors) for search_m3 / search_late_interaction /
search_lexical. Explicit ids are 7 + 3 * global row."""
import numpy as np
import pytest

import linear_sharded_tools as L
import m3_fused_tools as F

pytestmark = pytest.mark.gpu

K, POOL = L.K, 30
BLOCKS = (2500, 450, 100, 60)                  # rows of the four inserted blocks: the first three must go to ranks 2, 0, 1
NEW_A, NEW_C = 10, 5                           # terms the first and the third block introduce: numbers 300 .. 309, 310 .. 314


def gid(rows):
    return 7 + 3 * np.asarray(rows, dtype=np.int64)


def cuda(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()                     # (a copy: the worlds' arrays are read-only)


def bits(t):
    import torch
    t = t.cpu()
    return t.view(torch.int64).numpy().copy() if t.dtype == torch.float64 else t.numpy().copy()


def same(got, exp, what):
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        np.testing.assert_array_equal(bits(g), bits(e), err_msg=f"{what}: output {i}")


def refused(exc, call, *words):
    with pytest.raises(exc) as ei:
        call()
    for w in words:
        assert w in str(ei.value), str(ei.value)


# ---- the BM25 / temporal / tenant world --------------------------------------------------------------------------------------
class HybridWorld:
    def __init__(self):
        from optimized_rag_amd import RagEngine
        from optimized_rag_amd.bm25 import Bm25Postings
        from optimized_rag_amd.sharded import ShardedHybridIndex
        w = L.world()
        self.w = w
        rng = np.random.default_rng(77)
        self.mirror = Bm25Postings(w["indptr"].copy(), w["doc"].copy(), w["tf"].copy(), w["doc_len"].copy(), w["idf"].copy(), w["avgdl"],
                                   vocab={f"w{t}": t for t in range(L.N_TERMS)})
        # the rows that will be inserted: embeddings near existing ones, texts over the old vocabulary and the new terms
        n_new = sum(BLOCKS)
        self.new_emb = (w["emb"][rng.integers(0, L.N, n_new)] + 0.5 * rng.standard_normal((n_new, L.D))).astype(np.float32)
        self.new_ten = rng.integers(0, 3, n_new).astype(np.int32)
        self.new_tmp = np.where(rng.uniform(size=n_new) < 0.4, 0.1 * rng.uniform(size=n_new), 0.0)
        texts = []
        for i in range(n_new):
            words = [f"w{int(t)}" for t in rng.choice([rng.integers(0, 5), rng.integers(5, 60), rng.integers(60, L.N_TERMS)], 1 + int(rng.integers(0, 6)))]
            if i >= BLOCKS[0] or i % 3 == 0:                       # the first block's terms are used by it and by every later block
                words += [f"n{int(j)}" for j in rng.integers(0, NEW_A, 2)]
            if i >= BLOCKS[0] + BLOCKS[1]:
                words += [f"m{int(rng.integers(0, NEW_C))}"]
            texts.append(" ".join(words))
        texts[0] = " ".join(f"n{j}" for j in range(NEW_A)) + " " + texts[0]                                # numbers them 300 .. 309 in order
        c0 = BLOCKS[0] + BLOCKS[1]
        texts[c0] = " ".join(f"m{j}" for j in range(NEW_C)) + " " + texts[c0]                              # 310 .. 314
        self.texts = texts
        # queries: the world's, and four over the new terms
        extra = [[300, 7], [305], [310, 300, 2], [312, -1]]
        terms_of = list(w["terms_of"]) + extra
        self.Q = len(terms_of)
        self.ptr = cuda(np.cumsum([0] + [len(t) for t in terms_of]).astype(np.int32))
        self.terms = cuda(np.asarray([x for t in terms_of for x in t], np.int32))
        q_emb = np.concatenate([w["q_emb"], self.new_emb[[3, BLOCKS[0] + 5, c0 + 7, 11]]]).astype(np.float32)
        self.q = cuda(q_emb)
        self.tenant_q = np.concatenate([w["tenant_q"], [-1, 1, 0, 2]]).astype(np.int32)
        # handles
        self.whole = RagEngine(dim=L.D, device=0)
        self.whole.set_option("bm25_keep_tf", 1)
        self.whole.index_load(np.ascontiguousarray(w["emb"]), ids=gid(np.arange(L.N)))
        self.mirror.load(self.whole)
        self.whole.set_temporal(w["temporal"])
        self.whole.set_tenants(w["tenants"])
        self.ix = []
        for r, (lo, hi) in enumerate(L.BOUNDS):
            e = RagEngine(dim=L.D, device=0)
            e.set_option("bm25_keep_tf", 1)
            ix = ShardedHybridIndex(e, rank=r, world=3)
            ix.load_shard(np.ascontiguousarray(w["emb"][lo:hi]), lo, self.mirror.shard(lo, hi), temporal=np.ascontiguousarray(w["temporal"][lo:hi]),
                          ids=gid(np.arange(lo, hi)))
            e.set_tenants(np.ascontiguousarray(w["tenants"][lo:hi]))
            self.ix.append(ix)
        self.agree()
        self.next_row, self.block_at, self.owners, self.live = L.N, 0, [], np.ones(L.N, bool)

    def agree(self):
        lays = [ix.local_layout() for ix in self.ix]
        for ix in self.ix:
            ix.agree_layout(lays)

    def close(self):
        for e in [self.whole] + [ix.engine for ix in self.ix]:
            e.close()

    def insert(self, b):
        n = BLOCKS[b]
        sl = slice(self.block_at, self.block_at + n)
        ids = gid(np.arange(self.next_row, self.next_row + n))
        block = self.mirror.extend(self.texts[sl])
        emb, ten, tmp = self.new_emb[sl], self.new_ten[sl], self.new_tmp[sl]
        got = [ix.insert_rows(emb, ids, tenants=ten, temporal=tmp, postings=block) for ix in self.ix]
        assert len(set(got)) == 1, got                                 # every rank computed the same owner and first row
        first = self.whole.index_insert(emb, ids=ids, tenants=ten, temporal=tmp)
        self.whole.bm25_append(block["indptr"], block["doc"], block["tf"], block["doc_len"], block["idf_new"], block["n_terms_total"])
        assert first == self.next_row
        self.next_row += n
        self.block_at += n
        self.live = np.concatenate([self.live, np.ones(n, bool)])
        self.owners.append(got[0][0])
        return got[0]

    def delete(self, ids, tenant=-1):
        n = sum(ix.delete_local(ids, tenant) for ix in self.ix)
        assert n == self.whole.index_delete(ids, tenant=tenant)
        rows = (np.asarray(ids) - 7) // 3
        rows = rows[(rows >= 0) & (rows < self.next_row)]
        if tenant < 0:
            self.live[rows] = False
        return n

    # the searches, sharded (the halves of the classes, stacked) and on the whole handle
    def sharded_dense(self, tenant):
        import torch
        W, Q = len(self.ix), self.Q
        recv = torch.empty((W, 2, Q, K), dtype=torch.int64, device="cuda")
        for r, ix in enumerate(self.ix):
            ix.engine.dense_topk_dev(self.q, K, recv[r, 0], None, recv[r, 1].view(torch.float64), tenant=tenant)
        ids, sc = torch.empty((Q, K), dtype=torch.int64, device="cuda"), torch.empty((Q, K), dtype=torch.float64, device="cuda")
        self.ix[0].engine.merge_topk_dev(recv, recv.view(torch.float64)[:, 1], ids, sc, n_lists=W, list_stride=2 * Q * K)
        return ids, sc

    def whole_dense(self, tenant):
        import torch
        ids, sc = torch.empty((self.Q, K), dtype=torch.int64, device="cuda"), torch.empty((self.Q, K), dtype=torch.float64, device="cuda")
        self.whole.dense_topk_dev(self.q, K, ids, None, sc, tenant=tenant)
        return ids, sc

    def sharded_rrf(self, tenant):
        import torch
        sends = [ix.local_lists(self.q, self.ptr, self.terms, POOL, K, tenant).clone() for ix in self.ix]
        o = self.ix[1].fuse_gathered(torch.stack(sends), K)
        return o["keys"], o["rrf"], o["ranks"]

    def sharded_linear(self, tenant):
        import torch
        W, Q = len(self.ix), self.Q
        mx = torch.empty((W, Q), dtype=torch.float64, device="cuda")
        parts = torch.empty((W, 5, Q, K), dtype=torch.int64, device="cuda")
        for r, ix in enumerate(self.ix):
            ix.engine.hybrid_linear_begin_dev(self.ptr, self.terms, mx[r], tenant=tenant)
        for r, ix in enumerate(self.ix):
            ix.engine.hybrid_linear_finish_dev(self.q, mx, K, *L.WEIGHTS, parts[r], tenant=tenant)
        o = dict(ids=torch.empty((Q, K), dtype=torch.int64, device="cuda"),
                 **{n: torch.empty((Q, K), dtype=torch.float64, device="cuda") for n in L.NAMES[1:]})
        self.ix[2].engine.hybrid_linear_merge_gathered_dev(parts, *(o[n] for n in L.NAMES))
        return [o[n] for n in L.NAMES]

    def check(self, what):
        import torch
        for tenant in (-1, 1, self.tenant_q):
            tag = f"{what}, tenant {'per query' if isinstance(tenant, np.ndarray) else tenant}"
            same(self.sharded_dense(tenant), self.whole_dense(tenant), f"search, {tag}")
            same(self.sharded_rrf(tenant), self.whole.hybrid_rrf_dev(self.q, self.ptr, self.terms, POOL, K, tenant=tenant), f"search_hybrid, {tag}")
            exp = self.whole.hybrid_linear_dev(self.q, self.ptr, self.terms, K, *L.WEIGHTS, tenant=tenant)
            same(self.sharded_linear(tenant), [exp[n] for n in L.NAMES], f"search_linear, {tag}")
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def hw():
    h = HybridWorld()
    yield h
    h.close()


def planned_owners(bounds, blocks):
    """the owners the policy gives the blocks, from the layout alone"""
    from optimized_rag_amd.sharded import ShardedDenseIndex
    rows, owners = [hi - lo for lo, hi in bounds], []
    for n in blocks:
        o = ShardedDenseIndex.owner_of(rows)
        rows[o] += n
        owners.append(o)
    return owners


def test_preconditions_of_the_sequences(hw, mw):
    """what the two sequences below rely on, asserted before they run (the heads that the deletes remove are taken from the
    lists as they stand at that point, and asserted there)"""
    # each rank owns one of the first three blocks, in both worlds
    assert planned_owners(L.BOUNDS, BLOCKS[:3]) == [2, 0, 1]
    assert planned_owners(M3_BOUNDS, [hi - lo for lo, hi in M3_BLOCKS[:3]]) == [2, 0, 1]
    # the last shard is shorter than the pool and than k
    assert L.BOUNDS[2][1] - L.BOUNDS[2][0] < K < POOL and M3_BOUNDS[2][1] - M3_BOUNDS[2][0] < K
    # an exact dense tie spans two shards: the rows are copies of each other, and the whole handle lists them lower id first
    a, b = L.TIE
    assert L.BOUNDS[0][0] <= a < L.BOUNDS[0][1] <= b < L.BOUNDS[1][1] and np.array_equal(hw.w["emb"][a], hw.w["emb"][b])
    ids0, sc0 = hw.whole_dense(-1)
    assert bits(ids0)[2, :2].tolist() == gid(L.TIE).tolist() and bits(sc0)[2, 0] == bits(sc0)[2, 1]
    # a BM25 term that block 0 introduces (owner: rank 2) is used by block 1 (owner: rank 0, whose handle will not know it) and
    # asked for by a query
    first_new = {f"n{j}" for j in range(NEW_A)}
    assert first_new <= set(" ".join(hw.texts[:BLOCKS[0]]).split())
    assert first_new & set(" ".join(hw.texts[BLOCKS[0]:BLOCKS[0] + BLOCKS[1]]).split())
    assert not first_new & set(hw.mirror.vocab) and 300 in hw.terms.cpu().numpy()
    # bge-m3: the corpus has the rows of every block, and every block brings postings and token vectors
    assert M3_BLOCKS[-1][1] <= F.N_A
    for lo, hi in M3_BLOCKS:
        assert mw.lexical(np.arange(lo, hi)).nnz > 0 and mw.vecs(lo, hi)[1][-1] > 0


def test_hybrid_shards_through_the_whole_sequence(hw):
    """three inserts with three owners, deletes on every shard, a compaction of one shard, a fourth insert, a statistics refresh:
    after each step search / search_hybrid / search_linear equal the whole handle, for scalar and per-query tenants"""
    from optimized_rag_amd.sharded import ShardedDenseIndex
    hw.check("as loaded")
    for b in range(3):
        rows = [ix.engine.n_rows for ix in hw.ix]
        owner, first = hw.insert(b)
        assert owner == ShardedDenseIndex.owner_of(rows) == (2, 0, 1)[b] and first == rows[owner]
        assert [ix.engine.n_rows for ix in hw.ix] == [r + (BLOCKS[b] if i == owner else 0) for i, r in enumerate(rows)]
        for ix in hw.ix:                                              # inserted through the map: ids resolve on their owner only
            info = ix.engine.index_id_map_info()
            assert info["enabled"] == 1 and info["ids_ascending"] == 1 and info["entries"] == ix.engine.n_rows
        hw.check(f"after insert {b}")
    # a term of block 0 (owned by rank 2) was needed by block 1 on rank 0, whose handle had never seen it
    assert sorted(hw.owners) == [0, 1, 2]
    assert "n0" in hw.texts[0] and any("n" in t for t in hw.texts[BLOCKS[0]:BLOCKS[0] + BLOCKS[1]])
    assert hw.ix[0].engine.bm25_segment_stats()["n_terms"] == L.N_TERMS + NEW_A
    assert hw.ix[1].engine.bm25_segment_stats()["n_terms"] == L.N_TERMS + NEW_A + NEW_C
    # deletes on every shard, old rows and inserted ones; the head of a dense list and of a BM25 list among them
    d_ids, _ = hw.whole_dense(-1)
    bm25_of = lambda: hw.whole.bm25_topk(hw.ptr.cpu().numpy(), hw.terms.cpu().numpy(), K)[0]
    head_dense, head_bm25 = int(bits(d_ids)[5, 0]), int(bm25_of()[9, 0])
    assert head_dense >= 0 and head_bm25 >= 0
    victims = np.unique(np.concatenate([gid([3, 50, 2099, 2100, 2200, 4590, 4594, 4599, L.N + 1, L.N + 2400, L.N + 2600, L.N + 2990]),
                                        gid(np.arange(1000, 1400)), [head_dense, head_bm25, 5, 8, -1]]))
    n = hw.delete(victims)
    assert n == len(victims) - 3                                      # 5, 8 and -1 are nobody's id
    for ix in hw.ix:
        info = ix.engine.index_id_map_info()
        assert info["tombstones"] > 0 and info["entries"] + info["tombstones"] == ix.engine.n_rows
    assert head_dense not in bits(hw.whole_dense(-1)[0])[5] and head_bm25 not in bm25_of()[9]
    hw.check("after the deletes")
    assert hw.delete(gid([60, 61, 62]), tenant=0) == 1                # rows 60 .. 62 are tenants 0, 1, 2
    hw.check("after a delete under a tenant")
    # a compaction of shard 0 only
    before = hw.ix[0].engine.n_rows
    row_map = hw.ix[0].compact_local()
    assert (row_map < 0).sum() == before - hw.ix[0].engine.n_rows > 400
    hw.agree()
    info = hw.ix[0].engine.index_id_map_info()
    assert (info["tombstones"], info["rebuilds"] >= 1, info["ids_ascending"]) == (0, True, 1)
    hw.check("after compacting shard 0")
    rows = [ix.engine.n_rows for ix in hw.ix]
    owner, first = hw.insert(3)
    assert owner == ShardedDenseIndex.owner_of(rows) == rows.index(min(rows)) and first == rows[owner]
    hw.check("after insert 3")
    # statistics over every shard's live documents == rag_bm25_refresh on the whole handle
    stats = [ix.local_statistics() for ix in hw.ix]
    got = [ix.apply_statistics(stats) for ix in hw.ix]
    idf, info = hw.whole.bm25_refresh(0.25)
    for g_idf, g_avgdl in got:
        np.testing.assert_array_equal(g_idf.view(np.int64), idf.view(np.int64))
        assert g_avgdl == info["avgdl_after"]
    assert info["idf_max_abs_change"] > 0
    hw.check("after the statistics refresh")


def test_hybrid_shard_refusals_leave_the_handles_usable(hw):
    from optimized_rag_amd import RagError
    ix = hw.ix[1]
    emb = hw.new_emb[:2]
    top = ix.layout()["max_id"]
    rows = [x.engine.n_rows for x in hw.ix]
    refused(ValueError, lambda: ix.insert_rows(emb, [top, top + 1], tenants=[0, 0], temporal=[0.0, 0.0], postings=None), "above the largest id")
    refused(ValueError, lambda: ix.insert_rows(emb, [top + 9, top + 8], tenants=[0, 0], temporal=[0.0, 0.0], postings=None), "ascending")
    refused(ValueError, lambda: ix.insert_rows(emb, [top + 8, top + 9], tenants=[0, 0], temporal=[0.0, 0.0], postings=None), "postings are required")
    refused(ValueError, lambda: ix.load_shard(emb, 0, ids=[5, 5]), "ascending")
    assert [x.engine.n_rows for x in hw.ix] == rows and ix.layout()["max_id"] == top
    # the gate of the shard entries: without the map, today's refusal; with ids that do not ascend, the one that says so
    e = hw.ix[2].engine
    import torch
    mx = torch.empty((hw.Q,), dtype=torch.float64, device="cuda")
    part = torch.empty((4, hw.Q, POOL), dtype=torch.int64, device="cuda")
    cand = torch.full((hw.Q, POOL), -1, dtype=torch.int64, device="cuda")
    ids = gid(np.arange(e.n_rows)) + 10 ** 9
    e.index_id_map(False)
    refused(RagError, lambda: e.hybrid_linear_begin_dev(hw.ptr, hw.terms, mx), "(-3)", "the index has explicit ids; a row shard is loaded with id_base")
    refused(RagError, lambda: e.m3_score_ids_dev(cand, part, q_emb=hw.q, w=(1.0, 0.0, 0.0)), "(-3)", "the index has explicit ids; a row shard is loaded with id_base")
    e.index_id_map(True)
    e.hybrid_linear_begin_dev(hw.ptr, hw.terms, mx)
    cur = np.array([i for i in range(e.n_rows)], dtype=np.int64)
    real = np.empty(e.n_rows, dtype=np.int64)
    # read the shard's ids back through the map's inverse: ask for every id of the corpus
    asked = gid(np.arange(hw.next_row))
    r = e.rows_of_ids(asked)
    real[r[r >= 0]] = asked[r >= 0]
    assert (r >= 0).sum() == e.n_rows - e.index_deleted_rows()
    live = np.zeros(e.n_rows, bool)
    live[r[r >= 0]] = True
    real[~live] = 10 ** 12 + cur[~live]                                # deleted rows: any unused ids
    bad = real.copy()
    a, b = np.nonzero(live)[0][:2]
    bad[a], bad[b] = real[b], real[a]
    e.set_ids(bad)
    assert e.index_id_map_info()["ids_ascending"] == 0
    refused(RagError, lambda: e.hybrid_linear_begin_dev(hw.ptr, hw.terms, mx), "(-3)", "ascend")
    refused(RagError, lambda: e.m3_score_ids_dev(cand, part, q_emb=hw.q, w=(1.0, 0.0, 0.0)), "(-3)", "ascend")
    e.set_ids(real)
    assert e.index_id_map_info()["ids_ascending"] == 1
    hw.check("after the refusals")


# ---- the learned-sparse / token-vector world ---------------------------------------------------------------------------------
N0 = 6000                                      # rows loaded; rows [N0, N0 + 3910) of corpus A arrive as four blocks
M3_BOUNDS = ((0, 2800), (2800, 5992), (5992, N0))
M3_BLOCKS = ((N0, N0 + 3300), (N0 + 3300, N0 + 3750), (N0 + 3750, N0 + 3850), (N0 + 3850, N0 + 3910))      # owners 2, 0, 1, then the compacted shard


class M3World:
    def __init__(self):
        from optimized_rag_amd import RagEngine
        from optimized_rag_amd.sharded import ShardedM3Index
        from optimized_rag_amd.sparse import LexicalPostings
        self.w, self.a = F.world(), F.corpus_a()
        w, a = self.w, self.a
        self.emb = np.array(w["emb"])
        self.ptr, self.terms, self.wts = (cuda(x) for x in a["packed"])
        self.q, self.qv, self.qo = cuda(w["q_emb"]), cuda(w["qv"]), cuda(w["qo"])
        self.Q = self.q.shape[0]
        self.tenant_q = (np.arange(self.Q) % 4 - 1).astype(np.int32)

        def lexical(rows):
            ip, doc, wt = F.csr_of_rows(np.asarray(rows))
            return LexicalPostings(ip, doc, wt, len(rows))

        self.lexical = lexical
        self.vecs = lambda lo, hi: (np.array(w["d_vecs"][w["d_off"][lo]:w["d_off"][hi]]), (w["d_off"][lo:hi + 1] - w["d_off"][lo]).astype(np.int64))
        spare = (M3_BLOCKS[-1][1] - N0, int(w["d_off"][M3_BLOCKS[-1][1]] - w["d_off"][N0]))
        self.whole = RagEngine(dim=F.DIM, device=0)
        ShardedM3Index(self.whole, rank=0, world=1).load_shard(self.emb[:N0], 0, lexical(np.arange(N0)), *self.vecs(0, N0), ids=gid(np.arange(N0)),
                                                             token_reserve=spare)
        self.whole.set_tenants(np.ascontiguousarray(w["tenants"][:N0]))
        self.ix = []
        for r, (lo, hi) in enumerate(M3_BOUNDS):
            e = RagEngine(dim=F.DIM, device=0)
            ix = ShardedM3Index(e, rank=r, world=3)
            ix.load_shard(self.emb[lo:hi], lo, lexical(np.arange(lo, hi)), *self.vecs(lo, hi), ids=gid(np.arange(lo, hi)), token_reserve=spare)
            e.set_tenants(np.ascontiguousarray(w["tenants"][lo:hi]))
            self.ix.append(ix)
        self.agree()

    agree = HybridWorld.agree
    close = HybridWorld.close

    def insert(self, b, owner=None, device=False):
        """device: the shards get the lexical block doc-major in CUDA tensors (the layout of lexical_compact_dev, rag_sparse_append_dev)"""
        lo, hi = M3_BLOCKS[b]
        rows = np.arange(lo, hi)
        ten = np.ascontiguousarray(self.w["tenants"][lo:hi])
        block = self.lexical(rows)
        lex = dict(indptr=block.indptr, doc=block.doc, weight=block.weight, n_docs=hi - lo, n_terms_total=F.V_A)
        tv, off = self.vecs(lo, hi)
        given = lex
        if device:
            term_of = np.repeat(np.arange(F.V_A, dtype=np.int64), np.diff(block.indptr))
            order = np.lexsort((term_of, block.doc))
            ptr = np.zeros(hi - lo + 1, dtype=np.int64)
            np.cumsum(np.bincount(block.doc, minlength=hi - lo), out=ptr[1:])
            given = (cuda(ptr.astype(np.int32)), cuda(term_of[order].astype(np.int32)), cuda(block.weight[order]), F.V_A)
        got = [ix.insert_rows(self.emb[lo:hi], gid(rows), tenants=ten, owner=owner, lexical=given, token_vecs=tv, token_off=off) for ix in self.ix]
        assert len(set(got)) == 1, got
        self.whole.index_insert(self.emb[lo:hi], ids=gid(rows), tenants=ten)
        self.whole.sparse_append(lex["indptr"], lex["doc"], lex["weight"], hi - lo, F.V_A)
        self.whole.tokvec_append(tv, off)
        return got[0]

    def delete(self, ids):
        n = sum(ix.delete_local(ids) for ix in self.ix)
        assert n == self.whole.index_delete(ids)
        return n

    def sharded_m3(self, mode, wgt, tenant):
        import torch
        sends = [ix.local_lists(self.q, self.ptr, self.terms, self.wts, POOL, K, mode=mode, tenant=tenant).clone() for ix in self.ix]
        recv = torch.stack(sends)
        cands = [ix.candidates_gathered(recv, K, mode=mode).clone() for ix in self.ix]
        for c in cands[1:]:
            assert torch.equal(c, cands[0])
        parts = [ix.score_local(cands[0], self.q, self.ptr, self.terms, self.wts, self.qv, self.qo, POOL, K, w=wgt).clone() for ix in self.ix]
        o = self.ix[1].combine_gathered(cands[0], torch.stack(parts), POOL, K, w=wgt)
        return o["ids"], o["scores"], o["components"], o["candidates"]

    def sharded_lexical(self, tenant):
        import torch
        W, Q = len(self.ix), self.Q
        recv = torch.empty((W, 2, Q, K), dtype=torch.int64, device="cuda")
        for r, ix in enumerate(self.ix):
            ix.engine.sparse_topk_dev(self.ptr, self.terms, self.wts, K, recv[r, 0], None, recv[r, 1].view(torch.float64), tenant=tenant)
        ids, sc = torch.empty((Q, K), dtype=torch.int64, device="cuda"), torch.empty((Q, K), dtype=torch.float64, device="cuda")
        self.ix[0].engine.merge_topk_dev(recv, recv.view(torch.float64)[:, 1], ids, sc, n_lists=W, list_stride=2 * Q * K)
        return ids, sc

    def whole_lexical(self, tenant):
        import torch
        ids, sc = torch.empty((self.Q, K), dtype=torch.int64, device="cuda"), torch.empty((self.Q, K), dtype=torch.float64, device="cuda")
        self.whole.sparse_topk_dev(self.ptr, self.terms, self.wts, K, ids, None, sc, tenant=tenant)
        return ids, sc

    def check(self, what):
        import torch
        kw = dict(term_ptr=self.ptr, terms=self.terms, weights=self.wts, q_vecs=self.qv, q_off=self.qo)
        for tenant in (-1, self.tenant_q):
            tag = f"{what}, tenant {'per query' if isinstance(tenant, np.ndarray) else tenant}"
            for mode in (1, 2):
                exp = self.whole.retrieve_m3_dev(self.q, POOL, K, mode=mode, tenant=tenant, **kw)
                same(self.sharded_m3(mode, (0.4, 0.2, 0.4), tenant), exp, f"search_m3 mode {mode}, {tag}")
            ids, sc, cand = self.whole.retrieve_maxsim_dev(self.q, self.qv, self.qo, POOL, K, term_ptr=self.ptr, terms=self.terms, weights=self.wts, tenant=tenant)
            got = self.sharded_m3(1, (0.0, 0.0, 1.0), tenant)
            same((got[0], got[1], got[3]), (ids, sc, cand), f"search_late_interaction, {tag}")
            same(self.sharded_lexical(tenant), self.whole_lexical(tenant), f"search_lexical, {tag}")
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def mw():
    m = M3World()
    yield m
    m.close()


def test_m3_shards_through_the_whole_sequence(mw):
    """search_m3 (modes 1 and 2), search_late_interaction and search_lexical after every step of: three inserts with three owners
    (the third as a device block), deletes on every shard, a compaction of one shard, a fourth insert that lands on the compacted
    shard. Ownership of a candidate is the id map's answer."""
    import torch
    from optimized_rag_amd.sharded import ShardedDenseIndex
    mw.check("as loaded")
    owners = []
    for b in range(3):
        rows = [ix.engine.n_rows for ix in mw.ix]
        owner, first = mw.insert(b, device=b == 2)
        assert owner == ShardedDenseIndex.owner_of(rows) == (2, 0, 1)[b] and first == rows[owner]
        assert [ix.engine.n_rows for ix in mw.ix] == [r + (M3_BLOCKS[b][1] - M3_BLOCKS[b][0] if i == owner else 0) for i, r in enumerate(rows)]
        for ix in mw.ix:
            info = ix.engine.index_id_map_info()
            assert info["enabled"] == 1 and info["ids_ascending"] == 1 and info["entries"] == ix.engine.n_rows
        owners.append(owner)
        mw.check(f"after insert {b}")
    assert sorted(owners) == [0, 1, 2]
    # every rank resolves the ids of its own block and of no other
    for b, owner in enumerate(owners):
        blk = gid(np.arange(*M3_BLOCKS[b]))
        for r, ix in enumerate(mw.ix):
            got = ix.engine.rows_of_ids(blk)
            assert (got >= 0).all() if r == owner else (got < 0).all()
    # deletes on every shard, old rows and rows of every block; the head of a dense list and of a sparse list among them
    d_ids = torch.empty((mw.Q, K), dtype=torch.int64, device="cuda")
    d_sc = torch.empty((mw.Q, K), dtype=torch.float64, device="cuda")
    mw.whole.dense_topk_dev(mw.q, K, d_ids, None, d_sc)
    head_dense, head_sparse = int(bits(d_ids)[6, 0]), int(bits(mw.whole_lexical(-1)[0])[4, 0])
    assert head_dense >= 0 and head_sparse >= 0
    victims = np.unique(np.concatenate([gid([0, 17, 2799, 2800, 4000, 5989, 5990, 5999, N0 + 5, N0 + 3400, N0 + 3800]), gid(np.arange(3000, 3300)),
                                        [head_dense, head_sparse]]))
    assert mw.delete(victims) == len(victims)
    mw.whole.dense_topk_dev(mw.q, K, d_ids, None, d_sc)
    assert head_dense not in bits(d_ids)[6] and head_sparse not in bits(mw.whole_lexical(-1)[0])[4]
    mw.check("after the deletes")
    # a compaction of shard 1 only, which then has the fewest rows: the fourth block is appended to the compacted shard
    before = mw.ix[1].engine.n_rows
    row_map = mw.ix[1].compact_local()
    assert (row_map < 0).sum() == before - mw.ix[1].engine.n_rows >= 300
    mw.agree()
    info = mw.ix[1].engine.index_id_map_info()
    assert (info["tombstones"], info["rebuilds"] >= 1, info["ids_ascending"]) == (0, True, 1)
    mw.check("after compacting shard 1")
    rows = [ix.engine.n_rows for ix in mw.ix]
    owner, first = mw.insert(3)
    assert owner == ShardedDenseIndex.owner_of(rows) == 1 and first == rows[1]
    assert (mw.ix[1].engine.rows_of_ids(gid(np.arange(*M3_BLOCKS[3]))) == first + np.arange(M3_BLOCKS[3][1] - M3_BLOCKS[3][0])).all()
    mw.check("after insert 3")
