"""The same batch before and after the index changes: no answer depends on what the handle held or answered before.

Handle `e` answers a batch at state A (both with a tenant and without), is written to, and answers again at state B. The second
answer is compared bit for bit with a handle `f` loaded directly at state B and never called before (one per tenant argument:
within its batch the seven entries follow each other on `f` as they do on `e`), and with the CPU oracles
of the neighbouring tests under their bars (dense: ids exact, 1e-9, tests/test_live_index_gpu.py; BM25: exact; RRF: keys and
ranks exact, 1e-12; linear fusion: rows exact, 1e-12, tests/test_stream_order_gpu.py; rerank: candidates exact, sigmoid 1e-3,
logits 4e-3, tests/test_pipeline_gpu.py; three-way score: dense 1e-9, sparse bits, score (wc / sum) * 1e-4 + 1e-9,
tests/test_m3_fused_gpu.py). At the end the A batch on a fresh A-state handle must equal what `e` answered at A, so that two
equal wrong answers cannot pass.

What `e` carries over from A are the grow-only workspaces of the handle (tests/test_workspace_table_cpu.py), carved at B by
other sizes. The sharpest case is lin_ws (api.hip linear_carve): it is laid out by the row count, raw [256][n] float64 then raw32
[256][ld] float32, and zero-filled only when it grows. When a SMALLER index is loaded on the handle (rag_index_load: it leaves
lin_ws alone) the float32 plane starts inside what was the float64 plane, and its pad rows [n, next multiple of 256), which the
last tile of the fused emission reads, hold halves of old float64 BM25 scores:
test_the_pad_rows_of_raw32_hold_non_finite_words_after_the_replacement shows on the CPU that these words include Inf / NaN at the
shapes used here, so a pass of shrink_by_replacement means the emission masks rows >= n_rows, not that the bytes were harmless.
The shrink by COMPACTION cannot show this, and neither can an insert: every live write that changes the row count frees lin_ws
(live.hip live_rows_changed, called by compact_publish and by the insert), so the next linear call allocates it anew and
zero-fills it. Those transitions carry over the other workspaces only.

Measured on an MI355X, one run (also in DESIGN.md section 4.7): 8 of the 21,120 pad words after the replacement are not finite;
every comparison held on the library as it stood, so the library is unchanged. The 9 tests take 5 s behind a started process,
none above 2.1 s in the whole suite (the first test of a process that loads a cross-encoder also pays the runtime's one-time
load of its kernels: 12 s when this file runs alone).
"""
import numpy as np
import pytest

from oracle import bert_oracle as B
from oracle import rag_oracle as O
import m3_fused_tools as F
import m3_tools as M
import sparse_tools as S
import stream_tools as T
import test_stream_order_gpu as A
import tokvec_tools as V

pytestmark = pytest.mark.gpu

D, TOK, VS = 64, 64, 1600
NP, NA, NB = 8600, 6000, 1060             # rows of the pool, of state A, live rows after the shrink (1060 = 4 * 256 + 36: 220 pad rows)
QL, QS, QR = 96, 24, 4                    # queries of the linear calls, of the other searches, of the rerank
POOL, K, RPOOL, RK, LP = 20, 10, 8, 4, 32
ABG = (0.5, 0.3, 0.2)                     # alpha, beta, gamma (gamma != 0: the temporal plane is read)
W3 = (0.4, 0.2, 0.4)
TENANTS = (1, -1)                         # in this order: the last writer of lin_ws in a state is the unfiltered batch
QB = 256                                  # api.hip linear_batch at these row counts
_W = {}


def world():
    if _W:
        return _W
    rng = np.random.default_rng(6464)
    w = {}
    w["emb"] = rng.standard_normal((NP, D)).astype(np.float32)
    w["ids"] = (7000 + 3 * np.arange(NP)).astype(np.int64)
    w["ten"] = rng.integers(0, 3, NP).astype(np.int32)
    w["tmp"] = rng.random(NP)
    docs = [rng.integers(0, 400, int(n)) for n in rng.integers(6, 19, NP)]        # 6 to 18 words: the BM25 scores take many values
    w["texts"] = [" ".join(f"t{t}" for t in d) for d in docs]
    w["q"] = (w["emb"][rng.integers(0, NP, QL)] + 0.4 * rng.standard_normal((QL, D))).astype(np.float32)
    w["queries"] = [" ".join([f"t{t}" for t in docs[int(rng.integers(0, NP))]][:11] + ["zzz"]) for _ in range(QL)]
    w["csr"] = S.make_corpus(n_docs=NP, n_terms=VS, seed=9)
    sq = [(rng.choice(VS - S.N_EMPTY, int(n), replace=False), (rng.random(int(n)) * 2.0).astype(np.float32) + np.float32(1e-3))
          for n in rng.integers(1, 9, QS)]
    sq[5] = (np.zeros(0, np.int32), np.zeros(0, np.float32))
    w["sq"] = sq
    counts = rng.integers(1, 9, NP)
    w["d_vecs"] = V.unit_rows(rng, int(counts.sum()), TOK)
    w["d_off"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    qc = rng.integers(1, 13, QS)
    qc[3] = 0
    w["qlist"] = [V.unit_rows(rng, int(c), TOK) for c in qc]
    w["tok"] = rng.integers(200, 2000, (NP, 20)).astype(np.int32)
    w["tok_len"] = rng.integers(3, 21, NP).astype(np.int32)
    w["q_tok"] = rng.integers(200, 2000, (QR, 6)).astype(np.int32)
    w["q_len"] = rng.integers(1, 7, QR).astype(np.int32)
    w["ce_w"] = B.seeded_weights(A.CE_CFG, 11)
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    w["ce_t"] = flatten_state_dict(w["ce_w"], A.CE_CFG["layers"])
    _W.update(w)
    return _W


def tv_of(rows):
    """(vectors, offsets) of the token-vector documents of the pool rows `rows`"""
    w = world()
    off = w["d_off"]
    n = off[rows + 1] - off[rows]
    idx = np.concatenate([np.arange(off[r], off[r + 1]) for r in rows]) if len(rows) else np.zeros(0, np.int64)
    return np.ascontiguousarray(w["d_vecs"][idx]), np.concatenate([[0], np.cumsum(n)]).astype(np.int64)


class State:
    """The host mirror of what a handle holds, in the handle's row space: src[row] = the pool row, live[row], the keyword and the
    learned-sparse postings as the library's own mirrors keep them (frozen statistics through extend and compacted)."""

    def __init__(self, lo, hi):
        from optimized_rag_amd.bm25 import Bm25Postings
        from optimized_rag_amd.sparse import LexicalPostings
        w = world()
        self.src = np.arange(lo, hi)
        self.live = np.ones(hi - lo, bool)
        self.post = Bm25Postings.from_corpus(w["texts"][lo:hi])
        self.lex = LexicalPostings(*w["csr"], NP).shard(lo, hi)

    def delete(self, eng, rows):
        assert eng.index_delete(world()["ids"][self.src[rows]]) == len(rows)
        self.live[rows] = False

    def compacted(self, row_map):
        np.testing.assert_array_equal(row_map >= 0, self.live)
        self.post.compacted(row_map)
        self.lex.compacted(row_map)
        self.src = self.src[self.live]
        self.live = np.ones(len(self.src), bool)

    def insert(self, eng, lo, hi):
        w = world()
        new = np.arange(lo, hi)
        first = eng.index_insert(w["emb"][new], ids=w["ids"][new], tenants=w["ten"][new], temporal=w["tmp"][new], tokens=w["tok"][new],
                                 token_lens=w["tok_len"][new])
        assert first == len(self.src)
        self.post.append_to(eng, self.post.extend(w["texts"][lo:hi]))
        from optimized_rag_amd.sparse import LexicalPostings
        self.lex.append_to(eng, self.lex.extend(LexicalPostings(*w["csr"], NP).shard(lo, hi)))
        eng.tokvec_append(*tv_of(new))
        self.src = np.concatenate([self.src, new])
        self.live = np.concatenate([self.live, np.ones(hi - lo, bool)])

    def view(self):
        """the live rows alone, as a handle loaded with them holds them: (pool rows, keyword postings, sparse postings, live rows of self)"""
        from optimized_rag_amd.bm25 import Bm25Postings
        from optimized_rag_amd.sparse import LexicalPostings
        p, x = self.post, self.lex
        post = Bm25Postings(p.indptr.copy(), p.doc.copy(), p.tf.copy(), p.doc_len.copy(), p.idf.copy(), p.avgdl, dict(p.vocab), p.k1, p.b, p.epsilon)
        lex = LexicalPostings(x.indptr.copy(), x.doc.copy(), x.weight.copy(), x.n_docs)
        lv = np.nonzero(self.live)[0]
        if len(lv) < len(self.live):
            row_map = np.where(self.live, np.cumsum(self.live) - 1, -1)
            post.compacted(row_map)
            lex.compacted(row_map)
        return self.src[lv], post, lex, lv


def load(eng, src, post, lex, reserve=0):
    """everything the entries need over the pool rows `src`; `reserve` > 0: through rag_index_reserve and an append"""
    w = world()
    if reserve:
        eng.index_reserve(reserve)
        eng.index_append(w["emb"][src])
        eng.set_ids(w["ids"][src])
    else:
        eng.index_load(w["emb"][src], ids=w["ids"][src])
    eng.index_id_map()
    eng.set_tenants(w["ten"][src])
    eng.set_temporal(w["tmp"][src])
    post.load(eng)
    lex.load(eng)
    eng.tokvec_reserve(NP, int(w["d_off"][-1]), TOK)              # headroom for every row of the pool
    eng.tokvec_append(*tv_of(src))
    eng.tokens_load(w["tok"][src], w["tok_len"][src])
    eng.ce_load(A.CE_CFG, w["ce_t"])
    return eng


@pytest.fixture
def engine():
    from optimized_rag_amd import RagEngine
    made = []

    def make(**options):
        e = RagEngine(dim=D, device=0)
        made.append(e)
        for name, value in options.items():
            e.set_option(name, value)
        return e

    yield make
    for e in made:
        e.close()


def fresh(engine, st):
    src, post, lex, lv = st.view()
    return load(engine(), src, post, lex), lv


# ---- the batch --------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("dense_topk_dev", "bm25_topk_dev", "hybrid_rrf_dev", "hybrid_linear_dev", "hybrid_linear_pair", "retrieve_rerank_dev", "retrieve_m3_dev")


def answers(eng, post, tenant, only=ENTRIES):
    """name -> (arrays in id space, rows or None) of the seven entries at one tenant argument, on the default stream"""
    import torch
    w = world()
    out, i64, i32, f64 = A.out, torch.int64, torch.int32, torch.float64
    ptr, terms = post.encode_queries(w["queries"])
    lp, lt, lw = S.pack_queries(w["sq"])
    qv, qo = M.pack(w["qlist"], TOK)
    d = T.to_dev(dict(q=w["q"], ptr=ptr, terms=terms, lp=lp, lt=lt, lw=lw, qv=qv, qo=qo, q_tok=w["q_tok"], q_len=w["q_len"]))
    q, pt = d["q"][:QS], d["ptr"][:QS + 1]
    res = {}
    if "dense_topk_dev" in only:
        ids, rows, sc = out((QS, K), i64), out((QS, K), i32), out((QS, K), f64)
        eng.dense_topk_dev(q, K, ids, rows, sc, tenant=tenant)
        res["dense_topk_dev"] = ([ids, sc], rows)
    if "bm25_topk_dev" in only:
        ids, rows, sc, mx = out((QS, K), i64), out((QS, K), i32), out((QS, K), f64), out((QS,), f64)
        eng.bm25_topk_dev(pt, d["terms"], K, ids, rows, sc, mx, tenant=tenant)
        res["bm25_topk_dev"] = ([ids, sc, mx], rows)
    if "hybrid_rrf_dev" in only:
        res["hybrid_rrf_dev"] = ([t.clone() for t in eng.hybrid_rrf_dev(q, pt, d["terms"], POOL, K, tenant=tenant)], None)
    if "hybrid_linear_dev" in only:
        o = eng.hybrid_linear_dev(d["q"], d["ptr"], d["terms"], K, *ABG, tenant=tenant)
        res["hybrid_linear_dev"] = ([o[n].clone() for n in ("ids", "hybrid", "semantic", "keyword", "temporal")], o["rows"].clone())
    if "hybrid_linear_pair" in only:
        mx, gmx = out((QL,), f64), out((1, QL), f64)
        part, gpart = out((5, QL, K), i64), out((1, 5, QL, K), i64)
        o = [out((QL, K), i64)] + [out((QL, K), f64) for _ in range(4)]
        eng.hybrid_linear_begin_dev(d["ptr"], d["terms"], mx, tenant=tenant)
        gmx[0].copy_(mx)
        eng.hybrid_linear_finish_dev(d["q"], gmx, K, *ABG, part, tenant=tenant)
        gpart[0].copy_(part)
        eng.hybrid_linear_merge_gathered_dev(gpart, *o)
        res["hybrid_linear_pair"] = (o + [mx, part], None)
    if "retrieve_rerank_dev" in only:
        r = eng.retrieve_rerank_dev(d["q"][:QR], d["q_tok"], d["q_len"], RPOOL, RK, term_ptr=d["ptr"][:QR + 1], terms=d["terms"], L_pair=LP, tenant=tenant)
        res["retrieve_rerank_dev"] = ([t.clone() for t in r], None)
    if "retrieve_m3_dev" in only:
        r = eng.retrieve_m3_dev(q, POOL, K, term_ptr=d["lp"], terms=d["lt"], weights=d["lw"], q_vecs=d["qv"], q_off=d["qo"], mode=2, w=W3, tenant=tenant)
        res["retrieve_m3_dev"] = ([t.clone() for t in r], None)
    torch.cuda.synchronize()
    return {n: ([t.cpu().numpy() for t in a], None if r is None else r.cpu().numpy()) for n, (a, r) in res.items()}


def bits(a):
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(got, exp, lv, what):
    """bit for bit; the rows of `exp` (a handle of the live rows alone) are the live rows lv of `got`'s handle"""
    assert set(got) == set(exp)
    for name in got:
        (ga, gr), (xa, xr) = got[name], exp[name]
        for i, (g, x) in enumerate(zip(ga, xa)):
            np.testing.assert_array_equal(bits(g), bits(x), err_msg=f"{what}: {name} output {i}")
        if gr is not None:
            np.testing.assert_array_equal(gr, np.where(xr >= 0, lv[np.maximum(xr, 0)], -1), err_msg=f"{what}: {name} rows")


# ---- the oracles ------------------------------------------------------------------------------------------------------------------------
def raw_scores(post, qi):
    ptr, terms = post.encode_queries([world()["queries"][qi]])
    return O.bm25_scores_csr(post.indptr, post.doc, post.tf, post.doc_len, post.idf, post.avgdl, terms.tolist())


def padded(x, n, fill):
    x = list(x)
    return x + [fill] * (n - len(x))


def against_the_oracles(st, got, tenant):
    """`got` of a handle at state st against float64 numpy over the live rows; the bars are the module docstring's"""
    w = world()
    src, post, lex, _ = st.view()
    emb, ids, ten, tmp = w["emb"][src], w["ids"][src], w["ten"][src], w["tmp"][src]
    mine = np.nonzero(ten == tenant)[0] if tenant >= 0 else np.arange(len(src))
    hidden = np.ones(len(src), bool)
    hidden[mine] = False
    cos = O.cosine_matrix(w["q"], emb[mine])                                   # [QL][mine]
    d_top = [mine[O.stable_topk_desc(cos[qi], POOL)] for qi in range(QS)]
    raws = {}

    def keyword(qi):
        if qi not in raws:
            raw = raw_scores(post, qi)
            m = raw[mine].max() if len(mine) and raw[mine].max() > 0 else 1.0
            raws[qi] = (raw, m)
        return raws[qi]

    if "dense_topk_dev" in got:
        (gid, gsc), grow = got["dense_topk_dev"]
        for qi in range(QS):
            top = d_top[qi][:K]
            np.testing.assert_array_equal(gid[qi], ids[top])
            assert np.abs(gsc[qi] - cos[qi][O.stable_topk_desc(cos[qi], K)]).max() < 1e-9
    if "bm25_topk_dev" in got:
        (gid, gsc, gmx), grow = got["bm25_topk_dev"]
        for qi in range(0, QS, 3):
            raw, m = keyword(qi)
            top = mine[O.stable_topk_desc(raw[mine], K)]
            np.testing.assert_array_equal(gid[qi], ids[top])
            np.testing.assert_array_equal(gsc[qi], raw[top] / m)
            assert gmx[qi] == m
    if "hybrid_rrf_dev" in got:
        (keys, rrf, ranks), _ = got["hybrid_rrf_dev"]
        for qi in range(0, QS, 3):
            raw, _m = keyword(qi)
            b_top = mine[O.stable_topk_desc(raw[mine], POOL)]
            ok, osc, orank = O.rrf_fuse([[int(ids[r]) for r in d_top[qi]], [int(ids[r]) for r in b_top]], k=60, top_k=K)
            assert keys[qi].tolist() == ok and ranks[qi].tolist() == orank
            np.testing.assert_allclose(rrf[qi], osc, rtol=0, atol=1e-12)
    for name in ("hybrid_linear_dev", "hybrid_linear_pair"):
        if name not in got:
            continue
        gid, hyb, sem, kw, tm = got[name][0][:5]
        for qi in range(0, QL, 7):
            raw, m = keyword(qi)
            key = raw[mine] / m
            fused = (ABG[0] * cos[qi] + ABG[1] * key) + ABG[2] * tmp[mine]
            top = O.stable_topk_desc(fused, K)
            np.testing.assert_array_equal(gid[qi], ids[mine[top]], err_msg=f"{name} query {qi}")
            for g, x in ((hyb, fused), (sem, cos[qi]), (kw, key), (tm, tmp[mine])):
                np.testing.assert_allclose(g[qi], x[top], rtol=0, atol=1e-12)
    if "retrieve_rerank_dev" in got:
        (rid, rsc, rlg, cand), _ = got["retrieve_rerank_dev"]
        tol = 1e-3
        ocand = np.full((QR, RPOOL), -1, np.int64)
        for qi in range(QR):
            raw, _m = keyword(qi)
            b_top = mine[O.stable_topk_desc(raw[mine], RPOOL)]
            keys, _, _ = O.rrf_fuse([[int(r) for r in d_top[qi][:RPOOL]], [int(r) for r in b_top]], k=60, top_k=RPOOL)
            ocand[qi, :len(keys)] = keys
        np.testing.assert_array_equal(cand, np.where(ocand >= 0, ids[np.maximum(ocand, 0)], -1))
        pid, ptt, plen = A.build_pairs(w["q_tok"], w["q_len"], ocand, w["tok"][src], w["tok_len"][src], LP)
        ologit = B.forward_logits(w["ce_w"], A.CE_CFG, pid.astype(np.int64), ptt.astype(np.int64), plen.astype(np.int64)).reshape(QR, RPOOL)
        oscore = np.array([[O.sigmoid(float(x)) for x in row] for row in ologit])
        for qi in range(QR):
            order = sorted(range(RPOOL), key=lambda j: -oscore[qi, j])
            np.testing.assert_allclose(rsc[qi], [oscore[qi, j] for j in order[:RK]], atol=tol)
            np.testing.assert_allclose(rlg[qi], [ologit[qi, j] for j in order[:RK]], atol=4 * tol)
            if np.abs(np.diff([oscore[qi, j] for j in order[:RK + 1]])).min() > 2 * tol:
                assert rid[qi].tolist() == [int(ids[ocand[qi, j]]) for j in order[:RK]]
    if "retrieve_m3_dev" in got:
        (mid, msc, comp, cand), _ = got["retrieve_m3_dev"]
        row_of = {int(i): r for r, i in enumerate(ids)}
        stored = V.fp16_round(w["d_vecs"])
        wd, ws, wc = W3
        for qi in range(QS):
            t, qw = w["sq"][qi]
            s = S.scores(lex.indptr, lex.doc, lex.weight, len(src), t, qw)
            s_rows, _ = S.topk(s, POOL, hidden)
            union = {int(ids[r]) for r in d_top[qi]} | {int(ids[r]) for r in s_rows if r >= 0}
            assert set(cand[qi][cand[qi] >= 0].tolist()) == union, f"three-way candidates of query {qi}"
            vq = w["qlist"][qi]
            for j in range(K):
                if mid[qi, j] < 0:
                    continue
                r = row_of[int(mid[qi, j])]
                dn, sp, cb = comp[qi, j]
                c64 = F.cosine64(w["q"][qi], emb[r:r + 1])[0]
                assert abs(dn - c64) < 1e-9
                assert S.bits(sp) == S.bits(s[r])
                p = int(src[r])
                ref_c = M.maxsim(vq, stored[w["d_off"][p]:w["d_off"][p + 1]]) if len(vq) else 0.0
                assert abs(msc[qi, j] - F.combine(c64, s[r], ref_c, W3)) < (wc / (wd + ws + wc)) * 1e-4 + 1e-9
                assert S.bits(msc[qi, j]) == S.bits(F.combine(dn, sp, cb, W3))


# ---- the pad rows of raw32 ----------------------------------------------------------------------------------------------------------------
def plane(n, elt):
    return -(-(n * elt) // 256) * 256


def pad_words(raw_a, n_a, n_b, ld_b):
    """The float32 words that the pad rows [n_b, next multiple of 256) of raw32 hold at state B, for the QL queries of the batch,
    when lin_ws was last written at state A with the float64 scores raw_a [QL][n_a] and has not grown since (api.hip linear_carve:
    raw [QB][n] float64 at offset 0, raw32 [QB][ld] float32 behind it, each plane rounded up to 256 B). Asserts that raw32 at B lies
    wholly inside the raw plane of A and that the pad rows read lie inside the part of it that A's QL queries wrote."""
    raw_bytes_a = QB * n_a * 8
    base = plane(QB * n_b, 8)                                       # byte offset of raw32 at B
    assert plane(QB * n_b, 8) + QB * ld_b * 4 <= raw_bytes_a, "raw32 at B does not lie inside the raw plane of A"
    rows = np.arange(n_b, -(-n_b // 256) * 256)
    assert len(rows) > 0, "n_b is a multiple of the tile: there are no pad rows"
    word = base // 4 + np.arange(QL)[:, None] * ld_b + rows[None, :]
    assert word.max() * 4 + 4 <= QL * n_a * 8, "the pad rows lie beyond what A's batch wrote"
    return np.ascontiguousarray(raw_a, dtype=np.float64).reshape(-1).view(np.float32)[word]


def raw_at_a():
    st = State(0, NA)
    return np.stack([raw_scores(st.post, qi) for qi in range(QL)])


LD_AFTER_LOAD = 2048                      # dense.hip dense_index_build pads the fp16 plane to 8 tiles: 1060 rows -> 2048


def test_the_pad_rows_of_raw32_hold_non_finite_words_after_the_replacement():
    """(numpy only) A condition on the INPUTS of shrink_by_replacement, the one transition that keeps lin_ws: 6000 rows -> 1060 by
    rag_index_load. At A raw is 256 x 6000 x 8 = 12,288,000 B. At B raw takes 256 x 1060 x 8 = 2,170,880 B and raw32 follows at that
    offset: 256 x 2048 x 4 = 2,097,152 B, ending at 4,268,032, inside the 12,288,000 B. The 220 pad rows of the 96 queries then hold
    halves of the BM25 scores that queries 45 to 61 of the batch at A left there; a low half has a random exponent, so about one in
    256 is Inf or NaN. (After a compaction or an insert there is nothing of the kind to compute: live.hip live_rows_changed frees
    lin_ws, and the next call allocates and zero-fills it.)"""
    words = pad_words(raw_at_a(), NA, NB, LD_AFTER_LOAD)
    bad = int((~np.isfinite(words)).sum())
    print(f"ld {LD_AFTER_LOAD}: {words.size} pad words, {int((words != 0).sum())} not zero, {bad} not finite")
    assert bad >= 1, "the stale pad words are all finite: change the seed of world(), shrink_by_replacement proves nothing with it"


# ---- A -> B -----------------------------------------------------------------------------------------------------------------------------
def survivors():
    return np.sort(np.random.default_rng(17).choice(NA, NB, replace=False))


def shrink_by_compaction(eng, st):
    dead = np.setdiff1d(np.arange(NA), survivors())
    st.delete(eng, dead)
    st.compacted(eng.index_compact(keep_postings=True, keep_resident=True))
    assert eng.n_rows == NB


def shrink_by_plain_compaction(eng, st):
    """rag_index_compact leaves the keyword postings, the sparse postings and the token vectors stale: they are loaded again"""
    dead = np.setdiff1d(np.arange(NA), survivors())
    st.delete(eng, dead)
    st.compacted(eng.index_compact())
    src, post, lex, _ = st.view()
    post.load(eng)
    lex.load(eng)
    eng.tokvec_reserve(NP, int(world()["d_off"][-1]), TOK)
    eng.tokvec_append(*tv_of(src))


def replace(eng, st):
    """rag_index_load of another, smaller index with its own postings, temporal scores, token store and token vectors"""
    other = State(7000, 7000 + NB)
    st.__dict__.update(other.__dict__)
    load(eng, *st.view()[:3])


def grow(eng, st):
    st.insert(eng, 3000, 5500)


def delete_then_insert(eng, st):
    st.delete(eng, np.sort(np.random.default_rng(18).choice(NA, 500, replace=False)))
    st.insert(eng, NA, NA + 700)


# name -> (rows of state A, rag_index_reserve of the first load, the writes)
TRANSITIONS = {
    "shrink_by_compaction": ((0, NA), 0, shrink_by_compaction),
    "shrink_by_plain_compaction_and_reload": ((0, NA), 0, shrink_by_plain_compaction),
    "shrink_by_replacement": ((0, NA), 0, replace),
    "grow_inside_a_reservation": ((0, 3000), 8000, grow),
    "grow_past_the_loaded_planes": ((0, 3000), 0, grow),
    "delete_without_compaction_then_insert_more": ((0, NA), 0, delete_then_insert),
}


@pytest.mark.parametrize("name", sorted(TRANSITIONS))
def test_the_batch_after_the_writes_is_that_of_a_fresh_handle(engine, name):
    """What `e` still holds of state A differs by transition. rag_index_load (shrink_by_replacement) keeps every workspace, lin_ws
    with its stale planes among them. The live writes (compactions, inserts) keep the dense set, ix->ws where the postings stay,
    pipe_ws, tv_ws, qten and the cross-encoder's workspace, but free lin_ws (live.hip live_rows_changed), so the linear entries
    then run on a newly allocated, zero-filled lin_ws, as on `f`."""
    (lo, hi), reserve, write = TRANSITIONS[name]
    st = State(lo, hi)
    e = load(engine(), *st.view()[:3], reserve=reserve)
    at_a = {t: answers(e, st.post, t) for t in TENANTS}
    write(e, st)
    at_b = {t: answers(e, st.post, t) for t in TENANTS}
    for t in TENANTS:
        f, lv = fresh(engine, st)                                   # one per tenant: f has answered nothing before its batch
        same(at_b[t], answers(f, st.view()[1], t), lv, f"{name}, state B, tenant {t}")
        against_the_oracles(st, at_b[t], t)
    st_a = State(lo, hi)
    for t in TENANTS:
        g, lv = fresh(engine, st_a)
        same(at_a[t], answers(g, st_a.post, t), lv, f"{name}, state A, tenant {t}")


# ---- option flips between two calls on one handle -------------------------------------------------------------------------------------
def test_options_flipped_between_calls_give_the_same_bits(engine):
    """bm25_plan_slots (read per call), bm25_packed (read when postings are loaded: they are loaded again) and ce_ffn_fused (0, 1, -1)
    on one handle between batches: the header promises the same bits; the first batch is also held against the oracles. (The
    attention-mode option acts on 64-wide heads above 512 tokens only: the next test.)"""
    st = State(0, 3000)
    e = load(engine(), *st.view()[:3])
    first = {t: answers(e, st.post, t) for t in TENANTS}
    for t in TENANTS:
        against_the_oracles(st, first[t], t)
    lv = np.arange(3000)
    flips = [("bm25_plan_slots", 8, False), ("bm25_packed", 1, True), ("bm25_plan_slots", 0, False), ("bm25_packed", 0, True),
             ("ce_ffn_fused", 1, False), ("ce_ffn_fused", -1, False), ("ce_ffn_fused", 0, False)]
    for option, value, reload in flips:
        e.set_option(option, value)
        if reload:
            st.post.load(e)
        only = ("retrieve_rerank_dev",) if option.startswith("ce_") else ENTRIES
        for t in TENANTS:
            got = answers(e, st.post, t, only)
            same(got, {n: first[t][n] for n in got}, lv, f"{option} = {value}, tenant {t}")


def test_the_attention_mode_flipped_between_calls_gives_the_same_bits(engine):
    """ce_attn_stream on a model with 64-wide heads (128 / 2, the default model of tests/test_long_seq_gpu.py) at the 1024-token class:
    0 (streamed where it is the default), -1 (DIRECT), 1 (streamed), 0 again, a short batch between every two long ones so that the
    workspace is carved by another shape in between. Every long result has the bits of the first and every short one those of the
    first short one; the first long one is within the 4e-3 of the logits (tests/test_long_seq_gpu.py) of the float64 oracle."""
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    cfg = dict(vocab_size=2000, hidden=128, layers=2, heads=2, ffn=512, max_pos=1024, type_vocab=2, eps=1e-12)
    wts = B.seeded_weights(cfg, 8192)
    rng = np.random.default_rng(3)

    def batch(lens, L):
        lens = np.asarray(lens, np.int32)
        ids = rng.integers(5, cfg["vocab_size"], (len(lens), L)).astype(np.int32)
        ids[np.arange(L)[None, :] >= lens[:, None]] = 0
        tt = ((np.arange(L)[None, :] >= 9) & (np.arange(L)[None, :] < lens[:, None])).astype(np.int32)
        return ids, tt, lens

    long_, short = batch([700, 40, 1000], 1024), batch([64, 3, 17, 33, 50, 64, 9, 20], 64)
    e = engine()
    e.ce_load(cfg, flatten_state_dict(wts, cfg["layers"]))
    first_long, first_short = e.ce_score(*long_), e.ce_score(*short)
    exp = B.forward_logits(wts, cfg, long_[0].astype(np.int64), long_[1].astype(np.int64), long_[2], fast_erf=True)
    assert np.abs(first_long - exp).max() < 4e-3
    for form in (-1, 1, 0):
        e.set_option("ce_attn_stream", form)
        np.testing.assert_array_equal(bits(e.ce_score(*long_)), bits(first_long), err_msg=f"ce_attn_stream = {form}")
        np.testing.assert_array_equal(bits(e.ce_score(*short)), bits(first_short), err_msg=f"the short batch after ce_attn_stream = {form}")
