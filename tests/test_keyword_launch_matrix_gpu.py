"""GPU: the whole dispatch table of the keyword scoring launch in one place (csrc/bm25.hip: bm25_range_kernel and the launch path
around it). Four axes, every combination:
  postings  impact (doc, float64 impact) | packed (option bm25_packed; a packed base with its tail in the impact form) | learned-sparse
  tenant    none | one for the launch | one per query
  segments  base only (three 2048-document ranges: an exact first stage and a thresholded one) | base + appended tail (the tail
            starts inside the base's last range and owns a range of its own)
  entry     top-k host | top-k device | all-document scores host | BM25: the device scores call of the linear fusion
            (hybrid_linear_begin_dev: the largest raw score per query under its tenant)
with bm25_plan_slots = 2 and bm25_first_ranges = 1, five queries (no token, only unknown tokens, more tokens than plan slots,
an ordinary one, one rare term) and k below and above the number of matching documents.
Every result is held bit for bit (ids, rows, float64 scores) against the CSR oracle of the neighbouring tests
(oracle.rag_oracle.bm25_scores_csr, tests/sparse_tools.py), and the base + tail handle against the handle that loaded the merged
postings in one piece. No tolerance anywhere."""
import numpy as np
import pytest

import sparse_tools as S
from oracle import rag_oracle as O

pytestmark = pytest.mark.gpu

N, N0, DIM, ID_BASE = 5000, 3000, 32, 1000
KS = (3, 100)
OPTS = (("bm25_plan_slots", 2), ("bm25_first_ranges", 1), ("bm25_tail_fold", -1), ("sparse_tail_fold", -1))
QUERY_TENANTS = np.array([0, 2, -1, 1, 5], dtype=np.int32)              # 5 owns no row
_W = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def queries_over(df, rng):
    """the five queries as term numbers, from the document frequencies of the merged postings"""
    V = df.shape[0]
    by_df = np.argsort(-df, kind="stable")
    rare = int(np.nonzero((df >= 4) & (df < KS[1]))[0][0])
    assert df[by_df[60]] > KS[0]
    qs = [[], [-1, V + 3], [int(by_df[i]) for i in (3, 40, 3, 120, 7)], [int(by_df[10]), int(by_df[60])], [rare]]
    ptr = np.concatenate([[0], np.cumsum([len(q) for q in qs])]).astype(np.int32)
    terms = np.asarray([t for q in qs for t in q], dtype=np.int32)
    return qs, ptr, terms, (rng.random(terms.shape[0]) * 2.0).astype(np.float32) + np.float32(1e-3)


def block_of(indptr, doc, w, lo, hi):
    """the postings of the documents [lo, hi), renumbered from 0"""
    keep = (doc >= lo) & (doc < hi)
    term_of = np.repeat(np.arange(indptr.shape[0] - 1, dtype=np.int64), np.diff(indptr))
    out = np.zeros_like(indptr)
    np.cumsum(np.bincount(term_of[keep], minlength=indptr.shape[0] - 1), out=out[1:])
    return out, (doc[keep] - lo).astype(np.int32), w[keep].copy()


class World:
    """two handles over the same N rows - `whole` loaded in one piece, `live` as N0 rows + an appended block - the raw float64
    score of every (query, document) from the oracle, and the tenant of every row"""

    def __init__(self, form):
        from optimized_rag_amd import RagEngine
        rng = np.random.default_rng(41)
        self.form, self.sparse = form, form == "sparse"
        emb = rng.standard_normal((N, DIM)).astype(np.float32)
        self.ten = rng.integers(0, 3, N).astype(np.int32)
        self.whole, self.live = RagEngine(dim=DIM, device=0), RagEngine(dim=DIM, device=0)
        for e in (self.whole, self.live):
            for name, v in OPTS + (("bm25_packed", int(form == "packed")),):
                e.set_option(name, v)
        self.whole.index_load(emb, id_base=ID_BASE)
        self.whole.set_tenants(self.ten)
        self.live.index_load(emb[:N0], id_base=ID_BASE)
        self.live.set_tenants(self.ten[:N0])
        self.live.index_insert(emb[N0:], tenants=self.ten[N0:])
        if self.sparse:
            ip, doc, w = S.make_corpus(N, 1600, seed=5)
            self.whole.sparse_load(ip, doc, w, N)
            self.live.sparse_load(*S.cut(ip, doc, w, N0), N0)
            self.live.sparse_append(*block_of(ip, doc, w, N0, N), N - N0)
            self.qs, self.ptr, self.terms, self.qw = queries_over(np.diff(ip), rng)
            self.raw = S.all_scores(ip, doc, w, N, [(q, self.qw[self.ptr[i]:self.ptr[i + 1]]) for i, q in enumerate(self.qs)])
            seg = self.live.sparse_segment_stats()
        else:
            from optimized_rag_amd.bm25 import Bm25Postings
            lens = rng.poisson(8, N)
            toks = (rng.zipf(1.2, int(lens.sum())) - 1) % 300
            at = np.concatenate([[0], np.cumsum(lens)])
            texts = [" ".join(f"t{t}" for t in toks[at[i]:at[i + 1]]) for i in range(N)]
            p = Bm25Postings.from_corpus(texts[:N0]).load(self.live)
            p.append_to(self.live, p.extend(texts[N0:]))
            p.load(self.whole)                                           # the merged postings under the same frozen statistics
            self.qs, self.ptr, self.terms, self.qw = queries_over(np.diff(p.indptr), rng)
            self.raw = np.stack([O.bm25_scores_csr(p.indptr, p.doc, p.tf, p.doc_len, p.idf, p.avgdl, q) for q in self.qs])
            seg = self.live.bm25_segment_stats()
        assert seg["base_docs"] == N0 and seg["tail_docs"] == N - N0 and seg["folds"] == 0
        self.raw.setflags(write=False)

    def close(self):
        self.whole.close()
        self.live.close()

    def rows_of(self, tenant):
        return np.nonzero(self.ten == tenant)[0] if tenant >= 0 else np.arange(N)

    def expect_topk(self, k, tq):
        """rows (-1 padded), scores and - BM25 - the divisor of every query under its tenant"""
        rows = np.full((len(self.qs), k), -1, dtype=np.int32)
        sc = np.zeros((len(self.qs), k))
        mx = np.ones(len(self.qs))
        for qi, t in enumerate(tq):
            mine = self.rows_of(int(t))
            raw = self.raw[qi][mine]
            if self.sparse:
                hidden = np.ones(N, dtype=bool)
                hidden[mine] = False
                rows[qi], sc[qi] = S.topk(self.raw[qi], k, hidden)
            elif len(mine):
                mx[qi] = raw.max() if raw.max() > 0 else 1.0
                top = O.stable_topk_desc(raw, k)
                rows[qi, :len(top)], sc[qi, :len(top)] = mine[top], raw[top] / mx[qi]
        return rows, sc, mx

    def topk(self, eng, k, tenant, dev):
        """(ids, rows, scores[, raw_max]) of the five queries through the host or the device entry"""
        import torch
        Q = len(self.qs)
        if not dev:
            return (eng.sparse_topk(self.ptr, self.terms, self.qw, k, tenant=tenant) if self.sparse
                    else eng.bm25_topk(self.ptr, self.terms, k, tenant=tenant))
        o = [torch.empty((Q, k), dtype=torch.int64, device="cuda"), torch.empty((Q, k), dtype=torch.int32, device="cuda"),
             torch.empty((Q, k), dtype=torch.float64, device="cuda")]
        pd, td = torch.from_numpy(self.ptr).cuda(), torch.from_numpy(self.terms).cuda()
        if self.sparse:
            eng.sparse_topk_dev(pd, td, torch.from_numpy(self.qw).cuda(), k, *o, tenant=tenant)
        else:
            o.append(torch.empty((Q,), dtype=torch.float64, device="cuda"))
            eng.bm25_topk_dev(pd, td, k, o[0], o[1], o[2], raw_max_out=o[3], tenant=tenant)
        torch.cuda.synchronize()
        return tuple(x.cpu().numpy() for x in o)

    def scores(self, eng):
        return eng.sparse_scores(self.ptr, self.terms, self.qw) if self.sparse else eng.bm25_scores(self.ptr, self.terms)

    def local_max(self, eng, tenant):
        import torch
        out = torch.empty((len(self.qs),), dtype=torch.float64, device="cuda")
        eng.hybrid_linear_begin_dev(torch.from_numpy(self.ptr).cuda(), torch.from_numpy(self.terms).cuda(), out, tenant=tenant)
        torch.cuda.synchronize()
        return out.cpu().numpy()


@pytest.fixture(scope="module")
def worlds():
    def get(form):
        if form not in _W:
            _W[form] = World(form)
        return _W[form]

    yield get
    for w in _W.values():
        w.close()
    _W.clear()


@pytest.mark.parametrize("tenants", ["none", "launch", "per_query"])
@pytest.mark.parametrize("form", ["impact", "packed", "sparse"])
def test_every_launch_of_the_matrix(worlds, form, tenants):
    w = worlds(form)
    Q = len(w.qs)
    tenant = {"none": -1, "launch": 1, "per_query": QUERY_TENANTS}[tenants]
    tq = np.broadcast_to(np.asarray(tenant, dtype=np.int32), (Q,))
    for k in KS:
        rows, sc, mx = w.expect_topk(k, tq)
        owned = np.array([len(w.rows_of(int(t))) > 0 for t in tq])         # (a tenant without rows: no divisor to speak of)
        ids = np.where(rows >= 0, rows.astype(np.int64) + ID_BASE, -1)
        for seg, eng in (("base", w.whole), ("base+tail", w.live)):
            for dev in (False, True):
                got = w.topk(eng, k, tenant, dev)
                what = f"{form}, tenant {tenants}, {seg}, k={k}, {'device' if dev else 'host'}"
                np.testing.assert_array_equal(got[1], rows, err_msg=what)
                np.testing.assert_array_equal(got[0], ids, err_msg=what)
                np.testing.assert_array_equal(bits(got[2]), bits(sc), err_msg=what)
                if not w.sparse:
                    np.testing.assert_array_equal(bits(got[3][owned]), bits(mx[owned]), err_msg=what)
    if not w.sparse:                                                      # the device scores call of the linear fusion
        want = np.array([w.raw[qi][w.rows_of(int(t))].max() if len(w.rows_of(int(t))) else -np.inf for qi, t in enumerate(tq)])
        for seg, eng in (("base", w.whole), ("base+tail", w.live)):
            np.testing.assert_array_equal(bits(w.local_max(eng, tenant)), bits(want), err_msg=f"{form}, tenant {tenants}, {seg}")
    if tenants == "none":                                                 # all-document scores: the host entry takes no tenant
        for seg, eng in (("base", w.whole), ("base+tail", w.live)):
            np.testing.assert_array_equal(bits(w.scores(eng)), bits(w.raw), err_msg=f"{form}, {seg}")
