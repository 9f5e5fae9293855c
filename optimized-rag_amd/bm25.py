"""Host-side BM25 index builder: text -> term-major CSR postings + rank-bm25's float64 idf table.

Tokeniser and statistics follow the reference call site /root/reference/rag/retrieval.py:324-347
(`doc.lower().split()`, BM25Okapi defaults k1=1.5, b=0.75, epsilon=0.25). Scoring runs on the GPU
(csrc/bm25.hip) through rag_bm25_load_host / rag_bm25_topk_host / rag_bm25_scores_host.
"""
import math

import numpy as np

K1, B, EPSILON = 1.5, 0.75, 0.25


def tokenize(text):
    return text.lower().split()


class Bm25Postings:
    """CSR postings (term-major, docs ascending) + idf. Terms are numbered in first-appearance order, which is
    the dict order rank-bm25 sums idf in (the float64 mean depends on that order)."""

    def __init__(self, indptr, doc, tf, doc_len, idf, avgdl, vocab=None, k1=K1, b=B, epsilon=EPSILON):
        self.indptr, self.doc, self.tf, self.doc_len, self.idf = indptr, doc, tf, doc_len, idf
        self.avgdl, self.vocab, self.k1, self.b, self.epsilon = avgdl, vocab, k1, b, epsilon
        # mean of the idf table as built (sequential float64 sum): what a negative idf of a term that arrives LATER is replaced
        # with (extend), so that it does not depend on how the later documents were split into blocks
        self._frozen_mean = float(np.cumsum(idf)[-1]) / idf.shape[0] if idf.shape[0] else 0.0

    @property
    def n_docs(self):
        return int(self.doc_len.shape[0])

    @staticmethod
    def idf_table(df, n_docs, epsilon=EPSILON):
        """idf = ln(N-df+0.5) - ln(df+0.5); negatives replaced by epsilon * mean(idf) (sequential float64 sum).
        Every logarithm is `math.log` of a half-integer <= N + 0.5 (numpy's log is not guaranteed to round like libm's), so
        for a small corpus with a large vocabulary (the ad-hoc per-call index) the N + 1 possible values are tabulated once
        instead of two calls per term; the mean is the left-to-right running sum (`np.cumsum`), as `sum += idf` is."""
        df = np.asarray(df, dtype=np.int64)
        if df.size == 0:
            return np.zeros(0, dtype=np.float64)
        n_docs = int(n_docs)
        if 0 <= int(df.min()) and int(df.max()) <= n_docs and n_docs + 1 <= 2 * df.size:
            half_log = np.array([math.log(j + 0.5) for j in range(n_docs + 1)], dtype=np.float64)
            idf = half_log[n_docs - df] - half_log[df]
        else:           # large corpus: one pair of logarithms per DISTINCT document frequency (millions of terms share a few thousand)
            udf, inv = np.unique(df, return_inverse=True)
            idf = np.array([math.log(n_docs - int(d) + 0.5) - math.log(int(d) + 0.5) for d in udf], dtype=np.float64)[inv]
        avg = float(np.cumsum(idf)[-1]) / idf.size
        return np.where(idf < 0, epsilon * avg, idf)

    @classmethod
    def from_corpus(cls, corpus, k1=K1, b=B, epsilon=EPSILON):
        """Tokenise and build the CSR. Term numbers are assigned in first-appearance order (dict lookups only, no per-posting Python objects); the
        (term, doc) -> tf counting, the doc-ascending order inside a posting list and the offsets are one sort of the packed
        (term, doc) keys (the ad-hoc `hybrid_search` path builds an index per call: 100 passages of 200 tokens took 27 ms
        with per-posting Python loops, 5 ms this way)."""
        n = len(corpus)
        vocab, ids = {}, []
        doc_len = np.zeros(n, dtype=np.int32)
        for di, text in enumerate(corpus):
            toks = tokenize(text)
            doc_len[di] = len(toks)
            for w in toks:
                if w not in vocab:
                    vocab[w] = len(vocab)
            ids.extend(map(vocab.__getitem__, toks))
        V = len(vocab)
        term_of_tok = np.asarray(ids, dtype=np.int64)
        doc_of_tok = np.repeat(np.arange(n, dtype=np.int64), doc_len)
        key, tf = np.unique(term_of_tok * max(n, 1) + doc_of_tok, return_counts=True)     # sorted: term-major, docs ascending
        indptr = np.zeros(V + 1, dtype=np.int64)
        np.cumsum(np.bincount(key // max(n, 1), minlength=V), out=indptr[1:])
        doc = (key % max(n, 1)).astype(np.int32)
        avgdl = int(doc_len.sum()) / n if n else 0.0
        idf = cls.idf_table(np.diff(indptr), n, epsilon) if V else np.zeros(0)
        return cls(indptr, doc, tf.astype(np.int32), doc_len, idf, avgdl, vocab, k1, b, epsilon)

    # ---- appendable postings: the host mirror of rag_bm25_append_host -----------------------------------------------------
    def extend(self, texts):
        """Add documents after the existing ones. The mirror (indptr / doc / tf / doc_len / vocab) becomes exactly what
        `from_corpus(old + texts)` builds; the STATISTICS stay frozen, as they do on the device: `idf[:V_old]` and `avgdl` keep
        their values, a term first seen here gets ln(N - df + 0.5) - ln(df + 0.5) with N and df as they stand after this block
        (a negative value: epsilon * the mean of the table as built) and keeps it from then on. `refreshed()` gives the
        statistics a rebuild would. Returns the block `append_to` / `RagEngine.bm25_append` takes: the CSR of the new documents
        alone over the grown vocabulary, doc numbers relative to the block."""
        if self.vocab is None:
            raise ValueError("extend needs the vocabulary (postings built by from_corpus)")
        n_old, nb, V_old = self.n_docs, len(texts), len(self.vocab)
        vocab, ids = self.vocab, []
        bl = np.zeros(nb, dtype=np.int32)
        for di, text in enumerate(texts):
            toks = tokenize(text)
            bl[di] = len(toks)
            for w in toks:
                if w not in vocab:
                    vocab[w] = len(vocab)
            ids.extend(map(vocab.__getitem__, toks))
        V = len(vocab)
        term_of_tok = np.asarray(ids, dtype=np.int64)
        doc_of_tok = np.repeat(np.arange(nb, dtype=np.int64), bl)
        key, btf = np.unique(term_of_tok * max(nb, 1) + doc_of_tok, return_counts=True)
        bterm = key // max(nb, 1)
        bptr = np.zeros(V + 1, dtype=np.int64)
        np.cumsum(np.bincount(bterm, minlength=V), out=bptr[1:])
        bdoc = (key % max(nb, 1)).astype(np.int32)
        btf = btf.astype(np.int32)
        # merged mirror: every term's old list, then its new postings (the new documents have the larger numbers)
        odf = np.zeros(V, dtype=np.int64)
        odf[:V_old] = np.diff(self.indptr)
        bdf = np.diff(bptr)
        indptr = np.zeros(V + 1, dtype=np.int64)
        np.cumsum(odf + bdf, out=indptr[1:])
        nnz_o, nnz_b = int(self.indptr[-1]), int(bptr[-1])
        oterm = np.repeat(np.arange(V_old, dtype=np.int64), odf[:V_old])
        opos = indptr[oterm] + (np.arange(nnz_o, dtype=np.int64) - self.indptr[oterm])
        bpos = indptr[bterm] + odf[bterm] + (np.arange(nnz_b, dtype=np.int64) - bptr[bterm])
        doc = np.empty(nnz_o + nnz_b, dtype=np.int32)
        tf = np.empty(nnz_o + nnz_b, dtype=np.int32)
        doc[opos], tf[opos] = self.doc, self.tf
        doc[bpos], tf[bpos] = bdoc + np.int32(n_old), btf
        n = n_old + nb
        df_new = (odf + bdf)[V_old:]
        idf_new = np.array([math.log(n - int(d) + 0.5) - math.log(int(d) + 0.5) for d in df_new], dtype=np.float64)
        idf_new = np.where(idf_new < 0, self.epsilon * self._frozen_mean, idf_new)
        self.indptr, self.doc, self.tf = indptr, doc, tf
        self.doc_len = np.concatenate([self.doc_len, bl])
        self.idf = np.concatenate([self.idf, idf_new])
        return {"indptr": bptr, "doc": bdoc, "tf": btf, "doc_len": bl, "idf_new": idf_new, "n_terms_total": V}

    def append_to(self, engine, block):
        """Hand a block `extend` returned to the engine (after the rows themselves were inserted, or on a standalone BM25 handle)."""
        engine.bm25_append(block["indptr"], block["doc"], block["tf"], block["doc_len"], block["idf_new"], block["n_terms_total"])
        return self

    def compacted(self, row_map):
        """The host mirror of `RagEngine.index_compact(keep_postings=True)` (rag_index_compact_bm25), in place: row_map[old
        document] = its new number, or < 0 for a document that was deleted. Drops the postings and `doc_len` entries of the
        deleted documents and renumbers the rest; term numbers, `vocab`, `idf` and `avgdl` stay (frozen statistics: a term that
        loses every posting keeps its number and its idf, with an empty list). A compaction keeps the live rows in order, so the
        live entries of the map must be exactly 0 .. n_live-1 ascending; anything else, or a map of another length than
        `n_docs`, raises ValueError. Returns self."""
        row_map = np.asarray(row_map, dtype=np.int64)
        if row_map.shape != (self.n_docs,):
            raise ValueError(f"compacted: row_map must have one entry per document ({self.n_docs}), got shape {row_map.shape}")
        live = row_map >= 0
        n_live = int(live.sum())
        if not np.array_equal(row_map[live], np.arange(n_live, dtype=np.int64)):
            raise ValueError("compacted: the live entries of row_map must be 0 .. n_live-1 in ascending order")
        keep = live[self.doc]
        before = np.zeros(keep.shape[0] + 1, dtype=np.int64)      # survivors before each posting: the new offsets, read at the old
        np.cumsum(keep, out=before[1:])
        self.indptr = before[self.indptr]
        self.doc = row_map[self.doc[keep]].astype(np.int32)
        self.tf = self.tf[keep]
        self.doc_len = self.doc_len[live]
        return self

    def refreshed(self, epsilon=None):
        """A new object over the same (merged) CSR with idf / avgdl recomputed: what `from_corpus` over all texts gives."""
        eps = self.epsilon if epsilon is None else epsilon
        n = self.n_docs
        avgdl = int(self.doc_len.sum()) / n if n else 0.0
        idf = self.idf_table(np.diff(self.indptr), n, eps) if self.indptr.shape[0] > 1 else np.zeros(0)
        return Bm25Postings(self.indptr.copy(), self.doc.copy(), self.tf.copy(), self.doc_len.copy(), idf, avgdl, dict(self.vocab) if self.vocab is not None else None,
                            self.k1, self.b, eps)

    def refresh(self, live=None):
        """The host mirror of rag_bm25_refresh, in place: idf / avgdl over the documents where `live` is true (all by default),
        term numbers unchanged. For every term with df >= 1, ln(N - df + 0.5) - ln(df + 0.5) (`math.log`); mean = their
        left-to-right float64 sum in term-number order over their count, negative values included; every negative value becomes
        epsilon * mean. A term that lost every posting keeps its number, gets ln(N + 0.5) - ln(0.5) and stays out of the mean.
        This is `idf_table` restricted to the terms that still occur. `_frozen_mean` becomes the new mean, so a later `extend`
        floors the negative idf of a new term by it. Returns self."""
        n_all = self.n_docs
        live = np.ones(n_all, dtype=bool) if live is None else np.asarray(live, dtype=bool)
        if live.shape != (n_all,):
            raise ValueError(f"refresh: live must have one entry per document ({n_all}), got shape {live.shape}")
        n = int(live.sum())
        if n == 0:
            raise ValueError("refresh: no live document")
        V = self.indptr.shape[0] - 1
        term_of = np.repeat(np.arange(V, dtype=np.int64), np.diff(self.indptr))
        df = np.bincount(term_of[live[self.doc]], minlength=V).astype(np.int64)
        self.idf, self._frozen_mean = self.idf_of_counts(df, n, self.epsilon)
        self.avgdl = int(self.doc_len[live].sum()) / n
        return self

    @staticmethod
    def idf_of_counts(df, n_docs, epsilon=EPSILON):
        """The idf rule of `refresh` / rag_bm25_refresh from document frequencies alone (row shards sum theirs: sharded.py
        ShardedHybridIndex.refresh_statistics): df int64 [terms] over n_docs live documents -> (idf float64 [terms], mean)."""
        df = np.asarray(df, dtype=np.int64)
        n = int(n_docs)
        occ = df > 0
        udf, inv = np.unique(df, return_inverse=True)
        idf = np.array([math.log(n - int(d) + 0.5) - math.log(int(d) + 0.5) for d in udf], dtype=np.float64)[inv.reshape(-1)] \
            if df.size else np.zeros(0, dtype=np.float64)
        mean = float(np.cumsum(idf[occ])[-1]) / int(occ.sum()) if occ.any() else 0.0
        return np.where(occ & (idf < 0), epsilon * mean, idf), mean

    def refresh_on(self, engine, live=None):
        """`RagEngine.bm25_refresh` on the device and `refresh` on this mirror; the two idf tables must agree bit for bit.
        `live`: the documents the engine has not deleted (the mirror does not know the engine's deletes). Returns self."""
        idf, info = engine.bm25_refresh(self.epsilon)
        self.refresh(live)
        if not (np.array_equal(idf.view(np.int64), self.idf.view(np.int64)) and info["avgdl_after"] == self.avgdl):
            raise AssertionError("refresh_on: the engine's statistics differ from the host mirror's")
        return self

    def drift(self):
        """How far the frozen statistics are from what a rebuild would compute: lets a caller decide when to reload."""
        fresh = self.refreshed()
        d = np.abs(fresh.idf - self.idf)
        return {"avgdl_frozen": float(self.avgdl), "avgdl_true": float(fresh.avgdl),
                "idf_max_abs_change": float(d.max()) if d.size else 0.0}

    def shard(self, begin, end):
        """Doc-partitioned slice [begin, end) for row-sharded search: postings of the shard's docs
        with LOCAL doc numbers, the GLOBAL idf table / avgdl / vocabulary replicated (BM25 statistics are corpus-wide)."""
        counts = np.diff(self.indptr)
        term_of = np.repeat(np.arange(counts.shape[0], dtype=np.int64), counts)
        keep = (self.doc >= begin) & (self.doc < end)
        indptr = np.zeros(counts.shape[0] + 1, dtype=np.int64)
        np.cumsum(np.bincount(term_of[keep], minlength=counts.shape[0]), out=indptr[1:])
        return Bm25Postings(indptr, (self.doc[keep] - begin).astype(np.int32), self.tf[keep].copy(),
                            self.doc_len[begin:end].copy(), self.idf, self.avgdl, self.vocab, self.k1, self.b)

    def encode_queries(self, queries):
        """List[str] -> (term_ptr int32 [Q+1], terms int32) with repeats kept and -1 for unknown tokens."""
        ptr, terms = [0], []
        for q in queries:
            for w in tokenize(q):
                terms.append(self.vocab.get(w, -1))
            ptr.append(len(terms))
        return np.asarray(ptr, dtype=np.int32), np.asarray(terms, dtype=np.int32)

    def load(self, engine):
        engine.bm25_load(self.indptr, self.doc, self.tf, self.doc_len, self.idf, self.avgdl, self.k1, self.b)
        return self
