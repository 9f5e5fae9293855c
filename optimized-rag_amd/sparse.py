"""Host-side builder of the learned-sparse inverted index: {token id: weight} maps -> term-major CSR postings.

A learned-sparse model (bge-m3's lexical head through `LocalEmbeddingService.encode_multi`, SPLADE, anything that gives a
{token id: weight} map per text) scores a (query, document) pair as the sum over their shared token ids of the product of the two
weights. The semantics are restated from FlagEmbedding / SPLADE practice; parity with those upstream implementations is not
pinned by a test. Scoring runs on the GPU (csrc/bm25.hip, the learned-sparse form) through rag_sparse_load_host /
rag_sparse_topk_* / rag_hybrid_sparse_rrf_dev; this module is the counterpart of bm25.Bm25Postings for that index.
"""
import numpy as np


def _flatten(maps):
    """List of {token id: weight} -> (owner int64, token int64, weight float32), entries in map order."""
    owner, tok, w = [], [], []
    for i, m in enumerate(maps):
        owner.extend([i] * len(m))
        tok.extend(int(k) for k in m.keys())
        w.extend(float(v) for v in m.values())
    return np.asarray(owner, dtype=np.int64), np.asarray(tok, dtype=np.int64), np.asarray(w, dtype=np.float64).astype(np.float32)


class LexicalPostings:
    """CSR postings (term-major, docs strictly ascending inside a term) of float32 weights > 0. A term number is the model's
    token id, so queries need no vocabulary lookup."""

    def __init__(self, indptr, doc, weight, n_docs):
        self.indptr, self.doc, self.weight, self._n_docs = indptr, doc, weight, int(n_docs)

    @property
    def n_docs(self):
        return self._n_docs

    @property
    def n_terms(self):
        return int(self.indptr.shape[0] - 1)

    @property
    def nnz(self):
        return int(self.doc.shape[0])

    @classmethod
    def from_weights(cls, maps, n_terms=None):
        """maps[d] = {token id: weight} of document d. Weights become float32; an entry whose float32 weight is not > 0 is left
        out (it could add nothing), a weight that is not finite as float32 or a token id outside [0, n_terms) raises ValueError. n_terms defaults
        to the largest token id + 1."""
        n = len(maps)
        if n < 1:
            raise ValueError("from_weights: at least one document")
        owner, tok, w = _flatten(maps)
        if not np.isfinite(w).all():
            raise ValueError("from_weights: non-finite weight")
        keep = w > 0
        owner, tok, w = owner[keep], tok[keep], w[keep]
        V = int(n_terms) if n_terms is not None else (int(tok.max()) + 1 if tok.size else 1)
        if V < 1 or (tok.size and (int(tok.min()) < 0 or int(tok.max()) >= V)):
            raise ValueError(f"from_weights: token ids must lie in [0, {V})")
        key = tok * n + owner
        order = np.argsort(key, kind="stable")             # term-major, documents ascending
        key = key[order]
        if key.size > 1 and not (np.diff(key) > 0).all():
            raise ValueError("from_weights: a token id occurs twice in one document's map")
        indptr = np.zeros(V + 1, dtype=np.int64)
        np.cumsum(np.bincount(tok, minlength=V), out=indptr[1:])
        return cls(indptr, (key % n).astype(np.int32), np.ascontiguousarray(w[order]), n)

    @staticmethod
    def doc_major(maps, n_terms=None):
        """The same maps as a DOC-MAJOR block: (ptr int32 [n + 1] from 0, terms int32 ascending inside a document, weights
        float32) - the layout rag_lexical_compact_dev writes and `RagEngine.sparse_append_docs` takes. from_weights' rules: an
        entry whose float32 weight is not > 0 is left out, a weight that is not finite or a token id outside [0, n_terms) raises
        ValueError, as does a token id that occurs twice in one map. n_terms defaults to the largest token id + 1."""
        n = len(maps)
        if n < 1:
            raise ValueError("doc_major: at least one document")
        owner, tok, w = _flatten(maps)
        if not np.isfinite(w).all():
            raise ValueError("doc_major: non-finite weight")
        keep = w > 0
        owner, tok, w = owner[keep], tok[keep], w[keep]
        V = int(n_terms) if n_terms is not None else (int(tok.max()) + 1 if tok.size else 1)
        if V < 1 or (tok.size and (int(tok.min()) < 0 or int(tok.max()) >= V)):
            raise ValueError(f"doc_major: token ids must lie in [0, {V})")
        order = np.lexsort((tok, owner))                   # document-major, terms ascending
        key = (owner * V + tok)[order]
        if key.size > 1 and not (np.diff(key) > 0).all():
            raise ValueError("doc_major: a token id occurs twice in one document's map")
        if key.size >= 2**31:
            raise ValueError("doc_major: the block's offsets must fit int32")
        ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(owner, minlength=n), out=ptr[1:])
        return ptr.astype(np.int32), tok[order].astype(np.int32), np.ascontiguousarray(w[order])

    @classmethod
    def from_texts(cls, service, texts, batch=256, n_terms=None):
        """Lexical weights of `texts` from the service's lexical head (`encode_multi`, `batch` texts per call), then from_weights.
        n_terms defaults to the model's vocabulary size."""
        maps = []
        for b in range(0, len(texts), batch):
            out = service.encode_multi(texts[b:b + batch], return_dense=False, return_sparse=True, return_colbert_vecs=False)
            maps.extend(out["lexical_weights"])
        if n_terms is None:
            n_terms = getattr(service, "cfg", {}).get("vocab_size")
        return cls.from_weights(maps, n_terms)

    @staticmethod
    def encode_queries(maps):
        """List of {token id: weight} -> (term_ptr int32 [Q + 1], terms int32, weights float32). Each query's terms come in
        ASCENDING token id: the score is a float64 sum in query-token order, so this fixes its bits. Nothing is filtered: a
        token outside the vocabulary or with a weight that is not > 0 adds nothing on the device."""
        owner, tok, w = _flatten(maps)
        order = np.lexsort((tok, owner))
        ptr = np.zeros(len(maps) + 1, dtype=np.int64)
        np.cumsum(np.bincount(owner, minlength=len(maps)), out=ptr[1:])
        if tok.size and (int(tok.min()) < -2**31 or int(tok.max()) >= 2**31):
            raise ValueError("encode_queries: token ids must fit int32")
        return ptr.astype(np.int32), tok[order].astype(np.int32), np.ascontiguousarray(w[order])

    def shard(self, begin, end):
        """Doc-partitioned slice [begin, end) with LOCAL document numbers. Raw scores need no corpus-wide statistic: merging the
        shards' top-k lists (rag_merge_topk_dev over global ids) reproduces the unsharded list."""
        counts = np.diff(self.indptr)
        term_of = np.repeat(np.arange(counts.shape[0], dtype=np.int64), counts)
        keep = (self.doc >= begin) & (self.doc < end)
        indptr = np.zeros(counts.shape[0] + 1, dtype=np.int64)
        np.cumsum(np.bincount(term_of[keep], minlength=counts.shape[0]), out=indptr[1:])
        return LexicalPostings(indptr, (self.doc[keep] - begin).astype(np.int32), self.weight[keep].copy(), end - begin)

    def load(self, engine):
        engine.sparse_load(self.indptr, self.doc, self.weight, self.n_docs)
        return self

    # ---- live writes: the counterparts of Bm25Postings.extend / append_to / compacted ---------------------------------------
    def extend(self, maps_or_postings, n_terms=None):
        """Add documents after the existing ones: a list of {token id: weight} maps, or a LexicalPostings of the new documents
        alone (document numbers relative to the block). The mirror becomes what `from_weights(old maps + new maps)` builds over
        the grown vocabulary - every term's old list, then its new postings. n_terms: the vocabulary after the block (default:
        the larger of the mirror's and the block's); it may not shrink. Returns the relative block `append_to` /
        `RagEngine.sparse_append` takes."""
        block = maps_or_postings
        if not isinstance(block, LexicalPostings):
            block = LexicalPostings.from_weights(block, n_terms)
        V_old, nb = self.n_terms, block.n_docs
        V = max(V_old, block.n_terms) if n_terms is None else int(n_terms)
        if V < V_old or V < block.n_terms:
            raise ValueError(f"extend: n_terms may not shrink ({V} < {max(V_old, block.n_terms)})")
        odf = np.zeros(V, dtype=np.int64)
        odf[:V_old] = np.diff(self.indptr)
        bdf = np.zeros(V, dtype=np.int64)
        bdf[:block.n_terms] = np.diff(block.indptr)
        bptr = np.zeros(V + 1, dtype=np.int64)
        np.cumsum(bdf, out=bptr[1:])
        indptr = np.zeros(V + 1, dtype=np.int64)
        np.cumsum(odf + bdf, out=indptr[1:])
        nnz_o, nnz_b = self.nnz, block.nnz
        oterm = np.repeat(np.arange(V, dtype=np.int64), odf)
        bterm = np.repeat(np.arange(V, dtype=np.int64), bdf)
        opos = indptr[oterm] + (np.arange(nnz_o, dtype=np.int64) - self.indptr[oterm]) if nnz_o else np.zeros(0, dtype=np.int64)
        bpos = indptr[bterm] + odf[bterm] + (np.arange(nnz_b, dtype=np.int64) - bptr[bterm])
        doc = np.empty(nnz_o + nnz_b, dtype=np.int32)
        weight = np.empty(nnz_o + nnz_b, dtype=np.float32)
        doc[opos], weight[opos] = self.doc, self.weight
        doc[bpos], weight[bpos] = block.doc + np.int32(self._n_docs), block.weight
        self.indptr, self.doc, self.weight = indptr, doc, weight
        self._n_docs += nb
        return {"indptr": bptr, "doc": block.doc, "weight": block.weight, "n_docs": nb, "n_terms_total": V}

    def append_to(self, engine, block):
        """Hand a block `extend` returned to the engine (after the rows themselves were inserted, or on a handle without a
        dense index)."""
        engine.sparse_append(block["indptr"], block["doc"], block["weight"], block["n_docs"], block["n_terms_total"])
        return self

    def compacted(self, row_map):
        """The host mirror of `RagEngine.index_compact(keep_resident=True)` (rag_index_compact_live), in place: row_map[old
        document] = its new number, or < 0 for a document that was deleted. Drops the postings of the deleted documents and
        renumbers the rest; term numbers stay (a term that loses every posting keeps its number, with an empty list). The live
        entries of the map must be exactly 0 .. n_live-1 ascending; anything else, or a map of another length than `n_docs`,
        raises ValueError. Returns self."""
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
        self.weight = np.ascontiguousarray(self.weight[keep])
        self._n_docs = n_live
        return self


class ResidentLexical:
    """Stand-in for the LexicalPostings mirror of an index whose postings were built on the device
    (GpuDocumentIndex.build_lexical): it holds the two counts live writes are checked against - documents covered and terms
    known - and no posting. `export` reads the postings back when a host copy is wanted (to save them, or to `shard` them)."""

    def __init__(self, n_docs, n_terms):
        self.n_docs, self.n_terms = int(n_docs), int(n_terms)

    def appended(self, n_docs_new, n_terms_total):
        """Counts after a block of n_docs_new documents over n_terms_total terms was appended on the device. Returns self."""
        if int(n_terms_total) < self.n_terms:
            raise ValueError(f"appended: n_terms may not shrink ({int(n_terms_total)} < {self.n_terms})")
        self.n_docs += int(n_docs_new)
        self.n_terms = int(n_terms_total)
        return self

    def compacted(self, row_map):
        """The counts after `RagEngine.index_compact(keep_resident=True)`: LexicalPostings.compacted's checks of the row map,
        then n_docs = the live rows; term numbers stay. Returns self."""
        row_map = np.asarray(row_map, dtype=np.int64)
        if row_map.shape != (self.n_docs,):
            raise ValueError(f"compacted: row_map must have one entry per document ({self.n_docs}), got shape {row_map.shape}")
        live = row_map >= 0
        n_live = int(live.sum())
        if not np.array_equal(row_map[live], np.arange(n_live, dtype=np.int64)):
            raise ValueError("compacted: the live entries of row_map must be 0 .. n_live-1 in ascending order")
        self.n_docs = n_live
        return self

    def export(self, engine):
        """The resident postings as a LexicalPostings (rag_sparse_export_host): base and tail merged per term."""
        e = engine.sparse_export()
        return LexicalPostings(e["indptr"], e["doc"], e["weight"], e["n_docs"])
