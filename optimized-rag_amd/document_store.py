"""GpuDocumentIndex — the HBM-resident replacement of the pgvector tables, with `DocumentStore.search`'s surface
(/root/reference/rag/document_store.py:424-485) and `search_archival_memory`'s (database/operations.py:110-159).

`ORDER BY dc.embedding <=> %s::vector LIMIT %s` with `WHERE dc.agent_id = %s` becomes rag_dense_topk_* with a
per-row tenant filter; the exact-scan result (not the HNSW approximation) is what is reproduced. Row payloads
(content, filename, metadata) stay on the host; only embeddings live in HBM."""
import functools
import logging
import math
import threading
from typing import Any, Dict, List, Optional

import numpy as np

from .engine import get_engine

logger = logging.getLogger(__name__)


class _ShardRows:
    """List-like view of a shard's payload rows [begin, end): `rows[i]` reads one JSON line from disk."""

    def __init__(self, shard, begin, end):
        self.shard, self.begin, self.end = shard, begin, end

    def __len__(self):
        return self.end - self.begin

    def __getitem__(self, i):
        g = self.begin + int(i)
        r = self.shard.row(g)
        r["id"] = int(self.shard.ids[g])
        ts = float(self.shard.created_at[g])
        r["created_at"] = None if ts != ts else ts
        return r


class _RowView:
    """Payload rows after live writes: `base` (a list or _ShardRows) seen through `keep` (compaction), then appended rows."""

    def __init__(self, base, keep=None):
        self.base, self.keep, self.extra = base, keep, []

    def __len__(self):
        return (len(self.base) if self.keep is None else len(self.keep)) + len(self.extra)

    def __getitem__(self, i):
        n = len(self) - len(self.extra)
        i = int(i)
        if i >= n:
            return self.extra[i - n]
        return self.base[i if self.keep is None else int(self.keep[i])]

    def append(self, r):
        self.extra.append(r)


def _locked(fn):
    @functools.wraps(fn)
    def f(self, *a, **kw):
        with self._lock:
            return fn(self, *a, **kw)
    return f


def _enc_rows(enc, sel):
    """the texts `sel` of an encode_multi result"""
    return {k: None if v is None else ([v[i] for i in sel] if isinstance(v, list) else np.asarray(v)[list(sel)]) for k, v in enc.items()}


class GpuDocumentIndex:
    def __init__(self, embedding_service, dim: int = 1536, *, engine=None):
        self.embeddings = embedding_service            # same attribute name the reference's DocumentStore uses
        self.dim = dim
        self._engine = engine
        self.rows: List[Dict[str, Any]] = []
        self._tenant_id: Dict[str, int] = {}
        # live writes: one lock around writes and searches (a search sees a document's old chunk set or its new one, never a
        # mix); doc id -> row bookkeeping lives in the engine, (agent, document_id) -> chunk ids here
        self._lock = threading.RLock()
        self._next_id = 0
        self._doc_chunks: Dict[tuple, List[int]] = {}
        self._shard_without_doc_ids = False
        self._lexical = None                           # host mirror of the resident lexical postings (load_lexical), kept for live writes
        self._row_ids = np.zeros(0, dtype=np.int64)    # engine id of every row (the batched bge-m3 searches map the ids they get back)
        self._row_ids_sorted = None

    @property
    def engine(self):
        if self._engine is None:
            self._engine = get_engine(self.dim)
        return self._engine

    def bulk_load(self, rows: List[Dict[str, Any]], embeddings) -> None:
        """rows[i]: {content, agent_id, filename?, file_type?, metadata?, id?, created_at?}; embeddings [N, dim] float32
        (the export of document_chunks / archival_memory)."""
        emb = np.ascontiguousarray(embeddings, dtype=np.float32)
        assert emb.shape == (len(rows), self.dim)
        # a row without `id` carries its engine id (the row number) from here on: compaction renumbers rows, never ids
        self.rows = [r if "id" in r else dict(r, id=i) for i, r in enumerate(rows)]
        tenants = np.empty(len(rows), dtype=np.int32)
        for i, r in enumerate(rows):
            tenants[i] = self._tenant_id.setdefault(str(r.get("agent_id", "")), len(self._tenant_id))
        self.engine.index_load(emb)
        self.engine.set_tenants(tenants)
        # engine ids stay id_base + row (implicit); live writes address rows by the row's `id` where it has one
        self._doc_chunks = {}
        ids = []
        for i, r in enumerate(self.rows):
            ids.append(int(r.get("id", i)))
            if r.get("document_id") is not None:
                self._doc_chunks.setdefault((str(r.get("agent_id", "")), int(r["document_id"])), []).append(ids[-1])
        self._next_id = max(ids, default=-1) + 1
        self._set_row_ids(np.asarray(ids, dtype=np.int64))
        if any(int(r["id"]) != i for i, r in enumerate(self.rows)):
            self.engine.set_ids(np.asarray(ids, dtype=np.int64))

    def load_shard(self, shard, begin: int = 0, end: Optional[int] = None, chunk_rows: int = 131072, headroom_rows: int = 0,
                   with_tokens: bool = False) -> None:
        """Stream an exported shard directory (shard_format.py; path or open Shard) into the index: rows [begin, end),
        payloads stay on disk and are read lazily per hit, doc ids are the table's primary keys. headroom_rows reserves
        capacity for live inserts (growing a 115-GB share in place would need a second copy). with_tokens loads the shard's
        passage tokens as the resident token store (24 bits wide when its ids exceed 65535: shard_format.load_shard_into)."""
        from . import shard_format as SF
        sh = SF.open_shard(shard) if isinstance(shard, str) else shard
        end = sh.n_rows if end is None else end
        assert sh.dim == self.dim
        SF.load_shard_into(self.engine, sh, begin, end, chunk_rows, headroom_rows=headroom_rows, with_tokens=with_tokens)
        self._tenant_id = dict(sh.tenant_table)
        self.rows = _ShardRows(sh, begin, end)
        self._next_id = int(sh.ids[begin:end].max()) + 1 if end > begin else 0
        self._set_row_ids(np.array(sh.ids[begin:end], dtype=np.int64))
        self._doc_chunks = {}
        doc = getattr(sh, "document_ids", None)
        self._shard_without_doc_ids = doc is None
        if doc is not None:
            agent_of = {v: k for k, v in self._tenant_id.items()}
            for g in range(begin, end):
                if doc[g] >= 0:
                    self._doc_chunks.setdefault((agent_of[int(sh.tenants[g])], int(doc[g])), []).append(int(sh.ids[g]))

    # ---- live writes (rag_index_insert_host / rag_index_delete_host / rag_index_compact) --------------------------------
    @_locked
    def add_rows(self, rows: List[Dict[str, Any]], embeddings, *, lexical_weights=None, token_vectors=None) -> List[int]:
        """The incremental form of bulk_load: rows[i] {content, agent_id, id?, document_id?, ...} + embeddings [n, dim].
        A row without `id` gets the next one. Returns the ids; the rows are searchable on return.
        lexical_weights: one {token id: weight} map per row; when lexical postings are resident (load_lexical) the block is
        appended to them (rag_sparse_append_host) and search_lexical stays live. token_vectors: (vecs float32 [rows, tok_dim],
        offsets int64 [n + 1]), host arrays or CUDA tensors; when a token-vector store is resident the documents are appended to
        it (its reservation must have the headroom). Both happen under the same lock as the insert: a search sees all legs of
        the new rows or none. Without the arguments the behaviour is unchanged: the resident legs go stale / fall behind.
        Postings built on the device (build_lexical) have no host mirror: the maps then go as one doc-major block through
        rag_sparse_append_docs_host (LexicalPostings.doc_major; checked before anything is written, like the mirror's block)."""
        emb = np.ascontiguousarray(embeddings, dtype=np.float32).reshape(-1, self.dim)
        assert emb.shape[0] == len(rows)
        if not rows:
            return []
        lex_append = None
        if lexical_weights is not None and self._lexical is not None:
            from .sparse import LexicalPostings
            if len(lexical_weights) != len(rows):
                raise ValueError(f"add_rows: {len(lexical_weights)} lexical maps for {len(rows)} rows")
            if self._lexical.n_docs != len(self.rows):
                raise ValueError("add_rows: the lexical postings do not cover the current rows (load_lexical again)")
            top = max((int(k) for m in lexical_weights for k in m), default=-1)
            lex_terms = max(self._lexical.n_terms, top + 1)
            if self._resident_lexical():                             # either way the block is checked before anything is written
                lex_block = LexicalPostings.doc_major(lexical_weights, lex_terms)
                lex_append = lambda: (self.engine.sparse_append_docs(*lex_block, lex_terms), self._lexical.appended(len(rows), lex_terms))
            else:
                lex_block = LexicalPostings.from_weights(lexical_weights, lex_terms)
                lex_append = lambda: self._lexical.append_to(self.engine, self._lexical.extend(lex_block))
        return self._insert_rows(rows, emb, lex_append, token_vectors)

    def _insert_rows(self, rows, emb, lex_append, token_vectors) -> List[int]:
        """add_rows behind its checks of the lexical block (the caller holds the lock): the row insert, then the sparse leg
        (lex_append, or None), then the token vectors, then the payload rows."""
        store = token_vectors is not None and self.engine.tokvec_info()["dim"] > 0
        if store and self.engine.tokvec_info()["n_docs"] != len(self.rows):
            raise ValueError("add_rows: the token-vector store does not cover the current rows")
        ids = np.empty(len(rows), dtype=np.int64)
        ten = np.empty(len(rows), dtype=np.int32)
        for i, r in enumerate(rows):
            ids[i] = int(r["id"]) if r.get("id") is not None else self._next_id
            self._next_id = max(self._next_id, int(ids[i]) + 1)
            ten[i] = self._tenant_id.setdefault(str(r.get("agent_id", "")), len(self._tenant_id))
        self.engine.index_insert(emb, ids=ids, tenants=ten)
        if lex_append is not None:
            lex_append()
        if store:
            vecs, offsets = token_vectors
            if hasattr(vecs, "is_cuda"):
                self.engine.tokvec_append_dev(vecs, offsets, n_docs=len(rows))
            else:
                self.engine.tokvec_append(vecs, np.ascontiguousarray(offsets, dtype=np.int64)[:len(rows) + 1])
        if not isinstance(self.rows, (list, _RowView)):
            self.rows = _RowView(self.rows)
        self._set_row_ids(np.concatenate([self._row_ids, ids]))
        for i, r in enumerate(rows):
            r = dict(r, id=int(ids[i]))
            self.rows.append(r)
            if r.get("document_id") is not None:
                self._doc_chunks.setdefault((str(r.get("agent_id", "")), int(r["document_id"])), []).append(int(ids[i]))
        return [int(v) for v in ids]

    def _resident_lexical(self) -> bool:
        """the lexical postings were built on the device (build_lexical): a ResidentLexical stands in for the host mirror"""
        from .sparse import ResidentLexical
        return isinstance(self._lexical, ResidentLexical)

    def _delete_ids(self, agent_id, ids) -> int:
        t = self._tenant_id.get(str(agent_id))
        if t is None or not len(ids):
            return 0
        return self.engine.index_delete(np.asarray(ids, dtype=np.int64), tenant=t)

    @_locked
    def index_document_chunks(self, agent_id: str, document_id: int, chunks: List[Dict[str, Any]], embeddings, filename=None,
                              file_type=None, metadata: Optional[Dict[str, Any]] = None) -> Dict[str, int]:
        """The chunk phase of DocumentStore.upload_and_index (rag/document_store.py:343-390), after its transaction commits.
        chunks = what upload_and_index got from `self.chunker.chunk(content)`: dicts {content, metadata?}; metadata = its
        `full_metadata`. Each stored row is what the reference inserts: content with NUL removed (:372), metadata
        {**metadata, **chunk['metadata']} (:367-370); empty / non-finite embeddings are skipped (:355-364). The new chunks are
        inserted before the old ones are deleted, under the index lock: a search sees one chunk set or the other, and a failed
        insert leaves the old set in place."""
        rows, embs, skipped = [], [], 0
        for c, e in zip(chunks, embeddings):
            if not e or len(e) == 0 or any(math.isnan(float(v)) or math.isinf(float(v)) for v in e):
                skipped += 1
                continue
            rows.append({"content": c["content"].replace("\x00", ""), "agent_id": agent_id, "document_id": int(document_id),
                         "filename": filename, "file_type": file_type,
                         "metadata": {**(metadata or {}), **(c.get("metadata") or {})}})
            embs.append(e)
        key = (str(agent_id), int(document_id))
        old = self._doc_chunks.pop(key, [])
        try:
            if rows:
                self.add_rows(rows, np.asarray(embs, dtype=np.float32))
        except Exception:
            self._doc_chunks[key] = old
            raise
        self._delete_ids(agent_id, old)
        return {"chunks_created": len(rows), "chunks_skipped": skipped}

    @_locked
    def delete_document(self, agent_id: str, document_id: int) -> bool:
        """DocumentStore.delete_document (rag/document_store.py:524-542): True once the chunks are gone (whether or not the
        document existed), False on failure - a shard exported without document_ids.npy cannot name a document's rows."""
        try:
            key = (str(agent_id), int(document_id))
            if key not in self._doc_chunks and self._shard_without_doc_ids:
                logger.error("Delete failed: the loaded shard has no document ids (document_ids.npy)")
                return False
            self._delete_ids(agent_id, self._doc_chunks.pop(key, []))
            return True
        except Exception as e:
            logger.error(f"Delete failed: {e}")
            return False

    def insert_archival_memory(self, agent_id: str, content: str, embedding: List[float], metadata: Optional[Dict] = None) -> int:
        """DatabaseOperations.insert_archival_memory (database/operations.py:22-57): returns the new id."""
        return self.add_rows([{"agent_id": agent_id, "content": content, "metadata": metadata or {}}], [embedding])[0]

    def bulk_insert_archival_memory(self, agent_id: str, contents: List[str], embeddings: List[List[float]],
                                    metadatas: List[Dict]) -> List[int]:
        if not (len(contents) == len(embeddings) == len(metadatas)):
            raise ValueError("Contents, embeddings, and metadatas must have same length")
        return self.add_rows([{"agent_id": agent_id, "content": c, "metadata": m or {}} for c, m in zip(contents, metadatas)],
                             np.asarray(embeddings, dtype=np.float32).reshape(-1, self.dim))

    @_locked
    def delete_archival_memory(self, agent_id: str, memory_id: int) -> bool:
        """`DELETE FROM archival_memory WHERE id = %s AND agent_id = %s` (database/operations.py:162-172): rowcount > 0."""
        return self._delete_ids(agent_id, [int(memory_id)]) > 0

    @_locked
    def add_texts(self, agent_id: str, texts: List[str], *, batch: int = 64, document_id: Optional[int] = None,
                  metadata: Optional[Dict[str, Any]] = None) -> List[int]:
        """Embed `texts` and add them as rows of `agent_id`: ONE forward per batch gives all three heads of the embedding
        service - the dense vector, the lexical weights (when lexical postings are resident) and the token vectors (when a
        token-vector store is resident), which go from the forward's output tensor into the store and never exist on the host, as
        in build_token_vectors. Each batch goes through add_rows. Returns the ids.
        Over postings built on the device (build_lexical) the sparse leg stays there too: the outputs of rag_lexical_compact_dev go
        straight into rag_sparse_append_dev after the row insert, under the same lock, and no weight reaches the host. A block the
        library rejects (a token id at or past the postings' n_terms) then leaves the rows inserted and the postings stale - as
        a rejected block of the token-vector leg does - where the mirror route refuses before the insert."""
        import torch
        svc = self.embeddings
        texts = [str(t) for t in texts]
        want_lex = self._lexical is not None
        want_tok = self.engine.tokvec_info()["dim"] > 0
        svc._need_heads(want_lex, want_tok)
        skip = svc.special_ids()
        ids_out: List[int] = []
        batch = max(1, int(batch))
        for b in range(0, len(texts), batch):
            part = texts[b:b + batch]
            ids, tt, lens = svc.tokenize(part)
            n, L = ids.shape
            dense = torch.empty((n, self.dim), dtype=torch.float32, device="cuda")
            lex = torch.empty((n, L), dtype=torch.float32, device="cuda") if want_lex else None
            tok = off = None
            if want_tok:
                rows = int((np.clip(lens, 1, L).astype(np.int64) - 1).sum())
                tok = torch.empty((max(rows, 1), int(svc.engine.embed_tok_dim)), dtype=torch.float32, device="cuda")
                off = torch.empty((n + 1,), dtype=torch.int64, device="cuda")
            d_ids, d_lens = torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda()
            svc.engine.embed_multi_dev(d_ids, torch.from_numpy(tt).cuda(), d_lens, dense=dense, lex=lex, tok=tok, row_off=off)
            maps = lex_dev = None
            if want_lex:                                             # the largest weight > 0 of each token id, special tokens left out (encode_multi):
                ptr = torch.empty((n + 1,), dtype=torch.int32, device="cuda")                 # reduced on the device (rag_lexical_compact_dev)
                terms = torch.empty((n * L,), dtype=torch.int32, device="cuda")
                qw = torch.empty((n * L,), dtype=torch.float32, device="cuda")
                svc.engine.lexical_compact_dev(d_ids, lex, d_lens, ptr, terms, qw, skip_ids=skip)
                if self._resident_lexical():
                    lex_dev = (ptr, terms, qw)
                else:
                    ptr, terms, qw = self._to_host(ptr, terms, qw)
                    maps = [dict(zip(terms[a:b].tolist(), qw[a:b].tolist())) for a, b in zip(ptr[:-1], ptr[1:])]
            torch.cuda.synchronize()
            rows_ = [{"agent_id": agent_id, "content": t, "metadata": dict(metadata or {}),
                      **({"document_id": int(document_id)} if document_id is not None else {})} for t in part]
            tv = (tok, off) if want_tok else None
            if lex_dev is None:
                ids_out += self.add_rows(rows_, dense.cpu().numpy(), lexical_weights=maps, token_vectors=tv)
            else:                                                    # device-built postings: the compaction's outputs as they are
                if self._lexical.n_docs != len(self.rows):
                    raise ValueError("add_texts: the lexical postings do not cover the current rows (build_lexical again)")
                res = self._lexical
                dev_append = lambda: (self.engine.sparse_append_dev(*lex_dev, res.n_terms, n_docs_new=n), res.appended(n, res.n_terms))
                ids_out += self._insert_rows(rows_, dense.cpu().numpy().reshape(-1, self.dim), dev_append, tv)
        return ids_out

    @_locked
    def compact(self, keep_resident: bool = False) -> np.ndarray:
        """Drop deleted rows from HBM (rag_index_compact) and remap the payload rows; returns row_map[old row]. keep_resident
        (rag_index_compact_live): resident lexical postings and token vectors move with the rows and stay searchable, and the
        held lexical mirror (or the stand-in of device-built postings) is remapped; by default both end stale until they are
        loaded again."""
        row_map = self.engine.index_compact(keep_resident=True) if keep_resident else self.engine.index_compact()
        if self._lexical is not None:
            if keep_resident and self._lexical.n_docs == len(row_map):
                self._lexical.compacted(row_map)
            elif (row_map < 0).any():
                self._lexical = None                                 # stale on the device: nothing to mirror until load_lexical
        keep = np.nonzero(row_map >= 0)[0]
        if self._row_ids.shape[0] == row_map.shape[0]:
            self._set_row_ids(self._row_ids[keep])
        if isinstance(self.rows, list):
            self.rows = [self.rows[int(i)] for i in keep]
        else:
            v = self.rows if isinstance(self.rows, _RowView) else _RowView(self.rows)
            nb = len(v) - len(v.extra)
            base_keep = keep[keep < nb]
            mapped = _RowView(v.base, base_keep if v.keep is None else np.asarray(v.keep)[base_keep])
            mapped.extra = [v.extra[int(i) - nb] for i in keep[keep >= nb]]
            self.rows = mapped
        return row_map

    def _search_rows(self, agent_id, query_embeddings, top_k):
        if isinstance(agent_id, (list, tuple, np.ndarray)):
            return self._search_rows_mixed(agent_id, query_embeddings, top_k)
        if agent_id is not None and str(agent_id) not in self._tenant_id:
            Q = np.asarray(query_embeddings).reshape(-1, self.dim).shape[0]
            return np.full((Q, top_k), -1, dtype=np.int32), np.zeros((Q, top_k))
        tenant = -1 if agent_id is None else self._tenant_id[str(agent_id)]
        _, rows, scores = self.engine.dense_topk(np.asarray(query_embeddings, dtype=np.float32).reshape(-1, self.dim),
                                                 top_k, tenant=tenant)
        return rows, scores

    def _search_rows_mixed(self, agent_ids, query_embeddings, top_k):
        """One agent PER QUERY (agents mixed in one batch): ONE dense call with a tenant array (rag_dense_topk_tenants_host), row i
        filtered by agent_ids[i] (None: not filtered). An unknown agent owns no row: its query searches under a tenant number no
        row carries and comes back all padding, as the single call returns []."""
        q = np.asarray(query_embeddings, dtype=np.float32).reshape(-1, self.dim)
        if len(agent_ids) != q.shape[0]:
            raise ValueError(f"{len(agent_ids)} agent ids for {q.shape[0]} queries")
        nobody = max(self._tenant_id.values(), default=-1) + 1
        tenants = np.array([-1 if a is None else self._tenant_id.get(str(a), nobody) for a in agent_ids], dtype=np.int32)
        if not self._tenant_id and (tenants >= 0).any():             # no agent known at all (no tenant table): a filtered query finds nothing
            unfiltered = tenants < 0
            rows, scores = np.full((q.shape[0], top_k), -1, dtype=np.int32), np.zeros((q.shape[0], top_k))
            if unfiltered.any():
                _, rows[unfiltered], scores[unfiltered] = self.engine.dense_topk(q[unfiltered], top_k, tenant=-1)
            return rows, scores
        _, rows, scores = self.engine.dense_topk(q, top_k, tenant=tenants)
        return rows, scores

    def search(self, agent_id: str, query: str, top_k: int = 5, with_embeddings: bool = True) -> List[Dict[str, Any]]:
        try:
            q = self.embeddings.generate_embedding(query)            # outside the index lock: a network call in the reference
            with self._lock:
                return self._search_locked(agent_id, q, top_k, with_embeddings)
        except Exception as e:                                       # reference: log and return [] (:483-485)
            logger.error("Search failed: %s", e)
            return []

    def _search_locked(self, agent_id, q, top_k, with_embeddings):
        rows, scores = self._search_rows(agent_id, [q], top_k)
        hit = [int(r) for r in rows[0] if r >= 0]
        embs = self.engine.fetch_rows(hit) if (with_embeddings and hit) else None
        out = []
        for j, r in enumerate(hit):
            row = self.rows[r]
            d = {"content": row.get("content", ""), "filename": row.get("filename"), "file_type": row.get("file_type"),
                 "score": float(scores[0][j]), "metadata": row.get("metadata") or {}}
            if embs is not None:
                d["embedding"] = embs[j].tolist()                     # Python floats; saves apply_mmr's re-embedding calls
            out.append(d)
        return out

    # ---- learned-sparse retrieval (sparse.LexicalPostings; rag_sparse_*) ---------------------------------------------------
    @_locked
    def load_lexical(self, postings) -> None:
        """Make the lexical weights of the loaded rows searchable: `postings` is a sparse.LexicalPostings over exactly the rows of
        this index, in row order (e.g. LexicalPostings.from_texts(self.embeddings, contents)). Inserts and compaction leave them
        stale - search_lexical then answers [] - until this is called again with postings of the current rows."""
        if postings.n_docs != len(self.rows):
            raise ValueError(f"load_lexical: postings of {postings.n_docs} documents for an index of {len(self.rows)} rows")
        postings.load(self.engine)
        self._lexical = postings                       # the mirror grows and shrinks with add_rows(lexical_weights=...) / compact(keep_resident=True)

    @_locked
    def build_lexical(self, texts, batch: int = 64, n_terms: Optional[int] = None) -> None:
        """The counterpart of build_token_vectors for the lexical leg: compute the lexical weights of the rows' texts (texts[i]
        belongs to row i) and build the resident postings from them on the device, `batch` texts at a time - one forward with the
        lexical head, rag_lexical_compact_dev, rag_sparse_append_dev. No weight reaches the host and no host mirror is kept: a
        sparse.ResidentLexical holds the counts live writes are checked against (its `export` reads the postings back).
        Replaces any resident postings. n_terms defaults to the model's vocabulary size. Results equal load_lexical of
        LexicalPostings.from_texts over the same texts."""
        import torch
        from .sparse import ResidentLexical
        svc = self.embeddings
        texts = [str(t) for t in texts]
        if len(texts) != len(self.rows):
            raise ValueError(f"build_lexical: {len(texts)} texts for an index of {len(self.rows)} rows")
        if not texts:
            raise ValueError("build_lexical: the index holds no rows")
        svc._need_heads(True, False)
        if n_terms is None:
            n_terms = getattr(svc, "cfg", {}).get("vocab_size")
        if n_terms is None or int(n_terms) < 1:
            raise ValueError("build_lexical: n_terms is needed (the service names no vocabulary size)")
        skip = svc.special_ids()
        batch = max(1, int(batch))
        self.engine.sparse_clear()
        self._lexical = None
        for b in range(0, len(texts), batch):
            ids, tt, lens = svc.tokenize(texts[b:b + batch])
            n, L = ids.shape
            d_ids, d_lens = torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda()
            lex = torch.empty((n, L), dtype=torch.float32, device="cuda")
            svc.engine.embed_multi_dev(d_ids, torch.from_numpy(tt).cuda(), d_lens, lex=lex)
            ptr = torch.empty((n + 1,), dtype=torch.int32, device="cuda")
            terms = torch.empty((n * L,), dtype=torch.int32, device="cuda")
            qw = torch.empty((n * L,), dtype=torch.float32, device="cuda")
            svc.engine.lexical_compact_dev(d_ids, lex, d_lens, ptr, terms, qw, skip_ids=skip)
            self.engine.sparse_append_dev(ptr, terms, qw, int(n_terms))        # waits for the stream: resident and checked on return
        self._lexical = ResidentLexical(len(texts), int(n_terms))

    @_locked
    def export_lexical(self):
        """The lexical postings of the rows as a sparse.LexicalPostings: the held mirror (load_lexical), or the resident postings
        read back (build_lexical; rag_sparse_export_host) - to save them or to `shard` them. None when there are none."""
        return self._lexical.export(self.engine) if self._resident_lexical() else self._lexical

    def search_lexical(self, agent_id: str, query: str, top_k: int = 5, mode: str = "dense+sparse", pool: int = 100,
                       rrf_k: int = 60) -> List[Dict[str, Any]]:
        """First-stage retrieval with the embedder's lexical head. mode "sparse": the rows whose lexical weights share a token
        with the query's, by sum of weight products (rag_sparse_topk_host). mode "dense+sparse": reciprocal rank fusion of the
        dense top-`pool` (what `search` ranks by) and the sparse top-`pool`, dense list first. The query goes through ONE
        `encode_multi` forward for both its dense vector and its lexical map. Result dicts are `search`'s (without embeddings)
        plus `sparse_score` (0.0 for a fused hit the sparse list does not hold) and, fused, `rrf_score`; `score` is what the
        list is ranked by. Errors are logged and answered with []."""
        try:
            if mode not in ("dense+sparse", "sparse"):
                raise ValueError(f"unknown mode {mode!r}")
            fused = mode == "dense+sparse"
            out = self.embeddings.encode_multi([query], return_dense=fused, return_sparse=True, return_colbert_vecs=False)
            with self._lock:
                return self._search_lexical_locked(agent_id, out, top_k, fused, pool, rrf_k)
        except Exception as e:
            logger.error("Lexical search failed: %s", e)
            return []

    def _search_lexical_locked(self, agent_id, enc, top_k, fused, pool, rrf_k):
        from .sparse import LexicalPostings
        if agent_id is not None and str(agent_id) not in self._tenant_id:
            return []
        tenant = -1 if agent_id is None else self._tenant_id[str(agent_id)]
        ptr, terms, weights = LexicalPostings.encode_queries(enc["lexical_weights"])
        n = max(top_k, pool) if fused else top_k
        _, s_rows, s_scores = self.engine.sparse_topk(ptr, terms, weights, n, tenant=tenant)
        if not fused:
            hits = [(int(r), {"score": float(s), "sparse_score": float(s)}) for r, s in zip(s_rows[0], s_scores[0]) if r >= 0]
        else:
            q = np.asarray(enc["dense_vecs"], dtype=np.float32).reshape(1, self.dim)
            _, d_rows, _ = self.engine.dense_topk(q, n, tenant=tenant)
            lists = np.stack([d_rows[0], s_rows[0]]).astype(np.int64)[None]                 # rows as keys: [1, 2, n], -1 padded
            keys, rrf, _ = self.engine.rrf_fuse(lists, rrf_k=rrf_k, top_k=top_k)
            sparse_of = {int(r): float(s) for r, s in zip(s_rows[0], s_scores[0]) if r >= 0}
            hits = [(int(r), {"score": float(f), "sparse_score": sparse_of.get(int(r), 0.0), "rrf_score": float(f)})
                    for r, f in zip(keys[0], rrf[0]) if r >= 0]
        res = []
        for r, extra in hits:
            row = self.rows[r]
            res.append({"content": row.get("content", ""), "filename": row.get("filename"), "file_type": row.get("file_type"),
                        "metadata": row.get("metadata") or {}, **extra})
        return res

    # ---- late interaction over resident token vectors (rag_tokvec_*) -------------------------------------------------------
    @_locked
    def load_token_vectors(self, vecs, offsets, form: str = "fp16") -> None:
        """Make the rows' token vectors resident: float32 [rows, tok_dim] packed row after row, int64 offsets [len(self.rows) + 1]
        (e.g. embed_multi's outputs kept from an earlier ingest). They are stored as fp16, or with form="mxfp8" as block-scaled
        8-bit codes (33/64 of the bytes; add_rows, add_texts, compact and the searches follow the store's form); a compaction
        leaves them stale - and search_late_interaction falling back to `search` - until this or build_token_vectors runs again."""
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        if off.shape[0] - 1 != len(self.rows):
            raise ValueError(f"load_token_vectors: offsets of {off.shape[0] - 1} documents for an index of {len(self.rows)} rows")
        self.engine.tokvec_load(vecs, off, form=form)

    @_locked
    def build_token_vectors(self, texts, batch: int = 64, *, headroom_docs: int = 0, headroom_rows: int = 0, form: str = "fp16") -> None:
        """Compute the token vectors of the rows' texts (texts[i] belongs to row i) with the embedding service's token-vector head
        and append them to the resident store on the device, `batch` texts per forward: the vectors go from the forward's output
        tensor into the store and never exist on the host. headroom_docs / headroom_rows reserve room for the documents later
        add_rows(token_vectors=...) / add_texts calls append (a reservation does not grow; compact(keep_resident=True) returns the
        rows of deleted documents to it). form: "fp16" or "mxfp8", as load_token_vectors."""
        import torch
        svc = self.embeddings
        texts = [str(t) for t in texts]
        if len(texts) != len(self.rows):
            raise ValueError(f"build_token_vectors: {len(texts)} texts for an index of {len(self.rows)} rows")
        if not texts:
            raise ValueError("build_token_vectors: the index holds no rows")
        svc._need_heads(False, True)
        tok_dim = int(svc.engine.embed_tok_dim)
        batch = max(1, int(batch))
        batches = [svc.tokenize(texts[b:b + batch]) for b in range(0, len(texts), batch)]
        n_rows = [int((np.clip(lens, 1, ids.shape[1]).astype(np.int64) - 1).sum()) for ids, _, lens in batches]
        self.engine.tokvec_reserve(len(texts) + max(0, int(headroom_docs)), sum(n_rows) + max(0, int(headroom_rows)), tok_dim, form=form)
        for (ids, tt, lens), rows in zip(batches, n_rows):
            tok = torch.empty((max(rows, 1), tok_dim), dtype=torch.float32, device="cuda")
            off = torch.empty((len(lens) + 1,), dtype=torch.int64, device="cuda")
            svc.engine.embed_multi_dev(torch.from_numpy(ids).cuda(), torch.from_numpy(tt).cuda(), torch.from_numpy(lens).cuda(), tok=tok, row_off=off)
            self.engine.tokvec_append_dev(tok, off)          # waits for the stream: the block is resident and checked on return

    def search_late_interaction(self, agent_id: str, query: str, top_k: int = 5, pool: int = 100, mode: str = "dense") -> List[Dict[str, Any]]:
        """Retrieve `pool` candidates - mode "dense": what `search` ranks by; "dense+sparse": reciprocal rank fusion with the
        learned-sparse list, as search_lexical - and rerank them by MaxSim of the query's token vectors against the rows' resident
        ones (rag_tokvec_rerank_*). The query goes through ONE encode_multi forward. Result dicts are `search`'s (without
        embeddings) plus `colbert_score`, which `score` equals. mode "maxsim" has no candidate stage: every row the agent may see
        is scored by MaxSim on the device (RagEngine.tokvec_search_dev) and the best `top_k` are returned - retrieval by MaxSim, for
        a passage that neither the pooled vector nor the lexical weights would bring into the pool. Never raises: an error (no store, a stale one, a missing head) is
        logged and answered with `search`."""
        try:
            if mode == "maxsim":
                enc = self.embeddings.encode_multi([query], return_dense=False, return_sparse=False, return_colbert_vecs=True)
                with self._lock:
                    return self._search_maxsim_locked(agent_id, enc, top_k, int(pool))
            if mode not in ("dense", "dense+sparse"):
                raise ValueError(f"unknown mode {mode!r}")
            fused = mode == "dense+sparse"
            enc = self.embeddings.encode_multi([query], return_dense=True, return_sparse=fused, return_colbert_vecs=True)
            with self._lock:
                return self._search_late_locked(agent_id, enc, top_k, int(pool), fused)
        except Exception as e:
            logger.error("Late-interaction search failed, answering with search: %s", e)
            return self.search(agent_id, query, top_k, with_embeddings=False)

    def _search_late_locked(self, agent_id, enc, top_k, pool, fused, rrf_k=60):
        from .sparse import LexicalPostings
        if agent_id is not None and str(agent_id) not in self._tenant_id:
            return []
        info = self.engine.tokvec_info()
        if info["n_docs"] != len(self.rows):
            raise RuntimeError(f"token vectors of {info['n_docs']} documents for an index of {len(self.rows)} rows")
        tenant = -1 if agent_id is None else self._tenant_id[str(agent_id)]
        pool = max(1, min(256, max(pool, top_k)))
        k = min(int(top_k), pool)
        q = np.asarray(enc["dense_vecs"], dtype=np.float32).reshape(1, self.dim)
        _, d_rows, _ = self.engine.dense_topk(q, pool, tenant=tenant)
        cand = d_rows
        if fused:
            ptr, terms, weights = LexicalPostings.encode_queries(enc["lexical_weights"])
            _, s_rows, _ = self.engine.sparse_topk(ptr, terms, weights, pool, tenant=tenant)
            lists = np.stack([d_rows[0], s_rows[0]]).astype(np.int64)[None]                 # rows as keys: [1, 2, pool], -1 padded
            keys, _, _ = self.engine.rrf_fuse(lists, rrf_k=rrf_k, top_k=pool)
            cand = keys
        qv = np.ascontiguousarray(enc["colbert_vecs"][0], dtype=np.float32)
        _, rows, scores, _ = self.engine.tokvec_rerank(qv, np.array([0, qv.shape[0]], dtype=np.int64), np.asarray(cand, dtype=np.int32), k)
        res = []
        for r, s in zip(rows[0], scores[0]):
            if r < 0:
                continue
            row = self.rows[int(r)]
            res.append({"content": row.get("content", ""), "filename": row.get("filename"), "file_type": row.get("file_type"),
                        "score": float(s), "colbert_score": float(s), "metadata": row.get("metadata") or {}})
        return res

    def _search_maxsim_locked(self, agent_id, enc, top_k, pool):
        if agent_id is not None and str(agent_id) not in self._tenant_id:
            return []
        tenant = -1 if agent_id is None else self._tenant_id[str(agent_id)]
        pool = max(1, min(256, max(pool, top_k)))
        k = min(int(top_k), pool)
        qv = np.ascontiguousarray(enc["colbert_vecs"][0], dtype=np.float32)
        ids, scores, _ = self.engine.tokvec_search_dev(self._to_device(qv), self._to_device(np.array([0, qv.shape[0]], dtype=np.int64)), k,
                                                       pool=pool, tenant=tenant)
        ids, scores = self._to_host(ids, scores)
        res = []
        for r, s in zip(self._rows_of_ids(ids)[0], scores[0]):
            if r < 0:
                continue
            row = self.rows[int(r)]
            res.append({"content": row.get("content", ""), "filename": row.get("filename"), "file_type": row.get("file_type"),
                        "score": float(s), "colbert_score": float(s), "metadata": row.get("metadata") or {}})
        return res

    # ---- bge-m3's three-way score over the resident legs (rag_m3_score_rows_dev) --------------------------------------------
    def search_m3(self, agent_id: str, query: str, top_k: int = 5, pool: int = 100, weights=(0.4, 0.2, 0.4),
                  candidates: str = "union", device_query: bool = False) -> List[Dict[str, Any]]:
        """Rank by bge-m3's "colbert+sparse+dense" score: (w_colbert * colbert + w_sparse * sparse + w_dense * dense) / sum, weights =
        (dense, sparse, colbert), every component exact for every candidate and computed from resident data - the fp32 rows, the
        lexical postings (load_lexical), the token vectors (load_token_vectors / build_token_vectors). candidates "union": the dense
        top-`pool` and the sparse top-`pool` together (pool <= 128); "dense": the dense top-`pool`; "dense+sparse": their reciprocal
        rank fusion, top-`pool`. A weight of 0 leaves its component and its resident structure out. The query goes through ONE
        encode_multi forward. Result dicts are `search`'s (without embeddings) plus `dense_score`, `sparse_score`, `colbert_score`
        and `score`. Never raises: an error (a missing or stale leg, a missing head) is logged and answered with `search`.
        device_query: the query is tokenised on the host and everything else - forward, lexical compaction, candidates, score -
        runs on the device without a host round trip (search_m3_many's device_query, for one query); the same result."""
        try:
            if candidates not in ("union", "dense", "dense+sparse"):
                raise ValueError(f"unknown candidates {candidates!r}")
            w = tuple(float(x) for x in weights)
            if len(w) != 3:
                raise ValueError("weights are (dense, sparse, colbert)")
            need_sparse = w[1] > 0 or candidates != "dense"
            if device_query:
                res = self._m3_device_query(agent_id, [query], int(top_k), int(pool), w, candidates)
                if res is not None:
                    return res[0]
            enc = self.embeddings.encode_multi([query], return_dense=True, return_sparse=need_sparse, return_colbert_vecs=w[2] > 0)
            with self._lock:
                return self._search_m3_locked(agent_id, enc, top_k, int(pool), w, candidates)
        except Exception as e:
            logger.error("Three-way search failed, answering with search: %s", e)
            return self.search(agent_id, query, top_k, with_embeddings=False)

    def _search_m3_locked(self, agent_id, enc, top_k, pool, w, candidates, rrf_k=60):
        import torch
        from .sparse import LexicalPostings
        if agent_id is not None and str(agent_id) not in self._tenant_id:
            return []
        tenant = -1 if agent_id is None else self._tenant_id[str(agent_id)]
        pool = max(1, min(128 if candidates == "union" else 256, max(pool, top_k)))
        q = np.asarray(enc["dense_vecs"], dtype=np.float32).reshape(1, self.dim)
        _, d_rows, _ = self.engine.dense_topk(q, pool, tenant=tenant)
        cand = d_rows
        ptr = terms = qw = None
        if w[1] > 0 or candidates != "dense":
            ptr, terms, qw = LexicalPostings.encode_queries(enc["lexical_weights"])
        if candidates != "dense":
            _, s_rows, _ = self.engine.sparse_topk(ptr, terms, qw, pool, tenant=tenant)
            lists = np.stack([d_rows[0], s_rows[0]]).astype(np.int64)[None]                 # rows as keys: [1, 2, pool], -1 padded
            cand, _, _ = self.engine.rrf_fuse(lists, rrf_k=rrf_k, top_k=2 * pool if candidates == "union" else pool)
        cand = np.ascontiguousarray(cand, dtype=np.int32)
        k = min(int(top_k), cand.shape[1])
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
        qv = qo = None
        if w[2] > 0:
            v = np.ascontiguousarray(enc["colbert_vecs"][0], dtype=np.float32)
            qv = torch.from_numpy(v if v.shape[0] else np.zeros((1, max(v.shape[1], 1)), np.float32)).cuda()
            qo = dev(np.array([0, v.shape[0]], dtype=np.int64))
        sparse_in = w[1] > 0
        ids = torch.empty((1, k), dtype=torch.int64, device="cuda")
        rows = torch.empty((1, k), dtype=torch.int32, device="cuda")
        sc = torch.empty((1, k), dtype=torch.float64, device="cuda")
        comp = torch.empty((1, k, 3), dtype=torch.float64, device="cuda")
        t_ptr, t_terms, t_qw = (dev(ptr), dev(terms) if terms is not None and len(terms) else dev(np.zeros(1, np.int32)),
                                dev(qw) if qw is not None and len(qw) else dev(np.zeros(1, np.float32))) if sparse_in else (None, None, None)
        self.engine.m3_score_rows_dev(dev(cand), k, ids, sc, q_emb=dev(q), term_ptr=t_ptr, terms=t_terms, weights=t_qw, q_vecs=qv, q_off=qo,
                                      w=w, rows_out=rows, components_out=comp)
        torch.cuda.current_stream().synchronize()
        rows, sc, comp = rows.cpu().numpy()[0], sc.cpu().numpy()[0], comp.cpu().numpy()[0]
        res = []
        for r, s, c in zip(rows, sc, comp):
            if r < 0:
                continue
            row = self.rows[int(r)]
            res.append({"content": row.get("content", ""), "filename": row.get("filename"), "file_type": row.get("file_type"),
                        "score": float(s), "dense_score": float(c[0]), "sparse_score": float(c[1]), "colbert_score": float(c[2]),
                        "metadata": row.get("metadata") or {}})
        return res

    # ---- the bge-m3 searches for a batch of queries, one agent per query (rag_*_tenants_*) ----------------------------------
    def _set_row_ids(self, ids):
        self._row_ids, self._row_ids_sorted = ids, None

    def _rows_of_ids(self, ids):
        """Engine ids [Q, k] (-1 padded) -> rows of this index (-1 kept). An id that was deleted and inserted again names its
        latest row: a search never returns a deleted one."""
        ids = np.asarray(ids, dtype=np.int64)
        if self._row_ids.shape[0] != len(self.rows):
            raise RuntimeError("the ids of the index's rows are not known (rows were set without bulk_load / load_shard / add_rows)")
        if self._row_ids_sorted is None:
            order = np.argsort(self._row_ids, kind="stable")
            self._row_ids_sorted = (self._row_ids[order], order)
        sorted_ids, order = self._row_ids_sorted
        if not sorted_ids.shape[0]:
            return np.full(ids.shape, -1, dtype=np.int64)
        at = np.clip(np.searchsorted(sorted_ids, ids, side="right") - 1, 0, sorted_ids.shape[0] - 1)
        return np.where((ids >= 0) & (sorted_ids[at] == ids), order[at], -1)

    def _tenants_of(self, agent_id, n_queries):
        """int32 [n_queries]: the tenant number of every query's agent - one agent for all of them or a list with one per query;
        None: -1, not filtered; an unknown agent: a number no row carries, so its query comes back all padding
        (_search_rows_mixed's rule)."""
        agents = list(agent_id) if isinstance(agent_id, (list, tuple, np.ndarray)) else [agent_id] * n_queries
        if len(agents) != n_queries:
            raise ValueError(f"{len(agents)} agent ids for {n_queries} queries")
        nobody = max(self._tenant_id.values(), default=-1) + 1
        return np.array([-1 if a is None else self._tenant_id.get(str(a), nobody) for a in agents], dtype=np.int32)

    @staticmethod
    def _to_device(a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    @staticmethod
    def _to_host(*tensors):
        """the outputs of a device call queued on the current stream, as numpy arrays"""
        import torch
        torch.cuda.current_stream().synchronize()
        return [t.cpu().numpy() for t in tensors]

    def _payload(self, r, extra):
        row = self.rows[int(r)]
        return {"content": row.get("content", ""), "filename": row.get("filename"), "file_type": row.get("file_type"),
                "metadata": row.get("metadata") or {}, **extra}

    def search_lexical_many(self, agent_id, queries: List[str], top_k: int = 5, mode: str = "dense+sparse", pool: int = 100,
                            rrf_k: int = 60, device_query: bool = False) -> List[List[Dict[str, Any]]]:
        """Batched `search_lexical`: ONE encode_multi forward for all queries, then ONE search call with a tenant per query -
        rag_sparse_topk_tenants_host (mode "sparse") or rag_hybrid_sparse_rrf_tenants_dev (mode "dense+sparse"; the fused hits'
        `sparse_score` is then read back with one point lookup, rag_sparse_score_rows_host, whose bits are the search's).
        agent_id: one agent, None (not filtered), or a list with one of either per query. Element i equals
        `search_lexical(agent_id[i], queries[i], top_k, mode, pool, rrf_k)`; an unknown agent gets []. Errors are logged and
        answered with [] for every query. device_query: the queries' CSR is built on the device (the forward, then
        rag_lexical_compact_dev) and handed to the device forms of the same searches; the same result."""
        try:
            if mode not in ("dense+sparse", "sparse"):
                raise ValueError(f"unknown mode {mode!r}")
            if not queries:
                return []
            fused = mode == "dense+sparse"
            svc = self._device_query_service() if device_query else None
            if svc is not None:
                svc._need_heads(True, False)
                toks = svc.tokenize(list(queries))
                with self._lock:
                    res = self._search_lexical_many_device(agent_id, svc, toks, int(top_k), fused, pool, rrf_k)
                if res is not None:
                    return res
            enc = self.embeddings.encode_multi(list(queries), return_dense=fused, return_sparse=True, return_colbert_vecs=False)
            with self._lock:
                return self._search_lexical_many_locked(agent_id, enc, len(queries), int(top_k), fused, pool, rrf_k)
        except Exception as e:
            logger.error("Batched lexical search failed: %s", e)
            return [[] for _ in queries]

    def _search_lexical_many_locked(self, agent_id, enc, Q, top_k, fused, pool, rrf_k):
        from .sparse import LexicalPostings
        tenants = self._tenants_of(agent_id, Q)
        if not self._tenant_id and (tenants >= 0).any():                 # no agent known at all: a filtered query finds nothing
            return [[] for _ in range(Q)] if (tenants >= 0).all() else self._unfiltered_only(
                tenants, lambda sel: self._search_lexical_many_locked(None, _enc_rows(enc, sel), len(sel), top_k, fused, pool, rrf_k))
        ptr, terms, weights = LexicalPostings.encode_queries(enc["lexical_weights"])
        if not fused:
            _, rows, scores = self.engine.sparse_topk(ptr, terms, weights, top_k, tenant=tenants)
            return [[self._payload(r, {"score": float(s), "sparse_score": float(s)}) for r, s in zip(rows[i], scores[i]) if r >= 0]
                    for i in range(Q)]
        dev = self._to_device
        q = np.asarray(enc["dense_vecs"], dtype=np.float32).reshape(Q, self.dim)
        n = max(top_k, pool)
        keys, rrf, ranks = self.engine.hybrid_sparse_rrf_dev(dev(q), dev(ptr), dev(terms if len(terms) else np.zeros(1, np.int32)),
                                                             dev(weights if len(weights) else np.zeros(1, np.float32)), n, top_k,
                                                             rrf_k=rrf_k, tenant=tenants)
        keys, rrf, ranks = self._to_host(keys, rrf, ranks)
        rows = self._rows_of_ids(keys)
        sparse = self.engine.sparse_score_rows(ptr, terms, weights, rows.astype(np.int32))
        return [[self._payload(r, {"score": float(f), "sparse_score": float(s) if rk[1] > 0 else 0.0, "rrf_score": float(f)})
                 for r, f, s, rk in zip(rows[i], rrf[i], sparse[i], ranks[i]) if r >= 0] for i in range(Q)]

    # ---- the query path on the device (device_query=True): token ids in, nothing on the host until the results are copied out ----
    def _device_query_service(self):
        """the embedding service when it can hand over token ids (tokenize, special_ids, an engine), else None and one logged line"""
        svc = self.embeddings
        if all(callable(getattr(svc, m, None)) for m in ("tokenize", "special_ids", "_need_heads")) and getattr(svc, "engine", None) is not None:
            return svc
        logger.info("device_query: the embedding service offers no tokenize / special_ids; taking the host-assembled query path")
        return None

    def _query_forward_dev(self, svc, toks, want_dense, want_lex, want_tok):
        """embed_multi_dev + lexical_compact_dev on the service's engine, on the current stream: dict(q_emb, term_ptr, terms,
        weights, q_vecs, q_off) of CUDA tensors (None where not asked for), at the capacities rag_search_m3_tokens_dev uses"""
        import torch
        ids, tt, lens = (self._to_device(a) for a in toks)
        Q, L = ids.shape
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device="cuda")
        out = dict.fromkeys(("q_emb", "term_ptr", "terms", "weights", "q_vecs", "q_off"))
        lex = new((Q, L), torch.float32) if want_lex else None
        if want_dense:
            out["q_emb"] = new((Q, svc.dimensions), torch.float32)
        tok = None
        if want_tok:
            out["q_vecs"] = new((max(Q * (L - 1), 1), int(svc.engine.embed_tok_dim)), torch.float32)
            out["q_off"] = new((Q + 1,), torch.int64)
            tok = out["q_vecs"][:Q * (L - 1)]
        svc.engine.embed_multi_dev(ids, tt, lens, dense=out["q_emb"], lex=lex, tok=tok, row_off=out["q_off"])
        if want_lex:
            out.update(term_ptr=new((Q + 1,), torch.int32), terms=new((Q * L,), torch.int32), weights=new((Q * L,), torch.float32))
            svc.engine.lexical_compact_dev(ids, lex, lens, out["term_ptr"], out["terms"], out["weights"], skip_ids=svc.special_ids())
        return out

    def _m3_device_query(self, agent_id, queries, top_k, pool, w, candidates, rrf_k=60):
        """search_m3_many's result through the device query path, or None where that path does not apply (a service without
        token ids, more than a pool of the union asked for, no agent known at all): the caller goes on as without device_query.
        One call (rag_search_m3_tokens(_tenants)_dev) when the service runs on the index's engine, else the forward and the
        compaction on the service's engine and rag_retrieve_m3(_tenants)_dev on the index's, all on the current stream."""
        svc = self._device_query_service()
        if svc is None:
            return None
        need_sparse = w[1] > 0 or candidates != "dense"
        svc._need_heads(need_sparse, w[2] > 0)
        toks = svc.tokenize([str(q) for q in queries])                   # outside the index lock, as the forward of the host path
        with self._lock:
            Q = len(queries)
            tenants = self._tenants_of(agent_id, Q)
            if not self._tenant_id and (tenants >= 0).any():
                return None
            pool = max(1, min(128 if candidates == "union" else 256, max(pool, top_k)))      # search_m3's clamp
            k = min(top_k, 2 * pool if candidates == "union" else pool)
            if k > pool:
                return None
            mode = {"dense": 0, "dense+sparse": 1, "union": 2}[candidates]
            if svc.engine is self.engine:
                ids, tt, lens = (self._to_device(a) for a in toks)
                ids, sc, comp, _ = self.engine.search_m3_tokens_dev(ids, tt, lens, pool, k, skip_ids=svc.special_ids(), mode=mode, w=w,
                                                                    rrf_k=rrf_k, tenant=tenants)
            else:
                f = self._query_forward_dev(svc, toks, True, need_sparse, w[2] > 0)
                ids, sc, comp, _ = self.engine.retrieve_m3_dev(f.pop("q_emb"), pool, k, mode=mode, w=w, rrf_k=rrf_k, tenant=tenants, **f)
            ids, sc, comp = self._to_host(ids, sc, comp)
            rows = self._rows_of_ids(ids)
            return [[self._payload(r, {"score": float(s), "dense_score": float(c[0]), "sparse_score": float(c[1]), "colbert_score": float(c[2])})
                     for r, s, c in zip(rows[i], sc[i], comp[i]) if r >= 0] for i in range(Q)]

    def _search_lexical_many_device(self, agent_id, svc, toks, top_k, fused, pool, rrf_k):
        """_search_lexical_many_locked with the queries' CSR built on the device; None where it does not apply"""
        import torch
        Q = int(toks[0].shape[0])
        tenants = self._tenants_of(agent_id, Q)
        if not self._tenant_id and (tenants >= 0).any():
            return None
        f = self._query_forward_dev(svc, toks, fused, True, False)
        ptr, terms, qw = f["term_ptr"], f["terms"], f["weights"]
        if not fused:
            ids = torch.empty((Q, top_k), dtype=torch.int64, device="cuda")
            rows = torch.empty((Q, top_k), dtype=torch.int32, device="cuda")
            sc = torch.empty((Q, top_k), dtype=torch.float64, device="cuda")
            self.engine.sparse_topk_dev(ptr, terms, qw, top_k, ids, rows, sc, tenant=tenants)
            rows, sc = self._to_host(rows, sc)
            return [[self._payload(r, {"score": float(s), "sparse_score": float(s)}) for r, s in zip(rows[i], sc[i]) if r >= 0]
                    for i in range(Q)]
        keys, rrf, ranks = self.engine.hybrid_sparse_rrf_dev(f["q_emb"], ptr, terms, qw, max(top_k, pool), top_k, rrf_k=rrf_k, tenant=tenants)
        keys, rrf, ranks = self._to_host(keys, rrf, ranks)
        rows = self._rows_of_ids(keys)
        sparse = torch.empty((Q, top_k), dtype=torch.float64, device="cuda")
        self.engine.sparse_score_rows_dev(ptr, terms, qw, self._to_device(rows.astype(np.int32)), sparse)
        sparse, = self._to_host(sparse)
        return [[self._payload(r, {"score": float(f_), "sparse_score": float(s) if rk[1] > 0 else 0.0, "rrf_score": float(f_)})
                 for r, f_, s, rk in zip(rows[i], rrf[i], sparse[i], ranks[i]) if r >= 0] for i in range(Q)]

    def _unfiltered_only(self, tenants, run):
        """[] for every filtered query, run(sel) for the queries `sel` that are not filtered"""
        sel = [i for i, t in enumerate(tenants) if t < 0]
        out = [[] for _ in tenants]
        for i, res in zip(sel, run(sel)):
            out[i] = res
        return out

    def search_m3_many(self, agent_id, queries: List[str], top_k: int = 5, pool: int = 100, weights=(0.4, 0.2, 0.4),
                       candidates: str = "union", device_query: bool = False) -> List[List[Dict[str, Any]]]:
        """Batched `search_m3`: ONE encode_multi forward for all queries, then ONE device call with a tenant per query
        (rag_retrieve_m3_tenants_dev: candidates "dense" / "dense+sparse" / "union" = its modes 0 / 1 / 2) - candidates, the three
        components and the top-k without a host round trip in between. agent_id: one agent, None (not filtered), or a list with
        one of either per query. Element i equals `search_m3(agent_id[i], queries[i], top_k, pool, weights, candidates)`: the same
        rows in the same order, scores and components equal as floats; an unknown agent gets []. weights (0, 0, 1) with candidates
        "dense" is search_late_interaction's ranking. Never raises: an error is logged and answered with `search_many`.
        device_query (needs a local embedding service with `tokenize` and `special_ids`; any other falls back to the path above
        with one logged line): the queries are tokenised on the host and everything else runs on the device with no host round
        trip until the ids, scores and components are copied out - rag_search_m3_tokens(_tenants)_dev when the service runs on the
        index's engine, else embed_multi_dev + lexical_compact_dev on the service's engine and retrieve_m3_dev on the index's.
        The result is the same: the same rows in the same order, scores and components equal as floats."""
        try:
            if candidates not in ("union", "dense", "dense+sparse"):
                raise ValueError(f"unknown candidates {candidates!r}")
            w = tuple(float(x) for x in weights)
            if len(w) != 3:
                raise ValueError("weights are (dense, sparse, colbert)")
            if not queries:
                return []
            need_sparse = w[1] > 0 or candidates != "dense"
            if device_query:
                res = self._m3_device_query(agent_id, list(queries), int(top_k), int(pool), w, candidates)
                if res is not None:
                    return res
            enc = self.embeddings.encode_multi(list(queries), return_dense=True, return_sparse=need_sparse, return_colbert_vecs=w[2] > 0)
            with self._lock:
                return self._search_m3_many_locked(agent_id, enc, len(queries), int(top_k), int(pool), w, candidates)
        except Exception as e:
            logger.error("Batched three-way search failed, answering with search_many: %s", e)
            return self.search_many(agent_id, queries, top_k, with_embeddings=False)

    def _search_m3_many_locked(self, agent_id, enc, Q, top_k, pool, w, candidates, rrf_k=60):
        from .sparse import LexicalPostings
        tenants = self._tenants_of(agent_id, Q)
        if not self._tenant_id and (tenants >= 0).any():
            return [[] for _ in range(Q)] if (tenants >= 0).all() else self._unfiltered_only(
                tenants, lambda sel: self._search_m3_many_locked(None, _enc_rows(enc, sel), len(sel), top_k, pool, w, candidates, rrf_k))
        pool = max(1, min(128 if candidates == "union" else 256, max(pool, top_k)))      # search_m3's clamp
        k = min(top_k, 2 * pool if candidates == "union" else pool)
        if k > pool:                                                     # more than a pool of the union: past the one-call form
            agents = list(agent_id) if isinstance(agent_id, (list, tuple, np.ndarray)) else [agent_id] * Q
            return [self._search_m3_locked(a, _enc_rows(enc, [i]), top_k, pool, w, candidates, rrf_k) for i, a in enumerate(agents)]
        dev = self._to_device
        kw = {}
        if w[1] > 0 or candidates != "dense":
            ptr, terms, qw = LexicalPostings.encode_queries(enc["lexical_weights"])
            kw.update(term_ptr=dev(ptr), terms=dev(terms if len(terms) else np.zeros(1, np.int32)),
                      weights=dev(qw if len(qw) else np.zeros(1, np.float32)))
        if w[2] > 0:
            vecs = [np.ascontiguousarray(v, dtype=np.float32) for v in enc["colbert_vecs"]]
            off = np.concatenate([[0], np.cumsum([v.shape[0] for v in vecs])]).astype(np.int64)
            flat = np.concatenate(vecs) if off[-1] else np.zeros((1, max(vecs[0].shape[1], 1)), np.float32)
            kw.update(q_vecs=dev(flat), q_off=dev(off))
        q = np.asarray(enc["dense_vecs"], dtype=np.float32).reshape(Q, self.dim)
        mode = {"dense": 0, "dense+sparse": 1, "union": 2}[candidates]
        ids, sc, comp, _ = self.engine.retrieve_m3_dev(dev(q), pool, k, mode=mode, w=w, rrf_k=rrf_k, tenant=tenants, **kw)
        ids, sc, comp = self._to_host(ids, sc, comp)
        rows = self._rows_of_ids(ids)
        return [[self._payload(r, {"score": float(s), "dense_score": float(c[0]), "sparse_score": float(c[1]), "colbert_score": float(c[2])})
                 for r, s, c in zip(rows[i], sc[i], comp[i]) if r >= 0] for i in range(Q)]

    def search_many(self, agent_id: str, queries: List[str], top_k: int = 5, with_embeddings: bool = True) -> List[List[Dict[str, Any]]]:
        """Batched `search` (the reference agent can only submit one query per call, so nothing in
        its surface reaches the batched throughput): ONE embedding call for all queries when the service offers
        `generate_embeddings_batch`, ONE rag_dense_topk_host call with Q = len(queries), one row fetch. Element i equals
        `search(agent_id, queries[i], top_k, with_embeddings)`; on failure every element is [] (the reference's log-and-
        return-empty, :483-485). agent_id may be a list with one agent per query (a host serving many agents from one index
        batches their queries together): element i then equals `search(agent_id[i], queries[i], ...)`, [] for an unknown agent."""
        try:
            if not queries:
                return []
            if hasattr(self.embeddings, "generate_embeddings_batch"):
                embs = self.embeddings.generate_embeddings_batch(list(queries))
            else:
                embs = [self.embeddings.generate_embedding(q) for q in queries]
            with self._lock:                                         # embeddings first, outside the index lock
                return self._search_many_locked(agent_id, queries, embs, top_k, with_embeddings)
        except Exception as e:
            logger.error("Batched search failed: %s", e)
            return [[] for _ in queries]

    def _search_many_locked(self, agent_id, queries, embs, top_k, with_embeddings):
        rows, scores = self._search_rows(agent_id, embs, top_k)
        hits = [[int(r) for r in rows[i] if r >= 0] for i in range(len(queries))]
        flat = [r for h in hits for r in h]
        fetched = self.engine.fetch_rows(flat) if (with_embeddings and flat) else None
        out, pos = [], 0
        for i, h in enumerate(hits):
            res = []
            for j, r in enumerate(h):
                row = self.rows[r]
                d = {"content": row.get("content", ""), "filename": row.get("filename"), "file_type": row.get("file_type"),
                     "score": float(scores[i][j]), "metadata": row.get("metadata") or {}}
                if fetched is not None:
                    d["embedding"] = fetched[pos + j].tolist()
                res.append(d)
            pos += len(h)
            out.append(res)
        return out

    @_locked
    def search_batch(self, agent_id: Optional[str], query_embeddings, top_k: int = 20):
        """Batched entry the reference lacks: Q query embeddings at once -> (row indices [Q,k], cosines [Q,k]). agent_id: one
        agent for the batch, None (no filter), or a list with one agent (or None) per query."""
        return self._search_rows(agent_id, query_embeddings, top_k)

    @_locked
    def search_archival_memory(self, agent_id: str, query_embedding: List[float], limit: int = 5) -> List[Dict[str, Any]]:
        rows, scores = self._search_rows(agent_id, [query_embedding], limit)
        return [{"id": self.rows[int(r)].get("id", int(r)), "content": self.rows[int(r)].get("content", ""),
                 "metadata": self.rows[int(r)].get("metadata"), "similarity": float(s),
                 "created_at": self.rows[int(r)].get("created_at")}
                for r, s in zip(rows[0], scores[0]) if r >= 0]
