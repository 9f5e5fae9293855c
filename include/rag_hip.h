/*
 * rag_hip.h — C-ABI of librag_hip.so: the MI355X (gfx950) hybrid-retrieval + rerank engine.
 *
 * The reference (gabrielcheda/optimized-rag) is pure Python and has NO FFI of its own; the drop-in
 * boundary is its Python object graph. Each entry point below names the reference
 * Python call whose arithmetic it replaces (paths under /root/reference). The Python mirror classes in
 * optimized-rag_amd/ bind these symbols with ctypes and keep the reference's class/method surface.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; rag_last_error(h) gives the message.
 *   - plain pointers and sizes only; the caller owns every buffer; nothing throws across the ABI.
 *   - "_host" pointers are host memory (copied over PCIe inside the call, call is synchronous);
 *     "_dev"  pointers are device memory on the handle's GPU; those calls are asynchronous on `stream`, a
 *     hipStream_t passed as void*. NULL means the DEFAULT (null) stream, exactly as in HIP itself — frameworks
 *     whose current stream is the default stream (PyTorch) pass 0 and get correct ordering with their own work.
 *     The handle's private stream is only used by the synchronous *_host entry points.
 *   - one handle = one GPU = one process rank. Every entry point takes the handle's internal lock: the synchronous
 *     *_host calls may be issued from several threads at once (the reference graph is single-threaded,
 *     agent/rag_graph.py:506, but its DB pool allows 10 concurrent searches, database/connection.py:38-42); they
 *     run one after another. *_dev calls share the handle's device workspaces: issue them on ONE stream.
 *   - Ordering (pinned by tests/test_stream_order_gpu.py and, for the entries added since, tests/test_stream_order_resident_gpu.py;
 *     tests/test_stream_order_table_cpu.py fails for a *_dev entry declared here that neither file exercises). A *_dev call returns once its work is queued on `stream`; all it
 *     reads and writes is ordered on that stream as if it had run there alone: inputs produced earlier on the stream are
 *     seen, outputs may be consumed by later work on it, no other stream and no device-wide wait is needed. The calls that
 *     do wait for `stream` say so below (rag_tokens_append_dev, rag_tokvec_append_dev, rag_sparse_append_dev; any call that has to grow a workspace it used before frees
 *     the old one first, which waits for the device - the first call of a larger shape, not the steady state).
 *     A *_host call may be made while *_dev work of the handle is pending, from any thread, and behaves as if it ran after
 *     that work: it first waits for the device when a *_dev call was made on the handle since the last such wait (a
 *     device-wide wait, so *_dev work on any stream is covered; nothing is added to a *_host call that follows a *_host
 *     call, nor to any *_dev call). So a *_dev call queued before a host search or a host write (rag_index_set_tenants_host,
 *     rag_index_set_ids_host, rag_index_set_temporal_host, rag_tokens_load_host, rag_tokens_reserve, rag_tokens_load_wide_host,
 *     rag_tokens_reserve_wide, rag_bm25_load_host, rag_sparse_load_host, rag_tokvec_reserve, rag_tokvec_load_host,
 *     rag_tokvec_append_host, rag_tokvec_reserve_form, rag_tokvec_load_form_host,
 *     rag_bm25_append_host, rag_bm25_fold, rag_bm25_live_counts_host, rag_bm25_set_statistics_host, rag_bm25_refresh,
 *     rag_sparse_append_host, rag_sparse_fold, rag_index_compact_bm25, rag_index_compact_live, rag_index_load_host, rag_index_reserve,
 *     rag_index_id_map, rag_ce_load_host, rag_embed_load_host, the live writes) returns the result
 *     from before it, and the same call made afterwards the new one. rag_bm25_set_normalize, rag_set_option and
 *     rag_ce_set_pair_format do not
 *     wait: they change host state that a *_dev call reads while it enqueues, so a call queued earlier keeps the old value.
 *     rag_tokens_info reads host state only and waits for nothing.
 *     *_dev calls of one handle on SEVERAL streams stay unordered among themselves: that is the caller's to order.
 *     A result does not depend on the calls the handle served before: the per-handle workspaces are grow-only and carved anew by
 *     every call, so a call of another shape, another entry over the same workspace, or an index that shrank, grew or was
 *     replaced in between (live writes, compactions, rag_index_load_*, rag_index_reserve, an option flipped by rag_set_option)
 *     leaves nothing a later call can see - each call returns the bits it returns on a fresh handle in the same state
 *     (tests/test_call_history_gpu.py, tests/test_state_history_gpu.py; tests/test_workspace_table_cpu.py fails for a grow-only
 *     buffer that neither exercises).
 *   - doc ids are int64 (SQL BIGSERIAL ids, database/migrations/001_initial_schema.sql); scores are
 *     float64 because the reference computes every score as a Python float.
 */
#ifndef RAG_HIP_H
#define RAG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rag_ctx* rag_handle_t;

#define RAG_OK 0
#define RAG_ERR_ARG (-1)
#define RAG_ERR_HIP (-2)
#define RAG_ERR_STATE (-3)
#define RAG_ERR_NOMEM (-4)

/* ---- lifecycle ---------------------------------------------------------------------------- */
int rag_version(void);
int rag_device_count(int* n_out);
/* dim = embedding dimension (1536 for text-embedding-3-small, memory/embeddings.py:324-325). */
int rag_create(int device_id, int dim, rag_handle_t* out);
int rag_destroy(rag_handle_t h);
const char* rag_last_error(rag_handle_t h);
int rag_synchronize(rag_handle_t h);
/* Diagnostic / tuning switch of one handle (no reference counterpart). Every switch <name> takes its default from the
 * environment variable RAG_<NAME> ONCE, when rag_create runs; afterwards only this call changes it. Names: force_level,
 * stage_growth, no_smallq, no_second_pass, dense_linear_order, bm25_first_ranges, bm25_no_staging, bm25_packed, bm25_linear_grid, bm25_sort_merge, no_fork,
 * fork_max_q, bm25_plan_slots, bm25_ws_mb, bm25_tail_fold, bm25_keep_tf, sparse_tail_fold, tokvec_compact_rows, tokvec_scan_ws_mb, tokvec_scan_queries, ce_chunk_tokens, ce_mx, ce_attn_stream, ce_ffn_fused (DESIGN.md section 6;
 * ce_attn_stream: 0 = attention of 64-wide heads above length class 512 by the streamed kernel, -1 = by the global-memory form at
 * every class above 256, 1 = by the streamed kernel at every class above 512 whatever the default there - the same bits in all
 * three; ce_ffn_fused: the two FFN GEMMs of an MX layer as one launch (0 = where its per-workgroup slots fit
 * the cache, 1 = always, -1 = two launches) - the same bits in all three). Unknown name: RAG_ERR_ARG. */
int rag_set_option(rag_handle_t h, const char* name, int value);

/* ---- dense index: replaces the pgvector tables behind
 *      `ORDER BY dc.embedding <=> %s::vector LIMIT %s`  (rag/document_store.py:448-460)
 *      `ORDER BY embedding <=> %s::vector LIMIT %s`     (database/operations.py:126-137)
 * Rows are float32 (pgvector `vector(1536)` is float4). ids may be NULL (id = id_base + row).
 * Builds in HBM: fp32 master rows, fp16 unit-normalised rows (MFMA operand). Rows with a zero or
 * non-finite norm score 0.0 against every query (the reference's `return 0.0`, rag/retrieval.py:368-369).
 * ONLY those: every other float32 row or query - components that are all float32 denormals (norm down to 1e-45) up to
 * a norm just below float32 overflow - is normalised in float64 and gets the cosine the float64 scan gives it
 * (tests/test_dense_exactness_gpu.py sweeps 2^-140 ... 2^120; the device does not flush float32 denormals here). */
int rag_index_load_host(rag_handle_t h, const float* emb_host, const int64_t* ids_host, int64_t id_base,
                        int64_t n_rows);
int rag_index_load_dev(rag_handle_t h, const float* emb_dev, const int64_t* ids_dev, int64_t id_base,
                       int64_t n_rows, void* stream);
/* Chunked bulk load for shards that should not exist twice in memory (12.5M rows = 115 GB resident): reserve once,
 * append row blocks in order (host or device source), search at any time over the rows appended so far.
 * The bulk export of `document_chunks(id, agent_id, content, embedding)` (rag/document_store.py:210-221) maps onto
 * this directly. */
int rag_index_reserve(rag_handle_t h, int64_t n_rows_total, int64_t id_base);
int rag_index_append_host(rag_handle_t h, const float* emb_host, int64_t n_rows);
int rag_index_append_dev(rag_handle_t h, const float* emb_dev, int64_t n_rows, void* stream);
/* Optional multi-tenant filter: tenant_of_row[n_rows] (the `WHERE dc.agent_id = %s`,
 * rag/document_store.py:457). tenant < 0 in a search = no filter. */
int rag_index_set_tenants_host(rag_handle_t h, const int32_t* tenant_of_row_host, int64_t n_rows);
/* Explicit doc ids (e.g. the table's primary keys) for an index filled through rag_index_reserve/append: ids[n_rows],
 * n_rows == rows appended so far; NULL restores id = id_base + row. */
int rag_index_set_ids_host(rag_handle_t h, const int64_t* ids_host, int64_t n_rows);
int rag_index_rows(rag_handle_t h, int64_t* n_rows_out);

/* ---- live writes: the INSERT / DELETE the reference agent makes while it runs, without reloading the index.
 *      archival_memory_insert -> DatabaseOperations.insert_archival_memory (database/operations.py:22-57), the chunk inserts of
 *      DocumentStore.upload_and_index (rag/document_store.py:343-390), delete_document (:524-542), delete_archival_memory
 *      (database/operations.py:162-172, `WHERE id = %s AND agent_id = %s`).
 * Writes are synchronous and take the handle lock; each first waits for all work the handle's *_dev calls queued (on any
 * stream): a *_dev search queued before a write returns the result from before it.
 *
 * rag_index_insert_host: rows become searchable when the call returns, at rows [*first_row_out, +n). Per row: the float32
 * embedding, a doc id (ids may be NULL only on an implicit-id index, whose new rows then get id_base + row; the first insert
 * with explicit ids stores the id column), a tenant iff a tenant table is set, a temporal score iff temporal scores are set,
 * passage tokens [n][tok_L] + lens iff a token store is loaded (on an EMPTY index, tenants / temporal start those planes).
 * A missing plane, an id that is live already or repeated inside the block: RAG_ERR_ARG (the primary key of the SQL table).
 * Rows first fill the capacity rag_index_reserve left; past it every row-aligned plane grows (RAG_ERR_NOMEM when it cannot).
 * A failed insert leaves the index as it was. Inserting on a handle with no index creates one. Marks the BM25 postings stale.
 *
 * rag_index_delete_host: deletes the live rows whose id is in ids[n_ids] (and, tenant >= 0, whose tenant is `tenant`: the
 * `AND agent_id = %s`); *n_deleted_out = rows removed. Unknown / already deleted ids are not an error. Every search entry
 * point skips deleted rows (BM25 keeps the idf / avgdl of the loaded postings, normalises by the best live document;
 * rag_bm25_scores_host gives 0.0 for them); entry points that take explicit rows (fetch_rows, mmr_select_dev,
 * ce_build_pairs_dev) do not look. Results equal those of a fresh handle loaded with only the live rows, in row order.
 *
 * rag_index_compact: removes the deleted rows from every plane, stably and in place (at most 1 GiB of staging);
 * row_map_out[rows before] (may be NULL) = new row of each old row or -1, *n_rows_out = rows after. Doc ids never change
 * (an implicit-id index stores its ids first). Marks the BM25 postings stale.
 *
 * Stale postings: BM25 and hybrid entry points return RAG_ERR_STATE while the postings do not describe the current rows
 * (deletes do not make them stale). After inserts, rag_bm25_append_host of the new rows' postings makes them current again -
 * once EVERY inserted row is covered; after a rag_index_compact only rag_bm25_load_host of postings aligned with the new row
 * numbers does.
 *
 * rag_index_compact_bm25: rag_index_compact - the same arguments, the same effect on every row plane - that KEEPS the postings.
 * When postings are loaded and were describing the rows (no rag_index_compact since their load), they are renumbered through
 * the compaction's device row map and the postings of the deleted rows are dropped, base and tail both, before any row moves.
 * Afterwards every BM25 and hybrid result is BIT-IDENTICAL to a fresh handle that holds the live rows in row order and was
 * loaded with the compacted CSR (each term's surviving postings in order, renumbered), the same idf table (all terms known so
 * far), avgdl, k1 and b - and to what this handle returned immediately before the call, rows mapped through row_map_out
 * (deletes already hid the rows and froze the statistics). Term numbers never change; a term that loses every posting stays
 * in the vocabulary with an empty list and its idf.
 * Staleness is left as it was: postings that covered every row are current afterwards; if rows had been inserted but not yet
 * appended, the covered rows are remapped and the postings stay stale until rag_bm25_append_host of the remaining rows, in
 * their new order, covers them. After an earlier rag_index_compact (postings stale and compacted) the call behaves as
 * rag_index_compact: only a reload helps. Without postings, or with nothing deleted, it IS rag_index_compact (identity map;
 * postings, staleness and rag_bm25_segment_stats untouched).
 * Representation: base and tail are remapped SEPARATELY by a stable stream compaction of each posting array (no fold is
 * counted; `appends` survives): a bm25_packed base keeps its code bits and its table and gets new low document bits, the tail
 * stays a tail behind the new base size. base_docs + tail_docs = live covered rows, base_nnz + tail_nnz = surviving postings.
 * A tail without surviving rows is dropped; a base without surviving rows is replaced by the remapped tail (the (doc, impact)
 * form); when NO covered row survives there is nothing to keep and the postings end as after rag_index_compact.
 * Atomic: the new posting arrays, metadata and tables are allocated and built beside the old ones (the transient memory of
 * rag_bm25_fold) before the first row moves, and swapped in at the end: RAG_ERR_NOMEM leaves rows and postings as they were
 * (as in rag_index_compact, an index with implicit ids has had its ids plane written out by then: id = row, the same ids).
 * Synchronous, takes the handle lock, waits for queued *_dev work like every live write. Cost: the postings streamed twice on
 * the device; never a host rebuild or an upload of postings.
 *
 * rag_index_compact_live: rag_index_compact_bm25 - the same arguments, the same effect on every row plane and on the BM25
 * postings - that ALSO keeps the learned-sparse postings and the resident token-vector store.
 * Sparse postings: kept when they are loaded and were describing the rows (no rag_index_compact / rag_index_compact_bm25 since
 * their load). Base and tail are remapped separately through the device row map by the same stable stream compaction (the
 * float32 weights move as stored bits), postings of deleted rows are dropped, term numbers never change; a tail without
 * survivors is dropped, a base without survivors is replaced by the remapped tail, and when no covered row survives the
 * postings end as after rag_index_compact. Staleness is left as it was: rows inserted but not yet appended stay uncovered
 * until rag_sparse_append_host of the remaining rows, in their new order.
 * Token-vector store: documents [0, min(store documents, rows before)) move through the row map and a deleted document's rows
 * are dropped; documents the store holds at or past the index rows (a store filled ahead of the inserts) keep their order behind
 * the survivors. The offsets are rewritten, the document and row counts shrink - the freed rows are headroom of the same
 * reservation again - and the store is NOT marked stale. Vectors move as stored fp16 bits, in place, 16 bytes per lane, one
 * chunk of destination rows at a time through the compaction's staging buffer (option tokvec_compact_rows: token rows per
 * chunk, 0 = sized from the staging bound); beyond the store, the move needs 16 B per document (new offsets, first source
 * row), inside the 1 GiB staging bound whatever the store's size. A store that was stale already stays stale.
 * Atomic as rag_index_compact_bm25: the new posting arrays of both indexes, the store's new offsets and every workspace are
 * allocated and built beside the old ones before the first row of any plane moves and swapped in at the end; RAG_ERR_NOMEM
 * leaves rows, both posting sets and the store as they were. With nothing deleted the call moves and marks nothing.
 * Afterwards rag_sparse_*, rag_hybrid_sparse_rrf_dev, rag_tokvec_rerank_* (on mapped candidate rows) and rag_retrieve_maxsim_dev
 * are BIT-IDENTICAL to a fresh handle that holds the live rows in row order with the compacted sparse CSR and the surviving
 * documents' vectors loaded - and to what this handle returned immediately before the call, rows mapped through row_map_out.
 * rag_tokvec_fetch_host of every surviving document returns the bits it returned before. */
typedef struct rag_row_block {
    int64_t n;
    const float* emb;            /* [n][dim] */
    const int64_t* ids;          /* [n]; NULL only on an implicit-id index */
    const int32_t* tenants;      /* [n] (>= 0); required iff a tenant table is set */
    const double* temporal;      /* [n]; required iff temporal scores are set */
    const int32_t* tokens;       /* [n][tok_L]; required iff a token store is loaded */
    const int32_t* token_lens;   /* [n] */
} rag_row_block;
int rag_index_insert_host(rag_handle_t h, const rag_row_block* rows, int64_t* first_row_out);
int rag_index_delete_host(rag_handle_t h, const int64_t* ids, int64_t n_ids, int tenant, int64_t* n_deleted_out);
int rag_index_compact(rag_handle_t h, int64_t* row_map_out, int64_t* n_rows_out);
int rag_index_compact_bm25(rag_handle_t h, int64_t* row_map_out, int64_t* n_rows_out);
int rag_index_compact_live(rag_handle_t h, int64_t* row_map_out, int64_t* n_rows_out);
int rag_index_deleted_rows(rag_handle_t h, int64_t* n_deleted_out);

/* ---- id-to-row map: "which of my rows has this id?" on the device, for an index with explicit ids (the primary keys of a row
 *      shard that takes live writes). No reference counterpart: the reference asks PostgreSQL's primary-key index.
 * An open-addressing hash table in HBM with linear probing, an int64 key plane and an int32 row plane:
 *     home(id) = ((uint64_t)id * 0x9E3779B97F4A7C15) >> (64 - log2(slots))
 * slots is a power of two, at least 128 and at least twice the row capacity of the index, so live keys + tombstones stay at or
 * below slots / 2. Keys are ids >= 0 (-1 pads every list); an unused slot holds INT64_MIN. Erasing an id leaves a tombstone - the
 * key stays, its row becomes -1 - so probe chains stay intact, and inserting that id again takes its slot back. Which slot a key
 * occupies may depend on the order of the device's atomics; no lookup result does.
 *
 * rag_index_id_map: a host write (takes the lock, waits for queued *_dev work). enable = 1 builds the map now from the stored ids
 * of the live rows and keeps it maintained; enable = 0 frees it. On an index with implicit ids the call is legal and builds
 * nothing: lookups there are arithmetic on id_base. The build also decides ids_ascending: whether the ids of the live rows are
 * strictly ascending with the rows (implicit ids are). A duplicate live id or a negative id: RAG_ERR_ARG, the message names the
 * id, the map stays disabled. RAG_ERR_NOMEM changes nothing.
 * Maintenance, inside the existing writes, whose atomicity is unchanged: rag_index_insert_host adds the block's ids (ids must be
 * >= 0 while the map is enabled); when live keys + tombstones + n would pass slots / 2, or the grown row capacity asks for more
 * slots, a new table is allocated BEFORE anything is committed (a failed insert leaves index and map as they were) and built
 * from the whole id column afterwards - a rebuild, which also drops the tombstones; ids_ascending stays 1 only if the block
 * ascends and its first id is above the id of the last live row. rag_index_delete_host erases the ids it deleted. Every
 * rag_index_compact* and rag_index_set_ids_host rebuild the map and decide ids_ascending anew (between rebuilds it only ever goes
 * from 1 to 0); a duplicate or negative id given to rag_index_set_ids_host while the map is enabled: RAG_ERR_ARG, the ids are
 * set and the map is disabled. rag_index_load_* and rag_index_reserve replace the index and drop the map.
 * rag_index_append_host / _dev (rows of a reserved index, which carry no ids) leave the map as it is: the appended rows are unknown
 * to it, and entries does not count them, until rag_index_set_ids_host gives every row an id and rebuilds it.
 * With the map disabled every other entry makes exactly the launches it made without this section.
 *
 * rag_index_rows_of_ids_dev / _host: rows_out[i] = the row of ids[i], -1 for an unknown id, an id whose row is deleted, or a
 * negative id. One lane per id; a probe stops at the first unused slot. An index with explicit ids and no map: RAG_ERR_STATE. An
 * index with implicit ids: id - id_base where that is a live row. The _dev form is asynchronous on `stream` and ordered as the
 * preamble says.
 *
 * rag_index_id_map_info: host state only, waits for nothing. entries = live keys; longest_probe = the longest chain walked by
 * the last build or insert (1 = every key at home); hbm_bytes = 12 * slots; rebuilds counts the rebuilds since the map was
 * enabled. Implicit ids: slots = entries = 0, ids_ascending = 1. Disabled: all zero. */
typedef struct rag_id_map_info {
    int32_t enabled, ids_ascending;
    int64_t slots, entries, tombstones, longest_probe, hbm_bytes, rebuilds;
} rag_id_map_info;
int rag_index_id_map(rag_handle_t h, int enable);
int rag_index_rows_of_ids_dev(rag_handle_t h, const int64_t* ids_dev, int64_t n, int32_t* rows_out_dev, void* stream);
int rag_index_rows_of_ids_host(rag_handle_t h, const int64_t* ids_host, int64_t n, int32_t* rows_out_host);
int rag_index_id_map_info(rag_handle_t h, rag_id_map_info* out);
/* copy rows' fp32 embeddings back (kills apply_mmr's per-doc re-embedding, rag/nodes/helpers.py:215-223) */
int rag_index_fetch_rows_host(rag_handle_t h, const int64_t* rows_host, int n, float* out_host);

/* Exact cosine top-k over the resident index, Q queries at once.
 * Result = what an un-indexed `ORDER BY embedding <=> q LIMIT k` returns: cosine descending, ties by
 * lower row first; ids_out[Q*k] (-1 padded), rows_out[Q*k] local row numbers (may be NULL),
 * scores_out[Q*k] = 1 - distance as float64. Identical id sets to the float64 exact scan hold BY CONSTRUCTION:
 * the fp16 MFMA pass only discards rows whose score is more than 2*eps below the k-th best (eps = proven bound on
 * the fp16 error), survivors are rescored in float64; a float64 scan of every row is the overflow fallback.
 * eps (rag_dense_stats.eps) is pinned by tests on worst-case rows whose fp16 products all err the same way: they reach
 * max |fp16 score - cosine| = 0.85 eps at dim 64, 0.76 at dim 100, 0.78 at dim 384, 0.68 at dim 1536, and put a row of
 * the exact top-k 1.29 to 1.49 eps below the k-th best fp16 score (tests/fp16_adversary.py).
 * Alignment, ONE rule for every *_dev entry: a caller array that a kernel reads or writes through a type wider than its element
 * is marked "16-byte aligned" where it is declared, and the entry refuses any other address with RAG_ERR_ARG and a message
 * naming the array before it enqueues anything (tests/test_output_bounds_gpu.py). That is the float32 query matrix of every
 * dense-backed search - q_dev [Q][dim] of rag_dense_topk_dev, rag_hybrid_rrf_dev, rag_hybrid_sparse_rrf_dev, rag_hybrid_linear_dev,
 * rag_hybrid_linear_finish_dev, q_emb_dev of rag_retrieve_rerank_dev, rag_retrieve_maxsim_dev, rag_retrieve_m3_dev and of
 * rag_m3_score_rows_dev / rag_m3_score_ids_dev under a dense weight, and their _tenants forms: rows are read as float4; dim is a
 * multiple of 4, so every row of an aligned matrix is aligned - and the token-vector arrays (q_vecs, d_vecs of rag_maxsim_dev, the
 * q_vecs of the rag_tokvec_rerank / rag_retrieve_maxsim / m3 entries). Every other array, inputs and outputs alike, is read and
 * written element by element and needs its element's alignment only: emb_dev of rag_index_load_dev / rag_index_append_dev (copied
 * by the runtime before any kernel reads it), q_dev of rag_mmr_select_dev, vecs_dev of rag_tokvec_append_dev, every token-id,
 * length, term, weight and candidate array, and EVERY output array. Host pointers have no rule beyond the element's.
 * q_dev: float32 [Q][dim], 16-byte aligned. */
int rag_dense_topk_host(rag_handle_t h, const float* q_host, int n_queries, int k, int tenant,
                        int64_t* ids_out_host, int32_t* rows_out_host, double* scores_out_host);
int rag_dense_topk_dev(rag_handle_t h, const float* q_dev, int n_queries, int k, int tenant,
                       int64_t* ids_out_dev, int32_t* rows_out_dev, double* scores_out_dev, void* stream);

/* Counters of the last dense search (device counters are read back: synchronises). */
typedef struct rag_dense_stats {
    int32_t n_queries;
    int32_t proven_fast;      /* <= 256 survivors above tau: ranked in the fast path (exact by construction) */
    int32_t proven_wide;      /* more survivors (clusters, duplicates): ranked by the wide kernel            */
    int32_t exact_scan;       /* buffer overflowed in the second pass too: float64 scan of every row         */
    int32_t overflowed;       /* overflow events (any stage of the first pass)                               */
    int32_t shortlist;        /* k (the threshold is the k-th best score so far minus 2*eps)                 */
    int32_t stages;           /* threshold stages used                  */
    int32_t second_pass;      /* overflowed queries whose re-emission at the final threshold fitted the buffer */
    double eps;               /* rigorous |fp16 score - exact| bound    */
} rag_dense_stats;
int rag_dense_last_stats(rag_handle_t h, rag_dense_stats* out);

/* Names/launch geometry of the dominant kernel of the last dense search, for bench.py's roofline. */
int rag_dense_kernel_ms(rag_handle_t h, float* gemm_ms_out, int* gemm_launches_out);
int rag_set_profiling(rag_handle_t h, int enable);
/* Measurement hook (bench.py's rooflines; the reference has nothing to mirror): with profiling on, HIP event pairs are
 * recorded on the launch stream around stage 0 = every thresholded dense GEMM launch (== rag_dense_kernel_ms),
 * 1 = the BM25 posting-range + merge launches of each top-k call, 2 = each cross-encoder forward. Returns the summed
 * device time and the number of spans since profiling was (re)enabled; synchronises on the spans' end events. */
int rag_stage_kernel_ms(rag_handle_t h, int stage, float* ms_out, int* spans_out);

/* ---- merge of per-shard partial top-k lists (multi-GPU exchange step).
 * list l lives at ids_dev + l*list_stride / scores_dev + l*list_stride, each [Q][k] (ids int64, scores
 * float64, -1 padded); list_stride is in elements (Q*k when the lists are contiguous, 2*Q*k for an
 * all-gathered [rank][ids|scores][Q][k] buffer). Output [Q][k] by score desc, id asc. */
int rag_merge_topk_dev(rag_handle_t h, const int64_t* ids_dev, const double* scores_dev, int n_lists,
                       int64_t list_stride, int n_queries, int k, int64_t* ids_out_dev, double* scores_out_dev,
                       void* stream);

/* The fuse step of the row-sharded HYBRID search on every rank, after the one all-gather:
 * gathered_dev = [world][4][Q][pool] int64 = every rank's dense ids | dense cosines (float64 bits) | BM25 ids | RAW BM25
 * scores (float64 bits; rag_bm25_set_normalize(h, 0) on the shards). Merges the dense lists and the BM25 lists (score desc,
 * id asc), divides the merged BM25 scores by their GLOBAL maximum (when > 0, else 1.0: rag/retrieval.py:343-345 - the
 * shards cannot know it), then fuses the two MERGED lists with RRF (rag/reranker.py:224-271; RRF needs global ranks).
 * lists_out_dev [2][Q][pool] int64 = merged dense ids | merged BM25 ids, scores_out_dev [2][Q][pool] float64 = cosines |
 * normalised BM25; keys / rrf / ranks as rag_rrf_fuse_dev with n_lists = 2. Bit-identical to rag_hybrid_rrf_dev on the
 * unsharded index. */
int rag_hybrid_fuse_gathered_dev(rag_handle_t h, const int64_t* gathered_dev, int world, int n_queries, int pool, int k,
                                 int rrf_k, int64_t* lists_out_dev, double* scores_out_dev, int64_t* keys_out_dev,
                                 double* rrf_out_dev, int32_t* ranks_out_dev, void* stream);

/* ---- small pairwise cosine in float64: replaces the Python loops
 *      rag/consistency_checker.py:169-176, rag/context_compressor.py:227-228, rag/reranker.py:167-175,
 *      rag/nodes/helpers.py:232-243, rag/retrieval.py:253-256.  out[m*n] row-major, 0.0 on zero norm. */
int rag_pairwise_cosine_host(rag_handle_t h, const float* a_host, int m, const float* b_host, int n, int dim,
                             double* out_host);
/* the same on float64 inputs: the reference multiplies Python doubles (rag/retrieval.py:362-371), so the mirror classes hand the
 * agent's List[float] over unrounded - a pair sitting exactly on ConsistencyChecker's `>= 0.85` (rag/consistency_checker.py:179)
 * must not flip because its inputs were cast to float32 first. */
int rag_pairwise_cosine_f64_host(rag_handle_t h, const double* a_host, int m, const double* b_host, int n, int dim,
                                 double* out_host);

/* ---- reciprocal rank fusion: replaces ReciprocalRankFusion.fuse (rag/reranker.py:224-271).
 * lists_host: [Q][n_lists][list_len] int64 keys, -1 = padding (only at the tail of a list).
 * For each query: score[key] += 1.0/(rrf_k+rank) (rank from 1, list order), sort desc, first-seen
 * order on ties, top_k. Outputs -1 padded; ranks_out[Q][top_k][n_lists] = 1-based rank of the key's first
 * occurrence in each list (0 = absent) (may be NULL).
 * n_lists * list_len <= 1024 items per query (more: RAG_ERR_ARG); keys are any int64 >= 0; list_len = 0 is legal (nothing
 * to fuse, nothing is read: all outputs are padding); top_k may exceed the number of distinct keys. */
int rag_rrf_fuse_host(rag_handle_t h, const int64_t* lists_host, int n_queries, int n_lists, int list_len,
                      int rrf_k, int top_k, int64_t* keys_out_host, double* scores_out_host,
                      int32_t* ranks_out_host);

/* Device-pointer forms of the fusion / BM25 entry points (asynchronous on `stream`), and the whole hybrid path of
 * BASELINE.json configs[2] in one call: dense top-`pool` + BM25 top-`pool` -> RRF(rrf_k) -> top-k, nothing leaves HBM.
 * rag_rrf_fuse_dev: lists_dev is [Q][n_lists][list_len]. rag_hybrid_rrf_dev: q_dev float32 [Q][dim], 16-byte aligned (else
 * RAG_ERR_ARG, as in rag_dense_topk_dev); lists_ws_dev is caller scratch
 * [2][Q][pool] int64, scores_ws_dev [Q][pool] float64; keys are doc ids (BM25 rows use the dense index's id mapping,
 * the two indexes must be row-aligned). For batches of up to 4096 queries the BM25 leg of rag_hybrid_rrf_dev / rag_retrieve_rerank_dev
 * runs on an internal side stream that is forked from and joined back into `stream` by events: everything the call
 * reads and writes is still ordered on `stream` as if it had run there alone. */
int rag_rrf_fuse_dev(rag_handle_t h, const int64_t* lists_dev, int n_queries, int n_lists, int list_len, int rrf_k,
                     int top_k, int64_t* keys_out_dev, double* scores_out_dev, int32_t* ranks_out_dev, void* stream);
int rag_bm25_topk_dev(rag_handle_t h, const int32_t* term_ptr_dev, const int32_t* terms_dev, int n_queries, int k,
                      int tenant, int64_t* ids_out_dev, int32_t* rows_out_dev, double* scores_out_dev,
                      double* raw_max_out_dev, void* stream);
int rag_hybrid_rrf_dev(rag_handle_t h, const float* q_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                       int n_queries, int pool, int k, int rrf_k, int tenant, int64_t* lists_ws_dev,
                       double* scores_ws_dev, int64_t* keys_out_dev, double* rrf_out_dev, int32_t* ranks_out_dev,
                       void* stream);

/* ---- learned-sparse inverted index: weighted top-k and dense + sparse RRF. No reference counterpart: the reference has no
 * learned-sparse retrieval. The semantics are restated from FlagEmbedding's bge-m3 lexical matching / SPLADE practice (a
 * document is a {token id: weight} map, a query too, the score is the sum of the products over the shared tokens); parity with
 * those upstream implementations is NOT pinned by a test here.
 * The index lives in a slot of its own beside the BM25 postings (both may be resident) and runs the BM25 machinery - term-major
 * postings, one workgroup per (query, 2048-document range) with float64 accumulators in LDS, bracket tables, the per-call plan,
 * staged thresholds, the merges - on another posting form: (doc int32, weight float32), 8 B per posting resident (an int32
 * plane and a float32 plane) plus 32 B per term and the bracket tables (<= 4 B per 4 postings).
 * rag_sparse_load_host: term-major CSR, indptr_host[n_terms + 1] from 0, the documents of a term strictly ascending in
 *   [0, n_docs), weights finite and > 0; empty lists are legal. A term number is whatever the caller's vocabulary says (bge-m3:
 *   the token id, n_terms = 250,002). A malformed CSR, a weight that is not finite or <= 0, n_docs < 1 or n_terms < 1:
 *   RAG_ERR_ARG, and the resident postings stay as they were. A second load replaces the first. Synchronous; takes the
 *   handle lock and waits for queued *_dev work like every host write.
 * rag_sparse_info: documents, terms, postings and HBM bytes of the resident sparse index (all 0: none loaded).
 * Score: s(q, d) = sum_i (double)qweights[i] * (double)weight[terms[i], d] in float64, over the query's tokens in THEIR ORDER
 *   on the documents that hold the term. A float32 x float32 product is exact in float64, so the only rounding is the sum,
 *   and its order is fixed: every score bit equals the numpy loop `score[doc[a:e]] += float64(qw) * w[a:e].astype(float64)`
 *   run token by token. terms[i] < 0 or >= n_terms adds nothing; a token whose weight is not > 0 (NaN included) adds nothing;
 *   a term that occurs twice adds twice. Queries are CSR as for BM25: term_ptr[Q + 1], terms[], qweights[] parallel to terms[].
 * rag_sparse_topk_host / _dev: the documents with s > 0 by score descending, ties to the lower row, at most k; the rest of the
 *   k slots is ids -1 / rows -1 / scores 0.0. A document that matches nothing is NEVER returned (rag_bm25_topk_* returns
 *   zero-score rows because it mirrors a sort over the whole corpus; here they would pollute a fusion). Scores are raw.
 *   Limits: 1 <= n_queries <= 65535, 0 < k <= 1024, as rag_bm25_topk_*. rows_out may be NULL.
 *   When the postings cover exactly the dense index's rows, ids follow the index's id mapping (explicit ids or id_base + row),
 *   tenant >= 0 keeps that tenant's rows and deleted rows are hidden, as in BM25 (a hidden row is an empty slot). Without
 *   such an index ids are row numbers and tenant >= 0 is RAG_ERR_ARG.
 * rag_sparse_scores_host: out_host[Q][n_docs], every document's score, 0.0 for non-matching and hidden documents (small
 *   corpora, tests).
 * Live writes: rag_index_insert_host, rag_index_compact and rag_index_compact_bm25 leave the sparse postings STALE: every
 *   rag_sparse_* search and rag_hybrid_sparse_rrf_dev returns RAG_ERR_STATE until rag_sparse_load_host runs again (the handle
 *   stays usable; a compaction that finds no deleted row moves nothing and marks nothing). rag_index_delete_host does not:
 *   deleted rows are filtered. After inserts, rag_sparse_append_host (below, behind rag_bm25_segments) makes the postings
 *   current again; rag_index_compact_live renumbers them with the rows. A tenant per query: rag_sparse_topk_tenants_* and
 *   rag_hybrid_sparse_rrf_tenants_dev ("a tenant PER QUERY" below).
 * rag_hybrid_sparse_rrf_dev: rag_hybrid_rrf_dev with the sparse list in place of the BM25 list - dense top-`pool` and sparse
 *   top-`pool` (-1 padded at the tail), rag_rrf_fuse_dev semantics with n_lists = 2, dense first, top-k. Workspaces and limits
 *   as rag_hybrid_rrf_dev (q_dev 16-byte aligned; pool <= 256; lists_ws_dev [2][Q][pool] int64, scores_ws_dev [Q][pool]
 *   float64); the postings must be row-aligned with the index. Bit-identical to rag_dense_topk_dev + rag_sparse_topk_dev +
 *   rag_rrf_fuse_dev called one after another. The sparse leg forks onto the internal side stream as the BM25 leg of rag_hybrid_rrf_dev does (batches
 *   of up to 4096 queries; options no_fork / fork_max_q), joined back by events: everything is ordered on `stream`.
 * The _dev calls follow the ordering rules of the preamble.
 * Sharding: raw scores need no global statistic, so rag_merge_topk_dev over the per-shard lists (global ids through id_base
 *   or explicit ids) reproduces the unsharded list exactly. */
int rag_sparse_load_host(rag_handle_t h, const int64_t* indptr_host /*n_terms+1*/, const int32_t* doc_host /*nnz*/,
                         const float* weight_host /*nnz*/, int64_t n_docs, int64_t n_terms);
int rag_sparse_info(rag_handle_t h, int64_t* n_docs_out, int64_t* n_terms_out, int64_t* nnz_out, int64_t* hbm_bytes_out);
int rag_sparse_topk_host(rag_handle_t h, const int32_t* term_ptr_host /*Q+1*/, const int32_t* terms_host,
                         const float* qweights_host, int n_queries, int k, int tenant, int64_t* ids_out,
                         int32_t* rows_out /*may be NULL*/, double* scores_out);
int rag_sparse_topk_dev(rag_handle_t h, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev,
                        int n_queries, int k, int tenant, int64_t* ids_out_dev, int32_t* rows_out_dev /*may be NULL*/,
                        double* scores_out_dev, void* stream);
int rag_sparse_scores_host(rag_handle_t h, const int32_t* term_ptr_host, const int32_t* terms_host,
                           const float* qweights_host, int n_queries, double* out_host /*[Q][n_docs]*/);
int rag_hybrid_sparse_rrf_dev(rag_handle_t h, const float* q_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                              const float* qweights_dev, int n_queries, int pool, int k, int rrf_k, int tenant,
                              int64_t* lists_ws_dev, double* scores_ws_dev, int64_t* keys_out_dev, double* rrf_out_dev,
                              int32_t* ranks_out_dev, void* stream);

/* ---- greedy MMR selection on the device: replaces the Python loops of
 *      MMRDiversifier.diversify (rag/reranker.py:116-195; variant 0: lambda*rel + (1-lambda)*(1-max_sim), first pick has
 *      diversity 1.0) and apply_mmr (rag/nodes/helpers.py:183-260; variant 1: lambda*rel - (1-lambda)*max_sim).
 *      First maximal candidate wins ties, float64 throughout. n (pool) <= 256. sel_out = positions into the candidate
 *      list (-1 padded when fewer than top_k candidates), score_out = the MMR score each pick won with.
 *      _host: explicit candidate embeddings emb[n][dim]. _dev: candidates are rows of the resident index
 *      (rows_dev[Q][pool], -1 = empty), queries q_dev[Q][dim]; embeddings never leave HBM. */
int rag_mmr_select_host(rag_handle_t h, const float* query_host /*dim*/, const float* emb_host /*n x dim*/, int n, int dim,
                        int top_k, double lambda, int variant, int32_t* sel_out_host, double* score_out_host);
int rag_mmr_select_dev(rag_handle_t h, const float* q_dev, const int32_t* rows_dev, int n_queries, int pool, int top_k,
                       double lambda, int variant, int32_t* sel_out_dev, double* score_out_dev, void* stream);

/* ---- semantic chunker chain: replaces the sentence loop of SemanticChunker.chunk
 *      (rag/chunking.py:153-199): sentence i joins the running chunk when cos(running pairwise average, e_i) >= threshold
 *      and the chunk stays <= max_chunk characters, else the chunk closes if it has >= min_chunk characters (otherwise
 *      the sentence is absorbed). emb[n][dim] sentence embeddings, sent_len[n] = len(sentence);
 *      group_out[n] = chunk number of each sentence. n >= 1, 1 <= dim <= 8192 (the running average lives in LDS as
 *      float64: 64 KiB at the limit), else RAG_ERR_ARG. */
int rag_chunk_chain_host(rag_handle_t h, const float* emb_host, const int32_t* sent_len_host, int n, int dim,
                         double threshold, int max_chunk, int min_chunk, int32_t* group_out_host);

/* ---- BM25 over CSR postings: replaces BM25Okapi(tokenized_corpus).get_scores(query) + the /max
 *      normalisation (rag/retrieval.py:324-347). Postings are term-major CSR, docs ascending per term.
 *      idf[V] is computed by the host exactly as rank-bm25 does (float64). */
int rag_bm25_load_host(rag_handle_t h, const int64_t* indptr_host /*V+1*/, const int32_t* doc_host /*nnz*/,
                       const int32_t* tf_host /*nnz*/, const int32_t* doc_len_host /*N*/,
                       const double* idf_host /*V*/, int64_t n_docs, int64_t n_terms, double avgdl,
                       double k1, double b);
/* ---- appendable postings: BM25 and hybrid search stay live through rag_index_insert_host without re-uploading the CSR.
 * rag_bm25_append_host takes the postings of the NEXT n_docs_new rows after the rows the resident postings cover: a term-major
 * CSR over the handle's vocabulary (indptr[n_terms_total + 1], docs ascending per term and RELATIVE to the block's first row,
 * doc_len[n_docs_new]). Term numbers at or above the number of terms known so far are new terms; idf_new[n_terms_total - known]
 * are their idf values; n_terms_total may not shrink. STATISTICS ARE FROZEN at the last rag_bm25_load_host (or rag_bm25_refresh, below): avgdl, k1, b and the
 * idf of every known term keep their loaded values (the rule deletes follow), a new term keeps the idf it arrived with; a caller
 * who wants fresh statistics reloads. After any sequence of appends every BM25 and hybrid result is BIT-IDENTICAL to a fresh
 * handle that holds the same rows and was loaded with the merged CSR (all rows; each term's list = its old list followed by the
 * new postings), the concatenated idf table and the same avgdl, k1, b.
 * Synchronous, takes the handle lock, waits for queued *_dev work like every host write. RAG_ERR_STATE without loaded postings;
 * RAG_ERR_ARG for n_docs_new < 1, a malformed CSR, or a block that would cover more rows than a loaded dense index has (without
 * a dense index appends are always allowed); RAG_ERR_NOMEM when it cannot allocate. A failed append leaves postings, coverage
 * and staleness exactly as they were. The postings stop being stale exactly when, after the call, the covered rows equal the
 * index rows and nothing but inserts happened since they were last aligned (5 rows inserted, 3 appended: still stale).
 * Representation: the loaded postings (the base) are never touched; ONE tail segment holds every appended row and is rebuilt on
 * the device by each append - cost O(tail), never O(base) - always in the (doc, impact) form, also behind a bm25_packed base
 * (the two forms give the same float64 product). Every search scores base and tail as one index.
 * rag_bm25_fold merges the tail into the base on the device (per-term concatenation, tables rebuilt); results before and after
 * are bit-identical. It needs transient memory for the merged arrays: RAG_ERR_NOMEM changes nothing. RAG_ERR_STATE on a
 * bm25_packed base (the packed code table cannot absorb new (tf, length) pairs). Option bm25_tail_fold: > 0 = an append folds
 * by itself once the tail holds more than that many documents, -1 = never, 0 = the default policy. */
typedef struct rag_bm25_segments {
    int64_t base_docs, tail_docs, base_nnz, tail_nnz, n_terms, tail_bytes, appends, folds;
} rag_bm25_segments;
int rag_bm25_append_host(rag_handle_t h, const int64_t* indptr_host /*n_terms_total+1*/, const int32_t* doc_host,
                         const int32_t* tf_host, const int32_t* doc_len_host /*n_docs_new*/,
                         const double* idf_new_host /*n_terms_total - terms known so far*/, int64_t n_docs_new,
                         int64_t n_terms_total);
int rag_bm25_fold(rag_handle_t h);
int rag_bm25_segment_stats(rag_handle_t h, rag_bm25_segments* out);
/* ---- appendable learned-sparse postings: the rag_sparse_* searches, rag_hybrid_sparse_rrf_dev and rag_retrieve_maxsim_dev
 * mode 1 stay live through rag_index_insert_host. The same machinery as the BM25 append, over the sparse slot.
 * rag_sparse_append_host takes the postings of the NEXT n_docs_new rows after the rows the resident sparse postings cover: a
 * term-major CSR over the handle's vocabulary (indptr[n_terms_total + 1] from 0, documents strictly ascending per term and
 * RELATIVE to the block's first row, weights finite and > 0). n_terms_total may grow - new terms have empty base lists - and may
 * not shrink. Everything is validated on the host before anything is built: RAG_ERR_STATE without loaded sparse postings;
 * RAG_ERR_ARG for n_docs_new < 1, a malformed block, a weight that is not finite or <= 0, or a block that would cover more
 * rows than a loaded dense index has; RAG_ERR_NOMEM when it cannot allocate. A rejected or failed append leaves postings,
 * coverage and staleness exactly as they were. The postings stop being stale exactly when, after the call, the covered rows
 * equal the index rows and nothing but inserts happened since they were last aligned (5 rows inserted, 3 appended: still stale).
 * Representation: the loaded postings (the base) are never touched; ONE tail segment of the same form (int32 document plane,
 * float32 weight plane, idf 1.0, its own bracket tables) holds every appended row and is rebuilt on the device by each append
 * in O(tail). The tail is numbered from the base's last 2048-document range, so one search scores base and tail as one index.
 * After any sequence of appends and folds every result of rag_sparse_topk_* (with and without a tenant), rag_sparse_scores_host,
 * rag_hybrid_sparse_rrf_dev and rag_retrieve_maxsim_dev mode 1 is BIT-IDENTICAL to a fresh handle that holds the same rows and
 * was loaded by rag_sparse_load_host with the merged CSR (each term's list = its old list followed by the new postings): a
 * document lives in one segment only, so its float64 accumulator receives the same products in the same token order.
 * rag_sparse_fold merges the tail into the base on the device; results before and after are bit-identical; RAG_ERR_NOMEM
 * changes nothing. Option sparse_tail_fold has the meaning of bm25_tail_fold. rag_sparse_segment_stats reports the segments
 * (n_terms: terms known so far; tail_bytes: HBM bytes of the tail); rag_sparse_info reports base and tail together. */
int rag_sparse_append_host(rag_handle_t h, const int64_t* indptr_host /*n_terms_total+1*/, const int32_t* doc_host,
                           const float* weight_host, int64_t n_docs_new, int64_t n_terms_total);
int rag_sparse_fold(rag_handle_t h);
int rag_sparse_segment_stats(rag_handle_t h, rag_bm25_segments* out);
/* ---- the same append from a DOC-MAJOR block, on the device: the layout rag_lexical_compact_dev writes (doc_ptr int32
 * [n_docs_new + 1] from 0, each document's terms strictly ascending, float32 weights finite and > 0; nnz_cap: the capacity of
 * terms / weights). The library transposes it to the term-major block of rag_sparse_append_host on the device - a check and
 * count pass, a scan, and a stable counting sort over the term number, 6 bits a pass, so the result is the permutation
 * np.argsort(term * n + document, kind="stable") whatever the launch order - and only the per-term offsets (n_terms_total + 2
 * int64) come back to the host, where every segment is planned; no posting crosses PCIe.
 * rag_sparse_append_dev is a host WRITE that takes device memory: it waits for `stream` (the block's producer), takes the
 * handle's lock, waits for queued *_dev calls as every *_host write does, and returns once the postings are resident and
 * checked - the rules of rag_tokvec_append_dev. With postings resident every later result is BIT-IDENTICAL to
 * rag_sparse_append_host called with the transposed block (and so to a fresh handle loaded with the merged CSR); coverage,
 * staleness, vocabulary growth, option sparse_tail_fold and the automatic fold are that call's. WITHOUT sparse postings the
 * block becomes the base: rag_sparse_load_host of its transpose with n_docs = n_docs_new. A block of empty documents is legal.
 * RAG_ERR_ARG: n_docs_new < 1, a null array, doc_ptr[0] != 0, a decreasing offset, doc_ptr[n_docs_new] > nnz_cap (the producer
 * cut the block at its capacity), a term outside [0, n_terms_total), terms not strictly ascending inside a document, a weight
 * that is not finite or not > 0 (the message names the first fault and its position), a shrinking n_terms_total, a block that
 * would cover more rows than a loaded dense index has, 2^31 rows. RAG_ERR_NOMEM when it cannot allocate. A rejected or failed
 * call leaves postings, coverage, staleness and segment statistics exactly as they were.
 * rag_sparse_append_docs_host takes the same block from host arrays, staged and run through the same device path.
 * rag_sparse_clear drops the resident sparse postings (OK when there are none).
 * rag_sparse_export_host reads the resident postings back as ONE term-major CSR - per term the base list, then the tail's,
 * with global document numbers: indptr_out [n_terms + 1], doc_out / weight_out [nnz]. Called with the three arrays NULL it only
 * reports n_docs, n_terms and nnz (any of them may be NULL). RAG_ERR_STATE when nothing is loaded. It is how an index built on
 * the device is saved or re-sharded. */
int rag_sparse_append_dev(rag_handle_t h, const int32_t* doc_ptr_dev /*n_docs_new+1*/, const int32_t* terms_dev, const float* weights_dev,
                          int64_t n_docs_new, int64_t nnz_cap, int64_t n_terms_total, void* stream);
int rag_sparse_append_docs_host(rag_handle_t h, const int32_t* doc_ptr_host /*n_docs_new+1*/, const int32_t* terms_host,
                                const float* weights_host, int64_t n_docs_new, int64_t nnz_cap, int64_t n_terms_total);
int rag_sparse_clear(rag_handle_t h);
int rag_sparse_export_host(rag_handle_t h, int64_t* indptr_out, int32_t* doc_out, float* weight_out, int64_t* n_docs_out,
                           int64_t* n_terms_out, int64_t* nnz_out);
/* ---- statistics refresh: fresh idf / avgdl computed from, and written into, the RESIDENT postings. The reference builds a new
 * BM25Okapi over the corpus it has on every call (rag/retrieval.py:333-341); appends, deletes and compactions keep the
 * statistics of the last load instead, so an index that has doubled or lost a tenant ranks by numbers no rebuild would give.
 * Nothing larger than the per-term tables crosses PCIe.
 * Opt-in: option bm25_keep_tf (read by rag_bm25_load_host; default 0 = nothing below is kept and all three calls return
 * RAG_ERR_STATE). With it an unpacked base and the tail keep a uint16 term-frequency plane beside their (doc, impact) planes
 * (+2 B per posting; a term frequency above 65535 is RAG_ERR_ARG at load / append, the call changes nothing), every segment the
 * int32 length of its documents (+4 B per document), a bm25_packed base its two value tables (a few KB). Append, fold and
 * rag_index_compact_bm25 move these with the postings, through the same kernels and with the same atomicity. Search results
 * with the option set are bit-identical to the option off until a refresh runs.
 * rag_bm25_live_counts_host: counts over the LIVE covered documents (covered by the postings and not deleted - the predicate
 * every search applies; a standalone BM25 handle has no deleted rows): df_out[n_terms] (int32) = live postings of each term,
 * base and tail together (n_terms as rag_bm25_segment_stats reports it), the live documents N and the exact sum of their
 * lengths. Any output may be NULL. No live document is not an error here (all zero).
 * rag_bm25_set_statistics_host: installs idf[n_terms] and avgdl: every impact of base and tail is recomputed from the kept
 * tf / doc_len by the arithmetic of the load (a packed base: its impact table), and the per-term idf, avgdl and the
 * negative-idf bound of the linear fusion follow. Afterwards every BM25 and hybrid result is BIT-IDENTICAL to a fresh handle
 * that holds the same rows with the same deletes and was loaded with the merged CSR, this idf, this avgdl and the same k1, b.
 * Offsets, bracket tables and the order of the postings are untouched; postings of deleted rows are rewritten like the rest and
 * stay hidden. Later appends, folds and compactions keep their contracts with "frozen" meaning "as of the last load or refresh".
 * rag_bm25_refresh: both, with the idf rule of rank-bm25 0.2.2 in between, on the host in float64 with libm's log (the table is
 * bit-equal to Python's math.log arithmetic): for every term with df >= 1, ln(N - df + 0.5) - ln(df + 0.5); mean = their
 * left-to-right sum in term-number order over their count (negative values included); every negative value becomes
 * epsilon * mean. A term with df = 0 (it lost every posting to deletes) keeps its number, gets ln(N + 0.5) - ln(0.5) and
 * stays out of the mean (rank-bm25 would not know it). avgdl = sum of the live lengths / N. idf_out[n_terms] and info_out may be
 * NULL. The two halves exist on their own for row-sharded indexes (each rank counts, the sums are installed on every rank) and
 * for callers with another idf rule.
 * All three are synchronous, take the handle lock and wait for queued *_dev work like every host write. RAG_ERR_STATE: no
 * postings, postings loaded without bm25_keep_tf, stale postings, (refresh) no live covered document. RAG_ERR_ARG: a non-finite
 * epsilon, avgdl <= 0 or not finite, a non-finite idf. RAG_ERR_NOMEM: the scratch (df + idf, 12 B per term) cannot be had - it is
 * allocated before the first impact is overwritten. Any error return leaves postings and statistics as they were. */
typedef struct rag_bm25_refresh_info {
    int64_t n_docs_live, nnz_live, n_terms, terms_without_postings, negative_idf_terms;
    double avgdl_before, avgdl_after, idf_max_abs_change;
} rag_bm25_refresh_info;
int rag_bm25_live_counts_host(rag_handle_t h, int32_t* df_out_host /*n_terms*/, int64_t* n_docs_live_out, int64_t* sum_doc_len_out);
int rag_bm25_set_statistics_host(rag_handle_t h, const double* idf_host /*n_terms*/, double avgdl);
int rag_bm25_refresh(rag_handle_t h, double epsilon, double* idf_out_host /*n_terms*/, rag_bm25_refresh_info* info_out);
/* HBM bytes rag_bm25_load_host will take for a CSR with these offsets, computed on the host from indptr alone (no GPU call):
 * postings (doc id + float64 impact, 12 B each; 8 B with option bm25_packed: the impact is then idf * g[code of the posting's
 * (term frequency, document length) pair] - bit-identical, less HBM, a slower scoring loop), per-term metadata (32 B each) and
 * the per-term bracket tables that replace
 * a binary search of the posting list per (query token, 2048-document range). A term's table is sized by its document
 * frequency, so table bytes <= postings/12 for ANY vocabulary - the reference tokeniser (`doc.lower().split()`,
 * rag/retrieval.py:334-335) produces millions of distinct terms on a large shard. Lets a loader budget a shard before
 * uploading it. Any of the outputs may be NULL. */
/* (Option bm25_keep_tf is not counted here: it adds 2 B per posting - none for a bm25_packed base - and 4 B per document.) */
int rag_bm25_index_bytes(const int64_t* indptr_host, int64_t n_docs, int64_t n_terms, int64_t* postings_bytes_out,
                         int64_t* meta_bytes_out, int64_t* table_bytes_out);
/* Launch geometry of ONE scoring launch over `n_ranges_in_launch` 2048-document ranges and `n_queries` queries (host-only, no GPU
 * call; no reference counterpart: the reference scores a query with one numpy pass, rag/retrieval.py:341). out5 = {workgroups,
 * ranges, queries, query groups per range G, queries per group L}. L = 0: workgroup b scores (range b % ranges, query b / ranges).
 * L > 0 (from 128 queries on): XCD-aware columns - workgroup b belongs to XCD x = b % 8 and is its s = b / 8 -th; it scores column
 * c = x + 8 * (s / L), i.e. range c / G, query (c % G) * L + s % L, and exits if that range or query does not exist. Every (range,
 * query) pair is scored exactly once; tests/test_bm25_table_plan.py replays the rule. linear != 0 forces L = 0. */
int rag_bm25_grid_plan(int n_ranges_in_launch, int n_queries, int linear, int64_t* out5);
/* term_ptr[Q+1], terms[term_ptr[Q]] (query tokens WITH repeats; -1 = out-of-vocabulary).
 * scores_out are max-normalised as the reference does; raw_max_out[Q] (may be NULL) is the divisor.
 * tenant >= 0 (needs rag_index_set_tenants_host and postings row-aligned with the index): only that tenant's documents
 * can be returned - the `WHERE agent_id = %s` every reference query carries (rag/document_store.py:457); idf / avgdl stay
 * the statistics of the whole loaded corpus, the max-normalisation uses the tenant's own best score. tenant < 0: no filter.
 * The same filter applies to the BM25 leg of rag_hybrid_rrf_dev and rag_retrieve_rerank_dev (mode 1). */
int rag_bm25_topk_host(rag_handle_t h, const int32_t* term_ptr_host, const int32_t* terms_host, int n_queries,
                       int k, int tenant, int64_t* ids_out_host, int32_t* rows_out_host, double* scores_out_host,
                       double* raw_max_out_host);
/* on = 1 (default): top-k scores are divided by the per-query max as rag/retrieval.py:343-345 does. on = 0: top-k
 * scores stay raw; a row-sharded index merges the shards' raw lists first and divides by the
 * GLOBAL max afterwards. raw_max_out is written either way. */
int rag_bm25_set_normalize(rag_handle_t h, int on);
/* dense scores for a (small) corpus: out[Q][N] raw (un-normalised) BM25, for hybrid_search semantics */
int rag_bm25_scores_host(rag_handle_t h, const int32_t* term_ptr_host, const int32_t* terms_host, int n_queries,
                         double* out_host);
/* The same for an AD-HOC corpus, stateless: HybridRetriever.hybrid_search builds a fresh BM25Okapi over the corpus it is
 * handed on every call (rag/retrieval.py:333-341). The postings (arguments as rag_bm25_load_host) are uploaded, scored
 * and dropped inside the call; the resident postings of the index are not touched. out[Q][n_docs] raw scores. */
int rag_bm25_scores_adhoc_host(rag_handle_t h, const int64_t* indptr_host, const int32_t* doc_host, const int32_t* tf_host,
                               const int32_t* doc_len_host, const double* idf_host, int64_t n_docs, int64_t n_terms,
                               double avgdl, double k1, double b, const int32_t* term_ptr_host,
                               const int32_t* terms_host, int n_queries, double* out_host);

/* ---- weighted linear fusion + top-k: replaces rag/retrieval.py:294-322
 *      hybrid = alpha*semantic + beta*keyword + gamma*temporal, stable sort desc, [:top_k].
 *      0 < top_k <= min(n, 1024), else RAG_ERR_ARG; hybrid_out[n] holds every fused score, idx_out[top_k] the order. +-inf
 *      inputs sort as in Python; NaN fused scores are unspecified (as the reference's own sort is). */
int rag_linear_fuse_topk_host(rag_handle_t h, const double* semantic_host, const double* keyword_host,
                              const double* temporal_host /*NULL = zeros*/, int n, double alpha, double beta,
                              double gamma, int top_k, int32_t* idx_out_host, double* hybrid_out_host);

/* Index-level linear fusion (SURVEY.md section 8b `rag_hybrid_linear`): HybridRetriever.hybrid_search
 * (rag/retrieval.py:214-322) with the WHOLE resident index as its corpus. Per query and row:
 *   hybrid = (alpha * cosine + beta * keyword) + gamma * temporal      (:302, CPython's operation order, float64)
 * keyword = BM25Okapi score / max over all documents - under a tenant filter over the tenant's documents, the corpus the
 * reference would have been handed - (1.0 when that max is <= 0, :343-345); temporal = the per-row vector
 * of rag_index_set_temporal_host (RECENCY_WEIGHT * 0.5 ** (days_old / half_life), computed by the host as :266-292 does;
 * NULL = zeros). Result: stable sort descending (lower row first on ties), first k; rows_out are index rows, ids_out doc
 * ids, hybrid_out the float64 hybrid scores; semantic / keyword / temporal_out (each [Q*k], may be NULL) are the
 * components the reference returns next to them. alpha must be > 0; tenant as in rag_dense_topk_dev, and q_dev 16-byte aligned
 * as there. The postings must be
 * row-aligned with the index. Exact by the same construction as the dense search: the fp16 MFMA pass only discards rows
 * whose FUSED score is provably below the k-th best, survivors are rescored in float64. The bound on the fused fp16-pass
 * score is |alpha| * eps + 2^-21 * (|alpha| + |beta| * max|keyword| + |gamma| * max|temporal|): beta and gamma may have
 * either sign, temporal scores any finite magnitude (their maximum is tracked), and max|keyword| is 1 unless the query
 * postings hold negative idf values: then it is the larger of 1 and (k1 + 1) * (largest such |idf|) * (tokens of the
 * query) / max, a bound on every negative raw score of that query, so keyword scores far below -1 (a long query over terms that most
 * documents contain) are covered too.
 * rag_dense_stats.eps after this call is the bound at max|keyword| = 1. */
int rag_index_set_temporal_host(rag_handle_t h, const double* temporal_host, int64_t n_rows);
int rag_hybrid_linear_dev(rag_handle_t h, const float* q_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                          int n_queries, int k, double alpha, double beta, double gamma, int tenant,
                          int64_t* ids_out_dev, int32_t* rows_out_dev, double* hybrid_out_dev, double* semantic_out_dev,
                          double* keyword_out_dev, double* temporal_out_dev, void* stream);

/* ---- cross-encoder (BertForSequenceClassification, ms-marco-MiniLM-L-6-v2 shape): replaces
 *      CrossEncoder.predict (rag/reranker.py:355). Weights are handed over as float32 host arrays in the
 *      HF state-dict layout (nn.Linear [out,in]); see optimized-rag_amd/cross_encoder.py for the order. */
typedef struct rag_ce_config {
    int32_t vocab_size, hidden, layers, heads, ffn, max_pos, type_vocab, reserved;
    double ln_eps;
} rag_ce_config;
/* Shapes that load (rag_ce_load_host and rag_embed_load_host alike; anything else is RAG_ERR_ARG with a "ce_load:" message):
 * hidden a multiple of 128 up to 1024, ffn a multiple of 128, and a head dim (hidden / heads) of
 *   32 at every hidden size, or
 *   64 at hidden 128, 256, 512, 640, 768, 896 and 1024 - the BERT-base (768 / 12) and BERT-large (1024 / 16) shapes, the small
 *      BERTs (128 / 2, 256 / 4, 512 / 8). These run the split-fp16 forward with an attention instance of their own.
 * Hidden 384 takes head dim 32 only (12 heads): that width is the MX forward's, whose operands are laid out per 32-wide head.
 * type_vocab = 1 (RoBERTa / XLM-RoBERTa, whose position table the loader hands over without its first pad_token_id + 1 rows):
 * the one row of the token-type table is uploaded twice, so with such a model every token takes row 0 whatever token_type_ids
 * holds. */
int rag_ce_load_host(rag_handle_t h, const rag_ce_config* cfg, const float* const* tensors_host, int n_tensors);
/* input_ids/token_type_ids: [P][L] int32 (padded), lens[P]; logits_out[P] raw logits (float32).
 * lens[p] outside [1, seq_len] is clamped to it (0 and negative values count as 1, anything above seq_len as seq_len), once, before
 * any kernel uses it: row packing, attention and the pooling heads of rag_ce_score_* and rag_embed_* all see the clamped value.
 * seq_len is rounded up to an attention length class - 32, 64, 96, 128, 192, 256, 384, 512 for every model, and 768, 1024, 1536,
 * 2048, 3072, 4096, 6144, 8192 behind them for a model with 64-wide heads - which picks the attention instance and launch shape
 * (rag_ce_length_class below). seq_len may be at most
 *   min(max_pos, 8192) for a model with 64-wide heads (the long-context XLM-R-large checkpoints: bge-m3, bge-reranker-v2-m3),
 *   min(max_pos, 512)  for a model with 32-wide heads (its attention keeps a pair's K / V in LDS, and the MX forward is laid out
 *                      per 32-wide head);
 * a call past its model's limit is RAG_ERR_ARG - decided when the call is made, never at load - with a message that names the
 * limit and whether max_pos or the head width set it, and leaves the handle usable. rag_model_seq_limit reports the limit.
 * A result of rag_ce_score_* / rag_embed_* is a function of the sequence's own tokens, the model and the forward (option ce_mx,
 * the load-time probe) alone: bit-identical whatever seq_len and length class the call has - across 512 too: a 100-token sequence
 * scored in a seq_len = 3000 call returns the bits it returns in a seq_len = 128 call -, whatever the other sequences of the call
 * are, wherever the call is split into chunks and whichever attention form option ce_attn_stream selects
 * (tests/test_length_class_invariance_gpu.py, tests/test_long_seq_gpu.py).
 * The limits above are those of rag_ce_score_* and rag_embed_* alone: the resident token store (rag_tokens_*: L <= 512),
 * rag_ce_build_pairs_dev and rag_retrieve_rerank*_dev (L_pair <= 512) stay at 512 tokens. */
int rag_ce_score_host(rag_handle_t h, const int32_t* input_ids_host, const int32_t* token_type_ids_host,
                      const int32_t* lens_host, int n_pairs, int seq_len, float* logits_out_host);
int rag_ce_score_dev(rag_handle_t h, const int32_t* input_ids_dev, const int32_t* token_type_ids_dev,
                     const int32_t* lens_dev, int n_pairs, int seq_len, float* logits_out_dev, void* stream);
/* The attention length class a call of seq_len runs in on a model whose heads are head_dim wide (host-only, no GPU call; no reference
 * counterpart). RAG_ERR_ARG for seq_len < 1, a head_dim other than 32 or 64, a seq_len past that width's limit (512 / 8192), or a
 * NULL class_out. */
int rag_ce_length_class(int head_dim, int seq_len, int* class_out);
/* The longest seq_len the loaded model takes: min(max_pos, 512 or 8192 by head width). which: 0 = the cross-encoder
 * (rag_ce_load_host), 1 = the embedder (rag_embed_load_host); anything else RAG_ERR_ARG. RAG_ERR_STATE when none is loaded. Host
 * state only. */
int rag_model_seq_limit(rag_handle_t h, int which /* 0 cross-encoder, 1 embedder */, int* limit_out);

/* ---- local sentence-embedding model on the device: stands where the reference calls the OpenAI
 *      embeddings endpoint over HTTP for every query and every document - EmbeddingService._generate_embedding_uncached /
 *      _generate_batch_uncached (memory/embeddings.py:100-115, 226-246; dimension lookup :312-332). NOT a parity
 *      replacement: a local encoder produces DIFFERENT vectors than text-embedding-3-small, so an index must be built and
 *      queried with the same model (outside the 1e-3 contract of the north star; what is pinned is this forward against
 *      transformers.BertModel). The model is a BERT encoder (the cross-encoder's kernels; the shapes that load are
 *      rag_ce_load_host's, 64-wide heads included) behind sentence-transformers' Pooling + Normalize head: tensors as
 *      rag_ce_load_host WITHOUT the four pooler / classifier tensors (5 + 16 * layers). flags is a bit word:
 *        RAG_EMBED_NORMALIZE (1)  L2-normalise the pooled vector (x / max(|x|, 1e-12));
 *        RAG_EMBED_POOL_CLS  (2)  pool by the last hidden state of row 0 ([CLS]; sentence-transformers' pooling_mode_cls_token:
 *                                 no pooler dense, no tanh) instead of the mean over the real tokens;
 *      any other bit is RAG_ERR_ARG. 0 and 1 are what the former `normalize` argument meant.
 *      rag_embed_*: input_ids / token_type_ids [n_texts][L] int32 (padded), lens[n_texts]; out[n_texts][hidden] float32.
 *      lens clamping, the length classes and what a vector is a function of: as for rag_ce_score_* above. The mean runs over the
 *      clamped length. A 384-wide encoder takes the MX forward (hi16 + lo8 operands) by shape, without the classifier's load-time
 *      probe: on the stress weights of tests/ce_stress.py it stays within 2.4e-4 per component of the unit vector (bar 1e-3) and
 *      1 - cos <= 6.5e-7 (bar 1e-6, reached only with sharp attention heads; 1.2e-8 or less otherwise) of the float64 oracle;
 *      option ce_mx = -1 selects the split-fp16 forward (2.5e-5, 9.1e-9). DESIGN.md section 4.5. */
#define RAG_EMBED_NORMALIZE 1
#define RAG_EMBED_POOL_CLS 2
int rag_embed_load_host(rag_handle_t h, const rag_ce_config* cfg, const float* const* tensors_host, int n_tensors, int flags);
int rag_embed_host(rag_handle_t h, const int32_t* input_ids_host, const int32_t* token_type_ids_host, const int32_t* lens_host,
                   int n_texts, int seq_len, float* out_host);
int rag_embed_dev(rag_handle_t h, const int32_t* input_ids_dev, const int32_t* token_type_ids_dev, const int32_t* lens_dev,
                  int n_texts, int seq_len, float* out_dev, void* stream);
int rag_embed_dim(rag_handle_t h, int* dim_out);

/* ---- token-vector and lexical heads of the embedder (no reference counterpart: the three heads of bge-m3 - FlagEmbedding's
 *      BGEM3FlagModel - and the ColBERT checkpoints on shapes that load: colbertv2.0 768 -> 128, answerai-colbert-small 384 -> 96).
 *      Semantics restated from upstream, parity with upstream unpinned; x = the last hidden state [len][hidden]:
 *        lexical   w[t] = relu(lex_w . x[t] + lex_b) for every t < len;
 *        tokens    v[t - 1] = normalize(tok_w . x[t] + tok_b) for t = 1 ... len - 1 (row 0 dropped, the final [SEP] row kept;
 *                  x / max(|x|, 1e-12)): a text has len - 1 rows of tok_dim floats.
 *      rag_embed_heads_load_host attaches either head or both (a NULL matrix leaves that head as it was; both NULL: RAG_ERR_ARG) to
 *      the embedder rag_embed_load_host loaded - RAG_ERR_STATE when there is none; a later rag_embed_load_host drops the heads.
 *      tok_w [tok_dim][hidden], tok_b [tok_dim] or NULL (= 0), lex_w [hidden]: float32 host arrays (nn.Linear layout). tok_dim is a
 *      multiple of 32 in [32, 1024], else RAG_ERR_ARG. Every shape that loads takes heads; behind the 384-wide MX forward the last
 *      hidden state is rewritten into the split-fp16 layout once per call and the same head kernels run.
 *      rag_embed_multi_*: the inputs of rag_embed_*, one forward, up to three outputs, each of which may be NULL (all NULL: RAG_ERR_ARG):
 *        dense_out [n_texts][hidden]    exactly the bits rag_embed_* returns for the same input, load flags and options;
 *        lex_out   [n_texts][seq_len]   float32; positions at or past the clamped length are written as 0;
 *        tok_out   float32 rows PACKED text after text, text i = rows [row_off_out[i], row_off_out[i + 1]) = clamped len_i - 1 rows of
 *                  tok_dim floats; tok_rows_cap = the rows tok_out holds. row_off_out [n_texts + 1] int64 is filled by the library
 *                  (required with tok_out, optional otherwise). The library never writes a row at or past tok_rows_cap: _host returns
 *                  RAG_ERR_ARG before any launch when the cap is too small; _dev drops the rows past it, and row_off_out[n_texts] still
 *                  gives the true total.
 *      An output whose head is not loaded: RAG_ERR_STATE (the handle stays usable). Length limits, length classes, chunking, lens
 *      clamping and the invariance rule are those of rag_embed_*: every output of a text is a function of its own tokens and the
 *      model alone, bit-identical whatever seq_len, length class, chunk split and neighbours the call has. _dev: queued on `stream`,
 *      ordered as the other device-pointer calls; scratch belongs to the model. Against the float64 reference on seeded models (DESIGN.md
 *      4.5): token vectors within 1e-3 per component and 1 - cos < 1e-6, lexical weights within 2e-3 * |lex_w|_1. */
int rag_embed_heads_load_host(rag_handle_t h, const float* tok_w_host, const float* tok_b_host, int tok_dim, const float* lex_w_host,
                              float lex_b);
int rag_embed_multi_host(rag_handle_t h, const int32_t* input_ids_host, const int32_t* token_type_ids_host, const int32_t* lens_host,
                         int n_texts, int seq_len, float* dense_out_host, float* lex_out_host, float* tok_out_host, int64_t tok_rows_cap,
                         int64_t* row_off_out_host);
int rag_embed_multi_dev(rag_handle_t h, const int32_t* input_ids_dev, const int32_t* token_type_ids_dev, const int32_t* lens_dev,
                        int n_texts, int seq_len, float* dense_out_dev, float* lex_out_dev, float* tok_out_dev, int64_t tok_rows_cap,
                        int64_t* row_off_out_dev, void* stream);
/* Late interaction (MaxSim) over packed token vectors: out[p] = (1 / nq) * sum_i max_j <q row i, d row j> over the rows
 * [q_off[pair_q[p]], q_off[pair_q[p] + 1]) of q_vecs and [d_off[pair_d[p]], d_off[pair_d[p] + 1]) of d_vecs - the texts' own rows only;
 * a maximum may be negative. A pair whose index lies outside its side (-1 included) or whose side has no rows gives 0. q_vecs /
 * d_vecs: float32 [rows][dim], 16-byte aligned, dim a multiple of 32 in [32, 1024] (else RAG_ERR_ARG); q_off [n_q + 1], d_off
 * [n_d + 1] int64, non-decreasing from >= 0 (checked by _host; _dev trusts them); pair_q / pair_d [n_pairs] int32; out [n_pairs]
 * float32. One workgroup per pair, split-fp16 MFMA products (hi*hi + hi*lo + lo*hi): within 1e-4 of float64 on unit vectors.
 * Deterministic: a pair's result is bit-identical from run to run and whatever other pairs the call holds. _host stages its
 * arrays and waits; _dev is queued on `stream` and keeps nothing. */
int rag_maxsim_host(rag_handle_t h, const float* q_vecs_host, const int64_t* q_off_host, int n_q, const float* d_vecs_host,
                    const int64_t* d_off_host, int n_d, const int32_t* pair_q_host, const int32_t* pair_d_host, int n_pairs, int dim,
                    float* out_host);
int rag_maxsim_dev(rag_handle_t h, const float* q_vecs_dev, const int64_t* q_off_dev, int n_q, const float* d_vecs_dev,
                   const int64_t* d_off_dev, int n_d, const int32_t* pair_q_dev, const int32_t* pair_d_dev, int n_pairs, int dim,
                   float* out_dev, void* stream);
/* Lexical match: out[p] = sum over the token ids both texts of pair p hold of (largest weight of the id in q) * (largest weight of
 * the id in d), summed in float64 and returned as float32. ids / weights [n][L] int32 / float32 with lens [n] (clamped to [0, L]) for
 * each side; weights <= 0 contribute nothing; the ids in skip_ids (a HOST array in both forms, n_skip <= 8 else RAG_ERR_ARG: the
 * tokenizer's cls / eos / pad / unk) never match. A pair index outside its side gives 0. One workgroup per pair comparing ids:
 * lq * (lq + ld) compares - a few hundred per thread for a query of 32 tokens against a passage of 255, half a million (milliseconds)
 * for two texts of 8192 tokens, which is correct but not fast. */
int rag_lexical_match_host(rag_handle_t h, const int32_t* q_ids_host, const float* q_weights_host, const int32_t* q_lens_host, int n_q,
                           int q_seq_len, const int32_t* d_ids_host, const float* d_weights_host, const int32_t* d_lens_host, int n_d,
                           int d_seq_len, const int32_t* pair_q_host, const int32_t* pair_d_host, int n_pairs,
                           const int32_t* skip_ids_host, int n_skip, float* out_host);
int rag_lexical_match_dev(rag_handle_t h, const int32_t* q_ids_dev, const float* q_weights_dev, const int32_t* q_lens_dev, int n_q,
                          int q_seq_len, const int32_t* d_ids_dev, const float* d_weights_dev, const int32_t* d_lens_dev, int n_d,
                          int d_seq_len, const int32_t* pair_q_dev, const int32_t* pair_d_dev, int n_pairs,
                          const int32_t* skip_ids_host, int n_skip, float* out_dev, void* stream);
/* Lexical compaction: a text's per-position lexical weights (lex_out of rag_embed_multi_*) -> its sparse vector, the query or
 * document form the learned-sparse index takes (term_ptr / terms / qweights of rag_sparse_topk_*; a row of rag_sparse_append_host's
 * CSR). ids / weights [n_texts][seq_len] int32 / float32, lens [n_texts]. Text i contributes the positions t < clamp(lens[i], 0,
 * seq_len). A position is dropped if its id is in skip_ids (a HOST array in both forms, n_skip <= 8, as in rag_lexical_match_*), if
 * its id is < 0, or if its weight is not > 0 (NaN, 0.0, -0.0 and negatives; +inf and float32 subnormals are kept). Of the rest each
 * distinct id appears ONCE with the largest weight it carries, bit for bit, ids ascending within the text. Every id in
 * [0, 2^31 - 1] is legal, INT32_MAX included. term_ptr_out [n_texts + 1] int32: term_ptr_out[0] = 0, term_ptr_out[i + 1] -
 * term_ptr_out[i] = text i's count; terms_out / qweights_out: the texts' slices one after another. Layout, order and bits are those
 * of the Python path: sparse.LexicalPostings.encode_queries over the {token id: largest weight > 0} maps of
 * LocalEmbeddingService.encode_multi (tests/test_lexical_compact_cpu.py pins the two to each other).
 * terms_cap = the entries terms_out / qweights_out hold. The library never writes an entry at or past terms_cap: _host returns
 * RAG_ERR_ARG before any launch when the cap is too small; _dev drops what does not fit, and term_ptr_out[n_texts] still gives the
 * true total (the tok_rows_cap rule of rag_embed_multi_dev). n_texts * seq_len always suffices. With terms_cap = 0 the two arrays
 * may be NULL (counts only).
 * Limits: 1 <= n_texts <= 65535, 1 <= seq_len <= 8192 (the longest sequence the embedder takes), n_texts * seq_len < 2^31, else
 * RAG_ERR_ARG; a NULL array: RAG_ERR_ARG.
 * Deterministic: a text's slice is a function of its own row alone, whatever seq_len, neighbours or batch the call holds.
 * One workgroup per text sorts 64-bit (id, weight bits) keys in LDS (64 KiB at seq_len 8192), twice: the first pass leaves the
 * counts in term_ptr_out, one workgroup turns them into offsets in place, the second pass writes the packed output. _host stages
 * its arrays and waits; _dev is queued on `stream`, ordered as the preamble says, and keeps no workspace. */
int rag_lexical_compact_host(rag_handle_t h, const int32_t* ids_host /*[n][L]*/, const float* weights_host /*[n][L]*/,
                             const int32_t* lens_host /*[n]*/, int n_texts, int seq_len, const int32_t* skip_ids_host, int n_skip,
                             int32_t* term_ptr_out_host /*[n+1]*/, int32_t* terms_out_host, float* qweights_out_host, int64_t terms_cap);
int rag_lexical_compact_dev(rag_handle_t h, const int32_t* ids_dev /*[n][L]*/, const float* weights_dev /*[n][L]*/,
                            const int32_t* lens_dev /*[n]*/, int n_texts, int seq_len, const int32_t* skip_ids_host, int n_skip,
                            int32_t* term_ptr_out_dev /*[n+1]*/, int32_t* terms_out_dev, float* qweights_out_dev, int64_t terms_cap,
                            void* stream);

/* ---- retrieve + rerank in one device-resident call (BASELINE.json configs[3]): the composition of
 *      HybridRetriever.retrieve (rag/retrieval.py:122-212) and CrossEncoderReranker.rerank (rag/reranker.py:320-384:
 *      pairs [query, passage], raw logits, sigmoid, sort desc, [:top_k]) with the passages' token ids resident in HBM.
 *      rag_tokens_load_host: tokens[n_rows][L] passage WordPiece ids (no [CLS]/[SEP]) + lens[n_rows], row-aligned with the
 *      index. rag_retrieve_rerank_dev: mode 0 = dense top-pool candidates, mode 1 = dense + BM25 + RRF(rrf_k) top-pool;
 *      pairs are [CLS] query [SEP] passage [SEP] truncated 'longest_first' to max_length L_pair (what CrossEncoder.predict's
 *      tokenizer call does; the reference's max_length is 512, rag/reranker.py:290-294) and padded to it; outputs per query:
 *      ids_out[k] doc ids (-1 padded), scores_out[k] = sigmoid(logit) as float64, logits_out[k] raw logits,
 *      cand_out[pool] (may be NULL) the candidate list that was reranked. 0 < k <= pool <= 256. q_emb_dev float32 [Q][dim],
 *      16-byte aligned (else RAG_ERR_ARG; the token arrays are read element by element).
 *      Token store: 1 <= L <= 512, ids in [0, 65535] (the resident store is 16 bits wide); anything else is RAG_ERR_ARG. L_pair
 *      is at most 512 as well, whatever the loaded model's own limit (rag_model_seq_limit): the resident pipeline stays at 512
 *      tokens per pair. */
int rag_tokens_load_host(rag_handle_t h, const int32_t* tokens_host, const int32_t* lens_host, int64_t n_rows, int L);
/* Chunked form for stores that should not exist as one host array (a replicated 100M-passage store, SURVEY.md section 8e, is
 * 45 GB resident as uint16 and would be 90 GB as one int32 host array): reserve once, then append row blocks in order from
 * DEVICE memory (tokens_dev[n][L] int32, lens_dev[n]); each append returns after its rows are resident and checked.
 * An append before rag_tokens_reserve, past the reservation, or with an id outside [0, 65535] is RAG_ERR_ARG and is rejected
 * whole: the rows appended before stay, the row count does not move, and the same row range may be appended again. */
int rag_tokens_reserve(rag_handle_t h, int64_t n_rows_total, int L);
int rag_tokens_append_dev(rag_handle_t h, const int32_t* tokens_dev, const int32_t* lens_dev, int64_t n_rows, void* stream);
/* A 24-bit token store, opt-in, for models over a large vocabulary (XLM-RoBERTa's SentencePiece vocabulary has 250,002 entries:
 * the multilingual rerankers and embedders). id_bits is 16 or 24, anything else RAG_ERR_ARG; 16 is exactly rag_tokens_load_host /
 * rag_tokens_reserve. 24 keeps the uint16 plane for the low half of an id and adds a uint8 plane [rows][L] for bits 16-23: 3 B per
 * token where an int32 store would take 4, ids in [0, 16777215]. Every consumer follows the width the store was created with:
 * rag_tokens_append_dev narrows on the device into both planes and rejects a block whole if an id is outside [0, 16777215] (the
 * semantics above, the message names that range); rag_index_insert_host narrows the block on the host into both planes, grows
 * both past the reservation and leaves both untouched when it fails; rag_index_compact / rag_index_compact_bm25 move the byte
 * plane as one more row plane; rag_ce_build_pairs_dev and rag_retrieve_rerank[_tenants]_dev read lo | hi << 16. With ids below
 * 65536 a 24-bit store gives bit-identical results to a 16-bit one. rag_tokens_load_host and rag_tokens_reserve stay 16 bits wide
 * and, like these, replace whatever store the handle had. Stream ordering, locking and the wait for queued *_dev work are those of
 * rag_tokens_load_host / rag_tokens_reserve.
 * rag_tokens_info: rows resident, passage length and width (16 or 24) of the handle's store; any output may be NULL; without a
 * store 0 / 0 / 0. Host state only. */
int rag_tokens_load_wide_host(rag_handle_t h, const int32_t* tokens_host, const int32_t* lens_host, int64_t n_rows, int L,
                              int id_bits);
int rag_tokens_reserve_wide(rag_handle_t h, int64_t n_rows_total, int L, int id_bits);
int rag_tokens_info(rag_handle_t h, int64_t* rows_out, int* L_out, int* id_bits_out);
int rag_retrieve_rerank_dev(rag_handle_t h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                            const int32_t* q_tok_dev, const int32_t* q_len_dev, int Lq, int n_queries, int pool, int k,
                            int rrf_k, int tenant, int mode, int cls_id, int sep_id, int L_pair, int64_t* ids_out_dev,
                            double* scores_out_dev, float* logits_out_dev, int64_t* cand_out_dev, void* stream);
/* The layout the pair builder writes, per handle (default RAG_PAIR_BERT; rag_ce_load_host does not touch it). It applies to
 * rag_retrieve_rerank_dev, rag_retrieve_rerank_tenants_dev and rag_ce_build_pairs_dev; cls_id and sep_id stay call arguments
 * (XLM-R: <s> = 0, </s> = 2). RAG_PAIR_ROBERTA is what a RoBERTa / XLM-RoBERTa tokenizer's pair template produces: two separators
 * between the sides, every token type 0, the same 'longest_first' truncation over M = L_pair - 4 content tokens,
 * lens = ql + dl + 4, padding id 0 / type 0. Host state read while a call enqueues, as rag_set_option: no wait, a call queued
 * earlier keeps the old layout. An unknown format is RAG_ERR_ARG. */
#define RAG_PAIR_BERT    0   /* [cls] q [sep] d [sep],        token types 0 | 1, L_pair - 3 content tokens */
#define RAG_PAIR_ROBERTA 1   /* [cls] q [sep] [sep] d [sep],  token types all 0, L_pair - 4 content tokens */
int rag_ce_set_pair_format(rag_handle_t h, int format);

/* The pipeline's two small kernels on their own (row-sharded composition): pair assembly from GLOBAL
 * candidate doc ids against a replicated token store whose first row has id token_id_base; and sigmoid + stable top-k of
 * the logits of a [Q][pool] candidate table (rag/reranker.py:359,372-376). rag_rerank_topk_dev: 0 < k <= pool <= 256
 * (else RAG_ERR_ARG); slots with cand < 0 are skipped wherever they sit; equal scores keep candidate order; outputs are
 * padded with -1 / 0.0 / 0.0. */
int rag_ce_build_pairs_dev(rag_handle_t h, const int32_t* q_tok_dev, const int32_t* q_len_dev, int Lq, const int64_t* cand_dev,
                           int n_queries, int pool, int64_t token_id_base, int L_pair, int cls_id, int sep_id,
                           int32_t* ids_out_dev, int32_t* tt_out_dev, int32_t* lens_out_dev, void* stream);
int rag_rerank_topk_dev(rag_handle_t h, const float* logits_dev, const int64_t* cand_dev, int n_queries, int pool, int k,
                        int64_t* ids_out_dev, double* scores_out_dev, float* logits_out_dev, void* stream);

/* ---- resident token-vector store and late-interaction rerank on the device (no reference counterpart; the token vectors are the
 *      tok_out of rag_embed_multi_*). rag_maxsim_* scores pairs whose float32 vectors the caller passes; here the passages' vectors
 *      are computed once at ingest and kept in HBM as packed fp16 rows [rows][dim] with int64 offsets [n_docs + 1], so that a query
 *      costs its own forward only and a rerank reads half the bytes. Document i is row i of the dense index; a document with 0
 *      rows is legal. dim is a multiple of 32 in [32, 1024] (the limits of rag_maxsim_*), else RAG_ERR_ARG.
 * rag_tokvec_reserve: room for n_docs_total (>= 1) documents and rows_total (>= 0) rows; replaces any earlier store.
 * rag_tokvec_append_dev: the next n_docs documents from DEVICE memory: vecs_dev float32 [rows][dim], row_off_dev int64 [n_docs + 1] -
 *   the tok_out / row_off_out of rag_embed_multi_dev as they are. Offsets are taken relative to row_off[0] (rows row_off[0] ...
 *   row_off[n_docs] - 1 of vecs_dev are read). Like rag_tokens_append_dev it waits for `stream` and returns once the rows are
 *   resident and checked. A block is rejected whole with RAG_ERR_ARG when it comes before a reserve, goes past either reservation,
 *   has a negative first or a decreasing offset, or holds a value that rounds to NaN or inf as fp16 (NaN, inf, |x| >= 65520; a
 *   float32 in (65504, 65520) rounds to 65504 and is accepted): the counts do
 *   not move and the same block may be appended again. rag_tokvec_append_host: the same arguments from host arrays, staged in
 *   pieces of at most 64 Mi floats. rag_tokvec_load_host: reserve(n_docs, off[n_docs] - off[0], dim) + append_host.
 *   Conversion is float32 -> fp16 round to nearest even, on the device: the stored bits are numpy's x.astype(float16). Rows are not
 *   renormalised afterwards.
 * rag_tokvec_info: documents and rows appended so far, dim, HBM bytes of the reservation; all 0 without a store; host state only.
 * rag_tokvec_fetch_host: the stored rows of one document as float32 (exact) [*n_rows_out][dim], for tests; *n_rows_out is written
 *   first, RAG_ERR_ARG when it exceeds cap_rows or doc is outside the documents appended.
 * rag_tokvec_rerank_dev: for each of n_queries queries - float32 token vectors q_vecs [rows][dim] (16-byte aligned), int64 q_off
 *   [n_queries + 1], trusted as in rag_maxsim_dev - and each of its `pool` candidate rows cand_rows [Q][pool] int32:
 *     score[q][j] = (1 / nq) * sum_i max_r <vq[i], store[cand[q][j]][r]>
 *   then the top k by score descending, equal scores in candidate order. 0 < k <= pool <= 256, n_queries * pool < 2^24 (one
 *   workgroup per slot in one launch), else RAG_ERR_ARG. A slot with cand < 0, a row at or
 *   past the store's documents, a document with 0 rows or a query with 0 rows scores 0.0 and is skipped by the top-k. Outputs:
 *   ids_out [Q][k] int64 (the index's id mapping - explicit ids or id_base + row; -1 for a scored row the index does not have, e.g. a store filled
 *   ahead of the inserts: rows_out still names it; without an index the row numbers), rows_out
 *   [Q][k] int32 (may be NULL), scores_out [Q][k] float64 = the float32 pair score widened, padded with -1 / -1 / 0.0;
 *   pair_scores_out [Q][pool] float32 (may be NULL) every slot's score. Explicit rows: row visibility (deletes, tenants) is not
 *   looked at. _host: the same from host arrays (q_off checked), synchronous.
 *   Numerics: the float32 query is split into hi + lo fp16, the stored fp16 rows are exact MFMA operands, two
 *   mfma_f32_16x16x32_f16 per product (lo_q * d + hi_q * d) with fp32 accumulation, per-query maxima summed in float64 in query
 *   order: within 1e-4 of float64 MaxSim over the STORED (fp16-rounded) vectors, within 1e-3 of float64 MaxSim over the original
 *   float32 unit vectors (fp16 rounding moves a dot of unit vectors by at most 2^-11). A pair's score is a function of its own
 *   rows only: bit-identical from run to run, whatever pool, neighbours or batch surround it.
 * rag_retrieve_maxsim_dev: candidates, MaxSim rerank and top-k in one device-resident call, as rag_retrieve_rerank_dev does for the
 *   cross-encoder. q_emb and q_vecs 16-byte aligned (else RAG_ERR_ARG, before anything is queued). mode 0: the dense
 *   top-`pool` of q_emb [Q][dim index]; mode 1: the top-`pool` of dense + learned-sparse RRF
 *   (term_ptr / terms / qweights as rag_hybrid_sparse_rrf_dev, rrf_k), with tenant and deleted-row filtering as in those searches;
 *   then rag_tokvec_rerank_dev over those rows. ids_out / scores_out [Q][k], cand_out [Q][pool] int64 (may be NULL) the candidate
 *   ids. 1 <= n_queries <= 65535, 0 < k <= pool <= 256. Bit-identical to rag_dense_topk_dev (mode 0) or rag_hybrid_sparse_rrf_dev
 *   with k = pool (mode 1) followed by rag_tokvec_rerank_dev on the rows. Needs store documents == index rows, else RAG_ERR_STATE.
 *   Workspaces are handle-owned and grown as the preamble says (the first call of a larger shape frees the old one, which waits).
 *   mode 2, the exhaustive MaxSim search: no candidate stage. For each query the result is the top-`pool` of
 *     score[q][d] = (1 / nq) * sum_i max_r <vq[i], store[d][r]>
 *   over EVERY document d of the store that the query may see - not deleted, and of the query's tenant when one is given (the
 *   predicate of the other searches) - score descending, the lower row first on equal scores. ids_out / scores_out [Q][k] are the
 *   first k of that list (ids by the index's id mapping, scores the float32 pair score widened); cand_out [Q][pool] (may be NULL)
 *   holds the ids of the whole top-`pool` in that order; padding -1 / 0.0. A document without rows and a query without rows score
 *   0.0 and are never listed, as in rag_tokvec_rerank_dev. q_emb, term_ptr, terms, qweights and rrf_k are not read, and q_emb may
 *   be NULL in this mode only. Every other check of the entry holds: a usable store that is not stale and holds exactly the
 *   index's rows (else RAG_ERR_STATE), the tenant table when a tenant is asked for, q_vecs 16-byte aligned,
 *   1 <= n_queries <= 65535, 0 < k <= pool <= 256, n_queries * pool < 2^24. BIT-IDENTITY: for every listed (query, row),
 *   scores_out has the bits rag_tokvec_rerank_dev reports for that pair, in both storage forms - the scan scores a pair by the
 *   rerank kernel's own MFMA sequence, row maxima and float64 sum, and the call's last step is that rerank over the scan's
 *   top-`pool` rows. Cost: 2 * nq * nd * dim FLOP per pair and twice that issued (hi + lo query halves), over every visible
 *   document: a search for per-tenant corpora and mid-sized stores, an exact baseline on larger ones.
 *   The scan writes one 4-byte key per (query, document) of a sub-batch of Qb queries into a plane of the call's handle-owned workspace; option
 *   tokvec_scan_ws_mb (default 2048) bounds the plane, Qb = max(1, min(Q, bound / (4 * documents))), option tokvec_scan_queries
 *   (default 0 = derived) sets Qb itself. The same bits for every Qb. Modes 0 and 1 are unchanged by mode 2, workspace included.
 * Live writes, as the BM25 postings: rag_index_compact / rag_index_compact_bm25 mark the store STALE when deleted rows are removed
 * (rag_index_compact_live moves the store's documents with their rows instead and does not);
 *   every rag_tokvec_rerank_* and rag_retrieve_maxsim_dev then returns RAG_ERR_STATE until rag_tokvec_reserve / rag_tokvec_load_host
 *   runs again (the handle stays usable; a compaction that finds nothing deleted marks nothing). rag_index_insert_host leaves the
 *   store alone: rag_retrieve_maxsim_dev returns RAG_ERR_STATE until appends cover the new rows (reserve headroom for them).
 *   Deletes need nothing: the composite's searches hide deleted rows, and the explicit-row entries do not look.
 * Ordering: reserve / load / append_host / fetch / rerank_host are host calls (they wait for queued *_dev work); the _dev calls
 *   follow the preamble, rag_tokvec_append_dev waiting for `stream` as said.
 * Sharding: a candidate's token vectors live on the rank that holds its row, and the candidates come from GLOBAL lists, so a
 *   merge of per-shard results does not give rag_retrieve_maxsim_dev: the owning rank scores each candidate and the top-k runs
 *   over the gathered scores (the three rag_m3_*_gathered / _score_ids entries below with weights (0, 0, 1)).
 * Storage forms. A store is reserved in one of two forms; RAG_TOKVEC_FP16 (the default, everything above) or RAG_TOKVEC_MXFP8:
 *   OCP MXFP8, E4M3 codes with one shared power-of-two scale per 32 consecutive components, 33/64 of the fp16 form's passage
 *   bytes. For a block with amax = max |x|: the scale exponent e is the smallest integer with amax <= 448 * 2^e, clamped to
 *   [-15, 7] (e = -15 for an all-zero block), stored as one E8M0 byte e + 127. Each component is stored as E4M3(x * 2^-e) in the
 *   "FN" encoding (max 448, no infinities): round to nearest even, subnormals kept, a magnitude above 448 after scaling (possible
 *   only at the e = 7 clamp, amax > 57344) saturates to 448, the NaN codes are never stored, the sign of zero is kept. The stored
 *   value is code * 2^e. The clamps make every stored value an exact fp16 value (smallest step 2^-24, largest magnitude
 *   448 * 128 = 57344, at most 4 significant bits), and quantising stored values returns them unchanged.
 *   rag_tokvec_reserve_form: rag_tokvec_reserve with the form (rag_tokvec_reserve is form 0); an unknown form is RAG_ERR_ARG and
 *   leaves an earlier store as it is. rag_tokvec_load_form_host: reserve_form + append_host. rag_tokvec_form: the form of the
 *   store, -1 without one; host state only. rag_tokvec_append_* quantise on the device into the reserved form and reject exactly
 *   the blocks the fp16 form rejects (NaN, inf, |x| >= 65520; 65504 ... 65519 saturate to 57344). rag_tokvec_fetch_host returns
 *   code * 2^e as float32, exact. rag_tokvec_info's hbm_bytes is what is allocated: a row is dim code bytes, then its dim / 32 scale
 *   bytes, padded to a multiple of 16 bytes (at most 15 bytes of padding per row). Every rerank and composite entry serves either
 *   form without a new argument; the stored values are expanded to the fp16 operand exactly, so a pair's score is BIT-IDENTICAL
 *   to the fp16 form's score over a store loaded with the fetched rows: within 1e-4 of float64 MaxSim over the stored vectors.
 *   Against the ORIGINAL float32 unit rows: a component at or above the block's smallest normal 2^(e - 6) moves by at most
 *   2^-4 |x|, a smaller one by at most 2^(e - 10) <= 2^-18 amax, a dot of unit rows by at most 2^-4 + 2^-13 (typical: a few 1e-3,
 *   DESIGN.md section 4.5). rag_index_compact_live moves the stored bytes, scales with their rows, never requantised. */
#define RAG_TOKVEC_FP16 0
#define RAG_TOKVEC_MXFP8 1
int rag_tokvec_reserve(rag_handle_t h, int64_t n_docs_total, int64_t rows_total, int dim);
int rag_tokvec_reserve_form(rag_handle_t h, int64_t n_docs_total, int64_t rows_total, int dim, int form);
int rag_tokvec_load_form_host(rag_handle_t h, const float* vecs_host, const int64_t* off_host, int64_t n_docs, int dim, int form);
int rag_tokvec_form(rag_handle_t h, int* form_out);
int rag_tokvec_append_dev(rag_handle_t h, const float* vecs_dev, const int64_t* row_off_dev, int64_t n_docs, void* stream);
int rag_tokvec_append_host(rag_handle_t h, const float* vecs_host, const int64_t* row_off_host, int64_t n_docs);
int rag_tokvec_load_host(rag_handle_t h, const float* vecs_host, const int64_t* off_host, int64_t n_docs, int dim);
int rag_tokvec_info(rag_handle_t h, int64_t* n_docs_out, int64_t* rows_out, int* dim_out, int64_t* hbm_bytes_out);
int rag_tokvec_fetch_host(rag_handle_t h, int64_t doc, float* out_host, int64_t cap_rows, int64_t* n_rows_out);
int rag_tokvec_rerank_dev(rag_handle_t h, const float* q_vecs_dev, const int64_t* q_off_dev, const int32_t* cand_rows_dev,
                          int n_queries, int pool, int k, int64_t* ids_out_dev, int32_t* rows_out_dev /*may be NULL*/,
                          double* scores_out_dev, float* pair_scores_out_dev /*may be NULL*/, void* stream);
int rag_tokvec_rerank_host(rag_handle_t h, const float* q_vecs_host, const int64_t* q_off_host, const int32_t* cand_rows_host,
                           int n_queries, int pool, int k, int64_t* ids_out_host, int32_t* rows_out_host /*may be NULL*/,
                           double* scores_out_host, float* pair_scores_out_host /*may be NULL*/);
int rag_retrieve_maxsim_dev(rag_handle_t h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                            const float* qweights_dev, const float* q_vecs_dev, const int64_t* q_off_dev, int n_queries, int pool,
                            int k, int rrf_k, int tenant, int mode, int64_t* ids_out_dev, double* scores_out_dev,
                            int64_t* cand_out_dev /*may be NULL*/, void* stream);

/* ---- the three-way bge-m3 score over resident data: dense + sparse + MaxSim for given rows (no reference counterpart). The
 *      semantics are restated from FlagEmbedding's BGEM3FlagModel.compute_score, mode "colbert+sparse+dense" with its default
 *      weights (0.4, 0.2, 0.4) = (dense, sparse, colbert); parity with upstream is NOT pinned by a test here, as for the three heads.
 * rag_sparse_score_rows_dev / _host: the exact learned-sparse score of GIVEN rows - the point lookup the searches lack
 *   (rag_sparse_topk_* reports a document only if it made the list). Queries are CSR as in rag_sparse_topk_* (term_ptr [Q + 1],
 *   terms, qweights); cand_rows [Q][pool] int32; scores_out [Q][pool] float64. scores_out[q][j] is BIT-IDENTICAL to
 *   rag_sparse_scores_host(...)[q][cand_rows[q][j]] for a row that is not hidden: the float64 sum of (double)qw * (double)w over the
 *   query's tokens in their order, on the lists that hold the row. Token rules as above: a term < 0 or >= n_terms adds nothing, a
 *   weight not > 0 (NaN included) adds nothing, a repeated term adds twice. A slot with cand < 0 or cand >= the covered documents
 *   scores 0.0. Explicit rows: visibility (deletes, tenants) is not looked at, as in rag_tokvec_rerank_dev. 1 <= n_queries <= 65535,
 *   0 < pool <= 256, else RAG_ERR_ARG; RAG_ERR_STATE when the postings are stale or none are loaded. With appended postings a row
 *   below the base's documents is looked up in the base, any other row in the tail (its own metadata, tables and vocabulary: a term
 *   may be known to the tail only); a row lives in one segment, so the bit-identity with a fresh load of the merged CSR is the
 *   argument made for the searches. One workgroup per query; every (slot, token) lookup is one table read, a few binary steps, two
 *   16-byte loads and a weight load; only the sum is ordered. A score is a function of its query and row: the same bits at any
 *   pool, in any neighbourhood, from run to run.
 * rag_m3_score_rows_dev: for each query and each of its `pool` candidate rows cand_rows [Q][pool] int32, three components widened
 *   to float64:
 *     dense   = the float64 cosine of q_emb [Q][dim index] against the fp32 master row - the function the dense search's
 *               rescoring uses: the bits rag_dense_topk_* reports for that (query, row)
 *     sparse  = rag_sparse_score_rows_dev
 *     colbert = the float32 pair score of rag_tokvec_rerank_dev (its pair_scores_out); 0.0 for a document or a query without
 *               token vectors
 *   and  score = ((w_colbert * colbert + w_sparse * sparse) + w_dense * dense) / ((w_dense + w_sparse) + w_colbert)  in exactly
 *   this association, without fused multiply-add (Python's evaluation of the upstream formula). Then the top k by score
 *   descending, equal scores in candidate order. A slot is empty iff cand < 0 or cand >= the index rows; every other slot is
 *   ranked, whatever its score. Outputs: ids_out [Q][k] int64 (the index's id mapping), rows_out [Q][k] int32 (may be NULL),
 *   scores_out [Q][k] float64, components_out [Q][k][3] float64 in the order (dense, sparse, colbert) (may be NULL); padding
 *   -1 / -1 / 0.0 / 0.0. Weights: finite, each >= 0, sum > 0, else RAG_ERR_ARG. A weight of exactly 0 means its component is not
 *   computed, is reported as 0.0, and neither its query arrays nor its resident structure are required: w_colbert = 0 is upstream's
 *   "sparse+dense" with the same bits (0 * c and x + 0 are exact) and needs no token-vector store; w_sparse = 0 needs no sparse
 *   postings. Limits: 1 <= n_queries <= 65535, 0 < k <= pool <= 256, n_queries * pool < 2^24. A required structure that is
 *   missing, stale or does not cover exactly the index's rows: RAG_ERR_STATE (sparse postings of another row count: RAG_ERR_ARG,
 *   as in rag_hybrid_sparse_rrf_dev). q_emb and q_vecs 16-byte aligned. Explicit rows: visibility is not looked at.
 * rag_retrieve_m3_dev: candidates, then rag_m3_score_rows_dev, in one device-resident call. mode 0: the dense top-`pool`;
 *   mode 1: the top-`pool` of dense + learned-sparse RRF (both as rag_retrieve_maxsim_dev); mode 2: the UNION of the dense
 *   top-`pool` and the sparse top-`pool` - what rag_rrf_fuse_dev over the two lists returns at top_k = 2 * pool, in RRF order,
 *   -1 padded - so 2 * pool candidate slots and pool <= 128. Tenant and deleted rows are filtered by the searches. ids_out /
 *   scores_out [Q][k], components_out [Q][k][3] (may be NULL), cand_out [Q][slots] int64 (may be NULL) the candidate ids, slots =
 *   pool or 2 * pool. 0 < k <= pool. q_emb 16-byte aligned whatever w_dense is (the candidate search reads it). Modes 1 and 2
 *   need the query's terms and fresh, row-aligned sparse postings whatever
 *   w_sparse is. Bit-identical to the search entries (rag_dense_topk_dev; rag_hybrid_sparse_rrf_dev at k = pool; rag_dense_topk_dev
 *   + rag_sparse_topk_dev + rag_rrf_fuse_dev at top_k = 2 * pool) followed by rag_m3_score_rows_dev on their rows. Workspaces
 *   are handle-owned and grown as the preamble says. After the candidate stage and the MaxSim launch: three launches (cosines,
 *   point lookups, combine + select).
 * Live writes: the rules of the sparse postings and of the token-vector store hold for the components that use them;
 *   rag_sparse_append_host / rag_tokvec_append_* after inserts and rag_index_compact_live keep all three current.
 * Ordering: rag_sparse_score_rows_host is a host call; the _dev calls follow the preamble.
 * Sharding: the sparse LIST alone merges through rag_merge_topk_dev (raw scores need no global statistic). The composites do
 *   not: RRF needs global ranks and each candidate is scored by the rank that owns its row - the row-sharded entries below. */
int rag_sparse_score_rows_dev(rag_handle_t h, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev,
                              const int32_t* cand_rows_dev, int n_queries, int pool, double* scores_out_dev, void* stream);
int rag_sparse_score_rows_host(rag_handle_t h, const int32_t* term_ptr_host, const int32_t* terms_host, const float* qweights_host,
                               const int32_t* cand_rows_host, int n_queries, int pool, double* scores_out_host);
int rag_m3_score_rows_dev(rag_handle_t h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                          const float* qweights_dev, const float* q_vecs_dev, const int64_t* q_off_dev, const int32_t* cand_rows_dev,
                          int n_queries, int pool, int k, double w_dense, double w_sparse, double w_colbert, int64_t* ids_out_dev,
                          int32_t* rows_out_dev /*may be NULL*/, double* scores_out_dev, double* components_out_dev /*may be NULL*/,
                          void* stream);
int rag_retrieve_m3_dev(rag_handle_t h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                        const float* qweights_dev, const float* q_vecs_dev, const int64_t* q_off_dev, int n_queries, int pool, int k,
                        int rrf_k, int tenant, int mode, double w_dense, double w_sparse, double w_colbert, int64_t* ids_out_dev,
                        double* scores_out_dev, double* components_out_dev /*may be NULL*/, int64_t* cand_out_dev /*may be NULL*/,
                        void* stream);

/* ---- rag_retrieve_m3_dev over ROW SHARDS (one handle per GPU; DESIGN.md section 5, sharded.py ShardedM3Index). Every rank holds
 *      a contiguous row range loaded with id_base = its first global row: the embeddings, the doc-partitioned sparse postings and
 *      the token vectors of its own documents (either storage form); the query arrays are replicated. Two small all-gathers per
 *      batch, and three entries for the work between them:
 *        local lists (rag_dense_topk_dev and rag_sparse_topk_dev at k = pool, tenants as in those entries)  ->  gather 1  ->
 *        rag_m3_candidates_gathered_dev  ->  rag_m3_score_ids_dev  ->  gather 2  ->  rag_m3_combine_gathered_dev.
 *      RRF needs GLOBAL ranks, so the lists are merged before they are fused; a candidate's token vectors live on one rank, so
 *      the rank that owns a candidate scores it; the combine and the top-k then run over components that came from different ranks.
 * rag_m3_candidates_gathered_dev: gathered_dev = [world][4][Q][pool] int64 = every rank's dense ids | dense cosines (float64
 *   bits) | sparse ids | RAW sparse scores (float64 bits), -1 / 0.0 padded anywhere in a list. Merges the dense lists and the
 *   sparse lists as rag_merge_topk_dev does (score desc, id asc, -1 skipped, nothing normalised) into lists_out_dev [2][Q][pool]
 *   int64 and scores_out_dev [2][Q][pool] float64, then forms the candidate list of rag_retrieve_m3_dev in id space, cand_out_dev
 *   [Q][slots] int64: mode 0 the merged dense list (slots = pool); mode 1 the RRF of the two merged lists at rrf_k, top-pool
 *   (slots = pool); mode 2 the same RRF at top_k = 2 * pool (slots = 2 * pool, pool <= 128), -1 padded. In mode 0 planes 2-3 of
 *   gathered_dev are not read and the sparse halves of lists_out / scores_out are filled with -1 / 0.0. Limits: 1 <= n_queries <=
 *   65535, 0 < pool <= 256 (mode 2: 128), n_queries * slots < 2^24, world * pool <= 4092 (the merge kernel's LDS), else
 *   RAG_ERR_ARG. Needs no index. Bit-identical to the merged lists and the cand_out of rag_retrieve_m3_dev on the unsharded index
 *   (loaded with id_base): a merged list is the unsharded list because the order (score desc, id asc) is total and the scores are
 *   functions of (query, row); RRF then sees the same two lists.
 * rag_m3_score_ids_dev: cand_ids_dev [Q][slots] int64 GLOBAL ids (-1 = empty). A slot is OWNED iff id_base <= id < id_base +
 *   index rows. partial_out_dev [4][Q][slots] int64 = owned flag (1 / 0) | dense | sparse | colbert, the three components as float64
 *   bits (colbert: the float32 pair score widened) from the launches rag_m3_score_rows_dev uses, on row = id - id_base; an unowned
 *   slot carries 0 | 0.0 | 0.0 | 0.0. Weights as rag_m3_score_rows_dev: a weight of 0 computes nothing, writes 0.0 and requires
 *   neither its query arrays nor its resident structure. Limits: 1 <= n_queries <= 65535, 0 < slots <= 256, n_queries * slots <
 *   2^24. An index with explicit ids (rag_index_set_ids_host, or ids at the load) is accepted when its id map is enabled
 *   (rag_index_id_map) and ids_ascending holds: a slot is then OWNED iff the map holds the id and its row is live, and row = the
 *   map's row; one lookup launch takes the place of the id_base arithmetic, every other launch is the same. Without the map:
 *   RAG_ERR_STATE (ownership is defined through id_base alone); with the map but ids that do not ascend with the rows:
 *   RAG_ERR_STATE, the message says so (the merges over shards break ties by lower id, the local searches by lower row; the two
 *   agree exactly when ids ascend with rows on every shard). The other errors are those of rag_m3_score_rows_dev. Row visibility is not looked at: the candidate searches hid
 *   what is hidden. With w_dense == 0 and w_sparse == 0 the call is the late-interaction rerank: a slot MaxSim leaves empty (the
 *   query or the document has no token vectors) is reported UNOWNED, so the combine skips it as the top-k of rag_retrieve_maxsim_dev
 *   does. This is the one place where the three entries differ from rag_retrieve_m3_dev, which at weights (0, 0, w) ranks such a
 *   slot with 0.0.
 * rag_m3_combine_gathered_dev: gathered_dev = [world][4][Q][slots] int64, every rank's partial_out. Each slot takes the components
 *   of the rank that set its owned flag; a slot with cand < 0 or without an owner is empty (skipped, as cand < 0 is in
 *   rag_m3_score_rows_dev); with more than one owner - overlapping shards, a caller error - the LOWEST rank wins. Then the score,
 *   the stable top-k (score desc, slot asc) and the outputs of rag_retrieve_m3_dev: ids_out [Q][k] (the slot's cand id), scores_out
 *   [Q][k], components_out [Q][k][3] (may be NULL), padded -1 / 0.0. Weights: finite, each >= 0, sum > 0. Limits: world >= 1,
 *   1 <= n_queries <= 65535, 0 < k <= slots <= 256, n_queries * slots < 2^24. Needs no index. Bit-identical (ids, float64 score and
 *   component bits) to rag_retrieve_m3_dev on the unsharded index; with weights (0, 0, 1) the score is (1 * c + 0) + 0 over
 *   (0 + 0) + 1 = c exactly, so ids and scores are those of rag_retrieve_maxsim_dev.
 * Workspaces are handle-owned, carved once per call; all three follow the preamble's ordering rules. */
int rag_m3_candidates_gathered_dev(rag_handle_t h, const int64_t* gathered_dev, int world, int n_queries, int pool, int rrf_k, int mode,
                                   int64_t* lists_out_dev, double* scores_out_dev, int64_t* cand_out_dev, void* stream);
int rag_m3_score_ids_dev(rag_handle_t h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                         const float* qweights_dev, const float* q_vecs_dev, const int64_t* q_off_dev, const int64_t* cand_ids_dev,
                         int n_queries, int slots, double w_dense, double w_sparse, double w_colbert, int64_t* partial_out_dev,
                         void* stream);
int rag_m3_combine_gathered_dev(rag_handle_t h, const int64_t* cand_ids_dev, const int64_t* gathered_dev, int world, int n_queries,
                                int slots, int k, double w_dense, double w_sparse, double w_colbert, int64_t* ids_out_dev,
                                double* scores_out_dev, double* components_out_dev /*may be NULL*/, void* stream);

/* ---- rag_hybrid_linear_dev over ROW SHARDS (linear fusion over ROW SHARDS; DESIGN.md section 5, sharded.py
 *      ShardedHybridIndex.search_linear). Every rank holds a contiguous row range loaded with id_base = its first global row, the
 *      doc-partitioned postings of its rows (global idf / avgdl) and its slice of the temporal vector; the query arrays are
 *      replicated. With the maximum of the raw BM25 scores over EVERY rank's rows, a row's hybrid score depends on the query, the
 *      row and that maximum only, so the one-call entry is cut at the point where the maximum is known:
 *        rag_hybrid_linear_begin_dev  ->  gather 1: [world][Q] float64 maxima  ->  rag_hybrid_linear_finish_dev  ->
 *        gather 2: [world][5][Q][k] int64 blocks  ->  rag_hybrid_linear_merge_gathered_dev.
 * rag_hybrid_linear_batch: *max_queries_out = the query sub-batch rag_hybrid_linear_dev uses for the index as it stands,
 *   min(256, 8 GiB / (12 * rows)), at least 16. One begin / finish pair takes at most this many queries (the all-document score
 *   planes of one sub-batch are what the handle keeps between the two calls); ranks with different row counts agree on the
 *   smallest. Host state only: it waits for nothing.
 * rag_hybrid_linear_begin_dev: the first half of rag_hybrid_linear_dev for n_queries <= that limit (above it RAG_ERR_ARG, the
 *   message names the limit): one scoring pass writes every document's raw BM25 score into the handle's workspace and
 *   local_max_out_dev [n_queries] float64 = the largest raw score over this handle's visible documents of the query's tenant
 *   (deleted rows and other tenants' rows do not count), -inf when there is no such document. The handle keeps the score planes
 *   and the queries' token counts, and remembers n_queries, the row count and the tenant argument: it is "begun".
 * rag_hybrid_linear_finish_dev: gathered_max_dev [world][n_queries] float64, every rank's local maxima. Per query the maximum of
 *   the FINITE entries is the corpus maximum; with none (no document anywhere) the divisor is 1.0, as it is for a corpus maximum
 *   <= 0. Then the second half of rag_hybrid_linear_dev with that divisor: partial_out_dev [5][n_queries][k] int64 = ids | hybrid |
 *   semantic | keyword | temporal, the four score planes float64 bits, padded -1 / 0.0. world = 1 with the handle's own maxima
 *   gives the bits of rag_hybrid_linear_dev. q_dev 16-byte aligned (else RAG_ERR_ARG). The call consumes the begun state,
 *   whatever it returns. RAG_ERR_STATE: no begin
 *   before it; n_queries or the tenant argument (scalar against array, or other numbers) differ from the begin's; or the planes
 *   are gone - any *_host call on the handle in between (every write to the index or the postings is one, the live writes
 *   included), a device-pointer index load or append, or rag_hybrid_linear_dev / _tenants_dev, which reuse the workspace.
 *   Other *_dev calls may come in between.
 * Both: argument checks are rag_hybrid_linear_dev's (alpha > 0, finite weights, 0 < k <= 256, fresh row-aligned postings, a
 *   loaded tenant table for a tenant >= 0); an index with explicit ids under the gate of rag_m3_score_ids_dev: accepted with
 *   the id map enabled and ids_ascending (no lookup is made, only the order is needed), else RAG_ERR_STATE. The handle stays usable after every error.
 * rag_hybrid_linear_merge_gathered_dev: gathered_dev [world][5][n_queries][k] int64, every rank's partial_out. The global top-k
 *   by (hybrid desc, id asc), -1 slots skipped wherever they stand, each winner's three components copied with it; outputs
 *   [n_queries][k], padded -1 / 0.0; semantic / keyword / temporal_out_dev may be NULL. Needs no index. world * k <= 4092 (the
 *   merge kernel's LDS), else RAG_ERR_ARG.
 * Bit-identical (ids, hybrid and component bits) to rag_hybrid_linear_dev on the unsharded index loaded with id_base = 0, the
 *   merged postings and the whole temporal vector: the raw scores are per-document sums over the query's terms under global
 *   statistics, the maximum of the ranks' maxima is the corpus maximum, every other operand is per row, and the order (hybrid
 *   desc, id asc) is total, so the merge of the ranks' top-k lists is the top-k of the union.
 * The _tenants_ forms take tenants_host [n_queries] as the other per-query-tenant entries do. All follow the preamble's ordering
 *   rules; workspaces are handle-owned. */
int rag_hybrid_linear_batch(rag_handle_t h, int* max_queries_out);
int rag_hybrid_linear_begin_dev(rag_handle_t h, const int32_t* term_ptr_dev, const int32_t* terms_dev, int n_queries, int tenant,
                                double* local_max_out_dev, void* stream);
int rag_hybrid_linear_finish_dev(rag_handle_t h, const float* q_dev, const double* gathered_max_dev, int world, int n_queries, int k,
                                 double alpha, double beta, double gamma, int tenant, int64_t* partial_out_dev, void* stream);
int rag_hybrid_linear_merge_gathered_dev(rag_handle_t h, const int64_t* gathered_dev, int world, int n_queries, int k,
                                         int64_t* ids_out_dev, double* hybrid_out_dev, double* semantic_out_dev /*may be NULL*/,
                                         double* keyword_out_dev /*may be NULL*/, double* temporal_out_dev /*may be NULL*/,
                                         void* stream);

/* ---- agents mixed in one batch: a tenant PER QUERY. Each entry takes the arguments of its namesake with
 *      `const int32_t* tenants_host` [n_queries] where the namesake has `int tenant`: query i is filtered by tenants_host[i],
 *      a value < 0 leaves that query unfiltered. The result of query i is bit-identical to what the namesake returns for that
 *      query alone with tenant = tenants_host[i] (ids, rows, float64 score bits, raw maxima, candidate lists, logits): a tenant
 *      that owns no live row gives an all-padding result (-1 / 0.0), one with fewer than k live rows is padded, deleted rows
 *      stay hidden, and the linear fusion normalises each query's keyword score by its own tenant's best document.
 *      tenants_host is HOST memory in the *_dev entries too: the tenant number is what the caller's agent table holds on the
 *      host, and the library chooses the tiles to search from it there. It is consumed before the call returns (the caller may
 *      overwrite or free it at once); the device copy is written as ordinary work of `stream`, so the ordering rules of the
 *      preamble hold unchanged and, in the steady state, the call waits for nothing (the first call of a larger batch or of
 *      a longer tile union grows a handle-owned buffer, as workspace growth does in the preamble).
 *      Argument checks are the namesakes': a tenant >= 0 needs rag_index_set_tenants_host over the index's rows (a stale
 *      table is RAG_ERR_ARG), BM25 / hybrid / pipeline entries need postings that are row-aligned and not stale
 *      (RAG_ERR_STATE). A batch whose queries all name the same tenant (or none) runs exactly the namesake's path.
 *      Cost: the dense pass searches the union of the batch's tenants' tiles when every query is filtered and that union is
 *      shorter than the table, else every tile; each query filters the other tenants' rows out of it. */
int rag_dense_topk_tenants_host(rag_handle_t h, const float* q_host, int n_queries, int k, const int32_t* tenants_host,
                                int64_t* ids_out_host, int32_t* rows_out_host, double* scores_out_host);
int rag_dense_topk_tenants_dev(rag_handle_t h, const float* q_dev, int n_queries, int k, const int32_t* tenants_host,
                               int64_t* ids_out_dev, int32_t* rows_out_dev, double* scores_out_dev, void* stream);
int rag_bm25_topk_tenants_host(rag_handle_t h, const int32_t* term_ptr_host, const int32_t* terms_host, int n_queries, int k,
                               const int32_t* tenants_host, int64_t* ids_out_host, int32_t* rows_out_host,
                               double* scores_out_host, double* raw_max_out_host);
int rag_bm25_topk_tenants_dev(rag_handle_t h, const int32_t* term_ptr_dev, const int32_t* terms_dev, int n_queries, int k,
                              const int32_t* tenants_host, int64_t* ids_out_dev, int32_t* rows_out_dev, double* scores_out_dev,
                              double* raw_max_out_dev, void* stream);
int rag_hybrid_rrf_tenants_dev(rag_handle_t h, const float* q_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                               int n_queries, int pool, int k, int rrf_k, const int32_t* tenants_host, int64_t* lists_ws_dev,
                               double* scores_ws_dev, int64_t* keys_out_dev, double* rrf_out_dev, int32_t* ranks_out_dev,
                               void* stream);
int rag_hybrid_linear_tenants_dev(rag_handle_t h, const float* q_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                                  int n_queries, int k, double alpha, double beta, double gamma, const int32_t* tenants_host,
                                  int64_t* ids_out_dev, int32_t* rows_out_dev, double* hybrid_out_dev, double* semantic_out_dev,
                                  double* keyword_out_dev, double* temporal_out_dev, void* stream);
int rag_hybrid_linear_begin_tenants_dev(rag_handle_t h, const int32_t* term_ptr_dev, const int32_t* terms_dev, int n_queries,
                                        const int32_t* tenants_host, double* local_max_out_dev, void* stream);
int rag_hybrid_linear_finish_tenants_dev(rag_handle_t h, const float* q_dev, const double* gathered_max_dev, int world, int n_queries,
                                         int k, double alpha, double beta, double gamma, const int32_t* tenants_host,
                                         int64_t* partial_out_dev, void* stream);
int rag_retrieve_rerank_tenants_dev(rag_handle_t h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                                    const int32_t* q_tok_dev, const int32_t* q_len_dev, int Lq, int n_queries, int pool, int k,
                                    int rrf_k, const int32_t* tenants_host, int mode, int cls_id, int sep_id, int L_pair,
                                    int64_t* ids_out_dev, double* scores_out_dev, float* logits_out_dev, int64_t* cand_out_dev,
                                    void* stream);
/* The learned-sparse index and the bge-m3 composites (outputs as their namesakes': ids, rows, float64 scores, RRF scores and
 * ranks, components_out, cand_out). "Matches nothing" combines with the query's own tenant: a document is listed only if it is
 * visible to that query and its score is > 0. Only the candidate searches see the tenants: the MaxSim, cosine, point-lookup and
 * combine steps score the rows they are handed, which arrive filtered. The explicit-row entries (rag_tokvec_rerank_dev,
 * rag_m3_score_rows_dev, rag_sparse_score_rows_*) never look at visibility and have no such form. */
int rag_sparse_topk_tenants_host(rag_handle_t h, const int32_t* term_ptr_host, const int32_t* terms_host,
                                 const float* qweights_host, int n_queries, int k, const int32_t* tenants_host, int64_t* ids_out,
                                 int32_t* rows_out /*may be NULL*/, double* scores_out);
int rag_sparse_topk_tenants_dev(rag_handle_t h, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev,
                                int n_queries, int k, const int32_t* tenants_host, int64_t* ids_out_dev,
                                int32_t* rows_out_dev /*may be NULL*/, double* scores_out_dev, void* stream);
int rag_hybrid_sparse_rrf_tenants_dev(rag_handle_t h, const float* q_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                                      const float* qweights_dev, int n_queries, int pool, int k, int rrf_k,
                                      const int32_t* tenants_host, int64_t* lists_ws_dev, double* scores_ws_dev,
                                      int64_t* keys_out_dev, double* rrf_out_dev, int32_t* ranks_out_dev, void* stream);
int rag_retrieve_maxsim_tenants_dev(rag_handle_t h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                                    const float* qweights_dev, const float* q_vecs_dev, const int64_t* q_off_dev, int n_queries,
                                    int pool, int k, int rrf_k, const int32_t* tenants_host, int mode, int64_t* ids_out_dev,
                                    double* scores_out_dev, int64_t* cand_out_dev /*may be NULL*/, void* stream);
int rag_retrieve_m3_tenants_dev(rag_handle_t h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                                const float* qweights_dev, const float* q_vecs_dev, const int64_t* q_off_dev, int n_queries, int pool,
                                int k, int rrf_k, const int32_t* tenants_host, int mode, double w_dense, double w_sparse,
                                double w_colbert, int64_t* ids_out_dev, double* scores_out_dev,
                                double* components_out_dev /*may be NULL*/, int64_t* cand_out_dev /*may be NULL*/, void* stream);

/* ---- bge-m3 search from query token ids in one device-resident call: the forward, the compaction of its lexical weights and the
 *      three-way search, with nothing on the host in between (no reference counterpart).
 * rag_search_m3_tokens_dev is rag_embed_multi_dev on the handle's embedder (input_ids / token_type_ids [n_queries][seq_len],
 *   lens [n_queries]) into handle-owned buffers - dense [Q][hidden], lexical weights [Q][seq_len], token vectors at a capacity of
 *   Q * (seq_len - 1) rows (a text never has more: the capacity is known without reading lens) and their row offsets - then
 *   rag_lexical_compact_dev (skip_ids_host / n_skip: its arguments) at capacity Q * seq_len, then rag_retrieve_m3_dev with q_off =
 *   the forward's row offsets; pool, k, rrf_k, tenant, mode, the weights and the four outputs are rag_retrieve_m3_dev's. EVERY
 *   OUTPUT IS BIT-IDENTICAL to those three calls made one after another by the caller, for every mode and weight set: the call runs
 *   the same three functions with the same arguments on `stream`.
 *   What is not needed is neither computed nor required: w_colbert == 0 takes no token-vector head, workspace or store; w_sparse == 0
 *   with mode 0 takes no lexical head, no compaction and no postings.
 *   RAG_ERR_STATE: no embedder loaded (rag_embed_load_host), or a head the weights or the mode need is missing
 *   (rag_embed_heads_load_host); RAG_ERR_ARG: an embedder whose output width differs from the index dimension, or whose token
 *   vectors are not as wide as the resident store's; n_queries / seq_len outside rag_lexical_compact_dev's limits. Every argument
 *   and state error of the three underlying calls keeps its own code and message; those of the search and of the forward are
 *   reported before anything is queued.
 *   The buffers are planes of the handle-owned pipeline workspace, carved once per call beside rag_retrieve_m3_dev's own: nothing
 *   waits for the device in the steady state; the first call of a larger shape grows the workspace as the preamble says.
 * rag_search_m3_tokens_tenants_dev: the same with a tenant per query, under the rules of the "a tenant PER QUERY" block above. */
int rag_search_m3_tokens_dev(rag_handle_t h, const int32_t* input_ids_dev, const int32_t* token_type_ids_dev, const int32_t* lens_dev,
                             int n_queries, int seq_len, const int32_t* skip_ids_host, int n_skip, int pool, int k, int rrf_k, int tenant,
                             int mode, double w_dense, double w_sparse, double w_colbert, int64_t* ids_out_dev, double* scores_out_dev,
                             double* components_out_dev /*may be NULL*/, int64_t* cand_out_dev /*may be NULL*/, void* stream);
int rag_search_m3_tokens_tenants_dev(rag_handle_t h, const int32_t* input_ids_dev, const int32_t* token_type_ids_dev,
                                     const int32_t* lens_dev, int n_queries, int seq_len, const int32_t* skip_ids_host, int n_skip,
                                     int pool, int k, int rrf_k, const int32_t* tenants_host, int mode, double w_dense, double w_sparse,
                                     double w_colbert, int64_t* ids_out_dev, double* scores_out_dev,
                                     double* components_out_dev /*may be NULL*/, int64_t* cand_out_dev /*may be NULL*/, void* stream);

/* ---- the exchange step of the row-sharded search (the reference is single-process) bound to RCCL
 *      directly, for hosts that do not want torch.distributed in the path: ONE all-gather of each rank's partial top-k lists
 *      per stage, over xGMI, followed by rag_merge_topk_dev / rag_rrf_fuse_dev on every rank. librccl is opened at the first
 *      call (dlopen; the library has no link-time dependency on it).
 *      rag_comm_unique_id: 128 bytes created on ONE rank and handed to the others out of band (file, socket, torch store).
 *      rag_comm_init: collective over `world` ranks, one per GPU. rag_comm_allgather_dev: recv_dev[world][bytes] <- every
 *      rank's send_dev[bytes], asynchronous on `stream`. */
int rag_comm_unique_id(void* id128_out);
int rag_comm_init(rag_handle_t h, int rank, int world, const void* id128);
int rag_comm_allgather_dev(rag_handle_t h, const void* send_dev, void* recv_dev, size_t bytes, void* stream);
/* ranks of the communicator the gathers run on, as RCCL itself counts them (ncclCommCount): what bench.py reports next to the
 * rank count of torch's own collective layer */
int rag_comm_count(rag_handle_t h, int* count_out);
int rag_comm_destroy(rag_handle_t h);

#ifdef __cplusplus
}
#endif
#endif /* RAG_HIP_H */
