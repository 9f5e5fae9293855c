// Shared declarations for librag_hip.so (gfx950 only). See include/rag_hip.h for the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/rag_hip.h"

typedef _Float16 half_t;
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define RAG_CAND_CAP 4096        // per-query candidate buffer entries (u64 keys)
#define RAG_STAGE0_ROWS 2048     // rows whose scores are stored densely (no threshold yet)
#define RAG_STAGE_GROWTH 8       // each threshold stage covers ~8x the rows seen so far (RAG_STAGE_GROWTH env overrides, for tuning)
#define RAG_TILE 256             // GEMM tile edge (corpus rows x queries)
#define RAG_BK 64                // K-slice per LDS stage (halfs)
#define RAG_MAX_K 256            // largest k / shortlist supported by the select kernels
#define RAG_SCALE_LOG2 7         // unit rows are stored as fp16(128 * x): keeps fp16 out of subnormals

#define RAG_PROF_STAGES 3
struct rag_ce_model;             // cross_encoder.hip
struct rag_bm25_index;           // bm25.hip
struct rag_ctx;

// ---- device memory: the ONE owner of a hipMalloc allocation (and the only place that calls hipMalloc / hipFree). Move-only;
// the destructor, reset() and every re-allocation hipFree at once (callers rely on hipFree waiting for the device). Reads as
// a T* in kernel launches, copies and pointer arithmetic; structs passed to kernels by value keep raw pointers.
template <class T>
struct dev_buf {
    dev_buf() = default;
    dev_buf(dev_buf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    dev_buf& operator=(dev_buf&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~dev_buf() { reset(); }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    int alloc(rag_ctx* h, size_t n);                     // frees what it holds; RAG_ERR_HIP (h->err set, left empty) on failure
    int reserve(rag_ctx* h, size_t n) { return n <= n_ ? RAG_OK : alloc(h, n); }     // grow-only: contents are NOT kept
    operator T*() const { return p_; }
    T* get() const { return p_; }
    size_t size() const { return n_; }                   // elements

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

// Diagnostic / tuning switches of one handle. The defaults come from the environment (RAG_<NAME>) ONCE, in rag_create;
// rag_set_option(h, "<name>", value) changes them afterwards (tests flip them between calls on one handle). Nothing on a
// search path calls getenv.
struct rag_options {
    int force_level = 0;          // 1 / 2: every dense query through the wide ranking / the float64 exact scan
    int stage_growth = 0;         // dense stage growth (0 = the built-in schedule)
    int no_smallq = 0;            // disable the small-batch dense kernel variant
    int no_second_pass = 0;       // overflowed dense queries go straight to the float64 scan
    int dense_persist = 0;        // (experiment) thresholded stages as one persistent workgroup per CU instead of one workgroup per tile
    int dense_linear_order = 0;   // walk the tiles in table order (r1 behaviour, for A/B)
    int bm25_first_ranges = 0;    // exact first-stage BM25 ranges (0 = BM_FIRST_RANGES)
    int bm25_no_staging = 0;      // exact per-range select for every BM25 range
    int bm25_linear_grid = 0;     // scoring workgroups range-major (the ranges of one query side by side) instead of the XCD-aware column order
    int bm25_sort_merge = 0;      // fold the partial lists of a stage by the bitonic-sort kernel (r1-r2) instead of the per-wave selection
    int bm25_plan_slots = 0;      // planned token slots per query of a BM25 call (0 = sized by the per-call budget, bm25_pick_plan_t); tests force 8
    int bm25_ws_mb = 0;           // workspace budget of a device-pointer BM25 call in MiB (0 = 6 GiB): batches beyond it run in sub-batches
    int bm25_packed = 0;          // (read when postings are LOADED) 4-byte packed postings + shared impact table instead of (doc, impact)
    int bm25_keep_tf = 0;         // (read when postings are LOADED) keep uint16 term frequencies + document lengths (a packed base: its value tables) so that rag_bm25_refresh can recompute every impact on the device: +2 B per posting, +4 B per document
    int bm25_tail_fold = 0;       // appended postings: an append folds the tail into the base once it holds more than this many documents (-1 = never, 0 = the default policy, bm25.hip bm_default_fold_docs)
    int sparse_tail_fold = 0;     // the same for appended learned-sparse postings (rag_sparse_append_host)
    int tokvec_compact_rows = 0;  // rag_index_compact_live: token rows per staging chunk of the token-vector move (0 = sized from the staging bound); tests force a small value
    int tokvec_scan_ws_mb = 0;    // exhaustive MaxSim search (rag_retrieve_maxsim_dev mode 2): bound of the key plane [Qb][documents] in MiB (0 = 2048): batches beyond it run in sub-batches of Qb queries
    int tokvec_scan_queries = 0;  // ... or Qb itself (0 = derived from the bound); tests force small values
    int no_fork = 0;              // keep the BM25 leg of a small hybrid batch in line on the caller's stream
    int fork_max_q = 0;           // largest batch whose BM25 leg runs on the side stream beside the dense leg (0 = RAG_FORK_MAX_Q)
    int ce_chunk_tokens = 0;      // activation chunk size in tokens (0 = sized from the model)
    int ce_mx = 0;                // cross-encoder forward on hi16 + lo8 operands (ce_mx.h) wherever the shape allows it: 0 = yes if the load-time probe saw it hold (cross_encoder.hip ce_probe_mx), 1 = yes, -1 = never
    int ce_ffn_fused = 0;         // MX forward: FFN-up and FFN-down of a layer as ONE launch whose intermediate stays in per-workgroup slots (ce_mx.h mx_ffn_kernel): 0 = where the slots fit the cache (cross_encoder.hip mx_ffn_fused), 1 = always, -1 = never (two launches through h8); same bits either way
    int ce_attn_stream = 0;       // 64-wide heads, length classes above 512: 0 = the streamed attention kernel where it is the default (cross_encoder.hip launch_attention64), -1 = DIRECT everywhere above class 256, 1 = streamed at every class above 512
};

// Candidate state of one emit / select pass over `rows` queries (a multiple of RAG_TILE): dense.hip runs the batch through one
// instance and the re-emission of overflowed queries through a second, one tile wide.
struct dense_ws {
    dev_buf<half_t> q16;             // [rows][dim_pad]  fp16 unit query rows; pad rows of a query tile must be zero
    dev_buf<uint64_t> cand;          // [rows][RAG_CAND_CAP]
    dev_buf<unsigned> cnt;           // [rows]   emitted candidates (may exceed cap = overflow)
    dev_buf<float> tau;              // [2][rows] emission threshold = k-th best fp16-pass score so far - 2 eps; behind the thresholds of
                                     //          a pass, the int32 tenants of its query columns (per-query tenants, dense.hip column_tenants)
    dev_buf<float> bound;            // [rows]   -inf, or +inf once the candidate buffer overflowed (sticky)
    dev_buf<int> n_sorted;           // [rows]   survivors left in cand[] after the final select
    int alloc(rag_ctx* h, size_t rows, hipStream_t st);      // (re)allocates every plane and enqueues the zero fill of q16 on st
};

// Every device allocation of a handle, in two groups so that each can be released as a whole by assigning an empty value:
// the planes of the dense index (dropped by every index load, dense_free) ...
struct rag_index_mem {
    dev_buf<float> emb32;            // [n_rows][dim]        fp32 master rows
    dev_buf<half_t> emb16;           // [emb16_rows][dim_pad] fp16 (2^7 * unit rows), zero padded
    dev_buf<int64_t> ids;            // [n_rows] or null
    dev_buf<int32_t> tenants;        // [n_rows] or null
    dev_buf<int> bad_rows;           // device counter: rows with zero / non-finite norm
    dev_buf<char> scan_scores;       // exact-scan fallback: partial lists, 12 B per entry (allocated on first use)
    dev_buf<int32_t> tenant_tiles;   // concatenated per-tenant lists of 256-row tiles
    // live writes (live.hip). vis[row] = the row's tenant (0 without a tenant table) or RAG_DEAD_ROW once deleted; null while
    // nothing is deleted, so the search kernels keep their unfiltered path.
    dev_buf<int32_t> vis;
    // id-to-row map (idmap.hip, rag_index_id_map): open addressing over [slots] keys and rows, and its device counters
    dev_buf<int64_t> idmap_keys;     // [slots] id, or IDMAP_EMPTY
    dev_buf<int32_t> idmap_rows;     // [slots] row of the key, -1 = erased (a tombstone: the key stays)
    dev_buf<unsigned long long> idmap_stat;      // [IDMAP_STAT_WORDS]
};
// ... and everything else (dropped by rag_destroy, with the index planes)
struct rag_device_mem : rag_index_mem {
    dev_buf<double> side_scores;     // hybrid_legs: score scratch of the BM25 leg on the side stream
    dev_buf<double> temporal;        // [n_rows] per-row temporal score (linear fusion) or null
    dev_buf<char> lin_ws;            // rag_hybrid_linear_dev: raw BM25 + bias + max of one sub-batch (api.hip linear_ws); kept between rag_hybrid_linear_begin_dev and its finish
    // dense search workspace (sized for ws_q queries): the batch's candidate state, and what only the whole batch needs
    dense_ws ws;                     // [ws_qpad] rows
    dev_buf<float> q32;              // [ws_q][dim]     staging for host queries
    dev_buf<double> exact;           // [ws_qpad][RAG_CAND_CAP] float64 rescored cosines
    dev_buf<int> flag;               // [ws_qpad]   0 done, 2 needs exact scan, 3 scanned
    dev_buf<int> scan_list;          // [ws_qpad]   queries flagged 2 (appended by finalize_kernel; count = stats[7])
    dev_buf<int> stats;              // [8] device counters
    // second pass for overflowed queries: one 256-query tile of its own (dense.hip), and the list of those queries
    dense_ws ws_ovf;                 // [RAG_TILE] rows
    dev_buf<int> ovf_list;           // [RAG_TILE + 1] overflowed queries (appended by the final select), then their count
    // grow-only device arena of the synchronous *_host entry points: their per-call staging (queries in, results out, partial
    // lists) is carved from it, so an agent-facing call pays no allocation
    dev_buf<char> stage;
    // passage token store (pipeline.hip): [tok_rows][tok_L] uint16 WordPiece ids + lengths, row-aligned with the index
    dev_buf<uint16_t> tok;
    dev_buf<uint8_t> tok_hi;         // [tok_rows][tok_L] bits 16-23 of the ids: present iff the store is 24 bits wide (rag_tokens_*_wide)
    dev_buf<int32_t> tok_len;
    dev_buf<int> tok_bad;            // device counter of out-of-range token ids seen by the appends
    dev_buf<char> pipe_ws;           // retrieve_rerank_dev: candidate lists, pair tokens, logits of one call
    // per-query tenants (the *_tenants_* entries, query_tenants below): the batch's tenant numbers and the union of the batch's
    // tenant tile lists
    dev_buf<int32_t> qten;           // [>= n_queries]
    dev_buf<int32_t> union_tiles;    // [<= tiles of the index]
    // resident token-vector store (tokvec.hip): packed fp16 rows, document i = rows [tv_off[i], tv_off[i + 1]) = row i of the index
    dev_buf<half_t> tv;              // [tv_rows_cap][tv_dim] (form RAG_TOKVEC_FP16)
    dev_buf<uint8_t> tv8;            // form RAG_TOKVEC_MXFP8: [tv_rows_cap] rows of tokvec_row_bytes: dim E4M3 codes | dim / 32 E8M0 scales | pad to 16 B
    dev_buf<int64_t> tv_off;         // [tv_docs_cap + 1], tv_off[0] = 0
    dev_buf<int> tv_bad;             // [2] device counters of one append: values that are not finite as fp16, decreasing offsets
    dev_buf<char> tv_ws;             // rag_tokvec_rerank_*: pair scores float32 [Q][pool] | scored rows int32 [Q][pool] (-1 = empty slot)
};

struct rag_ctx : rag_device_mem {
    int device = 0;
    int n_cu = 0;                // compute units of `device` (rag_create): sizes the persistent grids
    int dim = 0;
    int dim_pad = 0;             // multiple of RAG_BK
    hipStream_t stream = nullptr;
    hipStream_t side_stream = nullptr;       // hybrid_legs: the BM25 leg of a small batch runs beside the dense leg
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::string err;
    rag_options opt;
    bool profiling = false;
    void* comm = nullptr;                    // ncclComm_t of comm.hip (RCCL, opened with dlopen), or null
    int comm_rank = 0, comm_world = 1;

    // dense index
    int64_t n_rows = 0, id_base = 0;
    bool index_loaded = false;   // rag_index_load_* / rag_index_reserve ran (an EMPTY index is a valid, searchable state)
    int64_t n_reserved = 0;      // rows allocated by rag_index_reserve (chunked bulk load), 0 otherwise
    double temporal_absmax = 0.0;                                      // max |temporal[i]| (sizes the fused emission margin)
    // rag_hybrid_linear_begin_dev ran and lin_ws still holds its score planes: what rag_hybrid_linear_finish_dev must be called
    // with. Dropped by finish, by rag_hybrid_linear_dev (it reuses lin_ws) and by every *_host entry (host_after_dev: each write
    // to the index or the postings is one).
    struct { bool on = false; int Q = 0; int64_t n_rows = 0; int tenant = -1; std::vector<int32_t> tenants; } lin_begun;
    std::unordered_map<int32_t, std::pair<int64_t, int>> tenant_span;  // tenant -> (offset, count) into tenant_tiles
    std::unordered_map<int32_t, std::vector<int32_t>> tenant_lists;    // host copy of those lists (inserts extend them)
    int64_t tenant_rows = 0;                                           // row count the tenant table was built for
    // live writes (live.hip). The row capacity of a plane is not kept here: it is its buffer's element count over its row
    // width (plane_rows and the row-plane list below), 0 for a plane that is absent.
    int64_t n_deleted = 0;
    // id-to-row map (idmap.hip): on = rag_index_id_map(h, 1) was called and every write keeps the map current. The table itself
    // (rag_index_mem::idmap_keys) exists only while the index stores explicit ids; slots == 0 without it.
    struct idmap_state {
        bool on = false;
        bool ascending = true;       // the ids of the live rows ascend strictly with the rows (implicit ids always do)
        int64_t slots = 0, entries = 0, tombstones = 0, longest_probe = 0, rebuilds = 0;
    } idmap;
    bool bm25_stale = false;     // rows were inserted or compacted since the postings were loaded: BM25 entry points refuse
    bool bm25_compacted = false; // ... and a compaction was among them: appended postings cannot align the rows again, only a reload

    // set by every *_dev entry, cleared by the device-wide wait a *_host entry then starts with (host_after_dev): a *_host
    // call behaves as if it ran after all *_dev work of the handle, on whatever stream that was queued
    bool dev_pending = false;
    int ws_q = 0;                    // queries the dense search workspace is sized for
    int q16_dirty = 0;               // rows [q16_dirty, ws_qpad) of ws.q16 are known to be zero (pad rows of a query tile must be)
    // one lock per handle, taken by every entry point: the reference's DocumentStore.search may be called from up to 10
    // threads (database/connection.py:38-42). *_host calls are then fully thread-safe (they are synchronous inside the
    // lock); *_dev calls are serialised while they enqueue and share the handle's workspaces, so they must target ONE stream.
    std::mutex mu;

    // profiling (rag_set_profiling): HIP event pairs recorded on the launch stream around the spans bench.py prices against
    // a roofline. Stage 0 = every dense_emit_kernel<false> launch, 1 = the BM25 range + merge launches of one top-k call,
    // 2 = one cross-encoder forward (all chunks of a rag_ce_score_dev / rag_retrieve_rerank_dev call).
    struct prof_spans { std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; int used = 0; };
    prof_spans prof[RAG_PROF_STAGES];
    rag_dense_stats last_stats = {};
    bool last_stats_valid = false;
    int last_q = 0, last_k = 0, last_stages = 0, last_shortlist = 0;
    double last_eps = 0;

    rag_bm25_index* bm25 = nullptr;
    rag_bm25_index* sparse = nullptr;        // learned-sparse postings (rag_sparse_load_host): a slot of its own beside the BM25 postings
    bool sparse_stale = false;               // rows were inserted or compacted since they were aligned: sparse entry points refuse until rag_sparse_append_host covers the inserted rows, or a reload
    bool sparse_compacted = false;           // ... and a plain compaction was among them: only a reload helps
    int64_t tok_rows = 0;                    // token store: rows filled so far (its reservation: tok_cap_rows below)
    int tok_L = 0;
    int64_t tv_docs = 0, tv_rows = 0;        // token-vector store: documents / rows appended so far ...
    int64_t tv_docs_cap = 0, tv_rows_cap = 0;    // ... and reserved (rag_tokvec_reserve); tv_docs_cap > 0 = a store exists
    int tv_dim = 0;
    int tv_form = 0;                         // RAG_TOKVEC_FP16 / RAG_TOKVEC_MXFP8, chosen by the reserve
    bool tv_stale = false;                   // a compaction renumbered the rows since the store was filled: its entries refuse until a reload
    int pair_format = RAG_PAIR_BERT;         // rag_ce_set_pair_format: read while a pair-building call enqueues
    // hipFuncSetAttribute (dynamic LDS above 64 KiB) is per device: remembered per handle, not per process. raise_lds: the
    // dynamic LDS each group of kernels was last raised to. dense.hip: the emit instantiations by [DENSE0][SMALLQ][FUSED], the
    // persistent ones by [FUSED], the select kernel; bm25.hip: the range kernels. cross_encoder.hip: the two GEMM families, and
    // the attention instantiations by [MX operands][query blocks per wave]: every instantiation is a kernel of its own.
    int attr_dense_emit_lds[2][2][2] = {}, attr_dense_persist_lds[2] = {}, attr_dense_select_lds = 0, attr_bm25_lds = 0;
    int attr_ce_gemm_lds = 0, attr_ce_mx_lds = 0, attr_ce_ffn_lds = 0;
    int attr_ce_attn_lds[2][3] = {};
    int attr_ce_attn64_lds = 0;              // the LDS-staged instance of ce_attention64_kernel (64-wide heads)
    int attr_ce_attn64s_lds = 0;             // its streamed instance (the length classes above 512)
    int attr_m3_gemm_lds = 0;                // the split GEMM with the fp32 epilogue (the embedder's token-vector head)
    int attr_m3_compact_lds = 0;             // the two instances of m3_lexical_compact_kernel (m3_heads.hip): 64 KiB of keys at seq_len 8192
    rag_ce_model* ce = nullptr;
    rag_ce_model* emb = nullptr;             // sentence-embedding encoder (rag_embed_load_host): the K7 kernels behind a mean-pooling head
};

#define HIP_TRY(h, expr)                                                                      \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                     \
            return RAG_ERR_HIP;                                                               \
        }                                                                                     \
    } while (0)

template <class T>
int dev_buf<T>::alloc(rag_ctx* h, size_t n) {
    reset();
    HIP_TRY(h, hipMalloc(&p_, n * sizeof(T)));
    n_ = n;
    return RAG_OK;
}

inline int dense_ws::alloc(rag_ctx* h, size_t rows, hipStream_t st) {
    int rc;
    if ((rc = q16.alloc(h, rows * h->dim_pad))) return rc;
    if ((rc = cand.alloc(h, rows * RAG_CAND_CAP))) return rc;
    if ((rc = cnt.alloc(h, rows))) return rc;
    if ((rc = tau.alloc(h, 2 * rows))) return rc;
    if ((rc = bound.alloc(h, rows))) return rc;
    if ((rc = n_sorted.alloc(h, rows))) return rc;
    // zero fills go on the search's own stream: a null-stream hipMemset is not ordered against a non-blocking stream
    HIP_TRY(h, hipMemsetAsync(q16, 0, rows * h->dim_pad * sizeof(half_t), st));
    return RAG_OK;
}

// one lock per handle (rag_ctx::mu): the first statement of every entry point
#define LOCK(h) std::lock_guard<std::mutex> lock_((h)->mu)

// ---- row-aligned planes: the buffers that hold one row per index row. THE list, in the order writes visit them, each with its
// row width in elements. f(plane id, pointer to the member of rag_device_mem, width) is called per plane until one returns
// non-zero; the member pointer applies to a handle and to any other rag_device_mem (the grown set of an insert) alike. A new
// plane is one line here plus what live.hip says about who feeds it (insert_feeds) and how it enters the index.
enum { PLANE_EMB32, PLANE_EMB16, PLANE_IDS, PLANE_TENANTS, PLANE_TEMPORAL, PLANE_VIS, PLANE_TOK, PLANE_TOK_HI, PLANE_TOK_LEN };
template <class F>
static int for_each_row_plane(const rag_ctx* h, F&& f) {
    int rc;
    if ((rc = f(PLANE_EMB32, &rag_device_mem::emb32, (int64_t)h->dim))) return rc;
    if ((rc = f(PLANE_EMB16, &rag_device_mem::emb16, (int64_t)h->dim_pad))) return rc;
    if ((rc = f(PLANE_IDS, &rag_device_mem::ids, (int64_t)1))) return rc;
    if ((rc = f(PLANE_TENANTS, &rag_device_mem::tenants, (int64_t)1))) return rc;
    if ((rc = f(PLANE_TEMPORAL, &rag_device_mem::temporal, (int64_t)1))) return rc;
    if ((rc = f(PLANE_VIS, &rag_device_mem::vis, (int64_t)1))) return rc;
    if ((rc = f(PLANE_TOK, &rag_device_mem::tok, (int64_t)h->tok_L))) return rc;
    if ((rc = f(PLANE_TOK_HI, &rag_device_mem::tok_hi, (int64_t)h->tok_L))) return rc;
    return f(PLANE_TOK_LEN, &rag_device_mem::tok_len, (int64_t)1);
}
// rows a plane has room for: 0 for an absent one
template <class T>
static inline int64_t plane_rows(const dev_buf<T>& b, int64_t width) { return width > 0 ? (int64_t)(b.size() / (size_t)width) : 0; }
static inline int64_t emb32_rows(const rag_ctx* h) { return plane_rows(h->emb32, h->dim); }
// the padded leading dimension of the fp16 operand (a multiple of RAG_TILE * 8) and of everything laid out beside it
static inline int64_t emb16_rows(const rag_ctx* h) { return plane_rows(h->emb16, h->dim_pad); }
// the token store's reservation, from the plane whose row is one element: tok and tok_hi are allocated with it
static inline int64_t tok_cap_rows(const rag_ctx* h) { return (int64_t)h->tok_len.size(); }
// what the writes and the filtered searches ask of the planes beside the rows
static inline bool tenants_cover(const rag_ctx* h, int64_t n) { return h->tenant_rows == n && (int64_t)h->tenants.size() >= n; }   // the table and its tile lists are for exactly n rows
static inline bool ids_cover(const rag_ctx* h, int64_t n) { return !h->ids || (int64_t)h->ids.size() >= n; }                        // implicit ids always do
static inline bool tokens_aligned(const rag_ctx* h, int64_t n) { return h->tok != nullptr && h->tok_rows == n; }                    // a token store filled to exactly n rows

// ---- kernel launches. Launches kernel k with every argument converted to the kernel's own parameter type: a dev_buf<T> reads as
// its T* or const T*, nullptr as whatever pointer the kernel takes. The call sites keep only the casts that really reinterpret.
template <class... KArgs, class... Args>
static void launch(void (*k)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t st, Args&&... args) {
    hipLaunchKernelGGL(k, grid, block, lds, st, static_cast<KArgs>(args)...);
}

// what a function returns after its launches: the first launch error since the last check, as h->err
static inline int launch_status(rag_ctx* h) {
    HIP_TRY(h, hipGetLastError());
    return RAG_OK;
}

// Dynamic LDS above the 64 KiB default: hipFuncSetAttribute is per kernel instantiation and per device. `have` is the handle's
// field for exactly these kernels (rag_ctx attr_*), raised when a launch needs more than they were given so far.
template <class... K>
static int raise_lds(rag_ctx* h, int& have, int need, K... kernels) {
    if (need <= have) return RAG_OK;
    for (const void* k : {reinterpret_cast<const void*>(kernels)...})
        HIP_TRY(h, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, need));
    have = need;
    return RAG_OK;
}

#define ARG_CHECK(h, cond, msg)                                                               \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            (h)->err = std::string("bad argument: ") + (msg);                                 \
            return RAG_ERR_ARG;                                                               \
        }                                                                                     \
    } while (0)

// a caller array that a kernel reads 16 bytes at a time (float4: exact_norm2_wave, exact_cosine_wave, normalize_rows_kernel, the
// MaxSim row loads): the entry refuses any other address before it enqueues anything (include/rag_hip.h says "16-byte aligned")
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// ---- row visibility: the one predicate every search kernel applies to an index row. vis = rag_ctx::vis when rows are
// deleted (tenant numbers with RAG_DEAD_ROW for deleted rows), else the tenant table under a tenant filter, else null.
// tenant >= 0: the row belongs to that tenant (a deleted row never does); tenant < 0: the row is not deleted.
#define RAG_DEAD_ROW ((int32_t)0x80000000)
__device__ __forceinline__ bool row_visible(const int32_t* __restrict__ vis, int64_t row, int tenant) {
    if (vis == nullptr) return true;
    const int32_t v = vis[row];
    return tenant >= 0 ? v == tenant : v != RAG_DEAD_ROW;
}
// the vis argument of a search over the resident index (host side)
static inline const int32_t* search_vis(const rag_ctx* h, int tenant) {
    return h->vis ? h->vis.get() : (tenant >= 0 ? h->tenants.get() : nullptr);
}

// ---- per-query tenants (rag_*_tenants_*): query i of the batch is filtered by its own tenant, < 0 = not filtered. Both null: the
// call's scalar tenant holds for every query. host = the caller's array (read while the call enqueues: the tile universe is chosen
// from it), dev = its copy in rag_ctx::qten, written on the call's stream by stage_query_tenants. A sub-batch offsets both.
struct query_tenants { const int32_t* host; const int32_t* dev; };
static inline query_tenants operator+(query_tenants t, int q0) {
    return t.host ? query_tenants{t.host + q0, t.dev + q0} : t;
}
// the tenant a kernel applies to query q (qten = query_tenants::dev or null)
__device__ __forceinline__ int tenant_of_query(const int32_t* __restrict__ qten, int q, int tenant) {
    return qten != nullptr ? qten[q] : tenant;
}
// ---- id space: what a search leg reports for a row of the index. map[row] where there is a map, else base + row. A leg takes it
// as an argument and hands it to its kernels; it never reads rag_ctx::ids / id_base itself. The entries pass the index's mapping,
// the candidate stage of the resident composites (pipeline.hip) row numbers.
struct id_space {
    const int64_t* map; int64_t base;
    static id_space of_index(const rag_ctx* h) { return {h->ids.get(), h->id_base}; }
    static id_space rows() { return {nullptr, 0}; }
    bool identity() const { return map == nullptr && base == 0; }
};

// host words -> device memory as ordinary work of `st`: the words travel as kernel arguments, so the host array is consumed when
// this returns and nothing waits for the stream (a pageable hipMemcpyAsync would). dense.hip
int upload_i32(rag_ctx* h, int32_t* dst_dev, const int32_t* src_host, size_t n, hipStream_t st);
int stage_query_tenants(rag_ctx* h, const int32_t* tenants_host, int Q, hipStream_t st, query_tenants* out);

// ---- profiling spans (no-ops unless rag_set_profiling(h, 1))
static inline int prof_begin(rag_ctx* h, int stage, hipStream_t st) {
    if (!h->profiling) return RAG_OK;
    auto& p = h->prof[stage];
    if ((int)p.ev.size() <= p.used) {
        hipEvent_t a, b;
        HIP_TRY(h, hipEventCreate(&a));
        HIP_TRY(h, hipEventCreate(&b));
        p.ev.push_back({a, b});
    }
    HIP_TRY(h, hipEventRecord(p.ev[p.used].first, st));
    return RAG_OK;
}
static inline int prof_end(rag_ctx* h, int stage, hipStream_t st) {
    if (!h->profiling) return RAG_OK;
    auto& p = h->prof[stage];
    HIP_TRY(h, hipEventRecord(p.ev[p.used].second, st));
    p.used++;
    return RAG_OK;
}

// ---- ordering of *_host calls behind *_dev calls. A *_dev call leaves its work queued on the caller's stream; the *_host
// entries run on the handle's private non-blocking stream over the SAME workspaces (dense search state, the models' activation
// planes) and replace planes a queued call reads, and their host-side bookkeeping (ws_q, q16_dirty, the models' workspace sizes) assumes that
// enqueue order is device order. So a *_host entry first waits for the device when *_dev work was queued since the last wait.
// Nothing is added to either path while a caller stays with one kind of call: no HIP call, one flag.
static inline int host_after_dev(rag_ctx* h) {
    h->lin_begun.on = false;                 // (a begun linear fusion does not survive a *_host call: rag_ctx::lin_begun)
    if (!h->dev_pending) return RAG_OK;
    HIP_TRY(h, hipDeviceSynchronize());
    h->dev_pending = false;
    return RAG_OK;
}

// ---- staging arena (see rag_ctx::stage): sum stage_size() of every piece, stage_reserve() once, stage_take() in the same order
static inline size_t stage_size(size_t n, size_t elt) { return (size_t)round_up((int64_t)(n * elt), 256); }
static inline int stage_reserve(rag_ctx* h, size_t bytes) {
    if (bytes <= h->stage.size()) return RAG_OK;
    if (h->stage) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return h->stage.alloc(h, (size_t)round_up((int64_t)(bytes + bytes / 4), 1 << 20));      // headroom: slightly larger batches do not reallocate
}
template <class T>
static inline T* stage_take(char*& p, size_t n) {
    T* r = reinterpret_cast<T*>(p);
    p += stage_size(n, sizeof(T));
    return r;
}
// ---- a per-call workspace carved from one buffer. A `planes` function names every plane once, as p = c.take<T>(elements); it runs
// twice: without memory, which sums the sizes (stage_size: each plane starts on a 256-byte boundary), then over the reserved buffer.
struct ws_carve {
    char* base;
    size_t bytes = 0;
    template <class T>
    T* take(size_t n) {
        T* r = base ? reinterpret_cast<T*>(base + bytes) : nullptr;
        bytes += stage_size(n, sizeof(T));
        return r;
    }
};

// ---- sortable keys: larger key = higher score, then lower row ---------------------------------
__host__ __device__ static inline uint32_t f32_orderable(float s) {
    uint32_t u = __builtin_bit_cast(uint32_t, s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ static inline float f32_from_orderable(uint32_t u) {
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    return __builtin_bit_cast(float, u);
}
__host__ __device__ static inline uint64_t make_key(float score, uint32_t row) {
    return ((uint64_t)f32_orderable(score) << 32) | (uint64_t)(0xFFFFFFFFu - row);
}
__host__ __device__ static inline uint32_t key_row(uint64_t k) { return 0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFu); }
__host__ __device__ static inline float key_score(uint64_t k) { return f32_from_orderable((uint32_t)(k >> 32)); }
__host__ __device__ static inline uint64_t f64_orderable(double s) {
    uint64_t u = __builtin_bit_cast(uint64_t, s);
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
__host__ __device__ static inline double f64_from_orderable(uint64_t u) {
    u = (u & 0x8000000000000000ull) ? (u & 0x7fffffffffffffffull) : ~u;
    return __builtin_bit_cast(double, u);
}

// entry points implemented per file
int dense_index_build(rag_ctx* h, const float* emb_dev, int64_t n_rows, hipStream_t st);
int dense_index_normalize_range(rag_ctx* h, int64_t first_row, int64_t n_rows, hipStream_t st);
// linear fusion inputs of one query sub-batch (rag_hybrid_linear_dev): float32 emission bias [Q][bias_ld], float64 raw BM25
// scores [Q][n] with their per-query divisor, per-row temporal scores (or null), the three weights
struct dense_fused {
    const float* bias; int64_t bias_ld;          // float32 raw BM25 scores [Q][bias_ld] (written by the scoring kernel itself)
    const float* qscale;                         // [Q] float(beta / max of the query)
    const float* margin;                         // [Q] added to 2 * eps for a query whose |keyword score| exceeds 1 (linear_scale_kernel)
    const float* gt;                             // [bias_ld] float(gamma * temporal) or null
    const double* raw; int64_t n;
    const double* mx; const double* temporal;
    double alpha, beta, gamma;
};
// fz == nullptr: plain cosine top-k. Otherwise the linear fusion of rag_hybrid_linear_dev (dense.hip)
// ids: what ids_dev reports (id_space); qt: per-query tenants (then `tenant` is not read)
int dense_search_fused(rag_ctx* h, const float* q_dev, int Q, int k, int tenant, int64_t* ids_dev, int32_t* rows_dev,
                       double* scores_dev, hipStream_t st, const dense_fused* fz, id_space ids, query_tenants qt = {nullptr, nullptr});
static inline int dense_search(rag_ctx* h, const float* q_dev, int Q, int k, int tenant, int64_t* ids_dev, int32_t* rows_dev,
                               double* scores_dev, hipStream_t st, id_space ids, query_tenants qt = {nullptr, nullptr}) {
    return dense_search_fused(h, q_dev, Q, k, tenant, ids_dev, rows_dev, scores_dev, st, nullptr, ids, qt);
}
void comm_free(rag_ctx* h);
// pipeline.hip: the dense and the keyword leg of a hybrid search into lists_dev [2][Q][pool], both in the id space `ids`
int hybrid_legs(rag_ctx* h, const float* q_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev, int Q, int pool, int tenant,
                int64_t* lists_dev, double* scores_ws_dev, hipStream_t st, id_space ids, query_tenants qt = {nullptr, nullptr},
                const float* qweights_dev = nullptr);
// the query terms and what bounds a negative raw BM25 score from them (bm25_negative_bound_args)
struct linear_neg_bound { const int32_t* term_ptr; double per_token; };
int linear_prepare(rag_ctx* h, const unsigned long long* max_key, linear_neg_bound nb, int Q, int64_t n, const double* temporal,
                   double beta, double gamma, double* mx, float* qscale, float* margin, float* gt, int64_t ld, hipStream_t st);
int linear_components(rag_ctx* h, const float* q_dev, const int32_t* rows_dev, int Q, int k, const dense_fused* fz, double* sem_out,
                      double* kw_out, double* tmp_out, hipStream_t st);
// the fusion over row shards (rag_hybrid_linear_begin_dev / _finish_dev / _merge_gathered_dev): max_key <-> float64 maxima on each
// side of the gather, and the merge of the ranks' [5][Q][k] blocks that carries the components with their row
int linear_max_out(rag_ctx* h, const unsigned long long* max_key, int Q, double* out_dev, hipStream_t st);
int linear_max_reduce(rag_ctx* h, const double* gathered_dev, int world, int Q, unsigned long long* max_key, hipStream_t st);
int linear_merge(rag_ctx* h, const int64_t* blocks, int world, int Q, int k, int64_t* ids_out, double* hyb_out, double* sem_out,
                 double* kw_out, double* tmp_out, hipStream_t st);
int dense_free(rag_ctx* h);
int dense_build_tenant_tiles(rag_ctx* h, const int32_t* tenants_host, int64_t n_rows);
int dense_tenant_tiles_append(rag_ctx* h, const int32_t* tenants_host, int64_t first_row, int64_t n);
int live_vis_rebuild(rag_ctx* h);
int bm25_fresh(rag_ctx* h);            // RAG_ERR_STATE while the postings are stale (inserts / compaction since the last load)
int live_vis_extend(rag_ctx* h, int64_t first_row, int64_t n);
// idmap.hip: the id-to-row map through the writes. A write that may need a larger (or a first) table allocates it with
// idmap_prepare BEFORE it commits anything (RAG_ERR_NOMEM: nothing changed) and hands it to idmap_rebuild afterwards; every
// function is a no-op while the map is disabled.
#define IDMAP_EMPTY ((int64_t)0x8000000000000000ull)     // an unused slot: no key (ids >= 0) equals it
#define IDMAP_STAT_WORDS 8
struct idmap_table { dev_buf<int64_t> keys; dev_buf<int32_t> rows; int64_t slots = 0; };
int64_t idmap_slots_for(int64_t row_capacity);
bool idmap_must_rebuild(const rag_ctx* h, int64_t n_new, int64_t row_capacity_after, bool explicit_after);
int idmap_prepare(rag_ctx* h, int64_t row_capacity, idmap_table* t);
int idmap_rebuild(rag_ctx* h, idmap_table* t);           // from the id plane and vis; t may be null or empty: in place
int idmap_insert_rows(rag_ctx* h, int64_t first_row, int64_t n, bool block_ascending);
int idmap_erase_deleted(rag_ctx* h, const int64_t* set_dev, int n_set);
void idmap_drop(rag_ctx* h);
// rows_out[i] = the live row of ids[i] or -1; owned (may be null) = 1 / 0 as int64. Explicit ids go through the map
// (RAG_ERR_STATE without one), implicit ids through id_base
int idmap_rows_of_ids(rag_ctx* h, const int64_t* ids_dev, int64_t n, int32_t* rows_out, int64_t* owned, hipStream_t st);
// what the entries that merge shards by id ask of an index with explicit ids: the map, and ids that ascend with the rows
int idmap_shard_gate(rag_ctx* h, const char* who, const char* refusal_without_map);
// postings through a compaction (rag_index_compact_bm25): built beside the resident ones from the device row map before any
// row moves, swapped in (or dropped) afterwards
// (ix / slot: the BM25 postings rag_ctx::bm25 or the learned-sparse postings rag_ctx::sparse)
int64_t bm25_base_docs(const rag_bm25_index* ix);
int64_t bm25_covered_docs(const rag_bm25_index* ix);
int bm25_compact_prepare(rag_ctx* h, const rag_bm25_index* ix, const int64_t* row_map_dev, int64_t base_live, int64_t covered_live,
                         rag_bm25_index** out);
void bm25_compact_commit(rag_bm25_index** slot, rag_bm25_index* nb);
void bm25_compact_discard(rag_bm25_index* nb);
int merge_topk(rag_ctx* h, const int64_t* ids, const double* scores, int n_lists, int64_t list_stride, int Q, int k,
               int64_t* ids_out, double* scores_out, hipStream_t st, int normalize = 0);
int pairwise_cosine(rag_ctx* h, const float* a_dev, int m, const float* b_dev, int n, int dim, double* out_dev,
                    hipStream_t st);
int pairwise_cosine_f64(rag_ctx* h, const double* a_dev, int m, const double* b_dev, int n, int dim, double* out_dev, hipStream_t st);
// fusion.hip
int rrf_fuse_host(rag_ctx* h, const int64_t* lists, int Q, int L, int len, int rrf_k, int top_k, int64_t* keys_out, double* scores_out,
                  int32_t* ranks_out);
int rrf_fuse_dev(rag_ctx* h, const int64_t* lists_dev, int Q, int L, int len, int64_t list_stride, int64_t query_stride, int rrf_k, int top_k,
                 int64_t* keys_dev, double* scores_dev, int32_t* ranks_dev, hipStream_t st);
int linear_fuse_topk_host(rag_ctx* h, const double* sem, const double* kw, const double* tmp, int n, double a, double b, double g, int top_k,
                          int32_t* idx_out, double* hyb_out);
// bm25.hip: the BM25 postings (h->bm25) ...
int bm25_load_host(rag_ctx* h, const int64_t* indptr, const int32_t* doc, const int32_t* tf, const int32_t* doc_len, const double* idf,
                   int64_t n_docs, int64_t n_terms, double avgdl, double k1, double b);
int bm25_append_host(rag_ctx* h, const int64_t* indptr, const int32_t* doc, const int32_t* tf, const int32_t* doc_len, const double* idf_new,
                     int64_t n_new, int64_t n_terms_total);
int bm25_fold(rag_ctx* h);
void bm25_free(rag_ctx* h);
int64_t bm25_n_docs(const rag_ctx* h);          // -1 without postings
int bm25_live_counts_host(rag_ctx* h, int32_t* df_out, int64_t* n_docs_live_out, int64_t* sum_doc_len_out);
int bm25_set_statistics_host(rag_ctx* h, const double* idf, double avgdl);
int bm25_refresh(rag_ctx* h, double epsilon, double* idf_out, rag_bm25_refresh_info* info_out);
int bm25_segment_stats(rag_ctx* h, rag_bm25_segments* out);
int bm25_index_bytes(const int64_t* indptr, int64_t n_docs, int64_t n_terms, int64_t* postings_out, int64_t* meta_out, int64_t* table_out);
int bm25_grid_plan(int n_ranges_in_launch, int n_queries, int linear, int64_t* out5);
int bm25_set_normalize(rag_ctx* h, int on);
int bm25_negative_bound_args(const rag_ctx* h, double* per_token_out);
int bm25_topk_host(rag_ctx* h, const int32_t* term_ptr, const int32_t* terms, int Q, int k, int tenant, int64_t* ids_out, int32_t* rows_out,
                   double* scores_out, double* raw_max_out, query_tenants qt);
// ids: what ids_dev reports for postings that cover exactly the index's rows; any other postings report row numbers
int bm25_topk_dev(rag_ctx* h, const int32_t* term_ptr_dev, const int32_t* terms_dev, int Q, int k, int tenant, int64_t* ids_dev, int32_t* rows_dev,
                  double* scores_dev, double* raw_max_dev, hipStream_t st, id_space ids, query_tenants qt);
int bm25_scores_host(rag_ctx* h, const int32_t* term_ptr, const int32_t* terms, int Q, double* out);
int bm25_scores_dev(rag_ctx* h, const int32_t* term_ptr_dev, const int32_t* terms_dev, int Q, double* out_dev, hipStream_t st, float* raw32_dev,
                    int64_t ld, unsigned long long* max_key_dev, int tenant, query_tenants qt);
int bm25_scores_adhoc_host(rag_ctx* h, const int64_t* indptr, const int32_t* doc, const int32_t* tf, const int32_t* doc_len, const double* idf,
                           int64_t n_docs, int64_t n_terms, double avgdl, double k1, double b, const int32_t* term_ptr, const int32_t* terms, int Q,
                           double* out);
// ... and the learned-sparse postings (h->sparse)
int sparse_load_host(rag_ctx* h, const int64_t* indptr, const int32_t* doc, const float* weight, int64_t n_docs, int64_t n_terms);
int sparse_append_host(rag_ctx* h, const int64_t* indptr, const int32_t* doc, const float* weight, int64_t n_new, int64_t n_terms_total);
int sparse_append_docs_dev(rag_ctx* h, const int32_t* doc_ptr, const int32_t* terms, const float* weights, int64_t n, int64_t nnz_cap,
                           int64_t n_terms_total);
int sparse_append_docs_host(rag_ctx* h, const int32_t* doc_ptr, const int32_t* terms, const float* weights, int64_t n, int64_t nnz_cap,
                            int64_t n_terms_total);
int sparse_clear(rag_ctx* h);
int sparse_export_host(rag_ctx* h, int64_t* indptr_out, int32_t* doc_out, float* weight_out, int64_t* n_docs_out, int64_t* n_terms_out,
                       int64_t* nnz_out);
int sparse_fold(rag_ctx* h);
void sparse_free(rag_ctx* h);
int sparse_info(const rag_ctx* h, int64_t* n_docs_out, int64_t* n_terms_out, int64_t* nnz_out, int64_t* hbm_bytes_out);
int sparse_segment_stats(rag_ctx* h, rag_bm25_segments* out);
int sparse_topk_host(rag_ctx* h, const int32_t* term_ptr, const int32_t* terms, const float* qweights, int Q, int k, int tenant, int64_t* ids_out,
                     int32_t* rows_out, double* scores_out, query_tenants qt);
int sparse_topk_dev(rag_ctx* h, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev, int Q, int k, int tenant,
                    int64_t* ids_dev, int32_t* rows_dev, double* scores_dev, hipStream_t st, id_space ids, query_tenants qt);
int sparse_scores_host(rag_ctx* h, const int32_t* term_ptr, const int32_t* terms, const float* qweights, int Q, double* out);
// The ONE precondition of a search that fuses keyword postings (sparse: h->sparse, else h->bm25) with the dense index by row: they are
// loaded, fresh (RAG_ERR_STATE while stale) and hold as many documents as the index has rows (RAG_ERR_ARG, "<who>: the ... postings
// must be row-aligned with the index" + note). Missing postings return missing_code, which differs by entry and is kept as it was:
//   RAG_ERR_ARG   "bad argument: no sparse index loaded (rag_sparse_load_host)"   rag_hybrid_sparse_rrf_dev, rag_retrieve_maxsim_dev
//   RAG_ERR_STATE "<who>: no sparse index loaded (rag_sparse_load_host)"          rag_m3_score_rows_dev, rag_retrieve_m3_dev
//   RAG_OK        (no message of their own: reported as not row-aligned)          rag_hybrid_rrf*_dev, rag_retrieve_rerank*_dev
int keyword_postings_aligned(rag_ctx* h, bool sparse, const char* who, int missing_code, const char* note = " (same number of documents)");
// mmr.hip, chunk_chain.hip
int mmr_select_dev(rag_ctx* h, const float* queries_dev, const float* emb_dev, const int32_t* rows_dev, int Q, int n, int dim, int top_k, double lam,
                   int variant, int32_t* sel_dev, double* score_dev, hipStream_t st);
int mmr_select_host(rag_ctx* h, const float* query, const float* emb, int n, int dim, int top_k, double lam, int variant, int32_t* sel_out,
                    double* score_out);
int chunk_chain_host(rag_ctx* h, const float* emb, const int32_t* sent_len, int n, int dim, double threshold, int max_chunk, int min_chunk,
                     int32_t* group_out);
// pipeline.hip: the passage token store, the pair builder and the sigmoid top-k on their own, and the resident composites
int tokens_load_host(rag_ctx* h, const int32_t* tokens, const int32_t* lens, int64_t n_rows, int L, int id_bits);
int tokens_reserve(rag_ctx* h, int64_t n_rows, int L, int id_bits);
int tokens_info(const rag_ctx* h, int64_t* rows_out, int* L_out, int* id_bits_out);
int tokens_append_dev(rag_ctx* h, const int32_t* tokens_dev, const int32_t* lens_dev, int64_t n_rows, hipStream_t st);
int ce_build_pairs_dev(rag_ctx* h, const int32_t* q_tok_dev, const int32_t* q_len_dev, int Lq, const int64_t* cand_dev, int Q, int pool,
                       int64_t token_id_base, int L_pair, int cls_id, int sep_id, int32_t* ids_out, int32_t* tt_out, int32_t* lens_out,
                       hipStream_t st);
int rerank_topk_dev(rag_ctx* h, const float* logits_dev, const int64_t* cand_dev, int Q, int pool, int k, int64_t* ids_out, double* scores_out,
                    float* logits_out, hipStream_t st);
int retrieve_rerank_dev(rag_ctx* h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev, const int32_t* q_tok_dev,
                        const int32_t* q_len_dev, int Lq, int Q, int pool, int k, int rrf_k, int tenant, int mode, int cls_id, int sep_id, int L_pair,
                        int64_t* ids_out, double* scores_out, float* logits_out, int64_t* cand_out, hipStream_t st, query_tenants qt);
int retrieve_maxsim_dev(rag_ctx* h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev,
                        const float* q_vecs_dev, const int64_t* q_off_dev, int Q, int pool, int k, int rrf_k, int tenant, int mode, int64_t* ids_out,
                        double* scores_out, int64_t* cand_out, hipStream_t st, query_tenants qt);
// cross_encoder.hip: the cross-encoder (h->ce) and the sentence-embedding encoder (h->emb). ids / tt / lens / out are host
// arrays (staged, the call waits) or device arrays (queued on st) as host_ptrs says.
int ce_load_host(rag_ctx* h, const rag_ce_config* cfg, const float* const* tensors, int n);
int ce_score(rag_ctx* h, const int32_t* ids, const int32_t* tt, const int32_t* lens, int P, int L, float* out, hipStream_t st,
             bool host_ptrs);
void ce_free(rag_ctx* h);
int ce_length_class(int d_head, int seq_len);
int ce_model_seq_limit(const rag_ctx* h, int which);
int embed_load_host(rag_ctx* h, const rag_ce_config* cfg, const float* const* tensors, int n, int flags);
int embed_run(rag_ctx* h, const int32_t* ids, const int32_t* tt, const int32_t* lens, int P, int L, float* out, hipStream_t st,
              bool host_ptrs);
int embed_dim(const rag_ctx* h);
int embed_tok_dim(const rag_ctx* h);     // width of the loaded token-vector head, 0 without one, -1 without an embedder
// the embedder's optional token-vector and lexical heads, and one forward with up to three outputs (cross_encoder.hip)
int embed_heads_load_host(rag_ctx* h, const float* tok_w, const float* tok_b, int tok_dim, const float* lex_w, float lex_b);
int embed_multi_host(rag_ctx* h, const int32_t* ids, const int32_t* tt, const int32_t* lens, int P, int L, float* dense, float* lex, float* tok,
                     int64_t tok_rows_cap, int64_t* row_off);
int embed_multi_dev(rag_ctx* h, const int32_t* ids, const int32_t* tt, const int32_t* lens, int P, int L, float* dense, float* lex, float* tok,
                    int64_t tok_rows_cap, int64_t* row_off, hipStream_t st);
// m3_heads.hip: pair scores over the heads' outputs
int maxsim_host(rag_ctx* h, const float* q, const int64_t* q_off, int n_q, const float* d, const int64_t* d_off, int n_d, const int32_t* pair_q,
                const int32_t* pair_d, int n_pairs, int dim, float* out);
int maxsim_dev(rag_ctx* h, const float* q, const int64_t* q_off, int n_q, const float* d, const int64_t* d_off, int n_d, const int32_t* pair_q,
               const int32_t* pair_d, int n_pairs, int dim, float* out, hipStream_t st);
int lexical_match_host(rag_ctx* h, const int32_t* q_ids, const float* q_w, const int32_t* q_lens, int n_q, int Lq, const int32_t* d_ids,
                       const float* d_w, const int32_t* d_lens, int n_d, int Ld, const int32_t* pair_q, const int32_t* pair_d, int n_pairs,
                       const int32_t* skip_ids, int n_skip, float* out);
int lexical_match_dev(rag_ctx* h, const int32_t* q_ids, const float* q_w, const int32_t* q_lens, int n_q, int Lq, const int32_t* d_ids,
                      const float* d_w, const int32_t* d_lens, int n_d, int Ld, const int32_t* pair_q, const int32_t* pair_d, int n_pairs,
                      const int32_t* skip_ids_host, int n_skip, float* out, hipStream_t st);
// ... and a text's per-position lexical weights reduced to its sorted sparse vector (rag_lexical_compact_*)
int lexical_compact_host(rag_ctx* h, const int32_t* ids, const float* w, const int32_t* lens, int n, int L, const int32_t* skip_ids, int n_skip,
                         int32_t* term_ptr_out, int32_t* terms_out, float* qw_out, int64_t cap);
int lexical_compact_dev(rag_ctx* h, const int32_t* ids, const float* w, const int32_t* lens, int n, int L, const int32_t* skip_ids_host, int n_skip,
                        int32_t* term_ptr_out, int32_t* terms_out, float* qw_out, int64_t cap, hipStream_t st);
// tokvec.hip: the resident token-vector store and MaxSim rerank over it. tokvec_rerank checks the store and its arguments, scores
// [Q][pool] slots and selects through tokvec_topk (pipeline.hip: the kernel behind rag_rerank_topk_dev, without the sigmoid).
int tokvec_reserve(rag_ctx* h, int64_t n_docs_total, int64_t rows_total, int dim, int form);
int tokvec_append(rag_ctx* h, const float* vecs, const int64_t* row_off, int64_t n_docs, hipStream_t st, bool host_ptrs);
int tokvec_load_host(rag_ctx* h, const float* vecs, const int64_t* off, int64_t n_docs, int dim, int form);
int tokvec_info(const rag_ctx* h, int64_t* docs_out, int64_t* rows_out, int* dim_out, int64_t* hbm_bytes_out);
int tokvec_form(const rag_ctx* h, int* form_out);             // RAG_TOKVEC_*, -1 without a store
int tokvec_fetch_host(rag_ctx* h, int64_t doc, float* out, int64_t cap_rows, int64_t* n_rows_out);
// the store through a compaction (rag_index_compact_live): everything allocated by tokvec_compact_prepare before a row of any
// plane moves; tokvec_compact_commit moves the rows in place through the compaction's staging buffer and swaps the offsets in
struct tokvec_compact_plan {
    dev_buf<int64_t> new_off;                // the store's offsets after the move [tv_docs_cap + 1]
    dev_buf<int64_t> src_start;              // [new documents] first OLD row of each surviving document
    std::vector<int64_t> new_off_h;          // host copy of new_off[0 .. docs_new]
    int64_t docs_new = 0, rows_new = 0, first_doc = 0, chunk_rows = 0;
    bool active = false;
};
int tokvec_compact_prepare(rag_ctx* h, const int64_t* row_map_host, int64_t n_map, size_t stage_bytes, tokvec_compact_plan* plan);
int tokvec_compact_commit(rag_ctx* h, tokvec_compact_plan* plan, char* stage, hipStream_t st);
int tokvec_usable(rag_ctx* h, const char* who);          // RAG_ERR_STATE without a store or with a stale one
int tokvec_covers_index(rag_ctx* h, const char* who);    // (after tokvec_usable) RAG_ERR_STATE unless the store holds exactly the index's rows
int tokvec_rerank(rag_ctx* h, const float* q_vecs, const int64_t* q_off, const int32_t* cand_rows, int Q, int pool, int k, int64_t* ids_out,
                  int32_t* rows_out, double* scores_out, float* pair_scores_out, hipStream_t st);
int tokvec_rerank_host(rag_ctx* h, const float* q_vecs, const int64_t* q_off, const int32_t* cand_rows, int Q, int pool, int k, int64_t* ids_out,
                       int32_t* rows_out, double* scores_out, float* pair_scores_out);
// every visible document of the store against every query: rows_out [Q][pool] int32 = each query's top-pool rows in rank order
// (score desc, row asc), -1 padded. plane = [tokvec_scan_batch(h, Q)][tv_docs] uint32 of the caller's workspace: the keys of one
// sub-batch of queries. The caller has checked the store, the index and the shape (retrieve_maxsim_dev, mode 2).
int tokvec_scan_batch(const rag_ctx* h, int Q);
int tokvec_scan(rag_ctx* h, const float* q_vecs, const int64_t* q_off, int Q, int pool, int tenant, query_tenants qt, uint32_t* plane,
                int32_t* rows_out, hipStream_t st);
int tokvec_topk(rag_ctx* h, const float* scores_dev, const int32_t* slot_rows_dev, int Q, int pool, int k, int64_t* ids_out, int32_t* rows_out,
                double* scores_out, hipStream_t st);
int tokvec_score_slots(rag_ctx* h, const float* q_vecs, const int64_t* q_off, const int32_t* cand_rows, int Q, int pool, const float** scores_out,
                       const int32_t** slots_out, hipStream_t st);
// the three-way bge-m3 score over resident data (pipeline.hip; rag_m3_score_rows_dev, rag_retrieve_m3_dev) and its components:
// the float64 cosine of given rows (dense.hip) and the learned-sparse point lookup (bm25.hip)
int dense_cosine_rows(rag_ctx* h, const float* q_dev, const int32_t* cand_rows_dev, int Q, int pool, double* out_dev, hipStream_t st);
int sparse_score_rows_dev(rag_ctx* h, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev,
                          const int32_t* cand_rows_dev, int Q, int pool, double* scores_dev, hipStream_t st);
int sparse_score_rows_host(rag_ctx* h, const int32_t* term_ptr, const int32_t* terms, const float* qweights, const int32_t* cand_rows, int Q,
                           int pool, double* scores_out);
int m3_score_rows_dev(rag_ctx* h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev,
                      const float* q_vecs_dev, const int64_t* q_off_dev, const int32_t* cand_rows_dev, int Q, int pool, int k, double w_dense,
                      double w_sparse, double w_colbert, int64_t* ids_out, int32_t* rows_out, double* scores_out, double* components_out,
                      hipStream_t st);
int retrieve_m3_dev(rag_ctx* h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev,
                    const float* q_vecs_dev, const int64_t* q_off_dev, int Q, int pool, int k, int rrf_k, int tenant, int mode, double w_dense,
                    double w_sparse, double w_colbert, int64_t* ids_out, double* scores_out, double* components_out, int64_t* cand_out,
                    hipStream_t st, query_tenants qt);
// the row-sharded form of retrieve_m3_dev, the halves on each side of its two all-gathers (rag_m3_candidates_gathered_dev,
// rag_m3_score_ids_dev, rag_m3_combine_gathered_dev): candidates from every rank's lists, the components of the slots this handle's
// rows own, combine + select over every rank's components. The two gathered ones need no index.
int m3_candidates_gathered_dev(rag_ctx* h, const int64_t* gathered_dev, int world, int Q, int pool, int rrf_k, int mode, int64_t* lists_out,
                               double* scores_out, int64_t* cand_out, hipStream_t st);
int m3_score_ids_dev(rag_ctx* h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev,
                     const float* q_vecs_dev, const int64_t* q_off_dev, const int64_t* cand_ids_dev, int Q, int slots, double w_dense,
                     double w_sparse, double w_colbert, int64_t* partial_out, hipStream_t st);
int m3_combine_gathered_dev(rag_ctx* h, const int64_t* cand_ids_dev, const int64_t* gathered_dev, int world, int Q, int slots, int k,
                            double w_dense, double w_sparse, double w_colbert, int64_t* ids_out, double* scores_out, double* components_out,
                            hipStream_t st);
// token ids -> the forward (h->emb), the compaction of its lexical weights, retrieve_m3_dev: rag_search_m3_tokens(_tenants)_dev
int search_m3_tokens_dev(rag_ctx* h, const int32_t* input_ids_dev, const int32_t* token_type_ids_dev, const int32_t* lens_dev, int Q, int L,
                         const int32_t* skip_ids_host, int n_skip, int pool, int k, int rrf_k, int tenant, int mode, double w_dense, double w_sparse,
                         double w_colbert, int64_t* ids_out, double* scores_out, double* components_out, int64_t* cand_out, hipStream_t st,
                         query_tenants qt);
