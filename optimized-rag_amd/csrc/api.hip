// C-ABI entry points of librag_hip.so (include/rag_hip.h). Thin: argument checks, host<->device
// staging for the *_host variants, dispatch to the kernels' host drivers.
#include "common.h"

#include <cctype>
#include <cmath>
#include <cstdlib>
#include <cstring>

static thread_local std::string g_null_err = "null handle";

// name -> member of rag_options; the environment default of option <name> is RAG_<NAME>
static const struct { const char* name; int rag_options::*field; } g_options[] = {
    {"force_level", &rag_options::force_level},         {"stage_growth", &rag_options::stage_growth},
    {"no_smallq", &rag_options::no_smallq},             {"no_second_pass", &rag_options::no_second_pass},
    {"dense_linear_order", &rag_options::dense_linear_order}, {"dense_persist", &rag_options::dense_persist},
    {"bm25_first_ranges", &rag_options::bm25_first_ranges}, {"bm25_no_staging", &rag_options::bm25_no_staging},
    {"bm25_packed", &rag_options::bm25_packed},         {"bm25_plan_slots", &rag_options::bm25_plan_slots},       {"bm25_ws_mb", &rag_options::bm25_ws_mb},
    {"bm25_tail_fold", &rag_options::bm25_tail_fold},     {"bm25_keep_tf", &rag_options::bm25_keep_tf},
    {"sparse_tail_fold", &rag_options::sparse_tail_fold}, {"tokvec_compact_rows", &rag_options::tokvec_compact_rows},
    {"tokvec_scan_ws_mb", &rag_options::tokvec_scan_ws_mb}, {"tokvec_scan_queries", &rag_options::tokvec_scan_queries},
    {"bm25_linear_grid", &rag_options::bm25_linear_grid},            {"bm25_sort_merge", &rag_options::bm25_sort_merge},
    {"no_fork", &rag_options::no_fork},                 {"fork_max_q", &rag_options::fork_max_q},
    {"ce_chunk_tokens", &rag_options::ce_chunk_tokens}, {"ce_mx", &rag_options::ce_mx},
    {"ce_attn_stream", &rag_options::ce_attn_stream},   {"ce_ffn_fused", &rag_options::ce_ffn_fused},
};
static void options_from_env(rag_options* o) {
    for (const auto& e : g_options) {
        std::string env = "RAG_";
        for (const char* c = e.name; *c; ++c) env += (char)toupper(*c);
        if (const char* v = getenv(env.c_str())) o->*(e.field) = atoi(v);
    }
}
// first statement after the lock and the argument checks of an entry that touches the device (common.h host_after_dev)
#define DEV_ENTRY(h)                                                                           \
    do {                                                                                      \
        HIP_TRY(h, hipSetDevice((h)->device));                                                \
        (h)->dev_pending = true;                                                              \
    } while (0)
#define HOST_ENTRY(h)                                                                          \
    do {                                                                                      \
        HIP_TRY(h, hipSetDevice((h)->device));                                                \
        if (int rc_ = host_after_dev(h)) return rc_;                                          \
    } while (0)

// ---- per-query tenants (rag_*_tenants_*). The scalar entry and its namesake share one body: tenants_host == nullptr is the
// scalar call. A UNIFORM array (every query the same tenant, or none filtered) is the scalar call with that tenant too, so the
// per-query kernels' path only runs where tenants really differ. Otherwise the array is copied to the device on the call's
// stream first - consumed before the entry returns, ordered like everything else the call queues.
struct entry_tenants { int tenant; query_tenants qt; };
static int entry_tenants_of(rag_ctx* h, int tenant, const int32_t* tenants_host, int Q, hipStream_t st, entry_tenants* out) {
    *out = {tenant, {nullptr, nullptr}};
    if (tenants_host == nullptr) return RAG_OK;
    const int32_t t0 = std::max(tenants_host[0], -1);
    bool uniform = true;
    for (int q = 1; q < Q && uniform; ++q) uniform = std::max(tenants_host[q], -1) == t0;
    out->tenant = t0;
    return uniform ? RAG_OK : stage_query_tenants(h, tenants_host, Q, st, &out->qt);
}

template <class T>
static int pairwise_cosine_host_t(rag_handle_t h, const T* a, int m, const T* b, int n, int dim, double* out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, m >= 0 && n >= 0 && dim > 0, "bad sizes");
    if (m == 0 || n == 0) return RAG_OK;
    ARG_CHECK(h, a && b && out, "null pointer");
    HOST_ENTRY(h);
    const bool same = (a == b && m == n);
    hipStream_t st = h->stream;
    int rc = stage_reserve(h, stage_size((size_t)m * dim, sizeof(T)) + stage_size(same ? 0 : (size_t)n * dim, sizeof(T)) + stage_size((size_t)m * n, 8));
    if (rc) return rc;
    char* p = h->stage;
    T* ad = stage_take<T>(p, (size_t)m * dim);
    T* bd = same ? ad : stage_take<T>(p, (size_t)n * dim);
    double* od = stage_take<double>(p, (size_t)m * n);
    HIP_TRY(h, hipMemcpyAsync(ad, a, (size_t)m * dim * sizeof(T), hipMemcpyHostToDevice, st));
    if (!same) HIP_TRY(h, hipMemcpyAsync(bd, b, (size_t)n * dim * sizeof(T), hipMemcpyHostToDevice, st));
    if constexpr (sizeof(T) == 8) rc = pairwise_cosine_f64(h, ad, m, bd, n, dim, od, st);
    else rc = pairwise_cosine(h, ad, m, bd, n, dim, od, st);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(out, od, (size_t)m * n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return RAG_OK;
}

extern "C" {

int rag_version(void) { return 200; }

int rag_device_count(int* n_out) {
    if (!n_out) return RAG_ERR_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        *n_out = 0;
        return RAG_ERR_HIP;
    }
    *n_out = n;
    return RAG_OK;
}

int rag_create(int device_id, int dim, rag_handle_t* out) {
    if (!out || dim <= 0 || dim % 4 != 0) return RAG_ERR_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0 || device_id < 0 || device_id >= n) return RAG_ERR_HIP;
    if (hipSetDevice(device_id) != hipSuccess) return RAG_ERR_HIP;
    rag_ctx* h = new rag_ctx();
    h->device = device_id;
    h->dim = dim;
    h->dim_pad = (int)round_up(dim, RAG_BK);
    options_from_env(&h->opt);
    if (hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, device_id) != hipSuccess || h->n_cu <= 0) h->n_cu = 256;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return RAG_ERR_HIP;
    }
    *out = h;
    return RAG_OK;
}

int rag_destroy(rag_handle_t h) {
    if (!h) return RAG_ERR_ARG;
    { LOCK(h); }                        // wait for a call in flight on another thread; the caller must not start new ones
    hipSetDevice(h->device);
    hipStreamSynchronize(h->stream);
    comm_free(h);
    dense_free(h);
    bm25_free(h);
    sparse_free(h);
    ce_free(h);
    static_cast<rag_device_mem&>(*h) = rag_device_mem();      // every device buffer the handle itself owns
    for (auto& p : h->prof)
        for (auto& e : p.ev) {
            hipEventDestroy(e.first);
            hipEventDestroy(e.second);
        }
    if (h->side_stream) { hipStreamSynchronize(h->side_stream); hipStreamDestroy(h->side_stream); hipEventDestroy(h->ev_fork); hipEventDestroy(h->ev_join); }
    hipStreamDestroy(h->stream);
    delete h;
    return RAG_OK;
}

const char* rag_last_error(rag_handle_t h) { return h ? h->err.c_str() : g_null_err.c_str(); }

int rag_synchronize(rag_handle_t h) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RAG_OK;
}

int rag_set_option(rag_handle_t h, const char* name, int value) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, name != nullptr, "set_option: null name");
    for (const auto& e : g_options)
        if (strcmp(e.name, name) == 0) {
            h->opt.*(e.field) = value;
            return RAG_OK;
        }
    h->err = std::string("bad argument: unknown option ") + name;
    return RAG_ERR_ARG;
}

int rag_set_profiling(rag_handle_t h, int enable) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    h->profiling = enable != 0;
    for (auto& p : h->prof) p.used = 0;      // (re)start collecting spans
    return RAG_OK;
}

// ---- dense index ---------------------------------------------------------------------------------
static int index_load_common(rag_ctx* h, const float* emb, const int64_t* ids, int64_t id_base, int64_t n_rows,
                             hipStream_t st, bool host) {
    ARG_CHECK(h, n_rows >= 0 && n_rows < (int64_t)0x7fffff00, "n_rows must fit int32 per GPU");
    ARG_CHECK(h, n_rows == 0 || emb != nullptr, "emb is null");
    if (host) HOST_ENTRY(h);
    else DEV_ENTRY(h);
    h->lin_begun.on = false;            // (the device-pointer load is a write too)
    dense_free(h);
    h->n_rows = n_rows;
    h->id_base = id_base;
    const hipMemcpyKind kind = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    if (n_rows > 0) {
        if (int rc = h->emb32.alloc(h, (size_t)n_rows * h->dim)) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->emb32, emb, (size_t)n_rows * h->dim * sizeof(float), kind, st));
        if (ids) {
            if (int rc = h->ids.alloc(h, (size_t)n_rows)) return rc;
            HIP_TRY(h, hipMemcpyAsync(h->ids, ids, (size_t)n_rows * sizeof(int64_t), kind, st));
        }
    }
    int rc = dense_index_build(h, h->emb32, n_rows, st);
    if (rc) return rc;
    h->index_loaded = true;
    if (host) HIP_TRY(h, hipStreamSynchronize(st));
    return RAG_OK;
}

int rag_index_load_host(rag_handle_t h, const float* emb_host, const int64_t* ids_host, int64_t id_base, int64_t n_rows) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    return index_load_common(h, emb_host, ids_host, id_base, n_rows, h->stream, true);
}

int rag_index_load_dev(rag_handle_t h, const float* emb_dev, const int64_t* ids_dev, int64_t id_base, int64_t n_rows,
                       void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    return index_load_common(h, emb_dev, ids_dev, id_base, n_rows, (hipStream_t)stream, false);
}

// ---- chunked bulk load (export of document_chunks / archival_memory in pieces) -------------------
int rag_index_reserve(rag_handle_t h, int64_t n_rows_total, int64_t id_base) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, n_rows_total > 0 && n_rows_total < (int64_t)0x7fffff00, "n_rows must fit int32 per GPU");
    HOST_ENTRY(h);
    dense_free(h);
    h->id_base = id_base;
    h->n_reserved = n_rows_total;
    const int64_t pad = round_up(n_rows_total, (int64_t)RAG_TILE * 8);
    int rc;
    if ((rc = h->emb32.alloc(h, (size_t)n_rows_total * h->dim))) return rc;
    if ((rc = h->emb16.alloc(h, (size_t)pad * h->dim_pad))) return rc;
    if ((rc = h->bad_rows.alloc(h, 1))) return rc;
    HIP_TRY(h, hipMemsetAsync(h->bad_rows, 0, sizeof(int), h->stream));
    // rows not appended yet (and the tile padding) must read as zero vectors
    HIP_TRY(h, hipMemsetAsync(h->emb16, 0, (size_t)pad * h->dim_pad * sizeof(half_t), h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->index_loaded = true;
    return RAG_OK;
}

static int index_append(rag_ctx* h, const float* emb, int64_t n, hipStream_t st, bool host) {
    ARG_CHECK(h, h->n_reserved > 0, "rag_index_reserve first");
    ARG_CHECK(h, n >= 0 && h->n_rows + n <= h->n_reserved, "append exceeds the reserved row count");
    ARG_CHECK(h, n == 0 || emb != nullptr, "emb is null");
    if (host) HOST_ENTRY(h);
    else DEV_ENTRY(h);
    h->lin_begun.on = false;
    if (n == 0) return RAG_OK;
    HIP_TRY(h, hipMemcpyAsync(h->emb32 + (size_t)h->n_rows * h->dim, emb, (size_t)n * h->dim * sizeof(float),
                              host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    int rc = dense_index_normalize_range(h, h->n_rows, n, st);
    if (rc) return rc;
    if (h->vis && (rc = live_vis_extend(h, h->n_rows, n))) return rc;      // appended rows are live
    h->n_rows += n;
    if (host) HIP_TRY(h, hipStreamSynchronize(st));
    return RAG_OK;
}

int rag_index_append_host(rag_handle_t h, const float* emb_host, int64_t n_rows) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    return index_append(h, emb_host, n_rows, h->stream, true);
}

int rag_index_append_dev(rag_handle_t h, const float* emb_dev, int64_t n_rows, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    return index_append(h, emb_dev, n_rows, (hipStream_t)stream, false);
}

int rag_index_set_tenants_host(rag_handle_t h, const int32_t* t, int64_t n_rows) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, t == nullptr || n_rows == h->n_rows, "tenant array length must equal the index row count");
    HOST_ENTRY(h);
    h->tenants.reset();
    int rc;
    if (t == nullptr || n_rows == 0) {                     // NULL clears the filter table
        if ((rc = dense_build_tenant_tiles(h, nullptr, 0))) return rc;
        return live_vis_rebuild(h);                        // deleted rows stay deleted
    }
    if ((rc = h->tenants.alloc(h, (size_t)n_rows))) return rc;
    HIP_TRY(h, hipMemcpy(h->tenants, t, (size_t)n_rows * sizeof(int32_t), hipMemcpyHostToDevice));
    if ((rc = dense_build_tenant_tiles(h, t, n_rows))) return rc;
    return live_vis_rebuild(h);
}

int rag_index_set_ids_host(rag_handle_t h, const int64_t* ids, int64_t n_rows) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, n_rows == h->n_rows, "id array length must equal the index row count");
    HOST_ENTRY(h);
    const bool stored = ids != nullptr && n_rows > 0;
    idmap_table map;                    // an enabled id map is rebuilt from the new column: its table before anything changes
    if (stored && idmap_must_rebuild(h, 0, std::max(emb32_rows(h), n_rows), true))
        if (int rc = idmap_prepare(h, std::max(emb32_rows(h), n_rows), &map)) return rc;
    h->ids.reset();
    if (stored) {
        int rc = h->ids.alloc(h, (size_t)n_rows);
        if (rc == RAG_OK && hipMemcpy(h->ids, ids, (size_t)n_rows * sizeof(int64_t), hipMemcpyHostToDevice) != hipSuccess) {
            h->err = "set_ids: the copy of the id column failed";
            rc = RAG_ERR_HIP;
        }
        if (rc) {                       // the id column is gone or undefined: a map of the old one must not outlive it
            h->ids.reset();
            idmap_drop(h);
            return rc;
        }
    }
    return idmap_rebuild(h, &map);
}

int rag_index_rows(rag_handle_t h, int64_t* n_rows_out) {
    if (!h || !n_rows_out) return RAG_ERR_ARG;
    LOCK(h);
    *n_rows_out = h->n_rows;
    return RAG_OK;
}

int rag_index_fetch_rows_host(rag_handle_t h, const int64_t* rows, int n, float* out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, n >= 0 && (n == 0 || (rows && out)), "null rows/out");
    HOST_ENTRY(h);
    for (int i = 0; i < n; ++i) {
        ARG_CHECK(h, rows[i] >= 0 && rows[i] < h->n_rows, "row out of range");
        HIP_TRY(h, hipMemcpyAsync(out + (size_t)i * h->dim, h->emb32 + (size_t)rows[i] * h->dim, h->dim * sizeof(float),
                                  hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RAG_OK;
}

// ---- dense search ----------------------------------------------------------------------------------
static int dense_topk_dev_entry(rag_handle_t h, const float* q_dev, int Q, int k, int tenant, const int32_t* tenants_host, int64_t* ids_dev,
                                int32_t* rows_dev, double* scores_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, q_dev && ids_dev && scores_dev, "null pointer");
    ARG_CHECK(h, aligned16(q_dev), "dense_topk: the queries (q_dev) must be 16-byte aligned");
    ARG_CHECK(h, Q > 0 && Q <= 65535, "1 <= n_queries <= 65535");
    DEV_ENTRY(h);
    entry_tenants t;
    if (int rc = entry_tenants_of(h, tenant, tenants_host, Q, (hipStream_t)stream, &t)) return rc;
    return dense_search(h, q_dev, Q, k, t.tenant, ids_dev, rows_dev, scores_dev, (hipStream_t)stream, id_space::of_index(h), t.qt);
}
int rag_dense_topk_dev(rag_handle_t h, const float* q_dev, int Q, int k, int tenant, int64_t* ids_dev, int32_t* rows_dev,
                       double* scores_dev, void* stream) {
    return dense_topk_dev_entry(h, q_dev, Q, k, tenant, nullptr, ids_dev, rows_dev, scores_dev, stream);
}
int rag_dense_topk_tenants_dev(rag_handle_t h, const float* q_dev, int Q, int k, const int32_t* tenants_host, int64_t* ids_dev,
                               int32_t* rows_dev, double* scores_dev, void* stream) {
    if (h && !tenants_host) { LOCK(h); ARG_CHECK(h, false, "null tenants array"); }
    return dense_topk_dev_entry(h, q_dev, Q, k, -1, tenants_host, ids_dev, rows_dev, scores_dev, stream);
}

static int dense_topk_host_entry(rag_handle_t h, const float* q_host, int Q, int k, int tenant, const int32_t* tenants_host, int64_t* ids_out,
                                 int32_t* rows_out, double* scores_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, q_host && ids_out && scores_out, "null pointer");
    ARG_CHECK(h, Q > 0 && Q <= 65535, "1 <= n_queries <= 65535");
    ARG_CHECK(h, k > 0 && k <= RAG_MAX_K, "0 < k <= 256");
    HOST_ENTRY(h);
    hipStream_t st = h->stream;
    const size_t n_out = (size_t)Q * k;
    int rc = stage_reserve(h, stage_size((size_t)Q * h->dim, 4) + 2 * stage_size(n_out, 8) + stage_size(n_out, 4));
    if (rc) return rc;
    char* p = h->stage;
    float* qd = stage_take<float>(p, (size_t)Q * h->dim);
    int64_t* ids_d = stage_take<int64_t>(p, n_out);
    double* sc_d = stage_take<double>(p, n_out);
    int32_t* rows_d = stage_take<int32_t>(p, n_out);
    entry_tenants t;
    if ((rc = entry_tenants_of(h, tenant, tenants_host, Q, st, &t))) return rc;
    HIP_TRY(h, hipMemcpyAsync(qd, q_host, (size_t)Q * h->dim * sizeof(float), hipMemcpyHostToDevice, st));
    rc = dense_search(h, qd, Q, k, t.tenant, ids_d, rows_d, sc_d, st, id_space::of_index(h), t.qt);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(ids_out, ids_d, n_out * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (rows_out) HIP_TRY(h, hipMemcpyAsync(rows_out, rows_d, n_out * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(scores_out, sc_d, n_out * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return RAG_OK;
}
int rag_dense_topk_host(rag_handle_t h, const float* q_host, int Q, int k, int tenant, int64_t* ids_out, int32_t* rows_out,
                        double* scores_out) {
    return dense_topk_host_entry(h, q_host, Q, k, tenant, nullptr, ids_out, rows_out, scores_out);
}
int rag_dense_topk_tenants_host(rag_handle_t h, const float* q_host, int Q, int k, const int32_t* tenants_host, int64_t* ids_out,
                                int32_t* rows_out, double* scores_out) {
    if (h && !tenants_host) { LOCK(h); ARG_CHECK(h, false, "null tenants array"); }
    return dense_topk_host_entry(h, q_host, Q, k, -1, tenants_host, ids_out, rows_out, scores_out);
}

int rag_dense_last_stats(rag_handle_t h, rag_dense_stats* out) {
    if (!h || !out) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, h->last_stats_valid && h->stats, "no dense search has run");
    int s[8];
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(s, h->stats, sizeof(s), hipMemcpyDeviceToHost));
    out->n_queries = h->last_q;
    out->proven_fast = s[0];
    out->proven_wide = s[1];
    out->exact_scan = s[2];
    out->overflowed = s[4];
    out->shortlist = h->last_shortlist;
    out->stages = h->last_stages;
    out->second_pass = s[5];
    out->eps = h->last_eps;
    return RAG_OK;
}

int rag_stage_kernel_ms(rag_handle_t h, int stage, float* ms_out, int* spans_out) {
    if (!h || !ms_out || !spans_out) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, stage >= 0 && stage < RAG_PROF_STAGES, "stage must be 0 (dense emit), 1 (bm25) or 2 (cross-encoder)");
    auto& p = h->prof[stage];
    ARG_CHECK(h, p.used > 0, "no span recorded for this stage (rag_set_profiling(h, 1) before the calls)");
    HIP_TRY(h, hipSetDevice(h->device));
    float total = 0.f;
    for (int i = 0; i < p.used; ++i) {
        HIP_TRY(h, hipEventSynchronize(p.ev[i].second));
        float ms = 0.f;
        HIP_TRY(h, hipEventElapsedTime(&ms, p.ev[i].first, p.ev[i].second));
        total += ms;
    }
    *ms_out = total;
    *spans_out = p.used;
    return RAG_OK;
}

int rag_dense_kernel_ms(rag_handle_t h, float* gemm_ms_out, int* launches_out) {
    return rag_stage_kernel_ms(h, 0, gemm_ms_out, launches_out);
}

int rag_merge_topk_dev(rag_handle_t h, const int64_t* ids_dev, const double* scores_dev, int n_lists, int64_t list_stride,
                       int Q, int k, int64_t* ids_out_dev, double* scores_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, ids_dev && scores_dev && ids_out_dev && scores_out_dev, "null pointer");
    DEV_ENTRY(h);
    return merge_topk(h, ids_dev, scores_dev, n_lists, list_stride, Q, k, ids_out_dev, scores_out_dev,
                      (hipStream_t)stream);
}

// The fuse step of the row-sharded hybrid search on every rank, after the ONE all-gather of the shards' lists.
int rag_hybrid_fuse_gathered_dev(rag_handle_t h, const int64_t* gathered_dev, int world, int Q, int pool, int k, int rrf_k,
                                 int64_t* lists_out_dev, double* scores_out_dev, int64_t* keys_out_dev, double* rrf_out_dev,
                                 int32_t* ranks_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, gathered_dev && lists_out_dev && scores_out_dev && keys_out_dev && rrf_out_dev, "hybrid_fuse_gathered: null pointer");
    ARG_CHECK(h, world > 0 && Q > 0 && pool > 0 && pool <= RAG_MAX_K && k > 0, "hybrid_fuse_gathered: bad sizes (0 < pool <= 256)");
    DEV_ENTRY(h);
    hipStream_t st = (hipStream_t)stream;
    const int64_t P = (int64_t)Q * pool, stride = 4 * P;
    const double* gs = reinterpret_cast<const double*>(gathered_dev);
    int rc = merge_topk(h, gathered_dev, gs + P, world, stride, Q, pool, lists_out_dev, scores_out_dev, st, 0);
    if (rc) return rc;
    if ((rc = merge_topk(h, gathered_dev + 2 * P, gs + 3 * P, world, stride, Q, pool, lists_out_dev + P, scores_out_dev + P, st, 1))) return rc;
    return rrf_fuse_dev(h, lists_out_dev, Q, 2, pool, P, pool, rrf_k, k, keys_out_dev, rrf_out_dev, ranks_out_dev, st);
}

int rag_pairwise_cosine_host(rag_handle_t h, const float* a, int m, const float* b, int n, int dim, double* out) {
    return pairwise_cosine_host_t<float>(h, a, m, b, n, dim, out);
}

int rag_pairwise_cosine_f64_host(rag_handle_t h, const double* a, int m, const double* b, int n, int dim, double* out) {
    return pairwise_cosine_host_t<double>(h, a, m, b, n, dim, out);
}

int rag_rrf_fuse_host(rag_handle_t h, const int64_t* lists, int Q, int L, int len, int rrf_k, int top_k, int64_t* keys_out,
                      double* scores_out, int32_t* ranks_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return rrf_fuse_host(h, lists, Q, L, len, rrf_k, top_k, keys_out, scores_out, ranks_out);
}

int rag_linear_fuse_topk_host(rag_handle_t h, const double* sem, const double* kw, const double* tmp, int n, double a,
                              double b, double g, int top_k, int32_t* idx_out, double* hyb_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return linear_fuse_topk_host(h, sem, kw, tmp, n, a, b, g, top_k, idx_out, hyb_out);
}

int rag_bm25_load_host(rag_handle_t h, const int64_t* indptr, const int32_t* doc, const int32_t* tf, const int32_t* doc_len,
                       const double* idf, int64_t n_docs, int64_t n_terms, double avgdl, double k1, double b) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return bm25_load_host(h, indptr, doc, tf, doc_len, idf, n_docs, n_terms, avgdl, k1, b);
}

int rag_bm25_append_host(rag_handle_t h, const int64_t* indptr, const int32_t* doc, const int32_t* tf, const int32_t* doc_len,
                         const double* idf_new, int64_t n_docs_new, int64_t n_terms_total) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return bm25_append_host(h, indptr, doc, tf, doc_len, idf_new, n_docs_new, n_terms_total);
}

int rag_bm25_fold(rag_handle_t h) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return bm25_fold(h);
}

int rag_bm25_live_counts_host(rag_handle_t h, int32_t* df_out_host, int64_t* n_docs_live_out, int64_t* sum_doc_len_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return bm25_live_counts_host(h, df_out_host, n_docs_live_out, sum_doc_len_out);
}

int rag_bm25_set_statistics_host(rag_handle_t h, const double* idf_host, double avgdl) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return bm25_set_statistics_host(h, idf_host, avgdl);
}

int rag_bm25_refresh(rag_handle_t h, double epsilon, double* idf_out_host, rag_bm25_refresh_info* info_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return bm25_refresh(h, epsilon, idf_out_host, info_out);
}

int rag_bm25_segment_stats(rag_handle_t h, rag_bm25_segments* out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    return bm25_segment_stats(h, out);
}

int rag_bm25_grid_plan(int n_ranges_in_launch, int n_queries, int linear, int64_t* out5) {
    return bm25_grid_plan(n_ranges_in_launch, n_queries, linear, out5);
}

int rag_bm25_index_bytes(const int64_t* indptr_host, int64_t n_docs, int64_t n_terms, int64_t* postings_bytes_out,
                         int64_t* meta_bytes_out, int64_t* table_bytes_out) {
    return bm25_index_bytes(indptr_host, n_docs, n_terms, postings_bytes_out, meta_bytes_out, table_bytes_out);
}

int rag_bm25_topk_host(rag_handle_t h, const int32_t* term_ptr, const int32_t* terms, int Q, int k, int tenant, int64_t* ids_out,
                       int32_t* rows_out, double* scores_out, double* raw_max_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return bm25_topk_host(h, term_ptr, terms, Q, k, tenant, ids_out, rows_out, scores_out, raw_max_out, {nullptr, nullptr});
}
int rag_bm25_topk_tenants_host(rag_handle_t h, const int32_t* term_ptr, const int32_t* terms, int Q, int k, const int32_t* tenants_host,
                               int64_t* ids_out, int32_t* rows_out, double* scores_out, double* raw_max_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, tenants_host && Q > 0 && Q <= 65535, "bm25: null tenants array or bad n_queries");
    HOST_ENTRY(h);
    entry_tenants t;                  // (staged on the stream bm25_run works on)
    if (int rc = entry_tenants_of(h, -1, tenants_host, Q, h->stream, &t)) return rc;
    return bm25_topk_host(h, term_ptr, terms, Q, k, t.tenant, ids_out, rows_out, scores_out, raw_max_out, t.qt);
}

int rag_bm25_topk_dev(rag_handle_t h, const int32_t* term_ptr_dev, const int32_t* terms_dev, int Q, int k, int tenant, int64_t* ids_dev,
                      int32_t* rows_dev, double* scores_dev, double* raw_max_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    DEV_ENTRY(h);
    return bm25_topk_dev(h, term_ptr_dev, terms_dev, Q, k, tenant, ids_dev, rows_dev, scores_dev, raw_max_dev,
                         (hipStream_t)stream, id_space::of_index(h), {nullptr, nullptr});
}
int rag_bm25_topk_tenants_dev(rag_handle_t h, const int32_t* term_ptr_dev, const int32_t* terms_dev, int Q, int k,
                              const int32_t* tenants_host, int64_t* ids_dev, int32_t* rows_dev, double* scores_dev, double* raw_max_dev,
                              void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, tenants_host && Q > 0 && Q <= 65535, "bm25: null tenants array or bad n_queries");
    DEV_ENTRY(h);
    entry_tenants t;
    if (int rc = entry_tenants_of(h, -1, tenants_host, Q, (hipStream_t)stream, &t)) return rc;
    return bm25_topk_dev(h, term_ptr_dev, terms_dev, Q, k, t.tenant, ids_dev, rows_dev, scores_dev, raw_max_dev, (hipStream_t)stream, id_space::of_index(h),
                         t.qt);
}

int rag_rrf_fuse_dev(rag_handle_t h, const int64_t* lists_dev, int Q, int L, int len, int rrf_k, int top_k, int64_t* keys_dev,
                     double* scores_dev, int32_t* ranks_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    DEV_ENTRY(h);
    return rrf_fuse_dev(h, lists_dev, Q, L, len, len, (int64_t)L * len, rrf_k, top_k, keys_dev, scores_dev, ranks_dev,
                        (hipStream_t)stream);
}

// dense top-pool + BM25 top-pool + RRF -> top-k, all on the device, one call (BASELINE.json configs[2]).
// lists_ws_dev: caller scratch [2][Q][pool] int64 (receives the dense, then the BM25 ranked id list);
// scores_ws_dev: caller scratch [Q][pool] float64.
static int hybrid_rrf_entry(rag_handle_t h, const float* q_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev, int Q, int pool,
                            int k, int rrf_k, int tenant, const int32_t* tenants_host, int64_t* lists_ws_dev, double* scores_ws_dev,
                            int64_t* keys_out_dev, double* rrf_out_dev, int32_t* ranks_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, Q > 0 && Q <= 65535, "hybrid: 1 <= n_queries <= 65535");
    ARG_CHECK(h, q_dev && term_ptr_dev && lists_ws_dev && scores_ws_dev && keys_out_dev && rrf_out_dev, "hybrid: null pointer");
    ARG_CHECK(h, aligned16(q_dev), "hybrid: the queries (q_dev) must be 16-byte aligned");
    ARG_CHECK(h, pool > 0 && pool <= RAG_MAX_K && k > 0, "hybrid: 0 < pool <= 256");
    if (int rc = keyword_postings_aligned(h, false, "hybrid", RAG_OK)) return rc;
    DEV_ENTRY(h);
    hipStream_t st = (hipStream_t)stream;
    entry_tenants t;
    int rc = entry_tenants_of(h, tenant, tenants_host, Q, st, &t);
    if (rc) return rc;
    if ((rc = hybrid_legs(h, q_dev, term_ptr_dev, terms_dev, Q, pool, t.tenant, lists_ws_dev, scores_ws_dev, st, id_space::of_index(h), t.qt)))
        return rc;
    return rrf_fuse_dev(h, lists_ws_dev, Q, 2, pool, (int64_t)Q * pool, pool, rrf_k, k, keys_out_dev, rrf_out_dev, ranks_out_dev, st);
}
int rag_hybrid_rrf_dev(rag_handle_t h, const float* q_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev, int Q, int pool,
                       int k, int rrf_k, int tenant, int64_t* lists_ws_dev, double* scores_ws_dev, int64_t* keys_out_dev,
                       double* rrf_out_dev, int32_t* ranks_out_dev, void* stream) {
    return hybrid_rrf_entry(h, q_dev, term_ptr_dev, terms_dev, Q, pool, k, rrf_k, tenant, nullptr, lists_ws_dev, scores_ws_dev, keys_out_dev,
                            rrf_out_dev, ranks_out_dev, stream);
}
int rag_hybrid_rrf_tenants_dev(rag_handle_t h, const float* q_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev, int Q, int pool,
                               int k, int rrf_k, const int32_t* tenants_host, int64_t* lists_ws_dev, double* scores_ws_dev,
                               int64_t* keys_out_dev, double* rrf_out_dev, int32_t* ranks_out_dev, void* stream) {
    if (h && !tenants_host) { LOCK(h); ARG_CHECK(h, false, "null tenants array"); }
    return hybrid_rrf_entry(h, q_dev, term_ptr_dev, terms_dev, Q, pool, k, rrf_k, -1, tenants_host, lists_ws_dev, scores_ws_dev, keys_out_dev,
                            rrf_out_dev, ranks_out_dev, stream);
}

// ---- learned-sparse inverted index (bm25.hip, "the learned-sparse inverted index") ------------------------------------------------
int rag_sparse_load_host(rag_handle_t h, const int64_t* indptr_host, const int32_t* doc_host, const float* weight_host, int64_t n_docs,
                         int64_t n_terms) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);                      // queued *_dev searches read the postings this call replaces
    return sparse_load_host(h, indptr_host, doc_host, weight_host, n_docs, n_terms);
}

int rag_sparse_append_host(rag_handle_t h, const int64_t* indptr_host, const int32_t* doc_host, const float* weight_host, int64_t n_docs_new,
                           int64_t n_terms_total) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);                      // queued *_dev searches read the tail this call replaces
    return sparse_append_host(h, indptr_host, doc_host, weight_host, n_docs_new, n_terms_total);
}

// The block is device memory, the call a host write: it waits for `stream` (the block's producer), then for every queued *_dev
// call as rag_sparse_append_host does, and builds on the handle's own stream.
int rag_sparse_append_dev(rag_handle_t h, const int32_t* doc_ptr_dev, const int32_t* terms_dev, const float* weights_dev, int64_t n_docs_new,
                          int64_t nnz_cap, int64_t n_terms_total, void* stream) {
    if (!h) return RAG_ERR_ARG;
    hipError_t e = hipSetDevice(h->device);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    LOCK(h);
    HIP_TRY(h, e);
    HOST_ENTRY(h);
    return sparse_append_docs_dev(h, doc_ptr_dev, terms_dev, weights_dev, n_docs_new, nnz_cap, n_terms_total);
}

int rag_sparse_append_docs_host(rag_handle_t h, const int32_t* doc_ptr_host, const int32_t* terms_host, const float* weights_host,
                                int64_t n_docs_new, int64_t nnz_cap, int64_t n_terms_total) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return sparse_append_docs_host(h, doc_ptr_host, terms_host, weights_host, n_docs_new, nnz_cap, n_terms_total);
}

int rag_sparse_clear(rag_handle_t h) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);                      // queued *_dev searches read the postings this call frees
    return sparse_clear(h);
}

int rag_sparse_export_host(rag_handle_t h, int64_t* indptr_out, int32_t* doc_out, float* weight_out, int64_t* n_docs_out,
                           int64_t* n_terms_out, int64_t* nnz_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return sparse_export_host(h, indptr_out, doc_out, weight_out, n_docs_out, n_terms_out, nnz_out);
}

int rag_sparse_fold(rag_handle_t h) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return sparse_fold(h);
}

int rag_sparse_segment_stats(rag_handle_t h, rag_bm25_segments* out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    return sparse_segment_stats(h, out);
}

int rag_sparse_info(rag_handle_t h, int64_t* n_docs_out, int64_t* n_terms_out, int64_t* nnz_out, int64_t* hbm_bytes_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    return sparse_info(h, n_docs_out, n_terms_out, nnz_out, hbm_bytes_out);
}

int rag_sparse_topk_host(rag_handle_t h, const int32_t* term_ptr_host, const int32_t* terms_host, const float* qweights_host, int n_queries,
                         int k, int tenant, int64_t* ids_out, int32_t* rows_out, double* scores_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return sparse_topk_host(h, term_ptr_host, terms_host, qweights_host, n_queries, k, tenant, ids_out, rows_out, scores_out, {nullptr, nullptr});
}
int rag_sparse_topk_tenants_host(rag_handle_t h, const int32_t* term_ptr_host, const int32_t* terms_host, const float* qweights_host,
                                 int n_queries, int k, const int32_t* tenants_host, int64_t* ids_out, int32_t* rows_out, double* scores_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, tenants_host && n_queries > 0 && n_queries <= 65535, "sparse: null tenants array or bad n_queries");
    HOST_ENTRY(h);
    entry_tenants t;                  // (staged on the stream bm25_run works on)
    if (int rc = entry_tenants_of(h, -1, tenants_host, n_queries, h->stream, &t)) return rc;
    return sparse_topk_host(h, term_ptr_host, terms_host, qweights_host, n_queries, k, t.tenant, ids_out, rows_out, scores_out, t.qt);
}

int rag_sparse_topk_dev(rag_handle_t h, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev, int n_queries,
                        int k, int tenant, int64_t* ids_dev, int32_t* rows_dev, double* scores_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    DEV_ENTRY(h);
    return sparse_topk_dev(h, term_ptr_dev, terms_dev, qweights_dev, n_queries, k, tenant, ids_dev, rows_dev, scores_dev, (hipStream_t)stream,
                           id_space::of_index(h), {nullptr, nullptr});
}
int rag_sparse_topk_tenants_dev(rag_handle_t h, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev, int n_queries,
                                int k, const int32_t* tenants_host, int64_t* ids_dev, int32_t* rows_dev, double* scores_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, tenants_host && n_queries > 0 && n_queries <= 65535, "sparse: null tenants array or bad n_queries");
    DEV_ENTRY(h);
    entry_tenants t;
    if (int rc = entry_tenants_of(h, -1, tenants_host, n_queries, (hipStream_t)stream, &t)) return rc;
    return sparse_topk_dev(h, term_ptr_dev, terms_dev, qweights_dev, n_queries, k, t.tenant, ids_dev, rows_dev, scores_dev, (hipStream_t)stream,
                           id_space::of_index(h), t.qt);
}

int rag_sparse_scores_host(rag_handle_t h, const int32_t* term_ptr_host, const int32_t* terms_host, const float* qweights_host,
                           int n_queries, double* out_host) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return sparse_scores_host(h, term_ptr_host, terms_host, qweights_host, n_queries, out_host);
}

// dense top-pool + learned-sparse top-pool + RRF -> top-k: rag_hybrid_rrf_dev with the sparse list in place of the BM25 list
// (hybrid_legs: the sparse leg forks onto the side stream exactly as the BM25 leg does).
static int hybrid_sparse_rrf_entry(rag_handle_t h, const float* q_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                                   const float* qweights_dev, int Q, int pool, int k, int rrf_k, int tenant, const int32_t* tenants_host,
                                   int64_t* lists_ws_dev, double* scores_ws_dev, int64_t* keys_out_dev, double* rrf_out_dev,
                                   int32_t* ranks_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, Q > 0 && Q <= 65535, "hybrid_sparse: 1 <= n_queries <= 65535");
    ARG_CHECK(h, q_dev && term_ptr_dev && qweights_dev && lists_ws_dev && scores_ws_dev && keys_out_dev && rrf_out_dev, "hybrid_sparse: null pointer");
    ARG_CHECK(h, aligned16(q_dev), "hybrid_sparse: the queries (q_dev) must be 16-byte aligned");
    ARG_CHECK(h, pool > 0 && pool <= RAG_MAX_K && k > 0, "hybrid_sparse: 0 < pool <= 256");
    if (int rc = keyword_postings_aligned(h, true, "hybrid_sparse", RAG_ERR_ARG)) return rc;
    DEV_ENTRY(h);
    hipStream_t st = (hipStream_t)stream;
    entry_tenants t;
    if (int rc = entry_tenants_of(h, tenant, tenants_host, Q, st, &t)) return rc;
    ARG_CHECK(h, t.tenant < 0 || h->tenants != nullptr, "hybrid_sparse: tenant filter requested but no tenants loaded");
    if (int rc = hybrid_legs(h, q_dev, term_ptr_dev, terms_dev, Q, pool, t.tenant, lists_ws_dev, scores_ws_dev, st, id_space::of_index(h), t.qt,
                             qweights_dev))
        return rc;
    return rrf_fuse_dev(h, lists_ws_dev, Q, 2, pool, (int64_t)Q * pool, pool, rrf_k, k, keys_out_dev, rrf_out_dev, ranks_out_dev, st);
}
int rag_hybrid_sparse_rrf_dev(rag_handle_t h, const float* q_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                              const float* qweights_dev, int Q, int pool, int k, int rrf_k, int tenant, int64_t* lists_ws_dev,
                              double* scores_ws_dev, int64_t* keys_out_dev, double* rrf_out_dev, int32_t* ranks_out_dev, void* stream) {
    return hybrid_sparse_rrf_entry(h, q_dev, term_ptr_dev, terms_dev, qweights_dev, Q, pool, k, rrf_k, tenant, nullptr, lists_ws_dev,
                                   scores_ws_dev, keys_out_dev, rrf_out_dev, ranks_out_dev, stream);
}
int rag_hybrid_sparse_rrf_tenants_dev(rag_handle_t h, const float* q_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                                      const float* qweights_dev, int Q, int pool, int k, int rrf_k, const int32_t* tenants_host,
                                      int64_t* lists_ws_dev, double* scores_ws_dev, int64_t* keys_out_dev, double* rrf_out_dev,
                                      int32_t* ranks_out_dev, void* stream) {
    if (h && !tenants_host) { LOCK(h); ARG_CHECK(h, false, "null tenants array"); }
    return hybrid_sparse_rrf_entry(h, q_dev, term_ptr_dev, terms_dev, qweights_dev, Q, pool, k, rrf_k, -1, tenants_host, lists_ws_dev,
                                   scores_ws_dev, keys_out_dev, rrf_out_dev, ranks_out_dev, stream);
}

// Per-row temporal score of the linear fusion: RECENCY_WEIGHT * 0.5 ** (days_old / half_life) computed by the host from
// created_at / uploaded_at exactly as rag/retrieval.py:266-292 does (shard_format.temporal_scores). NULL clears it (zeros).
int rag_index_set_temporal_host(rag_handle_t h, const double* temporal, int64_t n_rows) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, temporal == nullptr || n_rows == h->n_rows, "temporal array length must equal the index row count");
    HOST_ENTRY(h);
    h->temporal.reset();
    h->temporal_absmax = 0.0;
    if (temporal == nullptr || n_rows == 0) return RAG_OK;
    for (int64_t i = 0; i < n_rows; ++i) h->temporal_absmax = std::max(h->temporal_absmax, std::fabs(temporal[i]));
    ARG_CHECK(h, std::isfinite(h->temporal_absmax), "temporal scores must be finite");
    if (int rc = h->temporal.alloc(h, (size_t)n_rows)) return rc;
    HIP_TRY(h, hipMemcpy(h->temporal, temporal, (size_t)n_rows * sizeof(double), hipMemcpyHostToDevice));
    return RAG_OK;
}

// The two halves of a query sub-batch, shared by the one-call entries and by the begin / finish pair of the fusion over row
// shards (include/rag_hip.h "linear fusion over ROW SHARDS"). lin_ws, carved in one order by linear_carve:
struct linear_ws {
    double* raw; float* raw32;       // [QB][n] float64 BM25 scores of every document, [QB][ld] their float32 copy (the emission operand)
    double* mx; unsigned long long* max_key; float* qscale; float* margin;      // [QB] each (linear_scale_kernel)
    float* gt;                       // [ld] float(gamma * temporal)
    int32_t* term_ptr;               // [QB + 1] the query offsets of a begun sub-batch: finish takes the token counts from them
    int32_t* rows;                   // [QB][RAG_MAX_K] the rows of finish (its block carries ids)
    int QB; int64_t n, ld;
};
// queries per sub-batch: one query tile when the all-document scores fit 8 GB (2 GB + 1 GB at 1M rows), fewer on large
// shards (12.5M rows: 53 queries, 8 GB instead of 38 GB)
static int linear_batch(int64_t n) { return (int)std::max<int64_t>(16, std::min<int64_t>(256, ((int64_t)8 << 30) / (std::max<int64_t>(n, 1) * 12))); }
static int linear_carve(rag_ctx* h, hipStream_t st, linear_ws* w) {
    const int64_t n = h->n_rows, ld = emb16_rows(h);
    const int QB = linear_batch(n);
    const size_t need = stage_size((size_t)QB * n, 8) + stage_size((size_t)QB * ld, 4) + 2 * stage_size(QB, 8) + 2 * stage_size(QB, 4) + stage_size(ld, 4) +
                        stage_size((size_t)QB + 1, 4) + stage_size((size_t)QB * RAG_MAX_K, 4);
    if (need > h->lin_ws.size()) {
        h->lin_begun.on = false;
        if (int rc = h->lin_ws.alloc(h, need)) return rc;
        HIP_TRY(h, hipMemsetAsync(h->lin_ws, 0, need, st));      // the pad rows [n, ld) of raw32 are read by the last tile: keep them 0
    }
    char* p = h->lin_ws;
    w->raw = stage_take<double>(p, (size_t)QB * n);
    w->raw32 = stage_take<float>(p, (size_t)QB * ld);
    w->mx = stage_take<double>(p, QB);
    w->max_key = stage_take<unsigned long long>(p, QB);
    w->qscale = stage_take<float>(p, QB);
    w->margin = stage_take<float>(p, QB);
    w->gt = stage_take<float>(p, ld);
    w->term_ptr = stage_take<int32_t>(p, (size_t)QB + 1);
    w->rows = stage_take<int32_t>(p, (size_t)QB * RAG_MAX_K);
    w->QB = QB; w->n = n; w->ld = ld;
    return RAG_OK;
}
// what the entries ask of the weights and of the index (the messages are rag_hybrid_linear_dev's)
static int linear_check_weights(rag_ctx* h, int Q, int k, double alpha, double beta, double gamma) {
    ARG_CHECK(h, Q > 0 && k > 0 && k <= RAG_MAX_K, "hybrid_linear: need Q > 0 and 0 < k <= 256");
    ARG_CHECK(h, alpha > 0.0, "hybrid_linear: alpha must be positive (the cosine drives the candidate search)");
    ARG_CHECK(h, std::isfinite(alpha) && std::isfinite(beta) && std::isfinite(gamma), "hybrid_linear: weights must be finite");
    return RAG_OK;
}
static int linear_check_index(rag_ctx* h, int Q, int tenant, const int32_t* tenants_host) {
    ARG_CHECK(h, tenants_host == nullptr || Q <= 65535, "hybrid_linear: a tenant array takes n_queries <= 65535");
    if (tenants_host != nullptr)
        for (int q = 0; q < Q && tenant < 0; ++q) tenant = std::max(tenants_host[q], -1);      // (for the check below: some filtered query)
    ARG_CHECK(h, tenant < 0 || h->tenants != nullptr, "hybrid_linear: tenant filter requested but no tenants loaded");
    if (int rc = bm25_fresh(h)) return rc;
    ARG_CHECK(h, bm25_n_docs(h) == h->n_rows && h->n_rows > 0, "hybrid_linear: needs BM25 postings row-aligned with a non-empty index");
    return RAG_OK;
}
// half (a): ONE pass of the scoring kernel writes the float64 scores (exact fusion of the survivors), their float32 copy (the emission
// operand) and the per-query maximum; r3 re-read the 2 GB twice more (a one-workgroup-per-query max: 1.8 ms of a 4.5-ms call;
// a bias pass: 0.6 ms)
// (per-query tenants go with their sub-batch: the maximum is each query's own tenant's, the search filters by it)
static int linear_scores(rag_ctx* h, const linear_ws& w, const int32_t* term_ptr_dev, const int32_t* terms_dev, int qc, int tenant,
                         query_tenants qt, hipStream_t st) {
    HIP_TRY(h, hipMemsetAsync(w.max_key, 0, (size_t)qc * sizeof(unsigned long long), st));
    return bm25_scores_dev(h, term_ptr_dev, terms_dev, qc, w.raw, st, w.raw32, w.ld, w.max_key, tenant, qt);
}
// half (b): max_key -> divisor, beta / max, margin (token counts from term_ptr_dev), gamma * t when make_gt; the fused search; the
// components of the returned rows
static int linear_search(rag_ctx* h, const linear_ws& w, const int32_t* term_ptr_dev, bool make_gt, const float* q_dev, int qc, int k,
                         double alpha, double beta, double gamma, int tenant, query_tenants qt, int64_t* ids_out_dev, int32_t* rows_out_dev,
                         double* hybrid_out_dev, double* semantic_out_dev, double* keyword_out_dev, double* temporal_out_dev, hipStream_t st) {
    double neg_per_token = 0.0;
    if (int rc = bm25_negative_bound_args(h, &neg_per_token)) return rc;
    float* gt = (h->temporal != nullptr && gamma != 0.0) ? w.gt : nullptr;
    const linear_neg_bound nb = {term_ptr_dev, neg_per_token};
    int rc = linear_prepare(h, w.max_key, nb, qc, w.n, h->temporal, beta, gamma, w.mx, w.qscale, w.margin, make_gt ? gt : nullptr, w.ld, st);
    if (rc) return rc;
    const dense_fused fz = {w.raw32, w.ld, w.qscale, w.margin, gt, w.raw, w.n, w.mx, h->temporal, alpha, beta, gamma};
    if ((rc = dense_search_fused(h, q_dev, qc, k, tenant, ids_out_dev, rows_out_dev, hybrid_out_dev, st, &fz, id_space::of_index(h), qt))) return rc;
    if (semantic_out_dev || keyword_out_dev || temporal_out_dev)
        rc = linear_components(h, q_dev, rows_out_dev, qc, k, &fz, semantic_out_dev, keyword_out_dev, temporal_out_dev, st);
    return rc;
}

// HybridRetriever.hybrid_search (rag/retrieval.py:214-322) over the WHOLE resident index instead of a host-side corpus list:
// per query, hybrid = (alpha * cosine + beta * keyword) + gamma * temporal for every row (keyword = BM25Okapi score / max over
// the corpus, 1.0 when that max is <= 0; temporal from rag_index_set_temporal_host), stable sort descending, first k.
// The weights are the caller's (intent table or constructor defaults, :232-238). Queries are processed 256 at a time: the
// all-document BM25 scores of a sub-batch (float64, 2 GB at 1M rows) and their float32 emission bias stay in a workspace.
static int hybrid_linear_entry(rag_handle_t h, const float* q_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev, int Q, int k,
                               double alpha, double beta, double gamma, int tenant, const int32_t* tenants_host, int64_t* ids_out_dev,
                               int32_t* rows_out_dev, double* hybrid_out_dev, double* semantic_out_dev, double* keyword_out_dev,
                               double* temporal_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, q_dev && term_ptr_dev && ids_out_dev && rows_out_dev && hybrid_out_dev, "hybrid_linear: null pointer");
    ARG_CHECK(h, aligned16(q_dev), "hybrid_linear: the queries (q_dev) must be 16-byte aligned");
    if (int rc = linear_check_weights(h, Q, k, alpha, beta, gamma)) return rc;
    if (int rc = linear_check_index(h, Q, tenant, tenants_host)) return rc;
    DEV_ENTRY(h);
    h->lin_begun.on = false;            // the planes of a begun pair are overwritten
    hipStream_t st = (hipStream_t)stream;
    entry_tenants t;
    if (int rc = entry_tenants_of(h, tenant, tenants_host, Q, st, &t)) return rc;
    linear_ws w;
    if (int rc = linear_carve(h, st, &w)) return rc;
    for (int q0 = 0; q0 < Q; q0 += w.QB) {
        const int qc = std::min(w.QB, Q - q0);
        const size_t o = (size_t)q0 * k;
        int rc = linear_scores(h, w, term_ptr_dev + q0, terms_dev, qc, t.tenant, t.qt + q0, st);
        if (rc) return rc;
        rc = linear_search(h, w, term_ptr_dev + q0, q0 == 0, q_dev + (size_t)q0 * h->dim, qc, k, alpha, beta, gamma, t.tenant, t.qt + q0,
                           ids_out_dev + o, rows_out_dev + o, hybrid_out_dev + o, semantic_out_dev ? semantic_out_dev + o : nullptr,
                           keyword_out_dev ? keyword_out_dev + o : nullptr, temporal_out_dev ? temporal_out_dev + o : nullptr, st);
        if (rc) return rc;
    }
    return RAG_OK;
}
int rag_hybrid_linear_dev(rag_handle_t h, const float* q_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev, int Q, int k,
                          double alpha, double beta, double gamma, int tenant, int64_t* ids_out_dev, int32_t* rows_out_dev,
                          double* hybrid_out_dev, double* semantic_out_dev, double* keyword_out_dev, double* temporal_out_dev,
                          void* stream) {
    return hybrid_linear_entry(h, q_dev, term_ptr_dev, terms_dev, Q, k, alpha, beta, gamma, tenant, nullptr, ids_out_dev, rows_out_dev,
                               hybrid_out_dev, semantic_out_dev, keyword_out_dev, temporal_out_dev, stream);
}
int rag_hybrid_linear_tenants_dev(rag_handle_t h, const float* q_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev, int Q, int k,
                                  double alpha, double beta, double gamma, const int32_t* tenants_host, int64_t* ids_out_dev,
                                  int32_t* rows_out_dev, double* hybrid_out_dev, double* semantic_out_dev, double* keyword_out_dev,
                                  double* temporal_out_dev, void* stream) {
    if (h && !tenants_host) { LOCK(h); ARG_CHECK(h, false, "null tenants array"); }
    return hybrid_linear_entry(h, q_dev, term_ptr_dev, terms_dev, Q, k, alpha, beta, gamma, -1, tenants_host, ids_out_dev, rows_out_dev,
                               hybrid_out_dev, semantic_out_dev, keyword_out_dev, temporal_out_dev, stream);
}

// ---- the linear fusion over ROW SHARDS: the seam between the two halves, a gather of the ranks' maxima in between -------------
int rag_hybrid_linear_batch(rag_handle_t h, int* max_queries_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, max_queries_out != nullptr, "hybrid_linear_batch: null pointer");
    *max_queries_out = linear_batch(h->n_rows);
    return RAG_OK;
}

// what begin and finish share beyond the one-call entries' checks: one sub-batch, ids through id_base - or explicit ids that the
// id map vouches for (idmap.hip: enabled, and the ids ascend with the rows; the order is all that is needed here)
static int linear_check_shard(rag_ctx* h, const char* who, int Q) {
    if (int rc = idmap_shard_gate(h, who, ": the index has explicit ids; a row shard is loaded with id_base (the order across shards is id_base + row)"))
        return rc;
    const int QB = linear_batch(h->n_rows);
    if (Q > QB) {
        h->err = "bad argument: " + std::string(who) + ": n_queries " + std::to_string(Q) + " exceeds the sub-batch of this index, " +
                 std::to_string(QB) + " queries (rag_hybrid_linear_batch)";
        return RAG_ERR_ARG;
    }
    return RAG_OK;
}

static int hybrid_linear_begin_entry(rag_handle_t h, const int32_t* term_ptr_dev, const int32_t* terms_dev, int Q, int tenant,
                                     const int32_t* tenants_host, double* local_max_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    h->lin_begun.on = false;            // a begin replaces whatever was begun, and a failed one leaves nothing begun
    ARG_CHECK(h, term_ptr_dev && local_max_out_dev, "hybrid_linear_begin: null pointer");
    ARG_CHECK(h, Q > 0, "hybrid_linear_begin: need n_queries > 0");
    if (int rc = linear_check_index(h, Q, tenant, tenants_host)) return rc;
    if (int rc = linear_check_shard(h, "hybrid_linear_begin", Q)) return rc;
    DEV_ENTRY(h);
    hipStream_t st = (hipStream_t)stream;
    entry_tenants t;
    if (int rc = entry_tenants_of(h, tenant, tenants_host, Q, st, &t)) return rc;
    linear_ws w;
    if (int rc = linear_carve(h, st, &w)) return rc;
    if (int rc = linear_scores(h, w, term_ptr_dev, terms_dev, Q, t.tenant, t.qt, st)) return rc;
    HIP_TRY(h, hipMemcpyAsync(w.term_ptr, term_ptr_dev, ((size_t)Q + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    if (int rc = linear_max_out(h, w.max_key, Q, local_max_out_dev, st)) return rc;
    h->lin_begun.Q = Q;
    h->lin_begun.n_rows = h->n_rows;
    h->lin_begun.tenant = tenants_host ? -1 : std::max(tenant, -1);
    h->lin_begun.tenants.clear();
    if (tenants_host) h->lin_begun.tenants.assign(tenants_host, tenants_host + Q);
    h->lin_begun.on = true;
    return RAG_OK;
}
int rag_hybrid_linear_begin_dev(rag_handle_t h, const int32_t* term_ptr_dev, const int32_t* terms_dev, int Q, int tenant,
                                double* local_max_out_dev, void* stream) {
    return hybrid_linear_begin_entry(h, term_ptr_dev, terms_dev, Q, tenant, nullptr, local_max_out_dev, stream);
}
int rag_hybrid_linear_begin_tenants_dev(rag_handle_t h, const int32_t* term_ptr_dev, const int32_t* terms_dev, int Q,
                                        const int32_t* tenants_host, double* local_max_out_dev, void* stream) {
    if (h && !tenants_host) { LOCK(h); ARG_CHECK(h, false, "null tenants array"); }
    return hybrid_linear_begin_entry(h, term_ptr_dev, terms_dev, Q, -1, tenants_host, local_max_out_dev, stream);
}

static int hybrid_linear_finish_entry(rag_handle_t h, const float* q_dev, const double* gathered_max_dev, int world, int Q, int k,
                                      double alpha, double beta, double gamma, int tenant, const int32_t* tenants_host,
                                      int64_t* partial_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    const bool begun = h->lin_begun.on;
    h->lin_begun.on = false;            // consumed by this call, whatever comes of it
    ARG_CHECK(h, q_dev && gathered_max_dev && partial_out_dev, "hybrid_linear_finish: null pointer");
    ARG_CHECK(h, aligned16(q_dev), "hybrid_linear_finish: the queries (q_dev) must be 16-byte aligned");
    ARG_CHECK(h, world > 0, "hybrid_linear_finish: need world > 0");
    if (int rc = linear_check_weights(h, Q, k, alpha, beta, gamma)) return rc;
    bool same = begun && Q == h->lin_begun.Q && h->n_rows == h->lin_begun.n_rows && h->lin_ws != nullptr;
    if (same && tenants_host) same = (int)h->lin_begun.tenants.size() == Q && std::equal(tenants_host, tenants_host + Q, h->lin_begun.tenants.begin());
    else if (same) same = h->lin_begun.tenants.empty() && std::max(tenant, -1) == h->lin_begun.tenant;
    if (!same) {
        h->err = begun ? "hybrid_linear_finish: n_queries or the tenant argument differ from the rag_hybrid_linear_begin_dev before it"
                       : "hybrid_linear_finish: no rag_hybrid_linear_begin_dev before it, or a host call, a write or rag_hybrid_linear_dev "
                         "came in between (the score planes are gone)";
        return RAG_ERR_STATE;
    }
    if (int rc = linear_check_index(h, Q, tenant, tenants_host)) return rc;
    if (int rc = linear_check_shard(h, "hybrid_linear_finish", Q)) return rc;
    DEV_ENTRY(h);
    hipStream_t st = (hipStream_t)stream;
    entry_tenants t;
    if (int rc = entry_tenants_of(h, tenant, tenants_host, Q, st, &t)) return rc;
    linear_ws w;
    if (int rc = linear_carve(h, st, &w)) return rc;      // (sized by begin: nothing is allocated here)
    if (int rc = linear_max_reduce(h, gathered_max_dev, world, Q, w.max_key, st)) return rc;
    const size_t P = (size_t)Q * k;
    double* planes = reinterpret_cast<double*>(partial_out_dev + P);
    return linear_search(h, w, w.term_ptr, true, q_dev, Q, k, alpha, beta, gamma, t.tenant, t.qt, partial_out_dev, w.rows, planes,
                         planes + P, planes + 2 * P, planes + 3 * P, st);
}
int rag_hybrid_linear_finish_dev(rag_handle_t h, const float* q_dev, const double* gathered_max_dev, int world, int Q, int k,
                                 double alpha, double beta, double gamma, int tenant, int64_t* partial_out_dev, void* stream) {
    return hybrid_linear_finish_entry(h, q_dev, gathered_max_dev, world, Q, k, alpha, beta, gamma, tenant, nullptr, partial_out_dev, stream);
}
int rag_hybrid_linear_finish_tenants_dev(rag_handle_t h, const float* q_dev, const double* gathered_max_dev, int world, int Q, int k,
                                         double alpha, double beta, double gamma, const int32_t* tenants_host, int64_t* partial_out_dev,
                                         void* stream) {
    if (h && !tenants_host) { LOCK(h); ARG_CHECK(h, false, "null tenants array"); }
    return hybrid_linear_finish_entry(h, q_dev, gathered_max_dev, world, Q, k, alpha, beta, gamma, -1, tenants_host, partial_out_dev, stream);
}

int rag_hybrid_linear_merge_gathered_dev(rag_handle_t h, const int64_t* gathered_dev, int world, int Q, int k, int64_t* ids_out_dev,
                                         double* hybrid_out_dev, double* semantic_out_dev, double* keyword_out_dev,
                                         double* temporal_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, gathered_dev && ids_out_dev && hybrid_out_dev, "hybrid_linear_merge: null pointer");
    DEV_ENTRY(h);
    return linear_merge(h, gathered_dev, world, Q, k, ids_out_dev, hybrid_out_dev, semantic_out_dev, keyword_out_dev, temporal_out_dev,
                        (hipStream_t)stream);
}

int rag_bm25_set_normalize(rag_handle_t h, int on) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    // no wait: the switch is host state that a *_dev call reads while it enqueues, so a call queued earlier keeps the old value
    return bm25_set_normalize(h, on);
}

int rag_bm25_scores_host(rag_handle_t h, const int32_t* term_ptr, const int32_t* terms, int Q, double* out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return bm25_scores_host(h, term_ptr, terms, Q, out);
}

int rag_bm25_scores_adhoc_host(rag_handle_t h, const int64_t* indptr, const int32_t* doc, const int32_t* tf, const int32_t* doc_len,
                               const double* idf, int64_t n_docs, int64_t n_terms, double avgdl, double k1, double b,
                               const int32_t* term_ptr, const int32_t* terms, int Q, double* out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return bm25_scores_adhoc_host(h, indptr, doc, tf, doc_len, idf, n_docs, n_terms, avgdl, k1, b, term_ptr, terms, Q, out);
}

int rag_ce_load_host(rag_handle_t h, const rag_ce_config* cfg, const float* const* tensors, int n) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return ce_load_host(h, cfg, tensors, n);
}

int rag_ce_score_host(rag_handle_t h, const int32_t* ids, const int32_t* tt, const int32_t* lens, int P, int L, float* out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return ce_score(h, ids, tt, lens, P, L, out, h->stream, true);
}

int rag_ce_score_dev(rag_handle_t h, const int32_t* ids, const int32_t* tt, const int32_t* lens, int P, int L, float* out,
                     void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    DEV_ENTRY(h);
    return ce_score(h, ids, tt, lens, P, L, out, (hipStream_t)stream, false);
}

int rag_embed_load_host(rag_handle_t h, const rag_ce_config* cfg, const float* const* tensors, int n, int flags) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return embed_load_host(h, cfg, tensors, n, flags);
}

int rag_embed_host(rag_handle_t h, const int32_t* ids, const int32_t* tt, const int32_t* lens, int n_texts, int L, float* out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return embed_run(h, ids, tt, lens, n_texts, L, out, h->stream, true);
}

int rag_embed_dev(rag_handle_t h, const int32_t* ids, const int32_t* tt, const int32_t* lens, int n_texts, int L, float* out, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    DEV_ENTRY(h);
    return embed_run(h, ids, tt, lens, n_texts, L, out, (hipStream_t)stream, false);
}

int rag_embed_heads_load_host(rag_handle_t h, const float* tok_w, const float* tok_b, int tok_dim, const float* lex_w, float lex_b) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return embed_heads_load_host(h, tok_w, tok_b, tok_dim, lex_w, lex_b);
}

int rag_embed_multi_host(rag_handle_t h, const int32_t* ids, const int32_t* tt, const int32_t* lens, int n_texts, int L, float* dense_out,
                         float* lex_out, float* tok_out, int64_t tok_rows_cap, int64_t* row_off_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return embed_multi_host(h, ids, tt, lens, n_texts, L, dense_out, lex_out, tok_out, tok_rows_cap, row_off_out);
}

int rag_embed_multi_dev(rag_handle_t h, const int32_t* ids, const int32_t* tt, const int32_t* lens, int n_texts, int L, float* dense_out,
                        float* lex_out, float* tok_out, int64_t tok_rows_cap, int64_t* row_off_out, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    DEV_ENTRY(h);
    return embed_multi_dev(h, ids, tt, lens, n_texts, L, dense_out, lex_out, tok_out, tok_rows_cap, row_off_out, (hipStream_t)stream);
}

int rag_maxsim_host(rag_handle_t h, const float* q_vecs, const int64_t* q_off, int n_q, const float* d_vecs, const int64_t* d_off, int n_d,
                    const int32_t* pair_q, const int32_t* pair_d, int n_pairs, int dim, float* out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return maxsim_host(h, q_vecs, q_off, n_q, d_vecs, d_off, n_d, pair_q, pair_d, n_pairs, dim, out);
}

int rag_maxsim_dev(rag_handle_t h, const float* q_vecs, const int64_t* q_off, int n_q, const float* d_vecs, const int64_t* d_off, int n_d,
                   const int32_t* pair_q, const int32_t* pair_d, int n_pairs, int dim, float* out, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    DEV_ENTRY(h);
    return maxsim_dev(h, q_vecs, q_off, n_q, d_vecs, d_off, n_d, pair_q, pair_d, n_pairs, dim, out, (hipStream_t)stream);
}

int rag_lexical_match_host(rag_handle_t h, const int32_t* q_ids, const float* q_w, const int32_t* q_lens, int n_q, int Lq,
                           const int32_t* d_ids, const float* d_w, const int32_t* d_lens, int n_d, int Ld, const int32_t* pair_q,
                           const int32_t* pair_d, int n_pairs, const int32_t* skip_ids, int n_skip, float* out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return lexical_match_host(h, q_ids, q_w, q_lens, n_q, Lq, d_ids, d_w, d_lens, n_d, Ld, pair_q, pair_d, n_pairs, skip_ids, n_skip, out);
}

int rag_lexical_match_dev(rag_handle_t h, const int32_t* q_ids, const float* q_w, const int32_t* q_lens, int n_q, int Lq,
                          const int32_t* d_ids, const float* d_w, const int32_t* d_lens, int n_d, int Ld, const int32_t* pair_q,
                          const int32_t* pair_d, int n_pairs, const int32_t* skip_ids_host, int n_skip, float* out, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    DEV_ENTRY(h);
    return lexical_match_dev(h, q_ids, q_w, q_lens, n_q, Lq, d_ids, d_w, d_lens, n_d, Ld, pair_q, pair_d, n_pairs, skip_ids_host, n_skip, out,
                             (hipStream_t)stream);
}

int rag_lexical_compact_host(rag_handle_t h, const int32_t* ids, const float* weights, const int32_t* lens, int n_texts, int L,
                             const int32_t* skip_ids, int n_skip, int32_t* term_ptr_out, int32_t* terms_out, float* qweights_out,
                             int64_t terms_cap) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return lexical_compact_host(h, ids, weights, lens, n_texts, L, skip_ids, n_skip, term_ptr_out, terms_out, qweights_out, terms_cap);
}

int rag_lexical_compact_dev(rag_handle_t h, const int32_t* ids, const float* weights, const int32_t* lens, int n_texts, int L,
                            const int32_t* skip_ids_host, int n_skip, int32_t* term_ptr_out, int32_t* terms_out, float* qweights_out,
                            int64_t terms_cap, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    DEV_ENTRY(h);
    return lexical_compact_dev(h, ids, weights, lens, n_texts, L, skip_ids_host, n_skip, term_ptr_out, terms_out, qweights_out, terms_cap,
                               (hipStream_t)stream);
}

int rag_ce_length_class(int head_dim, int seq_len, int* class_out) {
    const int c = ce_length_class(head_dim, seq_len);
    if (!class_out || c == 0) return RAG_ERR_ARG;
    *class_out = c;
    return RAG_OK;
}

int rag_model_seq_limit(rag_handle_t h, int which, int* limit_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, limit_out && (which == 0 || which == 1), "model_seq_limit: which is 0 (cross-encoder) or 1 (embedder)");
    const int lim = ce_model_seq_limit(h, which);
    if (lim == 0) {
        h->err = which == 0 ? "no cross-encoder loaded" : "no embedding model loaded";
        return RAG_ERR_STATE;
    }
    *limit_out = lim;
    return RAG_OK;
}

int rag_embed_dim(rag_handle_t h, int* dim_out) {
    if (!h || !dim_out) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, embed_dim(h) > 0, "no embedding model loaded");
    *dim_out = embed_dim(h);
    return RAG_OK;
}

int rag_mmr_select_host(rag_handle_t h, const float* query, const float* emb, int n, int dim, int top_k, double lambda,
                        int variant, int32_t* sel_out, double* score_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return mmr_select_host(h, query, emb, n, dim, top_k, lambda, variant, sel_out, score_out);
}

// candidates = rows of the resident index (fp32 master rows): rows_dev[Q][pool], -1 = empty slot
int rag_mmr_select_dev(rag_handle_t h, const float* q_dev, const int32_t* rows_dev, int Q, int pool, int top_k, double lambda,
                       int variant, int32_t* sel_dev, double* score_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, h->emb32 != nullptr && rows_dev, "mmr_select_dev: no index loaded / null rows");
    DEV_ENTRY(h);
    return mmr_select_dev(h, q_dev, h->emb32, rows_dev, Q, pool, h->dim, top_k, lambda, variant, sel_dev, score_dev,
                          (hipStream_t)stream);
}

int rag_chunk_chain_host(rag_handle_t h, const float* emb, const int32_t* sent_len, int n, int dim, double threshold,
                         int max_chunk, int min_chunk, int32_t* group_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return chunk_chain_host(h, emb, sent_len, n, dim, threshold, max_chunk, min_chunk, group_out);
}

int rag_tokens_load_host(rag_handle_t h, const int32_t* tokens, const int32_t* lens, int64_t n_rows, int L) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return tokens_load_host(h, tokens, lens, n_rows, L, 16);
}

int rag_tokens_load_wide_host(rag_handle_t h, const int32_t* tokens, const int32_t* lens, int64_t n_rows, int L, int id_bits) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, id_bits == 16 || id_bits == 24, "tokens_load: id_bits must be 16 or 24");
    HOST_ENTRY(h);
    return tokens_load_host(h, tokens, lens, n_rows, L, id_bits);
}

int rag_tokens_reserve(rag_handle_t h, int64_t n_rows_total, int L) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return tokens_reserve(h, n_rows_total, L, 16);
}

int rag_tokens_reserve_wide(rag_handle_t h, int64_t n_rows_total, int L, int id_bits) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, id_bits == 16 || id_bits == 24, "tokens_reserve: id_bits must be 16 or 24");
    HOST_ENTRY(h);
    return tokens_reserve(h, n_rows_total, L, id_bits);
}

int rag_tokens_info(rag_handle_t h, int64_t* rows_out, int* L_out, int* id_bits_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    return tokens_info(h, rows_out, L_out, id_bits_out);
}

int rag_ce_set_pair_format(rag_handle_t h, int format) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, format == RAG_PAIR_BERT || format == RAG_PAIR_ROBERTA, "ce_set_pair_format: unknown pair format (RAG_PAIR_BERT or RAG_PAIR_ROBERTA)");
    // no wait: host state that a *_dev call reads while it enqueues (as rag_set_option), so a call queued earlier keeps the old layout
    h->pair_format = format;
    return RAG_OK;
}

int rag_tokens_append_dev(rag_handle_t h, const int32_t* tokens_dev, const int32_t* lens_dev, int64_t n_rows, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    DEV_ENTRY(h);
    return tokens_append_dev(h, tokens_dev, lens_dev, n_rows, (hipStream_t)stream);
}

int rag_retrieve_rerank_dev(rag_handle_t h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                            const int32_t* q_tok_dev, const int32_t* q_len_dev, int Lq, int Q, int pool, int k, int rrf_k,
                            int tenant, int mode, int cls_id, int sep_id, int L_pair, int64_t* ids_out_dev,
                            double* scores_out_dev, float* logits_out_dev, int64_t* cand_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, aligned16(q_emb_dev), "retrieve_rerank: the query embeddings (q_emb_dev) must be 16-byte aligned");
    DEV_ENTRY(h);
    return retrieve_rerank_dev(h, q_emb_dev, term_ptr_dev, terms_dev, q_tok_dev, q_len_dev, Lq, Q, pool, k, rrf_k, tenant, mode,
                               cls_id, sep_id, L_pair, ids_out_dev, scores_out_dev, logits_out_dev, cand_out_dev,
                               (hipStream_t)stream, {nullptr, nullptr});
}
int rag_retrieve_rerank_tenants_dev(rag_handle_t h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                                    const int32_t* q_tok_dev, const int32_t* q_len_dev, int Lq, int Q, int pool, int k, int rrf_k,
                                    const int32_t* tenants_host, int mode, int cls_id, int sep_id, int L_pair, int64_t* ids_out_dev,
                                    double* scores_out_dev, float* logits_out_dev, int64_t* cand_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, tenants_host && Q > 0 && Q <= 65535, "retrieve_rerank: null tenants array or bad n_queries");
    ARG_CHECK(h, aligned16(q_emb_dev), "retrieve_rerank: the query embeddings (q_emb_dev) must be 16-byte aligned");
    DEV_ENTRY(h);
    entry_tenants t;
    if (int rc = entry_tenants_of(h, -1, tenants_host, Q, (hipStream_t)stream, &t)) return rc;
    return retrieve_rerank_dev(h, q_emb_dev, term_ptr_dev, terms_dev, q_tok_dev, q_len_dev, Lq, Q, pool, k, rrf_k, t.tenant, mode,
                               cls_id, sep_id, L_pair, ids_out_dev, scores_out_dev, logits_out_dev, cand_out_dev,
                               (hipStream_t)stream, t.qt);
}

int rag_ce_build_pairs_dev(rag_handle_t h, const int32_t* q_tok_dev, const int32_t* q_len_dev, int Lq, const int64_t* cand_dev, int Q,
                           int pool, int64_t token_id_base, int L_pair, int cls_id, int sep_id, int32_t* ids_out_dev,
                           int32_t* tt_out_dev, int32_t* lens_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    DEV_ENTRY(h);
    return ce_build_pairs_dev(h, q_tok_dev, q_len_dev, Lq, cand_dev, Q, pool, token_id_base, L_pair, cls_id, sep_id, ids_out_dev,
                              tt_out_dev, lens_out_dev, (hipStream_t)stream);
}

int rag_rerank_topk_dev(rag_handle_t h, const float* logits_dev, const int64_t* cand_dev, int Q, int pool, int k, int64_t* ids_out_dev,
                        double* scores_out_dev, float* logits_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    DEV_ENTRY(h);
    return rerank_topk_dev(h, logits_dev, cand_dev, Q, pool, k, ids_out_dev, scores_out_dev, logits_out_dev, (hipStream_t)stream);
}

// ---- resident token-vector store and late-interaction rerank (tokvec.hip; the composite in pipeline.hip) ---------------------------
int rag_tokvec_reserve(rag_handle_t h, int64_t n_docs_total, int64_t rows_total, int dim) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);                      // queued *_dev reranks read the store this call replaces
    return tokvec_reserve(h, n_docs_total, rows_total, dim, RAG_TOKVEC_FP16);
}

int rag_tokvec_reserve_form(rag_handle_t h, int64_t n_docs_total, int64_t rows_total, int dim, int form) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return tokvec_reserve(h, n_docs_total, rows_total, dim, form);
}

int rag_tokvec_append_dev(rag_handle_t h, const float* vecs_dev, const int64_t* row_off_dev, int64_t n_docs, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    DEV_ENTRY(h);
    return tokvec_append(h, vecs_dev, row_off_dev, n_docs, (hipStream_t)stream, false);
}

int rag_tokvec_append_host(rag_handle_t h, const float* vecs_host, const int64_t* row_off_host, int64_t n_docs) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return tokvec_append(h, vecs_host, row_off_host, n_docs, h->stream, true);
}

int rag_tokvec_load_host(rag_handle_t h, const float* vecs_host, const int64_t* off_host, int64_t n_docs, int dim) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return tokvec_load_host(h, vecs_host, off_host, n_docs, dim, RAG_TOKVEC_FP16);
}

int rag_tokvec_load_form_host(rag_handle_t h, const float* vecs_host, const int64_t* off_host, int64_t n_docs, int dim, int form) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return tokvec_load_host(h, vecs_host, off_host, n_docs, dim, form);
}

int rag_tokvec_info(rag_handle_t h, int64_t* n_docs_out, int64_t* rows_out, int* dim_out, int64_t* hbm_bytes_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    return tokvec_info(h, n_docs_out, rows_out, dim_out, hbm_bytes_out);
}

int rag_tokvec_form(rag_handle_t h, int* form_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    return tokvec_form(h, form_out);
}

int rag_tokvec_fetch_host(rag_handle_t h, int64_t doc, float* out_host, int64_t cap_rows, int64_t* n_rows_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return tokvec_fetch_host(h, doc, out_host, cap_rows, n_rows_out);
}

int rag_tokvec_rerank_dev(rag_handle_t h, const float* q_vecs_dev, const int64_t* q_off_dev, const int32_t* cand_rows_dev, int Q, int pool,
                          int k, int64_t* ids_out_dev, int32_t* rows_out_dev, double* scores_out_dev, float* pair_scores_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    DEV_ENTRY(h);
    return tokvec_rerank(h, q_vecs_dev, q_off_dev, cand_rows_dev, Q, pool, k, ids_out_dev, rows_out_dev, scores_out_dev, pair_scores_out_dev,
                         (hipStream_t)stream);
}

int rag_tokvec_rerank_host(rag_handle_t h, const float* q_vecs_host, const int64_t* q_off_host, const int32_t* cand_rows_host, int Q, int pool,
                           int k, int64_t* ids_out_host, int32_t* rows_out_host, double* scores_out_host, float* pair_scores_out_host) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return tokvec_rerank_host(h, q_vecs_host, q_off_host, cand_rows_host, Q, pool, k, ids_out_host, rows_out_host, scores_out_host,
                              pair_scores_out_host);
}

int rag_retrieve_maxsim_dev(rag_handle_t h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                            const float* qweights_dev, const float* q_vecs_dev, const int64_t* q_off_dev, int Q, int pool, int k, int rrf_k,
                            int tenant, int mode, int64_t* ids_out_dev, double* scores_out_dev, int64_t* cand_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, aligned16(q_emb_dev), "retrieve_maxsim: the query embeddings (q_emb_dev) must be 16-byte aligned");
    ARG_CHECK(h, aligned16(q_vecs_dev), "retrieve_maxsim: the query's token vectors (q_vecs_dev) must be 16-byte aligned");
    DEV_ENTRY(h);
    return retrieve_maxsim_dev(h, q_emb_dev, term_ptr_dev, terms_dev, qweights_dev, q_vecs_dev, q_off_dev, Q, pool, k, rrf_k, tenant, mode,
                               ids_out_dev, scores_out_dev, cand_out_dev, (hipStream_t)stream, {nullptr, nullptr});
}
int rag_retrieve_maxsim_tenants_dev(rag_handle_t h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                                    const float* qweights_dev, const float* q_vecs_dev, const int64_t* q_off_dev, int Q, int pool, int k,
                                    int rrf_k, const int32_t* tenants_host, int mode, int64_t* ids_out_dev, double* scores_out_dev,
                                    int64_t* cand_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, tenants_host && Q > 0 && Q <= 65535, "retrieve_maxsim: null tenants array or bad n_queries");
    ARG_CHECK(h, aligned16(q_emb_dev), "retrieve_maxsim: the query embeddings (q_emb_dev) must be 16-byte aligned");
    ARG_CHECK(h, aligned16(q_vecs_dev), "retrieve_maxsim: the query's token vectors (q_vecs_dev) must be 16-byte aligned");
    DEV_ENTRY(h);
    entry_tenants t;
    if (int rc = entry_tenants_of(h, -1, tenants_host, Q, (hipStream_t)stream, &t)) return rc;
    return retrieve_maxsim_dev(h, q_emb_dev, term_ptr_dev, terms_dev, qweights_dev, q_vecs_dev, q_off_dev, Q, pool, k, rrf_k, t.tenant, mode,
                               ids_out_dev, scores_out_dev, cand_out_dev, (hipStream_t)stream, t.qt);
}

int rag_sparse_score_rows_dev(rag_handle_t h, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev,
                              const int32_t* cand_rows_dev, int n_queries, int pool, double* scores_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    DEV_ENTRY(h);
    return sparse_score_rows_dev(h, term_ptr_dev, terms_dev, qweights_dev, cand_rows_dev, n_queries, pool, scores_out_dev, (hipStream_t)stream);
}

int rag_sparse_score_rows_host(rag_handle_t h, const int32_t* term_ptr_host, const int32_t* terms_host, const float* qweights_host,
                               const int32_t* cand_rows_host, int n_queries, int pool, double* scores_out_host) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HOST_ENTRY(h);
    return sparse_score_rows_host(h, term_ptr_host, terms_host, qweights_host, cand_rows_host, n_queries, pool, scores_out_host);
}

int rag_m3_score_rows_dev(rag_handle_t h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                          const float* qweights_dev, const float* q_vecs_dev, const int64_t* q_off_dev, const int32_t* cand_rows_dev,
                          int n_queries, int pool, int k, double w_dense, double w_sparse, double w_colbert, int64_t* ids_out_dev,
                          int32_t* rows_out_dev, double* scores_out_dev, double* components_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    DEV_ENTRY(h);
    return m3_score_rows_dev(h, q_emb_dev, term_ptr_dev, terms_dev, qweights_dev, q_vecs_dev, q_off_dev, cand_rows_dev, n_queries, pool, k, w_dense,
                             w_sparse, w_colbert, ids_out_dev, rows_out_dev, scores_out_dev, components_out_dev, (hipStream_t)stream);
}

int rag_retrieve_m3_dev(rag_handle_t h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                        const float* qweights_dev, const float* q_vecs_dev, const int64_t* q_off_dev, int n_queries, int pool, int k,
                        int rrf_k, int tenant, int mode, double w_dense, double w_sparse, double w_colbert, int64_t* ids_out_dev,
                        double* scores_out_dev, double* components_out_dev, int64_t* cand_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, aligned16(q_emb_dev), "retrieve_m3: the query embeddings (q_emb_dev) must be 16-byte aligned (the candidate search reads them whatever the dense weight)");
    DEV_ENTRY(h);
    return retrieve_m3_dev(h, q_emb_dev, term_ptr_dev, terms_dev, qweights_dev, q_vecs_dev, q_off_dev, n_queries, pool, k, rrf_k, tenant, mode,
                           w_dense, w_sparse, w_colbert, ids_out_dev, scores_out_dev, components_out_dev, cand_out_dev, (hipStream_t)stream,
                           {nullptr, nullptr});
}
// the row-sharded three-way search: the three steps between the two all-gathers (pipeline.hip)
int rag_m3_candidates_gathered_dev(rag_handle_t h, const int64_t* gathered_dev, int world, int n_queries, int pool, int rrf_k, int mode,
                                   int64_t* lists_out_dev, double* scores_out_dev, int64_t* cand_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    DEV_ENTRY(h);
    return m3_candidates_gathered_dev(h, gathered_dev, world, n_queries, pool, rrf_k, mode, lists_out_dev, scores_out_dev, cand_out_dev,
                                      (hipStream_t)stream);
}
int rag_m3_score_ids_dev(rag_handle_t h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                         const float* qweights_dev, const float* q_vecs_dev, const int64_t* q_off_dev, const int64_t* cand_ids_dev,
                         int n_queries, int slots, double w_dense, double w_sparse, double w_colbert, int64_t* partial_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    DEV_ENTRY(h);
    return m3_score_ids_dev(h, q_emb_dev, term_ptr_dev, terms_dev, qweights_dev, q_vecs_dev, q_off_dev, cand_ids_dev, n_queries, slots, w_dense,
                            w_sparse, w_colbert, partial_out_dev, (hipStream_t)stream);
}
int rag_m3_combine_gathered_dev(rag_handle_t h, const int64_t* cand_ids_dev, const int64_t* gathered_dev, int world, int n_queries, int slots,
                                int k, double w_dense, double w_sparse, double w_colbert, int64_t* ids_out_dev, double* scores_out_dev,
                                double* components_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    DEV_ENTRY(h);
    return m3_combine_gathered_dev(h, cand_ids_dev, gathered_dev, world, n_queries, slots, k, w_dense, w_sparse, w_colbert, ids_out_dev,
                                   scores_out_dev, components_out_dev, (hipStream_t)stream);
}

int rag_retrieve_m3_tenants_dev(rag_handle_t h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                                const float* qweights_dev, const float* q_vecs_dev, const int64_t* q_off_dev, int n_queries, int pool, int k,
                                int rrf_k, const int32_t* tenants_host, int mode, double w_dense, double w_sparse, double w_colbert,
                                int64_t* ids_out_dev, double* scores_out_dev, double* components_out_dev, int64_t* cand_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, tenants_host && n_queries > 0 && n_queries <= 65535, "retrieve_m3: null tenants array or bad n_queries");
    ARG_CHECK(h, aligned16(q_emb_dev), "retrieve_m3: the query embeddings (q_emb_dev) must be 16-byte aligned (the candidate search reads them whatever the dense weight)");
    DEV_ENTRY(h);
    entry_tenants t;
    if (int rc = entry_tenants_of(h, -1, tenants_host, n_queries, (hipStream_t)stream, &t)) return rc;
    return retrieve_m3_dev(h, q_emb_dev, term_ptr_dev, terms_dev, qweights_dev, q_vecs_dev, q_off_dev, n_queries, pool, k, rrf_k, t.tenant, mode,
                           w_dense, w_sparse, w_colbert, ids_out_dev, scores_out_dev, components_out_dev, cand_out_dev, (hipStream_t)stream, t.qt);
}

int rag_search_m3_tokens_dev(rag_handle_t h, const int32_t* input_ids_dev, const int32_t* token_type_ids_dev, const int32_t* lens_dev,
                             int n_queries, int seq_len, const int32_t* skip_ids_host, int n_skip, int pool, int k, int rrf_k, int tenant,
                             int mode, double w_dense, double w_sparse, double w_colbert, int64_t* ids_out_dev, double* scores_out_dev,
                             double* components_out_dev, int64_t* cand_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    DEV_ENTRY(h);
    return search_m3_tokens_dev(h, input_ids_dev, token_type_ids_dev, lens_dev, n_queries, seq_len, skip_ids_host, n_skip, pool, k, rrf_k, tenant,
                                mode, w_dense, w_sparse, w_colbert, ids_out_dev, scores_out_dev, components_out_dev, cand_out_dev,
                                (hipStream_t)stream, {nullptr, nullptr});
}
int rag_search_m3_tokens_tenants_dev(rag_handle_t h, const int32_t* input_ids_dev, const int32_t* token_type_ids_dev, const int32_t* lens_dev,
                                     int n_queries, int seq_len, const int32_t* skip_ids_host, int n_skip, int pool, int k, int rrf_k,
                                     const int32_t* tenants_host, int mode, double w_dense, double w_sparse, double w_colbert,
                                     int64_t* ids_out_dev, double* scores_out_dev, double* components_out_dev, int64_t* cand_out_dev,
                                     void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, tenants_host && n_queries > 0 && n_queries <= 65535, "search_m3_tokens: null tenants array or bad n_queries");
    DEV_ENTRY(h);
    entry_tenants t;
    if (int rc = entry_tenants_of(h, -1, tenants_host, n_queries, (hipStream_t)stream, &t)) return rc;
    return search_m3_tokens_dev(h, input_ids_dev, token_type_ids_dev, lens_dev, n_queries, seq_len, skip_ids_host, n_skip, pool, k, rrf_k, t.tenant,
                                mode, w_dense, w_sparse, w_colbert, ids_out_dev, scores_out_dev, components_out_dev, cand_out_dev,
                                (hipStream_t)stream, t.qt);
}

}  // extern "C"
