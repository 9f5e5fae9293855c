// Live writes to the resident index (include/rag_hip.h: rag_index_insert_host, rag_index_delete_host, rag_index_compact,
// rag_index_compact_bm25, rag_index_deleted_rows): the INSERT / DELETE the reference agent issues on almost every turn (database/operations.py:22-57,
// 162-172; rag/document_store.py:343-390, 524-542) without reloading the index.
//
// Representation: a deleted row stays where it is and is marked RAG_DEAD_ROW in rag_ctx::vis (a copy of the tenant table, or
// zeros without one), which every search kernel reads through row_visible(). While nothing is deleted vis is null and the
// kernels run exactly as before. Compaction removes the marked rows from every plane, stably, in place.
#include "common.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#define LOCK(h) std::lock_guard<std::mutex> lock_((h)->mu)

// ---- kernels ------------------------------------------------------------------------------------------------------------
// vis[first, first + n) = tenant of the row (0 without a tenant table); keep_dead leaves deleted rows deleted
__global__ __launch_bounds__(256) void live_vis_fill_kernel(int32_t* __restrict__ vis, const int32_t* __restrict__ tenants,
                                                             int64_t first, int64_t n, int keep_dead) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t r = first + i;
        if (keep_dead && vis[r] == RAG_DEAD_ROW) continue;
        vis[r] = tenants != nullptr ? tenants[r] : 0;
    }
}

__global__ __launch_bounds__(256) void live_iota_ids_kernel(int64_t* __restrict__ ids, int64_t id_base, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) ids[i] = id_base + i;
}

// One pass over the stored id column for a whole id set (sorted, unique, staged from the host; binary-searched per row):
// counts the visible rows (row_visible(vis, row, tenant)) whose id is in the set and, with mark, deletes them.
// Serves rag_index_delete_host (mark = 1) and the duplicate check of rag_index_insert_host (mark = 0, tenant = -1).
__global__ __launch_bounds__(256) void live_idset_scan_kernel(const int64_t* __restrict__ ids, int64_t n_rows,
                                                               const int64_t* __restrict__ set, int n_set, int32_t* __restrict__ vis,
                                                               int tenant, int mark, unsigned long long* __restrict__ count) {
    for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < n_rows; row += (int64_t)gridDim.x * 256) {
        const int64_t id = ids[row];
        int lo = 0, hi = n_set;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (set[mid] < id) lo = mid + 1;
            else hi = mid;
        }
        if (lo == n_set || set[lo] != id || !row_visible(vis, row, tenant)) continue;
        if (mark) vis[row] = RAG_DEAD_ROW;
        atomicAdd(count, 1ull);
    }
}

// the same on an implicit-id index (id = id_base + row): a range check per id of the set, no pass over the rows
__global__ __launch_bounds__(256) void live_idrange_kernel(int64_t id_base, int64_t n_rows, const int64_t* __restrict__ set, int n_set,
                                                            int32_t* __restrict__ vis, int tenant, int mark,
                                                            unsigned long long* __restrict__ count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_set) return;
    const int64_t id = set[i];
    if (id < id_base || (uint64_t)id - (uint64_t)id_base >= (uint64_t)n_rows) return;
    const int64_t row = id - id_base;
    if (!row_visible(vis, row, tenant)) return;
    if (mark) vis[row] = RAG_DEAD_ROW;
    atomicAdd(count, 1ull);
}

// compaction, step 1: live rows per 256-row tile
__global__ __launch_bounds__(256) void live_tile_count_kernel(const int32_t* __restrict__ vis, int64_t n_rows, int* __restrict__ tile_cnt) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = row < n_rows && vis[row] != RAG_DEAD_ROW;
    const int c = __syncthreads_count(live);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = c;
}

// step 2 (after the exclusive scan of the tile counts): row_map[old] = new row or -1, src_rows[new] = old row
__global__ __launch_bounds__(256) void live_row_map_kernel(const int32_t* __restrict__ vis, int64_t n_rows, const int64_t* __restrict__ tile_off,
                                                            int64_t* __restrict__ row_map, int32_t* __restrict__ src_rows) {
    __shared__ int wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t row = (int64_t)blockIdx.x * 256 + tid;
    const bool live = row < n_rows && vis[row] != RAG_DEAD_ROW;
    const unsigned long long m = __ballot(live);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int off = 0;
    for (int i = 0; i < w; ++i) off += wsum[i];
    if (row < n_rows) {
        const int64_t nr = tile_off[blockIdx.x] + off + before;
        row_map[row] = live ? nr : -1;
        if (live) src_rows[nr] = (int32_t)row;
    }
}

// step 3, per plane and chunk of destination rows [d0, d0 + m): gather the chunk's source rows into the staging buffer. The
// chunk is then copied to its destination, which is contiguous and lies at or below every source of this and later chunks:
// the copy is safe in place.
template <class W>
__global__ __launch_bounds__(256) void live_compact_gather_kernel(const W* __restrict__ plane, uint32_t row_words,
                                                                   const int32_t* __restrict__ src_rows, uint32_t total,
                                                                   W* __restrict__ stage) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const uint32_t r = i / row_words, w = i - r * row_words;
        stage[i] = plane[(size_t)src_rows[r] * row_words + w];
    }
}

// ---- host helpers -----------------------------------------------------------------------------------------------------
static int grid_for(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 8192)); }

// vis rows [first, first + n) from the tenant table (0 without one, or where the table does not cover the rows), growing vis
int live_vis_extend(rag_ctx* h, int64_t first, int64_t n) {
    if (first + n > h->cap_vis) {
        const int64_t cap = std::max(first + n, std::max(h->cap32, h->n_rows));
        dev_buf<int32_t> nv;
        if (int rc = nv.alloc(h, (size_t)cap)) return rc;
        if (h->vis && first > 0) HIP_TRY(h, hipMemcpy(nv, h->vis, (size_t)first * sizeof(int32_t), hipMemcpyDeviceToDevice));
        h->vis = std::move(nv);
        h->cap_vis = cap;
    }
    if (n <= 0) return RAG_OK;
    const int32_t* ten = (h->tenants != nullptr && h->cap_ten >= first + n) ? h->tenants : nullptr;
    hipLaunchKernelGGL(live_vis_fill_kernel, dim3(grid_for(n)), dim3(256), 0, h->stream, h->vis, ten, first, n, 0);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RAG_OK;
}

// the tenant table was replaced (rag_index_set_tenants_host): new tenant numbers, deleted rows stay deleted
int live_vis_rebuild(rag_ctx* h) {
    if (!h->vis || h->n_rows == 0) return RAG_OK;
    const int32_t* ten = (h->tenants != nullptr && h->cap_ten >= h->n_rows) ? h->tenants : nullptr;
    hipLaunchKernelGGL(live_vis_fill_kernel, dim3(grid_for(h->n_rows)), dim3(256), 0, h->stream, h->vis, ten, (int64_t)0, h->n_rows, 1);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RAG_OK;
}

// every write first waits for whatever searches the handle's *_dev calls queued, on any stream: a search queued before a
// write returns the result from before it
static int live_begin(rag_ctx* h) {
    HIP_TRY(h, hipSetDevice(h->device));
    return host_after_dev(h);
}

// row-count-sized workspaces follow the row count: the linear-fusion workspace (its pad rows must read as zero) is
// reallocated by the next rag_hybrid_linear_dev; the float64-scan scratch is sized per call
static void live_rows_changed(rag_ctx* h) { h->lin_ws.reset(); }

// sorted, unique copy of an id array staged in the handle's arena; count slot behind it
static int stage_id_set(rag_ctx* h, const std::vector<int64_t>& set, int64_t** set_dev, unsigned long long** count_dev) {
    int rc = stage_reserve(h, stage_size(set.size(), 8) + stage_size(1, 8));
    if (rc) return rc;
    char* p = h->stage;
    *set_dev = stage_take<int64_t>(p, set.size());
    *count_dev = stage_take<unsigned long long>(p, 1);
    HIP_TRY(h, hipMemcpyAsync(*set_dev, set.data(), set.size() * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(*count_dev, 0, sizeof(unsigned long long), h->stream));
    return RAG_OK;
}

// visible rows whose id is in `set` (sorted, unique); mark = 1 deletes them
static int id_set_apply(rag_ctx* h, const std::vector<int64_t>& set, int tenant, int mark, int64_t* n_out) {
    *n_out = 0;
    if (set.empty() || h->n_rows == 0) return RAG_OK;
    int64_t* sd = nullptr;
    unsigned long long* cd = nullptr;
    int rc = stage_id_set(h, set, &sd, &cd);
    if (rc) return rc;
    if (h->ids)
        hipLaunchKernelGGL(live_idset_scan_kernel, dim3(grid_for(h->n_rows)), dim3(256), 0, h->stream, h->ids, h->n_rows, sd, (int)set.size(),
                           h->vis, tenant, mark, cd);
    else
        hipLaunchKernelGGL(live_idrange_kernel, dim3((unsigned)((set.size() + 255) / 256)), dim3(256), 0, h->stream, h->id_base, h->n_rows, sd,
                           (int)set.size(), h->vis, tenant, mark, cd);
    HIP_TRY(h, hipGetLastError());
    unsigned long long c = 0;
    HIP_TRY(h, hipMemcpyAsync(&c, cd, sizeof(c), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *n_out = (int64_t)c;
    return RAG_OK;
}

static int64_t grow_cap(int64_t cap, int64_t need) { return need <= cap ? cap : std::max(need, cap + cap / 8 + 256); }

extern "C" {

int rag_index_insert_host(rag_handle_t h, const rag_row_block* rb, int64_t* first_row_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, rb != nullptr, "insert: null row block");
    const int64_t n = rb->n;
    ARG_CHECK(h, n >= 0 && (n == 0 || rb->emb != nullptr), "insert: need n >= 0 and emb[n][dim]");
    int rc = live_begin(h);
    if (rc) return rc;
    const int64_t n0 = h->index_loaded ? h->n_rows : 0;
    ARG_CHECK(h, n0 + n < (int64_t)0x7fffff00, "insert: n_rows must fit int32 per GPU");
    const bool empty = n0 == 0;          // planes an empty index does not have yet may be started by this insert
    ARG_CHECK(h, rb->ids != nullptr || h->ids == nullptr, "insert: ids are required (the index stores explicit ids)");
    const bool has_ten = h->tenants != nullptr, has_tmp = h->temporal != nullptr, has_tok = h->tok != nullptr;
    ARG_CHECK(h, has_ten ? rb->tenants != nullptr : (rb->tenants == nullptr || empty),
              "insert: tenants are required iff the index has a tenant table");
    ARG_CHECK(h, has_tmp ? rb->temporal != nullptr : (rb->temporal == nullptr || empty),
              "insert: temporal scores are required iff the index has them");
    ARG_CHECK(h, has_tok ? (rb->tokens != nullptr && rb->token_lens != nullptr) : rb->tokens == nullptr,
              "insert: tokens and token_lens are required iff a token store is loaded");
    if (has_ten && !(h->tenant_rows == n0 && h->cap_ten >= n0)) {
        h->err = "insert: the tenant table is stale (rows were appended after rag_index_set_tenants_host)";
        return RAG_ERR_STATE;
    }
    if ((has_tmp && h->cap_tmp < n0) || (h->ids && h->cap_ids < n0) || (has_tok && h->tok_rows != n0)) {
        h->err = "insert: the temporal scores, ids or token store do not cover the index rows";
        return RAG_ERR_STATE;
    }
    if (first_row_out) *first_row_out = n0;
    if (n == 0) return RAG_OK;
    // ---- host-side checks of the block
    if (rb->tenants)
        for (int64_t i = 0; i < n; ++i) ARG_CHECK(h, rb->tenants[i] >= 0, "insert: tenant numbers must be >= 0");
    double tmax = 0.0;
    if (rb->temporal) {
        for (int64_t i = 0; i < n; ++i) tmax = std::max(tmax, std::fabs(rb->temporal[i]));
        ARG_CHECK(h, std::isfinite(tmax), "insert: temporal scores must be finite");
    }
    std::vector<uint16_t> tok16;
    std::vector<uint8_t> tok_hi8;        // bits 16-23, for a 24-bit store
    const bool wide_tok = has_tok && h->tok_hi != nullptr;
    if (has_tok) {
        const int L = h->tok_L;
        tok16.resize((size_t)n * L);
        if (wide_tok) tok_hi8.resize((size_t)n * L);
        for (int64_t i = 0; i < n * L; ++i) {
            const int32_t v = rb->tokens[i];
            if (wide_tok) {
                ARG_CHECK(h, v >= 0 && v <= 0xFFFFFF, "insert: token ids must be in [0, 16777215]");
                tok_hi8[(size_t)i] = (uint8_t)(v >> 16);
            } else {
                ARG_CHECK(h, v >= 0 && v <= 65535, "insert: token ids must be in [0, 65535]");
            }
            tok16[(size_t)i] = (uint16_t)v;
        }
    }
    std::vector<int64_t> set;
    if (rb->ids) {
        set.assign(rb->ids, rb->ids + n);
        std::sort(set.begin(), set.end());
        ARG_CHECK(h, std::adjacent_find(set.begin(), set.end()) == set.end(), "insert: an id is repeated inside the block");
        int64_t live = 0;
        if ((rc = id_set_apply(h, set, -1, 0, &live))) return rc;
        ARG_CHECK(h, live == 0, "insert: an id is already live in the index (primary key)");
    }
    // ---- capacity: first what rag_index_reserve left, then growth of every row-aligned plane (all allocated before any change)
    const int64_t need = n0 + n;
    const int64_t cap32 = grow_cap(std::max(h->cap32, n0), need);
    const int64_t pad = round_up(std::max(need, cap32), (int64_t)RAG_TILE * 8);
    const int64_t cap_ids = h->ids ? grow_cap(h->cap_ids, need) : cap32, cap_ten = h->tenants ? grow_cap(h->cap_ten, need) : cap32;
    const int64_t cap_tmp = h->temporal ? grow_cap(h->cap_tmp, need) : cap32, cap_vis = grow_cap(h->cap_vis, need);
    const int64_t cap_tok = grow_cap(h->tok_cap, need);
    rag_device_mem g;                    // the grown planes under the handle's field names: dropped whole unless committed below
    bool ok = true;
    auto grow = [&](auto& plane, bool wanted, int64_t rows, size_t row_elems) {
        ok = ok && (!wanted || plane.alloc(h, (size_t)rows * row_elems) == RAG_OK);
    };
    grow(g.emb32, cap32 != h->cap32 || !h->emb32, cap32, h->dim);
    grow(g.emb16, need > h->n_rows_pad || !h->emb16, pad, h->dim_pad);
    grow(g.ids, rb->ids && (!h->ids || need > h->cap_ids), cap_ids, 1);
    grow(g.tenants, rb->tenants && (!h->tenants || need > h->cap_ten), cap_ten, 1);
    grow(g.temporal, rb->temporal && (!h->temporal || need > h->cap_tmp), cap_tmp, 1);
    grow(g.vis, h->vis && need > h->cap_vis, cap_vis, 1);
    grow(g.tok, has_tok && need > h->tok_cap, cap_tok, h->tok_L);
    grow(g.tok_hi, wide_tok && need > h->tok_cap, cap_tok, h->tok_L);
    grow(g.tok_len, has_tok && need > h->tok_cap, cap_tok, 1);
    if (!ok) {
        (void)hipGetLastError();
        h->err = "insert: out of device memory while growing the index (reserve headroom with rag_index_reserve)";
        return RAG_ERR_NOMEM;
    }
    hipStream_t st = h->stream;
    if (!h->index_loaded) {              // inserting on a handle with no index creates one
        if (!h->bad_rows) {
            if ((rc = h->bad_rows.alloc(h, 1))) return rc;
            HIP_TRY(h, hipMemsetAsync(h->bad_rows, 0, sizeof(int), st));
        }
        h->n_rows = 0;
        h->id_base = 0;
        h->index_loaded = true;
    }
    // ---- commit, per grown plane: copy the used rows over (device to device), then move the new allocation into the handle,
    // which frees the old one
    auto commit = [&](auto& plane, auto& grown, size_t row_elems, int64_t* cap, int64_t new_cap) -> int {
        if (!grown) return RAG_OK;
        if (plane && n0 > 0)
            HIP_TRY(h, hipMemcpyAsync(grown, plane, (size_t)n0 * row_elems * sizeof(*grown.get()), hipMemcpyDeviceToDevice, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        plane = std::move(grown);
        if (cap) *cap = new_cap;
        return RAG_OK;
    };
    if ((rc = commit(h->emb32, g.emb32, h->dim, &h->cap32, cap32))) return rc;
    if (g.emb16)                         // tile padding and not-yet-written rows must read as zero vectors
        HIP_TRY(h, hipMemsetAsync(g.emb16 + (size_t)n0 * h->dim_pad, 0, (size_t)(pad - n0) * h->dim_pad * sizeof(half_t), st));
    if ((rc = commit(h->emb16, g.emb16, h->dim_pad, &h->n_rows_pad, pad))) return rc;
    if (g.ids && !h->ids && n0 > 0)      // implicit ids become a stored column (same values)
        hipLaunchKernelGGL(live_iota_ids_kernel, dim3(grid_for(n0)), dim3(256), 0, st, g.ids.get(), h->id_base, n0);
    if ((rc = commit(h->ids, g.ids, 1, &h->cap_ids, cap_ids))) return rc;
    if ((rc = commit(h->tenants, g.tenants, 1, &h->cap_ten, cap_ten))) return rc;
    if ((rc = commit(h->temporal, g.temporal, 1, &h->cap_tmp, cap_tmp))) return rc;
    if ((rc = commit(h->vis, g.vis, 1, &h->cap_vis, cap_vis))) return rc;
    if ((rc = commit(h->tok_hi, g.tok_hi, h->tok_L, nullptr, 0))) return rc;
    if ((rc = commit(h->tok, g.tok, h->tok_L, &h->tok_cap, cap_tok))) return rc;
    if ((rc = commit(h->tok_len, g.tok_len, 1, nullptr, 0))) return rc;
    HIP_TRY(h, hipMemcpyAsync(h->emb32 + (size_t)n0 * h->dim, rb->emb, (size_t)n * h->dim * sizeof(float), hipMemcpyHostToDevice, st));
    if ((rc = dense_index_normalize_range(h, n0, n, st))) return rc;
    if (rb->ids) HIP_TRY(h, hipMemcpyAsync(h->ids + n0, rb->ids, (size_t)n * 8, hipMemcpyHostToDevice, st));
    if (rb->tenants) HIP_TRY(h, hipMemcpyAsync(h->tenants + n0, rb->tenants, (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (rb->temporal) {
        HIP_TRY(h, hipMemcpyAsync(h->temporal + n0, rb->temporal, (size_t)n * 8, hipMemcpyHostToDevice, st));
        h->temporal_absmax = std::max(h->temporal_absmax, tmax);       // sizes the fused-emission error bound
    }
    if (has_tok) {
        HIP_TRY(h, hipMemcpyAsync(h->tok + (size_t)n0 * h->tok_L, tok16.data(), tok16.size() * 2, hipMemcpyHostToDevice, st));
        if (wide_tok) HIP_TRY(h, hipMemcpyAsync(h->tok_hi + (size_t)n0 * h->tok_L, tok_hi8.data(), tok_hi8.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(h, hipMemcpyAsync(h->tok_len + n0, rb->token_lens, (size_t)n * 4, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(h, hipStreamSynchronize(st));
    if (h->vis && (rc = live_vis_extend(h, n0, n))) return rc;
    if (rb->tenants && (rc = dense_tenant_tiles_append(h, rb->tenants, n0, n))) return rc;
    h->n_rows = need;
    if (has_tok) h->tok_rows = need;
    h->bm25_stale = true;
    h->sparse_stale = true;
    live_rows_changed(h);
    return RAG_OK;
}

int rag_index_delete_host(rag_handle_t h, const int64_t* ids, int64_t n_ids, int tenant, int64_t* n_deleted_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, n_ids >= 0 && n_ids < (int64_t)0x7fffffff && (n_ids == 0 || ids != nullptr), "delete: bad id array");
    if (n_deleted_out) *n_deleted_out = 0;
    int rc = live_begin(h);
    if (rc) return rc;
    if (!h->index_loaded || h->n_rows == 0 || n_ids == 0) return RAG_OK;
    ARG_CHECK(h, tenant < 0 || h->tenants != nullptr, "delete: tenant predicate given but no tenant table loaded");
    if (tenant >= 0 && !(h->tenant_rows == h->n_rows && h->cap_ten >= h->n_rows)) {
        h->err = "delete: the tenant table is stale (rows were appended after rag_index_set_tenants_host)";
        return RAG_ERR_STATE;
    }
    if (h->ids && h->cap_ids < h->n_rows) {
        h->err = "delete: the stored ids do not cover the index rows";
        return RAG_ERR_STATE;
    }
    std::vector<int64_t> set(ids, ids + n_ids);
    std::sort(set.begin(), set.end());
    set.erase(std::unique(set.begin(), set.end()), set.end());
    const bool created = h->vis == nullptr;
    if (created && (rc = live_vis_extend(h, 0, h->n_rows))) return rc;
    int64_t n_del = 0;
    if ((rc = id_set_apply(h, set, tenant, 1, &n_del))) return rc;
    if (created && n_del == 0) {             // nothing deleted: keep the searches on their unfiltered path
        h->vis.reset();
        h->cap_vis = 0;
    }
    h->n_deleted += n_del;
    if (n_deleted_out) *n_deleted_out = n_del;
    return RAG_OK;
}

int rag_index_deleted_rows(rag_handle_t h, int64_t* n_deleted_out) {
    if (!h || !n_deleted_out) return RAG_ERR_ARG;
    LOCK(h);
    *n_deleted_out = h->n_deleted;
    return RAG_OK;
}

#define LIVE_STAGING_BYTES ((size_t)1 << 30)       // bound of the compaction's device memory beyond the planes

// rag_index_compact (keep_postings = false: the postings end stale and compacted) and rag_index_compact_bm25 (true: loaded
// postings that describe the rows are renumbered through the row map, beside the old ones, BEFORE the first row moves, and
// swapped in once the rows have moved; bm25_stale is left as it was - current stays current, uncovered rows stay uncovered)
// and rag_index_compact_live (LIVE_KEEP_RESIDENT: the same for the learned-sparse postings as well, and the token-vector store's
// documents move with their rows - tokvec.hip, "the store through a compaction" - instead of going stale)
enum { LIVE_KEEP_NONE = 0, LIVE_KEEP_BM25 = 1, LIVE_KEEP_RESIDENT = 2 };
static int live_compact(rag_ctx* h, int64_t* row_map_out, int64_t* n_rows_out, int keep) {
    int rc = live_begin(h);
    if (rc) return rc;
    const int64_t n0 = h->index_loaded ? h->n_rows : 0;
    if (h->n_deleted == 0 || h->vis == nullptr) {
        if (row_map_out)
            for (int64_t i = 0; i < n0; ++i) row_map_out[i] = i;
        if (n_rows_out) *n_rows_out = n0;
        return RAG_OK;
    }
    if (h->ids && h->cap_ids < n0) {
        h->err = "compact: the stored ids do not cover the index rows";
        return RAG_ERR_STATE;
    }
    hipStream_t st = h->stream;
    // doc ids never change: an implicit-id index stores its ids before any row moves
    if (!h->ids) {
        const int64_t cap = std::max(h->cap32, n0);
        if ((rc = h->ids.alloc(h, (size_t)cap))) return rc;
        h->cap_ids = cap;
        hipLaunchKernelGGL(live_iota_ids_kernel, dim3(grid_for(n0)), dim3(256), 0, st, h->ids, h->id_base, n0);
        HIP_TRY(h, hipGetLastError());
    }
    const int64_t tiles = (n0 + RAG_TILE - 1) / RAG_TILE;
    // (the token-vector store's own maps are per document - new offsets and first source row, tokvec_compact_prepare - and count
    // against the same bound)
    const bool move_tv = keep == LIVE_KEEP_RESIDENT && h->tv_docs_cap > 0 && !h->tv_stale;
    const size_t tv_bytes = move_tv ? stage_size((size_t)h->tv_docs_cap + 1, 8) + stage_size((size_t)h->tv_docs + 1, 8) : 0;
    const size_t map_bytes = stage_size(tiles, 4) + stage_size(tiles, 8) + stage_size(n0, 8) + stage_size(n0, 4);
    ARG_CHECK(h, map_bytes + tv_bytes + ((size_t)64 << 20) <= LIVE_STAGING_BYTES, "compact: the row map of this index exceeds the 1 GiB staging bound");
    const size_t data_bytes = std::min<size_t>((size_t)512 << 20, LIVE_STAGING_BYTES - map_bytes - tv_bytes);
    dev_buf<char> ws;
    if (ws.alloc(h, map_bytes + data_bytes)) {
        (void)hipGetLastError();
        h->err = "compact: out of device memory for the staging buffer";
        return RAG_ERR_NOMEM;
    }
    char* p = ws;
    int* tile_cnt = stage_take<int>(p, tiles);
    int64_t* tile_off = stage_take<int64_t>(p, tiles);
    int64_t* row_map = stage_take<int64_t>(p, n0);
    int32_t* src_rows = stage_take<int32_t>(p, n0);
    char* data = p;
    auto fail = [&](hipError_t e, const char* what) {
        h->err = std::string("compact: ") + what + ": " + hipGetErrorString(e);
        return RAG_ERR_HIP;
    };
    hipLaunchKernelGGL(live_tile_count_kernel, dim3((unsigned)tiles), dim3(256), 0, st, h->vis, n0, tile_cnt);
    std::vector<int> cnt((size_t)tiles);
    hipError_t e = hipMemcpyAsync(cnt.data(), tile_cnt, (size_t)tiles * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(e, "tile counts");
    // exclusive scan of the per-tile live counts (tiles entries: 49K at 12.5M rows), and the first tile that loses a row:
    // rows before it do not move
    std::vector<int64_t> off((size_t)tiles);
    int64_t n_live = 0, first_move = -1;
    for (int64_t t = 0; t < tiles; ++t) {
        off[(size_t)t] = n_live;
        n_live += cnt[(size_t)t];
        if (first_move < 0 && cnt[(size_t)t] < std::min<int64_t>(RAG_TILE, n0 - t * RAG_TILE)) first_move = t * RAG_TILE;
    }
    if (first_move < 0) first_move = n0;
    e = hipMemcpyAsync(tile_off, off.data(), (size_t)tiles * 8, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return fail(e, "tile offsets");
    hipLaunchKernelGGL(live_row_map_kernel, dim3((unsigned)tiles), dim3(256), 0, st, h->vis, n0, tile_off, row_map, src_rows);
    // the postings of the rows that stay, under their new numbers: everything allocated and built here, nothing replaced yet
    struct new_postings {
        rag_bm25_index* p = nullptr;
        ~new_postings() { if (p) bm25_compact_discard(p); }
    } np, np_sparse;
    // one resident index (the BM25 or the learned-sparse postings) that describes the rows: remapped into `dst`
    auto prepare = [&](const rag_bm25_index* ix, bool compacted, new_postings& dst) -> int {
        const int64_t covered = bm25_covered_docs(ix);
        if (ix == nullptr || compacted || covered > n0) return RAG_OK;
        // live rows below row x: the scanned tile offsets + the live rows of x's own tile before it (at most 255 map entries)
        auto live_below = [&](int64_t x, int64_t* out) -> int {
            *out = n_live;
            if (x >= n0) return RAG_OK;
            const int64_t t0 = x / RAG_TILE * RAG_TILE;
            int64_t part[RAG_TILE];
            if (x > t0) HIP_TRY(h, hipMemcpyAsync(part, row_map + t0, (size_t)(x - t0) * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(h, hipStreamSynchronize(st));
            *out = off[(size_t)(t0 / RAG_TILE)];
            for (int64_t i = 0; i < x - t0; ++i) *out += part[i] >= 0;
            return RAG_OK;
        };
        int64_t base_live = 0, covered_live = 0;
        int rc2;
        if ((rc2 = live_below(bm25_base_docs(ix), &base_live))) return rc2;
        if ((rc2 = live_below(covered, &covered_live))) return rc2;
        return bm25_compact_prepare(h, ix, row_map, base_live, covered_live, &dst.p);
    };
    if (keep >= LIVE_KEEP_BM25 && (rc = prepare(h->bm25, h->bm25_compacted, np))) return rc;
    if (keep == LIVE_KEEP_RESIDENT && (rc = prepare(h->sparse, h->sparse_compacted, np_sparse))) return rc;
    // the token-vector store's new offsets and per-document source map, from a host copy of the row map
    tokvec_compact_plan tvp;
    if (move_tv) {
        std::vector<int64_t> map_h((size_t)n0);
        HIP_TRY(h, hipMemcpyAsync(map_h.data(), row_map, (size_t)n0 * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        if ((rc = tokvec_compact_prepare(h, map_h.data(), n0, data_bytes, &tvp))) return rc;
    }
    // every plane, chunk by chunk of destination rows through the staging buffer
    struct plane { void* p; size_t row_bytes; };
    std::vector<plane> planes = {{h->emb32, (size_t)h->dim * 4}, {h->emb16, (size_t)h->dim_pad * 2}, {h->ids, 8}};
    const bool ten = h->tenants && h->cap_ten >= n0, tmp = h->temporal && h->cap_tmp >= n0, tok = h->tok && h->tok_rows == n0;
    if (ten) planes.push_back({h->tenants, 4});
    if (tmp) planes.push_back({h->temporal, 8});
    if (tok) {
        planes.push_back({h->tok, (size_t)h->tok_L * 2});
        if (h->tok_hi) planes.push_back({h->tok_hi, (size_t)h->tok_L});      // a row of L bytes: any alignment
        planes.push_back({h->tok_len, 4});
    }
    for (const plane& pl : planes) {
        const int64_t chunk = std::max<int64_t>(1, (int64_t)(data_bytes / pl.row_bytes));
        for (int64_t d0 = first_move; d0 < n_live; d0 += chunk) {
            const int64_t m = std::min(chunk, n_live - d0);
            const size_t bytes = (size_t)m * pl.row_bytes;
#define LIVE_GATHER(W)                                                                                                       \
    {                                                                                                                        \
        const uint32_t rw = (uint32_t)(pl.row_bytes / sizeof(W)), total = (uint32_t)(bytes / sizeof(W));                     \
        hipLaunchKernelGGL(live_compact_gather_kernel<W>, dim3(grid_for(total)), dim3(256), 0, st, (const W*)pl.p, rw,       \
                           src_rows + d0, total, (W*)data);                                                                  \
    }
            if (pl.row_bytes % 16 == 0) LIVE_GATHER(uint4)
            else if (pl.row_bytes % 8 == 0) LIVE_GATHER(uint2)
            else if (pl.row_bytes % 4 == 0) LIVE_GATHER(uint32_t)
            else if (pl.row_bytes % 2 == 0) LIVE_GATHER(uint16_t)
            else LIVE_GATHER(uint8_t)
#undef LIVE_GATHER
            e = hipMemcpyAsync((char*)pl.p + (size_t)d0 * pl.row_bytes, data, bytes, hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) return fail(e, "row copy");
        }
    }
    // the rows past the new end are tile padding of the fp16 operand again: zero
    if (n0 > n_live) e = hipMemsetAsync(h->emb16 + (size_t)n_live * h->dim_pad, 0, (size_t)(n0 - n_live) * h->dim_pad * 2, st);
    if (e == hipSuccess && row_map_out) e = hipMemcpyAsync(row_map_out, row_map, (size_t)n0 * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return fail(e, "finish");
    if ((rc = tokvec_compact_commit(h, &tvp, data, st))) return rc;      // (the staging buffer is free again: same stream)
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(e, "finish");
    ws.reset();
    h->n_rows = n_live;
    if (tok) h->tok_rows = n_live;
    h->vis.reset();
    h->cap_vis = 0;
    h->n_deleted = 0;
    if (np_sparse.p) {                       // rag_index_compact_live: renumbered with the rows, staleness left as it was
        bm25_compact_commit(&h->sparse, np_sparse.p);
        np_sparse.p = nullptr;
    } else {                                 // not renumbered: a reload makes them current
        h->sparse_stale = true;
        h->sparse_compacted = true;
    }
    if (h->tv_docs_cap > 0 && !move_tv) h->tv_stale = true;      // nor are the resident token vectors, unless they moved (tokvec.hip)
    if (np.p) {
        bm25_compact_commit(&h->bm25, np.p);
        np.p = nullptr;
    } else {
        h->bm25_stale = true;
        h->bm25_compacted = true;
    }
    live_rows_changed(h);
    if (ten) {                               // tenant tile lists of the new row numbers
        std::vector<int32_t> t((size_t)n_live);
        if (n_live > 0) HIP_TRY(h, hipMemcpy(t.data(), h->tenants, (size_t)n_live * 4, hipMemcpyDeviceToHost));
        if ((rc = dense_build_tenant_tiles(h, n_live > 0 ? t.data() : nullptr, n_live))) return rc;
        h->tenant_rows = n_live;
    }
    if (n_rows_out) *n_rows_out = n_live;
    return RAG_OK;
}

int rag_index_compact(rag_handle_t h, int64_t* row_map_out, int64_t* n_rows_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    return live_compact(h, row_map_out, n_rows_out, LIVE_KEEP_NONE);
}

int rag_index_compact_bm25(rag_handle_t h, int64_t* row_map_out, int64_t* n_rows_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    return live_compact(h, row_map_out, n_rows_out, LIVE_KEEP_BM25);
}

int rag_index_compact_live(rag_handle_t h, int64_t* row_map_out, int64_t* n_rows_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    return live_compact(h, row_map_out, n_rows_out, LIVE_KEEP_RESIDENT);
}

}  // extern "C"
