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

// the tenant table where it covers rows [0, n), else null (vis then reads tenant 0)
static const int32_t* tenants_covering(const rag_ctx* h, int64_t n) {
    return (h->tenants != nullptr && (int64_t)h->tenants.size() >= n) ? h->tenants.get() : nullptr;
}

// vis rows [first, first + n) from the tenant table (0 without one, or where the table does not cover the rows), growing vis
int live_vis_extend(rag_ctx* h, int64_t first, int64_t n) {
    if (first + n > (int64_t)h->vis.size()) {
        const int64_t cap = std::max(first + n, std::max(emb32_rows(h), h->n_rows));
        dev_buf<int32_t> nv;
        if (int rc = nv.alloc(h, (size_t)cap)) return rc;
        if (h->vis && first > 0) HIP_TRY(h, hipMemcpy(nv, h->vis, (size_t)first * sizeof(int32_t), hipMemcpyDeviceToDevice));
        h->vis = std::move(nv);
    }
    if (n <= 0) return RAG_OK;
    hipLaunchKernelGGL(live_vis_fill_kernel, dim3(grid_for(n)), dim3(256), 0, h->stream, h->vis, tenants_covering(h, first + n), first, n, 0);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RAG_OK;
}

// the tenant table was replaced (rag_index_set_tenants_host): new tenant numbers, deleted rows stay deleted
int live_vis_rebuild(rag_ctx* h) {
    if (!h->vis || h->n_rows == 0) return RAG_OK;
    hipLaunchKernelGGL(live_vis_fill_kernel, dim3(grid_for(h->n_rows)), dim3(256), 0, h->stream, h->vis, tenants_covering(h, h->n_rows),
                       (int64_t)0, h->n_rows, 1);
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

// visible rows whose id is in `set` (sorted, unique); mark = 1 deletes them. set_dev_out (may be null): where the set was staged
static int id_set_apply(rag_ctx* h, const std::vector<int64_t>& set, int tenant, int mark, int64_t* n_out, const int64_t** set_dev_out = nullptr) {
    *n_out = 0;
    if (set_dev_out) *set_dev_out = nullptr;
    if (set.empty() || h->n_rows == 0) return RAG_OK;
    int64_t* sd = nullptr;
    unsigned long long* cd = nullptr;
    int rc = stage_id_set(h, set, &sd, &cd);
    if (rc) return rc;
    if (set_dev_out) *set_dev_out = sd;
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

// ---- insert -----------------------------------------------------------------------------------------------------------
// one rag_index_insert_host call: the block, where it lands, and what the host makes of it before anything changes
struct insert_job {
    const rag_row_block* rb;
    int64_t n0, n, need;                 // rows before, rows of the block, rows after
    bool has_tok, wide_tok;              // a token store is loaded / a 24-bit one
    double tmax = 0.0;                   // max |temporal score| of the block
    std::vector<uint16_t> tok16;         // the block's token ids narrowed: bits 0-15 ...
    std::vector<uint8_t> tok_hi8;        // ... and bits 16-23, for a 24-bit store
    bool ids_ascend = true;              // the block's ids ascend strictly (what the id map's ids_ascending asks of it)
};

// phase 1: the block brings exactly the planes the index has (an empty index may be started), and those cover its rows
static int insert_check(rag_ctx* h, const insert_job& in) {
    const rag_row_block* rb = in.rb;
    const int64_t n0 = in.n0;
    ARG_CHECK(h, n0 + in.n < (int64_t)0x7fffff00, "insert: n_rows must fit int32 per GPU");
    const bool empty = n0 == 0;          // planes an empty index does not have yet may be started by this insert
    ARG_CHECK(h, rb->ids != nullptr || h->ids == nullptr, "insert: ids are required (the index stores explicit ids)");
    const bool has_ten = h->tenants != nullptr, has_tmp = h->temporal != nullptr;
    ARG_CHECK(h, has_ten ? rb->tenants != nullptr : (rb->tenants == nullptr || empty),
              "insert: tenants are required iff the index has a tenant table");
    ARG_CHECK(h, has_tmp ? rb->temporal != nullptr : (rb->temporal == nullptr || empty),
              "insert: temporal scores are required iff the index has them");
    ARG_CHECK(h, in.has_tok ? (rb->tokens != nullptr && rb->token_lens != nullptr) : rb->tokens == nullptr,
              "insert: tokens and token_lens are required iff a token store is loaded");
    if (has_ten && !tenants_cover(h, n0)) {
        h->err = "insert: the tenant table is stale (rows were appended after rag_index_set_tenants_host)";
        return RAG_ERR_STATE;
    }
    if ((has_tmp && (int64_t)h->temporal.size() < n0) || !ids_cover(h, n0) || (in.has_tok && !tokens_aligned(h, n0))) {
        h->err = "insert: the temporal scores, ids or token store do not cover the index rows";
        return RAG_ERR_STATE;
    }
    return RAG_OK;
}

// phase 2, on the host: tenants >= 0, finite temporal scores, token ids narrowed to the store's width, ids unique and not live
static int insert_convert(rag_ctx* h, insert_job& in) {
    const rag_row_block* rb = in.rb;
    const int64_t n = in.n;
    if (rb->tenants)
        for (int64_t i = 0; i < n; ++i) ARG_CHECK(h, rb->tenants[i] >= 0, "insert: tenant numbers must be >= 0");
    if (rb->temporal) {
        for (int64_t i = 0; i < n; ++i) in.tmax = std::max(in.tmax, std::fabs(rb->temporal[i]));
        ARG_CHECK(h, std::isfinite(in.tmax), "insert: temporal scores must be finite");
    }
    if (in.has_tok) {
        const int L = h->tok_L;
        in.tok16.resize((size_t)n * L);
        if (in.wide_tok) in.tok_hi8.resize((size_t)n * L);
        for (int64_t i = 0; i < n * L; ++i) {
            const int32_t v = rb->tokens[i];
            if (in.wide_tok) {
                ARG_CHECK(h, v >= 0 && v <= 0xFFFFFF, "insert: token ids must be in [0, 16777215]");
                in.tok_hi8[(size_t)i] = (uint8_t)(v >> 16);
            } else {
                ARG_CHECK(h, v >= 0 && v <= 65535, "insert: token ids must be in [0, 65535]");
            }
            in.tok16[(size_t)i] = (uint16_t)v;
        }
    }
    if (rb->ids) {
        for (int64_t i = 1; i < n; ++i) in.ids_ascend = in.ids_ascend && rb->ids[i - 1] < rb->ids[i];
        if (h->idmap.on)
            for (int64_t i = 0; i < n; ++i) ARG_CHECK(h, rb->ids[i] >= 0, "insert: ids must be >= 0 while the id map is enabled");
        std::vector<int64_t> set(rb->ids, rb->ids + n);
        std::sort(set.begin(), set.end());
        ARG_CHECK(h, std::adjacent_find(set.begin(), set.end()) == set.end(), "insert: an id is repeated inside the block");
        int64_t live = 0;
        if (int rc = id_set_apply(h, set, -1, 0, &live)) return rc;
        ARG_CHECK(h, live == 0, "insert: an id is already live in the index (primary key)");
    }
    return RAG_OK;
}

// the planes this block writes rows into, or that follow the rows (vis): the others are left as they are
static bool insert_feeds(const rag_ctx* h, const insert_job& in, int plane) {
    switch (plane) {
    case PLANE_IDS: return in.rb->ids != nullptr;
    case PLANE_TENANTS: return in.rb->tenants != nullptr;
    case PLANE_TEMPORAL: return in.rb->temporal != nullptr;
    case PLANE_VIS: return h->vis != nullptr;
    case PLANE_TOK: case PLANE_TOK_LEN: return in.has_tok;
    case PLANE_TOK_HI: return in.wide_tok;
    default: return true;                // emb32, emb16
    }
}

// phase 3a: every plane the block feeds and that has no room for `need` rows is allocated anew in g, under the handle's field
// names; nothing of the handle changes, so a failure leaves the index as it was. The master rows first use what
// rag_index_reserve left, then grow by grow_cap; emb16 stays padded to 8 tiles beyond them; a plane started here gets the
// master rows' capacity; the three token planes grow together, by the reservation tok_len shows.
static int insert_grow(rag_ctx* h, const insert_job& in, rag_device_mem* g) {
    const int64_t need = in.need, master = grow_cap(std::max(emb32_rows(h), in.n0), need);
    bool ok = true;
    for_each_row_plane(h, [&](int id, auto mp, int64_t width) {
        const bool token = id == PLANE_TOK || id == PLANE_TOK_HI || id == PLANE_TOK_LEN;
        const int64_t cap = token ? tok_cap_rows(h) : plane_rows(h->*mp, width);
        if (!ok || !insert_feeds(h, in, id) || need <= cap) return RAG_OK;
        const int64_t rows = id == PLANE_EMB32   ? master
                             : id == PLANE_EMB16 ? round_up(std::max(need, master), (int64_t)RAG_TILE * 8)
                             : cap > 0           ? grow_cap(cap, need)
                                                 : master;
        ok = (g->*mp).alloc(h, (size_t)rows * width) == RAG_OK;
        return RAG_OK;
    });
    if (ok) return RAG_OK;
    (void)hipGetLastError();
    h->err = "insert: out of device memory while growing the index (reserve headroom with rag_index_reserve)";
    return RAG_ERR_NOMEM;
}

// inserting on a handle with no index creates one
static int insert_start_index(rag_ctx* h) {
    if (h->index_loaded) return RAG_OK;
    if (!h->bad_rows) {
        if (int rc = h->bad_rows.alloc(h, 1)) return rc;
        HIP_TRY(h, hipMemsetAsync(h->bad_rows, 0, sizeof(int), h->stream));
    }
    h->n_rows = 0;
    h->id_base = 0;
    h->index_loaded = true;
    return RAG_OK;
}

// phase 3b, per grown plane: copy the used rows over (device to device), then move the new allocation into the handle, which
// frees the old one
static int insert_move_in(rag_ctx* h, const insert_job& in, rag_device_mem* g) {
    hipStream_t st = h->stream;
    const int64_t n0 = in.n0;
    return for_each_row_plane(h, [&](int id, auto mp, int64_t width) -> int {
        auto& plane = h->*mp;
        auto& grown = g->*mp;
        if (!grown) return RAG_OK;
        const size_t row_bytes = (size_t)width * sizeof(*grown.get());
        if (id == PLANE_EMB16)               // tile padding and not-yet-written rows must read as zero vectors
            HIP_TRY(h, hipMemsetAsync(grown + (size_t)n0 * width, 0, (size_t)(plane_rows(grown, width) - n0) * row_bytes, st));
        if (id == PLANE_IDS && !plane && n0 > 0)      // implicit ids become a stored column (same values)
            hipLaunchKernelGGL(live_iota_ids_kernel, dim3(grid_for(n0)), dim3(256), 0, st, g->ids.get(), h->id_base, n0);
        if (plane && n0 > 0) HIP_TRY(h, hipMemcpyAsync(grown, plane, (size_t)n0 * row_bytes, hipMemcpyDeviceToDevice, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        plane = std::move(grown);
        return RAG_OK;
    });
}

// phase 4: the block's rows into every plane it feeds, then the new row count and what depends on it
static int insert_write(rag_ctx* h, const insert_job& in) {
    const rag_row_block* rb = in.rb;
    const int64_t n0 = in.n0, n = in.n;
    hipStream_t st = h->stream;
    int rc;
    HIP_TRY(h, hipMemcpyAsync(h->emb32 + (size_t)n0 * h->dim, rb->emb, (size_t)n * h->dim * sizeof(float), hipMemcpyHostToDevice, st));
    if ((rc = dense_index_normalize_range(h, n0, n, st))) return rc;
    if (rb->ids) HIP_TRY(h, hipMemcpyAsync(h->ids + n0, rb->ids, (size_t)n * 8, hipMemcpyHostToDevice, st));
    if (rb->tenants) HIP_TRY(h, hipMemcpyAsync(h->tenants + n0, rb->tenants, (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (rb->temporal) {
        HIP_TRY(h, hipMemcpyAsync(h->temporal + n0, rb->temporal, (size_t)n * 8, hipMemcpyHostToDevice, st));
        h->temporal_absmax = std::max(h->temporal_absmax, in.tmax);       // sizes the fused-emission error bound
    }
    if (in.has_tok) {
        HIP_TRY(h, hipMemcpyAsync(h->tok + (size_t)n0 * h->tok_L, in.tok16.data(), in.tok16.size() * 2, hipMemcpyHostToDevice, st));
        if (in.wide_tok)
            HIP_TRY(h, hipMemcpyAsync(h->tok_hi + (size_t)n0 * h->tok_L, in.tok_hi8.data(), in.tok_hi8.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(h, hipMemcpyAsync(h->tok_len + n0, rb->token_lens, (size_t)n * 4, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(h, hipStreamSynchronize(st));
    if (h->vis && (rc = live_vis_extend(h, n0, n))) return rc;
    if (rb->tenants && (rc = dense_tenant_tiles_append(h, rb->tenants, n0, n))) return rc;
    h->n_rows = in.need;
    if (in.has_tok) h->tok_rows = in.need;
    h->bm25_stale = true;
    h->sparse_stale = true;
    live_rows_changed(h);
    return RAG_OK;
}

// ---- compaction -------------------------------------------------------------------------------------------------------
#define LIVE_STAGING_BYTES ((size_t)1 << 30)       // bound of the compaction's device memory beyond the planes

// rag_index_compact (keep_postings = false: the postings end stale and compacted) and rag_index_compact_bm25 (true: loaded
// postings that describe the rows are renumbered through the row map, beside the old ones, BEFORE the first row moves, and
// swapped in once the rows have moved; bm25_stale is left as it was - current stays current, uncovered rows stay uncovered)
// and rag_index_compact_live (LIVE_KEEP_RESIDENT: the same for the learned-sparse postings as well, and the token-vector store's
// documents move with their rows - tokvec.hip, "the store through a compaction" - instead of going stale)
enum { LIVE_KEEP_NONE = 0, LIVE_KEEP_BM25 = 1, LIVE_KEEP_RESIDENT = 2 };

// postings built beside the resident ones: dropped unless committed
struct new_postings {
    rag_bm25_index* p = nullptr;
    ~new_postings() { if (p) bm25_compact_discard(p); }
};

// one compaction: the staging buffer and its carve, the row map's host side, and what was prepared beside the rows
struct compact_job {
    int keep;
    int64_t n0, tiles;                   // rows and 256-row tiles before
    bool move_tv;                        // the token-vector store's documents move with their rows
    dev_buf<char> ws;                    // tile_cnt [tiles] | tile_off [tiles] (its exclusive scan) | row_map [n0] (old row -> new row or -1) |
    int* tile_cnt;                       // src_rows [n_live] (new row -> old row) | data: one chunk of gathered rows
    int64_t *tile_off, *row_map;
    int32_t* src_rows;
    char* data;
    size_t data_bytes;
    std::vector<int64_t> off;            // host copy of tile_off
    int64_t n_live = 0, first_move = -1; // rows that stay; the first row of the first tile that loses one (rows before it do not move)
    new_postings np, np_sparse;
    tokvec_compact_plan tvp;
    bool ten = false, tok = false;       // the tenant table / the token store covered the rows and moved with them
};

static int compact_fail(rag_ctx* h, hipError_t e, const char* what) {
    h->err = std::string("compact: ") + what + ": " + hipGetErrorString(e);
    return RAG_ERR_HIP;
}

// the staging buffer: tile counts | tile offsets | row map | source rows | row data, within LIVE_STAGING_BYTES
// (the token-vector store's own maps are per document - new offsets and first source row, tokvec_compact_prepare - and count
// against the same bound)
static int compact_stage(rag_ctx* h, compact_job& c) {
    const int64_t n0 = c.n0, tiles = c.tiles;
    const size_t tv_bytes = c.move_tv ? stage_size((size_t)h->tv_docs_cap + 1, 8) + stage_size((size_t)h->tv_docs + 1, 8) : 0;
    const size_t map_bytes = stage_size(tiles, 4) + stage_size(tiles, 8) + stage_size(n0, 8) + stage_size(n0, 4);
    ARG_CHECK(h, map_bytes + tv_bytes + ((size_t)64 << 20) <= LIVE_STAGING_BYTES, "compact: the row map of this index exceeds the 1 GiB staging bound");
    c.data_bytes = std::min<size_t>((size_t)512 << 20, LIVE_STAGING_BYTES - map_bytes - tv_bytes);
    if (c.ws.alloc(h, map_bytes + c.data_bytes)) {
        (void)hipGetLastError();
        h->err = "compact: out of device memory for the staging buffer";
        return RAG_ERR_NOMEM;
    }
    char* p = c.ws;
    c.tile_cnt = stage_take<int>(p, tiles);
    c.tile_off = stage_take<int64_t>(p, tiles);
    c.row_map = stage_take<int64_t>(p, n0);
    c.src_rows = stage_take<int32_t>(p, n0);
    c.data = p;
    return RAG_OK;
}

// phase 1, the row map: live rows per tile, their exclusive scan on the host (tiles entries: 49K at 12.5M rows), the first tile
// that loses a row, then row_map and src_rows on the device
static int compact_row_map(rag_ctx* h, compact_job& c) {
    hipStream_t st = h->stream;
    const int64_t n0 = c.n0, tiles = c.tiles;
    hipLaunchKernelGGL(live_tile_count_kernel, dim3((unsigned)tiles), dim3(256), 0, st, h->vis, n0, c.tile_cnt);
    std::vector<int> cnt((size_t)tiles);
    hipError_t e = hipMemcpyAsync(cnt.data(), c.tile_cnt, (size_t)tiles * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return compact_fail(h, e, "tile counts");
    c.off.resize((size_t)tiles);
    for (int64_t t = 0; t < tiles; ++t) {
        c.off[(size_t)t] = c.n_live;
        c.n_live += cnt[(size_t)t];
        if (c.first_move < 0 && cnt[(size_t)t] < std::min<int64_t>(RAG_TILE, n0 - t * RAG_TILE)) c.first_move = t * RAG_TILE;
    }
    if (c.first_move < 0) c.first_move = n0;
    e = hipMemcpyAsync(c.tile_off, c.off.data(), (size_t)tiles * 8, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return compact_fail(h, e, "tile offsets");
    hipLaunchKernelGGL(live_row_map_kernel, dim3((unsigned)tiles), dim3(256), 0, st, h->vis, n0, c.tile_off, c.row_map, c.src_rows);
    return RAG_OK;
}

// live rows below row x: the scanned tile offsets + the live rows of x's own tile before it (at most 255 map entries)
static int compact_live_below(rag_ctx* h, const compact_job& c, int64_t x, int64_t* out) {
    *out = c.n_live;
    if (x >= c.n0) return RAG_OK;
    const int64_t t0 = x / RAG_TILE * RAG_TILE;
    int64_t part[RAG_TILE];
    if (x > t0) HIP_TRY(h, hipMemcpyAsync(part, c.row_map + t0, (size_t)(x - t0) * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *out = c.off[(size_t)(t0 / RAG_TILE)];
    for (int64_t i = 0; i < x - t0; ++i) *out += part[i] >= 0;
    return RAG_OK;
}

// one resident index (the BM25 or the learned-sparse postings) that describes the rows: remapped into `dst`
static int compact_remap_postings(rag_ctx* h, const compact_job& c, const rag_bm25_index* ix, bool compacted, new_postings& dst) {
    const int64_t covered = bm25_covered_docs(ix);
    if (ix == nullptr || compacted || covered > c.n0) return RAG_OK;
    int64_t base_live = 0, covered_live = 0;
    int rc;
    if ((rc = compact_live_below(h, c, bm25_base_docs(ix), &base_live))) return rc;
    if ((rc = compact_live_below(h, c, covered, &covered_live))) return rc;
    return bm25_compact_prepare(h, ix, c.row_map, base_live, covered_live, &dst.p);
}

// phase 2, what moves beside the rows: the postings of the rows that stay, under their new numbers, and the token-vector
// store's new offsets and per-document source map (from a host copy of the row map). Everything is allocated and built here,
// nothing is replaced yet.
static int compact_prepare(rag_ctx* h, compact_job& c) {
    int rc;
    if (c.keep >= LIVE_KEEP_BM25 && (rc = compact_remap_postings(h, c, h->bm25, h->bm25_compacted, c.np))) return rc;
    if (c.keep == LIVE_KEEP_RESIDENT && (rc = compact_remap_postings(h, c, h->sparse, h->sparse_compacted, c.np_sparse))) return rc;
    if (c.move_tv) {
        std::vector<int64_t> map_h((size_t)c.n0);
        HIP_TRY(h, hipMemcpyAsync(map_h.data(), c.row_map, (size_t)c.n0 * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if ((rc = tokvec_compact_prepare(h, map_h.data(), c.n0, c.data_bytes, &c.tvp))) return rc;
    }
    return RAG_OK;
}

// gathers `bytes` of rows (row_bytes each, sources src_rows) into the staging buffer, in the widest word that divides a row
template <class W>
static void gather_words(const void* plane, size_t row_bytes, const int32_t* src_rows, size_t bytes, char* stage, hipStream_t st) {
    const uint32_t rw = (uint32_t)(row_bytes / sizeof(W)), total = (uint32_t)(bytes / sizeof(W));
    hipLaunchKernelGGL(live_compact_gather_kernel<W>, dim3(grid_for(total)), dim3(256), 0, st, (const W*)plane, rw, src_rows, total, (W*)stage);
}
static void gather_rows(const void* plane, size_t row_bytes, const int32_t* src_rows, size_t bytes, char* stage, hipStream_t st) {
    if (row_bytes % 16 == 0) gather_words<uint4>(plane, row_bytes, src_rows, bytes, stage, st);
    else if (row_bytes % 8 == 0) gather_words<uint2>(plane, row_bytes, src_rows, bytes, stage, st);
    else if (row_bytes % 4 == 0) gather_words<uint32_t>(plane, row_bytes, src_rows, bytes, stage, st);
    else if (row_bytes % 2 == 0) gather_words<uint16_t>(plane, row_bytes, src_rows, bytes, stage, st);
    else gather_words<uint8_t>(plane, row_bytes, src_rows, bytes, stage, st);      // a row of L bytes: any alignment
}

// phase 3: every plane that covers the rows, chunk by chunk of destination rows through the staging buffer; then the fp16
// padding, the row map for the caller and the token-vector rows, and the one wait for all of it. vis does not move (it is
// dropped); the token planes move when the store is aligned with the index; any other plane when it has room for the rows.
static int compact_move_planes(rag_ctx* h, compact_job& c, int64_t* row_map_out) {
    hipStream_t st = h->stream;
    const int64_t n0 = c.n0, n_live = c.n_live;
    c.ten = h->tenants && (int64_t)h->tenants.size() >= n0;
    c.tok = tokens_aligned(h, n0);
    struct plane { char* p; size_t row_bytes; };
    std::vector<plane> planes;
    for_each_row_plane(h, [&](int id, auto mp, int64_t width) {
        const auto& b = h->*mp;
        const bool token = id == PLANE_TOK || id == PLANE_TOK_HI || id == PLANE_TOK_LEN;
        if (b && id != PLANE_VIS && (token ? c.tok : plane_rows(b, width) >= n0)) planes.push_back({(char*)b.get(), (size_t)width * sizeof(*b.get())});
        return RAG_OK;
    });
    hipError_t e = hipSuccess;
    for (const plane& pl : planes) {
        const int64_t chunk = std::max<int64_t>(1, (int64_t)(c.data_bytes / pl.row_bytes));
        for (int64_t d0 = c.first_move; d0 < n_live; d0 += chunk) {
            const size_t bytes = (size_t)std::min(chunk, n_live - d0) * pl.row_bytes;
            gather_rows(pl.p, pl.row_bytes, c.src_rows + d0, bytes, c.data, st);
            e = hipMemcpyAsync(pl.p + (size_t)d0 * pl.row_bytes, c.data, bytes, hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) return compact_fail(h, e, "row copy");
        }
    }
    // the rows past the new end are tile padding of the fp16 operand again: zero
    if (n0 > n_live) e = hipMemsetAsync(h->emb16 + (size_t)n_live * h->dim_pad, 0, (size_t)(n0 - n_live) * h->dim_pad * 2, st);
    if (e == hipSuccess && row_map_out) e = hipMemcpyAsync(row_map_out, c.row_map, (size_t)n0 * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return compact_fail(h, e, "finish");
    if (int rc = tokvec_compact_commit(h, &c.tvp, c.data, st)) return rc;      // (the staging buffer is free again: same stream)
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return compact_fail(h, e, "finish");
    return RAG_OK;
}

// phase 4: the new row count, no deleted rows, the prepared postings swapped in (or the resident ones stale), new tenant tiles
static int compact_publish(rag_ctx* h, compact_job& c) {
    const int64_t n_live = c.n_live;
    c.ws.reset();
    h->n_rows = n_live;
    if (c.tok) h->tok_rows = n_live;
    h->vis.reset();
    h->n_deleted = 0;
    if (c.np_sparse.p) {                     // rag_index_compact_live: renumbered with the rows, staleness left as it was
        bm25_compact_commit(&h->sparse, c.np_sparse.p);
        c.np_sparse.p = nullptr;
    } else {                                 // not renumbered: a reload makes them current
        h->sparse_stale = true;
        h->sparse_compacted = true;
    }
    if (h->tv_docs_cap > 0 && !c.move_tv) h->tv_stale = true;    // nor are the resident token vectors, unless they moved (tokvec.hip)
    if (c.np.p) {
        bm25_compact_commit(&h->bm25, c.np.p);
        c.np.p = nullptr;
    } else {
        h->bm25_stale = true;
        h->bm25_compacted = true;
    }
    live_rows_changed(h);
    if (c.ten) {                             // tenant tile lists of the new row numbers
        std::vector<int32_t> t((size_t)n_live);
        if (n_live > 0) HIP_TRY(h, hipMemcpy(t.data(), h->tenants, (size_t)n_live * 4, hipMemcpyDeviceToHost));
        if (int rc = dense_build_tenant_tiles(h, n_live > 0 ? t.data() : nullptr, n_live)) return rc;
        h->tenant_rows = n_live;
    }
    return RAG_OK;
}

static int live_compact(rag_ctx* h, int64_t* row_map_out, int64_t* n_rows_out, int keep) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    int rc = live_begin(h);
    if (rc) return rc;
    const int64_t n0 = h->index_loaded ? h->n_rows : 0;
    if (h->n_deleted == 0 || h->vis == nullptr) {
        if (row_map_out)
            for (int64_t i = 0; i < n0; ++i) row_map_out[i] = i;
        if (n_rows_out) *n_rows_out = n0;
        return RAG_OK;
    }
    if (!ids_cover(h, n0)) {
        h->err = "compact: the stored ids do not cover the index rows";
        return RAG_ERR_STATE;
    }
    // an enabled id map is rebuilt from the moved id column; an implicit-id index gets its first table here, before any row moves
    idmap_table map;
    if (h->idmap.on && !h->idmap_keys && (rc = idmap_prepare(h, std::max(emb32_rows(h), n0), &map))) return rc;
    // doc ids never change: an implicit-id index stores its ids before any row moves
    if (!h->ids) {
        if ((rc = h->ids.alloc(h, (size_t)std::max(emb32_rows(h), n0)))) return rc;
        hipLaunchKernelGGL(live_iota_ids_kernel, dim3(grid_for(n0)), dim3(256), 0, h->stream, h->ids, h->id_base, n0);
        HIP_TRY(h, hipGetLastError());
    }
    compact_job c{keep, n0, (n0 + RAG_TILE - 1) / RAG_TILE, keep == LIVE_KEEP_RESIDENT && h->tv_docs_cap > 0 && !h->tv_stale};
    if ((rc = compact_stage(h, c))) return rc;
    if ((rc = compact_row_map(h, c))) return rc;
    if ((rc = compact_prepare(h, c))) return rc;
    if ((rc = compact_move_planes(h, c, row_map_out))) return rc;
    if ((rc = compact_publish(h, c))) return rc;
    if ((rc = idmap_rebuild(h, &map))) return rc;
    if (n_rows_out) *n_rows_out = c.n_live;
    return RAG_OK;
}

extern "C" {

int rag_index_insert_host(rag_handle_t h, const rag_row_block* rb, int64_t* first_row_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, rb != nullptr, "insert: null row block");
    ARG_CHECK(h, rb->n >= 0 && (rb->n == 0 || rb->emb != nullptr), "insert: need n >= 0 and emb[n][dim]");
    int rc = live_begin(h);
    if (rc) return rc;
    const int64_t n0 = h->index_loaded ? h->n_rows : 0;
    insert_job in{rb, n0, rb->n, n0 + rb->n, h->tok != nullptr, h->tok != nullptr && h->tok_hi != nullptr};
    if ((rc = insert_check(h, in))) return rc;
    if (first_row_out) *first_row_out = in.n0;
    if (in.n == 0) return RAG_OK;
    if ((rc = insert_convert(h, in))) return rc;
    rag_device_mem g;                    // the grown planes: dropped whole unless moved into the handle
    if ((rc = insert_grow(h, in, &g))) return rc;
    // an enabled id map that has no room for the block (or no table yet) gets its new table now, while nothing has changed
    idmap_table map;
    const int64_t cap_after = grow_cap(std::max(emb32_rows(h), in.n0), in.need);
    const bool map_rebuild = idmap_must_rebuild(h, in.n, cap_after, rb->ids != nullptr || h->ids != nullptr);
    if (map_rebuild && (rc = idmap_prepare(h, cap_after, &map))) return rc;
    if ((rc = insert_start_index(h))) return rc;
    if ((rc = insert_move_in(h, in, &g))) return rc;
    if ((rc = insert_write(h, in))) return rc;
    return map_rebuild ? idmap_rebuild(h, &map) : idmap_insert_rows(h, in.n0, in.n, in.ids_ascend);
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
    if (tenant >= 0 && !tenants_cover(h, h->n_rows)) {
        h->err = "delete: the tenant table is stale (rows were appended after rag_index_set_tenants_host)";
        return RAG_ERR_STATE;
    }
    if (!ids_cover(h, h->n_rows)) {
        h->err = "delete: the stored ids do not cover the index rows";
        return RAG_ERR_STATE;
    }
    std::vector<int64_t> set(ids, ids + n_ids);
    std::sort(set.begin(), set.end());
    set.erase(std::unique(set.begin(), set.end()), set.end());
    const bool created = h->vis == nullptr;
    if (created && (rc = live_vis_extend(h, 0, h->n_rows))) return rc;
    int64_t n_del = 0;
    const int64_t* set_dev = nullptr;
    if ((rc = id_set_apply(h, set, tenant, 1, &n_del, &set_dev))) return rc;
    if (n_del > 0 && (rc = idmap_erase_deleted(h, set_dev, (int)set.size()))) return rc;
    if (created && n_del == 0) h->vis.reset();       // nothing deleted: keep the searches on their unfiltered path
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

int rag_index_compact(rag_handle_t h, int64_t* row_map_out, int64_t* n_rows_out) { return live_compact(h, row_map_out, n_rows_out, LIVE_KEEP_NONE); }
int rag_index_compact_bm25(rag_handle_t h, int64_t* row_map_out, int64_t* n_rows_out) { return live_compact(h, row_map_out, n_rows_out, LIVE_KEEP_BM25); }
int rag_index_compact_live(rag_handle_t h, int64_t* row_map_out, int64_t* n_rows_out) { return live_compact(h, row_map_out, n_rows_out, LIVE_KEEP_RESIDENT); }

}  // extern "C"
