// Device id-to-row map (include/rag_hip.h: rag_index_id_map, rag_index_rows_of_ids_dev / _host, rag_index_id_map_info): "which of my
// rows has this id?" for an index with explicit ids, without a pass over the id column. A row shard asks it for every candidate
// slot of every batch (pipeline.hip m3_score_ids_dev); an index with implicit ids answers by arithmetic and keeps no table.
//
// Representation: open addressing with linear probing over two planes in HBM, keys int64 [slots] and rows int32 [slots].
//   home(id) = ((uint64)id * 0x9E3779B97F4A7C15) >> (64 - log2(slots)),   slots a power of two >= 2 * the row capacity
// so the load (live keys + tombstones) stays at or below 1/2 and every probe chain ends at an unused slot. Keys are ids >= 0; an
// unused slot holds IDMAP_EMPTY. A slot is claimed by a 64-bit compare-and-swap on its key, then its row is written: which slot a
// key gets depends on the order of the atomics, what a lookup returns does not (a key is in exactly one slot of its chain).
// Erasing leaves a tombstone - the key stays, the row becomes -1 - so chains stay intact; inserting that id again finds its key
// and takes the slot back. Tombstones go when the table is rebuilt: by every compaction, by rag_index_set_ids_host, and by the
// insert that would take live keys + tombstones past slots / 2 or that grows the row capacity.
// Writes and lookups never overlap: writes are host calls that wait for queued *_dev work, lookups are ordered on their stream.
#include "common.h"

#include <algorithm>

enum { ST_ERR_KIND, ST_ERR_ID, ST_PROBE, ST_COUNT, ST_NOT_ASC };       // words of rag_index_mem::idmap_stat
enum { IDMAP_NEGATIVE = 1, IDMAP_DUPLICATE = 2 };

struct idmap_view { int64_t* keys; int32_t* rows; uint64_t mask; int shift; };

__device__ __forceinline__ uint64_t idmap_home(int64_t id, int shift) { return ((uint64_t)id * 0x9E3779B97F4A7C15ull) >> shift; }

// the slot that holds `id`, or mask + 1 when the chain ends without it
__device__ __forceinline__ uint64_t idmap_find(const idmap_view& m, int64_t id) {
    uint64_t s = idmap_home(id, m.shift);
    for (uint64_t step = 0; step <= m.mask; ++step) {
        const int64_t k = m.keys[s];
        if (k == id) return s;
        if (k == IDMAP_EMPTY) break;
        s = (s + 1) & m.mask;
    }
    return m.mask + 1;
}

__device__ __forceinline__ void idmap_refuse(unsigned long long* stat, int kind, int64_t id) {
    if (atomicCAS(&stat[ST_ERR_KIND], 0ull, (unsigned long long)kind) == 0ull) stat[ST_ERR_ID] = (unsigned long long)id;
}

__global__ __launch_bounds__(256) void idmap_clear_kernel(idmap_view m) {
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s <= m.mask; s += (uint64_t)gridDim.x * 256) {
        m.keys[s] = IDMAP_EMPTY;
        m.rows[s] = -1;
    }
}

// live rows [first, first + n) into the table. fresh: the table held none of these rows' keys before this launch (a build), so a
// key that is found there is a duplicate id; otherwise (an insert of ids that are not live) it is a tombstone, taken back and counted
__global__ __launch_bounds__(256) void idmap_put_kernel(idmap_view m, const int64_t* __restrict__ ids, const int32_t* __restrict__ vis,
                                                         int64_t first, int64_t n, int fresh, unsigned long long* __restrict__ stat) {
    int longest = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t row = first + i;
        if (vis != nullptr && vis[row] == RAG_DEAD_ROW) continue;
        const int64_t id = ids[row];
        if (id < 0) {
            idmap_refuse(stat, IDMAP_NEGATIVE, id);
            continue;
        }
        uint64_t s = idmap_home(id, m.shift);
        for (uint64_t step = 0; step <= m.mask; ++step) {
            const int64_t prev = (int64_t)atomicCAS(reinterpret_cast<unsigned long long*>(&m.keys[s]), (unsigned long long)IDMAP_EMPTY,
                                                    (unsigned long long)id);
            if (prev == IDMAP_EMPTY) {
                m.rows[s] = (int32_t)row;
                longest = max(longest, (int)step + 1);
                break;
            }
            if (prev == id) {
                if (!fresh && m.rows[s] < 0) {
                    m.rows[s] = (int32_t)row;
                    atomicAdd(&stat[ST_COUNT], 1ull);
                    longest = max(longest, (int)step + 1);
                } else {
                    idmap_refuse(stat, IDMAP_DUPLICATE, id);
                }
                break;
            }
            s = (s + 1) & m.mask;
        }
    }
    for (int o = 32; o > 0; o >>= 1) longest = max(longest, __shfl_xor(longest, o));
    if ((threadIdx.x & 63) == 0 && longest > 0) atomicMax(&stat[ST_PROBE], (unsigned long long)longest);
}

// do the ids of the live rows ascend strictly with the rows? Each live row against the next live row.
__global__ __launch_bounds__(256) void idmap_order_kernel(const int64_t* __restrict__ ids, const int32_t* __restrict__ vis, int64_t n,
                                                           unsigned long long* __restrict__ stat) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        if (vis != nullptr && vis[r] == RAG_DEAD_ROW) continue;
        int64_t nx = r + 1;
        while (vis != nullptr && nx < n && vis[nx] == RAG_DEAD_ROW) ++nx;
        if (nx < n && ids[r] >= ids[nx]) stat[ST_NOT_ASC] = 1ull;
    }
}

// an inserted block [first, ...) that ascends in itself: its first id against the last live row before it (one wave, walking back)
__global__ __launch_bounds__(64) void idmap_join_kernel(const int64_t* __restrict__ ids, const int32_t* __restrict__ vis, int64_t first,
                                                         unsigned long long* __restrict__ stat) {
    for (int64_t hi = first; hi > 0; hi -= 64) {
        const int64_t r = hi - 1 - threadIdx.x;
        const bool live = r >= 0 && (vis == nullptr || vis[r] != RAG_DEAD_ROW);
        const unsigned long long b = __ballot(live);
        if (b == 0ull) continue;
        const int lane = __ffsll((long long)b) - 1;          // the lowest lane holds the highest row
        if ((int)threadIdx.x == lane && ids[r] >= ids[first]) stat[ST_NOT_ASC] = 1ull;
        return;
    }
}

// the ids of a delete's set whose row the delete marked: their slots become tombstones
__global__ __launch_bounds__(256) void idmap_erase_kernel(idmap_view m, const int64_t* __restrict__ set, int n_set,
                                                           const int32_t* __restrict__ vis, unsigned long long* __restrict__ stat) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_set || set[i] < 0) return;
    const uint64_t s = idmap_find(m, set[i]);
    if (s > m.mask) return;
    const int32_t row = m.rows[s];
    if (row < 0 || vis[row] != RAG_DEAD_ROW) return;
    m.rows[s] = -1;
    atomicAdd(&stat[ST_COUNT], 1ull);
}

// one lane per id: the row the map holds for it, -1 for an unknown, an erased or a negative id. owned (may be null): plane 0 of a
// partial block of m3_score_ids_dev, 1 where the row is >= 0
__global__ __launch_bounds__(256) void idmap_lookup_kernel(idmap_view m, const int64_t* __restrict__ ids, int64_t n,
                                                            int32_t* __restrict__ rows_out, int64_t* __restrict__ owned) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t id = ids[i];
    int32_t row = -1;
    if (id >= 0) {
        const uint64_t s = idmap_find(m, id);
        if (s <= m.mask) row = m.rows[s];
    }
    rows_out[i] = row;
    if (owned != nullptr) owned[i] = row >= 0 ? 1 : 0;
}

// the same on implicit ids: id_base + row, and the deleted-row check
__global__ __launch_bounds__(256) void idmap_implicit_kernel(int64_t id_base, int64_t n_rows, const int32_t* __restrict__ vis,
                                                              const int64_t* __restrict__ ids, int64_t n, int32_t* __restrict__ rows_out,
                                                              int64_t* __restrict__ owned) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t id = ids[i];
    int32_t row = -1;
    if (id >= 0 && id >= id_base && id - id_base < n_rows && (vis == nullptr || vis[id - id_base] != RAG_DEAD_ROW)) row = (int32_t)(id - id_base);
    rows_out[i] = row;
    if (owned != nullptr) owned[i] = row >= 0 ? 1 : 0;
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static int grid_for(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 8192)); }

static idmap_view view_of(const rag_ctx* h) {
    const uint64_t slots = (uint64_t)h->idmap.slots;
    return {h->idmap_keys.get(), h->idmap_rows.get(), slots - 1, 64 - __builtin_ctzll(slots)};
}

int64_t idmap_slots_for(int64_t row_capacity) {
    int64_t s = 128;
    while (s < 2 * row_capacity) s <<= 1;
    return s;
}

bool idmap_must_rebuild(const rag_ctx* h, int64_t n_new, int64_t row_capacity_after, bool explicit_after) {
    const auto& m = h->idmap;
    if (!m.on || !explicit_after) return false;
    return h->idmap_keys == nullptr || m.entries + m.tombstones + n_new > m.slots / 2 || idmap_slots_for(row_capacity_after) > m.slots;
}

int idmap_prepare(rag_ctx* h, int64_t row_capacity, idmap_table* t) {
    const int64_t slots = idmap_slots_for(std::max(row_capacity, h->n_rows));
    bool ok = t->keys.alloc(h, (size_t)slots) == RAG_OK && t->rows.alloc(h, (size_t)slots) == RAG_OK;
    if (ok && !h->idmap_stat) ok = h->idmap_stat.alloc(h, IDMAP_STAT_WORDS) == RAG_OK;
    if (!ok) {
        (void)hipGetLastError();
        t->keys.reset();
        t->rows.reset();
        h->err = "id map: out of device memory for a table of " + std::to_string(slots) + " slots";
        return RAG_ERR_NOMEM;
    }
    t->slots = slots;
    return RAG_OK;
}

void idmap_drop(rag_ctx* h) {
    h->idmap_keys.reset();
    h->idmap_rows.reset();
    h->idmap_stat.reset();
    h->idmap = {};
}

static int stat_clear(rag_ctx* h) {
    HIP_TRY(h, hipMemsetAsync(h->idmap_stat, 0, IDMAP_STAT_WORDS * sizeof(unsigned long long), h->stream));
    return RAG_OK;
}
static int stat_read(rag_ctx* h, unsigned long long* out) {
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out, h->idmap_stat, IDMAP_STAT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RAG_OK;
}

int idmap_rebuild(rag_ctx* h, idmap_table* t) {
    auto& m = h->idmap;
    if (!m.on) return RAG_OK;
    if (!h->ids) {                               // implicit ids: lookups are arithmetic, and such ids ascend
        const int64_t rebuilds = m.rebuilds;
        idmap_drop(h);
        m.on = true;
        m.rebuilds = rebuilds;
        return RAG_OK;
    }
    if (t != nullptr && t->keys) {
        h->idmap_keys = std::move(t->keys);
        h->idmap_rows = std::move(t->rows);
        m.slots = t->slots;
    }
    if (!h->idmap_keys || !h->idmap_stat || m.slots < idmap_slots_for(h->n_rows)) {
        idmap_drop(h);
        h->err = "id map: no table for the rows of the index (the map is disabled)";
        return RAG_ERR_STATE;
    }
    const int64_t n = h->n_rows;
    const idmap_view v = view_of(h);
    if (int rc = stat_clear(h)) return rc;
    hipLaunchKernelGGL(idmap_clear_kernel, dim3(grid_for(m.slots)), dim3(256), 0, h->stream, v);
    if (n > 0) {
        hipLaunchKernelGGL(idmap_put_kernel, dim3(grid_for(n)), dim3(256), 0, h->stream, v, h->ids.get(), h->vis.get(), (int64_t)0, n, 1, h->idmap_stat.get());
        hipLaunchKernelGGL(idmap_order_kernel, dim3(grid_for(n)), dim3(256), 0, h->stream, h->ids.get(), h->vis.get(), n, h->idmap_stat.get());
    }
    unsigned long long st[IDMAP_STAT_WORDS];
    if (int rc = stat_read(h, st)) return rc;
    if (st[ST_ERR_KIND] != 0) {
        idmap_drop(h);
        h->err = std::string("bad argument: id map: ") + (st[ST_ERR_KIND] == IDMAP_NEGATIVE ? "negative id " : "duplicate live id ") +
                 std::to_string((int64_t)st[ST_ERR_ID]) + " (the map is disabled)";
        return RAG_ERR_ARG;
    }
    m.entries = n - h->n_deleted;
    m.tombstones = 0;
    m.longest_probe = (int64_t)st[ST_PROBE];
    m.ascending = st[ST_NOT_ASC] == 0;
    m.rebuilds++;
    return RAG_OK;
}

int idmap_insert_rows(rag_ctx* h, int64_t first_row, int64_t n, bool block_ascending) {
    auto& m = h->idmap;
    if (!m.on || !h->idmap_keys || !h->ids || n <= 0) return RAG_OK;
    if (int rc = stat_clear(h)) return rc;
    hipLaunchKernelGGL(idmap_put_kernel, dim3(grid_for(n)), dim3(256), 0, h->stream, view_of(h), h->ids.get(), h->vis.get(), first_row, n, 0,
                       h->idmap_stat.get());
    if (m.ascending && block_ascending && first_row > 0)
        hipLaunchKernelGGL(idmap_join_kernel, dim3(1), dim3(64), 0, h->stream, h->ids.get(), h->vis.get(), first_row, h->idmap_stat.get());
    unsigned long long st[IDMAP_STAT_WORDS];
    if (int rc = stat_read(h, st)) return rc;
    if (st[ST_ERR_KIND] != 0) {                  // (the insert checked both before it committed: not reached)
        idmap_drop(h);
        h->err = "id map: id " + std::to_string((int64_t)st[ST_ERR_ID]) + " of the inserted block is negative or live (the map is disabled)";
        return RAG_ERR_STATE;
    }
    const int64_t reused = (int64_t)st[ST_COUNT];
    m.entries += n;
    m.tombstones -= reused;
    m.longest_probe = (int64_t)st[ST_PROBE];
    m.ascending = m.ascending && block_ascending && st[ST_NOT_ASC] == 0;
    return RAG_OK;
}

int idmap_erase_deleted(rag_ctx* h, const int64_t* set_dev, int n_set) {
    auto& m = h->idmap;
    if (!m.on || !h->idmap_keys || n_set <= 0 || !h->vis) return RAG_OK;
    if (int rc = stat_clear(h)) return rc;
    hipLaunchKernelGGL(idmap_erase_kernel, dim3((unsigned)((n_set + 255) / 256)), dim3(256), 0, h->stream, view_of(h), set_dev, n_set, h->vis.get(),
                       h->idmap_stat.get());
    unsigned long long st[IDMAP_STAT_WORDS];
    if (int rc = stat_read(h, st)) return rc;
    m.entries -= (int64_t)st[ST_COUNT];
    m.tombstones += (int64_t)st[ST_COUNT];
    return RAG_OK;
}

int idmap_rows_of_ids(rag_ctx* h, const int64_t* ids_dev, int64_t n, int32_t* rows_out, int64_t* owned, hipStream_t st) {
    if (n <= 0) return RAG_OK;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (!h->ids) {
        hipLaunchKernelGGL(idmap_implicit_kernel, grid, dim3(256), 0, st, h->id_base, h->n_rows, h->vis.get(), ids_dev, n, rows_out, owned);
    } else {
        if (!h->idmap.on || !h->idmap_keys) {
            h->err = "rows_of_ids: the index has explicit ids and no id map (rag_index_id_map)";
            return RAG_ERR_STATE;
        }
        hipLaunchKernelGGL(idmap_lookup_kernel, grid, dim3(256), 0, st, view_of(h), ids_dev, n, rows_out, owned);
    }
    return launch_status(h);
}

int idmap_shard_gate(rag_ctx* h, const char* who, const char* refusal_without_map) {
    if (!h->ids) return RAG_OK;
    if (!h->idmap.on) {
        h->err = std::string(who) + refusal_without_map;
        return RAG_ERR_STATE;
    }
    if (!h->idmap.ascending) {
        h->err = std::string(who) + ": the explicit ids of the live rows do not ascend with the rows (rag_index_id_map_info ids_ascending): "
                 "the merges over shards break ties by lower id, the local searches by lower row";
        return RAG_ERR_STATE;
    }
    return RAG_OK;
}

extern "C" {

int rag_index_id_map(rag_handle_t h, int enable) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = host_after_dev(h)) return rc;
    if (!enable) {
        idmap_drop(h);
        return RAG_OK;
    }
    const int64_t n = h->index_loaded ? h->n_rows : 0;
    if (!ids_cover(h, n)) {
        h->err = "id_map: the stored ids do not cover the index rows";
        return RAG_ERR_STATE;
    }
    idmap_table t;
    if (h->ids)
        if (int rc = idmap_prepare(h, std::max(emb32_rows(h), n), &t)) return rc;
    h->idmap.on = true;
    if (int rc = idmap_rebuild(h, &t)) return rc;
    h->idmap.rebuilds = 0;
    return RAG_OK;
}

int rag_index_rows_of_ids_dev(rag_handle_t h, const int64_t* ids_dev, int64_t n, int32_t* rows_out_dev, void* stream) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, n >= 0 && (n == 0 || (ids_dev && rows_out_dev)), "rows_of_ids: need n >= 0 and both arrays");
    HIP_TRY(h, hipSetDevice(h->device));
    h->dev_pending = true;
    return idmap_rows_of_ids(h, ids_dev, n, rows_out_dev, nullptr, (hipStream_t)stream);
}

int rag_index_rows_of_ids_host(rag_handle_t h, const int64_t* ids, int64_t n, int32_t* rows_out) {
    if (!h) return RAG_ERR_ARG;
    LOCK(h);
    ARG_CHECK(h, n >= 0 && n < (int64_t)0x7fffffff && (n == 0 || (ids && rows_out)), "rows_of_ids: need 0 <= n < 2^31 and both arrays");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = host_after_dev(h)) return rc;
    if (n == 0) return RAG_OK;
    if (int rc = stage_reserve(h, stage_size((size_t)n, 8) + stage_size((size_t)n, 4))) return rc;
    char* p = h->stage;
    int64_t* ids_dev = stage_take<int64_t>(p, (size_t)n);
    int32_t* rows_dev = stage_take<int32_t>(p, (size_t)n);
    HIP_TRY(h, hipMemcpyAsync(ids_dev, ids, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    if (int rc = idmap_rows_of_ids(h, ids_dev, n, rows_dev, nullptr, h->stream)) return rc;
    HIP_TRY(h, hipMemcpyAsync(rows_out, rows_dev, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RAG_OK;
}

int rag_index_id_map_info(rag_handle_t h, rag_id_map_info* out) {
    if (!h || !out) return RAG_ERR_ARG;
    LOCK(h);
    const auto& m = h->idmap;
    *out = {};
    out->enabled = m.on ? 1 : 0;
    out->slots = m.slots;
    out->entries = m.entries;
    out->tombstones = m.tombstones;
    out->longest_probe = m.longest_probe;
    out->hbm_bytes = m.slots * (int64_t)(sizeof(int64_t) + sizeof(int32_t));
    out->ids_ascending = m.on && m.ascending ? 1 : 0;
    out->rebuilds = m.rebuilds;
    return RAG_OK;
}

}  // extern "C"
