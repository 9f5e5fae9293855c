// Retrieve + rerank as ONE device-resident call (BASELINE.json configs[3]: "hybrid top-100 -> ms-marco-MiniLM-L-6
// cross-encoder rerank -> top-20"): the composition the reference performs across
//   HybridRetriever.retrieve            /root/reference/rag/retrieval.py:122-212
//   CrossEncoderReranker.rerank         /root/reference/rag/reranker.py:320-384   (pairs [query, content] :346-352,
//                                        raw logits :355, sigmoid :359, sort desc by sigmoid, [:top_k] :372-376)
// with the passages' token ids resident in HBM next to their embeddings ("token store"), so
// between the query arriving and the top-k leaving nothing crosses PCIe.
//   1. candidates: dense top-pool (mode 0) or dense + BM25 + RRF -> top-pool (mode 1)
//   2. ce_build_pairs_kernel: [CLS] query [SEP] passage [SEP], token_type 0 | 1, truncated 'longest_first' to L_pair
//      (or the RoBERTa layout [CLS] query [SEP] [SEP] passage [SEP], all type 0: rag_ce_set_pair_format)
//   3. ce_score (cross_encoder.hip)
//   4. rerank_topk_kernel: sigmoid in float64, stable order (score desc, candidate order on ties), top-k
#include "common.h"

#include <cmath>

// The two candidate legs of the hybrid search: dense top-pool into lists[0], BM25 top-pool into lists[1] ([2][Q][pool]).
// They are independent: the BM25 leg runs on a side stream, forked from and joined back into the caller's stream by events.
// For a handful of queries both legs are latency-bound (one query: 0.6 ms of HBM-bound scan beside 0.2 ms of BM25 launches that
// occupy a quarter of the CUs: 0.99 -> 0.80 ms). Large batches (r2 kept them in line) gain less - the dense GEMM's 128-KiB
// workgroups leave room for ONE 20-KiB BM25 workgroup per CU - but the BM25 stages fill the thin opening stages, selects and
// the rescoring of the dense leg: 1024-query hybrid batches 6.85 -> 6.58 ms on one box (A/B by option fork_max_q).
// Option no_fork keeps the legs in line always; fork_max_q lowers the largest batch that forks.
// qweights_dev != null: the second leg is the learned-sparse index (rag_hybrid_sparse_rrf*_dev and the maxsim / m3 composites). Either
// keyword leg takes the call's per-query tenants, as the dense leg does.
#define RAG_FORK_MAX_Q 4096
int hybrid_legs(rag_ctx* h, const float* q_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev, int Q, int pool, int tenant,
                int64_t* lists_dev, double* scores_ws_dev, hipStream_t st, id_space ids, query_tenants qt, const float* qweights_dev) {
    int64_t* const bm_ids = lists_dev + (size_t)Q * pool;
    auto keyword_leg = [&](double* scores, hipStream_t s) -> int {
        if (qweights_dev != nullptr)
            return sparse_topk_dev(h, term_ptr_dev, terms_dev, qweights_dev, Q, pool, tenant, bm_ids, nullptr, scores, s, ids, qt);
        return bm25_topk_dev(h, term_ptr_dev, terms_dev, Q, pool, tenant, bm_ids, nullptr, scores, nullptr, s, ids, qt);
    };
    const int fork_max = h->opt.fork_max_q > 0 ? h->opt.fork_max_q : RAG_FORK_MAX_Q;
    if (Q > fork_max || h->opt.no_fork) {
        int rc = dense_search(h, q_dev, Q, pool, tenant, lists_dev, nullptr, scores_ws_dev, st, ids, qt);
        if (rc) return rc;
        return keyword_leg(scores_ws_dev, st);
    }
    if (!h->side_stream) {
        HIP_TRY(h, hipStreamCreateWithFlags(&h->side_stream, hipStreamNonBlocking));
        HIP_TRY(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
        HIP_TRY(h, hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    }
    const size_t need = (size_t)Q * pool;
    if (int rc = h->side_scores.reserve(h, std::max(need, (size_t)RAG_FORK_MAX_Q * RAG_MAX_K))) return rc;
    // inputs are ready wherever the caller's stream is now (the device copy of per-query tenants among them: written on st before this)
    HIP_TRY(h, hipEventRecord(h->ev_fork, st));
    HIP_TRY(h, hipStreamWaitEvent(h->side_stream, h->ev_fork, 0));
    int rc = keyword_leg(h->side_scores, h->side_stream);
    // the join is recorded and waited for even if a leg failed to launch: the caller's stream must never run ahead of the side stream
    HIP_TRY(h, hipEventRecord(h->ev_join, h->side_stream));
    const int rc2 = dense_search(h, q_dev, Q, pool, tenant, lists_dev, nullptr, scores_ws_dev, st, ids, qt);
    HIP_TRY(h, hipStreamWaitEvent(st, h->ev_join, 0));
    return rc ? rc : rc2;
}

// int32 token ids -> the 16-bit resident store (WordPiece vocabularies have < 65536 entries: 30522 for the MiniLM
// checkpoints); ids outside [0, 65535] are flagged
__global__ void tokens_narrow_kernel(const int32_t* __restrict__ in, uint16_t* __restrict__ out, int64_t n, int* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t v = in[i];
    if (v < 0 || v > 65535) atomicAdd(bad, 1);
    out[i] = (uint16_t)v;
}

// the same into a 24-bit store (rag_tokens_load_wide_host / rag_tokens_reserve_wide, id_bits = 24: XLM-R's vocabulary has
// 250,002 entries): the low half into the uint16 plane, bits 16-23 into a byte plane; ids outside [0, 16777215] are flagged
__global__ void tokens_narrow_wide_kernel(const int32_t* __restrict__ in, uint16_t* __restrict__ out, uint8_t* __restrict__ out_hi,
                                          int64_t n, int* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t v = in[i];
    if (v < 0 || v > 0xFFFFFF) atomicAdd(bad, 1);
    out[i] = (uint16_t)v;
    out_hi[i] = (uint8_t)(v >> 16);
}

// n ids at in -> store slots [at, at + n): both planes of a wide store, the one plane of a narrow one
static void tokens_narrow(rag_ctx* h, const int32_t* in, int64_t at, int64_t n, int* bad, hipStream_t st) {
    const dim3 grid((unsigned)((n + 255) / 256));
    if (h->tok_hi) hipLaunchKernelGGL(tokens_narrow_wide_kernel, grid, dim3(256), 0, st, in, h->tok + at, h->tok_hi + at, n, bad);
    else hipLaunchKernelGGL(tokens_narrow_kernel, grid, dim3(256), 0, st, in, h->tok + at, n, bad);
}
static const char* tokens_range_msg(const rag_ctx* h, bool append) {
    if (h->tok_hi) return append ? "tokens_append: token ids must be in [0, 16777215]" : "tokens_load: token ids must be in [0, 16777215]";
    return append ? "tokens_append: token ids must be in [0, 65535]" : "tokens_load: token ids must be in [0, 65535]";
}
static void tokens_drop(rag_ctx* h) {
    h->tok.reset();
    h->tok_hi.reset();
    h->tok_len.reset();
    h->tok_rows = 0;
}
// a load or a reserve that fails leaves no store behind: a half-built one would read as a reservation (tok_cap_rows)
struct tokens_pending { rag_ctx* h; bool done = false; ~tokens_pending() { if (!done) tokens_drop(h); } };

// The token store is kept as uint16: 2 B per token (51 GB for 100M x 256-token passages replicated per GPU, the budget of
// SURVEY.md section 8e; the r1 int32 store would have been 102 GB). The ABI takes int32 ids; they are narrowed on the
// device while streaming in (64 Mi tokens per piece through the staging arena). id_bits = 24 adds the byte plane: 3 B per token.
int tokens_load_host(rag_ctx* h, const int32_t* tokens, const int32_t* lens, int64_t n_rows, int L, int id_bits) {
    ARG_CHECK(h, id_bits == 16 || id_bits == 24, "tokens_load: id_bits must be 16 or 24");
    ARG_CHECK(h, tokens && lens && n_rows > 0 && L > 0 && L <= 512, "tokens_load: bad arguments (passage length <= 512)");
    tokens_drop(h);
    tokens_pending store{h};
    const int64_t total = n_rows * (int64_t)L, piece = (int64_t)64 << 20;
    int rc;
    if ((rc = h->tok.alloc(h, (size_t)total))) return rc;
    if (id_bits == 24 && (rc = h->tok_hi.alloc(h, (size_t)total))) return rc;
    if ((rc = h->tok_len.alloc(h, (size_t)n_rows))) return rc;
    if ((rc = stage_reserve(h, stage_size((size_t)std::min(total, piece), 4) + 256))) return rc;
    int32_t* buf = reinterpret_cast<int32_t*>(h->stage.get());
    int* bad = reinterpret_cast<int*>(h->stage + stage_size((size_t)std::min(total, piece), 4));
    HIP_TRY(h, hipMemsetAsync(bad, 0, sizeof(int), h->stream));
    for (int64_t o = 0; o < total; o += piece) {
        const int64_t nn = std::min(piece, total - o);
        HIP_TRY(h, hipMemcpyAsync(buf, tokens + o, (size_t)nn * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        tokens_narrow(h, buf, o, nn, bad, h->stream);
        HIP_TRY(h, hipStreamSynchronize(h->stream));                 // buf is reused by the next piece
    }
    int n_bad = 0;
    HIP_TRY(h, hipMemcpy(&n_bad, bad, sizeof(int), hipMemcpyDeviceToHost));
    ARG_CHECK(h, n_bad == 0, tokens_range_msg(h, false));
    HIP_TRY(h, hipMemcpy(h->tok_len, lens, (size_t)n_rows * sizeof(int32_t), hipMemcpyHostToDevice));
    h->tok_rows = n_rows;
    h->tok_L = L;
    store.done = true;
    return RAG_OK;
}

// Chunked fill from device memory (a replicated 100M-passage store is 45 GB as uint16 and would be 90 GB as one int32 host
// array): reserve once, append row blocks in order. tok_rows counts the rows appended so far; the reservation is
// what tok_len has room for (tok_cap_rows).
int tokens_reserve(rag_ctx* h, int64_t n_rows, int L, int id_bits) {
    ARG_CHECK(h, id_bits == 16 || id_bits == 24, "tokens_reserve: id_bits must be 16 or 24");
    ARG_CHECK(h, n_rows > 0 && L > 0 && L <= 512, "tokens_reserve: bad arguments (passage length <= 512)");
    tokens_drop(h);
    tokens_pending store{h};
    int rc;
    if ((rc = h->tok.alloc(h, (size_t)n_rows * L))) return rc;
    if (id_bits == 24 && (rc = h->tok_hi.alloc(h, (size_t)n_rows * L))) return rc;
    if ((rc = h->tok_len.alloc(h, (size_t)n_rows))) return rc;
    if ((rc = h->tok_bad.reserve(h, 1))) return rc;
    // cleared on the handle's stream and waited for: a null-stream hipMemset is not ordered against the non-blocking stream the
    // first rag_tokens_append_dev counts into it on
    HIP_TRY(h, hipMemsetAsync(h->tok_bad, 0, sizeof(int), h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->tok_L = L;
    store.done = true;
    return RAG_OK;
}

int tokens_info(const rag_ctx* h, int64_t* rows_out, int* L_out, int* id_bits_out) {
    const bool have = h->tok != nullptr;
    if (rows_out) *rows_out = have ? h->tok_rows : 0;
    if (L_out) *L_out = have ? h->tok_L : 0;
    if (id_bits_out) *id_bits_out = !have ? 0 : h->tok_hi ? 24 : 16;
    return RAG_OK;
}

int tokens_append_dev(rag_ctx* h, const int32_t* tokens_dev, const int32_t* lens_dev, int64_t n, hipStream_t st) {
    ARG_CHECK(h, tok_cap_rows(h) > 0, "tokens_append: rag_tokens_reserve first");
    ARG_CHECK(h, n >= 0 && h->tok_rows + n <= tok_cap_rows(h) && (n == 0 || (tokens_dev && lens_dev)), "tokens_append: exceeds the reservation");
    if (n == 0) return RAG_OK;
    const int64_t total = n * (int64_t)h->tok_L;
    tokens_narrow(h, tokens_dev, h->tok_rows * (int64_t)h->tok_L, total, h->tok_bad, st);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(h->tok_len + h->tok_rows, lens_dev, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    int n_bad = 0;                                                   // synchronous check: a load path, not a search path
    HIP_TRY(h, hipMemcpyAsync(&n_bad, h->tok_bad, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    if (n_bad != 0) {
        // the block is rejected whole (tok_rows does not move, its slots are overwritten by the next append); the counter starts
        // again at zero, or every later - valid - append on this handle would be rejected with it
        HIP_TRY(h, hipMemsetAsync(h->tok_bad, 0, sizeof(int), st));
        HIP_TRY(h, hipStreamSynchronize(st));
    }
    ARG_CHECK(h, n_bad == 0, tokens_range_msg(h, true));
    h->tok_rows += n;
    return RAG_OK;
}

// one wave per pair: cand[q][j] is a doc id (id_base + row) or -1. WIDE: the store is 24 bits wide, an id is lo | hi << 16.
// FMT (rag_ce_set_pair_format): RAG_PAIR_BERT [cls] q [sep] d [sep], types 0 | 1; RAG_PAIR_ROBERTA [cls] q [sep] [sep] d [sep], all 0
template <bool WIDE, int FMT>
__global__ __launch_bounds__(256) void ce_build_pairs_kernel(const int32_t* __restrict__ q_tok, const int32_t* __restrict__ q_len,
                                                              int Lq, const int64_t* __restrict__ cand, int64_t id_base,
                                                              const uint16_t* __restrict__ tok, const int32_t* __restrict__ tok_len,
                                                              int Ld, int64_t n_rows, int n_pairs, int pool, int L, int cls_id,
                                                              int sep_id, int32_t* __restrict__ ids, int32_t* __restrict__ tt,
                                                              int32_t* __restrict__ lens, const uint8_t* __restrict__ tok_hi) {
    constexpr int X = FMT == RAG_PAIR_ROBERTA ? 1 : 0;       // the second separator between the two sides
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= n_pairs) return;
    const int q = p / pool;
    const int64_t row = cand[p] < 0 ? -1 : cand[p] - id_base;
    // truncation = 'longest_first' to max_length L, as CrossEncoder.predict tokenises its pairs (SURVEY.md section 8c;
    // the fast tokenizer's rule, pinned against the `tokenizers` package by tests/test_pair_truncation.py): with
    // M = L - 3 content tokens (L - 4 in the RoBERTa layout) and n1 <= n2 the two lengths, the shorter side is kept whole
    // while it fits (n2 = max(n1, M - n1)); if both exceed their share, n1 = M / 2 and n2 = n1 + M % 2.
    int ql = max(0, min(q_len[q], Lq));
    int dl = (row >= 0 && row < n_rows) ? max(0, min(tok_len[row], Ld)) : 0;
    const int M = L - 3 - X;
    if (ql + dl > M) {
        const bool swap = ql > dl;
        int n1 = swap ? dl : ql, n2 = swap ? ql : dl;
        n2 = n1 > M ? n1 : max(n1, M - n1);
        if (n1 + n2 > M) { n1 = M / 2; n2 = n1 + M % 2; }
        ql = swap ? n2 : n1;
        dl = swap ? n1 : n2;
    }
    const int total = ql + dl + 3 + X;
    const int32_t* qt = q_tok + (size_t)q * Lq;
    const uint16_t* dt = tok + (size_t)(row < 0 ? 0 : row) * Ld;
    const uint8_t* dh = WIDE ? tok_hi + (size_t)(row < 0 ? 0 : row) * Ld : nullptr;
    for (int t = lane; t < L; t += 64) {
        int v = 0, ty = 0;
        if (t == 0) v = cls_id;
        else if (t <= ql) v = qt[t - 1];
        else if (t == ql + 1) v = sep_id;
        else if (X && t == ql + 2) v = sep_id;
        else if (t < ql + 2 + X + dl) {
            v = dt[t - ql - 2 - X];
            if constexpr (WIDE) v |= (int)dh[t - ql - 2 - X] << 16;
            ty = X ? 0 : 1;
        } else if (t == ql + 2 + X + dl) { v = sep_id; ty = X ? 0 : 1; }
        ids[(size_t)p * L + t] = v;
        tt[(size_t)p * L + t] = ty;
    }
    if (lane == 0) lens[p] = total;
}

// the instantiation for the handle's store width and pair layout (both read here, while the call enqueues)
static int launch_build_pairs(rag_ctx* h, const int32_t* q_tok, const int32_t* q_len, int Lq, const int64_t* cand, int64_t id_base, size_t P,
                              int pool, int L_pair, int cls_id, int sep_id, int32_t* ids, int32_t* tt, int32_t* lens, hipStream_t st) {
    auto k = h->tok_hi ? (h->pair_format == RAG_PAIR_ROBERTA ? ce_build_pairs_kernel<true, RAG_PAIR_ROBERTA> : ce_build_pairs_kernel<true, RAG_PAIR_BERT>)
                       : (h->pair_format == RAG_PAIR_ROBERTA ? ce_build_pairs_kernel<false, RAG_PAIR_ROBERTA> : ce_build_pairs_kernel<false, RAG_PAIR_BERT>);
    launch(k, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, st, q_tok, q_len, Lq, cand, id_base, h->tok, h->tok_len, h->tok_L, h->tok_rows,
           (int)P, pool, L_pair, cls_id, sep_id, ids, tt, lens, h->tok_hi);
    return launch_status(h);
}

// the rank of slot j (score `mine`) among the n slots of its query in LDS: how many slots that are ok beat it by (score desc,
// slot asc). Distinct slots get distinct ranks. The caller has synchronised the writes of s[] and ok[].
__device__ __forceinline__ int stable_rank(const double* s, const int* ok, int n, int j, double mine) {
    int rank = 0;
    for (int i = 0; i < n; ++i) rank += ok[i] && (s[i] > mine || (s[i] == mine && i < j));
    return rank;
}

// one workgroup per query, pool <= 256: stable rank by (sigmoid desc, candidate position asc).
// RAW (rag_tokvec_rerank_*, tokvec.hip): the score is the float32 itself, no sigmoid; slot_rows [Q][pool] int32 holds the row each
// slot was scored for, -1 = an empty slot, skipped; ids_out gets the row's doc id - idmap[row] or id_base + row for a row of the
// index (row < n_index), -1 for a row the index does not have (its id_base + row could be another row's explicit id); n_index < 0:
// no index, the row number - rows_out (may be null) the row, padding -1 / -1 / 0.0; cand and logit_out are not read.
template <bool RAW>
__global__ __launch_bounds__(256) void rerank_topk_kernel(const float* __restrict__ logits, const int64_t* __restrict__ cand, int pool,
                                                           int k, int64_t* __restrict__ ids_out, double* __restrict__ score_out,
                                                           float* __restrict__ logit_out, const int32_t* __restrict__ slot_rows,
                                                           const int64_t* __restrict__ idmap, int64_t n_index, int64_t id_base,
                                                           int32_t* __restrict__ rows_out) {
    __shared__ double s[256];
    __shared__ int ok[256];
    const int q = blockIdx.x, j = threadIdx.x;
    double mine = -1.0;
    int valid = 0;
    if (j < pool) {
        if constexpr (RAW) {
            valid = slot_rows[(size_t)q * pool + j] >= 0;
            if (valid) mine = (double)logits[(size_t)q * pool + j];
        } else {
            valid = cand[(size_t)q * pool + j] >= 0;
            if (valid) mine = 1.0 / (1.0 + exp(-(double)logits[(size_t)q * pool + j]));          // reranker.py:359
        }
    }
    s[j] = mine;
    ok[j] = valid;
    __syncthreads();
    for (int i = j; i < k; i += 256) {
        ids_out[(size_t)q * k + i] = -1;
        score_out[(size_t)q * k + i] = 0.0;
        if constexpr (RAW) {
            if (rows_out) rows_out[(size_t)q * k + i] = -1;
        } else {
            logit_out[(size_t)q * k + i] = 0.f;
        }
    }
    __syncthreads();
    if (j < pool && valid) {
        const int rank = stable_rank(s, ok, pool, j, mine);
        if (rank < k) {
            score_out[(size_t)q * k + rank] = mine;
            if constexpr (RAW) {
                const int64_t row = slot_rows[(size_t)q * pool + j];
                ids_out[(size_t)q * k + rank] = n_index < 0 ? row : row >= n_index ? (int64_t)-1 : idmap != nullptr ? idmap[row] : id_base + row;
                if (rows_out) rows_out[(size_t)q * k + rank] = (int32_t)row;
            } else {
                ids_out[(size_t)q * k + rank] = cand[(size_t)q * pool + j];
                logit_out[(size_t)q * k + rank] = logits[(size_t)q * pool + j];
            }
        }
    }
}
// the sigmoid instantiation, as rag_rerank_topk_dev and rag_retrieve_rerank_dev launch it
static void launch_rerank_topk(const float* logits, const int64_t* cand, int Q, int pool, int k, int64_t* ids_out, double* scores_out,
                               float* logits_out, hipStream_t st) {
    launch(rerank_topk_kernel<false>, dim3(Q), dim3(256), 0, st, logits, cand, pool, k, ids_out, scores_out, logits_out, nullptr, nullptr,
           (int64_t)0, (int64_t)0, nullptr);
}

// stable top-k of raw MaxSim scores over the slots tokvec_maxsim_kernel filled; ids follow the index's mapping, row numbers without one
int tokvec_topk(rag_ctx* h, const float* scores_dev, const int32_t* slot_rows_dev, int Q, int pool, int k, int64_t* ids_out, int32_t* rows_out,
                double* scores_out, hipStream_t st) {
    const bool idx = h->index_loaded;
    const id_space ids = idx ? id_space::of_index(h) : id_space::rows();
    launch(rerank_topk_kernel<true>, dim3(Q), dim3(256), 0, st, scores_dev, nullptr, pool, k, ids_out, scores_out, nullptr, slot_rows_dev, ids.map,
           idx ? h->n_rows : (int64_t)-1, ids.base, rows_out);
    return launch_status(h);
}

// The two pipeline kernels on their own, for the row-sharded composition (sharded.py::ShardedPipeline): candidates are
// GLOBAL doc ids from the merged lists; the token store is replicated (token_id_base = id of its first row).
int ce_build_pairs_dev(rag_ctx* h, const int32_t* q_tok_dev, const int32_t* q_len_dev, int Lq, const int64_t* cand_dev, int Q, int pool,
                       int64_t token_id_base, int L_pair, int cls_id, int sep_id, int32_t* ids_out, int32_t* tt_out, int32_t* lens_out,
                       hipStream_t st) {
    ARG_CHECK(h, h->tok != nullptr, "build_pairs: no token store loaded");
    ARG_CHECK(h, Q > 0 && pool > 0 && Lq > 0 && L_pair >= 8 && L_pair <= 512 && q_tok_dev && q_len_dev && cand_dev && ids_out && tt_out && lens_out,
              "build_pairs: bad arguments");
    const size_t P = (size_t)Q * pool;
    return launch_build_pairs(h, q_tok_dev, q_len_dev, Lq, cand_dev, token_id_base, P, pool, L_pair, cls_id, sep_id, ids_out, tt_out, lens_out, st);
}

int rerank_topk_dev(rag_ctx* h, const float* logits_dev, const int64_t* cand_dev, int Q, int pool, int k, int64_t* ids_out, double* scores_out,
                    float* logits_out, hipStream_t st) {
    ARG_CHECK(h, Q > 0 && pool > 0 && pool <= RAG_MAX_K && k > 0 && k <= pool && logits_dev && cand_dev && ids_out && scores_out && logits_out,
              "rerank_topk: 0 < k <= pool <= 256");
    launch_rerank_topk(logits_dev, cand_dev, Q, pool, k, ids_out, scores_out, logits_out, st);
    HIP_TRY(h, hipGetLastError());
    return RAG_OK;
}

__global__ void map_rows_to_ids_kernel(int64_t* __restrict__ v, int64_t n, const int64_t* __restrict__ idmap, int64_t id_base) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || v[i] < 0) return;
    v[i] = idmap ? idmap[v[i]] : id_base + v[i];
}
// n row numbers at v -> doc ids in place, as work of st (negative entries stay); nothing to launch where a row number is its id
static int map_rows_to_ids(rag_ctx* h, int64_t* v, size_t n, id_space ids, hipStream_t st) {
    if (ids.identity()) return RAG_OK;
    launch(map_rows_to_ids_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, v, (int64_t)n, ids.map, ids.base);
    return launch_status(h);
}

__global__ void rows_narrow_kernel(const int64_t* __restrict__ in, int32_t* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i] < 0 ? -1 : (int32_t)in[i];
}

// ---- the per-call workspace rag_ctx::pipe_ws: `planes` names every plane once (common.h ws_carve) and runs twice, to size and to carve
template <class F>
static int pipe_ws_carve(rag_ctx* h, F&& planes) {
    ws_carve sum{nullptr}, c{nullptr};
    planes(sum);
    if (int rc = h->pipe_ws.reserve(h, sum.bytes)) return rc;
    c.base = h->pipe_ws;
    planes(c);
    return RAG_OK;
}

// ---- the candidate stage of the three composites: [Q][S] candidate ROWS of the index into w.cand (-1 = an empty slot)
//   mode 0  the dense top-pool                                              S = pool
//   mode 1  dense top-pool + keyword top-pool, RRF -> top-pool              S = pool
//   mode 2  the same RRF at top_k = 2 * pool: the union of the two lists    S = 2 * pool
// The keyword leg is BM25 when qweights_dev is null and the learned-sparse index otherwise (hybrid_legs). It runs in ROW space
// (id_space::rows()): the token store and the token vectors are row-aligned and RRF only needs a consistent key space; each
// composite maps its outputs to doc ids at its end, so explicit doc ids (e.g. primary keys of a loaded shard) work as well as
// id_base + row. w.rows (where the composite asked for the plane): the same rows narrowed to int32.
static inline int cand_slots(int mode, int pool) { return mode == 2 ? 2 * pool : pool; }
struct cand_ws { int64_t* lists; double* sc; int64_t* cand; double* rrf; int32_t* ranks; int32_t* rows; };
// lists [2][Q][pool] i64 | scores [Q][pool] f64 | cand [Q][S] i64 | rrf [Q][S] f64 | ranks [Q][S][2] i32 | rows [Q][S] i32
static void cand_ws_planes(ws_carve& c, cand_ws& w, size_t P, size_t PS, bool narrow) {
    w.lists = c.take<int64_t>(2 * P);
    w.sc = c.take<double>(P);
    w.cand = c.take<int64_t>(PS);
    w.rrf = c.take<double>(PS);
    w.ranks = c.take<int32_t>(2 * PS);
    w.rows = narrow ? c.take<int32_t>(PS) : nullptr;
}
static int candidate_stage(rag_ctx* h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev,
                           int Q, int pool, int rrf_k, int tenant, query_tenants qt, int mode, const cand_ws& w, hipStream_t st) {
    const int S = cand_slots(mode, pool);
    const size_t P = (size_t)Q * pool, PS = (size_t)Q * S;
    int rc;
    if (mode == 0) {
        rc = dense_search(h, q_emb_dev, Q, pool, tenant, w.cand, nullptr, w.sc, st, id_space::rows(), qt);
    } else {
        rc = hybrid_legs(h, q_emb_dev, term_ptr_dev, terms_dev, Q, pool, tenant, w.lists, w.sc, st, id_space::rows(), qt, qweights_dev);
        if (!rc) rc = rrf_fuse_dev(h, w.lists, Q, 2, pool, (int64_t)P, pool, rrf_k, S, w.cand, w.rrf, w.ranks, st);
    }
    if (rc || w.rows == nullptr) return rc;
    launch(rows_narrow_kernel, dim3((unsigned)((PS + 255) / 256)), dim3(256), 0, st, w.cand, w.rows, (int64_t)PS);
    return launch_status(h);
}

int retrieve_rerank_dev(rag_ctx* h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev,
                        const int32_t* q_tok_dev, const int32_t* q_len_dev, int Lq, int Q, int pool, int k, int rrf_k, int tenant,
                        int mode, int cls_id, int sep_id, int L_pair, int64_t* ids_out, double* scores_out, float* logits_out,
                        int64_t* cand_out, hipStream_t st, query_tenants qt) {
    ARG_CHECK(h, h->ce != nullptr, "retrieve_rerank: no cross-encoder loaded");
    ARG_CHECK(h, tokens_aligned(h, h->n_rows), "retrieve_rerank: token store missing or not row-aligned with the index");
    ARG_CHECK(h, Q > 0 && pool > 0 && pool <= RAG_MAX_K && k > 0 && k <= pool, "retrieve_rerank: 0 < k <= pool <= 256");
    ARG_CHECK(h, L_pair >= 8 && L_pair <= 512 && Lq > 0 && q_emb_dev && q_tok_dev && q_len_dev && ids_out && scores_out && logits_out,
              "retrieve_rerank: bad arguments");
    ARG_CHECK(h, mode == 0 || (mode == 1 && term_ptr_dev && h->bm25 != nullptr), "retrieve_rerank: mode 1 needs BM25 postings and query terms");
    if (int rc = mode != 0 ? keyword_postings_aligned(h, false, "retrieve_rerank", RAG_OK, "") : RAG_OK) return rc;
    const size_t P = (size_t)Q * pool;
    cand_ws w;
    int32_t *pid, *ptt, *plen;
    float* logit;
    int rc = pipe_ws_carve(h, [&](ws_carve& c) {
        cand_ws_planes(c, w, P, P, false);
        pid = c.take<int32_t>(P * L_pair);       // pair ids [P][L]
        ptt = c.take<int32_t>(P * L_pair);       // pair token types [P][L]
        plen = c.take<int32_t>(P);               // pair lengths
        logit = c.take<float>(P);
    });
    if (rc) return rc;
    if ((rc = candidate_stage(h, q_emb_dev, term_ptr_dev, terms_dev, nullptr, Q, pool, rrf_k, tenant, qt, mode, w, st))) return rc;
    if ((rc = launch_build_pairs(h, q_tok_dev, q_len_dev, Lq, w.cand, 0, P, pool, L_pair, cls_id, sep_id, pid, ptt, plen, st))) return rc;
    if ((rc = ce_score(h, pid, ptt, plen, (int)P, L_pair, logit, st, false))) return rc;
    launch_rerank_topk(logit, w.cand, Q, pool, k, ids_out, scores_out, logits_out, st);
    HIP_TRY(h, hipGetLastError());
    if (cand_out) HIP_TRY(h, hipMemcpyAsync(cand_out, w.cand, P * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    const id_space ids = id_space::of_index(h);
    if ((rc = map_rows_to_ids(h, ids_out, (size_t)Q * k, ids, st))) return rc;
    return cand_out ? map_rows_to_ids(h, cand_out, P, ids, st) : RAG_OK;
}

// ---- retrieve + late-interaction rerank as one device-resident call (rag_retrieve_maxsim_dev): what retrieve_rerank_dev does for
// the cross-encoder, with the resident token vectors (tokvec.hip) in place of the token store and the forward.
//   1. candidates: dense top-pool (mode 0) or dense + learned-sparse RRF -> top-pool (mode 1), tenant and deleted rows filtered
//   2. tokvec_maxsim_kernel over the [Q][pool] candidate rows   3. the raw top-k of rerank_topk_kernel (which maps the ids)
// mode 2 has no candidate stage: tokvec_scan (tokvec.hip) scores every visible document of the store and hands over each query's
// top-pool rows in rank order; steps 2 and 3 then run over those rows as they are, so a listed pair's score is the rerank kernel's
// own. cand_out is the same ranking at k = pool. q_emb, the query's terms and rrf_k are not read; its planes are carved in mode 2 only.
int retrieve_maxsim_dev(rag_ctx* h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev,
                        const float* q_vecs_dev, const int64_t* q_off_dev, int Q, int pool, int k, int rrf_k, int tenant, int mode,
                        int64_t* ids_out, double* scores_out, int64_t* cand_out, hipStream_t st, query_tenants qt) {
    if (int rc = tokvec_usable(h, "retrieve_maxsim")) return rc;
    ARG_CHECK(h, Q > 0 && Q <= 65535 && pool > 0 && pool <= RAG_MAX_K && k > 0 && k <= pool, "retrieve_maxsim: 1 <= n_queries <= 65535, 0 < k <= pool <= 256");
    ARG_CHECK(h, (q_emb_dev || mode == 2) && q_vecs_dev && q_off_dev && ids_out && scores_out, "retrieve_maxsim: null argument");
    ARG_CHECK(h, mode == 0 || mode == 1 || mode == 2, "retrieve_maxsim: mode is 0 (dense), 1 (dense + sparse) or 2 (every document)");
    ARG_CHECK(h, h->index_loaded, "retrieve_maxsim: no index loaded");
    if (int rc = tokvec_covers_index(h, "retrieve_maxsim")) return rc;
    ARG_CHECK(h, (tenant < 0 && qt.host == nullptr) || h->tenants != nullptr, "retrieve_maxsim: tenant filter requested but no tenants loaded");
    if (mode == 1) {
        ARG_CHECK(h, term_ptr_dev && qweights_dev, "retrieve_maxsim: mode 1 needs the query's terms and weights");
        if (int rc = keyword_postings_aligned(h, true, "retrieve_maxsim", RAG_ERR_ARG)) return rc;
    }
    const size_t P = (size_t)Q * pool;
    if (mode == 2) {
        ARG_CHECK(h, (int64_t)Q * pool < ((int64_t)1 << 24), "retrieve_maxsim: n_queries * pool must be below 2^24");
        ARG_CHECK(h, (tenant < 0 && qt.host == nullptr) || tenants_cover(h, h->n_rows), "retrieve_maxsim: the tenant table does not cover the index's rows");
        int32_t* rows;
        double* cand_sc;
        uint32_t* plane;
        int rc = pipe_ws_carve(h, [&](ws_carve& c) {
            rows = c.take<int32_t>(P);                           // each query's top-pool rows, rank order
            cand_sc = c.take<double>(cand_out ? P : 0);          // the scores beside cand_out: nobody reads them
            plane = c.take<uint32_t>((size_t)tokvec_scan_batch(h, Q) * (size_t)h->tv_docs);      // the scan's keys of one sub-batch
        });
        if (rc) return rc;
        if ((rc = tokvec_scan(h, q_vecs_dev, q_off_dev, Q, pool, tenant, qt, plane, rows, st))) return rc;
        const float* sc;
        const int32_t* slot;
        if ((rc = tokvec_score_slots(h, q_vecs_dev, q_off_dev, rows, Q, pool, &sc, &slot, st))) return rc;
        if ((rc = tokvec_topk(h, sc, slot, Q, pool, k, ids_out, nullptr, scores_out, st))) return rc;
        return cand_out ? tokvec_topk(h, sc, slot, Q, pool, pool, cand_out, nullptr, cand_sc, st) : RAG_OK;
    }
    cand_ws w;
    int rc = pipe_ws_carve(h, [&](ws_carve& c) { cand_ws_planes(c, w, P, P, true); });
    if (rc) return rc;
    if ((rc = candidate_stage(h, q_emb_dev, term_ptr_dev, terms_dev, qweights_dev, Q, pool, rrf_k, tenant, qt, mode, w, st))) return rc;
    if ((rc = tokvec_rerank(h, q_vecs_dev, q_off_dev, w.rows, Q, pool, k, ids_out, nullptr, scores_out, nullptr, st))) return rc;
    if (!cand_out) return RAG_OK;
    HIP_TRY(h, hipMemcpyAsync(cand_out, w.cand, P * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    return map_rows_to_ids(h, cand_out, P, id_space::of_index(h), st);
}

// ---- the three-way bge-m3 score over resident data (rag_m3_score_rows_dev, rag_retrieve_m3_dev): upstream's compute_score mode
// "colbert+sparse+dense" for [Q][S] candidate rows, every component exact for every candidate:
//   dense   = the float64 cosine of the query against the fp32 master row   (cosine_rows_kernel, dense.hip: the rescoring's function)
//   sparse  = the float64 learned-sparse score of that row                  (sparse_point_kernel, bm25.hip)
//   colbert = the float32 pair score of tokvec_maxsim_kernel, widened       (tokvec.hip)
//   score   = ((w_colbert * colbert + w_sparse * sparse) + w_dense * dense) / ((w_dense + w_sparse) + w_colbert)
// in exactly this association (the file is built with -ffp-contract=off: no fused multiply-add), then the stable top-k. A weight of 0
// leaves its component out: not computed, reported as 0.0, its resident structure not required; 0 * 0.0 and x + 0.0 are exact,
// so w_colbert = 0 gives the bits of the two-way "sparse+dense" formula.
// One workgroup per query, S <= 256: rank by (score desc, slot asc) among the slots that hold a row of the index - whatever their
// score. ids follow the index's mapping; cand_out (may be null) gets every slot's id, -1 for an empty slot.
__global__ __launch_bounds__(256) void m3_combine_topk_kernel(const int32_t* __restrict__ rows, const double* __restrict__ dense,
                                                               const double* __restrict__ sparse, const float* __restrict__ colbert, int S, int k,
                                                               double wd, double ws, double wc, const int64_t* __restrict__ idmap,
                                                               int64_t n_index, int64_t id_base, int64_t* __restrict__ ids_out,
                                                               int32_t* __restrict__ rows_out, double* __restrict__ scores_out,
                                                               double* __restrict__ comp_out, int64_t* __restrict__ cand_out) {
    __shared__ double s[256];
    __shared__ int ok[256];
    const int q = blockIdx.x, j = threadIdx.x;
    double d = 0.0, sp = 0.0, c = 0.0, mine = 0.0;
    int valid = 0, row = -1;
    int64_t id = -1;
    if (j < S) {
        const size_t at = (size_t)q * S + j;
        row = rows[at];
        valid = row >= 0 && row < n_index;
        if (valid) {
            if (dense) d = dense[at];
            if (sparse) sp = sparse[at];
            if (colbert) c = (double)colbert[at];
            mine = ((wc * c + ws * sp) + wd * d) / ((wd + ws) + wc);
            id = idmap != nullptr ? idmap[row] : id_base + row;
        }
        if (cand_out) cand_out[at] = id;
    }
    s[j] = mine;
    ok[j] = valid;
    for (int i = j; i < k; i += 256) {
        const size_t o = (size_t)q * k + i;
        ids_out[o] = -1;
        scores_out[o] = 0.0;
        if (rows_out) rows_out[o] = -1;
        if (comp_out) comp_out[o * 3] = comp_out[o * 3 + 1] = comp_out[o * 3 + 2] = 0.0;
    }
    __syncthreads();
    if (valid) {
        const int rank = stable_rank(s, ok, S, j, mine);
        if (rank < k) {
            const size_t o = (size_t)q * k + rank;
            ids_out[o] = id;
            scores_out[o] = mine;
            if (rows_out) rows_out[o] = row;
            if (comp_out) {
                comp_out[o * 3] = d;
                comp_out[o * 3 + 1] = sp;
                comp_out[o * 3 + 2] = c;
            }
        }
    }
}

struct m3_weights { double dense, sparse, colbert; };

static int m3_weights_check(rag_ctx* h, const char* who, m3_weights w) {
    ARG_CHECK(h, std::isfinite(w.dense) && std::isfinite(w.sparse) && std::isfinite(w.colbert) && w.dense >= 0.0 && w.sparse >= 0.0 &&
                     w.colbert >= 0.0 && std::isfinite((w.dense + w.sparse) + w.colbert) && (w.dense + w.sparse) + w.colbert > 0.0,
              (std::string(who) + ": the weights must be finite, each >= 0, with a sum > 0").c_str());
    return RAG_OK;
}

// what both entries check: the weights, and the resident structures the non-zero ones need, aligned with the index's rows
static int m3_check(rag_ctx* h, const char* who, m3_weights w, const float* q_emb, const int32_t* term_ptr, const float* qweights,
                    const float* q_vecs, const int64_t* q_off) {
    const std::string me(who);
    if (int rc = m3_weights_check(h, who, w)) return rc;
    ARG_CHECK(h, h->index_loaded, (me + ": no index loaded").c_str());
    ARG_CHECK(h, w.dense == 0.0 || (q_emb != nullptr && (reinterpret_cast<uintptr_t>(q_emb) & 15) == 0),
              (me + ": a dense weight needs the query embeddings, 16-byte aligned").c_str());
    if (w.sparse > 0.0) {
        if (int rc = keyword_postings_aligned(h, true, who, RAG_ERR_STATE)) return rc;
        ARG_CHECK(h, term_ptr && qweights, (me + ": a sparse weight needs the query's terms and weights").c_str());
    }
    if (w.colbert > 0.0) {
        if (int rc = tokvec_usable(h, who)) return rc;
        if (int rc = tokvec_covers_index(h, who)) return rc;
        ARG_CHECK(h, q_vecs && q_off && (reinterpret_cast<uintptr_t>(q_vecs) & 15) == 0,
                  (me + ": a colbert weight needs the query's token vectors, 16-byte aligned, and their offsets").c_str());
    }
    return RAG_OK;
}

// the components of [Q][S] slots and the top-k: the MaxSim launch, then three more (cosines, point lookups, combine + select).
// dn / sp: float64 workspaces [Q][S] of the caller.
static int m3_score_slots(rag_ctx* h, m3_weights w, const float* q_emb, const int32_t* term_ptr, const int32_t* terms, const float* qweights,
                          const float* q_vecs, const int64_t* q_off, const int32_t* rows, int Q, int S, int k, double* dn, double* sp,
                          int64_t* ids_out, int32_t* rows_out, double* scores_out, double* comp_out, int64_t* cand_out, hipStream_t st) {
    int rc;
    const float* cb = nullptr;
    if (w.colbert > 0.0 && (rc = tokvec_score_slots(h, q_vecs, q_off, rows, Q, S, &cb, nullptr, st))) return rc;
    if (w.dense > 0.0 && (rc = dense_cosine_rows(h, q_emb, rows, Q, S, dn, st))) return rc;
    if (w.sparse > 0.0 && (rc = sparse_score_rows_dev(h, term_ptr, terms, qweights, rows, Q, S, sp, st))) return rc;
    const id_space ids = id_space::of_index(h);
    launch(m3_combine_topk_kernel, dim3((unsigned)Q), dim3(256), 0, st, rows, w.dense > 0.0 ? dn : nullptr, w.sparse > 0.0 ? sp : nullptr, cb, S, k,
           w.dense, w.sparse, w.colbert, ids.map, h->n_rows, ids.base, ids_out, rows_out, scores_out, comp_out, cand_out);
    return launch_status(h);
}

int m3_score_rows_dev(rag_ctx* h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev,
                      const float* q_vecs_dev, const int64_t* q_off_dev, const int32_t* cand_rows_dev, int Q, int pool, int k, double w_dense,
                      double w_sparse, double w_colbert, int64_t* ids_out, int32_t* rows_out, double* scores_out, double* components_out,
                      hipStream_t st) {
    ARG_CHECK(h, Q > 0 && Q <= 65535 && pool > 0 && pool <= RAG_MAX_K && k > 0 && k <= pool, "m3_score_rows: 1 <= n_queries <= 65535, 0 < k <= pool <= 256");
    ARG_CHECK(h, (int64_t)Q * pool < ((int64_t)1 << 24), "m3_score_rows: n_queries * pool must be below 2^24");
    ARG_CHECK(h, cand_rows_dev && ids_out && scores_out, "m3_score_rows: null argument");
    const m3_weights w = {w_dense, w_sparse, w_colbert};
    if (int rc = m3_check(h, "m3_score_rows", w, q_emb_dev, term_ptr_dev, qweights_dev, q_vecs_dev, q_off_dev)) return rc;
    const size_t P = (size_t)Q * pool;
    double *dn, *sp;                                                   // the dense and the sparse component [Q][pool]
    if (int rc = pipe_ws_carve(h, [&](ws_carve& c) { dn = c.take<double>(P); sp = c.take<double>(P); })) return rc;
    return m3_score_slots(h, w, q_emb_dev, term_ptr_dev, terms_dev, qweights_dev, q_vecs_dev, q_off_dev, cand_rows_dev, Q, pool, k, dn, sp, ids_out,
                          rows_out, scores_out, components_out, nullptr, st);
}

// candidates, then the three-way score, in one device-resident call. mode 0 / 1: the candidates of retrieve_maxsim_dev; mode 2: the
// UNION of the dense top-pool and the sparse top-pool = what rrf_fuse_dev over the two lists returns at top_k = 2 * pool (RRF order,
// -1 padded): 2 * pool slots. The candidate stage runs in row space as in retrieve_maxsim_dev; the combine kernel maps the ids.
struct m3_retrieve_ws { cand_ws cw; double *dn, *sp; };              // the candidate planes, the dense and the sparse component [Q][S]
static void m3_retrieve_planes(ws_carve& c, m3_retrieve_ws& w, int Q, int pool, int mode) {
    const size_t P = (size_t)Q * pool, PS = (size_t)Q * cand_slots(mode, pool);
    cand_ws_planes(c, w.cw, P, PS, true);
    w.dn = c.take<double>(PS);
    w.sp = c.take<double>(PS);
}
// every check of rag_retrieve_m3_dev: the arguments, then the resident structures the weights and the mode need
static int retrieve_m3_check(rag_ctx* h, const float* q_emb_dev, const int32_t* term_ptr_dev, const float* qweights_dev, const float* q_vecs_dev,
                             const int64_t* q_off_dev, int Q, int pool, int k, int tenant, int mode, m3_weights w, const int64_t* ids_out,
                             const double* scores_out, query_tenants qt) {
    ARG_CHECK(h, mode == 0 || mode == 1 || mode == 2, "retrieve_m3: mode is 0 (dense), 1 (dense + sparse RRF) or 2 (union of dense and sparse)");
    ARG_CHECK(h, Q > 0 && Q <= 65535 && pool > 0 && pool <= (mode == 2 ? RAG_MAX_K / 2 : RAG_MAX_K) && k > 0 && k <= pool,
              "retrieve_m3: 1 <= n_queries <= 65535, 0 < k <= pool <= 256 (mode 2: pool <= 128)");
    ARG_CHECK(h, (int64_t)Q * cand_slots(mode, pool) < ((int64_t)1 << 24), "retrieve_m3: n_queries * candidate slots must be below 2^24");
    ARG_CHECK(h, q_emb_dev && ids_out && scores_out, "retrieve_m3: null argument");
    if (int rc = m3_check(h, "retrieve_m3", w, q_emb_dev, term_ptr_dev, qweights_dev, q_vecs_dev, q_off_dev)) return rc;
    ARG_CHECK(h, (tenant < 0 && qt.host == nullptr) || h->tenants != nullptr, "retrieve_m3: tenant filter requested but no tenants loaded");
    if (mode != 0) {
        ARG_CHECK(h, term_ptr_dev && qweights_dev, "retrieve_m3: modes 1 and 2 need the query's terms and weights");
        if (int rc = keyword_postings_aligned(h, true, "retrieve_m3", RAG_ERR_STATE)) return rc;
    }
    return RAG_OK;
}
static int retrieve_m3_run(rag_ctx* h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev,
                           const float* q_vecs_dev, const int64_t* q_off_dev, int Q, int pool, int k, int rrf_k, int tenant, int mode, m3_weights w,
                           const m3_retrieve_ws& ws, int64_t* ids_out, double* scores_out, double* components_out, int64_t* cand_out, hipStream_t st,
                           query_tenants qt) {
    if (int rc = candidate_stage(h, q_emb_dev, term_ptr_dev, terms_dev, qweights_dev, Q, pool, rrf_k, tenant, qt, mode, ws.cw, st)) return rc;
    return m3_score_slots(h, w, q_emb_dev, term_ptr_dev, terms_dev, qweights_dev, q_vecs_dev, q_off_dev, ws.cw.rows, Q, cand_slots(mode, pool), k, ws.dn,
                          ws.sp, ids_out, nullptr, scores_out, components_out, cand_out, st);
}

int retrieve_m3_dev(rag_ctx* h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev,
                    const float* q_vecs_dev, const int64_t* q_off_dev, int Q, int pool, int k, int rrf_k, int tenant, int mode, double w_dense,
                    double w_sparse, double w_colbert, int64_t* ids_out, double* scores_out, double* components_out, int64_t* cand_out,
                    hipStream_t st, query_tenants qt) {
    const m3_weights w = {w_dense, w_sparse, w_colbert};
    if (int rc = retrieve_m3_check(h, q_emb_dev, term_ptr_dev, qweights_dev, q_vecs_dev, q_off_dev, Q, pool, k, tenant, mode, w, ids_out, scores_out, qt))
        return rc;
    m3_retrieve_ws ws;
    if (int rc = pipe_ws_carve(h, [&](ws_carve& c) { m3_retrieve_planes(c, ws, Q, pool, mode); })) return rc;
    return retrieve_m3_run(h, q_emb_dev, term_ptr_dev, terms_dev, qweights_dev, q_vecs_dev, q_off_dev, Q, pool, k, rrf_k, tenant, mode, w, ws, ids_out,
                           scores_out, components_out, cand_out, st, qt);
}

// ---- retrieve_m3_dev over row shards (sharded.py ShardedM3Index): the work between the two all-gathers of a batch.
//   gather 1  [world][4][Q][pool]  every rank's dense ids | cosine bits | sparse ids | raw sparse score bits
//   m3_candidates_gathered_dev     two merges (merge_topk_kernel: -1 skipped wherever it stands, nothing normalised), then the candidate
//                                  list of candidate_stage in ID space: RRF sees the two merged lists, which are the unsharded lists
//   m3_score_ids_dev               ids -> rows of this handle (m3_own_rows_kernel; explicit ids: the id map, idmap.hip), the three component launches of m3_score_slots over
//                                  the owned slots, packed as [4][Q][S] int64 (m3_pack_partial_kernel)
//   gather 2  [world][4][Q][S]
//   m3_combine_gathered_dev        m3_combine_topk_kernel with every slot's components taken from the rank that owns it
// The component kernels are the ones the unsharded call launches and each component is a function of (query, row), so every bit of
// the result is the unsharded call's.
int m3_candidates_gathered_dev(rag_ctx* h, const int64_t* gathered_dev, int world, int Q, int pool, int rrf_k, int mode, int64_t* lists_out,
                               double* scores_out, int64_t* cand_out, hipStream_t st) {
    ARG_CHECK(h, mode == 0 || mode == 1 || mode == 2, "m3_candidates_gathered: mode is 0 (dense), 1 (dense + sparse RRF) or 2 (union of dense and sparse)");
    ARG_CHECK(h, world > 0 && Q > 0 && Q <= 65535 && pool > 0 && pool <= (mode == 2 ? RAG_MAX_K / 2 : RAG_MAX_K),
              "m3_candidates_gathered: world >= 1, 1 <= n_queries <= 65535, 0 < pool <= 256 (mode 2: pool <= 128)");
    ARG_CHECK(h, (int64_t)world * pool <= 4092, "m3_candidates_gathered: world * pool must be <= 4092");
    const int S = cand_slots(mode, pool);
    ARG_CHECK(h, (int64_t)Q * S < ((int64_t)1 << 24), "m3_candidates_gathered: n_queries * candidate slots must be below 2^24");
    ARG_CHECK(h, gathered_dev && lists_out && scores_out && cand_out, "m3_candidates_gathered: null argument");
    const int64_t P = (int64_t)Q * pool, stride = 4 * P;
    const double* gs = reinterpret_cast<const double*>(gathered_dev);
    double* rrf = nullptr;                                             // the RRF scores [Q][S]: computed with the keys, not reported
    if (mode != 0)
        if (int rc = pipe_ws_carve(h, [&](ws_carve& c) { rrf = c.take<double>((size_t)Q * S); })) return rc;
    if (int rc = merge_topk(h, gathered_dev, gs + P, world, stride, Q, pool, lists_out, scores_out, st, 0)) return rc;
    if (mode == 0) {
        HIP_TRY(h, hipMemsetAsync(lists_out + P, 0xFF, (size_t)P * sizeof(int64_t), st));                  // -1
        HIP_TRY(h, hipMemsetAsync(scores_out + P, 0, (size_t)P * sizeof(double), st));
        HIP_TRY(h, hipMemcpyAsync(cand_out, lists_out, (size_t)P * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        return RAG_OK;
    }
    if (int rc = merge_topk(h, gathered_dev + 2 * P, gs + 3 * P, world, stride, Q, pool, lists_out + P, scores_out + P, st, 0)) return rc;
    return rrf_fuse_dev(h, lists_out, Q, 2, pool, P, pool, rrf_k, S, cand_out, rrf, nullptr, st);
}

// ids -> the rows of this handle: rows[i] = id - id_base where that is a row of the index, else -1 (an empty slot to the component
// kernels); owned[i] = 1 / 0, plane 0 of the partial block
__global__ __launch_bounds__(256) void m3_own_rows_kernel(const int64_t* __restrict__ cand, int64_t n, int64_t id_base, int64_t n_rows,
                                                           int32_t* __restrict__ rows, int64_t* __restrict__ owned) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t id = cand[i];
    const bool mine = id >= id_base && id - id_base < n_rows;          // (id >= id_base first: id = -1 never wraps)
    rows[i] = mine ? (int32_t)(id - id_base) : -1;
    owned[i] = mine ? 1 : 0;
}

// planes 1-3 of the partial block [4][n]: the float64 bits of the three components, 0.0 for an unowned slot or an absent component.
// scored != null (the late-interaction form, weights (0, 0, w)): the row MaxSim scored each slot for, -1 where it left the slot empty (a
// query or a document without token vectors) - such a slot is given up: flag 0, so the combine skips it as the MaxSim rerank's top-k does.
__global__ __launch_bounds__(256) void m3_pack_partial_kernel(const int32_t* __restrict__ rows, const double* __restrict__ dense,
                                                               const double* __restrict__ sparse, const float* __restrict__ colbert,
                                                               const int32_t* __restrict__ scored, int64_t n, int64_t* __restrict__ owned,
                                                               double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool mine = rows[i] >= 0;
    if (scored != nullptr && mine && scored[i] < 0) {
        mine = false;
        owned[i] = 0;
    }
    out[n + i] = mine && dense ? dense[i] : 0.0;
    out[2 * n + i] = mine && sparse ? sparse[i] : 0.0;
    out[3 * n + i] = mine && colbert ? (double)colbert[i] : 0.0;
}

int m3_score_ids_dev(rag_ctx* h, const float* q_emb_dev, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev,
                     const float* q_vecs_dev, const int64_t* q_off_dev, const int64_t* cand_ids_dev, int Q, int S, double w_dense, double w_sparse,
                     double w_colbert, int64_t* partial_out, hipStream_t st) {
    ARG_CHECK(h, Q > 0 && Q <= 65535 && S > 0 && S <= RAG_MAX_K, "m3_score_ids: 1 <= n_queries <= 65535, 0 < slots <= 256");
    ARG_CHECK(h, (int64_t)Q * S < ((int64_t)1 << 24), "m3_score_ids: n_queries * slots must be below 2^24");
    ARG_CHECK(h, cand_ids_dev && partial_out, "m3_score_ids: null argument");
    const m3_weights w = {w_dense, w_sparse, w_colbert};
    if (int rc = m3_check(h, "m3_score_ids", w, q_emb_dev, term_ptr_dev, qweights_dev, q_vecs_dev, q_off_dev)) return rc;
    if (int rc = idmap_shard_gate(h, "m3_score_ids", ": the index has explicit ids; a row shard is loaded with id_base (ownership is id_base <= id < id_base + rows)"))
        return rc;
    const size_t P = (size_t)Q * S;
    int32_t* rows;
    double *dn, *sp;
    if (int rc = pipe_ws_carve(h, [&](ws_carve& c) { rows = c.take<int32_t>(P); dn = c.take<double>(P); sp = c.take<double>(P); })) return rc;
    const dim3 grid((unsigned)((P + 255) / 256));
    int rc;
    // explicit ids (the gate passed: the id map is enabled): owned = the map holds the id and its row is live (idmap.hip)
    if (h->ids != nullptr) {
        if ((rc = idmap_rows_of_ids(h, cand_ids_dev, (int64_t)P, rows, partial_out, st))) return rc;
    } else {
        launch(m3_own_rows_kernel, grid, dim3(256), 0, st, cand_ids_dev, (int64_t)P, h->id_base, h->n_rows, rows, partial_out);
    }
    const float* cb = nullptr;
    const int32_t* scored = nullptr;
    if (w.colbert > 0.0 && (rc = tokvec_score_slots(h, q_vecs_dev, q_off_dev, rows, Q, S, &cb, &scored, st))) return rc;
    if (w.dense > 0.0 && (rc = dense_cosine_rows(h, q_emb_dev, rows, Q, S, dn, st))) return rc;
    if (w.sparse > 0.0 && (rc = sparse_score_rows_dev(h, term_ptr_dev, terms_dev, qweights_dev, rows, Q, S, sp, st))) return rc;
    const bool late = w.dense == 0.0 && w.sparse == 0.0;               // MaxSim alone: the late-interaction rerank
    launch(m3_pack_partial_kernel, grid, dim3(256), 0, st, rows, w.dense > 0.0 ? dn : nullptr, w.sparse > 0.0 ? sp : nullptr, cb,
           late ? scored : nullptr, (int64_t)P, partial_out, reinterpret_cast<double*>(partial_out));
    return launch_status(h);
}

// m3_combine_topk_kernel over gathered partial blocks: one workgroup per query, S <= 256. Slot j takes its components from the first
// rank r whose owned plane holds 1 at the slot (overlapping shards: the lowest rank wins); no owner, or cand < 0: an empty slot.
// part = [world][4][n] int64, n = Q * S. The score, the stable rank and the writes are m3_combine_topk_kernel's.
__global__ __launch_bounds__(256) void m3_combine_gathered_kernel(const int64_t* __restrict__ cand, const int64_t* __restrict__ part, int world,
                                                                   int64_t n, int S, int k, double wd, double ws, double wc,
                                                                   int64_t* __restrict__ ids_out, double* __restrict__ scores_out,
                                                                   double* __restrict__ comp_out) {
    __shared__ double s[256];
    __shared__ int ok[256];
    const int q = blockIdx.x, j = threadIdx.x;
    double d = 0.0, sp = 0.0, c = 0.0, mine = 0.0;
    int valid = 0;
    int64_t id = -1;
    if (j < S) {
        const size_t at = (size_t)q * S + j;
        id = cand[at];
        int owner = -1;
        for (int r = world - 1; r >= 0; --r)                           // (no early exit: the loads of the flags are independent)
            if (part[(size_t)r * 4 * n + at] != 0) owner = r;
        valid = id >= 0 && owner >= 0;
        if (valid) {
            const double* p = reinterpret_cast<const double*>(part + (size_t)owner * 4 * n);
            d = p[n + at];
            sp = p[2 * n + at];
            c = p[3 * n + at];
            mine = ((wc * c + ws * sp) + wd * d) / ((wd + ws) + wc);
        }
    }
    s[j] = mine;
    ok[j] = valid;
    for (int i = j; i < k; i += 256) {
        const size_t o = (size_t)q * k + i;
        ids_out[o] = -1;
        scores_out[o] = 0.0;
        if (comp_out) comp_out[o * 3] = comp_out[o * 3 + 1] = comp_out[o * 3 + 2] = 0.0;
    }
    __syncthreads();
    if (valid) {
        const int rank = stable_rank(s, ok, S, j, mine);
        if (rank < k) {
            const size_t o = (size_t)q * k + rank;
            ids_out[o] = id;
            scores_out[o] = mine;
            if (comp_out) {
                comp_out[o * 3] = d;
                comp_out[o * 3 + 1] = sp;
                comp_out[o * 3 + 2] = c;
            }
        }
    }
}

int m3_combine_gathered_dev(rag_ctx* h, const int64_t* cand_ids_dev, const int64_t* gathered_dev, int world, int Q, int S, int k, double w_dense,
                            double w_sparse, double w_colbert, int64_t* ids_out, double* scores_out, double* components_out, hipStream_t st) {
    ARG_CHECK(h, world > 0 && Q > 0 && Q <= 65535 && S > 0 && S <= RAG_MAX_K && k > 0 && k <= S,
              "m3_combine_gathered: world >= 1, 1 <= n_queries <= 65535, 0 < k <= slots <= 256");
    ARG_CHECK(h, (int64_t)Q * S < ((int64_t)1 << 24), "m3_combine_gathered: n_queries * slots must be below 2^24");
    ARG_CHECK(h, cand_ids_dev && gathered_dev && ids_out && scores_out, "m3_combine_gathered: null argument");
    if (int rc = m3_weights_check(h, "m3_combine_gathered", {w_dense, w_sparse, w_colbert})) return rc;
    launch(m3_combine_gathered_kernel, dim3((unsigned)Q), dim3(256), 0, st, cand_ids_dev, gathered_dev, world, (int64_t)Q * S, S, k, w_dense,
           w_sparse, w_colbert, ids_out, scores_out, components_out);
    return launch_status(h);
}

// ---- token ids in, the three-way ranking out (rag_search_m3_tokens_dev / _tenants_dev): rag_embed_multi_dev on the handle's embedder,
// rag_lexical_compact_dev on its lexical weights, rag_retrieve_m3_dev on the three results, with every intermediate - dense [Q][hidden],
// lexical [Q][L], token vectors [Q * (L - 1)][tok_dim] (a text has at most L - 1 rows: the capacity needs no look at lens), row offsets,
// the query CSR at capacity Q * L - carved from pipe_ws in ONE carve beside retrieve_m3_dev's own planes. The three stages are the
// functions behind those entries, called with the same arguments a caller would pass, on the same stream: the outputs are the bits
// of the three calls made one after another. What a zero weight or mode 0 does not need is neither carved nor computed.
int search_m3_tokens_dev(rag_ctx* h, const int32_t* input_ids_dev, const int32_t* token_type_ids_dev, const int32_t* lens_dev, int Q, int L,
                         const int32_t* skip_ids_host, int n_skip, int pool, int k, int rrf_k, int tenant, int mode, double w_dense, double w_sparse,
                         double w_colbert, int64_t* ids_out, double* scores_out, double* components_out, int64_t* cand_out, hipStream_t st,
                         query_tenants qt) {
    int tok_dim = 0;
    const int hidden = embed_dim(h);
    if (hidden < 0) {
        h->err = "search_m3_tokens: no embedding model loaded (rag_embed_load_host)";
        return RAG_ERR_STATE;
    }
    ARG_CHECK(h, hidden == h->dim, "search_m3_tokens: the embedder's output width differs from the index dimension");
    ARG_CHECK(h, Q > 0 && Q <= 65535 && L > 0 && L <= 8192 && (int64_t)Q * L < ((int64_t)1 << 31),
              "search_m3_tokens: 1 <= n_queries <= 65535, 1 <= seq_len <= 8192, n_queries * seq_len < 2^31");
    const m3_weights w = {w_dense, w_sparse, w_colbert};
    const bool want_tok = w_colbert > 0.0, want_lex = w_sparse > 0.0 || mode != 0;
    if (want_tok) {
        tok_dim = embed_tok_dim(h);
        if (tok_dim <= 0) {
            h->err = "search_m3_tokens: the token-vector head is not loaded (rag_embed_heads_load_host)";
            return RAG_ERR_STATE;
        }
    }
    m3_retrieve_ws ws;
    float *dense = nullptr, *lex = nullptr, *tok = nullptr, *qw = nullptr;
    int64_t* row_off = nullptr;
    int32_t *term_ptr = nullptr, *terms = nullptr;
    const int64_t tok_cap = (int64_t)Q * (L - 1), terms_cap = (int64_t)Q * L;
    int rc = pipe_ws_carve(h, [&](ws_carve& c) {
        if (mode >= 0 && mode <= 2 && pool > 0 && pool <= RAG_MAX_K) m3_retrieve_planes(c, ws, Q, pool, mode);
        dense = c.take<float>((size_t)Q * hidden);
        if (want_lex) {
            lex = c.take<float>((size_t)Q * L);
            term_ptr = c.take<int32_t>((size_t)Q + 1);
            terms = c.take<int32_t>((size_t)terms_cap);
            qw = c.take<float>((size_t)terms_cap);
        }
        if (want_tok) {
            tok = c.take<float>((size_t)std::max<int64_t>(tok_cap, 1) * tok_dim);
            row_off = c.take<int64_t>((size_t)Q + 1);
        }
    });
    if (rc) return rc;
    if ((rc = retrieve_m3_check(h, dense, term_ptr, qw, tok, row_off, Q, pool, k, tenant, mode, w, ids_out, scores_out, qt))) return rc;
    ARG_CHECK(h, !want_tok || tok_dim == h->tv_dim, "search_m3_tokens: the embedder's token vectors are not as wide as the resident store's");
    if ((rc = embed_multi_dev(h, input_ids_dev, token_type_ids_dev, lens_dev, Q, L, dense, lex, tok, tok_cap, row_off, st))) return rc;
    if (want_lex && (rc = lexical_compact_dev(h, input_ids_dev, lex, lens_dev, Q, L, skip_ids_host, n_skip, term_ptr, terms, qw, terms_cap, st))) return rc;
    return retrieve_m3_run(h, dense, term_ptr, terms, qw, tok, row_off, Q, pool, k, rrf_k, tenant, mode, w, ws, ids_out, scores_out, components_out,
                           cand_out, st, qt);
}
