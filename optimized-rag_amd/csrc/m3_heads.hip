// Pair scoring for the embedder's token-vector and lexical heads (rag_embed_multi_*; cross_encoder.hip computes the heads):
//   m3_maxsim_kernel          late interaction ("ColBERT" MaxSim): (1 / nq) * sum_i max_j <vq[i], vd[j]> over the texts' own rows
//   m3_lexical_match_kernel   sum over the token ids both texts hold of (max weight in q) * (max weight in d)
// and the reduction of a text's per-position lexical weights to its sorted sparse vector (rag_lexical_compact_*):
//   m3_lexical_compact_kernel one workgroup per text: the largest weight > 0 of each distinct id, ids ascending, by a sort in LDS
//   m3_term_ptr_kernel        the per-text counts -> term_ptr, one workgroup
// Semantics restated from FlagEmbedding's BGEM3FlagModel (colbert_score / compute_lexical_matching_score); parity with upstream is
// not pinned.
//
// MaxSim numerics: the operands are float32 unit vectors. A plain fp16 product loses 2 * 2^-11 on a dot of unit vectors, the whole
// 1e-3 score contract, so every operand is split on the fly into hi = fp16(x), lo = fp16(x - hi) and every product is three
// mfma_f32_16x16x32_f16: lo*hi + hi*lo + hi*hi with fp32 accumulation (the cross-encoder's scheme). Fragment maps as in
// ce_gemm_kernel: lane (fr = lane & 15, fq = lane >> 4) holds A[row fr][k = 8 fq ..+8] and B[col fr][the same k]; acc[r] =
// C[row 4 fq + r][col fr]. A = 16 document rows, B = 16 query rows, so a lane's four accumulators are four documents of ONE query:
// the maximum over documents is a lane-local max and two cross-lane steps.
// One workgroup (4 waves) per pair. Queries go in blocks of 32 rows (two B tiles per wave); wave w takes the document tile pairs
// w, w + 4, ... (two A tiles against two B tiles = four accumulator tiles) and reads its fragments straight from global memory, the
// floats of K-step k + 1 requested before step k is split and multiplied: a document row is read once per query block, the query
// block once per document tile pair (it stays in L2: 128 KiB at dim 1024). Memory-bound: 256 x 100 pairs of 32 x 255 rows at dim
// 1024 read their 26.7 GB of passages at 0.96 of the device's measured copy rate. Rows of a tile past the text's rows are loaded from the text's last row
// (never out of bounds) and masked out of the maximum, never zero-filled: a maximum may be negative. The per-query maxima of the
// four waves meet in LDS and ONE thread sums them in query order in float64: no atomics, the result is a function of the pair's
// own rows alone, bit-identical from run to run and whatever else the call holds.
#include "common.h"

#include <algorithm>
#include <cmath>

#define MS_QT 2          // 16-row query tiles per block of queries
#define MS_DT 2          // 16-row document tiles a wave holds against them at once

struct ms_raw8 { float4 a, b; };             // a lane's 8 consecutive floats of one row
__device__ __forceinline__ ms_raw8 ms_load8(const float* __restrict__ p) {
    return {*reinterpret_cast<const float4*>(p), *reinterpret_cast<const float4*>(p + 4)};
}
__device__ __forceinline__ void ms_split8(const ms_raw8& r, half8& hi, half8& lo) {
    const float v[8] = {r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z, r.b.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        hi[i] = (half_t)v[i];
        lo[i] = (half_t)(v[i] - (float)hi[i]);
    }
}

__global__ __launch_bounds__(256) void m3_maxsim_kernel(const float* __restrict__ q, const int64_t* __restrict__ q_off, int n_q,
                                                         const float* __restrict__ d, const int64_t* __restrict__ d_off, int n_d,
                                                         const int32_t* __restrict__ pair_q, const int32_t* __restrict__ pair_d, int dim,
                                                         float* __restrict__ out) {
    __shared__ float wmax[4][MS_QT * 16];
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    const int qi = pair_q[pair], di = pair_d[pair];
    int64_t q0 = 0, d0 = 0, nq = 0, nd = 0;
    if (qi >= 0 && qi < n_q && di >= 0 && di < n_d) {
        q0 = q_off[qi];
        nq = q_off[qi + 1] - q0;
        d0 = d_off[di];
        nd = d_off[di + 1] - d0;
    }
    if (nq <= 0 || nd <= 0) {                                  // an index outside its side, or an empty side (uniform over the workgroup)
        if (tid == 0) out[pair] = 0.f;
        return;
    }
    const int64_t nd_tiles = (nd + 15) >> 4;
    double total = 0.0;                                        // thread 0 alone
    for (int64_t qb = 0; qb < nq; qb += MS_QT * 16) {
        const float* qp[MS_QT];
        float best[MS_QT];
#pragma unroll
        for (int j = 0; j < MS_QT; ++j) {
            const int64_t row = min(qb + j * 16 + fr, nq - 1);
            qp[j] = q + (q0 + row) * dim + fq * 8;
            best[j] = -INFINITY;
        }
        for (int64_t dt0 = (int64_t)wv * MS_DT; dt0 < nd_tiles; dt0 += 4 * MS_DT) {
            const float* dp[MS_DT];
#pragma unroll
            for (int t = 0; t < MS_DT; ++t) dp[t] = d + (d0 + min((dt0 + t) * 16 + fr, nd - 1)) * dim + fq * 8;
            f32x4 acc[MS_DT][MS_QT];
#pragma unroll
            for (int t = 0; t < MS_DT; ++t)
#pragma unroll
                for (int j = 0; j < MS_QT; ++j) acc[t][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            // the floats of K-step k + 1 are requested before those of step k are split and multiplied
            ms_raw8 dr[MS_DT], qr[MS_QT];
#pragma unroll
            for (int t = 0; t < MS_DT; ++t) dr[t] = ms_load8(dp[t]);
#pragma unroll
            for (int j = 0; j < MS_QT; ++j) qr[j] = ms_load8(qp[j]);
            for (int k = 0; k < dim; k += 32) {
                const int kn = k + 32 < dim ? k + 32 : k;      // the last step re-reads itself: no branch around the loads
                ms_raw8 dn[MS_DT], qn[MS_QT];
#pragma unroll
                for (int t = 0; t < MS_DT; ++t) dn[t] = ms_load8(dp[t] + kn);
#pragma unroll
                for (int j = 0; j < MS_QT; ++j) qn[j] = ms_load8(qp[j] + kn);
                half8 ah[MS_DT], al[MS_DT], bh[MS_QT], bl[MS_QT];
#pragma unroll
                for (int t = 0; t < MS_DT; ++t) ms_split8(dr[t], ah[t], al[t]);
#pragma unroll
                for (int j = 0; j < MS_QT; ++j) ms_split8(qr[j], bh[j], bl[j]);
#pragma unroll
                for (int t = 0; t < MS_DT; ++t)
#pragma unroll
                    for (int j = 0; j < MS_QT; ++j) {
                        acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[t], bh[j], acc[t][j], 0, 0, 0);
                        acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[t], bl[j], acc[t][j], 0, 0, 0);
                        acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[t], bh[j], acc[t][j], 0, 0, 0);
                    }
#pragma unroll
                for (int t = 0; t < MS_DT; ++t) dr[t] = dn[t];
#pragma unroll
                for (int j = 0; j < MS_QT; ++j) qr[j] = qn[j];
            }
            // acc[t][j][r] = <document row (dt0 + t) * 16 + 4 fq + r, query row qb + 16 j + fr>; rows past the document stay out of the maximum
#pragma unroll
            for (int t = 0; t < MS_DT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if ((dt0 + t) * 16 + fq * 4 + r < nd) {
#pragma unroll
                        for (int j = 0; j < MS_QT; ++j) best[j] = fmaxf(best[j], acc[t][j][r]);
                    }
        }
#pragma unroll
        for (int j = 0; j < MS_QT; ++j) {
            best[j] = fmaxf(best[j], __shfl_xor(best[j], 16));
            best[j] = fmaxf(best[j], __shfl_xor(best[j], 32));
            if (lane < 16) wmax[wv][j * 16 + lane] = best[j];
        }
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < MS_QT * 16 && qb + i < nq; ++i)
                total += (double)fmaxf(fmaxf(wmax[0][i], wmax[1][i]), fmaxf(wmax[2][i], wmax[3][i]));
        __syncthreads();
    }
    if (tid == 0) out[pair] = (float)(total / (double)nq);
}

// ---- lexical match. One workgroup per pair. A query position counts when it is the FIRST holding its id, the id is not skipped
// and the id's largest query weight is > 0; it contributes that weight times the id's largest document weight (when > 0). Every
// position scans its own side for the first-occurrence test and the maximum, and the other side for the match: (lq + ld) id
// compares per query position, lq * (lq + ld) / 256 per thread - 0.5M for two texts of 8192 tokens (milliseconds), a few hundred
// for a query of 32 against a passage of 255. The products are summed in float64, per thread in position order, then by a fixed tree.
struct m3_skip {
    int32_t id[8];
    int n;
};

__global__ __launch_bounds__(256) void m3_lexical_match_kernel(const int32_t* __restrict__ q_ids, const float* __restrict__ q_w,
                                                                const int32_t* __restrict__ q_lens, int n_q, int Lq,
                                                                const int32_t* __restrict__ d_ids, const float* __restrict__ d_w,
                                                                const int32_t* __restrict__ d_lens, int n_d, int Ld,
                                                                const int32_t* __restrict__ pair_q, const int32_t* __restrict__ pair_d,
                                                                m3_skip skip, float* __restrict__ out) {
    __shared__ double part[256];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int qi = pair_q[pair], di = pair_d[pair];
    double s = 0.0;
    if (qi >= 0 && qi < n_q && di >= 0 && di < n_d) {
        const int lq = max(0, min(q_lens[qi], Lq)), ld = max(0, min(d_lens[di], Ld));
        const int32_t* qid = q_ids + (size_t)qi * Lq;
        const float* qw = q_w + (size_t)qi * Lq;
        const int32_t* did = d_ids + (size_t)di * Ld;
        const float* dw = d_w + (size_t)di * Ld;
        for (int i = tid; i < lq; i += 256) {
            const int32_t id = qid[i];
            bool use = true;
            for (int k = 0; k < skip.n; ++k) use = use && id != skip.id[k];
            if (!use) continue;
            float wq = qw[i];
            for (int j = 0; j < lq; ++j)
                if (qid[j] == id) {
                    if (j < i) { use = false; break; }
                    wq = fmaxf(wq, qw[j]);
                }
            if (!use || !(wq > 0.f)) continue;
            float wd = 0.f;
            for (int j = 0; j < ld; ++j)
                if (did[j] == id) wd = fmaxf(wd, dw[j]);
            if (wd > 0.f) s += (double)wq * (double)wd;
        }
    }
    part[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) part[tid] += part[tid + o];
        __syncthreads();
    }
    if (tid == 0) out[pair] = (float)part[0];
}

// ---- lexical compaction (rag_lexical_compact_*): a text's per-position lexical weights -> its sparse vector, the largest weight > 0
// of each distinct token id, ids ascending - what LexicalPostings.encode_queries builds from encode_multi's maps. One workgroup per
// text sorts 64-bit keys (id << 32 | weight bits) in LDS; a dropped position (past the length, a skipped or negative id, a weight
// that is not > 0) is the key of all ones, whose bit 63 no kept key has (ids end at 2^31 - 1), so it sorts behind every kept key and
// INT32_MAX stays a legal id. Positive float32 bit patterns order as their values do: after ONE ascending sort the last key of an
// id's run carries its largest weight, and a run's end is a position whose successor has another high word.
// Bitonic network over N = the power of two >= max(len, 64) keys. Stages whose partner distance is below 64 run in registers: a
// wave holds 64 consecutive keys, one per lane, and exchanges by lane shuffles (a distance below 32 keys would put lanes l and l + 16
// of a 32-lane LDS group on one bank: 2-way on every read); the stages at distance >= 64 read and write 32 consecutive 8-byte keys per
// 32-lane group, one 256-byte bank row, without conflicts. Each text is sorted twice - COUNT (the per-text counts, which the scan
// turns into term_ptr in place) and WRITE (the packed output at its offset) - rather than staged through an [n][L] plane: a query
// is tens of tokens, a passage's sort a few microseconds, and the call keeps no workspace.
#define LC_DROPPED 0xFFFFFFFFFFFFFFFFull

__device__ __forceinline__ unsigned long long lc_exchange(unsigned long long v, int idx, int j, int k) {
    const unsigned long long o = __shfl_xor(v, j);
    const bool keep_min = ((idx & j) == 0) == ((idx & k) == 0);
    return keep_min ? (v < o ? v : o) : (v < o ? o : v);
}

template <bool WRITE>
__global__ __launch_bounds__(256) void m3_lexical_compact_kernel(const int32_t* __restrict__ ids, const float* __restrict__ weights,
                                                                  const int32_t* __restrict__ lens, int L, m3_skip skip,
                                                                  int32_t* __restrict__ term_ptr, int32_t* __restrict__ terms_out,
                                                                  float* __restrict__ qweights_out, int64_t cap) {
    extern __shared__ unsigned long long lc_keys[];            // N keys
    __shared__ int wave_total[4];
    const int text = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = max(0, min(lens[text], L));
    int N = 64;
    while (N < m) N <<= 1;
    const int32_t* id_row = ids + (size_t)text * L;
    const float* w_row = weights + (size_t)text * L;
    // keys in, every phase up to k = 64 in registers
    for (int c = wv; c < (N >> 6); c += 4) {
        const int idx = (c << 6) + lane;
        unsigned long long v = LC_DROPPED;
        if (idx < m) {
            const int32_t id = id_row[idx];
            const float w = w_row[idx];
            bool use = id >= 0 && w > 0.f;
            for (int s = 0; s < skip.n; ++s) use = use && id != skip.id[s];
            if (use) v = ((unsigned long long)(uint32_t)id << 32) | (unsigned long long)__float_as_uint(w);
        }
        for (int k = 2; k <= 64; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) v = lc_exchange(v, idx, j, k);
        lc_keys[idx] = v;
    }
    __syncthreads();
    for (int k = 128; k <= N; k <<= 1) {
        for (int j = k >> 1; j >= 64; j >>= 1) {
            for (int p = tid; p < (N >> 1); p += 256) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                const unsigned long long a = lc_keys[i], b = lc_keys[i + j];
                if ((a > b) == ((i & k) == 0)) {
                    lc_keys[i] = b;
                    lc_keys[i + j] = a;
                }
            }
            __syncthreads();
        }
        for (int c = wv; c < (N >> 6); c += 4) {
            const int idx = (c << 6) + lane;
            unsigned long long v = lc_keys[idx];
            for (int j = 32; j > 0; j >>= 1) v = lc_exchange(v, idx, j, k);
            lc_keys[idx] = v;
        }
        __syncthreads();
    }
    // the run ends, counted in key order 256 at a time: a position's output slot is the run ends before it
    int before = 0;                                            // run ends in the chunks so far (the same in every thread)
    const int64_t base = WRITE ? (int64_t)term_ptr[text] : 0;
    for (int c0 = 0; c0 < N; c0 += 256) {
        const int i = c0 + tid;
        unsigned long long v = LC_DROPPED;
        bool end = false;
        if (i < N) {
            v = lc_keys[i];
            end = v != LC_DROPPED && (i == N - 1 || (lc_keys[i + 1] >> 32) != (v >> 32));
        }
        const unsigned long long vote = __ballot(end);
        if (lane == 0) wave_total[wv] = __popcll(vote);
        __syncthreads();
        int mine = before + __popcll(vote & ((1ull << lane) - 1ull));
        for (int x = 0; x < 4; ++x) {
            if (x < wv) mine += wave_total[x];
            before += wave_total[x];
        }
        if (WRITE && end && base + mine < cap) {
            terms_out[base + mine] = (int32_t)(v >> 32);
            qweights_out[base + mine] = __uint_as_float((uint32_t)v);
        }
        __syncthreads();
    }
    if (!WRITE && tid == 0) term_ptr[text + 1] = before;
}

// term_ptr[i + 1] holds text i's count on entry; on exit term_ptr is the exclusive prefix (term_ptr[0] = 0, term_ptr[n] = the call's
// true total). One workgroup, every thread a contiguous span of texts, as m3_row_off_kernel (cross_encoder.hip); in place: a thread
// reads and writes the entries of its own span only.
__global__ __launch_bounds__(1024) void m3_term_ptr_kernel(int32_t* __restrict__ term_ptr, int n) {
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    const int per = (n + 1023) / 1024;
    const int b = min(n, tid * per), e = min(n, b + per);
    int s = 0;
    for (int p = b; p < e; ++p) s += term_ptr[p + 1];
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int off = part[tid] - s;
    for (int p = b; p < e; ++p) {
        off += term_ptr[p + 1];
        term_ptr[p + 1] = off;
    }
    if (tid == 0) term_ptr[0] = 0;
}

// ------------------------------------------------------------------------------------------------
// Host side
// ------------------------------------------------------------------------------------------------
int maxsim_dev(rag_ctx* h, const float* q, const int64_t* q_off, int n_q, const float* d, const int64_t* d_off, int n_d, const int32_t* pair_q,
               const int32_t* pair_d, int n_pairs, int dim, float* out, hipStream_t st) {
    ARG_CHECK(h, n_pairs >= 0 && n_q >= 0 && n_d >= 0, "maxsim: negative count");
    ARG_CHECK(h, dim >= 32 && dim <= 1024 && dim % 32 == 0, "maxsim: dim must be a multiple of 32 in [32, 1024]");
    if (n_pairs == 0) return RAG_OK;
    ARG_CHECK(h, q_off && d_off && pair_q && pair_d && out, "maxsim: null argument");
    ARG_CHECK(h, (q || n_q == 0) && (d || n_d == 0), "maxsim: null vectors");
    ARG_CHECK(h, (reinterpret_cast<uintptr_t>(q) & 15) == 0 && (reinterpret_cast<uintptr_t>(d) & 15) == 0, "maxsim: vectors must be 16-byte aligned");
    launch(m3_maxsim_kernel, dim3((unsigned)n_pairs), dim3(256), 0, st, q, q_off, n_q, d, d_off, n_d, pair_q, pair_d, dim, out);
    return launch_status(h);
}

// copies n elements of a host array into a fresh device buffer on st
template <class T>
static int stage_in(rag_ctx* h, dev_buf<T>& b, const T* src, size_t n, hipStream_t st) {
    if (int rc = b.alloc(h, std::max<size_t>(n, 1))) return rc;
    if (n) HIP_TRY(h, hipMemcpyAsync(b, src, n * sizeof(T), hipMemcpyHostToDevice, st));
    return RAG_OK;
}

static bool offsets_ok(const int64_t* off, int n) {
    if (off[0] < 0) return false;
    for (int i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return false;
    return true;
}

int maxsim_host(rag_ctx* h, const float* q, const int64_t* q_off, int n_q, const float* d, const int64_t* d_off, int n_d, const int32_t* pair_q,
                const int32_t* pair_d, int n_pairs, int dim, float* out) {
    ARG_CHECK(h, n_pairs >= 0 && n_q >= 0 && n_d >= 0, "maxsim: negative count");
    ARG_CHECK(h, dim >= 32 && dim <= 1024 && dim % 32 == 0, "maxsim: dim must be a multiple of 32 in [32, 1024]");
    if (n_pairs == 0) return RAG_OK;
    ARG_CHECK(h, q_off && d_off && pair_q && pair_d && out, "maxsim: null argument");
    ARG_CHECK(h, offsets_ok(q_off, n_q) && offsets_ok(d_off, n_d), "maxsim: row offsets must start at >= 0 and never decrease");
    ARG_CHECK(h, (q || q_off[n_q] == 0) && (d || d_off[n_d] == 0), "maxsim: null vectors");
    hipStream_t st = h->stream;
    dev_buf<float> dq, dd, dout;
    dev_buf<int64_t> dqo, ddo;
    dev_buf<int32_t> dpq, dpd;
    int rc;
    if ((rc = stage_in(h, dq, q, (size_t)q_off[n_q] * dim, st)) || (rc = stage_in(h, dd, d, (size_t)d_off[n_d] * dim, st))) return rc;
    if ((rc = stage_in(h, dqo, q_off, (size_t)n_q + 1, st)) || (rc = stage_in(h, ddo, d_off, (size_t)n_d + 1, st))) return rc;
    if ((rc = stage_in(h, dpq, pair_q, (size_t)n_pairs, st)) || (rc = stage_in(h, dpd, pair_d, (size_t)n_pairs, st))) return rc;
    if ((rc = dout.alloc(h, (size_t)n_pairs))) return rc;
    rc = maxsim_dev(h, dq, dqo, n_q, dd, ddo, n_d, dpq, dpd, n_pairs, dim, dout, st);
    if (!rc) HIP_TRY(h, hipMemcpyAsync(out, dout, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return rc;
}

int lexical_match_dev(rag_ctx* h, const int32_t* q_ids, const float* q_w, const int32_t* q_lens, int n_q, int Lq, const int32_t* d_ids,
                      const float* d_w, const int32_t* d_lens, int n_d, int Ld, const int32_t* pair_q, const int32_t* pair_d, int n_pairs,
                      const int32_t* skip_ids_host, int n_skip, float* out, hipStream_t st) {
    ARG_CHECK(h, n_pairs >= 0 && n_q >= 0 && n_d >= 0 && Lq > 0 && Ld > 0, "lexical_match: bad counts");
    ARG_CHECK(h, n_skip >= 0 && n_skip <= 8 && (skip_ids_host || n_skip == 0), "lexical_match: at most 8 skip ids");
    if (n_pairs == 0) return RAG_OK;
    ARG_CHECK(h, pair_q && pair_d && out && (n_q == 0 || (q_ids && q_w && q_lens)) && (n_d == 0 || (d_ids && d_w && d_lens)), "lexical_match: null argument");
    m3_skip skip = {};
    for (int i = 0; i < n_skip; ++i) skip.id[i] = skip_ids_host[i];
    skip.n = n_skip;
    launch(m3_lexical_match_kernel, dim3((unsigned)n_pairs), dim3(256), 0, st, q_ids, q_w, q_lens, n_q, Lq, d_ids, d_w, d_lens, n_d, Ld, pair_q,
           pair_d, skip, out);
    return launch_status(h);
}

int lexical_match_host(rag_ctx* h, const int32_t* q_ids, const float* q_w, const int32_t* q_lens, int n_q, int Lq, const int32_t* d_ids,
                       const float* d_w, const int32_t* d_lens, int n_d, int Ld, const int32_t* pair_q, const int32_t* pair_d, int n_pairs,
                       const int32_t* skip_ids, int n_skip, float* out) {
    ARG_CHECK(h, n_pairs >= 0 && n_q >= 0 && n_d >= 0 && Lq > 0 && Ld > 0, "lexical_match: bad counts");
    if (n_pairs == 0) return RAG_OK;
    ARG_CHECK(h, pair_q && pair_d && out && (n_q == 0 || (q_ids && q_w && q_lens)) && (n_d == 0 || (d_ids && d_w && d_lens)), "lexical_match: null argument");
    hipStream_t st = h->stream;
    dev_buf<int32_t> dqi, dql, ddi, ddl, dpq, dpd;
    dev_buf<float> dqw, ddw, dout;
    int rc;
    if ((rc = stage_in(h, dqi, q_ids, (size_t)n_q * Lq, st)) || (rc = stage_in(h, dqw, q_w, (size_t)n_q * Lq, st)) ||
        (rc = stage_in(h, dql, q_lens, (size_t)n_q, st)))
        return rc;
    if ((rc = stage_in(h, ddi, d_ids, (size_t)n_d * Ld, st)) || (rc = stage_in(h, ddw, d_w, (size_t)n_d * Ld, st)) ||
        (rc = stage_in(h, ddl, d_lens, (size_t)n_d, st)))
        return rc;
    if ((rc = stage_in(h, dpq, pair_q, (size_t)n_pairs, st)) || (rc = stage_in(h, dpd, pair_d, (size_t)n_pairs, st))) return rc;
    if ((rc = dout.alloc(h, (size_t)n_pairs))) return rc;
    rc = lexical_match_dev(h, dqi, dqw, dql, n_q, Lq, ddi, ddw, ddl, n_d, Ld, dpq, dpd, n_pairs, skip_ids, n_skip, dout, st);
    if (!rc) HIP_TRY(h, hipMemcpyAsync(out, dout, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return rc;
}

static int lexical_compact_check(rag_ctx* h, const int32_t* ids, const float* w, const int32_t* lens, int n, int L, const int32_t* skip_ids,
                                 int n_skip, const int32_t* term_ptr_out, const int32_t* terms_out, const float* qw_out, int64_t cap) {
    ARG_CHECK(h, n >= 1 && n <= 65535 && L >= 1 && L <= 8192 && (int64_t)n * L < ((int64_t)1 << 31),
              "lexical_compact: 1 <= n_texts <= 65535, 1 <= seq_len <= 8192, n_texts * seq_len < 2^31");
    ARG_CHECK(h, n_skip >= 0 && n_skip <= 8 && (skip_ids || n_skip == 0), "lexical_compact: at most 8 skip ids");
    ARG_CHECK(h, cap >= 0, "lexical_compact: terms_cap must be >= 0");
    ARG_CHECK(h, ids && w && lens && term_ptr_out && ((terms_out && qw_out) || cap == 0), "lexical_compact: null argument");
    return RAG_OK;
}

static int lexical_compact_run(rag_ctx* h, const int32_t* ids, const float* w, const int32_t* lens, int n, int L, const int32_t* skip_ids,
                               int n_skip, int32_t* term_ptr_out, int32_t* terms_out, float* qw_out, int64_t cap, hipStream_t st) {
    m3_skip skip = {};
    for (int i = 0; i < n_skip; ++i) skip.id[i] = skip_ids[i];
    skip.n = n_skip;
    int N = 64;
    while (N < L) N <<= 1;
    const int lds = N * 8;
    if (int rc = raise_lds(h, h->attr_m3_compact_lds, lds, m3_lexical_compact_kernel<false>, m3_lexical_compact_kernel<true>)) return rc;
    launch(m3_lexical_compact_kernel<false>, dim3((unsigned)n), dim3(256), (size_t)lds, st, ids, w, lens, L, skip, term_ptr_out, nullptr, nullptr,
           (int64_t)0);
    launch(m3_term_ptr_kernel, dim3(1), dim3(1024), 0, st, term_ptr_out, n);
    if (cap > 0)
        launch(m3_lexical_compact_kernel<true>, dim3((unsigned)n), dim3(256), (size_t)lds, st, ids, w, lens, L, skip, term_ptr_out, terms_out, qw_out,
               cap);
    return launch_status(h);
}

int lexical_compact_dev(rag_ctx* h, const int32_t* ids, const float* w, const int32_t* lens, int n, int L, const int32_t* skip_ids_host, int n_skip,
                        int32_t* term_ptr_out, int32_t* terms_out, float* qw_out, int64_t cap, hipStream_t st) {
    if (int rc = lexical_compact_check(h, ids, w, lens, n, L, skip_ids_host, n_skip, term_ptr_out, terms_out, qw_out, cap)) return rc;
    return lexical_compact_run(h, ids, w, lens, n, L, skip_ids_host, n_skip, term_ptr_out, terms_out, qw_out, cap, st);
}

// Host arrays: the total is counted on the host before anything is queued (the distinct kept ids of each text), so a capacity that is
// too small is an error here; the device-pointer path then runs on staged copies and the call waits.
int lexical_compact_host(rag_ctx* h, const int32_t* ids, const float* w, const int32_t* lens, int n, int L, const int32_t* skip_ids, int n_skip,
                         int32_t* term_ptr_out, int32_t* terms_out, float* qw_out, int64_t cap) {
    int rc;
    if ((rc = lexical_compact_check(h, ids, w, lens, n, L, skip_ids, n_skip, term_ptr_out, terms_out, qw_out, cap))) return rc;
    int64_t total = 0;
    std::vector<int32_t> kept;
    for (int i = 0; i < n; ++i) {
        const int m = std::max(0, std::min(lens[i], L));
        kept.clear();
        for (int t = 0; t < m; ++t) {
            const int32_t id = ids[(size_t)i * L + t];
            bool use = id >= 0 && w[(size_t)i * L + t] > 0.f;
            for (int s = 0; s < n_skip; ++s) use = use && id != skip_ids[s];
            if (use) kept.push_back(id);
        }
        std::sort(kept.begin(), kept.end());
        total += std::unique(kept.begin(), kept.end()) - kept.begin();
    }
    ARG_CHECK(h, total <= cap, "lexical_compact: terms_cap is smaller than the call's terms");
    hipStream_t st = h->stream;
    const size_t n_tok = (size_t)n * L;
    dev_buf<int32_t> d_ids, d_lens, d_ptr, d_terms;
    dev_buf<float> d_w, d_qw;
    if ((rc = stage_in(h, d_ids, ids, n_tok, st)) || (rc = stage_in(h, d_w, w, n_tok, st)) || (rc = stage_in(h, d_lens, lens, (size_t)n, st))) return rc;
    if ((rc = d_ptr.alloc(h, (size_t)n + 1)) || (rc = d_terms.alloc(h, (size_t)std::max<int64_t>(total, 1))) ||
        (rc = d_qw.alloc(h, (size_t)std::max<int64_t>(total, 1))))
        return rc;
    rc = lexical_compact_run(h, d_ids, d_w, d_lens, n, L, skip_ids, n_skip, d_ptr, d_terms, d_qw, total, st);
    if (!rc) HIP_TRY(h, hipMemcpyAsync(term_ptr_out, d_ptr, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost, st));
    if (!rc && total > 0) {
        HIP_TRY(h, hipMemcpyAsync(terms_out, d_terms, (size_t)total * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipMemcpyAsync(qw_out, d_qw, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(h, hipStreamSynchronize(st));                   // also before the staging buffers go
    return rc;
}
