// Pair scoring for the embedder's token-vector and lexical heads (rag_embed_multi_*; cross_encoder.hip computes the heads):
//   m3_maxsim_kernel          late interaction ("ColBERT" MaxSim): (1 / nq) * sum_i max_j <vq[i], vd[j]> over the texts' own rows
//   m3_lexical_match_kernel   sum over the token ids both texts hold of (max weight in q) * (max weight in d)
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
