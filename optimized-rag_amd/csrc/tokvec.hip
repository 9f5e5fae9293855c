// Resident token-vector store and late-interaction rerank over it (rag_tokvec_*; rag_retrieve_maxsim_dev in pipeline.hip).
// The passages' token vectors ("ColBERT" rows, the tok_out of rag_embed_multi_*) are computed once at ingest and kept in HBM as
// packed fp16 rows [rows][dim] with int64 offsets [docs + 1]; document i is row i of the dense index. A query then costs one
// embedder forward (its own), and a rerank reads half the bytes rag_maxsim_* reads for the same pairs.
//   tokvec_convert_kernel     float32 -> fp16, round to nearest even (v_cvt_f16_f32), counting values that are not finite as fp16
//   tokvec_quant8_kernel      float32 -> block amax, scale exponent, E4M3 codes and the E8M0 scale byte; the same count
//   tokvec_offsets_kernel     a block's offsets, relative to its first, behind the store's; counting decreasing ones
//   tokvec_maxsim_kernel      score[q][j] = (1 / nq) * sum_i max_r <vq[i], store[cand[q][j]][r]>
//   tokvec_scan_kernel        the same score of EVERY visible document for every query, document-stationary (mode 2 of
//   tokvec_scan_select_kernel rag_retrieve_maxsim_dev: the exhaustive search), and the exact top-pool of a query's scores
//
// tokvec_maxsim_kernel carries over m3_maxsim_kernel's fragment map and masking (m3_heads.hip): lane (fr = lane & 15, fq = lane >> 4)
// holds A[row fr][k = 8 fq ..+8] and B[col fr][the same k], acc[r] = C[row 4 fq + r][col fr]; A = 16 document rows, B = 16 query
// rows. One workgroup (4 waves) per (query, candidate slot); queries in blocks of 32 rows; wave w takes the document tile groups
// w, w + 4, ... Rows of a tile past the document are loaded from its last row and masked out of the maximum, never zero-filled.
// What differs: the document fragment is loaded as fp16 (16 B per lane and row, half of the float32 path) straight into the A
// operand and is exact there; only the float32 query is split, per K-step, into hi = fp16(x), lo = fp16(x - hi), and a product is
// two mfma_f32_16x16x32_f16: lo_q * d + hi_q * d with fp32 accumulation. hi * fp16 products are exact in fp32, the split costs
// 2^-22 relative, the accumulation over at most 1024 terms 1024 * 2^-24 = 6.1e-5: within 1e-4 of float64 MaxSim over the STORED
// vectors, and (fp16 rounding of unit rows moves a dot by at most 2^-11) within 1e-3 of float64 MaxSim over the original ones.
// A wave holds 4 document tiles against the 2 query tiles when the document has more than 8 tiles (a 255-row passage is 16: every
// wave reads the query block once), else 2, so that short documents still spread over the waves; which of the two runs is a
// function of the document's own row count, and either gives every accumulator the same MFMA sequence: the same bits.
// The loads of K-step k + 1 are requested before the MFMAs of step k. Per-wave maxima meet in LDS and one thread sums them in
// query order in float64: no atomics; a pair's score is a function of its own rows, bit-identical whatever surrounds it.
// A store is reserved in one of two forms (tokvec_reserve's `form`): the fp16 rows above, or RAG_TOKVEC_MXFP8 - E4M3 codes with one
// power-of-two scale per 32 components, 33/64 of the bytes ("the 8-bit form" below: tokvec_quant8_kernel beside the convert
// kernel, tv_doc<FORM> for the scoring kernel's document operand, both instantiations of tokvec_maxsim_kernel<FORM>). Every stored
// value of the 8-bit form is an fp16 value and is expanded to the same half8, so its scores are the fp16 form's bits over the
// fetched rows; the fp16 instantiation is the kernel as it was (62 SGPR, 104 VGPR, 40 AGPR, no scratch).
#include "common.h"

#include <algorithm>
#include <cmath>

#define TV_QT 2          // 16-row query tiles per block of queries

__global__ __launch_bounds__(256) void tokvec_convert_kernel(const float* __restrict__ in, half_t* __restrict__ out, int64_t n,
                                                              int* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const half_t v = (half_t)in[i];                            // round to nearest even
    if (!(fabsf((float)v) <= 65504.f)) atomicAdd(bad, 1);      // NaN, or inf once rounded: a float32 inf or |x| >= 65520
    out[i] = v;
}

// dst[i] = base + off[i + 1] - off[0] for i < n (dst = the store's offsets behind the documents it holds); off[i + 1] < off[i] counts
__global__ __launch_bounds__(256) void tokvec_offsets_kernel(const int64_t* __restrict__ off, int64_t n, int64_t base, int64_t* __restrict__ dst,
                                                              int* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (off[i + 1] < off[i]) atomicAdd(bad, 1);
    dst[i] = base + (off[i + 1] - off[0]);
}

// ---- the 8-bit form (RAG_TOKVEC_MXFP8; the contract is in include/rag_hip.h) --------------------------------------------------
// A stored row is tokvec_row_bytes bytes: dim E4M3 ("FN": max 448, no infinities) codes, then dim / 32 E8M0 scale bytes (e + 127, one
// per block of 32 consecutive components), then zero to 15 bytes that nobody reads, so that every row starts on a 16-byte boundary
// and a row is a whole number of the 16-byte units the compaction moves. value = code * 2^e, e in [-15, 7]: exact in fp16.
__host__ __device__ __forceinline__ int tokvec_row_bytes(int dim, int form) {
    return form == RAG_TOKVEC_MXFP8 ? (dim + dim / 32 + 15) & ~15 : dim * (int)sizeof(half_t);
}

// One thread per 8 consecutive floats, four neighbouring lanes per block of 32 (n is a multiple of 32 and a workgroup starts on a
// block, so the four are in or out together). `first` is the position of in[0], in floats, behind the first row at `out`.
// e = the smallest integer with amax <= 448 * 2^e = 1.75 * 2^(8 + e): floor(log2 amax) - 8, one more when the mantissa is above
// 1.75, clamped to [-15, 7] (zero and float32 subnormals land on -15). x * 2^-e is exact; its magnitude, cut at 448, is rounded to
// nearest even on the E4M3 grid in integer arithmetic on the float's bits (at or above 2^-6: 3 mantissa bits kept, the carry
// running into the exponent) or as a multiple of 2^-9 below (rintf; 8 * 2^-9 is the code of 2^-6). The sign bit is x's, zero included.
__global__ __launch_bounds__(256) void tokvec_quant8_kernel(const float* __restrict__ in, uint8_t* __restrict__ out, int64_t first, int64_t n,
                                                             int dim, int stride, int* __restrict__ bad) {
    const int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
    if (t >= n) return;
    float v[8];
    float amax = 0.f;
    int nbad = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        v[i] = in[t + i];
        if (!(fabsf((float)(half_t)v[i]) <= 65504.f)) ++nbad;   // what the fp16 form rejects: NaN, inf, |x| >= 65520
        amax = fmaxf(amax, fabsf(v[i]));
    }
    if (nbad) atomicAdd(bad, nbad);
    amax = fmaxf(amax, __shfl_xor(amax, 1));
    amax = fmaxf(amax, __shfl_xor(amax, 2));
    const unsigned ab = __float_as_uint(amax);
    int e = (int)(ab >> 23) - 127 - 8 + ((ab & 0x7fffffu) > 0x600000u ? 1 : 0);
    e = e < -15 ? -15 : e > 7 ? 7 : e;
    const float inv = __uint_as_float((unsigned)(127 - e) << 23);
    unsigned w[2] = {0u, 0u};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float y = v[i] * inv;
        const float a = fminf(fabsf(y), 448.f);
        unsigned code;
        if (a >= 0.015625f) {
            unsigned b = __float_as_uint(a);
            b += 0x7ffffu + ((b >> 20) & 1u);
            code = ((((b >> 23) - 120u) << 3) | ((b >> 20) & 7u)) & 0x7fu;
        } else {
            code = (unsigned)rintf(a * 512.f);
        }
        code |= (__float_as_uint(y) >> 24) & 0x80u;
        w[i >> 2] |= code << (8 * (i & 3));
    }
    const int64_t g = first + t, row = g / dim;
    const int col = (int)(g - row * dim);
    uint8_t* rp = out + row * stride;
    *reinterpret_cast<uint2*>(rp + col) = make_uint2(w[0], w[1]);
    if ((col & 31) == 0) rp[dim + (col >> 5)] = (uint8_t)(e + 127);
}

// The document operand of a lane - 8 consecutive k of one row - per form: where it lies, what a load brings, and the half8 the MFMA
// reads. fp16: 16 bytes per K-step, as stored. 8-bit: 8 code bytes and the block's scale byte (the four fq lanes of a row read the
// same one), expanded by v_cvt_scalef32_pk_f16_fp8 with the scale 2^e as a float; every stored value is an fp16 value, so the
// expansion is exact and the operand is the one the fp16 form holds for the fetched rows. The 8-bit form loads TWO K-steps at a
// time (tv_query_block_q8): 2 x 8 code bytes and the two scale bytes as one 16-bit load, so that a lane has as many passage bytes
// in flight as the fp16 form's 16-byte load - with one step in flight the 8-bit kernel was slower than the fp16 one.
template <int FORM> struct tv_doc;
template <> struct tv_doc<RAG_TOKVEC_FP16> {
    typedef half_t elem;
    typedef half8 raw;
    static __device__ __forceinline__ int64_t stride(int dim) { return dim; }                   // in elem
    static __device__ __forceinline__ raw load(const elem* __restrict__ p, int k, int dim, int fq) { return *reinterpret_cast<const half8*>(p + k); }
    static __device__ __forceinline__ half8 expand(const raw& r) { return r; }
};
typedef _Float16 tv_half2 __attribute__((ext_vector_type(2)));
struct tv_raw_q8 { uint2 c0, c1; unsigned s; };       // the codes of K-steps k and k + 32, their scale bytes in bits 0-7 and 8-15
template <> struct tv_doc<RAG_TOKVEC_MXFP8> {
    typedef uint8_t elem;
    typedef tv_raw_q8 raw;
    static __device__ __forceinline__ int64_t stride(int dim) { return tokvec_row_bytes(dim, RAG_TOKVEC_MXFP8); }
    // p = the row + 8 fq; k a multiple of 64, k1 the second step (clamped by the caller to the row). The 16-bit scale load is
    // aligned (dim and k / 32 are even) and inside the row: when the second scale byte is not one of the row's dim / 32, that
    // count is odd, dim + dim / 32 is odd, and the byte is the first of the padding to 16
    static __device__ __forceinline__ raw load(const elem* __restrict__ p, int k, int k1, int dim, int fq) {
        return {*reinterpret_cast<const uint2*>(p + k), *reinterpret_cast<const uint2*>(p + k1),
                (unsigned)*reinterpret_cast<const uint16_t*>(p + (dim - fq * 8 + (k >> 5)))};
    }
    static __device__ __forceinline__ half8 expand(const uint2& c, unsigned s) {
        const float sc = __uint_as_float(s << 23);              // E8M0 byte -> 2^(s - 127)
        const tv_half2 a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c.x, sc, false), b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c.x, sc, true);
        const tv_half2 e = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c.y, sc, false), d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c.y, sc, true);
        return (half8){a[0], a[1], b[0], b[1], e[0], e[1], d[0], d[1]};
    }
};

struct tv_raw8 { float4 a, b; };             // a lane's 8 consecutive floats of one query row
__device__ __forceinline__ tv_raw8 tv_load8(const float* __restrict__ p) {
    return {*reinterpret_cast<const float4*>(p), *reinterpret_cast<const float4*>(p + 4)};
}
__device__ __forceinline__ void tv_split8(const tv_raw8& r, half8& hi, half8& lo) {
    const float v[8] = {r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z, r.b.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        hi[i] = (half_t)v[i];
        lo[i] = (half_t)(v[i] - (float)hi[i]);
    }
}

// one block of TV_QT * 16 query rows against every document tile group of this wave, DT tiles at a time: best[j] = the maximum over
// the wave's document rows for query row 16 j + fr (in the lanes of every fq, before the cross-lane steps)
template <int DT, int FORM>
__device__ __forceinline__ void tv_query_block(const typename tv_doc<FORM>::elem* __restrict__ doc, int64_t nd, int64_t nd_tiles, const float* const (&qp)[TV_QT],
                                               int dim, int wv, int fr, int fq, float (&best)[TV_QT]) {
    for (int64_t dt0 = (int64_t)wv * DT; dt0 < nd_tiles; dt0 += 4 * DT) {
        typedef tv_doc<FORM> D;
        const typename D::elem* dp[DT];
#pragma unroll
        for (int t = 0; t < DT; ++t) dp[t] = doc + min((dt0 + t) * 16 + fr, nd - 1) * D::stride(dim) + fq * 8;
        f32x4 acc[DT][TV_QT];
#pragma unroll
        for (int t = 0; t < DT; ++t)
#pragma unroll
            for (int j = 0; j < TV_QT; ++j) acc[t][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        typename D::raw dr[DT];
        tv_raw8 qr[TV_QT];
#pragma unroll
        for (int t = 0; t < DT; ++t) dr[t] = D::load(dp[t], 0, dim, fq);
#pragma unroll
        for (int j = 0; j < TV_QT; ++j) qr[j] = tv_load8(qp[j]);
        for (int k = 0; k < dim; k += 32) {
            const int kn = k + 32 < dim ? k + 32 : k;          // the last step re-reads itself: no branch around the loads
            typename D::raw dn[DT];
            tv_raw8 qn[TV_QT];
#pragma unroll
            for (int t = 0; t < DT; ++t) dn[t] = D::load(dp[t], kn, dim, fq);
#pragma unroll
            for (int j = 0; j < TV_QT; ++j) qn[j] = tv_load8(qp[j] + kn);
            half8 bh[TV_QT], bl[TV_QT];
#pragma unroll
            for (int j = 0; j < TV_QT; ++j) tv_split8(qr[j], bh[j], bl[j]);
#pragma unroll
            for (int t = 0; t < DT; ++t) {
                const half8 da = D::expand(dr[t]);
#pragma unroll
                for (int j = 0; j < TV_QT; ++j) {
                    acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(da, bl[j], acc[t][j], 0, 0, 0);
                    acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(da, bh[j], acc[t][j], 0, 0, 0);
                }
            }
#pragma unroll
            for (int t = 0; t < DT; ++t) dr[t] = dn[t];
#pragma unroll
            for (int j = 0; j < TV_QT; ++j) qr[j] = qn[j];
        }
        // acc[t][j][r] = <document row (dt0 + t) * 16 + 4 fq + r, query row 16 j + fr>; rows past the document stay out of the maximum
#pragma unroll
        for (int t = 0; t < DT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if ((dt0 + t) * 16 + fq * 4 + r < nd) {
#pragma unroll
                    for (int j = 0; j < TV_QT; ++j) best[j] = fmaxf(best[j], acc[t][j][r]);
                }
    }
}

// The same for the 8-bit form, two K-steps per iteration. Every accumulator sees the MFMAs of tv_query_block in the same order -
// per step lo_q * d then hi_q * d, steps ascending - on the same operands: the same bits. The loads of the NEXT pair of steps (and
// the query rows of the step after the current one) are requested before the current step's MFMAs. A dim of an odd number of steps
// (32, 96, ...) ends on a half pair: its second step is skipped (uniform over the grid), its loads re-read the last step.
// Where the compiler puts the requests: it sinks the second step's query loads into that step's branch and waits there with
// vmcnt(0), which also waits for the next pair's passage bytes - so the passage loads get about one step to arrive, not two.
// Forms that pin the order (scheduling barriers; a loop over whole pairs without the branch; single steps with three register
// stages) were compiled and cost the third wave per SIMD (170 VGPR) or waited at the loop top for the youngest stage; none was
// measured faster, none is kept. DESIGN 4.5 "8-bit token vectors" has the times.
template <int DT>
__device__ __forceinline__ void tv_query_block_q8(const uint8_t* __restrict__ doc, int64_t nd, int64_t nd_tiles, const float* const (&qp)[TV_QT],
                                                  int dim, int wv, int fr, int fq, float (&best)[TV_QT]) {
    typedef tv_doc<RAG_TOKVEC_MXFP8> D;
    const int last = dim - 32;
    for (int64_t dt0 = (int64_t)wv * DT; dt0 < nd_tiles; dt0 += 4 * DT) {
        const uint8_t* dp[DT];
#pragma unroll
        for (int t = 0; t < DT; ++t) dp[t] = doc + min((dt0 + t) * 16 + fr, nd - 1) * D::stride(dim) + fq * 8;
        f32x4 acc[DT][TV_QT];
#pragma unroll
        for (int t = 0; t < DT; ++t)
#pragma unroll
            for (int j = 0; j < TV_QT; ++j) acc[t][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        D::raw dr[DT];
        tv_raw8 qr[TV_QT];
#pragma unroll
        for (int t = 0; t < DT; ++t) dr[t] = D::load(dp[t], 0, min(32, last), dim, fq);
#pragma unroll
        for (int j = 0; j < TV_QT; ++j) qr[j] = tv_load8(qp[j]);
        for (int k = 0; k < dim; k += 64) {
            const int k1 = min(k + 32, last);                  // this pair's second step
            const int kn = k + 64 < dim ? k + 64 : k;          // the next pair; the last one re-reads itself: no branch around the loads
            D::raw dn[DT];
            tv_raw8 q1[TV_QT], qn[TV_QT];
#pragma unroll
            for (int j = 0; j < TV_QT; ++j) q1[j] = tv_load8(qp[j] + k1);
#pragma unroll
            for (int t = 0; t < DT; ++t) dn[t] = D::load(dp[t], kn, min(kn + 32, last), dim, fq);
            half8 bh[TV_QT], bl[TV_QT];
#pragma unroll
            for (int j = 0; j < TV_QT; ++j) tv_split8(qr[j], bh[j], bl[j]);
#pragma unroll
            for (int t = 0; t < DT; ++t) {
                const half8 da = D::expand(dr[t].c0, dr[t].s & 0xffu);
#pragma unroll
                for (int j = 0; j < TV_QT; ++j) {
                    acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(da, bl[j], acc[t][j], 0, 0, 0);
                    acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(da, bh[j], acc[t][j], 0, 0, 0);
                }
            }
#pragma unroll
            for (int j = 0; j < TV_QT; ++j) qn[j] = tv_load8(qp[j] + kn);
            if (k + 32 < dim) {
#pragma unroll
                for (int j = 0; j < TV_QT; ++j) tv_split8(q1[j], bh[j], bl[j]);
#pragma unroll
                for (int t = 0; t < DT; ++t) {
                    const half8 da = D::expand(dr[t].c1, dr[t].s >> 8);
#pragma unroll
                    for (int j = 0; j < TV_QT; ++j) {
                        acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(da, bl[j], acc[t][j], 0, 0, 0);
                        acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(da, bh[j], acc[t][j], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < DT; ++t) dr[t] = dn[t];
#pragma unroll
            for (int j = 0; j < TV_QT; ++j) qr[j] = qn[j];
        }
#pragma unroll
        for (int t = 0; t < DT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if ((dt0 + t) * 16 + fq * 4 + r < nd) {
#pragma unroll
                    for (int j = 0; j < TV_QT; ++j) best[j] = fmaxf(best[j], acc[t][j][r]);
                }
    }
}

// grid = Q * pool workgroups. slot[q][j] = the row that was scored, or -1 for an empty slot (score 0.0): cand < 0, a row at or past
// the store's documents, a document without rows, a query without rows.
template <int FORM>
__global__ __launch_bounds__(256) void tokvec_maxsim_kernel(const float* __restrict__ q, const int64_t* __restrict__ q_off,
                                                             const typename tv_doc<FORM>::elem* __restrict__ store,
                                                             const int64_t* __restrict__ d_off, int64_t n_docs,
                                                             const int32_t* __restrict__ cand, int pool, int dim, float* __restrict__ out,
                                                             int32_t* __restrict__ slot) {
    __shared__ float wmax[4][TV_QT * 16];
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    const int qi = pair / pool, di = cand[pair];
    const int64_t q0 = q_off[qi], nq = q_off[qi + 1] - q0;
    int64_t d0 = 0, nd = 0;
    if (di >= 0 && di < n_docs) {
        d0 = d_off[di];
        nd = d_off[di + 1] - d0;
    }
    if (nq <= 0 || nd <= 0) {                                  // uniform over the workgroup
        if (tid == 0) {
            out[pair] = 0.f;
            slot[pair] = -1;
        }
        return;
    }
    const int64_t nd_tiles = (nd + 15) >> 4;
    const typename tv_doc<FORM>::elem* doc = store + d0 * tv_doc<FORM>::stride(dim);
    double total = 0.0;                                        // thread 0 alone
    for (int64_t qb = 0; qb < nq; qb += TV_QT * 16) {
        const float* qp[TV_QT];
        float best[TV_QT];
#pragma unroll
        for (int j = 0; j < TV_QT; ++j) {
            const int64_t row = min(qb + j * 16 + fr, nq - 1);
            qp[j] = q + (q0 + row) * dim + fq * 8;
            best[j] = -INFINITY;
        }
        if constexpr (FORM == RAG_TOKVEC_MXFP8) {
            if (nd_tiles > 8) tv_query_block_q8<4>(doc, nd, nd_tiles, qp, dim, wv, fr, fq, best);
            else tv_query_block_q8<2>(doc, nd, nd_tiles, qp, dim, wv, fr, fq, best);
        } else {
            if (nd_tiles > 8) tv_query_block<4, FORM>(doc, nd, nd_tiles, qp, dim, wv, fr, fq, best);
            else tv_query_block<2, FORM>(doc, nd, nd_tiles, qp, dim, wv, fr, fq, best);
        }
#pragma unroll
        for (int j = 0; j < TV_QT; ++j) {
            best[j] = fmaxf(best[j], __shfl_xor(best[j], 16));
            best[j] = fmaxf(best[j], __shfl_xor(best[j], 32));
            if (lane < 16) wmax[wv][j * 16 + lane] = best[j];
        }
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < TV_QT * 16 && qb + i < nq; ++i)
                total += (double)fmaxf(fmaxf(wmax[0][i], wmax[1][i]), fmaxf(wmax[2][i], wmax[3][i]));
        __syncthreads();
    }
    if (tid == 0) {
        out[pair] = (float)(total / (double)nq);
        slot[pair] = di;
    }
}

// ---- exhaustive MaxSim search (rag_retrieve_maxsim_dev, mode 2): every visible document against every query of the batch ------
// tokvec_scan_kernel is document-stationary: workgroup (d, g) owns document d and loops over the G queries of group g, so a stored
// row comes from HBM once per query group and from L1 / L2 for the group's other queries - not once per pair, as the rerank grid
// reads it. The host picks G so that a few hundred documents still give every CU several workgroups (tokvec_scan).
// The bits are the rerank kernel's, by three things that are the same here and there, whatever iterates around them:
//   1. a pair's float32 dot products come from tv_query_block / tv_query_block_q8, unchanged: document-relative 16-row tiles,
//      clamped row loads, one accumulator per (tile, query tile), K-steps ascending, per step lo_q * d then hi_q * d on
//      mfma_f32_16x16x32_f16 with the passage as the exact fp16 A operand; which of the two instantiations (2 or 4 tiles per
//      wave) runs is the same function of the document's own row count;
//   2. the maximum of a query row over the document's rows (lanes, then waves through LDS) is order-free;
//   3. one thread sums the maxima in query-row order in float64 and stores (float)(total / nq).
// What the kernel writes is the score's orderable key (f32_orderable: larger key = higher score), 0 = "not ranked": a pair whose
// document the query may not see (row_visible with the query's own tenant), a document without rows, a query without rows.
// Those tests are made once per workgroup, 256 pairs at a time, and leave the group's ranked queries as an ascending list in LDS:
// the loop below runs over that list alone, and a document nobody in the group may see ends there - a tenant's search pays the
// MFMA work of the tenant's documents only. Every workgroup walks the queries in the same order, so neighbours share them in L2. A real score never
// has key 0 (that is the NaN of all ones). Plane [Qb][n_docs], written whole by every launch: nothing of an earlier call is read.
#define TV_SCAN_G 1024     // most queries one workgroup of the scan loops over
template <int FORM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void tokvec_scan_kernel(const float* __restrict__ q, const int64_t* __restrict__ q_off,
                                                           const typename tv_doc<FORM>::elem* __restrict__ store,
                                                           const int64_t* __restrict__ d_off, int64_t n_docs, const int32_t* __restrict__ vis,
                                                           const int32_t* __restrict__ qten, int tenant, int q_first, int n_q, int G, int dim,
                                                           uint32_t* __restrict__ plane) {
    __shared__ float wmax[4][TV_QT * 16];
    __shared__ unsigned short qlist[TV_SCAN_G];                  // the group's ranked queries, ascending, relative to g0
    __shared__ int wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    const int64_t di = blockIdx.x;
    const int g0 = blockIdx.y * G, g1 = min(g0 + G, n_q);         // this workgroup's queries, relative to q_first; G <= TV_SCAN_G
    const int64_t d0 = d_off[di], nd = d_off[di + 1] - d0;
    int n_list = 0;
    for (int c0 = g0; c0 < g1; c0 += 256) {                      // 256 pairs at a time: unranked ones are written, ranked ones listed in order
        const int ql = c0 + tid;
        bool is_ranked = false;
        if (ql < g1) {
            const int qi = q_first + ql;
            is_ranked = nd > 0 && q_off[qi + 1] > q_off[qi] && row_visible(vis, di, tenant_of_query(qten, qi, tenant));
            if (!is_ranked) plane[(size_t)ql * n_docs + di] = 0u;
        }
        const unsigned long long m = __ballot(is_ranked);
        if (lane == 0) wcnt[wv] = __popcll(m);
        __syncthreads();
        int at = n_list;
        for (int w = 0; w < wv; ++w) at += wcnt[w];
        if (is_ranked) qlist[at + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)(ql - g0);
        n_list += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
    if (n_list == 0) return;                                     // a document no query of the group may see costs this much
    const int64_t nd_tiles = (nd + 15) >> 4;
    const typename tv_doc<FORM>::elem* doc = store + d0 * tv_doc<FORM>::stride(dim);
    for (int i = 0; i < n_list; ++i) {
        const int ql = g0 + qlist[i], qi = q_first + ql;
        const int64_t q0 = q_off[qi], nq = q_off[qi + 1] - q0;
        double total = 0.0;                                    // thread 0 alone
        for (int64_t qb = 0; qb < nq; qb += TV_QT * 16) {
            const float* qp[TV_QT];
            float best[TV_QT];
#pragma unroll
            for (int j = 0; j < TV_QT; ++j) {
                const int64_t row = min(qb + j * 16 + fr, nq - 1);
                qp[j] = q + (q0 + row) * dim + fq * 8;
                best[j] = -INFINITY;
            }
            if constexpr (FORM == RAG_TOKVEC_MXFP8) {
                if (nd_tiles > 8) tv_query_block_q8<4>(doc, nd, nd_tiles, qp, dim, wv, fr, fq, best);
                else tv_query_block_q8<2>(doc, nd, nd_tiles, qp, dim, wv, fr, fq, best);
            } else {
                if (nd_tiles > 8) tv_query_block<4, FORM>(doc, nd, nd_tiles, qp, dim, wv, fr, fq, best);
                else tv_query_block<2, FORM>(doc, nd, nd_tiles, qp, dim, wv, fr, fq, best);
            }
#pragma unroll
            for (int j = 0; j < TV_QT; ++j) {
                best[j] = fmaxf(best[j], __shfl_xor(best[j], 16));
                best[j] = fmaxf(best[j], __shfl_xor(best[j], 32));
                if (lane < 16) wmax[wv][j * 16 + lane] = best[j];
            }
            __syncthreads();
            if (tid == 0)
                for (int i = 0; i < TV_QT * 16 && qb + i < nq; ++i)
                    total += (double)fmaxf(fmaxf(wmax[0][i], wmax[1][i]), fmaxf(wmax[2][i], wmax[3][i]));
            __syncthreads();
        }
        if (tid == 0) plane[(size_t)ql * n_docs + di] = f32_orderable((float)(total / (double)nq));
    }
}

// The exact select: one workgroup per query of the sub-batch over its plane row -> the query's top-pool rows in rank order (score
// desc, row asc), -1 padded. A ranked pair's sort key is make_key's (score key << 32 | ~row): distinct for distinct rows, so the
// pool-th largest key T is one pair and "key >= T" is exactly the top-pool. T comes from a radix select, 8 bits per pass from the
// top, over the keys that still match the chosen prefix; it stops as soon as the pairs that match are exactly the ones still
// wanted (with distinct scores: after the 4 score passes at the latest). Unranked pairs have key 0, are never counted and never
// taken; with fewer ranked pairs than `pool` the first pass says so and all of them are taken. The at
// most 256 survivors are gathered in any order and placed by counting the keys above each: the order of the atomics shows nowhere.
__global__ __launch_bounds__(256) void tokvec_scan_select_kernel(const uint32_t* __restrict__ plane, int64_t n_docs, int pool,
                                                                  int32_t* __restrict__ rows_out) {
    __shared__ unsigned hist[256];
    __shared__ uint64_t top[RAG_MAX_K];
    __shared__ unsigned s_sel, s_need, s_cnt, n_top;
    const int tid = threadIdx.x;
    const uint32_t* row = plane + (size_t)blockIdx.x * n_docs;
    auto key_of = [&](int64_t d) -> uint64_t {
        const uint32_t s = row[d];
        return s ? ((uint64_t)s << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)d) : 0ull;
    };
    uint64_t prefix = 0, mask = 0;
    unsigned need = (unsigned)min((int64_t)pool, n_docs);        // after the first pass at least `need` ranked keys match the prefix
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[tid] = 0u;
        __syncthreads();
        // scores of one batch share their leading bits: a thread adds a run of equal digits once, or every lane of every wave
        // would queue for the same counter
        unsigned run = 0u, run_bin = 0u;
        for (int64_t d = tid; d < n_docs; d += 256) {
            const uint64_t key = key_of(d);
            if (key == 0ull || (key & mask) != prefix) continue;
            const unsigned bin = (unsigned)(key >> shift) & 255u;
            if (bin == run_bin) { ++run; continue; }
            if (run) atomicAdd(&hist[run_bin], run);
            run_bin = bin;
            run = 1u;
        }
        if (run) atomicAdd(&hist[run_bin], run);
        __syncthreads();
        if (tid == 0) {
            unsigned left = need;
            int b = 255;
            for (; b >= 0 && hist[b] < left; --b) left -= hist[b];
            s_sel = (unsigned)(b < 0 ? 256 : b);                 // 256: fewer ranked keys than wanted (the first pass alone can find that)
            s_need = left;
            s_cnt = b < 0 ? 0u : hist[b];
            n_top = 0u;
        }
        __syncthreads();
        const unsigned sel = s_sel;
        const bool all = sel == 256u || s_cnt == s_need;         // every ranked key under this prefix is wanted: T = the prefix, zeros below
        if (sel != 256u) prefix |= (uint64_t)sel << shift;
        mask |= (uint64_t)0xff << shift;
        need = s_need;
        __syncthreads();
        if (all) break;
    }
    const uint64_t thr = prefix > 1ull ? prefix : 1ull;
    for (int64_t d = tid; d < n_docs; d += 256) {
        const uint64_t key = key_of(d);
        if (key >= thr) {
            const unsigned at = atomicAdd(&n_top, 1u);
            if (at < (unsigned)pool) top[at] = key;              // never more than pool: the keys are distinct
        }
    }
    __syncthreads();
    const int n = (int)min(n_top, (unsigned)pool);
    if (tid < pool) {
        int32_t* out = rows_out + (size_t)blockIdx.x * pool;
        if (tid < n) {
            const uint64_t mine = top[tid];
            int rank = 0;
            for (int i = 0; i < n; ++i) rank += top[i] > mine;
            out[rank] = (int32_t)key_row(mine);
        } else {
            out[tid] = -1;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Host side
// ------------------------------------------------------------------------------------------------
static void tokvec_drop(rag_ctx* h) {
    h->tv.reset();
    h->tv8.reset();
    h->tv_off.reset();
    h->tv_docs = h->tv_rows = h->tv_docs_cap = h->tv_rows_cap = 0;
    h->tv_dim = 0;
    h->tv_form = RAG_TOKVEC_FP16;
    h->tv_stale = false;
}

int tokvec_reserve(rag_ctx* h, int64_t n_docs_total, int64_t rows_total, int dim, int form) {
    ARG_CHECK(h, form == RAG_TOKVEC_FP16 || form == RAG_TOKVEC_MXFP8, "tokvec_reserve: unknown form (RAG_TOKVEC_FP16, RAG_TOKVEC_MXFP8)");
    ARG_CHECK(h, n_docs_total > 0 && n_docs_total < (int64_t)0x7fffff00 && rows_total >= 0, "tokvec_reserve: need 0 < documents < 2^31 and rows >= 0");
    ARG_CHECK(h, dim >= 32 && dim <= 1024 && dim % 32 == 0, "tokvec_reserve: dim must be a multiple of 32 in [32, 1024]");
    tokvec_drop(h);
    int rc;
    rc = form == RAG_TOKVEC_MXFP8 ? h->tv8.alloc(h, std::max<size_t>((size_t)rows_total * tokvec_row_bytes(dim, form), 16))
                                  : h->tv.alloc(h, std::max<size_t>((size_t)rows_total * dim, 8));
    if (rc || (rc = h->tv_off.alloc(h, (size_t)n_docs_total + 1)) ||
        (rc = h->tv_bad.reserve(h, 2))) {
        tokvec_drop(h);
        return rc;
    }
    // cleared on the handle's stream and waited for: a null-stream hipMemset is not ordered against the non-blocking stream an
    // append may count on
    HIP_TRY(h, hipMemsetAsync(h->tv_bad, 0, 2 * sizeof(int), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->tv_off, 0, sizeof(int64_t), h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->tv_docs_cap = n_docs_total;
    h->tv_rows_cap = rows_total;
    h->tv_dim = dim;
    h->tv_form = form;
    return RAG_OK;
}

// One block, from device memory (queued on st, then waited for) or host memory (staged in pieces of at most 64 Mi floats).
// Nothing the store counts moves before the whole block is resident and checked; a rejected block leaves only slots past the
// counts written, which the next append overwrites.
int tokvec_append(rag_ctx* h, const float* vecs, const int64_t* row_off, int64_t n, hipStream_t st, bool host_ptrs) {
    ARG_CHECK(h, h->tv_docs_cap > 0, "tokvec_append: rag_tokvec_reserve first");
    ARG_CHECK(h, n >= 0 && h->tv_docs + n <= h->tv_docs_cap, "tokvec_append: exceeds the reserved documents");
    if (n == 0) return RAG_OK;
    ARG_CHECK(h, row_off != nullptr, "tokvec_append: null offsets");
    const int dim = h->tv_dim;
    int64_t ends[2] = {0, 0};
    if (host_ptrs) {
        ends[0] = row_off[0];
        ends[1] = row_off[n];
        for (int64_t i = 0; i < n; ++i) ARG_CHECK(h, row_off[i + 1] >= row_off[i], "tokvec_append: row offsets must never decrease");
    } else {
        HIP_TRY(h, hipMemcpyAsync(&ends[0], row_off, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipMemcpyAsync(&ends[1], row_off + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
    }
    const int64_t rows = ends[1] - ends[0];
    ARG_CHECK(h, ends[0] >= 0 && rows >= 0, "tokvec_append: row offsets must start at >= 0 and never decrease");
    ARG_CHECK(h, h->tv_rows + rows <= h->tv_rows_cap, "tokvec_append: exceeds the reserved rows");
    ARG_CHECK(h, rows == 0 || vecs != nullptr, "tokvec_append: null vectors");
    const bool q8 = h->tv_form == RAG_TOKVEC_MXFP8;
    const int stride = tokvec_row_bytes(dim, h->tv_form);
    half_t* dst = q8 ? nullptr : h->tv + (size_t)h->tv_rows * dim;
    uint8_t* dst8 = q8 ? h->tv8 + (size_t)h->tv_rows * stride : nullptr;
    int64_t* dst_off = h->tv_off + h->tv_docs + 1;
    const int64_t total = rows * dim;
    const int64_t piece = (int64_t)64 << 20;                     // floats per launch (a grid stays far below 2^32 threads) and per staged copy
    auto convert = [&](const float* src_dev, int64_t at, int64_t cnt) {
        for (int64_t o = 0; o < cnt; o += piece) {
            const int64_t nn = std::min(piece, cnt - o);
            if (q8)       // a piece is a multiple of 32 floats: no block of 32 is cut
                launch(tokvec_quant8_kernel, dim3((unsigned)((nn / 8 + 255) / 256)), dim3(256), 0, st, src_dev + o, dst8, at + o, nn, dim, stride,
                       h->tv_bad.get());
            else
                launch(tokvec_convert_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, src_dev + o, dst + at + o, nn, h->tv_bad.get());
        }
    };
    if (host_ptrs) {
        std::vector<int64_t> abs_off((size_t)n);
        for (int64_t i = 0; i < n; ++i) abs_off[(size_t)i] = h->tv_rows + (row_off[i + 1] - ends[0]);
        HIP_TRY(h, hipMemcpyAsync(dst_off, abs_off.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
        dev_buf<float> buf;
        if (total > 0)
            if (int rc = buf.alloc(h, (size_t)std::min(total, piece))) return rc;
        const float* src = vecs + (size_t)ends[0] * dim;
        for (int64_t o = 0; o < total; o += piece) {
            const int64_t nn = std::min(piece, total - o);
            HIP_TRY(h, hipMemcpyAsync(buf, src + o, (size_t)nn * sizeof(float), hipMemcpyHostToDevice, st));
            convert(buf, o, nn);
            HIP_TRY(h, hipStreamSynchronize(st));              // buf is reused by the next piece; abs_off is consumed
        }
        HIP_TRY(h, hipStreamSynchronize(st));
    } else {
        launch(tokvec_offsets_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, row_off, n, h->tv_rows, dst_off, h->tv_bad + 1);
        // a block whose inner offsets leave [off[0], off[n]] is a decreasing one and is rejected below; the rows converted are
        // the contiguous span between its ends either way, inside vecs by the caller's contract and inside the reservation
        if (total > 0) convert(vecs + (size_t)ends[0] * dim, 0, total);
    }
    HIP_TRY(h, hipGetLastError());
    int bad[2] = {0, 0};                                         // synchronous check: a load path, not a search path
    HIP_TRY(h, hipMemcpyAsync(bad, h->tv_bad, sizeof(bad), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    if (bad[0] != 0 || bad[1] != 0) {
        // the counters start again at zero, or every later - valid - append on this handle would be rejected with this one
        HIP_TRY(h, hipMemsetAsync(h->tv_bad, 0, sizeof(bad), st));
        HIP_TRY(h, hipStreamSynchronize(st));
    }
    ARG_CHECK(h, bad[1] == 0, "tokvec_append: row offsets must never decrease");
    ARG_CHECK(h, bad[0] == 0, "tokvec_append: the vectors hold a value that is not finite as fp16");
    h->tv_docs += n;
    h->tv_rows += rows;
    return RAG_OK;
}

int tokvec_load_host(rag_ctx* h, const float* vecs, const int64_t* off, int64_t n_docs, int dim, int form) {
    ARG_CHECK(h, off != nullptr && n_docs > 0, "tokvec_load: need offsets and at least one document");
    ARG_CHECK(h, off[n_docs] >= off[0], "tokvec_load: row offsets must never decrease");
    if (int rc = tokvec_reserve(h, n_docs, off[n_docs] - off[0], dim, form)) return rc;
    return tokvec_append(h, vecs, off, n_docs, h->stream, true);
}

int tokvec_info(const rag_ctx* h, int64_t* docs_out, int64_t* rows_out, int* dim_out, int64_t* hbm_bytes_out) {
    const bool have = h->tv_docs_cap > 0;
    if (docs_out) *docs_out = have ? h->tv_docs : 0;
    if (rows_out) *rows_out = have ? h->tv_rows : 0;
    if (dim_out) *dim_out = have ? h->tv_dim : 0;
    if (hbm_bytes_out) *hbm_bytes_out = have ? (int64_t)(h->tv.size() * sizeof(half_t) + h->tv8.size() + h->tv_off.size() * sizeof(int64_t)) : 0;
    return RAG_OK;
}

int tokvec_form(const rag_ctx* h, int* form_out) {
    if (form_out) *form_out = h->tv_docs_cap > 0 ? h->tv_form : -1;
    return RAG_OK;
}

int tokvec_fetch_host(rag_ctx* h, int64_t doc, float* out, int64_t cap_rows, int64_t* n_rows_out) {
    ARG_CHECK(h, h->tv_docs_cap > 0, "tokvec_fetch: no token-vector store");
    ARG_CHECK(h, doc >= 0 && doc < h->tv_docs && n_rows_out != nullptr && cap_rows >= 0, "tokvec_fetch: document out of range or null count");
    int64_t span[2];
    HIP_TRY(h, hipMemcpyAsync(span, h->tv_off + doc, sizeof(span), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const int64_t n = span[1] - span[0];
    *n_rows_out = n;
    ARG_CHECK(h, n <= cap_rows && (n == 0 || out != nullptr), "tokvec_fetch: the document has more rows than the output holds");
    if (n == 0) return RAG_OK;
    if (h->tv_form == RAG_TOKVEC_MXFP8) {                        // code * 2^e, decoded here from the stored bytes
        const int dim = h->tv_dim, stride = tokvec_row_bytes(dim, h->tv_form);
        std::vector<uint8_t> raw((size_t)n * stride);
        HIP_TRY(h, hipMemcpyAsync(raw.data(), h->tv8 + (size_t)span[0] * stride, raw.size(), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (int64_t r = 0; r < n; ++r) {
            const uint8_t* rp = raw.data() + (size_t)r * stride;
            for (int c = 0; c < dim; ++c) {
                const int code = rp[c], ex = (code >> 3) & 15, man = code & 7, e = (int)rp[dim + c / 32] - 127;
                const float mag = ex ? std::ldexp((float)(8 + man), ex - 10 + e) : std::ldexp((float)man, e - 9);
                out[(size_t)r * dim + c] = code & 0x80 ? -mag : mag;
            }
        }
        return RAG_OK;
    }
    std::vector<half_t> tmp((size_t)n * h->tv_dim);
    HIP_TRY(h, hipMemcpyAsync(tmp.data(), h->tv + (size_t)span[0] * h->tv_dim, tmp.size() * sizeof(half_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < tmp.size(); ++i) out[i] = (float)tmp[i];
    return RAG_OK;
}

// ---- the store through a compaction (rag_index_compact_live) --------------------------------------------------------------
// A document is a variable-length group of rows, so the planes' fixed-row gather does not serve. The map is PER DOCUMENT (8 B: the
// first old row of each surviving document, beside the new offsets), never per token row. One chunk of destination rows
// [r0, r0 + m) at a time: each lane moves 16 bytes (fp16 bits, never converted) of destination row R into the staging buffer; the
// row's document is the LAST d in [doc_lo, doc_hi] with new_off[d] <= R (documents without rows share their start with the next
// one: the last owns the row), a search over the chunk's own documents, and its source row is src_start[d] + (R - new_off[d]).
// The chunk is then copied to its destination. In place and safe: chunks ascend, every source row lies at or above its
// destination (rows only move down), so a chunk's sources lie at or above r0 - untouched by the earlier chunks, which wrote
// below r0 - and are all in the staging buffer before the copy overwrites [r0, r0 + m).
// A row is tokvec_row_bytes bytes in either form. The 8-bit form's scale bytes (dim / 32 of them, 1 to 32: not a whole number of
// units on their own) lie behind their row's codes and the row is padded to a multiple of 16 bytes, so codes and scales move
// together as stored bits in the same units; the argument above is about rows and holds unchanged, and chunk_rows is derived from
// the form's row bytes.
__global__ __launch_bounds__(256) void tokvec_compact_gather_kernel(const uint4* __restrict__ store, int units_per_row,
                                                                     const int64_t* __restrict__ new_off, const int64_t* __restrict__ src_start,
                                                                     int64_t doc_lo, int64_t doc_hi, int64_t r0, int64_t total,
                                                                     uint4* __restrict__ stage) {
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
        const int64_t row = u / units_per_row, c = u - row * units_per_row, R = r0 + row;
        int64_t lo = doc_lo, hi = doc_hi + 1;                  // new_off[doc_lo] <= r0 <= R
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (new_off[mid] <= R) lo = mid; else hi = mid;
        }
        const int64_t src = src_start[lo] + (R - new_off[lo]);
        stage[u] = store[src * units_per_row + c];
    }
}

// Plans the move from the compaction's row map (host copy, n_map = index rows before): documents [0, min(tv_docs, n_map)) go
// through the map, documents the store holds past the index rows keep their order behind the survivors. Allocates the new
// offsets and the per-document source map (RAG_ERR_NOMEM changes nothing); plan->active stays false when there is no usable
// store or no document of it is deleted.
int tokvec_compact_prepare(rag_ctx* h, const int64_t* row_map, int64_t n_map, size_t stage_bytes, tokvec_compact_plan* plan) {
    plan->active = false;
    if (h->tv_docs_cap <= 0 || h->tv_stale || h->tv_docs == 0) return RAG_OK;
    hipStream_t st = h->stream;
    const int64_t nd = h->tv_docs, nd_map = std::min(nd, n_map);
    std::vector<int64_t> off((size_t)nd + 1);
    HIP_TRY(h, hipMemcpyAsync(off.data(), h->tv_off, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    std::vector<int64_t> src_start;
    plan->new_off_h.assign(1, 0);
    plan->first_doc = -1;
    for (int64_t d = 0; d < nd; ++d) {
        if (d < nd_map && row_map[d] < 0) {
            if (plan->first_doc < 0) plan->first_doc = (int64_t)src_start.size();
            continue;
        }
        src_start.push_back(off[(size_t)d]);
        plan->new_off_h.push_back(plan->new_off_h.back() + (off[(size_t)d + 1] - off[(size_t)d]));
    }
    if (plan->first_doc < 0) return RAG_OK;
    plan->docs_new = (int64_t)src_start.size();
    plan->rows_new = plan->new_off_h.back();
    const int64_t row_bytes = tokvec_row_bytes(h->tv_dim, h->tv_form);
    plan->chunk_rows = h->opt.tokvec_compact_rows > 0 ? h->opt.tokvec_compact_rows : (int64_t)(stage_bytes / (size_t)row_bytes);
    plan->chunk_rows = std::max<int64_t>(1, std::min(plan->chunk_rows, (int64_t)(stage_bytes / (size_t)row_bytes)));
    if (plan->new_off.alloc(h, (size_t)h->tv_docs_cap + 1) || plan->src_start.alloc(h, std::max<size_t>(1, src_start.size()))) {
        (void)hipGetLastError();
        plan->new_off.reset();
        plan->src_start.reset();
        h->err = "compact_live: out of device memory for the token-vector store's new offsets";
        return RAG_ERR_NOMEM;
    }
    HIP_TRY(h, hipMemcpyAsync(plan->new_off, plan->new_off_h.data(), plan->new_off_h.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (!src_start.empty())
        HIP_TRY(h, hipMemcpyAsync(plan->src_start, src_start.data(), src_start.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipStreamSynchronize(st));                        // src_start is a local
    plan->active = true;
    return RAG_OK;
}

// Moves the rows through `stage` (at least chunk_rows rows), waits, then swaps the offsets in and shrinks the counts: the freed
// rows are headroom of the same reservation again.
int tokvec_compact_commit(rag_ctx* h, tokvec_compact_plan* plan, char* stage, hipStream_t st) {
    if (!plan->active) return RAG_OK;
    // 16-byte units per row: dim / 8 of fp16 bits; the 8-bit form's row - codes, its dim / 32 scale bytes and the padding that
    // makes them a whole number of units - moves as one piece, stored bits, never requantised
    const size_t row_bytes = (size_t)tokvec_row_bytes(h->tv_dim, h->tv_form);
    const int upr = (int)(row_bytes / 16);
    char* base = h->tv_form == RAG_TOKVEC_MXFP8 ? reinterpret_cast<char*>(h->tv8.get()) : reinterpret_cast<char*>(h->tv.get());
    const std::vector<int64_t>& no = plan->new_off_h;
    const auto doc_of = [&](int64_t r) { return (int64_t)(std::upper_bound(no.begin(), no.begin() + plan->docs_new + 1, r) - no.begin()) - 1; };
    for (int64_t r0 = no[(size_t)plan->first_doc]; r0 < plan->rows_new; r0 += plan->chunk_rows) {
        const int64_t m = std::min(plan->chunk_rows, plan->rows_new - r0), total = m * upr;
        const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, (int64_t)1 << 20);
        launch(tokvec_compact_gather_kernel, dim3(blocks), dim3(256), 0, st, reinterpret_cast<const uint4*>(base), upr,
               plan->new_off.get(), plan->src_start.get(), doc_of(r0), doc_of(r0 + m - 1), r0, total, reinterpret_cast<uint4*>(stage));
        HIP_TRY(h, hipMemcpyAsync(base + (size_t)r0 * row_bytes, stage, (size_t)m * row_bytes,
                                  hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(st));
    h->tv_off = std::move(plan->new_off);
    h->tv_docs = plan->docs_new;
    h->tv_rows = plan->rows_new;
    plan->active = false;
    return RAG_OK;
}

int tokvec_usable(rag_ctx* h, const char* who) {
    if (h->tv_docs_cap <= 0) {
        h->err = std::string(who) + ": no token-vector store (rag_tokvec_reserve / rag_tokvec_load_host)";
        return RAG_ERR_STATE;
    }
    if (h->tv_stale) {
        h->err = std::string(who) + ": the token-vector store is stale (a compaction renumbered the rows since it was filled): reload it";
        return RAG_ERR_STATE;
    }
    return RAG_OK;
}
int tokvec_covers_index(rag_ctx* h, const char* who) {
    if (h->tv_docs == h->n_rows) return RAG_OK;
    h->err = std::string(who) + ": the token-vector store does not hold exactly the index's rows (append the vectors of the inserted rows)";
    return RAG_ERR_STATE;
}

// the MaxSim launch alone over [Q][pool] slots (the caller has checked the store and the shape): *scores_out / *slots_out point into
// the handle's tv_ws - every slot's float32 score, and the row it was scored for or -1
int tokvec_score_slots(rag_ctx* h, const float* q_vecs, const int64_t* q_off, const int32_t* cand_rows, int Q, int pool, const float** scores_out,
                       const int32_t** slots_out, hipStream_t st) {
    const size_t P = (size_t)Q * pool;
    if (int rc = h->tv_ws.reserve(h, stage_size(P, 4) * 2)) return rc;
    float* sc = reinterpret_cast<float*>(h->tv_ws.get());
    int32_t* slot = reinterpret_cast<int32_t*>(h->tv_ws.get() + stage_size(P, 4));
    if (h->tv_form == RAG_TOKVEC_MXFP8)
        launch(tokvec_maxsim_kernel<RAG_TOKVEC_MXFP8>, dim3((unsigned)P), dim3(256), 0, st, q_vecs, q_off, h->tv8.get(), h->tv_off.get(), h->tv_docs,
               cand_rows, pool, h->tv_dim, sc, slot);
    else
        launch(tokvec_maxsim_kernel<RAG_TOKVEC_FP16>, dim3((unsigned)P), dim3(256), 0, st, q_vecs, q_off, h->tv.get(), h->tv_off.get(), h->tv_docs,
               cand_rows, pool, h->tv_dim, sc, slot);
    *scores_out = sc;
    if (slots_out) *slots_out = slot;
    return launch_status(h);
}

int tokvec_rerank(rag_ctx* h, const float* q_vecs, const int64_t* q_off, const int32_t* cand_rows, int Q, int pool, int k, int64_t* ids_out,
                  int32_t* rows_out, double* scores_out, float* pair_scores_out, hipStream_t st) {
    if (int rc = tokvec_usable(h, "tokvec_rerank")) return rc;
    ARG_CHECK(h, Q > 0 && pool > 0 && pool <= RAG_MAX_K && k > 0 && k <= pool, "tokvec_rerank: need n_queries > 0 and 0 < k <= pool <= 256");
    // one 256-thread workgroup per slot, and a launch holds fewer than 2^32 threads
    ARG_CHECK(h, (int64_t)Q * pool < ((int64_t)1 << 24), "tokvec_rerank: n_queries * pool must be below 2^24");
    ARG_CHECK(h, q_vecs && q_off && cand_rows && ids_out && scores_out, "tokvec_rerank: null argument");
    ARG_CHECK(h, (reinterpret_cast<uintptr_t>(q_vecs) & 15) == 0, "tokvec_rerank: query vectors must be 16-byte aligned");
    const size_t P = (size_t)Q * pool;
    const float* sc;
    const int32_t* slot;
    if (int rc = tokvec_score_slots(h, q_vecs, q_off, cand_rows, Q, pool, &sc, &slot, st)) return rc;
    if (pair_scores_out) HIP_TRY(h, hipMemcpyAsync(pair_scores_out, sc, P * sizeof(float), hipMemcpyDeviceToDevice, st));
    return tokvec_topk(h, sc, slot, Q, pool, k, ids_out, rows_out, scores_out, st);
}

// The exhaustive search's candidate stage: scan + select per sub-batch of Qb queries, Qb from the plane's bound (options
// tokvec_scan_ws_mb / tokvec_scan_queries). The plane is carved from the call's workspace by the caller; a sub-batch's select has
// read it before the next scan of the same stream writes it.
// Query groups: a workgroup loops over G queries of one document. With many documents G = Qb (a stored row leaves HBM once per
// sub-batch); with few, the queries are split so that documents x groups stays near 8 workgroups per CU.
int tokvec_scan_batch(const rag_ctx* h, int Q) {
    if (h->opt.tokvec_scan_queries > 0) return std::min(Q, h->opt.tokvec_scan_queries);
    const size_t cap = (size_t)(h->opt.tokvec_scan_ws_mb > 0 ? h->opt.tokvec_scan_ws_mb : 2048) << 20;
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)Q, cap / (4 * (size_t)std::max<int64_t>(h->tv_docs, 1))));
}

int tokvec_scan(rag_ctx* h, const float* q_vecs, const int64_t* q_off, int Q, int pool, int tenant, query_tenants qt, uint32_t* plane,
                int32_t* rows_out, hipStream_t st) {
    const int64_t n_docs = h->tv_docs;
    if (n_docs == 0) {                                           // an empty index: nothing to rank
        HIP_TRY(h, hipMemsetAsync(rows_out, 0xff, (size_t)Q * pool * sizeof(int32_t), st));
        return RAG_OK;
    }
    const int Qb = tokvec_scan_batch(h, Q);
    // per-query tenants: some query is filtered, so the table is needed as under a scalar filter
    const int32_t* vis = h->vis ? h->vis.get() : (tenant >= 0 || qt.dev != nullptr) ? h->tenants.get() : nullptr;
    const int64_t want = 8 * (int64_t)std::max(h->n_cu, 1);
    for (int q0 = 0; q0 < Q; q0 += Qb) {
        const int nb = std::min(Qb, Q - q0);
        const int groups = (int)std::min<int64_t>(nb, std::max<int64_t>(1, (want + n_docs - 1) / n_docs));
        const int G = std::min((nb + groups - 1) / groups, TV_SCAN_G);
        const dim3 grid((unsigned)n_docs, (unsigned)((nb + G - 1) / G));
        if (h->tv_form == RAG_TOKVEC_MXFP8)
            launch(tokvec_scan_kernel<RAG_TOKVEC_MXFP8>, grid, dim3(256), 0, st, q_vecs, q_off, h->tv8.get(), h->tv_off.get(), n_docs, vis, qt.dev,
                   tenant, q0, nb, G, h->tv_dim, plane);
        else
            launch(tokvec_scan_kernel<RAG_TOKVEC_FP16>, grid, dim3(256), 0, st, q_vecs, q_off, h->tv.get(), h->tv_off.get(), n_docs, vis, qt.dev,
                   tenant, q0, nb, G, h->tv_dim, plane);
        launch(tokvec_scan_select_kernel, dim3((unsigned)nb), dim3(256), 0, st, plane, n_docs, pool, rows_out + (size_t)q0 * pool);
    }
    return launch_status(h);
}

int tokvec_rerank_host(rag_ctx* h, const float* q_vecs, const int64_t* q_off, const int32_t* cand_rows, int Q, int pool, int k, int64_t* ids_out,
                       int32_t* rows_out, double* scores_out, float* pair_scores_out) {
    if (int rc = tokvec_usable(h, "tokvec_rerank")) return rc;
    ARG_CHECK(h, Q > 0 && pool > 0 && pool <= RAG_MAX_K && k > 0 && k <= pool, "tokvec_rerank: need n_queries > 0 and 0 < k <= pool <= 256");
    ARG_CHECK(h, q_off && cand_rows && ids_out && scores_out, "tokvec_rerank: null argument");
    ARG_CHECK(h, q_off[0] >= 0, "tokvec_rerank: query offsets must start at >= 0 and never decrease");
    for (int i = 0; i < Q; ++i) ARG_CHECK(h, q_off[i + 1] >= q_off[i], "tokvec_rerank: query offsets must start at >= 0 and never decrease");
    ARG_CHECK(h, q_vecs || q_off[Q] == 0, "tokvec_rerank: null query vectors");
    hipStream_t st = h->stream;
    const size_t P = (size_t)Q * pool, K = (size_t)Q * k, nqv = (size_t)q_off[Q] * h->tv_dim;
    dev_buf<float> dq, dps;
    dev_buf<int64_t> dqo, dids;
    dev_buf<int32_t> dcand, drows;
    dev_buf<double> dsc;
    int rc;
    if ((rc = dq.alloc(h, std::max<size_t>(nqv, 4))) || (rc = dqo.alloc(h, (size_t)Q + 1)) || (rc = dcand.alloc(h, P)) || (rc = dids.alloc(h, K)) ||
        (rc = drows.alloc(h, K)) || (rc = dsc.alloc(h, K)) || (rc = dps.alloc(h, P)))
        return rc;
    if (nqv) HIP_TRY(h, hipMemcpyAsync(dq, q_vecs, nqv * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(dqo, q_off, ((size_t)Q + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(dcand, cand_rows, P * sizeof(int32_t), hipMemcpyHostToDevice, st));
    rc = tokvec_rerank(h, dq, dqo, dcand, Q, pool, k, dids, drows, dsc, dps, st);
    if (!rc) {
        HIP_TRY(h, hipMemcpyAsync(ids_out, dids, K * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        if (rows_out) HIP_TRY(h, hipMemcpyAsync(rows_out, drows, K * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipMemcpyAsync(scores_out, dsc, K * sizeof(double), hipMemcpyDeviceToHost, st));
        if (pair_scores_out) HIP_TRY(h, hipMemcpyAsync(pair_scores_out, dps, P * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(h, hipStreamSynchronize(st));
    return rc;
}
